"""A reconstruction against a ground-truth cloud, both directions, through the C ABI (include/immesh_closest.h, include/immesh_nearest.h):
  accuracy      the ground-truth points to the mesh: immesh_closest_points + immesh_closest_reduce
  completeness  area-weighted samples of the mesh to the ground-truth cloud: immesh_mesh_sample, immesh_cloud_index_build, immesh_nearest_samples
                (the samples never leave the device) + immesh_nearest_reduce
  chamfer       the sum of the two mean distances
  precision, recall, F-score at tau: the share of samples / of ground-truth points nearer than tau, from the two histograms with bin_width = tau
                (bin 0 is dist < tau), over the points that are finite; 2 P R / (P + R)
Eight options look at the mesh itself first (include/immesh_simplify.h, include/immesh_topology.h, include/immesh_smooth.h,
include/immesh_intersect.h), all off by default:
  --weld | --simplify CELL [--simplify-mode first|mean] [--keep-duplicate-faces]
                            first of all, before the fragment filter: weld the vertices of equal coordinates (--weld: a soup that repeats its vertices
                            becomes a mesh whose faces share indices) or cluster them on a grid of CELL (--simplify: the decimation), drop the faces
                            that collapse and, unless --keep-duplicate-faces, the faces given twice (immesh_simplify), and give the caster the result
                            on the device (immesh_simplify_apply).  The output gains a `simplify` block: the arguments and the pass' counts
  --min-component-faces N   analyse the mesh, keep the components of at least N faces, rebuild the caster from the kept faces, then evaluate: the floating
                            fragments of noise and moving objects leave the figures
  --topology                the counts of the mesh that is evaluated (components, boundary edges and loops, non-manifold and inconsistent edges,
                            Euler characteristic) in the output
  --orient first|fewest|viewpoint [--viewpoint X Y Z]
                            after the fragment filter and before everything else: analyse the mesh, give every manifold patch one winding
                            (immesh_topology_orient), write it over the caster's faces on the device (immesh_topology_orient_apply).  The output gains
                            an `orientation` block with the orientation's counts and a `signed` block from the accuracy query's dist and side: the
                            shares of the ground-truth points in front of, behind and in the plane of their closest face, and the signed mean
  --fill-holes MAX_EDGES [--fill-max-diagonal D]
                            after the fragment filter and the orientation, before --topology: analyse the mesh, close every simple boundary loop of at
                            most MAX_EDGES edges (and, with D > 0, of a box diagonal of at most D) by a fan over its own vertices
                            (immesh_topology_holes), and give the caster the closed mesh on the device (immesh_topology_holes_apply).  The output gains
                            a `holes` block with the pass' counts.  Orient first: a border between faces wound against each other is not simple
  --smooth N_STEPS [--smooth-lambda L] [--smooth-mu M] [--smooth-border fixed|along|free]
                            after the weld, the fragment filter, the orientation and the fill, before --topology and the sampling: N_STEPS steps of
                            Taubin smoothing over the one-ring (immesh_smooth; L = 0.5 and M = -0.53 by default, M = L is plain Laplacian smoothing;
                            the border vertices stay, slide along the border or move freely), and the caster gets the moved vertices on the device
                            (immesh_smooth_apply).  The output gains a `smooth` block: the arguments and the pass' counts
  --remove-self-intersections [--max-candidates N]
                            right after --weld / --simplify and before the fragment filter: find the pairs of faces that pass through each other
                            (immesh_self_intersect) and take every face of such a pair out on the device (immesh_self_intersect_apply); the fragment
                            filter, the orientation and --fill-holes then see the holes it left.  The output gains an `intersections_removed` block:
                            the pass' counts and the faces that went.  Weld first: the neighbours of an unwelded soup touch and count
  --manifold                after --weld / --simplify and --remove-self-intersections, before the fragment filter, the orientation and --fill-holes:
                            give every fan of faces round a vertex a vertex of its own (immesh_topology_analyse, immesh_topology_manifold,
                            immesh_topology_manifold_apply, and an analysis of the result): pinched vertices and fins come apart, no edge keeps three
                            uses, and the holes that touched in a vertex become simple loops that --fill-holes can close.  The output gains a
                            `manifold` block: the pass' counts, and n_nonmanifold_after, n_components_after and n_boundary_loops_after
  --self-intersections [--max-candidates N]
                            the self-intersection counts of the mesh that is evaluated, after every other clean-up option, in an `intersections`
                            block.  N bounds the candidate pairs of either option (2^24 by default): a mesh with more is refused
One option looks at the cloud first (include/immesh_align.h), off by default:
  --align point|plane [--align-max-dist D] [--align-iters N]
                            after every option above and before anything else reads the cloud: refine the cloud's pose against the mesh that is
                            evaluated by iterated closest-face least squares (immesh_align) from the identity, linearised about the cloud's mean, with
                            point or point-to-plane rows, pairs within D (1.0), at most N iterations (30), and move the cloud by the pose found.  The
                            output gains an `align` block: the options, status, iterations, pose and the rms per iteration
Three options clean the cloud itself before that (include/immesh_nearest.h, the Outliers rule and the Clusters rule), off by default:
  --cloud-outliers-knn K MULT | --cloud-outliers-radius R MIN
                            first of all that reads the cloud, before --align: index the cloud, drop the points whose mean distance to their K
                            nearest neighbours within --max-dist exceeds mu + MULT sigma over the cloud (immesh_knn_cloud,
                            immesh_cloud_outliers_statistical) and / or the points with fewer than MIN others within R (immesh_radius_count_cloud,
                            immesh_cloud_outliers_radius), shrink the index on the device (immesh_cloud_index_apply_outliers) and fetch the kept
                            points (immesh_cloud_index_points), so that accuracy, alignment and completeness see one cloud.  The output gains a
                            `cloud_outliers` block: the arguments, mu, sigma, the threshold and the counts
  --cloud-clusters R MIN_NB [--cluster-min-points N] [--cluster-keep-largest N]
                            after the two outlier rules, on the same index: Euclidean clusters of the cloud (immesh_cloud_clusters: DBSCAN with
                            radius R, a core point has at least MIN_NB others within R; MIN_NB = 0 is plain cluster extraction), then only the
                            clusters of at least N points and / or the N largest stay (immesh_cloud_clusters_select) and the index shrinks as
                            above: a small detached object that both outlier rules keep leaves the figures.  The `cloud_outliers` block gains a
                            `clusters` entry: the arguments, the number of clusters and the counts
One option compares orientations as well (include/immesh_normals.h), off by default:
  --normals K [--normals-max-dist D] [--normals-min-ratio R] [--viewpoint X Y Z]
                            after the outlier options and --align, behind the distances: a normal per ground-truth point from its K nearest
                            neighbours within D (--max-dist by default; a neighbourhood whose middle eigenvalue is not above R times its largest
                            is line-like and gets none; with --viewpoint the normals face that point), then |cos| between that normal and the
                            mesh's face normal in both directions (immesh_cloud_normals, immesh_normals_agree_cloud, immesh_normals_agree_samples,
                            immesh_normals_agree_reduce).  The output gains normal_consistency_accuracy (every ground-truth point with its closest
                            face), normal_consistency_completeness (every sample with its nearest ground-truth point), normal_consistency (their
                            mean) and a `normals` block: the arguments, the normals' counts, the pairs and the opposed share of each direction
The mesh is a PLY written by immesh_save_ply (binary little-endian: float x y z; list uchar int vertex_indices), or the live mesh of a context:
evaluate(h, cloud, ...) takes any HotPath whose caster has been built (h.raycast_build_mesh() / h.raycast_build_triangles()).

    python tools/mesh_eval.py --cloud gt.npy --ply rec_mesh.ply [--tau 0.05] [--max-dist 1.0] [--density 400] [--seed 0] [--out eval.json]
                              [--min-component-faces N] [--topology] [--orient MODE [--viewpoint X Y Z]]
                              [--fill-holes MAX_EDGES [--fill-max-diagonal D]]
                              [--weld | --simplify CELL [--simplify-mode first|mean]] [--keep-duplicate-faces]
                              [--smooth N_STEPS [--smooth-lambda L] [--smooth-mu M] [--smooth-border fixed|along|free]]
                              [--remove-self-intersections] [--self-intersections] [--max-candidates N] [--manifold]
                              [--align point|plane [--align-max-dist D] [--align-iters N]]
                              [--cloud-outliers-knn K MULT] [--cloud-outliers-radius R MIN]
                              [--cloud-clusters R MIN_NB [--cluster-min-points N] [--cluster-keep-largest N]]
                              [--normals K [--normals-max-dist D] [--normals-min-ratio R]]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from immesh_amd import capi  # noqa: E402


def read_ply(path):
    """the layout immesh_save_ply writes -> vtx (n, 3) float32, faces (m, 3) int32"""
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    if b"format binary_little_endian 1.0" not in head or b"property list uchar int vertex_indices" not in head:
        raise ValueError(f"{path}: not the binary little-endian layout of immesh_save_ply")
    lines = head.split(b"\n")
    nv = int([l for l in lines if l.startswith(b"element vertex")][0].split()[-1])
    nf = int([l for l in lines if l.startswith(b"element face")][0].split()[-1])
    vtx = np.frombuffer(body[:nv * 12], np.float32).reshape(-1, 3).copy()
    rec = np.frombuffer(body[nv * 12:nv * 12 + nf * 13], np.uint8).reshape(nf, 13)
    if nf and not np.all(rec[:, 0] == 3):
        raise ValueError(f"{path}: a face that is not a triangle")
    return vtx, rec[:, 1:].copy().view(np.int32).reshape(nf, 3)


def _side(st, hist):
    finite = st.n_points - st.n_not_finite
    return {"points": st.n_points, "finite": finite, "within_max_dist": st.n_with_face, "mean": st.mean, "rms": st.rms, "max": st.max_dist,
            "within_tau": int(hist[0]), "share_within_tau": (int(hist[0]) / finite) if finite else 0.0}


def _signed(dist, side):
    """the accuracy query by the side of the closest face -> dict; the shares are over the points with a face within max_dist"""
    has = dist >= 0
    n = int(has.sum())
    front, behind, in_plane = (int((side[has] == k).sum()) for k in (1, -1, 0))
    mean = float((dist[has].astype(np.float64) * side[has]).sum() / n) if n else 0.0
    return {"points_with_face": n, "front": front, "behind": behind, "in_plane": in_plane, "share_front": front / n if n else 0.0,
            "share_behind": behind / n if n else 0.0, "share_in_plane": in_plane / n if n else 0.0, "signed_mean": mean}


def normal_consistency(h, max_dist, k, normals_max_dist=None, min_ratio=0.0, viewpoint=None):
    """h: a HotPath whose index holds the ground-truth cloud and whose last nearest_samples query read the caster's current samples (evaluate leaves
    both so) -> dict: the three consistencies and the `normals` block.  A direction without a pair has consistency 0"""
    nd = max_dist if normals_max_dist is None else normals_max_dist
    made = h.cloud_normals(k, nd, min_ratio, capi.NORMALS_CANONICAL if viewpoint is None else capi.NORMALS_VIEWPOINT, viewpoint, want=())
    block = {"k": k, "max_dist": nd, "min_ratio": min_ratio, "viewpoint": None if viewpoint is None else [float(x) for x in viewpoint], **made}
    means = {}
    for name in ("completeness", "accuracy"):                                   # each reduced before the other replaces it
        counts = h.normals_agree_samples(fetch=False) if name == "completeness" else h.normals_agree_cloud(max_dist, fetch=False)
        st, _ = h.normals_agree_stats(1.0, 1)
        means[name] = st.mean
        block[name] = {**counts, "opposed_share": counts["opposed"] / counts["pairs"] if counts["pairs"] else 0.0}
    return {"normal_consistency_accuracy": means["accuracy"], "normal_consistency_completeness": means["completeness"],
            "normal_consistency": 0.5 * (means["accuracy"] + means["completeness"]), "normals": block}


def evaluate(h, cloud, tau=0.05, max_dist=1.0, density=400.0, seed=0, signed=False, normals=None):
    """h: a HotPath with a built caster; cloud (n, 3) float32 ground truth -> dict; signed: add the `signed` block (it means something once the mesh
    has been oriented); normals: the keyword arguments of normal_consistency (k, normals_max_dist, min_ratio, viewpoint) to add its figures"""
    cloud = np.ascontiguousarray(cloud, dtype=np.float32).reshape(-1, 3)
    got = h.closest_points(cloud, max_dist, want=("dist", "side") if signed else ())
    extra = {"signed": _signed(got["dist"], got["side"])} if signed else {}
    acc = _side(*h.closest_stats(tau, 1))
    n_samples = h.mesh_sample(density, seed, fetch=False)
    n_cloud, n_in = h.cloud_index_build(cloud)
    h.nearest_samples(max_dist, want=())
    com = _side(*h.nearest_stats(tau, 1))
    p, r = com["share_within_tau"], acc["share_within_tau"]
    if normals is not None:
        extra.update(normal_consistency(h, max_dist, **normals))
    return {"tau": tau, "max_dist": max_dist, "density": density, "seed": seed, "samples": n_samples, "cloud_points": n_cloud, "cloud_points_indexed": n_in,
            "accuracy": acc, "completeness": com, "chamfer": acc["mean"] + com["mean"], "precision": p, "recall": r,
            "f_score": (2.0 * p * r / (p + r)) if p + r > 0 else 0.0, **extra}


def drop_fragments(h, vtx, faces, min_component_faces):
    """h: a HotPath whose caster is built over (vtx, faces) -> the caster rebuilt over the components of at least min_component_faces faces;
    returns (its sizes, what was dropped)"""
    st = h.topology_analyse()
    _, kept = h.topology_select(min_faces=min_component_faces)
    return h.raycast_build_triangles(vtx, kept), {"min_component_faces": min_component_faces, "faces_before": len(faces), "faces_kept": len(kept),
                                                  "components_before": st.n_components}


ORIENT_MODES = {"first": capi.ORIENT_FIRST, "fewest": capi.ORIENT_FEWEST, "viewpoint": capi.ORIENT_VIEWPOINT}


def orient(h, mode, viewpoint=None):
    """h: a HotPath with a built caster -> its faces oriented on the device (analyse, orient, apply); returns the orientation's counts"""
    h.topology_analyse()
    st = h.topology_orient(ORIENT_MODES[mode], viewpoint if mode == "viewpoint" else None)
    h.topology_orient_apply()
    out = {"mode": mode, **{n: getattr(st, n) for n, _ in capi.OrientStats._fields_}}
    if mode == "viewpoint":
        out["viewpoint"] = [float(x) for x in viewpoint]
    return out


def fill_holes(h, max_edges, max_diagonal=0.0):
    """h: a HotPath with a built caster -> its small holes closed on the device (analyse, holes, apply); returns (the caster's sizes, the counts)"""
    h.topology_analyse()
    st = h.topology_holes(max_edges, max_diagonal)
    h.topology_holes_apply()
    return h._raycast_sizes(), {"max_edges": max_edges, "max_diagonal": max_diagonal, **{n: getattr(st, n) for n, _ in capi.HolesStats._fields_}}


def manifold(h, vtx):
    """h: a HotPath whose caster is built over the vertices vtx -> every fan of faces gets a vertex of its own on the device (analyse, manifold, apply, analyse again);
    returns (the caster's sizes, the new vertices and faces as the later steps need them on the host, the counts)"""
    h.topology_analyse()
    st = h.topology_manifold()
    vtx = np.concatenate([np.asarray(vtx, np.float32).reshape(-1, 3), h.topology_manifold_new_vertices()[1]])
    faces = h.topology_manifold_faces()[1]
    h.topology_manifold_apply()
    after = h.topology_analyse()
    return h._raycast_sizes(), vtx, faces, {**{n: getattr(st, n) for n, _ in capi.ManifoldStats._fields_}, "n_nonmanifold_after": after.n_nonmanifold,
                                            "n_components_after": after.n_components, "n_boundary_loops_after": after.n_boundary_loops}


SIMPLIFY_MODES = {"first": capi.SIMPLIFY_FIRST, "mean": capi.SIMPLIFY_MEAN}


def simplify(h, cell, mode="first", merge_duplicates=True):
    """h: a HotPath with a built caster -> its snapshot welded (cell == 0) or clustered on a grid of `cell` on the device (simplify, apply); returns
    (the caster's sizes, the new vertices and faces as the later steps need them on the host, the arguments and the counts)"""
    st = h.simplify(cell, SIMPLIFY_MODES[mode], merge_duplicates)
    vtx, faces = h.simplify_vertices()["vtx"], h.simplify_faces()
    h.simplify_apply()
    return h._raycast_sizes(), vtx, faces, {"cell": cell, "mode": mode, "merge_duplicates": bool(merge_duplicates),
                                            **{n: getattr(st, n) for n, _ in capi.SimplifyStats._fields_}}


SMOOTH_BORDERS = {"fixed": capi.SMOOTH_BORDER_FIXED, "along": capi.SMOOTH_BORDER_ALONG, "free": capi.SMOOTH_BORDER_FREE}


def smooth(h, n_steps, lam=0.5, mu=-0.53, border="fixed"):
    """h: a HotPath with a built caster -> its vertices smoothed on the device (smooth, apply); returns the arguments and the counts"""
    st = h.smooth(n_steps, lam, mu, SMOOTH_BORDERS[border])
    h.smooth_apply()
    return {"lambda": lam, "mu": mu, "border": border, **{n: getattr(st, n) for n, _ in capi.SmoothStats._fields_}}


def _intersect_stats(st):
    return {n: (list(st.n_share) if n == "n_share" else getattr(st, n)) for n, _ in capi.IntersectStats._fields_}


def self_intersections(h, max_candidates=1 << 24):
    """the self-intersection counts of the built caster's mesh -> dict"""
    return {"max_candidates": max_candidates, **_intersect_stats(h.self_intersect(max_candidates))}


def remove_self_intersections(h, faces, max_candidates=1 << 24):
    """h: a HotPath with a built caster over `faces` -> the faces of every intersecting pair taken out on the device (self_intersect, apply); returns
    (the caster's sizes, the kept faces as the later steps need them on the host, the counts and what went)"""
    st = h.self_intersect(max_candidates)
    kept = faces[h.self_intersect_faces()["face_map"] >= 0]
    h.self_intersect_apply()
    return h._raycast_sizes(), kept, {"max_candidates": max_candidates, **_intersect_stats(st), "faces_before": len(faces), "faces_removed": len(faces) - len(kept)}


def topology(h):
    """the counts of the built caster's mesh -> dict"""
    st = h.topology_analyse()
    return {n: getattr(st, n) for n, _ in capi.TopologyStats._fields_}


ALIGN_MODES = {"point": capi.ALIGN_POINT, "plane": capi.ALIGN_PLANE}


def align_cloud(h, cloud, mode, max_dist=1.0, max_iters=30):
    """h: a HotPath with a built caster -> (the cloud moved by the pose that the alignment finds from the identity, linearised about the cloud's mean;
    the options, status, iterations, pose and the rms per iteration)"""
    cloud = np.ascontiguousarray(cloud, dtype=np.float32).reshape(-1, 3)
    centre = capi.align_centre_mean(cloud)
    res, hist = h.align(cloud, capi.align_options(mode=ALIGN_MODES[mode], max_dist=max_dist, centre=centre, max_iters=max_iters))
    rot, pos = np.array(list(res.frame.rot)).reshape(3, 3), np.array(list(res.frame.pos))
    moved = (cloud.astype(np.float64) @ rot.T + pos).astype(np.float32)
    return moved, {"mode": mode, "max_dist": max_dist, "max_iters": max_iters, "centre": centre, "status": capi.ALIGN_STATUS[res.status],
                   "iterations": res.iterations, "rot": rot.reshape(-1).tolist(), "pos": pos.tolist(), "points_used": [int(v) for v in hist[:, 0]],
                   "rms": hist[:, 1].tolist()}


def filter_cloud(h, cloud, knn=None, radius=None, max_dist=1.0, clusters=None, cluster_min_points=0, cluster_keep_largest=0):
    """the stray points of a ground-truth cloud taken out on the device, statistical rule first when both are given: knn = (K, MULT) keeps the points
    whose mean distance to their K nearest neighbours (within max_dist) is at most mu + MULT sigma; radius = (R, MIN) keeps the points with at least
    MIN others within R; clusters = (R, MIN_NB), after the two: DBSCAN with radius R and MIN_NB neighbours for a core point, and only the clusters of
    at least cluster_min_points points and (cluster_keep_largest > 0) among that many largest stay; noise goes
    -> (the kept points as the index holds them, the rules' arguments and counts)"""
    cloud = np.ascontiguousarray(cloud, dtype=np.float32).reshape(-1, 3)
    out = {"points_before": len(cloud)}
    h.cloud_index_build(cloud)
    if knn is not None:
        k, mult = int(knn[0]), float(knn[1])
        h.knn_cloud(k, max_dist, want=())
        st = h.cloud_outliers_statistical(mult)
        h.cloud_index_apply_outliers()
        out["knn"] = {"k": k, "mult": mult, "max_dist": max_dist, **{n: v for n, v in st.items() if n != "keep"}}
    if radius is not None:
        r, min_neighbours = float(radius[0]), int(radius[1])
        h.radius_count_cloud(r)
        st = h.cloud_outliers_radius(min_neighbours)
        h.cloud_index_apply_outliers()
        out["radius"] = {"radius": r, "min_neighbours": min_neighbours, **{n: v for n, v in st.items() if n != "keep"}}
    if clusters is not None:
        r, min_neighbours = float(clusters[0]), int(clusters[1])
        found = h.cloud_clusters(r, min_neighbours, want=())
        st = h.cloud_clusters_select(min_points=int(cluster_min_points), keep_largest=int(cluster_keep_largest))
        h.cloud_index_apply_outliers()
        out["clusters"] = {"radius": r, "min_neighbours": min_neighbours, "min_points": int(cluster_min_points), "keep_largest": int(cluster_keep_largest),
                           "n_clusters": found["n_clusters"], **found["counts"], **{n: v for n, v in st.items() if n not in ("keep", "not_finite")}}
    kept = h.cloud_index_points()                       # the accuracy half runs on the same cloud as the completeness half
    out["points_kept"] = len(kept)
    return kept, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cloud", required=True, help="ground-truth points, .npy of shape (n, 3) or (n, >= 3)")
    ap.add_argument("--ply", required=True, help="a mesh written by immesh_save_ply")
    ap.add_argument("--tau", type=float, default=0.05)
    ap.add_argument("--max-dist", type=float, default=1.0, help="pairs farther apart count as unmatched (they leave the means, not the shares)")
    ap.add_argument("--density", type=float, default=400.0, help="samples per unit area of the mesh")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default="")
    ap.add_argument("--min-component-faces", type=int, default=0, help="drop the components with fewer faces before evaluating (0: keep everything)")
    ap.add_argument("--topology", action="store_true", help="add the evaluated mesh's topology counts to the output")
    ap.add_argument("--orient", choices=sorted(ORIENT_MODES), default=None, help="orient every manifold patch consistently before evaluating")
    ap.add_argument("--viewpoint", type=float, nargs=3, default=None, metavar=("X", "Y", "Z"), help="with --orient viewpoint: the point the faces should face")
    ap.add_argument("--fill-holes", type=int, default=0, metavar="MAX_EDGES", help="close the simple boundary loops of at most MAX_EDGES edges before evaluating (0: off)")
    ap.add_argument("--fill-max-diagonal", type=float, default=0.0, metavar="D", help="with --fill-holes: leave the loops whose box diagonal exceeds D (0: any)")
    ap.add_argument("--weld", action="store_true", help="weld the vertices of equal coordinates first of all (--simplify 0)")
    ap.add_argument("--simplify", type=float, default=None, metavar="CELL", help="cluster the vertices on a grid of CELL first of all (0: the weld)")
    ap.add_argument("--simplify-mode", choices=sorted(SIMPLIFY_MODES), default="first", help="with --simplify: a cluster's position, its first vertex or the mean")
    ap.add_argument("--keep-duplicate-faces", action="store_true", help="with --weld / --simplify: keep the faces given twice")
    ap.add_argument("--smooth", type=int, default=None, metavar="N_STEPS", help="smooth the vertices over their one-rings before sampling")
    ap.add_argument("--smooth-lambda", type=float, default=None, metavar="L", help="with --smooth: the factor of the even steps (0.5)")
    ap.add_argument("--smooth-mu", type=float, default=None, metavar="M", help="with --smooth: the factor of the odd steps (-0.53; M = L: Laplacian smoothing)")
    ap.add_argument("--smooth-border", choices=sorted(SMOOTH_BORDERS), default=None, help="with --smooth: what a border vertex does (fixed)")
    ap.add_argument("--remove-self-intersections", action="store_true", help="take the faces that pass through each other out, right after --weld / --simplify")
    ap.add_argument("--self-intersections", action="store_true", help="add the evaluated mesh's self-intersection counts to the output")
    ap.add_argument("--max-candidates", type=int, default=None, metavar="N", help="with either of the two: refuse a mesh with more candidate pairs (2^24)")
    ap.add_argument("--manifold", action="store_true", help="split every pinched vertex and fin: a vertex per fan of faces, before the orientation and --fill-holes")
    ap.add_argument("--align", choices=sorted(ALIGN_MODES), default=None, help="refine the cloud's pose against the evaluated mesh first (ICP with point or plane rows)")
    ap.add_argument("--align-max-dist", type=float, default=None, metavar="D", help="with --align: pairs farther apart do not take part (1.0)")
    ap.add_argument("--align-iters", type=int, default=None, metavar="N", help="with --align: at most N iterations (30)")
    ap.add_argument("--cloud-outliers-knn", type=float, nargs=2, default=None, metavar=("K", "MULT"),
                    help="drop the cloud points whose mean distance to their K nearest neighbours exceeds mu + MULT sigma, before everything that reads the cloud")
    ap.add_argument("--cloud-outliers-radius", type=float, nargs=2, default=None, metavar=("R", "MIN"),
                    help="drop the cloud points with fewer than MIN others within R, before everything that reads the cloud")
    ap.add_argument("--cloud-clusters", type=float, nargs=2, default=None, metavar=("R", "MIN_NB"),
                    help="cluster the cloud (DBSCAN: radius R, a core point has MIN_NB others within R) after the outlier rules and keep the clusters chosen below")
    ap.add_argument("--cluster-min-points", type=int, default=None, metavar="N", help="with --cloud-clusters: drop the clusters of fewer than N points (0)")
    ap.add_argument("--cluster-keep-largest", type=int, default=None, metavar="N", help="with --cloud-clusters: keep the N clusters with the most points only (0: all)")
    ap.add_argument("--normals", type=int, default=None, metavar="K", help="add the normal consistency: cloud normals from the K nearest neighbours (2 .. 64)")
    ap.add_argument("--normals-max-dist", type=float, default=None, metavar="D", help="with --normals: neighbours within D (--max-dist)")
    ap.add_argument("--normals-min-ratio", type=float, default=None, metavar="R", help="with --normals: no normal where the middle eigenvalue is not above R times the largest (0)")
    args = ap.parse_args()
    if args.normals is None and (args.normals_max_dist is not None or args.normals_min_ratio is not None):
        ap.error("--normals-max-dist and --normals-min-ratio go with --normals K")
    if args.normals is not None and not 2 <= args.normals <= 64:
        ap.error("--normals K: K is an integer in 2 .. 64")
    if args.cloud_outliers_knn is not None and not (args.cloud_outliers_knn[0] == int(args.cloud_outliers_knn[0]) and 1 <= args.cloud_outliers_knn[0] <= 64):
        ap.error("--cloud-outliers-knn K MULT: K is an integer in 1 .. 64")
    if args.cloud_outliers_radius is not None and not (args.cloud_outliers_radius[1] == int(args.cloud_outliers_radius[1]) and args.cloud_outliers_radius[1] >= 0):
        ap.error("--cloud-outliers-radius R MIN: MIN is an integer, not negative")
    if args.cloud_clusters is not None and not (args.cloud_clusters[1] == int(args.cloud_clusters[1]) and args.cloud_clusters[1] >= 0):
        ap.error("--cloud-clusters R MIN_NB: MIN_NB is an integer, not negative")
    if args.cloud_clusters is None and (args.cluster_min_points is not None or args.cluster_keep_largest is not None):
        ap.error("--cluster-min-points and --cluster-keep-largest go with --cloud-clusters R MIN_NB")
    if (args.cluster_min_points or 0) < 0 or (args.cluster_keep_largest or 0) < 0:
        ap.error("--cluster-min-points N, --cluster-keep-largest N: not negative")
    if args.align is None and (args.align_max_dist is not None or args.align_iters is not None):
        ap.error("--align-max-dist and --align-iters go with --align {point,plane}")
    if args.max_candidates is not None and not (args.remove_self_intersections or args.self_intersections):
        ap.error("--max-candidates N goes with --remove-self-intersections or --self-intersections")
    max_candidates = (1 << 24) if args.max_candidates is None else args.max_candidates
    if args.smooth is None and (args.smooth_lambda is not None or args.smooth_mu is not None or args.smooth_border is not None):
        ap.error("--smooth-lambda, --smooth-mu and --smooth-border go with --smooth N_STEPS")
    if args.smooth is not None and args.smooth < 0:
        ap.error("--smooth N_STEPS: not negative")
    if args.weld and args.simplify is not None:
        ap.error("--weld is --simplify 0: give one of them")
    if (args.keep_duplicate_faces or args.simplify_mode != "first") and not args.weld and args.simplify is None:
        ap.error("--simplify-mode and --keep-duplicate-faces go with --weld or --simplify CELL")
    if args.fill_max_diagonal and not args.fill_holes:
        ap.error("--fill-max-diagonal D goes with --fill-holes")
    if (args.orient == "viewpoint" and args.viewpoint is None) or (args.viewpoint is not None and args.orient != "viewpoint" and args.normals is None):
        ap.error("--viewpoint X Y Z goes with --orient viewpoint or --normals K, and only with them")
    cloud = np.load(args.cloud)[:, :3]
    vtx, faces = read_ply(args.ply)
    h = capi.HotPath(capi.load_hip_library(), capi.avia_config(cap_root_voxels=1 << 12, cap_scan_points=200000, cap_vertices=1 << 18, cap_triangles=1 << 20), "immesh_")
    try:
        sizes = h.raycast_build_triangles(vtx, faces)
        extra = {}
        if args.weld or args.simplify is not None:
            sizes, vtx, faces, extra["simplify"] = simplify(h, 0.0 if args.weld else args.simplify, args.simplify_mode, not args.keep_duplicate_faces)
        if args.remove_self_intersections:
            sizes, faces, extra["intersections_removed"] = remove_self_intersections(h, faces, max_candidates)
        if args.manifold:
            sizes, vtx, faces, extra["manifold"] = manifold(h, vtx)
        if args.min_component_faces > 0:
            sizes, extra["filter"] = drop_fragments(h, vtx, faces, args.min_component_faces)
        if args.orient:
            extra["orientation"] = orient(h, args.orient, args.viewpoint)
        if args.fill_holes:
            sizes, extra["holes"] = fill_holes(h, args.fill_holes, args.fill_max_diagonal)
        if args.smooth is not None:
            extra["smooth"] = smooth(h, args.smooth, 0.5 if args.smooth_lambda is None else args.smooth_lambda, -0.53 if args.smooth_mu is None else args.smooth_mu,
                                     args.smooth_border or "fixed")
        if args.topology:
            extra["topology"] = topology(h)
        if args.self_intersections:
            extra["intersections"] = self_intersections(h, max_candidates)
        if args.cloud_outliers_knn is not None or args.cloud_outliers_radius is not None or args.cloud_clusters is not None:   # the strays leave before the alignment weighs them
            cloud, extra["cloud_outliers"] = filter_cloud(h, cloud, args.cloud_outliers_knn, args.cloud_outliers_radius, args.max_dist, clusters=args.cloud_clusters,
                                                          cluster_min_points=args.cluster_min_points or 0, cluster_keep_largest=args.cluster_keep_largest or 0)
        if args.align:                                    # the cloud is moved before anything else reads it
            cloud, extra["align"] = align_cloud(h, cloud, args.align, 1.0 if args.align_max_dist is None else args.align_max_dist,
                                                30 if args.align_iters is None else args.align_iters)
        normals = None if args.normals is None else dict(k=args.normals, normals_max_dist=args.normals_max_dist, min_ratio=args.normals_min_ratio or 0.0,
                                                         viewpoint=args.viewpoint)
        out = dict(evaluate(h, cloud, args.tau, args.max_dist, args.density, args.seed, signed=bool(args.orient), normals=normals), mesh={"vertices": sizes[0], "faces": sizes[1], "faces_in_tree": sizes[2]},
                   **extra)
    finally:
        h.close()
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as fp:
            json.dump(out, fp, indent=1)


if __name__ == "__main__":
    main()
