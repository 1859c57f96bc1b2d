"""Cloud normals and normal consistency (include/immesh_normals.h) on a synthetic sheet: 1 M points of the surface z = 0.3 sin(x) cos(0.7 y) over
40 m x 40 m, displaced by Gaussian noise of 5 mm, in random order, against a triangulated 400 x 400 grid of the same surface (318 402 faces), and
  normals_k8 .. k32      immesh_cloud_normals, k in {8, 16, 32}, max_dist 0.5 m, min_ratio 0.01: the one fused launch (no list is stored)
  knn_cloud_k8 .. k32    immesh_knn_cloud on the same cloud with the same k and max_dist and both lists stored on the device (12 bytes x k x n):
                         the only way to the same neighbourhoods without the fused kernel (the PCA would follow on the host); the comparison
  agree_cloud            immesh_normals_agree_cloud, max_dist 0.5 m (the walk to the closest face and the rule), next to
  closest_points         immesh_closest_points of the same cloud (its traversal kernel)
  agree_samples          immesh_normals_agree_samples over about 1 M samples of the mesh, next to
  nearest_samples        immesh_nearest_samples of the same samples (its traversal kernel)
  agree_reduce           immesh_normals_agree_reduce, 100 bins
All times are device times from HIP events (immesh_normals_last_timing, immesh_knn_last_timing, immesh_closest_last_timing,
immesh_nearest_last_timing); copies are outside.  Every case is measured once per round after one warm-up round; the medians over the rounds are
reported with the spread (min, max) across rounds.  One JSON object on stdout, and in --out when given.

    python tools/normals_bench.py [--rounds 7] [--side 1000] [--out profiles/normals_bench.json]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from immesh_amd import capi  # noqa: E402

KS = (8, 16, 32)
EXTENT = 40.0


def surface(x, y):
    return 0.3 * np.sin(x) * np.cos(0.7 * y)


def sheet_cloud(side, rng):
    g = (np.arange(side) + 0.5) * (EXTENT / side)
    x, y = (a.reshape(-1) for a in np.meshgrid(g, g, indexing="ij"))
    pts = np.stack([x, y, surface(x, y)], axis=1) + rng.normal(scale=0.005, size=(side * side, 3))
    return pts[rng.permutation(side * side)].astype(np.float32)


def sheet_mesh(side):
    g = np.arange(side) * (EXTENT / (side - 1))
    x, y = (a.reshape(-1) for a in np.meshgrid(g, g, indexing="ij"))
    vtx = np.stack([x, y, surface(x, y)], axis=1).astype(np.float32)
    i, j = (a.reshape(-1) for a in np.meshgrid(np.arange(side - 1), np.arange(side - 1), indexing="ij"))
    a, b, c, d = i * side + j, (i + 1) * side + j, (i + 1) * side + j + 1, i * side + j + 1
    return vtx, np.concatenate([np.stack([a, b, c], axis=1), np.stack([a, c, d], axis=1)]).astype(np.int32)


def summary(v):
    return {"median": round(float(np.median(v)), 4), "min": round(float(np.min(v)), 4), "max": round(float(np.max(v)), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7, help="repetitions of the whole set")
    ap.add_argument("--side", type=int, default=1000, help="the cloud has side x side points")
    ap.add_argument("--mesh-side", type=int, default=400)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    hip = capi.load_hip_library()
    h = capi.HotPath(hip, capi.avia_config(cap_root_voxels=1 << 12, cap_scan_points=200000, cap_vertices=1 << 18, cap_triangles=1 << 20), "immesh_")
    rng = np.random.default_rng(0)
    cloud = sheet_cloud(args.side, rng)
    vtx, faces = sheet_mesh(args.mesh_side)
    sizes = h.raycast_build_triangles(vtx, faces)
    n_cloud = h.cloud_index_build(cloud)
    n_samples = h.mesh_sample(len(cloud) / (EXTENT * EXTENT), 1, fetch=False)

    keys = tuple("normals_k%d" % k for k in KS) + tuple("knn_cloud_k%d" % k for k in KS) + ("agree_cloud", "closest_points", "agree_samples",
                                                                                              "nearest_samples", "agree_reduce")
    times = {k: [] for k in keys}
    info, digest = {}, {}
    for rnd in range(-1, args.rounds):                                          # round -1: the warm-up of every shape, not recorded
        rec = {}
        for k in KS:
            h.knn_cloud(k, 0.5, want=("count", "index", "d2"))
            rec["knn_cloud_k%d" % k] = h.knn_timing()[0]
            made = h.cloud_normals(k, 0.5, 0.01, want=("curvature",))
            rec["normals_k%d" % k] = h.normals_timing()[0]
            digest["normals_k%d" % k] = [made["with_normal"], made["too_few"], made["line_like"], made["not_finite"], float(made["curvature"].sum())]
        h.cloud_normals(16, 0.5, 0.01, want=())
        h.closest_points(cloud, 0.5, want=())
        rec["closest_points"] = h.closest_timing()[0]
        acc = h.normals_agree_cloud(0.5, fetch=False)
        rec["agree_cloud"] = h.normals_timing()[1]
        st_acc, _ = h.normals_agree_stats(0.01, 100)
        rec["agree_reduce"] = h.normals_timing()[2]
        h.nearest_samples(0.5, want=())
        rec["nearest_samples"] = h.nearest_timing()[1]
        com = h.normals_agree_samples(fetch=False)
        rec["agree_samples"] = h.normals_timing()[1]
        st_com, _ = h.normals_agree_stats(0.01, 100)
        if rnd >= 0:
            for k in keys:
                times[k].append(rec[k])
        info = {"cloud_points": n_cloud[0], "cloud_points_in_tree": n_cloud[1], "samples": n_samples, "accuracy": acc, "completeness": com,
                "normal_consistency_accuracy": st_acc.mean, "normal_consistency_completeness": st_com.mean}

    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short=12", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    except Exception:  # noqa: BLE001
        commit = None
    out = {"metric": "cloud normals and normal consistency on a synthetic sheet (immesh_cloud_normals, immesh_normals_agree_cloud, "
                     "immesh_normals_agree_samples, immesh_normals_agree_reduce) next to immesh_knn_cloud with both lists stored, immesh_closest_points "
                     "and immesh_nearest_samples", "unit": "ms", "parent_commit": commit,
           "mesh": {"vertices": sizes[0], "faces": sizes[1], "faces_in_tree": sizes[2]}, "rounds": args.rounds, "case": info, "digest": digest,
           "times": {k: summary(v) for k, v in times.items()},
           "timing": "device time from HIP events: the fused normals launch with the memset of its counts; immesh_knn_cloud's traversal kernel writing "
                     "both lists; each agreement launch with the memset of its counts; the traversal kernels of immesh_closest_points and "
                     "immesh_nearest_samples; the reduction; copies are outside; median, min and max over the rounds, each round measuring every case once"}
    h.close()
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as fp:
            json.dump(out, fp, indent=1)


if __name__ == "__main__":
    main()
