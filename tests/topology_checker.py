"""The contract of include/immesh_topology.h in numpy: np.unique on the edge keys with counts, a plain union-find loop for the components and
the boundary loops, the boxes and the selection as loops.  analyse(vtx, faces) -> dict with every output of the device calls; select(...) -> the mask
and the kept faces.  Soup generators for both tiers live here too."""
import numpy as np

EDGE_BOUNDARY, EDGE_NONMANIFOLD, EDGE_INCONSISTENT = 0, 1, 2
STAT_NAMES = ("n_faces", "n_counting", "n_degenerate", "n_vertices_used", "n_edges", "n_boundary", "n_interior", "n_nonmanifold", "n_inconsistent",
              "n_components", "largest_component_faces", "n_boundary_loops", "largest_loop_edges", "euler")


def _classes(n, pairs):
    """union-find over 0 .. n - 1 -> the smallest member of every element's class"""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b in pairs:
        a, b = find(int(a)), find(int(b))
        if a != b:
            parent[max(a, b)] = min(a, b)
    return np.array([find(x) for x in range(n)], np.int64)


def analyse(vtx, faces):
    vtx = np.asarray(vtx, np.float32).reshape(-1, 3)
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    nf = len(faces)
    F = faces.astype(np.int64)
    counting = (F[:, 0] != F[:, 1]) & (F[:, 1] != F[:, 2]) & (F[:, 0] != F[:, 2]) if nf else np.zeros(0, bool)
    cf = np.nonzero(counting)[0]
    a, b = F[cf][:, [0, 1, 2]].reshape(-1), F[cf][:, [1, 2, 0]].reshape(-1)          # half-edge 3 j + k of the j-th counting face
    key = (np.minimum(a, b) << 32) | np.maximum(a, b)
    forward = a < b
    face_of = np.repeat(cf, 3)
    uniq, inv, uses = np.unique(key, return_inverse=True, return_counts=True)
    order = np.argsort(key, kind="stable")
    start = np.concatenate([[0], np.cumsum(uses)])[:-1].astype(np.int64)
    # the components: every use of an edge joins its face to the edge's first face
    head_face = face_of[order[start]] if len(uniq) else np.zeros(0, np.int64)
    label_all = _classes(nf, zip(face_of, head_face[inv]))
    label = np.where(counting, label_all, -1)
    roots = np.unique(label[counting])
    number = {int(r): i for i, r in enumerate(roots)}
    comp = np.array([number[int(l)] if l >= 0 else -1 for l in label], np.int32)
    n_comp = len(roots)
    # the edges' classes
    boundary = uses == 1
    two = np.nonzero(uses == 2)[0]
    inconsistent = np.zeros(len(uniq), bool)
    inconsistent[two] = forward[order[start[two]]] == forward[order[start[two] + 1]]
    nonmanifold = uses >= 3
    uv = np.stack([uniq >> 32, uniq & 0xFFFFFFFF], axis=-1).astype(np.int32) if len(uniq) else np.zeros((0, 2), np.int32)
    edges = {kind: (uv[m], uses[m].astype(np.int32)) for kind, m in ((EDGE_BOUNDARY, boundary), (EDGE_NONMANIFOLD, nonmanifold), (EDGE_INCONSISTENT, inconsistent))}
    # the component tables
    first = roots.astype(np.int32)
    n_faces_c, n_bound_c = np.zeros(n_comp, np.int32), np.zeros(n_comp, np.int32)
    box = np.empty((n_comp, 6), np.float32)
    box[:, :3], box[:, 3:] = np.inf, -np.inf
    V, FL, CL, isfinite = vtx.astype(np.float64).tolist(), F.tolist(), comp.tolist(), np.isfinite(vtx).tolist()   # (a float as a double: exact)
    lo, hi = [[np.inf] * 3 for _ in range(n_comp)], [[-np.inf] * 3 for _ in range(n_comp)]
    for f in cf.tolist():
        c = CL[f]
        n_faces_c[c] += 1
        for v in FL[f]:
            for k in range(3):
                if isfinite[v][k]:
                    x = V[v][k]
                    if x < lo[c][k]:
                        lo[c][k] = x
                    if x > hi[c][k]:
                        hi[c][k] = x
    if n_comp:
        box[:, :3], box[:, 3:] = np.array(lo), np.array(hi)
    for e in np.nonzero(boundary)[0]:
        n_bound_c[comp[head_face[e]]] += 1
    # the boundary loops: the graph of the boundary edges
    bu = uv[boundary].astype(np.int64)
    n_loops, largest_loop = 0, 0
    if len(bu):
        ids, flat = np.unique(bu.reshape(-1), return_inverse=True)
        cls = _classes(len(ids), flat.reshape(-1, 2))
        per = np.bincount(cls[flat.reshape(-1, 2)[:, 0]], minlength=len(ids))
        n_loops, largest_loop = int((per > 0).sum()), int(per.max())
    used = len(np.unique(F[cf].reshape(-1)))
    st = {"n_faces": nf, "n_counting": len(cf), "n_degenerate": nf - len(cf), "n_vertices_used": used, "n_edges": len(uniq), "n_boundary": int(boundary.sum()),
          "n_interior": len(two), "n_nonmanifold": int(nonmanifold.sum()), "n_inconsistent": int(inconsistent.sum()), "n_components": n_comp,
          "largest_component_faces": int(n_faces_c.max()) if n_comp else 0, "n_boundary_loops": n_loops, "largest_loop_edges": largest_loop,
          "euler": used - len(uniq) + len(cf)}
    return {"stats": st, "comp": comp, "first_face": first, "n_faces": n_faces_c, "n_boundary": n_bound_c, "box": box, "edges": edges}


def select(res, faces, min_faces=0, min_diagonal=0.0, keep_largest=0):
    """the Select rule on analyse()'s result -> (keep (n_faces,) int8, the kept faces (n, 3) int32)"""
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    n_comp = len(res["first_face"])
    ranked = sorted(range(n_comp), key=lambda c: (-int(res["n_faces"][c]), int(res["first_face"][c])))
    top = set(ranked[:keep_largest]) if keep_largest > 0 else set(range(n_comp))
    keepc = np.zeros(n_comp, bool)
    for c in range(n_comp):
        ok = int(res["n_faces"][c]) >= min_faces and c in top
        if ok and min_diagonal > 0:
            lo, hi = res["box"][c, :3].astype(np.float64), res["box"][c, 3:].astype(np.float64)
            if not (np.isfinite(lo).all() and np.isfinite(hi).all()):
                ok = False
            else:
                d = hi - lo
                ok = bool((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2] >= np.float64(min_diagonal) * np.float64(min_diagonal))
        keepc[c] = ok
    comp = res["comp"]
    keep = np.array([1 if c >= 0 and keepc[c] else 0 for c in comp.tolist()], np.int8)
    return keep, faces[keep != 0]


# ---- soups ---------------------------------------------------------------------------------------------------------------------------------------
def grid_sheet(m, n, holes=(), z=0.0, scale=1.0, origin=(0.0, 0.0)):
    """an m x n grid of cells, two consistently wound faces each; holes: cells (i, j) left out -> vtx ((m + 1)(n + 1), 3), faces"""
    i, j = np.meshgrid(np.arange(m + 1), np.arange(n + 1), indexing="ij")
    vtx = np.stack([origin[0] + scale * i, origin[1] + scale * j, np.full(i.shape, z)], axis=-1).reshape(-1, 3).astype(np.float32)
    ci, cj = np.meshgrid(np.arange(m), np.arange(n), indexing="ij")
    ci, cj = ci.reshape(-1), cj.reshape(-1)
    if len(holes):
        gone = np.zeros((m, n), bool)
        gone[tuple(np.asarray(holes).T)] = True
        keep = ~gone[ci, cj]
        ci, cj = ci[keep], cj[keep]
    v00, v10, v01, v11 = ci * (n + 1) + cj, (ci + 1) * (n + 1) + cj, ci * (n + 1) + cj + 1, (ci + 1) * (n + 1) + cj + 1
    faces = np.stack([np.stack([v00, v10, v11], axis=-1), np.stack([v00, v11, v01], axis=-1)], axis=1).reshape(-1, 3).astype(np.int32)
    return vtx, faces


def torus(m, n):
    """an m x n grid of cells with both directions wrapped: closed, consistently wound"""
    i, j = np.meshgrid(np.arange(m), np.arange(n), indexing="ij")
    th, ph = 2 * np.pi * i / m, 2 * np.pi * j / n
    vtx = np.stack([(2 + np.cos(ph)) * np.cos(th), (2 + np.cos(ph)) * np.sin(th), np.sin(ph)], axis=-1).reshape(-1, 3).astype(np.float32)
    i, j = i.reshape(-1), j.reshape(-1)
    v = lambda a, b: (a % m) * n + (b % n)
    faces = np.stack([np.stack([v(i, j), v(i + 1, j), v(i + 1, j + 1)], axis=-1), np.stack([v(i, j), v(i + 1, j + 1), v(i, j + 1)], axis=-1)], axis=1)
    return vtx, faces.reshape(-1, 3).astype(np.int32)


def moebius(n):
    """a band of n cells whose last cell joins the first with a flip"""
    t = 2 * np.pi * np.arange(n) / n
    vtx = np.concatenate([np.stack([(1 + s * np.cos(t / 2)) * np.cos(t), (1 + s * np.cos(t / 2)) * np.sin(t), s * np.sin(t / 2)], axis=-1) for s in (-0.3, 0.3)])
    faces = []
    for i in range(n):
        a, b = i, n + i
        c, d = (i + 1, n + i + 1) if i + 1 < n else (n, 0)                                # the flip: top meets bottom
        faces += [[a, c, d], [a, d, b]]
    return vtx.astype(np.float32), np.array(faces, np.int32)


TETRA = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]], np.int32)                 # outward, consistent


def tetrahedron(offset=(0.0, 0.0, 0.0)):
    return (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32) + np.asarray(offset, np.float32)), TETRA.copy()


def strip(n):
    """n faces (i, i + 1, i + 2): one component, its labels must travel the whole length"""
    vtx = np.stack([np.arange(n + 2) * 0.5, np.arange(n + 2) % 2, np.zeros(n + 2)], axis=-1).astype(np.float32)
    i = np.arange(n)
    return vtx, np.stack([i, i + 1, i + 2], axis=-1).astype(np.int32)


def random_soup(rng, n_faces, n_vtx=12):
    """random index triples over a few vertices: degenerate and duplicate faces and long runs occur"""
    vtx = rng.uniform(-4, 4, (n_vtx, 3)).astype(np.float32)
    faces = rng.integers(0, n_vtx, (n_faces, 3)).astype(np.int32)
    return vtx, faces


def sheet_with_fragments(rng, m, n, n_holes, n_fragments):
    """a grid sheet with one-cell holes, plus fragments of one to four faces (strips) far from each other: the benchmark's and the scale test's soup"""
    cells = rng.choice((m - 2) * (n - 2), n_holes, replace=False)
    holes = np.stack([1 + cells // (n - 2), 1 + cells % (n - 2)], axis=-1)
    vtx, faces = grid_sheet(m, n, holes, scale=0.05)
    vs, fs, base = [vtx], [faces], len(vtx)
    for k in range(n_fragments):
        nf = 1 + k % 4
        v, f = strip(nf)
        vs.append((v * 0.05 + rng.uniform(-50, 50, 3)).astype(np.float32))
        fs.append(f + base)
        base += len(v)
    faces = np.concatenate(fs).astype(np.int32)
    return np.concatenate(vs).astype(np.float32), faces[rng.permutation(len(faces))]
