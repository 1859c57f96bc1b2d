"""The Holes rule of include/immesh_topology.h in numpy: np.unique on the edge keys, a dict of the boundary half-edges that leave and enter every
vertex, topology_checker._classes for the loops, a plain walk for the cycle, a Python set for the chord test.
holes(vtx, faces, max_edges, max_diagonal) -> dict with every output of the device calls.  The soups the other checkers lack live here too."""
import numpy as np

import topology_checker as tc

FILLED, NONSIMPLE, OUTLINE, TOO_LONG, TOO_WIDE, BLOCKED = 0, 1, 2, 3, 4, 5
STAT_NAMES = ("n_loops", "n_simple", "n_nonsimple", "n_outline", "n_too_long", "n_too_wide", "n_blocked", "n_filled", "n_new_faces", "n_edges_closed",
              "largest_simple_loop_edges", "n_cycle_vertices")
TABLES = (("first_vertex", np.int32), ("n_edges", np.int32), ("status", np.int32), ("box", np.float32), ("cycle_start", np.int64))


def holes(vtx, faces, max_edges, max_diagonal=0.0):
    vtx = np.asarray(vtx, np.float32).reshape(-1, 3)
    F = np.asarray(faces, np.int64).reshape(-1, 3)
    counting = (F[:, 0] != F[:, 1]) & (F[:, 1] != F[:, 2]) & (F[:, 0] != F[:, 2]) if len(F) else np.zeros(0, bool)
    cf = np.nonzero(counting)[0]
    tail, head = F[cf][:, [0, 1, 2]].reshape(-1), F[cf][:, [1, 2, 0]].reshape(-1)
    key = (np.minimum(tail, head) << 32) | np.maximum(tail, head)
    face_of = np.repeat(cf, 3)
    uniq, inv, uses = np.unique(key, return_inverse=True, return_counts=True)
    edge_set = set(uniq.tolist())
    bh = np.nonzero(uses[inv] == 1)[0]                                                  # the boundary half-edges
    leaving, entering = {}, {}
    for t, h, f in zip(tail[bh].tolist(), head[bh].tolist(), face_of[bh].tolist()):
        leaving.setdefault(t, []).append((h, f))
        entering.setdefault(h, []).append(t)
    verts = sorted(set(leaving) | set(entering))
    where = {v: i for i, v in enumerate(verts)}
    cls = tc._classes(len(verts), [(where[t], where[h]) for t, h in zip(tail[bh].tolist(), head[bh].tolist())])
    label_of = {v: verts[int(cls[i])] for i, v in enumerate(verts)}                    # (ascending ids: the smallest member is the smallest vertex)
    labels = sorted(set(label_of.values()))
    number = {l: i for i, l in enumerate(labels)}
    n_loops = len(labels)
    members = [[] for _ in range(n_loops)]
    for v in verts:
        members[number[label_of[v]]].append(v)
    n_edges = np.zeros(n_loops, np.int32)
    for t in tail[bh].tolist():
        n_edges[number[label_of[t]]] += 1
    box = np.empty((n_loops, 6), np.float32)
    status, cycle_start = np.zeros(n_loops, np.int32), np.full(n_loops, -1, np.int64)
    cycles, new_faces, new_loop = [], [], []
    finite = np.isfinite(vtx)
    md = np.float64(max_diagonal)
    for l, label in enumerate(labels):
        P, ok = vtx[members[l]], finite[members[l]]
        for k in range(3):
            x = P[ok[:, k], k]
            box[l, k], box[l, 3 + k] = (x.min(), x.max()) if len(x) else (np.inf, -np.inf)
        if not all(len(leaving.get(v, ())) == 1 and len(entering.get(v, ())) == 1 for v in members[l]):
            status[l] = NONSIMPLE
            continue
        n = int(n_edges[l])
        cyc = [label]
        while len(cyc) < n:
            cyc.append(leaving[cyc[-1]][0][0])
        assert leaving[cyc[-1]][0][0] == label and sorted(cyc) == members[l] and n >= 3
        cycle_start[l] = sum(len(c) for c in cycles)
        cycles.append(cyc)
        lo, hi = box[l, :3].astype(np.float64), box[l, 3:].astype(np.float64)
        with np.errstate(all="ignore"):
            d = hi - lo
            wide = md > 0 and (not (np.isfinite(lo).all() and np.isfinite(hi).all()) or bool((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2] > md * md))
        if len({leaving[v][0][1] for v in cyc}) == 1:
            status[l] = OUTLINE
        elif n > max_edges:
            status[l] = TOO_LONG
        elif wide:
            status[l] = TOO_WIDE
        elif any(((min(label, cyc[k]) << 32) | max(label, cyc[k])) in edge_set for k in range(2, n - 1)):
            status[l] = BLOCKED
        else:
            for k in range(1, n - 1):
                new_faces.append([label, cyc[k + 1], cyc[k]])
                new_loop.append(l)
    simple = status != NONSIMPLE
    filled = status == FILLED
    st = {"n_loops": n_loops, "n_simple": int(simple.sum()), "n_nonsimple": int((~simple).sum())}
    st.update({"n_" + name: int((status == code).sum()) for name, code in (("outline", OUTLINE), ("too_long", TOO_LONG), ("too_wide", TOO_WIDE),
                                                                           ("blocked", BLOCKED), ("filled", FILLED))})
    st.update({"n_new_faces": len(new_faces), "n_edges_closed": int(n_edges[filled].sum()),
               "largest_simple_loop_edges": int(n_edges[simple].max()) if simple.any() else 0, "n_cycle_vertices": int(n_edges[simple].sum())})
    return {"stats": {k: st[k] for k in STAT_NAMES}, "first_vertex": np.array(labels, np.int32), "n_edges": n_edges, "status": status, "box": box,
            "cycle_start": cycle_start, "cycle": np.array([v for c in cycles for v in c], np.int32),
            "new_faces": np.array(new_faces, np.int32).reshape(-1, 3), "new_loop": np.array(new_loop, np.int32)}


def closed(faces, res):
    """faces ++ new_faces"""
    return np.concatenate([np.asarray(faces, np.int32).reshape(-1, 3), res["new_faces"]]).astype(np.int32)


def check_invariant(vtx, faces, res, max_edges, max_diagonal=0.0):
    """the analysis of faces ++ new_faces against the analysis of the faces, the tables adding up, and a second pass that fills nothing filled before"""
    before, after = tc.analyse(vtx, faces)["stats"], tc.analyse(vtx, closed(faces, res))["stats"]
    st = res["stats"]
    k, E = st["n_filled"], st["n_edges_closed"]
    assert st["n_loops"] == before["n_boundary_loops"] == len(res["status"]) and st["n_new_faces"] == len(res["new_faces"]) == E - 2 * k
    assert after["n_boundary"] == before["n_boundary"] - E and after["n_boundary_loops"] == before["n_boundary_loops"] - k
    assert after["n_edges"] == before["n_edges"] + E - 3 * k and after["n_counting"] == before["n_counting"] + E - 2 * k and after["euler"] == before["euler"] + k
    assert all(after[n] == before[n] for n in ("n_nonmanifold", "n_inconsistent", "n_vertices_used")) and after["n_components"] <= before["n_components"]
    assert st["n_simple"] + st["n_nonsimple"] == st["n_loops"] and st["n_cycle_vertices"] == len(res["cycle"]) == int(res["n_edges"][res["status"] != NONSIMPLE].sum())
    assert st["n_outline"] + st["n_too_long"] + st["n_too_wide"] + st["n_blocked"] + st["n_filled"] == st["n_simple"]
    assert res["n_edges"].sum() == before["n_boundary"] and (st["largest_simple_loop_edges"] <= before["largest_loop_edges"])
    again = holes(vtx, closed(faces, res), max_edges, max_diagonal)
    gone = set(res["first_vertex"][res["status"] == FILLED].tolist())
    assert not gone & set(again["first_vertex"][again["status"] == FILLED].tolist())
    return again


# ---- soups ---------------------------------------------------------------------------------------------------------------------------------------
def cylinder(n, reverse=False):
    """a band of n cells around the z axis, consistently wound: two simple n-loops, labels 0 (the bottom ring 0 .. n - 1) and n (the top ring)"""
    t = 2 * np.pi * np.arange(n) / n
    ring = np.stack([np.cos(t), np.sin(t)], axis=-1)
    vtx = np.concatenate([np.concatenate([ring, np.zeros((n, 1))], axis=1), np.concatenate([ring, np.ones((n, 1))], axis=1)]).astype(np.float32)
    i = np.arange(n)
    j = (i + 1) % n
    faces = np.stack([np.stack([i, j, n + j], axis=-1), np.stack([i, n + j, n + i], axis=-1)], axis=1).reshape(-1, 3).astype(np.int32)
    return vtx, (faces[:, [0, 2, 1]].copy() if reverse else faces)


def relabel(rng, vtx, faces):
    """the soup with its vertex indices shuffled -> (vtx, faces, new index of every old vertex)"""
    perm = rng.permutation(len(vtx))                                                    # new index of old vertex v: perm[v]
    out = np.empty_like(vtx)
    out[perm] = vtx
    return out, perm[np.asarray(faces, np.int64)].astype(np.int32), perm


def open_pyramid():
    """a tetrahedron without its face (0, 2, 1): one 3-loop, not an outline"""
    vtx, faces = tc.tetrahedron()
    return vtx, faces[1:].copy()


def blocked_sheet():
    """a 3 x 3 sheet without its middle cell, and a closed tetrahedron standing on v_0 and v_2 of that 4-loop: the chord {v_0, v_2} is its edge"""
    vtx, faces = tc.grid_sheet(3, 3, holes=[(1, 1)])
    cyc = holes(vtx, faces, 4)["cycle"]                                                 # label 0's loop is the border; the hole's cycle comes second
    hole = cyc[-4:]
    a, b = int(hole[0]), int(hole[2])
    top = np.array([[1.4, 1.4, 1.0], [1.6, 1.6, 1.0]], np.float32)
    remap = np.array([a, b, len(vtx), len(vtx) + 1])
    return np.concatenate([vtx, top]), np.concatenate([faces, remap[tc.TETRA].astype(np.int32)])


def touching_holes():
    """a 4 x 4 sheet without the cells (1, 1) and (2, 2), which touch in one vertex"""
    return tc.grid_sheet(4, 4, holes=[(1, 1), (2, 2)])


def sheet_with_long_hole(rng, n_long=4097, n_small=300):
    """one soup with a loop of n_long edges beside n_small one-cell holes: a cylinder of n_long cells closed at the top by a centre vertex, and a sheet
    with the one-cell holes far from it"""
    cv, cfaces = cylinder(n_long)
    top = len(cv)
    i = np.arange(n_long)
    cap = np.stack([n_long + i, n_long + (i + 1) % n_long, np.full(n_long, top)], axis=-1).astype(np.int32)
    cv = np.concatenate([cv, [[0.0, 0.0, 1.0]]]).astype(np.float32)
    m = 64
    cells = rng.choice(((m - 2) // 2) ** 2, n_small, replace=False)                    # every second cell: no two holes touch
    side = (m - 2) // 2
    holes_at = np.stack([1 + 2 * (cells // side), 1 + 2 * (cells % side)], axis=-1)
    sv, sf = tc.grid_sheet(m, m, holes_at, scale=0.05, origin=(10.0, 10.0))
    faces = np.concatenate([cfaces, cap, sf + len(cv)]).astype(np.int32)
    return np.concatenate([cv, sv]).astype(np.float32), faces[rng.permutation(len(faces))]
