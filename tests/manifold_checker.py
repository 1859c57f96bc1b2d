"""The Manifold rule of include/immesh_topology.h in numpy and plain Python: a dict of the edges' users, a plain union-find over the corners, the fans
sorted by (vertex, label).  manifold(vtx, faces) -> dict with every output of the device calls.  The soups the other checkers lack live here too."""
import numpy as np

import topology_checker as tc

STAT_NAMES = ("n_corners", "n_fans", "n_vertices_used", "n_singular_vertices", "most_fans_at_vertex", "n_new_vertices", "n_corners_moved", "n_faces_changed",
              "n_closed_fans", "n_open_fans", "largest_fan_corners", "n_nonmanifold_before")
TABLES = ("vertex", "first_face", "n_corners", "n_links", "index_out")


def manifold(vtx, faces):
    vtx = np.ascontiguousarray(vtx, np.float32).reshape(-1, 3)
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    nv, nf = len(vtx), len(faces)
    F = faces.tolist()
    counting = [len({a, b, c}) == 3 for a, b, c in F]
    users = {}                                                                          # edge -> its uses as (face, k): the edge from corner k to k + 1
    for f in range(nf):
        if counting[f]:
            for k in range(3):
                a, b = F[f][k], F[f][(k + 1) % 3]
                users.setdefault((min(a, b), max(a, b)), []).append((f, k))
    links = []                                                                          # pairs of corners, one pair per end of a two-use edge
    for (u, w), us in users.items():
        if len(us) == 2:
            (f, k), (g, m) = us
            for v in (u, w):
                links.append((3 * f + F[f].index(v), 3 * g + F[g].index(v)))
    root = tc._classes(3 * nf, links).tolist()                                          # the smallest corner of every corner's class
    corners = [c for c in range(3 * nf) if counting[c // 3]]
    fans = sorted({(F[root[c] // 3][root[c] % 3], root[c]) for c in corners})           # (vertex, root corner): ascending (vertex, label)
    number = {r: j for j, (_, r) in enumerate(fans)}
    n_fans = len(fans)
    vertex = np.array([v for v, _ in fans], np.int32)
    first_face = np.array([r // 3 for _, r in fans], np.int32)
    n_corners, n_links = np.zeros(n_fans, np.int32), np.zeros(n_fans, np.int32)
    for c in corners:
        n_corners[number[root[c]]] += 1
    for a, _ in links:
        n_links[number[root[a]]] += 1
    index_out, vsrc = np.zeros(n_fans, np.int32), []
    n_fans_out = np.zeros(nv, np.int32)
    for j, (v, _) in enumerate(fans):
        if n_fans_out[v] == 0:
            index_out[j] = v
        else:
            index_out[j] = nv + len(vsrc)
            vsrc.append(v)
        n_fans_out[v] += 1
    vsrc = np.array(vsrc, np.int32)
    vtx_out = np.concatenate([vtx.view(np.uint32), vtx.view(np.uint32)[vsrc]]).view(np.float32)   # the bits, whatever they say
    faces_out, fan_out = faces.copy().reshape(-1), np.full(3 * nf, -1, np.int32)
    for c in corners:
        fan_out[c] = number[root[c]]
        faces_out[c] = index_out[fan_out[c]]
    faces_out = faces_out.reshape(-1, 3)
    moved = faces_out != faces
    used = int((n_fans_out > 0).sum())
    closed = int((n_links == n_corners).sum())
    st = {"n_corners": len(corners), "n_fans": n_fans, "n_vertices_used": used, "n_singular_vertices": int((n_fans_out >= 2).sum()),
          "most_fans_at_vertex": int(n_fans_out.max()) if nv else 0, "n_new_vertices": n_fans - used, "n_corners_moved": int(moved.sum()),
          "n_faces_changed": int(moved.any(axis=1).sum()), "n_closed_fans": closed, "n_open_fans": n_fans - closed,
          "largest_fan_corners": int(n_corners.max()) if n_fans else 0, "n_nonmanifold_before": sum(1 for us in users.values() if len(us) >= 3)}
    return {"stats": {k: st[k] for k in STAT_NAMES}, "n_fans_out": n_fans_out, "vertex": vertex, "first_face": first_face, "n_corners": n_corners,
            "n_links": n_links, "index_out": index_out, "fan_out": fan_out.reshape(-1, 3), "faces_out": faces_out, "vsrc": vsrc, "vtx_out": vtx_out,
            "xyz": vtx_out[nv:]}


def check_invariant(vtx, faces, res):
    """the Invariant of the rule through topology_checker.analyse, the tables adding up, and a second pass that moves nothing -> the second pass"""
    before, after = tc.analyse(vtx, faces)["stats"], tc.analyse(res["vtx_out"], res["faces_out"])["stats"]
    st = res["stats"]
    assert after["n_nonmanifold"] == 0 and after["n_counting"] == before["n_counting"] and after["n_degenerate"] == before["n_degenerate"]
    assert after["n_vertices_used"] == st["n_fans"] and after["n_boundary"] + 2 * after["n_interior"] == 3 * after["n_counting"]
    assert after["n_interior"] >= before["n_interior"] and after["n_components"] >= before["n_components"]
    assert st["n_nonmanifold_before"] == before["n_nonmanifold"] and st["n_vertices_used"] == before["n_vertices_used"]
    assert st["n_corners"] == 3 * before["n_counting"] == int(res["n_corners"].sum()) and st["n_closed_fans"] + st["n_open_fans"] == st["n_fans"]
    assert st["n_new_vertices"] == len(res["vsrc"]) == len(res["vtx_out"]) - len(np.asarray(vtx).reshape(-1, 3)) == st["n_fans"] - st["n_vertices_used"]
    assert int(res["n_links"].sum()) == 2 * before["n_interior"] and (res["n_links"] <= res["n_corners"]).all()
    again = manifold(res["vtx_out"], res["faces_out"])
    assert again["stats"]["n_new_vertices"] == 0 and np.array_equal(again["faces_out"], res["faces_out"]) and again["stats"]["n_singular_vertices"] == 0
    assert again["stats"]["n_fans"] == st["n_fans"] and again["stats"]["n_corners_moved"] == 0
    return again


# ---- soups ---------------------------------------------------------------------------------------------------------------------------------------
def _points(n, seed=0):
    return np.random.default_rng(seed).uniform(-2, 2, (n, 3)).astype(np.float32)


def faces_on_a_vertex(k):
    """k faces that share vertex 0 and nothing else: k fans at one vertex"""
    i = np.arange(k)
    return _points(2 * k + 1, k), np.stack([np.zeros(k, np.int64), 1 + 2 * i, 2 + 2 * i], axis=-1).astype(np.int32)


def disc(k, closed):
    """k faces round vertex 0, each sharing an edge with the next: one fan, open (k + 1 rim vertices) or closed (k rim vertices, k >= 3)"""
    i = np.arange(k)
    rim = k if closed else k + 1
    t = 2 * np.pi * np.arange(rim) / rim
    vtx = np.concatenate([[[0.0, 0.0, 0.0]], np.stack([np.cos(t), np.sin(t), np.zeros(rim)], axis=-1)]).astype(np.float32)
    return vtx, np.stack([np.zeros(k, np.int64), 1 + i, 1 + (i + 1) % rim], axis=-1).astype(np.int32)


def faces_on_an_edge(k):
    """k faces on the edge {0, 1}, each with an apex of its own: a book of k pages"""
    return _points(k + 2, k), np.stack([np.zeros(k, np.int64), np.ones(k, np.int64), 2 + np.arange(k)], axis=-1).astype(np.int32)


def two_tetrahedra(shared):
    """two closed tetrahedra that share their first `shared` vertices (1: a vertex, 2: an edge)"""
    v0, f0 = tc.tetrahedron()
    v1 = v0[shared:] + np.float32(3.0)
    remap = np.concatenate([np.arange(shared), 4 + np.arange(4 - shared)])
    return np.concatenate([v0, v1]).astype(np.float32), np.concatenate([f0, remap[f0].astype(np.int32)])


def fin_on_a_sheet():
    """a 3 x 3 sheet and one more face standing on the edge {5, 6} between two of its interior vertices"""
    vtx, faces = tc.grid_sheet(3, 3)
    return np.concatenate([vtx, [[1.0, 1.5, 1.0]]]).astype(np.float32), np.concatenate([faces, [[5, 6, 16]]]).astype(np.int32)


def pinched_sheet():
    """two 3 x 3 sheets without their middle cells that share one vertex, a corner of either hole (vertex 5 of both): the two holes' loops run through
    one vertex with two fans"""
    va, fa = tc.grid_sheet(3, 3, holes=[(1, 1)])
    vb, fb = tc.grid_sheet(3, 3, holes=[(1, 1)], origin=(0.0, 0.0), z=1.0)
    remap = np.where(np.arange(16) == 5, 5, 16 + np.arange(16) - (np.arange(16) > 5))
    return np.concatenate([va, np.delete(vb, 5, axis=0)]).astype(np.float32), np.concatenate([fa, remap[fb].astype(np.int32)])


def pillow():
    """two faces on the same three vertices, wound against each other: closed, every fan has two corners and two links"""
    return _points(3, 3), np.array([[0, 1, 2], [0, 2, 1]], np.int32)


def glued_soup(rng, n_pieces, m=4):
    """n_pieces m x m sheets; every piece after the first is glued to an earlier one on a vertex, on an edge, or not at all, and the faces shuffled:
    singular vertices, fins and non-manifold edges at scale"""
    vs, fs, base = [], [], 0
    for p in range(n_pieces):
        v, f = tc.grid_sheet(m, m, origin=(float(rng.uniform(-50, 50)), float(rng.uniform(-50, 50))), z=float(rng.uniform(-5, 5)))
        f = f.astype(np.int64) + base
        how = int(rng.integers(0, 3)) if p else 2
        if how < 2:                                                                     # this piece's vertex 0 (and 1) become vertices of an earlier piece
            q = int(rng.integers(0, p))
            a = q * len(v) + int(rng.integers(0, m)) * (m + 1) + int(rng.integers(0, m))
            f[f == base] = a
            if how == 1:
                f[f == base + 1] = a + 1                                                # an edge of the earlier piece's grid
        vs.append(v)
        fs.append(f)
        base += len(v)
    faces = np.concatenate(fs).astype(np.int32)
    return np.concatenate(vs).astype(np.float32), faces[rng.permutation(len(faces))]
