"""The contract of include/immesh_simplify.h restated twice.  simplify() is the numpy restatement: np.unique on the cluster keys, a loop over the
member rank k = 0 .. largest - 1 that adds the k-th member of every cluster (the ascending sequential sum), a dict for the duplicates.  brute() is
plain Python for tiny inputs and shares nothing with it: every pair of vertices compared, Python floats, struct for the float rounding."""
import math
import struct

import numpy as np

STAT_NAMES = ("n_vertices_in", "n_vertices_used", "n_alone_not_finite", "n_alone_outside", "n_vertices_out", "largest_cluster", "n_faces_in",
              "n_not_counting", "n_collapsed", "n_duplicate", "n_faces_out")
FIRST, MEAN = 0, 1
KEPT, NOT_COUNTING, COLLAPSED, DUPLICATE = 0, 1, 2, 3
ARRAYS = (("vtx_out", np.float32), ("first_vertex", np.int32), ("n_members", np.int32), ("vmap", np.int32), ("fmap", np.int32), ("fstatus", np.int8),
          ("faces_out", np.int32))
Q_LIMIT = float(2 ** 20)


def simplify(vtx, faces, cell=0.0, mode=FIRST, merge_duplicates=True):
    vtx = np.ascontiguousarray(vtx, np.float32).reshape(-1, 3)
    faces = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    assert cell >= 0.0 and math.isfinite(cell) and mode in (FIRST, MEAN)
    nv, nf = len(vtx), len(faces)
    counting = (faces[:, 0] != faces[:, 1]) & (faces[:, 1] != faces[:, 2]) & (faces[:, 0] != faces[:, 2])
    used = np.zeros(nv, bool)
    used[faces[counting].reshape(-1)] = True
    finite = np.isfinite(vtx).all(axis=1)
    if cell > 0.0:
        with np.errstate(over="ignore", invalid="ignore"):
            q = np.floor(vtx.astype(np.float64) / np.float64(cell))
        inside = finite & ((q >= -Q_LIMIT) & (q < Q_LIMIT)).all(axis=1)
        keys = np.where(inside[:, None], q, 0.0).astype(np.int64)
    else:
        inside = finite
        keys = np.where(finite[:, None], vtx + np.float32(0.0), np.float32(0.0)).view(np.uint32).astype(np.int64)   # x + 0: -0 becomes +0
    normal = used & inside
    idx = np.arange(nv)
    label = idx.copy()                                                                  # an ALONE vertex is its own label
    if normal.any():
        _, inv = np.unique(keys[normal], axis=0, return_inverse=True)
        inv = inv.reshape(-1)
        smallest = np.full(inv.max() + 1, nv, np.int64)
        np.minimum.at(smallest, inv, idx[normal])
        label[normal] = smallest[inv]
    labels = np.unique(label[used])                                                     # ascending: the clusters' numbers
    vmap = np.full(nv, -1, np.int32)
    vmap[used] = np.searchsorted(labels, label[used])
    n_clusters = len(labels)
    n_members = np.bincount(vmap[used], minlength=n_clusters).astype(np.int32)
    first_vertex = labels.astype(np.int32)
    vtx_out = vtx[first_vertex].copy()
    if mode == MEAN and cell > 0.0 and n_clusters and n_members.max() > 1:
        members = idx[used][np.lexsort((idx[used], vmap[used]))]                        # by cluster, then ascending vertex index
        start = np.concatenate([[0], np.cumsum(n_members)[:-1]])
        many = np.nonzero(n_members > 1)[0]
        s = np.zeros((n_clusters, 3), np.float64)
        v64 = vtx.astype(np.float64)
        for k in range(int(n_members.max())):
            sel = many[n_members[many] > k]
            s[sel] = s[sel] + v64[members[start[sel] + k]]
        with np.errstate(over="ignore"):
            vtx_out[many] = (s[many] / n_members[many].astype(np.float64)[:, None]).astype(np.float32)
    g = vmap[faces]
    fstatus = np.zeros(nf, np.int8)
    fstatus[~counting] = NOT_COUNTING
    collapsed = counting & ((g[:, 0] == g[:, 1]) | (g[:, 1] == g[:, 2]) | (g[:, 0] == g[:, 2]))
    fstatus[collapsed] = COLLAPSED
    if merge_duplicates:
        seen = {}
        srt = np.sort(g, axis=1)
        for f in np.nonzero(fstatus == KEPT)[0].tolist():
            key = (int(srt[f, 0]), int(srt[f, 1]), int(srt[f, 2]))
            if key in seen:
                fstatus[f] = DUPLICATE
            else:
                seen[key] = f
    kept = fstatus == KEPT
    fmap = np.full(nf, -1, np.int32)
    fmap[kept] = np.arange(int(kept.sum()), dtype=np.int32)
    faces_out = np.ascontiguousarray(g[kept], np.int32).reshape(-1, 3)
    alone_nf, alone_out = used & ~finite, used & finite & ~inside
    stats = dict(n_vertices_in=nv, n_vertices_used=int(used.sum()), n_alone_not_finite=int(alone_nf.sum()), n_alone_outside=int(alone_out.sum()),
                 n_vertices_out=n_clusters, largest_cluster=int(n_members.max()) if n_clusters else 0, n_faces_in=nf,
                 n_not_counting=int((~counting).sum()), n_collapsed=int(collapsed.sum()), n_duplicate=int((fstatus == DUPLICATE).sum()),
                 n_faces_out=int(kept.sum()))
    return dict(stats=stats, vtx_out=vtx_out, first_vertex=first_vertex, n_members=n_members, vmap=vmap, fmap=fmap, fstatus=fstatus, faces_out=faces_out)


# ---- the brute force: plain Python, every pair ------------------------------------------------------------------------------------------------------
def _f32(x):
    try:
        return struct.unpack("<I", struct.pack("<f", x))[0]
    except OverflowError:
        return 0x7F800000 if x > 0 else 0xFF800000


def brute(vtx, faces, cell=0.0, mode=FIRST, merge_duplicates=True):
    """-> dict of plain lists; vtx_out as uint32 bit patterns"""
    bits = [[struct.unpack("<I", struct.pack("<f", float(x)))[0] if not math.isnan(float(x)) else int(np.float32(x).view(np.uint32)) for x in v] for v in vtx]
    val = [[struct.unpack("<f", struct.pack("<I", b))[0] for b in v] for v in bits]
    faces = [[int(i) for i in f] for f in faces]
    nv, nf = len(val), len(faces)
    counts = [len({*f}) == 3 for f in faces]
    used = [any(counts[k] and v in faces[k] for k in range(nf)) for v in range(nv)]

    def cells(v):
        out = []
        for x in val[v]:
            d = x / cell
            if math.isinf(d):
                return None
            qq = math.floor(d)
            if not -2 ** 20 <= qq < 2 ** 20:
                return None
            out.append(qq)
        return out

    kind = []                                                                           # 0 unused, 1 normal, 2 not finite, 3 outside
    for v in range(nv):
        if not used[v]:
            kind.append(0)
        elif any(math.isnan(x) or math.isinf(x) for x in val[v]):
            kind.append(2)
        elif cell > 0.0 and cells(v) is None:
            kind.append(3)
        else:
            kind.append(1)

    def together(u, v):
        if u == v:
            return True
        if kind[u] != 1 or kind[v] != 1:
            return False
        if cell > 0.0:
            return cells(u) == cells(v)
        return all(a == b for a, b in zip(val[u], val[v]))                              # as values: -0.0 == 0.0

    label = [min(u for u in range(nv) if used[u] and together(u, v)) if used[v] else -1 for v in range(nv)]
    labels = sorted({l for l in label if l >= 0})
    vmap = [labels.index(l) if l >= 0 else -1 for l in label]
    members = [[v for v in range(nv) if label[v] == l] for l in labels]
    vtx_out = []
    for l, mem in zip(labels, members):
        if mode == MEAN and cell > 0.0 and len(mem) > 1:
            row = []
            for j in range(3):
                s = 0.0
                for v in mem:
                    s = s + val[v][j]
                row.append(_f32(s / float(len(mem))))
            vtx_out.append(row)
        else:
            vtx_out.append(list(bits[l]))
    fstatus, kept_sets = [], []
    for f in range(nf):
        g = [vmap[i] for i in faces[f]]
        if not counts[f]:
            fstatus.append(NOT_COUNTING)
        elif len(set(g)) < 3:
            fstatus.append(COLLAPSED)
        elif merge_duplicates and any(fstatus[e] in (KEPT, DUPLICATE) and {vmap[i] for i in faces[e]} == set(g) for e in range(f)):
            fstatus.append(DUPLICATE)
        else:
            fstatus.append(KEPT)
    fmap, faces_out = [], []
    for f in range(nf):
        if fstatus[f] == KEPT:
            fmap.append(len(faces_out))
            faces_out.append([vmap[i] for i in faces[f]])
        else:
            fmap.append(-1)
    stats = dict(n_vertices_in=nv, n_vertices_used=sum(used), n_alone_not_finite=kind.count(2), n_alone_outside=kind.count(3), n_vertices_out=len(labels),
                 largest_cluster=max([len(m) for m in members], default=0), n_faces_in=nf, n_not_counting=counts.count(False),
                 n_collapsed=fstatus.count(COLLAPSED), n_duplicate=fstatus.count(DUPLICATE), n_faces_out=len(faces_out))
    return dict(stats=stats, vtx_out=vtx_out, first_vertex=labels, n_members=[len(m) for m in members], vmap=vmap, fmap=fmap, fstatus=fstatus,
                faces_out=faces_out)


def same_as_brute(res, ref):
    assert res["stats"] == ref["stats"], (res["stats"], ref["stats"])
    assert res["vtx_out"].view(np.uint32).tolist() == ref["vtx_out"]
    for k in ("first_vertex", "n_members", "vmap", "fmap", "fstatus", "faces_out"):
        assert res[k].tolist() == ref[k], k


def same(got, ref, what=""):
    """two results in simplify()'s shape, bit for bit (vtx_out as bits: a NaN of an ALONE vertex keeps its payload)"""
    assert got["stats"] == ref["stats"], (what, got["stats"], ref["stats"])
    for k, t in ARRAYS:
        assert got[k].dtype == ref[k].dtype == t and got[k].shape == ref[k].shape, (what, k, got[k].dtype, got[k].shape, ref[k].shape)
        assert got[k].tobytes() == ref[k].tobytes(), (what, k, got[k][:12], ref[k][:12])


# ---- the facts the header states -------------------------------------------------------------------------------------------------------------------------
def check_facts(vtx, faces, res, cell, mode, merge_duplicates=True):
    vtx = np.asarray(vtx, np.float32).reshape(-1, 3)
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    st, out, vmap = res["stats"], res["faces_out"], res["vmap"]
    n_out = st["n_vertices_out"]
    assert len(out) == st["n_faces_out"] == st["n_faces_in"] - st["n_not_counting"] - st["n_collapsed"] - st["n_duplicate"]
    assert ((out >= 0) & (out < n_out)).all() and ((out[:, 0] != out[:, 1]) & (out[:, 1] != out[:, 2]) & (out[:, 0] != out[:, 2])).all()
    assert int(res["n_members"].sum()) == st["n_vertices_used"] and (vmap >= 0).sum() == st["n_vertices_used"] and len(res["vtx_out"]) == n_out
    named = np.zeros(n_out, bool)
    named[out.reshape(-1)] = True
    alive = np.zeros(n_out, bool)                                                       # clusters that a kept face of the input names
    alive[vmap[faces[res["fstatus"] == KEPT]].reshape(-1)] = True
    assert np.array_equal(named, alive)                                                 # an output vertex no face uses lost all its faces
    if mode == FIRST or cell == 0.0:
        assert res["vtx_out"].tobytes() == vtx[res["first_vertex"]].tobytes()
        if named.all() and np.isfinite(res["vtx_out"]).all():
            again = simplify(res["vtx_out"], out, cell, mode, merge_duplicates)
            a = again["stats"]
            assert a["largest_cluster"] == (1 if n_out else 0) and a["n_collapsed"] == 0 and a["n_duplicate"] == 0 and a["n_not_counting"] == 0
            assert again["vtx_out"].tobytes() == res["vtx_out"].tobytes() and np.array_equal(again["faces_out"], out)
    elif cell > 0.0:
        # the members of a cell lie within cell (1 + 2^-52) of each other and the exact mean among them; the sequential double sum of n members is
        # off by at most n 2^-53 of the largest magnitude per step, and the result is rounded once to float: half a float spacing
        used = vmap >= 0
        m64 = res["vtx_out"].astype(np.float64)[vmap[used]]
        x64 = vtx.astype(np.float64)[used]
        ok = np.isfinite(x64).all(axis=1) & (res["n_members"][vmap[used]] > 1)
        n = float(st["largest_cluster"])
        bound = cell * (1 + 2.0 ** -40) + np.spacing(np.abs(res["vtx_out"][vmap[used]])).astype(np.float64) + n * n * 2.0 ** -52 * np.abs(x64)
        with np.errstate(invalid="ignore"):
            assert (np.abs(m64 - x64)[ok] <= bound[ok]).all()
    return res


# ---- generators ---------------------------------------------------------------------------------------------------------------------------------------------
CUBE_VTX = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], np.float32)                    # vertex 4 x + 2 y + z
CUBE_FACES = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]],
                      np.int32)                                                                                 # outward, consistent


def unshared(vtx, faces, rng=None):
    """every face with three vertices of its own (an STL-style soup); rng: the vertex indices shuffled"""
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    v = np.asarray(vtx, np.float32)[faces.reshape(-1)]
    f = np.arange(3 * len(faces), dtype=np.int32).reshape(-1, 3)
    return relabel(rng, v, f)[:2] if rng is not None else (v, f)


def relabel(rng, vtx, faces):
    """the vertex indices permuted: old vertex v becomes perm[v]"""
    perm = rng.permutation(len(vtx))
    out = np.empty_like(vtx)
    out[perm] = vtx
    return out, perm[faces].astype(np.int32), perm


def cluster_beside_many(rng, n_big=300, n_small=500):
    """one cell (cell = 1) holding n_big vertices beside n_small cells of one to three, every vertex in faces, the indices shuffled"""
    big = rng.uniform(0.05, 0.95, (n_big, 3))
    small = [np.array([3.0 + 2.0 * k, 0.0, 0.0]) + rng.uniform(0.05, 0.95, (1 + k % 3, 3)) for k in range(n_small)]
    vtx = np.concatenate([big] + small).astype(np.float32)
    nv = len(vtx)
    a = np.arange(nv)
    faces = np.stack([a, (a + 1) % nv, (a + 7) % nv], axis=-1).astype(np.int32)
    return relabel(rng, vtx, faces)[:2]


ORDER_TRIPLE = (float.fromhex("0x1.005decp+1"), float.fromhex("0x1.eca9d8p+50"), float.fromhex("0x1.960aaep+54"))   # one cell of cell = 2^62


def order_triple(order=(0, 1, 2)):
    """three vertices whose x are ORDER_TRIPLE in the given order, all in the cell q = 0 of cell = 2^62, and two faces that name them with three more"""
    x = np.array([ORDER_TRIPLE[i] for i in order], np.float32)
    assert x.astype(np.float64).tolist() == [ORDER_TRIPLE[i] for i in order]           # exact floats
    vtx = np.zeros((6, 3), np.float32)
    vtx[:3, 0] = x
    vtx[3:, 0] = -1.0                                                                   # the cell q = -1
    vtx[3:, 1] = [2.0 ** 63, 2.0 ** 64, 2.0 ** 65]                                      # each in a cell of its own
    return vtx, np.array([[0, 3, 4], [1, 4, 5], [2, 5, 3]], np.int32)


def status_soup():
    """every face status under the weld: vertex 3 welds with 0 and 5 with 1, 4 is unused; face 0 in all six rotations and windings, once more over
    the welded copies, a face that collapses under the weld, one that does not count, and one that collapses"""
    vtx = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 0], [5, 5, 5], [1, 0, 0]], np.float32)
    faces = np.array([[0, 1, 2], [1, 2, 0], [2, 0, 1], [0, 2, 1], [2, 1, 0], [1, 0, 2], [3, 5, 2], [0, 3, 1], [2, 2, 1], [0, 1, 5]], np.int32)
    return vtx, faces


def key_cases():
    """vertices in pairs that fall together or do not, with cell = 0.5: every vertex is named by a face of its own with two far helpers"""
    c = 0.5
    rows = [[-0.0, 0.0, 0.0], [0.0, -0.0, -0.0],                                       # 0, 1: zeros of both signs
            [np.nan, 1.0, 1.0], [np.nan, 1.0, 1.0],                                     # 2, 3: equal bits, never merged
            [np.inf, 1.0, 1.0], [np.inf, 1.0, 1.0],                                     # 4, 5
            [3 * c, 0.0, 0.0], [np.nextafter(np.float32(3 * c), np.float32(0)), 0.0, 0.0], [3 * c + 0.25, 0.0, 0.0],   # 6, 7, 8: on the wall k cell, below it, inside
            [-3 * c, 0.0, 0.0], [np.nextafter(np.float32(-3 * c), np.float32(-9)), 0.0, 0.0], [-3 * c + 0.25, 0.0, 0.0],   # 9, 10, 11: a negative k
            [(2 ** 20 - 1) * c, 9.0, 9.0], [(2 ** 20 - 1) * c + 0.25, 9.0, 9.0],        # 12, 13: q = 2^20 - 1, inside
            [-(2 ** 20) * c, 9.0, 9.0], [-(2 ** 20) * c + 0.25, 9.0, 9.0],              # 14, 15: q = -2^20, inside
            [2 ** 20 * c, 9.0, 9.0], [2 ** 20 * c, 9.0, 9.0],                           # 16, 17: q = 2^20: alone
            [-(2 ** 20) * c - 0.25, 9.0, 9.0], [-(2 ** 20) * c - 0.25, 9.0, 9.0],       # 18, 19: q = -2^20 - 1: alone
            [3e38, 9.0, 9.0], [3e38, 9.0, 9.0]]                                         # 20, 21: far outside
    vtx = np.array(rows, np.float32)
    n = len(vtx)
    helpers = np.array([[1000.0 + 7 * k, 500.0, 0.0] for k in range(2 * n)], np.float32)
    faces = np.array([[k, n + 2 * k, n + 2 * k + 1] for k in range(n)], np.int32)
    return np.concatenate([vtx, helpers]), faces, c
