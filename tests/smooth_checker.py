"""The contract of include/immesh_smooth.h restated twice.  smooth() and normals() are the numpy restatement: np.unique on the pair keys, then a loop
over the rank k = 0 .. largest - 1 that adds the k-th neighbour (the k-th face) of every vertex, which is the ascending sequential sum.  brute() and
brute_normals() are plain Python for tiny inputs and share nothing with them: sets per vertex, Python floats, struct for the float rounding."""
import math
import struct

import numpy as np

import topology_checker as tc

STAT_NAMES = ("n_vertices", "n_used", "n_not_finite", "n_border", "n_interior", "n_moving", "n_pairs", "max_valence", "n_steps", "n_held", "n_moved",
              "max_disp2")
UNUSED, NOT_FINITE, BORDER, INTERIOR = 0, 1, 2, 3
FIXED, ALONG, FREE = 0, 1, 2
ARRAYS = (("vtx_out", np.float32), ("vclass", np.int8), ("row_start", np.int64), ("neighbours", np.int32), ("uses", np.int32))


def _faces(vtx, faces):
    vtx = np.ascontiguousarray(vtx, np.float32).reshape(-1, 3)
    faces = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    counting = (faces[:, 0] != faces[:, 1]) & (faces[:, 1] != faces[:, 2]) & (faces[:, 0] != faces[:, 2])
    return vtx, faces, counting


def _ranked_sum(values, start, count):
    """s[i] = ((0 + values[start[i]]) + values[start[i] + 1]) + ... over count[i] rows of values (n, 3) float64, one rank at a time"""
    s = np.zeros((len(count), 3), np.float64)
    some = np.nonzero(count > 0)[0]
    for k in range(int(count.max()) if len(count) else 0):
        sel = some[count[some] > k]
        s[sel] = s[sel] + values[start[sel] + k]
    return s


def smooth(vtx, faces, n_steps=0, lam=0.5, mu=-0.53, border=FIXED):
    vtx, faces, counting = _faces(vtx, faces)
    assert 0 <= n_steps <= 65536 and -1.0 <= lam <= 1.0 and -1.0 <= mu <= 1.0 and border in (FIXED, ALONG, FREE)
    nv = len(vtx)
    F = faces[counting].astype(np.int64)
    a, b = F[:, [0, 1, 1, 2, 2, 0]].reshape(-1), F[:, [1, 0, 2, 1, 0, 2]].reshape(-1)   # both directions of the three edges
    keys, uses = np.unique((a << 32) | b, return_counts=True)
    rows, nbr = keys >> 32, keys & 0xFFFFFFFF
    row_start = np.searchsorted(rows, np.arange(nv + 1)).astype(np.int64)
    valence = np.diff(row_start)
    finite = np.isfinite(vtx).all(axis=1)
    on_border = np.zeros(nv, bool)
    on_border[rows[uses != 2]] = True
    vclass = np.where(valence == 0, UNUSED, np.where(~finite, NOT_FINITE, np.where(on_border, BORDER, INTERIOR))).astype(np.int8)
    row_class = vclass[rows]
    if border == FIXED:
        wanted = row_class == INTERIOR
    elif border == ALONG:
        wanted = (row_class == INTERIOR) | ((row_class == BORDER) & (uses != 2))
    else:
        wanted = row_class >= BORDER
    wanted &= finite[nbr]
    s_rows, s_nbr = rows[wanted], nbr[wanted]                                           # still ascending by row, then neighbour
    count = np.bincount(s_rows, minlength=nv).astype(np.int64)
    start = np.concatenate([[0], np.cumsum(count)[:-1]]).astype(np.int64) if nv else np.zeros(0, np.int64)
    mv = np.nonzero(count > 0)[0]
    P, n_held = vtx.copy(), 0
    for j in range(n_steps):
        w = np.float64(lam if j % 2 == 0 else mu)
        P64 = P.astype(np.float64)
        if len(mv):
            s = _ranked_sum(P64[s_nbr], start[mv], count[mv])
            m = s / count[mv].astype(np.float64)[:, None]
            x = P64[mv]
            t = m - x
            t = w * t
            with np.errstate(over="ignore"):
                r = (x + t).astype(np.float32)
            ok = np.isfinite(r).all(axis=1)
            n_held += int((~ok).sum())
            P = P.copy()
            P[mv[ok]] = r[ok]
    d = P[mv].astype(np.float64) - vtx[mv].astype(np.float64)
    disp2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    stats = dict(n_vertices=nv, n_used=int((valence > 0).sum()), n_not_finite=int((vclass == NOT_FINITE).sum()), n_border=int((vclass == BORDER).sum()),
                 n_interior=int((vclass == INTERIOR).sum()), n_moving=len(mv), n_pairs=len(keys), max_valence=int(valence.max()) if nv else 0, n_steps=n_steps,
                 n_held=n_held, n_moved=int((P.view(np.uint32) != vtx.view(np.uint32)).any(axis=1).sum()), max_disp2=float(disp2.max()) if len(mv) else 0.0)
    return dict(stats=stats, vtx_out=P, vclass=vclass, row_start=row_start, neighbours=nbr.astype(np.int32), uses=uses.astype(np.int32))


def normals(vtx, faces):
    """-> (normals (n_vtx, 3) float32, n_zero)"""
    vtx, faces, counting = _faces(vtx, faces)
    nv = len(vtx)
    finite = np.isfinite(vtx).all(axis=1)
    F = faces.astype(np.int64)
    ok = counting & finite[F].all(axis=1) if len(F) else np.zeros(0, bool)
    fi = np.nonzero(ok)[0]
    V = vtx.astype(np.float64)
    A, B, C = V[F[fi, 0]], V[F[fi, 1]], V[F[fi, 2]]
    p, q = B - A, C - A
    nf = np.stack([p[:, 1] * q[:, 2] - p[:, 2] * q[:, 1], p[:, 2] * q[:, 0] - p[:, 0] * q[:, 2], p[:, 0] * q[:, 1] - p[:, 1] * q[:, 0]], axis=-1)
    corner_v = F[fi].reshape(-1)                                                        # in face order: a stable sort by vertex keeps the faces ascending
    order = np.argsort(corner_v, kind="stable")
    count = np.bincount(corner_v, minlength=nv).astype(np.int64)
    start = np.concatenate([[0], np.cumsum(count)[:-1]]).astype(np.int64) if nv else np.zeros(0, np.int64)
    s = _ranked_sum(nf.reshape(-1, 3)[order // 3], start, count)
    q = (s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2]
    length = np.sqrt(q)
    out = np.zeros((nv, 3), np.float32)
    has = length > 0.0
    out[has] = (s[has] / length[has][:, None]).astype(np.float32)
    return out, int((~has).sum())


# ---- the brute force: plain Python ------------------------------------------------------------------------------------------------------------------------
def _f32(x):
    try:
        return struct.unpack("<I", struct.pack("<f", x))[0]
    except OverflowError:
        return 0x7F800000 if x > 0 else 0xFF800000


def _val(b):
    return struct.unpack("<f", struct.pack("<I", b))[0]


def _plain(vtx, faces):
    bits = [[int(b) for b in row] for row in np.ascontiguousarray(vtx, np.float32).reshape(-1, 3).view(np.uint32)]
    faces = [[int(i) for i in f] for f in np.asarray(faces).reshape(-1, 3)]
    return bits, faces, [f for f in faces if len({*f}) == 3]


def brute(vtx, faces, n_steps=0, lam=0.5, mu=-0.53, border=FIXED):
    """-> dict of plain lists; vtx_out as uint32 bit patterns"""
    bits, faces, cf = _plain(vtx, faces)
    nv = len(bits)
    finite = [all(math.isfinite(_val(b)) for b in row) for row in bits]
    ring = [sorted({u for f in cf if v in f for u in f if u != v}) for v in range(nv)]
    use = [[sum(1 for f in cf if u in f and v in f) for u in ring[v]] for v in range(nv)]
    vclass = [UNUSED if not ring[v] else NOT_FINITE if not finite[v] else BORDER if any(n != 2 for n in use[v]) else INTERIOR for v in range(nv)]
    lists = []
    for v in range(nv):
        if vclass[v] == INTERIOR or (vclass[v] == BORDER and border == FREE):
            lists.append([u for u in ring[v] if finite[u]])
        elif vclass[v] == BORDER and border == ALONG:
            lists.append([u for u, n in zip(ring[v], use[v]) if n != 2 and finite[u]])
        else:
            lists.append([])
    P, n_held = [list(row) for row in bits], 0
    for j in range(n_steps):
        w = lam if j % 2 == 0 else mu
        Q = [list(row) for row in P]
        for v in range(nv):
            if not lists[v]:
                continue
            r = []
            for k in range(3):
                s = 0.0
                for u in lists[v]:
                    s = s + _val(P[u][k])
                m = s / float(len(lists[v]))
                x = _val(P[v][k])
                t = m - x
                t = w * t
                r.append(_f32(x + t))
            if all(math.isfinite(_val(b)) for b in r):
                Q[v] = r
            else:
                n_held += 1
        P = Q
    disp = [0.0]
    for v in range(nv):
        if lists[v]:
            d = [_val(P[v][k]) - _val(bits[v][k]) for k in range(3)]
            disp.append((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    row_start = [0]
    for v in range(nv):
        row_start.append(row_start[-1] + len(ring[v]))
    stats = dict(n_vertices=nv, n_used=sum(1 for r in ring if r), n_not_finite=vclass.count(NOT_FINITE), n_border=vclass.count(BORDER),
                 n_interior=vclass.count(INTERIOR), n_moving=sum(1 for s in lists if s), n_pairs=row_start[-1], max_valence=max([len(r) for r in ring], default=0),
                 n_steps=n_steps, n_held=n_held, n_moved=sum(1 for v in range(nv) if P[v] != bits[v]), max_disp2=max(disp))
    return dict(stats=stats, vtx_out=P, vclass=vclass, row_start=row_start, neighbours=[u for r in ring for u in r], uses=[n for r in use for n in r])


def brute_normals(vtx, faces):
    """-> (rows of uint32 bit patterns, n_zero)"""
    bits, faces, _ = _plain(vtx, faces)
    val = [[_val(b) for b in row] for row in bits]
    finite = [all(math.isfinite(x) for x in row) for row in val]
    out, n_zero = [], 0
    for v in range(len(val)):
        s = [0.0, 0.0, 0.0]
        for f in faces:
            if len({*f}) == 3 and v in f and all(finite[i] for i in f):
                a, b, c = (val[i] for i in f)
                p, q = [b[k] - a[k] for k in range(3)], [c[k] - a[k] for k in range(3)]
                n = [p[1] * q[2] - p[2] * q[1], p[2] * q[0] - p[0] * q[2], p[0] * q[1] - p[1] * q[0]]
                s = [s[k] + n[k] for k in range(3)]
        length = math.sqrt((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2])
        if length > 0.0:
            out.append([_f32(s[k] / length) for k in range(3)])
        else:
            out.append([0, 0, 0])
            n_zero += 1
    return out, n_zero


def same_as_brute(res, ref):
    assert res["stats"] == ref["stats"], (res["stats"], ref["stats"])
    assert res["vtx_out"].view(np.uint32).tolist() == ref["vtx_out"]
    for k in ("vclass", "row_start", "neighbours", "uses"):
        assert res[k].tolist() == ref[k], k


def same(got, ref, what=""):
    """two results in smooth()'s shape, bit for bit (vtx_out as bits: a NaN keeps its payload, -0 is not +0)"""
    assert got["stats"] == ref["stats"], (what, got["stats"], ref["stats"])
    for k, t in ARRAYS:
        assert got[k].dtype == ref[k].dtype == t and got[k].shape == ref[k].shape, (what, k, got[k].dtype, got[k].shape, ref[k].shape)
        assert got[k].tobytes() == ref[k].tobytes(), (what, k, got[k][:12], ref[k][:12])


# ---- the facts the header states -------------------------------------------------------------------------------------------------------------------------
def check_facts(vtx, faces, res):
    vtx, faces, _ = _faces(vtx, faces)
    st, rs, nb, us, vclass = res["stats"], res["row_start"], res["neighbours"], res["uses"], res["vclass"]
    nv = len(vtx)
    ana = tc.analyse(vtx, faces)
    assert st["n_pairs"] == 2 * ana["stats"]["n_edges"] == len(nb) == len(us) == rs[-1] and rs[0] == 0 and len(rs) == nv + 1
    assert st["n_used"] == ana["stats"]["n_vertices_used"] == st["n_not_finite"] + st["n_border"] + st["n_interior"]
    ends = np.concatenate([ana["edges"][kind][0].reshape(-1) for kind in (tc.EDGE_BOUNDARY, tc.EDGE_NONMANIFOLD)])
    want = np.zeros(nv, bool)
    want[ends] = True
    want &= np.isfinite(vtx).all(axis=1)
    assert np.array_equal(vclass == BORDER, want)
    rows = np.repeat(np.arange(nv), np.diff(rs))
    assert (np.diff(rs) >= 0).all() and ((nb[1:] > nb[:-1]) | (rows[1:] != rows[:-1])).all() and (nb != rows).all()   # ascending, no vertex beside itself
    there = {(int(u), int(v)): int(n) for u, v, n in zip(rows, nb, us)}
    assert len(there) == len(nb) and all(there.get((v, u)) == n for (u, v), n in there.items())                        # symmetric, with the same uses
    if st["n_steps"] == 0:
        assert res["vtx_out"].tobytes() == vtx.tobytes() and st["n_moved"] == 0 and st["max_disp2"] == 0.0
    assert np.isfinite(res["vtx_out"][vclass >= BORDER]).all()
    return res


# ---- generators ---------------------------------------------------------------------------------------------------------------------------------------------
def noisy(rng, vtx, sigma):
    return (np.asarray(vtx, np.float64) + rng.normal(scale=sigma, size=np.shape(vtx))).astype(np.float32)


def torus_normals(m, n):
    """the analytic outward normals of tc.torus(m, n)'s vertices"""
    i, j = np.meshgrid(np.arange(m), np.arange(n), indexing="ij")
    th, ph = 2 * np.pi * i / m, 2 * np.pi * j / n
    return np.stack([np.cos(ph) * np.cos(th), np.cos(ph) * np.sin(th), np.sin(ph)], axis=-1).reshape(-1, 3)


def torus_distance(vtx):
    """the distances of points to the torus of tc.torus (major radius 2, minor radius 1)"""
    v = np.asarray(vtx, np.float64)
    return np.abs(np.hypot(np.hypot(v[:, 0], v[:, 1]) - 2.0, v[:, 2]) - 1.0)


def closed_fan(centre, ring):
    """centre 0 over the ring 1, 2, 3: a tetrahedron without its base, x given, y and z of a small triangle"""
    vtx = np.array([[centre, 0, 1], [ring[0], 1, 0], [ring[1], -1, 1], [ring[2], -1, -1]], np.float32)
    return vtx, np.array([[0, 1, 2], [0, 2, 3], [0, 3, 1]], np.int32)


def fan_beside_rings(rng, valence=300, n_small=500):
    """an open fan of `valence` spokes beside n_small closed fans of three, the vertex indices shuffled"""
    t = 2 * np.pi * np.arange(valence) / valence
    vs = [np.concatenate([[[0.0, 0.0, 0.3]], np.stack([np.cos(t), np.sin(t), 0 * t], axis=-1)])]
    k = np.arange(1, valence)
    fs = [np.stack([0 * k, k, k + 1], axis=-1)]
    base = valence + 1
    for i in range(n_small):
        v, f = closed_fan(0.0, (1.0, -0.5, -0.5))
        vs.append(v * 0.1 + np.array([3.0 + i, 0.0, 0.0]))
        fs.append(f + base)
        base += 4
    vtx = noisy(rng, np.concatenate(vs), 0.01)
    perm = rng.permutation(len(vtx))
    out = np.empty_like(vtx)
    out[perm] = vtx
    return out, perm[np.concatenate(fs)].astype(np.int32)


def fins():
    """a 4 x 2 sheet with a fin of two faces standing on its middle row (uses 3 along it), one face given twice more (uses up to 4), a face that does
    not count and an unused vertex"""
    vtx, faces = tc.grid_sheet(4, 2)                                                    # vertex 3 i + j; the middle row is j = 1
    top = np.array([[1.0, 1.0, 1.0], [2.0, 1.0, 1.0], [3.0, 1.0, 1.0], [9.0, 9.0, 9.0]], np.float32)   # 15, 16, 17 above 4, 7, 10; 18 unused
    fin = np.array([[4, 7, 16], [4, 16, 15], [7, 10, 17], [7, 17, 16]], np.int32)
    twice = np.array([[0, 3, 4], [4, 0, 3], [5, 5, 8]], np.int32)
    return np.concatenate([vtx, top]), np.concatenate([faces, fin, twice])


def with_specials(rng, vtx, n=4):
    """some vertices made NaN, +-inf and -0"""
    vtx = np.array(vtx, np.float32)
    pick = rng.choice(len(vtx), min(n, len(vtx)), replace=False)
    for i, v in enumerate(pick):
        vtx[v, rng.integers(0, 3)] = (np.nan, np.inf, -np.inf, -0.0)[i % 4]
    return vtx
