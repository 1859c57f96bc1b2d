"""numpy restatement of the closest-point contract (include/immesh_closest.h) by brute force: every point against every face, no hierarchy.
Every double operation is written in the header's order; numpy does not fuse multiply-adds, so the results are bit-identical to the kernels'.

The winner of a point is the face with the smallest D, and D = max(d2, L(the face's own box)) >= L by definition.  For a chunk of points the Box
arithmetic runs first: e_x e_x of every (point, face) pair over the full chunk x faces matrix, L of the pairs that this alone does not put beyond
r2 (L >= e_x e_x); the face with the smallest L gives an upper bound U = min(r2, its D), the pairs with L > U are dropped (their D exceeds a D
that counts, so they neither win nor tie), and the Face rule runs on the pairs that remain.  Point chunks are independent and run on a small thread pool (numpy releases the interpreter lock inside
its loops)."""
import math
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

LIMIT = 2.0 ** 128
NAN32 = np.array([0x7FC00000], np.uint32).view(np.float32)[0]


def _dot(p, q):
    return (p[..., 0] * q[..., 0] + p[..., 1] * q[..., 1]) + p[..., 2] * q[..., 2]


def _cross(p, q):
    return np.stack([p[..., 1] * q[..., 2] - p[..., 2] * q[..., 1], p[..., 2] * q[..., 0] - p[..., 0] * q[..., 2],
                     p[..., 0] * q[..., 1] - p[..., 1] * q[..., 0]], axis=-1)


def _unit(x):
    return np.where(x > 0, np.where(x < 1, x, 1.0), 0.0)                          # NaN -> 0


def points(rot, pos, pts):
    """the contract's Point rule -> p (n, 3) float64, ok (n,) bool; rot None: world coordinates"""
    f = np.asarray(pts, np.float32).reshape(-1, 3)
    ok = np.isfinite(f).all(axis=1)
    x = f.astype(np.float64)
    if rot is None:
        p = x
    else:
        rot = np.asarray(rot, np.float64).reshape(3, 3)
        pos = np.asarray(pos, np.float64).reshape(3)
        with np.errstate(all="ignore"):
            p = np.stack([((rot[k, 0] * x[:, 0] + rot[k, 1] * x[:, 1]) + rot[k, 2] * x[:, 2]) + pos[k] for k in range(3)], axis=-1)
    with np.errstate(all="ignore"):
        ok = ok & (np.abs(p) < LIMIT).all(axis=1)                                  # (false for NaN)
    return p, ok


def face_q(a, b, c):
    """the Face rule on vertices relative to the point (each (..., 3) float64) -> q (..., 3), side (...,) int8, region (...,) 1 .. 7"""
    ab, ac = b - a, c - a
    ma, mb, mc = -a, -b, -c
    d1, d2, d3, d4, d5, d6 = _dot(ab, ma), _dot(ac, ma), _dot(ab, mb), _dot(ac, mb), _dot(ab, mc), _dot(ac, mc)
    vc = d1 * d4 - d3 * d2
    vb = d5 * d2 - d1 * d6
    va = d3 * d6 - d5 * d4
    den_ab, den_ac = d1 - d3, d2 - d6
    e, g = d4 - d3, d5 - d6
    den_bc = e + g
    s = (va + vb) + vc
    with np.errstate(all="ignore"):
        v3 = _unit(d1 / np.where(den_ab != 0, den_ab, 1.0))
        w5 = _unit(d2 / np.where(den_ac != 0, den_ac, 1.0))
        w6 = _unit(e / np.where(den_bc != 0, den_bc, 1.0))
        inv = np.where(s != 0, 1.0 / np.where(s != 0, s, 1.0), 0.0)
        v7 = _unit(vb * inv)
        w7 = np.minimum(_unit(vc * inv), 1.0 - v7)
    tests = [(d1 <= 0) & (d2 <= 0),
             (d3 >= 0) & (d4 <= d3),
             (vc <= 0) & (d1 >= 0) & (d3 <= 0) & (den_ab != 0),
             (d6 >= 0) & (d5 <= d6),
             (vb <= 0) & (d2 >= 0) & (d6 <= 0) & (den_ac != 0),
             (va <= 0) & (e >= 0) & (g >= 0) & (den_bc != 0)]
    qs = [a, b, a + v3[..., None] * ab, c, a + w5[..., None] * ac, b + w6[..., None] * (c - b)]
    q = (a + ab * v7[..., None]) + ac * w7[..., None]
    region = np.full(q.shape[:-1], 7, np.int8)
    for k in range(5, -1, -1):                                                     # the first test that holds decides: apply them last to first
        q = np.where(tests[k][..., None], qs[k], q)
        region = np.where(tests[k], np.int8(k + 1), region)
    sd = _dot(_cross(ab, ac), ma)
    side = np.where(sd > 0, 1, np.where(sd < 0, -1, 0)).astype(np.int8)
    return q, side, region


def box_bound(p, lo, hi):
    """the Box rule: p (..., 3) float64, lo / hi (..., 3) floats widened -> L"""
    e = np.maximum(np.maximum(lo - p, p - hi), 0.0)
    return (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]


def pair(p, tri32):
    """one face per point: p (n, 3) float64, tri32 (n, 3 vertices, 3) float32 (finite) -> D (n,), q (n, 3), side (n,), d2 (n,), L (n,)"""
    t = tri32.astype(np.float64)
    q, side, _ = face_q(t[:, 0] - p, t[:, 1] - p, t[:, 2] - p)
    d2 = _dot(q, q)
    L = box_bound(p, tri32.min(axis=1).astype(np.float64), tri32.max(axis=1).astype(np.float64))
    return np.maximum(d2, L), q, side, d2, L


def face_result(rot, pos, pts, vtx, faces, face):
    """the per-face function: the D, xyz and side the contract gives point k for face[k] (>= 0, a face with finite vertices), whatever the other
    faces are -> D (n,) float64, xyz (n, 3) float32, side (n,) int8"""
    p, _ = points(rot, pos, pts)
    vtx = np.asarray(vtx, np.float32).reshape(-1, 3)
    tri = vtx[np.asarray(faces, np.int64).reshape(-1, 3)[np.asarray(face, np.int64)]]
    D, q, side, _, _ = pair(p, tri)
    return D, (p + q).astype(np.float32), side


def _soup(vtx, faces):
    vtx = np.asarray(vtx, np.float32).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    if len(faces) and (faces.min() < 0 or faces.max() >= len(vtx)):
        raise ValueError("vertex index out of range")
    P32 = vtx[faces] if len(faces) else np.zeros((0, 3, 3), np.float32)
    live = np.nonzero(np.isfinite(P32).all(axis=(1, 2)))[0]                       # the faces in the hierarchy
    P32 = P32[live]
    return live, P32, P32.min(axis=1).astype(np.float64), P32.max(axis=1).astype(np.float64)


def _chunk(p, P32, lo, hi, live, r2, buf):
    """points (already valid) x every face -> D (n,; -1 without a face), face (n,), q (n, 3), side (n,)"""
    n = len(p)
    best_D, best_f = np.full(n, -1.0), np.full(n, -1, np.int64)
    best_q, best_side = np.zeros((n, 3)), np.zeros(n, np.int8)
    # e_x e_x of every pair first, in buffers that are reused: L >= e_x e_x (adding squares never lowers a sum, rounded or not), so only the pairs
    # with e_x e_x <= r2 can have L <= r2
    t, u = buf[0][:n], buf[1][:n]
    px = p[:, 0][:, None]
    np.subtract(lo[0][None, :], px, out=t)
    np.subtract(px, hi[0][None, :], out=u)
    np.maximum(t, u, out=t)
    np.maximum(t, 0.0, out=t)
    np.multiply(t, t, out=t)
    r, f = np.nonzero(t <= r2)                                                       # (row-major: r is sorted)
    if len(r) == 0:
        return best_D, best_f, best_q, best_side
    L = t[r, f]
    for k in (1, 2):                                                                 # (e_x e_x + e_y e_y) + e_z e_z
        pk = p[r, k]
        e = np.maximum(np.maximum(lo[k][f] - pk, pk - hi[k][f]), 0.0)
        L = L + e * e
    keep = L <= r2
    r, f, L = r[keep], f[keep], L[keep]
    if len(r) == 0:
        return best_D, best_f, best_q, best_side
    # the face with the smallest L of every point gives U = its D when that counts: the winner's D is <= U, so only the pairs with L <= U remain
    starts = np.nonzero(np.concatenate([[True], r[1:] != r[:-1]]))[0]
    low = np.minimum.reduceat(L, starts)
    at = np.nonzero(L == np.repeat(low, np.diff(np.concatenate([starts, [len(r)]]))))[0]
    at = at[np.concatenate([[True], r[at][1:] != r[at][:-1]])]                      # the first of them per point
    U = np.full(n, r2)
    U[r[at]] = np.minimum(pair(p[r[at]], P32[f[at]])[0], r2)
    keep = L <= U[r]
    r, f = r[keep], f[keep]
    D, q, side, _, _ = pair(p[r], P32[f])
    keep = D <= r2
    r, f, D, q, side = r[keep], f[keep], D[keep], q[keep], side[keep]
    if len(r):
        order = np.lexsort((live[f], D, r))                                        # per point: the smallest D, then the smaller face index
        r_s = r[order]
        head = order[np.concatenate([[True], r_s[1:] != r_s[:-1]])]
        best_D[r[head]], best_f[r[head]], best_q[r[head]], best_side[r[head]] = D[head], live[f[head]], q[head], side[head]
    return best_D, best_f, best_q, best_side


def closest(rot, pos, pts, max_dist, vtx, faces, pairs_per_chunk=1 << 21, threads=None):
    """-> D (n,) float64, dist (n,) float32, face (n,) int32, xyz (n, 3) float32, side (n,) int8 per the contract; rot None: world coordinates"""
    p, ok = points(rot, pos, pts)
    n = len(p)
    live, P32, lo, hi = _soup(vtx, faces)
    r2 = float(max_dist) * float(max_dist)
    D, face = np.full(n, -1.0), np.full(n, -1, np.int64)
    q, side = np.zeros((n, 3)), np.zeros(n, np.int8)
    idx = np.nonzero(ok)[0]
    if len(idx) and len(live):
        step = max(1, pairs_per_chunk // len(live))
        parts = [idx[i:i + step] for i in range(0, len(idx), step)]
        threads = min(16, os.cpu_count() or 1) if threads is None else threads
        threads = max(1, min(threads, len(parts)))
        lanes = [parts[i::threads] for i in range(threads)]

        lo, hi = np.ascontiguousarray(lo.T), np.ascontiguousarray(hi.T)             # one row per axis

        def work(mine):                                                            # one pair of buffers per thread, reused over its chunks
            buf = (np.empty((step, len(live))), np.empty((step, len(live))))
            return [_chunk(p[part], P32, lo, hi, live, r2, buf) for part in mine]
        if threads > 1:
            with ThreadPoolExecutor(threads) as pool:
                done = list(pool.map(work, lanes))
        else:
            done = [work(lanes[0])]
        res = [None] * len(parts)
        for i, d in enumerate(done):
            res[i::threads] = d
        for part, (bd, bf, bq, bs) in zip(parts, res):
            D[part], face[part], q[part], side[part] = bd, bf, bq, bs
    have = face >= 0
    dist = np.where(have, np.sqrt(np.where(have, D, 0.0)).astype(np.float32), np.float32(-1.0)).astype(np.float32)
    with np.errstate(all="ignore"):
        xyz = np.where(have[:, None], (p + q).astype(np.float32), NAN32).astype(np.float32)
    return D, dist, face.astype(np.int32), xyz, side


def all_D(rot, pos, pts, vtx, faces):
    """D of every (point, face) pair, (n, n_faces) float64 (NaN for faces that are not in the hierarchy): for small cases, to count ties"""
    p, _ = points(rot, pos, pts)
    live, P32, _, _ = _soup(vtx, faces)
    out = np.full((len(p), len(np.asarray(faces).reshape(-1, 3))), np.nan)
    for j, f in enumerate(live):
        out[:, f] = pair(p, np.broadcast_to(P32[j], (len(p), 3, 3)))[0]
    return out


def stats(rot, pos, pts, dist, face, bin_width, n_bins):
    """the Stats rule over a query's dist and face -> dict (sums by math.fsum: the exact sums, correctly rounded), hist (n_bins,) int64"""
    _, ok = points(rot, pos, pts)
    face = np.asarray(face)
    have = face >= 0
    d = np.asarray(dist, np.float32)[have]
    dd = d.astype(np.float64)
    with np.errstate(all="ignore"):
        b = d / np.float32(bin_width)                                               # float arithmetic
    inside = b < np.float32(n_bins)
    hist = np.bincount(b[inside].astype(np.int64), minlength=n_bins).astype(np.int64)
    n = int(have.sum())
    s1, s2 = math.fsum(dd.tolist()), math.fsum((dd * dd).tolist())
    return {"n_points": len(face), "n_with_face": n, "n_not_finite": int((~ok).sum()), "n_no_face": int((ok & ~have).sum()),
            "n_overflow": int((~inside).sum()), "sum_dist": s1, "sum_dist2": s2, "mean": s1 / n if n else 0.0, "rms": math.sqrt(s2 / n) if n else 0.0,
            "max_dist": float(d.max()) if n else 0.0}, hist
