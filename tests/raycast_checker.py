"""numpy restatement of the ray caster's contract (include/immesh_raycast.h) by brute force: every ray against every face, no hierarchy.
Every double operation is written in the header's order; numpy does not fuse multiply-adds, so the results are bit-identical to the kernels'.

A fragment counts when Cover, Depth and Box all hold.  The three are a conjunction, so the order of evaluation is free: for a chunk of rays the
Box arithmetic (tn, tf of every (ray, face) pair: cheap, and it needs no cross product) runs first over the full chunk x faces matrix, the pairs
that Box and the range [t_min, t_max) already exclude (tn - g > tf + g, tn - g >= t_max, tf + g < t_min: each contradicts
t_min <= s < t_max and tn - g <= s <= tf + g) are dropped, and the rest of the contract runs on the pairs that remain.  Ray chunks are independent
and run on a small thread pool (numpy releases the interpreter lock inside its loops)."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import render_checker as rck

NEAREST, ANY = 0, 1
_NONE = np.uint64(0xFFFFFFFFFFFFFFFF)
_cross, _dot = rck._cross, rck._dot


def rays(rot, pos, dirs, origins=None):
    """the contract's Ray rule -> d (n, 3), o (n, 3) float64, ok (n,) bool"""
    rot = np.asarray(rot, np.float64).reshape(3, 3)
    pos = np.asarray(pos, np.float64).reshape(3)
    df = np.asarray(dirs, np.float32).reshape(-1, 3)
    ok = np.isfinite(df).all(axis=1) & (df != 0).any(axis=1)
    dd = df.astype(np.float64)
    with np.errstate(all="ignore"):
        d = np.stack([(rot[k, 0] * dd[:, 0] + rot[k, 1] * dd[:, 1]) + rot[k, 2] * dd[:, 2] for k in range(3)], axis=-1)
        if origins is None:
            o = np.broadcast_to(pos, d.shape).copy()
        else:
            of = np.asarray(origins, np.float32).reshape(-1, 3)
            ok &= np.isfinite(of).all(axis=1)
            oo = of.astype(np.float64)
            o = np.stack([((rot[k, 0] * oo[:, 0] + rot[k, 1] * oo[:, 1]) + rot[k, 2] * oo[:, 2]) + pos[k] for k in range(3)], axis=-1)
    ok &= np.isfinite(d).all(axis=1) & np.isfinite(o).all(axis=1)
    return d, o, ok


def _soup(vtx, faces):
    vtx = np.asarray(vtx, np.float32).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    if len(faces) and (faces.min() < 0 or faces.max() >= len(vtx)):
        raise ValueError("vertex index out of range")
    P32 = vtx[faces] if len(faces) else np.zeros((0, 3, 3), np.float32)      # (nf, 3 vertices, 3)
    live = np.nonzero(np.isfinite(P32).all(axis=(1, 2)))[0]                   # the faces in the hierarchy
    P32 = P32[live]
    lo = P32.min(axis=1).astype(np.float64)                                   # the float boxes, widened
    hi = P32.max(axis=1).astype(np.float64)
    return live, P32.astype(np.float64), lo, hi


def _slabs(d, o, lo, hi):
    """Box arithmetic of rays (R) x boxes (F) -> inside (R, F) bool, tn, tf (R, F)"""
    R, F = len(d), len(lo)
    tn = np.full((R, F), -np.inf)
    tf = np.full((R, F), np.inf)
    inside = np.ones((R, F), bool)
    t1, t2, m = np.empty((R, F)), np.empty((R, F)), np.empty((R, F))
    with np.errstate(all="ignore"):
        inv = 1.0 / d
        bound = (d != 0) & np.isfinite(inv)
        for k in range(3):
            b = bound[:, k]
            # rows whose axis does not bound t go through the same arithmetic and are put back to -inf / +inf (inv = 0 there keeps them finite)
            ok_, ik = o[:, k][:, None], np.where(b, inv[:, k], 0.0)[:, None]
            np.subtract(lo[None, :, k], ok_, out=t1); np.multiply(t1, ik, out=t1)
            np.subtract(hi[None, :, k], ok_, out=t2); np.multiply(t2, ik, out=t2)
            if b.all():
                np.minimum(t1, t2, out=m); np.maximum(tn, m, out=tn)
                np.maximum(t1, t2, out=m); np.minimum(tf, m, out=tf)
            else:
                bb = b[:, None]
                np.minimum(t1, t2, out=m); np.maximum(tn, m, out=tn, where=bb)
                np.maximum(t1, t2, out=m); np.minimum(tf, m, out=tf, where=bb)
                on = o[~b, k][:, None]
                inside[~b] &= (lo[None, :, k] <= on) & (on <= hi[None, :, k])
    return inside, tn, tf


def _chunk(d, o, P, lo, hi, live, t_min, t_max):
    """rays (already valid) x every face -> best key per ray (uint64; _NONE without a fragment)"""
    g = t_max * 2.0 ** -24
    best = np.full(len(d), _NONE, np.uint64)
    inside, tn, tf = _slabs(d, o, lo, hi)
    a, b = tn - g, tf + g
    cand = inside & ~(a > b) & ~(a >= t_max) & ~(b < t_min)
    r, f = np.nonzero(cand)
    if len(r) == 0:
        return best
    a, b = a[r, f], b[r, f]
    dr, orr = d[r], o[r]
    A, B, Cc = P[f, 0] - orr, P[f, 1] - orr, P[f, 2] - orr
    e0, e1, e2 = _dot(_cross(A, B), dr), _dot(_cross(B, Cc), dr), _dot(_cross(Cc, A), dr)
    n = _cross(B - A, Cc - A)
    na, nd = _dot(n, A), _dot(n, dr)
    ok = (((e0 >= 0) & (e1 >= 0) & (e2 >= 0)) | ((e0 <= 0) & (e1 <= 0) & (e2 <= 0))) & (nd != 0)
    with np.errstate(all="ignore"):
        s = na / np.where(ok, nd, 1.0)
    ok &= (s >= t_min) & (s < t_max) & (a <= s) & (s <= b)
    if ok.any():
        d32 = s[ok].astype(np.float32) + np.float32(0.0)                          # -0 is the distance +0
        key = (d32.view(np.uint32).astype(np.uint64) << np.uint64(32)) | live[f[ok]].astype(np.uint64)
        np.minimum.at(best, r[ok], key)
    return best


def cast(rot, pos, dirs, origins, t_min, t_max, vtx, faces, mode=NEAREST, pairs_per_chunk=1 << 18, threads=None):
    """-> t (n,) float32, face (n,) int32 per the contract"""
    d, o, ok = rays(rot, pos, dirs, origins)
    n = len(d)
    live, P, lo, hi = _soup(vtx, faces)
    best = np.full(n, _NONE, np.uint64)
    idx = np.nonzero(ok)[0]
    if len(idx) and len(live):
        step = max(1, pairs_per_chunk // len(live))
        parts = [idx[i:i + step] for i in range(0, len(idx), step)]
        work = lambda part: _chunk(d[part], o[part], P, lo, hi, live, float(t_min), float(t_max))
        threads = min(16, os.cpu_count() or 1) if threads is None else threads
        if threads > 1 and len(parts) > 1:
            with ThreadPoolExecutor(threads) as pool:
                res = list(pool.map(work, parts))
        else:
            res = [work(part) for part in parts]
        for part, b in zip(parts, res):
            best[part] = b
    hit = best != _NONE
    if mode == ANY:
        return np.where(hit, np.float32(0), np.float32(-1)).astype(np.float32), np.where(hit, 0, -1).astype(np.int32)
    t = np.where(hit, (best >> np.uint64(32)).astype(np.uint32).view(np.float32), np.float32(-1.0)).astype(np.float32)
    face = np.where(hit, (best & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32)
    return t, face


def hit_points(rot, pos, dirs, origins, t):
    """the Points rule: the hit rays' points in ray order -> (n_hit, 3) float32"""
    d, o, _ = rays(rot, pos, dirs, origins)
    hit = np.asarray(t) >= 0
    dist = np.asarray(t, np.float32)[hit].astype(np.float64)
    return (o[hit] + d[hit] * dist[:, None]).astype(np.float32)


def points(rot, pos, dirs, origins, t, res):
    """reinforced points of a NEAREST cast: the Points rule, thinned by the renderer's Thin rule -> (n, 3) float32 in ray order"""
    pts = hit_points(rot, pos, dirs, origins, t)
    return pts[rck.thin(pts, res)]
