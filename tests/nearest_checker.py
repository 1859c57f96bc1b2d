"""numpy restatement of the mesh-to-cloud contract (include/immesh_nearest.h) by brute force: every query against every cloud point, no hierarchy,
and the sampler as a plain loop over faces and samples with Python integers for the hash.
Every double operation is written in the header's order; numpy does not fuse multiply-adds, so the results are bit-identical to the kernels'.
The Point rule, the Box rule and the Stats rule are those of immesh_closest.h and are taken from its checker (tests/closest_checker.py)."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import closest_checker as cc

NAN32 = cc.NAN32
MASK = (1 << 64) - 1
G = 0x9E3779B97F4A7C15
MAX_SAMPLES = 2 ** 31 - 2

points = cc.points
box_bound = cc.box_bound


class TooManySamples(Exception):
    """the contract's IMMESH_E_CAPACITY: the int64 total of k_f exceeds 2^31 - 2"""


# ---- the hash ------------------------------------------------------------------------------------------------------------------------------------
def mix(z):
    z &= MASK
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & MASK
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & MASK
    z ^= z >> 31
    return z


def U(h):
    return float(h >> 11) * 2.0 ** -53                                             # (h >> 11 < 2^53: the conversion is exact)


def face_hash(seed, f):
    return mix((seed + G * (f + 1)) & MASK)


# ---- nearest ---------------------------------------------------------------------------------------------------------------------------------------
def distance2(p, c32):
    """the D rule for pairs: p (n, 3) float64, c32 (n, 3) float32 -> D (n,)"""
    e = c32.astype(np.float64) - p
    return (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]


def _chunk(p, cT, r2):
    """queries (valid) x every live cloud point -> D (m,; -1 without a neighbour), position among the live points (m,; -1)"""
    e = cT[0][None, :] - p[:, 0][:, None]
    D = e * e
    np.subtract(cT[1][None, :], p[:, 1][:, None], out=e)
    np.multiply(e, e, out=e)
    D += e                                                                           # (e_x e_x + e_y e_y)
    np.subtract(cT[2][None, :], p[:, 2][:, None], out=e)
    np.multiply(e, e, out=e)
    D += e                                                                           # ... + e_z e_z
    at = np.argmin(D, axis=1)                                                        # the first of the smallest: the smaller index
    best = D[np.arange(len(p)), at]
    have = best <= r2
    return np.where(have, best, -1.0), np.where(have, at, -1)


def nearest(rot, pos, pts, max_dist, cloud, pairs_per_chunk=1 << 21, threads=None):
    """-> D (n,) float64, dist (n,) float32, index (n,) int32, xyz (n, 3) float32 per the contract; rot None: world coordinates"""
    p, ok = points(rot, pos, pts)
    n = len(p)
    cloud = np.asarray(cloud, np.float32).reshape(-1, 3)
    live = np.nonzero(np.isfinite(cloud).all(axis=1))[0]                             # the points in the index
    r2 = float(max_dist) * float(max_dist)
    D, index = np.full(n, -1.0), np.full(n, -1, np.int64)
    idx = np.nonzero(ok)[0]
    if len(idx) and len(live):
        cT = np.ascontiguousarray(cloud[live].astype(np.float64).T)                  # one row per axis
        step = max(1, pairs_per_chunk // len(live))
        parts = [idx[i:i + step] for i in range(0, len(idx), step)]
        threads = min(16, os.cpu_count() or 1) if threads is None else threads
        threads = max(1, min(threads, len(parts)))

        def work(part):
            return _chunk(p[part], cT, r2)
        if threads > 1:
            with ThreadPoolExecutor(threads) as pool:
                done = list(pool.map(work, parts))
        else:
            done = [work(part) for part in parts]
        for part, (bd, at) in zip(parts, done):
            D[part] = bd
            index[part] = np.where(at >= 0, live[np.maximum(at, 0)], -1)
    have = index >= 0
    dist = np.where(have, np.sqrt(np.where(have, D, 0.0)).astype(np.float32), np.float32(-1.0)).astype(np.float32)
    xyz = np.full((n, 3), NAN32, np.float32)
    xyz[have] = cloud[index[have]]
    return D, dist, index.astype(np.int32), xyz


def stats(rot, pos, pts, dist, index, bin_width, n_bins):
    """the Stats rule over a query's dist and index -> dict with immesh_closest_stats' names (n_with_face: with a neighbour), hist (n_bins,) int64"""
    return cc.stats(rot, pos, pts, dist, index, bin_width, n_bins)


# ---- the sampler -----------------------------------------------------------------------------------------------------------------------------------
def _cross(p, q):
    return np.array([p[1] * q[2] - p[2] * q[1], p[2] * q[0] - p[0] * q[2], p[0] * q[1] - p[1] * q[0]])


def face_x(vtx, face, density):
    """x of one face (three indices), or None when the face is not in the hierarchy"""
    n_vtx = len(vtx)
    if any(int(i) < 0 or int(i) >= n_vtx for i in face):
        return None
    P = vtx[np.asarray(face, np.int64)]
    if not np.isfinite(P).all():
        return None
    A, B, C = P.astype(np.float64)
    with np.errstate(all="ignore"):
        n = _cross(B - A, C - A)
        return float((0.5 * np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])) * np.float64(density))


def face_count(x, seed, f):
    """k_f from x (None: not in the hierarchy)"""
    if x is None:
        return 0
    if not np.isfinite(x) or x >= 2.0 ** 31:
        return 2 ** 31
    fl = float(np.floor(x))
    return int(fl) + (1 if U(face_hash(seed, f)) < x - fl else 0)


def faces_x(vtx, faces, density):
    """x of every face at once (the same operations as face_x, in numpy) -> x (n,) float64, live (n,) bool"""
    n_vtx = len(vtx)
    live = ((faces >= 0) & (faces < n_vtx)).all(axis=1)
    P = vtx[np.where(live[:, None], faces, 0)] if n_vtx else np.zeros((len(faces), 3, 3), np.float32)
    live = live & np.isfinite(P).all(axis=(1, 2))
    A, B, C = (P[:, k].astype(np.float64) for k in range(3))
    with np.errstate(all="ignore"):
        ab, ac = B - A, C - A
        n = [ab[:, 1] * ac[:, 2] - ab[:, 2] * ac[:, 1], ab[:, 2] * ac[:, 0] - ab[:, 0] * ac[:, 2], ab[:, 0] * ac[:, 1] - ab[:, 1] * ac[:, 0]]
        return (0.5 * np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])) * np.float64(density), live


def counts(vtx, faces, density, seed):
    """k_f of every face, as Python integers"""
    vtx = np.asarray(vtx, np.float32).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    x, live = faces_x(vtx, faces, density)
    return [face_count(float(x[f]) if live[f] else None, seed, f) for f in range(len(faces))]


def uv(hf, j):
    """the folded barycentric pair of sample j of a face with hash hf"""
    u = U(mix((hf + G * (2 * j + 1)) & MASK))
    v = U(mix((hf + G * (2 * j + 2)) & MASK))
    if u + v > 1.0:
        u, v = 1.0 - u, 1.0 - v
    return u, v


def sample(vtx, faces, density, seed):
    """-> xyz (n, 3) float32, face (n,) int32 per the Samples rule; TooManySamples when the total exceeds 2^31 - 2"""
    vtx = np.asarray(vtx, np.float32).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    k = counts(vtx, faces, density, seed)
    total = sum(k)
    if total > MAX_SAMPLES:
        raise TooManySamples(total)
    xyz, face = np.zeros((total, 3), np.float32), np.zeros(total, np.int32)
    at = 0
    for f, kf in enumerate(k):
        if kf == 0:
            continue
        hf = face_hash(seed, f)
        A, B, C = vtx[faces[f]].astype(np.float64)
        ab, ac = B - A, C - A
        w = np.array([uv(hf, j) for j in range(kf)])
        with np.errstate(all="ignore"):
            xyz[at:at + kf] = ((A[None, :] + ab[None, :] * w[:, 0:1]) + ac[None, :] * w[:, 1:2]).astype(np.float32)
        face[at:at + kf] = f
        at += kf
    return xyz, face
