"""numpy restatement of the renderer's contract (include/immesh_render.h): depth / face image and reinforced points of a triangle soup.
Every double operation is written in the header's order; numpy does not fuse multiply-adds, so the results are bit-identical to the kernels'.
The per-face work runs over each face's candidate box (a batch of faces at a time, the (face, pixel) pairs flattened); `brute=True` tests every
pixel of the image instead, which shows the box loses nothing."""
import math

import numpy as np

_NONE = np.uint64(0xFFFFFFFFFFFFFFFF)


def _cam(cam):
    return (np.array(cam.rot, np.float64).reshape(3, 3), np.array(cam.pos, np.float64), int(cam.width), int(cam.height), float(cam.focus),
            float(cam.z_near), float(cam.z_far), float(cam.downsample_res))


def _cross(p, q):
    return np.stack([p[..., 1] * q[..., 2] - p[..., 2] * q[..., 1],
                     p[..., 2] * q[..., 0] - p[..., 0] * q[..., 2],
                     p[..., 0] * q[..., 1] - p[..., 1] * q[..., 0]], axis=-1)


def _dot(p, q):
    return (p[..., 0] * q[..., 0] + p[..., 1] * q[..., 1]) + p[..., 2] * q[..., 2]


def face_setup(cam, vtx, faces):
    """per face: ab, bc, ca, n, na, candidate box (u0, u1, v0, v1) and `live` (not skipped, not culled, box not empty)"""
    rot, pos, w, h, f, zn, zf, _ = _cam(cam)
    vtx = np.asarray(vtx, np.float32).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    if len(faces) and (faces.min() < 0 or faces.max() >= len(vtx)):
        raise ValueError("vertex index out of range")
    P = vtx.astype(np.float64)[faces]                                   # (nf, 3 vertices, 3)
    finite = np.isfinite(P).all(axis=(1, 2))
    P = np.where(finite[:, None, None], P, 0.0)
    d = P - pos
    A = np.stack([(rot[0, k] * d[..., 0] + rot[1, k] * d[..., 1]) + rot[2, k] * d[..., 2] for k in range(3)], axis=-1)
    a, b, c = A[:, 0], A[:, 1], A[:, 2]
    out = {"ab": _cross(a, b), "bc": _cross(b, c), "ca": _cross(c, a), "n": _cross(b - a, c - a)}
    out["na"] = _dot(out["n"], a)
    dep = -A[..., 2]
    live = finite & (dep.max(axis=1) >= zn) & (dep.min(axis=1) < zf)
    cx, cy = float(w // 2), float(h // 2)
    box = [np.full(len(faces), np.inf), np.full(len(faces), -np.inf), np.full(len(faces), np.inf), np.full(len(faces), -np.inf)]

    def extend(m, x, y, dd):
        with np.errstate(all="ignore"):
            U = cx + (x / dd) * f
            V = cy - (y / dd) * f
        box[0] = np.where(m, np.fmin(box[0], U), box[0]); box[1] = np.where(m, np.fmax(box[1], U), box[1])
        box[2] = np.where(m, np.fmin(box[2], V), box[2]); box[3] = np.where(m, np.fmax(box[3], V), box[3])

    for k in range(3):
        extend(dep[:, k] >= zn, A[:, k, 0], A[:, k, 1], dep[:, k])
    for k in range(3):
        j = (k + 1) % 3
        m = (dep[:, k] < zn) != (dep[:, j] < zn)
        with np.errstate(all="ignore"):
            t = (zn - dep[:, k]) / (dep[:, j] - dep[:, k])
            x = A[:, k, 0] + t * (A[:, j, 0] - A[:, k, 0])
            y = A[:, k, 1] + t * (A[:, j, 1] - A[:, k, 1])
        extend(m, x, y, zn)
    W, H = w + 4.0, h + 4.0
    with np.errstate(all="ignore"):
        u0 = np.maximum(0, np.floor(np.minimum(np.maximum(box[0], -4.0), W)) - 1.0)
        u1 = np.minimum(w - 1, np.ceil(np.minimum(np.maximum(box[1], -4.0), W)) + 1.0)
        v0 = np.maximum(0, np.floor(np.minimum(np.maximum(box[2], -4.0), H)) - 1.0)
        v1 = np.minimum(h - 1, np.ceil(np.minimum(np.maximum(box[3], -4.0), H)) + 1.0)
    u0, u1, v0, v1 = [np.nan_to_num(q, nan=0.0).astype(np.int64) for q in (u0, u1, v0, v1)]
    out["live"] = live & (u0 <= u1) & (v0 <= v1)
    out["finite"] = finite
    out["box"] = (u0, u1, v0, v1)
    return out


def _test_pairs(cam, S, fid, u, v, best):
    """the coverage / depth test for (face, pixel) pairs; min-reduce their keys into best (h * w uint64)"""
    rot, pos, w, h, f, zn, zf, _ = _cam(cam)
    cx, cy = w // 2, h // 2
    dirv = np.stack([(u - cx).astype(np.float64) / f, -((v - cy).astype(np.float64) / f), np.full(len(u), -1.0)], axis=-1)
    e0, e1, e2 = _dot(S["ab"][fid], dirv), _dot(S["bc"][fid], dirv), _dot(S["ca"][fid], dirv)
    cov = ((e0 >= 0) & (e1 >= 0) & (e2 >= 0)) | ((e0 <= 0) & (e1 <= 0) & (e2 <= 0))
    nd = _dot(S["n"][fid], dirv)
    ok = cov & (nd != 0)
    with np.errstate(all="ignore"):
        s = S["na"][fid] / np.where(ok, nd, 1.0)
    ok &= (s >= zn) & (s < zf)
    if not ok.any():
        return
    d32 = s[ok].astype(np.float32)
    key = (d32.view(np.uint32).astype(np.uint64) << np.uint64(32)) | fid[ok].astype(np.uint64)
    np.minimum.at(best, v[ok] * w + u[ok], key)


def render(cam, vtx, faces, brute=False, batch_pairs=1 << 22):
    """-> depth (h, w) float32, face (h, w) int32, the contract's image of the soup"""
    _, _, w, h, f, zn, zf, _ = _cam(cam)
    S = face_setup(cam, vtx, faces)
    best = np.full(w * h, _NONE, np.uint64)
    live = np.nonzero(S["live"])[0]
    if brute:   # every face without a non-finite vertex, over every pixel
        uu, vv = np.meshgrid(np.arange(w), np.arange(h))
        uu, vv = uu.reshape(-1), vv.reshape(-1)
        for fidx in np.nonzero(S["finite"])[0]:
            _test_pairs(cam, S, np.full(len(uu), fidx), uu, vv, best)
    else:
        u0, u1, v0, v1 = S["box"]
        bw = (u1 - u0 + 1)[live]
        area = bw * (v1 - v0 + 1)[live]
        start = 0
        while start < len(live):
            cum = np.cumsum(area[start:])
            stop = start + max(1, int(np.searchsorted(cum, batch_pairs, side="right")))
            fl, ar, bwl = live[start:stop], area[start:stop], bw[start:stop]
            fid = np.repeat(fl, ar)
            k = np.arange(int(ar.sum())) - np.repeat(np.cumsum(ar) - ar, ar)
            bwr = np.repeat(bwl, ar)
            _test_pairs(cam, S, fid, u0[fid] + k % bwr, v0[fid] + k // bwr, best)
            start = stop
    valid = best != _NONE
    d32 = (best >> np.uint64(32)).astype(np.uint32).view(np.float32)
    valid &= d32.astype(np.float64) < 0.99 * zf
    depth = np.where(valid, d32, np.float32(-1.0)).astype(np.float32).reshape(h, w)
    face = np.where(valid, (best & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32).reshape(h, w)
    return depth, face


def unproject(cam, depth):
    """world points of the valid pixels, pixel order -> (n, 3) float32, pixel indices"""
    rot, pos, w, h, f, _, _, _ = _cam(cam)
    idx = np.nonzero(depth.reshape(-1) >= 0)[0]
    u, v = idx % w, idx // w
    d = depth.reshape(-1)[idx].astype(np.float64)
    x = ((u - w // 2).astype(np.float64) / f) * d
    y = -((v - h // 2).astype(np.float64) / f) * d
    z = -d
    pts = np.stack([((rot[r, 0] * x + rot[r, 1] * y) + rot[r, 2] * z) + pos[r] for r in range(3)], axis=-1).astype(np.float32)
    return pts, idx


def _round_away(q):
    """std::round on float32: half away from zero, in float32; -0 folded into +0 (one cell, as the reference's int)"""
    r = np.trunc(q)
    r = r + np.where(np.abs(q - r) >= np.float32(0.5), np.sign(q), np.float32(0.0)).astype(np.float32)
    return (r + np.float32(0.0)).astype(np.float32)


def cells(pts, res):
    return _round_away(pts.astype(np.float32) / np.float32(res))


def thin(pts, res):
    """downsample_pts_result over points in pixel order: the first point of each cell stays -> kept indices (ascending)"""
    if np.float32(res) <= 0:
        return np.arange(len(pts))
    if len(pts) == 0:
        return np.zeros(0, np.int64)
    _, first = np.unique(cells(pts, res), axis=0, return_index=True)
    return np.sort(first)


def thin_naive(pts, res):
    """the same rule as a plain dict loop (what the reference's hash does, one point at a time)"""
    r32 = np.float32(res)
    seen, keep = set(), []
    for i, p in enumerate(np.asarray(pts, np.float32)):
        key = tuple(int(math.copysign(math.floor(abs(float(c / r32)) + 0.5), float(c))) for c in p)
        if key not in seen:
            seen.add(key)
            keep.append(i)
    return np.array(keep, np.int64)


def reinforce(cam, depth):
    """reinforced points of a depth image -> (n, 3) float32 in pixel order"""
    pts, _ = unproject(cam, depth)
    return pts[thin(pts, cam.downsample_res)]
