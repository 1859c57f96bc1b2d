"""numpy restatement of the colour pass's contract (include/immesh_shade.h): vertex colours (white, Heat over one coordinate, given bytes) and the
shaded pixel of the render contract's winner face.  Depth, face and the per-face values come from tests/render_checker.py; every double operation
is written in the header's order, numpy does not fuse multiply-adds, so the results are bit-identical to the kernels'."""
import numpy as np

import render_checker as rck

WHITE, AXIS, VERTEX = 0, 1, 2
_T = np.array([[0, 0, 1], [0, 1, 1], [0, 1, 0], [1, 1, 0], [1, 0, 0]], np.float64)     # tinycolormap's Heat


def heat(val):
    """set_color_by_axis's colour of val (float32, any shape) -> (..., 3) uint8 in R, G, B order"""
    x = 1.0 - np.asarray(val, np.float32).astype(np.float64)
    m = np.where(x < 1.0, x, 1.0)                       # std::min(1.0, x): a NaN gives 1
    c = np.where(0.0 < m, m, 0.0)                       # std::max(0.0, m)
    a = c * 4.0
    i = np.floor(a)
    t = a - i
    c0, c1 = _T[i.astype(np.int64)], _T[np.ceil(a).astype(np.int64)]
    col = (1.0 - t)[..., None] * c0 + t[..., None] * c1
    return (col * 255.0).astype(np.int64).astype(np.uint8)


def vertex_range(vtx, axis):
    """min / max of one coordinate over the vertices whose three coordinates are finite -> (lo, hi) float32; none: 0 / 0"""
    vtx = np.asarray(vtx, np.float32).reshape(-1, 3)
    ok = np.isfinite(vtx).all(axis=1)
    if not ok.any():
        return np.float32(0.0), np.float32(0.0)
    return vtx[ok, axis].min(), vtx[ok, axis].max()


def resolve_range(vtx, sh):
    """lo, hi (float32) as the pass uses them"""
    if sh.axis_min >= sh.axis_max:
        return vertex_range(vtx, sh.axis)
    return np.float32(sh.axis_min), np.float32(sh.axis_max)


def colourer_bytes(rgb, states, min_views):
    """immesh_colour_fetch's bytes under min_views: vertices with n_obs < min_views are 0, 0, 0"""
    return np.where((states["n_obs"] >= min_views)[:, None], rgb, 0).astype(np.uint8)


def vertex_colours(vtx, sh, vtx_rgb=None):
    """-> C (n, 3) uint8 in output order R, G, B, and the (lo, hi) of an AXIS pass ((0, 0) otherwise)"""
    vtx = np.asarray(vtx, np.float32).reshape(-1, 3)
    if sh.source == WHITE:
        return np.full((len(vtx), 3), 255, np.uint8), (0.0, 0.0)
    if sh.source == AXIS:
        lo, hi = resolve_range(vtx, sh)
        with np.errstate(all="ignore"):
            val = (vtx[:, sh.axis] - lo) / (hi - lo) if hi > lo else np.zeros(len(vtx), np.float32)
        assert val.dtype == np.float32
        return heat(val), (float(lo), float(hi))
    m = np.asarray(vtx_rgb, np.uint8).reshape(-1, 3)
    assert len(m) == len(vtx)
    return (m[:, ::-1] if sh.bgr else m).copy(), (0.0, 0.0)


def pixel_terms(cam, vtx, faces, face):
    """per covered pixel of `face` (h, w): its flat index, the weights wa, wb, wc and the light L of the contract"""
    rot, pos, w, h, f, _, _, _ = rck._cam(cam)
    S = rck.face_setup(cam, vtx, faces)
    idx = np.nonzero(face.reshape(-1) >= 0)[0]
    fid = face.reshape(-1)[idx].astype(np.int64)
    u, v = idx % w, idx // w
    dirv = np.stack([(u - w // 2).astype(np.float64) / f, -((v - h // 2).astype(np.float64) / f), np.full(len(u), -1.0)], axis=-1)
    e0, e1, e2 = rck._dot(S["ab"][fid], dirv), rck._dot(S["bc"][fid], dirv), rck._dot(S["ca"][fid], dirv)
    E = (e0 + e1) + e2
    zero = E == 0.0
    Es = np.where(zero, 1.0, E)
    third = 1.0 / 3.0
    wa, wb, wc = (np.where(zero, third, e / Es) for e in (e1, e2, e0))
    n = S["n"][fid]
    with np.errstate(all="ignore"):
        L = 0.2 + (np.abs(rck._dot(n, dirv)) / (np.sqrt(rck._dot(n, n)) * np.sqrt(rck._dot(dirv, dirv)))) * 0.5
    return idx, fid, wa, wb, wc, L


def shade(cam, vtx, faces, sh, vtx_rgb=None, depth_face=None, terms=None):
    """-> rgb (h, w, 3) uint8, depth, face, (lo, hi): the contract's image of the soup.  depth_face: a render of the same input, terms: its
    pixel_terms, to save their time when one input is shaded several ways"""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    depth, face = rck.render(cam, vtx, faces) if depth_face is None else depth_face
    C, lo_hi = vertex_colours(vtx, sh, vtx_rgb)
    h, w = face.shape
    rgb = np.empty((h * w, 3), np.uint8)
    rgb[:] = np.array(list(sh.background), np.uint8)
    idx, fid, wa, wb, wc, L = pixel_terms(cam, vtx, faces, face) if terms is None else terms
    if not sh.light:
        L = np.ones(len(idx))
    Ca, Cb, Cc = (C[faces[fid, k]].astype(np.float64) for k in range(3))
    obj = ((wa[:, None] * Ca + wb[:, None] * Cb) + wc[:, None] * Cc) / 255.0
    with np.errstate(all="ignore"):
        lit = L[:, None] * obj
        out = np.floor(np.fmin(np.fmax(lit, 0.0), 1.0) * 255.0 + 0.5)
    rgb[idx] = out.astype(np.int64).astype(np.uint8)
    return rgb.reshape(h, w, 3), depth, face, lo_hi
