"""Numpy restatement of the contract in include/immesh_colour.h (vertex colours from camera images): pose, projection, the 8-bit bilinear tap of
getSubPixel<cv::Vec3b>, selection_points_for_projection's loop, render_pts_in_voxels (PLAIN), thread_render_pts_in_voxel (VIEW) and
RGB_pts::update_rgb.  Every elementwise operation is one IEEE double operation in the header's order (numpy ufuncs never fuse), so PLAIN results are
comparable bit for bit; VIEW goes through libm's acos and is comparable to rounding."""
import numpy as np

PLAIN, VIEW = 0, 1
SET_ALL, SET_IDS, SET_RECENT, SET_RECENT_HEADS = 0, 1, 2, 3
STATE_DTYPE = np.dtype([("rgb", "<f8", 3), ("cov", "<f8", 3), ("first_exposure", "<f8"), ("obs_dis", "<f8"), ("last_obs_time", "<f8"),
                        ("n_obs", "<i4"), ("pad", "<i4")])


def fresh_state(n):
    """RGB_pts::clear() with g_initial_camera_exp_tim = 1"""
    st = np.zeros(n, STATE_DTYPE)
    st["first_exposure"] = 1.0
    return st


def std_round(x):
    """std::round: half away from zero (numpy's round is half to even)"""
    x = np.asarray(x, np.float64)
    a = np.abs(x)
    r = np.floor(a)
    r = r + (a - r >= 0.5)
    return np.copysign(r, x)


def update_rgb(st, idx, c, obs_dis, sigma, t, e):
    """RGB_pts::update_rgb (pointcloud_rgbd.cpp:125-195) on st[idx] (unique indices), in place -> (return values, first-observation mask)"""
    idx = np.asarray(idx, np.int64)
    k = len(idx)
    c = np.asarray(c, np.float64).reshape(k, 3)
    obs_dis, sigma, t, e = (np.broadcast_to(np.asarray(a, np.float64), (k,)) for a in (obs_dis, sigma, t, e))
    ret = np.zeros(k, np.int32)
    live = ~((c[:, 0] == 0) & (c[:, 1] == 0) & (c[:, 2] == 0))
    live &= ~((c[:, 0] > 255) & (c[:, 1] > 255) & (c[:, 2] > 255))
    s = st[idx]
    with np.errstate(all="ignore"):
        live &= ~((s["obs_dis"] != 0) & (obs_dis > s["obs_dis"] * 1.1))
        first = live & (s["n_obs"] == 0)
        upd = live & (s["n_obs"] != 0)
        new = s.copy()
        # first observation
        new["last_obs_time"][first] = t[first]
        new["obs_dis"][first] = obs_dis[first]
        new["first_exposure"][first] = e[first]
        new["rgb"][first] = c[first] * e[first, None]
        new["cov"][first] = sigma[first, None]
        new["n_obs"][first] = 1
        # State estimation for robotics, section 2.2.6
        sg = sigma[:, None]
        cov = s["cov"] + 0.15 * (t - s["last_obs_time"])[:, None]
        old = cov
        cov = np.sqrt(1.0 / (1.0 / cov / cov + 1.0 / sg / sg))
        rgb = cov * cov * (s["rgb"] / old / old + c * e[:, None] / sg / sg)
        mx = (rgb / s["first_exposure"][:, None]).max(axis=1)
        over = mx > 255
        rgb = np.where(over[:, None], rgb * 254.999 / mx[:, None], rgb)
        n1 = s["n_obs"] + 1
        new["cov"][upd] = cov[upd]
        new["rgb"][upd] = rgb[upd]
        new["obs_dis"][upd] = np.where(obs_dis < s["obs_dis"], obs_dis, s["obs_dis"])[upd]
        new["last_obs_time"][upd] = t[upd]
        new["n_obs"][upd] = n1[upd]
        new["first_exposure"][upd] = ((s["first_exposure"] * n1 + e) / (n1 + 1))[upd]
    st[idx] = new
    ret[upd] = 1
    return ret, first


class Cam:
    """the image's pose and gates as the contract derives them (im: capi.Image or anything with its fields)"""
    def __init__(self, im, mesh_voxel=0.4):
        self.rot = np.array(list(im.rot), np.float64).reshape(3, 3)
        self.pos = np.array(list(im.pos), np.float64)
        r, p = self.rot, self.pos
        self.tc = -((r[0] * p[0] + r[1] * p[1]) + r[2] * p[2])
        self.n = r[:, 2].copy()
        self.fx, self.fy, self.cx, self.cy = float(im.fx), float(im.fy), float(im.cx), float(im.cy)
        self.rows, self.cols = int(im.rows), int(im.cols)
        m = float(im.fov_margin)
        self.u_lo, self.u_hi = m * self.cols + 1, (1 - m) * self.cols
        self.v_lo, self.v_hi = m * self.rows + 1, (1 - m) * self.rows
        self.inv_exposure, self.obs_time = float(im.inv_exposure), float(im.obs_time)
        self.min_depth, self.max_depth, self.max_pe = float(im.min_depth), float(im.max_depth), float(im.max_pe_error)
        self.allow = max(0.05, 0.1 * mesh_voxel)


def project(cam, vpos):
    """-> d = p - pos (n, 3), u, v, front (pc.z >= 0.001), ok (front and available)"""
    p = np.asarray(vpos, np.float32).astype(np.float64).reshape(-1, 3)
    d = p - cam.pos
    r = cam.rot
    pc = ((r[0][None, :] * p[:, 0:1] + r[1][None, :] * p[:, 1:2]) + r[2][None, :] * p[:, 2:3]) + cam.tc[None, :]
    with np.errstate(all="ignore"):
        front = ~(pc[:, 2] < 0.001)
        u = (pc[:, 0] * cam.fx) / pc[:, 2] + cam.cx
        v = (pc[:, 1] * cam.fy) / pc[:, 2] + cam.cy
        ok = front & (u >= cam.u_lo) & (np.ceil(u) < cam.u_hi) & (v >= cam.v_lo) & (np.ceil(v) < cam.v_hi)
    return d, u, v, front, ok


def norm3(d):
    return np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])


def dot3(d, n):
    return (d[:, 0] * n[0] + d[:, 1] * n[1]) + d[:, 2] * n[2]


def r8(x):
    """saturate_cast<uchar>(double): round half to even, clamp"""
    return np.clip(np.rint(x), 0, 255).astype(np.int64)


def sample(img, u, v):
    """getSubPixel<cv::Vec3b>(img, v, u) for available (u, v): each of the four products rounded to 8 bits on its own, saturating sums -> (n, 3) float64"""
    img = np.asarray(img)
    rows, cols = img.shape[:2]
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    fr, fc = np.floor(v), np.floor(u)
    a, b = (v - fr)[:, None], (u - fc)[:, None]
    r0, c0 = fr.astype(np.int64), fc.astype(np.int64)
    r1, c1 = np.minimum(r0 + 1, rows - 1), np.minimum(c0 + 1, cols - 1)   # (one past the image only with weight 0)
    P = img.astype(np.float64)
    t00 = r8(((1.0 - a) * (1.0 - b)) * P[r0, c0])
    t10 = r8((a * (1.0 - b)) * P[r1, c0])
    t01 = r8(((1.0 - a) * b) * P[r0, c1])
    t11 = r8((a * b) * P[r1, c1])
    s = np.minimum(t00 + t10, 255)
    s = np.minimum(s + t01, 255)
    s = np.minimum(s + t11, 255)
    return s.astype(np.float64)


def select_loop(cu, cv, depth):
    """selection_points_for_projection's loop (pointcloud_rgbd.cpp:821-856) over candidates that passed the gates, in order -> kept positions, ascending"""
    mask_depth, mask_index = {}, {}
    for i in range(len(depth)):
        key = (int(cu[i]), int(cv[i]))
        dep = float(depth[i])
        if key not in mask_depth or float(mask_depth[key]) > dep:
            mask_index[key] = i
            mask_depth[key] = np.float32(dep)
    return np.array(sorted(mask_index.values()), np.int64)


def select_order_free(cu, cv, depth):
    """the same result without the order: with m = the cell's smallest (float)depth, the largest index with depth < (double)m, else the
    smallest index with (float)depth == m"""
    depth = np.asarray(depth, np.float64)
    f = depth.astype(np.float32)
    cells = {}
    for i in range(len(depth)):
        cells.setdefault((int(cu[i]), int(cv[i])), []).append(i)
    out = []
    for idx in cells.values():
        idx = np.array(idx)
        m = f[idx].min()
        below = idx[depth[idx] < np.float64(m)]
        out.append(below.max() if len(below) else idx[f[idx] == m].min())
    return np.array(sorted(out), np.int64)


def select(cam, vpos, cand, md):
    """the render set of a selection with cell size md -> (ids, positions in cand)"""
    cand = np.asarray(cand, np.int64)
    d, u, v, _, ok = project(cam, vpos[cand])
    depth = norm3(d)
    with np.errstate(all="ignore"):
        g = ~(depth > cam.max_depth) & ~(depth < cam.min_depth) & ok
    pos = np.flatnonzero(g)
    cu = np.trunc(std_round(u[pos] / md) * md).astype(np.int64)
    cv = np.trunc(std_round(v[pos] / md) * md).astype(np.int64)
    kept = pos[select_loop(cu, cv, depth[pos])] if len(pos) else pos
    return cand[kept], kept


def colour_image(st, vpos, img, im, model, cand, md=0.0, mesh_voxel=0.4):
    """one immesh_colour_image on the state st (in place) -> (stats dict, render-set ids, raw uv (n, 2) float32)"""
    cam = Cam(im, mesh_voxel)
    vpos = np.asarray(vpos, np.float32).reshape(-1, 3)
    cand = np.asarray(cand, np.int64)
    sel = select(cam, vpos, cand, md)[0] if md > 0 else cand
    d, u, v, front, ok = project(cam, vpos[sel])
    uv = np.stack([np.where(front, u, np.nan), np.where(front, v, np.nan)], axis=1).astype(np.float32)
    dot = dot3(d, cam.n)
    stats = dict(n_set=len(cand), n_selected=len(sel), n_hit=0, n_first=0, n_updated=0, pe_count=0, pe_sum=0.0, min_dis=0.0)
    if model == PLAIN:
        fin = dot[~np.isnan(dot)]
        dmin = min(3e8, fin.min()) if len(fin) else 3e8
        stats["min_dis"] = float(dmin)
        with np.errstate(all="ignore"):
            go = ~((dot - dmin > cam.allow) & (st["n_obs"][sel] > 5)) & ok
        k = np.flatnonzero(go)
        c = sample(img, u[k], v[k])
        ret, first = update_rgb(st, sel[k], c, dot[k], 1.5, cam.obs_time, cam.inv_exposure)
    else:
        dis = norm3(d)
        with np.errstate(all="ignore"):
            ang = np.arccos(dot / (dis + 0.0001)) * 57.3
            ang = np.where(ang < 5.0, 5.0, ang)
            dis = np.where(dis < 1.0, 1.0, dis)
            go = ~(ang > 30.0) & ok
        k = np.flatnonzero(go)
        c = sample(img, u[k], v[k])
        ret, first = update_rgb(st, sel[k], c, dis[k], (1.5 * dis[k]) * ang[k], cam.obs_time, cam.inv_exposure)
        s = st[sel[k]]
        with np.errstate(all="ignore"):
            rad = s["rgb"] / cam.inv_exposure
            pe_ok = (ret == 1) & ~((s["rgb"] / s["first_exposure"][:, None]).max(axis=1) > 254) & ~(rad.max(axis=1) > 245.0)
            err = np.minimum(np.abs(norm3(c) - norm3(rad)), cam.max_pe)
        stats["pe_count"] = int(pe_ok.sum())
        stats["pe_sum"] = float(err[pe_ok].sum())
        stats["view_angle"], stats["view_ok"] = ang, ok       # (for the test's distance-to-the-gates check)
    stats["n_hit"], stats["n_first"], stats["n_updated"] = len(k), int(first.sum()), int(ret.sum())
    return stats, sel, uv


def rgb8(st):
    """colour_fetch's rgb_out: rgb / first_exposure, clamped to [0, 255], truncated"""
    q = st["rgb"] / st["first_exposure"][:, None]
    return np.clip(q, 0, 255).astype(np.uint8)


def voxel_keys(xyz, voxel):
    """round(coord / mesh_voxel) of float positions: std::round of the f64 quotient (pointcloud_rgbd.cpp:467-472)"""
    return std_round(np.asarray(xyz, np.float32).astype(np.float64) / voxel).astype(np.int64)


def recent_set(vpos, scan_xyz, voxel, heads=False):
    """vertices (ascending) of the mesh voxels the scan's points fall in; heads: the smallest id of each such non-empty voxel"""
    seen = set(map(tuple, voxel_keys(scan_xyz, voxel)))
    vk = voxel_keys(vpos, voxel)
    ids, taken = [], set()
    for i, key in enumerate(map(tuple, vk)):
        if key in seen and not (heads and key in taken):
            ids.append(i)
            taken.add(key)
    return np.array(ids, np.int64)
