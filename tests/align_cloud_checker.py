"""numpy restatement of the Cloud rule of include/immesh_align.h: the winner by brute force under (D, index) in float64 (every source point against
every cloud point, no hierarchy: nearest_checker.nearest), q as the D rule's e_k, the rows and the 28 terms through align_checker._row (the mesh
rule's arithmetic, imported and not restated), the weight in scalar order, the system by math.fsum, and the loop over align_checker's solve and
update."""
import math

import numpy as np

import align_checker as ac
import closest_checker as cc
import nearest_checker as nc

POINT, PLANE = ac.POINT, ac.PLANE
N_TERMS = ac.N_TERMS


def correspondences(rot, pos, pts, max_dist, cloud):
    """-> p (n, 3), ok (n,), index (n,) int32 (-1: none), q (n, 3) = (double)c_j - p (zeros without a winner)"""
    p, ok = cc.points(rot, pos, pts)
    cloud = np.asarray(cloud, np.float32).reshape(-1, 3)
    _, _, index, _ = nc.nearest(rot, pos, pts, max_dist, cloud)
    q = np.zeros((len(p), 3))
    have = index >= 0
    q[have] = cloud[index[have]].astype(np.float64) - p[have]
    return p, ok, index, q


def weight(d, huber):
    """the Weight rule, one point after the other -> w (n,)"""
    return np.array([1.0 if float(x) <= huber else huber / float(x) for x in d]).reshape(len(d))


def terms(mode, p, centre, index, q, huber=0.0, normal=None, nstatus=None):
    """-> terms (n, 28) (zeros for a point that does not take part), used (n,) bool, flat (n,) bool (PLANE: a winner without a normal)"""
    n = len(p)
    out = np.zeros((n, N_TERMS))
    have = index >= 0
    flat = np.zeros(n, bool)
    if mode == PLANE:
        flat[have] = np.asarray(nstatus)[index[have]] != 0
    used = have & ~flat
    idx = np.nonzero(used)[0]
    if len(idx) == 0:
        return out, used, flat
    x = p[idx] - np.asarray(centre, np.float64).reshape(3)
    qq = q[idx]
    if mode == POINT:
        t = None
        for k in range(3):
            u = np.zeros((len(idx), 3))
            u[:, k] = 1.0
            t = ac._row(x, u, qq[:, k], t)
        d = np.sqrt((qq[:, 0] * qq[:, 0] + qq[:, 1] * qq[:, 1]) + qq[:, 2] * qq[:, 2])
    else:
        u = np.asarray(normal, np.float32).reshape(-1, 3)[index[idx]].astype(np.float64)
        r = cc._dot(u, qq)
        t = ac._row(x, u, r, None)
        d = np.abs(r)
    if huber > 0.0:
        t = weight(d, huber)[:, None] * t
    out[idx] = t
    return out, used, flat


def step(rot, pos, pts, mode, max_dist, centre, cloud, huber=0.0, normal=None, nstatus=None):
    """one step -> dict: index, terms, sums, bound, counts (n_used, n_not_finite, no neighbour, winner without a normal)"""
    p, ok, index, q = correspondences(rot, pos, pts, max_dist, cloud)
    tm, used, flat = terms(mode, p, centre, index, q, huber, normal, nstatus)
    sums, bound, counts = ac.system(tm, ok, index, used, flat)
    return {"index": index, "terms": tm, "sums": sums, "bound": bound, "counts": counts}


def loop(rot, pos, pts, mode, max_dist, centre, damping, max_iters, eps_rot, eps_trans, cloud, huber=0.0, normal=None, nstatus=None, summation="fsum"):
    """the Loop rule over this rule's step -> dict: rot, pos, status, iterations, history (iterations, 4), rms; align_checker.loop with the
    correspondences and the terms of the Cloud rule in their place"""
    rot = np.eye(3) if rot is None else np.asarray(rot, np.float64).reshape(3, 3)
    pos = np.zeros(3) if pos is None else np.asarray(pos, np.float64).reshape(3)
    need = 6 if mode == PLANE else 3
    status, hist, rms, it = ac.MAX_ITERS, [], 0.0, 0
    for it in range(max_iters):
        p, ok, index, q = correspondences(rot, pos, pts, max_dist, cloud)
        tm, used, flat = terms(mode, p, centre, index, q, huber, normal, nstatus)
        sums = ac._sum(tm, summation)
        n_used = int(used.sum())
        rows = n_used if mode == PLANE else 3 * n_used
        rms = math.sqrt(sums[27] / rows) if rows > 0 else 0.0
        nw = nv = 0.0
        stop = False
        if n_used < need:
            status, stop = ac.TOO_FEW, True
        else:
            bad, delta = ac.solve(sums, damping)
            if bad:
                status, stop = ac.DEGENERATE, True
            else:
                rot, pos = ac.update(rot, pos, centre, delta)
                d = delta.tolist()
                nw = math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
                nv = math.sqrt((d[3] * d[3] + d[4] * d[4]) + d[5] * d[5])
                if nw <= eps_rot and nv <= eps_trans:
                    status, stop = ac.CONVERGED, True
        hist.append([float(n_used), rms, nw, nv])
        if stop:
            break
    return {"rot": rot, "pos": pos, "status": status, "iterations": it + 1 if max_iters > 0 else 0, "history": np.array(hist).reshape(-1, 4), "rms": rms}


# ---- the convergence case of the tests ------------------------------------------------------------------------------------------------------------
TRUE_ROT = ac.rodrigues([1.0, 2.0, 3.0], math.radians(0.5))
TRUE_POS = np.array([0.012, -0.008, 0.010])
SHEET_MAX_DIST = 0.25


def sheet_cloud(n=40, size=6.0, amp=0.3):
    """the bumpy sheet z = amp sin(x) cos(1.3 y) of align_checker as a cloud: its n x n vertices -> (n n, 3) float32 (spacing size / (n - 1))"""
    g = np.linspace(0.0, size, n)
    X, Y = np.meshgrid(g, g, indexing="ij")
    return np.stack([X, Y, amp * np.sin(X) * np.cos(1.3 * Y)], axis=-1).reshape(-1, 3).astype(np.float32)


def sheet_normals(n=40, size=6.0, amp=0.3):
    """the sheet's analytic unit normals at its vertices, as floats, and their status (all 0): what the checker's loop uses in PLANE mode where no
    device has made any -> (n n, 3) float32, (n n,) uint8"""
    g = np.linspace(0.0, size, n)
    X, Y = np.meshgrid(g, g, indexing="ij")
    nx, ny = -amp * np.cos(X) * np.cos(1.3 * Y), 1.3 * amp * np.sin(X) * np.sin(1.3 * Y)
    nrm = np.stack([nx, ny, np.ones_like(nx)], axis=-1).reshape(-1, 3)
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    return nrm.astype(np.float32), np.zeros(len(nrm), np.uint8)


def convergence_case(every=3):
    """the target sheet and a source that is every `every`-th point of it moved by the inverse of the known pose (TRUE_ROT, TRUE_POS) and rounded to
    float: at the true pose every source point's twin is its winner, so the optimum's residuals are the float rounding of the coordinates
    -> cloud (n, 3) float32, source (m, 3) float32, centre (3,)"""
    cloud = sheet_cloud()
    twin = cloud[::every].astype(np.float64)
    src = ((twin - TRUE_POS) @ TRUE_ROT).astype(np.float32)                                 # x = R^T (w - t): R x + t = w
    return cloud, src, twin.mean(axis=0)


def rms_bound(cloud, src):
    """4 * 2^-24 * max|coordinate|: the float rounding of the stored coordinates, which bounds the optimum's rms"""
    return 4.0 * 2.0 ** -24 * float(max(np.abs(cloud).max(), np.abs(src).max()))
