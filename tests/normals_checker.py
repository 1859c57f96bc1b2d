"""numpy restatement of the Normals and Agreement rules of include/immesh_normals.h.  The neighbourhoods come from tests/knn_checker.py (knn_cloud by
brute force, or any (count, index) lists the caller gives: knn_tree's for the scale test, the device's own for the cross-check); the sums over a list
are sequential, in list order, vectorised over the points (column j of every list at a time); the cyclic Jacobi is vectorised over the points with
both branches of every step computed and chosen by np.where, so that every point sees exactly the scalar code's operations.  numpy does not fuse
multiply-adds, so the results are bit-identical to the kernels'.  The closest faces of the cloud direction come from tests/closest_checker.py."""
import numpy as np

import closest_checker as cc
import knn_checker as kc

NAN32 = cc.NAN32
CANONICAL, VIEWPOINT = 0, 1
PAIRS = (0, 1), (0, 2), (1, 2)                                                       # a sweep's order; the third position is 2, 1, 0


def jacobi(C6):
    """the Eigen step: C6 (n, 6) float64 = xx, xy, xz, yy, yz, zz -> lam (n, 3) by diagonal position, V (n, 3, 3) with V[:, i, j] row i, column j,
    sweeps (n,) the sweeps that rotated"""
    C6 = np.asarray(C6, np.float64).reshape(-1, 6)
    n = len(C6)
    A = {(0, 0): C6[:, 0].copy(), (0, 1): C6[:, 1].copy(), (0, 2): C6[:, 2].copy(), (1, 1): C6[:, 3].copy(), (1, 2): C6[:, 4].copy(), (2, 2): C6[:, 5].copy()}
    V = np.zeros((n, 3, 3))
    V[:, 0, 0] = V[:, 1, 1] = V[:, 2, 2] = 1.0
    sweeps = np.zeros(n, np.int32)
    with np.errstate(all="ignore"):
        for _ in range(64):
            rotated = np.zeros(n, bool)
            for p, q in PAIRS:
                r = 3 - p - q
                rp, rq = (min(r, p), max(r, p)), (min(r, q), max(r, q))
                app, aqq, apq, arp, arq = A[(p, p)], A[(q, q)], A[(p, q)], A[rp], A[rq]
                nz = apq != 0.0
                small = (np.abs(apq) <= 1e-300) | ((np.abs(app) + np.abs(apq) == np.abs(app)) & (np.abs(aqq) + np.abs(apq) == np.abs(aqq)))
                rot = nz & ~small
                theta = (aqq - app) / np.where(rot, 2.0 * apq, 1.0)
                t = np.where(theta >= 0.0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                A[(p, p)] = np.where(rot, app - t * apq, app)
                A[(q, q)] = np.where(rot, aqq + t * apq, aqq)
                A[rp] = np.where(rot, c * arp - s * arq, arp)
                A[rq] = np.where(rot, s * arp + c * arq, arq)
                A[(p, q)] = np.where(nz, 0.0, apq)
                vp, vq = V[:, :, p].copy(), V[:, :, q].copy()
                V[:, :, p] = np.where(rot[:, None], c[:, None] * vp - s[:, None] * vq, vp)
                V[:, :, q] = np.where(rot[:, None], s[:, None] * vp + c[:, None] * vq, vq)
                rotated |= rot
            sweeps += rotated
            if not rotated.any():                                                    # (a point whose sweep did not rotate has three zero off-diagonals:
                break                                                                #  the later sweeps of the others leave it as it is)
    return np.stack([A[(0, 0)], A[(1, 1)], A[(2, 2)]], axis=1), V, sweeps


def covariance(cloud, count, index):
    """the Offsets, Mean and Covariance steps for every point with count >= 2 (zeros elsewhere) -> C6 (n, 6)"""
    cloud = np.asarray(cloud, np.float32).reshape(-1, 3)
    n = len(cloud)
    count = np.asarray(count, np.int64)
    index = np.asarray(index, np.int64)
    index = index.reshape(n, index.size // n if n else 0)
    take = np.isfinite(cloud).all(axis=1) & (count >= 2)
    p = np.where(take[:, None], cloud.astype(np.float64), 0.0)
    m = (count + 1).astype(np.float64)
    with np.errstate(all="ignore"):
        q = []
        for j in range(index.shape[1]):
            used = take & (j < count)
            if not used.any():
                break
            c = cloud[np.where(used, index[:, j], 0)].astype(np.float64)
            q.append((used, np.where(used[:, None], c - p, 0.0)))
        S = np.zeros((n, 3))
        for used, qj in q:
            S = np.where(used[:, None], S + qj, S)
        g = S / m[:, None]
        r = 0.0 - g
        ab = (0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)
        T = np.stack([r[:, a] * r[:, b] for a, b in ab], axis=1)
        for used, qj in q:
            r = qj - g
            T = np.where(used[:, None], T + np.stack([r[:, a] * r[:, b] for a, b in ab], axis=1), T)
        C6 = T / m[:, None]
    return np.where(take[:, None], C6, 0.0)


def normals(cloud, k, max_dist, min_ratio=0.0, mode=CANONICAL, viewpoint=None, lists=None):
    """the Normals rule -> dict: normal (n, 3) float32, curvature (n,) float64, eig (n, 3) float64, count (n,) int32, status (n,) uint8, counts
    (4,) int64, sweeps (n,); lists: (count, index) under the Neighbours rule in cloud mode, made by knn_checker.knn_cloud when None"""
    assert 2 <= k <= 64 and 0.0 <= min_ratio < 1.0
    cloud = np.asarray(cloud, np.float32).reshape(-1, 3)
    n = len(cloud)
    if lists is None:
        lists = kc.knn_cloud(cloud, k, max_dist)[:2]
    count, index = np.asarray(lists[0], np.int32), np.asarray(lists[1])
    ok = np.isfinite(cloud).all(axis=1)
    lam, V, sweeps = jacobi(covariance(cloud, count, index))
    rows = np.arange(n)
    s = np.zeros(n, np.int64)
    s = np.where(lam[:, 1] < lam[rows, s], 1, s)
    s = np.where(lam[:, 2] < lam[rows, s], 2, s)
    o0, o1 = np.where(s == 0, 1, 0), np.where(s == 2, 1, 2)
    hi = np.where(lam[rows, o1] > lam[rows, o0], o1, o0)
    mid = np.where(hi == o0, o1, o0)
    eig = np.stack([lam[rows, s], lam[rows, mid], lam[rows, hi]], axis=1)
    total = (lam[:, 0] + lam[:, 1]) + lam[:, 2]
    with np.errstate(all="ignore"):
        curv = np.where(total > 0.0, eig[:, 0] / np.where(total > 0.0, total, 1.0), 0.0)
        line = ~(eig[:, 1] > float(min_ratio) * eig[:, 2])
    status = np.where(~ok, 2, np.where(count < 2, 1, np.where(line, 3, 0))).astype(np.uint8)
    u = V[rows, :, s]                                                                # column s
    big = np.zeros(n, np.int64)
    big = np.where(np.abs(u[:, 1]) > np.abs(u[rows, big]), 1, big)
    big = np.where(np.abs(u[:, 2]) > np.abs(u[rows, big]), 2, big)
    u = np.where((u[rows, big] < 0.0)[:, None], -u, u)
    if mode == VIEWPOINT:
        w = np.asarray(viewpoint, np.float64).reshape(1, 3) - np.where(ok[:, None], cloud.astype(np.float64), 0.0)
        t = (u[:, 0] * w[:, 0] + u[:, 1] * w[:, 1]) + u[:, 2] * w[:, 2]
        u = np.where((t < 0.0)[:, None], -u, u)
    length = np.sqrt((u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1]) + u[:, 2] * u[:, 2])
    normal = np.where((status == 0)[:, None], (u / length[:, None]).astype(np.float32), NAN32).astype(np.float32)
    given = (status == 0) | (status == 3)
    eig = np.where(given[:, None], eig, -1.0)
    curv = np.where(given, curv, -1.0)
    counts = np.array([(status == 0).sum(), (status == 1).sum(), (status == 3).sum(), (status == 2).sum()], np.int64)
    return dict(normal=normal, curvature=curv, eig=eig, count=count.copy(), status=status, counts=counts, sweeps=sweeps)


# ---- the Agreement rule --------------------------------------------------------------------------------------------------------------------------
def face_normals(vtx, faces):
    """the Face step -> cr (m, 3) float64, l2 (m,), part (m,) bool: the face takes part"""
    vtx = np.asarray(vtx, np.float32).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    in_range = ((faces >= 0) & (faces < len(vtx))).all(axis=1)
    P = vtx[np.where(in_range[:, None], faces, 0)].astype(np.float64) if len(vtx) else np.zeros((len(faces), 3, 3))
    with np.errstate(all="ignore"):
        cr = cc._cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
        l2 = cc._dot(cr, cr)
        part = in_range & np.isfinite(P).all(axis=(1, 2)) & np.isfinite(l2) & (l2 > 0.0)
    return cr, l2, part


def _agree(pair, face, normal_of, cr, l2, not_finite):
    """the Value step over the items with a pair -> agree (n,) float32, pair, counts (4,) int64"""
    f = np.where(pair, face, 0)
    nn = np.where(pair[:, None], normal_of, 0.0).astype(np.float64)
    with np.errstate(all="ignore"):
        s = cc._dot(cr[f], nn) / np.sqrt(np.where(pair, l2[f], 1.0)) if len(cr) else np.zeros(len(pair))
    agree = np.where(pair, s.astype(np.float32), NAN32).astype(np.float32)
    counts = np.array([pair.sum(), (pair & (s < 0.0)).sum(), (~pair & ~not_finite).sum(), not_finite.sum()], np.int64)
    return agree, pair, counts


def agree_samples(sample_face, index, normal, status, vtx, faces):
    """samples direction: the samples' faces, the nearest query's index_out, the cloud's normals and statuses -> agree, pair, counts"""
    sample_face, index = np.asarray(sample_face, np.int64), np.asarray(index, np.int64)
    cr, l2, part = face_normals(vtx, faces)
    at = np.where(index >= 0, index, 0)
    pair = (index >= 0) & (np.asarray(status)[at] == 0 if len(status) else False) & (part[sample_face] if len(part) else False)
    pair = np.broadcast_to(pair, sample_face.shape).copy()
    return _agree(pair, sample_face, np.asarray(normal, np.float32).reshape(-1, 3)[at] if len(status) else np.zeros((len(at), 3)), cr, l2,
                  np.zeros(len(sample_face), bool))


def agree_cloud(cloud, normal, status, max_dist, vtx, faces):
    """cloud direction -> agree, face (n,) int32, pair, counts; the closest faces by brute force (closest_checker.closest) over the points with a normal"""
    cloud = np.asarray(cloud, np.float32).reshape(-1, 3)
    status = np.asarray(status)
    cr, l2, part = face_normals(vtx, faces)
    face = np.full(len(cloud), -1, np.int32)
    has = np.nonzero(status == 0)[0]
    if len(has):
        face[has] = cc.closest(None, None, cloud[has], max_dist, vtx, faces)[2]
    pair = (face >= 0) & (part[np.where(face >= 0, face, 0)] if len(part) else False)
    pair = np.broadcast_to(pair, face.shape).copy()
    agree, pair, counts = _agree(pair, face.astype(np.int64), np.asarray(normal, np.float32).reshape(-1, 3), cr, l2, status == 2)
    return agree, face, pair, counts


def agree_stats(agree, pair, not_finite, bin_width, n_bins):
    """the Reduce step: closest_checker.stats over dist = |agree| of the pairs -> dict, hist"""
    n = len(agree)
    pts = np.zeros((n, 3), np.float32)
    pts[np.asarray(not_finite, bool)] = np.nan                                        # (the Stats rule counts a point that is not finite by its floats)
    dist = np.where(pair, np.abs(np.where(pair, agree, np.float32(0))), np.float32(-1)).astype(np.float32)
    return cc.stats(None, None, pts, dist, np.where(pair, 0, -1), bin_width, n_bins)
