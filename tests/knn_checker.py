"""numpy restatement of the Neighbours, Count and Outliers rules of include/immesh_nearest.h by brute force: every query against every cloud point in
chunks, D in the contract's order, np.lexsort on (index, D), and plain sequential sums for mean, mu and sigma (no pairwise or compensated sum).
numpy does not fuse multiply-adds, so the results are bit-identical to the kernels'.  The Point rule is that of tests/closest_checker.py.
For clouds too large for that (the scale test alone), a candidate search with scipy's cKDTree whose candidates are re-measured exactly and which is
widened until the tree cannot have decided a tie (knn_tree, radius_count_tree)."""
import math

import numpy as np

import closest_checker as cc

points = cc.points
MAX_K = 64


def _live(cloud):
    cloud = np.asarray(cloud, np.float32).reshape(-1, 3)
    return cloud, np.nonzero(np.isfinite(cloud).all(axis=1))[0]                      # the points in the index


def pair_d(p, cT):
    """the D rule: queries p (m, 3) float64 x cloud points cT (3, L) float64 (floats widened) -> D (m, L)"""
    e = cT[0][None, :] - p[:, 0][:, None]
    D = e * e
    e = cT[1][None, :] - p[:, 1][:, None]
    D = D + e * e                                                                    # (e_x e_x + e_y e_y)
    e = cT[2][None, :] - p[:, 2][:, None]
    return D + e * e                                                                 # ... + e_z e_z


def exact_d(p, c32):
    """the D rule for lists: p (m, 3) float64, c32 (m, c, 3) float32 -> D (m, c)"""
    e = c32.astype(np.float64) - p[:, None, :]
    return (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]


def _chunks(idx, n_live, pairs_per_chunk):
    step = max(1, pairs_per_chunk // max(n_live, 1))
    return [idx[i:i + step] for i in range(0, len(idx), step)]


def _candidates(p, part, cT, live, r2, skip):
    """D (m, L) of a chunk of valid queries with +inf where the point is no candidate"""
    D = pair_d(p[part], cT)
    with np.errstate(invalid="ignore"):
        D = np.where(D <= r2, D, np.inf)
    if skip is not None:
        D[live[None, :] == skip[part][:, None]] = np.inf                             # the point with the query's own index
    return D


def knn(rot, pos, pts, k, max_dist, cloud, skip=None, pairs_per_chunk=1 << 21):
    """the Neighbours rule -> count (n,) int32, index (n, k) int32, d2 (n, k) float64; skip (n,): the index that is no candidate of each query"""
    assert 1 <= k <= MAX_K
    p, ok = points(rot, pos, pts)
    n = len(p)
    cloud, live = _live(cloud)
    r2 = float(max_dist) * float(max_dist)
    count, index, d2 = np.zeros(n, np.int32), np.full((n, k), -1, np.int32), np.full((n, k), -1.0)
    idx = np.nonzero(ok)[0]
    if len(idx) and len(live):
        cT = np.ascontiguousarray(cloud[live].astype(np.float64).T)
        cols = np.arange(len(live))
        for part in _chunks(idx, len(live), pairs_per_chunk):
            D = _candidates(p, part, cT, live, r2, skip)
            order = np.lexsort((np.broadcast_to(cols, D.shape), D), axis=1)[:, :k]       # ascending (D, index): the columns ascend with the index
            Ds = np.take_along_axis(D, order, axis=1)
            have = np.isfinite(Ds)
            kk = Ds.shape[1]
            count[part] = have.sum(axis=1)
            index[part, :kk] = np.where(have, live[order], -1)
            d2[part, :kk] = np.where(have, Ds, -1.0)
    return count, index, d2


def mean_of(count, d2):
    """the Neighbours rule's mean: the sequential sum of sqrt(d2_j) in list order over (double)count; -1 without a neighbour"""
    s = np.zeros(len(count))
    for j in range(d2.shape[1]):
        used = j < count
        s = np.where(used, s + np.sqrt(np.where(used, d2[:, j], 0.0)), s)
    return np.where(count > 0, s / np.maximum(count, 1).astype(np.float64), -1.0)


def knn_cloud(cloud, k, max_dist, **kw):
    """cloud mode -> count, index, d2, mean: query i is cloud point i, and index i is no candidate"""
    cloud = np.asarray(cloud, np.float32).reshape(-1, 3)
    count, index, d2 = knn(None, None, cloud, k, max_dist, cloud, skip=np.arange(len(cloud)), **kw)
    return count, index, d2, mean_of(count, d2)


def radius_count(rot, pos, pts, radius, cloud, skip=None, pairs_per_chunk=1 << 21):
    """the Count rule -> (n,) int32"""
    p, ok = points(rot, pos, pts)
    cloud, live = _live(cloud)
    r2 = float(radius) * float(radius)
    count = np.zeros(len(p), np.int32)
    idx = np.nonzero(ok)[0]
    if len(idx) and len(live):
        cT = np.ascontiguousarray(cloud[live].astype(np.float64).T)
        for part in _chunks(idx, len(live), pairs_per_chunk):
            count[part] = np.isfinite(_candidates(p, part, cT, live, r2, skip)).sum(axis=1)
    return count


def radius_count_cloud(cloud, radius, **kw):
    cloud = np.asarray(cloud, np.float32).reshape(-1, 3)
    return radius_count(None, None, cloud, radius, cloud, skip=np.arange(len(cloud)), **kw)


# ---- the Outliers rule ---------------------------------------------------------------------------------------------------------------------------
def statistical(mean, count, finite, mult):
    """-> dict: mu, sigma, threshold, keep (n,) bool, kept, outliers, isolated, not_finite; the sums are plain left-to-right Python sums"""
    used = np.asarray(count) > 0
    vals = [float(v) for v in np.asarray(mean, np.float64)[used]]                    # ascending i
    n_used = len(vals)
    total = 0.0
    for v in vals:
        total = total + v
    mu = total / float(n_used) if n_used else 0.0
    sq = 0.0
    for v in vals:
        t = v - mu
        sq = sq + t * t
    sigma = math.sqrt(sq / float(n_used - 1)) if n_used > 1 else 0.0
    threshold = mu + float(mult) * sigma
    keep = used & (np.asarray(mean, np.float64) <= threshold)
    finite = np.asarray(finite, bool)
    return dict(mu=mu, sigma=sigma, threshold=threshold, keep=keep, kept=int(keep.sum()), outliers=int((used & ~keep).sum()),
                isolated=int((finite & ~used).sum()), not_finite=int((~finite).sum()))


def radius_rule(count, finite, min_neighbours):
    """-> dict: keep (n,) bool, kept, outliers (finite, not kept), isolated (finite, count == 0), not_finite"""
    finite = np.asarray(finite, bool)
    count = np.asarray(count, np.int64)
    keep = finite & (count >= int(min_neighbours))
    return dict(keep=keep, kept=int(keep.sum()), outliers=int((finite & ~keep).sum()), isolated=int((finite & (count == 0)).sum()),
                not_finite=int((~finite).sum()))


# ---- the scale test's candidate search -------------------------------------------------------------------------------------------------------------
def knn_tree(pts, k, max_dist, cloud, skip=None, extra=8):
    """the Neighbours rule for world queries with a cKDTree to find candidates: k + extra (+ 1 for the skipped index) nearest by the tree, every D
    re-measured in the contract's order and sorted by (D, index).  Where the search was cut off, the farthest candidate's exact D must lie strictly
    above the k-th D (or above r2 when fewer than k count): then every point the tree left out lies strictly beyond the list, and the tree has
    decided no tie.  Rows where that does not hold are searched again with twice the candidates."""
    from scipy.spatial import cKDTree
    p, ok = points(None, None, pts)
    n = len(p)
    cloud, live = _live(cloud)
    r2 = float(max_dist) * float(max_dist)
    count, index, d2 = np.zeros(n, np.int32), np.full((n, k), -1, np.int32), np.full((n, k), -1.0)
    if not len(live):
        return count, index, d2
    tree = cKDTree(cloud[live].astype(np.float64))
    todo = np.nonzero(ok)[0]
    m = min(len(live), k + extra + (skip is not None))
    while len(todo):
        _, at = tree.query(p[todo], k=m, workers=-1)
        at = at.reshape(len(todo), -1)
        cand = live[at]                                                              # (m == n_live: every point is a candidate, nothing is cut off)
        D = exact_d(p[todo], cloud[cand])
        far = D.max(axis=1)
        D = np.where(D <= r2, D, np.inf)
        if skip is not None:
            D[cand == skip[todo][:, None]] = np.inf
        order = np.lexsort((cand, D), axis=1)
        Ds, ids = np.take_along_axis(D, order, axis=1)[:, :k], np.take_along_axis(cand, order, axis=1)[:, :k]
        have = np.isfinite(Ds)
        full = have.sum(axis=1) == k
        bound = np.where(full, Ds[:, -1], r2)                                        # the k-th D, or r2 while fewer than k count
        settled = (far > bound) if m < len(live) else np.ones(len(todo), bool)       # (every point a candidate: nothing was left out)
        assert m == len(live) or (far[settled] > bound[settled]).all()               # the tree decided no tie in the rows that are taken
        rows = todo[settled]
        kk = Ds.shape[1]
        count[rows] = have[settled].sum(axis=1)
        index[rows, :kk] = np.where(have[settled], ids[settled], -1)
        d2[rows, :kk] = np.where(have[settled], Ds[settled], -1.0)
        todo = todo[~settled]
        m = min(len(live), 2 * m)
    return count, index, d2


def radius_count_tree(pts, radius, cloud, skip=None, slack=1e-9):
    """the Count rule for world queries: cKDTree.query_ball_point lengths just inside and just outside the radius; where the two differ (a point at
    the boundary, where the tree's arithmetic could decide) the exact D of every point of the larger ball is re-measured"""
    from scipy.spatial import cKDTree
    p, ok = points(None, None, pts)
    cloud, live = _live(cloud)
    r2 = float(radius) * float(radius)
    count = np.zeros(len(p), np.int32)
    idx = np.nonzero(ok)[0]
    if not len(live) or not len(idx):
        return count
    tree = cKDTree(cloud[live].astype(np.float64))
    inner = tree.query_ball_point(p[idx], radius * (1.0 - slack), return_length=True, workers=-1)
    outer = tree.query_ball_point(p[idx], radius * (1.0 + slack), return_length=True, workers=-1)
    if skip is not None:                                                             # the query's own point lies in both balls (D = 0)
        own = np.isin(skip[idx], live)
        inner, outer = inner - own, outer - own
    count[idx] = inner
    for row in np.nonzero(inner != outer)[0]:
        i = idx[row]
        cand = live[tree.query_ball_point(p[i], radius * (1.0 + slack))]
        D = exact_d(p[i:i + 1], cloud[cand][None])[0]
        count[i] = int(((D <= r2) & ((cand != skip[i]) if skip is not None else True)).sum())
    return count
