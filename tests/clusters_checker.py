"""numpy restatement of the Clusters rule of include/immesh_nearest.h by brute force, on the arithmetic of tests/knn_checker.py (pair_d / exact_d: D in
the contract's order, nothing fused): the full D matrix of the indexed points, the candidates D <= r2 off the diagonal, the counts, the core points, the
classes of the core points by min-label propagation with pointer jumping (plain numpy), the numbering by smallest core index, the border points'
smallest core candidate under (D, index), the table and the Select rule.
For clouds too large for a full matrix (the scale test, the deep chains), the candidates come from scipy's cKDTree.query_pairs at a radius widened by a
slack, EVERY pair re-measured exactly and kept only where D <= r2 (the tree's own arithmetic decides nothing), and the classes from
scipy.sparse.csgraph.connected_components.  Both paths share everything behind the candidate list."""
import numpy as np

import knn_checker as kc

KINDS = ("core", "border", "noise", "not_finite")


def _pairs_brute(cloud, live, r2):
    c64 = cloud[live].astype(np.float64)
    D = kc.pair_d(c64, np.ascontiguousarray(c64.T))                                   # (L, L): row i is query i
    assert D.tobytes() == np.ascontiguousarray(D.T).tobytes()                        # symmetric bit for bit (the contract says so)
    A = D <= r2
    np.fill_diagonal(A, False)                                                       # the point with the query's own index is no candidate
    si, di = np.nonzero(A)
    return live[si], live[di], D[si, di]


def _pairs_tree(cloud, live, radius, r2, slack=1e-6):
    from scipy.spatial import cKDTree
    if len(live) < 2:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0)
    tree = cKDTree(cloud[live].astype(np.float64))
    pr = tree.query_pairs(radius * (1.0 + slack), output_type="ndarray")             # i < j, each once
    a, b = live[pr[:, 0]], live[pr[:, 1]]
    D = kc.exact_d(cloud[a].astype(np.float64), cloud[b][:, None, :])[:, 0]          # every pair re-measured in the contract's order
    ok = D <= r2
    a, b, D = a[ok], b[ok], D[ok]
    return np.concatenate([a, b]), np.concatenate([b, a]), np.concatenate([D, D])    # both directions: D is symmetric bit for bit


def _classes_numpy(n, core, a, b):
    """root (n,) int64: the smallest index of each core point's class over the edges a - b (both directions given), -1 for the others"""
    root = np.where(core, np.arange(n), -1)
    if not len(a):
        return root
    order = np.argsort(a, kind="stable")
    a, b = a[order], b[order]
    starts = np.nonzero(np.r_[True, a[1:] != a[:-1]])[0]
    rows = a[starts]
    while True:
        new = root.copy()
        new[rows] = np.minimum(root[rows], np.minimum.reduceat(root[b], starts))     # the smallest label among a point and its neighbours
        idx = np.nonzero(core)[0]
        new[idx] = new[new[idx]]                                                     # pointer jumping
        if np.array_equal(new, root):
            return root
        root = new


def _classes_scipy(n, core, a, b):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    if not core.any():
        return np.full(n, -1, np.int64)
    _, comp = connected_components(coo_matrix((np.ones(len(a), np.int8), (a, b)), shape=(n, n)), directed=False)
    idx = np.nonzero(core)[0]
    low = np.full(comp.max() + 1 if n else 0, n, np.int64)
    np.minimum.at(low, comp[idx], idx)
    root = np.full(n, -1, np.int64)
    root[idx] = low[comp[idx]]
    return root


def _finish(cloud, finite, min_neighbours, src, dst, D, classes):
    n = len(cloud)
    count = np.bincount(src, minlength=n)
    core = finite & (count >= int(min_neighbours))
    both = core[src] & core[dst]
    root = classes(n, core, src[both], dst[both])
    kind = np.where(~finite, 3, np.where(core, 0, 2)).astype(np.uint8)
    cand = ~core[src] & core[dst]                                                    # a border point's core candidates
    s, d, dd = src[cand], dst[cand], D[cand]
    order = np.lexsort((d, dd, s))                                                   # per point ascending (D, index)
    s, d = s[order], d[order]
    if len(s):
        head = np.r_[True, s[1:] != s[:-1]]
        kind[s[head]] = 1
        root[s[head]] = root[d[head]]
    labels = np.unique(root[core])                                                   # ascending: the clusters' numbers
    assert (root[labels] == labels).all()
    label = np.where(root >= 0, np.searchsorted(labels, np.maximum(root, 0)), -1).astype(np.int32)
    nc = len(labels)
    member = label >= 0
    box = np.zeros((nc, 6), np.float32)
    if nc:
        lo, hi = np.full((nc, 3), np.inf, np.float32), np.full((nc, 3), -np.inf, np.float32)
        np.minimum.at(lo, label[member], cloud[member])
        np.maximum.at(hi, label[member], cloud[member])
        box = np.concatenate([lo, hi], axis=1)
    return dict(label=label, kind=kind, count=count.astype(np.int32), counts=[int((kind == k).sum()) for k in range(4)], n_clusters=nc,
                first=labels.astype(np.int32), n_points=np.bincount(label[member], minlength=nc).astype(np.int32),
                n_core=np.bincount(label[member & core], minlength=nc).astype(np.int32), box=box)


def clusters(cloud, radius, min_neighbours):
    """the Clusters rule by brute force -> dict: label (n,) int32, kind (n,) uint8, count (n,) int32, counts [core, border, noise, not finite],
    n_clusters, and the table first / n_points / n_core (n_clusters,) int32, box (n_clusters, 6) float32"""
    cloud, live = kc._live(cloud)
    finite = np.isfinite(cloud).all(axis=1)
    src, dst, D = _pairs_brute(cloud, live, float(radius) * float(radius))
    return _finish(cloud, finite, min_neighbours, src, dst, D, _classes_numpy)


def clusters_tree(cloud, radius, min_neighbours):
    """the same with the tree-assisted candidate search and scipy's connected components"""
    cloud, live = kc._live(cloud)
    finite = np.isfinite(cloud).all(axis=1)
    src, dst, D = _pairs_tree(cloud, live, float(radius), float(radius) * float(radius))
    return _finish(cloud, finite, min_neighbours, src, dst, D, _classes_scipy)


def select(ref, min_points=0, max_points=0, keep_largest=0, keep_noise=0):
    """the Select rule over a result of clusters() -> dict: keep (n,) bool, keepc (n_clusters,) bool, counts [kept, in a cluster and not kept,
    noise and not kept, not finite]"""
    npts = ref["n_points"].astype(np.int64)
    keepc = (npts >= int(min_points)) & ((int(max_points) == 0) | (npts <= int(max_points)))
    if int(keep_largest) > 0:
        rank = np.lexsort((np.arange(len(npts)), -npts))                             # most points first, ties to the smaller number, over ALL clusters
        top = np.zeros(len(npts), bool)
        top[rank[:int(keep_largest)]] = True
        keepc &= top
    label, kind = ref["label"], ref["kind"]
    member = label >= 0
    keep = np.zeros(len(label), bool)
    keep[member] = keepc[label[member]]
    if keep_noise:
        keep |= kind == 2
    return dict(keep=keep, keepc=keepc, counts=[int(keep.sum()), int((member & ~keep).sum()), int(((kind == 2) & ~keep).sum()), int((kind == 3).sum())])


def same_partition(label_a, label_b):
    """two labellings give the same partition (noise, -1, matching noise)"""
    a, b = np.asarray(label_a, np.int64), np.asarray(label_b, np.int64)
    if not np.array_equal(a < 0, b < 0):
        return False
    m = a >= 0
    pairs = np.unique(np.stack([a[m], b[m]], axis=1), axis=0)
    return len(pairs) == len(np.unique(a[m])) == len(np.unique(b[m]))
