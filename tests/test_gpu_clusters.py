"""Euclidean clusters of the indexed cloud on the device (include/immesh_nearest.h, the Clusters rule) against the brute-force numpy restatement
(tests/clusters_checker.py), bit for bit: tree sizes at which the build and the walk change path, the single-leaf tree, the distance boundary, deep
chains in three index orders, the border rules on an integer lattice, coincident points, cross-checks against the radius rule and under a permutation
of the rows, the planted scene's figures, select and apply, argument errors, state left over from a larger call, scale, the live path without side
effects, and tools/mesh_eval.py's filter."""
import ctypes as C

import numpy as np
import pytest

import clusters_checker as cl
import knn_checker as kc
from immesh_amd import capi, synth
from conftest import make_hip
from parity_utils import compare_plane_tables_fast
from test_clusters_cpu import BRIDGE_ORDERS, two_blobs_and_a_bridge
from test_gpu_knn import _sized_cloud
from test_gpu_nearest import _cloud, _err
from test_gpu_render import _small_cfg
from test_knn_cpu import sheet_with_strays

pytestmark = pytest.mark.gpu
E_INVAL, E_CAPACITY = -1, -4
COUNTS = ("core", "border", "noise", "not_finite")


@pytest.fixture(scope="module")
def hp():
    h = make_hip(capi.load_hip_library(), _small_cfg())
    yield h
    h.close()


def _run(h, radius, min_neighbours):
    """clusters and their table off the device in the checker's shape"""
    got = h.cloud_clusters(radius, min_neighbours)
    got["counts"] = [got["counts"][k] for k in COUNTS]
    got.update(h.cloud_clusters_table())
    return got


def _same(got, ref, what):
    """device dict == checker dict: the integers bit for bit, the boxes as values (the sign of a zero is not part of the contract)"""
    assert got["n_clusters"] == ref["n_clusters"] and got["counts"] == ref["counts"], (what, got["n_clusters"], ref["n_clusters"], got["counts"], ref["counts"])
    assert sum(got["counts"]) == len(ref["label"]), what
    for key in ("label", "kind", "first", "n_points", "n_core"):
        g, r = got[key], ref[key]
        assert g.dtype == r.dtype and g.shape == r.shape, (what, key, g.dtype, r.dtype, g.shape, r.shape)
        diff = np.nonzero(g != r)[0]
        assert len(diff) == 0, (what, key, len(diff), len(g), diff[:5].tolist(), g[diff[:5]].tolist(), r[diff[:5]].tolist())
    assert got["box"].dtype == np.float32 and got["box"].shape == ref["box"].shape and np.array_equal(got["box"], ref["box"]), (what, "box")


def _line(n):
    line = np.zeros((n, 3), np.float32)
    line[:, 0] = np.arange(n)
    return line


# ---- sizes -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_in", [0, 1, 2, 3, 63, 64, 65, 257])
def test_sizes_match_checker(hp, n_in):
    rng = np.random.default_rng(1900 + n_in)
    cloud = _sized_cloud(rng, n_in)
    assert hp.cloud_index_build(cloud) == (len(cloud), n_in)
    for radius in (1.5, 100.0):
        for min_nb in (0, 1, 3, 10 ** 6):
            ref = cl.clusters(cloud, radius, min_nb)
            _same(_run(hp, radius, min_nb), ref, (n_in, radius, min_nb))
            if min_nb == 10 ** 6:
                assert ref["n_clusters"] == 0 and ref["counts"][2] == n_in
            if radius == 100.0 and min_nb == 0 and n_in:
                assert ref["n_clusters"] == 1 and ref["n_points"].tolist() == [n_in]


def test_single_leaf_tree(hp):
    """the tree of one point names it as both children of the root: it is offered once and is a cluster of one, or noise"""
    cloud = np.array([[np.nan, 0, 0], [1, 2, 3]], np.float32)
    assert hp.cloud_index_build(cloud) == (2, 1)
    got = _run(hp, 2.0, 0)
    assert got["label"].tolist() == [-1, 0] and got["kind"].tolist() == [3, 0] and got["counts"] == [1, 0, 0, 1] and got["n_clusters"] == 1
    assert got["first"].tolist() == [1] and got["n_points"].tolist() == [1] and got["n_core"].tolist() == [1] and got["box"].tolist() == [[1, 2, 3, 1, 2, 3]]
    got = _run(hp, 2.0, 1)
    assert got["label"].tolist() == [-1, -1] and got["kind"].tolist() == [3, 2] and got["counts"] == [0, 0, 1, 1] and got["n_clusters"] == 0
    assert got["box"].shape == (0, 6)
    hp.cloud_index_build(np.zeros((0, 3), np.float32))                               # an empty index: zero clusters, no error
    got = _run(hp, 2.0, 0)
    assert got["n_clusters"] == 0 and got["counts"] == [0, 0, 0, 0] and got["label"].shape == (0,)
    assert hp.cloud_clusters_select()["keep"].shape == (0,) and len(hp.cloud_index_apply_outliers()) == 0


# ---- the boundary --------------------------------------------------------------------------------------------------------------------------------
def test_distance_boundary(hp):
    n = 40
    line = _line(n)
    hp.cloud_index_build(line)
    got = _run(hp, 1.0, 0)                                                           # D == r2 is a candidate
    assert got["n_clusters"] == 1 and got["label"].tolist() == [0] * n and got["box"].tolist() == [[0, 0, 0, n - 1, 0, 0]]
    _same(got, cl.clusters(line, 1.0, 0), "D == r2")
    below = np.nextafter(1.0, 0.0)
    got = _run(hp, below, 0)
    assert got["n_clusters"] == n and got["label"].tolist() == list(range(n)) and got["n_points"].tolist() == [1] * n
    _same(got, cl.clusters(line, below, 0), "below, 0")
    got = _run(hp, below, 1)
    assert got["n_clusters"] == 0 and got["counts"] == [0, 0, n, 0] and (got["label"] == -1).all()
    _same(got, cl.clusters(line, below, 1), "below, 1")
    _same(_run(hp, 1.0, 2), cl.clusters(line, 1.0, 2), "the ends are border points")


# ---- deep chains ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["ascending", "descending", "shuffled"])
def test_deep_chains(hp, order):
    """5000 collinear points 1.0 apart: one class through 4999 joins, whatever the index order; the unions stay within their step bound"""
    n = 5000
    idx = {"ascending": np.arange(n), "descending": np.arange(n)[::-1], "shuffled": np.random.default_rng(17).permutation(n)}[order]
    line = _line(n)[idx]
    hp.cloud_index_build(line)
    got = _run(hp, 1.0, 0)                                                           # (IMMESH_E_INTERNAL would raise)
    assert got["n_clusters"] == 1 and (got["label"] == 0).all() and (got["kind"] == 0).all() and got["counts"] == [n, 0, 0, 0]
    assert got["first"].tolist() == [0] and got["n_points"].tolist() == [n] and got["n_core"].tolist() == [n] and got["box"].tolist() == [[0, 0, 0, n - 1, 0, 0]]
    got = _run(hp, 1.0, 2)                                                           # the two ends have one neighbour each
    ends = sorted(int(np.nonzero(idx == e)[0][0]) for e in (0, n - 1))
    assert got["n_clusters"] == 1 and got["counts"] == [n - 2, 2, 0, 0] and np.nonzero(got["kind"] == 1)[0].tolist() == ends and (got["label"] == 0).all()
    assert got["first"].tolist() == [int(np.nonzero(got["kind"] == 0)[0][0])] and got["n_points"].tolist() == [n] and got["n_core"].tolist() == [n - 2]
    _same(got, cl.clusters_tree(line, 1.0, 2), order)


# ---- the border rules ------------------------------------------------------------------------------------------------------------------------------
def test_border_rules(hp):
    cloud, is_a, is_b, is_bridge, is_far = two_blobs_and_a_bridge((3, 1, 0), 5)
    hp.cloud_index_build(cloud)
    ref = cl.clusters(cloud, 2.0, 9)
    assert ref["n_clusters"] == 2 and ref["kind"][is_bridge].tolist() == [1] and ref["label"][is_bridge].tolist() == [0]      # the checker first: the nearer blob
    assert ref["kind"][is_far].tolist() == [2, 2]                                    # candidates, but none that is core: noise
    _same(_run(hp, 2.0, 9), ref, "bridge, nearer")
    _same(_run(hp, 2.0, 8), cl.clusters(cloud, 2.0, 8), "bridge, core")              # a core bridge joins the two
    holders = set()
    for k, order in enumerate(BRIDGE_ORDERS):
        cloud, is_a, is_b, is_bridge, is_far = two_blobs_and_a_bridge((4, 1, 0), 6, order)
        hp.cloud_index_build(cloud)
        ref = cl.clusters(cloud, 2.0, 9)
        ends = [int(np.nonzero((cloud == np.array(p, np.float32)).all(axis=1))[0][0]) for p in ((2, 1, 0), (6, 1, 0))]
        assert ref["n_clusters"] == 2 and ref["label"][is_bridge][0] == ref["label"][min(ends)]
        holders.add(bool(is_a[min(ends)]))
        got = _run(hp, 2.0, 9)
        _same(got, ref, ("bridge, tie", k))
        assert got["label"][is_bridge][0] == got["label"][min(ends)] and got["kind"][is_bridge].tolist() == [1]
    assert holders == {True, False}


# ---- coincident points -------------------------------------------------------------------------------------------------------------------------------
def test_coincident_points(hp):
    cloud = np.concatenate([np.tile(np.array([[1.5, -2, 3]], np.float32), (5, 1)), np.tile(np.array([[1.5, -2, 3.5]], np.float32), (70, 1))])
    hp.cloud_index_build(cloud)
    for radius, min_nb in ((0.25, 0), (0.25, 4), (0.25, 5), (0.25, 69), (0.25, 70), (0.5, 0), (0.5, 74), (0.5, 75), (1e-3, 1)):
        _same(_run(hp, radius, min_nb), cl.clusters(cloud, radius, min_nb), ("coincident", radius, min_nb))
    got = _run(hp, 0.25, 5)                                                          # the five have four others each: noise; the seventy are one cluster
    assert got["counts"] == [70, 0, 5, 0] and got["first"].tolist() == [5] and got["box"].tolist() == [[1.5, -2, 3.5, 1.5, -2, 3.5]]
    got = _run(hp, 0.5, 70)                                                          # 74 others within 0.5 of everyone
    assert got["n_clusters"] == 1 and got["counts"] == [75, 0, 0, 0] and got["box"].tolist() == [[1.5, -2, 3, 1.5, -2, 3.5]]


# ---- cross-checks ----------------------------------------------------------------------------------------------------------------------------------
def test_cross_checks(hp):
    rng = np.random.default_rng(62)
    cloud = _cloud(rng, 3000)
    cloud[200:220] = cloud[100:120]                                                  # coincident pairs
    fin = np.isfinite(cloud).all(axis=1)
    hp.cloud_index_build(cloud)
    count = hp.radius_count_cloud(0.7)
    # plain extraction: a cluster of two or more is a point with a neighbour
    got = _run(hp, 0.7, 0)
    _same(got, cl.clusters(cloud, 0.7, 0), "extraction")
    sel = hp.cloud_clusters_select(min_points=2)
    hp.radius_count_cloud(0.7)
    rule = hp.cloud_outliers_radius(1)
    assert np.array_equal(sel["keep"], rule["keep"]) and sel["kept"] == rule["kept"] and 100 < sel["kept"] < fin.sum() - 10
    # core exactly where the Count rule says so, and the clusters' own count launch leaves the index's last Count query alone
    hp.radius_count_cloud(0.9)
    for min_nb in (1, 3, 6):
        got = _run(hp, 0.7, min_nb)
        assert np.array_equal(got["kind"] == 0, fin & (count >= min_nb)), min_nb
        _same(got, cl.clusters(cloud, 0.7, min_nb), ("core", min_nb))
    assert np.array_equal(hp.cloud_outliers_radius(2)["keep"], kc.radius_rule(kc.radius_count_cloud(cloud, 0.9), fin, 2)["keep"])
    # a permutation of the rows gives the same partition and the same kinds
    ref = _run(hp, 0.7, 3)
    assert min(ref["counts"][:3]) > 50 and ref["n_clusters"] > 10
    perm = rng.permutation(len(cloud))
    hp.cloud_index_build(cloud[perm])
    got = _run(hp, 0.7, 3)
    assert np.array_equal(got["kind"], ref["kind"][perm]) and got["n_clusters"] == ref["n_clusters"] and got["counts"] == ref["counts"]
    core = got["kind"] == 0                                                          # (a border point at equal D from two clusters goes by index)
    assert cl.same_partition(got["label"][core], ref["label"][perm][core])
    assert sorted(got["n_core"].tolist()) == sorted(ref["n_core"].tolist())
    _same(got, cl.clusters(cloud[perm], 0.7, 3), "permuted")


# ---- the planted scene --------------------------------------------------------------------------------------------------------------------------------
def test_sheet_with_strays_figures(hp):
    cloud, planted = sheet_with_strays()
    n = len(cloud)
    assert hp.cloud_index_build(cloud) == (n, n - 3)
    got = _run(hp, 0.5, 0)
    assert got["n_clusters"] == 24 and sorted(got["n_points"].tolist())[-2:] == [2, 2000] and got["counts"] == [n - 3, 0, 0, 3]
    _same(got, cl.clusters(cloud, 0.5, 0), (0.5, 0))
    got = _run(hp, 0.5, 6)
    assert got["n_clusters"] == 1 and got["counts"] == [1979, 19, 27, 3] and (got["kind"][planted == 1] == 2).all() and (planted == 1).sum() == 20
    _same(got, cl.clusters(cloud, 0.5, 6), (0.5, 6))
    got = _run(hp, 0.3, 4)
    assert got["n_clusters"] == 21 and got["counts"] == [1557, 347, 121, 3]
    assert 0 < got["counts"][0] and 0 < got["counts"][1] and 0 < got["counts"][2]    # neither walk is idle
    _same(got, cl.clusters(cloud, 0.3, 4), (0.3, 4))
    t = hp.clusters_timing()
    assert len(t) == 4 and all(v > 0.0 for v in t)


# ---- select and apply ----------------------------------------------------------------------------------------------------------------------------------
def _segments(rng):
    """segments of 5, 3 and 5 lattice points far from each other (a planted tie in size), one point alone and a NaN row, rows shuffled"""
    rows = [(x, 0, 0) for x in range(5)] + [(x, 50, 0) for x in range(3)] + [(x, 0, 50) for x in range(5)] + [(200, 200, 200), (np.nan, 0, 0)]
    return np.array(rows, np.float32)[rng.permutation(len(rows))]


def _sel_same(got, want, what):
    assert np.array_equal(got["keep"], want["keep"]) and [got[k] for k in ("kept", "dropped", "noise", "not_finite")] == want["counts"], (what, got, want)
    assert sum(want["counts"]) == len(want["keep"])


def test_select_and_apply(hp):
    rng = np.random.default_rng(91)
    cloud = _segments(rng)
    fin = np.isfinite(cloud).all(axis=1)
    hp.cloud_index_build(cloud)
    ref = cl.clusters(cloud, 1.0, 1)
    assert sorted(ref["n_points"].tolist()) == [3, 5, 5] and ref["counts"] == [13, 0, 1, 1]
    _same(_run(hp, 1.0, 1), ref, "segments")
    fives = np.nonzero(ref["n_points"] == 5)[0]
    for what in (dict(), dict(min_points=4), dict(min_points=5), dict(min_points=6), dict(max_points=4), dict(min_points=3, max_points=3), dict(keep_largest=1),
                 dict(keep_largest=2), dict(keep_largest=3), dict(keep_largest=7), dict(keep_largest=1, max_points=4), dict(keep_largest=2, min_points=4),
                 dict(keep_noise=1), dict(min_points=9, keep_noise=1), dict(keep_largest=1, keep_noise=1)):
        _sel_same(hp.cloud_clusters_select(**what), cl.select(ref, **what), what)
    want = cl.select(ref, keep_largest=1)
    assert want["keepc"].tolist() == [k == fives[0] for k in range(3)]               # the tie in size goes to the smaller number
    assert cl.select(ref, keep_largest=1, max_points=4)["counts"][0] == 0            # ranked over ALL clusters: the three is not the largest
    # the mask replaces a radius-rule mask and is replaced by one
    hp.radius_count_cloud(1.0)
    rule = hp.cloud_outliers_radius(2)
    assert rule["kept"] == 7                                                         # the inner points of the segments
    sel = hp.cloud_clusters_select(min_points=4)
    assert sel["kept"] == 10
    hp.cloud_outliers_radius(2)
    kept = hp.cloud_index_apply_outliers()
    assert np.array_equal(kept, np.nonzero(rule["keep"])[0])
    hp.cloud_index_build(cloud)
    hp.radius_count_cloud(1.0); hp.cloud_outliers_radius(2)
    _run(hp, 1.0, 1)
    sel = hp.cloud_clusters_select(min_points=4, keep_noise=True)
    want = cl.select(ref, min_points=4, keep_noise=1)
    _sel_same(sel, want, "before the apply")
    kept = hp.cloud_index_apply_outliers()
    assert np.array_equal(kept, np.nonzero(want["keep"])[0]) and len(kept) == 11
    assert hp.cloud_index_points().tobytes() == cloud[want["keep"]].tobytes()
    for call in (hp.cloud_clusters_table, hp.cloud_clusters_select):                 # the clusters went with the old cloud
        with pytest.raises(RuntimeError, match=r"rc=-1: .*no immesh_cloud_clusters"):
            call()
    with pytest.raises(RuntimeError, match=r"rc=-1: .*no outlier mask"):
        hp.cloud_index_apply_outliers()
    new = cloud[want["keep"]]
    _same(_run(hp, 1.0, 1), cl.clusters(new, 1.0, 1), "after the apply")
    hp.cloud_index_build(new)                                                        # and with a rebuild
    for call in (hp.cloud_clusters_table, hp.cloud_clusters_select):
        with pytest.raises(RuntimeError, match=r"rc=-1: .*no immesh_cloud_clusters"):
            call()
    # a select that keeps nothing empties the index, and the empty index still answers
    _run(hp, 1.0, 1)
    assert hp.cloud_clusters_select(min_points=100)["kept"] == 0
    assert len(hp.cloud_index_apply_outliers()) == 0 and hp.cloud_index_points().shape == (0, 3)
    assert _run(hp, 1.0, 0)["n_clusters"] == 0 and fin.sum() == 14


# ---- errors ----------------------------------------------------------------------------------------------------------------------------------------
def test_argument_errors():
    lib = capi.load_hip_library()
    h = make_hip(lib, _small_cfg())
    try:
        cloud = np.array([[0, 0, -2], [0, 0, 3], [0, 1, 3]], np.float32)
        pts = np.array([[0, 0, 0], [0, 0, 2]], np.float32)
        P = C.c_void_p
        cc = lib.immesh_cloud_clusters; cc.argtypes = [P, C.c_double, C.c_int64, P, P, P, P]; cc.restype = C.c_int
        tb = lib.immesh_cloud_clusters_table; tb.argtypes = [P, P, P, P, P, C.c_int64, P]; tb.restype = C.c_int
        sl = lib.immesh_cloud_clusters_select; sl.argtypes = [P, C.c_int64, C.c_int64, C.c_int64, C.c_int32, P, P]; sl.restype = C.c_int
        ap = lib.immesh_cloud_index_apply_outliers; ap.argtypes = [P, P, C.c_int64, P]; ap.restype = C.c_int
        x = h.cloud_index()

        def refused(rc, text, code=E_INVAL):
            assert rc == code and text in _err(h), (rc, _err(h))

        for rc in (cc(x, 1.0, 0, None, None, None, None), tb(x, None, None, None, None, 0, None), sl(x, 0, 0, 0, 0, None, None)):
            refused(rc, b"no index has been built")
        h.cloud_index_build(cloud)

        def still_usable():
            got = h.cloud_clusters(1.0, 0)
            assert got["label"].tolist() == [0, 1, 1] and got["kind"].tolist() == [0, 0, 0] and got["n_clusters"] == 2
            assert h.cloud_clusters_table()["n_points"].tolist() == [1, 2]
            assert h.cloud_index_points().tobytes() == cloud.tobytes()
            assert h.nearest_points(pts, 10.0)["index"].tolist() == [0, 1] and h.radius_count_cloud(1.0).tolist() == [0, 1, 1]

        still_usable()
        h.cloud_index_build(cloud)                                                   # (a build drops the clusters)
        refused(tb(x, None, None, None, None, 0, None), b"no immesh_cloud_clusters")
        refused(sl(x, 0, 0, 0, 0, None, None), b"no immesh_cloud_clusters")
        for r in (0.0, -1.0, np.inf, -np.inf, np.nan):
            refused(cc(x, r, 0, None, None, None, None), b"radius")
        for m in (-1, 2 ** 31 - 1, 2 ** 40):
            refused(cc(x, 1.0, m, None, None, None, None), b"min_neighbours")
        refused(tb(x, None, None, None, None, 0, None), b"no immesh_cloud_clusters")  # refused calls leave no clusters
        still_usable()
        refused(cc(x, -1.0, 0, None, None, None, None), b"radius")                   # a refused call leaves the last clusters as they were
        assert h.cloud_clusters_table()["first"].tolist() == [0, 1]
        for bad in (-1, 2 ** 31 - 1, 2 ** 40):
            refused(sl(x, bad, 0, 0, 0, None, None), b"min_points")
            refused(sl(x, 0, bad, 0, 0, None, None), b"max_points")
            refused(sl(x, 0, 0, bad, 0, None, None), b"keep_largest")
        refused(ap(x, None, 0, None), b"no outlier mask")                            # refused selects leave no mask
        first, n = np.zeros(2, np.int32), C.c_int64(-1)
        refused(tb(x, first.ctypes.data_as(P), None, None, None, 1, C.byref(n)), b"cap 1 < 2 clusters", E_CAPACITY)
        assert n.value == 2
        refused(tb(x, first.ctypes.data_as(P), None, None, None, -1, None), b"cap is negative")
        assert tb(x, None, None, None, None, 0, C.byref(n)) == 0 and n.value == 2   # every output may be NULL
        still_usable()
        assert cc(x, 1.0, 1, None, None, None, None) == 0 and sl(x, 0, 0, 0, 0, None, None) == 0
        assert sl(x, 2 ** 31 - 2, 2 ** 31 - 2, 2 ** 31 - 2, -7, None, None) == 0 and cc(x, 1.0, 2 ** 31 - 2, None, None, None, None) == 0
        out = h.cloud_clusters_select(min_points=1)                                  # every point is noise at that min_neighbours
        assert out["keep"].tolist() == [False] * 3 and out["noise"] == 3
        h.cloud_clusters(1.0, 1)
        out = h.cloud_clusters_select(min_points=2)
        assert out["keep"].tolist() == [False, True, True] and (out["kept"], out["dropped"], out["noise"], out["not_finite"]) == (2, 0, 1, 0)
        assert ap(x, None, 0, C.byref(n)) == 0 and n.value == 2
        assert h.cloud_index_points().tobytes() == cloud[1:].tobytes()
        t = h.clusters_timing()
        assert len(t) == 4 and all(v >= 0.0 for v in t) and t[1] > 0.0
    finally:
        h.close()


# ---- state -----------------------------------------------------------------------------------------------------------------------------------------
def test_state_left_over_from_a_larger_call(hp):
    rng = np.random.default_rng(72)
    big, small = _cloud(rng, 4000), _cloud(rng, 70)
    hp.cloud_index_build(big)
    _run(hp, 0.8, 3); hp.cloud_clusters_select(min_points=5)
    hp.cloud_index_build(small)                                                      # from large to small
    for radius, min_nb in ((3.0, 2), (2.0, 0), (100.0, 5), (1.0, 1)):
        ref = cl.clusters(small, radius, min_nb)
        a = _run(hp, radius, min_nb)
        _same(a, ref, ("small", radius, min_nb))
        b = _run(hp, radius, min_nb)
        assert all(np.asarray(a[key]).tobytes() == np.asarray(b[key]).tobytes() for key in a)          # twice, the same bytes
        _sel_same(hp.cloud_clusters_select(min_points=3), cl.select(ref, min_points=3), ("small", radius, min_nb))
    only = hp.cloud_clusters(1.0, 1, want=("kind",))
    assert sorted(only) == ["counts", "kind", "n_clusters"] and np.array_equal(only["kind"], ref["kind"])


# ---- scale -------------------------------------------------------------------------------------------------------------------------------------------
def _scale_scene(seed=52, n=200000, spread=30.0):
    """six jittered sheets of 20 x 20 with 25 000 points each, sixty blobs of 500 points, scattered points in a cube of 2 x spread, coincident pairs,
    a NaN and an infinite row, rows shuffled"""
    rng = np.random.default_rng(seed)
    parts = []
    for _ in range(6):
        o = rng.uniform(-spread, spread - 20.0, 3)
        uv = rng.uniform(0, 20.0, (25000, 2))
        parts.append(np.concatenate([o[:2] + uv, o[2] + rng.normal(scale=0.01, size=(25000, 1))], axis=1))
    for _ in range(60):
        parts.append(rng.uniform(-spread, spread, 3) + rng.normal(scale=0.4, size=(500, 3)))
    parts.append(rng.uniform(-spread, spread, (n - sum(len(p) for p in parts), 3)))
    cloud = np.concatenate(parts).astype(np.float32)
    cloud[5000:5100] = cloud[4000:4100]
    cloud = cloud[rng.permutation(n)]
    cloud[7, 2] = np.nan
    cloud[n - 3, 0] = np.inf
    return cloud


def test_scale(hp):
    """200 000 points against the tree-assisted checker (tests/clusters_checker.py: every candidate pair re-measured exactly)"""
    cloud = _scale_scene()
    n = len(cloud)
    radius, min_nb = 0.3, 10
    ref = cl.clusters_tree(cloud, radius, min_nb)
    print("checker: %d clusters, kinds %s, largest %d" % (ref["n_clusters"], ref["counts"], ref["n_points"].max()))
    assert ref["n_clusters"] > 10 and min(ref["counts"][:3]) > 0.01 * n and ref["n_points"].max() <= 0.9 * n     # the checker first
    assert hp.cloud_index_build(cloud) == (n, n - 2)
    got = _run(hp, radius, min_nb)
    print("200k points: count %.3f ms, joins %.3f ms, border walk %.3f ms, numbering + table %.3f ms" % hp.clusters_timing())
    _same(got, ref, "scale")
    _sel_same(hp.cloud_clusters_select(min_points=1000, keep_largest=8), cl.select(ref, min_points=1000, keep_largest=8), "scale, select")
    got = _run(hp, radius, 0)
    print("min_neighbours 0: kinds %.3f ms, joins %.3f ms, border walk %.3f ms, numbering + table %.3f ms" % hp.clusters_timing())
    _same(got, cl.clusters_tree(cloud, radius, 0), "scale, extraction")


# ---- the live path ---------------------------------------------------------------------------------------------------------------------------------------
def test_live_path_is_untouched():
    """a indexes the stream's own world points between scans, clusters, selects and applies; b never does: both go on with the same poses, planes and
    meshes"""
    lib = capi.load_hip_library()
    cfg = capi.avia_config(cap_root_voxels=1 << 15, cap_scan_points=100000)
    a, b = make_hip(lib, cfg), make_hip(lib, cfg)
    try:
        extT = np.array(list(cfg.extT))
        world_pts = []

        def scan(k):
            R, t = synth.trajectory_pose(k)
            raw = synth.livox_scan(k, R, t, n_pts=20000, extT=extT)
            world_pts.append(((raw[::8, :3].astype(np.float64) + extT) @ R.T + t).astype(np.float32))
            if k == 0:
                for h in (a, b):
                    h.map_build(np.ascontiguousarray(raw[:, :3]), capi.make_state(R=R, t=t))
                return None
            down = synth.voxel_grid_downsample(raw, 0.4)
            prior = capi.make_state(R=R, t=t + np.array([0.01, 0.0, -0.01]), cov_diag=1e-5)
            sa, ia = a.process_scan(down, raw, prior, prior, frame_idx=k, do_mesh=True)
            sb, ib = b.process_scan(down, raw, prior, prior, frame_idx=k, do_mesh=True)
            assert ia == ib and np.array_equal(sa, sb)
            return sa

        for k in range(3):
            scan(k)
        planes, counters = a.dump_planes(), a.counters()
        cloud = np.concatenate(world_pts)
        a.cloud_index_build(cloud)
        ref = cl.clusters_tree(cloud, 0.5, 4)
        _same(_run(a, 0.5, 4), ref, "the stream's points")
        want = cl.select(ref, min_points=20)
        out = a.cloud_clusters_select(min_points=20)
        _sel_same(out, want, "the stream's points, select")
        assert 0 < out["kept"] < len(cloud)
        kept = a.cloud_index_apply_outliers()
        assert np.array_equal(kept, np.nonzero(want["keep"])[0])
        a.cloud_clusters(0.5, 0)
        assert compare_plane_tables_fast(planes, a.dump_planes(), 0.0) > 100 and a.counters() == counters
        for k in range(3, 5):
            scan(k)                                                                  # (asserts that a and b still agree)
        ea, eb = a.mesh_export(1.0, 20), b.mesh_export(1.0, 20)
        assert len(ea[1]) > 0 and ea[0].tobytes() == eb[0].tobytes() and ea[1].tobytes() == eb[1].tobytes()
        assert compare_plane_tables_fast(a.dump_planes(), b.dump_planes(), 0.0) > 100
    finally:
        a.close(); b.close()


# ---- tools/mesh_eval.py ------------------------------------------------------------------------------------------------------------------------------------
def blob_over_the_square():
    """the unit-square scene of the outlier test, a grid of ground-truth points 0.01 above the square, and a blob of 30 lattice points (5 x 3 x 2, 0.02
    apart) 0.3 above it, rows shuffled -> cloud, is_blob"""
    g = np.arange(41) / 40.0
    grid = np.concatenate([np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2), np.full((41 * 41, 1), 0.01)], axis=1)
    blob = np.array([[0.5 + 0.02 * i, 0.5 + 0.02 * j, 0.31 + 0.02 * k] for i in range(5) for j in range(3) for k in range(2)])
    cloud = np.concatenate([grid, blob]).astype(np.float32)[np.random.default_rng(4).permutation(41 * 41 + 30)]
    return cloud, cloud[:, 2] > 0.1


def test_mesh_eval_drops_the_blob(hp):
    """a small detached object has neighbours enough for both outlier rules; the clusters' size filter takes it and nothing else"""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import mesh_eval
    cloud, is_blob = blob_over_the_square()
    n_grid = 41 * 41
    assert is_blob.sum() == 30
    hp.raycast_build_triangles(np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], np.float32), np.array([[0, 1, 2], [0, 2, 3]], np.int32))
    # both outlier rules keep the blob: the checker first, then the tool
    ref = kc.knn_cloud(cloud, 8, 0.5)
    assert kc.statistical(ref[3], ref[0], np.ones(len(cloud), bool), 3.0)["keep"][is_blob].all()
    assert kc.radius_rule(kc.radius_count_cloud(cloud, 0.03), np.ones(len(cloud), bool), 2)["keep"].all()
    kept, out = mesh_eval.filter_cloud(hp, cloud, knn=(8, 3.0), radius=(0.03, 2), max_dist=0.5)
    assert (kept[:, 2] > 0.1).sum() == 30 and out["points_kept"] == len(kept) > n_grid and "clusters" not in out
    want = cl.select(cl.clusters(cloud, 0.04, 3), min_points=100)
    assert np.array_equal(want["keep"], ~is_blob)                                    # the checker first
    kept, out = mesh_eval.filter_cloud(hp, cloud, clusters=(0.04, 3), cluster_min_points=100)
    assert kept.tobytes() == cloud[~is_blob].tobytes() and out["points_before"] == len(cloud) and out["points_kept"] == n_grid
    c = out["clusters"]
    assert (c["n_clusters"], c["core"], c["border"], c["kept"], c["dropped"], c["noise"]) == (2, n_grid + 30, 0, n_grid, 30, 0)
    assert (c["radius"], c["min_neighbours"], c["min_points"], c["keep_largest"]) == (0.04, 3, 100, 0)
    res = mesh_eval.evaluate(hp, kept, tau=0.02, max_dist=0.5, density=2000.0, seed=1)
    assert res["cloud_points"] == n_grid == res["accuracy"]["within_tau"] and res["recall"] == 1.0
    assert mesh_eval.evaluate(hp, cloud, tau=0.02, max_dist=0.5, density=2000.0, seed=1)["recall"] < 1.0      # with the blob
    kept, out = mesh_eval.filter_cloud(hp, cloud, radius=(0.03, 2), clusters=(0.04, 3), cluster_keep_largest=1)  # behind the radius rule, the largest only
    assert kept.tobytes() == cloud[~is_blob].tobytes() and out["radius"]["kept"] == len(cloud) and out["clusters"]["kept"] == n_grid
