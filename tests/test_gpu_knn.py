"""k nearest neighbours, radius counts, outlier masks and their apply on the device (include/immesh_nearest.h, the Neighbours, Count and Outliers
rules) against the brute-force numpy restatement (tests/knn_checker.py), bit for bit: tree sizes at which the build and the walk change path, every
capacity of the k-list and partial lists, the single-leaf tree, exact ties across the k-th slot, the distance boundary, cross-checks against the
single-nearest query and between the modes, state left over from larger calls, both outlier rules and the apply, argument errors, scale, and the
live path without side effects."""
import ctypes as C

import numpy as np
import pytest

import knn_checker as kc
import nearest_checker as nc
from immesh_amd import capi, synth
from conftest import make_hip
from parity_utils import compare_plane_tables_fast
from test_gpu_nearest import _cloud, _err, _local, _queries
from test_gpu_render import _rand_rot, _small_cfg
from test_knn_cpu import sheet_with_strays

pytestmark = pytest.mark.gpu
E_INVAL, E_CAPACITY = -1, -4
KS = (1, 2, 3, 8, 63, 64)


@pytest.fixture(scope="module")
def hp():
    h = make_hip(capi.load_hip_library(), _small_cfg())
    yield h
    h.close()


def _same(got, ref, what, keys=("count", "index", "d2")):
    """device dict == checker tuple, bit for bit"""
    for key, r in zip(keys, ref):
        g = got[key]
        assert g.dtype == r.dtype and g.shape == r.shape, (what, key, g.dtype, r.dtype, g.shape, r.shape)
        if g.size == 0:
            continue
        diff = np.nonzero((g.reshape(len(g), -1).view(np.uint8) != np.ascontiguousarray(r).reshape(len(r), -1).view(np.uint8)).any(axis=1))[0]
        assert len(diff) == 0, (what, key, len(diff), len(g), diff[:5].tolist(), g[diff[:5]].tolist(), r[diff[:5]].tolist())


def _sized_cloud(rng, n_in, spread=5.0):
    """n_in finite points, a NaN point and an infinite point (from three points on), rows in random order: index order is not spatial order"""
    c = rng.uniform(-spread, spread, (n_in, 3)).astype(np.float32)
    if n_in >= 3:
        c = np.concatenate([c, np.array([[0, np.nan, 0], [np.inf, 0, 0]], np.float32)])[rng.permutation(n_in + 2)]
    return c


def _lattice(rng, m=4):
    g = np.arange(m, dtype=np.float32)
    c = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    return c[rng.permutation(len(c))]


# ---- sizes -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_in", [0, 1, 2, 3, 63, 64, 65, 257])
def test_sizes_match_checker(hp, n_in):
    rng = np.random.default_rng(900 + n_in)
    cloud = _sized_cloud(rng, n_in)
    assert hp.cloud_index_build(cloud) == (len(cloud), n_in)
    rot, pos = _rand_rot(rng), rng.uniform(-2, 2, 3)
    world = _queries(rng, cloud, 300, near=0.5)                                      # (a NaN query and a query 10^6 away are its last two)
    local = _local(world, rot, pos)
    for max_dist in (1.5, 100.0):
        for r, p, pts in ((None, None, world), (rot, pos, local)):
            frame = None if r is None else capi.ray_frame(r, p)
            for k in KS:
                ref = kc.knn(r, p, pts, k, max_dist, cloud)
                assert ref[0][-1] == 0 and ref[0][-2] == 0 and (ref[0].max() == min(k, n_in) or max_dist < 100.0)
                _same(hp.knn_points(pts, k, max_dist, frame), ref, (n_in, k, max_dist, r is not None))
            ref = kc.radius_count(r, p, pts, max_dist, cloud)
            assert ref.max() == n_in or max_dist < 100.0
            assert np.array_equal(hp.radius_count_points(pts, max_dist, frame), ref), (n_in, max_dist)
        for k in KS:
            _same(hp.knn_cloud(k, max_dist), kc.knn_cloud(cloud, k, max_dist), ("cloud", n_in, k, max_dist), keys=("count", "index", "d2", "mean"))
        assert np.array_equal(hp.radius_count_cloud(max_dist), kc.radius_count_cloud(cloud, max_dist))
    assert hp.knn_points(np.zeros((0, 3), np.float32), 3, 1.0)["index"].shape == (0, 3)


# ---- the single-leaf tree ----------------------------------------------------------------------------------------------------------------------
def test_single_leaf_tree_is_met_once(hp):
    """the tree of one point names it as both children of the root: the list holds it once, the counter counts it once"""
    cloud = np.array([[np.nan, 0, 0], [1, 2, 3]], np.float32)
    assert hp.cloud_index_build(cloud) == (2, 1)
    q = np.array([[1, 2, 3], [1, 2, 4], [9, 9, 9]], np.float32)
    got = hp.knn_points(q, 2, 2.0)
    assert got["count"].tolist() == [1, 1, 0] and got["index"].tolist() == [[1, -1], [1, -1], [-1, -1]] and got["d2"].tolist() == [[0, -1], [1, -1], [-1, -1]]
    assert hp.radius_count_points(q, 2.0).tolist() == [1, 1, 0]
    got = hp.knn_cloud(2, 2.0)
    assert got["count"].tolist() == [0, 0] and got["mean"].tolist() == [-1.0, -1.0] and (got["index"] == -1).all()
    assert hp.radius_count_cloud(2.0).tolist() == [0, 0]
    for k in KS:
        _same(hp.knn_points(q, k, 2.0), kc.knn(None, None, q, k, 2.0, cloud), k)


# ---- exact ties ----------------------------------------------------------------------------------------------------------------------------------
def test_exact_ties_straddle_the_kth_slot(hp):
    """a shuffled integer lattice: a cell centre has 8 equidistant points, a face centre 4, a lattice point 6 at distance 1; for every k from 1 to 9
    the tie straddles the k-th slot somewhere, and a lower index at the k-th D is met after the list is full"""
    rng = np.random.default_rng(31)
    cloud = _lattice(rng)
    hp.cloud_index_build(cloud)
    cells = np.stack(np.meshgrid(*[np.arange(3) + 0.5] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    faces = cells.copy(); faces[:, 2] -= 0.5
    q = np.concatenate([cells, faces, cloud.astype(np.float64)]).astype(np.float32)
    rot, pos = np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]]), np.array([1.0, -2.0, 0.5])         # exact in double: the ties stay ties
    local = _local(q, rot, pos)
    for k in range(1, 10):
        ref = kc.knn(None, None, q, k, 100.0, cloud)
        assert (ref[0] == k).all()
        _same(hp.knn_points(q, k, 100.0), ref, ("lattice", k))
        _same(hp.knn_points(local, k, 100.0, capi.ray_frame(rot, pos)), kc.knn(rot, pos, local, k, 100.0, cloud), ("lattice, frame", k))
        _same(hp.knn_cloud(k, 100.0), kc.knn_cloud(cloud, k, 100.0), ("lattice, cloud mode", k), keys=("count", "index", "d2", "mean"))
    ref = kc.knn(None, None, q[:27], 8, 100.0, cloud)
    assert (ref[2] == 0.75).all()                                                    # the checker first: all eight slots of a cell centre are one tie
    for radius in (np.sqrt(0.75), 1.0, np.sqrt(2.0)):
        assert np.array_equal(hp.radius_count_points(q, radius), kc.radius_count(None, None, q, radius, cloud))
        assert np.array_equal(hp.radius_count_cloud(radius), kc.radius_count_cloud(cloud, radius))
    # coincident points: the others at D = 0 by index, never the point's own
    cloud = np.concatenate([np.tile(np.array([[1.5, -2, 3]], np.float32), (5, 1)), np.tile(np.array([[1.5, -2, 3.5]], np.float32), (70, 1))])
    hp.cloud_index_build(cloud)
    for k in (1, 3, 4, 5, 64):
        ref = kc.knn_cloud(cloud, k, 1.0)
        _same(hp.knn_cloud(k, 1.0), ref, ("coincident", k), keys=("count", "index", "d2", "mean"))
        _same(hp.knn_points(cloud[:6], k, 1.0), kc.knn(None, None, cloud[:6], k, 1.0, cloud), ("coincident, points", k))
    got = hp.knn_cloud(3, 1.0)
    assert got["index"][:5].tolist() == [[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2], [0, 1, 2]] and (got["d2"][:5] == 0).all()
    assert hp.radius_count_cloud(0.25).tolist() == [4] * 5 + [69] * 70 and hp.radius_count_cloud(0.5).tolist() == [74] * 75


# ---- the boundary --------------------------------------------------------------------------------------------------------------------------------
def test_distance_boundary(hp):
    cloud = np.array([[0, 0, 2], [0, 0, -3], [7, 7, 7]], np.float32)
    hp.cloud_index_build(cloud)
    q = np.zeros((1, 3), np.float32)
    got = hp.knn_points(q, 2, 2.0)
    assert got["count"].tolist() == [1] and got["index"].tolist() == [[0, -1]] and got["d2"].tolist() == [[4.0, -1.0]]      # D == r2 counts
    assert hp.radius_count_points(q, 2.0).tolist() == [1] and hp.radius_count_points(q, 3.0).tolist() == [2]
    up = np.nextafter(2.0, 3.0)
    frame = capi.ray_frame(np.eye(3), [0.0, 0.0, 2.0 - up])                           # the next double above: D is the next double above r2
    assert kc.knn(np.eye(3), [0.0, 0.0, 2.0 - up], q, 2, 2.0, cloud)[0].tolist() == [0]
    assert hp.knn_points(q, 2, 2.0, frame)["count"].tolist() == [0] and hp.radius_count_points(q, 2.0, frame).tolist() == [0]
    assert hp.knn_points(q, 2, up, frame)["count"].tolist() == [1] and hp.radius_count_points(q, up, frame).tolist() == [1]
    # cloud mode: the two points on the axis are 5 apart
    assert hp.knn_cloud(1, 5.0)["count"].tolist() == [1, 1, 0] and hp.radius_count_cloud(5.0).tolist() == [1, 1, 0]
    below = np.nextafter(5.0, 0.0)
    assert hp.knn_cloud(1, below)["count"].tolist() == [0, 0, 0] and hp.radius_count_cloud(below).tolist() == [0, 0, 0]


# ---- cross-checks ----------------------------------------------------------------------------------------------------------------------------------
def test_cross_checks(hp):
    rng = np.random.default_rng(61)
    cloud = _cloud(rng, 3000)
    cloud[200:220] = cloud[100:120]                                                  # coincident pairs
    hp.cloud_index_build(cloud)
    q = _queries(rng, cloud, 2000, near=0.3)
    one, near = hp.knn_points(q, 1, 0.7), hp.nearest_points(q, 0.7, want=("d2", "index"))
    assert one["index"][:, 0].tobytes() == near["index"].tobytes() and one["d2"][:, 0].tobytes() == near["d2"].tobytes()
    assert np.array_equal(one["count"], (near["index"] >= 0).astype(np.int32)) and 0 < one["count"].sum() < len(q)
    for k in (8, 16):
        got, count = hp.knn_points(q, k, 0.9), hp.radius_count_points(q, 0.9)
        below = got["count"] < k
        assert np.array_equal(count[below], got["count"][below]) and (count[~below] >= k).all() and 20 < below.sum() < len(q) - 20
        assert np.array_equal(got["index"][:, 0], hp.nearest_points(q, 0.9, want=("index",))["index"])
    # cloud mode == point mode on the same points with each point's own index removed
    k = 8
    pm, cm = hp.knn_points(cloud, k + 1, 0.7), hp.knn_cloud(k, 0.7)
    own = pm["index"] == np.arange(len(cloud))[:, None]
    fin = np.isfinite(cloud).all(axis=1)
    assert (own.sum(axis=1) == fin).all()                                            # a finite point finds itself (D = 0, at most 1 coincident copy before it)
    order = np.argsort(own, axis=1, kind="stable")[:, :k]                            # the list without the point's own entry, order kept
    index, d2 = np.take_along_axis(pm["index"], order, axis=1), np.take_along_axis(pm["d2"], order, axis=1)
    assert index.tobytes() == cm["index"].tobytes() and d2.tobytes() == cm["d2"].tobytes() and np.array_equal(cm["count"], np.maximum(pm["count"] - 1, 0))
    _same(cm, kc.knn_cloud(cloud, k, 0.7), "cloud mode", keys=("count", "index", "d2", "mean"))
    assert np.array_equal(hp.radius_count_cloud(0.7), np.maximum(hp.radius_count_points(cloud, 0.7) - 1, 0))


# ---- state -----------------------------------------------------------------------------------------------------------------------------------------
def test_state_left_over_from_larger_calls(hp):
    rng = np.random.default_rng(71)
    big, small = _cloud(rng, 4000), _cloud(rng, 70)
    q = _queries(rng, small, 300, near=0.5)
    hp.cloud_index_build(big)
    hp.knn_points(_queries(rng, big, 3000), 64, 3.0); hp.knn_cloud(64, 3.0); hp.radius_count_cloud(3.0)
    hp.cloud_index_build(small)                                                      # from large to small
    for k in (64, 16, 5, 2):                                                         # k going down on one index: no stale slot of the longer lists
        _same(hp.knn_points(q, k, 3.0), kc.knn(None, None, q, k, 3.0, small), ("points", k))
        ref = kc.knn_cloud(small, k, 3.0)
        a = hp.knn_cloud(k, 3.0)
        _same(a, ref, ("cloud", k), keys=("count", "index", "d2", "mean"))
        b = hp.knn_cloud(k, 3.0)
        assert all(a[key].tobytes() == b[key].tobytes() for key in a)                # twice, the same bytes
        only = hp.knn_cloud(k, 3.0, want=("mean",))                                  # without lists on the device
        assert list(only) == ["mean"] and only["mean"].tobytes() == ref[3].tobytes()
        only = hp.knn_cloud(k, 3.0, want=("count", "mean"))
        assert only["mean"].tobytes() == ref[3].tobytes() and np.array_equal(only["count"], ref[0])
    assert np.array_equal(hp.radius_count_cloud(3.0), kc.radius_count_cloud(small, 3.0))


# ---- outliers and the apply --------------------------------------------------------------------------------------------------------------------------
def _stat_keys(d):
    return {key: d[key] for key in ("kept", "outliers", "isolated", "not_finite")}


def test_outliers_and_apply(hp):
    cloud, kind = sheet_with_strays()
    fin = np.isfinite(cloud).all(axis=1)
    n = len(cloud)
    assert hp.cloud_index_build(cloud) == (n, n - 3)
    # the statistical rule
    ref = kc.knn_cloud(cloud, 8, 5.0)
    got = hp.knn_cloud(8, 5.0, want=("count", "mean"))
    assert got["mean"].tobytes() == ref[3].tobytes() and np.array_equal(got["count"], ref[0])
    for mult in (0.0, 1.0, 3.0):
        want = kc.statistical(ref[3], ref[0], fin, mult)
        out = hp.cloud_outliers_statistical(mult)
        assert (out["mu"], out["sigma"], out["threshold"]) == (want["mu"], want["sigma"], want["threshold"]), mult
        assert np.array_equal(out["keep"], want["keep"]) and _stat_keys(out) == _stat_keys(want)
    assert not want["keep"][kind != 0].any() and want["isolated"] == 5 and want["not_finite"] == 3 and want["outliers"] >= 20
    # the radius rule replaces the mask
    rc_ref = kc.radius_count_cloud(cloud, 0.5)
    assert np.array_equal(hp.radius_count_cloud(0.5), rc_ref)
    for min_nb in (0, 1, 6, 10 ** 6):
        wr = kc.radius_rule(rc_ref, fin, min_nb)
        out = hp.cloud_outliers_radius(min_nb)
        assert np.array_equal(out["keep"], wr["keep"]) and _stat_keys(out) == _stat_keys(wr), min_nb
    assert wr["kept"] == 0 and kc.radius_rule(rc_ref, fin, 0)["kept"] == n - 3
    wr = kc.radius_rule(rc_ref, fin, 6)
    assert not wr["keep"][kind != 0].any() and wr["keep"][kind == 0].mean() > 0.9
    out = hp.cloud_outliers_radius(6)
    # the apply
    kept = hp.cloud_index_apply_outliers()
    assert kept.dtype == np.int32 and np.array_equal(kept, np.nonzero(wr["keep"])[0]) and (np.diff(kept) > 0).all()
    new = cloud[kept]
    assert hp.cloud_index_points().tobytes() == new.tobytes()
    g = hp.lib.immesh_cloud_index_sizes; g.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]; g.restype = C.c_int
    a, b = C.c_int64(0), C.c_int64(0)
    assert g(hp.cloud_index(), C.byref(a), C.byref(b)) == 0 and (a.value, b.value) == (len(new), len(new))
    with pytest.raises(RuntimeError, match=r"rc=-1: .*no nearest-point query"):
        hp.nearest_stats(0.1, 4)                                                     # a reduction after an apply
    with pytest.raises(RuntimeError, match=r"rc=-1: .*no outlier mask"):
        hp.cloud_index_apply_outliers()                                              # the mask went with the old cloud
    with pytest.raises(RuntimeError, match=r"rc=-1: .*no immesh_radius_count_cloud"):
        hp.cloud_outliers_radius(1)
    rng = np.random.default_rng(81)
    q = _queries(rng, new, 500, near=0.3, spread=10.0)
    ref = nc.nearest(None, None, q, 2.0, new)
    got = hp.nearest_points(q, 2.0)
    assert all(got[key].tobytes() == r.tobytes() for key, r in zip(("d2", "dist", "index", "xyz"), ref)) and (ref[2] >= 0).sum() > 100
    _same(hp.knn_points(q, 5, 2.0), kc.knn(None, None, q, 5, 2.0, new), "after the apply")
    # the caster's samples against the filtered index
    hp.raycast_build_triangles(np.array([[0, 0, 0], [10, 0, 0], [10, 10, 0], [0, 10, 0]], np.float32), np.array([[0, 1, 2], [0, 2, 3]], np.int32))
    xyz, _ = hp.mesh_sample(5.0, 3)                                                  # the square under the sheet
    ref = nc.nearest(None, None, xyz, 1.0, new)
    got = hp.nearest_samples(1.0)
    assert all(got[key].tobytes() == r.tobytes() for key, r in zip(("d2", "dist", "index", "xyz"), ref)) and len(xyz) == 500 and (ref[2] >= 0).all()
    # the statistical rule applied to the filtered cloud, then a mask that keeps nothing
    ref = kc.knn_cloud(new, 8, 5.0)
    hp.knn_cloud(8, 5.0, want=("mean",))
    want = kc.statistical(ref[3], ref[0], np.ones(len(new), bool), 1.0)
    out = hp.cloud_outliers_statistical(1.0)
    assert np.array_equal(out["keep"], want["keep"]) and 0 < want["kept"] < len(new)
    kept2 = hp.cloud_index_apply_outliers()
    assert np.array_equal(kept2, np.nonzero(want["keep"])[0]) and hp.cloud_index_points().tobytes() == new[kept2].tobytes()
    hp.radius_count_cloud(1e-6)
    out = hp.cloud_outliers_radius(5)
    assert out["kept"] == 0 and not out["keep"].any()
    assert len(hp.cloud_index_apply_outliers()) == 0 and hp.cloud_index_points().shape == (0, 3)
    assert g(hp.cloud_index(), C.byref(a), C.byref(b)) == 0 and (a.value, b.value) == (0, 0)
    assert hp.nearest_points(q, 100.0)["index"].tolist() == [-1] * len(q)
    assert hp.knn_points(q, 4, 100.0)["count"].tolist() == [0] * len(q) and hp.radius_count_points(q, 100.0).tolist() == [0] * len(q)
    assert hp.knn_cloud(4, 1.0)["mean"].shape == (0,)
    out = hp.cloud_outliers_statistical(1.0)                                         # n_used == 0 on an empty cloud: no error
    assert (out["mu"], out["sigma"], out["threshold"], out["kept"]) == (0.0, 0.0, 0.0, 0)
    # n_used == 0 on a cloud of isolated points keeps nothing
    far = cloud[kind == 3]
    hp.cloud_index_build(far)
    hp.knn_cloud(4, 1.0, want=("mean",))
    out = hp.cloud_outliers_statistical(2.0)
    assert (out["mu"], out["sigma"], out["threshold"]) == (0.0, 0.0, 0.0) and _stat_keys(out) == dict(kept=0, outliers=0, isolated=5, not_finite=0)


def test_mesh_eval_drops_the_strays(hp):
    """tools/mesh_eval.py's filter on the unit square against a grid of ground-truth points 0.01 above it and five strays high above: either rule
    takes the strays and nothing else, and the evaluation that follows runs on the kept points"""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import mesh_eval
    g = np.arange(41) / 40.0
    grid = np.concatenate([np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2), np.full((41 * 41, 1), 0.01)], axis=1)
    strays = np.array([[0.2, 0.2, 0.4], [0.5, 0.5, 0.3], [0.8, 0.1, 0.45], [0.1, 0.9, 0.35], [0.9, 0.9, 0.5]])
    cloud = np.concatenate([grid, strays]).astype(np.float32)[np.random.default_rng(3).permutation(41 * 41 + 5)]
    is_stray = cloud[:, 2] > 0.1
    hp.raycast_build_triangles(np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], np.float32), np.array([[0, 1, 2], [0, 2, 3]], np.int32))
    ref = kc.knn_cloud(cloud, 8, 0.5)
    want = kc.statistical(ref[3], ref[0], np.ones(len(cloud), bool), 3.0)
    assert np.array_equal(want["keep"], ~is_stray)                                   # the checker first
    kept, out = mesh_eval.filter_cloud(hp, cloud, knn=(8, 3.0), max_dist=0.5)
    assert kept.tobytes() == cloud[~is_stray].tobytes() and out["points_before"] == len(cloud) and out["points_kept"] == 41 * 41
    assert (out["knn"]["mu"], out["knn"]["sigma"], out["knn"]["threshold"]) == (want["mu"], want["sigma"], want["threshold"])
    assert (out["knn"]["kept"], out["knn"]["outliers"], out["knn"]["isolated"], out["knn"]["not_finite"]) == (41 * 41, 5, 0, 0)
    res = mesh_eval.evaluate(hp, kept, tau=0.02, max_dist=0.5, density=2000.0, seed=1)
    assert res["cloud_points"] == 41 * 41 == res["accuracy"]["within_tau"] and res["recall"] == 1.0 and abs(res["accuracy"]["mean"] - 0.01) < 1e-8
    assert mesh_eval.evaluate(hp, cloud, tau=0.02, max_dist=0.5, density=2000.0, seed=1)["recall"] < 1.0      # with the strays
    kept, out = mesh_eval.filter_cloud(hp, cloud, radius=(0.03, 2), max_dist=0.5)
    assert kept.tobytes() == cloud[~is_stray].tobytes() and (out["radius"]["kept"], out["radius"]["outliers"], out["radius"]["isolated"]) == (41 * 41, 5, 5)
    kept, out = mesh_eval.filter_cloud(hp, cloud, knn=(8, 3.0), radius=(0.03, 3), max_dist=0.5)                # both: the statistical rule first
    assert out["knn"]["kept"] == 41 * 41 and out["radius"]["kept"] == out["points_kept"] == 41 * 41 - 4 == len(kept)      # a corner has two others within 0.03


# ---- errors ----------------------------------------------------------------------------------------------------------------------------------------
def test_argument_errors():
    lib = capi.load_hip_library()
    h = make_hip(lib, _small_cfg())
    try:
        cloud = np.array([[0, 0, -2], [0, 0, 3], [0, 1, 3]], np.float32)
        pts = np.array([[0, 0, 0], [0, 0, 2]], np.float32)
        P = C.c_void_p
        kp = lib.immesh_knn_points; kp.argtypes = [P, P, P, C.c_int64, C.c_int32, C.c_double, P, P, P]; kp.restype = C.c_int
        kcl = lib.immesh_knn_cloud; kcl.argtypes = [P, C.c_int32, C.c_double, P, P, P, P]; kcl.restype = C.c_int
        rp = lib.immesh_radius_count_points; rp.argtypes = [P, P, P, C.c_int64, C.c_double, P]; rp.restype = C.c_int
        rcl = lib.immesh_radius_count_cloud; rcl.argtypes = [P, C.c_double, P]; rcl.restype = C.c_int
        os_ = lib.immesh_cloud_outliers_statistical; os_.argtypes = [P, C.c_double, P, P, P, P, P]; os_.restype = C.c_int
        orad = lib.immesh_cloud_outliers_radius; orad.argtypes = [P, C.c_int64, P, P]; orad.restype = C.c_int
        ap = lib.immesh_cloud_index_apply_outliers; ap.argtypes = [P, P, C.c_int64, P]; ap.restype = C.c_int
        gp = lib.immesh_cloud_index_points; gp.argtypes = [P, P, C.c_int64, P]; gp.restype = C.c_int
        x, pp = h.cloud_index(), pts.ctypes.data_as(P)

        def refused(rc, text, code=E_INVAL):
            assert rc == code and text in _err(h), (rc, _err(h))

        # an unbuilt index
        for rc in (kp(x, None, pp, 2, 1, 1.0, None, None, None), kcl(x, 1, 1.0, None, None, None, None), rp(x, None, pp, 2, 1.0, None),
                   rcl(x, 1.0, None), os_(x, 1.0, None, None, None, None, None), orad(x, 1, None, None), ap(x, None, 0, None), gp(x, None, 0, None)):
            refused(rc, b"no index has been built")
        h.cloud_index_build(cloud)

        def still_usable():
            got = h.knn_points(pts, 2, 10.0)
            assert got["index"].tolist() == [[0, 1], [1, 2]] and got["d2"].tolist() == [[4.0, 9.0], [1.0, 2.0]]
            assert h.knn_cloud(1, 10.0)["mean"].tolist() == [5.0, 1.0, 1.0] and h.radius_count_cloud(1.0).tolist() == [0, 1, 1]
            assert h.cloud_index_points().tobytes() == cloud.tobytes()
            assert h.nearest_points(pts, 10.0)["index"].tolist() == [0, 1]

        still_usable()
        h.cloud_index_build(cloud)                                                   # (a build drops the cloud-mode results)
        refused(os_(x, 1.0, None, None, None, None, None), b"no immesh_knn_cloud query")
        refused(orad(x, 1, None, None), b"no immesh_radius_count_cloud query")
        refused(ap(x, None, 0, None), b"no outlier mask")
        for k in (0, 65, -1):
            refused(kp(x, None, pp, 2, k, 1.0, None, None, None), b"1 <= k <= 64")
            refused(kcl(x, k, 1.0, None, None, None, None), b"1 <= k <= 64")
        for d in (0.0, -1.0, np.inf, -np.inf, np.nan):
            refused(kp(x, None, pp, 2, 1, d, None, None, None), b"max_dist")
            refused(kcl(x, 1, d, None, None, None, None), b"max_dist")
            refused(rp(x, None, pp, 2, d, None), b"radius")
            refused(rcl(x, d, None), b"radius")
        for n in (-1, 2 ** 31 - 1):
            refused(kp(x, None, pp, n, 1, 1.0, None, None, None), b"point array")
            refused(rp(x, None, pp, n, 1.0, None), b"point array")
        refused(kp(x, None, None, 2, 1, 1.0, None, None, None), b"point array")
        bad = capi.ray_frame(pos=[np.nan, 0, 0])
        refused(kp(x, C.byref(bad), pp, 2, 1, 1.0, None, None, None), b"finite")
        refused(rp(x, C.byref(bad), pp, 2, 1.0, None), b"finite")
        still_usable()
        for mult in (np.nan, -1.0, np.inf, -0.5):
            refused(os_(x, mult, None, None, None, None, None), b"mult")
        for m in (-1, 2 ** 31 - 1, 2 ** 40):
            refused(orad(x, m, None, None), b"min_neighbours")
        refused(ap(x, None, 0, None), b"no outlier mask")                            # refused rules leave no mask
        out = h.cloud_outliers_radius(1)
        assert out["keep"].tolist() == [False, True, True]
        kept, n = np.zeros(2, np.int32), C.c_int64(-1)
        refused(ap(x, kept.ctypes.data_as(P), 1, C.byref(n)), b"cap 1 < 2 kept points", E_CAPACITY)
        assert n.value == 2
        refused(ap(x, kept.ctypes.data_as(P), -1, None), b"cap is negative")
        xyz = np.zeros((3, 3), np.float32)
        refused(gp(x, xyz.ctypes.data_as(P), 2, C.byref(n)), b"cap 2 < 3 points", E_CAPACITY)
        assert n.value == 3
        still_usable()                                                               # the refused apply left the index as it was
        assert h.cloud_outliers_radius(1)["kept"] == 2
        assert ap(x, None, 0, C.byref(n)) == 0 and n.value == 2                      # every output may be NULL
        assert h.cloud_index_points().tobytes() == cloud[1:].tobytes()
        assert kp(x, None, pp, 2, 3, 1.0, None, None, None) == 0 and kcl(x, 3, 1.0, None, None, None, None) == 0
        assert rp(x, None, pp, 2, 1.0, None) == 0 and rcl(x, 1.0, None) == 0 and kp(x, None, None, 0, 3, 1.0, None, None, None) == 0
        assert os_(x, 1.0, None, None, None, None, None) == 0 and orad(x, 0, None, None) == 0
        t = h.knn_timing()
        assert len(t) == 3 and all(v >= 0.0 for v in t) and t[2] > 0.0
    finally:
        h.close()


# ---- scale -------------------------------------------------------------------------------------------------------------------------------------------
def test_scale(hp):
    """a 200 000-point cloud x 100 000 queries, k = 16, and the radius count, against the KD-tree-assisted checker (tests/knn_checker.py: every
    candidate re-measured exactly, the search widened until the tree cannot have decided a tie)"""
    rng = np.random.default_rng(51)
    cloud = _cloud(rng, 200000, spread=30.0)
    cloud[5000:5100] = cloud[4000:4100]                                              # coincident pairs
    assert hp.cloud_index_build(cloud) == (200000, 199998)
    pts = _queries(rng, cloud, 100000, near=0.3, spread=30.0)
    got = hp.knn_points(pts, 16, 1.5)
    t_knn = hp.knn_timing()[0]
    ref = kc.knn_tree(pts, 16, 1.5, cloud)
    print("200k points x 100k queries: k = 16 %.3f ms; full lists %.3f" % (t_knn, (ref[0] == 16).mean()))
    assert 0.05 < (ref[0] == 16).mean() < 0.999 and (ref[0] > 0).mean() > 0.9
    _same(got, ref, "scale, k = 16")
    count = hp.radius_count_points(pts, 1.5)
    print("radius count %.3f ms, mean count %.2f" % (hp.knn_timing()[0], count.mean()))
    assert np.array_equal(count, kc.radius_count_tree(pts, 1.5, cloud)) and count.max() > 10
    # cloud mode, mean only: the means of the lists a point-mode query over the same points gives
    sub = np.arange(0, 200000, 97)
    skip = np.arange(len(cloud))
    ref = kc.knn_tree(cloud, 16, 1.5, cloud, skip=skip)
    mean = hp.knn_cloud(16, 1.5, want=("mean",))["mean"]
    assert mean.tobytes() == kc.mean_of(ref[0], ref[2]).tobytes() and (mean[sub] >= 0).mean() > 0.9


# ---- the live path ---------------------------------------------------------------------------------------------------------------------------------------
def test_live_path_is_untouched():
    """a indexes the stream's own world points between scans, queries neighbours, masks and applies; b never does: both go on with the same poses,
    planes and meshes"""
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
        ref = kc.knn_tree(cloud, 8, 1.0, cloud, skip=np.arange(len(cloud)))
        got = a.knn_cloud(8, 1.0)
        _same(got, ref + (kc.mean_of(ref[0], ref[2]),), "the stream's points", keys=("count", "index", "d2", "mean"))
        out = a.cloud_outliers_statistical(2.0)
        assert 0 < out["kept"] < len(cloud)
        kept = a.cloud_index_apply_outliers()
        assert np.array_equal(kept, np.nonzero(out["keep"])[0])
        a.radius_count_points(cloud[::3], 0.5)
        assert compare_plane_tables_fast(planes, a.dump_planes(), 0.0) > 100 and a.counters() == counters
        for k in range(3, 5):
            scan(k)                                                                  # (asserts that a and b still agree)
        ea, eb = a.mesh_export(1.0, 20), b.mesh_export(1.0, 20)
        assert len(ea[1]) > 0 and ea[0].tobytes() == eb[0].tobytes() and ea[1].tobytes() == eb[1].tobytes()
        assert compare_plane_tables_fast(a.dump_planes(), b.dump_planes(), 0.0) > 100
    finally:
        a.close(); b.close()
