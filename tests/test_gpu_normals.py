"""Cloud normals and their agreement with the mesh on the device (include/immesh_normals.h, the Normals and Agreement rules) against the numpy
restatement (tests/normals_checker.py), bit for bit: cloud sizes at which the build and the walk change path crossed with every capacity of the
k-list at and past its edge, exact ties across the k-th slot, the distance boundary, the line gate at its edge, the sign rules, a cloud far from
the origin, cross-checks against immesh_knn_cloud and immesh_closest_points, both agreement directions and their reduction, the lifecycle, argument
errors, scale, tools/mesh_eval.py, and the live path without side effects."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import knn_checker as kc
import normals_checker as nk
from immesh_amd import capi, synth
from conftest import make_hip
from parity_utils import compare_plane_tables_fast
from test_gpu_nearest import _cloud, _err
from test_gpu_render import _small_cfg
from test_normals_cpu import noisy_sheet

pytestmark = pytest.mark.gpu
E_INVAL, E_CAPACITY = -1, -4
KEYS = ("normal", "curvature", "eig", "count", "status")
SQUARE_V = np.array([[0, 0, 0], [4, 0, 0], [4, 4, 0], [0, 4, 0]], np.float32)
SQUARE_F = np.array([[0, 1, 2], [0, 2, 3]], np.int32)


@pytest.fixture(scope="module")
def hp():
    h = make_hip(capi.load_hip_library(), _small_cfg())
    yield h
    h.close()


def _same(got, ref, what, keys=KEYS):
    """device dict == checker dict, bit for bit, and the four counts"""
    for key in keys:
        g, r = got[key], ref[key]
        assert g.dtype == r.dtype and g.shape == r.shape, (what, key, g.dtype, r.dtype, g.shape, r.shape)
        if g.size == 0:
            continue
        diff = np.nonzero((g.reshape(len(g), -1).view(np.uint8) != np.ascontiguousarray(r).reshape(len(r), -1).view(np.uint8)).any(axis=1))[0]
        assert len(diff) == 0, (what, key, len(diff), len(g), diff[:5].tolist(), g[diff[:5]].tolist(), r[diff[:5]].tolist())
    assert [got[key] for key in ("with_normal", "too_few", "line_like", "not_finite")] == ref["counts"].tolist(), what


def _check(hp, cloud, k, max_dist, min_ratio=0.0, mode=nk.CANONICAL, viewpoint=None, what="", lists=None):
    ref = nk.normals(cloud, k, max_dist, min_ratio, mode, viewpoint, lists=lists)
    got = hp.cloud_normals(k, max_dist, min_ratio, mode, viewpoint)
    _same(got, ref, (what, k, max_dist, min_ratio, mode))
    assert ref["counts"].sum() == len(cloud)
    return ref


def _plane_grid(m, spacing=1.0, z=0.0):
    g = np.arange(m, dtype=np.float32) * np.float32(spacing)
    return np.concatenate([np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2), np.full((m * m, 1), z, np.float32)], axis=1)


# ---- sizes ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 2, 3, 63, 64, 65, 257])
def test_sizes_match_checker(hp, n):
    """every capacity of the list (4, 16, 64) at and past its edge; m = 3 is the smallest neighbourhood with a normal; more neighbours asked for
    than exist"""
    rng = np.random.default_rng(1200 + n)
    cloud = _cloud(rng, n)
    n_in = int(np.isfinite(cloud).all(axis=1).sum())
    assert hp.cloud_index_build(cloud) == (n, n_in)
    for k in (2, 4, 5, 16, 17, 64):
        for max_dist in (2.5, 100.0):
            lists = kc.knn_cloud(cloud, k, max_dist)[:2]
            ref = _check(hp, cloud, k, max_dist, what=("sizes", n), lists=lists)
            if max_dist == 100.0:
                assert ref["counts"][3] == n - n_in and ((ref["count"][ref["status"] != 2] == min(k, n_in - 1)).all() or n_in == 0)
                assert ref["counts"][0] == (n_in if n_in >= 3 else 0)
        vp = [0.5, -0.25, 9.0]
        _check(hp, cloud, k, 100.0, 0.05, nk.VIEWPOINT, vp, what=("sizes, viewpoint", n), lists=lists)
    normal, status = hp.cloud_normals_get()
    last = nk.normals(cloud, 64, 100.0, 0.05, nk.VIEWPOINT, vp, lists=lists)
    assert normal.tobytes() == last["normal"].tobytes() and status.tobytes() == last["status"].tobytes()


# ---- exact ties ----------------------------------------------------------------------------------------------------------------------------------
def test_exact_ties_decide_the_neighbourhood(hp):
    """a shuffled integer lattice: a lattice point has 6 others at distance 1, 12 at sqrt 2, 8 at sqrt 3; for k inside such a shell the index order
    decides which points enter the covariance, so the reversed cloud gives other normals, and both equal the checker's"""
    rng = np.random.default_rng(33)
    g = np.arange(4, dtype=np.float32)
    lattice = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)[rng.permutation(64)]
    differs = 0
    for k in (3, 4, 5, 6, 9, 16, 17, 20):
        hp.cloud_index_build(lattice)
        a = _check(hp, lattice, k, 100.0, what="lattice")
        rev = np.ascontiguousarray(lattice[::-1])
        hp.cloud_index_build(rev)
        b = _check(hp, rev, k, 100.0, what="lattice reversed")
        differs += int((a["eig"].tobytes() != b["eig"][::-1].tobytes()))
    assert differs >= 4                                                              # the order of the indices did decide
    # copies of one point: D = 0 and C = 0 for all of them, line-like
    copies = np.tile(np.array([[1.5, -2, 3]], np.float32), (70, 1))
    hp.cloud_index_build(copies)
    for k in (2, 4, 5, 64):
        ref = _check(hp, copies, k, 1.0, what="copies")
        assert (ref["status"] == 3).all() and (ref["eig"] == 0.0).all() and (ref["curvature"] == 0.0).all() and (ref["count"] == k).all()


# ---- the boundary ----------------------------------------------------------------------------------------------------------------------------------
def test_max_dist_boundary(hp):
    cloud = np.array([[0, 0, 0], [1, 0, 0], [0, 2, 0]], np.float32)
    hp.cloud_index_build(cloud)
    ref = _check(hp, cloud, 2, 2.0, what="a neighbour at max_dist")
    assert ref["status"].tolist() == [0, 1, 1] and ref["count"].tolist() == [2, 1, 1]            # D == r2 counts
    ref = _check(hp, cloud, 2, np.nextafter(2.0, 0.0), what="max_dist one double below")
    assert ref["status"].tolist() == [1, 1, 1] and ref["count"].tolist() == [1, 1, 0]
    cloud[2, 1] = np.nextafter(np.float32(2.0), np.float32(3.0))                     # one float beyond
    hp.cloud_index_build(cloud)
    ref = _check(hp, cloud, 2, 2.0, what="a neighbour one float beyond max_dist")
    assert ref["status"].tolist() == [1, 1, 1] and ref["count"].tolist() == [1, 1, 0]
    assert (ref["normal"].view(np.uint32) == 0x7FC00000).all() and (ref["eig"] == -1.0).all() and (ref["curvature"] == -1.0).all()


# ---- the line gate -----------------------------------------------------------------------------------------------------------------------------------
def test_line_gate_at_its_edge(hp):
    """stars of four neighbours (+-a, 0, 0), (0, +-b, 0) round a point, far apart: C = diag(2 a a / 5, 2 b b / 5, 0) without a rotation, and with
    a = 2 b the two differ by the factor 4 exactly.  At min_ratio = 0.25 lambda_mid equals min_ratio lambda_hi and the star is refused; at the next
    double below 0.25 the product is the double below lambda_mid (lambda_mid is one ulp above it) and the star passes"""
    stars = []
    for centre, a, b in (((0, 0, 0), 2.0, 1.0), ((100, 0, 0), 1.0, 0.5), ((0, 100, 0), 4.0, 1.0), ((0, 0, 100), 1.0, 1.0)):
        c = np.array(centre, np.float64)
        stars += [c, c + [a, 0, 0], c - [a, 0, 0], c + [0, b, 0], c - [0, b, 0]]
    cloud = np.array(stars, np.float32)
    hp.cloud_index_build(cloud)
    at = ref = _check(hp, cloud, 4, 5.0, 0.25, what="lambda_mid == min_ratio lambda_hi")
    assert at["status"][[0, 5, 10, 15]].tolist() == [3, 3, 3, 0]
    for i in (0, 5):
        assert at["eig"][i, 1] == 0.25 * at["eig"][i, 2] and at["eig"][i, 0] == 0.0 and at["eig"][i, 1] > 0.0
    below = np.nextafter(0.25, 0.0)
    ref = _check(hp, cloud, 4, 5.0, below, what="lambda_mid one ulp above min_ratio lambda_hi")
    assert ref["status"][[0, 5, 10, 15]].tolist() == [0, 0, 3, 0]
    for i in (0, 5):
        assert ref["eig"][i, 1] == np.nextafter(below * ref["eig"][i, 2], np.inf) and ref["normal"][i].tolist() == [0.0, 0.0, 1.0]
    ref = _check(hp, cloud, 4, 5.0, 0.0, what="min_ratio 0")
    assert ref["status"][[0, 5, 10, 15]].tolist() == [0, 0, 0, 0]


# ---- the sign ----------------------------------------------------------------------------------------------------------------------------------------
def test_sign_rules(hp):
    grid = _plane_grid(5)
    hp.cloud_index_build(grid)
    for vp, z in (([9.0, -4.0, 0.0], 1.0), ([2.0, 2.0, 3.0], 1.0), ([2.0, 2.0, -3.0], -1.0), ([2.0, 2.0, 5e-324], 1.0), ([2.0, 2.0, -5e-324], -1.0)):
        ref = _check(hp, grid, 8, 100.0, 0.0, nk.VIEWPOINT, vp, what=("viewpoint", vp))     # in the tangent plane t == 0: the canonical sign stays
        assert (ref["normal"][:, 2] == z).all() and (ref["normal"][:, :2] == 0).all()
    # the planes x == y and x == -y: C_xx == C_yy gives theta == 0, t == 1 and a normal with |u_x| == |u_y| exactly: the lower component wins
    g = np.arange(5, dtype=np.float32)
    ij = np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2)
    for sy in (1.0, -1.0):
        cloud = np.stack([ij[:, 0], sy * ij[:, 0], ij[:, 1]], axis=1).astype(np.float32)
        hp.cloud_index_build(cloud)
        ref = _check(hp, cloud, 8, 100.0, what=("canonical tie", sy))
        n = ref["normal"]
        tie = np.abs(n[:, 0]) == np.abs(n[:, 1])
        assert (ref["status"] == 0).all() and tie.sum() >= 9 and (n[tie, 0] > 0).all() and (np.sign(n[tie, 1]) == -sy).all()
        _check(hp, cloud, 8, 100.0, 0.0, nk.VIEWPOINT, [-3.0, 2.0, 1.0], what=("canonical tie, viewpoint", sy))


# ---- far from the origin ---------------------------------------------------------------------------------------------------------------------------------
def test_far_from_the_origin(hp):
    cloud = noisy_sheet(offset=1e5)                                                  # floats 2^-7 apart: many exact ties, and offsets that are exact
    hp.cloud_index_build(cloud)
    for k in (6, 12):
        ref = _check(hp, cloud, k, 0.5, 0.01, what="sheet at 1e5")
        assert ref["counts"][0] > 300
    near = nk.normals(noisy_sheet(), 12, 0.5, 0.01)
    ok = (ref["status"] == 0) & (near["status"] == 0)
    cos = np.abs((ref["normal"][ok].astype(np.float64) * near["normal"][ok]).sum(axis=1))
    assert ok.sum() > 300 and np.median(cos) > 0.9                                   # the same sheet, up to the floats' spacing out there


# ---- cross-checks ------------------------------------------------------------------------------------------------------------------------------------
def test_cross_checks(hp):
    rng = np.random.default_rng(62)
    cloud = _cloud(rng, 3000)
    cloud[200:220] = cloud[100:120]                                                  # coincident pairs
    hp.cloud_index_build(cloud)
    for k in (4, 12, 40):
        lists = hp.knn_cloud(k, 0.9, want=("count", "index"))
        got = hp.cloud_normals(k, 0.9, 0.02)
        assert np.array_equal(got["count"], lists["count"]) and 0 < (got["count"] < k).sum() and ((got["count"] == k).sum() > 0 or k == 40)
        _same(got, nk.normals(cloud, k, 0.9, 0.02, lists=(lists["count"], lists["index"])), ("the device's own lists", k))
        assert got["with_normal"] > 1000
    # the cloud direction's faces are the closest query's
    vtx = rng.uniform(-5, 5, (400, 3)).astype(np.float32)
    faces = rng.integers(0, 400, (600, 3)).astype(np.int32)
    vtx[faces[:, 1]] = vtx[faces[:, 0]] + rng.uniform(-0.8, 0.8, (600, 3)).astype(np.float32)
    hp.raycast_build_triangles(vtx, faces)
    got = hp.normals_agree_cloud(0.7)
    has = hp.cloud_normals_get()[1] == 0
    near = hp.closest_points(cloud, 0.7, want=("face",))["face"]
    assert np.array_equal(got["face"][has], near[has]) and (got["face"][~has] == -1).all() and 100 < (near[has] >= 0).sum() < has.sum()


# ---- agreement -----------------------------------------------------------------------------------------------------------------------------------------
def _agreement_scene():
    """a square of two faces in z = 0, a zero-area face along y = 0 at z = 1, a face with a NaN vertex; cloud patches: over the square, beside the
    zero-area face (it is their closest face), far above everything, a lone point and a NaN point"""
    vtx = np.concatenate([SQUARE_V, np.array([[0, 0, 1], [2, 0, 1], [4, 0, 1], [np.nan, 1, 1]], np.float32)])
    faces = np.concatenate([SQUARE_F, np.array([[4, 5, 6], [0, 1, 7]], np.int32)])
    rng = np.random.default_rng(8)
    over = _plane_grid(15, 0.25, 0.05) + [0.25, 0.25, 0]
    over[:, 2] += rng.normal(0, 0.02, len(over))
    beside = _plane_grid(4, 0.2, 1.0) + [1.7, -1.3, 0]
    above = _plane_grid(4, 0.2, 10.0) + [1.0, 1.0, 0]
    cloud = np.concatenate([over, beside, above, [[30, 30, 30]], [[np.nan, 0, 0]]]).astype(np.float32)
    return vtx, faces, cloud[rng.permutation(len(cloud))]


def _stats_match(st, hist, want, want_hist, n):
    for key in ("n_points", "n_with_face", "n_not_finite", "n_no_face", "n_overflow", "max_dist"):
        assert getattr(st, key) == want[key], (key, getattr(st, key), want[key])
    assert np.array_equal(hist, want_hist) and int(hist.sum()) + st.n_overflow == st.n_with_face
    assert st.n_points == n == st.n_with_face + st.n_not_finite + st.n_no_face
    for key in ("sum_dist", "sum_dist2"):
        print(n, key, getattr(st, key), want[key], abs(getattr(st, key) - want[key]) / max(want[key], 1e-300), n * 2.0 ** -53)
        assert abs(getattr(st, key) - want[key]) <= n * 2.0 ** -53 * want[key], key
    m = st.n_with_face
    assert st.mean == (st.sum_dist / m if m else 0.0) and st.rms == (np.sqrt(st.sum_dist2 / m) if m else 0.0)


def test_agreement_both_directions(hp):
    vtx, faces, cloud = _agreement_scene()
    n = len(cloud)
    assert hp.raycast_build_triangles(vtx, faces)[2] == 3                            # the NaN face is not in the hierarchy
    hp.cloud_index_build(cloud)
    for mode, vp in ((nk.CANONICAL, None), (nk.VIEWPOINT, [2.0, 2.0, -7.0])):
        nrm = _check(hp, cloud, 8, 0.6, 0.02, mode, vp, what="agreement scene")
        assert nrm["counts"].tolist() == [n - 2, 1, 0, 1]
        # cloud direction
        got = hp.normals_agree_cloud(1.5)
        agree, face, pair, counts = nk.agree_cloud(cloud, nrm["normal"], nrm["status"], 1.5, vtx, faces)
        assert got["agree"].tobytes() == agree.tobytes() and got["face"].tobytes() == face.tobytes()
        assert [got[key] for key in ("pairs", "opposed", "no_pair", "not_finite")] == counts.tolist()
        assert counts[0] == 225 and counts[0] + counts[2] + counts[3] == n and counts[3] == 1 and (face == 2).sum() == 16 and not pair[face == 2].any()
        assert counts[1] == (225 if mode == nk.VIEWPOINT else 0)                     # the square's faces look up; the viewpoint lies below
        for bin_width, n_bins in ((0.01, 100), (0.3, 2), (1.0 / 2048, 2048)):
            _stats_match(*hp.normals_agree_stats(bin_width, n_bins), *nk.agree_stats(agree, pair, nrm["status"] == 2, bin_width, n_bins), n)
        st, _ = hp.normals_agree_stats(1.0, 1)
        assert st.mean > 0.95
        # samples direction
        xyz, sface = hp.mesh_sample(30.0, 5)
        index = hp.nearest_samples(0.2, want=("index",))["index"]
        got = hp.normals_agree_samples()
        agree, pair, counts = nk.agree_samples(sface, index, nrm["normal"], nrm["status"], vtx, faces)
        assert got["agree"].tobytes() == agree.tobytes() and [got[key] for key in ("pairs", "opposed", "no_pair", "not_finite")] == counts.tolist()
        assert counts[0] + counts[2] == len(xyz) and counts[3] == 0 and 100 < counts[0] < len(xyz) and counts[2] > 10 and set(sface.tolist()) == {0, 1}
        for bin_width, n_bins in ((0.01, 100), (0.3, 2)):
            _stats_match(*hp.normals_agree_stats(bin_width, n_bins), *nk.agree_stats(agree, pair, np.zeros(len(xyz), bool), bin_width, n_bins), len(xyz))
    # a caster without faces and an empty index are no errors
    hp.raycast_build_triangles(vtx, np.zeros((0, 3), np.int32))
    got = hp.normals_agree_cloud(1.5)
    assert (got["pairs"], got["no_pair"], got["not_finite"]) == (0, n - 1, 1) and (got["face"] == -1).all() and np.isnan(got["agree"]).all()
    assert hp.mesh_sample(30.0, 5, fetch=False) == 0
    hp.nearest_samples(0.2, want=())
    assert hp.normals_agree_samples()["agree"].shape == (0,) and hp.normals_agree_stats(0.1, 3)[0].n_points == 0
    hp.cloud_index_build(np.zeros((0, 3), np.float32))
    out = hp.cloud_normals(8, 1.0)
    assert out["normal"].shape == (0, 3) and (out["with_normal"], out["too_few"], out["line_like"], out["not_finite"]) == (0, 0, 0, 0)
    hp.raycast_build_triangles(SQUARE_V, SQUARE_F)
    assert hp.normals_agree_cloud(1.0)["pairs"] == 0 and hp.normals_agree_stats(0.1, 3)[0].n_points == 0


# ---- lifecycle -------------------------------------------------------------------------------------------------------------------------------------------
def test_lifecycle(hp):
    rng = np.random.default_rng(72)
    big, small = _cloud(rng, 4000), _cloud(rng, 70)
    hp.raycast_build_triangles(SQUARE_V, SQUARE_F)
    hp.cloud_index_build(big)
    hp.cloud_normals(64, 3.0)
    hp.normals_agree_cloud(3.0)
    hp.cloud_index_build(small)                                                      # from large to small: nothing of the larger call shows
    with pytest.raises(RuntimeError, match=r"rc=-1: .*no normals since"):
        hp.cloud_normals_get()                                                       # a build drops the normals
    with pytest.raises(RuntimeError, match=r"rc=-1: .*no normals since"):
        hp.normals_agree_cloud(3.0)
    with pytest.raises(RuntimeError, match=r"rc=-1: .*no agreement since"):
        hp.normals_agree_stats(0.1, 4)
    for k in (64, 16, 5, 2):
        a = hp.cloud_normals(k, 3.0)
        _same(a, nk.normals(small, k, 3.0), ("after a larger call", k))
        b = hp.cloud_normals(k, 3.0)
        assert all(a[key].tobytes() == b[key].tobytes() for key in KEYS)             # twice, the same bytes
    # the outlier state and the neighbour results are untouched by a normals call
    ref = kc.knn_cloud(small, 8, 5.0)
    hp.knn_cloud(8, 5.0, want=())
    hp.radius_count_cloud(2.0)
    hp.cloud_normals(5, 3.0, want=())
    hp.normals_agree_cloud(3.0, fetch=False)
    want = kc.statistical(ref[3], ref[0], np.isfinite(small).all(axis=1), 1.0)
    out = hp.cloud_outliers_statistical(1.0)
    assert (out["mu"], out["sigma"], out["threshold"]) == (want["mu"], want["sigma"], want["threshold"]) and np.array_equal(out["keep"], want["keep"])
    hp.cloud_normals(5, 3.0, want=())
    wr = kc.radius_rule(kc.radius_count_cloud(small, 2.0), np.isfinite(small).all(axis=1), 3)
    assert np.array_equal(hp.cloud_outliers_radius(3)["keep"], wr["keep"])
    hp.cloud_normals(5, 3.0, want=())                                                # between the mask and its apply
    kept = hp.cloud_index_apply_outliers()
    assert np.array_equal(kept, np.nonzero(wr["keep"])[0]) and 0 < len(kept) < len(small)
    with pytest.raises(RuntimeError, match=r"rc=-1: .*no normals since"):
        hp.cloud_normals_get()                                                       # an apply drops them as well
    with pytest.raises(RuntimeError, match=r"rc=-1: .*no normals since"):
        hp.normals_agree_cloud(3.0)
    _same(hp.cloud_normals(5, 3.0), nk.normals(small[kept], 5, 3.0), "after the apply")
    # a new normals call drops the agreement that read the old ones
    hp.normals_agree_cloud(3.0, fetch=False)
    hp.normals_agree_stats(0.1, 4)
    hp.cloud_normals(5, 3.0, want=())
    with pytest.raises(RuntimeError, match=r"rc=-1: .*no agreement since"):
        hp.normals_agree_stats(0.1, 4)


# ---- errors ------------------------------------------------------------------------------------------------------------------------------------------------
def test_argument_errors():
    lib = capi.load_hip_library()
    h, other = make_hip(lib, _small_cfg()), make_hip(lib, _small_cfg())
    try:
        P = C.c_void_p
        cn = lib.immesh_cloud_normals; cn.argtypes = [P, C.c_int32, C.c_double, C.c_double, C.c_int32] + [P] * 7; cn.restype = C.c_int
        get = lib.immesh_cloud_normals_get; get.argtypes = [P, P, P, C.c_int64, P]; get.restype = C.c_int
        ags = lib.immesh_normals_agree_samples; ags.argtypes = [P] * 4; ags.restype = C.c_int
        agc = lib.immesh_normals_agree_cloud; agc.argtypes = [P, P, C.c_double, P, P, P]; agc.restype = C.c_int
        red = lib.immesh_normals_agree_reduce; red.argtypes = [P, C.c_double, C.c_int32, P, P]; red.restype = C.c_int
        x, r = h.cloud_index(), h.raycaster()
        cloud = np.concatenate([_plane_grid(4), [[9, 9, 9]]]).astype(np.float32)

        def refused(rc, text, code=E_INVAL):
            assert rc == code and text in _err(h), (rc, _err(h))

        def args(k=4, max_dist=2.0, min_ratio=0.0, mode=0, vp=None):
            return (x, k, max_dist, min_ratio, mode, None if vp is None else np.array(vp, np.float64).ctypes.data_as(P)) + (None,) * 6

        for rc in (cn(*args()), get(x, None, None, 0, None), ags(x, r, None, None), agc(x, r, 1.0, None, None, None), red(x, 0.1, 4, None, None)):
            refused(rc, b"no index has been built")
        h.cloud_index_build(cloud)
        refused(get(x, None, None, 0, None), b"no normals since")
        refused(ags(x, r, None, None), b"no normals since")
        refused(agc(x, r, 1.0, None, None, None), b"no normals since")
        refused(red(x, 0.1, 4, None, None), b"no agreement since")

        def still_usable(normals=True):
            if normals:
                n, s = h.cloud_normals_get()
                assert s.tolist() == [0] * 16 + [1] and (n[:16] == [0, 0, 1]).all()
            assert h.knn_cloud(1, 100.0)["count"].tolist() == [1] * 17 and h.cloud_index_points().tobytes() == cloud.tobytes()
            assert h.nearest_points(cloud[:2], 10.0)["index"].tolist() == [0, 1]

        still_usable(False)
        assert h.cloud_normals(4, 2.0)["with_normal"] == 16
        for k in (1, 0, 65, -1):
            refused(cn(*args(k=k)), b"2 <= k <= 64")
        for d in (0.0, -1.0, np.inf, np.nan):
            refused(cn(*args(max_dist=d)), b"max_dist")
        for ratio in (-0.1, 1.0, 1.5, np.nan, np.inf, -np.inf):
            refused(cn(*args(min_ratio=ratio)), b"min_ratio")
        for mode in (2, -1):
            refused(cn(*args(mode=mode)), b"unknown mode")
        refused(cn(*args(mode=1)), b"viewpoint")
        for vp in ([np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf]):
            refused(cn(*args(mode=1, vp=vp)), b"viewpoint")
        assert cn(*args(mode=0, vp=[np.nan, 0, 0])) == 0                             # (read in viewpoint mode only)
        still_usable()                                                               # the refused calls left the normals as they were
        nrm, st = np.zeros((17, 3), np.float32), np.zeros(17, np.uint8)
        n = C.c_int64(-1)
        refused(get(x, nrm.ctypes.data_as(P), None, 16, C.byref(n)), b"cap 16 < 17 points", E_CAPACITY)
        assert n.value == 17
        refused(get(x, nrm.ctypes.data_as(P), st.ctypes.data_as(P), -1, None), b"cap is negative")
        # the caster
        refused(agc(x, None, 1.0, None, None, None), b"no caster")
        refused(ags(x, None, None, None), b"no caster")
        refused(agc(x, r, 1.0, None, None, None), b"no hierarchy has been built")
        refused(ags(x, r, None, None), b"no hierarchy has been built")
        other.raycast_build_triangles(SQUARE_V, SQUARE_F)
        refused(agc(x, other.raycaster(), 1.0, None, None, None), b"different contexts")
        refused(ags(x, other.raycaster(), None, None), b"different contexts")
        h.raycast_build_triangles(SQUARE_V, SQUARE_F)
        for d in (0.0, -1.0, np.inf, np.nan):
            refused(agc(x, r, d, None, None, None), b"max_dist")
        refused(ags(x, r, None, None), b"no samples since")
        h.mesh_sample(4.0, 1, fetch=False)
        refused(ags(x, r, None, None), b"no immesh_nearest_samples query")
        h.nearest_samples(1.0, want=())
        assert ags(x, r, None, None) == 0
        h.nearest_points(cloud[:3], 1.0)                                             # a point query is no query of the samples
        refused(ags(x, r, None, None), b"no immesh_nearest_samples query")
        h.nearest_samples(1.0, want=())
        h.mesh_sample(4.0, 2, fetch=False)                                           # sampled again: the query read the samples before
        refused(ags(x, r, None, None), b"no immesh_nearest_samples query")
        h.nearest_samples(1.0, want=())
        assert ags(x, r, None, None) == 0
        for bw, nb, text in ((0.0, 4, b"bin_width"), (np.nan, 4, b"bin_width"), (0.1, 0, b"n_bins"), (0.1, (1 << 20) + 1, b"n_bins")):
            refused(red(x, bw, nb, None, None), text)
        assert red(x, 0.1, 4, None, None) == 0 and agc(x, r, 1.0, None, None, None) == 0 and red(x, 0.1, 4, None, None) == 0
        still_usable()
        assert h.normals_agree_cloud(1.0)["pairs"] == 16
        t = h.normals_timing()
        assert len(t) == 3 and all(v > 0.0 for v in t)
    finally:
        h.close(); other.close()


# ---- scale -----------------------------------------------------------------------------------------------------------------------------------------------
def test_scale(hp):
    """20 000 points of a curved sheet, k = 16, with the KD-tree-assisted neighbour lists (tests/knn_checker.py: knn_tree)"""
    rng = np.random.default_rng(52)
    cloud = noisy_sheet(20000, seed=52) * np.float32(10.0)
    cloud[5000:5050] = cloud[4000:4050]                                              # coincident pairs
    cloud[77, 1] = np.nan
    cloud = cloud[rng.permutation(len(cloud))]
    hp.cloud_index_build(cloud)
    lists = kc.knn_tree(cloud, 16, 0.5, cloud, skip=np.arange(len(cloud)))[:2]
    got = hp.cloud_normals(16, 0.5, 0.01)
    print("20k points, k = 16: %.3f ms" % hp.normals_timing()[0])
    ref = nk.normals(cloud, 16, 0.5, 0.01, lists=lists)
    _same(got, ref, "scale")
    assert ref["counts"][0] > 19000 and ref["counts"][3] == 1 and 0 < (ref["count"] < 16).sum()


# ---- tools/mesh_eval.py ------------------------------------------------------------------------------------------------------------------------------------
def _sphere(n_lat=24, n_lon=48):
    """a latitude / longitude sphere of radius 1, wound outwards"""
    th = np.linspace(0, np.pi, n_lat + 1)[1:-1]
    ph = np.linspace(0, 2 * np.pi, n_lon, endpoint=False)
    ring = np.stack([np.outer(np.sin(th), np.cos(ph)), np.outer(np.sin(th), np.sin(ph)), np.outer(np.cos(th), np.ones(n_lon))], axis=-1).reshape(-1, 3)
    vtx = np.concatenate([ring, [[0, 0, 1], [0, 0, -1]]]).astype(np.float32)
    top, bottom = len(ring), len(ring) + 1
    faces = []
    for j in range(n_lon):
        j1 = (j + 1) % n_lon
        faces.append([top, j, j1])
        faces.append([bottom, (n_lat - 2) * n_lon + j1, (n_lat - 2) * n_lon + j])
        for i in range(n_lat - 2):
            a, b, c, d = i * n_lon + j, i * n_lon + j1, (i + 1) * n_lon + j, (i + 1) * n_lon + j1
            faces += [[a, c, d], [a, d, b]]
    return vtx, np.array(faces, np.int32)


def test_mesh_eval_carries_the_normals(hp):
    """a sphere against its own samples with --normals 12 --orient viewpoint: the figures the tool reports are the checker's over the checker's
    normals (a check that the plumbing carries the values, not a quality threshold)"""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import mesh_eval
    vtx, faces = _sphere()
    hp.raycast_build_triangles(vtx, faces)
    vp = [0.0, 0.0, 0.0]
    hp.topology_analyse()
    hp.topology_orient(capi.ORIENT_VIEWPOINT, vp)
    oriented = hp.topology_orient_faces()["faces"]                                   # what mesh_eval.orient is about to write over the caster's faces
    assert mesh_eval.orient(hp, "viewpoint", vp)["n_faces_flipped"] in (0, len(faces))   # one closed patch: it turns as a whole or not at all
    cloud, _ = hp.mesh_sample(150.0, 9)
    res = mesh_eval.evaluate(hp, cloud, tau=0.02, max_dist=0.5, density=100.0, seed=4, normals=dict(k=12, viewpoint=vp))
    # the same run with the checker's normals; the device's nearest indices are pinned by their own tests
    nrm = nk.normals(cloud, 12, 0.5, 0.0, nk.VIEWPOINT, vp, lists=kc.knn_tree(cloud, 12, 0.5, cloud, skip=np.arange(len(cloud)))[:2])
    xyz, sface = hp.mesh_sample(100.0, 4)
    index = hp.nearest_samples(0.5, want=("index",))["index"]
    agree, pair, _ = nk.agree_samples(sface, index, nrm["normal"], nrm["status"], vtx, oriented)
    want_com = np.abs(agree[pair].astype(np.float64)).mean()
    agree, _, pair, _ = nk.agree_cloud(cloud, nrm["normal"], nrm["status"], 0.5, vtx, oriented)
    want_acc = np.abs(agree[pair].astype(np.float64)).mean()
    print("normal consistency: accuracy %.6f completeness %.6f; opposed %.3f / %.3f" % (
        res["normal_consistency_accuracy"], res["normal_consistency_completeness"], res["normals"]["accuracy"]["opposed_share"],
        res["normals"]["completeness"]["opposed_share"]))
    assert res["normal_consistency_accuracy"] > want_acc - 1e-6 and res["normal_consistency_completeness"] > want_com - 1e-6
    # and not above either: the same floats summed in another order (each sum within n 2^-53 relative), and the two directions are not mixed up
    assert abs(res["normal_consistency_accuracy"] - want_acc) < 1e-9 and abs(res["normal_consistency_completeness"] - want_com) < 1e-9
    assert want_acc != want_com
    assert res["normal_consistency"] > 0.5 * (want_acc + want_com) - 1e-6 and res["normal_consistency"] > 0.97
    assert res["normals"]["with_normal"] == len(cloud) == nrm["counts"][0] and res["normals"]["accuracy"]["pairs"] == len(cloud)
    assert res["normals"]["completeness"]["pairs"] == len(xyz) == res["samples"] and len(index) == len(xyz)
    # the faces look at the centre and so do the normals: no pair is opposed
    assert res["normals"]["accuracy"]["opposed_share"] == 0.0 and res["normals"]["completeness"]["opposed_share"] == 0.0
    assert "normal_consistency" not in mesh_eval.evaluate(hp, cloud, tau=0.02, max_dist=0.5, density=100.0, seed=4)


# ---- the live path -------------------------------------------------------------------------------------------------------------------------------------------
def test_live_path_is_untouched():
    """a makes normals of the stream's own world points between scans and compares them with its live mesh; b never does: both go on with the same
    poses, planes and meshes"""
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
        lists = kc.knn_tree(cloud, 10, 1.0, cloud, skip=np.arange(len(cloud)))[:2]
        got = a.cloud_normals(10, 1.0, 0.01, nk.VIEWPOINT, [0.0, 0.0, 1.0])
        _same(got, nk.normals(cloud, 10, 1.0, 0.01, nk.VIEWPOINT, [0.0, 0.0, 1.0], lists=lists), "the stream's points")
        assert got["with_normal"] > len(cloud) // 2
        a.raycast_build_mesh(1.0, 20)
        out = a.normals_agree_cloud(1.0)
        assert out["pairs"] > 100 and a.normals_agree_stats(0.05, 20)[0].n_with_face == out["pairs"]
        a.mesh_sample(20.0, 1, fetch=False)
        a.nearest_samples(1.0, want=())
        assert a.normals_agree_samples()["pairs"] > 100
        assert compare_plane_tables_fast(planes, a.dump_planes(), 0.0) > 100 and a.counters() == counters
        for k in range(3, 5):
            scan(k)                                                                  # (asserts that a and b still agree)
        ea, eb = a.mesh_export(1.0, 20), b.mesh_export(1.0, 20)
        assert len(ea[1]) > 0 and ea[0].tobytes() == eb[0].tobytes() and ea[1].tobytes() == eb[1].tobytes()
        assert compare_plane_tables_fast(a.dump_planes(), b.dump_planes(), 0.0) > 100
    finally:
        a.close(); b.close()
