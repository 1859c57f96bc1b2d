"""Mesh-to-cloud distances on the device (include/immesh_nearest.h): the cloud index, the traversal, the sampler and the reduction against the
brute-force numpy restatement of the contract (tests/nearest_checker.py), bit for bit -- sizes at which the build and the query change path, rebuilds
of the index and the caster (one shared build) from large to small, equal and clustered codes, exact ties, the max_dist boundary, inputs that are
not finite, the cross-check against immesh_closest_points on the cloud as a soup of degenerate faces, the sampler on every size, the
device-resident path, statistics, the live mesh without side effects, determinism, argument errors, scale."""
import ctypes as C

import numpy as np
import pytest

import closest_checker as cc
import nearest_checker as nc
import raycast_checker as rcc
from immesh_amd import capi, synth
from conftest import make_hip
from parity_utils import compare_plane_tables_fast
from test_gpu_render import _rand_rot, _small_cfg, _soup

pytestmark = pytest.mark.gpu
I3, Z3 = np.eye(3), np.zeros(3)
KEYS = ("d2", "dist", "index", "xyz")
E_INVAL, E_CAPACITY = -1, -4


@pytest.fixture(scope="module")
def hp():
    h = make_hip(capi.load_hip_library(), _small_cfg())
    yield h
    h.close()


def _raw(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same(got, ref, what="", keys=KEYS):
    """device dict == checker tuple, bit for bit"""
    for k, r in zip(keys, ref):
        g = got[k]
        assert g.dtype == r.dtype and g.shape == r.shape, (what, k, g.dtype, r.dtype, g.shape, r.shape)
        if len(g) == 0:
            continue
        diff = np.nonzero((_raw(g).reshape(len(g), -1) != _raw(r).reshape(len(r), -1)).any(axis=1))[0]
        assert len(diff) == 0, (what, k, len(diff), len(g), diff[:5].tolist(), g[diff[:5]].tolist(), r[diff[:5]].tolist())


def _cloud(rng, n, spread=5.0):
    """n cloud points uniform in a cube; one NaN point and one infinite point when there is room"""
    c = rng.uniform(-spread, spread, (n, 3)).astype(np.float32)
    if n >= 60:
        c[7, 2] = np.nan
        c[n - 3, 0] = np.inf
    return c


def _queries(rng, cloud, n, near=0.05, spread=5.0):
    """n world queries: half of them within `near` of random finite cloud points, the rest uniform; a NaN query and a query 10^6 away"""
    q = rng.uniform(-spread, spread, (n, 3))
    fin = cloud[np.isfinite(cloud).all(axis=1)] if len(cloud) else cloud
    k = (n + 1) // 2
    if len(fin) and n:
        q[:k] = fin[rng.integers(len(fin), size=k)].astype(np.float64) + rng.uniform(-near, near, (k, 3)) / np.sqrt(3.0)
    q = q.astype(np.float32)
    if n >= 60:
        q[n - 1, 1] = np.nan
        q[n - 2] = [1e6, -1e6, 1e6]
    return q


def _local(pts, rot, pos):
    return ((pts.astype(np.float64) - pos) @ rot).astype(np.float32)


def _check(hp, rot, pos, pts, max_dist, cloud, ref=None, what=""):
    ref = nc.nearest(rot, pos, pts, max_dist, cloud) if ref is None else ref
    got = hp.nearest_points(pts, max_dist, None if rot is None else capi.ray_frame(rot, pos))
    _same(got, ref, what)
    return ref


def _err(h):
    f = h.lib.immesh_last_error; f.restype = C.c_char_p; f.argtypes = [C.c_void_p]
    return f(h.ctx)


def _as_soup(cloud):
    """the cloud as a soup of degenerate faces (i, i, i) for immesh_closest_points"""
    i = np.arange(len(cloud), dtype=np.int32)
    return cloud, np.stack([i, i, i], axis=-1)


# ---- sizes -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_cloud", [0, 1, 2, 3, 63, 64, 65, 257, 5000])
def test_sizes_match_checker(hp, n_cloud):
    rng = np.random.default_rng(300 + n_cloud)
    cloud = _cloud(rng, n_cloud)
    n_fin = int(np.isfinite(cloud).all(axis=1).sum())
    assert hp.cloud_index_build(cloud) == (n_cloud, n_fin)
    rot, pos = _rand_rot(rng), rng.uniform(-2, 2, 3)
    world = _queries(rng, cloud, 300)
    for frame, max_dist in ((None, 0.5), ((rot, pos), 0.5), (None, 100.0), ((rot, pos), 100.0)):
        r, p, pts = (None, None, world) if frame is None else (frame[0], frame[1], _local(world, *frame))
        ref = nc.nearest(r, p, pts, max_dist, cloud)
        if n_cloud:
            assert (ref[2] >= 0).sum() >= 100, (n_cloud, max_dist)                   # the checker first: the comparison is not one of misses alone
        else:
            assert (ref[2] < 0).all()
        assert ref[2][-1] == -1 and ref[2][-2] == -1
        _check(hp, r, p, pts, max_dist, cloud, ref, (n_cloud, max_dist, frame is not None))
    assert hp.nearest_points(np.zeros((0, 3), np.float32), 1.0)["index"].shape == (0,)


# ---- one build, two owners ------------------------------------------------------------------------------------------------------------------------
def test_rebuilds_of_both_owners_through_sizes(hp):
    """the caster and the cloud index of one context share one build: both rebuilt through a large tree, a single leaf, none, two, several workgroups
    and one wavefront, in that order, and queried after every rebuild -- a bound, a counter or a scratch buffer left over from the larger tree
    before, or a leaf count of 1 or 0 on the wrong branch, is a wrong bit here.  The soup of two faces has one with a NaN vertex: one leaf of two"""
    rng = np.random.default_rng(600)
    rot, pos = _rand_rot(rng), rng.uniform(-2, 2, 3)
    for n in (5000, 1, 0, 2, 257, 64):
        cloud = _cloud(rng, n)
        vtx, faces = _soup(rng, n, spread=5.0, size=0.4) if n else (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
        if n == 2:
            vtx[faces[1, 0], 1] = np.nan
        live = cc._soup(vtx, faces)[0]
        n_fin = int(np.isfinite(cloud).all(axis=1).sum())
        assert len(live) == len(rcc._soup(vtx, faces)[0]) and (len(live) < n if n in (5000, 2) else len(live) <= n)
        assert hp.raycast_build_triangles(vtx, faces) == (len(vtx), n, len(live))
        assert hp.cloud_index_build(cloud) == (n, n_fin)
        world = _queries(rng, cloud, 300)
        for r, p, pts, max_dist in ((None, None, world, 100.0), (rot, pos, _local(world, rot, pos), 2.0)):
            frame = None if r is None else capi.ray_frame(r, p)
            ref = cc.closest(r, p, pts, max_dist, vtx, faces)
            if max_dist == 100.0:                                                    # the checkers first: no comparison of misses alone
                assert (ref[2] >= 0).any() == (len(live) > 0), n
            _same(hp.closest_points(pts, max_dist, frame), ref, ("closest", n, max_dist), keys=("d2", "dist", "face", "xyz", "side"))
            ref = nc.nearest(r, p, pts, max_dist, cloud)
            assert (ref[2] >= 0).any() == (n_fin > 0), (n, max_dist)
            _same(hp.nearest_points(pts, max_dist, frame), ref, ("nearest", n, max_dist))
        dirs = rng.normal(size=(300, 3))
        if len(live):                                                                # half of the rays at the centroids of faces in the tree
            aim = vtx[faces[live[rng.integers(len(live), size=150)]]].astype(np.float64).mean(axis=1)
            dirs[:150] = (aim - pos) @ rot
        dirs = dirs.astype(np.float32)
        rt, rf = rcc.cast(rot, pos, dirs, None, 0.0, 200.0, vtx, faces)
        assert (rf >= 0).any() == (len(live) > 0), n
        t, f = hp.raycast(capi.ray_frame(rot, pos), dirs, None, 0.0, 200.0)
        assert np.array_equal(f, rf) and t.tobytes() == rt.tobytes(), (n, int((f != rf).sum()))


# ---- stack and build extremes --------------------------------------------------------------------------------------------------------------------
def test_copies_of_one_point(hp):
    """300 points with one Morton code and one D for every query: the keys differ in the position alone, and the lowest index wins"""
    rng = np.random.default_rng(1)
    cloud = np.tile(np.array([[0.25, -1.5, 3.0]], np.float32), (300, 1))
    assert hp.cloud_index_build(cloud) == (300, 300)
    pts = _queries(rng, cloud, 300, near=2.0)
    ref = _check(hp, None, None, pts, 50.0, cloud)
    assert (ref[2] >= 0).sum() >= 298 and set(ref[2].tolist()) == {-1, 0}


def test_clustered_codes(hp):
    """points at x = 2^-k, k = 0 .. 29: every split peels one point off, the deepest tree the code's 21 bits per axis allow, beside 200 random points"""
    rng = np.random.default_rng(2)
    k = np.arange(30)
    line = np.stack([2.0 ** -k, np.zeros(30), np.zeros(30)], axis=-1)
    cloud = np.concatenate([line, rng.uniform(0, 1, (200, 3))]).astype(np.float32)
    hp.cloud_index_build(cloud)
    pts = _queries(rng, cloud, 300, near=0.01, spread=1.0)
    pts[:30] = (line + [0, 0, 0.02 * 2.0 ** -29]).astype(np.float32)                  # one query at every peeled point
    pts[30:60] = (line + [0, 0, -3.0]).astype(np.float32)                            # and far below them: every box is open for a long time
    for max_dist in (10.0, 0.05):
        ref = _check(hp, None, None, pts, max_dist, cloud)
        assert len(set(ref[2][:30].tolist()) - {-1}) >= 10


def test_lopsided_cloud(hp):
    """1 far point and 999 in a 1 mm cube: the bounds stretch the codes so that the cube falls into very few cells"""
    rng = np.random.default_rng(3)
    cloud = np.concatenate([[[1000.0, -2000.0, 500.0]], 2.0 + rng.uniform(0, 1e-3, (999, 3))]).astype(np.float32)
    assert hp.cloud_index_build(cloud) == (1000, 1000)
    pts = np.concatenate([2.0 + rng.uniform(-1e-3, 2e-3, (250, 3)), rng.uniform(-3000, 3000, (50, 3))]).astype(np.float32)
    for max_dist in (1e-3, 1e4):
        ref = _check(hp, None, None, pts, max_dist, cloud)
        assert len(set(ref[2].tolist())) > 50
    assert 0 in ref[2].tolist()


# ---- exact ties --------------------------------------------------------------------------------------------------------------------------------------
def test_exact_ties_on_a_lattice(hp):
    """a unit lattice of 8^3 points queried at its cell centres (8 equidistant points) and face centres (4): the smallest index wins; the reversed
    cloud gives the same D and the smallest indices of the reversed order"""
    g = np.arange(8, dtype=np.float64)
    cloud = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float32)
    c = np.arange(7, dtype=np.float64) + 0.5
    cells = np.stack(np.meshgrid(c, c, c, indexing="ij"), axis=-1).reshape(-1, 3)
    faces = np.concatenate([np.stack(np.meshgrid(*[c if a != ax else g for a in range(3)], indexing="ij"), axis=-1).reshape(-1, 3) for ax in range(3)])
    pts = np.concatenate([cells, faces]).astype(np.float32)
    e = cloud.astype(np.float64)[None, :, :] - pts.astype(np.float64)[:, None, :]
    allD = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
    ties = (allD == allD.min(axis=1)[:, None]).sum(axis=1)
    assert (ties[:len(cells)] == 8).all() and (ties[len(cells):] == 4).all()
    hp.cloud_index_build(cloud)
    ref = _check(hp, None, None, pts, 2.0, cloud)
    assert np.array_equal(ref[2], np.argmax(allD == allD.min(axis=1)[:, None], axis=1))
    assert (ref[0][:len(cells)] == 0.75).all() and (ref[0][len(cells):] == 0.5).all()
    rev = cloud[::-1].copy()
    hp.cloud_index_build(rev)
    ref2 = _check(hp, None, None, pts, 2.0, rev)
    assert ref2[0].tobytes() == ref[0].tobytes() and ref2[1].tobytes() == ref[1].tobytes()
    want = np.array([(len(cloud) - 1 - np.nonzero(row == row.min())[0]).min() for row in allD])
    assert np.array_equal(ref2[2], want)


# ---- the max_dist boundary ------------------------------------------------------------------------------------------------------------------------------
def test_max_dist_boundary(hp):
    q = np.zeros((2, 3), np.float32)
    cloud = np.array([[0, 0, 2]], np.float32)
    hp.cloud_index_build(cloud)
    ref = _check(hp, None, None, q, 2.0, cloud)
    assert ref[2].tolist() == [0, 0] and ref[0].tolist() == [4.0, 4.0] and ref[1].tolist() == [2.0, 2.0]      # D == r2 counts
    far = np.array([[0, 0, np.nextafter(np.float32(2.0), np.float32(3.0))]], np.float32)                     # the cloud point one float further away
    hp.cloud_index_build(far)
    ref = _check(hp, None, None, q, 2.0, far)
    assert ref[2].tolist() == [-1, -1] and ref[0].tolist() == [-1.0, -1.0]
    # the next double above D: the frame lowers the query by one unit in the last place of 2
    hp.cloud_index_build(cloud)
    up = np.nextafter(2.0, 3.0)
    for z, want in ((0.0, 0), (2.0 - up, -1), (4.0, 0), (np.nextafter(4.0, 5.0), -1)):
        ref = _check(hp, I3, np.array([0.0, 0.0, z]), q, 2.0, cloud)
        assert ref[2].tolist() == [want, want], z
    # with more than one point: the same boundary inside a tree
    many = np.concatenate([cloud, far, [[0, 0, -2], [3, 0, 0]]]).astype(np.float32)
    hp.cloud_index_build(many)
    ref = _check(hp, None, None, q, 2.0, many)
    assert ref[2].tolist() == [0, 0]
    ref = _check(hp, None, None, q + np.float32(1e-3), 2.0, many)
    assert ref[2].tolist() == [0, 0] and ref[0][0] < 4.0


# ---- inputs that are not finite ---------------------------------------------------------------------------------------------------------------------------
def test_inputs_that_are_not_finite(hp):
    rng = np.random.default_rng(4)
    cloud = _cloud(rng, 400)
    cloud[rng.choice(400, 60, replace=False), rng.integers(0, 3, 60)] = rng.choice([np.nan, np.inf, -np.inf], 60)
    n_fin = int(np.isfinite(cloud).all(axis=1).sum())
    assert hp.cloud_index_build(cloud) == (400, n_fin) and n_fin < 345
    pts = _queries(rng, cloud, 300)
    pts[rng.choice(300, 40, replace=False), rng.integers(0, 3, 40)] = rng.choice([np.nan, np.inf, -np.inf], 40)
    ref = _check(hp, None, None, pts, 3.0, cloud)
    assert np.isfinite(cloud[ref[2][ref[2] >= 0]]).all()
    st, _ = hp.nearest_stats(0.1, 10)
    want, _ = nc.stats(None, None, pts, ref[1], ref[2], 0.1, 10)
    assert (st.n_points, st.n_with_face, st.n_not_finite, st.n_no_face) == (300, want["n_with_face"], want["n_not_finite"], want["n_no_face"])
    assert st.n_not_finite >= 30 and st.n_with_face >= 100
    # a frame that carries queries beyond 2^128: not finite by rule
    big = np.array([[2.0 ** 30, 0, 0], [1.0, 0, 0], [0, 2.0 ** 29, 0]], np.float32)
    for scale, n_bad in ((2.0 ** 100, 2), (2.0 ** 97, 0)):
        ref = _check(hp, I3 * scale, Z3, big, 3.0, cloud)
        st, _ = hp.nearest_stats(0.1, 10)
        assert st.n_not_finite == n_bad == int((~nc.points(I3 * scale, Z3, big)[1]).sum())
    # a cloud without a finite point: an empty index
    hp.cloud_index_build(np.full((5, 3), np.nan, np.float32))
    ref = _check(hp, None, None, pts, 3.0, np.full((5, 3), np.nan, np.float32))
    assert (ref[2] == -1).all()


# ---- the cross-check with the closest-face traversal ---------------------------------------------------------------------------------------------------------
def test_cross_check_with_closest_points(hp):
    rng = np.random.default_rng(5)
    cloud = _cloud(rng, 3000)
    pts = _queries(rng, cloud, 5000, near=0.2)
    hp.cloud_index_build(cloud)
    hp.raycast_build_triangles(*_as_soup(cloud))
    for frame, max_dist in ((None, 0.7), (capi.ray_frame(_rand_rot(rng), rng.uniform(-1, 1, 3)), 2.0)):
        a = hp.nearest_points(pts, max_dist, frame)
        b = hp.closest_points(pts, max_dist, frame, want=("d2", "dist", "face"))
        assert a["d2"].tobytes() == b["d2"].tobytes() and a["dist"].tobytes() == b["dist"].tobytes() and np.array_equal(a["index"], b["face"])
        assert 1000 < (a["index"] >= 0).sum() < 5000


# ---- the sampler ---------------------------------------------------------------------------------------------------------------------------------------------
def _check_samples(hp, vtx, faces, density, seed, what=""):
    ref = nc.sample(vtx, faces, density, seed)
    xyz, face = hp.mesh_sample(density, seed)
    _same({"xyz": xyz, "face": face}, ref, what, keys=("xyz", "face"))
    assert hp.mesh_sample(density, seed, fetch=False) == len(ref[0])
    return ref


@pytest.mark.parametrize("n_faces", [0, 1, 2, 255, 256, 257, 3000])
def test_sampler_matches_checker(hp, n_faces):
    rng = np.random.default_rng(400 + n_faces)
    vtx, faces = _soup(rng, n_faces, size=0.4) if n_faces else (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    hp.raycast_build_triangles(vtx, faces)
    seen = set()
    for density in (10.0, 60.0):
        for seed in (0, 0xFEDCBA9876543210):
            xyz, face = _check_samples(hp, vtx, faces, density, seed, (n_faces, density, seed))
            seen.add(xyz.tobytes())
            if n_faces:
                assert len(xyz) > 0 and np.all(np.diff(face) >= 0)
            else:
                assert len(xyz) == 0
    assert len(seen) == (4 if n_faces else 1)                                        # the seed and the density both matter


def test_sampler_integer_counts_and_faces_without_samples(hp):
    # x is an exact integer: legs 1 and 2^k, density 2 -> x = 2^k
    vtx = np.array([[0, 0, 0], [1, 0, 0], [0, 4, 0], [0, 0, 64]], np.float32)
    faces = np.array([[0, 1, 2], [0, 1, 3], [0, 2, 3]], np.int32)
    hp.raycast_build_triangles(vtx, faces)
    for seed in (0, 1, 2):
        xyz, face = _check_samples(hp, vtx, faces, 2.0, seed)
        assert np.bincount(face).tolist() == [4, 64, 256]
    # zero area, NaN vertices, faces of one point, between faces that have samples
    rng = np.random.default_rng(6)
    vtx = np.concatenate([rng.uniform(-2, 2, (30, 3)), [[np.nan, 0, 0], [0, np.inf, 0]]]).astype(np.float32)
    faces = rng.integers(0, 30, (200, 3)).astype(np.int32)
    faces[::4, 1] = faces[::4, 0]                                                     # a repeated vertex
    faces[1::8] = faces[1::8, :1]                                                     # a single point
    faces[2::10, 2] = 30 + (np.arange(len(faces[2::10])) % 2)                         # a vertex that is not finite
    hp.raycast_build_triangles(vtx, faces)
    xyz, face = _check_samples(hp, vtx, faces, 5.0, 9)
    k = np.bincount(face, minlength=200)
    assert (k[::4] == 0).all() and (k[1::8] == 0).all() and (k[2::10] == 0).all() and (k > 0).sum() > 80
    # an index out of range cannot reach the caster through immesh_raycast_build_triangles (it refuses the soup and keeps its snapshot); the rule
    # for such faces (the live mesh's export may hold them) is the checker's, tests/test_nearest_cpu.py
    bad = faces.copy()
    bad[3, 1] = 32
    with pytest.raises(RuntimeError, match=r"rc=-1: .*out of range"):
        hp.raycast_build_triangles(vtx, bad)
    assert nc.counts(vtx, bad, 5.0, 9)[3] == 0


def test_sampler_capacity(hp):
    vtx = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 3]], np.float32)
    faces = np.array([[0, 1, 2], [0, 1, 3]], np.int32)
    hp.raycast_build_triangles(vtx, faces)
    hp.cloud_index_build(vtx)
    ref = nc.sample(vtx, faces, 100.0, 1)
    n = len(ref[0])
    assert n == 200
    f = hp.lib.immesh_mesh_sample
    f.argtypes = [C.c_void_p, C.c_double, C.c_uint64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]; f.restype = C.c_int
    xyz, face, got = np.zeros((n, 3), np.float32), np.zeros(n, np.int32), C.c_int64(0)
    assert f(hp.raycaster(), 100.0, 1, xyz.ctypes.data_as(C.c_void_p), None, n - 1, C.byref(got)) == E_CAPACITY and got.value == n    # cap one below the count
    assert b"cap" in _err(hp)
    assert f(hp.raycaster(), 100.0, 1, None, face.ctypes.data_as(C.c_void_p), n - 1, None) == E_CAPACITY
    assert f(hp.raycaster(), 100.0, 1, xyz.ctypes.data_as(C.c_void_p), face.ctypes.data_as(C.c_void_p), n, None) == 0
    _same({"xyz": xyz, "face": face}, ref, keys=("xyz", "face"))
    # a density that saturates one face (x >= 2^31), one that makes x infinite, and a total of 2^31 without a saturated face
    for density in (1e10, 1.7e308, 2.0 ** 30):
        with pytest.raises(nc.TooManySamples):
            nc.sample(vtx, faces, density, 1)
        assert f(hp.raycaster(), density, 1, None, None, 0, C.byref(got)) == E_CAPACITY
        assert b"too many samples" in _err(hp)
        with pytest.raises(RuntimeError, match=r"rc=-1: .*no samples"):              # a refused sampling leaves no samples behind
            hp.nearest_samples(1.0)
        _check_samples(hp, vtx, faces, 100.0, 1)                                       # the caster stays usable
        t, fc = hp.raycast(capi.ray_frame(pos=[0.25, 0.25, 1.0]), np.array([[0, 0, -1]], np.float32), None, 0.0, 10.0)
        assert t.tolist() == [1.0] and fc.tolist() == [0]


def test_samples_lie_on_their_faces(hp):
    """every sample is within 2^-22 M of its own soup, M the largest coordinate magnitude: the sample is a point of the face in double (to 2^-50 M)
    whose three coordinates are rounded to float, each by at most 2^-24 M, sqrt(3) 2^-24 M in all -- below 2^-22 M with a factor 2 to spare"""
    rng = np.random.default_rng(7)
    vtx, faces = _soup(rng, 2000, size=0.5)
    hp.raycast_build_triangles(vtx, faces)
    xyz, face = hp.mesh_sample(20.0, 3)
    assert len(xyz) > 3000
    M = float(np.abs(vtx[np.isfinite(vtx)]).max())
    got = hp.closest_points(xyz, 1.0, want=("dist", "face"))
    print("samples", len(xyz), "largest distance to the soup", float(got["dist"].max()), "bound", 2.0 ** -22 * M)
    assert (got["face"] >= 0).all() and (got["dist"] <= np.float32(2.0 ** -22 * M)).all()
    # ... and within the same bound of the face it names
    tri = vtx[faces[face]]
    D = cc.pair(xyz.astype(np.float64), tri)[0]
    assert (np.sqrt(D) <= 2.0 ** -22 * M).all()


# ---- the device-resident path ------------------------------------------------------------------------------------------------------------------------------
def test_samples_queried_where_they_lie(hp):
    rng = np.random.default_rng(8)
    cloud = _cloud(rng, 4000, spread=20.0)
    hp.cloud_index_build(cloud)
    sizes = []
    for n_faces, density in ((3000, 10.0), (500, 4.0), (3000, 25.0)):                # a smaller set after a larger one: grow-only buffers keep no stale samples
        vtx, faces = _soup(rng, n_faces, size=0.4)
        hp.raycast_build_triangles(vtx, faces)
        with pytest.raises(RuntimeError, match=r"rc=-1: .*no samples"):
            hp.nearest_samples(2.0)                                                  # the samples of the previous snapshot are gone
        xyz, face = hp.mesh_sample(density, 12)
        a = hp.nearest_samples(2.0)
        sa, ha = hp.nearest_stats(0.05, 50)
        b = hp.nearest_points(xyz, 2.0)
        sb, hb = hp.nearest_stats(0.05, 50)
        assert all(a[k].tobytes() == b[k].tobytes() and a[k].shape == b[k].shape for k in KEYS)
        assert bytes(sa) == bytes(sb) and ha.tobytes() == hb.tobytes() and sa.n_points == len(xyz)
        _same(a, nc.nearest(None, None, xyz, 2.0, cloud), n_faces)
        assert 0 < (a["index"] >= 0).sum() < len(xyz)
        sizes.append(len(xyz))
    assert sizes[1] < sizes[0] < sizes[2]


# ---- statistics ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stats_case():
    rng = np.random.default_rng(9)
    cloud = _cloud(rng, 2000, spread=10.0)
    pts = _queries(rng, cloud, 50000, near=0.3, spread=10.0)
    pts[100:200, 0] = np.inf
    ref = nc.nearest(None, None, pts, 1.0, cloud)
    return cloud, pts, ref


@pytest.mark.parametrize("n_pts", [1, 64, 65, 50000])
def test_stats_match_checker(hp, stats_case, n_pts):
    cloud, pts, ref = stats_case
    pts = pts[len(pts) - n_pts:] if n_pts > 1 else pts[:1]
    ref = tuple(r[len(r) - n_pts:] if n_pts > 1 else r[:1] for r in ref)
    hp.cloud_index_build(cloud)
    _check(hp, None, None, pts, 1.0, cloud, ref)
    for n_bins, bin_width in ((1, 0.25), (7, 0.1), (1024, 1.0 / 1024), (1025, 1.0 / 1024), (1024, 1e-4)):
        want, hist = nc.stats(None, None, pts, ref[1], ref[2], bin_width, n_bins)
        st, h = hp.nearest_stats(bin_width, n_bins)
        for k in ("n_points", "n_with_face", "n_not_finite", "n_no_face", "n_overflow", "max_dist"):
            assert getattr(st, k) == want[k], (k, getattr(st, k), want[k])
        assert np.array_equal(h, hist) and int(h.sum()) + st.n_overflow == st.n_with_face
        assert st.n_points == n_pts == st.n_with_face + st.n_not_finite + st.n_no_face
        bound = n_pts * 2.0 ** -53
        for k in ("sum_dist", "sum_dist2"):
            print(n_pts, n_bins, k, getattr(st, k), want[k], abs(getattr(st, k) - want[k]) / max(want[k], 1e-300), bound)
            assert abs(getattr(st, k) - want[k]) <= bound * want[k], k
        n = st.n_with_face
        assert st.mean == (st.sum_dist / n if n else 0.0) and st.rms == (np.sqrt(st.sum_dist2 / n) if n else 0.0)
        assert st.bin_width == np.float32(bin_width)
        st2, h2 = hp.nearest_stats(bin_width, n_bins)
        assert bytes(st) == bytes(st2) and h.tobytes() == h2.tobytes()
    if n_pts == 50000:
        assert want["n_with_face"] > 20000 and want["n_no_face"] > 1000 and want["n_not_finite"] == 101 and want["n_overflow"] > 0


# ---- the live mesh -----------------------------------------------------------------------------------------------------------------------------------------------
def test_live_mesh_without_side_effects():
    """a samples its snapshot of the live mesh between scans and queries the samples against the stream's own world points, b never does: a's samples
    equal the checker's on the exported arrays, rays and closest-face queries keep their answers, and both contexts go on with the same bits"""
    lib = capi.load_hip_library()
    cfg = capi.avia_config(cap_root_voxels=1 << 15, cap_scan_points=100000)
    a, b = make_hip(lib, cfg), make_hip(lib, cfg)
    try:
        extT = np.array(list(cfg.extT))
        world_pts = []

        def scan(k):
            R, t = synth.trajectory_pose(k)
            raw = synth.livox_scan(k, R, t, n_pts=20000, extT=extT)
            world_pts.append(((raw[::4, :3].astype(np.float64) + extT) @ R.T + t).astype(np.float32))
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

        for k in range(4):
            state = scan(k)
        nv, nf, n_in = a.raycast_build_mesh(1.0, 20)
        vtx, faces = a.mesh_export(1.0, 20)
        assert (nv, nf) == (len(vtx), len(faces)) and 0 < n_in <= nf
        planes, counters = a.dump_planes(), a.counters()
        frame = a.ray_frame_from_state(state)
        dirs = np.random.default_rng(0).normal(size=(2000, 3)).astype(np.float32)
        rays = a.raycast(frame, dirs, None, 0.5, 100.0)
        cloud = np.concatenate(world_pts)
        closest = a.closest_points(cloud[::5], 1.0)
        # sample, index the stream's own points, query
        xyz, face = a.mesh_sample(20.0, 5)
        _same({"xyz": xyz, "face": face}, nc.sample(vtx, faces, 20.0, 5), "samples of the live mesh", keys=("xyz", "face"))
        assert len(xyz) > 1000
        assert a.cloud_index_build(cloud)[0] == len(cloud)
        got = a.nearest_samples(1.0)
        _same(got, nc.nearest(None, None, xyz, 1.0, cloud), "samples against the scans")
        st, _ = a.nearest_stats(0.01, 100)
        print("mesh-to-scan: %d of %d samples with a neighbour, mean %.4f m, rms %.4f m, max %.4f m" % (st.n_with_face, st.n_points, st.mean, st.rms, st.max_dist))
        assert st.n_with_face > len(xyz) // 2
        # rays and closest faces still give their old answers; the maps are untouched
        again = a.raycast(frame, dirs, None, 0.5, 100.0)
        assert again[0].tobytes() == rays[0].tobytes() and again[1].tobytes() == rays[1].tobytes() and (rays[1] >= 0).sum() > 100
        again = a.closest_points(cloud[::5], 1.0)
        assert all(again[k].tobytes() == closest[k].tobytes() for k in closest)
        assert compare_plane_tables_fast(planes, a.dump_planes(), 0.0) > 100 and a.counters() == counters
        for k in range(4, 6):
            scan(k)                                                                  # (asserts that a and b still agree)
            assert all(a.nearest_samples(1.0)[key].tobytes() == got[key].tobytes() for key in KEYS)      # the old snapshot's samples, the old bits
        ea, eb = a.mesh_export(1.0, 20), b.mesh_export(1.0, 20)
        assert len(ea[1]) != len(faces) and ea[0].tobytes() == eb[0].tobytes() and ea[1].tobytes() == eb[1].tobytes()
        assert compare_plane_tables_fast(a.dump_planes(), b.dump_planes(), 0.0) > 100
    finally:
        a.close(); b.close()


# ---- determinism, errors, scale --------------------------------------------------------------------------------------------------------------------------------
def test_deterministic():
    lib = capi.load_hip_library()
    a, b = make_hip(lib, _small_cfg()), make_hip(lib, _small_cfg())
    try:
        rng = np.random.default_rng(41)
        cloud = _cloud(rng, 20000, spread=10.0)
        vtx, faces = _soup(rng, 5000, spread=10.0, size=0.4)
        pts = _queries(rng, cloud, 20000, near=0.5, spread=10.0)
        a.cloud_index_build(cloud); a.raycast_build_triangles(vtx, faces)
        ra = a.nearest_points(pts, 2.0); sa, ha = a.nearest_stats(0.05, 64)
        xa = a.mesh_sample(15.0, 77); qa = a.nearest_samples(2.0)
        b.cloud_index_build(_cloud(rng, 3000)); b.raycast_build_triangles(*_soup(rng, 700))   # b: another cloud, soup and query first, then these twice
        b.nearest_points(pts[:777], 5.0); b.mesh_sample(3.0, 1)
        for _ in range(2):
            b.cloud_index_build(cloud); b.raycast_build_triangles(vtx, faces)
            rb = b.nearest_points(pts, 2.0); sb, hb = b.nearest_stats(0.05, 64)
            xb = b.mesh_sample(15.0, 77); qb = b.nearest_samples(2.0)
            assert all(ra[k].tobytes() == rb[k].tobytes() and qa[k].tobytes() == qb[k].tobytes() for k in KEYS)
            assert bytes(sa) == bytes(sb) and ha.tobytes() == hb.tobytes() and xa[0].tobytes() == xb[0].tobytes() and xa[1].tobytes() == xb[1].tobytes()
        assert (ra["index"] >= 0).sum() > 5000 and len(xa[0]) > 5000
    finally:
        a.close(); b.close()


def test_argument_errors():
    lib = capi.load_hip_library()
    h, other = make_hip(lib, _small_cfg()), make_hip(lib, _small_cfg())
    try:
        vtx = np.array([[-1, -1, -2], [1, -1, -2], [0, 1, -2]], np.float32)
        faces = np.array([[0, 1, 2]], np.int32)
        cloud = np.array([[0, 0, -2], [0, 0, 3]], np.float32)
        pts = np.array([[0, 0, 0], [0, 0, 2]], np.float32)
        with pytest.raises(RuntimeError, match=r"rc=-1: .*no index has been built"):
            h.nearest_points(pts, 10.0)                                              # a query before a build
        with pytest.raises(RuntimeError, match=r"rc=-1: .*built"):
            h.mesh_sample(1.0, 0)                                                    # samples before a caster is built
        h.raycast_build_triangles(vtx, faces)
        with pytest.raises(RuntimeError, match=r"rc=-1: .*no index has been built"):
            h.mesh_sample(1.0, 0); h.nearest_samples(10.0)                           # the samples exist, the index does not
        h.cloud_index_build(cloud)
        with pytest.raises(RuntimeError, match=r"rc=-1: .*no nearest-point query"):
            h.nearest_stats(0.1, 4)                                                  # the reduction before a query

        def still_usable():
            r = h.nearest_points(pts, 10.0)
            assert r["dist"].tolist() == [2.0, 1.0] and r["index"].tolist() == [0, 1] and r["d2"].tolist() == [4.0, 1.0]
            assert r["xyz"].tolist() == [[0, 0, -2], [0, 0, 3]]
            st, hist = h.nearest_stats(1.0, 2)
            assert (st.n_points, st.n_with_face, st.n_overflow, st.max_dist, st.sum_dist, st.sum_dist2) == (2, 2, 1, 2.0, 3.0, 5.0) and hist.tolist() == [0, 1]
            xyz, face = h.mesh_sample(4.0, 3)                                        # area 2, x = 8
            assert len(xyz) == 8 and (xyz[:, 2] == -2).all() and face.tolist() == [0] * 8
            s = h.nearest_samples(10.0)
            assert s["index"].tolist() == [0] * 8
            t, f = h.raycast(capi.ray_frame(), np.array([[0, 0, -1]], np.float32), None, 0.0, 10.0)
            assert t.tolist() == [2.0] and f.tolist() == [0]

        still_usable()
        for max_dist in (0.0, -1.0, np.inf, np.nan):
            with pytest.raises(RuntimeError, match=r"rc=-1: .*max_dist"):
                h.nearest_points(pts, max_dist)
            with pytest.raises(RuntimeError, match=r"rc=-1: .*max_dist"):
                h.nearest_samples(max_dist)
            still_usable()
        for density in (0.0, -1.0, np.inf, np.nan):
            with pytest.raises(RuntimeError, match=r"rc=-1: .*density"):
                h.mesh_sample(density, 0)
            still_usable()
        for bad in (capi.ray_frame(pos=[np.nan, 0, 0]), capi.ray_frame(rot=np.diag([1.0, np.inf, 1.0]))):
            with pytest.raises(RuntimeError, match=r"rc=-1: .*finite"):
                h.nearest_points(pts, 10.0, bad)
            still_usable()
        f = h.lib.immesh_nearest_points
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_double] + [C.c_void_p] * 4; f.restype = C.c_int
        g = h.lib.immesh_cloud_index_build; g.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]; g.restype = C.c_int
        for n in (-1, 2 ** 31 - 1, 2 ** 40):
            assert f(h.cloud_index(), None, pts.ctypes.data_as(C.c_void_p), n, 10.0, None, None, None, None) == E_INVAL
            assert b"point array" in _err(h)
            assert g(h.cloud_index(), cloud.ctypes.data_as(C.c_void_p), n) == E_INVAL      # a refused build leaves the index as it was
            assert b"point array" in _err(h)
            still_usable()
        assert g(h.cloud_index(), cloud.ctypes.data_as(C.c_void_p), 2 ** 30 + 1) == E_INVAL and b"2^30" in _err(h)
        assert g(h.cloud_index(), None, 2) == E_INVAL
        still_usable()
        assert f(h.cloud_index(), None, None, 2, 10.0, None, None, None, None) == E_INVAL
        assert f(h.cloud_index(), None, None, 0, 10.0, None, None, None, None) == 0         # no points, no array
        assert f(h.cloud_index(), None, pts.ctypes.data_as(C.c_void_p), 2, 10.0, None, None, None, None) == 0     # every output may be NULL
        for bin_width, n_bins, text in ((0.0, 4, "bin_width"), (-1.0, 4, "bin_width"), (np.inf, 4, "bin_width"), (np.nan, 4, "bin_width"), (0.1, 0, "n_bins"),
                                        (0.1, -3, "n_bins"), (0.1, (1 << 20) + 1, "n_bins")):
            with pytest.raises(RuntimeError, match=r"rc=-1: .*" + text):
                h.nearest_stats(bin_width, n_bins)
            still_usable()
        # the caster of another context
        other.raycast_build_triangles(vtx, faces)
        other.mesh_sample(4.0, 3)
        s = h.lib.immesh_nearest_samples; s.argtypes = [C.c_void_p, C.c_void_p, C.c_double] + [C.c_void_p] * 4; s.restype = C.c_int
        assert s(h.cloud_index(), other.raycaster(), 10.0, None, None, None, None) == E_INVAL and b"different contexts" in _err(h)
        assert s(h.cloud_index(), None, 10.0, None, None, None, None) == E_INVAL
        still_usable()
        assert s(h.cloud_index(), h.raycaster(), 10.0, None, None, None, None) == 0         # every output may be NULL
        # samples made before a _samples query: a rebuilt caster has none
        h.raycast_build_triangles(vtx, faces)
        with pytest.raises(RuntimeError, match=r"rc=-1: .*no samples"):
            h.nearest_samples(10.0)
        still_usable()
        # an empty index and a caster without faces are no errors
        assert h.cloud_index_build(np.zeros((0, 3), np.float32)) == (0, 0)
        r = h.nearest_points(pts, 10.0)
        assert r["index"].tolist() == [-1, -1] and r["dist"].tolist() == [-1.0, -1.0]
        st, _ = h.nearest_stats(1.0, 3)
        assert (st.n_with_face, st.n_no_face, st.mean, st.rms, st.max_dist) == (0, 2, 0.0, 0.0, 0.0)
        h.raycast_build_triangles(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
        xyz, face = h.mesh_sample(10.0, 0)
        assert len(xyz) == 0 and h.nearest_samples(1.0)["index"].shape == (0,)
        h.raycast_build_triangles(vtx, faces); h.cloud_index_build(cloud)
        still_usable()
    finally:
        h.close(); other.close()


def test_scale(hp):
    """a 200 000-point cloud x 100 000 queries: all of them against immesh_closest_points on the cloud as degenerate faces, a random 2 000 against
    every cloud point in numpy"""
    rng = np.random.default_rng(51)
    cloud = _cloud(rng, 200000, spread=30.0)
    assert hp.cloud_index_build(cloud) == (200000, 199998)
    pts = _queries(rng, cloud, 100000, near=0.3, spread=30.0)
    got = hp.nearest_points(pts, 3.0)
    print("200k points x 100k queries: build %.3f ms, query %.3f ms; with a neighbour %.3f" % (hp.nearest_timing()[:2] + ((got["index"] >= 0).mean(),)))
    have = got["index"] >= 0
    assert have.mean() > 0.9
    hp.raycast_build_triangles(*_as_soup(cloud))
    other = hp.closest_points(pts, 3.0, want=("d2", "dist", "face"))
    assert got["d2"].tobytes() == other["d2"].tobytes() and got["dist"].tobytes() == other["dist"].tobytes() and np.array_equal(got["index"], other["face"])
    pick = rng.choice(len(pts), 2000, replace=False)
    _same({k: got[k][pick] for k in KEYS}, nc.nearest(None, None, pts[pick], 3.0, cloud), "a random 2 000")
    assert got["xyz"][have].tobytes() == cloud[got["index"][have]].tobytes()
    assert (got["d2"][~have] == -1.0).all() and np.isnan(got["xyz"][~have]).all()


# ---- tools/mesh_eval.py ------------------------------------------------------------------------------------------------------------------------------------------
def test_mesh_eval_on_a_square(hp):
    """the unit square against a 101 x 101 grid of ground-truth points 0.01 above it: every ground-truth point is 0.01 from the mesh, every sample
    within sqrt(0.01^2 + 2 0.005^2) of a grid point"""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import mesh_eval
    vtx = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], np.float32)
    faces = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    g = np.arange(101) / 100.0
    cloud = np.concatenate([np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2), np.full((101 * 101, 1), 0.01)], axis=1).astype(np.float32)
    hp.raycast_build_triangles(vtx, faces)
    out = mesh_eval.evaluate(hp, cloud, tau=0.02, max_dist=0.5, density=5000.0, seed=1)
    assert out["samples"] == 5000 and out["cloud_points"] == 10201 == out["accuracy"]["within_tau"] and out["completeness"]["within_tau"] == 5000
    assert out["precision"] == out["recall"] == out["f_score"] == 1.0
    assert abs(out["accuracy"]["mean"] - 0.01) < 1e-8 and 0.01 <= out["completeness"]["mean"] <= 0.01225 and out["completeness"]["max"] <= 0.01225
    assert out["chamfer"] == out["accuracy"]["mean"] + out["completeness"]["mean"]
    out = mesh_eval.evaluate(hp, cloud, tau=0.005, max_dist=0.5, density=5000.0, seed=1)
    assert out["precision"] == out["recall"] == out["f_score"] == 0.0 and out["accuracy"]["within_max_dist"] == 10201
