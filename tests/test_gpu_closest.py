"""Point-to-mesh distances on the device (include/immesh_closest.h): the traversal and the reduction against the brute-force numpy restatement of the
contract (tests/closest_checker.py), bit for bit on D, dist, face, xyz and side -- sizes at which the build and the query change path, equal and
clustered codes, exact ties, faces of zero area, the max_dist boundary, a point that every box contains, face order, statistics, the live mesh
as a snapshot with no side effects on the maps, rays after a query, determinism, argument errors, scale."""
import ctypes as C

import numpy as np
import pytest

import closest_checker as cc
import raycast_checker as rcc
from immesh_amd import capi, synth
from conftest import make_hip
from parity_utils import compare_plane_tables_fast
from test_gpu_render import _lattice, _rand_rot, _small_cfg, _soup

pytestmark = pytest.mark.gpu
I3, Z3 = np.eye(3), np.zeros(3)
KEYS = ("d2", "dist", "face", "xyz", "side")


@pytest.fixture(scope="module")
def hp():
    h = make_hip(capi.load_hip_library(), _small_cfg())
    yield h
    h.close()


def _raw(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same(got, ref, what=""):
    """device dict == checker tuple, bit for bit"""
    for k, r in zip(KEYS, ref):
        g = got[k]
        assert g.dtype == r.dtype and g.shape == r.shape, (what, k, g.dtype, r.dtype, g.shape, r.shape)
        if len(g) == 0:
            continue
        diff = np.nonzero((_raw(g).reshape(len(g), -1) != _raw(r).reshape(len(r), -1)).any(axis=1))[0]
        assert len(diff) == 0, (what, k, len(diff), len(g), diff[:5].tolist(), g[diff[:5]].tolist(), r[diff[:5]].tolist())


def _points(rng, vtx, faces, n, near=0.1):
    """n world points: the first half within `near` of random points on random faces (so that a single point is one of them), the rest uniform in
    the soup's bounds; a NaN point and a point 10^6 away when there is room"""
    fin = np.nonzero(np.isfinite(vtx[faces]).all(axis=(1, 2)))[0] if len(faces) else np.zeros(0, np.int64)
    if len(fin):
        tri = vtx[faces[fin]].astype(np.float64)
        lo, hi = tri.min(axis=(0, 1)), tri.max(axis=(0, 1))
    else:
        lo, hi = -np.ones(3), np.ones(3)
    pts = rng.uniform(lo, hi, (n, 3))
    k = (n + 1) // 2
    if len(fin) and n:
        t = tri[rng.integers(len(fin), size=k)]
        pts[:k] = (t * rng.dirichlet(np.ones(3), size=k)[:, :, None]).sum(axis=1) + rng.uniform(-near, near, (k, 3)) / np.sqrt(3.0)
    pts = pts.astype(np.float32)
    if n >= 60:
        pts[n - 1, 1] = np.nan
        pts[n - 2] = [1e6, -1e6, 1e6]
    return pts


def _local(pts, rot, pos):
    """world points in the sensor frame (rounded to float: the contract's p is what the frame makes of them)"""
    return ((pts.astype(np.float64) - pos) @ rot).astype(np.float32)


def _check(hp, rot, pos, pts, max_dist, vtx, faces, ref=None, what=""):
    ref = cc.closest(rot, pos, pts, max_dist, vtx, faces) if ref is None else ref
    got = hp.closest_points(pts, max_dist, None if rot is None else capi.ray_frame(rot, pos))
    _same(got, ref, what)
    return ref


# ---- sizes ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_faces", [0, 1, 2, 3, 63, 64, 65, 257, 5000])
def test_sizes_match_checker(hp, n_faces):
    rng = np.random.default_rng(200 + n_faces)
    vtx, faces = _soup(rng, n_faces) if n_faces else (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    hp.raycast_build_triangles(vtx, faces)
    rot, pos = _rand_rot(rng), rng.uniform(-2, 2, 3)
    for n_pts in (0, 1, 63, 64, 65, 1000):
        world = _points(rng, vtx, faces, n_pts)
        for frame, max_dist in ((None, 0.5), ((rot, pos), 0.5), (None, 100.0)):
            r, p, pts = (None, None, world) if frame is None else (frame[0], frame[1], _local(world, *frame))
            ref = cc.closest(r, p, pts, max_dist, vtx, faces)
            if n_faces and n_pts:
                assert (ref[2] >= 0).any(), (n_faces, n_pts, max_dist)                # the checker first: the comparison is not one of misses alone
            else:
                assert (ref[2] < 0).all()
            if n_pts >= 60:
                assert ref[2][-1] == -1 and ref[2][-2] == -1
            _check(hp, r, p, pts, max_dist, vtx, faces, ref, (n_faces, n_pts, max_dist))


# ---- equal and clustered codes ---------------------------------------------------------------------------------------------------------------------
def test_copies_of_one_triangle(hp):
    """300 faces with one Morton code and one D for every point: the lowest index wins every point"""
    rng = np.random.default_rng(1)
    vtx = np.array([[-1, -1, -5], [1, -1, -5], [0, 1.5, -5]], np.float32)
    faces = np.tile(np.array([[0, 1, 2]], np.int32), (300, 1))
    assert hp.raycast_build_triangles(vtx, faces) == (3, 300, 300)
    pts = _points(rng, vtx, faces, 500, near=2.0)
    ref = _check(hp, None, None, pts, 50.0, vtx, faces)
    assert (ref[2] >= 0).sum() >= 498 and set(ref[2].tolist()) == {-1, 0}


def test_lopsided_tree(hp):
    """face centres at x = 2^-k, k = 0 .. 29: every split peels one face off, the deepest tree the code's 21 bits per axis allow, beside 200 random
    faces; the traversal's stack bound (raycast.hpp) holds it"""
    rng = np.random.default_rng(2)
    k = np.arange(30)
    c = np.stack([2.0 ** -k, np.zeros(30), np.zeros(30)], axis=-1)
    tri = np.array([[-0.2, -0.5, 0], [0.2, -0.5, 0], [0, 0.5, 0.1]])
    small = c[:, None, :] + tri[None] * (2.0 ** -k)[:, None, None] * 0.5
    more = rng.uniform(0, 1, (200, 1, 3)) + rng.normal(scale=0.02, size=(200, 3, 3))
    vtx = np.concatenate([small, more]).reshape(-1, 3).astype(np.float32)
    faces = np.arange(len(vtx), dtype=np.int32).reshape(-1, 3)
    hp.raycast_build_triangles(vtx, faces)
    pts = _points(rng, vtx, faces, 1000, near=0.01)
    pts[:30] = (c + [0, 0, 0.02 * 2.0 ** -29]).astype(np.float32)                       # one point at every peeled face
    pts[30:60] = (c * [1, 0, 0] + [0, 0, -3.0]).astype(np.float32)                      # and far below them: every box is open for a long time
    for max_dist in (10.0, 0.05):
        ref = _check(hp, None, None, pts, max_dist, vtx, faces)
        assert len(set(ref[2][:30].tolist()) - {-1}) >= 10


# ---- exact ties ---------------------------------------------------------------------------------------------------------------------------------------
def test_exact_ties_on_a_lattice(hp):
    """a dyadic lattice queried at its vertices, edge midpoints and face centroids, in the plane and lifted by 1 / 4: a vertex is shared by up to six
    faces that all give the same q and the same D, and the lowest index wins"""
    vtx, faces = _lattice(12, 10, 4.0, 256.0, 0, 0)                    # x, y multiples of 1 / 8, z = -4
    hp.raycast_build_triangles(vtx, faces)
    tri = vtx[faces].astype(np.float64)
    mids = np.concatenate([(tri[:, a] + tri[:, b]) / 2 for a, b in ((0, 1), (1, 2), (2, 0))])
    flat = np.concatenate([vtx.astype(np.float64), mids, tri.mean(axis=1)])
    pts = np.concatenate([flat, flat + [0, 0, 0.25], flat - [0, 0, 0.25]]).astype(np.float32)
    allD = cc.all_D(None, None, pts[:len(vtx)], vtx, faces)
    ties = (allD == allD.min(axis=1)[:, None]).sum(axis=1)
    assert (ties >= 2).mean() >= 0.5, float((ties >= 2).mean())
    assert np.array_equal(np.argmax(allD == allD.min(axis=1)[:, None], axis=1), cc.closest(None, None, pts[:len(vtx)], 1.0, vtx, faces)[2])
    ref = _check(hp, None, None, pts, 1.0, vtx, faces)
    assert (ref[2] >= 0).all()
    n = len(flat)
    assert np.all(ref[0][:n] == 0.0) and np.all(ref[0][n:] == 0.0625) and np.all(ref[1][n:] == np.float32(0.25))
    assert np.all(ref[4][:n] == 0) and len(set(ref[4][n:2 * n].tolist())) == 1 and np.all(ref[4][2 * n:] == -ref[4][n])
    assert np.array_equal(ref[2][:n], ref[2][n:2 * n]) and np.array_equal(ref[2][:n], ref[2][2 * n:])


# ---- faces of zero area, faces that are not finite ----------------------------------------------------------------------------------------------------
def test_zero_area_and_nan_faces(hp):
    rng = np.random.default_rng(4)
    vtx, faces = _soup(rng, 1000, spread=8.0, size=0.4)                 # 20 each: repeated vertex, collinear, flat, NaN vertex, ..., duplicates
    point = rng.uniform(-8, 8, (40, 3)).astype(np.float32)              # and 40 faces that are a single point, 40 whose first two vertices coincide
    vtx = np.concatenate([vtx, point]).astype(np.float32)
    extra = np.concatenate([np.stack([np.arange(40)] * 3, axis=-1) + 3000, np.stack([np.arange(40) + 3000, np.arange(40) + 3000, np.arange(40)], axis=-1)])
    faces = np.concatenate([faces, extra]).astype(np.int32)
    hp.raycast_build_triangles(vtx, faces)
    tri = vtx[faces]
    nan_face = ~np.isfinite(tri).all(axis=(1, 2))
    n = np.cross((tri[:, 1] - tri[:, 0]).astype(np.float64), (tri[:, 2] - tri[:, 0]).astype(np.float64))
    flat_face = ~nan_face & (np.abs(n).max(axis=1) <= 1e-6)
    assert nan_face.sum() >= 20 and flat_face.sum() >= 100
    # a point beside every vertex of every face (the NaN faces' finite vertices too), and a cloud
    at = tri.reshape(-1, 3)
    at = at[np.isfinite(at).all(axis=1)]
    pts = np.concatenate([at + rng.normal(scale=0.01, size=at.shape).astype(np.float32), at, _points(rng, vtx, faces, 1000)]).astype(np.float32)
    ref = _check(hp, None, None, pts, 2.0, vtx, faces)
    won = ref[2][ref[2] >= 0]
    assert not nan_face[won].any()                                       # (the checker's answer, which the device has just matched)
    assert flat_face[won].sum() >= 100 and (~flat_face[won]).sum() >= 1000
    assert np.isfinite(ref[3][ref[2] >= 0]).all() and (ref[4][ref[2] >= 0][flat_face[won] & (won >= 1000)] == 0).all()


# ---- the max_dist boundary ------------------------------------------------------------------------------------------------------------------------------
def test_max_dist_boundary(hp):
    vtx = np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0]], np.float32)
    faces = np.array([[0, 1, 2]], np.int32)
    hp.raycast_build_triangles(vtx, faces)
    pts = np.array([[1, 1, 2], [1, 1, -2], [6, -1, 2], [4000, 4000, 0], [1, 1, 0]], np.float32)      # D = 4, 4, 9, ..., 0
    ref = _check(hp, None, None, pts, 2.0, vtx, faces)
    assert ref[2].tolist() == [0, 0, -1, -1, 0] and ref[0].tolist() == [4.0, 4.0, -1.0, -1.0, 0.0]   # D == r2 counts
    below = np.nextafter(2.0, 0.0)
    assert below * below < 4.0
    ref = _check(hp, None, None, pts, below, vtx, faces)
    assert ref[2].tolist() == [-1, -1, -1, -1, 0]
    # the next double above D: the frame lifts the point by one unit in the last place of 2
    up = np.nextafter(2.0, 3.0)
    local = np.array([[1, 1, 0], [1, 1, 0]], np.float32)
    for z, want in ((2.0, 0), (up, -1), (-2.0, 0), (-up, -1)):
        ref = _check(hp, I3, np.array([0.0, 0.0, z]), local, 2.0, vtx, faces)
        assert ref[2].tolist() == [want, want], z
        if want == 0:
            assert ref[0].tolist() == [4.0, 4.0]
    assert up * up > 4.0
    ref = _check(hp, None, None, pts, 3.0, vtx, faces)
    assert ref[2].tolist() == [0, 0, 0, -1, 0]


# ---- a point that every box contains ----------------------------------------------------------------------------------------------------------------------
def test_point_enclosed_by_large_overlapping_faces(hp):
    """400 large faces with their vertices on the six sides of a cube, around query points inside it: nearly every node's box contains the point,
    L = 0, and pruning does nothing; the result stays right"""
    rng = np.random.default_rng(5)
    v = rng.uniform(-10, 10, (1200, 3))
    side = rng.integers(0, 6, 1200)
    v[np.arange(1200), side % 3] = np.where(side < 3, -10.0, 10.0)
    vtx, faces = v.astype(np.float32), np.arange(1200, dtype=np.int32).reshape(-1, 3)
    hp.raycast_build_triangles(vtx, faces)
    pts = rng.uniform(-3, 3, (300, 3)).astype(np.float32)
    p = pts.astype(np.float64)[:, None, :]
    tri = vtx[faces].astype(np.float64)
    inside = ((tri.min(axis=1)[None] <= p) & (p <= tri.max(axis=1)[None])).all(axis=2)
    assert inside.mean() > 0.3, inside.mean()
    ref = _check(hp, None, None, pts, 50.0, vtx, faces)
    assert (ref[2] >= 0).all() and len(set(ref[2].tolist())) > 50


# ---- face order -----------------------------------------------------------------------------------------------------------------------------------------
def test_face_order_does_not_change_the_distance(hp):
    rng = np.random.default_rng(6)
    vtx, faces = _soup(rng, 1000, spread=6.0, size=0.5)
    perm = rng.permutation(len(faces))
    pts = _points(rng, vtx, faces, 400)
    hp.raycast_build_triangles(vtx, faces)
    ref = _check(hp, None, None, pts, 3.0, vtx, faces)
    a = hp.closest_points(pts, 3.0)
    hp.raycast_build_triangles(vtx, faces[perm])
    _check(hp, None, None, pts, 3.0, vtx, faces[perm])
    b = hp.closest_points(pts, 3.0)
    assert a["d2"].tobytes() == b["d2"].tobytes() and a["dist"].tobytes() == b["dist"].tobytes()
    allD = cc.all_D(None, None, pts, vtx, faces)
    have = a["face"] >= 0
    single = have & ((allD == np.where(have, a["d2"], np.nan)[:, None]).sum(axis=1) == 1)
    assert single.sum() > 300 and (have & ~single).sum() > 0               # (the soup's duplicate faces tie)
    assert np.array_equal(perm[b["face"][single]], a["face"][single])
    assert a["xyz"][single].tobytes() == b["xyz"][single].tobytes() and a["side"][single].tobytes() == b["side"][single].tobytes()


# ---- statistics -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stats_case(hp):
    rng = np.random.default_rng(7)
    vtx, faces = _soup(rng, 2000, spread=10.0, size=0.5)
    pts = _points(rng, vtx, faces, 50000, near=0.3)
    pts[100:200, 0] = np.inf
    ref = cc.closest(None, None, pts, 1.5, vtx, faces)
    return vtx, faces, pts, ref


@pytest.mark.parametrize("n_pts", [1, 64, 65, 50000])
def test_stats_match_checker(hp, stats_case, n_pts):
    vtx, faces, pts, ref = stats_case
    pts = pts[len(pts) - n_pts:] if n_pts > 1 else pts[:1]                 # the tail holds the NaN, the far and the uniform points
    ref = tuple(r[len(r) - n_pts:] if n_pts > 1 else r[:1] for r in ref)
    hp.raycast_build_triangles(vtx, faces)
    _check(hp, None, None, pts, 1.5, vtx, faces, ref)
    for n_bins, bin_width in ((1, 0.25), (7, 0.1), (1024, 1.0 / 1024), (1025, 1.0 / 1024), (4096, 1.0 / 4096), (1024, 1e-4)):   # (the reduction counts up to 1024 bins in LDS)
        want, hist = cc.stats(None, None, pts, ref[1], ref[2], bin_width, n_bins)
        st, h = hp.closest_stats(bin_width, n_bins)
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
        st2, h2 = hp.closest_stats(bin_width, n_bins)
        assert bytes(st) == bytes(st2) and h.tobytes() == h2.tobytes()
    if n_pts == 50000:
        assert want["n_with_face"] > 20000 and want["n_no_face"] > 1000 and want["n_not_finite"] == 101 and want["n_overflow"] > 0
        print("50 000 points x 2 000 faces: query %.3f ms, reduction %.3f ms" % hp.closest_timing())


# ---- the live mesh ------------------------------------------------------------------------------------------------------------------------------------------
def test_live_mesh_snapshot_without_side_effects():
    """a queries its snapshot of the live mesh between scans, b never does: a's answers equal the checker on the exported arrays and stay the same
    bits while the stream goes on, and both contexts end with the same states, mesh and plane table"""
    lib = capi.load_hip_library()
    cfg = capi.avia_config(cap_root_voxels=1 << 15, cap_scan_points=100000)
    a, b = make_hip(lib, cfg), make_hip(lib, cfg)
    try:
        extT = np.array(list(cfg.extT))

        def scan(k):
            R, t = synth.trajectory_pose(k)
            raw = synth.livox_scan(k, R, t, n_pts=20000, extT=extT)
            if k == 0:
                for h in (a, b):
                    h.map_build(np.ascontiguousarray(raw[:, :3]), capi.make_state(R=R, t=t))
                return None, raw
            down = synth.voxel_grid_downsample(raw, 0.4)
            prior = capi.make_state(R=R, t=t + np.array([0.01, 0.0, -0.01]), cov_diag=1e-5)
            sa, ia = a.process_scan(down, raw, prior, prior, frame_idx=k, do_mesh=True)
            sb, ib = b.process_scan(down, raw, prior, prior, frame_idx=k, do_mesh=True)
            assert ia == ib and np.array_equal(sa, sb)
            return sa, raw

        for k in range(4):
            state, raw = scan(k)
        nv, nf, n_in = a.raycast_build_mesh(1.0, 20)
        vtx, faces = a.mesh_export(1.0, 20)
        assert (nv, nf) == (len(vtx), len(faces)) and 0 < n_in <= nf
        planes, counters = a.dump_planes(), a.counters()
        # the scan's own points: in the sensor frame under the estimated pose's frame, and as world floats
        frame = a.ray_frame_from_state(state)
        rot, pos = np.array(list(frame.rot)).reshape(3, 3), np.array(list(frame.pos))
        local = np.ascontiguousarray(raw[::10, :3])
        world = (local.astype(np.float64) @ rot.T + pos).astype(np.float32)
        ref = cc.closest(rot, pos, local, 1.0, vtx, faces)
        first = a.closest_points(local, 1.0, frame)
        _same(first, ref, "sensor frame")
        assert (ref[2] >= 0).mean() > 0.5, (ref[2] >= 0).mean()
        _same(a.closest_points(world, 1.0), cc.closest(None, None, world, 1.0, vtx, faces), "world")
        st, _ = a.closest_stats(0.01, 100)
        print("scan-to-mesh: %d of %d points with a face, mean %.4f m, rms %.4f m, max %.4f m" % (st.n_with_face, st.n_points, st.mean, st.rms, st.max_dist))
        assert compare_plane_tables_fast(planes, a.dump_planes(), 0.0) > 100 and a.counters() == counters
        for k in range(4, 6):
            scan(k)
            again = a.closest_points(local, 1.0, frame)
            assert all(again[key].tobytes() == first[key].tobytes() for key in KEYS)      # the old snapshot, the old bits
        ea, eb = a.mesh_export(1.0, 20), b.mesh_export(1.0, 20)
        assert len(ea[1]) != len(faces) and ea[0].tobytes() == eb[0].tobytes() and ea[1].tobytes() == eb[1].tobytes()
        assert compare_plane_tables_fast(a.dump_planes(), b.dump_planes(), 0.0) > 100
    finally:
        a.close(); b.close()


# ---- rays after a query -----------------------------------------------------------------------------------------------------------------------------------
def test_rays_after_a_query(hp):
    rng = np.random.default_rng(8)
    vtx, faces = _soup(rng, 3000)
    hp.raycast_build_triangles(vtx, faces)
    pts = _points(rng, vtx, faces, 2000)
    rot, pos = _rand_rot(rng), rng.uniform(-2, 2, 3)
    dirs = rng.normal(size=(3000, 3)).astype(np.float32)
    rt, rf = rcc.cast(rot, pos, dirs, None, 0.0, 100.0, vtx, faces)
    ref = _check(hp, None, None, pts, 1.0, vtx, faces)
    for _ in range(2):
        t, f = hp.raycast(capi.ray_frame(rot, pos), dirs, None, 0.0, 100.0)
        assert np.array_equal(f, rf) and t.tobytes() == rt.tobytes() and (rf >= 0).sum() > 100
        points = hp.raycast_points(0.05)
        _check(hp, None, None, pts, 1.0, vtx, faces, ref)
        assert hp.raycast_points(0.05).tobytes() == points.tobytes() and len(points) > 50  # the cast's points outlive a query
        hp.closest_stats(0.1, 8)


# ---- determinism, errors, scale -------------------------------------------------------------------------------------------------------------------------
def test_deterministic():
    lib = capi.load_hip_library()
    a, b = make_hip(lib, _small_cfg()), make_hip(lib, _small_cfg())
    try:
        rng = np.random.default_rng(41)
        vtx, faces = _soup(rng, 20000)
        other = _soup(rng, 3000)
        pts = _points(rng, vtx, faces, 20000, near=0.5)
        a.raycast_build_triangles(vtx, faces)
        ra = a.closest_points(pts, 2.0); sa, ha = a.closest_stats(0.05, 64)
        b.raycast_build_triangles(*other)                                       # b: another soup and another query first, then this one twice
        b.closest_points(pts[:777], 5.0)
        for _ in range(2):
            b.raycast_build_triangles(vtx, faces)
            rb = b.closest_points(pts, 2.0); sb, hb = b.closest_stats(0.05, 64)
            assert all(ra[k].tobytes() == rb[k].tobytes() for k in KEYS)
            assert bytes(sa) == bytes(sb) and ha.tobytes() == hb.tobytes()
        assert (ra["face"] >= 0).sum() > 5000
    finally:
        a.close(); b.close()


def test_argument_errors():
    h = make_hip(capi.load_hip_library(), _small_cfg())
    try:
        vtx = np.array([[-1, -1, -2], [1, -1, -2], [0, 1, -2]], np.float32)
        faces = np.array([[0, 1, 2]], np.int32)
        pts = np.array([[0, 0, 0], [0, 0, -5]], np.float32)
        with pytest.raises(RuntimeError, match=r"rc=-1: .*built"):
            h.closest_points(pts, 10.0)                                          # a query before a build
        h.raycast_build_triangles(vtx, faces)
        with pytest.raises(RuntimeError, match=r"rc=-1: .*no closest-point query"):
            h.closest_stats(0.1, 4)                                              # statistics before a query

        def still_usable():
            r = h.closest_points(pts, 10.0)
            assert r["dist"].tolist() == [2.0, 3.0] and r["face"].tolist() == [0, 0] and r["side"].tolist() == [1, -1]
            assert r["xyz"].tolist() == [[0, 0, -2], [0, 0, -2]] and r["d2"].tolist() == [4.0, 9.0]
            st, hist = h.closest_stats(1.0, 3)
            assert (st.n_points, st.n_with_face, st.n_overflow, st.max_dist, st.sum_dist, st.sum_dist2) == (2, 2, 1, 3.0, 5.0, 13.0) and hist.tolist() == [0, 0, 1]
            t, f = h.raycast(capi.ray_frame(), np.array([[0, 0, -1]], np.float32), None, 0.0, 10.0)
            assert t.tolist() == [2.0] and f.tolist() == [0]

        still_usable()
        for max_dist in (0.0, -1.0, np.inf, np.nan):
            with pytest.raises(RuntimeError, match=r"rc=-1: .*max_dist"):
                h.closest_points(pts, max_dist)
            still_usable()
        for bad in (capi.ray_frame(pos=[np.nan, 0, 0]), capi.ray_frame(rot=np.diag([1.0, np.inf, 1.0]))):
            with pytest.raises(RuntimeError, match=r"rc=-1: .*finite"):
                h.closest_points(pts, 10.0, bad)
            still_usable()
        f = h.lib.immesh_closest_points
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_double] + [C.c_void_p] * 5
        for n in (-1, 2 ** 31 - 1, 2 ** 40):
            assert f(h.raycaster(), None, pts.ctypes.data_as(C.c_void_p), n, 10.0, None, None, None, None, None) == -1
            assert b"point array" in h.lib.immesh_last_error(h.ctx)
            still_usable()
        assert f(h.raycaster(), None, None, 2, 10.0, None, None, None, None, None) == -1
        assert f(h.raycaster(), None, None, 0, 10.0, None, None, None, None, None) == 0       # no points, no array
        assert f(h.raycaster(), None, pts.ctypes.data_as(C.c_void_p), 2, 10.0, None, None, None, None, None) == 0    # every output may be NULL
        for bin_width, n_bins, text in ((0.0, 4, "bin_width"), (-1.0, 4, "bin_width"), (np.inf, 4, "bin_width"), (np.nan, 4, "bin_width"), (0.1, 0, "n_bins"),
                                        (0.1, -3, "n_bins"), (0.1, (1 << 20) + 1, "n_bins")):
            with pytest.raises(RuntimeError, match=r"rc=-1: .*" + text):
                h.closest_stats(bin_width, n_bins)
            still_usable()
        assert h.closest_stats(1.0, 1 << 20)[1].sum() == 2
        # a caster with no face in its tree answers -1; that is no error
        h.raycast_build_triangles(np.array([[np.nan, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), faces)
        r = h.closest_points(pts, 10.0)
        assert r["face"].tolist() == [-1, -1] and r["dist"].tolist() == [-1.0, -1.0]
        st, _ = h.closest_stats(1.0, 3)
        assert (st.n_with_face, st.n_no_face, st.mean, st.rms, st.max_dist) == (0, 2, 0.0, 0.0, 0.0)
        h.raycast_build_triangles(vtx, faces)
        still_usable()
    finally:
        h.close()


def test_scale(hp):
    """200 000 faces x 100 000 points; every 50th point against every face in numpy, exact; for all points the reported face reproduces the
    reported D, xyz and side"""
    rng = np.random.default_rng(51)
    vtx, faces = _soup(rng, 200000, spread=30.0, size=0.3)
    assert hp.raycast_build_triangles(vtx, faces)[1] == 200000
    pts = _points(rng, vtx, faces, 100000, near=0.3)
    got = hp.closest_points(pts, 3.0)
    print("200k faces x 100k points: query %.3f ms; with a face %.3f" % (hp.closest_timing()[0], (got["face"] >= 0).mean()))
    have = got["face"] >= 0
    assert have.mean() > 0.9
    pick = np.arange(0, len(pts), 50)
    assert len(pick) == 2000
    ref = cc.closest(None, None, pts[pick], 3.0, vtx, faces)
    _same({k: got[k][pick] for k in KEYS}, ref, "every 50th point")
    D, xyz, side = cc.face_result(None, None, pts[have], vtx, faces, got["face"][have])
    assert np.array_equal(D, got["d2"][have]) and xyz.tobytes() == got["xyz"][have].tobytes() and np.array_equal(side, got["side"][have])
    assert np.array_equal(np.sqrt(D).astype(np.float32), got["dist"][have]) and (D <= 9.0).all()
    assert (got["d2"][~have] == -1.0).all() and np.isnan(got["xyz"][~have]).all()
