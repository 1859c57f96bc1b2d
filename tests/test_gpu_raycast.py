"""Rays cast at a triangle soup and at the live mesh on the device (include/immesh_raycast.h): the hierarchy and the traversal kernel against the
brute-force numpy restatement of the contract (tests/raycast_checker.py), bit-exact -- sizes at which the build and the cast change path, equal and
clustered codes, exact ties, axis-parallel rays, range ends, ANY, reinforced points, the live mesh as a snapshot, no side effects on the map,
the rasterizer on the same pixel rays, determinism, argument errors, scale."""
import numpy as np
import pytest

import raycast_checker as rcc
import render_checker as rck
from immesh_amd import capi, synth
from conftest import make_hip
from parity_utils import compare_plane_tables_fast
from test_gpu_render import _lattice, _rand_rot, _small_cfg, _soup
from test_raycast_cpu import PINHOLE, pinhole_camera, pinhole_differences, pinhole_rays, pinhole_soup

pytestmark = pytest.mark.gpu
I3, Z3 = np.eye(3), np.zeros(3)


@pytest.fixture(scope="module")
def hp():
    h = make_hip(capi.load_hip_library(), _small_cfg())
    yield h
    h.close()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _aimed(rng, vtx, faces, n, pos=Z3, rot=I3, spread=0.6):
    """n sensor-frame directions: half random, half towards random points in and around random faces (so that small soups are hit too); a zero and
    a NaN direction among them when there is room"""
    dirs = rng.normal(size=(n, 3))
    fin = np.nonzero(np.isfinite(vtx[faces]).all(axis=(1, 2)))[0] if len(faces) else np.zeros(0, np.int64)
    if len(fin) and n:
        k = n // 2 + 1
        f = rng.choice(fin, size=k)
        w = rng.dirichlet(np.ones(3), size=k) + rng.normal(scale=spread * 0.2, size=(k, 3))
        target = (vtx[faces[f]].astype(np.float64) * w[:, :, None]).sum(axis=1) / w.sum(axis=1)[:, None]
        dirs[:k] = (target - pos) @ rot * rng.uniform(0.3, 2.0, (k, 1))              # rot^T (target - pos), not normalised
    dirs = dirs.astype(np.float32)
    if n >= 60:
        dirs[n - 1] = 0
        dirs[n - 2, 1] = np.nan
    return dirs


def _check(hp, rot, pos, dirs, origins, vtx, faces, t_min=0.0, t_max=200.0, res=None):
    """one NEAREST cast against the checker, bit for bit; with res, the reinforced points too -> (t, face) of the checker"""
    t, f = hp.raycast(capi.ray_frame(rot, pos), dirs, origins, t_min, t_max)
    rt, rf = rcc.cast(rot, pos, dirs, origins, t_min, t_max, vtx, faces)
    assert np.array_equal(f, rf), (int((f != rf).sum()), len(f))
    assert np.array_equal(_bits(t), _bits(rt)), int((_bits(t) != _bits(rt)).sum())
    for r in ([] if res is None else res):
        pts = hp.raycast_points(r)
        ref = rcc.points(rot, pos, dirs, origins, rt, r)
        assert pts.shape == ref.shape and np.array_equal(_bits(pts), _bits(ref)), r
        assert len(pts) <= int((rf >= 0).sum())
    return rt, rf


# ---- sizes ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_faces", [0, 1, 2, 3, 63, 64, 65, 257, 5000])
def test_sizes_match_checker(hp, n_faces):
    rng = np.random.default_rng(100 + n_faces)
    vtx, faces = _soup(rng, n_faces) if n_faces else (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    nv, nf, n_in = hp.raycast_build_triangles(vtx, faces)
    finite = int(np.isfinite(vtx[faces]).all(axis=(1, 2)).sum()) if n_faces else 0
    assert (nv, nf, n_in) == (len(vtx), n_faces, finite)
    frames = [(I3, Z3), (_rand_rot(rng), rng.uniform(-2, 2, 3)), (_rand_rot(rng), rng.uniform(-2, 2, 3))]
    hits = total = 0
    for n_rays in (0, 1, 63, 64, 65, 1000):
        for rot, pos in frames:
            for with_origins in (False, True):
                org = rng.uniform(-1, 1, (n_rays, 3)).astype(np.float32) if with_origins else None
                if with_origins and n_rays >= 60:
                    org[n_rays - 3, 2] = np.inf                                           # an origin that is not finite: a miss
                dirs = _aimed(rng, vtx, faces, n_rays, pos, rot)
                _, rf = _check(hp, rot, pos, dirs, org, vtx, faces)
                hits += int((rf >= 0).sum()); total += n_rays
    if n_faces >= 5000:
        assert hits >= 0.05 * total, (hits, total)
    elif n_faces:
        assert hits > 0


# ---- equal and clustered codes ---------------------------------------------------------------------------------------------------------------------
def test_copies_of_one_triangle(hp):
    """300 faces with one Morton code: the tree splits on the position alone, and the lowest index wins every hit"""
    rng = np.random.default_rng(1)
    vtx = np.array([[-1, -1, -5], [1, -1, -5], [0, 1.5, -5]], np.float32)
    faces = np.tile(np.array([[0, 1, 2]], np.int32), (300, 1))
    assert hp.raycast_build_triangles(vtx, faces) == (3, 300, 300)
    dirs = _aimed(rng, vtx, faces, 500)
    rt, rf = _check(hp, I3, Z3, dirs, None, vtx, faces)
    assert (rf >= 0).sum() > 100 and set(rf.tolist()) <= {-1, 0}


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
    for n, pos in enumerate((np.array([0.3, 0.1, -3.0]), np.array([-2.0, 0.0, 0.05]), np.array([0.0, 0.0, 1e-7]))):
        dirs = _aimed(rng, vtx, faces, 1000, pos, spread=0.1)
        dirs[:30] = (c + [0, 0, 0.02 * 2.0 ** -29] - pos).astype(np.float32)          # one ray at every peeled face
        _, rf = _check(hp, I3, pos, dirs, None, vtx, faces, t_max=50.0)
        assert (rf >= 0).sum() > 100
        if n == 0:                                                                      # seen from below, the larger peeled faces are hit one by one
            assert len(set(rf[:30].tolist()) - {-1}) >= 10


def test_one_face_spanning_the_scene(hp):
    rng = np.random.default_rng(3)
    vtx, faces = _soup(rng, 2000)
    big = np.array([[-40, -40, -22], [40, -40, -22], [0, 60, 25]], np.float32)
    vtx = np.concatenate([vtx, big]).astype(np.float32)
    faces = np.concatenate([faces[:1000], [[len(vtx) - 3, len(vtx) - 2, len(vtx) - 1]], faces[1000:]]).astype(np.int32)
    hp.raycast_build_triangles(vtx, faces)
    pos = np.array([0.5, -0.5, 1.0])
    dirs = _aimed(rng, vtx, faces, 2000, pos)
    _, rf = _check(hp, I3, pos, dirs, None, vtx, faces)
    assert (rf == 1000).sum() > 100 and ((rf >= 0) & (rf != 1000)).sum() > 100


# ---- exact ties, axis-parallel rays, range ends -----------------------------------------------------------------------------------------------------
def _grid_rays(n_half, step, f):
    u, v = np.meshgrid(np.arange(-n_half, n_half + 1) * step, np.arange(-n_half, n_half + 1) * step)
    return np.stack([u / f, -v / f, np.full(u.shape, -1.0)], axis=-1).reshape(-1, 3).astype(np.float32)


def test_exact_ties_on_a_lattice(hp):
    """a lattice of quads at distance 4 = 2^2 whose vertices lie on rays of slope k / 32: rays through every vertex, every edge midpoint and every
    diagonal's midpoint -- each is shared by two to six faces, and all of them are hit at exactly 4"""
    vtx, faces = _lattice(40, 30, 4.0, 256.0, 0, 0)                    # vertices every 8 / 256 in slope
    hp.raycast_build_triangles(vtx, faces)
    dirs = _grid_rays(30, 4, 256.0)                                     # every 4 / 256: vertices, edge midpoints, quad centres (on the diagonals)
    for rot, pos in ((I3, Z3),):
        rt, rf = _check(hp, rot, pos, dirs, None, vtx, faces, t_max=64.0, res=[0.05])
        hit = rf >= 0
        assert hit.sum() >= 31 * 31 and np.all(rt[hit] == np.float32(4.0))
    # the same rays, twice as long: t in units of |d|
    rt2, rf2 = _check(hp, I3, Z3, dirs * np.float32(2.0), None, vtx, faces, t_max=64.0)
    assert np.array_equal(rf2, rf) and np.all(rt2[rf2 >= 0] == np.float32(2.0))


def _axis_lattice(n=6):
    """unit quads with integer corners in the planes z = -3, x = 3 and y = -2, two triangles each"""
    vtx, faces = [], []
    for plane in range(3):
        for i in range(-n, n):
            for j in range(-n, n):
                q = [(i, j), (i + 1, j), (i + 1, j + 1), (i, j + 1)]
                p = [(a, b, -3) for a, b in q] if plane == 0 else [(3, a, b) for a, b in q] if plane == 1 else [(a, -2, b) for a, b in q]
                base = len(vtx)
                vtx += p
                faces += [(base, base + 1, base + 2), (base, base + 2, base + 3)]
    return np.array(vtx, np.float32), np.array(faces, np.int32)


def test_axis_parallel_rays_on_box_planes(hp):
    """d along +-x, +-y, +-z and inside the coordinate planes, origins with integer and half-integer coordinates: exactly on the planes of the
    faces' boxes and of the nodes' boxes, where an axis with d_k == 0 decides by lo <= o <= hi alone"""
    vtx, faces = _axis_lattice()
    hp.raycast_build_triangles(vtx, faces)
    g = np.arange(-4, 4.5, 0.5)
    X, Y = np.meshgrid(g, g)
    flat = np.stack([X.reshape(-1), Y.reshape(-1)], axis=-1)
    total = 0
    for d in ([0, 0, -1], [0, 0, 1], [1, 0, 0], [-1, 0, 0], [0, -1, 0], [0, 1, 0], [0, -2, 0], [1, 0, -1], [1, -1, 0], [0, -1, -1], [0.5, 0, -2], [-1, 1, 0]):
        d = np.array(d, np.float32)
        ax = int(np.argmax(np.abs(d)))
        org = np.zeros((len(flat), 3), np.float32)
        org[:, [k for k in range(3) if k != ax]] = flat                   # a sheet of origins across the main direction, through the world origin
        _, rf = _check(hp, I3, Z3, np.tile(d, (len(org), 1)), org, vtx, faces, t_max=32.0)
        total += int((rf >= 0).sum())
        _check(hp, I3, np.array([1.0, -1.0, 0.5]), np.tile(d, (len(org), 1)), org, vtx, faces, t_max=32.0)
    assert total > 1000


def test_range_ends_on_hits(hp):
    vtx, faces = _lattice(10, 10, 4.0, 256.0, 0, 0)
    hp.raycast_build_triangles(vtx, faces)
    dirs = np.concatenate([_grid_rays(5, 4, 256.0), _grid_rays(5, 4, 256.0) * np.float32(2.0)])         # hits at exactly 4 and at exactly 2
    n = len(dirs) // 2
    for t_min, t_max, first, second in ((4.0, 8.0, True, False), (0.0, 4.0, False, True), (2.0, 4.0, False, True), (0.0, 2.0, False, False),
                                        (2.0, np.nextafter(4.0, 5.0), True, True), (np.nextafter(2.0, 3.0), 4.0, False, False), (0.0, 0.5, False, False)):
        _, rf = _check(hp, I3, Z3, dirs, None, vtx, faces, t_min=t_min, t_max=t_max)
        assert bool((rf[:n] >= 0).all()) == first and bool((rf[:n] >= 0).any()) == first, (t_min, t_max)
        assert bool((rf[n:] >= 0).all()) == second and bool((rf[n:] >= 0).any()) == second, (t_min, t_max)


# ---- ANY, points ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_faces,seed", [(300, 21), (5000, 22)])
def test_any_equals_nearest_hit(hp, n_faces, seed):
    rng = np.random.default_rng(seed)
    vtx, faces = _soup(rng, n_faces)
    hp.raycast_build_triangles(vtx, faces)
    rot, pos = _rand_rot(rng), rng.uniform(-2, 2, 3)
    dirs = _aimed(rng, vtx, faces, 3000, pos, rot)
    org = rng.uniform(-1, 1, (3000, 3)).astype(np.float32)
    for o in (None, org):
        t, f = hp.raycast(capi.ray_frame(rot, pos), dirs, o, 0.5, 60.0)
        ta, fa = hp.raycast(capi.ray_frame(rot, pos), dirs, o, 0.5, 60.0, mode=capi.RAY_ANY)
        assert np.array_equal(fa, np.where(f >= 0, 0, -1)) and np.array_equal(ta, np.where(f >= 0, 0, -1).astype(np.float32))
        ra = rcc.cast(rot, pos, dirs, o, 0.5, 60.0, vtx, faces, mode=rcc.ANY)
        assert np.array_equal(ta, ra[0]) and np.array_equal(fa, ra[1])
        assert 0 < (fa == 0).sum() < len(fa)
        # the points are those of the last NEAREST cast, whatever was cast in ANY mode since
        ref = rcc.points(rot, pos, dirs, o, t, 0.05)
        assert np.array_equal(_bits(hp.raycast_points(0.05)), _bits(ref))


def test_points_match_checker(hp):
    rng = np.random.default_rng(31)
    vtx, faces = _soup(rng, 5000)
    hp.raycast_build_triangles(vtx, faces)
    rot, pos = _rand_rot(rng), rng.uniform(-2, 2, 3)
    dirs = _aimed(rng, vtx, faces, 4000, pos, rot, spread=0.05)               # clustered hits: cells shared by several rays
    _, rf = _check(hp, rot, pos, dirs, None, vtx, faces, res=[0.01, 0.05, 0.0, 0.5])
    org = rng.uniform(-1, 1, (4000, 3)).astype(np.float32)
    _check(hp, rot, pos, dirs, org, vtx, faces, res=[0.01, 0.05, 0.0])
    assert len(hp.raycast_points(0.0)) > len(hp.raycast_points(0.5)) > 0
    cap, n = np.zeros((1, 3), np.float32), capi.C.c_int64(0)
    f = hp.lib.immesh_raycast_points
    assert f(hp.raycaster(), 0.0, cap.ctypes.data_as(capi.C.c_void_p), 1, capi.C.byref(n)) == capi.E_CAPACITY and n.value > 1


# ---- the live mesh -----------------------------------------------------------------------------------------------------------------------------------
def _hdl64_dirs(n_az=2032, forward_half=False):
    """the body directions of synth.hdl64_scan's pattern: 64 rings, elevation +2 .. -24.33 degrees, n_az azimuth steps (forward_half: the steps
    with |azimuth| < 90 degrees)"""
    el = np.deg2rad(np.linspace(2.0, -24.33, 64))
    az = np.linspace(-np.pi, np.pi, n_az, endpoint=False)
    if forward_half:
        az = az[np.abs(az) < np.pi / 2]
    A, E = np.meshgrid(az, el, indexing="ij")
    return np.stack([np.cos(E) * np.cos(A), np.cos(E) * np.sin(A), np.sin(E)], axis=-1).reshape(-1, 3).astype(np.float32)


def _mesh_scan(h, cfg, k):
    extT = np.array(list(cfg.extT))
    R, t = synth.trajectory_pose(k)
    raw = synth.livox_scan(k, R, t, n_pts=40000, extT=extT)
    pw = (raw[:, :3].astype(np.float64) + extT) @ R.T + t
    pts = raw.copy(); pts[:, :3] = pw.astype(np.float32)
    h.mesh_scan(np.ascontiguousarray(pts), t, frame_idx=k)
    return R, t


def test_live_mesh_snapshot():
    """build_mesh == the checker on mesh_export's arrays, in the HDL-64 pattern from the last pose; the snapshot outlives two more scans.
    The four Livox scans span +-35.2 degrees of azimuth, so their mesh covers less than 19.6 % of a full sweep whatever the caster does (every 16th
    ray of the whole pattern: 14.7 % hit, measured on one MI355X).  The ~8000 rays are therefore every 8th ray of the sweep's forward half: the
    hits, and as many rays again that pass beside the mesh."""
    cfg = _small_cfg()
    h = make_hip(capi.load_hip_library(), cfg)
    try:
        for k in range(4):
            R, t = _mesh_scan(h, cfg, k)
        nv, nf, n_in = h.raycast_build_mesh(1.0, 20)
        vtx, faces = h.mesh_export(1.0, 20)
        assert (nv, nf) == (len(vtx), len(faces)) and 0 < n_in <= nf
        frame = h.ray_frame_from_state(capi.make_state(R=R, t=t))
        rot, pos = np.array(list(frame.rot)).reshape(3, 3), np.array(list(frame.pos))
        dirs = np.ascontiguousarray(_hdl64_dirs(forward_half=True)[::8])        # 1015 azimuth steps x 64 rings / 8 = 8120 rays
        tt, ff = h.raycast(frame, dirs, None, 0.5, 100.0)
        pts = h.raycast_points(0.01)
        rt, rf = rcc.cast(rot, pos, dirs, None, 0.5, 100.0, vtx, faces)
        assert np.array_equal(ff, rf) and np.array_equal(_bits(tt), _bits(rt))
        assert np.array_equal(_bits(pts), _bits(rcc.points(rot, pos, dirs, None, rt, 0.01)))
        assert (rf >= 0).mean() > 0.2, (rf >= 0).mean()
        for k in range(4, 6):
            _mesh_scan(h, cfg, k)
        vtx2, faces2 = h.mesh_export(1.0, 20)                                   # overwrites the context's export buffers
        assert len(faces2) != len(faces)
        t2, f2 = h.raycast(frame, dirs, None, 0.5, 100.0)
        assert t2.tobytes() == tt.tobytes() and f2.tobytes() == ff.tobytes()    # the old snapshot, the old bits
        assert h.raycast_build_mesh(1.0, 20)[:2] == (len(vtx2), len(faces2))
    finally:
        h.close()


def test_no_side_effects_on_the_maps():
    """a context that builds and casts between scans ends with the same mesh and the same plane table as one that never does"""
    lib = capi.load_hip_library()
    cfg = capi.avia_config(cap_root_voxels=1 << 15, cap_scan_points=100000)
    a, b = make_hip(lib, cfg), make_hip(lib, cfg)
    try:
        extT = np.array(list(cfg.extT))
        dirs = np.ascontiguousarray(_hdl64_dirs()[::64])
        R, t = synth.trajectory_pose(0)
        raw = synth.livox_scan(0, R, t, n_pts=20000, extT=extT)
        for h in (a, b):
            h.map_build(np.ascontiguousarray(raw[:, :3]), capi.make_state(R=R, t=t))
        for k in range(1, 4):
            R, t = synth.trajectory_pose(k)
            raw = synth.livox_scan(k, R, t, n_pts=20000, extT=extT)
            down = synth.voxel_grid_downsample(raw, 0.4)
            prior = capi.make_state(R=R, t=t + np.array([0.01, 0.0, -0.01]), cov_diag=1e-5)
            sa, ia = a.process_scan(down, raw, prior, prior, frame_idx=k, do_mesh=True)
            sb, ib = b.process_scan(down, raw, prior, prior, frame_idx=k, do_mesh=True)
            assert ia == ib and np.array_equal(sa, sb)
            a.raycast_build_mesh(1.0, 20)
            _, f = a.raycast(a.ray_frame_from_state(sa), dirs, None, 0.5, 100.0)
            a.raycast_points(0.01)
        assert (f >= 0).any()
        ea, eb = a.mesh_export(1.0, 20), b.mesh_export(1.0, 20)
        assert len(ea[1]) > 0 and ea[0].tobytes() == eb[0].tobytes() and ea[1].tobytes() == eb[1].tobytes()
        assert compare_plane_tables_fast(a.dump_planes(), b.dump_planes(), 0.0) > 100
    finally:
        a.close(); b.close()


# ---- the rasterizer on the same rays ------------------------------------------------------------------------------------------------------------------
def test_rasterizer_cross_check(hp):
    """the pixel rays of a 640 x 480 camera cast at a soup == render_triangles' depth and face images of it (the renderer has no Box rule and works in
    the camera's frame: the soup is one on which the two contracts agree everywhere, which the two checkers establish first)"""
    cam = pinhole_camera(PINHOLE["cam_seed"], 640, 480, 256.0)
    vtx, faces = pinhole_soup(PINHOLE["soup_seed"], PINHOLE["n_faces"], size=PINHOLE["size"])
    rot, pos = np.array(list(cam.rot)).reshape(3, 3), np.array(list(cam.pos))
    dirs = pinhole_rays(cam)
    rt, rf = rcc.cast(rot, pos, dirs, None, cam.z_near, cam.z_far, vtx, faces)
    n_diff, n_seen = pinhole_differences(cam, vtx, faces, rt, rf)
    assert n_diff == 0 and n_seen > 0.05 * 640 * 480, (n_diff, n_seen)
    hp.raycast_build_triangles(vtx, faces)
    t, f = hp.raycast(capi.ray_frame(rot, pos), dirs, None, cam.z_near, cam.z_far)
    depth, face = hp.render_triangles(cam, vtx, faces)
    depth, face = depth.reshape(-1), face.reshape(-1)
    seen = depth >= 0
    assert seen.sum() == n_seen
    assert np.array_equal(_bits(depth[seen]), _bits(t[seen])) and np.array_equal(face[seen], f[seen])
    assert np.all((f[~seen] < 0) | (t[~seen].astype(np.float64) >= 0.99 * cam.z_far))
    print("raycast build / cast ms", hp.raycast_timing()[:2], "render rasterize ms", hp.render_timing()[0])


# ---- determinism, errors, scale -------------------------------------------------------------------------------------------------------------------------
def test_deterministic():
    lib = capi.load_hip_library()
    a, b = make_hip(lib, _small_cfg()), make_hip(lib, _small_cfg())
    try:
        rng = np.random.default_rng(41)
        vtx, faces = _soup(rng, 20000)
        other = _soup(rng, 3000)
        rot, pos = _rand_rot(rng), rng.uniform(-2, 2, 3)
        dirs = _aimed(rng, vtx, faces, 20000, pos, rot)
        fr = capi.ray_frame(rot, pos)
        a.raycast_build_triangles(vtx, faces)
        ta, fa = a.raycast(fr, dirs, None, 0.0, 100.0); pa = a.raycast_points(0.02)
        b.raycast_build_triangles(*other)                                       # b: another soup first, then this one twice
        b.raycast(fr, dirs, None, 0.0, 100.0)
        for _ in range(2):
            b.raycast_build_triangles(vtx, faces)
            tb, fb = b.raycast(fr, dirs, None, 0.0, 100.0); pb = b.raycast_points(0.02)
            assert ta.tobytes() == tb.tobytes() and fa.tobytes() == fb.tobytes() and pa.tobytes() == pb.tobytes()
        assert (fa >= 0).sum() > 1000
    finally:
        a.close(); b.close()


def test_argument_errors():
    h = make_hip(capi.load_hip_library(), _small_cfg())
    try:
        vtx = np.array([[-1, -1, -2], [1, -1, -2], [0, 1, -2]], np.float32)
        faces = np.array([[0, 1, 2]], np.int32)
        dirs = np.array([[0, 0, -1], [0, 0, 1]], np.float32)
        fr = capi.ray_frame()
        with pytest.raises(RuntimeError, match=r"rc=-1: .*built"):
            h.raycast(fr, dirs)                                                  # cast before build
        h.raycast_build_triangles(vtx, faces)

        def still_usable():
            t, f = h.raycast(fr, dirs, None, 0.0, 10.0)
            assert t.tolist() == [2.0, -1.0] and f.tolist() == [0, -1]
            assert np.array_equal(h.raycast_points(0.0), np.array([[0, 0, -2]], np.float32))

        still_usable()
        for t_min, t_max in ((1.0, 1.0), (2.0, 1.0), (-0.5, 1.0), (0.0, np.inf), (np.nan, 1.0), (0.0, np.nan)):
            with pytest.raises(RuntimeError, match=r"rc=-1: .*t_min"):
                h.raycast(fr, dirs, None, t_min, t_max)
            still_usable()
        for bad in (capi.ray_frame(pos=[np.nan, 0, 0]), capi.ray_frame(rot=np.diag([1.0, np.inf, 1.0]))):
            with pytest.raises(RuntimeError, match=r"rc=-1: .*finite"):
                h.raycast(bad, dirs, None, 0.0, 10.0)
            still_usable()
        for bad in ([[0, 1, 3]], [[0, -1, 2]]):
            with pytest.raises(RuntimeError, match=r"rc=-1: .*out of range"):
                h.raycast_build_triangles(vtx, np.array(bad, np.int32))
            still_usable()                                                       # the refused soup left the built one alone
        with pytest.raises(RuntimeError, match=r"rc=-1: .*mode"):
            h.raycast(fr, dirs, None, 0.0, 10.0, mode=7)
        still_usable()
        out, n = np.zeros((1, 3), np.float32), capi.C.c_int64(0)
        h.raycast(fr, np.tile(dirs[:1], (5, 1)), None, 0.0, 10.0)
        f = h.lib.immesh_raycast_points
        assert f(h.raycaster(), 0.0, out.ctypes.data_as(capi.C.c_void_p), 1, capi.C.byref(n)) == capi.E_CAPACITY and n.value == 5
        still_usable()
    finally:
        h.close()


def test_scale(hp):
    """200 000 faces x 100 000 rays; 500 seeded rays against every face in numpy, exact"""
    rng = np.random.default_rng(51)
    vtx, faces = _soup(rng, 200000, spread=30.0, size=0.3)
    assert hp.raycast_build_triangles(vtx, faces)[1] == 200000
    rot, pos = _rand_rot(rng), rng.uniform(-2, 2, 3)
    dirs = rng.normal(size=(100000, 3)).astype(np.float32)
    t, f = hp.raycast(capi.ray_frame(rot, pos), dirs, None, 0.05, 200.0)
    ms = hp.raycast_timing()
    print("200k faces x 100k rays: build %.3f ms, cast %.3f ms; hit fraction %.3f" % (ms[0], ms[1], (f >= 0).mean()))
    assert (f >= 0).mean() > 0.2
    pick = np.sort(np.random.default_rng(52).choice(len(dirs), size=500, replace=False))
    rt, rf = rcc.cast(rot, pos, dirs[pick], None, 0.05, 200.0, vtx, faces)
    assert np.array_equal(f[pick], rf) and np.array_equal(_bits(t[pick]), _bits(rt))
