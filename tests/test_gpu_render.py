"""Mesh depth images on the device (include/immesh_render.h): the HIP rasterizer and the reinforced points against the numpy restatement of the
contract (tests/render_checker.py), bit-exact -- triangle soups, the live mesh, determinism, no side effects on the map, argument errors, scale."""
import numpy as np
import pytest

import render_checker as rck
from immesh_amd import capi, synth
from conftest import make_hip

pytestmark = pytest.mark.gpu


def _small_cfg():
    return capi.avia_config(cap_root_voxels=1 << 12, cap_scan_points=200000, cap_vertices=1 << 18, cap_triangles=1 << 20)


@pytest.fixture(scope="module")
def hp():
    h = make_hip(capi.load_hip_library(), _small_cfg())
    yield h
    h.close()


def _rand_rot(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def _soup(rng, n_faces, spread=20.0, size=0.25):
    """random triangles around the origin, with the awkward cases mixed in: degenerate (repeated vertex, collinear), edge-on, NaN vertices,
    duplicate faces (exact ties), faces crossing z_near of a camera at the origin"""
    centres = rng.uniform(-spread, spread, (n_faces, 3))
    near = np.linalg.norm(centres, axis=1) < 6.0                                   # keep clear of the cameras (|pos| <= 2): few screen-sized faces
    centres[near] *= (6.0 / np.maximum(np.linalg.norm(centres[near], axis=1), 1e-3))[:, None]
    vtx = (centres[:, None, :] + rng.normal(scale=size, size=(n_faces, 3, 3))).reshape(-1, 3).astype(np.float32)
    faces = np.arange(3 * n_faces, dtype=np.int32).reshape(-1, 3)
    k = n_faces // 50
    if k == 0:
        return vtx, faces
    idx = rng.choice(n_faces, size=6 * k, replace=False)
    d0, d1, d2, d3, d4, d5 = np.split(idx, 6)
    faces[d0, 2] = faces[d0, 1]                                                     # repeated vertex
    v = vtx.reshape(-1, 3, 3)
    v[d1, 2] = v[d1, 0] + np.float32(2.0) * (v[d1, 1] - v[d1, 0])                   # collinear
    v[d2, :, 2] = v[d2, :1, 2]                                                      # flat in z (edge-on for a camera looking along z)
    v[d3, 1, 0] = np.nan                                                            # NaN vertex
    v[d4, :, 2] = np.array([0.02, -1.0, -3.0], np.float32)                          # straddles z_near = 0.05 of a camera at the origin
    faces[d5] = faces[(d5 + 1) % n_faces]                                           # duplicate faces: exact ties, the lower index wins
    return vtx, faces


def _lattice(nx, ny, z, f, w, h, step_px=8):
    """a grid of quads whose vertices and edges lie exactly on pixel rays of a camera at the origin looking along -z"""
    us = np.arange(-(nx // 2), nx // 2 + 1) * step_px
    vs = np.arange(-(ny // 2), ny // 2 + 1) * step_px
    X, Y = np.meshgrid(us * z / f, -vs * z / f)
    vtx = np.stack([X, Y, np.full_like(X, -z)], axis=-1).reshape(-1, 3).astype(np.float32)
    cols = len(us)
    faces = []
    for j in range(len(vs) - 1):
        for i in range(cols - 1):
            a, b, c, d = j * cols + i, j * cols + i + 1, (j + 1) * cols + i + 1, (j + 1) * cols + i
            faces += [(a, b, c), (a, c, d)]
    return vtx, np.array(faces, np.int32)


def _check(hp, cam, vtx, faces):
    depth, face = hp.render_triangles(cam, vtx, faces)
    rd, rf = rck.render(cam, vtx, faces)
    assert np.array_equal(depth.view(np.uint32), rd.view(np.uint32)), int((depth.view(np.uint32) != rd.view(np.uint32)).sum())
    assert np.array_equal(face, rf), int((face != rf).sum())
    pts = hp.render_points()
    ref = rck.reinforce(cam, rd)
    assert pts.shape == ref.shape and np.array_equal(pts.view(np.uint32), ref.view(np.uint32))
    return depth, face, pts


@pytest.mark.parametrize("n_faces,size,seed", [(1, (640, 480), 0), (100, (640, 480), 1), (5000, (640, 480), 2), (30000, (1920, 1080), 3),
                                               (200000, (640, 480), 4), (20000, (333, 517), 5)])
def test_soup_matches_checker(hp, n_faces, size, seed):
    rng = np.random.default_rng(seed)
    vtx, faces = _soup(rng, n_faces)
    covered = 0
    for pose in range(3):
        cam = hp.default_depth_camera(width=size[0], height=size[1])
        if pose:
            cam.rot[:] = _rand_rot(rng).reshape(-1)
            cam.pos[:] = rng.uniform(-2, 2, 3)
        if pose == 2:
            cam.downsample_res = 0.0                  # every valid pixel
        depth, _, pts = _check(hp, cam, vtx, faces)
        covered += int((depth >= 0).sum())
        assert len(pts) <= int((depth >= 0).sum())
    if n_faces >= 5000:
        assert covered > 0.05 * size[0] * size[1]


def test_lattice_on_pixel_rays(hp):
    """edges and vertices exactly on pixel rays: the inclusive edge rule and the lower-index tie-break decide, identically"""
    for (w, h) in ((640, 480), (1920, 1080)):
        cam = hp.default_depth_camera(width=w, height=h, downsample_res=0.05)
        vtx, faces = _lattice(60, 40, 3.125, cam.focus, w, h)      # 3.125 / 400 = 2^-7: every vertex exactly on a pixel ray
        depth, face, _ = _check(hp, cam, vtx, faces)
        assert (depth >= 0).sum() >= 480 * 320
        assert np.all(depth[depth >= 0] == np.float32(3.125))


def test_live_mesh(hp):
    """render_mesh == the checker on mesh_export's arrays, at the last scan's pose, for smooth_factor 1 and 0"""
    cfg = _small_cfg()
    h = make_hip(capi.load_hip_library(), cfg)
    try:
        extT = np.array(list(cfg.extT))
        for k in range(4):
            R, t = synth.trajectory_pose(k)
            raw = synth.livox_scan(k, R, t, n_pts=40000, extT=extT)
            pw = (raw[:, :3].astype(np.float64) + extT) @ R.T + t
            pts = raw.copy(); pts[:, :3] = pw.astype(np.float32)
            h.mesh_scan(np.ascontiguousarray(pts), t, frame_idx=k)
        cam = h.camera_from_state(capi.make_state(R=R, t=t))
        for factor in (1.0, 0.0):
            depth, face = h.render_mesh(cam, factor, 20)
            pts_dev = h.render_points()
            vtx, faces = h.mesh_export(factor, 20)
            rd, rf = rck.render(cam, vtx, faces)
            assert np.array_equal(depth.view(np.uint32), rd.view(np.uint32))
            assert np.array_equal(face, rf)
            assert np.array_equal(pts_dev.view(np.uint32), rck.reinforce(cam, rd).view(np.uint32))
            assert (depth >= 0).mean() > 0.05, (depth >= 0).mean()
    finally:
        h.close()


def test_deterministic_and_no_side_effects():
    """two renders give identical bytes; the export before and after a render is identical; a stream that renders after every scan yields the
    same mesher lists as the same stream without rendering"""
    lib = capi.load_hip_library()
    cfg = _small_cfg()
    a, b = make_hip(lib, cfg), make_hip(lib, cfg)
    try:
        extT = np.array(list(cfg.extT))
        for k in range(4):
            R, t = synth.trajectory_pose(k)
            raw = synth.livox_scan(k, R, t, n_pts=30000, extT=extT)
            pw = (raw[:, :3].astype(np.float64) + extT) @ R.T + t
            pts = raw.copy(); pts[:, :3] = pw.astype(np.float32)
            pts = np.ascontiguousarray(pts)
            ma = a.mesh_scan(pts, t, frame_idx=k)
            cam = a.camera_from_state(capi.make_state(R=R, t=t))
            before = a.mesh_export(1.0, 20)
            d1, f1 = a.render_mesh(cam, 1.0, 20); p1 = a.render_points()
            d2, f2 = a.render_mesh(cam, 1.0, 20); p2 = a.render_points()
            after = a.mesh_export(1.0, 20)
            assert d1.tobytes() == d2.tobytes() and f1.tobytes() == f2.tobytes() and p1.tobytes() == p2.tobytes()
            assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes()
            mb = b.mesh_scan(pts, t, frame_idx=k)
            for key in ("new_vtx", "tri_add", "tri_rem", "tri_upd", "flip_add", "flip_upd", "smooth_ids", "smooth_xyz"):
                assert np.asarray(ma[key]).tobytes() == np.asarray(mb[key]).tobytes(), (k, key)
    finally:
        a.close(); b.close()


def test_argument_errors(hp):
    vtx = np.zeros((3, 3), np.float32); vtx[1, 0] = 1; vtx[2, 1] = 1; vtx[:, 2] = -2
    faces = np.array([[0, 1, 2]], np.int32)
    hp.render_triangles(hp.default_depth_camera(), vtx, faces)
    n_before = len(hp.render_points())
    bad = [dict(width=0), dict(height=-3), dict(width=8193), dict(focus=0.0), dict(focus=float("nan")), dict(z_near=0.0),
           dict(z_near=5.0, z_far=5.0), dict(z_far=float("inf")), dict(pos=[np.nan, 0, 0])]
    for over in bad:
        with pytest.raises(RuntimeError, match="rc=-1"):
            hp.render_triangles(hp.default_depth_camera(**over), vtx, faces)
        with pytest.raises(RuntimeError, match="rc=-1"):
            hp.render_mesh(hp.default_depth_camera(**over))
        assert len(hp.render_points()) == n_before                 # rejected before any launch: the last render's points stand
    with pytest.raises(RuntimeError, match="out of range"):
        hp.render_triangles(hp.default_depth_camera(), vtx, np.array([[0, 1, 3]], np.int32))
    with pytest.raises(RuntimeError, match="out of range"):
        hp.render_triangles(hp.default_depth_camera(), vtx, np.array([[0, -1, 2]], np.int32))


def test_scale_one_million_faces(hp):
    """~1 M faces at 640 x 480: at ~200 sampled pixels the winner covers the pixel and no face is nearer (all faces, numpy)"""
    rng = np.random.default_rng(7)
    n = 1 << 20
    vtx, faces = _soup(rng, n, spread=30.0, size=0.3)
    cam = hp.default_depth_camera()
    cam.rot[:] = _rand_rot(rng).reshape(-1)
    depth, face = hp.render_triangles(cam, vtx, faces)
    assert (depth >= 0).mean() > 0.2
    S = rck.face_setup(cam, vtx, faces)
    fin = np.nonzero(S["finite"])[0]                       # every face with finite vertices, whatever its box says
    w = cam.width
    best = np.full(w * cam.height, rck._NONE, np.uint64)
    for p in rng.choice(w * cam.height, size=200, replace=False):
        u, v = int(p % w), int(p // w)
        rck._test_pairs(cam, S, fin, np.full(len(fin), u), np.full(len(fin), v), best)
        key = best[p]
        d32 = np.array([key >> np.uint64(32)], np.uint64).astype(np.uint32).view(np.float32)[0]
        if key != rck._NONE and float(d32) < 0.99 * cam.z_far:
            assert depth[v, u] == d32 and face[v, u] == int(key & np.uint64(0xFFFFFFFF)), (u, v)
        else:
            assert depth[v, u] == -1 and face[v, u] == -1, (u, v)
