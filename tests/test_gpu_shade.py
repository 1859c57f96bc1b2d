"""Shaded and coloured images of the mesh on the device (include/immesh_shade.h) against the numpy restatement of the contract
(tests/shade_checker.py on tests/render_checker.py), byte for byte: triangle soups with every colour source, ties on pixel rays, a colour ramp, the
axis range, the live mesh coloured from camera images, determinism, no side effects, argument errors."""
import numpy as np
import pytest

import render_checker as rck
import shade_checker as sck
from immesh_amd import capi, synth
from conftest import make_hip

pytestmark = pytest.mark.gpu

BASE = np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])   # a camera of immesh_image on the LiDAR: z along its +x, x to the right, y down
SOURCES = (capi.SHADE_WHITE, capi.SHADE_AXIS, capi.SHADE_VERTEX)


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


def _soup(rng, n_faces, spread=12.0, size=0.6):
    """random triangles around the origin that share vertices with their neighbours in the list (so a vertex colour is read through several faces),
    with the awkward cases mixed in: a repeated vertex, NaN vertices, duplicate faces (exact ties), a vertex no face uses"""
    centres = rng.uniform(-spread, spread, (n_faces, 3))
    near = np.linalg.norm(centres, axis=1) < 4.0
    centres[near] *= (4.0 / np.maximum(np.linalg.norm(centres[near], axis=1), 1e-3))[:, None]
    vtx = (centres[:, None, :] + rng.normal(scale=size, size=(n_faces, 3, 3))).reshape(-1, 3).astype(np.float32)
    vtx = np.concatenate([vtx, np.array([[1e3, -1e3, 77.0]], np.float32)])          # unreferenced: it counts for the axis range all the same
    faces = np.arange(3 * n_faces, dtype=np.int32).reshape(-1, 3)
    k = n_faces // 25
    if k:
        idx = rng.choice(n_faces - 1, size=4 * k, replace=False)
        d0, d1, d2, d3 = np.split(idx, 4)
        faces[d0, 2] = faces[d0, 1]                                                  # repeated vertex
        vtx[3 * d1 + 1, 0] = np.nan                                                  # NaN vertex
        faces[d2] = faces[d2 + 1]                                                    # duplicate faces: the lower index wins
        faces[d3, 0] = faces[d3 + 1, 0]                                              # a vertex shared with the next face
    return vtx, faces


def _lattice(nx, ny, z, f, step_px=8):
    """a grid of quads whose vertices and edges lie exactly on pixel rays of a camera at the origin looking along -z (the render tests' lattice)
    -> vertices, faces, the vertices' pixel offsets (du, dv) from the principal point"""
    us = np.arange(-(nx // 2), nx // 2 + 1) * step_px
    vs = np.arange(-(ny // 2), ny // 2 + 1) * step_px
    X, Y = np.meshgrid(us * z / f, -vs * z / f)
    vtx = np.stack([X, Y, np.full_like(X, -z)], axis=-1).reshape(-1, 3).astype(np.float32)
    DU, DV = np.meshgrid(us, vs)
    cols = len(us)
    faces = []
    for j in range(len(vs) - 1):
        for i in range(cols - 1):
            a, b, c, d = j * cols + i, j * cols + i + 1, (j + 1) * cols + i + 1, (j + 1) * cols + i
            faces += [(a, b, c), (a, c, d)]
    return vtx, np.array(faces, np.int32), np.stack([DU.reshape(-1), DV.reshape(-1)], axis=-1)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _reference(hp, cam, vtx, faces):
    """what every shading of one input shares: the plain render on the device, the checker's render, the checker's per-pixel weights and light"""
    dev, ref = hp.render_triangles(cam, vtx, faces), rck.render(cam, vtx, faces)
    return dev, ref, sck.pixel_terms(cam, vtx, faces, ref[1])


def _check(hp, cam, vtx, faces, sh, col, ref_df):
    """one shade call against the checker (and against the plain render's depth / face, both from the device and the checker)"""
    rgb, depth, face = hp.shade_triangles(cam, vtx, faces, sh, vtx_rgb=col)
    want, _, _, lo_hi = sck.shade(cam, vtx, faces, sh, col, depth_face=ref_df[1], terms=ref_df[2])
    assert _same(depth, ref_df[0][0]) and _same(face, ref_df[0][1])                 # byte-identical to immesh_render_triangles
    assert _same(depth, ref_df[1][0]) and _same(face, ref_df[1][1])
    bad = np.nonzero((rgb != want).any(axis=2))
    assert len(bad[0]) == 0, (len(bad[0]), [(int(v), int(u), rgb[v, u].tolist(), want[v, u].tolist()) for v, u in zip(bad[0][:5], bad[1][:5])])
    assert (rgb[face < 0] == np.array(list(sh.background), np.uint8)).all()
    assert hp.shade_range() == lo_hi
    return rgb, depth, face


@pytest.mark.parametrize("n_faces,size,focus,seed", [(1, (160, 120), 100.0, 0), (100, (160, 120), 100.0, 1), (5000, (160, 120), 100.0, 2),
                                                     (3000, (640, 480), 400.0, 3), (800, (333, 217), 200.0, 4)])
def test_soup_matches_checker(hp, n_faces, size, focus, seed):
    rng = np.random.default_rng(seed)
    vtx, faces = _soup(rng, n_faces) if n_faces > 1 else (np.array([[-3, -2, -6], [4, -1, -9], [0, 3, -5]], np.float32), np.array([[0, 1, 2]], np.int32))
    col = rng.integers(0, 256, (len(vtx), 3)).astype(np.uint8)
    cam = hp.default_depth_camera(width=size[0], height=size[1], focus=focus)
    if seed >= 2:
        cam.rot[:] = _rand_rot(rng).reshape(-1)
        cam.pos[:] = rng.uniform(-1, 1, 3)
    ref_df = _reference(hp, cam, vtx, faces)
    pts = hp.render_points()
    assert (ref_df[0][1] >= 0).mean() > (0.2 if n_faces >= 800 else 0.005)
    distinct = set()
    for source in SOURCES:
        for light in (1, 0):
            sh = hp.default_shade(source=source, light=light, axis=seed % 3, background=(10 + seed, 20, 250))
            rgb, _, _ = _check(hp, cam, vtx, faces, sh, col if source == capi.SHADE_VERTEX else None, ref_df)
            distinct.add(rgb.tobytes())
            assert _same(hp.render_points(), pts)                                    # the reinforced points are the render's
    sh = hp.default_shade(source=capi.SHADE_VERTEX, bgr=1)
    rgb, _, _ = _check(hp, cam, vtx, faces, sh, col, ref_df)
    distinct.add(rgb.tobytes())
    assert len(distinct) == 7
    # any output may be left out
    only_rgb = hp.shade_triangles(cam, vtx, faces, sh, vtx_rgb=col, want_depth=False, want_face=False)
    assert only_rgb[1] is None and only_rgb[2] is None and _same(only_rgb[0], rgb)
    none = hp.shade_triangles(cam, vtx, faces, sh, vtx_rgb=col, want_rgb=False, want_depth=False)
    assert none[0] is None and _same(none[2], ref_df[0][1])


def test_ties_on_pixel_rays(hp):
    """the render tests' lattice with vertex colours (3.125 / 400 = 2^-7: every vertex on a pixel ray), byte-equal to the checker; and the same
    lattice at focus 512, depth 4, where the rays' directions du / 512 are exact too, so every edge function of the contract is: edges and vertices
    are inclusive and the smaller face index wins, a pixel on a lattice vertex shows that vertex's colour through the lowest face that touches it"""
    w, h = 640, 480
    rng = np.random.default_rng(5)
    for focus, z in ((400.0, 3.125), (512.0, 4.0)):
        cam = hp.default_depth_camera(width=w, height=h, focus=focus, downsample_res=0.05)
        vtx, faces, duv = _lattice(60, 40, z, focus)
        col = rng.integers(0, 256, (len(vtx), 3)).astype(np.uint8)
        ref_df = _reference(hp, cam, vtx, faces)
        for light in (1, 0):
            rgb, depth, face = _check(hp, cam, vtx, faces, hp.default_shade(source=capi.SHADE_VERTEX, light=light), col, ref_df)
        assert (depth >= 0).sum() >= 480 * 320 and np.all(depth[depth >= 0] == np.float32(z))
    lowest = np.full(len(vtx), len(faces), np.int64)
    np.minimum.at(lowest, faces.reshape(-1), np.repeat(np.arange(len(faces)), 3))
    u, v = w // 2 + duv[:, 0], h // 2 + duv[:, 1]
    assert np.array_equal(face[v, u], lowest)
    assert np.array_equal(rgb[v, u], col)                                            # (unlit: the last pass) weights 1, 0, 0
    # along an interior edge both faces cover the pixel: the lower index has it
    on_edge = (u[0] + 3, v[0])                                                       # between the first two vertices of the top row: faces 0 only
    assert face[on_edge[1], on_edge[0]] == 0
    shared = (u[0] + 3, v[0] + 3)                                                    # the diagonal a-c of the first quad: faces 0 and 1
    assert face[shared[1], shared[0]] == 0


def test_ramp_is_reproduced_within_one_level(hp):
    """fronto-parallel lattice, vertex bytes = a linear ramp of the vertices' pixel positions, unlit: interpolation over a fronto-parallel plane is
    exact in the image, so the picture is the ramp up to half a level from the vertex bytes' rounding and half a level from the output's"""
    w, h = 640, 480
    cam = hp.default_depth_camera(width=w, height=h)
    vtx, faces, duv = _lattice(60, 40, 3.125, cam.focus)

    def ramp(u, v):
        return np.stack([0.37 * u + 3.2, 0.45 * v + 10.0, 0.2 * u + 0.2 * v + 5.0], axis=-1)

    col = np.floor(ramp(w // 2 + duv[:, 0], h // 2 + duv[:, 1]) + 0.5).astype(np.uint8)
    rgb, depth, face = hp.shade_triangles(cam, vtx, faces, hp.default_shade(source=capi.SHADE_VERTEX, light=0), vtx_rgb=col)
    vv, uu = np.nonzero(face >= 0)
    assert len(uu) >= 480 * 320
    err = np.abs(rgb[vv, uu].astype(np.float64) - ramp(uu, vv))
    assert err.max() <= 1.0, err.max()
    assert err.max() > 0.4                                                           # (the bound is not slack)


def test_axis_range(hp):
    rng = np.random.default_rng(9)
    vtx, faces = _soup(rng, 400)
    vtx[5] = [np.nan, 0.0, 1e6]                                                     # not finite: its large z does not count
    vtx[9] = [0.0, np.inf, -1e6]
    cam = hp.default_depth_camera(width=160, height=120, focus=100.0)
    ref_df = _reference(hp, cam, vtx, faces)
    fin = np.isfinite(vtx).all(axis=1)
    assert not fin.all()
    for axis in (0, 1, 2):
        sh = hp.default_shade(source=capi.SHADE_AXIS, axis=axis)
        _check(hp, cam, vtx, faces, sh, None, ref_df)
        assert hp.shade_range() == (float(vtx[fin, axis].min()), float(vtx[fin, axis].max()))
    assert hp.shade_range()[1] == 77.0                                               # the vertex no face uses
    # an explicit range (the reference's running range is the caller's to keep): vertices outside it clamp to the table's ends
    sh = hp.default_shade(source=capi.SHADE_AXIS, axis=2, axis_min=-3.3, axis_max=4.7)
    rgb, _, _ = _check(hp, cam, vtx, faces, sh, None, ref_df)
    assert hp.shade_range() == (float(np.float32(-3.3)), float(np.float32(4.7)))
    hp.shade_triangles(cam, vtx, faces, hp.default_shade())
    assert hp.shade_range() == (0.0, 0.0)                                            # not an AXIS pass
    # hi <= lo after resolution: every finite vertex at one height -> val = 0 -> red, lit or not
    quad = np.array([[-2, -2, -3], [2, -2, -3], [2, 2, -3], [-2, 2, -3]], np.float32)
    qf = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    qdf = _reference(hp, cam, quad, qf)
    rgb, _, face = _check(hp, cam, quad, qf, hp.default_shade(source=capi.SHADE_AXIS, light=0), None, qdf)
    assert hp.shade_range() == (-3.0, -3.0) and (rgb[face >= 0] == [255, 0, 0]).all() and (face >= 0).any()
    # no finite vertex at all: range 0 / 0, nothing drawn
    nanv = np.full((3, 3), np.nan, np.float32)
    rgb, _, face = hp.shade_triangles(cam, nanv, np.array([[0, 1, 2]], np.int32), hp.default_shade(source=capi.SHADE_AXIS, background=(1, 2, 3)))
    assert hp.shade_range() == (0.0, 0.0) and (face == -1).all() and (rgb == [1, 2, 3]).all()
    # no vertex and no face
    rgb, _, face = hp.shade_triangles(cam, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), hp.default_shade(source=capi.SHADE_AXIS))
    assert hp.shade_range() == (0.0, 0.0) and (face == -1).all() and (rgb == 0).all()


def _image(h, R, t, seed):
    """a 320 x 240 frame of a camera on the LiDAR at pose (R, t), narrower than the LiDAR's field of view: some vertices stay unseen"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:240, 0:320]
    px = np.stack([x * 255 // 319, y * 255 // 239, (x * 3 + y * 5 + seed * 37) % 256], axis=-1).astype(np.uint8)
    px[60:120, 80:160] = rng.integers(1, 256, (60, 80, 3))
    return h.default_image(px, fx=300.0, fy=300.0, cx=159.7, cy=120.2, rot=R @ BASE, pos=t, obs_time=0.1 * seed, inv_exposure=0.01 + 0.002 * seed)


@pytest.fixture(scope="module")
def live():
    """a short scan stream (the size of the render tests' live mesh), coloured by two frames: the second sees a part of what the first saw"""
    cfg = _small_cfg()
    h = make_hip(capi.load_hip_library(), cfg)
    extT = np.array(list(cfg.extT))
    for k in range(4):
        R, t = synth.trajectory_pose(k)
        raw = synth.livox_scan(k, R, t, n_pts=40000, extT=extT)
        pw = (raw[:, :3].astype(np.float64) + extT) @ R.T + t
        pts = raw.copy(); pts[:, :3] = pw.astype(np.float32)
        h.mesh_scan(np.ascontiguousarray(pts), t, frame_idx=k)
    cam = h.camera_from_state(capi.make_state(R=R, t=t))
    h.colour_image(_image(h, R, t, 1), capi.COLOUR_PLAIN, capi.COLOUR_SET_ALL)
    h.colour_image(_image(h, R @ synth.yaw_R(0.25), t, 2), capi.COLOUR_PLAIN, capi.COLOUR_SET_ALL)
    yield h, cam
    h.close()


def test_live_mesh(live):
    """shade_mesh == the checker fed with mesh_export and colour_fetch, for every source; min_views = 2 blacks out the vertices one frame saw"""
    h, cam = live
    vtx, faces = h.mesh_export(1.0, 20)
    rgb_v, st = h.colour_fetch(n=len(vtx))
    assert (st["n_obs"] >= 2).sum() > 100 and (st["n_obs"] == 1).sum() > 100 and (st["n_obs"] == 0).sum() > 100
    ref = rck.render(cam, vtx, faces)
    plain = h.render_mesh(cam, 1.0, 20)
    assert (ref[0] >= 0).mean() > 0.05
    seen_black = False
    for source, over in ((capi.SHADE_WHITE, {}), (capi.SHADE_AXIS, {}), (capi.SHADE_VERTEX, dict(min_views=2, bgr=1)), (capi.SHADE_VERTEX, dict(light=0))):
        sh = h.default_shade(source=source, background=(30, 30, 60), **over)
        rgb, depth, face = h.shade_mesh(cam, sh, 1.0, 20)
        assert _same(depth, plain[0]) and _same(face, plain[1]) and _same(depth, ref[0]) and _same(face, ref[1])
        col = sck.colourer_bytes(rgb_v, st, sh.min_views) if source == capi.SHADE_VERTEX else None
        want, _, _, lo_hi = sck.shade(cam, vtx, faces, sh, col, depth_face=ref)
        assert int((rgb != want).any(axis=2).sum()) == 0
        assert h.shade_range() == lo_hi
        if source == capi.SHADE_AXIS:
            fin = np.isfinite(vtx).all(axis=1)
            assert lo_hi == (float(vtx[fin, 2].min()), float(vtx[fin, 2].max())) and lo_hi[0] < lo_hi[1]
        if over.get("min_views"):
            cov = face >= 0
            assert (rgb[cov] == 0).all(axis=1).any() and (rgb[cov] != 0).any(axis=1).any()
            seen_black = True
    assert seen_black
    # the raw positions (smooth_factor 0) are another export: still the checker's picture
    vtx0, faces0 = h.mesh_export(0.0, 20)
    sh = h.default_shade(source=capi.SHADE_VERTEX)
    rgb, depth, face = h.shade_mesh(cam, sh, 0.0, 20)
    want, wd, wf, _ = sck.shade(cam, vtx0, faces0, sh, sck.colourer_bytes(rgb_v, st, 0))
    assert _same(depth, wd) and _same(face, wf) and int((rgb != want).any(axis=2).sum()) == 0


def test_deterministic_and_no_side_effects(live):
    h, cam = live
    n = h.counters()["n_vertices"]
    export_before, colour_before = h.mesh_export(1.0, 20), h.colour_fetch(n=n)
    h.render_mesh(cam, 1.0, 20)
    pts_plain, timing_plain = h.render_points(), h.render_timing()
    assert len(pts_plain) > 0 and timing_plain[0] > 0
    for source in SOURCES:
        sh = h.default_shade(source=source, min_views=1)
        a = h.shade_mesh(cam, sh, 1.0, 20)
        pts_a = h.render_points()
        b = h.shade_mesh(cam, sh, 1.0, 20)
        assert all(_same(x, y) for x, y in zip(a, b))
        assert _same(pts_a, pts_plain) and _same(h.render_points(), pts_plain)      # render_points after a shade call = after a plain render
        assert h.render_timing()[0] > 0 and h.shade_timing() > 0
    export_after, colour_after = h.mesh_export(1.0, 20), h.colour_fetch(n=n)
    assert _same(export_before[0], export_after[0]) and _same(export_before[1], export_after[1])
    assert _same(colour_before[0], colour_after[0]) and colour_before[1].tobytes() == colour_after[1].tobytes()


def test_argument_errors(live):
    h, cam = live
    lib = h.lib
    vtx = np.array([[0, 0, -2], [1, 0, -2], [0, 1, -2]], np.float32)
    faces = np.array([[0, 1, 2]], np.int32)
    col = np.full((3, 3), 200, np.uint8)
    good = h.default_shade(source=capi.SHADE_AXIS, axis_min=-5.0, axis_max=5.0)
    h.shade_triangles(cam, vtx, faces, good)
    before = (h.render_points().tobytes(), h.shade_range(), h.shade_timing(), h.render_timing())
    assert before[1] == (-5.0, 5.0)

    def undisturbed():
        assert (h.render_points().tobytes(), h.shade_range(), h.shade_timing(), h.render_timing()) == before

    bad = [(dict(source=3), "source"), (dict(source=-1), "source"), (dict(axis=3), "axis"), (dict(axis=-1), "axis"),
           (dict(axis_min=float("nan")), "range"), (dict(axis_max=float("inf")), "range"), (dict(axis_min=-float("inf"), axis_max=1.0), "range"),
           (dict(axis_min=0.0, axis_max=1e300), "range")]
    for over, match in bad:
        sh = h.default_shade(**over)
        with pytest.raises(RuntimeError, match=r"rc=-1: .*" + match):
            h.shade_triangles(cam, vtx, faces, sh, vtx_rgb=col)
        undisturbed()
        with pytest.raises(RuntimeError, match=r"rc=-1: .*" + match):
            h.shade_mesh(cam, sh)
        undisturbed()
    vertex = h.default_shade(source=capi.SHADE_VERTEX)
    with pytest.raises(RuntimeError, match=r"rc=-1: .*without vertex colours"):
        h.shade_triangles(cam, vtx, faces, vertex)
    undisturbed()
    with pytest.raises(RuntimeError, match=r"rc=-1: .*without a colourer"):
        h.shade_mesh(cam, vertex, colourer=None)
    undisturbed()
    with pytest.raises(RuntimeError, match=r"rc=-1"):                               # the camera's checks come first, as in a render
        h.shade_triangles(hp_cam_bad(h), vtx, faces, good)
    undisturbed()
    with pytest.raises(RuntimeError, match="out of range"):
        h.shade_triangles(cam, vtx, np.array([[0, 1, 3]], np.int32), good)
    undisturbed()
    other = make_hip(lib, _small_cfg())
    try:
        with pytest.raises(RuntimeError, match=r"rc=-1: .*another context"):
            h.shade_mesh(cam, vertex, colourer=other.colourer())
        undisturbed()
    finally:
        other.close()
    sharded = make_hip(lib, capi.avia_config(cap_root_voxels=1 << 12, cap_scan_points=100000, cap_vertices=1 << 16, cap_triangles=1 << 18,
                                             shard_world=2, shard_rank=0, shard_mesh=1))
    try:
        with pytest.raises(RuntimeError, match=r"rc=-1: .*shard"):
            sharded.shade_mesh(cam, sharded.default_shade())
    finally:
        sharded.close()
    # and the good call still works afterwards
    rgb, _, face = h.shade_triangles(h.default_depth_camera(), vtx, faces, vertex, vtx_rgb=col)
    assert (face >= 0).any() and (rgb[face >= 0] > 0).all()


def hp_cam_bad(h):
    return h.default_depth_camera(width=0)
