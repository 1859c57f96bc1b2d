"""Vertex colours from camera images on the device (include/immesh_colour.h) against the numpy restatement of the contract (tests/colour_checker.py):
bit-exact for the PLAIN model, the sampling, the selection and the RECENT sets; to rounding (1e-12 relative, COVERAGE row a13's bound for results that
differ only by rounding order: the device's acos is not libm's) for the VIEW model.  Determinism, no side effects on the map, the coloured PLY,
argument errors."""
import numpy as np
import pytest

import colour_checker as cck
from immesh_amd import capi, synth
from conftest import make_hip

pytestmark = pytest.mark.gpu

CAPS = dict(cap_root_voxels=1 << 12, cap_scan_points=100000, cap_vertices=1 << 16, cap_triangles=1 << 18)
BASE = np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])   # camera z along world +x, x to the right (-y), y down (-z)
EXPOSURES = (0.01, 0.012, 0.008, 0.02, 0.01, 0.015, 0.009, 0.011)


def _cfg(**over):
    return capi.avia_config(**CAPS, **over)


def _plane(rng, n, x=None, y=None, z=None, noise=0.01):
    """n scan points (xyzI float32): each coordinate a (lo, hi) range or a constant with noise"""
    pts = np.zeros((n, 4), np.float32)
    for k, a in enumerate((x, y, z)):
        pts[:, k] = rng.uniform(a[0], a[1], n) if isinstance(a, tuple) else a + rng.normal(0.0, noise, n)
    pts[:, 3] = 10.0
    return pts


def _scans():
    """three small scans, below the append budget: a wall ahead that is wider than any view, a wall behind the cameras plus a sheet of points at
    x = 1 +- 2^-20 (pc.z either side of 0.001 for the cameras at x = 0.999), the ground (seen at grazing angles)"""
    rng = np.random.default_rng(11)
    wall = _plane(rng, 6000, x=6.0, y=(-6.0, 6.0), z=(-2.5, 2.5))
    behind = _plane(rng, 1500, x=-4.0, y=(-2.0, 2.0), z=(-1.0, 1.0))
    sheet = _plane(rng, 300, x=1.0, y=(-1.0, 1.0), z=(-0.6, 0.6), noise=0.0)
    sheet[:, 0] = rng.choice(np.array([1.0, 1.0 - 2.0 ** -20, 1.0 + 2.0 ** -20], np.float32), 300)
    ground = _plane(rng, 3000, x=(2.0, 9.0), y=(-3.0, 3.0), z=-1.5)
    return [wall, np.concatenate([behind, sheet]), ground]


def _build(h, scans):
    for k, pts in enumerate(scans):
        h.mesh_scan(np.ascontiguousarray(pts), np.zeros(3), frame_idx=k, fetch=False)
    return h.mesh_export(0.0, 20)[0]          # smooth_factor 0: the raw vertex positions


def _pixels(rows, cols, seed):
    """gradients plus a black and a white patch"""
    y, x = np.mgrid[0:rows, 0:cols]
    px = np.stack([x * 255 // (cols - 1), y * 255 // (rows - 1), (x * 3 + y * 5 + seed * 37) % 256], axis=-1).astype(np.uint8)
    px[rows // 4:rows // 2, cols // 4:cols // 2] = 0
    px[rows // 2:3 * rows // 4, cols // 2:3 * cols // 4] = 255
    return px


def _image(h, k, big=None, **over):
    """frame k of a moving camera: frames 0 and 1 axis-aligned at x = 0.999 (the sheet's pc.z is 1 - 0.999 or a hair less), the others yawed and
    pitched; 64 x 48 for k < 4, else 320 x 240 (big overrides); frame 2 is handed over with a row stride wider than its rows"""
    big = k >= 4 if big is None else big
    rows, cols, f = (240, 320, 200.0) if big else (48, 64, 40.0)
    px = _pixels(rows, cols, k)
    if k == 2:
        wide = np.zeros((rows, cols + 5, 3), np.uint8)
        wide[:, :cols] = px
        px = wide[:, :cols]
    yaw, pitch = (0.0, 0.0) if k < 2 else (0.03 * k - 0.1, 0.02 * k - 0.05)
    cp, sp = np.cos(pitch), np.sin(pitch)
    rot = synth.yaw_R(yaw) @ np.array([[cp, 0.0, sp], [0.0, 1.0, 0.0], [-sp, 0.0, cp]]) @ BASE
    pos = [0.999 + 1e-8 * k, 0.1 * k - 0.3, 0.05 * k - 0.2]
    args = dict(fx=f, fy=f * 1.01, cx=cols / 2 - 0.3, cy=rows / 2 + 0.2, rot=rot, pos=pos, inv_exposure=EXPOSURES[k % 8], obs_time=0.1 * k)
    args.update(over)
    im = h.default_image(px, **args)
    return im, np.ascontiguousarray(px)


def _step(h, ref, vpos, im, px, model, cset, cand, md=0.0, voxel=0.4):
    """one image on the device and on the checker (ref, in place); everything compared -> (device stats, checker stats)"""
    got = h.colour_image(im, model, cset, ids=cand if cset == capi.COLOUR_SET_IDS else None, select_min_dis=md)
    want, sel, uv = cck.colour_image(ref, vpos, px, im, model, cand, md, voxel)
    ids_d, uv_d = h.colour_selected()
    assert np.array_equal(ids_d, sel)
    assert np.array_equal(uv_d, uv, equal_nan=True)
    for key in ("n_set", "n_selected", "n_hit", "n_first", "n_updated", "pe_count"):
        assert got[key] == want[key], (key, got, want)
    rgb_d, st_d = h.colour_fetch(n=len(vpos))
    assert np.array_equal(st_d["n_obs"], ref["n_obs"])
    if model == cck.PLAIN:
        assert st_d.tobytes() == ref.tobytes()
        assert got["min_dis"] == want["min_dis"] and got["pe_sum"] == 0.0
        assert np.array_equal(rgb_d, cck.rgb8(ref))
    else:
        for f in ("rgb", "cov", "first_exposure", "obs_dis", "last_obs_time"):
            np.testing.assert_allclose(st_d[f], ref[f], rtol=1e-12, atol=0.0, err_msg=f)
        np.testing.assert_allclose(got["pe_sum"], want["pe_sum"], rtol=1e-12, atol=0.0)
        assert got["min_dis"] == 0.0
    assert np.array_equal(rgb_d, cck.rgb8(st_d))
    return got, want


@pytest.fixture(scope="module")
def lib():
    return capi.load_hip_library()


@pytest.fixture(scope="module")
def world(lib):
    """the three-scan map; tests take the colour state as they find it (the reference starts from a fetch)"""
    h = make_hip(lib, _cfg())
    scans = _scans()
    vpos = _build(h, scans)
    assert 2000 < len(vpos) < 20000
    yield h, vpos, scans
    h.close()


def _lattice_points():
    """a plane at x = 4 whose points project, for a camera at the origin with f = 32, c = (32, 24), exactly onto (k + 0.5, j + 0.5): 1 pixel = 0.125 m,
    above the 0.1 m minimum spacing"""
    y = -(np.arange(64) + 0.5 - 32.0) / 8.0
    z = -(np.arange(48) + 0.5 - 24.0) / 8.0
    Y, Z = np.meshgrid(y, z)
    pts = np.stack([np.full(Y.size, 4.0), Y.ravel(), Z.ravel(), np.full(Y.size, 10.0)], axis=1).astype(np.float32)
    return pts


@pytest.fixture(scope="module")
def lattice(lib):
    h = make_hip(lib, _cfg())
    vpos = _build(h, [_lattice_points()])
    assert len(vpos) == 64 * 48                      # every point became a vertex
    yield h, vpos
    h.close()


def _lattice_image(h, seed, **over):
    rng = np.random.default_rng(seed)
    px = rng.integers(0, 256, (48, 64, 3)).astype(np.uint8)
    px[:, :20] = 255                                 # white: 4 x R8(63.75) saturates
    px[:, 20:40] = 0                                 # black: update_rgb rejects
    px[:8, 40:] = 2                                  # 0.25 * 2 = 0.5 -> 0
    px[8:16, 40:] = 6                                # 0.25 * 6 = 1.5 -> 2
    px[16:24, 40:] = rng.integers(0, 128, (8, 24, 3)) * 2 + 1   # odd values
    args = dict(fx=32.0, fy=32.0, cx=32.0, cy=24.0, rot=BASE, pos=[0.0, 0.0, 0.0], obs_time=0.1 * seed, inv_exposure=EXPOSURES[seed % 8])
    args.update(over)
    return h.default_image(px, **args), px


def _stream(h, vpos, model, check):
    """eight frames from moving poses with varying exposure, every vertex, no selection -> the bytes of every fetch and the statistics"""
    ref = cck.fresh_state(len(vpos))
    cand = np.arange(len(vpos))
    out = []
    for k in range(8):
        im, px = _image(h, k)
        if check:
            if model == cck.PLAIN and k >= 6:
                # the distance gate fires: vertices that hold six observations are offered again, in view, farther than allow behind the nearest
                cam = cck.Cam(im)
                d, _, _, _, ok = cck.project(cam, vpos)
                dot = cck.dot3(d, cam.n)
                assert (ok & (ref["n_obs"] > 5) & (dot - dot.min() > cam.allow)).sum() > 100
            got, want = _step(h, ref, vpos, im, px, model, capi.COLOUR_SET_ALL, cand)
            if model == cck.VIEW:
                ang, ok = want["view_angle"], want["view_ok"]
                assert np.abs(ang[ok] - 30.0).min() > 1e-6
        else:
            got = h.colour_image(im, model, capi.COLOUR_SET_ALL)
        rgb, st = h.colour_fetch(n=len(vpos))
        out.append((rgb.tobytes(), st.tobytes(), tuple(sorted(got.items())), h.colour_selected()[1].tobytes()))
    return out, ref


def test_plain_stream(lib):
    """eight images (the n_obs > 5 gate of the distance test needs more than six observations): states and statistics bit-equal after every image"""
    h = make_hip(lib, _cfg())
    try:
        scans = _scans()
        vpos = _build(h, scans)
        cam = cck.Cam(_image(h, 0)[0])
        d, u, v, front, ok = cck.project(cam, vpos)
        pcz = cck.dot3(d, cam.n)
        assert (pcz < -1.0).any() and (front & ~ok).any() and ok.any()                    # behind the camera, outside the margin band, inside
        assert ((pcz > 0.00099) & ~front).any() and ((pcz < 0.00101) & front).any()       # pc.z just either side of 0.001
        _, ref = _stream(h, vpos, cck.PLAIN, True)
        assert ref["n_obs"].max() == 6 and (ref["n_obs"] == 0).any()                      # (the gate stops a vertex at six: dmin lies behind the camera)
    finally:
        h.close()


def test_plain_distance_gate_scales_with_the_mesh_voxel(lib):
    """allow = max(0.05, 0.1 mesh_voxel): with 0.8 m voxels it is 0.08.  A wall with 2 cm of noise seen head-on, coloured by an id list of its own
    vertices (so dmin is the wall's nearest vertex): by image 7 some vertices with six observations lie between 0.05 and 0.08 behind it (still
    updated) and some beyond 0.08 (skipped)"""
    h = make_hip(lib, _cfg(mesh_voxel=0.8, mesh_min_spacing=0.2))
    try:
        rng = np.random.default_rng(31)
        vpos = _build(h, [_plane(rng, 4000, x=6.0, y=(-3.0, 3.0), z=(-2.0, 2.0), noise=0.02), _plane(rng, 500, x=-4.0, y=(-1.0, 1.0), z=(-1.0, 1.0))])
        ids = np.flatnonzero(vpos[:, 0] > 5.0)
        assert 300 < len(ids) < len(vpos)
        ref = cck.fresh_state(len(vpos))
        seen = dict(between=0, beyond=0)
        for k in range(8):
            im, px = _image(h, k, rot=BASE, pos=[0.999, 0.02 * k, 0.01 * k])
            cam = cck.Cam(im, 0.8)
            assert cam.allow == 0.1 * 0.8
            d, _, _, _, ok = cck.project(cam, vpos[ids])
            gap = cck.dot3(d, cam.n)
            gap = gap - gap.min()
            full = ok & (ref["n_obs"][ids] > 5)
            seen["between"] += int((full & (gap > 0.05) & (gap <= cam.allow)).sum())
            seen["beyond"] += int((full & (gap > cam.allow)).sum())
            _step(h, ref, vpos, im, px, cck.PLAIN, capi.COLOUR_SET_IDS, ids, voxel=0.8)
        assert seen["between"] > 0 and seen["beyond"] > 0, seen
        assert ref["n_obs"][ids].max() > 6 and (ref["n_obs"][ids] == 6).any()
    finally:
        h.close()


def test_half_pixel_lattice(lattice):
    """vertices exactly on (k + 0.5, j + 0.5): the four taps weigh 0.25 each; the 8-bit rounding and saturation of every tap is reproduced"""
    h, vpos = lattice
    ref = h.colour_fetch(n=len(vpos))[1].copy()
    for seed in (1, 2):
        im, px = _lattice_image(h, seed)
        _, u, v, _, ok = cck.project(cck.Cam(im), vpos)
        assert np.all(u - np.floor(u) == 0.5) and np.all(v - np.floor(v) == 0.5)
        assert ok.sum() == 62 * 46                                                        # k = 0, 63 and j = 0, 47 lie in the margin band
        c = cck.sample(px, u[ok], v[ok])
        assert (c == 255).all(axis=1).any() and (c == 0).all(axis=1).any() and (c == 8).all(axis=1).any()
        got, _ = _step(h, ref, vpos, im, px, cck.PLAIN, capi.COLOUR_SET_ALL, np.arange(len(vpos)))
        assert got["n_hit"] == 62 * 46


def test_selection(world, lattice):
    """selection_points_for_projection: ids and raw (u, v) equal the loop's, for three cell sizes, from every vertex and from the voxel heads"""
    h, vpos, scans = world
    ref = h.colour_fetch(n=len(vpos))[1].copy()
    heads = cck.recent_set(vpos, scans[-1][:, :3], 0.4, heads=True)
    assert 10 < len(heads) < len(vpos)
    k = 3
    for md in (1.0, 4.0, 0.5):
        for cset, cand in ((capi.COLOUR_SET_ALL, np.arange(len(vpos))), (capi.COLOUR_SET_RECENT_HEADS, heads)):
            im, px = _image(h, k, big=True, obs_time=0.1 * k)
            got, _ = _step(h, ref, vpos, im, px, cck.PLAIN, cset, cand, md=md)
            assert 0 < got["n_selected"] < got["n_set"] and got["n_selected"] == len(h.colour_selected()[0])
            k += 1
    # crafted: on the lattice, the vertices at (31.5 | 32.5, 23.5 | 24.5) and their like are mirror images about the optical axis -- equal depths in one
    # 4-pixel cell; moving the camera by 2^-30 m makes them differ in double and agree in float, so (double)stored > depth decides
    hl, vl = lattice
    refl = hl.colour_fetch(n=len(vl))[1].copy()
    for n, (pos, md) in enumerate((([0.0, 0.0, 0.0], 4.0), ([0.0, 2.0 ** -30, 2.0 ** -31], 4.0), ([0.0, 2.0 ** -30, 0.0], 1.0), ([0.0, 0.0, 0.0], 0.5))):
        im, px = _lattice_image(hl, 3 + n, pos=pos)
        cam = cck.Cam(im)
        d, u, v, _, ok = cck.project(cam, vl)
        depth = cck.norm3(d)[ok]
        cells = np.stack([np.trunc(cck.std_round(u[ok] / md) * md), np.trunc(cck.std_round(v[ok] / md) * md), depth.astype(np.float32)], axis=1)
        _, counts = np.unique(cells, axis=0, return_counts=True)
        if md == 4.0:
            assert (counts > 1).any()                                                     # several vertices of one cell round to the same float depth
        got, _ = _step(hl, refl, vl, im, px, cck.PLAIN, capi.COLOUR_SET_ALL, np.arange(len(vl)), md=md)
        assert got["n_selected"] == len(hl.colour_selected()[0])


def test_recent_sets(lib):
    """RECENT = every vertex of the mesh voxels the last scan visited, RECENT_HEADS = the first vertex of each: keys round(coord / mesh_voxel) of the
    scan the test fed (below the append budget: every point is a candidate), applied to the exported raw positions"""
    h = make_hip(lib, _cfg())
    try:
        rng = np.random.default_rng(21)
        a = _plane(rng, 3000, x=6.0, y=(-3.0, 0.0), z=(-1.5, 1.5))
        b = _plane(rng, 3000, x=6.0, y=(-1.0, 2.0), z=(-1.5, 1.5))
        assert len(a) < h.cfg.mesh_append_budget and len(b) < h.cfg.mesh_append_budget
        im, px = _image(h, 2, big=True)
        assert h.colour_image(im, cck.PLAIN, capi.COLOUR_SET_RECENT)["n_set"] == 0        # nothing meshed yet: an empty set
        vpos = _build(h, [a, b])
        ref = h.colour_fetch(n=len(vpos))[1].copy()
        assert ref.tobytes() == cck.fresh_state(len(vpos)).tobytes()
        for k, (cset, is_heads) in enumerate(((capi.COLOUR_SET_RECENT, False), (capi.COLOUR_SET_RECENT_HEADS, True), (capi.COLOUR_SET_RECENT, False))):
            cand = cck.recent_set(vpos, b[:, :3], 0.4, heads=is_heads)
            assert 0 < len(cand) < len(vpos)
            before = ref.copy()
            im, px = _image(h, 2 + k, big=True)
            got, _ = _step(h, ref, vpos, im, px, cck.PLAIN, cset, cand)
            st_d = h.colour_fetch(n=len(vpos))[1]
            changed_d = np.flatnonzero([x.tobytes() != y.tobytes() for x, y in zip(st_d, before)])
            changed_c = np.flatnonzero([x.tobytes() != y.tobytes() for x, y in zip(ref, before)])
            assert np.array_equal(changed_d, changed_c) and len(changed_d) > 0 and np.isin(changed_d, cand).all()
        # selection from the heads, as selection_points_for_projection starts
        cand = cck.recent_set(vpos, b[:, :3], 0.4, heads=True)
        im, px = _image(h, 6, big=True)
        _step(h, ref, vpos, im, px, cck.PLAIN, capi.COLOUR_SET_RECENT_HEADS, cand, md=2.0)
    finally:
        h.close()


def test_view_model(world):
    """thread_render_pts_in_voxel: integers exact, doubles to 1e-12 relative; no vertex sits on the 30 degree gate or the 5 degree clamp"""
    h, vpos, _ = world
    ref = h.colour_fetch(n=len(vpos))[1].copy()
    cand = np.arange(len(vpos))
    total = dict(n_updated=0, pe_count=0, n_hit=0)
    for k in (0, 2, 3, 5, 6, 7):
        im, px = _image(h, k, obs_time=10.0 + 0.1 * k)
        cam = cck.Cam(im)
        d = cck.project(cam, vpos)[0]
        ang = np.arccos(cck.dot3(d, cam.n) / (cck.norm3(d) + 0.0001)) * 57.3
        assert np.abs(ang - 30.0).min() > 1e-6 and np.abs(ang - 5.0).min() > 1e-6         # every vertex, on the checker's own values
        got, want = _step(h, ref, vpos, im, px, cck.VIEW, capi.COLOUR_SET_ALL, cand)
        assert (want["view_angle"] > 30.0).any() and (want["view_angle"] == 5.0).any()    # both the gate and the clamp are taken
        for key in total:
            total[key] += got[key]
    assert total["n_updated"] > 0 and total["pe_count"] > 0 and total["n_hit"] > total["n_updated"]
    # an id list (every third vertex), with selection
    ids = np.arange(0, len(vpos), 3)
    im, px = _image(h, 4, obs_time=11.0)
    _step(h, ref, vpos, im, px, cck.VIEW, capi.COLOUR_SET_IDS, ids, md=2.0)


def test_deterministic(lib):
    """the same stream twice gives identical bytes: states, colours, statistics (pe_sum is summed in a fixed order), the raw (u, v)"""
    runs = []
    for _ in range(2):
        h = make_hip(lib, _cfg())
        try:
            vpos = _build(h, _scans())
            runs.append(_stream(h, vpos, cck.PLAIN, False)[0] + _stream(h, vpos, cck.VIEW, False)[0])
        finally:
            h.close()
    assert runs[0] == runs[1]
    assert any(dict(r[2])["pe_sum"] > 0 for r in runs[0])


def test_no_side_effects(lib):
    """the map's export and the mesher's result sizes are the same before and after colouring; vertices a later scan appends start from the zero state"""
    h = make_hip(lib, _cfg())
    try:
        scans = _scans()
        vpos = _build(h, scans[:2])
        before, lists = h.mesh_export(1.0, 20), h.mesh_fetch()
        h.colourer()
        for k in (2, 5):
            im, _ = _image(h, k)
            assert h.colour_image(im, cck.PLAIN, capi.COLOUR_SET_ALL)["n_hit"] > 0
        after, lists2 = h.mesh_export(1.0, 20), h.mesh_fetch()
        assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes()
        for key in lists:
            assert np.asarray(lists[key]).tobytes() == np.asarray(lists2[key]).tobytes(), key
        coloured = h.colour_fetch(n=len(vpos))[1]
        h.mesh_scan(np.ascontiguousarray(scans[2]), np.zeros(3), frame_idx=2, fetch=False)
        n_new = h.counters()["n_vertices"]
        assert n_new > len(vpos)
        st = h.colour_fetch()[1]
        assert len(st) == n_new and st[:len(vpos)].tobytes() == coloured.tobytes()
        assert st[len(vpos):].tobytes() == cck.fresh_state(n_new - len(vpos)).tobytes()
    finally:
        h.close()


def _read_ply(path):
    raw = open(path, "rb").read()
    head, body = raw[:raw.index(b"end_header\n") + 11], raw[raw.index(b"end_header\n") + 11:]
    lines = head.decode().split("\n")
    nv = int([ln for ln in lines if ln.startswith("element vertex")][0].split()[-1])
    nf = int([ln for ln in lines if ln.startswith("element face")][0].split()[-1])
    has_rgb = "property uchar red" in lines
    if has_rgb:
        assert lines[lines.index("property uchar red"):lines.index("property uchar red") + 3] == ["property uchar red", "property uchar green", "property uchar blue"]
    vdt = np.dtype([("xyz", "<f4", 3)] + ([("rgb", "u1", 3)] if has_rgb else []))
    v = np.frombuffer(body[:nv * vdt.itemsize], vdt)
    f = np.frombuffer(body[nv * vdt.itemsize:], np.dtype([("n", "u1"), ("idx", "<i4", 3)]))
    assert len(f) == nf and np.all(f["n"] == 3)
    return v, f["idx"]


def test_coloured_ply(world, tmp_path):
    h, vpos, _ = world
    im, _ = _image(h, 3, obs_time=20.0)
    h.colour_image(im, cck.PLAIN, capi.COLOUR_SET_ALL)
    rgb, st = h.colour_fetch(n=len(vpos))
    assert (st["n_obs"] == 0).any() and (st["n_obs"] >= 2).any() and rgb.any()
    plain, bgr, rgb_path = str(tmp_path / "a.ply"), str(tmp_path / "b.ply"), str(tmp_path / "c.ply")
    h.save_ply(plain, 1.0, 20)
    h.save_ply_rgb(bgr, 1.0, 20, min_views=2, bgr=True)
    h.save_ply_rgb(rgb_path, 1.0, 20, min_views=0, bgr=False)
    v0, f0 = _read_ply(plain)
    for path, min_views, flip in ((bgr, 2, True), (rgb_path, 0, False)):
        v, f = _read_ply(path)
        assert v["xyz"].tobytes() == v0["xyz"].tobytes() and f.tobytes() == f0.tobytes() and len(v) == len(vpos)
        want = np.where((st["n_obs"] >= min_views)[:, None], rgb[:, ::-1] if flip else rgb, 0)
        assert np.array_equal(v["rgb"], want)


def test_argument_errors(world, lib):
    h, vpos, _ = world
    nv = len(vpos)
    good, _ = _image(h, 3)
    h.colour_image(good, cck.PLAIN, capi.COLOUR_SET_ALL)
    before = h.colour_fetch(n=nv)[1].tobytes()
    sel_before = h.colour_selected()[0].tobytes()

    def bad(match, im=None, model=cck.PLAIN, cset=capi.COLOUR_SET_ALL, ids=None, md=0.0):
        with pytest.raises(RuntimeError, match=r"rc=-1: .*" + match):
            h.colour_image(good if im is None else im, model, cset, ids=ids, select_min_dis=md)
        assert h.colour_fetch(n=nv)[1].tobytes() == before and h.colour_selected()[0].tobytes() == sel_before

    bad("ascending", cset=capi.COLOUR_SET_IDS, ids=[5, 3])
    bad("ascending", cset=capi.COLOUR_SET_IDS, ids=[5, 5])
    bad("out of range", cset=capi.COLOUR_SET_IDS, ids=[0, nv])
    bad("out of range", cset=capi.COLOUR_SET_IDS, ids=[-1, 2])
    bad("position", im=_image(h, 3, pos=[np.nan, 0.0, 0.0])[0])
    bad("rotation", im=_image(h, 3, rot=np.full((3, 3), np.inf))[0])
    bad("intrinsics", im=_image(h, 3, fx=float("nan"))[0])
    bad("rows", im=h.default_image(np.zeros((1, 64, 3), np.uint8), fx=40.0, fy=40.0, cx=32.0, cy=0.5))
    bad("cols", im=_image(h, 3, cols=8193)[0])
    bad("stride", im=_image(h, 3, row_stride_bytes=3 * 64 - 1)[0])
    bad("data", im=_image(h, 3, data=None)[0])
    bad("model", model=7)
    bad("set", cset=9)
    bad("select_min_dis", md=float("nan"))
    bad("select_min_dis", md=1e-300)
    bad("select_min_dis", md=2000.0)
    bad("inv_exposure", im=_image(h, 3, inv_exposure=0.0)[0])
    sh = make_hip(lib, _cfg(shard_world=2, shard_rank=0, shard_mesh=1))
    try:
        with pytest.raises(RuntimeError, match="rc=-1: .*shard"):
            sh.colour_image(_image(sh, 3)[0], cck.PLAIN, capi.COLOUR_SET_ALL)
    finally:
        sh.close()
