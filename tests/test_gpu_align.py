"""Align a cloud to the mesh on the device (include/immesh_align.h) against the numpy restatement of the contract (tests/align_checker.py): the
per-point terms and faces bit for bit at the wavefront and workgroup edges, the folded system within the contract's bound, the rule's corners, the
three kernel shapes, determinism, the loop as the public pieces, convergence on a bumpy sheet, the statuses, the live mesh, argument errors."""
import ctypes as C
import math

import numpy as np
import pytest

import align_checker as ac
import closest_checker as cc
from immesh_amd import capi, synth
from conftest import make_hip
from test_gpu_closest import _local, _points
from test_gpu_render import _lattice, _rand_rot, _small_cfg, _soup

pytestmark = pytest.mark.gpu
SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 65537]
N_MAX = max(SIZES)
MAX_DIST = 0.5
CENTRE = np.array([1.5, -2.25, 0.75])
EPS = 2.0 ** -52


@pytest.fixture(scope="module")
def hp():
    h = make_hip(capi.load_hip_library(), _small_cfg())
    yield h
    h.close()


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _frame_arrays(fr):
    return np.array(list(fr.rot)).reshape(3, 3), np.array(list(fr.pos))


@pytest.fixture(scope="module")
def soup():
    """200 random faces (the awkward ones of test_gpu_render._soup among them), 65 537 points of which every smaller size is a prefix, and the
    checker's correspondences in the world and under a frame, made once: they depend on neither the mode nor the centre"""
    rng = np.random.default_rng(2026)
    vtx, faces = _soup(rng, 200)
    world = _points(rng, vtx, faces, N_MAX, near=0.3)
    world[5] = [np.nan, 0.0, 0.0]; world[7] = [0.0, np.inf, 0.0]; world[9] = [1e6, -1e6, 1e6]; world[70] = [0.0, 0.0, -np.inf]
    rot, pos = _rand_rot(rng), rng.uniform(-2, 2, 3)
    local = _local(world, rot, pos)
    out = {"vtx": vtx, "faces": faces, "cases": {}}
    for name, (r, p, pts) in {"world": (None, None, world), "frame": (rot, pos, local)}.items():
        out["cases"][name] = (r, p, pts, ac.correspondences(r, p, pts, MAX_DIST, vtx, faces))
    return out


def _reference(corr, n, mode, centre):
    p, ok, face, q, A = (x[:n] for x in corr)
    tm, used, flat = ac.terms(mode, p, centre, face, q, A)
    sums, bound, counts = ac.system(tm, ok, face, used, flat)
    return face, tm, sums, bound, counts


def _check_step(hp, pts, opts, frame, ref, what):
    face, tm, sums, bound, counts = ref
    n = len(pts)
    sy, gface, gterms = hp.align_step(pts, opts, frame, want_face=True, want_terms=True)
    assert gface.dtype == np.int32 and np.array_equal(gface, face), (what, np.nonzero(gface != face)[0][:5])
    rows = np.nonzero((gterms.view(np.uint64) != tm.view(np.uint64)).any(axis=1))[0] if n else []
    assert len(rows) == 0, (what, len(rows), rows[:3], gterms[rows[:1]], tm[rows[:1]])
    assert sy.counts() == counts and sum(counts) == n, (what, sy.counts(), counts)
    got = sy.sums()
    fs = np.array([math.fsum(gterms[:, k].tolist()) for k in range(28)])
    assert (np.abs(got - sums) <= n * EPS * bound).all(), (what, np.abs(got - sums) / np.maximum(bound, 1e-300))
    assert (np.abs(got - fs) <= n * EPS * bound).all(), what
    sy2, f2, t2 = hp.align_step(pts, opts, frame)                                        # nothing stored per point: the same bits
    assert f2 is None and t2 is None and bytes(sy2) == bytes(sy), what
    return sy


# ---- per-point terms and faces, the folded system ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_pts", SIZES)
def test_terms_faces_and_system_match_checker(hp, soup, n_pts):
    hp.raycast_build_triangles(soup["vtx"], soup["faces"])
    hp.align_set_variant(0)
    used = 0
    for name, (rot, pos, pts, corr) in soup["cases"].items():
        frame = None if rot is None else capi.ray_frame(rot, pos)
        for mode in (capi.ALIGN_POINT, capi.ALIGN_PLANE):
            for centre in (np.zeros(3), CENTRE):
                ref = _reference(corr, n_pts, mode, centre)
                sy = _check_step(hp, pts[:n_pts], capi.align_options(mode=mode, max_dist=MAX_DIST, centre=centre), frame, ref, (name, mode, n_pts))
                used += sy.n_used
    if n_pts >= 63:
        assert used > 0
    if n_pts == N_MAX:                                                                   # the checker first: every count occurs, the flat winners too
        _, _, _, _, counts = _reference(soup["cases"]["world"][3], n_pts, capi.ALIGN_PLANE, CENTRE)
        assert min(counts) > 0 and counts[1] == 4, counts


@pytest.mark.parametrize("n_pts", [1, 65, 257, 65537])
def test_the_three_kernel_shapes_give_the_same_bits(hp, soup, n_pts):
    hp.raycast_build_triangles(soup["vtx"], soup["faces"])
    rot, pos, pts, _ = soup["cases"]["frame"]
    try:
        for mode in (capi.ALIGN_POINT, capi.ALIGN_PLANE):
            opts = capi.align_options(mode=mode, max_dist=MAX_DIST, centre=CENTRE)
            got = []
            for variant in (0, 1, 2):
                hp.align_set_variant(variant)
                sy, face, terms = hp.align_step(pts[:n_pts], opts, capi.ray_frame(rot, pos), want_face=True, want_terms=True)
                got.append(bytes(sy) + _bits(face) + _bits(terms) + bytes(hp.align_step(pts[:n_pts], opts, capi.ray_frame(rot, pos))[0]))
            assert got[0] == got[1] == got[2], (mode, n_pts)
    finally:
        hp.align_set_variant(0)


# ---- the rule's corners ---------------------------------------------------------------------------------------------------------------------------------
ONE_VTX = np.array([[-4, -4, -2], [4, -4, -2], [0, 6, -2]], np.float32)
ONE_FACE = np.array([[0, 1, 2]], np.int32)


def test_points_that_are_not_finite(hp):
    hp.raycast_build_triangles(ONE_VTX, ONE_FACE)
    pts = np.array([[0, 0, 0], [np.nan, 0, 0], [0, -np.inf, 0], [3e38, 0, 0], [0.5, 0.5, -1]], np.float32)
    opts = capi.align_options(max_dist=10.0)
    sy, face, terms = hp.align_step(pts, opts, None, True, True)
    assert sy.counts() == (2, 2, 1, 0) and face.tolist() == [0, -1, -1, -1, 0]         # 3e38 is a finite float below 2^128: merely far away
    double = capi.ray_frame(rot=2.0 * np.eye(3))                                        # the frame pushes it past 2^128
    ref = ac.step(2.0 * np.eye(3), np.zeros(3), pts, ac.POINT, 10.0, np.zeros(3), ONE_VTX, ONE_FACE)
    sy, face, terms = hp.align_step(pts, opts, double, True, True)
    assert sy.counts() == ref["counts"] == (2, 3, 0, 0) and np.array_equal(face, ref["face"]) and _bits(terms) == _bits(ref["terms"])
    assert not terms[1:4].any()


def test_the_max_dist_boundary(hp):
    hp.raycast_build_triangles(ONE_VTX, ONE_FACE)
    pts = np.array([[0, 0, 0], [0, 0, -5], [0, 0, 0.5]], np.float32)                     # D = 4, 9, 6.25
    for max_dist, want in ((2.0, (1, 0, 2, 0)), (np.nextafter(2.0, 0.0), (0, 0, 3, 0)), (3.0, (3, 0, 0, 0)), (2.5, (2, 0, 1, 0))):
        sy, face, _ = hp.align_step(pts, capi.align_options(max_dist=max_dist), None, True)
        assert sy.counts() == want and (face >= 0).sum() == want[0], (max_dist, sy.counts())   # D == r2 counts as matched
        assert sy.counts() == ac.step(None, None, pts, ac.POINT, max_dist, np.zeros(3), ONE_VTX, ONE_FACE)["counts"]


def test_a_zero_area_winner(hp):
    vtx = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [0, 0, 0]], np.float32)             # collinear; and a == b == c
    for faces in (np.array([[0, 1, 2]], np.int32), np.array([[3, 3, 3]], np.int32), np.array([[0, 1, 1]], np.int32)):
        hp.raycast_build_triangles(vtx, faces)
        pts = np.array([[0.5, 0.25, 0.0], [3.0, 0.0, 1.0]], np.float32)
        for mode, want in ((capi.ALIGN_PLANE, (0, 0, 0, 2)), (capi.ALIGN_POINT, (2, 0, 0, 0))):
            ref = ac.step(None, None, pts, mode, 5.0, CENTRE, vtx, faces)
            sy, face, terms = hp.align_step(pts, capi.align_options(mode=mode, max_dist=5.0, centre=CENTRE), None, True, True)
            assert sy.counts() == ref["counts"] == want and face.tolist() == [0, 0] and _bits(terms) == _bits(ref["terms"])
            assert terms.any() == (mode == capi.ALIGN_POINT)
            assert (np.abs(sy.sums() - ref["sums"]) <= 2 * EPS * ref["bound"]).all()


def test_ties_on_a_lattice_go_to_the_lower_face(hp):
    vtx, faces = _lattice(12, 10, 4.0, 256.0, 0, 0)
    hp.raycast_build_triangles(vtx, faces)
    pts = np.concatenate([vtx, vtx + np.float32([0, 0, 0.25])]).astype(np.float32)
    allD = cc.all_D(None, None, pts[:len(vtx)], vtx, faces)
    assert ((allD == allD.min(axis=1, keepdims=True)).sum(axis=1) >= 2).sum() > 100      # the checker first: most vertices tie between faces
    for mode in (capi.ALIGN_POINT, capi.ALIGN_PLANE):
        ref = ac.step(None, None, pts, mode, 1.0, CENTRE, vtx, faces)
        assert np.array_equal(ref["face"][:len(vtx)], np.argmin(allD, axis=1))             # argmin: the first, the lower index
        sy, face, terms = hp.align_step(pts, capi.align_options(mode=mode, max_dist=1.0, centre=CENTRE), None, True, True)
        assert np.array_equal(face, ref["face"]) and _bits(terms) == _bits(ref["terms"]) and sy.counts() == ref["counts"]


def test_no_face_in_the_hierarchy_and_a_single_face(hp):
    pts = _points(np.random.default_rng(3), ONE_VTX, ONE_FACE, 300, near=0.5)
    nan_vtx = ONE_VTX.copy(); nan_vtx[1, 0] = np.nan
    for vtx, faces in ((np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)), (nan_vtx, ONE_FACE)):
        assert hp.raycast_build_triangles(vtx, faces)[2] == 0
        for mode in (capi.ALIGN_POINT, capi.ALIGN_PLANE):
            sy, face, terms = hp.align_step(pts, capi.align_options(mode=mode, max_dist=10.0), None, True, True)
            assert sy.counts() == (0, 1, 299, 0) and (face == -1).all() and not terms.any() and not sy.sums().any()
            res, hist = hp.align(pts, capi.align_options(mode=mode, max_dist=10.0))
            assert (res.status, res.iterations, len(hist)) == (capi.ALIGN_TOO_FEW, 1, 1) and bytes(res.frame) == bytes(capi.ray_frame())
    assert hp.raycast_build_triangles(ONE_VTX, ONE_FACE)[2] == 1                          # the single-leaf tree: the face is met twice
    for mode in (capi.ALIGN_POINT, capi.ALIGN_PLANE):
        ref = ac.step(None, None, pts, mode, 10.0, CENTRE, ONE_VTX, ONE_FACE)
        _check_step(hp, pts, capi.align_options(mode=mode, max_dist=10.0, centre=CENTRE), None,
                    (ref["face"], ref["terms"], ref["sums"], ref["bound"], ref["counts"]), ("single", mode))
        assert ref["counts"][0] == 298


# ---- determinism ---------------------------------------------------------------------------------------------------------------------------------------
def test_deterministic_and_independent_of_the_face_order(hp):
    rng = np.random.default_rng(12)
    vtx, faces = _soup(rng, 49)                                                           # below 50 faces: no duplicate face, so no tie between faces
    pts = _points(rng, vtx, faces, 5000, near=0.3)
    b = make_hip(capi.load_hip_library(), _small_cfg())
    try:
        hp.raycast_build_triangles(vtx, faces)
        b.raycast_build_triangles(vtx, faces[::-1])
        for mode in (capi.ALIGN_POINT, capi.ALIGN_PLANE):
            opts = capi.align_options(mode=mode, max_dist=1.0, centre=CENTRE, max_iters=4)
            one = hp.align_step(pts, opts, None, True, True)
            two = hp.align_step(pts, opts, None, True, True)
            assert bytes(one[0]) == bytes(two[0]) and _bits(one[1]) == _bits(two[1]) and _bits(one[2]) == _bits(two[2])
            assert one[0].n_used > 1000
            r1, h1 = hp.align(pts, opts)
            r2, h2 = hp.align(pts, opts)
            assert bytes(r1) == bytes(r2) and _bits(h1) == _bits(h2) and 1 <= r1.iterations == len(h1) <= 4
            rev = b.align_step(pts, opts, None, True, True)
            assert np.array_equal(np.where(rev[1] >= 0, len(faces) - 1 - rev[1], -1), one[1]) and _bits(rev[2]) == _bits(one[2])
            assert bytes(rev[0]) == bytes(one[0])                                         # the same terms in the same order: the same sums
            rb, hb = b.align(pts, opts)
            assert bytes(rb) == bytes(r1) and _bits(hb) == _bits(h1)
    finally:
        b.close()


# ---- the loop is the public pieces -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sheet():
    vtx, faces, cloud = ac.convergence_case()
    assert len(faces) == 1058 and cloud.shape == (4000, 3) and cloud.dtype == np.float32
    return vtx, faces, cloud, np.array(capi.align_centre_mean(cloud))


def _by_hand(hp, pts, opts, frame):
    """the Loop rule through align_step, align_solve and align_update -> (frame, status, iterations, history)"""
    need = 6 if opts.mode == capi.ALIGN_PLANE else 3
    centre = list(opts.centre)
    status, hist = capi.ALIGN_MAX_ITERS, []
    for it in range(opts.max_iters):
        sy, _, _ = hp.align_step(pts, opts, frame)
        rows = sy.n_used if opts.mode == capi.ALIGN_PLANE else 3 * sy.n_used
        rms = math.sqrt(sy.e / rows) if rows > 0 else 0.0
        nw = nv = 0.0
        stop = False
        if sy.n_used < need:
            status, stop = capi.ALIGN_TOO_FEW, True
        else:
            bad, delta = hp.align_solve(sy, opts.damping)
            if bad:
                status, stop = capi.ALIGN_DEGENERATE, True
            else:
                frame = hp.align_update(frame, centre, delta)
                d = delta.tolist()
                nw, nv = math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]), math.sqrt((d[3] * d[3] + d[4] * d[4]) + d[5] * d[5])
                if nw <= opts.eps_rot and nv <= opts.eps_trans:
                    status, stop = capi.ALIGN_CONVERGED, True
        hist.append([float(sy.n_used), rms, nw, nv])
        if stop:
            break
    return frame, status, it + 1, np.array(hist), sy


@pytest.mark.parametrize("mode", [capi.ALIGN_POINT, capi.ALIGN_PLANE])
def test_the_loop_equals_stepping_by_hand(hp, sheet, mode):
    vtx, faces, cloud, centre = sheet
    hp.raycast_build_triangles(vtx, faces)
    rng = np.random.default_rng(21)
    for frame0, eps, iters in ((capi.ray_frame(), 1e-10, 8), (capi.ray_frame(ac.rodrigues(rng.normal(size=3), 0.01), [0.01, 0.0, -0.02]), 1e-3, 8)):
        opts = capi.align_options(mode=mode, max_dist=0.5, centre=centre, max_iters=iters, eps_rot=eps, eps_trans=eps)
        frame, status, iterations, hist, sy = _by_hand(hp, cloud, opts, frame0)
        res, history = hp.align(cloud, opts, frame0)
        assert (res.status, res.iterations) == (status, iterations) and bytes(res.frame) == bytes(frame)
        assert _bits(history) == _bits(hist) and bytes(res.system) == bytes(sy) and res.rms == hist[-1, 1]
        if mode == capi.ALIGN_PLANE:
            assert status == capi.ALIGN_CONVERGED and iterations < iters
    res_none, _ = hp.align(cloud, opts)                                                    # no frame: the identity
    res_id, _ = hp.align(cloud, opts, capi.ray_frame())
    assert bytes(res_none) == bytes(res_id)
    _, h3 = hp.align(cloud, opts, history_cap=2)
    assert len(h3) == 2 and _bits(h3) == _bits(hp.align(cloud, opts)[1][:2])


# ---- convergence -----------------------------------------------------------------------------------------------------------------------------------------
# The tolerance of the final pose is measured, not chosen: the checker's loop was run on the CPU on this case (PLANE rows, max_dist 0.5, centre = the
# cloud's mean, 30 iterations, both eps 1e-10) once adding the terms one after the other in ascending point order and once in descending order
# (align_checker.loop(..., summation="ascending" / "descending")); both converge in 5 iterations and the largest difference of the two final poses
# is 1.11e-16 over the rotation's entries and 2.498001805406602e-16 over the position's.  100 times the larger figure:
POSE_TOL = 100 * 2.498001805406602e-16


def test_convergence_on_the_bumpy_sheet(hp, sheet):
    vtx, faces, cloud, centre = sheet
    hp.raycast_build_triangles(vtx, faces)
    ref = ac.loop(None, None, cloud, ac.PLANE, 0.5, centre, 0.0, 30, 1e-10, 1e-10, vtx, faces)
    res, hist = hp.align(cloud, centre="mean", mode=capi.ALIGN_PLANE, max_dist=0.5, max_iters=30, eps_rot=1e-10, eps_trans=1e-10)
    rot, pos = _frame_arrays(res.frame)
    print("iterations %d, rms %s, |pose - checker| rot %.3g pos %.3g" % (res.iterations, hist[:, 1].tolist(), np.abs(rot - ref["rot"]).max(),
                                                                        np.abs(pos - ref["pos"]).max()))
    assert res.status == capi.ALIGN_CONVERGED == ref["status"] and res.iterations == ref["iterations"]
    assert (np.diff(hist[1:, 1]) <= 0).all(), hist[:, 1]                                   # the rms does not rise after the second iteration
    assert np.abs(rot - ref["rot"]).max() <= POSE_TOL and np.abs(pos - ref["pos"]).max() <= POSE_TOL
    assert np.abs(pos - ac.TRUE_POS).max() <= 1e-4 and np.abs(rot - ac.TRUE_ROT).max() <= 1e-4
    # POINT rows slide along the sheet: the rms falls and 30 iterations are not enough
    res, hist = hp.align(cloud, centre="mean", mode=capi.ALIGN_POINT, max_dist=0.5, max_iters=30, eps_rot=1e-10, eps_trans=1e-10)
    assert (res.status, res.iterations) == (capi.ALIGN_MAX_ITERS, 30) and (np.diff(hist[:, 1]) < 0).all()


def test_a_single_plane_is_degenerate_until_damped(hp):
    rng = np.random.default_rng(5)
    vtx = np.array([[-10, -10, 0], [10, -10, 0], [0, 10, 0]], np.float32)
    hp.raycast_build_triangles(vtx, ONE_FACE)
    xy = rng.uniform(-3, 3, (50, 2))
    pts = np.concatenate([xy, 0.1 + 0.02 * xy[:, :1]], axis=1).astype(np.float32)         # a tilted plane above the face
    frame0 = capi.ray_frame(ac.rodrigues([0.0, 0.0, 1.0], 0.3), [0.1, 0.2, 0.0])
    res, hist = hp.align(pts, capi.align_options(mode=capi.ALIGN_PLANE, max_dist=1.0), frame0)
    assert (res.status, res.iterations) == (capi.ALIGN_DEGENERATE, 1) and bytes(res.frame) == bytes(frame0) and res.system.n_used == 50
    assert hist.tolist() == [[50.0, res.rms, 0.0, 0.0]] and res.rms > 0
    res, hist = hp.align(pts, capi.align_options(mode=capi.ALIGN_PLANE, max_dist=1.0, damping=1e-6), frame0)
    assert res.status in (capi.ALIGN_CONVERGED, capi.ALIGN_MAX_ITERS) and np.isfinite(np.array(list(res.frame.rot) + list(res.frame.pos))).all()
    assert hist[-1, 1] < 1e-6 < hist[0, 1]                                                   # and the cloud came down onto the plane


# ---- statuses ---------------------------------------------------------------------------------------------------------------------------------------------
def test_statuses(hp, sheet):
    vtx, faces, cloud, centre = sheet
    hp.raycast_build_triangles(vtx, faces)
    for mode in (capi.ALIGN_POINT, capi.ALIGN_PLANE):
        res, hist = hp.align(np.zeros((0, 3), np.float32), capi.align_options(mode=mode))
        assert (res.status, res.iterations, res.rms, len(hist)) == (capi.ALIGN_TOO_FEW, 1, 0.0, 1) and res.system.counts() == (0, 0, 0, 0)
    frame0 = capi.ray_frame(pos=[0.0, 0.0, 0.01])
    on = (cloud[:5].astype(np.float64) @ ac.TRUE_ROT.T + ac.TRUE_POS).astype(np.float32)
    res, _ = hp.align(on, capi.align_options(mode=capi.ALIGN_PLANE, max_dist=0.5), frame0)
    assert (res.status, res.iterations, res.system.n_used) == (capi.ALIGN_TOO_FEW, 1, 5) and bytes(res.frame) == bytes(frame0)
    res, _ = hp.align(on[:2], capi.align_options(mode=capi.ALIGN_POINT, max_dist=0.5), frame0)
    assert (res.status, res.system.n_used) == (capi.ALIGN_TOO_FEW, 2)
    res, _ = hp.align(on[:3], capi.align_options(mode=capi.ALIGN_POINT, max_dist=0.5, max_iters=2, damping=1e-9), frame0)
    assert res.status in (capi.ALIGN_MAX_ITERS, capi.ALIGN_CONVERGED, capi.ALIGN_DEGENERATE) and res.system.n_used == 3    # three points suffice
    res, hist = hp.align(cloud, capi.align_options(mode=capi.ALIGN_PLANE, max_dist=0.5, centre=centre, max_iters=1, eps_rot=1e-10, eps_trans=1e-10))
    assert (res.status, res.iterations, len(hist)) == (capi.ALIGN_MAX_ITERS, 1, 1) and bytes(res.frame) != bytes(capi.ray_frame())
    one, total = hp.align_timing()
    assert one > 0 and total == one


# ---- tools/mesh_eval.py --align ---------------------------------------------------------------------------------------------------------------------------
def test_mesh_eval_moves_the_cloud_by_the_found_pose(hp, sheet):
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import mesh_eval
    vtx, faces, cloud, centre = sheet
    hp.raycast_build_triangles(vtx, faces)
    before = mesh_eval.evaluate(hp, cloud, tau=0.01, max_dist=0.5, density=50.0)
    moved, block = mesh_eval.align_cloud(hp, cloud, "plane", 0.5, 30)
    after = mesh_eval.evaluate(hp, moved, tau=0.01, max_dist=0.5, density=50.0)
    assert block["status"] == "converged" and block["iterations"] == len(block["rms"]) <= 8 and block["centre"] == list(centre)
    assert moved.dtype == np.float32 and moved.shape == cloud.shape
    truth = (cloud.astype(np.float64) @ ac.TRUE_ROT.T + ac.TRUE_POS)
    assert np.abs(moved - truth).max() < 1e-5                                              # eps 1e-9 and float storage
    assert after["accuracy"]["mean"] < 1e-5 < 0.01 < before["accuracy"]["mean"] and set(after) == set(before)   # the evaluation gains no key


# ---- the live mesh -------------------------------------------------------------------------------------------------------------------------------------------
def test_live_mesh_step_matches_checker():
    lib = capi.load_hip_library()
    cfg = capi.avia_config(cap_root_voxels=1 << 15, cap_scan_points=100000)
    a = make_hip(lib, cfg)
    try:
        extT = np.array(list(cfg.extT))
        for k in range(4):
            R, t = synth.trajectory_pose(k)
            raw = synth.livox_scan(k, R, t, n_pts=20000, extT=extT)
            if k == 0:
                a.map_build(np.ascontiguousarray(raw[:, :3]), capi.make_state(R=R, t=t))
                continue
            down = synth.voxel_grid_downsample(raw, 0.4)
            prior = capi.make_state(R=R, t=t + np.array([0.01, 0.0, -0.01]), cov_diag=1e-5)
            state, _ = a.process_scan(down, raw, prior, prior, frame_idx=k, do_mesh=True)
        nv, nf, n_in = a.raycast_build_mesh(1.0, 20)
        vtx, faces = a.mesh_export(1.0, 20)
        assert (nv, nf) == (len(vtx), len(faces)) and n_in > 0
        frame = a.ray_frame_from_state(state)
        rot, pos = _frame_arrays(frame)
        rot, pos = ac.rodrigues([0.2, 1.0, -0.4], math.radians(0.5)) @ rot, pos + [0.03, -0.02, 0.02]    # a displaced frame
        local = np.ascontiguousarray(raw[::10, :3])[:2000]
        centre = np.array(capi.align_centre_mean(local, capi.ray_frame(rot, pos)))
        for mode in (capi.ALIGN_POINT, capi.ALIGN_PLANE):
            ref = ac.step(rot, pos, local, mode, 1.0, centre, vtx, faces)
            assert ref["counts"][0] > 1000, ref["counts"]
            _check_step(a, local, capi.align_options(mode=mode, max_dist=1.0, centre=centre), capi.ray_frame(rot, pos),
                        (ref["face"], ref["terms"], ref["sums"], ref["bound"], ref["counts"]), ("live", mode))
    finally:
        a.close()


# ---- argument errors -------------------------------------------------------------------------------------------------------------------------------------------
def test_argument_errors():
    h = make_hip(capi.load_hip_library(), _small_cfg())
    try:
        pts = np.array([[0, 0, 0], [0, 0, -5]], np.float32)
        good = dict(mode=capi.ALIGN_POINT, max_dist=10.0)
        for call in (lambda: h.align_step(pts, capi.align_options(**good)), lambda: h.align(pts, capi.align_options(**good))):
            with pytest.raises(RuntimeError, match=r"rc=-1: .*no hierarchy has been built"):
                call()                                                                     # a caster that was created but never built
        h.raycast_build_triangles(ONE_VTX, ONE_FACE)
        closest = h.closest_points(pts, 10.0)

        def still_usable():
            sy, face, _ = h.align_step(pts, capi.align_options(**good), None, True)
            assert sy.counts() == (2, 0, 0, 0) and face.tolist() == [0, 0] and sy.e == 13.0
            assert h.align(pts, capi.align_options(**good))[0].status == capi.ALIGN_TOO_FEW

        still_usable()
        nan, inf = np.nan, np.inf
        cases = [(dict(max_dist=v), "max_dist", True) for v in (0.0, -1.0, inf, nan)]
        cases += [(dict(mode=v), "mode", True) for v in (-1, 2)]
        cases += [(dict(centre=v), "centre is not finite", True) for v in ((nan, 0, 0), (0, inf, 0), (0, 0, -inf))]
        cases += [(dict(damping=v), "damping", False) for v in (-1e-9, inf, nan)]
        cases += [(dict(max_iters=v), "max_iters", False) for v in (0, -1, 10001)]
        cases += [(dict(eps_rot=v), "eps_rot", False) for v in (-1.0, inf, nan)] + [(dict(eps_trans=v), "eps_trans", False) for v in (-1.0, inf, nan)]
        for over, text, step_too in cases:
            opts = capi.align_options(**{**good, **over})
            with pytest.raises(RuntimeError, match=r"rc=-1: .*align: .*" + text):
                h.align(pts, opts)
            if step_too:
                with pytest.raises(RuntimeError, match=r"rc=-1: .*align_step: .*" + text):
                    h.align_step(pts, opts)
            still_usable()
        for bad in (capi.ray_frame(pos=[nan, 0, 0]), capi.ray_frame(rot=np.diag([1.0, inf, 1.0]))):
            with pytest.raises(RuntimeError, match=r"rc=-1: .*align: .*finite"):
                h.align(pts, capi.align_options(**good), bad)
            with pytest.raises(RuntimeError, match=r"rc=-1: .*align_step: .*finite"):
                h.align_step(pts, capi.align_options(**good), bad)
            still_usable()
        opts, res, sy = capi.align_options(**good), capi.AlignResult(), capi.AlignSystem()
        f = h.lib.immesh_align
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(capi.AlignOptions), C.POINTER(capi.AlignResult), C.c_void_p, C.c_int64]
        g = h.lib.immesh_align_step
        g.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(capi.AlignOptions), C.POINTER(capi.AlignSystem), C.c_void_p, C.c_void_p]
        p = pts.ctypes.data_as(C.c_void_p)
        for n in (-1, 2 ** 31 - 1, 2 ** 40):
            assert f(h.raycaster(), None, p, n, C.byref(opts), C.byref(res), None, 0) == -1 and b"align: bad point array" in h.lib.immesh_last_error(h.ctx)
            assert g(h.raycaster(), None, p, n, C.byref(opts), C.byref(sy), None, None) == -1 and b"align_step: bad point array" in h.lib.immesh_last_error(h.ctx)
            still_usable()
        assert f(h.raycaster(), None, None, 2, C.byref(opts), C.byref(res), None, 0) == -1
        assert f(h.raycaster(), None, None, 0, C.byref(opts), C.byref(res), None, 0) == 0 and res.status == capi.ALIGN_TOO_FEW    # no points, no array
        assert f(h.raycaster(), None, p, 2, C.byref(opts), None, None, 0) == -1 and b"result_out" in h.lib.immesh_last_error(h.ctx)
        assert f(h.raycaster(), None, p, 2, C.byref(opts), C.byref(res), None, 3) == -1 and b"history" in h.lib.immesh_last_error(h.ctx)
        assert f(h.raycaster(), None, p, 2, None, C.byref(res), None, 0) == -1 and b"options" in h.lib.immesh_last_error(h.ctx)
        assert g(h.raycaster(), None, p, 2, C.byref(opts), None, None, None) == 0                 # every output may be NULL
        with pytest.raises(RuntimeError, match=r"rc=-1: .*variant"):
            h.align_set_variant(3)
        still_usable()
        again = h.closest_points(pts, 10.0)
        assert all(again[k].tobytes() == closest[k].tobytes() for k in closest)
    finally:
        h.close()
