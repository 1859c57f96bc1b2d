"""Align a cloud to the indexed cloud on the device (include/immesh_align.h, the Cloud rule) against the numpy restatement of the contract
(tests/align_cloud_checker.py): winners and per-point terms bit for bit at the wavefront and workgroup edges, the folded system within the contract's
bound, ties, the mesh rule on degenerate faces, the sign modes of the normals, the two kernel shapes, the loop as the public pieces, the statuses,
convergence within the rounding of the coordinates, the index's other results left as they were, argument errors."""
import ctypes as C
import math

import numpy as np
import pytest

import align_checker as ac
import align_cloud_checker as acc
from immesh_amd import capi
from conftest import make_hip
from test_gpu_closest import _local
from test_gpu_render import _rand_rot, _small_cfg
import test_gpu_index_changes as ic

pytestmark = pytest.mark.gpu
SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 65537]
N_MAX = max(SIZES)
MAX_DIST = 0.2
HUBER = 0.05
CENTRE = np.array([3.5, 2.25, -0.75])
EPS = 2.0 ** -52
NORMALS = dict(k=8, max_dist=0.5, min_ratio=0.01)


@pytest.fixture(scope="module")
def hp():
    h = make_hip(capi.load_hip_library(), _small_cfg())
    yield h
    h.close()


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _target(rng):
    """a jittered bumpy sheet of 54 x 54 points over [0, 6]^2, three strays with no neighbour (normal status 1), six points on a line of their own
    (status 3), two points that are not finite (status 2; they are in no hierarchy), shuffled -> (2927, 3) float32"""
    g = np.linspace(0.0, 6.0, 54)
    X, Y = np.meshgrid(g, g, indexing="ij")
    sheet = np.stack([X, Y, 0.3 * np.sin(X) * np.cos(1.3 * Y)], axis=-1).reshape(-1, 3) + rng.uniform(-0.02, 0.02, (54 * 54, 3))
    strays = np.array([[20.0, 20.0, 20.0], [-15.0, 3.0, 2.0], [3.0, -12.0, 9.0]])
    line = np.stack([2.0 + 0.1 * np.arange(6), np.full(6, -5.0), np.zeros(6)], axis=-1)
    cloud = np.concatenate([sheet, strays, line, [[np.nan, 1.0, 0.0], [2.0, np.inf, 0.0]]]).astype(np.float32)
    return cloud[rng.permutation(len(cloud))], strays, line


@pytest.fixture(scope="module")
def case(hp):
    """the target, its normals as the device made them (the rule's input), 65 537 source points of which every smaller size is a prefix, and the
    checker's correspondences in the world and under a frame, made once: they depend on neither the mode, the centre nor huber"""
    rng = np.random.default_rng(2027)
    cloud, strays, line = _target(rng)
    xy = rng.uniform(-0.15, 6.15, (N_MAX, 2))
    world = np.concatenate([xy, (0.3 * np.sin(xy[:, :1]) * np.cos(1.3 * xy[:, 1:])) + rng.normal(scale=0.04, size=(N_MAX, 1))], axis=1)
    world[5] = [np.nan, 0.0, 0.0]; world[7] = [0.0, np.inf, 0.0]; world[9] = [1e6, -1e6, 1e6]; world[70] = [0.0, 0.0, -np.inf]
    world[100:103] = strays + rng.normal(scale=0.01, size=(3, 3))                          # winners without a normal: too few neighbours
    world[110:116] = line + rng.normal(scale=0.01, size=(6, 3))                            # ... line-like
    world = world.astype(np.float32)
    rot, pos = _rand_rot(rng), rng.uniform(-2, 2, 3)
    local = _local(world, rot, pos)
    assert hp.cloud_index_build(cloud) == (len(cloud), len(cloud) - 2)
    nr = hp.cloud_normals(mode=capi.NORMALS_CANONICAL, want=("normal", "status"), **NORMALS)
    assert (nr["too_few"], nr["line_like"], nr["not_finite"]) == (3, 6, 2), nr
    out = {"cloud": cloud, "normal": nr["normal"], "status": nr["status"], "cases": {}}
    for name, (r, p, pts) in {"world": (None, None, world), "frame": (rot, pos, local)}.items():
        out["cases"][name] = (r, p, pts, acc.correspondences(r, p, pts, MAX_DIST, cloud))
    return out


def _ready(hp, case, mode=None):
    """the case's index and normals on the device (another test may have built something else)"""
    hp.cloud_index_build(case["cloud"])
    hp.cloud_normals(mode=capi.NORMALS_CANONICAL if mode is None else mode, viewpoint=None if mode is None else [3.0, 3.0, -50.0], want=(), **NORMALS)
    hp.align_cloud_set_variant(1)


def _reference(case, corr, n, mode, centre, huber):
    p, ok, index, q = (x[:n] for x in corr)
    tm, used, flat = acc.terms(mode, p, centre, index, q, huber, case["normal"], case["status"])
    sums, bound, counts = ac.system(tm, ok, index, used, flat)
    return index, tm, sums, bound, counts


def _check_step(hp, pts, opts, huber, frame, ref, what):
    index, tm, sums, bound, counts = ref
    n = len(pts)
    sy, gindex, gterms = hp.align_cloud_step(pts, opts, huber, frame, want_index=True, want_terms=True)
    assert gindex.dtype == np.int32 and np.array_equal(gindex, index), (what, np.nonzero(gindex != index)[0][:5])
    rows = np.nonzero((gterms.view(np.uint64) != tm.view(np.uint64)).any(axis=1))[0] if n else []
    assert len(rows) == 0, (what, len(rows), rows[:3], gterms[rows[:1]], tm[rows[:1]])
    assert sy.counts() == counts and sum(counts) == n, (what, sy.counts(), counts)
    got = sy.sums()
    fs = np.array([math.fsum(gterms[:, k].tolist()) for k in range(28)])
    assert (np.abs(got - sums) <= n * EPS * bound).all(), (what, np.abs(got - sums) / np.maximum(bound, 1e-300))
    assert (np.abs(got - fs) <= n * EPS * bound).all(), what
    sy2, i2, t2 = hp.align_cloud_step(pts, opts, huber, frame)                              # nothing stored per point: the same bytes
    assert i2 is None and t2 is None and bytes(sy2) == bytes(sy), what
    sy3, _, _ = hp.align_cloud_step(pts, opts, huber, frame, want_index=True)               # and a second call
    assert bytes(sy3) == bytes(sy), what
    return sy


# the combinations of a size: both modes, in the world and under a frame, huber 0 and > 0, centre zero and not
COMBOS = [("world", 0.0, np.zeros(3)), ("world", HUBER, CENTRE), ("frame", 0.0, CENTRE), ("frame", HUBER, np.zeros(3))]


# ---- per-point winners and terms, the folded system ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_pts", SIZES)
def test_winners_terms_and_system_match_checker(hp, case, n_pts):
    _ready(hp, case)
    if n_pts == N_MAX:                                                                   # the checker first: every count occurs, and every status wins
        corr = case["cases"]["world"][3]
        counts = _reference(case, corr, n_pts, capi.ALIGN_PLANE, CENTRE, HUBER)[4]
        assert min(counts) > 0 and counts[1] == 3 and counts[3] == 9, counts
        won = set(case["status"][corr[2][corr[2] >= 0]].tolist())
        assert won == {0, 1, 3} and set(case["status"].tolist()) == {0, 1, 2, 3}           # (a point that is not finite is in no hierarchy)
        d = np.sqrt((corr[3] ** 2).sum(axis=1))[corr[2] >= 0]
        assert (d > HUBER).sum() > 100 and (d <= HUBER).sum() > 100                        # the weight acts on some points and not on others
    used = 0
    for name, huber, centre in COMBOS:
        rot, pos, pts, corr = case["cases"][name]
        frame = None if rot is None else capi.ray_frame(rot, pos)
        for mode in (capi.ALIGN_POINT, capi.ALIGN_PLANE):
            ref = _reference(case, corr, n_pts, mode, centre, huber)
            sy = _check_step(hp, pts[:n_pts], capi.align_options(mode=mode, max_dist=MAX_DIST, centre=centre), huber, frame, ref, (name, mode, huber, n_pts))
            used += sy.n_used
    if n_pts >= 63:
        assert used > 0


@pytest.mark.parametrize("n_cloud", [0, 1, 2])
def test_tiny_targets(hp, n_cloud):
    rng = np.random.default_rng(40 + n_cloud)
    cloud = np.array([[0.5, 0.25, 0.0], [0.5, 0.25, 0.125]], np.float32)[:n_cloud]
    assert hp.cloud_index_build(cloud) == (n_cloud, n_cloud)
    nr = hp.cloud_normals(want=("normal", "status"), **NORMALS)                            # one neighbour at most: no point has a normal
    pts = np.concatenate([np.tile(np.array([[0.5, 0.25, 0.0625]]), (3, 1)), rng.uniform(-0.5, 1.5, (254, 3))]).astype(np.float32)   # three exact ties
    for mode, huber in ((capi.ALIGN_POINT, 0.0), (capi.ALIGN_POINT, 0.3), (capi.ALIGN_PLANE, 0.3)):
        ref = acc.step(None, None, pts, mode, 0.75, CENTRE, cloud, huber, nr["normal"], nr["status"])
        sy = _check_step(hp, pts, capi.align_options(mode=mode, max_dist=0.75, centre=CENTRE), huber, None,
                         (ref["index"], ref["terms"], ref["sums"], ref["bound"], ref["counts"]), (n_cloud, mode, huber))
        if n_cloud == 0:
            assert sy.counts() == (0, 0, 257, 0)
        elif mode == capi.ALIGN_PLANE:
            assert sy.n_used == 0 and sy.n_flat > 3
        else:
            assert sy.n_used > 3 and ref["index"][:3].tolist() == [0, 0, 0]


# ---- ties ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_ties_go_to_the_smaller_index(hp):
    rng = np.random.default_rng(77)
    g = np.arange(5, dtype=np.float32)
    cloud = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    cloud = cloud[rng.permutation(len(cloud))]
    c = np.arange(4) + 0.5
    centres = np.stack(np.meshgrid(c, c, c, indexing="ij"), axis=-1).reshape(-1, 3)          # eight corners at the same D
    faces = np.stack(np.meshgrid(c, c, g, indexing="ij"), axis=-1).reshape(-1, 3)            # four
    edges = np.stack(np.meshgrid(c, g, g, indexing="ij"), axis=-1).reshape(-1, 3)            # two
    pts = np.concatenate([centres, faces, edges]).astype(np.float32)
    assert hp.cloud_index_build(cloud) == (125, 125) and len(pts) == 64 + 80 + 100
    ref = acc.step(None, None, pts, acc.POINT, 1.0, np.zeros(3), cloud)
    d = ((pts[:, None, :].astype(np.float64) - cloud[None].astype(np.float64)) ** 2).sum(axis=2)
    first = np.array([np.flatnonzero(row == row.min())[0] for row in d])
    assert ((d == d.min(axis=1)[:, None]).sum(axis=1) == np.repeat([8, 4, 2], [64, 80, 100])).all() and np.array_equal(ref["index"], first)
    for variant in (0, 1):
        hp.align_cloud_set_variant(variant)
        sy, index, terms = hp.align_cloud_step(pts, capi.align_options(max_dist=1.0), 0.0, None, True, True)
        assert np.array_equal(index, first) and _bits(terms) == _bits(ref["terms"]) and sy.n_used == len(pts), variant
    hp.align_cloud_set_variant(1)


# ---- the mesh rule on degenerate faces -------------------------------------------------------------------------------------------------------------------
def test_point_mode_equals_the_mesh_rule_on_degenerate_faces(hp, case):
    _ready(hp, case)
    n = len(case["cloud"])
    hp.raycast_build_triangles(case["cloud"], np.repeat(np.arange(n, dtype=np.int32)[:, None], 3, axis=1))
    for name, centre in (("world", np.zeros(3)), ("frame", CENTRE)):
        rot, pos, pts, _ = case["cases"][name]
        frame = None if rot is None else capi.ray_frame(rot, pos)
        opts = capi.align_options(mode=capi.ALIGN_POINT, max_dist=MAX_DIST, centre=centre)
        sc, index, tc = hp.align_cloud_step(pts, opts, 0.0, frame, True, True)
        sm, face, tm = hp.align_step(pts, opts, frame, True, True)
        assert np.array_equal(index, face) and _bits(tc) == _bits(tm) and bytes(sc) == bytes(sm), name
        assert sc.n_used > 60000 and sc.n_no_face > 0


# ---- the sign mode of the normals, the two kernel shapes -------------------------------------------------------------------------------------------------
def test_plane_systems_do_not_depend_on_the_sign_mode(hp, case):
    rot, pos, pts, _ = case["cases"]["frame"]
    opts = capi.align_options(mode=capi.ALIGN_PLANE, max_dist=MAX_DIST, centre=CENTRE)
    got, normals = [], []
    for mode in (capi.NORMALS_CANONICAL, capi.NORMALS_VIEWPOINT):
        _ready(hp, case, mode)
        normals.append(hp.cloud_normals_get()[0])
        for huber in (0.0, HUBER):
            sy, _, terms = hp.align_cloud_step(pts, opts, huber, capi.ray_frame(rot, pos), want_terms=True)
            got.append(bytes(sy) + _bits(terms))
    have = np.isfinite(normals[0]).all(axis=1)
    assert (normals[0][have] != normals[1][have]).any(axis=1).sum() > 100                  # the two modes do differ in sign
    assert got[0] == got[2] and got[1] == got[3]
    _ready(hp, case)


@pytest.mark.parametrize("n_pts", [1, 65, 257, 65537])
def test_the_two_kernel_shapes_give_the_same_bits(hp, case, n_pts):
    _ready(hp, case)
    rot, pos, pts, _ = case["cases"]["frame"]
    try:
        for mode in (capi.ALIGN_POINT, capi.ALIGN_PLANE):
            opts = capi.align_options(mode=mode, max_dist=MAX_DIST, centre=CENTRE)
            got = []
            for variant in (0, 1):
                hp.align_cloud_set_variant(variant)
                sy, index, terms = hp.align_cloud_step(pts[:n_pts], opts, HUBER, capi.ray_frame(rot, pos), True, True)
                got.append(bytes(sy) + _bits(index) + _bits(terms) + bytes(hp.align_cloud_step(pts[:n_pts], opts, HUBER, capi.ray_frame(rot, pos))[0]))
            assert got[0] == got[1], (mode, n_pts)
    finally:
        hp.align_cloud_set_variant(1)


# ---- the loop ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sheet():
    return acc.convergence_case()


def _sheet_ready(hp, sheet):
    cloud, src, centre = sheet
    assert hp.cloud_index_build(cloud) == (1600, 1600)
    assert hp.cloud_normals(8, 0.5, want=())["with_normal"] == 1600


@pytest.mark.parametrize("mode", [capi.ALIGN_POINT, capi.ALIGN_PLANE])
def test_loop_equals_stepping_by_hand(hp, sheet, mode):
    cloud, src, centre = sheet
    _sheet_ready(hp, sheet)
    for huber, max_iters in ((0.0, 30), (0.01, 2)):
        opts = capi.align_options(mode=mode, max_dist=acc.SHEET_MAX_DIST, centre=centre, max_iters=max_iters)
        frame0 = capi.ray_frame(pos=[0.001, 0.0, -0.001])
        res, hist = hp.align_cloud(src, opts, huber, frame0)
        frame, status, rows = capi.RayFrame.from_buffer_copy(frame0), capi.ALIGN_MAX_ITERS, []
        for it in range(max_iters):
            sy, _, _ = hp.align_cloud_step(src, opts, huber, frame)
            rms = math.sqrt(sy.e / (sy.n_used if mode == capi.ALIGN_PLANE else 3 * sy.n_used))
            bad, delta = hp.align_solve(sy, 0.0)
            assert not bad
            frame = hp.align_update(frame, centre, delta)
            d = delta.tolist()
            nw, nv = math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]), math.sqrt((d[3] * d[3] + d[4] * d[4]) + d[5] * d[5])
            rows.append([float(sy.n_used), rms, nw, nv])
            if nw <= opts.eps_rot and nv <= opts.eps_trans:
                status = capi.ALIGN_CONVERGED
                break
        assert (res.status, res.iterations) == (status, len(rows)) and status == (capi.ALIGN_CONVERGED if max_iters == 30 else capi.ALIGN_MAX_ITERS)
        assert bytes(res.frame) == bytes(frame) and bytes(res.system) == bytes(sy) and res.rms == rows[-1][1]
        assert _bits(hist) == _bits(np.array(rows))
        one, total = hp.align_cloud_timing()
        assert one > 0 and total >= one


@pytest.mark.parametrize("mode", [capi.ALIGN_POINT, capi.ALIGN_PLANE])
def test_converges_to_the_rounding_of_the_coordinates(hp, sheet, mode):
    """the source is a subset of the target moved by a known small motion and rounded to float: at the true pose every twin is the winner, so the
    optimum's rms is bounded by 4 * 2^-24 * max|coordinate|; tests/test_align_cloud_cpu.py asks the same of the checker's loop on these inputs"""
    cloud, src, centre = sheet
    _sheet_ready(hp, sheet)
    res, hist = hp.align_cloud(src, capi.align_options(mode=mode, max_dist=acc.SHEET_MAX_DIST), centre="mean")
    bound = acc.rms_bound(cloud, src)
    print("mode", mode, "status", res.status, "iterations", res.iterations, "rms", res.rms, "bound", bound)
    assert res.status == capi.ALIGN_CONVERGED
    assert res.rms <= bound, (res.rms, bound)
    assert res.system.n_used == len(src) and hist[0, 1] > 1e-3
    rot, pos = np.array(list(res.frame.rot)).reshape(3, 3), np.array(list(res.frame.pos))
    assert np.abs(rot - acc.TRUE_ROT).max() < 1e-6 and np.abs(pos - acc.TRUE_POS).max() < 1e-6


def test_cloud_align_tool_moves_b_onto_a(hp, sheet):
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import cloud_align
    cloud, src, centre = sheet
    for mode, huber in (("plane", 0.0), ("point", 0.0), ("plane", 0.05)):
        moved, block = cloud_align.align(hp, cloud, src, mode, 8, huber, acc.SHEET_MAX_DIST, 30, 0.5)
        assert block["status"] == "converged" and block["iterations"] == len(block["rms_history"]) <= 10 and block["fitness"] == 1.0
        assert moved.dtype == np.float32 and np.abs(moved - cloud[::3]).max() < 1e-5 and block["rms"] <= acc.rms_bound(cloud, src)


def test_statuses(hp, sheet):
    cloud, src, centre = sheet
    assert hp.cloud_index_build(np.zeros((0, 3), np.float32)) == (0, 0)                      # an empty index: TOO_FEW, no error
    res, hist = hp.align_cloud(src, capi.align_options(mode=capi.ALIGN_POINT))
    assert (res.status, res.iterations, res.rms, len(hist)) == (capi.ALIGN_TOO_FEW, 1, 0.0, 1) and res.system.counts() == (0, 0, len(src), 0)
    _sheet_ready(hp, sheet)
    frame0 = capi.ray_frame(pos=[0.0, 0.0, 0.01])
    for mode, n in ((capi.ALIGN_POINT, 2), (capi.ALIGN_PLANE, 5), (capi.ALIGN_POINT, 0)):
        res, _ = hp.align_cloud(cloud[:n], capi.align_options(mode=mode, max_dist=0.1), 0.0, frame0)
        assert (res.status, res.iterations, res.system.n_used) == (capi.ALIGN_TOO_FEW, 1, n) and bytes(res.frame) == bytes(frame0)
    res, hist = hp.align_cloud(src, capi.align_options(mode=capi.ALIGN_PLANE, max_dist=acc.SHEET_MAX_DIST, centre=centre, max_iters=1, eps_rot=1e-12, eps_trans=1e-12))
    assert (res.status, res.iterations, len(hist)) == (capi.ALIGN_MAX_ITERS, 1, 1) and bytes(res.frame) != bytes(capi.ray_frame())
    assert hp.align_cloud(src, capi.align_options(mode=capi.ALIGN_POINT, max_dist=acc.SHEET_MAX_DIST, centre=centre))[0].status == capi.ALIGN_CONVERGED
    line = np.stack([0.5 * np.arange(12), np.zeros(12), np.zeros(12)], axis=-1).astype(np.float32)   # a collinear target through the centre:
    assert hp.cloud_index_build(line) == (12, 12)                                          # no row constrains the rotation about it, H_00 == 0
    on = (line + np.array([0.1, 0.0, 0.0], np.float32)).astype(np.float32)
    res, hist = hp.align_cloud(on, capi.align_options(mode=capi.ALIGN_POINT, max_dist=0.2, damping=0.0), 0.0, frame0)
    assert (res.status, res.iterations, res.system.n_used) == (capi.ALIGN_DEGENERATE, 1, 12) and bytes(res.frame) == bytes(frame0)
    assert hist.tolist() == [[12.0, res.rms, 0.0, 0.0]] and res.rms > 0
    res, _ = hp.align_cloud(on, capi.align_options(mode=capi.ALIGN_POINT, max_dist=0.2, damping=1e-6), 0.0, frame0)
    assert res.status in (capi.ALIGN_CONVERGED, capi.ALIGN_MAX_ITERS)


# ---- the index's other results ----------------------------------------------------------------------------------------------------------------------------
OWN_PTS = (ic.CLOUD[np.isfinite(ic.CLOUD).all(axis=1)][::25] + np.float32(0.03)).astype(np.float32)   # near points of the index's cloud


def _align_on_the_index(h):
    for mode in (capi.ALIGN_POINT, capi.ALIGN_PLANE):
        opts = capi.align_options(mode=mode, max_dist=1.0, max_iters=3)
        for variant in (0, 1):
            h.align_cloud_set_variant(variant)
            sy, index, terms = h.align_cloud_step(OWN_PTS, opts, 0.1, None, True, True)
            assert sy.n_used > 0 and (index >= 0).sum() == sy.n_used + sy.n_flat
        h.align_cloud_set_variant(1)
        assert h.align_cloud(OWN_PTS, opts, 0.1)[0].iterations >= 1


def test_an_alignment_leaves_every_other_result_of_the_index(hp):
    """behind every derived result of the index (the last nearest query, neighbour and count queries, normals, agreement, clusters, the last mask), a
    step of both shapes and a loop in both modes: every fetch answers byte for byte as before, the apply keeps what the mask kept"""
    hp.raycast_build_triangles(ic.VTX, ic.FACES)
    ic._leaves(hp, _align_on_the_index)
    hp.nearest_points(ic.PTS, 1.0)                                                         # a query, a reduction and an apply still work
    assert hp.align_cloud_step(OWN_PTS, capi.align_options(max_dist=1.0), 0.1)[0].n_used > 0
    st, hist = hp.nearest_stats(0.25, 8)
    assert st.n_points == len(ic.PTS)


# ---- argument errors -------------------------------------------------------------------------------------------------------------------------------------------
def test_argument_errors(sheet):
    cloud, src, centre = sheet
    h = make_hip(capi.load_hip_library(), _small_cfg())
    try:
        pts = src[::13]
        good = dict(mode=capi.ALIGN_POINT, max_dist=0.25)
        plane = dict(mode=capi.ALIGN_PLANE, max_dist=0.25)
        calls = {"align_cloud_step": lambda o, *a, **k: h.align_cloud_step(pts, o, *a, **k), "align_cloud": lambda o, *a, **k: h.align_cloud(pts, o, *a, **k)}
        for who, call in calls.items():
            with pytest.raises(RuntimeError, match=rf"rc=-1: .*{who}: no index has been built"):
                call(capi.align_options(**good))                                           # an index that was created but never built
        h.cloud_index_build(cloud)
        for who, call in calls.items():
            with pytest.raises(RuntimeError, match=rf"rc=-1: .*{who}: PLANE mode needs the index's normals"):
                call(capi.align_options(**plane))
        h.cloud_normals(8, 0.5, want=())
        near = h.nearest_points(pts, 0.25)

        def still_usable():
            for o in (good, plane):
                sy, index, _ = h.align_cloud_step(pts, capi.align_options(**o), 0.0, None, True)
                assert sy.counts() == (len(pts), 0, 0, 0) and (index >= 0).all()
            assert h.align_cloud(pts, capi.align_options(**plane))[0].status == capi.ALIGN_CONVERGED
            assert _bits(h.nearest_stats(0.25, 8)[1]) == _bits(hist0)

        hist0 = h.nearest_stats(0.25, 8)[1]
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
            with pytest.raises(RuntimeError, match=r"rc=-1: .*align_cloud: .*" + text):
                h.align_cloud(pts, opts)
            if step_too:
                with pytest.raises(RuntimeError, match=r"rc=-1: .*align_cloud_step: .*" + text):
                    h.align_cloud_step(pts, opts)
        still_usable()
        for huber in (-1e-9, -inf, inf, nan):
            for who, call in calls.items():
                with pytest.raises(RuntimeError, match=rf"rc=-1: .*{who}: need huber >= 0, finite"):
                    call(capi.align_options(**good), huber)
        for bad in (capi.ray_frame(pos=[nan, 0, 0]), capi.ray_frame(rot=np.diag([1.0, inf, 1.0]))):
            for who, call in calls.items():
                with pytest.raises(RuntimeError, match=rf"rc=-1: .*{who}: .*finite"):
                    call(capi.align_options(**good), 0.0, bad)
        with pytest.raises(RuntimeError, match=r"rc=-1: .*align_cloud_step: options are NULL"):
            h.align_cloud_step(pts, None)
        still_usable()
        opts, res, sy = capi.align_options(**good), capi.AlignResult(), capi.AlignSystem()
        f = h.lib.immesh_align_cloud
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(capi.AlignOptions), C.c_double, C.POINTER(capi.AlignResult), C.c_void_p, C.c_int64]
        g = h.lib.immesh_align_cloud_step
        g.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(capi.AlignOptions), C.c_double, C.POINTER(capi.AlignSystem), C.c_void_p, C.c_void_p]
        err = h.lib.immesh_last_error; err.restype = C.c_char_p; err.argtypes = [C.c_void_p]
        p, x = pts.ctypes.data_as(C.c_void_p), h.cloud_index()
        for n in (-1, 2 ** 31 - 1, 2 ** 40):
            assert f(x, None, p, n, C.byref(opts), 0.0, C.byref(res), None, 0) == -1 and b"align_cloud: bad point array" in err(h.ctx)
            assert g(x, None, p, n, C.byref(opts), 0.0, C.byref(sy), None, None) == -1 and b"align_cloud_step: bad point array" in err(h.ctx)
        assert f(x, None, None, 2, C.byref(opts), 0.0, C.byref(res), None, 0) == -1
        assert f(x, None, None, 0, C.byref(opts), 0.0, C.byref(res), None, 0) == 0 and res.status == capi.ALIGN_TOO_FEW    # no points, no array
        assert f(x, None, p, 2, C.byref(opts), 0.0, None, None, 0) == -1 and b"align_cloud: result_out is NULL" in err(h.ctx)
        assert f(x, None, p, 2, C.byref(opts), 0.0, C.byref(res), None, 3) == -1 and b"align_cloud: bad history array" in err(h.ctx)
        assert f(x, None, p, 2, C.byref(opts), 0.0, C.byref(res), None, -1) == -1 and b"align_cloud: bad history array" in err(h.ctx)
        assert f(x, None, p, 2, None, 0.0, C.byref(res), None, 0) == -1 and b"align_cloud: options are NULL" in err(h.ctx)
        assert g(x, None, p, 2, C.byref(opts), 0.0, None, None, None) == 0                   # every output may be NULL
        for variant in (2, -1):
            with pytest.raises(RuntimeError, match=r"rc=-1: .*align_cloud_set_variant: variant"):
                h.align_cloud_set_variant(variant)
        still_usable()
        again = h.nearest_points(pts, 0.25)
        assert all(again[k].tobytes() == near[k].tobytes() for k in near)
        h.radius_count_cloud(0.3)
        m = h.cloud_outliers_radius(3)
        assert m["kept"] > 0 and len(h.cloud_index_apply_outliers()) == m["kept"]          # an apply drops the normals:
        for who, call in calls.items():
            with pytest.raises(RuntimeError, match=rf"rc=-1: .*{who}: PLANE mode needs the index's normals"):
                call(capi.align_options(**plane))
        assert h.align_cloud(pts, capi.align_options(**good))[0].system.n_used == len(pts)   # POINT mode needs none
        h.cloud_normals(8, 0.5, want=())
        assert h.align_cloud(pts, capi.align_options(**plane))[0].system.n_used == len(pts)
    finally:
        h.close()
