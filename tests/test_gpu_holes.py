"""The holes on the device (include/immesh_topology.h, the Holes rule) against the numpy restatement of the contract (tests/holes_checker.py), bit for
bit on every output: the stats, the loop tables with their boxes and cycle offsets, the cycles, the new faces and their loops.  Closed forms,
cylinders at the sizes where the ranking gains a round or the launches a wavefront or a workgroup, a long loop beside many short ones, every limit,
order-freedom, every fetch and error, the apply against a caster freshly built from faces ++ new_faces, the orientation before the holes, the live
mesh as a snapshot without side effects, scale, and tools/mesh_eval.py's --fill-holes."""
import ctypes as C
import importlib.util
import json
import os
import sys

import numpy as np
import pytest

import holes_checker as hc
import orient_checker as oc
import topology_checker as tc
from immesh_amd import capi, synth
from conftest import make_hip
from parity_utils import compare_plane_tables_fast
from test_gpu_render import _small_cfg
from test_gpu_topology import _device as _analysis, _same as _same_analysis, _write_ply

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARRAYS = hc.TABLES + (("cycle", np.int32), ("new_faces", np.int32), ("new_loop", np.int32))


@pytest.fixture(scope="module")
def hp():
    h = make_hip(capi.load_hip_library(), _small_cfg())
    yield h
    h.close()


def _err(h):
    f = h.lib.immesh_last_error; f.restype = C.c_char_p; f.argtypes = [C.c_void_p]
    return f(h.ctx)


def _device(h, max_edges, max_diagonal=0.0):
    """the holes pass, then every fetch, in the checker's shape"""
    st = h.topology_holes(max_edges, max_diagonal)
    out = {"stats": {n: getattr(st, n) for n in hc.STAT_NAMES}}
    out.update(h.topology_holes_loops())
    out["cycle"] = h.topology_holes_cycles()
    out["new_loop"], out["new_faces"] = h.topology_holes_faces()
    return out


def _same(got, ref, what=""):
    assert got["stats"] == ref["stats"], (what, got["stats"], ref["stats"])
    for k, t in ARRAYS:
        assert got[k].dtype == ref[k].dtype == t and got[k].shape == ref[k].shape, (what, k, got[k].shape, ref[k].shape)
        assert not (t == np.float32 and np.isnan(got[k]).any()) and np.array_equal(got[k], ref[k]), (what, k, got[k][:12], ref[k][:12])   # boxes as values


def _check(h, vtx, faces, max_edges, max_diagonal=0.0, what="", ref=None):
    """build, analyse, and the pass against the checker -> the checker's result"""
    h.raycast_build_triangles(vtx, faces)
    st = h.topology_analyse()
    ref = hc.holes(vtx, faces, max_edges, max_diagonal) if ref is None else ref
    _same(_device(h, max_edges, max_diagonal), ref, (what, max_edges, max_diagonal))
    assert ref["stats"]["n_loops"] == st.n_boundary_loops and int(ref["n_edges"].sum()) == st.n_boundary
    return ref


# ---- the CPU tier's shapes ---------------------------------------------------------------------------------------------------------------------------
def test_closed_forms_on_the_device(hp):
    ref = _check(hp, *hc.open_pyramid(), 3)
    assert ref["new_faces"].tolist() == [[0, 2, 1]]
    vtx, faces = hc.open_pyramid()
    assert _check(hp, vtx, faces[:1], 16)["status"].tolist() == [hc.OUTLINE]
    ref = _check(hp, *tc.grid_sheet(3, 3, holes=[(1, 1)]), 4)
    assert ref["new_faces"].tolist() == [[5, 10, 6], [5, 9, 10]] and ref["status"].tolist() == [hc.TOO_LONG, hc.FILLED]
    assert _check(hp, *hc.touching_holes(), 64)["status"].tolist() == [hc.FILLED, hc.NONSIMPLE]
    assert _check(hp, *hc.blocked_sheet(), 4)["status"].tolist() == [hc.TOO_LONG, hc.BLOCKED]
    assert _check(hp, *hc.blocked_sheet(), 64)["status"].tolist() == [hc.FILLED, hc.BLOCKED]
    assert _check(hp, *tc.moebius(9), 64)["status"].tolist() == [hc.NONSIMPLE]
    vtx, faces = tc.grid_sheet(3, 3, holes=[(1, 1)])
    faces[0] = faces[0][[0, 2, 1]]
    assert _check(hp, vtx, faces, 64)["status"].tolist() == [hc.NONSIMPLE, hc.FILLED]
    for n in (3, 8):
        assert _check(hp, *hc.cylinder(n, reverse=True), n)["stats"]["n_filled"] == 2


def test_limits_on_the_device(hp):
    vtx, faces = tc.grid_sheet(4, 5, holes=[(1, 1), (1, 2)])
    for max_edges, want in ((5, hc.TOO_LONG), (6, hc.FILLED), (7, hc.FILLED)):
        assert _check(hp, vtx, faces, max_edges)["status"][1] == want
    for md, want in ((0.0, hc.FILLED), (3.0, hc.FILLED), (2.0, hc.TOO_WIDE)):
        assert _check(hp, vtx, faces, 6, md)["status"][1] == want
    vtx, faces = tc.grid_sheet(5, 6, holes=[(i, j) for i in (1, 2, 3) for j in (1, 2, 3, 4)])
    assert _check(hp, vtx, faces, 64, 5.0)["status"].tolist() == [hc.TOO_WIDE, hc.FILLED]                                # a diagonal exactly equal passes
    assert _check(hp, vtx, faces, 64, float(np.nextafter(5.0, 0.0)))["status"].tolist() == [hc.TOO_WIDE, hc.TOO_WIDE]
    assert _check(hp, vtx, faces, 13, 5.0)["status"].tolist() == [hc.TOO_LONG, hc.TOO_LONG]
    vtx, faces = tc.grid_sheet(3, 3, holes=[(1, 1)])
    vtx[5, 0], vtx[6, 0], vtx[9, 0], vtx[10, 0] = np.nan, np.nan, np.inf, -np.inf
    assert _check(hp, vtx, faces, 4, 0.0)["box"][1].tolist() == [np.inf, 1, 0, -np.inf, 2, 0]
    assert _check(hp, vtx, faces, 4, 1e30)["status"].tolist() == [hc.TOO_LONG, hc.TOO_WIDE]
    vtx[10, 0] = 2.0
    assert _check(hp, vtx, faces, 4, 1.5)["status"].tolist() == [hc.TOO_LONG, hc.FILLED]


@pytest.mark.parametrize("case", range(11))
def test_sheets_with_fragments_match_checker(hp, case):
    rng = np.random.default_rng(700 + case)
    vtx, faces = tc.sheet_with_fragments(rng, 30, 30, 80, 20)
    ref = _check(hp, vtx, faces, 12, what=case)
    assert ref["stats"]["n_filled"] >= 30 and ref["stats"]["n_nonsimple"] >= 5


# ---- cylinders: the wavefront, the workgroup and every power-of-two round of the ranking ------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 4, 63, 64, 65, 129, 256, 257, 1024, 1025, 4097])
def test_cylinders(hp, n):
    vtx, faces = hc.cylinder(n)
    ref = _check(hp, vtx, faces, n, what=n)
    assert ref["stats"]["n_filled"] == 2 and ref["stats"]["n_new_faces"] == 2 * (n - 2) and ref["cycle"][:n].tolist() == list(range(n))
    if n > 3:
        none = _check(hp, vtx, faces, n - 1, what=(n, "one short"))
        assert none["stats"]["n_filled"] == 0 and none["stats"]["n_too_long"] == 2 and np.array_equal(none["cycle"], ref["cycle"])
    sv, sf, perm = hc.relabel(np.random.default_rng(n), vtx, faces)                    # the label lies mid-cycle and the terminal anywhere
    shuffled = _check(hp, sv, sf, n, what=(n, "shuffled"))
    assert shuffled["stats"] == ref["stats"]
    for l in range(2):
        cyc = shuffled["cycle"][l * n:(l + 1) * n]
        assert cyc[0] == cyc.min() and set(cyc.tolist()) in (set(perm[:n].tolist()), set(perm[n:].tolist()))


def test_a_long_loop_beside_three_hundred_short_ones(hp):
    rng = np.random.default_rng(8)
    vtx, faces = hc.sheet_with_long_hole(rng, 4097, 300)
    ref = _check(hp, vtx, faces, 4097)
    assert sorted(ref["n_edges"].tolist()) == [4] * 300 + [256, 4097] and ref["stats"]["n_filled"] == 302 and ref["stats"]["largest_simple_loop_edges"] == 4097
    short = _check(hp, vtx, faces, 16)
    assert short["stats"]["n_filled"] == 300 and short["stats"]["n_too_long"] == 2 and np.array_equal(short["cycle"], ref["cycle"])


# ---- nothing to do ---------------------------------------------------------------------------------------------------------------------------------------
def test_zero_faces_closed_torus_and_degenerate_faces(hp):
    zero = dict.fromkeys(hc.STAT_NAMES, 0)
    vtx = np.zeros((3, 3), np.float32)
    for v, f in ((vtx, np.zeros((0, 3), np.int32)), tc.torus(16, 16), (vtx, np.array([[0, 0, 1], [2, 2, 2], [1, 0, 1]] * 30, np.int32))):
        ref = _check(hp, v, f, 16, 1.0)
        assert ref["stats"] == zero and all(len(ref[k]) == 0 for k, _ in ARRAYS)
        n = len(f)
        hp.topology_holes_apply()                                                      # nothing to add: a rebuild of the same faces
        assert hp._raycast_sizes()[1] == n


# ---- order-freedom -------------------------------------------------------------------------------------------------------------------------------------
def test_face_order_changes_nothing_and_two_runs_give_equal_bits(hp):
    rng = np.random.default_rng(17)
    vtx, faces = tc.sheet_with_fragments(rng, 40, 30, 60, 40)
    vtx, faces = oc.with_moebius(vtx, faces, (9,))
    ref = _check(hp, vtx, faces, 12, 0.5)
    a, b = _device(hp, 12, 0.5), _device(hp, 12, 0.5)
    assert a["stats"] == b["stats"] and all(a[k].tobytes() == b[k].tobytes() for k, _ in ARRAYS)
    for seed in (1, 2):
        _check(hp, vtx, faces[np.random.default_rng(seed).permutation(len(faces))], 12, 0.5, ref=ref, what=("faces shuffled", seed))
    assert ref["stats"]["n_filled"] > 20 and ref["stats"]["n_nonsimple"] > 5 and ref["stats"]["n_too_wide"] + ref["stats"]["n_too_long"] >= 1


# ---- fetches and errors ------------------------------------------------------------------------------------------------------------------------------------
def test_fetches_lifecycle_and_argument_errors():
    h = make_hip(capi.load_hip_library(), _small_cfg())
    try:
        vtx, faces = tc.grid_sheet(6, 5, holes=[(1, 1), (3, 3), (4, 1)])
        ref = hc.holes(vtx, faces, 8)
        n_l, n_c, n_f = ref["stats"]["n_loops"], ref["stats"]["n_cycle_vertices"], ref["stats"]["n_new_faces"]
        assert (n_l, n_c, n_f) == (4, 34, 6)
        fetches = (h.topology_holes_loops, h.topology_holes_cycles, h.topology_holes_faces, h.topology_holes_apply)
        with pytest.raises(RuntimeError, match=r"rc=-1: .*built"):
            h.topology_holes(8)                                                       # before a build
        h.raycast_build_triangles(vtx, faces)
        with pytest.raises(RuntimeError, match=r"rc=-1: .*no analysis"):
            h.topology_holes(8)                                                       # before an analysis
        h.topology_analyse()
        for fetch in fetches:
            with pytest.raises(RuntimeError, match=r"rc=-1: .*no holes pass"):
                fetch()                                                               # a fetch or an apply before a pass
        _same(_device(h, 8), ref)
        h.topology_analyse()
        for fetch in fetches:
            with pytest.raises(RuntimeError, match=r"rc=-1: .*no holes pass"):
                fetch()                                                               # after a new analysis
        _same(_device(h, 8), ref)
        h.raycast_build_triangles(vtx, faces)
        for fetch in fetches:
            with pytest.raises(RuntimeError, match=r"rc=-1: .*no analysis"):
                fetch()                                                               # after a rebuild
        h.topology_analyse()
        _same(_device(h, 8), ref)
        h.topology_orient(oc.ORIENT_FIRST)
        h.topology_orient_apply()
        for fetch in fetches:
            with pytest.raises(RuntimeError, match=r"rc=-1: .*no analysis"):
                fetch()                                                               # after an orient-apply
        h.topology_analyse()
        for fetch in fetches:
            with pytest.raises(RuntimeError, match=r"rc=-1: .*no holes pass"):
                fetch()                                                               # and it does not come back with the next analysis

        def still_usable():
            _same(_device(h, 8), ref)

        still_usable()
        for bad in (2, 0, -1, -2 ** 40):
            with pytest.raises(RuntimeError, match=r"rc=-1: .*max_edges"):
                h.topology_holes(bad)
            assert np.array_equal(h.topology_holes_cycles(), ref["cycle"])            # refused before anything was touched: the last pass stays
            still_usable()
        for bad in (-1.0, -1e-300, np.nan, np.inf, -np.inf):
            with pytest.raises(RuntimeError, match=r"rc=-1: .*max_diagonal"):
                h.topology_holes(8, bad)
            still_usable()
        _same(_device(h, 2 ** 62, 1e300), hc.holes(vtx, faces, 2 ** 62, 1e300))
        f = h.lib.immesh_topology_holes; f.argtypes = [C.c_void_p, C.c_int64, C.c_double, C.c_void_p]
        assert f(None, 8, 0.0, None) == -1 and f(h.raycaster(), 8, 0.0, None) == 0     # stats may be NULL
        # loops
        g = h.lib.immesh_topology_holes_loops; g.argtypes = [C.c_void_p] + [C.c_void_p] * 5 + [C.c_int64, C.c_void_p]
        n = C.c_int64(-5)
        assert g(h.raycaster(), None, None, None, None, None, -1, C.byref(n)) == -1 and b"cap" in _err(h)
        assert g(None, None, None, None, None, None, 0, None) == -1 and g(h.raycaster(), None, None, None, None, None, 0, None) == 0
        for which, (k, t) in enumerate(hc.TABLES):
            room = np.zeros((n_l + 1,) + ref[k].shape[1:], t)
            args = [None] * 5
            args[which] = room.ctypes.data_as(C.c_void_p)
            n = C.c_int64(-5)
            assert g(h.raycaster(), *args, n_l - 1, C.byref(n)) == -4 and n.value == n_l and b"cap %d < %d" % (n_l - 1, n_l) in _err(h)
            assert not room.any()
            assert g(h.raycaster(), *args, n_l, C.byref(n)) == 0 and n.value == n_l and np.array_equal(room[:n_l], ref[k]) and not room[n_l:].any()
        # cycles
        g = h.lib.immesh_topology_holes_cycles; g.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
        room = np.zeros(n_c + 1, np.int32)
        n = C.c_int64(-5)
        assert g(h.raycaster(), None, 0, C.byref(n)) == 0 and n.value == n_c and g(h.raycaster(), None, 0, None) == 0 and g(None, None, 0, None) == -1
        assert g(h.raycaster(), None, -1, C.byref(n)) == -1 and b"cap" in _err(h)
        assert g(h.raycaster(), room.ctypes.data_as(C.c_void_p), n_c - 1, C.byref(n)) == -4 and n.value == n_c and not room.any()
        assert g(h.raycaster(), room.ctypes.data_as(C.c_void_p), n_c, C.byref(n)) == 0 and np.array_equal(room[:n_c], ref["cycle"]) and room[n_c] == 0
        # faces
        g = h.lib.immesh_topology_holes_faces; g.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
        loop, nf3 = np.zeros(n_f + 1, np.int32), np.zeros((n_f + 1, 3), np.int32)
        n = C.c_int64(-5)
        assert g(h.raycaster(), None, None, 0, C.byref(n)) == 0 and n.value == n_f and g(h.raycaster(), None, None, 0, None) == 0
        assert g(None, None, None, 0, None) == -1 and g(h.raycaster(), None, None, -1, C.byref(n)) == -1 and b"cap" in _err(h)
        assert g(h.raycaster(), loop.ctypes.data_as(C.c_void_p), None, n_f - 1, C.byref(n)) == -4 and n.value == n_f and not loop.any()
        assert g(h.raycaster(), None, nf3.ctypes.data_as(C.c_void_p), n_f - 1, C.byref(n)) == -4 and not nf3.any() and b"cap %d < %d" % (n_f - 1, n_f) in _err(h)
        assert g(h.raycaster(), loop.ctypes.data_as(C.c_void_p), None, n_f, C.byref(n)) == 0 and np.array_equal(loop[:n_f], ref["new_loop"])
        assert g(h.raycaster(), None, nf3.ctypes.data_as(C.c_void_p), n_f, C.byref(n)) == 0 and np.array_equal(nf3[:n_f], ref["new_faces"]) and not nf3[n_f].any()
        a = h.lib.immesh_topology_holes_apply; a.argtypes = [C.c_void_p]
        assert a(None) == -1
        t = h.lib.immesh_topology_holes_last_timing; t.argtypes = [C.c_void_p, C.c_void_p]
        assert t(h.raycaster(), None) == -1 and t(None, None) == -1 and h.topology_holes_timing()[0] > 0.0
        still_usable()
    finally:
        h.close()


# ---- apply -----------------------------------------------------------------------------------------------------------------------------------------------------
def test_apply_equals_a_fresh_build_from_the_closed_faces(hp):
    rng = np.random.default_rng(31)
    vtx, faces = tc.sheet_with_fragments(rng, 30, 20, 40, 40)
    vtx = vtx + rng.normal(scale=0.01, size=vtx.shape).astype(np.float32)
    dirs = (rng.normal(size=(2000, 3)) * np.array([0.3, 0.3, 1.0])).astype(np.float32)    # steep rays from a metre above the sheet (1.5 x 1.0)
    org = (rng.uniform(0.0, 1.0, (2000, 3)) * np.array([1.5, 1.0, 0.0]) + np.array([0.0, 0.0, 1.0])).astype(np.float32)
    dirs[:, 2] = -np.abs(dirs[:, 2]) - 0.5
    pts = np.concatenate([rng.uniform(-0.2, 1.7, (3000, 2)), rng.normal(scale=0.2, size=(3000, 1))], axis=1).astype(np.float32)
    other = make_hip(capi.load_hip_library(), _small_cfg())
    try:
        hp.raycast_build_triangles(vtx, faces)
        t0, f0 = hp.raycast(capi.ray_frame(), dirs, org, 0.0, 100.0)
        assert hp.mesh_sample(300.0, 7, fetch=False) > 500 and len(hp.raycast_points(0.05)) > 100   # samples and a cast's points: the apply discards both
        before = _analysis(hp)["stats"]
        ref = hc.holes(vtx, faces, 12)
        _same(_device(hp, 12), ref)
        k, E = ref["stats"]["n_filled"], ref["stats"]["n_edges_closed"]
        assert k >= 20 and ref["stats"]["n_nonsimple"] >= 3
        hp.topology_orient(oc.ORIENT_FIRST)                                           # an orientation of the same analysis: the apply discards it too
        hp.topology_holes_apply()
        assert hp.topology_holes_timing()[1] > 0.0
        for call in (hp.topology_faces, hp.topology_orient_faces, hp.topology_orient_apply, hp.topology_holes_loops, hp.topology_holes_cycles,
                     hp.topology_holes_faces, hp.topology_holes_apply, lambda: hp.topology_holes(12)):
            with pytest.raises(RuntimeError, match=r"rc=-1: .*no analysis"):
                call()
        with pytest.raises(RuntimeError, match=r"rc=-1: .*no NEAREST cast"):
            hp.raycast_points(0.05)
        with pytest.raises(RuntimeError, match=r"rc=-1: .*no samples"):
            hp.nearest_samples(1.0, want=())
        closed = hc.closed(faces, ref)
        other.raycast_build_triangles(vtx, closed)
        assert hp._raycast_sizes() == other._raycast_sizes() and hp._raycast_sizes()[1] == len(faces) + E - 2 * k
        # rays and closest points: equal to the fresh build's bit for bit; the rays that went through a hole now hit its fan
        t1, f1 = hp.raycast(capi.ray_frame(), dirs, org, 0.0, 100.0)
        t2, f2 = other.raycast(capi.ray_frame(), dirs, org, 0.0, 100.0)
        assert t1.tobytes() == t2.tobytes() and f1.tobytes() == f2.tobytes() and (f1 >= len(faces)).sum() > 10
        old = f1 < len(faces)
        assert np.array_equal(f1[old], f0[old]) and t1[old].tobytes() == t0[old].tobytes() and (f0[~old] < 0).sum() > 10   # new faces only add hits
        assert hp.raycast_points(0.05).tobytes() == other.raycast_points(0.05).tobytes()
        c1, c2 = hp.closest_points(pts, 5.0), other.closest_points(pts, 5.0)
        assert all(c1[k_].tobytes() == c2[k_].tobytes() for k_ in c1) and (c1["face"] >= len(faces)).sum() > 10
        s1, s2 = hp.mesh_sample(300.0, 7), other.mesh_sample(300.0, 7)
        assert len(s1[0]) > 500 and s1[0].tobytes() == s2[0].tobytes() and s1[1].tobytes() == s2[1].tobytes()
        # its analysis and the invariant
        after, fresh = _analysis(hp), _analysis(other)
        _same_analysis(after, fresh)
        _same_analysis(after, tc.analyse(vtx, closed))
        a = after["stats"]
        assert a["n_boundary"] == before["n_boundary"] - E and a["n_boundary_loops"] == before["n_boundary_loops"] - k
        assert a["n_edges"] == before["n_edges"] + E - 3 * k and a["n_counting"] == before["n_counting"] + E - 2 * k and a["euler"] == before["euler"] + k
        assert all(a[n] == before[n] for n in ("n_nonmanifold", "n_inconsistent", "n_vertices_used")) and a["n_components"] <= before["n_components"]
        # a second pass fills nothing
        again = _device(hp, 12)
        _same(again, hc.holes(vtx, closed, 12))
        assert again["stats"]["n_filled"] == 0 and again["stats"]["n_loops"] == ref["stats"]["n_loops"] - k
    finally:
        other.close()


def test_orient_apply_then_holes_on_a_flipped_sheet(hp):
    rng = np.random.default_rng(12)
    vtx, faces = tc.sheet_with_fragments(rng, 20, 20, 30, 0)                           # the sheet alone: one patch
    ref = _check(hp, vtx, faces, 12)
    flipped = oc.flip_random(rng, faces)[0]
    before = _check(hp, vtx, flipped, 12)
    assert before["stats"]["n_nonsimple"] > ref["stats"]["n_nonsimple"] and before["stats"]["n_filled"] < ref["stats"]["n_filled"]
    hp.topology_orient(oc.ORIENT_FIRST)
    oriented = hp.topology_orient_faces()["faces"]
    hp.topology_orient_apply()
    hp.topology_analyse()
    after = _device(hp, 12)
    _same(after, hc.holes(vtx, oriented, 12))
    assert after["stats"] == ref["stats"] and all(np.array_equal(after[k], ref[k]) for k in ("first_vertex", "n_edges", "status", "box", "cycle_start"))
    mirrored = not np.array_equal(oriented[0], faces[0])                               # FIRST keeps face 0 as it was flipped, and the patch follows
    for l in np.nonzero(ref["cycle_start"] >= 0)[0]:
        a = ref["cycle"][ref["cycle_start"][l]:ref["cycle_start"][l] + ref["n_edges"][l]]
        b = after["cycle"][ref["cycle_start"][l]:ref["cycle_start"][l] + ref["n_edges"][l]]
        assert a[0] == b[0] and np.array_equal(a[1:], b[1:][::-1] if mirrored else b[1:])


# ---- the live mesh ---------------------------------------------------------------------------------------------------------------------------------------------
def test_live_mesh_filled_without_side_effects():
    """a fills the holes of its snapshot of the live mesh and applies, b never does: a's answers equal the checker on the exported arrays, and both
    contexts go on to the same mesh and plane table"""
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
                return
            down = synth.voxel_grid_downsample(raw, 0.4)
            prior = capi.make_state(R=R, t=t + np.array([0.01, 0.0, -0.01]), cov_diag=1e-5)
            sa, ia = a.process_scan(down, raw, prior, prior, frame_idx=k, do_mesh=True)
            sb, ib = b.process_scan(down, raw, prior, prior, frame_idx=k, do_mesh=True)
            assert ia == ib and np.array_equal(sa, sb)

        for k in range(4):
            scan(k)
        nv, nf, _ = a.raycast_build_mesh(1.0, 20)
        vtx, faces = a.mesh_export(1.0, 20)
        assert (nv, nf) == (len(vtx), len(faces)) and nf > 1000
        planes, counters = a.dump_planes(), a.counters()
        a.topology_analyse()
        ref = hc.holes(vtx, faces, 16, 2.0)
        _same(_device(a, 16, 2.0), ref, "live mesh")
        st = ref["stats"]
        print("live mesh: %d faces, %d loops: %d simple (largest %d edges), %d not simple; %d outlines, %d too long, %d too wide, %d blocked, %d filled "
              "by %d new faces; holes %.3f ms" % (nf, st["n_loops"], st["n_simple"], st["largest_simple_loop_edges"], st["n_nonsimple"], st["n_outline"],
                                                  st["n_too_long"], st["n_too_wide"], st["n_blocked"], st["n_filled"], st["n_new_faces"],
                                                  a.topology_holes_timing()[0]))
        a.topology_holes_apply()
        _same_analysis(_analysis(a), tc.analyse(vtx, hc.closed(faces, ref)), "the closed snapshot")
        assert compare_plane_tables_fast(planes, a.dump_planes(), 0.0) > 100 and a.counters() == counters
        for k in range(4, 6):
            scan(k)
        ea, eb = a.mesh_export(1.0, 20), b.mesh_export(1.0, 20)
        assert len(ea[1]) != len(faces) and ea[0].tobytes() == eb[0].tobytes() and ea[1].tobytes() == eb[1].tobytes()
        assert compare_plane_tables_fast(a.dump_planes(), b.dump_planes(), 0.0) > 100
    finally:
        a.close(); b.close()


# ---- scale -------------------------------------------------------------------------------------------------------------------------------------------------------
def test_scale(hp):
    """the 320 x 320 sheet with 300 holes plus 2 000 fragments, faces shuffled: about 209 000 faces"""
    rng = np.random.default_rng(51)
    vtx, faces = tc.sheet_with_fragments(rng, 320, 320, 300, 2000)
    assert len(faces) > 200000
    ref = _check(hp, vtx, faces, 16)
    print("%d faces, %d loops: holes %.3f ms (the analysis before it %.3f ms)" % (len(faces), ref["stats"]["n_loops"], hp.topology_holes_timing()[0],
                                                                                 hp.topology_timing()[0]))
    st = ref["stats"]
    assert st["n_loops"] > 2000 and st["n_outline"] == 500 and st["n_filled"] >= 280 and st["n_too_long"] == 1 and st["largest_simple_loop_edges"] == 1280
    loops = hp.topology_analyse().n_boundary_loops
    hp.topology_holes(16)
    hp.topology_holes_apply()
    print("apply %.3f ms" % hp.topology_holes_timing()[1])
    assert hp.topology_analyse().n_boundary_loops == loops - st["n_filled"]


# ---- tools/mesh_eval.py --------------------------------------------------------------------------------------------------------------------------------------------
def test_mesh_eval_fills_the_hole(tmp_path, monkeypatch, capsys):
    spec = importlib.util.spec_from_file_location("mesh_eval", os.path.join(ROOT, "tools", "mesh_eval.py"))
    mesh_eval = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mesh_eval)
    vtx, faces = tc.grid_sheet(4, 4, holes=[(1, 1), (1, 2), (2, 1), (2, 2)], scale=0.5)   # a 2 x 2 sheet without its middle quarter
    rng = np.random.default_rng(3)
    cloud = np.concatenate([rng.uniform(0, 2, (8000, 2)), np.zeros((8000, 1))], axis=1).astype(np.float32)
    np.save(tmp_path / "cloud.npy", cloud)
    _write_ply(tmp_path / "holed.ply", vtx, faces)
    _write_ply(tmp_path / "whole.ply", *tc.grid_sheet(4, 4, scale=0.5))

    def run(ply, *more):
        out = tmp_path / "out.json"
        monkeypatch.setattr(sys, "argv", ["mesh_eval.py", "--cloud", str(tmp_path / "cloud.npy"), "--ply", str(tmp_path / ply), "--out", str(out)] + list(more))
        mesh_eval.main()
        printed = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
        res = json.load(open(out))
        assert printed == res
        return res

    plain = run("holed.ply")
    assert "holes" not in plain and list(plain) == ["tau", "max_dist", "density", "seed", "samples", "cloud_points", "cloud_points_indexed", "accuracy",
                                                    "completeness", "chamfer", "precision", "recall", "f_score", "mesh"]   # the option off: the output as it was
    filled = run("holed.ply", "--fill-holes", "8", "--topology")
    whole = run("whole.ply")
    assert filled["holes"] == dict(max_edges=8, max_diagonal=0.0, n_loops=2, n_simple=2, n_nonsimple=0, n_outline=0, n_too_long=1, n_too_wide=0, n_blocked=0,
                                   n_filled=1, n_new_faces=6, n_edges_closed=8, largest_simple_loop_edges=16, n_cycle_vertices=24)
    assert filled["mesh"]["faces"] == plain["mesh"]["faces"] + 6 and filled["topology"]["n_boundary_loops"] == 1 and filled["topology"]["euler"] == 1
    # the ground-truth points over the hole find the mesh again: the figure the tool calls recall rises to the whole sheet's, and the accuracy with it
    # completeness rises: the fan is sampled too, and every sample lies on the cloud's plane.  The ground-truth points over the hole find the mesh
    # again: recall rises to the whole sheet's, and the accuracy's mean distance falls
    assert filled["completeness"]["within_tau"] > plain["completeness"]["within_tau"] and filled["completeness"]["points"] == filled["samples"] > plain["samples"]
    assert plain["recall"] < 0.85 and filled["recall"] == whole["recall"] == 1.0 and filled["accuracy"]["mean"] < plain["accuracy"]["mean"]
    limited = run("holed.ply", "--fill-holes", "8", "--fill-max-diagonal", "1.0")
    assert limited["holes"]["n_too_wide"] == 1 and limited["holes"]["n_filled"] == 0 and limited["mesh"] == plain["mesh"] and limited["recall"] == plain["recall"]
    with pytest.raises(SystemExit):
        run("holed.ply", "--fill-max-diagonal", "1.0")
    capsys.readouterr()
