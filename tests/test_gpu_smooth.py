"""The one-ring table, the smoothing and the vertex normals on the device (include/immesh_smooth.h) against the numpy restatement of the contract
(tests/smooth_checker.py), bit for bit on every output: the stats, vtx_out as bits, the classes, the three adjacency arrays and the normals as bits.
Strips and sheets at the sizes where a launch gains a wavefront or a workgroup, a row a lane must walk, the sum that depends on its order, the hold,
vertices that are not finite, fins and duplicate faces, nothing to do, order-freedom, the apply against a caster freshly built from the result, every
error and capacity path, the live mesh as a snapshot without side effects, tools/mesh_eval.py's --smooth, tools/mesh_smooth.py, and scale."""
import ctypes as C
import importlib.util
import itertools
import json
import os
import sys
import time

import numpy as np
import pytest

import simplify_checker as sc
import smooth_checker as sm
import topology_checker as tc
from immesh_amd import capi, synth
from conftest import make_hip
from parity_utils import compare_plane_tables_fast
from test_gpu_render import _small_cfg
from test_gpu_topology import _device as _analysis, _same as _same_analysis, _write_ply

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BORDERS = (sm.FIXED, sm.ALONG, sm.FREE)
TAUBIN = (0.5, -0.53)


@pytest.fixture(scope="module")
def hp():
    h = make_hip(capi.load_hip_library(), _small_cfg())
    yield h
    h.close()


def _err(h):
    f = h.lib.immesh_last_error; f.restype = C.c_char_p; f.argtypes = [C.c_void_p]
    return f(h.ctx)


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _device(h, n_steps=0, lam=0.5, mu=-0.53, border=sm.FIXED):
    """the pass, then every fetch, in the checker's shape"""
    st = h.smooth(n_steps, lam, mu, border)
    out = {"stats": {n: getattr(st, n) for n in sm.STAT_NAMES}}
    got = h.smooth_vertices()
    out.update(vtx_out=got["vtx"], vclass=got["vclass"])
    out.update(h.smooth_adjacency())
    return out


def _same_normals(h, vtx, faces, what=""):
    got, ref = h.vertex_normals(), sm.normals(vtx, faces)
    assert got[0].dtype == np.float32 and got[0].tobytes() == ref[0].tobytes() and got[1] == ref[1], (what, got[1], ref[1])
    return ref


def _check(h, vtx, faces, n_steps=0, lam=0.5, mu=-0.53, border=sm.FIXED, what="", build=True):
    """build, and the pass against the checker -> the checker's result"""
    if build:
        h.raycast_build_triangles(vtx, faces)
    ref = sm.smooth(vtx, faces, n_steps, lam, mu, border)
    sm.same(_device(h, n_steps, lam, mu, border), ref, (what, n_steps, lam, mu, border))
    return ref


def _all_modes(h, vtx, faces, what="", steps=(0, 1, 2, 5), factors=TAUBIN):
    h.raycast_build_triangles(vtx, faces)
    _same_normals(h, vtx, faces, what)
    return [_check(h, vtx, faces, n, factors[0], factors[1], border, what, build=False) for border in BORDERS for n in steps]


# ---- sizes where a launch gains a wavefront or a workgroup ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 10, 11, 42, 43])
def test_strips_and_sheets_with_n_faces(hp, n):
    """6 n pairs: 60 and 66 either side of a wavefront, 252 and 258 either side of a workgroup"""
    rng = np.random.default_rng(n)
    vtx, faces = tc.strip(n)
    _all_modes(hp, sm.noisy(rng, vtx, 0.05), faces, ("strip", n))
    vtx, faces = tc.grid_sheet(3, (n + 5) // 6)
    _all_modes(hp, sm.noisy(rng, vtx, 0.05), faces[rng.permutation(len(faces))[:n]], ("sheet", n))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_strips_with_n_vertices(hp, n):
    rng = np.random.default_rng(n)
    vtx, faces = tc.strip(n - 2) if n >= 3 else (np.zeros((n, 3), np.float32), np.zeros((1, 3), np.int32))   # one vertex: a face that does not count
    assert len(vtx) == n
    refs = _all_modes(hp, sm.noisy(rng, vtx, 0.05), faces, ("strip of n vertices", n))
    assert refs[0]["stats"]["n_used"] == (n if n >= 3 else 0)


# ---- rows and their walks -------------------------------------------------------------------------------------------------------------------------------
def test_a_fan_of_valence_three_hundred_beside_five_hundred_small_rings(hp):
    vtx, faces = sm.fan_beside_rings(np.random.default_rng(77))
    for ref in _all_modes(hp, vtx, faces, steps=(0, 3)):
        assert ref["stats"]["max_valence"] == 300 and ref["stats"]["n_used"] == 301 + 4 * 500
    sm.check_facts(vtx, faces, ref)


def test_the_sum_that_depends_on_the_order_of_its_neighbours_and_the_hold(hp):
    got = set()
    for order in itertools.permutations(range(3)):
        vtx, faces = sm.closed_fan(0.0, [sc.ORDER_TRIPLE[i] for i in order])
        ref = _check(hp, vtx, faces, 1, 1.0, 1.0, sm.FREE, what=order)
        assert ref["stats"]["n_moving"] == 4
        got.add(int(ref["vtx_out"][0, 0].view(np.uint32)))
    assert len(got) == 2
    vtx, faces = sm.closed_fan(3e38, (-3e38, -3e38, -3e38))
    ref = _check(hp, vtx, faces, 1, -1.0, -1.0, sm.FREE)
    assert ref["stats"]["n_held"] == 4 and ref["vtx_out"].tobytes() == vtx.tobytes()
    ref = _check(hp, vtx, faces, 5, -1.0, 1.0, sm.FREE)                                 # held on the even steps, moving on the odd ones
    assert ref["stats"]["n_held"] > 0 and np.isfinite(ref["vtx_out"]).all()
    vtx, faces = sm.closed_fan(-0.0, (1.0, 2.0, 3.0))
    ref = _check(hp, vtx, faces, 1, 0.0, 0.0, sm.FREE)                                  # w == 0: -0 becomes +0
    assert ref["stats"]["n_moved"] == 1 and not np.signbit(ref["vtx_out"][0, 0])


def test_vertices_that_are_not_finite_as_neighbours_as_centres_and_unused(hp):
    rng = np.random.default_rng(9)
    vtx, faces = tc.grid_sheet(7, 6)
    vtx = np.concatenate([sm.noisy(rng, vtx, 0.05), [[np.nan, 0, 0], [np.inf, 1, 1], [-0.0, -0.0, -0.0]]]).astype(np.float32)   # three unused ones behind
    for k, bad in enumerate((np.nan, np.inf, -np.inf, -0.0)):
        vtx[9 + 7 * k, k % 3] = bad                                                     # interior vertices
        vtx[k + 1, (k + 1) % 3] = bad                                                   # border vertices
    for ref in _all_modes(hp, vtx, faces, steps=(0, 1, 4)):
        assert ref["stats"]["n_not_finite"] == 6 and ref["stats"]["n_used"] == 56
        assert ref["vtx_out"][ref["vclass"] <= sm.NOT_FINITE].tobytes() == vtx[ref["vclass"] <= sm.NOT_FINITE].tobytes()
    for case in range(6):
        v, f = tc.random_soup(rng, 60, 14)
        _all_modes(hp, sm.with_specials(rng, v, 4), f, ("soup with specials", case), steps=(0, 3), factors=(0.63, -0.67))


def test_duplicate_faces_fins_faces_that_do_not_count_and_zero_faces(hp):
    vtx, faces = sm.fins()
    refs = _all_modes(hp, vtx, faces)
    ref = refs[0]
    assert sorted(set(ref["uses"].tolist())) == [1, 2, 3, 4] and ref["vclass"][18] == sm.UNUSED and ref["stats"]["n_used"] == 18
    sm.check_facts(vtx, faces, ref)
    along = refs[len(refs) // 3 + 1]                                                    # ALONG, one step: vertex 4 follows the fin's foot, its end and the faces given twice
    assert along["stats"]["n_steps"] == 1 and along["vclass"][4] == sm.BORDER
    rs = along["row_start"]
    fin = [(int(u), int(n)) for u, n in zip(along["neighbours"][rs[4]:rs[5]], along["uses"][rs[4]:rs[5]]) if n != 2]
    assert fin == [(0, 4), (3, 4), (7, 3), (15, 1)]
    want = (((vtx[0].astype(np.float64) + vtx[3]) + vtx[7]) + vtx[15]) / 4.0
    assert along["vtx_out"][4].tolist() == (vtx[4] + 0.5 * (want - vtx[4].astype(np.float64))).astype(np.float32).tolist() == [1.0, 0.75, 0.125]
    rng = np.random.default_rng(2)
    for case in range(6):                                                               # random index triples: long runs of equal pairs
        v, f = tc.random_soup(rng, 300, 12)
        _all_modes(hp, v, f, ("soup", case), steps=(0, 3))
    vtx = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    for faces in (np.zeros((0, 3), np.int32), np.array([[0, 0, 1], [2, 2, 2]], np.int32)):
        for ref in _all_modes(hp, vtx, faces, steps=(0, 2)):
            assert ref["stats"] == dict(dict.fromkeys(sm.STAT_NAMES, 0), n_vertices=3, n_steps=ref["stats"]["n_steps"])
        assert hp.vertex_normals()[1] == 3
        hp.smooth(2)
        hp.smooth_apply()
        assert hp._raycast_sizes()[:2] == (3, len(faces))                               # (a face that does not count still has a box in the hierarchy)


def test_moebius_and_torus(hp):
    rng = np.random.default_rng(3)
    for vtx, faces in (tc.moebius(17), tc.torus(12, 7)):
        vtx = sm.noisy(rng, vtx, 0.03)
        for ref in _all_modes(hp, vtx, faces[rng.permutation(len(faces))], steps=(0, 1, 6)):
            sm.check_facts(vtx, faces, ref)
    assert ref["stats"]["n_border"] == 0 and ref["stats"]["max_valence"] == 6


# ---- order-freedom -------------------------------------------------------------------------------------------------------------------------------------------
def test_two_runs_a_permutation_of_the_faces_and_a_relabelling_of_the_vertices(hp):
    rng = np.random.default_rng(17)
    vtx, faces = tc.sheet_with_fragments(rng, 40, 30, 60, 40)
    vtx = sm.noisy(rng, vtx, 0.01)
    for border in BORDERS:
        ref = _check(hp, vtx, faces, 4, 0.5, -0.53, border)
        normals = _same_normals(hp, vtx, faces)
        sm.same(_device(hp, 4, 0.5, -0.53, border), _device(hp, 4, 0.5, -0.53, border), "two runs")
        per = _check(hp, vtx, faces[rng.permutation(len(faces))], 4, 0.5, -0.53, border)
        sm.same(per, ref, "the faces permuted")                                         # no output is indexed by face
        sv, sf, perm = sc.relabel(rng, vtx, faces)
        rel = _check(hp, sv, sf, 4, 0.5, -0.53, border)
        for k in ("n_vertices", "n_used", "n_not_finite", "n_border", "n_interior", "n_moving", "n_pairs", "max_valence", "n_steps", "n_held"):
            assert rel["stats"][k] == ref["stats"][k], k
        assert np.array_equal(rel["vclass"][perm], ref["vclass"]) and np.array_equal(np.diff(rel["row_start"])[perm], np.diff(ref["row_start"]))
        # the sums run in another order: a double sum of six floats moves by 2^-50 of its size, which can turn the float rounding of a step by one
        # last bit; a step passes an error e on as at most (|1 - w| + |w|) e, 1 e for 0.5 and 2.06 e for -0.53, so four steps stay below
        # ((1 * 2.06 + 1) + 1) * 2.06 + 1 < 10 last bits of the coordinate's largest magnitude
        tol = 10 * np.spacing(np.abs(ref["vtx_out"]).max(axis=0)).astype(np.float64)
        assert (np.abs(rel["vtx_out"][perm].astype(np.float64) - ref["vtx_out"]) <= tol).all()
        still = ref["vclass"] <= sm.NOT_FINITE
        assert rel["vtx_out"][perm][still].tobytes() == ref["vtx_out"][still].tobytes()
    assert normals[1] == 0


# ---- the apply ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("border", BORDERS)
def test_apply_equals_a_fresh_build_from_the_result(hp, border):
    rng = np.random.default_rng(31)
    vtx, faces = tc.sheet_with_fragments(rng, 30, 20, 40, 40)
    vtx = sm.noisy(rng, vtx, 0.01)
    dirs = (rng.normal(size=(2000, 3)) * np.array([0.3, 0.3, 1.0])).astype(np.float32)
    org = (rng.uniform(0.0, 1.0, (2000, 3)) * np.array([1.5, 1.0, 0.0]) + np.array([0.0, 0.0, 1.0])).astype(np.float32)
    dirs[:, 2] = -np.abs(dirs[:, 2]) - 0.5
    pts = np.concatenate([rng.uniform(-0.2, 1.7, (3000, 2)), rng.normal(scale=0.2, size=(3000, 1))], axis=1).astype(np.float32)
    other = make_hip(capi.load_hip_library(), _small_cfg())
    try:
        ref = _check(hp, vtx, faces, 5, 0.5, -0.53, border)
        assert ref["stats"]["n_moved"] > 300
        before = _same_normals(hp, vtx, faces)
        hp.raycast(capi.ray_frame(), dirs, org, 0.0, 100.0)
        assert hp.mesh_sample(300.0, 7, fetch=False) > 100 and len(hp.raycast_points(0.05)) > 100   # samples and a cast's points: the apply discards both
        _same_analysis(_analysis(hp), tc.analyse(vtx, faces))
        sm.same(dict(stats=ref["stats"], vtx_out=hp.smooth_vertices()["vtx"], vclass=hp.smooth_vertices()["vclass"], **hp.smooth_adjacency()), ref,
                "an analysis leaves the result alone")
        hp.simplify(0.0)                                                                # a simplification's result: the apply discards it
        hp.smooth_apply()
        assert hp.smooth_last_timing()[2] > 0.0
        for call in (hp.smooth_vertices, hp.smooth_adjacency, hp.smooth_apply):
            with pytest.raises(RuntimeError, match=r"rc=-1: .*no smooth pass"):
                call()                                                                  # a fetch after the apply
        with pytest.raises(RuntimeError, match=r"rc=-1: .*no simplify pass"):
            hp.simplify_faces()
        with pytest.raises(RuntimeError, match=r"rc=-1: .*no analysis"):
            hp.topology_faces()
        with pytest.raises(RuntimeError, match=r"rc=-1: .*no NEAREST cast"):
            hp.raycast_points(0.05)
        with pytest.raises(RuntimeError, match=r"rc=-1: .*no samples"):
            hp.nearest_samples(1.0, want=())
        other.raycast_build_triangles(ref["vtx_out"], faces)
        assert hp._raycast_sizes() == other._raycast_sizes() and hp._raycast_sizes()[:2] == (len(vtx), len(faces))
        t1, f1 = hp.raycast(capi.ray_frame(), dirs, org, 0.0, 100.0)
        t2, f2 = other.raycast(capi.ray_frame(), dirs, org, 0.0, 100.0)
        assert t1.tobytes() == t2.tobytes() and f1.tobytes() == f2.tobytes() and (f1 >= 0).sum() > 500
        assert hp.raycast_points(0.05).tobytes() == other.raycast_points(0.05).tobytes()
        c1, c2 = hp.closest_points(pts, 5.0), other.closest_points(pts, 5.0)
        assert all(c1[k].tobytes() == c2[k].tobytes() for k in c1) and (c1["face"] >= 0).all()
        s1, s2 = hp.mesh_sample(300.0, 7), other.mesh_sample(300.0, 7)
        assert len(s1[0]) > 100 and s1[0].tobytes() == s2[0].tobytes() and s1[1].tobytes() == s2[1].tobytes()
        after, fresh = _analysis(hp), _analysis(other)
        _same_analysis(after, fresh)
        _same_analysis(after, tc.analyse(ref["vtx_out"], faces))
        after_normals = _same_normals(hp, ref["vtx_out"], faces)                        # the normals follow the apply
        assert after_normals[0].tobytes() != before[0].tobytes() and other.vertex_normals()[0].tobytes() == after_normals[0].tobytes()
        sm.same(_device(hp, 2, 0.5, 0.5, border), sm.smooth(ref["vtx_out"], faces, 2, 0.5, 0.5, border), "a second pass over the applied result")
    finally:
        other.close()


def test_the_applies_of_orient_holes_and_simplify_and_a_rebuild_discard_a_smooth_result(hp):
    vtx, faces = tc.grid_sheet(6, 5, holes=[(1, 1), (3, 3)])
    fetches = (hp.smooth_vertices, hp.smooth_adjacency, hp.smooth_apply)
    for apply in ("orient", "holes", "simplify", "build"):
        ref = _check(hp, vtx, faces, 2, 0.5, -0.53, sm.ALONG)
        hp.topology_analyse()                                                           # an analysis leaves the result alone
        assert hp.smooth_vertices()["vtx"].tobytes() == ref["vtx_out"].tobytes() and np.array_equal(hp.smooth_adjacency()["uses"], ref["uses"])
        hp.vertex_normals()                                                             # and so do the normals
        assert hp.smooth_vertices()["vtx"].tobytes() == ref["vtx_out"].tobytes()
        if apply == "orient":
            hp.topology_orient(capi.ORIENT_FIRST)
            hp.topology_orient_apply()
        elif apply == "holes":
            hp.topology_holes(8)
            hp.topology_holes_apply()
        elif apply == "simplify":
            hp.simplify(0.0)
            hp.simplify_apply()
        else:
            hp.raycast_build_triangles(vtx, faces)
        for fetch in fetches:
            with pytest.raises(RuntimeError, match=r"rc=-1: .*no smooth pass"):
                fetch()


# ---- the normals -------------------------------------------------------------------------------------------------------------------------------------------------
def test_normals_of_a_flat_sheet_a_cancelled_sum_and_an_oriented_patch(hp):
    vtx, faces = tc.grid_sheet(5, 4, z=0.25, scale=0.3)
    hp.raycast_build_triangles(vtx, faces)
    ref = _same_normals(hp, vtx, faces)
    assert ref[1] == 0 and np.array_equal(ref[0], np.tile(np.array([0, 0, 1], np.float32), (len(vtx), 1)))
    hp.raycast_build_triangles(vtx, faces[:, [0, 2, 1]])
    assert np.array_equal(_same_normals(hp, vtx, faces[:, [0, 2, 1]])[0], np.tile(np.array([0, 0, -1], np.float32), (len(vtx), 1)))
    two = np.array([[0, 1, 2], [0, 2, 1], [2, 1, 3]], np.int32)                         # a face and its mirror image: vertex 0 cancels, 1 and 2 keep the third
    quad = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [5, 5, 5]], np.float32)
    hp.raycast_build_triangles(quad, two)
    ref = _same_normals(hp, quad, two)
    assert ref[1] == 2 and ref[0][[0, 4]].tobytes() == np.zeros((2, 3), np.float32).tobytes() and ref[0][3].tolist() == [0, 0, 1]
    rng = np.random.default_rng(6)                                                      # a torus with a third of its faces wound the other way
    vtx, faces = tc.torus(14, 9)
    vtx = sm.noisy(rng, vtx, 0.01)
    faces = faces.copy()
    flipped = rng.permutation(len(faces))[:len(faces) // 3]
    faces[flipped] = faces[flipped][:, [0, 2, 1]]
    hp.raycast_build_triangles(vtx, faces)
    mixed = _same_normals(hp, vtx, faces)
    hp.topology_analyse()
    assert hp.topology_orient(capi.ORIENT_FEWEST).n_faces_flipped == len(flipped)
    oriented = hp.topology_orient_faces()["faces"]
    hp.topology_orient_apply()
    ref = _same_normals(hp, vtx, oriented)
    assert ((ref[0].astype(np.float64) * sm.torus_normals(14, 9)).sum(axis=1) > 0.9).all() and ref[0].tobytes() != mixed[0].tobytes()
    hp.raycast_build_triangles(vtx, oriented[:, [0, 2, 1]])                             # every face flipped: every sign flipped, bit for bit
    assert hp.vertex_normals()[0].tobytes() == (-ref[0]).tobytes()


# ---- fetches and errors ------------------------------------------------------------------------------------------------------------------------------------------
def test_fetches_lifecycle_and_argument_errors():
    h = make_hip(capi.load_hip_library(), _small_cfg())
    try:
        vtx, faces = tc.grid_sheet(6, 5)
        vtx = sm.noisy(np.random.default_rng(1), vtx, 0.05)
        ref = sm.smooth(vtx, faces, 3, 0.5, -0.53, sm.ALONG)
        nv, n_p = len(vtx), ref["stats"]["n_pairs"]
        assert n_p == 2 * (6 * 6 + 7 * 5 + 30)
        fetches = (h.smooth_vertices, h.smooth_adjacency, h.smooth_apply)
        for call in (h.smooth, h.vertex_normals) + fetches:
            with pytest.raises(RuntimeError, match=r"rc=-1: .*built"):
                call()                                                                  # before a build
        h.raycast_build_triangles(vtx, faces)
        for fetch in fetches:
            with pytest.raises(RuntimeError, match=r"rc=-1: .*no smooth pass"):
                fetch()                                                                 # a fetch or an apply before a pass
        _same_normals(h, vtx, faces)                                                    # the normals need no pass, and are none
        for fetch in fetches:
            with pytest.raises(RuntimeError, match=r"rc=-1: .*no smooth pass"):
                fetch()

        def still_usable():
            sm.same(_device(h, 3, 0.5, -0.53, sm.ALONG), ref)

        still_usable()
        untouched = lambda: h.smooth_vertices()["vtx"].tobytes() == ref["vtx_out"].tobytes()   # refused before anything was touched: the last pass stays
        for bad in (-1, 65537, 2 ** 31 - 1, -2 ** 31):
            with pytest.raises(RuntimeError, match=r"rc=-1: .*n_steps"):
                h.smooth(bad)
            assert untouched()
        for bad in (np.nan, np.inf, -np.inf, 1.0000001, -1.0000001, 1e300):
            for args in ((3, bad, -0.53), (3, 0.5, bad)):
                with pytest.raises(RuntimeError, match=r"rc=-1: .*lambda and mu"):
                    h.smooth(*args)
            assert untouched()
        for bad in (-1, 3, 7, 2 ** 31 - 1):
            with pytest.raises(RuntimeError, match=r"rc=-1: .*border"):
                h.smooth(3, 0.5, -0.53, bad)
            assert untouched()
        assert h.smooth(65536, 1.0, -1.0).n_steps == 65536 and h.smooth(0, -1.0, 1.0).n_steps == 0   # the ends of the ranges are in
        f = h.lib.immesh_smooth; f.argtypes = [C.c_void_p, C.c_int32, C.c_double, C.c_double, C.c_int32, C.c_void_p]
        assert f(None, 3, 0.5, -0.53, 1, None) == -1 and f(h.raycaster(), 3, 0.5, -0.53, 1, None) == 0   # stats may be NULL
        # vertices
        g = h.lib.immesh_smooth_vertices; g.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        assert g(None, None, None) == -1 and g(h.raycaster(), None, None) == 0
        for which, k in enumerate(("vtx_out", "vclass")):
            room = np.zeros((nv + 1,) + ref[k].shape[1:], ref[k].dtype)
            args = [None] * 2
            args[which] = room.ctypes.data_as(C.c_void_p)
            assert g(h.raycaster(), *args) == 0 and room[:nv].tobytes() == ref[k].tobytes() and not room[nv:].any()
        # adjacency
        g = h.lib.immesh_smooth_adjacency; g.argtypes = [C.c_void_p] + [C.c_void_p] * 3 + [C.c_int64, C.c_void_p]
        n = C.c_int64(-5)
        assert g(h.raycaster(), None, None, None, -1, C.byref(n)) == -1 and b"cap" in _err(h)
        assert g(None, None, None, None, 0, None) == -1 and g(h.raycaster(), None, None, None, 0, None) == 0
        assert g(h.raycaster(), None, None, None, 0, C.byref(n)) == 0 and n.value == n_p
        for which, k in enumerate(("row_start", "neighbours", "uses")):
            room = np.zeros(len(ref[k]) + 1, ref[k].dtype)
            args = [None] * 3
            args[which] = room.ctypes.data_as(C.c_void_p)
            n = C.c_int64(-5)
            assert g(h.raycaster(), *args, n_p - 1, C.byref(n)) == -4 and n.value == n_p and b"cap %d < %d" % (n_p - 1, n_p) in _err(h)
            assert not room.any()
            assert g(h.raycaster(), *args, n_p, C.byref(n)) == 0 and n.value == n_p and room[:-1].tobytes() == ref[k].tobytes() and room[-1] == 0
        # normals
        g = h.lib.immesh_vertex_normals; g.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        n = C.c_int64(-5)
        assert g(None, None, None) == -1 and g(h.raycaster(), None, None) == 0 and g(h.raycaster(), None, C.byref(n)) == 0 and n.value == 0
        room = np.zeros((nv + 1, 3), np.float32)
        assert g(h.raycaster(), room.ctypes.data_as(C.c_void_p), None) == 0 and room[:nv].tobytes() == sm.normals(vtx, faces)[0].tobytes() and not room[nv].any()
        a = h.lib.immesh_smooth_apply; a.argtypes = [C.c_void_p]
        assert a(None) == -1
        t = h.lib.immesh_smooth_last_timing; t.argtypes = [C.c_void_p, C.c_void_p]
        assert t(h.raycaster(), None) == -1 and t(None, None) == -1 and h.smooth_last_timing()[0] > 0.0 and h.smooth_last_timing()[1] > 0.0
        still_usable()
        h.raycast_build_triangles(vtx, faces)                                           # a rebuild discards the result
        for fetch in fetches:
            with pytest.raises(RuntimeError, match=r"rc=-1: .*no smooth pass"):
                fetch()
        still_usable()
    finally:
        h.close()


# ---- the live mesh -----------------------------------------------------------------------------------------------------------------------------------------------
def test_live_mesh_smoothed_without_side_effects():
    """a smooths its snapshot of the live mesh and applies, b never does: a's answers equal the checker on the exported arrays, and both contexts go on
    to the same mesh and plane table"""
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
        _same_normals(a, vtx, faces, "live mesh")
        for border in BORDERS:
            ref = sm.smooth(vtx, faces, 10, 0.5, -0.53, border)
            sm.same(_device(a, 10, 0.5, -0.53, border), ref, ("live mesh", border))
        st = ref["stats"]
        print("live mesh: %d vertices, %d faces: %d border, %d interior, valence up to %d, %d moved by up to %.4f; one-ring %.3f ms, 10 steps %.3f ms"
              % (nv, nf, st["n_border"], st["n_interior"], st["max_valence"], st["n_moved"], st["max_disp2"] ** 0.5, *a.smooth_last_timing()[:2]))
        assert st["n_moved"] > 100 and st["n_used"] == st["n_border"] + st["n_interior"]
        a.smooth_apply()
        _same_analysis(_analysis(a), tc.analyse(ref["vtx_out"], faces), "the smoothed snapshot")
        _same_normals(a, ref["vtx_out"], faces, "the smoothed snapshot")
        assert compare_plane_tables_fast(planes, a.dump_planes(), 0.0) > 100 and a.counters() == counters
        for k in range(4, 6):
            scan(k)
        ea, eb = a.mesh_export(1.0, 20), b.mesh_export(1.0, 20)
        assert len(ea[1]) != len(faces) and ea[0].tobytes() == eb[0].tobytes() and ea[1].tobytes() == eb[1].tobytes()
        assert compare_plane_tables_fast(a.dump_planes(), b.dump_planes(), 0.0) > 100
    finally:
        a.close(); b.close()


# ---- the tools ---------------------------------------------------------------------------------------------------------------------------------------------------
def _noisy_cube_sheet(rng, n=12):
    """the six sides of the unit cube as n x n sheets welded along the cube's edges, with noise; a cloud on the cube's sides"""
    vs, fs = [], []
    for axis in range(3):
        for side in (0.0, 1.0):
            v, f = tc.grid_sheet(n, n, scale=1.0 / n)
            v = np.insert(v[:, :2], axis, side, axis=1)
            fs.append(f + sum(len(x) for x in vs))
            vs.append(v)
    vtx, faces = np.concatenate(vs).astype(np.float32), np.concatenate(fs).astype(np.int32)
    welded = sc.simplify(vtx, faces)
    cloud = rng.uniform(0, 1, (6000, 3))
    cloud[np.arange(6000), rng.integers(0, 3, 6000)] = rng.integers(0, 2, 6000)
    return sm.noisy(rng, welded["vtx_out"], 0.01), welded["faces_out"], cloud.astype(np.float32)


def test_mesh_eval_smooths_a_noisy_cube(tmp_path, monkeypatch, capsys):
    mesh_eval = _tool("mesh_eval")
    rng = np.random.default_rng(3)
    vtx, faces, cloud = _noisy_cube_sheet(rng)
    _write_ply(tmp_path / "cube.ply", vtx, faces)
    np.save(tmp_path / "cloud.npy", cloud)

    def run(*more):
        out = tmp_path / "out.json"
        monkeypatch.setattr(sys, "argv", ["mesh_eval.py", "--cloud", str(tmp_path / "cloud.npy"), "--ply", str(tmp_path / "cube.ply"), "--out", str(out)] + list(more))
        mesh_eval.main()
        printed = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
        res = json.load(open(out))
        assert printed == res
        return res

    plain = run()
    assert list(plain) == ["tau", "max_dist", "density", "seed", "samples", "cloud_points", "cloud_points_indexed", "accuracy", "completeness", "chamfer",
                           "precision", "recall", "f_score", "mesh"]                    # the options off: the output as it was
    smooth = run("--smooth", "10")
    assert smooth["smooth"] == dict({"lambda": 0.5, "mu": -0.53, "border": "fixed"}, **sm.smooth(vtx, faces, 10, 0.5, -0.53, sm.FIXED)["stats"])
    assert smooth["mesh"] == plain["mesh"] and list(smooth) == list(plain) + ["smooth"]
    print("noisy cube: accuracy mean %.5f -> %.5f, F-score %.4f -> %.4f after 10 Taubin steps"
          % (plain["accuracy"]["mean"], smooth["accuracy"]["mean"], plain["f_score"], smooth["f_score"]))
    other = run("--smooth", "4", "--smooth-lambda", "0.3", "--smooth-mu", "0.3", "--smooth-border", "free", "--topology")
    assert other["smooth"] == dict({"lambda": 0.3, "mu": 0.3, "border": "free"}, **sm.smooth(vtx, faces, 4, 0.3, 0.3, sm.FREE)["stats"])
    assert other["topology"]["n_components"] == 1 and other["topology"]["euler"] == 2
    none = run("--smooth", "0")
    assert none["smooth"]["n_moved"] == 0 and {k: v for k, v in none.items() if k != "smooth"} == plain
    for bad in (["--smooth-lambda", "0.3"], ["--smooth-mu", "0.3"], ["--smooth-border", "free"], ["--smooth", "-1"], ["--smooth", "3", "--smooth-border", "up"]):
        with pytest.raises(SystemExit):
            run(*bad)
    with pytest.raises(RuntimeError, match=r"lambda and mu"):
        run("--smooth", "3", "--smooth-lambda", "2")
    capsys.readouterr()


def test_mesh_smooth_writes_the_checkers_vertices_and_normals(tmp_path, monkeypatch, capsys):
    mesh_smooth = _tool("mesh_smooth")
    rng = np.random.default_rng(5)
    vtx, faces, _ = _noisy_cube_sheet(rng, 6)
    _write_ply(tmp_path / "in.ply", vtx, faces)
    ref = sm.smooth(vtx, faces, 6, 0.5, -0.53, sm.ALONG)
    monkeypatch.setattr(sys, "argv", ["mesh_smooth.py", str(tmp_path / "in.ply"), str(tmp_path / "out.ply"), "--steps", "6", "--border", "along", "--normals"])
    mesh_smooth.main()
    printed = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert {k: printed[k] for k in sm.STAT_NAMES} == ref["stats"] and printed["n_zero_normals"] == 0
    v, n, f = mesh_smooth.read_ply_normals(tmp_path / "out.ply")
    assert v.tobytes() == ref["vtx_out"].tobytes() and np.array_equal(f, faces) and n.tobytes() == sm.normals(ref["vtx_out"], faces)[0].tobytes()
    monkeypatch.setattr(sys, "argv", ["mesh_smooth.py", str(tmp_path / "in.ply"), str(tmp_path / "plain.ply"), "--steps", "6", "--border", "along"])
    mesh_smooth.main()
    capsys.readouterr()
    v, f = _tool("mesh_eval").read_ply(tmp_path / "plain.ply")                          # without --normals: the layout immesh_save_ply writes
    assert v.tobytes() == ref["vtx_out"].tobytes() and np.array_equal(f, faces)


# ---- scale -----------------------------------------------------------------------------------------------------------------------------------------------------------
def test_scale(hp):
    """a 316 x 316 sheet, about 200 000 faces, noisy, the faces and the vertex indices shuffled: 10 Taubin steps and the normals"""
    rng = np.random.default_rng(51)
    vtx, faces = tc.grid_sheet(316, 316, scale=0.05)
    vtx, faces, _ = sc.relabel(rng, sm.noisy(rng, vtx, 0.01), faces[rng.permutation(len(faces))])
    assert len(faces) == 199712 and len(vtx) == 317 * 317
    t0 = time.perf_counter()
    ref = _check(hp, vtx, faces, 10, 0.5, -0.53, sm.ALONG)
    ms = hp.smooth_last_timing()
    t1 = time.perf_counter()
    _same_normals(hp, vtx, faces)
    print("%d vertices, %d faces: one-ring %.3f ms, 10 steps %.3f ms, normals with their copy %.1f ms wall" % (len(vtx), len(faces), ms[0], ms[1], (time.perf_counter() - t1) * 1e3))
    st = ref["stats"]
    assert st["n_pairs"] == 2 * (3 * 316 * 316 + 2 * 316) and st["max_valence"] == 6 and st["n_border"] == 4 * 316 and st["n_moving"] == len(vtx) and st["n_held"] == 0
    hp.smooth_apply()
    assert hp.topology_analyse().n_components == 1
    print("the checker and the device together: %.1f s" % (time.perf_counter() - t0))
