"""The manifold pass on the device (include/immesh_topology.h, the Manifold rule) against the numpy restatement of the contract
(tests/manifold_checker.py), bit for bit on every output: the stats, the fans per vertex, the fan tables, fan_out and faces_out, the new vertices'
sources and bits.  The CPU tier's closed forms and soups; one vertex with many fans and one fan with many faces at the sizes where the launches gain
a wavefront or a workgroup and the scans a block; order-freedom; every fetch and error; the apply against a caster freshly built from
(vtx_out, faces_out); the chain split, orient, holes; the live mesh as a snapshot without side effects; the tools; scale."""
import ctypes as C
import importlib.util
import json
import os
import sys

import numpy as np
import pytest

import holes_checker as hc
import manifold_checker as mc
import orient_checker as oc
import topology_checker as tc
from immesh_amd import capi, synth
from conftest import make_hip
from parity_utils import compare_plane_tables_fast
from test_gpu_render import _small_cfg
from test_gpu_topology import _device as _analysis, _same as _same_analysis, _write_ply

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARRAYS = (("n_fans_out", np.int32),) + tuple((k, np.int32) for k in mc.TABLES) + (("fan_out", np.int32), ("faces_out", np.int32), ("vsrc", np.int32),
                                                                                  ("xyz", np.float32))
SIZES = (2, 63, 64, 65, 255, 256, 257, 300, 4097)


@pytest.fixture(scope="module")
def hp():
    h = make_hip(capi.load_hip_library(), _small_cfg())
    yield h
    h.close()


def _err(h):
    f = h.lib.immesh_last_error; f.restype = C.c_char_p; f.argtypes = [C.c_void_p]
    return f(h.ctx)


def _device(h):
    """the pass, then every fetch, in the checker's shape"""
    st = h.topology_manifold()
    out = {"stats": {n: getattr(st, n) for n in mc.STAT_NAMES}, "n_fans_out": h.topology_manifold_vertices()}
    out.update(h.topology_manifold_fans())
    out["fan_out"], out["faces_out"] = h.topology_manifold_faces()
    out["vsrc"], out["xyz"] = h.topology_manifold_new_vertices()
    return out


def _same(got, ref, what=""):
    assert got["stats"] == ref["stats"], (what, got["stats"], ref["stats"])
    for k, t in ARRAYS:
        assert got[k].dtype == ref[k].dtype == t and got[k].shape == ref[k].shape, (what, k, got[k].shape, ref[k].shape)
        assert got[k].tobytes() == ref[k].tobytes(), (what, k, got[k][:12], ref[k][:12])                  # the new vertices by their bits


def _check(h, vtx, faces, what="", ref=None):
    """build, analyse, and the pass against the checker -> the checker's result"""
    h.raycast_build_triangles(vtx, faces)
    st = h.topology_analyse()
    ref = mc.manifold(vtx, faces) if ref is None else ref
    _same(_device(h), ref, what)
    assert ref["stats"]["n_nonmanifold_before"] == st.n_nonmanifold and ref["stats"]["n_vertices_used"] == st.n_vertices_used
    return ref


# ---- the CPU tier's shapes ---------------------------------------------------------------------------------------------------------------------------
def test_closed_forms_on_the_device(hp):
    assert _check(hp, *mc.faces_on_a_vertex(1))["stats"]["n_fans"] == 3
    assert _check(hp, *mc.faces_on_a_vertex(2))["faces_out"].tolist() == [[0, 1, 2], [5, 3, 4]]
    assert _check(hp, *mc.two_tetrahedra(1))["stats"]["n_new_vertices"] == 1
    ref = _check(hp, *mc.two_tetrahedra(2))
    assert (ref["stats"]["n_new_vertices"], ref["stats"]["n_closed_fans"], ref["stats"]["n_open_fans"], ref["stats"]["n_nonmanifold_before"]) == (2, 4, 4, 1)
    assert _check(hp, *mc.fin_on_a_sheet())["faces_out"][-1].tolist() == [17, 18, 16]
    assert _check(hp, *mc.faces_on_an_edge(3))["faces_out"].tolist() == [[0, 1, 2], [5, 7, 3], [6, 8, 4]]
    assert _check(hp, *hc.touching_holes())["vsrc"].tolist() == [12]
    assert _check(hp, *mc.pinched_sheet())["vsrc"].tolist() == [5]
    for soup, closed, opened in ((tc.torus(5, 4), 20, 0), (tc.moebius(9), 0, 18), (mc.pillow(), 3, 0), (oc.klein(4, 5), 20, 0)):
        ref = _check(hp, *soup)
        assert (ref["stats"]["n_closed_fans"], ref["stats"]["n_open_fans"], ref["stats"]["n_corners_moved"]) == (closed, opened, 0)
        assert np.array_equal(ref["faces_out"], soup[1])


def test_faces_that_do_not_count_unused_vertices_and_bit_copies_on_the_device(hp):
    vtx, faces = mc.faces_on_a_vertex(3)
    vtx = np.concatenate([vtx, np.ones((2, 3), np.float32)])
    faces = np.concatenate([[[0, 0, 1]], faces[:2], [[7, 2, 2]], faces[2:], [[0, 8, 0]]]).astype(np.int32)
    vtx.view(np.uint32)[0] = [0x7FC12345, 0x80000000, 0xFFC00001]                       # a NaN with a payload, -0, a negative NaN with another
    ref = _check(hp, vtx, faces)
    assert ref["xyz"].view(np.uint32).tolist() == [[0x7FC12345, 0x80000000, 0xFFC00001]] * 2 and ref["n_fans_out"].tolist() == [3, 1, 1, 1, 1, 1, 1, 0, 0]
    assert ref["fan_out"][[0, 3, 5]].tolist() == [[-1] * 3] * 3


@pytest.mark.parametrize("group", range(4))
def test_random_soups_match_checker(hp, group):
    most = 0
    for case in range(11 * group, 11 * group + 11):                                     # the CPU tier's 44 soups
        rng = np.random.default_rng(9000 + case)
        vtx, faces = tc.random_soup(rng, int(rng.integers(1, 201)), int(rng.integers(5, 31)))
        ref = _check(hp, vtx, faces, what=case)
        most = max(most, ref["stats"]["most_fans_at_vertex"])
    assert most >= 3


# ---- one vertex with many fans, one fan with many faces ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", SIZES)
def test_faces_that_share_only_a_vertex(hp, k):
    vtx, faces = mc.faces_on_a_vertex(k)
    ref = _check(hp, vtx, faces, what=k)
    assert ref["stats"] == dict(n_corners=3 * k, n_fans=3 * k, n_vertices_used=2 * k + 1, n_singular_vertices=1, most_fans_at_vertex=k, n_new_vertices=k - 1,
                                n_corners_moved=k - 1, n_faces_changed=k - 1, n_closed_fans=0, n_open_fans=3 * k, largest_fan_corners=1, n_nonmanifold_before=0)
    assert ref["faces_out"][1:, 0].tolist() == list(range(2 * k + 1, 3 * k)) and (ref["vsrc"] == 0).all()
    sv, sf, perm = hc.relabel(np.random.default_rng(k), vtx, faces)                     # the singular vertex anywhere among the others
    moved = _check(hp, sv, sf, what=(k, "relabelled"))
    assert moved["stats"] == ref["stats"] and (moved["vsrc"] == perm[0]).all() and moved["n_fans_out"][perm[0]] == k


@pytest.mark.parametrize("closed", [False, True])
@pytest.mark.parametrize("k", SIZES)
def test_disc_round_one_vertex(hp, k, closed):
    if closed and k < 3:
        k = 3                                                                           # the smallest closed disc
    vtx, faces = mc.disc(k, closed)
    faces = faces[np.random.default_rng(k).permutation(k)]                              # the unions arrive in no order
    ref = _check(hp, vtx, faces, what=(k, closed))
    assert ref["stats"]["n_new_vertices"] == 0 and ref["stats"]["largest_fan_corners"] == k and np.array_equal(ref["faces_out"], faces)
    assert (ref["n_corners"][0], ref["n_links"][0]) == (k, k if closed else k - 1) and ref["stats"]["n_closed_fans"] == (1 if closed else 0)


def test_many_faces_on_one_edge_copies_of_one_face_degenerate_faces_and_none(hp):
    ref = _check(hp, *mc.faces_on_an_edge(300))
    assert ref["stats"]["n_new_vertices"] == 2 * 299 and ref["stats"]["most_fans_at_vertex"] == 300 and ref["stats"]["n_nonmanifold_before"] == 1
    vtx = mc.faces_on_a_vertex(1)[0]
    ref = _check(hp, vtx, np.tile(np.array([[0, 1, 2]], np.int32), (300, 1)))           # every edge has 300 uses: 300 lone faces afterwards
    assert ref["stats"]["n_new_vertices"] == 3 * 299 and ref["stats"]["n_nonmanifold_before"] == 3 and ref["faces_out"][299].tolist() == [301, 600, 899]
    zero = dict.fromkeys(mc.STAT_NAMES, 0)
    degenerate = np.array([[0, 0, 1], [2, 2, 2], [1, 0, 1]] * 30, np.int32)
    ref = _check(hp, vtx, degenerate)
    assert ref["stats"] == zero and np.array_equal(ref["faces_out"], degenerate) and (ref["fan_out"] == -1).all()
    hp.topology_manifold_apply()                                                       # nothing to move: a rebuild of the same soup
    assert hp._raycast_sizes()[:2] == (3, 90)
    ref = _check(hp, vtx, np.zeros((0, 3), np.int32))
    assert ref["stats"] == zero and ref["n_fans_out"].tolist() == [0, 0, 0]
    hp.topology_manifold_apply()
    assert hp._raycast_sizes()[:2] == (3, 0)
    ref = _check(hp, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    assert ref["stats"] == zero
    hp.topology_manifold_apply()
    assert hp._raycast_sizes()[:2] == (0, 0)


def test_strips_of_one_to_257_faces(hp):
    for n in range(1, 258):
        vtx, faces = tc.strip(n)
        ref = _check(hp, vtx, faces, what=n)
        assert ref["stats"]["n_fans"] == n + 2 and ref["stats"]["n_new_vertices"] == 0 and ref["stats"]["largest_fan_corners"] == min(n, 3)


# ---- order-freedom -------------------------------------------------------------------------------------------------------------------------------------
def _partition(res, face_of=None, vertex_of=None):
    """the fans as a set of (vertex, the faces of the fan, n_links), in the names of another ordering when given"""
    members = [[] for _ in range(len(res["vertex"]))]
    for f, row in enumerate(res["fan_out"].tolist()):
        for j in row:
            if j >= 0:
                members[j].append(f if face_of is None else int(face_of[f]))
    return {(int(v) if vertex_of is None else int(vertex_of[v]), tuple(sorted(m)), int(n)) for v, m, n in zip(res["vertex"], members, res["n_links"])}


def test_face_order_vertex_names_and_two_runs(hp):
    rng = np.random.default_rng(17)
    vtx, faces = mc.glued_soup(rng, 120)
    ref = _check(hp, vtx, faces)
    assert ref["stats"]["n_singular_vertices"] > 40 and ref["stats"]["n_nonmanifold_before"] > 10
    a, b = _device(hp), _device(hp)
    assert a["stats"] == b["stats"] and all(a[k].tobytes() == b[k].tobytes() for k, _ in ARRAYS)
    order_free = [n for n in mc.STAT_NAMES if n not in ("n_corners_moved", "n_faces_changed")]   # which fan keeps its vertex goes by the labels
    for seed in (1, 2):
        p = np.random.default_rng(seed).permutation(len(faces))
        got = _check(hp, vtx, faces[p], what=("faces shuffled", seed))
        assert [got["stats"][n] for n in order_free] == [ref["stats"][n] for n in order_free] and np.array_equal(got["n_fans_out"], ref["n_fans_out"])
        assert _partition(got, face_of=p) == _partition(ref)
    sv, sf, perm = hc.relabel(rng, vtx, faces)
    got = _check(hp, sv, sf, what="vertices relabelled")
    inverse = np.argsort(perm)
    assert got["stats"] == ref["stats"] and np.array_equal(got["n_fans_out"][perm], ref["n_fans_out"]) and _partition(got, vertex_of=inverse) == _partition(ref)
    assert np.array_equal(got["faces_out"] != sf, ref["faces_out"] != faces)            # the same corners move: the labels are the faces'


# ---- fetches and errors ------------------------------------------------------------------------------------------------------------------------------------
def test_fetches_lifecycle_and_argument_errors():
    h = make_hip(capi.load_hip_library(), _small_cfg())
    try:
        vtx, faces = mc.glued_soup(np.random.default_rng(3), 12)
        ref = mc.manifold(vtx, faces)
        n_f, n_n, nv, nf = ref["stats"]["n_fans"], ref["stats"]["n_new_vertices"], len(vtx), len(faces)
        assert n_n >= 3
        fetches = (h.topology_manifold_vertices, h.topology_manifold_fans, h.topology_manifold_faces, h.topology_manifold_new_vertices, h.topology_manifold_apply)
        with pytest.raises(RuntimeError, match=r"rc=-1: .*topology_manifold: .*built"):
            h.topology_manifold()                                                     # before a build
        h.raycast_build_triangles(vtx, faces)
        with pytest.raises(RuntimeError, match=r"rc=-1: .*topology_manifold: no analysis"):
            h.topology_manifold()                                                     # before an analysis
        h.topology_analyse()
        for fetch in fetches:
            with pytest.raises(RuntimeError, match=r"rc=-1: .*no manifold pass since the last analysis"):
                fetch()                                                               # a fetch or an apply before a pass
        _same(_device(h), ref)
        h.topology_analyse()
        for fetch in fetches:
            with pytest.raises(RuntimeError, match=r"rc=-1: .*no manifold pass"):
                fetch()                                                               # after a new analysis
        _same(_device(h), ref)
        h.raycast_build_triangles(vtx, faces)
        for fetch in fetches:
            with pytest.raises(RuntimeError, match=r"rc=-1: .*no analysis"):
                fetch()                                                               # after a rebuild
        h.topology_analyse()
        _same(_device(h), ref)
        h.topology_orient(oc.ORIENT_FIRST)
        h.topology_orient_apply()
        for fetch in fetches:
            with pytest.raises(RuntimeError, match=r"rc=-1: .*no analysis"):
                fetch()                                                               # after another pass' apply
        h.topology_analyse()
        for fetch in fetches:
            with pytest.raises(RuntimeError, match=r"rc=-1: .*no manifold pass"):
                fetch()                                                               # and it does not come back with the next analysis
        h.raycast_build_triangles(vtx, faces)
        h.topology_analyse()
        _same(_device(h), ref)
        f = h.lib.immesh_topology_manifold; f.argtypes = [C.c_void_p, C.c_void_p]
        assert f(None, None) == -1 and f(h.raycaster(), None) == 0                     # stats may be NULL
        # vertices and faces: no cap, NULL asks for nothing
        g = h.lib.immesh_topology_manifold_vertices; g.argtypes = [C.c_void_p, C.c_void_p]
        assert g(None, None) == -1 and g(h.raycaster(), None) == 0
        g = h.lib.immesh_topology_manifold_faces; g.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        only = np.zeros((nf, 3), np.int32)
        assert g(None, None, None) == -1 and g(h.raycaster(), None, None) == 0
        assert g(h.raycaster(), only.ctypes.data_as(C.c_void_p), None) == 0 and np.array_equal(only, ref["fan_out"])
        assert g(h.raycaster(), None, only.ctypes.data_as(C.c_void_p)) == 0 and np.array_equal(only, ref["faces_out"])
        # fans
        g = h.lib.immesh_topology_manifold_fans; g.argtypes = [C.c_void_p] + [C.c_void_p] * 5 + [C.c_int64, C.c_void_p]
        n = C.c_int64(-5)
        assert g(h.raycaster(), None, None, None, None, None, -1, C.byref(n)) == -1 and b"topology_manifold_fans: cap is negative" in _err(h)
        assert g(None, None, None, None, None, None, 0, None) == -1 and g(h.raycaster(), None, None, None, None, None, 0, None) == 0
        assert g(h.raycaster(), None, None, None, None, None, 0, C.byref(n)) == 0 and n.value == n_f
        for which, k in enumerate(mc.TABLES):
            room = np.zeros(n_f + 1, np.int32)
            args = [None] * 5
            args[which] = room.ctypes.data_as(C.c_void_p)
            n = C.c_int64(-5)
            assert g(h.raycaster(), *args, n_f - 1, C.byref(n)) == -4 and n.value == n_f and b"cap %d < %d fans" % (n_f - 1, n_f) in _err(h)
            assert not room.any()
            assert g(h.raycaster(), *args, n_f, C.byref(n)) == 0 and n.value == n_f and np.array_equal(room[:n_f], ref[k]) and room[n_f] == 0
        # new vertices
        g = h.lib.immesh_topology_manifold_new_vertices; g.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
        vsrc, xyz = np.zeros(n_n + 1, np.int32), np.zeros((n_n + 1, 3), np.float32)
        n = C.c_int64(-5)
        assert g(h.raycaster(), None, None, 0, C.byref(n)) == 0 and n.value == n_n and g(h.raycaster(), None, None, 0, None) == 0
        assert g(None, None, None, 0, None) == -1 and g(h.raycaster(), None, None, -1, C.byref(n)) == -1 and b"cap is negative" in _err(h)
        assert g(h.raycaster(), vsrc.ctypes.data_as(C.c_void_p), None, n_n - 1, C.byref(n)) == -4 and n.value == n_n and not vsrc.any()
        assert g(h.raycaster(), None, xyz.ctypes.data_as(C.c_void_p), n_n - 1, C.byref(n)) == -4 and not xyz.any()
        assert b"cap %d < %d new vertices" % (n_n - 1, n_n) in _err(h)
        assert g(h.raycaster(), vsrc.ctypes.data_as(C.c_void_p), None, n_n, C.byref(n)) == 0 and np.array_equal(vsrc[:n_n], ref["vsrc"]) and vsrc[n_n] == 0
        assert g(h.raycaster(), None, xyz.ctypes.data_as(C.c_void_p), n_n, C.byref(n)) == 0 and xyz[:n_n].tobytes() == ref["xyz"].tobytes() and not xyz[n_n].any()
        a = h.lib.immesh_topology_manifold_apply; a.argtypes = [C.c_void_p]
        assert a(None) == -1
        t = h.lib.immesh_topology_manifold_last_timing; t.argtypes = [C.c_void_p, C.c_void_p]
        assert t(h.raycaster(), None) == -1 and t(None, None) == -1 and h.topology_manifold_timing()[0] > 0.0
        _same(_device(h), ref)
        assert h._raycast_sizes()[:2] == (nv, nf)                                       # nothing has reached the caster
    finally:
        h.close()


# ---- apply -----------------------------------------------------------------------------------------------------------------------------------------------------
def test_apply_equals_a_fresh_build_from_the_split_soup(hp):
    rng = np.random.default_rng(31)
    vtx, faces = mc.glued_soup(rng, 60)
    vtx = ((vtx - vtx.min(axis=0)) / np.float32(25.0)).astype(np.float32)               # into a box of about 4 x 4 x 0.4
    dirs = (rng.normal(size=(2000, 3)) * np.array([0.3, 0.3, 1.0])).astype(np.float32)
    dirs[:, 2] = -np.abs(dirs[:, 2]) - 0.5
    org = (rng.uniform(0.0, 1.0, (2000, 3)) * np.array([4.2, 4.2, 0.0]) + np.array([0.0, 0.0, 2.0])).astype(np.float32)
    pts = rng.uniform(-0.2, 4.4, (3000, 3)).astype(np.float32) * np.array([1.0, 1.0, 0.1], np.float32)
    other = make_hip(capi.load_hip_library(), _small_cfg())
    try:
        hp.raycast_build_triangles(vtx, faces)
        t0, f0 = hp.raycast(capi.ray_frame(), dirs, org, 0.0, 100.0)
        assert (f0 >= 0).sum() > 50 and hp.mesh_sample(300.0, 7, fetch=False) > 500 and len(hp.raycast_points(0.05)) > 20
        before = _analysis(hp)["stats"]
        ref = mc.manifold(vtx, faces)
        _same(_device(hp), ref)
        assert ref["stats"]["n_new_vertices"] >= 20 and before["n_nonmanifold"] >= 5
        hp.topology_orient(oc.ORIENT_FIRST)                                           # an orientation and a holes pass of the same analysis: the apply
        hp.topology_holes(8)                                                          # discards them too
        hp.topology_manifold_apply()
        assert hp.topology_manifold_timing()[1] > 0.0
        for call in (hp.topology_faces, hp.topology_orient_faces, hp.topology_holes_loops, hp.topology_manifold_faces, hp.topology_manifold_apply,
                     hp.topology_manifold):
            with pytest.raises(RuntimeError, match=r"rc=-1: .*no analysis"):
                call()
        with pytest.raises(RuntimeError, match=r"rc=-1: .*no NEAREST cast"):
            hp.raycast_points(0.05)
        with pytest.raises(RuntimeError, match=r"rc=-1: .*no samples"):
            hp.nearest_samples(1.0, want=())
        other.raycast_build_triangles(ref["vtx_out"], ref["faces_out"])
        assert hp._raycast_sizes() == other._raycast_sizes() and hp._raycast_sizes()[:2] == (len(vtx) + ref["stats"]["n_new_vertices"], len(faces))
        # rays, closest points and samples: equal to the fresh build's bit for bit, and to the unsplit soup's, whose faces lie where they lay
        t1, f1 = hp.raycast(capi.ray_frame(), dirs, org, 0.0, 100.0)
        t2, f2 = other.raycast(capi.ray_frame(), dirs, org, 0.0, 100.0)
        assert t1.tobytes() == t2.tobytes() and f1.tobytes() == f2.tobytes() and t1.tobytes() == t0.tobytes() and f1.tobytes() == f0.tobytes()
        assert hp.raycast_points(0.05).tobytes() == other.raycast_points(0.05).tobytes()
        c1, c2 = hp.closest_points(pts, 5.0), other.closest_points(pts, 5.0)
        assert "side" in c1 and all(c1[k_].tobytes() == c2[k_].tobytes() for k_ in c1) and (c1["face"] >= 0).all()
        s1, s2 = hp.mesh_sample(300.0, 7), other.mesh_sample(300.0, 7)
        assert len(s1[0]) > 500 and s1[0].tobytes() == s2[0].tobytes() and s1[1].tobytes() == s2[1].tobytes()
        # its analysis and the Invariant
        after, fresh = _analysis(hp), _analysis(other)
        _same_analysis(after, fresh)
        _same_analysis(after, tc.analyse(ref["vtx_out"], ref["faces_out"]))
        a = after["stats"]
        assert a["n_nonmanifold"] == 0 and a["n_counting"] == before["n_counting"] and a["n_degenerate"] == before["n_degenerate"]
        assert a["n_vertices_used"] == ref["stats"]["n_fans"] and a["n_boundary"] + 2 * a["n_interior"] == 3 * a["n_counting"]
        assert a["n_interior"] >= before["n_interior"] and a["n_components"] >= before["n_components"]
        # a second pass moves nothing
        again = _device(hp)
        _same(again, mc.manifold(ref["vtx_out"], ref["faces_out"]))
        assert again["stats"]["n_new_vertices"] == 0 and again["stats"]["n_corners_moved"] == 0 and np.array_equal(again["faces_out"], ref["faces_out"])
    finally:
        other.close()


@pytest.mark.parametrize("soup, max_edges, unsplit_want, split_want", [("touching_holes", 64, (2, 1, 1), (2, 0, 2)), ("pinched_sheet", 8, (3, 1, 0), (4, 0, 2))])
def test_split_orient_holes_fills_both_holes(hp, soup, max_edges, unsplit_want, split_want):
    """(loops, loops that are not simple, filled loops) before and after the split: the holes that met in a vertex both fill"""
    vtx, faces = hc.touching_holes() if soup == "touching_holes" else mc.pinched_sheet()
    hp.raycast_build_triangles(vtx, faces)
    hp.topology_analyse()
    unsplit = hp.topology_holes(max_edges)
    assert (unsplit.n_loops, unsplit.n_nonsimple, unsplit.n_filled) == unsplit_want
    ref = mc.manifold(vtx, faces)
    _same(_device(hp), ref)
    assert ref["stats"]["n_new_vertices"] == 1
    hp.topology_manifold_apply()
    hp.topology_analyse()
    hp.topology_orient(oc.ORIENT_FIRST)
    hp.topology_orient_apply()
    st = hp.topology_analyse()
    holes = hp.topology_holes(max_edges)
    oriented = oc.orient(ref["vtx_out"], ref["faces_out"], oc.ORIENT_FIRST)["faces"]
    want = hc.holes(ref["vtx_out"], oriented, max_edges)["stats"]
    assert {n: getattr(holes, n) for n in hc.STAT_NAMES} == want and st.n_nonmanifold == 0
    assert (holes.n_loops, holes.n_nonsimple, holes.n_filled) == split_want
    hp.topology_holes_apply()
    assert hp.topology_analyse().n_boundary_loops == holes.n_loops - holes.n_filled


# ---- the live mesh ---------------------------------------------------------------------------------------------------------------------------------------------
def test_live_mesh_split_without_side_effects():
    """a splits the snapshot of its live mesh and applies, b never does: a's answers equal the checker on the exported arrays, and both contexts go on
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
        a.topology_analyse()
        ref = mc.manifold(vtx, faces)
        _same(_device(a), ref, "live mesh")
        st = ref["stats"]
        print("live mesh: %d faces, %d used vertices, %d fans: %d singular vertices (at most %d fans), %d new vertices, %d non-manifold edges before; "
              "manifold %.3f ms" % (nf, st["n_vertices_used"], st["n_fans"], st["n_singular_vertices"], st["most_fans_at_vertex"], st["n_new_vertices"],
                                    st["n_nonmanifold_before"], a.topology_manifold_timing()[0]))
        a.topology_manifold_apply()
        _same_analysis(_analysis(a), tc.analyse(ref["vtx_out"], ref["faces_out"]), "the split snapshot")
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
    """6 300 sheets of 32 faces glued on vertices and edges, faces shuffled: about 200 000 faces"""
    rng = np.random.default_rng(51)
    vtx, faces = mc.glued_soup(rng, 6300)
    assert len(faces) > 200000
    ref = _check(hp, vtx, faces)
    st = ref["stats"]
    print("%d faces, %d fans, %d new vertices: manifold %.3f ms (the analysis before it %.3f ms)" % (len(faces), st["n_fans"], st["n_new_vertices"],
                                                                                                   hp.topology_manifold_timing()[0], hp.topology_timing()[0]))
    assert st["n_singular_vertices"] > 3000 and st["n_nonmanifold_before"] > 1000 and st["n_new_vertices"] >= st["n_singular_vertices"]
    hp.topology_manifold_apply()
    print("apply %.3f ms" % hp.topology_manifold_timing()[1])
    after = hp.topology_analyse()
    assert after.n_nonmanifold == 0 and after.n_vertices_used == st["n_fans"] and hp.topology_manifold().n_new_vertices == 0


# ---- the tools -----------------------------------------------------------------------------------------------------------------------------------------------------
def _load(name):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_mesh_eval_manifold_and_mesh_manifold(tmp_path, monkeypatch, capsys):
    mesh_eval, mesh_manifold = _load("mesh_eval"), _load("mesh_manifold")
    vtx, faces = tc.grid_sheet(4, 4, holes=[(1, 1), (2, 2)], scale=0.5)                 # hc.touching_holes() on a 2 x 2 square
    rng = np.random.default_rng(3)
    np.save(tmp_path / "cloud.npy", np.concatenate([rng.uniform(0, 2, (8000, 2)), np.zeros((8000, 1))], axis=1).astype(np.float32))
    _write_ply(tmp_path / "pinched.ply", vtx, faces)

    def run(*more):
        out = tmp_path / "out.json"
        monkeypatch.setattr(sys, "argv", ["mesh_eval.py", "--cloud", str(tmp_path / "cloud.npy"), "--ply", str(tmp_path / "pinched.ply"), "--out", str(out)] + list(more))
        mesh_eval.main()
        printed = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
        assert printed == json.load(open(out))
        return printed

    plain = run("--orient", "first", "--fill-holes", "8", "--topology")
    assert "manifold" not in plain and plain["holes"]["n_nonsimple"] == 1 and plain["holes"]["n_filled"] == 0 and plain["topology"]["n_boundary_loops"] == 2
    split = run("--manifold", "--orient", "first", "--fill-holes", "8", "--topology")
    want = mc.manifold(vtx, faces)["stats"]
    assert split["manifold"] == dict(want, n_nonmanifold_after=0, n_components_after=1, n_boundary_loops_after=2)
    # the two holes are one simple loop of eight edges now, which a fan of six faces closes; the outline stays
    assert split["holes"]["n_nonsimple"] == 0 and split["holes"]["n_filled"] == 1 and split["topology"]["n_boundary_loops"] == 1
    assert split["mesh"]["vertices"] == plain["mesh"]["vertices"] + 1 and split["mesh"]["faces"] == plain["mesh"]["faces"] + 6
    assert split["recall"] > plain["recall"]
    monkeypatch.setattr(sys, "argv", ["mesh_manifold.py", str(tmp_path / "pinched.ply"), str(tmp_path / "split.ply")])
    mesh_manifold.main()
    printed = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert {k: printed[k] for k in mc.STAT_NAMES} == want and printed["manifold_ms"] > 0
    v2, f2 = mesh_eval.read_ply(tmp_path / "split.ply")
    ref = mc.manifold(vtx, faces)
    assert v2.tobytes() == ref["vtx_out"].tobytes() and np.array_equal(f2, ref["faces_out"])
