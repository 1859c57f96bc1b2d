"""The weld and the vertex clustering on the device (include/immesh_simplify.h) against the numpy restatement of the contract
(tests/simplify_checker.py), bit for bit on every output: the stats, vtx_out as bits, the cluster tables, the maps and faces_out.  Strips at the sizes
where a launch gains a wavefront or a workgroup, a cluster that spans them, the mean that depends on its order, every key case, numbering under a
shuffle, every face status, nothing to do, order-freedom, the apply against a caster freshly built from the result, the reason for the feature end
to end, every error and capacity path, the live mesh as a snapshot without side effects, tools/mesh_eval.py's --weld, and scale."""
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
import topology_checker as tc
from immesh_amd import capi, synth
from conftest import make_hip
from parity_utils import compare_plane_tables_fast
from test_gpu_render import _small_cfg
from test_gpu_topology import _device as _analysis, _same as _same_analysis, _write_ply

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hp():
    h = make_hip(capi.load_hip_library(), _small_cfg())
    yield h
    h.close()


def _err(h):
    f = h.lib.immesh_last_error; f.restype = C.c_char_p; f.argtypes = [C.c_void_p]
    return f(h.ctx)


def _device(h, cell=0.0, mode=sc.FIRST, merge=True):
    """the pass, then every fetch, in the checker's shape"""
    st = h.simplify(cell, mode, merge)
    out = {"stats": {n: getattr(st, n) for n in sc.STAT_NAMES}}
    tables = h.simplify_vertices()
    out.update(vtx_out=tables["vtx"], first_vertex=tables["first_vertex"], n_members=tables["n_members"])
    out.update(h.simplify_maps())
    out["faces_out"] = h.simplify_faces()
    return out


def _check(h, vtx, faces, cell=0.0, mode=sc.FIRST, merge=True, what="", ref=None):
    """build, and the pass against the checker -> the checker's result"""
    h.raycast_build_triangles(vtx, faces)
    ref = sc.simplify(vtx, faces, cell, mode, merge) if ref is None else ref
    sc.same(_device(h, cell, mode, merge), ref, (what, cell, mode, merge))
    return ref


# ---- sizes where a launch gains a wavefront or a workgroup ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_strips_with_n_faces_and_with_n_vertices(hp, n):
    vtx, faces = tc.grid_sheet(1, (n + 1) // 2)
    by_faces = (vtx, faces[:n])                                                         # n faces of a strip of the sheet
    by_vtx = tc.strip(n - 2) if n >= 3 else (np.zeros((n, 3), np.float32), np.zeros((1, 3), np.int32))   # n vertices (one vertex: a face that does not count)
    for v, f in (by_faces, by_vtx):
        assert len(f) == n or len(v) == n
        for cell, mode in ((0.0, sc.FIRST), (2.0, sc.FIRST), (2.0, sc.MEAN)):
            _check(hp, v, f, cell, mode, what=n)
        uv, uf = sc.unshared(v, f, np.random.default_rng(n))
        ref = _check(hp, uv, uf, what=(n, "unshared"))
        shared = sc.simplify(v, f)["stats"]
        assert len(ref["faces_out"]) == shared["n_faces_out"] and (shared["n_not_counting"] > 0 or ref["stats"]["n_vertices_out"] == shared["n_vertices_out"])


@pytest.mark.parametrize("mode", [sc.FIRST, sc.MEAN])
def test_a_cluster_of_three_hundred_beside_five_hundred_small_ones(hp, mode):
    vtx, faces = sc.cluster_beside_many(np.random.default_rng(77))
    ref = _check(hp, vtx, faces, 1.0, mode)
    assert ref["stats"]["largest_cluster"] == 300 and ref["stats"]["n_vertices_out"] == 501
    sc.check_facts(vtx, faces, ref, 1.0, mode)


def test_the_mean_that_depends_on_the_order_of_its_members(hp):
    got = set()
    for order in itertools.permutations(range(3)):
        vtx, faces = sc.order_triple(order)
        ref = _check(hp, vtx, faces, 2.0 ** 62, sc.MEAN, what=order)
        assert ref["n_members"].tolist() == [3, 1, 1, 1]
        got.add(int(ref["vtx_out"][0, 0].view(np.uint32)))
        _check(hp, vtx, faces, 2.0 ** 62, sc.FIRST, what=order)
    assert len(got) == 2


# ---- keys, numbering, statuses ---------------------------------------------------------------------------------------------------------------------------
def test_keys_zeros_nan_range_edges_overflow_and_cell_walls(hp):
    vtx, faces, c = sc.key_cases()
    for cell, mode in ((c, sc.FIRST), (c, sc.MEAN), (0.0, sc.FIRST), (0.0, sc.MEAN), (5e-324, sc.MEAN), (1e300, sc.MEAN)):
        ref = _check(hp, vtx, faces, cell, mode)
        assert ref["stats"]["n_alone_not_finite"] == 4
    m = sc.simplify(vtx, faces, c)["vmap"]
    assert m[0] == m[1] and m[2] != m[3] and m[6] == m[8] != m[7] and m[9] == m[11] != m[10] and m[12] == m[13] and m[14] == m[15] and m[16] != m[17]
    walls = (np.arange(-40, 41)[:, None] * np.array([[0.3, 0.0, 0.0]])).astype(np.float32)   # ties on the walls of cell = 0.3, both signs
    a = np.arange(len(walls))
    _check(hp, walls, np.stack([a, (a + 1) % len(a), (a + 2) % len(a)], axis=-1).astype(np.int32), 0.3, sc.MEAN)


def test_labels_and_numbering_under_a_shuffle_of_the_vertex_indices(hp):
    rng = np.random.default_rng(5)
    ref = _check(hp, *sc.unshared(sc.CUBE_VTX, sc.CUBE_FACES, rng))
    assert ref["stats"]["n_vertices_out"] == 8 and all(ref["first_vertex"][c] == np.nonzero(ref["vmap"] == c)[0].min() for c in range(8))
    vtx, faces = tc.sheet_with_fragments(rng, 20, 17, 12, 9)
    plain = _check(hp, vtx, faces, 0.11, sc.MEAN)
    sv, sf, perm = sc.relabel(rng, vtx, faces)
    shuffled = _check(hp, sv, sf, 0.11, sc.MEAN)
    assert shuffled["stats"] == plain["stats"] and sorted(shuffled["n_members"].tolist()) == sorted(plain["n_members"].tolist())
    assert np.array_equal(shuffled["first_vertex"], np.sort(shuffled["first_vertex"]))


def test_every_status_and_duplicates_in_all_six_rotations_and_windings(hp):
    vtx, faces = sc.status_soup()
    on = _check(hp, vtx, faces, merge=True)
    assert on["fstatus"].tolist() == [0, 3, 3, 3, 3, 3, 3, 2, 1, 2] and on["faces_out"].tolist() == [[0, 1, 2]]
    off = _check(hp, vtx, faces, merge=False)
    assert off["fstatus"].tolist() == [0] * 7 + [2, 1, 2] and off["stats"]["n_duplicate"] == 0 and len(off["faces_out"]) == 7
    rng = np.random.default_rng(2)
    for case in range(6):                                                               # random index triples: long runs of duplicates
        v, f = tc.random_soup(rng, 300, 12)
        for merge in (True, False):
            _check(hp, v, f, 0.0, sc.FIRST, merge, what=case)
            _check(hp, v, f, 3.0, sc.MEAN, merge, what=case)


def test_zero_faces_and_a_soup_whose_faces_all_collapse(hp):
    vtx = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    ref = _check(hp, vtx, np.zeros((0, 3), np.int32), 0.5, sc.MEAN)
    assert ref["stats"] == dict(dict.fromkeys(sc.STAT_NAMES, 0), n_vertices_in=3) and ref["vmap"].tolist() == [-1, -1, -1]
    hp.simplify_apply()
    assert hp._raycast_sizes() == (0, 0, 0)
    ref = _check(hp, vtx, np.array([[0, 0, 1], [2, 2, 2]], np.int32))                   # faces, none of which counts
    assert ref["stats"]["n_not_counting"] == 2 and ref["stats"]["n_vertices_out"] == 0
    hp.simplify_apply()
    assert hp._raycast_sizes() == (0, 0, 0)
    vtx, faces = tc.grid_sheet(5, 4, scale=0.1)
    ref = _check(hp, vtx, faces, 10.0, sc.MEAN)
    assert ref["stats"]["n_faces_out"] == 0 and ref["stats"]["n_collapsed"] == 40 and ref["stats"]["n_vertices_out"] == 1 and ref["stats"]["largest_cluster"] == 30
    hp.simplify_apply()                                                                 # the cluster that lost all its faces is kept
    assert hp._raycast_sizes() == (1, 0, 0) and hp.topology_analyse().n_faces == 0
    t, face = hp.raycast(capi.ray_frame(), np.array([[0, 0, -1]], np.float32), np.array([[0.2, 0.2, 1]], np.float32), 0.0, 10.0)
    assert t.tolist() == [-1.0] and face.tolist() == [-1]


# ---- order-freedom -------------------------------------------------------------------------------------------------------------------------------------------
def test_a_permutation_of_the_faces_permutes_fmap_and_faces_out_and_nothing_else(hp):
    rng = np.random.default_rng(17)
    vtx, faces = tc.sheet_with_fragments(rng, 40, 30, 60, 40)
    for cell, mode in ((0.0, sc.FIRST), (0.12, sc.MEAN)):
        ref = _check(hp, vtx, faces, cell, mode)
        a, b = _device(hp, cell, mode), _device(hp, cell, mode)
        sc.same(a, b, "two runs")
        p = rng.permutation(len(faces))
        per = _check(hp, vtx, faces[p], cell, mode)
        assert per["stats"] == ref["stats"] and ref["stats"]["n_duplicate"] == 0       # (a duplicate's survivor is the one that comes first)
        assert all(per[k].tobytes() == ref[k].tobytes() for k in ("vtx_out", "first_vertex", "n_members", "vmap"))
        assert np.array_equal(per["fstatus"], ref["fstatus"][p]) and np.array_equal(per["fmap"] >= 0, ref["fmap"][p] >= 0)
        kept = per["fmap"] >= 0
        assert np.array_equal(per["faces_out"][per["fmap"][kept]], ref["faces_out"][ref["fmap"][p][kept]])
        assert cell == 0.0 or ref["stats"]["n_collapsed"] > 500


@pytest.mark.parametrize("case", range(11))
def test_welding_the_unshared_soup_gives_the_shared_soups_analysis(hp, case):
    rng = np.random.default_rng(700 + case)
    vtx, faces = tc.sheet_with_fragments(rng, 30, 30, 80, 20)
    want = tc.analyse(vtx, faces)["stats"]
    uv, uf = sc.unshared(vtx, faces, rng)
    ref = _check(hp, uv, uf, what=case)
    assert ref["stats"]["n_vertices_in"] == 3 * len(faces) and ref["stats"]["n_vertices_out"] == want["n_vertices_used"] and ref["stats"]["n_faces_out"] == len(faces)
    before = hp.topology_analyse()
    assert before.n_components == len(faces) and before.n_boundary == 3 * len(faces)
    hp.simplify_apply()
    st = hp.topology_analyse()
    assert {n: getattr(st, n) for n in tc.STAT_NAMES} == want


# ---- the apply ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell,mode", [(0.0, sc.FIRST), (0.13, sc.MEAN)])
def test_apply_equals_a_fresh_build_from_the_result(hp, cell, mode):
    rng = np.random.default_rng(31)
    vtx, faces = tc.sheet_with_fragments(rng, 30, 20, 40, 40)
    vtx = vtx + rng.normal(scale=0.01, size=vtx.shape).astype(np.float32)
    faces = np.concatenate([faces, faces[:50][:, [2, 0, 1]]])
    if cell == 0.0:
        vtx, faces = sc.unshared(vtx, faces, rng)
    dirs = (rng.normal(size=(2000, 3)) * np.array([0.3, 0.3, 1.0])).astype(np.float32)
    org = (rng.uniform(0.0, 1.0, (2000, 3)) * np.array([1.5, 1.0, 0.0]) + np.array([0.0, 0.0, 1.0])).astype(np.float32)
    dirs[:, 2] = -np.abs(dirs[:, 2]) - 0.5
    pts = np.concatenate([rng.uniform(-0.2, 1.7, (3000, 2)), rng.normal(scale=0.2, size=(3000, 1))], axis=1).astype(np.float32)
    other = make_hip(capi.load_hip_library(), _small_cfg())
    try:
        ref = _check(hp, vtx, faces, cell, mode)
        assert ref["stats"]["n_duplicate"] >= 50 and ref["stats"]["n_vertices_out"] < len(vtx)
        hp.raycast(capi.ray_frame(), dirs, org, 0.0, 100.0)
        assert hp.mesh_sample(300.0, 7, fetch=False) > 100 and len(hp.raycast_points(0.05)) > 100   # samples and a cast's points: the apply discards both
        hp.topology_analyse()
        hp.simplify_apply()
        assert hp.simplify_last_timing()[1] > 0.0
        for call in (hp.simplify_vertices, hp.simplify_maps, hp.simplify_faces, hp.simplify_apply):
            with pytest.raises(RuntimeError, match=r"rc=-1: .*no simplify pass"):
                call()                                                                  # a fetch after the apply
        with pytest.raises(RuntimeError, match=r"rc=-1: .*no analysis"):
            hp.topology_faces()
        with pytest.raises(RuntimeError, match=r"rc=-1: .*no NEAREST cast"):
            hp.raycast_points(0.05)
        with pytest.raises(RuntimeError, match=r"rc=-1: .*no samples"):
            hp.nearest_samples(1.0, want=())
        other.raycast_build_triangles(ref["vtx_out"], ref["faces_out"])
        assert hp._raycast_sizes() == other._raycast_sizes() and hp._raycast_sizes()[:2] == (len(ref["vtx_out"]), len(ref["faces_out"]))
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
        _same_analysis(after, tc.analyse(ref["vtx_out"], ref["faces_out"]))
        again = _device(hp, cell, sc.FIRST)                                             # a second pass over the applied result
        sc.same(again, sc.simplify(ref["vtx_out"], ref["faces_out"], cell, sc.FIRST))
        assert cell > 0.0 or (again["stats"]["largest_cluster"] == 1 and again["stats"]["n_faces_out"] == len(ref["faces_out"]))
    finally:
        other.close()


def test_the_applies_of_orient_and_holes_discard_a_simplify_result(hp):
    vtx, faces = tc.grid_sheet(6, 5, holes=[(1, 1), (3, 3)])
    fetches = (hp.simplify_vertices, hp.simplify_maps, hp.simplify_faces, hp.simplify_apply)
    for apply in ("orient", "holes", "build"):
        ref = _check(hp, vtx, faces, 2.0, sc.MEAN)
        hp.topology_analyse()                                                           # an analysis leaves the result alone
        sc.same(dict(_device(hp, 2.0, sc.MEAN)), ref)
        assert np.array_equal(hp.simplify_faces(), ref["faces_out"])
        if apply == "orient":
            hp.topology_orient(capi.ORIENT_FIRST)
            hp.topology_orient_apply()
        elif apply == "holes":
            hp.topology_holes(8)
            hp.topology_holes_apply()
        else:
            hp.raycast_build_triangles(vtx, faces)
        for fetch in fetches:
            with pytest.raises(RuntimeError, match=r"rc=-1: .*no simplify pass"):
                fetch()


def test_the_unshared_cube_becomes_one_closed_consistently_wound_surface(hp):
    rng = np.random.default_rng(8)
    vtx, faces = sc.unshared(sc.CUBE_VTX, sc.CUBE_FACES, rng)
    faces[::2] = faces[::2][:, [0, 2, 1]]                                               # every other face wound the other way
    hp.raycast_build_triangles(vtx, faces)
    st = hp.topology_analyse()
    assert (st.n_components, st.n_boundary, st.n_vertices_used) == (12, 36, 36)         # topology is a matter of indices: twelve lone faces
    welded = hp.simplify(0.0)
    assert (welded.n_vertices_out, welded.n_faces_out, welded.largest_cluster) == (8, 12, 6)
    hp.simplify_apply()
    st = hp.topology_analyse()
    assert (st.n_components, st.n_boundary, st.euler, st.n_vertices_used, st.n_nonmanifold) == (1, 0, 2, 8, 0) and st.n_inconsistent > 0
    assert hp.topology_orient(capi.ORIENT_FIRST).n_inconsistent_after == 0
    hp.topology_orient_apply()
    st = hp.topology_analyse()
    assert (st.n_components, st.n_boundary, st.euler, st.n_inconsistent) == (1, 0, 2, 0)


# ---- fetches and errors ------------------------------------------------------------------------------------------------------------------------------------------
def test_fetches_lifecycle_and_argument_errors():
    h = make_hip(capi.load_hip_library(), _small_cfg())
    try:
        vtx, faces = tc.grid_sheet(6, 5)
        faces = np.concatenate([faces, faces[:3]])
        ref = sc.simplify(vtx, faces, 2.0, sc.MEAN)
        n_v, n_f = ref["stats"]["n_vertices_out"], ref["stats"]["n_faces_out"]
        assert (n_v, n_f) == (12, 12)
        fetches = (h.simplify_vertices, h.simplify_maps, h.simplify_faces, h.simplify_apply)
        with pytest.raises(RuntimeError, match=r"rc=-1: .*built"):
            h.simplify(2.0)                                                             # before a build
        for fetch in fetches:
            with pytest.raises(RuntimeError, match=r"rc=-1: .*built"):
                fetch()
        h.raycast_build_triangles(vtx, faces)
        for fetch in fetches:
            with pytest.raises(RuntimeError, match=r"rc=-1: .*no simplify pass"):
                fetch()                                                                 # a fetch or an apply before a pass

        def still_usable():
            sc.same(_device(h, 2.0, sc.MEAN), ref)

        still_usable()
        for bad in (-1.0, -1e-300, np.nan, np.inf, -np.inf):
            with pytest.raises(RuntimeError, match=r"rc=-1: .*cell"):
                h.simplify(bad)
            assert np.array_equal(h.simplify_faces(), ref["faces_out"])                 # refused before anything was touched: the last pass stays
        for bad in (-1, 2, 7, 2 ** 31 - 1):
            for cell in (0.0, 2.0):                                                     # the weld reads and validates the mode too
                with pytest.raises(RuntimeError, match=r"rc=-1: .*mode"):
                    h.simplify(cell, bad)
            assert np.array_equal(h.simplify_faces(), ref["faces_out"])
        f = h.lib.immesh_simplify; f.argtypes = [C.c_void_p, C.c_double, C.c_int32, C.c_int32, C.c_void_p]
        assert f(None, 2.0, 1, 1, None) == -1 and f(h.raycaster(), 2.0, 1, 1, None) == 0   # stats may be NULL
        assert f(h.raycaster(), 2.0, 1, -7, None) == 0 and h.simplify_faces().tobytes() == ref["faces_out"].tobytes()   # any value but 0 merges
        # vertices
        g = h.lib.immesh_simplify_vertices; g.argtypes = [C.c_void_p] + [C.c_void_p] * 3 + [C.c_int64, C.c_void_p]
        n = C.c_int64(-5)
        assert g(h.raycaster(), None, None, None, -1, C.byref(n)) == -1 and b"cap" in _err(h)
        assert g(None, None, None, None, 0, None) == -1 and g(h.raycaster(), None, None, None, 0, None) == 0
        assert g(h.raycaster(), None, None, None, 0, C.byref(n)) == 0 and n.value == n_v
        for which, k in enumerate(("vtx_out", "first_vertex", "n_members")):
            room = np.zeros((n_v + 1,) + ref[k].shape[1:], ref[k].dtype)
            args = [None] * 3
            args[which] = room.ctypes.data_as(C.c_void_p)
            n = C.c_int64(-5)
            assert g(h.raycaster(), *args, n_v - 1, C.byref(n)) == -4 and n.value == n_v and b"cap %d < %d" % (n_v - 1, n_v) in _err(h)
            assert not room.any()
            assert g(h.raycaster(), *args, n_v, C.byref(n)) == 0 and n.value == n_v and room[:n_v].tobytes() == ref[k].tobytes() and not room[n_v:].any()
        # maps
        g = h.lib.immesh_simplify_maps; g.argtypes = [C.c_void_p] + [C.c_void_p] * 3
        assert g(None, None, None, None) == -1 and g(h.raycaster(), None, None, None) == 0
        for which, k in enumerate(("vmap", "fmap", "fstatus")):
            room = np.zeros(len(ref[k]) + 1, ref[k].dtype)
            args = [None] * 3
            args[which] = room.ctypes.data_as(C.c_void_p)
            assert g(h.raycaster(), *args) == 0 and np.array_equal(room[:-1], ref[k]) and room[-1] == 0
        # faces
        g = h.lib.immesh_simplify_faces; g.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
        room = np.zeros((n_f + 1, 3), np.int32)
        n = C.c_int64(-5)
        assert g(h.raycaster(), None, 0, C.byref(n)) == 0 and n.value == n_f and g(h.raycaster(), None, 0, None) == 0 and g(None, None, 0, None) == -1
        assert g(h.raycaster(), None, -1, C.byref(n)) == -1 and b"cap" in _err(h)
        assert g(h.raycaster(), room.ctypes.data_as(C.c_void_p), n_f - 1, C.byref(n)) == -4 and n.value == n_f and not room.any()
        assert b"cap %d < %d" % (n_f - 1, n_f) in _err(h)
        assert g(h.raycaster(), room.ctypes.data_as(C.c_void_p), n_f, C.byref(n)) == 0 and np.array_equal(room[:n_f], ref["faces_out"]) and not room[n_f].any()
        a = h.lib.immesh_simplify_apply; a.argtypes = [C.c_void_p]
        assert a(None) == -1
        t = h.lib.immesh_simplify_last_timing; t.argtypes = [C.c_void_p, C.c_void_p]
        assert t(h.raycaster(), None) == -1 and t(None, None) == -1 and h.simplify_last_timing()[0] > 0.0
        still_usable()
        h.raycast_build_triangles(vtx, faces)                                           # a rebuild discards the result
        for fetch in fetches:
            with pytest.raises(RuntimeError, match=r"rc=-1: .*no simplify pass"):
                fetch()
        still_usable()
    finally:
        h.close()


# ---- the live mesh -----------------------------------------------------------------------------------------------------------------------------------------------
def test_live_mesh_simplified_without_side_effects():
    """a clusters its snapshot of the live mesh and applies, b never does: a's answers equal the checker on the exported arrays, and both contexts go on
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
        sc.same(_device(a), sc.simplify(vtx, faces), "live mesh, weld")
        ref = sc.simplify(vtx, faces, 0.5, sc.MEAN)
        sc.same(_device(a, 0.5, sc.MEAN), ref, "live mesh, cell 0.5")
        st = ref["stats"]
        print("live mesh: %d vertices, %d faces -> %d vertices, %d faces at cell 0.5 (largest cluster %d, %d collapsed, %d duplicate); simplify %.3f ms"
              % (nv, nf, st["n_vertices_out"], st["n_faces_out"], st["largest_cluster"], st["n_collapsed"], st["n_duplicate"], a.simplify_last_timing()[0]))
        assert 0 < st["n_faces_out"] < nf and st["n_vertices_out"] < nv
        a.simplify_apply()
        _same_analysis(_analysis(a), tc.analyse(ref["vtx_out"], ref["faces_out"]), "the simplified snapshot")
        assert compare_plane_tables_fast(planes, a.dump_planes(), 0.0) > 100 and a.counters() == counters
        for k in range(4, 6):
            scan(k)
        ea, eb = a.mesh_export(1.0, 20), b.mesh_export(1.0, 20)
        assert len(ea[1]) != len(faces) and ea[0].tobytes() == eb[0].tobytes() and ea[1].tobytes() == eb[1].tobytes()
        assert compare_plane_tables_fast(a.dump_planes(), b.dump_planes(), 0.0) > 100
    finally:
        a.close(); b.close()


# ---- tools/mesh_eval.py ------------------------------------------------------------------------------------------------------------------------------------------
def test_mesh_eval_welds_the_unshared_cube(tmp_path, monkeypatch, capsys):
    spec = importlib.util.spec_from_file_location("mesh_eval", os.path.join(ROOT, "tools", "mesh_eval.py"))
    mesh_eval = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mesh_eval)
    rng = np.random.default_rng(3)
    _write_ply(tmp_path / "cube.ply", *sc.unshared(sc.CUBE_VTX, sc.CUBE_FACES, rng))
    cloud = rng.uniform(0, 1, (6000, 3))
    cloud[np.arange(6000), rng.integers(0, 3, 6000)] = rng.integers(0, 2, 6000)        # on the cube's six sides
    np.save(tmp_path / "cloud.npy", cloud.astype(np.float32))

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
    lone = run("--topology")
    assert lone["topology"]["n_components"] == 12 and {k: v for k, v in lone.items() if k != "topology"} == plain
    welded = run("--weld", "--topology")
    assert welded["simplify"] == dict(cell=0.0, mode="first", merge_duplicates=True, n_vertices_in=36, n_vertices_used=36, n_alone_not_finite=0,
                                      n_alone_outside=0, n_vertices_out=8, largest_cluster=6, n_faces_in=12, n_not_counting=0, n_collapsed=0, n_duplicate=0,
                                      n_faces_out=12)
    assert welded["topology"]["n_components"] == 1 and welded["topology"]["n_boundary"] == 0 and welded["topology"]["euler"] == 2
    assert welded["mesh"]["vertices"] == 8 and welded["mesh"]["faces"] == 12 and welded["accuracy"] == plain["accuracy"] and welded["samples"] == plain["samples"]
    same = run("--simplify", "0", "--topology", "--min-component-faces", "2")          # the fragment filter sees the welded mesh: one component of 12
    assert same["filter"]["faces_kept"] == 12 and same["filter"]["components_before"] == 1 and same["topology"] == welded["topology"]
    coarse = run("--simplify", "0.75", "--simplify-mode", "mean", "--keep-duplicate-faces")   # a cell per corner: the weld by another route
    assert coarse["simplify"] == dict(welded["simplify"], cell=0.75, mode="mean", merge_duplicates=False) and coarse["mesh"] == welded["mesh"]
    for bad in (["--weld", "--simplify", "1"], ["--simplify-mode", "mean"], ["--keep-duplicate-faces"]):
        with pytest.raises(SystemExit):
            run(*bad)
    capsys.readouterr()


# ---- scale -----------------------------------------------------------------------------------------------------------------------------------------------------------
def test_scale(hp):
    """a 316 x 316 sheet, about 200 000 faces, unshared and shuffled (600 000 vertices): the weld, then the shared sheet at four grid steps"""
    rng = np.random.default_rng(51)
    vtx, faces = tc.grid_sheet(316, 316, scale=0.05)
    faces = faces[rng.permutation(len(faces))]
    uv, uf = sc.unshared(vtx, faces, rng)
    assert len(uf) == 199712 and len(uv) == 3 * len(uf)
    t0 = time.perf_counter()
    ref = _check(hp, uv, uf)
    print("%d vertices, %d faces: weld %.3f ms" % (len(uv), len(uf), hp.simplify_last_timing()[0]))
    assert ref["stats"]["n_vertices_out"] == 317 * 317 and ref["stats"]["n_faces_out"] == len(uf) and ref["stats"]["largest_cluster"] == 6
    hp.simplify_apply()
    assert hp.topology_analyse().n_components == 1
    for mode in (sc.FIRST, sc.MEAN):
        ref = _check(hp, vtx, faces, 0.2, mode)
        print("cell 0.2 mode %d: %d -> %d faces, simplify %.3f ms" % (mode, len(faces), ref["stats"]["n_faces_out"], hp.simplify_last_timing()[0]))
        assert ref["stats"]["largest_cluster"] >= 16 and 10000 < ref["stats"]["n_faces_out"] < 14000
    print("the checker and the device together: %.1f s" % (time.perf_counter() - t0))
