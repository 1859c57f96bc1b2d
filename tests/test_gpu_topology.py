"""Mesh topology on the device (include/immesh_topology.h) against the numpy restatement of the contract (tests/topology_checker.py), bit for bit on
every output (box zeros as values): sizes at which the launches change shape, label propagation along a strip in three face orders, long runs of one
key, the closed forms of the CPU tier, order-freedom, boxes with NaN vertices, every arm of the Select rule, rebuilding from the kept faces,
lifecycle and argument errors, the live mesh as a snapshot without side effects, scale, and tools/mesh_eval.py's fragment filter."""
import ctypes as C
import importlib.util
import json
import os
import sys

import numpy as np
import pytest

import closest_checker as cc
import raycast_checker as rcc
import topology_checker as tc
from immesh_amd import capi, synth
from conftest import make_hip
from parity_utils import compare_plane_tables_fast
from test_gpu_render import _small_cfg, _soup
from test_topology_cpu import CLOSED_FORMS, check_closed_form

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = (tc.EDGE_BOUNDARY, tc.EDGE_NONMANIFOLD, tc.EDGE_INCONSISTENT)
TABLES = ("first_face", "n_faces", "n_boundary")


@pytest.fixture(scope="module")
def hp():
    h = make_hip(capi.load_hip_library(), _small_cfg())
    yield h
    h.close()


def _err(h):
    f = h.lib.immesh_last_error; f.restype = C.c_char_p; f.argtypes = [C.c_void_p]
    return f(h.ctx)


def _device(h):
    """analyse, then every fetch, in the checker's shape"""
    st = h.topology_analyse()
    out = {"stats": {n: getattr(st, n) for n in tc.STAT_NAMES}, "comp": h.topology_faces(), "edges": {k: h.topology_edges(k) for k in KINDS}}
    out.update(h.topology_components())
    return out


def _same(got, ref, what=""):
    assert got["stats"] == ref["stats"], (what, got["stats"], ref["stats"])
    for k in ("comp",) + TABLES:
        assert got[k].dtype == ref[k].dtype == np.int32 and np.array_equal(got[k], ref[k]), (what, k, got[k][:10], ref[k][:10])
    assert got["box"].dtype == ref["box"].dtype == np.float32 and got["box"].shape == ref["box"].shape
    assert not np.isnan(got["box"]).any() and np.array_equal(got["box"], ref["box"]), (what, "box")     # as values: -0 == +0, inf == inf
    for kind in KINDS:
        for g, r in zip(got["edges"][kind], ref["edges"][kind]):
            assert g.dtype == r.dtype == np.int32 and g.shape == r.shape and np.array_equal(g, r), (what, "edges", kind)


def _check(h, vtx, faces, ref=None, what=""):
    h.raycast_build_triangles(vtx, faces)
    ref = tc.analyse(vtx, faces) if ref is None else ref
    got = _device(h)
    _same(got, ref, what)
    return ref


def _check_select(h, ref, faces, what="", **kw):
    keep, kept = h.topology_select(**kw)
    want_keep, want_kept = tc.select(ref, faces, **kw)
    assert keep.dtype == np.int8 and np.array_equal(keep, want_keep), (what, kw, keep[:20], want_keep[:20])
    assert kept.dtype == np.int32 and np.array_equal(kept, want_kept), (what, kw)
    return want_keep, want_kept


# ---- sizes -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_faces", [0, 1, 2, 3, 64, 65, 256, 257, 1000])
def test_sizes_match_checker(hp, n_faces):
    for seed, n_vtx in ((0, 12), (1, 5), (2, 40)):
        rng = np.random.default_rng(1000 * seed + n_faces)
        vtx, faces = tc.random_soup(rng, n_faces, n_vtx)
        ref = _check(hp, vtx, faces, what=(n_faces, n_vtx))
        if n_faces >= 64 and n_vtx == 12:                                              # the checker first: degenerate and duplicate faces and long runs do occur
            assert ref["stats"]["n_degenerate"] > 0 and ref["stats"]["n_nonmanifold"] > 0 and ref["edges"][tc.EDGE_NONMANIFOLD][1].max() >= 3
        for kw in (dict(), dict(min_faces=2), dict(min_diagonal=3.0), dict(keep_largest=1), dict(min_faces=1, min_diagonal=0.5, keep_largest=3)):
            _check_select(hp, ref, faces, n_faces, **kw)
    if n_faces == 0:
        assert all(v == 0 for v in ref["stats"].values())


def test_all_faces_degenerate(hp):
    vtx = np.zeros((3, 3), np.float32)
    faces = np.array([[0, 0, 1], [2, 2, 2], [1, 0, 1]] * 30, np.int32)
    ref = _check(hp, vtx, faces)
    assert ref["stats"]["n_counting"] == 0 and ref["stats"]["n_degenerate"] == 90 and (ref["comp"] == -1).all()
    keep, kept = _check_select(hp, ref, faces)
    assert not keep.any() and len(kept) == 0


# ---- propagation -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["natural", "reversed", "shuffled"])
def test_strip_labels_travel_the_whole_length(hp, order):
    vtx, faces = tc.strip(4097)
    if order == "reversed":
        faces = faces[::-1].copy()
    elif order == "shuffled":
        faces = faces[np.random.default_rng(5).permutation(len(faces))]
    ref = _check(hp, vtx, faces, what=order)
    assert ref["stats"]["n_components"] == 1 and (ref["comp"] == 0).all() and ref["n_faces"].tolist() == [4097] and ref["stats"]["n_boundary_loops"] == 1
    assert ref["stats"]["largest_loop_edges"] == ref["stats"]["n_boundary"] == 4099


def test_300_faces_on_one_edge(hp):
    vtx = np.random.default_rng(6).uniform(-1, 1, (302, 3)).astype(np.float32)
    faces = np.stack([np.zeros(300), np.ones(300), np.arange(300) + 2], axis=-1).astype(np.int32)
    faces[::2] = faces[::2, [1, 0, 2]]                                                # both directions
    ref = _check(hp, vtx, faces)
    assert ref["stats"]["n_components"] == 1 and ref["stats"]["n_nonmanifold"] == 1 and ref["stats"]["n_boundary"] == 600
    assert ref["edges"][tc.EDGE_NONMANIFOLD][0].tolist() == [[0, 1]] and ref["edges"][tc.EDGE_NONMANIFOLD][1].tolist() == [300]


def test_300_copies_of_one_face(hp):
    vtx = np.array([[-1, -1, -5], [1, -1, -5], [0, 1.5, -5]], np.float32)
    faces = np.tile(np.array([[0, 1, 2]], np.int32), (300, 1))
    ref = _check(hp, vtx, faces)
    assert ref["stats"]["n_components"] == 1 and ref["stats"]["n_edges"] == 3 and ref["edges"][tc.EDGE_NONMANIFOLD][1].tolist() == [300, 300, 300]
    assert ref["stats"]["euler"] == 3 - 3 + 300


# ---- closed forms --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CLOSED_FORMS))
def test_closed_forms_on_the_device(hp, name):
    vtx, faces = CLOSED_FORMS[name][0]()
    hp.raycast_build_triangles(vtx, faces)
    got = _device(hp)
    check_closed_form(name, got["stats"], got["edges"])
    _same(got, tc.analyse(vtx, faces), name)


# ---- order-freedom -------------------------------------------------------------------------------------------------------------------------------------
def test_face_order_permutes_the_partition_and_nothing_else(hp):
    rng = np.random.default_rng(7)
    vtx, faces = tc.sheet_with_fragments(rng, 30, 20, 12, 80)
    faces = np.concatenate([faces, tc.random_soup(rng, 200, 25)[1] + 40]).astype(np.int32)
    ref = _check(hp, vtx, faces)
    a = _device(hp)
    b = _device(hp)                                                                   # two analyses of one soup: equal bits
    assert a["stats"] == b["stats"] and all(a[k].tobytes() == b[k].tobytes() for k in ("comp", "box") + TABLES)
    assert all(x.tobytes() == y.tobytes() for kind in KINDS for x, y in zip(a["edges"][kind], b["edges"][kind]))
    perm = rng.permutation(len(faces))
    _check(hp, vtx, faces[perm])
    p = _device(hp)
    assert p["stats"] == a["stats"]
    assert all(x.tobytes() == y.tobytes() for kind in KINDS for x, y in zip(a["edges"][kind], p["edges"][kind]))
    pairs = set(zip(a["comp"][perm].tolist(), p["comp"].tolist()))                    # face perm[i] of a is face i of p: one partition
    assert len(pairs) == len({x for x, _ in pairs}) == len({y for _, y in pairs}) == a["stats"]["n_components"] + 1
    inv = np.argsort(perm)
    for ca, cp in pairs:                                                              # the labels follow the permutation
        if ca >= 0:
            assert p["first_face"][cp] == inv[np.nonzero(a["comp"] == ca)[0]].min() and p["n_faces"][cp] == a["n_faces"][ca]
            assert p["n_boundary"][cp] == a["n_boundary"][ca] and np.array_equal(p["box"][cp], a["box"][ca])
    assert ref["stats"]["n_components"] > 80


# ---- boxes -----------------------------------------------------------------------------------------------------------------------------------------------
def test_boxes_with_vertices_that_are_not_finite(hp):
    vtx = np.array([[0, 0, 0], [1, 0, -0.0], [0, 1, 0], [np.nan, 5, 2], [7, np.inf, 2], [1, -np.inf, 1],                   # a NaN / inf vertex in a finite component
                    [np.nan, np.nan, np.nan], [np.inf, np.nan, -np.inf], [np.nan, np.inf, np.nan],                       # no finite float at all
                    [np.nan, 1, 2], [np.nan, 3, 5], [np.nan, 0, 0]], np.float32)                                        # no finite x
    faces = np.array([[0, 1, 2], [2, 1, 3], [3, 1, 4], [4, 3, 5], [6, 7, 8], [9, 10, 11]], np.int32)
    ref = _check(hp, vtx, faces)
    assert ref["stats"]["n_components"] == 3
    assert ref["box"][0].tolist() == [0, -0.0, 0, 7, 5, 2] and ref["box"][1].tolist() == [np.inf] * 3 + [-np.inf] * 3
    assert ref["box"][2].tolist() == [np.inf, 0, 0, -np.inf, 3, 5]
    for md, want in ((0.0, [1, 1, 1, 1, 1, 1]), (1e-300, [1, 1, 1, 1, 0, 0]), (1.0, [1, 1, 1, 1, 0, 0]), (9.0, [0, 0, 0, 0, 0, 0])):
        keep, _ = _check_select(hp, ref, faces, md, min_diagonal=md)
        assert keep.tolist() == want, md                                              # a component without a finite box fails any min_diagonal > 0


# ---- select ------------------------------------------------------------------------------------------------------------------------------------------------
def _select_soup():
    """strips of 1, 2, 3, 3 and 5 faces and a (3, 4, 0) right triangle, each with vertices of its own, a degenerate face between them"""
    vs, fs, base = [], [], 0
    for k, n in enumerate((3, 1, 5, 2, 3)):
        v, f = tc.strip(n)
        vs.append(v + np.float32(16 * k)); fs.append(f + base); base += len(v)
    vs.append(np.array([[100, 100, 100], [103, 100, 100], [100, 104, 100]], np.float32)); fs.append(np.array([[0, 1, 2], [1, 1, 2]], np.int32) + base)
    return np.concatenate(vs).astype(np.float32), np.concatenate(fs).astype(np.int32)


def test_select_rule(hp):
    vtx, faces = _select_soup()
    ref = _check(hp, vtx, faces)
    assert ref["n_faces"].tolist() == [3, 1, 5, 2, 3, 1] and ref["comp"][-1] == -1
    assert _check_select(hp, ref, faces, min_faces=3)[0].sum() == 11                  # on a component's size
    assert _check_select(hp, ref, faces, min_faces=4)[0].sum() == 5                   # and one past it
    assert _check_select(hp, ref, faces, min_faces=6)[0].sum() == 0
    # the triangle's diagonal is exactly 5: 9 + 16 = 25, every square exact
    assert ref["box"][5].tolist() == [100, 100, 100, 103, 104, 100]
    tri = ref["comp"] == 5
    assert _check_select(hp, ref, faces, min_diagonal=5.0)[0][tri].tolist() == [1]
    assert _check_select(hp, ref, faces, min_diagonal=float(np.nextafter(5.0, 6.0)))[0][tri].tolist() == [0]
    assert _check_select(hp, ref, faces, min_diagonal=float(np.nextafter(5.0, 0.0)))[0][tri].tolist() == [1]
    # the two components of three faces tie: the smaller label goes first
    for k, want in ((1, [2]), (2, [0, 2]), (3, [0, 2, 4]), (4, [0, 2, 3, 4]), (6, [0, 1, 2, 3, 4, 5]), (100, [0, 1, 2, 3, 4, 5])):
        keep, _ = _check_select(hp, ref, faces, keep_largest=k)
        assert sorted(set(ref["comp"][keep != 0].tolist())) == want, k
    keep, _ = _check_select(hp, ref, faces, min_faces=4, keep_largest=2)              # the ranking is among all components: 0 is ranked second and then fails min_faces
    assert sorted(set(ref["comp"][keep != 0].tolist())) == [2]
    _check_select(hp, ref, faces, min_faces=2, min_diagonal=1.0, keep_largest=3)
    # a cap one short of the count: the count comes back, the mask too
    f = hp.lib.immesh_topology_select
    f.argtypes = [C.c_void_p, C.c_int64, C.c_double, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    n, keep, out = C.c_int64(0), np.zeros(len(faces), np.int8), np.zeros((14, 3), np.int32)
    args = (hp.raycaster(), 2, 0.0, 0, keep.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    assert f(*args, 12, C.byref(n)) == -4 and n.value == 13 and b"cap 12 < 13" in _err(hp)
    assert np.array_equal(keep, tc.select(ref, faces, min_faces=2)[0])
    assert f(*args, 13, C.byref(n)) == 0 and n.value == 13 and np.array_equal(out[:13], tc.select(ref, faces, min_faces=2)[1])
    with pytest.raises(RuntimeError, match=r"rc=-4: .*cap 12 < 13"):
        hp.topology_select(min_faces=2, cap=12)
    g = hp.lib.immesh_topology_components; g.argtypes = [C.c_void_p] + [C.c_void_p] * 4 + [C.c_int64, C.c_void_p]
    first = np.zeros(6, np.int32)
    assert g(hp.raycaster(), first.ctypes.data_as(C.c_void_p), None, None, None, 5, C.byref(n)) == -4 and n.value == 6
    assert g(hp.raycaster(), first.ctypes.data_as(C.c_void_p), None, None, None, 6, C.byref(n)) == 0 and first.tolist() == ref["first_face"].tolist()
    e = hp.lib.immesh_topology_edges; e.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    uses = np.zeros(64, np.int32)
    nb = ref["stats"]["n_boundary"]
    assert e(hp.raycaster(), 0, None, uses.ctypes.data_as(C.c_void_p), nb - 1, C.byref(n)) == -4 and n.value == nb
    assert e(hp.raycaster(), 0, None, uses.ctypes.data_as(C.c_void_p), nb, C.byref(n)) == 0 and uses[:nb].tolist() == [1] * nb


def test_rebuilding_from_the_kept_faces(hp):
    rng = np.random.default_rng(9)
    vtx, faces = tc.sheet_with_fragments(rng, 24, 24, 10, 120)
    ref = _check(hp, vtx, faces)
    keep, kept = _check_select(hp, ref, faces, min_faces=3)
    kept_comps = sorted(set(ref["comp"][keep != 0].tolist()))
    assert 1 < len(kept_comps) < ref["stats"]["n_components"]
    again = _check(hp, vtx, kept)
    assert again["stats"]["n_components"] == len(kept_comps) and again["n_faces"].tolist() == ref["n_faces"][kept_comps].tolist()
    assert np.array_equal(again["box"], ref["box"][kept_comps]) and again["n_boundary"].tolist() == ref["n_boundary"][kept_comps].tolist()
    assert again["stats"]["n_counting"] == len(kept) == int(keep.sum())
    keep2, kept2 = _check_select(hp, again, kept, min_faces=3)
    assert keep2.all() and np.array_equal(kept2, kept)


# ---- lifecycle and errors ------------------------------------------------------------------------------------------------------------------------------------
def test_lifecycle_and_argument_errors():
    h = make_hip(capi.load_hip_library(), _small_cfg())
    try:
        vtx, faces = tc.grid_sheet(3, 2)
        with pytest.raises(RuntimeError, match=r"rc=-1: .*built"):
            h.topology_analyse()                                                      # an analysis before a build
        h.raycast_build_triangles(vtx, faces)
        fetches = (h.topology_faces, h.topology_components, lambda: h.topology_edges(tc.EDGE_BOUNDARY), h.topology_select)
        for fetch in fetches:
            with pytest.raises(RuntimeError, match=r"rc=-1: .*no analysis"):
                fetch()                                                               # a fetch before an analysis
        ref = tc.analyse(vtx, faces)
        _same(_device(h), ref)
        h.raycast_build_triangles(vtx, faces)
        for fetch in fetches:
            with pytest.raises(RuntimeError, match=r"rc=-1: .*no analysis"):
                fetch()                                                               # a fetch after a rebuild
        assert h.topology_timing()[0] > 0.0

        def still_usable():
            _same(_device(h), ref)
            _check_select(h, ref, faces, min_faces=1)

        still_usable()
        for kw, text in ((dict(min_faces=-1), "min_faces"), (dict(keep_largest=-1), "keep_largest"), (dict(min_diagonal=-1.0), "min_diagonal"),
                         (dict(min_diagonal=np.nan), "min_diagonal"), (dict(min_diagonal=np.inf), "min_diagonal"), (dict(cap=-1), "cap")):
            with pytest.raises(RuntimeError, match=r"rc=-1: .*" + text):
                h.topology_select(**kw)
            still_usable()
        for kind in (-1, 3, 99):
            with pytest.raises(RuntimeError, match=r"rc=-1: .*kind"):
                h.topology_edges(kind)
            still_usable()
        n = C.c_int64(0)
        e = h.lib.immesh_topology_edges; e.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
        assert e(h.raycaster(), 0, None, None, -1, C.byref(n)) == -1 and b"cap" in _err(h)
        g = h.lib.immesh_topology_components; g.argtypes = [C.c_void_p] + [C.c_void_p] * 4 + [C.c_int64, C.c_void_p]
        assert g(h.raycaster(), None, None, None, None, -1, C.byref(n)) == -1 and b"cap" in _err(h)
        a = h.lib.immesh_topology_analyse; a.argtypes = [C.c_void_p, C.c_void_p]
        assert a(None, None) == -1 and a(h.raycaster(), None) == 0                     # stats may be NULL
        f = h.lib.immesh_topology_faces; f.argtypes = [C.c_void_p, C.c_void_p]
        assert f(h.raycaster(), None) == 0 and f(None, None) == -1
        s = h.lib.immesh_topology_select; s.argtypes = [C.c_void_p, C.c_int64, C.c_double, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
        assert s(h.raycaster(), 0, 0.0, 0, None, None, 0, None) == 0                   # every output may be NULL
        still_usable()
        # a failed build leaves the caster and its analysis as they were
        with pytest.raises(RuntimeError, match=r"rc=-1: .*out of range"):
            h.raycast_build_triangles(vtx, np.array([[0, 1, 99]], np.int32))
        _same(_device(h), ref)
        # a caster with zero faces analyses to all zeros
        h.raycast_build_triangles(vtx, np.zeros((0, 3), np.int32))
        got = _device(h)
        assert all(v == 0 for v in got["stats"].values()) and len(got["comp"]) == 0 and len(got["first_face"]) == 0
        keep, kept = h.topology_select(min_faces=1)
        assert len(keep) == 0 and len(kept) == 0
        h.raycast_build_triangles(vtx, faces)
        with pytest.raises(RuntimeError, match=r"rc=-1: .*no analysis"):
            h.topology_faces()
        still_usable()
    finally:
        h.close()


def test_rays_and_closest_points_after_an_analysis(hp):
    rng = np.random.default_rng(10)
    vtx, faces = _soup(rng, 3000)
    hp.raycast_build_triangles(vtx, faces)
    dirs = rng.normal(size=(2000, 3)).astype(np.float32)
    pts = rng.uniform(-20, 20, (2000, 3)).astype(np.float32)
    t0, f0 = hp.raycast(capi.ray_frame(), dirs, None, 0.0, 100.0)
    points0 = hp.raycast_points(0.05)
    c0 = hp.closest_points(pts, 5.0)
    assert (f0 >= 0).sum() > 50 and (c0["face"] >= 0).sum() > 100
    ref = tc.analyse(vtx, faces)
    for _ in range(2):
        _same(_device(hp), ref)
        _check_select(hp, ref, faces, min_faces=2, keep_largest=5)
        assert hp.raycast_points(0.05).tobytes() == points0.tobytes()                 # the cast's points outlive an analysis
        t1, f1 = hp.raycast(capi.ray_frame(), dirs, None, 0.0, 100.0)
        c1 = hp.closest_points(pts, 5.0)
        assert t1.tobytes() == t0.tobytes() and f1.tobytes() == f0.tobytes() and all(c0[k].tobytes() == c1[k].tobytes() for k in c0)
    rt, rf = rcc.cast(np.eye(3), np.zeros(3), dirs[:200], None, 0.0, 100.0, vtx, faces)
    assert np.array_equal(f1[:200], rf) and t1[:200].tobytes() == rt.tobytes()
    assert np.array_equal(c1["face"][:100], cc.closest(None, None, pts[:100], 5.0, vtx, faces)[2])


# ---- the live mesh ---------------------------------------------------------------------------------------------------------------------------------------------
def test_live_mesh_snapshot_without_side_effects():
    """a analyses its snapshot of the live mesh between scans, b never does: a's answers equal the checker on the exported arrays, and both contexts go
    on to the same mesh and plane table"""
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
        ref = tc.analyse(vtx, faces)
        _same(_device(a), ref, "live mesh")
        st = ref["stats"]
        print("live mesh: %d faces, %d components (largest %d), %d boundary edges in %d loops, %d non-manifold, %d inconsistent, euler %d; analysis %.3f ms"
              % (nf, st["n_components"], st["largest_component_faces"], st["n_boundary"], st["n_boundary_loops"], st["n_nonmanifold"], st["n_inconsistent"],
                 st["euler"], a.topology_timing()[0]))
        _check_select(a, ref, faces, min_faces=10)
        assert compare_plane_tables_fast(planes, a.dump_planes(), 0.0) > 100 and a.counters() == counters
        for k in range(4, 6):
            scan(k)
        _same(_device(a), ref, "the old snapshot")                                # the snapshot is the caster's own: the stream has not touched it
        ea, eb = a.mesh_export(1.0, 20), b.mesh_export(1.0, 20)
        assert len(ea[1]) != len(faces) and ea[0].tobytes() == eb[0].tobytes() and ea[1].tobytes() == eb[1].tobytes()
        assert compare_plane_tables_fast(a.dump_planes(), b.dump_planes(), 0.0) > 100
    finally:
        a.close(); b.close()


# ---- scale -------------------------------------------------------------------------------------------------------------------------------------------------------
def test_scale(hp):
    """a 320 x 320 sheet with 300 holes plus 2 000 fragments, faces shuffled: about 209 000 faces against the checker"""
    rng = np.random.default_rng(51)
    vtx, faces = tc.sheet_with_fragments(rng, 320, 320, 300, 2000)
    assert len(faces) > 200000
    ref = _check(hp, vtx, faces)
    print("%d faces: analysis %.3f ms" % (len(faces), hp.topology_timing()[0]))
    assert ref["stats"]["n_components"] == 2001 and ref["stats"]["largest_component_faces"] == 2 * (320 * 320 - 300) and ref["stats"]["n_boundary_loops"] > 2000
    keep, kept = _check_select(hp, ref, faces, min_faces=5)
    assert len(kept) == ref["stats"]["largest_component_faces"]
    print("select %.3f ms" % hp.topology_timing()[1])
    _check_select(hp, ref, faces, keep_largest=100)


# ---- tools/mesh_eval.py --------------------------------------------------------------------------------------------------------------------------------------------
def _write_ply(path, vtx, faces):
    """the layout immesh_save_ply writes"""
    head = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\nelement face %d\n"
            "property list uchar int vertex_indices\nend_header\n" % (len(vtx), len(faces))).encode()
    rec = np.zeros((len(faces), 13), np.uint8)
    rec[:, 0] = 3
    rec[:, 1:] = np.ascontiguousarray(faces, np.int32).view(np.uint8).reshape(len(faces), 12)
    with open(path, "wb") as fp:
        fp.write(head + np.ascontiguousarray(vtx, np.float32).tobytes() + rec.tobytes())


def test_mesh_eval_drops_the_fragment(tmp_path, monkeypatch, capsys):
    spec = importlib.util.spec_from_file_location("mesh_eval", os.path.join(ROOT, "tools", "mesh_eval.py"))
    mesh_eval = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mesh_eval)
    square = np.array([[0, 0, 0], [2, 0, 0], [2, 2, 0], [0, 2, 0]], np.float32)
    far = np.array([[50, 50, 50], [51, 50, 50], [50, 51, 50]], np.float32)
    rng = np.random.default_rng(3)
    cloud = np.concatenate([rng.uniform(0, 2, (4000, 2)), rng.normal(scale=0.02, size=(4000, 1))], axis=1).astype(np.float32)
    np.save(tmp_path / "cloud.npy", cloud)
    _write_ply(tmp_path / "both.ply", np.concatenate([far, square]), np.array([[3, 4, 5], [0, 1, 2], [3, 5, 6]], np.int32))   # the fragment between the square's faces
    _write_ply(tmp_path / "square.ply", square, np.array([[0, 1, 2], [0, 2, 3]], np.int32))

    def run(ply, *more):
        out = tmp_path / "out.json"
        monkeypatch.setattr(sys, "argv", ["mesh_eval.py", "--cloud", str(tmp_path / "cloud.npy"), "--ply", str(tmp_path / ply), "--out", str(out)] + list(more))
        mesh_eval.main()
        printed = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
        res = json.load(open(out))
        assert printed == res
        return res

    alone = run("square.ply")
    assert "topology" not in alone and "filter" not in alone                          # both options off: the output as it was
    both = run("both.ply")
    filtered = run("both.ply", "--min-component-faces", "2", "--topology")
    figures = [k for k in alone if k != "mesh"]
    assert all(json.dumps(filtered[k]) == json.dumps(alone[k]) for k in figures), (filtered, alone)        # bit for bit: repr round-trips a double
    assert both["samples"] > alone["samples"] and both["completeness"]["share_within_tau"] < alone["completeness"]["share_within_tau"]
    assert filtered["filter"] == {"min_component_faces": 2, "faces_before": 3, "faces_kept": 2, "components_before": 2}
    assert filtered["topology"]["n_components"] == 1 and filtered["topology"]["n_boundary"] == 4 and filtered["topology"]["euler"] == 1
    assert filtered["mesh"]["faces"] == 2 and both["mesh"]["faces"] == 3
