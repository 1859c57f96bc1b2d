"""The orientation on the device (include/immesh_topology.h, the Orientation rule) against the numpy restatement of the contract
(tests/orient_checker.py), bit for bit on every output and in all three modes: sizes at which the launches change shape, propagation along a strip
in three face orders, non-orientable patches, flipped closed and open surfaces, long runs of one key, every arm of the modes, order-freedom, the
apply against a caster freshly built from the oriented faces, lifecycle and argument errors, the live mesh as a snapshot without side effects,
scale, and tools/mesh_eval.py's --orient."""
import ctypes as C
import importlib.util
import json
import os
import sys

import numpy as np
import pytest

import orient_checker as oc
import topology_checker as tc
from immesh_amd import capi, synth
from conftest import make_hip
from parity_utils import compare_plane_tables_fast
from test_gpu_render import _small_cfg, _soup
from test_gpu_topology import _device as _analysis, _same as _same_analysis, _write_ply

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VIEW = (0.5, -0.25, 30.0)


@pytest.fixture(scope="module")
def hp():
    h = make_hip(capi.load_hip_library(), _small_cfg())
    yield h
    h.close()


def _err(h):
    f = h.lib.immesh_last_error; f.restype = C.c_char_p; f.argtypes = [C.c_void_p]
    return f(h.ctx)


def _device(h, mode, o=None):
    """orient, then every fetch, in the checker's shape"""
    st = h.topology_orient(mode, o if mode == oc.ORIENT_VIEWPOINT else None)
    out = {"stats": {n: getattr(st, n) for n in oc.STAT_NAMES}}
    out.update(h.topology_orient_faces())
    out.update(h.topology_orient_patches())
    return out


def _same(got, ref, what=""):
    assert got["stats"] == ref["stats"], (what, got["stats"], ref["stats"])
    for k, t in (("patch", np.int32), ("flip", np.int8), ("faces", np.int32)) + tuple((k, np.int32) for k in oc.TABLES):
        assert got[k].dtype == ref[k].dtype == t and got[k].shape == ref[k].shape and np.array_equal(got[k], ref[k]), (what, k, got[k][:10], ref[k][:10])


def _check(h, vtx, faces, modes=oc.MODES, o=VIEW, what=""):
    """build, analyse, and every mode against the checker -> the checker's results by mode"""
    h.raycast_build_triangles(vtx, faces)
    st = h.topology_analyse()
    part = oc.partition(faces)
    refs = {}
    for mode in modes:
        refs[mode] = oc.orient(vtx, faces, mode, o, part)
        _same(_device(h, mode, o), refs[mode], (what, mode))
        assert refs[mode]["stats"]["n_inconsistent_before"] == st.n_inconsistent
    return refs


# ---- sizes -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_faces", [0, 1, 2, 3, 64, 65, 256, 257, 1000])
def test_sizes_match_checker(hp, n_faces):
    for seed, n_vtx in ((0, 12), (1, 40), (2, 200)):
        rng = np.random.default_rng(1000 * seed + n_faces)
        vtx, faces = tc.random_soup(rng, n_faces, n_vtx)
        refs = _check(hp, vtx, faces, what=(n_faces, n_vtx))
    if n_faces == 0:
        assert all(v == 0 for v in refs[0]["stats"].values()) and len(refs[0]["faces"]) == 0
    if n_faces == 1000:                                                                # (200 vertices) the checker first: patches of several faces, wound both ways
        assert refs[0]["stats"]["largest_patch_faces"] > 2 and 10 <= refs[0]["stats"]["n_inconsistent_before"] and refs[0]["stats"]["n_faces_flipped"] > 5


def test_all_faces_degenerate(hp):
    vtx = np.zeros((3, 3), np.float32)
    faces = np.array([[0, 0, 1], [2, 2, 2], [1, 0, 1]] * 30, np.int32)
    refs = _check(hp, vtx, faces)
    assert refs[0]["stats"]["n_patches"] == 0 and (refs[0]["patch"] == -1).all() and np.array_equal(refs[0]["faces"], faces)


# ---- propagation -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["natural", "reversed", "shuffled"])
def test_strip_flips_alternate_over_the_whole_length(hp, order):
    vtx, faces = tc.strip(4097)
    if order == "reversed":
        faces = faces[::-1].copy()
    elif order == "shuffled":
        faces = faces[np.random.default_rng(5).permutation(len(faces))]
    refs = _check(hp, vtx, faces, what=order)
    first = refs[oc.ORIENT_FIRST]
    assert first["stats"]["n_patches"] == 1 and first["stats"]["n_inconsistent_before"] == 4096 and first["stats"]["n_inconsistent_after"] == 0
    along = first["flip"][np.argsort(faces[:, 0])]                                     # in the strip's own order
    assert (along[1:] != along[:-1]).all() and first["flip"][0] == 0
    assert refs[oc.ORIENT_FEWEST]["stats"]["n_faces_flipped"] == 2048


# ---- non-orientable patches -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["moebius 9", "moebius 2049", "klein 16 x 16"])
def test_nonorientable_patches_are_left_alone(hp, name):
    vtx, faces = {"moebius 9": lambda: tc.moebius(9), "moebius 2049": lambda: tc.moebius(2049), "klein 16 x 16": lambda: oc.klein(16, 16)}[name]()
    refs = _check(hp, vtx, faces, what=name)
    for ref in refs.values():
        st = ref["stats"]
        assert st["n_patches"] == st["n_nonorientable"] == 1 and st["n_faces_flipped"] == 0 and st["n_faces_nonorientable"] == len(faces)
        assert st["n_inconsistent_after"] == st["n_inconsistent_before"] >= 1 and np.array_equal(ref["faces"], faces)
    faces2 = faces.copy()                                                              # cut the band / the bottle: it becomes orientable
    faces2[0] = [0, 0, 0]
    if name.startswith("moebius"):
        assert _check(hp, vtx, faces2, what=name + " cut")[0]["stats"]["n_nonorientable"] == 0


# ---- flipped closed and open surfaces ----------------------------------------------------------------------------------------------------------------------
def test_flipped_torus_and_flipped_sheet_with_bands(hp):
    rng = np.random.default_rng(21)
    vtx, faces = tc.torus(16, 16)
    flipped, mask = oc.flip_random(rng, faces)
    refs = _check(hp, vtx, flipped, what="torus")
    want = mask ^ mask[0]                                                              # FIRST follows face 0
    assert np.array_equal(refs[oc.ORIENT_FIRST]["flip"] != 0, want) and refs[oc.ORIENT_FIRST]["stats"]["n_inconsistent_after"] == 0
    assert refs[oc.ORIENT_FEWEST]["stats"]["n_faces_flipped"] == min(want.sum(), (~want).sum())
    vtx, faces = tc.sheet_with_fragments(rng, 30, 20, 12, 80)
    vtx, faces = oc.with_moebius(vtx, oc.flip_random(rng, faces)[0], (7, 9, 12))
    refs = _check(hp, vtx, faces, what="sheet")
    st = refs[oc.ORIENT_VIEWPOINT]["stats"]
    assert st["n_nonorientable"] == 3 and st["n_orientable"] == 81 and st["n_faces_nonorientable"] == 2 * (7 + 9 + 12) and st["n_inconsistent_after"] >= 3
    sheet = refs[oc.ORIENT_VIEWPOINT]["patch"] == np.argmax(refs[oc.ORIENT_VIEWPOINT]["n_faces"])
    assert (oc.view_sign(vtx, refs[oc.ORIENT_VIEWPOINT]["faces"], VIEW)[sheet] == 1).all()      # the sheet shows its front to the viewpoint above it


# ---- runs ----------------------------------------------------------------------------------------------------------------------------------------------------
def test_long_runs_join_nothing(hp):
    vtx = np.random.default_rng(6).uniform(-1, 1, (302, 3)).astype(np.float32)
    faces = np.stack([np.zeros(300), np.ones(300), np.arange(300) + 2], axis=-1).astype(np.int32)
    faces[::2] = faces[::2, [1, 0, 2]]
    refs = _check(hp, vtx, faces, what="300 faces on one edge")
    assert refs[0]["stats"]["n_patches"] == 300 and refs[0]["stats"]["largest_patch_faces"] == 1 and refs[0]["patch"].tolist() == list(range(300))
    vtx = np.array([[-1, -1, -5], [1, -1, -5], [0, 1.5, -5]], np.float32)
    refs = _check(hp, vtx, np.tile(np.array([[0, 1, 2]], np.int32), (300, 1)), what="300 copies")
    assert refs[0]["stats"]["n_patches"] == 300 and refs[0]["stats"]["n_faces_flipped"] == 0
    refs = _check(hp, vtx, np.array([[0, 1, 2], [0, 1, 2]], np.int32), what="2 copies")
    assert refs[0]["flip"].tolist() == [0, 1] and refs[0]["n_inconsistent"].tolist() == [3] and refs[0]["faces"].tolist() == [[0, 1, 2], [0, 2, 1]]


# ---- modes -----------------------------------------------------------------------------------------------------------------------------------------------------
def test_modes(hp):
    vtx, faces = tc.grid_sheet(9, 7)
    faces[0] = faces[0][[0, 2, 1]]
    refs = _check(hp, vtx, faces, o=(1.0, 1.0, 5.0), what="one face reversed")
    assert refs[oc.ORIENT_FIRST]["flip"].tolist() == [0] + [1] * 125 and refs[oc.ORIENT_FIRST]["stats"]["n_patches_inverted"] == 0
    assert refs[oc.ORIENT_FEWEST]["flip"].tolist() == [1] + [0] * 125 and refs[oc.ORIENT_FEWEST]["stats"]["n_patches_inverted"] == 1
    assert refs[oc.ORIENT_VIEWPOINT]["flip"].tolist() == [1] + [0] * 125
    assert _check(hp, vtx, faces, (oc.ORIENT_VIEWPOINT,), o=(1.0, 1.0, -5.0))[2]["flip"].tolist() == [0] + [1] * 125
    refs = _check(hp, *tc.strip(4096), modes=(oc.ORIENT_FEWEST,), what="a tie")
    assert refs[1]["stats"]["n_patches_inverted"] == 0 and refs[1]["stats"]["n_faces_flipped"] == 2048 and refs[1]["flip"][0] == 0
    vtx, faces = tc.tetrahedron()
    assert _check(hp, vtx, faces, (oc.ORIENT_VIEWPOINT,), o=(0.2, 0.2, 0.2))[2]["flip"].tolist() == [1] * 4       # from inside every face shows its back
    assert _check(hp, vtx, faces, (oc.ORIENT_VIEWPOINT,), o=(-1e6, -2e6, -3e6))[2]["flip"].tolist() == [0] * 4    # far outside: three fronts, one back
    assert _check(hp, vtx, faces, (oc.ORIENT_VIEWPOINT,), o=(1e6, 2e6, 3e6))[2]["flip"].tolist() == [1] * 4       # and from the other side one front
    assert _check(hp, vtx, faces, (oc.ORIENT_VIEWPOINT,), o=(3e38, -3e38, 3e38))[2]["stats"]["n_patches"] == 1    # the largest floats: no overflow in double
    # a roof of two faces wound alike, seen from one side of its ridge: one vote each way, a tie keeps FIRST
    roof = np.array([[0, 0, 1], [0, 1, 1], [1, 0, 0], [-1, 0, 0]], np.float32)
    roof_faces = np.array([[0, 1, 2], [1, 0, 3]], np.int32)
    assert sorted(oc.view_sign(roof, roof_faces, (5.0, 0.5, 1.0)).tolist()) == [-1, 1]
    assert _check(hp, roof, roof_faces, (oc.ORIENT_VIEWPOINT,), o=(5.0, 0.5, 1.0))[2]["stats"]["n_patches_inverted"] == 0
    assert _check(hp, roof, roof_faces[:, [0, 2, 1]], (oc.ORIENT_VIEWPOINT,), o=(5.0, 0.5, 1.0))[2]["stats"]["n_faces_flipped"] == 0
    # a viewpoint in the sheet's plane: s = 0, nobody votes
    vtx, faces = tc.grid_sheet(4, 3)
    faces[0] = faces[0][[0, 2, 1]]
    ref = _check(hp, vtx, faces, (oc.ORIENT_VIEWPOINT,), o=(9.0, 9.0, 0.0))[2]
    assert not oc.view_sign(vtx, faces, (9.0, 9.0, 0.0)).any() and ref["flip"].tolist() == [0] + [1] * 23
    # NaN / inf vertices and a face of zero area: no vote, but flipped with their patch
    vtx = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [np.nan, 2, 0], [2, np.inf, 0], [2, 0, 0]], np.float32)
    faces = np.array([[0, 2, 1], [0, 3, 2], [3, 4, 2], [1, 2, 5], [0, 1, 6]], np.int32)
    ref = _check(hp, vtx, faces, (oc.ORIENT_VIEWPOINT,), o=(0.5, 0.5, 3.0))[2]
    assert oc.view_sign(vtx, faces, (0.5, 0.5, 3.0)).tolist() == [-1, -1, 0, 0, 0] and ref["flip"].tolist() == [1] * 5


# ---- order-freedom -------------------------------------------------------------------------------------------------------------------------------------
def test_face_order_permutes_patches_flips_and_tables(hp):
    rng = np.random.default_rng(7)
    vtx, faces = tc.sheet_with_fragments(rng, 30, 20, 12, 80)
    faces = np.concatenate([oc.flip_random(rng, faces, 0.3)[0], tc.random_soup(rng, 200, 25)[1] + 40]).astype(np.int32)
    vtx, faces = oc.with_moebius(vtx, faces, (9,))
    _check(hp, vtx, faces)
    a = {m: _device(hp, m, VIEW) for m in oc.MODES}
    b = {m: _device(hp, m, VIEW) for m in oc.MODES}                                    # two runs: equal bits
    assert all(a[m]["stats"] == b[m]["stats"] and all(a[m][k].tobytes() == b[m][k].tobytes() for k in ("patch", "flip", "faces") + oc.TABLES) for m in oc.MODES)
    perm = rng.permutation(len(faces))
    _check(hp, vtx, faces[perm])
    p = {m: _device(hp, m, VIEW) for m in oc.MODES}
    inv = np.argsort(perm)
    for m in oc.MODES:
        assert {k: v for k, v in p[m]["stats"].items() if k not in ("n_faces_flipped", "n_patches_inverted")} == \
               {k: v for k, v in a[m]["stats"].items() if k not in ("n_faces_flipped", "n_patches_inverted")}
        pairs = set(zip(a[m]["patch"][perm].tolist(), p[m]["patch"].tolist()))        # face perm[i] of a is face i of p: one partition
        assert len(pairs) == len({x for x, _ in pairs}) == len({y for _, y in pairs}) == a[m]["stats"]["n_patches"] + 1
        for ca, cp in pairs:
            if ca < 0:
                continue
            mine = np.nonzero(a[m]["patch"] == ca)[0]
            assert p[m]["first_face"][cp] == inv[mine].min() and all(p[m][k][cp] == a[m][k][ca] for k in ("n_faces", "orientable", "n_inconsistent"))
            fa, fp = a[m]["flip"][mine], p[m]["flip"][inv[mine]]
            assert (fa == fp).all() or (fa != fp).all()                              # the patch as a whole, or its mirror image
            if m == oc.ORIENT_FIRST:
                assert p[m]["flip"][p[m]["first_face"][cp]] == 0                     # FIRST follows the new label face
            elif m == oc.ORIENT_FEWEST and 2 * a[m]["n_flipped"][ca] != a[m]["n_faces"][ca]:
                assert (fa == fp).all()                                              # no tie: the decision does not look at the order
            elif m == oc.ORIENT_VIEWPOINT and a[m]["orientable"][ca]:
                votes = oc.view_sign(vtx, a[m]["faces"][mine], VIEW)
                if (votes > 0).sum() != (votes < 0).sum():
                    assert (fa == fp).all()
    assert a[0]["stats"]["n_patches"] > 80 and a[0]["stats"]["n_nonorientable"] >= 1


# ---- apply -----------------------------------------------------------------------------------------------------------------------------------------------------
def test_apply_equals_a_fresh_build_from_the_oriented_faces(hp):
    rng = np.random.default_rng(31)
    vtx, faces = tc.sheet_with_fragments(rng, 30, 20, 12, 40)
    vtx = vtx + rng.normal(scale=0.01, size=vtx.shape).astype(np.float32)              # off the plane: sides are decided, not ties
    vtx, faces = oc.with_moebius(vtx, oc.flip_random(rng, faces)[0], (9,), offset=3.0)
    dirs = (rng.normal(size=(2000, 3)) * np.array([0.3, 0.3, 1.0])).astype(np.float32)    # steep rays from a metre above the sheet (1.5 x 1.0)
    org = (rng.uniform(0.0, 1.0, (2000, 3)) * np.array([1.5, 1.0, 0.0]) + np.array([0.0, 0.0, 1.0])).astype(np.float32)
    dirs[:, 2] = -np.abs(dirs[:, 2]) - 0.5
    pts = np.concatenate([rng.uniform(-0.2, 1.7, (3000, 2)), rng.normal(scale=0.2, size=(3000, 1))], axis=1).astype(np.float32)
    other = make_hip(capi.load_hip_library(), _small_cfg())
    try:
        hp.raycast_build_triangles(vtx, faces)
        t0, f0 = hp.raycast(capi.ray_frame(), dirs, org, 0.0, 100.0)
        c0 = hp.closest_points(pts, 5.0)
        assert (f0 >= 0).sum() > 500 and (c0["side"] != 0).sum() > 2500
        assert hp.mesh_sample(300.0, 7, fetch=False) > 500 and len(hp.raycast_points(0.05)) > 100   # samples and a cast's points: the apply discards both
        before = _analysis(hp)
        ref = oc.orient(vtx, faces, oc.ORIENT_FEWEST)
        _same(_device(hp, oc.ORIENT_FEWEST), ref)
        assert 100 < ref["stats"]["n_faces_flipped"] and ref["stats"]["n_nonorientable"] == 1
        hp.topology_orient_apply()
        assert hp.topology_orient_timing()[0] > 0.0
        # everything a build discards is discarded
        for call in (hp.topology_faces, hp.topology_orient_faces, hp.topology_orient_patches, hp.topology_orient_apply, lambda: hp.topology_orient(0)):
            with pytest.raises(RuntimeError, match=r"rc=-1: .*no analysis"):
                call()
        with pytest.raises(RuntimeError, match=r"rc=-1: .*no NEAREST cast"):
            hp.raycast_points(0.05)
        with pytest.raises(RuntimeError, match=r"rc=-1: .*no samples"):
            hp.nearest_samples(1.0, want=())
        other.raycast_build_triangles(vtx, ref["faces"])
        assert hp._raycast_sizes() == other._raycast_sizes()
        # rays: equal to the fresh build's and to the cast before the apply, bit for bit
        t1, f1 = hp.raycast(capi.ray_frame(), dirs, org, 0.0, 100.0)
        t2, f2 = other.raycast(capi.ray_frame(), dirs, org, 0.0, 100.0)
        assert t1.tobytes() == t2.tobytes() == t0.tobytes() and f1.tobytes() == f2.tobytes() == f0.tobytes()
        assert hp.raycast_points(0.05).tobytes() == other.raycast_points(0.05).tobytes()
        # closest points: equal to the fresh build's bit for bit.  Against the query before the apply: the side negates exactly on flipped winners
        # and an unflipped winner's outputs keep their bits.  A flipped face's closest point is immesh_closest.h's Face rule on (a, c, b): the same
        # six dot products under other names, but va + vb + vc and a + ab v + ac w are summed in another order, a few double roundings on d2
        # (bound here: 16 ulp), so dist and xyz move by one float at the most, and a point that lies as near to two faces (their common edge) may
        # change its winner.
        c1, c2 = hp.closest_points(pts, 5.0), other.closest_points(pts, 5.0)
        assert all(c1[k].tobytes() == c2[k].tobytes() for k in c1)
        same = (c0["face"] >= 0) & (c1["face"] == c0["face"])
        assert (c0["face"] >= 0).all() and (~same).sum() <= len(pts) // 100
        flipped = same & (ref["flip"][np.maximum(c0["face"], 0)] != 0)
        kept = same & ~flipped
        assert flipped.sum() > 100 and np.array_equal(c1["side"][flipped], -c0["side"][flipped]) and (c0["side"][flipped] != 0).sum() > 100
        assert all(c1[k][kept].tobytes() == c0[k][kept].tobytes() for k in c0)
        assert (np.abs(c1["d2"][flipped] - c0["d2"][flipped]) <= 2.0 ** -48 * c0["d2"][flipped]).all()
        assert (np.abs(c1["dist"][flipped] - c0["dist"][flipped]) <= np.spacing(c0["dist"][flipped])).all()
        assert (np.abs(c1["xyz"][flipped] - c0["xyz"][flipped]) <= np.spacing(np.abs(c0["xyz"][flipped]))).all()
        # the sampler and a fresh analysis
        s1, s2 = hp.mesh_sample(300.0, 7), other.mesh_sample(300.0, 7)
        assert len(s1[0]) > 500 and s1[0].tobytes() == s2[0].tobytes() and s1[1].tobytes() == s2[1].tobytes()
        after, fresh = _analysis(hp), _analysis(other)
        _same_analysis(after, fresh)
        _same_analysis(after, tc.analyse(vtx, ref["faces"]))
        assert after["stats"]["n_inconsistent"] == ref["stats"]["n_inconsistent_after"] >= 1
        assert {k: v for k, v in after["stats"].items() if k != "n_inconsistent"} == {k: v for k, v in before["stats"].items() if k != "n_inconsistent"}
        assert all(np.array_equal(after[k], before[k]) for k in ("comp", "first_face", "n_faces", "n_boundary", "box"))
        assert all(np.array_equal(x, y) for kind in (tc.EDGE_BOUNDARY, tc.EDGE_NONMANIFOLD) for x, y in zip(after["edges"][kind], before["edges"][kind]))
        # oriented once, a FIRST orientation flips nothing
        again = _device(hp, oc.ORIENT_FIRST)
        _same(again, oc.orient(vtx, ref["faces"], oc.ORIENT_FIRST))
        assert again["stats"]["n_faces_flipped"] == 0 and not again["flip"].any() and np.array_equal(again["faces"], ref["faces"])
    finally:
        other.close()


# ---- lifecycle and errors ------------------------------------------------------------------------------------------------------------------------------------
def test_lifecycle_and_argument_errors():
    h = make_hip(capi.load_hip_library(), _small_cfg())
    try:
        vtx, faces = tc.grid_sheet(3, 2)
        faces = oc.flip_random(np.random.default_rng(2), faces)[0]
        refs = {m: oc.orient(vtx, faces, m, VIEW) for m in oc.MODES}
        with pytest.raises(RuntimeError, match=r"rc=-1: .*built"):
            h.topology_orient(0)                                                      # before a build
        h.raycast_build_triangles(vtx, faces)
        with pytest.raises(RuntimeError, match=r"rc=-1: .*no analysis"):
            h.topology_orient(0)                                                      # before an analysis
        h.topology_analyse()
        fetches = (h.topology_orient_faces, h.topology_orient_patches, h.topology_orient_apply)
        for fetch in fetches:
            with pytest.raises(RuntimeError, match=r"rc=-1: .*no orientation"):
                fetch()                                                               # a fetch or an apply before an orient
        _same(_device(h, 0), refs[0])
        h.topology_analyse()
        for fetch in fetches:
            with pytest.raises(RuntimeError, match=r"rc=-1: .*no orientation"):
                fetch()                                                               # after a new analysis
        _same(_device(h, 1), refs[1])
        h.raycast_build_triangles(vtx, faces)
        for fetch in fetches:
            with pytest.raises(RuntimeError, match=r"rc=-1: .*no analysis"):
                fetch()                                                               # after a rebuild
        h.topology_analyse()

        def still_usable():
            for m in oc.MODES:
                _same(_device(h, m, VIEW), refs[m])

        still_usable()
        for mode in (-1, 3, 99):
            with pytest.raises(RuntimeError, match=r"rc=-1: .*mode"):
                h.topology_orient(mode)
            still_usable()
        with pytest.raises(RuntimeError, match=r"rc=-1: .*viewpoint"):
            h.topology_orient(oc.ORIENT_VIEWPOINT)                                    # no viewpoint
        for bad in ((np.nan, 0, 0), (0, np.inf, 0), (0, 0, -np.inf), (2.0 ** 128, 0, 0), (0, -2.0 ** 128, 0)):
            with pytest.raises(RuntimeError, match=r"rc=-1: .*viewpoint"):
                h.topology_orient(oc.ORIENT_VIEWPOINT, bad)
            still_usable()
        big = float(np.nextafter(2.0 ** 128, 0.0))
        _same(_device(h, oc.ORIENT_VIEWPOINT, (big, -big, big)), oc.orient(vtx, faces, oc.ORIENT_VIEWPOINT, (big, -big, big)))
        o = h.lib.immesh_topology_orient; o.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
        assert o(None, 0, None, None) == -1 and o(h.raycaster(), 0, None, None) == 0   # stats may be NULL
        nan3 = np.full(3, np.nan)
        assert o(h.raycaster(), 1, nan3.ctypes.data_as(C.c_void_p), None) == 0         # the viewpoint is read with VIEWPOINT only
        n = C.c_int64(-5)
        g = h.lib.immesh_topology_orient_patches; g.argtypes = [C.c_void_p] + [C.c_void_p] * 5 + [C.c_int64, C.c_void_p]
        assert g(h.raycaster(), None, None, None, None, None, -1, C.byref(n)) == -1 and b"cap" in _err(h)
        n_p = refs[1]["stats"]["n_patches"]
        first = np.zeros(n_p + 1, np.int32)
        assert g(h.raycaster(), first.ctypes.data_as(C.c_void_p), None, None, None, None, n_p - 1, C.byref(n)) == -4 and n.value == n_p
        assert b"cap %d < %d" % (n_p - 1, n_p) in _err(h)
        n = C.c_int64(-5)
        assert g(h.raycaster(), first.ctypes.data_as(C.c_void_p), None, None, None, None, n_p, C.byref(n)) == 0 and n.value == n_p
        assert first[:n_p].tolist() == refs[1]["first_face"].tolist()
        assert g(h.raycaster(), None, None, None, None, None, 0, None) == 0            # every output may be NULL
        f = h.lib.immesh_topology_orient_faces; f.argtypes = [C.c_void_p] * 4
        assert f(h.raycaster(), None, None, None) == 0 and f(None, None, None, None) == -1
        flip = np.zeros(len(faces), np.int8)
        assert f(h.raycaster(), None, flip.ctypes.data_as(C.c_void_p), None) == 0 and np.array_equal(flip, refs[1]["flip"])
        a = h.lib.immesh_topology_orient_apply; a.argtypes = [C.c_void_p]
        assert a(None) == -1
        t = h.lib.immesh_topology_orient_last_timing; t.argtypes = [C.c_void_p, C.c_void_p]
        assert t(h.raycaster(), None) == -1 and h.topology_orient_timing()[0] > 0.0
        still_usable()
        # a caster with zero faces orients to all zeros, and applies
        h.raycast_build_triangles(vtx, np.zeros((0, 3), np.int32))
        h.topology_analyse()
        for m in oc.MODES:
            got = _device(h, m, VIEW)
            assert all(v == 0 for v in got["stats"].values()) and len(got["patch"]) == 0 and len(got["first_face"]) == 0 and got["faces"].shape == (0, 3)
        h.topology_orient_apply()
        h.raycast_build_triangles(vtx, faces)
        h.topology_analyse()
        still_usable()
    finally:
        h.close()


# ---- the live mesh ---------------------------------------------------------------------------------------------------------------------------------------------
def test_live_mesh_oriented_without_side_effects():
    """a orients its snapshot of the live mesh towards the last sensor position and applies it, b never does: a's answers equal the checker on the
    exported arrays, and both contexts go on to the same mesh and plane table"""
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
        R, t = synth.trajectory_pose(3)
        sensor = np.asarray(R, np.float64) @ extT + np.asarray(t, np.float64)
        a.topology_analyse()
        ref = oc.orient(vtx, faces, oc.ORIENT_VIEWPOINT, sensor)
        _same(_device(a, oc.ORIENT_VIEWPOINT, sensor), ref, "live mesh")
        st = ref["stats"]
        print("live mesh: %d faces, %d patches (largest %d), %d non-orientable with %d faces, %d faces flipped, %d patches inverted, inconsistent %d -> %d; "
              "orient %.3f ms" % (nf, st["n_patches"], st["largest_patch_faces"], st["n_nonorientable"], st["n_faces_nonorientable"], st["n_faces_flipped"],
                                  st["n_patches_inverted"], st["n_inconsistent_before"], st["n_inconsistent_after"], a.topology_orient_timing()[0]))
        a.topology_orient_apply()
        _same_analysis(_analysis(a), tc.analyse(vtx, ref["faces"]), "the oriented snapshot")
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
    """the 320 x 320 sheet with 300 holes plus 2 000 fragments, half the faces flipped at random, faces shuffled: about 209 000 faces"""
    rng = np.random.default_rng(51)
    vtx, faces = tc.sheet_with_fragments(rng, 320, 320, 300, 2000)
    faces = oc.flip_random(rng, faces)[0]
    assert len(faces) > 200000
    refs = _check(hp, vtx, faces, (oc.ORIENT_FEWEST, oc.ORIENT_VIEWPOINT), o=(8.0, 8.0, 40.0))
    print("%d faces: orient %.3f ms (the analysis before it %.3f ms)" % (len(faces), hp.topology_orient_timing()[0], hp.topology_timing()[0]))
    st = refs[oc.ORIENT_VIEWPOINT]["stats"]
    assert st["n_patches"] == 2001 and st["n_nonorientable"] == 0 and st["largest_patch_faces"] == 2 * (320 * 320 - 300) and st["n_inconsistent_before"] > 100000
    assert 90000 < refs[oc.ORIENT_FEWEST]["stats"]["n_faces_flipped"] <= len(faces) // 2
    hp.topology_orient_apply()
    print("apply %.3f ms" % hp.topology_orient_timing()[1])
    assert hp.topology_analyse().n_inconsistent == 0


# ---- tools/mesh_eval.py --------------------------------------------------------------------------------------------------------------------------------------------
def test_mesh_eval_orients_the_square(tmp_path, monkeypatch, capsys):
    spec = importlib.util.spec_from_file_location("mesh_eval", os.path.join(ROOT, "tools", "mesh_eval.py"))
    mesh_eval = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mesh_eval)
    square = np.array([[0, 0, 0], [2, 0, 0], [2, 2, 0], [0, 2, 0]], np.float32)
    rng = np.random.default_rng(3)
    cloud = np.concatenate([rng.uniform(0, 2, (4000, 2)), np.abs(rng.normal(scale=0.02, size=(4000, 1)))], axis=1).astype(np.float32)   # on and above the square
    np.save(tmp_path / "cloud.npy", cloud)
    _write_ply(tmp_path / "against.ply", square, np.array([[0, 1, 2], [0, 3, 2]], np.int32))    # wound against each other
    _write_ply(tmp_path / "alike.ply", square, np.array([[0, 1, 2], [0, 2, 3]], np.int32))

    def run(ply, *more):
        out = tmp_path / "out.json"
        monkeypatch.setattr(sys, "argv", ["mesh_eval.py", "--cloud", str(tmp_path / "cloud.npy"), "--ply", str(tmp_path / ply), "--out", str(out)] + list(more))
        mesh_eval.main()
        printed = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
        res = json.load(open(out))
        assert printed == res
        return res

    plain = run("against.ply")
    assert "orientation" not in plain and "signed" not in plain and "topology" not in plain    # the option off: the output as it was
    assert list(plain) == ["tau", "max_dist", "density", "seed", "samples", "cloud_points", "cloud_points_indexed", "accuracy", "completeness", "chamfer",
                           "precision", "recall", "f_score", "mesh"]
    alike = run("alike.ply")
    above = run("against.ply", "--orient", "viewpoint", "--viewpoint", "1", "1", "5", "--topology")
    below = run("against.ply", "--orient", "viewpoint", "--viewpoint", "1", "1", "-5")
    # from above the second face is flipped: the evaluated mesh is alike.ply's, figure for figure (repr round-trips a double)
    assert {k: json.dumps(v) for k, v in above.items() if k in alike} == {k: json.dumps(v) for k, v in alike.items()}
    for res in (above, below):
        for k in ("recall", "cloud_points", "cloud_points_indexed", "mesh"):                                                 # distances to the mesh look at the
            assert json.dumps(res[k]) == json.dumps(plain[k]), k                                                             # winding in their last bits only
        assert all(res["accuracy"][k] == pytest.approx(plain["accuracy"][k], rel=1e-6) for k in plain["accuracy"])              # (the sampler does look)
        assert res["orientation"]["n_patches"] == 1 and res["orientation"]["n_faces_flipped"] == 1 and res["orientation"]["n_inconsistent_before"] == 1
        assert res["orientation"]["n_inconsistent_after"] == 0 and res["orientation"]["mode"] == "viewpoint"
        sg = res["signed"]
        assert sg["points_with_face"] == 4000 == sg["front"] + sg["behind"] + sg["in_plane"]
    assert above["topology"]["n_inconsistent"] == 0 and "topology" not in below
    assert above["signed"]["behind"] == 0 and above["signed"]["front"] > 3000 and above["signed"]["signed_mean"] > 0
    assert below["signed"]["front"] == 0 and below["signed"]["behind"] == above["signed"]["front"] and below["signed"]["in_plane"] == above["signed"]["in_plane"]
    assert below["signed"]["signed_mean"] == -above["signed"]["signed_mean"]
    first = run("against.ply", "--orient", "first")
    assert first["orientation"]["mode"] == "first" and "viewpoint" not in first["orientation"] and first["signed"]["front"] in (0, above["signed"]["front"])
    with pytest.raises(SystemExit):
        run("against.ply", "--orient", "viewpoint")
    capsys.readouterr()
