"""The self-intersection pass on the device (include/immesh_intersect.h) against the numpy restatements of the contract (tests/intersect_checker.py),
bit for bit on every output: the stats, the pairs, the masks, n_partners and face_map.  Two crossing faces in every vertex and index order, shared
vertices, closed ends and ties, the sizes where a launch gains a wavefront or a workgroup (faces, candidates, hits), one face with 300 partners, 300
copies of one face, order-freedom, the cap, the apply against a caster freshly built from the kept faces, every error and capacity path, the live
mesh as a snapshot without side effects, tools/mesh_eval.py's two options, and scale.  Soups of up to 400 faces go through both checkers."""
import ctypes as C
import importlib.util
import json
import os
import sys
import time

import numpy as np
import pytest

import intersect_checker as ic
import topology_checker as tc
from immesh_amd import capi, synth
from conftest import make_hip
from parity_utils import compare_plane_tables_fast
from test_gpu_render import _small_cfg
from test_gpu_topology import _write_ply

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = r"rc=-1: .*no self-intersection pass"


@pytest.fixture(scope="module")
def hp():
    h = make_hip(capi.load_hip_library(), _small_cfg())
    yield h
    h.close()


def _err(h):
    f = h.lib.immesh_last_error; f.restype = C.c_char_p; f.argtypes = [C.c_void_p]
    return f(h.ctx)


def _stats(st):
    return {n: (list(st.n_share) if n == "n_share" else getattr(st, n)) for n in ic.STAT_NAMES}


def _device(h, cap=ic.CAP):
    """the pass, then every fetch, in the checker's shape"""
    out = {"stats": _stats(h.self_intersect(cap))}
    out["pairs"], out["mask"] = h.self_intersect_pairs()
    out.update(h.self_intersect_faces())
    return out


def _check(h, vtx, faces, what="", ref=None):
    """build, and the pass against the checker (both checkers on a small soup) -> the checker's result"""
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    h.raycast_build_triangles(vtx, faces)
    if ref is None:
        ref = ic.both(vtx, faces, what) if len(faces) <= 400 else ic.grid(vtx, faces)
    assert ref["stats"]["n_candidates"] <= ic.CAP
    ic.same(_device(h), ref, what)
    return ref


# ---- two crossing faces and vertex orders ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["one_edge_of_each", "two_edges_of_the_second"])
def test_two_crossing_faces_in_every_vertex_order_and_both_index_orders(hp, which):
    """a crossing in general position has two ends, so a pair without a common vertex sets two bits; every bit is seen in its position, rotating a
    face's indices rotates its three bits and swapping the faces swaps the halves (single bits: the next test)"""
    faces, base = {"one_edge_of_each": (ic.CROSS_ONE_EACH, 0b001010), "two_edges_of_the_second": (ic.CROSS_TWO_OF_B, 0b101000)}[which]
    seen = 0
    for swap in (False, True):
        for ra in range(3):
            for rb in range(3):
                a, b = np.roll(faces[0], -ra), np.roll(faces[1], -rb)
                ref = _check(hp, ic.CROSS_VTX, np.stack([b, a] if swap else [a, b]), (which, swap, ra, rb))
                want = ic.rotate_mask(base, ra, rb)
                want = ic.swap_mask(want) if swap else want
                assert ref["mask"].tolist() == [want] and ref["pairs"].tolist() == [[0, 1]] and ref["stats"]["n_pairs_share0"] == 1
                seen |= want
    assert seen == 63


# ---- shared vertices -------------------------------------------------------------------------------------------------------------------------------------
def test_a_shared_vertex_pierced_and_not_pierced_sets_only_the_far_edges_bits(hp):
    seen = set()
    for swap in (False, True):
        for ra in range(3):
            for rb in range(3):
                a, b = np.roll(ic.FAN_PIERCED[0], -ra), np.roll(ic.FAN_PIERCED[1], -rb)
                ref = _check(hp, ic.FAN_VTX, np.stack([b, a] if swap else [a, b]), ("fan", swap, ra, rb))
                want = ic.rotate_mask(2, ra, rb)
                want = ic.swap_mask(want) if swap else want
                assert ref["mask"].tolist() == [want] and ref["stats"]["n_share"] == [0, 1, 0, 0] and ref["stats"]["n_pairs_share1"] == 1
                seen.add(want)
                a = np.roll(ic.FAN_NOT_PIERCED[0], -ra)
                ref = _check(hp, ic.FAN_VTX, np.stack([b, a] if swap else [a, b]))
                assert ref["stats"]["n_share"] == [0, 1, 0, 0] and ref["stats"]["n_pairs"] == 0 and ref["n_partners"].tolist() == [0, 0]
    assert seen == {1, 2, 4, 8, 16, 32}                                                 # each mask bit alone, in its position


def test_edge_neighbours_duplicates_and_faces_that_take_no_part(hp):
    fold = np.array([[0, 0, 0], [4, 0, 0], [1, 3, 0], [2, 2, 0], [1, 1, -1], [1, 1, 1], [9, 9, 0.5], [np.nan, 0, 0], [1, 1, np.inf]], np.float32)
    ref = _check(hp, fold, [[0, 1, 2], [1, 0, 3]])                                      # folded flat onto its neighbour
    assert ref["stats"]["n_share"] == [0, 0, 1, 0] and ref["stats"]["n_pairs"] == 0
    ref = _check(hp, fold, [[0, 1, 2], [2, 0, 1], [1, 0, 2]])                           # the same three indices, rotated and wound back
    assert ref["stats"]["n_share"] == [0, 0, 0, 3] and ref["stats"]["n_pairs"] == 0
    # face 2 crosses faces 0 and 1; a face with a repeated index and two with a vertex that is not finite lie across them and take no part
    faces = np.array([[0, 1, 2], [1, 0, 3], [4, 5, 6], [4, 5, 4], [4, 5, 7], [8, 4, 6], [6, 6, 6]], np.int32)
    ref = _check(hp, fold, faces)
    st = ref["stats"]
    assert (st["n_faces"], st["n_in_tree"], st["n_taking_part"]) == (7, 5, 3) and st["n_pairs"] == 2 and ref["n_partners"].tolist() == [1, 1, 2, 0, 0, 0, 0]
    assert ref["face_map"].tolist() == [-1, -1, -1, 0, 1, 2, 3]
    hp.self_intersect_apply()                                                           # they were not judged: they stay
    assert hp._raycast_sizes() == (9, 4, 2)
    again = _device(hp)
    assert again["stats"]["n_taking_part"] == 0 and again["stats"]["n_candidates"] == 0 and again["n_partners"].tolist() == [0, 0, 0, 0]


# ---- closed ends and ties --------------------------------------------------------------------------------------------------------------------------------
TRI = np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0]], np.float32)


def _with(second):
    return np.concatenate([TRI, np.array(second, np.float32)]), np.array([[0, 1, 2], [3, 4, 5]], np.int32)


def test_closed_ends_zero_cover_terms_and_touching_boxes(hp):
    ref = _check(hp, *_with([[1, 1, 0], [1, 2, 3], [2, 1, 3]]), "an endpoint in the other face")   # s == 0 and s == 1; the boxes touch in z = 0
    assert ref["mask"].tolist() == [0b101000]
    ref = _check(hp, *_with([[0, 0, -1], [0, 0, 1], [-3, -3, 0]]), "an edge through a vertex")     # two Cover terms are 0
    assert ref["stats"]["n_pairs"] == 1 and ref["mask"][0] & 0b001000
    ref = _check(hp, *_with([[2, 0, -1], [2, 0, 1], [2, -3, 0]]), "an edge through an edge")       # one Cover term is 0
    assert ref["stats"]["n_pairs"] == 1 and ref["mask"][0] & 0b001000
    ref = _check(hp, *_with([[4, 0, 0], [8, 1, 2], [8, -1, 2]]), "boxes that touch in x = 4, the hit in that plane")
    assert ref["stats"]["n_candidates"] == 1 and ref["stats"]["n_pairs"] == 1
    # an edge that ends 2^-60 below the face: in double 1 - 2^-60 is 1, so the Segment rule alone finds s == 1; the boxes miss, and the pair never counts
    tiny = np.float32(2.0 ** -60)
    vtx, faces = _with([[1, 1, -1], [1, 1, -tiny], [2, 2, -1]])
    assert ic.hit(vtx[3], vtx[4], vtx[:3]) and vtx[3:, 2].max() < vtx[:3, 2].min()
    ref = _check(hp, vtx, faces, "boxes that miss, arithmetic that would hit")
    assert ref["stats"]["n_candidates"] == 0 and ref["stats"]["n_taking_part"] == 2
    ref = _check(hp, *_with([[1, 1, -1], [1, 1, 0], [2, 2, -1]]), "the same edge ending in the face")
    assert ref["stats"]["n_candidates"] == 1 and ref["mask"].tolist() == [0b011000]
    up = np.nextafter(np.float32(4), np.float32(5))                                     # boxes that miss by one float ulp in x
    ref = _check(hp, *_with([[up, 0, -1], [up, 0, 1], [5, 0, 0]]), "one ulp apart")
    assert ref["stats"]["n_candidates"] == 0
    ref = _check(hp, *_with([[4, 0, -1], [4, 0, 1], [5, 0, 0]]), "touching in x = 4: the edge passes through the vertex")
    assert ref["stats"]["n_candidates"] == 1 and ref["stats"]["n_pairs"] == 1


def test_coplanar_overlaps_are_candidates_and_not_pairs(hp):
    ref = _check(hp, np.concatenate([TRI, TRI + np.array([1, 1, 0], np.float32)]), [[0, 1, 2], [3, 4, 5]], "z = 0")
    assert ref["stats"]["n_share"] == [1, 0, 0, 0] and ref["stats"]["n_pairs"] == 0
    tilted = np.array([[6, 0, 0], [0, 6, 0], [0, 0, 6], [4, 1, 1], [1, 4, 1], [1, 1, 4]], np.float32)   # x + y + z = 6 in integers: every nd is exactly 0
    for faces in ([[0, 1, 2], [3, 4, 5]], [[3, 5, 4], [2, 0, 1]]):
        ref = _check(hp, tilted, faces, "an integer tilted plane")
        assert ref["stats"]["n_share"] == [1, 0, 0, 0] and ref["stats"]["n_pairs"] == 0


def test_touching_neighbours_count_unwelded_and_not_welded(hp):
    vtx, faces = ic.sheet(5, 4, lambda x, y: 0.25 * x * y)
    welded = _check(hp, vtx, faces, "welded")
    assert welded["stats"]["n_pairs"] == 0 and welded["stats"]["n_share"][2] > 0
    loose = _check(hp, *ic.unshared(vtx, faces), "unwelded")
    assert loose["stats"]["n_share"][1:] == [0, 0, 0] and loose["stats"]["n_faces_hit"] == len(faces) and loose["stats"]["n_candidates"] == welded["stats"]["n_candidates"]
    hp.simplify(0.0)                                                                    # the weld gives the indices back, and the pairs go
    hp.simplify_apply()
    again = _device(hp)
    assert again["stats"] == welded["stats"]


# ---- launch boundaries -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 255, 256, 257])
def test_crossing_strips_of_n_faces(hp, n):
    vtx, faces = ic.crossing_strips(n)
    ref = _check(hp, vtx, faces, n)
    assert ref["stats"]["n_faces"] == n and (n < 2 or ref["stats"]["n_pairs"] >= n // 2)
    if n < 2:
        assert ref["stats"] == dict(dict.fromkeys(ic.STAT_NAMES, 0), n_faces=1, n_in_tree=1, n_taking_part=1, n_share=[0, 0, 0, 0])


@pytest.mark.parametrize("n_hit,n_near", [(100, 155), (100, 156), (100, 157), (255, 0), (256, 0), (257, 0), (255, 40), (256, 40), (257, 40)])
def test_counted_candidates_and_counted_hits(hp, n_hit, n_near):
    rng = np.random.default_rng(n_hit + n_near)
    ref = _check(hp, *ic.big_and_small(n_hit, n_near, rng), (n_hit, n_near))
    st = ref["stats"]
    assert (st["n_candidates"], st["n_pairs"], st["max_partners"], st["n_faces_hit"]) == (n_hit + n_near, n_hit, n_hit, n_hit + 1)


def test_one_large_face_crossed_by_three_hundred_small_ones(hp):
    ref = _check(hp, *ic.big_and_small(300, 0))                                         # lane 0 counts 300: above a workgroup's width
    assert ref["stats"]["max_partners"] == 300 and ref["n_partners"][0] == 300 and ref["stats"]["n_candidates"] == 300
    ref = _check(hp, *ic.big_and_small(300, 0, np.random.default_rng(9)))               # the large face anywhere: it is i of some pairs and j of others
    assert ref["stats"]["max_partners"] == 300 and (ref["pairs"][:, 0] != ref["pairs"][0, 0]).any()


def test_three_hundred_copies_of_one_face(hp):
    vtx = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    ref = _check(hp, vtx, np.tile(np.array([[0, 1, 2]], np.int32), (300, 1)))           # the stack-depth soup of raycast.hpp
    assert ref["stats"]["n_share"] == [0, 0, 0, 44850] and ref["stats"]["n_pairs"] == 0
    ref = _check(hp, *ic.unshared(vtx, np.tile(np.array([[0, 1, 2]], np.int32), (300, 1))))
    assert ref["stats"]["n_share"] == [44850, 0, 0, 0] and ref["stats"]["n_pairs"] == 0   # coplanar, each fully evaluated


# ---- order-freedom -----------------------------------------------------------------------------------------------------------------------------------------
def test_a_permutation_of_the_faces_gives_the_same_pairs_and_a_second_build_the_same_bytes(hp):
    rng = np.random.default_rng(23)
    vtx, faces = ic.join(ic.crossing_sheets(rng, 14, 11), ic.jittered_sheet(rng, 12, 12))
    ref = _check(hp, vtx, faces)
    assert ref["stats"]["n_pairs_share0"] > 50 and ref["stats"]["n_pairs_share1"] > 0
    a = _device(hp)
    hp.raycast_build_triangles(vtx, faces)
    b = _device(hp)
    ic.same(a, b, "two builds")
    p = rng.permutation(len(faces))                                                     # new face k is old face p[k]
    per = _check(hp, vtx, faces[p])
    assert {k: v for k, v in per["stats"].items()} == ref["stats"] and np.array_equal(per["n_partners"], ref["n_partners"][p])
    old = {}
    for (i, j), m in zip(ref["pairs"].tolist(), ref["mask"].tolist()):
        old[(i, j)] = m
    for (i, j), m in zip(per["pairs"].tolist(), per["mask"].tolist()):
        oi, oj = int(p[i]), int(p[j])
        assert old.pop((oi, oj) if oi < oj else (oj, oi)) == (m if oi < oj else ic.swap_mask(m))
    assert not old


# ---- the cap ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_the_cap_on_the_candidates(hp):
    vtx, faces = ic.crossing_sheets(np.random.default_rng(4), 6, 5)
    ref = _check(hp, vtx, faces)
    n = ref["stats"]["n_candidates"]
    assert n > 100
    f = hp.lib.immesh_self_intersect; f.argtypes = [C.c_void_p, C.c_int64, C.POINTER(capi.IntersectStats)]; f.restype = C.c_int
    st = capi.IntersectStats()
    st.n_pairs = -7
    assert f(hp.raycaster(), n - 1, C.byref(st)) == -4 and b"self_intersect: cap %d < %d candidate pairs" % (n - 1, n) in _err(hp)
    assert (st.n_faces, st.n_in_tree, st.n_taking_part, st.n_candidates) == tuple(ref["stats"][k] for k in ("n_faces", "n_in_tree", "n_taking_part", "n_candidates"))
    for fetch in (hp.self_intersect_pairs, hp.self_intersect_faces, hp.self_intersect_apply):
        with pytest.raises(RuntimeError, match=NONE):
            fetch()                                                                     # no result exists, not even the last pass'
    assert f(hp.raycaster(), 1, None) == -4 and f(hp.raycaster(), n, C.byref(st)) == 0 and _stats(st) == ref["stats"]
    ic.same(_device(hp, n), ref, "at the count")


# ---- the apply -----------------------------------------------------------------------------------------------------------------------------------------------------
def test_apply_equals_a_fresh_build_from_the_kept_faces(hp):
    rng = np.random.default_rng(31)
    vtx, faces = ic.join(ic.crossing_sheets(rng, 20, 15), ic.jittered_sheet(rng, 10, 10))
    faces = np.concatenate([faces, np.array([[0, 0, 1]], np.int32)])                    # one that takes no part and stays
    dirs = (rng.normal(size=(2000, 3)) * np.array([0.3, 0.3, 1.0])).astype(np.float32)
    org = (rng.uniform(0.0, 1.0, (2000, 3)) * np.array([20.0, 15.0, 0.0]) + np.array([0.0, 0.0, 9.0])).astype(np.float32)
    dirs[:, 2] = -np.abs(dirs[:, 2]) - 0.5
    pts = np.concatenate([rng.uniform(-1.0, 21.0, (3000, 2)), rng.normal(scale=2.0, size=(3000, 1))], axis=1).astype(np.float32)
    other = make_hip(capi.load_hip_library(), _small_cfg())
    try:
        loops_before = tc.analyse(vtx, faces)["stats"]["n_boundary_loops"]
        ref = _check(hp, vtx, faces)
        assert ref["stats"]["n_faces_hit"] > 50 and ref["face_map"][-1] >= 0
        hp.raycast(capi.ray_frame(), dirs, org, 0.0, 100.0)
        assert hp.mesh_sample(2.0, 7, fetch=False) > 100 and len(hp.raycast_points(0.05)) > 100   # samples and a cast's points: the apply discards both
        hp.topology_analyse()
        hp.simplify(0.0)
        hp.self_intersect_apply()
        assert hp.self_intersect_timing()[2] > 0.0
        for call in (hp.self_intersect_pairs, hp.self_intersect_faces, hp.self_intersect_apply):
            with pytest.raises(RuntimeError, match=NONE):
                call()                                                                  # a fetch after the apply
        with pytest.raises(RuntimeError, match=r"rc=-1: .*no analysis"):
            hp.topology_faces()
        with pytest.raises(RuntimeError, match=r"rc=-1: .*no simplify pass"):
            hp.simplify_faces()
        with pytest.raises(RuntimeError, match=r"rc=-1: .*no NEAREST cast"):
            hp.raycast_points(0.05)
        with pytest.raises(RuntimeError, match=r"rc=-1: .*no samples"):
            hp.nearest_samples(1.0, want=())
        other.raycast_build_triangles(vtx, ref["kept"])
        assert hp._raycast_sizes() == other._raycast_sizes() and hp._raycast_sizes()[:2] == (len(vtx), len(ref["kept"]))
        t1, f1 = hp.raycast(capi.ray_frame(), dirs, org, 0.0, 100.0)
        t2, f2 = other.raycast(capi.ray_frame(), dirs, org, 0.0, 100.0)
        assert t1.tobytes() == t2.tobytes() and f1.tobytes() == f2.tobytes() and (f1 >= 0).sum() > 500
        assert hp.raycast_points(0.05).tobytes() == other.raycast_points(0.05).tobytes()
        c1, c2 = hp.closest_points(pts, 50.0), other.closest_points(pts, 50.0)
        assert all(c1[k].tobytes() == c2[k].tobytes() for k in c1) and (c1["face"] >= 0).all()
        s1, s2 = hp.mesh_sample(2.0, 7), other.mesh_sample(2.0, 7)
        assert len(s1[0]) > 100 and s1[0].tobytes() == s2[0].tobytes() and s1[1].tobytes() == s2[1].tobytes()
        again = _device(hp)                                                             # a kept face had no partner, and removal creates none
        ic.same(again, ic.grid(vtx, ref["kept"]), "after the apply")
        assert again["stats"]["n_pairs"] == 0 and again["stats"]["n_faces"] == len(ref["kept"])
        want = tc.analyse(vtx, ref["kept"])["stats"]
        st = hp.topology_analyse()
        assert st.n_boundary_loops == want["n_boundary_loops"] > loops_before          # the loops the removal opened
        assert hp.topology_holes(64).n_loops == want["n_boundary_loops"]
    finally:
        other.close()


# ---- fetches and errors --------------------------------------------------------------------------------------------------------------------------------------------
def test_fetches_lifecycle_and_argument_errors():
    h = make_hip(capi.load_hip_library(), _small_cfg())
    try:
        vtx, faces = ic.crossing_sheets(np.random.default_rng(4), 6, 5)
        ref = ic.both(vtx, faces)
        n_p, n_f = ref["stats"]["n_pairs"], len(faces)
        assert n_p > 5
        fetches = (h.self_intersect_pairs, h.self_intersect_faces, h.self_intersect_apply)
        with pytest.raises(RuntimeError, match=r"rc=-1: .*built"):
            h.self_intersect()                                                          # before a build
        for fetch in fetches:
            with pytest.raises(RuntimeError, match=r"rc=-1: .*built"):
                fetch()
        h.raycast_build_triangles(vtx, faces)
        for fetch in fetches:
            with pytest.raises(RuntimeError, match=NONE):
                fetch()                                                                 # a fetch or an apply before a pass

        def still_usable():
            ic.same(_device(h), ref)

        still_usable()
        for bad in (0, -1, 2 ** 31 - 1, 2 ** 40, -2 ** 63):
            with pytest.raises(RuntimeError, match=r"rc=-1: .*max_candidates"):
                h.self_intersect(bad)
            assert h.self_intersect_pairs()[0].tobytes() == ref["pairs"].tobytes()      # refused before anything was touched: the last pass stays
        f = h.lib.immesh_self_intersect; f.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]; f.restype = C.c_int
        assert f(None, 100, None) == -1 and f(h.raycaster(), 2 ** 31 - 2, None) == 0    # stats may be NULL; the largest cap
        # pairs
        g = h.lib.immesh_self_intersect_pairs; g.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]; g.restype = C.c_int
        n = C.c_int64(-5)
        assert g(h.raycaster(), None, None, -1, C.byref(n)) == -1 and b"self_intersect_pairs: cap is negative" in _err(h)
        assert g(None, None, None, 0, None) == -1 and g(h.raycaster(), None, None, 0, None) == 0
        assert g(h.raycaster(), None, None, 0, C.byref(n)) == 0 and n.value == n_p
        for which, k in enumerate(("pairs", "mask")):
            room = np.zeros((n_p + 1,) + ref[k].shape[1:], ref[k].dtype)
            args = [None] * 2
            args[which] = room.ctypes.data_as(C.c_void_p)
            n = C.c_int64(-5)
            assert g(h.raycaster(), *args, n_p - 1, C.byref(n)) == -4 and n.value == n_p and b"self_intersect_pairs: cap %d < %d pairs" % (n_p - 1, n_p) in _err(h)
            assert not room.any()
            assert g(h.raycaster(), *args, n_p, C.byref(n)) == 0 and n.value == n_p and room[:n_p].tobytes() == ref[k].tobytes() and not room[n_p:].any()
        # faces
        g = h.lib.immesh_self_intersect_faces; g.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]; g.restype = C.c_int
        assert g(None, None, None) == -1 and g(h.raycaster(), None, None) == 0
        for which, k in enumerate(("n_partners", "face_map")):
            room = np.zeros(n_f + 1, np.int32)
            args = [None] * 2
            args[which] = room.ctypes.data_as(C.c_void_p)
            assert g(h.raycaster(), *args) == 0 and np.array_equal(room[:-1], ref[k]) and room[-1] == 0
        a = h.lib.immesh_self_intersect_apply; a.argtypes = [C.c_void_p]; a.restype = C.c_int
        assert a(None) == -1
        t = h.lib.immesh_self_intersect_last_timing; t.argtypes = [C.c_void_p, C.c_void_p]; t.restype = C.c_int
        ms = h.self_intersect_timing()
        assert t(h.raycaster(), None) == -1 and t(None, None) == -1 and ms[0] > 0.0 and ms[1] > 0.0
        still_usable()
        h.raycast_build_triangles(vtx, faces)                                           # a rebuild discards the result
        for fetch in fetches:
            with pytest.raises(RuntimeError, match=NONE):
                fetch()
        still_usable()
        # nothing to do: zero faces, and an apply of them
        h.raycast_build_triangles(vtx, np.zeros((0, 3), np.int32))
        got = _device(h)
        assert got["stats"] == dict(dict.fromkeys(ic.STAT_NAMES, 0), n_share=[0, 0, 0, 0]) and len(got["pairs"]) == 0 and len(got["n_partners"]) == 0
        h.self_intersect_apply()
        assert h._raycast_sizes() == (len(vtx), 0, 0)
    finally:
        h.close()


# ---- the live mesh -----------------------------------------------------------------------------------------------------------------------------------------------
def test_live_mesh_checked_and_cleaned_without_side_effects():
    """a looks for the self-intersections of its snapshot of the live mesh and applies, b never does: a's answers equal the checker on the exported
    arrays, and both contexts go on to the same mesh and plane table"""
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
        ref = ic.grid(vtx, faces)
        ic.same(_device(a), ref, "live mesh")
        st = ref["stats"]
        print("live mesh: %d faces, %d candidates (%.2f per face), %d pairs over %d faces; candidates %.3f ms, tests %.3f ms"
              % ((nf, st["n_candidates"], st["n_candidates"] / nf, st["n_pairs"], st["n_faces_hit"]) + a.self_intersect_timing()[:2]))
        a.self_intersect_apply()
        assert a._raycast_sizes()[1] == nf - st["n_faces_hit"] and _device(a)["stats"]["n_pairs"] == 0
        assert compare_plane_tables_fast(planes, a.dump_planes(), 0.0) > 100 and a.counters() == counters
        for k in range(4, 6):
            scan(k)
        ea, eb = a.mesh_export(1.0, 20), b.mesh_export(1.0, 20)
        assert len(ea[1]) != len(faces) and ea[0].tobytes() == eb[0].tobytes() and ea[1].tobytes() == eb[1].tobytes()
        assert compare_plane_tables_fast(a.dump_planes(), b.dump_planes(), 0.0) > 100
    finally:
        a.close(); b.close()


# ---- tools/mesh_eval.py ------------------------------------------------------------------------------------------------------------------------------------------
def test_mesh_eval_reports_and_removes_self_intersections(tmp_path, monkeypatch, capsys):
    spec = importlib.util.spec_from_file_location("mesh_eval", os.path.join(ROOT, "tools", "mesh_eval.py"))
    mesh_eval = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mesh_eval)
    rng = np.random.default_rng(3)
    vtx, faces = ic.crossing_sheets(rng, 8, 6)
    ref = ic.both(vtx, faces)
    _write_ply(tmp_path / "crossed.ply", vtx, faces)
    cloud = np.concatenate([rng.uniform(0, 1, (4000, 2)) * np.array([8.0, 6.0]), np.zeros((4000, 1))], axis=1)
    np.save(tmp_path / "cloud.npy", cloud.astype(np.float32))

    def run(*more):
        out = tmp_path / "out.json"
        monkeypatch.setattr(sys, "argv", ["mesh_eval.py", "--cloud", str(tmp_path / "cloud.npy"), "--ply", str(tmp_path / "crossed.ply"), "--out", str(out)] + list(more))
        mesh_eval.main()
        printed = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
        res = json.load(open(out))
        assert printed == res
        return res

    plain = run()
    assert list(plain) == ["tau", "max_dist", "density", "seed", "samples", "cloud_points", "cloud_points_indexed", "accuracy", "completeness", "chamfer",
                           "precision", "recall", "f_score", "mesh"]                    # the options off: the output as it was
    seen = run("--self-intersections")
    assert seen["intersections"] == dict(ref["stats"], max_candidates=1 << 24) and {k: v for k, v in seen.items() if k != "intersections"} == plain
    gone = run("--remove-self-intersections", "--self-intersections", "--topology", "--max-candidates", "100000")
    assert gone["intersections_removed"] == dict(ref["stats"], max_candidates=100000, faces_before=len(faces), faces_removed=ref["stats"]["n_faces_hit"])
    after = ic.both(vtx, ref["kept"])["stats"]
    assert gone["intersections"] == dict(after, max_candidates=100000) and after["n_pairs"] == 0
    assert gone["mesh"]["faces"] == len(ref["kept"]) and gone["topology"]["n_boundary_loops"] == tc.analyse(vtx, ref["kept"])["stats"]["n_boundary_loops"]
    kept = run("--remove-self-intersections", "--min-component-faces", "1", "--fill-holes", "64")   # the filter and the fill see the holes it left
    assert kept["filter"]["faces_before"] == len(ref["kept"]) and kept["holes"]["n_loops"] == gone["topology"]["n_boundary_loops"]
    for bad in (["--max-candidates", "5"], ["--self-intersections", "--max-candidates", "0"]):
        with pytest.raises((SystemExit, RuntimeError)):
            run(*bad)
    capsys.readouterr()


# ---- scale -----------------------------------------------------------------------------------------------------------------------------------------------------------
def test_scale(hp):
    """two crossing noisy sheets of 158 x 158 cells, 99 856 faces in all, against the grid checker: equality only"""
    rng = np.random.default_rng(51)
    vtx, faces = ic.crossing_sheets(rng, 158, 158)
    faces = faces[rng.permutation(len(faces))]
    assert len(faces) == 99856
    t0 = time.perf_counter()
    ref = _check(hp, vtx, faces)
    st = ref["stats"]
    print("%d faces, %d candidates, %d pairs: candidates %.3f ms, tests %.3f ms; the checker and the device together %.1f s"
          % ((len(faces), st["n_candidates"], st["n_pairs"]) + hp.self_intersect_timing()[:2] + (time.perf_counter() - t0,)))
    assert st["n_pairs"] > 500 and st["n_candidates"] > 5 * len(faces)
