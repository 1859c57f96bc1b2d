"""CPU tier of the manifold pass (include/immesh_topology.h, the Manifold rule): the header as plain C99 with the new declarations, the library's new
symbols, immesh_manifold_stats' layout, and the checker (tests/manifold_checker.py) against a brute force that shares nothing with it, against
closed forms counted by hand, and against the Invariant that makes the contract checkable: an analysis of (vtx_out, faces_out) has no non-manifold
edge and as many used vertices as there were fans, a second pass moves nothing, and after the orientation no boundary loop is left non-simple."""
import ctypes as C
import os
import re
import subprocess
from collections import deque

import numpy as np
import pytest

import holes_checker as hc
import manifold_checker as mc
import orient_checker as oc
import topology_checker as tc
from immesh_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "immesh_topology.h")
NEW_SYMBOLS = ("immesh_topology_manifold", "immesh_topology_manifold_vertices", "immesh_topology_manifold_fans", "immesh_topology_manifold_faces",
               "immesh_topology_manifold_new_vertices", "immesh_topology_manifold_apply", "immesh_topology_manifold_last_timing")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(capi.hip_library_path()):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "immesh_amd", "csrc"), "-j8"])
    return capi.load_hip_library()


# ---- the boundary ----------------------------------------------------------------------------------------------------------------------------
def test_header_is_plain_c99_with_the_manifold_pass(tmp_path):
    src = tmp_path / "alone.c"
    src.write_text('#include "immesh_topology.h"\nint main(void) { immesh_manifold_stats s; float ms[2]; int rc;\n'
                   '  rc = immesh_topology_manifold(0, &s) + immesh_topology_manifold_vertices(0, 0) + immesh_topology_manifold_fans(0, 0, 0, 0, 0, 0, 0, 0)\n'
                   '     + immesh_topology_manifold_faces(0, 0, 0) + immesh_topology_manifold_new_vertices(0, 0, 0, 0, 0) + immesh_topology_manifold_apply(0)\n'
                   '     + immesh_topology_manifold_last_timing(0, ms);\n'
                   '  return rc + (int)s.n_fans; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "alone.o")])


def test_library_exports_the_manifold_pass(lib):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    fns = sorted(set(re.findall(r"\b(immesh_[a-z_0-9]+)\s*\(", src)))
    for must in NEW_SYMBOLS:
        assert must in fns
    missing = [f for f in fns if not hasattr(lib, f)]
    assert not missing, missing


def test_manifold_stats_layout(tmp_path):
    names = [n for n, _ in capi.ManifoldStats._fields_]
    assert tuple(names) == mc.STAT_NAMES
    prog = tmp_path / "layout.c"
    prog.write_text('#include "immesh_topology.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void) {\n  printf("%zu", sizeof(immesh_manifold_stats));\n'
                    + "".join('  printf(" %%zu", offsetof(immesh_manifold_stats, %s));\n' % n for n in names) + "  return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(prog), "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe]).split()]
    assert got == [C.sizeof(capi.ManifoldStats)] + [getattr(capi.ManifoldStats, n).offset for n in names]
    assert got == [96] + [8 * i for i in range(12)]
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.findall(r"int64_t (\w+);", re.search(r"typedef struct immesh_manifold_stats \{(.*?)\}", text, re.S).group(1)) == names


# ---- a brute force that shares nothing with the checker ----------------------------------------------------------------------------------------------
def _brute(faces, n_vtx):
    """per vertex the set of incident counting faces, adjacency by "the two users of a two-use edge at this vertex" with Python sets, a breadth-first
    search -> the fans as sorted (vertex, label, faces of the fan, links) tuples"""
    F = [tuple(int(x) for x in f) for f in np.asarray(faces).reshape(-1, 3)]
    ok = [f for f in range(len(F)) if len(set(F[f])) == 3]
    fans = []
    for v in range(n_vtx):
        at = {f for f in ok if v in F[f]}
        adj = {f: set() for f in at}
        n_link_edges = {}
        for w in range(n_vtx):
            if w == v:
                continue
            on = [f for f in ok if v in F[f] and w in F[f]]                              # the users of {v, w}: a counting face uses an edge once
            if len(on) == 2:
                adj[on[0]].add(on[1])
                adj[on[1]].add(on[0])
                n_link_edges[frozenset(on)] = n_link_edges.get(frozenset(on), 0) + 1
        left = set(at)
        while left:
            first = min(left)
            seen, todo = {first}, deque([first])
            while todo:
                for g in adj[todo.popleft()] - seen:
                    seen.add(g)
                    todo.append(g)
            left -= seen
            fans.append((v, first, tuple(sorted(seen)), sum(n for pair, n in n_link_edges.items() if pair <= seen)))
    return sorted(fans)


def _fans_of(res):
    members = [[] for _ in range(len(res["vertex"]))]
    for f, row in enumerate(res["fan_out"].tolist()):
        for j in row:
            if j >= 0:
                members[j].append(f)
    return [(int(v), int(l), tuple(sorted(m)), int(n)) for v, l, m, n in zip(res["vertex"], res["first_face"], members, res["n_links"])]


@pytest.mark.parametrize("case", range(100))
def test_checker_against_the_brute_force_on_tiny_soups(case):
    rng = np.random.default_rng(4000 + case)
    vtx, faces = tc.random_soup(rng, int(rng.integers(1, 25)), int(rng.integers(4, 9)))
    res = mc.manifold(vtx, faces)
    assert _fans_of(res) == _brute(faces, len(vtx))
    assert res["n_corners"].tolist() == [len(m) for _, _, m, _ in _fans_of(res)]
    # the output index: the first fan of a vertex keeps it, the others are numbered behind the vertices in fan order
    seen, new = set(), 0
    for j, v in enumerate(res["vertex"].tolist()):
        if v in seen:
            assert res["index_out"][j] == len(vtx) + new and res["vsrc"][new] == v
            new += 1
        else:
            assert res["index_out"][j] == v
        seen.add(v)
    assert new == len(res["vsrc"]) and np.array_equal(res["faces_out"][res["fan_out"] >= 0], res["index_out"][res["fan_out"][res["fan_out"] >= 0]])
    assert np.array_equal(res["faces_out"][res["fan_out"] < 0], np.asarray(faces)[res["fan_out"] < 0])


# ---- closed forms ----------------------------------------------------------------------------------------------------------------------------------
def _stats(**kw):
    st = dict.fromkeys(mc.STAT_NAMES, 0)
    st.update(kw)
    return st


def test_one_face_two_faces_on_a_vertex_and_nothing():
    res = mc.manifold(*mc.faces_on_a_vertex(1))
    assert res["stats"] == _stats(n_corners=3, n_fans=3, n_vertices_used=3, most_fans_at_vertex=1, n_open_fans=3, largest_fan_corners=1)
    assert res["faces_out"].tolist() == [[0, 1, 2]] and res["fan_out"].tolist() == [[0, 1, 2]] and res["n_links"].tolist() == [0, 0, 0]
    vtx, faces = mc.faces_on_a_vertex(2)
    res = mc.manifold(vtx, faces)
    assert res["stats"] == _stats(n_corners=6, n_fans=6, n_vertices_used=5, n_singular_vertices=1, most_fans_at_vertex=2, n_new_vertices=1, n_corners_moved=1,
                                  n_faces_changed=1, n_open_fans=6, largest_fan_corners=1)
    assert res["faces_out"].tolist() == [[0, 1, 2], [5, 3, 4]] and res["vsrc"].tolist() == [0] and res["n_fans_out"].tolist() == [2, 1, 1, 1, 1]
    assert res["vertex"].tolist() == [0, 0, 1, 2, 3, 4] and res["first_face"].tolist() == [0, 1, 0, 0, 1, 1] and res["index_out"].tolist() == [0, 5, 1, 2, 3, 4]
    mc.check_invariant(vtx, faces, res)
    empty = mc.manifold(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    assert empty["stats"] == _stats() and empty["faces_out"].shape == (0, 3) and empty["vtx_out"].shape == (0, 3)


def test_two_tetrahedra_on_a_vertex_and_on_an_edge():
    vtx, faces = mc.two_tetrahedra(1)
    res = mc.manifold(vtx, faces)
    assert res["stats"] == _stats(n_corners=24, n_fans=8, n_vertices_used=7, n_singular_vertices=1, most_fans_at_vertex=2, n_new_vertices=1, n_corners_moved=3,
                                  n_faces_changed=3, n_closed_fans=8, largest_fan_corners=3)
    after = tc.analyse(res["vtx_out"], res["faces_out"])["stats"]
    assert after["n_components"] == 2 and after["euler"] == 4 and after["n_boundary"] == 0
    mc.check_invariant(vtx, faces, res)
    vtx, faces = mc.two_tetrahedra(2)                                                   # the shared edge has four uses
    before = tc.analyse(vtx, faces)["stats"]
    assert before["n_nonmanifold"] == 1 and before["n_components"] == 1 and tc.analyse(vtx, faces)["edges"][tc.EDGE_NONMANIFOLD][1].tolist() == [4]
    res = mc.manifold(vtx, faces)
    # at either end of the edge the faces of one tetrahedron are a path of three whose two ends use the edge: a fan each, open
    assert res["stats"] == _stats(n_corners=24, n_fans=8, n_vertices_used=6, n_singular_vertices=2, most_fans_at_vertex=2, n_new_vertices=2, n_corners_moved=6,
                                  n_faces_changed=4, n_closed_fans=4, n_open_fans=4, largest_fan_corners=3, n_nonmanifold_before=1)
    out = tc.analyse(res["vtx_out"], res["faces_out"])
    assert out["stats"]["n_components"] == 2 and out["stats"]["n_boundary"] == 0 and out["stats"]["n_nonmanifold"] == 0 and out["stats"]["euler"] == 4
    for comp in range(2):                                                               # two closed surfaces, Euler 2 each
        assert tc.analyse(res["vtx_out"], res["faces_out"][out["comp"] == comp])["stats"]["euler"] == 2
    mc.check_invariant(vtx, faces, res)


def test_fin_book_and_touching_holes():
    vtx, faces = mc.fin_on_a_sheet()
    res = mc.manifold(vtx, faces)
    st = res["stats"]
    assert st["n_nonmanifold_before"] == 1 and st["n_new_vertices"] == 2 and st["n_singular_vertices"] == 2 and st["n_faces_changed"] == 1
    assert res["faces_out"][:-1].tolist() == faces[:-1].tolist() and res["faces_out"][-1].tolist() == [17, 18, 16] and res["vsrc"].tolist() == [5, 6]
    sheet, healed = tc.analyse(*tc.grid_sheet(3, 3))["stats"], tc.analyse(res["vtx_out"], res["faces_out"])["stats"]
    assert healed["n_interior"] == sheet["n_interior"] and healed["n_boundary"] == sheet["n_boundary"] + 3 and healed["n_components"] == 2
    mc.check_invariant(vtx, faces, res)
    vtx, faces = mc.faces_on_an_edge(3)                                                 # a book of three pages: three lone faces afterwards
    res = mc.manifold(vtx, faces)
    assert res["stats"] == _stats(n_corners=9, n_fans=9, n_vertices_used=5, n_singular_vertices=2, most_fans_at_vertex=3, n_new_vertices=4, n_corners_moved=4,
                                  n_faces_changed=2, n_open_fans=9, largest_fan_corners=1, n_nonmanifold_before=1)
    assert res["faces_out"].tolist() == [[0, 1, 2], [5, 7, 3], [6, 8, 4]] and res["vsrc"].tolist() == [0, 0, 1, 1]
    mc.check_invariant(vtx, faces, res)
    vtx, faces = hc.touching_holes()
    before = hc.holes(vtx, faces, 64)
    assert before["status"].tolist() == [hc.FILLED, hc.NONSIMPLE] and before["n_edges"].tolist() == [16, 8] and before["stats"]["n_filled"] == 1
    res = mc.manifold(vtx, faces)
    assert res["stats"]["n_new_vertices"] == 1 and res["stats"]["n_singular_vertices"] == 1 and res["vsrc"].tolist() == [12]
    after = hc.holes(res["vtx_out"], res["faces_out"], 64)                              # 1 filled loop of 2 becomes 2 filled loops of 2: one loop of 24
    assert after["stats"]["n_loops"] == 2 and after["stats"]["n_nonsimple"] == 0 and after["stats"]["n_filled"] == 2
    mc.check_invariant(vtx, faces, res)


def test_torus_moebius_and_pillow_move_nothing():
    vtx, faces = tc.torus(5, 4)
    res = mc.manifold(vtx, faces)
    assert res["stats"] == _stats(n_corners=120, n_fans=20, n_vertices_used=20, most_fans_at_vertex=1, n_closed_fans=20, largest_fan_corners=6)
    assert np.array_equal(res["faces_out"], faces) and (res["n_links"] == 6).all() and (res["n_corners"] == 6).all()
    vtx, faces = tc.moebius(9)                                                          # every vertex lies on the one border: open fans, paths of
    res = mc.manifold(vtx, faces)                                                       # three faces but at the flipped join (0: four, 9: two)
    assert res["stats"] == _stats(n_corners=54, n_fans=18, n_vertices_used=18, most_fans_at_vertex=1, n_open_fans=18, largest_fan_corners=4)
    assert np.array_equal(res["faces_out"], faces) and res["n_corners"].tolist() == [4] + [3] * 8 + [2] + [3] * 8
    assert np.array_equal(res["n_links"], res["n_corners"] - 1)
    vtx, faces = mc.pillow()
    res = mc.manifold(vtx, faces)
    assert res["stats"] == _stats(n_corners=6, n_fans=3, n_vertices_used=3, most_fans_at_vertex=1, n_closed_fans=3, largest_fan_corners=2)
    assert res["n_links"].tolist() == [2, 2, 2] and res["n_corners"].tolist() == [2, 2, 2] and np.array_equal(res["faces_out"], faces)


def test_faces_that_do_not_count_unused_vertices_and_bit_copies():
    vtx, faces = mc.faces_on_a_vertex(3)
    vtx = np.concatenate([vtx, np.ones((2, 3), np.float32)])                            # two unused vertices behind
    faces = np.concatenate([[[0, 0, 1]], faces[:2], [[7, 2, 2]], faces[2:], [[0, 8, 0]]]).astype(np.int32)
    bits = vtx.view(np.uint32)
    bits[0] = [0x7FC12345, 0x80000000, 0xFFC00001]                                      # a NaN with a payload, -0, a negative NaN with another
    res = mc.manifold(vtx, faces)
    assert res["fan_out"][[0, 3, 5]].tolist() == [[-1] * 3] * 3 and res["faces_out"][[0, 3, 5]].tolist() == faces[[0, 3, 5]].tolist()
    assert res["n_fans_out"].tolist() == [3, 1, 1, 1, 1, 1, 1, 0, 0] and res["stats"]["n_new_vertices"] == 2 and res["stats"]["n_vertices_used"] == 7
    assert res["faces_out"][[1, 2, 4]].tolist() == [[0, 1, 2], [9, 3, 4], [10, 5, 6]] and res["first_face"][:3].tolist() == [1, 2, 4]
    assert res["vtx_out"].view(np.uint32)[9:].tolist() == [bits[0].tolist()] * 2 and np.array_equal(res["vtx_out"].view(np.uint32)[:9], bits)
    assert np.array_equal(res["xyz"].view(np.uint32), res["vtx_out"].view(np.uint32)[9:])
    mc.check_invariant(vtx, faces, res)
    degenerate = mc.manifold(vtx, np.array([[1, 1, 2], [3, 3, 3]], np.int32))
    assert degenerate["stats"] == _stats() and (degenerate["fan_out"] == -1).all() and degenerate["n_fans_out"].sum() == 0


# ---- the Invariant on random soups -----------------------------------------------------------------------------------------------------------------
def _soup(case):
    rng = np.random.default_rng(9000 + case)
    return tc.random_soup(rng, int(rng.integers(1, 201)), int(rng.integers(5, 31)))


@pytest.mark.parametrize("case", range(44))
def test_invariant_and_idempotence_on_random_soups(case):
    vtx, faces = _soup(case)
    res = mc.manifold(vtx, faces)
    again = mc.check_invariant(vtx, faces, res)
    assert again["stats"]["n_closed_fans"] + again["stats"]["n_open_fans"] == res["stats"]["n_fans"]
    assert np.array_equal(again["vtx_out"].view(np.uint32), res["vtx_out"].view(np.uint32))


def test_the_random_soups_have_non_manifold_edges_with_many_uses():
    most, with_nm = 0, 0
    for case in range(44):
        nm = tc.analyse(*_soup(case))["edges"][tc.EDGE_NONMANIFOLD][1]
        with_nm += len(nm) > 0
        most = max(most, int(nm.max()) if len(nm) else 0)
    assert with_nm >= 15 and most >= 8


@pytest.mark.parametrize("case", range(45))
def test_no_nonsimple_loop_after_split_orient_holes(case):
    vtx, faces = _soup(100 + case)
    res = mc.manifold(vtx, faces)
    oriented = oc.orient(res["vtx_out"], res["faces_out"], oc.ORIENT_FIRST)
    assert oriented["stats"]["n_nonorientable"] == 0                                    # the rule's premise: it holds on every one of these soups
    assert hc.holes(res["vtx_out"], oriented["faces"], 64)["stats"]["n_nonsimple"] == 0


def test_those_soups_had_nonsimple_loops_before_the_split():
    n = 0
    for case in range(45):
        vtx, faces = _soup(100 + case)
        n += hc.holes(vtx, oc.orient(vtx, faces, oc.ORIENT_FIRST)["faces"], 64)["stats"]["n_nonsimple"] > 0
    assert n >= 20, n


def test_pinched_sheet_both_holes_fill_after_the_split():
    vtx, faces = mc.pinched_sheet()
    before = hc.holes(vtx, faces, 8)["stats"]
    assert (before["n_loops"], before["n_nonsimple"], before["n_filled"]) == (3, 1, 0)    # the two holes are one loop of eight edges through vertex 5
    res = mc.manifold(vtx, faces)
    assert res["vsrc"].tolist() == [5] and res["stats"]["n_singular_vertices"] == 1 and res["stats"]["n_nonmanifold_before"] == 0
    after = hc.holes(res["vtx_out"], res["faces_out"], 8)["stats"]
    assert (after["n_loops"], after["n_nonsimple"], after["n_filled"], after["n_too_long"]) == (4, 0, 2, 2)
    mc.check_invariant(vtx, faces, res)
