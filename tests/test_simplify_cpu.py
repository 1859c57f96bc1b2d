"""CPU tier of the weld and the vertex clustering (include/immesh_simplify.h): the header as plain C99 on its own, the library's new symbols,
immesh_simplify_stats' layout, and the checker (tests/simplify_checker.py) against its brute force, closed forms, every key case at its edge, the
duplicates in every rotation and winding, the facts the header states, and the one cluster whose mean depends on the order of the sum."""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import simplify_checker as sc
import topology_checker as tc
from immesh_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "immesh_simplify.h")
NEW_SYMBOLS = ("immesh_simplify", "immesh_simplify_vertices", "immesh_simplify_maps", "immesh_simplify_faces", "immesh_simplify_apply",
               "immesh_simplify_last_timing")
DEFINES = (("IMMESH_SIMPLIFY_FIRST", sc.FIRST), ("IMMESH_SIMPLIFY_MEAN", sc.MEAN), ("IMMESH_FACE_KEPT", sc.KEPT), ("IMMESH_FACE_NOT_COUNTING", sc.NOT_COUNTING),
           ("IMMESH_FACE_COLLAPSED", sc.COLLAPSED), ("IMMESH_FACE_DUPLICATE", sc.DUPLICATE))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(capi.hip_library_path()):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "immesh_amd", "csrc"), "-j8"])
    return capi.load_hip_library()


# ---- the boundary ----------------------------------------------------------------------------------------------------------------------------
def test_header_is_plain_c99_on_its_own(tmp_path):
    src = tmp_path / "alone.c"
    src.write_text('#include "immesh_simplify.h"\nint main(void) { immesh_simplify_stats s; float ms[2]; int rc;\n'
                   '  s.n_faces_out = IMMESH_SIMPLIFY_FIRST + IMMESH_SIMPLIFY_MEAN + IMMESH_FACE_KEPT + IMMESH_FACE_NOT_COUNTING + IMMESH_FACE_COLLAPSED + IMMESH_FACE_DUPLICATE;\n'
                   '  rc = immesh_simplify(0, 0.0, IMMESH_SIMPLIFY_FIRST, 1, &s) + immesh_simplify_vertices(0, 0, 0, 0, 0, 0) + immesh_simplify_maps(0, 0, 0, 0)\n'
                   '     + immesh_simplify_faces(0, 0, 0, 0) + immesh_simplify_apply(0) + immesh_simplify_last_timing(0, ms);\n'
                   '  return rc + (int)s.n_faces_out; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "alone.o")])


def test_library_exports_the_simplification(lib):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    fns = sorted(set(re.findall(r"\b(immesh_[a-z_0-9]+)\s*\(", src)))
    assert fns == sorted(NEW_SYMBOLS)
    missing = [f for f in fns if not hasattr(lib, f)]
    assert not missing, missing


def test_simplify_stats_layout(tmp_path):
    names = [n for n, _ in capi.SimplifyStats._fields_]
    assert tuple(names) == sc.STAT_NAMES
    prog = tmp_path / "layout.c"
    prog.write_text('#include "immesh_simplify.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void) {\n  printf("%zu", sizeof(immesh_simplify_stats));\n'
                    + "".join('  printf(" %%zu", offsetof(immesh_simplify_stats, %s));\n' % n for n in names) + "  return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(prog), "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe]).split()]
    assert got == [C.sizeof(capi.SimplifyStats)] + [getattr(capi.SimplifyStats, n).offset for n in names]
    assert got == [88] + [8 * i for i in range(11)]
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.findall(r"int64_t (\w+);", re.search(r"typedef struct immesh_simplify_stats \{(.*?)\}", text, re.S).group(1)) == names
    assert (capi.SIMPLIFY_FIRST, capi.SIMPLIFY_MEAN, capi.FACE_KEPT, capi.FACE_NOT_COUNTING, capi.FACE_COLLAPSED, capi.FACE_DUPLICATE) == tuple(v for _, v in DEFINES)
    for name, val in DEFINES:
        assert re.search(r"#define %s %d\b" % (name, val), text)


# ---- the checker against the brute force ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(12))
def test_checker_equals_brute_force_on_random_tiny_soups(case):
    rng = np.random.default_rng(900 + case)
    nv = int(rng.integers(4, 14))
    vtx = (rng.integers(-6, 7, (nv, 3)) * 0.25).astype(np.float32)                     # a coarse lattice: equal floats, shared cells, cell walls
    vtx[rng.random((nv, 3)) < 0.08] = -0.0
    if case % 3 == 1:
        vtx[rng.integers(nv), rng.integers(3)] = [np.nan, np.inf, -np.inf][case // 3 % 3]
        vtx[rng.integers(nv), 0] = np.float32(3e6)                                     # outside the grid of cell = 0.5
    faces = rng.integers(0, nv, (int(rng.integers(1, 24)), 3)).astype(np.int32)
    for cell, mode, merge in itertools.product((0.0, 0.5, 1.0, 3.0), (sc.FIRST, sc.MEAN), (True, False)):
        res = sc.simplify(vtx, faces, cell, mode, merge)
        sc.same_as_brute(res, sc.brute(vtx, faces, cell, mode, merge))
        sc.check_facts(vtx, faces, res, cell, mode, merge)


# ---- closed forms -------------------------------------------------------------------------------------------------------------------------------------
def test_unshared_cube_welds_to_eight_vertices_and_a_closed_surface():
    vtx, faces = sc.unshared(sc.CUBE_VTX, sc.CUBE_FACES)
    assert len(vtx) == 36 and tc.analyse(vtx, faces)["stats"]["n_components"] == 12 and tc.analyse(vtx, faces)["stats"]["n_boundary"] == 36
    res = sc.check_facts(vtx, faces, sc.simplify(vtx, faces), 0.0, sc.FIRST)
    assert res["stats"] == dict(n_vertices_in=36, n_vertices_used=36, n_alone_not_finite=0, n_alone_outside=0, n_vertices_out=8, largest_cluster=6,
                                n_faces_in=12, n_not_counting=0, n_collapsed=0, n_duplicate=0, n_faces_out=12)
    st = tc.analyse(res["vtx_out"], res["faces_out"])["stats"]
    assert st["euler"] == 2 and st["n_components"] == 1 and st["n_boundary"] == 0 and st["n_inconsistent"] == 0
    assert sorted(res["n_members"].tolist()) == [4] * 6 + [6] * 2 and res["first_vertex"].tolist() == sorted(res["first_vertex"].tolist())
    rng = np.random.default_rng(4)
    sv, sf = sc.unshared(sc.CUBE_VTX, sc.CUBE_FACES, rng)                              # labels and numbering under a shuffle of the vertex indices
    shuffled = sc.check_facts(sv, sf, sc.simplify(sv, sf), 0.0, sc.FIRST)
    sc.same_as_brute(shuffled, sc.brute(sv, sf))
    assert shuffled["stats"] == res["stats"] and tc.analyse(shuffled["vtx_out"], shuffled["faces_out"])["stats"] == st
    assert all(shuffled["first_vertex"][c] == np.nonzero(shuffled["vmap"] == c)[0].min() for c in range(8))


def test_grid_sheet_with_a_cell_of_two_grid_steps():
    vtx, faces = tc.grid_sheet(8, 6)                                                    # 9 x 7 vertices at integers: cells of 2 hold 2 x 2, the last row / column 1
    for mode in (sc.FIRST, sc.MEAN):
        res = sc.check_facts(vtx, faces, sc.simplify(vtx, faces, 2.0, mode), 2.0, mode)
        st = res["stats"]
        assert st["n_vertices_out"] == 5 * 4 and st["largest_cluster"] == 4 and st["n_faces_out"] == 2 * 4 * 3 and st["n_duplicate"] == 0
        assert st["n_collapsed"] == 96 - 24 and sorted(set(res["n_members"].tolist())) == [1, 2, 4]
        coarse = tc.analyse(res["vtx_out"], res["faces_out"])["stats"]
        assert coarse["n_components"] == 1 and coarse["euler"] == 1 and coarse["n_inconsistent"] == 0 and coarse["n_nonmanifold"] == 0
    assert res["vtx_out"][0].tolist() == [0.5, 0.5, 0.0]
    first = sc.simplify(vtx, faces, 2.0, sc.FIRST)
    assert first["vtx_out"][0].tolist() == [0.0, 0.0, 0.0] and first["first_vertex"][:4].tolist() == [0, 2, 4, 6]
    assert sc.simplify(vtx, faces, 0.0, sc.MEAN)["vtx_out"].tobytes() == vtx.tobytes()   # the weld ignores the mode


def test_every_face_status_and_the_six_rotations_and_windings():
    vtx, faces = sc.status_soup()
    res = sc.check_facts(vtx, faces, sc.simplify(vtx, faces), 0.0, sc.FIRST)
    assert res["fstatus"].tolist() == [0, 3, 3, 3, 3, 3, 3, 2, 1, 2] and res["faces_out"].tolist() == [[0, 1, 2]] and res["vmap"].tolist() == [0, 1, 2, 0, -1, 1]
    assert res["fmap"].tolist() == [0] + [-1] * 9 and res["stats"]["n_duplicate"] == 6 and res["stats"]["n_vertices_used"] == 5
    off = sc.check_facts(vtx, faces, sc.simplify(vtx, faces, merge_duplicates=False), 0.0, sc.FIRST, False)
    assert off["fstatus"].tolist() == [0] * 7 + [2, 1, 2] and off["stats"]["n_duplicate"] == 0
    assert off["faces_out"].tolist() == [[0, 1, 2], [1, 2, 0], [2, 0, 1], [0, 2, 1], [2, 1, 0], [1, 0, 2], [0, 1, 2]]   # rotation and winding kept
    for r in (res, off):
        sc.same_as_brute(r, sc.brute(vtx, faces, merge_duplicates=r is res))
    first = np.array([[3, 5, 2], [0, 1, 2]], np.int32)                                 # the smaller face index is the one kept, as it is wound
    assert sc.simplify(vtx, first)["faces_out"].tolist() == [[0, 1, 2]] and sc.simplify(vtx, first[:, [0, 2, 1]])["faces_out"].tolist() == [[0, 2, 1]]


# ---- keys -------------------------------------------------------------------------------------------------------------------------------------------------
def test_keys_zeros_nan_walls_range_edges_and_overflow():
    vtx, faces, c = sc.key_cases()
    for mode in (sc.FIRST, sc.MEAN):
        res = sc.check_facts(vtx, faces, sc.simplify(vtx, faces, c, mode), c, mode)
        sc.same_as_brute(res, sc.brute(vtx, faces, c, mode))
        m = res["vmap"]
        assert m[0] == m[1] and m[2] != m[3] and m[4] != m[5]
        assert m[6] == m[8] != m[7] and m[9] == m[11] != m[10]                          # a vertex on k cell belongs to cell k, for negative k too
        assert m[12] == m[13] and m[14] == m[15] and m[16] != m[17] and m[18] != m[19] and m[20] != m[21]
        assert res["stats"]["n_alone_not_finite"] == 4 and res["stats"]["n_alone_outside"] == 6
    assert res["vtx_out"][m[0]].view(np.uint32).tolist() == [0, 0, 0]                   # the mean of -0 and +0, summed from 0.0
    assert res["vtx_out"][m[2]].tobytes() == vtx[2].tobytes()
    weld = sc.check_facts(vtx, faces, sc.simplify(vtx, faces), 0.0, sc.FIRST)
    sc.same_as_brute(weld, sc.brute(vtx, faces))
    w = weld["vmap"]
    assert w[0] == w[1] and w[2] != w[3] and w[4] != w[5] and w[16] == w[17] and w[18] == w[19] and w[20] == w[21] and w[6] != w[8]
    assert weld["vtx_out"][w[0]].view(np.uint32).tolist() == [0x80000000, 0, 0]         # FIRST: the label's floats bit for bit, its -0 included
    assert weld["stats"]["n_alone_not_finite"] == 4 and weld["stats"]["n_alone_outside"] == 0
    tiny = sc.check_facts(vtx, faces, sc.simplify(vtx, faces, 5e-324, sc.MEAN), 5e-324, sc.MEAN)   # x / cell overflows to infinity: alone
    sc.same_as_brute(tiny, sc.brute(vtx, faces, 5e-324, sc.MEAN))
    t = tiny["vmap"]
    assert t[0] == t[1] and t[6] != t[8] and t[20] != t[21] and tiny["stats"]["largest_cluster"] == 2
    assert tiny["stats"]["n_alone_outside"] == int((np.isfinite(vtx).all(axis=1) & (vtx != 0).any(axis=1)).sum()) == len(vtx) - 6   # all but zeros, NaN, inf


# ---- the facts on larger soups ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(6))
def test_first_is_idempotent_and_mean_stays_within_the_cell(case):
    rng = np.random.default_rng(40 + case)
    vtx, faces = tc.sheet_with_fragments(rng, 24, 20, 30, 12)
    vtx = vtx + rng.normal(scale=0.004, size=vtx.shape).astype(np.float32)
    faces = np.concatenate([faces, faces[rng.integers(0, len(faces), 40)][:, [1, 2, 0]], faces[rng.integers(0, len(faces), 40)][:, [0, 2, 1]]])
    for cell in (0.0, 0.1, 0.23):
        for mode in (sc.FIRST, sc.MEAN):
            res = sc.check_facts(vtx, faces, sc.simplify(vtx, faces, cell, mode), cell, mode)
            assert res["stats"]["n_duplicate"] >= 40 and (cell == 0.0 or res["stats"]["n_collapsed"] > 100)
    uv, uf = sc.unshared(vtx, faces[:-80], rng)
    welded = sc.check_facts(uv, uf, sc.simplify(uv, uf), 0.0, sc.FIRST)
    assert tc.analyse(welded["vtx_out"], welded["faces_out"])["stats"] == tc.analyse(vtx, faces[:-80])["stats"]


def test_a_cluster_spanning_workgroups_beside_many_small_ones():
    rng = np.random.default_rng(77)
    vtx, faces = sc.cluster_beside_many(rng)
    for mode in (sc.FIRST, sc.MEAN):
        res = sc.check_facts(vtx, faces, sc.simplify(vtx, faces, 1.0, mode), 1.0, mode)
        assert res["stats"]["largest_cluster"] == 300 and res["stats"]["n_vertices_out"] == 501 and sorted(set(res["n_members"].tolist())) == [1, 2, 3, 300]


def test_the_mean_of_one_cluster_depends_on_the_order_of_its_members():
    cell = 2.0 ** 62
    got = {}
    for order in itertools.permutations(range(3)):
        vtx, faces = sc.order_triple(order)
        res = sc.check_facts(vtx, faces, sc.simplify(vtx, faces, cell, sc.MEAN), cell, sc.MEAN)
        sc.same_as_brute(res, sc.brute(vtx, faces, cell, sc.MEAN))
        assert res["stats"]["n_vertices_out"] == 4 and res["n_members"].tolist() == [3, 1, 1, 1] and res["vmap"][:3].tolist() == [0, 0, 0]
        s = 0.0
        for i in order:
            s = s + sc.ORDER_TRIPLE[i]
        assert res["vtx_out"][0, 0] == np.float32(s / 3.0)
        got[order] = int(res["vtx_out"][0, 0].view(np.uint32))
        first = sc.simplify(vtx, faces, cell, sc.FIRST)
        assert first["vtx_out"][0, 0] == np.float32(sc.ORDER_TRIPLE[order[0]])
    assert len(set(got.values())) == 2, got                                             # the sequential sum rounds to two different floats
