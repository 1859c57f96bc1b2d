"""CPU tier of the holes (include/immesh_topology.h, the Holes rule): the header as plain C99 with the new declarations, the library's new symbols,
immesh_holes_stats' layout, and the checker (tests/holes_checker.py) against closed forms, at each limit, and against the invariant that makes the
contract checkable: an analysis of faces ++ new_faces has the boundary edges, loops, edges, faces and Euler characteristic the filled loops predict,
and a second pass fills nothing that the first one filled."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import holes_checker as hc
import orient_checker as oc
import topology_checker as tc
from immesh_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "immesh_topology.h")
NEW_SYMBOLS = ("immesh_topology_holes", "immesh_topology_holes_loops", "immesh_topology_holes_cycles", "immesh_topology_holes_faces",
               "immesh_topology_holes_apply", "immesh_topology_holes_last_timing")
STATUS = (("IMMESH_HOLE_FILLED", hc.FILLED), ("IMMESH_HOLE_NONSIMPLE", hc.NONSIMPLE), ("IMMESH_HOLE_OUTLINE", hc.OUTLINE), ("IMMESH_HOLE_TOO_LONG", hc.TOO_LONG),
          ("IMMESH_HOLE_TOO_WIDE", hc.TOO_WIDE), ("IMMESH_HOLE_BLOCKED", hc.BLOCKED))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(capi.hip_library_path()):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "immesh_amd", "csrc"), "-j8"])
    return capi.load_hip_library()


# ---- the boundary ----------------------------------------------------------------------------------------------------------------------------
def test_header_is_plain_c99_with_the_holes(tmp_path):
    src = tmp_path / "alone.c"
    src.write_text('#include "immesh_topology.h"\nint main(void) { immesh_holes_stats s; float ms[2]; int rc;\n'
                   '  s.n_loops = IMMESH_HOLE_FILLED + IMMESH_HOLE_NONSIMPLE + IMMESH_HOLE_OUTLINE + IMMESH_HOLE_TOO_LONG + IMMESH_HOLE_TOO_WIDE + IMMESH_HOLE_BLOCKED;\n'
                   '  rc = immesh_topology_holes(0, 16, 0.0, &s) + immesh_topology_holes_loops(0, 0, 0, 0, 0, 0, 0, 0) + immesh_topology_holes_cycles(0, 0, 0, 0)\n'
                   '     + immesh_topology_holes_faces(0, 0, 0, 0, 0) + immesh_topology_holes_apply(0) + immesh_topology_holes_last_timing(0, ms);\n'
                   '  return rc + (int)s.n_loops; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "alone.o")])


def test_library_exports_the_holes(lib):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    fns = sorted(set(re.findall(r"\b(immesh_[a-z_0-9]+)\s*\(", src)))
    for must in NEW_SYMBOLS:
        assert must in fns
    missing = [f for f in fns if not hasattr(lib, f)]
    assert not missing, missing


def test_holes_stats_layout(tmp_path):
    names = [n for n, _ in capi.HolesStats._fields_]
    assert tuple(names) == hc.STAT_NAMES
    prog = tmp_path / "layout.c"
    prog.write_text('#include "immesh_topology.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void) {\n  printf("%zu", sizeof(immesh_holes_stats));\n'
                    + "".join('  printf(" %%zu", offsetof(immesh_holes_stats, %s));\n' % n for n in names) + "  return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(prog), "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe]).split()]
    assert got == [C.sizeof(capi.HolesStats)] + [getattr(capi.HolesStats, n).offset for n in names]
    assert got == [96] + [8 * i for i in range(12)]
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.findall(r"int64_t (\w+);", re.search(r"typedef struct immesh_holes_stats \{(.*?)\}", text, re.S).group(1)) == names
    assert (capi.HOLE_FILLED, capi.HOLE_NONSIMPLE, capi.HOLE_OUTLINE, capi.HOLE_TOO_LONG, capi.HOLE_TOO_WIDE, capi.HOLE_BLOCKED) == tuple(v for _, v in STATUS)
    for name, val in STATUS:
        assert re.search(r"#define %s %d\b" % (name, val), text)


# ---- closed forms ----------------------------------------------------------------------------------------------------------------------------------
def _euler(vtx, faces):
    return tc.analyse(vtx, faces)["stats"]["euler"]


def test_open_pyramid_lone_face_and_one_cell_hole():
    vtx, faces = hc.open_pyramid()
    res = hc.holes(vtx, faces, 3)
    assert res["status"].tolist() == [hc.FILLED] and res["cycle"].tolist() == [0, 1, 2] and res["new_faces"].tolist() == [[0, 2, 1]]
    assert _euler(vtx, faces) == 1 and _euler(vtx, hc.closed(faces, res)) == 2
    assert sorted(map(tuple, hc.closed(faces, res).tolist())) == sorted(map(tuple, tc.TETRA.tolist()))      # the face taken away, as it was wound
    hc.check_invariant(vtx, faces, res, 3)
    lone = hc.holes(vtx, faces[:1], 16)                                                 # a lone face: its own outline
    assert lone["status"].tolist() == [hc.OUTLINE] and lone["stats"]["n_outline"] == 1 and lone["stats"]["n_simple"] == 1 and len(lone["new_faces"]) == 0
    assert lone["cycle"].tolist() == faces[0].tolist() and lone["cycle_start"].tolist() == [0]
    vtx, faces = tc.grid_sheet(3, 3, holes=[(1, 1)])
    res = hc.holes(vtx, faces, 4)
    assert res["first_vertex"].tolist() == [0, 5] and res["n_edges"].tolist() == [12, 4] and res["status"].tolist() == [hc.TOO_LONG, hc.FILLED]
    assert res["cycle_start"].tolist() == [0, 12] and res["cycle"][12:].tolist() == [5, 6, 10, 9]
    assert res["new_faces"].tolist() == [[5, 10, 6], [5, 9, 10]] and res["new_loop"].tolist() == [1, 1]
    assert res["box"][1].tolist() == [1, 1, 0, 2, 2, 0]
    hc.check_invariant(vtx, faces, res, 4)
    full = tc.analyse(*tc.grid_sheet(3, 3))["stats"]
    assert {k: v for k, v in tc.analyse(vtx, hc.closed(faces, res))["stats"].items()} == full      # the sheet as if no cell had been left out
    assert hc.holes(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), 8)["stats"] == dict.fromkeys(hc.STAT_NAMES, 0)
    assert hc.holes(*tc.torus(5, 4), 8)["stats"] == dict.fromkeys(hc.STAT_NAMES, 0)


@pytest.mark.parametrize("n", [3, 8])
def test_cylinder_fills_both_ends_and_reverses_with_its_winding(n):
    vtx, faces = hc.cylinder(n)
    res = hc.holes(vtx, faces, n)
    assert res["first_vertex"].tolist() == [0, n] and res["status"].tolist() == [0, 0] and res["n_edges"].tolist() == [n, n]
    assert res["cycle"].tolist() == list(range(n)) + [n] + list(range(2 * n - 1, n, -1))
    assert res["stats"] == dict(n_loops=2, n_simple=2, n_nonsimple=0, n_outline=0, n_too_long=0, n_too_wide=0, n_blocked=0, n_filled=2,
                                n_new_faces=2 * (n - 2), n_edges_closed=2 * n, largest_simple_loop_edges=n, n_cycle_vertices=2 * n)
    assert _euler(vtx, faces) == 0 and _euler(vtx, hc.closed(faces, res)) == 2
    hc.check_invariant(vtx, faces, res, n)
    rev = hc.holes(*hc.cylinder(n, reverse=True), n)                                    # v_0 stays, the rest runs the other way
    for l in range(2):
        a, b = res["cycle"][l * n:(l + 1) * n], rev["cycle"][l * n:(l + 1) * n]
        assert a[0] == b[0] and a[1:].tolist() == b[1:][::-1].tolist()
    assert hc.holes(vtx, faces, n - 1 if n > 3 else 3, 0.0)["stats"]["n_filled"] == (0 if n > 3 else 2)


def test_nonsimple_blocked_and_moebius():
    vtx, faces = hc.touching_holes()
    res = hc.holes(vtx, faces, 64)
    assert res["n_edges"].tolist() == [16, 8] and res["status"].tolist() == [hc.FILLED, hc.NONSIMPLE] and res["cycle_start"].tolist() == [0, -1]
    assert res["stats"]["n_nonsimple"] == 1 and res["stats"]["n_cycle_vertices"] == 16 and (res["new_loop"] == 0).all()
    hc.check_invariant(vtx, faces, res, 64)
    vtx, faces = hc.blocked_sheet()
    res = hc.holes(vtx, faces, 4)
    assert res["status"].tolist() == [hc.TOO_LONG, hc.BLOCKED] and res["stats"]["n_blocked"] == 1 and len(res["new_faces"]) == 0
    assert tc.analyse(vtx, faces)["stats"]["n_nonmanifold"] == 0
    hc.check_invariant(vtx, faces, res, 4)
    vtx, faces = tc.moebius(9)                                                          # one loop of 18 edges; the flip winds two neighbours against each other
    res = hc.holes(vtx, faces, 64)
    assert res["n_edges"].tolist() == [18] and res["status"].tolist() == [hc.NONSIMPLE] and len(res["cycle"]) == 0
    vtx, faces = tc.grid_sheet(3, 3, holes=[(1, 1)])                                    # neighbours wound against each other: face 0 lies on the border
    faces[0] = faces[0][[0, 2, 1]]
    assert hc.holes(vtx, faces, 64)["status"].tolist() == [hc.NONSIMPLE, hc.FILLED]


def test_each_limit_on_one_past_and_exactly_at_its_value():
    vtx, faces = tc.grid_sheet(4, 5, holes=[(1, 1), (1, 2)])                            # one hole of two cells: 6 edges, box 1 x 2
    for max_edges, want in ((5, hc.TOO_LONG), (6, hc.FILLED), (7, hc.FILLED)):
        res = hc.holes(vtx, faces, max_edges)
        assert res["n_edges"].tolist() == [18, 6] and res["status"][1] == want
        hc.check_invariant(vtx, faces, res, max_edges)
    for md, want in ((0.0, hc.FILLED), (3.0, hc.FILLED), (2.0, hc.TOO_WIDE)):           # the squares are compared: 5 against 0 (off), 9 and 4
        res = hc.holes(vtx, faces, 6, md)
        assert res["status"][1] == want, md
        hc.check_invariant(vtx, faces, res, 6, md)
    vtx, faces = tc.grid_sheet(5, 6, holes=[(i, j) for i in (1, 2, 3) for j in (1, 2, 3, 4)])   # a 3 x 4 box: its diagonal is exactly 5
    border = hc.holes(vtx, faces, 64, 5.0)
    assert border["n_edges"].tolist() == [22, 14] and border["status"].tolist() == [hc.TOO_WIDE, hc.FILLED]              # exactly equal passes
    assert hc.holes(vtx, faces, 64, float(np.nextafter(5.0, 0.0)))["status"].tolist() == [hc.TOO_WIDE, hc.TOO_WIDE]
    assert hc.holes(vtx, faces, 13, 5.0)["status"].tolist() == [hc.TOO_LONG, hc.TOO_LONG]                               # TOO_LONG comes first


def test_box_with_a_nan_vertex():
    vtx, faces = tc.grid_sheet(3, 3, holes=[(1, 1)])
    vtx[5, 0] = np.nan
    vtx[6, 0] = np.nan
    vtx[9, 0] = np.inf
    vtx[10, 0] = -np.inf                                                                # no finite x on the hole's loop
    any_size = hc.holes(vtx, faces, 4, 0.0)
    assert any_size["status"].tolist() == [hc.TOO_LONG, hc.FILLED] and any_size["box"][1].tolist() == [np.inf, 1, 0, -np.inf, 2, 0]
    assert hc.holes(vtx, faces, 4, 1e30)["status"].tolist() == [hc.TOO_LONG, hc.TOO_WIDE]
    vtx[10, 0] = 2.0                                                                    # one finite x: a box of no width
    res = hc.holes(vtx, faces, 4, 1.5)
    assert res["status"].tolist() == [hc.TOO_LONG, hc.FILLED] and res["box"][1].tolist() == [2, 1, 0, 2, 2, 0]


# ---- the invariant on random soups ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(11))
def test_invariant_and_idempotence_on_sheets_with_fragments(case):
    rng = np.random.default_rng(700 + case)
    vtx, faces = tc.sheet_with_fragments(rng, 30, 30, 80, 20)
    res = hc.holes(vtx, faces, 12)
    again = hc.check_invariant(vtx, faces, res, 12)
    st = res["stats"]
    assert st["n_filled"] >= 30 and st["n_nonsimple"] >= 5 and st["n_outline"] == 5 and st["n_too_long"] == 1 and st["n_blocked"] == 0
    assert again["stats"]["n_filled"] == 0 and again["stats"]["n_loops"] == st["n_loops"] - st["n_filled"]
    assert tc.analyse(vtx, hc.closed(faces, res))["stats"]["n_components"] == tc.analyse(vtx, faces)["stats"]["n_components"]
    # the fan is wound like its neighbours, and the cycles are cycles of boundary half-edges
    half = {(int(f[k]), int(f[(k + 1) % 3])) for f in faces for k in range(3)}
    for l in np.nonzero(res["cycle_start"] >= 0)[0]:
        cyc = res["cycle"][res["cycle_start"][l]:res["cycle_start"][l] + res["n_edges"][l]].tolist()
        assert cyc[0] == res["first_vertex"][l] == min(cyc) and all((a, b) in half and (b, a) not in half for a, b in zip(cyc, cyc[1:] + cyc[:1]))


def test_flipped_sheet_before_and_after_the_orientation():
    rng = np.random.default_rng(12)
    vtx, faces = tc.sheet_with_fragments(rng, 20, 20, 30, 0)                           # the sheet alone: one patch
    ref = hc.holes(vtx, faces, 12)
    flipped = oc.flip_random(rng, faces)[0]
    before = hc.holes(vtx, flipped, 12)
    assert before["stats"]["n_loops"] == ref["stats"]["n_loops"] and before["stats"]["n_nonsimple"] > ref["stats"]["n_nonsimple"]
    assert before["stats"]["n_filled"] < ref["stats"]["n_filled"]
    hc.check_invariant(vtx, flipped, before, 12)
    oriented = oc.orient(vtx, flipped, oc.ORIENT_FIRST)
    after = hc.holes(vtx, oriented["faces"], 12)
    # every patch as the sheet's generator wound it, or its mirror image: the loops and their statuses are those of the unflipped sheet, and a
    # cycle is the same one or, on a mirrored patch, runs the other way from the same label
    assert after["stats"] == ref["stats"] and all(np.array_equal(after[k], ref[k]) for k in ("first_vertex", "n_edges", "status", "box", "cycle_start"))
    for l in np.nonzero(ref["cycle_start"] >= 0)[0]:
        a = ref["cycle"][ref["cycle_start"][l]:ref["cycle_start"][l] + ref["n_edges"][l]]
        b = after["cycle"][ref["cycle_start"][l]:ref["cycle_start"][l] + ref["n_edges"][l]]
        assert a[0] == b[0] and (np.array_equal(a, b) or np.array_equal(a[1:], b[1:][::-1]))
    hc.check_invariant(vtx, oriented["faces"], after, 12)
