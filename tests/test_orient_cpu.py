"""CPU tier of the orientation (include/immesh_topology.h, the Orientation rule): the header as plain C99 with the new declarations, the library's
new symbols, immesh_orient_stats' layout, and the checker (tests/orient_checker.py) against closed forms, against the orientation double cover through
a plain union-find on random soups and flipped sheets, and against the invariant that makes the contract checkable: an analysis of faces_out counts
n_inconsistent_after inconsistent edges and is otherwise the analysis of the faces."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import orient_checker as oc
import topology_checker as tc
from immesh_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "immesh_topology.h")
NEW_SYMBOLS = ("immesh_topology_orient", "immesh_topology_orient_faces", "immesh_topology_orient_patches", "immesh_topology_orient_apply",
               "immesh_topology_orient_last_timing")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(capi.hip_library_path()):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "immesh_amd", "csrc"), "-j8"])
    return capi.load_hip_library()


# ---- the boundary ----------------------------------------------------------------------------------------------------------------------------
def test_header_is_plain_c99_with_the_orientation(tmp_path):
    src = tmp_path / "alone.c"
    src.write_text('#include "immesh_topology.h"\nint main(void) { immesh_orient_stats s; double o[3] = {0.0, 0.0, 0.0}; float ms[2]; int rc;\n'
                   '  s.n_patches = IMMESH_ORIENT_FIRST + IMMESH_ORIENT_FEWEST + IMMESH_ORIENT_VIEWPOINT;\n'
                   '  rc = immesh_topology_orient(0, IMMESH_ORIENT_VIEWPOINT, o, &s) + immesh_topology_orient_faces(0, 0, 0, 0)\n'
                   '     + immesh_topology_orient_patches(0, 0, 0, 0, 0, 0, 0, 0) + immesh_topology_orient_apply(0) + immesh_topology_orient_last_timing(0, ms);\n'
                   '  return rc + (int)s.n_patches; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "alone.o")])


def test_library_exports_the_orientation(lib):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    fns = sorted(set(re.findall(r"\b(immesh_[a-z_0-9]+)\s*\(", src)))
    for must in NEW_SYMBOLS:
        assert must in fns
    missing = [f for f in fns if not hasattr(lib, f)]
    assert not missing, missing


def test_orient_stats_layout(tmp_path):
    names = [n for n, _ in capi.OrientStats._fields_]
    assert tuple(names) == oc.STAT_NAMES
    prog = tmp_path / "layout.c"
    prog.write_text('#include "immesh_topology.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void) {\n  printf("%zu", sizeof(immesh_orient_stats));\n'
                    + "".join('  printf(" %%zu", offsetof(immesh_orient_stats, %s));\n' % n for n in names) + "  return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(prog), "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe]).split()]
    assert got == [C.sizeof(capi.OrientStats)] + [getattr(capi.OrientStats, n).offset for n in names]
    assert got == [72] + [8 * i for i in range(9)]
    declared = re.findall(r"int64_t (\w+);", re.search(r"typedef struct immesh_orient_stats \{(.*?)\}", re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S), re.S).group(1))
    assert declared == names
    assert (capi.ORIENT_FIRST, capi.ORIENT_FEWEST, capi.ORIENT_VIEWPOINT) == (oc.ORIENT_FIRST, oc.ORIENT_FEWEST, oc.ORIENT_VIEWPOINT)
    for name, val in (("IMMESH_ORIENT_FIRST", 0), ("IMMESH_ORIENT_FEWEST", 1), ("IMMESH_ORIENT_VIEWPOINT", 2)):
        assert re.search(r"#define %s %d\b" % (name, val), open(HEADER).read())


# ---- closed forms ----------------------------------------------------------------------------------------------------------------------------------
def _two_tetrahedra_on_an_edge():
    v0, f0 = tc.tetrahedron()
    v1, f1 = tc.tetrahedron((3.0, 0.0, 0.0))
    remap = np.array([0, 1, 6, 7])
    return np.concatenate([v0, v1]), np.concatenate([f0, remap[f1].astype(np.int32)])


def check_invariant(vtx, faces, res):
    """an analysis of faces_out: n_inconsistent_after inconsistent edges, everything else as the analysis of the faces"""
    before, after = tc.analyse(vtx, faces), tc.analyse(vtx, res["faces"])
    assert after["stats"]["n_inconsistent"] == res["stats"]["n_inconsistent_after"] and before["stats"]["n_inconsistent"] == res["stats"]["n_inconsistent_before"]
    assert {k: v for k, v in after["stats"].items() if k != "n_inconsistent"} == {k: v for k, v in before["stats"].items() if k != "n_inconsistent"}
    for k in ("comp", "first_face", "n_faces", "n_boundary", "box"):
        assert np.array_equal(after[k], before[k]), k
    for kind in (tc.EDGE_BOUNDARY, tc.EDGE_NONMANIFOLD):
        assert all(np.array_equal(x, y) for x, y in zip(after["edges"][kind], before["edges"][kind]))
    # and the tables add up
    st = res["stats"]
    assert st["n_patches"] == len(res["first_face"]) == st["n_orientable"] + st["n_nonorientable"] and res["n_faces"].sum() == before["stats"]["n_counting"]
    assert res["n_inconsistent"].sum() == st["n_inconsistent_before"] and res["n_flipped"].sum() == st["n_faces_flipped"] == int(res["flip"].sum())
    assert (st["n_inconsistent_after"] == 0) == (st["n_nonorientable"] == 0)
    assert np.array_equal(np.sort(res["faces"], axis=1), np.sort(np.asarray(faces, np.int32).reshape(-1, 3), axis=1))


@pytest.mark.parametrize("mode", oc.MODES)
def test_checker_closed_forms(mode):
    o = (0.3, 0.2, 7.0)
    vtx, faces = tc.strip(33)                                                         # every neighbour pair of a strip is wound alike
    res = oc.orient(vtx, faces, oc.ORIENT_FIRST)
    assert res["base"].tolist() == [f & 1 for f in range(33)] and res["flip"].tolist() == [f & 1 for f in range(33)]
    assert res["stats"] == dict(n_patches=1, n_orientable=1, n_nonorientable=0, largest_patch_faces=33, n_faces_flipped=16, n_faces_nonorientable=0,
                                n_patches_inverted=0, n_inconsistent_before=32, n_inconsistent_after=0)
    check_invariant(vtx, faces, res)
    assert oc.orient(vtx, faces, oc.ORIENT_FEWEST)["flip"].tolist() == res["flip"].tolist()          # 16 of 33: the fewest already
    vtx, faces = tc.strip(34)
    assert oc.orient(vtx, faces, oc.ORIENT_FEWEST)["stats"]["n_patches_inverted"] == 0              # 17 of 34: a tie keeps FIRST
    vtx, faces = tc.torus(16, 16)
    res = oc.orient(vtx, faces, mode, o)
    if mode != oc.ORIENT_VIEWPOINT:
        assert not res["flip"].any() and res["stats"]["n_inconsistent_before"] == 0 and res["stats"]["n_patches"] == 1
    assert res["flip"].min() == res["flip"].max()                                     # all or nothing
    check_invariant(vtx, faces, res)
    for vtx, faces in (tc.moebius(9), oc.klein(16, 16), oc.klein(3, 3)):
        res = oc.orient(vtx, faces, mode, o)
        assert res["stats"]["n_patches"] == 1 and res["stats"]["n_nonorientable"] == 1 and res["orientable"].tolist() == [0] and not res["flip"].any()
        assert res["stats"]["n_inconsistent_after"] == res["stats"]["n_inconsistent_before"] >= 1 and res["stats"]["n_faces_nonorientable"] == len(faces)
        assert np.array_equal(res["faces"], faces)
        check_invariant(vtx, faces, res)
    st = tc.analyse(*oc.klein(16, 16))["stats"]
    assert st["n_boundary"] == 0 and st["n_nonmanifold"] == 0 and st["euler"] == 0 and st["n_components"] == 1 and st["n_counting"] == 512
    vtx, faces = np.eye(3, dtype=np.float32), np.array([[0, 1, 2], [0, 1, 2]], np.int32)   # two copies of one face: wound alike on three shared edges
    res = oc.orient(vtx, faces, oc.ORIENT_FIRST)
    assert res["flip"].tolist() == [0, 1] and res["faces"].tolist() == [[0, 1, 2], [0, 2, 1]] and res["n_inconsistent"].tolist() == [3]
    check_invariant(vtx, faces, res)
    vtx, faces = _two_tetrahedra_on_an_edge()
    res = oc.orient(vtx, faces, mode, o)
    assert tc.analyse(vtx, faces)["stats"]["n_components"] == 1 and res["stats"]["n_patches"] == 2   # a fan joins components, not patches
    assert res["patch"].tolist() == [0] * 4 + [1] * 4 and res["first_face"].tolist() == [0, 4]
    check_invariant(vtx, faces, res)


def test_checker_modes_and_votes():
    vtx, faces = tc.grid_sheet(4, 3)
    faces[0] = faces[0][[0, 2, 1]]
    first, fewest = oc.orient(vtx, faces, oc.ORIENT_FIRST), oc.orient(vtx, faces, oc.ORIENT_FEWEST)
    assert first["flip"].tolist() == [0] + [1] * 23 and first["stats"]["n_patches_inverted"] == 0
    assert fewest["flip"].tolist() == [1] + [0] * 23 and fewest["stats"]["n_patches_inverted"] == 1 and fewest["n_flipped"].tolist() == [1]
    # the sheet's faces (v00, v10, v11) show their front to +z
    assert oc.view_sign(*tc.grid_sheet(4, 3), (1.0, 1.0, 5.0)).tolist() == [1] * 24 and oc.view_sign(*tc.grid_sheet(4, 3), (1.0, 1.0, -5.0)).tolist() == [-1] * 24
    above, below = oc.orient(vtx, faces, oc.ORIENT_VIEWPOINT, (1, 1, 5)), oc.orient(vtx, faces, oc.ORIENT_VIEWPOINT, (1, 1, -5))
    assert above["flip"].tolist() == [1] + [0] * 23 and below["flip"].tolist() == [0] + [1] * 23
    assert oc.view_sign(vtx, above["faces"], (1, 1, 5)).tolist() == [1] * 24
    in_plane = oc.orient(vtx, faces, oc.ORIENT_VIEWPOINT, (9, 9, 0))                  # s = 0 everywhere: a tie keeps FIRST
    assert oc.view_sign(vtx, faces, (9, 9, 0)).tolist() == [0] * 24 and in_plane["flip"].tolist() == first["flip"].tolist()
    # the outward tetrahedron: from inside every face shows its back
    vtx, faces = tc.tetrahedron()
    assert oc.view_sign(vtx, faces, (0.2, 0.2, 0.2)).tolist() == [-1] * 4 and oc.orient(vtx, faces, oc.ORIENT_VIEWPOINT, (0.2, 0.2, 0.2))["flip"].tolist() == [1] * 4
    # vertices that are not finite and a face of zero area do not vote, and are flipped with their patch all the same
    vtx = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [np.nan, 2, 0], [2, np.inf, 0], [2, 0, 0]], np.float32)
    faces = np.array([[0, 2, 1], [0, 3, 2], [3, 4, 2], [1, 2, 5], [0, 1, 6]], np.int32)   # two real faces with their back to +z, NaN, inf, zero area
    assert oc.view_sign(vtx, faces, (0.5, 0.5, 3.0)).tolist() == [-1, -1, 0, 0, 0]
    res = oc.orient(vtx, faces, oc.ORIENT_VIEWPOINT, (0.5, 0.5, 3.0))
    assert res["stats"]["n_patches"] == 1 and res["stats"]["n_patches_inverted"] == 1 and res["flip"].tolist() == [1] * 5
    check_invariant(vtx, faces, res)


# ---- an independent method: the orientation double cover through a plain union-find -------------------------------------------------------------------
def _double_cover(faces):
    """-> label (-1), base, orientable per face"""
    f, g, d, counting = oc.pairs(faces)
    n = len(counting)
    cls = tc._classes(2 * n, [(2 * x, 2 * y + z) for x, y, z in zip(f, g, d)] + [(2 * x + 1, 2 * y + 1 - z) for x, y, z in zip(f, g, d)])
    r0, r1 = cls[0::2], cls[1::2]
    return np.where(counting, r0 >> 1, -1), np.where(counting & (r0 != r1), r0 & 1, 0), r0 != r1


def _soups():
    rng = np.random.default_rng(404)
    for k in range(6):
        yield tc.random_soup(rng, int(rng.integers(1, 160)), n_vtx=int(rng.integers(5, 60)))
    for k in range(3):
        vtx, faces = tc.sheet_with_fragments(rng, 12, 9, 5, 20)
        yield oc.with_moebius(vtx, oc.flip_random(rng, faces)[0], (5, 9))
    yield tc.torus(7, 5)[0], oc.flip_random(rng, tc.torus(7, 5)[1])[0]
    yield oc.klein(5, 4)[0], oc.flip_random(rng, oc.klein(5, 4)[1])[0]


@pytest.mark.parametrize("case", range(11))
def test_checker_against_the_double_cover(case):
    vtx, faces = list(_soups())[case]
    label, base, orientable = _double_cover(faces)
    for mode in oc.MODES:
        res = oc.orient(vtx, faces, mode, (0.5, -0.25, 30.0))
        assert res["first_face"].tolist() == sorted(set(label[label >= 0].tolist()))
        assert np.array_equal(res["patch"] >= 0, label >= 0) and np.array_equal(res["first_face"][res["patch"][label >= 0]], label[label >= 0])
        assert np.array_equal(res["orientable"][res["patch"][label >= 0]] != 0, orientable[label >= 0])
        assert np.array_equal(res["base"], base)
        if mode == oc.ORIENT_FIRST:
            assert np.array_equal(res["flip"], base)
        check_invariant(vtx, faces, res)
    if case >= 6:
        assert res["stats"]["n_inconsistent_before"] > 10
    if 6 <= case < 9:
        assert res["stats"]["n_nonorientable"] == 2 and res["stats"]["n_orientable"] > 10
