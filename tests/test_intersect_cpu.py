"""CPU tier of the self-intersection pass (include/immesh_intersect.h): the header as plain C99 on its own, the library's new symbols,
immesh_intersect_stats' layout, and the two checkers (tests/intersect_checker.py) against each other and against closed forms: height fields without
a pair, crossing and jittered sheets, every single-bit mask from a hand-made pair, rotations and swaps of two crossing faces."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import intersect_checker as ic
from immesh_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "immesh_intersect.h")
NEW_SYMBOLS = ("immesh_self_intersect", "immesh_self_intersect_pairs", "immesh_self_intersect_faces", "immesh_self_intersect_apply",
               "immesh_self_intersect_last_timing")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(capi.hip_library_path()):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "immesh_amd", "csrc"), "-j8"])
    return capi.load_hip_library()


# ---- the boundary ----------------------------------------------------------------------------------------------------------------------------
def test_header_is_plain_c99_on_its_own(tmp_path):
    src = tmp_path / "alone.c"
    src.write_text('#include "immesh_intersect.h"\nint main(void) { immesh_intersect_stats s; float ms[3]; int rc;\n'
                   '  s.n_share[3] = 0;\n'
                   '  rc = immesh_self_intersect(0, 1, &s) + immesh_self_intersect_pairs(0, 0, 0, 0, 0) + immesh_self_intersect_faces(0, 0, 0)\n'
                   '     + immesh_self_intersect_apply(0) + immesh_self_intersect_last_timing(0, ms);\n'
                   '  return rc + (int)s.n_share[3]; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "alone.o")])


def test_library_exports_the_intersection_pass(lib):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    fns = sorted(set(re.findall(r"\b(immesh_[a-z_0-9]+)\s*\(", src)))
    assert fns == sorted(NEW_SYMBOLS)
    missing = [f for f in fns if not hasattr(lib, f)]
    assert not missing, missing


def test_intersect_stats_layout(tmp_path):
    names = [n for n, _ in capi.IntersectStats._fields_]
    assert tuple(names) == ic.STAT_NAMES
    prog = tmp_path / "layout.c"
    prog.write_text('#include "immesh_intersect.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void) {\n  printf("%zu", sizeof(immesh_intersect_stats));\n'
                    + "".join('  printf(" %%zu", offsetof(immesh_intersect_stats, %s));\n' % n for n in names) + "  return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(prog), "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe]).split()]
    assert got == [C.sizeof(capi.IntersectStats)] + [getattr(capi.IntersectStats, n).offset for n in names]
    assert got == [104, 0, 8, 16, 24, 32, 64, 72, 80, 88, 96]
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.findall(r"int64_t (\w+)(?:\[4\])?;", re.search(r"typedef struct immesh_intersect_stats \{(.*?)\}", text, re.S).group(1)) == names


# ---- the two checkers ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(6))
def test_the_two_checkers_agree_on_mid_size_soups(case):
    rng = np.random.default_rng(100 + case)
    soups = (ic.crossing_sheets(rng, 14, 11), ic.jittered_sheet(rng, 16, 15), ic.unshared(*ic.crossing_sheets(rng, 6, 5)),
             ic.join(ic.big_and_small(40, 30, rng), ic.jittered_sheet(rng, 9, 9)))
    for k, (vtx, faces) in enumerate(soups):
        if case % 2:
            faces = faces[rng.permutation(len(faces))]
        if case == 5:
            vtx = vtx.copy(); vtx[rng.integers(len(vtx)), rng.integers(3)] = [np.nan, np.inf][k % 2]   # faces that are not in the tree
            faces = faces.copy(); faces[rng.integers(len(faces)), 1] = faces[rng.integers(len(faces)), 0]   # (most likely) one that does not count
        res = ic.both(vtx, faces, (case, k))
        assert res["stats"]["n_pairs"] > 0 and res["stats"]["n_candidates"] > res["stats"]["n_pairs"]


@pytest.mark.parametrize("kind", ["flat", "noisy", "tilted"])
def test_height_fields_have_no_pair(kind):
    rng = np.random.default_rng(7)
    z = {"flat": None, "noisy": ic.noisy(rng, 0.4), "tilted": lambda x, y: 0.75 * x - 0.3 * y + rng.normal(scale=0.2, size=x.shape)}[kind]
    vtx, faces = ic.sheet(8, 8, z)
    st = ic.both(vtx, faces, kind)["stats"]
    assert st["n_faces"] == 128 and st["n_pairs"] == 0 and st["n_faces_hit"] == 0 and st["n_candidates"] > 600 and st["n_share"][3] == 0
    assert st["n_share"][2] == 176 and st["n_share"][1] == 469                        # the sheet's edge and corner neighbours


def test_crossing_sheets_and_the_jittered_sheet():
    rng = np.random.default_rng(1)
    res = ic.both(*ic.crossing_sheets(rng, 4, 8))                                       # 128 faces: two sheets of 64
    st = res["stats"]
    assert 20 <= st["n_pairs"] <= 60 and st["n_pairs_share1"] == 0 and (res["pairs"][:, 0] < 64).all() and (res["pairs"][:, 1] >= 64).all()
    assert all(bin(int(m)).count("1") >= 2 for m in res["mask"])                       # a crossing in general position has two ends
    res = ic.both(*ic.jittered_sheet(rng, 8, 8))
    st = res["stats"]
    assert st["n_pairs"] > 5 and st["n_pairs_share1"] > 0 and st["n_pairs_share0"] > 0 and st["n_faces_hit"] > st["max_partners"] >= 1
    assert st["n_pairs"] == st["n_pairs_share0"] + st["n_pairs_share1"] and res["n_partners"].sum() == 2 * st["n_pairs"]
    assert len(res["kept"]) == 128 - st["n_faces_hit"] and (res["face_map"] >= 0).sum() == len(res["kept"])


def test_every_single_bit_mask_comes_from_a_pair_that_shares_a_vertex():
    """a crossing that starts in a shared vertex has one other end: the far edge of one face in the other face"""
    seen = set()
    for swap in (False, True):
        for ra in range(3):
            for rb in range(3):
                a, b = np.roll(ic.FAN_PIERCED[0], -ra), np.roll(ic.FAN_PIERCED[1], -rb)
                faces = np.stack([b, a] if swap else [a, b]).astype(np.int32)
                res = ic.both(ic.FAN_VTX, faces)
                want = ic.rotate_mask(2, ra, rb)
                want = ic.swap_mask(want) if swap else want
                assert res["mask"].tolist() == [want] and res["stats"]["n_share"] == [0, 1, 0, 0] and res["stats"]["n_pairs_share1"] == 1
                seen.add(want)
    assert seen == {1, 2, 4, 8, 16, 32}
    res = ic.both(ic.FAN_VTX, ic.FAN_NOT_PIERCED)
    assert res["stats"]["n_candidates"] == 1 and res["stats"]["n_pairs"] == 0


def test_rotating_a_face_rotates_its_bits_and_swapping_the_faces_swaps_the_halves():
    for faces, base in ((ic.CROSS_ONE_EACH, 0b001010), (ic.CROSS_TWO_OF_B, 0b101000)):
        seen = 0
        for swap in (False, True):
            for ra in range(3):
                for rb in range(3):
                    a, b = np.roll(faces[0], -ra), np.roll(faces[1], -rb)
                    res = ic.both(ic.CROSS_VTX, np.stack([b, a] if swap else [a, b]).astype(np.int32))
                    want = ic.rotate_mask(base, ra, rb)
                    want = ic.swap_mask(want) if swap else want
                    assert res["mask"].tolist() == [want] and res["pairs"].tolist() == [[0, 1]] and res["n_partners"].tolist() == [1, 1]
                    seen |= want
        assert seen == 63


def test_closed_ends_boxes_and_what_the_rule_does_not_detect():
    tri = np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0]], np.float32)
    # an endpoint in the other face: the edges that end there count with s == 0 and s == 1
    touch = np.concatenate([tri, np.array([[1, 1, 0], [1, 2, 3], [2, 1, 3]], np.float32)])
    res = ic.both(touch, [[0, 1, 2], [3, 4, 5]])
    assert res["mask"].tolist() == [0b101000]
    # boxes that miss by one float ulp: not a candidate, whatever the arithmetic would say
    up = np.nextafter(np.float32(4), np.float32(5))
    apart = np.concatenate([tri, np.array([[up, 0, -1], [up, 1, 1], [5, 0, 0]], np.float32)])
    assert ic.both(apart, [[0, 1, 2], [3, 4, 5]])["stats"]["n_candidates"] == 0
    # coplanar overlap: a candidate, every nd is exactly 0
    flat = np.concatenate([tri, tri + np.array([1, 1, 0], np.float32)])
    st = ic.both(flat, [[0, 1, 2], [3, 4, 5]])["stats"]
    assert st["n_candidates"] == 1 and st["n_share"][0] == 1 and st["n_pairs"] == 0
    # an edge neighbour folded flat onto its neighbour, and a duplicate
    fold = np.array([[0, 0, 0], [4, 0, 0], [1, 3, 0], [2, 2, 0]], np.float32)
    st = ic.both(fold, [[0, 1, 2], [1, 0, 3], [0, 1, 2]])["stats"]
    assert st["n_share"] == [0, 0, 2, 1] and st["n_pairs"] == 0
    # neighbours of an unwelded soup touch and count; welded, they do not
    vtx, faces = ic.sheet(3, 2, lambda x, y: 0.25 * x * y)
    assert ic.both(vtx, faces)["stats"]["n_pairs"] == 0
    loose = ic.both(*ic.unshared(vtx, faces))["stats"]
    assert loose["n_pairs"] > 0 and loose["n_share"][1:] == [0, 0, 0] and loose["n_faces_hit"] == len(faces)


def test_the_soups_with_counted_candidates_and_hits():
    for n_hit, n_near in ((255, 0), (256, 0), (257, 0), (100, 155), (100, 156), (100, 157), (300, 0)):
        st = ic.both(*ic.big_and_small(n_hit, n_near))["stats"]
        assert (st["n_candidates"], st["n_pairs"], st["max_partners"], st["n_faces_hit"]) == (n_hit + n_near, n_hit, n_hit, n_hit + 1)
    for n in (1, 2, 3, 63, 64, 65, 255, 256, 257):
        vtx, faces = ic.crossing_strips(n)
        st = ic.both(vtx, faces)["stats"]
        assert st["n_faces"] == n and (n < 2 or st["n_pairs"] >= n // 2)
