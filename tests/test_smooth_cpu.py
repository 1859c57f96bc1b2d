"""CPU tier of the one-ring table, the smoothing and the vertex normals (include/immesh_smooth.h): the header as plain C99 on its own, the library's
new symbols, immesh_smooth_stats' layout, and the checker (tests/smooth_checker.py) against its brute force, the facts the header states against the
topology checker, what Taubin and Laplace do to a noisy torus, the border rules on a sheet, the sum whose result depends on its order, the hold, and
the zero a step with w == 0 turns around."""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import simplify_checker as sc
import smooth_checker as sm
import topology_checker as tc
from immesh_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "immesh_smooth.h")
NEW_SYMBOLS = ("immesh_smooth", "immesh_smooth_vertices", "immesh_smooth_adjacency", "immesh_smooth_apply", "immesh_smooth_last_timing",
               "immesh_vertex_normals")
DEFINES = (("IMMESH_VERTEX_UNUSED", sm.UNUSED), ("IMMESH_VERTEX_NOT_FINITE", sm.NOT_FINITE), ("IMMESH_VERTEX_BORDER", sm.BORDER),
           ("IMMESH_VERTEX_INTERIOR", sm.INTERIOR), ("IMMESH_SMOOTH_BORDER_FIXED", sm.FIXED), ("IMMESH_SMOOTH_BORDER_ALONG", sm.ALONG),
           ("IMMESH_SMOOTH_BORDER_FREE", sm.FREE), ("IMMESH_SMOOTH_MAX_STEPS", 65536))
FACTORS = ((0.5, -0.53), (0.5, 0.5), (1.0, -1.0), (0.0, 0.3), (-0.25, 0.9), (0.63, -0.67))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(capi.hip_library_path()):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "immesh_amd", "csrc"), "-j8"])
    return capi.load_hip_library()


# ---- the boundary ----------------------------------------------------------------------------------------------------------------------------
def test_header_is_plain_c99_on_its_own(tmp_path):
    src = tmp_path / "alone.c"
    src.write_text('#include "immesh_smooth.h"\nint main(void) { immesh_smooth_stats s; float ms[3]; int rc;\n'
                   '  s.n_moved = ' + " + ".join(n for n, _ in DEFINES) + ';\n'
                   '  rc = immesh_smooth(0, 0, 0.5, -0.53, IMMESH_SMOOTH_BORDER_FIXED, &s) + immesh_smooth_vertices(0, 0, 0)\n'
                   '     + immesh_smooth_adjacency(0, 0, 0, 0, 0, 0) + immesh_smooth_apply(0) + immesh_smooth_last_timing(0, ms) + immesh_vertex_normals(0, 0, 0);\n'
                   '  return rc + (int)s.n_moved; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "alone.o")])


def test_library_exports_the_smoothing(lib):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    fns = sorted(set(re.findall(r"\b(immesh_[a-z_0-9]+)\s*\(", src)))
    assert fns == sorted(NEW_SYMBOLS)
    missing = [f for f in fns if not hasattr(lib, f)]
    assert not missing, missing


def test_smooth_stats_layout_and_constants(tmp_path):
    names = [n for n, _ in capi.SmoothStats._fields_]
    assert tuple(names) == sm.STAT_NAMES
    prog = tmp_path / "layout.c"
    prog.write_text('#include "immesh_smooth.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void) {\n  printf("%zu", sizeof(immesh_smooth_stats));\n'
                    + "".join('  printf(" %%zu", offsetof(immesh_smooth_stats, %s));\n' % n for n in names)
                    + "".join('  printf(" %%d", %s);\n' % n for n, _ in DEFINES) + "  return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(prog), "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe]).split()]
    assert got == [C.sizeof(capi.SmoothStats)] + [getattr(capi.SmoothStats, n).offset for n in names] + [v for _, v in DEFINES]
    assert (capi.VERTEX_UNUSED, capi.VERTEX_NOT_FINITE, capi.VERTEX_BORDER, capi.VERTEX_INTERIOR) == (sm.UNUSED, sm.NOT_FINITE, sm.BORDER, sm.INTERIOR)
    assert (capi.SMOOTH_BORDER_FIXED, capi.SMOOTH_BORDER_ALONG, capi.SMOOTH_BORDER_FREE) == (sm.FIXED, sm.ALONG, sm.FREE)


# ---- the checker against the brute force ---------------------------------------------------------------------------------------------------------
def _cases():
    rng = np.random.default_rng(2024)
    for k in range(60):
        yield "soup %d" % k, tc.random_soup(rng, int(rng.integers(1, 40)), int(rng.integers(3, 14)))
    for k in range(40):
        v, f = tc.random_soup(rng, int(rng.integers(4, 40)), int(rng.integers(4, 14)))
        yield "soup with specials %d" % k, (sm.with_specials(rng, v, int(rng.integers(1, 5))), f)
    for k in range(30):
        m, n = int(rng.integers(2, 6)), int(rng.integers(2, 6))
        holes = [(int(rng.integers(0, m)), int(rng.integers(0, n))) for _ in range(int(rng.integers(0, 3)))]
        v, f = tc.grid_sheet(m, n, holes)
        v = sm.noisy(rng, v, 0.1)
        yield "sheet %d" % k, (sm.with_specials(rng, v, 2) if k % 3 == 0 else v, f[rng.permutation(len(f))])
    for k, (m, n) in enumerate(((3, 3), (4, 3), (5, 4), (6, 3))):
        v, f = tc.torus(m, n)
        yield "torus %d" % k, (sm.noisy(rng, v, 0.05), f)
    for k, n in enumerate((3, 4, 5, 8)):
        v, f = tc.moebius(n)
        yield "moebius %d" % k, (sm.noisy(rng, v, 0.05), f)
    yield "fins", sm.fins()
    yield "no face", (np.zeros((3, 3), np.float32), np.zeros((0, 3), np.int32))
    yield "nothing", (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))


def test_checker_against_the_brute_force_and_the_facts():
    n = 0
    for k, (name, (vtx, faces)) in enumerate(_cases()):
        for border in (sm.FIXED, sm.ALONG, sm.FREE):
            lam, mu = FACTORS[(k + border) % len(FACTORS)]
            n_steps = (k + 2 * border) % 5
            res = sm.smooth(vtx, faces, n_steps, lam, mu, border)
            sm.same_as_brute(res, sm.brute(vtx, faces, n_steps, lam, mu, border))
            sm.check_facts(vtx, faces, res)
            n += 1
        got, n_zero = sm.normals(vtx, faces)
        assert (got.view(np.uint32).tolist(), n_zero) == sm.brute_normals(vtx, faces), name
    assert n > 400


# ---- what the rule does ------------------------------------------------------------------------------------------------------------------------------
def test_taubin_denoises_a_torus_and_laplace_shrinks_it():
    rng = np.random.default_rng(12)
    vtx, faces = tc.torus(40, 24)
    noisy = (vtx.astype(np.float64) + sm.torus_normals(40, 24) * rng.normal(scale=0.02, size=(len(vtx), 1))).astype(np.float32)
    rms = lambda v: float(np.sqrt(np.mean(sm.torus_distance(v) ** 2)))
    before = rms(noisy)
    taubin = sm.smooth(noisy, faces, 10, 0.5, -0.53, sm.FIXED)
    laplace = sm.smooth(noisy, faces, 10, 0.5, 0.5, sm.FIXED)
    print("rms distance to the torus: %.4f before, %.4f after 10 steps of (0.5, -0.53), %.4f after 10 steps of (0.5, 0.5)"
          % (before, rms(taubin["vtx_out"]), rms(laplace["vtx_out"])))
    assert 0.018 < before < 0.022
    assert rms(taubin["vtx_out"]) < before < rms(laplace["vtx_out"])
    assert taubin["stats"]["n_interior"] == taubin["stats"]["n_moving"] == taubin["stats"]["n_moved"] == len(vtx) and taubin["stats"]["n_border"] == 0
    assert taubin["stats"]["max_valence"] == 6 and taubin["stats"]["n_pairs"] == 6 * len(vtx) and taubin["stats"]["n_held"] == 0
    got, n_zero = sm.normals(taubin["vtx_out"], faces)
    assert n_zero == 0 and ((got.astype(np.float64) * sm.torus_normals(40, 24)).sum(axis=1) > 0.95).all()   # wound outwards, and close to the analytic ones


def test_the_border_rules_on_a_noisy_sheet():
    rng = np.random.default_rng(4)
    vtx, faces = tc.grid_sheet(6, 5)
    vtx = sm.noisy(rng, vtx, 0.05)
    moved = {}
    for border in (sm.FIXED, sm.ALONG, sm.FREE):
        res = sm.smooth(vtx, faces, 3, 0.5, -0.53, border)
        on_border = res["vclass"] == sm.BORDER
        assert on_border.sum() == 22 == res["stats"]["n_border"] and res["stats"]["n_interior"] == 20
        moved[border] = int((res["vtx_out"][on_border].view(np.uint32) != vtx[on_border].view(np.uint32)).any(axis=1).sum())
        assert res["stats"]["n_moving"] == (20 if border == sm.FIXED else 42)
    assert moved == {sm.FIXED: 0, sm.ALONG: 22, sm.FREE: 22}
    along = sm.smooth(vtx, faces, 1, 1.0, 1.0, sm.ALONG)["vtx_out"]                     # a border vertex goes to the mean of its two border neighbours
    assert along[1].tolist() == ((vtx[0].astype(np.float64) + vtx[2]) / 2.0).astype(np.float32).tolist()


def test_the_sum_depends_on_its_order_the_hold_and_the_zero():
    got = set()
    for order in itertools.permutations(range(3)):
        vtx, faces = sm.closed_fan(0.0, [sc.ORDER_TRIPLE[i] for i in order])
        assert vtx[1:, 0].astype(np.float64).tolist() == [sc.ORDER_TRIPLE[i] for i in order]
        res = sm.smooth(vtx, faces, 1, 1.0, 1.0, sm.FREE)
        sm.same_as_brute(res, sm.brute(vtx, faces, 1, 1.0, 1.0, sm.FREE))
        assert res["stats"]["n_moving"] == 4 and res["stats"]["n_border"] == 3 and res["vclass"][0] == sm.INTERIOR
        got.add(int(res["vtx_out"][0, 0].view(np.uint32)))
    assert len(got) == 2
    vtx, faces = sm.closed_fan(3e38, (-3e38, -3e38, -3e38))                             # x + (-1)(m - x) overflows a float at every vertex
    res = sm.smooth(vtx, faces, 1, -1.0, -1.0, sm.FREE)
    sm.same_as_brute(res, sm.brute(vtx, faces, 1, -1.0, -1.0, sm.FREE))
    assert res["stats"]["n_held"] == 4 and res["stats"]["n_moved"] == 0 and res["vtx_out"].tobytes() == vtx.tobytes() and res["stats"]["max_disp2"] == 0.0
    vtx, faces = sm.closed_fan(-0.0, (1.0, 2.0, 3.0))
    assert np.signbit(vtx[0, 0])
    res = sm.smooth(vtx, faces, 1, 0.0, 0.0, sm.FREE)
    sm.same_as_brute(res, sm.brute(vtx, faces, 1, 0.0, 0.0, sm.FREE))
    assert res["vtx_out"][0, 0] == 0.0 and not np.signbit(res["vtx_out"][0, 0]) and res["stats"]["n_moved"] == 1 and res["stats"]["max_disp2"] == 0.0
    assert res["vtx_out"][1:].tobytes() == vtx[1:].tobytes()
