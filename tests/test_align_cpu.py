"""CPU tier of the alignment (include/immesh_align.h): the checker (tests/align_checker.py) against independent statements of what it computes --
numpy's least squares on the stacked rows, a series of the matrix exponential, the known pose of the convergence case -- the header as plain C with
the ctypes records' sizes and offsets, and the library's two pure host functions (the solve, the update) against the checker."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import align_checker as ac
from immesh_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rows(mode, p, centre, face, q, A):
    """the stacked rows (J, r) of the taking-part points, written independently of the checker's terms: plain numpy cross products"""
    J, r = [], []
    for i in np.nonzero(face >= 0)[0]:
        x = p[i] - centre
        if mode == ac.POINT:
            for k in range(3):
                u = np.eye(3)[k]
                J.append(np.concatenate([np.cross(x, u), u])); r.append(q[i, k])
        else:
            n = np.cross(A[i, 1] - A[i, 0], A[i, 2] - A[i, 0])
            if not np.dot(n, n) > 0:
                continue
            u = n / np.linalg.norm(n)
            J.append(np.concatenate([np.cross(x, u), u])); r.append(np.dot(u, A[i, 0]))
    return np.array(J), np.array(r)


@pytest.fixture(scope="module")
def case():
    vtx, faces, cloud = ac.convergence_case()
    return vtx, faces, cloud, cloud.astype(np.float64).mean(axis=0)


@pytest.mark.parametrize("mode", [ac.POINT, ac.PLANE])
def test_delta_equals_least_squares_on_the_stacked_rows(case, mode):
    vtx, faces, cloud, centre = case
    pts = cloud[:600]
    p, ok, face, q, A = ac.correspondences(None, None, pts, 0.5, vtx, faces)
    tm, used, flat = ac.terms(mode, p, centre, face, q, A)
    sums, _, counts = ac.system(tm, ok, face, used, flat)
    assert counts[0] > 300 and sum(counts) == len(pts)
    bad, delta = ac.solve(sums, 0.0)
    J, r = _rows(mode, p, centre, face, q, A)
    assert len(r) == (3 if mode == ac.POINT else 1) * counts[0]
    ref = np.linalg.lstsq(J, r, rcond=None)[0]
    assert not bad and np.linalg.cond(J) < 100                                      # well conditioned: the centre is the cloud's mean
    assert np.abs(delta - ref).max() <= 1e-10, np.abs(delta - ref).max()
    # and the terms are the rows' outer products: H = J^T J, g = J^T r, e = r . r
    H = np.array([[sums[ac.h_index(min(a, b), max(a, b))] for b in range(6)] for a in range(6)])
    assert np.allclose(H, J.T @ J, rtol=1e-12, atol=1e-12) and np.allclose(sums[21:27], J.T @ r, rtol=1e-12, atol=1e-12)
    assert math.isclose(sums[27], float(r @ r), rel_tol=1e-12)


def _series(w, n=30):
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], np.float64)
    out, term = np.eye(3), np.eye(3)
    for k in range(1, n):
        term = term @ K / k
        out = out + term
    return out


def test_exp_is_the_matrix_exponential_and_orthogonal():
    rng = np.random.default_rng(3)
    ws = [rng.normal(size=3) * s for s in (1.0, 0.3, 1e-2, 1e-5, 1e-7, 2.0 ** -26, 2.0 ** -27, 1e-12, 0.0) for _ in range(4)]
    ws += [np.array([0.0, 0.0, 2.0 ** -26]), np.array([np.nextafter(2.0 ** -26, 0), 0.0, 0.0]), np.array([1.5, -2.0, 0.5])]
    for w in ws:
        E = ac.exp(w)
        assert np.abs(E - _series(w)).max() <= 1e-14, (w, np.abs(E - _series(w)).max())
        assert np.abs(E @ E.T - np.eye(3)).max() <= 1e-14, w


def test_update_moves_points_about_the_centre():
    rng = np.random.default_rng(4)
    R0, t0, ce = ac.rodrigues(rng.normal(size=3), 0.7), rng.normal(size=3) * 10, rng.normal(size=3) * 100
    delta = np.concatenate([rng.normal(size=3) * 0.1, rng.normal(size=3)])
    R1, t1 = ac.update(R0, t0, ce, delta)
    x = rng.normal(size=(5, 3))
    want = (ac.exp(delta[:3]) @ ((x @ R0.T + t0) - ce).T).T + ce + delta[3:]           # p' = Exp(w) (p - centre) + centre + v
    assert np.abs((x @ R1.T + t1) - want).max() < 1e-12


def _plane_system(n=50):
    """points above the single face z = 0: every row is (cross(x, e_z), e_z), so H has rank 3 (rotation about z and the two translations in the plane
    are free)"""
    rng = np.random.default_rng(5)
    vtx = np.array([[-10, -10, 0], [10, -10, 0], [0, 10, 0]], np.float32)
    faces = np.array([[0, 1, 2]], np.int32)
    pts = np.concatenate([rng.uniform(-3, 3, (n, 2)), rng.uniform(0.01, 0.2, (n, 1))], axis=1).astype(np.float32)
    return vtx, faces, pts


def test_rank_deficient_system_is_degenerate_until_damped():
    vtx, faces, pts = _plane_system()
    s = ac.step(None, None, pts, ac.PLANE, 1.0, np.zeros(3), vtx, faces)
    assert s["counts"] == (len(pts), 0, 0, 0)
    bad, delta = ac.solve(s["sums"], 0.0)
    assert bad and not delta.any()
    bad, delta = ac.solve(s["sums"], 1e-6)
    assert not bad and np.isfinite(delta).all() and abs(delta[5]) > 0.01               # it moves along z, towards the plane
    assert ac.solve(np.zeros(28), 0.0)[0] and ac.solve(np.full(28, np.nan), 1.0)[0]
    r = ac.loop(None, None, pts, ac.PLANE, 1.0, np.zeros(3), 0.0, 5, 1e-10, 1e-10, vtx, faces)
    assert r["status"] == ac.DEGENERATE and r["iterations"] == 1 and np.array_equal(r["rot"], np.eye(3)) and not r["pos"].any()


def test_the_loop_recovers_the_known_pose(case):
    """The cloud lies on the sheet's faces once moved by (TRUE_ROT, TRUE_POS); its float storage leaves ~2e-8 m of noise.  If this fails, the input of
    the GPU tier's convergence test is wrong, not the library."""
    vtx, faces, cloud, centre = case
    r = ac.loop(None, None, cloud, ac.PLANE, 0.5, centre, 0.0, 30, 1e-10, 1e-10, vtx, faces)
    assert r["status"] == ac.CONVERGED and 3 <= r["iterations"] <= 10
    rms = r["history"][:, 1]
    assert (np.diff(rms[1:]) <= 0).all() and rms[-1] < 1e-6, rms
    dR = r["rot"] @ ac.TRUE_ROT.T
    angle = math.acos(min(1.0, (np.trace(dR) - 1.0) / 2.0))
    assert angle <= 1e-4 and np.abs(r["pos"] - ac.TRUE_POS).max() <= 1e-4, (angle, r["pos"] - ac.TRUE_POS)
    # POINT rows on the same case: it slides along the sheet, linearly; the rms falls and 30 iterations do not converge
    r = ac.loop(None, None, cloud[:1000], ac.POINT, 0.5, centre, 0.0, 8, 1e-10, 1e-10, vtx, faces)
    assert r["status"] == ac.MAX_ITERS and r["iterations"] == 8 and (np.diff(r["history"][:, 1]) < 0).all()


def test_statuses_of_the_loop():
    vtx, faces, pts = _plane_system(5)
    none = np.zeros((0, 3), np.float32)
    for mode, p, want in ((ac.PLANE, none, ac.TOO_FEW), (ac.POINT, none, ac.TOO_FEW), (ac.PLANE, pts, ac.TOO_FEW), (ac.POINT, pts[:2], ac.TOO_FEW)):
        r = ac.loop(None, None, p, mode, 1.0, np.zeros(3), 1e-6, 4, 1e-10, 1e-10, vtx, faces)
        assert (r["status"], r["iterations"]) == (want, 1) and np.array_equal(r["rot"], np.eye(3)) and not r["pos"].any()


# ---- the header and the bindings ---------------------------------------------------------------------------------------------------------------------
LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "immesh_align.h"
#define F(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))
int main(void) {
    printf("immesh_align_options %zu\nimmesh_align_system %zu\nimmesh_align_result %zu\n", sizeof(immesh_align_options), sizeof(immesh_align_system),
           sizeof(immesh_align_result));
    F(immesh_align_options, mode); F(immesh_align_options, max_iters); F(immesh_align_options, max_dist); F(immesh_align_options, centre);
    F(immesh_align_options, damping); F(immesh_align_options, eps_rot); F(immesh_align_options, eps_trans);
    F(immesh_align_system, H); F(immesh_align_system, g); F(immesh_align_system, e); F(immesh_align_system, n_used);
    F(immesh_align_system, n_not_finite); F(immesh_align_system, n_no_face); F(immesh_align_system, n_flat);
    F(immesh_align_result, frame); F(immesh_align_result, status); F(immesh_align_result, iterations); F(immesh_align_result, system);
    F(immesh_align_result, rms);
    printf("%d %d %d %d %d %d\n", IMMESH_ALIGN_POINT, IMMESH_ALIGN_PLANE, IMMESH_ALIGN_CONVERGED, IMMESH_ALIGN_MAX_ITERS, IMMESH_ALIGN_TOO_FEW,
           IMMESH_ALIGN_DEGENERATE);
    return 0;
}
"""


def test_header_is_plain_c_and_the_records_match(tmp_path):
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text(LAYOUT_C)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    got = dict(line.rsplit(" ", 1) for line in lines[:-2])
    records = {"immesh_align_options": capi.AlignOptions, "immesh_align_system": capi.AlignSystem, "immesh_align_result": capi.AlignResult}
    want = {name: str(C.sizeof(t)) for name, t in records.items()}
    for name, t in records.items():
        want.update({f"{name}.{f}": str(getattr(t, f).offset) for f, _ in t._fields_})
    assert got == want
    assert lines[-2].split() == [str(v) for v in (capi.ALIGN_POINT, capi.ALIGN_PLANE, capi.ALIGN_CONVERGED, capi.ALIGN_MAX_ITERS, capi.ALIGN_TOO_FEW,
                                                  capi.ALIGN_DEGENERATE)]
    assert (ac.POINT, ac.PLANE, ac.CONVERGED, ac.MAX_ITERS, ac.TOO_FEW, ac.DEGENERATE) == (0, 1, 0, 1, 2, 3) and capi.ALIGN_TERMS == ac.N_TERMS
    text = open(os.path.join(ROOT, "include", "immesh_align.h")).read()
    assert '#include "immesh_raycast.h"' in text and "immesh_closest.h" not in text        # the point-to-mesh header's rule: no other header names it
    for other in os.listdir(os.path.join(ROOT, "include")):                                   # nothing includes it
        assert other == "immesh_align.h" or "immesh_align.h" not in open(os.path.join(ROOT, "include", other)).read(), other


@pytest.fixture(scope="module")
def lib():
    return capi.load_hip_library()                                                            # loads without a device, as test_capi_symbols.py does


def test_library_exports_the_calls(lib):
    for name in ("immesh_align_default_options", "immesh_align_step", "immesh_align_solve", "immesh_align_update", "immesh_align",
                 "immesh_align_last_timing", "immesh_align_set_variant"):
        assert hasattr(lib, name), name
    f = lib.immesh_align_default_options; f.argtypes = [C.POINTER(capi.AlignOptions)]; f.restype = None
    o = capi.AlignOptions()
    f(C.byref(o))
    assert bytes(o) == bytes(capi.align_options())


def _system(sums):
    s = capi.AlignSystem()
    s.H[:], s.g[:], s.e = list(sums[:21]), list(sums[21:27]), float(sums[27])
    return s


def test_library_solve_and_update_agree_with_the_checker(lib, case):
    vtx, faces, cloud, centre = case
    rng = np.random.default_rng(6)
    for mode in (ac.POINT, ac.PLANE):
        sums = ac.step(None, None, cloud[:400], mode, 0.5, centre, vtx, faces)["sums"]
        for damping in (0.0, 1e-3):
            bad, delta = capi.align_solve(lib, _system(sums), damping)
            rbad, rdelta = ac.solve(sums, damping)
            assert not bad and not rbad and np.abs(delta - rdelta).max() <= 1e-12 * np.abs(rdelta).max()
            rot, pos = ac.rodrigues(rng.normal(size=3), 0.4), rng.normal(size=3) * 5
            got = capi.align_update(lib, capi.ray_frame(rot, pos), centre, delta)
            rrot, rpos = ac.update(rot, pos, centre, rdelta)
            assert np.abs(np.array(list(got.rot)).reshape(3, 3) - rrot).max() <= 1e-12
            assert np.abs(np.array(list(got.pos)) - rpos).max() <= 1e-12 * max(1.0, np.abs(rpos).max())
    for w in (np.zeros(3), np.array([1e-9, 0, 0]), np.array([2.0 ** -26, 0, 0]), np.array([0.5, -1.0, 2.0])):   # both arms of Exp
        d = np.concatenate([w, [0.1, 0.2, 0.3]])
        got = capi.align_update(lib, capi.ray_frame(), [1.0, 2.0, 3.0], d)
        rrot, rpos = ac.update(np.eye(3), np.zeros(3), [1.0, 2.0, 3.0], d)
        assert np.abs(np.array(list(got.rot)).reshape(3, 3) - rrot).max() <= 1e-12 and np.abs(np.array(list(got.pos)) - rpos).max() <= 1e-12


def test_library_degenerate_cases_agree_exactly(lib):
    vtx, faces, pts = _plane_system()
    sums = ac.step(None, None, pts, ac.PLANE, 1.0, np.zeros(3), vtx, faces)["sums"]
    tiny = sums.copy(); tiny[ac.h_index(5, 5)] = 0.0                                         # and a zero on the diagonal
    nan = sums.copy(); nan[3] = np.nan
    for s, damping in ((sums, 0.0), (np.zeros(28), 0.0), (tiny, 0.0), (nan, 1.0), (sums, 2.0 ** -45 * sums[:21].max())):
        bad, delta = capi.align_solve(lib, _system(s), damping)
        assert bad and ac.solve(s, damping)[0] and not delta.any()
    bad, delta = capi.align_solve(lib, _system(sums), 1e-6)
    rbad, rdelta = ac.solve(sums, 1e-6)
    assert not bad and not rbad and np.abs(delta - rdelta).max() <= 1e-12 * np.abs(rdelta).max()
    f = lib.immesh_align_solve; f.argtypes = [C.POINTER(capi.AlignSystem), C.c_double, C.c_void_p]; f.restype = C.c_int
    out = np.zeros(6)
    for damping in (-1.0, np.inf, np.nan):
        assert f(C.byref(_system(sums)), damping, out.ctypes.data_as(C.c_void_p)) == -1
