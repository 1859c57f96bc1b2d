"""The numpy restatement of the Normals and Agreement rules (tests/normals_checker.py, include/immesh_normals.h) pinned without a GPU: known
answers, a cross-check of the normals against numpy.linalg.eigh, the vectorised Jacobi against the oracle library's orc_sym3_eigen bit for bit, and
the Agreement rule on a hand-made soup."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import knn_checker as kc
import normals_checker as nk


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "immesh_normals.h")


# ---- the boundary --------------------------------------------------------------------------------------------------------------------------------
def test_header_is_plain_c99_and_names_no_sibling(tmp_path):
    """the header alone, and with the headers that define the index's typedef and the statistics struct before and after it; it names neither (their
    rule), and no other header names it"""
    body = "int main(void) { struct immesh_cloud_index* x = 0; return (x != 0) + IMMESH_NORMALS_VIEWPOINT + IMMESH_RAY_NEAREST; }\n"
    full = ("int main(void) { immesh_closest_stats s; immesh_cloud_index* x = 0; double v[3] = {0, 0, 0}; int64_t c[4]; s.n_points = 0; "
            "return (int)s.n_points + immesh_cloud_normals(x, 8, 1.0, 0.0, IMMESH_NORMALS_CANONICAL, v, 0, 0, 0, 0, 0, c) + "
            "immesh_normals_agree_reduce(x, 1.0, 1, &s, 0); }\n")
    others = '#include "immesh_nearest.h"\n#include "immesh_closest.h"\n'
    for k, text in enumerate(('#include "immesh_normals.h"\n' + body, '#include "immesh_normals.h"\n' + others + full, others + '#include "immesh_normals.h"\n' + full)):
        src = tmp_path / ("unit%d.c" % k)
        src.write_text(text)
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-c", "-I", os.path.join(ROOT, "include"), str(src),
                               "-o", str(tmp_path / ("unit%d.o" % k))])
    text = open(HEADER).read()
    assert '#include "immesh_raycast.h"' in text and "struct immesh_cloud_index;" in text and "struct immesh_closest_stats;" in text
    for name in os.listdir(os.path.join(ROOT, "include")):
        if name != "immesh_normals.h":
            assert "immesh_normals.h" not in open(os.path.join(ROOT, "include", name)).read(), name
            assert name in ("immesh_raycast.h", "immesh_c_api.h") or name not in text, name


def test_declared_symbols_and_bindings():
    from immesh_amd import capi
    code = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    fns = sorted(set(re.findall(r"\b(immesh_[a-z_0-9]+)\s*\(", code)))
    assert fns == ["immesh_cloud_normals", "immesh_cloud_normals_get", "immesh_normals_agree_cloud", "immesh_normals_agree_reduce",
                   "immesh_normals_agree_samples", "immesh_normals_last_timing"]
    assert (capi.NORMALS_CANONICAL, capi.NORMALS_VIEWPOINT) == (nk.CANONICAL, nk.VIEWPOINT) == (0, 1)
    assert re.search(r"#define IMMESH_NORMALS_CANONICAL 0\b", code) and re.search(r"#define IMMESH_NORMALS_VIEWPOINT 1\b", code)
    for name in ("cloud_normals", "cloud_normals_get", "normals_agree_samples", "normals_agree_cloud", "normals_agree_stats", "normals_timing"):
        assert callable(getattr(capi.HotPath, name))
    if os.path.exists(capi.hip_library_path()):                                      # (built: every declared symbol is exported)
        lib = capi.load_hip_library()
        assert not [f for f in fns if not hasattr(lib, f)]


def noisy_sheet(n=400, seed=7, offset=0.0):
    """n points of a gently curved sheet with noise across it, in random order"""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(-1.0, 1.0, (n, 2))
    z = 0.15 * np.sin(2.0 * xy[:, 0]) + 0.1 * xy[:, 1] ** 2 + rng.normal(0.0, 0.004, n)
    return (np.concatenate([xy, z[:, None]], axis=1) + offset).astype(np.float32)


# ---- known answers ---------------------------------------------------------------------------------------------------------------------------------
def test_plane_lattice_has_the_plane_normal():
    g = np.arange(6, dtype=np.float32)
    cloud = np.concatenate([np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2), np.zeros((36, 1), np.float32)], axis=1)
    for c in (cloud, cloud[np.random.default_rng(1).permutation(36)]):
        out = nk.normals(c, 8, 100.0)
        assert (out["status"] == 0).all() and (out["count"] == 8).all() and out["counts"].tolist() == [36, 0, 0, 0]
        assert out["normal"].tobytes() == np.tile(np.array([0, 0, 1], np.float32), (36, 1)).tobytes()
        assert (out["eig"][:, 0] == 0.0).all() and (out["curvature"] == 0.0).all() and (out["eig"][:, 1] > 0).all()


def test_cubic_lattice_interior_point_needs_no_rotation():
    g = np.arange(4, dtype=np.float32)
    cloud = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    out = nk.normals(cloud, 6, 100.0)
    inner = np.nonzero(((cloud >= 1) & (cloud <= 2)).all(axis=1))[0]
    assert len(inner) == 8 and (out["count"][inner] == 6).all() and (out["sweeps"][inner] == 0).all()
    # six neighbours at distance 1 along the axes: C = diag(2 / 7), three equal eigenvalues, position 0 wins, V = I
    assert (out["eig"][inner] == 2.0 / 7.0).all() and (out["status"][inner] == 0).all()
    assert out["normal"][inner].tobytes() == np.tile(np.array([1, 0, 0], np.float32), (8, 1)).tobytes()
    assert (out["curvature"][inner] == (2.0 / 7.0) / ((2.0 / 7.0 + 2.0 / 7.0) + 2.0 / 7.0)).all()


def test_collinear_points_are_line_like():
    cloud = np.stack([np.arange(10), 2 * np.arange(10), np.zeros(10)], axis=1).astype(np.float32)
    out = nk.normals(cloud, 4, 100.0, min_ratio=0.0)
    assert (out["status"] == 3).all() and out["counts"].tolist() == [0, 0, 10, 0]
    assert np.isnan(out["normal"]).all() and (out["normal"].view(np.uint32) == 0x7FC00000).all()
    assert (out["eig"][:, 1] <= 0.0).all() and (out["eig"][:, 2] > 0.0).all() and (out["curvature"] >= 0.0).all()   # eig and curvature are given


def test_statuses_and_placeholders():
    cloud = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [np.nan, 0, 0], [50, 50, 50], [0, 0, 1]], np.float32)
    out = nk.normals(cloud, 3, 2.0)
    assert out["status"].tolist() == [0, 0, 0, 2, 1, 0] and out["count"].tolist() == [3, 3, 3, 0, 0, 3] and out["counts"].tolist() == [4, 1, 0, 1]
    for i in (3, 4):
        assert (out["normal"][i].view(np.uint32) == 0x7FC00000).all() and (out["eig"][i] == -1.0).all() and out["curvature"][i] == -1.0
    assert np.isfinite(out["normal"][[0, 1, 2, 5]]).all()


def test_viewpoint_flips_and_keeps_on_zero():
    g = np.arange(5, dtype=np.float32)
    cloud = np.concatenate([np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2), np.zeros((25, 1), np.float32)], axis=1)
    up = nk.normals(cloud, 8, 100.0, mode=nk.VIEWPOINT, viewpoint=[2.0, 2.0, 3.0])["normal"]
    down = nk.normals(cloud, 8, 100.0, mode=nk.VIEWPOINT, viewpoint=[2.0, 2.0, -3.0])["normal"]
    flat = nk.normals(cloud, 8, 100.0, mode=nk.VIEWPOINT, viewpoint=[9.0, -4.0, 0.0])["normal"]       # in the plane: t == 0, the canonical sign stays
    assert (up[:, 2] == 1).all() and (down[:, 2] == -1).all() and (flat[:, 2] == 1).all() and (down[:, :2] == 0).all()


# ---- against numpy.linalg.eigh -----------------------------------------------------------------------------------------------------------------------
def test_normals_against_eigh():
    """the smallest eigenvector of the same neighbourhoods by LAPACK.  The angle between two computed eigenvectors is bounded by the error of the
    matrix over the gap: with the gap lambda_mid - lambda_s >= 1e-3 lambda_hi and at most 64 sweeps of rotations of relative error 2^-52 each,
    1e3 x 64 x 2^-52 = 1.4e-11; 1e-10 is that rounded up"""
    cloud = noisy_sheet()
    count, index, _, _ = kc.knn_cloud(cloud, 12, 100.0)
    out = nk.normals(cloud, 12, 100.0, lists=(count, index))
    assert (out["status"] == 0).all()
    gap_ok = out["eig"][:, 1] - out["eig"][:, 0] >= 1e-3 * out["eig"][:, 2]
    assert gap_ok.sum() == len(cloud) == 400                                          # the restriction hides nothing
    worst = 0.0
    for i in np.nonzero(gap_ok)[0]:
        q = np.concatenate([np.zeros((1, 3)), cloud[index[i]].astype(np.float64) - cloud[i].astype(np.float64)])
        r = q - q.mean(axis=0)
        w, v = np.linalg.eigh(r.T @ r / len(q))
        n = out["normal"][i].astype(np.float64)
        worst = max(worst, np.linalg.norm(np.cross(v[:, 0], n / np.linalg.norm(n))))
        assert abs(w[0] - out["eig"][i, 0]) <= 1e-12 * w[2] and abs(w[2] - out["eig"][i, 2]) <= 1e-12 * w[2]
    print("sine of the angle to eigh's normal, float normals: %.3g; sweeps at most %d" % (worst, out["sweeps"].max()))
    # the stored normal is a float: its direction is within 2^-24 per component of the double one; the double one is what the bound is about
    lam, V, _ = nk.jacobi(nk.covariance(cloud, count, index))
    worst = 0.0
    for i in range(len(cloud)):
        q = np.concatenate([np.zeros((1, 3)), cloud[index[i]].astype(np.float64) - cloud[i].astype(np.float64)])
        r = q - q.mean(axis=0)
        _, v = np.linalg.eigh(r.T @ r / len(q))
        worst = max(worst, np.linalg.norm(np.cross(v[:, 0], V[i][:, int(np.argmin(lam[i]))])))
    print("sine of the angle to eigh's normal, double eigenvectors: %.3g" % worst)
    assert worst <= 1e-10


# ---- the Jacobi against the oracle library ---------------------------------------------------------------------------------------------------------------
def test_jacobi_equals_the_oracle_bit_for_bit(oracle_lib):
    cloud = noisy_sheet()
    count, index, _, _ = kc.knn_cloud(cloud, 12, 100.0)
    C6 = nk.covariance(cloud, count, index)
    rng = np.random.default_rng(5)
    extra = []
    for _ in range(100):                                                             # and matrices that are no covariance of a sheet
        B = rng.normal(size=(3, 3)) * rng.choice([1e-6, 1.0, 1e4])
        A = B @ B.T
        extra.append([A[0, 0], A[0, 1], A[0, 2], A[1, 1], A[1, 2], A[2, 2]])
    extra += [[2, 0, 0, 2, 0, 2], [1, 1e-320, 0, 1, 0, 1], [1, 1e-20, 1e-20, 2, 1e-20, 3], [0, 0, 0, 0, 0, 0], [1, 1, 1, 1, 1, 1], [3, -1, 0, 3, 0, 5]]
    C6 = np.concatenate([C6, np.array(extra, np.float64)])
    lam, V, _ = nk.jacobi(C6)
    f = oracle_lib.orc_sym3_eigen
    f.argtypes = [C.c_void_p] * 3; f.restype = None
    for i, c in enumerate(C6):
        A = np.array([c[0], c[1], c[2], c[1], c[3], c[4], c[2], c[4], c[5]], np.float64)
        ev, vv = np.zeros(3), np.zeros(9)
        f(A.ctypes.data_as(C.c_void_p), ev.ctypes.data_as(C.c_void_p), vv.ctypes.data_as(C.c_void_p))
        assert ev.tobytes() == lam[i].tobytes() and vv.tobytes() == np.ascontiguousarray(V[i]).tobytes(), (i, c.tolist(), ev.tolist(), lam[i].tolist())


# ---- the Agreement rule ------------------------------------------------------------------------------------------------------------------------------
def test_agreement_on_a_tilted_square():
    """a square in the plane z = x (normal (-1, 0, 1) / sqrt 2) of two faces, a zero-area face and a face with a NaN vertex"""
    vtx = np.array([[0, 0, 0], [2, 0, 2], [2, 2, 2], [0, 2, 0], [5, 5, 5], [6, 6, 6], [7, 7, 7], [np.nan, 0, 0]], np.float32)
    faces = np.array([[0, 1, 2], [0, 2, 3], [4, 5, 6], [0, 1, 7]], np.int32)
    cr, l2, part = nk.face_normals(vtx, faces)
    assert part.tolist() == [True, True, False, False] and cr[0].tolist() == [-4.0, 0.0, 4.0] and l2[0] == 32.0 and l2[2] == 0.0
    r = np.float32(np.sqrt(0.5))
    normal = np.array([[-r, 0, r], [r, 0, -r], [0, 1, 0], [np.nan] * 3, [0, 0, 1]], np.float32)
    status = np.array([0, 0, 0, 1, 0], np.uint8)
    sface = np.array([0, 1, 0, 1, 2, 3, 0, 1], np.int64)
    index = np.array([0, 1, 2, 3, 0, 0, -1, 4], np.int64)
    agree, pair, counts = nk.agree_samples(sface, index, normal, status, vtx, faces)
    assert pair.tolist() == [True, True, True, False, False, False, False, True] and counts.tolist() == [4, 1, 4, 0]
    want = (-4.0 * float(-r) + 4.0 * float(r)) / np.sqrt(32.0)
    assert agree[0] == np.float32(want) and agree[1] == np.float32(-want) and agree[2] == 0.0 and abs(float(agree[0]) - 1.0) < 1e-7
    assert agree[7] == np.float32(4.0 / np.sqrt(32.0)) and (agree[~pair].view(np.uint32) == 0x7FC00000).all()
    st, hist = nk.agree_stats(agree, pair, np.zeros(8, bool), 0.25, 4)               # |s| of the two aligned pairs rounds to 1 or just below it
    assert st["n_with_face"] == 4 and st["n_no_face"] == 4 and st["n_not_finite"] == 0 and hist[:3].tolist() == [1, 0, 1] and hist[3] + st["n_overflow"] == 2
    assert st["sum_dist"] == float(agree[0]) + float(agree[0]) + float(agree[7])
    # cloud direction: points above the square, one beyond max_dist, one without a normal, one that is not finite
    cloud = np.array([[1, 0.5, 1.25], [0.5, 1.5, 0.25], [1, 1, 9], [1, 1, 1.1], [np.nan, 0, 0]], np.float32)
    normal = np.array([[-r, 0, r], [r, 0, -r], [0, 0, 1], [np.nan] * 3, [np.nan] * 3], np.float32)
    status = np.array([0, 0, 0, 3, 2], np.uint8)
    agree, face, pair, counts = nk.agree_cloud(cloud, normal, status, 1.0, vtx, faces)
    assert face.tolist() == [0, 1, -1, -1, -1] and pair.tolist() == [True, True, False, False, False] and counts.tolist() == [2, 1, 2, 1]
    assert agree[0] == np.float32(want) and agree[1] == np.float32(-want)
    st, _ = nk.agree_stats(agree, pair, status == 2, 0.5, 2)
    assert (st["n_with_face"], st["n_no_face"], st["n_not_finite"]) == (2, 2, 1)
