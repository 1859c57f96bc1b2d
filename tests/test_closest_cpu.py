"""CPU tier of the closest-point queries (include/immesh_closest.h): the header as plain C99, the library's new symbols, immesh_closest_stats'
layout, and the brute-force checker (tests/closest_checker.py) against closed forms, on faces of zero area, on the two properties that make pruning
exact (L is monotone under box containment, D >= L of the face's own box), against a dense sampling of the face in long double (and a
least-squares projection where scipy is installed), and its histogram rule against a plain loop."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import closest_checker as cc
from immesh_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "immesh_closest.h")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(capi.hip_library_path()):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "immesh_amd", "csrc"), "-j8"])
    return capi.load_hip_library()


# ---- the boundary ----------------------------------------------------------------------------------------------------------------------------
def test_header_is_plain_c99(tmp_path):
    src = tmp_path / "alone.c"
    src.write_text('#include "immesh_closest.h"\nint main(void) { immesh_closest_stats s; s.n_points = 0; return (int)s.n_points + IMMESH_RAY_NEAREST; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "alone.o")])


def test_no_header_includes_it():
    for name in os.listdir(os.path.join(ROOT, "include")):
        if name != "immesh_closest.h":
            assert "immesh_closest.h" not in open(os.path.join(ROOT, "include", name)).read(), name
    assert '#include "immesh_raycast.h"' in open(HEADER).read()


def test_library_exports_every_declared_symbol(lib):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    fns = sorted(set(re.findall(r"\b(immesh_[a-z_0-9]+)\s*\(", src)))
    for must in ("immesh_closest_points", "immesh_closest_reduce", "immesh_closest_last_timing"):
        assert must in fns
    missing = [f for f in fns if not hasattr(lib, f)]
    assert not missing, missing


def test_stats_layout(tmp_path):
    names = [n for n, _ in capi.ClosestStats._fields_]
    prog = tmp_path / "layout.c"
    prog.write_text('#include "immesh_closest.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void) {\n  printf("%zu", sizeof(immesh_closest_stats));\n'
                    + "".join('  printf(" %%zu", offsetof(immesh_closest_stats, %s));\n' % n for n in names) + "  return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(prog), "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe]).split()]
    assert got == [C.sizeof(capi.ClosestStats)] + [getattr(capi.ClosestStats, n).offset for n in names]
    assert got == [80, 0, 8, 16, 24, 32, 40, 48, 56, 64, 72, 76]
    declared = re.findall(r"(\w+)(?:, (\w+))?;", re.search(r"typedef struct immesh_closest_stats \{(.*?)\}", re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S), re.S).group(1))
    assert [n for pair in declared for n in pair if n] == names


# ---- closed forms ----------------------------------------------------------------------------------------------------------------------------
TRI = np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0]], np.float32)           # a right triangle in z = 0, counter-clockwise seen from +z
# (x, y) of the query, the closest point, the squared distance in the plane, the region of the contract's Face rule
REGIONS = [((-1, -1), (0, 0), 2.0, 1), ((6, -1), (4, 0), 5.0, 2), ((2, -1), (2, 0), 1.0, 3), ((-1, 6), (0, 4), 5.0, 4), ((-1, 2), (0, 2), 1.0, 5),
           ((3, 3), (2, 2), 2.0, 6), ((1, 1), (1, 1), 0.0, 7)]


@pytest.mark.parametrize("height", [0.5, -0.5, 0.0, 8.0, -0.0078125])
def test_seven_regions_of_a_right_triangle(height):
    pts = np.array([[x, y, height] for (x, y), _, _, _ in REGIONS], np.float32)
    D, dist, face, xyz, side = cc.closest(None, None, pts, 100.0, TRI, [[0, 1, 2]])
    assert face.tolist() == [0] * 7
    assert D.tolist() == [d + height * height for _, _, d, _ in REGIONS]
    assert xyz.tolist() == [[qx, qy, 0.0] for _, (qx, qy), _, _ in REGIONS]
    assert side.tolist() == [int(np.sign(height))] * 7
    assert np.array_equal(dist, np.sqrt(D).astype(np.float32))
    p, _ = cc.points(None, None, pts)
    t = TRI.astype(np.float64)
    assert cc.face_q(t[0] - p, t[1] - p, t[2] - p)[2].tolist() == [r for _, _, _, r in REGIONS]
    # the other vertex order: the same points, the other side
    assert cc.closest(None, None, pts, 100.0, TRI, [[0, 2, 1]])[4].tolist() == [-int(np.sign(height))] * 7
    # a frame: the triangle seen from a sensor at (1, 2, 3) turned a quarter about z gives the same world answers
    rot, pos = np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]]), np.array([1.0, 2, 3])
    local = ((pts.astype(np.float64) - pos) @ rot).astype(np.float32)
    D2, _, _, xyz2, side2 = cc.closest(rot, pos, local, 100.0, TRI, [[0, 1, 2]])
    assert np.array_equal(D2, D) and np.array_equal(xyz2, xyz) and np.array_equal(side2, side)


def test_max_dist_and_points_that_are_not_finite():
    pts = np.array([[1, 1, 2], [1, 1, np.nan], [np.inf, 0, 0], [1, 1, 2.0000002]], np.float32)
    D, dist, face, xyz, side = cc.closest(None, None, pts, 2.0, TRI, [[0, 1, 2]])
    assert face.tolist() == [0, -1, -1, -1] and D.tolist() == [4.0, -1.0, -1.0, -1.0] and dist.tolist() == [2.0, -1.0, -1.0, -1.0]
    assert np.isnan(xyz[1:]).all() and side.tolist() == [1, 0, 0, 0]
    assert np.array_equal(xyz[1:].view(np.uint32), np.full((3, 3), 0x7FC00000, np.uint32))
    st, _ = cc.stats(None, None, pts, dist, face, 1.0, 4)
    assert (st["n_points"], st["n_with_face"], st["n_not_finite"], st["n_no_face"]) == (4, 1, 2, 1)
    # a frame that carries a point beyond 2^128: not finite by rule
    assert cc.points(np.eye(3) * 2.0 ** 100, np.zeros(3), np.array([[2.0 ** 30, 0, 0]], np.float32))[1].tolist() == [False]
    assert cc.points(np.eye(3) * 2.0 ** 97, np.zeros(3), np.array([[2.0 ** 30, 0, 0]], np.float32))[1].tolist() == [True]
    # a face with a vertex that is not finite never counts; an empty soup answers -1
    bad = np.concatenate([TRI, [[np.nan, 0, 0]]]).astype(np.float32)
    assert cc.closest(None, None, pts[:1], 5.0, bad, [[0, 1, 3], [0, 1, 2]])[2].tolist() == [1]
    assert cc.closest(None, None, pts[:1], 5.0, bad, [[0, 1, 3]])[2].tolist() == [-1]
    assert cc.closest(None, None, pts[:1], 5.0, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))[2].tolist() == [-1]


def _segment_distance(q, a, c):
    ld = np.longdouble
    q, a, c = q.astype(ld), a.astype(ld), c.astype(ld)
    ac = c - a
    den = (ac * ac).sum(axis=-1)
    t = np.clip(((q - a) * ac).sum(axis=-1) / np.where(den > 0, den, 1), 0, 1)
    return np.sqrt((((a + t[..., None] * ac) - q) ** 2).sum(axis=-1))


def test_zero_area_faces_give_finite_points_of_the_face():
    rng = np.random.default_rng(7)
    n = 4000
    a = rng.uniform(-3, 3, (n, 3)).astype(np.float32)
    c = (a + rng.normal(size=(n, 3))).astype(np.float32)
    mid = (a + np.float32(0.25) * (c - a)).astype(np.float32)                       # (rounded: collinear up to float rounding, as a soup holds them)
    far = (a + np.float32(2.0) * (c - a)).astype(np.float32)
    pts = rng.uniform(-4, 4, (n, 3)).astype(np.float32)
    p = pts.astype(np.float64)
    shapes = {"a == b": (a, a, c, a, c), "b == c": (a, c, c, a, c), "a == c": (a, c, a, a, c), "collinear, b between": (a, mid, c, a, c),
              "collinear, c between": (a, far, c, a, far), "a == b == c": (a, a, a, a, a)}
    for name, (v0, v1, v2, e0, e1) in shapes.items():
        tri = np.stack([v0, v1, v2], axis=1)
        D, q, side, d2, L = cc.pair(p, tri)
        assert np.isfinite(q).all() and np.isfinite(D).all(), name
        off = _segment_distance(p + q, e0.astype(np.float64), e1.astype(np.float64))
        assert off.max() < 1e-6, (name, float(off.max()))                          # q is a point of the (degenerate) face: on its segment, up to the floats' rounding of mid / far
        true = _segment_distance(p, e0.astype(np.float64), e1.astype(np.float64))
        assert (np.sqrt(d2) >= true * (1 - 1e-6) - 1e-6).all(), name               # so d2 is an upper bound of the distance
        if "==" in name:
            assert (side == 0).all(), name                                         # cross(ab, ac) is exactly zero
        if name == "a == b == c":
            assert np.array_equal(q, a.astype(np.float64) - p)
        if name in ("a == b", "b == c", "a == c"):                                 # exactly a segment: the contract finds its nearest point
            assert np.abs(np.sqrt(d2) - true).max() < 1e-9, (name, float(np.abs(np.sqrt(d2) - true).max()))


# ---- what makes pruning exact ------------------------------------------------------------------------------------------------------------------
def test_box_bound_is_monotone_under_containment():
    """10^5 random nested float boxes: the enclosing box never has the larger L.  (No counter-example exists: rounding is monotone.  This pins the
    arithmetic: a rewrite of L that is not monotone, such as one with a fused multiply-add, fails here.)"""
    rng = np.random.default_rng(8)
    n = 100000
    scale = 10.0 ** rng.uniform(-3, 3, (n, 1))
    lo = (rng.uniform(-1, 1, (n, 3)) * scale).astype(np.float32)
    hi = (lo + np.abs(rng.normal(size=(n, 3)) * scale).astype(np.float32)).astype(np.float32)
    grow = np.abs(rng.normal(size=(2, n, 3)) * scale * 10.0 ** rng.uniform(-8, 0, (n, 1))).astype(np.float32)
    grow[:, rng.random(n) < 0.2] = 0                                                # equal boxes too
    lo2, hi2 = (lo - grow[0]).astype(np.float32), (hi + grow[1]).astype(np.float32)
    assert (lo2 <= lo).all() and (hi2 >= hi).all()
    p = np.where(rng.random((n, 1)) < 0.3, lo.astype(np.float64) - 1e-9 * scale * rng.random((n, 3)), rng.uniform(-3, 3, (n, 3)) * scale)   # some points graze a face of the box
    inner = cc.box_bound(p, lo.astype(np.float64), hi.astype(np.float64))
    outer = cc.box_bound(p, lo2.astype(np.float64), hi2.astype(np.float64))
    assert (outer <= inner).all()
    assert (inner > 0).sum() > n // 2 and (outer < inner).sum() > n // 4


def test_face_distance_is_never_below_its_own_box_bound():
    rng = np.random.default_rng(9)
    n = 100000
    tri = (rng.uniform(-5, 5, (n, 1, 3)) + rng.normal(scale=10.0 ** rng.uniform(-4, 0.5, (n, 1, 1)), size=(n, 3, 3))).astype(np.float32)
    near = rng.random(n) < 0.5                                                      # half the points within 1e-4 of the face: d2 and L are rounding noise apart
    w = rng.dirichlet(np.ones(3), size=n)
    on_face = (tri.astype(np.float64) * w[:, :, None]).sum(axis=1)
    p = np.where(near[:, None], on_face + rng.normal(scale=1e-4, size=(n, 3)), rng.uniform(-8, 8, (n, 3)))
    D, q, side, d2, L = cc.pair(p, tri)
    assert (D >= L).all() and (D >= d2).all() and np.array_equal(D, np.maximum(d2, L))
    print("D raised above d2 by the box bound in", int((D > d2).sum()), "of", n, "pairs; largest relative lift", float(((D - d2) / np.maximum(D, 1e-300)).max()))
    assert ((D - d2) <= 1e-12 * D).all()                                            # the lift is rounding noise: geometrically the closest point lies in the box


# ---- an independent cross-check ----------------------------------------------------------------------------------------------------------------
def test_against_a_dense_sampling_in_long_double():
    """the sampled minimum over a barycentric grid of the face is >= d2 (1 - eps) (no sample is nearer than the closest point) and its distance
    is within the grid's step (the longest edge / N) of the checker's"""
    rng = np.random.default_rng(10)
    n, N = 300, 160
    tri = (rng.uniform(-5, 5, (n, 1, 3)) + rng.normal(scale=10.0 ** rng.uniform(-1.5, 0.5, (n, 1, 1)), size=(n, 3, 3))).astype(np.float32)
    tri[:30, 2] = tri[:30, 0] + np.float32(0.01) * (tri[:30, 1] - tri[:30, 0]) + np.float32(1e-3) * tri[:30, 2]   # slivers
    p = rng.uniform(-6, 6, (n, 3))
    p[100:200] = (tri[100:200].astype(np.float64) * rng.dirichlet(np.ones(3), size=100)[:, :, None]).sum(axis=1) + rng.normal(scale=0.05, size=(100, 3))
    _, q, _, d2, _ = cc.pair(p, tri)
    ld = np.longdouble
    i, j = np.meshgrid(np.arange(N + 1), np.arange(N + 1), indexing="ij")
    keep = i + j <= N
    v, w = (i[keep] / ld(N)), (j[keep] / ld(N))
    t = tri.astype(ld) - p.astype(ld)[:, None, :]
    s = t[:, None, 0] + v[None, :, None] * (t[:, None, 1] - t[:, None, 0]) + w[None, :, None] * (t[:, None, 2] - t[:, None, 0])
    sampled = (s * s).sum(axis=-1).min(axis=1)
    edge = np.sqrt(np.max([((tri[:, a] - tri[:, b]).astype(np.float64) ** 2).sum(axis=-1) for a, b in ((0, 1), (1, 2), (2, 0))], axis=0))
    assert (sampled >= d2 * (1 - 1e-12)).all(), float((sampled / d2).min())
    assert (np.sqrt(sampled.astype(np.float64)) <= np.sqrt(d2) + edge / N).all()
    try:
        from scipy.optimize import nnls
    except ImportError:
        return
    worst = 0.0
    for k in range(n):                                                              # min |lam_a a + lam_b b + lam_c c|, lam >= 0, sum lam = 1 (a heavy row holds the sum)
        M = (tri[k].astype(np.float64) - p[k]).T
        big = 1e4 * np.abs(M).max()
        lam, _ = nnls(np.vstack([M, np.full((1, 3), big)]), np.array([0, 0, 0, big]))
        lam /= lam.sum()
        ref = np.linalg.norm(M @ lam)
        worst = max(worst, abs(ref - np.sqrt(d2[k])) / max(edge[k], np.sqrt(d2[k])))
    assert worst < 1e-6, worst


# ---- statistics --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bin_width,n_bins", [(0.1, 7), (0.25, 1), (1e-3, 1024), (3.0, 5)])
def test_histogram_rule_against_a_plain_loop(bin_width, n_bins):
    rng = np.random.default_rng(11)
    dist = np.abs(rng.normal(scale=0.4, size=3000)).astype(np.float32)
    dist[:50] = (np.arange(50) * np.float32(bin_width)).astype(np.float32)          # on the bin edges
    face = np.where(rng.random(3000) < 0.8, 5, -1)
    pts = np.zeros((3000, 3), np.float32)
    pts[np.nonzero(face < 0)[0][::3], 0] = np.nan
    st, hist = cc.stats(None, None, pts, dist, face, bin_width, n_bins)
    bw = np.float32(bin_width)
    want, over, s1, s2, mx = [0] * n_bins, 0, 0.0, 0.0, 0.0
    for d, f in zip(dist, face):
        if f < 0:
            continue
        b = np.float32(d / bw)
        if b < np.float32(n_bins):
            want[int(b)] += 1
        else:
            over += 1
        mx = max(mx, float(d))
    assert hist.tolist() == want and st["n_overflow"] == over and sum(want) + over == st["n_with_face"] == int((face >= 0).sum())
    assert st["max_dist"] == mx and st["n_not_finite"] == int(np.isnan(pts).any(axis=1).sum()) > 0
    assert st["n_no_face"] == int((face < 0).sum()) - st["n_not_finite"]
    d64 = dist[face >= 0].astype(np.float64)
    assert abs(st["sum_dist"] - d64.sum()) <= len(d64) * 2.0 ** -53 * d64.sum()
    assert st["mean"] == st["sum_dist"] / st["n_with_face"] and st["rms"] == np.sqrt(st["sum_dist2"] / st["n_with_face"])
