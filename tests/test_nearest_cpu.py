"""CPU tier of the mesh-to-cloud distances (include/immesh_nearest.h): the header as plain C99, the library's new symbols, the reuse of
immesh_closest_stats, known answers of the hash, and the brute-force checker (tests/nearest_checker.py) against closed forms, on the property that
makes pruning exact (L of a point's own box is D bit for bit; L is monotone under containment), and the sampler's counting, folding and uniformity."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import nearest_checker as nc
from immesh_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "immesh_nearest.h")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(capi.hip_library_path()):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "immesh_amd", "csrc"), "-j8"])
    return capi.load_hip_library()


def _code():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


# ---- the boundary ----------------------------------------------------------------------------------------------------------------------------
def test_header_is_plain_c99(tmp_path):
    body = ('int main(void) { immesh_cloud_index* x = 0; struct immesh_closest_stats* s = 0; '
            'return (x != 0) + (s != 0) + IMMESH_RAY_NEAREST; }\n')
    full = ('int main(void) { immesh_closest_stats s; immesh_cloud_index* x = 0; s.n_points = 0; '
            'return (int)s.n_points + (x != 0) + immesh_nearest_reduce(x, 1.0, 1, &s, 0); }\n')
    # alone, and with the header that defines the statistics struct before and after it
    for k, text in enumerate(('#include "immesh_nearest.h"\n' + body, '#include "immesh_closest.h"\n#include "immesh_nearest.h"\n' + full,
                              '#include "immesh_nearest.h"\n#include "immesh_closest.h"\n' + full)):
        src = tmp_path / ("unit%d.c" % k)
        src.write_text(text)
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-c", "-I", os.path.join(ROOT, "include"), str(src),
                               "-o", str(tmp_path / ("unit%d.o" % k))])


def test_no_header_includes_it():
    for name in os.listdir(os.path.join(ROOT, "include")):
        if name != "immesh_nearest.h":
            assert "immesh_nearest.h" not in open(os.path.join(ROOT, "include", name)).read(), name
    # the header of the closest-face queries forbids every other header to name it (tests/test_closest_cpu.py), so this one cannot include it: it
    # includes the ray caster's header and names the statistics struct by its tag
    text = open(HEADER).read()
    assert '#include "immesh_raycast.h"' in text and "struct immesh_closest_stats;" in text and "immesh_closest.h" not in text


def test_library_exports_every_declared_symbol(lib):
    fns = sorted(set(re.findall(r"\b(immesh_[a-z_0-9]+)\s*\(", _code())))
    for must in ("immesh_cloud_index_create", "immesh_cloud_index_destroy", "immesh_cloud_index_build", "immesh_cloud_index_sizes", "immesh_mesh_sample",
                 "immesh_nearest_points", "immesh_nearest_samples", "immesh_nearest_reduce", "immesh_nearest_last_timing"):
        assert must in fns
    missing = [f for f in fns if not hasattr(lib, f)]
    assert not missing, missing


def test_closest_stats_is_reused():
    """no struct layout of its own: the header defines no struct body, and the reduction takes immesh_closest_stats"""
    code = _code()
    assert "{" not in code.replace('extern "C" {', "") and "typedef struct immesh_cloud_index immesh_cloud_index;" in code
    assert re.search(r"immesh_nearest_reduce\([^)]*struct immesh_closest_stats\* stats", code)
    assert "with a neighbour" in open(HEADER).read()
    assert {n for n, _ in capi.ClosestStats._fields_} >= {"n_with_face", "n_no_face", "n_not_finite"}


# ---- the hash ----------------------------------------------------------------------------------------------------------------------------------
def test_mix_is_splitmix64():
    """splitmix64 seeded with 0 adds G to its state and mixes it: its published first outputs"""
    want = [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F, 0xF88BB8A8724C81EC]
    assert [nc.mix(nc.G * (i + 1)) for i in range(4)] == want
    assert nc.face_hash(0, 0) == want[0] and nc.face_hash(0, 3) == want[3]
    assert nc.mix(0) == 0 and nc.mix(1 << 64) == 0                                   # arithmetic mod 2^64


def test_unit_interval_ends():
    assert nc.U(0) == 0.0
    assert nc.U(2 ** 64 - 1) == 1.0 - 2.0 ** -53 < 1.0
    assert nc.U(1 << 11) == 2.0 ** -53 and nc.U((1 << 11) - 1) == 0.0


# ---- closed forms ------------------------------------------------------------------------------------------------------------------------------
def test_equidistant_query_takes_the_smaller_index():
    cloud = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, 0, -1], [5, 5, 5]], np.float32)
    D, dist, index, xyz = nc.nearest(None, None, np.zeros((1, 3), np.float32), 10.0, cloud)
    assert (D.tolist(), dist.tolist(), index.tolist(), xyz.tolist()) == ([1.0], [1.0], [0], [[1.0, 0.0, 0.0]])
    D, _, index, xyz = nc.nearest(None, None, np.zeros((1, 3), np.float32), 10.0, cloud[::-1])
    assert D.tolist() == [1.0] and index.tolist() == [1] and xyz.tolist() == [[0.0, 0.0, -1.0]]
    # a frame: the same cloud seen from a sensor at (1, 2, 3) turned a quarter about z
    rot, pos = np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]]), np.array([1.0, 2, 3])
    local = ((np.zeros((1, 3)) - pos) @ rot).astype(np.float32)
    assert nc.nearest(rot, pos, local, 10.0, cloud)[2].tolist() == [0]


def test_max_dist_boundary():
    cloud = np.array([[0, 0, 2]], np.float32)
    q = np.zeros((1, 3), np.float32)
    D, dist, index, xyz = nc.nearest(None, None, q, 2.0, cloud)
    assert (D.tolist(), dist.tolist(), index.tolist()) == ([4.0], [2.0], [0])                  # D == r2 counts
    up = np.nextafter(2.0, 3.0)
    assert up * up > 4.0
    D, dist, index, xyz = nc.nearest(np.eye(3), np.array([0.0, 0.0, 2.0 - up]), q, 2.0, cloud)   # the next double above: the frame lowers the query by one unit in the last place of 2
    assert (D.tolist(), dist.tolist(), index.tolist()) == ([-1.0], [-1.0], [-1])
    assert np.array_equal(xyz.view(np.uint32), np.full((1, 3), 0x7FC00000, np.uint32))
    far = np.nextafter(np.float32(2.0), np.float32(3.0))
    assert nc.nearest(None, None, q, 2.0, np.array([[0, 0, far]], np.float32))[2].tolist() == [-1]


def test_a_cloud_point_that_is_not_finite_never_wins():
    cloud = np.array([[np.nan, 0, 0], [0, np.inf, 0], [3, 0, 0], [0, 0, -np.inf]], np.float32)
    q = np.array([[0, 0, 0], [2.9, 0, 0], [np.nan, 0, 0], [0, np.inf, 0]], np.float32)
    D, dist, index, xyz = nc.nearest(None, None, q, 100.0, cloud)
    assert index.tolist() == [2, 2, -1, -1] and D[:2].tolist() == [9.0, float((3.0 - np.float64(np.float32(2.9))) ** 2)]
    assert nc.nearest(None, None, q, 100.0, cloud[[0, 1, 3]])[2].tolist() == [-1] * 4
    assert nc.nearest(None, None, q, 100.0, np.zeros((0, 3), np.float32))[2].tolist() == [-1] * 4
    st, _ = nc.stats(None, None, q, dist, index, 1.0, 4)
    assert (st["n_points"], st["n_with_face"], st["n_not_finite"], st["n_no_face"]) == (4, 2, 2, 0)
    assert nc.points(np.eye(3) * 2.0 ** 100, np.zeros(3), np.array([[2.0 ** 30, 0, 0]], np.float32))[1].tolist() == [False]


# ---- what makes pruning exact --------------------------------------------------------------------------------------------------------------------
def test_own_box_bound_is_the_distance_bit_for_bit():
    rng = np.random.default_rng(1)
    n = 10000
    scale = 10.0 ** rng.uniform(-6, 6, (n, 1))
    c = (rng.uniform(-1, 1, (n, 3)) * scale).astype(np.float32)
    p = np.where(rng.random((n, 1)) < 0.3, c.astype(np.float64) + rng.normal(size=(n, 3)) * scale * 1e-9, rng.uniform(-2, 2, (n, 3)) * scale)
    p[:100] = c[:100]                                                                # the query on the point
    D = nc.distance2(p, c)
    L = nc.box_bound(p, c.astype(np.float64), c.astype(np.float64))
    assert D.tobytes() == L.tobytes() and (D[:100] == 0).all() and (D > 0).sum() > n // 2


def test_box_bound_is_monotone_under_containment():
    """a box that contains the point's own box never has the larger L: D >= L(every enclosing box), exactly"""
    rng = np.random.default_rng(2)
    n = 100000
    scale = 10.0 ** rng.uniform(-3, 3, (n, 1))
    c = (rng.uniform(-1, 1, (n, 3)) * scale).astype(np.float32)
    grow = np.abs(rng.normal(size=(2, n, 3)) * scale * 10.0 ** rng.uniform(-8, 0, (n, 1))).astype(np.float32)
    grow[:, rng.random(n) < 0.2] = 0
    lo, hi = (c - grow[0]).astype(np.float32), (c + grow[1]).astype(np.float32)
    assert (lo <= c).all() and (hi >= c).all()
    p = np.where(rng.random((n, 1)) < 0.3, lo.astype(np.float64) - 1e-9 * scale * rng.random((n, 3)), rng.uniform(-3, 3, (n, 3)) * scale)
    D = nc.distance2(p, c)
    outer = nc.box_bound(p, lo.astype(np.float64), hi.astype(np.float64))
    assert (outer <= D).all() and (outer < D).sum() > n // 4 and (outer > 0).sum() > n // 4


# ---- the sampler ---------------------------------------------------------------------------------------------------------------------------------
RIGHT = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)                          # area 1 / 2


def test_an_integer_x_gives_exactly_x_samples():
    for density, want in ((2.0, 1), (16.0, 8), (600.0, 300)):
        for seed in (0, 1, 2 ** 64 - 1):
            assert nc.face_x(RIGHT, [0, 1, 2], density) == float(want)
            assert nc.counts(RIGHT, [[0, 1, 2]], density, seed) == [want]
            xyz, face = nc.sample(RIGHT, [[0, 1, 2]], density, seed)
            assert len(xyz) == want and face.tolist() == [0] * want
    # a fraction rounds either way, by the face's own hash
    ks = {nc.counts(RIGHT, [[0, 1, 2]], 3.0, seed)[0] for seed in range(40)}
    assert ks == {1, 2}


def test_faces_without_area_or_not_finite_give_none():
    vtx = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 0, 0], [np.nan, 0, 0], [0, np.inf, 0]], np.float32)
    faces = [[0, 0, 1], [0, 1, 3], [1, 1, 1], [0, 1, 4], [5, 1, 2], [0, 1, 6], [-1, 1, 2], [0, 1, 2]]
    for density in (0.5, 1e3, 1e30):
        k = nc.counts(vtx, faces, density, 7)
        assert k[:7] == [0] * 7, (density, k)
    assert nc.counts(vtx, faces, 1e3, 7)[7] == 500
    xyz, face = nc.sample(vtx, faces, 1e3, 7)
    assert len(xyz) == 500 and set(face.tolist()) == {7}


def test_saturation_leads_to_the_capacity_error():
    big = (RIGHT * np.float32(1e6)).astype(np.float32)
    assert nc.counts(big, [[0, 1, 2]], 1.0, 0) == [2 ** 31]                          # x = 5e11 >= 2^31
    assert nc.counts(big, [[0, 1, 2]], 1e300, 0) == [2 ** 31]                        # x is not finite
    with pytest.raises(nc.TooManySamples):
        nc.sample(big, [[0, 1, 2]], 1.0, 0)
    # below saturation, above the total's bound: 2^31 - 2 is the last total that passes
    x_ok = float(nc.MAX_SAMPLES)
    assert nc.face_count(x_ok, 0, 0) == nc.MAX_SAMPLES and nc.face_count(x_ok + 1.0, 0, 0) == nc.MAX_SAMPLES + 1
    assert nc.face_count(2.0 ** 31 - 0.5, 0, 0) in (2 ** 31 - 1, 2 ** 31) and nc.face_count(2.0 ** 31, 0, 0) == 2 ** 31


def test_fold_keeps_the_pair_inside_the_triangle():
    worst, folded = 0.0, 0
    for f in range(50):
        hf = nc.face_hash(11, f)
        for j in range(400):
            u0, v0 = nc.U(nc.mix((hf + nc.G * (2 * j + 1)) & nc.MASK)), nc.U(nc.mix((hf + nc.G * (2 * j + 2)) & nc.MASK))
            u, v = nc.uv(hf, j)
            assert 0.0 <= u <= 1.0 and 0.0 <= v <= 1.0 and u + v <= 1.0
            if u0 + v0 > 1.0:
                folded += 1
                assert (u, v) == (1.0 - u0, 1.0 - v0) and 1.0 - u == u0 and 1.0 - v == v0     # both differences are exact
            worst = max(worst, u + v)
    assert folded > 8000 and worst > 0.999
    # the extreme pair: u = v = 1 - 2^-53 folds to 2^-53 each
    top = 1.0 - 2.0 ** -53
    assert (1.0 - top) + (1.0 - top) <= 1.0


def test_samples_are_uniform_on_a_right_triangle():
    """density 10^5 per unit area on the triangle of area 1 / 2: x = 50 000 exactly, so the count is x; the share of each of the four mid-point
    sub-triangles (equal areas) is binomial(n, 1 / 4): within 5 standard deviations sqrt(3 / (16 n)) of 1 / 4"""
    density = 1e5
    x = nc.face_x(RIGHT, [0, 1, 2], density)
    xyz, _ = nc.sample(RIGHT, [[0, 1, 2]], density, 2024)
    n = len(xyz)
    assert abs(n - x) <= 1 and x == 50000.0
    a, b = xyz[:, 0].astype(np.float64), xyz[:, 1].astype(np.float64)
    assert (xyz[:, 2] == 0).all() and (a >= 0).all() and (b >= 0).all() and (a + b <= 1.0 + 2.0 ** -23).all()
    share = [np.mean(a > 0.5), np.mean(b > 0.5), np.mean((a + b) < 0.5), np.mean((a <= 0.5) & (b <= 0.5) & ((a + b) >= 0.5))]
    sigma = math.sqrt(0.25 * 0.75 / n)
    print("shares", share, "5 sigma", 5 * sigma)
    assert abs(sum(share) - 1.0) < 1e-12
    for s in share:
        assert abs(s - 0.25) <= 5 * sigma, (share, sigma)


def test_vectorised_x_equals_the_plain_one():
    rng = np.random.default_rng(3)
    vtx = np.concatenate([rng.normal(scale=3.0, size=(60, 3)), [[np.nan, 0, 0], [0, -np.inf, 0]]]).astype(np.float32)
    faces = rng.integers(-2, 66, (500, 3))
    x, live = nc.faces_x(vtx, faces, 7.5)
    plain = [nc.face_x(vtx, f, 7.5) for f in faces]
    assert [None if not l else float(v) for v, l in zip(x, live)] == plain and 100 < live.sum() < 480


# ---- tools/mesh_eval.py ----------------------------------------------------------------------------------------------------------------------------
def test_mesh_eval_reads_the_ply_layout_of_save_ply(tmp_path):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import mesh_eval
    vtx = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [np.nan, 2, 3]], np.float32)
    faces = np.array([[0, 1, 2], [2, 1, 3]], np.int32)
    head = ("ply\nformat binary_little_endian 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\nelement face 2\n"
            "property list uchar int vertex_indices\nend_header\n").encode()
    body = vtx.tobytes() + b"".join(b"\x03" + f.tobytes() for f in faces)
    path = tmp_path / "m.ply"
    path.write_bytes(head + body)
    v, f = mesh_eval.read_ply(str(path))
    assert v.tobytes() == vtx.tobytes() and np.array_equal(f, faces) and f.dtype == np.int32
    path.write_bytes(head.replace(b"binary_little_endian", b"ascii") + body)
    with pytest.raises(ValueError):
        mesh_eval.read_ply(str(path))
