"""CPU tier of the k nearest neighbours, radius counts and outlier rules (include/immesh_nearest.h): the extended header is still plain C99 in its
three arrangements and defines no struct body, the library exports every declared symbol, and the brute-force checker (tests/knn_checker.py)
against closed forms: ties across the k-th slot, coincident points, the distance boundary, the statistics' corner cases, planted strays, and the
KD-tree-assisted path of the scale test against the chunked brute force."""
import os
import re
import subprocess

import numpy as np
import pytest

import knn_checker as kc
from immesh_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "immesh_nearest.h")
NEW = ("immesh_knn_points", "immesh_knn_cloud", "immesh_radius_count_points", "immesh_radius_count_cloud", "immesh_cloud_outliers_statistical",
       "immesh_cloud_outliers_radius", "immesh_cloud_index_apply_outliers", "immesh_cloud_index_points", "immesh_knn_last_timing")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(capi.hip_library_path()):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "immesh_amd", "csrc"), "-j8"])
    return capi.load_hip_library()


def _code():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


# ---- the boundary ----------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_new_entry_points_in_plain_c99(tmp_path):
    code = _code()
    fns = set(re.findall(r"\b(immesh_[a-z_0-9]+)\s*\(", code))
    assert set(NEW) <= fns, sorted(set(NEW) - fns)
    assert "{" not in code.replace('extern "C" {', "")                               # still no struct body: results go out through plain pointers
    for rule in ("The Neighbours rule", "the Count rule", "the Outliers rule"):
        assert rule in open(HEADER).read(), rule
    body = ('int main(void) { immesh_cloud_index* x = 0; int32_t c[2]; int64_t n[4]; double m[3]; float ms[3]; uint8_t keep[2];\n'
            '  return immesh_knn_points(x, 0, 0, 0, 3, 1.0, c, 0, 0) + immesh_knn_cloud(x, 3, 1.0, c, 0, 0, m) + immesh_radius_count_points(x, 0, 0, 0, 1.0, c)\n'
            '    + immesh_radius_count_cloud(x, 1.0, c) + immesh_cloud_outliers_statistical(x, 2.0, m, m + 1, m + 2, n, keep)\n'
            '    + immesh_cloud_outliers_radius(x, 2, n, keep) + immesh_cloud_index_apply_outliers(x, c, 2, n) + immesh_cloud_index_points(x, ms, 1, n)\n'
            '    + immesh_knn_last_timing(x, ms); }\n')
    for k, text in enumerate(('#include "immesh_nearest.h"\n' + body, '#include "immesh_closest.h"\n#include "immesh_nearest.h"\n' + body,
                              '#include "immesh_nearest.h"\n#include "immesh_closest.h"\n' + body)):
        src = tmp_path / ("unit%d.c" % k)
        src.write_text(text)
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-c", "-I", os.path.join(ROOT, "include"), str(src),
                               "-o", str(tmp_path / ("unit%d.o" % k))])


def test_library_exports_the_new_symbols(lib):
    missing = [f for f in NEW if not hasattr(lib, f)]
    assert not missing, missing


# ---- closed forms ------------------------------------------------------------------------------------------------------------------------------
def _lattice(m=3):
    g = np.arange(m, dtype=np.float32)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)


def test_cell_centre_takes_the_three_smallest_indices():
    """the centre of a lattice cell has eight equidistant corners: k = 3 gives the three smallest indices, whatever the rows' order"""
    cloud = _lattice()
    q = np.array([[0.5, 0.5, 0.5]], np.float32)
    corners = [i for i, c in enumerate(cloud) if (c <= 1).all()]
    assert len(corners) == 8
    count, index, d2 = kc.knn(None, None, q, 3, 10.0, cloud)
    assert count.tolist() == [3] and index.tolist() == [sorted(corners)[:3]] and d2.tolist() == [[0.75] * 3]
    perm = np.random.default_rng(0).permutation(len(cloud))
    count, index, d2 = kc.knn(None, None, q, 3, 10.0, cloud[perm])
    want = sorted(int(np.nonzero(perm == c)[0][0]) for c in corners)[:3]
    assert index.tolist() == [want] and d2.tolist() == [[0.75] * 3]
    # k = 9 straddles the tie: the eight corners by index, then the nearest of the next shell (D = 0.5^2 + 0.5^2 + 1.5^2 = 2.75), by index again
    count, index, d2 = kc.knn(None, None, q, 9, 10.0, cloud)
    assert count.tolist() == [9] and index[0, :8].tolist() == sorted(corners) and d2[0, 8] == 2.75
    shell = [i for i, c in enumerate(cloud) if kc.exact_d(q.astype(np.float64), c[None, None])[0, 0] == 2.75]
    assert index[0, 8] == min(shell) and len(shell) == 12                            # corners of the cell with one coordinate moved to 2: 3 axes x 4


def test_coincident_points_in_cloud_mode():
    cloud = np.tile(np.array([[1.5, -2.0, 3.0]], np.float32), (5, 1))
    count, index, d2, mean = kc.knn_cloud(cloud, 3, 1.0)
    assert count.tolist() == [3] * 5 and (d2 == 0.0).all() and mean.tolist() == [0.0] * 5
    assert index.tolist() == [[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2], [0, 1, 2]]  # the others at D = 0 by index, never the point's own
    count, index, d2, mean = kc.knn_cloud(cloud[:3], 3, 1.0)                         # two others only: a partial list
    assert count.tolist() == [2] * 3 and index.tolist() == [[1, 2, -1], [0, 2, -1], [0, 1, -1]] and d2[:, 2].tolist() == [-1.0] * 3
    assert kc.radius_count_cloud(cloud, 1e-3).tolist() == [4] * 5
    assert kc.radius_count(None, None, cloud[:1], 1e-3, cloud).tolist() == [5]        # point mode: the coincident query counts every copy


def test_distance_boundary():
    cloud = np.array([[0, 0, 2], [0, 0, -3]], np.float32)
    q = np.zeros((1, 3), np.float32)
    count, index, d2 = kc.knn(None, None, q, 2, 2.0, cloud)
    assert count.tolist() == [1] and index.tolist() == [[0, -1]] and d2.tolist() == [[4.0, -1.0]]            # D == r2 counts
    assert kc.radius_count(None, None, q, 2.0, cloud).tolist() == [1] and kc.radius_count(None, None, q, 3.0, cloud).tolist() == [2]
    up = np.nextafter(2.0, 3.0)
    pos = np.array([0.0, 0.0, 2.0 - up])                                              # the frame lowers the query by one unit in the last place of 2
    assert kc.knn(np.eye(3), pos, q, 2, 2.0, cloud)[0].tolist() == [0]
    assert kc.radius_count(np.eye(3), pos, q, 2.0, cloud).tolist() == [0]
    far = np.nextafter(np.float32(2.0), np.float32(3.0))
    assert kc.radius_count(None, None, q, 2.0, np.array([[0, 0, far]], np.float32)).tolist() == [0]
    # queries and cloud points that are not finite
    bad = np.array([[np.nan, 0, 0], [0, 0, 1], [np.inf, 0, 0]], np.float32)
    count, index, d2, mean = kc.knn_cloud(bad, 2, 10.0)
    assert count.tolist() == [0, 0, 0] and mean.tolist() == [-1.0] * 3 and (index == -1).all()
    assert kc.knn(None, None, bad, 1, 10.0, cloud)[0].tolist() == [0, 1, 0]


def test_mean_is_the_sequential_sum():
    cloud = np.array([[0, 0, 0], [3, 0, 0], [0, 4, 0], [0, 0, 12]], np.float32)
    count, index, d2, mean = kc.knn_cloud(cloud, 3, 100.0)
    assert index[0].tolist() == [1, 2, 3] and d2[0].tolist() == [9.0, 16.0, 144.0] and mean[0] == ((3.0 + 4.0) + 12.0) / 3.0
    count, index, d2, mean = kc.knn_cloud(cloud, 3, 4.5)                              # the far point sees nobody
    assert count.tolist() == [2, 1, 1, 0] and mean.tolist() == [3.5, 3.0, 4.0, -1.0]


def test_statistics_corner_cases():
    fin = np.ones(3, bool)
    out = kc.statistical(np.array([-1.0, -1.0, -1.0]), np.zeros(3, int), fin, 1.0)    # n_used == 0
    assert (out["mu"], out["sigma"], out["threshold"], out["kept"], out["isolated"]) == (0.0, 0.0, 0.0, 0, 3) and not out["keep"].any()
    out = kc.statistical(np.array([-1.0, 2.5, -1.0]), np.array([0, 4, 0]), fin, 3.0)  # n_used == 1: sigma = 0, the one point is kept
    assert (out["mu"], out["sigma"], out["threshold"]) == (2.5, 0.0, 2.5) and out["keep"].tolist() == [False, True, False]
    mean, count = np.array([1.0, 2.0, 3.0, 6.0]), np.ones(4, int)
    out = kc.statistical(mean, count, np.ones(4, bool), 0.0)                          # mult == 0: the threshold is the mean
    assert out["mu"] == 3.0 and out["threshold"] == 3.0 and out["keep"].tolist() == [True, True, True, False]
    assert out["sigma"] == np.sqrt(((4.0 + 1.0) + 0.0 + 9.0) / 3.0)
    assert (out["kept"], out["outliers"], out["isolated"], out["not_finite"]) == (3, 1, 0, 0)


def sheet_with_strays(seed=5, n_sheet=2000, n_stray=20, n_nan=3, n_far=5):
    """a jittered sheet z ~ 0 over [0, 10]^2, strays 1 - 3 above it, points that are not finite and points far from everything, rows shuffled
    -> cloud (n, 3) float32, kind (n,): 0 sheet, 1 stray, 2 not finite, 3 far"""
    rng = np.random.default_rng(seed)
    sheet = np.concatenate([rng.uniform(0, 10, (n_sheet, 2)), rng.normal(scale=0.01, size=(n_sheet, 1))], axis=1)
    stray = np.concatenate([rng.uniform(1, 9, (n_stray, 2)), rng.uniform(1.0, 3.0, (n_stray, 1))], axis=1)
    nan = rng.uniform(0, 10, (n_nan, 3))
    nan[np.arange(n_nan), np.arange(n_nan) % 3] = [np.nan, np.inf, -np.inf][:n_nan]
    far = 1000.0 * (2 + np.arange(n_far))[:, None] * np.array([[1.0, -1.0, 1.0]])
    cloud = np.concatenate([sheet, stray, nan, far]).astype(np.float32)
    kind = np.repeat([0, 1, 2, 3], [n_sheet, n_stray, n_nan, n_far])
    perm = rng.permutation(len(cloud))
    return cloud[perm], kind[perm]


def test_masks_find_the_planted_strays():
    cloud = np.array([[x, y, 0] for x in range(6) for y in range(6)] + [[2.5, 2.5, 4.0], [0, 0, -5.0], [5, 5, 6.0]], np.float32)
    fin = np.isfinite(cloud).all(axis=1)
    count, _, _, mean = kc.knn_cloud(cloud, 4, 100.0)
    out = kc.statistical(mean, count, fin, 2.0)
    assert out["keep"].tolist() == [True] * 36 + [False] * 3 and (out["kept"], out["outliers"], out["isolated"]) == (36, 3, 0)
    rc = kc.radius_count_cloud(cloud, 1.5)
    assert rc[-3:].tolist() == [0, 0, 0] and rc[:36].min() == 3 and rc[:36].max() == 8
    out = kc.radius_rule(rc, fin, 3)
    assert out["keep"].tolist() == [True] * 36 + [False] * 3 and (out["kept"], out["outliers"], out["isolated"], out["not_finite"]) == (36, 3, 3, 0)
    assert kc.radius_rule(rc, fin, 0)["kept"] == 39 and kc.radius_rule(rc, fin, 4)["kept"] == 32      # the four corners have three
    # the larger fixture the device test uses: every stray and every far point goes, nearly all of the sheet stays
    cloud, kind = sheet_with_strays()
    fin = np.isfinite(cloud).all(axis=1)
    count, _, _, mean = kc.knn_cloud(cloud, 8, 5.0)
    out = kc.statistical(mean, count, fin, 3.0)
    assert not out["keep"][kind != 0].any() and out["keep"][kind == 0].mean() > 0.97
    assert (out["isolated"], out["not_finite"]) == (5, 3) and out["kept"] + out["outliers"] + 8 == len(cloud)


# ---- the scale test's path ------------------------------------------------------------------------------------------------------------------------
def test_tree_assisted_path_equals_the_brute_force():
    rng = np.random.default_rng(11)
    cloud = rng.uniform(-5, 5, (2000, 3)).astype(np.float32)
    cloud[100:110] = cloud[90:100]                                                   # coincident pairs: exact ties at D = 0 in cloud mode
    cloud[7, 1] = np.nan
    cloud[:60] = np.round(cloud[:60])                                                # a few lattice points: ties for lattice queries
    q = np.concatenate([rng.uniform(-5, 5, (500, 3)), np.round(rng.uniform(-5, 5, (100, 3))) + 0.5]).astype(np.float32)
    q[3, 0] = np.inf
    for k, max_dist in ((1, 0.5), (16, 1.0), (16, 100.0), (64, 1.5)):
        a, b = kc.knn(None, None, q, k, max_dist, cloud), kc.knn_tree(q, k, max_dist, cloud)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)), (k, max_dist)
        if max_dist == 100.0:
            assert (np.delete(a[0], 3) == k).all() and a[0][3] == 0                  # full lists, but for the query that is not finite
    skip = np.arange(len(cloud))
    a, b = kc.knn(None, None, cloud, 16, 1.0, cloud, skip=skip), kc.knn_tree(cloud, 16, 1.0, cloud, skip=skip)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)) and (a[2][100:110, 0] == 0.0).all()
    for radius in (0.3, 1.0):
        assert np.array_equal(kc.radius_count(None, None, q, radius, cloud), kc.radius_count_tree(q, radius, cloud))
        assert np.array_equal(kc.radius_count_cloud(cloud, radius), kc.radius_count_tree(cloud, radius, cloud, skip=skip))
