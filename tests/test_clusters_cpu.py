"""CPU tier of the Euclidean clusters (include/immesh_nearest.h, the Clusters rule): the extended header is still plain C99 in its arrangements and
defines no struct body, the library exports every declared symbol, and the brute-force checker (tests/clusters_checker.py) against closed forms and
planted scenes: the sheet with strays at three settings, two blobs and a bridge, the distance boundary, a chain, the Select rule against a hand-made
table, and the tree-assisted path of the scale test against the brute force."""
import os
import re
import subprocess

import numpy as np
import pytest

import clusters_checker as cl
import knn_checker as kc
from immesh_amd import capi
from test_knn_cpu import sheet_with_strays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "immesh_nearest.h")
NEW = ("immesh_cloud_clusters", "immesh_cloud_clusters_table", "immesh_cloud_clusters_select", "immesh_cloud_clusters_last_timing")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(capi.hip_library_path()):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "immesh_amd", "csrc"), "-j8"])
    return capi.load_hip_library()


# ---- the boundary ----------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_new_entry_points_in_plain_c99(tmp_path):
    text = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    fns = set(re.findall(r"\b(immesh_[a-z_0-9]+)\s*\(", code))
    assert set(NEW) <= fns, sorted(set(NEW) - fns)
    assert "{" not in code.replace('extern "C" {', "")                               # still no struct body
    assert "The Clusters rule" in text and text.index("the Outliers rule") < text.index("The Clusters rule")
    body = ('int main(void) { immesh_cloud_index* x = 0; int32_t c[2]; int64_t n[4]; float ms[6]; uint8_t k[2];\n'
            '  return immesh_cloud_clusters(x, 1.0, 0, c, k, n, n) + immesh_cloud_clusters_table(x, c, c, c, ms, 1, n)\n'
            '    + immesh_cloud_clusters_select(x, 0, 0, 0, 1, n, k) + immesh_cloud_clusters_last_timing(x, ms) + IMMESH_E_INTERNAL; }\n')
    for i, text in enumerate(('#include "immesh_nearest.h"\n' + body, '#include "immesh_topology.h"\n#include "immesh_nearest.h"\n' + body,
                              '#include "immesh_nearest.h"\n#include "immesh_topology.h"\n' + body)):
        src = tmp_path / ("unit%d.c" % i)
        src.write_text(text)
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-c", "-I", os.path.join(ROOT, "include"), str(src),
                               "-o", str(tmp_path / ("unit%d.o" % i))])


def test_library_exports_the_new_symbols(lib):
    missing = [f for f in NEW if not hasattr(lib, f)]
    assert not missing, missing


# ---- planted scenes ----------------------------------------------------------------------------------------------------------------------------
def test_sheet_with_strays_at_three_settings():
    cloud, planted = sheet_with_strays()
    n = len(cloud)
    a = cl.clusters(cloud, 0.5, 0)                                                   # plain Euclidean cluster extraction: every finite point is core
    assert a["n_clusters"] == 24 and a["counts"] == [n - 3, 0, 0, 3] and sorted(a["n_points"].tolist())[-2:] == [2, 2000]
    assert (a["n_points"] == a["n_core"]).all() and (a["label"][planted == 2] == -1).all()
    b = cl.clusters(cloud, 0.5, 6)
    assert b["n_clusters"] == 1 and b["counts"] == [1979, 19, 27, 3] and (b["kind"][planted == 1] == 2).all() and (planted == 1).sum() == 20
    assert b["n_points"].tolist() == [1998] and b["n_core"].tolist() == [1979]
    c = cl.clusters(cloud, 0.3, 4)
    assert c["n_clusters"] == 21 and c["counts"] == [1557, 347, 121, 3]
    for r in (a, b, c):
        assert sum(r["counts"]) == n and r["n_points"].sum() == r["counts"][0] + r["counts"][1] and r["n_core"].sum() == r["counts"][0]
        assert (np.diff(r["first"]) > 0).all() and (r["kind"][r["first"]] == 0).all() and (r["label"][r["first"]] == np.arange(r["n_clusters"])).all()
        assert np.array_equal(r["count"], kc.radius_count_cloud(cloud, 0.5 if r is not c else 0.3))
        for k in range(r["n_clusters"]):                                             # a label is its cluster's smallest core index; the box holds its members
            m = r["label"] == k
            assert np.nonzero(m & (r["kind"] == 0))[0][0] == r["first"][k]
            assert r["box"][k].tolist() == cloud[m].min(axis=0).tolist() + cloud[m].max(axis=0).tolist()


def two_blobs_and_a_bridge(bridge, b_x0, order=None):
    """two 3 x 3 x 2 blobs of lattice points (x in 0 .. 2 and in b_x0 .. b_x0 + 2), a bridge point, and two points far away that see only each other
    -> cloud (39, 3) float32 in the given row order, is_a, is_b, is_bridge, is_far (masks in that order)"""
    g = np.array([[x, y, z] for x in range(3) for y in range(3) for z in range(2)], np.float32)
    cloud = np.concatenate([g, g + np.array([b_x0, 0, 0], np.float32), np.array([bridge], np.float32), np.array([[100, 0, 0], [101, 0, 0]], np.float32)])
    what = np.repeat([0, 1, 2, 3], [18, 18, 1, 2])
    if order is not None:
        cloud, what = cloud[order], what[order]
    return cloud, what == 0, what == 1, what == 2, what == 3


# row orders of the scene: as built (blob A holds the lower indices), reversed (blob B does), and two shuffles
BRIDGE_ORDERS = (np.arange(39), np.arange(39)[::-1].copy(), np.random.default_rng(1).permutation(39), np.random.default_rng(2).permutation(39))


def test_two_blobs_and_a_bridge():
    # radius 2, min_neighbours 9: a blob's corner has exactly nine others within 2, the bridge at (3, 1, 0) has seven of A and one of B
    cloud, is_a, is_b, is_bridge, is_far = two_blobs_and_a_bridge((3, 1, 0), 5)
    count = kc.radius_count_cloud(cloud, 2.0)
    assert count[is_a | is_b].min() == 9 and count[is_bridge].tolist() == [8] and count[is_far].tolist() == [1, 1]
    r = cl.clusters(cloud, 2.0, 9)
    assert r["n_clusters"] == 2 and r["counts"] == [36, 1, 2, 0] and r["first"].tolist() == [0, 18]
    assert (r["label"][is_a] == 0).all() and (r["label"][is_b] == 1).all()           # the bridge joins nothing: two clusters stay two
    assert r["kind"][is_bridge].tolist() == [1] and r["label"][is_bridge].tolist() == [0]      # D = 1 from A, D = 4 from B
    assert r["kind"][is_far].tolist() == [2, 2] and r["label"][is_far].tolist() == [-1, -1]     # candidates, but none that is core
    assert r["n_points"].tolist() == [19, 18] and r["n_core"].tolist() == [18, 18]
    assert r["box"].tolist() == [[0, 0, 0, 3, 2, 1], [5, 0, 0, 7, 2, 1]]
    # with the bridge core (min_neighbours 8) it joins the two blobs
    r = cl.clusters(cloud, 2.0, 8)
    assert r["n_clusters"] == 1 and r["counts"] == [37, 0, 2, 0]
    # moved to exactly equal D from both: the cluster of the smaller core index, whichever blob holds it
    holders = set()
    for order in BRIDGE_ORDERS:
        cloud, is_a, is_b, is_bridge, is_far = two_blobs_and_a_bridge((4, 1, 0), 6, order)
        r = cl.clusters(cloud, 2.0, 9)
        assert r["n_clusters"] == 2 and r["counts"] == [36, 1, 2, 0] and kc.radius_count_cloud(cloud, 2.0)[is_bridge].tolist() == [2]
        ends = [int(np.nonzero((cloud == np.array(p, np.float32)).all(axis=1))[0][0]) for p in ((2, 1, 0), (6, 1, 0))]
        assert r["label"][is_bridge][0] == r["label"][min(ends)]
        holders.add(bool(is_a[min(ends)]))
    assert holders == {True, False}                                                  # either blob held the smaller index in some order


def test_boundary_and_chain():
    line = np.zeros((40, 3), np.float32)
    line[:, 0] = np.arange(40)
    r = cl.clusters(line, 1.0, 0)                                                    # D == r2 is a candidate
    assert r["n_clusters"] == 1 and r["label"].tolist() == [0] * 40 and r["box"].tolist() == [[0, 0, 0, 39, 0, 0]]
    below = np.nextafter(1.0, 0.0)
    r = cl.clusters(line, below, 0)
    assert r["n_clusters"] == 40 and r["label"].tolist() == list(range(40)) and r["n_points"].tolist() == [1] * 40
    r = cl.clusters(line, below, 1)
    assert r["n_clusters"] == 0 and r["counts"] == [0, 0, 40, 0] and (r["label"] == -1).all() and r["box"].shape == (0, 6)
    r = cl.clusters(line, 1.0, 2)                                                    # the two ends have one neighbour: border points of the chain
    assert r["n_clusters"] == 1 and r["counts"] == [38, 2, 0, 0] and r["first"].tolist() == [1] and r["kind"][[0, 39]].tolist() == [1, 1]
    for order in (np.arange(40)[::-1], np.random.default_rng(2).permutation(40)):
        r = cl.clusters(line[order], 1.0, 0)
        assert r["n_clusters"] == 1 and r["first"].tolist() == [0]
    empty = cl.clusters(np.zeros((0, 3), np.float32), 1.0, 0)
    assert empty["n_clusters"] == 0 and empty["counts"] == [0, 0, 0, 0]
    bad = cl.clusters(np.array([[np.nan, 0, 0], [0, np.inf, 0]], np.float32), 1.0, 0)
    assert bad["n_clusters"] == 0 and bad["counts"] == [0, 0, 0, 2] and bad["kind"].tolist() == [3, 3]
    same = np.tile(np.array([[1.5, -2, 3]], np.float32), (5, 1))                     # coincident points are each other's candidates at D = 0
    assert cl.clusters(same, 1e-3, 4)["counts"] == [5, 0, 0, 0] and cl.clusters(same, 1e-3, 5)["counts"] == [0, 0, 5, 0]


def test_select_against_a_hand_made_table():
    ref = dict(n_points=np.array([5, 9, 9, 2, 7], np.int32), label=np.array([0, 1, -1, 2, 3, -1, 4, 1, -1], np.int32),
               kind=np.array([0, 0, 2, 1, 0, 3, 0, 1, 2], np.uint8))
    assert cl.select(ref)["keepc"].tolist() == [True] * 5 and cl.select(ref)["counts"] == [6, 0, 2, 1]
    assert cl.select(ref, keep_noise=1)["counts"] == [8, 0, 0, 1]
    assert cl.select(ref, min_points=7)["keepc"].tolist() == [False, True, True, False, True]
    assert cl.select(ref, min_points=3, max_points=8)["keepc"].tolist() == [True, False, False, False, True]
    assert cl.select(ref, keep_largest=1)["keepc"].tolist() == [False, True, False, False, False]          # the tie goes to the smaller number
    assert cl.select(ref, keep_largest=2)["keepc"].tolist() == [False, True, True, False, False]
    assert cl.select(ref, keep_largest=3, max_points=8)["keepc"].tolist() == [False, False, False, False, True]   # ranked over ALL clusters
    assert cl.select(ref, keep_largest=9)["keepc"].tolist() == [True] * 5
    out = cl.select(ref, min_points=6)
    assert out["keep"].tolist() == [False, True, False, True, False, False, True, True, False] and out["counts"] == [4, 2, 2, 1]
    assert cl.select(ref, min_points=10, keep_noise=1)["keep"].tolist() == [False, False, True, False, False, False, False, False, True]


# ---- the scale test's path ------------------------------------------------------------------------------------------------------------------------
def test_tree_assisted_path_equals_the_brute_force():
    rng = np.random.default_rng(12)
    cloud = rng.uniform(-5, 5, (2500, 3)).astype(np.float32)
    cloud[100:110] = cloud[90:100]                                                   # coincident pairs
    cloud[7, 1] = np.nan
    cloud[:300] = np.round(cloud[:300])                                              # lattice points: pairs at exactly 1.0
    for radius, min_nb in ((1.0, 0), (1.0, 12), (0.6, 2), (0.8, 4)):
        a, b = cl.clusters(cloud, radius, min_nb), cl.clusters_tree(cloud, radius, min_nb)
        for key in a:
            assert (a[key].tobytes() == b[key].tobytes()) if isinstance(a[key], np.ndarray) else a[key] == b[key], (radius, min_nb, key)
        assert a["n_clusters"] > 3 and (min_nb == 0 or min(a["counts"][:3]) > 0)
    assert cl.same_partition(a["label"], a["label"][::-1][::-1]) and not cl.same_partition(a["label"], np.roll(a["label"], 1))
