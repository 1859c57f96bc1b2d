"""Row a20 at its size boundaries: every route a voxel can take through the per-voxel triangulation, on inputs that provably land there.

The route depends on the neighbourhood size n_u: the register-resident triangulation (n_u <= 64; one launch or split in two), mesh_delaunay_voxel with
its tables in LDS (65..256, and what the fast path hands over), the same with its tables in a block's slice of global scratch (257..1024).  Inside each
there is a second fork: the live triangles gathered from the smallest-vertex lists either fit an on-chip list (512 entries below 257 vertices, 2048
above) or are classified straight from the vertex lists.  The oracle has no routes -- one plain-double Bowyer-Watson for every size -- so each test
first proves FROM THE ORACLE's n_u and old-set sizes (never from the code under test) that its input lands where it is meant to, then asks for
what every mesher parity test asks for: ids and every triangle / flip list bit-equal, smoothed positions to 1e-9, n_u per voxel and the counters equal.

The oracle side of a stream is computed once per module and shared (it is the larger part of a test's time)."""
import numpy as np
import pytest

from immesh_amd import capi
from conftest import make_oracle, make_hip
from parity_utils import compare_scan

pytestmark = pytest.mark.gpu

FAST_MAX, LDS_MAX, GEN_MAX = 64, 256, 1024        # largest n_u of the three routes (mesh_kernels.hip mesh_delaunay_general_kernel)
FAST_OLD_CAP, LDS_OLD_CAP, GEN_OLD_CAP = 512, 512, 2048   # DF_OLD_CAP, 2 * CAP at CAP = 256, 2 * CAP at CAP = MV_REL_CAP
GEN_BLOCKS = 32                                   # MV_GEN_BLOCKS: one scratch slice per block
COUNTER_KEYS = ("n_app", "n_new", "v_act", "n_v", "n_u", "t_v", "t_add", "t_rem", "n_vertices", "n_triangles_live", "n_degenerate_skips")
CAPS = dict(cap_root_voxels=1 << 12, cap_scan_points=200000, cap_vertices=1 << 16, cap_triangles=1 << 21)


def _xyzi(p):
    p = np.asarray(p, np.float64)
    return np.ascontiguousarray(np.concatenate([p, np.ones((len(p), 1))], axis=1).astype(np.float32))


# ---- the streams (plain numpy; each returns cfg, scans, cam) ------------------------------------------------------------------------------------------
def lattice_stream():
    """A jittered cubic lattice at 1.06 x the admission spacing, spacing ratio 4.9, filling a 2.4 m cube, delivered in random thirds: the
    neighbourhoods grow through every route from scan to scan, and scans 1 and 2 re-mesh what the earlier ones left."""
    cfg = capi.avia_config(mesh_append_budget=200000, **CAPS)
    cfg.mesh_min_spacing = 0.4 / 4.9
    spacing = cfg.mesh_min_spacing
    rng = np.random.default_rng(41)
    n = int(2.4 / (1.06 * spacing))
    g = np.stack(np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij"), axis=-1).reshape(-1, 3)
    p = (g + 0.5) * 1.06 * spacing + rng.uniform(-0.02, 0.02, g.shape) * spacing
    p = p[rng.permutation(len(p))]
    return cfg, [_xyzi(c) for c in np.array_split(p, 3)], np.array([-3.0, 1.0, 1.0])


def thin_volumetric_stream():
    """3000 uniform points a scan in a 4 m cube, shipped constants: small neighbourhoods, but triangles of many projection planes pile up around them."""
    cfg = capi.avia_config(**CAPS)
    rng = np.random.default_rng(31)
    return cfg, [_xyzi(rng.uniform(0.0, 4.0, (3000, 3))) for _ in range(4)], np.array([-3.0, 1.0, 1.0])


def exact_lattice_stream():
    """An exact 20^3 cubic lattice (coordinates are multiples of 1 / 64) at spacing ratio 4.9 on 0.5 m voxels, in two random halves: cocircular and
    collinear quadruples everywhere, on neighbourhoods above 256."""
    cfg = capi.avia_config(mesh_append_budget=200000, **CAPS)
    cfg.mesh_voxel = 0.5
    cfg.mesh_min_spacing = 0.5 / 4.9
    g = np.stack(np.meshgrid(np.arange(20), np.arange(20), np.arange(20), indexing="ij"), axis=-1).reshape(-1, 3)
    p = 1.0 + g * (7.0 / 64.0)
    assert np.array_equal(p.astype(np.float32).astype(np.float64), p)          # the float32 round trip is exact
    p = p[np.random.default_rng(43).permutation(len(p))]
    return cfg, [_xyzi(c) for c in np.array_split(p, 2)], np.array([-3.0, 1.0, 1.0])


def smallest_stream():
    """Two isolated mesh voxels (5 m apart: no shared neighbourhood).  Voxel A holds exactly 3 vertices; voxel B holds 4 of which three lie on one
    line (exactly, in space: binary fractions, so they are collinear in any projection up to its rounding).  The re-scan adds one vertex to each.
    The points are off any common plane by centimetres where that is possible (a 3-vertex set is planar by nature), the in-plane extents differ:
    the PCA has three distinct eigenvalues."""
    cfg = capi.avia_config(**CAPS)
    a = np.array([[2.0, 2.0, 2.0], [2.140625, 1.984375, 2.015625], [2.03125, 2.15625, 1.984375]])
    d = np.array([0.125, 0.03125, 0.015625])
    b0 = np.array([6.65625, 1.9375, 1.96875])
    b = np.stack([b0, b0 + d, b0 + 2 * d, b0 + np.array([0.0625, 0.171875, -0.015625])])
    assert np.array_equal(np.cross(b[1] - b[0], b[2] - b[0]), np.zeros(3))     # exactly collinear
    first = np.concatenate([a, b])
    second = np.array([[2.109375, 2.109375, 2.046875], [6.84375, 2.125, 2.03125]])
    for s in (first, second):
        assert np.array_equal(s.astype(np.float32).astype(np.float64), s)
    return cfg, [_xyzi(first), _xyzi(second)], np.array([-3.0, 1.0, 1.0])


# ---- the oracle side, once per stream -------------------------------------------------------------------------------------------------------------------
_STREAMS = {"lattice": lattice_stream, "thin": thin_volumetric_stream, "exact": exact_lattice_stream, "smallest": smallest_stream}
_ORACLE = {}


def oracle_run(oracle_lib, name):
    """cfg, scans, cam, per-scan records {m, n_u, old, skips} and the final counters of the oracle on the named stream (cached; read-only)."""
    if name not in _ORACLE:
        cfg, scans, cam = _STREAMS[name]()
        o = make_oracle(oracle_lib, cfg)
        o.set_threads(8, 1)                      # (the voxel-parallel part only; the results do not depend on it)
        recs, skips = [], 0
        for k, pts in enumerate(scans):
            m = o.mesh_scan(pts, cam, frame_idx=k)
            n_u, old = o.mesh_neighbourhood_sizes().copy(), o.mesh_old_set_sizes().copy()
            assert len(n_u) == len(old) == m["n_voxels_meshed"]
            s = o.counters()["n_degenerate_skips"]
            recs.append({"m": m, "n_u": n_u, "old": old, "skips": s - skips})
            skips = s
            for a in list(m.values()) + [n_u, old]:
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
        _ORACLE[name] = (cfg, scans, cam, recs, o.counters())
        o.close()
    return _ORACLE[name]


def route_table(recs):
    """per scan: voxels, max n_u, voxels per route, the largest gathered old set per route"""
    rows = []
    for r in recs:
        n_u, old = r["n_u"], r["old"]
        sel = (n_u <= FAST_MAX, (n_u > FAST_MAX) & (n_u <= LDS_MAX), n_u > LDS_MAX)
        rows.append({"voxels": len(n_u), "max_n_u": int(n_u.max()) if len(n_u) else 0, "per_route": tuple(int(s.sum()) for s in sel),
                     "max_old": tuple(int(old[s].max()) if s.any() else 0 for s in sel), "skips": r["skips"]})
    return rows


def hip_matches_oracle(hip_lib, run, tag):
    """feed the stream to the HIP library; every scan's lists and n_u, and the counters at the end, against the oracle's record"""
    cfg, scans, cam, recs, counters = run
    h = make_hip(hip_lib, cfg)
    try:
        for k, (pts, rec) in enumerate(zip(scans, recs)):
            mh = h.mesh_scan(pts, cam, frame_idx=k)
            compare_scan(rec["m"], mh, f"{tag} scan {k}")
            np.testing.assert_array_equal(h.mesh_neighbourhood_sizes(), rec["n_u"], err_msg=f"{tag} scan {k} n_u")
        ch = h.counters()
        for key in COUNTER_KEYS:
            assert ch[key] == counters[key], (tag, key, ch[key], counters[key])
    finally:
        h.close()


# ---- (a) ----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", ["0", "1"])
def test_every_route_and_every_boundary_in_one_stream(oracle_lib, hip_lib, split, monkeypatch):
    """All three routes in one stream, with a voxel at each side of both thresholds (n_u = 64, 65, 256, 257), more voxels above 256 in one scan than
    the general launch has blocks (a block walks several: its scratch slice is reused), voxels above 256 re-meshed in a scan that removes triangles
    and rewrites flips, and voxels of 65..256 whose gathered old set overflows the 512-entry list.  split 1: the fast path as two launches
    (mesh_tri64_kernel + mesh_diff64_kernel), its hand-over (tri_nf = -1) crossing them.

    Oracle, per scan (voxels; max n_u; voxels <= 64 / 65..256 / > 256; largest old set per route):
      0: 334; 181; 105 / 229 / 0;   0 / 0 / 0          (sizes 63, 64, 65 present)
      1: 342; 265;  67 / 263 / 12;  275 / 1144 / 1144  (63, 64, 255, 256, 257)
      2: 342; 337;  29 / 232 / 81;  371 / 1530 / 1878  (63, 64, 65)
    The largest old set above 256 vertices, 1878, stays 170 below its 2048-entry list: that overflow branch remains unreached."""
    monkeypatch.setenv("IMMESH_SPLIT", split)   # (read when a context is created)
    run = oracle_run(oracle_lib, "lattice")
    recs = run[3]
    table = route_table(recs)
    print("lattice stream, oracle:", table)
    sizes = set(np.concatenate([r["n_u"] for r in recs]).tolist())
    assert {FAST_MAX, FAST_MAX + 1, LDS_MAX, LDS_MAX + 1} <= sizes, sorted(s for s in sizes if 60 < s < 70 or 250 < s < 262)
    assert max(sizes) <= GEN_MAX
    assert max(t["per_route"][2] for t in table) > GEN_BLOCKS                                   # pigeonhole: some block reuses its slice
    assert any(t["per_route"][2] > 0 and len(r["m"]["tri_rem"]) > 0 and len(r["m"]["tri_upd"]) > 0 for t, r in zip(table, recs))
    assert max(t["max_old"][1] for t in table) > LDS_OLD_CAP                                   # classified straight from the vertex lists, tables in LDS
    hip_matches_oracle(hip_lib, run, f"lattice split {split}")


# ---- (b) ----------------------------------------------------------------------------------------------------------------------------------------------------
def test_old_set_longer_than_the_fast_path_list(oracle_lib, hip_lib):
    """Fast-path voxels (n_u <= 64) whose smallest-vertex lists hold more live triangles than the 512-entry LDS list, beside fast-path voxels that
    stay below it: both branches of mesh_delaunay64.inc's diff in one launch.

    Oracle, per scan (voxels; max n_u; voxels <= 64 / 65..256 / > 256; largest old set per route):
      0: 463; 49;  463 / 0 / 0;    0 / 0 / 0
      1: 856; 67;  855 / 1 / 0;    441 / 361 / 0
      2: 911; 72;  883 / 28 / 0;   725 / 618 / 0
      3: 892; 83;  691 / 201 / 0;  604 / 755 / 0"""
    run = oracle_run(oracle_lib, "thin")
    recs = run[3]
    print("thin volumetric stream, oracle:", route_table(recs))
    both = False
    for r in recs:
        fast = r["n_u"] <= FAST_MAX
        both |= bool((r["old"][fast] > FAST_OLD_CAP).any() and ((r["old"][fast] > 0) & (r["old"][fast] < FAST_OLD_CAP)).any())
    assert both                                     # one scan = one launch with a voxel on either side
    hip_matches_oracle(hip_lib, run, "thin volumetric")


# ---- (c) ----------------------------------------------------------------------------------------------------------------------------------------------------
def test_exact_lattice_on_the_global_scratch_route(oracle_lib, hip_lib):
    """Degenerate predicates (exact cocircular / collinear quadruples: the set-based insertion rule, points that are not inserted) on the route above
    256 vertices; the count of not-inserted points must be the oracle's.

    Oracle, per scan (voxels; max n_u; voxels <= 64 / 65..256 / > 256; largest old set per route; points not inserted):
      0: 125; 224; 8 / 117 / 0;  0 / 0 / 0;        0
      1: 125; 336; 0 / 118 / 7;  0 / 1182 / 1373;  1255"""
    run = oracle_run(oracle_lib, "exact")
    recs, counters = run[3], run[4]
    table = route_table(recs)
    print("exact lattice stream, oracle:", table)
    assert max(t["per_route"][2] for t in table) > 0 and max(t["max_n_u"] for t in table) <= GEN_MAX
    assert counters["n_degenerate_skips"] > 0
    hip_matches_oracle(hip_lib, run, "exact lattice")       # (n_degenerate_skips is among the counters compared)


# ---- (d) ----------------------------------------------------------------------------------------------------------------------------------------------------
def test_smallest_neighbourhoods_on_the_fast_path(oracle_lib, hip_lib):
    """n_u = 3 (one triangle, nothing to insert after the first) and n_u = 4 with three vertices on a line (a first triangle cannot be the first three
    points; the sliver is for the angle filter), then one more vertex in each: the re-scan diffs against the triangles of the first."""
    run = oracle_run(oracle_lib, "smallest")
    recs = run[3]
    assert recs[0]["n_u"].tolist() == [3, 4] and recs[1]["n_u"].tolist() == [4, 5]     # (voxel order: ascending key, A before B)
    assert recs[0]["old"].tolist() == [0, 0] and len(recs[0]["m"]["tri_add"]) >= 2
    assert min(recs[1]["old"]) >= 1                                                       # the re-scan has something to diff against
    hip_matches_oracle(hip_lib, run, "smallest")
