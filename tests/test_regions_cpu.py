"""The region-bucket contract of include/immesh_regions.h without a GPU:
  * tests/region_checker.py pinned to the reference's OWN Triangle_manager (oracle/_ref/libref_triangle.so).  The wrapper shows the manager's live set
    bucket by bucket (rt_live walks m_triangle_set_in_region), not the bucket boundaries: the checker's partition is right when that sequence splits
    into exactly as many maximal runs of equal checker key as the checker has non-empty regions -- a misfiled triangle that lands inside another
    bucket's run makes more runs than keys;
  * the header is plain C, its struct layout is the binding's, and the library exports what it declares."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from immesh_amd import capi, synth
from conftest import make_oracle
from ref_triangle_mirror import RefTriangleMirror
from region_checker import RegionChecker, region_keys, round_half_away

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "immesh_regions.h")


def world_scan(k, n, cfg):
    """scan k in the world frame with the true pose (the stream of test_hip_diff_lists_on_the_reference_triangle_manager)"""
    R, t = synth.trajectory_pose(k)
    extT = np.array(list(cfg.extT))
    raw = synth.livox_scan(k, R, t, n_pts=n, extT=extT)
    pw = (raw[:, :3].astype(np.float64) + extT) @ R.T + t
    out = raw.copy()
    out[:, :3] = pw.astype(np.float32)
    return np.ascontiguousarray(out), t


def live_sequence(mirror):
    """the manager's live triangles in rt_live's order: bucket after bucket"""
    n = int(mirror.lib.rt_live_size(mirror.ctx))
    tri = np.zeros((max(n, 1), 3), np.int32); flip = np.zeros(max(n, 1), np.uint8)
    assert int(mirror.lib.rt_live(mirror.ctx, tri.ctypes.data_as(C.c_void_p), flip.ctypes.data_as(C.c_void_p), n)) == n
    return tri[:n]


def runs_and_keys(mirror, chk):
    """(maximal runs of equal checker key in the manager's bucket-by-bucket sequence, non-empty checker regions, live triangles)"""
    seq = live_sequence(mirror)
    assert set(map(tuple, seq.tolist())) == chk.live()                       # union equal
    keys = region_keys(chk.vtx, seq, chk.S, chk.rounding)
    runs = 0 if len(keys) == 0 else 1 + int(np.count_nonzero(np.any(keys[1:] != keys[:-1], axis=1)))
    return runs, sum(1 for s in chk.sets if s), len(seq)


def test_round_half_away_is_std_round():
    x = np.array([0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 0.49999999999999994, -0.49999999999999994, 0.0, -0.0, 1e15 + 0.5, 3.4999999999999996, 7.0, -7.2])
    want = np.array([1, -1, 2, -2, 3, -3, 0, 0, 0, 0, 1e15 + 1, 3, 7, -7], np.float64)
    np.testing.assert_array_equal(round_half_away(x), want)


@pytest.mark.parametrize("region", [10.0, 2.0])
def test_checker_partition_is_the_reference_managers(oracle_lib, ref_tri_lib, region):
    cfg = capi.avia_config(cap_root_voxels=1 << 12, cap_scan_points=200000, cap_vertices=1 << 18, cap_triangles=1 << 20, mesh_region=region)
    o = make_oracle(oracle_lib, cfg)
    mirror = RefTriangleMirror(ref_tri_lib, region)
    chk = RegionChecker(region)
    n_rem = 0
    for k in range(8):
        pts, cam = world_scan(k, 40000, cfg)
        m = o.mesh_scan(pts, cam, frame_idx=k)
        assert mirror.apply(m, k) == 0
        n_rem += chk.apply(m)[0]
    runs, keys, n_live = runs_and_keys(mirror, chk)
    print(f"mesh_region {region}: {n_live} live triangles, {runs} runs, {keys} non-empty regions of {len(chk.keys)}")
    assert n_rem > 1000 and n_live > 10000 and keys >= 20
    assert runs == keys
    mirror.close()


def tie_soup(S=10.0):
    """For each axis and each of centroid / S = +-0.5, +-1.5, +-2.5 one tie triangle (all three vertices at the tie coordinate - 1, + 0, + 1 on that axis:
    x = 4, 5, 6 -> centroid 5 -> bucket 1), interleaved among 4 partner triangles of the bucket half-away-from-zero gives it and 4 of its neighbour
    towards zero (centroids 1-4 m inside those buckets).  -> (vertices (n, 3) float32, triangles (n, 3) sorted, in insertion order)"""
    vtx, tris = [], []

    def tri_at(c, axis, spread):
        base = len(vtx)
        u, w = (axis + 1) % 3, (axis + 2) % 3
        for d, du, dw in ((-1.0, 0.0, 0.0), (0.0, spread, 0.0), (1.0, 0.0, spread)):
            p = [0.0, 0.0, 0.0]
            p[axis] = c[axis] + d; p[u] = c[u] + du; p[w] = c[w] + dw
            vtx.append(p)
        tris.append((base, base + 1, base + 2))

    lane = 0
    for axis in range(3):
        for q in (0.5, -0.5, 1.5, -1.5, 2.5, -2.5):
            c = [0.0, 0.0, 0.0]
            u, w = (axis + 1) % 3, (axis + 2) % 3
            c[u] = 0.3 + 0.01 * lane; c[w] = -0.2 + 0.01 * lane        # small offsets on the other axes: bucket 0 there, every vertex distinct
            lane += 1
            sgn = 1.0 if q > 0 else -1.0
            away = sgn * (abs(q) + 0.5) * S                             # centre of the bucket half-away-from-zero chooses
            toward = sgn * (abs(q) - 0.5) * S                           # its neighbour towards zero
            order = []
            for i in range(4):
                order.append(("p", away + sgn * (-4.0 + i)))            # 1-4 m inside the tie's bucket, measured from the tie plane
                order.append(("p", toward + sgn * (4.0 - i)))
                if i == 1:
                    order.append(("t", q * S))
            for kind, x in order:
                cc = list(c); cc[axis] = x
                tri_at(cc, axis, 0.25)
    return np.array(vtx, np.float32), np.array(tris, np.int32)


def test_tie_soup_against_the_reference_manager(ref_tri_lib):
    S = 10.0
    vtx, tris = tie_soup(S)
    assert len(tris) == 162
    # every tie centroid is exactly on a bucket boundary
    p = vtx.astype(np.float64)
    c = ((p[tris[:, 0]] + p[tris[:, 1]]) + p[tris[:, 2]]) / 3.0 / S
    assert np.count_nonzero(np.any(np.abs(c - np.trunc(c)) == 0.5, axis=1)) == 18
    m = {"new_vtx": vtx, "vtx_base": 0, "tri_rem": np.zeros((0, 3), np.int32), "tri_add": tris, "flip_add": np.zeros(len(tris), np.uint8),
         "tri_upd": np.zeros((0, 3), np.int32), "flip_upd": np.zeros(0, np.uint8)}

    def run(rounding):
        mirror = RefTriangleMirror(ref_tri_lib, S)
        assert mirror.apply(m, 0) == 0
        chk = RegionChecker(S, rounding)
        chk.apply(m)
        runs, keys, n = runs_and_keys(mirror, chk)
        mirror.close()
        return runs, keys

    runs, keys = run(round_half_away)
    print("half away from zero:", runs, "runs,", keys, "keys")
    assert runs == keys
    # the case has teeth: any other rounding misfiles the ties into the middle of another bucket's run
    for name, wrong in (("np.round", np.round), ("floor(x + 0.5)", lambda x: np.floor(np.asarray(x) + 0.5)), ("truncation", np.trunc)):
        r, k = run(wrong)
        print(f"{name}: {r} runs, {k} keys")
        assert r != k, name


def test_header_is_plain_c_and_layout_matches_the_binding(tmp_path):
    src = open(HEADER).read()
    body = src[src.index("typedef struct immesh_region_info {"):src.index("} immesh_region_info;")]
    names = []
    for decl in re.findall(r"\b(?:int64_t|int32_t)\s+([^;]+);", body):
        names += [re.sub(r"\[\d+\]", "", n).strip() for n in decl.split(",")]
    assert names == [n for n, _ in capi.RegionInfo._fields_]
    prog = tmp_path / "layout.c"
    prog.write_text('#include "immesh_regions.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void) {\n  printf("%zu", sizeof(immesh_region_info));\n' +
                    "".join(f'  printf(" %zu", offsetof(immesh_region_info, {n}));\n' for n in names) + "  return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(prog), "-o", exe])
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == 32 == C.sizeof(capi.RegionInfo)
    assert got[1:] == [getattr(capi.RegionInfo, n).offset for n in names]
    assert [capi.REGION_DTYPE.fields[n][1] for n in names] == got[1:]


def test_library_exports_every_function_of_the_header():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    funcs = re.findall(r"\b(immesh_\w+)\s*\(", src)
    assert set(funcs) == {"immesh_mesh_regions_enable", "immesh_mesh_regions", "immesh_mesh_regions_sync", "immesh_mesh_regions_fetch", "immesh_region_keys",
                          "immesh_mesh_regions_error"}
    so = capi.hip_library_path()
    assert os.path.exists(so), "build the library first (__graft_entry__.build)"
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for f in funcs:
        assert f in exported, f
