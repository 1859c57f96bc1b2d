"""The renderer's region buckets on the device (include/immesh_regions.h) against tests/region_checker.py -- the contract's restatement, pinned to the
reference's own Triangle_manager by tests/test_regions_cpu.py.  Everything is integer- or bit-exact."""
import ctypes as C
import threading

import numpy as np
import pytest

from immesh_amd import capi, synth
from conftest import make_hip
from region_checker import RegionChecker, region_keys
from test_regions_cpu import world_scan, tie_soup

pytestmark = pytest.mark.gpu

CAPS = dict(cap_root_voxels=1 << 12, cap_scan_points=200000, cap_vertices=1 << 18, cap_triangles=1 << 20)


def _check_table(h, chk, tag):
    tab = h.mesh_regions()
    keys, n_tri, dirty = chk.table()
    assert len(tab) == len(keys), tag
    np.testing.assert_array_equal(tab["key"].reshape(-1, 3), keys, err_msg=f"{tag} keys in index order")
    np.testing.assert_array_equal(tab["index"], np.arange(len(keys)), err_msg=tag)
    np.testing.assert_array_equal(tab["n_triangles"], n_tri, err_msg=f"{tag} n_triangles")
    np.testing.assert_array_equal(tab["dirty"], dirty, err_msg=f"{tag} dirty")
    return tab


def _check_sync(h, chk, res, want, tag, params=(1.0, 20, 0.0)):
    """res = a fetched sync, want = RegionChecker.sync()'s answer for the same moment"""
    reg = res["regions"]
    assert [int(r) for r in reg["index"]] == [r for r, _ in want], f"{tag} taken regions"
    np.testing.assert_array_equal(reg["key"].reshape(-1, 3), np.array([chk.keys[r] for r, _ in want], np.int32).reshape(-1, 3), err_msg=tag)
    counts = np.array([len(t) for _, t in want], np.int64)
    np.testing.assert_array_equal(reg["n_triangles"], counts, err_msg=f"{tag} counts")
    np.testing.assert_array_equal(reg["first"], np.concatenate([[0], np.cumsum(counts)])[:-1], err_msg=f"{tag} offsets")
    tris = [t for _, ts in want for t in ts]
    np.testing.assert_array_equal(res["tri"], np.array(tris, np.int32).reshape(-1, 3), err_msg=f"{tag} triplets (region rank, then lexicographic)")
    np.testing.assert_array_equal(res["flip"], np.array([chk.flips[t] for t in tris], np.uint8), err_msg=f"{tag} flips")
    if len(tris):
        disp = h.mesh_display_vertices(res["tri"].reshape(-1), *params)
        assert res["xyz"].tobytes() == disp.tobytes(), f"{tag} display positions"     # (byte-equal: NaNs included)


@pytest.mark.parametrize("cadence", [1, 3])
@pytest.mark.parametrize("region", [10.0, 2.0])
def test_stream_parity(hip_lib, region, cadence):
    """Table after every scan, taken regions + buffers at every sync, nothing reported twice."""
    cfg = capi.avia_config(mesh_region=region, **CAPS)
    h = make_hip(hip_lib, cfg)
    h.mesh_regions_enable()
    chk = RegionChecker(region)
    max_rem, clean_max, created = 0, 0, []
    for k in range(8):
        pts, cam = world_scan(k, 40000, cfg)
        m = h.mesh_scan(pts, cam, frame_idx=k)
        n_rem, n_new = chk.apply(m)
        max_rem = max(max_rem, n_rem); created.append(n_new)
        _check_table(h, chk, f"scan {k}")
        if (k + 1) % cadence == 0 or k == 7:
            n_clean = len(chk.keys) - int(np.count_nonzero(chk.table()[2]))
            if k > 0:
                clean_max = max(clean_max, n_clean)
            want = chk.sync()
            res = h.mesh_regions_sync(1.0, 20, 0.0)
            assert np.all(res["regions"]["dirty"] == 1)
            _check_sync(h, chk, res, want, f"scan {k} sync")
            assert h.mesh_regions_sync(1.0, 20, 0.0, fetch=False) == (0, 0)            # a second sync straight away: nothing
            assert not _check_table(h, chk, f"scan {k} after sync")["dirty"].any()
    print(f"mesh_region {region} cadence {cadence}: regions created per scan {created}, most removals in a scan {max_rem}, most clean regions at a sync {clean_max}")
    assert max_rem > 1000 and len(chk.keys) >= 20                                        # the stream exercises removals and region creation
    if cadence == 1 and region == 2.0:
        assert clean_max >= 1                                                            # ... and regions that must NOT be returned
    h.close()


def test_force_all_returns_every_region(hip_lib):
    cfg = capi.avia_config(mesh_region=2.0, **CAPS)
    h = make_hip(hip_lib, cfg)
    h.mesh_regions_enable()
    chk = RegionChecker(2.0)
    for k in range(5):
        pts, cam = world_scan(k, 40000, cfg)
        chk.apply(h.mesh_scan(pts, cam, frame_idx=k))
    h.mesh_regions_sync(1.0, 20, 0.0, fetch=False); chk.sync()                           # flags cleared: force_all must not care
    res = h.mesh_regions_sync(1.0, 20, 0.0, force_all=True)
    want = chk.sync(force_all=True)
    assert len(res["regions"]) == len(chk.keys) == len(h.mesh_regions()) and not res["regions"]["dirty"].any()
    _check_sync(h, chk, res, want, "force_all")
    vtx, faces = h.mesh_export(smooth_factor=0.0)
    exported = {tuple(sorted(map(int, f))) for f in faces}
    got = set(map(tuple, res["tri"].tolist()))
    assert len(got) == len(res["tri"]) == len(exported) == h.counters()["n_triangles_live"]
    assert got == exported
    h.close()


def test_many_regions_created_by_one_job(hip_lib):
    """The offline entry on a 12 m x 12 m surface at mesh_region 2: every region is created by ONE job; indices = first appearance in the add list."""
    n = 40000
    cfg = capi.avia_config(cap_root_voxels=1 << 12, cap_scan_points=200000, cap_vertices=1 << 17, cap_triangles=1 << 20, mesh_append_budget=50000000, mesh_region=2.0)
    h = make_hip(hip_lib, cfg)
    h.mesh_regions_enable()
    rng = np.random.default_rng(31)
    x = rng.uniform(-6, 6, n); y = rng.uniform(-6, 6, n)
    z = 0.2 * np.sin(x) + 0.1 * np.cos(1.7 * y) + rng.normal(0, 0.003, n)
    pts = np.stack([x, y, z, rng.uniform(0, 100, n)], axis=1).astype(np.float32)
    m = h.reconstruct_mesh_from_pointcloud(pts, 0.01)
    chk = RegionChecker(2.0)
    _, created = chk.apply(m)
    assert created >= 36 and len(m["tri_add"]) > 15000
    _check_table(h, chk, "offline cloud")
    _check_sync(h, chk, h.mesh_regions_sync(1.0, 20, 0.0), chk.sync(), "offline cloud sync")
    h.close()


def test_key_rule_on_ties(hip_lib):
    cfg = capi.avia_config(mesh_region=10.0, **CAPS)
    h = make_hip(hip_lib, cfg)                                                           # (works with the table off)
    vtx, tris = tie_soup(10.0)
    np.testing.assert_array_equal(h.region_keys(vtx, tris), region_keys(vtx, tris, 10.0))
    assert set(np.abs(h.region_keys(vtx, tris)).max(axis=1).tolist()) >= {1, 2, 3}
    # ties far from the origin (float32 spacing ~1e-3 m at 1e4 m: integers are still exact) and everything mirrored to negative coordinates
    far = vtx.copy(); far[:, 0] += 10000.0; far[:, 1] -= 10000.0
    for v in (far, -far, -vtx):
        np.testing.assert_array_equal(h.region_keys(v, tris), region_keys(v, tris, 10.0))
    rng = np.random.default_rng(5)
    for centre in (0.0, 1e4, -1e4):
        v = (centre + rng.uniform(-40, 40, (3000, 3))).astype(np.float32)
        v[:600] = np.round(v[:600])                                                     # integer coordinates: sums hit .0 / .333 / .5 patterns
        t = np.sort(rng.integers(0, len(v), (5000, 3)), axis=1).astype(np.int32)
        t[:1000] = np.sort(rng.integers(0, 600, (1000, 3)), axis=1)
        np.testing.assert_array_equal(h.region_keys(v, t), region_keys(v, t, 10.0))
    h2 = make_hip(hip_lib, capi.avia_config(mesh_region=2.0, **CAPS))
    np.testing.assert_array_equal(h2.region_keys(vtx, tris), region_keys(vtx, tris, 2.0))
    h.close(); h2.close()


def test_two_contexts_are_byte_identical(hip_lib):
    cfg = capi.avia_config(mesh_region=2.0, **CAPS)
    outs = []
    for _ in range(2):
        h = make_hip(hip_lib, cfg)
        h.mesh_regions_enable()
        blob = []
        for k in range(5):
            pts, cam = world_scan(k, 40000, cfg)
            h.mesh_scan(pts, cam, frame_idx=k, fetch=False)
            blob.append(h.mesh_regions().tobytes())
            if k % 2 == 0:
                res = h.mesh_regions_sync(1.0, 20, 0.0)
                blob += [res[key].tobytes() for key in ("regions", "tri", "flip", "xyz")]
        outs.append(blob)
        h.close()
    assert len(outs[0]) > 10 and outs[0] == outs[1]


def test_sync_from_a_third_thread_beside_the_scan_loop(hip_lib):
    """The renderer's thread synchronises while the scan thread registers and meshes asynchronously: every snapshot is self-consistent, and the latest
    buffer of every region over all syncs is the final live set -- no update lost."""
    torch = pytest.importorskip("torch")
    cfg = capi.avia_config(cap_root_voxels=1 << 16, cap_scan_points=200000, cap_vertices=1 << 18, cap_triangles=1 << 20, mesh_region=2.0)
    extT = np.array(list(cfg.extT))
    scans = []
    for k in range(12):
        Rk, tk = synth.trajectory_pose(k)
        raw = synth.livox_scan(k, Rk, tk, n_pts=30000, extT=extT)
        scans.append((torch.from_numpy(synth.voxel_grid_downsample(raw, 0.4)).cuda(), torch.from_numpy(raw).cuda(), Rk, tk))
    h = make_hip(hip_lib, cfg)
    h.mesh_regions_enable()
    st = capi.make_state(R=scans[0][2], t=scans[0][3])
    h.map_build(np.ascontiguousarray(scans[0][1].cpu().numpy()[:, :3]), st)
    st[12:15] = [1.0, 0, 0]; st[15:18] = [0, 0, np.deg2rad(2.0)]
    prior = synth.forward_without_imu(st)
    st, _ = h.process_scan(scans[1][0].data_ptr(), scans[1][1].data_ptr(), prior, prior, frame_idx=1, do_mesh=1, n_ds=scans[1][0].shape[0], n_raw=scans[1][1].shape[0])
    stop, started, errors, seen = threading.Event(), threading.Event(), [], []

    def renderer():
        try:
            while not stop.is_set():
                seen.append(h.mesh_regions_sync(1.0, 20, 0.0))
                started.set()
        except Exception as e:   # noqa: BLE001
            errors.append(e)
            started.set()
    th = threading.Thread(target=renderer); th.start()
    assert started.wait(120)                                                             # the renderer is synchronising by the time the loop starts
    for k in range(2, 12):
        prior = synth.forward_without_imu(st)
        st, _ = h.process_scan(scans[k][0].data_ptr(), scans[k][1].data_ptr(), prior, prior, frame_idx=k, do_mesh=2, n_ds=scans[k][0].shape[0], n_raw=scans[k][1].shape[0])
    h.mesh_wait()
    stop.set(); th.join()
    assert not errors, errors
    seen.append(h.mesh_regions_sync(1.0, 20, 0.0))
    print(f"{len(seen)} syncs, {sum(len(s['regions']) > 0 for s in seen)} of them returned regions")
    assert len(seen) >= 2 and len(seen[0]["regions"]) > 0
    vtx, faces = h.mesh_export(smooth_factor=0.0)                                        # raw positions never change: the final array serves every snapshot
    latest = {}
    for s in seen:
        reg = s["regions"]
        assert int(reg["n_triangles"].sum()) == len(s["tri"])
        keys = region_keys(vtx, s["tri"], 2.0)
        for q in reg:
            a, b = int(q["first"]), int(q["first"]) + int(q["n_triangles"])
            assert np.all(keys[a:b] == q["key"]), "a triangle outside its region's bucket"
            latest[int(q["index"])] = (tuple(int(v) for v in q["key"]), set(map(tuple, s["tri"][a:b].tolist())))
    tab = h.mesh_regions()
    assert not tab["dirty"].any() and set(latest) == set(range(len(tab)))
    final = np.sort(faces, axis=1)
    want = {}
    for t, key in zip(map(tuple, final.tolist()), map(tuple, region_keys(vtx, final, 2.0).tolist())):
        want.setdefault(key, set()).add(t)
    got = {key: tris for key, tris in latest.values() if tris}
    assert got == want
    np.testing.assert_array_equal(tab["n_triangles"], [len(latest[r][1]) for r in range(len(tab))])
    h.close()


def test_no_side_effects(hip_lib):
    """Per-scan lists with the table on are bit-equal to a context without; with the table never enabled no kernel of csrc/regions is launched."""
    cfg = capi.avia_config(mesh_region=2.0, **CAPS)
    a, b = make_hip(hip_lib, cfg), make_hip(hip_lib, cfg)
    b.mesh_regions_enable()
    for k in range(4):
        pts, cam = world_scan(k, 40000, cfg)
        ma, mb = a.mesh_scan(pts, cam, frame_idx=k), b.mesh_scan(pts, cam, frame_idx=k)
        for key in ma:
            assert np.asarray(ma[key]).tobytes() == np.asarray(mb[key]).tobytes(), (k, key)
        if k == 1:
            b.mesh_regions_sync(1.0, 20, 0.0)
    a.close(); b.close()
    names = []
    for on in (False, True):
        h = make_hip(hip_lib, cfg)
        if on:
            h.mesh_regions_enable()
        h.profile_enable(True)
        for k in range(3):
            pts, cam = world_scan(k, 40000, cfg)
            h.mesh_scan(pts, cam, frame_idx=k, fetch=False)
        names.append(set(h.profile_read()))
        h.close()
    assert not [n for n in names[0] if n.startswith("regions_")]
    assert {"regions_mark_kernel", "regions_order_kernel"} <= names[1]                  # (the probe does see them when they run)


def _raises(fn, rc):
    with pytest.raises(RuntimeError) as e:
        fn()
    msg = str(e.value)
    assert f"rc={rc}:" in msg and len(msg.split(":", 1)[1].strip()) > 0, msg


def test_argument_errors(hip_lib):
    cfg = capi.avia_config(mesh_region=2.0, **CAPS)
    h = make_hip(hip_lib, cfg)
    assert h.mesh_regions_error() == ""
    _raises(lambda: h.mesh_regions_sync(1.0, 20, 0.0), -1)                              # table off
    _raises(lambda: h.mesh_regions(), -1)
    pts, cam = world_scan(0, 40000, cfg)
    h.mesh_scan(pts, cam, frame_idx=0, fetch=False)
    _raises(lambda: h.mesh_regions_enable(), -1)                                         # after the first job
    assert h.mesh_regions_error()
    h.close()
    h = make_hip(hip_lib, cfg)
    h.mesh_regions_enable()
    _raises(lambda: h.mesh_regions_fetch(0, 0), -1)                                      # nothing synchronised yet
    h.mesh_scan(pts, cam, frame_idx=0, fetch=False)
    n = len(h.mesh_regions())
    assert n > 1
    f = hip_lib.immesh_mesh_regions; f.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]; f.restype = C.c_int
    small = np.zeros(1, capi.REGION_DTYPE); got = C.c_int32(0)
    assert f(h.ctx, small.ctypes.data_as(C.c_void_p), 1, C.byref(got)) == -4 and got.value == n and h.mesh_regions_error()
    _raises(lambda: h.mesh_regions_sync(1.0, 10, 0.0), -1)                               # only the reference's k = 20
    _raises(lambda: h.mesh_regions_sync(1.0, 20, 3.0 * 1.25 * cfg.mesh_voxel), -1)      # beyond the reach of the 20-NN pull
    _raises(lambda: h.region_keys(np.zeros((3, 3), np.float32), np.array([[0, 1, 3]], np.int32)), -1)
    assert len(h.mesh_regions_sync(1.0, 20, 0.0)["regions"]) == n                        # the failed calls took nothing
    h.close()
    sh = make_hip(hip_lib, capi.avia_config(mesh_region=2.0, shard_world=2, shard_rank=0, shard_mesh=1, **CAPS))
    _raises(lambda: sh.mesh_regions_enable(), -1)                                        # sharded mesher: out of scope
    sh.close()
