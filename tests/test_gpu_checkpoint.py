"""Checkpoints on the device (include/immesh_checkpoint.h): a context that loads a checkpoint goes on exactly as the saving one -- poses, plane
table, mesh lists, counters, bit for bit --, the region table and the colour state survive, the file follows content and not capacity, and every
refusal names its field and leaves the context as created."""
import os
import shutil

import numpy as np
import pytest

import checkpoint_checker as ck
from immesh_amd import capi, synth
from conftest import make_hip

pytestmark = pytest.mark.gpu
CAPS = dict(cap_root_voxels=1 << 16, cap_scan_points=200000, cap_vertices=1 << 18, cap_triangles=1 << 20)
MESH_KEYS = ("new_vtx", "tri_add", "flip_add", "tri_rem", "tri_upd", "flip_upd", "smooth_ids", "smooth_xyz")
N_SCANS, SAVE_AT = 8, 4


def _bytes(a):
    return np.ascontiguousarray(a).tobytes()


@pytest.fixture(scope="module")
def scans():
    """the stream of test_gpu_mesher.py::test_process_scan_full_pipeline, eight scans long: (down-sampled, raw, R, t) per scan"""
    cfg = capi.avia_config(**CAPS)
    extT = np.array(list(cfg.extT))
    out = []
    for k in range(N_SCANS + 1):
        R, t = synth.trajectory_pose(k)
        raw = synth.livox_scan(k, R, t, n_pts=30000, extT=extT)
        out.append((np.ascontiguousarray(synth.voxel_grid_downsample(raw, 0.4)), np.ascontiguousarray(raw), R, t))
    return out


def _start(hip_lib, scans, build=True, **over):
    h = make_hip(hip_lib, capi.avia_config(**dict(CAPS, **over)))
    st = capi.make_state(R=scans[0][2], t=scans[0][3])
    if build:
        h.map_build(np.ascontiguousarray(scans[0][1][:, :3]), st)
    st[12:15] = [1.0, 0, 0]; st[15:18] = [0, 0, np.deg2rad(2.0)]
    return h, st


def _run(h, st, scans, ks, do_mesh, fetch=True):
    """scans ks through immesh_process_scan -> (state, [(348-double state, n_iter, n_match, mesh lists or None) per scan])"""
    rec = []
    for k in ks:
        prior = synth.forward_without_imu(st)
        st, info = h.process_scan(scans[k][0], scans[k][1], prior, prior, frame_idx=k, do_mesh=do_mesh)
        lists = None
        if fetch:
            if do_mesh == 2:
                h.mesh_wait()
            lists = h.mesh_fetch()
        rec.append((st.copy(), info["n_iter"], info["n_match"], lists))
    return st, rec


def _planes(h):
    """the plane table, every record bit for bit.  immesh_dump_planes appends its records through an atomic counter, so their order is the order in
    which wavefronts happened to run -- it differs between two dumps of one context; (key, layer, path) names a node, and sorts the table"""
    p = h.dump_planes()
    order = np.lexsort((p["path"], p["layer"], p["key"][:, 2], p["key"][:, 1], p["key"][:, 0]))
    return p[order].tobytes()


def _final(h):
    n = h.counters()["n_vertices"]
    vtx, faces = h.mesh_export(1.0, 20)
    return {"counters": h.counters(), "planes": _planes(h), "export": (_bytes(vtx), _bytes(faces)),
            "smooth": _bytes(h.smooth_pts(np.arange(n, dtype=np.int32)))}


def _same_scans(a, b, tag):
    assert len(a) == len(b)
    for k, ((s1, i1, n1, m1), (s2, i2, n2, m2)) in enumerate(zip(a, b)):
        np.testing.assert_array_equal(s1, s2, err_msg=f"{tag}: state, scan {k}")
        assert (i1, n1) == (i2, n2), (tag, k)
        for key in MESH_KEYS:
            np.testing.assert_array_equal(m1[key], m2[key], err_msg=f"{tag}: {key}, scan {k}")


def _same_final(a, b, tag, planes=True):
    for key in a["counters"]:
        assert a["counters"][key] == b["counters"][key], (tag, key)
    if planes:
        assert a["planes"] == b["planes"], tag
    assert a["export"] == b["export"], tag
    assert a["smooth"] == b["smooth"], tag   # (bytes: NaNs included)


@pytest.fixture(scope="module")
def run_c(hip_lib, scans):
    """the uninterrupted run C (synchronous meshing), computed once: every scan's record and the final state"""
    h, st = _start(hip_lib, scans)
    _, rec = _run(h, st, scans, range(1, N_SCANS + 1), 1)
    fin = _final(h)
    h.close()
    return rec, fin


@pytest.fixture(scope="module")
def saved(hip_lib, scans, tmp_path_factory):
    """a checkpoint of the stream after scan SAVE_AT (synchronous meshing) -> (path, info, the state to go on from)"""
    h, st = _start(hip_lib, scans)
    st, _ = _run(h, st, scans, range(1, SAVE_AT + 1), 1)
    path = str(tmp_path_factory.mktemp("ckpt") / "map.ckpt")
    info = h.checkpoint_save(path)
    h.close()
    return path, info, st


@pytest.mark.parametrize("do_mesh", [1, 2])
def test_resume_equals_uninterrupted(hip_lib, scans, run_c, tmp_path, do_mesh):
    rec_c, fin_c = run_c
    if do_mesh == 2:   # (C of the asynchronous leg: its own run; the synchronous one is the shared reference)
        hc, st = _start(hip_lib, scans)
        _, rec_c2 = _run(hc, st, scans, range(1, N_SCANS + 1), 2)
        fin_c2 = _final(hc)
        hc.close()
        _same_scans(rec_c, rec_c2, "C asynchronous vs synchronous")
        _same_final(fin_c, fin_c2, "C asynchronous vs synchronous")
    # ---- A: scans 1..4, save (asynchronous: without waiting for the mesher -- the save drains), save again, go on
    a, st = _start(hip_lib, scans)
    st_a, _ = _run(a, st, scans, range(1, SAVE_AT + 1), do_mesh, fetch=do_mesh == 1)
    ca = a.counters() if do_mesh == 1 else None
    p1, p2, p3 = (str(tmp_path / n) for n in ("a1.ckpt", "a2.ckpt", "b.ckpt"))
    info = a.checkpoint_save(p1)
    if ca is not None:
        assert ca["t_rem"] > 0 and ca["n_refits"] > 0, ca    # dead pool entries, removal stamps and refits are in play at the save point
    assert info["n_triangles_pool"] > info["n_triangles_live"] > 0 and info["scans_meshed"] == SAVE_AT and info["map_updates"] == SAVE_AT
    a.checkpoint_save(p2)
    raw1 = open(p1, "rb").read()
    assert raw1 == open(p2, "rb").read(), "two saves of one state differ"
    assert not os.path.exists(p1 + ".tmp")
    ck.read(p1)                                               # the numpy reader: every section's checksum, the header's
    assert info["file_bytes"] == len(raw1) and info["ms"][3] > 0
    # ---- B: fresh, load, save straight away (A's file), go on
    b, _ = _start(hip_lib, scans, build=False)
    linfo = b.checkpoint_load(p1)
    assert {k: v for k, v in linfo.items() if k not in ("ms", "cfg")} == {k: v for k, v in info.items() if k not in ("ms", "cfg")}
    b.checkpoint_save(p3)
    assert open(p3, "rb").read() == raw1, "a loaded context saves another file than the one it loaded"
    _, rec_a = _run(a, st_a.copy(), scans, range(SAVE_AT + 1, N_SCANS + 1), do_mesh)
    _, rec_b = _run(b, st_a.copy(), scans, range(SAVE_AT + 1, N_SCANS + 1), do_mesh)
    _same_scans(rec_c[SAVE_AT:], rec_a, "C vs A")
    _same_scans(rec_c[SAVE_AT:], rec_b, "C vs B")
    fin_a, fin_b = _final(a), _final(b)
    _same_final(fin_c, fin_a, "C vs A")
    _same_final(fin_c, fin_b, "C vs B")
    a.close(); b.close()


def test_regions_and_colour_survive(hip_lib, tmp_path):
    from test_gpu_colour import _image
    from test_gpu_regions import CAPS as RG_CAPS
    from test_regions_cpu import world_scan
    cfg = capi.avia_config(mesh_region=2.0, **RG_CAPS)
    world = [world_scan(k, 40000, cfg) for k in range(6)]

    def image(h, k):
        im, px = _image(h, k, big=True, pos=list(world[k][1]))
        return im, px

    def feed(h, ks):
        out = []
        for k in ks:
            h.mesh_scan(world[k][0], world[k][1], frame_idx=k, fetch=False)
            if k in (1, 3, 5):
                im, px = image(h, k)
                out.append(h.colour_image(im, capi.COLOUR_PLAIN, capi.COLOUR_SET_ALL))
            if k == 2:
                h.mesh_regions_sync(1.0, 20, 0.0, fetch=False)
        return out

    def colours(h):
        rgb, st = h.colour_fetch()
        return _bytes(rgb), _bytes(st)

    a = make_hip(hip_lib, cfg)
    a.mesh_regions_enable()
    stats = feed(a, range(5))
    assert len(stats) == 2 and all(s["n_hit"] > 0 for s in stats), stats     # two images, both colour vertices
    path = str(tmp_path / "rg.ckpt")
    info = a.checkpoint_save(path)
    assert info["has_regions"] == 1 and info["has_colour"] == 1 and info["n_regions"] >= 2
    ra = a.mesh_regions()
    print("regions at the save point:", len(ra), "dirty:", int(ra["dirty"].sum()), "image hits:", [s["n_hit"] for s in stats])
    assert len(ra) == info["n_regions"] and ra["dirty"].any()                  # dirty flags are part of the state
    b = make_hip(hip_lib, cfg)                                                 # the table is off: load turns it on
    b.colourer()
    linfo = b.checkpoint_load(path)
    assert linfo["has_regions"] == 1 and linfo["has_colour"] == 1
    assert b.mesh_regions().tobytes() == ra.tobytes()
    assert colours(b) == colours(a)
    for h in (a, b):
        feed(h, [5])
    sa, sb = a.mesh_regions_sync(1.0, 20, 0.0), b.mesh_regions_sync(1.0, 20, 0.0)
    assert len(sa["tri"]) > 0
    for key in ("regions", "tri", "flip", "xyz"):
        assert _bytes(sa[key]) == _bytes(sb[key]), key
    assert a.mesh_regions().tobytes() == b.mesh_regions().tobytes()
    assert colours(a) == colours(b)
    # without a colourer the section is skipped, and info says so
    c = make_hip(hip_lib, cfg)
    linfo = c.checkpoint_load(path, colourer=False)
    assert linfo["has_regions"] == 1 and linfo["has_colour"] == 0
    assert c.mesh_regions().tobytes() == ra.tobytes()
    # a context with the table on refuses a file without the section
    d = make_hip(hip_lib, cfg)
    d.mesh_scan(world[0][0], world[0][1], frame_idx=0, fetch=False)
    plain = str(tmp_path / "plain.ckpt")
    assert d.checkpoint_save(plain, colourer=False)["has_regions"] == 0
    e = make_hip(hip_lib, cfg)
    e.mesh_regions_enable()
    with pytest.raises(capi.CheckpointError, match="region") as err:
        e.checkpoint_load(plain)
    assert err.value.rc == capi.E_INVAL
    for h in (a, b, c, d, e):
        h.close()


def test_deep_octree_state(hip_lib, tmp_path):
    """velodyne.yaml's deep octrees (the stream of test_register_and_update_stream_parity_kitti) fill the extension tables and the leaf chunks;
    the free list is filled by test_update_state_machine_freeze's 12 x 400 points of one wall patch, fed as further updates of the same map."""
    cfg = capi.velodyne_config(cap_root_voxels=1 << 14, cap_scan_points=200000)
    clouds = []
    for k in range(6):
        R, t = synth.trajectory_pose(k)
        raw = synth.hdl64_scan(k, R, t, n_az=700)
        clouds.append((R, t, np.ascontiguousarray(raw[:, :3]) if k == 0 else synth.voxel_grid_downsample(raw, 0.5)))
    rng = np.random.default_rng(11)
    patch = [np.stack([rng.uniform(5.0, 6.0, 400), rng.uniform(-0.5, 0.5, 400), -1.3 + rng.normal(0, 0.004, 400)], axis=1).astype(np.float32) for _ in range(12)]

    def start():
        h = make_hip(hip_lib, cfg)
        st = capi.make_state(R=clouds[0][0], t=clouds[0][1])
        h.map_build(clouds[0][2], st)
        st[12:15] = [1.0, 0, 0]; st[15:18] = [0, 0, np.deg2rad(2.0)]
        return h, st

    def go(h, st, ks):
        poses = []
        for k in ks:
            prior = synth.forward_without_imu(st)
            st, info = h.register(clouds[k][2], prior, prior)
            h.map_update(clouds[k][2], st)
            poses.append((st.copy(), info["n_iter"], info["n_match"]))
        return st, poses

    def freeze(h):
        for p in patch:
            h.map_update(p, capi.make_state())

    c, st = start()
    st, _ = go(c, st, range(1, 4)); freeze(c)
    _, want = go(c, st, range(4, 6))
    a, st = start()
    st, _ = go(a, st, range(1, 4)); freeze(a)
    path = str(tmp_path / "deep.ckpt")
    info = a.checkpoint_save(path)
    _, secs = a.checkpoint_probe(path)
    by = {s["name"]: s for s in secs}
    print("deep octree checkpoint:", {k: info[k] for k in ("n_nodes", "n_point_chunks", "n_free_chunks", "n_ext_tables", "n_leaf_chunks", "map_updates")})
    assert info["n_ext_tables"] > 0 and info["n_leaf_chunks"] > 0 and info["n_free_chunks"] > 0
    assert by["reg.ext"]["bytes"] > 0 and by["reg.leaf"]["bytes"] > 0 and by["reg.free_ready"]["bytes"] + by["reg.free_pending"]["bytes"] > 0
    assert info["map_updates"] == 3 + 12
    b = make_hip(hip_lib, cfg)
    b.checkpoint_load(path)
    assert _planes(b) == _planes(a)
    _, got_a = go(a, st.copy(), range(4, 6))
    _, got_b = go(b, st.copy(), range(4, 6))
    for (s0, i0, n0), (s1, i1, n1), (s2, i2, n2) in zip(want, got_a, got_b):
        np.testing.assert_array_equal(s0, s1); np.testing.assert_array_equal(s0, s2)
        assert (i0, n0) == (i1, n1) == (i2, n2)
    pc = _planes(c)
    assert _planes(a) == pc and _planes(b) == pc
    ca, cb, cc = a.counters(), b.counters(), c.counters()
    for key in cc:
        assert ca[key] == cc[key] == cb[key], key
    for h in (a, b, c):
        h.close()


def test_size_follows_content(hip_lib, scans, saved, tmp_path):
    """Two halves.  (1) The saved map moved into a context whose pools are four times larger (the table sizes, which must match, stay) and saved
    from there: the file differs from the original in the header's cfg (and the header checksum over it) and nowhere else.  (2) The same four scans
    run in a context with all four capacities x 4: every section has the same size and record count -- the triangle HASH's too -- except the
    five arrays of the triangle POOL (mesh.t_*), whose length is not a function of the scans: the pool holds more entries than the hash points to
    (57728 against 45978 in one run), and how many more differs from run to run of one configuration (measured on this stream: 57656 and 57923 in
    two runs with the capacities above; 57348 .. 58044 over five runs with other capacities; live triangles, vertices, voxels, nodes, chunks,
    adjacency chunks equal in all).  Those five sections are held to their own context's count.  The table sections hold (slot index, entry) pairs, and a larger table spreads the same keys
    over other slots: their payload -- with it the header's masks and the checksums -- follows the table size."""
    path, info, _ = saved
    raw0 = open(path, "rb").read()
    nodes = 4 * ((1 << 16) + (1 << 15))
    m, _ = _start(hip_lib, scans, build=False, cap_nodes=nodes, cap_point_chunks=2 * nodes)
    m.checkpoint_load(path)
    moved = str(tmp_path / "moved.ckpt")
    m.checkpoint_save(moved)
    m.close()
    raw1 = open(moved, "rb").read()
    h0, h1 = ck.read(path)[0], ck.read(moved)[0]
    assert len(raw0) == len(raw1) and raw0[ck.HEADER_DTYPE.itemsize:] == raw1[ck.HEADER_DTYPE.itemsize:], "section table or payload differ"
    for name in h0.dtype.names:
        assert (_bytes(h0[name]) == _bytes(h1[name])) == (name not in ("cfg", "header_checksum")), name
    c0, c1 = capi.Config.from_buffer_copy(h0["cfg"].tobytes()), capi.Config.from_buffer_copy(h1["cfg"].tobytes())
    assert (c1.cap_nodes, c1.cap_point_chunks) == (nodes, 2 * nodes) and (c0.cap_nodes, c0.cap_point_chunks) == (0, 0)
    # ---- (2)
    h, st = _start(hip_lib, scans, **{k: 4 * v for k, v in CAPS.items()})
    _run(h, st, scans, range(1, SAVE_AT + 1), 1)
    big = str(tmp_path / "big.ckpt")
    binfo = h.checkpoint_save(big)
    h.close()
    (_, s1), (_, s2) = capi.checkpoint_probe(hip_lib, path), capi.checkpoint_probe(hip_lib, big)
    assert [s["name"] for s in s1] == [s["name"] for s in s2]
    pool = {"mesh.t_v": 12, "mesh.t_word": 8, "mesh.t_live": 4, "mesh.t_rem_seq": 4, "mesh.t_flip": 1}
    print("triangle pool entries:", info["n_triangles_pool"], binfo["n_triangles_pool"], "live:", info["n_triangles_live"], binfo["n_triangles_live"],
          "hash entries:", [s["records"] for s in s1 + s2 if s["name"] == "mesh.thash.slot"])
    for a, b in zip(s1, s2):
        if a["name"] in pool:
            for s, i in ((a, info), (b, binfo)):
                assert (s["records"], s["bytes"]) == (i["n_triangles_pool"], pool[a["name"]] * i["n_triangles_pool"]), a["name"]
        else:
            assert (a["bytes"], a["records"]) == (b["bytes"], b["records"]), a["name"]
    assert binfo["file_bytes"] == os.path.getsize(big)
    for key in info:
        if key not in ("cfg", "ms", "n_triangles_pool", "file_bytes"):
            assert info[key] == binfo[key], key
    h2 = ck.read(big)[0]
    assert list(h2["masks"]) == [4 * (int(v) + 1) - 1 for v in h0["masks"]]
    assert _bytes(h2["rec"]) == _bytes(h0["rec"])


def test_larger_pools_and_refusals(hip_lib, scans, run_c, saved, tmp_path):
    rec_c, fin_c = run_c
    path, info, st4 = saved
    rest = range(SAVE_AT + 1, N_SCANS + 1)

    def refused(h, p, rc, pattern):
        with pytest.raises(capi.CheckpointError, match=pattern) as e:
            h.checkpoint_load(p)
        assert e.value.rc == rc, (e.value.rc, e.value.msg)

    # ---- larger pools (same table sizes): the map moves in and goes on to C's bits
    nodes = 2 * ((1 << 16) + (1 << 15))
    b, _ = _start(hip_lib, scans, build=False, cap_nodes=nodes, cap_point_chunks=4 * nodes)
    b.checkpoint_load(path)
    _, rec_b = _run(b, st4.copy(), scans, rest, 1)
    _same_scans(rec_c[SAVE_AT:], rec_b, "C vs larger pools")
    _same_final(fin_c, _final(b), "C vs larger pools")
    b.close()
    # ---- files a standard context refuses: another voxel_size (the header edited, its checksum made right again), a truncated copy
    header, table, sections = ck.read(path)
    other, cut = str(tmp_path / "voxel_size.ckpt"), str(tmp_path / "cut.ckpt")
    cfg2 = capi.Config.from_buffer_copy(header["cfg"].tobytes())
    cfg2.voxel_size = 0.6
    h2 = header.copy(); h2["cfg"] = np.void(bytes(cfg2)); h2["header_checksum"] = ck.header_checksum(h2, table)
    shutil.copyfile(path, other)
    with open(other, "r+b") as f:
        f.write(h2.tobytes())
    with open(cut, "wb") as f:
        f.write(open(path, "rb").read()[:-4096])
    d, st = _start(hip_lib, scans, build=False)
    refused(d, other, capi.E_INVAL, "voxel_size")
    refused(d, cut, capi.E_FORMAT, "file length")
    refused(d, str(tmp_path / "missing.ckpt"), capi.E_IO, "cannot open")
    d.map_build(np.ascontiguousarray(scans[0][1][:, :3]), capi.make_state(R=scans[0][2], t=scans[0][3]))
    _, rec_d = _run(d, st, scans, range(1, N_SCANS + 1), 1)
    _same_scans(rec_c, rec_d, "C vs a context that refused two files")
    _same_final(fin_c, _final(d), "C vs a context that refused two files")
    refused(d, path, capi.E_INVAL, "no map build, update, scan or mesh job")      # a used context
    # save into a directory that does not exist: IMMESH_E_IO, neither the file nor its .tmp
    gone = str(tmp_path / "no_such_dir" / "x.ckpt")
    with pytest.raises(capi.CheckpointError) as e:
        d.checkpoint_save(gone)
    assert e.value.rc == capi.E_IO and not os.path.exists(gone) and not os.path.exists(gone + ".tmp") and not os.path.exists(os.path.dirname(gone))
    d.close()
    # ---- another table size: cap_root_voxels doubled.  Untouched: the whole stream gives C's bits
    e2, st = _start(hip_lib, scans, build=False, cap_root_voxels=1 << 17)
    refused(e2, path, capi.E_INVAL, "cap_root_voxels")
    e2.map_build(np.ascontiguousarray(scans[0][1][:, :3]), capi.make_state(R=scans[0][2], t=scans[0][3]))
    _, rec_e = _run(e2, st, scans, range(1, N_SCANS + 1), 1)
    _same_scans(rec_c, rec_e, "C vs a context with another hash size")
    _same_final(fin_c, _final(e2), "C vs a context with another hash size")
    e2.close()
    # ---- a node pool one below the file's count.  Such a context cannot hold scans 4..8 either: untouched = it runs scans 1..3 to C's bits
    f2, st = _start(hip_lib, scans, build=False, cap_nodes=info["n_nodes"] - 1)
    refused(f2, path, capi.E_CAPACITY, "cap_nodes")
    f2.map_build(np.ascontiguousarray(scans[0][1][:, :3]), capi.make_state(R=scans[0][2], t=scans[0][3]))
    _, rec_f = _run(f2, st, scans, range(1, SAVE_AT), 1)
    _same_scans(rec_c[:SAVE_AT - 1], rec_f, "C vs a context with a small node pool")
    f2.close()
    # ---- a sharded context neither loads nor saves
    g = make_hip(hip_lib, capi.avia_config(shard_world=2, shard_rank=0, **CAPS))
    refused(g, path, capi.E_INVAL, "sharded")
    with pytest.raises(capi.CheckpointError, match="sharded") as e:
        g.checkpoint_save(str(tmp_path / "shard.ckpt"))
    assert e.value.rc == capi.E_INVAL and not os.path.exists(str(tmp_path / "shard.ckpt"))
    g.close()
    # ---- one payload byte flipped inside a dense section (the vertex positions: no table a kernel would walk): found after placing
    by = {t["name"].decode(): t for t in table}
    flipped = str(tmp_path / "flipped.ckpt")
    raw = bytearray(open(path, "rb").read())
    raw[int(by["mesh.v_pos"]["offset"]) + int(by["mesh.v_pos"]["bytes"]) // 2] ^= 0x10
    open(flipped, "wb").write(bytes(raw))
    capi.checkpoint_probe(hip_lib, flipped)          # header and table are intact: the probe accepts it
    k, _ = _start(hip_lib, scans, build=False)
    refused(k, flipped, capi.E_FORMAT, "checksum mismatch in section mesh.v_pos")
    k.close()                                        # (nothing else may be run on it)
