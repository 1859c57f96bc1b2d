#!/usr/bin/env python3
"""Timing of immesh_checkpoint_save / _load on one GPU (profiler off) -> profiles/checkpoint_timing.json.

Two workloads: the map of tests/test_gpu_checkpoint.py (map_build + 4 scans), and bench.py's C3 state (the surveyed registration map and the mesh
map pre-seeded from the corridor survey, built by bench.py's own functions; --map-voxels sets its size).  Per workload: medians of --repeats saves
and loads after one warm-up of each, file bytes per section, the four ms fields, the device phase (table pack + checksums; host clock around
launches and the final synchronise) with its algorithmic bytes as a share of 8 TB/s, and the two bounds a save's wall time is to be read against,
measured in the same run: a plain pinned copy of the file's byte count (D2H and H2D) and a plain write / read of that many bytes from pinned
memory on the same file system.  `rebuild_s` is what it takes without checkpoints: building the state from its scans."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from immesh_amd import capi, synth   # noqa: E402

HBM_BYTES_PER_S = 8.0e12
TABLE_ENTRY = {"reg.hash": 16, "mesh.grid": 32, "mesh.vox": 16, "mesh.thash": 4, "rg.hash": 16}


def build_tests_map(hip, torch, dev, args):
    cfg = capi.avia_config(cap_root_voxels=1 << 16, cap_scan_points=200000, cap_vertices=1 << 18, cap_triangles=1 << 20)
    h = capi.HotPath(hip, cfg, "immesh_")
    extT = np.array(list(cfg.extT))
    R0, t0 = synth.trajectory_pose(0)
    scans = []
    for k in range(5):
        R, t = synth.trajectory_pose(k)
        raw = synth.livox_scan(k, R, t, n_pts=30000, extT=extT)
        scans.append((synth.voxel_grid_downsample(raw, 0.4), raw))
    t_build = time.time()
    st = capi.make_state(R=R0, t=t0)
    h.map_build(np.ascontiguousarray(scans[0][1][:, :3]), st)
    st[12:15] = [1.0, 0, 0]; st[15:18] = [0, 0, np.deg2rad(2.0)]
    for k in range(1, 5):
        prior = synth.forward_without_imu(st)
        st, _ = h.process_scan(scans[k][0], scans[k][1], prior, prior, frame_idx=k, do_mesh=1)
    return h, cfg, time.time() - t_build, "map_build + 4 scans of 30000 points (tests/test_gpu_checkpoint.py)"


def build_c3(hip, torch, dev, args):
    import bench
    side = float(np.sqrt(args.map_voxels / 8.8)) + 40.0
    cfg = capi.avia_config(device=0, cap_root_voxels=int(args.map_voxels * 1.3) + (1 << 16), cap_scan_points=2_500_000, cap_vertices=1 << args.mesh_cap_log2,
                           cap_triangles=1 << (args.mesh_cap_log2 + 1))
    h = capi.HotPath(hip, cfg, "immesh_")
    t_build = time.time()
    n_map = bench.build_big_map(h, cfg, torch, dev, args.map_voxels, side)
    P = bench.corridor_cloud(torch, dev, args.corridor_scans)
    cam0 = synth.trajectory_pose(0)[1] + np.array([0.0, 0.0, 1.0])
    pkg = int(cfg.mesh_append_budget)
    for a in range(0, P.shape[0], pkg):
        ch = P[a:a + pkg].contiguous()
        h.mesh_scan(ch.data_ptr(), cam0, frame_idx=0, n=ch.shape[0], fetch=False)
    return h, cfg, time.time() - t_build, f"bench.py's C3 state: survey of {int(n_map)} root voxels + mesh map seeded from the corridor of {args.corridor_scans} scans"


def bounds(torch, dev, nbytes, directory):
    """plain pinned D2H / H2D copy and plain write / read of nbytes (medians of 3)"""
    host = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
    devb = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    out = {}
    for name, (dst, src) in (("d2h_ms", (host, devb)), ("h2d_ms", (devb, host))):
        ts = []
        for _ in range(4):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); dst.copy_(src, non_blocking=True); b.record(); b.synchronize()
            ts.append(a.elapsed_time(b))
        out[name] = statistics.median(ts[1:])
    view = memoryview(host.numpy())
    path = os.path.join(directory, "bound.bin")
    tw, tr = [], []
    for _ in range(3):
        t0 = time.perf_counter()
        fd = os.open(path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
        off = 0
        while off < nbytes:
            off += os.write(fd, view[off:off + (16 << 20)])
        os.fsync(fd); os.close(fd)
        tw.append(1e3 * (time.perf_counter() - t0))
        t0 = time.perf_counter()
        fd = os.open(path, os.O_RDONLY)
        off = 0
        while off < nbytes:
            off += os.readv(fd, [view[off:off + (16 << 20)]])
        os.close(fd)
        tr.append(1e3 * (time.perf_counter() - t0))
    os.unlink(path)
    out["write_fsync_ms"], out["read_ms"] = statistics.median(tw), statistics.median(tr)
    out["read_note"] = "the file had just been written: served from the page cache"
    return out


def run(name, builder, hip, torch, dev, args, directory):
    h, cfg, rebuild_s, what = builder(hip, torch, dev, args)
    path = os.path.join(directory, name + ".ckpt")
    saves, loads = [], []
    for i in range(args.repeats + 1):
        info = h.checkpoint_save(path, colourer=False)
        if i:
            saves.append(info["ms"])
    _, secs = capi.checkpoint_probe(hip, path)
    for i in range(args.repeats + 1):
        b = capi.HotPath(hip, cfg, "immesh_")
        linfo = b.checkpoint_load(path, colourer=False)
        b.close()
        if i:
            loads.append(linfo["ms"])
    h.close()
    med = lambda rows: [round(statistics.median(r[k] for r in rows), 3) for k in range(4)]   # noqa: E731
    nbytes = info["file_bytes"]
    by = {s["name"]: s for s in secs}
    masks = {"reg.hash": 1, "mesh.grid": 1, "mesh.vox": 1, "mesh.thash": 1}
    while masks["reg.hash"] < 2 * (cfg.cap_root_voxels): masks["reg.hash"] <<= 1
    while masks["mesh.grid"] < 2 * cfg.cap_vertices: masks["mesh.grid"] <<= 1
    masks["mesh.vox"] = masks["mesh.grid"]
    while masks["mesh.thash"] < 2 * cfg.cap_triangles: masks["mesh.thash"] <<= 1
    table_bytes = sum(2 * masks[t] * TABLE_ENTRY[t] + by[t + ".slot"]["bytes"] + by[t + ".ent"]["bytes"] for t in masks)   # count + pack read the table, pack writes the records
    algo = table_bytes + sum(s["bytes"] for s in secs)                                                                   # + every section is read once by its checksum
    s_med, l_med = med(saves), med(loads)
    bnd = bounds(torch, dev, nbytes, directory)
    os.unlink(path)
    res = {"workload": what, "file_bytes": nbytes, "sections": {s["name"]: {"bytes": s["bytes"], "records": s["records"]} for s in secs},
           "counts": {k: v for k, v in info.items() if k.startswith("n_") or k in ("scans_meshed", "map_updates")},
           "repeats": args.repeats, "save_ms_median": dict(zip(("device", "copies", "file", "wall"), s_med)),
           "load_ms_median": dict(zip(("device", "copies", "file", "wall"), l_med)),
           "save_device_phase": {"ms": s_med[0], "algorithmic_bytes": int(algo), "share_of_8_TBps": round(algo / (s_med[0] * 1e-3) / HBM_BYTES_PER_S, 4) if s_med[0] > 0 else None,
                                 "note": "host clock around the launches and their synchronise (allocations of the packed buffers included); not HIP events"},
           "bounds": {k: (round(v, 3) if isinstance(v, float) else v) for k, v in bnd.items()},
           "save_wall_over_larger_bound": round(s_med[3] / max(bnd["d2h_ms"], bnd["write_fsync_ms"]), 2),
           "load_wall_over_larger_bound": round(l_med[3] / max(bnd["h2d_ms"], bnd["read_ms"]), 2),
           "rebuild_s": round(rebuild_s, 2)}
    print(json.dumps({name: {k: res[k] for k in ("file_bytes", "save_ms_median", "load_ms_median", "bounds", "rebuild_s")}}), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="tests,c3")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--map-voxels", type=float, default=10e6)
    ap.add_argument("--mesh-cap-log2", type=int, default=24)
    ap.add_argument("--corridor-scans", type=int, default=56, help="length of the stream whose corridor seeds the mesh map (bench.py's default run: 1 + warm-up 5 + 50 steps)")
    ap.add_argument("--dir", default=None, help="directory the checkpoints are written to (default: a temporary directory)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "checkpoint_timing.json"))
    args = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    hip = capi.load_hip_library()
    builders = {"tests": build_tests_map, "c3": build_c3}
    out = {"tool": "tools/checkpoint_bench.py", "device": torch.cuda.get_device_name(0), "argv": sys.argv[1:], "not_measured": [
        "device phase by HIP events (the figure is a host clock around the launches)", "kernel statistics under rocprofv3 --kernel-trace --stats",
        "a load from a cold page cache"]}
    with tempfile.TemporaryDirectory(dir=args.dir) as d:
        out["directory"] = "temporary directory" if args.dir is None else "--dir"
        for name in args.workloads.split(","):
            out[name] = run(name, builders[name], hip, torch, dev, args, d)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
