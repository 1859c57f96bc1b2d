"""Cost of the device-side region buckets (include/immesh_regions.h) on the bench's workload: the registration map pre-built from bench.py's survey,
the MESH map pre-seeded from its corridor survey (bench's own helpers, imported; bench.py itself is not changed), then the asynchronous full-pipeline
loop (immesh_process_scan, IMMESH_MESH_ASYNC) on GPU-generated scans.  Variants, each in a child process of its own, alternated (the order rotates from
one repetition to the next) and repeated:

    parent   another build of the library (--parent-lib, through IMMESH_HIP_LIBRARY), regions unknown to it     [skipped without --parent-lib]
    off      this tree's library, region table never enabled -- meant to be the parent's launch sequence
    on       region table enabled: one marking launch per mesh job

Per child: scans/s of the timed loop (wall clock, ending in immesh_mesh_wait + a device synchronise).  The `on` child then continues the stream and
every --refresh-every scans times one refresh (immesh_mesh_regions_sync + _fetch, wall clock ending in the fetch's synchronise) beside what the
parent offers for the purpose (immesh_mesh_export + _export_fetch of the whole mesh), and finally runs a few scans under the library's own profiler
for the device time of the marking launch.  One JSON object on stdout, and in --out when given.

    python tools/regions_bench.py [--parent-lib PATH] [--reps 5] [--steps 300] [--out profiles/regions_bench.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(args):
    import bench  # noqa: E402  (seeding helpers: build_big_map, corridor_cloud, livox_scan_torch)
    from immesh_amd import capi, synth
    capi.one_hip_runtime()          # before torch: one HIP runtime in the process, as in bench.py
    import torch
    hip = capi.load_hip_library()
    dev = torch.device("cuda", 0)
    on = args.child == "on"
    cfg = capi.avia_config(cap_root_voxels=int(args.map_voxels * 1.3) + (1 << 16), cap_scan_points=2_500_000, cap_vertices=1 << 24, cap_triangles=1 << 25)
    h = capi.HotPath(hip, cfg, "immesh_")
    bytes_before = h.device_bytes()
    if on:
        h.mesh_regions_enable()
    n_refresh_scans = args.refresh_scans if on else 0
    n_prof = args.profile_scans if on else 0
    n_total = 1 + args.warmup + args.steps + args.refresh_scans + args.profile_scans   # (the same stream and survey corridor for every variant)
    extT = np.array(list(cfg.extT))
    d_raw, d_down, n_ds = [], [], []
    for k in range(n_total):
        Rk, tk = synth.trajectory_pose(k)
        r = bench.livox_scan_torch(torch, dev, k, Rk, tk, args.pts, extT)
        dn, _ = h.downsample(r.data_ptr(), 0.4, n=r.shape[0], stride=4, to_host=True)
        d_raw.append(r); d_down.append(torch.from_numpy(dn).to(dev)); n_ds.append(len(dn))
    side = float(np.sqrt(args.map_voxels / 8.8)) + 40.0
    bench.build_big_map(h, cfg, torch, dev, args.map_voxels, side)
    P = bench.corridor_cloud(torch, dev, n_total)
    cam0 = synth.trajectory_pose(0)[1] + np.array([0.0, 0.0, 1.0])
    pkg = int(cfg.mesh_append_budget)
    for a in range(0, P.shape[0], pkg):
        ch = P[a:a + pkg].contiguous()
        h.mesh_scan(ch.data_ptr(), cam0, frame_idx=0, n=ch.shape[0], fetch=False)
    cs = h.counters()
    seed = {"cloud_points": int(P.shape[0]), "vertices": int(cs["n_vertices"]), "triangles_live": int(cs["n_triangles_live"])}
    del P
    R0, t0 = synth.trajectory_pose(0)
    st = capi.make_state(R=R0, t=t0)
    st[12:15] = [1.0, 0, 0]; st[15:18] = [0, 0, np.deg2rad(2.0)]
    h.process_scan(d_down[0].data_ptr(), d_raw[0].data_ptr(), st, st, frame_idx=0, do_mesh=1, n_ds=n_ds[0], n_raw=d_raw[0].shape[0])

    def run(k, state, mode=2):
        prior = capi.forward_without_imu_native(hip, state)
        return h.process_scan(d_down[k].data_ptr(), d_raw[k].data_ptr(), prior, prior, frame_idx=k, do_mesh=mode, n_ds=n_ds[k], n_raw=d_raw[k].shape[0])[0]

    k = 1
    if on:
        h.mesh_regions_sync(1.0, 20, 0.0, fetch=False)     # the survey's regions are the viewer's first full upload, not a refresh
    for _ in range(args.warmup):
        st = run(k, st); k += 1
    h.mesh_wait(); torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(args.steps):
        st = run(k, st); k += 1
    h.mesh_wait(); torch.cuda.synchronize()
    dt = time.perf_counter() - t
    out = {"variant": args.child, "device": torch.cuda.get_device_name(0), "library": os.path.relpath(capi.hip_library_path(), ROOT), "scans_per_s": round(args.steps / dt, 1), "steps": args.steps, "survey_mesh": seed,
           "device_bytes_before_enable": int(bytes_before), "device_bytes": int(h.device_bytes())}
    if on:
        # ---- refreshes: every `refresh_every` scans one sync + fetch, and for comparison one whole-mesh export + fetch (what the parent offers)
        import ctypes as C
        exp = hip.immesh_mesh_export; exp.argtypes = [C.c_void_p, C.c_double, C.c_int32, C.c_void_p, C.c_void_p]; exp.restype = C.c_int
        ref_ms, exp_ms, moved = [], [], []
        for i in range(n_refresh_scans):
            st = run(k, st); k += 1
            if (i + 1) % args.refresh_every:
                continue
            h.mesh_wait()
            t = time.perf_counter()
            res = h.mesh_regions_sync(1.0, 20, 0.0)
            ref_ms.append(1e3 * (time.perf_counter() - t))
            n_reg, live = len(h.mesh_regions()), h.counters()["n_triangles_live"]
            moved.append({"regions": len(res["regions"]), "regions_total": n_reg, "triangles": len(res["tri"]), "triangles_live": int(live)})
            t = time.perf_counter()
            vtx, faces = h.mesh_export(1.0, 20)
            exp_ms.append(1e3 * (time.perf_counter() - t))
            del vtx, faces, res
        out["refresh"] = {"every_scans": args.refresh_every, "sync_plus_fetch_ms": [round(x, 3) for x in ref_ms], "whole_mesh_export_plus_fetch_ms": [round(x, 3) for x in exp_ms],
                          "moved": moved}
        # ---- the marking launch under the library's own profiler (HIP events around each kernel; the mesher runs un-captured and one job at a time)
        h.mesh_wait()
        h.profile_enable(True)
        h.profile_read(reset=True)
        for _ in range(n_prof):
            st = run(k, st, mode=1); k += 1
        prof = h.profile_read()
        h.profile_enable(False)
        out["marking_launch"] = {name: {"launches": int(v["launches"]), "us_per_launch": round(1e3 * v["total_ms"] / max(1, v["launches"]), 2)}
                                 for name, v in prof.items() if name.startswith("regions_")}
        mesher = {name: v for name, v in prof.items() if name.startswith("mesh_") and v["launches"]}
        out["mesher_kernels_us_per_scan_under_profiler"] = round(1e3 * sum(v["total_ms"] for v in mesher.values()) / max(1, n_prof), 1)
    h.close()
    print("REGIONS_BENCH_CHILD " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default="", help="(internal) run one variant in this process")
    ap.add_argument("--parent-lib", default="", help="libimmesh_hip.so built from the parent commit")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=300, help="timed scans per child (a window of tens of milliseconds measures the scheduler)")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--pts", type=int, default=100000)
    ap.add_argument("--map-voxels", type=float, default=10e6)
    ap.add_argument("--refresh-scans", type=int, default=40)
    ap.add_argument("--refresh-every", type=int, default=10)
    ap.add_argument("--profile-scans", type=int, default=10)
    ap.add_argument("--child-timeout", type=float, default=280.0)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.child:
        return child(args)
    variants = (["parent"] if args.parent_lib else []) + ["off", "on"]
    runs = {v: [] for v in variants}
    for rep in range(args.reps):
        for v in variants[rep % len(variants):] + variants[:rep % len(variants)]:   # alternated, the order rotated: drift and position in the sequence hit every variant alike
            env = dict(os.environ)
            env.pop("IMMESH_HIP_LIBRARY", None)
            if v == "parent":
                env["IMMESH_HIP_LIBRARY"] = os.path.abspath(args.parent_lib)
            cmd = [sys.executable, os.path.abspath(__file__), "--child", v] + [f"--{k.replace('_', '-')}={getattr(args, k)}" for k in
                   ("steps", "warmup", "pts", "map_voxels", "refresh_scans", "refresh_every", "profile_scans")]
            p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=args.child_timeout)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("REGIONS_BENCH_CHILD ")]
            if p.returncode != 0 or not line:
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                raise SystemExit(f"variant {v} (repetition {rep}) failed with status {p.returncode}: nothing more is started")
            runs[v].append(json.loads(line[-1][len("REGIONS_BENCH_CHILD "):]))
            print(f"[regions_bench] rep {rep} {v}: {runs[v][-1]['scans_per_s']} scans/s", file=sys.stderr, flush=True)
    summary = {}
    for v in variants:
        r = np.array([x["scans_per_s"] for x in runs[v]])
        summary[v] = {"scans_per_s": r.tolist(), "median": round(float(np.median(r)), 1), "min": float(r.min()), "max": float(r.max()),
                      "spread_percent_of_median": round(100.0 * float(r.max() - r.min()) / float(np.median(r)), 2)}
    on_runs = runs["on"]
    ref = [x for r in on_runs for x in r["refresh"]["sync_plus_fetch_ms"]]
    exp = [x for r in on_runs for x in r["refresh"]["whole_mesh_export_plus_fetch_ms"]]
    moved = [m for r in on_runs for m in r["refresh"]["moved"]]
    out = {"metric": "device-side region buckets on the bench's workload (asynchronous full pipeline, survey mesh)", "device": on_runs[0]["device"],
           "reps": args.reps, "steps": args.steps, "warmup": args.warmup, "pts": args.pts, "map_voxels": args.map_voxels,
           "scans_per_s": summary,
           "refresh": {"every_scans": args.refresh_every, "n": len(ref),
                       "sync_plus_fetch_ms_median": round(float(np.median(ref)), 3) if ref else None, "sync_plus_fetch_ms_max": round(float(np.max(ref)), 3) if ref else None,
                       "whole_mesh_export_plus_fetch_ms_median": round(float(np.median(exp)), 3) if exp else None,
                       "regions_moved_share_median": round(float(np.median([m["regions"] / max(1, m["regions_total"]) for m in moved])), 4) if moved else None,
                       "triangles_moved_share_median": round(float(np.median([m["triangles"] / max(1, m["triangles_live"]) for m in moved])), 4) if moved else None,
                       "samples": moved[:8]},
           "marking_launch": [r["marking_launch"] for r in on_runs], "mesher_kernels_us_per_scan_under_profiler": [r["mesher_kernels_us_per_scan_under_profiler"] for r in on_runs],
           "survey_mesh": on_runs[0]["survey_mesh"], "device_bytes_of_the_table": on_runs[0]["device_bytes"] - on_runs[0]["device_bytes_before_enable"],
           "timing": "scans/s: wall clock of `steps` immesh_process_scan(IMMESH_MESH_ASYNC) calls ending in immesh_mesh_wait + a device synchronise; refresh: wall "
                     "clock of immesh_mesh_regions_sync + _fetch (ends in the fetch's stream synchronise) after immesh_mesh_wait, beside immesh_mesh_export + "
                     "_export_fetch at the same moment; marking launch: HIP events of the library's profiler (immesh_profile_read), synchronous meshing"}
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as fp:
            json.dump(out, fp, indent=1)


if __name__ == "__main__":
    main()
