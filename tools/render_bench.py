"""Render timings on the bench's survey mesh (include/immesh_render.h): the MESH map pre-seeded from bench.py's corridor survey (its own seeding
helper, imported; bench.py itself is not changed), then immesh_render_mesh from LiDAR poses along the stream at 640 x 480 and 1920 x 1080.
Reports medians of the export (immesh_mesh_export, wall clock: it synchronises), rasterize and reinforce (HIP events on the renderer's stream,
immesh_renderer_last_timing) and the whole render_mesh call.  One JSON object on stdout, and in --out when given.

    python tools/render_bench.py [--scans 70] [--reps 5] [--out profiles/render_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (seeding helper: corridor_cloud)
from immesh_amd import capi, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=70, help="stream length whose corridor is surveyed (bench.py --full: 5 + 50 + 15 scans)")
    ap.add_argument("--reps", type=int, default=5, help="renders per pose and size")
    ap.add_argument("--poses", type=int, default=8, help="poses along the stream")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    capi.one_hip_runtime()          # before torch: one HIP runtime in the process, as in bench.py
    import torch
    hip = capi.load_hip_library()
    dev = torch.device("cuda", 0)
    cfg = capi.avia_config(cap_root_voxels=1 << 16, cap_scan_points=200000, cap_vertices=1 << 24, cap_triangles=1 << 25)
    h = capi.HotPath(hip, cfg, "immesh_")
    t0 = time.time()
    P = bench.corridor_cloud(torch, dev, args.scans)
    cam0 = synth.trajectory_pose(0)[1] + np.array([0.0, 0.0, 1.0])
    pkg = int(cfg.mesh_append_budget)
    for a in range(0, P.shape[0], pkg):
        ch = P[a:a + pkg].contiguous()
        h.mesh_scan(ch.data_ptr(), cam0, frame_idx=0, n=ch.shape[0], fetch=False)
    torch.cuda.synchronize()
    cs = h.counters()
    seed = {"cloud_points": int(P.shape[0]), "vertices": int(cs["n_vertices"]), "triangles_live": int(cs["n_triangles_live"]), "seconds": round(time.time() - t0, 1)}
    del P
    print(f"[render_bench] survey mesh: {seed}", file=sys.stderr, flush=True)

    exp = hip.immesh_mesh_export; exp.argtypes = [C.c_void_p, C.c_double, C.c_int32, C.c_void_p, C.c_void_p]; exp.restype = C.c_int
    nv, nf = C.c_int64(0), C.c_int64(0)
    t_exp = []
    for _ in range(args.reps):
        t = time.perf_counter()
        h._check(exp(h.ctx, 1.0, 20, C.byref(nv), C.byref(nf)), "mesh_export")
        t_exp.append(1e3 * (time.perf_counter() - t))
    poses = np.linspace(0, args.scans - 1, args.poses).round().astype(int)
    sizes = {}
    for (w, hgt) in ((640, 480), (1920, 1080)):
        rast, rein, call, cover, npts = [], [], [], [], []
        for k in poses:
            R, t = synth.trajectory_pose(int(k))
            cam = h.camera_from_state(capi.make_state(R=R, t=t), h.default_depth_camera(width=w, height=hgt))
            h.render_mesh(cam, 1.0, 20, want_depth=False, want_face=False)          # first render at this size grows the buffers
            for _ in range(args.reps):
                tc = time.perf_counter()
                depth, _ = h.render_mesh(cam, 1.0, 20, want_depth=True, want_face=False)
                call.append(1e3 * (time.perf_counter() - tc))
                a_, b_ = h.render_timing()
                rast.append(a_); rein.append(b_)
            cover.append(float((depth >= 0).mean()))
            npts.append(len(h.render_points()))
        sizes[f"{w}x{hgt}"] = {"rasterize_ms_median": round(float(np.median(rast)), 4), "reinforce_ms_median": round(float(np.median(rein)), 4),
                               "rasterize_plus_reinforce_ms_median": round(float(np.median(np.array(rast) + np.array(rein))), 4),
                               "rasterize_ms_max": round(float(np.max(rast)), 4), "render_mesh_call_ms_median": round(float(np.median(call)), 4),
                               "covered_fraction_per_pose": [round(c, 4) for c in cover], "reinforced_points_per_pose": npts}
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short=12", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    except Exception:  # noqa: BLE001
        commit = None
    out = {"metric": "mesh depth render (immesh_render_mesh) on the bench's survey mesh", "unit": "ms",
           "device": torch.cuda.get_device_name(0), "parent_commit": commit, "kernel_sources_sha16": bench.kernel_sources_sha(),
           "survey_mesh": seed, "export_faces": int(nf.value), "export_vertices": int(nv.value),
           "export_ms_median": round(float(np.median(t_exp)), 4), "poses": [int(k) for k in poses], "reps_per_pose": args.reps,
           "camera": "focus 400, z 0.05 / 200, cell 0.01, pose immesh_camera_from_state(trajectory_pose(k))", "sizes": sizes,
           "timing": "export: wall clock of immesh_mesh_export (synchronous, smooth_factor 1, knn 20); rasterize / reinforce: HIP events on the "
                     "renderer's stream (rasterize includes the host read of the pair count between setup and binning); call: wall clock of "
                     "render_mesh incl. its export and the depth read-back"}
    h.close()
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as fp:
            json.dump(out, fp, indent=1)


if __name__ == "__main__":
    main()
