"""Ray-cast timings on the bench's survey mesh (include/immesh_raycast.h): the MESH map pre-seeded from bench.py's corridor survey (its own seeding
helper, imported; bench.py itself is not changed), then immesh_raycast_build_mesh and casts from LiDAR poses along the stream in two scan patterns:
the HDL-64 sweep (64 rings x 2032 azimuth steps = 130 048 rays, synth.hdl64_scan's pattern) and a 100 000-ray Livox rosette (synth.livox_scan's
Halton pattern).  Then the 640 x 480 pixel rays of the depth camera against immesh_render_triangles on the same exported soup -- the rasterizer is
the comparison, not a bar: it amortises a face over a tile, the caster does not.  Reports medians of the device times (HIP events on the caster's
stream, immesh_raycaster_last_timing) after a warm-up per shape, and the wall clock of the calls.  One JSON object on stdout, and in --out when given.

    python tools/raycast_bench.py [--scans 70] [--reps 5] [--out profiles/raycast_bench.json]
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

import bench  # noqa: E402  (seeding helper: corridor_cloud)
from immesh_amd import capi, synth  # noqa: E402


def hdl64_dirs(n_az=2032):
    el = np.deg2rad(np.linspace(2.0, -24.33, 64))
    az = np.linspace(-np.pi, np.pi, n_az, endpoint=False)
    A, E = np.meshgrid(az, el, indexing="ij")
    return np.stack([np.cos(E) * np.cos(A), np.cos(E) * np.sin(A), np.sin(E)], axis=-1).reshape(-1, 3).astype(np.float32)


def livox_dirs(n=100000, k=0):
    az = (synth.halton(n, 2, 1 + k * n) - 0.5) * np.deg2rad(70.4)
    el = (synth.halton(n, 3, 1 + k * n) - 0.5) * np.deg2rad(77.2)
    return np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], axis=1).astype(np.float32)


def med(v):
    return round(float(np.median(v)), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=70, help="stream length whose corridor is surveyed (bench.py --full: 5 + 50 + 15 scans)")
    ap.add_argument("--reps", type=int, default=5, help="timed casts per pose and pattern, after one warm-up")
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
    print(f"[raycast_bench] survey mesh: {seed}", file=sys.stderr, flush=True)

    # ---- build: the export, the copy and the hierarchy
    h.raycast_build_mesh(1.0, 20)                                               # grows the buffers
    build_ms, build_call = [], []
    for _ in range(args.reps):
        t = time.perf_counter()
        sizes = h.raycast_build_mesh(1.0, 20)
        build_call.append(1e3 * (time.perf_counter() - t))
        build_ms.append(h.raycast_timing()[0])

    # ---- casts in the sensors' patterns
    poses = np.linspace(0, args.scans - 1, args.poses).round().astype(int)
    patterns = {}
    for name, dirs in (("hdl64_130048", hdl64_dirs()), ("livox_100000", livox_dirs())):
        cast, rein, call, hit, npts = [], [], [], [], []
        for k in poses:
            R, t = synth.trajectory_pose(int(k))
            fr = h.ray_frame_from_state(capi.make_state(R=R, t=t))
            h.raycast(fr, dirs, None, 0.5, 200.0)                               # warm-up at this shape
            for _ in range(args.reps):
                tc = time.perf_counter()
                _, f = h.raycast(fr, dirs, None, 0.5, 200.0, want_t=False)
                call.append(1e3 * (time.perf_counter() - tc))
                cast.append(h.raycast_timing()[1])
                pts = h.raycast_points(0.01)
                rein.append(h.raycast_timing()[2])
            hit.append(round(float((f >= 0).mean()), 4)); npts.append(len(pts))
        patterns[name] = {"rays": len(dirs), "cast_ms_median": med(cast), "cast_ms_max": round(float(np.max(cast)), 4), "reinforce_ms_median": med(rein),
                          "raycast_call_ms_median": med(call), "hit_fraction_per_pose": hit, "reinforced_points_per_pose": npts}

    # ---- the depth camera's pixel rays: the caster against the rasterizer on the same soup
    vtx, faces = h.mesh_export(1.0, 20)
    w, hgt = 640, 480
    u, v = np.meshgrid(np.arange(w), np.arange(hgt))
    cast, rast, agree = [], [], []
    for k in poses:
        R, t = synth.trajectory_pose(int(k))
        cam = h.camera_from_state(capi.make_state(R=R, t=t), h.default_depth_camera(width=w, height=hgt))
        pix = np.stack([(u - w // 2) / cam.focus, -((v - hgt // 2) / cam.focus), np.full(u.shape, -1.0)], axis=-1).reshape(-1, 3).astype(np.float32)
        fr = capi.ray_frame(np.array(list(cam.rot)).reshape(3, 3), list(cam.pos))
        h.raycast(fr, pix, None, cam.z_near, cam.z_far)
        h.render_triangles(cam, vtx, faces)
        for _ in range(args.reps):
            _, f = h.raycast(fr, pix, None, cam.z_near, cam.z_far, want_t=False)
            cast.append(h.raycast_timing()[1])
            _, face = h.render_triangles(cam, vtx, faces, want_depth=False)
            rast.append(h.render_timing()[0])
        agree.append(round(float((face.reshape(-1) == f).mean()), 5))           # (the pixel rays are floats here: not the bit-exact comparison of the tests)
    pixel = {"rays": w * hgt, "cast_ms_median": med(cast), "rasterize_ms_median": med(rast), "same_face_fraction_per_pose": agree}

    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short=12", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    except Exception:  # noqa: BLE001
        commit = None
    out = {"metric": "rays cast at the bench's survey mesh (immesh_raycast)", "unit": "ms", "device": torch.cuda.get_device_name(0), "parent_commit": commit,
           "kernel_sources_sha16": bench.kernel_sources_sha(), "survey_mesh": seed, "snapshot": {"vertices": sizes[0], "faces": sizes[1], "faces_in_tree": sizes[2]},
           "build_ms_median": med(build_ms), "build_mesh_call_ms_median": med(build_call), "poses": [int(k) for k in poses], "reps_per_pose": args.reps,
           "range": "t_min 0.5, t_max 200 (patterns); z 0.05 / 200 (pixel rays)", "patterns": patterns, "pixel_rays_640x480": pixel,
           "timing": "build / cast / reinforce: HIP events on the caster's stream (build includes the host read of the face count; copies of rays and "
                     "results are outside); *_call: wall clock of the call incl. the export (build) and the copies (cast); rasterize: "
                     "immesh_renderer_last_timing[0] of immesh_render_triangles on the exported soup"}
    h.close()
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as fp:
            json.dump(out, fp, indent=1)


if __name__ == "__main__":
    main()
