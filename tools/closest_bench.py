"""Closest-point timings on the bench's survey mesh (include/immesh_closest.h): the MESH map pre-seeded from bench.py's corridor survey (its own
seeding helper, imported; bench.py itself is not changed), then immesh_raycast_build_mesh and immesh_closest_points on
  scan        the world points of a 100 000-point Livox scan from a pose on the stream (max_dist 1 m)
  scan+0.05   the same points displaced by 0.05 m along random directions (max_dist 1 m)
  scan+1      the same points displaced by 1 m (max_dist 2 m)
  uniform0.5  100 000 points uniform in the snapshot's bounds, max_dist 0.5 m
  uniform5    the same points, max_dist 5 m
the reduction of each (immesh_closest_reduce, 100 bins), and in the same call immesh_raycast on a 100 000-ray Livox rosette from the same pose -- the
ray cast is the comparison, not a bar.  All times are device times from HIP events on the caster's stream (immesh_closest_last_timing,
immesh_raycaster_last_timing); copies are outside.  A round measures every case once, after one warm-up round; the medians over the rounds are
reported with the spread (min, max) across rounds.  One JSON object on stdout, and in --out when given.

    python tools/closest_bench.py [--scans 70] [--rounds 7] [--out profiles/closest_bench.json]
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


def livox_dirs(n=100000, k=0):
    az = (synth.halton(n, 2, 1 + k * n) - 0.5) * np.deg2rad(70.4)
    el = (synth.halton(n, 3, 1 + k * n) - 0.5) * np.deg2rad(77.2)
    return np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], axis=1).astype(np.float32)


def summary(v):
    return {"median": round(float(np.median(v)), 4), "min": round(float(np.min(v)), 4), "max": round(float(np.max(v)), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=70, help="stream length whose corridor is surveyed (bench.py --full: 5 + 50 + 15 scans)")
    ap.add_argument("--rounds", type=int, default=7, help="repetitions of the whole set")
    ap.add_argument("--pose", type=int, default=35, help="the scan whose points are queried")
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
    print(f"[closest_bench] survey mesh: {seed}", file=sys.stderr, flush=True)
    sizes = h.raycast_build_mesh(1.0, 20)
    vtx, _ = h.mesh_export(1.0, 20)
    fin = vtx[np.isfinite(vtx).all(axis=1)]
    lo, hi = fin.min(axis=0).astype(np.float64), fin.max(axis=0).astype(np.float64)

    rng = np.random.default_rng(0)
    extT = np.array(list(cfg.extT))
    R, t = synth.trajectory_pose(args.pose)
    raw = synth.livox_scan(args.pose, R, t, n_pts=100000, extT=extT)
    world = (raw[:, :3].astype(np.float64) + extT) @ R.T + t
    unit = rng.normal(size=world.shape)
    unit /= np.linalg.norm(unit, axis=1)[:, None]
    uniform = rng.uniform(lo, hi, world.shape).astype(np.float32)
    cases = [("scan", world.astype(np.float32), 1.0), ("scan+0.05", (world + 0.05 * unit).astype(np.float32), 1.0), ("scan+1", (world + unit).astype(np.float32), 2.0),
             ("uniform0.5", uniform, 0.5), ("uniform5", uniform, 5.0)]
    frame = h.ray_frame_from_state(capi.make_state(R=R, t=t))
    dirs = livox_dirs()

    times = {name: {"query": [], "reduce": []} for name, _, _ in cases}
    ray_ms, info = [], {}
    for rnd in range(-1, args.rounds):                                          # round -1: the warm-up of every shape, not recorded
        for name, pts, max_dist in cases:
            res = h.closest_points(pts, max_dist, want=("face",))
            if rnd >= 0:
                times[name]["query"].append(h.closest_timing()[0])
            st, _ = h.closest_stats(max_dist / 100.0, 100)
            if rnd >= 0:
                times[name]["reduce"].append(h.closest_timing()[1])
            info[name] = {"points": len(pts), "max_dist": max_dist, "with_face_fraction": round(float((res["face"] >= 0).mean()), 4),
                          "mean_dist": round(st.mean, 5), "rms_dist": round(st.rms, 5), "max_dist_found": round(st.max_dist, 5)}
        _, f = h.raycast(frame, dirs, None, 0.5, 200.0, want_t=False)
        if rnd >= 0:
            ray_ms.append(h.raycast_timing()[1])
    results = {name: dict(info[name], **{k: summary(v) for k, v in times[name].items()}) for name, _, _ in cases}

    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short=12", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    except Exception:  # noqa: BLE001
        commit = None
    out = {"metric": "closest face of every point on the bench's survey mesh (immesh_closest_points)", "unit": "ms", "device": torch.cuda.get_device_name(0),
           "parent_commit": commit, "kernel_sources_sha16": bench.kernel_sources_sha(), "survey_mesh": seed,
           "snapshot": {"vertices": sizes[0], "faces": sizes[1], "faces_in_tree": sizes[2]}, "pose": args.pose, "rounds": args.rounds, "cases": results,
           "raycast_livox_100000": dict(summary(ray_ms), hit_fraction=round(float((f >= 0).mean()), 4)),
           "timing": "device time from HIP events on the caster's stream: the traversal kernel, the two "
                     "reduction kernels with the histogram's memset, and immesh_raycast's traversal kernel; copies are outside; median, min and max over "
                     "the rounds, each round measuring every case once"}
    h.close()
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as fp:
            json.dump(out, fp, indent=1)


if __name__ == "__main__":
    main()
