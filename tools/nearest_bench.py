"""Mesh-to-cloud timings on the bench's survey mesh (include/immesh_nearest.h): the MESH map pre-seeded from bench.py's corridor survey (its own
seeding helper, imported; bench.py itself is not changed), then immesh_raycast_build_mesh and
  sample        immesh_mesh_sample at the density that gives about 100 000 samples: the counts, and the scan + the emit launch
  build         immesh_cloud_index_build over a 1 M-point cloud: samples of the same mesh at ten times the density and another seed, displaced by
                Gaussian noise of 2 cm -- a ground-truth scan of the surface
  nearest       immesh_nearest_samples of the 100 000 samples against it (max_dist 1 m), and its reduction (100 bins)
and in the same call immesh_closest_points of the same 100 000 samples, fetched, on the mesh they came from -- the closest-face query is the
comparison, not a bar.  All times are device times from HIP events on the caster's and the index's streams (immesh_mesh_sample_last_timing,
immesh_nearest_last_timing, immesh_closest_last_timing); copies and the read-backs of the two counts are outside.  A round measures every case once,
after one warm-up round; the medians over the rounds are reported with the spread (min, max) across rounds.  One JSON object on stdout, and in --out
when given.

    python tools/nearest_bench.py [--scans 70] [--rounds 7] [--out profiles/nearest_bench.json]
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


def summary(v):
    return {"median": round(float(np.median(v)), 4), "min": round(float(np.min(v)), 4), "max": round(float(np.max(v)), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=70, help="stream length whose corridor is surveyed (bench.py --full: 5 + 50 + 15 scans)")
    ap.add_argument("--rounds", type=int, default=7, help="repetitions of the whole set")
    ap.add_argument("--samples", type=int, default=100000)
    ap.add_argument("--cloud", type=int, default=1000000)
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
    print(f"[nearest_bench] survey mesh: {seed}", file=sys.stderr, flush=True)
    sizes = h.raycast_build_mesh(1.0, 20)

    # the density: the count at 1 per unit area is the area up to rounding; one correction step
    density = args.samples / max(h.mesh_sample(1.0, 0, fetch=False), 1)
    density *= args.samples / max(h.mesh_sample(density, 0, fetch=False), 1)
    rng = np.random.default_rng(0)
    gt, _ = h.mesh_sample(density * args.cloud / args.samples, 1)
    gt = (gt.astype(np.float64) + rng.normal(scale=0.02, size=gt.shape)).astype(np.float32)

    keys = ("sample_count", "sample_emit", "index_build", "nearest_samples", "nearest_reduce", "closest_points")
    times = {k: [] for k in keys}
    info = {}
    for rnd in range(-1, args.rounds):                                          # round -1: the warm-up of every shape, not recorded
        rec = {}
        xyz, _ = h.mesh_sample(density, 0)
        rec["sample_count"], rec["sample_emit"] = h.mesh_sample_timing()
        n_cloud = h.cloud_index_build(gt)
        rec["index_build"] = h.nearest_timing()[0]
        res = h.nearest_samples(1.0, want=("index",))
        rec["nearest_samples"] = h.nearest_timing()[1]
        st, _ = h.nearest_stats(0.01, 100)
        rec["nearest_reduce"] = h.nearest_timing()[2]
        face = h.closest_points(xyz, 1.0, want=("face",))["face"]
        rec["closest_points"] = h.closest_timing()[0]
        if rnd >= 0:
            for k in keys:
                times[k].append(rec[k])
        info = {"density_per_m2": round(density, 3), "samples": len(xyz), "cloud_points": n_cloud[0],
                "cloud_points_in_tree": n_cloud[1], "with_neighbour_fraction": round(float((res["index"] >= 0).mean()), 4), "mean_dist": round(st.mean, 5),
                "rms_dist": round(st.rms, 5), "max_dist_found": round(st.max_dist, 5), "closest_with_face_fraction": round(float((face >= 0).mean()), 4)}

    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short=12", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    except Exception:  # noqa: BLE001
        commit = None
    out = {"metric": "mesh-to-cloud distances on the bench's survey mesh (immesh_mesh_sample, immesh_cloud_index_build, immesh_nearest_samples)", "unit": "ms",
           "device": torch.cuda.get_device_name(0), "parent_commit": commit, "kernel_sources_sha16": bench.kernel_sources_sha(), "survey_mesh": seed,
           "snapshot": {"vertices": sizes[0], "faces": sizes[1], "faces_in_tree": sizes[2]}, "rounds": args.rounds, "case": info,
           "times": {k: summary(v) for k, v in times.items()},
           "timing": "device time from HIP events on the caster's stream (the count kernel; the scan and the emit kernel; immesh_closest_points' traversal "
                     "kernel) and on the index's stream (mark, scan, compact, codes, sort, hierarchy, refit; the traversal kernel; the two reduction kernels "
                     "with the histogram's memset); copies and the read-backs of the counts are outside; median, min and max over the rounds, each round "
                     "measuring every case once"}
    h.close()
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as fp:
            json.dump(out, fp, indent=1)


if __name__ == "__main__":
    main()
