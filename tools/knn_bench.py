"""k nearest neighbours, radius counts and outlier removal on the bench's survey mesh (include/immesh_nearest.h, the Neighbours, Count and Outliers
rules): the workload of tools/nearest_bench.py -- the MESH map pre-seeded from bench.py's corridor survey (its own seeding helper, imported; bench.py
itself is not changed), about 100 000 samples of its snapshot as queries, and a 1 M-point cloud of samples of the same mesh at ten times the density
and another seed, displaced by Gaussian noise of 2 cm -- and
  knn_k1 .. knn_k64   immesh_knn_points of the samples, k in {1, 8, 16, 64}, max_dist 1 m, lists fetched
  radius_count        immesh_radius_count_points of the samples, radius 0.1 m
  knn_cloud_k16_mean  immesh_knn_cloud, k = 16, max_dist 1 m, the mean only (no list is stored on the device)
  mask                immesh_cloud_outliers_statistical (mult 2): the mask kernel (the read-back of the means and the host's mu and sigma are outside)
  apply               immesh_cloud_index_apply_outliers: the scan of the mask, the compaction and the build over the kept points
and in the same call immesh_nearest_samples of the same samples on the same index -- the single-nearest query is the comparison, not a bar.
All times are device times from HIP events on the index's stream (immesh_knn_last_timing, immesh_nearest_last_timing); copies are outside.  A round
builds the index anew (the apply shrinks it) and measures every case once, after one warm-up round; the medians over the rounds are reported with
the spread (min, max) across rounds.  One JSON object on stdout, and in --out when given.

    python tools/knn_bench.py [--scans 70] [--rounds 7] [--out profiles/knn_bench.json]
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

KS = (1, 8, 16, 64)


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
    print(f"[knn_bench] survey mesh: {seed}", file=sys.stderr, flush=True)
    sizes = h.raycast_build_mesh(1.0, 20)

    density = args.samples / max(h.mesh_sample(1.0, 0, fetch=False), 1)
    density *= args.samples / max(h.mesh_sample(density, 0, fetch=False), 1)
    rng = np.random.default_rng(0)
    gt, _ = h.mesh_sample(density * args.cloud / args.samples, 1)
    gt = (gt.astype(np.float64) + rng.normal(scale=0.02, size=gt.shape)).astype(np.float32)
    xyz, _ = h.mesh_sample(density, 0)

    keys = tuple("knn_k%d" % k for k in KS) + ("radius_count", "knn_cloud_k16_mean", "mask", "apply", "nearest_samples")
    times = {k: [] for k in keys}
    info, digest = {}, {}
    for rnd in range(-1, args.rounds):                                          # round -1: the warm-up of every shape, not recorded
        rec = {}
        n_cloud = h.cloud_index_build(gt)
        h.nearest_samples(1.0, want=("index",))
        rec["nearest_samples"] = h.nearest_timing()[1]
        for k in KS:
            res = h.knn_points(xyz, k, 1.0)
            rec["knn_k%d" % k] = h.knn_timing()[0]
            digest["knn_k%d" % k] = [int(res["count"].sum()), int(res["index"].astype(np.int64).sum()), float(res["d2"].sum())]
        count = h.radius_count_points(xyz, 0.1)
        rec["radius_count"] = h.knn_timing()[0]
        mean = h.knn_cloud(16, 1.0, want=("mean",))["mean"]
        rec["knn_cloud_k16_mean"] = h.knn_timing()[0]
        digest["knn_cloud_k16_mean"] = float(mean.sum())
        st = h.cloud_outliers_statistical(2.0)
        rec["mask"] = h.knn_timing()[1]
        kept = h.cloud_index_apply_outliers()
        rec["apply"] = h.knn_timing()[2]
        if rnd >= 0:
            for k in keys:
                times[k].append(rec[k])
        info = {"density_per_m2": round(density, 3), "samples": len(xyz), "cloud_points": n_cloud[0], "cloud_points_in_tree": n_cloud[1],
                "radius_count_mean": round(float(count.mean()), 3), "k64_full_lists_fraction": round(float((res["count"] == 64).mean()), 4),
                "mu": st["mu"], "sigma": st["sigma"], "threshold": st["threshold"],
                "kept": st["kept"], "outliers": st["outliers"], "isolated": st["isolated"], "not_finite": st["not_finite"], "points_after_apply": len(kept)}

    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short=12", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    except Exception:  # noqa: BLE001
        commit = None
    out = {"metric": "k nearest neighbours, radius counts and outlier removal on the bench's survey mesh (immesh_knn_points, immesh_radius_count_points, "
                     "immesh_knn_cloud, immesh_cloud_outliers_statistical, immesh_cloud_index_apply_outliers)", "unit": "ms",
           "device": torch.cuda.get_device_name(0), "parent_commit": commit, "kernel_sources_sha16": bench.kernel_sources_sha(), "survey_mesh": seed,
           "snapshot": {"vertices": sizes[0], "faces": sizes[1], "faces_in_tree": sizes[2]}, "rounds": args.rounds, "case": info, "digest": digest,
           "times": {k: summary(v) for k, v in times.items()},
           "timing": "device time from HIP events on the index's stream: the traversal kernel of each query; the mask kernel with the memset of its counts; "
                     "the scan of the mask, the compaction and the whole build over the kept points; immesh_nearest_samples' traversal kernel; copies, the "
                     "read-back of the means and the host's mu and sigma are outside; median, min and max over the rounds, each round measuring every case once"}
    h.close()
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as fp:
            json.dump(out, fp, indent=1)


if __name__ == "__main__":
    main()
