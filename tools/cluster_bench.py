"""Euclidean clusters of a 1 M-point cloud on the bench's survey mesh (include/immesh_nearest.h, the Clusters rule): the cloud of tools/knn_bench.py
-- the MESH map pre-seeded from bench.py's corridor survey (its own seeding helper, imported; bench.py itself is not changed), 1 M samples of its
snapshot displaced by Gaussian noise of 2 cm -- and, per radius,
  radius_count_cloud   immesh_radius_count_cloud: the same walk without the joins, the yardstick
  clusters_nb0         immesh_cloud_clusters with min_neighbours = 0 (plain cluster extraction): kinds, joins, numbering and table
  clusters_nbM         immesh_cloud_clusters with min_neighbours = M (--min-neighbours): count and kinds, joins, border walk, numbering and table
with the joins launch as a multiple of the yardstick beside the mean candidate count of the radius, and once
  select, apply        immesh_cloud_clusters_select (keep the largest cluster: the mask kernel) and immesh_cloud_index_apply_outliers
All times are device times from HIP events on the index's stream (immesh_cloud_clusters_last_timing, immesh_knn_last_timing); copies and the one
read-back that sizes the table are outside.  Every case is measured once per round after one warm-up round; the medians over the rounds are reported
with the spread (min, max).  One JSON object on stdout, and in --out when given.

    python tools/cluster_bench.py [--scans 70] [--rounds 5] [--radii 0.03 0.05 0.1 0.2] [--min-neighbours 6] [--out profiles/cluster_bench.json]
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

SPANS = ("count", "joins", "border", "table")


def summary(v):
    return {"median": round(float(np.median(v)), 4), "min": round(float(np.min(v)), 4), "max": round(float(np.max(v)), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=70, help="stream length whose corridor is surveyed (bench.py --full: 5 + 50 + 15 scans)")
    ap.add_argument("--rounds", type=int, default=5, help="repetitions of the whole set")
    ap.add_argument("--cloud", type=int, default=1000000)
    ap.add_argument("--radii", type=float, nargs="+", default=[0.03, 0.05, 0.1, 0.2])
    ap.add_argument("--min-neighbours", type=int, default=6)
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
    print(f"[cluster_bench] survey mesh: {seed}", file=sys.stderr, flush=True)
    sizes = h.raycast_build_mesh(1.0, 20)

    density = args.cloud / max(h.mesh_sample(1.0, 0, fetch=False), 1)
    density *= args.cloud / max(h.mesh_sample(density, 0, fetch=False), 1)
    rng = np.random.default_rng(0)
    gt, _ = h.mesh_sample(density, 1)
    gt = (gt.astype(np.float64) + rng.normal(scale=0.02, size=gt.shape)).astype(np.float32)
    n_cloud = h.cloud_index_build(gt)

    m = args.min_neighbours
    times, info = {}, {}
    for rnd in range(-1, args.rounds):                                          # round -1: the warm-up of every shape, not recorded
        rec = {}
        for r in args.radii:
            tag = "r%g" % r
            count = h.radius_count_cloud(r)
            rec[tag + "/radius_count_cloud"] = h.knn_timing()[0]
            case = {"mean_candidates": round(float(count.mean()), 3)}
            for name, nb in (("clusters_nb0", 0), ("clusters_nb%d" % m, m)):
                res = h.cloud_clusters(r, nb, want=())
                for span, ms in zip(SPANS, h.clusters_timing()):
                    rec["%s/%s/%s" % (tag, name, span)] = ms
                case[name] = {"n_clusters": res["n_clusters"], **res["counts"]}
            info[tag] = case
        if rnd >= 0:
            for k, v in rec.items():
                times.setdefault(k, []).append(v)
    st = h.cloud_clusters_select(keep_largest=1)                                # over the last clusters
    t_select = h.knn_timing()[1]
    kept = h.cloud_index_apply_outliers()
    t_apply = h.knn_timing()[2]

    med = {k: float(np.median(v)) for k, v in times.items()}
    for r in args.radii:
        tag = "r%g" % r
        base = med[tag + "/radius_count_cloud"]
        for name in ("clusters_nb0", "clusters_nb%d" % m):
            info[tag][name]["joins_over_radius_count"] = round(med["%s/%s/joins" % (tag, name)] / base, 3) if base > 0 else None
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short=12", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    except Exception:  # noqa: BLE001
        commit = None
    out = {"metric": "Euclidean clusters of a 1 M-point cloud on the bench's survey mesh (immesh_cloud_clusters) beside immesh_radius_count_cloud at the same radius",
           "unit": "ms", "device": torch.cuda.get_device_name(0), "parent_commit": commit, "kernel_sources_sha16": bench.kernel_sources_sha(), "survey_mesh": seed,
           "snapshot": {"vertices": sizes[0], "faces": sizes[1], "faces_in_tree": sizes[2]}, "rounds": args.rounds, "cloud_points": n_cloud[0],
           "cloud_points_in_tree": n_cloud[1], "min_neighbours": m, "case": info, "times": {k: summary(v) for k, v in times.items()},
           "select_keep_largest_1": {"mask_ms": round(t_select, 4), "apply_ms": round(t_apply, 4), "kept": st["kept"], "dropped": st["dropped"],
                                     "noise": st["noise"], "points_after_apply": len(kept)},
           "timing": "device time from HIP events on the index's stream: count = the Count launch (when min_neighbours > 0) and the kind kernel; joins = the "
                     "joins launch alone; border = the border walk; table = the flatten, the scan and the table launches; copies and the read-back of the "
                     "number of clusters are outside; median, min and max over the rounds, each round measuring every case once"}
    h.close()
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as fp:
            json.dump(out, fp, indent=1)


if __name__ == "__main__":
    main()
