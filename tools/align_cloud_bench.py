"""Cloud-to-cloud alignment timings (include/immesh_align.h, the Cloud rule) on a synthetic target: the vertices of a bumpy sheet
(tests/align_checker.py's bumpy_sheet) of about 10 000, 100 000 and 1 000 000 points, 0.1 m apart, indexed, with normals from 8 neighbours; the
source is the same number of points, the target's jittered by 2 cm and displaced by 2 degrees about its centre and 5 cm:
  step          the device time of one immesh_align_cloud_step at the displaced pose, PLANE and POINT rows, huber 0 and 0.1, for both kernel
                shapes: fused (one launch, its registers held to the walk's occupancy) and split (the default: the walk stores winner and q, a second
                launch forms and folds the terms)
  loop          immesh_align_cloud from the displaced pose, PLANE rows: iterations, status, the device time summed over its steps, the wall time
                of the call (the upload of the source, the launches, one 256 B copy and the host solve per iteration)
  yardstick     immesh_nearest_points (no output copied back) plus immesh_nearest_reduce for the same points at the same pose on the same index in
                the same process: the existing traversal of the same hierarchy, which stores 29 B per point and reduces them in a second pass
Device times are from HIP events on the index's stream.  Each figure is the median (with min and max) of --rounds rounds after a warm-up.  No gate:
the numbers are recorded.  The clouds are synthetic: convergence on real scans and partial overlap under huber are not measured here.  One JSON
object on stdout, and in --out when given.

    python tools/align_cloud_bench.py [--sides 100 317 1000] [--rounds 7] [--out profiles/align_cloud_bench.json]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import align_checker as ac  # noqa: E402
from immesh_amd import capi  # noqa: E402

VARIANTS = {"fused": 0, "split": 1}
CELL, MAX_DIST, HUBER, JITTER = 0.1, 2.0, 0.1, 0.02


def summary(v):
    return {"median": round(float(np.median(v)), 4), "min": round(float(np.min(v)), 4), "max": round(float(np.max(v)), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sides", type=int, nargs="+", default=[100, 317, 1000], help="points per side of the sheet: side^2 points")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    h = capi.HotPath(capi.load_hip_library(), capi.avia_config(cap_root_voxels=1 << 12, cap_scan_points=200000, cap_vertices=1 << 18, cap_triangles=1 << 20), "immesh_")
    out = {"rounds": args.rounds, "cell": CELL, "max_dist": MAX_DIST, "huber": HUBER, "jitter": JITTER, "displacement": {"degrees": 2.0, "metres": 0.05},
           "synthetic": True, "sizes": []}
    try:
        for side in args.sides:
            g = np.linspace(0.0, CELL * (side - 1), side)
            X, Y = np.meshgrid(g, g, indexing="ij")
            target = np.stack([X, Y, 0.3 * np.sin(X) * np.cos(1.3 * Y)], axis=-1).reshape(-1, 3).astype(np.float32)
            rng = np.random.default_rng(side)
            world = target.astype(np.float64) + rng.uniform(-JITTER, JITTER, target.shape)
            mid = world.mean(axis=0)
            R, t = ac.rodrigues([1.0, 2.0, 3.0], math.radians(2.0)), np.array([0.03, -0.02, 0.0346])        # |t| = 0.05
            src = ((world - mid - t) @ R + mid).astype(np.float32)                        # R (x - mid) + mid + t = w: the pose to be found
            centre = capi.align_centre_mean(src)
            n, n_in = h.cloud_index_build(target)
            nr = h.cloud_normals(8, 0.5, want=())
            rec = {"side": side, "target_points": n, "source_points": len(src), "with_normal": nr["with_normal"], "normals_ms": round(h.normals_timing()[0], 4),
                   "step_ms": {}}
            for mode, name in ((capi.ALIGN_PLANE, "plane"), (capi.ALIGN_POINT, "point")):
                for huber, tag in ((0.0, ""), (HUBER, "_huber")):
                    opts = capi.align_options(mode=mode, max_dist=MAX_DIST, centre=centre)
                    bits = set()
                    for variant, v in VARIANTS.items():
                        h.align_cloud_set_variant(v)
                        ms = []
                        for rnd in range(-1, args.rounds):                                 # round -1: the warm-up (allocations), not recorded
                            sy, _, _ = h.align_cloud_step(src, opts, huber)
                            if rnd >= 0:
                                ms.append(h.align_cloud_timing()[0])
                        bits.add(bytes(sy))
                        rec["step_ms"][f"{name}{tag}_{variant}"] = summary(ms)
                    assert len(bits) == 1, "the kernel shapes disagree"
                    rec[f"{name}{tag}_used"] = sy.n_used
            h.align_cloud_set_variant(1)                                                   # the default
            opts = capi.align_options(mode=capi.ALIGN_PLANE, max_dist=MAX_DIST, centre=centre, max_iters=50, eps_rot=1e-9, eps_trans=1e-9)
            rec["loop"] = {}
            for huber, tag in ((0.0, "plane"), (HUBER, "plane_huber")):
                dev, wall = [], []
                for rnd in range(-1, args.rounds):
                    t0 = time.perf_counter()
                    res, hist = h.align_cloud(src, opts, huber)
                    t1 = time.perf_counter()
                    if rnd >= 0:
                        dev.append(h.align_cloud_timing()[1]); wall.append((t1 - t0) * 1e3)
                rot, pos = np.array(list(res.frame.rot)).reshape(3, 3), np.array(list(res.frame.pos))
                moved = src.astype(np.float64) @ rot.T + pos
                rec["loop"][tag] = {"status": capi.ALIGN_STATUS[res.status], "iterations": res.iterations, "rms_first": hist[0, 1], "rms_last": hist[-1, 1],
                                    "fitness": res.system.n_used / max(len(src), 1), "max_error_to_truth": float(np.abs(moved - world).max()),
                                    "device_ms": summary(dev), "wall_ms": summary(wall)}
            query, reduce_ = [], []
            for rnd in range(-1, args.rounds):
                h.nearest_points(src, MAX_DIST, want=())
                st, _ = h.nearest_stats(0.05, 64)
                if rnd >= 0:
                    ms = h.nearest_timing()
                    query.append(ms[1]); reduce_.append(ms[2])
            both = [a + b for a, b in zip(query, reduce_)]
            rec["yardstick_ms"] = {"nearest_points": summary(query), "nearest_reduce": summary(reduce_), "sum": summary(both), "with_neighbour": st.n_with_face}
            rec["step_over_yardstick"] = {k: round(v["median"] / max(rec["yardstick_ms"]["sum"]["median"], 1e-9), 3) for k, v in rec["step_ms"].items()}
            rec["step_within_yardstick_range"] = {k: bool(v["median"] <= rec["yardstick_ms"]["sum"]["max"]) for k, v in rec["step_ms"].items()}
            out["sizes"].append(rec)
            print(json.dumps(rec), file=sys.stderr, flush=True)
    finally:
        h.close()
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as fp:
            json.dump(out, fp, indent=1)


if __name__ == "__main__":
    main()
