"""Alignment timings on a bumpy sheet (include/immesh_align.h; tests/align_checker.py's bumpy_sheet) of about 10 000, 100 000 and 500 000 faces, cells
of 0.1 m, with a cloud of twice as many points sampled on its faces and displaced by 2 degrees about its centre and 5 cm:
  step          the device time of one immesh_align_step at the displaced pose (PLANE rows; POINT rows beside it), for each of the three kernel
                shapes: fused (the default: its registers are held to the walk's occupancy), split (the walk stores face and q, a second launch
                forms and folds the terms), fused_uncapped (the fused kernel as the register allocator leaves it)
  loop          immesh_align from the displaced pose, PLANE rows: iterations, status, the device time summed over its steps, the wall time of the call
                (the upload of the cloud, the launches, one 256 B copy and the host solve per iteration)
  yardstick     immesh_closest_points (no output copied back) plus immesh_closest_reduce for the same points at the same pose in the same process:
                the existing traversal of the same hierarchy, which stores 37 B per point and reduces them in a second pass
Device times are from HIP events on the caster's stream.  Each figure is the median (with min and max) of --rounds rounds after a warm-up.  No gate:
the numbers are recorded.  One JSON object on stdout, and in --out when given.

    python tools/align_bench.py [--sides 72 225 501] [--rounds 7] [--out profiles/align_bench.json]
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

VARIANTS = {"fused": 0, "split": 1, "fused_uncapped": 2}
CELL, MAX_DIST = 0.1, 2.0


def summary(v):
    return {"median": round(float(np.median(v)), 4), "min": round(float(np.min(v)), 4), "max": round(float(np.max(v)), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sides", type=int, nargs="+", default=[72, 225, 501], help="vertices per side of the sheet: 2 (side - 1)^2 faces")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    h = capi.HotPath(capi.load_hip_library(), capi.avia_config(cap_root_voxels=1 << 12, cap_scan_points=200000, cap_vertices=1 << 18, cap_triangles=1 << 20), "immesh_")
    out = {"rounds": args.rounds, "cell": CELL, "max_dist": MAX_DIST, "displacement": {"degrees": 2.0, "metres": 0.05}, "sizes": []}
    try:
        for side in args.sides:
            vtx, faces = ac.bumpy_sheet(side, CELL * (side - 1))
            world = ac.sample_on_faces(vtx, faces, 2 * len(faces), side)
            mid = world.mean(axis=0)
            R, t = ac.rodrigues([1.0, 2.0, 3.0], math.radians(2.0)), np.array([0.03, -0.02, 0.0346])        # |t| = 0.05
            cloud = ((world - mid - t) @ R + mid).astype(np.float32)                      # R (x - mid) + mid + t = w: the pose to be found
            centre = capi.align_centre_mean(cloud)
            h.raycast_build_triangles(vtx, faces)
            rec = {"side": side, "faces": len(faces), "points": len(cloud), "step_ms": {}}
            for mode, name in ((capi.ALIGN_PLANE, "plane"), (capi.ALIGN_POINT, "point")):
                opts = capi.align_options(mode=mode, max_dist=MAX_DIST, centre=centre)
                bits = set()
                for variant, v in VARIANTS.items():
                    h.align_set_variant(v)
                    ms = []
                    for rnd in range(-1, args.rounds):                                     # round -1: the warm-up (allocations), not recorded
                        sy, _, _ = h.align_step(cloud, opts)
                        if rnd >= 0:
                            ms.append(h.align_timing()[0])
                    bits.add(bytes(sy))
                    rec["step_ms"][f"{name}_{variant}"] = summary(ms)
                assert len(bits) == 1, "the kernel shapes disagree"
                rec[f"{name}_used"] = sy.n_used
            h.align_set_variant(0)
            opts = capi.align_options(mode=capi.ALIGN_PLANE, max_dist=MAX_DIST, centre=centre, max_iters=30, eps_rot=1e-9, eps_trans=1e-9)
            dev, wall = [], []
            for rnd in range(-1, args.rounds):
                t0 = time.perf_counter()
                res, hist = h.align(cloud, opts)
                t1 = time.perf_counter()
                if rnd >= 0:
                    dev.append(h.align_timing()[1]); wall.append((t1 - t0) * 1e3)
            rot, pos = np.array(list(res.frame.rot)).reshape(3, 3), np.array(list(res.frame.pos))
            moved = cloud.astype(np.float64) @ rot.T + pos
            rec["loop"] = {"status": capi.ALIGN_STATUS[res.status], "iterations": res.iterations, "rms_first": hist[0, 1], "rms_last": hist[-1, 1],
                           "max_error_to_truth": float(np.abs(moved - world).max()), "device_ms": summary(dev), "wall_ms": summary(wall)}
            query, reduce_ = [], []
            for rnd in range(-1, args.rounds):
                h.closest_points(cloud, MAX_DIST, want=())
                st, _ = h.closest_stats(0.05, 64)
                if rnd >= 0:
                    ms = h.closest_timing()
                    query.append(ms[0]); reduce_.append(ms[1])
            both = [a + b for a, b in zip(query, reduce_)]
            rec["yardstick_ms"] = {"closest_points": summary(query), "closest_reduce": summary(reduce_), "sum": summary(both), "with_face": st.n_with_face}
            rec["step_over_yardstick"] = {k: round(v["median"] / max(rec["yardstick_ms"]["sum"]["median"], 1e-9), 3) for k, v in rec["step_ms"].items()}
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
