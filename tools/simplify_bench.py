"""Weld and vertex-clustering timings on tools/topology_bench.py's 1 M-face soup (include/immesh_simplify.h): a grid sheet with one-cell holes plus a
few thousand fragments, the faces shuffled.
  weld          the soup with its vertices unshared (three of its own per face) and shuffled, cell = 0: the two-pass 96-bit sort
  cell k        the shared soup at a cell of k grid steps, FIRST and MEAN: the one-pass 64-bit sort; MEAN adds the walk of one lane per cluster
  simplify      immesh_simplify: mark, keys, the sort(s), heads, scan, runs, labels, scan, clusters, (mean,) vmap, faces, the two sort passes of the
                duplicates, scan, compact -- every launch; the one read-back of the counters is outside
  apply         immesh_simplify_apply: the buffers change places and the caster's hierarchy is built over the result (the build is all of it)
Both are device times from HIP events on the caster's stream (immesh_simplify_last_timing).  Every round rebuilds the caster from the soup, since
an apply leaves the smaller mesh behind.  Beside them the wall time of the numpy checker (tests/simplify_checker.py) on the same input, on this
machine's CPU -- the restatement of the contract, not a tuned CPU implementation -- and the comparison of every output of the last round with it.
No gate: the numbers are recorded.  One JSON object on stdout, and in --out when given.

    python tools/simplify_bench.py [--side 700] [--holes 3000] [--fragments 4000] [--cells 2 4 16] [--rounds 7] [--out profiles/simplify_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import simplify_checker as sc  # noqa: E402
import topology_checker as tc  # noqa: E402
from immesh_amd import capi  # noqa: E402

STEP = 0.05                                                                             # the sheet's grid step (tc.sheet_with_fragments)


def summary(v):
    return {"median": round(float(np.median(v)), 4), "min": round(float(np.min(v)), 4), "max": round(float(np.max(v)), 4)}


def device(h):
    out = h.simplify_vertices()
    out["vtx_out"] = out.pop("vtx")
    out.update(h.simplify_maps())
    out["faces_out"] = h.simplify_faces()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=700, help="cells per side of the sheet (two faces per cell)")
    ap.add_argument("--holes", type=int, default=3000)
    ap.add_argument("--fragments", type=int, default=4000)
    ap.add_argument("--cells", type=int, nargs="*", default=[2, 4, 16], help="cells in grid steps")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--no-checker", action="store_true", help="skip the CPU side (for a run under a profiler)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    vtx, faces = tc.sheet_with_fragments(rng, args.side, args.side, args.holes, args.fragments)
    cases = [("weld_unshared", sc.unshared(vtx, faces, rng), 0.0, sc.FIRST)]
    for k in args.cells:
        cases += [("cell_%d_%s" % (k, name), (vtx, faces), k * STEP, mode) for name, mode in (("first", sc.FIRST), ("mean", sc.MEAN))]
    h = capi.HotPath(capi.load_hip_library(), capi.avia_config(cap_root_voxels=1 << 12, cap_scan_points=200000, cap_vertices=1 << 18, cap_triangles=1 << 20), "immesh_")
    results = {}
    try:
        for name, (v, f), cell, mode in cases:
            times = {"build": [], "simplify": [], "apply": []}
            for rnd in range(-1, args.rounds):                                   # round -1: the warm-up (allocations), not recorded
                h.raycast_build_triangles(v, f)
                build_ms = h.raycast_timing()[0]
                st = h.simplify(cell, mode, True)
                if rnd == args.rounds - 1 and not args.no_checker:
                    got = device(h)
                h.simplify_apply()
                if rnd >= 0:
                    ms = h.simplify_last_timing()
                    times["build"].append(build_ms); times["simplify"].append(ms[0]); times["apply"].append(ms[1])
            stats = {n: getattr(st, n) for n, _ in capi.SimplifyStats._fields_}
            cpu = None
            if not args.no_checker:
                t0 = time.perf_counter()
                ref = sc.simplify(v, f, cell, mode, True)
                seconds = round(time.perf_counter() - t0, 3)
                assert ref["stats"] == stats and all(got[k].tobytes() == ref[k].tobytes() for k, _ in sc.ARRAYS), "the device and the checker disagree: " + name
                cpu = {"checker_seconds": seconds, "cpus": os.cpu_count()}
            results[name] = {"cell": cell, "cell_grid_steps": round(cell / STEP), "mode": ("first", "mean")[mode], "vertices": len(v), "faces": len(f), "stats": stats,
                             "times": {k: summary(t) for k, t in times.items()}, "cpu": cpu}
    finally:
        h.close()
    out = {"metric": "weld and vertex clustering on a 1 M-face soup (immesh_simplify, immesh_simplify_apply)", "unit": "ms",
           "soup": {"sheet_cells": [args.side, args.side], "holes": args.holes, "fragments": args.fragments, "vertices": len(vtx), "faces": len(faces),
                    "face_order": "shuffled", "grid_step": STEP},
           "rounds": args.rounds, "cases": results,
           "timing": "device time from HIP events on the caster's stream: simplify = every launch of the pass; apply = the build of the hierarchy over the "
                     "result; build = the build of the input's hierarchy in the same rounds; copies of the results are outside; median, min and max over "
                     "the rounds.  cpu: wall time of tests/simplify_checker.py on the same input in one Python process"}
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as fp:
            json.dump(out, fp, indent=1)


if __name__ == "__main__":
    main()
