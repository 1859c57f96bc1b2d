"""One-ring, smoothing and vertex-normal timings on tools/topology_bench.py's 1 M-face soup with noise on its vertices (include/immesh_smooth.h): a
grid sheet with one-cell holes plus a few thousand fragments, the faces shuffled.
  one_ring      emit, the 64-bit pair sort, heads, scan, runs, entries, rows and classes, lists: everything before the first step
  step          one Jacobi step, from passes of 10 and of 100 steps (the steps' span over their number; the span includes the launch that counts what
                moved)
  apply         immesh_smooth_apply: the buffers change places and the caster's hierarchy is built over the moved vertices (the build is all of it)
  normals       immesh_vertex_normals without the copy to the host: wall time around the call, which ends with its one read-back of n_zero
  build         the caster's build of the same input in the same rounds: what one pass over this mesh costs
one_ring, step and apply are device times from HIP events on the caster's stream (immesh_smooth_last_timing).  Every round rebuilds the caster from
the soup, since an apply leaves the moved mesh behind.  Beside them the wall time of the numpy checker (tests/smooth_checker.py) on the same input, on
this machine's CPU -- the restatement of the contract, not a tuned CPU implementation -- and the comparison of every output of the last round with
it.  No gate: the numbers are recorded.  One JSON object on stdout, and in --out when given.

    python tools/smooth_bench.py [--side 700] [--holes 3000] [--fragments 4000] [--steps 10 100] [--rounds 7] [--out profiles/smooth_bench.json]
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

import smooth_checker as sm  # noqa: E402
import topology_checker as tc  # noqa: E402
from immesh_amd import capi  # noqa: E402

SIGMA = 0.01                                                                            # a fifth of the sheet's grid step


def summary(v):
    return {"median": round(float(np.median(v)), 4), "min": round(float(np.min(v)), 4), "max": round(float(np.max(v)), 4)}


def device(h):
    out = h.smooth_vertices()
    out["vtx_out"] = out.pop("vtx")
    out.update(h.smooth_adjacency())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=700, help="cells per side of the sheet (two faces per cell)")
    ap.add_argument("--holes", type=int, default=3000)
    ap.add_argument("--fragments", type=int, default=4000)
    ap.add_argument("--steps", type=int, nargs="*", default=[10, 100])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--no-checker", action="store_true", help="skip the CPU side (for a run under a profiler)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    vtx, faces = tc.sheet_with_fragments(rng, args.side, args.side, args.holes, args.fragments)
    vtx = sm.noisy(rng, vtx, SIGMA)
    h = capi.HotPath(capi.load_hip_library(), capi.avia_config(cap_root_voxels=1 << 12, cap_scan_points=200000, cap_vertices=1 << 18, cap_triangles=1 << 20), "immesh_")
    results = {}
    try:
        for n_steps in args.steps:
            times = {"build": [], "one_ring": [], "steps": [], "step": [], "apply": [], "normals_wall": []}
            for rnd in range(-1, args.rounds):                                   # round -1: the warm-up (allocations), not recorded
                h.raycast_build_triangles(vtx, faces)
                build_ms = h.raycast_timing()[0]
                st = h.smooth(n_steps, 0.5, -0.53, capi.SMOOTH_BORDER_FIXED)
                if rnd == args.rounds - 1 and not args.no_checker:
                    got = device(h)
                h.smooth_apply()
                t0 = time.perf_counter()
                _, n_zero = h.vertex_normals(fetch=False)
                normals_ms = (time.perf_counter() - t0) * 1e3
                if rnd >= 0:
                    ms = h.smooth_last_timing()
                    for k, v in (("build", build_ms), ("one_ring", ms[0]), ("steps", ms[1]), ("step", ms[1] / max(n_steps, 1)), ("apply", ms[2]),
                                 ("normals_wall", normals_ms)):
                        times[k].append(v)
            stats = {n: getattr(st, n) for n, _ in capi.SmoothStats._fields_}
            cpu = None
            if not args.no_checker:
                normals_dev = h.vertex_normals()
                t0 = time.perf_counter()
                ref = sm.smooth(vtx, faces, n_steps, 0.5, -0.53, sm.FIXED)
                seconds = round(time.perf_counter() - t0, 3)
                assert ref["stats"] == stats and all(got[k].tobytes() == ref[k].tobytes() for k, _ in sm.ARRAYS), "the device and the checker disagree: %d steps" % n_steps
                t0 = time.perf_counter()
                normals_ref = sm.normals(ref["vtx_out"], faces)
                normals_seconds = round(time.perf_counter() - t0, 3)
                assert normals_dev[0].tobytes() == normals_ref[0].tobytes() and normals_dev[1] == normals_ref[1] == n_zero, "the normals and the checker disagree"
                cpu = {"checker_seconds": seconds, "normals_checker_seconds": normals_seconds, "cpus": os.cpu_count()}
            results["steps_%d" % n_steps] = {"n_steps": n_steps, "stats": stats, "n_zero_normals": n_zero, "times": {k: summary(t) for k, t in times.items()}, "cpu": cpu}
    finally:
        h.close()
    out = {"metric": "one-ring, Taubin smoothing and vertex normals on a 1 M-face soup (immesh_smooth, immesh_smooth_apply, immesh_vertex_normals)", "unit": "ms",
           "soup": {"sheet_cells": [args.side, args.side], "holes": args.holes, "fragments": args.fragments, "vertices": len(vtx), "faces": len(faces),
                    "face_order": "shuffled", "noise_sigma": SIGMA},
           "rounds": args.rounds, "cases": results,
           "timing": "device time from HIP events on the caster's stream: one_ring = every launch before the first step; steps = the step launches and the "
                     "launch that counts what moved, step = steps / n_steps; apply = the build of the hierarchy over the moved vertices; build = the build "
                     "of the input's hierarchy in the same rounds; normals_wall = wall time of immesh_vertex_normals without the copy of the normals; "
                     "median, min and max over the rounds.  cpu: wall time of tests/smooth_checker.py on the same input in one Python process"}
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as fp:
            json.dump(out, fp, indent=1)


if __name__ == "__main__":
    main()
