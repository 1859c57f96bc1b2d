"""Hole filling timings on tools/topology_bench.py's 1 M-face soup (include/immesh_topology.h, the Holes rule): a grid sheet with one-cell holes plus
a few thousand fragments, the faces shuffled.
  holes         immesh_topology_holes: init, degrees, flags, scan, rank_init, the ranking's rounds (one launch each), boxes, scan, scatter, limits,
                chords, decide, scan, emit -- every launch; the one read-back of the counters is outside
  apply         immesh_topology_holes_apply: the faces and the new faces copied side by side on the device, and the caster's hierarchy built over
                them (the build is nearly all of it: immesh_raycast_build_triangles' device part)
Both are device times from HIP events on the caster's stream (immesh_topology_holes_last_timing).  Every round rebuilds the caster from the soup and
analyses it again, since an apply leaves a closed mesh behind; the analysis' time of the same rounds is recorded beside the others.  Beside them the
wall time of the numpy checker (tests/holes_checker.py: np.unique, dicts and a walk in Python) on the same soup, on this machine's CPU -- the
brute-force restatement, not a tuned CPU implementation.  No gate: the numbers are recorded.  One JSON object on stdout, and in --out when given.

    python tools/holes_bench.py [--side 700] [--holes 3000] [--fragments 4000] [--max-edges 16] [--rounds 7] [--out profiles/holes_bench.json]
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

import holes_checker as hc  # noqa: E402
import topology_checker as tc  # noqa: E402
from immesh_amd import capi  # noqa: E402


def summary(v):
    return {"median": round(float(np.median(v)), 4), "min": round(float(np.min(v)), 4), "max": round(float(np.max(v)), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=700, help="cells per side of the sheet (two faces per cell)")
    ap.add_argument("--holes", type=int, default=3000)
    ap.add_argument("--fragments", type=int, default=4000)
    ap.add_argument("--max-edges", type=int, default=16)
    ap.add_argument("--max-diagonal", type=float, default=0.0)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--no-checker", action="store_true", help="skip the CPU side (for a run under a profiler)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    vtx, faces = tc.sheet_with_fragments(rng, args.side, args.side, args.holes, args.fragments)
    h = capi.HotPath(capi.load_hip_library(), capi.avia_config(cap_root_voxels=1 << 12, cap_scan_points=200000, cap_vertices=1 << 18, cap_triangles=1 << 20), "immesh_")
    try:
        times = {"analyse": [], "holes": [], "apply": []}
        for rnd in range(-1, args.rounds):                                       # round -1: the warm-up (allocations), not recorded
            sizes = h.raycast_build_triangles(vtx, faces)
            before = h.topology_analyse()
            st = h.topology_holes(args.max_edges, args.max_diagonal)
            if rnd == args.rounds - 1:
                got = dict(h.topology_holes_loops(), cycle=h.topology_holes_cycles())
                got["new_loop"], got["new_faces"] = h.topology_holes_faces()
            h.topology_holes_apply()
            if rnd >= 0:
                times["analyse"].append(h.topology_timing()[0]); times["holes"].append(h.topology_holes_timing()[0]); times["apply"].append(h.topology_holes_timing()[1])
        stats = {n: getattr(st, n) for n, _ in capi.HolesStats._fields_}
        after = h.topology_analyse()
        loops = {"before": before.n_boundary_loops, "after": after.n_boundary_loops, "largest_loop_edges": before.largest_loop_edges,
                 "boundary_edges_before": before.n_boundary, "boundary_edges_after": after.n_boundary, "faces_after": after.n_faces}
    finally:
        h.close()
    cpu = None
    if not args.no_checker:
        t0 = time.perf_counter()
        ref = hc.holes(vtx, faces, args.max_edges, args.max_diagonal)
        seconds = round(time.perf_counter() - t0, 3)
        assert ref["stats"] == stats and all(np.array_equal(got[k], ref[k]) for k in got), "the device and the checker disagree"
        assert loops["after"] == loops["before"] - stats["n_filled"] and loops["boundary_edges_after"] == loops["boundary_edges_before"] - stats["n_edges_closed"]
        cpu = {"checker_seconds": seconds, "cpus": os.cpu_count()}
    out = {"metric": "ordered boundary cycles and hole filling on a 1 M-face soup (immesh_topology_holes, immesh_topology_holes_apply)", "unit": "ms",
           "soup": {"sheet_cells": [args.side, args.side], "holes": args.holes, "fragments": args.fragments, "vertices": sizes[0], "faces": sizes[1],
                    "face_order": "shuffled"},
           "max_edges": args.max_edges, "max_diagonal": args.max_diagonal, "stats": stats, "loops": loops, "rounds": args.rounds,
           "times": {k: summary(v) for k, v in times.items()}, "cpu": cpu,
           "timing": "device time from HIP events on the caster's stream: holes = every launch of the pass; apply = two copies on the device and the build of "
                     "the hierarchy over faces ++ new_faces; analyse = the analysis of the soup in the same rounds; copies of the results are outside; "
                     "median, min and max over the rounds.  cpu: wall time of tests/holes_checker.py on the same soup in one Python process"}
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as fp:
            json.dump(out, fp, indent=1)


if __name__ == "__main__":
    main()
