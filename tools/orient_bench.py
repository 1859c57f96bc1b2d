"""Orientation timings on tools/topology_bench.py's 1 M-face soup with half the faces flipped at random (include/immesh_topology.h, the Orientation
rule): a grid sheet with one-cell holes plus a few thousand fragments, the faces shuffled, every face reversed with probability one half.
  orient        immesh_topology_orient in each of the three modes: init, link (the double cover's unions), flatten, scan, patches, inconsistent,
                decide, flip -- every launch; the one read-back of the counters is outside
  apply         immesh_topology_orient_apply: the oriented faces copied over the caster's on the device
Both are device times from HIP events on the caster's stream (immesh_topology_orient_last_timing).  Every round rebuilds the caster from the flipped
soup and analyses it again, since an apply leaves an oriented mesh behind; the analysis' time of the same rounds is recorded beside the others.
Beside them the wall time of the numpy checker (tests/orient_checker.py: np.unique, a breadth-first search in Python) on the same soup, on this
machine's CPU -- the brute-force restatement, not a tuned CPU implementation.  No gate: the numbers are recorded.  For scale: the analysis of the
unflipped soup was measured at 3.85 ms, its union pass at 1.81 ms of that.  One JSON object on stdout, and in --out when
given.

    python tools/orient_bench.py [--side 700] [--holes 3000] [--fragments 4000] [--rounds 7] [--out profiles/orient_bench.json]
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

import orient_checker as oc  # noqa: E402
import topology_checker as tc  # noqa: E402
from immesh_amd import capi  # noqa: E402

MODES = (("first", capi.ORIENT_FIRST), ("fewest", capi.ORIENT_FEWEST), ("viewpoint", capi.ORIENT_VIEWPOINT))


def summary(v):
    return {"median": round(float(np.median(v)), 4), "min": round(float(np.min(v)), 4), "max": round(float(np.max(v)), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=700, help="cells per side of the sheet (two faces per cell)")
    ap.add_argument("--holes", type=int, default=3000)
    ap.add_argument("--fragments", type=int, default=4000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--no-checker", action="store_true", help="skip the CPU side (for a run under a profiler)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    vtx, faces = tc.sheet_with_fragments(rng, args.side, args.side, args.holes, args.fragments)
    faces = oc.flip_random(rng, faces)[0]
    viewpoint = (0.025 * args.side, 0.025 * args.side, 100.0)                      # above the middle of the sheet
    h = capi.HotPath(capi.load_hip_library(), capi.avia_config(cap_root_voxels=1 << 12, cap_scan_points=200000, cap_vertices=1 << 18, cap_triangles=1 << 20), "immesh_")
    try:
        times = {"analyse": [], "apply": [], **{"orient_" + name: [] for name, _ in MODES}}
        stats, got = {}, {}
        for rnd in range(-1, args.rounds):                                       # round -1: the warm-up (allocations), not recorded
            sizes = h.raycast_build_triangles(vtx, faces)
            h.topology_analyse()
            for name, mode in MODES:
                st = h.topology_orient(mode, viewpoint if name == "viewpoint" else None)
                if rnd >= 0:
                    times["orient_" + name].append(h.topology_orient_timing()[0])
                stats[name] = {n: getattr(st, n) for n, _ in capi.OrientStats._fields_}
                if rnd == args.rounds - 1:
                    got[name] = h.topology_orient_faces()
            h.topology_orient_apply()
            if rnd >= 0:
                times["analyse"].append(h.topology_timing()[0]); times["apply"].append(h.topology_orient_timing()[1])
        after = h.topology_analyse().n_inconsistent
    finally:
        h.close()
    cpu = None
    if not args.no_checker:
        t0 = time.perf_counter()
        part = oc.partition(faces)
        t1 = time.perf_counter()
        seconds = {}
        for name, mode in MODES:
            t2 = time.perf_counter()
            ref = oc.orient(vtx, faces, mode, viewpoint, part)
            seconds[name] = round(time.perf_counter() - t2, 3)
            assert ref["stats"] == stats[name] and all(np.array_equal(got[name][k], ref[k]) for k in ("patch", "flip", "faces")), "the device and the checker disagree"
        assert after == stats["viewpoint"]["n_inconsistent_after"]
        cpu = {"checker_partition_seconds": round(t1 - t0, 3), "checker_mode_seconds": seconds, "cpus": os.cpu_count()}
    out = {"metric": "orientation of a 1 M-face soup with half its faces flipped (immesh_topology_orient, immesh_topology_orient_apply)", "unit": "ms",
           "soup": {"sheet_cells": [args.side, args.side], "holes": args.holes, "fragments": args.fragments, "vertices": sizes[0], "faces": sizes[1],
                    "face_order": "shuffled", "flipped": "every face with probability 1/2"},
           "viewpoint": list(viewpoint), "stats": stats, "inconsistent_after_apply": after, "rounds": args.rounds,
           "times": {k: summary(v) for k, v in times.items()}, "cpu": cpu,
           "context": "the analysis of the unflipped soup: 3.85 ms, its union pass 1.81 ms of that (DESIGN.md, section 18); not a target",
           "timing": "device time from HIP events on the caster's stream: orient = init, link, flatten, scan, patches, inconsistent, decide, flip; apply = one "
                     "copy on the device; analyse = the analysis of the flipped soup in the same rounds; copies of the results are outside; median, min and "
                     "max over the rounds.  cpu: wall time of tests/orient_checker.py on the same soup in one Python process"}
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as fp:
            json.dump(out, fp, indent=1)


if __name__ == "__main__":
    main()
