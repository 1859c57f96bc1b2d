"""Mesh-topology timings on a 1 M-face soup (include/immesh_topology.h): a grid sheet with one-cell holes plus a few thousand fragments of one to
four faces, the faces shuffled (tests/topology_checker.py's sheet_with_fragments, the scale test's soup at five times the size).
  analyse       immesh_topology_analyse: every launch and the one read-back of the count of counting faces between them
  select        immesh_topology_select(min_faces = 5): decide, mask, scan, compact
Both are device times from HIP events on the caster's stream (immesh_topology_last_timing); copies of the results are outside.  Beside them the wall
time of the numpy checker (tests/topology_checker.py: np.unique, a Python union-find loop, the boxes as a loop) on the same soup, on this machine's
CPU -- the brute-force restatement, not a tuned CPU implementation -- and, where scipy is installed, of scipy.sparse.csgraph.connected_components on
the face-edge graph (the components alone).  No gate: the numbers are recorded.  One JSON object on stdout, and in --out when given.

    python tools/topology_bench.py [--side 700] [--holes 3000] [--fragments 4000] [--rounds 7] [--out profiles/topology_bench.json]
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

import topology_checker as tc  # noqa: E402
from immesh_amd import capi  # noqa: E402


def summary(v):
    return {"median": round(float(np.median(v)), 4), "min": round(float(np.min(v)), 4), "max": round(float(np.max(v)), 4)}


def scipy_components(faces):
    try:
        import scipy.sparse as sp
        from scipy.sparse.csgraph import connected_components
    except ImportError:
        return None
    t0 = time.perf_counter()
    F = faces.astype(np.int64)
    cf = np.nonzero((F[:, 0] != F[:, 1]) & (F[:, 1] != F[:, 2]) & (F[:, 0] != F[:, 2]))[0]
    a, b = F[cf].reshape(-1), F[cf][:, [1, 2, 0]].reshape(-1)
    _, eid = np.unique((np.minimum(a, b) << 32) | np.maximum(a, b), return_inverse=True)
    n = len(faces) + int(eid.max()) + 1
    g = sp.coo_matrix((np.ones(len(eid), np.int8), (np.repeat(cf, 3), len(faces) + eid)), shape=(n, n))
    _, lab = connected_components(g, directed=False)
    return {"seconds": round(time.perf_counter() - t0, 3), "components": len(set(lab[cf].tolist()))}


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
    h = capi.HotPath(capi.load_hip_library(), capi.avia_config(cap_root_voxels=1 << 12, cap_scan_points=200000, cap_vertices=1 << 18, cap_triangles=1 << 20), "immesh_")
    try:
        sizes = h.raycast_build_triangles(vtx, faces)
        times = {"analyse": [], "select": []}
        for rnd in range(-1, args.rounds):                                       # round -1: the warm-up (allocations), not recorded
            st = h.topology_analyse()
            keep, kept = h.topology_select(min_faces=5)
            if rnd >= 0:
                ms = h.topology_timing()
                times["analyse"].append(ms[0]); times["select"].append(ms[1])
        stats = {n: getattr(st, n) for n, _ in capi.TopologyStats._fields_}
        build_ms = h.raycast_timing()[0]
    finally:
        h.close()
    cpu = None
    if not args.no_checker:
        t0 = time.perf_counter()
        ref = tc.analyse(vtx, faces)
        t1 = time.perf_counter()
        want_keep, want_kept = tc.select(ref, faces, min_faces=5)
        t2 = time.perf_counter()
        assert ref["stats"] == stats and np.array_equal(keep, want_keep) and np.array_equal(kept, want_kept), "the device and the checker disagree"
        cpu = {"checker_analyse_seconds": round(t1 - t0, 3), "checker_select_seconds": round(t2 - t1, 3), "cpus": os.cpu_count(),
               "scipy_connected_components": scipy_components(faces)}
    out = {"metric": "mesh topology of a 1 M-face soup (immesh_topology_analyse, immesh_topology_select)", "unit": "ms",
           "soup": {"sheet_cells": [args.side, args.side], "holes": args.holes, "fragments": args.fragments, "vertices": sizes[0], "faces": sizes[1],
                    "face_order": "shuffled"},
           "stats": stats, "kept_faces_min_faces_5": int(len(kept)), "rounds": args.rounds, "times": {k: summary(v) for k, v in times.items()},
           "caster_build_ms_for_scale": round(build_ms, 4), "cpu": cpu,
           "timing": "device time from HIP events on the caster's stream: analyse = mark, scan, the read-back of the count, vertices, emit, pair sort, "
                     "classify (both union-finds), flatten, scan, preset, components, boundary, largest; select = decide, mask, scan, compact; copies of the "
                     "results are outside; median, min and max over the rounds.  cpu: wall time of tests/topology_checker.py on the same soup in one "
                     "Python process"}
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as fp:
            json.dump(out, fp, indent=1)


if __name__ == "__main__":
    main()
