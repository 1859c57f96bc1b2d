"""Self-intersection timings on two crossing noisy sheets (include/immesh_intersect.h; tests/intersect_checker.py's crossing_sheets) at a few sizes:
  candidates    immesh_self_intersect's first span: the count walk, the read-back of the total, the scan and the emit walk
  tests         its second span: the segment tests, flag / scan / compaction of the hits, the read-back of their number, the sort, the pairs
  apply         immesh_self_intersect_apply: the compaction of the kept faces and the caster's build over them (the build is nearly all of it)
All three are device times from HIP events on the caster's stream (immesh_self_intersect_last_timing); every round rebuilds the caster from the soup,
since an apply leaves a mesh without pairs behind.  Beside them: candidates per face, candidate pairs tested per second (the tests span), pairs found,
and for comparison the closest-point query (immesh_closest_points, the nearest existing walk of the same hierarchy) for as many points as the mesh
has faces: the faces' centroids moved off the surface.  With --checker the pairs are compared with the grid checker's and its wall time recorded.  No
gate: the numbers are recorded.  One JSON object on stdout, and in --out when given.

    python tools/intersect_bench.py [--sides 50 112 158 354] [--rounds 7] [--checker] [--out profiles/intersect_bench.json]
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

import intersect_checker as ic  # noqa: E402
from immesh_amd import capi  # noqa: E402


def summary(v):
    return {"median": round(float(np.median(v)), 4), "min": round(float(np.min(v)), 4), "max": round(float(np.max(v)), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sides", type=int, nargs="+", default=[50, 112, 158, 354], help="cells per side of each sheet (four faces per cell in all)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--checker", action="store_true", help="compare the pairs with the grid checker's (sizes up to 158) and record its wall time")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    h = capi.HotPath(capi.load_hip_library(), capi.avia_config(cap_root_voxels=1 << 12, cap_scan_points=200000, cap_vertices=1 << 18, cap_triangles=1 << 20), "immesh_")
    out = {"rounds": args.rounds, "sizes": []}
    try:
        for side in args.sides:
            vtx, faces = ic.crossing_sheets(np.random.default_rng(side), side, side)
            pts = vtx[faces].astype(np.float64).mean(axis=1) + np.array([0.0, 0.0, 0.05])
            times = {"build": [], "candidates": [], "tests": [], "apply": [], "closest": []}
            for rnd in range(-1, args.rounds):                                   # round -1: the warm-up (allocations), not recorded
                h.raycast_build_triangles(vtx, faces)
                h.closest_points(pts, 10.0, want=())
                st = h.self_intersect(1 << 30)
                if rnd == args.rounds - 1:
                    pairs, mask = h.self_intersect_pairs()
                h.self_intersect_apply()
                if rnd >= 0:
                    ms = h.self_intersect_timing()
                    times["candidates"].append(ms[0]); times["tests"].append(ms[1]); times["apply"].append(ms[2])
                    times["closest"].append(h.closest_timing()[0])
            again = h.self_intersect(1 << 30)
            assert again.n_pairs == 0, again.n_pairs
            rec = {"side": side, "faces": len(faces), "candidates": st.n_candidates, "candidates_per_face": round(st.n_candidates / len(faces), 3),
                   "n_share": list(st.n_share), "pairs": st.n_pairs, "faces_hit": st.n_faces_hit, "max_partners": st.max_partners,
                   "ms": {k: summary(v) for k, v in times.items() if v},
                   "candidates_tested_per_second": round(st.n_candidates / (np.median(times["tests"]) * 1e-3), 0),
                   "candidates_found_per_second": round(st.n_candidates / (np.median(times["candidates"]) * 1e-3), 0),
                   "pairs_per_second": round(st.n_pairs / ((np.median(times["candidates"]) + np.median(times["tests"])) * 1e-3), 0),
                   "candidates_over_closest": round(float(np.median(times["candidates"]) / np.median(times["closest"])), 3)}
            if args.checker and side <= 158:
                t0 = time.perf_counter()
                ref = ic.grid(vtx, faces)
                rec["checker_seconds"] = round(time.perf_counter() - t0, 3)
                assert ref["stats"]["n_candidates"] == st.n_candidates and ref["pairs"].tobytes() == pairs.tobytes() and ref["mask"].tobytes() == mask.tobytes()
                rec["checker_equal"] = True
            out["sizes"].append(rec)
    finally:
        h.close()
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as fp:
            json.dump(out, fp, indent=1)


if __name__ == "__main__":
    main()
