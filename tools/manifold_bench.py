"""Manifold-pass timings beside the analysis (include/immesh_topology.h, the Manifold rule) on two kinds of soup at about 10 k, 100 k and 500 k faces:
  sheet         tools/topology_bench.py's soup (tests/topology_checker.py's sheet_with_fragments, the faces shuffled): nothing to split, the cost of
                asking
  glued         tests/manifold_checker.py's glued_soup: 4 x 4 sheets glued on vertices and edges, the faces shuffled: singular vertices in thousands
Per soup:
  analyse       immesh_topology_analyse of the same rounds
  manifold      immesh_topology_manifold: init, link, flatten, links, scan, (the read-back of the number of fans,) keys, sort, fans, run heads, scan,
                run starts, table, vertices, emit -- every launch and that one read-back
  apply         immesh_topology_manifold_apply: two buffers change places and the caster's hierarchy is built over them (the build is all of it)
All are device times from HIP events on the caster's stream.  Every round rebuilds the caster from the soup, since an apply leaves a split mesh
behind.  Soups of at most --check-faces faces are compared with the checker, every output.  No gate: the numbers are recorded.  One JSON object on
stdout, and in --out when given.

    python tools/manifold_bench.py [--sides 70 224 500] [--rounds 7] [--check-faces 120000] [--out profiles/manifold_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import manifold_checker as mc  # noqa: E402
import topology_checker as tc  # noqa: E402
from immesh_amd import capi  # noqa: E402


def summary(v):
    return {"median": round(float(np.median(v)), 4), "min": round(float(np.min(v)), 4), "max": round(float(np.max(v)), 4)}


def measure(h, vtx, faces, rounds, check):
    times = {"analyse": [], "manifold": [], "apply": []}
    for rnd in range(-1, rounds):                                                # round -1: the warm-up (allocations), not recorded
        sizes = h.raycast_build_triangles(vtx, faces)
        before = h.topology_analyse()
        st = h.topology_manifold()
        if rnd == rounds - 1 and check:
            got = dict(h.topology_manifold_fans(), n_fans_out=h.topology_manifold_vertices())
            got["fan_out"], got["faces_out"] = h.topology_manifold_faces()
            got["vsrc"], got["xyz"] = h.topology_manifold_new_vertices()
        h.topology_manifold_apply()
        if rnd >= 0:
            times["analyse"].append(h.topology_timing()[0]); times["manifold"].append(h.topology_manifold_timing()[0]); times["apply"].append(h.topology_manifold_timing()[1])
    stats = {n: getattr(st, n) for n, _ in capi.ManifoldStats._fields_}
    after = h.topology_analyse()
    assert after.n_nonmanifold == 0 and after.n_vertices_used == stats["n_fans"], "the split soup does not keep the rule's invariant"
    if check:
        ref = mc.manifold(vtx, faces)
        assert ref["stats"] == stats and all(got[k].tobytes() == ref[k].tobytes() for k in got), "the device and the checker disagree"
    return {"vertices": sizes[0], "faces": sizes[1], "half_edges": 3 * before.n_counting, "stats": stats, "checked": bool(check),
            "times": {k: summary(v) for k, v in times.items()},
            "manifold_ns_per_half_edge": round(1e6 * float(np.median(times["manifold"])) / max(3 * before.n_counting, 1), 4),
            "analyse_ns_per_half_edge": round(1e6 * float(np.median(times["analyse"])) / max(3 * before.n_counting, 1), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sides", type=int, nargs="+", default=[70, 224, 500], help="cells per side of the sheet (two faces per cell); the glued soup gets as many faces")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--check-faces", type=int, default=120000, help="compare the soups of at most so many faces with the checker (0: none)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    h = capi.HotPath(capi.load_hip_library(), capi.avia_config(cap_root_voxels=1 << 12, cap_scan_points=200000, cap_vertices=1 << 18, cap_triangles=1 << 20), "immesh_")
    soups = []
    try:
        for side in args.sides:
            rng = np.random.default_rng(side)
            vtx, faces = tc.sheet_with_fragments(rng, side, side, max(side * side // 160, 1), max(side * side // 120, 1))
            soups.append({"kind": "sheet", "sheet_cells": [side, side], **measure(h, vtx, faces, args.rounds, len(faces) <= args.check_faces)})
            vtx, faces = mc.glued_soup(rng, max(len(faces) // 32, 1))
            soups.append({"kind": "glued", "pieces": len(faces) // 32, **measure(h, vtx, faces, args.rounds, len(faces) <= args.check_faces)})
    finally:
        h.close()
    out = {"metric": "one vertex per fan of faces beside the analysis (immesh_topology_manifold, immesh_topology_manifold_apply, immesh_topology_analyse)",
           "unit": "ms", "rounds": args.rounds, "soups": soups,
           "timing": "device time from HIP events on the caster's stream: manifold = every launch of the pass and its one read-back; apply = the build of the "
                     "hierarchy over the split soup; analyse = the analysis of the soup in the same rounds; copies of the results are outside; median, min and "
                     "max over the rounds"}
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as fp:
            json.dump(out, fp, indent=1)


if __name__ == "__main__":
    main()
