#!/usr/bin/env python3
"""immesh_colourer_last_timing for a 640 x 480 frame over maps of ~100 k, ~1 M and ~cap_vertices vertices (a lattice plane, every point a vertex,
seen from 40 m above): set ALL, with and without selection, both models; median of 20 after 5 warm-ups, with the algorithmic bytes per image and the
fraction of the HBM roof they imply.  Writes the JSON named on the command line (default profiles/colour_timing.json) after every stage.

usage: tools/colour_bench.py [out.json]"""
import json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from immesh_amd import capi

HBM_ROOF = 8.0e12   # bytes / s, MI355X
lib = capi.load_hip_library()
cfg = capi.avia_config(cap_root_voxels=1 << 12, cap_scan_points=1 << 20, cap_vertices=1 << 22, cap_triangles=1 << 24, mesh_append_budget=1 << 21)
h = capi.HotPath(lib, cfg, "immesh_")
out = {"image": "640x480", "hbm_roof_bytes_per_s": HBM_ROOF, "cap_vertices": 1 << 22, "stages": []}
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "colour_timing.json")

def strip(x0, nx, ny):
    """nx x ny lattice points, 0.125 m apart, on the plane z = 0, from x = x0"""
    gx, gy = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    p = np.zeros((gx.size, 4), np.float32)
    p[:, 0] = x0 + gx.ravel() * 0.125; p[:, 1] = gy.ravel() * 0.125 - ny * 0.0625; p[:, 3] = 10.0
    return p

rng = np.random.default_rng(3)
px = rng.integers(1, 256, (480, 640, 3)).astype(np.uint8)
NY = 2040
def feed(x_from, x_to, frame):
    """lattice columns [x_from, x_to) in scans of at most 2^20 points"""
    per = (1 << 20) // NY
    while x_from < x_to:
        n = min(per, x_to - x_from)
        t0 = time.time()
        h.mesh_scan(strip(x_from * 0.125, n, NY), np.array([0.0, 0.0, 30.0]), frame_idx=frame, fetch=False)
        print("scan", frame, "columns", x_from, "+", n, "vertices", h.counters()["n_vertices"], "%.2f s" % (time.time() - t0), flush=True)
        x_from += n; frame += 1
    return frame

def measure(tag):
    nv = h.counters()["n_vertices"]
    # looking straight down on the middle of what is meshed, from 40 m: the frame covers 64 m x 48 m
    ext = nv / NY * 0.125
    rot = np.array([[1.0, 0.0, 0.0], [0.0, -1.0, 0.0], [0.0, 0.0, -1.0]])
    stage = {"n_vertices": nv, "runs": []}
    for model in (capi.COLOUR_PLAIN, capi.COLOUR_VIEW):
        for md in (0.0, 1.0):
            ms, stats = [], None
            for k in range(25):
                im = h.default_image(px, fx=400.0, fy=400.0, cx=320.0, cy=240.0, rot=rot, pos=[ext / 2 + 0.01 * k, 0.003 * k, 40.0], obs_time=0.05 * k,
                                     inv_exposure=0.01)
                stats = h.colour_image(im, model, capi.COLOUR_SET_ALL, select_min_dis=md)
                if k >= 5:
                    ms.append(h.colour_timing())
            med = np.median(np.array(ms), axis=0)
            hits = stats["n_hit"]
            # algorithmic bytes: positions (12 B) and the raw (u, v) (8 B) per vertex of the render set, PLAIN reads the positions once more for dmin and
            # n_obs (4 B) for its gate; per hit 76 B of state read + 76 B written + 12 B of image taps; selection: positions + 12 B of records written
            # and read back + the 12-byte cells of the table cleared
            n_sel = stats["n_selected"]
            b = n_sel * (12 + 8) + (n_sel * (12 + 4) if model == capi.COLOUR_PLAIN else 0) + hits * (76 + 76 + 12)
            b_sel = (nv * (12 + 12 + 12 + 4 + 4) + (640 + 3) * (480 + 3) * 12) if md > 0 else 0
            run = {"model": "PLAIN" if model == 0 else "VIEW", "select_min_dis": md, "upload_ms": float(med[0]), "select_ms": float(med[1]),
                   "update_ms": float(med[2]), "n_selected": n_sel, "n_hit": hits, "update_bytes": int(b), "select_bytes": int(b_sel),
                   "update_roof_fraction": float(b / (med[2] * 1e-3) / HBM_ROOF) if med[2] > 0 else None,
                   "select_roof_fraction": float(b_sel / (med[1] * 1e-3) / HBM_ROOF) if md > 0 and med[1] > 0 else None}
            print(tag, run, flush=True)
            stage["runs"].append(run)
    out["stages"].append(stage)
    json.dump(out, open(OUT, "w"), indent=1)

frame = feed(0, 49, 0)            # 49 x 2040 = 99 960
measure("100k")
frame = feed(49, 490, frame)      # 999 600
measure("1M")
frame = feed(490, 2040, frame)    # 4 161 600 (cap_vertices = 4 194 304)
measure("cap")
h.close()
print("done")
