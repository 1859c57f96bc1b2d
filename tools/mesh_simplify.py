"""Weld or decimate a mesh file on the device (include/immesh_simplify.h): read, pass, fetch, write.
  --cell 0 (the default)  welds the vertices of equal coordinates: a soup that repeats its vertices becomes a mesh whose faces share indices
  --cell C                clusters the vertices on a grid of C; --mode first keeps a cluster's first vertex where it is, --mode mean takes the mean
Faces that collapse go, and so do faces given twice unless --keep-duplicate-faces; vertices no face uses are dropped.  The PLY layout is the one
immesh_save_ply writes (binary little-endian: float x y z; list uchar int vertex_indices).  One JSON object with the pass' counts on stdout.

    python tools/mesh_simplify.py IN.ply OUT.ply [--cell C] [--mode first|mean] [--keep-duplicate-faces]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from immesh_amd import capi  # noqa: E402
from mesh_eval import SIMPLIFY_MODES, read_ply  # noqa: E402


def write_ply(path, vtx, faces):
    """the layout immesh_save_ply writes"""
    head = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\nelement face %d\n"
            "property list uchar int vertex_indices\nend_header\n" % (len(vtx), len(faces))).encode()
    rec = np.zeros((len(faces), 13), np.uint8)
    rec[:, 0] = 3
    rec[:, 1:] = np.ascontiguousarray(faces, np.int32).view(np.uint8).reshape(len(faces), 12)
    with open(path, "wb") as fp:
        fp.write(head + np.ascontiguousarray(vtx, np.float32).tobytes() + rec.tobytes())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("ply_in")
    ap.add_argument("ply_out")
    ap.add_argument("--cell", type=float, default=0.0, help="the grid's cell (0: weld the vertices of equal coordinates)")
    ap.add_argument("--mode", choices=sorted(SIMPLIFY_MODES), default="first")
    ap.add_argument("--keep-duplicate-faces", action="store_true")
    args = ap.parse_args()
    vtx, faces = read_ply(args.ply_in)
    h = capi.HotPath(capi.load_hip_library(), capi.avia_config(cap_root_voxels=1 << 12, cap_scan_points=200000, cap_vertices=1 << 18, cap_triangles=1 << 20), "immesh_")
    try:
        h.raycast_build_triangles(vtx, faces)
        st = h.simplify(args.cell, SIMPLIFY_MODES[args.mode], not args.keep_duplicate_faces)
        write_ply(args.ply_out, h.simplify_vertices()["vtx"], h.simplify_faces())
        ms = h.simplify_last_timing()[0]
    finally:
        h.close()
    print(json.dumps({"cell": args.cell, "mode": args.mode, "merge_duplicates": not args.keep_duplicate_faces,
                      **{n: getattr(st, n) for n, _ in capi.SimplifyStats._fields_}, "simplify_ms": round(ms, 4)}), flush=True)


if __name__ == "__main__":
    main()
