"""Split the pinched vertices and fins of a mesh file on the device (include/immesh_topology.h, the Manifold rule): read, analyse, pass, fetch, write.
Every fan of faces round a vertex gets a vertex of its own: the first fan keeps the vertex, the others get bit copies of it behind the old vertices.
The faces keep their number and order; no edge of the output has three uses and no vertex two fans.  The PLY layout is the one immesh_save_ply writes
(binary little-endian: float x y z; list uchar int vertex_indices).  One JSON object with the pass' counts on stdout.

    python tools/mesh_manifold.py IN.ply OUT.ply
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
from mesh_eval import read_ply  # noqa: E402
from mesh_simplify import write_ply  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("ply_in")
    ap.add_argument("ply_out")
    args = ap.parse_args()
    vtx, faces = read_ply(args.ply_in)
    h = capi.HotPath(capi.load_hip_library(), capi.avia_config(cap_root_voxels=1 << 12, cap_scan_points=200000, cap_vertices=1 << 18, cap_triangles=1 << 20), "immesh_")
    try:
        h.raycast_build_triangles(vtx, faces)
        h.topology_analyse()
        st = h.topology_manifold()
        write_ply(args.ply_out, np.concatenate([vtx, h.topology_manifold_new_vertices()[1]]), h.topology_manifold_faces()[1])
        ms = h.topology_manifold_timing()[0]
    finally:
        h.close()
    print(json.dumps({**{n: getattr(st, n) for n, _ in capi.ManifoldStats._fields_}, "manifold_ms": round(ms, 4)}), flush=True)


if __name__ == "__main__":
    main()
