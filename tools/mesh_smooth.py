"""Smooth a mesh file on the device (include/immesh_smooth.h): read, pass, fetch, write.
  --steps N               N Jacobi steps over the one-ring, the factor --lambda on even and --mu on odd steps (Taubin: mu < -lambda < 0, which does not
                          shrink; mu == lambda is plain Laplacian smoothing, which does)
  --border fixed|along|free   a border vertex (on a boundary or a non-manifold edge) stays, slides along the border, or moves as an interior one
  --normals               write area-weighted vertex normals of the smoothed mesh as nx ny nz per vertex
The faces are written as they were read.  The PLY layout is the one immesh_save_ply writes (binary little-endian: float x y z; list uchar int
vertex_indices), with float nx ny nz behind z under --normals.  One JSON object with the pass' counts on stdout.

    python tools/mesh_smooth.py IN.ply OUT.ply [--steps 10] [--lambda 0.5] [--mu -0.53] [--border fixed|along|free] [--normals]
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
from mesh_eval import SMOOTH_BORDERS, read_ply  # noqa: E402


def write_ply(path, vtx, faces, normals=None):
    """the layout immesh_save_ply writes; with normals: float nx ny nz behind z"""
    props = "property float x\nproperty float y\nproperty float z\n" + ("property float nx\nproperty float ny\nproperty float nz\n" if normals is not None else "")
    head = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\n%selement face %d\nproperty list uchar int vertex_indices\nend_header\n"
            % (len(vtx), props, len(faces))).encode()
    rows = np.ascontiguousarray(vtx, np.float32).reshape(-1, 3)
    if normals is not None:
        rows = np.concatenate([rows, np.ascontiguousarray(normals, np.float32).reshape(-1, 3)], axis=1)
    rec = np.zeros((len(faces), 13), np.uint8)
    rec[:, 0] = 3
    rec[:, 1:] = np.ascontiguousarray(faces, np.int32).view(np.uint8).reshape(len(faces), 12)
    with open(path, "wb") as fp:
        fp.write(head + np.ascontiguousarray(rows).tobytes() + rec.tobytes())


def read_ply_normals(path):
    """a file of write_ply(..., normals) -> vtx, normals, faces"""
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    if b"property float nx\nproperty float ny\nproperty float nz\n" not in head:
        raise ValueError(f"{path}: no vertex normals")
    lines = head.split(b"\n")
    nv = int([l for l in lines if l.startswith(b"element vertex")][0].split()[-1])
    nf = int([l for l in lines if l.startswith(b"element face")][0].split()[-1])
    rows = np.frombuffer(body[:nv * 24], np.float32).reshape(-1, 6)
    rec = np.frombuffer(body[nv * 24:nv * 24 + nf * 13], np.uint8).reshape(nf, 13)
    return rows[:, :3].copy(), rows[:, 3:].copy(), rec[:, 1:].copy().view(np.int32).reshape(nf, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("ply_in")
    ap.add_argument("ply_out")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--lambda", dest="lam", type=float, default=0.5)
    ap.add_argument("--mu", type=float, default=-0.53)
    ap.add_argument("--border", choices=sorted(SMOOTH_BORDERS), default="fixed")
    ap.add_argument("--normals", action="store_true")
    args = ap.parse_args()
    vtx, faces = read_ply(args.ply_in)
    h = capi.HotPath(capi.load_hip_library(), capi.avia_config(cap_root_voxels=1 << 12, cap_scan_points=200000, cap_vertices=1 << 18, cap_triangles=1 << 20), "immesh_")
    try:
        h.raycast_build_triangles(vtx, faces)
        st = h.smooth(args.steps, args.lam, args.mu, SMOOTH_BORDERS[args.border])
        out = h.smooth_vertices()["vtx"]
        ms = h.smooth_last_timing()
        extra = {}
        normals = None
        if args.normals:
            h.smooth_apply()                                                            # the normals are of the caster's snapshot
            normals, extra["n_zero_normals"] = h.vertex_normals()
        write_ply(args.ply_out, out, faces, normals)
    finally:
        h.close()
    print(json.dumps({"lambda": args.lam, "mu": args.mu, "border": args.border, **{n: getattr(st, n) for n, _ in capi.SmoothStats._fields_}, **extra,
                      "one_ring_ms": round(ms[0], 4), "steps_ms": round(ms[1], 4)}), flush=True)


if __name__ == "__main__":
    main()
