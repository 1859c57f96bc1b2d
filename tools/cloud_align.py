"""Align cloud B to cloud A on the device (include/immesh_align.h, the Cloud rule): A is indexed (and given normals from its K nearest neighbours for
plane rows), B is refined from the identity by nearest-point least squares, linearised about its mean.  It refines a pose that is already within
--max-dist; it is no global registration.

    python tools/cloud_align.py A.ply B.npy [--mode point|plane] [--normals K] [--huber H] [--max-dist D] [--iters N] [--out B_moved.npy] [--json OUT]

A and B: .npy of shape (n, >= 3), or .ply with float x, y, z as the vertex element's first three properties (ascii or binary little-endian).  It
prints the frame, the status, the iterations, the fitness n_used / n_pts and the rms, and writes B moved (.npy or .ply by the name given).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from immesh_amd import capi  # noqa: E402

MODES = {"point": capi.ALIGN_POINT, "plane": capi.ALIGN_PLANE}
PLY_TYPES = {b"char": "i1", b"uchar": "u1", b"short": "<i2", b"ushort": "<u2", b"int": "<i4", b"uint": "<u4", b"float": "<f4", b"double": "<f8",
             b"int8": "i1", b"uint8": "u1", b"int16": "<i2", b"uint16": "<u2", b"int32": "<i4", b"uint32": "<u4", b"float32": "<f4", b"float64": "<f8"}


def read_cloud(path):
    """-> (n, 3) float32"""
    if path.endswith(".npy"):
        return np.ascontiguousarray(np.load(path)[:, :3], dtype=np.float32)
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    lines = [l.strip() for l in head.split(b"\n")]
    at = [i for i, l in enumerate(lines) if l.startswith(b"element vertex")]
    if not at or [l for l in lines[:at[0]] if l.startswith(b"element")]:
        raise ValueError(f"{path}: the vertex element is not the first one")
    n = int(lines[at[0]].split()[-1])
    props = []
    for l in lines[at[0] + 1:]:
        if not l.startswith(b"property"):
            break
        w = l.split()
        if w[1] == b"list":
            raise ValueError(f"{path}: a list property in the vertex element")
        props.append((w[2].decode(), PLY_TYPES[w[1]]))
    if [p[0] for p in props[:3]] != ["x", "y", "z"]:
        raise ValueError(f"{path}: the vertex element does not begin with x, y, z")
    if b"format ascii" in head:
        rows = np.array(body.split()[:n * len(props)], dtype=np.float64).reshape(n, len(props))
        return np.ascontiguousarray(rows[:, :3], dtype=np.float32)
    if b"format binary_little_endian" not in head:
        raise ValueError(f"{path}: neither ascii nor binary little-endian")
    rec = np.frombuffer(body, np.dtype(props), count=n)
    return np.ascontiguousarray(np.stack([rec["x"], rec["y"], rec["z"]], axis=-1), dtype=np.float32)


def write_cloud(path, pts):
    pts = np.ascontiguousarray(pts, dtype=np.float32)
    if path.endswith(".npy"):
        np.save(path, pts)
        return
    with open(path, "wb") as fp:
        fp.write(b"ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\nend_header\n" % len(pts))
        fp.write(pts.astype("<f4").tobytes())


def align(h, a, b, mode="plane", normals=16, huber=0.0, max_dist=1.0, max_iters=50, normals_max_dist=None):
    """h: a HotPath -> (B moved (n, 3) float32, a dict: frame, status, iterations, fitness, rms and the history)"""
    a, b = np.ascontiguousarray(a, np.float32).reshape(-1, 3), np.ascontiguousarray(b, np.float32).reshape(-1, 3)
    n, n_in = h.cloud_index_build(a)
    block = {"mode": mode, "huber": huber, "max_dist": max_dist, "max_iters": max_iters, "target_points": n, "target_points_indexed": n_in, "points": len(b)}
    if mode == "plane":
        nr = h.cloud_normals(normals, max_dist if normals_max_dist is None else normals_max_dist, want=())
        block["normals"] = {"k": normals, "with_normal": nr["with_normal"], "too_few": nr["too_few"], "line_like": nr["line_like"]}
    centre = capi.align_centre_mean(b)
    res, hist = h.align_cloud(b, capi.align_options(mode=MODES[mode], max_dist=max_dist, centre=centre, max_iters=max_iters), huber)
    rot, pos = np.array(list(res.frame.rot)).reshape(3, 3), np.array(list(res.frame.pos))
    moved = (b.astype(np.float64) @ rot.T + pos).astype(np.float32)
    block.update({"centre": centre, "status": capi.ALIGN_STATUS[res.status], "iterations": res.iterations, "rot": rot.reshape(-1).tolist(), "pos": pos.tolist(),
                  "fitness": res.system.n_used / max(len(b), 1), "rms": res.rms, "points_used": [int(v) for v in hist[:, 0]], "rms_history": hist[:, 1].tolist(),
                  "no_neighbour": res.system.n_no_face, "winner_without_normal": res.system.n_flat, "not_finite": res.system.n_not_finite,
                  "device_ms": h.align_cloud_timing()[1]})
    return moved, block


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("a", help="the target cloud A (.npy or .ply)")
    ap.add_argument("b", help="the cloud B that is moved (.npy or .ply)")
    ap.add_argument("--mode", choices=sorted(MODES), default="plane")
    ap.add_argument("--normals", type=int, default=16, metavar="K", help="plane rows: A's normals from its K nearest neighbours (2 .. 64)")
    ap.add_argument("--normals-max-dist", type=float, default=None, metavar="D", help="... within D (--max-dist)")
    ap.add_argument("--huber", type=float, default=0.0, metavar="H", help="down-weight the pairs whose distance (point) or plane residual (plane) exceeds H (0: off)")
    ap.add_argument("--max-dist", type=float, default=1.0, metavar="D", help="pairs farther apart do not take part")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default="", help="write B moved here (.npy or .ply)")
    ap.add_argument("--json", default="", help="write the printed block here too")
    args = ap.parse_args()
    a, b = read_cloud(args.a), read_cloud(args.b)
    h = capi.HotPath(capi.load_hip_library(), capi.avia_config(cap_root_voxels=1 << 12, cap_scan_points=200000, cap_vertices=1 << 18, cap_triangles=1 << 20), "immesh_")
    try:
        moved, block = align(h, a, b, args.mode, args.normals, args.huber, args.max_dist, args.iters, args.normals_max_dist)
    finally:
        h.close()
    print("frame rot", np.array(block["rot"]).reshape(3, 3).tolist(), "pos", block["pos"])
    print("status", block["status"], "iterations", block["iterations"], "fitness", round(block["fitness"], 6), "rms", block["rms"])
    if args.out:
        write_cloud(args.out, moved)
    if args.json:
        with open(args.json, "w") as fp:
            json.dump(block, fp, indent=1)


if __name__ == "__main__":
    main()
