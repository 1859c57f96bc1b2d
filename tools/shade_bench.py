"""Timings of the colour pass behind the renderer (include/immesh_shade.h) beside the same call's rasterize time:
  live   the GPU tests' live mesh (four synthetic Livox scans of 40 000 points, coloured by two 320 x 240 frames), immesh_shade_mesh at 640 x 480
  soup   the render tests' one-million-face soup (tests/test_gpu_render.py::test_scale_one_million_faces: seed 7, spread 30, size 0.3),
         immesh_shade_triangles at 1920 x 1080
Every source, light on; medians over --reps calls after --warmup calls; HIP events on the renderer's stream (immesh_renderer_last_shade_ms,
immesh_renderer_last_timing).  One JSON object on stdout, and in --out when given.

    python tools/shade_bench.py [--reps 20] [--warmup 3] [--out profiles/shade_timing.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from immesh_amd import capi, synth  # noqa: E402

BASE = np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])
# axis: the range from the vertices (the min / max reduction runs); axis_given: the caller's range (it does not)
SOURCES = (("white", capi.SHADE_WHITE, {}), ("axis", capi.SHADE_AXIS, {}), ("axis_given", capi.SHADE_AXIS, dict(axis_min=-50.0, axis_max=50.0)),
           ("vertex", capi.SHADE_VERTEX, {}))


def _rand_rot(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def _soup(rng, n_faces, spread, size):
    """the render tests' soup (their _soup, same draws in the same order)"""
    centres = rng.uniform(-spread, spread, (n_faces, 3))
    near = np.linalg.norm(centres, axis=1) < 6.0
    centres[near] *= (6.0 / np.maximum(np.linalg.norm(centres[near], axis=1), 1e-3))[:, None]
    vtx = (centres[:, None, :] + rng.normal(scale=size, size=(n_faces, 3, 3))).reshape(-1, 3).astype(np.float32)
    faces = np.arange(3 * n_faces, dtype=np.int32).reshape(-1, 3)
    k = n_faces // 50
    idx = rng.choice(n_faces, size=6 * k, replace=False)
    d0, d1, d2, d3, d4, d5 = np.split(idx, 6)
    faces[d0, 2] = faces[d0, 1]
    v = vtx.reshape(-1, 3, 3)
    v[d1, 2] = v[d1, 0] + np.float32(2.0) * (v[d1, 1] - v[d1, 0])
    v[d2, :, 2] = v[d2, :1, 2]
    v[d3, 1, 0] = np.nan
    v[d4, :, 2] = np.array([0.02, -1.0, -3.0], np.float32)
    faces[d5] = faces[(d5 + 1) % n_faces]
    return vtx, faces


def _image(h, R, t, seed):
    y, x = np.mgrid[0:240, 0:320]
    px = np.stack([x * 255 // 319, y * 255 // 239, (x * 3 + y * 5 + seed * 37) % 256], axis=-1).astype(np.uint8)
    return h.default_image(px, fx=300.0, fy=300.0, cx=159.7, cy=120.2, rot=R @ BASE, pos=t, obs_time=0.1 * seed, inv_exposure=0.01 + 0.002 * seed)


def _measure(call, h, reps, warmup):
    shade, rast, rein = [], [], []
    for k in range(warmup + reps):
        face = call()
        if k >= warmup:
            shade.append(h.shade_timing())
            a, b = h.render_timing()
            rast.append(a); rein.append(b)
    med = lambda x: round(float(np.median(x)), 4)   # noqa: E731
    return {"shade_ms_median": med(shade), "shade_ms_min": round(float(np.min(shade)), 4), "rasterize_ms_median": med(rast),
            "reinforce_ms_median": med(rein), "covered_fraction": round(float((face >= 0).mean()), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    hip = capi.load_hip_library()
    cfg = capi.avia_config(cap_root_voxels=1 << 12, cap_scan_points=200000, cap_vertices=1 << 18, cap_triangles=1 << 20)
    h = capi.HotPath(hip, cfg, "immesh_")
    out = {"metric": "colour pass (immesh_renderer_last_shade_ms) beside the same call's rasterize (immesh_renderer_last_timing)", "unit": "ms",
           "reps": args.reps, "warmup": args.warmup, "light": 1}
    # ---- live mesh, 640 x 480
    extT = np.array(list(cfg.extT))
    for k in range(4):
        R, t = synth.trajectory_pose(k)
        raw = synth.livox_scan(k, R, t, n_pts=40000, extT=extT)
        pw = (raw[:, :3].astype(np.float64) + extT) @ R.T + t
        pts = raw.copy(); pts[:, :3] = pw.astype(np.float32)
        h.mesh_scan(np.ascontiguousarray(pts), t, frame_idx=k, fetch=False)
    cam = h.camera_from_state(capi.make_state(R=R, t=t))
    h.colour_image(_image(h, R, t, 1), capi.COLOUR_PLAIN, capi.COLOUR_SET_ALL)
    h.colour_image(_image(h, R @ synth.yaw_R(0.25), t, 2), capi.COLOUR_PLAIN, capi.COLOUR_SET_ALL)
    vtx, faces = h.mesh_export(1.0, 20)
    live = {"vertices": int(len(vtx)), "faces": int(len(faces)), "size": "640x480"}
    for name, source, over in SOURCES:
        sh = h.default_shade(source=source, min_views=1, **over)
        live[name] = _measure(lambda: h.shade_mesh(cam, sh, 1.0, 20, want_rgb=True, want_depth=False)[2], h, args.reps, args.warmup)
    out["live_mesh"] = live
    # ---- one million faces, 1920 x 1080
    rng = np.random.default_rng(7)
    vtx, faces = _soup(rng, 1 << 20, 30.0, 0.3)
    cam = h.default_depth_camera(width=1920, height=1080)
    cam.rot[:] = _rand_rot(rng).reshape(-1)
    col = rng.integers(0, 256, (len(vtx), 3)).astype(np.uint8)
    soup = {"vertices": int(len(vtx)), "faces": int(len(faces)), "size": "1920x1080"}
    for name, source, over in SOURCES:
        sh = h.default_shade(source=source, **over)
        soup[name] = _measure(lambda: h.shade_triangles(cam, vtx, faces, sh, vtx_rgb=col if source == capi.SHADE_VERTEX else None, want_depth=False)[2],
                              h, args.reps, args.warmup)
    out["soup_1m"] = soup
    h.close()
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as fp:
            json.dump(out, fp, indent=1)


if __name__ == "__main__":
    main()
