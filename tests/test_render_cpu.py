"""CPU tier of the mesh depth renderer (include/immesh_render.h): the numpy checker against closed forms, its thinning against a plain dict loop,
the library's new symbols and immesh_camera's layout, and the host-only camera entry points against a numpy restatement of get_last_avr_pose."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import render_checker as rck
from immesh_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "immesh_render.h")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(capi.hip_library_path()):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "immesh_amd", "csrc"), "-j8"])
    return capi.load_hip_library()


def _cam(lib, **over):
    return capi.default_depth_camera(lib, **over)


def _quad(z, half=2.0):
    """fronto-parallel square at depth z in front of a camera at the origin; faces (0,1,2), (0,2,3) share the diagonal 0-2"""
    vtx = np.array([[-half, -half, -z], [half, -half, -z], [half, half, -z], [-half, half, -z]], np.float32)
    return vtx, np.array([[0, 1, 2], [0, 2, 3]], np.int32)


def test_fronto_parallel_quad(lib):
    cam = _cam(lib, width=64, height=48, focus=20.0)
    vtx, faces = _quad(3.7)
    depth, face = rck.render(cam, vtx, faces)
    cov = depth >= 0
    assert cov.sum() == 21 * 21 and np.all(depth[cov] == np.float32(3.7)) and np.all(face[~cov] == -1)
    # the shared diagonal: pixels with (u - cx) == -(v - cy) lie exactly on it; both faces cover them, the lower index wins
    _, f1 = rck.render(cam, vtx, faces[1:])
    diag = [(cam.height // 2 - k, cam.width // 2 + k) for k in range(-10, 11)]
    assert all(f1[v, u] == 0 for v, u in diag)                           # face 1 alone covers the diagonal ...
    assert all(face[v, u] == 0 for v, u in diag)                         # ... and face 0 wins it
    assert np.array_equal(rck.render(cam, vtx, faces, brute=True)[1], face)


def test_tilted_plane(lib):
    """plane depth s = z0 + alpha x: along the pixel ray (dx, dy, -1) the closed form is s = z0 / (1 - alpha dx)"""
    cam = _cam(lib, width=80, height=60, focus=50.0)
    z0, alpha = 5.0, 0.4
    xs = np.array([-3.0, 3.0])
    ys = np.array([-3.0, 3.0])
    P = [(x, y, -(z0 + alpha * x)) for y in ys for x in xs]
    vtx = np.array(P, np.float32)
    faces = np.array([[0, 1, 3], [0, 3, 2]], np.int32)
    depth, _ = rck.render(cam, vtx, faces)
    vv, uu = np.nonzero(depth >= 0)
    assert len(uu) > 1000
    # the plane through the float vertices: s = -(z(x)) with z linear in x; fit from the float vertices
    a = (float(vtx[1, 2]) - float(vtx[0, 2])) / (float(vtx[1, 0]) - float(vtx[0, 0]))
    b = float(vtx[0, 2]) - a * float(vtx[0, 0])
    dx = (uu - cam.width // 2) / cam.focus
    closed = (-b) / (1.0 + a * dx)
    np.testing.assert_allclose(depth[vv, uu], closed, rtol=2e-7, atol=0)


def test_face_straddling_the_near_plane(lib):
    cam = _cam(lib, width=64, height=64, focus=30.0, z_near=0.5)
    vtx = np.array([[0.0, 0.0, -0.1], [1.5, -1.0, -3.0], [-1.5, -1.0, -3.0]], np.float32)
    faces = np.array([[0, 1, 2]], np.int32)
    depth, face = rck.render(cam, vtx, faces)
    cov = depth >= 0
    assert cov.sum() > 40 and depth[cov].min() >= np.float32(0.5)
    assert depth[0:cam.height // 2 - 2].max() < 0            # the rays above the centre meet the plane nearer than z_near or not at all
    # pixels near the vertex in front of z_near are cut, and the clipped box loses nothing against every pixel of the image
    bd, bf = rck.render(cam, vtx, faces, brute=True)
    assert np.array_equal(bd.view(np.uint32), depth.view(np.uint32)) and np.array_equal(bf, face)


def test_face_behind_the_camera(lib):
    cam = _cam(lib, width=32, height=32, focus=16.0)
    vtx = np.array([[-1.0, -1.0, 2.0], [1.0, -1.0, 2.0], [0.0, 1.0, 2.0]], np.float32)      # +z: behind a camera looking along -z
    depth, face = rck.render(cam, vtx, np.array([[0, 1, 2]], np.int32))
    assert np.all(depth == -1) and np.all(face == -1)
    bd, _ = rck.render(cam, vtx, np.array([[0, 1, 2]], np.int32), brute=True)
    assert np.all(bd == -1)                                              # its mirror image through the centre is not drawn either
    # one vertex behind, two in front: only the part in front, and the box agrees with every pixel
    vtx2 = np.array([[0.0, 0.0, 1.0], [1.0, -1.0, -2.0], [-1.0, -1.0, -2.0]], np.float32)
    d2, f2 = rck.render(cam, vtx2, np.array([[0, 1, 2]], np.int32))
    b2, g2 = rck.render(cam, vtx2, np.array([[0, 1, 2]], np.int32), brute=True)
    assert (d2 >= 0).sum() > 20 and np.array_equal(d2.view(np.uint32), b2.view(np.uint32)) and np.array_equal(f2, g2)


def test_far_cut(lib):
    """depth is kept only where (double)d32 < 0.99 z_far (convert_depth_buffer_to_truth_depth)"""
    cam = _cam(lib, width=32, height=32, focus=16.0, z_far=100.0)
    for z, kept in ((98.9, True), (99.0, False), (99.5, False)):
        vtx, faces = _quad(z, half=z)
        depth, face = rck.render(cam, vtx, faces)
        assert (depth >= 0).all() == kept and (face >= 0).all() == kept, z


def test_thinning_matches_dict_loop():
    rng = np.random.default_rng(3)
    pts = rng.normal(scale=0.05, size=(20000, 3)).astype(np.float32)
    pts[::7] = pts[::7].round(2)                                          # many points on cell boundaries
    pts[5::11] = -pts[5::11]
    for res in (0.01, 0.003, 0.05):
        assert np.array_equal(rck.thin(pts, res), rck.thin_naive(pts, res)), res
    assert np.array_equal(rck.thin(pts, 0.0), np.arange(len(pts)))
    # half-way values round away from zero (std::round), -0 and +0 are one cell
    q = np.array([[0.5, -0.5, 1.5], [-0.4, 0.4, -0.0], [0.0, 0.0, 0.0], [0.6, -0.6, 1.5]], np.float32)
    assert rck.cells(q, 1.0).tolist() == [[1.0, -1.0, 2.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [1.0, -1.0, 2.0]]
    assert rck.thin(q, 1.0).tolist() == [0, 1] == rck.thin_naive(q, 1.0).tolist()


def _render_functions():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(immesh_[a-z_0-9]+)\s*\(", src)))


def test_library_exports_render_symbols(lib):
    fns = _render_functions()
    for must in ("immesh_default_depth_camera", "immesh_camera_from_state", "immesh_renderer_create", "immesh_renderer_destroy",
                 "immesh_render_triangles", "immesh_render_mesh", "immesh_render_points", "immesh_renderer_last_timing"):
        assert must in fns
    missing = [f for f in fns if not hasattr(lib, f)]
    assert not missing, missing
    assert '#include "immesh_render.h"' in open(os.path.join(ROOT, "include", "immesh_c_api.h")).read()


def test_camera_layout_matches_header(tmp_path):
    """immesh_camera's field order from the header, sizes and offsets from a C compiler"""
    src = open(HEADER).read()
    body = src[src.index("typedef struct immesh_camera {"):src.index("} immesh_camera;")]
    names = []
    for decl in re.findall(r"\b(?:double|int32_t)\s+([^;]+);", body):
        names += [re.sub(r"\[\d+\]", "", n).strip() for n in decl.split(",")]
    assert names == [n for n, _ in capi.Camera._fields_]
    prog = tmp_path / "layout.c"
    prog.write_text('#include "immesh_c_api.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void) {\n  printf("%zu", sizeof(immesh_camera));\n' +
                    "".join(f'  printf(" %zu", offsetof(immesh_camera, {n}));\n' for n in names) + "  return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(prog), "-o", exe])
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == C.sizeof(capi.Camera)
    assert got[1:] == [getattr(capi.Camera, n).offset for n in names]


def _quat_from_rot(R):
    w = np.sqrt(max(0.0, 1.0 + R[0, 0] + R[1, 1] + R[2, 2])) / 2
    x = np.copysign(np.sqrt(max(0.0, 1.0 + R[0, 0] - R[1, 1] - R[2, 2])) / 2, R[2, 1] - R[1, 2])
    y = np.copysign(np.sqrt(max(0.0, 1.0 - R[0, 0] + R[1, 1] - R[2, 2])) / 2, R[0, 2] - R[2, 0])
    z = np.copysign(np.sqrt(max(0.0, 1.0 - R[0, 0] - R[1, 1] + R[2, 2])) / 2, R[1, 0] - R[0, 1])
    return np.array([w, x, y, z])


def _rot_from_quat(q):
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def test_camera_from_state_and_default(lib):
    cam = capi.default_depth_camera(lib)
    assert (cam.width, cam.height, cam.focus, cam.z_near, cam.z_far) == (640, 480, 400.0, 0.05, 200.0)
    assert cam.downsample_res == 0.01 and list(cam.rot) == [1, 0, 0, 0, 1, 0, 0, 0, 1] and list(cam.pos) == [0, 0, 0]
    M = np.array([[0, 0, -1], [-1, 0, 0], [0, 1, 0]], float)          # lidar_frame_to_camera_frame
    rng = np.random.default_rng(11)
    for _ in range(20):
        q, r = np.linalg.qr(rng.normal(size=(3, 3)))
        R = q * np.sign(np.diag(r))
        if np.linalg.det(R) < 0:
            R[:, 0] = -R[:, 0]
        t = rng.uniform(-50, 50, 3)
        c = capi.camera_from_state(lib, capi.make_state(R=R, t=t), capi.default_depth_camera(lib, width=320))
        rot = np.array(c.rot).reshape(3, 3)
        assert np.array_equal(rot, R @ M) and np.array_equal(np.array(c.pos), t)
        assert c.width == 320 and c.height == 480                       # the pose only
        # get_last_avr_pose with its one-frame window: q_avr = q_first * exp(log(q_first^-1 q_first) / 1) = q_first, then q_avr * M
        q_first = _quat_from_rot(R)
        np.testing.assert_allclose(rot, _rot_from_quat(q_first) @ M, rtol=0, atol=1e-12)
        # GL convention: the camera looks along its -z = the LiDAR's +x, its +y is the LiDAR's +z
        np.testing.assert_allclose(rot @ [0, 0, -1], R[:, 0], atol=1e-15)
        np.testing.assert_allclose(rot @ [0, 1, 0], R[:, 2], atol=1e-15)
