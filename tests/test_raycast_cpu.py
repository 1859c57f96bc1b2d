"""CPU tier of the ray caster (include/immesh_raycast.h): the header as plain C99, the library's new symbols, immesh_ray_frame's layout, the
host-only frame entry point against numpy, the brute-force checker (tests/raycast_checker.py) against closed forms, and the checker against the
renderer's checker on the pixel rays of a pinhole camera."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import raycast_checker as rcc
import render_checker as rck
from immesh_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "immesh_raycast.h")
I3, Z3 = np.eye(3), np.zeros(3)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(capi.hip_library_path()):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "immesh_amd", "csrc"), "-j8"])
    return capi.load_hip_library()


# ---- the boundary ----------------------------------------------------------------------------------------------------------------------------
def test_header_is_plain_c99(tmp_path):
    src = tmp_path / "alone.c"
    src.write_text('#include "immesh_raycast.h"\nint main(void) { immesh_ray_frame f; f.pos[0] = 0.0; return (int)f.pos[0] + IMMESH_RAY_NEAREST; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "alone.o")])


def test_c_api_header_does_not_include_it():
    assert "immesh_raycast.h" not in open(os.path.join(ROOT, "include", "immesh_c_api.h")).read()


def test_library_exports_every_declared_symbol(lib):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    fns = sorted(set(re.findall(r"\b(immesh_[a-z_0-9]+)\s*\(", src)))
    for must in ("immesh_ray_frame_from_state", "immesh_raycaster_create", "immesh_raycaster_destroy", "immesh_raycast_build_triangles",
                 "immesh_raycast_build_mesh", "immesh_raycast_sizes", "immesh_raycast", "immesh_raycast_points", "immesh_raycaster_last_timing"):
        assert must in fns
    missing = [f for f in fns if not hasattr(lib, f)]
    assert not missing, missing


def test_ray_frame_layout(tmp_path):
    prog = tmp_path / "layout.c"
    prog.write_text('#include "immesh_raycast.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void) {\n'
                    '  printf("%zu %zu %zu", sizeof(immesh_ray_frame), offsetof(immesh_ray_frame, rot), offsetof(immesh_ray_frame, pos));\n  return 0;\n}\n')
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(prog), "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe]).split()]
    assert got == [C.sizeof(capi.RayFrame), capi.RayFrame.rot.offset, capi.RayFrame.pos.offset] == [96, 0, 72]


def test_ray_frame_from_state_matches_numpy(lib):
    rng = np.random.default_rng(11)
    f = lib.immesh_ray_frame_from_state; f.argtypes = [C.POINTER(capi.Config), C.c_void_p, C.POINTER(capi.RayFrame)]; f.restype = C.c_int
    for _ in range(20):
        cfg = capi.avia_config()
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        cfg.extR[:] = [float(x) for x in q.reshape(-1)]
        cfg.extT[:] = [float(x) for x in rng.normal(size=3)]
        R, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        t = rng.normal(scale=30.0, size=3)
        st = capi.make_state(R=R, t=t)
        fr = capi.RayFrame()
        assert f(C.byref(cfg), st.ctypes.data_as(C.c_void_p), C.byref(fr)) == 0
        Rs, ts = st[:9].reshape(3, 3), st[9:12]
        E, T = np.array(list(cfg.extR)).reshape(3, 3), np.array(list(cfg.extT))
        rot = np.array([[(Rs[i, 0] * E[0, j] + Rs[i, 1] * E[1, j]) + Rs[i, 2] * E[2, j] for j in range(3)] for i in range(3)])
        pos = np.array([((Rs[i, 0] * T[0] + Rs[i, 1] * T[1]) + Rs[i, 2] * T[2]) + ts[i] for i in range(3)])
        assert np.array(list(fr.rot)).tobytes() == rot.reshape(-1).tobytes()
        assert np.array(list(fr.pos)).tobytes() == pos.tobytes()
    assert f(None, None, None) == capi.E_INVAL


# ---- closed forms of the checker -------------------------------------------------------------------------------------------------------------
def _tri(z, half=1.0):
    """a triangle in the plane z = -z around the -z axis, and a second one sharing its edge 0-1 (y = -half) and its vertex 0"""
    vtx = np.array([[-half, -half, -z], [half, -half, -z], [0.0, half, -z], [0.0, -3 * half, -z], [-3 * half, 0.0, -z]], np.float32)
    return vtx, np.array([[0, 1, 2], [1, 0, 3], [0, 4, 3]], np.int32)


def _cast(dirs, vtx, faces, origins=None, t_min=0.0, t_max=100.0, rot=I3, pos=Z3, mode=rcc.NEAREST):
    return rcc.cast(rot, pos, np.asarray(dirs, np.float32).reshape(-1, 3), origins, t_min, t_max, vtx, faces, mode=mode, threads=1)


def test_head_on_power_of_two():
    vtx, faces = _tri(4.0)
    t, f = _cast([[0, 0, -1], [0, 0, -2], [0, 0, 1], [0, 0, 0], [np.nan, 0, -1], [5, 0, -1]], vtx, faces[:1])
    assert t.tolist() == [4.0, 2.0, -1.0, -1.0, -1.0, -1.0] and f.tolist() == [0, 0, -1, -1, -1, -1]      # t in units of |d|; behind, zero, NaN, wide
    # a rotated, shifted frame that maps the same sensor ray onto the same world ray
    rot = np.array([[0.0, 0, 1], [0, 1, 0], [-1, 0, 0]])                                              # sensor +x -> world -z
    t, f = _cast([[1, 0, 0]], vtx, faces[:1], rot=rot, pos=np.array([0.0, 0.0, 4.0]))
    assert t.tolist() == [8.0] and f.tolist() == [0]
    t, f = _cast([[1, 0, 0]], vtx, faces[:1], origins=np.array([[-4.0, 0, 0]], np.float32), rot=rot, pos=np.array([0.0, 0.0, 4.0]))
    assert t.tolist() == [12.0] and f.tolist() == [0]                                                 # the origin moves 4 back along the ray
    ta, fa = _cast([[0, 0, -1], [5, 0, -1]], vtx, faces[:1], mode=rcc.ANY)
    assert ta.tolist() == [0.0, -1.0] and fa.tolist() == [0, -1]


def test_range_ends():
    vtx, faces = _tri(4.0)
    d = [[0, 0, -1]]
    assert _cast(d, vtx, faces[:1], t_min=4.0, t_max=8.0)[1].tolist() == [0]          # s == t_min counts
    assert _cast(d, vtx, faces[:1], t_min=0.0, t_max=4.0)[1].tolist() == [-1]         # s == t_max does not
    assert _cast(d, vtx, faces[:1], t_min=np.nextafter(4.0, 5.0), t_max=8.0)[1].tolist() == [-1]
    assert _cast(d, vtx, faces[:1], t_min=0.0, t_max=np.nextafter(4.0, 5.0))[1].tolist() == [0]


def test_origin_in_the_face_plane_is_distance_plus_zero():
    """s = -0 (na = +0, nd < 0) with t_min = 0: the distance +0, nearer than any face behind it, whatever the face order"""
    vtx, faces = _tri(4.0)
    far = (vtx + np.array([0, 0, -3], np.float32)).astype(np.float32)
    both = np.concatenate([far, vtx])
    fc = np.concatenate([faces[:1], faces[:1] + 5]).astype(np.int32)
    for d in ([0, 0, -1], [0, 0, 1]):
        t, f = _cast([d], both, fc, origins=np.array([[0, 0, -4]], np.float32))
        assert f.tolist() == [1] and t.view(np.uint32).tolist() == [0]
    t, f = _cast([[0, 0, -1]], both, fc, origins=np.array([[0, 0, -4]], np.float32), t_min=2.0 ** -20)
    assert f.tolist() == [0] and t.tolist() == [3.0]


def test_shared_edge_and_vertex_take_the_lower_index():
    vtx, faces = _tri(4.0)
    # (0, -1, -4) is the midpoint of the edge 0-1 shared by faces 0 and 1; (-1, -1, -4) is vertex 0, shared by all three
    t, f = _cast([[0, -1, -4], [-1, -1, -4]], vtx, faces)
    assert f.tolist() == [0, 0] and t.tolist() == [1.0, 1.0]
    t, f = _cast([[0, -1, -4], [-1, -1, -4]], vtx, faces[1:])
    assert f.tolist() == [0, 0]                                                        # without face 0 the next lower index takes both
    t, f = _cast([[0, -1, -4], [-1, -1, -4]], vtx, faces[2:])
    assert f.tolist() == [-1, 0]                                                       # the last face holds the vertex only
    order = np.array([2, 1, 0])
    t, f = _cast([[0, -1, -4], [-1, -1, -4]], vtx, faces[order])
    assert f.tolist() == [1, 0]                                                        # the index decides, not the face


def test_axis_parallel_ray_on_the_box_plane():
    """d = (0, 0, -1): x and y do not bound t; the origin must lie inside the face's box on them, planes included"""
    vtx = np.array([[0, 0, -2], [1, 0, -2], [1, 1, -2], [0, 1, -2]], np.float32)
    faces = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    org = np.array([[0, 0.5, 0], [1, 0.5, 0], [0.5, 0, 0], [0.5, 1, 0], [0, 0, 0], [1, 1, 0], [np.nextafter(np.float32(1), np.float32(2)), 0.5, 0],
                    [np.nextafter(np.float32(0), np.float32(-1)), 0.5, 0], [0.5, 0.5, 0]], np.float32)
    t, f = _cast(np.tile([[0, 0, -1]], (len(org), 1)), vtx, faces, origins=org)
    assert f.tolist() == [1, 0, 0, 1, 0, 0, -1, -1, 0]
    assert t[f >= 0].tolist() == [2.0] * 7
    # a ray lying in the face's plane: nd == 0, never a hit, although the box test passes
    t, f = _cast([[1, 0, 0]], vtx, faces, origins=np.array([[-1, 0.5, -2]], np.float32))
    assert f.tolist() == [-1]


def test_degenerate_and_nan_faces_never_hit():
    vtx = np.array([[-1, -1, -4], [1, -1, -4], [0, 1, -4], [0, 0, -4], [np.nan, 0, -4], [0, 3, -4]], np.float32)
    rays_ = [[0, 0, -1], [0, -1, -4], [0, 0.25, -1]]
    for face in ([0, 1, 1], [0, 0, 0], [3, 3, 3], [0, 1, 4], [4, 4, 4], [2, 3, 5]):   # repeated vertex, a point, collinear, NaN vertex
        t, f = _cast(rays_, vtx, np.array([face], np.int32))
        assert f.tolist() == [-1, -1, -1] and t.tolist() == [-1.0, -1.0, -1.0], face
    t, f = _cast(rays_, vtx, np.array([[0, 1, 4], [0, 1, 2]], np.int32))
    assert f.tolist() == [1, 1, 1]                                                     # the NaN face keeps its index; the others' do not shift
    with pytest.raises(ValueError):
        _cast(rays_, vtx, np.array([[0, 1, 6]], np.int32))


def test_points_rule():
    vtx, faces = _tri(4.0)
    dirs = np.array([[0, 0, -1], [5, 0, -1], [0.001, 0, -1], [0.0625, 0, -1]], np.float32)
    pos = np.array([10.0, 20.0, 30.0])
    v2 = (vtx.astype(np.float64) + pos).astype(np.float32)
    t, f = _cast(dirs, v2, faces[:1], pos=pos)
    assert f.tolist() == [0, -1, 0, 0]
    pts = rcc.points(I3, pos, dirs, None, t, 0.0)
    assert np.array_equal(pts, np.array([[10, 20, 26], [10.004, 20, 26], [10.25, 20, 26]], np.float32))
    assert len(rcc.points(I3, pos, dirs, None, t, 0.05)) == 2                          # the second hit falls into the first one's cell
    assert np.array_equal(rcc.points(I3, pos, dirs, None, t, 0.05), pts[[0, 2]])


# ---- the two checkers on a pinhole camera's rays -------------------------------------------------------------------------------------------------
def pinhole_soup(seed, n_faces, spread=20.0, size=0.25):
    """random triangles at least 6 m from the origin (test_gpu_render's _soup without its awkward cases): no degenerate faces, none edge-on to a
    camera within 2 m of the origin, none crossing its z_near"""
    rng = np.random.default_rng(seed)
    centres = rng.uniform(-spread, spread, (n_faces, 3))
    near = np.linalg.norm(centres, axis=1) < 6.0
    centres[near] *= (6.0 / np.maximum(np.linalg.norm(centres[near], axis=1), 1e-3))[:, None]
    vtx = (centres[:, None, :] + rng.normal(scale=size, size=(n_faces, 3, 3))).reshape(-1, 3).astype(np.float32)
    return vtx, np.arange(3 * n_faces, dtype=np.int32).reshape(-1, 3)


def pinhole_camera(seed, width, height, focus):
    rng = np.random.default_rng(seed)
    cam = capi.Camera()
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    cam.rot[:] = [float(x) for x in q.reshape(-1)]
    cam.pos[:] = [float(x) for x in rng.uniform(-1, 1, 3)]
    cam.width, cam.height, cam.focus, cam.z_near, cam.z_far, cam.downsample_res = width, height, focus, 0.05, 200.0, 0.01
    return cam


def pinhole_rays(cam):
    """the renderer's Ray rule for every pixel, as floats -- exact only where (u - cx) / f is a float: focus a power of two"""
    u, v = np.meshgrid(np.arange(cam.width), np.arange(cam.height))
    cx, cy = cam.width // 2, cam.height // 2
    dirs = np.stack([(u - cx).astype(np.float64) / cam.focus, -((v - cy).astype(np.float64) / cam.focus), np.full(u.shape, -1.0)], axis=-1).reshape(-1, 3)
    d32 = dirs.astype(np.float32)
    assert np.array_equal(d32.astype(np.float64), dirs)
    return d32


def pinhole_differences(cam, vtx, faces, t, f):
    """pixels where a cast on the pixel rays (t, f) and the renderer's checker differ, under the renderer's 0.99 z_far cut"""
    depth, face = rck.render(cam, vtx, faces)
    depth, face = depth.reshape(-1), face.reshape(-1)
    seen = depth >= 0
    bad = seen & ((depth.view(np.uint32) != t.view(np.uint32)) | (face != f))
    cut = ~seen & ~((f < 0) | (t.astype(np.float64) >= 0.99 * cam.z_far))          # -1 in the image: a miss, or a hit behind the cut
    return int(bad.sum() + cut.sum()), int(seen.sum())


PINHOLE = dict(soup_seed=5, cam_seed=6, n_faces=1000, size=0.5)   # (test_gpu_raycast casts the same soup from the same pose at 640 x 480)


def test_pinhole_cross_check_of_the_two_checkers():
    """64 x 48 pixel rays cast by the brute-force checker == the renderer's checker's image: zero differing pixels"""
    cam = pinhole_camera(PINHOLE["cam_seed"], 64, 48, 32.0)
    vtx, faces = pinhole_soup(PINHOLE["soup_seed"], PINHOLE["n_faces"], size=PINHOLE["size"])
    t, f = rcc.cast(np.array(list(cam.rot)).reshape(3, 3), np.array(list(cam.pos)), pinhole_rays(cam), None, cam.z_near, cam.z_far, vtx, faces)
    n_diff, n_seen = pinhole_differences(cam, vtx, faces, t, f)
    assert n_seen > 0.05 * 64 * 48, n_seen
    assert n_diff == 0, n_diff
