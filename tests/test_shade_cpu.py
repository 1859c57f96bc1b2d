"""CPU tier of the colour pass behind the renderer (include/immesh_shade.h): the library's new symbols, immesh_shade's layout and defaults, and the
numpy checker (tests/shade_checker.py) against closed forms -- the Heat table, the Lambert term of a tilted facet, a pixel on a vertex, and the
perspective-correct weight at the screen midpoint of an edge that runs from depth 1 to depth 3."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import shade_checker as sck
from immesh_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "immesh_shade.h")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(capi.hip_library_path()):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "immesh_amd", "csrc"), "-j8"])
    return capi.load_hip_library()


def _shade_functions():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(immesh_[a-z_0-9]+)\s*\(", src)))


def test_library_exports_shade_symbols(lib):
    fns = _shade_functions()
    assert fns == sorted(["immesh_default_shade", "immesh_shade_triangles", "immesh_shade_mesh", "immesh_shade_range", "immesh_renderer_last_shade_ms"])
    missing = [f for f in fns if not hasattr(lib, f)]
    assert not missing, missing
    assert '#include "immesh_shade.h"' in open(os.path.join(ROOT, "include", "immesh_c_api.h")).read()


def test_shade_layout_matches_header(tmp_path):
    """immesh_shade's field order from the header, sizes and offsets from a C compiler; the source constants"""
    src = open(HEADER).read()
    body = src[src.index("typedef struct immesh_shade {"):src.index("} immesh_shade;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in re.findall(r"\b(?:double|int32_t|uint8_t)\s+([^;]+);", body):
        names += [re.sub(r"\[\d+\]", "", n).strip() for n in decl.split(",")]
    assert names == [n for n, _ in capi.Shade._fields_]
    prog = tmp_path / "layout.c"
    prog.write_text('#include "immesh_c_api.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void) {\n  printf("%zu", sizeof(immesh_shade));\n' +
                    "".join(f'  printf(" %zu", offsetof(immesh_shade, {n}));\n' for n in names) +
                    '  printf(" %d %d %d", IMMESH_SHADE_WHITE, IMMESH_SHADE_AXIS, IMMESH_SHADE_VERTEX);\n  return 0;\n}\n')
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(prog), "-o", exe])
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == C.sizeof(capi.Shade)
    assert got[1:-3] == [getattr(capi.Shade, n).offset for n in names]
    assert got[-3:] == [capi.SHADE_WHITE, capi.SHADE_AXIS, capi.SHADE_VERTEX] == [sck.WHITE, sck.AXIS, sck.VERTEX]
    # the header on its own, before immesh_c_api.h, compiles as well
    alone = tmp_path / "alone.c"
    alone.write_text('#include "immesh_shade.h"\nint main(void) { immesh_shade s; immesh_default_shade(&s); return s.source; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "include"), str(alone), "-o", str(tmp_path / "alone.o")])


def test_default_shade(lib):
    sh = capi.Shade()
    C.memset(C.byref(sh), 0xAB, C.sizeof(sh))
    lib.immesh_default_shade.argtypes = [C.POINTER(capi.Shade)]; lib.immesh_default_shade.restype = None
    lib.immesh_default_shade(C.byref(sh))
    assert (sh.source, sh.axis, sh.light, sh.bgr, sh.min_views) == (capi.SHADE_WHITE, 2, 1, 0, 0)
    assert list(sh.background) == [0, 0, 0] and sh.pad == 0 and sh.axis_min == 0.0 and sh.axis_max == 0.0
    over = capi.default_shade(lib, source=capi.SHADE_AXIS, axis=1, background=(9, 8, 7), axis_min=-1.5, axis_max=2.5)
    assert (over.source, over.axis, list(over.background), over.axis_min, over.axis_max, over.light) == (1, 1, [9, 8, 7], -1.5, 2.5, 1)


def test_heat_table():
    """set_color_by_axis: val 0 (the lowest vertex) is red, val 1 blue, through yellow, green and cyan"""
    got = sck.heat(np.array([0.0, 0.25, 0.5, 0.75, 1.0], np.float32))
    assert got.tolist() == [[255, 0, 0], [255, 255, 0], [0, 255, 0], [0, 255, 255], [0, 0, 255]]
    # Clamp01 outside [0, 1] and std::min's answer to a NaN (x = NaN -> 1 -> the colour of val = 0); between two knots the lerp truncates
    assert sck.heat(np.array([-3.0, 7.0, np.nan], np.float32)).tolist() == [[255, 0, 0], [0, 0, 255], [255, 0, 0]]
    assert sck.heat(np.float32(0.125)).tolist() == [255, 127, 0]          # x = 0.875, a = 3.5: (1, 0.5, 0) -> 127.5 truncated
    assert sck.heat(np.float32(0.875)).tolist() == [0, 127, 255]


def test_axis_range_and_colours(lib):
    vtx = np.array([[0, 0, -2.0], [1, 0, 2.0], [np.nan, 0, 50.0], [0, np.inf, -50.0], [2, 2, 0.0]], np.float32)
    assert sck.vertex_range(vtx, 2) == (np.float32(-2.0), np.float32(2.0))           # the NaN / inf vertices do not count, on any coordinate
    assert sck.vertex_range(vtx[2:4], 2) == (0.0, 0.0)
    sh = capi.default_shade(lib, source=capi.SHADE_AXIS)
    col, lo_hi = sck.vertex_colours(vtx, sh)
    assert lo_hi == (-2.0, 2.0) and col[[0, 1, 4]].tolist() == [[255, 0, 0], [0, 0, 255], [0, 255, 0]]
    sh = capi.default_shade(lib, source=capi.SHADE_AXIS, axis_min=-6.0, axis_max=2.0)   # explicit: z = 0 sits at val 0.75
    col, lo_hi = sck.vertex_colours(vtx, sh)
    assert lo_hi == (-6.0, 2.0) and col[4].tolist() == [0, 255, 255]
    flat = np.array([[0, 0, 1.0], [1, 0, 1.0]], np.float32)                             # hi <= lo: val = 0 everywhere
    assert sck.vertex_colours(flat, capi.default_shade(lib, source=capi.SHADE_AXIS))[0].tolist() == [[255, 0, 0]] * 2
    m = np.array([[1, 2, 3], [4, 5, 6]], np.uint8)
    assert sck.vertex_colours(flat, capi.default_shade(lib, source=capi.SHADE_VERTEX, bgr=1), m)[0].tolist() == [[3, 2, 1], [6, 5, 4]]
    assert sck.vertex_colours(flat, capi.default_shade(lib, source=capi.SHADE_VERTEX), m)[0].tolist() == m.tolist()


def test_tilted_facet_is_lit_by_its_angle(lib):
    """a facet whose normal stands 60 degrees from the central ray: L = 0.2 + 0.5 cos 60 = 0.45, white gives 0.45 * 255 = 114.75 -> 115; seen from
    behind (the face's winding reversed) the light is the same: |n . l|"""
    cam = capi.default_depth_camera(lib, width=64, height=48, focus=40.0)
    t = np.tan(np.radians(60.0))                                   # plane z = -5 - t x: normal (sin 60, 0, cos 60)
    vtx = np.array([[-1.0, -2.0, -5.0 + t], [1.0, -2.0, -5.0 - t], [0.0, 3.0, -5.0]], np.float32)
    for faces in ([[0, 1, 2]], [[0, 2, 1]]):
        faces = np.array(faces, np.int32)
        sh = capi.default_shade(lib, background=(7, 8, 9))
        rgb, depth, face, _ = sck.shade(cam, vtx, faces, sh)
        cy, cx = cam.height // 2, cam.width // 2
        assert face[cy, cx] == 0 and abs(depth[cy, cx] - 5.0) < 1e-5
        idx, _, _, _, _, L = sck.pixel_terms(cam, vtx, faces, face)
        centre = L[list(idx).index(cy * cam.width + cx)]
        assert abs(centre - 0.45) < 1e-6
        assert rgb[cy, cx].tolist() == [115, 115, 115]
        assert (rgb[face < 0] == [7, 8, 9]).all() and (face < 0).any()
        unlit, _, _, _ = sck.shade(cam, vtx, faces, capi.default_shade(lib, light=0))
        assert (unlit[face >= 0] == 255).all() and (unlit[face < 0] == 0).all()


def test_pixel_on_a_vertex_gets_its_colour(lib):
    """vertices exactly on pixel rays (coordinates are small binary fractions: every product of the contract is exact): the pixel's weights are 1, 0, 0"""
    cam = capi.default_depth_camera(lib, width=64, height=48, focus=512.0)      # 4 / 512 = 2^-7, and the rays' du / 512 are exact as well
    z = 4.0
    px = np.array([[-20, -10], [24, -6], [3, 18]])                 # pixel offsets (du, dv) of the three vertices from the principal point
    vtx = np.array([[du * z / 512.0, -dv * z / 512.0, -z] for du, dv in px], np.float32)
    col = np.array([[250, 3, 77], [1, 200, 31], [90, 91, 255]], np.uint8)
    faces = np.array([[0, 1, 2]], np.int32)
    rgb, _, face, _ = sck.shade(cam, vtx, faces, capi.default_shade(lib, source=capi.SHADE_VERTEX, light=0), col)
    idx, _, wa, wb, wc, _ = sck.pixel_terms(cam, vtx, faces, face)
    for k, (du, dv) in enumerate(px):
        u, v = cam.width // 2 + du, cam.height // 2 + dv
        assert face[v, u] == 0 and rgb[v, u].tolist() == col[k].tolist()
        j = list(idx).index(v * cam.width + u)
        assert [wa[j], wb[j], wc[j]] == [1.0 if k == i else 0.0 for i in range(3)]
    swapped, _, _, _ = sck.shade(cam, vtx, faces, capi.default_shade(lib, source=capi.SHADE_VERTEX, light=0, bgr=1), col)
    assert swapped[cam.height // 2 + px[0][1], cam.width // 2 + px[0][0]].tolist() == [77, 3, 250]


def test_edge_midpoint_is_perspective_correct(lib):
    """edge a-b from depth 1 to depth 3, its ends on pixels 24 and 40 of the centre row: the screen midpoint (pixel 32, the central ray) meets the edge
    at depth 1.5, a quarter of the way along: the near end weighs 0.75 (affine interpolation in the image would say 0.5)"""
    cam = capi.default_depth_camera(lib, width=64, height=48, focus=16.0)
    vtx = np.array([[-0.5, 0.0, -1.0], [1.5, 0.0, -3.0], [0.5, -2.0, -2.0]], np.float32)
    faces = np.array([[0, 1, 2]], np.int32)
    col = np.array([[200, 40, 0], [0, 120, 0], [9, 9, 255]], np.uint8)
    cy, cx = cam.height // 2, cam.width // 2
    sh = capi.default_shade(lib, source=capi.SHADE_VERTEX, light=0)
    rgb, depth, face, _ = sck.shade(cam, vtx, faces, sh, col)
    assert face[cy, cx - 8] == 0 and face[cy, cx + 8] == 0 and face[cy, cx] == 0          # the ends and the midpoint lie on the (inclusive) edge
    assert depth[cy, cx] == np.float32(1.5)
    idx, _, wa, wb, wc, L = sck.pixel_terms(cam, vtx, faces, face)
    k = list(idx).index(cy * cam.width + cx)
    assert (wa[k], wb[k], wc[k]) == (0.75, 0.25, 0.0)
    assert rgb[cy, cx].tolist() == [150, 60, 0]                                           # affine: (100, 80, 0)
    assert rgb[cy, cx - 8].tolist() == [200, 40, 0] and rgb[cy, cx + 8].tolist() == [0, 120, 0]
    # lit: n = (-4, 0, -4), |n . l| = 1 / sqrt 2, L = 0.2 + 0.35355 = 0.55355: 150 -> 83.03, 60 -> 33.21 (no tie near)
    assert abs(L[k] - (0.2 + 0.5 / np.sqrt(2.0))) < 1e-15
    lit, _, _, _ = sck.shade(cam, vtx, faces, capi.default_shade(lib, source=capi.SHADE_VERTEX), col)
    assert lit[cy, cx].tolist() == [83, 33, 0]
