"""What the host scaffold shared by the renderer, the colourer and the caster must not move: the refusal texts of the soup check,
the finite-pose check and the points fetch, letter for letter; the thinning tail at the sizes where its table changes, on both of its owners, against
the two checkers; and the device memory a renderer and a colourer give back when they are destroyed.  Every case states the behaviour of the library
before the scaffold was shared: the file passes unchanged on that library too."""
import ctypes as C

import numpy as np
import pytest

import raycast_checker as rcc
import render_checker as rck
import topology_checker as tc
from immesh_amd import capi
from conftest import make_hip
from test_gpu_render import _small_cfg
from test_raycast_cpu import pinhole_rays

pytestmark = pytest.mark.gpu
VTX, FACES = tc.grid_sheet(6, 5)                                                        # 42 vertices, 60 faces at z = 0
W, H, FOCUS, RES = 64, 48, 32.0, 0.3                                                    # (a power of two: the pixel rays are exact floats)
POS = np.array([3.0, 2.5, 4.0])                                                         # above the sheet's centre, looking down with a tilt


def _rot():
    a, b = 0.2, 0.3
    rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    rz = np.array([[np.cos(b), -np.sin(b), 0], [np.sin(b), np.cos(b), 0], [0, 0, 1]])
    return rx @ rz


ROT = _rot()


def _camera(h, w=W, hh=H, res=RES, **over):
    return h.default_depth_camera(width=w, height=hh, focus=FOCUS, downsample_res=res, rot=over.pop("rot", ROT), pos=over.pop("pos", POS), **over)


@pytest.fixture(scope="module")
def hp():
    h = make_hip(capi.load_hip_library(), _small_cfg())
    yield h
    h.close()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- fresh owners on the fixture's context: the wrapper's calls run on them while they stand in for the context's own -------------------------------------
class _Own:
    def __init__(self, h, kind):
        self.h, self.kind, self.attr = h, kind, "_" + kind
        f = getattr(h.lib, f"immesh_{kind}_create"); f.argtypes = [C.c_void_p]; f.restype = C.c_void_p
        self.p = f(h.ctx)
        assert self.p, kind

    def __enter__(self):
        self.saved = getattr(self.h, self.attr, None)
        setattr(self.h, self.attr, C.c_void_p(self.p))
        return self.h

    def __exit__(self, *exc):
        g = getattr(self.h.lib, f"immesh_{self.kind}_destroy"); g.argtypes = [C.c_void_p]; g.restype = None
        g(C.c_void_p(self.p))
        setattr(self.h, self.attr, self.saved)


# ---- refusal texts ------------------------------------------------------------------------------------------------------------------------------------
def _refused(h, rc, text, call, *args):
    """call(*args) is refused with code rc and exactly `text` behind it"""
    with pytest.raises(RuntimeError) as e:
        call(*args)
    head, sep, got = str(e.value).partition(f"rc={rc}: ")
    assert sep and got == text, (str(e.value), text)


def _soup_call(h, who, vtx, n_vtx, faces, n_faces):
    """the three entry points that take a host soup, with the counts and the pointers as given (None: NULL)"""
    pv, pf = capi._ptr(vtx), capi._ptr(faces)
    if who == "raycast_build_triangles":
        f = h.lib.immesh_raycast_build_triangles; f.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64]; f.restype = C.c_int
        rc = f(h.raycaster(), pv, n_vtx, pf, n_faces)
    elif who == "render_triangles":
        f = h.lib.immesh_render_triangles
        f.argtypes = [C.c_void_p, C.POINTER(capi.Camera), C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]; f.restype = C.c_int
        rc = f(h.renderer(), C.byref(_camera(h)), pv, n_vtx, pf, n_faces, None, None)
    else:
        f = h.lib.immesh_shade_triangles
        f.argtypes = [C.c_void_p, C.POINTER(capi.Camera), C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.POINTER(capi.Shade), C.c_void_p,
                      C.c_void_p, C.c_void_p]
        f.restype = C.c_int
        rc = f(h.renderer(), C.byref(_camera(h)), pv, n_vtx, pf, n_faces, None, C.byref(h.default_shade()), None, None, None)
    h._check(rc, who)


def _points_call(h, who, out, cap):
    """immesh_render_points / immesh_raycast_points (res = 0) with the room as given -> *n_out"""
    n = C.c_int64(-7)
    if who == "render_points":
        f = h.lib.immesh_render_points; f.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]; f.restype = C.c_int
        rc = f(h.renderer(), capi._ptr(out), cap, C.byref(n))
    else:
        f = h.lib.immesh_raycast_points; f.argtypes = [C.c_void_p, C.c_double, C.c_void_p, C.c_int64, C.c_void_p]; f.restype = C.c_int
        rc = f(h.raycaster(), 0.0, capi._ptr(out), cap, C.byref(n))
    h._check(rc, who)
    return n.value


SOUP_CALLS = ("render_triangles", "shade_triangles", "raycast_build_triangles")


def _with(faces, face, corner, value):
    bad = faces.copy()
    bad[face, corner] = value
    return bad


def _soup_rows(h):
    for who in SOUP_CALLS:
        arrays = f"{who}: bad vertex / face arrays"
        _refused(h, -1, arrays, _soup_call, h, who, VTX, -1, FACES, len(FACES))                     # a negative count
        _refused(h, -1, arrays, _soup_call, h, who, VTX, len(VTX), FACES, -1)
        _refused(h, -1, arrays, _soup_call, h, who, None, len(VTX), FACES, len(FACES))              # a NULL array with a positive count
        _refused(h, -1, arrays, _soup_call, h, who, VTX, len(VTX), None, len(FACES))
        _refused(h, -1, f"{who}: face 7 has vertex index -1 out of range [0, 42)", _soup_call, h, who, VTX, len(VTX), _with(FACES, 7, 1, -1), len(FACES))
        _refused(h, -1, f"{who}: face 59 has vertex index 42 out of range [0, 42)", _soup_call, h, who, VTX, len(VTX), _with(FACES, 59, 2, 42), len(FACES))


def _pose_rows(h):
    nan_rot, inf_pos = ROT.copy(), POS.copy()
    nan_rot[1, 2] = np.nan
    inf_pos[2] = np.inf
    px = np.zeros((16, 16, 3), np.uint8)
    dirs = pinhole_rays(_camera(h))[:5]
    for rot, pos, what in ((nan_rot, POS, "rotation"), (ROT, inf_pos, "position")):
        _refused(h, -1, f"render: camera {what} is not finite", h.render_triangles, _camera(h, rot=rot, pos=pos), VTX, FACES)
        _refused(h, -1, f"raycast: frame {what} is not finite", h.raycast, capi.ray_frame(rot, pos), dirs)
        _refused(h, -1, f"colour: camera {what} is not finite", h.colour_image, h.default_image(px, rot=rot, pos=pos))


def _cap_rows(h):
    n_r, n_c = len(h.render_points()), len(h.raycast_points(0.0))
    assert n_r > 1 and n_c > 1
    for who, n in (("render_points", n_r), ("raycast_points", n_c)):
        out = np.zeros((n, 3), np.float32)
        _refused(h, capi.E_CAPACITY, f"{who}: cap {n - 1} < {n} points", _points_call, h, who, out, n - 1)
        assert _points_call(h, who, None, n - 1) == n                                               # no output array: the count alone


REFUSED = {"soup": _soup_rows, "pose": _pose_rows, "cap": _cap_rows}


def _state(h):
    """what a refused call must leave: the last render's points, the caster's sizes, the last cast's points"""
    return h.render_points().tobytes(), h._raycast_sizes(), h.raycast_points(0.0).tobytes()


@pytest.mark.parametrize("rows", list(REFUSED))
def test_refusal_texts_are_exact_and_leave_the_objects_as_they_were(hp, rows):
    cam = _camera(hp)
    hp.render_triangles(cam, VTX, FACES)
    assert hp.raycast_build_triangles(VTX, FACES) == (42, 60, 60)
    hp.raycast(capi.ray_frame(ROT, POS), pinhole_rays(cam))
    before = _state(hp)
    assert len(before[0]) > 12 and len(before[2]) > 12
    REFUSED[rows](hp)
    assert _state(hp) == before


def test_no_points_need_no_room(hp):
    """cap = 0 with an output array is fine when there is nothing to copy"""
    away = _camera(hp, rot=ROT @ np.diag([1.0, -1.0, -1.0]))                                        # looking up: no pixel sees the sheet
    depth, _ = hp.render_triangles(away, VTX, FACES)
    assert (depth < 0).all()
    hp.raycast_build_triangles(VTX, FACES)
    hp.raycast(capi.ray_frame(ROT, POS), np.zeros((0, 3), np.float32))
    out = np.zeros((1, 3), np.float32)
    for who in ("render_points", "raycast_points"):
        assert _points_call(hp, who, out, 0) == 0
        assert _points_call(hp, who, None, 0) == 0


# ---- the thinning tail ----------------------------------------------------------------------------------------------------------------------------------
# n rays -> the camera with n pixels (the renderer has no image of 0 pixels); 511 / 512 / 513: the table's floor of 1024 slots, 3072: 8192 slots
CAMERAS = {1: (1, 1), 511: (73, 7), 512: (32, 16), 513: (27, 19), 3072: (W, H)}
_refs = {}


def _rays():
    """the pixel rays of the 64 x 48 camera, from the image's centre on: the first of them hits the sheet"""
    if "rays" not in _refs:
        cam = capi.Camera()
        cam.width, cam.height, cam.focus = W, H, FOCUS
        dirs = np.roll(pinhole_rays(cam), -((H // 2) * W + W // 2), axis=0)
        t, f = rcc.cast(ROT, POS, dirs, None, 0.05, 200.0, VTX, FACES)
        assert 0 < (f >= 0).sum() < len(f) and f[0] >= 0
        _refs["rays"] = (dirs, t)
    return _refs["rays"]


def _cast_ref(n, res):
    if ("cast", n, res) not in _refs:
        dirs, t = _rays()
        _refs["cast", n, res] = rcc.points(ROT, POS, dirs[:n], None, t[:n], res)
    return _refs["cast", n, res]


def _render_ref(h, n, res):
    if ("render", n, res) not in _refs:
        cam = _camera(h, *CAMERAS[n], res=res)
        _refs["render", n, res] = rck.reinforce(cam, rck.render(cam, VTX, FACES)[0])
    return _refs["render", n, res]


def _same(got, ref, what):
    print(what, "points", len(got), "checker", len(ref))
    assert got.shape == ref.shape and np.array_equal(_bits(got), _bits(ref)), what


@pytest.mark.parametrize("n", [0, 1, 511, 512, 513, 3072])
def test_thinning_tail_on_the_caster(hp, n):
    """res > 0 on a fresh caster, res = 0, res > 0 again; then on another caster res = 0 first, so that cells, slot and table are grown late"""
    dirs, t = _rays()
    for order in ((RES, 0.0, RES), (0.0, RES)):
        with _Own(hp, "raycaster") as h:
            assert h.raycast_build_triangles(VTX, FACES) == (42, 60, 60)
            got_t, _ = h.raycast(capi.ray_frame(ROT, POS), dirs[:n], None, 0.05, 200.0)
            assert np.array_equal(_bits(got_t), _bits(t[:n]))
            for res in order:
                _same(h.raycast_points(res), _cast_ref(n, res), ("caster", n, order, res))
    assert len(_cast_ref(n, RES)) <= len(_cast_ref(n, 0.0)) == int((t[:n] >= 0).sum())
    if n >= 511:
        assert 0 < len(_cast_ref(n, RES)) < len(_cast_ref(n, 0.0))                                 # the cells are shared: the thinning decides


@pytest.mark.parametrize("n", [1, 511, 512, 513, 3072])
def test_thinning_tail_on_the_renderer(hp, n):
    for order in ((RES, 0.0, RES), (0.0, RES)):
        with _Own(hp, "renderer") as h:
            for res in order:
                h.render_triangles(_camera(h, *CAMERAS[n], res=res), VTX, FACES, want_depth=False, want_face=False)
                _same(h.render_points(), _render_ref(h, n, res), ("renderer", n, order, res))
    if n >= 511:
        assert 0 < len(_render_ref(hp, n, RES)) < len(_render_ref(hp, n, 0.0))


# ---- lifetime -------------------------------------------------------------------------------------------------------------------------------------------
def _free_bytes():
    import torch
    return torch.cuda.mem_get_info(0)[0]


def test_fifty_renderers_and_colourers_give_their_memory_back(hp):
    """50 x (create, one 64 x 48 shade call with res > 0 or one 16 x 16 image, destroy) on one context: free device memory after the last cycle equals
    free device memory after the first"""
    px = np.full((16, 16, 3), 90, np.uint8)
    cam = _camera(hp)
    free = []
    for cycle in range(50):
        with _Own(hp, "renderer") as h:
            rgb, _, _ = h.shade_triangles(cam, VTX, FACES, h.default_shade(source=capi.SHADE_AXIS))
            assert rgb.any() and len(h.render_points()) > 0
        with _Own(hp, "colourer") as h:
            h.colour_image(h.default_image(px, fx=16.0, fy=16.0, cx=8.0, cy=8.0))
        free.append(_free_bytes())
    print("free device memory after cycle 1, 2, 25, 50:", free[0], free[1], free[24], free[49])
    assert free[49] == free[0], (free[0], free[49], free[0] - free[49])
