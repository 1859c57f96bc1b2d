"""CPU tier of the vertex colourer (include/immesh_colour.h): the numpy checker against records of the reference's own update_rgb
(tests/golden/colour_update_r07.npz, written by tools/make_golden_colour.py), closed forms of the 8-bit bilinear tap, the selection loop against its
order-free form, and the boundary -- exported symbols, struct layouts against the header, the default image.  No device is touched."""
import ctypes as C
import os
import re

import numpy as np

import colour_checker as cck
from immesh_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "immesh_colour.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "colour_update_r07.npz")


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def test_update_rgb_matches_the_reference_records():
    g = np.load(GOLDEN)
    n_obs, n_pts = g["ret"].shape
    assert n_obs * n_pts >= 20000
    st = cck.fresh_state(n_pts)
    idx = np.arange(n_pts)
    for j in range(n_obs):
        ret, _ = cck.update_rgb(st, idx, g["c"][j].astype(np.float64), g["obs_dis"][j], g["sigma"][j], g["t"][j], g["e"][j])
        assert np.array_equal(ret, g["ret"][j]), j
        assert np.array_equal(st["n_obs"], g["n_obs"][j]), j
        assert np.array_equal(_bits(st["rgb"]), _bits(g["rgb"][j])), j
        for k in range(3):
            assert np.array_equal(_bits(st["cov"][:, k]), _bits(g["cov"][j])), (j, k)
        assert np.array_equal(_bits(st["first_exposure"]), _bits(g["first_exposure"][j])), j
        assert np.array_equal(_bits(st["obs_dis"]), _bits(g["state_obs_dis"][j])), j
        assert np.array_equal(_bits(st["last_obs_time"]), _bits(g["last_obs_time"][j])), j
    # the records take every branch
    assert (g["ret"] == 1).any() and (g["ret"] == 0).any() and (g["c"] == 0).all(axis=2).any() and len(np.unique(g["e"])) > 2


def test_sampling_closed_forms():
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (12, 16, 3)).astype(np.uint8)
    # integer (u, v) returns the pixel -- also in the last column / row, where the zero-weight taps lie one past the image
    u, v = np.meshgrid(np.arange(16.0), np.arange(12.0))
    got = cck.sample(img, u.ravel(), v.ravel())
    assert np.array_equal(got, img.reshape(-1, 3).astype(np.float64))
    # a = b = 0.5 on four pixels of 255: 4 x R8(63.75) = 4 x 64 saturates at 255
    white = np.full((4, 4, 3), 255, np.uint8)
    assert np.array_equal(cck.sample(white, [1.5], [1.5]), [[255.0, 255.0, 255.0]])
    # half to even: 0.25 * 2 = 0.5 -> 0 and 0.25 * 6 = 1.5 -> 2, per tap
    assert np.array_equal(cck.sample(np.full((4, 4, 3), 2, np.uint8), [1.5], [1.5]), [[0.0, 0.0, 0.0]])
    assert np.array_equal(cck.sample(np.full((4, 4, 3), 6, np.uint8), [1.5], [1.5]), [[8.0, 8.0, 8.0]])
    # each product is rounded on its own: weights 0.75 / 0.25 along u on (10, 30) -> R8(7.5) + R8(7.5) = 8 + 8, not R8(15)
    two = np.zeros((3, 4, 3), np.uint8); two[:, 1] = 10; two[:, 2] = 30
    assert np.array_equal(cck.sample(two, [1.25], [1.0]), [[16.0, 16.0, 16.0]])
    assert cck.std_round(np.array([0.5, 1.5, 2.5, -0.5, 0.49999999999999994])).tolist() == [1.0, 2.0, 3.0, -1.0, 0.0]


def test_selection_loop_equals_order_free_form():
    """depths a few float or double spacings apart and repeated values, so (double)stored > depth decides"""
    rng = np.random.default_rng(5)
    for trial in range(300):
        n = int(rng.integers(1, 40))
        base = np.float64(np.float32(rng.uniform(3.0, 50.0)))
        ulp32 = np.spacing(np.float32(base)).astype(np.float64)
        steps = rng.integers(-3, 4, n) * ulp32 * rng.choice([0.0, 0.25, 0.5, 1.0], n) + rng.integers(-3, 4, n) * np.spacing(base)
        depth = base + steps
        depth[rng.random(n) < 0.3] = base
        cu, cv = rng.integers(0, 3, n), rng.integers(0, 2, n)
        assert np.array_equal(cck.select_loop(cu, cv, depth), cck.select_order_free(cu, cv, depth)), trial


def test_symbols_exported():
    lib = capi.load_hip_library()
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    fns = sorted(set(re.findall(r"\b(immesh_[a-z_0-9]+)\s*\(", src)))
    assert set(fns) >= {"immesh_default_image", "immesh_colourer_create", "immesh_colourer_destroy", "immesh_colour_image", "immesh_colour_selected",
                        "immesh_colour_fetch", "immesh_save_ply_rgb", "immesh_colourer_last_timing"}
    missing = [f for f in fns if not hasattr(lib, f)]
    assert not missing, missing
    assert '#include "immesh_colour.h"' in open(os.path.join(ROOT, "include", "immesh_c_api.h")).read()


def _header_fields(name):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = src[src.index("typedef struct %s {" % name):src.index("} %s;" % name)]
    out = []
    for typ, names in re.findall(r"\b(const uint8_t\*|double|int32_t|int64_t)\s+([^;]+);", body):
        for nm in names.split(","):
            m = re.match(r"\s*([A-Za-z_0-9]+)(?:\[(\d+)\])?\s*$", nm)
            out.append((m.group(1), typ, int(m.group(2) or 1)))
    return out


def test_struct_layouts_match_header():
    size = {"const uint8_t*": 8, "double": 8, "int32_t": 4, "int64_t": 8}
    img = _header_fields("immesh_image")
    assert [n for n, _, _ in img] == [n for n, _ in capi.Image._fields_]
    assert C.sizeof(capi.Image) == sum(size[t] * k for _, t, k in img) == 200
    st = _header_fields("immesh_colour_stats")
    assert [n for n, _, _ in st] == [n for n, _ in capi.ColourStats._fields_]
    assert C.sizeof(capi.ColourStats) == sum(size[t] * k for _, t, k in st) == 64
    cs = _header_fields("immesh_colour_state")
    assert [n for n, _, _ in cs] == list(capi.COLOUR_STATE_DTYPE.names) == list(cck.STATE_DTYPE.names)
    assert capi.COLOUR_STATE_DTYPE.itemsize == sum(size[t] * k for _, t, k in cs) == 80
    assert capi.COLOUR_STATE_DTYPE == cck.STATE_DTYPE


def test_default_image():
    im = capi.default_image(capi.load_hip_library())
    assert (im.fov_margin, im.inv_exposure, im.min_depth, im.max_depth, im.max_pe_error) == (0.005, 0.01, 3.0, 200.0, 40.0)
    assert list(im.rot) == [1, 0, 0, 0, 1, 0, 0, 0, 1] and list(im.pos) == [0, 0, 0]
    assert (im.rows, im.cols, im.row_stride_bytes, im.fx, im.fy, im.cx, im.cy, im.obs_time) == (0, 0, 0, 0, 0, 0, 0, 0) and not im.data
    px = np.zeros((48, 64, 3), np.uint8)
    im = capi.default_image(capi.load_hip_library(), px, fx=50.0, pos=[1, 2, 3])
    assert (im.rows, im.cols, im.row_stride_bytes, im.fx) == (48, 64, 192, 50.0) and list(im.pos) == [1, 2, 3] and im.data == px.ctypes.data
