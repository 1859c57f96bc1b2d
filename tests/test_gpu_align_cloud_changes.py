"""What the Cloud rule changed beside itself: immesh_align runs its loop through the statements both rules now share and gives the bytes the library
gave before (tests/golden/align_loop_parent.npz: recorded from the parent commit's library with golden_case() below), and an index that ran an
alignment gives its device memory back."""
import os

import numpy as np
import pytest

import align_checker as ac
import align_cloud_checker as acc
from immesh_amd import capi
from conftest import make_hip
from test_gpu_render import _small_cfg

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "align_loop_parent.npz")


def golden_case(h):
    """immesh_align on a fixed small case: the bumpy sheet of align_checker, 600 points, both modes, from the identity and from a frame, every stop
    of the loop (CONVERGED, MAX_ITERS, TOO_FEW, DEGENERATE), a short history -> {name: uint8 array of the result's and the history's bytes}"""
    vtx, faces, cloud = ac.convergence_case(600, 11)
    centre = capi.align_centre_mean(cloud)
    h.raycast_build_triangles(vtx, faces)
    out = {}

    def run(name, pts, opts, frame=None, history_cap=None):
        res, hist = h.align(pts, opts, frame, history_cap=history_cap)
        out[name] = np.frombuffer(bytes(res) + np.ascontiguousarray(hist).tobytes(), np.uint8).copy()
        return res

    for mode, tag in ((capi.ALIGN_POINT, "point"), (capi.ALIGN_PLANE, "plane")):
        res = run(tag + "_long", cloud, capi.align_options(mode=mode, max_dist=0.5, centre=centre, max_iters=40))
        assert res.iterations > 2 and (mode == capi.ALIGN_POINT or res.status == capi.ALIGN_CONVERGED)
        assert run(tag + "_max_iters", cloud, capi.align_options(mode=mode, max_dist=0.5, max_iters=2), capi.ray_frame(pos=[0.01, 0.0, 0.0]), 1).status == capi.ALIGN_MAX_ITERS
        assert run(tag + "_too_few", cloud[:2], capi.align_options(mode=mode, max_dist=0.5)).status == capi.ALIGN_TOO_FEW
    flat = np.zeros((3, 3), np.float32); flat[1, 0] = 8.0; flat[2, 1] = 8.0                   # one face in z = 0: a plane constrains three of six
    h.raycast_build_triangles(flat, np.array([[0, 1, 2]], np.int32))
    xy = np.random.default_rng(4).uniform(1.0, 3.0, (30, 2))
    pts = np.concatenate([xy, np.full((30, 1), 0.05)], axis=1).astype(np.float32)
    assert run("plane_degenerate", pts, capi.align_options(mode=capi.ALIGN_PLANE, max_dist=1.0)).status == capi.ALIGN_DEGENERATE
    return out


def test_align_gives_the_parents_bytes_through_the_shared_loop():
    h = make_hip(capi.load_hip_library(), _small_cfg())
    try:
        got = golden_case(h)
    finally:
        h.close()
    want = np.load(GOLDEN)
    assert sorted(want.files) == sorted(got)
    for name in want.files:
        assert got[name].tobytes() == want[name].tobytes(), name


def _free_bytes():
    import torch
    return torch.cuda.mem_get_info(0)[0]


def test_fifty_indices_that_ran_an_alignment_give_their_memory_back():
    """50 x (create an index, build, normals, a step of both shapes with per-point outputs, a loop in both modes, destroy) on one context: free device
    memory after the last cycle equals free device memory after the first"""
    cloud, src, centre = acc.convergence_case()
    h = make_hip(capi.load_hip_library(), _small_cfg())
    destroy = h.lib.immesh_cloud_index_destroy; destroy.argtypes = [capi.C.c_void_p]; destroy.restype = None
    try:
        free = []
        for cycle in range(50):
            assert h.cloud_index_build(cloud) == (1600, 1600)
            h.cloud_normals(8, 0.5, want=())
            for variant in (0, 1):
                h.align_cloud_set_variant(variant)
                sy, index, terms = h.align_cloud_step(src, capi.align_options(mode=capi.ALIGN_PLANE, max_dist=acc.SHEET_MAX_DIST), 0.01, None, True, True)
                assert sy.n_used == len(src)
            for mode in (capi.ALIGN_POINT, capi.ALIGN_PLANE):
                assert h.align_cloud(src, capi.align_options(mode=mode, max_dist=acc.SHEET_MAX_DIST), centre=centre)[0].status == capi.ALIGN_CONVERGED
            destroy(h._cloud_index)
            h._cloud_index = None
            free.append(_free_bytes())
        print("free device memory after cycle 1, 2, 25, 50:", free[0], free[1], free[24], free[49])
        assert free[49] == free[0], (free[0], free[49], free[0] - free[49])
    finally:
        h.close()
