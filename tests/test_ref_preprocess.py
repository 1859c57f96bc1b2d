"""The oracle's sensor decoders pinned to the REFERENCE'S OWN code: oracle/_ref/libref_preprocess.so is Preprocess::avia_handler and
Preprocess::velodyne_handler (src/preprocess.cpp:139-232, 497-528) compiled from where they lie behind ROS / PCL shaped stubs (oracle/Makefile,
oracle/ref_preprocess/ref_preprocess_wrap.cpp: excerpts cut by line range at build time, nothing copied).  SURVEY 8(f) rank 4 was "restated from the
source" until round 6; the HIP decoders are compared with this oracle on the GPU (tests/test_decode.py::test_hip_decode_matches_oracle)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import make_oracle, ROOT
from test_decode import _cfg, _livox_msg, _velo_msg, _livox_edge_cases, _velo_gate_xyzi, _velo_pack, _bits, VELO_LAYOUTS, VELO_N_SCANS

VP = C.c_void_p


@pytest.fixture(scope="module")
def ref_pp():
    so = os.path.join(ROOT, "oracle", "_ref", "libref_preprocess.so")
    if os.path.exists("/root/reference/src/preprocess.cpp"):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "ref"], stdout=subprocess.DEVNULL)
    elif not os.path.exists(so):
        pytest.skip("oracle/_ref/libref_preprocess.so not built and /root/reference absent")
    lib = C.CDLL(so)
    lib.rp_avia.argtypes = [VP, C.c_int, C.c_int, C.c_int, C.c_double, VP, C.c_int]
    lib.rp_velodyne.argtypes = [VP, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, VP, C.c_int]
    return lib


def test_avia_handler_of_the_reference_equals_the_oracle(oracle_lib, ref_pp):
    o = make_oracle(oracle_lib, _cfg())
    for seed, n in ((5, 120000), (9, 24000), (11, 7)):
        m = _livox_msg(n, seed=seed)
        w = np.ascontiguousarray(m.view(np.uint8).reshape(-1, 19))
        for n_scans, filt, blind in ((6, 1, 1.0), (6, 3, 4.0), (4, 7, 0.5), (6, 2, 0.0)):
            oo, no = o.decode_livox(w, n_scans, filt, blind)
            out = np.zeros((n, 5), np.float32)
            nr = ref_pp.rp_avia(w.ctypes.data_as(VP), n, n_scans, filt, blind, out.ctypes.data_as(VP), n)
            assert nr == no, (seed, n_scans, filt, blind)
            np.testing.assert_array_equal(out[:nr], oo[:no])     # which points, in which order, x y z reflectivity offset_time / 1e6: bit for bit
    assert no >= 0


def test_velodyne_handler_of_the_reference_equals_the_oracle(oracle_lib, ref_pp):
    o = make_oracle(oracle_lib, _cfg())
    for seed, n in ((6, 130000), (3, 2048)):
        v, _ = _velo_msg(n, seed=seed)
        d = np.ascontiguousarray(v.view(np.uint8).reshape(-1, 32))
        for n_scans in (64, 32):
            oo, no = o.decode_velodyne(d, 32, (0, 4, 8, 16), n_scans)
            out = np.zeros((n, 5), np.float32)
            nr = ref_pp.rp_velodyne(d.ctypes.data_as(VP), n, 32, 0, 4, 8, 16, n_scans, out.ctypes.data_as(VP), n)
            assert nr == no and 0 < no < n
            np.testing.assert_array_equal(out[:nr, :4], oo[:no, :4])   # (the handler leaves curvature unset: PointType's 0)


def test_avia_handler_of_the_reference_equals_the_oracle_at_the_gates(oracle_lib, ref_pp):
    """blind^2 and one float either side, reflectivity 4 / 5, line n_scans - 1 / n_scans / 255, NaN coordinates, stamps above 2^24, a filter
    above the number of valid points, n = 1, no valid line."""
    o = make_oracle(oracle_lib, _cfg())
    for m, n_scans, filt, blind in _livox_edge_cases():
        w = np.ascontiguousarray(m.view(np.uint8).reshape(-1, 19))
        oo, no = o.decode_livox(w, n_scans, filt, blind)
        out = np.zeros((len(m), 5), np.float32)
        nr = ref_pp.rp_avia(w.ctypes.data_as(VP), len(m), n_scans, filt, blind, out.ctypes.data_as(VP), len(m))
        assert nr == no, (len(m), filt, blind)
        np.testing.assert_array_equal(_bits(out[:nr]), _bits(oo[:no]))


def test_velodyne_handler_of_the_reference_equals_the_oracle_at_the_gates(oracle_lib, ref_pp):
    """Every float within 4096 spacings of each elevation gate, the origin, +-90 deg, NaN / inf in each coordinate, subnormals: the same points
    kept bit for bit (the reference drops the NaN elevations through int(NaN) == INT_MIN, the oracle by an explicit test), for every layout."""
    o = make_oracle(oracle_lib, _cfg())
    xyzi = _velo_gate_xyzi()
    n = len(xyzi)
    for step, offs in VELO_LAYOUTS:
        d = np.ascontiguousarray(_velo_pack(xyzi, step, offs))
        for n_scans in VELO_N_SCANS:
            oo, no = o.decode_velodyne(d, step, offs, n_scans)
            out = np.zeros((n, 5), np.float32)
            nr = ref_pp.rp_velodyne(d.ctypes.data_as(VP), n, step, *offs, n_scans, out.ctypes.data_as(VP), n)
            assert nr == no and 0 < no < n, (step, n_scans)
            np.testing.assert_array_equal(_bits(out[:nr, :4]), _bits(oo[:no, :4]))
