"""Sensor decode: Preprocess::avia_handler (feature extraction off) and Preprocess::velodyne_handler
(src/preprocess.cpp:139-232, 497-526) on the wire formats (livox_ros_driver/CustomMsg points, sensor_msgs/PointCloud2 data)."""
import numpy as np
import pytest

from immesh_amd import capi
from conftest import make_oracle, make_hip, fetch_device

LIVOX = np.dtype([("offset_time", "<u4"), ("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("reflectivity", "u1"), ("tag", "u1"), ("line", "u1")])   # 19 bytes, packed
VELO = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("pad", "<f4"), ("intensity", "<f4"), ("time", "<f4"), ("ring", "<u2"), ("pad2", "V6")])  # 32 bytes (PCL layout)


def _cfg():
    return capi.avia_config(cap_root_voxels=1 << 10, cap_scan_points=200000, cap_vertices=1 << 12, cap_triangles=1 << 14)


def _livox_msg(n, seed=0):
    rng = np.random.default_rng(seed)
    m = np.zeros(n, LIVOX)
    assert LIVOX.itemsize == 19
    m["offset_time"] = np.sort(rng.integers(0, 100_000_000, n)).astype(np.uint32)
    d = rng.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1)[:, None]
    r = rng.uniform(0.2, 60.0, n)
    m["x"], m["y"], m["z"] = (d * r[:, None]).astype(np.float32).T
    m["reflectivity"] = rng.integers(0, 256, n)
    m["tag"] = rng.integers(0, 256, n)
    m["line"] = rng.integers(0, 8, n)          # lines 6 and 7 are not below N_SCANS = 6
    return m


def _livox_expected(m, n_scans, filt, blind):
    out, valid = [], 0
    for i in range(1, len(m)):
        if m["line"][i] < n_scans:
            valid += 1
            if valid % filt == 0:
                x, y, z = np.float32(m["x"][i]), np.float32(m["y"][i]), np.float32(m["z"][i])
                if m["reflectivity"][i] > 4 and float(np.float32(np.float32(x * x + y * y) + z * z)) > blind * blind:
                    out.append([x, y, z, np.float32(m["reflectivity"][i]), np.float32(m["offset_time"][i]) / np.float32(1000000)])
    return np.array(out, np.float32).reshape(-1, 5)


def test_oracle_avia_handler_known_answers(oracle_lib):
    o = make_oracle(oracle_lib, _cfg())
    m = _livox_msg(5000)
    for filt, blind in ((1, 1.0), (3, 4.0)):
        out, n = o.decode_livox(m.view(np.uint8).reshape(-1, 19), 6, filt, blind)
        exp = _livox_expected(m, 6, filt, blind)
        assert n == len(exp) and 500 < n < 5000
        np.testing.assert_array_equal(out, exp)
    assert m["line"][0] < 6 and not np.any(np.all(out[:, :3] == [m["x"][0], m["y"][0], m["z"][0]], axis=1))   # the loop starts at point 1




def _livox_edge_cases(n_scans=6):
    """(message, n_scans, point_filter_num, blind) at the boundaries of every avia_handler gate: x^2+y^2+z^2 on blind^2 and one float either
    side, reflectivity 4 / 5, line n_scans - 1 / n_scans / 255, NaN and inf coordinates, offset times where u32 -> float rounds, a filter
    larger than the number of valid points, n = 1, no valid line at all."""
    rng = np.random.default_rng(21)
    rows = [(0, 9.0, 9.0, 9.0, 100, 0)]                                    # point 0: the loop starts at point 1
    for b in (0.5, 0.3, 1.0):
        f = np.float32(b)
        for v in (np.nextafter(f, np.float32(0)), f, np.nextafter(f, np.float32(np.inf))):
            rows += [(0, v, 0.0, 0.0, 100, 0), (0, 0.0, -v, 0.0, 100, 1), (0, 0.0, 0.0, v, 100, 2)]
        c = np.float32(b / np.sqrt(3.0))
        for k in range(-3, 4):                                             # the float sum of three squares lands on, below and above blind^2
            v = np.array([c], np.float32).view(np.int32) + k
            v = v.view(np.float32)[0]
            rows.append((0, v, -v, v, 100, 3))
    for refl in (0, 3, 4, 5, 6, 255):
        rows.append((0, 5.0, 0.0, 0.0, refl, 0))
    for line in (n_scans - 1, n_scans, n_scans + 1, 255):
        rows.append((0, 0.0, 5.0, 0.0, 100, line))
    nan, inf = np.nan, np.inf
    for xyz in ((nan, 0, 0), (0, nan, 0), (0, 0, nan), (nan, nan, nan), (inf, 0, 0), (0, -inf, 0), (inf, -inf, 0), (-0.0, -0.0, -0.0), (1e-40, 0, 0)):
        rows.append((0, *xyz, 100, 1))
    for _ in range(300):
        d = rng.normal(size=3)
        rows.append((0, *(d / np.linalg.norm(d) * rng.uniform(0.1, 5.0)), int(rng.integers(0, 256)), int(rng.integers(0, 9))))
    m = np.zeros(len(rows), LIVOX)
    for i, r in enumerate(rows):
        m[i] = (0, np.float32(r[1]), np.float32(r[2]), np.float32(r[3]), r[4], i % 251, r[5])
    times = np.array([0, 1, 999_999, 1_000_000, 2**24 - 1, 2**24, 2**24 + 1, 2**24 + 3, 2**25 + 1, 2**25 + 3, 123_456_789, 2**31 - 1, 2**31, 2**31 + 1,
                      2**32 - 129, 2**32 - 128, 2**32 - 1], np.uint64)
    m["offset_time"] = np.concatenate([times, rng.integers(0, 2**32, len(m) - len(times), dtype=np.uint64)]).astype(np.uint32)
    perm = np.concatenate([[0], 1 + rng.permutation(len(m) - 1)])          # gates in a mixed order (point 0 stays the skipped one)
    m = m[perm]
    cases = [(m, n_scans, filt, blind) for blind in (0.5, 0.3, 1.0) for filt in (1, 2)]
    valid = int(np.sum(m["line"][1:] < n_scans))
    cases.append((m, n_scans, valid + 1, 0.5))                             # point_filter_num above the number of valid points: nothing
    cases.append((m[:1], n_scans, 1, 0.5))                                 # n = 1: nothing
    none = m.copy(); none["line"] = np.maximum(none["line"], n_scans)
    cases.append((none, n_scans, 1, 0.5))                                  # no valid line: nothing
    return cases


def test_oracle_avia_handler_gate_boundaries(oracle_lib):
    o = make_oracle(oracle_lib, _cfg())
    sizes = []
    for m, n_scans, filt, blind in _livox_edge_cases():
        out, n = o.decode_livox(m.view(np.uint8).reshape(-1, 19), n_scans, filt, blind)
        with np.errstate(all="ignore"):
            exp = _livox_expected(m, n_scans, filt, blind)
        assert n == len(exp), (filt, blind)
        np.testing.assert_array_equal(out.view(np.uint32), exp.view(np.uint32))
        sizes.append(n)
    assert min(sizes[:6]) > 50 and sizes[6:] == [0, 0, 0]
    m = _livox_edge_cases()[0][0]
    out, _ = o.decode_livox(m.view(np.uint8).reshape(-1, 19), 6, 1, 0.5)
    on_gate = (out[:, 0] == np.float32(0.5)) | (out[:, 1] == -np.float32(0.5)) | (out[:, 2] == np.float32(0.5))
    assert not np.any(on_gate & (np.sum(out[:, :3] != 0, axis=1) == 1))    # |p| == blind exactly is not > blind: dropped
    assert np.any(out[:, 0] == np.nextafter(np.float32(0.5), np.float32(1)))
    assert set(np.unique(out[:, 3]).tolist()) >= {5.0} and out[:, 3].min() >= 5                  # reflectivity 4 dropped, 5 kept
    assert np.all(np.isfinite(out[:, :3]) | np.isinf(out[:, :3]))                                 # NaN points never kept


# ---- velodyne_handler ----------------------------------------------------------------------------------------------------------------
# PointCloud2 layouts: (point_step, byte offsets of x, y, z, intensity)
VELO_LAYOUTS = ((32, (0, 4, 8, 16)), (16, (0, 4, 8, 12)), (48, (16, 20, 24, 0)), (64, (48, 52, 56, 60)))
VELO_N_SCANS = (16, 32, 33, 64, 128)
# The kept set is exactly the floats q = z / sqrtf(x*x + y*y) in [q_lo, q_hi] (as bit patterns), found by enumerating all 2^32 float q through
# the reference's expression with glibc's atanf.  64: the lowest rows are cut at scan_id 51 (-18.08 deg); 32 and 16: at -24.33 deg.
VELO_Q_INTERVAL = {64: (0xbea7264c, 0x3d0f0915), 32: (0xbee77fec, 0x3d0f0915), 16: (0xbee77fec, 0x3d0f0915)}
VELO_GATES_DEG = (2.0, -8.83, -18.08, -24.33)   # angle > 2; the branch at -8.83; scan_id 51 for n_scans 64; angle < -24.33
VELO_WINDOW = 4096                               # floats either side of each gate


def _f32(bits):
    return np.array([bits], np.uint32).view(np.float32)[0]


def _ordered(f):
    b = np.array([f], np.float32).view(np.uint32)[0]
    return -int(b & 0x7fffffff) if b & 0x80000000 else int(b)


def _from_ordered(k):
    return _f32((0x80000000 | -k) if k < 0 else k)


def _velo_q(xyzi):
    """q = z / sqrtf(x*x + y*y) in float32, as the handler computes it (and the device, without -ffp-contract)."""
    x, y, z = (np.ascontiguousarray(xyzi[:, k], np.float32) for k in range(3))
    with np.errstate(all="ignore"):
        return z / np.sqrt(x * x + y * y)


def _velo_expected(xyzi, q_lo, q_hi):
    q = _velo_q(xyzi)
    keep = (q >= q_lo) & (q <= q_hi)                                       # (NaN fails both)
    out = np.zeros((int(keep.sum()), 5), np.float32)
    out[:, :4] = xyzi[keep]
    return out


def _velo_pack(xyzi, step, offsets, seed=0):
    """n x step PointCloud2 bytes, x y z intensity at the given offsets, every other byte random."""
    n = len(xyzi)
    d = np.random.default_rng(seed).integers(0, 256, (n, step), dtype=np.uint8)
    for k, off in enumerate(offsets):
        d[:, off:off + 4] = np.ascontiguousarray(xyzi[:, k], np.float32).view(np.uint8).reshape(n, 4)
    return d


def _velo_msg(n, seed=1):
    rng = np.random.default_rng(seed)
    m = np.zeros(n, VELO)
    assert VELO.itemsize == 32
    az = rng.uniform(-np.pi, np.pi, n)
    el = np.deg2rad(rng.uniform(-30.0, 6.0, n))       # beyond the HDL-64 fan on both sides
    r = rng.uniform(1.0, 80.0, n)
    m["x"], m["y"], m["z"] = (r * np.cos(el) * np.cos(az)).astype(np.float32), (r * np.cos(el) * np.sin(az)).astype(np.float32), (r * np.sin(el)).astype(np.float32)
    m["intensity"] = rng.uniform(0, 255, n).astype(np.float32)
    return m, np.rad2deg(el)


def _velo_xyzi(m):
    return np.stack([m["x"], m["y"], m["z"], m["intensity"]], axis=1).astype(np.float32)


VELO_SPECIAL = [(0, 0, 0), (-0.0, 0, 0), (0, -0.0, -0.0), (0, 0, 1), (0, 0, -1),                     # 0/0 = NaN; z/0 = +-inf (+-90 deg)
                (np.nan, 0, 0), (0, np.nan, 0), (0, 0, np.nan), (1, 0, np.nan), (np.nan, np.nan, np.nan),
                (np.inf, 0, 0), (-np.inf, 0, 0), (0, np.inf, 0), (0, -np.inf, 0), (0, 0, np.inf), (0, 0, -np.inf),
                (1, 0, np.inf), (1, 0, -np.inf), (np.inf, np.inf, np.inf), (np.inf, 0, np.inf), (np.inf, 0, -1),
                (1e-40, 0, 0), (1e-40, 0, 1e-41), (1, 0, 1e-40), (1, 0, -1e-40), (1, 0, -0.0), (1, -0.0, 0), (-0.0, -0.0, 1),
                (1e-40, 1e-40, -3e-41), (1e-20, 1e-20, -4e-21), (-1e-20, 1e-20, -5.3e-21), (3e-23, 0, -1e-23), (1e19, 1e19, -4e18),
                (1e20, 0, 3e18), (-2e-38, 0, 6e-40)]                   # subnormal squares and quotients near the gates


def _velo_gate_xyzi(seed=7, n_ordinary=3000):
    """Every float q from -VELO_WINDOW to +VELO_WINDOW spacings around each gate as (1, 0, q) (so that q is exactly z), the special points
    (origin, +-90 deg, NaN and inf in each coordinate, subnormals, -0.0) and ordinary points of a fan, shuffled together."""
    rng = np.random.default_rng(seed)
    zs = []
    for a in VELO_GATES_DEG:
        b = np.array([np.tan(np.deg2rad(a))], np.float32).view(np.int32)[0]
        zs.append((b + np.arange(-VELO_WINDOW, VELO_WINDOW + 1)).astype(np.int32).view(np.float32))
    z = np.concatenate(zs)
    gate = np.stack([np.ones_like(z), np.zeros_like(z), z, rng.uniform(0, 255, len(z)).astype(np.float32)], axis=1)
    special = np.array([(*p, 7.0) for p in VELO_SPECIAL], np.float32)
    ordinary = _velo_xyzi(_velo_msg(n_ordinary, seed=seed)[0])
    xyzi = np.concatenate([gate, special, ordinary])
    return np.ascontiguousarray(xyzi[rng.permutation(len(xyzi))])


def _oracle_q_interval(o, n_scans):
    """[q_lo, q_hi] found by bisection against the oracle itself, one point (1, 0, q) at a time (q = 0 is kept for every n_scans)."""
    def keep(k):
        xyzi = np.array([[1.0, 0.0, _from_ordered(k), 0.0]], np.float32)
        return o.decode_velodyne(_velo_pack(xyzi, 16, (0, 4, 8, 12)), 16, (0, 4, 8, 12), n_scans)[1] == 1
    dropped, kept = _ordered(-np.inf), 0
    while kept - dropped > 1:
        mid = dropped + (kept - dropped) // 2
        if keep(mid): kept = mid
        else: dropped = mid
    q_lo = _from_ordered(kept)
    kept, dropped = 0, _ordered(np.inf)
    while dropped - kept > 1:
        mid = kept + (dropped - kept) // 2
        if keep(mid): kept = mid
        else: dropped = mid
    return q_lo, _from_ordered(kept)


def _velo_q_interval(o, n_scans):
    if n_scans in VELO_Q_INTERVAL:
        return tuple(_f32(b) for b in VELO_Q_INTERVAL[n_scans])
    return _oracle_q_interval(o, n_scans)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_oracle_velodyne_handler_known_answers(oracle_lib):
    o = make_oracle(oracle_lib, _cfg())
    for n_scans, (lo, hi) in VELO_Q_INTERVAL.items():                      # the oracle's bisection reproduces the enumeration's table
        got = _oracle_q_interval(o, n_scans)
        assert (_bits([got[0]])[0], _bits([got[1]])[0]) == (lo, hi), n_scans
    assert _oracle_q_interval(o, 33) == _velo_q_interval(o, 32)            # N_SCANS / 2 is what counts
    lo128, hi128 = _velo_q_interval(o, 128)                                 # N_SCANS / 2 >= 51: the lower branch is cut entirely, at -8.83 deg
    assert hi128 == _f32(0x3d0f0915) and abs(np.rad2deg(np.arctan(float(lo128))) + 8.83) < 1e-5
    xyzi = _velo_gate_xyzi()
    q = _velo_q(xyzi)
    for n_scans in VELO_N_SCANS:
        lo, hi = _velo_q_interval(o, n_scans)
        windows = [np.float32(np.tan(np.deg2rad(a))) for a in VELO_GATES_DEG]
        spacing = [np.spacing(np.abs(w)) * VELO_WINDOW for w in windows]
        assert any(abs(lo - w) < s for w, s in zip(windows, spacing)) and abs(hi - windows[0]) < spacing[0]   # both ends inside a window
        exp = _velo_expected(xyzi, lo, hi)
        for step, offs in VELO_LAYOUTS:
            out, n = o.decode_velodyne(_velo_pack(xyzi, step, offs), step, offs, n_scans)
            assert n == len(exp), (n_scans, step)                          # exact: every float of every window on the right side of its gate
            np.testing.assert_array_equal(_bits(out), _bits(exp))
        assert not np.any(np.isnan(exp[:, :3])) and np.any(np.isnan(q))                  # NaN and origin points dropped
        on = (xyzi[:, 0] == 1) & (xyzi[:, 1] == 0)
        assert np.sum(on & (xyzi[:, 2] >= lo) & (xyzi[:, 2] <= hi)) > VELO_WINDOW    # (the windows really straddle the ends)
    m, el = _velo_msg(20000)
    out, n = o.decode_velodyne(m.view(np.uint8).reshape(-1, 32), 32, (0, 4, 8, 16), 64)
    np.testing.assert_array_equal(_bits(out), _bits(_velo_expected(_velo_xyzi(m), *_velo_q_interval(o, 64))))
    assert np.all(out[:, 4] == 0.0) and 0.3 * len(m) < n < 0.8 * len(m)
    ang = np.rad2deg(np.arctan(out[:, 2] / np.hypot(out[:, 0], out[:, 1])))
    assert ang.max() <= 2.0 + 1e-3 and ang.min() >= -18.58 - 1e-3


@pytest.mark.gpu
def test_hip_decode_matches_oracle(oracle_lib, hip_lib):
    o, h = make_oracle(oracle_lib, _cfg()), make_hip(hip_lib, _cfg())
    m = _livox_msg(120000, seed=5)
    w = m.view(np.uint8).reshape(-1, 19)
    cases = [(m, 6, filt, blind) for filt, blind in ((1, 1.0), (3, 4.0), (7, 0.5))] + _livox_edge_cases()
    for mm, n_scans, filt, blind in cases:
        w = mm.view(np.uint8).reshape(-1, 19)
        oo, n_o = o.decode_livox(w, n_scans, filt, blind)
        oh, n_h = h.decode_livox(w, n_scans, filt, blind)
        assert n_h == n_o, (len(mm), filt, blind)
        np.testing.assert_array_equal(_bits(oh), _bits(oo))
    v, _ = _velo_msg(130000, seed=6)
    msgs = [(_velo_xyzi(v), VELO_LAYOUTS[0], (64,), v.view(np.uint8).reshape(-1, 32))]
    gate = _velo_gate_xyzi()
    msgs += [(gate, lay, VELO_N_SCANS, _velo_pack(gate, *lay)) for lay in VELO_LAYOUTS]
    for xyzi, (step, offs), scans, d in msgs:
        for n_scans in scans:
            oo, n_o = o.decode_velodyne(d, step, offs, n_scans)
            oh, n_h = h.decode_velodyne(d, step, offs, n_scans)
            assert n_h == n_o, (len(d), step, n_scans)                       # bit-exact: the gates are decided on the host's q interval
            np.testing.assert_array_equal(_bits(oh), _bits(oo))


@pytest.mark.gpu
def test_hip_velodyne_drops_nan_and_origin_points(oracle_lib, hip_lib):
    """No-return points of a real cloud: (0,0,0) and NaN coordinates have a NaN elevation, which the reference drops (int(NaN) is INT_MIN on
    x86-64) and the device used to keep (v_cvt_i32_f64 of NaN is 0)."""
    o, h = make_oracle(oracle_lib, _cfg()), make_hip(hip_lib, _cfg())
    xyzi = np.array([(0, 0, 0, 1), (np.nan, 0, 0, 2), (0, np.nan, 0, 3), (0, 0, np.nan, 4), (np.nan, np.nan, np.nan, 5), (5, 1, -0.5, 6)], np.float32)
    d = _velo_pack(xyzi, 32, (0, 4, 8, 16))
    oo, n_o = o.decode_velodyne(d, 32, (0, 4, 8, 16), 64)
    oh, n_h = h.decode_velodyne(d, 32, (0, 4, 8, 16), 64)
    assert n_o == 1 and oo[0, 3] == 6
    assert n_h == n_o
    np.testing.assert_array_equal(_bits(oh), _bits(oo))


@pytest.mark.gpu
def test_hip_decode_refuses_invalid_layouts(hip_lib):
    import ctypes as C
    h = make_hip(hip_lib, _cfg())
    xyzi = _velo_xyzi(_velo_msg(64, seed=2)[0])
    f = h._f("decode_velodyne"); f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int32] * 7 + [C.c_void_p, C.c_void_p]
    d = np.ascontiguousarray(_velo_pack(xyzi, 64, (0, 4, 8, 12)))
    out = np.zeros((len(d), 5), np.float32)

    def call(step, offs, n_scans=64, n=len(d)):
        n_out = C.c_int32(-7)
        rc = f(h.ctx, d.ctypes.data_as(C.c_void_p), n, step, *offs, n_scans, out.ctypes.data_as(C.c_void_p), C.byref(n_out))
        return rc, n_out.value
    IMMESH_E_INVAL = -1
    for step, offs in ((16, (0, 4, 8, 13)), (32, (0, 4, 29, 16)), (15, (0, 4, 8, 11)), (65, (0, 4, 8, 12)), (64, (0, 4, 8, 61)),
                       (32, (-1, 4, 8, 16)), (32, (0, 4, 8, -4)), (8, (0, 4, 0, 4))):
        assert call(step, offs)[0] == IMMESH_E_INVAL, (step, offs)
    assert call(32, (0, 4, 8, 16), n_scans=0)[0] == IMMESH_E_INVAL
    assert call(32, (0, 4, 8, 16), n=0)[0] == IMMESH_E_INVAL
    rc, n = call(16, (0, 4, 8, 12))                                         # the edges that are allowed: step 16 and 64, a field ending at the step
    assert rc == 0 and n > 0
    assert call(64, (48, 52, 56, 60))[0] == 0
    dead = np.array([(0, 0, 1, 1), (0, 0, 0, 2), (np.nan, 0, 0, 3), (1, 0, 0.5, 4), (1, 0, -1, 5)] * 20, np.float32)   # every point dropped
    oh, n_h = h.decode_velodyne(_velo_pack(dead, 32, (0, 4, 8, 16)), 32, (0, 4, 8, 16), 64)
    assert n_h == 0 and len(oh) == 0


@pytest.mark.gpu
def test_hip_front_end_chain_matches_the_checker(oracle_lib, hip_lib):
    """decode -> undistort -> downsample on device pointers, each stage compared with the checker's chain: the decode bit for bit with the
    oracle's, the undistortion of the device-resident decode within one float spacing (order exact) of the oracle's undistortion of the
    oracle's decode, the VoxelGrid of the device-resident cloud bit for bit with synth.voxel_grid_downsample of the fetched cloud.  The
    velodyne message carries no-return points (origin, NaN): nothing non-finite reaches the VoxelGrid."""
    import ctypes as C
    from immesh_amd import synth
    from test_undistort import _assert_within_one_spacing
    cfg = _cfg()
    o, h = make_oracle(oracle_lib, cfg), make_hip(hip_lib, cfg)
    lm = _livox_msg(120000, seed=5)
    vm = _velo_xyzi(_velo_msg(130000, seed=6)[0])
    rng = np.random.default_rng(8)
    holes = rng.choice(len(vm), 3000, replace=False)
    vm[holes[:1000], :3] = 0.0
    vm[holes[1000:], rng.integers(0, 3, 2000)] = np.nan
    vd = _velo_pack(vm, 32, (0, 4, 8, 16))
    imu = np.zeros((8, 7)); imu[:, 0] = np.linspace(0.0125, 0.1, 8)
    imu[:, 1:4] = (0.1, -0.2, 0.6); imu[:, 4:7] = (0.3, -0.2, 9.9)
    f = h._f("undistort"); f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    for kind, decode in (("livox", lambda lib, **kw: lib.decode_livox(lm.view(np.uint8).reshape(-1, 19), 6, 1, 1.0, **kw)),
                         ("velodyne", lambda lib, **kw: lib.decode_velodyne(vd, 32, (0, 4, 8, 16), 64, **kw))):
        oo, n_o = decode(o)
        _, n = decode(h, to_host=False)
        dec = fetch_device(h.decode_result_ptr(), (n, 5))
        assert n == n_o, kind
        np.testing.assert_array_equal(_bits(dec), _bits(oo), err_msg=kind)
        st = capi.make_state(cov_diag=1e-4); st[12:15] = (1.5, 0.2, -0.1); st[21:24] = [0, 0, -9.81]
        ic_o, ic_h = capi.make_imu_ctx(cfg, gyr0=(0.1, -0.2, 0.6)), capi.make_imu_ctx(cfg, gyr0=(0.1, -0.2, 0.6))
        und_o, st_o, _ = o.undistort(oo, imu, 0.0, 0.0, ic_o, st)
        st_h, lut = st.copy(), C.c_double(0.0)
        assert f(h.ctx, C.c_void_p(h.decode_result_ptr()), n, imu.ctypes.data_as(C.c_void_p), len(imu), 0.0, C.byref(lut), C.byref(ic_h),
                 st_h.ctypes.data_as(C.c_void_p), None) == 0
        und = fetch_device(h.undistort_result_ptr(), (n, 4))
        _assert_within_one_spacing(und, und_o, kind)
        np.testing.assert_allclose(st_h, st_o, rtol=1e-11, atol=1e-14)
        assert np.all(np.isfinite(und[:, :3])), kind
        ds, n_ds = h.downsample(h.undistort_result_ptr(), 0.4, n=n, stride=4, to_host=True)
        ref = synth.voxel_grid_downsample(und, 0.4)
        assert n_ds == len(ref) and 1000 < n_ds < n, kind
        np.testing.assert_array_equal(_bits(ds), _bits(ref), err_msg=kind)
