"""The VoxelGrid down-sampling (COVERAGE.md row f1: immesh_downsample, immesh_downsample_begin / _end; ds_kernels.hip, pre_host.cpp) route by route on the
clouds of tests/downsample_cases.py, every one of whose claims test_downsample_cases_cpu.py shows on the spec and the checker first.

The hashed form (ds_hash_kernel, ds_leaf_sort_kernel, ds_scatter_kernel, ds_leaf_emit_kernel) and the radix pipeline (ds_minmax_kernel, ds_index_kernel, the
sort, ds_heads_kernel, ds_centroid_kernel) give the same bits by design, so no comparison of results shows which one ran.  The in-library profiler does: every
route assertion below is the pair (launches of ds_hash_kernel, launches of ds_minmax_kernel) of ONE call, against the route the case predicts from how it was
built -- (1, 0) hashed, (1, 1) given up and redone, (0, 1) on an IMMESH_DS_RADIX context.  With the profiler on the asynchronous pair runs without its graph
(and without its gate), so its route is taken with the profiler on and its result, through the graph, with the profiler off.

Every result is compared with synth.voxel_grid_downsample bit for bit: the count and all values."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import downsample_cases as D
from immesh_amd import capi, synth
from conftest import make_hip, fetch_device

pytestmark = pytest.mark.gpu

HASHED, GAVE_UP, RADIX_ONLY = (1, 0), (1, 1), (0, 1)


def _cfg(cap_scan=1 << 18):
    return capi.avia_config(cap_root_voxels=1 << 12, cap_scan_points=cap_scan, cap_vertices=1 << 16, cap_triangles=1 << 18)


def _make_ctx(hip_lib, cfg, **env):
    assert "IMMESH_DS_RADIX" not in os.environ
    os.environ.update(env)
    try:
        return make_hip(hip_lib, cfg)
    finally:
        for k in env:
            del os.environ[k]


@pytest.fixture(scope="module")
def ctxs(hip_lib):
    """(default context, IMMESH_DS_RADIX context), shared by the module: what one cloud leaves behind the next one meets"""
    h = _make_ctx(hip_lib, _cfg())
    hr = _make_ctx(hip_lib, _cfg(), IMMESH_DS_RADIX="1")
    yield h, hr
    h.close(); hr.close()


@functools.lru_cache(maxsize=None)
def _spec(name):
    c = D.ordinary() if name == "ordinary" else D.by_name(name)
    ref = synth.voxel_grid_downsample(c.pts, c.leaf)
    assert len(ref) == c.n_leaves
    ref.setflags(write=False)
    return ref


def _route(h):
    p = h.profile_read(reset=True)
    return tuple(int(p.get(k, {"launches": 0})["launches"]) for k in ("ds_hash_kernel", "ds_minmax_kernel"))


def _same(got, n, ref, what):
    assert n == len(ref), what
    assert got.shape == ref.shape and got.tobytes() == ref.tobytes(), what


def _ordinary_takes_the_hashed_form(h, pair):
    """right behind a fall-back: a table left occupied or counters left set would send this cloud to the radix pipeline too"""
    o = D.ordinary()
    if pair:
        h.downsample_begin(o.pts, o.leaf)
        n, ptr = h.downsample_end()
        got = fetch_device(ptr, (n, 3))
    else:
        got, n = h.downsample(o.pts, o.leaf)
    assert _route(h) == HASHED, "the cloud behind a fall-back fell back too" + (" (pair)" if pair else "")
    _same(got, n, _spec("ordinary"), "ordinary behind a fall-back")


def _check(h, hr, c, pts, ref):
    import torch
    want = HASHED if c.route == "hash" else GAVE_UP
    stride = pts.shape[1]
    tag = f"{c.name} (stride {stride})"
    d = torch.from_numpy(pts.copy()).cuda()
    h.profile_enable(True); hr.profile_enable(True)
    try:
        h.profile_read(reset=True); hr.profile_read(reset=True)
        # host input, host output -- and the same bytes a second time
        got, n = h.downsample(pts, c.leaf)
        assert _route(h) == want, tag
        _same(got, n, ref, tag)
        if want == GAVE_UP:
            _ordinary_takes_the_hashed_form(h, pair=False)
        got2, n2 = h.downsample(pts, c.leaf)
        assert _route(h) == want, tag + " second call"
        _same(got2, n2, ref, tag + " second call")
        # device input, no output buffer: the result stays in the context
        _, n3 = h.downsample(d.data_ptr(), c.leaf, n=len(pts), stride=stride, to_host=False)
        assert _route(h) == want, tag + " device input"
        _same(fetch_device(h.downsample_result_ptr(), (n3, 3)), n3, ref, tag + " device input, device-resident result")
        # the asynchronous pair, plain launches: its route
        h.downsample_begin(d.data_ptr(), c.leaf, n=len(pts), stride=stride)
        n4, ptr = h.downsample_end()
        assert _route(h) == want, tag + " pair"
        _same(fetch_device(ptr, (n4, 3)), n4, ref, tag + " pair, profiler on")
        if want == GAVE_UP:
            _ordinary_takes_the_hashed_form(h, pair=True)
        # the radix pipeline alone
        gr, nr = hr.downsample(pts, c.leaf)
        assert _route(hr) == RADIX_ONLY, tag
        _same(gr, nr, ref, tag + " IMMESH_DS_RADIX")
        assert gr.tobytes() == got.tobytes(), tag
        _, nr2 = hr.downsample(d.data_ptr(), c.leaf, n=len(pts), stride=stride, to_host=False)
        _same(fetch_device(hr.downsample_result_ptr(), (nr2, 3)), nr2, ref, tag + " IMMESH_DS_RADIX, device-resident")
    finally:
        h.profile_enable(False); hr.profile_enable(False)
    # the pair as the scan loop runs it: one graph launch; host cloud (staged by the job) and device cloud
    for src, kw in ((pts, {}), (d.data_ptr(), {"n": len(pts), "stride": stride})):
        h.downsample_begin(src, c.leaf, **kw)
        n5, ptr = h.downsample_end()
        _same(fetch_device(ptr, (n5, 3)), n5, ref, tag + " pair, graph")
    hr.downsample_begin(pts, c.leaf)
    n6, ptr = hr.downsample_end()
    _same(fetch_device(ptr, (n6, 3)), n6, ref, tag + " pair on the IMMESH_DS_RADIX context")


def test_the_profiler_names_the_route(ctxs):
    """the premise of every route assertion, on a cloud nothing is special about: one call is one ds_hash_kernel launch on the default context and none of
    ds_minmax_kernel; on the IMMESH_DS_RADIX context it is the other way round; the pair counts the same way; with the profiler off nothing is counted"""
    h, hr = ctxs
    o = D.ordinary()
    assert o.route == "hash"
    for ctx, want in ((h, HASHED), (hr, RADIX_ONLY)):
        ctx.profile_enable(True)
        try:
            ctx.profile_read(reset=True)
            got, n = ctx.downsample(o.pts, o.leaf)
            prof = ctx.profile_read()
            assert _route(ctx) == want
            _same(got, n, _spec("ordinary"), "ordinary")
            if want == HASHED:
                assert {k: prof[k]["launches"] for k in ("ds_leaf_sort_kernel", "ds_scatter_kernel", "ds_leaf_emit_kernel", "ds_publish_kernel")} == \
                    {"ds_leaf_sort_kernel": 1, "ds_scatter_kernel": 1, "ds_leaf_emit_kernel": 1, "ds_publish_kernel": 1}
                assert prof.get("ds_centroid_kernel", {"launches": 0})["launches"] == 0
                ctx.downsample_begin(o.pts, o.leaf)
                n2, ptr = ctx.downsample_end()
                assert _route(ctx) == HASHED
                _same(fetch_device(ptr, (n2, 3)), n2, _spec("ordinary"), "ordinary, pair")
            else:
                assert {k: prof[k]["launches"] for k in ("ds_index_kernel", "ds_heads_kernel", "ds_centroid_kernel")} == \
                    {"ds_index_kernel": 1, "ds_heads_kernel": 1, "ds_centroid_kernel": 1}
            assert _route(ctx) == (0, 0)
        finally:
            ctx.profile_enable(False)
        ctx.downsample(o.pts, o.leaf)
        assert _route(ctx) == (0, 0)


CASES = [c.name for f in D.FAMILIES if f != "big-radix" for c in D.family(f)]


@pytest.mark.parametrize("name", CASES)
def test_every_case_on_every_route(ctxs, name):
    """synchronous entry (host and device input, host and device-resident output, twice), the asynchronous pair (plain launches and graph), the radix
    pipeline alone: counts and values against the spec, the route against the case's prediction, and an ordinary cloud hashed right behind every fall-back"""
    h, hr = ctxs
    c = D.by_name(name)
    _check(h, hr, c, c.pts, _spec(name))


@pytest.mark.parametrize("name", D.STRIDE3)
def test_three_floats_per_point(ctxs, name):
    """the same through n x 3 arrays, from host memory and from a device pointer"""
    h, hr = ctxs
    c = D.by_name(name)
    _check(h, hr, c, c.xyz3(), _spec(name))


def test_minmax_grid_stride_above_262144_points(hip_lib):
    """ds_minmax_kernel's 1024 workgroups of 256 threads stride from 262 145 points on; the extremes of this cloud lie with points of the second sweep.
    Contexts of cap_scan_points = 1 << 19."""
    (c,) = D.family("big-radix")
    ref = synth.voxel_grid_downsample(c.pts, c.leaf)
    assert len(ref) == c.n_leaves and min(q for q, _ in c.pinned) >= 262144
    h = _make_ctx(hip_lib, _cfg(1 << 19))
    hr = _make_ctx(hip_lib, _cfg(1 << 19), IMMESH_DS_RADIX="1")
    try:
        _check(h, hr, c, c.pts, ref)
    finally:
        h.close(); hr.close()


def test_the_result_of_a_job_outlives_the_next_job(ctxs):
    """include/immesh_c_api.h: _end's result is `valid until the second _begin after it`.  Job k's buffer read again after job k + 1 (another cloud) has
    been begun and collected: unchanged -- whether k, k + 1 or both were redone by the radix pipeline inside _end.  After job k + 2 nothing is promised."""
    h, _ = ctxs
    names = ("sizes", "ordinary", "sizes+2049", "key-x-hi-out", "many-long-770x65", "sizes+2049", "sizes", "tiles-run200")
    prev = None
    for name in names:
        c = D.ordinary() if name == "ordinary" else D.by_name(name)
        h.downsample_begin(c.pts, c.leaf)
        n, ptr = h.downsample_end()
        got = fetch_device(ptr, (n, 3))
        _same(got, n, _spec(name), name)
        if prev is not None:
            pname, pptr, pgot = prev
            assert pptr != ptr
            assert fetch_device(pptr, pgot.shape).tobytes() == pgot.tobytes(), f"job {pname}'s result changed under job {name}"
        prev = (name, ptr, got)


def test_the_pair_behind_an_asynchronous_scan(hip_lib):
    """behind an asynchronous immesh_process_scan the job is held at its gate (here no registration follows: the gate's own bound lets it through).
    Graph and gate together, on hashed clouds and on clouds that are redone inside _end."""
    import torch
    cfg = capi.avia_config(cap_root_voxels=1 << 16, cap_scan_points=100000)
    h = make_hip(hip_lib, cfg)
    try:
        extT = np.array(list(cfg.extT))
        R0, t0 = synth.trajectory_pose(0)
        raw0 = np.ascontiguousarray(synth.livox_scan(0, R0, t0, n_pts=30000, extT=extT))
        st = capi.make_state(R=R0, t=t0)
        h.map_build(np.ascontiguousarray(raw0[:, :3]), st)
        st[12:15] = [1.0, 0, 0]; st[15:18] = [0, 0, np.deg2rad(2.0)]
        R1, t1 = synth.trajectory_pose(1)
        raw1 = np.ascontiguousarray(synth.livox_scan(1, R1, t1, n_pts=30000, extT=extT))
        down1 = np.ascontiguousarray(synth.voxel_grid_downsample(raw1, 0.4))
        d_raw, d_down = torch.from_numpy(raw1).cuda(), torch.from_numpy(down1).cuda()
        prior = synth.forward_without_imu(st)
        h.process_scan(d_down.data_ptr(), d_raw.data_ptr(), prior, prior, frame_idx=1, do_mesh=0x10, n_ds=len(down1), n_raw=len(raw1))   # (no wait: the scan loop's form)
        for name in ("sizes", "sizes+2049", "ordinary", "key-x-hi-out", "key-y-lo-out", "ordinary", "many-long-770x65", "tiles-run64-at63"):
            c = D.ordinary() if name == "ordinary" else D.by_name(name)
            h.downsample_begin(c.pts, c.leaf)
            n, ptr = h.downsample_end()
            _same(fetch_device(ptr, (n, 3)), n, _spec(name), name)
    finally:
        h.close()


# ---- arguments and capacities ---------------------------------------------------------------------------------------
def _raw(h):
    f = h._f("downsample"); f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.c_void_p, C.c_int32, C.c_void_p]
    b = h._f("downsample_begin"); b.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_double]; b.restype = C.c_int
    e = h._f("downsample_end"); e.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_void_p)]; e.restype = C.c_int
    le = h.lib.immesh_last_error; le.restype = C.c_char_p; le.argtypes = [C.c_void_p]
    return f, b, e, (lambda: le(h.ctx).decode())


def _still_usable(h):
    o = D.ordinary()
    got, n = h.downsample(o.pts, o.leaf)
    _same(got, n, _spec("ordinary"), "the context after a refused call")


def test_bad_arguments_are_refused_with_a_text_and_leave_the_context_usable(ctxs):
    h, _ = ctxs
    f, b, e, err = _raw(h)
    o = D.ordinary()
    p = o.pts.ctypes.data_as(C.c_void_p)
    out = np.zeros((o.n, 3), np.float32)
    po = out.ctypes.data_as(C.c_void_p)
    n_out = C.c_int32(-7)
    cap = int(h.cfg.cap_scan_points)
    tiny = 1e-39            # 1 / leaf = 1e39: above the largest float32, the factor would be infinite
    with np.errstate(over="ignore", under="ignore"):
        assert np.isinf(np.float32(1.0 / tiny)) and np.float32(1.0 / 1e300) == 0
    bad = [("n = 0", 0, 4, 0.5), ("n above cap_scan_points", cap + 1, 4, 0.5), ("stride 5", o.n, 5, 0.5), ("stride 2", o.n, 2, 0.5), ("leaf 0", o.n, 4, 0.0),
           ("leaf negative", o.n, 4, -0.4), ("leaf NaN", o.n, 4, float("nan")), ("leaf with an infinite 1 / leaf", o.n, 4, tiny), ("leaf infinite", o.n, 4, float("inf")),
           ("leaf with 1 / leaf == 0 in float32", o.n, 4, 1e300)]
    for what, n, stride, leaf in bad:
        n_out.value = -7
        assert f(h.ctx, p, n, stride, leaf, po, o.n, C.byref(n_out)) == capi.E_INVAL, what
        assert err() == "bad arguments" and n_out.value == -7, what
        assert b(h.ctx, p, n, stride, leaf) == capi.E_INVAL, what + " (_begin)"
        assert err() == "bad arguments", what
        ne, ptr = C.c_int32(0), C.c_void_p(0)
        assert e(h.ctx, C.byref(ne), C.byref(ptr)) == capi.E_INVAL and "no job in flight" in err(), what      # the refused _begin left no job behind
        _still_usable(h)
    assert f(h.ctx, p, o.n, 4, 0.5, po, o.n, None) == capi.E_INVAL and err() == "bad arguments"               # n_out NULL
    assert f(h.ctx, None, o.n, 4, 0.5, po, o.n, C.byref(n_out)) == capi.E_INVAL and err() == "bad arguments"  # pts NULL
    _still_usable(h)


def test_an_output_buffer_one_leaf_short(ctxs):
    """IMMESH_E_CAPACITY, *n_out set to the leaf count, nothing written to the buffer, and the whole result still on the device -- on both routes"""
    h, hr = ctxs
    f, _, _, err = _raw(h)
    for ctx in (h, hr):
        for name in ("ordinary", "sizes+2049"):
            c = D.ordinary() if name == "ordinary" else D.by_name(name)
            ref = _spec(name)
            out = np.full((len(ref), 3), -5.0, np.float32)
            n_out = C.c_int32(0)
            rc = f(ctx.ctx, c.pts.ctypes.data_as(C.c_void_p), c.n, 4, c.leaf, out.ctypes.data_as(C.c_void_p), len(ref) - 1, C.byref(n_out))
            le = ctx.lib.immesh_last_error; le.restype = C.c_char_p; le.argtypes = [C.c_void_p]
            assert rc == capi.E_CAPACITY and le(ctx.ctx).decode() == "output buffer too small", name
            assert n_out.value == len(ref) and (out == -5.0).all(), name
            _same(fetch_device(ctx.downsample_result_ptr(), (len(ref), 3)), n_out.value, ref, name + ": the device-resident result of a call refused for capacity")
            rc = f(ctx.ctx, c.pts.ctypes.data_as(C.c_void_p), c.n, 4, c.leaf, out.ctypes.data_as(C.c_void_p), len(ref), C.byref(n_out))     # exactly enough
            assert rc == 0
            _same(out, n_out.value, ref, name + " into a buffer of exactly n_out leaves")
            _still_usable(ctx)


def test_begin_twice_and_end_without_a_job(ctxs):
    h, _ = ctxs
    _, b, e, err = _raw(h)
    n, ptr = C.c_int32(0), C.c_void_p(0)
    assert e(h.ctx, C.byref(n), C.byref(ptr)) == capi.E_INVAL and err() == "immesh_downsample_end: no job in flight"
    c, o = D.by_name("sizes"), D.ordinary()
    h.downsample_begin(c.pts, c.leaf)
    assert b(h.ctx, o.pts.ctypes.data_as(C.c_void_p), o.n, 4, o.leaf) == capi.E_INVAL and "has not been collected" in err()
    with pytest.raises(RuntimeError, match="asynchronous job is in flight"):
        h.downsample(o.pts, o.leaf)
    ng, p = h.downsample_end()                       # the job the refused calls found in flight: untouched by them
    _same(fetch_device(p, (ng, 3)), ng, _spec("sizes"), "the job behind a refused second _begin")
    assert e(h.ctx, C.byref(n), C.byref(ptr)) == capi.E_INVAL and err() == "immesh_downsample_end: no job in flight"
    _still_usable(h)
