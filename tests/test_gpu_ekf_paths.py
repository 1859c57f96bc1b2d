"""The device forms of the 18-state iterated update (COVERAGE.md row a14) on every route, decision path and grid boundary: the resident grid
(rp_update / rp_posterior in residual_persistent_kernel), the per-pass chain (ekf_step_wave in ekf_step_kernel, reached through IMMESH_RP_FORCE_ABORT) and
the host loop (imh::EkfLoop::step, IMMESH_HOST_EKF or max_iter outside [2, 62)), against the oracle on the case table of tests/ekf_checker.py.

Per case and route: n_iter and n_match equal the oracle's; state and covariance within the case's bound (C_DEVICE * sum_k b_k, + the format floor on the
state -- ekf_checker.py) of the oracle's; the routes within twice that of each other; a second call gives the same bits.  tests/test_ekf_cpu.py holds the
CPU side: the oracle against the long-double checker, and that every case's outcome is robust under a perturbation of the size of its bound."""
import ctypes as C
import os

import numpy as np
import pytest

import ekf_checker as K
from conftest import make_hip, make_oracle
from parity_utils import clouds_within_rounding, compare_plane_tables

pytestmark = pytest.mark.gpu

ROUTE_ENV = {"resident": {}, "chain": {"IMMESH_RP_FORCE_ABORT": "1"}, "host": {"IMMESH_HOST_EKF": "1"}}


def _make_ctx(hip_lib, route, max_iter, rp_blocks=0, **caps):
    env = dict(ROUTE_ENV[route])
    if route == "host" and not 2 <= max_iter < 62:
        env = {}                                   # the edges of use_fused_ekf send these to the host loop by themselves
    if rp_blocks:
        env["IMMESH_RP_BLOCKS"] = str(rp_blocks)
    assert not any(k in os.environ for k in ("IMMESH_RP_FORCE_ABORT", "IMMESH_HOST_EKF", "IMMESH_RP_BLOCKS"))
    os.environ.update(env)
    try:
        cfg = K.config(max_iter)
        for k, v in caps.items():
            setattr(cfg, k, v)
        return make_hip(hip_lib, cfg)
    finally:
        for k in env:
            del os.environ[k]


class Contexts:
    """one context per route / knob / max_iter, the map built once (immesh_register does not change it)"""
    def __init__(self, hip_lib, scene):
        self.lib, self.scene, self.ctx = hip_lib, scene, {}

    def get(self, route, max_iter, rp_blocks=0):
        key = (route, max_iter, rp_blocks)
        if key not in self.ctx:
            h = _make_ctx(self.lib, route, max_iter, rp_blocks)
            h.map_build(self.scene.map_pts, self.scene.st0)
            self.ctx[key] = h
        return self.ctx[key]


@pytest.fixture(scope="module")
def sc(oracle_lib):
    return K.scene(oracle_lib)


@pytest.fixture(scope="module")
def ctxs(hip_lib, sc):
    c = Contexts(hip_lib, sc)
    yield c
    for h in c.ctx.values():
        h.close()


@pytest.mark.parametrize("name", [c.name for c in K.CASES])
def test_case_on_every_route(sc, ctxs, name):
    case = K.CASE_BY_NAME[name]
    r = sc.result(case)
    prior, state = sc.inputs(case)
    pts = sc.points(case)
    outs, problems = {}, []
    for route in case.routes:
        h = ctxs.get(route, case.max_iter, case.rp_blocks)
        fb = h.registration_fallbacks()
        s1, i1 = h.register(pts, prior, state)
        s2, i2 = h.register(pts, prior, state)
        fb = h.registration_fallbacks() - fb
        outs[route] = s1
        e_st, e_cov = np.abs(s1[:24] - r["post"][:24]).max(), np.abs(s1[24:] - r["post"][24:]).max()
        print(f"{name} [{route}]: n_iter {i1['n_iter']} (oracle {r['n_iter']}) n_match {i1['n_match']} (oracle {r['n_match']}) |state - oracle| {e_st:.3e} "
              f"(bound {r['bound_state']:.3e}) |cov - oracle| {e_cov:.3e} (bound {r['bound_cov']:.3e}) fallbacks {fb}")
        if fb != (2 if route == "chain" else 0):
            problems.append(f"{route}: {fb} fallbacks to the per-pass chain in two registrations")
        if (i1["n_iter"], i1["n_match"]) != (r["n_iter"], r["n_match"]):
            problems.append(f"{route}: n_iter / n_match {i1['n_iter']} / {i1['n_match']}, oracle {r['n_iter']} / {r['n_match']}")
        if not e_st <= r["bound_state"]:
            problems.append(f"{route}: state differs from the oracle's by {e_st:.3e} > {r['bound_state']:.3e}")
        if not e_cov <= r["bound_cov"]:
            problems.append(f"{route}: covariance differs from the oracle's by {e_cov:.3e} > {r['bound_cov']:.3e}")
        if s1.tobytes() != s2.tobytes() or i1 != i2:
            problems.append(f"{route}: a second call gave other bits ({np.abs(s1 - s2).max():.3e})")
    routes = list(outs)
    for i, a in enumerate(routes):
        for b in routes[i + 1:]:
            d_st, d_cov = np.abs(outs[a][:24] - outs[b][:24]).max(), np.abs(outs[a][24:] - outs[b][24:]).max()
            print(f"{name} [{a} - {b}]: state {d_st:.3e} covariance {d_cov:.3e}")
            if not (d_st <= 2 * r["bound_state"] and d_cov <= 2 * r["bound_cov"]):
                problems.append(f"{a} and {b} differ by {d_st:.3e} / {d_cov:.3e} (state / covariance)")
    assert not problems, "\n".join(problems)


@pytest.mark.parametrize("n_raw", [4096, 4097])
def test_epilogue_prefetch_and_its_remainder_loop(oracle_lib, hip_lib, sc, n_raw):
    """The resident grid's epilogue moves the full scan into the mesher's world buffer 16 points per thread with a remainder loop behind: n_ds = 200 is one
    workgroup (G = 1), so n_raw = 16 * 256 * G = 4096 is exactly the prefetched part and 4097 leaves one point to the remainder.  The world cloud equals the
    formula at the device's own posterior, and the plane table after the map update (the epilogue prepared it) equals the oracle's.  (The scan is meshed:
    without a mesh job the epilogue is handed no full scan at all.)"""
    h = _make_ctx(hip_lib, "resident", 4)
    o = make_oracle(oracle_lib, K.config(4))
    h.map_build(sc.map_pts, sc.st0); o.map_build(sc.map_pts, sc.st0)
    down = np.ascontiguousarray(sc.down[::27][:200])
    raw = np.ascontiguousarray(sc.raw1[:n_raw])
    assert len(down) == 200 and len(raw) == n_raw
    prior = K.pose_prior(0.3, 1e-4)
    sh, ih = h.process_scan(down, raw, prior, prior, frame_idx=1, do_mesh=1)
    so, io = o.process_scan(down, raw, prior, prior, frame_idx=1, do_mesh=1)
    assert ih == io and h.registration_fallbacks() == 0, (ih, io)
    np.testing.assert_allclose(sh[:24], so[:24], rtol=0, atol=1e-9)
    world = h.mesh_world_scan()
    assert world.shape == (n_raw, 4)
    cfg = K.config(4)
    extR, extT = np.array(list(cfg.extR)).reshape(3, 3), np.array(list(cfg.extT))
    want = ((raw[:, :3].astype(np.float64) @ extR.T + extT) @ sh[:9].reshape(3, 3).T + sh[9:12]).astype(np.float32)
    assert clouds_within_rounding(world[:, :3], want)
    np.testing.assert_array_equal(world[:, 3], raw[:, 3])
    assert compare_plane_tables(o.dump_planes(), h.dump_planes()) > 100
    h.close()


def _raw_register(h, pts, prior, state):
    f = h.lib.immesh_register; f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int32] + [C.c_void_p] * 7
    buf = np.array(state, np.float64, copy=True)
    rc = f(h.ctx, pts.ctypes.data_as(C.c_void_p), len(pts), np.ascontiguousarray(prior).ctypes.data_as(C.c_void_p), buf.ctypes.data_as(C.c_void_p), None, None, None, None, None)
    e = h.lib.immesh_last_error; e.restype = C.c_char_p; e.argtypes = [C.c_void_p]
    return rc, e(h.ctx).decode(), buf


def _raw_process_scan(h, down, raw, prior, state):
    f = h.lib.immesh_process_scan; f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    buf = np.array(state, np.float64, copy=True)
    rc = f(h.ctx, down.ctypes.data_as(C.c_void_p), len(down), raw.ctypes.data_as(C.c_void_p), len(raw), np.ascontiguousarray(prior).ctypes.data_as(C.c_void_p),
           buf.ctypes.data_as(C.c_void_p), 1, 0, None, None)
    e = h.lib.immesh_last_error; e.restype = C.c_char_p; e.argtypes = [C.c_void_p]
    return rc, e(h.ctx).decode(), buf


@pytest.mark.parametrize("route", K.ALL_ROUTES)
def test_singular_prior_is_refused_the_same_way_on_every_route(hip_lib, sc, route):
    """include/immesh_c_api.h, immesh_register: a prior covariance whose 6 x 6 pose block is not finite and invertible is refused on the host, before
    anything is launched (so no kernel ever sees it): IMMESH_E_INVAL and one text on every route, state_inout untouched, and the next good registration on
    the context equals a fresh context's bit for bit."""
    h, fresh = _make_ctx(hip_lib, route, 4), _make_ctx(hip_lib, route, 4)
    h.map_build(sc.map_pts, sc.st0); fresh.map_build(sc.map_pts, sc.st0)
    good = K.pose_prior(0.3, 1e-4)
    raw = np.ascontiguousarray(sc.raw1[:4096])
    for tag, P in K.singular_covariances().items():
        bad = good.copy(); bad[24:] = P.reshape(-1)
        for call in (lambda: _raw_register(h, sc.down, bad, bad), lambda: _raw_process_scan(h, sc.down, raw, bad, bad)):
            rc, text, buf = call()
            assert (rc, text) == (-1, "singular prior covariance"), (route, tag, rc, text)       # IMMESH_E_INVAL
            assert buf.tobytes() == bad.tobytes(), (route, tag)
    s_h, i_h = h.register(sc.down, good, good)
    s_f, i_f = fresh.register(sc.down, good, good)
    assert i_h == i_f and s_h.tobytes() == s_f.tobytes()
    r = sc.result(K.CASE_BY_NAME["a-scale0.3-cov0.0001"])
    assert (i_h["n_iter"], i_h["n_match"]) == (r["n_iter"], r["n_match"])
    assert h.registration_fallbacks() == (1 if route == "chain" else 0)
    h.close(); fresh.close()
