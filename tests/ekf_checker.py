"""The 18-state iterated update (COVERAGE.md row a14) restated in numpy.longdouble, the case table that the CPU tier (test_ekf_cpu.py) and the GPU tier
(test_gpu_ekf_paths.py) share, and the bound both compare values under.

The checker is ONE step of the reference's algebra as ekf_host.hpp restates it (src/voxel_mapping.cpp:1585-1646): S = H^T R^-1 H (padded to 18 x 18)
+ P^-1, K1 = S^-1 by one full 18 x 18 solve (no block form, no regrouping), G = K1 HTH, solution = K1 HTz + vec - G vec with vec = prior [-] state,
state [+]= solution, the convergence / rematch / stop rule, and at a stop the posterior (I - G) P.  Exp / Log keep the reference's thresholds: Exp is the
identity below 1e-5, Log is 0.5 K below 1e-3 (include/so3_math.h:71-98).

Bound.  The rounding of one step scales as
    b_k = eps * (kappa_2(P) + kappa_2(S_k)) * max(|sol_k|_inf, |vec_k|_inf)          (for the covariance: |P|_max in place of the last factor)
with eps = 2^-52; the constant in front of it is measured on the CPU -- C_ORC, the largest |oracle step - longdouble step| / b_k over every iteration
of every case (test_ekf_cpu.py asserts it), floored at 1 -- and the device forms get C = 16 * C_ORC rounded up to a power of two: they chain a 6 x 6
inverse, a 12 x 6 product and a regrouped solution where the oracle does one inverse; the same kappa * eps form, a larger constant.  The bound on a
posterior is C * sum_k b_k (the step is a contraction near its fixed point while the match set holds, so the per-pass errors add at most).

b_k describes the ALGEBRA of a step and vanishes with the solution; the iterate it is added to does not: R <- R Exp(sol) and t <- t + sol are rounded
to double whatever the size of `sol`.  FORMAT_FLOOR is that rounding per pass (below) and is added to a bound on a STATE, never multiplied by C."""
import ctypes as C

import numpy as np

from immesh_amd import capi, synth

LD = np.longdouble
EPS = 2.0 ** -52

# Measured on the CPU by test_ekf_cpu.py::test_oracle_step_equals_the_longdouble_step_on_every_iteration, oracle against this checker only (never
# against a device form): raw value beside the constant.
C_ORC_MEASURED = 5.867   # at a-scale0-cov1e-10, pass 0 (state == prior held tight: a solution of 1e-14 against a `vec` that is Log of R^T R in double)
C_ORC = 6.0              # the measured value rounded up to the next integer (another libm's last bit must not fail the measurement)
C_DEVICE = 128.0         # 16 * C_ORC = 96, rounded up to a power of two
# Rounding of the iterate itself in one pass, in units of eps * max(1, |state|_inf): the 3 x 3 product R Exp(sol) is three-term sums of products of
# entries <= 1 whose factors (sin, 1 - cos, the normalised axis, K K) each carry an ulp or two -- 8 eps covers it -- and t + sol is half an ulp of t.
FORMAT_FLOOR = 8.0


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# one step in long double
def _inv(A):
    """Gauss-Jordan with partial pivoting in long double (numpy.linalg has no long double)"""
    n = len(A)
    M = np.concatenate([np.array(A, LD), np.eye(n, dtype=LD)], axis=1)
    for col in range(n):
        piv = col + int(np.argmax(np.abs(M[col:, col])))
        if M[piv, col] == 0:
            raise np.linalg.LinAlgError("singular")
        if piv != col:
            M[[piv, col]] = M[[col, piv]]
        M[col] = M[col] / M[col, col]
        f = M[:, col].copy(); f[col] = 0
        M -= f[:, None] * M[col][None, :]
    return M[:, n:]


def _skew_unit(r):
    return np.array([[0, -r[2], r[1]], [r[2], 0, -r[0]], [-r[1], r[0], 0]], LD)


def exp_ld(v):
    v = np.asarray(v, LD)
    norm = np.sqrt((v * v).sum())
    if not norm > LD(0.00001):
        return np.eye(3, dtype=LD)
    K = _skew_unit(v / norm)
    return np.eye(3, dtype=LD) + np.sin(norm) * K + (LD(1) - np.cos(norm)) * (K @ K)


def log_ld(R):
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    theta = LD(0) if tr > LD(3.0) - LD(1e-6) else np.arccos(LD(0.5) * (tr - 1))
    K = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]], LD)
    if abs(theta) < LD(0.001):
        return LD(0.5) * K
    return (LD(0.5) * theta / np.sin(theta)) * K


def state_minus(a24, b24):
    a, b = np.asarray(a24, LD), np.asarray(b24, LD)
    out = np.zeros(18, LD)
    out[:3] = log_ld(b[:9].reshape(3, 3).T @ a[:9].reshape(3, 3))
    out[3:] = a[9:24] - b[9:24]
    return out


def state_plus(s24, d):
    s, d = np.array(s24, LD), np.asarray(d, LD)
    s[:9] = (s[:9].reshape(3, 3) @ exp_ld(d[:3])).reshape(-1)
    s[9:24] += d[3:]
    return s


def step(HTH, HTz, prior24, state24, P, it, rematch, max_iter):
    """One step.  HTH 36, HTz 6, prior / iterate 24 doubles (R row-major, t, vel, bg, ba, g), P 18 x 18, the pass index, the rematch count on entry.
    Returns sol, vec, the new iterate, converged, the rematch count on exit, stop, the posterior covariance (None unless stopped) and S."""
    P = np.asarray(P, LD).reshape(18, 18)
    H6 = np.asarray(HTH, LD).reshape(6, 6)
    S = _inv(P)
    S[:6, :6] += H6
    K1 = _inv(S)
    G = np.zeros((18, 18), LD)
    G[:, :6] = K1[:, :6] @ H6
    vec = state_minus(prior24, state24)
    sol = K1[:, :6] @ np.asarray(HTz, LD) + vec - G[:, :6] @ vec[:6]
    new = state_plus(state24, sol)
    rn, tn = np.sqrt((sol[:3] ** 2).sum()), np.sqrt((sol[3:6] ** 2).sum())
    converged = bool(rn * LD(57.3) < LD(0.01) and tn * 100 < LD(0.015))
    if converged or (rematch == 0 and it == max_iter - 2):
        rematch += 1
    stop = rematch >= 2 or it == max_iter - 1
    cov = (np.eye(18, dtype=LD) - G) @ P if stop else None
    return dict(sol=sol, vec=vec, state=new, converged=converged, rematch=rematch, stop=bool(stop), cov=cov, S=S)


def step_bounds(S, P, sol, vec):
    """(b_k for values, b_k for the covariance) of one step, from float64 condition numbers"""
    k = np.linalg.cond(np.asarray(P, np.float64).reshape(18, 18)) + np.linalg.cond(np.asarray(S, np.float64))
    P = np.asarray(P, np.float64)
    return EPS * k * max(np.abs(np.asarray(sol, np.float64)).max(), np.abs(np.asarray(vec, np.float64)).max()), EPS * k * np.abs(P).max()


def replay(trace, prior, state, max_iter):
    """Feed every iteration of an oracle trace (its own HTH, HTz and entry state) to the checker.  Returns per iteration the checker's step and b_k."""
    P = state[24:].reshape(18, 18)
    entry, rematch, out = np.asarray(state[:24]), 0, []
    for k, r in enumerate(trace):
        s = step(r["HTH"], r["HTz"], prior[:24], entry, P, k, rematch, max_iter)
        s["b"], s["b_cov"] = step_bounds(s["S"], P, s["sol"], s["vec"])
        out.append(s)
        rematch, entry = s["rematch"], r["state"]
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the case table
PERT_W, PERT_T = np.array([2e-3, -3e-3, 2.5e-3]), np.array([0.03, -0.02, 0.015])
DECISION_PRIORS = ((0.0, 1e-13), (0.0, 1e-10), (0.0, 1e-8), (0.02, 1e-6), (0.3, 1e-4), (1.0, 1e-4), (3.0, 1e-4))   # test_ref_lio.py's seven
DELTA_ROT = (0.0, 5e-4, 9.99e-4, 1.001e-3, 0.04, 0.049, 0.06, 0.5)   # (0.049: just inside the device's series branch, where its truncation is largest)
SIZES_DEFAULT = (1, 63, 64, 65, 255, 256, 257, 1024, 1025, 16384, 16385, 40000)
FUSED, HOST = ("resident", "chain"), ("host",)
ALL_ROUTES = FUSED + HOST


def pose_prior(scale, cov_diag):
    R1, t1 = synth.trajectory_pose(1)
    return capi.make_state(R=R1 @ synth.so3_exp(PERT_W * scale), t=t1 + PERT_T * scale, cov_diag=cov_diag)


def _with_cov(P):
    s = pose_prior(0.3, 1.0)
    s[24:] = np.asarray(P, np.float64).reshape(-1)
    return s


def _random_spd(seed, lo=1e-10, hi=1e-2):
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.normal(size=(18, 18)))
    P = (Q * np.logspace(np.log10(lo), np.log10(hi), 18)) @ Q.T
    return 0.5 * (P + P.T)


class Case:
    """name; family; max_iter; routes; pts: 'down' | 'floor' | 'far' | ('raw', n) | ('stride', k); rp_blocks (IMMESH_RP_BLOCKS, 0 = unset); make(scene) -> (prior, state)"""
    def __init__(self, name, family, make, max_iter=4, routes=ALL_ROUTES, pts="down", rp_blocks=0):
        self.name, self.family, self.make, self.max_iter, self.routes, self.pts, self.rp_blocks = name, family, make, max_iter, routes, pts, rp_blocks

    def __repr__(self):
        return self.name


def _same(make_state):
    def make(scene):
        s = make_state(scene)
        return s.copy(), s
    return make


def _delta_case(mag):
    def make(scene):
        # pose variance 1e-2: the measurement dominates.  The other twelve variances are free: 1e-5 puts their information (1e5) inside the spectrum of
        # H^T R^-1 H (1e5 .. 6e8), which keeps kappa(S) -- and with it the bound -- as small as this prior pose block allows
        state = _with_cov(np.diag([1e-2] * 6 + [1e-5] * 12))
        axis = np.array([0.6, -0.48, 0.64])                 # unit
        prior = state.copy()
        # Exp as the reference has it: the identity below 1e-5 (no listed magnitude but 0 is below)
        prior[:9] = (state[:9].reshape(3, 3) @ synth.so3_exp(axis * mag)).reshape(-1)
        prior[9:12] = state[9:12] + 0.3 * np.array([2.0, -1.0, 2.0]) / 3.0
        return prior, state
    return make


def _dense_cov(scene):
    """five forward_without_imu steps without an update from a converged posterior: strong pose-velocity (and rotation-rate) cross blocks"""
    s = scene.converged_posterior()
    for _ in range(5):
        s = synth.forward_without_imu(s)
    return _with_cov(s[24:])


CASES = []
for _sc, _cv in DECISION_PRIORS:                                                                    # (a) decision paths
    CASES.append(Case(f"a-scale{_sc:g}-cov{_cv:g}", "a", _same(lambda sc, _s=_sc, _c=_cv: pose_prior(_s, _c))))
for _mi in (2, 3, 4, 61, 1, 62):                                                                    # (b) max_iter
    for _tag, (_sc, _cv) in (("far", (3.0, 1e-4)), ("conv", (0.0, 1e-10))):
        CASES.append(Case(f"b-iter{_mi}-{_tag}", "b", _same(lambda sc, _s=_sc, _c=_cv: pose_prior(_s, _c)), max_iter=_mi, routes=HOST if _mi in (1, 62) else FUSED))
for _m in DELTA_ROT:                                                                                # (c) prior != state
    CASES.append(Case(f"c-drot{_m:g}", "c", _delta_case(_m)))
for _cv in (1e-13, 1e-2, 1e2):                                                                      # (d) covariance shapes
    # 1e+2 leaves the pose to the measurement alone: kappa(S) ~ 1e9 puts the bound at micrometres, and among the 1 600 matches of the full down-sampled
    # scan one always sits that close to its gate (test_ekf_cpu.py's robustness condition); every 16th point (339 of them, ~100 matches) is robust
    CASES.append(Case(f"d-diag{_cv:g}", "d", _same(lambda sc, _c=_cv: pose_prior(0.3, _c)), pts=("stride", 16) if _cv == 1e2 else "down"))
CASES.append(Case("d-rot1e-10-trans1e-2", "d", _same(lambda sc: _with_cov(np.diag([1e-10] * 3 + [1e-2] * 15)))))
CASES.append(Case("d-dense-propagated", "d", _same(_dense_cov)))
CASES.append(Case("d-random-spd-kappa1e8", "d", _same(lambda sc: _with_cov(_random_spd(20261018)))))
CASES.append(Case("e-floor-only", "e", _same(lambda sc: pose_prior(0.3, 1e-4)), pts="floor"))      # (e) geometry
CASES.append(Case("e-zero-matches", "e", _same(lambda sc: pose_prior(0.3, 1e-4)), pts="far"))
for _n in SIZES_DEFAULT:                                                                            # (f) sizes on the resident grid
    CASES.append(Case(f"f-n{_n}", "f", _same(lambda sc: pose_prior(0.3, 1e-4)), routes=FUSED, pts=("raw", _n)))
# IMMESH_RP_BLOCKS = 1 / 2: more tiles than 4 G at small n (the pass-independent part is recomputed per pass); 256 / 257 at G = 1 are the switch itself
for _b, _ns in ((1, (256, 257, 1024, 1025)), (2, (2048, 2049))):
    for _n in _ns:
        CASES.append(Case(f"f-blocks{_b}-n{_n}", "f", _same(lambda sc: pose_prior(0.3, 1e-4)), routes=("resident",), pts=("raw", _n), rp_blocks=_b))
CASE_BY_NAME = {c.name: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the scene and the oracle's results, computed once per process and shared
VP = C.c_void_p


def _p(a):
    return a.ctypes.data_as(VP)


def config(max_iter=4):
    return capi.avia_config(cap_root_voxels=1 << 16, cap_scan_points=100000, max_iter=max_iter)


class Scene:
    """synth.livox_scan, avia: the map is scan 0 (30 000 points), the registered scan is scan 1 (40 000 points; down-sampled at 0.4 unless a size is named)"""
    def __init__(self, oracle_lib):
        self.lib = oracle_lib
        extT = np.array(list(config().extT))
        self.st0 = capi.make_state(*synth.trajectory_pose(0))
        self.map_pts = np.ascontiguousarray(synth.livox_scan(0, *synth.trajectory_pose(0), n_pts=30000, extT=extT)[:, :3])
        self.raw1 = synth.livox_scan(1, *synth.trajectory_pose(1), n_pts=40000, extT=extT)
        self.down = synth.voxel_grid_downsample(self.raw1, 0.4)
        R1, t1 = synth.trajectory_pose(1)
        # the floor alone: near the ground plane and at least half a metre (a voxel) away from every box of the scene's lattice, whose walls stand on it
        world = (self.down.astype(np.float64) + extT) @ R1.T + t1
        cell = np.mod(world[:, :2], synth.LATTICE)
        off_box = ((cell < synth.BOX_LO - 0.5) | (cell > synth.BOX_HI + 0.5)).any(axis=1)
        self.floor = np.ascontiguousarray(self.down[(np.abs(world[:, 2] - synth.GROUND_Z) < 0.1) & off_box])
        self.far = (np.random.default_rng(3).uniform(-1, 1, (500, 3)) + [0, 0, 500.0]).astype(np.float32)
        self._oracles, self._inputs, self._results, self._post = {}, {}, {}, None

    def points(self, case):
        if isinstance(case.pts, tuple):
            return np.ascontiguousarray(self.raw1[:case.pts[1], :3] if case.pts[0] == "raw" else self.down[::case.pts[1]])
        return {"down": self.down, "floor": self.floor, "far": self.far}[case.pts]

    def oracle(self, max_iter):
        if max_iter not in self._oracles:
            o = capi.HotPath(self.lib, config(max_iter), prefix="orc_")
            o.map_build(self.map_pts, self.st0)
            self._oracles[max_iter] = o
        return self._oracles[max_iter]

    def converged_posterior(self):
        if self._post is None:
            s = pose_prior(0.3, 1e-4)
            self._post, _ = self.trace(4, self.down, s, s)
        return self._post

    def inputs(self, case):
        if case.name not in self._inputs:
            self._inputs[case.name] = case.make(self)
        return self._inputs[case.name]

    def trace(self, max_iter, pts, prior, state):
        f = self.lib.orc_register_trace; f.restype = C.c_int
        f.argtypes = [VP, VP, C.c_int32, VP, VP, C.c_int32] + [VP] * 12
        cap, n = max_iter, len(pts)
        out = np.array(state, dtype=np.float64, copy=True)
        HTH, HTz, sol = np.zeros((cap, 36)), np.zeros((cap, 6)), np.zeros((cap, 18))
        st, cov, nm, fl = np.zeros((cap, 24)), np.zeros((cap, 324)), np.zeros(cap, np.int32), np.zeros((cap, 2), np.int32)
        it = f(self.oracle(max_iter).ctx, _p(pts), n, _p(np.ascontiguousarray(prior)), _p(out), cap, _p(HTH), _p(HTz), _p(sol), None, _p(st), _p(cov), _p(nm),
               None, _p(fl), None, None, None)
        assert 0 < it <= cap
        return out, [dict(HTH=HTH[k], HTz=HTz[k], sol=sol[k], state=st[k], cov=cov[k], n_match=int(nm[k]), converged=int(fl[k, 0]), stop=int(fl[k, 1]))
                     for k in range(it)]

    def result(self, case):
        """the oracle's posterior and trace of a case, the checker's replay of it, and the bounds on the posterior state / covariance for a device form"""
        if case.name not in self._results:
            prior, state = self.inputs(case)
            post, tr = self.trace(case.max_iter, self.points(case), prior, state)
            rep = replay(tr, prior, state, case.max_iter)
            sum_b, sum_bc = sum(s["b"] for s in rep), sum(s["b_cov"] for s in rep)
            floor = len(tr) * FORMAT_FLOOR * EPS * max(1.0, np.abs(post[:24]).max())
            self._results[case.name] = dict(post=post, trace=tr, replay=rep, n_iter=len(tr), n_match=tr[-1]["n_match"],
                                            path=tuple((r["converged"], r["stop"]) for r in tr), matches=tuple(r["n_match"] for r in tr),
                                            sum_b=sum_b, bound_state=C_DEVICE * sum_b + floor, bound_cov=C_DEVICE * sum_bc, floor=floor)
        return self._results[case.name]


def singular_covariances():
    """the three unusable pose blocks of the input contract (include/immesh_c_api.h, immesh_register): zero, a NaN entry, one zero row and column"""
    base = np.eye(18) * 1e-4
    zero = base.copy(); zero[:6, :6] = 0
    nan = base.copy(); nan[2, 4] = nan[4, 2] = np.nan
    row = base.copy(); row[3, :] = 0; row[:, 3] = 0
    return {"zero-pose-block": zero, "nan-entry": nan, "zero-row-and-column": row}


def perturbed(state, d):
    """the pose of a 348-double state moved by d along (1, 1, 1) in translation and in rotation (first order: d is far below Exp's 1e-5 threshold)"""
    s = np.array(state, np.float64, copy=True)
    w = np.full(3, float(d))
    s[:9] = (s[:9].reshape(3, 3) @ (np.eye(3) + np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]))).reshape(-1)
    s[9:12] += w
    return s


def robust_under(sc, case, res, sign):
    """does moving the case's poses (prior and entry state alike) by sign * its bound leave the match count of every iteration and the path unchanged?"""
    prior, state = sc.inputs(case)
    d = sign * res["bound_state"]
    _, tr = sc.trace(case.max_iter, sc.points(case), perturbed(prior, d), perturbed(state, d))
    return tuple((r["converged"], r["stop"]) for r in tr) == res["path"] and tuple(r["n_match"] for r in tr) == res["matches"]


_SCENE = None


def scene(oracle_lib):
    global _SCENE
    if _SCENE is None:
        _SCENE = Scene(oracle_lib)
    return _SCENE
