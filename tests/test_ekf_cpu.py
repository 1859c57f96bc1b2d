"""CPU tier of the 18-state iterated update (COVERAGE.md row a14): the oracle's step and the product's host step (imh::EkfLoop::step, through the
stand-alone program tests/c/ekf_host_step.cpp, built plain and with -fsanitize=address,undefined) against the long-double checker of
tests/ekf_checker.py, on every iteration of every case of the table the GPU tier (test_gpu_ekf_paths.py) runs on the three device routes.

Discrete outcomes (converged / rematch / stop, the path) are exact.  Values: |oracle - checker| <= C_ORC * b_k, the constant measured here and
written down in ekf_checker.py; the iterate additionally gets the rounding of its own format (FORMAT_FLOOR).  A case may be compared on the device
only if the oracle's outcome is robust under a perturbation of the size of its bound: asserted here for every case."""
import os
import subprocess

import numpy as np
import pytest

import ekf_checker as K
from conftest import ROOT

NAMES = [c.name for c in K.CASES]


@pytest.fixture(scope="module")
def sc(oracle_lib):
    return K.scene(oracle_lib)


def _ratio(err, b):
    return err / b if b > 0 else (0.0 if err == 0 else np.inf)


def test_checker_inverse_exp_and_log_keep_the_reference_thresholds():
    rng = np.random.default_rng(1)
    A = rng.normal(size=(18, 18)); A = A @ A.T + np.eye(18)
    assert np.abs((K._inv(A) @ A.astype(K.LD)).astype(np.float64) - np.eye(18)).max() < 1e-15
    with pytest.raises(np.linalg.LinAlgError):
        K._inv(np.zeros((6, 6)))
    assert np.array_equal(K.exp_ld([6e-6, 6e-6, 5e-6]), np.eye(3))                                  # |v| < 1e-5: the identity
    for mag in (2e-5, 9.99e-4, 1.001e-3, 0.04, 0.06, 0.5, 3.0):
        w = np.array([0.6, -0.48, 0.64], K.LD) * K.LD(mag)
        back = K.log_ld(K.exp_ld(w))
        # below 1e-3 Log is first order (0.5 K = sin(theta) axis): error theta^3 / 6; above it is exact to the format
        assert float(np.abs(back - w).max()) <= (mag ** 3 / 6 * 1.01 if mag < 1e-3 else 1e-15 * max(1, 1 / mag)), mag


def test_decision_priors_take_every_path(sc):
    """(a), from the oracle alone: a path of length 2, a forced rematch (no iteration converged up to max_iter - 2, where the count is forced), a run to
    max_iter; (b): the early stop and the cap are both seen over the max_iter values, 1 and 2 included."""
    paths = [sc.result(c)["path"] for c in K.CASES if c.family == "a"]
    assert len(paths) == 7
    assert any(len(p) == 2 for p in paths), paths
    assert any(len(p) == 4 and not any(cv for cv, _ in p[:3]) for p in paths), paths       # rematch_num went 0 -> 1 at it == 2 without convergence
    assert any(len(p) == 4 for p in paths), paths
    lens = {c.name: sc.result(c)["n_iter"] for c in K.CASES if c.family == "b"}
    for mi in (1, 2, 3, 4):
        assert lens[f"b-iter{mi}-far"] == mi                                               # the cap
    assert lens["b-iter1-conv"] == 1 and all(lens[f"b-iter{mi}-conv"] == 2 for mi in (2, 3, 4, 61, 62))   # the early stop
    assert 4 < lens["b-iter61-far"] < 61 and lens["b-iter62-far"] == lens["b-iter61-far"]  # far, yet it converges long before a cap of 61
    for p in paths:
        assert p[-1][1] == 1 and not any(st for _, st in p[:-1])


def test_forced_rematch_cannot_move_the_stop():
    """Why no registration output can tell `it == max_iter - 2` from `it == max_iter - 1` (or from no forced rematch at all) in the voxel-map routes: the
    forced count is taken one pass before the cap, and the pass after it stops at the cap whatever the count.  Every convergence sequence up to
    max_iter = 8, exhaustively.  (The count only steers the nearest-neighbour re-search of the legacy ikd path.)  So a device copy of the rule with that
    constant wrong is an equivalent mutant of these routes; the copies are held by n_iter on every path above instead."""
    def stop_pass(conv, max_iter, forced_at):
        rematch = 0
        for it in range(max_iter):
            if conv[it] or (rematch == 0 and forced_at is not None and it == max_iter - forced_at):
                rematch += 1
            if rematch >= 2 or it == max_iter - 1:
                return it
    for max_iter in range(1, 9):
        for bits in range(1 << max_iter):
            conv = [(bits >> k) & 1 for k in range(max_iter)]
            assert stop_pass(conv, max_iter, 2) == stop_pass(conv, max_iter, 1) == stop_pass(conv, max_iter, None)


def test_geometry_cases_are_what_they_claim(sc):
    r = sc.result(K.CASE_BY_NAME["e-floor-only"])
    # rank 3 up to the noise of the fitted normals: of the translations only z is measured (its eigenvector is the floor's normal), and the rotation block
    # has two strong directions (roll, pitch) and a weak one (yaw)
    H = r["trace"][0]["HTH"].reshape(6, 6)
    ev_t, vec_t = np.linalg.eigh(H[3:, 3:])
    ev_r = np.linalg.eigvalsh(H[:3, :3])
    assert r["n_match"] > 500 and ev_t[2] > 100 * ev_t[1] and abs(vec_t[2, 2]) > 0.999 and ev_r[1] > 100 * ev_r[0], (ev_t, ev_r)
    z = sc.result(K.CASE_BY_NAME["e-zero-matches"])
    assert z["matches"] == (0, 0) and np.array_equal(z["post"][:24], sc.inputs(K.CASE_BY_NAME["e-zero-matches"])[0][:24])
    dense = sc.inputs(K.CASE_BY_NAME["d-dense-propagated"])[1][24:].reshape(18, 18)
    assert np.abs(dense[6:, :6]).max() > 0.1 * np.abs(dense[:6, :6]).max()                               # T = P21 P11^-1 is far from zero
    rnd = sc.inputs(K.CASE_BY_NAME["d-random-spd-kappa1e8"])[1][24:].reshape(18, 18)
    assert 5e7 < np.linalg.cond(rnd) < 2e8
    assert abs(np.linalg.cond(sc.inputs(K.CASE_BY_NAME["d-rot1e-10-trans1e-2"])[1][24:].reshape(18, 18)[:6, :6]) - 1e8) < 1


@pytest.mark.parametrize("name", NAMES)
def test_oracle_step_equals_the_longdouble_step_on_every_iteration(sc, name):
    """every iteration through orc_register_trace, the checker fed that iteration's own HTH, HTz and entry state: decisions exact, the solution and the
    posterior covariance within C_ORC * b_k (this is the measurement of C_ORC: the ratio is printed), the iterate within that + the format floor"""
    case = K.CASE_BY_NAME[name]
    r = sc.result(case)
    assert r["trace"][-1]["stop"] == 1 and len(r["trace"]) <= case.max_iter
    worst = 0.0
    for k, (o, s) in enumerate(zip(r["trace"], r["replay"])):
        assert (o["converged"], o["stop"]) == (int(s["converged"]), int(s["stop"])), (name, k)
        e_sol = float(np.abs(np.asarray(o["sol"], K.LD) - s["sol"]).max())
        e_st = float(np.abs(np.asarray(o["state"], K.LD) - s["state"]).max())
        worst = max(worst, _ratio(e_sol, s["b"]))
        assert e_st <= K.C_ORC * s["b"] + K.FORMAT_FLOOR * K.EPS * max(1.0, np.abs(o["state"]).max()), (name, k, e_st, s["b"])
        if s["stop"]:
            worst = max(worst, _ratio(float(np.abs(np.asarray(o["cov"], K.LD).reshape(18, 18) - s["cov"]).max()), s["b_cov"]))
            assert np.array_equal(r["post"][24:], o["cov"]) and np.array_equal(r["post"][:24], o["state"])
    print(f"{name}: path {r['path']} matches {r['matches']} max |oracle - checker| / b_k = {worst:.3f}; device bounds: state {r['bound_state']:.3e} "
          f"(sum b_k {r['sum_b']:.3e}, format floor {r['floor']:.3e}), covariance {r['bound_cov']:.3e}")
    assert worst <= K.C_ORC, (name, worst)


def test_constants_follow_from_the_measurement():
    assert K.C_ORC >= max(1.0, K.C_ORC_MEASURED) and K.C_ORC - K.C_ORC_MEASURED < 1.0
    assert K.C_DEVICE == 2.0 ** np.ceil(np.log2(16 * K.C_ORC))


@pytest.mark.parametrize("name", NAMES)
def test_oracle_outcome_is_robust_under_the_case_bound(sc, name):
    """moving prior and entry pose by +- the bound a device form is held to leaves the match count of every iteration and the path unchanged: a
    device form inside its bound cannot legitimately take another path.  No case is exempt."""
    case = K.CASE_BY_NAME[name]
    r = sc.result(case)
    assert K.robust_under(sc, case, r, +1) and K.robust_under(sc, case, r, -1), (name, r["bound_state"])


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the product's host step as a stand-alone program
N_IN, N_OUT = 417, 352


@pytest.fixture(scope="module")
def host_step_programs(tmp_path_factory):
    # (the sanitizer runtimes are linked into the program: it runs whatever else the environment preloads)
    d = tmp_path_factory.mktemp("ekf_host_step")
    src, inc = os.path.join(ROOT, "tests", "c", "ekf_host_step.cpp"), os.path.join(ROOT, "immesh_amd", "csrc")
    out = {}
    for tag, flags in (("plain", ["-O2"]), ("sanitized", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"])):
        exe = str(d / f"ekf_host_step_{tag}")
        subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror"] + flags + ["-I", inc, src, "-o", exe])
        out[tag] = exe
    return d, out


def _run_program(d, exe, records, tag):
    fin, fout = str(d / f"in_{tag}.bin"), str(d / f"out_{tag}.bin")
    np.ascontiguousarray(records, np.float64).tofile(fin)
    p = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    assert p.stdout.strip() == f"{len(records)} steps"
    return np.fromfile(fout, np.float64).reshape(len(records), N_OUT)


@pytest.mark.parametrize("build", ["plain", "sanitized"])
def test_host_step_program_equals_the_checker(sc, host_step_programs, build):
    """imh::EkfLoop::step -- product code: the host loop of IMMESH_HOST_EKF, of max_iter outside [2, 62) and of the legacy ikd path -- on every iteration
    of every case, one record each (its HTH, HTz, entry state, pass index and rematch count on entry): decisions exact, iterate and posterior covariance
    within C_ORC * b_k (+ the format floor) of the long-double step.  Both builds must give the same bytes; the sanitized one must stay silent."""
    d, exes = host_step_programs
    recs, want = [], []
    for case in K.CASES:
        prior, state = sc.inputs(case)
        r = sc.result(case)
        entry, rematch = state[:24], 0
        for k, (o, s) in enumerate(zip(r["trace"], r["replay"])):
            recs.append(np.concatenate([o["HTH"], o["HTz"], prior[:24], entry, state[24:], [k, rematch, case.max_iter]]))
            want.append((case.name, k, s, state[24:]))
            entry, rematch = o["state"], s["rematch"]
    recs = np.array(recs)
    assert recs.shape[1] == N_IN and len(recs) > 150
    got = _run_program(d, exes[build], recs, build)
    for (name, k, s, P), g in zip(want, got):
        assert (int(g[24]), int(g[25]), int(g[26]), int(g[27])) == (int(s["stop"]), s["rematch"], 0, 1), (name, k)
        e_st = float(np.abs(np.asarray(g[:24], K.LD) - s["state"]).max())
        assert e_st <= K.C_ORC * s["b"] + K.FORMAT_FLOOR * K.EPS * max(1.0, np.abs(g[:24]).max()), (name, k, e_st, s["b"])
        if s["stop"]:
            e_cov = float(np.abs(np.asarray(g[28:], K.LD).reshape(18, 18) - s["cov"]).max())
            assert e_cov <= K.C_ORC * s["b_cov"], (name, k, e_cov, s["b_cov"])
        else:
            assert np.array_equal(g[28:], P), (name, k)
    if build == "sanitized":
        assert np.array_equal(got, _run_program(d, exes["plain"], recs, "plain_again"))


@pytest.mark.parametrize("build", ["plain", "sanitized"])
def test_host_step_refuses_a_singular_covariance_and_leaves_the_state(sc, host_step_programs, build):
    """the host loop checks its 18 x 18 inverses: `singular` set, stop returned, the iterate and the covariance as on entry; imh::pose_block_usable (the
    check every route makes before anything is launched) refuses each of the three, and accepts a covariance that is singular OUTSIDE the pose block --
    which the 18 x 18 inverse of the host loop then refuses"""
    d, exes = host_step_programs
    case = K.CASE_BY_NAME["a-scale0.3-cov0.0001"]
    prior, state = sc.inputs(case)
    o = sc.result(case)["trace"][0]
    covs = dict(K.singular_covariances())
    outside = np.eye(18) * 1e-4; outside[9, 9] = 0
    covs["zero-variance-outside-the-pose-block"] = outside
    recs = np.array([np.concatenate([o["HTH"], o["HTz"], prior[:24], state[:24], P.reshape(-1), [0, 0, 4]]) for P in covs.values()])
    got = _run_program(d, exes[build], recs, build + "_singular")
    for (tag, P), g in zip(covs.items(), got):
        usable = tag == "zero-variance-outside-the-pose-block"
        assert int(g[27]) == int(usable), tag
        if tag != "nan-entry":     # (a NaN has no zero pivot: the host loop relies on the entry check for it)
            assert (int(g[24]), int(g[26])) == (1, 1), tag
            assert np.array_equal(g[:24], state[:24]) and np.array_equal(g[28:], P.reshape(-1), equal_nan=True), tag
