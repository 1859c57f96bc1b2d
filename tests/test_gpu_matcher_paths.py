"""The plane matcher of the registration passes (COVERAGE.md rows a10 - a12: residual_pass, match_tree, match_trees_coop, plane_gates, test_plane in
reg_kernels.hip) path by path, on the cases of tests/matcher_cases.py -- every one of whose claims test_matcher_cases_cpu.py shows on the checker first.

Every scan goes through immesh_residuals on two contexts: the default one (match_trees_coop: the wavefront's (point, leaf) pairs 64 at a time) and
IMMESH_MATCH_SEQ (match_tree: the lane-by-lane walk).  Against the checker: match_idx identical, n_plane_tests and n_extra_probe equal, dis bit-equal, normals
within 1e-5, r_inv rtol 1e-6, HTH / HTz rtol 1e-7 (the bars of test_residuals_parity); the two contexts byte-equal; a second call byte-equal.  The scans'
own claims (tests, probes, matches per scan) are asserted of the device too; they come from the builder, none from the device.

The two matchers give equal results by design, so no comparison of outputs shows which one ran: that the IMMESH_MATCH_SEQ context runs match_tree is what
mutation 1 of profiles/matcher_paths_mutants.log shows (a change of match_tree's tie rule alone fails this file)."""
import os

import numpy as np
import pytest

import matcher_cases as M
from conftest import make_hip, make_oracle
from parity_utils import compare_plane_tables

pytestmark = pytest.mark.gpu

TOL = 1e-5
KNOBS = ("IMMESH_MATCH_SEQ", "IMMESH_RP_FORCE_ABORT")


def _make_ctx(hip_lib, cfg, **env):
    assert not any(k in os.environ for k in KNOBS)
    os.environ.update(env)
    try:
        return make_hip(hip_lib, cfg)
    finally:
        for k in env:
            del os.environ[k]


class Three:
    """one family's map on the checker, the default context and the IMMESH_MATCH_SEQ context; `with Three(...) as t:` closes all three"""
    def __init__(self, oracle_lib, hip_lib, fam):
        self.fam, self.open = fam, []
        try:
            self.o = self._keep(make_oracle(oracle_lib, fam.cfg))
            self.coop = self._keep(_make_ctx(hip_lib, fam.cfg))
            self.seq = self._keep(_make_ctx(hip_lib, fam.cfg, IMMESH_MATCH_SEQ="1"))
            for h in self.open:
                M.build_map(h, fam)
            self.table = self.o.dump_planes()
            for h in (self.coop, self.seq):
                compare_plane_tables(self.table, h.dump_planes(), TOL)
        except BaseException:
            self.close()
            raise

    def _keep(self, h):
        self.open.append(h)
        return h

    def close(self):
        for h in self.open:
            h.close()
        self.open = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def check(self, name, pts, cov, claims=None, same_sign=False):
        ro = M.run_scan(self.o, self.fam, pts, cov)
        a = M.run_scan(self.coop, self.fam, pts, cov)
        a2 = M.run_scan(self.coop, self.fam, pts, cov)
        b = M.run_scan(self.seq, self.fam, pts, cov)
        print(f"{name}: {len(pts)} points, matches {ro['n_match']} / {a['n_match']} / {b['n_match']} (checker / coop / seq), tests {ro['n_plane_tests']} / "
              f"{a['n_plane_tests']} / {b['n_plane_tests']}, probes {ro['n_extra_probe']} / {a['n_extra_probe']} / {b['n_extra_probe']}")
        if claims is not None:
            assert (ro["n_plane_tests"], ro["n_extra_probe"], ro["match_idx"].tolist()) == claims, name
        for tag, rh in (("coop", a), ("seq", b)):
            np.testing.assert_array_equal(rh["match_idx"], ro["match_idx"], err_msg=f"{name} [{tag}]")
            assert (rh["n_plane_tests"], rh["n_extra_probe"]) == (ro["n_plane_tests"], ro["n_extra_probe"]), (name, tag)
            sg = np.ones(len(ro["dis"])) if same_sign else np.sign(np.sum(rh["normals"] * ro["normals"], axis=1))
            np.testing.assert_allclose(rh["normals"] * sg[:, None], ro["normals"], rtol=0, atol=TOL, err_msg=f"{name} [{tag}]")
            np.testing.assert_array_equal(rh["dis"] * sg.astype(np.float32), ro["dis"], err_msg=f"{name} [{tag}] dis")        # bit-equal (row a12)
            np.testing.assert_allclose(rh["r_inv"], ro["r_inv"], rtol=1e-6, err_msg=f"{name} [{tag}]")
            np.testing.assert_allclose(rh["HTH"], ro["HTH"], rtol=1e-7, atol=1e-7 * np.abs(ro["HTH"]).max(), err_msg=f"{name} [{tag}]")
            np.testing.assert_allclose(rh["HTz"], ro["HTz"], rtol=1e-7, atol=1e-7 * np.abs(ro["HTz"]).max(), err_msg=f"{name} [{tag}]")
        for k in ("match_idx", "normals", "dis", "r_inv", "HTH", "HTz"):
            assert a[k].tobytes() == a2[k].tobytes(), (name, k, "a second call gave other bytes")
            assert a[k].tobytes() == b[k].tobytes(), (name, k, "IMMESH_MATCH_SEQ gave other bytes")
        return ro, a

    def check_scan(self, s, same_sign=False):
        return self.check(s.name, s.points(), s.cov, (sum(s.tests), sum(s.extra), [i for i, m in enumerate(s.match) if m]), same_sign)


@pytest.mark.parametrize("order", ["forward", "reverse"])
def test_list_shapes_wave_compositions_and_pair_counts(oracle_lib, hip_lib, order):
    """leaf lists of 0, 1, 2, 3, 14, 15, 16, 30, 31, 46 leaves and one with an emptied slot; n = 1, 63, 64, 65; one tree lane among planar lanes, 64 on 64
    roots, 64 on one root, lanes without a voxel between tree lanes, unequal lists; steps of 1, 63, 64, 65 and 960 pairs -- in both insertion orders"""
    fam = M.generic_family(order)
    with Three(oracle_lib, hip_lib, fam) as t:
        for s in M.generic_scans(fam) + [c[1] for c in M.register_cases(fam)[:2]]:
            t.check_scan(s)


@pytest.mark.parametrize("order", ["small-first", "small-last"])
def test_exact_ties_go_to_the_smaller_depth_first_key(oracle_lib, hip_lib, order):
    """two and three partners; in one batch of 64 pairs, in different batches of one step, in different lines (steps); the partner with the smaller key
    inserted first and inserted last; a tie behind the sigma gate.  The winner shows in the sign of dis (+-1 / 64), which is compared bit for bit."""
    fam = M.tie_family(order)
    with Three(oracle_lib, hip_lib, fam) as t:
        for h in (t.coop, t.seq):           # zero-variance map on the device before any tie is asserted
            tab = h.dump_planes()
            pl = tab[tab["is_plane"] == 1]
            assert len(pl) == sum(r.n_leaves() if r.kind == "tree" else 1 for r in fam.roots) and (pl["plane_var"] == 0).all()
            assert (pl["normal"] == np.array([0.0, 0.0, 1.0])).all()
            eq = pl[(pl["key"] == np.array(fam.by_name["range-eq"].key)).all(axis=1) & (pl["path"] == 0)]
            assert len(eq) == 1 and eq[0]["radius"] == np.float32(0.125)       # the radius the range gate is met with exactly
        for s in M.tie_scans(fam):
            ro, a = t.check_scan(s, same_sign=True)
            for j, i in enumerate(ro["match_idx"]):
                root, c = fam.by_name[s.winner[i][0]], s.winner[i][1]
                assert a["dis"][j] == np.float32(s.points()[i][2] - root.plane_z(c, True)), (s.name, i)      # the builder's arithmetic: the claimed cell's plane
        for s in M.gate_equality_scans(fam):       # dis == 3 sigma is rejected, range == 3 radius accepted: on a leaf (both walks) and on a planar root
            t.check_scan(s, same_sign=True)


def test_the_tie_at_half_a_metre(oracle_lib, hip_lib):
    for reverse in (False, True):
        sm = M.Small(True, reverse)
        with Three(oracle_lib, hip_lib, sm) as t:
            for h in (t.coop, t.seq):
                assert (h.dump_planes()["plane_var"] == 0).all()
            ro, a = t.check("small", sm.queries(), M.QUERY_COV, (32, 0, [0, 1, 2, 3]), same_sign=True)
            assert (a["dis"] == np.float32(1.0 / 64)).all()
    sh = M.Small(False, False)
    with Three(oracle_lib, hip_lib, sh) as t:
        ro, a = t.check("small-shipped", sh.queries(), M.QUERY_COV, (32, 0, [0, 1, 2, 3]))
        assert np.sign(ro["dis"]).tolist() == [1, 1, 1, -1]          # (the device's equal the checker's: check) -- the tie above is real and decides


def test_max_layer_zero_and_the_retry_round(oracle_lib, hip_lib):
    """max_layer = 0; the own root accepting nothing with the neighbour absent, a planar root (accepting, rejecting), a tree (a cooperative call with some
    lanes of two wavefronts in it), the own root again; float32 positions either side of centre +- quarter on each axis; the own root accepting"""
    for fam in (M.Flat(), M.Retry()):
        with Three(oracle_lib, hip_lib, fam) as t:
            t.check_scan(fam.scan())


def _one_flip(pts, dec):
    return len(dec) >= 1000 and dec[0] and not dec[-1] and int((dec[1:] != dec[:-1]).sum()) == 1


def test_gate_sweeps_and_points_above_a_centre_on_planar_roots(oracle_lib, hip_lib):
    """test_plane's gates (planar roots, both contexts): 1024 consecutive float32 positions across the range gate and across the sigma gate (located on the
    checker), and 81 points on the normal through a plane's centre, where dis_to_center - dis_to_plane^2 rounds to either sign"""
    g = M.Gates()
    with Three(oracle_lib, hip_lib, g) as t:
        for name, (pts, dec) in M.gate_sweeps(t.o, g).items():
            assert _one_flip(pts, dec), name
            t.check(name, pts, 1e-6)
        pts = M.centre_line(t.o, g)
        ro, a = t.check("above-centre", pts, 1e-6)
        assert 0 < ro["n_match"] < len(pts)


def test_gate_sweeps_and_points_above_a_centre_on_a_leaf(oracle_lib, hip_lib):
    """the leaf paths' own gates (match_trees_coop's copies and match_tree's leaf loop): the same sweeps and the same line on a generic leaf of a tree root
    under the shipped error model, every swept lane between matched lanes of the 30-leaf root, whose full front line puts 15 pairs between any two swept pairs
    of a step: a swept pair is evaluated by a lane other than its owner's (matcher_cases.swept_pair_lanes, asserted in the CPU tier; lane 63 alone coincides)"""
    fam = M.generic_family("forward")
    with Three(oracle_lib, hip_lib, fam) as t:
        for name, (pts, dec) in M.leaf_gate_sweeps(t.o, fam).items():
            assert _one_flip(pts[1::2], dec), name
            t.check(name, pts, M.LEAF_COV)
        pts = M.leaf_centre_line(t.o, fam)
        ro, a = t.check("leaf-above-centre", pts, M.LEAF_COV)
        assert len(pts) // 2 < ro["n_match"] < len(pts)          # the lanes in between match; of the 81 some do, some have a NaN range


ROUTES = {"resident": {}, "chain": {"IMMESH_RP_FORCE_ABORT": "1"}, "resident-seq": {"IMMESH_MATCH_SEQ": "1"},
          "chain-seq": {"IMMESH_RP_FORCE_ABORT": "1", "IMMESH_MATCH_SEQ": "1"}}


@pytest.mark.parametrize("route", list(ROUTES))
def test_register_on_the_resident_grid_and_on_the_chain(oracle_lib, hip_lib, route):
    """immesh_register on more than 256 points -- wavefronts 0 - 3 of a resident workgroup and a second workgroup -- with either matcher: the all-matched
    composition; the one with an empty list, the emptied slot, lanes without a voxel, lists of 1 / 2 / 3 and unequal lists; the retry round with every kind
    of neighbour (the tree neighbour: a second cooperative call with some lanes of every wavefront); max_layer = 0.  n_iter, n_match, the counters of
    plane tests and probes over all passes, and the last pass's matches equal the checker's."""
    made = {}
    try:
        for fam, s, prior in M.register_cases(M.generic_family("forward")):
            if fam not in made:
                made[fam] = (make_oracle(oracle_lib, fam.cfg), _make_ctx(hip_lib, fam.cfg, **ROUTES[route]))
                for x in made[fam]:
                    M.build_map(x, fam)
            o, h = made[fam]
            fb = h.registration_fallbacks()
            o.counters(reset=True); h.counters(reset=True)
            so, io = o.register(s.points(), prior, prior)
            sh, ih = h.register(s.points(), prior, prior)
            co, ch = o.counters(), h.counters()
            fb = h.registration_fallbacks() - fb
            print(f"{s.name} [{route}]: {len(s.pts)} points, n_iter {ih['n_iter']} (checker {io['n_iter']}) n_match {ih['n_match']} (checker {io['n_match']}) "
                  f"tests {ch['n_plane_tests']} ({co['n_plane_tests']}) probes {ch['n_extra_probe']} ({co['n_extra_probe']}) fallbacks {fb}")
            assert fb == (1 if route.startswith("chain") else 0), s.name
            assert (ih["n_iter"], ih["n_match"]) == (io["n_iter"], io["n_match"]), s.name
            assert (ch["n_plane_tests"], ch["n_extra_probe"]) == (co["n_plane_tests"], co["n_extra_probe"]), s.name
            if s.name != "register":
                assert io["n_match"] < len(s.pts) and co["n_extra_probe"] > 0, s.name          # unmatched and retried lanes occur
            np.testing.assert_allclose(sh[:24], so[:24], rtol=0, atol=1e-5, err_msg=s.name)
            po, qo = o.last_matches()
            ph, qh = h.last_matches()
            np.testing.assert_array_equal(ph, po, err_msg=s.name)
            sg = np.sign(np.sum(qh[:, :3] * qo[:, :3], axis=1))
            np.testing.assert_allclose(qh[:, :3] * sg[:, None], qo[:, :3], rtol=0, atol=1e-5, err_msg=s.name)
            np.testing.assert_allclose(qh[:, 3] * sg, qo[:, 3], rtol=0, atol=1e-5, err_msg=s.name)
    finally:
        for o, h in made.values():
            o.close(); h.close()
