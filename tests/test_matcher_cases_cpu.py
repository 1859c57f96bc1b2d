"""Every claim of tests/matcher_cases.py shown on the CPU checker (oracle/orc_voxelmap.hpp build_residual_list / build_single_residual) before
test_gpu_matcher_paths.py compares the device with it, and -- where oracle/_ref/libref_voxelmap.so is built -- on the reference's own BuildResidualListOMP /
build_single_residual (rv_residual_list): list lengths = planar descendants in the plane table = n_plane_tests of a one-point query; winners; retries; exact
ties (plane_var all zero, the partners' probabilities recomputed from the table equal as doubles, the checker picks the smallest depth-first key, the same
clouds under the shipped error model pick another plane); gate sweeps with exactly one change of the decision."""
import ctypes as C
import os

import numpy as np
import pytest

import matcher_cases as M
from immesh_amd import capi
from conftest import make_oracle, ROOT


def _tap_on(oracle_lib, o):
    oracle_lib.orc_debug_tap.argtypes = [C.c_void_p, C.c_int32]
    oracle_lib.orc_debug_tap(o.ctx, 1)


def _tap(oracle_lib, o, which):
    f = oracle_lib.orc_debug_pv; f.restype = C.c_int64; f.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
    n = f(o.ctx, which, None, None, None, 0)
    p, pw, var = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 9))
    f(o.ctx, which, p.ctypes.data_as(C.c_void_p), pw.ctypes.data_as(C.c_void_p), var.ctypes.data_as(C.c_void_p), n)
    return p, pw, var


def _leaf_record(table, root, c):
    """the plane-table record of cell c of a tree root (layer 2, path = o1 | o2 << 3), or of a planar root (c is None)"""
    t = M.planes_of_root(table, root.key)
    t = t[t["layer"] == 0] if c is None else t[(t["layer"] == 2) & (t["path"] == ((c >> 3) | ((c & 7) << 3)))]
    assert len(t) == 1, (root.name, c, len(t))
    return t[0]


def check_scan(o, fam, table, s, per_point=True):
    """the scan's totals, and every point alone: tests, probe, match, winner (the normal and d of the result are the claimed leaf's)"""
    if per_point:
        for i, p in enumerate(s.points()):
            q = M.run_scan(o, fam, p[None, :], s.cov)
            assert (q["n_plane_tests"], q["n_extra_probe"], q["n_match"]) == (s.tests[i], s.extra[i], int(s.match[i])), (s.name, i, p)
    r = M.run_scan(o, fam, s.points(), s.cov)           # (last: the checker's tap then holds the whole scan)
    assert r["n_plane_tests"] == sum(s.tests), (s.name, r["n_plane_tests"], sum(s.tests))
    assert r["n_extra_probe"] == sum(s.extra), (s.name, r["n_extra_probe"], sum(s.extra))
    assert r["match_idx"].tolist() == [i for i, m in enumerate(s.match) if m], s.name
    pts = s.points()
    for j, i in enumerate(r["match_idx"]):
        if s.winner[i] is None:
            continue
        rec = _leaf_record(table, fam.by_name[s.winner[i][0]], s.winner[i][1])
        assert np.array_equal(r["normals"][j], rec["normal"]), (s.name, i, s.winner[i])
        p, nf = pts[i].astype(np.float64), rec["normal"].astype(np.float32).astype(np.float64)
        want = np.float32(p[0] * nf[0] + p[1] * nf[1] + p[2] * nf[2] + float(rec["d"]))     # the residual as written: float normal, identity pose
        assert r["dis"][j] == want, (s.name, i, r["dis"][j], want)
    return r


# ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["forward", "reverse"])
def test_list_shapes_wave_compositions_and_pair_counts(oracle_lib, order):
    fam = M.generic_family(order)
    o = make_oracle(oracle_lib, fam.cfg)
    H = fam.by_name["H"]
    seen = {}
    def each(s):
        if s in (H.spoil[1] - 1, H.spoil[1]):
            seen[s] = M.planes_of_root(o.dump_planes(), H.key)
    M.build_map(o, fam, each=each)
    # the emptied slot: the leaf of cell seq[7] is in the table before update 46 and gone after it, nothing else of the root changed
    before, after = seen[H.spoil[1] - 1], seen[H.spoil[1]]
    gone = (H.spoil[0] >> 3) | ((H.spoil[0] & 7) << 3)
    assert len(before) == 15 and len(after) == 14 and gone in before["path"] and gone not in after["path"]
    assert set(after["path"].tolist()) == set(before["path"].tolist()) - {gone} and H.lines()[0][7] is None and H.line_counts() == [14]
    table = o.dump_planes()
    for r in fam.roots:
        pl = M.planes_of_root(table, r.key)
        if r.kind == "planar":
            assert len(pl) == 1 and pl[0]["layer"] == 0
        else:
            assert len(pl) == r.n_leaves() and (pl["layer"] == 2).all(), (r.name, len(pl))
            assert sum(r.line_counts()) == r.n_leaves()
    assert {fam.by_name[f"T{n}"].n_leaves() for n in M.LIST_LENGTHS} == {1, 2, 3, 14, 15, 16, 30, 31, 46}
    assert fam.by_name["T16"].line_counts() == [1, 15] and fam.by_name["T31"].line_counts() == [1, 15, 15] and fam.by_name["T46"].line_counts() == [1, 15, 15, 15]
    scans = M.generic_scans(fam)
    names = {s.name: s for s in scans}
    for name, pairs in M.PAIR_CLAIMS.items():
        assert names[name].step_pairs() == pairs, (name, names[name].step_pairs())
    assert names["unequal"].step_pairs()[0] > names["unequal"].step_pairs()[-1] > 0           # lanes drop out step by step
    for s in scans + [c[1] for c in M.register_cases(fam)[:2]]:
        check_scan(o, fam, table, s)
    mixed = M.register_cases(fam)[1][1]
    assert 0 in mixed.tests and 1 in mixed.extra and False in mixed.match and {1, 2, 3, 14, 46} <= set(mixed.tests)


@pytest.mark.parametrize("order", ["small-first", "small-last"])
def test_exact_ties(oracle_lib, order):
    fam = M.tie_family(order)
    o = make_oracle(oracle_lib, fam.cfg)
    _tap_on(oracle_lib, o)
    M.build_map(o, fam)
    table = o.dump_planes()
    planes = table[table["is_plane"] == 1]
    assert len(planes) == sum(r.n_leaves() if r.kind == "tree" else 1 for r in fam.roots)
    assert (planes["plane_var"] == 0).all() and (planes["normal"] == np.array([0.0, 0.0, 1.0])).all()
    for name in ("pair-adjacent", "pair-ends", "pair-lines", "pair-lines46", "three-a-lines", "E0"):
        r = fam.by_name[name]
        pos = {c: (li, line.index(c)) for li, line in enumerate(r.lines()) for c in line if c in (0, 2, 4, 6)}
        if name == "pair-adjacent":
            assert pos[0][0] == pos[4][0] and abs(pos[0][1] - pos[4][1]) == 1
        elif name in ("pair-ends", "E0"):
            assert {pos[0], pos[4]} == {(0, 0), (0, 14)}
        else:
            assert pos[0][0] != pos[4][0]                      # different lines: different enumeration steps
        if pos[0][0] == pos[4][0]:
            assert (pos[0][1] < pos[4][1]) == (order == "small-first")                  # one line: slots in insertion order
        else:
            assert (pos[0][0] > pos[4][0]) == (order == "small-first")                  # the line of the first insertions is the back of the chain
    assert M.batch_split_lanes()[:3] == [4, 8, 12] and len(M.batch_split_lanes()) == 14
    n_ties = 0
    for s in M.tie_scans(fam):
        r = check_scan(o, fam, table, s, per_point=len(s.pts) <= 4)
        _, pw, var = _tap(oracle_lib, o, 2)
        assert len(pw) == len(s.pts)
        for i in range(len(s.pts)):
            if not s.partners[i]:
                continue
            root = fam.by_name[s.winner[i][0]]
            pl = M.planes_of_root(table, root.key)
            prob = np.zeros(len(pl))
            for k, rec in enumerate(pl):      # build_single_residual in its written order, on the table's records
                n, c = rec["normal"], rec["center"]
                dp = np.float32(abs(n[0] * pw[i][0] + n[1] * pw[i][1] + n[2] * pw[i][2] + float(rec["d"])))
                dc = np.float32((c[0] - pw[i][0]) ** 2 + (c[1] - pw[i][1]) ** 2 + (c[2] - pw[i][2]) ** 2)
                with np.errstate(invalid="ignore"):
                    rd = np.sqrt(np.float32(dc - dp * dp))
                if not rd <= np.float32(3.0) * rec["radius"]:
                    continue
                J = np.array([pw[i][0] - c[0], pw[i][1] - c[1], pw[i][2] - c[2], -n[0], -n[1], -n[2]])
                pv = rec["plane_var"].reshape(6, 6)
                sig = 0.0
                for cc in range(6):
                    t = 0.0
                    for rr in range(6):
                        t += J[rr] * pv[rr, cc]
                    sig += t * J[cc]
                V = var[i].reshape(3, 3)
                vn = [V[0, a] * n[0] + V[1, a] * n[1] + V[2, a] * n[2] for a in range(3)]
                sig += vn[0] * n[0] + vn[1] * n[1] + vn[2] * n[2]
                if float(dp) < fam.cfg.sigma_num * np.sqrt(sig):
                    prob[k] = 1.0 / np.sqrt(sig) * np.exp(-0.5 * float(dp) * float(dp) / sig)
            if not s.match[i]:
                assert (prob == 0).all()      # every partner fails the sigma gate
                continue
            top = np.flatnonzero(prob == prob.max())
            cells = sorted(int(((p & 7) << 3) | (p >> 3)) for p in pl["path"][top])
            assert cells == sorted(s.partners[i]) and prob.max() > 0, (s.name, i, cells, s.partners[i])
            keys = [M.dfs_key(p, 2) for p in pl["path"][top]]
            win = pl[top[int(np.argmin(keys))]]
            assert ((win["path"] & 7) << 3 | (win["path"] >> 3)) == s.winner[i][1] == min(s.partners[i])
            j = r["match_idx"].tolist().index(i)
            assert r["dis"][j] == np.float32(pw[i][2] + float(win["d"])) and abs(r["dis"][j]) == 1.0 / 64
            n_ties += 1
    assert n_ties > 150
    # the gates met exactly: the radius that makes range_dis == 3 radius is exact in the table, and each point alone decides as claimed
    rec = _leaf_record(table, fam.by_name["range-eq"], 0)
    assert rec["radius"] == np.float32(0.125) and np.array_equal(rec["center"][:2], fam.by_name["range-eq"].cell_centre(0)[:2])
    for s in M.gate_equality_scans(fam):
        check_scan(o, fam, table, s)
    # the same clouds under the shipped error model: plane_var is not zero, and another plane wins at least one of the queries
    ship = M.tie_family(order, shipped=True)
    os_ = make_oracle(oracle_lib, ship.cfg)
    M.build_map(os_, ship)
    assert (os_.dump_planes()["plane_var"] != 0).any()
    flipped = 0
    for s, s2 in zip(M.tie_scans(fam), M.tie_scans(ship)):
        if s.cov != M.QUERY_COV:
            continue
        a, b = M.run_scan(o, fam, s.points(), s.cov), M.run_scan(os_, ship, s2.points(), s2.cov)
        assert np.array_equal(a["match_idx"], b["match_idx"])
        flipped += int((np.sign(a["dis"]) != np.sign(b["dis"])).sum())
    assert flipped >= 1


@pytest.mark.parametrize("reverse", [False, True])
def test_the_tie_at_half_a_metre(oracle_lib, reverse):
    """avia.yaml's voxel: one root, eight leaves at layer 1, the point 1 / 64 from four of them: the leaf with path 0 wins (dis = +1 / 64) for either
    order of the build cloud; under the shipped error model x = 10.3 goes to octant 4 (dis = -1 / 64)."""
    sm = M.Small(True, reverse)
    o = make_oracle(oracle_lib, sm.cfg)
    o.map_build(sm.build, sm.map_state())
    t = o.dump_planes()
    assert len(t) == 9 and (t["is_plane"] == (t["layer"] == 1)).all() and (t["plane_var"] == 0).all()
    q = sm.build.astype(np.float64)
    assert np.linalg.eigvalsh(np.cov(q.T, bias=True))[0] > 0.0125                    # the root's own fit (0.0147): well above planer_threshold
    for p in sm.queries():
        r = M.run_scan(o, sm, p[None, :])
        assert r["n_plane_tests"] == 8 and r["n_extra_probe"] == 0 and r["n_match"] == 1 and r["dis"][0] == np.float32(1.0 / 64)
    sh = M.Small(False, reverse)
    o2 = make_oracle(oracle_lib, sh.cfg)
    o2.map_build(sh.build, sh.map_state())
    r = M.run_scan(o2, sh, sh.queries())
    assert r["dis"].tolist() == [1.0 / 64, 1.0 / 64, 1.0 / 64, -1.0 / 64]


def test_max_layer_zero_and_the_retry_round(oracle_lib):
    for fam, s in ((M.Flat(), M.Flat().scan()), (M.Retry(), M.Retry().scan()), (M.Flat(), M.Flat().scan(n=280)), (M.Retry(), M.Retry().scan(reps=22, step=0.002))):
        o = make_oracle(oracle_lib, fam.cfg)
        o.map_build(fam.build, fam.map_state())
        r = M.run_scan(o, fam, s.points(), s.cov)
        assert r["n_plane_tests"] == sum(s.tests) and r["n_extra_probe"] == sum(s.extra)
        assert r["match_idx"].tolist() == [i for i, m in enumerate(s.match) if m]
        for i, p in enumerate(s.points()):
            q = M.run_scan(o, fam, p[None, :], s.cov)
            assert (q["n_plane_tests"], q["n_extra_probe"], q["n_match"]) == (s.tests[i], s.extra[i], int(s.match[i])), (s.name, i, p)
    s = M.Retry().scan()
    assert {(t, m) for t, m, e in zip(s.tests, s.match, s.extra) if e} == {(1, False), (2, False), (2, True), (9, True)}   # absent / rejecting / planar / tree


def test_gate_sweeps_change_the_decision_exactly_once(oracle_lib):
    g = M.Gates()
    o = make_oracle(oracle_lib, g.cfg)
    o.map_build(g.build, g.map_state())
    for name, (pts, dec) in M.gate_sweeps(o, g).items():
        assert len(pts) >= 1000 and dec[0] and not dec[-1], name
        assert int((dec[1:] != dec[:-1]).sum()) == 1, name            # accepted up to the gate, rejected beyond it
    pts = M.centre_line(o, g)
    r = M.run_scan(o, g, pts, 1e-6)
    print("above the centre:", r["n_match"], "of", len(pts), "accepted (a rejected one has dis_to_center - dis_to_plane^2 < 0: the range is NaN)")
    assert r["n_plane_tests"] == len(pts) and 0 < r["n_match"] < len(pts)       # both roundings occur
    # the same on a leaf of a tree root (the leaf paths have gates of their own), the swept lanes between matched lanes of another root
    fam = M.generic_family("forward")
    o = make_oracle(oracle_lib, fam.cfg)
    M.build_map(o, fam)
    for name, (pts, dec) in M.leaf_gate_sweeps(o, fam).items():
        assert len(dec) >= 1000 and dec[0] and not dec[-1] and int((dec[1:] != dec[:-1]).sum()) == 1, name
    pts = M.leaf_centre_line(o, fam)
    r = M.run_scan(o, fam, pts, M.LEAF_COV)
    print("above a leaf's centre:", r["n_match"] - 81, "of 81 accepted")
    assert r["n_plane_tests"] == 81 * 30 + 81 and 81 < r["n_match"] < 162
    # who evaluates a swept pair: from the lists' lines and the prefix sums of step 0, a lane other than its owner's (lane 63 alone coincides)
    lanes = M.swept_pair_lanes(fam)
    assert len(lanes) == 32 and [(l, e) for l, e in lanes if l == e] == [(63, 63)] and lanes[0] == (1, 15) and lanes[1] == (3, 31)
    tail = M.swept_pair_lanes(fam, 34)                            # the centre line's last, partial wavefront of 34 lanes
    assert all(l != e for l, e in tail) and tail[-1] == (33, 15)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the reference's own matcher
# ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rv():
    so = os.path.join(ROOT, "oracle", "_ref", "libref_voxelmap.so")
    if not os.path.exists(so):
        pytest.skip("oracle/_ref/libref_voxelmap.so not built")
    lib = C.CDLL(so)
    lib.rv_create.restype = C.c_void_p; lib.rv_create.argtypes = [C.c_double, C.c_int, C.c_void_p, C.c_int, C.c_double]
    lib.rv_destroy.argtypes = [C.c_void_p]
    lib.rv_build.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    lib.rv_update.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    lib.rv_residual_list.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_double] + [C.c_void_p] * 6
    return lib


def _ref_map(rv, oracle_lib, fam):
    """the family's map in the checker and in the reference's own octree (fed the checker's point lists, as test_ref_voxelmap.py does)"""
    o = make_oracle(oracle_lib, fam.cfg)
    _tap_on(oracle_lib, o)
    li = (C.c_int * 5)(*list(fam.cfg.layer_init))
    m = rv.rv_create(fam.cfg.voxel_size, fam.cfg.max_layer, li, fam.cfg.max_points_size, fam.cfg.planer_threshold)
    o.map_build(fam.build, fam.map_state())
    p, _, var = _tap(oracle_lib, o, 0)
    rv.rv_build(m, p.ctypes.data_as(C.c_void_p), var.ctypes.data_as(C.c_void_p), len(p))
    for u in getattr(fam, "updates", []):
        if len(u):
            o.map_update(u, fam.map_state())
            p, _, var = _tap(oracle_lib, o, 1)
            rv.rv_update(m, p.ctypes.data_as(C.c_void_p), var.ctypes.data_as(C.c_void_p), len(p), 1)
    return o, m


def _ref_scan(rv, oracle_lib, o, m, fam, pts, cov):
    r = M.run_scan(o, fam, pts, cov)
    _, pw, var = _tap(oracle_lib, o, 2)
    n = len(pw)
    idx, nrm, cen, d, lay = np.zeros(n, np.int32), np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n), np.zeros(n, np.int32)
    k = rv.rv_residual_list(m, pw.ctypes.data_as(C.c_void_p), var.ctypes.data_as(C.c_void_p), n, fam.cfg.voxel_size, fam.cfg.sigma_num, idx.ctypes.data_as(C.c_void_p),
                            nrm.ctypes.data_as(C.c_void_p), cen.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p), lay.ctypes.data_as(C.c_void_p), None)
    assert k == r["n_match"] and np.array_equal(idx[:k], r["match_idx"])
    return r, nrm[:k], cen[:k], d[:k], lay[:k]


@pytest.mark.parametrize("order", ["small-first", "small-last"])
def test_the_reference_recursion_breaks_the_ties_the_same_way(oracle_lib, rv, order):
    fam = M.tie_family(order)
    o, m = _ref_map(rv, oracle_lib, fam)
    n = 0
    for s in M.tie_scans(fam):
        r, nrm, cen, d, lay = _ref_scan(rv, oracle_lib, o, m, fam, s.points(), s.cov)
        for j, i in enumerate(r["match_idx"]):
            root, c = fam.by_name[s.winner[i][0]], s.winner[i][1]
            assert d[j] == -root.plane_z(c, True) and np.array_equal(cen[j][:2], root.cell_centre(c)[:2]) and lay[j] == 2, (s.name, i)   # the plane of the claimed cell
            assert r["dis"][j] == np.float32(s.points()[i][2] + d[j])
            n += 1
    assert n > 200
    rv.rv_destroy(m)
    for reverse in (False, True):
        sm = M.Small(True, reverse)
        o, m = _ref_map(rv, oracle_lib, sm)
        r, nrm, cen, d, lay = _ref_scan(rv, oracle_lib, o, m, sm, sm.queries(), M.QUERY_COV)
        assert len(d) == 4 and (d == -0.125).all() and (cen[:, :2] == np.array([10.125, 10.125])).all() and (lay == 1).all()      # octant 0
        rv.rv_destroy(m)


def test_the_reference_matcher_on_the_list_shapes(oracle_lib, rv):
    fam = M.generic_family("forward")
    o, m = _ref_map(rv, oracle_lib, fam)
    for s in M.generic_scans(fam):
        r, nrm, cen, d, lay = _ref_scan(rv, oracle_lib, o, m, fam, s.points(), s.cov)
        np.testing.assert_allclose(nrm, r["normals"], rtol=0, atol=1e-9)
    rv.rv_destroy(m)
    for fam in (M.Flat(), M.Retry()):
        o, m = _ref_map(rv, oracle_lib, fam)
        s = fam.scan()
        r, nrm, cen, d, lay = _ref_scan(rv, oracle_lib, o, m, fam, s.points(), s.cov)
        np.testing.assert_allclose(nrm, r["normals"], rtol=0, atol=1e-9)
        rv.rv_destroy(m)
