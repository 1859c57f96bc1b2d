"""CPU tier of the map-update route suite: every case of map_update_cases.py is run on the checker (oracle/, pinned to the reference's compiled octree by
test_ref_voxelmap.py) and shown to be what it claims -- its preconditions in the checker's table, its eigenvalue margins, the key tie, its predicted
route -- and the predictor's verdict for the voxels the fused kernel finishes is held against what the checker then does."""
import numpy as np
import pytest

import map_update_cases as mc
from conftest import make_oracle

TOL = 1e-5


def _record(table, key):
    for r in table:
        if r["layer"] == 0 and tuple(int(k) for k in r["key"]) == key:
            return r
    return None


@pytest.fixture(scope="module")
def runs(oracle_lib):
    """family name -> per probe step: (table before, scan, checker's keys, prediction, table after); computed once, never changed"""
    cache = {}

    def get(name):
        if name not in cache:
            fam = mc.FAMILIES[name]()
            o = make_oracle(oracle_lib, fam.cfg)
            mc.tap_on(o)
            steps = {}
            for step in range(fam.n_steps):
                before = o.dump_planes() if step in fam.probes else None
                pts = mc.run_step(o, fam, step)
                if step in fam.probes:
                    keys = mc.oracle_keys(o, len(pts))
                    pred = mc.predict(before, pts, keys, fam.cfg, fam.env, fam.retained(step))
                    steps[step] = (before, pts, keys, pred, o.dump_planes())
            cache[name] = (fam, steps)
        return cache[name]
    return get


@pytest.mark.parametrize("name", list(mc.FAMILIES))
def test_cases_are_what_they_claim(runs, name):
    fam, steps = runs(name)
    n_claims = 0
    for v in fam.vox:
        for step, c in v.claims.items():
            before, pts, keys, pred, after = steps[step]
            rec, pre, p = _record(before, v.key), c["pre"], pred[v.key]
            tag = f"{name}/{v.name} step {step}"
            if pre.get("absent"):
                assert rec is None, tag
            else:
                assert rec is not None, tag
                for field, want in pre.items():
                    assert int(rec[field]) == want, f"{tag}: {field} = {int(rec[field])}, the case needs {want}"
            assert p["cnt"] == len(v.scan[step]), tag
            assert p["route"] == c["route"] and p["state"] == c["state"], f"{tag}: predicted {p['route']} / state {p['state']}"
            if c["n_ref"] is not None:
                assert p["n_ref"] == c["n_ref"], tag
            n_claims += 1
    assert n_claims > 0


@pytest.mark.parametrize("name", list(mc.FAMILIES))
def test_numpy_replay_order_is_the_checkers(runs, name):
    """the builder orders a batch by its own restatement of the key; the checker's keys must give the same order in every voxel (ties aside)"""
    fam, steps = runs(name)
    for step, (before, pts, keys, pred, after) in steps.items():
        rk = [tuple(k) for k in mc.root_keys(pts, fam.cfg.voxel_size)]
        byk = fam.by_key()
        assert set(rk) == {v.key for v in fam.vox if step in v.scan and len(v.scan[step])}     # every point fell into its own voxel
        for key in set(rk):
            idx = np.array([i for i, k in enumerate(rk) if k == key])
            got = np.asarray(pts)[idx[np.lexsort((idx, keys[idx]))]]
            np.testing.assert_array_equal(got, byk[key].replay[step], err_msg=f"{name}/{byk[key].name} step {step}")


@pytest.mark.parametrize("name", list(mc.FAMILIES))
def test_margins(runs, name):
    """no predicted verdict rests on rounding: every eigenvalue the predictor evaluated is 5 % away from the threshold, and where the diagonal bound
    must NOT decide an intermediate refit, the smallest per-axis variance is 5 % above it"""
    fam, steps = runs(name)
    byk = fam.by_key()
    n = 0
    for step, (before, pts, keys, pred, after) in steps.items():
        for key, p in pred.items():
            for lam in p["eigs"]:
                assert abs(lam / mc.THR - 1.0) >= mc.MARGIN, f"{name}/{byk[key].name} step {step}: lambda_min / threshold = {lam / mc.THR}"
                n += 1
            if byk[key].zy and step in byk[key].claims:
                assert len(p["axis_vars"]) >= 2
                for av in p["axis_vars"]:
                    assert av > (1 + mc.MARGIN) * mc.THR, f"{name}/{byk[key].name}: per-axis variance {av}"
            elif byk[key].name == "slab" and step in byk[key].claims:
                assert p["axis_vars"] and all(av < (1 - mc.MARGIN) * mc.THR for av in p["axis_vars"])
    assert n > 0 or name.startswith("D")     # (the deep-octree families' planar roots: one at most -- their verdicts are the children's, checked below)


@pytest.mark.parametrize("name", list(mc.FAMILIES))
def test_predictor_against_the_checker(runs, name):
    """states 1 and 2: the flags and counts the predictor derives are the checker's after the update; state 1 and unrefitted records are unchanged"""
    fam, steps = runs(name)
    n = 0
    for step, (before, pts, keys, pred, after) in steps.items():
        for key, p in pred.items():
            if p["state"] == 3:
                continue
            r = _record(after, key)
            got = (int(r["is_plane"]), int(r["update_enable"]), int(r["n_points"]), int(r["new_points"]))
            assert got == p["final"], f"{name} {key} step {step}: checker {got}, predictor {p['final']}"
            if p["state"] == 1 or p["n_ref"] == 0:
                b = _record(before, key)
                for fld in ("center", "normal", "d", "radius", "min_eig", "plane_var"):
                    assert np.array_equal(b[fld], r[fld])
            n += 1
    assert n > 0 or name.startswith("D")     # (the deep-octree families hand every voxel over: nothing for this test there)


def _node(table, key, layer, path):
    for r in table:
        if r["layer"] == layer and r["path"] == path and tuple(int(k) for k in r["key"]) == key:
            return r
    return None


@pytest.mark.parametrize("name", list(mc.FAMILIES))
def test_descendants_are_what_the_cases_claim(runs, name):
    """the destination kinds below a subdivided root: each claimed child's record in the checker's table before and after the probe update (None = not
    in the table: missing, or still filling up)"""
    fam, steps = runs(name)
    for v in fam.vox:
        for step, claims in v.children.items():
            before, _, _, _, after = steps[step]
            for layer, path, want_b, want_a in claims:
                for table, want, when in ((before, want_b, "before"), (after, want_a, "after")):
                    r = _node(table, v.key, layer, path)
                    tag = f"{name}/{v.name} step {step} layer {layer} path {path} {when}"
                    if want is None:
                        assert r is None, tag
                    else:
                        assert r is not None, tag
                        for field, val in want.items():
                            assert int(r[field]) == val, f"{tag}: {field} = {int(r[field])}, the case needs {val}"


@pytest.mark.parametrize("name", list(mc.FAMILIES))
def test_no_fit_of_the_checker_sits_next_to_the_threshold(runs, name):
    """child fits are the checker's, not the predictor's: every plane in every table after a probe update has lambda_min 5 % below the threshold (the
    fits that must NOT be planar are asserted by the builder on the exact point sets: assert_non_planar)"""
    fam, steps = runs(name)
    for step, s in steps.items():
        pl = s[4][s[4]["is_plane"] == 1]
        assert len(pl) and float(pl["min_eig"].max()) < (1 - mc.MARGIN) * mc.THR, (name, step, float(pl["min_eig"].max()) / mc.THR)


def test_census_covers_every_route_and_boundary(runs):
    have = set()
    for name in mc.FAMILIES:
        fam, steps = runs(name)
        for v in fam.vox:
            for step, c in v.claims.items():
                p = steps[step][3][v.key]
                have.add((name, p["route"], c["boundary"]))
    missing = [r for r in mc.REQUIRED if r not in have]
    assert not missing, missing
    routes = {r for _, r, _ in have}
    assert routes >= {"dropped", "fused", "planar_root", "planar_node", "general", "leaves", "octants"}
    big = sum(1 for name in mc.FAMILIES for step, s in runs(name)[1].items() for p in s[3].values() if p["big"])
    assert big >= 6


def test_the_key_tie_is_a_tie_and_shows(oracle_lib):
    """two different points with bit-equal keys in the checker; swapping them in scan order moves the checker's plane of that voxel by > 100 x TOL"""
    fam = mc.family_a()
    v = [v for v in fam.vox if v.tie][0]
    step, i, j = v.tie
    tables = []
    for swap in (False, True):
        o = make_oracle(oracle_lib, fam.cfg)
        mc.tap_on(o)
        for s in range(step):
            mc.run_step(o, fam, s)
        pts = fam.scan(step).copy()
        where = [int(np.flatnonzero((pts == q).all(axis=1))[0]) for q in (v.scan[step][i], v.scan[step][j])]
        assert not np.array_equal(pts[where[0]], pts[where[1]])
        if swap:
            pts[where] = pts[where[::-1]]
        o.map_update(pts, mc.state())
        keys = mc.oracle_keys(o, len(pts))
        assert keys[where[0]] == keys[where[1]], "not a tie in the checker"
        tables.append(_record(o.dump_planes(), v.key))
    a, b = tables
    assert a["is_plane"] == 1 and b["is_plane"] == 1 and a["n_points"] == 13
    moved = np.abs(a["center"] - b["center"]).max() / max(1.0, np.abs(a["center"]).max())
    assert moved > 100 * TOL, moved


def test_every_point_keeps_clear_of_faces_and_octant_planes():
    for name, make in mc.FAMILIES.items():
        fam = make()
        byk = fam.by_key()
        for step in range(fam.n_steps):
            pts = fam.scan(step).astype(np.float64)
            if not len(pts):
                continue
            r = np.mod(pts, fam.geo.grid)
            d = np.minimum(r, fam.geo.grid - r)
            zy = np.array([byk[tuple(k)].zy for k in mc.root_keys(pts, fam.cfg.voxel_size)])
            assert d[:, :2].min() >= 0.01 and d[~zy, 2].min() >= 0.01, (name, step, d.min(axis=0))
            # the z = y slab lies in planar roots only (nothing compares its z with an octant plane); it still keeps clear of the root's faces
            rz = np.mod(pts[zy, 2], fam.geo.vs)
            assert not zy.any() or min(rz.min(), (fam.geo.vs - rz).min()) >= 0.01
