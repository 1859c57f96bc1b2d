"""The map update on the device (replay_fused_kernel / replay_list_kernel / replay_sub_kernel, reg_kernels.hip) against the CPU checker, route by route.

The cases and the route predictor are map_update_cases.py; test_map_update_cases_cpu.py shows on the checker alone that every case is what it claims.
Here each family runs on the checker and on two device contexts -- one with IMMESH_DEBUG and a trace file, one without.  After the build and after every
update: the plane tables within the project's bar (compare_plane_tables, TOL = 1e-5, every count and flag exact), the refit counters and the root-voxel
count equal, and the two device dumps bit-equal once sorted.  (n_nodes is not compared: the checker reports 0 there, it has no node pool.)

Route proof.  After a probe update the traced context's debug buffer is read back: word 7 of the fused kernel's record of touched voxel t
(64 + 8 t + 7) is cnt | n_ref << 8 | state << 16 -- the multiset over the n_touched records must be the predictor's -- and words 12 / 13 count the
list kernel's voxels that the planar batch path consumed completely and that needed the general state machine.  Voxels that replay_split_leaves or
replay_split_root cut into work items, and voxels ordered in global scratch (more than 64 points), leave the list kernel before it counts: their
number is the handed-over records minus the two counts, and it must be the predictor's too."""
import numpy as np
import pytest

import map_update_cases as mc
from conftest import make_oracle, make_hip
from parity_utils import compare_plane_tables, plane_index

pytestmark = pytest.mark.gpu
TOL = 1e-5
DBG_FUSED_OFF = 64


def _max_deviation(a, b):
    """largest deviation of any compared value, in units of its own tolerance (1.0 = the bar)"""
    ia, ib = plane_index(a), plane_index(b)
    worst = 0.0
    for k, i in ia.items():
        ra, rb = a[i], b[ib[k]]
        if not ra["is_plane"]:
            continue
        s = 1.0 if np.dot(ra["normal"], rb["normal"]) >= 0 else -1.0
        pa, pb = ra["plane_var"].reshape(6, 6), rb["plane_var"].reshape(6, 6).copy()
        pb[0:3, 3:6] *= s; pb[3:6, 0:3] *= s
        worst = max(worst, np.abs(rb["normal"] * s - ra["normal"]).max(), np.abs(rb["center"] - ra["center"]).max() / max(1.0, np.abs(ra["center"]).max()),
                    abs(rb["d"] * s - ra["d"]) / max(1.0, abs(ra["d"])), abs(float(rb["radius"]) - float(ra["radius"])), abs(float(rb["min_eig"]) - float(ra["min_eig"])),
                    np.abs(pb - pa).max() / max(np.abs(pa).max(), 1e-300))
    return worst / TOL


def _counts_equal(a, b, max_layer):
    """compare_plane_tables compares the point counts of planes and of layer-4 nodes.  Here also: nodes that stopped updating, and non-planar nodes at the
    configuration's LAST layer, whatever it is (they keep their points and refit every sixth one).  A non-planar node above the last layer is left out: the
    checker keeps a cut node's buffer until the node's next visit, the device drops it at the cut -- nothing reads it in between."""
    ia, ib = plane_index(a), plane_index(b)
    for k, i in ia.items():
        ra, rb = a[i], b[ib[k]]
        if ra["is_plane"] or ra["update_enable"] == 0 or ra["layer"] == max_layer:
            assert (ra["n_points"], ra["new_points"]) == (rb["n_points"], rb["new_points"]), f"point counts differ at {k}: {ra['n_points']},{ra['new_points']} vs {rb['n_points']},{rb['new_points']}"


def _trace(path, n_touched):
    w = np.fromfile(path, dtype=np.uint64)
    rec = w[DBG_FUSED_OFF + 8 * np.arange(n_touched) + 7].astype(np.int64)
    ms = sorted((int(r & 0xFF), int((r >> 8) & 0xFF), int(r >> 16)) for r in rec)
    return ms, {k: int(w[k]) for k in (12, 13)}


def _run_family(name, oracle_lib, hip_lib, monkeypatch, tmp_path, record_property, env_on_second=True):
    fam = mc.FAMILIES[name]()
    trace = tmp_path / "trace.bin"
    for k, v in fam.env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("IMMESH_DEBUG", "1")
    monkeypatch.setenv("IMMESH_TRACE_FILE", str(trace))
    h = make_hip(hip_lib, fam.cfg)                     # knobs are read when the context is created
    monkeypatch.delenv("IMMESH_DEBUG")
    monkeypatch.delenv("IMMESH_TRACE_FILE")
    if not env_on_second:
        for k in fam.env:
            monkeypatch.delenv(k)
    h2 = make_hip(hip_lib, fam.cfg)
    o = make_oracle(oracle_lib, fam.cfg)
    mc.tap_on(o)
    probe_scan = np.ascontiguousarray(fam.scan(0)[::3]) if fam.residual_probe else None
    worst, seen_routes = 0.0, {}
    for step in range(fam.n_steps):
        before = o.dump_planes() if step in fam.probes else None
        h.counters()                                   # (zeroes the debug buffer's counter words)
        pts = mc.run_step(o, fam, step)
        mc.run_step(h, fam, step); mc.run_step(h2, fam, step)
        a, b = o.dump_planes(), h.dump_planes()
        tag = f"{name} step {step}"
        try:
            compare_plane_tables(a, b, TOL)
            _counts_equal(a, b, int(fam.cfg.max_layer))
        except AssertionError as e:
            raise AssertionError(f"{tag}: {e}") from e
        worst = max(worst, _max_deviation(a, b))
        co, ch = o.counters(), h.counters()
        for c in ("n_refits", "n_refit_pts", "n_root_voxels"):
            assert ch[c] == co[c], f"{tag}: {c} device {ch[c]}, checker {co[c]}"
        d1, d2 = mc.sorted_dump(h), mc.sorted_dump(h2)
        assert d1.tobytes() == d2.tobytes(), f"{tag}: the traced context's dump differs from the untraced one's"
        if step in fam.probes:
            assert max(len(v.scan[step]) for v in fam.vox if step in v.scan) <= 255     # cnt and n_ref share bits above that
            keys = mc.oracle_keys(o, len(pts))
            pred = mc.predict(before, pts, keys, fam.cfg, fam.env, fam.retained(step))
            ms, fast, general, routes = mc.census(pred)
            got_ms, words = _trace(trace, len(pred))
            assert got_ms == ms, f"{tag}: (cnt, n_ref, state) records differ: device-only {_diff(got_ms, ms)}, predictor-only {_diff(ms, got_ms)}"
            assert (words[12], words[13]) == (fast, general), f"{tag}: list kernel consumed {words[12]} voxels on the planar path, {words[13]} on the general one; predicted {fast}, {general}"
            # voxels cut into work items (replay_split_leaves / replay_split_root) or ordered in global scratch leave the list kernel before it counts:
            # handed-over voxels minus the two counts is their number (nothing records them one by one)
            n_handed = sum(1 for r in got_ms if r[2] == 3)
            uncounted = sum(1 for p in pred.values() if p["state"] == 3 and p["fast"] is None)
            assert n_handed - words[12] - words[13] == uncounted, f"{tag}: {n_handed - words[12] - words[13]} handed-over voxels were split or ordered in scratch, predicted {uncounted} ({routes})"
            for p in pred.values():
                seen_routes[p["route"]] = seen_routes.get(p["route"], 0) + 1
        if probe_scan is not None and step >= 1:
            ro, rh = o.residuals(probe_scan, mc.state()), h.residuals(probe_scan, mc.state())
            np.testing.assert_array_equal(rh["match_idx"], ro["match_idx"], err_msg=tag)
            assert h.counters()["n_plane_tests"] == o.counters()["n_plane_tests"], tag
    record_property("max_deviation_in_units_of_TOL", float(worst))
    record_property("routes", seen_routes)
    print(f"[map_update_paths] {name}: max deviation {worst:.3e} x TOL, routes {seen_routes}")
    for c in (h, h2, o):
        c.close()
    return fam


def _diff(a, b):
    b = list(b)
    out = []
    for x in a:
        if x in b:
            b.remove(x)
        else:
            out.append(x)
    return out[:8]


@pytest.mark.parametrize("name", ["A", "B", "C", "C12", "D", "D-split0", "D3", "G"])
def test_every_route_against_the_checker(name, oracle_lib, hip_lib, monkeypatch, tmp_path, record_property):
    _run_family(name, oracle_lib, hip_lib, monkeypatch, tmp_path, record_property)


def test_fused_grid_of_32_workgroups_equals_the_default_grid(oracle_lib, hip_lib, monkeypatch, tmp_path, record_property):
    """200 settled roots on 128 wavefronts (IMMESH_FUSED_WGS=32, traced) against a default context (untraced): dumps bit-equal, both equal to the checker"""
    _run_family("G-wgs32", oracle_lib, hip_lib, monkeypatch, tmp_path, record_property, env_on_second=False)


def test_a_record_without_a_refit_is_bit_unchanged(hip_lib):
    """new_points + cnt = 5 and a full planar root: the device's own record of the voxel is the same bytes before and after the update (counts aside)"""
    fam = mc.family_a()
    h = make_hip(hip_lib, fam.cfg)
    for step in range(2):
        mc.run_step(h, fam, step)
    before = mc.sorted_dump(h)
    mc.run_step(h, fam, 2)
    after = mc.sorted_dump(h)
    n = 0
    for v in fam.vox:
        c = v.claims.get(2)
        if not (c and c["exact"]):
            continue
        (rb,) = [r for r in before if r["layer"] == 0 and tuple(r["key"]) == v.key]
        (ra,) = [r for r in after if r["layer"] == 0 and tuple(r["key"]) == v.key]
        for fld in ("is_plane", "update_enable", "radius", "min_eig", "d", "center", "normal", "plane_var"):
            assert np.array_equal(ra[fld], rb[fld]), (v.name, fld)
        assert ra["n_points"] == rb["n_points"] + (len(v.scan[2]) if c["state"] == 2 else 0)
        n += 1
    assert n == 2
    h.close()


@pytest.mark.parametrize("which", ["cap_point_chunks", "cap_nodes"])
def test_pool_exhaustion_is_an_error_not_a_fault(which, oracle_lib, hip_lib):
    """a 30-point batch on four new roots with a pool too small for it: map_update returns IMMESH_E_CAPACITY with a message, the process goes on, and a
    fresh, adequately sized context then matches the checker.  (Every use of alloc_chunk / node_alloc / node_ensure_chunk / make_child on the update's
    routes returns before a failed allocation's -1 could index anything.  The dump is not taken from the exhausted context: node_alloc's bump counter has run
    past the pool there, and dump_planes_kernel walks as many nodes as the counter says.)"""
    small = dict(cap_point_chunks=4) if which == "cap_point_chunks" else dict(cap_nodes=3, cap_point_chunks=4096)
    fam = mc.Family("pool", "avia", small)
    first = fam.new_vox("first")
    fam.put(first, 0, fam.geo.sheet(fam.rng, 6))
    for i in range(4):
        v = fam.new_vox(f"new{i}")
        fam.put(v, 1, fam.geo.sheet(fam.rng, 30))
    h = make_hip(hip_lib, fam.cfg)
    mc.run_step(h, fam, 0)
    with pytest.raises(RuntimeError) as ei:
        mc.run_step(h, fam, 1)
    assert f"rc={mc.capi.E_CAPACITY}" in str(ei.value)
    assert ("point-chunk pool" if which == "cap_point_chunks" else "node pool") in str(ei.value)
    h.close()
    cfg = mc.make_config("avia", {})
    o, g = make_oracle(oracle_lib, cfg), make_hip(hip_lib, cfg)
    for step in range(2):
        for c in (o, g):
            (c.map_build if step == 0 else c.map_update)(fam.scan(step), mc.state())
    assert compare_plane_tables(o.dump_planes(), g.dump_planes(), TOL) == 5
    g.close(); o.close()
