"""The discard row and column of the manifold pass (include/immesh_topology.h, the Manifold rule; the table in raycast_host.cpp), in the manner of
test_gpu_intersect_changes.py, whose soup, fetches and changes this file reads from test_gpu_snapshot_changes.py: the pass' result goes when the
snapshot changes -- a rebuild and every apply, its own included -- and with a new analysis, whose half-edges it read; its own apply discards every other
result that read the snapshot; and a pass discards nothing but its own earlier result."""
import numpy as np
import pytest

import intersect_checker as ic
from immesh_amd import capi
from conftest import make_hip
from test_gpu_render import _small_cfg
from test_gpu_snapshot_changes import AFTER_A_CHANGE, CHANGES, FACES, FETCHES, VTX, _bytes, _produce

pytestmark = pytest.mark.gpu
NONE = "no manifold pass since the last analysis"


@pytest.fixture(scope="module")
def hp():
    h = make_hip(capi.load_hip_library(), _small_cfg())
    h.cloud_index_build(np.random.default_rng(5).uniform(0.0, 5.0, (64, 3)))            # what nearest_samples measures the samples against
    yield h
    h.close()


def _fetch(h):
    return _bytes([h.topology_manifold_vertices(), h.topology_manifold_fans(), h.topology_manifold_faces(), h.topology_manifold_new_vertices()])


def _produce_all(h):
    """every derived result of test_gpu_snapshot_changes.py and the self-intersection pass, then the manifold pass -> (their bytes, the pass' bytes)"""
    before = _produce(h)
    h.self_intersect(ic.CAP)
    before["intersect"] = _bytes([h.self_intersect_pairs(), h.self_intersect_faces()])
    st = h.topology_manifold()
    assert (st.n_corners, st.n_fans, st.n_vertices_used, st.n_new_vertices) == (168, 42, 42, 0)
    return before, _fetch(h)


ALL_FETCHES = dict(FETCHES, intersect=(lambda h: [h.self_intersect_pairs(), h.self_intersect_faces()], "no self-intersection pass"))
ALL_CHANGES = dict(CHANGES)
ALL_CHANGES["self_intersect_apply"] = (lambda h: h.self_intersect_apply(), AFTER_A_CHANGE)
ALL_CHANGES["manifold_apply"] = (lambda h: h.topology_manifold_apply(), AFTER_A_CHANGE)


@pytest.mark.parametrize("change", list(ALL_CHANGES))
def test_a_change_of_the_snapshot_or_a_new_analysis_discards_the_pass(hp, change):
    before, own = _produce_all(hp)
    call, after = ALL_CHANGES[change]
    call(hp)
    text = NONE if change == "analyse" else "no analysis"
    for fetch in (hp.topology_manifold_vertices, hp.topology_manifold_fans, hp.topology_manifold_faces, hp.topology_manifold_new_vertices,
                  hp.topology_manifold_apply):
        with pytest.raises(RuntimeError, match=r"rc=-1: .*" + text):
            fetch()
    for name, (fetch, refusal) in ALL_FETCHES.items():                                  # and the other rows hold with the pass in the caster
        gone = after.get(name, None if change == "analyse" else refusal)
        if gone is None:
            assert _bytes(fetch(hp)) == before[name], (change, name)
        else:
            with pytest.raises(RuntimeError, match=r"rc=-1: .*" + gone):
                fetch(hp)
    if change != "analyse":
        hp.topology_analyse()                                                           # and it does not come back with the next analysis
        with pytest.raises(RuntimeError, match=r"rc=-1: .*" + NONE):
            hp.topology_manifold_faces()


def test_a_pass_leaves_every_other_result_as_it_was(hp):
    before, own = _produce_all(hp)
    hp.topology_manifold()
    assert _fetch(hp) == own
    for name, (fetch, _) in ALL_FETCHES.items():
        assert _bytes(fetch(hp)) == before[name], name
    for other in (lambda h: h.topology_orient(capi.ORIENT_FEWEST), lambda h: h.topology_holes(3), lambda h: h.simplify(0.5, capi.SIMPLIFY_MEAN),
                  lambda h: h.smooth(3, 0.5, 0.5), lambda h: h.vertex_normals(), lambda h: h.self_intersect(ic.CAP), lambda h: h.topology_select(min_faces=2),
                  lambda h: h.topology_edges(capi.EDGE_BOUNDARY)):
        other(hp)
        assert _fetch(hp) == own                                                        # and no other pass discards this one's
    assert (VTX.shape, FACES.shape) == ((42, 3), (56, 3))
