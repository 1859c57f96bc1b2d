"""The discard rows of the self-intersection pass (include/immesh_intersect.h; the table in raycast_host.cpp), in the manner of
test_gpu_snapshot_changes.py, whose soup, fetches and changes this file reads: the pass' result goes when the snapshot changes -- a rebuild and every
apply, the orientation's included, and its own -- and a new analysis leaves it; its own apply discards every other result that read the snapshot; and
a pass discards nothing but its own earlier result."""
import numpy as np
import pytest

import intersect_checker as ic
from immesh_amd import capi
from conftest import make_hip
from test_gpu_render import _small_cfg
from test_gpu_snapshot_changes import AFTER_A_CHANGE, CHANGES, FACES, FETCHES, VTX, _bytes, _produce

pytestmark = pytest.mark.gpu
NONE = "no self-intersection pass"


@pytest.fixture(scope="module")
def hp():
    h = make_hip(capi.load_hip_library(), _small_cfg())
    h.cloud_index_build(np.random.default_rng(5).uniform(0.0, 5.0, (64, 3)))            # what nearest_samples measures the samples against
    yield h
    h.close()


def _fetch(h):
    return _bytes([h.self_intersect_pairs(), h.self_intersect_faces()])


def _produce_all(h):
    """every derived result of test_gpu_snapshot_changes.py, then the pass -> (their bytes, the pass' bytes)"""
    before = _produce(h)
    st = h.self_intersect(ic.CAP)
    assert (st.n_faces, st.n_taking_part, st.n_pairs) == (56, 56, 0) and st.n_candidates > 56
    return before, _fetch(h)


@pytest.mark.parametrize("change", list(CHANGES) + ["self_intersect_apply"])
def test_a_change_of_the_snapshot_discards_the_pass_and_an_analysis_leaves_it(hp, change):
    before, own = _produce_all(hp)
    call, after = CHANGES[change] if change in CHANGES else (lambda h: h.self_intersect_apply(), AFTER_A_CHANGE)
    call(hp)
    if change == "analyse":
        assert _fetch(hp) == own
    else:
        for fetch in (hp.self_intersect_pairs, hp.self_intersect_faces, hp.self_intersect_apply):
            with pytest.raises(RuntimeError, match=r"rc=-1: .*" + NONE):
                fetch()
    for name, (fetch, _) in FETCHES.items():                                            # and the other rows hold with the pass in the caster
        if after[name] is None:
            assert _bytes(fetch(hp)) == before[name], (change, name)
        else:
            with pytest.raises(RuntimeError, match=r"rc=-1: .*" + after[name]):
                fetch(hp)


def test_a_pass_leaves_every_other_result_as_it_was(hp):
    before, own = _produce_all(hp)
    hp.self_intersect(ic.CAP)
    assert _fetch(hp) == own
    for name, (fetch, _) in FETCHES.items():
        assert _bytes(fetch(hp)) == before[name], name
    for other in (lambda h: h.topology_orient(capi.ORIENT_FEWEST), lambda h: h.topology_holes(3), lambda h: h.simplify(0.5, capi.SIMPLIFY_MEAN),
                  lambda h: h.smooth(3, 0.5, 0.5), lambda h: h.vertex_normals()):
        other(hp)
        assert _fetch(hp) == own                                                        # and no other pass discards this one's
    assert (VTX.shape, FACES.shape) == ((42, 3), (56, 3))
