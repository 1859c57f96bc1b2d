"""The alignment (include/immesh_align.h) beside the caster's other results, in the manner of test_gpu_snapshot_changes.py, whose soup and fetches
this file reads: an alignment is a question about points -- it owns its buffers, discards nothing and leaves the last closest query, the NEAREST cast's
points, the samples, the analysis and every pass' result byte for byte as they were -- and after a rebuild it answers for the new snapshot."""
import numpy as np
import pytest

import align_checker as ac
from immesh_amd import capi
from conftest import make_hip
from test_gpu_render import _small_cfg
from test_gpu_snapshot_changes import FACES, FETCHES, VTX, _bytes, _produce

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hp():
    h = make_hip(capi.load_hip_library(), _small_cfg())
    h.cloud_index_build(np.random.default_rng(5).uniform(0.0, 5.0, (64, 3)))            # what nearest_samples measures the samples against
    yield h
    h.close()


def _cloud(n=700):
    rng = np.random.default_rng(17)
    return np.concatenate([rng.uniform(0.0, 1.0, (n, 2)) * [6.0, 5.0], rng.uniform(-0.05, 0.05, (n, 1))], axis=1).astype(np.float32)


@pytest.mark.parametrize("mode", [capi.ALIGN_POINT, capi.ALIGN_PLANE])
def test_an_alignment_leaves_every_other_result_as_it_was(hp, mode):
    before = _produce(hp)                                     # a closest query, a NEAREST cast, a sampling, an analysis, ..., a smoothing pass
    pts = _cloud()
    opts = capi.align_options(mode=mode, max_dist=1.0, damping=1e-6, max_iters=3)
    for variant in (0, 1, 2):
        hp.align_set_variant(variant)
        sy, face, terms = hp.align_step(pts, opts, capi.ray_frame(pos=[0.0, 0.0, 0.02]), want_face=True, want_terms=True)
        assert sy.n_used > 300 and (face >= 0).sum() == sy.n_used + sy.n_flat
        res, hist = hp.align(pts, opts)
        assert res.iterations == len(hist) >= 1
        for name, (fetch, _) in FETCHES.items():
            assert _bytes(fetch(hp)) == before[name], (variant, name)
    hp.align_set_variant(0)
    assert (VTX.shape, FACES.shape) == ((42, 3), (56, 3))


def test_after_a_rebuild_the_alignment_answers_for_the_new_snapshot(hp):
    pts = _cloud(300)
    opts = capi.align_options(mode=capi.ALIGN_POINT, max_dist=3.0)
    hp.raycast_build_triangles(VTX, FACES)
    first = hp.align_step(pts, opts, None, True, True)
    other_vtx = (VTX.astype(np.float64) * [1.0, 1.0, 0.0] + [0.25, -0.5, 1.0]).astype(np.float32)      # the sheet moved up and aside
    other_faces = FACES[::-1][:40]
    for vtx, faces in ((other_vtx, other_faces), (VTX, FACES)):
        hp.raycast_build_triangles(vtx, faces)
        ref = ac.step(None, None, pts, ac.POINT, 3.0, np.zeros(3), vtx, faces)
        sy, face, terms = hp.align_step(pts, opts, None, True, True)
        assert np.array_equal(face, ref["face"]) and terms.tobytes() == ref["terms"].tobytes() and sy.counts() == ref["counts"]
        res, _ = hp.align(pts, capi.align_options(mode=capi.ALIGN_POINT, max_dist=3.0, max_iters=1))
        assert bytes(res.system) == bytes(sy)                                            # the loop's first step is that step (no frame: the identity)
    assert bytes(sy) == bytes(first[0]) and terms.tobytes() == first[2].tobytes()
    assert terms.tobytes() != ac.step(None, None, pts, ac.POINT, 3.0, np.zeros(3), other_vtx, other_faces)["terms"].tobytes()
