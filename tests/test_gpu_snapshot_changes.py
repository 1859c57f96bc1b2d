"""What a change of the caster's snapshot discards, and what every other call leaves alone: the whole rule in one table.  A change
of the snapshot is a rebuild or the apply of an orientation, a holes pass, a simplification or a smoothing pass; a new analysis discards only what
read the old one.  Every row produces every derived result first, so a flag that one change forgets to clear shows as a fetch that still answers."""
import numpy as np
import pytest

import topology_checker as tc
from immesh_amd import capi
from conftest import make_hip
from test_gpu_render import _small_cfg

pytestmark = pytest.mark.gpu
VTX, FACES = tc.grid_sheet(6, 5, holes=[(1, 1), (3, 3)])                                # 42 vertices, 56 faces: two four-edge loops and the outline


@pytest.fixture(scope="module")
def hp():
    h = make_hip(capi.load_hip_library(), _small_cfg())
    h.cloud_index_build(np.random.default_rng(5).uniform(0.0, 5.0, (64, 3)))            # what nearest_samples measures the samples against
    yield h
    h.close()


# the derived results in the order they are produced: name -> (the fetch, the refusal after a change of the snapshot)
FETCHES = {
    "points": (lambda h: h.raycast_points(0.05), "no NEAREST cast"),
    "samples": (lambda h: h.nearest_samples(1.0), "no samples"),
    "closest": (lambda h: h.closest_stats(0.25, 8), None),                              # the last query's results stay readable, whatever changes
    "analysis": (lambda h: h.topology_faces(), "no analysis"),
    "orientation": (lambda h: h.topology_orient_faces(), "no analysis"),
    "holes": (lambda h: h.topology_holes_loops(), "no analysis"),
    "simplify": (lambda h: h.simplify_faces(), "no simplify pass"),
    "smooth": (lambda h: h.smooth_vertices(), "no smooth pass"),
}
AFTER_A_CHANGE = {name: text for name, (_, text) in FETCHES.items()}
AFTER_AN_ANALYSIS = dict.fromkeys(FETCHES, None)
AFTER_AN_ANALYSIS.update(orientation="no orientation since the last analysis", holes="no holes pass since the last analysis")


def _bytes(x):
    if isinstance(x, dict):
        return b"".join(_bytes(x[k]) for k in sorted(x))
    if isinstance(x, (tuple, list)):
        return b"".join(_bytes(v) for v in x)
    return x.tobytes() if isinstance(x, np.ndarray) else bytes(x)                       # (a ctypes record)


def _cast(h, mode=capi.RAY_NEAREST):
    rng = np.random.default_rng(11)
    org = np.concatenate([rng.uniform(0.0, 1.0, (48, 2)) * np.array([6.0, 5.0]), np.ones((48, 1))], axis=1).astype(np.float32)
    dirs = np.tile(np.array([0.0, 0.0, -1.0], np.float32), (48, 1))                     # straight down; those over a hole miss
    return h.raycast(capi.ray_frame(), dirs, org, 0.0, 10.0, mode)


def _produce(h):
    """a fresh build, then every derived result -> the bytes of every fetch"""
    h.raycast_build_triangles(VTX, FACES)
    t, _ = _cast(h)
    assert (t >= 0).sum() >= 24 and len(h.raycast_points(0.05)) == (t >= 0).sum()
    assert 200 < h.mesh_sample(20.0, 7, fetch=False) < 2000
    pts = np.random.default_rng(13).uniform(-1.0, 6.0, (5, 3)).astype(np.float32)
    assert (h.closest_points(pts, 20.0)["face"] >= 0).all()
    st = h.topology_analyse()
    assert (st.n_faces, st.n_vertices_used, st.n_boundary_loops) == (56, 42, 3)
    h.topology_orient(capi.ORIENT_FIRST)
    hs = h.topology_holes(8)
    assert (hs.n_filled, hs.n_too_long) == (2, 1)                                       # the two four-edge loops; the outline stays
    h.simplify(0.0)
    h.smooth(2)
    return {name: _bytes(fetch(h)) for name, (fetch, _) in FETCHES.items()}             # every fetch answers


CHANGES = {
    "rebuild": (lambda h: h.raycast_build_triangles(VTX, FACES), AFTER_A_CHANGE),
    "orient_apply": (lambda h: h.topology_orient_apply(), AFTER_A_CHANGE),
    "holes_apply": (lambda h: h.topology_holes_apply(), AFTER_A_CHANGE),
    "simplify_apply": (lambda h: h.simplify_apply(), AFTER_A_CHANGE),
    "smooth_apply": (lambda h: h.smooth_apply(), AFTER_A_CHANGE),
    "analyse": (lambda h: h.topology_analyse(), AFTER_AN_ANALYSIS),
}


@pytest.mark.parametrize("change", list(CHANGES))
def test_a_change_of_the_snapshot_discards_every_result_that_read_it(hp, change):
    before = _produce(hp)
    call, after = CHANGES[change]
    call(hp)
    for name, (fetch, _) in FETCHES.items():
        if after[name] is None:
            assert _bytes(fetch(hp)) == before[name], (change, name)                    # it stays (the analysis: a fresh one of the same snapshot)
        else:
            with pytest.raises(RuntimeError, match=r"rc=-1: .*" + after[name]):
                fetch(hp)


# the calls that produce or read a result and must discard no other: name -> (the call, the result that is its own)
OTHERS = {
    "orient": (lambda h: h.topology_orient(capi.ORIENT_FEWEST), "orientation"),
    "holes": (lambda h: h.topology_holes(3), "holes"),
    "simplify": (lambda h: h.simplify(0.5, capi.SIMPLIFY_MEAN), "simplify"),
    "smooth": (lambda h: h.smooth(3, 0.5, 0.5), "smooth"),
    "vertex_normals": (lambda h: h.vertex_normals(), None),
    "cast_any": (lambda h: _cast(h, capi.RAY_ANY), None),
}


@pytest.mark.parametrize("other", list(OTHERS))
def test_every_other_call_leaves_the_other_results_as_they_were(hp, other):
    before = _produce(hp)
    call, own = OTHERS[other]
    call(hp)
    for name, (fetch, _) in FETCHES.items():
        got = _bytes(fetch(hp))                                                         # its own result answers too: it is a new one
        assert name == own or got == before[name], (other, name)
