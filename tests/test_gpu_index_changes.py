"""What a change of a cloud index's cloud discards, and what every other call leaves alone: the whole rule in one table.  A change
of the cloud is a build or the apply of a mask; new normals discard only the agreement that read the old ones.  Every row rebuilds the index and
produces every derived result first, so a flag that one change forgets to clear shows as a fetch that still answers, and a buffer that one call
borrows from another record shows as a fetch whose bytes differ."""
import ctypes as C

import numpy as np
import pytest

import topology_checker as tc
from immesh_amd import capi
from conftest import make_hip
from test_gpu_render import _small_cfg

pytestmark = pytest.mark.gpu
VTX, FACES = tc.grid_sheet(6, 5)                                                        # 42 vertices, 60 faces at z = 0


def _cloud():
    """a jittered 20 x 15 sheet over the mesh, six strays well above it, two points that are not finite"""
    rng = np.random.default_rng(3)
    i, j = np.meshgrid(np.arange(20), np.arange(15), indexing="ij")
    sheet = np.stack([0.3 * i.ravel() + 0.15, 0.33 * j.ravel() + 0.15, np.zeros(300)], axis=-1) + rng.uniform(-0.05, 0.05, (300, 3))
    strays = rng.uniform(0.0, 5.0, (6, 3)) + np.array([0.0, 0.0, 3.0])
    cloud = np.concatenate([sheet, strays, [[np.nan, 1.0, 0.0], [2.0, np.inf, 0.0]]]).astype(np.float32)
    return cloud[rng.permutation(len(cloud))]


CLOUD = _cloud()
PTS = np.random.default_rng(17).uniform(-1.0, 6.0, (9, 3)).astype(np.float32)           # the queries of the point-mode calls


@pytest.fixture(scope="module")
def hp():
    h, other = make_hip(capi.load_hip_library(), _small_cfg()), make_hip(capi.load_hip_library(), _small_cfg())
    h.raycast_build_triangles(VTX, FACES)
    other.raycast_build_triangles(VTX, FACES)                                           # the caster of another context, with samples of its own
    other.mesh_sample(20.0, 7, fetch=False)
    h.other = other
    yield h
    h.close()
    other.close()


# the derived results in the order they are produced: name -> (the fetch, the refusal after a change of the cloud).  The Neighbours and the Count
# query are read through the rule that reads them: its answer is a function of their buffers alone.  The last mask has no fetch: the apply reads it.
FETCHES = {
    "nearest": (lambda h: h.nearest_stats(0.25, 8), "no nearest-point query"),
    "knn": (lambda h: h.cloud_outliers_statistical(1.0), "no immesh_knn_cloud query since"),
    "count": (lambda h: h.cloud_outliers_radius(3), "no immesh_radius_count_cloud query since"),
    "normals": (lambda h: h.cloud_normals_get(), "no normals since"),
    "agreement": (lambda h: h.normals_agree_stats(0.25, 8), "no agreement since"),
    "clusters": (lambda h: h.cloud_clusters_table(), "no immesh_cloud_clusters call since"),
}


def _bytes(x):
    if isinstance(x, dict):
        return b"".join(_bytes(x[k]) for k in sorted(x))
    if isinstance(x, (tuple, list)):
        return b"".join(_bytes(v) for v in x)
    if isinstance(x, (int, float)):
        return np.float64(x).tobytes()
    return x.tobytes() if isinstance(x, np.ndarray) else bytes(x)                       # (a ctypes record)


def _refused(text, call, *args, rc=-1):
    with pytest.raises(RuntimeError, match=rf"rc={rc}: .*" + text):
        call(*args)


def _produce(h):
    """fresh samples and a fresh build, then every derived result; the last mask is the statistical rule's with mult = 0.5 -> the indices it keeps"""
    assert 200 < h.mesh_sample(20.0, 7, fetch=False) < 2000
    assert h.cloud_index_build(CLOUD) == (308, 306)
    assert (h.nearest_samples(1.0)["index"] >= 0).all()
    assert (h.knn_cloud(8, 1.0, want=("count",))["count"] > 0).sum() >= 300
    assert (h.radius_count_cloud(0.6) >= 3).sum() >= 250
    n = h.cloud_normals(8, 1.0, want=())
    assert n["with_normal"] >= 250 and n["not_finite"] == 2
    assert h.normals_agree_samples(fetch=False)["pairs"] > 100
    assert h.normals_agree_cloud(1.0, fetch=False)["pairs"] >= 250                      # the agreement that stays: the cloud direction's
    assert h.cloud_clusters(0.6, 3, want=())["n_clusters"] >= 1
    m = h.cloud_outliers_statistical(0.5)
    assert 0 < m["outliers"] and m["kept"] + m["outliers"] + m["isolated"] + m["not_finite"] == 308
    return np.flatnonzero(m["keep"]).astype(np.int32)


def _leaves(h, call, own=(), gone=(), then=None):
    """call(h) behind _produce leaves every fetch byte for byte but those in `own`, which answer anew, and those in `gone`, which refuse; and it
    leaves the last mask: the apply keeps what the mask kept.  The fetches of the two outlier rules make masks of their own and the apply is a change,
    hence a second _produce."""
    _produce(h)
    before = {name: _bytes(fetch(h)) for name, (fetch, _) in FETCHES.items()}           # every fetch answers
    call(h)
    if then is not None:
        then(h)
    for name, (fetch, _) in FETCHES.items():
        if name in gone:
            _refused(gone[name], fetch, h)
        else:
            got = _bytes(fetch(h))                                                      # its own result answers too: it is a new one
            assert name in own or got == before[name], name
    mask = _produce(h)
    call(h)
    if "mask" not in own:
        assert np.array_equal(h.cloud_index_apply_outliers(), mask)


CHANGES = {
    "build": lambda h, mask: h.cloud_index_build(CLOUD) == (308, 306),
    "apply": lambda h, mask: np.array_equal(h.cloud_index_apply_outliers(), mask),
}


@pytest.mark.parametrize("change", list(CHANGES))
def test_a_change_of_the_cloud_discards_every_result_made_on_it(hp, change):
    mask = _produce(hp)
    for fetch, _ in list(FETCHES.values())[::-1]:                                       # every fetch answers; the last mask is the statistical rule's again
        fetch(hp)
    assert CHANGES[change](hp, np.flatnonzero(hp.cloud_outliers_statistical(0.5)["keep"]))
    for fetch, text in FETCHES.values():
        _refused(text, fetch, hp)
    _refused("no outlier mask since", hp.cloud_index_apply_outliers)                    # the mask went too: no second apply
    _refused("no normals since", hp.normals_agree_cloud, 1.0)
    assert len(hp.cloud_index_points()) == (308 if change == "build" else len(mask))


def test_new_normals_discard_the_agreement_alone(hp):
    _leaves(hp, lambda h: h.cloud_normals(8, 1.0, want=()), gone={"agreement": "no agreement since"})      # the same normals again: their bytes stay too


def _samples_agreement_refuses(h):
    _refused("no immesh_nearest_samples query of this caster", h.normals_agree_samples, False)


# the calls that produce or read a result and must discard no other: name -> (the call, the results that are its own, what else holds afterwards)
OTHERS = {
    "knn_points": (lambda h: h.knn_points(PTS, 4, 2.0), (), None),
    "radius_count_points": (lambda h: h.radius_count_points(PTS, 0.9), (), None),
    "nearest_points": (lambda h: h.nearest_points(PTS, 2.0), ("nearest",), _samples_agreement_refuses),    # the stored agreement's stats stay
    "cloud_clusters": (lambda h: h.cloud_clusters(0.9, 2, want=()), ("clusters",), None),                  # its counts are not the Count query's
    "cloud_clusters_select": (lambda h: h.cloud_clusters_select(min_points=5), ("mask",), None),
    "mesh_sample": (lambda h: h.mesh_sample(20.0, 8, fetch=False), (), _samples_agreement_refuses),
}


@pytest.mark.parametrize("other", list(OTHERS))
def test_every_other_call_leaves_the_other_results_as_they_were(hp, other):
    call, own, then = OTHERS[other]
    _leaves(hp, call, own, then=then)


def test_the_apply_behind_a_select_uses_the_selects_mask(hp):
    mask = _produce(hp)
    keep = np.flatnonzero(hp.cloud_clusters_select(min_points=5)["keep"])
    assert 0 < len(keep) < 306 and not np.array_equal(keep, mask)                       # the strays, as noise, and the two others go
    assert np.array_equal(hp.cloud_index_apply_outliers(), keep)                        # its mask, not the statistical rule's


def _raw(h, name, *args):
    f = getattr(h.lib, name)
    f.restype = C.c_int
    f.argtypes = [C.c_void_p] + [C.c_double if isinstance(a, float) else C.c_int64 if isinstance(a, int) else C.c_void_p for a in args]
    h._check(f(h.cloud_index(), *args), name)


def _bad_radius(h):
    for r in (0.0, -1.0, float("inf"), float("nan")):
        _refused("need 0 < radius, finite", h.radius_count_cloud, r)
        _refused("need 0 < radius, finite", h.radius_count_points, PTS, r)
        _refused("need 0 < radius, finite", h.cloud_clusters, r, 3)
        _refused("need 0 < max_dist, finite", h.knn_cloud, 8, r)
        _refused("need 0 < max_dist, finite", h.nearest_samples, r)
        _refused("need 0 < max_dist, finite", h.cloud_normals, 8, r)
        _refused("need 0 < max_dist, finite", h.normals_agree_cloud, r)


def _k_zero(h):
    _refused("need 1 <= k <= 64, got 0", h.knn_cloud, 0, 1.0)
    _refused("need 1 <= k <= 64, got 0", h.knn_points, PTS, 0, 1.0)
    _refused("need 2 <= k <= 64, got 0", h.cloud_normals, 0, 1.0)


def _cap_too_small(h):
    out, n = np.zeros((308, 3), np.float32).ctypes.data_as(C.c_void_p), C.c_int64(0)
    _refused("cap 1 < ", _raw, h, "immesh_cloud_index_apply_outliers", out, 1, C.byref(n), rc=-4)
    _refused("cap 307 < 308 points", _raw, h, "immesh_cloud_normals_get", out, None, 307, None, rc=-4)
    _refused("cap 0 < ", _raw, h, "immesh_cloud_clusters_table", out, None, None, None, 0, None, rc=-4)
    _refused("cap is negative", _raw, h, "immesh_cloud_index_points", out, -1, None)


def _another_context(h):
    r = h.other.raycaster()
    _refused("different contexts", _raw, h, "immesh_nearest_samples", r, 1.0, None, None, None, None)
    _refused("different contexts", _raw, h, "immesh_normals_agree_samples", r, None, None)
    _refused("different contexts", _raw, h, "immesh_normals_agree_cloud", r, 1.0, None, None, None)


REFUSED = {"bad_radius": _bad_radius, "k_zero": _k_zero, "cap_too_small": _cap_too_small, "another_context": _another_context}


@pytest.mark.parametrize("refused", list(REFUSED))
def test_a_refused_call_leaves_the_index_as_it_was(hp, refused):
    _leaves(hp, REFUSED[refused])
