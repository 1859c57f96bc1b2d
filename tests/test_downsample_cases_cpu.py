"""The clouds of tests/downsample_cases.py, shown on the CPU before the device sees them (COVERAGE.md row f1): the spec (synth.voxel_grid_downsample),
the checker (orc_downsample) and a third restatement that shares nothing with either (a dictionary from the cell triple to the scan indices, float32
scalars added one by one, the output sorted by (k, j, i)) agree bit for bit on every case; the census, the cell extremes and the largest leaf that the
route is predicted from are recomputed from the points; the order of the sum matters in every size class a case is there for; on the wall cases every
point's cell is the one the case wrote down."""
import collections

import numpy as np
import pytest

import downsample_cases as D
from immesh_amd import capi, synth
from conftest import make_oracle


@pytest.fixture(scope="module")
def orc(oracle_lib):
    return make_oracle(oracle_lib, capi.avia_config())


@pytest.mark.parametrize("fam", D.FAMILIES)
def test_spec_checker_and_dictionary_agree_and_the_cases_are_what_they_declare(orc, fam):
    for c in D.family(fam) + ([D.ordinary()] if fam == "sizes" else []):
        ref = synth.voxel_grid_downsample(c.pts, c.leaf)
        got, n = orc.downsample(c.pts, c.leaf)
        assert n == len(ref) == c.n_leaves, c
        assert got.tobytes() == ref.tobytes(), c
        third, sizes = D.restate(c.pts, c.leaf)
        assert third.tobytes() == ref.tobytes(), c
        # the census and what the route is predicted from, recomputed from the points
        cells = D.cells_of(c.pts, c.leaf)
        assert sorted(sizes) == c.sizes and sorted(collections.Counter(cells).values()) == c.sizes, c
        assert min(min(t) for t in cells) == c.cell_lo and max(max(t) for t in cells) == c.cell_hi, c
        in_range = all(-D.BIAS <= v < D.BIAS for t in cells for v in t)
        assert c.route == ("hash" if in_range and max(sizes) <= D.LEAF_CAP else "radix"), c
        # the spec's own index stays inside int64
        lo, hi = np.array(cells).min(axis=0), np.array(cells).max(axis=0)
        assert int(np.prod([int(h) - int(l) + 1 for l, h in zip(lo, hi)])) <= 1 << 63, c
        # the pinned members are where the builder put them
        by_cell = collections.Counter(cells)
        for q, size in c.pinned:
            assert by_cell[cells[q]] == size, (c, q)
        # the three-column form is the same cloud
        got3, n3 = orc.downsample(c.xyz3(), c.leaf)
        assert n3 == n and got3.tobytes() == ref.tobytes(), c


@pytest.mark.parametrize("fam", D.FAMILIES)
def test_the_order_of_the_sum_matters_in_every_size_class(fam):
    """every leaf summed in DESCENDING scan order: in each size class the case is there for at least one leaf's centroid changes -- a device that added
    a leaf's members in any other order than the scan's could not pass by luck"""
    for c in D.family(fam) + ([D.ordinary()] if fam == "sizes" else []):
        if not c.classes:
            continue
        fwd, sizes = D.restate(c.pts, c.leaf, only_sizes=set(c.classes))
        rev, _ = D.restate(c.pts, c.leaf, reverse=True, only_sizes=set(c.classes))
        changed = (fwd != rev).any(axis=1)
        for s in c.classes:
            assert changed[np.array(sizes) == s].any(), (c, s)
    if fam == "sizes":      # of the eleven leaves of `sizes` all but the leaves of one and of two points
        c = D.by_name("sizes")
        fwd, sizes = D.restate(c.pts, c.leaf)
        rev, _ = D.restate(c.pts, c.leaf, reverse=True)
        assert sorted(np.array(sizes)[(fwd != rev).any(axis=1)].tolist()) == sorted(D.ORDER_CLASSES)


def test_cells_of_the_points_on_leaf_walls():
    low = 0
    for c in D.family("walls"):
        inv = np.float32(1.0 / c.leaf)
        cells = np.floor(c.pts[:, :3] * inv).astype(np.int64)
        np.testing.assert_array_equal(cells, c.cells, err_msg=c.name)
        assert D.cells_of(c.pts, c.leaf) == [tuple(r) for r in c.cells.tolist()], c
        if c.leaf == 0.4:
            low += 1
            axis = "xyz".index(c.name[6])
            k = np.rint(c.pts[:, axis].astype(np.float64) / 0.4).astype(int)
            assert sorted(k[c.cells[:, axis] == k - 1].tolist()) == sorted(D.WALL_04_LOW) and (np.abs(c.cells[:, axis] - k) <= 1).all(), c
        else:
            # both zeros in cell 0, both negative denormals in cell -1 (kept, not flushed), the wall itself in the upper cell, one float32 below it in the lower
            axis = "xyz".index(c.name[6])
            x = c.pts[:, axis]
            assert (c.cells[x == 0, axis] == 0).all() and (x == 0).sum() == 2 and np.signbit(x[x == 0]).sum() == 1
            den = (x < 0) & (np.abs(x) < np.finfo(np.float32).tiny)
            assert den.sum() == 2 and (c.cells[den, axis] == -1).all()
    assert low == 3
