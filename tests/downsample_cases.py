"""The clouds of the VoxelGrid's path tests (COVERAGE.md row f1): tests/test_downsample_cases_cpu.py shows every claim made here on the spec and the
checker, tests/test_gpu_downsample_paths.py runs the clouds through the device.

A cloud is built from NAMED LEAVES: `c` points strictly inside one cell (i, j, k) of the grid.  Inside a cell the offsets span three decades, so a
float32 sum of more than two members depends on the order of the terms; the rows are shuffled, so a leaf's members lie scattered over the scan
indices, and where a case is about particular scan indices (0, n - 1, a bitmap word) members are pinned there after the shuffle.

Every case DECLARES, from how it was built and from nothing computed of its points:
  sizes      the multiset of leaf sizes (sorted list); the leaf count is its length
  cell_lo/hi the smallest / largest cell index over the three axes
  route      "hash" (the five-launch form is accepted) iff every cell lies in [-2^20, 2^20) on every axis and no leaf has more than 2048 points;
             "radix" otherwise (the hashed form gives up, the radix pipeline takes over)
  classes    the leaf sizes the case is there for: the order of the sum must matter in at least one leaf of each
  cells      (walls only) the cell of every point, in scan order, written down by the builder

Sizes the device code switches on (ds_kernels.hip): 64 | 65 points (short / long leaf), 2048 | 2049 (DSH_LEAF_CAP), 131 072 | 131 073 scan points
(DSH_BITMAP_PTS: bitmap / sorting network), 768 long leaves (DSH_BIG_BLOCKS), 512 leaves per sort chunk, 131 072 leaves and points per sweep of the fixed
grids, 64 sorted points per tile of ds_centroid_kernel, 262 144 points per sweep of ds_minmax_kernel."""
import functools

import numpy as np

BIAS = 1 << 20          # DSH_BIAS: cells -BIAS .. BIAS - 1 fit the packed key
LEAF_CAP = 2048         # DSH_LEAF_CAP
# float32(k) * float32(0.4), times float32(2.5), falls below k for these k of -50 .. 50 (the multiple lies in cell k - 1): written down here, shown in the CPU tier
WALL_04_LOW = (-47, -42, -31, -26, -21, -13)


class Case:
    def __init__(self, name, pts, leaf, sizes, cell_lo, cell_hi, classes=(), cells=None, pinned=()):
        self.name, self.leaf = name, leaf
        self.pts = np.ascontiguousarray(pts, np.float32)
        self.pts.setflags(write=False)
        self.sizes = sorted(sizes)
        self.n_leaves = len(self.sizes)
        self.cell_lo, self.cell_hi = int(cell_lo), int(cell_hi)
        self.route = "hash" if (self.cell_lo >= -BIAS and self.cell_hi < BIAS and self.sizes[-1] <= LEAF_CAP) else "radix"
        self.classes = tuple(classes)
        self.cells = cells
        self.pinned = tuple(pinned)      # (scan index, leaf size) pairs the builder placed

    @property
    def n(self):
        return len(self.pts)

    def xyz3(self):
        """the cloud as an n x 3 array (stride 3)"""
        return np.ascontiguousarray(self.pts[:, :3])

    def __repr__(self):
        return f"Case({self.name}: n={self.n}, leaves={self.n_leaves}, {self.route})"


class Builder:
    """leaves by cell; `build` shuffles, pins and returns the Case"""
    def __init__(self, leaf, seed):
        assert leaf in (0.5, 1.0)          # inv = 2 or 1: p * inv is exact, so `strictly inside` is decided here and not by rounding
        self.leaf, self.rng = leaf, np.random.default_rng(seed)
        self.blocks, self.sizes, self.cells, self.used, self.pins = [], [], [], set(), []
        self.lo, self.hi = None, None

    def _draw(self, cells, c):
        """m x c x 3 float32: c points strictly inside each cell"""
        m = len(cells)
        # offsets over three decades (0.001 .. 0.9 of the cell): sums of them round differently in another order.  Far out (per axis) a float32 has a few
        # fractional bits left: eighths of a cell are exact up to 2^21 cells of half a metre
        u = np.where((np.abs(cells) >= (1 << 16))[:, None, :], self.rng.integers(1, 8, size=(m, c, 3)).astype(np.float64) / 8.0,
                     10.0 ** self.rng.uniform(-3.0, -0.05, size=(m, c, 3)))
        want = np.broadcast_to(cells[:, None, :], (m, c, 3))
        p = ((want + u) * self.leaf).astype(np.float32)
        bad = (np.floor(p.astype(np.float64) / self.leaf).astype(np.int64) != want).any(axis=2)      # (float64 of a float32 over 1 or 0.5: exact)
        p[bad] = ((want[bad] + 0.5) * self.leaf).astype(np.float32)                                   # a member rounded onto a wall goes to the cell's middle
        assert (np.floor(p.astype(np.float64) / self.leaf).astype(np.int64) == want).all()
        return p

    def _add_many(self, cells, c):
        """c points strictly inside each of the (distinct, unused) cells: m x 3 integers"""
        cells = np.asarray(cells, np.int64).reshape(-1, 3)
        m = len(cells)
        tup = [tuple(r) for r in cells.tolist()]
        assert c >= 1 and len(set(tup)) == m and not (self.used & set(tup))
        self.used.update(tup)
        p = self._draw(cells, c)
        first = len(self.sizes)
        self.blocks.append((p.reshape(-1, 3), np.repeat(np.arange(first, first + m), c)))
        self.sizes += [c] * m
        self.cells += tup
        lo, hi = int(cells.min()), int(cells.max())
        self.lo = lo if self.lo is None else min(self.lo, lo)
        self.hi = hi if self.hi is None else max(self.hi, hi)
        return first

    def add(self, cell, c, pin=()):
        """c points strictly inside `cell`; pin = scan indices (negative: from the end) that members of this leaf are to occupy"""
        lid = self._add_many([cell], c)
        for q in pin:
            self.pins.append((q, lid))
        return self

    def add_row(self, start, sizes, axis=0, pin_last=()):
        """leaves of the given sizes in consecutive cells along `axis` from `start`: consecutive in the output order too"""
        for t, c in enumerate(sizes):
            cell = list(start); cell[axis] += t
            self.add(cell, c, pin=pin_last if t == len(sizes) - 1 else ())
        return self

    def fill(self, n_leaves, c, origin=(200, 200, 200), side=None):
        """n_leaves leaves of c points each in distinct cells of a cube beside the named ones"""
        side = side or int(np.ceil(n_leaves ** (1.0 / 3.0))) + 1
        v = self.rng.choice(side ** 3, size=n_leaves, replace=False)
        self._add_many(np.stack([origin[0] + v % side, origin[1] + (v // side) % side, origin[2] + v // (side * side)], axis=1), c)
        return self

    def build(self, name, classes=(), shuffle=True):
        pts = np.concatenate([b[0] for b in self.blocks])
        lab = np.concatenate([b[1] for b in self.blocks])
        n = len(pts)
        if shuffle:
            perm = self.rng.permutation(n)
            pts, lab = pts[perm], lab[perm]
        taken, pinned = set(), []
        for q, lid in self.pins:
            q = q % n
            assert q not in taken
            if lab[q] != lid:
                cand = [j for j in np.flatnonzero(lab == lid) if j not in taken]
                j = cand[0]
                pts[[q, j]] = pts[[j, q]]; lab[[q, j]] = lab[[j, q]]
            taken.add(q)
            pinned.append((q, self.sizes[lid]))
        # a size class the case is there for must hold a leaf whose float32 centroid depends on the order of the sum (ascending against descending scan
        # order); where chance made none, the class's first leaf is drawn again with other magnitudes -- the CPU tier checks the outcome by its own means
        def depends_on_order(rows):
            q, c = pts[rows], np.float32(len(rows))
            return bool((np.cumsum(q, axis=0, dtype=np.float32)[-1] / c != np.cumsum(q[::-1], axis=0, dtype=np.float32)[-1] / c).any())
        for size in sorted(set(classes)):
            lids = [l for l, c in enumerate(self.sizes) if c == size]
            rows = [np.flatnonzero(lab == l) for l in lids]
            for _ in range(200):
                if any(depends_on_order(r) for r in rows):
                    break
                pts[rows[0]] = self._draw(np.array([self.cells[lids[0]]], np.int64), size)[0]
            else:
                raise AssertionError((name, size))
        out = np.zeros((n, 4), np.float32)
        out[:, :3] = pts
        out[:, 3] = self.rng.uniform(0, 255, n).astype(np.float32)      # the intensity column: never read by the VoxelGrid
        return Case(name, out, self.leaf, self.sizes, self.lo, self.hi, classes, pinned=pinned)


# ---- the cases ------------------------------------------------------------------------------------------------------
SIZES = (1, 2, 63, 64, 65, 66, 127, 128, 129, 2047, 2048)
ORDER_CLASSES = tuple(s for s in SIZES if s > 2)      # one term, and two terms (a + b == b + a), cannot depend on the order


def _sizes(extra=None):
    b = Builder(0.5, 11 if extra is None else 12)
    for t, c in enumerate(SIZES):
        # the long leaves' members at both ends of the scan and in its last, partial bitmap word (4 740 = 148 * 32 + 4)
        b.add((3 * t - 9, 2 - t, t % 3 - 1), c, pin={65: (0,), 2048: (-1,), 129: (-3,)}.get(c, ()))
    if extra:
        b.add((40, -3, 2), extra)
    return b.build("sizes" if extra is None else f"sizes+{extra}", ORDER_CLASSES + ((extra,) if extra else ()))


def _bitmap_edge():
    out = []
    b = Builder(0.5, 21)            # n = 131 072: the bitmap at its last size, every word whole
    b.add((0, 0, 0), 65, pin=(0, 131050)).add((5, -2, 1), 2048, pin=(131071, 131040, 1))
    b.fill((131072 - 65 - 2048) // 33, 33)          # 3 907 leaves of 33 points: 128 931 points ...
    rest = 131072 - 65 - 2048 - ((131072 - 65 - 2048) // 33) * 33
    b.add((-7, 9, 3), rest)                          # ... and one of 28
    out.append(b.build("bitmap-131072", (65, 2048)))
    b = Builder(0.5, 22)            # n = 131 073: the sorting network, padded (65 -> 128, 129 -> 256, 2047 -> 2048) and unpadded (128, 2048)
    longs = (65, 128, 129, 2047, 2048)
    for t, c in enumerate(longs):
        b.add((4 * t, -t, 2), c, pin={65: (0,), 2047: (-1,), 129: (1, -2)}.get(c, ()))
    left = 131073 - sum(longs)
    b.fill(left // 33, 33)
    b.add((-7, 9, 3), left - (left // 33) * 33)
    out.append(b.build("network-131073", longs))
    return out


def _many_long():
    b = Builder(0.5, 31)
    b.fill(770, 65, origin=(-4, -4, -4))            # two more than DSH_BIG_BLOCKS: the long-leaf loop strides
    return [b.build("many-long-770x65", (65,))]


def _many_leaves():
    out = []
    for nl in (511, 512, 513, 1025, 1537, 64 * 512, 64 * 512 + 1, 140000):      # chunks: 1, 1, 2, 3, 4, 64, 65, 274
        b = Builder(0.5, 40 + nl % 97)
        b.fill(nl, 1, origin=(-30, -30, -30))
        out.append(b.build(f"leaves-{nl}"))
    return out


def _ordinary_part(b):
    """a few hundred points around the origin: leaves of assorted sizes, among them long ones"""
    b.add_row((-3, 1, 0), (5, 1, 70, 2, 33, 64, 65, 9))
    b.fill(60, 3, origin=(-6, -6, -6), side=5)
    return b


def _key_range():
    out = []
    ends = (("lo-in", -BIAS), ("hi-in", BIAS - 1), ("hi-out", BIAS), ("lo-out", -BIAS - 1))
    for axis in range(3):
        for tag, v in ends:
            b = _ordinary_part(Builder(0.5, 50 + 4 * axis + len(tag)))
            cell = [2, -1, 3]; cell[axis] = v
            b.add(cell, 3)
            # the cell a key that wrapped would alias: one past the top of a field carries into the next one (x = 2^20 -> (-2^20, y + 1, z),
            # y = 2^20 -> (x, -2^20, z + 1)); the z field is the topmost, and one below the bottom borrows from every field above
            al = list(cell)
            if v == BIAS and axis < 2:
                al[axis] = -BIAS; al[axis + 1] += 1
                b.add(al, 2)
            out.append(b.build(f"key-{'xyz'[axis]}-{tag}", (65, 70)))
    b = _ordinary_part(Builder(0.5, 71))
    b.add((-BIAS, -BIAS, -BIAS), 4).add((BIAS - 1, BIAS - 1, BIAS - 1), 5)     # extents 2^21 each: the spec's index reaches 2^63 - 1 and no further
    out.append(b.build("key-xyz-in", (65, 70)))
    b = _ordinary_part(Builder(0.5, 72))
    b.add((BIAS, BIAS, BIAS), 4)
    out.append(b.build("key-xyz-hi-out", (65, 70)))
    b = _ordinary_part(Builder(0.5, 73))
    b.add((-BIAS - 1, -BIAS - 1, -BIAS - 1), 4)
    out.append(b.build("key-xyz-lo-out", (65, 70)))
    return out


def _walls():
    """points ON leaf walls: the cell is written down here from the rule (floor of the float32 product), never computed from the cloud"""
    out = []
    f32 = np.float32
    for axis in range(3):
        xs, cs = [], []
        for k in (1, 2, 3, 7, 100, 4095):                      # leaf 0.5: k * 0.5 is exact and so is its product with inv = 2
            for s in (1, -1):
                w = f32(s * k * 0.5)
                xs += [np.nextafter(w, f32(-np.inf)), w, np.nextafter(w, f32(np.inf))]
                cs += [s * k - 1, s * k, s * k]
        xs += [f32(0.0), f32(-0.0), f32(-1e-45), f32(-1e-40), f32(1e-45)]      # signed zeros; the smallest and a larger negative denormal: cell -1
        cs += [0, 0, -1, -1, 0]
        rng = np.random.default_rng(80 + axis)
        pts = np.zeros((len(xs), 4), np.float32)
        pts[:, :3] = (10.0 ** rng.uniform(-3.0, -0.4, size=(len(xs), 3))).astype(np.float32)     # the other two axes: inside cell 0
        pts[:, axis] = np.array(xs, np.float32)
        cells = np.zeros((len(xs), 3), np.int64); cells[:, axis] = cs
        perm = rng.permutation(len(xs))
        pts, cells = pts[perm], cells[perm]
        _, cnt = np.unique(cells, axis=0, return_counts=True)
        out.append(Case(f"walls-{'xyz'[axis]}-0.5", pts, 0.5, cnt.tolist(), min(cs), max(cs), cells=cells))
        # leaf 0.4 (avia.yaml): inv = float32(2.5); the 101 multiples k * float32(0.4), six of which round into the cell below
        ks = np.arange(-50, 51)
        pts = np.zeros((101, 4), np.float32)
        pts[:, :3] = (10.0 ** rng.uniform(-3.0, -0.5, size=(101, 3))).astype(np.float32)
        pts[:, axis] = ks.astype(np.float32) * np.float32(0.4)
        cells = np.zeros((101, 3), np.int64); cells[:, axis] = [k - 1 if k in WALL_04_LOW else k for k in ks]
        perm = rng.permutation(101)
        pts, cells = pts[perm], cells[perm]
        _, cnt = np.unique(cells, axis=0, return_counts=True)
        out.append(Case(f"walls-{'xyz'[axis]}-0.4", pts, 0.4, cnt.tolist(), int(cells.min()), int(cells.max()), cells=cells))
    return out


def _radix_tiles():
    """shapes of the SORTED cloud against ds_centroid_kernel's tiles of 64: leaves in consecutive cells along x are consecutive runs of the sorted order.
    Every shape twice: as it is (the radix pipeline on an IMMESH_DS_RADIX context) and, `-fb`, with its LAST leaf moved to z cell 2^20 -- still the last
    leaf of the output, the sorted shape unchanged, and the hashed form of a default context gives up on it and falls back to the same pipeline."""
    out = []

    def rows(name, start, sizes, classes=()):
        out.append(Builder(0.5, 100 + len(out)).add_row(start, sizes).build(name, classes))
        b = Builder(0.5, 100 + len(out)).add_row(start, sizes[:-1]) if len(sizes) > 1 else Builder(0.5, 100 + len(out))
        b.add((start[0] + len(sizes) - 1, start[1], BIAS), sizes[-1])
        out.append(b.build(name + "-fb", classes))

    for n in (1, 63, 64, 65, 128, 129):
        for tail in (1, 3):          # the last point of the sorted cloud alone in its leaf (n_out's `+ own flag`), and not alone
            if tail > n:
                continue
            sizes, left, t = [], n - tail, 0
            while left > 0:
                c = min(left, (5, 1, 7, 2, 11, 1, 3)[t % 7]); sizes.append(c); left -= c; t += 1
            rows(f"tiles-n{n}-tail{tail}", (-4, 0, 0), sizes + [tail], (3,) if tail == 3 else ())
    for s in (0, 63, 64, 65):        # a run of 64 from sorted position s: starts on a tile boundary (0, 64), ends on one (0 -> 64, 64 -> 128), straddles (63, 65)
        rows(f"tiles-run64-at{s}", (-20, 1, -1), [1] * s + [64, 1, 1, 2], (64,))
    rows("tiles-run200", (-5, 0, 2), [1] * 10 + [200] + [1] * 5, (200,))     # tiles 1 and 2 hold no head
    rows("tiles-one-leaf-129", (3, -3, 3), [129], (129,))
    return out


def _big_radix():
    """262 144 + 257 points: ds_minmax_kernel's grid (1024 x 256 threads) strides; the cloud's extremes are held by points of the second sweep only"""
    n = 262144 + 257
    b = Builder(0.5, 140)
    b.add((-90, 0, 0), 1, pin=(262144 + 5,)).add((0, -91, 0), 1, pin=(262144 + 6,)).add((0, 0, -92), 1, pin=(262144 + 7,))
    b.add((93, 0, 0), 1, pin=(-1,)).add((0, 94, 0), 1, pin=(-2,)).add((0, 0, 95), 1, pin=(-3,))
    b.add((5, 1, 1), 300).add((6, 1, 1), 65)
    left = n - 6 - 365
    b.fill(left // 4, 4, origin=(-40, -40, -40), side=42)
    b.add((7, 1, 1), left - (left // 4) * 4)
    return [b.build("radix-262401", (300, 65))]


@functools.lru_cache(maxsize=None)
def family(name):
    return {"sizes": lambda: [_sizes(), _sizes(2049)], "bitmap-edge": _bitmap_edge, "many-long": _many_long, "many-leaves": _many_leaves,
            "key-range": _key_range, "walls": _walls, "radix-tiles": _radix_tiles, "big-radix": _big_radix}[name]()


FAMILIES = ("sizes", "bitmap-edge", "many-long", "many-leaves", "key-range", "walls", "radix-tiles", "big-radix")
# the cases that also go in as n x 3 arrays
STRIDE3 = ("sizes", "sizes+2049", "network-131073", "key-x-hi-out", "walls-x-0.4", "tiles-run200", "tiles-run200-fb", "tiles-n65-tail1", "tiles-n65-tail1-fb", "leaves-1025")


def all_cases():
    return [c for f in FAMILIES for c in family(f)]


def by_name(name):
    for c in all_cases():
        if c.name == name:
            return c
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def ordinary():
    """a cloud nothing is special about: after a fall-back it must take the hashed form again"""
    b = _ordinary_part(Builder(0.5, 7))
    b.fill(900, 2, origin=(10, -20, 5))
    return b.build("ordinary", (65, 70))


# ---- the third restatement: a dictionary, Python scalars, nothing shared with synth.voxel_grid_downsample or the checker -------------------
def cells_of(pts, leaf):
    """cell triple of every point: floor of the float32 product with float32(1 / leaf), taken one Python float at a time"""
    import math
    inv = np.float32(1.0 / leaf)
    prod = (np.asarray(pts[:, :3], np.float32) * inv).tolist()      # (the float32 products, exact as Python floats)
    return [(math.floor(x), math.floor(y), math.floor(z)) for x, y, z in prod]


def restate(pts, leaf, reverse=False, only_sizes=None):
    """-> (centroids n_out x 3 in (k, j, i) order, leaf sizes in that order).  reverse: every leaf summed in descending scan order.
    only_sizes: leaves of other sizes are left out (for the order-sensitivity check)."""
    members = {}
    for i, c in enumerate(cells_of(pts, leaf)):
        members.setdefault(c, []).append(i)
    keys = sorted(members, key=lambda c: (c[2], c[1], c[0]))
    cols = [[np.float32(v) for v in pts[:, a].tolist()] for a in range(3)]
    out, sizes = [], []
    for c in keys:
        m = members[c]
        if only_sizes is not None and len(m) not in only_sizes:
            continue
        if reverse:
            m = m[::-1]
        row = []
        for a in range(3):
            s = np.float32(0.0)
            col = cols[a]
            for i in m:
                s = s + col[i]
            row.append(s / np.float32(len(m)))
        out.append(row); sizes.append(len(m))
    return np.array(out, np.float32).reshape(-1, 3), sizes
