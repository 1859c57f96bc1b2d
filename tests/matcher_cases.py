"""Cases for the plane matcher (residual_pass / match_tree / match_trees_coop / plane_gates / test_plane, reg_kernels.hip; COVERAGE.md rows a10 - a12) --
plain numpy, no GPU.  Every claim made here is proven on the CPU checker by test_matcher_cases_cpu.py before test_gpu_matcher_paths.py compares the device.

MAPS.  A family is one configuration and one map: a build cloud and a sequence of update clouds.  Voxels are 2 m with max_layer 3 (cells of 1 / 0.5 / 0.25 m),
except the families that restate a construction at 0.5 m.  A TREE ROOT is built in two stages so that the order of its leaf list is known:

  * the build cloud holds a SKELETON: one point in each of the root's 64 layer-2 cells (a point of the cell's future patch), at the height of its plane.  The
    root and its eight layer-1 children see 64 / 8 points on two sheets 1 m / 0.5 m apart and are non-planar; every layer-2 child holds one point and is not
    initialised.  The root's leaf list is empty.
  * update s adds the other 11 points of a flat 4 x 3 patch to cell seq[s] of the root.  The cell's child node reaches its sixth point (skeleton + 5), is fitted, is planar,
    and is appended to the root's leaf list (regmap.hpp leaf_insert: the first free slot of the chain, else a new 15-slot line in FRONT of the chain).

So after the updates the list of a root with sequence seq holds seq[0..14] in slots 0..14 of its last line, seq[15..29] in the line before it, and so on;
the matcher walks the lines from the front (the newest line first).  `Root.lines()` restates that rule; nothing of it is read back from the device: what the
tests compare are the matcher's outputs, which do not depend on the order -- except through the tie rule, which is what the order is varied for.

CELLS are numbered c = 8 * o1 + o2 with o = 4 * xbit + 2 * ybit + zbit (the reference's octant index), so ascending c is the depth-first order of the
reference's recursion and c is monotone in the device's dfs_key.

EXACT families have dept_err = beam_err = 0 and are built and updated with a zero pose covariance: every point covariance is zero, every coordinate is
dyadic, every plane has the normal (0, 0, 1) and plane_var exactly zero, so two planes at the same distance from a point give it the same probability to
the last bit.  GENERIC families keep the shipped error model and jitter every coordinate: no two probabilities can be equal."""
import numpy as np

from immesh_amd import capi

VS, MAX_LAYER = 2.0, 3
SLOTS = 15                          # IM_LEAF_SLOTS: node ids of one leaf-list line
WAVE = 64
QUERY_COV = 1e-4                    # pose covariance of the queries: gives every query a non-zero covariance of its own
PX = np.array([-3, -1, 1, 3]) / 8.0  # a patch: 4 x 2 points about the cell centre, in units of the cell size
PY = np.array([-1, 1]) / 4.0


def make_config(exact, voxel_size=VS, max_layer=MAX_LAYER, **over):
    over.setdefault("cap_root_voxels", 1 << 12)
    over.setdefault("cap_scan_points", 20000)
    over.setdefault("cap_nodes", 1 << 15)           # a tree root takes 73 nodes: 5 600 in the largest family
    cfg = capi.avia_config(voxel_size=voxel_size, max_layer=max_layer, **over)
    for i in range(3):
        cfg.extT[i] = 0.0
    if exact:
        cfg.dept_err = 0.0; cfg.beam_err = 0.0
    return cfg


def f32_steps(x, k):
    """the float32 k steps above (k < 0: below) x"""
    a = np.array([x], np.float32)
    i = a.view(np.int32)
    assert a[0] > 0
    return (i + np.int32(k)).view(np.float32)[0]


def f32_range(x, lo, hi):
    """consecutive positive float32 values x[lo .. hi) steps from x"""
    a = np.array([x], np.float32)
    assert a[0] > 0
    return (a.view(np.int32)[0] + np.arange(lo, hi, dtype=np.int32)).view(np.float32)


def dfs_key(path, layer):
    """regmap.hpp dfs_key: the octant indices of a node's path, first layer in the most significant place"""
    k = 0
    for l in range(1, int(layer) + 1):
        k |= ((int(path) >> (3 * (l - 1))) & 7) << (3 * (4 - l))
    return k


def cell_origin(c):
    """min corner of layer-2 cell c (0.5 m) inside its root, local coordinates"""
    o1, o2 = c >> 3, c & 7
    return np.array([(o1 >> 2 & 1) * 1.0 + (o2 >> 2 & 1) * 0.5, (o1 >> 1 & 1) * 1.0 + (o2 >> 1 & 1) * 0.5, (o1 & 1) * 1.0 + (o2 & 1) * 0.5])


class Root:
    """one root voxel.  kind: 'tree' (skeleton + one patch per update, in the order seq), 'planar' (one flat sheet over the voxel), 'junk' (a non-planar
    root none of whose children is ever fitted: its list stays empty)"""
    def __init__(self, name, key, kind="tree", seq=(), levels=None, spoil=None, narrow=()):
        self.name, self.key, self.kind, self.seq = name, tuple(int(k) for k in key), kind, list(seq)
        self.narrow = tuple(narrow)               # cells whose patch is the 2 x 6 one of _patch12n (exact families)
        self.origin = np.array(self.key, float) * VS
        self.levels = dict(levels or {})          # cell -> height of its plane above the cell's floor (default: see level())
        self.spoil = spoil                        # (cell, update index): that update turns the cell's leaf non-planar

    def level(self, c, exact):
        if c in self.levels:
            return self.levels[c]
        return 0.25 if exact else 0.25 + (((c * 37) % 64) - 32) / 64.0 * 0.2       # generic: neighbours in x / y / z are 6 / 3 / 1 cm apart

    def plane_z(self, c, exact):
        return self.origin[2] + cell_origin(c)[2] + self.level(c, exact)

    def cell_centre(self, c):
        return self.origin + cell_origin(c) + 0.25

    def n_leaves(self, after_update=None):
        n = len(self.seq) if after_update is None else min(len(self.seq), after_update + 1)
        if self.spoil and (after_update is None or after_update >= self.spoil[1]):
            n -= 1
        return n if self.kind == "tree" else 0

    def lines(self):
        """the leaf list as leaf_insert leaves it, front line first: [[cell or None] * 15, ...] (None: a slot emptied by leaf_remove)"""
        chain = []
        for c in self.seq:
            for line in chain:
                if None in line:
                    line[line.index(None)] = c
                    break
            else:
                chain.insert(0, [c] + [None] * (SLOTS - 1))
        if self.spoil:
            for line in chain:
                if self.spoil[0] in line:
                    line[line.index(self.spoil[0])] = None
        return chain

    def line_counts(self):
        return [sum(1 for c in line if c is not None) for line in self.lines()]


def _grid(centre_xy, size, z, rng, ys):
    x, y = np.meshgrid(centre_xy[0] + PX * size, centre_xy[1] + np.asarray(ys) * size, indexing="ij")
    n = x.size
    p = np.stack([x.ravel(), y.ravel(), np.full(n, z)], axis=1)
    if rng is not None:
        p[:, :2] += rng.uniform(-size / 64, size / 64, (n, 2))
        p[:, 2] += np.clip(rng.normal(0, 0.0015, n), -0.003, 0.003)
    return p


def _patch8(centre_xy, size, z, rng):
    """4 x 2 points: x offsets +-3/8, +-1/8, y offsets +-1/4 of the cell size"""
    return _grid(centre_xy, size, z, rng, PY)


SKEL = 4    # index of the skeleton point (x offset -1/8, y offset 0) in the 4 x 3 grid


def _patch12(centre_xy, size, z, rng):
    """4 x 3 points (y offsets -1/4, 0, 1/4): a tree root's leaf.  Point SKEL is the cell's skeleton point (build cloud); the other 11 come with the
    cell's update: the node is fitted at its 6th point and refitted at its 12th over all twelve, so the plane's centre is the cell's centre and
    its radius sqrt(10 / 128) / 2 of the cell size (0.14 m at 0.5 m: the range gate reaches 0.42 m)"""
    return _grid(centre_xy, size, z, rng, (-0.25, 0.0, 0.25))


def _patch12n(centre_xy, size, z, rng):
    """2 x 6 points, x offsets +-1/4 of the cell size: the largest eigenvalue is (size / 4)^2 exactly, the radius size / 4 (0.125 m at 0.5 m) and
    3 radius = 0.375 m: numbers a float32 coordinate can meet exactly"""
    x, y = np.meshgrid(centre_xy[0] + np.array([-0.25, 0.25]) * size, centre_xy[1] + np.array([-5, -3, -1, 1, 3, 5]) / 16.0 * size, indexing="ij")
    assert rng is None
    return np.stack([x.ravel(), y.ravel(), np.full(12, z)], axis=1)


class Family:
    def __init__(self, name, exact, roots, seed=7, shipped=False):
        """shipped (exact families only): the same dyadic clouds under the shipped dept_err / beam_err -- plane_var is then not zero"""
        self.name, self.exact, self.roots = name, exact, roots
        self.cfg = make_config(exact and not shipped)
        self.by_name = {r.name: r for r in roots}
        assert len({r.key for r in roots}) == len(roots)
        self.rng = None if exact else np.random.default_rng(seed)
        self.build, self.updates = self._clouds()

    def map_state(self):
        return capi.make_state(cov_diag=0.0 if self.exact else 1e-8)

    def query_state(self, cov=QUERY_COV):
        return capi.make_state(cov_diag=cov)

    def _jit(self, p, s):
        return p if self.rng is None else p + self.rng.uniform(-s, s, np.shape(p))

    def _clouds(self):
        build, n_upd = [], max([len(r.seq) for r in self.roots] + [r.spoil[1] + 1 for r in self.roots if r.spoil] + [0])
        upd = [[] for _ in range(n_upd)]
        for r in self.roots:
            if r.kind == "planar":      # an 8 x 8 sheet over the voxel (dyadic), 0.3 m above its floor: a planar root, radius 0.8 m
                g = (np.arange(8) + 0.5) / 8.0 * VS
                x, y = np.meshgrid(g, g, indexing="ij")
                p = np.stack([x.ravel(), y.ravel(), np.full(64, 0.3125)], axis=1)
                if self.rng is not None:
                    p[:, :2] += self.rng.uniform(-0.05, 0.05, (64, 2)); p[:, 2] += np.clip(self.rng.normal(0, 0.002, 64), -0.004, 0.004)
                build.append(r.origin + p)
                continue
            patch = lambda c, z, rng: (_patch12n if c in r.narrow else _patch12)((r.origin + cell_origin(c))[:2] + 0.25, 0.5, z, rng)
            for c in range(64):         # the skeleton (tree and junk roots alike)
                o = r.origin + cell_origin(c)
                z = r.level(c, self.exact) if r.kind == "tree" else 0.25
                build.append(patch(c, o[2] + z, None)[SKEL:SKEL + 1])
            for s, c in enumerate(r.seq):
                upd[s].append(np.delete(patch(c, r.plane_z(c, self.exact), self.rng), SKEL, axis=0))
            if r.spoil:                 # 12 points on a second sheet 0.25 m above the leaf's plane: its second refit sees 9 + 12 points on two sheets
                c, s = r.spoil
                o = r.origin + cell_origin(c)
                z = r.plane_z(c, self.exact) + 0.25
                assert r.level(c, self.exact) + 0.25 < 0.49 and s >= r.seq.index(c) + 1
                a = _patch8(o[:2] + 0.25, 0.5, z, self.rng)
                b = _patch8(o[:2] + 0.25 + 1.0 / 64, 0.5, z, self.rng)[:4]
                upd[s].append(np.concatenate([a, b]))
        f32 = lambda a: np.ascontiguousarray(np.concatenate(a), dtype=np.float32)
        return f32(build), [f32(u) if u else np.zeros((0, 3), np.float32) for u in upd]

    # -- queries --------------------------------------------------------------------------------------------------------------------------------
    def q_leaf(self, root, c, dz=0.004, dxy=(0.03, -0.02)):
        """a point just above the plane of cell c of a tree root, near the cell's centre: that leaf wins"""
        r = self.by_name[root]
        p = r.cell_centre(c)
        return np.array([p[0] + dxy[0], p[1] + dxy[1], r.plane_z(c, self.exact) + dz])

    def q_planar(self, root, u=0.37, v=0.61, dz=0.004):
        r = self.by_name[root]
        return r.origin + np.array([u * VS, v * VS, 0.3125 + dz])

    def q_junk(self, root, u=0.3, v=0.6, w=0.2):
        return self.by_name[root].origin + np.array([u, v, w]) * VS

    def q_between(self, root, cells, frac=0.5):
        """EXACT families: the point in the middle of the centres of `cells` (2: neighbours in x; 4: the cells round a vertical edge), `frac` of the way from
        the lowest to the highest of their planes"""
        r = self.by_name[root]
        xy = np.mean([r.cell_centre(c)[:2] for c in cells], axis=0)
        zs = [r.plane_z(c, True) for c in cells]
        return np.array([xy[0], xy[1], min(zs) + frac * (max(zs) - min(zs))])


class Scan:
    """one call of immesh_residuals: points in lane order (point i is lane i % 64 of wavefront i // 64 of residual_kernel) with what is claimed of each"""
    def __init__(self, name, family, what):
        self.name, self.family, self.what = name, family, what
        self.pts, self.tests, self.extra, self.match, self.winner, self.partners = [], [], [], [], [], []
        self.cov = QUERY_COV

    def add(self, p, tests, match=True, extra=0, winner=None, partners=()):
        """winner: (root name, cell) of the leaf that must win, or None where the claim is only match / no match; partners: the cells of that root whose
        planes give the point one probability, the largest (exact families)"""
        self.pts.append(p); self.tests.append(tests); self.extra.append(extra); self.match.append(match); self.winner.append(winner)
        self.partners.append(tuple(partners))
        return self

    def points(self):
        return np.ascontiguousarray(np.array(self.pts), dtype=np.float32)

    def step_pairs(self, wave=0):
        """(point, leaf) pairs of every enumeration step of match_trees_coop in the first round of wavefront `wave`: each tree lane puts the next line of
        its root's list on the work list, front line first"""
        lanes = [self._lane_root[i] for i in range(wave * WAVE, min(len(self.pts), (wave + 1) * WAVE))]
        counts = [r.line_counts() if r is not None and r.kind == "tree" else [] for r in lanes]
        return [sum(c[s] for c in counts if len(c) > s) for s in range(max([len(c) for c in counts] + [0]))]


def scan_of(fam, name, what, lanes):
    """lanes: list of ('leaf', root, cell) | ('planar', root) | ('junk', root) | ('none',) -- one query each, the claims derived from the root's list"""
    s = Scan(name, fam, what)
    s._lane_root = []
    for k, ln in enumerate(lanes):
        jit = ((k * 13) % 17 - 8) / 8.0 * 0.02        # every lane its own point
        if ln[0] == "leaf":
            r = fam.by_name[ln[1]]
            s.add(fam.q_leaf(ln[1], ln[2], dxy=(0.03 + jit, -0.02 - 0.5 * jit)), tests=r.n_leaves(), winner=(ln[1], ln[2]))
        elif ln[0] == "planar":
            r = fam.by_name[ln[1]]
            s.add(fam.q_planar(ln[1], u=0.37 + jit, v=0.61 - jit), tests=1, winner=(ln[1], None))
        elif ln[0] == "junk":           # a non-planar root with an empty list: nothing tested, the neighbour probed (and absent)
            r = fam.by_name[ln[1]]
            s.add(fam.q_junk(ln[1], u=0.3 + jit), tests=0, match=False, extra=1)
        else:                           # no voxel there: not matched, not retried
            r = None
            s.add(np.array([-20.0 - k * 0.01, -20.0, 0.5]), tests=0, match=False, extra=0)
        s._lane_root.append(r)
    return s


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the generic family: list shapes, wave composition, pair counts
# ---------------------------------------------------------------------------------------------------------------------------------------------------
LIST_LENGTHS = (1, 2, 3, 14, 15, 16, 30, 31, 46)


def _seq(n, order):
    """n cells for a list of n leaves: forward = ascending depth-first key, reverse = descending"""
    cells = list(range(n))
    if order == "reverse":
        cells.reverse()
    return cells


def generic_family(order="forward"):
    roots, k = [], 0
    def key():
        nonlocal k
        k += 1
        return (2 + 2 * (k % 10), 2 + 2 * (k // 10), 0)          # two voxels apart: no root is a neighbour of another
    for n in LIST_LENGTHS:
        roots.append(Root(f"T{n}", key(), seq=_seq(n, order)))
    roots.append(Root("P", key(), kind="planar"))
    roots.append(Root("J", key(), kind="junk"))
    roots.append(Root("H", key(), seq=_seq(15, order), spoil=(_seq(15, order)[7], 46)))   # slot 7 of its one line emptied by update 46
    for j in range(64):
        roots.append(Root(f"F{j}", key(), seq=_seq(15, order)))
    return Family(f"generic-{order}", False, roots)


def generic_scans(fam):
    out = []
    T = lambda n, i=0: ("leaf", f"T{n}", fam.by_name[f"T{n}"].seq[i % n])
    for n in LIST_LENGTHS:
        # one tree lane alone: every list length, every position of the target in the list (first / last slot, front / back line)
        out.append(scan_of(fam, f"list{n}", f"one point on a list of {n} leaves; target in each position",
                           [T(n, i) for i in sorted({0, n // 2, n - 1, min(n - 1, 14), min(n - 1, 15)})]))
    out.append(scan_of(fam, "empty-list", "a non-planar root with an empty list beside a tree lane", [("junk", "J"), T(15), ("junk", "J")]))
    out.append(scan_of(fam, "hole", "a list of 14 with an emptied slot inside its line",
                       [("leaf", "H", c) for c in fam.by_name["H"].seq if c != fam.by_name["H"].spoil[0]]))
    for n in (1, 63, 64, 65):
        out.append(scan_of(fam, f"n{n}", f"{n} points, every lane a tree lane on its own root", [("leaf", f"F{j % 64}", fam.by_name["F0"].seq[j % 15]) for j in range(n)]))
    out.append(scan_of(fam, "one-tree-lane", "one tree lane among 63 planar-root lanes", [("planar", "P")] * 37 + [T(31, 20)] + [("planar", "P")] * 26))
    out.append(scan_of(fam, "64x64", "64 tree lanes on 64 roots: 960 pairs in one step", [("leaf", f"F{j}", fam.by_name["F0"].seq[(j * 7) % 15]) for j in range(64)]))
    out.append(scan_of(fam, "64x1", "64 tree lanes on one root of 46 leaves: 64 + 960 + 960 + 960 pairs", [T(46, j) for j in range(64)]))
    out.append(scan_of(fam, "gaps", "lanes without a voxel and planar lanes between tree lanes", [(("none",), T(16, 3), ("planar", "P"), ("none",), T(3, 1), ("junk", "J"))[j % 6] for j in range(64)]))
    out.append(scan_of(fam, "unequal", "lists of 1 .. 46 in one wave: lanes finish while others continue", [T(LIST_LENGTHS[j % 9], j) for j in range(64)]))
    out.append(scan_of(fam, "pairs1", "1 pair in the step", [("planar", "P")] * 5 + [T(1)] + [("none",)] * 3))
    out.append(scan_of(fam, "pairs63", "63 pairs: 4 full lines + 3", [T(15, 1), T(15, 2), T(3, 0), T(15, 4), T(15, 14)]))
    out.append(scan_of(fam, "pairs64", "64 pairs: 64 lanes on a list of 1", [T(1)] * 64))
    out.append(scan_of(fam, "pairs65", "65 pairs: 63 lists of 1 and one of 2", [T(1)] * 40 + [T(2, 1)] + [T(1)] * 23))
    return out


PAIR_CLAIMS = {"pairs1": [1], "pairs63": [63], "pairs64": [64], "pairs65": [65], "64x64": [960], "64x1": [64, 960, 960, 960], "one-tree-lane": [1, 15, 15],
               "n1": [15], "n63": [945], "n64": [960]}


def register_scan(fam, n=320):
    """>= 257 points for immesh_register: tree lanes in every wavefront of a 256-thread workgroup, planar lanes between them"""
    lanes = []
    for j in range(n):
        m = j % 5
        lanes.append(("planar", "P") if m == 4 else ("leaf", f"F{(j * 3) % 64}", fam.by_name["F0"].seq[j % 15]) if m < 2 else
                     ("leaf", f"T{LIST_LENGTHS[3 + j % 6]}", fam.by_name[f"T{LIST_LENGTHS[3 + j % 6]}"].seq[j % LIST_LENGTHS[3 + j % 6]]))
    return scan_of(fam, "register", "tree lanes in every wavefront of a resident workgroup", lanes)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the exact family: ties
# ---------------------------------------------------------------------------------------------------------------------------------------------------
D32 = 1.0 / 32


def tie_family(order, shipped=False):
    """Cells 0, 4, 2, 6 are the four lower cells of octant 0 round the vertical edge x = y = 0.5 (depth-first order 0 < 2 < 4 < 6).  `order` = 'small-first':
    the partner with the smaller key is inserted first; 'small-last': it is inserted last."""
    others = [c for c in range(8, 64)]
    def seq(n, first, last):
        mid = [c for c in others if c not in first + last][:n - len(first) - len(last)]
        s = first + mid + last
        assert len(s) == n and len(set(s)) == n
        return s
    sw = (lambda a, b: (a, b)) if order == "small-first" else (lambda a, b: (b, a))
    lv2 = {0: 0.25, 4: 0.25 + D32, 2: 0.125, 6: 0.125}              # two partners: 0 (+1/64) and 4 (-1/64) for a point half-way; 2 and 6 are out of range of it
    lv3a = {0: 0.25, 2: 0.25 + D32, 4: 0.25 + D32, 6: 0.4375}       # three partners at the edge: 0 (+), 2 (-), 4 (-); the key picks 0
    lv3b = {0: 0.25 + D32, 2: 0.25, 4: 0.25 + D32, 6: 0.4375}       # 0 (-), 2 (+), 4 (-): the key picks 0, the mirror of lv3a in the sign of dis
    lv3c = {0: 0.4375, 2: 0.25 + D32, 4: 0.25, 6: 0.25 + D32}       # partners 2 (-), 4 (+), 6 (-) with 0 a loser: the key picks 2
    roots, k = [], 0
    def add(name, **kw):
        nonlocal k
        k += 1
        roots.append(Root(name, (4 + 2 * (k % 10), 2 + 2 * (k // 10), 0), **kw))
    # the gates met exactly (see gate_equality_scans): keys chosen for the points (2, 2) and (4, 8), whose 1 + x^2 + y^2 is a square
    roots.append(Root("sigma-eq-leaf", (1, 1, 0), seq=seq(15, [0], []), levels={0: 0.25}))
    roots.append(Root("sigma-eq-root", (2, 4, 0), kind="planar"))
    roots.append(Root("range-eq", (1, 5, 0), seq=seq(15, [0, 4], []), levels={0: 0.375, 4: 0.25}, narrow=(0,)))
    a, b = sw([0], [4])
    add("pair-adjacent", seq=seq(15, a + b, []), levels=lv2)                       # slots 0 and 1: one batch of 64 whatever the lane
    add("pair-ends", seq=seq(15, a, b), levels=lv2)                                # slots 0 and 14 of a full line
    add("pair-lines", seq=seq(30, a, b), levels=lv2)                               # first slot of the back line, last slot of the front line: different steps
    add("pair-lines46", seq=seq(46, a, b), levels=lv2)                             # back line and a front line of one leaf
    four = [0, 2, 4, 6] if order == "small-first" else [6, 4, 2, 0]
    for nm, lv in (("three-a", lv3a), ("three-b", lv3b), ("three-c", lv3c)):
        add(nm, seq=seq(15, four[:2], four[2:]), levels=lv)                        # slots 0, 1, 13, 14 of one line
        add(nm + "-lines", seq=seq(31, four[:2], four[2:]), levels=lv)             # two in the back line, one in the middle line, one alone in the front line
    for j in range(64):                                                           # 64 full-line lanes: lane j owns pairs 15 j .. 15 j + 14 of the step's 960
        add(f"E{j}", seq=seq(15, a, b), levels=lv2)
    return Family(f"tie-{order}" + ("-shipped" if shipped else ""), True, roots, shipped=shipped)


def tie_scans(fam):
    """every scan's points are exact ties; winner = the partner with the smallest depth-first key, readable from the sign of dis"""
    out = []
    def pair(s, root):
        r = fam.by_name[root]
        return s.add(fam.q_between(root, [0, 4]), tests=r.n_leaves(), winner=(root, 0), partners=(0, 4))
    for root in ("pair-adjacent", "pair-ends", "pair-lines", "pair-lines46"):
        out.append(pair(Scan(root, fam, "two partners"), root))
    for root, win in (("three-a", 0), ("three-b", 0), ("three-c", 2), ("three-a-lines", 0), ("three-b-lines", 0), ("three-c-lines", 2)):
        s = Scan(root, fam, "three partners round a vertical edge")
        r = fam.by_name[root]
        lo = min(r.levels[c] for c in (0, 2, 4, 6))
        s.add(fam.q_between(root, [0, 2, 4, 6], frac=(D32 / 2) / (0.4375 - lo)), tests=r.n_leaves(), winner=(root, win), partners=(2, 4, 6) if win else (0, 2, 4))
        out.append(s)
    s = Scan("ties-960", fam, "64 full-line lanes, partners in the first and the last slot: lanes 4, 8, 12, ... have them in different batches of the step")
    for j in range(64):
        pair(s, f"E{j}")
    out.append(s)
    s = Scan("ties-one-root", fam, "64 lanes on one root, all tied")
    for j in range(64):
        pair(s, "pair-lines")
    out.append(s)
    s = Scan("ties-mixed", fam, "tied and untied lanes, lists of 15 / 30 / 31 / 46 in one wave")
    for j in range(64):
        root = ("pair-ends", "pair-lines", "three-a-lines", "pair-lines46", "three-c", "three-b-lines")[j % 6]
        if j % 4 == 3:
            c = fam.by_name[root].seq[(5 + j) % 15]
            s.add(fam.q_leaf(root, c, dz=1.0 / 256, dxy=(1.0 / 32, -1.0 / 64)), tests=fam.by_name[root].n_leaves(), winner=(root, c))
        elif root.startswith("pair"):
            pair(s, root)
        else:
            r = fam.by_name[root]
            lo = min(r.levels[c] for c in (0, 2, 4, 6))
            s.add(fam.q_between(root, [0, 2, 4, 6], frac=(D32 / 2) / (0.4375 - lo)), tests=r.n_leaves(), winner=(root, 2 if "three-c" in root else 0),
                  partners=(2, 4, 6) if "three-c" in root else (0, 2, 4))
    out.append(s)
    # all partners fail the sigma gate: a pose covariance of 1e-10 leaves 3 sigma far below the 1 / 64 to either plane
    s = Scan("tie-sigma-fail", fam, "a tie whose partners all fail the sigma gate: no match, one probe of the (absent) neighbour")
    s.cov = 1e-10
    for root in ("pair-ends", "pair-lines", "three-a"):
        r = fam.by_name[root]
        p = fam.q_between(root, [0, 4]) if root.startswith("pair") else fam.q_between(root, [0, 2, 4, 6], frac=(D32 / 2) / (0.4375 - 0.25))
        s.add(p, tests=r.n_leaves(), match=False, extra=1, winner=(root, 0), partners=(0, 4) if root.startswith("pair") else (0, 2, 4))
    out.append(s)
    return out


SIGMA_EQ_COV = 2.0 ** -12


def gate_equality_scans(fam):
    """EXACT families: points that meet a gate exactly, and their float32 neighbours.
    sigma gate (dis < sigma_num sqrt(sigma_l)): with plane_var = 0 and the normal (0, 0, 1), sigma_l is the point's var_zz = c (1 + x^2 + y^2) for a pose
    covariance c I at the identity.  c = 2^-12 and (x, y) = (2, 2) give sigma_l = 9 / 4096 and 3 sigma = 9 / 64; (4, 8) gives 27 / 64: a point that far above a
    plane is NOT accepted, the float32 below it is.  (2, 2) is the corner of a tree root's cell 0 (the leaf path), (4, 8) lies on a planar root (test_plane).
    range gate (range_dis <= 3 radius): the leaf of cell 0 of 'range-eq' has radius 1 / 8; a point in its plane 3 / 8 from its centre is accepted (dis = 0),
    the float32 beyond it goes to the neighbouring leaf of cell 4, 1 / 8 below (dis = +1 / 8)."""
    out = []
    s = Scan("sigma-eq", fam, "dis_to_plane == sigma_num * sqrt(sigma_l): rejected; one float32 nearer: accepted -- on a leaf and on a planar root")
    s.cov = SIGMA_EQ_COV
    r = fam.by_name["sigma-eq-leaf"]
    z = np.float32(r.plane_z(0, True) + 9.0 / 64)
    s.add(np.array([2.0, 2.0, z]), tests=15, match=False, extra=1, winner=None)
    s.add(np.array([2.0, 2.0, f32_steps(z, -1)]), tests=15, match=True, winner=("sigma-eq-leaf", 0))
    s.add(np.array([2.0, 2.0, f32_steps(z, 1)]), tests=15, match=False, extra=1)
    z = np.float32(0.3125 + 27.0 / 64)
    s.add(np.array([4.0, 8.0, z]), tests=1, match=False, extra=1)
    s.add(np.array([4.0, 8.0, f32_steps(z, -1)]), tests=1, match=True, winner=("sigma-eq-root", None))
    s.add(np.array([4.0, 8.0, f32_steps(z, 1)]), tests=1, match=False, extra=1)
    out.append(s)
    s = Scan("range-eq", fam, "range_dis == 3 radius on a leaf: accepted; one float32 further: the neighbouring leaf")
    r = fam.by_name["range-eq"]
    c = r.cell_centre(0)
    x, z = np.float32(c[0] + 0.375), r.plane_z(0, True)
    s.add(np.array([x, c[1], z]), tests=15, winner=("range-eq", 0))
    s.add(np.array([f32_steps(x, -1), c[1], z]), tests=15, winner=("range-eq", 0))
    s.add(np.array([f32_steps(x, 1), c[1], z]), tests=15, winner=("range-eq", 4))
    out.append(s)
    return out


def batch_split_lanes():
    """lanes of a 64 x 15 step whose first and last slot fall into different batches of 64 pairs"""
    return [j for j in range(64) if (15 * j) // 64 != (15 * j + 14) // 64]


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the construction at 0.5 m (avia.yaml's voxel): one root, eight leaves at layer 1
# ---------------------------------------------------------------------------------------------------------------------------------------------------
class Small:
    """root voxel (20, 20, 0) of 0.5 m, map built at t = (10.25, 0, 0); each octant holds a flat 8-point patch: z = 0.125 in the lower and 0.375 in the
    upper octants, except octant 4 (x high, y low, z low) at 0.15625.  A point at y = 10.125, z = 0.140625 is 1 / 64 from the planes of octants 0, 2, 6
    (below it) and 4 (above it)."""
    T = (10.25, 0.0, 0.0)
    XS = (10.13, 10.2, 10.25, 10.3)

    def __init__(self, exact=True, reverse=False):
        self.cfg = make_config(exact, voxel_size=0.5, max_layer=2)
        self.exact = exact
        pts = []
        for o in range(8):
            org = np.array([10.0 + (o >> 2 & 1) * 0.25, 10.0 + (o >> 1 & 1) * 0.25, (o & 1) * 0.25])
            z = 0.15625 if o == 4 else org[2] + 0.125
            pts.append(_patch8(org[:2] + 0.125, 0.25, z, None))
        w = np.concatenate(pts[::-1] if reverse else pts)
        self.build = np.ascontiguousarray(w - np.array(self.T), dtype=np.float32)

    def map_state(self):
        return capi.make_state(t=self.T, cov_diag=0.0)

    def query_state(self, cov=QUERY_COV):
        return capi.make_state(t=self.T, cov_diag=cov)

    def queries(self):
        w = np.array([[x, 10.125, 0.140625] for x in self.XS])
        return np.ascontiguousarray(w.astype(np.float32).astype(np.float64) - np.array(self.T), dtype=np.float32)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# max_layer = 0
# ---------------------------------------------------------------------------------------------------------------------------------------------------
class Flat:
    """max_layer = 0: a planar root is tested, a non-planar root has nothing below it (match_tree returns, residual_pass makes no tree lane of it)"""
    def __init__(self):
        self.cfg = make_config(False, voxel_size=VS, max_layer=0)
        rng = np.random.default_rng(3)
        g = (np.arange(6) + 0.5) / 6.0 * VS
        x, y = np.meshgrid(g, g, indexing="ij")
        sheet = np.stack([x.ravel(), y.ravel(), np.full(36, 0.3)], axis=1) + rng.uniform(-0.003, 0.003, (36, 3))
        blob = rng.uniform(0.1, 1.9, (40, 3))
        self.o_plane, self.o_blob = np.array([4.0, 4.0, 0.0]), np.array([8.0, 4.0, 0.0])
        self.build = np.ascontiguousarray(np.concatenate([self.o_plane + sheet, self.o_blob + blob]), dtype=np.float32)

    def map_state(self):
        return capi.make_state(cov_diag=1e-8)

    def query_state(self, cov=QUERY_COV):
        return capi.make_state(cov_diag=cov)

    def scan(self, n=70):
        s = Scan("max-layer-0", self, "max_layer = 0: planar root tested, non-planar root has no list")
        for j in range(n):
            x, y = 0.3 + 0.02 * (j % 70), 0.9 + 0.2 * (j // 70)
            if j % 2:
                s.add(self.o_blob + np.array([x, y, 0.7]), tests=0, match=False, extra=1)
            else:
                s.add(self.o_plane + np.array([x, y, 0.304]), tests=1, match=True, extra=0)
        return s


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the retry round (0.5 m voxels round the origin, where loc = p / voxel_size meets centre +- quarter inside the voxel)
# ---------------------------------------------------------------------------------------------------------------------------------------------------
class Retry:
    """BuildResidualListOMP compares loc = (float)(p / voxel_size) -- voxel units -- with the voxel's centre +- quarter in metres.  In the voxel
    with key 0 on an axis (0.5 m: centre 0.25, quarter 0.125) that is p > 0.1875 -> key + 1, p < 0.0625 -> key - 1, else the own key.  The own root
    (0, 0, 0) is a planar root whose plane is a 4 cm patch in its far corner: every query fails its range gate, so every query is retried.
    Neighbours: (1, 0, 0) a planar root that accepts, (0, 0, -1) a tree (0.5 m root, 8 leaves at layer 1) that accepts, (0, 0, 1) a planar root that rejects
    (range gate), (-1, 0, 0), (0, +-1, 0) and every other key absent."""
    LO, HI = 0.0625, 0.1875

    def __init__(self):
        self.cfg = make_config(False, voxel_size=0.5, max_layer=2)
        rng = np.random.default_rng(5)
        own = np.array([0.45, 0.45, 0.45]) + np.concatenate([rng.uniform(-0.02, 0.02, (12, 2)), rng.uniform(-0.001, 0.001, (12, 1))], axis=1)
        # (1, 0, 0): a strip along the face x = 0.5, horizontal at z = 0.125
        strip = np.stack([0.5 + rng.uniform(0.01, 0.06, 30), rng.uniform(0.01, 0.49, 30), 0.125 + rng.uniform(-0.002, 0.002, 30)], axis=1)
        # (0, 0, -1): eight octants of 0.25 m, each a horizontal patch; the upper ones 3 cm below z = 0 (the queries are straight above the first)
        tree = []
        for o in range(8):
            org = np.array([(o >> 2 & 1) * 0.25, (o >> 1 & 1) * 0.25, -0.5 + (o & 1) * 0.25])
            tree.append(_patch8(org[:2] + 0.125, 0.25, (-0.03 if o & 1 else -0.375) + (o - 4) * 0.002, rng))
        far = np.array([0.45, 0.45, 0.95]) + np.concatenate([rng.uniform(-0.02, 0.02, (12, 2)), rng.uniform(-0.001, 0.001, (12, 1))], axis=1)
        self.build = np.ascontiguousarray(np.concatenate([own, strip, np.concatenate(tree), far]), dtype=np.float32)

    def map_state(self):
        return capi.make_state(cov_diag=1e-8)

    def query_state(self, cov=1e-2):
        return capi.make_state(cov_diag=cov)

    def scan(self, reps=6, step=0.004):
        """per axis the four float32 positions either side of the two thresholds, the other axes in the middle band; then the own root accepting"""
        assert 0.125 + step * reps < self.HI
        s = Scan("retry", self, "own root accepts nothing; neighbour absent / planar / tree / rejecting / the own root again")
        s.cov = 1e-2
        lo, hi = np.float32(self.LO), np.float32(self.HI)
        edge = [(f32_steps(lo, -1), -1), (lo, 0), (hi, 0), (f32_steps(hi, 1), 1)]
        base = np.array([0.125, 0.125, 0.125])
        # what the neighbour does with a point of the middle band: tests it runs, whether it accepts
        nb = {(1, 0, 0): (1, True), (0, 0, -1): (8, True), (0, 0, 1): (1, False), (0, 0, 0): (1, False)}
        for rep in range(reps):                   # 12 points each: the tree neighbour's lanes lie in every wavefront
            for ax in range(3):
                for v, d in edge:
                    p = base.copy(); p[ax] = v
                    p[(ax + 1) % 3] += step * rep
                    k = tuple(d if a == ax else 0 for a in range(3))
                    t, ok = nb.get(k, (0, False))
                    s.add(p, tests=1 + t, match=ok, extra=1)
        for j in range(3):                        # the own root accepts: no probe
            s.add(np.array([0.45 + 0.005 * j, 0.45, 0.452]), tests=1, match=True, extra=0)
        return s


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# gate sweeps: generic planes, shipped error model; the position of each flip is found on the checker by bisection over float32 values
# ---------------------------------------------------------------------------------------------------------------------------------------------------
SWEEP = 1024


class Gates:
    """two planar roots under the shipped error model, every coordinate jittered.  The range gate is swept on a SMALL plane (a 6 cm patch in the middle of
    its voxel, 3 radius ~ 5 cm: the gate closes inside the voxel); the sigma gate on a sloped sheet over the whole voxel (3 sigma ~ 4 cm above it)."""
    def __init__(self):
        self.cfg = make_config(False)
        rng = np.random.default_rng(9)
        self.o_small, self.o_sheet = np.array([4.0, 4.0, 0.0]), np.array([8.0, 4.0, 0.0])
        small = np.array([1.0, 1.0, 0.5]) + np.concatenate([rng.uniform(-0.03, 0.03, (20, 2)), rng.uniform(-0.001, 0.001, (20, 1))], axis=1)
        g = (np.arange(6) + 0.5) / 6.0 * VS
        x, y = np.meshgrid(g, g, indexing="ij")
        sheet = np.stack([x.ravel(), y.ravel(), 0.3 + 0.05 * x.ravel()], axis=1) + rng.uniform(-0.003, 0.003, (36, 3))
        self.build = np.ascontiguousarray(np.concatenate([self.o_small + small, self.o_sheet + sheet]), dtype=np.float32)

    def map_state(self):
        return capi.make_state(cov_diag=1e-8)

    def query_state(self, cov=1e-6):
        return capi.make_state(cov_diag=cov)

    def range_line(self, x):
        """points of the small plane's voxel, in its plane, x metres (float32) along +x: the range gate closes somewhere past 3 radius"""
        x = np.asarray(x, np.float32)
        return np.stack([x, np.full(len(x), np.float32(5.013)), np.full(len(x), np.float32(0.5004))], axis=1)

    RANGE_BRACKET = (5.0, 5.3)

    def sigma_line(self, z):
        """points above the sloped sheet, z metres (float32) up: the sigma gate closes where dis reaches 3 sigma"""
        z = np.asarray(z, np.float32)
        return np.stack([np.full(len(z), np.float32(9.13)), np.full(len(z), np.float32(5.07)), z], axis=1)

    SIGMA_BRACKET = (0.37, 1.2)

    def above_centre(self, centre, normal, h):
        """float32 points on the normal through a plane's centre: dis_to_center - dis_to_plane^2 is zero up to rounding, of either sign"""
        return np.ascontiguousarray(np.asarray(centre)[None, :] + np.asarray(h)[:, None] * np.asarray(normal)[None, :], dtype=np.float32)


def bisect_f32(decide, lo, hi):
    """decide(x: float32) -> bool with decide(lo) != decide(hi): the float32 x with decide(x) == decide(lo) whose successor decides otherwise"""
    a, b = np.array([lo], np.float32).view(np.int32)[0], np.array([hi], np.float32).view(np.int32)[0]
    da = decide(np.array([a], np.int32).view(np.float32)[0])
    assert da != decide(np.array([b], np.int32).view(np.float32)[0]), "the bracket does not hold a flip"
    while b - a > 1:
        m = (int(a) + int(b)) // 2
        if decide(np.array([m], np.int32).view(np.float32)[0]) == da:
            a = m
        else:
            b = m
    return np.array([a], np.int32).view(np.float32)[0]


UNREACHED = {
    "coop == false for node ids beyond 26 bits": "needs 2^26 nodes (24 GB of node records); IMMESH_MATCH_SEQ runs the same match_tree on every case instead",
    "ties on the resident grid": "immesh_register moves the pose after its first pass, so no later pass sees an exact tie; ties go through immesh_residuals",
    "the sharded map": "one device here; test_gpu_sharded.py compares the sharded matcher's sums with the unsharded ones",
}


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# running a family on a library (the checker or the device: capi.HotPath of either)
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def build_map(h, fam, upto=None, each=None):
    """map_build + the family's updates (all, or the first `upto`); each(s): called after update s"""
    h.map_build(fam.build, fam.map_state())
    for s, u in enumerate(getattr(fam, "updates", [])[:upto]):
        if len(u):
            h.map_update(u, fam.map_state())
        if each:
            each(s)


def run_scan(h, fam, pts, cov=QUERY_COV):
    """immesh_residuals / orc_residuals on pts -> the result dict + the call's n_plane_tests / n_extra_probe"""
    h.counters(reset=True)
    r = h.residuals(np.ascontiguousarray(pts, dtype=np.float32), fam.query_state(cov))
    c = h.counters()
    r["n_plane_tests"], r["n_extra_probe"] = c["n_plane_tests"], c["n_extra_probe"]
    return r


def planes_of_root(table, key):
    t = table[(table["key"] == np.array(key, np.int64)).all(axis=1)]
    return t[t["is_plane"] == 1]


def gate_sweeps(o, g):
    """the two sweeps of Gates, located on the library `o` (the checker): -> {name: (points, decisions)}"""
    out = {}
    for name, line, bracket in (("range", g.range_line, g.RANGE_BRACKET), ("sigma", g.sigma_line, g.SIGMA_BRACKET)):
        decide = lambda x: run_scan(o, g, line(np.array([x], np.float32)), 1e-6)["n_match"] == 1
        edge = bisect_f32(decide, *bracket)
        pts = line(f32_range(edge, -SWEEP // 2, SWEEP // 2))
        r = run_scan(o, g, pts, 1e-6)
        dec = np.zeros(len(pts), bool); dec[r["match_idx"]] = True
        out[name] = (pts, dec)
    return out


def centre_line(o, g):
    """points on the normal through the sheet's centre, within a centimetre of it: dis_to_center - dis_to_plane^2 rounds to either sign"""
    t = o.dump_planes()
    rec = t[(t["key"] == np.array([4, 2, 0])).all(axis=1)][0]
    return g.above_centre(rec["center"], rec["normal"], np.arange(-40, 41) * 0.00025)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the gates of the LEAF paths (match_trees_coop's and match_tree's own copies): the same bisected sweeps on a generic leaf of a tree root
# ---------------------------------------------------------------------------------------------------------------------------------------------------
LEAF_ROOT, LEAF_CELL, LEAF_COV = "T1", 0, 1e-6


def leaf_lines(fam):
    """lines of float32 points at the one leaf of root T1 of a generic family (shipped error model, jittered plane): along +x in its plane (the range gate
    closes near 3 radius = 0.42 m from its centre, inside the root; no other plane of the root can take the point) and straight up from near its centre
    (the sigma gate closes some centimetres above it) -> {name: (line function, bracket)}"""
    r = fam.by_name[LEAF_ROOT]
    c, z = r.cell_centre(LEAF_CELL), r.plane_z(LEAF_CELL, False)
    rng_line = lambda x: np.stack([np.asarray(x, np.float32), np.full(len(x), np.float32(c[1] + 0.011)), np.full(len(x), np.float32(z + 0.002))], axis=1)
    sig_line = lambda h: np.stack([np.full(len(h), np.float32(c[0] + 0.031)), np.full(len(h), np.float32(c[1] - 0.017)), np.asarray(h, np.float32)], axis=1)
    return {"leaf-range": (rng_line, (c[0] + 0.3, c[0] + 0.6)), "leaf-sigma": (sig_line, (z + 0.004, z + 0.24))}


FILLER = "T30"      # the root of the lanes between the swept lanes: its front line is FULL (lines of 15 and 15), see swept_pair_lanes


def interleave(fam, pts):
    """pts with a matched lane of the 30-leaf root before each (even lanes: the filler, odd lanes: the swept leaf's root).  In the first enumeration step
    an even lane puts 15 pairs on the work list and an odd lane its one pair, so the swept pairs lie far from their owners' positions: swept_pair_lanes"""
    r = fam.by_name[FILLER]
    n = len(r.seq)
    fill = np.array([fam.q_leaf(FILLER, r.seq[k % n], dxy=(0.03 - 0.0005 * (k % 40), -0.02 + 0.0003 * (k % 50))) for k in range(len(pts))], np.float32)
    out = np.empty((2 * len(pts), 3), np.float32)
    out[0::2], out[1::2] = fill, pts
    return out


def swept_pair_lanes(fam, n_lanes=WAVE):
    """[(owner lane, evaluating lane)] of the swept leaf's pair in a wavefront of `n_lanes` interleaved points, restated from match_trees_coop: in step 0
    lane l contributes the front line of its root's list (Root.lines()), the pairs are numbered by the prefix sum over the lanes, and pair idx is evaluated
    by lane idx % 64 of its batch.  The swept root has one line of one leaf, so step 0 is the only step that holds its pair."""
    front = lambda name: fam.by_name[name].line_counts()[0]
    assert fam.by_name[LEAF_ROOT].line_counts() == [1]
    cnt = [front(FILLER) if l % 2 == 0 else front(LEAF_ROOT) for l in range(n_lanes)]
    start = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    return [(l, int(start[l]) % WAVE) for l in range(1, n_lanes, 2)]


def leaf_gate_sweeps(o, fam):
    """-> {name: (interleaved points, decisions of the swept points)}; located on the library `o` (the checker)"""
    out = {}
    for name, (line, bracket) in leaf_lines(fam).items():
        decide = lambda x: run_scan(o, fam, line(np.array([x], np.float32)), LEAF_COV)["n_match"] == 1
        edge = bisect_f32(decide, *bracket)
        pts = interleave(fam, line(f32_range(edge, -SWEEP // 2, SWEEP // 2)))
        r = run_scan(o, fam, pts, LEAF_COV)
        dec = np.zeros(len(pts), bool); dec[r["match_idx"]] = True
        assert dec[0::2].all()                       # the lanes in between all match
        out[name] = (pts, dec[1::2])
    return out


def leaf_centre_line(o, fam):
    """points on the normal through the leaf's centre (interleaved as above): dis_to_center - dis_to_plane^2 rounds to either sign"""
    r = fam.by_name[LEAF_ROOT]
    pl = planes_of_root(o.dump_planes(), r.key)
    assert len(pl) == 1
    h = np.arange(-40, 41) * 0.00025
    return interleave(fam, np.ascontiguousarray(pl[0]["center"][None, :] + h[:, None] * pl[0]["normal"][None, :], dtype=np.float32))


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# immesh_register: the compositions with unmatched, retried and short-list lanes, padded with matched lanes to more than one 256-thread workgroup
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def concat_scans(name, what, scans):
    s = Scan(name, scans[0].family, what)
    s.cov = scans[0].cov
    for a in scans:
        for k in ("pts", "tests", "extra", "match", "winner", "partners"):
            getattr(s, k).extend(getattr(a, k))
    return s


def register_cases(fam):
    """(family, scan, prior) for immesh_register on the resident grid and on the chain; every scan has >= 257 points.  generic family: the compositions
    with an empty list, the emptied slot, lanes without a voxel, lists of 1 / 2 / 3 and unequal lists, each followed by the matched lanes of register_scan;
    Retry (every kind of neighbour in every wavefront of the workgroup, the tree neighbour a cooperative call of some lanes) and max_layer = 0"""
    by = {s.name: s for s in generic_scans(fam)}
    pad = register_scan(fam, 200)
    prior = capi.make_state(t=[0.0015, -0.001, 0.0012], cov_diag=1e-4)
    out = [(fam, register_scan(fam), prior)]
    out.append((fam, concat_scans("register-mixed", "empty list, emptied slot, no voxel, short and unequal lists, then matched lanes",
                                  [by["empty-list"], by["gaps"], by["hole"], by["list1"], by["list2"], by["list3"], by["unequal"], pad]), prior))
    rt, fl = Retry(), Flat()
    out.append((rt, rt.scan(reps=22, step=0.002), capi.make_state(t=[0.0, 0.0, 0.0], cov_diag=1e-2)))
    out.append((fl, fl.scan(n=280), capi.make_state(t=[0.001, -0.001, 0.0015], cov_diag=1e-4)))
    for f, s, _ in out:
        assert len(s.pts) >= 257, s.name
    return out
