"""numpy / Python restatement of the region-bucket contract of include/immesh_regions.h (the reference's Triangle_manager::insert_triangle_to_list /
erase_triangle_from_list, Sync_triangle_set and synchronize_triangle_list_for_disp).  Test infrastructure: nothing here runs on the device.

    key       ((p0 + p1) + p2) / 3.0 per component in float64 from the float32 vertex positions, divided by the region size, std::round
    table     regions in creation order (first insertion of a key; a scan commits all removals, then its insertions in add-list order)
    dirty     set by creation, insertion, and a removal that finds the region; cleared by a sync that takes the region
    sync      the dirty regions (all with force_all) in index order, each with its live triplets in lexicographic order
"""
import numpy as np


def round_half_away(x):
    """std::round on float64, exactly: x - trunc(x) is exact in binary floating point, so the tie test is too (np.round rounds ties to even and
    floor(x + 0.5) rounds 0.49999999999999994 up: neither is used)."""
    x = np.asarray(x, np.float64)
    t = np.trunc(x)
    frac = x - t
    return t + np.where(frac >= 0.5, 1.0, 0.0) - np.where(frac <= -0.5, 1.0, 0.0)


def region_keys(vtx_xyz, tri, region_size, rounding=round_half_away):
    """keys (n, 3) int32 of the triangles `tri` (n, 3) -- vertex ids used in the order given (the contract: sorted triplets)"""
    p = np.asarray(vtx_xyz, np.float32).astype(np.float64).reshape(-1, 3)
    t = np.asarray(tri, np.int64).reshape(-1, 3)
    c = ((p[t[:, 0]] + p[t[:, 1]]) + p[t[:, 2]]) / 3.0
    return rounding(c / np.float64(region_size)).astype(np.int64).astype(np.int32)


class RegionChecker:
    def __init__(self, region_size, rounding=round_half_away):
        self.S = float(region_size)
        self.rounding = rounding
        self.vtx = np.zeros((0, 3), np.float32)
        self.index = {}      # key -> region index
        self.keys = []       # region index -> key (tuple of three ints): m_triangle_set_vector order
        self.sets = []       # region index -> set of sorted triplets
        self.dirty = []      # m_if_required_synchronized
        self.flips = {}      # live triplet -> m_index_flip

    def keys_of(self, tri):
        return [tuple(int(v) for v in k) for k in region_keys(self.vtx, tri, self.S, self.rounding)]

    def apply(self, m):
        """m = HotPath.mesh_fetch() of one scan (a fetch dict).  Returns (removals, regions created)."""
        nv = np.asarray(m["new_vtx"], np.float32).reshape(-1, 3)
        if "vtx_base" in m and len(nv):
            assert m["vtx_base"] == len(self.vtx)
        self.vtx = np.concatenate([self.vtx, nv], axis=0)
        rem = [tuple(map(int, t)) for t in np.asarray(m["tri_rem"]).reshape(-1, 3)]
        add = [tuple(map(int, t)) for t in np.asarray(m["tri_add"]).reshape(-1, 3)]
        for tri, key in zip(rem, self.keys_of(rem) if rem else []):            # remove_triangle_list first ...
            r = self.index.get(key)
            self.flips.pop(tri, None)
            if r is None:
                continue
            self.sets[r].discard(tri)
            self.dirty[r] = True
        created = 0
        fa = np.asarray(m.get("flip_add", np.zeros(len(add), np.uint8))).reshape(-1)
        for tri, key, f in zip(add, self.keys_of(add) if add else [], fa):     # ... then the insertions, in add-list order
            r = self.index.get(key)
            if r is None:
                r = len(self.keys)
                self.index[key] = r; self.keys.append(key); self.sets.append(set()); self.dirty.append(True)
                created += 1
            self.sets[r].add(tri)
            self.dirty[r] = True
            self.flips[tri] = int(f)
        if "tri_upd" in m:
            for tri, f in zip(np.asarray(m["tri_upd"]).reshape(-1, 3), np.asarray(m["flip_upd"]).reshape(-1)):   # flips do not touch the flags
                self.flips[tuple(map(int, tri))] = int(f)
        return len(rem), created

    def table(self):
        """(keys (n, 3), n_triangles (n), dirty (n)) in index order"""
        n = len(self.keys)
        return (np.array(self.keys, np.int32).reshape(n, 3), np.array([len(s) for s in self.sets], np.int32), np.array(self.dirty, np.int32).reshape(n))

    def live(self):
        out = set()
        for s in self.sets:
            out |= s
        return out

    def sync(self, force_all=False):
        """[(region index, sorted list of live triplets)] of the taken regions; clears their flags"""
        out = []
        for r in range(len(self.keys)):
            if force_all or self.dirty[r]:
                out.append((r, sorted(self.sets[r])))
                self.dirty[r] = False
        return out
