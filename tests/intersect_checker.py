"""Two restatements of the contract in include/immesh_intersect.h, in numpy.  They share the segment test `hit` and nothing else:

  brute(vtx, faces)   every i < j: a loop over i, the closed box test against all j > i, then the masks case by case (sets for the shared indices)
  grid(vtx, faces)    candidates from a uniform grid over the boxes (a face in every cell its box touches, pairs of one cell, the exact box test),
                      the shared indices from an index comparison table, all six bits computed and the rule's bits selected

Both return {"stats": dict, "pairs": (n, 2) int32 ascending, "mask": (n,) uint8, "n_partners": (n_faces,) int32, "face_map": (n_faces,) int32,
"kept": the kept faces}.  Soups for the tests stand below them."""
import numpy as np

STAT_NAMES = ("n_faces", "n_in_tree", "n_taking_part", "n_candidates", "n_share", "n_pairs", "n_pairs_share0", "n_pairs_share1", "n_faces_hit",
              "max_partners")
CAP = 1 << 24


def _cross(p, q):
    return np.stack([p[..., 1] * q[..., 2] - p[..., 2] * q[..., 1], p[..., 2] * q[..., 0] - p[..., 0] * q[..., 2],
                     p[..., 0] * q[..., 1] - p[..., 1] * q[..., 0]], axis=-1)


def _dot(p, q):
    return (p[..., 0] * q[..., 0] + p[..., 1] * q[..., 1]) + p[..., 2] * q[..., 2]


def hit(p, q, T):
    """the Segment rule: p, q (..., 3) float32, T (..., 3, 3) float32 -> bool (...)"""
    o = p.astype(np.float64); d = q.astype(np.float64) - o
    a, b, c = (T[..., k, :].astype(np.float64) - o for k in range(3))
    e = np.stack([_dot(_cross(a, b), d), _dot(_cross(b, c), d), _dot(_cross(c, a), d)], axis=-1)
    n = _cross(b - a, c - a); na = _dot(n, a); nd = _dot(n, d)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        s = na / nd
    return ((e >= 0).all(-1) | (e <= 0).all(-1)) & (nd != 0) & (s >= 0) & (s <= 1)


def taking_part(vtx, faces):
    """-> (in the tree, takes part), bool per face"""
    vtx = np.asarray(vtx, np.float32).reshape(-1, 3); faces = np.asarray(faces, np.int32).reshape(-1, 3)
    in_tree = np.isfinite(vtx[faces]).all(axis=(1, 2)) if len(faces) else np.zeros(0, bool)
    counting = (faces[:, 0] != faces[:, 1]) & (faces[:, 1] != faces[:, 2]) & (faces[:, 0] != faces[:, 2])
    return in_tree, in_tree & counting


def _boxes(vtx, faces):
    with np.errstate(invalid="ignore"):
        tri = vtx[faces]
        return tri.min(axis=1), tri.max(axis=1)


def _result(vtx, faces, in_tree, take, n_share, I, J, mask, sh):
    nf = len(faces)
    on = mask != 0
    I, J, mask, sh = I[on], J[on], mask[on], sh[on]
    order = np.lexsort((J, I))
    I, J, mask, sh = I[order], J[order], mask[order], sh[order]
    n_partners = (np.bincount(I, minlength=nf) + np.bincount(J, minlength=nf)).astype(np.int32)
    keep = n_partners == 0
    face_map = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32)
    stats = dict(n_faces=nf, n_in_tree=int(in_tree.sum()), n_taking_part=int(take.sum()), n_candidates=int(sum(n_share)), n_share=[int(x) for x in n_share],
                 n_pairs=len(I), n_pairs_share0=int((sh == 0).sum()), n_pairs_share1=int((sh == 1).sum()), n_faces_hit=int((~keep).sum()),
                 max_partners=int(n_partners.max()) if nf else 0)
    return {"stats": stats, "pairs": np.stack([I, J], axis=-1).astype(np.int32).reshape(-1, 2), "mask": mask.astype(np.uint8), "n_partners": n_partners,
            "face_map": face_map, "kept": faces[keep]}


# ---- the brute force -------------------------------------------------------------------------------------------------------------------------------------
def brute(vtx, faces):
    vtx = np.asarray(vtx, np.float32).reshape(-1, 3); faces = np.asarray(faces, np.int32).reshape(-1, 3)
    in_tree, take = taking_part(vtx, faces)
    lo, hi = _boxes(vtx, faces)
    ci, cj = [], []
    for i in np.nonzero(take)[0]:
        later = take[i + 1:] & (lo[i] <= hi[i + 1:]).all(axis=1) & (lo[i + 1:] <= hi[i]).all(axis=1)
        j = np.nonzero(later)[0] + i + 1
        ci.append(np.full(len(j), i)); cj.append(j)
    I = np.concatenate(ci) if ci else np.zeros(0, np.int64)
    J = np.concatenate(cj) if cj else np.zeros(0, np.int64)
    I, J = I.astype(np.int64), J.astype(np.int64)
    mask = np.zeros(len(I), np.int64)
    sh = np.array([len(set(faces[i].tolist()) & set(faces[j].tolist())) for i, j in zip(I, J)], np.int64).reshape(-1)
    A, B = vtx[faces[I]], vtx[faces[J]]
    zero = np.nonzero(sh == 0)[0]
    for k in range(3):
        mask[zero] |= hit(A[zero, k], A[zero, (k + 1) % 3], B[zero]).astype(np.int64) << k
        mask[zero] |= hit(B[zero, k], B[zero, (k + 1) % 3], A[zero]).astype(np.int64) << (3 + k)
    for c in np.nonzero(sh == 1)[0]:                                                    # one pair at a time: the edge that does not name the shared vertex
        fa, fb = faces[I[c]].tolist(), faces[J[c]].tolist()
        v = (set(fa) & set(fb)).pop()
        for half, (own, other, tri) in enumerate(((fa, A[c], B[c]), (fb, B[c], A[c]))):
            for k in range(3):
                if v not in (own[k], own[(k + 1) % 3]) and hit(other[k], other[(k + 1) % 3], tri):
                    mask[c] |= 1 << (3 * half + k)
    return _result(vtx, faces, in_tree, take, np.bincount(sh, minlength=4)[:4], I, J, mask, sh)


# ---- the grid --------------------------------------------------------------------------------------------------------------------------------------------
def grid_candidates(lo, hi, ids):
    """the pairs i < j of `ids` whose boxes overlap, closed, by a uniform grid -> I, J (unordered)"""
    if len(ids) < 2:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    lo, hi = lo[ids].astype(np.float64), hi[ids].astype(np.float64)
    origin, top = lo.min(axis=0), hi.max(axis=0)
    cell = np.maximum(np.maximum(2.0 * (hi - lo).mean(axis=0), (top - origin) / 128.0), 1e-300)
    c0 = np.floor((lo - origin) / cell).astype(np.int64); c1 = np.floor((hi - origin) / cell).astype(np.int64)
    span = c1 - c0 + 1
    per = span.prod(axis=1)
    owner = np.repeat(np.arange(len(ids)), per)
    rank = np.arange(per.sum()) - np.repeat(np.cumsum(per) - per, per)
    sx, sy = span[owner, 0], span[owner, 1]
    cx = c0[owner, 0] + rank % sx; cy = c0[owner, 1] + (rank // sx) % sy; cz = c0[owner, 2] + rank // (sx * sy)
    key = (cx * 1024 + cy) * 1024 + cz                                                  # at most 129 cells per axis
    order = np.argsort(key, kind="stable")
    key, owner = key[order], owner[order]
    out = []
    d = 1
    while d < len(key):
        same = key[d:] == key[:-d]
        if not same.any():
            break
        out.append(np.stack([owner[:-d][same], owner[d:][same]], axis=-1))
        d += 1
    if not out:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    pr = np.concatenate(out)
    pr = np.unique(np.sort(pr, axis=1), axis=0)                                         # a pair shares many cells
    a, b = pr[:, 0], pr[:, 1]
    ok = (lo[a] <= hi[b]).all(axis=1) & (lo[b] <= hi[a]).all(axis=1)
    return ids[a[ok]].astype(np.int64), ids[b[ok]].astype(np.int64)


def grid(vtx, faces):
    vtx = np.asarray(vtx, np.float32).reshape(-1, 3); faces = np.asarray(faces, np.int32).reshape(-1, 3)
    in_tree, take = taking_part(vtx, faces)
    lo, hi = _boxes(vtx, faces)
    I, J = grid_candidates(lo, hi, np.nonzero(take)[0])
    fa, fb = faces[I], faces[J]
    eq = fa[:, :, None] == fb[:, None, :]
    sh = eq.sum(axis=(1, 2))
    ka, kb = eq.any(axis=2).argmax(axis=1), eq.any(axis=1).argmax(axis=1)
    A, B = vtx[fa], vtx[fb]
    bits = np.stack([hit(A[:, k], A[:, (k + 1) % 3], B) for k in range(3)] + [hit(B[:, k], B[:, (k + 1) % 3], A) for k in range(3)], axis=-1)
    allowed = np.zeros((len(I), 6), bool)
    allowed[sh == 0] = True
    one = np.nonzero(sh == 1)[0]
    allowed[one, (ka[one] + 1) % 3] = True
    allowed[one, 3 + (kb[one] + 1) % 3] = True
    mask = ((bits & allowed) * (1 << np.arange(6))).sum(axis=1).astype(np.int64)
    return _result(vtx, faces, in_tree, take, np.bincount(sh, minlength=4)[:4], I, J, mask, sh)


def same(got, ref, what=""):
    """every output bit for bit"""
    assert got["stats"] == ref["stats"], (what, got["stats"], ref["stats"])
    for k in ("pairs", "mask", "n_partners", "face_map"):
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape and got[k].tobytes() == ref[k].tobytes(), (what, k)


def both(vtx, faces, what=""):
    """the two checkers on one soup, equal -> the result"""
    a, b = grid(vtx, faces), brute(vtx, faces)
    same(a, b, what)
    assert np.array_equal(a["kept"], b["kept"])
    return a


# ---- soups -----------------------------------------------------------------------------------------------------------------------------------------------
def sheet(m, n, z=None, scale=1.0, origin=(0.0, 0.0, 0.0)):
    """an m x n grid of cells, two faces each, over shared vertices; z: a function of the (x, y) arrays"""
    i, j = np.meshgrid(np.arange(m + 1), np.arange(n + 1), indexing="ij")
    x, y = origin[0] + scale * i, origin[1] + scale * j
    zz = np.full(x.shape, origin[2]) if z is None else origin[2] + z(x, y)
    vtx = np.stack([x, y, zz], axis=-1).reshape(-1, 3).astype(np.float32)
    ci, cj = (a.reshape(-1) for a in np.meshgrid(np.arange(m), np.arange(n), indexing="ij"))
    v00, v10, v01, v11 = ci * (n + 1) + cj, (ci + 1) * (n + 1) + cj, ci * (n + 1) + cj + 1, (ci + 1) * (n + 1) + cj + 1
    faces = np.stack([np.stack([v00, v10, v11], axis=-1), np.stack([v00, v11, v01], axis=-1)], axis=1).reshape(-1, 3).astype(np.int32)
    return vtx, faces


def join(*soups):
    vtx, faces, base = [], [], 0
    for v, f in soups:
        vtx.append(np.asarray(v, np.float32).reshape(-1, 3)); faces.append(np.asarray(f, np.int32).reshape(-1, 3) + base)
        base += len(vtx[-1])
    return np.concatenate(vtx), np.concatenate(faces).astype(np.int32)


def noisy(rng, amp):
    return lambda x, y: rng.normal(scale=amp, size=x.shape)


def crossing_sheets(rng, m, n, noise=0.02, slope=0.37):
    """a noisy sheet about z = 0 and a second one tilted through it (vertices of its own), 4 m n faces in all"""
    a = sheet(m, n, noisy(rng, noise))
    b = sheet(m, n, lambda x, y: slope * (x - 0.5 * m + 0.21) + rng.normal(scale=noise, size=x.shape), origin=(0.13, 0.29, 0.0))
    return join(a, b)


def jittered_sheet(rng, m, n, amp=0.7, height=0.5):
    """a rough sheet whose vertices are moved in x and y by up to amp of a cell: faces fold through their neighbours and their neighbours' neighbours"""
    vtx, faces = sheet(m, n, noisy(rng, height))
    vtx[:, :2] += rng.uniform(-amp, amp, (len(vtx), 2)).astype(np.float32)
    return vtx, faces


def unshared(vtx, faces):
    faces = np.asarray(faces, np.int32)
    return np.asarray(vtx, np.float32)[faces].reshape(-1, 3), np.arange(3 * len(faces), dtype=np.int32).reshape(-1, 3)


def big_and_small(n_hit, n_near, rng=None):
    """face 0: a large face in z = 0 over the lower-left half of the square [0, 128]^2; then n_hit small upright faces that cross it and n_near that cross
    z = 0 inside its box but outside the face: n_hit + n_near candidates (the small ones stand apart), n_hit pairs, all with face 0"""
    assert n_hit <= 400 and n_near <= 300
    vtx = [[0.0, 0.0, 0.0], [128.0, 0.0, 0.0], [0.0, 128.0, 0.0]]
    faces = [[0, 1, 2]]
    spots = [(1.0 + 2 * (k % 20), 1.0 + 2 * (k // 20)) for k in range(n_hit)]           # x + y < 80: inside the face
    spots += [(127.0 - 2 * (k % 20), 127.0 - 2 * (k // 20)) for k in range(n_near)]      # x + y > 180: outside it, inside its box
    for x, y in spots:
        b = len(vtx)
        vtx += [[x, y, -0.5], [x + 0.5, y + 0.25, -0.5], [x + 0.25, y + 0.125, 0.75]]
        faces.append([b, b + 1, b + 2])
    vtx, faces = np.array(vtx, np.float32), np.array(faces, np.int32)
    if rng is not None:
        p = rng.permutation(len(faces))
        faces = faces[p]
    return vtx, faces


def crossing_strips(n):
    """n faces: a flat strip along x and an upright strip that crosses it along the same line, the faces split between them"""
    na = (n + 1) // 2
    a = sheet((na + 1) // 2, 1, origin=(0.0, -0.5, 0.0))
    b = sheet((n - na + 1) // 2, 1, origin=(0.25, 0.0, -0.5)) if n > na else (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    bv = b[0].copy()
    if len(bv):
        bv[:, [1, 2]] = np.stack([np.full(len(bv), 0.0625), b[0][:, 1] - 0.5], axis=-1)   # y -> z: the strip stands in the plane y = 1 / 16
    vtx, faces = join((a[0], a[1][:na]), (bv, b[1][:n - na]))
    return vtx, faces


# two faces that share vertex 0; the far edge of the first (1 -> 2) passes through the second, inside the fan of the shared vertex
FAN_VTX = np.array([[0, 0, 0], [2, 1, 1], [2, 1, -1], [3, 0, 0], [3, 3, 0], [2, -1, -1]], np.float32)
FAN_PIERCED = np.array([[0, 1, 2], [0, 3, 4]], np.int32)                                # the segment (2, 1, +-1) crosses z = 0 at (2, 1): inside (0, 3, 4)
FAN_NOT_PIERCED = np.array([[0, 5, 2], [0, 3, 4]], np.int32)                            # the first face lies below z = 0 and meets it in vertex 0 alone
# two faces without a common vertex, both ways a crossing in general position ends: an edge of each in the other (bits 1 and 3), and two edges of the
# second in the first (bits 3 and 5)
CROSS_VTX = np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0], [1, 1, -1], [1, 1, 1], [5, 5, 0.5], [1.5, 1, 1], [1, 1.5, 1]], np.float32)
CROSS_ONE_EACH = np.array([[0, 1, 2], [3, 4, 5]], np.int32)
CROSS_TWO_OF_B = np.array([[0, 1, 2], [3, 6, 7]], np.int32)


def rotate_mask(mask, ra, rb):
    """the mask of (A, B) after A's indices were rotated left by ra and B's by rb: edge k of the rotated face is edge (k + r) mod 3 of the face"""
    out = 0
    for k in range(3):
        out |= ((mask >> ((k + ra) % 3)) & 1) << k
        out |= ((mask >> (3 + (k + rb) % 3)) & 1) << (3 + k)
    return out


def swap_mask(mask):
    """the mask of (B, A)"""
    return ((mask & 7) << 3) | (mask >> 3)
