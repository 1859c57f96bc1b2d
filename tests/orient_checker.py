"""The Orientation rule of include/immesh_topology.h in numpy: np.unique on the edge keys for the edges with two uses, a breadth-first search with
parity over them, the modes as loops.  orient(vtx, faces, mode, viewpoint) -> dict with every output of the device calls.  The soups the topology
checker lacks live here too: the Klein bottle, random flips, appended Moebius bands."""
from collections import deque

import numpy as np

import topology_checker as tc

ORIENT_FIRST, ORIENT_FEWEST, ORIENT_VIEWPOINT = 0, 1, 2
MODES = (ORIENT_FIRST, ORIENT_FEWEST, ORIENT_VIEWPOINT)
STAT_NAMES = ("n_patches", "n_orientable", "n_nonorientable", "largest_patch_faces", "n_faces_flipped", "n_faces_nonorientable", "n_patches_inverted",
              "n_inconsistent_before", "n_inconsistent_after")
TABLES = ("first_face", "n_faces", "orientable", "n_flipped", "n_inconsistent")


def pairs(faces):
    """the edges with exactly two uses by counting faces -> (f, g, disagree) arrays, and the mask of counting faces"""
    F = np.asarray(faces, np.int64).reshape(-1, 3)
    counting = (F[:, 0] != F[:, 1]) & (F[:, 1] != F[:, 2]) & (F[:, 0] != F[:, 2]) if len(F) else np.zeros(0, bool)
    cf = np.nonzero(counting)[0]
    a, b = F[cf][:, [0, 1, 2]].reshape(-1), F[cf][:, [1, 2, 0]].reshape(-1)
    key = (np.minimum(a, b) << 32) | np.maximum(a, b)
    forward, face_of = a < b, np.repeat(cf, 3)
    uniq, uses = np.unique(key, return_counts=True)
    order = np.argsort(key, kind="stable")
    start = np.concatenate([[0], np.cumsum(uses)])[:-1].astype(np.int64)
    two = start[uses == 2]
    h0, h1 = order[two], order[two + 1]
    return face_of[h0], face_of[h1], (forward[h0] == forward[h1]).astype(np.int64), counting


def view_sign(vtx, faces, o):
    """s per face about the viewpoint o: float64, in the order the contract writes"""
    V = np.asarray(vtx, np.float32).reshape(-1, 3)
    F = np.asarray(faces, np.int64).reshape(-1, 3)
    o = np.asarray(o, np.float64).reshape(3)
    with np.errstate(all="ignore"):
        a, b, c = (V[F[:, k]].astype(np.float64) - o for k in range(3))
        u, w, ma = b - a, c - a, -a
        n = np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], axis=-1)
        t = (n[:, 0] * ma[:, 0] + n[:, 1] * ma[:, 1]) + n[:, 2] * ma[:, 2]
    s = np.where(t > 0, 1, np.where(t < 0, -1, 0))
    finite = np.isfinite(V[F]).all(axis=(1, 2)) if len(F) else np.zeros(0, bool)
    zero_area = (n == 0).all(axis=1)
    return np.where(finite & ~zero_area, s, 0).astype(np.int64)


def partition(faces):
    """the part of the rule no mode touches: the patches, their bases and whether they are orientable, by a breadth-first search with parity"""
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    nf = len(faces)
    f, g, d, counting = pairs(faces)
    adj = [[] for _ in range(nf)]
    for x, y, z in zip(f.tolist(), g.tolist(), d.tolist()):
        adj[x].append((y, z))
        adj[y].append((x, z))
    label, base = [-1] * nf, [0] * nf
    orientable = {}
    for seed in np.nonzero(counting)[0].tolist():             # ascending: a patch is first met at its smallest face
        if label[seed] >= 0:
            continue
        label[seed], ok, todo = seed, True, deque([seed])
        while todo:
            x = todo.popleft()
            for y, z in adj[x]:
                if label[y] < 0:
                    label[y], base[y] = seed, base[x] ^ z
                    todo.append(y)
                elif base[y] != base[x] ^ z:
                    ok = False
        orientable[seed] = ok
    firsts = sorted(orientable)
    number = {l: i for i, l in enumerate(firsts)}
    patch = np.array([number[l] if l >= 0 else -1 for l in label], np.int32)
    return f, d, counting, np.array(base, np.int64), orientable, firsts, patch


def orient(vtx, faces, mode=ORIENT_FIRST, viewpoint=None, part=None):
    """part: partition(faces), when several modes are asked of one soup"""
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    nf = len(faces)
    f, d, counting, base, orientable, firsts, patch = partition(faces) if part is None else part
    n_p = len(firsts)
    s = view_sign(vtx, faces, viewpoint) if mode == ORIENT_VIEWPOINT else np.zeros(nf, np.int64)
    vote = np.where(base == 1, -s, s)
    cf, pc = np.nonzero(counting)[0], patch[counting]

    def per_patch(mask):                                      # the number of counting faces with mask, per patch
        return np.bincount(pc[mask[cf]], minlength=n_p).astype(np.int64)

    ori = np.array([1 if orientable[l] else 0 for l in firsts], np.int32)
    if n_p:
        base = np.where((patch >= 0) & (ori[patch] == 1), base, 0)   # a non-orientable patch has no base
    n_faces = per_patch(np.ones(nf, bool))
    b1 = per_patch(base == 1)
    if mode == ORIENT_FEWEST:
        inv = 2 * b1 > n_faces
    elif mode == ORIENT_VIEWPOINT:
        inv = per_patch(vote < 0) > per_patch(vote > 0)
    else:
        inv = np.zeros(n_p, bool)
    inv = inv & (ori == 1)
    flip = np.zeros(nf, np.int8)
    flip[cf] = np.where(ori[pc] == 1, base[cf] ^ inv[pc].astype(np.int64), 0)
    n_flipped = per_patch(flip != 0).astype(np.int32)
    n_inc = np.bincount(patch[f][d == 1], minlength=n_p).astype(np.int32)
    n_faces, inverted = n_faces.astype(np.int32), int(inv.sum())
    out = faces.copy()
    out[flip != 0] = faces[flip != 0][:, [0, 2, 1]]
    st = {"n_patches": n_p, "n_orientable": int(ori.sum()), "n_nonorientable": n_p - int(ori.sum()), "largest_patch_faces": int(n_faces.max()) if n_p else 0,
          "n_faces_flipped": int(flip.sum()), "n_faces_nonorientable": int(n_faces[ori == 0].sum()), "n_patches_inverted": inverted,
          "n_inconsistent_before": int(d.sum()), "n_inconsistent_after": int(n_inc[ori == 0].sum())}
    return {"stats": st, "patch": patch, "flip": flip, "faces": out, "base": base.astype(np.int8), "first_face": np.array(firsts, np.int32), "n_faces": n_faces,
            "orientable": ori, "n_flipped": n_flipped, "n_inconsistent": n_inc}


# ---- soups ---------------------------------------------------------------------------------------------------------------------------------------
def klein(m, n):
    """the torus' grid with the wrap in i joined flipped (j -> -j): closed, one patch, non-orientable.  m, n >= 3."""
    i, j = np.meshgrid(np.arange(m), np.arange(n), indexing="ij")
    th, ph = 2 * np.pi * i / m, 2 * np.pi * j / n
    vtx = np.stack([(2 + np.cos(ph)) * np.cos(th), (2 + np.cos(ph)) * np.sin(th), np.sin(ph)], axis=-1).reshape(-1, 3).astype(np.float32)
    i, j = i.reshape(-1), j.reshape(-1)

    def v(a, b):
        b = np.where(a >= m, -b, b)
        return (a % m) * n + (b % n)

    faces = np.stack([np.stack([v(i, j), v(i + 1, j), v(i + 1, j + 1)], axis=-1), np.stack([v(i, j), v(i + 1, j + 1), v(i, j + 1)], axis=-1)], axis=1)
    return vtx, faces.reshape(-1, 3).astype(np.int32)


def flip_random(rng, faces, share=0.5):
    """a random subset of the faces with their last two indices swapped -> (faces, the mask)"""
    faces = np.asarray(faces, np.int32).reshape(-1, 3).copy()
    mask = rng.random(len(faces)) < share
    faces[mask] = faces[mask][:, [0, 2, 1]]
    return faces, mask


def with_moebius(vtx, faces, cells=(9,), offset=100.0):
    """the soup with Moebius bands of the given numbers of cells appended, each on vertices of its own, far away"""
    vs, fs, base = [np.asarray(vtx, np.float32).reshape(-1, 3)], [np.asarray(faces, np.int32).reshape(-1, 3)], len(vtx)
    for k, n in enumerate(cells):
        v, f = tc.moebius(n)
        vs.append((v + np.float32(offset * (k + 1))).astype(np.float32))
        fs.append(f + base)
        base += len(v)
    return np.concatenate(vs).astype(np.float32), np.concatenate(fs).astype(np.int32)
