"""numpy restatement of the alignment contract (include/immesh_align.h): the correspondences by brute force through closest_checker.closest (every
point against every face, no hierarchy), the rows and the 28 terms per point with every double operation in the header's order (element by element
over the points: numpy does not fuse multiply-adds, so the terms are bit-identical to the kernels'), the system by math.fsum (the exact sums,
correctly rounded), and the solve, Exp, the update and the loop in Python floats, statement by statement as the header writes them."""
import math

import numpy as np

import closest_checker as cc

POINT, PLANE = 0, 1
CONVERGED, MAX_ITERS, TOO_FEW, DEGENERATE = 0, 1, 2, 3
N_TERMS = 28


def h_index(a, b):
    return a * (13 - a) // 2 + (b - a)


def correspondences(rot, pos, pts, max_dist, vtx, faces):
    """-> p (n, 3), ok (n,), face (n,) int32 (-1: none), q (n, 3), A (n, 3 corners, 3) relative to p (zeros without a face)"""
    p, ok = cc.points(rot, pos, pts)
    _, _, face, _, _ = cc.closest(rot, pos, pts, max_dist, vtx, faces)
    n = len(p)
    q, A = np.zeros((n, 3)), np.zeros((n, 3, 3))
    have = np.nonzero(face >= 0)[0]
    if len(have):
        vtx = np.asarray(vtx, np.float32).reshape(-1, 3)
        tri = vtx[np.asarray(faces, np.int64).reshape(-1, 3)[face[have]]]
        q[have] = cc.pair(p[have], tri)[1]
        A[have] = tri.astype(np.float64) - p[have][:, None, :]
    return p, ok, face, q, A


def _row(x, u, r, t):
    """one row (j, r), j = (cross(x, u), u), added to the terms t (None: the row that begins the sums) -> t"""
    j = np.concatenate([cc._cross(x, u), u], axis=-1)
    new = np.empty((len(x), N_TERMS))
    for a in range(6):
        for b in range(a, 6):
            new[:, h_index(a, b)] = j[:, a] * j[:, b]
        new[:, 21 + a] = j[:, a] * r
    new[:, 27] = r * r
    return new if t is None else t + new


def terms(mode, p, centre, face, q, A):
    """-> terms (n, 28) (zeros for a point that does not take part), used (n,) bool, flat (n,) bool"""
    n = len(p)
    out = np.zeros((n, N_TERMS))
    have = face >= 0
    flat = np.zeros(n, bool)
    idx = np.nonzero(have)[0]
    if len(idx) == 0:
        return out, have.copy(), flat
    x = p[idx] - np.asarray(centre, np.float64).reshape(3)
    if mode == POINT:
        t = None
        for k in range(3):
            u = np.zeros((len(idx), 3))
            u[:, k] = 1.0
            t = _row(x, u, q[idx, k], t)
        out[idx] = t
        return out, have.copy(), flat
    a, b, c = A[idx, 0], A[idx, 1], A[idx, 2]
    ab, ac = b - a, c - a
    nrm = cc._cross(ab, ac)
    with np.errstate(all="ignore"):
        nn = cc._dot(nrm, nrm)
        good = np.isfinite(nn) & (nn > 0)
        s = np.sqrt(np.where(good, nn, 1.0))
        u = nrm / s[:, None]
        t = _row(x, u, cc._dot(u, a), None)
    out[idx[good]] = t[good]
    flat[idx[~good]] = True
    return out, have & ~flat, flat


def system(tm, ok, face, used, flat):
    """the System rule -> (sums (28,) by math.fsum, bound (28,) = the sum of |term|, counts (n_used, n_not_finite, n_no_face, n_flat))"""
    sums = np.array([math.fsum(tm[:, k].tolist()) for k in range(N_TERMS)])
    bound = np.array([math.fsum(np.abs(tm[:, k]).tolist()) for k in range(N_TERMS)])
    return sums, bound, (int(used.sum()), int((~ok).sum()), int((ok & (face < 0)).sum()), int(flat.sum()))


def step(rot, pos, pts, mode, max_dist, centre, vtx, faces):
    """one step -> dict: face, terms, sums, bound, counts"""
    p, ok, face, q, A = correspondences(rot, pos, pts, max_dist, vtx, faces)
    tm, used, flat = terms(mode, p, centre, face, q, A)
    sums, bound, counts = system(tm, ok, face, used, flat)
    return {"face": face, "terms": tm, "sums": sums, "bound": bound, "counts": counts}


def solve(sums, damping):
    """the Solve rule on the 28 sums -> (degenerate, delta (6,))"""
    H, g = [float(v) for v in sums[:21]], [float(v) for v in sums[21:27]]
    A = [[H[h_index(min(a, b), max(a, b))] for b in range(6)] for a in range(6)]
    for a in range(6):
        A[a][a] = A[a][a] + float(damping)
    m = A[0][0]
    for a in range(1, 6):
        if A[a][a] > m:
            m = A[a][a]
    L = [[0.0] * 6 for _ in range(6)]
    for j in range(6):
        s = A[j][j]
        for k in range(j):
            s = s - L[j][k] * L[j][k]
        if not math.isfinite(s) or s <= 0.0 or s <= 2.0 ** -40 * m:
            return True, np.zeros(6)
        L[j][j] = math.sqrt(s)
        for i in range(j + 1, 6):
            t = A[i][j]
            for k in range(j):
                t = t - L[i][k] * L[j][k]
            L[i][j] = t / L[j][j]
    y, d = [0.0] * 6, [0.0] * 6
    for i in range(6):
        t = g[i]
        for k in range(i):
            t = t - L[i][k] * y[k]
        y[i] = t / L[i][i]
    for i in range(5, -1, -1):
        t = y[i]
        for k in range(i + 1, 6):
            t = t - L[k][i] * d[k]
        d[i] = t / L[i][i]
    return False, np.array(d)


def exp(w):
    """the Exp rule -> (3, 3)"""
    w = [float(v) for v in w]
    K = [[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]]
    th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
    th = math.sqrt(th2)
    E = np.zeros((3, 3))
    if th < 2.0 ** -26:
        for i in range(3):
            for j in range(3):
                E[i, j] = (1.0 if i == j else 0.0) + K[i][j]
        return E
    a = math.sin(th) / th
    h = math.sin(0.5 * th)
    b = (2.0 * (h * h)) / th2
    for i in range(3):
        for j in range(3):
            kk = (K[i][0] * K[0][j] + K[i][1] * K[1][j]) + K[i][2] * K[2][j]
            E[i, j] = ((1.0 if i == j else 0.0) + a * K[i][j]) + b * kk
    return E


def update(rot, pos, centre, delta):
    """the Update rule -> rot' (3, 3), pos' (3,)"""
    E = exp(delta[:3]).tolist()
    R = np.asarray(rot, np.float64).reshape(3, 3).tolist()
    t, ce, v = [float(x) for x in pos], [float(x) for x in centre], [float(x) for x in delta[3:]]
    R2 = [[(E[i][0] * R[0][j] + E[i][1] * R[1][j]) + E[i][2] * R[2][j] for j in range(3)] for i in range(3)]
    d = [t[k] - ce[k] for k in range(3)]
    t2 = [(((E[i][0] * d[0] + E[i][1] * d[1]) + E[i][2] * d[2]) + ce[i]) + v[i] for i in range(3)]
    return np.array(R2), np.array(t2)


def _sum(tm, summation):
    if summation == "fsum":
        return np.array([math.fsum(tm[:, k].tolist()) for k in range(N_TERMS)])
    if len(tm) == 0:
        return np.zeros(N_TERMS)
    return np.add.accumulate(tm if summation == "ascending" else tm[::-1], axis=0)[-1]     # one addition after the other, in point order


def loop(rot, pos, pts, mode, max_dist, centre, damping, max_iters, eps_rot, eps_trans, vtx, faces, summation="fsum"):
    """the Loop rule -> dict: rot, pos, status, iterations, history (iterations, 4), rms.  summation: "fsum", or the terms added one after the other
    in "ascending" / "descending" point order (any fixed order is within the contract's bound)"""
    rot = np.eye(3) if rot is None else np.asarray(rot, np.float64).reshape(3, 3)
    pos = np.zeros(3) if pos is None else np.asarray(pos, np.float64).reshape(3)
    need = 6 if mode == PLANE else 3
    status, hist, rms, it = MAX_ITERS, [], 0.0, 0
    for it in range(max_iters):
        p, ok, face, q, A = correspondences(rot, pos, pts, max_dist, vtx, faces)
        tm, used, flat = terms(mode, p, centre, face, q, A)
        sums = _sum(tm, summation)
        n_used = int(used.sum())
        rows = n_used if mode == PLANE else 3 * n_used
        rms = math.sqrt(sums[27] / rows) if rows > 0 else 0.0
        nw = nv = 0.0
        stop = False
        if n_used < need:
            status, stop = TOO_FEW, True
        else:
            bad, delta = solve(sums, damping)
            if bad:
                status, stop = DEGENERATE, True
            else:
                rot, pos = update(rot, pos, centre, delta)
                d = delta.tolist()
                nw = math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
                nv = math.sqrt((d[3] * d[3] + d[4] * d[4]) + d[5] * d[5])
                if nw <= eps_rot and nv <= eps_trans:
                    status, stop = CONVERGED, True
        hist.append([float(n_used), rms, nw, nv])
        if stop:
            break
    return {"rot": rot, "pos": pos, "status": status, "iterations": it + 1 if max_iters > 0 else 0, "history": np.array(hist).reshape(-1, 4), "rms": rms}


# ---- the convergence case of the tests ------------------------------------------------------------------------------------------------------------
def bumpy_sheet(n=24, size=6.0, amp=0.3):
    """z = amp sin(x) cos(1.3 y) on an n x n grid of vertices over [0, size]^2 -> vtx (n n, 3) float32, faces (2 (n - 1)^2, 3) int32"""
    g = np.linspace(0.0, size, n)
    X, Y = np.meshgrid(g, g, indexing="ij")
    vtx = np.stack([X, Y, amp * np.sin(X) * np.cos(1.3 * Y)], axis=-1).reshape(-1, 3).astype(np.float32)
    faces = []
    for i in range(n - 1):
        for j in range(n - 1):
            a, b, c, d = i * n + j, (i + 1) * n + j, (i + 1) * n + j + 1, i * n + j + 1
            faces += [(a, b, c), (a, c, d)]
    return vtx, np.array(faces, np.int32)


def sample_on_faces(vtx, faces, n_pts, seed):
    """n_pts points on random faces by barycentric weights from a seeded generator, in float64"""
    rng = np.random.default_rng(seed)
    tri = vtx[faces[rng.integers(len(faces), size=n_pts)]].astype(np.float64)
    w = rng.dirichlet(np.ones(3), size=n_pts)
    return (tri * w[:, :, None]).sum(axis=1)


def rodrigues(axis, angle):
    """an independent rotation matrix (the closed form with cos), for the tests' known poses"""
    k = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1.0 - math.cos(angle)) * (K @ K)


TRUE_ROT = rodrigues([1.0, 2.0, 3.0], math.radians(3.0))
TRUE_POS = np.array([0.05, -0.03, 0.04])


def convergence_case(n_pts=4000, seed=7):
    """the sheet and a cloud on its faces moved by the inverse of the known pose (TRUE_ROT, TRUE_POS), stored as floats: aligning the cloud from the
    identity recovers that pose -> vtx, faces, cloud (n_pts, 3) float32"""
    vtx, faces = bumpy_sheet()
    world = sample_on_faces(vtx, faces, n_pts, seed)
    return vtx, faces, ((world - TRUE_POS) @ TRUE_ROT).astype(np.float32)               # x = R^T (w - t): R x + t = w
