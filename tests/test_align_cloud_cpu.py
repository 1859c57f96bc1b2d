"""The Cloud rule's checker (tests/align_cloud_checker.py) against itself, without a device: hand-made cases worked out by hand, the sign invariance
of the PLANE terms, the huber boundary d == huber, and its loop recovering a known motion within the bound the device test asks of the library."""
import math

import numpy as np

import align_checker as ac
import align_cloud_checker as acc


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def test_winner_q_and_point_terms_by_hand():
    cloud = np.array([[1, 0, 0], [0, 2, 0], [np.nan, 0, 0], [5, 5, 5]], np.float32)
    pts = np.array([[0, 0, 0], [0, 1.5, 0], [9, 9, 9], [np.inf, 0, 0], [0.5, 1, 0]], np.float32)
    s = acc.step(None, None, pts, acc.POINT, 2.0, np.zeros(3), cloud)
    assert s["index"].tolist() == [0, 1, -1, -1, 0]                                      # the last one: D = 1.25 to both, the smaller index wins
    assert s["counts"] == (3, 1, 1, 0)
    t = s["terms"][0]                                                                   # x = 0, q = (1, 0, 0): H = diag(0, 0, 0, 1, 1, 1), g = (0, 0, 0, 1, 0, 0)
    assert [t[ac.h_index(a, a)] for a in range(6)] == [0, 0, 0, 1, 1, 1] and t[21:27].tolist() == [0, 0, 0, 1, 0, 0] and t[27] == 1.0
    t = s["terms"][1]                                                                   # x = (0, 1.5, 0), q = (0, 0.5, 0): e = 0.25, g_v = q, g_omega = cross(x, q) = 0
    assert t[27] == 0.25 and t[21:27].tolist() == [0, 0, 0, 0, 0.5, 0]
    assert not s["terms"][2:4].any()
    assert s["sums"][27] == 1.0 + 0.25 + 1.25


def test_frame_centre_and_empty_cloud():
    rot, pos = ac.rodrigues([0, 0, 1], math.pi / 2), np.array([1.0, 0.0, 0.0])
    cloud = np.array([[1, 1, 0]], np.float32)
    pts = np.array([[1, 0, 0]], np.float32)                                              # R x + t = (1, 1, 0) up to the rounding of cos(pi / 2)
    s = acc.step(rot, pos, pts, acc.POINT, 0.5, np.array([1.0, 1.0, 0.0]), cloud)
    assert s["index"].tolist() == [0] and s["sums"][27] < 1e-30
    empty = acc.step(None, None, pts, acc.PLANE, 0.5, np.zeros(3), np.zeros((0, 3), np.float32), normal=np.zeros((0, 3)), nstatus=np.zeros(0, np.uint8))
    assert empty["counts"] == (0, 0, 1, 0) and not empty["terms"].any()
    r = acc.loop(None, None, pts, acc.POINT, 0.5, np.zeros(3), 0.0, 5, 1e-9, 1e-9, np.zeros((0, 3), np.float32))
    assert (r["status"], r["iterations"], r["rms"]) == (ac.TOO_FEW, 1, 0.0)


def test_plane_terms_by_hand_statuses_and_sign_invariance():
    rng = np.random.default_rng(5)
    cloud = rng.uniform(-1, 1, (40, 3)).astype(np.float32)
    nrm = rng.normal(size=(40, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1)[:, None]).astype(np.float32)
    nst = np.zeros(40, np.uint8)
    nst[[3, 7, 11]] = [1, 2, 3]
    pts = (cloud.astype(np.float64) + rng.normal(scale=0.01, size=(40, 3))).astype(np.float32)
    centre = np.array([0.1, -0.2, 0.3])
    for huber in (0.0, 0.004):
        a = acc.step(None, None, pts, acc.PLANE, 0.5, centre, cloud, huber, nrm, nst)
        b = acc.step(None, None, pts, acc.PLANE, 0.5, centre, cloud, huber, -nrm, nst)
        flip = nrm * np.where(np.arange(40) % 2, -1, 1)[:, None].astype(np.float32)
        c = acc.step(None, None, pts, acc.PLANE, 0.5, centre, cloud, huber, flip, nst)
        assert a["index"].tolist() == list(range(40)) and a["counts"] == (37, 0, 0, 3)
        assert not a["terms"][[3, 7, 11]].any()
        assert _bits(a["terms"]) == _bits(b["terms"]) == _bits(c["terms"]) and _bits(a["sums"]) == _bits(b["sums"])
    i = 0                                                                               # one row by hand
    a = acc.step(None, None, pts, acc.PLANE, 0.5, centre, cloud, 0.0, nrm, nst)
    p = pts[i].astype(np.float64)
    q, u, x = cloud[i].astype(np.float64) - p, nrm[i].astype(np.float64), p - centre
    r = (u[0] * q[0] + u[1] * q[1]) + u[2] * q[2]
    j = [x[1] * u[2] - x[2] * u[1], x[2] * u[0] - x[0] * u[2], x[0] * u[1] - x[1] * u[0], u[0], u[1], u[2]]
    assert a["terms"][i, 27] == r * r and a["terms"][i, 21:27].tolist() == [v * r for v in j] and a["terms"][i, ac.h_index(1, 4)] == j[1] * j[4]


def test_huber_boundary():
    cloud = np.array([[0, 0, 0]], np.float32)
    nrm, nst = np.array([[0, 0, 1]], np.float32), np.zeros(1, np.uint8)
    pts = np.array([[0.3, 0.4, 0.0], [0.0, 0.0, -0.5], [0.0, 0.0, -1.0]], np.float32)       # POINT: d = sqrt(D) = 0.5 (as floats: close to), 0.5, 1.0
    for mode in (acc.POINT, acc.PLANE):
        plain = acc.step(None, None, pts, mode, 2.0, np.zeros(3), cloud, 0.0, nrm, nst)["terms"]
        at = acc.step(None, None, pts, mode, 2.0, np.zeros(3), cloud, 0.5, nrm, nst)["terms"]
        assert _bits(at[1]) == _bits(plain[1])                                          # d == huber exactly: w = 1.0
        assert _bits(at[2]) == _bits(0.5 * plain[2]) and at[2, 27] == 0.5                # d = 1: w = 0.5 / 1
        below = acc.step(None, None, pts, mode, 2.0, np.zeros(3), cloud, np.nextafter(0.5, 0.0), nrm, nst)["terms"]
        w = np.nextafter(0.5, 0.0) / 0.5
        assert w < 1.0 and _bits(below[1]) == _bits(w * plain[1]) and below[1, 27] < plain[1, 27]
    assert acc.weight(np.array([0.0, 0.5, 2.0]), 0.5).tolist() == [1.0, 1.0, 0.25]


def test_loop_recovers_the_known_motion_within_the_rounding_bound():
    cloud, src, centre = acc.convergence_case()
    nrm, nst = acc.sheet_normals()
    bound = acc.rms_bound(cloud, src)
    assert bound < 2e-6
    for mode in (acc.POINT, acc.PLANE):
        r = acc.loop(None, None, src, mode, acc.SHEET_MAX_DIST, centre, 0.0, 30, 1e-9, 1e-9, cloud, 0.0, nrm, nst)
        assert r["status"] == ac.CONVERGED and r["iterations"] <= 8, (mode, r["status"], r["iterations"])
        assert r["rms"] <= bound < r["history"][0, 1], (mode, r["rms"], bound)
        assert np.abs(r["rot"] - acc.TRUE_ROT).max() < 1e-7 and np.abs(r["pos"] - acc.TRUE_POS).max() < 1e-7
        assert (r["history"][:, 0] == len(src)).all()


def test_cloud_align_tool_reads_and_writes_clouds(tmp_path):
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import cloud_align
    pts = np.random.default_rng(1).uniform(-5, 5, (17, 3)).astype(np.float32)
    for name in ("b.npy", "b.ply"):
        cloud_align.write_cloud(str(tmp_path / name), pts)
        assert _bits(cloud_align.read_cloud(str(tmp_path / name))) == _bits(pts)
    np.save(str(tmp_path / "wide.npy"), np.concatenate([pts.astype(np.float64), np.ones((17, 2))], axis=1))
    assert _bits(cloud_align.read_cloud(str(tmp_path / "wide.npy"))) == _bits(pts)
    with open(str(tmp_path / "a.ply"), "w") as fp:
        fp.write("ply\nformat ascii 1.0\nelement vertex 2\nproperty float x\nproperty float y\nproperty float z\nproperty uchar red\nend_header\n")
        fp.write("0.5 1 -2 255\n3 4.25 5 0\n")
    assert cloud_align.read_cloud(str(tmp_path / "a.ply")).tolist() == [[0.5, 1.0, -2.0], [3.0, 4.25, 5.0]]
    rec = np.zeros(3, np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("intensity", "<f4"), ("ring", "<u2")]))
    rec["x"], rec["y"], rec["z"] = [1, 2, 3], [4, 5, 6], [7, 8, 9]
    with open(str(tmp_path / "c.ply"), "wb") as fp:
        fp.write(b"ply\nformat binary_little_endian 1.0\nelement vertex 3\nproperty float x\nproperty float y\nproperty float z\nproperty float intensity\n"
                 b"property ushort ring\nend_header\n" + rec.tobytes())
    assert cloud_align.read_cloud(str(tmp_path / "c.ply")).tolist() == [[1, 4, 7], [2, 5, 8], [3, 6, 9]]
