#!/usr/bin/env python3
"""Golden records of RGB_pts::update_rgb for tests/test_colour_cpu.py -> tests/golden/colour_update_r07.npz.

Runs only where the reference tree exists.  It cuts src/meshing/r3live/pointcloud_rgbd.cpp:118-195 (the constants and update_rgb) at run time into a
temporary directory, compiles the cut behind a ten-line vec_3 stand-in and a bare RGB_pts with the six colour fields (g++ -O2 -ffp-contract=off), and
drives it with a stream of observations that takes every branch: black pixel, first observation, the 1.1 distance gate, the clamp at 255, a nearer
observation, changing exposure.  Inputs, the state after every call and the return values are written; nothing cut from or compiled from the reference
leaves the temporary directory.

2 000 points x 12 observations.  The three covariances of a point are equal by construction (one sigma for the three channels, as both callers
pass it) and stored once; compressed, the file stays below the repository's 1 MiB limit for a committed file.

usage: tools/make_golden_colour.py [reference root, default /root/reference]"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_PTS, N_OBS = 2000, 12

PRELUDE = r"""
#include <cmath>
#include <cstdio>
#include <vector>
using namespace std;
struct vec_3 {
    double v[3];
    vec_3() { v[0] = v[1] = v[2] = 0; }
    vec_3(double a, double b, double c) { v[0] = a; v[1] = b; v[2] = c; }
    double operator()(int i) const { return v[i]; }
    double norm() const { return std::sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]); }
    double maxCoeff() const { double m = v[0]; if (v[1] > m) m = v[1]; if (v[2] > m) m = v[2]; return m; }
    vec_3 operator/(double s) const { return vec_3(v[0] / s, v[1] / s, v[2] / s); }
};
struct RGB_pts {
    double m_rgb[3] = {0, 0, 0}, m_cov_rgb[3] = {0, 0, 0};
    int m_N_rgb = 0;
    double m_obs_dis = 0, m_last_obs_time = 0, m_first_obs_exposure_time = 1.0;   // RGB_pts::clear(), g_initial_camera_exp_tim = 1
    int update_rgb(const vec_3& rgb, const double obs_dis, const vec_3 obs_sigma, const double obs_time, const double current_exposure_time);
};
#include "cut.inc"
int main(int argc, char** argv) {
    FILE* fi = fopen(argv[1], "rb");
    FILE* fo = fopen(argv[2], "wb");
    long dims[2];
    if (!fi || !fo || fread(dims, sizeof(long), 2, fi) != 2) return 1;
    std::vector<RGB_pts> pts(dims[0]);
    for (long j = 0; j < dims[1]; j++)
        for (long p = 0; p < dims[0]; p++) {
            double in[7];   // c0 c1 c2 obs_dis sigma t e
            if (fread(in, sizeof(double), 7, fi) != 7) return 2;
            RGB_pts& q = pts[p];
            const int ret = q.update_rgb(vec_3(in[0], in[1], in[2]), in[3], vec_3(in[4], in[4], in[4]), in[5], in[6]);
            const double out[11] = {q.m_rgb[0], q.m_rgb[1], q.m_rgb[2], q.m_cov_rgb[0], q.m_cov_rgb[1], q.m_cov_rgb[2], q.m_first_obs_exposure_time,
                                    q.m_obs_dis, q.m_last_obs_time, (double)q.m_N_rgb, (double)ret};
            fwrite(out, sizeof(double), 11, fo);
        }
    fclose(fo);
    return 0;
}
"""


def make_inputs():
    rng = np.random.default_rng(707)
    c = rng.integers(0, 256, (N_OBS, N_PTS, 3)).astype(np.uint8)
    c[rng.random((N_OBS, N_PTS)) < 0.06] = 0                                     # black pixel: rejected
    c[rng.random((N_OBS, N_PTS)) < 0.05] = 255                                   # white: drives the clamp at 255 when the exposure changes
    bright = rng.random(N_PTS) < 0.3
    c[:, bright] = np.maximum(c[:, bright], 236)
    base = rng.uniform(1.0, 20.0, N_PTS)
    factor = rng.choice([0.7, 0.9, 0.97, 1.0, 1.05, 1.1, 1.1000001, 1.15, 1.3], (N_OBS, N_PTS))   # nearer observations, both sides of the 1.1 gate
    obs_dis = base[None, :] * factor
    view = rng.random(N_PTS) < 0.5                                               # half the points with VIEW's sigma, half with PLAIN's 1.5
    ang = rng.integers(20, 121, (N_OBS, N_PTS)) * 0.25                             # 5 .. 30 degrees in quarter steps (few distinct values: the file compresses)
    sigma = np.where(view[None, :], (1.5 * np.maximum(obs_dis, 1.0)) * ang, 1.5)
    t = (0.1 * np.arange(N_OBS))[:, None] + rng.integers(0, 50, (N_OBS, N_PTS)) / 1000.0
    e = np.broadcast_to(rng.choice([0.005, 0.01, 0.02, 0.035], N_OBS)[:, None], (N_OBS, N_PTS)).copy()
    e[0] = 0.01
    return c, obs_dis, sigma, t, e


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    src = os.path.join(ref, "src", "meshing", "r3live", "pointcloud_rgbd.cpp")
    if not os.path.exists(src):
        sys.exit(f"{src} not found: this tool runs only where the reference tree exists")
    c, obs_dis, sigma, t, e = make_inputs()
    with tempfile.TemporaryDirectory() as tmp:
        with open(src) as f:
            lines = f.readlines()
        with open(os.path.join(tmp, "cut.inc"), "w") as f:
            f.writelines(lines[117:195])                                         # :118-195
        with open(os.path.join(tmp, "drive.cpp"), "w") as f:
            f.write(PRELUDE)
        exe = os.path.join(tmp, "drive")
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++14", "-o", exe, os.path.join(tmp, "drive.cpp")])
        rec = np.concatenate([c.astype(np.float64), obs_dis[..., None], sigma[..., None], t[..., None], e[..., None]], axis=2)
        with open(os.path.join(tmp, "in.bin"), "wb") as f:
            f.write(np.array([N_PTS, N_OBS], np.int64).tobytes())
            f.write(np.ascontiguousarray(rec).tobytes())
        subprocess.check_call([exe, os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")])
        out = np.fromfile(os.path.join(tmp, "out.bin"), np.float64).reshape(N_OBS, N_PTS, 11)
    rgb, cov, first, s_dis, last, n_obs, ret = out[..., 0:3], out[..., 3:6], out[..., 6], out[..., 7], out[..., 8], out[..., 9], out[..., 10]
    assert np.all(cov[..., 0] == cov[..., 1]) and np.all(cov[..., 0] == cov[..., 2])
    # every branch is taken
    n_prev = np.concatenate([np.zeros((1, N_PTS)), n_obs[:-1]])
    d_prev = np.concatenate([np.zeros((1, N_PTS)), s_dis[:-1]])
    black = (c == 0).all(axis=2)
    gate = ~black & (d_prev != 0) & (obs_dis > d_prev * 1.1)
    firsts = (n_prev == 0) & (n_obs == 1)
    nearer = (ret == 1) & (s_dis < d_prev)
    clamp = (ret == 1) & (np.abs((rgb / np.concatenate([np.ones((1, N_PTS)), first[:-1]])[..., None]).max(axis=2) - 254.999) < 1e-9)
    cover = dict(black=int(black.sum()), gate=int(gate.sum()), first=int(firsts.sum()), updated=int((ret == 1).sum()), nearer=int(nearer.sum()),
                 clamp=int(clamp.sum()), exposures=len(np.unique(e)))
    print(cover)
    assert all(v > 0 for v in cover.values()) and cover["exposures"] > 2, cover
    path = os.path.join(ROOT, "tests", "golden", "colour_update_r07.npz")
    np.savez_compressed(path, c=c, obs_dis=obs_dis, sigma=sigma, t=t, e=e[:, 0].copy(), rgb=rgb, cov=cov[..., 0].copy(), first_exposure=first,
                        state_obs_dis=s_dis, last_obs_time=last, n_obs=n_obs.astype(np.int8), ret=ret.astype(np.int8))
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
