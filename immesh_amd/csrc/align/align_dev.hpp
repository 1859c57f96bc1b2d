// Device code the two step kernels of the alignment share (align_kernels.hip: a cloud to the caster's snapshot; align_cloud_kernels.hip: a cloud to
// the indexed cloud): one row's contribution to the 28 terms, and the workgroup's fold.  The final fold over the workgroups' partials is one launch,
// al_launch_fold of align.hpp, which both files queue behind their step.
#pragma once
#include "align.hpp"
#include "../raycast/raycast_dev.hpp"

namespace {

constexpr int AL_BLOCK = RC_BLOCK;
constexpr int AL_WAVES = AL_BLOCK / 64;
static_assert(AL_WAVES == 4, "the fold adds four wavefront partials in index order");

struct AlCentre { double c[3]; };

// one row (j, r), j = (cross(x, u), u), added to the terms (first: the row that begins the sums)
__device__ __forceinline__ void al_row(const double* x, const double* u, double r, bool first, double* t) {
    double j[6];
    rc_cross(x, u, j);
    j[3] = u[0]; j[4] = u[1]; j[5] = u[2];
    int idx = 0;
#pragma unroll
    for (int a = 0; a < 6; a++)
#pragma unroll
        for (int b = a; b < 6; b++, idx++) {
            const double v = j[a] * j[b];
            t[idx] = first ? v : t[idx] + v;
        }
#pragma unroll
    for (int a = 0; a < 6; a++) {
        const double v = j[a] * r;
        t[21 + a] = first ? v : t[21 + a] + v;
    }
    const double rr = r * r;
    t[27] = first ? rr : t[27] + rr;
}

// The workgroup's fold of (t, c) -> out[0], written by lanes 0 .. 31.  Every lane of the workgroup calls it.
__device__ __forceinline__ void al_block_fold(double* t, long long* c, AlSystemDev* out) {
    __shared__ double s_t[AL_WAVES][AL_TERMS];
    __shared__ long long s_c[AL_WAVES][4];
#pragma unroll
    for (int k = 0; k < AL_TERMS; k++) {
        double v = t[k];
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
        t[k] = v;
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
        long long v = c[k];
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
        c[k] = v;
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < AL_TERMS; k++) s_t[w][k] = t[k];
#pragma unroll
        for (int k = 0; k < 4; k++) s_c[w][k] = c[k];
    }
    __syncthreads();
    const int k = threadIdx.x;
    if (k < AL_TERMS) out->s[k] = ((s_t[0][k] + s_t[1][k]) + s_t[2][k]) + s_t[3][k];
    else if (k < AL_TERMS + 4) out->n[k - AL_TERMS] = ((s_c[0][k - AL_TERMS] + s_c[1][k - AL_TERMS]) + s_c[2][k - AL_TERMS]) + s_c[3][k - AL_TERMS];
}

inline AlCentre al_centre(const double* c) { return AlCentre{{c[0], c[1], c[2]}}; }

}  // namespace
