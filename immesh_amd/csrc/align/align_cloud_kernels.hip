// One step of the alignment of a cloud to the indexed cloud for gfx950 (include/immesh_align.h, the Cloud rule, has the exact contract).
//   step      one source point per lane: the Point rule (dq_point), the distance walk of raycast_dev.hpp (dq_walk) over the index's hierarchy with a
//             leaf that is D of a cloud point and keeps nothing: the walk carries the bound and the winner's index alone.  Behind the walk the
//             winner's three floats are loaded once more (the same floats minus the same p: q, whose squares are D bit for bit), in PLANE mode its
//             stored normal and status; then the rows (al_row), the weight, the 28 terms and the workgroup's fold (al_block_fold) of align_dev.hpp.
//             The kernel's registers are held to the walk's occupancy from the start (DESIGN section 26 measured that on the caster's walk).
//   split     the same step in two launches (the walk stores winner and q, the second forms and folds the terms): immesh_align_cloud_set_variant 1,
//             the default by measurement; the fused kernel is variant 0
//   fold      the final fold is al_launch_fold of align_kernels.hip: the same launch as the mesh rule's, so the same order of additions
// Double arithmetic is written in the contract's order; the library builds with -ffp-contract=off, so nothing is fused.
#include "align_dev.hpp"

namespace {

// the walk's leaf: D of a cloud point by the mesh-to-cloud header's D rule; nothing of the winner is kept but what the walk keeps itself
struct AcPointLeaf {
    const float* __restrict__ cloud;
    const double* p;
    __device__ __forceinline__ double dist(int32_t j) const {
        const float* c = cloud + 3 * (int64_t)j;
        const double e0 = (double)c[0] - p[0], e1 = (double)c[1] - p[1], e2 = (double)c[2] - p[2];
        return (e0 * e0 + e1 * e1) + e2 * e2;
    }
    __device__ __forceinline__ void accept() const {}
};

// what both launches read of the target: the cloud, and in PLANE mode the stored normals and their status
struct AcTarget {
    const float* __restrict__ cloud;
    const float* __restrict__ normal;
    const uint8_t* __restrict__ nstatus;
};

// q of winner j: the e_k of the D rule
__device__ __forceinline__ void ac_q(const float* __restrict__ cloud, int32_t j, const double* p, double* q) {
    const float* c = cloud + 3 * (int64_t)j;
    q[0] = (double)c[0] - p[0]; q[1] = (double)c[1] - p[1]; q[2] = (double)c[2] - p[2];
}

// the terms of a point with winner j; false: PLANE mode and a winner without a normal (t is left as it was)
__device__ __forceinline__ bool ac_terms(int mode, double huber, const double* p, const AlCentre& ce, const double* q, const AcTarget& tg, int32_t j, double* t) {
    const double x[3] = {p[0] - ce.c[0], p[1] - ce.c[1], p[2] - ce.c[2]};
    double d;
    if (mode == 0) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const double u[3] = {k == 0 ? 1.0 : 0.0, k == 1 ? 1.0 : 0.0, k == 2 ? 1.0 : 0.0};
            al_row(x, u, q[k], k == 0, t);
        }
        d = sqrt((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]);
    } else {
        if (tg.nstatus[j] != 0) return false;
        const float* nf = tg.normal + 3 * (int64_t)j;
        const double u[3] = {(double)nf[0], (double)nf[1], (double)nf[2]};
        const double r = rc_dot(u, q);
        al_row(x, u, r, true, t);
        d = fabs(r);
    }
    if (huber > 0.0) {
        const double w = d <= huber ? 1.0 : huber / d;
#pragma unroll
        for (int k = 0; k < AL_TERMS; k++) t[k] = w * t[k];
    }
    return true;
}

// what follows the walk of point i: its terms and counts, the per-point outputs, the workgroup's partial
__device__ __forceinline__ void ac_finish(bool in_range, int64_t i, bool ok, int32_t best_j, const double* p, const double* q, int mode, double huber,
                                          const AlCentre& ce, const AcTarget& tg, AlSystemDev* __restrict__ part, int32_t* __restrict__ index_out,
                                          double* __restrict__ terms_out) {
    double t[AL_TERMS];
#pragma unroll
    for (int k = 0; k < AL_TERMS; k++) t[k] = 0.0;
    long long c[4] = {0, 0, 0, 0};
    if (in_range) {
        if (best_j >= 0) {
            if (ac_terms(mode, huber, p, ce, q, tg, best_j, t)) c[0] = 1;
            else c[3] = 1;
        } else if (ok) {
            c[2] = 1;
        } else {
            c[1] = 1;
        }
        if (index_out) index_out[i] = best_j;
        if (terms_out) {
#pragma unroll
            for (int k = 0; k < AL_TERMS; k++) terms_out[AL_TERMS * i + k] = t[k];
        }
    }
    al_block_fold(t, c, part + blockIdx.x);
}

// the fused step (variant 0): the walk, the reload, the terms and the fold in one launch, the registers held to 80 (six wavefronts per SIMD); the
// fold's tail spills to scratch instead, once per lane behind the walk.  Measured, it is level with the split pair up to 100 000 points and 11 %
// slower at 1 000 000, where the point walk's own eight wavefronts per SIMD count: the split pair is the default
__global__ void __attribute__((amdgpu_waves_per_eu(6, 8))) __launch_bounds__(AL_BLOCK)
alc_step_kernel(RcFrame fr, int has_frame, const float* __restrict__ pts, int64_t n_pts, double r2, int mode, double huber, AlCentre ce, AcTarget tg,
                const RcNode* __restrict__ nodes, int64_t n_in, AlSystemDev* __restrict__ part, int32_t* __restrict__ index_out, double* __restrict__ terms_out) {
    const int64_t i = (int64_t)blockIdx.x * AL_BLOCK + threadIdx.x;
    const bool in_range = i < n_pts;
    double p[3] = {0.0, 0.0, 0.0}, q[3] = {0.0, 0.0, 0.0};
    const bool ok = in_range && dq_point(fr, has_frame != 0, pts, i, p);
    double best = r2;
    int32_t best_j = -1;
    AcPointLeaf leaf = {tg.cloud, p};
    if (ok && n_in > 0) dq_walk(nodes, p, best, best_j, leaf);
    if (best_j >= 0) ac_q(tg.cloud, best_j, p, q);
    ac_finish(in_range, i, ok, best_j, p, q, mode, huber, ce, tg, part, index_out, terms_out);
}

// the split variant's first launch: the walk alone
__global__ void __launch_bounds__(AL_BLOCK) alc_walk_kernel(RcFrame fr, int has_frame, const float* __restrict__ pts, int64_t n_pts, double r2,
                                                            const float* __restrict__ cloud, const RcNode* __restrict__ nodes, int64_t n_in,
                                                            int32_t* __restrict__ sindex, double* __restrict__ sq) {
    const int64_t i = (int64_t)blockIdx.x * AL_BLOCK + threadIdx.x;
    if (i >= n_pts) return;
    double p[3], q[3] = {0.0, 0.0, 0.0};
    const bool ok = dq_point(fr, has_frame != 0, pts, i, p);
    double best = r2;
    int32_t best_j = -1;
    AcPointLeaf leaf = {cloud, p};
    if (ok && n_in > 0) dq_walk(nodes, p, best, best_j, leaf);
    if (best_j >= 0) ac_q(cloud, best_j, p, q);
    sindex[i] = best_j >= 0 ? best_j : (ok ? -1 : -2);
    for (int k = 0; k < 3; k++) sq[3 * i + k] = q[k];
}

// the split variant's second launch: the terms of the stored winners and the fold
__global__ void __launch_bounds__(AL_BLOCK) alc_terms_kernel(RcFrame fr, int has_frame, const float* __restrict__ pts, int64_t n_pts, int mode, double huber,
                                                             AlCentre ce, AcTarget tg, const int32_t* __restrict__ sindex, const double* __restrict__ sq,
                                                             AlSystemDev* __restrict__ part, int32_t* __restrict__ index_out, double* __restrict__ terms_out) {
    const int64_t i = (int64_t)blockIdx.x * AL_BLOCK + threadIdx.x;
    const bool in_range = i < n_pts;
    double p[3] = {0.0, 0.0, 0.0}, q[3] = {0.0, 0.0, 0.0};
    int32_t j = -1;
    bool ok = false;
    if (in_range) {
        j = sindex[i];
        ok = j != -2;
        if (j >= 0) {
            (void)dq_point(fr, has_frame != 0, pts, i, p);
            for (int k = 0; k < 3; k++) q[k] = sq[3 * i + k];
        } else {
            j = -1;
        }
    }
    ac_finish(in_range, i, ok, j, p, q, mode, huber, ce, tg, part, index_out, terms_out);
}

}  // namespace

void alc_launch_step(hipStream_t s, const RcFrame& fr, int has_frame, const float* pts, int64_t n_pts, double r2, int mode, const double* centre, double huber,
                     const float* cloud, const float* normal, const uint8_t* nstatus, const RcNode* nodes, int64_t n_in, AlSystemDev* part, AlSystemDev* res,
                     int32_t* index_out, double* terms_out) {
    const int64_t blocks = al_blocks(n_pts);
    if (blocks > 0)
        alc_step_kernel<<<(unsigned)blocks, AL_BLOCK, 0, s>>>(fr, has_frame, pts, n_pts, r2, mode, huber, al_centre(centre), AcTarget{cloud, normal, nstatus},
                                                              nodes, n_in, part, index_out, terms_out);
    al_launch_fold(s, part, blocks, res);
}

void alc_launch_step_split(hipStream_t s, const RcFrame& fr, int has_frame, const float* pts, int64_t n_pts, double r2, int mode, const double* centre,
                           double huber, const float* cloud, const float* normal, const uint8_t* nstatus, const RcNode* nodes, int64_t n_in, int32_t* sindex,
                           double* sq, AlSystemDev* part, AlSystemDev* res, int32_t* index_out, double* terms_out) {
    const int64_t blocks = al_blocks(n_pts);
    if (blocks > 0) {
        alc_walk_kernel<<<(unsigned)blocks, AL_BLOCK, 0, s>>>(fr, has_frame, pts, n_pts, r2, cloud, nodes, n_in, sindex, sq);
        alc_terms_kernel<<<(unsigned)blocks, AL_BLOCK, 0, s>>>(fr, has_frame, pts, n_pts, mode, huber, al_centre(centre), AcTarget{cloud, normal, nstatus},
                                                               sindex, sq, part, index_out, terms_out);
    }
    al_launch_fold(s, part, blocks, res);
}
