// One step of the alignment of a cloud to the caster's snapshot for gfx950 (include/immesh_align.h has the exact contract these kernels implement).
//   step      one point per lane: the Point rule (dq_point), the distance walk of raycast_dev.hpp (dq_walk) with the closest query's Face rule as its
//             leaf, which keeps the winner's q; the winner's corners are loaded once more behind the walk (the same floats minus the same p: the
//             same bits) so that the walk carries 3 doubles of the winner, not 12; then the 28 terms and the fold
//   fold      over the wavefront by a butterfly of shuffles (both lanes add the same two values, so every lane ends with the same bits), the four
//             wavefronts' partials through LDS in index order, one AlSystemDev per workgroup; then one workgroup folds the partials, lane t taking
//             t, t + AL_BLOCK, ... in that order, and goes through the same fold: a fixed order that depends on n_pts alone.  No double atomics.
//   split     the same step in two launches (the walk stores face and q, the second forms and folds the terms): kept for the measurement, as is
//             the fused kernel without its register cap (immesh_align_set_variant; tools/align_bench.py)
// Double arithmetic is written in the contract's order; the library builds with -ffp-contract=off, so nothing is fused.
#include "align_dev.hpp"   // al_row, al_block_fold: the cloud-to-cloud step (align_cloud_kernels.hip) shares them

namespace {

// the walk's leaf: D of a face by the closest query's Face rule; of the face that was accepted last, its q
struct AlFaceLeaf {
    const float* __restrict__ vtx;
    const int32_t* __restrict__ faces;
    const double* p;
    double q[3], best_q[3];
    __device__ __forceinline__ double dist(int32_t f) {
        float lo[3], hi[3];
        double A[3][3];
        rc_load_face(vtx, faces, f, p, lo, hi, A);
        rc_face_point(A[0], A[1], A[2], q);
        return fmax(rc_dot(q, q), dq_box(p, lo, hi));
    }
    __device__ __forceinline__ void accept() { best_q[0] = q[0]; best_q[1] = q[1]; best_q[2] = q[2]; }
};

// the terms of a point with a winner; false: PLANE mode and a flat winner (t is left as it was)
__device__ __forceinline__ bool al_terms(int mode, const double* p, const AlCentre& ce, const double* q, const float* __restrict__ vtx,
                                         const int32_t* __restrict__ faces, int32_t f, double* t) {
    const double x[3] = {p[0] - ce.c[0], p[1] - ce.c[1], p[2] - ce.c[2]};
    if (mode == 0) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const double u[3] = {k == 0 ? 1.0 : 0.0, k == 1 ? 1.0 : 0.0, k == 2 ? 1.0 : 0.0};
            al_row(x, u, q[k], k == 0, t);
        }
        return true;
    }
    float lo[3], hi[3];
    double A[3][3];
    rc_load_face(vtx, faces, f, p, lo, hi, A);
    const double ab[3] = {A[1][0] - A[0][0], A[1][1] - A[0][1], A[1][2] - A[0][2]};
    const double ac[3] = {A[2][0] - A[0][0], A[2][1] - A[0][1], A[2][2] - A[0][2]};
    double n[3];
    rc_cross(ab, ac, n);
    const double nn = rc_dot(n, n);
    if (!(isfinite(nn) && nn > 0.0)) return false;
    const double s = sqrt(nn);
    const double u[3] = {n[0] / s, n[1] / s, n[2] / s};
    al_row(x, u, rc_dot(u, A[0]), true, t);
    return true;
}

// what follows the walk of point i: its terms and counts, the per-point outputs, the workgroup's partial
__device__ __forceinline__ void al_finish(bool in_range, int64_t i, bool ok, int32_t best_f, const double* p, const double* q, int mode, const AlCentre& ce,
                                          const float* __restrict__ vtx, const int32_t* __restrict__ faces, AlSystemDev* __restrict__ part,
                                          int32_t* __restrict__ face_out, double* __restrict__ terms_out) {
    double t[AL_TERMS];
#pragma unroll
    for (int k = 0; k < AL_TERMS; k++) t[k] = 0.0;
    long long c[4] = {0, 0, 0, 0};
    if (in_range) {
        if (best_f >= 0) {
            if (al_terms(mode, p, ce, q, vtx, faces, best_f, t)) c[0] = 1;
            else c[3] = 1;
        } else if (ok) {
            c[2] = 1;
        } else {
            c[1] = 1;
        }
        if (face_out) face_out[i] = best_f;
        if (terms_out) {
#pragma unroll
            for (int k = 0; k < AL_TERMS; k++) terms_out[AL_TERMS * i + k] = t[k];
        }
    }
    al_block_fold(t, c, part + blockIdx.x);
}

__device__ __forceinline__ void al_step_body(const RcFrame& fr, int has_frame, const float* __restrict__ pts, int64_t n_pts, double r2, int mode,
                                             const AlCentre& ce, const float* __restrict__ vtx, const int32_t* __restrict__ faces,
                                             const RcNode* __restrict__ nodes, int64_t n_in, AlSystemDev* __restrict__ part,
                                             int32_t* __restrict__ face_out, double* __restrict__ terms_out) {
    const int64_t i = (int64_t)blockIdx.x * AL_BLOCK + threadIdx.x;
    const bool in_range = i < n_pts;
    double p[3] = {0.0, 0.0, 0.0};
    const bool ok = in_range && dq_point(fr, has_frame != 0, pts, i, p);
    double best = r2;
    int32_t best_f = -1;
    AlFaceLeaf leaf = {vtx, faces, p, {}, {0.0, 0.0, 0.0}};
    if (ok && n_in > 0) dq_walk(nodes, p, best, best_f, leaf);
    al_finish(in_range, i, ok, best_f, p, leaf.best_q, mode, ce, vtx, faces, part, face_out, terms_out);
}

// the fused step as the register allocator leaves it, kept for the measurement: the fold's 28 live doubles set the kernel's registers (138 VGPRs, three
// wavefronts per SIMD where the walk alone has 76 and six), and the walk pays: 1.4 to 1.5 times the capped kernel's time from 100 000 faces on
__global__ void __launch_bounds__(AL_BLOCK) al_step_kernel(RcFrame fr, int has_frame, const float* __restrict__ pts, int64_t n_pts, double r2, int mode,
                                                           AlCentre ce, const float* __restrict__ vtx, const int32_t* __restrict__ faces,
                                                           const RcNode* __restrict__ nodes, int64_t n_in, AlSystemDev* __restrict__ part,
                                                           int32_t* __restrict__ face_out, double* __restrict__ terms_out) {
    al_step_body(fr, has_frame, pts, n_pts, r2, mode, ce, vtx, faces, nodes, n_in, part, face_out, terms_out);
}

// THE STEP (variant 0): the same with the registers held to the walk's own occupancy (80 VGPRs, six wavefronts per SIMD); the fold's tail spills 87
// registers to scratch instead, once per lane behind the walk (DESIGN section 26 has the figures of the three shapes)
__global__ void __attribute__((amdgpu_waves_per_eu(6, 8))) __launch_bounds__(AL_BLOCK)
al_step_capped_kernel(RcFrame fr, int has_frame, const float* __restrict__ pts, int64_t n_pts, double r2, int mode, AlCentre ce, const float* __restrict__ vtx,
                      const int32_t* __restrict__ faces, const RcNode* __restrict__ nodes, int64_t n_in, AlSystemDev* __restrict__ part,
                      int32_t* __restrict__ face_out, double* __restrict__ terms_out) {
    al_step_body(fr, has_frame, pts, n_pts, r2, mode, ce, vtx, faces, nodes, n_in, part, face_out, terms_out);
}

// the split variant's first launch: the walk alone
__global__ void __launch_bounds__(AL_BLOCK) al_walk_kernel(RcFrame fr, int has_frame, const float* __restrict__ pts, int64_t n_pts, double r2,
                                                           const float* __restrict__ vtx, const int32_t* __restrict__ faces, const RcNode* __restrict__ nodes,
                                                           int64_t n_in, int32_t* __restrict__ sface, double* __restrict__ sq) {
    const int64_t i = (int64_t)blockIdx.x * AL_BLOCK + threadIdx.x;
    if (i >= n_pts) return;
    double p[3];
    const bool ok = dq_point(fr, has_frame != 0, pts, i, p);
    double best = r2;
    int32_t best_f = -1;
    AlFaceLeaf leaf = {vtx, faces, p, {}, {0.0, 0.0, 0.0}};
    if (ok && n_in > 0) dq_walk(nodes, p, best, best_f, leaf);
    sface[i] = best_f >= 0 ? best_f : (ok ? -1 : -2);
    for (int k = 0; k < 3; k++) sq[3 * i + k] = leaf.best_q[k];
}

// the split variant's second launch: the terms of the stored winners and the fold
__global__ void __launch_bounds__(AL_BLOCK) al_terms_kernel(RcFrame fr, int has_frame, const float* __restrict__ pts, int64_t n_pts, int mode, AlCentre ce,
                                                            const float* __restrict__ vtx, const int32_t* __restrict__ faces,
                                                            const int32_t* __restrict__ sface, const double* __restrict__ sq,
                                                            AlSystemDev* __restrict__ part, int32_t* __restrict__ face_out, double* __restrict__ terms_out) {
    const int64_t i = (int64_t)blockIdx.x * AL_BLOCK + threadIdx.x;
    const bool in_range = i < n_pts;
    double p[3] = {0.0, 0.0, 0.0}, q[3] = {0.0, 0.0, 0.0};
    int32_t f = -1;
    bool ok = false;
    if (in_range) {
        f = sface[i];
        ok = f != -2;
        if (f >= 0) {
            (void)dq_point(fr, has_frame != 0, pts, i, p);
            for (int k = 0; k < 3; k++) q[k] = sq[3 * i + k];
        } else {
            f = -1;
        }
    }
    al_finish(in_range, i, ok, f, p, q, mode, ce, vtx, faces, part, face_out, terms_out);
}

// one workgroup: lane t folds partials t, t + AL_BLOCK, ... in that order, then the workgroup's fold
__global__ void __launch_bounds__(AL_BLOCK) al_fold_kernel(const AlSystemDev* __restrict__ part, int64_t n_part, AlSystemDev* __restrict__ res) {
    double t[AL_TERMS];
#pragma unroll
    for (int k = 0; k < AL_TERMS; k++) t[k] = 0.0;
    long long c[4] = {0, 0, 0, 0};
    for (int64_t j = threadIdx.x; j < n_part; j += AL_BLOCK) {
#pragma unroll
        for (int k = 0; k < AL_TERMS; k++) t[k] += part[j].s[k];
#pragma unroll
        for (int k = 0; k < 4; k++) c[k] += part[j].n[k];
    }
    al_block_fold(t, c, res);
}

}  // namespace

int64_t al_blocks(int64_t n_pts) { return (n_pts + AL_BLOCK - 1) / AL_BLOCK; }

void al_launch_fold(hipStream_t s, const AlSystemDev* part, int64_t n_part, AlSystemDev* res) { al_fold_kernel<<<1, AL_BLOCK, 0, s>>>(part, n_part, res); }

void al_launch_step(hipStream_t s, bool capped, const RcFrame& fr, int has_frame, const float* pts, int64_t n_pts, double r2, int mode, const double* centre,
                    const float* vtx, const int32_t* faces, const RcNode* nodes, int64_t n_in, AlSystemDev* part, AlSystemDev* res, int32_t* face_out,
                    double* terms_out) {
    const int64_t blocks = al_blocks(n_pts);
    if (blocks > 0 && capped)
        al_step_capped_kernel<<<(unsigned)blocks, AL_BLOCK, 0, s>>>(fr, has_frame, pts, n_pts, r2, mode, al_centre(centre), vtx, faces, nodes, n_in, part,
                                                                    face_out, terms_out);
    else if (blocks > 0)
        al_step_kernel<<<(unsigned)blocks, AL_BLOCK, 0, s>>>(fr, has_frame, pts, n_pts, r2, mode, al_centre(centre), vtx, faces, nodes, n_in, part, face_out,
                                                             terms_out);
    al_launch_fold(s, part, blocks, res);
}

void al_launch_step_split(hipStream_t s, const RcFrame& fr, int has_frame, const float* pts, int64_t n_pts, double r2, int mode, const double* centre,
                          const float* vtx, const int32_t* faces, const RcNode* nodes, int64_t n_in, int32_t* sface, double* sq, AlSystemDev* part,
                          AlSystemDev* res, int32_t* face_out, double* terms_out) {
    const int64_t blocks = al_blocks(n_pts);
    if (blocks > 0) {
        al_walk_kernel<<<(unsigned)blocks, AL_BLOCK, 0, s>>>(fr, has_frame, pts, n_pts, r2, vtx, faces, nodes, n_in, sface, sq);
        al_terms_kernel<<<(unsigned)blocks, AL_BLOCK, 0, s>>>(fr, has_frame, pts, n_pts, mode, al_centre(centre), vtx, faces, sface, sq, part, face_out,
                                                              terms_out);
    }
    al_launch_fold(s, part, blocks, res);
}
