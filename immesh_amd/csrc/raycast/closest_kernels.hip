// Closest face of every point for gfx950 (include/immesh_closest.h has the exact contract these kernels implement), on the ray caster's hierarchy.
//   query     one point per lane on the distance walk of raycast_dev.hpp (dq_walk): the leaf is the contract's Face rule, and the face that wins
//             keeps its closest point and the point's side.  Points are taken in arrival order: sorting them by Morton code first was measured
//             and lost.
//   stats     for this query and the nearest-point query alike: per-workgroup partials (counts, the largest dist, two double sums by a fixed tree over the lanes; integer atomics for the histogram,
//             in LDS first when it has at most DQ_LDS_BINS bins), then one workgroup folds the partials in index order: the same bits on every call
// Double arithmetic is written in the contract's order; the library builds with -ffp-contract=off, so nothing is fused.
#include "raycast.hpp"
#include "raycast_dev.hpp"

namespace {

// the walk's leaf: D of a face, and, of the face that was accepted last, its q and the side of the point
struct RcFaceLeaf {
    const float* __restrict__ vtx;
    const int32_t* __restrict__ faces;
    const double* p;
    double A[3][3], q[3];           // the face evaluated last: its corners relative to p, its closest point
    double best_q[3];
    int best_side;
    __device__ __forceinline__ double dist(int32_t f) {
        float lo[3], hi[3];
        rc_load_face(vtx, faces, f, p, lo, hi, A);
        rc_face_point(A[0], A[1], A[2], q);
        return fmax(rc_dot(q, q), dq_box(p, lo, hi));
    }
    __device__ __forceinline__ void accept() {
        best_q[0] = q[0]; best_q[1] = q[1]; best_q[2] = q[2];
        const double u[3] = {A[1][0] - A[0][0], A[1][1] - A[0][1], A[1][2] - A[0][2]};
        const double w[3] = {A[2][0] - A[0][0], A[2][1] - A[0][1], A[2][2] - A[0][2]};
        const double ma[3] = {-A[0][0], -A[0][1], -A[0][2]};
        double n[3];
        rc_cross(u, w, n);
        const double sd = rc_dot(n, ma);
        best_side = sd > 0.0 ? 1 : (sd < 0.0 ? -1 : 0);
    }
};

__global__ void __launch_bounds__(RC_BLOCK) rc_closest_kernel(RcFrame fr, int has_frame, const float* __restrict__ pts,
                                                              int64_t n_pts, double r2, const float* __restrict__ vtx, const int32_t* __restrict__ faces,
                                                              const RcNode* __restrict__ nodes, int64_t n_in, double* __restrict__ d2_out,
                                                              float* __restrict__ dist_out, int32_t* __restrict__ face_out, float* __restrict__ xyz_out,
                                                              int8_t* __restrict__ side_out, uint8_t* __restrict__ status_out) {
    const int64_t i = (int64_t)blockIdx.x * RC_BLOCK + threadIdx.x;
    if (i >= n_pts) return;
    double p[3];
    const bool ok = dq_point(fr, has_frame != 0, pts, i, p);
    double best = r2;              // the bound: r2 until a face counts, then the best D
    int32_t best_f = -1;
    RcFaceLeaf leaf = {vtx, faces, p, {}, {}, {0.0, 0.0, 0.0}, 0};
    if (ok && n_in > 0) dq_walk(nodes, p, best, best_f, leaf);
    const float nanf32 = __uint_as_float(0x7FC00000u);
    const bool have = best_f >= 0;
    d2_out[i] = have ? best : -1.0;
    dist_out[i] = have ? (float)sqrt(best) : -1.0f;
    face_out[i] = best_f;
    for (int k = 0; k < 3; k++) xyz_out[3 * i + k] = have ? (float)(p[k] + leaf.best_q[k]) : nanf32;
    side_out[i] = (int8_t)(have ? leaf.best_side : 0);
    status_out[i] = have ? 0 : (ok ? 1 : 2);
}

// ---- the reduction -------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void dq_fold(DqStatsDev& a, const DqStatsDev& b) {
    a.sum += b.sum; a.sum2 += b.sum2;
    a.n_face += b.n_face; a.n_not_finite += b.n_not_finite; a.n_no_face += b.n_no_face;
    a.max_dist = fmaxf(a.max_dist, b.max_dist);
}

// the workgroup's tree over s[0 .. RC_BLOCK): s[t] += s[t + stride], stride = RC_BLOCK / 2 .. 1 -- a fixed order
__device__ __forceinline__ void dq_tree(DqStatsDev* s) {
    for (int stride = RC_BLOCK / 2; stride >= 1; stride >>= 1) {
        __syncthreads();
        if ((int)threadIdx.x < stride) dq_fold(s[threadIdx.x], s[threadIdx.x + stride]);
    }
    __syncthreads();
}

__global__ void __launch_bounds__(RC_BLOCK) dq_stats_kernel(const float* __restrict__ dist, const uint8_t* __restrict__ status, int64_t n_pts, float bin_width,
                                                            int32_t n_bins, DqStatsDev* __restrict__ part, unsigned long long* hist) {
    __shared__ DqStatsDev s[RC_BLOCK];
    __shared__ uint32_t s_hist[DQ_LDS_BINS + 1];                  // [n_bins]: the overflow count
    const bool in_lds = n_bins <= DQ_LDS_BINS;                    // most of a cloud falls into a few bins: count them here, not on one global address
    if (in_lds) {
        for (int b = threadIdx.x; b <= n_bins; b += RC_BLOCK) s_hist[b] = 0u;
        __syncthreads();
    }
    const int64_t i = (int64_t)blockIdx.x * RC_BLOCK + threadIdx.x;
    DqStatsDev me = {0.0, 0.0, 0, 0, 0, 0.0f, 0};
    if (i < n_pts) {
        const uint8_t st = status[i];
        if (st == 0) {
            const float d = dist[i];
            const double dd = (double)d;
            me.sum = dd; me.sum2 = dd * dd; me.n_face = 1; me.max_dist = d;
            const float b = d / bin_width;
            const int32_t bin = b < (float)n_bins ? (int32_t)b : n_bins;
            if (in_lds) atomicAdd(&s_hist[bin], 1u);
            else atomicAdd(&hist[bin], 1ull);
        } else if (st == 2) {
            me.n_not_finite = 1;
        } else {
            me.n_no_face = 1;
        }
    }
    s[threadIdx.x] = me;
    dq_tree(s);                                                   // (its barriers also complete s_hist)
    if (threadIdx.x == 0) part[blockIdx.x] = s[0];
    if (in_lds)
        for (int b = threadIdx.x; b <= n_bins; b += RC_BLOCK)
            if (s_hist[b]) atomicAdd(&hist[b], (unsigned long long)s_hist[b]);
}

// one workgroup: lane t folds partials t, t + RC_BLOCK, ... in that order, then the tree
__global__ void __launch_bounds__(RC_BLOCK) dq_fold_kernel(const DqStatsDev* __restrict__ part, int64_t n_part, DqStatsDev* __restrict__ res) {
    __shared__ DqStatsDev s[RC_BLOCK];
    DqStatsDev me = {0.0, 0.0, 0, 0, 0, 0.0f, 0};
    for (int64_t j = threadIdx.x; j < n_part; j += RC_BLOCK) dq_fold(me, part[j]);
    s[threadIdx.x] = me;
    dq_tree(s);
    if (threadIdx.x == 0) res[0] = s[0];
}

}  // namespace

void rc_launch_closest(hipStream_t s, const RcFrame& fr, int has_frame, const float* pts, int64_t n_pts, double r2, const float* vtx,
                     const int32_t* faces, const RcNode* nodes, int64_t n_in, double* d2, float* dist, int32_t* face, float* xyz, int8_t* side,
                     uint8_t* status) {
    if (n_pts > 0)
        rc_closest_kernel<<<rc_grid(n_pts), RC_BLOCK, 0, s>>>(fr, has_frame, pts, n_pts, r2, vtx, faces, nodes, n_in, d2, dist, face, xyz, side, status);
}

int64_t dq_stats_blocks(int64_t n_pts) { return (n_pts + RC_BLOCK - 1) / RC_BLOCK; }

void dq_launch_stats(hipStream_t s, const float* dist, const uint8_t* status, int64_t n_pts, float bin_width, int32_t n_bins, DqStatsDev* part,
                     unsigned long long* hist, DqStatsDev* res) {
    const int64_t blocks = dq_stats_blocks(n_pts);
    if (blocks > 0) dq_stats_kernel<<<(unsigned)blocks, RC_BLOCK, 0, s>>>(dist, status, n_pts, bin_width, n_bins, part, hist);
    dq_fold_kernel<<<1, RC_BLOCK, 0, s>>>(part, blocks, res);
}
