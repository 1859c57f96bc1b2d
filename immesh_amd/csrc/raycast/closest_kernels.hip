// Closest face of every point for gfx950 (include/immesh_closest.h has the exact contract these kernels implement), on the ray caster's hierarchy.
//   query     one point per lane, a per-lane stack in private memory (depth bound: raycast.hpp), the child with the smaller box bound L first.  A
//             node is skipped only when L of its own box exceeds r2 or the best D so far; D >= L of every enclosing box holds exactly, so no
//             face that wins or ties is ever skipped.  The bound kept on the stack is a float rounded DOWN: it never exceeds L.
//             Points are taken in arrival order: sorting them by Morton code first was measured and lost.
//   stats     per-workgroup partials (counts, the largest dist, two double sums by a fixed tree over the lanes; integer atomics for the histogram,
//             in LDS first when it has at most CL_LDS_BINS bins), then one workgroup folds the partials in index order: the same bits on every call
// Double arithmetic is written in the contract's order; the library builds with -ffp-contract=off, so nothing is fused.
#include "raycast.hpp"
#include "raycast_dev.hpp"

namespace {

inline unsigned cl_grid(int64_t n) { return (unsigned)((n + RC_BLOCK - 1) / RC_BLOCK); }

// the contract's Point rule: false when the point has no face by rule
__device__ __forceinline__ bool cl_point(const RcFrame& fr, int has_frame, const float* __restrict__ pts, int64_t i, double* p) {
    const float f[3] = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
    bool ok = isfinite(f[0]) && isfinite(f[1]) && isfinite(f[2]);
    const double x[3] = {(double)f[0], (double)f[1], (double)f[2]};
    for (int k = 0; k < 3; k++) {
        p[k] = has_frame ? ((fr.rot[3 * k] * x[0] + fr.rot[3 * k + 1] * x[1]) + fr.rot[3 * k + 2] * x[2]) + fr.pos[k] : x[k];
        ok = ok && fabs(p[k]) < 0x1p128;   // (false for NaN)
    }
    return ok;
}

// the contract's Box bound of a float box
__device__ __forceinline__ double cl_box(const double* p, const float* lo, const float* hi) {
    double e[3];
    for (int k = 0; k < 3; k++) e[k] = fmax(fmax((double)lo[k] - p[k], p[k] - (double)hi[k]), 0.0);
    return (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2];
}

__device__ __forceinline__ float cl_round_down(double x) {   // x >= 0: the largest float <= x
    float f = (float)x;
    if ((double)f > x) f = __uint_as_float(__float_as_uint(f) - 1u);
    return f;
}

__device__ __forceinline__ double cl_unit(double x) { return x > 0.0 ? (x < 1.0 ? x : 1.0) : 0.0; }   // held to [0, 1]; NaN -> 0

// the contract's Face rule: q, the closest point of the face (a, b, c relative to the query) by the region method
__device__ __forceinline__ void cl_closest(const double* a, const double* b, const double* c, double* q) {
    double ab[3], ac[3], ma[3], mb[3], mc[3];
    for (int k = 0; k < 3; k++) { ab[k] = b[k] - a[k]; ac[k] = c[k] - a[k]; ma[k] = -a[k]; mb[k] = -b[k]; mc[k] = -c[k]; }
    const double d1 = rc_dot(ab, ma), d2 = rc_dot(ac, ma);
    if (d1 <= 0.0 && d2 <= 0.0) { q[0] = a[0]; q[1] = a[1]; q[2] = a[2]; return; }
    const double d3 = rc_dot(ab, mb), d4 = rc_dot(ac, mb);
    if (d3 >= 0.0 && d4 <= d3) { q[0] = b[0]; q[1] = b[1]; q[2] = b[2]; return; }
    const double vc = d1 * d4 - d3 * d2;
    const double den_ab = d1 - d3;
    if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0 && den_ab != 0.0) {
        const double v = cl_unit(d1 / den_ab);
        for (int k = 0; k < 3; k++) q[k] = a[k] + v * ab[k];
        return;
    }
    const double d5 = rc_dot(ab, mc), d6 = rc_dot(ac, mc);
    if (d6 >= 0.0 && d5 <= d6) { q[0] = c[0]; q[1] = c[1]; q[2] = c[2]; return; }
    const double vb = d5 * d2 - d1 * d6;
    const double den_ac = d2 - d6;
    if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0 && den_ac != 0.0) {
        const double w = cl_unit(d2 / den_ac);
        for (int k = 0; k < 3; k++) q[k] = a[k] + w * ac[k];
        return;
    }
    const double va = d3 * d6 - d5 * d4;
    const double e43 = d4 - d3, e56 = d5 - d6;
    const double den_bc = e43 + e56;
    if (va <= 0.0 && e43 >= 0.0 && e56 >= 0.0 && den_bc != 0.0) {
        const double w = cl_unit(e43 / den_bc);
        for (int k = 0; k < 3; k++) q[k] = b[k] + w * (c[k] - b[k]);
        return;
    }
    const double sum = (va + vb) + vc;
    const double inv = sum != 0.0 ? 1.0 / sum : 0.0;
    const double v = cl_unit(vb * inv);
    const double w1 = cl_unit(vc * inv), rest = 1.0 - v;
    const double w = w1 < rest ? w1 : rest;
    for (int k = 0; k < 3; k++) q[k] = (a[k] + ab[k] * v) + ac[k] * w;
}

__global__ void __launch_bounds__(RC_BLOCK) rc_closest_kernel(RcFrame fr, int has_frame, const float* __restrict__ pts,
                                                              int64_t n_pts, double r2, const float* __restrict__ vtx, const int32_t* __restrict__ faces,
                                                              const RcNode* __restrict__ nodes, int64_t n_in, double* __restrict__ d2_out,
                                                              float* __restrict__ dist_out, int32_t* __restrict__ face_out, float* __restrict__ xyz_out,
                                                              int8_t* __restrict__ side_out, uint8_t* __restrict__ status_out) {
    const int64_t i = (int64_t)blockIdx.x * RC_BLOCK + threadIdx.x;
    if (i >= n_pts) return;
    double p[3];
    const bool ok = cl_point(fr, has_frame, pts, i, p);
    double best = r2;              // the bound: r2 until a face counts, then the best D
    int32_t best_f = -1;
    double best_q[3] = {0.0, 0.0, 0.0};
    int best_side = 0;
    if (ok && n_in > 0) {
        int32_t stack[RC_STACK];
        float stack_key[RC_STACK];
        int sp = 0;
        int32_t cur = 0;
        for (;;) {
            if (cur < 0) {   // a face
                const int32_t f = ~cur;
                float lo[3], hi[3];
                double A[3][3];
                for (int k = 0; k < 3; k++) {
                    const float* v = vtx + 3 * (int64_t)faces[3 * (int64_t)f + k];
                    for (int j = 0; j < 3; j++) {
                        const float x = v[j];
                        lo[j] = k ? fminf(lo[j], x) : x;
                        hi[j] = k ? fmaxf(hi[j], x) : x;
                        A[k][j] = (double)x - p[j];
                    }
                }
                double q[3];
                cl_closest(A[0], A[1], A[2], q);
                const double D = fmax(rc_dot(q, q), cl_box(p, lo, hi));
                // a face met twice (the single-face tree) ties with itself and changes nothing
                if (D < best || (D == best && (best_f < 0 || f < best_f))) {
                    best = D; best_f = f;
                    best_q[0] = q[0]; best_q[1] = q[1]; best_q[2] = q[2];
                    const double u[3] = {A[1][0] - A[0][0], A[1][1] - A[0][1], A[1][2] - A[0][2]};
                    const double w[3] = {A[2][0] - A[0][0], A[2][1] - A[0][1], A[2][2] - A[0][2]};
                    const double ma[3] = {-A[0][0], -A[0][1], -A[0][2]};
                    double n[3];
                    rc_cross(u, w, n);
                    const double sd = rc_dot(n, ma);
                    best_side = sd > 0.0 ? 1 : (sd < 0.0 ? -1 : 0);
                }
            } else {
                const RcNode& nd = nodes[cur];
                const double l0 = cl_box(p, nd.lo[0], nd.hi[0]), l1 = cl_box(p, nd.lo[1], nd.hi[1]);
                const bool h0 = !(l0 > best), h1 = !(l1 > best);
                const int32_t c0 = nd.child[0], c1 = nd.child[1];
                if (h0 && h1) {
                    const bool first0 = l0 <= l1;       // the nearer child first: its faces prune the other
                    stack[sp] = first0 ? c1 : c0;
                    stack_key[sp] = cl_round_down(first0 ? l1 : l0);
                    sp++;
                    cur = first0 ? c0 : c1;
                    continue;
                }
                if (h0 || h1) { cur = h0 ? c0 : c1; continue; }
            }
            // next entry whose bound has not been overtaken
            bool found = false;
            while (sp > 0) {
                sp--;
                if (!((double)stack_key[sp] > best)) { cur = stack[sp]; found = true; break; }
            }
            if (!found) break;
        }
    }
    const float nanf32 = __uint_as_float(0x7FC00000u);
    const bool have = best_f >= 0;
    d2_out[i] = have ? best : -1.0;
    dist_out[i] = have ? (float)sqrt(best) : -1.0f;
    face_out[i] = best_f;
    for (int k = 0; k < 3; k++) xyz_out[3 * i + k] = have ? (float)(p[k] + best_q[k]) : nanf32;
    side_out[i] = (int8_t)(have ? best_side : 0);
    status_out[i] = have ? 0 : (ok ? 1 : 2);
}

// ---- the reduction -------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void cl_fold(ClStatsDev& a, const ClStatsDev& b) {
    a.sum += b.sum; a.sum2 += b.sum2;
    a.n_face += b.n_face; a.n_not_finite += b.n_not_finite; a.n_no_face += b.n_no_face;
    a.max_dist = fmaxf(a.max_dist, b.max_dist);
}

// the workgroup's tree over s[0 .. RC_BLOCK): s[t] += s[t + stride], stride = RC_BLOCK / 2 .. 1 -- a fixed order
__device__ __forceinline__ void cl_tree(ClStatsDev* s) {
    for (int stride = RC_BLOCK / 2; stride >= 1; stride >>= 1) {
        __syncthreads();
        if ((int)threadIdx.x < stride) cl_fold(s[threadIdx.x], s[threadIdx.x + stride]);
    }
    __syncthreads();
}

__global__ void __launch_bounds__(RC_BLOCK) cl_stats_kernel(const float* __restrict__ dist, const uint8_t* __restrict__ status, int64_t n_pts, float bin_width,
                                                            int32_t n_bins, ClStatsDev* __restrict__ part, unsigned long long* hist) {
    __shared__ ClStatsDev s[RC_BLOCK];
    __shared__ uint32_t s_hist[CL_LDS_BINS + 1];                  // [n_bins]: the overflow count
    const bool in_lds = n_bins <= CL_LDS_BINS;                    // most of a cloud falls into a few bins: count them here, not on one global address
    if (in_lds) {
        for (int b = threadIdx.x; b <= n_bins; b += RC_BLOCK) s_hist[b] = 0u;
        __syncthreads();
    }
    const int64_t i = (int64_t)blockIdx.x * RC_BLOCK + threadIdx.x;
    ClStatsDev me = {0.0, 0.0, 0, 0, 0, 0.0f, 0};
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
    cl_tree(s);                                                   // (its barriers also complete s_hist)
    if (threadIdx.x == 0) part[blockIdx.x] = s[0];
    if (in_lds)
        for (int b = threadIdx.x; b <= n_bins; b += RC_BLOCK)
            if (s_hist[b]) atomicAdd(&hist[b], (unsigned long long)s_hist[b]);
}

// one workgroup: lane t folds partials t, t + RC_BLOCK, ... in that order, then the tree
__global__ void __launch_bounds__(RC_BLOCK) cl_fold_kernel(const ClStatsDev* __restrict__ part, int64_t n_part, ClStatsDev* __restrict__ res) {
    __shared__ ClStatsDev s[RC_BLOCK];
    ClStatsDev me = {0.0, 0.0, 0, 0, 0, 0.0f, 0};
    for (int64_t j = threadIdx.x; j < n_part; j += RC_BLOCK) cl_fold(me, part[j]);
    s[threadIdx.x] = me;
    cl_tree(s);
    if (threadIdx.x == 0) res[0] = s[0];
}

}  // namespace

void cl_launch_query(hipStream_t s, const RcFrame& fr, int has_frame, const float* pts, int64_t n_pts, double r2, const float* vtx,
                     const int32_t* faces, const RcNode* nodes, int64_t n_in, double* d2, float* dist, int32_t* face, float* xyz, int8_t* side,
                     uint8_t* status) {
    if (n_pts > 0)
        rc_closest_kernel<<<cl_grid(n_pts), RC_BLOCK, 0, s>>>(fr, has_frame, pts, n_pts, r2, vtx, faces, nodes, n_in, d2, dist, face, xyz, side, status);
}

int64_t cl_stats_blocks(int64_t n_pts) { return (n_pts + RC_BLOCK - 1) / RC_BLOCK; }

void cl_launch_stats(hipStream_t s, const float* dist, const uint8_t* status, int64_t n_pts, float bin_width, int32_t n_bins, ClStatsDev* part,
                     unsigned long long* hist, ClStatsDev* res) {
    const int64_t blocks = cl_stats_blocks(n_pts);
    if (blocks > 0) cl_stats_kernel<<<(unsigned)blocks, RC_BLOCK, 0, s>>>(dist, status, n_pts, bin_width, n_bins, part, hist);
    cl_fold_kernel<<<1, RC_BLOCK, 0, s>>>(part, blocks, res);
}
