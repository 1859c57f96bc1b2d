// k nearest neighbours, radius counts, outlier masks and the compaction of their apply for gfx950 (include/immesh_nearest.h, the Neighbours, Count and
// Outliers rules, is the exact contract these kernels implement).
//   knn       one query per lane on the offering walk of raycast_dev.hpp (dq_walk_offer) over the index's hierarchy; the lane keeps the k best
//             (D, index) pairs as a sorted insertion list in private memory beside the walk's stack; the walk's bound is r2 until the list is
//             full and its k-th D from then on.  The list and the choice of its compile-time capacity (KN_SIZES) live in knn_dev.hpp, which the normals share.
//             Cloud mode reads query i from the cloud itself, never offers index i, and folds the mean of the list's distances into the same lane.
//   count     the same walk with r2 as its bound throughout; the sink counts.
//   masks     one lane per cloud point; the four counts are integer folds (pass_dev.hpp), one atomic per workgroup and count.
//   compact   one lane per cloud point behind the renderer's exclusive scan of the mask.
// Double arithmetic is written in the contract's order; the library builds with -ffp-contract=off, so nothing is fused.  Plain C++ and vector
// stores only: no floating-point atomic, no cross-lane operation on a distance.
#include "raycast.hpp"
#include "raycast_dev.hpp"
#include "knn_dev.hpp"
#include "pass_dev.hpp"

namespace {

// query i of a launch: mode 2 reads cloud point i where it lies (no frame); false when the query has no candidates by rule
template <int MODE>
__device__ __forceinline__ bool kn_query(const RcFrame& fr, const float* __restrict__ pts, const float* __restrict__ cloud, int64_t i, double* p) {
    return dq_point(fr, MODE == 1, MODE == 2 ? cloud : pts, i, p);
}

struct KnCounter {
    const float* __restrict__ cloud;
    const double* p;
    double r2;
    int32_t skip, n;
    __device__ __forceinline__ double offer(int32_t j) {
        if (j != skip && kn_dist(cloud, p, j) <= r2) n++;
        return r2;
    }
};

template <int MODE, int CAP>
__global__ void __launch_bounds__(RC_BLOCK) kn_knn_kernel(RcFrame fr, const float* __restrict__ pts, int64_t n, int32_t k, double r2,
                                                          const float* __restrict__ cloud, const RcNode* __restrict__ nodes, int64_t n_in,
                                                          int32_t* __restrict__ count_out, int32_t* __restrict__ index_out, double* __restrict__ d2_out,
                                                          double* __restrict__ mean_out, uint8_t* __restrict__ status_out) {
    const int64_t i = (int64_t)blockIdx.x * RC_BLOCK + threadIdx.x;
    if (i >= n) return;
    double p[3];
    const bool ok = kn_query<MODE>(fr, pts, cloud, i, p);
    KnList<CAP> list;
    list.cloud = cloud; list.p = p; list.r2 = r2; list.k = k; list.skip = MODE == 2 ? (int32_t)i : -1; list.n = 0;
    if (ok && n_in > 0) dq_walk_offer(nodes, n_in, p, r2, list);
    const int32_t cnt = list.n;
    count_out[i] = cnt;
    if (index_out)
        for (int32_t j = 0; j < k; j++) {
            index_out[i * k + j] = j < cnt ? list.id[j] : -1;
            d2_out[i * k + j] = j < cnt ? list.d[j] : -1.0;
        }
    if (MODE == 2) {
        double sum = 0.0;
        for (int32_t j = 0; j < cnt; j++) sum += sqrt(list.d[j]);
        mean_out[i] = cnt > 0 ? sum / (double)cnt : -1.0;
    }
    status_out[i] = cnt > 0 ? 0 : (ok ? 1 : 2);
}

template <int MODE>
__global__ void __launch_bounds__(RC_BLOCK) kn_count_kernel(RcFrame fr, const float* __restrict__ pts, int64_t n, double r2, const float* __restrict__ cloud,
                                                            const RcNode* __restrict__ nodes, int64_t n_in, int32_t* __restrict__ count_out,
                                                            uint8_t* __restrict__ status_out) {
    const int64_t i = (int64_t)blockIdx.x * RC_BLOCK + threadIdx.x;
    if (i >= n) return;
    double p[3];
    const bool ok = kn_query<MODE>(fr, pts, cloud, i, p);
    KnCounter counter = {cloud, p, r2, MODE == 2 ? (int32_t)i : -1, 0};
    if (ok && n_in > 0) dq_walk_offer(nodes, n_in, p, r2, counter);
    count_out[i] = counter.n;
    status_out[i] = counter.n > 0 ? 0 : (ok ? 1 : 2);
}

// ---- the masks ----------------------------------------------------------------------------------------------------------------------------------
// the four counts are a partition of the cloud: kept, used but above the threshold, isolated (finite, count == 0), not finite
__global__ void __launch_bounds__(RC_BLOCK) kn_mask_statistical_kernel(const double* __restrict__ mean, const uint8_t* __restrict__ status, int64_t n,
                                                                       double threshold, int32_t* __restrict__ flag, uint8_t* __restrict__ keep8,
                                                                       unsigned long long* cnt) {
    __shared__ uint32_t lds[RC_BLOCK / 64];
    const int64_t i = (int64_t)blockIdx.x * RC_BLOCK + threadIdx.x;
    const bool in = i < n;
    const uint8_t st = in ? status[i] : 0;
    const bool keep = in && st == 0 && mean[i] <= threshold;        // used_i && mean_i <= threshold
    if (in) { flag[i] = keep ? 1 : 0; keep8[i] = keep ? 1 : 0; }
    pd_block_add<uint32_t>(keep ? 1u : 0u, cnt + 0, lds);
    pd_block_add<uint32_t>(in && !keep && st == 0 ? 1u : 0u, cnt + 1, lds);
    pd_block_add<uint32_t>(in && st == 1 ? 1u : 0u, cnt + 2, lds);
    pd_block_add<uint32_t>(in && st == 2 ? 1u : 0u, cnt + 3, lds);
}

// isolated counts the finite points without a neighbour; with min_neighbours == 0 they are kept as well, so here it is not a class of its own
__global__ void __launch_bounds__(RC_BLOCK) kn_mask_radius_kernel(const int32_t* __restrict__ count, const uint8_t* __restrict__ status, int64_t n,
                                                                  int32_t min_neighbours, int32_t* __restrict__ flag, uint8_t* __restrict__ keep8,
                                                                  unsigned long long* cnt) {
    __shared__ uint32_t lds[RC_BLOCK / 64];
    const int64_t i = (int64_t)blockIdx.x * RC_BLOCK + threadIdx.x;
    const bool in = i < n;
    const uint8_t st = in ? status[i] : 0;
    const bool keep = in && st != 2 && count[i] >= min_neighbours;  // finite_i && count_i >= min_neighbours
    if (in) { flag[i] = keep ? 1 : 0; keep8[i] = keep ? 1 : 0; }
    pd_block_add<uint32_t>(keep ? 1u : 0u, cnt + 0, lds);
    pd_block_add<uint32_t>(in && !keep && st != 2 ? 1u : 0u, cnt + 1, lds);
    pd_block_add<uint32_t>(in && st == 1 ? 1u : 0u, cnt + 2, lds);
    pd_block_add<uint32_t>(in && st == 2 ? 1u : 0u, cnt + 3, lds);
}

__global__ void __launch_bounds__(RC_BLOCK) kn_compact_kernel(const float* __restrict__ pts, const int32_t* __restrict__ flag, const int32_t* __restrict__ off,
                                                              int64_t n, int64_t n_kept, float* __restrict__ out, int32_t* __restrict__ kept) {
    const int64_t i = (int64_t)blockIdx.x * RC_BLOCK + threadIdx.x;
    if (i >= n || !flag[i]) return;
    const int64_t o = off[i];
    if (o < 0 || o >= n_kept) return;   // (the scan of this mask never gives one)
    for (int k = 0; k < 3; k++) out[3 * o + k] = pts[3 * i + k];
    kept[o] = (int32_t)i;
}

template <int MODE>
void kn_knn_sized(hipStream_t s, const RcFrame& fr, const float* pts, int64_t n, int32_t k, double r2, const float* cloud, const RcNode* nodes, int64_t n_in,
                  int32_t* count, int32_t* index, double* d2, double* mean, uint8_t* status) {
    // KN_SIZES (knn_dev.hpp): the list's capacities
    kn_sized(k, [&](auto cap) {
        kn_knn_kernel<MODE, decltype(cap)::value><<<rc_grid(n), RC_BLOCK, 0, s>>>(fr, pts, n, k, r2, cloud, nodes, n_in, count, index, d2, mean, status);
    });
}

}  // namespace

void kn_launch_knn(hipStream_t s, const RcFrame& fr, int mode, const float* pts, int64_t n, int32_t k, double r2, const float* cloud, const RcNode* nodes,
                   int64_t n_in, int32_t* count, int32_t* index, double* d2, double* mean, uint8_t* status) {
    if (n <= 0 || k < 1 || k > 64) return;
    if (!index || !d2) { index = nullptr; d2 = nullptr; }
    if (mode == 2) kn_knn_sized<2>(s, fr, pts, n, k, r2, cloud, nodes, n_in, count, index, d2, mean, status);
    else if (mode == 1) kn_knn_sized<1>(s, fr, pts, n, k, r2, cloud, nodes, n_in, count, index, d2, mean, status);
    else kn_knn_sized<0>(s, fr, pts, n, k, r2, cloud, nodes, n_in, count, index, d2, mean, status);
}

void kn_launch_count(hipStream_t s, const RcFrame& fr, int mode, const float* pts, int64_t n, double r2, const float* cloud, const RcNode* nodes, int64_t n_in,
                     int32_t* count, uint8_t* status) {
    if (n <= 0) return;
    if (mode == 2) kn_count_kernel<2><<<rc_grid(n), RC_BLOCK, 0, s>>>(fr, pts, n, r2, cloud, nodes, n_in, count, status);
    else if (mode == 1) kn_count_kernel<1><<<rc_grid(n), RC_BLOCK, 0, s>>>(fr, pts, n, r2, cloud, nodes, n_in, count, status);
    else kn_count_kernel<0><<<rc_grid(n), RC_BLOCK, 0, s>>>(fr, pts, n, r2, cloud, nodes, n_in, count, status);
}

void kn_launch_mask_statistical(hipStream_t s, const double* mean, const uint8_t* status, int64_t n, double threshold, int32_t* flag, uint8_t* keep8,
                                unsigned long long* cnt) {
    if (n > 0) kn_mask_statistical_kernel<<<rc_grid(n), RC_BLOCK, 0, s>>>(mean, status, n, threshold, flag, keep8, cnt);
}

void kn_launch_mask_radius(hipStream_t s, const int32_t* count, const uint8_t* status, int64_t n, int32_t min_neighbours, int32_t* flag, uint8_t* keep8,
                           unsigned long long* cnt) {
    if (n > 0) kn_mask_radius_kernel<<<rc_grid(n), RC_BLOCK, 0, s>>>(count, status, n, min_neighbours, flag, keep8, cnt);
}

void kn_launch_compact(hipStream_t s, const float* pts, const int32_t* flag, const int32_t* off, int64_t n, int64_t n_kept, float* out, int32_t* kept) {
    if (n > 0) kn_compact_kernel<<<rc_grid(n), RC_BLOCK, 0, s>>>(pts, flag, off, n, n_kept, out, kept);
}
