// Euclidean clusters of the index's cloud for gfx950 (include/immesh_nearest.h, the Clusters rule, is the exact contract these kernels implement).
//   kind      one lane per cloud point: finite or not, core or not from the Count launch's counts (knn_kernels.hip, cloud mode), parent[i] = i.
//   join      the hot launch.  Every core lane runs the offering walk of raycast_dev.hpp (dq_walk_offer) with r2 as its bound throughout; its sink
//             takes a leaf j only when j < i, j is core and D <= r2 -- D between two cloud points is symmetric bit for bit, so the lower index of
//             every pair is enough -- and unites the two in the lock-free union-find of pass_dev.hpp (tp_union).  Hooks go larger root under smaller,
//             so a class' root is its smallest index, which is its label.  The lane remembers an index that it has seen as its class' root and
//             skips the union when parent[j] is that index: j then hangs under a member of the lane's class, and classes only ever merge.
//   flatten   root[i] for the core lanes: strictly downwards, as the topology's.
//   border    the lanes that are finite and not core walk with a one-best sink over the core leaves: r2 until a candidate is held, its D from then
//             on; a leaf replaces the holder when it is smaller under (D, index).  The walk enters a node at L == bound, so a lower index at the
//             same D is still met.
//   table     behind the exclusive scan of "core and its own root": the numbers, n_points / n_core by integer atomicAdd, the box by atomicMin /
//             atomicMax on order-preserving keys, folded cluster by cluster within a wavefront first, as the topology's component table is.
//   mask      the Select rule's mask from the per-cluster keep that the host decided.
// Double arithmetic is written in the contract's order; the library builds with -ffp-contract=off, so nothing is fused.  Plain C++, vector stores and
// integer atomics only: no floating-point atomic, no cross-lane operation on a distance.
#include "raycast.hpp"
#include "raycast_dev.hpp"
#include "knn_dev.hpp"
#include "pass_dev.hpp"

namespace {

constexpr uint32_t CL_KEY_NONE_LO = 0xFFFFFFFFu, CL_KEY_NONE_HI = 0u;
constexpr int CL_FOLD_ROUNDS = 4;   // clusters folded per wavefront before the lanes left over send their own atomics

__device__ __forceinline__ void cl_widen(const float* __restrict__ cloud, int64_t i, double* p) {
    for (int k = 0; k < 3; k++) p[k] = (double)cloud[3 * i + k];
}

__global__ void __launch_bounds__(RC_BLOCK) cl_kind_kernel(const float* __restrict__ cloud, int64_t n, const int32_t* __restrict__ count, int32_t min_neighbours,
                                                           uint8_t* __restrict__ core, uint8_t* __restrict__ kind, int32_t* __restrict__ parent,
                                                           int32_t* __restrict__ root) {
    const int64_t i = (int64_t)blockIdx.x * RC_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint8_t k = !pd_finite3(cloud, i) ? 3 : (!count || count[i] >= min_neighbours) ? 0 : 2;
    core[i] = k;
    kind[i] = k;
    parent[i] = (int32_t)i;
    root[i] = -1;
}

struct ClJoiner {
    const float* __restrict__ cloud;
    const uint8_t* __restrict__ core;
    int32_t* parent;
    const double* p;
    double r2;
    int32_t i, seen;   // seen: an index that was the root of i's class when the lane last looked
    bool bad;
    __device__ __forceinline__ double offer(int32_t j) {
        if (j < i && core[j] == 0 && kn_dist(cloud, p, j) <= r2 && tp_load(parent + j) != seen) {
            if (!tp_union(parent, i, j)) bad = true;
            int64_t steps = 2 * ((int64_t)i + 2);
            const int32_t r = tp_find(parent, i, steps);
            if (r < 0) bad = true;
            else seen = r;
        }
        return r2;
    }
};

__global__ void __launch_bounds__(RC_BLOCK) cl_join_kernel(const float* __restrict__ cloud, int64_t n, double r2, const RcNode* __restrict__ nodes, int64_t n_in,
                                                           const uint8_t* __restrict__ core, int32_t* parent, unsigned long long* cnt) {
    const int64_t i = (int64_t)blockIdx.x * RC_BLOCK + threadIdx.x;
    if (i >= n || core[i] != 0) return;
    double p[3];
    cl_widen(cloud, i, p);
    ClJoiner join = {cloud, core, parent, p, r2, (int32_t)i, tp_load(parent + i), false};
    dq_walk_offer(nodes, n_in, p, r2, join);
    if (join.bad) atomicMax(cnt + CL_ERROR, 1ull);
}

__global__ void __launch_bounds__(RC_BLOCK) cl_flatten_kernel(int64_t n, const uint8_t* __restrict__ core, const int32_t* __restrict__ parent,
                                                              int32_t* __restrict__ root, int32_t* __restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * RC_BLOCK + threadIdx.x;
    if (i >= n) return;
    int32_t x = -1;
    if (core[i] == 0) {
        x = (int32_t)i;
        for (int32_t q = parent[x]; q != x; q = parent[x]) x = q;   // strictly downwards: it ends
        root[i] = x;
    }
    flag[i] = x == (int32_t)i ? 1 : 0;
}

struct ClNearestCore {
    const float* __restrict__ cloud;
    const uint8_t* __restrict__ core;
    const double* p;
    double r2, best;
    int32_t id;
    __device__ __forceinline__ double offer(int32_t j) {
        if (core[j] == 0) {
            const double D = kn_dist(cloud, p, j);
            if (D <= r2 && (id < 0 || D < best || (D == best && j < id))) { best = D; id = j; }
        }
        return id < 0 ? r2 : best;
    }
};

__global__ void __launch_bounds__(RC_BLOCK) cl_border_kernel(const float* __restrict__ cloud, int64_t n, double r2, const RcNode* __restrict__ nodes, int64_t n_in,
                                                             const uint8_t* __restrict__ core, uint8_t* __restrict__ kind, int32_t* root) {
    const int64_t i = (int64_t)blockIdx.x * RC_BLOCK + threadIdx.x;
    if (i >= n || core[i] != 2) return;
    double p[3];
    cl_widen(cloud, i, p);
    ClNearestCore sink = {cloud, core, p, r2, 0.0, -1};
    dq_walk_offer(nodes, n_in, p, r2, sink);
    if (sink.id < 0) return;                  // noise: kind stays 2, root stays -1
    kind[i] = 1;
    root[i] = root[sink.id];                  // (a core lane's root: the flatten launch wrote it, this launch writes the others' only)
}

__global__ void __launch_bounds__(RC_BLOCK) cl_preset_kernel(int64_t n_clusters, int32_t* __restrict__ first, int32_t* __restrict__ npts, int32_t* __restrict__ ncore,
                                                             uint32_t* __restrict__ boxkey) {
    const int64_t c = (int64_t)blockIdx.x * RC_BLOCK + threadIdx.x;
    if (c >= n_clusters) return;
    first[c] = -1;
    npts[c] = 0;
    ncore[c] = 0;
    for (int j = 0; j < 3; j++) { boxkey[6 * c + j] = CL_KEY_NONE_LO; boxkey[6 * c + 3 + j] = CL_KEY_NONE_HI; }
}

__global__ void __launch_bounds__(RC_BLOCK) cl_table_kernel(const float* __restrict__ cloud, int64_t n, const uint8_t* __restrict__ kind, const int32_t* __restrict__ root,
                                                            const int32_t* __restrict__ num, int64_t n_clusters, int32_t* __restrict__ label,
                                                            int32_t* __restrict__ first, int32_t* npts, int32_t* ncore, uint32_t* boxkey, unsigned long long* cnt) {
    __shared__ uint32_t lds[RC_BLOCK / 64];
    const int64_t i = (int64_t)blockIdx.x * RC_BLOCK + threadIdx.x;
    const bool in = i < n;
    const uint8_t k = in ? kind[i] : 255;
    int32_t c = -1;
    uint32_t key[3] = {0u, 0u, 0u};
    if (in) {
        const int32_t r = k <= 1 ? root[i] : -1;
        if (r >= 0 && r < n) {
            const int32_t m = num[r];
            if (m >= 0 && m < n_clusters) c = m;          // (the scan of these flags never gives another)
        }
        label[i] = c;
        if (c >= 0) {
            if (r == (int32_t)i) first[c] = (int32_t)i;
            for (int j = 0; j < 3; j++) key[j] = pd_key(cloud[3 * i + j]);   // a member is finite
        }
    }
    // one atomic per word, wavefront and cluster for the first CL_FOLD_ROUNDS clusters of a wavefront (a sheet's 64 points are one round whatever
    // their order); the lanes left over send their own: those words are not contended.  Every lane takes part in the shuffles.
    const bool is_core = k == 0;
    unsigned long long todo = __ballot(c >= 0);
    for (int round = 0; todo != 0 && round < CL_FOLD_ROUNDS; round++) {
        const int leader = __ffsll((long long)todo) - 1;
        const int32_t c0 = __shfl(c, leader, 64);
        const bool mine = c == c0;
        const unsigned long long m = __ballot(mine), mc = __ballot(mine && is_core);
        uint32_t l[3], h[3];
        for (int j = 0; j < 3; j++) {
            l[j] = pd_wave_min(mine ? key[j] : CL_KEY_NONE_LO);
            h[j] = pd_wave_max(mine ? key[j] : CL_KEY_NONE_HI);
        }
        if ((int)(threadIdx.x & 63) == leader) {
            atomicAdd(npts + c0, (int32_t)__popcll(m));
            if (mc) atomicAdd(ncore + c0, (int32_t)__popcll(mc));
            for (int j = 0; j < 3; j++) {
                atomicMin(boxkey + 6 * (int64_t)c0 + j, l[j]);
                atomicMax(boxkey + 6 * (int64_t)c0 + 3 + j, h[j]);
            }
        }
        todo &= ~m;
    }
    if ((todo >> (threadIdx.x & 63)) & 1ull) {
        atomicAdd(npts + c, 1);
        if (is_core) atomicAdd(ncore + c, 1);
        for (int j = 0; j < 3; j++) {
            atomicMin(boxkey + 6 * (int64_t)c + j, key[j]);
            atomicMax(boxkey + 6 * (int64_t)c + 3 + j, key[j]);
        }
    }
    for (int q = 0; q < 4; q++) pd_block_add<uint32_t>(k == q ? 1u : 0u, cnt + q, lds);
}

__global__ void __launch_bounds__(RC_BLOCK) cl_unkey_kernel(int64_t n_words, const uint32_t* __restrict__ boxkey, float* __restrict__ box) {
    const int64_t w = (int64_t)blockIdx.x * RC_BLOCK + threadIdx.x;
    if (w < n_words) box[w] = pd_unkey(boxkey[w]);       // (every cluster has a core member, which is finite: no key is a preset)
}

// the four counts are a partition of the cloud: kept, in a cluster and not kept, noise and not kept, not finite
__global__ void __launch_bounds__(RC_BLOCK) cl_mask_kernel(int64_t n, const uint8_t* __restrict__ kind, const int32_t* __restrict__ label,
                                                           const int32_t* __restrict__ keepc, int64_t n_clusters, int32_t keep_noise, int32_t* __restrict__ flag,
                                                           uint8_t* __restrict__ keep8, unsigned long long* cnt) {
    __shared__ uint32_t lds[RC_BLOCK / 64];
    const int64_t i = (int64_t)blockIdx.x * RC_BLOCK + threadIdx.x;
    const bool in = i < n;
    const uint8_t k = in ? kind[i] : 255;
    const int32_t c = in ? label[i] : -1;
    const bool member = k <= 1 && c >= 0 && c < n_clusters;
    const bool keep = member ? keepc[c] != 0 : (k == 2 && keep_noise != 0);
    if (in) { flag[i] = keep ? 1 : 0; keep8[i] = keep ? 1 : 0; }
    pd_block_add<uint32_t>(keep ? 1u : 0u, cnt + 0, lds);
    pd_block_add<uint32_t>(k <= 1 && !keep ? 1u : 0u, cnt + 1, lds);
    pd_block_add<uint32_t>(k == 2 && !keep ? 1u : 0u, cnt + 2, lds);
    pd_block_add<uint32_t>(k == 3 ? 1u : 0u, cnt + 3, lds);
}

}  // namespace

void cl_launch_kind(hipStream_t s, const float* cloud, int64_t n, const int32_t* count, int32_t min_neighbours, uint8_t* core, uint8_t* kind, int32_t* parent,
                    int32_t* root) {
    if (n > 0) cl_kind_kernel<<<rc_grid(n), RC_BLOCK, 0, s>>>(cloud, n, count, min_neighbours, core, kind, parent, root);
}

void cl_launch_join(hipStream_t s, const float* cloud, int64_t n, double r2, const RcNode* nodes, int64_t n_in, const uint8_t* core, int32_t* parent,
                    unsigned long long* cnt) {
    if (n > 0 && n_in > 0) cl_join_kernel<<<rc_grid(n), RC_BLOCK, 0, s>>>(cloud, n, r2, nodes, n_in, core, parent, cnt);
}

void cl_launch_flatten(hipStream_t s, int64_t n, const uint8_t* core, const int32_t* parent, int32_t* root, int32_t* flag) {
    if (n > 0) cl_flatten_kernel<<<rc_grid(n), RC_BLOCK, 0, s>>>(n, core, parent, root, flag);
}

void cl_launch_border(hipStream_t s, const float* cloud, int64_t n, double r2, const RcNode* nodes, int64_t n_in, const uint8_t* core, uint8_t* kind,
                      int32_t* root) {
    if (n > 0 && n_in > 0) cl_border_kernel<<<rc_grid(n), RC_BLOCK, 0, s>>>(cloud, n, r2, nodes, n_in, core, kind, root);
}

void cl_launch_preset(hipStream_t s, int64_t n_clusters, int32_t* first, int32_t* npts, int32_t* ncore, uint32_t* boxkey) {
    if (n_clusters > 0) cl_preset_kernel<<<rc_grid(n_clusters), RC_BLOCK, 0, s>>>(n_clusters, first, npts, ncore, boxkey);
}

void cl_launch_table(hipStream_t s, const float* cloud, int64_t n, const uint8_t* kind, const int32_t* root, const int32_t* num, int64_t n_clusters,
                     int32_t* label, int32_t* first, int32_t* npts, int32_t* ncore, uint32_t* boxkey, unsigned long long* cnt) {
    if (n > 0) cl_table_kernel<<<rc_grid(n), RC_BLOCK, 0, s>>>(cloud, n, kind, root, num, n_clusters, label, first, npts, ncore, boxkey, cnt);
}

void cl_launch_unkey(hipStream_t s, int64_t n_clusters, const uint32_t* boxkey, float* box) {
    if (n_clusters > 0) cl_unkey_kernel<<<rc_grid(6 * n_clusters), RC_BLOCK, 0, s>>>(6 * n_clusters, boxkey, box);
}

void cl_launch_mask(hipStream_t s, int64_t n, const uint8_t* kind, const int32_t* label, const int32_t* keepc, int64_t n_clusters, int32_t keep_noise,
                    int32_t* flag, uint8_t* keep8, unsigned long long* cnt) {
    if (n > 0) cl_mask_kernel<<<rc_grid(n), RC_BLOCK, 0, s>>>(n, kind, label, keepc, n_clusters, keep_noise, flag, keep8, cnt);
}
