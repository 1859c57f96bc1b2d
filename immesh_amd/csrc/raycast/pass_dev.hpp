// Device primitives shared by the kernels of the passes over the caster's snapshot (topology/, simplify/, smooth/, intersect/, and the sampler and the
// build of raycast/) and by the clusters of the cloud index: the folds of a count into one word, the capped grid, the float keys, the lock-free
// union-find, the rule "a face counts" and the run kernels of sorted 64-bit keys.  Integers, min / max and bit patterns only: nothing here depends on the order of anything.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "raycast_dev.hpp"

namespace {

// ---- wavefront folds: every lane of the wavefront calls, every lane gets the result ----------------------------------------------------------
__device__ __forceinline__ uint32_t pd_wave_sum(uint32_t v) {
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}
__device__ __forceinline__ unsigned long long pd_wave_sum(unsigned long long v) {
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}
__device__ __forceinline__ uint32_t pd_wave_min(uint32_t v) {
    for (int m = 32; m >= 1; m >>= 1) { const uint32_t o = __shfl_xor(v, m, 64); v = o < v ? o : v; }
    return v;
}
__device__ __forceinline__ uint32_t pd_wave_max(uint32_t v) {
    for (int m = 32; m >= 1; m >>= 1) { const uint32_t o = __shfl_xor(v, m, 64); v = o > v ? o : v; }
    return v;
}

// ---- workgroup folds ----------------------------------------------------------------------------------------------------------------------------
// word += the workgroup's sum of v / word = max(word, the workgroup's largest v).  Every lane of a workgroup of RC_BLOCK calls these, once per
// counter, outside every branch and after its loop; lds is the caller's [RC_BLOCK / 64] array of the value's type, free again when the call returns
// (the trailing barrier).  No atomic is sent for a zero.  T is uint32_t where a workgroup's sum stays below 2^31 (a lane counts items of an int
// count), unsigned long long where one lane alone can pass that (candidates per face, samples per face).
// One atomic per workgroup and counter, and not one per wavefront: 46 000 of those on one word (2 952 000 vertices) cost 12 ns each, one after the
// other, which was a third of the weld's pass.
template <typename T>
__device__ __forceinline__ void pd_block_add(T v, unsigned long long* word, T* lds) {
    v = pd_wave_sum(v);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        T t = 0;
        for (int w = 0; w < RC_BLOCK / 64; w++) t += lds[w];
        if (t) atomicAdd(word, (unsigned long long)t);
    }
    __syncthreads();
}
__device__ __forceinline__ void pd_block_max(uint32_t v, unsigned long long* word, uint32_t* lds) {
    v = pd_wave_max(v);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (int w = 0; w < RC_BLOCK / 64; w++) t = lds[w] > t ? lds[w] : t;
        if (t) atomicMax(word, (unsigned long long)t);
    }
    __syncthreads();
}
// the same for a double that is neither negative nor NaN: such doubles order as their bits do
__device__ __forceinline__ void pd_block_max_f64(double v, unsigned long long* word, double* lds) {
    for (int m = 32; m >= 1; m >>= 1) { const double o = __shfl_xor(v, m, 64); v = o > v ? o : v; }
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int w = 0; w < RC_BLOCK / 64; w++) t = lds[w] > t ? lds[w] : t;
        if (t > 0.0) atomicMax(word, (unsigned long long)__double_as_longlong(t));
    }
    __syncthreads();
}

// the launches that fold go over their items in a grid-stride loop with at most PD_MAX_BLOCKS workgroups and keep their counts in registers
constexpr int PD_MAX_BLOCKS = 1024;
inline unsigned pd_grid_capped(int64_t n) { return rc_grid(n) < (unsigned)PD_MAX_BLOCKS ? rc_grid(n) : (unsigned)PD_MAX_BLOCKS; }

// ---- floats <-> unsigned keys of the same order ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t pd_key(float v) {
    const uint32_t u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float pd_unkey(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }

// ---- union-find: shared by the mesh topology (topology/) and the clusters of the cloud index (clusters_kernels.hip) ------------------------------
__device__ __forceinline__ int32_t tp_load(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of x as this lane sees it, halving the path on the way (the grandparent is an ancestor of x and stays one: hooks happen at roots only);
// -1 when the steps ran out
__device__ __forceinline__ int32_t tp_find(int32_t* parent, int32_t x, int64_t& steps) {
    int32_t p = tp_load(parent + x);
    while (p != x) {
        const int32_t g = tp_load(parent + p);
        if (g != p) atomicMin(parent + x, g);
        x = p;
        p = g;
        if (--steps < 0) return -1;
    }
    return x;
}

// false when the bound was hit
__device__ __forceinline__ bool tp_union(int32_t* parent, int32_t a, int32_t b) {
    int64_t steps = 2 * ((int64_t)a + (int64_t)b + 2);
    for (;;) {
        a = tp_find(parent, a, steps);
        b = tp_find(parent, b, steps);
        if (a < 0 || b < 0) return false;
        if (a == b) return true;
        if (a < b) { const int32_t t = a; a = b; b = t; }
        const int32_t old = atomicCAS(parent + a, a, b);     // the larger root under the smaller
        if (old == a) return true;
        a = old;                                             // a was hooked meanwhile, under old < a: go on from there
        if (--steps < 0) return false;
    }
}

// ---- a face counts: its three indices lie in [0, n_vtx) and are pairwise distinct; a vertex is finite: its three floats are ---------------------
__device__ __forceinline__ bool pd_counts(int64_t a, int64_t b, int64_t c, int64_t n_vtx) {
    return !(a < 0 || b < 0 || c < 0 || a >= n_vtx || b >= n_vtx || c >= n_vtx || a == b || b == c || a == c);
}
__device__ __forceinline__ bool pd_finite3(const float* __restrict__ vtx, int64_t v) {
    return isfinite(vtx[3 * v]) && isfinite(vtx[3 * v + 1]) && isfinite(vtx[3 * v + 2]);
}

// ---- runs of equal keys among n sorted keys (64-bit ones in every caller) ----------------------------------------------------------------------
// Templates on the key's and the positions' type, deduced from the arguments: a kernel that is no template would be compiled into the device code
// of every file that includes this header, a template only into the two that launch it (topology_host.cpp, smooth_host.cpp).
// head[i] = 1 where a run begins
template <typename K>
__global__ void __launch_bounds__(RC_BLOCK) pd_run_heads_kernel(const K* __restrict__ key, int64_t n, int32_t* __restrict__ head) {
    const int64_t i = (int64_t)blockIdx.x * RC_BLOCK + threadIdx.x;
    if (i >= n) return;
    head[i] = i == 0 || key[i] != key[i - 1] ? 1 : 0;
}
// after the exclusive scan of head: start[r] = the first position of run r, and start[the number of runs] = n, so that run r is as long as
// start[r + 1] - start[r].  start has `room` entries (the runs and the sentinel: n + 1 always suffices); every store is checked against it.
template <typename I>
__global__ void __launch_bounds__(RC_BLOCK) pd_run_starts_kernel(int64_t n, const I* __restrict__ head, const I* __restrict__ scan, I* __restrict__ start,
                                                                 int64_t room) {
    const int64_t i = (int64_t)blockIdx.x * RC_BLOCK + threadIdx.x;
    if (i >= n) return;
    const I h = head[i];
    const int64_t r = scan[i];
    if (h && r >= 0 && r < room) start[r] = (I)i;
    if (i == n - 1) {                                           // the one lane that knows the number of runs
        const int64_t runs = r + h;
        if (runs >= 0 && runs < room) start[runs] = (I)n;
    }
}
template <typename K>
inline void pd_launch_run_heads(hipStream_t s, const K* key, int64_t n, int32_t* head) {
    if (n > 0) pd_run_heads_kernel<<<rc_grid(n), RC_BLOCK, 0, s>>>(key, n, head);
}
template <typename I>
inline void pd_launch_run_starts(hipStream_t s, int64_t n, const I* head, const I* scan, I* start, int64_t room) {
    if (n > 0) pd_run_starts_kernel<<<rc_grid(n), RC_BLOCK, 0, s>>>(n, head, scan, start, room);
}

}  // namespace
