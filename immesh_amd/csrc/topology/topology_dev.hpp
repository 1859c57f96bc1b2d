// Device helpers shared by the kernels of the mesh topology: topology_kernels.hip (the analysis), orient_kernels.hip (the orientation) and
// holes_kernels.hip (the holes).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../raycast/pass_dev.hpp"   // the folds, the float keys, the rule "a face counts", the run kernels: shared with the other passes

namespace {

constexpr int TP_BLOCK = 256;
static_assert(TP_BLOCK == RC_BLOCK, "the shared folds of pass_dev.hpp are written for workgroups of RC_BLOCK");
constexpr int TP_FOLD_ROUNDS = 4;   // components / patches folded per wavefront before the lanes left over send their own atomics
inline unsigned tp_grid(int64_t n) { return (unsigned)((n + TP_BLOCK - 1) / TP_BLOCK); }

// one atomic per wavefront: the lanes with `pred` counted by a ballot (every lane of the wavefront calls this)
__device__ __forceinline__ void tp_count(bool pred, unsigned long long* word) {
    const unsigned long long m = __ballot(pred);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(word, (unsigned long long)__popcll(m));
}

// ---- union-find ---------------------------------------------------------------------------------------------------------------------------
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

// forward: i_k < i_(k + 1 mod 3) of half-edge h = 3 f + k
__device__ __forceinline__ bool tp_forward(const int32_t* __restrict__ faces, int32_t h) {
    const int64_t f = h / 3;
    const int k = h - 3 * (int32_t)f;
    return faces[3 * f + k] < faces[3 * f + (k == 2 ? 0 : k + 1)];
}

// sorted half-edge i is the head of a run of exactly two: an edge with two uses, whose users are val[i] / 3 and val[i + 1] / 3
__device__ __forceinline__ bool tp_pair_head(const unsigned long long* __restrict__ key, int64_t i, int64_t n_half) {
    if (i + 1 >= n_half) return false;
    const unsigned long long k = key[i];
    if (i > 0 && key[i - 1] == k) return false;
    return key[i + 1] == k && !(i + 2 < n_half && key[i + 2] == k);
}

}  // namespace
