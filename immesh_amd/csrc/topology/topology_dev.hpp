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

// (the union-find, tp_load / tp_find / tp_union, lives in pass_dev.hpp: the clusters of the cloud index share it)

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
