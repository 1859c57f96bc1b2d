// Device pieces of the k nearest neighbours shared by knn_kernels.hip (the Neighbours rule of include/immesh_nearest.h) and normals_kernels.hip (the
// Normals rule of include/immesh_normals.h, whose neighbourhood is that list): the D rule of a cloud point, the k-best list that is the offering
// walk's sink, and the choice of the list's compile-time capacity.
#pragma once
#include <type_traits>
#include "raycast_dev.hpp"

namespace {

// the D rule for cloud point j
__device__ __forceinline__ double kn_dist(const float* __restrict__ cloud, const double* p, int32_t j) {
    const float* c = cloud + 3 * (int64_t)j;
    const double e0 = (double)c[0] - p[0], e1 = (double)c[1] - p[1], e2 = (double)c[2] - p[2];
    return (e0 * e0 + e1 * e1) + e2 * e2;
}

// the k best (D, index) pairs seen so far, ascending; slots [0, n) are filled.  offer() is the walk's leaf.
template <int CAP>
struct KnList {
    const float* __restrict__ cloud;
    const double* p;
    double r2;
    int32_t k, skip, n;
    double d[CAP];
    int32_t id[CAP];
    __device__ __forceinline__ double bound() const { return n == k ? d[k - 1] : r2; }
    __device__ __forceinline__ double offer(int32_t j) {
        if (j == skip) return bound();
        const double D = kn_dist(cloud, p, j);
        if (!(D <= r2)) return bound();
        if (n == k && !(D < d[k - 1] || (D == d[k - 1] && j < id[k - 1]))) return d[k - 1];   // not among the k best under (D, index)
        int s = n == k ? k - 1 : n;                     // the slot that opens: the last one when full (its pair leaves), else the next free one
        while (s > 0 && (d[s - 1] > D || (d[s - 1] == D && id[s - 1] > j))) {
            d[s] = d[s - 1]; id[s] = id[s - 1];
            s--;
        }
        d[s] = D; id[s] = j;
        if (n < k) n++;
        return bound();
    }
};

// KN_SIZES: the list's capacities.  launch(std::integral_constant<int, CAP>) starts the kernel whose list holds k pairs, so that a small k does not
// pay for 64 slots; 1 <= k <= 64 is the caller's to check.
template <class Launch>
inline void kn_sized(int32_t k, Launch&& launch) {
    if (k <= 4) launch(std::integral_constant<int, 4>{});
    else if (k <= 16) launch(std::integral_constant<int, 16>{});
    else launch(std::integral_constant<int, 64>{});
}

}  // namespace
