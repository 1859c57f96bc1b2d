// Device helpers shared by the ray caster's kernels (raycast_kernels.hip) and the closest-point kernels (closest_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace {

__device__ __forceinline__ void rc_cross(const double* p, const double* q, double* o) {
    o[0] = p[1] * q[2] - p[2] * q[1];
    o[1] = p[2] * q[0] - p[0] * q[2];
    o[2] = p[0] * q[1] - p[1] * q[0];
}
__device__ __forceinline__ double rc_dot(const double* p, const double* q) { return (p[0] * q[0] + p[1] * q[1]) + p[2] * q[2]; }

}  // namespace
