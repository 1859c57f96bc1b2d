// The colour pass behind the mesh rasterizer for gfx950 (include/immesh_shade.h has the exact contract these kernels implement).
//   range    two stages: up to 1 024 workgroups stride over the vertices and reduce the min / max of one coordinate over the finite ones, as
//            order-preserving 32-bit keys, by shuffles and LDS to one pair per workgroup; one workgroup reduces the pairs.  No atomics: a first version
//            with one atomicMin per wavefront on two words spent 0.19 ms of 0.21 on them at 3.1 M vertices (8 192 wavefronts, all resident at once, all
//            looking at the initial value).  min and max are order-free, so the result is the same on every run
//   colours  one lane per vertex: the Heat byte triple of its coordinate, or the caller's / the colourer's bytes under min_views and bgr, packed into
//            one dword so that the pixel pass does one load per vertex (WHITE needs no array)
//   shade    deferred: one lane per pixel in the resolve kernel's 16 x 16 tiles, so neighbouring lanes read the same face record; the record's first
//            96 bytes (ab, bc, ca, n) as six 16-byte loads, three indices, three packed colours; e0, e1, e2 and nd are recomputed from the record and the
//            pixel's ray exactly as rd_resolve_kernel computed them (same operations, same order), nothing of the setup is redone
// Double arithmetic is written in the contract's order; the library builds with -ffp-contract=off, so nothing is fused.
#include <algorithm>
#include "render.hpp"
#include "../../../include/immesh_shade.h"

namespace {

__device__ __forceinline__ uint32_t sh_key(float x) {   // unsigned order = float order (finite values)
    const uint32_t b = __float_as_uint(x);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float sh_unkey(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }

// min of lo and max of hi over the workgroup, valid in lane 0
__device__ __forceinline__ void sh_block_minmax(uint32_t& lo, uint32_t& hi) {
    __shared__ uint32_t s_lo[RD_BLOCK / 64], s_hi[RD_BLOCK / 64];
    for (int d = 32; d >= 1; d >>= 1) {
        lo = min(lo, (uint32_t)__shfl_xor((int)lo, d, 64));
        hi = max(hi, (uint32_t)__shfl_xor((int)hi, d, 64));
    }
    if ((threadIdx.x & 63) == 0) { s_lo[threadIdx.x >> 6] = lo; s_hi[threadIdx.x >> 6] = hi; }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int k = 1; k < RD_BLOCK / 64; k++) { lo = min(lo, s_lo[k]); hi = max(hi, s_hi[k]); }
}

// stage 1: part[2 b], part[2 b + 1] = the smallest and largest key of workgroup b's vertices (0xFFFFFFFF / 0: none)
__global__ void __launch_bounds__(RD_BLOCK) rd_shade_range_kernel(const float* __restrict__ vtx, int64_t n_vtx, int axis, uint32_t* __restrict__ part) {
    uint32_t lo = 0xFFFFFFFFu, hi = 0u;
    for (int64_t i = (int64_t)blockIdx.x * RD_BLOCK + threadIdx.x; i < n_vtx; i += (int64_t)gridDim.x * RD_BLOCK) {
        const float x = vtx[3 * i], y = vtx[3 * i + 1], z = vtx[3 * i + 2];
        if (!isfinite(x) || !isfinite(y) || !isfinite(z)) continue;
        const uint32_t k = sh_key(axis == 0 ? x : (axis == 1 ? y : z));
        lo = min(lo, k); hi = max(hi, k);
    }
    sh_block_minmax(lo, hi);
    if (threadIdx.x == 0) { part[2 * blockIdx.x] = lo; part[2 * blockIdx.x + 1] = hi; }
}

// stage 2 (one workgroup): keys[0], keys[1] = the smallest and largest key of the n_part partials
__global__ void __launch_bounds__(RD_BLOCK) rd_shade_range_final_kernel(const uint32_t* __restrict__ part, int n_part, uint32_t* __restrict__ keys) {
    uint32_t lo = 0xFFFFFFFFu, hi = 0u;
    for (int b = threadIdx.x; b < n_part; b += RD_BLOCK) { lo = min(lo, part[2 * b]); hi = max(hi, part[2 * b + 1]); }
    sh_block_minmax(lo, hi);
    if (threadIdx.x == 0) { keys[0] = lo; keys[1] = hi; }
}

__device__ __forceinline__ uint32_t sh_byte(double col) { return (uint32_t)(uint8_t)(int)(col * 255.0); }

__global__ void __launch_bounds__(RD_BLOCK) rd_shade_colours_kernel(RdShade sh, const float* __restrict__ vtx, int64_t n_vtx, const uint8_t* __restrict__ bytes,
                                                                    RdColourState st, const uint32_t* __restrict__ keys, uint32_t* __restrict__ col,
                                                                    float* __restrict__ range) {
    const int64_t i = (int64_t)blockIdx.x * RD_BLOCK + threadIdx.x;
    uint32_t m0, m1, m2;   // memory channels 0, 1, 2
    if (sh.source == IMMESH_SHADE_AXIS) {
        float lo = sh.lo, hi = sh.hi;
        if (sh.range_from_vertices) {
            const uint32_t k0 = keys[0], k1 = keys[1];
            const bool none = k0 > k1;
            lo = none ? 0.0f : sh_unkey(k0); hi = none ? 0.0f : sh_unkey(k1);
        }
        if (i == 0) { range[0] = lo; range[1] = hi; }
        if (i >= n_vtx) return;
        const float p = vtx[3 * i + sh.axis];
        const float val = hi <= lo ? 0.0f : (p - lo) / (hi - lo);
        const double x = 1.0 - (double)val;
        const double m = x < 1.0 ? x : 1.0;
        const double c = 0.0 < m ? m : 0.0;
        const double a = c * 4.0;
        const double fi = floor(a);
        const double t = a - fi;
        const int i0 = (int)fi, i1 = (int)ceil(a);
        // T = (0,0,1), (0,1,1), (0,1,0), (1,1,0), (1,0,0)
        const double r0 = i0 >= 3 ? 1.0 : 0.0, r1 = i1 >= 3 ? 1.0 : 0.0;
        const double g0 = (i0 >= 1 && i0 <= 3) ? 1.0 : 0.0, g1 = (i1 >= 1 && i1 <= 3) ? 1.0 : 0.0;
        const double b0 = i0 <= 1 ? 1.0 : 0.0, b1 = i1 <= 1 ? 1.0 : 0.0;
        m0 = sh_byte((1.0 - t) * r0 + t * r1);
        m1 = sh_byte((1.0 - t) * g0 + t * g1);
        m2 = sh_byte((1.0 - t) * b0 + t * b1);
        col[i] = m0 | (m1 << 8) | (m2 << 16);
        return;
    }
    if (i >= n_vtx) return;
    if (bytes) {
        m0 = bytes[3 * i]; m1 = bytes[3 * i + 1]; m2 = bytes[3 * i + 2];
    } else {   // immesh_colour_fetch's bytes: rgb / first_exposure, clamped to [0, 255] and truncated
        const double fe = st.first_exposure[i];
        const bool seen = st.n_obs[i] >= sh.min_views;
        uint32_t q[3];
        for (int k = 0; k < 3; k++) {
            const double v = st.rgb[k][i] / fe;
            q[k] = seen ? (uint32_t)(uint8_t)(v > 255.0 ? 255 : (v > 0.0 ? (int)v : 0)) : 0u;
        }
        m0 = q[0]; m1 = q[1]; m2 = q[2];
    }
    col[i] = sh.bgr ? (m2 | (m1 << 8) | (m0 << 16)) : (m0 | (m1 << 8) | (m2 << 16));
}

__global__ void __launch_bounds__(RD_BLOCK) rd_shade_kernel(RdCam c, RdShade sh, const RdFace* __restrict__ rec, const int32_t* __restrict__ faces,
                                                            const int32_t* __restrict__ face, const uint32_t* __restrict__ col, uint8_t* __restrict__ rgb) {
    const int t = blockIdx.x;
    const int lane = threadIdx.x;
    const int u = (t % c.tiles_x) * RD_TILE + (lane % RD_TILE), v = (t / c.tiles_x) * RD_TILE + lane / RD_TILE;
    if (u >= c.w || v >= c.h) return;
    const int64_t i = (int64_t)v * c.w + u;
    const int32_t f = face[i];
    uint32_t out = sh.background;
    if (f >= 0) {
        const double2* q = reinterpret_cast<const double2*>(rec + f);   // ab, bc, ca, n: the record's first 96 bytes
        const double2 q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3], q4 = q[4], q5 = q[5];
        const int32_t ia = faces[3 * (int64_t)f], ib = faces[3 * (int64_t)f + 1], ic = faces[3 * (int64_t)f + 2];
        const uint32_t ca = col ? col[ia] : 0xFFFFFFu, cb = col ? col[ib] : 0xFFFFFFu, cc = col ? col[ic] : 0xFFFFFFu;
        const double ab[3] = {q0.x, q0.y, q1.x}, bc[3] = {q1.y, q2.x, q2.y}, cA[3] = {q3.x, q3.y, q4.x}, n[3] = {q4.y, q5.x, q5.y};
        const double dir[3] = {(double)(u - c.cx) / c.f, -((double)(v - c.cy) / c.f), -1.0};
        const double e0 = (ab[0] * dir[0] + ab[1] * dir[1]) + ab[2] * dir[2];
        const double e1 = (bc[0] * dir[0] + bc[1] * dir[1]) + bc[2] * dir[2];
        const double e2 = (cA[0] * dir[0] + cA[1] * dir[1]) + cA[2] * dir[2];
        const double E = (e0 + e1) + e2;
        double wa = 1.0 / 3.0, wb = 1.0 / 3.0, wc = 1.0 / 3.0;
        if (E != 0.0) { wa = e1 / E; wb = e2 / E; wc = e0 / E; }
        double L = 1.0;
        if (sh.light) {
            const double nd = (n[0] * dir[0] + n[1] * dir[1]) + n[2] * dir[2];
            const double nn = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2];
            const double dd = (dir[0] * dir[0] + dir[1] * dir[1]) + dir[2] * dir[2];
            L = 0.2 + (fabs(nd) / (sqrt(nn) * sqrt(dd))) * 0.5;
        }
        out = 0;
        for (int k = 0; k < 3; k++) {
            const double Ca = (double)((ca >> (8 * k)) & 255u), Cb = (double)((cb >> (8 * k)) & 255u), Cc = (double)((cc >> (8 * k)) & 255u);
            const double obj = ((wa * Ca + wb * Cb) + wc * Cc) / 255.0;
            const double o = floor(fmin(fmax(L * obj, 0.0), 1.0) * 255.0 + 0.5);
            out |= (uint32_t)(uint8_t)(int)o << (8 * k);
        }
    }
    // three byte stores per lane.  A tile row is 48 contiguous bytes whose start, 3 (v width + u0), is dword-aligned only for some widths and rows;
    // staging the tile through LDS into dword stores measured 8 % slower at 1920 x 1080
    uint8_t* o = rgb + 3 * i;
    o[0] = (uint8_t)out; o[1] = (uint8_t)(out >> 8); o[2] = (uint8_t)(out >> 16);
}

inline unsigned sh_grid(int64_t n) { return (unsigned)((n + RD_BLOCK - 1) / RD_BLOCK); }

}  // namespace

static int rd_shade_range_parts(int64_t n_vtx) { return (int)std::min<int64_t>((n_vtx + RD_BLOCK - 1) / RD_BLOCK, RD_SHADE_RANGE_PARTS); }

void rd_launch_shade_range(hipStream_t s, const float* vtx, int64_t n_vtx, int axis, uint32_t* part, uint32_t* keys) {
    const int n_part = rd_shade_range_parts(n_vtx);   // (no vertex: no partial, the final pass writes "none")
    if (n_part > 0) rd_shade_range_kernel<<<(unsigned)n_part, RD_BLOCK, 0, s>>>(vtx, n_vtx, axis, part);
    rd_shade_range_final_kernel<<<1, RD_BLOCK, 0, s>>>(part, n_part, keys);
}

void rd_launch_shade_colours(hipStream_t s, const RdShade& sh, const float* vtx, int64_t n_vtx, const uint8_t* bytes, const RdColourState& st,
                             const uint32_t* keys, uint32_t* col, float* range) {
    rd_shade_colours_kernel<<<std::max(1u, sh_grid(n_vtx)), RD_BLOCK, 0, s>>>(sh, vtx, n_vtx, bytes, st, keys, col, range);   // (lane 0 writes the range)
}

void rd_launch_shade(hipStream_t s, const RdCam& cam, const RdShade& sh, const RdFace* rec, const int32_t* faces, const int32_t* face, const uint32_t* col,
                     uint8_t* rgb) {
    rd_shade_kernel<<<(unsigned)(cam.tiles_x * cam.tiles_y), RD_BLOCK, 0, s>>>(cam, sh, rec, faces, face, col, rgb);
}
