// Mesh depth rasterizer + LiDAR point reinforcement for gfx950 (include/immesh_render.h has the exact contract these kernels implement).
//   setup    one lane per face: camera-frame vertices, the contract's cross products, the candidate box, the face's (face, 16x16 tile) pair count
//   bin      one lane per pair (the face found by binary search over the pair offsets, so a face that covers the screen is spread over many lanes):
//            count per tile, then scatter face ids into the tiles' bins
//   resolve  one 256-lane workgroup per tile, one lane per pixel: the bin streamed through LDS 256 faces at a time; each lane keeps
//            min((bits(d32) << 32) | face) in a register -- positive floats order as unsigned, so the result does not depend on bin order
//   reinforce  unproject the valid pixels, cell hash (a slot is claimed by the first pixel index CAS'd into it, atomicMin of the pixel index),
//            keep the cell winners, compact by prefix sum: pixel order, the sequential rule's result
// Double arithmetic is written in the contract's order; the library builds with -ffp-contract=off, so nothing is fused.
#include <rocprim/device/device_scan.hpp>
#include "render.hpp"

namespace {

__device__ __forceinline__ void rd_cross(const double* p, const double* q, double* o) {
    o[0] = p[1] * q[2] - p[2] * q[1];
    o[1] = p[2] * q[0] - p[0] * q[2];
    o[2] = p[0] * q[1] - p[1] * q[0];
}
__device__ __forceinline__ double rd_dot(const double* p, const double* q) { return (p[0] * q[0] + p[1] * q[1]) + p[2] * q[2]; }

__device__ __forceinline__ void rd_extend(const RdCam& c, double x, double y, double d, double* box) {
    const double U = (double)c.cx + (x / d) * c.f;
    const double V = (double)c.cy - (y / d) * c.f;
    box[0] = fmin(box[0], U); box[1] = fmax(box[1], U);
    box[2] = fmin(box[2], V); box[3] = fmax(box[3], V);
}

__global__ void __launch_bounds__(RD_BLOCK) rd_setup_kernel(RdCam c, const float* __restrict__ vtx, int64_t n_vtx, const int32_t* __restrict__ faces,
                                                            int64_t n_faces, RdFace* __restrict__ rec, int64_t* __restrict__ cnt) {
    const int64_t f = (int64_t)blockIdx.x * RD_BLOCK + threadIdx.x;
    if (f >= n_faces) return;
    double A[3][3];
    bool ok = true;
    for (int k = 0; k < 3; k++) {
        const int32_t id = faces[3 * f + k];
        if (id < 0 || (int64_t)id >= n_vtx) { ok = false; break; }
        const double p[3] = {(double)vtx[3 * (int64_t)id], (double)vtx[3 * (int64_t)id + 1], (double)vtx[3 * (int64_t)id + 2]};
        if (!isfinite(p[0]) || !isfinite(p[1]) || !isfinite(p[2])) { ok = false; break; }
        const double d[3] = {p[0] - c.pos[0], p[1] - c.pos[1], p[2] - c.pos[2]};
        for (int j = 0; j < 3; j++) A[k][j] = (c.rot[j] * d[0] + c.rot[3 + j] * d[1]) + c.rot[6 + j] * d[2];
    }
    int64_t pairs = 0;
    if (ok) {
        const double dep[3] = {-A[0][2], -A[1][2], -A[2][2]};
        const double dmax = fmax(fmax(dep[0], dep[1]), dep[2]), dmin = fmin(fmin(dep[0], dep[1]), dep[2]);
        if (dmax >= c.z_near && dmin < c.z_far) {
            double box[4] = {INFINITY, -INFINITY, INFINITY, -INFINITY};
            for (int k = 0; k < 3; k++)
                if (dep[k] >= c.z_near) rd_extend(c, A[k][0], A[k][1], dep[k], box);
            for (int k = 0; k < 3; k++) {
                const int j = k == 2 ? 0 : k + 1;
                if ((dep[k] < c.z_near) != (dep[j] < c.z_near)) {
                    const double t = (c.z_near - dep[k]) / (dep[j] - dep[k]);
                    rd_extend(c, A[k][0] + t * (A[j][0] - A[k][0]), A[k][1] + t * (A[j][1] - A[k][1]), c.z_near, box);
                }
            }
            const double W = (double)c.w + 4.0, H = (double)c.h + 4.0;
            const int u0 = max(0, (int)(floor(fmin(fmax(box[0], -4.0), W)) - 1.0));
            const int u1 = min(c.w - 1, (int)(ceil(fmin(fmax(box[1], -4.0), W)) + 1.0));
            const int v0 = max(0, (int)(floor(fmin(fmax(box[2], -4.0), H)) - 1.0));
            const int v1 = min(c.h - 1, (int)(ceil(fmin(fmax(box[3], -4.0), H)) + 1.0));
            if (u0 <= u1 && v0 <= v1) {
                RdFace r;
                rd_cross(A[0], A[1], r.ab);
                rd_cross(A[1], A[2], r.bc);
                rd_cross(A[2], A[0], r.ca);
                const double e[3] = {A[1][0] - A[0][0], A[1][1] - A[0][1], A[1][2] - A[0][2]};
                const double g[3] = {A[2][0] - A[0][0], A[2][1] - A[0][1], A[2][2] - A[0][2]};
                rd_cross(e, g, r.n);
                r.na = rd_dot(r.n, A[0]);
                r.u0 = u0; r.u1 = u1; r.v0 = v0; r.v1 = v1; r.pad[0] = r.pad[1] = 0;
                rec[f] = r;
                pairs = (int64_t)(u1 / RD_TILE - u0 / RD_TILE + 1) * (v1 / RD_TILE - v0 / RD_TILE + 1);
            }
        }
    }
    cnt[f] = pairs;   // culled faces: no pairs, their record is never read
}

__global__ void __launch_bounds__(RD_BLOCK) rd_bin_kernel(RdCam c, const RdFace* __restrict__ rec, const int64_t* __restrict__ foff, int64_t n_faces,
                                                          int64_t n_pairs, int pass, int32_t* tile_cnt, const int32_t* __restrict__ tile_off,
                                                          int32_t* tile_fill, int32_t* __restrict__ bins) {
    const int64_t p = (int64_t)blockIdx.x * RD_BLOCK + threadIdx.x;
    if (p >= n_pairs) return;
    int64_t lo = 0, hi = n_faces - 1;   // the face f with foff[f] <= p < foff[f + 1]
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (foff[mid + 1] > p) hi = mid; else lo = mid + 1;
    }
    const int64_t k = p - foff[lo];
    const RdFace& r = rec[lo];
    const int tx0 = r.u0 / RD_TILE, ty0 = r.v0 / RD_TILE, ntx = r.u1 / RD_TILE - tx0 + 1;
    const int t = (ty0 + (int)(k / ntx)) * c.tiles_x + tx0 + (int)(k % ntx);
    if (pass == 0) atomicAdd(&tile_cnt[t], 1);
    else bins[tile_off[t] + atomicAdd(&tile_fill[t], 1)] = (int32_t)lo;
}

__global__ void __launch_bounds__(RD_BLOCK) rd_resolve_kernel(RdCam c, const RdFace* __restrict__ rec, const int32_t* __restrict__ tile_cnt,
                                                              const int32_t* __restrict__ tile_off, const int32_t* __restrict__ bins,
                                                              float* __restrict__ depth, int32_t* __restrict__ face) {
    __shared__ RdFace s_rec[RD_BLOCK];
    __shared__ int32_t s_id[RD_BLOCK];
    const int t = blockIdx.x;
    const int lane = threadIdx.x;
    const int u = (t % c.tiles_x) * RD_TILE + (lane % RD_TILE), v = (t / c.tiles_x) * RD_TILE + lane / RD_TILE;
    const double dir[3] = {(double)(u - c.cx) / c.f, -((double)(v - c.cy) / c.f), -1.0};
    const int n = tile_cnt[t], off = tile_off[t];
    unsigned long long best = ~0ull;
    for (int base = 0; base < n; base += RD_BLOCK) {
        const int m = min(RD_BLOCK, n - base);
        __syncthreads();
        if (lane < m) {
            const int32_t f = bins[off + base + lane];
            s_id[lane] = f;
            s_rec[lane] = rec[f];
        }
        __syncthreads();
        for (int k = 0; k < m; k++) {
            const RdFace& r = s_rec[k];
            if (u < r.u0 || u > r.u1 || v < r.v0 || v > r.v1) continue;
            const double e0 = rd_dot(r.ab, dir), e1 = rd_dot(r.bc, dir), e2 = rd_dot(r.ca, dir);
            if (!((e0 >= 0.0 && e1 >= 0.0 && e2 >= 0.0) || (e0 <= 0.0 && e1 <= 0.0 && e2 <= 0.0))) continue;
            const double nd = rd_dot(r.n, dir);
            if (nd == 0.0) continue;
            const double s = r.na / nd;
            if (!(s >= c.z_near && s < c.z_far)) continue;
            const unsigned long long key = ((unsigned long long)__float_as_uint((float)s) << 32) | (uint32_t)s_id[k];
            best = key < best ? key : best;
        }
    }
    if (u >= c.w || v >= c.h) return;
    float d_out = -1.0f;
    int32_t f_out = -1;
    if (best != ~0ull) {
        const float d32 = __uint_as_float((uint32_t)(best >> 32));
        if ((double)d32 < 0.99 * c.z_far) { d_out = d32; f_out = (int32_t)(uint32_t)best; }
    }
    const int64_t i = (int64_t)v * c.w + u;
    depth[i] = d_out;
    face[i] = f_out;
}

__global__ void __launch_bounds__(RD_BLOCK) rd_unproject_kernel(RdCam c, float res, const float* __restrict__ depth, float* __restrict__ pts,
                                                                float* __restrict__ cells, int32_t* __restrict__ keep) {
    const int64_t i = (int64_t)blockIdx.x * RD_BLOCK + threadIdx.x;
    if (i >= (int64_t)c.w * c.h) return;
    const float d32 = depth[i];
    if (!(d32 >= 0.0f)) { keep[i] = 0; return; }
    const int u = (int)(i % c.w), v = (int)(i / c.w);
    const double d = (double)d32;
    const double x = ((double)(u - c.cx) / c.f) * d, y = -((double)(v - c.cy) / c.f) * d, z = -d;
    for (int r = 0; r < 3; r++) {
        const float w = (float)(((c.rot[3 * r] * x + c.rot[3 * r + 1] * y) + c.rot[3 * r + 2] * z) + c.pos[r]);
        pts[3 * i + r] = w;
        if (res > 0.0f) cells[3 * i + r] = roundf(w / res) + 0.0f;   // + 0: -0 and +0 are one cell, as the reference's int
    }
    keep[i] = res > 0.0f ? 0 : 1;
}

__device__ __forceinline__ uint32_t rd_hash(const float* cell) {
    uint32_t h = __float_as_uint(cell[0]) * 0x9E3779B1u;
    h = (h ^ (h >> 15)) + __float_as_uint(cell[1]) * 0x85EBCA77u;
    h = (h ^ (h >> 13)) + __float_as_uint(cell[2]) * 0xC2B2AE3Du;
    return h ^ (h >> 16);
}

__global__ void __launch_bounds__(RD_BLOCK) rd_hash_insert_kernel(int64_t n_pix, const float* __restrict__ depth, const float* __restrict__ cells,
                                                                  int32_t* tab_rep, uint32_t* tab_min, uint32_t mask, uint32_t* __restrict__ slot_of) {
    const int64_t i = (int64_t)blockIdx.x * RD_BLOCK + threadIdx.x;
    if (i >= n_pix || !(depth[i] >= 0.0f)) return;
    const float* my = cells + 3 * i;
    uint32_t slot = rd_hash(my) & mask;
    // the table holds at least twice the pixels, so an empty slot is always found within mask + 1 probes
    for (uint32_t probe = 0; probe <= mask; probe++) {
        int32_t rep = __hip_atomic_load(&tab_rep[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (rep < 0) {
            const int32_t prev = atomicCAS(&tab_rep[slot], -1, (int32_t)i);
            if (prev == -1) break;
            rep = prev;
        }
        const float* other = cells + 3 * (int64_t)rep;   // written by the previous launch
        if (__float_as_uint(other[0]) == __float_as_uint(my[0]) && __float_as_uint(other[1]) == __float_as_uint(my[1]) &&
            __float_as_uint(other[2]) == __float_as_uint(my[2]))
            break;
        slot = (slot + 1) & mask;
    }
    atomicMin(&tab_min[slot], (uint32_t)i);
    slot_of[i] = slot;
}

__global__ void __launch_bounds__(RD_BLOCK) rd_hash_keep_kernel(int64_t n_pix, const float* __restrict__ depth, const uint32_t* __restrict__ tab_min,
                                                                const uint32_t* __restrict__ slot_of, int32_t* __restrict__ keep) {
    const int64_t i = (int64_t)blockIdx.x * RD_BLOCK + threadIdx.x;
    if (i >= n_pix) return;
    keep[i] = (depth[i] >= 0.0f && tab_min[slot_of[i]] == (uint32_t)i) ? 1 : 0;
}

__global__ void __launch_bounds__(RD_BLOCK) rd_compact_kernel(int64_t n_pix, const float* __restrict__ pts, const int32_t* __restrict__ keep,
                                                              const int32_t* __restrict__ koff, float* __restrict__ out, int64_t* n_out) {
    const int64_t i = (int64_t)blockIdx.x * RD_BLOCK + threadIdx.x;
    if (i >= n_pix) return;
    if (keep[i]) {
        const int64_t o = koff[i];
        out[3 * o] = pts[3 * i]; out[3 * o + 1] = pts[3 * i + 1]; out[3 * o + 2] = pts[3 * i + 2];
    }
    if (i == n_pix - 1) n_out[0] = (int64_t)koff[i] + keep[i];
}

inline unsigned rd_grid(int64_t n) { return (unsigned)((n + RD_BLOCK - 1) / RD_BLOCK); }

}  // namespace

size_t rd_scan_temp_bytes(int64_t n_faces, int n_tiles, int64_t n_pix) {
    size_t a = 0, b = 0, d = 0;
    (void)rocprim::inclusive_scan(nullptr, a, (const int64_t*)nullptr, (int64_t*)nullptr, (size_t)n_faces, rocprim::plus<int64_t>(), (hipStream_t)0);
    (void)rocprim::exclusive_scan(nullptr, b, (const int32_t*)nullptr, (int32_t*)nullptr, (int32_t)0, (size_t)n_tiles, rocprim::plus<int32_t>(), (hipStream_t)0);
    (void)rocprim::exclusive_scan(nullptr, d, (const int32_t*)nullptr, (int32_t*)nullptr, (int32_t)0, (size_t)n_pix, rocprim::plus<int32_t>(), (hipStream_t)0);
    return std::max(a, std::max(b, d));
}

void rd_launch_setup(hipStream_t s, const RdCam& cam, const float* vtx, int64_t n_vtx, const int32_t* faces, int64_t n_faces, RdFace* rec, int64_t* cnt) {
    if (n_faces > 0) rd_setup_kernel<<<rd_grid(n_faces), RD_BLOCK, 0, s>>>(cam, vtx, n_vtx, faces, n_faces, rec, cnt);
}

void rd_scan_pairs(hipStream_t s, void* temp, size_t temp_bytes, const int64_t* cnt, int64_t* foff, int64_t n_faces) {
    (void)hipMemsetAsync(foff, 0, sizeof(int64_t), s);
    if (n_faces > 0) (void)rocprim::inclusive_scan(temp, temp_bytes, cnt, foff + 1, (size_t)n_faces, rocprim::plus<int64_t>(), s);
}

void rd_launch_bin(hipStream_t s, const RdCam& cam, const RdFace* rec, const int64_t* foff, int64_t n_faces, int64_t n_pairs, int pass, int32_t* tile_cnt,
                   const int32_t* tile_off, int32_t* tile_fill, int32_t* bins) {
    if (n_pairs > 0) rd_bin_kernel<<<rd_grid(n_pairs), RD_BLOCK, 0, s>>>(cam, rec, foff, n_faces, n_pairs, pass, tile_cnt, tile_off, tile_fill, bins);
}

void rd_scan_i32(hipStream_t s, void* temp, size_t temp_bytes, const int32_t* in, int32_t* out, int64_t n) {
    (void)rocprim::exclusive_scan(temp, temp_bytes, in, out, (int32_t)0, (size_t)n, rocprim::plus<int32_t>(), s);
}

void rd_launch_resolve(hipStream_t s, const RdCam& cam, const RdFace* rec, const int32_t* tile_cnt, const int32_t* tile_off, const int32_t* bins,
                       float* depth, int32_t* face) {
    rd_resolve_kernel<<<(unsigned)(cam.tiles_x * cam.tiles_y), RD_BLOCK, 0, s>>>(cam, rec, tile_cnt, tile_off, bins, depth, face);
}

void rd_launch_unproject(hipStream_t s, const RdCam& cam, float res, const float* depth, float* pts, float* cells, int32_t* keep) {
    rd_unproject_kernel<<<rd_grid((int64_t)cam.w * cam.h), RD_BLOCK, 0, s>>>(cam, res, depth, pts, cells, keep);
}

void rd_launch_hash_insert(hipStream_t s, int64_t n_pix, const float* depth, const float* cells, int32_t* tab_rep, uint32_t* tab_min, uint32_t mask,
                           uint32_t* slot_of) {
    rd_hash_insert_kernel<<<rd_grid(n_pix), RD_BLOCK, 0, s>>>(n_pix, depth, cells, tab_rep, tab_min, mask, slot_of);
}

void rd_launch_hash_keep(hipStream_t s, int64_t n_pix, const float* depth, const uint32_t* tab_min, const uint32_t* slot_of, int32_t* keep) {
    rd_hash_keep_kernel<<<rd_grid(n_pix), RD_BLOCK, 0, s>>>(n_pix, depth, tab_min, slot_of, keep);
}

void rd_launch_compact(hipStream_t s, int64_t n_pix, const float* pts, const int32_t* keep, const int32_t* koff, float* out, int64_t* n_out) {
    rd_compact_kernel<<<rd_grid(n_pix), RD_BLOCK, 0, s>>>(n_pix, pts, keep, koff, out, n_out);
}
