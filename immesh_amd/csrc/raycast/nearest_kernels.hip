// Mesh-to-cloud distances for gfx950 (include/immesh_nearest.h has the exact contract these kernels implement).
//   build     cn_mark / cn_compact: the finite points of a cloud with their boxes (lo == hi == the point), the bounds of the centres and the count,
//             in the layout the caster's build launches read (raycast.hpp); codes, sort, Karras' construction and the refit are the caster's own
//   nearest   one query per lane, a per-lane stack in private memory (depth bound: raycast.hpp; the keys (code, position) are distinct here too), the
//             child with the smaller box bound L first.  A node is skipped only when L of its own box exceeds r2 or the best D so far; a point's D
//             is L of its own box bit for bit, and L is monotone under containment, so no point that wins or ties is ever skipped.
//             The bound kept on the stack is a float rounded DOWN: it never exceeds L.
//   sampler   ms_count: k_f of every face and their int64 total (integer atomics, one per workgroup); the offsets are the renderer's device scan;
//             ms_emit: one lane per sample, which finds its face by binary search in the offsets; sample (f, j) depends on f, j, the seed and the
//             face alone, so the launch shape cannot show (one lane per face looping over its samples measures the same: DESIGN.md)
// Double arithmetic is written in the contract's order; the library builds with -ffp-contract=off, so nothing is fused.
#include "raycast.hpp"
#include "raycast_dev.hpp"

namespace {

inline unsigned cn_grid(int64_t n) { return (unsigned)((n + RC_BLOCK - 1) / RC_BLOCK); }

// floats -> unsigned keys of the same order (as the caster's build keeps its bounds)
__device__ __forceinline__ uint32_t cn_key(float v) {
    const uint32_t u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// ---- build ------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(RC_BLOCK) cn_mark_kernel(const float* __restrict__ xyz, int64_t n_pts, int32_t* __restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * RC_BLOCK + threadIdx.x;
    if (i >= n_pts) return;
    flag[i] = (isfinite(xyz[3 * i]) && isfinite(xyz[3 * i + 1]) && isfinite(xyz[3 * i + 2])) ? 1 : 0;
}

__global__ void __launch_bounds__(RC_BLOCK) cn_compact_kernel(const float* __restrict__ xyz, int64_t n_pts, const int32_t* __restrict__ flag,
                                                              const int32_t* __restrict__ off, int32_t* __restrict__ ids, float* __restrict__ box,
                                                              uint32_t* bounds, int64_t* n_in) {
    __shared__ uint32_t s_b[6];
    if (threadIdx.x < 6) s_b[threadIdx.x] = threadIdx.x < 3 ? 0xFFFFFFFFu : 0u;
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * RC_BLOCK + threadIdx.x;
    if (i < n_pts && flag[i]) {
        const int64_t o = off[i];
        for (int j = 0; j < 3; j++) {
            const float c = xyz[3 * i + j];
            box[6 * o + j] = c;
            box[6 * o + 3 + j] = c;
            const uint32_t k = cn_key(0.5f * c + 0.5f * c);   // the centre as rc_launch_codes computes it from the box
            atomicMin(&s_b[j], k);
            atomicMax(&s_b[3 + j], k);
        }
        ids[o] = (int32_t)i;
    }
    if (i == n_pts - 1) n_in[0] = (int64_t)off[i] + flag[i];
    __syncthreads();
    if (threadIdx.x < 3) { if (s_b[threadIdx.x] != 0xFFFFFFFFu) atomicMin(&bounds[threadIdx.x], s_b[threadIdx.x]); }
    else if (threadIdx.x < 6) { if (s_b[threadIdx.x] != 0u) atomicMax(&bounds[threadIdx.x], s_b[threadIdx.x]); }
}

// ---- nearest ----------------------------------------------------------------------------------------------------------------------------
// the contract's Point rule: false when the query has no neighbour by rule
template <bool FRAME>
__device__ __forceinline__ bool cn_point(const RcFrame& fr, const float* __restrict__ pts, int64_t i, double* p) {
    const float f[3] = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
    bool ok = isfinite(f[0]) && isfinite(f[1]) && isfinite(f[2]);
    const double x[3] = {(double)f[0], (double)f[1], (double)f[2]};
    for (int k = 0; k < 3; k++) {
        p[k] = FRAME ? ((fr.rot[3 * k] * x[0] + fr.rot[3 * k + 1] * x[1]) + fr.rot[3 * k + 2] * x[2]) + fr.pos[k] : x[k];
        ok = ok && fabs(p[k]) < 0x1p128;   // (false for NaN)
    }
    return ok;
}

// the contract's Box bound of a float box
__device__ __forceinline__ double cn_box(const double* p, const float* lo, const float* hi) {
    double e[3];
    for (int k = 0; k < 3; k++) e[k] = fmax(fmax((double)lo[k] - p[k], p[k] - (double)hi[k]), 0.0);
    return (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2];
}

__device__ __forceinline__ float cn_round_down(double x) {   // x >= 0: the largest float <= x
    float f = (float)x;
    if ((double)f > x) f = __uint_as_float(__float_as_uint(f) - 1u);
    return f;
}

template <bool FRAME>
__global__ void __launch_bounds__(RC_BLOCK) cn_nearest_kernel(RcFrame fr, const float* __restrict__ pts, int64_t n, double r2,
                                                              const float* __restrict__ cloud, const RcNode* __restrict__ nodes, int64_t n_in,
                                                              double* __restrict__ d2_out, float* __restrict__ dist_out, int32_t* __restrict__ index_out,
                                                              float* __restrict__ xyz_out, uint8_t* __restrict__ status_out) {
    const int64_t i = (int64_t)blockIdx.x * RC_BLOCK + threadIdx.x;
    if (i >= n) return;
    double p[3];
    const bool ok = cn_point<FRAME>(fr, pts, i, p);
    double best = r2;              // the bound: r2 until a point counts, then the best D
    int32_t best_i = -1;
    if (ok && n_in > 0) {
        int32_t stack[RC_STACK];
        float stack_key[RC_STACK];
        int sp = 0;
        int32_t cur = 0;
        for (;;) {
            if (cur < 0) {   // a cloud point
                const int32_t j = ~cur;
                const float* c = cloud + 3 * (int64_t)j;
                const double e0 = (double)c[0] - p[0], e1 = (double)c[1] - p[1], e2 = (double)c[2] - p[2];
                const double D = (e0 * e0 + e1 * e1) + e2 * e2;
                // a point met twice (the single-point tree) ties with itself and changes nothing
                if (D < best || (D == best && (best_i < 0 || j < best_i))) { best = D; best_i = j; }
            } else {
                const RcNode& nd = nodes[cur];
                const double l0 = cn_box(p, nd.lo[0], nd.hi[0]), l1 = cn_box(p, nd.lo[1], nd.hi[1]);
                const bool h0 = !(l0 > best), h1 = !(l1 > best);
                const int32_t c0 = nd.child[0], c1 = nd.child[1];
                if (h0 && h1) {
                    const bool first0 = l0 <= l1;       // the nearer child first: its points prune the other
                    stack[sp] = first0 ? c1 : c0;
                    stack_key[sp] = cn_round_down(first0 ? l1 : l0);
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
    const bool have = best_i >= 0;
    d2_out[i] = have ? best : -1.0;
    dist_out[i] = have ? (float)sqrt(best) : -1.0f;
    index_out[i] = best_i;
    const float nanf32 = __uint_as_float(0x7FC00000u);
    for (int k = 0; k < 3; k++) xyz_out[3 * i + k] = have ? cloud[3 * (int64_t)best_i + k] : nanf32;
    status_out[i] = have ? 0 : (ok ? 1 : 2);
}

// ---- the sampler ------------------------------------------------------------------------------------------------------------------------
constexpr unsigned long long MS_G = 0x9E3779B97F4A7C15ull;

__device__ __forceinline__ unsigned long long ms_mix(unsigned long long z) {
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}
__device__ __forceinline__ double ms_unit(unsigned long long h) { return (double)(h >> 11) * 0x1p-53; }
__device__ __forceinline__ unsigned long long ms_face_hash(unsigned long long seed, int64_t f) { return ms_mix(seed + MS_G * (unsigned long long)(f + 1)); }

// A, ab, ac of face f in double; false when the face is not in the hierarchy (n_vtx < 0: the caller knows that it is)
__device__ __forceinline__ bool ms_face(const float* __restrict__ vtx, int64_t n_vtx, const int32_t* __restrict__ faces, int64_t f, double* A, double* ab,
                                        double* ac) {
    double P[3][3];
    bool ok = true;
    for (int k = 0; k < 3; k++) {
        const int32_t id = faces[3 * f + k];
        if (n_vtx >= 0 && (id < 0 || (int64_t)id >= n_vtx)) return false;
        for (int j = 0; j < 3; j++) {
            const float x = vtx[3 * (int64_t)id + j];
            ok = ok && isfinite(x);
            P[k][j] = (double)x;
        }
    }
    for (int j = 0; j < 3; j++) { A[j] = P[0][j]; ab[j] = P[1][j] - P[0][j]; ac[j] = P[2][j] - P[0][j]; }
    return ok;
}

__global__ void __launch_bounds__(RC_BLOCK) ms_count_kernel(const float* __restrict__ vtx, int64_t n_vtx, const int32_t* __restrict__ faces, int64_t n_faces,
                                                            double density, unsigned long long seed, int32_t* __restrict__ cnt, unsigned long long* total) {
    __shared__ unsigned long long s_sum[RC_BLOCK];
    const int64_t f = (int64_t)blockIdx.x * RC_BLOCK + threadIdx.x;
    unsigned long long k = 0;
    if (f < n_faces) {
        double A[3], ab[3], ac[3];
        if (ms_face(vtx, n_vtx, faces, f, A, ab, ac)) {
            double nrm[3];
            rc_cross(ab, ac, nrm);
            const double x = (0.5 * sqrt(rc_dot(nrm, nrm))) * density;
            if (!isfinite(x) || x >= 0x1p31) {
                k = 1ull << 31;
            } else {
                const double fl = floor(x);
                k = (unsigned long long)fl + (ms_unit(ms_face_hash(seed, f)) < x - fl ? 1ull : 0ull);
            }
        }
        cnt[f] = k > 0x7FFFFFFFull ? 0x7FFFFFFF : (int32_t)k;   // (a total with such a face is refused before the offsets are read)
    }
    s_sum[threadIdx.x] = k;
    for (int stride = RC_BLOCK / 2; stride >= 1; stride >>= 1) {
        __syncthreads();
        if ((int)threadIdx.x < stride) s_sum[threadIdx.x] += s_sum[threadIdx.x + stride];
    }
    if (threadIdx.x == 0 && s_sum[0]) atomicAdd(total, s_sum[0]);
}

__device__ __forceinline__ void ms_sample(const double* A, const double* ab, const double* ac, unsigned long long hf, int64_t j, float* out) {
    double u = ms_unit(ms_mix(hf + MS_G * (unsigned long long)(2 * j + 1)));
    double v = ms_unit(ms_mix(hf + MS_G * (unsigned long long)(2 * j + 2)));
    if (u + v > 1.0) { u = 1.0 - u; v = 1.0 - v; }
    for (int k = 0; k < 3; k++) out[k] = (float)((A[k] + ab[k] * u) + ac[k] * v);
}

// one lane per sample: its face is the last one whose offset is not above the sample's position (faces without samples share their offset with the
// next face, so that face has samples)
__global__ void __launch_bounds__(RC_BLOCK) ms_emit_kernel(const float* __restrict__ vtx, const int32_t* __restrict__ faces, int64_t n_faces,
                                                                  unsigned long long seed, const int32_t* __restrict__ off, int64_t n_samples,
                                                                  float* __restrict__ xyz, int32_t* __restrict__ face) {
    const int64_t s = (int64_t)blockIdx.x * RC_BLOCK + threadIdx.x;
    if (s >= n_samples) return;
    int64_t lo = 0, hi = n_faces;                  // the first face in (lo, hi) whose offset is above s, or n_faces; off[0] == 0 <= s
    while (hi - lo > 1) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if ((int64_t)off[mid] <= s) lo = mid; else hi = mid;
    }
    const int64_t f = lo;
    double A[3], ab[3], ac[3];
    (void)ms_face(vtx, -1, faces, f, A, ab, ac);    // a face with samples is in the hierarchy
    float out[3];
    ms_sample(A, ab, ac, ms_face_hash(seed, f), s - (int64_t)off[f], out);
    for (int k = 0; k < 3; k++) xyz[3 * s + k] = out[k];
    face[s] = (int32_t)f;
}

}  // namespace

void cn_launch_mark(hipStream_t s, const float* xyz, int64_t n_pts, int32_t* flag) {
    if (n_pts > 0) cn_mark_kernel<<<cn_grid(n_pts), RC_BLOCK, 0, s>>>(xyz, n_pts, flag);
}

void cn_launch_compact(hipStream_t s, const float* xyz, int64_t n_pts, const int32_t* flag, const int32_t* off, int32_t* ids, float* box, uint32_t* bounds,
                       int64_t* n_in) {
    if (n_pts > 0) cn_compact_kernel<<<cn_grid(n_pts), RC_BLOCK, 0, s>>>(xyz, n_pts, flag, off, ids, box, bounds, n_in);
}

void cn_launch_nearest(hipStream_t s, const RcFrame& fr, int has_frame, const float* pts, int64_t n, double r2, const float* cloud, const RcNode* nodes,
                       int64_t n_in, double* d2, float* dist, int32_t* index, float* xyz, uint8_t* status) {
    if (n <= 0) return;
    if (has_frame) cn_nearest_kernel<true><<<cn_grid(n), RC_BLOCK, 0, s>>>(fr, pts, n, r2, cloud, nodes, n_in, d2, dist, index, xyz, status);
    else cn_nearest_kernel<false><<<cn_grid(n), RC_BLOCK, 0, s>>>(fr, pts, n, r2, cloud, nodes, n_in, d2, dist, index, xyz, status);
}

void cn_launch_nearest_world(hipStream_t s, const float* world_pts, int64_t n, double r2, const float* cloud, const RcNode* nodes, int64_t n_in, double* d2,
                             float* dist, int32_t* index, float* xyz, uint8_t* status) {
    const RcFrame none = {};
    if (n > 0) cn_nearest_kernel<false><<<cn_grid(n), RC_BLOCK, 0, s>>>(none, world_pts, n, r2, cloud, nodes, n_in, d2, dist, index, xyz, status);
}

void ms_launch_count(hipStream_t s, const float* vtx, int64_t n_vtx, const int32_t* faces, int64_t n_faces, double density, uint64_t seed, int32_t* cnt,
                     unsigned long long* total) {
    if (n_faces > 0) ms_count_kernel<<<cn_grid(n_faces), RC_BLOCK, 0, s>>>(vtx, n_vtx, faces, n_faces, density, (unsigned long long)seed, cnt, total);
}

void ms_launch_emit(hipStream_t s, const float* vtx, const int32_t* faces, int64_t n_faces, uint64_t seed, const int32_t* off, int64_t n_samples, float* xyz,
                    int32_t* face) {
    if (n_samples > 0 && n_faces > 0)
        ms_emit_kernel<<<cn_grid(n_samples), RC_BLOCK, 0, s>>>(vtx, faces, n_faces, (unsigned long long)seed, off, n_samples, xyz, face);
}
