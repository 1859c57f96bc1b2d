// Mesh-to-cloud distances for gfx950 (include/immesh_nearest.h has the exact contract these kernels implement).
//   nearest   one query per lane on the distance walk of raycast_dev.hpp (dq_walk) over the index's hierarchy (a point is a box whose lo == hi;
//             built by rc_tree_build like the caster's): the leaf is the squared distance to a cloud point, which is the Box bound of the point's
//             own box bit for bit
//   sampler   ms_count: k_f of every face and their int64 total (integer atomics, one per workgroup); the offsets are the renderer's device scan;
//             ms_emit: one lane per sample, which finds its face by binary search in the offsets; sample (f, j) depends on f, j, the seed and the
//             face alone, so the launch shape cannot show (one lane per face looping over its samples measures the same: DESIGN.md)
// Double arithmetic is written in the contract's order; the library builds with -ffp-contract=off, so nothing is fused.
#include "raycast.hpp"
#include "raycast_dev.hpp"
#include "pass_dev.hpp"   // the sampler's fold of its total

namespace {

// ---- nearest ----------------------------------------------------------------------------------------------------------------------------
// the walk's leaf: D of a cloud point; the winner's index is all that is kept
struct CnPointLeaf {
    const float* __restrict__ cloud;
    const double* p;
    __device__ __forceinline__ double dist(int32_t j) const {
        const float* c = cloud + 3 * (int64_t)j;
        const double e0 = (double)c[0] - p[0], e1 = (double)c[1] - p[1], e2 = (double)c[2] - p[2];
        return (e0 * e0 + e1 * e1) + e2 * e2;
    }
    __device__ __forceinline__ void accept() const {}
};

template <bool FRAME>
__global__ void __launch_bounds__(RC_BLOCK) cn_nearest_kernel(RcFrame fr, const float* __restrict__ pts, int64_t n, double r2,
                                                              const float* __restrict__ cloud, const RcNode* __restrict__ nodes, int64_t n_in,
                                                              double* __restrict__ d2_out, float* __restrict__ dist_out, int32_t* __restrict__ index_out,
                                                              float* __restrict__ xyz_out, uint8_t* __restrict__ status_out) {
    const int64_t i = (int64_t)blockIdx.x * RC_BLOCK + threadIdx.x;
    if (i >= n) return;
    double p[3];
    const bool ok = dq_point(fr, FRAME, pts, i, p);
    double best = r2;              // the bound: r2 until a point counts, then the best D
    int32_t best_i = -1;
    CnPointLeaf leaf = {cloud, p};
    if (ok && n_in > 0) dq_walk(nodes, p, best, best_i, leaf);
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
    __shared__ unsigned long long lds[RC_BLOCK / 64];
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
    pd_block_add<unsigned long long>(k, total, lds);            // 64 bits: a face counts up to 2^31 samples
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

void cn_launch_nearest(hipStream_t s, const RcFrame& fr, int has_frame, const float* pts, int64_t n, double r2, const float* cloud, const RcNode* nodes,
                       int64_t n_in, double* d2, float* dist, int32_t* index, float* xyz, uint8_t* status) {
    if (n <= 0) return;
    if (has_frame) cn_nearest_kernel<true><<<rc_grid(n), RC_BLOCK, 0, s>>>(fr, pts, n, r2, cloud, nodes, n_in, d2, dist, index, xyz, status);
    else cn_nearest_kernel<false><<<rc_grid(n), RC_BLOCK, 0, s>>>(fr, pts, n, r2, cloud, nodes, n_in, d2, dist, index, xyz, status);
}

void ms_launch_count(hipStream_t s, const float* vtx, int64_t n_vtx, const int32_t* faces, int64_t n_faces, double density, uint64_t seed, int32_t* cnt,
                     unsigned long long* total) {
    if (n_faces > 0) ms_count_kernel<<<rc_grid(n_faces), RC_BLOCK, 0, s>>>(vtx, n_vtx, faces, n_faces, density, (unsigned long long)seed, cnt, total);
}

void ms_launch_emit(hipStream_t s, const float* vtx, const int32_t* faces, int64_t n_faces, uint64_t seed, const int32_t* off, int64_t n_samples, float* xyz,
                    int32_t* face) {
    if (n_samples > 0 && n_faces > 0)
        ms_emit_kernel<<<rc_grid(n_samples), RC_BLOCK, 0, s>>>(vtx, faces, n_faces, (unsigned long long)seed, off, n_samples, xyz, face);
}
