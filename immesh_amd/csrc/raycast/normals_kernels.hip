// Normals of the index's cloud and their agreement with the caster's face normals for gfx950 (include/immesh_normals.h, the Normals and Agreement
// rules, is the exact contract these kernels implement).
//   normals   one launch, one cloud point per lane.  The offering walk of raycast_dev.hpp (dq_walk_offer) fills the lane's k-best list (knn_dev.hpp:
//             the list of knn_kernels.hip, in private memory beside the walk's stack, its capacity a compile-time size).  The same lane then reads
//             the listed points again (twice: the mean, then the covariance about it), runs the cyclic Jacobi of dev_math.hpp, picks the column of
//             the smallest eigenvalue, signs it and writes 12 + 8 + 24 + 4 + 1 bytes.  No n x k list reaches memory.
//   agree     cloud direction: one launch, one cloud point per lane; a point with a normal walks to its exact closest face (dq_walk with the closest
//             query's Face rule as its leaf) and evaluates the rule there.  Samples direction: one lane per sample, reading the sampler's face ids
//             and the nearest query's indices where they lie.  Both write |s| and a status the distance queries' reduction reads as it is.
//   counts    integer folds (pass_dev.hpp), one atomic per workgroup and count.
// Double arithmetic is written in the contract's order; the library builds with -ffp-contract=off, so nothing is fused.  Plain C++ and vector
// stores only: no floating-point atomic, no cross-lane operation on a double.
#include "raycast.hpp"
#include "raycast_dev.hpp"
#include "knn_dev.hpp"
#include "pass_dev.hpp"
#include "../dev_math.hpp"

namespace {

struct NrView { double v[3]; };

template <int CAP>
__global__ void __launch_bounds__(RC_BLOCK) nr_normals_kernel(int64_t n, int32_t k, double r2, double min_ratio, int use_view, NrView view,
                                                              const float* __restrict__ cloud, const RcNode* __restrict__ nodes, int64_t n_in,
                                                              float* __restrict__ normal_out, double* __restrict__ curv_out, double* __restrict__ eig_out,
                                                              int32_t* __restrict__ count_out, uint8_t* __restrict__ status_out, unsigned long long* cnt) {
    __shared__ uint32_t lds[RC_BLOCK / 64];
    const int64_t i = (int64_t)blockIdx.x * RC_BLOCK + threadIdx.x;
    const bool in = i < n;
    int status = -1;
    if (in) {
        double p[3];
        const bool ok = dq_point(RcFrame{}, false, cloud, i, p);
        KnList<CAP> list;
        list.cloud = cloud; list.p = p; list.r2 = r2; list.k = k; list.skip = (int32_t)i; list.n = 0;
        if (ok && n_in > 0) dq_walk_offer(nodes, n_in, p, r2, list);
        const int32_t cnt_i = list.n;
        const float nanf32 = __uint_as_float(0x7FC00000u);
        float nrm[3] = {nanf32, nanf32, nanf32};
        double eig[3] = {-1.0, -1.0, -1.0}, curv = -1.0;
        status = !ok ? 2 : (cnt_i < 2 ? 1 : 0);
        if (status == 0) {
            const double m = (double)(cnt_i + 1);
            // the mean of the offsets, the point's own zero included
            double g[3] = {0.0, 0.0, 0.0};
            for (int32_t j = 0; j < cnt_i; j++) {
                const float* c = cloud + 3 * (int64_t)list.id[j];
                for (int a = 0; a < 3; a++) g[a] = g[a] + ((double)c[a] - p[a]);
            }
            for (int a = 0; a < 3; a++) g[a] = g[a] / m;
            // the covariance about it: xx, xy, xz, yy, yz, zz, begun with the point's own term
            double r[3] = {0.0 - g[0], 0.0 - g[1], 0.0 - g[2]};
            double t[6] = {r[0] * r[0], r[0] * r[1], r[0] * r[2], r[1] * r[1], r[1] * r[2], r[2] * r[2]};
            for (int32_t j = 0; j < cnt_i; j++) {
                const float* c = cloud + 3 * (int64_t)list.id[j];
                for (int a = 0; a < 3; a++) r[a] = ((double)c[a] - p[a]) - g[a];
                t[0] = t[0] + r[0] * r[0]; t[1] = t[1] + r[0] * r[1]; t[2] = t[2] + r[0] * r[2];
                t[3] = t[3] + r[1] * r[1]; t[4] = t[4] + r[1] * r[2]; t[5] = t[5] + r[2] * r[2];
            }
            for (int a = 0; a < 6; a++) t[a] = t[a] / m;
            const double C[9] = {t[0], t[1], t[2], t[1], t[3], t[4], t[2], t[4], t[5]};
            double ev[3], V[9];
            imd::sym3_eigen_jacobi(C, ev, V);
            int s = 0;
            if (ev[1] < ev[s]) s = 1;
            if (ev[2] < ev[s]) s = 2;
            const int o0 = s == 0 ? 1 : 0, o1 = s == 2 ? 1 : 2;     // the other two positions, ascending
            const int hi = ev[o1] > ev[o0] ? o1 : o0, mid = hi == o0 ? o1 : o0;
            eig[0] = ev[s]; eig[1] = ev[mid]; eig[2] = ev[hi];
            const double sum = (ev[0] + ev[1]) + ev[2];
            curv = sum > 0.0 ? ev[s] / sum : 0.0;
            if (!(ev[mid] > min_ratio * ev[hi])) {
                status = 3;
            } else {
                double u[3] = {V[s], V[3 + s], V[6 + s]};
                int big = 0;
                if (fabs(u[1]) > fabs(u[big])) big = 1;
                if (fabs(u[2]) > fabs(u[big])) big = 2;
                bool neg = u[big] < 0.0;
                if (neg) { u[0] = -u[0]; u[1] = -u[1]; u[2] = -u[2]; }
                if (use_view) {
                    const double w[3] = {view.v[0] - p[0], view.v[1] - p[1], view.v[2] - p[2]};
                    if (rc_dot(u, w) < 0.0) { u[0] = -u[0]; u[1] = -u[1]; u[2] = -u[2]; }
                }
                const double len = sqrt(rc_dot(u, u));
                for (int a = 0; a < 3; a++) nrm[a] = (float)(u[a] / len);
            }
        }
        for (int a = 0; a < 3; a++) { normal_out[3 * i + a] = nrm[a]; eig_out[3 * i + a] = eig[a]; }
        curv_out[i] = curv;
        count_out[i] = cnt_i;
        status_out[i] = (uint8_t)status;
    }
    pd_block_add<uint32_t>(status == 0 ? 1u : 0u, cnt + 0, lds);
    pd_block_add<uint32_t>(status == 1 ? 1u : 0u, cnt + 1, lds);
    pd_block_add<uint32_t>(status == 3 ? 1u : 0u, cnt + 2, lds);
    pd_block_add<uint32_t>(status == 2 ? 1u : 0u, cnt + 3, lds);
}

// the walk's leaf: D of a face by the closest query's Face rule (the walk keeps the winner's index; nothing else of it is needed)
struct NrFaceLeaf {
    const float* __restrict__ vtx;
    const int32_t* __restrict__ faces;
    const double* p;
    __device__ __forceinline__ double dist(int32_t f) {
        float lo[3], hi[3];
        double A[3][3], q[3];
        rc_load_face(vtx, faces, f, p, lo, hi, A);
        rc_face_point(A[0], A[1], A[2], q);
        return fmax(rc_dot(q, q), dq_box(p, lo, hi));
    }
    __device__ __forceinline__ void accept() {}
};

// the Agreement rule's Face and Value for face f (0 <= f < n_faces) and the float normal nrm: false when the face does not take part
__device__ __forceinline__ bool nr_agree(const float* __restrict__ vtx, int64_t n_vtx, const int32_t* __restrict__ faces, int64_t f,
                                         const float* __restrict__ nrm, double* s_out) {
    double P[3][3];
    for (int c = 0; c < 3; c++) {
        const int64_t v = faces[3 * f + c];
        if (v < 0 || v >= n_vtx) return false;
        for (int a = 0; a < 3; a++) P[c][a] = (double)vtx[3 * v + a];
    }
    double ab[3], ac[3], cr[3];
    for (int a = 0; a < 3; a++) { ab[a] = P[1][a] - P[0][a]; ac[a] = P[2][a] - P[0][a]; }
    rc_cross(ab, ac, cr);
    const double l2 = rc_dot(cr, cr);
    if (!(l2 > 0.0) || !isfinite(l2)) return false;          // (a vertex that is not finite gives an l2 that is not finite)
    const double nn[3] = {(double)nrm[0], (double)nrm[1], (double)nrm[2]};
    *s_out = rc_dot(cr, nn) / sqrt(l2);
    return true;
}

// what both directions write, and their four counts: st 0 a pair, 1 no pair, 2 the cloud point is not finite
__device__ __forceinline__ void nr_agree_store(bool in, int64_t i, int st, double s, float* __restrict__ agree_out, float* __restrict__ abs_out,
                                               uint8_t* __restrict__ st_out, unsigned long long* cnt, uint32_t* lds) {
    if (in) {
        const float a = st == 0 ? (float)s : __uint_as_float(0x7FC00000u);
        agree_out[i] = a;
        abs_out[i] = st == 0 ? fabsf(a) : -1.0f;
        st_out[i] = (uint8_t)st;
    }
    pd_block_add<uint32_t>(in && st == 0 ? 1u : 0u, cnt + 0, lds);
    pd_block_add<uint32_t>(in && st == 0 && s < 0.0 ? 1u : 0u, cnt + 1, lds);
    pd_block_add<uint32_t>(in && st == 1 ? 1u : 0u, cnt + 2, lds);
    pd_block_add<uint32_t>(in && st == 2 ? 1u : 0u, cnt + 3, lds);
}

__global__ void __launch_bounds__(RC_BLOCK) nr_agree_cloud_kernel(const float* __restrict__ cloud, const float* __restrict__ normal,
                                                                  const uint8_t* __restrict__ nstatus, int64_t n, double r2, const float* __restrict__ vtx,
                                                                  int64_t n_vtx, const int32_t* __restrict__ faces, int64_t n_faces,
                                                                  const RcNode* __restrict__ nodes, int64_t n_in, float* __restrict__ agree_out,
                                                                  float* __restrict__ abs_out, int32_t* __restrict__ face_out, uint8_t* __restrict__ st_out,
                                                                  unsigned long long* cnt) {
    __shared__ uint32_t lds[RC_BLOCK / 64];
    const int64_t i = (int64_t)blockIdx.x * RC_BLOCK + threadIdx.x;
    const bool in = i < n;
    int st = 1;
    double s = 0.0;
    if (in) {
        const uint8_t ns = nstatus[i];
        int32_t best_f = -1;
        if (ns == 2) st = 2;
        if (ns == 0 && n_in > 0) {
            double p[3];
            (void)dq_point(RcFrame{}, false, cloud, i, p);       // (a point with a normal is finite)
            double best = r2;
            NrFaceLeaf leaf = {vtx, faces, p};
            dq_walk(nodes, p, best, best_f, leaf);
            if (best_f >= 0 && best_f < n_faces && nr_agree(vtx, n_vtx, faces, best_f, normal + 3 * i, &s)) st = 0;
        }
        face_out[i] = best_f;
    }
    nr_agree_store(in, i, st, s, agree_out, abs_out, st_out, cnt, lds);
}

__global__ void __launch_bounds__(RC_BLOCK) nr_agree_samples_kernel(const int32_t* __restrict__ sface, const int32_t* __restrict__ index, int64_t n,
                                                                    const float* __restrict__ normal, const uint8_t* __restrict__ nstatus, int64_t n_pts,
                                                                    const float* __restrict__ vtx, int64_t n_vtx, const int32_t* __restrict__ faces,
                                                                    int64_t n_faces, float* __restrict__ agree_out, float* __restrict__ abs_out,
                                                                    uint8_t* __restrict__ st_out, unsigned long long* cnt) {
    __shared__ uint32_t lds[RC_BLOCK / 64];
    const int64_t j = (int64_t)blockIdx.x * RC_BLOCK + threadIdx.x;
    const bool in = j < n;
    int st = 1;
    double s = 0.0;
    if (in) {
        const int64_t at = index[j], f = sface[j];
        if (at >= 0 && at < n_pts && nstatus[at] == 0 && f >= 0 && f < n_faces && nr_agree(vtx, n_vtx, faces, f, normal + 3 * at, &s)) st = 0;
    }
    nr_agree_store(in, j, st, s, agree_out, abs_out, st_out, cnt, lds);
}

}  // namespace

void nr_launch_normals(hipStream_t s, int64_t n, int32_t k, double r2, double min_ratio, const double* viewpoint, const float* cloud, const RcNode* nodes,
                       int64_t n_in, float* normal, double* curv, double* eig, int32_t* count, uint8_t* status, unsigned long long* cnt) {
    if (n <= 0 || k < 2 || k > 64) return;
    NrView view = {{0.0, 0.0, 0.0}};
    if (viewpoint)
        for (int a = 0; a < 3; a++) view.v[a] = viewpoint[a];
    // KN_SIZES (knn_dev.hpp): the list's capacities
    kn_sized(k, [&](auto cap) {
        nr_normals_kernel<decltype(cap)::value><<<rc_grid(n), RC_BLOCK, 0, s>>>(n, k, r2, min_ratio, viewpoint ? 1 : 0, view, cloud, nodes, n_in, normal, curv,
                                                                                  eig, count, status, cnt);
    });
}

void nr_launch_agree_cloud(hipStream_t s, const float* cloud, const float* normal, const uint8_t* nstatus, int64_t n, double r2, const float* vtx, int64_t n_vtx,
                           const int32_t* faces, int64_t n_faces, const RcNode* nodes, int64_t n_in, float* agree, float* abs_agree, int32_t* face,
                           uint8_t* status, unsigned long long* cnt) {
    if (n > 0)
        nr_agree_cloud_kernel<<<rc_grid(n), RC_BLOCK, 0, s>>>(cloud, normal, nstatus, n, r2, vtx, n_vtx, faces, n_faces, nodes, n_in, agree, abs_agree, face,
                                                               status, cnt);
}

void nr_launch_agree_samples(hipStream_t s, const int32_t* sface, const int32_t* index, int64_t n, const float* normal, const uint8_t* nstatus, int64_t n_pts,
                             const float* vtx, int64_t n_vtx, const int32_t* faces, int64_t n_faces, float* agree, float* abs_agree, uint8_t* status,
                             unsigned long long* cnt) {
    if (n > 0)
        nr_agree_samples_kernel<<<rc_grid(n), RC_BLOCK, 0, s>>>(sface, index, n, normal, nstatus, n_pts, vtx, n_vtx, faces, n_faces, agree, abs_agree, status,
                                                                 cnt);
}
