// The one-ring table, Taubin smoothing and vertex normals of the caster's snapshot for gfx950 (include/immesh_smooth.h is the exact contract these
// kernels implement).
//   emit       one lane per face: its six directed pairs as keys (u << 32) | v; a face that does not count emits the key above every real one.  One
//              64-bit pair sort follows: the pairs then ascend by u, then v, and a run of equal keys is as long as the uses of its edge
//   heads / runs / entries   run heads, and behind the scan of the heads every run's first position (pass_dev.hpp's run kernels, launched by
//              smooth_host.cpp); a run's length is the next run's first position
//              less its own, so neighbours[] and uses[] are one gather per entry: no lane walks a run for this
//   rows       one lane per vertex bisects the sorted keys for the position where its row begins (and the next row: its valence), reads the border
//              flag the entries left, and has its class
//   lists      one lane per entry: the neighbour, or -1 when the entry is not in the smoothing list of its row.  The step filters on this sign and
//              never reads a class or a use count again
//   step       one lane per vertex sums its row in order: the order IS the contract, so this walk is sequential, bounded by the valence, with three
//              independent sums per lane
//   incidence / normals   three (vertex, face) pairs per face that counts and is finite, one stable 32-bit pair sort by vertex, one lane per vertex
//              walks its run in ascending face
//   counters   integers (and one maximum of a double that is not negative, compared as bits), folded per workgroup before one atomic each
//              (pass_dev.hpp's folds; the launches that count go over their items in a grid-stride loop, pd_grid_capped)
// Integers, float bits and sequential double sums (compiled with -ffp-contract=off): the results do not depend on the order of anything.  Every
// scatter index is checked against its room before the store.
#include "smooth.hpp"
#include "../raycast/raycast_dev.hpp"
#include "../topology/topology_dev.hpp"
#include "../../../include/immesh_smooth.h"

namespace {

// the first position in [0, n) whose key is >= want (n: none)
template <typename K>
__device__ __forceinline__ int64_t sm_lower_bound(const K* __restrict__ key, int64_t n, K want) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (key[mid] < want) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}
// the runs that begin before position i of n6 > 0 (i == n6: all of them).  Where this is asked, i begins a run or is n6.
__device__ __forceinline__ int64_t sm_runs_before(const int32_t* __restrict__ head, const int32_t* __restrict__ scan, int64_t n6, int64_t i) {
    return i < n6 ? (int64_t)scan[i] : (int64_t)scan[n6 - 1] + head[n6 - 1];
}

__global__ void __launch_bounds__(TP_BLOCK) sm_emit_kernel(const int32_t* __restrict__ faces, int64_t n_faces, int64_t n_vtx,
                                                           unsigned long long* __restrict__ key, int32_t* __restrict__ val) {
    const int64_t f = (int64_t)blockIdx.x * TP_BLOCK + threadIdx.x;
    if (f >= n_faces) return;
    const int64_t a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    const unsigned long long apart = (unsigned long long)n_vtx << 32;
    unsigned long long k[6] = {apart, apart, apart, apart, apart, apart};
    if (pd_counts(a, b, c, n_vtx)) {
        const unsigned long long ua = (unsigned long long)a, ub = (unsigned long long)b, uc = (unsigned long long)c;
        k[0] = (ua << 32) | ub; k[1] = (ub << 32) | ua;
        k[2] = (ub << 32) | uc; k[3] = (uc << 32) | ub;
        k[4] = (uc << 32) | ua; k[5] = (ua << 32) | uc;
    }
    for (int e = 0; e < 6; e++) {
        key[6 * f + e] = k[e];
        val[6 * f + e] = (int32_t)(6 * f + e);
    }
}

__global__ void __launch_bounds__(TP_BLOCK) sm_entries_kernel(const unsigned long long* __restrict__ key, int64_t n6, int64_t n_vtx,
                                                              const int32_t* __restrict__ head, const int32_t* __restrict__ scan,
                                                              const int32_t* __restrict__ rstart, int32_t* __restrict__ neighbours,
                                                              int32_t* __restrict__ uses, int8_t* flag) {
    const int64_t p = (int64_t)blockIdx.x * TP_BLOCK + threadIdx.x;
    if (p >= n6 || p >= sm_runs_before(head, scan, n6, n6)) return;
    const int64_t at = rstart[p], next = rstart[p + 1];
    if (at < 0 || at >= n6 || next <= at || next > n6) return;  // (a run has a member: never)
    const unsigned long long k = key[at];
    const int64_t u = (int64_t)(k >> 32), v = (int64_t)(k & 0xFFFFFFFFull);
    if (u >= n_vtx || v >= n_vtx) return;                       // the run of the faces that do not count: the last one, no entry
    const int64_t n = next - at;
    neighbours[p] = (int32_t)v;
    uses[p] = (int32_t)n;
    if (n != 2) flag[SM_FLAG_BORDER * n_vtx + u] = 1;           // every writer stores the same value; v's row has the mirrored entry
}

__global__ void __launch_bounds__(TP_BLOCK) sm_rows_kernel(const float* __restrict__ vtx, int64_t n_vtx, const unsigned long long* __restrict__ key,
                                                           int64_t n6, const int32_t* __restrict__ head, const int32_t* __restrict__ scan,
                                                           const int8_t* __restrict__ flag, long long* __restrict__ row_start,
                                                           int8_t* __restrict__ vclass, unsigned long long* cnt) {
    __shared__ uint32_t lds[TP_BLOCK / 64];
    uint32_t n_used = 0, n_not_finite = 0, n_border = 0, n_interior = 0, valence = 0;
    for (int64_t base = (int64_t)blockIdx.x * TP_BLOCK; base <= n_vtx; base += (int64_t)gridDim.x * TP_BLOCK) {
        const int64_t v = base + threadIdx.x;
        if (v > n_vtx) continue;
        const int64_t beg = sm_runs_before(head, scan, n6, sm_lower_bound(key, n6, (unsigned long long)v << 32));
        row_start[v] = beg;
        if (v == n_vtx) { cnt[SM_N_PAIRS] = (unsigned long long)beg; continue; }   // the one writer
        const int64_t len = sm_runs_before(head, scan, n6, sm_lower_bound(key, n6, (unsigned long long)(v + 1) << 32)) - beg;
        int c = IMMESH_VERTEX_UNUSED;
        if (len > 0) c = !pd_finite3(vtx, v) ? IMMESH_VERTEX_NOT_FINITE : flag[SM_FLAG_BORDER * n_vtx + v] ? IMMESH_VERTEX_BORDER : IMMESH_VERTEX_INTERIOR;
        vclass[v] = (int8_t)c;
        n_used += c != IMMESH_VERTEX_UNUSED;
        n_not_finite += c == IMMESH_VERTEX_NOT_FINITE;
        n_border += c == IMMESH_VERTEX_BORDER;
        n_interior += c == IMMESH_VERTEX_INTERIOR;
        valence = (uint32_t)len > valence ? (uint32_t)len : valence;
    }
    pd_block_add(n_used, cnt + SM_N_USED, lds);
    pd_block_add(n_not_finite, cnt + SM_N_NOT_FINITE, lds);
    pd_block_add(n_border, cnt + SM_N_BORDER, lds);
    pd_block_add(n_interior, cnt + SM_N_INTERIOR, lds);
    pd_block_max(valence, cnt + SM_MAX_VALENCE, lds);
}

__global__ void __launch_bounds__(TP_BLOCK) sm_lists_kernel(const unsigned long long* __restrict__ key, int64_t n6, int64_t n_vtx,
                                                            const int32_t* __restrict__ head, const int32_t* __restrict__ scan,
                                                            const int32_t* __restrict__ rstart, const int32_t* __restrict__ neighbours,
                                                            const int32_t* __restrict__ uses, const int8_t* __restrict__ vclass, int border,
                                                            int32_t* __restrict__ sn, int8_t* flag) {
    const int64_t p = (int64_t)blockIdx.x * TP_BLOCK + threadIdx.x;
    if (p >= n6 || p >= sm_runs_before(head, scan, n6, n6)) return;
    const int64_t at = rstart[p];
    if (at < 0 || at >= n6) return;
    const int64_t u = (int64_t)(key[at] >> 32);
    if (u >= n_vtx) return;                                     // the run of the faces that do not count
    const int64_t v = neighbours[p];
    bool in = false;
    if (v >= 0 && v < n_vtx && vclass[v] >= IMMESH_VERTEX_BORDER) {   // a neighbour is used: FINITE is BORDER or INTERIOR
        const int c = vclass[u];
        in = c == IMMESH_VERTEX_INTERIOR ||
             (c == IMMESH_VERTEX_BORDER && (border == IMMESH_SMOOTH_BORDER_FREE || (border == IMMESH_SMOOTH_BORDER_ALONG && uses[p] != 2)));
    }
    sn[p] = in ? (int32_t)v : -1;
    if (in) flag[SM_FLAG_MOVING * n_vtx + u] = 1;               // every writer stores the same value
}

__global__ void __launch_bounds__(TP_BLOCK) sm_step_kernel(const float* __restrict__ p_in, float* __restrict__ p_out, int64_t n_vtx,
                                                           const long long* __restrict__ row_start, const int32_t* __restrict__ sn, int64_t n6, double w,
                                                           unsigned long long* cnt) {
    __shared__ uint32_t lds[TP_BLOCK / 64];
    uint32_t n_held = 0;
    for (int64_t base = (int64_t)blockIdx.x * TP_BLOCK; base < n_vtx; base += (int64_t)gridDim.x * TP_BLOCK) {
        const int64_t v = base + threadIdx.x;
        if (v >= n_vtx) continue;
        const float x[3] = {p_in[3 * v], p_in[3 * v + 1], p_in[3 * v + 2]};
        float r[3] = {x[0], x[1], x[2]};
        int64_t beg = row_start[v], end = row_start[v + 1];
        if (beg < 0 || end > n6 || end < beg) end = beg;        // (the rows lie in the table: never)
        double s[3] = {0.0, 0.0, 0.0};
        int64_t n = 0;
        for (int64_t p = beg; p < end; p++) {
            const int64_t u = sn[p];
            if (u < 0 || u >= n_vtx) continue;
            s[0] = s[0] + (double)p_in[3 * u];
            s[1] = s[1] + (double)p_in[3 * u + 1];
            s[2] = s[2] + (double)p_in[3 * u + 2];
            n++;
        }
        if (n > 0) {
            for (int k = 0; k < 3; k++) {
                const double m = s[k] / (double)n, xk = (double)x[k];
                double t = m - xk;
                t = w * t;
                r[k] = (float)(xk + t);
            }
            if (!(isfinite(r[0]) && isfinite(r[1]) && isfinite(r[2]))) {
                r[0] = x[0]; r[1] = x[1]; r[2] = x[2];
                n_held++;
            }
        }
        p_out[3 * v] = r[0];
        p_out[3 * v + 1] = r[1];
        p_out[3 * v + 2] = r[2];
    }
    pd_block_add(n_held, cnt + SM_N_HELD, lds);
}

__global__ void __launch_bounds__(TP_BLOCK) sm_finish_kernel(const float* __restrict__ p0, const float* __restrict__ pn, int64_t n_vtx,
                                                             const int8_t* __restrict__ flag, unsigned long long* cnt) {
    __shared__ uint32_t lds[TP_BLOCK / 64];
    __shared__ double lds_d[TP_BLOCK / 64];
    uint32_t n_moving = 0, n_moved = 0;
    double disp2 = 0.0;
    for (int64_t base = (int64_t)blockIdx.x * TP_BLOCK; base < n_vtx; base += (int64_t)gridDim.x * TP_BLOCK) {
        const int64_t v = base + threadIdx.x;
        if (v >= n_vtx) continue;
        const float a[3] = {p0[3 * v], p0[3 * v + 1], p0[3 * v + 2]}, b[3] = {pn[3 * v], pn[3 * v + 1], pn[3 * v + 2]};
        n_moved += __float_as_uint(a[0]) != __float_as_uint(b[0]) || __float_as_uint(a[1]) != __float_as_uint(b[1]) ||
                   __float_as_uint(a[2]) != __float_as_uint(b[2]);
        if (flag[SM_FLAG_MOVING * n_vtx + v]) {                 // a MOVING vertex is finite before and after: d2 is no NaN
            n_moving++;
            const double d[3] = {(double)b[0] - (double)a[0], (double)b[1] - (double)a[1], (double)b[2] - (double)a[2]};
            const double d2 = rc_dot(d, d);
            disp2 = d2 > disp2 ? d2 : disp2;
        }
    }
    pd_block_add(n_moving, cnt + SM_N_MOVING, lds);
    pd_block_add(n_moved, cnt + SM_N_MOVED, lds);
    pd_block_max_f64(disp2, cnt + SM_MAX_DISP2, lds_d);
}

__global__ void __launch_bounds__(TP_BLOCK) sm_incidence_kernel(const float* __restrict__ vtx, int64_t n_vtx, const int32_t* __restrict__ faces,
                                                                int64_t n_faces, uint32_t* __restrict__ key, int32_t* __restrict__ val) {
    const int64_t f = (int64_t)blockIdx.x * TP_BLOCK + threadIdx.x;
    if (f >= n_faces) return;
    const int64_t i[3] = {faces[3 * f], faces[3 * f + 1], faces[3 * f + 2]};
    const bool in = pd_counts(i[0], i[1], i[2], n_vtx) && pd_finite3(vtx, i[0]) && pd_finite3(vtx, i[1]) && pd_finite3(vtx, i[2]);
    for (int e = 0; e < 3; e++) {
        key[3 * f + e] = in ? (uint32_t)i[e] : (uint32_t)n_vtx;
        val[3 * f + e] = (int32_t)f;
    }
}

__global__ void __launch_bounds__(TP_BLOCK) sm_normals_kernel(const float* __restrict__ vtx, int64_t n_vtx, const int32_t* __restrict__ faces,
                                                              int64_t n_faces, const uint32_t* __restrict__ key, const int32_t* __restrict__ val,
                                                              float* __restrict__ normals, unsigned long long* cnt) {
    __shared__ uint32_t lds[TP_BLOCK / 64];
    uint32_t n_zero = 0;
    const int64_t n3 = 3 * n_faces;
    for (int64_t base = (int64_t)blockIdx.x * TP_BLOCK; base < n_vtx; base += (int64_t)gridDim.x * TP_BLOCK) {
        const int64_t v = base + threadIdx.x;
        if (v >= n_vtx) continue;
        const int64_t beg = sm_lower_bound(key, n3, (uint32_t)v), end = sm_lower_bound(key, n3, (uint32_t)(v + 1));
        double s[3] = {0.0, 0.0, 0.0};
        for (int64_t p = beg; p < end; p++) {
            const int64_t f = val[p];
            if (f < 0 || f >= n_faces) continue;
            const int64_t ia = faces[3 * f], ib = faces[3 * f + 1], ic = faces[3 * f + 2];   // (a face of the table counts: its indices are in range)
            double ab[3], ac[3], n[3];
            for (int k = 0; k < 3; k++) {
                const double a = (double)vtx[3 * ia + k];
                ab[k] = (double)vtx[3 * ib + k] - a;
                ac[k] = (double)vtx[3 * ic + k] - a;
            }
            rc_cross(ab, ac, n);
            s[0] = s[0] + n[0];
            s[1] = s[1] + n[1];
            s[2] = s[2] + n[2];
        }
        const double len = sqrt(rc_dot(s, s));
        float o[3] = {0.0f, 0.0f, 0.0f};
        if (len > 0.0) for (int k = 0; k < 3; k++) o[k] = (float)(s[k] / len);
        else n_zero++;
        normals[3 * v] = o[0];
        normals[3 * v + 1] = o[1];
        normals[3 * v + 2] = o[2];
    }
    pd_block_add(n_zero, cnt + SM_N_ZERO, lds);
}

}  // namespace

void sm_launch_emit(hipStream_t s, const int32_t* faces, int64_t n_faces, int64_t n_vtx, unsigned long long* key, int32_t* val) {
    if (n_faces > 0) sm_emit_kernel<<<tp_grid(n_faces), TP_BLOCK, 0, s>>>(faces, n_faces, n_vtx, key, val);
}
void sm_launch_entries(hipStream_t s, const unsigned long long* key, int64_t n6, int64_t n_vtx, const int32_t* head, const int32_t* scan, const int32_t* rstart,
                       int32_t* neighbours, int32_t* uses, int8_t* flag) {
    if (n6 > 0) sm_entries_kernel<<<tp_grid(n6), TP_BLOCK, 0, s>>>(key, n6, n_vtx, head, scan, rstart, neighbours, uses, flag);
}
void sm_launch_rows(hipStream_t s, const float* vtx, int64_t n_vtx, const unsigned long long* key, int64_t n6, const int32_t* head, const int32_t* scan,
                    const int8_t* flag, long long* row_start, int8_t* vclass, unsigned long long* cnt) {
    if (n6 > 0 && n_vtx > 0) sm_rows_kernel<<<pd_grid_capped(n_vtx + 1), TP_BLOCK, 0, s>>>(vtx, n_vtx, key, n6, head, scan, flag, row_start, vclass, cnt);
}
void sm_launch_lists(hipStream_t s, const unsigned long long* key, int64_t n6, int64_t n_vtx, const int32_t* head, const int32_t* scan, const int32_t* rstart,
                     const int32_t* neighbours, const int32_t* uses, const int8_t* vclass, int border, int32_t* sn, int8_t* flag) {
    if (n6 > 0) sm_lists_kernel<<<tp_grid(n6), TP_BLOCK, 0, s>>>(key, n6, n_vtx, head, scan, rstart, neighbours, uses, vclass, border, sn, flag);
}
void sm_launch_step(hipStream_t s, const float* p_in, float* p_out, int64_t n_vtx, const long long* row_start, const int32_t* sn, int64_t n6, double w,
                    unsigned long long* cnt) {
    if (n_vtx > 0) sm_step_kernel<<<pd_grid_capped(n_vtx), TP_BLOCK, 0, s>>>(p_in, p_out, n_vtx, row_start, sn, n6, w, cnt);
}
void sm_launch_finish(hipStream_t s, const float* p0, const float* pn, int64_t n_vtx, const int8_t* flag, unsigned long long* cnt) {
    if (n_vtx > 0) sm_finish_kernel<<<pd_grid_capped(n_vtx), TP_BLOCK, 0, s>>>(p0, pn, n_vtx, flag, cnt);
}
void sm_launch_incidence(hipStream_t s, const float* vtx, int64_t n_vtx, const int32_t* faces, int64_t n_faces, uint32_t* key, int32_t* val) {
    if (n_faces > 0) sm_incidence_kernel<<<tp_grid(n_faces), TP_BLOCK, 0, s>>>(vtx, n_vtx, faces, n_faces, key, val);
}
void sm_launch_normals(hipStream_t s, const float* vtx, int64_t n_vtx, const int32_t* faces, int64_t n_faces, const uint32_t* key, const int32_t* val,
                       float* normals, unsigned long long* cnt) {
    if (n_vtx > 0) sm_normals_kernel<<<pd_grid_capped(n_vtx), TP_BLOCK, 0, s>>>(vtx, n_vtx, faces, n_faces, key, val, normals, cnt);
}
