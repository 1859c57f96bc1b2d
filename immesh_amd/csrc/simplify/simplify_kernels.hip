// Weld and vertex clustering of the caster's snapshot for gfx950 (include/immesh_simplify.h is the exact contract these kernels implement).
//   mark       one lane per face: the vertices of counting faces are used
//   keys       one lane per vertex: the cluster key and what the vertex is to the clustering.  A vertex that shares no cluster (unused, not finite,
//              outside the grid) gets a key above every other, so the stable pair sort (values = the vertex indices, ascending) leaves the members of
//              a cluster side by side in ascending index and the head of a run is its label
//   heads / runs / labels   run heads, and behind the scan of the heads the run's first and one-past-last position and every vertex' label: no lane
//              walks a run for this
//   clusters   behind the scan of the label flags (the cluster number by ascending label): the heads fill the cluster tables; FIRST is this gather
//   mean       one lane per cluster sums its run in the sorted order, which is ascending vertex index: the order IS the contract, so this walk is the
//              one place a lane follows a run, bounded by the run's length and by n_vtx
//   faces / duplicates / compact   the mapped triples; the kept candidates sorted by their sorted triple, the non-heads of a run are the duplicates
//   counters   integers, folded per workgroup before one atomic each (pass_dev.hpp's folds; the four launches that count go over their items in a
//              grid-stride loop, pd_grid_capped)
// Integers, float bits and one sequential double sum (compiled with -ffp-contract=off): the results do not depend on the order of anything.  Every
// scatter index is checked against its room before the store.
#include "simplify.hpp"
#include "../topology/topology_dev.hpp"
#include "../../../include/immesh_simplify.h"

namespace {

// sp_mark_kernel and sp_faces_kernel write the rule "a face counts" out, as they did before pass_dev.hpp, and do not call its pd_counts: through
// the function (here or as a private helper of this file) both kernels compile to other instructions, one apart and with two to three VGPRs more,
// and the simplify span then measured 0.005 ms above the parent's median in all seven cases of tools/simplify_bench.py over seven alternating runs,
// above the parent's range in one (0.5698 ms over 0.5604 - 0.5685).  Written out, both kernels are the parent's instruction for instruction.
__global__ void __launch_bounds__(TP_BLOCK) sp_mark_kernel(const int32_t* __restrict__ faces, int64_t n_faces, int64_t n_vtx, int32_t* state) {
    const int64_t f = (int64_t)blockIdx.x * TP_BLOCK + threadIdx.x;
    if (f >= n_faces) return;
    const int64_t a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    if (a < 0 || b < 0 || c < 0 || a >= n_vtx || b >= n_vtx || c >= n_vtx || a == b || b == c || a == c) return;
    state[a] = SP_NORMAL;                                       // every writer stores the same value
    state[b] = SP_NORMAL;
    state[c] = SP_NORMAL;
}

__global__ void __launch_bounds__(TP_BLOCK) sp_keys_kernel(const float* __restrict__ vtx, int64_t n_vtx, double cell, int32_t* __restrict__ state,
                                                           unsigned long long* __restrict__ k64, uint32_t* __restrict__ k32, int32_t* __restrict__ iota,
                                                           unsigned long long* cnt) {
    __shared__ uint32_t lds[TP_BLOCK / 64];
    uint32_t n_used = 0, n_not_finite = 0, n_outside = 0;
    for (int64_t base = (int64_t)blockIdx.x * TP_BLOCK; base < n_vtx; base += (int64_t)gridDim.x * TP_BLOCK) {
        const int64_t v = base + threadIdx.x;
        if (v >= n_vtx) continue;
        int32_t st = state[v];
        unsigned long long hi = SP_KEY_APART;
        uint32_t lo = 0xFFFFFFFFu;
        if (st == SP_NORMAL) {
            const float x[3] = {vtx[3 * v], vtx[3 * v + 1], vtx[3 * v + 2]};
            if (!pd_finite3(vtx, v)) st = SP_ALONE_NOT_FINITE;
            else if (cell > 0.0) {
                unsigned long long key = 0;
                for (int j = 0; j < 3; j++) {
                    const double q = floor((double)x[j] / cell);
                    if (!(q >= -1048576.0 && q < 1048576.0)) st = SP_ALONE_OUTSIDE;     // (an infinite quotient fails both)
                    else key = (key << RC_AXIS_BITS) | (unsigned long long)((long long)q + 1048576ll);
                }
                if (st == SP_NORMAL) { hi = key; lo = 0u; }
            } else {
                uint32_t k[3];
                for (int j = 0; j < 3; j++) k[j] = pd_key(x[j] == 0.0f ? 0.0f : x[j]);  // -0 onto +0
                hi = ((unsigned long long)k[0] << 32) | (unsigned long long)k[1];
                lo = k[2];
            }
        }
        state[v] = st;
        k64[v] = hi;
        k32[v] = lo;
        iota[v] = (int32_t)v;
        n_used += st != SP_UNUSED;
        n_not_finite += st == SP_ALONE_NOT_FINITE;
        n_outside += st == SP_ALONE_OUTSIDE;
    }
    pd_block_add(n_used, cnt + SP_N_USED, lds);
    pd_block_add(n_not_finite, cnt + SP_N_ALONE_NOT_FINITE, lds);
    pd_block_add(n_outside, cnt + SP_N_ALONE_OUTSIDE, lds);
}

__global__ void __launch_bounds__(TP_BLOCK) sp_gather64_kernel(const unsigned long long* __restrict__ k64, const int32_t* __restrict__ idx, int64_t n,
                                                               unsigned long long* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * TP_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int64_t j = idx[i];
    out[i] = j >= 0 && j < n ? k64[j] : SP_KEY_APART;           // (a permutation of 0 .. n - 1: always in range)
}

__global__ void __launch_bounds__(TP_BLOCK) sp_heads_kernel(const int32_t* __restrict__ sv, int64_t n_vtx, const int32_t* __restrict__ state,
                                                            const unsigned long long* __restrict__ k64, const uint32_t* __restrict__ k32,
                                                            int32_t* __restrict__ head) {
    const int64_t i = (int64_t)blockIdx.x * TP_BLOCK + threadIdx.x;
    if (i >= n_vtx) return;
    int32_t h = 1;
    if (i > 0) {
        const int64_t v = sv[i], p = sv[i - 1];
        if (v >= 0 && v < n_vtx && p >= 0 && p < n_vtx)
            h = !(state[v] == SP_NORMAL && state[p] == SP_NORMAL && k64[v] == k64[p] && k32[v] == k32[p]);
    }
    head[i] = h;
}

__global__ void __launch_bounds__(TP_BLOCK) sp_runs_kernel(int64_t n_vtx, const int32_t* __restrict__ head, const int32_t* __restrict__ scan,
                                                           int32_t* __restrict__ rstart, int32_t* __restrict__ rend) {
    const int64_t i = (int64_t)blockIdx.x * TP_BLOCK + threadIdx.x;
    if (i >= n_vtx) return;
    const int32_t h = head[i];
    const int64_t r = (int64_t)scan[i] + h - 1;
    if (r < 0 || r >= n_vtx) return;                            // (position 0 is a head: never)
    if (h) rstart[r] = (int32_t)i;
    if (i + 1 == n_vtx || head[i + 1]) rend[r] = (int32_t)(i + 1);
}

__global__ void __launch_bounds__(TP_BLOCK) sp_labels_kernel(const int32_t* __restrict__ sv, int64_t n_vtx, const int32_t* __restrict__ state,
                                                             const int32_t* __restrict__ head, const int32_t* __restrict__ scan,
                                                             const int32_t* __restrict__ rstart, int32_t* __restrict__ lab, int32_t* __restrict__ islab) {
    const int64_t i = (int64_t)blockIdx.x * TP_BLOCK + threadIdx.x;
    if (i >= n_vtx) return;
    const int32_t h = head[i];
    const int64_t v = sv[i], r = (int64_t)scan[i] + h - 1;
    if (v < 0 || v >= n_vtx || r < 0 || r >= n_vtx) return;
    const int64_t at = rstart[r];
    if (at < 0 || at >= n_vtx) return;
    lab[v] = sv[at];
    islab[v] = h && state[v] != SP_UNUSED ? 1 : 0;
}

__global__ void __launch_bounds__(TP_BLOCK) sp_clusters_kernel(const float* __restrict__ vtx, const int32_t* __restrict__ sv, int64_t n_vtx,
                                                               const int32_t* __restrict__ state, const int32_t* __restrict__ head,
                                                               const int32_t* __restrict__ scan, const int32_t* __restrict__ rend,
                                                               const int32_t* __restrict__ cnum, int32_t* __restrict__ first, int32_t* __restrict__ nmem,
                                                               int32_t* __restrict__ cstart, float* __restrict__ vtx_out, unsigned long long* cnt) {
    __shared__ uint32_t lds[TP_BLOCK / 64];
    uint32_t n_mine = 0, largest = 0;
    for (int64_t base = (int64_t)blockIdx.x * TP_BLOCK; base < n_vtx; base += (int64_t)gridDim.x * TP_BLOCK) {
        const int64_t i = base + threadIdx.x;
        if (i >= n_vtx || !head[i]) continue;
        const int64_t v = sv[i], r = scan[i];
        if (v >= 0 && v < n_vtx && r < n_vtx && state[v] != SP_UNUSED) {
            const int64_t c = cnum[v], len = (int64_t)rend[r] - i;
            if (c >= 0 && c < n_vtx && len >= 1 && i + len <= n_vtx) {
                n_mine++;
                largest = (uint32_t)len > largest ? (uint32_t)len : largest;
                first[c] = (int32_t)v;
                nmem[c] = (int32_t)len;
                cstart[c] = (int32_t)i;
                vtx_out[3 * c] = vtx[3 * v];
                vtx_out[3 * c + 1] = vtx[3 * v + 1];
                vtx_out[3 * c + 2] = vtx[3 * v + 2];
            }
        }
    }
    pd_block_add(n_mine, cnt + SP_N_CLUSTERS, lds);
    pd_block_max(largest, cnt + SP_LARGEST, lds);
}

__global__ void __launch_bounds__(TP_BLOCK) sp_mean_kernel(const float* __restrict__ vtx, const int32_t* __restrict__ sv, int64_t n_vtx,
                                                           const int32_t* __restrict__ nmem, const int32_t* __restrict__ cstart,
                                                           const unsigned long long* __restrict__ cnt, float* __restrict__ vtx_out) {
    const int64_t c = (int64_t)blockIdx.x * TP_BLOCK + threadIdx.x;
    if (c >= n_vtx || c >= (int64_t)cnt[SP_N_CLUSTERS]) return;
    const int64_t n = nmem[c], at = cstart[c];
    if (n < 2 || at < 0 || at + n > n_vtx) return;              // one member: its floats stay as the gather left them
    double s[3] = {0.0, 0.0, 0.0};
    for (int64_t k = 0; k < n; k++) {
        const int64_t v = sv[at + k];
        if (v < 0 || v >= n_vtx) return;
        s[0] = s[0] + (double)vtx[3 * v];
        s[1] = s[1] + (double)vtx[3 * v + 1];
        s[2] = s[2] + (double)vtx[3 * v + 2];
    }
    for (int j = 0; j < 3; j++) vtx_out[3 * c + j] = (float)(s[j] / (double)n);
}

__global__ void __launch_bounds__(TP_BLOCK) sp_vmap_kernel(int64_t n_vtx, const int32_t* __restrict__ state, const int32_t* __restrict__ lab,
                                                           const int32_t* __restrict__ cnum, int32_t* __restrict__ vmap) {
    const int64_t v = (int64_t)blockIdx.x * TP_BLOCK + threadIdx.x;
    if (v >= n_vtx) return;
    int32_t m = -1;
    if (state[v] != SP_UNUSED) {
        const int64_t l = lab[v];
        if (l >= 0 && l < n_vtx) m = cnum[l];
    }
    vmap[v] = m;
}

__global__ void __launch_bounds__(TP_BLOCK) sp_faces_kernel(const int32_t* __restrict__ faces, int64_t n_faces, int64_t n_vtx, const int32_t* __restrict__ vmap,
                                                            int8_t* __restrict__ fstatus, int32_t* __restrict__ keep, unsigned long long* __restrict__ f64,
                                                            uint32_t* __restrict__ f32, int32_t* __restrict__ iota, unsigned long long* cnt) {
    __shared__ uint32_t lds[TP_BLOCK / 64];
    uint32_t n_not_counting = 0, n_collapsed = 0;
    for (int64_t base = (int64_t)blockIdx.x * TP_BLOCK; base < n_faces; base += (int64_t)gridDim.x * TP_BLOCK) {
        const int64_t f = base + threadIdx.x;
        if (f >= n_faces) continue;
        int status;
        const int64_t a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
        unsigned long long hi = SP_KEY_APART;
        uint32_t lo = 0xFFFFFFFFu;
        if (a < 0 || b < 0 || c < 0 || a >= n_vtx || b >= n_vtx || c >= n_vtx || a == b || b == c || a == c) status = IMMESH_FACE_NOT_COUNTING;   // (written out: above)
        else {
            const int32_t g0 = vmap[a], g1 = vmap[b], g2 = vmap[c];
            if (g0 == g1 || g1 == g2 || g0 == g2 || g0 < 0 || g1 < 0 || g2 < 0) status = IMMESH_FACE_COLLAPSED;   // (a used vertex has a cluster: never < 0)
            else {
                status = IMMESH_FACE_KEPT;
                const uint32_t lo01 = (uint32_t)min(g0, g1), hi01 = (uint32_t)max(g0, g1), u2 = (uint32_t)g2;
                const uint32_t s0 = min(lo01, u2), s2 = max(hi01, u2), s1 = lo01 + hi01 + u2 - s0 - s2;            // (modulo 2^32: the middle one fits)
                hi = ((unsigned long long)s0 << 32) | (unsigned long long)s1;
                lo = s2;
            }
        }
        fstatus[f] = (int8_t)status;
        keep[f] = status == IMMESH_FACE_KEPT ? 1 : 0;
        if (f64) { f64[f] = hi; f32[f] = lo; iota[f] = (int32_t)f; }
        n_not_counting += status == IMMESH_FACE_NOT_COUNTING;
        n_collapsed += status == IMMESH_FACE_COLLAPSED;
    }
    pd_block_add(n_not_counting, cnt + SP_N_NOT_COUNTING, lds);
    pd_block_add(n_collapsed, cnt + SP_N_COLLAPSED, lds);
}

__global__ void __launch_bounds__(TP_BLOCK) sp_duplicates_kernel(const int32_t* __restrict__ sf, int64_t n_faces, const unsigned long long* __restrict__ f64,
                                                                 const uint32_t* __restrict__ f32, int8_t* __restrict__ fstatus, int32_t* __restrict__ keep,
                                                                 unsigned long long* cnt) {
    __shared__ uint32_t lds[TP_BLOCK / 64];
    uint32_t n_dup = 0;
    for (int64_t base = (int64_t)blockIdx.x * TP_BLOCK; base < n_faces; base += (int64_t)gridDim.x * TP_BLOCK) {
        const int64_t i = base + threadIdx.x;
        if (i == 0 || i >= n_faces) continue;
        const int64_t f = sf[i], p = sf[i - 1];
        if (f >= 0 && f < n_faces && p >= 0 && p < n_faces) {
            const unsigned long long k = f64[f];                // a face that is not a candidate keeps SP_KEY_APART: the keys tell, nothing here is read
            const bool dup = k != SP_KEY_APART && k == f64[p] && f32[f] == f32[p];   // that another lane of this launch writes
            if (dup) { fstatus[f] = IMMESH_FACE_DUPLICATE; keep[f] = 0; n_dup++; }
        }
    }
    pd_block_add(n_dup, cnt + SP_N_DUPLICATE, lds);
}

__global__ void __launch_bounds__(TP_BLOCK) sp_compact_kernel(const int32_t* __restrict__ faces, int64_t n_faces, const int32_t* __restrict__ vmap,
                                                              const int32_t* __restrict__ keep, const int32_t* __restrict__ koff,
                                                              int32_t* __restrict__ faces_out, int32_t* __restrict__ fmap, unsigned long long* cnt) {
    const int64_t f = (int64_t)blockIdx.x * TP_BLOCK + threadIdx.x;
    if (f >= n_faces) return;
    const int32_t k = keep[f];
    const int64_t j = koff[f];
    if (f == n_faces - 1) cnt[SP_N_FACES_OUT] = (unsigned long long)(j + k);
    if (!k || j < 0 || j >= n_faces) { fmap[f] = -1; return; }
    fmap[f] = (int32_t)j;
    for (int e = 0; e < 3; e++) faces_out[3 * j + e] = vmap[faces[3 * f + e]];   // (a kept face counts: its indices are in range)
}

}  // namespace

void sp_launch_mark(hipStream_t s, const int32_t* faces, int64_t n_faces, int64_t n_vtx, int32_t* state) {
    if (n_faces > 0) sp_mark_kernel<<<tp_grid(n_faces), TP_BLOCK, 0, s>>>(faces, n_faces, n_vtx, state);
}
void sp_launch_keys(hipStream_t s, const float* vtx, int64_t n_vtx, double cell, int32_t* state, unsigned long long* k64, uint32_t* k32, int32_t* iota,
                    unsigned long long* cnt) {
    if (n_vtx > 0) sp_keys_kernel<<<pd_grid_capped(n_vtx), TP_BLOCK, 0, s>>>(vtx, n_vtx, cell, state, k64, k32, iota, cnt);
}
void sp_launch_gather64(hipStream_t s, const unsigned long long* k64, const int32_t* idx, int64_t n, unsigned long long* out) {
    if (n > 0) sp_gather64_kernel<<<tp_grid(n), TP_BLOCK, 0, s>>>(k64, idx, n, out);
}
void sp_launch_heads(hipStream_t s, const int32_t* sv, int64_t n_vtx, const int32_t* state, const unsigned long long* k64, const uint32_t* k32, int32_t* head) {
    if (n_vtx > 0) sp_heads_kernel<<<tp_grid(n_vtx), TP_BLOCK, 0, s>>>(sv, n_vtx, state, k64, k32, head);
}
void sp_launch_runs(hipStream_t s, int64_t n_vtx, const int32_t* head, const int32_t* scan, int32_t* rstart, int32_t* rend) {
    if (n_vtx > 0) sp_runs_kernel<<<tp_grid(n_vtx), TP_BLOCK, 0, s>>>(n_vtx, head, scan, rstart, rend);
}
void sp_launch_labels(hipStream_t s, const int32_t* sv, int64_t n_vtx, const int32_t* state, const int32_t* head, const int32_t* scan, const int32_t* rstart,
                      int32_t* lab, int32_t* islab) {
    if (n_vtx > 0) sp_labels_kernel<<<tp_grid(n_vtx), TP_BLOCK, 0, s>>>(sv, n_vtx, state, head, scan, rstart, lab, islab);
}
void sp_launch_clusters(hipStream_t s, const float* vtx, const int32_t* sv, int64_t n_vtx, const int32_t* state, const int32_t* head, const int32_t* scan,
                        const int32_t* rend, const int32_t* cnum, int32_t* first, int32_t* nmem, int32_t* cstart, float* vtx_out, unsigned long long* cnt) {
    if (n_vtx > 0) sp_clusters_kernel<<<pd_grid_capped(n_vtx), TP_BLOCK, 0, s>>>(vtx, sv, n_vtx, state, head, scan, rend, cnum, first, nmem, cstart, vtx_out, cnt);
}
void sp_launch_mean(hipStream_t s, const float* vtx, const int32_t* sv, int64_t n_vtx, const int32_t* nmem, const int32_t* cstart, const unsigned long long* cnt,
                    float* vtx_out) {
    if (n_vtx > 0) sp_mean_kernel<<<tp_grid(n_vtx), TP_BLOCK, 0, s>>>(vtx, sv, n_vtx, nmem, cstart, cnt, vtx_out);
}
void sp_launch_vmap(hipStream_t s, int64_t n_vtx, const int32_t* state, const int32_t* lab, const int32_t* cnum, int32_t* vmap) {
    if (n_vtx > 0) sp_vmap_kernel<<<tp_grid(n_vtx), TP_BLOCK, 0, s>>>(n_vtx, state, lab, cnum, vmap);
}
void sp_launch_faces(hipStream_t s, const int32_t* faces, int64_t n_faces, int64_t n_vtx, const int32_t* vmap, int8_t* fstatus, int32_t* keep,
                     unsigned long long* f64, uint32_t* f32, int32_t* iota, unsigned long long* cnt) {
    if (n_faces > 0) sp_faces_kernel<<<pd_grid_capped(n_faces), TP_BLOCK, 0, s>>>(faces, n_faces, n_vtx, vmap, fstatus, keep, f64, f32, iota, cnt);
}
void sp_launch_duplicates(hipStream_t s, const int32_t* sf, int64_t n_faces, const unsigned long long* f64, const uint32_t* f32, int8_t* fstatus, int32_t* keep,
                          unsigned long long* cnt) {
    if (n_faces > 0) sp_duplicates_kernel<<<pd_grid_capped(n_faces), TP_BLOCK, 0, s>>>(sf, n_faces, f64, f32, fstatus, keep, cnt);
}
void sp_launch_compact(hipStream_t s, const int32_t* faces, int64_t n_faces, const int32_t* vmap, const int32_t* keep, const int32_t* koff, int32_t* faces_out,
                       int32_t* fmap, unsigned long long* cnt) {
    if (n_faces > 0) sp_compact_kernel<<<tp_grid(n_faces), TP_BLOCK, 0, s>>>(faces, n_faces, vmap, keep, koff, faces_out, fmap, cnt);
}
