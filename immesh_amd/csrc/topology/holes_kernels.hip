// The holes of the analysed snapshot for gfx950 (include/immesh_topology.h, the Holes rule, is the exact contract these kernels implement).
//   init       one lane per vertex: the loop's label, the root of the analysis' vparent (parent <= x: a root is its class's smallest vertex)
//   degrees    one lane per SORTED half-edge; the head of a run of one is a boundary half-edge and counts itself at its tail and its head
//   flags      one lane per vertex: a boundary vertex with other degrees than one in, one out marks its loop as not simple
//   rank_init  the list ranking's start.  A simple loop is one directed cycle; broken at its label it is a list that ends at the vertex whose
//              successor is the label.  jump: d[v] += d[nxt[v]], nxt[v] = nxt[nxt[v]], from one buffer into the other, one launch per round,
//              ceil(log2(the largest loop's edges)) rounds: a round reads only what an earlier launch wrote, so no lane waits for another, no load
//              can see a stale line of this launch, and no lane walks a loop -- the border of a sheet costs a lane what a one-cell hole does.
//              Afterwards d is the distance to the list's end and a vertex's place in the cycle is n_edges - 1 - d.
//   boxes      one lane per vertex, atomicMin / atomicMax on order-preserving keys, folded per wavefront and loop first (tp_components_kernel's fold)
//   scatter    the cycles into their slots; every slot remembers its loop, so that the two passes over the slots need no search
//   limits / chords / decide   the status of every loop; a chord is looked up in the analysis' sorted keys by binary search
//   emit       the fan's faces behind the prefix sum of the filled loops' n_edges - 2
// All of it integers and min / max: the results do not depend on the order of anything.
#include "topology.hpp"
#include "topology_dev.hpp"
#include "../../../include/immesh_topology.h"

namespace {

__global__ void __launch_bounds__(TP_BLOCK) hl_init_kernel(int64_t n_vtx, const int32_t* __restrict__ vparent, int32_t* __restrict__ vt) {
    const int64_t v = (int64_t)blockIdx.x * TP_BLOCK + threadIdx.x;
    if (v >= n_vtx) return;
    int32_t x = (int32_t)v;
    for (int32_t p = vparent[x]; p != x; p = vparent[x]) x = p;   // strictly downwards: it ends
    vt[HV_LAB * n_vtx + v] = x;
    vt[HV_IN * n_vtx + v] = 0;
    vt[HV_OUT * n_vtx + v] = 0;
    vt[HV_SUCC * n_vtx + v] = -1;
    vt[HV_LFACE * n_vtx + v] = -1;
    vt[HV_BAD * n_vtx + v] = 0;
}

__global__ void __launch_bounds__(TP_BLOCK) hl_degrees_kernel(const unsigned long long* __restrict__ key, const int32_t* __restrict__ val, int64_t n_half,
                                                              const int32_t* __restrict__ faces, int64_t n_vtx, int32_t* vt) {
    const int64_t i = (int64_t)blockIdx.x * TP_BLOCK + threadIdx.x;
    if (i >= n_half) return;
    const unsigned long long k = key[i];
    if ((i > 0 && key[i - 1] == k) || (i + 1 < n_half && key[i + 1] == k)) return;
    const int32_t h = val[i];
    const int64_t f = h / 3;
    const int j = h - 3 * (int32_t)f;
    const int64_t t = faces[3 * f + j], hd = faces[3 * f + (j == 2 ? 0 : j + 1)];   // (a counting face: its indices are in range)
    atomicAdd(vt + HV_OUT * n_vtx + t, 1);
    atomicAdd(vt + HV_IN * n_vtx + hd, 1);
    vt[HV_SUCC * n_vtx + t] = (int32_t)hd;     // several writers only where HV_OUT ends above 1, and there nobody reads it
    vt[HV_LFACE * n_vtx + t] = (int32_t)f;
}

__global__ void __launch_bounds__(TP_BLOCK) hl_flags_kernel(int64_t n_vtx, int32_t* vt) {
    const int64_t v = (int64_t)blockIdx.x * TP_BLOCK + threadIdx.x;
    if (v >= n_vtx) return;
    const int32_t in = vt[HV_IN * n_vtx + v], out = vt[HV_OUT * n_vtx + v], lab = vt[HV_LAB * n_vtx + v];
    const bool boundary = (in | out) != 0;
    if (boundary && !(in == 1 && out == 1)) vt[HV_BAD * n_vtx + lab] = 1;
    vt[HV_ROOT * n_vtx + v] = boundary && lab == (int32_t)v ? 1 : 0;
}

__global__ void __launch_bounds__(TP_BLOCK) hl_rank_init_kernel(int64_t n_vtx, const int32_t* __restrict__ vt, const int32_t* __restrict__ loop_cnt,
                                                                int64_t n_loops, int32_t* __restrict__ lt, uint32_t* __restrict__ box, HlRank* __restrict__ rk) {
    const int64_t v = (int64_t)blockIdx.x * TP_BLOCK + threadIdx.x;
    if (v >= n_vtx) return;
    const int32_t lab = vt[HV_LAB * n_vtx + v];
    const bool boundary = (vt[HV_IN * n_vtx + v] | vt[HV_OUT * n_vtx + v]) != 0;
    const bool simple = boundary && vt[HV_BAD * n_vtx + lab] == 0;
    const int32_t s1 = vt[HV_SUCC * n_vtx + v];
    HlRank r = {-1, 0};
    if (simple && s1 != lab) { r.nxt = s1; r.d = 1; }
    rk[v] = r;
    if (!vt[HV_ROOT * n_vtx + v]) return;
    const int64_t l = vt[HV_NUM * n_vtx + v];
    if (l >= n_loops) return;                                  // (the analysis counted the same labels: never)
    const int32_t n = loop_cnt[v];
    int32_t status = simple ? IMMESH_HOLE_FILLED : IMMESH_HOLE_NONSIMPLE;
    if (simple && n == 3) {
        const int32_t s2 = vt[HV_SUCC * n_vtx + s1];
        const int32_t f0 = vt[HV_LFACE * n_vtx + v];
        if (f0 == vt[HV_LFACE * n_vtx + s1] && f0 == vt[HV_LFACE * n_vtx + s2]) status = IMMESH_HOLE_OUTLINE;
    }
    lt[HL_FIRST * n_loops + l] = (int32_t)v;
    lt[HL_NEDGES * n_loops + l] = n;
    lt[HL_STATUS * n_loops + l] = status;
    lt[HL_SLEN * n_loops + l] = simple ? n : 0;
    lt[HL_BLOCKED * n_loops + l] = 0;
    for (int j = 0; j < 3; j++) { box[6 * l + j] = TP_KEY_NONE_LO; box[6 * l + 3 + j] = TP_KEY_NONE_HI; }
}

__global__ void __launch_bounds__(TP_BLOCK) hl_jump_kernel(int64_t n_vtx, const HlRank* __restrict__ in, HlRank* __restrict__ out) {
    const int64_t v = (int64_t)blockIdx.x * TP_BLOCK + threadIdx.x;
    if (v >= n_vtx) return;
    HlRank r = in[v];
    if (r.nxt >= 0) {
        const HlRank q = in[r.nxt];
        r.d += q.d;
        r.nxt = q.nxt;
    }
    out[v] = r;
}

__global__ void __launch_bounds__(TP_BLOCK) hl_boxes_kernel(const float* __restrict__ vtx, int64_t n_vtx, const int32_t* __restrict__ vt, int64_t n_loops,
                                                            uint32_t* box) {
    const int64_t v = (int64_t)blockIdx.x * TP_BLOCK + threadIdx.x;
    int32_t l = -1;
    uint32_t lo[3] = {TP_KEY_NONE_LO, TP_KEY_NONE_LO, TP_KEY_NONE_LO}, hi[3] = {TP_KEY_NONE_HI, TP_KEY_NONE_HI, TP_KEY_NONE_HI};
    if (v < n_vtx && (vt[HV_IN * n_vtx + v] | vt[HV_OUT * n_vtx + v]) != 0) {
        l = vt[HV_NUM * n_vtx + vt[HV_LAB * n_vtx + v]];
        if (l >= n_loops) l = -1;
        for (int j = 0; j < 3; j++) {
            const float x = vtx[3 * v + j];
            if (l >= 0 && isfinite(x)) lo[j] = hi[j] = pd_key(x);
        }
    }
    // the fold of tp_components_kernel: one atomic per word, wavefront and loop for the first TP_FOLD_ROUNDS loops of the wavefront (the border of a
    // sheet runs through consecutive vertices), single atomics for the lanes left over
    unsigned long long todo = __ballot(l >= 0);
    for (int round = 0; todo != 0 && round < TP_FOLD_ROUNDS; round++) {
        const int leader = __ffsll((long long)todo) - 1;
        const int32_t l0 = __shfl(l, leader, 64);
        const bool mine = l == l0;
        const unsigned long long m = __ballot(mine);
        uint32_t a[3], b[3];
        for (int j = 0; j < 3; j++) {
            a[j] = pd_wave_min(mine ? lo[j] : TP_KEY_NONE_LO);
            b[j] = pd_wave_max(mine ? hi[j] : TP_KEY_NONE_HI);
        }
        if ((int)(threadIdx.x & 63) == leader)
            for (int j = 0; j < 3; j++) {
                if (a[j] != TP_KEY_NONE_LO) atomicMin(box + 6 * (int64_t)l0 + j, a[j]);
                if (b[j] != TP_KEY_NONE_HI) atomicMax(box + 6 * (int64_t)l0 + 3 + j, b[j]);
            }
        todo &= ~m;
    }
    if ((todo >> (threadIdx.x & 63)) & 1ull)
        for (int j = 0; j < 3; j++) {
            if (lo[j] != TP_KEY_NONE_LO) atomicMin(box + 6 * (int64_t)l + j, lo[j]);
            if (hi[j] != TP_KEY_NONE_HI) atomicMax(box + 6 * (int64_t)l + 3 + j, hi[j]);
        }
}

__global__ void __launch_bounds__(TP_BLOCK) hl_scatter_kernel(int64_t n_vtx, const int32_t* __restrict__ vt, const HlRank* __restrict__ rk,
                                                              const int32_t* __restrict__ lt, int64_t n_loops, int32_t* __restrict__ cycle,
                                                              int32_t* __restrict__ cloop, int64_t n_room) {
    const int64_t v = (int64_t)blockIdx.x * TP_BLOCK + threadIdx.x;
    if (v >= n_vtx || (vt[HV_IN * n_vtx + v] | vt[HV_OUT * n_vtx + v]) == 0) return;
    const int32_t lab = vt[HV_LAB * n_vtx + v];
    if (vt[HV_BAD * n_vtx + lab]) return;
    const int64_t l = vt[HV_NUM * n_vtx + lab];
    if (l >= n_loops) return;
    const int64_t n = lt[HL_NEDGES * n_loops + l], pos = n - 1 - rk[v].d, p = lt[HL_CSTART * n_loops + l] + pos;
    if (pos < 0 || pos >= n || p >= n_room) return;             // (a ranked cycle: never)
    cycle[p] = (int32_t)v;
    cloop[p] = (int32_t)l;
}

__global__ void __launch_bounds__(TP_BLOCK) hl_limits_kernel(int64_t n_loops, int32_t* __restrict__ lt, const uint32_t* __restrict__ box, int64_t max_edges,
                                                             double max_diagonal, int64_t* __restrict__ cstart64, unsigned long long* cnt) {
    const int64_t l = (int64_t)blockIdx.x * TP_BLOCK + threadIdx.x;
    if (l >= n_loops) return;
    const int32_t n = lt[HL_NEDGES * n_loops + l], slen = lt[HL_SLEN * n_loops + l], start = lt[HL_CSTART * n_loops + l];
    int32_t status = lt[HL_STATUS * n_loops + l];
    if (status == IMMESH_HOLE_FILLED) {
        if ((int64_t)n > max_edges) status = IMMESH_HOLE_TOO_LONG;
        else if (max_diagonal > 0.0) {
            double d[3];
            bool have = true;
            for (int j = 0; j < 3; j++) {
                const uint32_t lo = box[6 * l + j], hi = box[6 * l + 3 + j];
                have = have && lo != TP_KEY_NONE_LO && hi != TP_KEY_NONE_HI;
                d[j] = (double)pd_unkey(hi) - (double)pd_unkey(lo);
            }
            if (!have || (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2] > max_diagonal * max_diagonal) status = IMMESH_HOLE_TOO_WIDE;
        }
        lt[HL_STATUS * n_loops + l] = status;
    }
    cstart64[l] = slen > 0 ? (int64_t)start : -1;
    if (l == n_loops - 1) cnt[HC_N_CYCLE] = (unsigned long long)((int64_t)start + slen);
}

__global__ void __launch_bounds__(TP_BLOCK) hl_chords_kernel(int64_t n_room, const unsigned long long* __restrict__ cnt, const int32_t* __restrict__ cycle,
                                                             const int32_t* __restrict__ cloop, const unsigned long long* __restrict__ key, int64_t n_half,
                                                             int32_t* lt, int64_t n_loops) {
    const int64_t p = (int64_t)blockIdx.x * TP_BLOCK + threadIdx.x;
    if (p >= n_room || p >= (int64_t)cnt[HC_N_CYCLE]) return;
    const int64_t l = cloop[p];
    if (l < 0 || l >= n_loops || lt[HL_STATUS * n_loops + l] != IMMESH_HOLE_FILLED) return;
    const int64_t start = lt[HL_CSTART * n_loops + l], k = p - start, n = lt[HL_NEDGES * n_loops + l];
    if (k < 2 || k > n - 2) return;
    const uint32_t a = (uint32_t)cycle[start], b = (uint32_t)cycle[p];
    const unsigned long long want = ((unsigned long long)(a < b ? a : b) << 32) | (unsigned long long)(a < b ? b : a);
    int64_t lo = 0, hi = n_half;                                // the first key >= want
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (key[mid] < want) lo = mid + 1;
        else hi = mid;
    }
    if (lo < n_half && key[lo] == want) lt[HL_BLOCKED * n_loops + l] = 1;   // every writer stores the same value
}

__global__ void __launch_bounds__(TP_BLOCK) hl_decide_kernel(int64_t n_loops, int32_t* __restrict__ lt, unsigned long long* cnt) {
    const int64_t l = (int64_t)blockIdx.x * TP_BLOCK + threadIdx.x;
    const bool in = l < n_loops;
    int32_t status = -1, n = 0;
    if (in) {
        status = lt[HL_STATUS * n_loops + l];
        n = lt[HL_NEDGES * n_loops + l];
        if (status == IMMESH_HOLE_FILLED && lt[HL_BLOCKED * n_loops + l]) status = IMMESH_HOLE_BLOCKED;
        lt[HL_STATUS * n_loops + l] = status;
        lt[HL_FILL * n_loops + l] = status == IMMESH_HOLE_FILLED ? n - 2 : 0;
    }
    const bool simple = in && status != IMMESH_HOLE_NONSIMPLE, filled = in && status == IMMESH_HOLE_FILLED;
    tp_count(simple, cnt + HC_N_SIMPLE);
    tp_count(in && status == IMMESH_HOLE_NONSIMPLE, cnt + HC_N_NONSIMPLE);
    tp_count(in && status == IMMESH_HOLE_OUTLINE, cnt + HC_N_OUTLINE);
    tp_count(in && status == IMMESH_HOLE_TOO_LONG, cnt + HC_N_TOO_LONG);
    tp_count(in && status == IMMESH_HOLE_TOO_WIDE, cnt + HC_N_TOO_WIDE);
    tp_count(in && status == IMMESH_HOLE_BLOCKED, cnt + HC_N_BLOCKED);
    tp_count(filled, cnt + HC_N_FILLED);
    const uint32_t closed = pd_wave_sum(filled ? (uint32_t)n : 0u);   // (a wavefront's loops have fewer than 2^31 - 2 boundary edges together)
    const uint32_t largest = pd_wave_max(simple ? (uint32_t)n : 0u);
    if ((threadIdx.x & 63) == 0) {
        if (closed) atomicAdd(cnt + HC_N_CLOSED, (unsigned long long)closed);
        if (largest) atomicMax(cnt + HC_LARGEST_SIMPLE, (unsigned long long)largest);
    }
}

__global__ void __launch_bounds__(TP_BLOCK) hl_emit_kernel(int64_t n_room, const int32_t* __restrict__ cycle, const int32_t* __restrict__ cloop,
                                                           const int32_t* __restrict__ lt, int64_t n_loops, int32_t* __restrict__ new_faces,
                                                           int32_t* __restrict__ new_loop, unsigned long long* cnt) {
    const int64_t p = (int64_t)blockIdx.x * TP_BLOCK + threadIdx.x;
    if (p == 0) cnt[HC_N_NEW] = (unsigned long long)((int64_t)lt[HL_FOFF * n_loops + n_loops - 1] + lt[HL_FILL * n_loops + n_loops - 1]);
    if (p >= n_room || p >= (int64_t)cnt[HC_N_CYCLE]) return;
    const int64_t l = cloop[p];
    if (l < 0 || l >= n_loops || lt[HL_STATUS * n_loops + l] != IMMESH_HOLE_FILLED) return;
    const int64_t start = lt[HL_CSTART * n_loops + l], k = p - start, n = lt[HL_NEDGES * n_loops + l];
    if (k < 1 || k > n - 2) return;
    const int64_t j = (int64_t)lt[HL_FOFF * n_loops + l] + k - 1;
    if (j >= n_room) return;                                    // (the fans have fewer faces than the cycles have slots: never)
    new_faces[3 * j] = cycle[start];
    new_faces[3 * j + 1] = cycle[p + 1];                        // k + 1 <= n - 1: inside the loop's slots
    new_faces[3 * j + 2] = cycle[p];
    new_loop[j] = (int32_t)l;
}

}  // namespace

void hl_launch_init(hipStream_t s, int64_t n_vtx, const int32_t* vparent, int32_t* vt) {
    if (n_vtx > 0) hl_init_kernel<<<tp_grid(n_vtx), TP_BLOCK, 0, s>>>(n_vtx, vparent, vt);
}
void hl_launch_degrees(hipStream_t s, const unsigned long long* key, const int32_t* val, int64_t n_half, const int32_t* faces, int64_t n_vtx, int32_t* vt) {
    if (n_half > 0) hl_degrees_kernel<<<tp_grid(n_half), TP_BLOCK, 0, s>>>(key, val, n_half, faces, n_vtx, vt);
}
void hl_launch_flags(hipStream_t s, int64_t n_vtx, int32_t* vt) {
    if (n_vtx > 0) hl_flags_kernel<<<tp_grid(n_vtx), TP_BLOCK, 0, s>>>(n_vtx, vt);
}
void hl_launch_rank_init(hipStream_t s, int64_t n_vtx, const int32_t* vt, const int32_t* loop_cnt, int64_t n_loops, int32_t* lt, uint32_t* box, HlRank* rk) {
    if (n_vtx > 0) hl_rank_init_kernel<<<tp_grid(n_vtx), TP_BLOCK, 0, s>>>(n_vtx, vt, loop_cnt, n_loops, lt, box, rk);
}
void hl_launch_jump(hipStream_t s, int64_t n_vtx, const HlRank* in, HlRank* out) {
    if (n_vtx > 0) hl_jump_kernel<<<tp_grid(n_vtx), TP_BLOCK, 0, s>>>(n_vtx, in, out);
}
void hl_launch_boxes(hipStream_t s, const float* vtx, int64_t n_vtx, const int32_t* vt, int64_t n_loops, uint32_t* box) {
    if (n_vtx > 0) hl_boxes_kernel<<<tp_grid(n_vtx), TP_BLOCK, 0, s>>>(vtx, n_vtx, vt, n_loops, box);
}
void hl_launch_scatter(hipStream_t s, int64_t n_vtx, const int32_t* vt, const HlRank* rk, const int32_t* lt, int64_t n_loops, int32_t* cycle, int32_t* cloop,
                       int64_t n_room) {
    if (n_vtx > 0) hl_scatter_kernel<<<tp_grid(n_vtx), TP_BLOCK, 0, s>>>(n_vtx, vt, rk, lt, n_loops, cycle, cloop, n_room);
}
void hl_launch_limits(hipStream_t s, int64_t n_loops, int32_t* lt, const uint32_t* box, int64_t max_edges, double max_diagonal, int64_t* cstart64,
                      unsigned long long* cnt) {
    if (n_loops > 0) hl_limits_kernel<<<tp_grid(n_loops), TP_BLOCK, 0, s>>>(n_loops, lt, box, max_edges, max_diagonal, cstart64, cnt);
}
void hl_launch_chords(hipStream_t s, int64_t n_room, const unsigned long long* cnt, const int32_t* cycle, const int32_t* cloop, const unsigned long long* key,
                      int64_t n_half, int32_t* lt, int64_t n_loops) {
    if (n_room > 0) hl_chords_kernel<<<tp_grid(n_room), TP_BLOCK, 0, s>>>(n_room, cnt, cycle, cloop, key, n_half, lt, n_loops);
}
void hl_launch_decide(hipStream_t s, int64_t n_loops, int32_t* lt, unsigned long long* cnt) {
    if (n_loops > 0) hl_decide_kernel<<<tp_grid(n_loops), TP_BLOCK, 0, s>>>(n_loops, lt, cnt);
}
void hl_launch_emit(hipStream_t s, int64_t n_room, const int32_t* cycle, const int32_t* cloop, const int32_t* lt, int64_t n_loops, int32_t* new_faces,
                    int32_t* new_loop, unsigned long long* cnt) {
    if (n_room > 0 && n_loops > 0) hl_emit_kernel<<<tp_grid(n_room), TP_BLOCK, 0, s>>>(n_room, cycle, cloop, lt, n_loops, new_faces, new_loop, cnt);
}
