// Mesh topology for gfx950 (include/immesh_topology.h has the exact contract these kernels implement).
//   mark       one lane per face: counting or not, its own parent, its vertices marked as used
//   emit       one lane per counting face: its three half-edges, key (min << 32) | max, value 3 f + k, compacted by the prefix sum of the marks
//   classify   one lane per SORTED half-edge.  A run head (key differs from its predecessor's) looks at positions i + 1 and i + 2 and knows 1 / 2 / >= 3
//              uses: no lane walks a run.  Every other lane joins its face to its predecessor's face; a boundary head joins its two vertices in the
//              second union-find.  Counts: a ballot per wavefront, one atomic per wavefront and counter.
//   union-find parent[x] <= x at all times, so a root is its class's smallest member and the label needs no pass of its own.  The larger root is
//              hooked under the smaller by atomicCAS.  Inside the launch every read of a parent is an agent-scope relaxed atomic load and every write
//              an atomic: a plain load may keep returning a stale line of another XCD's L2 for the rest of the kernel, and a retry fed by it would
//              spin.  Progress after a lost CAS comes from the value the CAS returned.  Every step moves to a strictly smaller index, so a union
//              of a and b ends within a + b steps; the loop gives up at twice that and raises cnt[TP_ERROR].
//   flatten    a launch of its own: label[f] = the root (the parents no longer change, plain loads)
//   components dense numbers from the prefix sum of the root flags; face counts by integer atomics, boxes by atomicMin / atomicMax on order-preserving
//              keys, folded per wavefront and component first: one atomic per word
//   boundary   the boundary heads once more, now that the components are numbered: boundary edges per component, edges per loop
// All of it integers and min / max: the results do not depend on the order of anything.
#include "topology.hpp"
#include "topology_dev.hpp"   // the union-find and the ballot counts (the orientation's and the holes' kernels use them too), and with it raycast/pass_dev.hpp

namespace {

// ---- analyse ------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(TP_BLOCK) tp_mark_kernel(const int32_t* __restrict__ faces, int64_t n_faces, int64_t n_vtx, int32_t* __restrict__ flag,
                                                           int32_t* __restrict__ parent, int32_t* used) {
    const int64_t f = (int64_t)blockIdx.x * TP_BLOCK + threadIdx.x;
    if (f >= n_faces) return;
    const int64_t a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    // (both build calls give indices in range; a face with one out of range would not count, so that nothing below indexes outside its arrays)
    const bool ok = pd_counts(a, b, c, n_vtx);
    flag[f] = ok ? 1 : 0;
    parent[f] = (int32_t)f;
    if (ok) { used[a] = 1; used[b] = 1; used[c] = 1; }
}

__global__ void __launch_bounds__(TP_BLOCK) tp_vertices_kernel(int64_t n_vtx, const int32_t* __restrict__ used, int32_t* __restrict__ vparent,
                                                               int32_t* __restrict__ loop_cnt, unsigned long long* cnt) {
    const int64_t v = (int64_t)blockIdx.x * TP_BLOCK + threadIdx.x;
    const bool in = v < n_vtx;
    if (in) { vparent[v] = (int32_t)v; loop_cnt[v] = 0; }
    tp_count(in && used[v] != 0, cnt + TP_N_VERTICES);
}

__global__ void __launch_bounds__(TP_BLOCK) tp_emit_kernel(const int32_t* __restrict__ faces, int64_t n_faces, const int32_t* __restrict__ flag,
                                                           const int32_t* __restrict__ off, unsigned long long* __restrict__ key, int32_t* __restrict__ val) {
    const int64_t f = (int64_t)blockIdx.x * TP_BLOCK + threadIdx.x;
    if (f >= n_faces || !flag[f]) return;
    const int64_t j = 3 * (int64_t)off[f];
    const uint32_t id[3] = {(uint32_t)faces[3 * f], (uint32_t)faces[3 * f + 1], (uint32_t)faces[3 * f + 2]};
    for (int k = 0; k < 3; k++) {
        const uint32_t a = id[k], b = id[k == 2 ? 0 : k + 1];
        key[j + k] = ((unsigned long long)(a < b ? a : b) << 32) | (unsigned long long)(a < b ? b : a);
        val[j + k] = (int32_t)(3 * f + k);
    }
}

__global__ void __launch_bounds__(TP_BLOCK) tp_classify_kernel(const unsigned long long* __restrict__ key, const int32_t* __restrict__ val, int64_t n_half,
                                                               const int32_t* __restrict__ faces, int32_t* parent, int32_t* vparent, unsigned long long* cnt) {
    const int64_t i = (int64_t)blockIdx.x * TP_BLOCK + threadIdx.x;
    const bool in = i < n_half;
    unsigned long long k = 0;
    bool head = false, same1 = false, same2 = false, inconsistent = false;
    if (in) {
        k = key[i];
        head = i == 0 || key[i - 1] != k;
        if (head) {
            same1 = i + 1 < n_half && key[i + 1] == k;
            same2 = same1 && i + 2 < n_half && key[i + 2] == k;
            if (same1 && !same2) inconsistent = tp_forward(faces, val[i]) == tp_forward(faces, val[i + 1]);
        }
    }
    tp_count(head, cnt + TP_N_EDGES);
    tp_count(head && !same1, cnt + TP_N_BOUNDARY);
    tp_count(head && same1 && !same2, cnt + TP_N_INTERIOR);
    tp_count(head && same2, cnt + TP_N_NONMANIFOLD);
    tp_count(inconsistent, cnt + TP_N_INCONSISTENT);
    if (!in) return;
    bool ok = true;
    if (!head) ok = tp_union(parent, val[i] / 3, val[i - 1] / 3);
    else if (!same1) ok = tp_union(vparent, (int32_t)(k >> 32), (int32_t)(k & 0xFFFFFFFFull));
    if (!ok) atomicMax(cnt + TP_ERROR, 1ull);
}

__global__ void __launch_bounds__(TP_BLOCK) tp_flatten_kernel(const int32_t* __restrict__ parent, const int32_t* __restrict__ flag, int64_t n_faces,
                                                              int32_t* __restrict__ label, int32_t* __restrict__ root) {
    const int64_t f = (int64_t)blockIdx.x * TP_BLOCK + threadIdx.x;
    if (f >= n_faces) return;
    int32_t x = -1;
    if (flag[f]) {
        x = (int32_t)f;
        for (int32_t p = parent[x]; p != x; p = parent[x]) x = p;   // strictly downwards: it ends
    }
    label[f] = x;
    root[f] = x == (int32_t)f ? 1 : 0;
}

__global__ void __launch_bounds__(TP_BLOCK) tp_preset_kernel(int64_t n_bound, int32_t* __restrict__ nfaces, int32_t* __restrict__ nbound, uint32_t* __restrict__ box) {
    const int64_t c = (int64_t)blockIdx.x * TP_BLOCK + threadIdx.x;
    if (c >= n_bound) return;
    nfaces[c] = 0;
    nbound[c] = 0;
    for (int j = 0; j < 3; j++) { box[6 * c + j] = TP_KEY_NONE_LO; box[6 * c + 3 + j] = TP_KEY_NONE_HI; }
}

__global__ void __launch_bounds__(TP_BLOCK) tp_components_kernel(const float* __restrict__ vtx, const int32_t* __restrict__ faces, int64_t n_faces,
                                                                 const int32_t* __restrict__ label, const int32_t* __restrict__ root,
                                                                 const int32_t* __restrict__ num, int32_t* __restrict__ comp, int32_t* __restrict__ first,
                                                                 int32_t* nfaces, uint32_t* box, unsigned long long* cnt) {
    const int64_t f = (int64_t)blockIdx.x * TP_BLOCK + threadIdx.x;
    int32_t c = -1;
    uint32_t lo[3] = {TP_KEY_NONE_LO, TP_KEY_NONE_LO, TP_KEY_NONE_LO}, hi[3] = {TP_KEY_NONE_HI, TP_KEY_NONE_HI, TP_KEY_NONE_HI};
    if (f < n_faces) {
        const int32_t l = label[f];
        if (l >= 0) {
            c = num[l];
            if (root[f]) first[c] = (int32_t)f;
            for (int k = 0; k < 3; k++) {
                const float* v = vtx + 3 * (int64_t)faces[3 * f + k];   // (a counting face: its indices are in range)
                for (int j = 0; j < 3; j++) {
                    const float x = v[j];
                    if (isfinite(x)) {
                        const uint32_t q = pd_key(x);
                        lo[j] = q < lo[j] ? q : lo[j];
                        hi[j] = q > hi[j] ? q : hi[j];
                    }
                }
            }
        }
        comp[f] = c;
        if (f == n_faces - 1) cnt[TP_N_COMPONENTS] = (unsigned long long)((int64_t)num[f] + root[f]);
    }
    // One atomic per word, wavefront and component: the wavefront's faces are folded component by component (every lane takes part in the shuffles,
    // lanes of other components with the presets, which change no minimum or maximum).  A sheet's 64 faces are one round whatever the face order; a
    // million single atomics on the sheet's seven words took 32 ms.  After TP_FOLD_ROUNDS rounds the lanes left over (a
    // wavefront of many small fragments) send their own: those words are not contended.
    unsigned long long todo = __ballot(c >= 0);
    for (int round = 0; todo != 0 && round < TP_FOLD_ROUNDS; round++) {
        const int leader = __ffsll((long long)todo) - 1;
        const int32_t c0 = __shfl(c, leader, 64);
        const bool mine = c == c0;
        const unsigned long long m = __ballot(mine);
        uint32_t l[3], h[3];
        for (int j = 0; j < 3; j++) {
            l[j] = pd_wave_min(mine ? lo[j] : TP_KEY_NONE_LO);
            h[j] = pd_wave_max(mine ? hi[j] : TP_KEY_NONE_HI);
        }
        if ((int)(threadIdx.x & 63) == leader) {
            atomicAdd(nfaces + c0, (int32_t)__popcll(m));
            for (int j = 0; j < 3; j++) {
                if (l[j] != TP_KEY_NONE_LO) atomicMin(box + 6 * (int64_t)c0 + j, l[j]);
                if (h[j] != TP_KEY_NONE_HI) atomicMax(box + 6 * (int64_t)c0 + 3 + j, h[j]);
            }
        }
        todo &= ~m;
    }
    if ((todo >> (threadIdx.x & 63)) & 1ull) {
        atomicAdd(nfaces + c, 1);
        for (int j = 0; j < 3; j++) {
            if (lo[j] != TP_KEY_NONE_LO) atomicMin(box + 6 * (int64_t)c + j, lo[j]);
            if (hi[j] != TP_KEY_NONE_HI) atomicMax(box + 6 * (int64_t)c + 3 + j, hi[j]);
        }
    }
}

__global__ void __launch_bounds__(TP_BLOCK) tp_boundary_kernel(const unsigned long long* __restrict__ key, const int32_t* __restrict__ val, int64_t n_half,
                                                               const int32_t* __restrict__ comp, const int32_t* __restrict__ vparent, int32_t* nbound,
                                                               int32_t* loop_cnt, unsigned long long* cnt) {
    const int64_t i = (int64_t)blockIdx.x * TP_BLOCK + threadIdx.x;
    bool opened = false;
    uint32_t edges = 0;
    if (i < n_half) {
        const unsigned long long k = key[i];
        if ((i == 0 || key[i - 1] != k) && !(i + 1 < n_half && key[i + 1] == k)) {
            atomicAdd(nbound + comp[val[i] / 3], 1);
            int32_t x = (int32_t)(k >> 32);
            for (int32_t p = vparent[x]; p != x; p = vparent[x]) x = p;
            const int32_t before = atomicAdd(loop_cnt + x, 1);
            opened = before == 0;
            edges = (uint32_t)before + 1u;
        }
    }
    tp_count(opened, cnt + TP_N_LOOPS);
    edges = pd_wave_max(edges);                              // the largest count any lane saw is the largest loop's final count
    if ((threadIdx.x & 63) == 0 && edges) atomicMax(cnt + TP_LARGEST_LOOP, (unsigned long long)edges);
}

__global__ void __launch_bounds__(TP_BLOCK) tp_largest_kernel(const int32_t* __restrict__ root, const int32_t* __restrict__ num, const int32_t* __restrict__ nfaces,
                                                              int64_t n_faces, unsigned long long* cnt) {
    const int64_t f = (int64_t)blockIdx.x * TP_BLOCK + threadIdx.x;
    uint32_t n = 0;
    if (f < n_faces && root[f]) n = (uint32_t)nfaces[num[f]];
    n = pd_wave_max(n);
    if ((threadIdx.x & 63) == 0 && n) atomicMax(cnt + TP_LARGEST_COMPONENT, (unsigned long long)n);
}

// ---- edge lists (the run heads and run starts are pass_dev.hpp's, launched by topology_host.cpp) -----------------------------------------------
__global__ void __launch_bounds__(TP_BLOCK) tp_pick_kernel(const int32_t* __restrict__ start, int64_t n_edges, const int32_t* __restrict__ val,
                                                           const int32_t* __restrict__ faces, int32_t kind, int32_t* __restrict__ pick) {
    const int64_t e = (int64_t)blockIdx.x * TP_BLOCK + threadIdx.x;
    if (e >= n_edges) return;
    const int32_t at = start[e], u = start[e + 1] - at;
    bool is;
    if (kind == 0) is = u == 1;
    else if (kind == 1) is = u >= 3;
    else is = u == 2 && tp_forward(faces, val[at]) == tp_forward(faces, val[at + 1]);
    pick[e] = is ? 1 : 0;
}

__global__ void __launch_bounds__(TP_BLOCK) tp_edges_kernel(const int32_t* __restrict__ start, int64_t n_edges, const unsigned long long* __restrict__ key,
                                                            const int32_t* __restrict__ pick, const int32_t* __restrict__ off, int32_t* __restrict__ uv,
                                                            int32_t* __restrict__ uses) {
    const int64_t e = (int64_t)blockIdx.x * TP_BLOCK + threadIdx.x;
    if (e >= n_edges || !pick[e]) return;
    const int64_t j = off[e];
    const unsigned long long k = key[start[e]];
    uv[2 * j] = (int32_t)(k >> 32);
    uv[2 * j + 1] = (int32_t)(k & 0xFFFFFFFFull);
    uses[j] = start[e + 1] - start[e];
}

// ---- select -----------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(TP_BLOCK) tp_rank_keys_kernel(const int32_t* __restrict__ nfaces, int64_t n_comp, unsigned long long* __restrict__ rank_key,
                                                                int32_t* __restrict__ iota) {
    const int64_t c = (int64_t)blockIdx.x * TP_BLOCK + threadIdx.x;
    if (c >= n_comp) return;
    rank_key[c] = ((unsigned long long)(0x7FFFFFFF - nfaces[c]) << 32) | (unsigned long long)c;   // most faces first, then the smaller label (= number)
    iota[c] = (int32_t)c;
}

__global__ void __launch_bounds__(TP_BLOCK) tp_decide_kernel(const int32_t* __restrict__ nfaces, const uint32_t* __restrict__ box, int64_t n_comp,
                                                             int64_t min_faces, double min_diagonal, int64_t keep_largest, const int32_t* __restrict__ sorted,
                                                             int32_t* __restrict__ keepc) {
    const int64_t i = (int64_t)blockIdx.x * TP_BLOCK + threadIdx.x;
    if (i >= n_comp) return;
    const int64_t c = sorted ? sorted[i] : i;
    bool keep = (int64_t)nfaces[c] >= min_faces && (keep_largest == 0 || i < keep_largest);
    if (min_diagonal > 0.0) {
        double d[3];
        bool have = true;
        for (int j = 0; j < 3; j++) {
            const uint32_t lo = box[6 * c + j], hi = box[6 * c + 3 + j];
            have = have && lo != TP_KEY_NONE_LO && hi != TP_KEY_NONE_HI;
            d[j] = (double)pd_unkey(hi) - (double)pd_unkey(lo);
        }
        keep = keep && have && (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2] >= min_diagonal * min_diagonal;
    }
    keepc[c] = keep ? 1 : 0;
}

__global__ void __launch_bounds__(TP_BLOCK) tp_mask_kernel(const int32_t* __restrict__ comp, const int32_t* __restrict__ keepc, int64_t n_faces,
                                                           int32_t* __restrict__ keep32, int8_t* __restrict__ keep8) {
    const int64_t f = (int64_t)blockIdx.x * TP_BLOCK + threadIdx.x;
    if (f >= n_faces) return;
    const int32_t c = comp[f];
    const int32_t k = c >= 0 ? keepc[c] : 0;
    keep32[f] = k;
    keep8[f] = (int8_t)k;
}

__global__ void __launch_bounds__(TP_BLOCK) tp_compact_kernel(const int32_t* __restrict__ faces, const int32_t* __restrict__ keep32, const int32_t* __restrict__ off,
                                                              int64_t n_faces, int32_t* __restrict__ faces_out, unsigned long long* cnt) {
    const int64_t f = (int64_t)blockIdx.x * TP_BLOCK + threadIdx.x;
    if (f >= n_faces) return;
    if (keep32[f]) {
        const int64_t j = 3 * (int64_t)off[f];
        for (int k = 0; k < 3; k++) faces_out[j + k] = faces[3 * f + k];
    }
    if (f == n_faces - 1) cnt[TP_N_KEPT] = (unsigned long long)((int64_t)off[f] + keep32[f]);
}

}  // namespace

void tp_launch_mark(hipStream_t s, const int32_t* faces, int64_t n_faces, int64_t n_vtx, int32_t* flag, int32_t* parent, int32_t* used) {
    if (n_faces > 0) tp_mark_kernel<<<tp_grid(n_faces), TP_BLOCK, 0, s>>>(faces, n_faces, n_vtx, flag, parent, used);
}
void tp_launch_vertices(hipStream_t s, int64_t n_vtx, const int32_t* used, int32_t* vparent, int32_t* loop_cnt, unsigned long long* cnt) {
    if (n_vtx > 0) tp_vertices_kernel<<<tp_grid(n_vtx), TP_BLOCK, 0, s>>>(n_vtx, used, vparent, loop_cnt, cnt);
}
void tp_launch_emit(hipStream_t s, const int32_t* faces, int64_t n_faces, const int32_t* flag, const int32_t* off, unsigned long long* key, int32_t* val) {
    if (n_faces > 0) tp_emit_kernel<<<tp_grid(n_faces), TP_BLOCK, 0, s>>>(faces, n_faces, flag, off, key, val);
}
void tp_launch_classify(hipStream_t s, const unsigned long long* key, const int32_t* val, int64_t n_half, const int32_t* faces, int32_t* parent,
                        int32_t* vparent, unsigned long long* cnt) {
    if (n_half > 0) tp_classify_kernel<<<tp_grid(n_half), TP_BLOCK, 0, s>>>(key, val, n_half, faces, parent, vparent, cnt);
}
void tp_launch_flatten(hipStream_t s, const int32_t* parent, const int32_t* flag, int64_t n_faces, int32_t* label, int32_t* root) {
    if (n_faces > 0) tp_flatten_kernel<<<tp_grid(n_faces), TP_BLOCK, 0, s>>>(parent, flag, n_faces, label, root);
}
void tp_launch_preset(hipStream_t s, int64_t n_bound, int32_t* nfaces, int32_t* nbound, uint32_t* box) {
    if (n_bound > 0) tp_preset_kernel<<<tp_grid(n_bound), TP_BLOCK, 0, s>>>(n_bound, nfaces, nbound, box);
}
void tp_launch_components(hipStream_t s, const float* vtx, int64_t n_vtx, const int32_t* faces, int64_t n_faces, const int32_t* label, const int32_t* root,
                          const int32_t* num, int32_t* comp, int32_t* first, int32_t* nfaces, uint32_t* box, unsigned long long* cnt) {
    (void)n_vtx;
    if (n_faces > 0) tp_components_kernel<<<tp_grid(n_faces), TP_BLOCK, 0, s>>>(vtx, faces, n_faces, label, root, num, comp, first, nfaces, box, cnt);
}
void tp_launch_boundary(hipStream_t s, const unsigned long long* key, const int32_t* val, int64_t n_half, const int32_t* comp, const int32_t* vparent,
                        int32_t* nbound, int32_t* loop_cnt, unsigned long long* cnt) {
    if (n_half > 0) tp_boundary_kernel<<<tp_grid(n_half), TP_BLOCK, 0, s>>>(key, val, n_half, comp, vparent, nbound, loop_cnt, cnt);
}
void tp_launch_largest(hipStream_t s, const int32_t* root, const int32_t* num, const int32_t* nfaces, int64_t n_faces, unsigned long long* cnt) {
    if (n_faces > 0) tp_largest_kernel<<<tp_grid(n_faces), TP_BLOCK, 0, s>>>(root, num, nfaces, n_faces, cnt);
}

void tp_launch_pick(hipStream_t s, const int32_t* start, int64_t n_edges, const int32_t* val, const int32_t* faces, int32_t kind, int32_t* pick) {
    if (n_edges > 0) tp_pick_kernel<<<tp_grid(n_edges), TP_BLOCK, 0, s>>>(start, n_edges, val, faces, kind, pick);
}
void tp_launch_edges(hipStream_t s, const int32_t* start, int64_t n_edges, const unsigned long long* key, const int32_t* pick, const int32_t* off,
                     int32_t* uv, int32_t* uses) {
    if (n_edges > 0) tp_edges_kernel<<<tp_grid(n_edges), TP_BLOCK, 0, s>>>(start, n_edges, key, pick, off, uv, uses);
}

void tp_launch_rank_keys(hipStream_t s, const int32_t* nfaces, int64_t n_comp, unsigned long long* rank_key, int32_t* iota) {
    if (n_comp > 0) tp_rank_keys_kernel<<<tp_grid(n_comp), TP_BLOCK, 0, s>>>(nfaces, n_comp, rank_key, iota);
}
void tp_launch_decide(hipStream_t s, const int32_t* nfaces, const uint32_t* box, int64_t n_comp, int64_t min_faces, double min_diagonal,
                      int64_t keep_largest, const int32_t* sorted, int32_t* keepc) {
    if (n_comp > 0) tp_decide_kernel<<<tp_grid(n_comp), TP_BLOCK, 0, s>>>(nfaces, box, n_comp, min_faces, min_diagonal, keep_largest, sorted, keepc);
}
void tp_launch_mask(hipStream_t s, const int32_t* comp, const int32_t* keepc, int64_t n_faces, int32_t* keep32, int8_t* keep8) {
    if (n_faces > 0) tp_mask_kernel<<<tp_grid(n_faces), TP_BLOCK, 0, s>>>(comp, keepc, n_faces, keep32, keep8);
}
void tp_launch_compact(hipStream_t s, const int32_t* faces, const int32_t* keep32, const int32_t* off, int64_t n_faces, int32_t* faces_out,
                       unsigned long long* cnt) {
    if (n_faces > 0) tp_compact_kernel<<<tp_grid(n_faces), TP_BLOCK, 0, s>>>(faces, keep32, off, n_faces, faces_out, cnt);
}
