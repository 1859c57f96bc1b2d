// One vertex per fan of faces for gfx950 (include/immesh_topology.h, the Manifold rule, has the exact contract these kernels implement; DESIGN.md,
// section 27).
//   A corner is 3 f + k, vertex i_k of counting face f.  The analysis' union-find as it is (topology_dev.hpp: parent[x] <= x, agent-scope atomic
//   loads, the step bound of DESIGN.md, section 18, with node indices below 3 n_faces) runs over the corners: an edge with exactly two uses joins
//   its users' corners at its smaller vertex, and those at its larger one.  A root is its class's smallest corner, and the faces of one fan differ
//   (a counting face has one corner at a vertex), so root / 3 is the fan's label.
//   init      one lane per corner: parent, and the two per-root counts zeroed
//   link      one lane per SORTED half-edge: the head of a run of exactly two does the two unions
//   flatten   a launch of its own (the parents no longer change, plain loads): the root per corner, the root flags, n_corners per root
//   links     the heads of runs of two again: n_links per root, one integer atomic per end
//   keys      after the scan of the root flags: (vertex << 32) | corner of every root, compacted; the host reads their number and sorts them
//   fans      one lane per sorted key, which is fan j: its vertex, and j for its root corner
//   (the runs of equal vertices by pass_dev.hpp's run kernels: a run's head is the fan that keeps the vertex, and a fan that is no head is new
//   vertex j - scan[j], the fans before it that are no heads: the scan of the heads serves as the second prefix sum)
//   table     one lane per fan: the tables, vsrc, the bit copy of the new vertex, the fans' counters
//   vertices  one lane per run: n_fans_out, the vertices' counters
//   emit      one lane per face: faces_out, fan_out, the faces' counters
// All of it integers and bit copies: the results do not depend on the order of anything.  The counters go through the workgroup folds of
// pass_dev.hpp: one atomic per workgroup and counter.
#include "topology.hpp"
#include "topology_dev.hpp"

namespace {

// the corners of half-edge h at its edge's smaller and larger vertex
__device__ __forceinline__ void mf_ends(const int32_t* __restrict__ faces, int32_t h, int32_t& at_min, int32_t& at_max) {
    const int32_t f = h / 3, k = h - 3 * f;
    const int32_t a = h, b = 3 * f + (k == 2 ? 0 : k + 1);
    const bool fwd = faces[a] < faces[b];
    at_min = fwd ? a : b;
    at_max = fwd ? b : a;
}

__global__ void __launch_bounds__(TP_BLOCK) mf_init_kernel(int64_t n3, int32_t* __restrict__ parent, int32_t* __restrict__ ncnt, int32_t* __restrict__ nlnk) {
    const int64_t i = (int64_t)blockIdx.x * TP_BLOCK + threadIdx.x;
    if (i >= n3) return;
    parent[i] = (int32_t)i;
    ncnt[i] = 0;
    nlnk[i] = 0;
}

__global__ void __launch_bounds__(TP_BLOCK) mf_link_kernel(const unsigned long long* __restrict__ key, const int32_t* __restrict__ val, int64_t n_half,
                                                           const int32_t* __restrict__ faces, int32_t* parent, unsigned long long* cnt) {
    const int64_t i = (int64_t)blockIdx.x * TP_BLOCK + threadIdx.x;
    if (i >= n_half || !tp_pair_head(key, i, n_half)) return;
    int32_t lo0, hi0, lo1, hi1;
    mf_ends(faces, val[i], lo0, hi0);
    mf_ends(faces, val[i + 1], lo1, hi1);
    const bool ok = tp_union(parent, lo0, lo1) && tp_union(parent, hi0, hi1);
    if (!ok) atomicMax(cnt + MF_ERROR, 1ull);
}

__global__ void __launch_bounds__(TP_BLOCK) mf_flatten_kernel(const int32_t* __restrict__ parent, const int32_t* __restrict__ flag, int64_t n3,
                                                              int32_t* __restrict__ root, int32_t* __restrict__ isroot, int32_t* ncnt) {
    const int64_t c = (int64_t)blockIdx.x * TP_BLOCK + threadIdx.x;
    if (c >= n3) return;
    int32_t r = -1;
    if (flag[c / 3]) {
        r = (int32_t)c;
        for (int32_t p = parent[r]; p != r; p = parent[r]) r = p;   // strictly downwards: it ends
        atomicAdd(ncnt + r, 1);
    }
    root[c] = r;
    isroot[c] = r == (int32_t)c ? 1 : 0;
}

__global__ void __launch_bounds__(TP_BLOCK) mf_links_kernel(const unsigned long long* __restrict__ key, const int32_t* __restrict__ val, int64_t n_half,
                                                            const int32_t* __restrict__ faces, const int32_t* __restrict__ root, int32_t* nlnk) {
    const int64_t i = (int64_t)blockIdx.x * TP_BLOCK + threadIdx.x;
    if (i >= n_half || !tp_pair_head(key, i, n_half)) return;
    int32_t lo, hi;
    mf_ends(faces, val[i], lo, hi);                             // (a corner of a counting face: its root is one)
    atomicAdd(nlnk + root[lo], 1);
    atomicAdd(nlnk + root[hi], 1);
}

__global__ void __launch_bounds__(TP_BLOCK) mf_keys_kernel(const int32_t* __restrict__ faces, const int32_t* __restrict__ isroot, const int32_t* __restrict__ off,
                                                           int64_t n3, unsigned long long* __restrict__ key, int32_t* __restrict__ val, int64_t n_room) {
    const int64_t c = (int64_t)blockIdx.x * TP_BLOCK + threadIdx.x;
    if (c >= n3 || !isroot[c]) return;
    const int64_t j = off[c];
    if (j < 0 || j >= n_room) return;
    key[j] = ((unsigned long long)(uint32_t)faces[c] << 32) | (unsigned long long)c;
    val[j] = (int32_t)c;
}

__global__ void __launch_bounds__(TP_BLOCK) mf_fans_kernel(const unsigned long long* __restrict__ key, int64_t n_fans, int64_t n3, int32_t* __restrict__ fv,
                                                           int32_t* __restrict__ fanof) {
    const int64_t j = (int64_t)blockIdx.x * TP_BLOCK + threadIdx.x;
    if (j >= n_fans) return;
    const unsigned long long k = key[j];
    fv[j] = (int32_t)(k >> 32);
    const int64_t c = (int64_t)(k & 0xFFFFFFFFull);
    if (c < n3) fanof[c] = (int32_t)j;
}

__global__ void __launch_bounds__(TP_BLOCK) mf_table_kernel(int64_t n_fans, const unsigned long long* __restrict__ key, const int32_t* __restrict__ head,
                                                            const int32_t* __restrict__ scan, const int32_t* __restrict__ ncnt,
                                                            const int32_t* __restrict__ nlnk, const uint32_t* __restrict__ vtx, int64_t n_vtx, int64_t n_new,
                                                            int32_t* __restrict__ ft, int32_t* __restrict__ vsrc, uint32_t* __restrict__ vtx_out,
                                                            unsigned long long* cnt) {
    __shared__ uint32_t lds[TP_BLOCK / 64];
    const int64_t j = (int64_t)blockIdx.x * TP_BLOCK + threadIdx.x;
    uint32_t closed = 0, open = 0, corners = 0;
    if (j < n_fans) {
        const unsigned long long k = key[j];
        const int64_t v = (int64_t)(k >> 32), c = (int64_t)(k & 0xFFFFFFFFull);
        const int32_t nc = ncnt[c], nl = nlnk[c];
        int64_t index = v;
        if (!head[j]) {                                         // a new vertex: the bits of its source
            const int64_t m = j - scan[j];
            index = n_vtx + m;
            if (m >= 0 && m < n_new && v < n_vtx) {
                vsrc[m] = (int32_t)v;
                for (int t = 0; t < 3; t++) vtx_out[3 * index + t] = vtx[3 * v + t];
            }
        }
        ft[MT_VERTEX * n_fans + j] = (int32_t)v;
        ft[MT_FIRST * n_fans + j] = (int32_t)(c / 3);
        ft[MT_NCORNERS * n_fans + j] = nc;
        ft[MT_NLINKS * n_fans + j] = nl;
        ft[MT_INDEX * n_fans + j] = (int32_t)index;
        closed = nl == nc ? 1u : 0u;
        open = 1u - closed;
        corners = (uint32_t)nc;
    }
    pd_block_add(closed, cnt + MF_N_CLOSED, lds);
    pd_block_add(open, cnt + MF_N_OPEN, lds);
    pd_block_max(corners, cnt + MF_LARGEST_FAN, lds);
}

__global__ void __launch_bounds__(TP_BLOCK) mf_vertices_kernel(int64_t n_runs, const int32_t* __restrict__ start, const int32_t* __restrict__ fv, int64_t n_fans,
                                                               int64_t n_vtx, int32_t* __restrict__ nfans_out, unsigned long long* cnt) {
    __shared__ uint32_t lds[TP_BLOCK / 64];
    const int64_t r = (int64_t)blockIdx.x * TP_BLOCK + threadIdx.x;
    uint32_t n = 0;
    if (r < n_runs) {
        const int64_t b = start[r], e = start[r + 1];
        if (b >= 0 && b < e && e <= n_fans) {
            const int64_t v = fv[b];
            n = (uint32_t)(e - b);
            if (v >= 0 && v < n_vtx) nfans_out[v] = (int32_t)n;
        }
    }
    pd_block_add(n >= 2 ? 1u : 0u, cnt + MF_N_SINGULAR, lds);
    pd_block_max(n, cnt + MF_MOST_FANS, lds);
}

__global__ void __launch_bounds__(TP_BLOCK) mf_emit_kernel(const int32_t* __restrict__ faces, int64_t n_faces, const int32_t* __restrict__ flag,
                                                           const int32_t* __restrict__ root, const int32_t* __restrict__ fanof, const int32_t* __restrict__ ft,
                                                           int64_t n_fans, int32_t* __restrict__ faces_out, int32_t* __restrict__ fan_out,
                                                           unsigned long long* cnt) {
    __shared__ uint32_t lds[TP_BLOCK / 64];
    const int64_t f = (int64_t)blockIdx.x * TP_BLOCK + threadIdx.x;
    uint32_t moved = 0;
    if (f < n_faces) {
        const bool counts = flag[f] != 0;
        for (int k = 0; k < 3; k++) {
            const int64_t c = 3 * f + k;
            const int32_t old = faces[c];
            int32_t fan = -1, index = old;
            if (counts) {
                const int32_t r = root[c];
                const int64_t j = r >= 0 ? fanof[r] : -1;
                if (j >= 0 && j < n_fans) { fan = (int32_t)j; index = ft[MT_INDEX * n_fans + j]; }
            }
            faces_out[c] = index;
            fan_out[c] = fan;
            moved += index != old ? 1u : 0u;
        }
    }
    pd_block_add(moved, cnt + MF_N_MOVED, lds);
    pd_block_add(moved ? 1u : 0u, cnt + MF_N_CHANGED, lds);
}

}  // namespace

void mf_launch_init(hipStream_t s, int64_t n3, int32_t* parent, int32_t* ncnt, int32_t* nlnk) {
    if (n3 > 0) mf_init_kernel<<<tp_grid(n3), TP_BLOCK, 0, s>>>(n3, parent, ncnt, nlnk);
}
void mf_launch_link(hipStream_t s, const unsigned long long* key, const int32_t* val, int64_t n_half, const int32_t* faces, int32_t* parent,
                    unsigned long long* cnt) {
    if (n_half > 0) mf_link_kernel<<<tp_grid(n_half), TP_BLOCK, 0, s>>>(key, val, n_half, faces, parent, cnt);
}
void mf_launch_flatten(hipStream_t s, const int32_t* parent, const int32_t* flag, int64_t n3, int32_t* root, int32_t* isroot, int32_t* ncnt) {
    if (n3 > 0) mf_flatten_kernel<<<tp_grid(n3), TP_BLOCK, 0, s>>>(parent, flag, n3, root, isroot, ncnt);
}
void mf_launch_links(hipStream_t s, const unsigned long long* key, const int32_t* val, int64_t n_half, const int32_t* faces, const int32_t* root,
                     int32_t* nlnk) {
    if (n_half > 0) mf_links_kernel<<<tp_grid(n_half), TP_BLOCK, 0, s>>>(key, val, n_half, faces, root, nlnk);
}
void mf_launch_keys(hipStream_t s, const int32_t* faces, const int32_t* isroot, const int32_t* off, int64_t n3, unsigned long long* key, int32_t* val,
                    int64_t n_room) {
    if (n3 > 0 && n_room > 0) mf_keys_kernel<<<tp_grid(n3), TP_BLOCK, 0, s>>>(faces, isroot, off, n3, key, val, n_room);
}
void mf_launch_fans(hipStream_t s, const unsigned long long* key, int64_t n_fans, int64_t n3, int32_t* fv, int32_t* fanof) {
    if (n_fans > 0) mf_fans_kernel<<<tp_grid(n_fans), TP_BLOCK, 0, s>>>(key, n_fans, n3, fv, fanof);
}
void mf_launch_table(hipStream_t s, int64_t n_fans, const unsigned long long* key, const int32_t* head, const int32_t* scan, const int32_t* ncnt,
                     const int32_t* nlnk, const float* vtx, int64_t n_vtx, int64_t n_new, int32_t* ft, int32_t* vsrc, float* vtx_out, unsigned long long* cnt) {
    if (n_fans > 0)
        mf_table_kernel<<<tp_grid(n_fans), TP_BLOCK, 0, s>>>(n_fans, key, head, scan, ncnt, nlnk, (const uint32_t*)vtx, n_vtx, n_new, ft, vsrc, (uint32_t*)vtx_out,
                                                             cnt);
}
void mf_launch_vertices(hipStream_t s, int64_t n_runs, const int32_t* start, const int32_t* fv, int64_t n_fans, int64_t n_vtx, int32_t* nfans_out,
                        unsigned long long* cnt) {
    if (n_runs > 0) mf_vertices_kernel<<<tp_grid(n_runs), TP_BLOCK, 0, s>>>(n_runs, start, fv, n_fans, n_vtx, nfans_out, cnt);
}
void mf_launch_emit(hipStream_t s, const int32_t* faces, int64_t n_faces, const int32_t* flag, const int32_t* root, const int32_t* fanof, const int32_t* ft,
                    int64_t n_fans, int32_t* faces_out, int32_t* fan_out, unsigned long long* cnt) {
    if (n_faces > 0) mf_emit_kernel<<<tp_grid(n_faces), TP_BLOCK, 0, s>>>(faces, n_faces, flag, root, fanof, ft, n_fans, faces_out, fan_out, cnt);
}
