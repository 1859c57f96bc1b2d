// Consistent winding per manifold patch for gfx950 (include/immesh_topology.h has the exact contract these kernels implement).
//   The orientation double cover: node 2 f + s is "face f with flip s".  For an edge with exactly two uses, users f and g, d = 1 when the two uses
//   have one direction (the faces disagree): 2 f is joined with 2 g + d and 2 f + 1 with 2 g + 1 - d, by the analysis' union-find as it is
//   (topology_dev.hpp: parent[x] <= x, agent-scope atomic loads, the step bound of DESIGN.md, section 18, with node indices below 2 n_faces).
//   A root is its class's smallest node.  The patch of f has either two classes -- the one of 2 label, and its mirror image, whose smallest node is
//   2 label + 1 because every other face of the patch has a larger index -- or, when a cycle of disagreements closes on itself, one.  So with
//   r = root(2 f): the label is r >> 1, the patch is non-orientable when root(2 f + 1) == r, and otherwise base[f] = r & 1.
//   init          one lane per node
//   link          one lane per SORTED half-edge: the head of a run of exactly two does the two unions
//   flatten       a launch of its own (the parents no longer change, plain loads): label, base, the root flags
//   patches       dense numbers from the prefix sum of the root flags; the per-patch face counts, base counts and votes by integer atomics, folded
//                 per wavefront and patch first, as tp_components_kernel does: one atomic per word
//   inconsistent  the heads of runs of two again: the inconsistent edges per patch, folded the same way
//   decide        one lane per patch: inverted or not by the mode, the final flips, the stats' counters
//   flip          one lane per face: flip_out and faces_out
// All of it integers, and the signs of one double expression per face: the results do not depend on the order of anything.
#include "topology.hpp"
#include "topology_dev.hpp"

namespace {

struct OtPoint { double x[3]; };

// Adds the lanes with p[j] to tab[j][c] for every lane with c >= 0: the wavefront's lanes are folded patch by patch with ballots, one atomic per
// word, wavefront and patch; after TP_FOLD_ROUNDS rounds the lanes left over (a wavefront of many small patches, whose words nobody contends for)
// send their own.  Every lane of the wavefront calls this.
template <int N>
__device__ __forceinline__ void ot_fold(int32_t c, const bool (&p)[N], int32_t* const (&tab)[N]) {
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(c >= 0);
    for (int round = 0; todo != 0 && round < TP_FOLD_ROUNDS; round++) {
        const int leader = __ffsll((long long)todo) - 1;
        const int32_t c0 = __shfl(c, leader, 64);
        const bool mine = c == c0;
        const unsigned long long m = __ballot(mine);
        for (int j = 0; j < N; j++) {
            const int n = __popcll(__ballot(mine && p[j]));
            if (lane == leader && n) atomicAdd(tab[j] + c0, n);
        }
        todo &= ~m;
    }
    if ((todo >> lane) & 1ull)
        for (int j = 0; j < N; j++)
            if (p[j]) atomicAdd(tab[j] + c, 1);
}

// the contract's sign of face (ia, ib, ic) about the viewpoint o: immesh_closest.h's side rule with p = o
__device__ __forceinline__ int ot_sign(const float* __restrict__ vtx, int64_t ia, int64_t ib, int64_t ic, const OtPoint& o) {
    double A[3][3];
    const int64_t id[3] = {ia, ib, ic};
    bool finite = true;
    for (int k = 0; k < 3; k++)
        for (int j = 0; j < 3; j++) {
            const float x = vtx[3 * id[k] + j];
            finite = finite && isfinite(x);
            A[k][j] = (double)x - o.x[j];
        }
    if (!finite) return 0;
    const double u[3] = {A[1][0] - A[0][0], A[1][1] - A[0][1], A[1][2] - A[0][2]};
    const double w[3] = {A[2][0] - A[0][0], A[2][1] - A[0][1], A[2][2] - A[0][2]};
    const double ma[3] = {-A[0][0], -A[0][1], -A[0][2]};
    const double n[3] = {u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]};
    const double t = (n[0] * ma[0] + n[1] * ma[1]) + n[2] * ma[2];
    return t > 0.0 ? 1 : (t < 0.0 ? -1 : 0);   // (0 for NaN)
}

__global__ void __launch_bounds__(TP_BLOCK) ot_init_kernel(int64_t n_nodes, int32_t* __restrict__ cover) {
    const int64_t i = (int64_t)blockIdx.x * TP_BLOCK + threadIdx.x;
    if (i < n_nodes) cover[i] = (int32_t)i;
}

__global__ void __launch_bounds__(TP_BLOCK) ot_link_kernel(const unsigned long long* __restrict__ key, const int32_t* __restrict__ val, int64_t n_half,
                                                           const int32_t* __restrict__ faces, int32_t* cover, unsigned long long* cnt) {
    const int64_t i = (int64_t)blockIdx.x * TP_BLOCK + threadIdx.x;
    if (i >= n_half || !tp_pair_head(key, i, n_half)) return;
    const int32_t h0 = val[i], h1 = val[i + 1];
    const int32_t f = h0 / 3, g = h1 / 3;                    // (two faces: a counting face uses three different edges)
    const int32_t d = tp_forward(faces, h0) == tp_forward(faces, h1) ? 1 : 0;
    const bool ok = tp_union(cover, 2 * f, 2 * g + d) && tp_union(cover, 2 * f + 1, 2 * g + 1 - d);
    if (!ok) atomicMax(cnt + OT_ERROR, 1ull);
}

__global__ void __launch_bounds__(TP_BLOCK) ot_flatten_kernel(const int32_t* __restrict__ cover, const int32_t* __restrict__ flag, int64_t n_faces,
                                                              int32_t* __restrict__ label, int8_t* __restrict__ base, int32_t* __restrict__ root) {
    const int64_t f = (int64_t)blockIdx.x * TP_BLOCK + threadIdx.x;
    if (f >= n_faces) return;
    int32_t l = -1;
    int8_t b = 0;
    if (flag[f]) {
        int32_t r0 = (int32_t)(2 * f), r1 = (int32_t)(2 * f + 1);
        for (int32_t p = cover[r0]; p != r0; p = cover[r0]) r0 = p;   // strictly downwards: it ends
        for (int32_t p = cover[r1]; p != r1; p = cover[r1]) r1 = p;
        l = r0 >> 1;
        b = r0 == r1 ? 2 : (int8_t)(r0 & 1);                 // 2: the patch is non-orientable
    }
    label[f] = l;
    base[f] = b;
    root[f] = l == (int32_t)f ? 1 : 0;
}

__global__ void __launch_bounds__(TP_BLOCK) ot_patches_kernel(const float* __restrict__ vtx, const int32_t* __restrict__ faces, int64_t n_faces,
                                                              const int32_t* __restrict__ label, const int8_t* __restrict__ base,
                                                              const int32_t* __restrict__ root, const int32_t* __restrict__ num, int32_t mode, OtPoint o,
                                                              int32_t* __restrict__ patch, int32_t* tab, int64_t n_bound, unsigned long long* cnt) {
    const int64_t f = (int64_t)blockIdx.x * TP_BLOCK + threadIdx.x;
    int32_t c = -1;
    bool p[4] = {false, false, false, false};                // counts, base = 1, votes +1, votes -1
    if (f < n_faces) {
        const int32_t l = label[f];
        if (l >= 0) {
            c = num[l];
            const int8_t b = base[f];
            if (root[f]) { tab[OT_FIRST * n_bound + c] = (int32_t)f; tab[OT_ORIENTABLE * n_bound + c] = b == 2 ? 0 : 1; }
            p[0] = true;
            p[1] = b == 1;
            if (mode == 2) {
                const int s = ot_sign(vtx, faces[3 * f], faces[3 * f + 1], faces[3 * f + 2], o);   // (a counting face: its indices are in range)
                const int vote = b == 1 ? -s : s;
                p[2] = vote > 0;
                p[3] = vote < 0;
            }
        }
        patch[f] = c;
        if (f == n_faces - 1) cnt[OT_N_PATCHES] = (unsigned long long)((int64_t)num[f] + root[f]);
    }
    int32_t* const t[4] = {tab + OT_NFACES * n_bound, tab + OT_NBASE1 * n_bound, tab + OT_VOTE_PLUS * n_bound, tab + OT_VOTE_MINUS * n_bound};
    ot_fold<4>(c, p, t);
}

__global__ void __launch_bounds__(TP_BLOCK) ot_inconsistent_kernel(const unsigned long long* __restrict__ key, const int32_t* __restrict__ val, int64_t n_half,
                                                                   const int32_t* __restrict__ faces, const int32_t* __restrict__ patch, int32_t* tab,
                                                                   int64_t n_bound) {
    const int64_t i = (int64_t)blockIdx.x * TP_BLOCK + threadIdx.x;
    int32_t c = -1;
    if (i < n_half && tp_pair_head(key, i, n_half) && tp_forward(faces, val[i]) == tp_forward(faces, val[i + 1])) c = patch[val[i] / 3];
    const bool p[1] = {c >= 0};
    int32_t* const t[1] = {tab + OT_NINCONSISTENT * n_bound};
    ot_fold<1>(c, p, t);
}

__global__ void __launch_bounds__(TP_BLOCK) ot_decide_kernel(int64_t n_bound, int32_t mode, int32_t* __restrict__ tab, unsigned long long* cnt) {
    const int64_t c = (int64_t)blockIdx.x * TP_BLOCK + threadIdx.x;
    const int64_t n_patches = (int64_t)cnt[OT_N_PATCHES];    // written by the patches launch before this one
    const bool in = c < n_patches && c < n_bound;
    bool orientable = false, invert = false;
    uint32_t n = 0, flipped = 0, inconsistent = 0;
    if (in) {
        orientable = tab[OT_ORIENTABLE * n_bound + c] != 0;
        n = (uint32_t)tab[OT_NFACES * n_bound + c];
        const uint32_t b1 = (uint32_t)tab[OT_NBASE1 * n_bound + c];
        if (orientable) {
            if (mode == 1) invert = 2ull * b1 > (unsigned long long)n;
            else if (mode == 2) invert = tab[OT_VOTE_MINUS * n_bound + c] > tab[OT_VOTE_PLUS * n_bound + c];
            flipped = invert ? n - b1 : b1;
        } else {
            inconsistent = (uint32_t)tab[OT_NINCONSISTENT * n_bound + c];
        }
        tab[OT_INVERT * n_bound + c] = invert ? 1 : 0;
        tab[OT_NFLIPPED * n_bound + c] = (int32_t)flipped;
    }
    // (a wavefront's sums stay below the number of faces, so they fit 32 bits)
    tp_count(in && orientable, cnt + OT_N_ORIENTABLE);
    tp_count(in && !orientable, cnt + OT_N_NONORIENTABLE);
    tp_count(invert, cnt + OT_N_INVERTED);
    const uint32_t largest = pd_wave_max(n), f_sum = pd_wave_sum(flipped), n_sum = pd_wave_sum(in && !orientable ? n : 0u), i_sum = pd_wave_sum(inconsistent);
    if ((threadIdx.x & 63) == 0) {
        if (largest) atomicMax(cnt + OT_LARGEST_PATCH, (unsigned long long)largest);
        if (f_sum) atomicAdd(cnt + OT_N_FLIPPED, (unsigned long long)f_sum);
        if (n_sum) atomicAdd(cnt + OT_N_FACES_NONORIENTABLE, (unsigned long long)n_sum);
        if (i_sum) atomicAdd(cnt + OT_INCONSISTENT_AFTER, (unsigned long long)i_sum);
    }
}

__global__ void __launch_bounds__(TP_BLOCK) ot_flip_kernel(const int32_t* __restrict__ faces, int64_t n_faces, const int32_t* __restrict__ patch,
                                                           const int8_t* __restrict__ base, const int32_t* __restrict__ tab, int64_t n_bound,
                                                           int8_t* __restrict__ flip, int32_t* __restrict__ faces_out) {
    const int64_t f = (int64_t)blockIdx.x * TP_BLOCK + threadIdx.x;
    if (f >= n_faces) return;
    const int32_t c = patch[f];
    const int8_t b = base[f];
    const bool fl = c >= 0 && b != 2 && ((int32_t)b ^ tab[OT_INVERT * n_bound + c]) != 0;
    flip[f] = fl ? 1 : 0;
    const int32_t i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
    faces_out[3 * f] = i0;
    faces_out[3 * f + 1] = fl ? i2 : i1;
    faces_out[3 * f + 2] = fl ? i1 : i2;
}

}  // namespace

void ot_launch_init(hipStream_t s, int64_t n_nodes, int32_t* cover) {
    if (n_nodes > 0) ot_init_kernel<<<tp_grid(n_nodes), TP_BLOCK, 0, s>>>(n_nodes, cover);
}
void ot_launch_link(hipStream_t s, const unsigned long long* key, const int32_t* val, int64_t n_half, const int32_t* faces, int32_t* cover,
                    unsigned long long* cnt) {
    if (n_half > 0) ot_link_kernel<<<tp_grid(n_half), TP_BLOCK, 0, s>>>(key, val, n_half, faces, cover, cnt);
}
void ot_launch_flatten(hipStream_t s, const int32_t* cover, const int32_t* flag, int64_t n_faces, int32_t* label, int8_t* base, int32_t* root) {
    if (n_faces > 0) ot_flatten_kernel<<<tp_grid(n_faces), TP_BLOCK, 0, s>>>(cover, flag, n_faces, label, base, root);
}
void ot_launch_patches(hipStream_t s, const float* vtx, const int32_t* faces, int64_t n_faces, const int32_t* label, const int8_t* base, const int32_t* root,
                       const int32_t* num, int32_t mode, const double* o, int32_t* patch, int32_t* tab, int64_t n_bound, unsigned long long* cnt) {
    OtPoint p = {{0.0, 0.0, 0.0}};
    if (o) { p.x[0] = o[0]; p.x[1] = o[1]; p.x[2] = o[2]; }
    if (n_faces > 0) ot_patches_kernel<<<tp_grid(n_faces), TP_BLOCK, 0, s>>>(vtx, faces, n_faces, label, base, root, num, mode, p, patch, tab, n_bound, cnt);
}
void ot_launch_inconsistent(hipStream_t s, const unsigned long long* key, const int32_t* val, int64_t n_half, const int32_t* faces, const int32_t* patch,
                            int32_t* tab, int64_t n_bound) {
    if (n_half > 0) ot_inconsistent_kernel<<<tp_grid(n_half), TP_BLOCK, 0, s>>>(key, val, n_half, faces, patch, tab, n_bound);
}
void ot_launch_decide(hipStream_t s, int64_t n_bound, int32_t mode, int32_t* tab, unsigned long long* cnt) {
    if (n_bound > 0) ot_decide_kernel<<<tp_grid(n_bound), TP_BLOCK, 0, s>>>(n_bound, mode, tab, cnt);
}
void ot_launch_flip(hipStream_t s, const int32_t* faces, int64_t n_faces, const int32_t* patch, const int8_t* base, const int32_t* tab, int64_t n_bound,
                    int8_t* flip, int32_t* faces_out) {
    if (n_faces > 0) ot_flip_kernel<<<tp_grid(n_faces), TP_BLOCK, 0, s>>>(faces, n_faces, patch, base, tab, n_bound, flip, faces_out);
}
