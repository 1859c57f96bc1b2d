// Self-intersections of the caster's snapshot for gfx950 (include/immesh_intersect.h has the exact contract these kernels implement).
//   candidates  one lane per face walks the caster's hierarchy with its own float box against the two child boxes of each node: float comparisons
//               only, a per-lane stack in private memory (depth bound: raycast.hpp), the second child pushed.  A leaf's box in its parent is the
//               face's float box exactly (the refit stores it), so a leaf reached is a pair whose boxes overlap; the lane counts it when j > i and j
//               takes part.  Count launch, scan, emit launch: the emit repeats the walk and writes into the face's own slot range.  No lane waits
//               on another.
//   tests       one lane per candidate, no divergence but the three cases of sh: the contract's Segment rule in its order with rc_cross / rc_dot;
//               flag, scan and compaction of the hits, the sort of the hits' keys (sort.o), then i, j, mask and n_partners per sorted hit.
//               One lane per pair and not six, one per segment: measured, DESIGN.md section 24 has the two numbers
// Double arithmetic is written in the contract's order; the library builds with -ffp-contract=off, so nothing is fused.
#include "intersect.hpp"
#include "../raycast/raycast_dev.hpp"
#include "../raycast/pass_dev.hpp"   // the folds of the counters (64 bits: a lane of the walk counts up to n_faces candidates), the rule "a face counts"

namespace {

__global__ void __launch_bounds__(RC_BLOCK) ix_take_kernel(const float* __restrict__ vtx, int64_t n_vtx, const int32_t* __restrict__ faces, int64_t n_faces,
                                                           int8_t* __restrict__ take, unsigned long long* cnt) {
    __shared__ unsigned long long lds[RC_BLOCK / 64];
    const int64_t f = (int64_t)blockIdx.x * RC_BLOCK + threadIdx.x;
    bool ok = false;
    if (f < n_faces) {
        const int64_t a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
        // (an index out of range or a vertex that is not finite is the hierarchy's mark: such a face is not in the tree)
        ok = pd_counts(a, b, c, n_vtx) && pd_finite3(vtx, a) && pd_finite3(vtx, b) && pd_finite3(vtx, c);
        take[f] = ok ? 1 : 0;
    }
    pd_block_add<unsigned long long>(ok ? 1ull : 0ull, cnt + IX_N_TAKING, lds);
}

// closed overlap of two float boxes on all three axes
__device__ __forceinline__ bool ix_overlap(const float* lo, const float* hi, const float* blo, const float* bhi) {
    return lo[0] <= bhi[0] && blo[0] <= hi[0] && lo[1] <= bhi[1] && blo[1] <= hi[1] && lo[2] <= bhi[2] && blo[2] <= hi[2];
}

// EMIT: keys[off[i] + k] = (i << 32) | j; else cnt32[i] and the total
template <bool EMIT>
__global__ void __launch_bounds__(RC_BLOCK) ix_walk_kernel(const float* __restrict__ vtx, const int32_t* __restrict__ faces, int64_t n_faces,
                                                           const int8_t* __restrict__ take, const RcNode* __restrict__ nodes, int64_t n_in,
                                                           int32_t* __restrict__ cnt32, const int32_t* __restrict__ off,
                                                           unsigned long long* __restrict__ keys, unsigned long long* cnt) {
    __shared__ unsigned long long lds[RC_BLOCK / 64];
    const int64_t i = (int64_t)blockIdx.x * RC_BLOCK + threadIdx.x;
    unsigned long long k = 0;
    if (i < n_faces && n_in > 0 && take[i]) {
        float lo[3], hi[3];
        for (int c = 0; c < 3; c++) {
            const float* v = vtx + 3 * (int64_t)faces[3 * i + c];
            for (int j = 0; j < 3; j++) {
                lo[j] = c ? fminf(lo[j], v[j]) : v[j];
                hi[j] = c ? fmaxf(hi[j], v[j]) : v[j];
            }
        }
        const int64_t base = EMIT ? (int64_t)off[i] : 0;
        int32_t stack[RC_STACK];
        int sp = 0;
        int32_t cur = 0;
        for (;;) {
            if (cur < 0) {   // a leaf whose box overlaps: the single-leaf tree's doubled child is i itself
                const int64_t j = ~cur;
                if (j > i && take[j]) {
                    if (EMIT) keys[base + (int64_t)k] = ((unsigned long long)i << 32) | (unsigned long long)j;
                    k++;
                }
            } else {
                const RcNode& nd = nodes[cur];
                const bool h0 = ix_overlap(lo, hi, nd.lo[0], nd.hi[0]), h1 = ix_overlap(lo, hi, nd.lo[1], nd.hi[1]);
                const int32_t c0 = nd.child[0], c1 = nd.child[1];
                if (h0 && h1) { stack[sp++] = c1; cur = c0; continue; }
                if (h0 || h1) { cur = h0 ? c0 : c1; continue; }
            }
            if (sp == 0) break;
            cur = stack[--sp];
        }
    }
    if (!EMIT) {
        if (i < n_faces) cnt32[i] = k > 0x7FFFFFFFull ? 0x7FFFFFFF : (int32_t)k;   // (a total with such a face is refused before the offsets are read)
        pd_block_add<unsigned long long>(k, cnt + IX_N_CANDIDATES, lds);
    }
}

// the contract's Segment rule: the segment p -> q against the face (t0, t1, t2), all floats widened to double
__device__ __forceinline__ bool ix_hit(const float* p, const float* q, const float (*T)[3]) {
    double o[3], d[3], A[3][3];
    for (int k = 0; k < 3; k++) {
        o[k] = (double)p[k];
        d[k] = (double)q[k] - (double)p[k];
    }
    for (int c = 0; c < 3; c++)
        for (int k = 0; k < 3; k++) A[c][k] = (double)T[c][k] - o[k];
    double ab[3], bc[3], ca[3], n[3];
    rc_cross(A[0], A[1], ab);
    rc_cross(A[1], A[2], bc);
    rc_cross(A[2], A[0], ca);
    const double e0 = rc_dot(ab, d), e1 = rc_dot(bc, d), e2 = rc_dot(ca, d);
    if (!((e0 >= 0.0 && e1 >= 0.0 && e2 >= 0.0) || (e0 <= 0.0 && e1 <= 0.0 && e2 <= 0.0))) return false;
    const double u[3] = {A[1][0] - A[0][0], A[1][1] - A[0][1], A[1][2] - A[0][2]};
    const double w[3] = {A[2][0] - A[0][0], A[2][1] - A[0][1], A[2][2] - A[0][2]};
    rc_cross(u, w, n);
    const double na = rc_dot(n, A[0]);
    const double nd = rc_dot(n, d);
    if (nd == 0.0) return false;
    const double s = na / nd;
    return s >= 0.0 && s <= 1.0;
}

__global__ void __launch_bounds__(RC_BLOCK) ix_test_kernel(const float* __restrict__ vtx, const int32_t* __restrict__ faces,
                                                           const unsigned long long* __restrict__ keys, int64_t n_cand, uint8_t* __restrict__ cmask,
                                                           int32_t* __restrict__ flag, unsigned long long* cnt) {
    __shared__ unsigned int s_cnt[8];
    if (threadIdx.x < 8) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const int64_t c = (int64_t)blockIdx.x * RC_BLOCK + threadIdx.x;
    if (c < n_cand) {
        const unsigned long long key = keys[c];
        const int64_t fi = (int64_t)(key >> 32), fj = (int64_t)(key & 0xFFFFFFFFull);
        int32_t ia[3], ib[3];
        float A[3][3], B[3][3];
        for (int k = 0; k < 3; k++) {
            ia[k] = faces[3 * fi + k];
            ib[k] = faces[3 * fj + k];
            for (int j = 0; j < 3; j++) {
                A[k][j] = vtx[3 * (int64_t)ia[k] + j];
                B[k][j] = vtx[3 * (int64_t)ib[k] + j];
            }
        }
        int sh = 0, ka = 0, kb = 0;                   // the faces count: an index of A equals at most one of B
        for (int a = 0; a < 3; a++)
            for (int b = 0; b < 3; b++)
                if (ia[a] == ib[b]) { sh++; ka = a; kb = b; }
        unsigned m = 0;
        if (sh == 0) {
            for (int k = 0; k < 3; k++) {
                if (ix_hit(A[k], A[(k + 1) % 3], B)) m |= 1u << k;
                if (ix_hit(B[k], B[(k + 1) % 3], A)) m |= 8u << k;
            }
        } else if (sh == 1) {                         // the edge opposite the shared vertex: it starts at the next corner
            const int ea = (ka + 1) % 3, eb = (kb + 1) % 3;
            if (ix_hit(A[ea], A[(ea + 1) % 3], B)) m |= 1u << ea;
            if (ix_hit(B[eb], B[(eb + 1) % 3], A)) m |= 8u << eb;
        }
        cmask[c] = (uint8_t)m;
        flag[c] = m ? 1 : 0;
        atomicAdd(&s_cnt[sh], 1u);
        if (m) {
            atomicAdd(&s_cnt[4], 1u);
            if (sh < 2) atomicAdd(&s_cnt[5 + sh], 1u);
        }
    }
    __syncthreads();
    if (threadIdx.x < 7 && s_cnt[threadIdx.x]) {
        const int dst = threadIdx.x < 4 ? IX_N_SHARE0 + (int)threadIdx.x : (threadIdx.x == 4 ? IX_N_PAIRS : IX_N_PAIRS_SHARE0 + (int)threadIdx.x - 5);
        atomicAdd(cnt + dst, (unsigned long long)s_cnt[threadIdx.x]);
    }
}

__global__ void __launch_bounds__(RC_BLOCK) ix_compact_kernel(const unsigned long long* __restrict__ keys, const uint8_t* __restrict__ cmask,
                                                              const int32_t* __restrict__ flag, const int32_t* __restrict__ hoff, int64_t n_cand, int bits,
                                                              unsigned long long* __restrict__ hkey, int32_t* __restrict__ hval) {
    const int64_t c = (int64_t)blockIdx.x * RC_BLOCK + threadIdx.x;
    if (c >= n_cand || !flag[c]) return;
    const unsigned long long key = keys[c];
    const int64_t h = hoff[c];
    hkey[h] = ((key >> 32) << bits) | (key & 0xFFFFFFFFull);
    hval[h] = (int32_t)cmask[c];
}

__global__ void __launch_bounds__(RC_BLOCK) ix_pairs_kernel(const unsigned long long* __restrict__ hkey, const int32_t* __restrict__ hval, int64_t n_hits,
                                                            int bits, int32_t* __restrict__ pairs, uint8_t* __restrict__ pmask, int32_t* npart) {
    const int64_t h = (int64_t)blockIdx.x * RC_BLOCK + threadIdx.x;
    if (h >= n_hits) return;
    const unsigned long long key = hkey[h];
    const int32_t i = (int32_t)(key >> bits), j = (int32_t)(key & ((1ull << bits) - 1ull));
    pairs[2 * h] = i;
    pairs[2 * h + 1] = j;
    pmask[h] = (uint8_t)hval[h];
    atomicAdd(npart + i, 1);
    atomicAdd(npart + j, 1);
}

__global__ void __launch_bounds__(RC_BLOCK) ix_keep_kernel(const int32_t* __restrict__ npart, int64_t n_faces, int32_t* __restrict__ keep,
                                                           unsigned long long* cnt) {
    __shared__ unsigned long long lds[RC_BLOCK / 64];
    __shared__ uint32_t lds_max[RC_BLOCK / 64];
    const int64_t f = (int64_t)blockIdx.x * RC_BLOCK + threadIdx.x;
    int32_t p = 0;
    if (f < n_faces) {
        p = npart[f];
        keep[f] = p == 0 ? 1 : 0;
    }
    pd_block_add<unsigned long long>(p > 0 ? 1ull : 0ull, cnt + IX_N_FACES_HIT, lds);
    pd_block_max(p > 0 ? (uint32_t)p : 0u, cnt + IX_MAX_PARTNERS, lds_max);
}

__global__ void __launch_bounds__(RC_BLOCK) ix_map_kernel(const int32_t* __restrict__ faces, int64_t n_faces, const int32_t* __restrict__ keep,
                                                          const int32_t* __restrict__ koff, int32_t* __restrict__ fmap, int32_t* __restrict__ faces_out) {
    const int64_t f = (int64_t)blockIdx.x * RC_BLOCK + threadIdx.x;
    if (f >= n_faces) return;
    const bool k = keep[f] != 0;
    const int64_t g = koff[f];
    if (fmap) fmap[f] = k ? (int32_t)g : -1;
    if (faces_out && k)
        for (int c = 0; c < 3; c++) faces_out[3 * g + c] = faces[3 * f + c];
}

}  // namespace

void ix_launch_take(hipStream_t s, const float* vtx, int64_t n_vtx, const int32_t* faces, int64_t n_faces, int8_t* take, unsigned long long* cnt) {
    if (n_faces > 0) ix_take_kernel<<<rc_grid(n_faces), RC_BLOCK, 0, s>>>(vtx, n_vtx, faces, n_faces, take, cnt);
}

void ix_launch_walk(hipStream_t s, const float* vtx, const int32_t* faces, int64_t n_faces, const int8_t* take, const RcNode* nodes, int64_t n_in, int32_t* cnt32,
                    const int32_t* off, unsigned long long* keys, unsigned long long* cnt) {
    if (n_faces <= 0) return;
    if (keys) ix_walk_kernel<true><<<rc_grid(n_faces), RC_BLOCK, 0, s>>>(vtx, faces, n_faces, take, nodes, n_in, cnt32, off, keys, cnt);
    else ix_walk_kernel<false><<<rc_grid(n_faces), RC_BLOCK, 0, s>>>(vtx, faces, n_faces, take, nodes, n_in, cnt32, off, keys, cnt);
}

void ix_launch_test(hipStream_t s, const float* vtx, const int32_t* faces, const unsigned long long* keys, int64_t n_cand, uint8_t* cmask, int32_t* flag,
                    unsigned long long* cnt) {
    if (n_cand > 0) ix_test_kernel<<<rc_grid(n_cand), RC_BLOCK, 0, s>>>(vtx, faces, keys, n_cand, cmask, flag, cnt);
}

void ix_launch_compact(hipStream_t s, const unsigned long long* keys, const uint8_t* cmask, const int32_t* flag, const int32_t* hoff, int64_t n_cand, int bits,
                       unsigned long long* hkey, int32_t* hval) {
    if (n_cand > 0) ix_compact_kernel<<<rc_grid(n_cand), RC_BLOCK, 0, s>>>(keys, cmask, flag, hoff, n_cand, bits, hkey, hval);
}

void ix_launch_pairs(hipStream_t s, const unsigned long long* hkey, const int32_t* hval, int64_t n_hits, int bits, int32_t* pairs, uint8_t* pmask, int32_t* npart) {
    if (n_hits > 0) ix_pairs_kernel<<<rc_grid(n_hits), RC_BLOCK, 0, s>>>(hkey, hval, n_hits, bits, pairs, pmask, npart);
}

void ix_launch_keep(hipStream_t s, const int32_t* npart, int64_t n_faces, int32_t* keep, unsigned long long* cnt) {
    if (n_faces > 0) ix_keep_kernel<<<rc_grid(n_faces), RC_BLOCK, 0, s>>>(npart, n_faces, keep, cnt);
}

void ix_launch_map(hipStream_t s, const int32_t* faces, int64_t n_faces, const int32_t* keep, const int32_t* koff, int32_t* fmap, int32_t* faces_out) {
    if (n_faces > 0) ix_map_kernel<<<rc_grid(n_faces), RC_BLOCK, 0, s>>>(faces, n_faces, keep, koff, fmap, faces_out);
}
