// Ray casting at a triangle soup for gfx950 (include/immesh_raycast.h has the exact contract these kernels implement).
//   build     of the caster's faces and of a cloud index's points alike: mark the items that enter the tree, compact them with their float boxes,
//             reduce the bounds of the box centres (order-preserving keys, atomicMin / atomicMax), 63-bit Morton codes, rocPRIM's stable radix sort (sort.o; equal codes keep face order), Karras'
//             construction (one lane per interior node), bottom-up refit (one lane per leaf, the second arrival at a node goes on)
//   cast      one ray per lane, a per-lane stack in private memory (depth bound: raycast.hpp), the nearer child first; a node is skipped only
//             by the contract's Box arithmetic on its own box, which can never cull a face that counts
//   reinforce the hit points and their cells; thinning and compaction are the renderer's launches (render.hpp)
// Double arithmetic is written in the contract's order; the library builds with -ffp-contract=off, so nothing is fused.
#include "raycast.hpp"
#include "raycast_dev.hpp"
#include "pass_dev.hpp"   // the order-preserving float keys

namespace {

// ---- build ------------------------------------------------------------------------------------------------------------------------------
// SOUP: the items are the faces of src; else the points of the cloud src.xyz
template <bool SOUP>
__global__ void __launch_bounds__(RC_BLOCK) rc_mark_kernel(RcLeaves src, int64_t n, int32_t* __restrict__ flag) {
    const int64_t f = (int64_t)blockIdx.x * RC_BLOCK + threadIdx.x;
    if (f >= n) return;
    bool ok = true;
    for (int k = 0; k < (SOUP ? 3 : 1); k++) {
        int64_t id = f;
        if (SOUP) {
            id = src.faces[3 * f + k];
            if (id < 0 || id >= src.n_vtx) { ok = false; break; }
        }
        for (int j = 0; j < 3; j++) ok = ok && isfinite(src.xyz[3 * id + j]);
    }
    flag[f] = ok ? 1 : 0;
}

template <bool SOUP>
__global__ void __launch_bounds__(RC_BLOCK) rc_compact_kernel(RcLeaves src, int64_t n, const int32_t* __restrict__ flag, const int32_t* __restrict__ off,
                                                              int32_t* __restrict__ ids, float* __restrict__ box, uint32_t* bounds, int64_t* n_in) {
    __shared__ uint32_t s_b[6];
    if (threadIdx.x < 6) s_b[threadIdx.x] = threadIdx.x < 3 ? 0xFFFFFFFFu : 0u;
    __syncthreads();
    const int64_t f = (int64_t)blockIdx.x * RC_BLOCK + threadIdx.x;
    if (f < n && flag[f]) {
        const int64_t i = off[f];
        for (int j = 0; j < 3; j++) {
            float lo, hi;
            if (SOUP) {
                const float a = src.xyz[3 * (int64_t)src.faces[3 * f] + j], b = src.xyz[3 * (int64_t)src.faces[3 * f + 1] + j],
                            c = src.xyz[3 * (int64_t)src.faces[3 * f + 2] + j];
                lo = fminf(fminf(a, b), c);
                hi = fmaxf(fmaxf(a, b), c);
            } else {
                lo = hi = src.xyz[3 * f + j];
            }
            box[6 * i + j] = lo;
            box[6 * i + 3 + j] = hi;
            const uint32_t k = pd_key(0.5f * lo + 0.5f * hi);   // the centre, as rc_codes_kernel computes it from the box; halves first, so it cannot overflow
            atomicMin(&s_b[j], k);
            atomicMax(&s_b[3 + j], k);
        }
        ids[i] = (int32_t)f;
    }
    if (f == n - 1) n_in[0] = (int64_t)off[f] + flag[f];
    __syncthreads();
    if (threadIdx.x < 3) { if (s_b[threadIdx.x] != 0xFFFFFFFFu) atomicMin(&bounds[threadIdx.x], s_b[threadIdx.x]); }
    else if (threadIdx.x < 6) { if (s_b[threadIdx.x] != 0u) atomicMax(&bounds[threadIdx.x], s_b[threadIdx.x]); }
}

__device__ __forceinline__ unsigned long long rc_spread3(unsigned long long v) {   // 21 bits -> every third bit
    v &= 0x1FFFFFull;
    v = (v | (v << 32)) & 0x1F00000000FFFFull;
    v = (v | (v << 16)) & 0x1F0000FF0000FFull;
    v = (v | (v << 8)) & 0x100F00F00F00F00Full;
    v = (v | (v << 4)) & 0x10C30C30C30C30C3ull;
    v = (v | (v << 2)) & 0x1249249249249249ull;
    return v;
}

__global__ void __launch_bounds__(RC_BLOCK) rc_codes_kernel(const float* __restrict__ box, int64_t n_in, const uint32_t* __restrict__ bounds,
                                                            unsigned long long* __restrict__ code, int32_t* __restrict__ iota) {
    const int64_t i = (int64_t)blockIdx.x * RC_BLOCK + threadIdx.x;
    if (i >= n_in) return;
    unsigned long long c = 0;
    for (int j = 0; j < 3; j++) {
        const double lo = (double)pd_unkey(bounds[j]), hi = (double)pd_unkey(bounds[3 + j]);
        const double ctr = (double)(0.5f * box[6 * i + j] + 0.5f * box[6 * i + 3 + j]);
        const double ext = hi - lo;
        double q = ext > 0.0 ? ((ctr - lo) / ext) * 2097152.0 : 0.0;       // 2^21 cells per axis
        q = fmin(fmax(q, 0.0), 2097151.0);
        c |= rc_spread3((unsigned long long)q) << j;
    }
    code[i] = c;
    iota[i] = (int32_t)i;
}

// common-prefix length of the keys (code, position) of leaves i and j; -1 outside the array
__device__ __forceinline__ int rc_delta(const unsigned long long* __restrict__ code, int64_t n, int64_t i, int64_t j) {
    if (j < 0 || j >= n) return -1;
    const unsigned long long a = code[i], b = code[j];
    if (a != b) return __clzll((long long)(a ^ b));
    return 64 + __clz((int)((uint32_t)i ^ (uint32_t)j));
}

__global__ void __launch_bounds__(RC_BLOCK) rc_hierarchy_kernel(const unsigned long long* __restrict__ code, const int32_t* __restrict__ ids,
                                                                const int32_t* __restrict__ pos_sorted, int64_t n, RcNode* __restrict__ nodes,
                                                                int32_t* __restrict__ leaf_parent) {
    const int64_t i = (int64_t)blockIdx.x * RC_BLOCK + threadIdx.x;
    if (i >= n - 1) return;
    // Karras 2012, "Maximizing parallelism in the construction of BVHs, octrees, and k-d trees": direction, range, split of interior node i
    const int dir = rc_delta(code, n, i, i + 1) - rc_delta(code, n, i, i - 1) >= 0 ? 1 : -1;
    const int dmin = rc_delta(code, n, i, i - dir);
    int64_t lmax = 2;
    while (rc_delta(code, n, i, i + lmax * dir) > dmin) lmax <<= 1;
    int64_t l = 0;
    for (int64_t t = lmax >> 1; t >= 1; t >>= 1)
        if (rc_delta(code, n, i, i + (l + t) * dir) > dmin) l += t;
    const int64_t j = i + l * dir;
    const int dnode = rc_delta(code, n, i, j);
    int64_t sp = 0;
    for (int64_t t = (l + 1) >> 1;; t = (t + 1) >> 1) {
        if (rc_delta(code, n, i, i + (sp + t) * dir) > dnode) sp += t;
        if (t == 1) break;
    }
    const int64_t gamma = i + sp * dir + (dir < 0 ? -1 : 0);
    const int64_t first = i < j ? i : j, last = i < j ? j : i;
    const int64_t kid[2] = {gamma, gamma + 1};
    const bool leaf[2] = {first == gamma, last == gamma + 1};
    for (int k = 0; k < 2; k++) {
        if (leaf[k]) {
            nodes[i].child[k] = ~ids[pos_sorted[kid[k]]];
            leaf_parent[kid[k]] = (int32_t)((i << 1) | k);
        } else {
            nodes[i].child[k] = (int32_t)kid[k];
            nodes[kid[k]].parent = (int32_t)((i << 1) | k);
        }
    }
    if (i == 0) nodes[0].parent = -1;
    nodes[i].count = 0;
}

__device__ __forceinline__ void rc_store_f(float* p, float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ float rc_load_f(float* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// One lane per leaf walks towards the root.  At a node it stores the box it brings into the node's slot for that child (agent-scope stores), then
// adds to the node's counter (acquire-release, agent scope): the first arrival stops, the second reads the other slot (agent-scope loads), unites
// the two and goes on.  A union is a min / max per coordinate, so the boxes do not depend on which lane arrived first.
__global__ void __launch_bounds__(RC_BLOCK) rc_refit_kernel(const float* __restrict__ box, const int32_t* __restrict__ pos_sorted,
                                                            const int32_t* __restrict__ leaf_parent, int64_t n, RcNode* nodes) {
    const int64_t i = (int64_t)blockIdx.x * RC_BLOCK + threadIdx.x;
    if (i >= n) return;
    float lo[3], hi[3];
    const int64_t p = pos_sorted[i];
    for (int j = 0; j < 3; j++) { lo[j] = box[6 * p + j]; hi[j] = box[6 * p + 3 + j]; }
    int32_t up = leaf_parent[i];
    for (int level = 0; level < RC_STACK && up >= 0; level++) {   // a leaf has at most RC_STACK interior ancestors
        RcNode* nd = nodes + (up >> 1);
        const int k = up & 1;
        for (int j = 0; j < 3; j++) { rc_store_f(&nd->lo[k][j], lo[j]); rc_store_f(&nd->hi[k][j], hi[j]); }
        if (__hip_atomic_fetch_add(&nd->count, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == 0) return;
        for (int j = 0; j < 3; j++) {
            lo[j] = fminf(lo[j], rc_load_f(&nd->lo[1 - k][j]));
            hi[j] = fmaxf(hi[j], rc_load_f(&nd->hi[1 - k][j]));
        }
        up = nd->parent;
    }
}

__global__ void rc_single_kernel(const float* __restrict__ box, const int32_t* __restrict__ ids, RcNode* __restrict__ nodes) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    RcNode nd;
    for (int j = 0; j < 3; j++) {
        nd.lo[0][j] = nd.lo[1][j] = box[j];
        nd.hi[0][j] = nd.hi[1][j] = box[3 + j];
    }
    nd.child[0] = nd.child[1] = ~ids[0];
    nd.parent = -1; nd.count = 2;
    nodes[0] = nd;
}

// ---- cast -------------------------------------------------------------------------------------------------------------------------------
struct RcRay {
    double o[3], d[3], inv[3];
    bool bound[3];        // the axis bounds t (d_k != 0 and 1 / d_k finite)
    bool ok;
};

__device__ __forceinline__ RcRay rc_ray(const RcFrame& fr, const float* __restrict__ dirs, const float* __restrict__ origins, int64_t i) {
    RcRay r;
    const float df[3] = {dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2]};
    r.ok = isfinite(df[0]) && isfinite(df[1]) && isfinite(df[2]) && !(df[0] == 0.0f && df[1] == 0.0f && df[2] == 0.0f);
    const double dd[3] = {(double)df[0], (double)df[1], (double)df[2]};
    for (int k = 0; k < 3; k++) r.d[k] = (fr.rot[3 * k] * dd[0] + fr.rot[3 * k + 1] * dd[1]) + fr.rot[3 * k + 2] * dd[2];
    if (origins) {
        const float of[3] = {origins[3 * i], origins[3 * i + 1], origins[3 * i + 2]};
        r.ok = r.ok && isfinite(of[0]) && isfinite(of[1]) && isfinite(of[2]);
        const double oo[3] = {(double)of[0], (double)of[1], (double)of[2]};
        for (int k = 0; k < 3; k++) r.o[k] = ((fr.rot[3 * k] * oo[0] + fr.rot[3 * k + 1] * oo[1]) + fr.rot[3 * k + 2] * oo[2]) + fr.pos[k];
    } else {
        for (int k = 0; k < 3; k++) r.o[k] = fr.pos[k];
    }
    for (int k = 0; k < 3; k++) {
        r.ok = r.ok && isfinite(r.d[k]) && isfinite(r.o[k]);
        r.inv[k] = 1.0 / r.d[k];
        r.bound[k] = r.d[k] != 0.0 && isfinite(r.inv[k]);
    }
    return r;
}

// the contract's Box arithmetic on any float box: false when an unbounded axis excludes the origin; else tn, tf
__device__ __forceinline__ bool rc_slab(const RcRay& r, const float* lo, const float* hi, double* tn, double* tf) {
    double n = -INFINITY, f = INFINITY;
    bool in = true;
    for (int k = 0; k < 3; k++) {
        const double l = (double)lo[k], h = (double)hi[k];
        if (r.bound[k]) {
            const double t1 = (l - r.o[k]) * r.inv[k], t2 = (h - r.o[k]) * r.inv[k];
            n = fmax(n, fmin(t1, t2));
            f = fmin(f, fmax(t1, t2));
        } else {
            in = in && l <= r.o[k] && r.o[k] <= h;
        }
    }
    *tn = n; *tf = f;
    return in;
}

// may a box with these tn, tf hold a face that counts?  *key = (float)(tn - g), the NEAREST bound
__device__ __forceinline__ bool rc_box_open(double tn, double tf, double g, double t_min, double t_max, float* key) {
    const double a = tn - g, b = tf + g;
    *key = (float)a;
    return !(a > b) && !(a >= t_max) && !(b < t_min);
}

__global__ void __launch_bounds__(RC_BLOCK) rc_cast_kernel(RcFrame fr, const float* __restrict__ dirs, const float* __restrict__ origins, int64_t n_rays,
                                                           double t_min, double t_max, int mode, const float* __restrict__ vtx,
                                                           const int32_t* __restrict__ faces, const RcNode* __restrict__ nodes, int64_t n_in,
                                                           float* __restrict__ t_out, int32_t* __restrict__ face_out) {
    const int64_t i = (int64_t)blockIdx.x * RC_BLOCK + threadIdx.x;
    if (i >= n_rays) return;
    const RcRay r = rc_ray(fr, dirs, origins, i);
    const double g = t_max * 0x1p-24;
    unsigned long long best = ~0ull;          // (bits(d32) << 32) | face: non-negative floats order as unsigned
    float best_t = INFINITY;
    bool any = false;
    if (r.ok && n_in > 0) {
        int32_t stack[RC_STACK];
        float stack_key[RC_STACK];
        int sp = 0;
        int32_t cur = 0;
        for (;;) {
            if (cur < 0) {   // a face
                const int32_t f = ~cur;
                float lo[3], hi[3];
                double A[3][3];
                rc_load_face(vtx, faces, f, r.o, lo, hi, A);
                double ab[3], bc[3], ca[3], n[3];
                rc_cross(A[0], A[1], ab);
                rc_cross(A[1], A[2], bc);
                rc_cross(A[2], A[0], ca);
                const double e0 = rc_dot(ab, r.d), e1 = rc_dot(bc, r.d), e2 = rc_dot(ca, r.d);
                if ((e0 >= 0.0 && e1 >= 0.0 && e2 >= 0.0) || (e0 <= 0.0 && e1 <= 0.0 && e2 <= 0.0)) {
                    const double u[3] = {A[1][0] - A[0][0], A[1][1] - A[0][1], A[1][2] - A[0][2]};
                    const double w[3] = {A[2][0] - A[0][0], A[2][1] - A[0][1], A[2][2] - A[0][2]};
                    rc_cross(u, w, n);
                    const double na = rc_dot(n, A[0]);
                    const double nd = rc_dot(n, r.d);
                    if (nd != 0.0) {
                        const double s = na / nd;
                        double tn, tf;
                        if (s >= t_min && s < t_max && rc_slab(r, lo, hi, &tn, &tf) && tn - g <= s && s <= tf + g) {
                            any = true;
                            if (mode != 0) break;
                            const float d32 = (float)s + 0.0f;   // + 0: s = -0 (the origin in the face's plane, t_min = 0) is the distance +0
                            const unsigned long long key = ((unsigned long long)__float_as_uint(d32) << 32) | (uint32_t)f;
                            if (key < best) { best = key; best_t = d32; }
                        }
                    }
                }
            } else {
                const RcNode& nd = nodes[cur];
                double tn0, tf0, tn1, tf1;
                float k0, k1;
                bool h0 = rc_slab(r, nd.lo[0], nd.hi[0], &tn0, &tf0);
                bool h1 = rc_slab(r, nd.lo[1], nd.hi[1], &tn1, &tf1);
                h0 = rc_box_open(tn0, tf0, g, t_min, t_max, &k0) && h0 && !(k0 > best_t);
                h1 = rc_box_open(tn1, tf1, g, t_min, t_max, &k1) && h1 && !(k1 > best_t);
                const int32_t c0 = nd.child[0], c1 = nd.child[1];
                if (h0 && h1) {
                    const bool first0 = k0 <= k1;       // the nearer child first: its hits prune the other
                    stack[sp] = first0 ? c1 : c0;
                    stack_key[sp] = first0 ? k1 : k0;
                    sp++;
                    cur = first0 ? c0 : c1;
                    continue;
                }
                if (h0 || h1) { cur = h0 ? c0 : c1; continue; }
            }
            // next entry whose bound can still hold the winner
            bool found = false;
            while (sp > 0) {
                sp--;
                if (!(stack_key[sp] > best_t)) { cur = stack[sp]; found = true; break; }
            }
            if (!found) break;
        }
    }
    float t = -1.0f;
    int32_t f = -1;
    if (mode != 0) {
        if (any) { t = 0.0f; f = 0; }
    } else if (best != ~0ull) {
        t = __uint_as_float((uint32_t)(best >> 32));
        f = (int32_t)(uint32_t)best;
    }
    t_out[i] = t;
    face_out[i] = f;
}

// ---- reinforce --------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(RC_BLOCK) rc_points_kernel(RcFrame fr, const float* __restrict__ dirs, const float* __restrict__ origins, int64_t n_rays,
                                                             float res, const float* __restrict__ t, float* __restrict__ pts, float* __restrict__ cells,
                                                             int32_t* __restrict__ keep) {
    const int64_t i = (int64_t)blockIdx.x * RC_BLOCK + threadIdx.x;
    if (i >= n_rays) return;
    const float d32 = t[i];
    if (!(d32 >= 0.0f)) { keep[i] = 0; return; }
    const RcRay r = rc_ray(fr, dirs, origins, i);
    const double d = (double)d32;
    for (int k = 0; k < 3; k++) {
        const float w = (float)(r.o[k] + r.d[k] * d);
        pts[3 * i + k] = w;
        if (res > 0.0f) cells[3 * i + k] = roundf(w / res) + 0.0f;   // + 0: -0 and +0 are one cell (the renderer's Thin rule)
    }
    keep[i] = res > 0.0f ? 0 : 1;
}

}  // namespace

void rc_launch_mark(hipStream_t s, const RcLeaves& src, int64_t n, int32_t* flag) {
    if (n <= 0) return;
    if (src.faces) rc_mark_kernel<true><<<rc_grid(n), RC_BLOCK, 0, s>>>(src, n, flag);
    else rc_mark_kernel<false><<<rc_grid(n), RC_BLOCK, 0, s>>>(src, n, flag);
}

void rc_launch_compact(hipStream_t s, const RcLeaves& src, int64_t n, const int32_t* flag, const int32_t* off, int32_t* ids, float* box, uint32_t* bounds,
                       int64_t* n_in) {
    if (n <= 0) return;
    if (src.faces) rc_compact_kernel<true><<<rc_grid(n), RC_BLOCK, 0, s>>>(src, n, flag, off, ids, box, bounds, n_in);
    else rc_compact_kernel<false><<<rc_grid(n), RC_BLOCK, 0, s>>>(src, n, flag, off, ids, box, bounds, n_in);
}

void rc_launch_codes(hipStream_t s, const float* box, int64_t n_in, const uint32_t* bounds, unsigned long long* code, int32_t* iota) {
    if (n_in > 0) rc_codes_kernel<<<rc_grid(n_in), RC_BLOCK, 0, s>>>(box, n_in, bounds, code, iota);
}

void rc_launch_hierarchy(hipStream_t s, const unsigned long long* code, const int32_t* ids, const int32_t* pos_sorted, int64_t n_in, RcNode* nodes,
                         int32_t* leaf_parent) {
    if (n_in > 1) rc_hierarchy_kernel<<<rc_grid(n_in - 1), RC_BLOCK, 0, s>>>(code, ids, pos_sorted, n_in, nodes, leaf_parent);
}

void rc_launch_refit(hipStream_t s, const float* box, const int32_t* pos_sorted, const int32_t* leaf_parent, int64_t n_in, RcNode* nodes) {
    if (n_in > 1) rc_refit_kernel<<<rc_grid(n_in), RC_BLOCK, 0, s>>>(box, pos_sorted, leaf_parent, n_in, nodes);
}

void rc_launch_single(hipStream_t s, const float* box, const int32_t* ids, RcNode* nodes) { rc_single_kernel<<<1, 64, 0, s>>>(box, ids, nodes); }

void rc_launch_cast(hipStream_t s, const RcFrame& fr, const float* dirs, const float* origins, int64_t n_rays, double t_min, double t_max, int mode,
                    const float* vtx, const int32_t* faces, const RcNode* nodes, int64_t n_in, float* t, int32_t* face) {
    if (n_rays > 0) rc_cast_kernel<<<rc_grid(n_rays), RC_BLOCK, 0, s>>>(fr, dirs, origins, n_rays, t_min, t_max, mode, vtx, faces, nodes, n_in, t, face);
}

void rc_launch_points(hipStream_t s, const RcFrame& fr, const float* dirs, const float* origins, int64_t n_rays, float res, const float* t, float* pts,
                      float* cells, int32_t* keep) {
    if (n_rays > 0) rc_points_kernel<<<rc_grid(n_rays), RC_BLOCK, 0, s>>>(fr, dirs, origins, n_rays, res, t, pts, cells, keep);
}
