// Device helpers shared by the kernels on the caster's hierarchy: raycast_kernels.hip, closest_kernels.hip, nearest_kernels.hip, align/align_kernels.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "raycast.hpp"

namespace {

inline unsigned rc_grid(int64_t n) { return (unsigned)((n + RC_BLOCK - 1) / RC_BLOCK); }

__device__ __forceinline__ void rc_cross(const double* p, const double* q, double* o) {
    o[0] = p[1] * q[2] - p[2] * q[1];
    o[1] = p[2] * q[0] - p[0] * q[2];
    o[2] = p[0] * q[1] - p[1] * q[0];
}
__device__ __forceinline__ double rc_dot(const double* p, const double* q) { return (p[0] * q[0] + p[1] * q[1]) + p[2] * q[2]; }

// face f: its float box, and its corners as doubles relative to the origin o
__device__ __forceinline__ void rc_load_face(const float* __restrict__ vtx, const int32_t* __restrict__ faces, int32_t f, const double* o, float* lo,
                                             float* hi, double (*A)[3]) {
    for (int k = 0; k < 3; k++) {
        const float* v = vtx + 3 * (int64_t)faces[3 * (int64_t)f + k];
        for (int j = 0; j < 3; j++) {
            const float x = v[j];
            lo[j] = k ? fminf(lo[j], x) : x;
            hi[j] = k ? fmaxf(hi[j], x) : x;
            A[k][j] = (double)x - o[j];
        }
    }
}

// ---- distance queries (closest face, nearest cloud point): the contracts' shared rules and the one walk --------------------------------------
// the contracts' Point rule: false when the point has no answer by rule
__device__ __forceinline__ bool dq_point(const RcFrame& fr, bool has_frame, const float* __restrict__ pts, int64_t i, double* p) {
    const float f[3] = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
    bool ok = isfinite(f[0]) && isfinite(f[1]) && isfinite(f[2]);
    const double x[3] = {(double)f[0], (double)f[1], (double)f[2]};
    for (int k = 0; k < 3; k++) {
        p[k] = has_frame ? ((fr.rot[3 * k] * x[0] + fr.rot[3 * k + 1] * x[1]) + fr.rot[3 * k + 2] * x[2]) + fr.pos[k] : x[k];
        ok = ok && fabs(p[k]) < 0x1p128;   // (false for NaN)
    }
    return ok;
}

// the contracts' Box bound of a float box
__device__ __forceinline__ double dq_box(const double* p, const float* lo, const float* hi) {
    double e[3];
    for (int k = 0; k < 3; k++) e[k] = fmax(fmax((double)lo[k] - p[k], p[k] - (double)hi[k]), 0.0);
    return (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2];
}

__device__ __forceinline__ double rc_unit(double x) { return x > 0.0 ? (x < 1.0 ? x : 1.0) : 0.0; }   // held to [0, 1]; NaN -> 0

// the closest-point contract's Face rule (the closest query and the alignment step share it): q, the closest point of the face (a, b, c relative to the query) by the region method
__device__ __forceinline__ void rc_face_point(const double* a, const double* b, const double* c, double* q) {
    double ab[3], ac[3], ma[3], mb[3], mc[3];
    for (int k = 0; k < 3; k++) { ab[k] = b[k] - a[k]; ac[k] = c[k] - a[k]; ma[k] = -a[k]; mb[k] = -b[k]; mc[k] = -c[k]; }
    const double d1 = rc_dot(ab, ma), d2 = rc_dot(ac, ma);
    if (d1 <= 0.0 && d2 <= 0.0) { q[0] = a[0]; q[1] = a[1]; q[2] = a[2]; return; }
    const double d3 = rc_dot(ab, mb), d4 = rc_dot(ac, mb);
    if (d3 >= 0.0 && d4 <= d3) { q[0] = b[0]; q[1] = b[1]; q[2] = b[2]; return; }
    const double vc = d1 * d4 - d3 * d2;
    const double den_ab = d1 - d3;
    if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0 && den_ab != 0.0) {
        const double v = rc_unit(d1 / den_ab);
        for (int k = 0; k < 3; k++) q[k] = a[k] + v * ab[k];
        return;
    }
    const double d5 = rc_dot(ab, mc), d6 = rc_dot(ac, mc);
    if (d6 >= 0.0 && d5 <= d6) { q[0] = c[0]; q[1] = c[1]; q[2] = c[2]; return; }
    const double vb = d5 * d2 - d1 * d6;
    const double den_ac = d2 - d6;
    if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0 && den_ac != 0.0) {
        const double w = rc_unit(d2 / den_ac);
        for (int k = 0; k < 3; k++) q[k] = a[k] + w * ac[k];
        return;
    }
    const double va = d3 * d6 - d5 * d4;
    const double e43 = d4 - d3, e56 = d5 - d6;
    const double den_bc = e43 + e56;
    if (va <= 0.0 && e43 >= 0.0 && e56 >= 0.0 && den_bc != 0.0) {
        const double w = rc_unit(e43 / den_bc);
        for (int k = 0; k < 3; k++) q[k] = b[k] + w * (c[k] - b[k]);
        return;
    }
    const double sum = (va + vb) + vc;
    const double inv = sum != 0.0 ? 1.0 / sum : 0.0;
    const double v = rc_unit(vb * inv);
    const double w1 = rc_unit(vc * inv), rest = 1.0 - v;
    const double w = w1 < rest ? w1 : rest;
    for (int k = 0; k < 3; k++) q[k] = (a[k] + ab[k] * v) + ac[k] * w;
}

__device__ __forceinline__ float dq_round_down(double x) {   // x >= 0: the largest float <= x
    float f = (float)x;
    if ((double)f > x) f = __uint_as_float(__float_as_uint(f) - 1u);
    return f;
}

// The best-first walk of one point p: a per-lane stack in private memory (depth bound: raycast.hpp), the child with the smaller box bound L first.
// A node is skipped only when L of its own box exceeds `best` (r2 on entry, then the best D); the bound kept on the stack is a float rounded DOWN, so
// it never exceeds L (has the argument that this prunes exactly).  leaf.dist(id) is D of leaf id; the walk alone decides
// whether it wins -- a smaller D, or an equal D and a lower id -- and then calls leaf.accept().  A leaf met twice (the single-leaf tree) ties with
// itself and changes nothing.
template <class Leaf>
__device__ __forceinline__ void dq_walk(const RcNode* __restrict__ nodes, const double* p, double& best, int32_t& best_id, Leaf& leaf) {
    int32_t stack[RC_STACK];
    float stack_key[RC_STACK];
    int sp = 0;
    int32_t cur = 0;
    for (;;) {
        if (cur < 0) {   // a leaf
            const int32_t id = ~cur;
            const double D = leaf.dist(id);
            if (D < best || (D == best && (best_id < 0 || id < best_id))) {
                best = D; best_id = id;
                leaf.accept();
            }
        } else {
            const RcNode& nd = nodes[cur];
            const double l0 = dq_box(p, nd.lo[0], nd.hi[0]), l1 = dq_box(p, nd.lo[1], nd.hi[1]);
            const bool h0 = !(l0 > best), h1 = !(l1 > best);
            const int32_t c0 = nd.child[0], c1 = nd.child[1];
            if (h0 && h1) {
                const bool first0 = l0 <= l1;       // the nearer child first: its leaves prune the other
                stack[sp] = first0 ? c1 : c0;
                stack_key[sp] = dq_round_down(first0 ? l1 : l0);
                sp++;
                cur = first0 ? c0 : c1;
                continue;
            }
            if (h0 || h1) { cur = h0 ? c0 : c1; continue; }
        }
        // next entry whose bound has not been overtaken
        bool found = false;
        while (sp > 0) {
            sp--;
            if (!((double)stack_key[sp] > best)) { cur = stack[sp]; found = true; break; }
        }
        if (!found) break;
    }
}

// dq_walk's sibling for queries that keep more than one leaf (k nearest, radius count): the same order, the same pruning rule !(L > bound) and the
// same float keys rounded down, but the leaf is *offered* -- sink.offer(id) takes it or not and returns the bound that holds from then on (r2 until a
// k-list is full, then its k-th D; r2 throughout for a count).  The bound never grows.  A node with L == bound is still entered: it can hold a point
// at the k-th D with a lower index.  The single-leaf tree names its one leaf as both children (rc_launch_single); a list
// would hold it twice and a counter count it twice, so n_in == 1 is offered once, by rule, and no node is read.
template <class Sink>
__device__ __forceinline__ void dq_walk_offer(const RcNode* __restrict__ nodes, int64_t n_in, const double* p, double bound, Sink& sink) {
    if (n_in == 1) { (void)sink.offer(~nodes[0].child[0]); return; }
    int32_t stack[RC_STACK];
    float stack_key[RC_STACK];
    int sp = 0;
    int32_t cur = 0;
    for (;;) {
        if (cur < 0) {   // a leaf
            bound = sink.offer(~cur);
        } else {
            const RcNode& nd = nodes[cur];
            const double l0 = dq_box(p, nd.lo[0], nd.hi[0]), l1 = dq_box(p, nd.lo[1], nd.hi[1]);
            const bool h0 = !(l0 > bound), h1 = !(l1 > bound);
            const int32_t c0 = nd.child[0], c1 = nd.child[1];
            if (h0 && h1) {
                const bool first0 = l0 <= l1;
                stack[sp] = first0 ? c1 : c0;
                stack_key[sp] = dq_round_down(first0 ? l1 : l0);
                sp++;
                cur = first0 ? c0 : c1;
                continue;
            }
            if (h0 || h1) { cur = h0 ? c0 : c1; continue; }
        }
        bool found = false;
        while (sp > 0) {
            sp--;
            if (!((double)stack_key[sp] > bound)) { cur = stack[sp]; found = true; break; }
        }
        if (!found) break;
    }
}

}  // namespace
