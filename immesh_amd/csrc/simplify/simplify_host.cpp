// Host side of the weld and the vertex clustering (include/immesh_simplify.h): argument checks, grow-only buffers in the caster's RcSimplify record,
// the pass, its fetches and the apply on the caster's stream.  Nothing here is allocated or launched before the first immesh_simplify.  The host
// knows n_vtx and n_faces, which bound every table (a cluster per vertex, a kept face per face), so no read-back lies between the launches; the
// counters come back once, at the end.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <string>
#include <utility>
#include "../host_ctx.hpp"
#include "../../../include/immesh_simplify.h"
#include "simplify.hpp"

static_assert(sizeof(immesh_simplify_stats) == 11 * 8 && offsetof(immesh_simplify_stats, n_vertices_in) == 0 &&
                  offsetof(immesh_simplify_stats, n_vertices_used) == 8 && offsetof(immesh_simplify_stats, n_alone_not_finite) == 16 &&
                  offsetof(immesh_simplify_stats, n_alone_outside) == 24 && offsetof(immesh_simplify_stats, n_vertices_out) == 32 &&
                  offsetof(immesh_simplify_stats, largest_cluster) == 40 && offsetof(immesh_simplify_stats, n_faces_in) == 48 &&
                  offsetof(immesh_simplify_stats, n_not_counting) == 56 && offsetof(immesh_simplify_stats, n_collapsed) == 64 &&
                  offsetof(immesh_simplify_stats, n_duplicate) == 72 && offsetof(immesh_simplify_stats, n_faces_out) == 80,
              "immesh_simplify_stats layout (immesh_amd/capi.py mirrors it)");

namespace {

enum { SS_VTX_IN = 0, SS_USED, SS_NOT_FINITE, SS_OUTSIDE, SS_VTX_OUT, SS_LARGEST, SS_FACES_IN, SS_NOT_COUNTING, SS_COLLAPSED, SS_DUPLICATE, SS_FACES_OUT };
constexpr int64_t SP_MAX_VTX = 0x7FFFFFFE;                      // the sort's and the scan's int count

int sp_grow(immesh_raycaster* r, RcBuf& b, size_t bytes) { return rc_grow(r->ctx, "simplify", b, bytes); }

int sp_events(immesh_raycaster* r) {
    immesh_ctx* c = r->ctx;
    for (hipEvent_t& e : r->sp.ev)
        if (!e) HIPCHK(c, hipEventCreate(&e));
    if (!r->sp.h_cnt) HIPCHK(c, hipHostMalloc((void**)&r->sp.h_cnt, SP_COUNTERS * 8));
    return 0;
}

int sp_passed(immesh_raycaster* r, const char* who) {
    if (!r->built) { r->ctx->err = std::string(who) + ": no hierarchy has been built (immesh_raycast_build_triangles / _build_mesh)"; return IMMESH_E_INVAL; }
    if (!r->sp.have) { r->ctx->err = std::string(who) + ": no simplify pass since the caster's last build or apply (immesh_simplify)"; return IMMESH_E_INVAL; }
    return 0;
}

int sp_index_bits(int64_t n) {   // the bits the indices 0 .. n - 1 need
    int bits = 1;
    while (bits < 32 && ((int64_t)1 << bits) < n) bits++;
    return bits;
}

}  // namespace

extern "C" {

int immesh_simplify(immesh_raycaster* r, double cell, int32_t mode, int32_t merge_duplicates, immesh_simplify_stats* stats) {
    if (!r) return IMMESH_E_INVAL;
    immesh_ctx* c = r->ctx;
    if (!r->built) { c->err = "simplify: no hierarchy has been built (immesh_raycast_build_triangles / _build_mesh)"; return IMMESH_E_INVAL; }
    if (!(cell >= 0.0) || !std::isfinite(cell)) { c->err = "simplify: need 0 <= cell, finite"; return IMMESH_E_INVAL; }
    if (mode != IMMESH_SIMPLIFY_FIRST && mode != IMMESH_SIMPLIFY_MEAN) { c->err = "simplify: unknown mode " + std::to_string(mode); return IMMESH_E_INVAL; }
    const int64_t nv = r->n_vtx, nf = r->n_faces, ns = std::max(nv, nf);
    if (nv > SP_MAX_VTX) { c->err = "simplify: more than 2^31 - 2 vertices (" + std::to_string(nv) + ")"; return IMMESH_E_INVAL; }
    (void)hipSetDevice(c->cfg.device);
    hipStream_t s = r->s;
    RcSimplify& o = r->sp;
    int rc;
    o.have = false;
    if ((rc = sp_events(r))) return rc;
    if ((rc = sp_grow(r, o.cnt, SP_COUNTERS * 8))) return rc;
    unsigned long long* cnt = (unsigned long long*)o.cnt.p;
    const bool work = nf > 0 && nv > 0;
    if (work) {
        RcBuf* const per_vtx[] = {&o.state, &o.k32, &o.cnum, &o.first, &o.nmem, &o.cstart, &o.vmap};
        for (RcBuf* b : per_vtx)
            if ((rc = sp_grow(r, *b, (size_t)nv * 4))) return rc;
        if ((rc = sp_grow(r, o.k64, (size_t)nv * 8))) return rc;
        if ((rc = sp_grow(r, o.vtx_out, (size_t)nv * 12))) return rc;
        RcBuf* const per_face[] = {&o.fk32, &o.keep, &o.koff, &o.fmap};
        for (RcBuf* b : per_face)
            if ((rc = sp_grow(r, *b, (size_t)nf * 4))) return rc;
        if ((rc = sp_grow(r, o.fk64, (size_t)nf * 8))) return rc;
        if ((rc = sp_grow(r, o.fstatus, (size_t)nf))) return rc;
        if ((rc = sp_grow(r, o.faces_out, (size_t)nf * 12))) return rc;
        if ((rc = sp_grow(r, o.key_a, (size_t)ns * 8))) return rc;
        if ((rc = sp_grow(r, o.key_b, (size_t)ns * 8))) return rc;
        RcBuf* const sorts[] = {&o.k32s, &o.iota, &o.val_a, &o.val_b};
        for (RcBuf* b : sorts)
            if ((rc = sp_grow(r, *b, (size_t)ns * 4))) return rc;
        const size_t temp = std::max({exclusive_sum_temp_bytes((int)ns), sort_pairs_u64_temp_bytes((int)ns), sort_pairs_u32_temp_bytes((int)ns)}) + 256;
        if ((rc = sp_grow(r, r->tree.temp, temp))) return rc;  // the caster's scan and sort scratch
    }
    HIPCHK(c, hipEventRecord(o.ev[0], s));
    HIPCHK(c, hipMemsetAsync(cnt, 0, SP_COUNTERS * 8, s));
    if (work) {
        const float* vtx = (const float*)r->vtx.p;
        const int32_t* faces = (const int32_t*)r->faces.p;
        void* temp = r->tree.temp.p;
        const size_t temp_bytes = r->tree.temp.bytes;
        int32_t *state = (int32_t*)o.state.p, *cnum = (int32_t*)o.cnum.p, *vmap = (int32_t*)o.vmap.p, *iota = (int32_t*)o.iota.p;
        int32_t *val_a = (int32_t*)o.val_a.p, *val_b = (int32_t*)o.val_b.p;
        unsigned long long *k64 = (unsigned long long*)o.k64.p, *key_a = (unsigned long long*)o.key_a.p, *key_b = (unsigned long long*)o.key_b.p;
        uint32_t *k32 = (uint32_t*)o.k32.p, *k32s = (uint32_t*)o.k32s.p;
        // the vertices: mark, keys, the stable sort with values = the vertex indices
        HIPCHK(c, hipMemsetAsync(state, 0, (size_t)nv * 4, s));
        sp_launch_mark(s, faces, nf, nv, state);
        sp_launch_keys(s, vtx, nv, cell, state, k64, k32, iota, cnt);
        if (cell > 0.0) {
            sort_pairs_u64(s, temp, temp_bytes, k64, key_b, iota, val_b, (int)nv, 64);   // 63 bits of cell and the bit that sets the others apart
        } else {                                                // 96 bits: two stable passes, the low word first
            sort_pairs_u32(s, temp, temp_bytes, k32, k32s, iota, val_a, (int)nv, 32);
            sp_launch_gather64(s, k64, val_a, nv, key_a);
            sort_pairs_u64(s, temp, temp_bytes, key_a, key_b, val_a, val_b, (int)nv, 64);
        }
        // the sorts' buffers are free again: the run tables lie in them
        const int32_t* sv = val_b;
        int32_t *head = (int32_t*)k32s, *scan = val_a, *rstart = (int32_t*)key_a, *rend = rstart + nv, *lab = (int32_t*)key_b, *islab = lab + nv;
        sp_launch_heads(s, sv, nv, state, k64, k32, head);
        exclusive_sum_i32(s, temp, temp_bytes, head, scan, (int)nv);
        sp_launch_runs(s, nv, head, scan, rstart, rend);
        sp_launch_labels(s, sv, nv, state, head, scan, rstart, lab, islab);
        exclusive_sum_i32(s, temp, temp_bytes, islab, cnum, (int)nv);
        sp_launch_clusters(s, vtx, sv, nv, state, head, scan, rend, cnum, (int32_t*)o.first.p, (int32_t*)o.nmem.p, (int32_t*)o.cstart.p, (float*)o.vtx_out.p,
                           cnt);
        if (mode == IMMESH_SIMPLIFY_MEAN && cell > 0.0)
            sp_launch_mean(s, vtx, sv, nv, (const int32_t*)o.nmem.p, (const int32_t*)o.cstart.p, cnt, (float*)o.vtx_out.p);
        sp_launch_vmap(s, nv, state, lab, cnum, vmap);
        // the faces: the mapped triples, the duplicates by a sort of the sorted triples (values = the face indices), the compaction
        int8_t* fstatus = (int8_t*)o.fstatus.p;
        int32_t *keep = (int32_t*)o.keep.p, *koff = (int32_t*)o.koff.p;
        unsigned long long* fk64 = (unsigned long long*)o.fk64.p;
        uint32_t* fk32 = (uint32_t*)o.fk32.p;
        if (merge_duplicates) {
            const int bits = sp_index_bits(nv);                 // a new index is below n_vtx; the key that sets the others apart stays above in these bits too
            sp_launch_faces(s, faces, nf, nv, vmap, fstatus, keep, fk64, fk32, iota, cnt);
            sort_pairs_u32(s, temp, temp_bytes, fk32, k32s, iota, val_a, (int)nf, bits);
            sp_launch_gather64(s, fk64, val_a, nf, key_a);
            sort_pairs_u64(s, temp, temp_bytes, key_a, key_b, val_a, val_b, (int)nf, 32 + bits);
            sp_launch_duplicates(s, val_b, nf, fk64, fk32, fstatus, keep, cnt);
        } else {
            sp_launch_faces(s, faces, nf, nv, vmap, fstatus, keep, nullptr, nullptr, nullptr, cnt);
        }
        exclusive_sum_i32(s, temp, temp_bytes, keep, koff, (int)nf);
        sp_launch_compact(s, faces, nf, vmap, keep, koff, (int32_t*)o.faces_out.p, (int32_t*)o.fmap.p, cnt);
    }
    HIPCHK(c, hipEventRecord(o.ev[1], s));
    unsigned long long* h = o.h_cnt;
    HIPCHK(c, hipMemcpyAsync(h, cnt, SP_COUNTERS * 8, hipMemcpyDeviceToHost, s));   // the one read-back
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(s));
    (void)hipEventElapsedTime(&o.ms[0], o.ev[0], o.ev[1]);
    int64_t* st = o.st;
    st[SS_VTX_IN] = nv; st[SS_USED] = (int64_t)h[SP_N_USED]; st[SS_NOT_FINITE] = (int64_t)h[SP_N_ALONE_NOT_FINITE];
    st[SS_OUTSIDE] = (int64_t)h[SP_N_ALONE_OUTSIDE]; st[SS_VTX_OUT] = (int64_t)h[SP_N_CLUSTERS]; st[SS_LARGEST] = (int64_t)h[SP_LARGEST];
    st[SS_FACES_IN] = nf; st[SS_NOT_COUNTING] = (int64_t)h[SP_N_NOT_COUNTING]; st[SS_COLLAPSED] = (int64_t)h[SP_N_COLLAPSED];
    st[SS_DUPLICATE] = (int64_t)h[SP_N_DUPLICATE]; st[SS_FACES_OUT] = (int64_t)h[SP_N_FACES_OUT];
    if (!work) st[SS_NOT_COUNTING] = nf;                        // (faces without a vertex to name: no build accepts them)
    o.have = true;
    if (stats) std::memcpy(stats, st, sizeof(*stats));
    return 0;
}

int immesh_simplify_vertices(immesh_raycaster* r, float* vtx_out, int32_t* first_vertex, int32_t* n_members, int64_t cap, int64_t* n_out) {
    if (!r) return IMMESH_E_INVAL;
    immesh_ctx* c = r->ctx;
    int rc;
    if ((rc = sp_passed(r, "simplify_vertices"))) return rc;
    if (cap < 0) { c->err = "simplify_vertices: cap is negative"; return IMMESH_E_INVAL; }
    const RcSimplify& o = r->sp;
    const int64_t n = o.st[SS_VTX_OUT];
    if (n_out) *n_out = n;
    if ((!vtx_out && !first_vertex && !n_members) || n == 0) return 0;
    if (cap < n) {
        c->err = "simplify_vertices: cap " + std::to_string(cap) + " < " + std::to_string(n) + " clusters";
        return IMMESH_E_CAPACITY;
    }
    (void)hipSetDevice(c->cfg.device);
    if (vtx_out) HIPCHK(c, hipMemcpy(vtx_out, o.vtx_out.p, (size_t)n * 12, hipMemcpyDeviceToHost));
    if (first_vertex) HIPCHK(c, hipMemcpy(first_vertex, o.first.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    if (n_members) HIPCHK(c, hipMemcpy(n_members, o.nmem.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    return 0;
}

int immesh_simplify_maps(immesh_raycaster* r, int32_t* vmap, int32_t* fmap, int8_t* fstatus) {
    if (!r) return IMMESH_E_INVAL;
    immesh_ctx* c = r->ctx;
    int rc;
    if ((rc = sp_passed(r, "simplify_maps"))) return rc;
    const RcSimplify& o = r->sp;
    const int64_t nv = r->n_vtx, nf = r->n_faces;
    (void)hipSetDevice(c->cfg.device);
    if (nf == 0 || nv == 0) {                                   // nothing was launched: no vertex is used and no face counts
        if (vmap && nv > 0) std::memset(vmap, 0xFF, (size_t)nv * 4);
        if (fmap && nf > 0) std::memset(fmap, 0xFF, (size_t)nf * 4);
        if (fstatus && nf > 0) std::memset(fstatus, IMMESH_FACE_NOT_COUNTING, (size_t)nf);
        return 0;
    }
    if (vmap && nv > 0) HIPCHK(c, hipMemcpy(vmap, o.vmap.p, (size_t)nv * 4, hipMemcpyDeviceToHost));
    if (fmap) HIPCHK(c, hipMemcpy(fmap, o.fmap.p, (size_t)nf * 4, hipMemcpyDeviceToHost));
    if (fstatus) HIPCHK(c, hipMemcpy(fstatus, o.fstatus.p, (size_t)nf, hipMemcpyDeviceToHost));
    return 0;
}

int immesh_simplify_faces(immesh_raycaster* r, int32_t* faces_out, int64_t cap, int64_t* n_out) {
    if (!r) return IMMESH_E_INVAL;
    immesh_ctx* c = r->ctx;
    int rc;
    if ((rc = sp_passed(r, "simplify_faces"))) return rc;
    if (cap < 0) { c->err = "simplify_faces: cap is negative"; return IMMESH_E_INVAL; }
    const int64_t n = r->sp.st[SS_FACES_OUT];
    if (n_out) *n_out = n;
    if (!faces_out || n == 0) return 0;
    if (cap < n) {
        c->err = "simplify_faces: cap " + std::to_string(cap) + " < " + std::to_string(n) + " kept faces";
        return IMMESH_E_CAPACITY;
    }
    (void)hipSetDevice(c->cfg.device);
    HIPCHK(c, hipMemcpy(faces_out, r->sp.faces_out.p, (size_t)n * 12, hipMemcpyDeviceToHost));
    return 0;
}

int immesh_simplify_apply(immesh_raycaster* r) {
    if (!r) return IMMESH_E_INVAL;
    immesh_ctx* c = r->ctx;
    int rc;
    if ((rc = sp_passed(r, "simplify_apply"))) return rc;
    RcSimplify& o = r->sp;
    const int64_t nv = o.st[SS_VTX_OUT], nf = o.st[SS_FACES_OUT];
    (void)hipSetDevice(c->cfg.device);
    hipStream_t s = r->s;
    HIPCHK(c, hipEventRecord(o.ev[2], s));
    if (nv > 0) {                                               // (zero clusters: nothing was launched and the result's buffers may not exist)
        std::swap(r->vtx.p, o.vtx_out.p);                       // the stream is idle: the pass synchronised
        std::swap(r->vtx.bytes, o.vtx_out.bytes);
        std::swap(r->faces.p, o.faces_out.p);
        std::swap(r->faces.bytes, o.faces_out.bytes);
    }
    o.have = false;
    r->ot.have = false;
    r->hl.have = false;
    r->so.have = false;                                         // (the build discards a smoothing pass too)
    rc = rc_build(r, nv, nf);                                   // discards the last cast, the samples and the analysis; the stream is idle on return
    if (rc) return rc;
    HIPCHK(c, hipEventRecord(o.ev[3], s));
    HIPCHK(c, hipStreamSynchronize(s));
    (void)hipEventElapsedTime(&o.ms[1], o.ev[2], o.ev[3]);
    return 0;
}

int immesh_simplify_last_timing(immesh_raycaster* r, float* ms) {
    if (!r || !ms) return IMMESH_E_INVAL;
    ms[0] = r->sp.ms[0]; ms[1] = r->sp.ms[1];
    return 0;
}

}  // extern "C"
