// Host side of the weld and the vertex clustering (include/immesh_simplify.h): argument checks, grow-only buffers in the caster's RcSimplify record,
// the pass, its fetches and the apply on the caster's stream.  Nothing here is allocated or launched before the first immesh_simplify.  The host
// knows n_vtx and n_faces, which bound every table (a cluster per vertex, a kept face per face), so no read-back lies between the launches; the
// counters come back once, at the end.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <string>
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

constexpr int64_t SP_MAX_VTX = 0x7FFFFFFE;                      // the sort's and the scan's int count

int sp_grow(immesh_raycaster* r, RcBuf& b, size_t bytes) { return rc_pass_grow(r->sp, b, bytes); }

int sp_passed(immesh_raycaster* r, const char* who) {
    const int rc = rc_built(r, who);
    return rc ? rc : rc_passed(r, who, r->sp, "no simplify pass since the caster's last build or apply (immesh_simplify)");
}

}  // namespace

extern "C" {

int immesh_simplify(immesh_raycaster* r, double cell, int32_t mode, int32_t merge_duplicates, immesh_simplify_stats* stats) {
    if (!r) return IMMESH_E_INVAL;
    immesh_ctx* c = r->ctx;
    int rc;
    if ((rc = rc_built(r, "simplify"))) return rc;
    if (!(cell >= 0.0) || !std::isfinite(cell)) { c->err = "simplify: need 0 <= cell, finite"; return IMMESH_E_INVAL; }
    if (mode != IMMESH_SIMPLIFY_FIRST && mode != IMMESH_SIMPLIFY_MEAN) { c->err = "simplify: unknown mode " + std::to_string(mode); return IMMESH_E_INVAL; }
    const int64_t nv = r->n_vtx, nf = r->n_faces, ns = std::max(nv, nf);
    if (nv > SP_MAX_VTX) { c->err = "simplify: more than 2^31 - 2 vertices (" + std::to_string(nv) + ")"; return IMMESH_E_INVAL; }
    (void)hipSetDevice(c->cfg.device);
    hipStream_t s = r->s;
    RcSimplify& o = r->sp;
    o.have = false;
    if ((rc = rc_pass_ready(c, s, "simplify", o, SP_COUNTERS, SP_COUNTERS))) return rc;
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
    if ((rc = rc_pass_begin(o, 0))) return rc;
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
            const int bits = rc_index_bits(nv);                 // a new index is below n_vtx; the key that sets the others apart stays above in these bits too
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
    if ((rc = rc_pass_end(o, 0, 1, 0, 0, SP_COUNTERS))) return rc;   // the one read-back
    const unsigned long long* h = o.h_cnt;
    immesh_simplify_stats& st = o.st;
    st.n_vertices_in = nv; st.n_vertices_used = (int64_t)h[SP_N_USED]; st.n_alone_not_finite = (int64_t)h[SP_N_ALONE_NOT_FINITE];
    st.n_alone_outside = (int64_t)h[SP_N_ALONE_OUTSIDE]; st.n_vertices_out = (int64_t)h[SP_N_CLUSTERS]; st.largest_cluster = (int64_t)h[SP_LARGEST];
    st.n_faces_in = nf; st.n_not_counting = (int64_t)h[SP_N_NOT_COUNTING]; st.n_collapsed = (int64_t)h[SP_N_COLLAPSED];
    st.n_duplicate = (int64_t)h[SP_N_DUPLICATE]; st.n_faces_out = (int64_t)h[SP_N_FACES_OUT];
    if (!work) st.n_not_counting = nf;                          // (faces without a vertex to name: no build accepts them)
    o.have = true;
    if (stats) *stats = st;
    return 0;
}

int immesh_simplify_vertices(immesh_raycaster* r, float* vtx_out, int32_t* first_vertex, int32_t* n_members, int64_t cap, int64_t* n_out) {
    if (!r) return IMMESH_E_INVAL;
    immesh_ctx* c = r->ctx;
    int rc;
    if ((rc = sp_passed(r, "simplify_vertices"))) return rc;
    const RcSimplify& o = r->sp;
    const int64_t n = o.st.n_vertices_out;
    if ((rc = rc_cap(c, "simplify_vertices", cap, n, n_out, vtx_out || first_vertex || n_members, "clusters"))) return rc;
    (void)hipSetDevice(c->cfg.device);
    if ((rc = rc_fetch(c, vtx_out, o.vtx_out.p, (size_t)n * 12))) return rc;
    if ((rc = rc_fetch(c, first_vertex, o.first.p, (size_t)n * 4))) return rc;
    return rc_fetch(c, n_members, o.nmem.p, (size_t)n * 4);
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
    if ((rc = rc_fetch(c, vmap, o.vmap.p, (size_t)nv * 4))) return rc;
    if ((rc = rc_fetch(c, fmap, o.fmap.p, (size_t)nf * 4))) return rc;
    return rc_fetch(c, fstatus, o.fstatus.p, (size_t)nf);
}

int immesh_simplify_faces(immesh_raycaster* r, int32_t* faces_out, int64_t cap, int64_t* n_out) {
    if (!r) return IMMESH_E_INVAL;
    immesh_ctx* c = r->ctx;
    int rc;
    if ((rc = sp_passed(r, "simplify_faces"))) return rc;
    const int64_t n = r->sp.st.n_faces_out;
    if ((rc = rc_cap(c, "simplify_faces", cap, n, n_out, faces_out != nullptr, "kept faces"))) return rc;
    (void)hipSetDevice(c->cfg.device);
    return rc_fetch(c, faces_out, r->sp.faces_out.p, (size_t)n * 12);
}

int immesh_simplify_apply(immesh_raycaster* r) {
    if (!r) return IMMESH_E_INVAL;
    immesh_ctx* c = r->ctx;
    int rc;
    if ((rc = sp_passed(r, "simplify_apply"))) return rc;
    RcSimplify& o = r->sp;
    const int64_t nv = o.st.n_vertices_out, nf = o.st.n_faces_out;
    (void)hipSetDevice(c->cfg.device);
    hipStream_t s = r->s;
    HIPCHK(c, hipEventRecord(o.ev[2], s));
    if (nv > 0) {                                               // (zero clusters: nothing was launched and the result's buffers may not exist)
        rc_swap(r->vtx, o.vtx_out);                             // the stream is idle: the pass synchronised
        rc_swap(r->faces, o.faces_out);
    }
    if ((rc = rc_build(r, nv, nf))) return rc;                  // discards what read the snapshot, this pass too; the stream is idle on return
    return rc_pass_span(o, 2, 3, 1);
}

int immesh_simplify_last_timing(immesh_raycaster* r, float* ms) {
    if (!r || !ms) return IMMESH_E_INVAL;
    ms[0] = r->sp.ms[0]; ms[1] = r->sp.ms[1];
    return 0;
}

}  // extern "C"
