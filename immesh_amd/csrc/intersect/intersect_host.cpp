// Host side of the self-intersection pass (include/immesh_intersect.h): argument checks, grow-only buffers in the caster's RcIntersect record, the
// pass, its fetches and the apply on the caster's stream.  Nothing here is allocated or launched before the first immesh_self_intersect.  Two counts
// come back between the launches, through the pass' pinned words: the candidates (checked against max_candidates; they size the per-candidate
// buffers) and the hits (they size the sort).
#include <algorithm>
#include <cstddef>
#include <cstring>
#include <string>
#include "../host_ctx.hpp"
#include "../../../include/immesh_intersect.h"
#include "../render/render.hpp"
#include "intersect.hpp"

static_assert(sizeof(immesh_intersect_stats) == 13 * 8 && offsetof(immesh_intersect_stats, n_faces) == 0 && offsetof(immesh_intersect_stats, n_in_tree) == 8 &&
                  offsetof(immesh_intersect_stats, n_taking_part) == 16 && offsetof(immesh_intersect_stats, n_candidates) == 24 &&
                  offsetof(immesh_intersect_stats, n_share) == 32 && offsetof(immesh_intersect_stats, n_pairs) == 64 &&
                  offsetof(immesh_intersect_stats, n_pairs_share0) == 72 && offsetof(immesh_intersect_stats, n_pairs_share1) == 80 &&
                  offsetof(immesh_intersect_stats, n_faces_hit) == 88 && offsetof(immesh_intersect_stats, max_partners) == 96,
              "immesh_intersect_stats layout (immesh_amd/capi.py mirrors it)");

namespace {

constexpr int64_t IX_MAX_CANDIDATES = 0x7FFFFFFE;               // the sort's and the scan's int count

int ix_grow(immesh_raycaster* r, RcBuf& b, size_t bytes) { return rc_pass_grow(r->ix, b, bytes); }

int ix_passed(immesh_raycaster* r, const char* who) {
    const int rc = rc_built(r, who);
    return rc ? rc : rc_passed(r, who, r->ix, "no self-intersection pass since the caster's last build or apply (immesh_self_intersect)");
}

// the counters [first, first + n) to the pinned words; the stream is idle on return
int ix_read(immesh_raycaster* r, RcIntersect& o, int first, int n) {
    immesh_ctx* c = r->ctx;
    HIPCHK(c, hipMemcpyAsync(o.h_cnt + first, (const unsigned long long*)o.cnt.p + first, (size_t)n * 8, hipMemcpyDeviceToHost, r->s));
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(r->s));
    return 0;
}

}  // namespace

extern "C" {

int immesh_self_intersect(immesh_raycaster* r, int64_t max_candidates, immesh_intersect_stats* stats) {
    if (!r) return IMMESH_E_INVAL;
    immesh_ctx* c = r->ctx;
    int rc;
    if ((rc = rc_built(r, "self_intersect"))) return rc;
    if (max_candidates < 1 || max_candidates > IX_MAX_CANDIDATES) {
        c->err = "self_intersect: need 1 <= max_candidates <= 2^31 - 2 (" + std::to_string(max_candidates) + ")";
        return IMMESH_E_INVAL;
    }
    const int64_t nv = r->n_vtx, nf = r->n_faces;
    (void)hipSetDevice(c->cfg.device);
    hipStream_t s = r->s;
    RcIntersect& o = r->ix;
    o.have = false;
    if ((rc = rc_pass_ready(c, s, "self_intersect", o, IX_COUNTERS, IX_COUNTERS))) return rc;
    unsigned long long* cnt = (unsigned long long*)o.cnt.p;
    if (nf > 0) {
        RcBuf* const per_face[] = {&o.cnt32, &o.off, &o.npart, &o.keep, &o.koff, &o.fmap};
        for (RcBuf* b : per_face)
            if ((rc = ix_grow(r, *b, (size_t)nf * 4))) return rc;
        if ((rc = ix_grow(r, o.take, (size_t)nf))) return rc;
        if ((rc = ix_grow(r, r->tree.temp, rd_scan_temp_bytes(1, 1, nf) + 256))) return rc;   // the caster's scan and sort scratch
    }
    const float* vtx = (const float*)r->vtx.p;
    const int32_t* faces = (const int32_t*)r->faces.p;
    const RcNode* nodes = (const RcNode*)r->tree.nodes.p;
    const int8_t* take = (const int8_t*)o.take.p;
    int32_t *cnt32 = (int32_t*)o.cnt32.p, *off = (int32_t*)o.off.p, *npart = (int32_t*)o.npart.p, *keep = (int32_t*)o.keep.p, *koff = (int32_t*)o.koff.p;
    immesh_intersect_stats& st = o.st;
    st = immesh_intersect_stats{};
    st.n_faces = nf; st.n_in_tree = r->tree.n_in;
    // ---- candidates: count, the one round trip for the total, scan, emit
    if ((rc = rc_pass_begin(o, 0))) return rc;
    ix_launch_take(s, vtx, nv, faces, nf, (int8_t*)o.take.p, cnt);
    ix_launch_walk(s, vtx, faces, nf, take, nodes, r->tree.n_in, cnt32, nullptr, nullptr, cnt);
    if ((rc = ix_read(r, o, 0, 2))) return rc;
    const int64_t n_cand = (int64_t)o.h_cnt[IX_N_CANDIDATES];
    st.n_taking_part = (int64_t)o.h_cnt[IX_N_TAKING]; st.n_candidates = n_cand;
    if (n_cand > max_candidates) {
        if ((rc = rc_pass_span(o, 0, 1, 0))) return rc;
        if (stats) *stats = st;                                 // n_candidates and the counts before it; no result exists
        c->err = "self_intersect: cap " + std::to_string(max_candidates) + " < " + std::to_string(n_cand) + " candidate pairs";
        return IMMESH_E_CAPACITY;
    }
    if (n_cand > 0) {
        if ((rc = ix_grow(r, o.key, (size_t)n_cand * 8))) return rc;
        if ((rc = ix_grow(r, o.cmask, (size_t)n_cand))) return rc;
        if ((rc = ix_grow(r, o.flag, (size_t)n_cand * 4))) return rc;
        if ((rc = ix_grow(r, o.hoff, (size_t)n_cand * 4))) return rc;
        if ((rc = ix_grow(r, r->tree.temp, rd_scan_temp_bytes(1, 1, std::max(nf, n_cand)) + 256))) return rc;
        rd_scan_i32(s, r->tree.temp.p, r->tree.temp.bytes, cnt32, off, nf);
        ix_launch_walk(s, vtx, faces, nf, take, nodes, r->tree.n_in, nullptr, off, (unsigned long long*)o.key.p, cnt);
    }
    if ((rc = rc_pass_span(o, 0, 1, 0))) return rc;
    // ---- tests: the masks, flag / scan / compaction of the hits, the round trip for their number, the sort, the pairs and n_partners
    const int bits = rc_index_bits(nf);
    int64_t n_hits = 0;
    HIPCHK(c, hipEventRecord(o.ev[2], s));
    if (nf > 0) HIPCHK(c, hipMemsetAsync(npart, 0, (size_t)nf * 4, s));
    if (n_cand > 0) {
        const unsigned long long* key = (const unsigned long long*)o.key.p;
        int32_t *flag = (int32_t*)o.flag.p, *hoff = (int32_t*)o.hoff.p;
        ix_launch_test(s, vtx, faces, key, n_cand, (uint8_t*)o.cmask.p, flag, cnt);
        if ((rc = ix_read(r, o, IX_N_PAIRS, 1))) return rc;
        n_hits = (int64_t)o.h_cnt[IX_N_PAIRS];
        if (n_hits > 0) {
            if ((rc = ix_grow(r, o.hkey_a, (size_t)n_hits * 8))) return rc;
            if ((rc = ix_grow(r, o.hkey_b, (size_t)n_hits * 8))) return rc;
            if ((rc = ix_grow(r, o.hval_a, (size_t)n_hits * 4))) return rc;
            if ((rc = ix_grow(r, o.hval_b, (size_t)n_hits * 4))) return rc;
            if ((rc = ix_grow(r, o.pairs, (size_t)n_hits * 8))) return rc;
            if ((rc = ix_grow(r, o.pmask, (size_t)n_hits))) return rc;
            if ((rc = ix_grow(r, r->tree.temp, std::max(rd_scan_temp_bytes(1, 1, std::max(nf, n_cand)), sort_pairs_u64_temp_bytes((int)n_hits)) + 256))) return rc;
            rd_scan_i32(s, r->tree.temp.p, r->tree.temp.bytes, flag, hoff, n_cand);
            ix_launch_compact(s, key, (const uint8_t*)o.cmask.p, flag, hoff, n_cand, bits, (unsigned long long*)o.hkey_a.p, (int32_t*)o.hval_a.p);
            sort_pairs_u64(s, r->tree.temp.p, r->tree.temp.bytes, (const unsigned long long*)o.hkey_a.p, (unsigned long long*)o.hkey_b.p,
                           (const int32_t*)o.hval_a.p, (int32_t*)o.hval_b.p, (int)n_hits, 2 * bits);
            ix_launch_pairs(s, (const unsigned long long*)o.hkey_b.p, (const int32_t*)o.hval_b.p, n_hits, bits, (int32_t*)o.pairs.p, (uint8_t*)o.pmask.p, npart);
        }
    }
    if (nf > 0) {
        ix_launch_keep(s, npart, nf, keep, cnt);
        rd_scan_i32(s, r->tree.temp.p, r->tree.temp.bytes, keep, koff, nf);
        ix_launch_map(s, faces, nf, keep, koff, (int32_t*)o.fmap.p, nullptr);
    }
    if ((rc = rc_pass_end(o, 2, 3, 1, 0, IX_COUNTERS))) return rc;
    const unsigned long long* h = o.h_cnt;
    for (int k = 0; k < 4; k++) st.n_share[k] = (int64_t)h[IX_N_SHARE0 + k];
    st.n_pairs = (int64_t)h[IX_N_PAIRS]; st.n_pairs_share0 = (int64_t)h[IX_N_PAIRS_SHARE0]; st.n_pairs_share1 = (int64_t)h[IX_N_PAIRS_SHARE1];
    st.n_faces_hit = (int64_t)h[IX_N_FACES_HIT]; st.max_partners = (int64_t)h[IX_MAX_PARTNERS];
    o.have = true;
    if (stats) *stats = st;
    return 0;
}

int immesh_self_intersect_pairs(immesh_raycaster* r, int32_t* pairs, uint8_t* mask, int64_t cap, int64_t* n_out) {
    if (!r) return IMMESH_E_INVAL;
    immesh_ctx* c = r->ctx;
    int rc;
    if ((rc = ix_passed(r, "self_intersect_pairs"))) return rc;
    const RcIntersect& o = r->ix;
    const int64_t n = o.st.n_pairs;
    if ((rc = rc_cap(c, "self_intersect_pairs", cap, n, n_out, pairs || mask, "pairs"))) return rc;
    (void)hipSetDevice(c->cfg.device);
    if ((rc = rc_fetch(c, pairs, o.pairs.p, (size_t)n * 8))) return rc;
    return rc_fetch(c, mask, o.pmask.p, (size_t)n);
}

int immesh_self_intersect_faces(immesh_raycaster* r, int32_t* n_partners, int32_t* face_map_out) {
    if (!r) return IMMESH_E_INVAL;
    immesh_ctx* c = r->ctx;
    int rc;
    if ((rc = ix_passed(r, "self_intersect_faces"))) return rc;
    const RcIntersect& o = r->ix;
    (void)hipSetDevice(c->cfg.device);
    if ((rc = rc_fetch(c, n_partners, o.npart.p, (size_t)r->n_faces * 4))) return rc;
    return rc_fetch(c, face_map_out, o.fmap.p, (size_t)r->n_faces * 4);
}

int immesh_self_intersect_apply(immesh_raycaster* r) {
    if (!r) return IMMESH_E_INVAL;
    immesh_ctx* c = r->ctx;
    int rc;
    if ((rc = ix_passed(r, "self_intersect_apply"))) return rc;
    RcIntersect& o = r->ix;
    const int64_t nf = r->n_faces, n_kept = nf - o.st.n_faces_hit;
    (void)hipSetDevice(c->cfg.device);
    hipStream_t s = r->s;
    if (nf > 0 && (rc = ix_grow(r, o.faces_out, (size_t)nf * 12))) return rc;
    HIPCHK(c, hipEventRecord(o.ev[4], s));
    if (nf > 0) {
        ix_launch_map(s, (const int32_t*)r->faces.p, nf, (const int32_t*)o.keep.p, (const int32_t*)o.koff.p, nullptr, (int32_t*)o.faces_out.p);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipStreamSynchronize(s));                     // the buffers change places on an idle stream
        rc_swap(r->faces, o.faces_out);
    }
    if ((rc = rc_build(r, r->n_vtx, n_kept))) return rc;        // discards what read the snapshot, this pass too; the stream is idle on return
    return rc_pass_span(o, 4, 5, 2);
}

int immesh_self_intersect_last_timing(immesh_raycaster* r, float* ms) {
    if (!r || !ms) return IMMESH_E_INVAL;
    ms[0] = r->ix.ms[0]; ms[1] = r->ix.ms[1]; ms[2] = r->ix.ms[2];
    return 0;
}

}  // extern "C"
