// Host side of the one-ring table, the smoothing and the vertex normals (include/immesh_smooth.h): argument checks, grow-only buffers in the caster's
// RcSmooth record, the pass, its fetches and the apply on the caster's stream.  Nothing here is allocated or launched before the first immesh_smooth
// (the normals' incidence table: before the first immesh_vertex_normals).  The host knows n_vtx and n_faces, which bound every table (an entry per
// directed pair, a row per vertex), so no read-back lies between the launches; the counters come back once, at the end.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <string>
#include "../host_ctx.hpp"
#include "../../../include/immesh_smooth.h"
#include "smooth.hpp"
#include "../raycast/pass_dev.hpp"   // the run kernels of the one-ring

static_assert(sizeof(immesh_smooth_stats) == 12 * 8 && offsetof(immesh_smooth_stats, n_vertices) == 0 && offsetof(immesh_smooth_stats, n_used) == 8 &&
                  offsetof(immesh_smooth_stats, n_not_finite) == 16 && offsetof(immesh_smooth_stats, n_border) == 24 &&
                  offsetof(immesh_smooth_stats, n_interior) == 32 && offsetof(immesh_smooth_stats, n_moving) == 40 &&
                  offsetof(immesh_smooth_stats, n_pairs) == 48 && offsetof(immesh_smooth_stats, max_valence) == 56 &&
                  offsetof(immesh_smooth_stats, n_steps) == 64 && offsetof(immesh_smooth_stats, n_held) == 72 &&
                  offsetof(immesh_smooth_stats, n_moved) == 80 && offsetof(immesh_smooth_stats, max_disp2) == 88,
              "immesh_smooth_stats layout (immesh_amd/capi.py mirrors it)");

namespace {

constexpr int64_t SM_MAX_COUNT = 0x7FFFFFFE;                    // the sort's and the scan's int count

int sm_grow(immesh_raycaster* r, RcBuf& b, size_t bytes) { return rc_pass_grow(r->so, b, bytes); }

int sm_sizes(immesh_raycaster* r, const char* who) {
    if (6 * r->n_faces > SM_MAX_COUNT) { r->ctx->err = std::string(who) + ": more than 2^31 - 2 directed pairs (6 x " + std::to_string(r->n_faces) + " faces)"; return IMMESH_E_INVAL; }
    if (r->n_vtx > SM_MAX_COUNT) { r->ctx->err = std::string(who) + ": more than 2^31 - 2 vertices (" + std::to_string(r->n_vtx) + ")"; return IMMESH_E_INVAL; }
    return 0;
}

int sm_passed(immesh_raycaster* r, const char* who) {
    const int rc = rc_built(r, who);
    return rc ? rc : rc_passed(r, who, r->so, "no smooth pass since the caster's last build or apply (immesh_smooth)");
}

}  // namespace

extern "C" {

int immesh_smooth(immesh_raycaster* r, int32_t n_steps, double lambda, double mu, int32_t border, immesh_smooth_stats* stats) {
    if (!r) return IMMESH_E_INVAL;
    immesh_ctx* c = r->ctx;
    int rc;
    if ((rc = rc_built(r, "smooth"))) return rc;
    if (n_steps < 0 || n_steps > IMMESH_SMOOTH_MAX_STEPS) { c->err = "smooth: need 0 <= n_steps <= 65536, got " + std::to_string(n_steps); return IMMESH_E_INVAL; }
    if (!std::isfinite(lambda) || !std::isfinite(mu) || lambda < -1.0 || lambda > 1.0 || mu < -1.0 || mu > 1.0) {
        c->err = "smooth: need lambda and mu finite and in [-1, 1]";
        return IMMESH_E_INVAL;
    }
    if (border != IMMESH_SMOOTH_BORDER_FIXED && border != IMMESH_SMOOTH_BORDER_ALONG && border != IMMESH_SMOOTH_BORDER_FREE) {
        c->err = "smooth: unknown border rule " + std::to_string(border);
        return IMMESH_E_INVAL;
    }
    if ((rc = sm_sizes(r, "smooth"))) return rc;
    const int64_t nv = r->n_vtx, nf = r->n_faces, n6 = 6 * nf;
    (void)hipSetDevice(c->cfg.device);
    hipStream_t s = r->s;
    RcSmooth& o = r->so;
    o.have = false;
    if ((rc = rc_pass_ready(c, s, "smooth", o, SM_COUNTERS, SM_COUNTERS))) return rc;
    unsigned long long* cnt = (unsigned long long*)o.cnt.p;
    const bool ring = nf > 0 && nv > 0;
    if (nv > 0) {
        if ((rc = sm_grow(r, o.row_start, (size_t)(nv + 1) * 8))) return rc;
        if ((rc = sm_grow(r, o.vclass, (size_t)nv))) return rc;
        if ((rc = sm_grow(r, o.flag, (size_t)nv * SM_FLAGS))) return rc;
        for (RcBuf& b : o.pos)
            if ((rc = sm_grow(r, b, (size_t)nv * 12))) return rc;
    }
    if (ring) {
        if ((rc = sm_grow(r, o.key_a, (size_t)n6 * 8))) return rc;
        if ((rc = sm_grow(r, o.key_b, (size_t)n6 * 8))) return rc;
        if ((rc = sm_grow(r, o.rstart, (size_t)(n6 + 1) * 4))) return rc;
        RcBuf* const per_pair[] = {&o.val_a, &o.val_b, &o.neighbours, &o.uses, &o.sn};
        for (RcBuf* b : per_pair)
            if ((rc = sm_grow(r, *b, (size_t)n6 * 4))) return rc;
        const size_t temp = std::max(exclusive_sum_temp_bytes((int)n6), sort_pairs_u64_temp_bytes((int)n6)) + 256;
        if ((rc = sm_grow(r, r->tree.temp, temp))) return rc;   // the caster's scan and sort scratch
    }
    const float* vtx = (const float*)r->vtx.p;
    if ((rc = rc_pass_begin(o, 0))) return rc;
    if (nv > 0) {
        HIPCHK(c, hipMemsetAsync(o.flag.p, 0, (size_t)nv * SM_FLAGS, s));
        if (!ring) {                                            // no face: every vertex is unused and every row empty
            HIPCHK(c, hipMemsetAsync(o.row_start.p, 0, (size_t)(nv + 1) * 8, s));
            HIPCHK(c, hipMemsetAsync(o.vclass.p, 0, (size_t)nv, s));
        }
    }
    if (ring) {
        void* temp = r->tree.temp.p;
        const size_t temp_bytes = r->tree.temp.bytes;
        unsigned long long *key_a = (unsigned long long*)o.key_a.p, *key_b = (unsigned long long*)o.key_b.p;
        int32_t *rstart = (int32_t*)o.rstart.p, *neighbours = (int32_t*)o.neighbours.p, *uses = (int32_t*)o.uses.p;
        int8_t *flag = (int8_t*)o.flag.p, *vclass = (int8_t*)o.vclass.p;
        sm_launch_emit(s, (const int32_t*)r->faces.p, nf, nv, key_a, (int32_t*)o.val_a.p);
        sort_pairs_u64(s, temp, temp_bytes, key_a, key_b, (const int32_t*)o.val_a.p, (int32_t*)o.val_b.p, (int)n6, 32 + rc_index_bits(nv + 1));
        int32_t *head = (int32_t*)key_a, *scan = head + n6;     // the unsorted keys are done with: the heads and their scan lie in them
        pd_launch_run_heads(s, key_b, n6, head);
        exclusive_sum_i32(s, temp, temp_bytes, head, scan, (int)n6);
        pd_launch_run_starts(s, n6, head, scan, rstart, n6 + 1);
        sm_launch_entries(s, key_b, n6, nv, head, scan, rstart, neighbours, uses, flag);
        sm_launch_rows(s, vtx, nv, key_b, n6, head, scan, flag, (long long*)o.row_start.p, vclass, cnt);
        sm_launch_lists(s, key_b, n6, nv, head, scan, rstart, neighbours, uses, vclass, border, (int32_t*)o.sn.p, flag);
    }
    HIPCHK(c, hipEventRecord(o.ev[1], s));
    HIPCHK(c, hipEventRecord(o.ev[2], s));
    o.cur = 0;
    if (nv > 0) {
        if (n_steps == 0 || !ring) {                            // nothing moves: the snapshot bit for bit
            HIPCHK(c, hipMemcpyAsync(o.pos[0].p, vtx, (size_t)nv * 12, hipMemcpyDeviceToDevice, s));
        } else {
            const float* p_in = vtx;
            for (int32_t j = 0; j < n_steps; j++) {
                float* p_out = (float*)o.pos[j & 1].p;
                sm_launch_step(s, p_in, p_out, nv, (const long long*)o.row_start.p, (const int32_t*)o.sn.p, n6, (j & 1) ? mu : lambda, cnt);
                p_in = p_out;
            }
            o.cur = (n_steps - 1) & 1;
        }
        sm_launch_finish(s, vtx, (const float*)o.pos[o.cur].p, nv, (const int8_t*)o.flag.p, cnt);
    }
    if ((rc = rc_pass_end(o, 2, 3, 1, 0, SM_COUNTERS))) return rc;   // the one read-back; it ends both spans
    (void)hipEventElapsedTime(&o.ms[0], o.ev[0], o.ev[1]);
    const unsigned long long* h = o.h_cnt;
    immesh_smooth_stats& st = o.st;
    st.n_vertices = nv; st.n_used = (int64_t)h[SM_N_USED]; st.n_not_finite = (int64_t)h[SM_N_NOT_FINITE]; st.n_border = (int64_t)h[SM_N_BORDER];
    st.n_interior = (int64_t)h[SM_N_INTERIOR]; st.n_moving = (int64_t)h[SM_N_MOVING]; st.n_pairs = (int64_t)h[SM_N_PAIRS];
    st.max_valence = (int64_t)h[SM_MAX_VALENCE]; st.n_steps = n_steps; st.n_held = (int64_t)h[SM_N_HELD]; st.n_moved = (int64_t)h[SM_N_MOVED];
    std::memcpy(&st.max_disp2, &h[SM_MAX_DISP2], 8);
    o.have = true;
    if (stats) *stats = st;
    return 0;
}

int immesh_smooth_vertices(immesh_raycaster* r, float* vtx_out, int8_t* vclass) {
    if (!r) return IMMESH_E_INVAL;
    immesh_ctx* c = r->ctx;
    int rc;
    if ((rc = sm_passed(r, "smooth_vertices"))) return rc;
    const RcSmooth& o = r->so;
    const int64_t nv = r->n_vtx;
    if (nv == 0) return 0;
    (void)hipSetDevice(c->cfg.device);
    if ((rc = rc_fetch(c, vtx_out, o.pos[o.cur].p, (size_t)nv * 12))) return rc;
    return rc_fetch(c, vclass, o.vclass.p, (size_t)nv);
}

int immesh_smooth_adjacency(immesh_raycaster* r, int64_t* row_start, int32_t* neighbours, int32_t* uses, int64_t cap, int64_t* n_out) {
    if (!r) return IMMESH_E_INVAL;
    immesh_ctx* c = r->ctx;
    int rc;
    if ((rc = sm_passed(r, "smooth_adjacency"))) return rc;
    const RcSmooth& o = r->so;
    const int64_t n = o.st.n_pairs, nv = r->n_vtx;
    if ((rc = rc_cap(c, "smooth_adjacency", cap, n, n_out, row_start || neighbours || uses, "entries"))) return rc;
    (void)hipSetDevice(c->cfg.device);
    if (row_start && nv == 0) row_start[0] = 0;
    else if ((rc = rc_fetch(c, row_start, o.row_start.p, (size_t)(nv + 1) * 8))) return rc;
    if ((rc = rc_fetch(c, neighbours, o.neighbours.p, (size_t)n * 4))) return rc;
    return rc_fetch(c, uses, o.uses.p, (size_t)n * 4);
}

int immesh_smooth_apply(immesh_raycaster* r) {
    if (!r) return IMMESH_E_INVAL;
    immesh_ctx* c = r->ctx;
    int rc;
    if ((rc = sm_passed(r, "smooth_apply"))) return rc;
    RcSmooth& o = r->so;
    const int64_t nv = r->n_vtx, nf = r->n_faces;
    (void)hipSetDevice(c->cfg.device);
    hipStream_t s = r->s;
    HIPCHK(c, hipEventRecord(o.ev[4], s));
    if (nv > 0) {                                               // (no vertex: nothing was launched and the result's buffers may not exist)
        rc_swap(r->vtx, o.pos[o.cur]);                          // the stream is idle: the pass synchronised
    }
    if ((rc = rc_build(r, nv, nf))) return rc;                  // discards what read the snapshot, this pass too; the stream is idle on return
    return rc_pass_span(o, 4, 5, 2);
}

int immesh_smooth_last_timing(immesh_raycaster* r, float* ms) {
    if (!r || !ms) return IMMESH_E_INVAL;
    ms[0] = r->so.ms[0]; ms[1] = r->so.ms[1]; ms[2] = r->so.ms[2];
    return 0;
}

int immesh_vertex_normals(immesh_raycaster* r, float* normals_out, int64_t* n_zero) {
    if (!r) return IMMESH_E_INVAL;
    immesh_ctx* c = r->ctx;
    int rc;
    if ((rc = rc_built(r, "vertex_normals"))) return rc;
    if ((rc = sm_sizes(r, "vertex_normals"))) return rc;
    const int64_t nv = r->n_vtx, nf = r->n_faces, n3 = 3 * nf;
    if (n_zero) *n_zero = 0;
    if (nv == 0) return 0;
    (void)hipSetDevice(c->cfg.device);
    hipStream_t s = r->s;
    RcSmooth& o = r->so;
    if ((rc = rc_pass_ready(c, s, "smooth", o, SM_COUNTERS, SM_COUNTERS))) return rc;
    if ((rc = sm_grow(r, o.normals, (size_t)nv * 12))) return rc;
    if (nf > 0) {
        RcBuf* const per_corner[] = {&o.nkey_a, &o.nkey_b, &o.nval_a, &o.nval_b};
        for (RcBuf* b : per_corner)
            if ((rc = sm_grow(r, *b, (size_t)n3 * 4))) return rc;
        if ((rc = sm_grow(r, r->tree.temp, sort_pairs_u32_temp_bytes((int)n3) + 256))) return rc;   // the caster's sort scratch
    }
    unsigned long long* cnt = (unsigned long long*)o.cnt.p;     // (the pass' other counters are on the host since its end)
    HIPCHK(c, hipMemsetAsync(cnt + SM_N_ZERO, 0, 8, s));
    if (nf > 0) {
        sm_launch_incidence(s, (const float*)r->vtx.p, nv, (const int32_t*)r->faces.p, nf, (uint32_t*)o.nkey_a.p, (int32_t*)o.nval_a.p);
        sort_pairs_u32(s, r->tree.temp.p, r->tree.temp.bytes, (const uint32_t*)o.nkey_a.p, (uint32_t*)o.nkey_b.p, (const int32_t*)o.nval_a.p, (int32_t*)o.nval_b.p,
                       (int)n3, rc_index_bits(nv + 1));         // stable: the faces of a vertex stay in ascending order
    }
    sm_launch_normals(s, (const float*)r->vtx.p, nv, (const int32_t*)r->faces.p, nf, (const uint32_t*)o.nkey_b.p, (const int32_t*)o.nval_b.p, (float*)o.normals.p,
                      cnt);
    HIPCHK(c, hipMemcpyAsync(o.h_cnt + SM_N_ZERO, cnt + SM_N_ZERO, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(s));
    if (n_zero) *n_zero = (int64_t)o.h_cnt[SM_N_ZERO];
    return rc_fetch(c, normals_out, o.normals.p, (size_t)nv * 12);
}

}  // extern "C"
