// Host side of the holes (include/immesh_topology.h, the Holes rule): argument checks, grow-only buffers in the caster's RcHoles record, the pass, its
// fetches and the apply on the caster's stream.  Nothing here is allocated or launched before the first immesh_topology_holes.  It reads what the
// analysis left on the device: the sorted half-edges, the boundary vertices' union-find and the loops' edge counts.  The host already has every
// number that sizes a buffer or a launch (n_boundary_loops the tables, n_boundary the cycle slots, largest_loop_edges the ranking's rounds), so no
// read-back lies between the launches; the counters come back once, at the end.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <string>
#include "../host_ctx.hpp"
#include "../../../include/immesh_topology.h"
#include "topology.hpp"

static_assert(sizeof(immesh_holes_stats) == 12 * 8 && offsetof(immesh_holes_stats, n_loops) == 0 && offsetof(immesh_holes_stats, n_simple) == 8 &&
                  offsetof(immesh_holes_stats, n_nonsimple) == 16 && offsetof(immesh_holes_stats, n_outline) == 24 &&
                  offsetof(immesh_holes_stats, n_too_long) == 32 && offsetof(immesh_holes_stats, n_too_wide) == 40 &&
                  offsetof(immesh_holes_stats, n_blocked) == 48 && offsetof(immesh_holes_stats, n_filled) == 56 &&
                  offsetof(immesh_holes_stats, n_new_faces) == 64 && offsetof(immesh_holes_stats, n_edges_closed) == 72 &&
                  offsetof(immesh_holes_stats, largest_simple_loop_edges) == 80 && offsetof(immesh_holes_stats, n_cycle_vertices) == 88,
              "immesh_holes_stats layout (immesh_amd/capi.py mirrors it)");
static_assert(sizeof(HlRank) == 8, "HlRank layout");

namespace {

constexpr int64_t HL_MAX_VTX = 0x7FFFFFFF;                      // the scan's int count
constexpr int64_t HL_MAX_FACES = (int64_t)1 << RC_INDEX_BITS;   // what a build takes
constexpr int64_t HL_MAX_ANALYSED = ((int64_t)0x7FFFFFFE) / 3;  // what an analysis takes

int hl_grow(immesh_raycaster* r, RcBuf& b, size_t bytes) { return rc_pass_grow(r->hl, b, bytes); }

int hl_passed(immesh_raycaster* r, const char* who) {
    const int rc = rc_analysed(r, who);
    return rc ? rc : rc_passed(r, who, r->hl, "no holes pass since the last analysis (immesh_topology_holes)");
}

}  // namespace

extern "C" {

int immesh_topology_holes(immesh_raycaster* r, int64_t max_edges, double max_diagonal, immesh_holes_stats* stats) {
    if (!r) return IMMESH_E_INVAL;
    immesh_ctx* c = r->ctx;
    int rc;
    if ((rc = rc_analysed(r, "topology_holes"))) return rc;
    if (max_edges < 3) { c->err = "topology_holes: max_edges " + std::to_string(max_edges) + " is below 3"; return IMMESH_E_INVAL; }
    if (!(max_diagonal >= 0.0) || !std::isfinite(max_diagonal)) { c->err = "topology_holes: need 0 <= max_diagonal, finite"; return IMMESH_E_INVAL; }
    if (r->n_vtx > HL_MAX_VTX) { c->err = "topology_holes: more than 2^31 - 1 vertices (" + std::to_string(r->n_vtx) + ")"; return IMMESH_E_INVAL; }
    (void)hipSetDevice(c->cfg.device);
    hipStream_t s = r->s;
    const RcTopology& q = r->tp;
    RcHoles& o = r->hl;
    const int64_t nv = r->n_vtx, n_half = q.n_half, n_loops = q.st.n_boundary_loops, n_room = q.st.n_boundary, largest = q.st.largest_loop_edges;
    o.have = false;
    if ((rc = rc_pass_ready(c, s, "topology_holes", o, HC_COUNTERS, HC_COUNTERS))) return rc;
    unsigned long long* cnt = (unsigned long long*)o.cnt.p;
    if (n_loops > 0) {
        if ((rc = hl_grow(r, o.vt, (size_t)nv * HV_TABLES * 4))) return rc;
        if ((rc = hl_grow(r, o.rk_a, (size_t)nv * sizeof(HlRank)))) return rc;
        if ((rc = hl_grow(r, o.rk_b, (size_t)nv * sizeof(HlRank)))) return rc;
        if ((rc = hl_grow(r, o.lt, (size_t)n_loops * HL_TABLES * 4))) return rc;
        if ((rc = hl_grow(r, o.box, (size_t)n_loops * 24))) return rc;
        if ((rc = hl_grow(r, o.cstart, (size_t)n_loops * 8))) return rc;
        if ((rc = hl_grow(r, o.cycle, (size_t)n_room * 4))) return rc;
        if ((rc = hl_grow(r, o.cloop, (size_t)n_room * 4))) return rc;
        if ((rc = hl_grow(r, o.new_faces, (size_t)n_room * 12))) return rc;
        if ((rc = hl_grow(r, o.new_loop, (size_t)n_room * 4))) return rc;
        if ((rc = hl_grow(r, r->tree.temp, exclusive_sum_temp_bytes((int)std::max(nv, n_loops)) + 256))) return rc;   // the caster's scan scratch
    }
    if ((rc = rc_pass_begin(o, 0))) return rc;
    if (n_loops > 0) {
        const unsigned long long* key = (const unsigned long long*)q.key_b.p;
        int32_t *vt = (int32_t*)o.vt.p, *lt = (int32_t*)o.lt.p, *cycle = (int32_t*)o.cycle.p, *cloop = (int32_t*)o.cloop.p;
        uint32_t* box = (uint32_t*)o.box.p;
        HlRank* rk[2] = {(HlRank*)o.rk_a.p, (HlRank*)o.rk_b.p};
        hl_launch_init(s, nv, (const int32_t*)q.vparent.p, vt);
        hl_launch_degrees(s, key, (const int32_t*)q.val_b.p, n_half, (const int32_t*)r->faces.p, nv, vt);
        hl_launch_flags(s, nv, vt);
        exclusive_sum_i32(s, r->tree.temp.p, r->tree.temp.bytes, vt + HV_ROOT * nv, vt + HV_NUM * nv, (int)nv);
        hl_launch_rank_init(s, nv, vt, (const int32_t*)q.loop_cnt.p, n_loops, lt, box, rk[0]);
        int rounds = 0;
        while (((int64_t)1 << rounds) < largest) rounds++;      // a list of n vertices is ranked when the pointers span n - 1
        for (int i = 0; i < rounds; i++) hl_launch_jump(s, nv, rk[i & 1], rk[(i + 1) & 1]);
        hl_launch_boxes(s, (const float*)r->vtx.p, nv, vt, n_loops, box);
        exclusive_sum_i32(s, r->tree.temp.p, r->tree.temp.bytes, lt + HL_SLEN * n_loops, lt + HL_CSTART * n_loops, (int)n_loops);
        hl_launch_scatter(s, nv, vt, rk[rounds & 1], lt, n_loops, cycle, cloop, n_room);
        hl_launch_limits(s, n_loops, lt, box, max_edges, max_diagonal, (int64_t*)o.cstart.p, cnt);
        hl_launch_chords(s, n_room, cnt, cycle, cloop, key, n_half, lt, n_loops);
        hl_launch_decide(s, n_loops, lt, cnt);
        exclusive_sum_i32(s, r->tree.temp.p, r->tree.temp.bytes, lt + HL_FILL * n_loops, lt + HL_FOFF * n_loops, (int)n_loops);
        hl_launch_emit(s, n_room, cycle, cloop, lt, n_loops, (int32_t*)o.new_faces.p, (int32_t*)o.new_loop.p, cnt);
    }
    if ((rc = rc_pass_end(o, 0, 1, 0, 0, HC_COUNTERS))) return rc;   // the one read-back
    const unsigned long long* h = o.h_cnt;
    immesh_holes_stats& st = o.st;
    st.n_loops = n_loops; st.n_simple = (int64_t)h[HC_N_SIMPLE]; st.n_nonsimple = (int64_t)h[HC_N_NONSIMPLE];
    st.n_outline = (int64_t)h[HC_N_OUTLINE]; st.n_too_long = (int64_t)h[HC_N_TOO_LONG]; st.n_too_wide = (int64_t)h[HC_N_TOO_WIDE];
    st.n_blocked = (int64_t)h[HC_N_BLOCKED]; st.n_filled = (int64_t)h[HC_N_FILLED]; st.n_new_faces = (int64_t)h[HC_N_NEW];
    st.n_edges_closed = (int64_t)h[HC_N_CLOSED]; st.largest_simple_loop_edges = (int64_t)h[HC_LARGEST_SIMPLE]; st.n_cycle_vertices = (int64_t)h[HC_N_CYCLE];
    o.n_loops = n_loops;
    o.have = true;
    if (stats) *stats = st;
    return 0;
}

int immesh_topology_holes_loops(immesh_raycaster* r, int32_t* first_vertex, int32_t* n_edges, int32_t* status, float* box, int64_t* cycle_start, int64_t cap,
                                int64_t* n_out) {
    if (!r) return IMMESH_E_INVAL;
    immesh_ctx* c = r->ctx;
    int rc;
    if ((rc = hl_passed(r, "topology_holes_loops"))) return rc;
    const RcHoles& o = r->hl;
    const int64_t n = o.n_loops;
    const bool wanted = first_vertex || n_edges || status || box || cycle_start;
    if ((rc = rc_cap(c, "topology_holes_loops", cap, n, n_out, wanted, "loops"))) return rc;
    if (!wanted || n == 0) return 0;
    (void)hipSetDevice(c->cfg.device);
    const int32_t* lt = (const int32_t*)o.lt.p;
    int32_t* const out[3] = {first_vertex, n_edges, status};
    const int which[3] = {HL_FIRST, HL_NEDGES, HL_STATUS};
    for (int k = 0; k < 3; k++)
        if ((rc = rc_fetch(c, out[k], lt + which[k] * n, (size_t)n * 4))) return rc;
    if (box && (rc = tp_fetch_boxes(c, box, o.box, n))) return rc;
    return rc_fetch(c, cycle_start, o.cstart.p, (size_t)n * 8);
}

int immesh_topology_holes_cycles(immesh_raycaster* r, int32_t* cycle_out, int64_t cap, int64_t* n_out) {
    if (!r) return IMMESH_E_INVAL;
    immesh_ctx* c = r->ctx;
    int rc;
    if ((rc = hl_passed(r, "topology_holes_cycles"))) return rc;
    const int64_t n = r->hl.st.n_cycle_vertices;
    if ((rc = rc_cap(c, "topology_holes_cycles", cap, n, n_out, cycle_out != nullptr, "cycle vertices"))) return rc;
    (void)hipSetDevice(c->cfg.device);
    return rc_fetch(c, cycle_out, r->hl.cycle.p, (size_t)n * 4);
}

int immesh_topology_holes_faces(immesh_raycaster* r, int32_t* loop_out, int32_t* faces_out, int64_t cap, int64_t* n_out) {
    if (!r) return IMMESH_E_INVAL;
    immesh_ctx* c = r->ctx;
    int rc;
    if ((rc = hl_passed(r, "topology_holes_faces"))) return rc;
    const int64_t n = r->hl.st.n_new_faces;
    if ((rc = rc_cap(c, "topology_holes_faces", cap, n, n_out, loop_out || faces_out, "new faces"))) return rc;
    (void)hipSetDevice(c->cfg.device);
    if ((rc = rc_fetch(c, loop_out, r->hl.new_loop.p, (size_t)n * 4))) return rc;
    return rc_fetch(c, faces_out, r->hl.new_faces.p, (size_t)n * 12);
}

int immesh_topology_holes_apply(immesh_raycaster* r) {
    if (!r) return IMMESH_E_INVAL;
    immesh_ctx* c = r->ctx;
    int rc;
    if ((rc = hl_passed(r, "topology_holes_apply"))) return rc;
    RcHoles& o = r->hl;
    const int64_t nf = r->n_faces, n_new = o.st.n_new_faces, total = nf + n_new;
    if (total > HL_MAX_FACES || total > HL_MAX_ANALYSED) {
        c->err = "topology_holes_apply: " + std::to_string(nf) + " faces and " + std::to_string(n_new) + " new ones exceed 2^30 faces or 2^31 - 2 half-edges";
        return IMMESH_E_INVAL;
    }
    (void)hipSetDevice(c->cfg.device);
    hipStream_t s = r->s;
    if ((rc = hl_grow(r, o.merged, (size_t)total * 12))) return rc;
    HIPCHK(c, hipEventRecord(o.ev[2], s));
    if (nf > 0) HIPCHK(c, hipMemcpyAsync(o.merged.p, r->faces.p, (size_t)nf * 12, hipMemcpyDeviceToDevice, s));
    if (n_new > 0) HIPCHK(c, hipMemcpyAsync((int32_t*)o.merged.p + 3 * nf, o.new_faces.p, (size_t)n_new * 12, hipMemcpyDeviceToDevice, s));
    rc_swap(r->faces, o.merged);                                // the stream runs in order: the copies are queued before the build reads them
    if ((rc = rc_build(r, r->n_vtx, total))) return rc;         // discards what read the snapshot, this pass too; the stream is idle on return
    return rc_pass_span(o, 2, 3, 1);
}

int immesh_topology_holes_last_timing(immesh_raycaster* r, float* ms) {
    if (!r || !ms) return IMMESH_E_INVAL;
    ms[0] = r->hl.ms[0]; ms[1] = r->hl.ms[1];
    return 0;
}

}  // extern "C"
