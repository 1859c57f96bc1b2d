// Host side of the mesh topology (include/immesh_topology.h): argument checks, grow-only buffers in the caster's RcTopology record, the analysis, the
// fetches and the selection on the caster's stream.  Nothing here is allocated or launched before the first immesh_topology_analyse.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <string>
#include <vector>
#include "../host_ctx.hpp"
#include "../../../include/immesh_topology.h"
#include "topology.hpp"
#include "../raycast/pass_dev.hpp"   // the run kernels of the edge lists

static_assert(sizeof(immesh_topology_stats) == 14 * 8 && offsetof(immesh_topology_stats, n_faces) == 0 && offsetof(immesh_topology_stats, n_counting) == 8 &&
                  offsetof(immesh_topology_stats, n_degenerate) == 16 && offsetof(immesh_topology_stats, n_vertices_used) == 24 &&
                  offsetof(immesh_topology_stats, n_edges) == 32 && offsetof(immesh_topology_stats, n_boundary) == 40 &&
                  offsetof(immesh_topology_stats, n_interior) == 48 && offsetof(immesh_topology_stats, n_nonmanifold) == 56 &&
                  offsetof(immesh_topology_stats, n_inconsistent) == 64 && offsetof(immesh_topology_stats, n_components) == 72 &&
                  offsetof(immesh_topology_stats, largest_component_faces) == 80 && offsetof(immesh_topology_stats, n_boundary_loops) == 88 &&
                  offsetof(immesh_topology_stats, largest_loop_edges) == 96 && offsetof(immesh_topology_stats, euler) == 104,
              "immesh_topology_stats layout (immesh_amd/capi.py mirrors it)");

namespace {

constexpr int64_t TP_MAX_FACES = ((int64_t)0x7FFFFFFE) / 3;   // 3 n_faces <= 2^31 - 2: the sort's int count, the half-edge id

int tp_grow(immesh_raycaster* r, RcBuf& b, size_t bytes) { return rc_pass_grow(r->tp, b, bytes); }

// scan and sort scratch: the caster's (the reinforce pass and the sampler share it too)
int tp_temp(immesh_raycaster* r, int64_t n_scan, int64_t n_sort) {
    const size_t need = std::max(exclusive_sum_temp_bytes((int)std::max<int64_t>(n_scan, 1)), sort_pairs_u64_temp_bytes((int)std::max<int64_t>(n_sort, 1))) + 256;
    return tp_grow(r, r->tree.temp, need);
}

}  // namespace

int tp_fetch_boxes(immesh_ctx* c, float* box, const RcBuf& keys, int64_t n) {
    std::vector<uint32_t> k((size_t)n * 6);
    HIPCHK(c, hipMemcpy(k.data(), keys.p, (size_t)n * 24, hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < 6 * n; i++) box[i] = tp_unkey_host(k[(size_t)i], i % 6 < 3);
    return 0;
}

extern "C" {

int immesh_topology_analyse(immesh_raycaster* r, immesh_topology_stats* stats) {
    if (!r) return IMMESH_E_INVAL;
    immesh_ctx* c = r->ctx;
    RcTopology& q = r->tp;
    int rc;
    if ((rc = rc_built(r, "topology_analyse"))) return rc;
    const int64_t nf = r->n_faces, nv = r->n_vtx;
    if (nf > TP_MAX_FACES) { c->err = "topology_analyse: 3 n_faces exceeds 2^31 - 2 (" + std::to_string(nf) + " faces)"; return IMMESH_E_INVAL; }
    (void)hipSetDevice(c->cfg.device);
    hipStream_t s = r->s;
    q.have = false;
    rc_analysis_changed(r);
    if ((rc = rc_pass_ready(c, s, "topology", q, TP_COUNTERS, TP_COUNTERS + 2))) return rc;
    if ((rc = tp_grow(r, q.flag, (size_t)nf * 4))) return rc;
    if ((rc = tp_grow(r, q.off, (size_t)nf * 4))) return rc;
    if ((rc = tp_grow(r, q.parent, (size_t)nf * 4))) return rc;
    if ((rc = tp_grow(r, q.label, (size_t)nf * 4))) return rc;
    if ((rc = tp_grow(r, q.root, (size_t)nf * 4))) return rc;
    if ((rc = tp_grow(r, q.num, (size_t)nf * 4))) return rc;
    if ((rc = tp_grow(r, q.comp, (size_t)nf * 4))) return rc;
    if ((rc = tp_grow(r, q.used, (size_t)nv * 4))) return rc;
    if ((rc = tp_grow(r, q.vparent, (size_t)nv * 4))) return rc;
    if ((rc = tp_grow(r, q.loop_cnt, (size_t)nv * 4))) return rc;
    if ((rc = tp_temp(r, nf, 3 * nf))) return rc;
    const int32_t* faces = (const int32_t*)r->faces.p;
    int32_t *flag = (int32_t*)q.flag.p, *off = (int32_t*)q.off.p, *parent = (int32_t*)q.parent.p, *vparent = (int32_t*)q.vparent.p;
    unsigned long long* cnt = (unsigned long long*)q.cnt.p;
    unsigned long long* h = q.h_cnt;
    if ((rc = rc_pass_begin(q, 0))) return rc;
    int64_t n_counting = 0;
    if (nf > 0) {
        if (nv > 0) HIPCHK(c, hipMemsetAsync(q.used.p, 0, (size_t)nv * 4, s));
        tp_launch_mark(s, faces, nf, nv, flag, parent, (int32_t*)q.used.p);
        exclusive_sum_i32(s, r->tree.temp.p, r->tree.temp.bytes, flag, off, (int)nf);
        h[TP_COUNTERS] = h[TP_COUNTERS + 1] = 0;
        HIPCHK(c, hipMemcpyAsync(&h[TP_COUNTERS], off + (nf - 1), 4, hipMemcpyDeviceToHost, s));     // the one count the host needs: it sizes the
        HIPCHK(c, hipMemcpyAsync(&h[TP_COUNTERS + 1], flag + (nf - 1), 4, hipMemcpyDeviceToHost, s));  // half-edge and the component tables
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipStreamSynchronize(s));
        n_counting = (int64_t)h[TP_COUNTERS] + (int64_t)h[TP_COUNTERS + 1];
    }
    const int64_t n_half = 3 * n_counting;
    if (n_counting > 0) {
        if ((rc = tp_grow(r, q.key_a, (size_t)n_half * 8))) return rc;
        if ((rc = tp_grow(r, q.key_b, (size_t)n_half * 8))) return rc;
        if ((rc = tp_grow(r, q.val_a, (size_t)n_half * 4))) return rc;
        if ((rc = tp_grow(r, q.val_b, (size_t)n_half * 4))) return rc;
        if ((rc = tp_grow(r, q.first, (size_t)n_counting * 4))) return rc;
        if ((rc = tp_grow(r, q.nfaces, (size_t)n_counting * 4))) return rc;
        if ((rc = tp_grow(r, q.nbound, (size_t)n_counting * 4))) return rc;
        if ((rc = tp_grow(r, q.box, (size_t)n_counting * 24))) return rc;
        unsigned long long *key_a = (unsigned long long*)q.key_a.p, *key_b = (unsigned long long*)q.key_b.p;
        int32_t *val_a = (int32_t*)q.val_a.p, *val_b = (int32_t*)q.val_b.p;
        tp_launch_vertices(s, nv, (const int32_t*)q.used.p, vparent, (int32_t*)q.loop_cnt.p, cnt);
        tp_launch_emit(s, faces, nf, flag, off, key_a, val_a);
        sort_pairs_u64(s, r->tree.temp.p, r->tree.temp.bytes, key_a, key_b, val_a, val_b, (int)n_half, 32 + rc_index_bits(nv));
        tp_launch_classify(s, key_b, val_b, n_half, faces, parent, vparent, cnt);
    }
    if (nf > 0) {
        int32_t *label = (int32_t*)q.label.p, *root = (int32_t*)q.root.p, *num = (int32_t*)q.num.p, *comp = (int32_t*)q.comp.p;
        tp_launch_flatten(s, parent, flag, nf, label, root);
        exclusive_sum_i32(s, r->tree.temp.p, r->tree.temp.bytes, root, num, (int)nf);
        tp_launch_preset(s, n_counting, (int32_t*)q.nfaces.p, (int32_t*)q.nbound.p, (uint32_t*)q.box.p);
        tp_launch_components(s, (const float*)r->vtx.p, nv, faces, nf, label, root, num, comp, (int32_t*)q.first.p, (int32_t*)q.nfaces.p, (uint32_t*)q.box.p, cnt);
        if (n_counting > 0) {
            tp_launch_boundary(s, (const unsigned long long*)q.key_b.p, (const int32_t*)q.val_b.p, n_half, comp, vparent, (int32_t*)q.nbound.p,
                               (int32_t*)q.loop_cnt.p, cnt);
            tp_launch_largest(s, root, num, (const int32_t*)q.nfaces.p, nf, cnt);
        }
    }
    if ((rc = rc_pass_end(q, 0, 1, 0, 0, TP_COUNTERS))) return rc;
    if (h[TP_ERROR]) {
        c->err = "topology_analyse: a union did not finish within its step bound (a defect of the library)";
        return IMMESH_E_INTERNAL;
    }
    immesh_topology_stats& st = q.st;
    st.n_faces = nf; st.n_counting = n_counting; st.n_degenerate = nf - n_counting;
    st.n_vertices_used = (int64_t)h[TP_N_VERTICES]; st.n_edges = (int64_t)h[TP_N_EDGES];
    st.n_boundary = (int64_t)h[TP_N_BOUNDARY]; st.n_interior = (int64_t)h[TP_N_INTERIOR]; st.n_nonmanifold = (int64_t)h[TP_N_NONMANIFOLD];
    st.n_inconsistent = (int64_t)h[TP_N_INCONSISTENT];
    st.n_components = (int64_t)h[TP_N_COMPONENTS]; st.largest_component_faces = (int64_t)h[TP_LARGEST_COMPONENT];
    st.n_boundary_loops = (int64_t)h[TP_N_LOOPS]; st.largest_loop_edges = (int64_t)h[TP_LARGEST_LOOP];
    st.euler = st.n_vertices_used - st.n_edges + n_counting;
    q.n_counting = n_counting; q.n_half = n_half;
    q.have = true;
    if (stats) *stats = st;
    return 0;
}

int immesh_topology_faces(immesh_raycaster* r, int32_t* comp_out) {
    if (!r) return IMMESH_E_INVAL;
    immesh_ctx* c = r->ctx;
    int rc;
    if ((rc = rc_analysed(r, "topology_faces"))) return rc;
    (void)hipSetDevice(c->cfg.device);
    return rc_fetch(c, comp_out, r->tp.comp.p, (size_t)r->n_faces * 4);
}

int immesh_topology_components(immesh_raycaster* r, int32_t* first_face, int32_t* n_faces, int32_t* n_boundary, float* box, int64_t cap, int64_t* n_out) {
    if (!r) return IMMESH_E_INVAL;
    immesh_ctx* c = r->ctx;
    int rc;
    if ((rc = rc_analysed(r, "topology_components"))) return rc;
    const RcTopology& q = r->tp;
    const int64_t n = q.st.n_components;
    const bool wanted = first_face || n_faces || n_boundary || box;
    if ((rc = rc_cap(c, "topology_components", cap, n, n_out, wanted, "components"))) return rc;
    if (!wanted || n == 0) return 0;
    (void)hipSetDevice(c->cfg.device);
    if ((rc = rc_fetch(c, first_face, q.first.p, (size_t)n * 4))) return rc;
    if ((rc = rc_fetch(c, n_faces, q.nfaces.p, (size_t)n * 4))) return rc;
    if ((rc = rc_fetch(c, n_boundary, q.nbound.p, (size_t)n * 4))) return rc;
    return box ? tp_fetch_boxes(c, box, q.box, n) : 0;
}

int immesh_topology_edges(immesh_raycaster* r, int32_t kind, int32_t* uv, int32_t* uses, int64_t cap, int64_t* n_out) {
    if (!r) return IMMESH_E_INVAL;
    immesh_ctx* c = r->ctx;
    int rc;
    if ((rc = rc_analysed(r, "topology_edges"))) return rc;
    if (kind != IMMESH_EDGE_BOUNDARY && kind != IMMESH_EDGE_NONMANIFOLD && kind != IMMESH_EDGE_INCONSISTENT) {
        c->err = "topology_edges: unknown kind " + std::to_string(kind);
        return IMMESH_E_INVAL;
    }
    RcTopology& q = r->tp;
    const int64_t n = kind == IMMESH_EDGE_BOUNDARY ? q.st.n_boundary : kind == IMMESH_EDGE_NONMANIFOLD ? q.st.n_nonmanifold : q.st.n_inconsistent;
    if ((rc = rc_cap(c, "topology_edges", cap, n, n_out, uv || uses, "edges"))) return rc;
    if ((!uv && !uses) || n == 0) return 0;
    (void)hipSetDevice(c->cfg.device);
    hipStream_t s = r->s;
    const int64_t n_half = q.n_half, n_edges = q.st.n_edges;
    if ((rc = tp_temp(r, n_half, 1))) return rc;
    if ((rc = tp_grow(r, q.head, (size_t)n_half * 4))) return rc;
    if ((rc = tp_grow(r, q.eid, (size_t)n_half * 4))) return rc;
    if ((rc = tp_grow(r, q.start, (size_t)(n_edges + 1) * 4))) return rc;
    if ((rc = tp_grow(r, q.pick, (size_t)n_edges * 4))) return rc;
    if ((rc = tp_grow(r, q.poff, (size_t)n_edges * 4))) return rc;
    if ((rc = tp_grow(r, q.uv, (size_t)n * 8))) return rc;
    if ((rc = tp_grow(r, q.uses, (size_t)n * 4))) return rc;
    const unsigned long long* key = (const unsigned long long*)q.key_b.p;
    int32_t *head = (int32_t*)q.head.p, *eid = (int32_t*)q.eid.p, *start = (int32_t*)q.start.p, *pick = (int32_t*)q.pick.p, *poff = (int32_t*)q.poff.p;
    pd_launch_run_heads(s, key, n_half, head);
    exclusive_sum_i32(s, r->tree.temp.p, r->tree.temp.bytes, head, eid, (int)n_half);
    pd_launch_run_starts(s, n_half, head, eid, start, n_edges + 1);
    tp_launch_pick(s, start, n_edges, (const int32_t*)q.val_b.p, (const int32_t*)r->faces.p, kind, pick);
    exclusive_sum_i32(s, r->tree.temp.p, r->tree.temp.bytes, pick, poff, (int)n_edges);
    tp_launch_edges(s, start, n_edges, key, pick, poff, (int32_t*)q.uv.p, (int32_t*)q.uses.p);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(s));
    if ((rc = rc_fetch(c, uv, q.uv.p, (size_t)n * 8))) return rc;
    return rc_fetch(c, uses, q.uses.p, (size_t)n * 4);
}

int immesh_topology_select(immesh_raycaster* r, int64_t min_faces, double min_diagonal, int64_t keep_largest, int8_t* keep_out, int32_t* faces_out,
                           int64_t cap, int64_t* n_kept) {
    if (!r) return IMMESH_E_INVAL;
    immesh_ctx* c = r->ctx;
    int rc;
    if ((rc = rc_analysed(r, "topology_select"))) return rc;
    if (min_faces < 0) { c->err = "topology_select: min_faces is negative"; return IMMESH_E_INVAL; }
    if (keep_largest < 0) { c->err = "topology_select: keep_largest is negative"; return IMMESH_E_INVAL; }
    if (!(min_diagonal >= 0.0) || !std::isfinite(min_diagonal)) { c->err = "topology_select: need 0 <= min_diagonal, finite"; return IMMESH_E_INVAL; }
    if ((rc = rc_cap_negative(c, "topology_select", cap))) return rc;
    (void)hipSetDevice(c->cfg.device);
    hipStream_t s = r->s;
    RcTopology& q = r->tp;
    const int64_t nf = r->n_faces, n_comp = q.st.n_components;
    int64_t kept = 0;
    if (nf > 0) {
        if ((rc = tp_temp(r, nf, n_comp))) return rc;
        if ((rc = tp_grow(r, q.keepc, (size_t)n_comp * 4))) return rc;
        if ((rc = tp_grow(r, q.keep32, (size_t)nf * 4))) return rc;
        if ((rc = tp_grow(r, q.keep8, (size_t)nf))) return rc;
        if ((rc = tp_grow(r, q.koff, (size_t)nf * 4))) return rc;
        if ((rc = tp_grow(r, q.out, (size_t)nf * 12))) return rc;
        const int32_t* sorted = nullptr;
        if (keep_largest > 0 && n_comp > 0) {
            if ((rc = tp_grow(r, q.rank_a, (size_t)n_comp * 8))) return rc;
            if ((rc = tp_grow(r, q.rank_b, (size_t)n_comp * 8))) return rc;
            if ((rc = tp_grow(r, q.iota_a, (size_t)n_comp * 4))) return rc;
            if ((rc = tp_grow(r, q.iota_b, (size_t)n_comp * 4))) return rc;
        }
        HIPCHK(c, hipEventRecord(q.ev[2], s));
        if (keep_largest > 0 && n_comp > 0) {   // the ranking: a sort of (-n_faces, label) by the pair sort
            tp_launch_rank_keys(s, (const int32_t*)q.nfaces.p, n_comp, (unsigned long long*)q.rank_a.p, (int32_t*)q.iota_a.p);
            sort_pairs_u64(s, r->tree.temp.p, r->tree.temp.bytes, (const unsigned long long*)q.rank_a.p, (unsigned long long*)q.rank_b.p,
                           (const int32_t*)q.iota_a.p, (int32_t*)q.iota_b.p, (int)n_comp, 64);
            sorted = (const int32_t*)q.iota_b.p;
        }
        tp_launch_decide(s, (const int32_t*)q.nfaces.p, (const uint32_t*)q.box.p, n_comp, min_faces, min_diagonal, keep_largest, sorted, (int32_t*)q.keepc.p);
        tp_launch_mask(s, (const int32_t*)q.comp.p, (const int32_t*)q.keepc.p, nf, (int32_t*)q.keep32.p, (int8_t*)q.keep8.p);
        exclusive_sum_i32(s, r->tree.temp.p, r->tree.temp.bytes, (const int32_t*)q.keep32.p, (int32_t*)q.koff.p, (int)nf);
        tp_launch_compact(s, (const int32_t*)r->faces.p, (const int32_t*)q.keep32.p, (const int32_t*)q.koff.p, nf, (int32_t*)q.out.p,
                          (unsigned long long*)q.cnt.p);
        if ((rc = rc_pass_end(q, 2, 3, 1, TP_N_KEPT, 1))) return rc;
        kept = (int64_t)q.h_cnt[TP_N_KEPT];
        if ((rc = rc_fetch(c, keep_out, q.keep8.p, (size_t)nf))) return rc;
    }
    if ((rc = rc_cap(c, "topology_select", cap, kept, n_kept, faces_out != nullptr, "kept faces"))) return rc;
    return rc_fetch(c, faces_out, q.out.p, (size_t)kept * 12);
}

int immesh_topology_last_timing(immesh_raycaster* r, float ms[2]) {
    if (!r || !ms) return IMMESH_E_INVAL;
    ms[0] = r->tp.ms[0]; ms[1] = r->tp.ms[1];
    return 0;
}

}  // extern "C"
