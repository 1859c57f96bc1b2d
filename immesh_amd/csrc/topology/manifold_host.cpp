// Host side of the manifold pass (include/immesh_topology.h, the Manifold rule): argument checks, grow-only buffers in the caster's RcManifold
// record, the pass, its fetches and the apply on the caster's stream.  Nothing here is allocated or launched before the first
// immesh_topology_manifold.  It reads what the analysis left on the device: the marks of the counting faces and the sorted half-edges.  One read-back
// lies between the launches, as in the analysis: the number of fans, which sizes the sort of their keys and their tables.
#include <algorithm>
#include <cstddef>
#include <string>
#include "../host_ctx.hpp"
#include "../../../include/immesh_topology.h"
#include "topology.hpp"
#include "../raycast/pass_dev.hpp"   // the run kernels of the fans' vertices

static_assert(sizeof(immesh_manifold_stats) == 12 * 8 && offsetof(immesh_manifold_stats, n_corners) == 0 && offsetof(immesh_manifold_stats, n_fans) == 8 &&
                  offsetof(immesh_manifold_stats, n_vertices_used) == 16 && offsetof(immesh_manifold_stats, n_singular_vertices) == 24 &&
                  offsetof(immesh_manifold_stats, most_fans_at_vertex) == 32 && offsetof(immesh_manifold_stats, n_new_vertices) == 40 &&
                  offsetof(immesh_manifold_stats, n_corners_moved) == 48 && offsetof(immesh_manifold_stats, n_faces_changed) == 56 &&
                  offsetof(immesh_manifold_stats, n_closed_fans) == 64 && offsetof(immesh_manifold_stats, n_open_fans) == 72 &&
                  offsetof(immesh_manifold_stats, largest_fan_corners) == 80 && offsetof(immesh_manifold_stats, n_nonmanifold_before) == 88,
              "immesh_manifold_stats layout (immesh_amd/capi.py mirrors it)");

namespace {

constexpr int64_t MF_MAX_VTX = 0x7FFFFFFF;                      // an index is an int32

int mf_grow(immesh_raycaster* r, RcBuf& b, size_t bytes) { return rc_pass_grow(r->mf, b, bytes); }

int mf_passed(immesh_raycaster* r, const char* who) {
    const int rc = rc_analysed(r, who);
    return rc ? rc : rc_passed(r, who, r->mf, "no manifold pass since the last analysis (immesh_topology_manifold)");
}

}  // namespace

extern "C" {

int immesh_topology_manifold(immesh_raycaster* r, immesh_manifold_stats* stats) {
    if (!r) return IMMESH_E_INVAL;
    immesh_ctx* c = r->ctx;
    int rc;
    if ((rc = rc_analysed(r, "topology_manifold"))) return rc;
    (void)hipSetDevice(c->cfg.device);
    hipStream_t s = r->s;
    const RcTopology& q = r->tp;
    RcManifold& o = r->mf;
    const int64_t nf = r->n_faces, nv = r->n_vtx, n3 = 3 * nf, n_half = q.n_half, n_used = q.st.n_vertices_used;   // (3 n_faces <= 2^31 - 2: the analysis)
    o.have = false;
    if ((rc = rc_pass_ready(c, s, "topology_manifold", o, MF_COUNTERS, MF_COUNTERS + 2))) return rc;
    RcBuf* const per_corner[] = {&o.parent, &o.root, &o.isroot, &o.off, &o.ncnt, &o.nlnk, &o.fanof, &o.faces_out, &o.fan_out};
    for (RcBuf* b : per_corner)
        if ((rc = mf_grow(r, *b, (size_t)n3 * 4))) return rc;
    if ((rc = mf_grow(r, o.nfans, (size_t)nv * 4))) return rc;
    if ((rc = mf_grow(r, o.start, (size_t)(n_used + 1) * 4))) return rc;
    if ((rc = mf_grow(r, r->tree.temp, exclusive_sum_temp_bytes((int)std::max<int64_t>(n3, 1)) + 256))) return rc;   // the caster's scan scratch
    const int32_t *faces = (const int32_t*)r->faces.p, *flag = (const int32_t*)q.flag.p, *val = (const int32_t*)q.val_b.p;
    const unsigned long long* key = (const unsigned long long*)q.key_b.p;
    int32_t *parent = (int32_t*)o.parent.p, *root = (int32_t*)o.root.p, *isroot = (int32_t*)o.isroot.p, *off = (int32_t*)o.off.p;
    int32_t *ncnt = (int32_t*)o.ncnt.p, *nlnk = (int32_t*)o.nlnk.p, *fanof = (int32_t*)o.fanof.p;
    unsigned long long* cnt = (unsigned long long*)o.cnt.p;
    unsigned long long* h = o.h_cnt;
    if ((rc = rc_pass_begin(o, 0))) return rc;
    int64_t n_fans = 0;
    if (n_half > 0) {
        mf_launch_init(s, n3, parent, ncnt, nlnk);
        mf_launch_link(s, key, val, n_half, faces, parent, cnt);
        mf_launch_flatten(s, parent, flag, n3, root, isroot, ncnt);
        mf_launch_links(s, key, val, n_half, faces, root, nlnk);
        exclusive_sum_i32(s, r->tree.temp.p, r->tree.temp.bytes, isroot, off, (int)n3);
        h[MF_COUNTERS] = h[MF_COUNTERS + 1] = 0;
        HIPCHK(c, hipMemcpyAsync(&h[MF_COUNTERS], off + (n3 - 1), 4, hipMemcpyDeviceToHost, s));        // the one count the host needs: it sizes the
        HIPCHK(c, hipMemcpyAsync(&h[MF_COUNTERS + 1], isroot + (n3 - 1), 4, hipMemcpyDeviceToHost, s));   // sort and the fans' tables
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipStreamSynchronize(s));
        n_fans = (int64_t)h[MF_COUNTERS] + (int64_t)h[MF_COUNTERS + 1];
    }
    if (n_fans < n_used || n_fans > n_half) {   // every used vertex has a fan, every fan a corner of its own
        c->err = "topology_manifold: " + std::to_string(n_fans) + " fans for " + std::to_string(n_used) + " used vertices (a defect of the library)";
        return IMMESH_E_INTERNAL;
    }
    const int64_t n_new = n_fans - n_used;
    if ((rc = mf_grow(r, o.vtx_out, (size_t)(nv + n_new) * 12))) return rc;
    if (nv > 0) {
        HIPCHK(c, hipMemsetAsync(o.nfans.p, 0, (size_t)nv * 4, s));
        HIPCHK(c, hipMemcpyAsync(o.vtx_out.p, r->vtx.p, (size_t)nv * 12, hipMemcpyDeviceToDevice, s));
    }
    if (n_fans > 0) {
        if ((rc = mf_grow(r, o.key_a, (size_t)n_fans * 8))) return rc;
        if ((rc = mf_grow(r, o.key_b, (size_t)n_fans * 8))) return rc;
        RcBuf* const per_fan[] = {&o.val_a, &o.val_b, &o.fv, &o.head, &o.scan};
        for (RcBuf* b : per_fan)
            if ((rc = mf_grow(r, *b, (size_t)n_fans * 4))) return rc;
        if ((rc = mf_grow(r, o.ft, (size_t)n_fans * MT_TABLES * 4))) return rc;
        if ((rc = mf_grow(r, o.vsrc, (size_t)n_new * 4))) return rc;
        if ((rc = mf_grow(r, r->tree.temp, sort_pairs_u64_temp_bytes((int)n_fans) + 256))) return rc;
        unsigned long long *key_a = (unsigned long long*)o.key_a.p, *key_b = (unsigned long long*)o.key_b.p;
        int32_t *fv = (int32_t*)o.fv.p, *head = (int32_t*)o.head.p, *scan = (int32_t*)o.scan.p, *start = (int32_t*)o.start.p, *ft = (int32_t*)o.ft.p;
        mf_launch_keys(s, faces, isroot, off, n3, key_a, (int32_t*)o.val_a.p, n_fans);
        sort_pairs_u64(s, r->tree.temp.p, r->tree.temp.bytes, key_a, key_b, (const int32_t*)o.val_a.p, (int32_t*)o.val_b.p, (int)n_fans,
                       32 + rc_index_bits(nv));
        mf_launch_fans(s, key_b, n_fans, n3, fv, fanof);
        pd_launch_run_heads(s, fv, n_fans, head);
        exclusive_sum_i32(s, r->tree.temp.p, r->tree.temp.bytes, head, scan, (int)n_fans);
        pd_launch_run_starts(s, n_fans, head, scan, start, n_used + 1);
        mf_launch_table(s, n_fans, key_b, head, scan, ncnt, nlnk, (const float*)r->vtx.p, nv, n_new, ft, (int32_t*)o.vsrc.p, (float*)o.vtx_out.p, cnt);
        mf_launch_vertices(s, n_used, start, fv, n_fans, nv, (int32_t*)o.nfans.p, cnt);
    }
    mf_launch_emit(s, faces, nf, flag, root, fanof, (const int32_t*)o.ft.p, n_fans, (int32_t*)o.faces_out.p, (int32_t*)o.fan_out.p, cnt);
    if ((rc = rc_pass_end(o, 0, 1, 0, 0, MF_COUNTERS))) return rc;
    if (h[MF_ERROR]) {
        c->err = "topology_manifold: a union did not finish within its step bound (a defect of the library)";
        return IMMESH_E_INTERNAL;
    }
    immesh_manifold_stats& st = o.st;
    st.n_corners = n_half; st.n_fans = n_fans; st.n_vertices_used = n_used; st.n_singular_vertices = (int64_t)h[MF_N_SINGULAR];
    st.most_fans_at_vertex = (int64_t)h[MF_MOST_FANS]; st.n_new_vertices = n_new; st.n_corners_moved = (int64_t)h[MF_N_MOVED];
    st.n_faces_changed = (int64_t)h[MF_N_CHANGED]; st.n_closed_fans = (int64_t)h[MF_N_CLOSED]; st.n_open_fans = (int64_t)h[MF_N_OPEN];
    st.largest_fan_corners = (int64_t)h[MF_LARGEST_FAN]; st.n_nonmanifold_before = q.st.n_nonmanifold;
    o.n_fans = n_fans;
    o.have = true;
    if (stats) *stats = st;
    return 0;
}

int immesh_topology_manifold_vertices(immesh_raycaster* r, int32_t* n_fans_out) {
    if (!r) return IMMESH_E_INVAL;
    immesh_ctx* c = r->ctx;
    int rc;
    if ((rc = mf_passed(r, "topology_manifold_vertices"))) return rc;
    (void)hipSetDevice(c->cfg.device);
    return rc_fetch(c, n_fans_out, r->mf.nfans.p, (size_t)r->n_vtx * 4);
}

int immesh_topology_manifold_fans(immesh_raycaster* r, int32_t* vertex, int32_t* first_face, int32_t* n_corners, int32_t* n_links, int32_t* index_out,
                                  int64_t cap, int64_t* n_out) {
    if (!r) return IMMESH_E_INVAL;
    immesh_ctx* c = r->ctx;
    int rc;
    if ((rc = mf_passed(r, "topology_manifold_fans"))) return rc;
    const RcManifold& o = r->mf;
    const int64_t n = o.n_fans;
    const bool wanted = vertex || first_face || n_corners || n_links || index_out;
    if ((rc = rc_cap(c, "topology_manifold_fans", cap, n, n_out, wanted, "fans"))) return rc;
    if (!wanted || n == 0) return 0;
    (void)hipSetDevice(c->cfg.device);
    const int32_t* ft = (const int32_t*)o.ft.p;
    int32_t* const out[MT_TABLES] = {vertex, first_face, n_corners, n_links, index_out};
    for (int k = 0; k < MT_TABLES; k++)
        if ((rc = rc_fetch(c, out[k], ft + k * n, (size_t)n * 4))) return rc;
    return 0;
}

int immesh_topology_manifold_faces(immesh_raycaster* r, int32_t* fan_out, int32_t* faces_out) {
    if (!r) return IMMESH_E_INVAL;
    immesh_ctx* c = r->ctx;
    int rc;
    if ((rc = mf_passed(r, "topology_manifold_faces"))) return rc;
    (void)hipSetDevice(c->cfg.device);
    if ((rc = rc_fetch(c, fan_out, r->mf.fan_out.p, (size_t)r->n_faces * 12))) return rc;
    return rc_fetch(c, faces_out, r->mf.faces_out.p, (size_t)r->n_faces * 12);
}

int immesh_topology_manifold_new_vertices(immesh_raycaster* r, int32_t* vsrc, float* xyz, int64_t cap, int64_t* n_out) {
    if (!r) return IMMESH_E_INVAL;
    immesh_ctx* c = r->ctx;
    int rc;
    if ((rc = mf_passed(r, "topology_manifold_new_vertices"))) return rc;
    const RcManifold& o = r->mf;
    const int64_t n = o.st.n_new_vertices;
    if ((rc = rc_cap(c, "topology_manifold_new_vertices", cap, n, n_out, vsrc || xyz, "new vertices"))) return rc;
    if (n == 0) return 0;
    (void)hipSetDevice(c->cfg.device);
    if ((rc = rc_fetch(c, vsrc, o.vsrc.p, (size_t)n * 4))) return rc;
    return rc_fetch(c, xyz, (const float*)o.vtx_out.p + 3 * r->n_vtx, (size_t)n * 12);
}

int immesh_topology_manifold_apply(immesh_raycaster* r) {
    if (!r) return IMMESH_E_INVAL;
    immesh_ctx* c = r->ctx;
    int rc;
    if ((rc = mf_passed(r, "topology_manifold_apply"))) return rc;
    RcManifold& o = r->mf;
    const int64_t nf = r->n_faces, n_new = o.st.n_new_vertices, total = r->n_vtx + n_new;
    if (total > MF_MAX_VTX) {
        c->err = "topology_manifold_apply: " + std::to_string(r->n_vtx) + " vertices and " + std::to_string(n_new) + " new ones exceed 2^31 - 1";
        return IMMESH_E_INVAL;
    }
    (void)hipSetDevice(c->cfg.device);
    HIPCHK(c, hipEventRecord(o.ev[2], r->s));
    if (total > 0) rc_swap(r->vtx, o.vtx_out);                  // the stream is idle: the pass synchronised
    if (nf > 0) rc_swap(r->faces, o.faces_out);
    if ((rc = rc_build(r, total, nf))) return rc;               // discards what read the snapshot, this pass too; the stream is idle on return
    return rc_pass_span(o, 2, 3, 1);
}

int immesh_topology_manifold_last_timing(immesh_raycaster* r, float* ms) {
    if (!r || !ms) return IMMESH_E_INVAL;
    ms[0] = r->mf.ms[0]; ms[1] = r->mf.ms[1];
    return 0;
}

}  // extern "C"
