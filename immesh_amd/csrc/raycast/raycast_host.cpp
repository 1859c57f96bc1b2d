// Host side of the ray caster (include/immesh_raycast.h): the shared scaffold of rc_host.hpp, argument checks, the build and cast sequences on the caster's stream.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include "../host_ctx.hpp"
#include "../../../include/immesh_raycast.h"
#include "../render/render.hpp"
#include "raycast.hpp"

int rc_grow(immesh_ctx* c, const char* who, RcBuf& b, size_t bytes) {
    if (bytes == 0) bytes = 16;
    if (b.bytes >= bytes) return 0;
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr; b.bytes = 0;
    const size_t want = bytes + bytes / 4;
    if (hipMalloc(&b.p, want) != hipSuccess) {
        (void)hipGetLastError();
        c->err = std::string(who) + ": hipMalloc(" + std::to_string(want) + " B) failed";
        return IMMESH_E_NOMEM;
    }
    b.bytes = want;
    return 0;
}

int rc_finite_pose(immesh_ctx* c, const char* who, const char* noun, const double rot[9], const double pos[3]) {
    for (int i = 0; i < 9; i++)
        if (!std::isfinite(rot[i])) { c->err = std::string(who) + ": " + noun + " rotation is not finite"; return IMMESH_E_INVAL; }
    for (int i = 0; i < 3; i++)
        if (!std::isfinite(pos[i])) { c->err = std::string(who) + ": " + noun + " position is not finite"; return IMMESH_E_INVAL; }
    return 0;
}

int rc_frame(immesh_ctx* c, const char* who, const immesh_ray_frame* frame, RcFrame* fr) {
    const int rc = rc_finite_pose(c, who, "frame", frame->rot, frame->pos);
    if (rc) return rc;
    std::memcpy(fr->rot, frame->rot, sizeof(fr->rot));
    std::memcpy(fr->pos, frame->pos, sizeof(fr->pos));
    return 0;
}

int rc_fetch(immesh_ctx* c, void* dst, const void* src, size_t bytes) {
    if (dst && bytes > 0) HIPCHK(c, hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return 0;
}

int rc_cap_negative(immesh_ctx* c, const char* who, int64_t cap) {
    if (cap < 0) { c->err = std::string(who) + ": cap is negative"; return IMMESH_E_INVAL; }
    return 0;
}

int rc_cap(immesh_ctx* c, const char* who, int64_t cap, int64_t n, int64_t* n_out, bool wanted, const char* noun) {
    const int rc = rc_cap_negative(c, who, cap);
    if (rc) return rc;
    if (n_out) *n_out = n;
    if (wanted && cap < n) {
        c->err = std::string(who) + ": cap " + std::to_string(cap) + " < " + std::to_string(n) + " " + noun;
        return IMMESH_E_CAPACITY;
    }
    return 0;
}

int rc_built(immesh_raycaster* r, const char* who) {
    if (!r->built) { r->ctx->err = std::string(who) + ": no hierarchy has been built (immesh_raycast_build_triangles / _build_mesh)"; return IMMESH_E_INVAL; }
    return 0;
}

int rc_analysed(immesh_raycaster* r, const char* who) {
    const int rc = rc_built(r, who);
    if (rc) return rc;
    if (!r->tp.have) { r->ctx->err = std::string(who) + ": no analysis since the caster's last build (immesh_topology_analyse)"; return IMMESH_E_INVAL; }
    return 0;
}

int rc_have(immesh_ctx* c, const char* who, bool have, const char* none) {
    if (!have) { c->err = std::string(who) + ": " + none; return IMMESH_E_INVAL; }
    return 0;
}

int rc_passed(immesh_raycaster* r, const char* who, const RcPass& p, const char* none) { return rc_have(r->ctx, who, p.have, none); }

int rc_positive(immesh_ctx* c, const char* who, const char* what, double v) {
    if (!(v > 0.0) || !std::isfinite(v)) { c->err = std::string(who) + ": need 0 < " + what + ", finite"; return IMMESH_E_INVAL; }
    return 0;
}

int rc_points(immesh_ctx* c, const char* who, const float* pts, int64_t n) {
    if (n < 0 || n > RC_MAX_COUNT || (n > 0 && !pts)) { c->err = std::string(who) + ": bad point array"; return IMMESH_E_INVAL; }
    return 0;
}

int rc_count_arg(immesh_ctx* c, const char* who, const char* what, int64_t v) {
    if (v < 0 || v > RC_MAX_COUNT) { c->err = std::string(who) + ": need " + what + " in [0, 2^31 - 2]"; return IMMESH_E_INVAL; }
    return 0;
}

int rc_check_soup(immesh_ctx* c, const char* who, int64_t max_faces, const float* vtx, int64_t n_vtx, const int32_t* faces, int64_t n_faces) {
    if (n_vtx < 0 || n_faces < 0 || n_faces > max_faces || (n_vtx > 0 && !vtx) || (n_faces > 0 && !faces)) {
        c->err = std::string(who) + ": bad vertex / face arrays";
        return IMMESH_E_INVAL;
    }
    for (int64_t i = 0; i < 3 * n_faces; i++)
        if (faces[i] < 0 || (int64_t)faces[i] >= n_vtx) {
            c->err = std::string(who) + ": face " + std::to_string(i / 3) + " has vertex index " + std::to_string(faces[i]) + " out of range [0, " +
                     std::to_string(n_vtx) + ")";
            return IMMESH_E_INVAL;
        }
    return 0;
}

int rc_upload_soup(immesh_ctx* c, const char* who, hipStream_t s, RcBuf& d_vtx, RcBuf& d_faces, const float* vtx, int64_t n_vtx, const int32_t* faces,
                   int64_t n_faces) {
    int rc;
    if ((rc = rc_grow(c, who, d_vtx, (size_t)n_vtx * 12))) return rc;
    if ((rc = rc_grow(c, who, d_faces, (size_t)n_faces * 12))) return rc;
    if (n_vtx > 0) HIPCHK(c, hipMemcpyAsync(d_vtx.p, vtx, (size_t)n_vtx * 12, hipMemcpyHostToDevice, s));
    if (n_faces > 0) HIPCHK(c, hipMemcpyAsync(d_faces.p, faces, (size_t)n_faces * 12, hipMemcpyHostToDevice, s));
    return 0;
}

int cx_built(immesh_cloud_index* x, const char* who) { return rc_have(x->ctx, who, x->built, "no index has been built (immesh_cloud_index_build)"); }

int cx_caster(immesh_cloud_index* x, const immesh_raycaster* r, const char* who) {
    const int rc = rc_have(x->ctx, who, r != nullptr, "no caster");
    return rc ? rc : rc_have(x->ctx, who, r->ctx == x->ctx, "the caster and the index belong to different contexts");
}

int cx_caster_built(immesh_cloud_index* x, const immesh_raycaster* r, const char* who, bool sampled) {
    const int rc = rc_have(x->ctx, who, r->built, "no hierarchy has been built on the caster");
    return rc || !sampled ? rc : rc_have(x->ctx, who, r->sm.have, "no samples since the caster's last build (immesh_mesh_sample)");
}

int rc_span_end(immesh_ctx* c, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1, float* ms, void* dst, const void* src, size_t bytes) {
    HIPCHK(c, hipEventRecord(ev1, s));
    if (bytes > 0) HIPCHK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s));   // the read-back
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(s));
    (void)hipEventElapsedTime(ms, ev0, ev1);
    return 0;
}

int rc_thin_grow(immesh_ctx* c, const char* who, RcThin& th, RcBuf& temp, int64_t n, float res, uint32_t* mask) {
    int rc;
    if ((rc = rc_grow(c, who, temp, rd_scan_temp_bytes(1, 1, n) + 256))) return rc;
    if ((rc = rc_grow(c, who, th.pts, (size_t)n * 12))) return rc;
    if ((rc = rc_grow(c, who, th.keep, (size_t)n * 4))) return rc;
    if ((rc = rc_grow(c, who, th.koff, (size_t)n * 4))) return rc;
    if ((rc = rc_grow(c, who, th.out, (size_t)n * 12))) return rc;
    if ((rc = rc_grow(c, who, th.small, 16))) return rc;
    *mask = 0;
    if (res > 0.0f) {
        uint64_t slots = 1024;
        while (slots < 2 * (uint64_t)n) slots <<= 1;
        *mask = (uint32_t)(slots - 1);
        if ((rc = rc_grow(c, who, th.cells, (size_t)n * 12))) return rc;
        if ((rc = rc_grow(c, who, th.slot, (size_t)n * 4))) return rc;
        if ((rc = rc_grow(c, who, th.tab, (size_t)slots * 8))) return rc;
    }
    return 0;
}

int rc_thin_run(immesh_ctx* c, hipStream_t s, RcThin& th, RcBuf& temp, int64_t n, float res, uint32_t mask, const float* depth) {
    int32_t* keep = (int32_t*)th.keep.p;
    if (res > 0.0f) {
        int32_t* tab_rep = (int32_t*)th.tab.p;
        uint32_t* tab_min = (uint32_t*)(tab_rep + (size_t)mask + 1);
        HIPCHK(c, hipMemsetAsync(tab_rep, 0xFF, ((size_t)mask + 1) * 8, s));   // rep -1, min 0xFFFFFFFF
        rd_launch_hash_insert(s, n, depth, (const float*)th.cells.p, tab_rep, tab_min, mask, (uint32_t*)th.slot.p);
        rd_launch_hash_keep(s, n, depth, tab_min, (const uint32_t*)th.slot.p, keep);
    }
    rd_scan_i32(s, temp.p, temp.bytes, keep, (int32_t*)th.koff.p, n);
    rd_launch_compact(s, n, (const float*)th.pts.p, keep, (const int32_t*)th.koff.p, (float*)th.out.p, (int64_t*)th.small.p);
    return 0;
}

int rc_thin_fetch(immesh_ctx* c, const char* who, const RcThin& th, int64_t n_points, float* xyz_out, int64_t cap, int64_t* n_out) {
    if (n_out) *n_out = n_points;
    if (!xyz_out || n_points == 0) return 0;
    if (cap < n_points) {
        c->err = std::string(who) + ": cap " + std::to_string(cap) + " < " + std::to_string(n_points) + " points";
        return IMMESH_E_CAPACITY;
    }
    (void)hipSetDevice(c->cfg.device);
    return rc_fetch(c, xyz_out, th.out.p, (size_t)n_points * 12);
}

int rc_pass_ready(immesh_ctx* c, hipStream_t s, const char* who, RcPass& p, int n_cnt, int n_pinned) {
    for (hipEvent_t& e : p.ev)
        if (!e) HIPCHK(c, hipEventCreate(&e));
    if (!p.h_cnt) HIPCHK(c, hipHostMalloc((void**)&p.h_cnt, (size_t)n_pinned * 8));
    p.ctx = c; p.s = s; p.who = who; p.n_cnt = n_cnt;
    return rc_pass_grow(p, p.cnt, (size_t)n_cnt * 8);
}

int cx_ready(immesh_cloud_index* x, RcPass& p, int n_cnt, int n_pinned) {
    (void)hipSetDevice(x->ctx->cfg.device);
    return rc_pass_ready(x->ctx, x->s, "cloud_index", p, n_cnt, n_pinned);
}

int rc_pass_grow(const RcPass& p, RcBuf& b, size_t bytes) { return rc_grow(p.ctx, p.who, b, bytes); }

int rc_pass_begin(RcPass& p, int e0) {
    HIPCHK(p.ctx, hipEventRecord(p.ev[e0], p.s));
    HIPCHK(p.ctx, hipMemsetAsync(p.cnt.p, 0, (size_t)p.n_cnt * 8, p.s));
    return 0;
}

int rc_pass_end(RcPass& p, int e0, int e1, int span, int first, int n) {
    return rc_span_end(p.ctx, p.s, p.ev[e0], p.ev[e1], &p.ms[span], p.h_cnt + first, (const unsigned long long*)p.cnt.p + first, (size_t)n * 8);
}

int rc_pass_span(RcPass& p, int e0, int e1, int span) {
    HIPCHK(p.ctx, hipEventRecord(p.ev[e1], p.s));
    HIPCHK(p.ctx, hipStreamSynchronize(p.s));
    (void)hipEventElapsedTime(&p.ms[span], p.ev[e0], p.ev[e1]);
    return 0;
}

float rc_pass_ms(const RcPass& p, int e0, int e1) {
    float ms = 0.0f;
    (void)hipEventElapsedTime(&ms, p.ev[e0], p.ev[e1]);
    return ms;
}

void rc_pass_counts(const RcPass& p, int64_t counts[4]) {
    if (counts)
        for (int i = 0; i < 4; i++) counts[i] = (int64_t)p.h_cnt[i];
}

int rc_tree_build(immesh_ctx* c, const char* who, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1, int64_t* h_count, RcTree& t, int64_t n, const RcLeaves& src) {
    int rc;
    const size_t temp_bytes = std::max(rd_scan_temp_bytes(1, 1, std::max<int64_t>(n, 1)), sort_pairs_u64_temp_bytes((int)std::max<int64_t>(n, 1))) + 256;
    if ((rc = rc_grow(c, who, t.flag, (size_t)n * 4))) return rc;
    if ((rc = rc_grow(c, who, t.off, (size_t)n * 4))) return rc;
    if ((rc = rc_grow(c, who, t.ids, (size_t)n * 4))) return rc;
    if ((rc = rc_grow(c, who, t.box, (size_t)n * 24))) return rc;
    if ((rc = rc_grow(c, who, t.bounds, 32))) return rc;
    if ((rc = rc_grow(c, who, t.temp, temp_bytes))) return rc;
    int32_t *flag = (int32_t*)t.flag.p, *off = (int32_t*)t.off.p, *ids = (int32_t*)t.ids.p;
    float* box = (float*)t.box.p;
    uint32_t* bounds = (uint32_t*)t.bounds.p;
    int64_t* d_n_in = (int64_t*)(bounds + 6);
    HIPCHK(c, hipEventRecord(ev0, s));
    HIPCHK(c, hipMemsetAsync(bounds, 0xFF, 12, s));
    HIPCHK(c, hipMemsetAsync(bounds + 3, 0, 20, s));
    int64_t n_in = 0;
    if (n > 0) {
        rc_launch_mark(s, src, n, flag);
        rd_scan_i32(s, t.temp.p, t.temp.bytes, flag, off, n);
        rc_launch_compact(s, src, n, flag, off, ids, box, bounds, d_n_in);
        HIPCHK(c, hipMemcpyAsync(h_count, d_n_in, 8, hipMemcpyDeviceToHost, s));   // the one count the host needs: it sizes the tree
        HIPCHK(c, hipStreamSynchronize(s));
        n_in = h_count[0];
    }
    if (n_in > 0) {
        if ((rc = rc_grow(c, who, t.code_a, (size_t)n_in * 8))) return rc;
        if ((rc = rc_grow(c, who, t.code_b, (size_t)n_in * 8))) return rc;
        if ((rc = rc_grow(c, who, t.pos_a, (size_t)n_in * 4))) return rc;
        if ((rc = rc_grow(c, who, t.pos_b, (size_t)n_in * 4))) return rc;
        if ((rc = rc_grow(c, who, t.leaf, (size_t)n_in * 4))) return rc;
        if ((rc = rc_grow(c, who, t.nodes, (size_t)n_in * sizeof(RcNode)))) return rc;
        RcNode* nodes = (RcNode*)t.nodes.p;
        if (n_in == 1) {
            rc_launch_single(s, box, ids, nodes);
        } else {
            unsigned long long *code_a = (unsigned long long*)t.code_a.p, *code_b = (unsigned long long*)t.code_b.p;
            int32_t *pos_a = (int32_t*)t.pos_a.p, *pos_b = (int32_t*)t.pos_b.p, *leaf = (int32_t*)t.leaf.p;
            rc_launch_codes(s, box, n_in, bounds, code_a, pos_a);
            sort_pairs_u64(s, t.temp.p, t.temp.bytes, code_a, code_b, pos_a, pos_b, (int)n_in, RC_CODE_BITS);
            rc_launch_hierarchy(s, code_b, ids, pos_b, n_in, nodes, leaf);
            rc_launch_refit(s, box, pos_b, leaf, n_in, nodes);
        }
    }
    HIPCHK(c, hipEventRecord(ev1, s));
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(s));
    t.n_in = n_in;
    return 0;
}

static constexpr int64_t RC_MAX_FACES = (int64_t)1 << RC_INDEX_BITS;

// What a change of the caster's state discards.  A change of the snapshot is a build (rc_build: a rebuild, and the applies of a holes pass, a
// manifold pass, a simplification and a smoothing pass, which end in one) or the apply of an orientation, which keeps the hierarchy.  A new analysis replaces the old.
//
//   derived result                              | the snapshot changes  | a new analysis
//   the last NEAREST cast, its reinforced points | discarded             | stay
//   the samples (sm)                             | discarded             | stay
//   the analysis (tp)                            | discarded             | replaced
//   the orientation (ot), the holes pass (hl),   | discarded (they read the analysis) | discarded
//   the manifold pass (mf)                       |
//   the simplification's result (sp)             | discarded             | stays
//   the smoothing pass' result (so)              | discarded             | stays
//   the intersection pass' result (ix)           | discarded             | stays
//   the closest-point results of the last query  | stay                  | stay
//
// The closest-point results stay readable on purpose: they are answers about the points of a query, not a view of the snapshot.  immesh_raycast
// handles have_cast itself (a NEAREST cast replaces the last one, an ANY cast leaves it), and a pass clears its own `have` when it starts.  A new
// derived result adds one line to one of these two functions and nowhere else.
void rc_analysis_changed(immesh_raycaster* r) {
    r->ot.have = false;   // an orientation belongs to the analysis whose half-edges it read
    r->hl.have = false;   // and so does a holes pass
    r->mf.have = false;   // and a manifold pass
}

void rc_snapshot_changed(immesh_raycaster* r) {
    r->have_cast = false; r->n_points = 0;
    r->sm.have = false;
    r->tp.have = false;
    rc_analysis_changed(r);
    r->sp.have = false;
    r->so.have = false;
    r->ix.have = false;
}

// What a change of a cloud index's state discards.  A change of the cloud is immesh_cloud_index_build or immesh_cloud_index_apply_outliers; new
// normals are an immesh_cloud_normals call.
//
//   derived result                              | the cloud changes     | new normals
//   the last nearest query (q)                   | discarded             | stays
//   the last cloud-mode Neighbours query (kn)    | discarded             | stays
//   the last cloud-mode Count query (kn)         | discarded             | stays
//   the last mask (kn)                           | discarded             | stays
//   the normals (nr)                             | discarded             | replaced
//   the agreement (nr.a)                         | discarded             | discarded (it read the normals)
//   the clusters (cl)                            | discarded             | stay
//
// A producer clears its own flag when it starts: a point-mode query has none and discards nothing, a clusters call counts into buffers of its own and
// leaves the Count query, and the three producers of a mask share cx_mask_begin.  A new rule on the index adds one line to one of these two functions
// and nowhere else.
void cx_normals_changed(immesh_cloud_index* x) {
    x->nr.a.have = false;   // an agreement belongs to the normals it read
}

void cx_cloud_changed(immesh_cloud_index* x) {
    x->q.have = false;
    x->kn.have_knn = x->kn.have_count = x->kn.have_mask = false;
    x->nr.have = false;
    cx_normals_changed(x);
    x->cl.have = false;
}

// the hierarchy over r->vtx / r->faces (already on the device, queued on the caster's stream)
int rc_build(immesh_raycaster* r, int64_t n_vtx, int64_t n_faces) {
    r->built = false;
    rc_snapshot_changed(r);
    const RcLeaves src = {(const float*)r->vtx.p, n_vtx, (const int32_t*)r->faces.p};
    const int rc = rc_tree_build(r->ctx, "raycast", r->s, r->ev[0], r->ev[1], r->h_small, r->tree, n_faces, src);
    if (rc) return rc;
    (void)hipEventElapsedTime(&r->ms[0], r->ev[0], r->ev[1]);
    r->n_vtx = n_vtx; r->n_faces = n_faces;
    r->built = true;
    return 0;
}

extern "C" {

int immesh_ray_frame_from_state(const immesh_config* cfg, const double* state, immesh_ray_frame* frame) {
    if (!cfg || !state || !frame) return IMMESH_E_INVAL;
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++)
            frame->rot[3 * i + j] = (state[3 * i] * cfg->extR[j] + state[3 * i + 1] * cfg->extR[3 + j]) + state[3 * i + 2] * cfg->extR[6 + j];
        frame->pos[i] = ((state[3 * i] * cfg->extT[0] + state[3 * i + 1] * cfg->extT[1]) + state[3 * i + 2] * cfg->extT[2]) + state[9 + i];
    }
    return 0;
}

immesh_raycaster* immesh_raycaster_create(immesh_ctx* ctx) {
    if (!ctx) return nullptr;
    (void)hipSetDevice(ctx->cfg.device);
    immesh_raycaster* r = new immesh_raycaster();
    r->ctx = ctx;
    bool ok = hipStreamCreateWithFlags(&r->s, hipStreamNonBlocking) == hipSuccess;
    for (int i = 0; i < 6 && ok; i++) ok = hipEventCreate(&r->ev[i]) == hipSuccess;
    ok = ok && hipHostMalloc((void**)&r->h_small, 32) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        ctx->err = "immesh_raycaster_create: stream / event / pinned allocation failed";
        immesh_raycaster_destroy(r);
        return nullptr;
    }
    return r;
}

void immesh_raycaster_destroy(immesh_raycaster* r) {
    if (!r) return;
    (void)hipSetDevice(r->ctx->cfg.device);
    if (r->s) (void)hipStreamSynchronize(r->s);
    rc_destroy_events(r->ev, 6);
    if (r->h_small) (void)hipHostFree(r->h_small);
    if (r->s) (void)hipStreamDestroy(r->s);
    delete r;   // the records release their buffers, events and pinned words
}

int immesh_raycast_build_triangles(immesh_raycaster* r, const float* vtx_xyz, int64_t n_vtx, const int32_t* faces, int64_t n_faces) {
    if (!r) return IMMESH_E_INVAL;
    immesh_ctx* c = r->ctx;
    // before anything is touched: a refused soup leaves the built snapshot as it was
    int rc = rc_check_soup(c, "raycast_build_triangles", RC_MAX_FACES, vtx_xyz, n_vtx, faces, n_faces);
    if (rc) return rc;
    (void)hipSetDevice(c->cfg.device);
    r->built = false;
    if ((rc = rc_upload_soup(c, "raycast", r->s, r->vtx, r->faces, vtx_xyz, n_vtx, faces, n_faces))) return rc;
    return rc_build(r, n_vtx, n_faces);
}

int immesh_raycast_build_mesh(immesh_raycaster* r, double smooth_factor, int32_t knn) {
    if (!r) return IMMESH_E_INVAL;
    immesh_ctx* c = r->ctx;
    int64_t nv = 0, nf = 0;
    int rc = immesh_mesh_export(c, smooth_factor, knn, &nv, &nf);   // synchronises the ctx stream: the arrays are complete
    if (rc) return rc;
    if (nf > RC_MAX_FACES) { c->err = "raycast_build_mesh: more than 2^30 faces"; return IMMESH_E_CAPACITY; }
    const MeshHost& h = c->mesh_host;
    (void)hipSetDevice(c->cfg.device);
    r->built = false;
    if ((rc = rc_grow(c, "raycast", r->vtx, (size_t)nv * 12))) return rc;
    if ((rc = rc_grow(c, "raycast", r->faces, (size_t)nf * 12))) return rc;
    // the snapshot: the caster's own copies, complete before this call returns (rc_build synchronises), so the next export may overwrite its arrays
    if (nv > 0) HIPCHK(c, hipMemcpyAsync(r->vtx.p, h.exp_vtx, (size_t)nv * 12, hipMemcpyDeviceToDevice, r->s));
    if (nf > 0) HIPCHK(c, hipMemcpyAsync(r->faces.p, h.exp_faces, (size_t)nf * 12, hipMemcpyDeviceToDevice, r->s));
    return rc_build(r, nv, nf);
}

int immesh_raycast_sizes(immesh_raycaster* r, int64_t* n_vtx, int64_t* n_faces, int64_t* n_in_tree) {
    if (!r) return IMMESH_E_INVAL;
    if (!r->built) { r->ctx->err = "raycast_sizes: no hierarchy has been built"; return IMMESH_E_INVAL; }
    if (n_vtx) *n_vtx = r->n_vtx;
    if (n_faces) *n_faces = r->n_faces;
    if (n_in_tree) *n_in_tree = r->tree.n_in;
    return 0;
}

int immesh_raycast(immesh_raycaster* r, const immesh_ray_frame* frame, const float* dirs, const float* origins, int64_t n_rays, double t_min, double t_max,
                   int32_t mode, float* t_out, int32_t* face_out) {
    if (!r) return IMMESH_E_INVAL;
    immesh_ctx* c = r->ctx;
    int rc = rc_built(r, "raycast");
    if (rc) return rc;
    if (!frame) { c->err = "raycast: frame is NULL"; return IMMESH_E_INVAL; }
    if (n_rays < 0 || n_rays > (int64_t)0x7FFFFFFE || (n_rays > 0 && !dirs)) { c->err = "raycast: bad ray arrays"; return IMMESH_E_INVAL; }
    if (mode != IMMESH_RAY_NEAREST && mode != IMMESH_RAY_ANY) { c->err = "raycast: unknown mode " + std::to_string(mode); return IMMESH_E_INVAL; }
    if (!(t_min >= 0.0) || !(t_min < t_max) || !std::isfinite(t_max)) { c->err = "raycast: need 0 <= t_min < t_max, both finite"; return IMMESH_E_INVAL; }
    RcFrame fr;
    if ((rc = rc_frame(c, "raycast", frame, &fr))) return rc;
    (void)hipSetDevice(c->cfg.device);
    hipStream_t s = r->s;
    const int m = mode == IMMESH_RAY_NEAREST ? 0 : 1;   // an ANY cast leaves the last NEAREST cast's rays and distances where the reinforce pass reads them
    if (m == 0) { r->have_cast = false; r->n_points = 0; }
    if ((rc = rc_grow(c, "raycast", r->dirs[m], (size_t)n_rays * 12))) return rc;
    if (origins && (rc = rc_grow(c, "raycast", r->org[m], (size_t)n_rays * 12))) return rc;
    if ((rc = rc_grow(c, "raycast", r->t[m], (size_t)n_rays * 4))) return rc;
    if ((rc = rc_grow(c, "raycast", r->face[m], (size_t)n_rays * 4))) return rc;
    if (n_rays > 0) {
        HIPCHK(c, hipMemcpyAsync(r->dirs[m].p, dirs, (size_t)n_rays * 12, hipMemcpyHostToDevice, s));
        if (origins) HIPCHK(c, hipMemcpyAsync(r->org[m].p, origins, (size_t)n_rays * 12, hipMemcpyHostToDevice, s));
    }
    HIPCHK(c, hipEventRecord(r->ev[2], s));
    rc_launch_cast(s, fr, (const float*)r->dirs[m].p, origins ? (const float*)r->org[m].p : nullptr, n_rays, t_min, t_max, mode, (const float*)r->vtx.p,
                   (const int32_t*)r->faces.p, (const RcNode*)r->tree.nodes.p, r->tree.n_in, (float*)r->t[m].p, (int32_t*)r->face[m].p);
    if ((rc = rc_span_end(c, s, r->ev[2], r->ev[3], &r->ms[1]))) return rc;
    if (t_out && n_rays > 0) HIPCHK(c, hipMemcpy(t_out, r->t[m].p, (size_t)n_rays * 4, hipMemcpyDeviceToHost));
    if (face_out && n_rays > 0) HIPCHK(c, hipMemcpy(face_out, r->face[m].p, (size_t)n_rays * 4, hipMemcpyDeviceToHost));
    if (m == 0) { r->have_cast = true; r->have_origins = origins != nullptr; r->n_rays = n_rays; r->frame = fr; }
    return 0;
}

int immesh_raycast_points(immesh_raycaster* r, double downsample_res, float* xyz_out, int64_t cap, int64_t* n_out) {
    if (!r) return IMMESH_E_INVAL;
    immesh_ctx* c = r->ctx;
    if (std::isnan(downsample_res)) { c->err = "raycast_points: downsample_res is NaN"; return IMMESH_E_INVAL; }
    if (!r->have_cast) { c->err = "raycast_points: no NEAREST cast since the last build"; return IMMESH_E_INVAL; }
    (void)hipSetDevice(c->cfg.device);
    hipStream_t s = r->s;
    const int64_t n = r->n_rays;
    const float res = (float)downsample_res;
    r->n_points = 0;
    if (n > 0) {
        int rc;
        uint32_t mask = 0;
        RcThin& th = r->th;
        if ((rc = rc_thin_grow(c, "raycast", th, r->tree.temp, n, res, &mask))) return rc;
        const float* t = (const float*)r->t[0].p;   // the tail's depth array: -1 = no point
        HIPCHK(c, hipEventRecord(r->ev[4], s));
        rc_launch_points(s, r->frame, (const float*)r->dirs[0].p, r->have_origins ? (const float*)r->org[0].p : nullptr, n, res, t, (float*)th.pts.p,
                         (float*)th.cells.p, (int32_t*)th.keep.p);
        if ((rc = rc_thin_run(c, s, th, r->tree.temp, n, res, mask, t))) return rc;
        if ((rc = rc_span_end(c, s, r->ev[4], r->ev[5], &r->ms[2], r->h_small + 1, th.small.p, 8))) return rc;
        r->n_points = r->h_small[1];
    }
    return rc_thin_fetch(c, "raycast_points", r->th, r->n_points, xyz_out, cap, n_out);
}

int immesh_raycaster_last_timing(immesh_raycaster* r, float ms[3]) {
    if (!r || !ms) return IMMESH_E_INVAL;
    ms[0] = r->ms[0]; ms[1] = r->ms[1]; ms[2] = r->ms[2];
    return 0;
}

}  // extern "C"
