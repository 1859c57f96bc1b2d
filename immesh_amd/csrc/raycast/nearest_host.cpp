// Host side of the mesh-to-cloud distances (include/immesh_nearest.h): the cloud index (argument checks, grow-only buffers, the build, the queries and
// the reduction on the index's stream) and the sampler of a built caster's snapshot (on the caster's stream, in the caster's buffers).  Nothing here
// is allocated or launched unless an index is created or a sample is drawn.
#include <algorithm>
#include <cmath>
#include <string>
#include "../host_ctx.hpp"
#include "../../../include/immesh_closest.h"
#include "../../../include/immesh_nearest.h"
#include "../render/render.hpp"
#include "raycast.hpp"

namespace {

constexpr int64_t CN_MAX_POINTS = (int64_t)1 << RC_INDEX_BITS;

int cn_check_query(immesh_cloud_index* x, const char* who, double max_dist) {
    const int rc = cx_built(x, who);
    return rc ? rc : rc_positive(x->ctx, who, "max_dist", max_dist);
}

int cn_grow_results(immesh_cloud_index* x, size_t n) {
    immesh_ctx* c = x->ctx;
    RcDist& q = x->q;
    int rc;
    if ((rc = rc_grow(c, "cloud_index", q.d2, n * 8))) return rc;
    if ((rc = rc_grow(c, "cloud_index", q.dist, n * 4))) return rc;
    if ((rc = rc_grow(c, "cloud_index", q.id, n * 4))) return rc;
    if ((rc = rc_grow(c, "cloud_index", q.xyz, n * 12))) return rc;
    return rc_grow(c, "cloud_index", q.status, n);
}

// behind the traversal launch: the end of the query's span, the copies
int cn_finish_query(immesh_cloud_index* x, int64_t n_q, double* d2_out, float* dist_out, int32_t* index_out, float* xyz_out) {
    int rc;
    if ((rc = rc_span_end(x->ctx, x->s, x->ev[2], x->ev[3], &x->ms[1]))) return rc;
    if ((rc = rc_dist_copy(x->ctx, x->q, n_q, d2_out, dist_out, index_out, xyz_out))) return rc;
    x->q.n = n_q;
    x->q.have = true;
    return 0;
}

int ms_events(immesh_raycaster* r) {
    immesh_ctx* c = r->ctx;
    for (hipEvent_t& e : r->sm.ev)
        if (!e) HIPCHK(c, hipEventCreate(&e));
    if (!r->sm.done) HIPCHK(c, hipEventCreateWithFlags(&r->sm.done, hipEventDisableTiming));
    if (!r->sm.h_total) HIPCHK(c, hipHostMalloc((void**)&r->sm.h_total, 8));
    return 0;
}

}  // namespace

extern "C" {

// ---- the index ------------------------------------------------------------------------------------------------------------------------------
immesh_cloud_index* immesh_cloud_index_create(immesh_ctx* ctx) {
    if (!ctx) return nullptr;
    (void)hipSetDevice(ctx->cfg.device);
    immesh_cloud_index* x = new immesh_cloud_index();
    x->ctx = ctx;
    bool ok = hipStreamCreateWithFlags(&x->s, hipStreamNonBlocking) == hipSuccess;
    for (int i = 0; i < 6 && ok; i++) ok = hipEventCreate(&x->ev[i]) == hipSuccess;
    ok = ok && hipHostMalloc((void**)&x->h_small, 32) == hipSuccess;
    ok = ok && hipHostMalloc((void**)&x->q.h_res, sizeof(DqStatsDev)) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        ctx->err = "immesh_cloud_index_create: stream / event / pinned allocation failed";
        immesh_cloud_index_destroy(x);
        return nullptr;
    }
    return x;
}

void immesh_cloud_index_destroy(immesh_cloud_index* x) {
    if (!x) return;
    (void)hipSetDevice(x->ctx->cfg.device);
    if (x->s) (void)hipStreamSynchronize(x->s);
    rc_destroy_events(x->ev, 6);
    if (x->h_small) (void)hipHostFree(x->h_small);
    if (x->s) (void)hipStreamDestroy(x->s);
    delete x;   // the records release their buffers and pinned words
}

int immesh_cloud_index_build(immesh_cloud_index* x, const float* xyz, int64_t n_pts) {
    if (!x) return IMMESH_E_INVAL;
    immesh_ctx* c = x->ctx;
    // before anything is touched: a refused cloud leaves the built index as it was
    int rc;
    if ((rc = rc_points(c, "cloud_index_build", xyz, n_pts))) return rc;
    if (n_pts > CN_MAX_POINTS) { c->err = "cloud_index_build: more than 2^30 points"; return IMMESH_E_INVAL; }
    (void)hipSetDevice(c->cfg.device);
    x->built = false;
    cx_cloud_changed(x);   // every derived result belongs to the cloud it was made on
    if ((rc = rc_grow(c, "cloud_index", x->pts, (size_t)n_pts * 12))) return rc;
    if (n_pts > 0) HIPCHK(c, hipMemcpyAsync(x->pts.p, xyz, (size_t)n_pts * 12, hipMemcpyHostToDevice, x->s));
    const RcLeaves src = {(const float*)x->pts.p, n_pts, nullptr};
    if ((rc = rc_tree_build(c, "cloud_index", x->s, x->ev[0], x->ev[1], x->h_small, x->tree, n_pts, src))) return rc;
    (void)hipEventElapsedTime(&x->ms[0], x->ev[0], x->ev[1]);
    x->n_pts = n_pts;
    x->built = true;
    return 0;
}

int immesh_cloud_index_sizes(immesh_cloud_index* x, int64_t* n_pts, int64_t* n_in_tree) {
    if (!x) return IMMESH_E_INVAL;
    if (!x->built) { x->ctx->err = "cloud_index_sizes: no index has been built"; return IMMESH_E_INVAL; }
    if (n_pts) *n_pts = x->n_pts;
    if (n_in_tree) *n_in_tree = x->tree.n_in;
    return 0;
}

// ---- the queries ----------------------------------------------------------------------------------------------------------------------------
int immesh_nearest_points(immesh_cloud_index* x, const immesh_ray_frame* frame, const float* pts, int64_t n_q, double max_dist, double* d2_out,
                          float* dist_out, int32_t* index_out, float* xyz_out) {
    if (!x) return IMMESH_E_INVAL;
    immesh_ctx* c = x->ctx;
    int rc;
    if ((rc = cn_check_query(x, "nearest_points", max_dist))) return rc;
    if ((rc = rc_points(c, "nearest_points", pts, n_q))) return rc;
    RcFrame fr = {};
    if (frame && (rc = rc_frame(c, "nearest_points", frame, &fr))) return rc;
    (void)hipSetDevice(c->cfg.device);
    hipStream_t s = x->s;
    x->q.have = false;
    const size_t n = (size_t)n_q;
    if ((rc = rc_grow(c, "cloud_index", x->q_pts, n * 12))) return rc;
    if ((rc = cn_grow_results(x, n))) return rc;
    x->q_rc = nullptr;
    if (n_q > 0) HIPCHK(c, hipMemcpyAsync(x->q_pts.p, pts, n * 12, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipEventRecord(x->ev[2], s));
    cn_launch_nearest(s, fr, frame != nullptr, (const float*)x->q_pts.p, n_q, max_dist * max_dist, (const float*)x->pts.p, (const RcNode*)x->tree.nodes.p, x->tree.n_in,
                      (double*)x->q.d2.p, (float*)x->q.dist.p, (int32_t*)x->q.id.p, (float*)x->q.xyz.p, (uint8_t*)x->q.status.p);
    return cn_finish_query(x, n_q, d2_out, dist_out, index_out, xyz_out);
}

int immesh_nearest_samples(immesh_cloud_index* x, immesh_raycaster* r, double max_dist, double* d2_out, float* dist_out, int32_t* index_out, float* xyz_out) {
    if (!x) return IMMESH_E_INVAL;
    immesh_ctx* c = x->ctx;
    int rc;
    if ((rc = cx_caster(x, r, "nearest_samples")) || (rc = cn_check_query(x, "nearest_samples", max_dist)) || (rc = cx_caster_built(x, r, "nearest_samples", true)))
        return rc;
    (void)hipSetDevice(c->cfg.device);
    hipStream_t s = x->s;
    x->q.have = false;
    const int64_t n_q = r->sm.n;
    x->q_rc = r; x->q_gen = r->sm.gen;   // which samples this query reads (the agreement of include/immesh_normals.h asks)
    if ((rc = cn_grow_results(x, (size_t)n_q))) return rc;
    HIPCHK(c, hipStreamWaitEvent(s, r->sm.done, 0));   // the samples are complete before the traversal reads them
    HIPCHK(c, hipEventRecord(x->ev[2], s));
    cn_launch_nearest(s, RcFrame{}, 0, (const float*)r->sm.xyz.p, n_q, max_dist * max_dist, (const float*)x->pts.p, (const RcNode*)x->tree.nodes.p, x->tree.n_in,
                      (double*)x->q.d2.p, (float*)x->q.dist.p, (int32_t*)x->q.id.p, (float*)x->q.xyz.p, (uint8_t*)x->q.status.p);
    return cn_finish_query(x, n_q, d2_out, dist_out, index_out, xyz_out);
}

int immesh_nearest_reduce(immesh_cloud_index* x, double bin_width, int32_t n_bins, immesh_closest_stats* stats, int64_t* hist_out) {
    if (!x) return IMMESH_E_INVAL;
    return rc_dist_reduce(x->ctx, "nearest_stats", "cloud_index", "no nearest-point query has been made on this index", x->s, x->ev[4], x->ev[5], &x->ms[2],
                          x->q, bin_width, n_bins, stats, hist_out);
}

int immesh_nearest_last_timing(immesh_cloud_index* x, float ms[3]) {
    if (!x || !ms) return IMMESH_E_INVAL;
    ms[0] = x->ms[0]; ms[1] = x->ms[1]; ms[2] = x->ms[2];
    return 0;
}

// ---- the sampler ----------------------------------------------------------------------------------------------------------------------------
int immesh_mesh_sample(immesh_raycaster* r, double density, uint64_t seed, float* xyz_out, int32_t* face_out, int64_t cap, int64_t* n_out) {
    if (!r) return IMMESH_E_INVAL;
    immesh_ctx* c = r->ctx;
    RcSample& q = r->sm;
    int rc;
    if ((rc = rc_built(r, "mesh_sample"))) return rc;
    if ((rc = rc_positive(c, "mesh_sample", "density", density))) return rc;
    (void)hipSetDevice(c->cfg.device);
    hipStream_t s = r->s;
    q.have = false; q.n = 0;
    if ((rc = ms_events(r))) return rc;
    const int64_t nf = r->n_faces;
    if ((rc = rc_grow(c, "raycast", q.cnt, (size_t)nf * 4))) return rc;
    if ((rc = rc_grow(c, "raycast", q.off, (size_t)nf * 4))) return rc;
    if ((rc = rc_grow(c, "raycast", q.total, 8))) return rc;
    if ((rc = rc_grow(c, "raycast", r->tree.temp, rd_scan_temp_bytes(1, 1, std::max<int64_t>(nf, 1)) + 256))) return rc;
    HIPCHK(c, hipEventRecord(q.ev[0], s));
    HIPCHK(c, hipMemsetAsync(q.total.p, 0, 8, s));
    ms_launch_count(s, (const float*)r->vtx.p, r->n_vtx, (const int32_t*)r->faces.p, nf, density, seed, (int32_t*)q.cnt.p, (unsigned long long*)q.total.p);
    if ((rc = rc_span_end(c, s, q.ev[0], q.ev[1], &q.ms[0], q.h_total, q.total.p, 8))) return rc;   // the one count the host needs: it sizes the samples
    const int64_t total = q.h_total[0];
    if (total < 0 || total > RC_MAX_COUNT) {
        c->err = "mesh_sample: too many samples (" + std::to_string(total) + " > 2^31 - 2)";
        return IMMESH_E_CAPACITY;
    }
    if ((rc = rc_grow(c, "raycast", q.xyz, (size_t)total * 12))) return rc;
    if ((rc = rc_grow(c, "raycast", q.face, (size_t)total * 4))) return rc;
    HIPCHK(c, hipEventRecord(q.ev[2], s));
    if (nf > 0) rd_scan_i32(s, r->tree.temp.p, r->tree.temp.bytes, (const int32_t*)q.cnt.p, (int32_t*)q.off.p, nf);
    ms_launch_emit(s, (const float*)r->vtx.p, (const int32_t*)r->faces.p, nf, seed, (const int32_t*)q.off.p, total, (float*)q.xyz.p, (int32_t*)q.face.p);
    HIPCHK(c, hipEventRecord(q.ev[3], s));
    HIPCHK(c, hipEventRecord(q.done, s));
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(s));
    (void)hipEventElapsedTime(&q.ms[1], q.ev[2], q.ev[3]);
    q.n = total;
    q.have = true;
    q.gen++;
    if (n_out) *n_out = total;
    if ((!xyz_out && !face_out) || total == 0) return 0;
    if (cap < total) {
        c->err = "mesh_sample: cap " + std::to_string(cap) + " < " + std::to_string(total) + " samples";
        return IMMESH_E_CAPACITY;
    }
    if (xyz_out) HIPCHK(c, hipMemcpy(xyz_out, q.xyz.p, (size_t)total * 12, hipMemcpyDeviceToHost));
    if (face_out) HIPCHK(c, hipMemcpy(face_out, q.face.p, (size_t)total * 4, hipMemcpyDeviceToHost));
    return 0;
}

int immesh_mesh_sample_count(immesh_raycaster* r, int64_t* n_out) {
    if (!r) return IMMESH_E_INVAL;
    if (!r->built || !r->sm.have) { r->ctx->err = "mesh_sample_count: no samples since the caster's last build (immesh_mesh_sample)"; return IMMESH_E_INVAL; }
    if (n_out) *n_out = r->sm.n;
    return 0;
}

int immesh_mesh_sample_last_timing(immesh_raycaster* r, float ms[2]) {
    if (!r || !ms) return IMMESH_E_INVAL;
    ms[0] = r->sm.ms[0]; ms[1] = r->sm.ms[1];
    return 0;
}

}  // extern "C"
