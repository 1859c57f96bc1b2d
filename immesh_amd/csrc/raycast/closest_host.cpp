// Host side of the closest-point queries (include/immesh_closest.h) on a built ray caster: argument checks, grow-only buffers, the query and the
// reduction on the caster's stream; and what a distance query's record (RcDist) shares with the cloud index: the result copies and the reduction.
// Nothing here is allocated or launched unless a query is made.
#include <cmath>
#include <string>
#include "../host_ctx.hpp"
#include "../../../include/immesh_closest.h"
#include "raycast.hpp"

int rc_dist_copy(immesh_ctx* c, const RcDist& q, int64_t n_q, double* d2_out, float* dist_out, int32_t* id_out, float* xyz_out) {
    const size_t n = (size_t)n_q;
    if (n == 0) return 0;
    if (d2_out) HIPCHK(c, hipMemcpy(d2_out, q.d2.p, n * 8, hipMemcpyDeviceToHost));
    if (dist_out) HIPCHK(c, hipMemcpy(dist_out, q.dist.p, n * 4, hipMemcpyDeviceToHost));
    if (id_out) HIPCHK(c, hipMemcpy(id_out, q.id.p, n * 4, hipMemcpyDeviceToHost));
    if (xyz_out) HIPCHK(c, hipMemcpy(xyz_out, q.xyz.p, n * 12, hipMemcpyDeviceToHost));
    return 0;
}

int rc_dist_reduce(immesh_ctx* c, const char* who, const char* grow_who, const char* none, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1, float* ms,
                   RcDist& q, double bin_width, int32_t n_bins, immesh_closest_stats* stats, int64_t* hist_out) {
    int rc;
    if ((rc = rc_positive(c, who, "bin_width", bin_width))) return rc;
    if (n_bins < 1 || n_bins > (1 << 20)) { c->err = std::string(who) + ": n_bins " + std::to_string(n_bins) + " outside [1, 2^20]"; return IMMESH_E_INVAL; }
    if ((rc = rc_have(c, who, q.have, none))) return rc;
    (void)hipSetDevice(c->cfg.device);
    const int64_t blocks = dq_stats_blocks(q.n);
    const size_t hist_bytes = ((size_t)n_bins + 1) * 8;
    if ((rc = rc_grow(c, grow_who, q.part, (size_t)blocks * sizeof(DqStatsDev)))) return rc;
    if ((rc = rc_grow(c, grow_who, q.hist, hist_bytes))) return rc;
    if ((rc = rc_grow(c, grow_who, q.res, sizeof(DqStatsDev)))) return rc;
    const float bw = (float)bin_width;
    HIPCHK(c, hipEventRecord(ev0, s));
    HIPCHK(c, hipMemsetAsync(q.hist.p, 0, hist_bytes, s));
    dq_launch_stats(s, (const float*)q.dist.p, (const uint8_t*)q.status.p, q.n, bw, n_bins, (DqStatsDev*)q.part.p, (unsigned long long*)q.hist.p,
                    (DqStatsDev*)q.res.p);
    if ((rc = rc_span_end(c, s, ev0, ev1, ms, q.h_res, q.res.p, sizeof(DqStatsDev)))) return rc;
    int64_t overflow = 0;
    HIPCHK(c, hipMemcpy(&overflow, (const char*)q.hist.p + (size_t)n_bins * 8, 8, hipMemcpyDeviceToHost));
    if (hist_out) HIPCHK(c, hipMemcpy(hist_out, q.hist.p, (size_t)n_bins * 8, hipMemcpyDeviceToHost));
    if (stats) {
        const DqStatsDev& d = *q.h_res;
        stats->n_points = q.n;
        stats->n_with_face = d.n_face;
        stats->n_not_finite = d.n_not_finite;
        stats->n_no_face = d.n_no_face;
        stats->n_overflow = overflow;
        stats->sum_dist = d.sum;
        stats->sum_dist2 = d.sum2;
        stats->mean = d.n_face > 0 ? d.sum / (double)d.n_face : 0.0;
        stats->rms = d.n_face > 0 ? std::sqrt(d.sum2 / (double)d.n_face) : 0.0;
        stats->max_dist = d.max_dist;
        stats->bin_width = bw;
    }
    return 0;
}

namespace {

int rc_closest_events(immesh_raycaster* r) {
    immesh_ctx* c = r->ctx;
    for (hipEvent_t& e : r->cl.ev)
        if (!e) HIPCHK(c, hipEventCreate(&e));
    if (!r->cl.q.h_res) HIPCHK(c, hipHostMalloc((void**)&r->cl.q.h_res, sizeof(DqStatsDev)));
    return 0;
}

}  // namespace

extern "C" {

int immesh_closest_points(immesh_raycaster* r, const immesh_ray_frame* frame, const float* pts, int64_t n_pts, double max_dist, double* d2_out,
                          float* dist_out, int32_t* face_out, float* xyz_out, int8_t* side_out) {
    if (!r) return IMMESH_E_INVAL;
    immesh_ctx* c = r->ctx;
    RcClosest& cl = r->cl;
    RcDist& q = cl.q;
    int rc;
    if ((rc = rc_built(r, "closest_points"))) return rc;
    if ((rc = rc_points(c, "closest_points", pts, n_pts)) || (rc = rc_positive(c, "closest_points", "max_dist", max_dist))) return rc;
    RcFrame fr = {};
    if (frame && (rc = rc_frame(c, "closest_points", frame, &fr))) return rc;
    (void)hipSetDevice(c->cfg.device);
    hipStream_t s = r->s;
    q.have = false;
    if ((rc = rc_closest_events(r))) return rc;
    const size_t n = (size_t)n_pts;
    if ((rc = rc_grow(c, "raycast", cl.pts, n * 12))) return rc;
    if ((rc = rc_grow(c, "raycast", q.d2, n * 8))) return rc;
    if ((rc = rc_grow(c, "raycast", q.dist, n * 4))) return rc;
    if ((rc = rc_grow(c, "raycast", q.id, n * 4))) return rc;
    if ((rc = rc_grow(c, "raycast", q.xyz, n * 12))) return rc;
    if ((rc = rc_grow(c, "raycast", cl.side, n))) return rc;
    if ((rc = rc_grow(c, "raycast", q.status, n))) return rc;
    if (n_pts > 0) HIPCHK(c, hipMemcpyAsync(cl.pts.p, pts, n * 12, hipMemcpyHostToDevice, s));
    const double r2 = max_dist * max_dist;
    HIPCHK(c, hipEventRecord(cl.ev[0], s));
    rc_launch_closest(s, fr, frame != nullptr, (const float*)cl.pts.p, n_pts, r2, (const float*)r->vtx.p, (const int32_t*)r->faces.p,
                      (const RcNode*)r->tree.nodes.p, r->tree.n_in, (double*)q.d2.p, (float*)q.dist.p, (int32_t*)q.id.p, (float*)q.xyz.p, (int8_t*)cl.side.p,
                      (uint8_t*)q.status.p);
    if ((rc = rc_span_end(c, s, cl.ev[0], cl.ev[1], &cl.ms[0]))) return rc;
    if ((rc = rc_dist_copy(c, q, n_pts, d2_out, dist_out, face_out, xyz_out))) return rc;
    if (side_out && n_pts > 0) HIPCHK(c, hipMemcpy(side_out, cl.side.p, n, hipMemcpyDeviceToHost));
    q.n = n_pts;
    q.have = true;
    return 0;
}

int immesh_closest_reduce(immesh_raycaster* r, double bin_width, int32_t n_bins, immesh_closest_stats* stats, int64_t* hist_out) {
    if (!r) return IMMESH_E_INVAL;
    RcClosest& cl = r->cl;
    return rc_dist_reduce(r->ctx, "closest_stats", "raycast", "no closest-point query has been made on this caster", r->s, cl.ev[2], cl.ev[3], &cl.ms[1], cl.q,
                          bin_width, n_bins, stats, hist_out);
}

int immesh_closest_last_timing(immesh_raycaster* r, float ms[2]) {
    if (!r || !ms) return IMMESH_E_INVAL;
    ms[0] = r->cl.ms[0]; ms[1] = r->cl.ms[1];
    return 0;
}

}  // extern "C"
