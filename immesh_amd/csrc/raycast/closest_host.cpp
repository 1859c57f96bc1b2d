// Host side of the closest-point queries (include/immesh_closest.h) on a built ray caster: argument checks, grow-only buffers, the query and the
// reduction on the caster's stream.  Nothing here is allocated or launched unless a query is made.
#include <cmath>
#include <cstring>
#include <string>
#include "../host_ctx.hpp"
#include "../../../include/immesh_closest.h"
#include "raycast.hpp"

namespace {

int cl_events(immesh_raycaster* r) {
    immesh_ctx* c = r->ctx;
    for (hipEvent_t& e : r->cl.ev)
        if (!e) HIPCHK(c, hipEventCreate(&e));
    if (!r->cl.h_res) HIPCHK(c, hipHostMalloc((void**)&r->cl.h_res, sizeof(ClStatsDev)));
    return 0;
}

}  // namespace

extern "C" {

int immesh_closest_points(immesh_raycaster* r, const immesh_ray_frame* frame, const float* pts, int64_t n_pts, double max_dist, double* d2_out,
                          float* dist_out, int32_t* face_out, float* xyz_out, int8_t* side_out) {
    if (!r) return IMMESH_E_INVAL;
    immesh_ctx* c = r->ctx;
    RcClosest& q = r->cl;
    if (!r->built) { c->err = "closest_points: no hierarchy has been built (immesh_raycast_build_triangles / _build_mesh)"; return IMMESH_E_INVAL; }
    if (n_pts < 0 || n_pts > (int64_t)0x7FFFFFFE || (n_pts > 0 && !pts)) { c->err = "closest_points: bad point array"; return IMMESH_E_INVAL; }
    if (!(max_dist > 0.0) || !std::isfinite(max_dist)) { c->err = "closest_points: need 0 < max_dist, finite"; return IMMESH_E_INVAL; }
    RcFrame fr = {};
    if (frame) {
        for (int i = 0; i < 9; i++)
            if (!std::isfinite(frame->rot[i])) { c->err = "closest_points: frame rotation is not finite"; return IMMESH_E_INVAL; }
        for (int i = 0; i < 3; i++)
            if (!std::isfinite(frame->pos[i])) { c->err = "closest_points: frame position is not finite"; return IMMESH_E_INVAL; }
        std::memcpy(fr.rot, frame->rot, sizeof(fr.rot));
        std::memcpy(fr.pos, frame->pos, sizeof(fr.pos));
    }
    (void)hipSetDevice(c->cfg.device);
    hipStream_t s = r->s;
    int rc;
    q.have_query = false;
    if ((rc = cl_events(r))) return rc;
    const size_t n = (size_t)n_pts;
    if ((rc = rc_grow(r, q.pts, n * 12))) return rc;
    if ((rc = rc_grow(r, q.d2, n * 8))) return rc;
    if ((rc = rc_grow(r, q.dist, n * 4))) return rc;
    if ((rc = rc_grow(r, q.face, n * 4))) return rc;
    if ((rc = rc_grow(r, q.xyz, n * 12))) return rc;
    if ((rc = rc_grow(r, q.side, n))) return rc;
    if ((rc = rc_grow(r, q.status, n))) return rc;
    if (n_pts > 0) HIPCHK(c, hipMemcpyAsync(q.pts.p, pts, n * 12, hipMemcpyHostToDevice, s));
    const double r2 = max_dist * max_dist;
    HIPCHK(c, hipEventRecord(q.ev[0], s));
    cl_launch_query(s, fr, frame != nullptr, (const float*)q.pts.p, n_pts, r2, (const float*)r->vtx.p,
                    (const int32_t*)r->faces.p, (const RcNode*)r->nodes.p, r->n_in, (double*)q.d2.p, (float*)q.dist.p, (int32_t*)q.face.p, (float*)q.xyz.p,
                    (int8_t*)q.side.p, (uint8_t*)q.status.p);
    HIPCHK(c, hipEventRecord(q.ev[1], s));
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(s));
    (void)hipEventElapsedTime(&q.ms[0], q.ev[0], q.ev[1]);
    if (n_pts > 0) {
        if (d2_out) HIPCHK(c, hipMemcpy(d2_out, q.d2.p, n * 8, hipMemcpyDeviceToHost));
        if (dist_out) HIPCHK(c, hipMemcpy(dist_out, q.dist.p, n * 4, hipMemcpyDeviceToHost));
        if (face_out) HIPCHK(c, hipMemcpy(face_out, q.face.p, n * 4, hipMemcpyDeviceToHost));
        if (xyz_out) HIPCHK(c, hipMemcpy(xyz_out, q.xyz.p, n * 12, hipMemcpyDeviceToHost));
        if (side_out) HIPCHK(c, hipMemcpy(side_out, q.side.p, n, hipMemcpyDeviceToHost));
    }
    q.n_pts = n_pts;
    q.have_query = true;
    return 0;
}

int immesh_closest_reduce(immesh_raycaster* r, double bin_width, int32_t n_bins, immesh_closest_stats* stats, int64_t* hist_out) {
    if (!r) return IMMESH_E_INVAL;
    immesh_ctx* c = r->ctx;
    RcClosest& q = r->cl;
    if (!(bin_width > 0.0) || !std::isfinite(bin_width)) { c->err = "closest_stats: need 0 < bin_width, finite"; return IMMESH_E_INVAL; }
    if (n_bins < 1 || n_bins > (1 << 20)) { c->err = "closest_stats: n_bins " + std::to_string(n_bins) + " outside [1, 2^20]"; return IMMESH_E_INVAL; }
    if (!q.have_query) { c->err = "closest_stats: no closest-point query has been made on this caster"; return IMMESH_E_INVAL; }
    (void)hipSetDevice(c->cfg.device);
    hipStream_t s = r->s;
    int rc;
    const int64_t blocks = cl_stats_blocks(q.n_pts);
    const size_t hist_bytes = ((size_t)n_bins + 1) * 8;
    if ((rc = rc_grow(r, q.part, (size_t)blocks * sizeof(ClStatsDev)))) return rc;
    if ((rc = rc_grow(r, q.hist, hist_bytes))) return rc;
    if ((rc = rc_grow(r, q.res, sizeof(ClStatsDev)))) return rc;
    const float bw = (float)bin_width;
    HIPCHK(c, hipEventRecord(q.ev[2], s));
    HIPCHK(c, hipMemsetAsync(q.hist.p, 0, hist_bytes, s));
    cl_launch_stats(s, (const float*)q.dist.p, (const uint8_t*)q.status.p, q.n_pts, bw, n_bins, (ClStatsDev*)q.part.p, (unsigned long long*)q.hist.p,
                    (ClStatsDev*)q.res.p);
    HIPCHK(c, hipEventRecord(q.ev[3], s));
    HIPCHK(c, hipMemcpyAsync(q.h_res, q.res.p, sizeof(ClStatsDev), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(s));
    (void)hipEventElapsedTime(&q.ms[1], q.ev[2], q.ev[3]);
    int64_t overflow = 0;
    HIPCHK(c, hipMemcpy(&overflow, (const char*)q.hist.p + (size_t)n_bins * 8, 8, hipMemcpyDeviceToHost));
    if (hist_out) HIPCHK(c, hipMemcpy(hist_out, q.hist.p, (size_t)n_bins * 8, hipMemcpyDeviceToHost));
    if (stats) {
        const ClStatsDev& d = *q.h_res;
        stats->n_points = q.n_pts;
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

int immesh_closest_last_timing(immesh_raycaster* r, float ms[2]) {
    if (!r || !ms) return IMMESH_E_INVAL;
    ms[0] = r->cl.ms[0]; ms[1] = r->cl.ms[1];
    return 0;
}

}  // extern "C"
