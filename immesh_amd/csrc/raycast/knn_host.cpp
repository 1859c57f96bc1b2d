// Host side of the k nearest neighbours, the radius counts, the two outlier rules and their apply on a cloud index (include/immesh_nearest.h, the
// Neighbours, Count and Outliers rules): argument checks, grow-only buffers and the launches on the index's stream.  Every check stands before the
// first launch and before anything of the index is touched, so a refused call leaves the index as it was.  Nothing here is allocated or launched
// unless one of these entry points is called.
#include <algorithm>
#include <cmath>
#include <string>
#include "../host_ctx.hpp"
#include "../../../include/immesh_closest.h"
#include "../../../include/immesh_nearest.h"
#include "../render/render.hpp"
#include "raycast.hpp"

namespace {

constexpr int64_t KN_MAX_QUERY = (int64_t)0x7FFFFFFE;
constexpr int32_t KN_MAX_K = 64;

int kn_check(immesh_cloud_index* x, const char* who, const char* what, double dist) {
    immesh_ctx* c = x->ctx;
    if (!x->built) { c->err = std::string(who) + ": no index has been built (immesh_cloud_index_build)"; return IMMESH_E_INVAL; }
    if (!(dist > 0.0) || !std::isfinite(dist)) { c->err = std::string(who) + ": need 0 < " + what + ", finite"; return IMMESH_E_INVAL; }
    return 0;
}

int kn_check_k(immesh_cloud_index* x, const char* who, int32_t k) {
    if (k < 1 || k > KN_MAX_K) { x->ctx->err = std::string(who) + ": need 1 <= k <= 64, got " + std::to_string(k); return IMMESH_E_INVAL; }
    return 0;
}

int kn_check_points(immesh_cloud_index* x, const char* who, const immesh_ray_frame* frame, const float* pts, int64_t n, RcFrame* fr) {
    if (n < 0 || n > KN_MAX_QUERY || (n > 0 && !pts)) { x->ctx->err = std::string(who) + ": bad point array"; return IMMESH_E_INVAL; }
    if (frame) return rc_frame(x->ctx, who, frame, fr);
    return 0;
}

// the events and the pinned counts, at the first call
int kn_ready(immesh_cloud_index* x) {
    immesh_ctx* c = x->ctx;
    (void)hipSetDevice(c->cfg.device);
    for (hipEvent_t& e : x->kn.ev)
        if (!e) HIPCHK(c, hipEventCreate(&e));
    if (!x->kn.h_cnt) HIPCHK(c, hipHostMalloc((void**)&x->kn.h_cnt, 4 * 8));
    return 0;
}

// the query points of a point-mode call on the device
int kn_upload(immesh_cloud_index* x, const float* pts, int64_t n) {
    immesh_ctx* c = x->ctx;
    const int rc = rc_grow(c, "cloud_index", x->kn.pts, (size_t)n * 12);
    if (rc) return rc;
    if (n > 0) HIPCHK(c, hipMemcpyAsync(x->kn.pts.p, pts, (size_t)n * 12, hipMemcpyHostToDevice, x->s));
    return 0;
}

// behind a traversal launch: the end event, the wait, the span
int kn_finish(immesh_cloud_index* x) {
    immesh_ctx* c = x->ctx;
    HIPCHK(c, hipEventRecord(x->kn.ev[1], x->s));
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(x->s));
    (void)hipEventElapsedTime(&x->kn.ms[0], x->kn.ev[0], x->kn.ev[1]);
    return 0;
}

// the Neighbours query behind its checks.  mode 0 / 1: n host points without / with a frame; mode 2: the cloud itself
int kn_knn(immesh_cloud_index* x, int mode, const RcFrame& fr, const float* pts, int64_t n, int32_t k, double max_dist, int32_t* count_out, int32_t* index_out,
           double* d2_out, double* mean_out) {
    immesh_ctx* c = x->ctx;
    RcKnn& q = x->kn;
    int rc;
    if ((rc = kn_ready(x))) return rc;
    if (mode == 2) q.have_knn = false;
    const bool lists = index_out || d2_out;
    const size_t m = (size_t)n, mk = m * (size_t)k;
    RcBuf& status = mode == 2 ? q.status : q.pstatus;
    if (mode != 2 && (rc = kn_upload(x, pts, n))) return rc;
    if ((rc = rc_grow(c, "cloud_index", q.cnt, m * 4))) return rc;
    if ((rc = rc_grow(c, "cloud_index", status, m))) return rc;
    if (mode == 2 && (rc = rc_grow(c, "cloud_index", q.mean, m * 8))) return rc;
    if (lists && ((rc = rc_grow(c, "cloud_index", q.idx, mk * 4)) || (rc = rc_grow(c, "cloud_index", q.d2, mk * 8)))) return rc;
    HIPCHK(c, hipEventRecord(q.ev[0], x->s));
    kn_launch_knn(x->s, fr, mode, mode == 2 ? (const float*)x->pts.p : (const float*)q.pts.p, n, k, max_dist * max_dist, (const float*)x->pts.p,
                  (const RcNode*)x->tree.nodes.p, x->tree.n_in, (int32_t*)q.cnt.p, lists ? (int32_t*)q.idx.p : nullptr, lists ? (double*)q.d2.p : nullptr,
                  (double*)q.mean.p, (uint8_t*)status.p);
    if ((rc = kn_finish(x))) return rc;
    if ((rc = rc_fetch(c, count_out, q.cnt.p, m * 4))) return rc;
    if ((rc = rc_fetch(c, index_out, q.idx.p, mk * 4))) return rc;
    if ((rc = rc_fetch(c, d2_out, q.d2.p, mk * 8))) return rc;
    if (mode == 2) {
        if ((rc = rc_fetch(c, mean_out, q.mean.p, m * 8))) return rc;
        q.have_knn = true;
    }
    return 0;
}

int kn_count(immesh_cloud_index* x, int mode, const RcFrame& fr, const float* pts, int64_t n, double radius, int32_t* count_out) {
    immesh_ctx* c = x->ctx;
    RcKnn& q = x->kn;
    int rc;
    if ((rc = kn_ready(x))) return rc;
    if (mode == 2) q.have_count = false;
    RcBuf& cnt = mode == 2 ? q.rcnt : q.cnt;
    RcBuf& status = mode == 2 ? q.rstatus : q.pstatus;
    if (mode != 2 && (rc = kn_upload(x, pts, n))) return rc;
    if ((rc = rc_grow(c, "cloud_index", cnt, (size_t)n * 4))) return rc;
    if ((rc = rc_grow(c, "cloud_index", status, (size_t)n))) return rc;
    HIPCHK(c, hipEventRecord(q.ev[0], x->s));
    kn_launch_count(x->s, fr, mode, mode == 2 ? (const float*)x->pts.p : (const float*)q.pts.p, n, radius * radius, (const float*)x->pts.p,
                    (const RcNode*)x->tree.nodes.p, x->tree.n_in, (int32_t*)cnt.p, (uint8_t*)status.p);
    if ((rc = kn_finish(x))) return rc;
    if ((rc = rc_fetch(c, count_out, cnt.p, (size_t)n * 4))) return rc;
    if (mode == 2) q.have_count = true;
    return 0;
}

// a mask launch between its events; statistical: count == nullptr
int kn_mask(immesh_cloud_index* x, const int32_t* count, const uint8_t* status, double threshold, int32_t min_neighbours, int64_t counts[4], uint8_t* keep_out) {
    immesh_ctx* c = x->ctx;
    RcKnn& q = x->kn;
    const int64_t n = x->n_pts;
    int rc;
    q.have_mask = false;
    if ((rc = rc_grow(c, "cloud_index", q.flag, (size_t)n * 4))) return rc;
    if ((rc = rc_grow(c, "cloud_index", q.keep8, (size_t)n))) return rc;
    if ((rc = rc_grow(c, "cloud_index", q.mcnt, 4 * 8))) return rc;
    unsigned long long* cnt = (unsigned long long*)q.mcnt.p;
    HIPCHK(c, hipEventRecord(q.ev[2], x->s));
    HIPCHK(c, hipMemsetAsync(cnt, 0, 4 * 8, x->s));
    if (count) kn_launch_mask_radius(x->s, count, status, n, min_neighbours, (int32_t*)q.flag.p, (uint8_t*)q.keep8.p, cnt);
    else kn_launch_mask_statistical(x->s, (const double*)q.mean.p, status, n, threshold, (int32_t*)q.flag.p, (uint8_t*)q.keep8.p, cnt);
    HIPCHK(c, hipEventRecord(q.ev[3], x->s));
    HIPCHK(c, hipMemcpyAsync(q.h_cnt, cnt, 4 * 8, hipMemcpyDeviceToHost, x->s));
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(x->s));
    (void)hipEventElapsedTime(&q.ms[1], q.ev[2], q.ev[3]);
    q.n_kept = (int64_t)q.h_cnt[0];
    q.have_mask = true;
    if (counts)
        for (int i = 0; i < 4; i++) counts[i] = (int64_t)q.h_cnt[i];
    return rc_fetch(c, keep_out, q.keep8.p, (size_t)n);
}

}  // namespace

extern "C" {

int immesh_knn_points(immesh_cloud_index* x, const immesh_ray_frame* frame, const float* pts, int64_t n, int32_t k, double max_dist, int32_t* count_out,
                      int32_t* index_out, double* d2_out) {
    if (!x) return IMMESH_E_INVAL;
    int rc;
    RcFrame fr = {};
    if ((rc = kn_check(x, "knn_points", "max_dist", max_dist)) || (rc = kn_check_k(x, "knn_points", k)) ||
        (rc = kn_check_points(x, "knn_points", frame, pts, n, &fr)))
        return rc;
    return kn_knn(x, frame ? 1 : 0, fr, pts, n, k, max_dist, count_out, index_out, d2_out, nullptr);
}

int immesh_knn_cloud(immesh_cloud_index* x, int32_t k, double max_dist, int32_t* count_out, int32_t* index_out, double* d2_out, double* mean_out) {
    if (!x) return IMMESH_E_INVAL;
    int rc;
    if ((rc = kn_check(x, "knn_cloud", "max_dist", max_dist)) || (rc = kn_check_k(x, "knn_cloud", k))) return rc;
    return kn_knn(x, 2, RcFrame{}, nullptr, x->n_pts, k, max_dist, count_out, index_out, d2_out, mean_out);
}

int immesh_radius_count_points(immesh_cloud_index* x, const immesh_ray_frame* frame, const float* pts, int64_t n, double radius, int32_t* count_out) {
    if (!x) return IMMESH_E_INVAL;
    int rc;
    RcFrame fr = {};
    if ((rc = kn_check(x, "radius_count_points", "radius", radius)) || (rc = kn_check_points(x, "radius_count_points", frame, pts, n, &fr))) return rc;
    return kn_count(x, frame ? 1 : 0, fr, pts, n, radius, count_out);
}

int immesh_radius_count_cloud(immesh_cloud_index* x, double radius, int32_t* count_out) {
    if (!x) return IMMESH_E_INVAL;
    int rc;
    if ((rc = kn_check(x, "radius_count_cloud", "radius", radius))) return rc;
    return kn_count(x, 2, RcFrame{}, nullptr, x->n_pts, radius, count_out);
}

int immesh_cloud_outliers_statistical(immesh_cloud_index* x, double mult, double* mu_out, double* sigma_out, double* threshold_out, int64_t counts[4],
                                      uint8_t* keep_out) {
    if (!x) return IMMESH_E_INVAL;
    immesh_ctx* c = x->ctx;
    RcKnn& q = x->kn;
    if (!x->built) { c->err = "cloud_outliers_statistical: no index has been built (immesh_cloud_index_build)"; return IMMESH_E_INVAL; }
    if (!q.have_knn) { c->err = "cloud_outliers_statistical: no immesh_knn_cloud query since the index's last build or apply"; return IMMESH_E_INVAL; }
    if (!(mult >= 0.0) || !std::isfinite(mult)) { c->err = "cloud_outliers_statistical: need 0 <= mult, finite"; return IMMESH_E_INVAL; }
    (void)hipSetDevice(c->cfg.device);
    // the Outliers rule's mu and sigma: exact host code over the means, read back once (a mean is -1 exactly when count == 0, else >= 0)
    const int64_t n = x->n_pts;
    q.h_mean.resize((size_t)n);
    int rc;
    if ((rc = rc_fetch(c, q.h_mean.data(), q.mean.p, (size_t)n * 8))) return rc;
    int64_t n_used = 0;
    double sum = 0.0;
    for (int64_t i = 0; i < n; i++)
        if (q.h_mean[i] >= 0.0) { sum += q.h_mean[i]; n_used++; }
    const double mu = n_used > 0 ? sum / (double)n_used : 0.0;
    double sq = 0.0;
    for (int64_t i = 0; i < n; i++)
        if (q.h_mean[i] >= 0.0) { const double t = q.h_mean[i] - mu; sq += t * t; }
    const double sigma = n_used > 1 ? std::sqrt(sq / (double)(n_used - 1)) : 0.0;
    const double threshold = mu + mult * sigma;
    if (mu_out) *mu_out = mu;
    if (sigma_out) *sigma_out = sigma;
    if (threshold_out) *threshold_out = threshold;
    return kn_mask(x, nullptr, (const uint8_t*)q.status.p, threshold, 0, counts, keep_out);
}

int immesh_cloud_outliers_radius(immesh_cloud_index* x, int64_t min_neighbours, int64_t counts[4], uint8_t* keep_out) {
    if (!x) return IMMESH_E_INVAL;
    immesh_ctx* c = x->ctx;
    RcKnn& q = x->kn;
    if (!x->built) { c->err = "cloud_outliers_radius: no index has been built (immesh_cloud_index_build)"; return IMMESH_E_INVAL; }
    if (!q.have_count) { c->err = "cloud_outliers_radius: no immesh_radius_count_cloud query since the index's last build or apply"; return IMMESH_E_INVAL; }
    if (min_neighbours < 0 || min_neighbours > KN_MAX_QUERY) { c->err = "cloud_outliers_radius: need min_neighbours in [0, 2^31 - 2]"; return IMMESH_E_INVAL; }
    (void)hipSetDevice(c->cfg.device);
    return kn_mask(x, (const int32_t*)q.rcnt.p, (const uint8_t*)q.rstatus.p, 0.0, (int32_t)min_neighbours, counts, keep_out);
}

int immesh_cloud_index_apply_outliers(immesh_cloud_index* x, int32_t* kept_index_out, int64_t cap, int64_t* n_out) {
    if (!x) return IMMESH_E_INVAL;
    immesh_ctx* c = x->ctx;
    RcKnn& q = x->kn;
    if (!x->built) { c->err = "cloud_index_apply_outliers: no index has been built (immesh_cloud_index_build)"; return IMMESH_E_INVAL; }
    if (!q.have_mask) { c->err = "cloud_index_apply_outliers: no outlier mask since the index's last build or apply"; return IMMESH_E_INVAL; }
    const int64_t n = x->n_pts, n_kept = q.n_kept;
    int rc;
    if ((rc = rc_cap(c, "cloud_index_apply_outliers", cap, n_kept, n_out, kept_index_out != nullptr, "kept points"))) return rc;
    (void)hipSetDevice(c->cfg.device);
    hipStream_t s = x->s;
    if ((rc = rc_grow(c, "cloud_index", q.off, (size_t)n * 4))) return rc;
    if ((rc = rc_grow(c, "cloud_index", q.out, (size_t)n_kept * 12))) return rc;
    if ((rc = rc_grow(c, "cloud_index", q.kept, (size_t)n_kept * 4))) return rc;
    if ((rc = rc_grow(c, "cloud_index", x->tree.temp, rd_scan_temp_bytes(1, 1, std::max<int64_t>(n, 1)) + 256))) return rc;
    // from here on the index changes: the scan of the mask, the compaction, the build over the compacted cloud
    x->built = false; x->q.have = false;
    q.changed();
    x->nr.changed();   // the normals belong to the cloud they were made on
    x->cl.changed();   // and so do the clusters
    HIPCHK(c, hipEventRecord(q.ev[4], s));
    if (n > 0) rd_scan_i32(s, x->tree.temp.p, x->tree.temp.bytes, (const int32_t*)q.flag.p, (int32_t*)q.off.p, n);
    kn_launch_compact(s, (const float*)x->pts.p, (const int32_t*)q.flag.p, (const int32_t*)q.off.p, n, n_kept, (float*)q.out.p, (int32_t*)q.kept.p);
    rc_swap(x->pts, q.out);   // the compacted cloud becomes the index's
    const RcLeaves src = {(const float*)x->pts.p, n_kept, nullptr};
    if ((rc = rc_tree_build(c, "cloud_index", s, x->ev[0], x->ev[1], x->h_small, x->tree, n_kept, src))) return rc;
    (void)hipEventElapsedTime(&x->ms[0], x->ev[0], x->ev[1]);
    HIPCHK(c, hipEventRecord(q.ev[5], s));
    HIPCHK(c, hipStreamSynchronize(s));
    (void)hipEventElapsedTime(&q.ms[2], q.ev[4], q.ev[5]);
    x->n_pts = n_kept;
    x->built = true;
    return rc_fetch(c, kept_index_out, q.kept.p, (size_t)n_kept * 4);
}

int immesh_cloud_index_points(immesh_cloud_index* x, float* xyz_out, int64_t cap, int64_t* n_out) {
    if (!x) return IMMESH_E_INVAL;
    immesh_ctx* c = x->ctx;
    if (!x->built) { c->err = "cloud_index_points: no index has been built (immesh_cloud_index_build)"; return IMMESH_E_INVAL; }
    int rc;
    if ((rc = rc_cap(c, "cloud_index_points", cap, x->n_pts, n_out, xyz_out != nullptr, "points"))) return rc;
    (void)hipSetDevice(c->cfg.device);
    return rc_fetch(c, xyz_out, x->pts.p, (size_t)x->n_pts * 12);
}

int immesh_knn_last_timing(immesh_cloud_index* x, float ms[3]) {
    if (!x || !ms) return IMMESH_E_INVAL;
    ms[0] = x->kn.ms[0]; ms[1] = x->kn.ms[1]; ms[2] = x->kn.ms[2];
    return 0;
}

}  // extern "C"
