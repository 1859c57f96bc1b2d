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

constexpr int32_t KN_MAX_K = 64;

int kn_check(immesh_cloud_index* x, const char* who, const char* what, double dist) {
    const int rc = cx_built(x, who);
    return rc ? rc : rc_positive(x->ctx, who, what, dist);
}

int kn_check_k(immesh_cloud_index* x, const char* who, int32_t k) {
    if (k < 1 || k > KN_MAX_K) { x->ctx->err = std::string(who) + ": need 1 <= k <= 64, got " + std::to_string(k); return IMMESH_E_INVAL; }
    return 0;
}

int kn_check_points(immesh_cloud_index* x, const char* who, const immesh_ray_frame* frame, const float* pts, int64_t n, RcFrame* fr) {
    const int rc = rc_points(x->ctx, who, pts, n);
    return rc || !frame ? rc : rc_frame(x->ctx, who, frame, fr);
}

// the query points of a point-mode call on the device
int kn_upload(immesh_cloud_index* x, const float* pts, int64_t n) {
    const int rc = rc_pass_grow(x->kn, x->kn.pts, (size_t)n * 12);
    if (rc) return rc;
    if (n > 0) HIPCHK(x->ctx, hipMemcpyAsync(x->kn.pts.p, pts, (size_t)n * 12, hipMemcpyHostToDevice, x->s));
    return 0;
}

// the Neighbours query behind its checks.  mode 0 / 1: n host points without / with a frame; mode 2: the cloud itself
int kn_knn(immesh_cloud_index* x, int mode, const RcFrame& fr, const float* pts, int64_t n, int32_t k, double max_dist, int32_t* count_out, int32_t* index_out,
           double* d2_out, double* mean_out) {
    immesh_ctx* c = x->ctx;
    RcKnn& q = x->kn;
    int rc;
    if ((rc = cx_ready(x, q, 4, 4))) return rc;
    if (mode == 2) q.have_knn = false;
    const bool lists = index_out || d2_out;
    const size_t m = (size_t)n, mk = m * (size_t)k;
    RcBuf& status = mode == 2 ? q.status : q.pstatus;
    if (mode != 2 && (rc = kn_upload(x, pts, n))) return rc;
    if ((rc = rc_pass_grow(q, q.count, m * 4))) return rc;
    if ((rc = rc_pass_grow(q, status, m))) return rc;
    if (mode == 2 && (rc = rc_pass_grow(q, q.mean, m * 8))) return rc;
    if (lists && ((rc = rc_pass_grow(q, q.idx, mk * 4)) || (rc = rc_pass_grow(q, q.d2, mk * 8)))) return rc;
    HIPCHK(c, hipEventRecord(q.ev[0], x->s));
    kn_launch_knn(x->s, fr, mode, mode == 2 ? (const float*)x->pts.p : (const float*)q.pts.p, n, k, max_dist * max_dist, (const float*)x->pts.p,
                  (const RcNode*)x->tree.nodes.p, x->tree.n_in, (int32_t*)q.count.p, lists ? (int32_t*)q.idx.p : nullptr, lists ? (double*)q.d2.p : nullptr,
                  (double*)q.mean.p, (uint8_t*)status.p);
    if ((rc = rc_pass_end(q, 0, 1, 0, 0, 0))) return rc;
    if ((rc = rc_fetch(c, count_out, q.count.p, m * 4))) return rc;
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
    if ((rc = cx_ready(x, q, 4, 4))) return rc;
    if (mode == 2) q.have_count = false;
    RcBuf& cnt = mode == 2 ? q.rcnt : q.count;
    RcBuf& status = mode == 2 ? q.rstatus : q.pstatus;
    if (mode != 2 && (rc = kn_upload(x, pts, n))) return rc;
    if ((rc = rc_pass_grow(q, cnt, (size_t)n * 4))) return rc;
    if ((rc = rc_pass_grow(q, status, (size_t)n))) return rc;
    HIPCHK(c, hipEventRecord(q.ev[0], x->s));
    kn_launch_count(x->s, fr, mode, mode == 2 ? (const float*)x->pts.p : (const float*)q.pts.p, n, radius * radius, (const float*)x->pts.p,
                    (const RcNode*)x->tree.nodes.p, x->tree.n_in, (int32_t*)cnt.p, (uint8_t*)status.p);
    if ((rc = rc_pass_end(q, 0, 1, 0, 0, 0))) return rc;
    if ((rc = rc_fetch(c, count_out, cnt.p, (size_t)n * 4))) return rc;
    if (mode == 2) q.have_count = true;
    return 0;
}

}  // namespace

int cx_mask_begin(immesh_cloud_index* x, CxMask* m) {
    RcKnn& q = x->kn;
    int rc;
    if ((rc = cx_ready(x, q, 4, 4))) return rc;
    q.have_mask = false;
    if ((rc = rc_pass_grow(q, q.flag, (size_t)x->n_pts * 4)) || (rc = rc_pass_grow(q, q.keep8, (size_t)x->n_pts))) return rc;
    *m = {(int32_t*)q.flag.p, (uint8_t*)q.keep8.p, (unsigned long long*)q.cnt.p};
    return rc_pass_begin(q, 2);
}

int cx_mask_end(immesh_cloud_index* x, int64_t counts[4], uint8_t* keep_out) {
    RcKnn& q = x->kn;
    const int rc = rc_pass_end(q, 2, 3, 1, 0, 4);
    if (rc) return rc;
    q.n_kept = (int64_t)q.h_cnt[0];
    q.have_mask = true;
    rc_pass_counts(q, counts);
    return rc_fetch(x->ctx, keep_out, q.keep8.p, (size_t)x->n_pts);
}

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
    int rc;
    if ((rc = cx_built(x, "cloud_outliers_statistical"))) return rc;
    if ((rc = rc_have(c, "cloud_outliers_statistical", q.have_knn, "no immesh_knn_cloud query since the index's last build or apply"))) return rc;
    if (!(mult >= 0.0) || !std::isfinite(mult)) { c->err = "cloud_outliers_statistical: need 0 <= mult, finite"; return IMMESH_E_INVAL; }
    (void)hipSetDevice(c->cfg.device);
    // the Outliers rule's mu and sigma: exact host code over the means, read back once (a mean is -1 exactly when count == 0, else >= 0)
    const int64_t n = x->n_pts;
    q.h_mean.resize((size_t)n);
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
    CxMask m;
    if ((rc = cx_mask_begin(x, &m))) return rc;
    kn_launch_mask_statistical(x->s, (const double*)q.mean.p, (const uint8_t*)q.status.p, n, threshold, m.flag, m.keep8, m.cnt);
    return cx_mask_end(x, counts, keep_out);
}

int immesh_cloud_outliers_radius(immesh_cloud_index* x, int64_t min_neighbours, int64_t counts[4], uint8_t* keep_out) {
    if (!x) return IMMESH_E_INVAL;
    immesh_ctx* c = x->ctx;
    RcKnn& q = x->kn;
    int rc;
    if ((rc = cx_built(x, "cloud_outliers_radius"))) return rc;
    if ((rc = rc_have(c, "cloud_outliers_radius", q.have_count, "no immesh_radius_count_cloud query since the index's last build or apply"))) return rc;
    if ((rc = rc_count_arg(c, "cloud_outliers_radius", "min_neighbours", min_neighbours))) return rc;
    CxMask m;
    if ((rc = cx_mask_begin(x, &m))) return rc;
    kn_launch_mask_radius(x->s, (const int32_t*)q.rcnt.p, (const uint8_t*)q.rstatus.p, x->n_pts, (int32_t)min_neighbours, m.flag, m.keep8, m.cnt);
    return cx_mask_end(x, counts, keep_out);
}

int immesh_cloud_index_apply_outliers(immesh_cloud_index* x, int32_t* kept_index_out, int64_t cap, int64_t* n_out) {
    if (!x) return IMMESH_E_INVAL;
    immesh_ctx* c = x->ctx;
    RcKnn& q = x->kn;
    int rc;
    if ((rc = cx_built(x, "cloud_index_apply_outliers"))) return rc;
    if ((rc = rc_have(c, "cloud_index_apply_outliers", q.have_mask, "no outlier mask since the index's last build or apply"))) return rc;
    const int64_t n = x->n_pts, n_kept = q.n_kept;
    if ((rc = rc_cap(c, "cloud_index_apply_outliers", cap, n_kept, n_out, kept_index_out != nullptr, "kept points"))) return rc;
    (void)hipSetDevice(c->cfg.device);
    hipStream_t s = x->s;
    if ((rc = rc_pass_grow(q, q.off, (size_t)n * 4))) return rc;
    if ((rc = rc_pass_grow(q, q.out, (size_t)n_kept * 12))) return rc;
    if ((rc = rc_pass_grow(q, q.kept, (size_t)n_kept * 4))) return rc;
    if ((rc = rc_pass_grow(q, x->tree.temp, rd_scan_temp_bytes(1, 1, std::max<int64_t>(n, 1)) + 256))) return rc;
    // from here on the index changes: the scan of the mask, the compaction, the build over the compacted cloud
    x->built = false;
    cx_cloud_changed(x);
    HIPCHK(c, hipEventRecord(q.ev[4], s));
    if (n > 0) rd_scan_i32(s, x->tree.temp.p, x->tree.temp.bytes, (const int32_t*)q.flag.p, (int32_t*)q.off.p, n);
    kn_launch_compact(s, (const float*)x->pts.p, (const int32_t*)q.flag.p, (const int32_t*)q.off.p, n, n_kept, (float*)q.out.p, (int32_t*)q.kept.p);
    rc_swap(x->pts, q.out);   // the compacted cloud becomes the index's
    const RcLeaves src = {(const float*)x->pts.p, n_kept, nullptr};
    if ((rc = rc_tree_build(c, "cloud_index", s, x->ev[0], x->ev[1], x->h_small, x->tree, n_kept, src))) return rc;
    (void)hipEventElapsedTime(&x->ms[0], x->ev[0], x->ev[1]);
    if ((rc = rc_pass_span(q, 4, 5, 2))) return rc;
    x->n_pts = n_kept;
    x->built = true;
    return rc_fetch(c, kept_index_out, q.kept.p, (size_t)n_kept * 4);
}

int immesh_cloud_index_points(immesh_cloud_index* x, float* xyz_out, int64_t cap, int64_t* n_out) {
    if (!x) return IMMESH_E_INVAL;
    immesh_ctx* c = x->ctx;
    int rc;
    if ((rc = cx_built(x, "cloud_index_points"))) return rc;
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
