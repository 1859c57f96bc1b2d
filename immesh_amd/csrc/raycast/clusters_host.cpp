// Host side of the Euclidean clusters of a cloud index (include/immesh_nearest.h, the Clusters rule): argument checks, grow-only buffers in the index's
// RcClusters record, the launches on the index's stream, the table's fetch and the Select rule's per-cluster decision.  Every check stands before the
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

constexpr int64_t CL_MAX_ARG = (int64_t)0x7FFFFFFE;

int cl_built(immesh_cloud_index* x, const char* who) {
    if (!x->built) { x->ctx->err = std::string(who) + ": no index has been built (immesh_cloud_index_build)"; return IMMESH_E_INVAL; }
    return 0;
}

int cl_have(immesh_cloud_index* x, const char* who) {
    int rc;
    if ((rc = cl_built(x, who))) return rc;
    if (!x->cl.have) { x->ctx->err = std::string(who) + ": no immesh_cloud_clusters call since the index's last build or apply"; return IMMESH_E_INVAL; }
    return 0;
}

int cl_check_count(immesh_cloud_index* x, const char* who, const char* what, int64_t v) {
    if (v < 0 || v > CL_MAX_ARG) { x->ctx->err = std::string(who) + ": need " + what + " in [0, 2^31 - 2]"; return IMMESH_E_INVAL; }
    return 0;
}

int cl_grow(immesh_cloud_index* x, RcBuf& b, size_t bytes) { return rc_grow(x->ctx, "cloud_index", b, bytes); }

// the events, the pinned words and the device counters, at the first call
int cl_ready(immesh_cloud_index* x) {
    immesh_ctx* c = x->ctx;
    (void)hipSetDevice(c->cfg.device);
    for (hipEvent_t& e : x->cl.ev)
        if (!e) HIPCHK(c, hipEventCreate(&e));
    if (!x->cl.h_cnt) HIPCHK(c, hipHostMalloc((void**)&x->cl.h_cnt, CL_PINNED * 8));
    return cl_grow(x, x->cl.dcnt, CL_COUNTERS * 8);
}

float cl_span(hipEvent_t a, hipEvent_t b) {
    float ms = 0.0f;
    (void)hipEventElapsedTime(&ms, a, b);
    return ms;
}

}  // namespace

extern "C" {

int immesh_cloud_clusters(immesh_cloud_index* x, double radius, int64_t min_neighbours, int32_t* label_out, uint8_t* kind_out, int64_t counts[4],
                          int64_t* n_clusters_out) {
    if (!x) return IMMESH_E_INVAL;
    immesh_ctx* c = x->ctx;
    RcClusters& q = x->cl;
    int rc;
    if ((rc = cl_built(x, "cloud_clusters"))) return rc;
    if (!(radius > 0.0) || !std::isfinite(radius)) { c->err = "cloud_clusters: need 0 < radius, finite"; return IMMESH_E_INVAL; }
    if ((rc = cl_check_count(x, "cloud_clusters", "min_neighbours", min_neighbours))) return rc;
    if ((rc = cl_ready(x))) return rc;
    hipStream_t s = x->s;
    q.have = false;
    const int64_t n = x->n_pts, n_in = x->tree.n_in;
    const size_t m = (size_t)n;
    const bool counted = min_neighbours > 0;
    if (counted && ((rc = cl_grow(x, q.cnt, m * 4)) || (rc = cl_grow(x, q.status, m)))) return rc;
    if ((rc = cl_grow(x, q.core, m)) || (rc = cl_grow(x, q.kind, m))) return rc;
    if ((rc = cl_grow(x, q.parent, m * 4)) || (rc = cl_grow(x, q.root, m * 4)) || (rc = cl_grow(x, q.flag, m * 4))) return rc;
    if ((rc = cl_grow(x, q.num, m * 4)) || (rc = cl_grow(x, q.label, m * 4))) return rc;
    if ((rc = cl_grow(x, x->tree.temp, rd_scan_temp_bytes(1, 1, std::max<int64_t>(n, 1)) + 256))) return rc;
    const float* cloud = (const float*)x->pts.p;
    const RcNode* nodes = (const RcNode*)x->tree.nodes.p;
    const double r2 = radius * radius;
    uint8_t *core = (uint8_t*)q.core.p, *kind = (uint8_t*)q.kind.p;
    int32_t *parent = (int32_t*)q.parent.p, *root = (int32_t*)q.root.p, *flag = (int32_t*)q.flag.p, *num = (int32_t*)q.num.p;
    unsigned long long* cnt = (unsigned long long*)q.dcnt.p;
    unsigned long long* h = q.h_cnt;
    HIPCHK(c, hipMemsetAsync(cnt, 0, CL_COUNTERS * 8, s));
    // the count (its buffers are the clusters' own: the index's last Count query stays) and the kinds
    HIPCHK(c, hipEventRecord(q.ev[0], s));
    if (counted) kn_launch_count(s, RcFrame{}, 2, cloud, n, r2, cloud, nodes, n_in, (int32_t*)q.cnt.p, (uint8_t*)q.status.p);
    cl_launch_kind(s, cloud, n, counted ? (const int32_t*)q.cnt.p : nullptr, (int32_t)min_neighbours, core, kind, parent, root);
    HIPCHK(c, hipEventRecord(q.ev[1], s));
    // the joins
    HIPCHK(c, hipEventRecord(q.ev[2], s));
    cl_launch_join(s, cloud, n, r2, nodes, n_in, core, parent, cnt);
    HIPCHK(c, hipEventRecord(q.ev[3], s));
    // the roots; the border walk reads them
    HIPCHK(c, hipEventRecord(q.ev[6], s));
    cl_launch_flatten(s, n, core, parent, root, flag);
    HIPCHK(c, hipEventRecord(q.ev[4], s));
    if (counted) cl_launch_border(s, cloud, n, r2, nodes, n_in, core, kind, root);
    HIPCHK(c, hipEventRecord(q.ev[5], s));
    // the numbering: the one count the host needs sizes the table
    for (int i = 0; i < CL_PINNED; i++) h[i] = 0;
    if (n > 0) {
        rd_scan_i32(s, x->tree.temp.p, x->tree.temp.bytes, flag, num, n);
        HIPCHK(c, hipMemcpyAsync(&h[5], num + (n - 1), 4, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipMemcpyAsync(&h[6], flag + (n - 1), 4, hipMemcpyDeviceToHost, s));
    }
    HIPCHK(c, hipEventRecord(q.ev[7], s));
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(s));
    const int64_t n_clusters = (int64_t)h[5] + (int64_t)h[6];
    const size_t nc = (size_t)n_clusters;
    if ((rc = cl_grow(x, q.first, nc * 4)) || (rc = cl_grow(x, q.npts, nc * 4)) || (rc = cl_grow(x, q.ncore, nc * 4))) return rc;
    if ((rc = cl_grow(x, q.boxkey, nc * 24)) || (rc = cl_grow(x, q.box, nc * 24))) return rc;
    // the table
    HIPCHK(c, hipEventRecord(q.ev[8], s));
    cl_launch_preset(s, n_clusters, (int32_t*)q.first.p, (int32_t*)q.npts.p, (int32_t*)q.ncore.p, (uint32_t*)q.boxkey.p);
    cl_launch_table(s, cloud, n, kind, root, num, n_clusters, (int32_t*)q.label.p, (int32_t*)q.first.p, (int32_t*)q.npts.p, (int32_t*)q.ncore.p,
                    (uint32_t*)q.boxkey.p, cnt);
    cl_launch_unkey(s, n_clusters, (const uint32_t*)q.boxkey.p, (float*)q.box.p);
    HIPCHK(c, hipEventRecord(q.ev[9], s));
    HIPCHK(c, hipMemcpyAsync(h, cnt, CL_COUNTERS * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(s));
    q.ms[0] = cl_span(q.ev[0], q.ev[1]);
    q.ms[1] = cl_span(q.ev[2], q.ev[3]);
    q.ms[2] = counted ? cl_span(q.ev[4], q.ev[5]) : 0.0f;
    q.ms[3] = (cl_span(q.ev[6], q.ev[4]) + cl_span(q.ev[5], q.ev[7])) + cl_span(q.ev[8], q.ev[9]);   // the flatten, the scan, the table
    if (h[CL_ERROR]) {
        c->err = "cloud_clusters: a union did not finish within its step bound (a defect of the library)";
        return IMMESH_E_INTERNAL;
    }
    q.n_clusters = n_clusters;
    q.have = true;
    if (counts)
        for (int i = 0; i < 4; i++) counts[i] = (int64_t)h[i];
    if (n_clusters_out) *n_clusters_out = n_clusters;
    if ((rc = rc_fetch(c, label_out, q.label.p, m * 4))) return rc;
    return rc_fetch(c, kind_out, q.kind.p, m);
}

int immesh_cloud_clusters_table(immesh_cloud_index* x, int32_t* first_out, int32_t* n_points_out, int32_t* n_core_out, float* box_out, int64_t cap,
                                int64_t* n_out) {
    if (!x) return IMMESH_E_INVAL;
    immesh_ctx* c = x->ctx;
    int rc;
    if ((rc = cl_have(x, "cloud_clusters_table"))) return rc;
    const RcClusters& q = x->cl;
    const int64_t n = q.n_clusters;
    const bool wanted = first_out || n_points_out || n_core_out || box_out;
    if ((rc = rc_cap(c, "cloud_clusters_table", cap, n, n_out, wanted, "clusters"))) return rc;
    if (!wanted || n == 0) return 0;
    (void)hipSetDevice(c->cfg.device);
    if ((rc = rc_fetch(c, first_out, q.first.p, (size_t)n * 4))) return rc;
    if ((rc = rc_fetch(c, n_points_out, q.npts.p, (size_t)n * 4))) return rc;
    if ((rc = rc_fetch(c, n_core_out, q.ncore.p, (size_t)n * 4))) return rc;
    return rc_fetch(c, box_out, q.box.p, (size_t)n * 24);
}

int immesh_cloud_clusters_select(immesh_cloud_index* x, int64_t min_points, int64_t max_points, int64_t keep_largest, int32_t keep_noise, int64_t counts[4],
                                 uint8_t* keep_out) {
    if (!x) return IMMESH_E_INVAL;
    immesh_ctx* c = x->ctx;
    RcClusters& q = x->cl;
    RcKnn& k = x->kn;
    int rc;
    if ((rc = cl_have(x, "cloud_clusters_select"))) return rc;
    if ((rc = cl_check_count(x, "cloud_clusters_select", "min_points", min_points))) return rc;
    if ((rc = cl_check_count(x, "cloud_clusters_select", "max_points", max_points))) return rc;
    if ((rc = cl_check_count(x, "cloud_clusters_select", "keep_largest", keep_largest))) return rc;
    (void)hipSetDevice(c->cfg.device);
    hipStream_t s = x->s;
    const int64_t n = x->n_pts, nc = q.n_clusters;
    // the mask is the index's last mask: its events, buffers and pinned counts are those of the Outliers rules (knn_host.cpp)
    for (hipEvent_t& e : k.ev)
        if (!e) HIPCHK(c, hipEventCreate(&e));
    if (!k.h_cnt) HIPCHK(c, hipHostMalloc((void**)&k.h_cnt, 4 * 8));
    // the Select rule per cluster: host code over n_points, read back once
    q.h_npts.resize((size_t)nc);
    q.h_keepc.resize((size_t)nc);
    if ((rc = rc_fetch(c, q.h_npts.data(), q.npts.p, (size_t)nc * 4))) return rc;
    for (int64_t i = 0; i < nc; i++) {
        const int64_t p = q.h_npts[(size_t)i];
        q.h_keepc[(size_t)i] = p >= min_points && (max_points == 0 || p <= max_points) ? 1 : 0;
    }
    if (keep_largest > 0 && keep_largest < nc) {   // the ranking over ALL clusters: most points first, ties to the smaller number
        q.h_rank.resize((size_t)nc);
        for (int64_t i = 0; i < nc; i++) q.h_rank[(size_t)i] = (int32_t)i;
        const int32_t* np = q.h_npts.data();
        std::sort(q.h_rank.begin(), q.h_rank.end(), [np](int32_t a, int32_t b) { return np[a] != np[b] ? np[a] > np[b] : a < b; });
        for (int64_t r = keep_largest; r < nc; r++) q.h_keepc[(size_t)q.h_rank[(size_t)r]] = 0;
    }
    k.have_mask = false;
    if ((rc = cl_grow(x, q.keepc, (size_t)nc * 4))) return rc;
    if ((rc = cl_grow(x, k.flag, (size_t)n * 4))) return rc;
    if ((rc = cl_grow(x, k.keep8, (size_t)n))) return rc;
    if ((rc = cl_grow(x, k.mcnt, 4 * 8))) return rc;
    unsigned long long* cnt = (unsigned long long*)k.mcnt.p;
    if (nc > 0) HIPCHK(c, hipMemcpyAsync(q.keepc.p, q.h_keepc.data(), (size_t)nc * 4, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipEventRecord(k.ev[2], s));
    HIPCHK(c, hipMemsetAsync(cnt, 0, 4 * 8, s));
    cl_launch_mask(s, n, (const uint8_t*)q.kind.p, (const int32_t*)q.label.p, (const int32_t*)q.keepc.p, nc, keep_noise, (int32_t*)k.flag.p, (uint8_t*)k.keep8.p, cnt);
    HIPCHK(c, hipEventRecord(k.ev[3], s));
    HIPCHK(c, hipMemcpyAsync(k.h_cnt, cnt, 4 * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(s));
    (void)hipEventElapsedTime(&k.ms[1], k.ev[2], k.ev[3]);
    k.n_kept = (int64_t)k.h_cnt[0];
    k.have_mask = true;
    if (counts)
        for (int i = 0; i < 4; i++) counts[i] = (int64_t)k.h_cnt[i];
    return rc_fetch(c, keep_out, k.keep8.p, (size_t)n);
}

int immesh_cloud_clusters_last_timing(immesh_cloud_index* x, float ms[4]) {
    if (!x || !ms) return IMMESH_E_INVAL;
    for (int i = 0; i < 4; i++) ms[i] = x->cl.ms[i];
    return 0;
}

}  // extern "C"
