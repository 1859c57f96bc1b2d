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

int cl_have(immesh_cloud_index* x, const char* who) {
    const int rc = cx_built(x, who);
    return rc ? rc : rc_have(x->ctx, who, x->cl.have, "no immesh_cloud_clusters call since the index's last build or apply");
}

}  // namespace

extern "C" {

int immesh_cloud_clusters(immesh_cloud_index* x, double radius, int64_t min_neighbours, int32_t* label_out, uint8_t* kind_out, int64_t counts[4],
                          int64_t* n_clusters_out) {
    if (!x) return IMMESH_E_INVAL;
    immesh_ctx* c = x->ctx;
    RcClusters& q = x->cl;
    int rc;
    if ((rc = cx_built(x, "cloud_clusters"))) return rc;
    if ((rc = rc_positive(c, "cloud_clusters", "radius", radius))) return rc;
    if ((rc = rc_count_arg(c, "cloud_clusters", "min_neighbours", min_neighbours))) return rc;
    if ((rc = cx_ready(x, q, CL_COUNTERS, CL_PINNED))) return rc;
    hipStream_t s = x->s;
    q.have = false;
    const int64_t n = x->n_pts, n_in = x->tree.n_in;
    const size_t m = (size_t)n;
    const bool counted = min_neighbours > 0;
    if (counted && ((rc = rc_pass_grow(q, q.count, m * 4)) || (rc = rc_pass_grow(q, q.status, m)))) return rc;
    if ((rc = rc_pass_grow(q, q.core, m)) || (rc = rc_pass_grow(q, q.kind, m))) return rc;
    if ((rc = rc_pass_grow(q, q.parent, m * 4)) || (rc = rc_pass_grow(q, q.root, m * 4)) || (rc = rc_pass_grow(q, q.flag, m * 4))) return rc;
    if ((rc = rc_pass_grow(q, q.num, m * 4)) || (rc = rc_pass_grow(q, q.label, m * 4))) return rc;
    if ((rc = rc_pass_grow(q, x->tree.temp, rd_scan_temp_bytes(1, 1, std::max<int64_t>(n, 1)) + 256))) return rc;
    const float* cloud = (const float*)x->pts.p;
    const RcNode* nodes = (const RcNode*)x->tree.nodes.p;
    const double r2 = radius * radius;
    uint8_t *core = (uint8_t*)q.core.p, *kind = (uint8_t*)q.kind.p;
    int32_t *parent = (int32_t*)q.parent.p, *root = (int32_t*)q.root.p, *flag = (int32_t*)q.flag.p, *num = (int32_t*)q.num.p;
    unsigned long long* cnt = (unsigned long long*)q.cnt.p;
    unsigned long long* h = q.h_cnt;
    HIPCHK(c, hipMemsetAsync(cnt, 0, CL_COUNTERS * 8, s));
    // the count (its buffers are the clusters' own: the index's last Count query stays) and the kinds
    HIPCHK(c, hipEventRecord(q.ev[0], s));
    if (counted) kn_launch_count(s, RcFrame{}, 2, cloud, n, r2, cloud, nodes, n_in, (int32_t*)q.count.p, (uint8_t*)q.status.p);
    cl_launch_kind(s, cloud, n, counted ? (const int32_t*)q.count.p : nullptr, (int32_t)min_neighbours, core, kind, parent, root);
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
    if ((rc = rc_pass_end(q, 5, 7, 3, 0, 0))) return rc;
    const float scan_ms = q.ms[3];
    const int64_t n_clusters = (int64_t)h[5] + (int64_t)h[6];
    const size_t nc = (size_t)n_clusters;
    if ((rc = rc_pass_grow(q, q.first, nc * 4)) || (rc = rc_pass_grow(q, q.npts, nc * 4)) || (rc = rc_pass_grow(q, q.ncore, nc * 4))) return rc;
    if ((rc = rc_pass_grow(q, q.boxkey, nc * 24)) || (rc = rc_pass_grow(q, q.box, nc * 24))) return rc;
    // the table
    HIPCHK(c, hipEventRecord(q.ev[8], s));
    cl_launch_preset(s, n_clusters, (int32_t*)q.first.p, (int32_t*)q.npts.p, (int32_t*)q.ncore.p, (uint32_t*)q.boxkey.p);
    cl_launch_table(s, cloud, n, kind, root, num, n_clusters, (int32_t*)q.label.p, (int32_t*)q.first.p, (int32_t*)q.npts.p, (int32_t*)q.ncore.p,
                    (uint32_t*)q.boxkey.p, cnt);
    cl_launch_unkey(s, n_clusters, (const uint32_t*)q.boxkey.p, (float*)q.box.p);
    if ((rc = rc_pass_end(q, 8, 9, 3, 0, CL_COUNTERS))) return rc;
    q.ms[0] = rc_pass_ms(q, 0, 1);
    q.ms[1] = rc_pass_ms(q, 2, 3);
    q.ms[2] = counted ? rc_pass_ms(q, 4, 5) : 0.0f;
    q.ms[3] = (rc_pass_ms(q, 6, 4) + scan_ms) + q.ms[3];   // the flatten, the scan, the table
    if (h[CL_ERROR]) {
        c->err = "cloud_clusters: a union did not finish within its step bound (a defect of the library)";
        return IMMESH_E_INTERNAL;
    }
    q.n_clusters = n_clusters;
    q.have = true;
    rc_pass_counts(q, counts);
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
    int rc;
    if ((rc = cl_have(x, "cloud_clusters_select"))) return rc;
    if ((rc = rc_count_arg(c, "cloud_clusters_select", "min_points", min_points))) return rc;
    if ((rc = rc_count_arg(c, "cloud_clusters_select", "max_points", max_points))) return rc;
    if ((rc = rc_count_arg(c, "cloud_clusters_select", "keep_largest", keep_largest))) return rc;
    (void)hipSetDevice(c->cfg.device);
    hipStream_t s = x->s;
    const int64_t n = x->n_pts, nc = q.n_clusters;
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
    if ((rc = rc_pass_grow(q, q.keepc, (size_t)nc * 4))) return rc;
    if (nc > 0) HIPCHK(c, hipMemcpyAsync(q.keepc.p, q.h_keepc.data(), (size_t)nc * 4, hipMemcpyHostToDevice, s));
    // the mask is the index's last mask, as the Outliers rules' is (knn_host.cpp)
    CxMask m;
    if ((rc = cx_mask_begin(x, &m))) return rc;
    cl_launch_mask(s, n, (const uint8_t*)q.kind.p, (const int32_t*)q.label.p, (const int32_t*)q.keepc.p, nc, keep_noise, m.flag, m.keep8, m.cnt);
    return cx_mask_end(x, counts, keep_out);
}

int immesh_cloud_clusters_last_timing(immesh_cloud_index* x, float ms[4]) {
    if (!x || !ms) return IMMESH_E_INVAL;
    for (int i = 0; i < 4; i++) ms[i] = x->cl.ms[i];
    return 0;
}

}  // extern "C"
