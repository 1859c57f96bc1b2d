// Host side of the cloud normals and of their agreement with a caster's face normals (include/immesh_normals.h, the Normals and Agreement rules):
// argument checks, grow-only buffers and the launches on the index's stream.  Every check stands before the first launch and before anything of the
// index is touched, so a refused call leaves the index as it was.  Nothing here is allocated or launched unless one of these entry points is called.
#include <cmath>
#include <string>
#include "../host_ctx.hpp"
#include "../../../include/immesh_closest.h"
#include "../../../include/immesh_normals.h"
#include "raycast.hpp"

namespace {

// the events, the pinned counts and the reduction's pinned result, at the first call
int nr_ready(immesh_cloud_index* x) {
    immesh_ctx* c = x->ctx;
    RcNormals& q = x->nr;
    (void)hipSetDevice(c->cfg.device);
    for (hipEvent_t& e : q.ev)
        if (!e) HIPCHK(c, hipEventCreate(&e));
    if (!q.h_cnt) HIPCHK(c, hipHostMalloc((void**)&q.h_cnt, 4 * 8));
    if (!q.a.h_res) HIPCHK(c, hipHostMalloc((void**)&q.a.h_res, sizeof(DqStatsDev)));
    return rc_grow(c, "cloud_index", q.dcnt, 4 * 8);
}

// behind a launch that counts: the end event, the four counts, the wait, the span
int nr_finish(immesh_cloud_index* x, int e0, int span, int64_t counts[4]) {
    immesh_ctx* c = x->ctx;
    RcNormals& q = x->nr;
    HIPCHK(c, hipEventRecord(q.ev[e0 + 1], x->s));
    HIPCHK(c, hipMemcpyAsync(q.h_cnt, q.dcnt.p, 4 * 8, hipMemcpyDeviceToHost, x->s));
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(x->s));
    (void)hipEventElapsedTime(&q.ms[span], q.ev[e0], q.ev[e0 + 1]);
    if (counts)
        for (int i = 0; i < 4; i++) counts[i] = (int64_t)q.h_cnt[i];
    return 0;
}

// what both agreement calls ask of the index and the caster
int nr_check_agree(immesh_cloud_index* x, immesh_raycaster* r, const char* who) {
    immesh_ctx* c = x->ctx;
    const std::string w(who);
    if (!x->built) { c->err = w + ": no index has been built (immesh_cloud_index_build)"; return IMMESH_E_INVAL; }
    if (!x->nr.have) { c->err = w + ": no normals since the index's last build or apply (immesh_cloud_normals)"; return IMMESH_E_INVAL; }
    if (!r) { c->err = w + ": no caster"; return IMMESH_E_INVAL; }
    if (r->ctx != c) { c->err = w + ": the caster and the index belong to different contexts"; return IMMESH_E_INVAL; }
    if (!r->built) { c->err = w + ": no hierarchy has been built on the caster"; return IMMESH_E_INVAL; }
    return 0;
}

// the agreement's buffers for n items
int nr_grow_agree(immesh_cloud_index* x, size_t n) {
    immesh_ctx* c = x->ctx;
    RcNormals& q = x->nr;
    int rc;
    if ((rc = rc_grow(c, "cloud_index", q.agree, n * 4))) return rc;
    if ((rc = rc_grow(c, "cloud_index", q.a.dist, n * 4))) return rc;
    return rc_grow(c, "cloud_index", q.a.status, n);
}

}  // namespace

extern "C" {

int immesh_cloud_normals(immesh_cloud_index* x, int32_t k, double max_dist, double min_ratio, int32_t mode, const double* viewpoint, float* normal_out,
                         double* curvature_out, double* eig_out, int32_t* count_out, uint8_t* status_out, int64_t counts[4]) {
    if (!x) return IMMESH_E_INVAL;
    immesh_ctx* c = x->ctx;
    RcNormals& q = x->nr;
    if (!x->built) { c->err = "cloud_normals: no index has been built (immesh_cloud_index_build)"; return IMMESH_E_INVAL; }
    if (k < 2 || k > 64) { c->err = "cloud_normals: need 2 <= k <= 64, got " + std::to_string(k); return IMMESH_E_INVAL; }
    if (!(max_dist > 0.0) || !std::isfinite(max_dist)) { c->err = "cloud_normals: need 0 < max_dist, finite"; return IMMESH_E_INVAL; }
    if (!(min_ratio >= 0.0) || !(min_ratio < 1.0)) { c->err = "cloud_normals: need 0 <= min_ratio < 1"; return IMMESH_E_INVAL; }
    if (mode != IMMESH_NORMALS_CANONICAL && mode != IMMESH_NORMALS_VIEWPOINT) {
        c->err = "cloud_normals: unknown mode " + std::to_string(mode);
        return IMMESH_E_INVAL;
    }
    if (mode == IMMESH_NORMALS_VIEWPOINT &&
        (!viewpoint || !std::isfinite(viewpoint[0]) || !std::isfinite(viewpoint[1]) || !std::isfinite(viewpoint[2]))) {
        c->err = "cloud_normals: the viewpoint is not finite";
        return IMMESH_E_INVAL;
    }
    int rc;
    if ((rc = nr_ready(x))) return rc;
    q.changed();   // the normals of an earlier call go, and the agreement that read them
    const int64_t n = x->n_pts;
    const size_t m = (size_t)n;
    if ((rc = rc_grow(c, "cloud_index", q.normal, m * 12))) return rc;
    if ((rc = rc_grow(c, "cloud_index", q.status, m))) return rc;
    if ((rc = rc_grow(c, "cloud_index", q.curv, m * 8))) return rc;
    if ((rc = rc_grow(c, "cloud_index", q.eig, m * 24))) return rc;
    if ((rc = rc_grow(c, "cloud_index", q.cnt, m * 4))) return rc;
    HIPCHK(c, hipEventRecord(q.ev[0], x->s));
    HIPCHK(c, hipMemsetAsync(q.dcnt.p, 0, 4 * 8, x->s));
    nr_launch_normals(x->s, n, k, max_dist * max_dist, min_ratio, mode == IMMESH_NORMALS_VIEWPOINT ? viewpoint : nullptr, (const float*)x->pts.p,
                      (const RcNode*)x->tree.nodes.p, x->tree.n_in, (float*)q.normal.p, (double*)q.curv.p, (double*)q.eig.p, (int32_t*)q.cnt.p,
                      (uint8_t*)q.status.p, (unsigned long long*)q.dcnt.p);
    if ((rc = nr_finish(x, 0, 0, counts))) return rc;
    q.n = n;
    q.have = true;
    if ((rc = rc_fetch(c, normal_out, q.normal.p, m * 12))) return rc;
    if ((rc = rc_fetch(c, curvature_out, q.curv.p, m * 8))) return rc;
    if ((rc = rc_fetch(c, eig_out, q.eig.p, m * 24))) return rc;
    if ((rc = rc_fetch(c, count_out, q.cnt.p, m * 4))) return rc;
    return rc_fetch(c, status_out, q.status.p, m);
}

int immesh_cloud_normals_get(immesh_cloud_index* x, float* normal_out, uint8_t* status_out, int64_t cap, int64_t* n_out) {
    if (!x) return IMMESH_E_INVAL;
    immesh_ctx* c = x->ctx;
    if (!x->built) { c->err = "cloud_normals_get: no index has been built (immesh_cloud_index_build)"; return IMMESH_E_INVAL; }
    if (!x->nr.have) { c->err = "cloud_normals_get: no normals since the index's last build or apply (immesh_cloud_normals)"; return IMMESH_E_INVAL; }
    int rc;
    if ((rc = rc_cap(c, "cloud_normals_get", cap, x->nr.n, n_out, normal_out != nullptr || status_out != nullptr, "points"))) return rc;
    (void)hipSetDevice(c->cfg.device);
    if ((rc = rc_fetch(c, normal_out, x->nr.normal.p, (size_t)x->nr.n * 12))) return rc;
    return rc_fetch(c, status_out, x->nr.status.p, (size_t)x->nr.n);
}

int immesh_normals_agree_samples(immesh_cloud_index* x, immesh_raycaster* r, float* agree_out, int64_t counts[4]) {
    if (!x) return IMMESH_E_INVAL;
    immesh_ctx* c = x->ctx;
    RcNormals& q = x->nr;
    int rc;
    if ((rc = nr_check_agree(x, r, "normals_agree_samples"))) return rc;
    if (!r->sm.have) { c->err = "normals_agree_samples: no samples since the caster's last build (immesh_mesh_sample)"; return IMMESH_E_INVAL; }
    if (!x->q.have || x->q_rc != r || x->q_gen != r->sm.gen || x->q.n != r->sm.n) {
        c->err = "normals_agree_samples: no immesh_nearest_samples query of this caster since its last sampling";
        return IMMESH_E_INVAL;
    }
    if ((rc = nr_ready(x))) return rc;
    q.a.have = false;
    const int64_t n = r->sm.n;
    if ((rc = nr_grow_agree(x, (size_t)n))) return rc;
    HIPCHK(c, hipStreamWaitEvent(x->s, r->sm.done, 0));   // the samples are complete before the launch reads their faces
    HIPCHK(c, hipEventRecord(q.ev[2], x->s));
    HIPCHK(c, hipMemsetAsync(q.dcnt.p, 0, 4 * 8, x->s));
    nr_launch_agree_samples(x->s, (const int32_t*)r->sm.face.p, (const int32_t*)x->q.id.p, n, (const float*)q.normal.p, (const uint8_t*)q.status.p, q.n,
                            (const float*)r->vtx.p, r->n_vtx, (const int32_t*)r->faces.p, r->n_faces, (float*)q.agree.p, (float*)q.a.dist.p,
                            (uint8_t*)q.a.status.p, (unsigned long long*)q.dcnt.p);
    if ((rc = nr_finish(x, 2, 1, counts))) return rc;
    q.a.n = n;
    q.a.have = true;
    return rc_fetch(c, agree_out, q.agree.p, (size_t)n * 4);
}

int immesh_normals_agree_cloud(immesh_cloud_index* x, immesh_raycaster* r, double max_dist, float* agree_out, int32_t* face_out, int64_t counts[4]) {
    if (!x) return IMMESH_E_INVAL;
    immesh_ctx* c = x->ctx;
    RcNormals& q = x->nr;
    int rc;
    if ((rc = nr_check_agree(x, r, "normals_agree_cloud"))) return rc;
    if (!(max_dist > 0.0) || !std::isfinite(max_dist)) { c->err = "normals_agree_cloud: need 0 < max_dist, finite"; return IMMESH_E_INVAL; }
    if ((rc = nr_ready(x))) return rc;
    q.a.have = false;
    const int64_t n = q.n;
    if ((rc = nr_grow_agree(x, (size_t)n))) return rc;
    if ((rc = rc_grow(c, "cloud_index", q.face, (size_t)n * 4))) return rc;
    HIPCHK(c, hipEventRecord(q.ev[2], x->s));
    HIPCHK(c, hipMemsetAsync(q.dcnt.p, 0, 4 * 8, x->s));
    nr_launch_agree_cloud(x->s, (const float*)x->pts.p, (const float*)q.normal.p, (const uint8_t*)q.status.p, n, max_dist * max_dist, (const float*)r->vtx.p,
                          r->n_vtx, (const int32_t*)r->faces.p, r->n_faces, (const RcNode*)r->tree.nodes.p, r->tree.n_in, (float*)q.agree.p,
                          (float*)q.a.dist.p, (int32_t*)q.face.p, (uint8_t*)q.a.status.p, (unsigned long long*)q.dcnt.p);
    if ((rc = nr_finish(x, 2, 1, counts))) return rc;
    q.a.n = n;
    q.a.have = true;
    if ((rc = rc_fetch(c, agree_out, q.agree.p, (size_t)n * 4))) return rc;
    return rc_fetch(c, face_out, q.face.p, (size_t)n * 4);
}

int immesh_normals_agree_reduce(immesh_cloud_index* x, double bin_width, int32_t n_bins, immesh_closest_stats* stats, int64_t* hist_out) {
    if (!x) return IMMESH_E_INVAL;
    immesh_ctx* c = x->ctx;
    RcNormals& q = x->nr;
    if (!x->built) { c->err = "normals_agree_reduce: no index has been built (immesh_cloud_index_build)"; return IMMESH_E_INVAL; }
    if (!q.have || !q.a.have) {   // (before the events exist: rc_dist_reduce records them)
        c->err = "normals_agree_reduce: no agreement since the index's last normals (immesh_normals_agree_samples, immesh_normals_agree_cloud)";
        return IMMESH_E_INVAL;
    }
    return rc_dist_reduce(c, "normals_agree_reduce", "cloud_index", "no agreement has been made on this index", x->s, q.ev[4], q.ev[5], &q.ms[2], q.a,
                          bin_width, n_bins, stats, hist_out);
}

int immesh_normals_last_timing(immesh_cloud_index* x, float ms[3]) {
    if (!x || !ms) return IMMESH_E_INVAL;
    ms[0] = x->nr.ms[0]; ms[1] = x->nr.ms[1]; ms[2] = x->nr.ms[2];
    return 0;
}

}  // extern "C"
