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

constexpr const char* NR_NONE = "no normals since the index's last build or apply (immesh_cloud_normals)";

// what both agreement calls ask of the index and the caster
int nr_check_agree(immesh_cloud_index* x, immesh_raycaster* r, const char* who, bool sampled) {
    int rc;
    if ((rc = cx_built(x, who)) || (rc = rc_have(x->ctx, who, x->nr.have, NR_NONE)) || (rc = cx_caster(x, r, who))) return rc;
    return cx_caster_built(x, r, who, sampled);
}

// the record ready, the old agreement gone, its buffers for n items and the reduction's pinned result
int nr_agree_begin(immesh_cloud_index* x, size_t n) {
    RcNormals& q = x->nr;
    int rc;
    if ((rc = cx_ready(x, q, 4, 4))) return rc;
    if (!q.a.h_res) HIPCHK(x->ctx, hipHostMalloc((void**)&q.a.h_res, sizeof(DqStatsDev)));
    q.a.have = false;
    if ((rc = rc_pass_grow(q, q.agree, n * 4))) return rc;
    if ((rc = rc_pass_grow(q, q.a.dist, n * 4))) return rc;
    return rc_pass_grow(q, q.a.status, n);
}

// behind an agreement launch: the span's end, the four counts, the agreement valid
int nr_agree_end(immesh_cloud_index* x, int64_t n, int64_t counts[4]) {
    RcNormals& q = x->nr;
    const int rc = rc_pass_end(q, 2, 3, 1, 0, 4);
    if (rc) return rc;
    rc_pass_counts(q, counts);
    q.a.n = n;
    q.a.have = true;
    return 0;
}

}  // namespace

extern "C" {

int immesh_cloud_normals(immesh_cloud_index* x, int32_t k, double max_dist, double min_ratio, int32_t mode, const double* viewpoint, float* normal_out,
                         double* curvature_out, double* eig_out, int32_t* count_out, uint8_t* status_out, int64_t counts[4]) {
    if (!x) return IMMESH_E_INVAL;
    immesh_ctx* c = x->ctx;
    RcNormals& q = x->nr;
    int rc;
    if ((rc = cx_built(x, "cloud_normals"))) return rc;
    if (k < 2 || k > 64) { c->err = "cloud_normals: need 2 <= k <= 64, got " + std::to_string(k); return IMMESH_E_INVAL; }
    if ((rc = rc_positive(c, "cloud_normals", "max_dist", max_dist))) return rc;
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
    if ((rc = cx_ready(x, q, 4, 4))) return rc;
    q.have = false;   // the normals of an earlier call go,
    cx_normals_changed(x);   // and the agreement that read them
    const int64_t n = x->n_pts;
    const size_t m = (size_t)n;
    if ((rc = rc_pass_grow(q, q.normal, m * 12))) return rc;
    if ((rc = rc_pass_grow(q, q.status, m))) return rc;
    if ((rc = rc_pass_grow(q, q.curv, m * 8))) return rc;
    if ((rc = rc_pass_grow(q, q.eig, m * 24))) return rc;
    if ((rc = rc_pass_grow(q, q.count, m * 4))) return rc;
    if ((rc = rc_pass_begin(q, 0))) return rc;
    nr_launch_normals(x->s, n, k, max_dist * max_dist, min_ratio, mode == IMMESH_NORMALS_VIEWPOINT ? viewpoint : nullptr, (const float*)x->pts.p,
                      (const RcNode*)x->tree.nodes.p, x->tree.n_in, (float*)q.normal.p, (double*)q.curv.p, (double*)q.eig.p, (int32_t*)q.count.p,
                      (uint8_t*)q.status.p, (unsigned long long*)q.cnt.p);
    if ((rc = rc_pass_end(q, 0, 1, 0, 0, 4))) return rc;
    rc_pass_counts(q, counts);
    q.n = n;
    q.have = true;
    if ((rc = rc_fetch(c, normal_out, q.normal.p, m * 12))) return rc;
    if ((rc = rc_fetch(c, curvature_out, q.curv.p, m * 8))) return rc;
    if ((rc = rc_fetch(c, eig_out, q.eig.p, m * 24))) return rc;
    if ((rc = rc_fetch(c, count_out, q.count.p, m * 4))) return rc;
    return rc_fetch(c, status_out, q.status.p, m);
}

int immesh_cloud_normals_get(immesh_cloud_index* x, float* normal_out, uint8_t* status_out, int64_t cap, int64_t* n_out) {
    if (!x) return IMMESH_E_INVAL;
    immesh_ctx* c = x->ctx;
    int rc;
    if ((rc = cx_built(x, "cloud_normals_get")) || (rc = rc_have(c, "cloud_normals_get", x->nr.have, NR_NONE))) return rc;
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
    if ((rc = nr_check_agree(x, r, "normals_agree_samples", true))) return rc;
    if (!x->q.have || x->q_rc != r || x->q_gen != r->sm.gen || x->q.n != r->sm.n) {
        c->err = "normals_agree_samples: no immesh_nearest_samples query of this caster since its last sampling";
        return IMMESH_E_INVAL;
    }
    const int64_t n = r->sm.n;
    if ((rc = nr_agree_begin(x, (size_t)n))) return rc;
    HIPCHK(c, hipStreamWaitEvent(x->s, r->sm.done, 0));   // the samples are complete before the launch reads their faces
    if ((rc = rc_pass_begin(q, 2))) return rc;
    nr_launch_agree_samples(x->s, (const int32_t*)r->sm.face.p, (const int32_t*)x->q.id.p, n, (const float*)q.normal.p, (const uint8_t*)q.status.p, q.n,
                            (const float*)r->vtx.p, r->n_vtx, (const int32_t*)r->faces.p, r->n_faces, (float*)q.agree.p, (float*)q.a.dist.p,
                            (uint8_t*)q.a.status.p, (unsigned long long*)q.cnt.p);
    if ((rc = nr_agree_end(x, n, counts))) return rc;
    return rc_fetch(c, agree_out, q.agree.p, (size_t)n * 4);
}

int immesh_normals_agree_cloud(immesh_cloud_index* x, immesh_raycaster* r, double max_dist, float* agree_out, int32_t* face_out, int64_t counts[4]) {
    if (!x) return IMMESH_E_INVAL;
    immesh_ctx* c = x->ctx;
    RcNormals& q = x->nr;
    int rc;
    if ((rc = nr_check_agree(x, r, "normals_agree_cloud", false))) return rc;
    if ((rc = rc_positive(c, "normals_agree_cloud", "max_dist", max_dist))) return rc;
    const int64_t n = q.n;
    if ((rc = nr_agree_begin(x, (size_t)n))) return rc;
    if ((rc = rc_pass_grow(q, q.face, (size_t)n * 4))) return rc;
    if ((rc = rc_pass_begin(q, 2))) return rc;
    nr_launch_agree_cloud(x->s, (const float*)x->pts.p, (const float*)q.normal.p, (const uint8_t*)q.status.p, n, max_dist * max_dist, (const float*)r->vtx.p,
                          r->n_vtx, (const int32_t*)r->faces.p, r->n_faces, (const RcNode*)r->tree.nodes.p, r->tree.n_in, (float*)q.agree.p,
                          (float*)q.a.dist.p, (int32_t*)q.face.p, (uint8_t*)q.a.status.p, (unsigned long long*)q.cnt.p);
    if ((rc = nr_agree_end(x, n, counts))) return rc;
    if ((rc = rc_fetch(c, agree_out, q.agree.p, (size_t)n * 4))) return rc;
    return rc_fetch(c, face_out, q.face.p, (size_t)n * 4);
}

int immesh_normals_agree_reduce(immesh_cloud_index* x, double bin_width, int32_t n_bins, immesh_closest_stats* stats, int64_t* hist_out) {
    if (!x) return IMMESH_E_INVAL;
    immesh_ctx* c = x->ctx;
    RcNormals& q = x->nr;
    int rc;   // (asked before the events exist: rc_dist_reduce records them)
    if ((rc = cx_built(x, "normals_agree_reduce")) ||
        (rc = rc_have(c, "normals_agree_reduce", q.have && q.a.have, "no agreement since the index's last normals (immesh_normals_agree_samples, immesh_normals_agree_cloud)")))
        return rc;
    return rc_dist_reduce(c, "normals_agree_reduce", "cloud_index", "no agreement has been made on this index", x->s, q.ev[4], q.ev[5], &q.ms[2], q.a,
                          bin_width, n_bins, stats, hist_out);
}

int immesh_normals_last_timing(immesh_cloud_index* x, float ms[3]) {
    if (!x || !ms) return IMMESH_E_INVAL;
    ms[0] = x->nr.ms[0]; ms[1] = x->nr.ms[1]; ms[2] = x->nr.ms[2];
    return 0;
}

}  // extern "C"
