// Host side of the alignment of a cloud to the indexed cloud (include/immesh_align.h, the Cloud rule): argument checks, a record of its own on the
// index (RcCloudAlign: the index's query results, neighbour results, masks, clusters and normals are not touched), the step on the index's stream and
// the loop, which is align_host.cpp's al_loop over this rule's step.  Every check stands before the first launch and before anything of the index is
// touched.  Nothing here is allocated or launched unless an alignment to the index is asked for.
#include <cmath>
#include <cstring>
#include <string>
#include "../host_ctx.hpp"
#include "../../../include/immesh_align.h"
#include "align.hpp"

namespace {

constexpr int ALC_WORDS = (int)(sizeof(AlSystemDev) / 8);   // the folded system as the record's counters: 28 sums and 4 counts

// what both entry points ask of the index and of the options a step reads
int alc_check_step(immesh_cloud_index* x, const char* who, const immesh_align_options* o, double huber) {
    immesh_ctx* c = x->ctx;
    int rc;
    if ((rc = cx_built(x, who)) || (rc = al_check_step(c, who, o))) return rc;
    if (!al_nonneg_finite(huber)) { c->err = std::string(who) + ": need huber >= 0, finite"; return IMMESH_E_INVAL; }
    if (o->mode == IMMESH_ALIGN_PLANE)
        return rc_have(c, who, x->nr.have && x->nr.n == x->n_pts, "PLANE mode needs the index's normals: none since its last build or apply (immesh_cloud_normals)");
    return 0;
}

// the record ready, its buffers for n_pts points, the cloud on the device (queued on the index's stream)
int alc_upload(immesh_cloud_index* x, const float* pts, int64_t n_pts, bool want_index, bool want_terms) {
    RcCloudAlign& a = x->ca;
    int rc;
    const size_t n = (size_t)n_pts;
    if ((rc = cx_ready(x, a, ALC_WORDS, ALC_WORDS))) return rc;
    if ((rc = rc_pass_grow(a, a.pts, n * 12))) return rc;
    if ((rc = rc_pass_grow(a, a.part, (size_t)al_blocks(n_pts) * sizeof(AlSystemDev)))) return rc;
    if (a.variant == 1) {
        if ((rc = rc_pass_grow(a, a.sindex, n * 4))) return rc;
        if ((rc = rc_pass_grow(a, a.sq, n * 24))) return rc;
    }
    if (want_index && (rc = rc_pass_grow(a, a.index, n * 4))) return rc;
    if (want_terms && (rc = rc_pass_grow(a, a.terms, n * AL_TERMS * 8))) return rc;
    if (n_pts > 0) HIPCHK(x->ctx, hipMemcpyAsync(a.pts.p, pts, n * 12, hipMemcpyHostToDevice, x->s));
    return 0;
}

struct AlcStep {
    immesh_cloud_index* x;
    int has_frame;
    int64_t n_pts;
    const immesh_align_options* opts;
    double huber;
    int32_t* index_dev;
    double* terms_dev;
};

// one step over the uploaded cloud: the launches, the folded system to pinned memory, the stream idle
int alc_step(void* self, const RcFrame& fr, immesh_align_system* sys, float* ms) {
    const AlcStep& l = *(const AlcStep*)self;
    immesh_cloud_index* x = l.x;
    RcCloudAlign& a = x->ca;
    const immesh_align_options& o = *l.opts;
    const double r2 = o.max_dist * o.max_dist;
    const bool plane = o.mode == IMMESH_ALIGN_PLANE;
    const float* normal = plane ? (const float*)x->nr.normal.p : nullptr;
    const uint8_t* nstatus = plane ? (const uint8_t*)x->nr.status.p : nullptr;
    HIPCHK(x->ctx, hipEventRecord(a.ev[0], x->s));
    if (a.variant == 1)
        alc_launch_step_split(x->s, fr, l.has_frame, (const float*)a.pts.p, l.n_pts, r2, o.mode, o.centre, l.huber, (const float*)x->pts.p, normal, nstatus,
                              (const RcNode*)x->tree.nodes.p, x->tree.n_in, (int32_t*)a.sindex.p, (double*)a.sq.p, (AlSystemDev*)a.part.p,
                              (AlSystemDev*)a.cnt.p, l.index_dev, l.terms_dev);
    else
        alc_launch_step(x->s, fr, l.has_frame, (const float*)a.pts.p, l.n_pts, r2, o.mode, o.centre, l.huber, (const float*)x->pts.p, normal, nstatus,
                        (const RcNode*)x->tree.nodes.p, x->tree.n_in, (AlSystemDev*)a.part.p, (AlSystemDev*)a.cnt.p, l.index_dev, l.terms_dev);
    const int rc = rc_span_end(x->ctx, x->s, a.ev[0], a.ev[1], &a.ms[0], a.h_cnt, a.cnt.p, sizeof(AlSystemDev));
    if (rc) return rc;
    std::memcpy(sys, a.h_cnt, sizeof(AlSystemDev));
    *ms = a.ms[0];
    return 0;
}

}  // namespace

extern "C" {

int immesh_align_cloud_step(immesh_cloud_index* x, const immesh_ray_frame* frame, const float* pts, int64_t n_pts, const immesh_align_options* opts,
                            double huber, immesh_align_system* system_out, int32_t* index_out, double* terms_out) {
    if (!x) return IMMESH_E_INVAL;
    immesh_ctx* c = x->ctx;
    RcCloudAlign& a = x->ca;
    int rc;
    if ((rc = alc_check_step(x, "align_cloud_step", opts, huber))) return rc;
    if ((rc = rc_points(c, "align_cloud_step", pts, n_pts))) return rc;
    RcFrame fr = {};
    if (frame && (rc = rc_frame(c, "align_cloud_step", frame, &fr))) return rc;
    if ((rc = alc_upload(x, pts, n_pts, index_out != nullptr, terms_out != nullptr))) return rc;
    AlcStep st = {x, frame != nullptr, n_pts, opts, huber, index_out ? (int32_t*)a.index.p : nullptr, terms_out ? (double*)a.terms.p : nullptr};
    immesh_align_system sys;
    float ms;
    if ((rc = alc_step(&st, fr, &sys, &ms))) return rc;
    a.ms[1] = ms;
    if (system_out) *system_out = sys;
    const size_t n = (size_t)n_pts;
    if ((rc = rc_fetch(c, index_out, a.index.p, n * 4))) return rc;
    return rc_fetch(c, terms_out, a.terms.p, n * AL_TERMS * 8);
}

int immesh_align_cloud(immesh_cloud_index* x, const immesh_ray_frame* frame0, const float* pts, int64_t n_pts, const immesh_align_options* opts, double huber,
                       immesh_align_result* result_out, double* history_out, int64_t history_cap) {
    if (!x) return IMMESH_E_INVAL;
    immesh_ctx* c = x->ctx;
    int rc;
    if ((rc = alc_check_step(x, "align_cloud", opts, huber))) return rc;
    if ((rc = al_check_loop(c, "align_cloud", opts))) return rc;
    if ((rc = rc_points(c, "align_cloud", pts, n_pts))) return rc;
    if ((rc = al_check_loop_out(c, "align_cloud", result_out, history_out, history_cap))) return rc;
    RcFrame fr;
    al_identity(&fr);
    if (frame0 && (rc = rc_frame(c, "align_cloud", frame0, &fr))) return rc;
    if ((rc = alc_upload(x, pts, n_pts, false, false))) return rc;
    AlcStep st = {x, 1, n_pts, opts, huber, nullptr, nullptr};
    return al_loop(*opts, fr, alc_step, &st, &x->ca.ms[1], result_out, history_out, history_cap);
}

int immesh_align_cloud_last_timing(immesh_cloud_index* x, float ms[2]) {
    if (!x || !ms) return IMMESH_E_INVAL;
    ms[0] = x->ca.ms[0]; ms[1] = x->ca.ms[1];
    return 0;
}

int immesh_align_cloud_set_variant(immesh_cloud_index* x, int32_t variant) {
    if (!x) return IMMESH_E_INVAL;
    if (variant < 0 || variant > 1) { x->ctx->err = "align_cloud_set_variant: variant " + std::to_string(variant) + " is neither 0 (fused) nor 1 (split)"; return IMMESH_E_INVAL; }
    x->ca.variant = variant;
    return 0;
}

}  // extern "C"
