// Host side of the alignment of a cloud to the caster's snapshot (include/immesh_align.h): argument checks, grow-only buffers of its own (RcAlign: the
// closest query's results are not touched), the step on the caster's stream, the exact 6 x 6 solve, the update and the loop that keeps the cloud on
// the device.  Nothing here is allocated or launched unless an alignment is asked for.
#include <cmath>
#include <cstring>
#include <string>
#include "../host_ctx.hpp"
#include "../../../include/immesh_align.h"
#include "align.hpp"

static_assert(sizeof(immesh_align_options) == 64, "immesh_align_options layout");
static_assert(sizeof(immesh_align_system) == sizeof(AlSystemDev), "the folded system is copied as it lies");
static_assert(sizeof(immesh_align_result) == 368, "immesh_align_result layout");

bool al_nonneg_finite(double x) { return x >= 0.0 && std::isfinite(x); }

// ---- shared with the cloud rule (align_cloud_host.cpp): align.hpp declares them -----------------------------------------------------------------------
// the checks a step makes of its options: what it reads
int al_check_step(immesh_ctx* c, const char* who_, const immesh_align_options* o) {
    const std::string who = who_;
    if (!o) { c->err = who + ": options are NULL"; return IMMESH_E_INVAL; }
    if (const int rc = rc_positive(c, who.c_str(), "max_dist", o->max_dist)) return rc;
    if (o->mode != IMMESH_ALIGN_POINT && o->mode != IMMESH_ALIGN_PLANE) { c->err = who + ": mode " + std::to_string(o->mode) + " is neither 0 (POINT) nor 1 (PLANE)"; return IMMESH_E_INVAL; }
    for (int k = 0; k < 3; k++)
        if (!std::isfinite(o->centre[k])) { c->err = who + ": centre is not finite"; return IMMESH_E_INVAL; }
    return 0;
}

// what the loop reads of its options besides
int al_check_loop(immesh_ctx* c, const char* who_, const immesh_align_options* opts) {
    const std::string who = who_;
    if (!al_nonneg_finite(opts->damping)) { c->err = who + ": need damping >= 0, finite"; return IMMESH_E_INVAL; }
    if (opts->max_iters < 1 || opts->max_iters > 10000) { c->err = who + ": max_iters " + std::to_string(opts->max_iters) + " outside [1, 10000]"; return IMMESH_E_INVAL; }
    if (!al_nonneg_finite(opts->eps_rot) || !al_nonneg_finite(opts->eps_trans)) { c->err = who + ": need eps_rot and eps_trans >= 0, finite"; return IMMESH_E_INVAL; }
    return 0;
}

int al_check_loop_out(immesh_ctx* c, const char* who_, const immesh_align_result* result_out, const double* history_out, int64_t history_cap) {
    const std::string who = who_;
    if (!result_out) { c->err = who + ": result_out is NULL"; return IMMESH_E_INVAL; }
    if (history_cap < 0 || (history_cap > 0 && !history_out)) { c->err = who + ": bad history array"; return IMMESH_E_INVAL; }
    return 0;
}

void al_identity(RcFrame* fr) {
    *fr = RcFrame{};
    fr->rot[0] = fr->rot[4] = fr->rot[8] = 1.0;
}

// The Loop rule of the header, for both rules: the statements between two steps stand here and nowhere else.
int al_loop(const immesh_align_options& o, const RcFrame& fr0, AlStepFn step, void* self, float* total_ms, immesh_align_result* result_out,
            double* history_out, int64_t history_cap) {
    int rc;
    RcFrame fr = fr0;
    immesh_ray_frame frame;
    std::memcpy(frame.rot, fr.rot, sizeof fr.rot);
    std::memcpy(frame.pos, fr.pos, sizeof fr.pos);
    const int64_t need = o.mode == IMMESH_ALIGN_PLANE ? 6 : 3;
    immesh_align_result res = {};
    res.status = IMMESH_ALIGN_MAX_ITERS;
    float total = 0.0f;
    for (int it = 0; it < o.max_iters; it++) {
        std::memcpy(fr.rot, frame.rot, sizeof fr.rot);
        std::memcpy(fr.pos, frame.pos, sizeof fr.pos);
        float ms = 0.0f;
        if ((rc = step(self, fr, &res.system, &ms))) return rc;
        total += ms;
        res.iterations = it + 1;
        const int64_t rows = o.mode == IMMESH_ALIGN_PLANE ? res.system.n_used : 3 * res.system.n_used;
        res.rms = rows > 0 ? std::sqrt(res.system.e / (double)rows) : 0.0;
        double delta[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, nw = 0.0, nv = 0.0;
        bool stop = false;
        if (res.system.n_used < need) {
            res.status = IMMESH_ALIGN_TOO_FEW;
            stop = true;
        } else if (immesh_align_solve(&res.system, o.damping, delta) != 0) {
            res.status = IMMESH_ALIGN_DEGENERATE;
            stop = true;
        } else {
            (void)immesh_align_update(&frame, o.centre, delta, &frame);
            nw = std::sqrt((delta[0] * delta[0] + delta[1] * delta[1]) + delta[2] * delta[2]);
            nv = std::sqrt((delta[3] * delta[3] + delta[4] * delta[4]) + delta[5] * delta[5]);
            if (nw <= o.eps_rot && nv <= o.eps_trans) {
                res.status = IMMESH_ALIGN_CONVERGED;
                stop = true;
            }
        }
        if (it < history_cap) {
            double* h = history_out + 4 * (size_t)it;
            h[0] = (double)res.system.n_used; h[1] = res.rms; h[2] = nw; h[3] = nv;
        }
        if (stop) break;
    }
    *total_ms = total;
    res.frame = frame;
    *result_out = res;
    return 0;
}

namespace {

int al_h_index(int a, int b) { return a * (13 - a) / 2 + (b - a); }   // a <= b

int al_check_points(immesh_ctx* c, const std::string& who, const float* pts, int64_t n_pts) {
    return rc_points(c, who.c_str(), pts, n_pts);
}

// the record's events and pinned words, the cloud on the device (queued on the caster's stream)
int al_upload(immesh_raycaster* r, const float* pts, int64_t n_pts) {
    immesh_ctx* c = r->ctx;
    RcAlign& al = r->al;
    (void)hipSetDevice(c->cfg.device);
    for (hipEvent_t& e : al.ev)
        if (!e) HIPCHK(c, hipEventCreate(&e));
    if (!al.h_res) HIPCHK(c, hipHostMalloc((void**)&al.h_res, sizeof(AlSystemDev)));
    int rc;
    const size_t n = (size_t)n_pts;
    if ((rc = rc_grow(c, "align", al.pts, n * 12))) return rc;
    if ((rc = rc_grow(c, "align", al.part, (size_t)al_blocks(n_pts) * sizeof(AlSystemDev)))) return rc;
    if ((rc = rc_grow(c, "align", al.res, sizeof(AlSystemDev)))) return rc;
    if (al.variant == 1) {
        if ((rc = rc_grow(c, "align", al.sface, n * 4))) return rc;
        if ((rc = rc_grow(c, "align", al.sq, n * 24))) return rc;
    }
    if (n_pts > 0) HIPCHK(c, hipMemcpyAsync(al.pts.p, pts, n * 12, hipMemcpyHostToDevice, r->s));
    return 0;
}

// one step over the uploaded cloud: the launches, the folded system to pinned memory, the stream idle; ms[0] = its device time
int al_step(immesh_raycaster* r, const RcFrame& fr, int has_frame, int64_t n_pts, const immesh_align_options& o, immesh_align_system* sys, int32_t* face_dev,
            double* terms_dev) {
    immesh_ctx* c = r->ctx;
    RcAlign& al = r->al;
    hipStream_t s = r->s;
    const double r2 = o.max_dist * o.max_dist;
    HIPCHK(c, hipEventRecord(al.ev[0], s));
    if (al.variant == 1)
        al_launch_step_split(s, fr, has_frame, (const float*)al.pts.p, n_pts, r2, o.mode, o.centre, (const float*)r->vtx.p, (const int32_t*)r->faces.p,
                             (const RcNode*)r->tree.nodes.p, r->tree.n_in, (int32_t*)al.sface.p, (double*)al.sq.p, (AlSystemDev*)al.part.p,
                             (AlSystemDev*)al.res.p, face_dev, terms_dev);
    else
        al_launch_step(s, al.variant == 0, fr, has_frame, (const float*)al.pts.p, n_pts, r2, o.mode, o.centre, (const float*)r->vtx.p, (const int32_t*)r->faces.p,
                       (const RcNode*)r->tree.nodes.p, r->tree.n_in, (AlSystemDev*)al.part.p, (AlSystemDev*)al.res.p, face_dev, terms_dev);
    HIPCHK(c, hipEventRecord(al.ev[1], s));
    HIPCHK(c, hipMemcpyAsync(al.h_res, al.res.p, sizeof(AlSystemDev), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(s));
    (void)hipEventElapsedTime(&al.ms[0], al.ev[0], al.ev[1]);
    std::memcpy(sys, al.h_res, sizeof(AlSystemDev));
    return 0;
}

// the loop's step on the caster: the uploaded cloud under a frame, nothing stored per point
struct AlMeshLoop {
    immesh_raycaster* r;
    int64_t n_pts;
    const immesh_align_options* opts;
};
int al_mesh_step(void* self, const RcFrame& fr, immesh_align_system* sys, float* ms) {
    const AlMeshLoop& l = *(const AlMeshLoop*)self;
    const int rc = al_step(l.r, fr, 1, l.n_pts, *l.opts, sys, nullptr, nullptr);
    *ms = l.r->al.ms[0];
    return rc;
}

}  // namespace

extern "C" {

void immesh_align_default_options(immesh_align_options* o) {
    if (!o) return;
    *o = immesh_align_options{};
    o->mode = IMMESH_ALIGN_POINT;
    o->max_iters = 30;
    o->max_dist = 1.0;
    o->eps_rot = 1e-9;
    o->eps_trans = 1e-9;
}

int immesh_align_solve(const immesh_align_system* sys, double damping, double delta_out[6]) {
    if (!sys || !delta_out || !al_nonneg_finite(damping)) return IMMESH_E_INVAL;
    for (int k = 0; k < 6; k++) delta_out[k] = 0.0;
    double A[6][6], L[6][6] = {};
    for (int a = 0; a < 6; a++)
        for (int b = a; b < 6; b++) A[a][b] = A[b][a] = sys->H[al_h_index(a, b)];
    for (int a = 0; a < 6; a++) A[a][a] = A[a][a] + damping;
    double m = A[0][0];
    for (int a = 1; a < 6; a++)
        if (A[a][a] > m) m = A[a][a];
    for (int j = 0; j < 6; j++) {
        double s = A[j][j];
        for (int k = 0; k < j; k++) s = s - L[j][k] * L[j][k];
        if (!std::isfinite(s) || s <= 0.0 || s <= 0x1p-40 * m) return 1;
        L[j][j] = std::sqrt(s);
        for (int i = j + 1; i < 6; i++) {
            double t = A[i][j];
            for (int k = 0; k < j; k++) t = t - L[i][k] * L[j][k];
            L[i][j] = t / L[j][j];
        }
    }
    double y[6], d[6];
    for (int i = 0; i < 6; i++) {
        double t = sys->g[i];
        for (int k = 0; k < i; k++) t = t - L[i][k] * y[k];
        y[i] = t / L[i][i];
    }
    for (int i = 5; i >= 0; i--) {
        double t = y[i];
        for (int k = i + 1; k < 6; k++) t = t - L[k][i] * d[k];
        d[i] = t / L[i][i];
    }
    for (int k = 0; k < 6; k++) delta_out[k] = d[k];
    return 0;
}

int immesh_align_update(const immesh_ray_frame* frame, const double centre[3], const double delta[6], immesh_ray_frame* frame_out) {
    if (!frame || !centre || !delta || !frame_out) return IMMESH_E_INVAL;
    const double w[3] = {delta[0], delta[1], delta[2]};
    const double K[3][3] = {{0.0, -w[2], w[1]}, {w[2], 0.0, -w[0]}, {-w[1], w[0], 0.0}};
    const double th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2];
    const double th = std::sqrt(th2);
    double E[3][3];
    if (th < 0x1p-26) {
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) E[i][j] = (i == j ? 1.0 : 0.0) + K[i][j];
    } else {
        const double a = std::sin(th) / th;
        const double h = std::sin(0.5 * th);
        const double b = (2.0 * (h * h)) / th2;
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) {
                const double kk = (K[i][0] * K[0][j] + K[i][1] * K[1][j]) + K[i][2] * K[2][j];
                E[i][j] = ((i == j ? 1.0 : 0.0) + a * K[i][j]) + b * kk;
            }
    }
    immesh_ray_frame out;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) out.rot[3 * i + j] = (E[i][0] * frame->rot[j] + E[i][1] * frame->rot[3 + j]) + E[i][2] * frame->rot[6 + j];
    const double d[3] = {frame->pos[0] - centre[0], frame->pos[1] - centre[1], frame->pos[2] - centre[2]};
    for (int i = 0; i < 3; i++) out.pos[i] = (((E[i][0] * d[0] + E[i][1] * d[1]) + E[i][2] * d[2]) + centre[i]) + delta[3 + i];
    *frame_out = out;
    return 0;
}

int immesh_align_step(immesh_raycaster* r, const immesh_ray_frame* frame, const float* pts, int64_t n_pts, const immesh_align_options* opts,
                      immesh_align_system* system_out, int32_t* face_out, double* terms_out) {
    if (!r) return IMMESH_E_INVAL;
    immesh_ctx* c = r->ctx;
    RcAlign& al = r->al;
    int rc;
    if ((rc = rc_built(r, "align_step"))) return rc;
    if ((rc = al_check_step(c, "align_step", opts))) return rc;
    if ((rc = al_check_points(c, "align_step", pts, n_pts))) return rc;
    RcFrame fr = {};
    if (frame && (rc = rc_frame(c, "align_step", frame, &fr))) return rc;
    if ((rc = al_upload(r, pts, n_pts))) return rc;
    const size_t n = (size_t)n_pts;
    if (face_out && (rc = rc_grow(c, "align", al.face, n * 4))) return rc;
    if (terms_out && (rc = rc_grow(c, "align", al.terms, n * AL_TERMS * 8))) return rc;
    immesh_align_system sys;
    if ((rc = al_step(r, fr, frame != nullptr, n_pts, *opts, &sys, face_out ? (int32_t*)al.face.p : nullptr, terms_out ? (double*)al.terms.p : nullptr)))
        return rc;
    al.ms[1] = al.ms[0];
    if (system_out) *system_out = sys;
    if ((rc = rc_fetch(c, face_out, al.face.p, n * 4))) return rc;
    return rc_fetch(c, terms_out, al.terms.p, n * AL_TERMS * 8);
}

int immesh_align(immesh_raycaster* r, const immesh_ray_frame* frame0, const float* pts, int64_t n_pts, const immesh_align_options* opts,
                 immesh_align_result* result_out, double* history_out, int64_t history_cap) {
    if (!r) return IMMESH_E_INVAL;
    immesh_ctx* c = r->ctx;
    RcAlign& al = r->al;
    int rc;
    if ((rc = rc_built(r, "align"))) return rc;
    if ((rc = al_check_step(c, "align", opts))) return rc;
    if ((rc = al_check_loop(c, "align", opts))) return rc;
    if ((rc = al_check_points(c, "align", pts, n_pts))) return rc;
    if ((rc = al_check_loop_out(c, "align", result_out, history_out, history_cap))) return rc;
    RcFrame fr;
    al_identity(&fr);
    if (frame0 && (rc = rc_frame(c, "align", frame0, &fr))) return rc;
    if ((rc = al_upload(r, pts, n_pts))) return rc;
    AlMeshLoop self = {r, n_pts, opts};
    return al_loop(*opts, fr, al_mesh_step, &self, &al.ms[1], result_out, history_out, history_cap);
}

int immesh_align_last_timing(immesh_raycaster* r, float ms[2]) {
    if (!r || !ms) return IMMESH_E_INVAL;
    ms[0] = r->al.ms[0]; ms[1] = r->al.ms[1];
    return 0;
}

int immesh_align_set_variant(immesh_raycaster* r, int32_t variant) {
    if (!r) return IMMESH_E_INVAL;
    if (variant < 0 || variant > 2) { r->ctx->err = "align_set_variant: variant " + std::to_string(variant) + " is none of 0 (fused), 1 (split), 2 (fused, registers not capped)"; return IMMESH_E_INVAL; }
    r->al.variant = variant;
    return 0;
}

}  // extern "C"
