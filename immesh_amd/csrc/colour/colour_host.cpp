// Host side of the vertex colourer (include/immesh_colour.h): argument checks, the colour state, grow-only buffers, the launch sequence of one image on
// the colourer's stream.  One image costs one host-to-device copy (the frame, through pinned staging) and one 64-byte copy back (the statistics);
// every count in between -- candidates of a RECENT set, holders of the selection -- stays on the device, the launches are sized by their upper bound.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>
#include "../host_ctx.hpp"
#include "../../../include/immesh_colour.h"
#include "../raycast/rc_host.hpp"
#include "colour.hpp"

struct immesh_colourer {
    immesh_ctx* ctx = nullptr;
    hipStream_t s = nullptr;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    ClState st = {};
    void* st_block = nullptr;                 // the state arrays, one allocation
    immesh_colour_stats* h_stats = nullptr;   // pinned (immesh_ctx::pinned)
    char* h_stage = nullptr; size_t h_stage_bytes = 0;   // pinned staging: the frame, an id list
    RcBuf img, ids, flags, off, cand, cell, depth, sel, uv, tab, temp, partials, small, fetch;
    int64_t n_sel = 0;                        // render set of the last image
    bool sel_identity = false;                // ... it is 0 .. n_sel - 1 (set ALL without selection: no list was written)
    const int32_t* d_sel = nullptr;
    float ms[3] = {0.0f, 0.0f, 0.0f};
};

namespace {

// The frame's staging buffer grows with the image size and is freed with the colourer, so it is a pinned allocation of the colourer's own:
// immesh_ctx::pinned (host_ctx.hpp) hands out fixed-size blocks that live until immesh_destroy -- right for the 64-byte statistics block, not for this.
int cl_grow_stage(immesh_colourer* r, size_t need) {
    if (r->h_stage_bytes >= need) return 0;
    if (r->h_stage) (void)hipHostFree(r->h_stage);
    r->h_stage = nullptr; r->h_stage_bytes = 0;
    const size_t want = need + need / 4 + 4096;
    if (hipHostMalloc((void**)&r->h_stage, want, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        r->h_stage = nullptr;
        r->ctx->err = "colour: hipHostMalloc(" + std::to_string(want) + " B) failed";
        return IMMESH_E_NOMEM;
    }
    r->h_stage_bytes = want;
    return 0;
}

int cl_inval(immesh_ctx* c, const std::string& msg) { c->err = "colour: " + msg; return IMMESH_E_INVAL; }

int cl_check_image(immesh_ctx* c, const immesh_image* im, int32_t model, int32_t set, double md) {
    if (!im) return cl_inval(c, "image is NULL");
    if (model != IMMESH_COLOUR_PLAIN && model != IMMESH_COLOUR_VIEW) return cl_inval(c, "unknown model " + std::to_string(model));
    if (set < IMMESH_COLOUR_SET_ALL || set > IMMESH_COLOUR_SET_RECENT_HEADS) return cl_inval(c, "unknown set " + std::to_string(set));
    if (!im->data) return cl_inval(c, "image data is NULL");
    if (im->rows < 2 || im->cols < 2 || im->rows > 8192 || im->cols > 8192)
        return cl_inval(c, "rows and cols must be in 2..8192 (got " + std::to_string(im->rows) + " x " + std::to_string(im->cols) + ")");
    if (im->row_stride_bytes < 3 * (int64_t)im->cols) return cl_inval(c, "row_stride_bytes " + std::to_string(im->row_stride_bytes) + " is below 3 * cols");
    for (double v : {im->fx, im->fy, im->cx, im->cy})
        if (!std::isfinite(v)) return cl_inval(c, "intrinsics are not finite");
    const int rc = rc_finite_pose(c, "colour", "camera", im->rot, im->pos);
    if (rc) return rc;
    if (!(im->fov_margin >= 0.0) || !(im->fov_margin < 0.5)) return cl_inval(c, "fov_margin must be in [0, 0.5)");
    if (!(im->inv_exposure > 0.0) || !std::isfinite(im->inv_exposure)) return cl_inval(c, "inv_exposure must be finite and > 0");
    for (double v : {im->obs_time, im->min_depth, im->max_depth, im->max_pe_error})
        if (!std::isfinite(v)) return cl_inval(c, "obs_time, min_depth, max_depth and max_pe_error must be finite");
    if (std::isnan(md) || md > 1024.0 || (md > 0.0 && md < 1.0 / 1024.0))
        return cl_inval(c, "select_min_dis must be <= 0 (no selection) or in [1 / 1024, 1024] pixels");
    return 0;
}

}  // namespace

immesh_ctx* cl_colourer_ctx(const immesh_colourer* c) { return c->ctx; }
const ClState& cl_colourer_state(const immesh_colourer* c) { return c->st; }

extern "C" {

void immesh_default_image(immesh_image* img) {
    if (!img) return;
    std::memset(img, 0, sizeof(*img));
    img->rot[0] = img->rot[4] = img->rot[8] = 1.0;
    img->fov_margin = 0.005;
    img->inv_exposure = 0.01;
    img->min_depth = 3.0; img->max_depth = 200.0;
    img->max_pe_error = 40.0;
}

immesh_colourer* immesh_colourer_create(immesh_ctx* ctx) {
    if (!ctx) return nullptr;
    (void)hipSetDevice(ctx->cfg.device);
    immesh_colourer* r = new immesh_colourer();
    r->ctx = ctx;
    const int64_t cap = ctx->mesh.shard_world > 1 ? 0 : ctx->mesh.cap_verts;   // (a sharded mesher: every call returns IMMESH_E_INVAL, no state is kept)
    bool ok = ctx->knobs.make_stream(&r->s, ctx->prio_least, false) == hipSuccess;
    for (int i = 0; i < 4 && ok; i++) ok = hipEventCreate(&r->ev[i]) == hipSuccess;
    ok = ok && ctx->pinned(&r->h_stats, (immesh_colour_stats**)nullptr, 1) == 0;
    ok = ok && hipMalloc(&r->st_block, (size_t)cap * 76 + 64) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        ctx->err = "immesh_colourer_create: stream / event / pinned / state (" + std::to_string((size_t)cap * 76) + " B) allocation failed";
        immesh_colourer_destroy(r);
        return nullptr;
    }
    double* d = (double*)r->st_block;
    for (int k = 0; k < 3; k++) { r->st.rgb[k] = d + (size_t)k * cap; r->st.cov[k] = d + (size_t)(3 + k) * cap; }
    r->st.first_exposure = d + (size_t)6 * cap; r->st.obs_dis = d + (size_t)7 * cap; r->st.last_obs_time = d + (size_t)8 * cap;
    r->st.n_obs = (int32_t*)(d + (size_t)9 * cap);
    r->st.cap = cap;
    cl_launch_state_init(r->s, r->st);
    if (hipStreamSynchronize(r->s) != hipSuccess) {
        ctx->err = "immesh_colourer_create: initialising the colour state failed";
        immesh_colourer_destroy(r);
        return nullptr;
    }
    return r;
}

void immesh_colourer_destroy(immesh_colourer* r) {
    if (!r) return;
    (void)hipSetDevice(r->ctx->cfg.device);
    if (r->s) (void)hipStreamSynchronize(r->s);
    if (r->st_block) (void)hipFree(r->st_block);
    rc_destroy_events(r->ev, 4);
    if (r->h_stage) (void)hipHostFree(r->h_stage);
    if (r->s) (void)hipStreamDestroy(r->s);
    delete r;   // the members release their buffers (h_stats belongs to the context's pinned blocks)
}

int immesh_colour_image(immesh_colourer* r, const immesh_image* im, int32_t model, int32_t set, const int32_t* ids, int64_t n_ids, double md,
                        immesh_colour_stats* out) {
    if (!r) return IMMESH_E_INVAL;
    immesh_ctx* c = r->ctx;
    if (c->mesh.shard_world > 1) return cl_inval(c, "not available on a sharded mesher (shard_mesh)");
    int rc = cl_check_image(c, im, model, set, md);
    if (rc) return rc;
    (void)hipSetDevice(c->cfg.device);
    mesh_wait_all(c);   // the map between two jobs: every submitted scan is meshed
    MeshHost& h = c->mesh_host;
    const MeshDev& m = c->mesh;
    const int nv = h.n_vertices;
    if (set == IMMESH_COLOUR_SET_IDS) {
        if (n_ids < 0 || n_ids > nv || (n_ids > 0 && !ids)) return cl_inval(c, "bad id list (" + std::to_string(n_ids) + " ids, " + std::to_string(nv) + " vertices)");
        for (int64_t i = 0; i < n_ids; i++) {
            if (ids[i] < 0 || ids[i] >= nv) return cl_inval(c, "id " + std::to_string(ids[i]) + " at " + std::to_string(i) + " is out of range [0, " + std::to_string(nv) + ")");
            if (i > 0 && ids[i] <= ids[i - 1]) return cl_inval(c, "ids must be strictly ascending (at " + std::to_string(i) + ")");
        }
    }
    // from here on buffers may be regrown: the last call's render set is gone whatever happens (immesh_colour_selected never reads a freed list)
    r->n_sel = 0; r->d_sel = nullptr; r->sel_identity = false;
    const bool select = md > 0.0;
    const bool recent = set == IMMESH_COLOUR_SET_RECENT || set == IMMESH_COLOUR_SET_RECENT_HEADS;
    const int n_bound = set == IMMESH_COLOUR_SET_IDS ? (int)n_ids : nv;   // upper bound of the candidate count (and of the render set)

    // ---- the image as the kernels read it
    ClCam cam;
    std::memcpy(cam.rot, im->rot, sizeof(cam.rot));
    std::memcpy(cam.pos, im->pos, sizeof(cam.pos));
    for (int k = 0; k < 3; k++) {
        cam.tc[k] = -((im->rot[k] * im->pos[0] + im->rot[3 + k] * im->pos[1]) + im->rot[6 + k] * im->pos[2]);
        cam.n[k] = im->rot[3 * k + 2];
    }
    cam.fx = im->fx; cam.fy = im->fy; cam.cx = im->cx; cam.cy = im->cy;
    cam.u_lo = im->fov_margin * im->cols + 1; cam.u_hi = (1 - im->fov_margin) * im->cols;
    cam.v_lo = im->fov_margin * im->rows + 1; cam.v_hi = (1 - im->fov_margin) * im->rows;
    cam.inv_exposure = im->inv_exposure; cam.obs_time = im->obs_time; cam.min_depth = im->min_depth; cam.max_depth = im->max_depth;
    cam.max_pe = im->max_pe_error; cam.allow = std::max(0.05, 0.1 * m.voxel);
    cam.rows = im->rows; cam.cols = im->cols; cam.stride = 3 * (int64_t)im->cols;

    // ---- buffers (grow-only: nothing is allocated after the first image of a size)
    const size_t img_bytes = (size_t)im->rows * (size_t)cam.stride;
    const size_t ids_bytes = set == IMMESH_COLOUR_SET_IDS ? (((size_t)n_ids * 4 + 63) & ~(size_t)63) : 0;
    const int pad = select ? (int)std::ceil(md / 2.0) + 2 : 0;
    const int tab_w = im->cols + pad;
    const int64_t tab_n = select ? (int64_t)tab_w * (im->rows + pad) : 0;
    const int n_blocks = std::max(1, cl_update_blocks(n_bound));
    const size_t nb = (size_t)std::max(n_bound, 1);
    if ((rc = cl_grow_stage(r, img_bytes + ids_bytes))) return rc;
    if ((rc = rc_grow(c, "colour", r->img, img_bytes))) return rc;
    if ((rc = rc_grow(c, "colour", r->small, sizeof(ClCounters) + sizeof(immesh_colour_stats)))) return rc;
    if ((rc = rc_grow(c, "colour", r->uv, nb * 8))) return rc;
    if ((rc = rc_grow(c, "colour", r->partials, (size_t)n_blocks * 8))) return rc;
    if (ids_bytes && (rc = rc_grow(c, "colour", r->ids, ids_bytes))) return rc;
    if (recent || select) {
        if ((rc = rc_grow(c, "colour", r->flags, nb * 4))) return rc;
        if ((rc = rc_grow(c, "colour", r->off, nb * 4))) return rc;
        if ((rc = rc_grow(c, "colour", r->temp, exclusive_sum_temp_bytes((int)nb) + 256))) return rc;
    }
    if (recent && (rc = rc_grow(c, "colour", r->cand, nb * 4))) return rc;
    if (select) {
        if ((rc = rc_grow(c, "colour", r->cell, nb * 4))) return rc;
        if ((rc = rc_grow(c, "colour", r->depth, nb * 8))) return rc;
        if ((rc = rc_grow(c, "colour", r->sel, nb * 4))) return rc;
        if ((rc = rc_grow(c, "colour", r->tab, (size_t)tab_n * 12))) return rc;
    }
    hipStream_t s = r->s;
    ClCounters* cnt = (ClCounters*)r->small.p;
    void* d_stats = (char*)r->small.p + sizeof(ClCounters);

    // ---- upload: the frame row by row into pinned staging (the stride is dropped), one copy; the id list behind it
    for (int y = 0; y < im->rows; y++) std::memcpy(r->h_stage + (size_t)y * cam.stride, im->data + (size_t)y * im->row_stride_bytes, (size_t)cam.stride);
    if (ids_bytes) std::memcpy(r->h_stage + img_bytes, ids, (size_t)n_ids * 4);
    HIPCHK(c, hipEventRecord(r->ev[0], s));   // (behind the host's packing: ms[0] is the copies alone)
    HIPCHK(c, hipMemcpyAsync(r->img.p, r->h_stage, img_bytes, hipMemcpyHostToDevice, s));
    if (ids_bytes) HIPCHK(c, hipMemcpyAsync(r->ids.p, r->h_stage + img_bytes, (size_t)n_ids * 4, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipEventRecord(r->ev[1], s));

    // ---- candidate set
    cl_launch_counters_init(s, cnt, n_bound, n_bound);
    const int32_t* d_cand = set == IMMESH_COLOUR_SET_IDS ? (const int32_t*)r->ids.p : nullptr;   // nullptr: 0 .. n - 1
    if (recent && nv > 0) {
        const int par = (int)(h.submitted % MESH_NPAR);   // the counters of the last meshed scan (none yet: zero)
        HIPCHK(c, hipMemsetAsync(r->flags.p, 0, (size_t)nv * 4, s));
        cl_launch_mark_recent(s, m.recent, h.mpar[par].sc + SC_RECENT, m.vx_npts, m.vx_pts, MV_VOX_CAP, nv, set == IMMESH_COLOUR_SET_RECENT_HEADS ? 1 : 0,
                              (int32_t*)r->flags.p);
        exclusive_sum_i32(s, r->temp.p, r->temp.bytes, (const int32_t*)r->flags.p, (int32_t*)r->off.p, nv);
        cl_launch_compact(s, (const int32_t*)r->flags.p, (const int32_t*)r->off.p, nullptr, nv, (int32_t*)r->cand.p, &cnt->n_cand);
        d_cand = (const int32_t*)r->cand.p;
    }
    // ---- selection
    const int32_t* d_sel = d_cand;
    if (select && n_bound > 0) {
        uint32_t* tab_min = (uint32_t*)r->tab.p;
        int32_t* tab_hi = (int32_t*)(tab_min + tab_n);
        uint32_t* tab_lo = (uint32_t*)(tab_hi + tab_n);
        HIPCHK(c, hipMemsetAsync(r->tab.p, 0xFF, (size_t)tab_n * 12, s));   // min 0xFFFFFFFF, hi -1, lo 0xFFFFFFFF
        cl_launch_select_min(s, cam, m.v_pos, d_cand, n_bound, cnt, md, tab_w, tab_n, (int32_t*)r->cell.p, (double*)r->depth.p, tab_min);
        cl_launch_select_rank(s, n_bound, cnt, (const int32_t*)r->cell.p, (const double*)r->depth.p, tab_min, tab_hi, tab_lo);
        cl_launch_select_keep(s, n_bound, cnt, (const int32_t*)r->cell.p, tab_hi, tab_lo, (int32_t*)r->flags.p);
        exclusive_sum_i32(s, r->temp.p, r->temp.bytes, (const int32_t*)r->flags.p, (int32_t*)r->off.p, n_bound);
        cl_launch_compact(s, (const int32_t*)r->flags.p, (const int32_t*)r->off.p, d_cand, n_bound, (int32_t*)r->sel.p, &cnt->n_sel);
        d_sel = (const int32_t*)r->sel.p;
    } else if (recent && nv > 0) {
        // (the render set is the candidate set: its count is known on the device only)
        HIPCHK(c, hipMemcpyAsync(&cnt->n_sel, &cnt->n_cand, 4, hipMemcpyDeviceToDevice, s));
    }
    HIPCHK(c, hipEventRecord(r->ev[2], s));

    // ---- update
    if (model == IMMESH_COLOUR_PLAIN) cl_launch_dmin(s, cam, m.v_pos, d_sel, n_bound, cnt);
    if (n_bound > 0) cl_launch_update(s, cam, model, m.v_pos, d_sel, n_bound, cnt, (const uint8_t*)r->img.p, r->st, (float*)r->uv.p, (double*)r->partials.p);
    cl_launch_finalize(s, model, cnt, (const double*)r->partials.p, n_bound > 0 ? n_blocks : 0, d_stats);
    if ((rc = rc_span_end(c, s, r->ev[2], r->ev[3], &r->ms[2], r->h_stats, d_stats, sizeof(immesh_colour_stats)))) return rc;
    for (int k = 0; k < 2; k++) (void)hipEventElapsedTime(&r->ms[k], r->ev[k], r->ev[k + 1]);   // the three spans share that one synchronisation
    r->n_sel = r->h_stats->n_selected;
    r->d_sel = d_sel;
    r->sel_identity = d_sel == nullptr;
    if (out) *out = *r->h_stats;
    return 0;
}

int immesh_colour_selected(immesh_colourer* r, int32_t* ids_out, float* uv_out, int64_t cap, int64_t* n_out) {
    if (!r) return IMMESH_E_INVAL;
    immesh_ctx* c = r->ctx;
    if (n_out) *n_out = r->n_sel;
    if ((!ids_out && !uv_out) || r->n_sel == 0) return 0;
    if (cap < r->n_sel) { c->err = "colour_selected: cap " + std::to_string(cap) + " < " + std::to_string(r->n_sel) + " vertices"; return IMMESH_E_CAPACITY; }
    (void)hipSetDevice(c->cfg.device);
    if (ids_out) {
        if (r->sel_identity) for (int64_t i = 0; i < r->n_sel; i++) ids_out[i] = (int32_t)i;
        else HIPCHK(c, hipMemcpy(ids_out, r->d_sel, (size_t)r->n_sel * 4, hipMemcpyDeviceToHost));
    }
    if (uv_out) HIPCHK(c, hipMemcpy(uv_out, r->uv.p, (size_t)r->n_sel * 8, hipMemcpyDeviceToHost));
    return 0;
}

int immesh_colour_fetch(immesh_colourer* r, const int32_t* ids, int64_t n, uint8_t* rgb_out, immesh_colour_state* state_out) {
    if (!r) return IMMESH_E_INVAL;
    immesh_ctx* c = r->ctx;
    if (n < 0 || (!ids && n > r->st.cap) || n > (int64_t)0x7fffffff) return cl_inval(c, "colour_fetch: bad count " + std::to_string(n));
    if (ids)
        for (int64_t i = 0; i < n; i++)
            if (ids[i] < 0 || (int64_t)ids[i] >= r->st.cap) return cl_inval(c, "colour_fetch: id " + std::to_string(ids[i]) + " is out of range");
    if (n == 0 || (!rgb_out && !state_out)) return 0;
    (void)hipSetDevice(c->cfg.device);
    // gathered on the device into array-of-structures records, CL_FETCH_CHUNK vertices at a time: the temporary stays at 5 MB however many are asked for
    constexpr int64_t CL_FETCH_CHUNK = 1 << 16;
    const size_t b_ids = (size_t)CL_FETCH_CHUNK * 4, b_state = (size_t)CL_FETCH_CHUNK * sizeof(immesh_colour_state);
    int rc;
    if ((rc = rc_grow(c, "colour", r->fetch, b_ids + b_state + (size_t)CL_FETCH_CHUNK * 3))) return rc;
    char* d = (char*)r->fetch.p;
    hipStream_t s = r->s;
    for (int64_t i0 = 0; i0 < n; i0 += CL_FETCH_CHUNK) {
        const int64_t k = std::min(CL_FETCH_CHUNK, n - i0);
        if (ids) HIPCHK(c, hipMemcpyAsync(d, ids + i0, (size_t)k * 4, hipMemcpyHostToDevice, s));
        cl_launch_gather(s, r->st, ids ? (const int32_t*)d : nullptr, i0, k, (uint8_t*)(d + b_ids + b_state), d + b_ids);
        HIPCHK(c, hipGetLastError());
        if (state_out) HIPCHK(c, hipMemcpyAsync(state_out + i0, d + b_ids, (size_t)k * sizeof(immesh_colour_state), hipMemcpyDeviceToHost, s));
        if (rgb_out) HIPCHK(c, hipMemcpyAsync(rgb_out + 3 * i0, d + b_ids + b_state, (size_t)k * 3, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));   // (the chunk's buffers are reused)
    }
    return 0;
}

// immesh_save_ply's layout plus uchar red green blue per vertex (binary little-endian)
int immesh_save_ply_rgb(immesh_colourer* r, const char* path, double smooth_factor, int32_t knn, int32_t min_views, int32_t bgr) {
    if (!r || !path) return IMMESH_E_INVAL;
    immesh_ctx* c = r->ctx;
    if (c->mesh.shard_world > 1) return cl_inval(c, "not available on a sharded mesher (shard_mesh)");
    int64_t nv = 0, nf = 0;
    int rc = immesh_mesh_export(c, smooth_factor, knn, &nv, &nf);
    if (rc) return rc;
    std::vector<float> v((size_t)nv * 3);
    std::vector<int32_t> f((size_t)nf * 3);
    std::vector<uint8_t> rgb((size_t)nv * 3);
    std::vector<immesh_colour_state> st((size_t)nv);
    if ((rc = immesh_mesh_export_fetch(c, v.data(), f.data()))) return rc;
    if ((rc = immesh_colour_fetch(r, nullptr, nv, rgb.data(), st.data()))) return rc;
    FILE* fp = std::fopen(path, "wb");
    if (!fp) { c->err = std::string("cannot open ") + path; return IMMESH_E_INVAL; }
    std::fprintf(fp, "ply\nformat binary_little_endian 1.0\ncomment immesh-mi355x\nelement vertex %lld\nproperty float x\nproperty float y\nproperty float z\n"
                     "property uchar red\nproperty uchar green\nproperty uchar blue\n"
                     "element face %lld\nproperty list uchar int vertex_indices\nend_header\n", (long long)nv, (long long)nf);
    std::vector<unsigned char> vrec((size_t)nv * 15);
    for (int64_t i = 0; i < nv; i++) {
        unsigned char* q = &vrec[(size_t)i * 15];
        std::memcpy(q, &v[(size_t)i * 3], 12);
        const bool seen = st[(size_t)i].n_obs >= min_views;
        const uint8_t* p = &rgb[(size_t)i * 3];
        q[12] = seen ? p[bgr ? 2 : 0] : 0; q[13] = seen ? p[1] : 0; q[14] = seen ? p[bgr ? 0 : 2] : 0;
    }
    std::fwrite(vrec.data(), 1, vrec.size(), fp);
    std::vector<unsigned char> rec((size_t)nf * 13);
    for (int64_t i = 0; i < nf; i++) { rec[(size_t)i * 13] = 3; std::memcpy(&rec[(size_t)i * 13 + 1], &f[(size_t)i * 3], 12); }
    std::fwrite(rec.data(), 1, rec.size(), fp);
    const bool ok = std::fclose(fp) == 0;
    if (!ok) { c->err = std::string("write failed: ") + path; return IMMESH_E_INVAL; }
    return 0;
}

int immesh_colourer_last_timing(immesh_colourer* r, float ms[3]) {
    if (!r || !ms) return IMMESH_E_INVAL;
    ms[0] = r->ms[0]; ms[1] = r->ms[1]; ms[2] = r->ms[2];
    return 0;
}

}  // extern "C"
