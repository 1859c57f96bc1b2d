// Host side of the mesh depth rasterizer (include/immesh_render.h): argument checks, grow-only buffers, the launch sequence on the renderer's stream.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <string>
#include "../host_ctx.hpp"
#include "../../../include/immesh_shade.h"
#include "../colour/colour.hpp"
#include "../raycast/rc_host.hpp"
#include "render.hpp"

struct immesh_renderer {
    immesh_ctx* ctx = nullptr;
    hipStream_t s = nullptr;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    hipEvent_t ev_shade[2] = {nullptr, nullptr};
    int64_t* h_small = nullptr;   // pinned: [0] pairs of the render, [1] reinforced points, [2] the colour pass's range (two floats)
    RcBuf vtx, faces, rec, cnt, foff, temp, tiles, bins, depth, face;
    RcThin th;                       // reinforce
    RcBuf vrgb, vcol, rgb, srange;   // the colour pass: a soup's vertex bytes, packed vertex colours, the image, range keys + range + partials
    int64_t n_points = 0;
    float ms[2] = {0.0f, 0.0f};
    float shade_ms = 0.0f;
    double shade_lo_hi[2] = {0.0, 0.0};
};

// one colour pass behind a render: the checked immesh_shade and where the VERTEX colours come from
struct RdShadeJob {
    RdShade sh;
    const uint8_t* d_bytes = nullptr;   // VERTEX, soup: n_vtx x 3 bytes in device memory
    RdColourState st = {};              // VERTEX, live mesh: the colourer's arrays
    uint8_t* rgb_out = nullptr;
};

namespace {

constexpr int64_t RD_MAX_FACES = (int64_t)INT_MAX - 1;

int rd_check_camera(immesh_renderer* r, const immesh_camera* cam) {
    if (!cam) { r->ctx->err = "render: camera is NULL"; return IMMESH_E_INVAL; }
    if (cam->width <= 0 || cam->height <= 0 || cam->width > 8192 || cam->height > 8192) {
        r->ctx->err = "render: width and height must be in 1..8192 (got " + std::to_string(cam->width) + " x " + std::to_string(cam->height) + ")";
        return IMMESH_E_INVAL;
    }
    if (!(cam->focus > 0.0) || !std::isfinite(cam->focus)) { r->ctx->err = "render: focus must be finite and > 0"; return IMMESH_E_INVAL; }
    if (!(cam->z_near > 0.0) || !(cam->z_near < cam->z_far) || !std::isfinite(cam->z_far)) {
        r->ctx->err = "render: need 0 < z_near < z_far, both finite";
        return IMMESH_E_INVAL;
    }
    const int rc = rc_finite_pose(r->ctx, "render", "camera", cam->rot, cam->pos);
    if (rc) return rc;
    if (std::isnan(cam->downsample_res)) { r->ctx->err = "render: downsample_res is NaN"; return IMMESH_E_INVAL; }
    return 0;
}

// the colour pass's arguments (include/immesh_shade.h) -> job->sh
int rd_check_shade(immesh_renderer* r, const immesh_shade* sh, RdShadeJob* job) {
    immesh_ctx* c = r->ctx;
    if (!sh) { c->err = "shade: immesh_shade is NULL"; return IMMESH_E_INVAL; }
    if (sh->source != IMMESH_SHADE_WHITE && sh->source != IMMESH_SHADE_AXIS && sh->source != IMMESH_SHADE_VERTEX) {
        c->err = "shade: unknown source " + std::to_string(sh->source);
        return IMMESH_E_INVAL;
    }
    if (sh->axis < 0 || sh->axis > 2) { c->err = "shade: axis must be 0, 1 or 2 (got " + std::to_string(sh->axis) + ")"; return IMMESH_E_INVAL; }
    const float lo = (float)sh->axis_min, hi = (float)sh->axis_max;
    if (!std::isfinite(sh->axis_min) || !std::isfinite(sh->axis_max) || !std::isfinite(lo) || !std::isfinite(hi)) {
        c->err = "shade: the axis range must be finite (as floats)";
        return IMMESH_E_INVAL;
    }
    RdShade& o = job->sh;
    o.source = sh->source; o.axis = sh->axis; o.light = sh->light ? 1 : 0; o.bgr = sh->bgr ? 1 : 0; o.min_views = sh->min_views;
    o.range_from_vertices = sh->axis_min >= sh->axis_max ? 1 : 0;
    o.lo = lo; o.hi = hi;
    o.background = (uint32_t)sh->background[0] | ((uint32_t)sh->background[1] << 8) | ((uint32_t)sh->background[2] << 16);
    return 0;
}

// rasterize n_faces faces of device arrays (vtx n_vtx x 3 floats, faces n_faces x 3 ints), reinforce, copy the requested outputs to the host
// with a job: the colour pass behind it (include/immesh_shade.h), on the same stream, under an event pair of its own
int rd_render(immesh_renderer* r, const immesh_camera* cam, const float* d_vtx, int64_t n_vtx, const int32_t* d_faces, int64_t n_faces, float* depth_out,
              int32_t* face_out, const RdShadeJob* job = nullptr) {
    immesh_ctx* c = r->ctx;
    hipStream_t s = r->s;
    r->n_points = 0;
    RdCam rc;
    std::memcpy(rc.rot, cam->rot, sizeof(rc.rot));
    std::memcpy(rc.pos, cam->pos, sizeof(rc.pos));
    rc.f = cam->focus; rc.z_near = cam->z_near; rc.z_far = cam->z_far;
    rc.w = cam->width; rc.h = cam->height; rc.cx = cam->width / 2; rc.cy = cam->height / 2;
    rc.tiles_x = (rc.w + RD_TILE - 1) / RD_TILE; rc.tiles_y = (rc.h + RD_TILE - 1) / RD_TILE;
    const int n_tiles = rc.tiles_x * rc.tiles_y;
    const int64_t n_pix = (int64_t)rc.w * rc.h;
    const float res = (float)cam->downsample_res;
    int rc_ = 0;
    if ((rc_ = rc_grow(c, "render", r->rec, (size_t)n_faces * sizeof(RdFace)))) return rc_;
    if ((rc_ = rc_grow(c, "render", r->cnt, (size_t)n_faces * 8))) return rc_;
    if ((rc_ = rc_grow(c, "render", r->foff, (size_t)(n_faces + 1) * 8))) return rc_;
    if ((rc_ = rc_grow(c, "render", r->temp, rd_scan_temp_bytes(n_faces, n_tiles, n_pix) + 256))) return rc_;
    if ((rc_ = rc_grow(c, "render", r->tiles, (size_t)n_tiles * 12))) return rc_;
    if ((rc_ = rc_grow(c, "render", r->depth, (size_t)n_pix * 4))) return rc_;
    if ((rc_ = rc_grow(c, "render", r->face, (size_t)n_pix * 4))) return rc_;
    uint32_t mask = 0;
    RcThin& th = r->th;
    if ((rc_ = rc_thin_grow(c, "render", th, r->temp, n_pix, res, &mask))) return rc_;
    if (job) {
        if ((rc_ = rc_grow(c, "render", r->rgb, (size_t)n_pix * 3))) return rc_;
        if ((rc_ = rc_grow(c, "render", r->srange, 16 + 8 * (size_t)RD_SHADE_RANGE_PARTS))) return rc_;
        if (job->sh.source != IMMESH_SHADE_WHITE && (rc_ = rc_grow(c, "render", r->vcol, (size_t)n_vtx * 4))) return rc_;
    }
    RdFace* rec = (RdFace*)r->rec.p;
    int64_t* cnt = (int64_t*)r->cnt.p;
    int64_t* foff = (int64_t*)r->foff.p;
    int32_t* tile_cnt = (int32_t*)r->tiles.p;
    int32_t* tile_off = tile_cnt + n_tiles;
    int32_t* tile_fill = tile_off + n_tiles;
    float* depth = (float*)r->depth.p;
    int32_t* face = (int32_t*)r->face.p;

    // ---- rasterize
    HIPCHK(c, hipEventRecord(r->ev[0], s));
    rd_launch_setup(s, rc, d_vtx, n_vtx, d_faces, n_faces, rec, cnt);
    rd_scan_pairs(s, r->temp.p, r->temp.bytes, cnt, foff, n_faces);
    HIPCHK(c, hipMemcpyAsync(r->h_small, foff + n_faces, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    const int64_t n_pairs = r->h_small[0];
    if (n_pairs > (int64_t)INT_MAX) {
        c->err = "render: " + std::to_string(n_pairs) + " (face, tile) pairs in one render, more than 2^31 - 1";
        return IMMESH_E_CAPACITY;
    }
    if ((rc_ = rc_grow(c, "render", r->bins, (size_t)n_pairs * 4))) return rc_;
    HIPCHK(c, hipMemsetAsync(tile_cnt, 0, (size_t)n_tiles * 12, s));
    rd_launch_bin(s, rc, rec, foff, n_faces, n_pairs, 0, tile_cnt, nullptr, nullptr, nullptr);
    rd_scan_i32(s, r->temp.p, r->temp.bytes, tile_cnt, tile_off, n_tiles);
    rd_launch_bin(s, rc, rec, foff, n_faces, n_pairs, 1, tile_cnt, tile_off, tile_fill, (int32_t*)r->bins.p);
    rd_launch_resolve(s, rc, rec, tile_cnt, tile_off, (const int32_t*)r->bins.p, depth, face);
    HIPCHK(c, hipEventRecord(r->ev[1], s));

    // ---- reinforce
    rd_launch_unproject(s, rc, res, depth, (float*)th.pts.p, (float*)th.cells.p, (int32_t*)th.keep.p);
    if ((rc_ = rc_thin_run(c, s, th, r->temp, n_pix, res, mask, depth))) return rc_;
    if ((rc_ = rc_span_end(c, s, r->ev[1], r->ev[2], &r->ms[1], r->h_small + 1, th.small.p, 8))) return rc_;
    r->n_points = r->h_small[1];
    (void)hipEventElapsedTime(&r->ms[0], r->ev[0], r->ev[1]);   // (complete since the synchronisation above)

    // ---- colour pass
    if (job) {
        const RdShade& sh = job->sh;
        uint32_t* keys = (uint32_t*)r->srange.p;
        float* range = (float*)(keys + 2);
        const bool axis = sh.source == IMMESH_SHADE_AXIS;
        HIPCHK(c, hipEventRecord(r->ev_shade[0], s));
        if (axis && sh.range_from_vertices) rd_launch_shade_range(s, d_vtx, n_vtx, sh.axis, (uint32_t*)(range + 2), keys);
        if (sh.source != IMMESH_SHADE_WHITE) rd_launch_shade_colours(s, sh, d_vtx, n_vtx, job->d_bytes, job->st, keys, (uint32_t*)r->vcol.p, range);
        rd_launch_shade(s, rc, sh, rec, d_faces, face, sh.source == IMMESH_SHADE_WHITE ? nullptr : (const uint32_t*)r->vcol.p, (uint8_t*)r->rgb.p);
        if ((rc_ = rc_span_end(c, s, r->ev_shade[0], r->ev_shade[1], &r->shade_ms, r->h_small + 2, range, axis ? 8 : 0))) return rc_;
        float lo_hi[2] = {0.0f, 0.0f};
        if (axis) std::memcpy(lo_hi, r->h_small + 2, 8);
        r->shade_lo_hi[0] = (double)lo_hi[0]; r->shade_lo_hi[1] = (double)lo_hi[1];
        if (job->rgb_out) HIPCHK(c, hipMemcpy(job->rgb_out, r->rgb.p, (size_t)n_pix * 3, hipMemcpyDeviceToHost));
    }
    if (depth_out) HIPCHK(c, hipMemcpy(depth_out, depth, (size_t)n_pix * 4, hipMemcpyDeviceToHost));
    if (face_out) HIPCHK(c, hipMemcpy(face_out, face, (size_t)n_pix * 4, hipMemcpyDeviceToHost));
    return 0;
}

}  // namespace

extern "C" {

void immesh_default_depth_camera(immesh_camera* cam) {
    if (!cam) return;
    std::memset(cam, 0, sizeof(*cam));
    cam->rot[0] = cam->rot[4] = cam->rot[8] = 1.0;
    cam->width = 640; cam->height = 480;
    cam->focus = 400.0;
    cam->z_near = 0.05; cam->z_far = 200.0;
    cam->downsample_res = 0.01;
}

int immesh_camera_from_state(const double* state, immesh_camera* cam) {
    if (!state || !cam) return IMMESH_E_INVAL;
    static const double M[9] = {0, 0, -1, -1, 0, 0, 0, 1, 0};   // lidar_frame_to_camera_frame, ImMesh_node.cpp:174
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) cam->rot[3 * i + j] = (state[3 * i] * M[j] + state[3 * i + 1] * M[3 + j]) + state[3 * i + 2] * M[6 + j];
    for (int i = 0; i < 3; i++) cam->pos[i] = state[9 + i];
    return 0;
}

immesh_renderer* immesh_renderer_create(immesh_ctx* ctx) {
    if (!ctx) return nullptr;
    (void)hipSetDevice(ctx->cfg.device);
    immesh_renderer* r = new immesh_renderer();
    r->ctx = ctx;
    bool ok = hipStreamCreateWithFlags(&r->s, hipStreamNonBlocking) == hipSuccess;
    for (int i = 0; i < 3 && ok; i++) ok = hipEventCreate(&r->ev[i]) == hipSuccess;
    for (int i = 0; i < 2 && ok; i++) ok = hipEventCreate(&r->ev_shade[i]) == hipSuccess;
    ok = ok && hipHostMalloc((void**)&r->h_small, 32) == hipSuccess;
    if (!ok) {
        ctx->err = "immesh_renderer_create: stream / event / pinned allocation failed";
        immesh_renderer_destroy(r);
        return nullptr;
    }
    return r;
}

void immesh_renderer_destroy(immesh_renderer* r) {
    if (!r) return;
    (void)hipSetDevice(r->ctx->cfg.device);
    if (r->s) (void)hipStreamSynchronize(r->s);
    rc_destroy_events(r->ev, 3);
    rc_destroy_events(r->ev_shade, 2);
    if (r->h_small) (void)hipHostFree(r->h_small);
    if (r->s) (void)hipStreamDestroy(r->s);
    delete r;   // the members release their buffers
}

int immesh_render_triangles(immesh_renderer* r, const immesh_camera* cam, const float* vtx_xyz, int64_t n_vtx, const int32_t* faces, int64_t n_faces,
                            float* depth_out, int32_t* face_out) {
    if (!r) return IMMESH_E_INVAL;
    immesh_ctx* c = r->ctx;
    int rc = rd_check_camera(r, cam);
    if (rc) return rc;
    if ((rc = rc_check_soup(c, "render_triangles", RD_MAX_FACES, vtx_xyz, n_vtx, faces, n_faces))) return rc;
    (void)hipSetDevice(c->cfg.device);
    if ((rc = rc_upload_soup(c, "render", r->s, r->vtx, r->faces, vtx_xyz, n_vtx, faces, n_faces))) return rc;
    return rd_render(r, cam, (const float*)r->vtx.p, n_vtx, (const int32_t*)r->faces.p, n_faces, depth_out, face_out);
}

int immesh_render_mesh(immesh_renderer* r, const immesh_camera* cam, double smooth_factor, int32_t knn, float* depth_out, int32_t* face_out) {
    if (!r) return IMMESH_E_INVAL;
    immesh_ctx* c = r->ctx;
    int rc = rd_check_camera(r, cam);
    if (rc) return rc;
    int64_t nv = 0, nf = 0;
    if ((rc = immesh_mesh_export(c, smooth_factor, knn, &nv, &nf))) return rc;   // synchronises the ctx stream: the arrays are complete
    if (nf >= (int64_t)INT_MAX) { c->err = "render_mesh: more than 2^31 - 2 faces"; return IMMESH_E_CAPACITY; }
    const MeshHost& h = c->mesh_host;
    (void)hipSetDevice(c->cfg.device);
    return rd_render(r, cam, (const float*)h.exp_vtx, nv, h.exp_faces, nf, depth_out, face_out);
}

int immesh_render_points(immesh_renderer* r, float* xyz_out, int64_t cap, int64_t* n_out) {
    if (!r) return IMMESH_E_INVAL;
    return rc_thin_fetch(r->ctx, "render_points", r->th, r->n_points, xyz_out, cap, n_out);
}

int immesh_renderer_last_timing(immesh_renderer* r, float ms[2]) {
    if (!r || !ms) return IMMESH_E_INVAL;
    ms[0] = r->ms[0]; ms[1] = r->ms[1];
    return 0;
}

// ---- include/immesh_shade.h
void immesh_default_shade(immesh_shade* sh) {
    if (!sh) return;
    std::memset(sh, 0, sizeof(*sh));
    sh->source = IMMESH_SHADE_WHITE;
    sh->axis = 2;
    sh->light = 1;
}

int immesh_shade_triangles(immesh_renderer* r, const immesh_camera* cam, const float* vtx_xyz, int64_t n_vtx, const int32_t* faces, int64_t n_faces,
                           const uint8_t* vtx_rgb, const immesh_shade* sh, uint8_t* rgb_out, float* depth_out, int32_t* face_out) {
    if (!r) return IMMESH_E_INVAL;
    immesh_ctx* c = r->ctx;
    int rc = rd_check_camera(r, cam);
    if (rc) return rc;
    RdShadeJob job;
    if ((rc = rd_check_shade(r, sh, &job))) return rc;
    if ((rc = rc_check_soup(c, "shade_triangles", RD_MAX_FACES, vtx_xyz, n_vtx, faces, n_faces))) return rc;
    const bool bytes = sh->source == IMMESH_SHADE_VERTEX;
    if (bytes && !vtx_rgb) { c->err = "shade_triangles: source VERTEX without vertex colours"; return IMMESH_E_INVAL; }
    (void)hipSetDevice(c->cfg.device);
    if ((rc = rc_upload_soup(c, "render", r->s, r->vtx, r->faces, vtx_xyz, n_vtx, faces, n_faces))) return rc;
    if (bytes) {
        if ((rc = rc_grow(c, "render", r->vrgb, (size_t)n_vtx * 3))) return rc;
        if (n_vtx > 0) HIPCHK(c, hipMemcpyAsync(r->vrgb.p, vtx_rgb, (size_t)n_vtx * 3, hipMemcpyHostToDevice, r->s));
        job.d_bytes = (const uint8_t*)r->vrgb.p;
    }
    job.rgb_out = rgb_out;
    return rd_render(r, cam, (const float*)r->vtx.p, n_vtx, (const int32_t*)r->faces.p, n_faces, depth_out, face_out, &job);
}

int immesh_shade_mesh(immesh_renderer* r, const immesh_camera* cam, immesh_colourer* colourer, double smooth_factor, int32_t knn, const immesh_shade* sh,
                      uint8_t* rgb_out, float* depth_out, int32_t* face_out) {
    if (!r) return IMMESH_E_INVAL;
    immesh_ctx* c = r->ctx;
    if (c->mesh.shard_world > 1) { c->err = "shade_mesh: not available on a sharded mesher (shard_mesh)"; return IMMESH_E_INVAL; }
    int rc = rd_check_camera(r, cam);
    if (rc) return rc;
    RdShadeJob job;
    if ((rc = rd_check_shade(r, sh, &job))) return rc;
    const bool vertex = sh->source == IMMESH_SHADE_VERTEX;
    if (vertex && !colourer) { c->err = "shade_mesh: source VERTEX without a colourer"; return IMMESH_E_INVAL; }
    if (vertex && cl_colourer_ctx(colourer) != c) { c->err = "shade_mesh: the colourer belongs to another context"; return IMMESH_E_INVAL; }
    int64_t nv = 0, nf = 0;
    if ((rc = immesh_mesh_export(c, smooth_factor, knn, &nv, &nf))) return rc;   // synchronises the ctx stream: the arrays are complete
    if (nf >= (int64_t)INT_MAX) { c->err = "shade_mesh: more than 2^31 - 2 faces"; return IMMESH_E_CAPACITY; }
    if (vertex) {
        const ClState& st = cl_colourer_state(colourer);   // export vertex i is vertex i of the map (immesh_save_ply_rgb)
        if (nv > st.cap) { c->err = "shade_mesh: the export has more vertices than the colourer holds"; return IMMESH_E_CAPACITY; }
        for (int k = 0; k < 3; k++) job.st.rgb[k] = st.rgb[k];
        job.st.first_exposure = st.first_exposure; job.st.n_obs = st.n_obs;
    }
    job.rgb_out = rgb_out;
    const MeshHost& h = c->mesh_host;
    (void)hipSetDevice(c->cfg.device);
    return rd_render(r, cam, (const float*)h.exp_vtx, nv, h.exp_faces, nf, depth_out, face_out, &job);
}

int immesh_shade_range(immesh_renderer* r, double lo_hi[2]) {
    if (!r || !lo_hi) return IMMESH_E_INVAL;
    lo_hi[0] = r->shade_lo_hi[0]; lo_hi[1] = r->shade_lo_hi[1];
    return 0;
}

int immesh_renderer_last_shade_ms(immesh_renderer* r, float* ms) {
    if (!r || !ms) return IMMESH_E_INVAL;
    *ms = r->shade_ms;
    return 0;
}

}  // extern "C"
