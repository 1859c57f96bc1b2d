/* immesh_colour.h -- per-vertex radiance of the mesh map from camera images, on the device (libimmesh_hip.so).
 *
 * Reference: README 2.3 "rapid, lossless texture reconstruction".  RGB_pts carries m_rgb, m_cov_rgb, m_N_rgb, m_obs_dis, m_last_obs_time and
 * m_first_obs_exposure_time; every camera frame updates them:
 *   src/meshing/r3live/pointcloud_rgbd.cpp:754-768   Global_map::render_with_a_image
 *   src/meshing/r3live/pointcloud_rgbd.cpp:554-605   render_pts_in_voxels                                  (IMMESH_COLOUR_PLAIN)
 *   src/meshing/r3live/pointcloud_rgbd.cpp:613-751   thread_render_pts_in_voxel, render_pts_in_voxels_mp   (IMMESH_COLOUR_VIEW)
 *   src/meshing/r3live/pointcloud_rgbd.cpp:770-874   selection_points_for_projection
 *   src/meshing/r3live/pointcloud_rgbd.cpp:118-195   RGB_pts::update_rgb
 *   src/meshing/r3live/image_frame.cpp:136-239, :323-358   project_3d_point_in_this_img, getSubPixel, get_rgb
 *   src/meshing/r3live/pointcloud_rgbd.cpp:876-919   save_to_pcd
 * Here the vertex store stays in HBM; the colour state lives beside it in an object of its own (the colourer), one image is uploaded per call and only
 * a 64-byte statistics block comes back.  Nothing is allocated or launched unless a colourer is created.
 *
 * These declarations are part of the C ABI of immesh_c_api.h (which includes this file).  They live in a header of their own because the C++ oracle
 * mirrors immesh_c_api.h's per-scan entry points one-to-one; the colourer's checker is a restatement of the contract below (tests/colour_checker.py).
 *
 * ---- Contract (exact; all arithmetic in IEEE double, in the order written, no fused multiply-add) -------------------------------------------
 *   Pose:    rot[r][k] = rot[3 r + k].  n = (rot[2], rot[5], rot[8]) (the optical axis, m_image_norm).
 *            tc[k] = -((rot[0][k] pos[0] + rot[1][k] pos[1]) + rot[2][k] pos[2]), once per image on the host.
 *            The vertex is p = (double)v_pos, raw, never smoothed; d = p - pos;  pc[k] = ((rot[0][k] p.x + rot[1][k] p.y) + rot[2][k] p.z) + tc[k].
 *            (The reference rotates with Eigen's quaternion product; that rounding is not reproduced.)
 *   Project: a miss when pc.z < 0.001.  u = (pc.x fx) / pc.z + cx,  v = (pc.y fy) / pc.z + cy.
 *            Available when u >= m cols + 1 && ceil(u) < (1 - m) cols && v >= m rows + 1 && ceil(v) < (1 - m) rows, m = fov_margin.
 *   Sample:  getSubPixel<cv::Vec3b>: r0 = floor(v), c0 = floor(u), a = v - r0, b = u - c0; P[r][c] the 8-bit pixel.  Per channel
 *              t00 = R8(((1 - a) (1 - b)) P[r0][c0]),  t10 = R8((a (1 - b)) P[r0 + 1][c0]),
 *              t01 = R8(((1 - a) b) P[r0][c0 + 1]),    t11 = R8((a b) P[r0 + 1][c0 + 1]),      c = S8(S8(S8(t00 + t10) + t01) + t11)
 *            R8(x) = round-half-to-even, clamped to [0, 255];  S8(x) = min(x, 255): every product is rounded to 8 bits on its own before the sums
 *            (OpenCV's double * Vec<uchar, 3> and Vec<uchar, 3> + Vec<uchar, 3>; restated from the published matx.hpp and saturate.hpp, not
 *            pinned by compiled OpenCV code).  Row r0 + 1 or column c0 + 1 can lie one past the image only when a or b is exactly 0, where its
 *            product is 0 whatever the pixel: the tap is read from the last row / column instead.
 *   Select:  (select_min_dis = md > 0) for candidate i in ascending order: depth = sqrt((d.x^2 + d.y^2) + d.z^2); skipped when depth > max_depth or
 *            depth < min_depth, or not projected and available.  Cell = ((int)(std::round(u / md) md), (int)(std::round(v / md) md)), std::round half
 *            away from zero.  The candidate takes the cell iff the cell is empty or (double)stored > depth, and stores (float)depth.  The holders
 *            of the cells after the last candidate are the render set, ascending.  md <= 0: the whole candidate set.
 *   PLAIN:   over the render set S: d_i = (d.x n.x + d.y n.y) + d.z n.z (vertices behind the camera included); dmin = min(3e8, min_S d_i) is
 *            reported as min_dis; allow = max(0.05, 0.1 mesh_voxel).  A vertex is skipped when d_i - dmin > allow && n_obs > 5.  Else project,
 *            sample, update_rgb(c, d_i, (1.5, 1.5, 1.5), obs_time, inv_exposure).
 *   VIEW:    dot = d_i as above, dis = depth as above; ang = acos(dot / (dis + 0.0001)) 57.3; ang = ang < 5 ? 5 : ang; dis = dis < 1 ? 1 : dis;
 *            skipped when ang > 30.  Else project, sample, sigma = (1.5 dis) ang, update_rgb(c, dis, (sigma, sigma, sigma), obs_time, inv_exposure).
 *            When it returns 1: unless max_k(rgb[k] / first_exposure) > 254 or max_k(rgb[k] / inv_exposure) > 245,
 *            pe_sum += min(| |c| - |rgb / inv_exposure| |, max_pe_error) and pe_count += 1, |x| = sqrt((x0^2 + x1^2) + x2^2).  pe_sum is summed in a
 *            fixed order (per-workgroup partials, then one pass over them): the same bytes on every run; acos is the device's, so VIEW agrees
 *            with a host evaluation to rounding (1e-12 relative), not bit for bit.  min_dis is 0.
 *   update_rgb(c, obs_dis, sigma, t, e) (pointcloud_rgbd.cpp:125-195), on the vertex state (rgb, cov, n_obs, obs_dis, last_obs_time, first_exposure):
 *            return 0 when c is (0, 0, 0), when every channel of c is > 255, or when obs_dis != 0 (the state's) && obs_dis > obs_dis(state) 1.1.
 *            n_obs == 0: last_obs_time = t, obs_dis = obs_dis, first_exposure = e, rgb[k] = c[k] e, cov[k] = sigma, n_obs = 1, return 0.
 *            Else per channel: cov = cov + 0.15 (t - last_obs_time); old = cov; cov = sqrt(1 / ((1 / cov) / cov + (1 / sigma) / sigma));
 *            rgb = (cov cov) ((rgb / old) / old + ((c e) / sigma) / sigma).  Then mx = max_k(rgb[k] / first_exposure); mx > 255: rgb[k] = (rgb[k] 254.999) / mx.
 *            obs_dis(state) = min(obs_dis(state), obs_dis); last_obs_time = t; n_obs += 1; first_exposure = (first_exposure n_obs + e) / (n_obs + 1)
 *            (n_obs after the increment); return 1.
 *   Stats:   n_set = candidates; n_selected = render set; n_hit = update_rgb calls; n_first = calls that found n_obs == 0 and initialised the vertex;
 *            n_updated = calls that returned 1 (both models).
 *   Sets:    candidates always in ascending vertex id (the reference's unordered_set order is undefined).  ALL: every vertex.  IDS: the caller's list,
 *            strictly ascending and in range.  RECENT: every vertex of every mesh voxel the last meshed scan visited (m_voxels_recent_visited with
 *            m_recent_visited_voxel_activated_time = 0, as ImMesh runs).  RECENT_HEADS: the smallest vertex id (m_pts_in_grid[0]) of each such
 *            non-empty voxel, what selection_points_for_projection starts from.
 *   Outputs: rgb_out[k] = rgb[k] / first_exposure (get_rgb), clamped to [0, 255] and truncated, in memory-channel order.  A fresh vertex is all zeros
 *            with first_exposure = 1 (RGB_pts::clear, g_initial_camera_exp_tim).
 * Threading as immesh_render_mesh: call from the thread that drives the scan loop; the call drains queued mesh jobs, reads the map and writes only the
 * colourer's own arrays.  A context with shard_mesh set returns IMMESH_E_INVAL.  Arguments are validated before any launch: finite pose, intrinsics,
 * times and gates, 0 <= fov_margin < 0.5, inv_exposure > 0, rows and cols in 2..8192, row_stride_bytes >= 3 cols, data not NULL, a known model and
 * set, select_min_dis not NaN and either <= 0 or in [1 / 1024, 1024] pixels (the cell index stays an int); else IMMESH_E_INVAL with text in immesh_last_error(ctx) and the state untouched.
 */
#ifndef IMMESH_COLOUR_H
#define IMMESH_COLOUR_H
#include "immesh_c_api.h"
#ifdef __cplusplus
extern "C" {
#endif

#define IMMESH_COLOUR_PLAIN 0          /* render_pts_in_voxels */
#define IMMESH_COLOUR_VIEW 1           /* thread_render_pts_in_voxel */
#define IMMESH_COLOUR_SET_ALL 0
#define IMMESH_COLOUR_SET_IDS 1
#define IMMESH_COLOUR_SET_RECENT 2
#define IMMESH_COLOUR_SET_RECENT_HEADS 3

typedef struct immesh_image {
    const uint8_t* data;       /* host memory, 3 interleaved 8-bit channels (CV_8UC3), channel order as stored */
    int32_t rows, cols;
    int64_t row_stride_bytes;
    double fx, fy, cx, cy;
    double rot[9], pos[3];     /* camera-to-world rotation (row-major) and camera centre: Image_frame::m_pose_w2c_q / m_pose_w2c_t (despite their names) */
    double fov_margin;         /* 0.005 */
    double inv_exposure;       /* m_image_inverse_exposure_time, 0.01 */
    double obs_time;
    double min_depth, max_depth;   /* selection only: 3 / 200 */
    double max_pe_error;       /* g_maximum_pe_error, 40 */
} immesh_image;

typedef struct immesh_colour_stats {
    int64_t n_set, n_selected, n_hit, n_first, n_updated, pe_count;
    double pe_sum, min_dis;
} immesh_colour_stats;

typedef struct immesh_colour_state {
    double rgb[3], cov[3], first_exposure, obs_dis, last_obs_time;
    int32_t n_obs, pad;
} immesh_colour_state;

/* everything zero but: identity pose, fov_margin 0.005, inv_exposure 0.01, depths 3 / 200, max_pe_error 40 */
void immesh_default_image(immesh_image* img);

/* Owns the colour state of cap_vertices vertices (76 bytes each, structure of arrays), the image staging buffers and its stream; calls on one
 * colourer must be serialised.  Destroy it before immesh_destroy(ctx). */
typedef struct immesh_colourer immesh_colourer;
immesh_colourer* immesh_colourer_create(immesh_ctx* ctx);   /* NULL on failure (immesh_last_error(ctx)) */
void immesh_colourer_destroy(immesh_colourer* c);

/* One camera frame.  ids / n_ids are read for IMMESH_COLOUR_SET_IDS only; out may be NULL. */
int immesh_colour_image(immesh_colourer* c, const immesh_image* img, int32_t model, int32_t set, const int32_t* ids, int64_t n_ids,
                        double select_min_dis, immesh_colour_stats* out);
/* The render set of the last immesh_colour_image, ascending id; uv_out (cap x 2 floats) = the raw (u, v) as floats (NaN where pc.z < 0.001; a set
 * taken without selection also holds vertices that are not available).  Both outputs may be NULL to query the count.
 * A call that fails its argument checks leaves the previous render set standing; one that fails later (memory, HIP) leaves an empty one. */
int immesh_colour_selected(immesh_colourer* c, int32_t* ids_out, float* uv_out, int64_t cap, int64_t* n_out);
/* Colours and states of n vertices: ids (any order, in range), or NULL for vertices 0 .. n - 1.  rgb_out (n x 3 bytes) and state_out may be NULL. */
int immesh_colour_fetch(immesh_colourer* c, const int32_t* ids, int64_t n, uint8_t* rgb_out, immesh_colour_state* state_out);
/* immesh_save_ply's vertices and faces plus uchar red green blue per vertex.  Vertices with n_obs < min_views are written 0 0 0 (not dropped: the
 * faces index them).  bgr = 1 takes red from channel 2 (save_to_pcd: the images are BGR). */
int immesh_save_ply_rgb(immesh_colourer* c, const char* path, double smooth_factor, int32_t knn, int32_t min_views, int32_t bgr);
/* Device time of the last immesh_colour_image, milliseconds from HIP events on the colourer's stream: [0] upload (the copies of the image and the id list from pinned staging; the host's packing into it is not included)
 * [1] select (candidate set, selection) [2] update (dmin, projection + sampling + update_rgb, statistics). */
int immesh_colourer_last_timing(immesh_colourer* c, float ms[3]);

#ifdef __cplusplus
}
#endif
#endif
