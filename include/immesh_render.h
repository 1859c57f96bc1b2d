/* immesh_render.h -- mesh depth images on the device for LiDAR point reinforcement (libimmesh_hip.so).
 *
 * Reference: README 6.1 "LiDAR pointcloud reinforcement".  The GUI thread rasterizes the live mesh from the current LiDAR pose through the
 * OpenGL depth buffer and turns every valid pixel back into a 3-D point:
 *   src/ImMesh_node.cpp:169-206                          get_last_avr_pose: the camera pose from the LiDAR pose
 *   src/ImMesh_node.cpp:305-329                          render, read back, draw
 *   src/tools/openGL_libs/openGL_camera_view.cpp:316-415 depth conversion + unprojection (Cam_view::unproject_point at :397-404)
 *   src/tools/openGL_libs/openGL_camera.hpp:254-285      get_truth_depth, downsample_pts_result
 * Here the live mesh stays in HBM and a HIP rasterizer replaces the GL pass.
 *
 * These declarations are part of the C ABI of immesh_c_api.h (which includes this file).  They live in a header of their own because the
 * C++ oracle mirrors immesh_c_api.h's per-scan entry points one-to-one; the renderer's checker is a restatement of the contract below
 * (tests/render_checker.py), not the oracle.
 *
 * ---- Contract (exact; all arithmetic in IEEE double, in the order written, no fused multiply-add) -------------------------------------------
 *   cross(p, q) = (p.y q.z - p.z q.y,  p.z q.x - p.x q.z,  p.x q.y - p.y q.x);   dot(p, q) = (p.x q.x + p.y q.y) + p.z q.z
 *   cx = width / 2, cy = height / 2 (integer division, as Cam_view::set_gl_projection), f = focus.
 *   Vertex:  a = rot^T ((double)p - pos), component k = (rot[0][k] d.x + rot[1][k] d.y) + rot[2][k] d.z.  A face with a vertex that is not
 *            finite is skipped (exported isolated vertices can be NaN); an index out of range is IMMESH_E_INVAL (triangle soup).
 *   Face:    ab = cross(a, b), bc = cross(b, c), ca = cross(c, a), n = cross(b - a, c - a), na = dot(n, a); vertex depths -a.z, -b.z, -c.z.
 *            Culled when every vertex depth is < z_near or every one is >= z_far.
 *   Bounds:  the face's candidate pixels are a box.  Its corners come from the face clipped to depth >= z_near: every vertex of depth
 *            d >= z_near, and for each edge (p, q) of (a, b), (b, c), (c, a) with exactly one end nearer than z_near the point p + t (q - p),
 *            t = (z_near - d_p) / (d_q - d_p), x and y only, at depth d = z_near.  Each corner projects to U = cx + (x / d) f, V = cy - (y / d) f.
 *            With Umin, Umax clamped to [-4, width + 4]: columns max(0, floor(Umin) - 1) .. min(width - 1, ceil(Umax) + 1), rows likewise; an
 *            empty box culls the face.  The box holds every pixel the face covers; it only decides where rounding noise alone passes an edge
 *            test (an edge that points at the camera centre).
 *   Ray:     pixel (u, v) (column, row; row 0 at the top; integers, no half-pixel offset): dir = ((u - cx) / f, -((v - cy) / f), -1), the ray
 *            Cam_view::unproject_point uses, so a reinforced point lies on the mesh.  The reference samples GL at (u + 0.5, h - v - 0.5), unprojects
 *            at (u, v) and clamps row 0 to row 1, and quantises depth through a 16/24-bit buffer; none of that is reproduced.
 *   Cover:   e0 = dot(ab, dir), e1 = dot(bc, dir), e2 = dot(ca, dir); covered when all three are >= 0 or all three are <= 0 (edges and vertices
 *            inclusive, no face culling).
 *   Depth:   nd = dot(n, dir); nd == 0 skips; s = na / nd; the fragment counts only if z_near <= s < z_far (this replaces near / far clipping).
 *   Winner:  d32 = (float)s; the pixel keeps the smallest d32, on equal d32 the smaller face index.
 *   Output:  depth = d32 where (double)d32 < 0.99 z_far (convert_depth_buffer_to_truth_depth), else -1; face = the winner's index, -1 where
 *            depth is -1.  depth_out / face_out are height x width, row-major, row 0 at the top; either may be NULL.
 *   Points:  pixels in i = v width + u order; a valid pixel gives, with d = (double)d32, x = ((u - cx) / f) d, y = -((v - cy) / f) d, z = -d,
 *            the world point (float)(((rot[r][0] x + rot[r][1] y) + rot[r][2] z) + pos[r]).
 *   Thin:    downsample_res > 0: cell = std::round(coordinate / (float)downsample_res), in float, per coordinate (downsample_pts_result); the first
 *            pixel of a cell in pixel order keeps it.  <= 0: every valid pixel.  Output in pixel order.
 * Arguments are validated before any launch: 0 < width, height <= 8192, focus > 0, 0 < z_near < z_far (all finite), finite pose; else IMMESH_E_INVAL
 * with text in immesh_last_error(ctx).  More than 2^31 - 1 (face, 16x16 tile) pairs in one render is IMMESH_E_CAPACITY.
 */
#ifndef IMMESH_RENDER_H
#define IMMESH_RENDER_H
#include "immesh_c_api.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct immesh_camera {
    double rot[9];          /* camera-to-world rotation, row-major, GL convention: looks along its -z, +y up (Cam_view::m_camera_rot) */
    double pos[3];          /* camera centre in the world (Cam_view::m_camera_pos) */
    int32_t width, height;  /* pixels; principal point (width / 2, height / 2) in integer division (Cam_view::set_gl_projection) */
    double focus;           /* fx = fy in pixels (the depth view: 400) */
    double z_near, z_far;   /* Cam_view defaults 0.05 / 200 */
    double downsample_res;  /* reinforced-point cell in metres (m_depth_downsample_resolution = 0.01); <= 0: keep every pixel */
} immesh_camera;

/* 640 x 480, focus 400, z 0.05 / 200, cell 0.01, identity pose (the GUI's depth view, openGL_camera.hpp:216 and ImMesh_node.cpp:305-329) */
void immesh_default_depth_camera(immesh_camera* cam);
/* get_last_avr_pose (ImMesh_node.cpp:169-206) with its window of one frame: rot = R M, M = [[0,0,-1],[-1,0,0],[0,1,0]]
 * (lidar_frame_to_camera_frame, :174), pos = t, from the API's state layout ([0:9] R row-major, [9:12] t).  Sets the pose only.  Host only. */
int immesh_camera_from_state(const double* state, immesh_camera* cam);

/* Owns its device buffers and its stream; calls on one renderer must be serialised.  Destroy it before immesh_destroy(ctx). */
typedef struct immesh_renderer immesh_renderer;
immesh_renderer* immesh_renderer_create(immesh_ctx* ctx);   /* NULL on failure (immesh_last_error(ctx)) */
void immesh_renderer_destroy(immesh_renderer* r);

/* Any triangle soup in host memory; face index = position in `faces` (n_faces x 3 vertex indices into vtx_xyz, n_vtx x 3 floats). */
int immesh_render_triangles(immesh_renderer* r, const immesh_camera* cam, const float* vtx_xyz, int64_t n_vtx, const int32_t* faces, int64_t n_faces,
                            float* depth_out, int32_t* face_out);
/* The live mesh exactly as immesh_mesh_export(ctx, smooth_factor, knn) exports it (called first, unchanged; its arrays are rasterized where they lie
 * in HBM); face index = export order.  The export's threading rule holds: call from the thread that drives the scan loop.  Drains queued mesh
 * jobs; the map is not modified. */
int immesh_render_mesh(immesh_renderer* r, const immesh_camera* cam, double smooth_factor, int32_t knn, float* depth_out, int32_t* face_out);
/* Reinforced points of the renderer's last render, pixel order; xyz_out (cap x 3 floats) may be NULL to query the count. */
int immesh_render_points(immesh_renderer* r, float* xyz_out, int64_t cap, int64_t* n_out);
/* Device time of the last render, milliseconds from HIP events on the renderer's stream: [0] rasterize (setup, binning, per-tile resolve)
 * [1] reinforce (unproject, thinning, compaction).  Host-to-device copies of a soup and the read-back of the outputs are not included. */
int immesh_renderer_last_timing(immesh_renderer* r, float ms[2]);

#ifdef __cplusplus
}
#endif
#endif
