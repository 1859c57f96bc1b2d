/* immesh_raycast.h -- rays cast at the live mesh or at a triangle soup, nearest hit per ray, on the device (libimmesh_hip.so).
 *
 * Reference: README 6.1 "LiDAR pointcloud reinforcement" returns points through a pinhole depth image (include/immesh_render.h).  The reference
 * has no ray caster; this module gives the same reinforcement in the sensor's own scan pattern (an HDL-64 sweep of 360 degrees, a Livox rosette)
 * and the primitive behind line-of-sight, visibility and mesh-against-ground-truth queries: an arbitrary set of rays, the first hit of each.
 * A bounding-volume hierarchy over the faces is built on the device; the traversal prunes with a box test that cannot change the result.
 *
 * A header of its own that includes immesh_c_api.h (which does not include it): the C++ oracle mirrors immesh_c_api.h one-to-one, and the
 * caster's checker is a brute-force restatement of the contract below (tests/raycast_checker.py), not the oracle.
 *
 * ---- Contract (exact; all arithmetic in IEEE double, in the order written, no fused multiply-add) -------------------------------------------
 *   cross(p, q) and dot(p, q) exactly as in immesh_render.h:
 *   cross(p, q) = (p.y q.z - p.z q.y,  p.z q.x - p.x q.z,  p.x q.y - p.y q.x);   dot(p, q) = (p.x q.x + p.y q.y) + p.z q.z
 *   Ray:     dir, org are floats in the sensor frame, widened to double.  d_k = (rot[k][0] dir.x + rot[k][1] dir.y) + rot[k][2] dir.z.
 *            o = pos when `origins` is NULL, else o_k = ((rot[k][0] org.x + rot[k][1] org.y) + rot[k][2] org.z) + pos[k].
 *            d is not normalised: t is in units of |d|.  A ray with a float of dir or org that is not finite, with dir = (0, 0, 0), or with a
 *            component of d or o that is not finite, is a miss (not an error).
 *   Face:    a face with a vertex that is not finite is left out of the hierarchy (it never counts).  With a, b, c = (double)vertex - o:
 *            ab = cross(a, b), bc = cross(b, c), ca = cross(c, a), n = cross(b - a, c - a), na = dot(n, a)   (the renderer's Face rule).
 *   Cover:   e0 = dot(ab, d), e1 = dot(bc, d), e2 = dot(ca, d); covered when all three are >= 0 or all three are <= 0.
 *   Depth:   nd = dot(n, d); nd == 0 skips the face; s = na / nd; the fragment counts only if t_min <= s < t_max.
 *   Box:     lo_k, hi_k = the smallest and the largest of the face's three float coordinates k.  Axis k with d_k == 0, or with
 *            inv = 1.0 / d_k not finite: the face fails unless lo_k <= o_k <= hi_k, and the axis does not bound t.  Any other axis:
 *            t1 = ((double)lo_k - o_k) inv, t2 = ((double)hi_k - o_k) inv, near_k = min(t1, t2), far_k = max(t1, t2).
 *            tn = the largest near_k, tf = the smallest far_k (-inf / +inf when no axis bounds t), g = t_max 2^-24.
 *            The fragment counts only if additionally tn - g <= s <= tf + g.
 *            Geometrically this rejects nothing (a covered point lies in the face's box); it decides only what happens to grazing faces whose s
 *            is rounding noise, and it gives every enclosing box a test that can never cull a face which counts (DESIGN.md has the argument).
 *   Winner:  (IMMESH_RAY_NEAREST) d32 = (float)s + 0.0f (s = -0, an origin in the face's plane with t_min = 0, is the distance +0); the ray keeps
 *            the smallest d32, on equal d32 the smaller face index.  t_out = d32, face_out = that index; both -1 without a fragment.
 *   Any:     (IMMESH_RAY_ANY) t_out = 0 and face_out = 0 when any fragment counts, else both -1.  Which fragment was found does not show.
 *   Points:  rays in index order; a hit ray of the last NEAREST cast gives, with d = (double)d32, the point (float)(o_k + d_k d), k = 0, 1, 2.
 *   Thin:    the renderer's rule word for word: downsample_res > 0: cell = std::round(coordinate / (float)downsample_res), in float, per
 *            coordinate; the first ray of a cell in ray order keeps it.  <= 0: every hit ray.  Output in ray order.
 * The result of a cast is a function of the soup and the rays alone: not of how the hierarchy was built, of the order of atomics or of the
 * launch shape.
 * Validated before any launch: a built caster, 0 <= t_min < t_max (both finite), a finite frame, n_rays in [0, 2^31 - 2]; else IMMESH_E_INVAL with
 * text in immesh_last_error(ctx).
 */
#ifndef IMMESH_RAYCAST_H
#define IMMESH_RAYCAST_H
#include "immesh_c_api.h"
#ifdef __cplusplus
extern "C" {
#endif

#define IMMESH_RAY_NEAREST 0
#define IMMESH_RAY_ANY 1

typedef struct immesh_ray_frame {
    double rot[9];          /* sensor-to-world rotation, row-major */
    double pos[3];          /* sensor origin in the world */
} immesh_ray_frame;

/* The LiDAR frame of a pose: from the API's state layout ([0:9] R row-major, [9:12] t) and the configuration's extrinsic,
 * rot[i][j] = (R[i][0] extR[0][j] + R[i][1] extR[1][j]) + R[i][2] extR[2][j],  pos[i] = ((R[i][0] extT[0] + R[i][1] extT[1]) + R[i][2] extT[2]) + t[i].
 * Host only. */
int immesh_ray_frame_from_state(const immesh_config* cfg, const double* state, immesh_ray_frame* frame);

/* Owns its stream, events and grow-only device buffers; nothing is allocated or launched unless one is created.  Calls on one caster must be
 * serialised by the caller.  Destroy it before immesh_destroy(ctx). */
typedef struct immesh_raycaster immesh_raycaster;
immesh_raycaster* immesh_raycaster_create(immesh_ctx* ctx);   /* NULL on failure (immesh_last_error(ctx)) */
void immesh_raycaster_destroy(immesh_raycaster* rc);

/* Build the hierarchy over a triangle soup in host memory; face index = position in `faces` (n_faces x 3 vertex indices into vtx_xyz, n_vtx x 3
 * floats).  An index out of range is IMMESH_E_INVAL.  A failed build leaves the caster as it was. */
int immesh_raycast_build_triangles(immesh_raycaster* rc, const float* vtx_xyz, int64_t n_vtx, const int32_t* faces, int64_t n_faces);
/* Build it over the live mesh exactly as immesh_mesh_export(ctx, smooth_factor, knn) exports it (called first, unchanged; the export's threading
 * rule holds: call from the thread that drives the scan loop); face index = export order.  The export's arrays are COPIED into the caster's own
 * buffers: a built caster is a snapshot that stays valid, and may be cast against from another thread, while the scan loop goes on. */
int immesh_raycast_build_mesh(immesh_raycaster* rc, double smooth_factor, int32_t knn);
/* The built snapshot: vertices, faces, and the faces in the hierarchy (those without a vertex that is not finite).  Any pointer may be NULL. */
int immesh_raycast_sizes(immesh_raycaster* rc, int64_t* n_vtx, int64_t* n_faces, int64_t* n_in_tree);

/* Cast n_rays rays.  dirs: n_rays x 3 floats in the sensor frame, host memory; origins: likewise, or NULL (every ray starts at frame->pos).
 * t_out (n_rays floats) and face_out (n_rays int32) may each be NULL. */
int immesh_raycast(immesh_raycaster* rc, const immesh_ray_frame* frame, const float* dirs, const float* origins, int64_t n_rays, double t_min,
                   double t_max, int32_t mode, float* t_out, int32_t* face_out);
/* Reinforced points of the caster's last NEAREST cast, ray order, thinned by downsample_res; xyz_out (cap x 3 floats) may be NULL to query the
 * count.  cap < the count is IMMESH_E_CAPACITY. */
int immesh_raycast_points(immesh_raycaster* rc, double downsample_res, float* xyz_out, int64_t cap, int64_t* n_out);
/* Device time in milliseconds from HIP events on the caster's stream: [0] the last build (marking, sort, hierarchy, refit, and the one read-back
 * of the face count between them)  [1] the last cast (the traversal kernel)  [2] the last reinforce (points, thinning, compaction).  Copies of
 * the soup and the rays to the device and of the results back are not included. */
int immesh_raycaster_last_timing(immesh_raycaster* rc, float ms[3]);

#ifdef __cplusplus
}
#endif
#endif
