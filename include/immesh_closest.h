/* immesh_closest.h -- point-to-mesh distances on the device: the closest face of every point, on a built ray caster (libimmesh_hip.so).
 *
 * Reference: none.  The reference reports cloud-to-mesh error in its paper but ships no code for it; nothing pins this module but the contract
 * below and its two checkers (tests/closest_checker.py by brute force, and the sampled cross-check in tests/test_closest_cpu.py).
 * It answers "how far is this point from the mesh": the accuracy of a reconstruction against a ground-truth scan, the distance of the current scan
 * to the surface built so far, clearance for a planner.  It works on an immesh_raycaster built by either build call of immesh_raycast.h: the
 * snapshot, its vertex and face buffers and its hierarchy serve rays and distance queries alike.  The traversal prunes with a box bound that
 * cannot change the result.
 *
 * A header of its own that includes immesh_raycast.h (which does not include it).
 *
 * ---- Contract (exact; all arithmetic in IEEE double, in the order written, no fused multiply-add) -------------------------------------------
 *   dot(p, q) and cross(p, q) exactly as in immesh_raycast.h.  unit(x) = x when 0 < x < 1, 1 when x >= 1, 0 otherwise (also for NaN).
 *   Point:   pts are floats, widened to double: x.  frame == NULL: p = x.  Else p_k = ((rot[k][0] x.x + rot[k][1] x.y) + rot[k][2] x.z) + pos[k].
 *            A point with a float that is not finite, or with a p_k that is not finite or not below 2^128 in magnitude (the range of the float
 *            coordinates the soup lives in; it keeps every product below finite), has no face and is counted as not finite.
 *   Face:    a face with a vertex that is not finite is not in the hierarchy (it never counts).  a, b, c = (double)vertex - p.
 *            ab = b - a, ac = c - a;  d1 = dot(ab, -a), d2 = dot(ac, -a), d3 = dot(ab, -b), d4 = dot(ac, -b), d5 = dot(ab, -c), d6 = dot(ac, -c);
 *            vc = d1 d4 - d3 d2, vb = d5 d2 - d1 d6, va = d3 d6 - d5 d4.  q, the closest point relative to p, by the first test that holds:
 *              1  d1 <= 0 and d2 <= 0:                                            q = a
 *              2  d3 >= 0 and d4 <= d3:                                           q = b
 *              3  vc <= 0, d1 >= 0, d3 <= 0 and d1 - d3 != 0:                     v = unit(d1 / (d1 - d3)),  q_k = a_k + v ab_k
 *              4  d6 >= 0 and d5 <= d6:                                           q = c
 *              5  vb <= 0, d2 >= 0, d6 <= 0 and d2 - d6 != 0:                     w = unit(d2 / (d2 - d6)),  q_k = a_k + w ac_k
 *              6  va <= 0, e = d4 - d3 >= 0, g = d5 - d6 >= 0 and e + g != 0:     w = unit(e / (e + g)),     q_k = b_k + w (c_k - b_k)
 *              7  otherwise: s = (va + vb) + vc, i = 1 / s (0 when s == 0), v = unit(vb i), w = min(unit(vc i), 1 - v),
 *                 q_k = (a_k + ab_k v) + ac_k w
 *            An edge test whose denominator is zero does not hold, and a zero s gives q = a: no quotient has a zero denominator, every weight
 *            lies in [0, 1] (v + w <= 1 in 7), and every face with finite vertices gets a finite q that is a point of the face.  For a face of zero
 *            area (a == b, collinear vertices, a == b == c) q is a point of the face and d2 an upper bound of its distance.
 *            d2 = dot(q, q).
 *   Box:     for a float box (lo, hi): e_k = max(max((double)lo_k - p_k, p_k - (double)hi_k), 0), L = (e_x e_x + e_y e_y) + e_z e_z.
 *            Rounding is monotone, so a box that contains another per coordinate has an L that is not larger, exactly.
 *   D:       D = max(d2, L(the face's own float box: the smallest and the largest of its three float coordinates k)).  Geometrically the max
 *            changes nothing (the closest point lies in the box); it makes D >= L(every enclosing box) hold exactly, which is what lets the
 *            traversal skip a node whose L exceeds the best D so far without ever skipping a face that wins or ties.
 *            A face counts only if D <= r2, r2 = max_dist max_dist.
 *   Winner:  the smallest D; on equal D the smaller face index (a point nearest to a shared vertex gets the same q from every face around it).
 *   Outputs: d2_out = D;  dist_out = (float)sqrt(D), the double square root correctly rounded;  face_out = the index;
 *            xyz_out_k = (float)(p_k + q_k) with the winner's q;  side_out = the sign (+1, 0, -1) of dot(cross(ab, ac), -a) of the winner: the side
 *            of its plane by the snapshot's vertex order, 0 in the plane and for a face whose cross(ab, ac) is zero.
 *            Without a face: d2_out = -1, dist_out = -1, face_out = -1, xyz_out = three quiet NaNs (0x7FC00000), side_out = 0.
 *   Stats:   over the caster's last query, dist = dist_out of the points with a face.  max_dist = the largest dist (0 without one);
 *            sum_dist = the sum of (double)dist, sum_dist2 = the sum of (double)dist (double)dist (each term exact), both in a fixed order of
 *            additions that depends on n_pts alone (two calls give the same bits; the order itself is not part of the contract: each sum is
 *            within n 2^-53 relative of the exact sum);  mean = sum_dist / n_with_face, rms = sqrt(sum_dist2 / n_with_face), 0 without a face.
 *            Histogram, in float: b = dist / (float)bin_width; a point with b < n_bins adds one to bin (int)b, any other to n_overflow.
 * The result of a query is a function of the soup and the points alone: not of how the hierarchy was built, of the order in which lanes or
 * nodes are visited, or of the launch shape.
 * Validated before any launch: a built caster, 0 < max_dist finite, a finite frame when one is given, n_pts in [0, 2^31 - 2];
 * 0 < bin_width finite, 1 <= n_bins <= 2^20, a query before the statistics; else IMMESH_E_INVAL with text in immesh_last_error(ctx).
 * A caster with no face in its hierarchy answers "no face" for every point; that is not an error.
 */
#ifndef IMMESH_CLOSEST_H
#define IMMESH_CLOSEST_H
#include "immesh_raycast.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct immesh_closest_stats {
    int64_t n_points;        /* points of the last query */
    int64_t n_with_face;
    int64_t n_not_finite;    /* the Point rule */
    int64_t n_no_face;       /* finite, but no face within max_dist */
    int64_t n_overflow;      /* points with a face beyond the histogram's last bin */
    double sum_dist, sum_dist2;
    double mean, rms;
    float max_dist;
    float bin_width;         /* the histogram's bin width as used: (float)bin_width */
} immesh_closest_stats;

/* The closest face of n_pts points (n_pts x 3 floats, host memory): world coordinates when frame is NULL, else sensor coordinates transformed as
 * ray origins are.  Every output may be NULL: d2_out n_pts doubles, dist_out n_pts floats, face_out n_pts int32, xyz_out n_pts x 3 floats,
 * side_out n_pts int8.  Nothing is allocated or launched for these queries before the first one; the buffers are grow-only, as the caster's. */
int immesh_closest_points(immesh_raycaster* rc, const immesh_ray_frame* frame, const float* pts, int64_t n_pts, double max_dist, double* d2_out,
                          float* dist_out, int32_t* face_out, float* xyz_out, int8_t* side_out);
/* The caster's last query reduced on the device.  stats and hist_out (n_bins int64 counts) may each be NULL. */
int immesh_closest_reduce(immesh_raycaster* rc, double bin_width, int32_t n_bins, immesh_closest_stats* stats, int64_t* hist_out);
/* Device time in milliseconds from HIP events on the caster's stream: [0] the last query (the traversal kernel)  [1] the last reduction.  Copies of
 * the points to the device and of the results back are not included. */
int immesh_closest_last_timing(immesh_raycaster* rc, float ms[2]);

#ifdef __cplusplus
}
#endif
#endif
