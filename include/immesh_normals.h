/* immesh_normals.h -- normals of a point cloud on the cloud index, and normal consistency between the cloud and the mesh (libimmesh_hip.so).
 *
 * Reference: none, as for the mesh-to-cloud header (the one that declares immesh_cloud_index_build and immesh_knn_cloud).  Nothing pins this module
 * but the contract below and its numpy checker (tests/normals_checker.py), whose Jacobi is pinned bit for bit to the oracle library's orc_sym3_eigen
 * and whose normals are cross-checked against numpy.linalg.eigh.
 * Accuracy, completeness, Chamfer distance and F-score (tools/mesh_eval.py) are distances; none compares surface orientation.  Normal consistency is
 * the third figure of a reconstruction evaluation: the mean |cos| between the mesh's face normal and the ground-truth normal at corresponding points.
 * A ground-truth scan has no normals, so this header makes them: per cloud point, the direction of least variance of its k nearest neighbours, in one
 * launch on the index's hierarchy that stores no neighbour list.  Then it pairs them with face normals in both directions (every cloud point with its
 * closest face; every sample of the mesh with its nearest cloud point) and reduces |cos| on the device.
 *
 * A header of its own; no other header includes it.  It works on the cloud index of the mesh-to-cloud header and reuses the statistics struct of the
 * point-to-mesh header (the one that declares immesh_closest_points), and names both by their tags only (struct immesh_cloud_index, struct
 * immesh_closest_stats: the same types, no layout of its own): the rule of either header is that no other header names it, so this one includes the
 * ray caster's header alone and cites their rules by name.  A caller includes the mesh-to-cloud header for the index, and the point-to-mesh header to
 * read the statistics, in any order.
 *
 * ---- Contract (exact; all arithmetic in IEEE double, in the order written, no fused multiply-add) -------------------------------------------
 * The Point, Cloud, D and Neighbours rules are those of the mesh-to-cloud header, unchanged; the Face, Box, D and Winner rules of a closest face are
 * those of the point-to-mesh header, unchanged.  c_i is cloud point i (three floats).
 *   Normals rule (cloud mode only; parameters k, max_dist, min_ratio, mode, viewpoint[3]):
 *     Neighbourhood: cloud point i itself, then its list L_1 .. L_count under the Neighbours rule in cloud mode with (k, max_dist): count_i points in
 *              ascending (D, index) order.  m = count_i + 1.  2 <= k <= 64.
 *     Status:  one uint8 per point: 2 the point is not finite; else 1 too few neighbours (count_i < 2); else 3 line-like (the Line gate); else 0: the
 *              point has a normal.
 *     Offsets: q_0 = 0;  q_j,a = (double)c_{L_j},a - (double)c_i,a.  Everything is centred on the point itself: a cloud far from the origin loses
 *              nothing.
 *     Mean:    S_a = 0; for j = 1 .. count: S_a = S_a + q_j,a.  g_a = S_a / (double)m.
 *     Covariance: r_j = q_j - g (j = 0 .. count; r_0,a = 0 - g_a).  For ab in xx, xy, xz, yy, yz, zz: T = r_0,a r_0,b; for j = 1 .. count:
 *              T = T + r_j,a r_j,b.  C_ab = T / (double)m.  C is symmetric by construction: C_ba is C_ab.
 *     Eigen:   the cyclic Jacobi of the library's plane fits (dev_math.hpp, sym3_eigen_jacobi), restated:
 *              A = C, V = I (V[i][j], row i, column j).  Up to 64 sweeps; a sweep visits the pairs (p, q) = (0, 1), (0, 2), (1, 2) in that order, r the
 *              third position, and each pair sees what the pairs before it left.  For a pair:
 *                A_pq == 0: nothing happens.
 *                else if |A_pq| <= 1e-300, or (|A_pp| + |A_pq| == |A_pp| and |A_qq| + |A_pq| == |A_qq|): A_pq = 0 and nothing else changes.
 *                else (a rotation): theta = (A_qq - A_pp) / (2 A_pq);  t = (theta >= 0 ? 1 : -1) / (|theta| + sqrt(theta theta + 1));
 *                  c = 1 / sqrt(t t + 1);  s = t c.  With the old values on the right:  A_pp = A_pp - t A_pq;  A_qq = A_qq + t A_pq;
 *                  A_rp = c A_rp - s A_rq;  A_rq = s A_rp + c A_rq;  A_pq = 0;  for i = 0, 1, 2: V[i][p] = c V[i][p] - s V[i][q],
 *                  V[i][q] = s V[i][p] + c V[i][q].
 *              A sweep without a rotation ends the loop.  lambda_d = A_dd, d = 0, 1, 2: the eigenvalue at diagonal position d; column d of V is its
 *              vector.
 *              s = the position of the smallest lambda, the lowest position on ties.  hi = among the other two the position of the larger lambda,
 *              the lower position on ties.  mid = the remaining position.
 *     Line gate: status 3 when !(lambda_mid > min_ratio lambda_hi).  0 <= min_ratio < 1, finite.  At min_ratio = 0 only a neighbourhood with
 *              lambda_mid <= 0 (collinear or coincident points) is refused.
 *     Normal:  u_a = V[a][s].  Canonical sign: the component with the largest |u_a| (the lowest a on ties) is made positive by negating all three
 *              when it is negative.  mode == IMMESH_NORMALS_VIEWPOINT: w_a = viewpoint_a - (double)c_i,a, t = (u_x w_x + u_y w_y) + u_z w_z; u is
 *              negated when t < 0; on t == 0 the canonical sign stays.  len = sqrt((u_x u_x + u_y u_y) + u_z u_z);  normal_out_a = (float)(u_a / len).
 *     Outputs: eig_out three doubles lambda_s, lambda_mid, lambda_hi;  curvature_out one double: lambda_s / ((lambda_0 + lambda_1) + lambda_2) when
 *              that sum is > 0, else 0 (the surface variation);  count_out = count_i (int32);  status_out.
 *              Status 1 and 2: the normal is three quiet NaNs (0x7FC00000), eig = -1, -1, -1, curvature = -1.  Status 3: the normal is three quiet
 *              NaNs; eig and curvature are given.
 *              counts (four int64): [0] with a normal  [1] too few neighbours  [2] line-like  [3] not finite; they sum to the cloud's size.
 *     The normals and statuses stay on the device in buffers of their own, for the Agreement rule and immesh_cloud_normals_get.  A build and an
 *     apply of the index drop them.  The call leaves the index's query results, neighbour results and outlier masks as they were.
 *   Agreement rule (a face normal against a point normal):
 *     Face:    A, B, C the face's vertices widened to double; ab = B - A, ac = C - A, cr = cross(ab, ac) as in immesh_raycast.h; l2 = dot(cr, cr).
 *              A face takes part when it is in the hierarchy (its indices in range, nine finite coordinates) and l2 is finite and > 0.
 *     Value:   n = the stored float normal widened.  s = dot(cr, n) / sqrt(l2);  agree_out = (float)s.  A pair is opposed when s < 0.
 *     Pairs, samples direction: sample j of the caster's last samples pairs its face with cloud point index_out[j] of the index's last
 *              immesh_nearest_samples query when index_out[j] >= 0, that cloud point has status 0 and the face takes part.
 *     Pairs, cloud direction: cloud point i, read where it lies on the device (no frame), pairs with its closest face within max_dist when it has
 *              status 0, such a face exists and that face takes part.  face_out[i] = the closest face of a point with status 0, -1 when there is
 *              none within max_dist, and -1 for every point without status 0 (it is not walked).
 *     Without a pair agree_out is a quiet NaN (0x7FC00000).
 *     counts (four int64): [0] pairs  [1] opposed pairs (they are among [0])  [2] no pair  [3] the cloud point is not finite (status 2; always 0
 *              in the samples direction).  [0] + [2] + [3] is the number of cloud points, or of samples.
 *     Reduce:  the Stats rule of the point-to-mesh header over the index's last agreement of either direction with dist = fabsf(agree_out) of the
 *              pairs.  struct immesh_closest_stats is reused as it is: n_with_face reads "pairs", n_no_face "no pair", n_not_finite as counts[3].
 *              mean is the normal consistency of that direction.
 * Every result is a function of the cloud, the soup, the samples and the parameters alone: not of how a hierarchy was built, of the order in which
 * lanes or nodes are visited, or of the launch shape.
 * Validated before any launch: a built index; 2 <= k <= 64; 0 < max_dist finite; 0 <= min_ratio < 1; a known mode; a finite viewpoint in viewpoint
 * mode; normals made since the index's last build or apply (get, agreement); a built caster of the index's context (agreement); an
 * immesh_nearest_samples query of this caster made since its last sampling (samples direction); an agreement since the last normals before its
 * reduce; 0 < bin_width finite, 1 <= n_bins <= 2^20; else IMMESH_E_INVAL with text in immesh_last_error(ctx), and the index stays as it was.
 * An empty index (every count is 0) and a caster without faces (no pair) are no errors.
 */
#ifndef IMMESH_NORMALS_H
#define IMMESH_NORMALS_H
#include "immesh_raycast.h"
#ifdef __cplusplus
extern "C" {
#endif

struct immesh_cloud_index;     /* the cloud index of the mesh-to-cloud header (its typedef immesh_cloud_index names the same type) */
struct immesh_closest_stats;   /* defined by the point-to-mesh header; n_with_face reads "pairs" here */

#define IMMESH_NORMALS_CANONICAL 0   /* the canonical sign alone */
#define IMMESH_NORMALS_VIEWPOINT 1   /* towards viewpoint[3] (read in this mode only; may be NULL otherwise) */

/* The Normals rule for every point of the index's cloud.  The outputs are sized by the cloud (immesh_cloud_index_sizes, points given): normal_out
 * n x 3 floats, curvature_out n doubles, eig_out n x 3 doubles, count_out n int32, status_out n uint8, counts four int64; each may be NULL.  Nothing
 * is allocated or launched for normals before the first call. */
int immesh_cloud_normals(struct immesh_cloud_index* ix, int32_t k, double max_dist, double min_ratio, int32_t mode, const double* viewpoint, float* normal_out,
                         double* curvature_out, double* eig_out, int32_t* count_out, uint8_t* status_out, int64_t counts[4]);
/* The normals and statuses as they lie on the device.  n_out (may be NULL) receives the cloud's size; cap below it with an output given is
 * IMMESH_E_CAPACITY. */
int immesh_cloud_normals_get(struct immesh_cloud_index* ix, float* normal_out, uint8_t* status_out, int64_t cap, int64_t* n_out);
/* The Agreement rule, samples direction: agree_out one float per sample of the caster's last samples (immesh_mesh_sample_count).  The index's stream
 * waits on the event the caster records after sampling.  Both objects belong to one context; the caller serialises calls on both. */
int immesh_normals_agree_samples(struct immesh_cloud_index* ix, immesh_raycaster* rc, float* agree_out, int64_t counts[4]);
/* The Agreement rule, cloud direction: agree_out one float and face_out one int32 per cloud point. */
int immesh_normals_agree_cloud(struct immesh_cloud_index* ix, immesh_raycaster* rc, double max_dist, float* agree_out, int32_t* face_out, int64_t counts[4]);
/* The index's last agreement of either direction reduced on the device.  stats and hist_out (n_bins int64 counts) may each be NULL. */
int immesh_normals_agree_reduce(struct immesh_cloud_index* ix, double bin_width, int32_t n_bins, struct immesh_closest_stats* stats, int64_t* hist_out);
/* Device time in milliseconds from HIP events on the index's stream: [0] the last normals launch  [1] the last agreement launch  [2] the last
 * reduction.  Copies are not included. */
int immesh_normals_last_timing(struct immesh_cloud_index* ix, float ms[3]);

#ifdef __cplusplus
}
#endif
#endif
