/* immesh_nearest.h -- mesh-to-cloud distances on the device: a deterministic sampler of a built ray caster's snapshot, an index over a point cloud,
 * and the nearest cloud point of every query point (libimmesh_hip.so).
 *
 * Reference: none, as for immesh_raycast.h and the point-to-mesh distances (immesh_closest_points).  Nothing pins this module but the contract
 * below, its brute-force checker (tests/nearest_checker.py) and a bit-for-bit cross-check against immesh_closest_points on the cloud as a soup of
 * degenerate faces (i, i, i).
 * immesh_closest_points answers "how far are the ground-truth points from the mesh" (accuracy).  This header answers the other half, "how far are
 * points of the mesh from the nearest ground-truth point" (completeness): sample the snapshot, index the ground-truth cloud, query the samples where
 * they lie, on the device.  Chamfer distance and F-score need both directions (tools/mesh_eval.py).
 *
 * A header of its own; no other header includes it.  It includes immesh_raycast.h and names the result struct of the point-to-mesh header by its
 * tag only (struct immesh_closest_stats: the same struct, no layout of its own), because that header's rule is that no other header names it;
 * a caller that reads the statistics includes both headers, in either order.
 *
 * ---- Contract (exact; all arithmetic in IEEE double, in the order written, no fused multiply-add) -------------------------------------------
 *   Point:   (queries) pts are floats, widened to double: x.  frame == NULL: p = x.  Else p_k = ((rot[k][0] x.x + rot[k][1] x.y) + rot[k][2] x.z) + pos[k].
 *            A point with a float that is not finite, or with a p_k that is not finite or not below 2^128 in magnitude (the range of the float
 *            coordinates the cloud lives in; it keeps every product below finite), has no neighbour and is counted as not finite.
 *   Cloud:   a cloud point with a float that is not finite is not in the index (it never counts).  The index of a point is its position in the array.
 *   D:       for a cloud point c: e_k = (double)c_k - p_k, D = (e_x e_x + e_y e_y) + e_z e_z.  A point counts only if D <= r2, r2 = max_dist max_dist.
 *   Winner:  the smallest D; on equal D the smaller point index.
 *   Outputs: d2_out = D;  dist_out = (float)sqrt(D), the double square root correctly rounded;  index_out = the winner's index;
 *            xyz_out = the winner's three floats, copied.
 *            Without a neighbour: d2_out = -1, dist_out = -1, index_out = -1, xyz_out = three quiet NaNs (0x7FC00000).
 *   Box:     the Box rule of the point-to-mesh contract: for a float box (lo, hi), e_k = max(max((double)lo_k - p_k, p_k - (double)hi_k), 0),
 *            L = (e_x e_x + e_y e_y) + e_z e_z; a box that contains another per coordinate has an L that is not larger, exactly.  For a cloud
 *            point's own box (lo == hi == c), L is D bit for bit: max(c_k - p_k, p_k - c_k) is |c_k - p_k| (the two differences are each other's
 *            negation, exactly) and its square is the same product.  So D >= L(every enclosing box) holds exactly, and the traversal may skip a node
 *            whose L exceeds r2 or the best D so far (strictly) without ever skipping a point that wins or ties.
 *   Samples: G = 0x9E3779B97F4A7C15; integers are 64-bit, arithmetic mod 2^64.
 *            mix(z): z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31.   U(h) = (double)(h >> 11) * 2^-53.
 *            Face f of the snapshot, A, B, C its vertices widened to double: ab = B - A, ac = C - A, n = cross(ab, ac) (as in immesh_raycast.h),
 *            x = (0.5 * sqrt(dot(n, n))) * density.  A face that is not in the hierarchy (an index out of range, a vertex that is not finite) has
 *            k_f = 0.  Else, x not finite or x >= 2^31: k_f = 2^31.  Else h_f = mix(seed + G (f + 1)), k_f = floor(x) + (U(h_f) < x - floor(x)).
 *            The total is the int64 sum of k_f; above 2^31 - 2 it is IMMESH_E_CAPACITY ("too many samples"), an error and not a fault.
 *            Sample j of face f (0 <= j < k_f) sits at position (the sum of k over the faces before f) + j:
 *              u = U(mix(h_f + G (2j + 1))), v = U(mix(h_f + G (2j + 2)));  if u + v > 1: u = 1 - u, v = 1 - v (both exact);
 *              xyz_k = (float)((A_k + ab_k u) + ac_k v);  face_out = f.
 *            Counts and offsets are integers: the order of the samples is a function of the soup, the density and the seed.  The expected count
 *            of a face is its area times the density, so plain, unweighted statistics over the samples are area-weighted.
 *   Stats:   the Stats rule of the point-to-mesh contract over the index's last query of either kind, dist = dist_out of the points with a neighbour.
 *            struct immesh_closest_stats is reused as it is: n_with_face reads "with a neighbour", n_no_face "finite, but no neighbour within max_dist".
 * The result of a query is a function of the cloud and the points alone: not of how the hierarchy was built, of the order in which lanes or nodes are
 * visited, or of the launch shape.
 * Validated before any launch: a built index (queries), a built caster (sampler, _samples); 0 < max_dist finite; 0 < density finite; a finite frame
 * when one is given; n and n_pts in [0, 2^31 - 2], the build at most 2^30 points; samples made since the caster's last build before a _samples query;
 * the caster and the index of one context; 0 < bin_width finite, 1 <= n_bins <= 2^20, a query before the reduction; else IMMESH_E_INVAL with text in
 * immesh_last_error(ctx).  An empty index (no point, or none that is finite) answers "no neighbour" for every query, and a caster with no face
 * gives zero samples; neither is an error.
 *
 * ---- The Neighbours rule, the Count rule, the Outliers rule (the same arithmetic; the Point, Cloud, D and Box rules above stay as they stand) ------
 *   Candidates: for a query p, the cloud points in the index with D <= r2 (r2 = max_dist max_dist, or radius radius).  In cloud mode the query is
 *            cloud point i itself, read where it lies on the device (its floats widened, no frame), and the point with index i is no candidate;
 *            another point with equal coordinates is one, at D = 0.  A cloud point that is not finite is a query "not finite" without candidates.
 *   Neighbours: 1 <= k <= 64.  The result is the first min(k, #candidates) candidates in ascending (D, index) order, in that order.
 *            count_out[i] (int32) their number; index_out[i k + j] (int32) and d2_out[i k + j] (double) the j-th; slots j >= count hold -1 and -1.0.
 *            Cloud mode: mean_out[i] = (the sum over j, in list order, of sqrt(d2_j)) / (double)count, a sequential sum of correctly rounded double
 *            square roots; -1.0 when count == 0.  Every output may be NULL; with both lists NULL the n x k lists are not stored on the device at all.
 *   Count:   count_out[i] (int32) = the number of candidates.
 *   Outliers, statistical (over the index's last cloud-mode Neighbours query): used = the cloud points with count > 0, n_used their number;
 *            mu = (the sequential double sum of mean_i over used, ascending i) / (double)n_used;
 *            sigma = sqrt((the sequential sum of (mean_i - mu) (mean_i - mu) over used, ascending i) / (double)(n_used - 1)), 0 when n_used <= 1;
 *            threshold = mu + mult sigma;  keep_i = used_i && mean_i <= threshold.  mu and sigma are host code over the mean array read back once;
 *            the mask is made on the device from the threshold.  n_used == 0: mu = sigma = threshold = 0, nothing is kept, and that is no error.
 *            counts: [0] kept  [1] statistical outliers (used, above the threshold)  [2] isolated (finite, count == 0)  [3] not finite; they sum to
 *            the cloud's size.
 *   Outliers, radius (over the index's last cloud-mode Count query): keep_i = finite_i && count_i >= min_neighbours, min_neighbours >= 0.
 *            counts: [0] kept  [1] finite and not kept  [2] isolated (finite, count == 0: kept when min_neighbours == 0, else among [1])
 *            [3] not finite; [0] + [1] + [3] is the cloud's size.
 *            keep_out (either rule) is one uint8 per cloud point, 1 for a kept point.
 *   Apply:   the kept points of the index's last mask, in ascending old index, become the index's cloud (a scan of the mask, a compaction and the
 *            build, all on the device).  kept_index_out receives the old index of every new point: cap < their number with kept_index_out given is
 *            IMMESH_E_CAPACITY, and the index stays as it was.  Earlier query results and masks of the index are dropped: a reduction afterwards is
 *            IMMESH_E_INVAL, and so is an Outliers call before a new cloud-mode query.  An index left empty answers "no neighbour" and is no error.
 * These results, too, are functions of the cloud, the queries and the parameters alone.
 * Validated before any launch: a built index; 1 <= k <= 64; 0 < max_dist and 0 < radius, finite; mult finite and >= 0; min_neighbours in
 * [0, 2^31 - 2]; the matching cloud-mode query made since the last build or apply before an Outliers call; a mask before the apply; the point array
 * and the frame as above; else IMMESH_E_INVAL with text, and the index stays as it was.
 *
 * ---- The Clusters rule (Euclidean cluster extraction, DBSCAN; the same arithmetic; exact and free of any order, like everything above) ---------------
 *   Candidates: as in the Count rule in cloud mode, r2 = radius radius: for cloud point i the other points in the index with D <= r2.  D between two
 *            cloud points is symmetric bit for bit: (double)c_j - (double)c_i is the exact negation of (double)c_i - (double)c_j, and the squares
 *            and their sums are the same products in the same order.  So "j is a candidate of i" is a symmetric relation.
 *            count_i = the number of candidates of i.
 *   Kind:    (uint8)  3 not finite;  0 core: finite and count_i >= min_neighbours, min_neighbours >= 0;  1 border: finite, not core, and at least one
 *            candidate is core;  2 noise: finite, not core, and no candidate is core.  With min_neighbours == 0 every finite point is core: that is
 *            plain Euclidean cluster extraction, and nothing is counted at all.
 *   Cluster: two core points are joined when each is the other's candidate.  The clusters are the classes of the transitive closure of that relation
 *            over the core points, and over them only: a border point joins nothing, and two clusters that both reach one stay two.
 *            A cluster's label is its smallest core index; the clusters are numbered 0 .. n_clusters - 1 by ascending label.
 *   Border:  a border point gets the cluster of its core candidate that is smallest under (D, index).
 *   Outputs: label_out[i] (int32) the cluster's number, -1 for noise and for a point that is not finite;  kind_out[i] the kind;
 *            counts: [0] core  [1] border  [2] noise  [3] not finite; they sum to the cloud's size;  n_clusters the number of clusters.
 *   Table:   per cluster, by number: first = the label;  n_points = core plus border;  n_core;  box = lo xyz, hi xyz over the floats of all its
 *            members, compared as values (the sign of a zero is not part of the contract, as in the topology's table).
 *   Select:  (after the Select rule of the mesh topology's header)  a cluster is kept when n_points >= min_points, and max_points == 0 || n_points <=
 *            max_points, and keep_largest == 0 or it is among the keep_largest clusters with the most points, counted over ALL clusters, ties to
 *            the smaller number.  keep_i = point i is in a kept cluster, or (keep_noise != 0 and its kind is noise).
 *            counts: [0] kept  [1] in a cluster and not kept  [2] noise and not kept  [3] not finite; they sum to the cloud's size.
 *            The mask becomes the index's last mask: immesh_cloud_index_apply_outliers applies it as it applies the Outliers rules'.
 * Validated before any launch: a built index; 0 < radius, finite; min_neighbours, min_points, max_points and keep_largest in [0, 2^31 - 2]; a
 * Clusters call since the last build or apply before a table or a select; cap as in the other fetches; else IMMESH_E_INVAL with text (cap below the
 * count with an output given: IMMESH_E_CAPACITY), and the index stays as it was.  An empty index gives zero clusters and is no error.
 * IMMESH_E_INTERNAL (as in the mesh topology's header): a union did not finish within its proven bound of steps (a defect of the library, never of the
 * input); the clusters are void.
 */
#ifndef IMMESH_NEAREST_H
#define IMMESH_NEAREST_H
#include "immesh_raycast.h"
#ifdef __cplusplus
extern "C" {
#endif

/* An index over a point cloud: a stream, events and grow-only device buffers of its own, like the caster.  Nothing is allocated or launched unless
 * one is created.  Destroy it before its context.  Calls on one index are serialised by the caller. */
typedef struct immesh_cloud_index immesh_cloud_index;
struct immesh_closest_stats;   /* defined by the point-to-mesh header; n_with_face reads "with a neighbour" here */
immesh_cloud_index* immesh_cloud_index_create(immesh_ctx* ctx);   /* NULL on failure (immesh_last_error(ctx)) */
void immesh_cloud_index_destroy(immesh_cloud_index* ix);

/* Copies n_pts x 3 floats (host memory) to the device and builds the hierarchy over the finite ones, one point per leaf.  A refused build leaves
 * the index as it was. */
int immesh_cloud_index_build(immesh_cloud_index* ix, const float* xyz, int64_t n_pts);
/* Sizes of the built index (each pointer may be NULL): points given, points in the hierarchy. */
int immesh_cloud_index_sizes(immesh_cloud_index* ix, int64_t* n_pts, int64_t* n_in_tree);

/* Samples the caster's snapshot per the Samples rule.  The samples stay on the device in the caster's own grow-only buffers until the next call or
 * the next build.  n_out (may be NULL) receives the count.  xyz_out (count x 3 floats) and face_out (count int32) may each be NULL; with both NULL
 * only the count is returned.  cap < the count with an output given is IMMESH_E_CAPACITY (the samples stay valid on the device). */
int immesh_mesh_sample(immesh_raycaster* rc, double density, uint64_t seed, float* xyz_out, int32_t* face_out, int64_t cap, int64_t* n_out);

/* The count of the caster's last samples; IMMESH_E_INVAL when none have been made since its last build.  It sizes the outputs of immesh_nearest_samples. */
int immesh_mesh_sample_count(immesh_raycaster* rc, int64_t* n_out);

/* The nearest cloud point of n points (n x 3 floats, host memory): world coordinates when frame is NULL, else sensor coordinates transformed as ray
 * origins are.  Every output may be NULL: d2_out n doubles, dist_out n floats, index_out n int32, xyz_out n x 3 floats. */
int immesh_nearest_points(immesh_cloud_index* ix, const immesh_ray_frame* frame, const float* pts, int64_t n, double max_dist, double* d2_out,
                          float* dist_out, int32_t* index_out, float* xyz_out);
/* The same for the caster's last samples (world coordinates), read where they lie on the device: the index's stream waits on an event the caster
 * records after sampling.  Outputs are sized by the sample count.  Both objects belong to one context; the caller serialises calls on both. */
int immesh_nearest_samples(immesh_cloud_index* ix, immesh_raycaster* rc, double max_dist, double* d2_out, float* dist_out, int32_t* index_out,
                           float* xyz_out);
/* The index's last query of either kind reduced on the device.  stats and hist_out (n_bins int64 counts) may each be NULL. */
int immesh_nearest_reduce(immesh_cloud_index* ix, double bin_width, int32_t n_bins, struct immesh_closest_stats* stats, int64_t* hist_out);
/* Device time in milliseconds from HIP events on the index's stream: [0] the last build  [1] the last query (the traversal kernel)  [2] the last
 * reduction.  Copies are not included. */
int immesh_nearest_last_timing(immesh_cloud_index* ix, float ms[3]);
/* Device time in milliseconds of the caster's last immesh_mesh_sample (HIP events on the caster's stream): [0] the counts  [1] the scan and the emit
 * launch.  The read-back of the total lies between the two and is not included. */
int immesh_mesh_sample_last_timing(immesh_raycaster* rc, float ms[2]);

/* The Neighbours rule for n points (n x 3 floats, host memory; frame as for immesh_nearest_points): count_out n int32, index_out n x k int32,
 * d2_out n x k doubles; each may be NULL. */
int immesh_knn_points(immesh_cloud_index* ix, const immesh_ray_frame* frame, const float* pts, int64_t n, int32_t k, double max_dist, int32_t* count_out,
                      int32_t* index_out, double* d2_out);
/* The same in cloud mode: every point of the index's cloud against the others; the outputs are sized by the cloud (immesh_cloud_index_sizes, points
 * given); mean_out one double per point.  The means and the counts stay on the device for immesh_cloud_outliers_statistical. */
int immesh_knn_cloud(immesh_cloud_index* ix, int32_t k, double max_dist, int32_t* count_out, int32_t* index_out, double* d2_out, double* mean_out);
/* The Count rule for n points, and in cloud mode (the counts stay on the device for immesh_cloud_outliers_radius). */
int immesh_radius_count_points(immesh_cloud_index* ix, const immesh_ray_frame* frame, const float* pts, int64_t n, double radius, int32_t* count_out);
int immesh_radius_count_cloud(immesh_cloud_index* ix, double radius, int32_t* count_out);
/* The Outliers rules: the mask of the cloud on the device, for immesh_cloud_index_apply_outliers.  mu, sigma, threshold, counts (four int64) and
 * keep_out (one uint8 per cloud point) may each be NULL. */
int immesh_cloud_outliers_statistical(immesh_cloud_index* ix, double mult, double* mu, double* sigma, double* threshold, int64_t counts[4],
                                      uint8_t* keep_out);
int immesh_cloud_outliers_radius(immesh_cloud_index* ix, int64_t min_neighbours, int64_t counts[4], uint8_t* keep_out);
/* The Apply rule.  n_out (may be NULL) receives the number of kept points; kept_index_out (that many int32) may be NULL. */
int immesh_cloud_index_apply_outliers(immesh_cloud_index* ix, int32_t* kept_index_out, int64_t cap, int64_t* n_out);
/* The index's cloud as it lies on the device (points given x 3 floats, points that are not finite included); cap < that count with xyz_out given is
 * IMMESH_E_CAPACITY.  n_out may be NULL. */
int immesh_cloud_index_points(immesh_cloud_index* ix, float* xyz_out, int64_t cap, int64_t* n_out);
/* Device time in milliseconds from HIP events on the index's stream: [0] the last traversal of these queries  [1] the last mask  [2] the last apply
 * (scan, compaction and build).  Copies are not included. */
int immesh_knn_last_timing(immesh_cloud_index* ix, float ms[3]);

/* The Clusters rule.  IMMESH_E_INTERNAL is the code of the mesh topology's header (the same tokens: the two headers go together in either order). */
#ifndef IMMESH_E_INTERNAL
#define IMMESH_E_INTERNAL (-8)
#endif
/* The clusters of the index's cloud: label_out one int32 and kind_out one uint8 per cloud point, counts four int64; every output may be NULL.  The
 * clusters stay on the device for the table and the select.  The index's last Count query is not touched. */
int immesh_cloud_clusters(immesh_cloud_index* ix, double radius, int64_t min_neighbours, int32_t* label_out, uint8_t* kind_out, int64_t counts[4],
                          int64_t* n_clusters);
/* The Table rule over the last clusters: one entry per cluster (box_out six floats); each output may be NULL, n_out too. */
int immesh_cloud_clusters_table(immesh_cloud_index* ix, int32_t* first_out, int32_t* n_points_out, int32_t* n_core_out, float* box_out, int64_t cap,
                                int64_t* n_out);
/* The Select rule over the last clusters: the mask of the cloud on the device, for immesh_cloud_index_apply_outliers.  counts (four int64) and
 * keep_out (one uint8 per cloud point) may each be NULL. */
int immesh_cloud_clusters_select(immesh_cloud_index* ix, int64_t min_points, int64_t max_points, int64_t keep_largest, int32_t keep_noise,
                                 int64_t counts[4], uint8_t* keep_out);
/* Device time in milliseconds of the last immesh_cloud_clusters from HIP events on the index's stream: [0] the count and the kinds (the kinds alone
 * when min_neighbours == 0)  [1] the joins  [2] the border walk (0 when min_neighbours == 0)  [3] the numbering and the table.  Copies are not included. */
int immesh_cloud_clusters_last_timing(immesh_cloud_index* ix, float ms[4]);

#ifdef __cplusplus
}
#endif
#endif
