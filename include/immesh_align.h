/* immesh_align.h -- align a cloud to the mesh: iterated closest-face least squares (ICP) on a built ray caster (libimmesh_hip.so).
 *
 * Reference: none.  The reference registers scans to its plane map, never a cloud to its mesh; nothing pins this module but the contract below and
 * its checker (tests/align_checker.py: brute-force correspondences, scalar float64 arithmetic in the written order, math.fsum for the sums).
 * It answers "which small rigid motion brings this cloud onto the mesh": the refinement every evaluation protocol applies before accuracy,
 * completeness, Chamfer and F-score are read, because a survey scan registered by hand or by GPS is a few centimetres and a fraction of a degree
 * off.  It refines a pose that is already within max_dist; it is no global registration.  It works on an immesh_raycaster built by either build
 * call of immesh_raycast.h and, like the closest query, is a question about points: it changes nothing of the caster's snapshot or of any result
 * derived from it, and the last closest query's results stay byte for byte across an alignment.
 *
 * A header of its own that includes immesh_raycast.h; nothing includes it.  Its contract stands on the rules of the point-to-mesh header (the one that
 * declares immesh_closest_points), which it cites by their names and does not include: that header's rule is that no other header names it, and
 * no type of it is needed here.
 *
 * ---- Contract (exact; all arithmetic in IEEE double, in the order written, no fused multiply-add) -------------------------------------------
 *   dot, cross, the Point, Face, Box, D and Winner rules: those of immesh_closest_points' header, unchanged, with r2 = max_dist max_dist.
 *   Correspondence: p = the point under the current frame (Point rule).  The winning face gives q (its closest point relative to p), its corners
 *            a, b, c relative to p and ab = b - a, ac = c - a.  A point without a winner is counted n_no_face, or n_not_finite by the Point rule,
 *            and contributes nothing.
 *   Reference point: x_k = p_k - centre_k.  The motion is linearised about `centre` (three doubles of the options, zero by default): about the
 *            cloud's centroid instead of the world's origin H stays well conditioned 300 m away from the origin.
 *   Rows:    with delta = (omega, v) a row is (j, r), j six doubles: the model of the residual is r - dot6(j, delta).
 *            POINT (mode 0): three rows k = 0, 1, 2 with u = e_k (the unit vector: 1.0 at k, 0.0 elsewhere; the products with its zeros are made):
 *              j = (cross(x, u), u), r = q_k.
 *            PLANE (mode 1): one row.  n = cross(ab, ac), nn = dot(n, n).  A winner whose nn is not both finite and > 0 is counted n_flat and the
 *              point contributes nothing.  Else s = sqrt(nn), u_k = n_k / s, j = (cross(x, u), u), r = dot(u, a).
 *   Terms:   28 doubles per taking-part point, in this order: H_ab for a <= b row by row (H_00 .. H_05, H_11 .. H_15, .. H_55: index
 *            a (13 - a) / 2 + (b - a)), then g_0 .. g_5, then e.  H_ab = the sum over the rows of j[a] j[b], g_a = of j[a] r, e = of r r, each
 *            begun with row 0's product and continued in ascending k: (t_0 + t_1) + t_2.  These 28 doubles are exact by contract; a point that
 *            does not take part has 28 zeros.
 *   System:  the 28 sums over the taking-part points and the counts n_used, n_not_finite, n_no_face, n_flat (their sum is n_pts).  The sums are
 *            made in a fixed order of additions that depends on n_pts alone: two calls give the same bits.  The order itself is not part of the
 *            contract: each sum lies within n_pts 2^-52 (the sum of |term|) of the exact sum.
 *   Solve:   (host)  A_ab = A_ba = H_ab, then A_aa = H_aa + damping.  m = the largest A_aa (m = A_00; a larger A_aa replaces it).
 *            Cholesky A = L L^T column by column, j = 0 .. 5:
 *              s = A_jj; for k = 0 .. j - 1: s = s - L_jk L_jk.  The pivot s fails when it is not finite, when s <= 0 or when s <= 2^-40 m:
 *              DEGENERATE (the return value 1; delta is set to six zeros).  L_jj = sqrt(s).
 *              for i = j + 1 .. 5: t = A_ij; for k = 0 .. j - 1: t = t - L_ik L_jk;  L_ij = t / L_jj.
 *            forward, i = 0 .. 5:  t = g_i; for k = 0 .. i - 1: t = t - L_ik y_k;  y_i = t / L_ii.
 *            back, i = 5 .. 0:     t = y_i; for k = i + 1 .. 5: t = t - L_ki delta_k;  delta_i = t / L_ii.
 *   Exp:     K = [omega]x = ((0, -w2, w1), (w2, 0, -w0), (-w1, w0, 0)), th2 = dot(omega, omega), th = sqrt(th2).
 *            th < 2^-26: E = I + K (E_ij = I_ij + K_ij).  Else a = sin(th) / th, h = sin(0.5 th), b = (2 (h h)) / th2 (which is (1 - cos th) / th2
 *            without its cancellation), KK_ij = (K_i0 K_0j + K_i1 K_1j) + K_i2 K_2j, E_ij = (I_ij + a K_ij) + b KK_ij: Rodrigues' formula.
 *            sin is the C library's: it may differ from another library's in the last place, so Exp is not bit for bit across platforms.
 *   Update:  R' = E R: R'_ij = (E_i0 R_0j + E_i1 R_1j) + E_i2 R_2j.  d = t - centre;  t'_i = (((E_i0 d_0 + E_i1 d_1) + E_i2 d_2) + centre_i) + v_i.
 *            No re-orthonormalisation: R' R'^T - I stays within a few 2^-52 per update.
 *   Loop:    frame = frame0 (the identity when NULL); for it = 0 .. max_iters - 1:
 *              the step at frame -> system; iterations = it + 1; rows = 3 n_used (POINT) or n_used (PLANE); rms = sqrt(e / rows), 0 without a row.
 *              n_used < 3 (POINT) / 6 (PLANE): TOO_FEW, stop (the frame is not changed).   The solve fails: DEGENERATE, stop (the same).
 *              frame = Update(frame, centre, delta).  sqrt(dot(omega, omega)) <= eps_rot and sqrt(dot(v, v)) <= eps_trans: CONVERGED, stop.
 *            otherwise MAX_ITERS.  None of the four is an error return.  A history row is (n_used, rms, |omega|, |v|), the last two 0 for
 *            an iteration without a solution.
 * The result is a function of the soup, the points, the frame and the options alone: not of how the hierarchy was built, of the order in which
 * lanes or nodes are visited, or of the launch shape.  A caster with no face in its hierarchy gives TOO_FEW; that is not an error.
 * Validated before any launch: a built caster; a finite frame when one is given, a finite centre; 0 < max_dist finite; mode 0 or 1; damping >= 0
 * finite; 1 <= max_iters <= 10000; eps_rot, eps_trans >= 0 finite; n_pts in [0, 2^31 - 2]; else IMMESH_E_INVAL with text in immesh_last_error(ctx).
 * immesh_align_step checks what it reads: the caster, the frame, the centre, max_dist, mode and the points.
 *
 * ---- Cloud rule: align a cloud to the indexed cloud (nearest-point least squares) ---------------------------------------------------------------------
 * The target is the cloud of an immesh_cloud_index (the mesh-to-cloud header's, the one that declares immesh_nearest_points; named here by its tag
 * alone, and that header is not included), not a mesh: scan-to-scan registration, a sweep placed in a survey cloud, an alignment before any mesh
 * exists.  All arithmetic is IEEE double, in the order written, no fused multiply-add.  The Point, Cloud, D, Winner and Box rules are those of the
 * mesh-to-cloud header, with r2 = max_dist max_dist.  Reference point, Rows, Terms, System, Solve, Exp, Update and Loop are the rules above, word for
 * word, except where stated here.
 *   Correspondence: p = the source point under the current frame (Point rule).  The winner is the cloud point c_j with the smallest D; on equal D
 *            the smaller index wins.  q_k = (double)c_j,k - p_k: these are the e_k of the D rule, so D is (q_x q_x + q_y q_y) + q_z q_z bit for bit.
 *            A point without a winner is counted n_no_face (read here: no neighbour), one that fails the Point rule n_not_finite; neither contributes.
 *   POINT rows: as above: three rows j = (cross(x, e_k), e_k), r = q_k.  On a caster built from the target as a soup of degenerate faces (i, i, i) the
 *            mesh rule's Face rule returns the corner, its q is this q and its D this D (the Box bound of a point's own box is D), so in POINT mode
 *            with huber == 0 the two rules give the same terms and the same system, bit for bit.
 *   PLANE rows: one row.  It needs the index's stored normals (immesh_cloud_normals, made since the index's last build or apply); without them the
 *            call is IMMESH_E_INVAL with text, before any launch.  A winner whose normal status is not 0 is counted n_flat (read here: a winner
 *            without a normal) and the point contributes nothing.  Else u_a = the stored float normal widened to double -- it is not renormalised:
 *            |u| is 1 within float rounding --, j = (cross(x, u), u), r = (u_x q_x + u_y q_y) + u_z q_z.
 *            Negating u negates j and r exactly (every product and sum of cross and of r changes its sign and nothing else), and the 28 terms are
 *            products of two of them: they do not depend on the sign mode the normals were made with.
 *   Weight:  huber >= 0, finite.  huber == 0: the terms are as above.  huber > 0: d = sqrt(D) (POINT), d = |r| (PLANE); w = 1.0 when d <= huber, else
 *            w = huber / d; each of the 28 terms t becomes w t.  The rms of the Loop rule is then the weighted one: sqrt of the weighted e over the
 *            rows.
 *   Loop:    as above: TOO_FEW below 3 (POINT) / 6 (PLANE) used points.  An empty index gives TOO_FEW; that is not an error.
 * Validated before any launch: what immesh_align checks (a built index in the caster's place), huber, and in PLANE mode the normals; else
 * IMMESH_E_INVAL with text.  A refused call leaves the index as it was, and a call that succeeds leaves the index's query results, neighbour results,
 * masks, clusters and normals byte for byte as they were.
 */
#ifndef IMMESH_ALIGN_H
#define IMMESH_ALIGN_H
#include "immesh_raycast.h"
#ifdef __cplusplus
extern "C" {
#endif

#define IMMESH_ALIGN_POINT 0
#define IMMESH_ALIGN_PLANE 1

#define IMMESH_ALIGN_CONVERGED 0
#define IMMESH_ALIGN_MAX_ITERS 1
#define IMMESH_ALIGN_TOO_FEW 2
#define IMMESH_ALIGN_DEGENERATE 3

typedef struct immesh_align_options {
    int32_t mode;            /* IMMESH_ALIGN_POINT / _PLANE */
    int32_t max_iters;
    double max_dist;
    double centre[3];
    double damping;
    double eps_rot, eps_trans;
} immesh_align_options;

typedef struct immesh_align_system {
    double H[21];            /* a <= b, row by row */
    double g[6];
    double e;
    int64_t n_used, n_not_finite, n_no_face, n_flat;
} immesh_align_system;

typedef struct immesh_align_result {
    immesh_ray_frame frame;  /* the final frame */
    int32_t status;          /* IMMESH_ALIGN_CONVERGED .. _DEGENERATE */
    int32_t iterations;      /* steps made */
    immesh_align_system system;   /* the last step's */
    double rms;              /* the last step's */
} immesh_align_result;

/* mode POINT, max_iters 30, max_dist 1, centre 0, damping 0, eps_rot 1e-9, eps_trans 1e-9 */
void immesh_align_default_options(immesh_align_options* opts);

/* One step at `frame` (NULL: the points are world coordinates): pts n_pts x 3 floats in host memory.  It reads mode, max_dist and centre of opts.
 * face_out (n_pts int32, -1 without a face) and terms_out (n_pts x 28 doubles) may each be NULL; they exist for the tests, and when both are NULL the
 * kernel stores nothing per point.  Nothing is allocated or launched for an alignment before the first one; the buffers are grow-only. */
int immesh_align_step(immesh_raycaster* rc, const immesh_ray_frame* frame, const float* pts, int64_t n_pts, const immesh_align_options* opts,
                      immesh_align_system* system_out, int32_t* face_out, double* terms_out);
/* The Solve rule: 0, or 1 for DEGENERATE.  Pure host code; needs no caster.  A negative or non-finite damping is IMMESH_E_INVAL. */
int immesh_align_solve(const immesh_align_system* system, double damping, double delta_out[6]);
/* The Update rule.  Pure host code; frame_out may be frame. */
int immesh_align_update(const immesh_ray_frame* frame, const double centre[3], const double delta[6], immesh_ray_frame* frame_out);
/* The Loop rule.  The cloud goes to the device once; an iteration is the step's launches, one copy of the folded system to pinned memory and the host
 * solve (the two functions above).  history_out (may be NULL) receives min(iterations, history_cap) rows of 4 doubles. */
int immesh_align(immesh_raycaster* rc, const immesh_ray_frame* frame0, const float* pts, int64_t n_pts, const immesh_align_options* opts,
                 immesh_align_result* result_out, double* history_out, int64_t history_cap);
/* Device time in milliseconds from HIP events on the caster's stream: [0] the last step  [1] the sum over the last loop's steps (the last step's
 * after an immesh_align_step).  The copy of the points to the device is not included. */
int immesh_align_last_timing(immesh_raycaster* rc, float ms[2]);
/* For measurements (tools/align_bench.py): 0 the fused step (the default: one launch walks, forms the terms and folds them, its registers held to
 * the walk's occupancy), 1 the split step -- the walk stores face and q per point, a second launch forms and folds the terms --, 2 the fused step
 * without the register cap.  All give the same bits; DESIGN section 26 has their figures. */
int immesh_align_set_variant(immesh_raycaster* rc, int32_t variant);

/* ---- the Cloud rule: the same options, system and result, their layouts unchanged ---- */
struct immesh_cloud_index;     /* the cloud index of the mesh-to-cloud header (its typedef immesh_cloud_index names the same type) */

/* One step at `frame` (NULL: the points are world coordinates) against the index's cloud.  It reads mode, max_dist and centre of opts.  index_out
 * (n_pts int32: the winner, -1 without one) and terms_out (n_pts x 28 doubles) may each be NULL; when both are NULL nothing is stored per point.
 * Nothing is allocated or launched for this rule before its first call; the buffers are grow-only and the launches run on the index's stream. */
int immesh_align_cloud_step(struct immesh_cloud_index* ix, const immesh_ray_frame* frame, const float* pts, int64_t n_pts,
                            const immesh_align_options* opts, double huber, immesh_align_system* system_out, int32_t* index_out, double* terms_out);
/* The Loop rule over that step, with immesh_align_solve and immesh_align_update.  history_out as immesh_align's. */
int immesh_align_cloud(struct immesh_cloud_index* ix, const immesh_ray_frame* frame0, const float* pts, int64_t n_pts, const immesh_align_options* opts,
                       double huber, immesh_align_result* result_out, double* history_out, int64_t history_cap);
/* Device time in milliseconds from HIP events on the index's stream: [0] the last step  [1] the sum over the last loop's steps (the last step's
 * after an immesh_align_cloud_step).  The copy of the points to the device is not included. */
int immesh_align_cloud_last_timing(struct immesh_cloud_index* ix, float ms[2]);
/* For measurements (tools/align_cloud_bench.py): 0 the fused step, one launch whose registers are held to the walk's occupancy; 1 the split step --
 * the walk stores winner and q per point, a second launch forms and folds the terms.  Both give the same bits.  The default is 1: measured, the fused
 * step is level with the split one up to 100 000 points and 11 % slower at 1 000 000. */
int immesh_align_cloud_set_variant(struct immesh_cloud_index* ix, int32_t variant);

#ifdef __cplusplus
}
#endif
#endif
