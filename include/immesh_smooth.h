/* immesh_smooth.h -- the one-ring table, Taubin (lambda | mu) smoothing and area-weighted vertex normals of a built ray caster's snapshot on the
 * device (libimmesh_hip.so).
 *
 * Reference: none.  The reference's Global_map::smooth_pts (carried as immesh_smooth_pts) is a kNN average of the live map's points for display: it
 * knows nothing of the faces, cannot run on a loaded mesh and shrinks what it smooths.  Nothing pins this module but the contract below and its
 * checker (tests/smooth_checker.py: np.unique on the pair keys and a loop over the rank k that adds the k-th neighbour of every vertex; beside it a
 * brute force in plain Python that shares nothing with it).
 * The clean-up chain (analyse, fragment filter, orient, fill holes, weld and decimate) leaves the vertex positions alone.  The fans of the holes rule
 * and the cluster means of immesh_simplify put vertices where the rule says, not where the surface is, and a LiDAR mesh is noisy to begin with.  What
 * moves a vertex towards its surface, and what gives it a normal, both gather over the vertex's one-ring, so the table comes first.
 *
 * A header of its own that includes immesh_raycast.h (which does not include it).  It works on an immesh_raycaster built by either build call and
 * needs no analysis.
 *
 * ---- Contract (exact: integers, float bits, and one sequential IEEE double sum per coordinate in a stated order; nothing depends on the order of
 *      lanes, atomics or launches) ----------------------------------------------------------------------------------------------------------------
 * Counting face, used vertex, edge and uses(e) are as in the topology module.  A vertex is FINITE when its three floats in the snapshot are finite;
 * this is decided once, on the input of the pass.
 *   One-ring: L(v) = the distinct vertices u such that {u, v} is an edge of a counting face, in ascending u; with each entry goes uses({u, v}).
 *            row_start has n_vtx + 1 int64 entries (L(v) is neighbours[row_start[v] .. row_start[v + 1])), neighbours[] and uses[] are int32.
 *            n_pairs = the sum of |L(v)| = 2 n_edges of an analysis of the same snapshot.  Whether a vertex is FINITE plays no part here: the table
 *            is a function of the face array alone.
 *   Class:   int8 per vertex, the first that applies:
 *              IMMESH_VERTEX_UNUSED     (0)  not used by a counting face;
 *              IMMESH_VERTEX_NOT_FINITE (1)  used and not FINITE;
 *              IMMESH_VERTEX_BORDER     (2)  an endpoint of an edge with uses != 2 (a boundary edge or a non-manifold one);
 *              IMMESH_VERTEX_INTERIOR   (3)  otherwise.
 *   Smoothing list S(v), in L(v)'s order:
 *              UNUSED and NOT_FINITE: empty.
 *              INTERIOR: the FINITE members of L(v).
 *              BORDER:   IMMESH_SMOOTH_BORDER_FIXED (0)  empty;
 *                        IMMESH_SMOOTH_BORDER_ALONG (1)  the FINITE u of L(v) with uses({u, v}) != 2: the border slides along itself (and along a
 *                                                        non-manifold fin);
 *                        IMMESH_SMOOTH_BORDER_FREE  (2)  as INTERIOR.
 *            v is MOVING when S(v) is not empty.  The lists do not change between the steps.
 *   Step j = 0 .. n_steps - 1: the factor w is lambda for even j and mu for odd j.  Plain Laplacian smoothing is mu == lambda; Taubin is
 *            mu < -lambda < 0.  Every vertex reads the positions P_j and writes P_(j + 1) (Jacobi); P_0 is the snapshot.  A vertex that is not
 *            MOVING is copied bit for bit.  For a MOVING v, per coordinate k:
 *              s = 0.0;  s = s + (double)P_j[u][k] over u in S(v) in order;  m = s / (double)|S(v)|;  x = (double)P_j[v][k];  t = m - x;  t = w * t;
 *              r_k = (float)(x + t), round to nearest even.
 *            IEEE double throughout, no fused multiply-add, nothing reassociated.
 *   Hold:    if any of r_0, r_1, r_2 is not finite, v keeps all three floats of P_j for this step, and n_held counts the event (in vertex-steps).
 *            So a MOVING vertex is finite after every step, and no sum ever sees a value that is not finite.
 *   Consequences: n_steps == 0 returns the snapshot bit for bit.  A step with w == 0 is not the identity on bits: t is then a zero with the sign of
 *            w (m - x), and x + t turns a coordinate -0 into +0 unless t is -0 too.
 *   Stats:   n_vertices, n_used, n_not_finite, n_border, n_interior, n_moving, n_pairs, max_valence (the largest |L(v)|), n_steps, n_held,
 *            n_moved (the vertices with a float of P_n that differs in bits from P_0), and one double, max_disp2: the largest
 *            (dx dx + dy dy) + dz dz with d = (double)P_n - (double)P_0 over the MOVING vertices, 0 without one.  A maximum is order-free.
 *   Apply:   afterwards the caster behaves in every call as one freshly built by immesh_raycast_build_triangles from vtx_out and the same faces:
 *            equal answers bit for bit, and everything a build discards is discarded, this result included.  vtx_out changes places with the
 *            caster's vertex buffer on the device, then the caster's own build runs: boxes and Morton codes change, so the hierarchy is rebuilt,
 *            not kept.  There is no host round trip of the mesh.
 *   Vertex normals are of the current snapshot; they need no smoothing pass, and they follow an apply.
 *            F(v) = the counting faces that name v and whose three vertices are all FINITE, in ascending face index.  Per face (i0, i1, i2), with
 *            a, b, c its vertices widened to double in that order, whichever of them v is: n_f = cross(b - a, c - a), cross and dot as in
 *            immesh_raycast.h.  Per coordinate s = 0.0, then s = s + n_f over F(v) in order.  q = dot(s, s), len = sqrt(q), the double square root
 *            correctly rounded as the closest-point query requires.  If len > 0 the normal is (float)(s_k / len); otherwise it is three +0 floats and
 *            n_zero counts the vertex: an empty F(v), a cancelled sum, an underflowed q.
 *            q cannot overflow: a difference of two floats is below 2^129, a component of n_f below 2^259, a sum over fewer than 2^31 faces below
 *            2^290, and q below 3 * 2^580 < 2^1024.
 * Validated before any launch: a built caster; 0 <= n_steps <= 65536; lambda and mu finite and in [-1, 1]; border one of the three;
 * 6 n_faces <= 2^31 - 2 and n_vtx <= 2^31 - 2 (the sort's and the scan's int counts); cap >= 0; a smoothing pass of the current snapshot before any
 * fetch or apply -- else IMMESH_E_INVAL with text in immesh_last_error(ctx), and nothing touched.  A rebuild of the caster discards the result, and so
 * do immesh_topology_orient_apply, immesh_topology_holes_apply and immesh_simplify_apply.  Zero faces give zeros in every count but n_vertices (and
 * n_steps); that is not an error.
 */
#ifndef IMMESH_SMOOTH_H
#define IMMESH_SMOOTH_H
#include "immesh_raycast.h"
#ifdef __cplusplus
extern "C" {
#endif

#define IMMESH_VERTEX_UNUSED 0
#define IMMESH_VERTEX_NOT_FINITE 1
#define IMMESH_VERTEX_BORDER 2
#define IMMESH_VERTEX_INTERIOR 3

#define IMMESH_SMOOTH_BORDER_FIXED 0
#define IMMESH_SMOOTH_BORDER_ALONG 1
#define IMMESH_SMOOTH_BORDER_FREE 2

#define IMMESH_SMOOTH_MAX_STEPS 65536

typedef struct immesh_smooth_stats {
    int64_t n_vertices;               /* vertices of the snapshot */
    int64_t n_used;
    int64_t n_not_finite;
    int64_t n_border;
    int64_t n_interior;
    int64_t n_moving;
    int64_t n_pairs;                  /* the one-ring's entries: 2 n_edges */
    int64_t max_valence;
    int64_t n_steps;
    int64_t n_held;                   /* vertex-steps */
    int64_t n_moved;
    double max_disp2;
} immesh_smooth_stats;

/* The rule above on the caster's snapshot; stats may be NULL.  Nothing is allocated or launched for this module before the first call; the buffers
 * are grow-only.  The result stays on the device for the calls below until the caster is rebuilt or an apply (this one, the orientation's, the
 * holes' or the simplification's) has run.  No read-back lies between its launches. */
int immesh_smooth(immesh_raycaster* rc, int32_t n_steps, double lambda, double mu, int32_t border, immesh_smooth_stats* stats);
/* P_n, 3 floats per vertex of the snapshot, and the classes; each may be NULL. */
int immesh_smooth_vertices(immesh_raycaster* rc, float* vtx_out /* 3 n_vtx */, int8_t* vclass /* n_vtx */);
/* The one-ring table.  Every pointer may be NULL; n_out gets n_pairs.  With any array given, cap < n_pairs is IMMESH_E_CAPACITY ("cap %d < %d";
 * n_out is still set and nothing is written).  cap counts the entries of neighbours and uses; row_start always has n_vtx + 1. */
int immesh_smooth_adjacency(immesh_raycaster* rc, int64_t* row_start /* n_vtx + 1 */, int32_t* neighbours, int32_t* uses, int64_t cap, int64_t* n_out);
/* The Apply rule: vtx_out changes places with the caster's vertex buffer on the device, then the caster's own build. */
int immesh_smooth_apply(immesh_raycaster* rc);
/* Device time in milliseconds from HIP events on the caster's stream. */
int immesh_smooth_last_timing(immesh_raycaster* rc, float ms[3]);   /* [0] the one-ring and classes  [1] the steps  [2] the apply */
/* The Vertex normals rule on the current snapshot; each pointer may be NULL.  Its incidence table is allocated at the first call, never before. */
int immesh_vertex_normals(immesh_raycaster* rc, float* normals_out /* 3 n_vtx */, int64_t* n_zero);

#ifdef __cplusplus
}
#endif
#endif
