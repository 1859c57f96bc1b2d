/* immesh_simplify.h -- weld, duplicate-face removal and vertex-clustering decimation of a built ray caster's snapshot on the device
 * (libimmesh_hip.so).
 *
 * Reference: none.  The reference writes its mesh to a PLY and leaves "make it smaller" to a desktop tool, as it left "remove isolated pieces";
 * nothing pins this module but the contract below and its checker (tests/simplify_checker.py: np.unique on the cluster keys, a loop over the
 * member rank for the means, a dict for the duplicates; beside it a brute force in plain Python that shares nothing with it).
 * The topology module (immesh_topology_analyse and what follows it) rests on one sentence: "topology is a matter of indices".  That is only
 * useful for a mesh whose faces share vertex indices.  A soup that repeats its vertices (an STL-style export, two exports concatenated, a per-region vertex buffer) analyses as one component per face with
 * every edge a boundary; a face given twice turns three manifold edges into non-manifold ones; and a map of millions of faces wants to be made
 * smaller before it is evaluated.  All three are one rule: vertices that fall together become one, and the faces follow.
 *
 * A header of its own that includes immesh_raycast.h (which does not include it).  It works on an immesh_raycaster built by either build call and
 * needs no analysis.
 *
 * ---- Contract (exact: integers, float bits, and for MEAN one sequential IEEE double sum per coordinate; nothing depends on the order of lanes,
 *      atomics or launches) ----------------------------------------------------------------------------------------------------------------------
 * immesh_simplify(rc, cell, mode, merge_duplicates, stats) clusters the used vertices of the snapshot; nothing reaches the caster before _apply.
 *   Counting face:  as in the topology module: three pairwise different indices.  A vertex is USED when a counting face names it.  Unused vertices
 *            take part in nothing and are dropped.
 *   Cluster: every used vertex belongs to exactly one cluster.
 *            cell == 0 (weld): two used vertices with three finite floats each are together when their floats are equal as values, coordinate by
 *              coordinate; -0 equals +0.
 *            cell > 0: for a used vertex with three finite floats, q_k = floor((double)x_k / cell) per coordinate (IEEE double division, an exact
 *              floor).  The vertex is INSIDE when -2^20 <= q_k < 2^20 holds for all three, tested on the doubles (an infinite quotient is
 *              outside).  Two INSIDE vertices are together when their three q_k are equal.
 *            ALONE: a used vertex with a float that is not finite is a cluster of one; with cell > 0 so is a finite vertex that is not INSIDE.
 *              An ALONE vertex is never merged, not even with a vertex of the same bits.  So the pass has no error that is found after a launch.
 *            A cluster's LABEL is its smallest vertex index; clusters are numbered 0 .. n_clusters - 1 by ascending label, and vmap[v] is that
 *            number (-1 for an unused vertex).
 *   Position of cluster c:
 *            IMMESH_SIMPLIFY_FIRST  the three floats of the label vertex, bit for bit.  No vertex is moved.
 *            IMMESH_SIMPLIFY_MEAN   a cluster of one member gives that vertex's floats bit for bit.  Otherwise, per coordinate, s = 0.0, then
 *                      s = s + (double)x over the members in ascending vertex index, then m = s / (double)n, and the result is (float)m, round to
 *                      nearest even.  No fused multiply-add, nothing reassociated.
 *            With cell == 0 the mode is read, validated and otherwise ignored: positions are FIRST's.
 *   Faces:   counting face f = (i0, i1, i2) maps to g = (vmap[i0], vmap[i1], vmap[i2]): f's rotation and winding are kept.  Its status is the first
 *            that applies:
 *              IMMESH_FACE_NOT_COUNTING (1);
 *              IMMESH_FACE_COLLAPSED    (2)  two entries of g are equal;
 *              IMMESH_FACE_DUPLICATE    (3)  merge_duplicates != 0, and a face with a smaller index has status 0 or 3 and the same SET of three new
 *                                            indices, in any rotation and either winding;
 *              IMMESH_FACE_KEPT         (0).
 *            faces_out = the mapped triples of the kept faces in face order; fmap[f] = the face's position in faces_out, or -1; fstatus[f] = the
 *            status.  With merge_duplicates == 0 nothing is a duplicate.
 *   Per cluster: first_vertex (the label), n_members.
 *   Stats:   n_vertices_in (the snapshot's), n_vertices_used, n_alone_not_finite, n_alone_outside, n_vertices_out (= n_clusters), largest_cluster,
 *            n_faces_in, n_not_counting, n_collapsed, n_duplicate, n_faces_out.
 *   Facts:   every face of faces_out counts and has its indices in [0, n_vertices_out).  A cluster that loses all its faces (they collapsed, or
 *            were duplicates) is KEPT: n_vertices_out counts clusters, not the vertices that faces_out still names, so vtx_out may hold vertices
 *            no face uses.  With FIRST, a second pass with the same arguments over (vtx_out, faces_out) has every cluster of size one, nothing
 *            collapsed, nothing duplicate, and returns its input -- when every cluster of the first pass kept a face.  For MEAN no idempotence is
 *            claimed: a rounded mean can cross a cell wall.  With MEAN and cell > 0 every output coordinate lies within cell of every member's
 *            coordinate, up to one float rounding.
 *   Apply:   afterwards the caster behaves in every call as one freshly built by immesh_raycast_build_triangles from vtx_out and faces_out: equal
 *            answers bit for bit, and everything a build discards is discarded, this result included.  The buffers change places on the device
 *            and the caster's own build runs; there is no host round trip of the mesh.  n_faces_out == 0 is a valid build.
 * Validated before any launch: a built caster; 0 <= cell finite; mode one of the two; cap >= 0; n_vtx <= 2^31 - 2 (the sort's and the scan's int
 * count); a result of the current snapshot before any fetch or apply -- else IMMESH_E_INVAL with text in immesh_last_error(ctx).  A rebuild of the
 * caster discards the result, and so do immesh_topology_orient_apply and immesh_topology_holes_apply: the faces changed.  Zero faces give zeros in
 * every count but n_vertices_in; that is not an error.
 */
#ifndef IMMESH_SIMPLIFY_H
#define IMMESH_SIMPLIFY_H
#include "immesh_raycast.h"
#ifdef __cplusplus
extern "C" {
#endif

#define IMMESH_SIMPLIFY_FIRST 0
#define IMMESH_SIMPLIFY_MEAN 1

#define IMMESH_FACE_KEPT 0
#define IMMESH_FACE_NOT_COUNTING 1
#define IMMESH_FACE_COLLAPSED 2
#define IMMESH_FACE_DUPLICATE 3

typedef struct immesh_simplify_stats {
    int64_t n_vertices_in;            /* vertices of the snapshot */
    int64_t n_vertices_used;
    int64_t n_alone_not_finite;
    int64_t n_alone_outside;
    int64_t n_vertices_out;           /* n_clusters: a cluster that lost all its faces is kept */
    int64_t largest_cluster;
    int64_t n_faces_in;               /* faces of the snapshot */
    int64_t n_not_counting;
    int64_t n_collapsed;
    int64_t n_duplicate;
    int64_t n_faces_out;
} immesh_simplify_stats;

/* The rule above on the caster's snapshot; stats may be NULL.  Nothing is allocated or launched for this module before the first call; the buffers
 * are grow-only.  The result stays on the device for the calls below until the caster is rebuilt or an apply (this one, the orientation's or the
 * holes') has run.  No read-back lies between its launches. */
int immesh_simplify(immesh_raycaster* rc, double cell, int32_t mode, int32_t merge_duplicates, immesh_simplify_stats* stats);
/* The cluster tables, n_vertices_out entries each (vtx_out: 3 floats per cluster).  Every pointer may be NULL; n_out gets n_vertices_out.  With any
 * array given, cap < n_vertices_out is IMMESH_E_CAPACITY (n_out is still set). */
int immesh_simplify_vertices(immesh_raycaster* rc, float* vtx_out /* 3 per cluster */, int32_t* first_vertex, int32_t* n_members, int64_t cap,
                             int64_t* n_out);
/* vmap n_vtx int32, fmap n_faces int32, fstatus n_faces int8; each may be NULL. */
int immesh_simplify_maps(immesh_raycaster* rc, int32_t* vmap /* n_vtx */, int32_t* fmap /* n_faces */, int8_t* fstatus /* n_faces */);
/* The kept faces over the new indices, 3 per face.  faces_out may be NULL; n_out gets n_faces_out.  With it given, cap < n_faces_out is
 * IMMESH_E_CAPACITY. */
int immesh_simplify_faces(immesh_raycaster* rc, int32_t* faces_out /* 3 per kept face */, int64_t cap, int64_t* n_out);
/* The Apply rule: vtx_out and faces_out change places with the caster's buffers on the device, then the caster's own build. */
int immesh_simplify_apply(immesh_raycaster* rc);
/* Device time in milliseconds from HIP events on the caster's stream: [0] the last pass (every launch)  [1] the last apply (the build of the
 * hierarchy). */
int immesh_simplify_last_timing(immesh_raycaster* rc, float ms[2]);   /* [0] simplify  [1] apply */

#ifdef __cplusplus
}
#endif
#endif
