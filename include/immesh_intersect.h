/* immesh_intersect.h -- self-intersections of a built ray caster's snapshot on the device (libimmesh_hip.so): the pairs of faces that pass through
 * each other, per face the number of such pairs, and their removal.
 *
 * Reference: none.  The reference writes its mesh and never asks whether it folds through itself; nothing pins this module but the contract below
 * and its checkers (tests/intersect_checker.py: a brute force over all i < j, and a uniform-grid candidate finder; the two share only the segment
 * test).
 * Three links of the clean-up chain put faces or vertices "where the rule says, not where the surface is" (include/immesh_smooth.h): the hole fans
 * are not geometry-aware, vertex clustering snaps whole cells together, Taubin steps with a free or sliding border move vertices across their
 * neighbours.  Each can fold the surface through itself, and so does a small share of the incremental mesher's own voxel triangulations.  side_out of
 * the closest-point query, a signed accuracy, exported normals and ray-cast visibility mean little across a fold; this module says whether there is
 * one, where, and takes the offending faces out so that the Holes rule can close what remains.
 *
 * A header of its own that includes immesh_raycast.h (which does not include it).  It works on an immesh_raycaster built by either build call and
 * needs no analysis: it reads the caster's vertices, faces and hierarchy.
 *
 * ---- Contract (exact: integers are compared bit for bit; all arithmetic in IEEE double, in the order written, no fused multiply-add; nothing
 *      depends on how the hierarchy was built, on lanes, on atomics or on launches) ---------------------------------------------------------------
 *   Face:      a face TAKES PART when it is in the hierarchy (it has no vertex that is not finite: immesh_raycast.h, the Face rule) and is a
 *              counting face as in the topology module: three pairwise different indices.  n_taking_part counts these faces.
 *   Candidate: an unordered pair i < j of faces that take part whose float boxes overlap, closed, on all three axes:
 *              lo_i[k] <= hi_j[k] && lo_j[k] <= hi_i[k], with lo, hi as in the caster's Box rule (the smallest and the largest of the face's three
 *              float coordinates k).  n_candidates is their number: a function of the soup alone.  The box test is part of the rule as the
 *              caster's Box rule is part of the cast's: a pair whose boxes are disjoint never counts, whatever rounding makes of its arithmetic, and
 *              so no enclosing node box can cull a pair that counts (DESIGN.md has the argument).
 *   Shared:    sh(i, j) = the number of vertex indices the two faces have in common, 0 to 3 -- by INDEX, not by position.  On an unwelded soup
 *              (every face with vertices of its own) every neighbour touches its neighbour at s = 0 or s = 1 and COUNTS as a pair; weld first
 *              (immesh_simplify with cell == 0, include/immesh_simplify.h).  n_share[4] counts the candidates by sh.
 *   Segment:   hit(p, q, T) for the segment from vertex p to vertex q and the face T = (t0, t1, t2) is the caster's Face, Cover and Depth rule word
 *              for word with o = (double)p and d_k = (double)q_k - (double)p_k:  a, b, c = (double)t0 - o, (double)t1 - o, (double)t2 - o;
 *              ab = cross(a, b), bc = cross(b, c), ca = cross(c, a), n = cross(b - a, c - a), na = dot(n, a);
 *              e0 = dot(ab, d), e1 = dot(bc, d), e2 = dot(ca, d): covered when all three are >= 0 or all three are <= 0;
 *              nd = dot(n, d); nd == 0 skips; s = na / nd; the fragment counts when 0 <= s <= 1, closed at both ends.  There is no g margin: the
 *              Candidate rule stands in for it.  Nothing here can be NaN (the vertices are finite floats); an s that overflows fails the comparison.
 *   Pair mask: 6 bits.  With A = face i and B = face j, i < j:  bit k (k = 0, 1, 2) = hit(A_k, A_((k+1) mod 3), B);
 *              bit 3 + k = hit(B_k, B_((k+1) mod 3), A).  Which bits are evaluated depends on sh:
 *                sh == 0  all six;
 *                sh == 1  only the one edge of each face that does not contain the shared vertex; the other four bits are 0;
 *                sh >= 2  none: an edge neighbour can only meet its neighbour along the shared edge or by lying in its plane, and a duplicate is
 *                         the weld's business.
 *              The pair INTERSECTS when its mask is not 0.
 *   Not detected, by rule:  coplanar overlaps (every nd is 0, or noise that Cover rejects);  edge neighbours folded onto each other (sh == 2 is
 *              never evaluated);  duplicates (sh == 3 likewise).
 *   Results:   the intersecting pairs in ascending (i, j) with their masks;  per face n_partners[f] = the pairs it is in, as i or as j (int32; 0 for
 *              a face that does not take part).
 *   Stats:     n_faces, n_in_tree, n_taking_part, n_candidates, n_share[4], n_pairs, n_pairs_share0, n_pairs_share1, n_faces_hit (faces with
 *              n_partners > 0), max_partners.
 *   Apply:     the faces with n_partners == 0 are kept, in order -- those that do not take part included: they were not judged.  The others go; the
 *              vertices stay.  face_map[f] = the new index of old face f, or -1 (fetch it before the apply).  Afterwards the caster behaves in every
 *              call as one freshly built by immesh_raycast_build_triangles from the same vertices and the kept faces: equal answers bit for bit, and
 *              everything a build discards is discarded, this result included.  The compaction runs on the device, the result changes places with
 *              the caster's face buffer, and the caster's own build follows.  A second pass after an apply finds n_pairs == 0: a kept face had no
 *              partner, and removal creates none.
 * Validated before any launch: a built caster; max_candidates in [1, 2^31 - 2]; cap >= 0; a result of the current snapshot before any fetch or apply
 * -- else IMMESH_E_INVAL with text in immesh_last_error(ctx), and nothing is touched.  A rebuild of the caster and every apply (the orientation's
 * too: the mask bits are named by each face's vertex order) discard the result; a new analysis leaves it.  Zero faces, or one, give zeros; that is
 * not an error.
 */
#ifndef IMMESH_INTERSECT_H
#define IMMESH_INTERSECT_H
#include "immesh_raycast.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct immesh_intersect_stats {
    int64_t n_faces;                  /* faces of the snapshot */
    int64_t n_in_tree;                /* those without a vertex that is not finite */
    int64_t n_taking_part;            /* and with three pairwise different indices */
    int64_t n_candidates;
    int64_t n_share[4];               /* the candidates by shared vertex indices */
    int64_t n_pairs;
    int64_t n_pairs_share0;
    int64_t n_pairs_share1;
    int64_t n_faces_hit;              /* faces with n_partners > 0: what an apply removes */
    int64_t max_partners;
} immesh_intersect_stats;

/* The rule above on the caster's snapshot; stats may be NULL.  Nothing is allocated or launched for this module before the first call; the buffers
 * are grow-only and sized by the candidates the snapshot has, never by max_candidates.  A snapshot with more than max_candidates candidate pairs is
 * IMMESH_E_CAPACITY ("cap <max_candidates> < <n> candidate pairs"): no result exists then, and stats->n_candidates and the counts before it are
 * still written (300 000 copies of one face have 4.5e10 candidates).  The candidate count comes back to the host once, the hit count once. */
int immesh_self_intersect(immesh_raycaster* rc, int64_t max_candidates, immesh_intersect_stats* stats);
/* The intersecting pairs in ascending (i, j): pairs[2 h], pairs[2 h + 1] = i, j; mask[h] = the pair mask.  Each pointer may be NULL; n_out gets
 * n_pairs.  With an array given, cap < n_pairs is IMMESH_E_CAPACITY (n_out is still set). */
int immesh_self_intersect_pairs(immesh_raycaster* rc, int32_t* pairs /* 2 cap */, uint8_t* mask /* cap */, int64_t cap, int64_t* n_out);
/* n_partners and face_map, n_faces int32 each; each may be NULL. */
int immesh_self_intersect_faces(immesh_raycaster* rc, int32_t* n_partners /* n_faces */, int32_t* face_map_out /* n_faces */);
/* The Apply rule: the kept faces are compacted on the device and change places with the caster's face buffer, then the caster's own build. */
int immesh_self_intersect_apply(immesh_raycaster* rc);
/* Device time in milliseconds from HIP events on the caster's stream: [0] the candidates of the last pass (count, the read-back of the total, scan,
 * emit)  [1] its tests, the compaction and the sort of the hits (and the read-back of their number)  [2] the last apply (compaction and build). */
int immesh_self_intersect_last_timing(immesh_raycaster* rc, float ms[3]);

#ifdef __cplusplus
}
#endif
#endif
