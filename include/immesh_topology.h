/* immesh_topology.h -- the topology of a built ray caster's snapshot on the device: connected components, open edges, non-manifold and
 * inconsistently wound edges, boundary loops, the Euler characteristic, a filter that drops small fragments, one winding per manifold patch, the
 * boundary cycles in order with a fill of the small holes, and a split of every pinched vertex and fin (libimmesh_hip.so).
 *
 * Reference: none.  The reference writes its mesh to a PLY and leaves "remove isolated pieces" to a desktop tool; nothing pins this module but the
 * contract below and its checker (tests/topology_checker.py: np.unique on the edge keys, a plain union-find loop).
 * It answers the first questions asked of a reconstructed mesh -- how many pieces, how many holes, how much of it is manifold -- and it removes the
 * floating fragments of noise and moving objects before an accuracy figure is taken (tools/mesh_eval.py --min-component-faces).  It works on an
 * immesh_raycaster built by either build call of immesh_raycast.h and reads the snapshot's vertex and face buffers where they lie.
 *
 * A header of its own that includes immesh_raycast.h (which does not include it).
 *
 * ---- Contract (exact: integers, and min / max of floats; nothing depends on the order of lanes, atomics or launches) --------------------------
 * Everything is a function of the face array alone, plus the vertex floats for the boxes.
 *   Counting face:  a face counts when its three indices are pairwise different.  The others are n_degenerate, get component -1 and take part in
 *            nothing below.  Whether a vertex is finite plays no part: topology is a matter of indices, only the boxes look at coordinates (so a
 *            face that the caster's hierarchy leaves out for a NaN vertex still counts here).  Duplicate faces are NOT removed: a face given twice
 *            is two faces, and shows up as three edges with two more uses each.
 *   Edge:    face (i0, i1, i2) uses the undirected edges {i0, i1}, {i1, i2}, {i2, i0}; use k is FORWARD when i_k < i_(k+1 mod 3).
 *            uses(e) = the number of uses of e by counting faces; n_edges = the number of distinct edges.
 *            Boundary: uses == 1.  Interior: uses == 2.  Non-manifold: uses >= 3.
 *            Inconsistent: uses == 2 and both uses have the same direction (two faces wound alike traverse a shared edge in opposite directions).
 *            An inconsistent edge is also an interior edge: n_edges = n_boundary + n_interior + n_nonmanifold.
 *   Vertices: n_vertices_used = the number of distinct indices in counting faces;  euler = n_vertices_used - n_edges + n_counting.
 *   Component: two counting faces are adjacent when they use a common edge, whatever its uses; components are the classes of the transitive
 *            closure.  Sharing only a vertex does not join.  A component's LABEL is its smallest face index; components are numbered
 *            0 .. n_components - 1 by ascending label, and comp_out[f] is that number (-1 for a face that does not count).  Per component:
 *              first_face  the label
 *              n_faces     its counting faces
 *              n_boundary  the boundary edges of its faces
 *              box         lo x y z, hi x y z: per coordinate the smallest and the largest of the FINITE floats among the vertices of its faces;
 *                          +inf / -inf for a coordinate without one.  Compared as values: the sign of a zero is not part of the contract.
 *   Loops:   take the graph whose edges are the boundary edges.  n_boundary_loops = the number of its connected components, and
 *            largest_loop_edges = the most boundary edges in one of them (0 without a boundary edge).  Two loops that touch in a vertex are ONE:
 *            this counts connected pieces of the boundary, not cycles.
 *   Edge list: the edges of the asked kind in ascending order of (min index, max index): uv = (min, max), and uses.
 *            IMMESH_EDGE_INCONSISTENT lists the inconsistent edges (uses = 2); IMMESH_EDGE_BOUNDARY and IMMESH_EDGE_NONMANIFOLD as above.
 *   Select:  a component is kept when all of these hold:
 *              n_faces >= min_faces;
 *              min_diagonal == 0, or its box has a finite float in every coordinate and, with d_k = (double)hi_k - (double)lo_k,
 *              (d_x d_x + d_y d_y) + d_z d_z >= min_diagonal min_diagonal  (IEEE double, in the order written, no fused multiply-add);
 *              a component whose box lacks a coordinate fails when min_diagonal > 0;
 *              keep_largest == 0, or it is among the keep_largest components with the most faces (of ALL components, whatever the other two tests
 *              say), ties going to the smaller label.
 *            keep_out[f] = 1 for the faces of kept components, else 0 (also for faces that do not count).  faces_out = the kept faces with their
 *            original vertex indices, in face order; n_kept = their number.
 * Validated before any launch: a built caster; 3 n_faces <= 2^31 - 2 (the sort's int count and the half-edge id 3 f + k; stricter than the
 * caster's own limit); kind one of the three; min_faces >= 0, keep_largest >= 0, 0 <= min_diagonal finite; cap >= 0; an analysis of the current
 * snapshot before any fetch or select -- else IMMESH_E_INVAL with text in immesh_last_error(ctx).  A rebuild of the caster discards the analysis.
 * A caster with zero faces analyses to all zeros; that is not an error.
 * IMMESH_E_INTERNAL: a union did not finish within its proven bound of steps (a defect of the library, never of the input); the analysis is void.
 *
 * ---- Orientation (exact: integers, and per face the sign of one double expression; as order-free as the above) --------------------------------
 * immesh_topology_orient gives every manifold patch of the analysed snapshot one consistent winding; nothing reaches the caster before _apply.
 *   Patch:   two counting faces are patch-adjacent when they are the two users of an edge with uses == 2.  Edges with one use, or with three and
 *            more, join nothing: across a fan there is no "other side" to agree with.  Patches are the classes of the transitive closure (finer than
 *            the components).  A patch's LABEL is its smallest face index; patches are numbered 0 .. n_patches - 1 by ascending label, and
 *            patch_out[f] is that number (-1 for a face that does not count).
 *   Relation: the two users of such an edge AGREE when their uses have opposite directions (the edge is not inconsistent), else they DISAGREE.
 *   Orientable: a patch is orientable when a map base: its faces -> {0, 1} exists with base[label] = 0 and base[f] xor base[g] = disagree(f, g)
 *            for every patch-adjacent pair; the map is then unique.  Otherwise the patch is non-orientable (a Moebius band, a Klein bottle): its
 *            faces are never flipped, in any mode, and the stats and the tables report it.
 *   Mode:    decides per orientable patch whether the whole patch is inverted; then flip = base xor 1, else flip = base.
 *            IMMESH_ORIENT_FIRST     never: the label face keeps its winding.
 *            IMMESH_ORIENT_FEWEST    inverted when 2 #{base = 1} > n_faces: the fewest faces change; a tie keeps FIRST.
 *            IMMESH_ORIENT_VIEWPOINT a vote of the patch's faces about a viewpoint o (three doubles).  Per face, with its vertices widened to double,
 *                      a, b, c = v - o;  t = dot(cross(b - a, c - a), -a), cross and dot exactly as in immesh_raycast.h (IEEE double, in the order
 *                      written, no fused multiply-add);  s = +1 when t > 0, -1 when t < 0, else 0 -- also for a NaN t, for a face with a vertex
 *                      that is not finite, and for a face of zero area: the side rule of immesh_closest_points with p = o.  The face votes s when base = 0
 *                      and -s when base = 1 (its sign once wound like the label face).  The patch is inverted when strictly more faces vote -1
 *                      than +1; a tie keeps FIRST.  Afterwards the majority of a patch's faces show their front to the viewpoint.
 *   Per face: flip_out[f] = the final flip (0 for a face that does not count and for the faces of a non-orientable patch);  faces_out[f] = face f as
 *            (i0, i2, i1) when flipped, else unchanged: all n_faces faces in face order, the faces that do not count copied.
 *   Per patch: first_face (the label), n_faces, orientable (0 / 1), n_flipped (the final flips; 0 when non-orientable), n_inconsistent (the
 *            inconsistent edges between two of its faces, before orienting).
 *   Stats:   n_patches, n_orientable, n_nonorientable, largest_patch_faces, n_faces_flipped, n_faces_nonorientable, n_patches_inverted,
 *            n_inconsistent_before (the analysis' count), n_inconsistent_after (the sum of n_inconsistent over the non-orientable patches: 0 exactly
 *            when every patch is orientable; an analysis of faces_out counts exactly this many and is otherwise unchanged).
 *   Apply:   writes faces_out over the caster's face buffer on the device.  Afterwards the caster behaves in every call as one freshly built from the
 *            same vertices and faces_out by immesh_raycast_build_triangles: equal answers bit for bit, and everything a build discards is discarded
 *            (the last cast, the samples, the analysis, the orientation).  The hierarchy stays: boxes do not depend on winding.  A ray cast is
 *            bit-identical before and after.  side_out of immesh_closest_points negates exactly on a flipped winner; its closest point is the
 *            Face rule on (a, c, b), so d2 may differ in its last bits, and a point as near to two faces may change its winner.
 * Validated before any launch: an analysis of the current snapshot (the orientation reads its sorted half-edges); mode one of the three; with
 * VIEWPOINT a viewpoint of three finite doubles below 2^128 in magnitude; cap >= 0; an orientation of the current analysis before any fetch or apply
 * -- else IMMESH_E_INVAL with text in immesh_last_error(ctx).  A rebuild of the caster or a new analysis discards the orientation.  Zero faces orient
 * to all zeros; that is not an error.  IMMESH_E_INTERNAL as above; the orientation is void.
 *
 * ---- Holes (exact: integers, and min / max of floats for the boxes; as order-free as the above) -------------------------------------------------
 * immesh_topology_holes gives the ordered cycle of every simple boundary loop of the analysed snapshot and closes the small ones by a fan of new
 * faces over existing vertices; nothing reaches the caster before _apply.  The rules about counting faces and edges above apply unchanged.
 *   Boundary half-edge: the one use of an edge with uses == 1, directed as its face traverses it: use k of face (i0, i1, i2) goes from i_k (its
 *            TAIL) to i_(k+1 mod 3) (its HEAD).
 *   Loop:    a loop of the analysis: a connected piece of the graph of the boundary edges.  Its LABEL is its smallest vertex index; loops are numbered
 *            0 .. n_loops - 1 by ascending label, n_loops = the analysis' n_boundary_loops, and n_edges is the loop's number of boundary edges.
 *   Simple:  a vertex is simple when exactly one boundary half-edge leaves it and exactly one enters it; a loop is simple when all its vertices are,
 *            and is then one directed cycle.  Its CYCLE is v_0 = the label, v_(j+1) = the head of the half-edge that leaves v_j: n_edges vertices,
 *            n_edges >= 3.  Two holes that touch in a vertex, neighbours wound against each other and a boundary through a non-manifold vertex are
 *            not simple: such loops have no cycle and are never filled (orient and apply first: a consistently wound patch has directed borders).
 *   Box:     lo x y z, hi x y z per loop: per coordinate the smallest and the largest of the FINITE floats among its vertices, +inf / -inf for a
 *            coordinate without one -- the components' box rule.
 *   Status:  one per loop, the first that applies:
 *              IMMESH_HOLE_NONSIMPLE  the loop is not simple;
 *              IMMESH_HOLE_OUTLINE    its boundary half-edges all belong to one face (a 3-loop: a lone face's own outline, whose fill would be that
 *                                     face's mirror image);
 *              IMMESH_HOLE_TOO_LONG   n_edges > max_edges;
 *              IMMESH_HOLE_TOO_WIDE   max_diagonal > 0 and either the box lacks a finite float in a coordinate or, with
 *                                     d_k = (double)hi_k - (double)lo_k, (d_x d_x + d_y d_y) + d_z d_z > max_diagonal max_diagonal (IEEE double, in the
 *                                     order written, no fused multiply-add: Select's arithmetic with the inequality turned round);
 *              IMMESH_HOLE_BLOCKED    some chord {v_0, v_k}, 2 <= k <= n_edges - 2, is already an edge of the mesh, whatever its uses: the fan would
 *                                     make it non-manifold;
 *              IMMESH_HOLE_FILLED     (= 0) otherwise.
 *   Fill:    a filled loop of n edges gets the n - 2 faces (v_0, v_(k+1), v_k), k = 1 .. n - 2: each traverses its boundary edge against the existing
 *            use, so the fan is wound like its neighbours.  new_faces lists them loop by loop in loop order, k ascending; new_loop[j] is the loop
 *            number of new face j.  No vertex is added or moved.
 *   Invariant: with k filled loops of E boundary edges together, an analysis of faces ++ new_faces has n_boundary - E, n_boundary_loops - k,
 *            n_edges + E - 3 k, n_counting + E - 2 k, euler + k; n_nonmanifold, n_inconsistent and n_vertices_used unchanged; n_components not
 *            larger; and a second holes pass with the same limits fills nothing that the first one filled.
 *   Stats:   n_loops = n_simple + n_nonsimple; the simple ones are n_outline + n_too_long + n_too_wide + n_blocked + n_filled; n_new_faces;
 *            n_edges_closed (E); largest_simple_loop_edges; n_cycle_vertices = the sum of n_edges over the simple loops.
 *   Cycles:  cycle_out = the cycles of the simple loops concatenated in loop order; cycle_start[l] = the offset of loop l's cycle in it, -1 for a
 *            loop that is not simple.
 *   Apply:   afterwards the caster behaves in every call as one freshly built by immesh_raycast_build_triangles from the same vertices and
 *            faces ++ new_faces: equal answers bit for bit, and everything a build discards is discarded (the last cast, the samples, the analysis,
 *            the orientation, the holes).
 * Validated before any launch: an analysis of the current snapshot; n_vtx <= 2^31 - 1 (the scan over the vertices); max_edges >= 3;
 * 0 <= max_diagonal finite; cap >= 0; a holes pass of the current analysis before any fetch or apply; for the apply n_faces + n_new <= 2^30 and
 * 3 (n_faces + n_new) <= 2^31 - 2, so that the result can be analysed -- else IMMESH_E_INVAL with text in immesh_last_error(ctx).  A rebuild of the
 * caster, a new analysis or an orient-apply discards the holes pass.  Zero loops give all zeros; that is not an error.
 *
 * ---- Manifold (exact: integers, and bit copies of floats; as order-free as the above) -----------------------------------------------------------
 * immesh_topology_manifold gives every fan of faces round a vertex a vertex of its own: the step a desktop tool calls "split non-manifold
 * vertices".  It reads the analysis of the current snapshot; nothing reaches the caster before _apply.  The rules about counting faces, edges and
 * uses above apply unchanged.
 *   Corner:  corner 3 f + k is vertex i_k of counting face f.  A face that does not count has no corners.
 *   Link:    two corners at the same vertex v, in faces f and g, are linked when f and g are the two users of an edge with uses == 2 that has v as
 *            an endpoint.  The direction of the uses plays no part: the rule works on an unoriented mesh.  Edges with one use, or with three and
 *            more, link nothing (the patch rule of the Orientation).
 *   Fan:     the fans are the classes of the transitive closure of the links among the corners of one vertex.  A fan's LABEL is the smallest face
 *            index among its corners; n_corners is the number of its faces; n_links the number of linking edges between two of its corners.  A fan
 *            is CLOSED when n_links == n_corners, else OPEN.  Fans are numbered 0 .. n_fans - 1 by ascending (vertex, label).
 *   Output index: the fan of v with the smallest label keeps index v.  Every other fan gets a new index n_vtx + j, j counting the new vertices in
 *            fan order; vsrc[j] is the source vertex, and new vertex j is a bit copy of the three floats of vsrc[j], NaN payloads and the sign of a
 *            zero included.  vtx_out = vtx ++ the copies.  Unused vertices stay where they are.
 *   Faces:   faces_out holds all n_faces faces in face order, each corner replaced by its fan's output index; the faces that do not count are
 *            copied.  fan_out[3 f + k] is the fan number of the corner, or -1.
 *   Per vertex: n_fans_out[v] = the number of fans at v, 0 for an unused vertex.  A vertex is SINGULAR when it has 2 or more fans.
 *   Stats:   n_corners (3 n_counting), n_fans, n_vertices_used, n_singular_vertices, most_fans_at_vertex, n_new_vertices (n_fans -
 *            n_vertices_used), n_corners_moved (corners whose index changes), n_faces_changed (faces with such a corner), n_closed_fans,
 *            n_open_fans, largest_fan_corners, n_nonmanifold_before (the analysis' count).
 *   Guarantee: the output has no non-manifold edge and no singular vertex, for any input.  An output edge {a, b} is used by exactly the original
 *            users of {u, w} whose corners lie in fan a at u and in fan b at w.  Within a fan each corner has at most two links, one per edge of
 *            its face at the vertex, and a connected graph of degree at most 2 is a path or a cycle.  A corner whose face uses an edge {u, w} that
 *            is not interior has lost the link across that edge, so it is an end of a path, and a path has two ends: at most two users of any
 *            original edge share a fan at u, hence an output edge.  Original links survive as output edges with two uses (both ends of a linking
 *            edge keep their two users together), so the corners of an output vertex are still one class: every used output vertex has one fan.
 *   Invariant: an analysis of (vtx_out, faces_out) has n_nonmanifold == 0; n_counting and n_degenerate unchanged; n_vertices_used == n_fans;
 *            n_boundary + 2 n_interior == 3 n_counting; n_interior and n_components not smaller.  A second pass on that output has
 *            n_new_vertices == 0 and faces_out equal to its input.  When every patch of the output is orientable and its orientation is applied,
 *            every boundary loop is simple.
 *   Apply:   afterwards the caster behaves in every call as one freshly built by immesh_raycast_build_triangles from vtx_out and faces_out: equal
 *            answers bit for bit, and everything a build discards is discarded.  No host round trip of the mesh.
 * Validated before any launch: an analysis of the current snapshot; cap >= 0; a manifold pass of the current analysis before any fetch or apply;
 * for the apply n_vtx + n_new_vertices <= 2^31 - 1 -- else IMMESH_E_INVAL with text in immesh_last_error(ctx).  A rebuild of the caster, a new
 * analysis or any apply discards the result.  Zero faces give all zeros; that is not an error.  IMMESH_E_INTERNAL as above; the pass is void.
 */
#ifndef IMMESH_TOPOLOGY_H
#define IMMESH_TOPOLOGY_H
#include "immesh_raycast.h"
#ifdef __cplusplus
extern "C" {
#endif

#define IMMESH_E_INTERNAL (-8)

#define IMMESH_EDGE_BOUNDARY 0
#define IMMESH_EDGE_NONMANIFOLD 1
#define IMMESH_EDGE_INCONSISTENT 2

typedef struct immesh_topology_stats {
    int64_t n_faces;                  /* faces of the snapshot */
    int64_t n_counting;
    int64_t n_degenerate;             /* n_faces - n_counting */
    int64_t n_vertices_used;
    int64_t n_edges;
    int64_t n_boundary;
    int64_t n_interior;
    int64_t n_nonmanifold;
    int64_t n_inconsistent;
    int64_t n_components;
    int64_t largest_component_faces;
    int64_t n_boundary_loops;
    int64_t largest_loop_edges;
    int64_t euler;
} immesh_topology_stats;

/* Analyse the caster's snapshot; stats may be NULL.  Nothing is allocated or launched for this module before the first analysis; the buffers are
 * grow-only, as the caster's.  The analysis stays on the device for the calls below until the caster is rebuilt. */
int immesh_topology_analyse(immesh_raycaster* rc, immesh_topology_stats* stats);
/* comp_out[f], n_faces int32. */
int immesh_topology_faces(immesh_raycaster* rc, int32_t* comp_out /* n_faces */);
/* The component tables, n_components entries each (box: 6 floats per component).  Every pointer may be NULL; n_out gets n_components.  With any
 * array given, cap < n_components is IMMESH_E_CAPACITY (n_out is still set). */
int immesh_topology_components(immesh_raycaster* rc, int32_t* first_face, int32_t* n_faces, int32_t* n_boundary, float* box /* 6 per component */,
                               int64_t cap, int64_t* n_out);
/* The edges of one kind.  uv and uses may be NULL; n_out gets the count.  With an array given, cap < the count is IMMESH_E_CAPACITY. */
int immesh_topology_edges(immesh_raycaster* rc, int32_t kind, int32_t* uv /* 2 per edge */, int32_t* uses, int64_t cap, int64_t* n_out);
/* The Select rule.  keep_out and faces_out may be NULL; n_kept gets the number of kept faces.  With faces_out given, cap < n_kept is
 * IMMESH_E_CAPACITY (n_kept and keep_out are still set). */
int immesh_topology_select(immesh_raycaster* rc, int64_t min_faces, double min_diagonal, int64_t keep_largest, int8_t* keep_out /* n_faces */,
                           int32_t* faces_out /* 3 per kept face */, int64_t cap, int64_t* n_kept);
/* Device time in milliseconds from HIP events on the caster's stream: [0] the last analysis (every launch, and the one read-back of the count of
 * counting faces between them)  [1] the last select.  Copies of the results to the host are not included. */
int immesh_topology_last_timing(immesh_raycaster* rc, float ms[2]);   /* [0] analyse  [1] select */

#define IMMESH_ORIENT_FIRST 0
#define IMMESH_ORIENT_FEWEST 1
#define IMMESH_ORIENT_VIEWPOINT 2

typedef struct immesh_orient_stats {
    int64_t n_patches;
    int64_t n_orientable;
    int64_t n_nonorientable;
    int64_t largest_patch_faces;
    int64_t n_faces_flipped;
    int64_t n_faces_nonorientable;
    int64_t n_patches_inverted;
    int64_t n_inconsistent_before;    /* the analysis' n_inconsistent */
    int64_t n_inconsistent_after;     /* what an analysis of faces_out counts */
} immesh_orient_stats;

/* Orient the analysed snapshot by the Orientation rule; viewpoint is read with IMMESH_ORIENT_VIEWPOINT only (NULL otherwise); stats may be NULL.
 * Nothing is allocated or launched for the orientation before the first call; the buffers are grow-only.  The result stays on the device for the
 * calls below until the caster is rebuilt, analysed again or _apply has run.  No read-back lies between its launches. */
int immesh_topology_orient(immesh_raycaster* rc, int32_t mode, const double viewpoint[3], immesh_orient_stats* stats);
/* patch_out n_faces int32, flip_out n_faces int8, faces_out 3 n_faces int32; each may be NULL. */
int immesh_topology_orient_faces(immesh_raycaster* rc, int32_t* patch_out, int8_t* flip_out, int32_t* faces_out);
/* The patch tables, n_patches entries each.  Every pointer may be NULL; n_out gets n_patches.  With any array given, cap < n_patches is
 * IMMESH_E_CAPACITY (n_out is still set). */
int immesh_topology_orient_patches(immesh_raycaster* rc, int32_t* first_face, int32_t* n_faces, int32_t* orientable, int32_t* n_flipped,
                                   int32_t* n_inconsistent, int64_t cap, int64_t* n_out);
/* The Apply rule: one copy on the device, no host round trip. */
int immesh_topology_orient_apply(immesh_raycaster* rc);
/* Device time in milliseconds from HIP events on the caster's stream: [0] the last orient (every launch)  [1] the last apply. */
int immesh_topology_orient_last_timing(immesh_raycaster* rc, float ms[2]);   /* [0] orient  [1] apply */

#define IMMESH_HOLE_FILLED 0
#define IMMESH_HOLE_NONSIMPLE 1
#define IMMESH_HOLE_OUTLINE 2
#define IMMESH_HOLE_TOO_LONG 3
#define IMMESH_HOLE_TOO_WIDE 4
#define IMMESH_HOLE_BLOCKED 5

typedef struct immesh_holes_stats {
    int64_t n_loops;                  /* the analysis' n_boundary_loops */
    int64_t n_simple;
    int64_t n_nonsimple;
    int64_t n_outline;
    int64_t n_too_long;
    int64_t n_too_wide;
    int64_t n_blocked;
    int64_t n_filled;
    int64_t n_new_faces;
    int64_t n_edges_closed;           /* the boundary edges of the filled loops */
    int64_t largest_simple_loop_edges;
    int64_t n_cycle_vertices;         /* the sum of n_edges over the simple loops */
} immesh_holes_stats;

/* The Holes rule on the analysed snapshot; stats may be NULL.  Nothing is allocated or launched for the holes before the first call; the buffers are
 * grow-only.  The result stays on the device for the calls below until the caster is rebuilt, analysed again, or an apply (this one or the
 * orientation's) has run.  No read-back lies between its launches. */
int immesh_topology_holes(immesh_raycaster* rc, int64_t max_edges, double max_diagonal, immesh_holes_stats* stats);
/* The loop tables, n_loops entries each (box: 6 floats per loop).  Every pointer may be NULL; n_out gets n_loops.  With any array given,
 * cap < n_loops is IMMESH_E_CAPACITY (n_out is still set). */
int immesh_topology_holes_loops(immesh_raycaster* rc, int32_t* first_vertex, int32_t* n_edges, int32_t* status, float* box /* 6 per loop */,
                                int64_t* cycle_start, int64_t cap, int64_t* n_out);
/* The boundary cycles in order: n_cycle_vertices int32.  cycle_out may be NULL; n_out gets the count.  With it given, cap < the count is
 * IMMESH_E_CAPACITY. */
int immesh_topology_holes_cycles(immesh_raycaster* rc, int32_t* cycle_out, int64_t cap, int64_t* n_out);
/* The new faces: loop_out n_new_faces int32, faces_out 3 per new face; each may be NULL; n_out gets n_new_faces.  With an array given,
 * cap < n_new_faces is IMMESH_E_CAPACITY. */
int immesh_topology_holes_faces(immesh_raycaster* rc, int32_t* loop_out, int32_t* faces_out, int64_t cap, int64_t* n_out);
/* The Apply rule: the faces and the new faces side by side in one device buffer, then the caster's own build; no host round trip of the mesh. */
int immesh_topology_holes_apply(immesh_raycaster* rc);
/* Device time in milliseconds from HIP events on the caster's stream: [0] the last holes pass (every launch)  [1] the last apply (the copies and the
 * build of the hierarchy). */
int immesh_topology_holes_last_timing(immesh_raycaster* rc, float ms[2]);   /* [0] holes  [1] apply */

typedef struct immesh_manifold_stats {
    int64_t n_corners;                /* 3 n_counting */
    int64_t n_fans;
    int64_t n_vertices_used;
    int64_t n_singular_vertices;
    int64_t most_fans_at_vertex;
    int64_t n_new_vertices;           /* n_fans - n_vertices_used */
    int64_t n_corners_moved;
    int64_t n_faces_changed;
    int64_t n_closed_fans;
    int64_t n_open_fans;
    int64_t largest_fan_corners;
    int64_t n_nonmanifold_before;     /* the analysis' n_nonmanifold */
} immesh_manifold_stats;

/* The Manifold rule on the analysed snapshot; stats may be NULL.  Nothing is allocated or launched for the pass before the first call; the buffers
 * are grow-only.  The result stays on the device for the calls below until the caster is rebuilt, analysed again, or any apply has run.  One
 * read-back lies between its launches: the number of fans, which sizes the sort of their keys. */
int immesh_topology_manifold(immesh_raycaster* rc, immesh_manifold_stats* stats);
/* n_fans_out[v], n_vtx int32. */
int immesh_topology_manifold_vertices(immesh_raycaster* rc, int32_t* n_fans_out /* n_vtx */);
/* The fan tables, n_fans entries each.  Every pointer may be NULL; n_out gets n_fans.  With any array given, cap < n_fans is IMMESH_E_CAPACITY
 * (n_out is still set). */
int immesh_topology_manifold_fans(immesh_raycaster* rc, int32_t* vertex, int32_t* first_face, int32_t* n_corners, int32_t* n_links, int32_t* index_out,
                                  int64_t cap, int64_t* n_out);
/* fan_out and faces_out, 3 n_faces int32 each; each may be NULL. */
int immesh_topology_manifold_faces(immesh_raycaster* rc, int32_t* fan_out, int32_t* faces_out);
/* The new vertices: vsrc n_new_vertices int32, xyz 3 floats per new vertex; each may be NULL; n_out gets n_new_vertices.  With an array given,
 * cap < n_new_vertices is IMMESH_E_CAPACITY. */
int immesh_topology_manifold_new_vertices(immesh_raycaster* rc, int32_t* vsrc, float* xyz, int64_t cap, int64_t* n_out);
/* The Apply rule: vtx_out and faces_out change places with the caster's buffers, then the caster's own build; no host round trip of the mesh. */
int immesh_topology_manifold_apply(immesh_raycaster* rc);
/* Device time in milliseconds from HIP events on the caster's stream: [0] the last manifold pass (every launch, and the one read-back of the number
 * of fans between them)  [1] the last apply (the build of the hierarchy). */
int immesh_topology_manifold_last_timing(immesh_raycaster* rc, float ms[2]);   /* [0] manifold  [1] apply */

#ifdef __cplusplus
}
#endif
#endif
