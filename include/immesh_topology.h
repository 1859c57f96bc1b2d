/* immesh_topology.h -- the topology of a built ray caster's snapshot on the device: connected components, open edges, non-manifold and
 * inconsistently wound edges, boundary loops, the Euler characteristic, and a filter that drops small fragments (libimmesh_hip.so).
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

#ifdef __cplusplus
}
#endif
#endif
