// Mesh topology of the caster's snapshot (include/immesh_topology.h): the launches topology_host.cpp sequences (the caster's record of them, RcTopology, is in
// raycast/raycast.hpp beside its other records).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstring>
#include "../raycast/raycast.hpp"

// the analysis' device counters (int64 each; zeroed before every analysis)
enum {
    TP_N_EDGES = 0, TP_N_BOUNDARY, TP_N_INTERIOR, TP_N_NONMANIFOLD, TP_N_INCONSISTENT, TP_N_VERTICES, TP_N_COMPONENTS, TP_LARGEST_COMPONENT, TP_N_LOOPS,
    TP_LARGEST_LOOP, TP_ERROR, TP_N_KEPT, TP_COUNTERS = 16
};

// box keys: rc_compact_kernel's order-preserving keys.  Only finite floats are entered, so the presets stay apart from every key.
constexpr uint32_t TP_KEY_NONE_LO = 0xFFFFFFFFu, TP_KEY_NONE_HI = 0u;
inline float tp_unkey_host(uint32_t k, bool lo) {
    uint32_t u;
    if (k == (lo ? TP_KEY_NONE_LO : TP_KEY_NONE_HI)) u = lo ? 0x7F800000u : 0xFF800000u;   // no finite float: +inf / -inf
    else u = (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k;
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}
// box[6 i] = the floats of n boxes' keys on the device (lo xyz, hi xyz): the components' and the loops' (topology_host.cpp)
int tp_fetch_boxes(immesh_ctx* c, float* box, const RcBuf& keys, int64_t n);

// analyse ---------------------------------------------------------------------------------------------------------------------------------
// flag[f] = 1 for a counting face (three pairwise different indices in [0, n_vtx)), parent[f] = f, used[v] = 1 for its vertices (used zeroed by the caller)
void tp_launch_mark(hipStream_t s, const int32_t* faces, int64_t n_faces, int64_t n_vtx, int32_t* flag, int32_t* parent, int32_t* used);
// vparent[v] = v, loop_cnt[v] = 0, cnt[TP_N_VERTICES] += the used vertices
void tp_launch_vertices(hipStream_t s, int64_t n_vtx, const int32_t* used, int32_t* vparent, int32_t* loop_cnt, unsigned long long* cnt);
// counting face f, the off[f]-th: key[3 off[f] + k] = (min << 32) | max of use k, val[...] = 3 f + k
void tp_launch_emit(hipStream_t s, const int32_t* faces, int64_t n_faces, const int32_t* flag, const int32_t* off, unsigned long long* key, int32_t* val);
// one lane per sorted half-edge: run heads classify their edge (cnt[TP_N_EDGES .. TP_N_INCONSISTENT], one atomic per wavefront and counter) and
// join a boundary edge's vertices in vparent; every other lane joins its face to its predecessor's in parent.  cnt[TP_ERROR] != 0: a union ran out
// of its step bound.
void tp_launch_classify(hipStream_t s, const unsigned long long* key, const int32_t* val, int64_t n_half, const int32_t* faces, int32_t* parent,
                        int32_t* vparent, unsigned long long* cnt);
// label[f] = the root of f (-1: not counting), root[f] = 1 when f is a root
void tp_launch_flatten(hipStream_t s, const int32_t* parent, const int32_t* flag, int64_t n_faces, int32_t* label, int32_t* root);
// the component tables before they are filled, n_bound entries: nfaces = nbound = 0, box keys = 0xFFFFFFFF x 3 (lo), 0 x 3 (hi)
void tp_launch_preset(hipStream_t s, int64_t n_bound, int32_t* nfaces, int32_t* nbound, uint32_t* box);
// comp[f] = num[label[f]] (-1: not counting); first[c], nfaces[c], box keys (all preset) of the components; cnt[TP_N_COMPONENTS]
void tp_launch_components(hipStream_t s, const float* vtx, int64_t n_vtx, const int32_t* faces, int64_t n_faces, const int32_t* label, const int32_t* root,
                          const int32_t* num, int32_t* comp, int32_t* first, int32_t* nfaces, uint32_t* box, unsigned long long* cnt);
// the boundary heads again: nbound[comp] (preset), the loops' edge counts in loop_cnt[root vertex], cnt[TP_N_LOOPS], cnt[TP_LARGEST_LOOP]
void tp_launch_boundary(hipStream_t s, const unsigned long long* key, const int32_t* val, int64_t n_half, const int32_t* comp, const int32_t* vparent,
                        int32_t* nbound, int32_t* loop_cnt, unsigned long long* cnt);
// cnt[TP_LARGEST_COMPONENT] = the largest nfaces[c]
void tp_launch_largest(hipStream_t s, const int32_t* root, const int32_t* num, const int32_t* nfaces, int64_t n_faces, unsigned long long* cnt);

// edge lists ------------------------------------------------------------------------------------------------------------------------------
// (head[i] = 1 for a run head of the sorted keys, start[e] = the position of edge e's head, start[n_edges] = n_half: raycast/pass_dev.hpp's run kernels)
// pick[e] = 1 when edge e is of `kind`
void tp_launch_pick(hipStream_t s, const int32_t* start, int64_t n_edges, const int32_t* val, const int32_t* faces, int32_t kind, int32_t* pick);
// the picked edges, in order: uv[2 j], uses[j]
void tp_launch_edges(hipStream_t s, const int32_t* start, int64_t n_edges, const unsigned long long* key, const int32_t* pick, const int32_t* off,
                     int32_t* uv, int32_t* uses);

// orient (orient_kernels.hip) -------------------------------------------------------------------------------------------------------------
// the orientation's device counters (int64 each; zeroed before every orientation)
enum {
    OT_N_PATCHES = 0, OT_N_ORIENTABLE, OT_N_NONORIENTABLE, OT_LARGEST_PATCH, OT_N_FLIPPED, OT_N_FACES_NONORIENTABLE, OT_N_INVERTED, OT_INCONSISTENT_AFTER,
    OT_ERROR, OT_COUNTERS = 16
};
// the per-patch tables: int32 arrays of n_bound entries each in one buffer (zeroed before every orientation), tab + k * n_bound.  The first five are
// what immesh_topology_orient_patches returns; the others feed the decision.
enum { OT_FIRST = 0, OT_NFACES, OT_ORIENTABLE, OT_NFLIPPED, OT_NINCONSISTENT, OT_NBASE1, OT_VOTE_PLUS, OT_VOTE_MINUS, OT_INVERT, OT_TABLES };
// cover[i] = i for the 2 n_faces nodes of the double cover
void ot_launch_init(hipStream_t s, int64_t n_nodes, int32_t* cover);
// one lane per sorted half-edge: the head of a run of exactly two, users f and g, d = both uses have one direction, joins 2 f with 2 g + d and
// 2 f + 1 with 2 g + 1 - d.  cnt[OT_ERROR] != 0: a union ran out of its step bound.
void ot_launch_link(hipStream_t s, const unsigned long long* key, const int32_t* val, int64_t n_half, const int32_t* faces, int32_t* cover,
                    unsigned long long* cnt);
// r = the root of 2 f: label[f] = r >> 1 (-1: not counting); base[f] = 2 for a face of a non-orientable patch (2 f and 2 f + 1 have one root), else
// r & 1; root[f] = 1 when f is its patch's label
void ot_launch_flatten(hipStream_t s, const int32_t* cover, const int32_t* flag, int64_t n_faces, int32_t* label, int8_t* base, int32_t* root);
// patch[f] = num[label[f]] (-1); the tables OT_FIRST, OT_ORIENTABLE, OT_NFACES, OT_NBASE1 and, in mode 2, the votes about the viewpoint o;
// cnt[OT_N_PATCHES]
void ot_launch_patches(hipStream_t s, const float* vtx, const int32_t* faces, int64_t n_faces, const int32_t* label, const int8_t* base, const int32_t* root,
                       const int32_t* num, int32_t mode, const double* o, int32_t* patch, int32_t* tab, int64_t n_bound, unsigned long long* cnt);
// the heads of runs of two again, now that the patches are numbered: OT_NINCONSISTENT
void ot_launch_inconsistent(hipStream_t s, const unsigned long long* key, const int32_t* val, int64_t n_half, const int32_t* faces, const int32_t* patch,
                            int32_t* tab, int64_t n_bound);
// one lane per patch, n_patches read from cnt[OT_N_PATCHES] on the device: OT_INVERT and OT_NFLIPPED by the mode, and the counters of the stats
void ot_launch_decide(hipStream_t s, int64_t n_bound, int32_t mode, int32_t* tab, unsigned long long* cnt);
// flip[f] and faces_out[3 f]: (i0, i2, i1) when flipped
void ot_launch_flip(hipStream_t s, const int32_t* faces, int64_t n_faces, const int32_t* patch, const int8_t* base, const int32_t* tab, int64_t n_bound,
                    int8_t* flip, int32_t* faces_out);

// holes (holes_kernels.hip) ---------------------------------------------------------------------------------------------------------------
// the holes pass' device counters (int64 each; zeroed before every pass)
enum {
    HC_N_SIMPLE = 0, HC_N_NONSIMPLE, HC_N_OUTLINE, HC_N_TOO_LONG, HC_N_TOO_WIDE, HC_N_BLOCKED, HC_N_FILLED, HC_N_NEW, HC_N_CLOSED, HC_LARGEST_SIMPLE,
    HC_N_CYCLE, HC_COUNTERS = 16
};
// the per-vertex tables: int32 arrays of n_vtx entries each in one buffer, vt + k * n_vtx.  HV_LAB the loop's label (the root of the analysis'
// vparent), HV_IN / HV_OUT the boundary half-edges that enter / leave, HV_SUCC / HV_LFACE the head and the face of one that leaves (read where
// HV_OUT is 1), HV_BAD[label] the loop is not simple, HV_ROOT the vertex is a loop's label, HV_NUM its exclusive prefix sum
enum { HV_LAB = 0, HV_IN, HV_OUT, HV_SUCC, HV_LFACE, HV_BAD, HV_ROOT, HV_NUM, HV_TABLES };
// the per-loop tables: int32 arrays of n_loops entries each in one buffer, lt + k * n_loops.  The first three are what immesh_topology_holes_loops
// returns.  HL_SLEN n_edges of a simple loop, else 0, HL_CSTART its exclusive prefix sum; HL_FILL the new faces of a filled loop, HL_FOFF its sum
enum { HL_FIRST = 0, HL_NEDGES, HL_STATUS, HL_SLEN, HL_CSTART, HL_BLOCKED, HL_FILL, HL_FOFF, HL_TABLES };
// one entry of the list ranking: the next vertex on the broken cycle (-1: none) and the distance to it
struct HlRank { int32_t nxt, d; };
// HV_LAB by a walk up vparent (the analysis is finished: plain loads), HV_IN = HV_OUT = HV_BAD = 0, HV_SUCC = HV_LFACE = -1
void hl_launch_init(hipStream_t s, int64_t n_vtx, const int32_t* vparent, int32_t* vt);
// one lane per sorted half-edge: the head of a run of one, tail t to head h in its face's direction: HV_OUT[t] and HV_IN[h] by integer atomics,
// HV_SUCC[t] = h and HV_LFACE[t] plain stores
void hl_launch_degrees(hipStream_t s, const unsigned long long* key, const int32_t* val, int64_t n_half, const int32_t* faces, int64_t n_vtx, int32_t* vt);
// HV_BAD[label] = 1 where a boundary vertex is not simple (every writer stores the same value), HV_ROOT
void hl_launch_flags(hipStream_t s, int64_t n_vtx, int32_t* vt);
// after the scan of HV_ROOT.  Per vertex of a simple loop: the ranking's start, the cycle broken at its label (the vertex whose successor is the label
// ends the list).  Per label: HL_FIRST, HL_NEDGES (the analysis' loop_cnt), HL_SLEN, HL_BLOCKED = 0, the box keys preset, and HL_STATUS =
// NONSIMPLE, OUTLINE (a 3-loop whose three leaving faces are one) or FILLED for now
void hl_launch_rank_init(hipStream_t s, int64_t n_vtx, const int32_t* vt, const int32_t* loop_cnt, int64_t n_loops, int32_t* lt, uint32_t* box, HlRank* rk);
// one round of pointer jumping from `in` to `out`: d += d[nxt], nxt = nxt[nxt]; a round reads only what an earlier launch wrote
void hl_launch_jump(hipStream_t s, int64_t n_vtx, const HlRank* in, HlRank* out);
// the box keys of the loops from their vertices, folded per wavefront and loop first
void hl_launch_boxes(hipStream_t s, const float* vtx, int64_t n_vtx, const int32_t* vt, int64_t n_loops, uint32_t* box);
// after the scan of HL_SLEN: cycle[HL_CSTART[l] + n_edges - 1 - d] = v and cloop[...] = l for the vertices of the simple loops (n_room entries each)
void hl_launch_scatter(hipStream_t s, int64_t n_vtx, const int32_t* vt, const HlRank* rk, const int32_t* lt, int64_t n_loops, int32_t* cycle, int32_t* cloop,
                       int64_t n_room);
// one lane per loop: TOO_LONG and TOO_WIDE where nothing earlier applies; cstart64[l] (-1: not simple); cnt[HC_N_CYCLE]
void hl_launch_limits(hipStream_t s, int64_t n_loops, int32_t* lt, const uint32_t* box, int64_t max_edges, double max_diagonal, int64_t* cstart64,
                      unsigned long long* cnt);
// one lane per cycle slot (n_room lanes, cnt[HC_N_CYCLE] of them at work): slot k of a loop still FILLED, 2 <= k <= n_edges - 2, looks its chord
// {v_0, v_k} up in the sorted keys by binary search; found: HL_BLOCKED[l] = 1
void hl_launch_chords(hipStream_t s, int64_t n_room, const unsigned long long* cnt, const int32_t* cycle, const int32_t* cloop, const unsigned long long* key,
                      int64_t n_half, int32_t* lt, int64_t n_loops);
// one lane per loop: the final HL_STATUS, HL_FILL, and the counters of the stats
void hl_launch_decide(hipStream_t s, int64_t n_loops, int32_t* lt, unsigned long long* cnt);
// after the scan of HL_FILL, one lane per cycle slot: slot k of a filled loop, 1 <= k <= n_edges - 2, writes new face HL_FOFF[l] + k - 1 =
// (v_0, v_(k+1), v_k) and its loop (n_room faces of room); cnt[HC_N_NEW]
void hl_launch_emit(hipStream_t s, int64_t n_room, const int32_t* cycle, const int32_t* cloop, const int32_t* lt, int64_t n_loops, int32_t* new_faces,
                    int32_t* new_loop, unsigned long long* cnt);

// manifold (manifold_kernels.hip) ---------------------------------------------------------------------------------------------------------
// the manifold pass' device counters (int64 each; zeroed before every pass)
enum {
    MF_N_SINGULAR = 0, MF_MOST_FANS, MF_N_MOVED, MF_N_CHANGED, MF_N_CLOSED, MF_N_OPEN, MF_LARGEST_FAN, MF_ERROR, MF_COUNTERS = 16
};
// the per-fan tables: int32 arrays of n_fans entries each in one buffer, ft + k * n_fans: what immesh_topology_manifold_fans returns
enum { MT_VERTEX = 0, MT_FIRST, MT_NCORNERS, MT_NLINKS, MT_INDEX, MT_TABLES };
// parent[c] = c, ncnt[c] = nlnk[c] = 0 for the n3 = 3 n_faces corners
void mf_launch_init(hipStream_t s, int64_t n3, int32_t* parent, int32_t* ncnt, int32_t* nlnk);
// one lane per sorted half-edge: the head of a run of exactly two joins its users' corners at the edge's smaller vertex, and those at its larger
// one.  cnt[MF_ERROR] != 0: a union ran out of its step bound.
void mf_launch_link(hipStream_t s, const unsigned long long* key, const int32_t* val, int64_t n_half, const int32_t* faces, int32_t* parent,
                    unsigned long long* cnt);
// root[c] = the root of corner c (-1: its face does not count), isroot[c], ncnt[root] += 1
void mf_launch_flatten(hipStream_t s, const int32_t* parent, const int32_t* flag, int64_t n3, int32_t* root, int32_t* isroot, int32_t* ncnt);
// the heads of runs of two again: nlnk[root] += 1 at either end
void mf_launch_links(hipStream_t s, const unsigned long long* key, const int32_t* val, int64_t n_half, const int32_t* faces, const int32_t* root,
                     int32_t* nlnk);
// after the scan of isroot: key[off[c]] = (vertex << 32) | c and val[off[c]] = c for the roots (n_room entries of room)
void mf_launch_keys(hipStream_t s, const int32_t* faces, const int32_t* isroot, const int32_t* off, int64_t n3, unsigned long long* key, int32_t* val,
                    int64_t n_room);
// sorted key j is fan j: fv[j] = its vertex, fanof[its root corner] = j
void mf_launch_fans(hipStream_t s, const unsigned long long* key, int64_t n_fans, int64_t n3, int32_t* fv, int32_t* fanof);
// after the run heads of fv and their scan: the tables; a fan that is no head is new vertex m = j - scan[j]: vsrc[m], and the three words of
// its source in vtx_out[3 (n_vtx + m)] (n_new of room); cnt[MF_N_CLOSED], [MF_N_OPEN], [MF_LARGEST_FAN]
void mf_launch_table(hipStream_t s, int64_t n_fans, const unsigned long long* key, const int32_t* head, const int32_t* scan, const int32_t* ncnt,
                     const int32_t* nlnk, const float* vtx, int64_t n_vtx, int64_t n_new, int32_t* ft, int32_t* vsrc, float* vtx_out, unsigned long long* cnt);
// one lane per run of fv (start: n_runs + 1 entries): nfans_out[vertex] = the run's length (zeroed by the caller); cnt[MF_N_SINGULAR], [MF_MOST_FANS]
void mf_launch_vertices(hipStream_t s, int64_t n_runs, const int32_t* start, const int32_t* fv, int64_t n_fans, int64_t n_vtx, int32_t* nfans_out,
                        unsigned long long* cnt);
// faces_out[3 f + k] = the output index of the corner's fan, fan_out[3 f + k] its number; a face that does not count is copied, with -1;
// cnt[MF_N_MOVED], [MF_N_CHANGED]
void mf_launch_emit(hipStream_t s, const int32_t* faces, int64_t n_faces, const int32_t* flag, const int32_t* root, const int32_t* fanof, const int32_t* ft,
                    int64_t n_fans, int32_t* faces_out, int32_t* fan_out, unsigned long long* cnt);

// select ----------------------------------------------------------------------------------------------------------------------------------
// rank_key[c] = ((2^31 - 1 - nfaces[c]) << 32) | c, iota[c] = c
void tp_launch_rank_keys(hipStream_t s, const int32_t* nfaces, int64_t n_comp, unsigned long long* rank_key, int32_t* iota);
// keepc[c] by the Select rule, one lane per rank i: c = sorted[i], the components by rank (nullptr when keep_largest == 0: c = i)
void tp_launch_decide(hipStream_t s, const int32_t* nfaces, const uint32_t* box, int64_t n_comp, int64_t min_faces, double min_diagonal,
                      int64_t keep_largest, const int32_t* sorted, int32_t* keepc);
// keep32[f] / keep8[f] = the face's component is kept
void tp_launch_mask(hipStream_t s, const int32_t* comp, const int32_t* keepc, int64_t n_faces, int32_t* keep32, int8_t* keep8);
// faces_out[3 off[f]] = face f for the kept faces; cnt[TP_N_KEPT] = their number
void tp_launch_compact(hipStream_t s, const int32_t* faces, const int32_t* keep32, const int32_t* off, int64_t n_faces, int32_t* faces_out,
                       unsigned long long* cnt);
