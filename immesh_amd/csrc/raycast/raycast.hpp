// Ray casting at a triangle soup (include/immesh_raycast.h): the hierarchy's records and the launches raycast_host.cpp sequences.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <vector>
#include "rc_host.hpp"
#include "../../../include/immesh_closest.h"   // (and immesh_raycast.h): the frame and the distance statistics
#include "../../../include/immesh_topology.h"    // the stats the passes' records hold
#include "../../../include/immesh_simplify.h"
#include "../../../include/immesh_smooth.h"
#include "../../../include/immesh_intersect.h"

constexpr int RC_BLOCK = 256;
// The sort key of a face is (Morton code of its box centre, position among the faces that enter the tree): RC_CODE_BITS + RC_INDEX_BITS bits, all
// keys distinct.  Karras' construction gives every interior node a distinct common-prefix length on a root-to-leaf path, so a leaf has at most
// RC_CODE_BITS + RC_INDEX_BITS interior ancestors.  The traversal pushes at most one entry (the farther child) per interior node on its current
// path, so its stack never holds more than that many entries, whatever the soup (300 copies of one face, centres at 2^-k).
constexpr int RC_AXIS_BITS = 21;
constexpr int RC_CODE_BITS = 3 * RC_AXIS_BITS;
constexpr int RC_INDEX_BITS = 30;                 // at most 2^30 faces (checked by the host): positions differ in one of their low 30 bits
constexpr int RC_STACK = 96;
static_assert(RC_STACK >= RC_CODE_BITS + RC_INDEX_BITS, "the traversal stack must hold one entry per bit of the sort key");
static_assert(RC_CODE_BITS <= 63, "the code's top bit stays clear: clz of two distinct codes is >= 1");

// one interior node, 64 B: the float boxes of its two children (min / max of float coordinates: they contain their faces' float boxes exactly)
// and the children themselves -- >= 0: an interior node, < 0: ~child is a face index (a leaf holds one face)
struct alignas(16) RcNode {
    float lo[2][3], hi[2][3];
    int32_t child[2];
    int32_t parent;                               // (parent node << 1) | side; -1: the root (node 0)
    int32_t count;                                // refit: children that have arrived
};
static_assert(sizeof(RcNode) == 64, "RcNode layout");

struct RcFrame { double rot[9], pos[3]; };

// one partial of a distance query's reduction (closest face, nearest cloud point), and its folded result
struct DqStatsDev {
    double sum, sum2;
    int64_t n_face, n_not_finite, n_no_face;
    float max_dist;
    int32_t pad;
};
static_assert(sizeof(DqStatsDev) == 48, "DqStatsDev layout");
constexpr int DQ_LDS_BINS = 1024;

// the items of a build, one per leaf: the faces of a soup, or (faces == nullptr) the points of a cloud, xyz[3 i]: a point is a box whose lo == hi
struct RcLeaves {
    const float* xyz;
    int64_t n_vtx;
    const int32_t* faces;
};

// build -----------------------------------------------------------------------------------------------------------------------------------
// flag[i] = 1 when item i enters the tree: a face with its indices in range and nine finite coordinates, a point with three finite floats
void rc_launch_mark(hipStream_t s, const RcLeaves& src, int64_t n, int32_t* flag);
// ids[off[i]] = i for the marked items, box[6 j] = the float box (lo xyz, hi xyz) of ids[j]; bounds[6] (order-preserving keys, preset to
// 0xFFFFFFFF x 3, 0 x 3) = min / max over the boxes' centres;  n_in[0] = the number of marked items
void rc_launch_compact(hipStream_t s, const RcLeaves& src, int64_t n, const int32_t* flag, const int32_t* off, int32_t* ids, float* box, uint32_t* bounds,
                       int64_t* n_in);
// code[i] = the Morton code of box i's centre in the bounds, iota[i] = i (the sort's values)
void rc_launch_codes(hipStream_t s, const float* box, int64_t n_in, const uint32_t* bounds, unsigned long long* code, int32_t* iota);
// Karras' construction over the sorted codes (ties broken by position): nodes[0 .. n_in - 2], leaf_parent[i] = (node << 1) | side; sorted leaf i is
// item ids[pos_sorted[i]].  n_in >= 2.
void rc_launch_hierarchy(hipStream_t s, const unsigned long long* code, const int32_t* ids, const int32_t* pos_sorted, int64_t n_in, RcNode* nodes,
                         int32_t* leaf_parent);
// bottom-up refit, one lane per leaf, one counter per interior node
void rc_launch_refit(hipStream_t s, const float* box, const int32_t* pos_sorted, const int32_t* leaf_parent, int64_t n_in, RcNode* nodes);
// the tree of a single item: node 0 with that item as both children (a face tested twice gives the same fragment twice)
void rc_launch_single(hipStream_t s, const float* box, const int32_t* ids, RcNode* nodes);

// cast: t[i], face[i] per the contract (mode 0 NEAREST, 1 ANY); n_in == 0: every ray misses
void rc_launch_cast(hipStream_t s, const RcFrame& fr, const float* dirs, const float* origins, int64_t n_rays, double t_min, double t_max, int mode,
                    const float* vtx, const int32_t* faces, const RcNode* nodes, int64_t n_in, float* t, int32_t* face);
// reinforce: pts[3 i] of the hit rays (t[i] >= 0), cells when res > 0, keep[i] = res > 0 ? 0 : hit
void rc_launch_points(hipStream_t s, const RcFrame& fr, const float* dirs, const float* origins, int64_t n_rays, float res, const float* t, float* pts,
                      float* cells, int32_t* keep);

// ---- the host records: RcBuf, the shared checks, the end of a span and the thinning tail are rc_host.hpp's (the renderer and the colourer use them too)
// checks a frame (rc_finite_pose: "<who>: frame rotation / position is not finite") and copies it
int rc_frame(immesh_ctx* c, const char* who, const immesh_ray_frame* frame, RcFrame* fr);

// a hierarchy and the scratch of its build: the caster's over faces, the cloud index's over points
struct RcTree {
    RcBuf nodes;
    RcBuf flag, off, ids, box, bounds, code_a, code_b, pos_a, pos_b, leaf, temp;
    int64_t n_in = 0;                                          // leaves
};
// Builds t over the n items of src (already on the device, queued on s): mark, scan, compact, one host round trip for the count that sizes the tree
// (h_count, pinned), then codes, pair sort, Karras' construction and the refit, or the single-leaf tree.  ev0 / ev1 are recorded around the launches;
// s is idle on return.
int rc_tree_build(immesh_ctx* c, const char* who, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1, int64_t* h_count, RcTree& t, int64_t n, const RcLeaves& src);

// the results of a distance query (closest face, nearest cloud point) and their reduction
struct RcDist {
    RcBuf d2, dist, id, xyz, status;                           // the last query
    RcBuf part, hist, res;                                     // the reduction: per-workgroup partials, histogram, folded result
    DqStatsDev* h_res = nullptr;                               // pinned; allocated by the owner
    int64_t n = 0;
    bool have = false;
    ~RcDist() { if (h_res) (void)hipHostFree(h_res); }
};
// d2, dist, id, xyz of the last query to the host arrays that are not NULL (the stream is idle)
int rc_dist_copy(immesh_ctx* c, const RcDist& q, int64_t n, double* d2_out, float* dist_out, int32_t* id_out, float* xyz_out);
// the reduction behind immesh_closest_reduce and immesh_nearest_reduce: `who` prefixes the messages, `grow_who` those of rc_grow, `none` is the text
// when no query has been made; ev0 / ev1 are recorded around the launches and *ms is their span
int rc_dist_reduce(immesh_ctx* c, const char* who, const char* grow_who, const char* none, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1, float* ms,
                   RcDist& q, double bin_width, int32_t n_bins, immesh_closest_stats* stats, int64_t* hist_out);

// closest-point queries: allocated at the first query, never before
struct RcClosest {
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};   // query, reduction: begin / end
    RcDist q;                                                  // id: the face
    RcBuf pts, side;                                           // the last query's points; the side of the face
    float ms[2] = {0.0f, 0.0f};
    ~RcClosest() { rc_destroy_events(ev, 4); }
};

// one partial of an alignment step's fold, and the folded system (include/immesh_align.h): the 28 sums in the header's order, then n_used,
// n_not_finite, n_no_face, n_flat
struct AlSystemDev {
    double s[28];
    int64_t n[4];
};
static_assert(sizeof(AlSystemDev) == 256, "AlSystemDev layout");

// alignment of a cloud to the snapshot (include/immesh_align.h; align/align_host.cpp): allocated at the first step, never before.  Its buffers, events
// and pinned words are its own: the last closest query's results stay as they are across an alignment.
struct RcAlign {
    hipEvent_t ev[2] = {nullptr, nullptr};                     // a step: begin / end
    RcBuf pts, part, res;                                      // the cloud; per-workgroup partials; the folded system
    RcBuf face, terms;                                         // per point, only when asked for
    RcBuf sface, sq;                                           // the split variant's face and q per point
    AlSystemDev* h_res = nullptr;                              // pinned
    int variant = 0;                                           // 0 fused (registers capped), 1 split, 2 fused, not capped
    float ms[2] = {0.0f, 0.0f};
    ~RcAlign() {
        rc_destroy_events(ev, 2);
        if (h_res) (void)hipHostFree(h_res);
    }
};

// samples of the snapshot (include/immesh_nearest.h): allocated at the first immesh_mesh_sample, never before
struct RcSample {
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};   // counts, scan + emit: begin / end
    hipEvent_t done = nullptr;                                 // recorded behind the emit launch: a cloud index's stream waits on it
    RcBuf cnt, off, total, xyz, face;                          // k_f, its exclusive prefix sum, the int64 total; the last samples
    int64_t* h_total = nullptr;                                // pinned
    bool have = false;                                         // samples of the current snapshot exist
    int64_t n = 0;
    uint64_t gen = 0;                                          // counts the samplings: a query of the samples remembers which one it read
    float ms[2] = {0.0f, 0.0f};
    ~RcSample() {
        rc_destroy_events(ev, 4);
        rc_destroy_events(&done, 1);
        if (h_total) (void)hipHostFree(h_total);
    }
};

// What the seven passes over the snapshot share (analysis, orientation, holes, manifold, simplification, smoothing, self-intersections), and the four
// rules of the cloud index (neighbours, normals, clusters, alignment): the events of their spans, the device counters and their pinned copy, all created by
// rc_pass_ready at the pass' first call and never before, on the owner's context and stream; `have`: a result of the current snapshot (of the current
// analysis, for the orientation, the holes and the manifold pass; of the index's current cloud) exists.  rc_snapshot_changed / rc_analysis_changed and
// cx_cloud_changed / cx_normals_changed below clear it.
struct RcPass {
    hipEvent_t ev[10] = {};                                    // begin / end of up to five spans (the clusters call has five)
    unsigned long long* h_cnt = nullptr;                       // pinned: the counters, and what the pass asks for behind them
    RcBuf cnt;                                                 // n_cnt int64 (the pass' header names them)
    immesh_ctx* ctx = nullptr;                                 // the owner's context and stream
    hipStream_t s = nullptr;
    const char* who = "";                                      // the prefix of the pass' rc_grow messages
    int n_cnt = 0;
    bool have = false;
    float ms[4] = {0.0f, 0.0f, 0.0f, 0.0f};                    // the spans' device time, as the pass reports it
    ~RcPass() {
        rc_destroy_events(ev, 10);
        if (h_cnt) (void)hipHostFree(h_cnt);
    }
};

// the topology of the snapshot (include/immesh_topology.h; topology/topology_host.cpp): allocated at the first immesh_topology_analyse, never before
struct RcTopology : RcPass {                                   // spans: analyse, select; pinned [16] / [17]: the two words of n_counting
    RcBuf flag, off, used, parent, vparent, loop_cnt;          // per face / per vertex
    RcBuf key_a, key_b, val_a, val_b;                          // the half-edges; _b sorted (kept for the edge lists)
    RcBuf label, root, num, comp;                              // per face
    RcBuf first, nfaces, nbound, box;                          // per component (sized by the counting faces)
    RcBuf head, eid, start, pick, poff, uv, uses;              // edge lists
    RcBuf rank_a, rank_b, iota_a, iota_b, keepc, keep32, keep8, koff, out;   // select
    int64_t n_counting = 0, n_half = 0;
    immesh_topology_stats st = {};
};

// the orientation of the snapshot's manifold patches (include/immesh_topology.h; topology/orient_host.cpp): allocated at the first
// immesh_topology_orient, never before.  It reads the analysis' flag and sorted half-edges in RcTopology.
struct RcOrient : RcPass {                                     // spans: orient, apply
    RcBuf cover;                                               // the double cover's parents: node 2 f + s is face f with flip s
    RcBuf label, base, root, num, patch, flip, out;            // per face (base, flip: int8; out: the oriented faces)
    RcBuf tab;                                                 // per patch, OT_TABLES int32 arrays of n_counting entries each
    int64_t n_bound = 0;                                       // the tables' stride: the analysis' counting faces
    immesh_orient_stats st = {};
};

// the holes of the snapshot's boundary (include/immesh_topology.h, the Holes rule; topology/holes_host.cpp): allocated at the first
// immesh_topology_holes, never before.  It reads the analysis' sorted half-edges, vparent and loop_cnt in RcTopology.
struct RcHoles : RcPass {                                      // spans: holes, apply
    RcBuf vt, rk_a, rk_b;                                      // per vertex: HV_TABLES int32 arrays, the list ranking's two buffers
    RcBuf lt, box, cstart;                                     // per loop: HL_TABLES int32 arrays, the box keys, cycle_start as int64
    RcBuf cycle, cloop, new_faces, new_loop;                   // per boundary edge: the cycles' slots and their loops; the fans' faces and their loops
    RcBuf merged;                                              // the apply's faces ++ new_faces: it changes places with the caster's face buffer
    int64_t n_loops = 0;                                       // the tables' stride
    immesh_holes_stats st = {};
};

// one vertex per fan of faces (include/immesh_topology.h, the Manifold rule; topology/manifold_host.cpp): allocated at the first
// immesh_topology_manifold, never before.  It reads the analysis' flag and sorted half-edges in RcTopology.
struct RcManifold : RcPass {                                   // spans: manifold, apply; pinned [16] / [17]: the two words of n_fans
    RcBuf parent, root, isroot, off, ncnt, nlnk, fanof;        // per corner (3 n_faces)
    RcBuf key_a, key_b, val_a, val_b;                          // per fan: (vertex << 32) | root corner; _b sorted
    RcBuf fv, head, scan, ft, vsrc;                            // per fan: its vertex, the run heads of the vertices and their scan, MT_TABLES int32 arrays
    RcBuf start, nfans;                                        // per used vertex (and one more): its run of fans; per vertex: n_fans_out
    RcBuf vtx_out, faces_out, fan_out;                         // the result: the apply makes the first two change places with the caster's buffers
    int64_t n_fans = 0;                                        // the tables' stride
    immesh_manifold_stats st = {};
};

// weld and vertex clustering of the snapshot (include/immesh_simplify.h; simplify/simplify_host.cpp): allocated at the first immesh_simplify, never
// before.  It needs no analysis: it reads the caster's vertex and face buffers.
struct RcSimplify : RcPass {                                   // spans: simplify, apply
    RcBuf state, k64, k32, cnum, first, nmem, cstart, vmap;    // per vertex / per cluster (at most one cluster per vertex)
    RcBuf fk64, fk32, keep, koff, fstatus, fmap;               // per face
    RcBuf key_a, key_b, k32s, iota, val_a, val_b;              // the sorts' buffers, max(n_vtx, n_faces) entries: the vertices' first, then the faces'
    RcBuf vtx_out, faces_out;                                  // the result: the apply makes them change places with the caster's buffers
    immesh_simplify_stats st = {};
};

// the one-ring table, Taubin smoothing and vertex normals of the snapshot (include/immesh_smooth.h; smooth/smooth_host.cpp): allocated at the first
// immesh_smooth (the normals' incidence table at the first immesh_vertex_normals), never before.  It needs no analysis: it reads the caster's vertex
// and face buffers.
struct RcSmooth : RcPass {                                     // spans: one-ring and classes, steps, apply
    RcBuf key_a, key_b, val_a, val_b;                          // the directed pairs, 6 n_faces: _b sorted; _a holds the heads and their scan afterwards
    RcBuf rstart;                                              // per run of equal keys, and one more
    RcBuf neighbours, uses, sn;                                // per entry of the one-ring (at most 6 n_faces); sn: the neighbour, or -1 outside S(v)
    RcBuf row_start, vclass, flag;                             // per vertex: int64 (and one more), int8, SM_FLAGS int8 arrays
    RcBuf pos[2];                                              // the steps' two position buffers; pos[cur] is vtx_out
    RcBuf nkey_a, nkey_b, nval_a, nval_b, normals;             // the normals: (vertex, face) pairs, 3 n_faces; 3 floats per vertex
    int cur = 0;
    immesh_smooth_stats st = {};
};

// the self-intersections of the snapshot (include/immesh_intersect.h; intersect/intersect_host.cpp): allocated at the first immesh_self_intersect,
// never before.  It needs no analysis: it reads the caster's vertex and face buffers and its hierarchy.
struct RcIntersect : RcPass {                                  // spans: candidates, tests, apply
    RcBuf take, cnt32, off, npart, keep, koff, fmap;           // per face (take: int8)
    RcBuf key, cmask, flag, hoff;                              // per candidate: (i << 32) | j, the pair mask (uint8), mask != 0 and its scan
    RcBuf hkey_a, hkey_b, hval_a, hval_b, pairs, pmask;        // per hit: the sort's buffers (_b sorted), then i, j as int32 and the mask as uint8
    RcBuf faces_out;                                           // the apply's kept faces: they change places with the caster's face buffer
    immesh_intersect_stats st = {};
};

// the caster (include/immesh_raycast.h, include/immesh_closest.h): raycast_host.cpp owns it, closest_host.cpp adds its queries
struct immesh_raycaster {
    immesh_ctx* ctx = nullptr;
    hipStream_t s = nullptr;
    hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // build, cast, reinforce: begin / end
    int64_t* h_small = nullptr;   // pinned: [0] faces in the tree, [1] reinforced points
    RcBuf vtx, faces;                                                              // the built snapshot
    RcTree tree;                                                                   // (its temp also serves the reinforce pass and the sampler)
    RcBuf dirs[2], org[2], t[2], face[2];                                          // the last cast of each mode ([0] NEAREST: the reinforce pass reads it)
    RcThin th;                                                                     // reinforce
    bool built = false;
    int64_t n_vtx = 0, n_faces = 0;
    // the last NEAREST cast, as the reinforce pass reads it
    bool have_cast = false, have_origins = false;
    int64_t n_rays = 0;
    RcFrame frame = {};
    int64_t n_points = 0;
    float ms[3] = {0.0f, 0.0f, 0.0f};
    RcClosest cl;
    RcAlign al;
    RcSample sm;
    RcTopology tp;
    RcOrient ot;
    RcHoles hl;
    RcManifold mf;
    RcSimplify sp;
    RcSmooth so;
    RcIntersect ix;
};
// the hierarchy over r->vtx / r->faces (already on the device, queued on the caster's stream); it discards what belongs to the snapshot before
int rc_build(immesh_raycaster* r, int64_t n_vtx, int64_t n_faces);
// the discard rule (its table stands above them in raycast_host.cpp): what read the snapshot, and what read the analysis
void rc_snapshot_changed(immesh_raycaster* r);
void rc_analysis_changed(immesh_raycaster* r);
// the state an entry point needs, each refusal with the caller's name in front: a hierarchy has been built; that, and an analysis of the snapshot
// exists; p holds a result ("<who>: <none>" otherwise)
int rc_built(immesh_raycaster* r, const char* who);
int rc_analysed(immesh_raycaster* r, const char* who);
int rc_passed(immesh_raycaster* r, const char* who, const RcPass& p, const char* none);
// A pass on its owner's stream.  ready: the events and n_pinned pinned words if absent, the n_cnt device counters; the pass remembers c, s and `who`,
// which prefixes the messages of this and every later rc_pass_grow.  begin: ev[e0] recorded, the counters zeroed.  end: rc_span_end over ev[e0],
// ev[e1] and ms[span] with the counters [first, first + n) copied to h_cnt (n == 0: no copy).  span: an end without counters or error check (an
// apply).  ms: e0 .. e1 of recorded events.  counts: h_cnt[0 .. 3] to a caller's array that may be NULL.
int rc_pass_ready(immesh_ctx* c, hipStream_t s, const char* who, RcPass& p, int n_cnt, int n_pinned);
int rc_pass_grow(const RcPass& p, RcBuf& b, size_t bytes);
int rc_pass_begin(RcPass& p, int e0);
int rc_pass_end(RcPass& p, int e0, int e1, int span, int first, int n);
int rc_pass_span(RcPass& p, int e0, int e1, int span);
float rc_pass_ms(const RcPass& p, int e0, int e1);
void rc_pass_counts(const RcPass& p, int64_t counts[4]);

// closest face of every point (closest_kernels.hip) --------------------------------------------------------------------------------------------
// status[i]: 0 a face, 1 no face within max_dist, 2 the point is not finite.  has_frame == 0: the points are world coordinates.
void rc_launch_closest(hipStream_t s, const RcFrame& fr, int has_frame, const float* pts, int64_t n_pts, double r2, const float* vtx,
                       const int32_t* faces, const RcNode* nodes, int64_t n_in, double* d2, float* dist, int32_t* face, float* xyz, int8_t* side, uint8_t* status);
// part[b] = the partial of workgroup b (dq_stats_blocks(n_pts) of them), hist[0 .. n_bins) += the bins, hist[n_bins] += the overflow (hist zeroed by the
// caller; up to DQ_LDS_BINS bins are counted in LDS first);
// then res[0] = the partials folded in index order
int64_t dq_stats_blocks(int64_t n_pts);
void dq_launch_stats(hipStream_t s, const float* dist, const uint8_t* status, int64_t n_pts, float bin_width, int32_t n_bins, DqStatsDev* part,
                     unsigned long long* hist, DqStatsDev* res);

// ---- mesh-to-cloud distances (include/immesh_nearest.h): nearest_host.cpp owns the index and the sampler's host side ---------------------------------
// k nearest neighbours, radius counts, the outlier masks and their apply on a cloud index (knn_host.cpp): allocated at the first call of one of
// them, never before.  Its three flags stand for RcPass' one.
struct RcKnn : RcPass {                                        // spans: traversal, mask, apply; counters: the last mask's four counts
    RcBuf pts;                                                 // the last point-mode query's points
    RcBuf count, idx, d2;                                      // the last Neighbours query of either mode: counts, and the lists when asked for
    RcBuf mean, status;                                        // the last cloud-mode Neighbours query (the statistical rule reads them)
    RcBuf rcnt, rstatus;                                       // the last cloud-mode Count query (the radius rule reads them)
    RcBuf pstatus;                                             // a point-mode query's status (nothing reads it afterwards)
    RcBuf flag, keep8, off;                                    // the last mask as int32 and uint8 (cx_mask_begin / cx_mask_end), its scan
    RcBuf out, kept;                                           // the apply: out changes places with the index's cloud; kept: the old indices
    std::vector<double> h_mean;                                // the statistical rule's one read-back
    bool have_knn = false, have_count = false, have_mask = false;
    int64_t n_kept = 0;
};

// the Euclidean clusters of the index's cloud (include/immesh_nearest.h, the Clusters rule; clusters_host.cpp): allocated at the first
// immesh_cloud_clusters, never before.  Its counts are its own: the index's last Count query stays as it is.
constexpr int CL_ERROR = 4, CL_COUNTERS = 5, CL_PINNED = 8;   // device words: the four counts, the error flag; pinned: those, and [5], [6] the scan's total in two halves
struct RcClusters : RcPass {                                   // events: count, joins, border walk, numbering, table; spans: count, joins, border walk, the rest
    RcBuf count, status;                                       // the Count launch's outputs
    RcBuf core, kind;                                          // per point, uint8: the kind before the border walk (0 core, 2 finite and not core, 3 not finite), and after
    RcBuf parent, root, flag, num, label;                      // per point, int32: the union-find, the class' root (-1: none), root == self, its scan, the number
    RcBuf first, npts, ncore, boxkey, box;                     // per cluster: the table (boxkey: six order-preserving keys, box: their floats)
    RcBuf keepc;                                               // a select's per-cluster keep (int32)
    std::vector<int32_t> h_npts, h_keepc, h_rank;              // a select's one read-back, its answer, the ranking
    int64_t n_clusters = 0;
};

// the normals of the index's cloud and their agreement with a caster's face normals (include/immesh_normals.h; normals_host.cpp): allocated at the
// first call of one of them, never before.
struct RcNormals : RcPass {                                    // spans: normals, agreement, reduction; counters: the four counts of the last launch
    RcBuf normal, status;                                      // the last normals: 3 floats and a uint8 per cloud point (the agreement reads them)
    RcBuf curv, eig, count;                                    // the last normals call's other outputs
    RcBuf agree, face;                                         // the last agreement: s as a float; the cloud direction's closest face
    RcDist a;                                                  // the last agreement as the reduction reads it: dist = |s|, status 0 a pair / 1 none / 2 not finite
    int64_t n = 0;                                             // the cloud's size when the normals were made
};

// alignment of a cloud to the index's cloud (include/immesh_align.h, the Cloud rule; align/align_cloud_host.cpp): allocated at the first step, never
// before.  It keeps nothing that a later call reads: every call uploads its source cloud and answers from its own launches, so a change of the
// index's cloud has nothing of it to discard.
struct RcCloudAlign : RcPass {                                 // span: a step; ms[1]: the sum over the last loop; cnt / h_cnt: the folded system (32 words) and its pinned copy
    RcBuf pts, part;                                           // the source cloud; per-workgroup partials
    RcBuf index, terms;                                        // per point, only when asked for
    RcBuf sindex, sq;                                          // the split variant's winner and q per point
    int variant = 1;                                           // 0 fused (registers capped), 1 split: the default, by measurement
};

// An index over a point cloud: the caster's hierarchy with a point as a box whose lo == hi, built by the same rc_tree_build, one point per leaf.
struct immesh_cloud_index {
    immesh_ctx* ctx = nullptr;
    hipStream_t s = nullptr;
    hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};    // build, query, reduction: begin / end
    int64_t* h_small = nullptr;   // pinned: [0] points in the tree
    RcBuf pts;                                                                     // the built cloud
    RcTree tree;
    RcBuf q_pts;                                                                   // the last query's host-copied points
    RcDist q;                                                                      // id: the cloud point
    const immesh_raycaster* q_rc = nullptr;                                        // the last query read this caster's samples (nullptr: host points)
    uint64_t q_gen = 0;                                                            // ... of this sampling
    bool built = false;
    int64_t n_pts = 0;
    float ms[3] = {0.0f, 0.0f, 0.0f};
    RcKnn kn;
    RcNormals nr;
    RcClusters cl;
    RcCloudAlign ca;
};
// the index's discard rule (its table stands above them in raycast_host.cpp): what was made on the cloud, and what read the normals
void cx_cloud_changed(immesh_cloud_index* x);
void cx_normals_changed(immesh_cloud_index* x);
// the state an entry point needs: an index has been built; r is a caster of the index's context; it has a hierarchy and, when asked, samples
int cx_built(immesh_cloud_index* x, const char* who);
int cx_caster(immesh_cloud_index* x, const immesh_raycaster* r, const char* who);
int cx_caster_built(immesh_cloud_index* x, const immesh_raycaster* r, const char* who, bool sampled);
// rc_pass_ready for a rule of the index, on the index's stream with "cloud_index" in front of its messages
int cx_ready(immesh_cloud_index* x, RcPass& p, int n_cnt, int n_pinned);
// The index's last mask (knn_host.cpp): the two outlier rules and the clusters' select each launch their kernel between the two, writing *m.  begin:
// the record ready, the old mask gone, the buffers grown, the mask span begun with the four counts zeroed.  end: the span ended, n_kept and the mask
// valid, counts[] and keep_out (either may be NULL) filled.
struct CxMask {
    int32_t* flag;                                             // keep_i as the apply's scan reads it
    uint8_t* keep8;                                            // keep_i as it is fetched
    unsigned long long* cnt;                                   // the rule's four counts
};
int cx_mask_begin(immesh_cloud_index* x, CxMask* m);
int cx_mask_end(immesh_cloud_index* x, int64_t counts[4], uint8_t* keep_out);

// nearest cloud point of every query; status[i] as rc_launch_closest writes it (0 a neighbour, 1 none within max_dist, 2 the query is not finite), so
// dq_launch_stats reduces it.  n_in == 0 reads no node.  has_frame == 0: pts are world floats (the host's points, or the sampler's on the device).
void cn_launch_nearest(hipStream_t s, const RcFrame& fr, int has_frame, const float* pts, int64_t n, double r2, const float* cloud, const RcNode* nodes,
                       int64_t n_in, double* d2, float* dist, int32_t* index, float* xyz, uint8_t* status);
// the sampler: cnt[f] = min(k_f, 2^31 - 1), total[0] (zeroed by the caller) += k_f
void ms_launch_count(hipStream_t s, const float* vtx, int64_t n_vtx, const int32_t* faces, int64_t n_faces, double density, uint64_t seed, int32_t* cnt,
                     unsigned long long* total);
// sample s of n_samples (the total, below 2^31 - 1): sample s - off[f] of the face f it falls into by the offsets
void ms_launch_emit(hipStream_t s, const float* vtx, const int32_t* faces, int64_t n_faces, uint64_t seed, const int32_t* off, int64_t n_samples, float* xyz,
                    int32_t* face);

// ---- k nearest neighbours, radius counts, outlier masks and their apply (include/immesh_nearest.h, the Neighbours / Count / Outliers rules): knn_host.cpp
// the transfer lists of the last k-nearest query, n x k entries (not grown, and not written, when neither list is asked for)
// status[i]: 0 candidates, 1 finite but none within the distance, 2 the query is not finite.  mode 0: pts are world floats, 1: pts through fr,
// 2: cloud mode (query i is cloud point i, and index i is no candidate).  index / d2 may both be NULL (no list is stored); mean only in mode 2.
void kn_launch_knn(hipStream_t s, const RcFrame& fr, int mode, const float* pts, int64_t n, int32_t k, double r2, const float* cloud, const RcNode* nodes,
                   int64_t n_in, int32_t* count, int32_t* index, double* d2, double* mean, uint8_t* status);
void kn_launch_count(hipStream_t s, const RcFrame& fr, int mode, const float* pts, int64_t n, double r2, const float* cloud, const RcNode* nodes, int64_t n_in,
                     int32_t* count, uint8_t* status);
// the masks: flag[i] (int32, what the scan reads) = keep8[i] = keep_i; cnt[0 .. 3] (zeroed by the caller) += kept, outliers, isolated, not finite
void kn_launch_mask_statistical(hipStream_t s, const double* mean, const uint8_t* status, int64_t n, double threshold, int32_t* flag, uint8_t* keep8,
                                unsigned long long* cnt);
void kn_launch_mask_radius(hipStream_t s, const int32_t* count, const uint8_t* status, int64_t n, int32_t min_neighbours, int32_t* flag, uint8_t* keep8,
                           unsigned long long* cnt);
// the apply's compaction behind the exclusive scan of flag: out[off[i]] = pts[i], kept[off[i]] = i for the kept points (off[i] checked against n_kept)
void kn_launch_compact(hipStream_t s, const float* pts, const int32_t* flag, const int32_t* off, int64_t n, int64_t n_kept, float* out, int32_t* kept);

// ---- Euclidean clusters of the cloud (include/immesh_nearest.h, the Clusters rule): clusters_host.cpp; one lane per cloud point throughout
// core[i] = kind[i] = 3 not finite, 0 finite and count[i] >= min_neighbours (count == nullptr: every finite point), else 2; parent[i] = i, root[i] = -1
void cl_launch_kind(hipStream_t s, const float* cloud, int64_t n, const int32_t* count, int32_t min_neighbours, uint8_t* core, uint8_t* kind, int32_t* parent,
                    int32_t* root);
// the joins: every core lane walks with the bound r2 and unites itself with the core leaves of a lower index within r2; cnt[CL_ERROR] is raised when a
// union runs out of its steps
void cl_launch_join(hipStream_t s, const float* cloud, int64_t n, double r2, const RcNode* nodes, int64_t n_in, const uint8_t* core, int32_t* parent,
                    unsigned long long* cnt);
// root[i] = the root of core point i's class (its smallest index), flag[i] = core and root[i] == i
void cl_launch_flatten(hipStream_t s, int64_t n, const uint8_t* core, const int32_t* parent, int32_t* root, int32_t* flag);
// the lanes with core[i] == 2 walk for their best core leaf under (D, index): kind[i] = 1 and root[i] = that leaf's root, or kind[i] stays 2
void cl_launch_border(hipStream_t s, const float* cloud, int64_t n, double r2, const RcNode* nodes, int64_t n_in, const uint8_t* core, uint8_t* kind,
                      int32_t* root);
// first / npts / ncore / boxkey of n_clusters clusters preset; then, behind the exclusive scan num of flag: label[i] = num[root[i]] or -1, the table's
// integer folds, cnt[0 .. 3] += core, border, noise, not finite; then box = the keys' floats
void cl_launch_preset(hipStream_t s, int64_t n_clusters, int32_t* first, int32_t* npts, int32_t* ncore, uint32_t* boxkey);
void cl_launch_table(hipStream_t s, const float* cloud, int64_t n, const uint8_t* kind, const int32_t* root, const int32_t* num, int64_t n_clusters,
                     int32_t* label, int32_t* first, int32_t* npts, int32_t* ncore, uint32_t* boxkey, unsigned long long* cnt);
void cl_launch_unkey(hipStream_t s, int64_t n_clusters, const uint32_t* boxkey, float* box);
// the Select rule's mask from the per-cluster keep: flag[i] = keep8[i] = keep_i; cnt[0 .. 3] (zeroed by the caller) += kept, in a cluster and not kept,
// noise and not kept, not finite
void cl_launch_mask(hipStream_t s, int64_t n, const uint8_t* kind, const int32_t* label, const int32_t* keepc, int64_t n_clusters, int32_t keep_noise,
                    int32_t* flag, uint8_t* keep8, unsigned long long* cnt);

// ---- normals of the cloud and their agreement with face normals (include/immesh_normals.h, the Normals / Agreement rules): normals_host.cpp
// one cloud point per lane: normal[3 i], curv[i], eig[3 i], count[i], status[i] (0 a normal, 1 too few, 3 line-like, 2 not finite); cnt[0 .. 3] (zeroed
// by the caller) += with a normal, too few, line-like, not finite.  viewpoint == nullptr: the canonical sign alone.  No list is stored.
void nr_launch_normals(hipStream_t s, int64_t n, int32_t k, double r2, double min_ratio, const double* viewpoint, const float* cloud, const RcNode* nodes,
                       int64_t n_in, float* normal, double* curv, double* eig, int32_t* count, uint8_t* status, unsigned long long* cnt);
// agree[i] = (float)s or a quiet NaN, abs_agree[i] = |agree[i]| (-1 without a pair), status[i] = 0 a pair, 1 no pair, 2 the cloud point is not finite;
// cnt[0 .. 3] (zeroed by the caller) += pairs, opposed pairs, no pair, not finite.  Cloud direction: face[i] = the closest face of a point with a normal
void nr_launch_agree_cloud(hipStream_t s, const float* cloud, const float* normal, const uint8_t* nstatus, int64_t n, double r2, const float* vtx, int64_t n_vtx,
                           const int32_t* faces, int64_t n_faces, const RcNode* nodes, int64_t n_in, float* agree, float* abs_agree, int32_t* face,
                           uint8_t* status, unsigned long long* cnt);
// samples direction: sample j has face sface[j] and nearest cloud point index[j] (-1: none); index is checked against n_pts, sface against n_faces
void nr_launch_agree_samples(hipStream_t s, const int32_t* sface, const int32_t* index, int64_t n, const float* normal, const uint8_t* nstatus, int64_t n_pts,
                             const float* vtx, int64_t n_vtx, const int32_t* faces, int64_t n_faces, float* agree, float* abs_agree, uint8_t* status,
                             unsigned long long* cnt);
