// The one-ring table, Taubin smoothing and vertex normals of the caster's snapshot (include/immesh_smooth.h): the launches smooth_host.cpp sequences
// (the caster's record of them, RcSmooth, is in raycast/raycast.hpp beside its other records).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../raycast/raycast.hpp"

// the pass' device counters (int64 each, SM_MAX_DISP2 the bits of a double that is not negative; zeroed before every pass)
enum {
    SM_N_USED = 0, SM_N_NOT_FINITE, SM_N_BORDER, SM_N_INTERIOR, SM_N_MOVING, SM_N_PAIRS, SM_MAX_VALENCE, SM_N_HELD, SM_N_MOVED, SM_MAX_DISP2, SM_N_ZERO,
    SM_COUNTERS = 16
};
// per vertex flags (int8): SM_FLAG_BORDER an endpoint of an edge with uses != 2, SM_FLAG_MOVING S(v) is not empty
enum { SM_FLAG_BORDER = 0, SM_FLAG_MOVING = 1, SM_FLAGS = 2 };

// The pair key of a directed edge is (u << 32) | v: row u, neighbour v.  A face that does not count emits six times the key (n_vtx << 32), above
// every real one, so the sort needs 32 + rc_index_bits(n_vtx + 1) bits and the rows end where that run begins.

// ---- the one-ring ----------------------------------------------------------------------------------------------------------------------------------------
// one lane per face: key[6 f .. 6 f + 5] = its six directed pairs, val[6 f + e] = 6 f + e (the sort's values; nothing reads them)
void sm_launch_emit(hipStream_t s, const int32_t* faces, int64_t n_faces, int64_t n_vtx, unsigned long long* key, int32_t* val);
// (the run heads of the sorted keys and, after their scan, rstart are raycast/pass_dev.hpp's run kernels: the length of run p is
// rstart[p + 1] - rstart[p] = uses of its edge: both directions are emitted per use.  rstart has n6 + 1 entries.)
// one lane per run whose row is a vertex: neighbours[p], uses[p], and flag[SM_FLAG_BORDER n_vtx + u] = 1 for the row u of an edge with uses != 2
// (every writer stores the same value; flag zeroed by the caller).  The order is already ascending by u, then v.
void sm_launch_entries(hipStream_t s, const unsigned long long* key, int64_t n6, int64_t n_vtx, const int32_t* head, const int32_t* scan, const int32_t* rstart,
                       int32_t* neighbours, int32_t* uses, int8_t* flag);
// one lane per vertex and one more: row_start[v] = the rank of the first sorted key >= (v << 32) (the position where u changes, found by bisection: no
// lane walks a run), vclass[v]; cnt[SM_N_USED], [SM_N_NOT_FINITE], [SM_N_BORDER], [SM_N_INTERIOR], [SM_MAX_VALENCE], [SM_N_PAIRS]
void sm_launch_rows(hipStream_t s, const float* vtx, int64_t n_vtx, const unsigned long long* key, int64_t n6, const int32_t* head, const int32_t* scan,
                    const int8_t* flag, long long* row_start, int8_t* vclass, unsigned long long* cnt);
// one lane per entry: sn[p] = the neighbour when it belongs to S(u) of its row u, else -1; flag[SM_FLAG_MOVING n_vtx + u] = 1 for a row with a member
void sm_launch_lists(hipStream_t s, const unsigned long long* key, int64_t n6, int64_t n_vtx, const int32_t* head, const int32_t* scan, const int32_t* rstart,
                     const int32_t* neighbours, const int32_t* uses, const int8_t* vclass, int border, int32_t* sn, int8_t* flag);
// ---- the steps -------------------------------------------------------------------------------------------------------------------------------------------
// one step: one lane per vertex walks its row of sn in order (three independent double sums); cnt[SM_N_HELD]
void sm_launch_step(hipStream_t s, const float* p_in, float* p_out, int64_t n_vtx, const long long* row_start, const int32_t* sn, int64_t n6, double w,
                    unsigned long long* cnt);
// one lane per vertex: cnt[SM_N_MOVING], [SM_N_MOVED], [SM_MAX_DISP2] from P_0 and P_n
void sm_launch_finish(hipStream_t s, const float* p0, const float* pn, int64_t n_vtx, const int8_t* flag, unsigned long long* cnt);
// ---- the normals -----------------------------------------------------------------------------------------------------------------------------------------
// one lane per face: key[3 f + e] = its e-th vertex when the face counts and its three vertices are finite, else n_vtx; val[3 f + e] = f
void sm_launch_incidence(hipStream_t s, const float* vtx, int64_t n_vtx, const int32_t* faces, int64_t n_faces, uint32_t* key, int32_t* val);
// after the stable sort by vertex (the faces of a vertex then ascend): one lane per vertex finds its run by bisection and walks it; cnt[SM_N_ZERO]
void sm_launch_normals(hipStream_t s, const float* vtx, int64_t n_vtx, const int32_t* faces, int64_t n_faces, const uint32_t* key, const int32_t* val,
                       float* normals, unsigned long long* cnt);
