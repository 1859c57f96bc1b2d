// Weld and vertex clustering of the caster's snapshot (include/immesh_simplify.h): the launches simplify_host.cpp sequences (the caster's record of
// them, RcSimplify, is in raycast/raycast.hpp beside its other records).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../raycast/raycast.hpp"

// the pass' device counters (int64 each; zeroed before every pass)
enum {
    SP_N_USED = 0, SP_N_ALONE_NOT_FINITE, SP_N_ALONE_OUTSIDE, SP_N_CLUSTERS, SP_LARGEST, SP_N_NOT_COUNTING, SP_N_COLLAPSED, SP_N_DUPLICATE, SP_N_FACES_OUT,
    SP_COUNTERS = 16
};
// state[v]: what a vertex is to the clustering.  Only SP_NORMAL vertices share a cluster; the two ALONE kinds are clusters of one.
enum { SP_UNUSED = 0, SP_NORMAL, SP_ALONE_NOT_FINITE, SP_ALONE_OUTSIDE };
// the key of a vertex that is not SP_NORMAL: above every key a SP_NORMAL vertex can have (bit 63 is clear in a cell key; the top word of a weld key is
// the order-preserving key of a finite float, which 0xFFFFFFFF is not), so the stable sort puts them behind the runs and never between two members
constexpr unsigned long long SP_KEY_APART = 0xFFFFFFFFFFFFFFFFull;

// state[v] = SP_NORMAL for the vertices of counting faces (three pairwise different indices in [0, n_vtx)); state zeroed by the caller
void sp_launch_mark(hipStream_t s, const int32_t* faces, int64_t n_faces, int64_t n_vtx, int32_t* state);
// per vertex: the final state, the cluster key k64[v] (cell > 0: the three q_k + 2^20 in 21 bits each; cell == 0: the order-preserving keys of x and
// y, -0 folded onto +0) and k32[v] (cell == 0: the key of z; else 0), iota[v] = v; cnt[SP_N_USED], [SP_N_ALONE_NOT_FINITE], [SP_N_ALONE_OUTSIDE]
void sp_launch_keys(hipStream_t s, const float* vtx, int64_t n_vtx, double cell, int32_t* state, unsigned long long* k64, uint32_t* k32, int32_t* iota,
                    unsigned long long* cnt);
// out[i] = k64[idx[i]]: the high word in the order the first of two stable passes left
void sp_launch_gather64(hipStream_t s, const unsigned long long* k64, const int32_t* idx, int64_t n, unsigned long long* out);
// one lane per sorted position: head[i] = 1 where a run begins (a vertex that is not SP_NORMAL is a run of its own)
void sp_launch_heads(hipStream_t s, const int32_t* sv, int64_t n_vtx, const int32_t* state, const unsigned long long* k64, const uint32_t* k32, int32_t* head);
// after the scan of head (run r = scan[i] + head[i] - 1): rstart[r] = the head's position, rend[r] = one past the run's last
void sp_launch_runs(hipStream_t s, int64_t n_vtx, const int32_t* head, const int32_t* scan, int32_t* rstart, int32_t* rend);
// lab[v] = the label of v's run (the head's vertex: the sort is stable over ascending indices), islab[v] = 1 for the label of a used vertex's run
void sp_launch_labels(hipStream_t s, const int32_t* sv, int64_t n_vtx, const int32_t* state, const int32_t* head, const int32_t* scan, const int32_t* rstart,
                      int32_t* lab, int32_t* islab);
// after the scan of islab (cnum): one lane per sorted position, the heads of used runs fill their cluster's tables: first[c], nmem[c], cstart[c] (the
// run's first position) and vtx_out[3 c] = the label's floats; cnt[SP_N_CLUSTERS], [SP_LARGEST]
void sp_launch_clusters(hipStream_t s, const float* vtx, const int32_t* sv, int64_t n_vtx, const int32_t* state, const int32_t* head, const int32_t* scan,
                        const int32_t* rend, const int32_t* cnum, int32_t* first, int32_t* nmem, int32_t* cstart, float* vtx_out, unsigned long long* cnt);
// IMMESH_SIMPLIFY_MEAN: one lane per cluster (cnt[SP_N_CLUSTERS] of the n_vtx lanes at work) of two members and more sums its run in order
void sp_launch_mean(hipStream_t s, const float* vtx, const int32_t* sv, int64_t n_vtx, const int32_t* nmem, const int32_t* cstart, const unsigned long long* cnt,
                    float* vtx_out);
// vmap[v] = cnum[lab[v]] (-1: unused)
void sp_launch_vmap(hipStream_t s, int64_t n_vtx, const int32_t* state, const int32_t* lab, const int32_t* cnum, int32_t* vmap);
// per face: fstatus (NOT_COUNTING, COLLAPSED or KEPT for now), keep[f]; with keys != nullptr the sorted new triple a < b < c as f64[f] = (a << 32) | b,
// f32[f] = c (SP_KEY_APART / 0xFFFFFFFF for a face that is not kept), iota[f] = f; cnt[SP_N_NOT_COUNTING], [SP_N_COLLAPSED]
void sp_launch_faces(hipStream_t s, const int32_t* faces, int64_t n_faces, int64_t n_vtx, const int32_t* vmap, int8_t* fstatus, int32_t* keep,
                     unsigned long long* f64, uint32_t* f32, int32_t* iota, unsigned long long* cnt);
// one lane per sorted position: a kept face whose predecessor is kept and has the same triple becomes DUPLICATE; cnt[SP_N_DUPLICATE]
void sp_launch_duplicates(hipStream_t s, const int32_t* sf, int64_t n_faces, const unsigned long long* f64, const uint32_t* f32, int8_t* fstatus, int32_t* keep,
                          unsigned long long* cnt);
// after the scan of keep (koff): faces_out[3 koff[f]] = the mapped triple of a kept face, fmap[f] = koff[f] (-1); cnt[SP_N_FACES_OUT]
void sp_launch_compact(hipStream_t s, const int32_t* faces, int64_t n_faces, const int32_t* vmap, const int32_t* keep, const int32_t* koff, int32_t* faces_out,
                       int32_t* fmap, unsigned long long* cnt);
