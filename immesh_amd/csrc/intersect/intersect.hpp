// Self-intersections of the caster's snapshot (include/immesh_intersect.h): the launches intersect_host.cpp sequences (the caster's record of them,
// RcIntersect, is in raycast/raycast.hpp beside its other records).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../raycast/raycast.hpp"

// the pass' device counters (int64 each; zeroed before every pass)
enum {
    IX_N_TAKING = 0, IX_N_CANDIDATES, IX_N_SHARE0, IX_N_SHARE1, IX_N_SHARE2, IX_N_SHARE3, IX_N_PAIRS, IX_N_PAIRS_SHARE0, IX_N_PAIRS_SHARE1, IX_N_FACES_HIT,
    IX_MAX_PARTNERS,
    IX_COUNTERS = 16
};

// take[f] = 1 for a face that takes part (indices in [0, n_vtx), nine finite floats, three pairwise different indices); cnt[IX_N_TAKING]
void ix_launch_take(hipStream_t s, const float* vtx, int64_t n_vtx, const int32_t* faces, int64_t n_faces, int8_t* take, unsigned long long* cnt);
// The walk, one lane per face i: every leaf j > i that takes part and whose float box overlaps i's is a candidate.
//   keys == nullptr: cnt32[i] = min(the candidates of i, 2^31 - 1), cnt[IX_N_CANDIDATES] += the candidates of i
//   else:            keys[off[i] + k] = (i << 32) | j for the k-th candidate the same walk meets
void ix_launch_walk(hipStream_t s, const float* vtx, const int32_t* faces, int64_t n_faces, const int8_t* take, const RcNode* nodes, int64_t n_in, int32_t* cnt32,
                    const int32_t* off, unsigned long long* keys, unsigned long long* cnt);
// one lane per candidate: cmask[c] = the pair mask, flag[c] = mask != 0; cnt[IX_N_SHARE0 .. 3], [IX_N_PAIRS], [IX_N_PAIRS_SHARE0 / 1]
void ix_launch_test(hipStream_t s, const float* vtx, const int32_t* faces, const unsigned long long* keys, int64_t n_cand, uint8_t* cmask, int32_t* flag,
                    unsigned long long* cnt);
// after the scan of flag (hoff): hkey[hoff[c]] = (i << bits) | j, hval[hoff[c]] = the mask, for the candidates that intersect
void ix_launch_compact(hipStream_t s, const unsigned long long* keys, const uint8_t* cmask, const int32_t* flag, const int32_t* hoff, int64_t n_cand, int bits,
                       unsigned long long* hkey, int32_t* hval);
// one lane per sorted hit: pairs[2 h] = i, pairs[2 h + 1] = j, pmask[h], npart[i] += 1, npart[j] += 1 (npart zeroed by the caller)
void ix_launch_pairs(hipStream_t s, const unsigned long long* hkey, const int32_t* hval, int64_t n_hits, int bits, int32_t* pairs, uint8_t* pmask, int32_t* npart);
// per face: keep[f] = npart[f] == 0; cnt[IX_N_FACES_HIT], [IX_MAX_PARTNERS]
void ix_launch_keep(hipStream_t s, const int32_t* npart, int64_t n_faces, int32_t* keep, unsigned long long* cnt);
// after the scan of keep (koff): fmap[f] = koff[f] or -1; with faces_out != nullptr (the apply) faces_out[3 koff[f]] = the kept face
void ix_launch_map(hipStream_t s, const int32_t* faces, int64_t n_faces, const int32_t* keep, const int32_t* koff, int32_t* fmap, int32_t* faces_out);
