// Alignment of a cloud to the caster's snapshot (include/immesh_align.h): the launches align_host.cpp sequences.
#pragma once
#include "../raycast/raycast.hpp"

constexpr int AL_TERMS = 28;

// workgroups of a step over n_pts points (one lane per point); 0 for no point
int64_t al_blocks(int64_t n_pts);
// The fused step: per point the walk, the terms and the fold over the workgroup -> part[b] for workgroup b; then res[0] = the partials folded in
// index order by one workgroup (zeros and zero counts for no point).  face_out / terms_out may each be nullptr: then nothing is stored per point.
// capped: the kernel whose registers are held to the walk's occupancy (the default; the same bits either way).
void al_launch_step(hipStream_t s, bool capped, const RcFrame& fr, int has_frame, const float* pts, int64_t n_pts, double r2, int mode, const double* centre,
                    const float* vtx, const int32_t* faces, const RcNode* nodes, int64_t n_in, AlSystemDev* part, AlSystemDev* res, int32_t* face_out,
                    double* terms_out);
// The split step, the same bits: the walk stores sface[i] (-1 no face, -2 not finite) and sq[3 i] (the winner's q), a second launch loads the
// winner again, forms the terms and folds them.
void al_launch_step_split(hipStream_t s, const RcFrame& fr, int has_frame, const float* pts, int64_t n_pts, double r2, int mode, const double* centre,
                          const float* vtx, const int32_t* faces, const RcNode* nodes, int64_t n_in, int32_t* sface, double* sq, AlSystemDev* part,
                          AlSystemDev* res, int32_t* face_out, double* terms_out);
