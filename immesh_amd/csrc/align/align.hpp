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
// res[0] = part[0 .. n_part) folded in index order by one workgroup, lane t taking t, t + 256, ... (zeros and zero counts for n_part == 0): the final
// fold of every step, of this rule and of the cloud rule
void al_launch_fold(hipStream_t s, const AlSystemDev* part, int64_t n_part, AlSystemDev* res);

// ---- the cloud rule (include/immesh_align.h, "Cloud rule"; align_cloud_kernels.hip, align_cloud_host.cpp): the target is the index's cloud ----------
// The fused step, its registers held to the walk's occupancy: per point the walk for the winner under (D, index), q = the winner minus p, the rows
// (mode 1 reads normal[3 j] and nstatus[j] of the winner j; a status other than 0 counts n_flat), the weight (huber > 0) and the fold -> part[b]; then
// al_launch_fold.  index_out / terms_out may each be nullptr.
void alc_launch_step(hipStream_t s, const RcFrame& fr, int has_frame, const float* pts, int64_t n_pts, double r2, int mode, const double* centre, double huber,
                     const float* cloud, const float* normal, const uint8_t* nstatus, const RcNode* nodes, int64_t n_in, AlSystemDev* part, AlSystemDev* res,
                     int32_t* index_out, double* terms_out);
// The split step, the same bits: the walk stores sindex[i] (-1 no neighbour, -2 not finite) and sq[3 i] (q), a second launch forms and folds.
void alc_launch_step_split(hipStream_t s, const RcFrame& fr, int has_frame, const float* pts, int64_t n_pts, double r2, int mode, const double* centre,
                           double huber, const float* cloud, const float* normal, const uint8_t* nstatus, const RcNode* nodes, int64_t n_in, int32_t* sindex,
                           double* sq, AlSystemDev* part, AlSystemDev* res, int32_t* index_out, double* terms_out);

// ---- what both rules' host sides share (align_host.cpp) ------------------------------------------------------------------------------------------------
struct immesh_align_options;
struct immesh_align_system;
struct immesh_align_result;
// the checks of the options a step reads, and of those the loop reads besides; of the loop's outputs.  `who` stands in front of every text.
int al_check_step(immesh_ctx* c, const char* who, const immesh_align_options* o);
int al_check_loop(immesh_ctx* c, const char* who, const immesh_align_options* o);
int al_check_loop_out(immesh_ctx* c, const char* who, const immesh_align_result* result_out, const double* history_out, int64_t history_cap);
bool al_nonneg_finite(double x);
void al_identity(RcFrame* fr);
// The Loop rule, once: from fr0, step(self, frame, system, ms) makes one step at a frame and reports its device time.  *total_ms = the steps' sum.
typedef int (*AlStepFn)(void* self, const RcFrame& fr, immesh_align_system* sys, float* ms);
int al_loop(const immesh_align_options& o, const RcFrame& fr0, AlStepFn step, void* self, float* total_ms, immesh_align_result* result_out,
            double* history_out, int64_t history_cap);
