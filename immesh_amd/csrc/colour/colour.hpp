// Vertex colours from camera images (include/immesh_colour.h): device records and the launches colour_host.cpp sequences.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

constexpr int CL_BLOCK = 256;

// the image and its pose as the kernels read them (the host computes tc, n, the availability bounds and allow once per image)
struct ClCam {
    double rot[9], tc[3], pos[3], n[3];
    double fx, fy, cx, cy;
    double u_lo, u_hi, v_lo, v_hi;     // m cols + 1, (1 - m) cols, m rows + 1, (1 - m) rows
    double inv_exposure, obs_time, min_depth, max_depth, max_pe, allow;
    int32_t rows, cols;
    int64_t stride;
};

// colour state, structure of arrays over cap vertices: a wavefront's loads and stores of one field are contiguous
struct ClState {
    double* rgb[3]; double* cov[3]; double* first_exposure; double* obs_dis; double* last_obs_time;
    int32_t* n_obs;
    int64_t cap;
};

// counters of one image in device memory; cl_launch_finalize turns them into an immesh_colour_stats
struct ClCounters {
    int32_t n_cand, n_sel;
    unsigned long long n_hit, n_first, n_updated, pe_count;
    unsigned long long dmin_key;       // order-preserving bit pattern of the smallest d_i (PLAIN)
    unsigned long long pad;
};

// a colourer's context and its state where it lies in device memory (colour_host.cpp), for the renderer's colour pass (include/immesh_shade.h): every
// colourer call returns with its stream synchronised, so between two calls the arrays are complete
struct immesh_colourer;
struct immesh_ctx;
immesh_ctx* cl_colourer_ctx(const immesh_colourer* c);
const ClState& cl_colourer_state(const immesh_colourer* c);

void cl_launch_state_init(hipStream_t s, const ClState& st);
// counters <- {n_cand, n_sel, 0 ..., key(3e8)}
void cl_launch_counters_init(hipStream_t s, ClCounters* cnt, int32_t n_cand, int32_t n_sel);
// RECENT sets: flags[id] = 1 for every vertex (heads = 0) or the smallest vertex id (heads = 1) of the voxels recent[0 .. *n_recent)
void cl_launch_mark_recent(hipStream_t s, const int32_t* recent, const int32_t* n_recent, const int32_t* vx_npts, const int32_t* vx_pts, int vox_cap, int n_vtx,
                           int heads, int32_t* flags);
// out[off[i]] = src ? src[i] : i where flags[i], i < n; *n_out = number of flags set
void cl_launch_compact(hipStream_t s, const int32_t* flags, const int32_t* off, const int32_t* src, int n, int32_t* out, int32_t* n_out);
// selection, pass 1: per candidate the gates, cell[i] (-1: out) and depth[i]; the cell's smallest (float)depth in tab_min
void cl_launch_select_min(hipStream_t s, const ClCam& cam, const float* v_pos, const int32_t* cand, int n_bound, const ClCounters* cnt, double md, int tab_w,
                          int64_t tab_n, int32_t* cell, double* depth, uint32_t* tab_min);
// pass 2: tab_hi = largest index with depth < (double)min, tab_lo = smallest index with (float)depth == min
void cl_launch_select_rank(hipStream_t s, int n_bound, const ClCounters* cnt, const int32_t* cell, const double* depth, const uint32_t* tab_min, int32_t* tab_hi,
                           uint32_t* tab_lo);
// pass 3: keep[i] = 1 for the holder of its cell
void cl_launch_select_keep(hipStream_t s, int n_bound, const ClCounters* cnt, const int32_t* cell, const int32_t* tab_hi, const uint32_t* tab_lo, int32_t* keep);
// PLAIN: dmin over the render set
void cl_launch_dmin(hipStream_t s, const ClCam& cam, const float* v_pos, const int32_t* sel, int n_bound, ClCounters* cnt);
// one lane per vertex of the render set: gates, projection, sampling, update_rgb; uv[2 i] = raw (u, v); partials[block] = the block's photometric error
// (cl_update_blocks(n_bound) of them)
void cl_launch_update(hipStream_t s, const ClCam& cam, int model, const float* v_pos, const int32_t* sel, int n_bound, ClCounters* cnt, const uint8_t* img,
                      const ClState& st, float* uv, double* partials);
int cl_update_blocks(int n_bound);
// stats (an immesh_colour_stats in device memory) from the counters and the partials, summed in block order
void cl_launch_finalize(hipStream_t s, int model, const ClCounters* cnt, const double* partials, int n_blocks, void* stats);
// fetch: out_rgb[3 i], out_state[i], i < n, for vertex ids[i] (ids == nullptr: first + i)
void cl_launch_gather(hipStream_t s, const ClState& st, const int32_t* ids, int64_t first, int64_t n, uint8_t* out_rgb, void* out_state);
