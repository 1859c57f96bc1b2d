// Mesh depth rasterizer + LiDAR point reinforcement (include/immesh_render.h): device records and the launches render_host.cpp sequences.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

constexpr int RD_TILE = 16;          // tile edge in pixels: one 256-lane workgroup (four wave64) resolves one tile
constexpr int RD_BLOCK = 256;

// one face after setup: the contract's per-face values (include/immesh_render.h) and its candidate pixel box; 128 B
struct alignas(16) RdFace {
    double ab[3], bc[3], ca[3], n[3], na;
    int32_t u0, u1, v0, v1;          // candidate box, inclusive; u0 > u1: culled
    int32_t pad[2];
};
static_assert(sizeof(RdFace) == 128, "RdFace layout");

struct RdCam {                       // the camera as the kernels read it
    double rot[9], pos[3];
    double f, z_near, z_far;
    int32_t w, h, cx, cy;
    int32_t tiles_x, tiles_y;
};

size_t rd_scan_temp_bytes(int64_t n_faces, int n_tiles, int64_t n_pix);
// setup: per face -> rec[f], tile pairs of the face in cnt[f] (int64)
void rd_launch_setup(hipStream_t s, const RdCam& cam, const float* vtx, int64_t n_vtx, const int32_t* faces, int64_t n_faces, RdFace* rec, int64_t* cnt);
// foff[0] = 0, foff[f + 1] = pairs of faces 0..f
void rd_scan_pairs(hipStream_t s, void* temp, size_t temp_bytes, const int64_t* cnt, int64_t* foff, int64_t n_faces);
// pass 0: tile_cnt[t] += pairs of tile t;  pass 1: bins[tile_off[t] + k] = face (k from tile_fill)
void rd_launch_bin(hipStream_t s, const RdCam& cam, const RdFace* rec, const int64_t* foff, int64_t n_faces, int64_t n_pairs, int pass, int32_t* tile_cnt,
                   const int32_t* tile_off, int32_t* tile_fill, int32_t* bins);
void rd_scan_i32(hipStream_t s, void* temp, size_t temp_bytes, const int32_t* in, int32_t* out, int64_t n);
// per-tile resolve: depth[h*w] (float, -1 invalid), face[h*w] (-1 invalid)
void rd_launch_resolve(hipStream_t s, const RdCam& cam, const RdFace* rec, const int32_t* tile_cnt, const int32_t* tile_off, const int32_t* bins,
                       float* depth, int32_t* face);
// reinforce: unproject valid pixels, thin on the cell hash (res > 0), keep[i] = 1 for the kept pixels
void rd_launch_unproject(hipStream_t s, const RdCam& cam, float res, const float* depth, float* pts, float* cells, int32_t* keep);   // cells: rounded floats
void rd_launch_hash_insert(hipStream_t s, int64_t n_pix, const float* depth, const float* cells, int32_t* tab_rep, uint32_t* tab_min, uint32_t mask,
                           uint32_t* slot_of);
void rd_launch_hash_keep(hipStream_t s, int64_t n_pix, const float* depth, const uint32_t* tab_min, const uint32_t* slot_of, int32_t* keep);
// out[koff[i]] = pts[i] for kept pixels; n_out[0] = kept count
void rd_launch_compact(hipStream_t s, int64_t n_pix, const float* pts, const int32_t* keep, const int32_t* koff, float* out, int64_t* n_out);

// ---- the colour pass behind the rasterizer (include/immesh_shade.h; shade_kernels.hip)
struct RdShade {                     // the pass as the kernels read it
    int32_t source, axis, light, bgr, min_views;
    int32_t range_from_vertices;     // AXIS: lo / hi are decoded from the range keys instead of taken from here
    float lo, hi;
    uint32_t background;             // R | G << 8 | B << 16
};
// the colourer's state arrays as the vertex-colour kernel reads them (colour/colour.hpp's ClState, without its header)
struct RdColourState {
    const double* rgb[3];
    const double* first_exposure;
    const int32_t* n_obs;
};
// keys[0], keys[1] = order-preserving keys of the smallest and the largest coordinate `axis` over the vertices with three finite coordinates
// (0xFFFFFFFF / 0 when there is none), in two stages through part (2 * RD_SHADE_RANGE_PARTS words)
constexpr int RD_SHADE_RANGE_PARTS = 1024;
void rd_launch_shade_range(hipStream_t s, const float* vtx, int64_t n_vtx, int axis, uint32_t* part, uint32_t* keys);
// col[i] = R | G << 8 | B << 16 of vertex i (AXIS: Heat; VERTEX: bytes n_vtx x 3, or st when bytes is nullptr); range[0..1] = lo, hi as used
void rd_launch_shade_colours(hipStream_t s, const RdShade& sh, const float* vtx, int64_t n_vtx, const uint8_t* bytes, const RdColourState& st,
                             const uint32_t* keys, uint32_t* col, float* range);
// one lane per pixel in the resolve kernel's tiles: rgb[3 i] from face[i], rec[face], the face's indices and their colours (col: nullptr for WHITE)
void rd_launch_shade(hipStream_t s, const RdCam& cam, const RdShade& sh, const RdFace* rec, const int32_t* faces, const int32_t* face, const uint32_t* col,
                     uint8_t* rgb);
