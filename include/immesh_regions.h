/* immesh_regions.h -- the renderer's region buckets, kept on the device (libimmesh_hip.so).
 *
 * Reference: Triangle_manager files every triangle into a 10 m cube ("region"), one Sync_triangle_set with a "needs synchronising" flag each,
 * and the renderer thread turns the flagged buckets into float vertex buffers:
 *   src/meshing/r3live/triangle.cpp:3-10, 35-70     get_triangle_center, insert_triangle_to_list, erase_triangle_from_list
 *   src/meshing/r3live/triangle.hpp:40-113          Sync_triangle_set (m_if_required_synchronized, get_triangle_set(.., reset_status))
 *   src/meshing/r3live/triangle.hpp:121-123         m_triangle_set_vector (creation order), m_triangle_set_in_region
 *   src/meshing/mesh_rec_display.cpp:78-103         unparse_triangle_set_to_vector
 *   src/meshing/mesh_rec_display.cpp:139-156, 220-260   synchronize_triangle_list_for_disp, service_refresh_and_synchronize_triangle
 * Here the device keeps the region table, marks regions as mesh jobs are committed, and on request hands out the buckets that changed since
 * the last refresh, each as a ready vertex buffer.  A viewer needs no per-triangle host structure.
 *
 * These declarations live in a header of their own (not immesh_c_api.h): the C++ oracle mirrors immesh_c_api.h one-to-one, while the checker of
 * this part is a restatement of the contract below (tests/region_checker.py), pinned to the reference's own Triangle_manager.
 *
 * ---- Contract (exact; S = immesh_config::mesh_region) ------------------------------------------------------------------------------------------
 *   Key:    of a triangle with sorted vertex ids (i0 < i1 < i2) and RAW vertex positions p (the floats of the vertex store widened to double,
 *           RGB_pts::get_pos() without the smooth flag): c = ((p[i0] + p[i1]) + p[i2]) / 3.0 per component in IEEE double, no fused multiply-add;
 *           key = ((int32)std::round(c.x / S), (int32)std::round(c.y / S), (int32)std::round(c.z / S)), std::round = half away from zero.
 *           Vertex positions never change, so a triangle's key is fixed for the life of the map.  |key| must stay below 2^20.
 *   Table:  a region exists from the first insertion of a triangle with its key; index = position in m_triangle_set_vector = creation order.
 *           A mesh job commits all its removals, then its insertions in the order of the sorted add list: the new regions of a job are numbered
 *           by the first add-list position at which their key appears.  Erasing creates no region; an emptied region stays, with 0 triangles.
 *   Dirty:  set at creation, by every insertion into the region and by every removal from it; not by flip updates nor by smoothed positions.
 *           Cleared only by a synchronisation that takes the region.
 *   Sync:   takes the dirty regions (every region, empty ones included, with force_all = g_force_refresh_triangle) in index order; per region its
 *           live triangles in lexicographic order of the sorted triplet (the reference iterates a pointer-ordered std::set: unspecified), each as
 *           the triplet, its m_index_flip byte and the display positions of ids [0], [1], [2] of the SORTED triplet (the flip is not applied to
 *           the order) -- nine floats, bit for bit what immesh_mesh_display_vertices returns for those ids with the same
 *           (smooth_factor, knn, maximum_smooth_dis).
 *
 * Threading: immesh_mesh_regions, _sync, _fetch, immesh_region_keys and immesh_mesh_regions_error may be called from a thread of their own beside
 * immesh_process_scan(.., IMMESH_MESH_ASYNC) and the collector, like immesh_smooth_pts.  They see the map between two mesh jobs, and they never
 * touch immesh_last_error's string: their error text is kept apart and returned by immesh_mesh_regions_error.
 */
#ifndef IMMESH_REGIONS_H
#define IMMESH_REGIONS_H
#include "immesh_c_api.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct immesh_region_info {   /* 32 bytes */
    int32_t key[3];        /* round(centroid / mesh_region) (triangle.cpp:37-40) */
    int32_t index;         /* position in m_triangle_set_vector: creation order, stable (triangle.cpp:47) */
    int32_t n_triangles;   /* live triangles in the bucket (Sync_triangle_set::get_triangle_set_size) */
    int32_t dirty;         /* m_if_required_synchronized (immesh_mesh_regions: now; sync results: the flag the sync found -- 0 only when force_all took the region) */
    int64_t first;         /* sync results: offset of the bucket's first triangle in the fetched arrays; immesh_mesh_regions: 0 */
} immesh_region_info;

/* Switches the region table on (1) before the first mesh job of the context and allocates its device state (counted by immesh_device_bytes).
 * After the first job: IMMESH_E_INVAL (creation order could not be the reference's any more).  Off (the default) nothing of this header is
 * allocated or launched.  A sharded mesher (shard_world > 1 with shard_mesh) is refused.  At most 65536 regions (IMMESH_E_CAPACITY from the mesh job). */
int immesh_mesh_regions_enable(immesh_ctx* ctx, int32_t on);
/* The whole table in index order (m_triangle_set_vector), flags untouched.  out == NULL queries the count; cap < count: IMMESH_E_CAPACITY. */
int immesh_mesh_regions(immesh_ctx* ctx, immesh_region_info* out, int32_t cap, int32_t* n_out);
/* synchronize_triangle_list_for_disp (mesh_rec_display.cpp:139-156) + unparse_triangle_set_to_vector (:78-103) for every taken region: snapshots the
 * dirty regions (all when force_all), clears their flags and builds their buffers on the device, where they stay until the next sync.  knn must
 * be 20; maximum_smooth_dis as immesh_smooth_pts.  A region changed by a job that starts after the snapshot stays dirty. */
int immesh_mesh_regions_sync(immesh_ctx* ctx, double smooth_factor, int32_t knn, double maximum_smooth_dis, int32_t force_all,
                             int32_t* n_regions_out, int64_t* n_triangles_out);
/* Results of the last sync: regions (n_regions), tri (n x 3 sorted triplets), flip (n), xyz (n x 9 floats); any pointer may be NULL. */
int immesh_mesh_regions_fetch(immesh_ctx* ctx, immesh_region_info* regions, int32_t* tri, uint8_t* flip, float* xyz);
/* The key rule on the device for caller-supplied triangles (host arrays; vertex ids in any order, used as given: pass sorted triplets for
 * the contract's sum order): what a host mirror needs to partition a scan's lists by bucket.  Works with the table off. */
int immesh_region_keys(immesh_ctx* ctx, const float* vtx_xyz, int64_t n_vtx, const int32_t* tri, int64_t n_tri, int32_t* keys_out /* n_tri x 3 */);
/* Error text of the context's last failed call of this header ("" when none); the pointer stays valid until the calling thread asks again. */
const char* immesh_mesh_regions_error(immesh_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif
