// Region buckets of the renderer on the device (include/immesh_regions.h): device state, the launches regions_host.cpp sequences, and the hook
// the mesher's phase B calls.  Only the kernels of this directory take RegionsDev: MeshDev (passed by value to every mesher kernel) is untouched.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <mutex>
#include <string>
#include <vector>
#include "../../../include/immesh_regions.h"

constexpr int RG_CAP_REGIONS = 1 << 16;      // regions a context can hold (10 m cubes: 65 km^2 of ground); more: IMMESH_E_CAPACITY from the mesh job
constexpr int RG_HASH_CAP = 1 << 18;         // open-addressing table, load <= 1/4
constexpr int RG_KEY_BIAS = 1 << 20;         // |key| < 2^20 per axis (packed 3 x 21 bits, as the mesh-voxel keys)
constexpr int RG_OVERFLOW_CODE = 15;         // value left in the job's SC_OVERFLOW slot (mesh_overflow's table)

// key == ~0: empty.  val: region index, -1 from the slot's creation until regions_order_kernel numbers it.  first: lowest add-list position of the
// job that created it (0xFFFFFFFF before the first atomicMin) -- a 0xFF fill is the empty table.
struct RgEnt { unsigned long long key; int32_t val; uint32_t first; };
static_assert(sizeof(RgEnt) == 16, "one round trip per lookup");

enum { RG_N = 0, RG_NEW, RG_SEL_REGIONS, RG_SEL_TRIS, RG_BAD, RG_NLIST, RG_COUNTERS = 8 };

struct RegionsDev {
    RgEnt* ent;               // [RG_HASH_CAP]
    int32_t* r_key;           // [RG_CAP_REGIONS][3]
    int32_t* r_nlive;         // live triangles per region
    int32_t* r_dirty;         // m_if_required_synchronized
    int32_t* t_region;        // [cap_tris] region of every triangle-pool entry, -1 until its first insertion (pool entries persist after erase)
    int32_t* new_slots;       // [RG_CAP_REGIONS] hash slots created by the running job
    int32_t* cnt;             // [RG_COUNTERS]: regions, created by the running job, last sync's regions / triangles, consistency flag, voxel-list length
    // sync scratch
    int32_t* sel_rank;        // [RG_CAP_REGIONS] rank among the taken regions, -1: not taken
    int32_t* sel_first;       // offset of the region's first triangle in the result arrays
    int32_t* sel_fill;        // scatter cursor
    immesh_region_info* sel_info;   // [RG_CAP_REGIONS] the taken regions, in index order
    double region_size;
    int32_t cap_tris;
};

// what the marking launch reads of the job (the mesher's own arrays; lengths from the job's device counters)
struct RegionsJob {
    const int32_t* sc;        // the job's per-scan counters
    int32_t* overflow;        // its SC_OVERFLOW slot
    const int32_t* list_rem;  // removal list: triangle indices, sc[i_rem] entries
    const int32_t* add_sorted;// add list sorted by triplet: triangle indices, sc[i_add] entries
    const int32_t* t_v;       // sorted triplets of the pool
    const float* v_pos;       // raw vertex positions
    int32_t i_rem, i_add, cap_list;
};

struct RegionsHost {
    bool on = false;
    RegionsDev d{};
    std::mutex mu;                            // one table query / sync / fetch / key evaluation at a time
    std::mutex err_mu; std::string err;       // error text of this header's calls (never immesh_ctx::err: these run beside the scan thread)
    // results of the last sync (grow-only device buffers)
    bool have_sync = false;
    std::vector<immesh_region_info> sync_regions;
    int64_t sync_tris = 0;
    void* res = nullptr; size_t res_bytes = 0;        // tri | xyz | flip of the last sync
    void* work = nullptr; size_t work_bytes = 0;      // sort keys / indices / voxels
    void* tmp = nullptr; size_t tmp_bytes = 0;        // radix sort temporary
    char* h_stage = nullptr; size_t h_stage_bytes = 0;   // pinned staging of _fetch and of the table query
    void* keys_dev = nullptr; size_t keys_bytes = 0;  // immesh_region_keys staging
};

void rg_launch_mark(hipStream_t s, const RegionsDev& d, const RegionsJob& j);   // per job, between the adjacency commit and the publish
void rg_launch_select(hipStream_t s, const RegionsDev& d, int force_all);
void rg_launch_redirty(hipStream_t s, const RegionsDev& d, int n_sel);   // undo of the snapshot's flag clearing, for a sync that fails behind it
void rg_launch_scatter(hipStream_t s, const RegionsDev& d, const int32_t* t_live, const int32_t* pc_tris, int32_t* tri_idx, int n_sel);
void rg_launch_sort_keys(hipStream_t s, const RegionsDev& d, const int32_t* t_v, const int32_t* tri_idx, int n, int which, unsigned long long* k64);
void rg_launch_emit(hipStream_t s, const RegionsDev& d, const int32_t* t_v, const int8_t* t_flip, const int32_t* tri_sorted, int n, int32_t* tri_out, uint8_t* flip_out);
void rg_launch_unique_voxels(hipStream_t s, const uint32_t* vox_sorted, int n, int32_t* list, int32_t* count);
void rg_launch_keys(hipStream_t s, const float* vtx, const int32_t* tri, int64_t n_tri, double region_size, int32_t* keys_out);

struct immesh_ctx;
struct MeshDev;
int regions_create(immesh_ctx* c);              // host record only (mesh_alloc)
void regions_free(immesh_ctx* c);               // mesh_free
void regions_enqueue_mark(immesh_ctx* c, const MeshDev& m, hipStream_t s, const int32_t* add_sorted);   // mesh_enqueue_b
