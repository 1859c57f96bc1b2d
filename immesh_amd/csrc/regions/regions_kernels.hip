// Region buckets of the renderer (include/immesh_regions.h): the per-job marking launch and the kernels of a synchronisation.
//   regions_mark_kernel    per job: removals decrement their region; adds look their key up or create the region (provisional: numbered below)
//   regions_order_kernel   per job, one workgroup: numbers the job's new regions by the first add-list position of their key (the reference
//                          inserts in add-list order, Triangle_manager::insert_triangle_to_list), then files the triangles that waited for a number
//   regions_select_kernel  sync, one workgroup: taken regions, their ranks and triangle offsets (two prefix sums), flags cleared
//   regions_scatter_kernel sync: one streaming pass over the triangle pool (t_live + t_region, 8 B per entry) into per-region segments
//   regions_sort_keys / regions_emit / regions_unique_voxels: order by (region rank, triplet) with the radix sort of the mesh export; triplet + flip out
#include "regions.hpp"
#include "../prof.hpp"

#define RGD __device__ __forceinline__
static constexpr unsigned long long RG_EMPTY = ~0ull;
static constexpr unsigned long long RG_KMASK = (1ull << 21) - 1;

// THE key rule (triangle.cpp:3-10, 37-40): c = ((p0 + p1) + p2) / 3.0, key = std::round(c / S) per component, in double, in this order
// (-ffp-contract=off: no fused multiply-add); round() is half away from zero.  Used by the marking launch and by immesh_region_keys.
RGD void rg_key_of(const float* __restrict__ v_pos, int i0, int i1, int i2, double S, int key[3]) {
#pragma unroll
    for (int k = 0; k < 3; k++) {
        double c = ((double)v_pos[(size_t)i0 * 3 + k] + (double)v_pos[(size_t)i1 * 3 + k]) + (double)v_pos[(size_t)i2 * 3 + k];
        c = c / 3.0;
        key[k] = (int)round(c / S);
    }
}
RGD bool rg_pack(const int key[3], unsigned long long& packed) {
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; k++) ok = ok && key[k] > -RG_KEY_BIAS && key[k] < RG_KEY_BIAS;
    packed = ((unsigned long long)(key[0] + RG_KEY_BIAS) & RG_KMASK) | (((unsigned long long)(key[1] + RG_KEY_BIAS) & RG_KMASK) << 21) |
             (((unsigned long long)(key[2] + RG_KEY_BIAS) & RG_KMASK) << 42);
    return ok;
}
RGD unsigned int rg_hash(unsigned long long k) {
    k ^= k >> 30; k *= 0xbf58476d1ce4e5b9ull; k ^= k >> 27; k *= 0x94d049bb133111ebull; k ^= k >> 31;
    return (unsigned int)k & (unsigned int)(RG_HASH_CAP - 1);
}

__global__ __launch_bounds__(256) void regions_mark_kernel(RegionsDev d, RegionsJob j) {
    const int n_rem = min(j.sc[j.i_rem], j.cap_list), n_add = min(j.sc[j.i_add], j.cap_list);
    const int gid = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
    // Triangle_manager::erase_triangle_from_list: a removed triangle was live, so its region is on file
    for (int i = gid; i < n_rem; i += stride) {
        const int t = j.list_rem[i];
        if (t < 0 || t >= d.cap_tris) continue;
        const int r = d.t_region[t];
        if (r >= 0) { atomicSub(&d.r_nlive[r], 1); d.r_dirty[r] = 1; }
    }
    // Triangle_manager::insert_triangle_to_list
    for (int i = gid; i < n_add; i += stride) {
        const int t = j.add_sorted[i];
        if (t < 0 || t >= d.cap_tris) continue;
        const int r = d.t_region[t];
        if (r >= 0) { atomicAdd(&d.r_nlive[r], 1); d.r_dirty[r] = 1; continue; }   // an erased triangle that comes back: same vertices, same key
        int key[3];
        rg_key_of(j.v_pos, j.t_v[(size_t)t * 3 + 0], j.t_v[(size_t)t * 3 + 1], j.t_v[(size_t)t * 3 + 2], d.region_size, key);
        unsigned long long packed;
        if (!rg_pack(key, packed)) { *j.overflow = RG_OVERFLOW_CODE; continue; }
        unsigned int slot = rg_hash(packed);
        bool found = false;
        for (int probe = 0; probe < RG_HASH_CAP; probe++, slot = (slot + 1) & (RG_HASH_CAP - 1)) {
            unsigned long long k = __hip_atomic_load(&d.ent[slot].key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (k == RG_EMPTY) {
                k = atomicCAS(&d.ent[slot].key, RG_EMPTY, packed);
                if (k == RG_EMPTY) {   // this lane created the region
                    const int pos = atomicAdd(&d.cnt[RG_NEW], 1);
                    if (pos < RG_CAP_REGIONS) d.new_slots[pos] = (int)slot; else *j.overflow = RG_OVERFLOW_CODE;
                    k = packed;
                }
            }
            if (k == packed) { found = true; break; }
        }
        if (!found) { *j.overflow = RG_OVERFLOW_CODE; continue; }
        const int val = d.ent[slot].val;   // >= 0: numbered by an earlier job; -1: created by this job (by this lane or another)
        if (val >= 0) { d.t_region[t] = val; atomicAdd(&d.r_nlive[val], 1); d.r_dirty[val] = 1; }
        else { atomicMin(&d.ent[slot].first, (unsigned int)i); d.t_region[t] = -2 - (int)slot; }
    }
}

__global__ __launch_bounds__(1024) void regions_order_kernel(RegionsDev d, RegionsJob j) {
    __shared__ unsigned int s_first[1024];
    const int tid = threadIdx.x;
    const int n_new = d.cnt[RG_NEW], base = d.cnt[RG_N];
    if (n_new == 0) return;   // (uniform: the usual job)
    if (n_new > RG_CAP_REGIONS - base) {
        __syncthreads();
        if (tid == 0) { *j.overflow = RG_OVERFLOW_CODE; d.cnt[RG_NEW] = 0; }
        return;
    }
    // rank of a new region = number of new regions whose key appears earlier in the add list (the positions are distinct)
    for (int own0 = 0; own0 < n_new; own0 += 1024) {
        const int own = own0 + tid;
        const int slot = own < n_new ? d.new_slots[own] : -1;
        const unsigned int f = slot >= 0 ? d.ent[slot].first : 0u;
        int rank = 0;
        for (int k0 = 0; k0 < n_new; k0 += 1024) {
            __syncthreads();
            s_first[tid] = k0 + tid < n_new ? d.ent[d.new_slots[k0 + tid]].first : 0xFFFFFFFFu;
            __syncthreads();
            const int lim = min(1024, n_new - k0);
            for (int k = 0; k < lim; k++) rank += s_first[k] < f ? 1 : 0;
        }
        if (slot >= 0) {
            const int idx = base + rank;
            const unsigned long long key = d.ent[slot].key;
            d.ent[slot].val = idx;
            d.r_key[(size_t)idx * 3 + 0] = (int)(key & RG_KMASK) - RG_KEY_BIAS;
            d.r_key[(size_t)idx * 3 + 1] = (int)((key >> 21) & RG_KMASK) - RG_KEY_BIAS;
            d.r_key[(size_t)idx * 3 + 2] = (int)((key >> 42) & RG_KMASK) - RG_KEY_BIAS;
            d.r_nlive[idx] = 0;
            d.r_dirty[idx] = 1;
        }
    }
    __threadfence_block();
    __syncthreads();
    const int n_add = min(j.sc[j.i_add], j.cap_list);
    for (int i = tid; i < n_add; i += 1024) {
        const int t = j.add_sorted[i];
        if (t < 0 || t >= d.cap_tris) continue;
        const int v = d.t_region[t];
        if (v <= -2) {
            const int idx = d.ent[-2 - v].val;
            d.t_region[t] = idx;
            if (idx >= 0) atomicAdd(&d.r_nlive[idx], 1);
        }
    }
    __syncthreads();
    if (tid == 0) { d.cnt[RG_N] = base + n_new; d.cnt[RG_NEW] = 0; }
}

void rg_launch_mark(hipStream_t s, const RegionsDev& d, const RegionsJob& j) {
    KLAUNCH(regions_mark_kernel, dim3(64), dim3(256), 0, s, d, j);
    KLAUNCH(regions_order_kernel, dim3(1), dim3(1024), 0, s, d, j);
}

// ---- synchronisation ------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void regions_select_kernel(RegionsDev d, int force_all) {
    __shared__ int s_a[2][1024], s_b[2][1024];
    __shared__ int s_carry[2];
    const int tid = threadIdx.x;
    const int n = min(d.cnt[RG_N], RG_CAP_REGIONS);
    if (tid == 0) { s_carry[0] = 0; s_carry[1] = 0; }
    __syncthreads();
    for (int base = 0; base < n; base += 1024) {
        const int r = base + tid;
        const int was_dirty = r < n ? d.r_dirty[r] : 0;
        const bool take = r < n && (force_all || was_dirty);
        const int c = take ? max(d.r_nlive[r], 0) : 0;
        int cur = 0;
        s_a[0][tid] = take ? 1 : 0; s_b[0][tid] = c;
        __syncthreads();
        for (int off = 1; off < 1024; off <<= 1) {   // inclusive scan of both columns
            const int a = s_a[cur][tid] + (tid >= off ? s_a[cur][tid - off] : 0), b = s_b[cur][tid] + (tid >= off ? s_b[cur][tid - off] : 0);
            s_a[cur ^ 1][tid] = a; s_b[cur ^ 1][tid] = b;
            cur ^= 1;
            __syncthreads();
        }
        const int rank = s_carry[0] + s_a[cur][tid] - (take ? 1 : 0), first = s_carry[1] + s_b[cur][tid] - c;
        if (r < n) {
            d.sel_rank[r] = take ? rank : -1; d.sel_first[r] = first; d.sel_fill[r] = 0;
            if (take) {
                immesh_region_info q;
                q.key[0] = d.r_key[(size_t)r * 3 + 0]; q.key[1] = d.r_key[(size_t)r * 3 + 1]; q.key[2] = d.r_key[(size_t)r * 3 + 2];
                q.index = r; q.n_triangles = c; q.dirty = was_dirty ? 1 : 0; q.first = first;
                d.sel_info[rank] = q;
                d.r_dirty[r] = 0;   // get_triangle_set(.., reset_status = true)
            }
        }
        __syncthreads();
        if (tid == 1023) { s_carry[0] += s_a[cur][1023]; s_carry[1] += s_b[cur][1023]; }
        __syncthreads();
    }
    if (tid == 0) { d.cnt[RG_SEL_REGIONS] = s_carry[0]; d.cnt[RG_SEL_TRIS] = s_carry[1]; d.cnt[RG_BAD] = 0; d.cnt[RG_NLIST] = 0; }
}
void rg_launch_select(hipStream_t s, const RegionsDev& d, int force_all) { KLAUNCH(regions_select_kernel, dim3(1), dim3(1024), 0, s, d, force_all); }

// a sync that fails after the snapshot (out of memory for its buffers) gives the taken regions their flags back: no update is lost
__global__ void regions_redirty_kernel(RegionsDev d, int n_sel) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_sel && d.sel_info[i].dirty) d.r_dirty[d.sel_info[i].index] = 1;
}
void rg_launch_redirty(hipStream_t s, const RegionsDev& d, int n_sel) { KLAUNCH(regions_redirty_kernel, dim3((n_sel + 255) / 256), dim3(256), 0, s, d, n_sel); }

// Live triangles of taken regions -> tri_idx[sel_first[region] + k], k in arrival order (sorted afterwards).  Neighbouring pool entries were created by
// the same job and mostly share a region: the lanes of a wavefront that do are served by ONE atomic on the region's cursor.
__global__ __launch_bounds__(256) void regions_scatter_kernel(RegionsDev d, const int32_t* __restrict__ t_live, const int32_t* __restrict__ pc_tris, int32_t* __restrict__ tri_idx, int n_sel) {
    const int nt = min(*pc_tris, d.cap_tris);
    const int lane = threadIdx.x & 63;
    const int stride = gridDim.x * blockDim.x;
    for (int t0 = blockIdx.x * blockDim.x; t0 < nt; t0 += stride) {
        const int t = t0 + threadIdx.x;
        int r = -1;
        if (t < nt && t_live[t]) { r = d.t_region[t]; if (r < 0 || r >= RG_CAP_REGIONS || d.sel_rank[r] < 0) r = -1; }
        unsigned long long todo = __ballot(r >= 0);
        while (todo) {
            const int leader = __ffsll((long long)todo) - 1;
            const int rl = __shfl(r, leader);
            const unsigned long long same = __ballot(r == rl) & todo;
            int base = 0;
            if (lane == leader) base = atomicAdd(&d.sel_fill[rl], __popcll(same));
            base = __shfl(base, leader);
            if (r == rl) {
                const int k = base + __popcll(same & ((1ull << lane) - 1ull));
                const int pos = d.sel_first[rl] + k;
                if (k < d.r_nlive[rl] && pos < n_sel) tri_idx[pos] = t; else d.cnt[RG_BAD] = 1;
            }
            todo &= ~same;
        }
    }
}
void rg_launch_scatter(hipStream_t s, const RegionsDev& d, const int32_t* t_live, const int32_t* pc_tris, int32_t* tri_idx, int n_sel) {
    KLAUNCH(regions_scatter_kernel, dim3(1024), dim3(256), 0, s, d, t_live, pc_tris, tri_idx, n_sel);
}

// two stable radix passes give (region rank, v0, v1, v2): which 0 -> (v1, v2), which 1 -> (rank, v0).  An unfilled entry (-1) sorts last.
__global__ void regions_sort_keys_kernel(RegionsDev d, const int32_t* __restrict__ t_v, const int32_t* __restrict__ tri_idx, int n, int which, unsigned long long* __restrict__ k64) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int t = tri_idx[i];
    unsigned long long k = ~0ull;
    if (t >= 0 && t < d.cap_tris) {
        if (which == 0) k = ((unsigned long long)(unsigned int)t_v[(size_t)t * 3 + 1] << 32) | (unsigned long long)(unsigned int)t_v[(size_t)t * 3 + 2];
        else {
            const int r = d.t_region[t];
            const unsigned int rank = (r >= 0 && r < RG_CAP_REGIONS) ? (unsigned int)d.sel_rank[r] : 0xFFFFu;
            k = ((unsigned long long)rank << 32) | (unsigned long long)(unsigned int)t_v[(size_t)t * 3 + 0];
        }
    }
    k64[i] = k;
}
void rg_launch_sort_keys(hipStream_t s, const RegionsDev& d, const int32_t* t_v, const int32_t* tri_idx, int n, int which, unsigned long long* k64) {
    KLAUNCH(regions_sort_keys_kernel, dim3((n + 255) / 256), dim3(256), 0, s, d, t_v, tri_idx, n, which, k64);
}

// sorted triplet (the flip is not applied to the order: unparse_triangle_set_to_vector reads m_tri_pts_id[0..2]) + m_index_flip
__global__ void regions_emit_kernel(const int32_t* __restrict__ t_v, const int8_t* __restrict__ t_flip, const int32_t* __restrict__ tri_sorted, int n, int cap_tris,
                                    int32_t* __restrict__ tri_out, uint8_t* __restrict__ flip_out, int32_t* __restrict__ bad) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int t = tri_sorted[i];
    if (t < 0 || t >= cap_tris) {   // a segment the scatter did not fill: the table and the pool disagree (reported by the host)
        *bad = 1;
        tri_out[(size_t)i * 3 + 0] = tri_out[(size_t)i * 3 + 1] = tri_out[(size_t)i * 3 + 2] = -1; flip_out[i] = 0;
        return;
    }
    tri_out[(size_t)i * 3 + 0] = t_v[(size_t)t * 3 + 0]; tri_out[(size_t)i * 3 + 1] = t_v[(size_t)t * 3 + 1]; tri_out[(size_t)i * 3 + 2] = t_v[(size_t)t * 3 + 2];
    flip_out[i] = (uint8_t)t_flip[t];
}
void rg_launch_emit(hipStream_t s, const RegionsDev& d, const int32_t* t_v, const int8_t* t_flip, const int32_t* tri_sorted, int n, int32_t* tri_out, uint8_t* flip_out) {
    KLAUNCH(regions_emit_kernel, dim3((n + 255) / 256), dim3(256), 0, s, t_v, t_flip, tri_sorted, n, d.cap_tris, tri_out, flip_out, d.cnt + RG_BAD);
}

// the mesh voxels whose vertices still want smoothing (mesh_query_voxels_kernel's answers >= 0), each once: the list of launch_mesh_query_smooth
__global__ void regions_unique_voxels_kernel(const uint32_t* __restrict__ vox_sorted, int n, int32_t* __restrict__ list, int32_t* __restrict__ count) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t v = vox_sorted[i];
    if (v < 0x80000000u && (i == 0 || vox_sorted[i - 1] != v)) list[atomicAdd(count, 1)] = (int32_t)v;
}
void rg_launch_unique_voxels(hipStream_t s, const uint32_t* vox_sorted, int n, int32_t* list, int32_t* count) {
    KLAUNCH(regions_unique_voxels_kernel, dim3((n + 255) / 256), dim3(256), 0, s, vox_sorted, n, list, count);
}

__global__ void regions_keys_kernel(const float* __restrict__ vtx, const int32_t* __restrict__ tri, long long n_tri, double S, int32_t* __restrict__ keys_out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_tri) return;
    int key[3];
    rg_key_of(vtx, tri[i * 3 + 0], tri[i * 3 + 1], tri[i * 3 + 2], S, key);
    keys_out[i * 3 + 0] = key[0]; keys_out[i * 3 + 1] = key[1]; keys_out[i * 3 + 2] = key[2];
}
void rg_launch_keys(hipStream_t s, const float* vtx, const int32_t* tri, int64_t n_tri, double region_size, int32_t* keys_out) {
    KLAUNCH(regions_keys_kernel, dim3((unsigned)((n_tri + 255) / 256)), dim3(256), 0, s, vtx, tri, (long long)n_tri, region_size, keys_out);
}
