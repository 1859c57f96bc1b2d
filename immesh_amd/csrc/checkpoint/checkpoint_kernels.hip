// Kernels of the checkpoints (include/immesh_checkpoint.h): occupied-slot compaction of the open-addressing tables, its inverse, and the section
// checksum.  All of it is memory-bound streaming: 16-byte loads per lane, one pass per table for the count and one for the pack, no atomics in global
// memory (per-workgroup counts -> rocPRIM exclusive scan on the host side -> ordered scatter), so the packed order is the ascending slot order and two
// saves of one state write the same bytes.
#include "checkpoint.hpp"
#include "../prof.hpp"
#include "../regmap.hpp"
#include "../mesh_kernels.hpp"
#include "../regions/regions.hpp"

namespace {

constexpr int CK_BLOCK = 256;
constexpr int CK_ITEMS = 4;                        // slots per lane: a workgroup covers CK_BLOCK * CK_ITEMS consecutive slots, item-major (coalesced)
constexpr int CK_TILE = CK_BLOCK * CK_ITEMS;
constexpr int CK_SUM_BLOCKS_MAX = 1024;

struct TriEnt { int32_t word; };
static_assert(sizeof(HashEnt) == 16 && sizeof(MeshVoxEnt) == 16 && sizeof(RgEnt) == 16 && sizeof(MeshGridEnt) == 32 && sizeof(TriEnt) == 4, "table entry sizes");

// one entry in registers, moved with the widest loads its size allows
template <int BYTES> struct CkRaw;
template <> struct CkRaw<16> { ulonglong2 a; };
template <> struct CkRaw<32> { ulonglong2 a, b; };
template <> struct CkRaw<4> { int32_t a; };
template <int BYTES> __device__ __forceinline__ CkRaw<BYTES> ck_load(const void* base, uint64_t i) { return ((const CkRaw<BYTES>*)base)[i]; }
template <int BYTES> __device__ __forceinline__ void ck_store(void* base, uint64_t i, const CkRaw<BYTES>& v) { ((CkRaw<BYTES>*)base)[i] = v; }

// occupied = key (or word) not all-ones.  KEY_AT: byte offset of the 64-bit key inside the entry (HashEnt / MeshVoxEnt / RgEnt: 0, MeshGridEnt: 16)
template <int BYTES, int KEY_AT> __device__ __forceinline__ bool ck_occupied(const CkRaw<BYTES>& v);
template <> __device__ __forceinline__ bool ck_occupied<16, 0>(const CkRaw<16>& v) { return v.a.x != ~0ull; }
template <> __device__ __forceinline__ bool ck_occupied<32, 16>(const CkRaw<32>& v) { return v.b.x != ~0ull; }
template <> __device__ __forceinline__ bool ck_occupied<4, 0>(const CkRaw<4>& v) { return v.a != -1; }
static_assert(offsetof(HashEnt, key) == 0 && offsetof(MeshVoxEnt, key) == 0 && offsetof(RgEnt, key) == 0 && offsetof(MeshGridEnt, key) == 16, "key offsets");

template <int BYTES, int KEY_AT>
__global__ __launch_bounds__(CK_BLOCK) void ck_count_kernel(const void* __restrict__ ents, uint64_t n_slots, int32_t* __restrict__ block_counts) {
    __shared__ int wave_cnt[CK_BLOCK / 64];
    const uint64_t base = (uint64_t)blockIdx.x * CK_TILE;
    int mine = 0;   // (lane 0 of each wavefront: occupied slots of the wavefront's items)
#pragma unroll
    for (int it = 0; it < CK_ITEMS; it++) {
        const uint64_t i = base + (uint64_t)it * CK_BLOCK + threadIdx.x;
        const bool occ = i < n_slots && ck_occupied<BYTES, KEY_AT>(ck_load<BYTES>(ents, i));
        mine += __popcll(__ballot(occ));
    }
    if ((threadIdx.x & 63) == 0) wave_cnt[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
#pragma unroll
        for (int w = 0; w < CK_BLOCK / 64; w++) t += wave_cnt[w];
        block_counts[blockIdx.x] = t;
    }
}

template <int BYTES, int KEY_AT>
__global__ __launch_bounds__(CK_BLOCK) void ck_pack_kernel(const void* __restrict__ ents, uint64_t n_slots, const int32_t* __restrict__ block_base,
                                                           uint32_t* __restrict__ out_slots, void* __restrict__ out_ents) {
    __shared__ int wave_cnt[CK_ITEMS][CK_BLOCK / 64];
    const uint64_t base = (uint64_t)blockIdx.x * CK_TILE;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    CkRaw<BYTES> v[CK_ITEMS];
    bool occ[CK_ITEMS];
    int rank[CK_ITEMS];
#pragma unroll
    for (int it = 0; it < CK_ITEMS; it++) {
        const uint64_t i = base + (uint64_t)it * CK_BLOCK + threadIdx.x;
        occ[it] = false;
        if (i < n_slots) { v[it] = ck_load<BYTES>(ents, i); occ[it] = ck_occupied<BYTES, KEY_AT>(v[it]); }
        const unsigned long long mask = __ballot(occ[it]);
        rank[it] = __popcll(mask & ((1ull << lane) - 1ull));
        if (lane == 0) wave_cnt[it][wave] = __popcll(mask);
    }
    __syncthreads();
    int64_t pos = block_base[blockIdx.x];
#pragma unroll
    for (int it = 0; it < CK_ITEMS; it++) {
#pragma unroll
        for (int w = 0; w < CK_BLOCK / 64; w++) {
            if (w == wave && occ[it]) {
                const uint64_t i = base + (uint64_t)it * CK_BLOCK + threadIdx.x;
                out_slots[pos + rank[it]] = (uint32_t)i;
                ck_store<BYTES>(out_ents, (uint64_t)(pos + rank[it]), v[it]);
            }
            pos += wave_cnt[it][w];
        }
    }
}

template <int BYTES>
__global__ __launch_bounds__(CK_BLOCK) void ck_unpack_kernel(void* __restrict__ ents, uint64_t n_slots, const uint32_t* __restrict__ slots, const void* __restrict__ packed,
                                                             int64_t n, int32_t* __restrict__ bad) {
    const int64_t stride = (int64_t)gridDim.x * CK_BLOCK;
    for (int64_t i = (int64_t)blockIdx.x * CK_BLOCK + threadIdx.x; i < n; i += stride) {
        const uint64_t slot = slots[i];
        if (slot < n_slots) ck_store<BYTES>(ents, slot, ck_load<BYTES>(packed, (uint64_t)i));
        else atomicAdd(bad, 1);   // (a file that passed its checksums never gets here)
    }
}

__device__ __forceinline__ unsigned long long ck_mix(unsigned long long w, unsigned long long i) { return imd::hash64(w ^ (i * 0x9E3779B97F4A7C15ull)); }

// sum of a workgroup's values: wavefront shuffles, then the wavefronts' sums through LDS; the result is valid in thread 0
__device__ __forceinline__ unsigned long long ck_block_sum(unsigned long long acc) {
    __shared__ unsigned long long wave_sum[CK_BLOCK / 64];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = acc;
    __syncthreads();
    unsigned long long t = 0;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 0; w < CK_BLOCK / 64; w++) t += wave_sum[w];
    }
    return t;
}

// stage 1: partials[block] = the block's share of the section's sum.  Lanes take pairs of words (one 16-byte load); the odd word and the zero-padded
// tail (bytes not a multiple of 8) go to the last thread of the grid
__global__ __launch_bounds__(CK_BLOCK) void ck_checksum_kernel(const unsigned long long* __restrict__ data, unsigned long long bytes, unsigned long long* __restrict__ partials) {
    const unsigned long long full = bytes >> 3, pairs = full >> 1;
    const unsigned long long stride = (unsigned long long)gridDim.x * CK_BLOCK;
    unsigned long long acc = 0;
    const ulonglong2* d2 = (const ulonglong2*)data;
    for (unsigned long long p = (unsigned long long)blockIdx.x * CK_BLOCK + threadIdx.x; p < pairs; p += stride) {
        const ulonglong2 v = d2[p];
        acc += ck_mix(v.x, 2 * p) + ck_mix(v.y, 2 * p + 1);
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == CK_BLOCK - 1) {
        if (full & 1) acc += ck_mix(data[full - 1], full - 1);
        const int tail = (int)(bytes & 7);
        if (tail) {
            const unsigned char* b = (const unsigned char*)data + (full << 3);
            unsigned long long w = 0;
            for (int k = 0; k < tail; k++) w |= (unsigned long long)b[k] << (8 * k);
            acc += ck_mix(w, full);
        }
    }
    const unsigned long long t = ck_block_sum(acc);
    if (threadIdx.x == 0) partials[blockIdx.x] = t;
}
// stage 2: one workgroup sums the partials
__global__ __launch_bounds__(CK_BLOCK) void ck_checksum_final_kernel(const unsigned long long* __restrict__ partials, int n, unsigned long long* __restrict__ out) {
    unsigned long long acc = 0;
    for (int i = threadIdx.x; i < n; i += CK_BLOCK) acc += partials[i];
    const unsigned long long t = ck_block_sum(acc);
    if (threadIdx.x == 0) *out = t;
}

}  // namespace

int ck_checksum_blocks(size_t bytes) {
    const size_t pairs = bytes >> 4;
    const size_t per_block = (size_t)CK_BLOCK * 8;   // eight pairs per lane before the grid is capped
    return (int)std::min<size_t>(std::max<size_t>((pairs + per_block - 1) / per_block, 1), CK_SUM_BLOCKS_MAX);
}
void ck_launch_checksum(hipStream_t s, const void* data, size_t bytes, unsigned long long* partials, unsigned long long* out) {
    const int nb = ck_checksum_blocks(bytes);
    KLAUNCH(ck_checksum_kernel, dim3(nb), dim3(CK_BLOCK), 0, s, (const unsigned long long*)data, (unsigned long long)bytes, partials);
    KLAUNCH(ck_checksum_final_kernel, dim3(1), dim3(CK_BLOCK), 0, s, partials, nb, out);
}

int ck_table_blocks(uint64_t n_slots) { return (int)((n_slots + CK_TILE - 1) / CK_TILE); }
int ck_table_entry_bytes(int table) { return table == CKT_GRID ? 32 : table == CKT_TRI ? 4 : 16; }

void ck_launch_count(hipStream_t s, int table, const void* ents, uint64_t n_slots, int32_t* block_counts) {
    const dim3 g(ck_table_blocks(n_slots)), b(CK_BLOCK);
    if (table == CKT_GRID) KLAUNCH((ck_count_kernel<32, 16>), g, b, 0, s, ents, n_slots, block_counts);
    else if (table == CKT_TRI) KLAUNCH((ck_count_kernel<4, 0>), g, b, 0, s, ents, n_slots, block_counts);
    else KLAUNCH((ck_count_kernel<16, 0>), g, b, 0, s, ents, n_slots, block_counts);
}
void ck_launch_pack(hipStream_t s, int table, const void* ents, uint64_t n_slots, const int32_t* block_base, uint32_t* out_slots, void* out_ents) {
    const dim3 g(ck_table_blocks(n_slots)), b(CK_BLOCK);
    if (table == CKT_GRID) KLAUNCH((ck_pack_kernel<32, 16>), g, b, 0, s, ents, n_slots, block_base, out_slots, out_ents);
    else if (table == CKT_TRI) KLAUNCH((ck_pack_kernel<4, 0>), g, b, 0, s, ents, n_slots, block_base, out_slots, out_ents);
    else KLAUNCH((ck_pack_kernel<16, 0>), g, b, 0, s, ents, n_slots, block_base, out_slots, out_ents);
}
void ck_launch_unpack(hipStream_t s, int table, void* ents, uint64_t n_slots, const uint32_t* slots, const void* packed, int64_t n, int32_t* bad) {
    if (n <= 0) return;
    const dim3 g((unsigned)std::min<int64_t>((n + CK_BLOCK - 1) / CK_BLOCK, 4096)), b(CK_BLOCK);
    if (table == CKT_GRID) KLAUNCH((ck_unpack_kernel<32>), g, b, 0, s, ents, n_slots, slots, packed, n, bad);
    else if (table == CKT_TRI) KLAUNCH((ck_unpack_kernel<4>), g, b, 0, s, ents, n_slots, slots, packed, n, bad);
    else KLAUNCH((ck_unpack_kernel<16>), g, b, 0, s, ents, n_slots, slots, packed, n, bad);
}
