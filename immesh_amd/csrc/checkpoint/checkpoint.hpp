// Checkpoints (include/immesh_checkpoint.h): the file's header, and the launches checkpoint_host.cpp sequences.  The kernels of this directory
// take plain pointers: RegMapDev / MeshDev / RegionsDev are read and written where they lie, by the host code, section by section.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../../include/immesh_checkpoint.h"

constexpr int CK_N_REC = 16, CK_N_COUNT = 16, CK_N_TABLES = 5;
constexpr int64_t CK_ALIGN = 64;                 // sections start at multiples of this
constexpr size_t CK_STAGE_BYTES = 16u << 20;     // each of the two pinned staging buffers of a save / load

// counts[] of the header
enum { CKC_ROOTS = 0, CKC_NODES, CKC_CHUNKS, CKC_FREE_READY, CKC_FREE_PENDING, CKC_EXT, CKC_LEAF, CKC_VERTS, CKC_VOXELS, CKC_TRIS, CKC_LIVE, CKC_ADJ, CKC_REGIONS,
       CKC_SCANS_MESHED, CKC_MAP_UPDATES, CKC_MESH_JOBS };
// the open-addressing tables, and masks[] of the header (the region hash has a fixed size)
enum { CKT_REG = 0, CKT_GRID, CKT_VOX, CKT_TRI, CKT_REGION };

struct CkFileHeader {
    char magic[8];                 // "IMMESHCK"
    int32_t version, header_bytes, n_sections, section_bytes;
    int64_t file_bytes, payload_offset;
    uint64_t header_checksum;      // over header + section table, this field zero
    int32_t has_regions, has_colour;
    int32_t rec[CK_N_REC];         // record sizes and strides of the saving library (ck_rec_names)
    uint64_t masks[4];             // hmask, g_mask, x_mask, th_mask
    int64_t counts[CK_N_COUNT];
    immesh_config cfg;
};
static_assert(sizeof(CkFileHeader) == 568, "checkpoint header layout");
static_assert(sizeof(immesh_checkpoint_section) == 56, "section table entry layout");

// the section's checksum (immesh_checkpoint.h): two stages, workgroup partials then one workgroup; out = one 64-bit word in device memory.
// data is 8-byte aligned; `partials` holds ck_checksum_blocks(bytes) words
int ck_checksum_blocks(size_t bytes);
void ck_launch_checksum(hipStream_t s, const void* data, size_t bytes, unsigned long long* partials, unsigned long long* out);
// occupied slots of an open-addressing table (key or word not all-ones), in ascending slot order: block_counts[b] (ck_table_blocks(n_slots) + 1 entries;
// the host scans them exclusively in place) -> slots[i], ents[i]
int ck_table_blocks(uint64_t n_slots);
void ck_launch_count(hipStream_t s, int table, const void* ents, uint64_t n_slots, int32_t* block_counts);
void ck_launch_pack(hipStream_t s, int table, const void* ents, uint64_t n_slots, const int32_t* block_base, uint32_t* out_slots, void* out_ents);
// the packed records back into a table that immesh_create left empty; *bad counts slot indices outside the table (nothing is written for them)
void ck_launch_unpack(hipStream_t s, int table, void* ents, uint64_t n_slots, const uint32_t* slots, const void* packed, int64_t n, int32_t* bad);
int ck_table_entry_bytes(int table);
