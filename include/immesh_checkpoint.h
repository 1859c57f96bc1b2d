/* immesh_checkpoint.h -- save and restore the registration map and the mesh map (libimmesh_hip.so).
 *
 * Everything the library knows lives in device memory.  A checkpoint is one file that holds the state between two scans, so that a run can stop
 * and go on later, a map can be built once and localised against in another process, and a map can move into a context with larger pools.
 * There are no flags, no partial saves and no second format.
 *
 * ---- Contract -------------------------------------------------------------------------------------------------------------------------------------
 * Save   is called from the scan thread (the thread that calls immesh_process_scan), like immesh_counters.  It drains what is in flight -- queued
 *        mesh jobs, a pending or deferred map-update tail -- and writes the state between two scans.  It changes nothing: a run that saves in the
 *        middle produces the same bits afterwards as one that does not.  The file is written to path + ".tmp", flushed, fsync'ed and renamed: a
 *        failed save leaves no file at `path` that was not there before, and no path + ".tmp".  Two saves of the same state write the same bytes.
 * Holds  the registration map (hash, node pool, point chunks, extension tables, leaf chunks, free lists, counters, update sequence number, refit
 *        statistics); the persistent part of the mesh map (vertex store incl. smoothed positions, dedupe grid, voxel hash and the per-voxel arrays
 *        with their stamps, triangle pool with word / live / removal stamp / flip and its hash, adjacency, persistent counters, scan sequence number,
 *        cumulative per-scan counters, vertex and live-triangle counts, the mesh job ordinal); the host's cumulative immesh_counters_t; the region
 *        table when it is on; the ten colour arrays when a colourer is passed.
 * Not    per-job results (immesh_mesh_fetch, immesh_last_matches, timings, the last region sync), per-scan scratch, the legacy ikd map, captured
 *        graphs, and the per-update list heads of the registration hash (their stamps are per update and the update sequence number is restored, so
 *        a zeroed table is equivalent).
 * Load   is only accepted on a context on which no map build, update, scan or mesh job has run since immesh_create (IMMESH_E_INVAL otherwise).
 *        Everything is validated against the header and the section table -- by the code behind immesh_checkpoint_probe -- before any device byte is
 *        touched: file length, version, the record sizes written at save, the algorithm parameters of immesh_config (voxel_size, max_layer,
 *        layer_init, max_points_size, planer_threshold, the noise model, mesh_*; they must be equal: IMMESH_E_INVAL), the derived table
 *        sizes (hash masks following cap_root_voxels, cap_vertices, cap_triangles; equal: IMMESH_E_INVAL) and the pool capacities (cap_nodes,
 *        cap_point_chunks, extension tables, leaf chunks, cap_vertices, cap_triangles, adjacency chunks; at least the used counts:
 *        IMMESH_E_CAPACITY).  A refusal at this stage names the field and leaves the context exactly as created.
 *        A checksum mismatch found after placing returns IMMESH_E_FORMAT: the context's maps are then undefined and it may only be destroyed.
 *        After a successful load the context continues exactly as the saving one would have: the same poses, plane table, mesh lists and job
 *        ordinals, bit for bit.
 * Shards contexts with shard_world > 1 are refused by save and load (IMMESH_E_INVAL).
 * Regions load turns the region table on itself when the file has the section (legal: no job has run).  A context that already has it on and a file
 *        without the section is refused (IMMESH_E_INVAL).
 * Colour is saved when a colourer is passed, and restored when the file has the section and a colourer is given; otherwise it is skipped, and
 *        info->has_colour says which (1: written / restored, 0: not).
 * Size   follows content, not capacity: bump-allocated pools are written as their used prefix, open-addressing tables as their occupied slots
 *        (slot index, entry) in ascending slot order, put back into the same slots -- which is why the table sizes must match and why nothing depends
 *        on insertion order.
 *
 * ---- File (little endian) ----------------------------------------------------------------------------------------------------------------------
 *   [0, 568)       header: magic "IMMESHCK", version, header bytes, section count, section entry bytes, file bytes, payload offset, header checksum
 *                  (over header + section table with this field zero), has_regions, has_colour, 16 record sizes, 4 table masks, 16 counts, the
 *                  saving context's immesh_config (DESIGN.md section 14 lists the fields with their offsets)
 *   [568, ...)     section table: n_sections x immesh_checkpoint_section, in file order
 *   payload        the sections, each at a multiple of 64 bytes, gaps zero
 *   Checksum of a section: sum over its 8-byte words w_i (tail zero-padded) of mix64(w_i ^ (i * 0x9E3779B97F4A7C15)) mod 2^64, mix64 = the
 *   splitmix64 finaliser.  tests/checkpoint_checker.py states the same in numpy.
 */
#ifndef IMMESH_CHECKPOINT_H
#define IMMESH_CHECKPOINT_H
#include "immesh_c_api.h"
#include "immesh_colour.h"
#ifdef __cplusplus
extern "C" {
#endif

#define IMMESH_E_IO      (-6)   /* open / read / write / rename failed (text in immesh_last_error) */
#define IMMESH_E_FORMAT  (-7)   /* not a checkpoint, other version or record sizes, truncated, sections inconsistent, checksum mismatch */
#define IMMESH_CHECKPOINT_VERSION 1

typedef struct immesh_checkpoint_section {   /* 56 bytes: one entry of the file's section table */
    char name[24];
    int64_t offset, bytes, records;
    uint64_t checksum;
} immesh_checkpoint_section;

typedef struct immesh_checkpoint_info {
    int32_t version, n_sections;
    int32_t has_regions, has_colour;
    int64_t file_bytes;
    immesh_config cfg;                      /* the saving context's, as given to immesh_create */
    int64_t n_root_voxels, n_nodes, n_point_chunks, n_free_chunks, n_ext_tables, n_leaf_chunks;
    int64_t n_vertices, n_mesh_voxels, n_triangles_pool, n_triangles_live, n_adj_chunks, n_regions;
    int64_t scans_meshed, map_updates;      /* the mesher's scan sequence number, the registration map's update sequence number */
    float ms[4];                            /* save / load only: device pack or unpack + checksums, copies, file, wall */
} immesh_checkpoint_info;

int immesh_checkpoint_save(immesh_ctx* ctx, immesh_colourer* colourer /* or NULL */, const char* path, immesh_checkpoint_info* info /* or NULL */);
int immesh_checkpoint_load(immesh_ctx* ctx, immesh_colourer* colourer /* or NULL */, const char* path, immesh_checkpoint_info* info /* or NULL */);
/* Host only, no device: reads and validates header and section table.  sections (or NULL) receives up to cap entries; info->n_sections is the
 * file's count.  err (or NULL) receives the text of a refusal. */
int immesh_checkpoint_probe(const char* path, immesh_checkpoint_info* info, immesh_checkpoint_section* sections, int32_t cap, char* err, int32_t err_cap);

#ifdef __cplusplus
}
#endif
#endif
