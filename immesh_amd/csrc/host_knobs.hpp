// Every environment switch the library reads, in one place.  The ONE rule: Knobs::from_env() runs when a context is created (immesh_create) and the
// context keeps the result as c->knobs; nothing else in csrc/ looks at the environment.  INTEGRATION.md carries the same list as a table
// (tests/test_host_knobs.py holds the two together).
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>

struct Knobs {
    bool debug = false;            // IMMESH_DEBUG: in-kernel phase timers of the registration and the mesher (printed by immesh_counters / after every mesh job)
    bool debug_waits = false;      // IMMESH_DEBUG_WAITS: how long the scan thread stands in mesh_next_world_buffer + the mesher's phase marks (printed by mesh_free)
    std::string trace_file;        // IMMESH_TRACE_FILE (with IMMESH_DEBUG): immesh_counters writes the per-wavefront trace records of the LAST launches there (tools/trace_report.py)
    int split_general = -1;        // IMMESH_SPLIT_GENERAL: subtree work items of the map update (regmap.hpp); unset (-1) = on for deep octrees (max_layer >= 3)
    bool no_priority = false;      // IMMESH_NO_PRIORITY: every stream at the default priority (else: registration highest, mesher lowest)
    int mesh_cus = 0;              // IMMESH_MESH_CUS=n, 8 <= n < 1024 (measurement knob): the mesher's streams and the pre-processing stream are confined to n CUs; else 0
    int rp_blocks = 0;             // IMMESH_RP_BLOCKS (>= 1): grid cap of residual_persistent_kernel; unset (0) = half of the device's resident workgroups - 1
    bool rp_force_abort = false;   // IMMESH_RP_FORCE_ABORT (tests): every resident-grid registration gives up in its first gather
    bool match_seq = false;        // IMMESH_MATCH_SEQ (A/B): the lane-by-lane leaf walk of rounds 1-5 instead of the wave-cooperative one
    bool host_ekf = false;         // IMMESH_HOST_EKF (debugging): the round-1 host loop (one round trip per pass)
    // IMMESH_SERIAL_SAFE (counter collection: rocprofv3 --pmc runs one kernel at a time, and a mesher kernel polling a flag that a kernel queued BEHIND it on
    // another stream will store never sees it): the mesher waits for an event behind the map update's launches instead, and the VoxelGrid is not gated --
    // same kernels, same data, a more conservative order
    bool serial_safe = false;
    bool serial_order = false;     // IMMESH_SERIAL_ORDER (host loop): map growth first, then the hand-over to the mesher -- the order of the reference's map_incremental_grow
    bool ds_radix = false;         // IMMESH_DS_RADIX: immesh_downsample goes straight to the radix pipeline (no hashed form)
    bool ds_no_gate = false;       // IMMESH_DS_NO_GATE: the asynchronous VoxelGrid is never held back until the next registration launch runs
    bool no_graph = false;         // IMMESH_NO_GRAPH: plain launches instead of hipGraph replay (mesher phases, asynchronous VoxelGrid)
    // IMMESH_NO_SPLIT / IMMESH_SPLIT: the triangulations on the third stream, the diff at the head of phase B: 0 never (IMMESH_NO_SPLIT / IMMESH_SPLIT=0),
    // 1 always (IMMESH_SPLIT=<non-zero>), 2 while the mesher is behind (with the third job in flight; default)
    int split_mode = 2;
    int mesh_room = 0;             // IMMESH_MESH_ROOM=1..MESH_NPAR (measurement knob): a fixed number of mesh jobs in flight (2 = rounds 1-5); unset (0) = the worker decides
    bool no_pipeline = false;      // IMMESH_NO_PIPELINE: phase A of scan k+1 never overlaps phase B of scan k
    int tri_stream = 1;            // IMMESH_TRI_STREAM (measurement knob): the split triangulations run on 0 the fetch stream, 1 the pre-processing stream (default), 2 the null stream
    int fused_wgs = 768;           // IMMESH_FUSED_WGS (>= 32; measurement knob, tools/r06_fused.sh): grid cap of replay_fused_kernel
    int list_div = 0;              // IMMESH_LIST_DIV (>= 4; measurement knob, tools/r06_c4div.sh): points per workgroup of replay_list_kernel's grid; 0 = 32 (deep octrees) / 128
    int mesh_grid_div = 1;         // IMMESH_MESH_GRID_DIV (>= 1): divides the fixed grids of the mesher's knn / triangulation launches

    static Knobs from_env(int mesh_npar) {
        auto on = [](const char* name) { return getenv(name) != nullptr; };
        auto num = [](const char* name, int unset) { const char* e = getenv(name); return e ? atoi(e) : unset; };
        Knobs k;
        k.debug = on("IMMESH_DEBUG"); k.debug_waits = on("IMMESH_DEBUG_WAITS");
        if (const char* e = getenv("IMMESH_TRACE_FILE")) k.trace_file = e;
        if (on("IMMESH_SPLIT_GENERAL")) k.split_general = num("IMMESH_SPLIT_GENERAL", 0);
        k.no_priority = on("IMMESH_NO_PRIORITY");
        k.mesh_cus = num("IMMESH_MESH_CUS", 0); if (k.mesh_cus < 8 || k.mesh_cus >= 1024) k.mesh_cus = 0;
        if (on("IMMESH_RP_BLOCKS")) k.rp_blocks = std::max(1, num("IMMESH_RP_BLOCKS", 0));
        k.rp_force_abort = on("IMMESH_RP_FORCE_ABORT"); k.match_seq = on("IMMESH_MATCH_SEQ"); k.host_ekf = on("IMMESH_HOST_EKF");
        k.serial_safe = on("IMMESH_SERIAL_SAFE"); k.serial_order = on("IMMESH_SERIAL_ORDER");
        k.ds_radix = on("IMMESH_DS_RADIX"); k.ds_no_gate = on("IMMESH_DS_NO_GATE");
        k.no_graph = on("IMMESH_NO_GRAPH");
        k.split_mode = on("IMMESH_NO_SPLIT") ? 0 : 2;
        if (on("IMMESH_SPLIT")) k.split_mode = num("IMMESH_SPLIT", 0) == 0 ? 0 : 1;
        if (on("IMMESH_MESH_ROOM")) k.mesh_room = std::min(std::max(num("IMMESH_MESH_ROOM", 0), 1), mesh_npar);
        k.no_pipeline = on("IMMESH_NO_PIPELINE");
        k.tri_stream = num("IMMESH_TRI_STREAM", 1);
        { const int v = num("IMMESH_FUSED_WGS", 0); k.fused_wgs = v >= 32 ? v : 768; }
        { const int v = num("IMMESH_LIST_DIV", 0); k.list_div = v >= 4 ? v : 0; }
        k.mesh_grid_div = std::max(1, num("IMMESH_MESH_GRID_DIV", 1));
        return k;
    }

    // A non-blocking stream of the given priority -- or, for the streams IMMESH_MESH_CUS confines (`maskable`), one restricted to the first mesh_cus CUs.
    // CU-masked streams are BLOCKING streams on which event-timed launches failed intermittently (garbage counters / memory faults / hangs with the
    // in-library profiler on, tools/debug_profiler.sh) and the gain is within noise with the round-2 kernels -- so the mask is opt-in.
    hipError_t make_stream(hipStream_t* s, int priority, bool maskable) const {
        if (!maskable || !mesh_cus) return hipStreamCreateWithPriority(s, hipStreamNonBlocking, priority);
        uint32_t mask[32];
        std::memset(mask, 0, sizeof(mask));
        for (int i = 0; i < mesh_cus; i++) mask[i >> 5] |= 1u << (i & 31);
        return hipExtStreamCreateWithCUMask(s, 32, mask);
    }
};
