// The stages before the path (include/immesh_c_api.h): the input fence, sensor decode, undistortion and the VoxelGrid entry points, on the
// pre-processing stream.  Context, registration and map: c_api.cpp.
#include "host_ctx.hpp"
#include "imu_host.hpp"
#include <cmath>

extern "C" {

// The stages before the path run on their own stream (they do not read the map) with their own scratch, so they overlap the previous scan's
// map update when immesh_process_scan was asynchronous.  What they share with that scan are its INPUT clouds: the result buffers below are the
// down-sampled / raw clouds an asynchronous immesh_process_scan may still be reading (point_var, transform) -- writers wait for ev_inputs_free.
// "the last asynchronous scan has consumed its input clouds": an event on the registration stream, or -- when the registration launch consumed them in
// its epilogue -- that launch's flag in pinned memory (it arrives a few microseconds behind the pose the caller already holds)
// wait (bounded) until the pinned "input clouds consumed" flag of the registration launch's epilogue has reached inputs_seq; the flag trails the pose the
// caller already holds by a few microseconds, so the wait spins with a pause instead of sleeping, and hands over to the stream when it takes longer
static int wait_inputs_flag(immesh_ctx* c) {
    volatile unsigned long long* f = c->h_epi_flag;
    bool held;
    if (const int rc = wait_pinned(c, c->stream, [&] { return *f >= c->inputs_seq; }, std::chrono::milliseconds(500), std::chrono::microseconds(200), &held)) return rc;
    if (!held) { c->err = "the scan's input clouds were not released (registration stream idle, flag not stored)"; return IMMESH_E_HIP; }
    return 0;
}
static int pre_inputs_fence(immesh_ctx* c) {
    if (c->inputs_seq) return wait_inputs_flag(c);
    HIPCHK(c, hipStreamWaitEvent(c->stream_pre, c->ev_inputs_cur, 0));
    return 0;
}
int immesh_inputs_consumed(immesh_ctx* c) {
    if (!c) return IMMESH_E_INVAL;
    (void)hipSetDevice(c->cfg.device);
    if (c->inputs_seq) return wait_inputs_flag(c);   // the registration launch consumed them in its epilogue: the flag the launch behind it stores, in pinned memory
    HIPCHK(c, hipEventSynchronize(c->ev_inputs_cur));
    return 0;
}
static int pre_resolve(immesh_ctx* c, const void* p, size_t bytes, void* staging, const void** dev_out) {
    if (is_device_ptr(p)) { *dev_out = p; return 0; }
    if (const int frc = pre_inputs_fence(c)) return frc;   // the staging buffers double as immesh_process_scan's own staging
    HIPCHK(c, hipMemcpyAsync(staging, p, bytes, hipMemcpyHostToDevice, c->stream_pre));
    *dev_out = staging;
    return 0;
}
#define PRE_OUTPUT_FENCE(c) do { if (const int _frc = pre_inputs_fence(c)) return _frc; } while (0)

// ---- sensor decode: flag -> exclusive scan -> compact, in arrival order
static int decode_finish(immesh_ctx* c, int n, float* out_xyzit, int32_t* n_out) {
    int32_t cnt = 0;
    HIPCHK(c, hipMemcpyAsync(&cnt, c->p_nseg, 4, hipMemcpyDeviceToHost, c->stream_pre));
    HIPCHK(c, hipStreamSynchronize(c->stream_pre));
    if (out_xyzit && cnt > 0) HIPCHK(c, hipMemcpy(out_xyzit, c->d_und_in, (size_t)cnt * 20, hipMemcpyDefault));
    if (n_out) *n_out = cnt;
    (void)n;
    return 0;
}
// Preprocess::avia_handler, feature_enabled == false   src/preprocess.cpp:139-232
int immesh_decode_livox(immesh_ctx* c, const uint8_t* wire, int32_t n, int32_t n_scans, int32_t point_filter_num, double blind, float* out_xyzit, int32_t* n_out) {
    if (!c || !wire || n <= 0 || n > c->cap_scan || n_scans <= 0 || point_filter_num <= 0) { if (c) c->err = "bad arguments"; return IMMESH_E_INVAL; }
    (void)hipSetDevice(c->cfg.device);
    ProfBind _pb(c);
    hipStream_t s = c->stream_pre;
    const void* d_in;
    int rc;
    if (!c->d_raw_stage && (rc = c->dalloc(&c->d_raw_stage, (size_t)c->cap_scan * 64))) return rc;
    if ((rc = pre_resolve(c, wire, (size_t)n * 19, c->d_raw_stage, &d_in))) return rc;
    int32_t* flag = c->p_idx_a; int32_t* scan = c->p_idx_b; int32_t* keep = c->p_idx_c; int32_t* pos = c->p_seg;
    launch_decode_livox_count(s, (const uint8_t*)d_in, n, n_scans, flag);
    exclusive_sum_i32(s, c->p_sort_temp, c->sort_temp_bytes, flag, scan, n);
    launch_decode_livox_keep(s, (const uint8_t*)d_in, n, n_scans, point_filter_num, blind * blind, scan, keep);
    exclusive_sum_i32(s, c->p_sort_temp, c->sort_temp_bytes, keep, pos, n);
    PRE_OUTPUT_FENCE(c);
    launch_decode_livox_emit(s, (const uint8_t*)d_in, n, keep, pos, c->d_und_in, c->p_nseg);
    return decode_finish(c, n, out_xyzit, n_out);
}
// velodyne_handler's elevation gates as a function of the float q = z / sqrtf(x*x + y*y), in the reference's own expression (host glibc atanf)
static bool velodyne_keep_q(float q, int n_scans) {
    const float angle = (float)((double)(std::atan(q) * 180) / M_PI);
    if (std::isnan(angle)) return false;   // (the reference's int(NaN) is INT_MIN on x86-64: scan_id < 0)
    int scan_id;
    if (angle >= -8.83) scan_id = int((2 - angle) * 3.0 + 0.5);
    else scan_id = n_scans / 2 + int((-8.83 - angle) * 2.0 + 0.5);
    return !(angle > 2 || angle < -24.33 || scan_id > 50 || scan_id < 0);
}
// Float <-> integer in the order of the values (-0.0 and +0.0 share 0), -0x7f800000 (-inf) .. 0x7f800000 (+inf).
static int32_t f32_ordered(float f) { uint32_t b; std::memcpy(&b, &f, 4); return (b & 0x80000000u) ? -(int32_t)(b & 0x7fffffffu) : (int32_t)b; }
static float ordered_f32(int32_t k) { const uint32_t b = k < 0 ? (0x80000000u | (uint32_t)(-k)) : (uint32_t)k; float f; std::memcpy(&f, &b, 4); return f; }
// The kept points are exactly those with q_lo <= q <= q_hi.  This rests on angle(q) being monotone non-decreasing in q, i.e. on glibc's atanf
// being monotone: then the gates (angle <= 2, angle >= -24.33, and below -8.83 a scan_id that grows as the angle falls, cut at 50) keep one
// interval of angles, hence one interval of q.  An enumeration of all 2^32 floats q with glibc 2.35's atanf found exactly one such interval for
// n_scans 16, 32 and 64 (q_lo 0xbee77fec / 0xbea7264c, q_hi 0x3d0f0915).  q = 0 (angle 0, scan_id 6) is kept for every n_scans >= 1, so each
// end is found by a bisection over the ordered float bit patterns on its side of 0: about 2 x 31 atanf calls.  For n_scans / 2 >= 51 the lower
// branch is cut entirely and q_lo falls on the -8.83 degree boundary by itself.
static void velodyne_q_interval(int n_scans, float* q_lo, float* q_hi) {
    int32_t dropped = f32_ordered(-INFINITY), kept = 0;   // angle -90: dropped
    while (kept - dropped > 1) { const int32_t m = dropped + (kept - dropped) / 2; (velodyne_keep_q(ordered_f32(m), n_scans) ? kept : dropped) = m; }
    *q_lo = ordered_f32(kept);
    kept = 0; dropped = f32_ordered(INFINITY);             // angle +90: dropped
    while (dropped - kept > 1) { const int32_t m = kept + (dropped - kept) / 2; (velodyne_keep_q(ordered_f32(m), n_scans) ? kept : dropped) = m; }
    *q_hi = ordered_f32(kept);
}
// Preprocess::velodyne_handler   src/preprocess.cpp:497-526
int immesh_decode_velodyne(immesh_ctx* c, const uint8_t* data, int32_t n, int32_t point_step, int32_t off_x, int32_t off_y, int32_t off_z, int32_t off_intensity,
                           int32_t n_scans, float* out_xyzit, int32_t* n_out) {
    const int32_t mx = std::max(std::max(off_x, off_y), std::max(off_z, off_intensity));
    if (!c || !data || n <= 0 || n > c->cap_scan || point_step < 16 || point_step > 64 || std::min(std::min(off_x, off_y), std::min(off_z, off_intensity)) < 0 || mx + 4 > point_step ||
        n_scans <= 0) {
        if (c) c->err = "bad arguments (point_step 16..64, float32 fields inside the point, n_scans >= 1)";
        return IMMESH_E_INVAL;
    }
    float q_lo, q_hi;
    velodyne_q_interval(n_scans, &q_lo, &q_hi);
    (void)hipSetDevice(c->cfg.device);
    ProfBind _pb(c);
    hipStream_t s = c->stream_pre;
    const void* d_in;
    int rc;
    if (!c->d_raw_stage && (rc = c->dalloc(&c->d_raw_stage, (size_t)c->cap_scan * 64))) return rc;
    if ((rc = pre_resolve(c, data, (size_t)n * point_step, c->d_raw_stage, &d_in))) return rc;
    int32_t* keep = c->p_idx_c; int32_t* pos = c->p_seg;
    launch_decode_velodyne_keep(s, (const uint8_t*)d_in, n, point_step, off_x, off_y, off_z, q_lo, q_hi, keep);
    exclusive_sum_i32(s, c->p_sort_temp, c->sort_temp_bytes, keep, pos, n);
    PRE_OUTPUT_FENCE(c);
    launch_decode_velodyne_emit(s, (const uint8_t*)d_in, n, point_step, off_x, off_y, off_z, off_intensity, keep, pos, c->d_und_in, c->p_nseg);
    return decode_finish(c, n, out_xyzit, n_out);
}
const float* immesh_decode_result(immesh_ctx* c) { return c ? c->d_und_in : nullptr; }

// ImuProcess::UndistortPcl (src/IMU_Processing.cpp:755-958): IMU forward propagation on the host, per-point compensation on the device
int immesh_undistort(immesh_ctx* c, const float* pts, int32_t n, const immesh_imu_sample* imu, int32_t n_imu, double lidar_beg_time,
                     double* last_update_time, immesh_imu_ctx* ic, double* state_inout, float* out_xyzi) {
    if (!c || !pts || n <= 0 || n > c->cap_scan || n_imu < 0 || (n_imu > 0 && !imu) || n_imu > 62 || !last_update_time || !ic || !state_inout) {
        if (c) c->err = "bad arguments (at most 62 IMU samples per package)";
        return IMMESH_E_INVAL;
    }
    (void)hipSetDevice(c->cfg.device);
    ProfBind _pb(c);
    hipStream_t s = c->stream_pre;
    const void* d_in;
    int rc = pre_resolve(c, pts, (size_t)n * 20, c->d_und_in, &d_in);
    if (rc) return rc;
    float end_curv = 0.f;   // curvature of the package's last point in arrival order (pcl_end_time, :785)
    HIPCHK(c, hipMemcpyAsync(&end_curv, (const float*)d_in + (size_t)(n - 1) * 5 + 4, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    imh::State st;
    imh::load_state(state_inout, st);
    std::vector<imh::ImuPose> poses;
    imh::imu_forward(imu, n_imu, lidar_beg_time, last_update_time, end_curv, *ic, st, poses);
    imh::store_state(st, state_inout);
    std::vector<double> tab(poses.size() * 23 + 24);
    for (size_t k = 0; k < poses.size(); k++) std::memcpy(&tab[k * 23], &poses[k], 23 * sizeof(double));
    double* fe = &tab[poses.size() * 23];
    std::memcpy(fe, st.R, 72); std::memcpy(fe + 9, st.t, 24); std::memcpy(fe + 12, ic->lid_rot_to_imu, 72); std::memcpy(fe + 21, ic->lid_offset_to_imu, 24);
    HIPCHK(c, hipMemcpyAsync(c->d_und_tab, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice, s));
    launch_undistort_keys(s, (const float*)d_in, n, c->p_slot, c->p_idx_a);
    sort_pairs_u32(s, c->p_sort_temp, c->sort_temp_bytes, c->p_slot, c->p_slot_s, c->p_idx_a, c->p_idx_c, n, 32);   // stable: equal stamps keep arrival order
    PRE_OUTPUT_FENCE(c);
    launch_undistort(s, (const float*)d_in, c->p_idx_c, n, c->d_und_tab, (int)poses.size(), c->d_und_tab + poses.size() * 23, c->d_und_out);
    if (out_xyzi) {
        HIPCHK(c, hipMemcpyAsync(out_xyzi, c->d_und_out, (size_t)n * 16, hipMemcpyDefault, s));
    }
    HIPCHK(c, hipStreamSynchronize(s));   // (also keeps `tab` alive until the upload has run)
    return 0;
}
const float* immesh_undistort_result(immesh_ctx* c) { return c ? c->d_und_out : nullptr; }

// immesh_downsample's result (c->d_ds_out, cnt leaves) to the caller's buffer, host or device memory
static int ds_copy_out(immesh_ctx* c, int32_t cnt, float* out_xyz, int32_t cap_out) {
    if (!out_xyz) return 0;
    if (cnt > cap_out) { c->err = "output buffer too small"; return IMMESH_E_CAPACITY; }
    HIPCHK(c, hipMemcpyAsync(out_xyz, c->d_ds_out, (size_t)cnt * 12, is_device_ptr(out_xyz) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c->stream_pre));
    HIPCHK(c, hipStreamSynchronize(c->stream_pre));
    return 0;
}
// a leaf the grid can be formed with: positive (a NaN is not), and float32(1 / leaf) -- the factor every cell index is taken with -- finite and not zero
static bool ds_leaf_ok(double leaf) {
    if (!(leaf > 0)) return false;
    const float inv = (float)(1.0 / leaf);
    return std::isfinite(inv) && inv > 0.f;
}
// pcl::VoxelGrid stand-in on the device (the stage before lio_state_estimation, src/voxel_mapping.cpp:1888-1891)
int immesh_downsample(immesh_ctx* c, const float* pts, int32_t n, int32_t stride, double leaf, float* out_xyz, int32_t cap_out, int32_t* n_out) {
    if (!c || !pts || n <= 0 || n > c->cap_scan || (stride != 3 && stride != 4) || !ds_leaf_ok(leaf) || !n_out) { if (c) c->err = "bad arguments"; return IMMESH_E_INVAL; }
    // the synchronous call and an asynchronous job share the pinned parameter block, the leaf table, the counters and the ticket word: between
    // immesh_downsample_begin and immesh_downsample_end the job's kernels still read them
    if (c->dsa.active) { c->err = "immesh_downsample: an asynchronous job is in flight (collect it with immesh_downsample_end first)"; return IMMESH_E_INVAL; }
    (void)hipSetDevice(c->cfg.device);
    ProfBind _pb(c);
    hipStream_t s = c->stream_pre;
    const void* d_pts;
    int rc = pre_resolve(c, pts, (size_t)n * stride * 4, stride == 4 ? (void*)c->d_pts_raw : (void*)c->d_pts_down, &d_pts);
    if (rc) return rc;
    const float inv = (float)(1.0 / leaf);   // np.float32(1.0 / leaf)
    if (!c->knobs.ds_radix && !c->ds_skip_hash) {
        // the hashed form (ds_kernels.hip: leaf table, leaf sort, point scatter + output positions, per-leaf ordered sums, publish); the radix pipeline below only when that gives up
        PRE_OUTPUT_FENCE(c);
        *c->h_ds_dyn = DsDyn{(const float*)d_pts, c->d_ds_out, n, stride, inv, 0, nullptr, 0, 0};
        launch_ds_hash_pipeline(s, c->d_ds_dyn, c->p_htab, c->p_htab_cap, c->p_idx_a, c->p_idx_b, c->p_key_b, c->p_idx_c, c->p_pool4, (int32_t*)c->p_slot, c->p_nseg + 12, c->p_nseg + 8);
        launch_ds_publish(s, c->p_nseg + 12, c->d_ds_info, c->d_ds_dyn);
        HIPCHK(c, hipStreamSynchronize(s));
        const int32_t info[2] = {c->h_ds_info[0], c->h_ds_info[1]};
        if (!info[1]) {
            *n_out = info[0];
            return ds_copy_out(c, info[0], out_xyz, cap_out);
        }
        launch_ds_table_reset(s, c->p_htab, c->p_htab_cap);   // (a cell outside the key's range, a full table or a leaf above 2048 points: the general path)
    }
    int32_t* mm = c->p_nseg;                 // 6 ints of scratch: floor(min), floor(max)
    const int init[6] = {0x7FFFFFFF, 0x7FFFFFFF, 0x7FFFFFFF, (int)0x80000000, (int)0x80000000, (int)0x80000000};
    HIPCHK(c, hipMemcpyAsync(mm, init, sizeof(init), hipMemcpyHostToDevice, s));
    launch_ds_minmax(s, (const float*)d_pts, n, stride, inv, mm);
    launch_ds_index(s, (const float*)d_pts, n, stride, inv, mm, c->p_key_a, c->p_idx_a);
    // the leaf index is below dx * dy * dz: sorting only its significant bits (typically ~24 of 64) cuts the radix passes from 8 to 3 -- worth the
    // small read-back of the grid extents
    int h_mm[6];
    HIPCHK(c, hipMemcpyAsync(h_mm, mm, sizeof(h_mm), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    int key_bits = 1;
    {
        const unsigned long long total = (unsigned long long)((long long)h_mm[3] - h_mm[0] + 1) * (unsigned long long)((long long)h_mm[4] - h_mm[1] + 1) *
                                         (unsigned long long)((long long)h_mm[5] - h_mm[2] + 1);
        while (key_bits < 64 && (total >> key_bits) != 0) key_bits++;
    }
    sort_pairs_u64(s, c->p_sort_temp, c->sort_temp_bytes, c->p_key_a, c->p_key_b, c->p_idx_a, c->p_idx_b, n, key_bits);   // stable: ties keep scan order
    launch_ds_heads(s, c->p_key_b, n, c->p_idx_c);
    exclusive_sum_i32(s, c->p_sort_temp, c->sort_temp_bytes, c->p_idx_c, c->p_idx_c, n);
    PRE_OUTPUT_FENCE(c);
    launch_ds_centroid(s, (const float*)d_pts, n, stride, c->p_key_b, c->p_idx_b, c->p_idx_c, c->d_ds_out, c->p_nseg + 8);
    int32_t cnt = 0;
    HIPCHK(c, hipMemcpyAsync(&cnt, c->p_nseg + 8, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    *n_out = cnt;
    return ds_copy_out(c, cnt, out_xyz, cap_out);
}
const float* immesh_downsample_result(immesh_ctx* c) { return c ? c->d_ds_out : nullptr; }

// ---- the asynchronous pair: the VoxelGrid of scan k+1 enqueued on the pre-processing stream beside scan k's registration, collected later.  The
// hashed form needs nothing from the host in between; when it gives up (flag in the job's pinned info) the job is redone synchronously.
// the asynchronous VoxelGrid's launch sequence (parameters are in the pinned block already)
static int ds_job_launch(immesh_ctx* c) {
    hipStream_t s = c->stream_pre;
    auto enqueue = [&]() -> int {
        launch_ds_gate(s, c->d_ds_dyn);
        launch_ds_hash_pipeline(s, c->d_ds_dyn, c->p_htab, c->p_htab_cap, c->p_idx_a, c->p_idx_b, c->p_key_b, c->p_idx_c, c->p_pool4, (int32_t*)c->p_slot, c->p_nseg + 12, c->p_nseg + 8);
        launch_ds_publish(s, c->p_nseg + 12, c->d_ds_info, c->d_ds_dyn);   // [0] leaves, [1] fall-back wanted, [2] the job's ticket -> pinned memory; device counters back to zero
        return 0;
    };
    int rc;
    if (c->knobs.no_graph || c->prof.on) { if ((rc = enqueue())) return rc; }
    else {
        // the launches never change (everything cloud-specific is in the pinned block): captured once, replayed with ONE call
        if (!c->ds_graph) {
            hipGraph_t g = nullptr;
            HIPCHK(c, hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
            const int erc = enqueue();
            const hipError_t ce = hipStreamEndCapture(s, &g);
            if (erc || ce != hipSuccess || !g) { if (g) (void)hipGraphDestroy(g); c->err = "hipGraph capture of the VoxelGrid failed"; return IMMESH_E_HIP; }
            const hipError_t ie = hipGraphInstantiate(&c->ds_graph, g, nullptr, nullptr, 0);
            (void)hipGraphDestroy(g);
            if (ie != hipSuccess) { c->ds_graph = nullptr; c->err = std::string("hipGraphInstantiate(VoxelGrid): ") + hipGetErrorString(ie); return IMMESH_E_HIP; }
        }
        HIPCHK(c, hipGraphLaunch(c->ds_graph, s));
    }
    return 0;
}
int immesh_downsample_begin(immesh_ctx* c, const float* pts, int32_t n, int32_t stride, double leaf) {
    if (!c || !pts || n <= 0 || n > c->cap_scan || (stride != 3 && stride != 4) || !ds_leaf_ok(leaf)) { if (c) c->err = "bad arguments"; return IMMESH_E_INVAL; }
    if (c->dsa.active) { c->err = "immesh_downsample_begin: the previous job has not been collected (immesh_downsample_end)"; return IMMESH_E_INVAL; }
    (void)hipSetDevice(c->cfg.device);
    ProfBind _pb(c);
    immesh_ctx::DsAsync& a = c->dsa;
    int rc;
    if (!a.ready) {   // first use: all or nothing (a failed allocation leaves the job state untouched; what was allocated stays in the context's pool)
        int32_t* info = nullptr; float* o0 = nullptr; float* o1 = nullptr; float* stg = nullptr;
        if ((rc = c->dalloc(&o0, (size_t)c->cap_scan * 3)) || (rc = c->dalloc(&o1, (size_t)c->cap_scan * 3)) || (rc = c->dalloc(&stg, (size_t)c->cap_scan * 4))) return rc;
        if ((rc = c->pinned(&info, (int32_t**)nullptr, 16))) return rc;
        const int init[6] = {0x7FFFFFFF, 0x7FFFFFFF, 0x7FFFFFFF, (int)0x80000000, (int)0x80000000, (int)0x80000000};
        std::memcpy(info + 8, init, sizeof(init));   // (pinned: the source of the asynchronous initialisation below)
        a.h_info = info; a.out[0] = o0; a.out[1] = o1; a.stage = stg; a.ready = true;   // (completion is the ticket ds_publish_kernel stores to pinned memory: no event)
    }
    hipStream_t s = c->stream_pre;
    const void* d_pts;
    // a HOST cloud is staged into the job's OWN buffer: the context's staging buffers (d_pts_raw / d_pts_down) are written by the next
    // immesh_process_scan / immesh_register with host inputs on the registration stream, which is not ordered against this stream
    if (is_device_ptr(pts)) d_pts = pts;
    else { HIPCHK(c, hipMemcpyAsync(a.stage, pts, (size_t)n * stride * 4, hipMemcpyHostToDevice, s)); d_pts = a.stage; }
    a.par ^= 1; a.n = n; a.stride = stride; a.leaf = leaf; a.d_in = d_pts;
    const float inv = (float)(1.0 / leaf);
    // six launches (a gate in front of the five that do the work), nothing the host has to look at in between (the radix pipeline needed the grid extents for its sort width): leaf table, leaf sort,
    // point scatter + output positions, per-leaf ordered sums, publish (ds_kernels.hip)
    PRE_OUTPUT_FENCE(c);   // (the buffer being written was the input of the scan before the one in flight: its point_var has to be through)
    if (++a.ticket <= 0) a.ticket = 1;
    // a scan loop (the last scan was an asynchronous immesh_process_scan): the sequence is held at its gate until the NEXT registration launch is running
    const bool gate = c->ds_gate_ok && !c->knobs.ds_no_gate && !c->knobs.serial_safe && !c->prof.on;
    *c->h_ds_dyn = DsDyn{(const float*)d_pts, a.out[a.par], n, stride, inv, a.ticket, gate ? &c->d_regstate->started : nullptr, gate ? (int32_t)(long long)(c->res_ticket + 1) : 0, 0};   // (pinned: read by thread 0 of every workgroup; the previous job has been collected)
    if ((rc = ds_job_launch(c))) return rc;
    a.active = true;
    return 0;
}
int immesh_downsample_end(immesh_ctx* c, int32_t* n_out, const float** dev_xyz) {
    if (!c || !n_out) return IMMESH_E_INVAL;
    immesh_ctx::DsAsync& a = c->dsa;
    if (!a.active) { c->err = "immesh_downsample_end: no job in flight"; return IMMESH_E_INVAL; }
    (void)hipSetDevice(c->cfg.device);
    {
        // the publishing kernel's ticket in pinned memory (bounded spin, then the stream)
        volatile int32_t* flag = c->h_ds_info + 2;
        bool held;
        if (const int rc = wait_pinned(c, c->stream_pre, [&] { return *flag == a.ticket; }, std::chrono::milliseconds(200), WAIT_NO_YIELD, &held)) return rc;
        if (c->prof.on) HIPCHK(c, hipStreamSynchronize(c->stream_pre));
        if (!held) { a.active = false; c->err = "immesh_downsample_end: the VoxelGrid launches did not complete"; return IMMESH_E_HIP; }
    }
    a.active = false;
    a.h_info[0] = c->h_ds_info[0]; a.h_info[1] = c->h_ds_info[1];
    if (a.h_info[1]) {
        // the hashed form gave up (a cell outside the key's range, a leaf above 2048 points): the general path, synchronously (it resets the table)
        int32_t cnt = 0;
        launch_ds_table_reset(c->stream_pre, c->p_htab, c->p_htab_cap);
        c->ds_skip_hash = true;
        const int rc = immesh_downsample(c, (const float*)a.d_in, a.n, a.stride, a.leaf, nullptr, 0, &cnt);
        c->ds_skip_hash = false;
        if (rc) return rc;
        HIPCHK(c, hipMemcpy(a.out[a.par], c->d_ds_out, (size_t)cnt * 12, hipMemcpyDeviceToDevice));
        a.h_info[0] = cnt;
    }
    *n_out = a.h_info[0];
    if (dev_xyz) *dev_xyz = a.out[a.par];
    return 0;
}

// void reconstruct_mesh_from_pointcloud(pcl::PointCloud<pcl::PointXYZI>::Ptr, double)   src/ImMesh_mesh_reconstruction.cpp:328-345:
// VoxelGrid(leaf) -> one package with the identity pose, frame 0 -> incremental_mesh_reconstruction
int immesh_reconstruct_mesh_from_pointcloud(immesh_ctx* c, const float* pts_xyzi, int32_t n, double leaf) {
    if (!c || !pts_xyzi || n <= 0 || n > c->cap_scan || leaf <= 0) { if (c) c->err = "bad arguments"; return IMMESH_E_INVAL; }
    int32_t n_ds = 0;
    int rc = immesh_downsample(c, pts_xyzi, n, 4, leaf, nullptr, 0, &n_ds);
    if (rc) return rc;
    (void)hipSetDevice(c->cfg.device);
    ProfBind _pb(c);
    float* world = mesh_next_world_buffer(c);
    launch_ds_expand_xyzi(c->stream, c->d_ds_out, n_ds, world);
    const double origin[3] = {0.0, 0.0, 0.0};   // pose_t of the package: Eigen::Vector3d::Zero()
    const long id = mesh_submit(c, world, n_ds, origin, 0);
    return mesh_wait(c, id);
}

}  // extern "C"
