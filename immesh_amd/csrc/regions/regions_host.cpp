// Host sequencing of the region table (include/immesh_regions.h): enable, the per-job marking hook of the mesher's phase B, table query,
// synchronisation (select -> scatter -> sort -> emit -> display positions through the smooth_pts query kernels) and fetch.
// The entries below may run on a thread of their own beside the scan loop: they follow immesh_smooth_pts' rule (launch_mu from "both mesher
// streams idle" to "results built", work on stream_q) and keep their error text in RegionsHost::err, never in immesh_ctx::err.
#include "../host_ctx.hpp"
#include "regions.hpp"
#include <algorithm>
#include <cstring>

static int rg_fail(RegionsHost* R, int rc, const std::string& msg) {
    std::lock_guard<std::mutex> lk(R->err_mu);
    R->err = msg;
    return rc;
}
#define RHIP(R, expr)                                                                                       \
    do {                                                                                                    \
        hipError_t _e = (expr);                                                                             \
        if (_e != hipSuccess) return rg_fail((R), IMMESH_E_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)

static int rg_grow_dev(RegionsHost* R, void** p, size_t* have, size_t need, const char* what) {
    if (*have >= need) return 0;
    if (*p) (void)hipFree(*p);
    *p = nullptr; *have = 0;
    const size_t want = need + need / 4 + 4096;
    if (hipMalloc(p, want) != hipSuccess) { (void)hipGetLastError(); *p = nullptr; return rg_fail(R, IMMESH_E_NOMEM, std::string("hipMalloc(") + what + ")"); }
    *have = want;
    return 0;
}
static int rg_grow_stage(RegionsHost* R, size_t need) {
    if (R->h_stage_bytes >= need) return 0;
    if (R->h_stage) (void)hipHostFree(R->h_stage);
    R->h_stage = nullptr; R->h_stage_bytes = 0;
    const size_t want = need + need / 2 + (1 << 16);
    if (hipHostMalloc((void**)&R->h_stage, want, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); R->h_stage = nullptr; return rg_fail(R, IMMESH_E_NOMEM, "hipHostMalloc(region staging)"); }
    R->h_stage_bytes = want;
    return 0;
}

int regions_create(immesh_ctx* c) {
    c->mesh_host.regions = new (std::nothrow) RegionsHost();
    if (!c->mesh_host.regions) { c->err = "out of host memory"; return IMMESH_E_NOMEM; }
    return 0;
}
void regions_free(immesh_ctx* c) {
    RegionsHost* R = c->mesh_host.regions;
    if (!R) return;
    if (R->res) (void)hipFree(R->res);
    if (R->work) (void)hipFree(R->work);
    if (R->tmp) (void)hipFree(R->tmp);
    if (R->keys_dev) (void)hipFree(R->keys_dev);
    if (R->h_stage) (void)hipHostFree(R->h_stage);
    delete R;   // (the table itself came from the context's pool)
    c->mesh_host.regions = nullptr;
}

void regions_enqueue_mark(immesh_ctx* c, const MeshDev& m, hipStream_t s, const int32_t* add_sorted) {
    const RegionsHost* R = c->mesh_host.regions;
    if (!R || !R->on) return;
    RegionsJob j;
    j.sc = m.sc; j.overflow = m.sc + SC_OVERFLOW; j.list_rem = m.list_rem; j.add_sorted = add_sorted; j.t_v = m.t_v; j.v_pos = m.v_pos;
    j.i_rem = SC_REM; j.i_add = SC_ADD; j.cap_list = m.cap_list;
    rg_launch_mark(s, R->d, j);
}

// both mesher streams idle: the map between two jobs (the caller holds launch_mu, so no job is enqueued meanwhile)
static int rg_quiesce(immesh_ctx* c, RegionsHost* R) {
    RHIP(R, hipStreamSynchronize(c->mesh_host.stream));
    RHIP(R, hipStreamSynchronize(c->mesh_host.stream_b));
    return 0;
}

// buffers of the taken regions (the snapshot -- regions_select_kernel -- has run; n_sel regions, n triangles, nv vertices)
static int rg_build(immesh_ctx* c, RegionsHost* R, hipStream_t s, int n_sel, int64_t n, int nv, double smooth_factor, double max_dis) {
    MeshHost& h = c->mesh_host;
    const MeshDev& m = c->mesh;
    const RegionsDev& d = R->d;
    int rc;
    int32_t cnt[RG_COUNTERS];
    R->sync_regions.resize((size_t)n_sel);
    if (n_sel > 0) RHIP(R, hipMemcpyAsync(R->sync_regions.data(), d.sel_info, (size_t)n_sel * sizeof(immesh_region_info), hipMemcpyDeviceToHost, s));
    if (n > 0) {
        const size_t n3 = (size_t)n * 3;
        // results: tri (n x 3) | xyz (n x 9 floats) | flip (n)
        if ((rc = rg_grow_dev(R, &R->res, &R->res_bytes, (size_t)n * (12 + 36 + 1) + 64, "region buffers"))) return rc;
        int32_t* tri = (int32_t*)R->res; float* xyz = (float*)(tri + n3); uint8_t* flip = (uint8_t*)(xyz + (size_t)n * 9);
        // scratch: three index arrays, two 64-bit key arrays | per id: voxel, sorted voxel, two dummy value arrays, voxel list
        if ((rc = rg_grow_dev(R, &R->work, &R->work_bytes, (size_t)n * (12 + 16) + n3 * 20 + 64, "region scratch"))) return rc;
        unsigned long long* k64a = (unsigned long long*)R->work; unsigned long long* k64b = k64a + n;
        int32_t* idx_a = (int32_t*)(k64b + n); int32_t* idx_b = idx_a + n; int32_t* idx_c = idx_b + n;
        int32_t* vox = idx_c + n; uint32_t* vox_s = (uint32_t*)(vox + n3); int32_t* dv_a = (int32_t*)(vox_s + n3); int32_t* dv_b = dv_a + n3; int32_t* list = dv_b + n3;
        if ((rc = rg_grow_dev(R, &R->tmp, &R->tmp_bytes, std::max(sort_pairs_u64_temp_bytes((int)n), sort_pairs_u32_temp_bytes((int)n3)) + 256, "region sort scratch"))) return rc;
        // ---- one streaming pass over the pool, then (region rank, v0, v1, v2) by two stable radix passes
        RHIP(R, hipMemsetAsync(idx_a, 0xFF, (size_t)n * 4, s));
        rg_launch_scatter(s, d, m.t_live, m.pc + PC_TRIS, idx_a, (int)n);
        rg_launch_sort_keys(s, d, m.t_v, idx_a, (int)n, 0, k64a);
        sort_pairs_u64(s, R->tmp, R->tmp_bytes, k64a, k64b, idx_a, idx_b, (int)n, 64);
        rg_launch_sort_keys(s, d, m.t_v, idx_b, (int)n, 1, k64a);
        sort_pairs_u64(s, R->tmp, R->tmp_bytes, k64a, k64b, idx_b, idx_c, (int)n, 48);
        rg_launch_emit(s, d, m.t_v, m.t_flip, idx_c, (int)n, tri, flip);
        // ---- display positions of the 3 n ids: the kernels of immesh_mesh_display_vertices, the voxel list built on the device
        launch_mesh_query_voxels(s, m, tri, (int)n3, nv, 1, vox);
        sort_pairs_u32(s, R->tmp, R->tmp_bytes, (const uint32_t*)vox, vox_s, dv_a, dv_b, (int)n3, 32);
        rg_launch_unique_voxels(s, vox_s, (int)n3, list, d.cnt + RG_NLIST);
        RHIP(R, hipMemcpyAsync(cnt, d.cnt, sizeof(cnt), hipMemcpyDeviceToHost, s));
        RHIP(R, hipStreamSynchronize(s));
        if (cnt[RG_BAD]) return rg_fail(R, IMMESH_E_HIP, "region sync: the region table and the triangle pool disagree");
        const int n_list = cnt[RG_NLIST];
        if (n_list > 0) {
            const size_t need = (size_t)std::max(nv, 1) * 24;
            if (h.q_exp_bytes < need) {   // (shared with immesh_smooth_pts: both hold launch_mu)
                if (h.q_exp) (void)hipFree(h.q_exp);
                h.q_exp = nullptr; h.q_exp_bytes = 0;
                if (hipMalloc(&h.q_exp, need + need / 4) != hipSuccess) { (void)hipGetLastError(); return rg_fail(R, IMMESH_E_NOMEM, "hipMalloc(smooth_pts)"); }
                h.q_exp_bytes = need + need / 4;
            }
            launch_mesh_query_smooth(s, m, list, n_list, smooth_factor, max_dis, (double*)h.q_exp);
        }
        launch_mesh_query_gather(s, m, tri, vox, (int)n3, (const double*)h.q_exp, 1, nullptr, xyz);
    }
    RHIP(R, hipStreamSynchronize(s));
    return 0;
}

extern "C" {

const char* immesh_mesh_regions_error(immesh_ctx* c) {
    static thread_local std::string copy;
    if (!c || !c->mesh_host.regions) return "";
    RegionsHost* R = c->mesh_host.regions;
    std::lock_guard<std::mutex> lk(R->err_mu);
    copy = R->err;
    return copy.c_str();
}

int immesh_mesh_regions_enable(immesh_ctx* c, int32_t on) {
    if (!c || !c->mesh_host.regions) return IMMESH_E_INVAL;
    RegionsHost* R = c->mesh_host.regions;
    MeshHost& h = c->mesh_host;
    std::lock_guard<std::mutex> lr(R->mu);
    {
        std::lock_guard<std::mutex> lk(h.mu);
        if (h.submitted > 0) return rg_fail(R, IMMESH_E_INVAL, "the region table is switched before the first mesh job of the context (creation order is the reference's only from an empty map)");
    }
    if (c->mesh.shard_world > 1) return rg_fail(R, IMMESH_E_INVAL, "the region table is not available on a sharded mesher (shard_world > 1)");
    if (!(c->cfg.mesh_region > 0)) return rg_fail(R, IMMESH_E_INVAL, "mesh_region must be positive");
    if (!on) { R->on = false; return 0; }
    if (R->on) return 0;
    (void)hipSetDevice(c->cfg.device);
    RegionsDev& d = R->d;
    if (!d.ent) {
        int rc;
#define A(ptr, n) if ((rc = c->dalloc(&(ptr), (size_t)(n)))) return rg_fail(R, rc, c->err)
        A(d.ent, RG_HASH_CAP); A(d.r_key, (size_t)RG_CAP_REGIONS * 3); A(d.r_nlive, RG_CAP_REGIONS); A(d.r_dirty, RG_CAP_REGIONS);
        A(d.t_region, c->mesh.cap_tris); A(d.new_slots, RG_CAP_REGIONS); A(d.cnt, RG_COUNTERS);
        A(d.sel_rank, RG_CAP_REGIONS); A(d.sel_first, RG_CAP_REGIONS); A(d.sel_fill, RG_CAP_REGIONS); A(d.sel_info, RG_CAP_REGIONS);
#undef A
        d.region_size = c->cfg.mesh_region; d.cap_tris = c->mesh.cap_tris;
        hipStream_t s = c->stream;
        RHIP(R, hipMemsetAsync(d.ent, 0xFF, (size_t)RG_HASH_CAP * sizeof(RgEnt), s));   // (key == ~0: empty, val == -1, first == 0xFFFFFFFF)
        RHIP(R, hipMemsetAsync(d.t_region, 0xFF, (size_t)d.cap_tris * 4, s));
        RHIP(R, hipMemsetAsync(d.r_nlive, 0, (size_t)RG_CAP_REGIONS * 4, s));
        RHIP(R, hipMemsetAsync(d.r_dirty, 0, (size_t)RG_CAP_REGIONS * 4, s));
        RHIP(R, hipMemsetAsync(d.cnt, 0, RG_COUNTERS * 4, s));
        RHIP(R, hipStreamSynchronize(s));
    }
    R->on = true;
    return 0;
}

int immesh_mesh_regions(immesh_ctx* c, immesh_region_info* out, int32_t cap, int32_t* n_out) {
    if (!c || !c->mesh_host.regions) return IMMESH_E_INVAL;
    RegionsHost* R = c->mesh_host.regions;
    if (!n_out) return rg_fail(R, IMMESH_E_INVAL, "bad arguments");
    if (!R->on) return rg_fail(R, IMMESH_E_INVAL, "the region table is off (immesh_mesh_regions_enable)");
    (void)hipSetDevice(c->cfg.device);
    MeshHost& h = c->mesh_host;
    std::lock_guard<std::mutex> lr(R->mu);
    int rc;
    if ((rc = rg_grow_stage(R, 64 + (size_t)RG_CAP_REGIONS * 20))) return rc;
    int32_t* h_cnt = (int32_t*)R->h_stage;
    int32_t* h_key = h_cnt + 16; int32_t* h_nl = h_key + (size_t)RG_CAP_REGIONS * 3; int32_t* h_dirty = h_nl + RG_CAP_REGIONS;
    int n = 0;
    {
        std::lock_guard<std::mutex> lq(h.launch_mu);
        if ((rc = rg_quiesce(c, R))) return rc;
        hipStream_t s = h.stream_q;
        RHIP(R, hipMemcpyAsync(h_cnt, R->d.cnt, RG_COUNTERS * 4, hipMemcpyDeviceToHost, s));
        RHIP(R, hipStreamSynchronize(s));
        n = std::min(std::max(h_cnt[RG_N], 0), RG_CAP_REGIONS);
        *n_out = n;
        if (!out || n == 0) return 0;
        if (cap < n) return rg_fail(R, IMMESH_E_CAPACITY, "output buffer too small for the region table");
        RHIP(R, hipMemcpyAsync(h_key, R->d.r_key, (size_t)n * 12, hipMemcpyDeviceToHost, s));
        RHIP(R, hipMemcpyAsync(h_nl, R->d.r_nlive, (size_t)n * 4, hipMemcpyDeviceToHost, s));
        RHIP(R, hipMemcpyAsync(h_dirty, R->d.r_dirty, (size_t)n * 4, hipMemcpyDeviceToHost, s));
        RHIP(R, hipStreamSynchronize(s));
    }
    for (int r = 0; r < n; r++) {
        immesh_region_info& q = out[r];
        q.key[0] = h_key[(size_t)r * 3 + 0]; q.key[1] = h_key[(size_t)r * 3 + 1]; q.key[2] = h_key[(size_t)r * 3 + 2];
        q.index = r; q.n_triangles = h_nl[r]; q.dirty = h_dirty[r] ? 1 : 0; q.first = 0;
    }
    return 0;
}

int immesh_mesh_regions_sync(immesh_ctx* c, double smooth_factor, int32_t knn, double max_dis, int32_t force_all, int32_t* n_regions_out, int64_t* n_triangles_out) {
    if (!c || !c->mesh_host.regions) return IMMESH_E_INVAL;
    RegionsHost* R = c->mesh_host.regions;
    if (!R->on) return rg_fail(R, IMMESH_E_INVAL, "the region table is off (immesh_mesh_regions_enable)");
    if (knn != MV_KNN) return rg_fail(R, IMMESH_E_INVAL, "region sync: only knn = 20 (the reference's g_ply_smooth_k) is supported");
    MeshHost& h = c->mesh_host;
    const MeshDev& m = c->mesh;
    if (max_dis <= 0) max_dis = m.voxel * 0.8;   // (pointcloud_rgbd.cpp:940-943)
    if (!(max_dis <= m.accept * 2.0)) return rg_fail(R, IMMESH_E_INVAL, "region sync: maximum_smooth_dis above 2.5 x the mesh voxel (the search radius of the device's 20-NN pull)");
    (void)hipSetDevice(c->cfg.device);
    std::lock_guard<std::mutex> lr(R->mu);
    std::lock_guard<std::mutex> lq(h.launch_mu);
    int rc;
    if ((rc = rg_quiesce(c, R))) return rc;
    hipStream_t s = h.stream_q;
    const RegionsDev& d = R->d;
    R->have_sync = false;
    // ---- snapshot: taken regions, ranks, offsets; flags cleared
    rg_launch_select(s, d, force_all ? 1 : 0);
    int32_t cnt[RG_COUNTERS], pc[PC_COUNT];
    RHIP(R, hipMemcpyAsync(cnt, d.cnt, sizeof(cnt), hipMemcpyDeviceToHost, s));
    RHIP(R, hipMemcpyAsync(pc, m.pc, sizeof(pc), hipMemcpyDeviceToHost, s));
    RHIP(R, hipStreamSynchronize(s));
    const int n_sel = cnt[RG_SEL_REGIONS];
    const int64_t n = cnt[RG_SEL_TRIS];
    const int nv = pc[PC_VERTS];
    if (n_sel < 0 || n_sel > RG_CAP_REGIONS || n < 0 || n > (int64_t)m.cap_tris) return rg_fail(R, IMMESH_E_HIP, "region sync: corrupt selection counters");
    if ((rc = rg_build(c, R, s, n_sel, n, nv, smooth_factor, max_dis))) {
        if (n_sel > 0) { rg_launch_redirty(s, d, n_sel); (void)hipStreamSynchronize(s); }   // the taken regions stay dirty: nothing is lost
        return rc;
    }
    R->sync_tris = n;
    R->have_sync = true;
    if (n_regions_out) *n_regions_out = n_sel;
    if (n_triangles_out) *n_triangles_out = n;
    return 0;
}

int immesh_mesh_regions_fetch(immesh_ctx* c, immesh_region_info* regions, int32_t* tri, uint8_t* flip, float* xyz) {
    if (!c || !c->mesh_host.regions) return IMMESH_E_INVAL;
    RegionsHost* R = c->mesh_host.regions;
    if (!R->on) return rg_fail(R, IMMESH_E_INVAL, "the region table is off (immesh_mesh_regions_enable)");
    (void)hipSetDevice(c->cfg.device);
    std::lock_guard<std::mutex> lr(R->mu);
    if (!R->have_sync) return rg_fail(R, IMMESH_E_INVAL, "no finished immesh_mesh_regions_sync to fetch from");
    if (regions && !R->sync_regions.empty()) std::memcpy(regions, R->sync_regions.data(), R->sync_regions.size() * sizeof(immesh_region_info));
    const size_t n = (size_t)R->sync_tris;
    if (n == 0 || (!tri && !flip && !xyz)) return 0;
    const int32_t* d_tri = (const int32_t*)R->res; const float* d_xyz = (const float*)(d_tri + n * 3); const uint8_t* d_flip = (const uint8_t*)(d_xyz + n * 9);
    struct Part { void* dst; const void* src; size_t bytes; };
    const Part parts[3] = {{tri, d_tri, n * 12}, {xyz, d_xyz, n * 36}, {flip, d_flip, n}};
    size_t total = 0;
    for (const Part& q : parts) if (q.dst) total += (q.bytes + 63) & ~(size_t)63;
    int rc;
    if ((rc = rg_grow_stage(R, total))) return rc;
    hipStream_t s = c->mesh_host.stream_q;
    size_t off = 0;
    for (const Part& q : parts) if (q.dst) { RHIP(R, hipMemcpyAsync(R->h_stage + off, q.src, q.bytes, hipMemcpyDeviceToHost, s)); off += (q.bytes + 63) & ~(size_t)63; }
    RHIP(R, hipStreamSynchronize(s));
    off = 0;
    for (const Part& q : parts) if (q.dst) { std::memcpy(q.dst, R->h_stage + off, q.bytes); off += (q.bytes + 63) & ~(size_t)63; }
    return 0;
}

int immesh_region_keys(immesh_ctx* c, const float* vtx_xyz, int64_t n_vtx, const int32_t* tri, int64_t n_tri, int32_t* keys_out) {
    if (!c || !c->mesh_host.regions) return IMMESH_E_INVAL;
    RegionsHost* R = c->mesh_host.regions;
    if (n_tri < 0 || n_vtx < 0 || (n_tri > 0 && (!vtx_xyz || !tri || !keys_out)) || n_tri > (1ll << 28) || n_vtx > (1ll << 30)) return rg_fail(R, IMMESH_E_INVAL, "bad arguments");
    if (!(c->cfg.mesh_region > 0)) return rg_fail(R, IMMESH_E_INVAL, "mesh_region must be positive");
    if (n_tri == 0) return 0;
    for (int64_t i = 0; i < n_tri * 3; i++) if (tri[i] < 0 || tri[i] >= n_vtx) return rg_fail(R, IMMESH_E_INVAL, "region keys: vertex index out of range");
    (void)hipSetDevice(c->cfg.device);
    std::lock_guard<std::mutex> lr(R->mu);
    int rc;
    const size_t bv = ((size_t)n_vtx * 12 + 63) & ~(size_t)63, bt = ((size_t)n_tri * 12 + 63) & ~(size_t)63;
    if ((rc = rg_grow_dev(R, &R->keys_dev, &R->keys_bytes, bv + 2 * bt, "region keys"))) return rc;
    if ((rc = rg_grow_stage(R, bv + 2 * bt))) return rc;
    char* dv = (char*)R->keys_dev;
    hipStream_t s = c->mesh_host.stream_q;
    std::memcpy(R->h_stage, vtx_xyz, (size_t)n_vtx * 12);
    std::memcpy(R->h_stage + bv, tri, (size_t)n_tri * 12);
    RHIP(R, hipMemcpyAsync(dv, R->h_stage, bv + bt, hipMemcpyHostToDevice, s));
    rg_launch_keys(s, (const float*)dv, (const int32_t*)(dv + bv), n_tri, c->cfg.mesh_region, (int32_t*)(dv + bv + bt));
    RHIP(R, hipMemcpyAsync(R->h_stage + bv + bt, dv + bv + bt, (size_t)n_tri * 12, hipMemcpyDeviceToHost, s));
    RHIP(R, hipStreamSynchronize(s));
    std::memcpy(keys_out, R->h_stage + bv + bt, (size_t)n_tri * 12);
    return 0;
}

}  // extern "C"
