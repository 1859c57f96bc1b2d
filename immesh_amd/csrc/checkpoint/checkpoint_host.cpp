// Host side of the checkpoints (include/immesh_checkpoint.h): the file's layout, its validation (immesh_checkpoint_probe, shared by load), the
// quiesce, and the streaming of the sections between device memory and the file through two pinned staging buffers -- the copy of chunk k+1 runs
// beside the file thread's write of chunk k (load: the mirror image).  Everything is allocated for the call and released before it returns.
#include "../host_ctx.hpp"
#include "../regions/regions.hpp"
#include "../colour/colour.hpp"
#include "checkpoint.hpp"
#include <algorithm>
#include <cerrno>
#include <condition_variable>
#include <cstring>
#include <fcntl.h>
#include <mutex>
#include <sys/stat.h>
#include <thread>
#include <unistd.h>

namespace {

using clk = std::chrono::steady_clock;
double ms_since(clk::time_point t0) { return std::chrono::duration<double, std::milli>(clk::now() - t0).count(); }

const char* const ck_rec_names[CK_N_REC] = {"sizeof(NodeRec)", "sizeof(HashEnt)", "sizeof(MeshGridEnt)", "sizeof(MeshVoxEnt)", "sizeof(RgEnt)", "MV_VOX_CAP", "MV_ADJ_STRIDE",
                                            "IM_CHUNK_PTS", "IM_PT_DOUBLES", "IM_EXT_CHUNKS", "leaf chunk words", "sizeof(immesh_counters_t)", "SC_COUNT", "PC_COUNT",
                                            "MESH_NPAR", "STATS_WORDS"};
void ck_rec_values(int32_t* r) {
    const int32_t v[CK_N_REC] = {(int32_t)sizeof(NodeRec), (int32_t)sizeof(HashEnt), (int32_t)sizeof(MeshGridEnt), (int32_t)sizeof(MeshVoxEnt), (int32_t)sizeof(RgEnt), MV_VOX_CAP,
                                 MV_ADJ_STRIDE, IM_CHUNK_PTS, IM_PT_DOUBLES, IM_EXT_CHUNKS, IM_LEAF_SLOTS + 1, (int32_t)sizeof(immesh_counters_t), SC_COUNT, PC_COUNT,
                                 MESH_NPAR, STATS_WORDS};
    std::memcpy(r, v, sizeof(v));
}

// the host's share of the state: one small section
struct CkHostState {
    immesh_counters_t cnt;       // immesh_ctx::cnt
    int64_t cum[SC_COUNT];       // MeshHost::cum
    int64_t n_live, jobs;        // MeshHost::n_live; MeshHost::submitted (== completed: the save drained the queue)
    int32_t seq, n_vertices;     // MeshHost::seq, ::n_vertices
    int32_t upd_seq, pad;        // RegMapDev::upd_seq
};

uint64_t ck_checksum_host(const void* data, size_t bytes, uint64_t first_word = 0) {
    const unsigned char* b = (const unsigned char*)data;
    uint64_t sum = 0;
    const size_t full = bytes >> 3;
    for (size_t i = 0; i < full; i++) { uint64_t w; std::memcpy(&w, b + 8 * i, 8); sum += imd::hash64(w ^ ((first_word + i) * 0x9E3779B97F4A7C15ull)); }
    if (bytes & 7) { uint64_t w = 0; std::memcpy(&w, b + 8 * full, bytes & 7); sum += imd::hash64(w ^ ((first_word + full) * 0x9E3779B97F4A7C15ull)); }
    return sum;
}

struct CkSpec {
    char name[24];
    int64_t elem, records;
    char* ptr;        // where the section lies (device memory, or host memory with `host`); null: a table part before its staging exists, or skipped
    bool host;
    int table, part;  // table >= 0: part 0 = slot indices, 1 = entries
    int64_t bytes() const { return elem * records; }
};

const char* const ck_table_names[CK_N_TABLES] = {"reg.hash", "mesh.grid", "mesh.vox", "mesh.thash", "rg.hash"};

// The sections of a file with this header, in file order; with a context, where each lies.  ONE list for save, probe and load.
std::vector<CkSpec> ck_sections(const CkFileHeader& h, const int64_t* tab, immesh_ctx* c, immesh_colourer* col, CkHostState* hs) {
    std::vector<CkSpec> v;
    auto D = [&](const char* name, int64_t elem, int64_t n, const void* p, bool host = false) {
        CkSpec s{};
        std::strncpy(s.name, name, sizeof(s.name) - 1);
        s.elem = elem; s.records = n; s.ptr = (char*)p; s.host = host; s.table = -1; s.part = 0;
        v.push_back(s);
    };
    auto T = [&](int t) {
        const std::string base = ck_table_names[t];
        D((base + ".slot").c_str(), 4, tab[t], nullptr); v.back().table = t; v.back().part = 0;
        D((base + ".ent").c_str(), ck_table_entry_bytes(t), tab[t], nullptr); v.back().table = t; v.back().part = 1;
    };
    const int64_t* n = h.counts;
    const RegMapDev* m = c ? &c->map : nullptr;
    const MeshDev* q = c ? &c->mesh : nullptr;
#define P(x) (c ? (const void*)(x) : nullptr)
    D("reg.counters", 4, 16, P(m->counters));
    D("reg.stats", 8, STATS_WORDS, P(c->d_stats));
    T(CKT_REG);
    D("reg.nodes", sizeof(NodeRec), n[CKC_NODES], P(m->nodes));
    D("reg.chunks", (int64_t)IM_CHUNK_PTS * IM_PT_DOUBLES * 8, n[CKC_CHUNKS], P(m->chunk_data));
    D("reg.ext", (int64_t)IM_EXT_CHUNKS * 4, n[CKC_EXT], P(m->ext_tables));
    D("reg.leaf", (IM_LEAF_SLOTS + 1) * 4, n[CKC_LEAF], P(m->leaf_chunks));
    D("reg.free_ready", 4, n[CKC_FREE_READY], P(m->free_ready));
    D("reg.free_pending", 4, n[CKC_FREE_PENDING], P(m->free_pending));
    D("mesh.pc", 4, PC_COUNT, P(q->pc));
    D("mesh.v_pos", 12, n[CKC_VERTS], P(q->v_pos));
    D("mesh.v_smooth", 24, n[CKC_VERTS], P(q->v_smooth));
    D("mesh.v_voxel", 4, n[CKC_VERTS], P(q->v_voxel));
    T(CKT_GRID);
    T(CKT_VOX);
    D("mesh.vx_key", 8, n[CKC_VOXELS], P(q->vx_key));
    D("mesh.vx_npts", 4, n[CKC_VOXELS], P(q->vx_npts));
    D("mesh.vx_pts", (int64_t)MV_VOX_CAP * 4, n[CKC_VOXELS], P(q->vx_pts));
    D("mesh.vx_meshing_times", 4, n[CKC_VOXELS], P(q->vx_meshing_times));
    D("mesh.vx_new_added", 4, n[CKC_VOXELS], P(q->vx_new_added));
    D("mesh.vx_stamp", 4, n[CKC_VOXELS], P(q->vx_stamp));
    for (int p = 0; p < MESH_NPAR; p++) D(("mesh.vx_rank_seq" + std::to_string(p)).c_str(), 4, n[CKC_VOXELS], P(c->mesh_host.mpar[p].vx_rank_seq));
    D("mesh.vx_short_axis", 24, n[CKC_VOXELS], P(q->vx_short_axis));
    D("mesh.t_v", 12, n[CKC_TRIS], P(q->t_v));
    D("mesh.t_word", 8, n[CKC_TRIS], P(q->t_word));
    D("mesh.t_live", 4, n[CKC_TRIS], P(q->t_live));
    D("mesh.t_rem_seq", 4, n[CKC_TRIS], P(q->t_rem_seq));
    D("mesh.t_flip", 1, n[CKC_TRIS], P(q->t_flip));
    T(CKT_TRI);
    D("mesh.a_head", 4, n[CKC_VERTS], P(q->a_head));
    D("mesh.a_chunks", (int64_t)MV_ADJ_STRIDE * 4, n[CKC_ADJ], P(q->a_chunks));
    D("host.state", sizeof(CkHostState), 1, hs, true);
    if (h.has_regions) {
        const RegionsDev* d = (c && c->mesh_host.regions && c->mesh_host.regions->d.ent) ? &c->mesh_host.regions->d : nullptr;
#define PR(x) (d ? (const void*)(x) : nullptr)
        D("rg.cnt", 4, RG_COUNTERS, PR(d->cnt));
        T(CKT_REGION);
        D("rg.r_key", 12, n[CKC_REGIONS], PR(d->r_key));
        D("rg.r_nlive", 4, n[CKC_REGIONS], PR(d->r_nlive));
        D("rg.r_dirty", 4, n[CKC_REGIONS], PR(d->r_dirty));
        D("rg.t_region", 4, n[CKC_TRIS], PR(d->t_region));
#undef PR
    }
    if (h.has_colour) {
        const ClState* st = col ? &cl_colourer_state(col) : nullptr;
        for (int k = 0; k < 3; k++) D(("cl.rgb" + std::to_string(k)).c_str(), 8, n[CKC_VERTS], st ? st->rgb[k] : nullptr);
        for (int k = 0; k < 3; k++) D(("cl.cov" + std::to_string(k)).c_str(), 8, n[CKC_VERTS], st ? st->cov[k] : nullptr);
        D("cl.first_exposure", 8, n[CKC_VERTS], st ? st->first_exposure : nullptr);
        D("cl.obs_dis", 8, n[CKC_VERTS], st ? st->obs_dis : nullptr);
        D("cl.last_obs_time", 8, n[CKC_VERTS], st ? st->last_obs_time : nullptr);
        D("cl.n_obs", 4, n[CKC_VERTS], st ? st->n_obs : nullptr);
    }
#undef P
    return v;
}

int64_t align_up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }

void ck_fill_info(const CkFileHeader& h, immesh_checkpoint_info* info) {
    if (!info) return;
    std::memset(info, 0, sizeof(*info));
    info->version = h.version; info->n_sections = h.n_sections; info->has_regions = h.has_regions; info->has_colour = h.has_colour;
    info->file_bytes = h.file_bytes; info->cfg = h.cfg;
    const int64_t* n = h.counts;
    info->n_root_voxels = n[CKC_ROOTS]; info->n_nodes = n[CKC_NODES]; info->n_point_chunks = n[CKC_CHUNKS]; info->n_free_chunks = n[CKC_FREE_READY] + n[CKC_FREE_PENDING];
    info->n_ext_tables = n[CKC_EXT]; info->n_leaf_chunks = n[CKC_LEAF]; info->n_vertices = n[CKC_VERTS]; info->n_mesh_voxels = n[CKC_VOXELS];
    info->n_triangles_pool = n[CKC_TRIS]; info->n_triangles_live = n[CKC_LIVE]; info->n_adj_chunks = n[CKC_ADJ]; info->n_regions = n[CKC_REGIONS];
    info->scans_meshed = n[CKC_SCANS_MESHED]; info->map_updates = n[CKC_MAP_UPDATES];
}

bool read_all(int fd, void* dst, size_t n, int64_t off) {
    char* p = (char*)dst;
    while (n) {
        const ssize_t r = pread(fd, p, n, (off_t)off);
        if (r < 0 && errno == EINTR) continue;
        if (r <= 0) return false;
        p += r; n -= (size_t)r; off += r;
    }
    return true;
}
bool write_all(int fd, const void* src, size_t n, int64_t off) {
    const char* p = (const char*)src;
    while (n) {
        const ssize_t r = pwrite(fd, p, n, (off_t)off);
        if (r < 0 && errno == EINTR) continue;
        if (r <= 0) return false;
        p += r; n -= (size_t)r; off += r;
    }
    return true;
}

// Header and section table of the file behind `fd`, validated.  Every refusal names its fault.
int ck_probe_fd(int fd, CkFileHeader& h, std::vector<immesh_checkpoint_section>& secs, std::string& err) {
    struct stat sb;
    if (fstat(fd, &sb) != 0) { err = std::string("fstat: ") + std::strerror(errno); return IMMESH_E_IO; }
    const int64_t len = (int64_t)sb.st_size;
    if (len < (int64_t)sizeof(CkFileHeader)) { err = "truncated: the file is shorter than a checkpoint header"; return IMMESH_E_FORMAT; }
    if (!read_all(fd, &h, sizeof(h), 0)) { err = std::string("read: ") + std::strerror(errno); return IMMESH_E_IO; }
    if (std::memcmp(h.magic, "IMMESHCK", 8) != 0) { err = "not a checkpoint (magic)"; return IMMESH_E_FORMAT; }
    if (h.version != IMMESH_CHECKPOINT_VERSION) { err = "version " + std::to_string(h.version) + ", this library reads version " + std::to_string(IMMESH_CHECKPOINT_VERSION); return IMMESH_E_FORMAT; }
    if (h.header_bytes != (int32_t)sizeof(CkFileHeader) || h.section_bytes != (int32_t)sizeof(immesh_checkpoint_section)) { err = "header or section entry size differs from this library's"; return IMMESH_E_FORMAT; }
    int32_t rec[CK_N_REC];
    ck_rec_values(rec);
    for (int i = 0; i < CK_N_REC; i++)
        if (h.rec[i] != rec[i]) { err = std::string("record size ") + ck_rec_names[i] + ": file " + std::to_string(h.rec[i]) + ", library " + std::to_string(rec[i]); return IMMESH_E_FORMAT; }
    if (h.file_bytes != len) { err = "file length " + std::to_string(len) + ", the header says " + std::to_string(h.file_bytes) + " (truncated?)"; return IMMESH_E_FORMAT; }
    const int64_t table_end = (int64_t)sizeof(CkFileHeader) + (int64_t)h.n_sections * (int64_t)sizeof(immesh_checkpoint_section);
    if (h.n_sections < 1 || h.n_sections > 256 || h.payload_offset < table_end || h.payload_offset > len || h.payload_offset % 8) { err = "section count or payload offset out of range"; return IMMESH_E_FORMAT; }
    for (int i = 0; i < CK_N_COUNT; i++) if (h.counts[i] < 0 || h.counts[i] > 0x7fffffffLL) { err = "count " + std::to_string(i) + " out of range"; return IMMESH_E_FORMAT; }
    secs.resize((size_t)h.n_sections);
    if (!read_all(fd, secs.data(), secs.size() * sizeof(secs[0]), sizeof(CkFileHeader))) { err = std::string("read: ") + std::strerror(errno); return IMMESH_E_IO; }
    auto nm = [](const immesh_checkpoint_section& s) { return std::string(s.name, strnlen(s.name, sizeof(s.name))); };
    for (const auto& s : secs) {
        if (s.offset < h.payload_offset || s.offset % 8 || s.bytes < 0 || s.records < 0) { err = "section " + nm(s) + " has an invalid offset or size"; return IMMESH_E_FORMAT; }
        if (s.offset > len || s.bytes > len - s.offset) { err = "section " + nm(s) + " runs past the end of the file"; return IMMESH_E_FORMAT; }
    }
    {
        std::vector<int> ord(secs.size());
        for (size_t i = 0; i < ord.size(); i++) ord[i] = (int)i;
        std::sort(ord.begin(), ord.end(), [&](int a, int b) { return secs[a].offset != secs[b].offset ? secs[a].offset < secs[b].offset : a < b; });
        for (size_t i = 1; i < ord.size(); i++) {
            const auto &a = secs[ord[i - 1]], &b = secs[ord[i]];
            if (a.bytes > 0 && b.bytes > 0 && a.offset + a.bytes > b.offset) { err = "sections " + nm(a) + " and " + nm(b) + " overlap"; return IMMESH_E_FORMAT; }
        }
    }
    // the table against the list this header implies (names, order, record counts, bytes)
    int64_t tab[CK_N_TABLES] = {0, 0, 0, 0, 0};
    for (const auto& s : secs)
        for (int t = 0; t < CK_N_TABLES; t++) if (nm(s) == std::string(ck_table_names[t]) + ".slot") tab[t] = s.records;
    const std::vector<CkSpec> want = ck_sections(h, tab, nullptr, nullptr, nullptr);
    if (want.size() != secs.size()) { err = "sections inconsistent: " + std::to_string(secs.size()) + " in the table, the header implies " + std::to_string(want.size()); return IMMESH_E_FORMAT; }
    for (size_t i = 0; i < want.size(); i++)
        if (nm(secs[i]) != want[i].name || secs[i].records != want[i].records || secs[i].bytes != want[i].bytes()) {
            err = "sections inconsistent: entry " + std::to_string(i) + " is " + nm(secs[i]) + " (" + std::to_string(secs[i].records) + " records, " + std::to_string(secs[i].bytes) +
                  " bytes), the header implies " + want[i].name + " (" + std::to_string(want[i].records) + " records, " + std::to_string(want[i].bytes()) + " bytes)";
            return IMMESH_E_FORMAT;
        }
    {
        CkFileHeader z = h;
        z.header_checksum = 0;
        const uint64_t sum = ck_checksum_host(&z, sizeof(z)) + ck_checksum_host(secs.data(), secs.size() * sizeof(secs[0]), sizeof(z) / 8);
        if (sum != h.header_checksum) { err = "checksum mismatch in the header or the section table: computed " + std::to_string(sum) + ", stored " + std::to_string(h.header_checksum); return IMMESH_E_FORMAT; }
    }
    return 0;
}

// Two pinned staging buffers between the thread that copies (device side) and the thread that reads or writes the file.  Chunk k is bytes
// [k * CK_STAGE_BYTES, ...) of the payload and lives in buffer k % 2.
struct CkPipe {
    char* buf[2] = {nullptr, nullptr};
    bool full[2] = {false, false};
    std::mutex mu;
    std::condition_variable cv;
    bool failed = false, abort = false;
    std::string err;
    double file_ms = 0;
    std::thread th;
    int64_t n_chunks = 0;

    int64_t chunk_len(int64_t k, int64_t total) const { return std::min<int64_t>((int64_t)CK_STAGE_BYTES, total - k * (int64_t)CK_STAGE_BYTES); }
    void start(bool writing, int fd, int64_t payload_offset, int64_t total) {
        n_chunks = (total + (int64_t)CK_STAGE_BYTES - 1) / (int64_t)CK_STAGE_BYTES;
        th = std::thread([=] {
            for (int64_t k = 0; k < n_chunks; k++) {
                const int b = (int)(k & 1);
                {
                    std::unique_lock<std::mutex> lk(mu);
                    cv.wait(lk, [&] { return abort || full[b] == writing; });
                    if (abort) return;
                }
                const auto t0 = clk::now();
                const int64_t off = payload_offset + k * (int64_t)CK_STAGE_BYTES;
                const size_t n = (size_t)chunk_len(k, total);
                const bool ok = writing ? write_all(fd, buf[b], n, off) : read_all(fd, buf[b], n, off);
                file_ms += ms_since(t0);
                {
                    std::lock_guard<std::mutex> lk(mu);
                    if (!ok) { failed = true; err = std::string(writing ? "write: " : "read: ") + (errno ? std::strerror(errno) : "short file"); }
                    full[b] = !writing;
                }
                cv.notify_all();
                if (!ok) return;
            }
        });
    }
    // the copying thread: wait until buffer b is `want_full`; false when the file thread failed
    bool acquire(int b, bool want_full) {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return failed || full[b] == want_full; });
        return !failed;
    }
    void release(int b, bool now_full) {
        { std::lock_guard<std::mutex> lk(mu); full[b] = now_full; }
        cv.notify_all();
    }
    void finish(bool give_up) {
        if (give_up) { { std::lock_guard<std::mutex> lk(mu); abort = true; } cv.notify_all(); }
        if (th.joinable()) th.join();
    }
};

// everything a call allocates, released when it returns
struct CkScratch {
    std::vector<void*> dev;
    char* stage[2] = {nullptr, nullptr};
    int fd = -1;
    ~CkScratch() {
        for (void* p : dev) (void)hipFree(p);
        for (char* p : stage) if (p) (void)hipHostFree(p);
        if (fd >= 0) close(fd);
    }
    int alloc(immesh_ctx* c, void** out, size_t bytes) {
        void* p = nullptr;
        if (hipMalloc(&p, bytes ? bytes : 16) != hipSuccess) { (void)hipGetLastError(); c->err = "checkpoint: hipMalloc(" + std::to_string(bytes) + " B) failed"; return IMMESH_E_NOMEM; }
        dev.push_back(p);
        *out = p;
        return 0;
    }
    int staging(immesh_ctx* c) {
        for (char*& p : stage)
            if (hipHostMalloc((void**)&p, CK_STAGE_BYTES, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); p = nullptr; c->err = "checkpoint: hipHostMalloc(staging) failed"; return IMMESH_E_NOMEM; }
        return 0;
    }
};

struct CkPlaced { CkSpec spec; int64_t offset; };   // offset: relative to the payload's first byte

// Move the payload between the sections' memory and the file, chunk by chunk.  A section without an address is skipped (load: left out; its bytes are read
// and dropped).  *copy_ms: time this thread spent issuing and waiting for copies.
int ck_stream(immesh_ctx* c, hipStream_t s, bool saving, int fd, int64_t payload_offset, int64_t total, const std::vector<CkPlaced>& secs, CkScratch& scr, double* copy_ms, double* file_ms) {
    CkPipe pipe;
    pipe.buf[0] = scr.stage[0]; pipe.buf[1] = scr.stage[1];
    pipe.start(saving, fd, payload_offset, total);
    int rc = 0;
    for (int64_t k = 0; k < pipe.n_chunks && !rc; k++) {
        const int b = (int)(k & 1);
        if (!pipe.acquire(b, !saving)) break;
        const auto t0 = clk::now();
        const int64_t lo = k * (int64_t)CK_STAGE_BYTES, hi = lo + pipe.chunk_len(k, total);
        int64_t cursor = lo;   // save: everything between the sections is written as zeros
        for (const CkPlaced& p : secs) {
            const int64_t a = std::max(lo, p.offset), e = std::min(hi, p.offset + p.spec.bytes());
            if (a >= e) continue;
            char* stage = pipe.buf[b] + (a - lo);
            if (saving && a > cursor) std::memset(pipe.buf[b] + (cursor - lo), 0, (size_t)(a - cursor));
            cursor = std::max(cursor, e);
            if (!p.spec.ptr) { if (saving) std::memset(stage, 0, (size_t)(e - a)); continue; }
            char* mem = p.spec.ptr + (a - p.offset);
            hipError_t he = hipSuccess;
            if (p.spec.host) { if (saving) std::memcpy(stage, mem, (size_t)(e - a)); else std::memcpy(mem, stage, (size_t)(e - a)); }
            else if (saving) he = hipMemcpyAsync(stage, mem, (size_t)(e - a), hipMemcpyDeviceToHost, s);
            else he = hipMemcpyAsync(mem, stage, (size_t)(e - a), hipMemcpyHostToDevice, s);
            if (he != hipSuccess) { c->err = std::string("checkpoint: hipMemcpyAsync: ") + hipGetErrorString(he); rc = IMMESH_E_HIP; break; }
        }
        if (saving && hi > cursor) std::memset(pipe.buf[b] + (cursor - lo), 0, (size_t)(hi - cursor));
        const hipError_t se = hipStreamSynchronize(s);
        if (!rc && se != hipSuccess) { c->err = std::string("checkpoint: hipStreamSynchronize: ") + hipGetErrorString(se); rc = IMMESH_E_HIP; }
        *copy_ms += ms_since(t0);
        if (!rc) pipe.release(b, saving);
    }
    pipe.finish(rc != 0);
    *file_ms += pipe.file_ms;
    if (!rc && pipe.failed) { c->err = "checkpoint: " + pipe.err; rc = IMMESH_E_IO; }
    return rc;
}

#define CKHIP(c, expr)                                                                                      \
    do {                                                                                                    \
        hipError_t _e = (expr);                                                                             \
        if (_e != hipSuccess) { (c)->err = std::string("checkpoint: " #expr ": ") + hipGetErrorString(_e); return IMMESH_E_HIP; } \
    } while (0)

struct CkTableRef { void* ents; uint64_t n_slots; };
void ck_tables(immesh_ctx* c, CkTableRef* t) {
    t[CKT_REG] = {c->map.htab, c->map.hmask + 1};
    t[CKT_GRID] = {c->mesh.g_ent, c->mesh.g_mask + 1};
    t[CKT_VOX] = {c->mesh.x_ent, c->mesh.x_mask + 1};
    t[CKT_TRI] = {c->mesh.th_slots, c->mesh.th_mask + 1};
    const RegionsHost* R = c->mesh_host.regions;
    t[CKT_REGION] = {R && R->d.ent ? (void*)R->d.ent : nullptr, (uint64_t)RG_HASH_CAP};
}

// checksums of the sections that lie in device memory (d_sums[i]) and of the host's section, into sums[]
int ck_checksums(immesh_ctx* c, hipStream_t s, const std::vector<CkPlaced>& secs, CkScratch& scr, std::vector<uint64_t>& sums) {
    unsigned long long *d_sums = nullptr, *d_part = nullptr;
    int rc;
    if ((rc = scr.alloc(c, (void**)&d_sums, secs.size() * 8)) || (rc = scr.alloc(c, (void**)&d_part, 1024 * 8))) return rc;
    CKHIP(c, hipMemsetAsync(d_sums, 0, secs.size() * 8, s));
    for (size_t i = 0; i < secs.size(); i++) {
        const CkSpec& p = secs[i].spec;
        if (p.ptr && !p.host && p.bytes() > 0) ck_launch_checksum(s, p.ptr, (size_t)p.bytes(), d_part, d_sums + i);
    }
    sums.assign(secs.size(), 0);
    CKHIP(c, hipMemcpyAsync(sums.data(), d_sums, secs.size() * 8, hipMemcpyDeviceToHost, s));
    CKHIP(c, hipStreamSynchronize(s));
    CKHIP(c, hipGetLastError());
    for (size_t i = 0; i < secs.size(); i++)
        if (secs[i].spec.ptr && secs[i].spec.host) sums[i] = ck_checksum_host(secs[i].spec.ptr, (size_t)secs[i].spec.bytes());
    return 0;
}

// both mesher streams idle, nothing pending on the registration stream: the caller holds launch_mu (and the region table's mutex)
int ck_quiesce(immesh_ctx* c) {
    CKHIP(c, hipStreamSynchronize(c->stream));
    CKHIP(c, hipStreamSynchronize(c->mesh_host.stream));
    CKHIP(c, hipStreamSynchronize(c->mesh_host.stream_b));
    return 0;
}

}  // namespace

extern "C" {

int immesh_checkpoint_probe(const char* path, immesh_checkpoint_info* info, immesh_checkpoint_section* sections, int32_t cap, char* err, int32_t err_cap) {
    auto say = [&](const std::string& m) { if (err && err_cap > 0) { std::strncpy(err, m.c_str(), (size_t)err_cap - 1); err[err_cap - 1] = 0; } };
    say("");
    if (!path) { say("path is NULL"); return IMMESH_E_INVAL; }
    const int fd = open(path, O_RDONLY | O_CLOEXEC);
    if (fd < 0) { say(std::string("cannot open ") + path + ": " + std::strerror(errno)); return IMMESH_E_IO; }
    CkFileHeader h;
    std::vector<immesh_checkpoint_section> secs;
    std::string e;
    const int rc = ck_probe_fd(fd, h, secs, e);
    close(fd);
    if (rc) { say(e); return rc; }
    ck_fill_info(h, info);
    for (int i = 0; sections && i < cap && i < (int)secs.size(); i++) sections[i] = secs[(size_t)i];
    return 0;
}

int immesh_checkpoint_save(immesh_ctx* c, immesh_colourer* col, const char* path, immesh_checkpoint_info* info) {
    if (!c) return IMMESH_E_INVAL;
    if (!path || !*path) { c->err = "checkpoint: path is empty"; return IMMESH_E_INVAL; }
    if (col && cl_colourer_ctx(col) != c) { c->err = "checkpoint: the colourer belongs to another context"; return IMMESH_E_INVAL; }
    if (c->cfg.shard_world > 1) { c->err = "checkpoint: sharded contexts (shard_world > 1) are not saved"; return IMMESH_E_INVAL; }
    (void)hipSetDevice(c->cfg.device);
    const auto t_wall = clk::now();
    // ---- drain: queued mesh jobs, then a pending or deferred map-update tail (immesh_counters settles it)
    int rc;
    if ((rc = immesh_mesh_wait(c))) return rc;
    immesh_counters_t tmp;
    if ((rc = immesh_counters(c, &tmp, 0))) return rc;
    MeshHost& h = c->mesh_host;
    RegionsHost* R = h.regions;
    std::unique_lock<std::mutex> lr;
    if (R) lr = std::unique_lock<std::mutex>(R->mu);
    std::lock_guard<std::mutex> lq(h.launch_mu);
    if ((rc = ck_quiesce(c))) return rc;
    hipStream_t s = h.stream_q;
    CkScratch scr;
    const std::string tmp_path = std::string(path) + ".tmp";
    scr.fd = open(tmp_path.c_str(), O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0644);
    if (scr.fd < 0) { c->err = "checkpoint: cannot create " + tmp_path + ": " + std::strerror(errno); return IMMESH_E_IO; }
    auto fail = [&](int code) { if (scr.fd >= 0) { close(scr.fd); scr.fd = -1; } (void)unlink(tmp_path.c_str()); return code; };

    // ---- header: counts from the device counters
    const auto t_dev = clk::now();
    int32_t rcnt[16], pc[PC_COUNT], rg[RG_COUNTERS] = {};
    const bool regions_on = R && R->on && R->d.ent;
    hipError_t he = hipMemcpyAsync(rcnt, c->map.counters, sizeof(rcnt), hipMemcpyDeviceToHost, s);
    if (he == hipSuccess) he = hipMemcpyAsync(pc, c->mesh.pc, sizeof(pc), hipMemcpyDeviceToHost, s);
    if (he == hipSuccess && regions_on) he = hipMemcpyAsync(rg, R->d.cnt, sizeof(rg), hipMemcpyDeviceToHost, s);
    if (he == hipSuccess) he = hipStreamSynchronize(s);
    if (he != hipSuccess) { c->err = std::string("checkpoint: reading the counters: ") + hipGetErrorString(he); return fail(IMMESH_E_HIP); }
    CkFileHeader hd;
    std::memset(&hd, 0, sizeof(hd));
    std::memcpy(hd.magic, "IMMESHCK", 8);
    hd.version = IMMESH_CHECKPOINT_VERSION; hd.header_bytes = (int32_t)sizeof(hd); hd.section_bytes = (int32_t)sizeof(immesh_checkpoint_section);
    hd.has_regions = regions_on ? 1 : 0; hd.has_colour = col ? 1 : 0;
    ck_rec_values(hd.rec);
    hd.masks[0] = c->map.hmask; hd.masks[1] = c->mesh.g_mask; hd.masks[2] = c->mesh.x_mask; hd.masks[3] = c->mesh.th_mask;
    hd.cfg = c->cfg;
    auto clampc = [](int64_t v, int64_t cap) { return std::max<int64_t>(0, std::min(v, cap)); };
    int64_t* n = hd.counts;
    n[CKC_ROOTS] = rcnt[6]; n[CKC_NODES] = clampc(rcnt[0], c->map.cap_nodes); n[CKC_CHUNKS] = clampc(rcnt[1], c->map.cap_chunks);
    n[CKC_FREE_READY] = clampc(rcnt[2], c->map.cap_chunks); n[CKC_FREE_PENDING] = clampc(rcnt[3], c->map.cap_chunks);
    n[CKC_EXT] = clampc(rcnt[4], c->map.cap_ext); n[CKC_LEAF] = clampc(rcnt[8], c->map.cap_leaf_chunks);
    n[CKC_VERTS] = clampc(pc[PC_VERTS], c->mesh.cap_verts); n[CKC_VOXELS] = clampc(pc[PC_VOXELS], c->mesh.cap_voxels); n[CKC_TRIS] = clampc(pc[PC_TRIS], c->mesh.cap_tris);
    n[CKC_LIVE] = h.n_live; n[CKC_ADJ] = clampc(pc[PC_ADJ_CHUNKS], c->mesh.cap_adj_chunks); n[CKC_REGIONS] = regions_on ? clampc(rg[RG_N], RG_CAP_REGIONS) : 0;
    n[CKC_SCANS_MESHED] = h.seq; n[CKC_MAP_UPDATES] = c->map.upd_seq;
    CkHostState hs;
    std::memset(&hs, 0, sizeof(hs));
    hs.cnt = c->cnt; std::memcpy(hs.cum, h.cum, sizeof(hs.cum)); hs.n_live = h.n_live; hs.seq = h.seq; hs.n_vertices = h.n_vertices; hs.upd_seq = c->map.upd_seq;
    { std::lock_guard<std::mutex> lk(h.mu); hs.jobs = h.submitted; }
    n[CKC_MESH_JOBS] = hs.jobs;
    if (col && cl_colourer_state(col).cap < n[CKC_VERTS]) { c->err = "checkpoint: the colourer holds fewer vertices than the map"; return fail(IMMESH_E_INVAL); }

    // ---- the tables: count -> exclusive scan -> pack, in ascending slot order
    CkTableRef tabs[CK_N_TABLES];
    ck_tables(c, tabs);
    int64_t tab[CK_N_TABLES] = {0, 0, 0, 0, 0};
    int32_t* d_counts[CK_N_TABLES] = {};
    int32_t totals[CK_N_TABLES] = {};
    uint32_t* d_slots[CK_N_TABLES] = {};
    void* d_ents[CK_N_TABLES] = {};
    const int n_tables = regions_on ? CK_N_TABLES : CK_N_TABLES - 1;
    {
        size_t scan_bytes = 0;
        for (int t = 0; t < n_tables; t++) scan_bytes = std::max(scan_bytes, exclusive_sum_temp_bytes(ck_table_blocks(tabs[t].n_slots) + 1));
        void* d_scan = nullptr;
        if ((rc = scr.alloc(c, &d_scan, scan_bytes + 256))) return fail(rc);
        for (int t = 0; t < n_tables; t++) {
            const int nb = ck_table_blocks(tabs[t].n_slots);
            if ((rc = scr.alloc(c, (void**)&d_counts[t], (size_t)(nb + 1) * 4))) return fail(rc);
            (void)hipMemsetAsync(d_counts[t] + nb, 0, 4, s);
            ck_launch_count(s, t, tabs[t].ents, tabs[t].n_slots, d_counts[t]);
            exclusive_sum_i32(s, d_scan, scan_bytes + 256, d_counts[t], d_counts[t], nb + 1);
            (void)hipMemcpyAsync(&totals[t], d_counts[t] + nb, 4, hipMemcpyDeviceToHost, s);
        }
        if ((he = hipStreamSynchronize(s)) != hipSuccess || (he = hipGetLastError()) != hipSuccess) { c->err = std::string("checkpoint: counting the tables: ") + hipGetErrorString(he); return fail(IMMESH_E_HIP); }
        for (int t = 0; t < n_tables; t++) {
            tab[t] = totals[t];
            if ((rc = scr.alloc(c, (void**)&d_slots[t], (size_t)tab[t] * 4)) || (rc = scr.alloc(c, &d_ents[t], (size_t)tab[t] * ck_table_entry_bytes(t)))) return fail(rc);
            if (tab[t] > 0) ck_launch_pack(s, t, tabs[t].ents, tabs[t].n_slots, d_counts[t], d_slots[t], d_ents[t]);
        }
    }
    // ---- placement, checksums
    std::vector<CkSpec> specs = ck_sections(hd, tab, c, col, &hs);
    hd.n_sections = (int32_t)specs.size();
    hd.payload_offset = align_up((int64_t)sizeof(hd) + (int64_t)specs.size() * (int64_t)sizeof(immesh_checkpoint_section), CK_ALIGN);
    std::vector<CkPlaced> placed;
    int64_t total = 0;
    for (CkSpec& p : specs) {
        if (p.table >= 0) p.ptr = p.part == 0 ? (char*)d_slots[p.table] : (char*)d_ents[p.table];
        placed.push_back({p, total});
        total = align_up(total + p.bytes(), CK_ALIGN);
    }
    hd.file_bytes = hd.payload_offset + total;
    std::vector<uint64_t> sums;
    if ((rc = ck_checksums(c, s, placed, scr, sums))) return fail(rc);
    const double ms_dev = ms_since(t_dev);
    std::vector<immesh_checkpoint_section> table(placed.size());
    for (size_t i = 0; i < placed.size(); i++) {
        std::memset(&table[i], 0, sizeof(table[i]));
        std::memcpy(table[i].name, placed[i].spec.name, sizeof(table[i].name));
        table[i].offset = hd.payload_offset + placed[i].offset; table[i].bytes = placed[i].spec.bytes(); table[i].records = placed[i].spec.records; table[i].checksum = sums[i];
    }
    hd.header_checksum = 0;
    hd.header_checksum = ck_checksum_host(&hd, sizeof(hd)) + ck_checksum_host(table.data(), table.size() * sizeof(table[0]), sizeof(hd) / 8);

    // ---- the payload through the staging buffers, then header and table, flush, rename
    double ms_copy = 0, ms_file = 0;
    if ((rc = scr.staging(c))) return fail(rc);
    if ((rc = ck_stream(c, s, true, scr.fd, hd.payload_offset, total, placed, scr, &ms_copy, &ms_file))) return fail(rc);
    {
        const auto t0 = clk::now();
        std::vector<char> head((size_t)hd.payload_offset, 0);
        std::memcpy(head.data(), &hd, sizeof(hd));
        std::memcpy(head.data() + sizeof(hd), table.data(), table.size() * sizeof(table[0]));
        bool ok = write_all(scr.fd, head.data(), head.size(), 0) && fsync(scr.fd) == 0;
        const int cfd = scr.fd;
        scr.fd = -1;
        ok = (close(cfd) == 0) && ok;
        if (!ok) { c->err = "checkpoint: write / fsync of " + tmp_path + " failed: " + std::strerror(errno); return fail(IMMESH_E_IO); }
        if (rename(tmp_path.c_str(), path) != 0) { c->err = std::string("checkpoint: rename to ") + path + " failed: " + std::strerror(errno); return fail(IMMESH_E_IO); }
        ms_file += ms_since(t0);
    }
    ck_fill_info(hd, info);
    if (info) { info->ms[0] = (float)ms_dev; info->ms[1] = (float)ms_copy; info->ms[2] = (float)ms_file; info->ms[3] = (float)ms_since(t_wall); }
    return 0;
}

int immesh_checkpoint_load(immesh_ctx* c, immesh_colourer* col, const char* path, immesh_checkpoint_info* info) {
    if (!c) return IMMESH_E_INVAL;
    if (!path || !*path) { c->err = "checkpoint: path is empty"; return IMMESH_E_INVAL; }
    if (col && cl_colourer_ctx(col) != c) { c->err = "checkpoint: the colourer belongs to another context"; return IMMESH_E_INVAL; }
    if (c->cfg.shard_world > 1) { c->err = "checkpoint: sharded contexts (shard_world > 1) are not loaded into"; return IMMESH_E_INVAL; }
    (void)hipSetDevice(c->cfg.device);
    const auto t_wall = clk::now();
    CkScratch scr;
    scr.fd = open(path, O_RDONLY | O_CLOEXEC);
    if (scr.fd < 0) { c->err = std::string("checkpoint: cannot open ") + path + ": " + std::strerror(errno); return IMMESH_E_IO; }
    CkFileHeader hd;
    std::vector<immesh_checkpoint_section> table;
    int rc;
    { std::string e; if ((rc = ck_probe_fd(scr.fd, hd, table, e))) { c->err = "checkpoint: " + e; return rc; } }
    MeshHost& h = c->mesh_host;
    RegionsHost* R = h.regions;
    const int64_t* n = hd.counts;
    // ---- the context: fresh, same algorithm parameters, same table sizes, pools large enough
    {
        bool used = c->pending || c->tail_deferred || c->map.upd_seq != 0 || h.seq != 0;
        { std::lock_guard<std::mutex> lk(h.mu); used = used || h.submitted != 0; }
        int32_t rcnt[16], pc[PC_COUNT];
        CKHIP(c, hipMemcpyAsync(rcnt, c->map.counters, sizeof(rcnt), hipMemcpyDeviceToHost, h.stream_q));
        CKHIP(c, hipMemcpyAsync(pc, c->mesh.pc, sizeof(pc), hipMemcpyDeviceToHost, h.stream_q));
        CKHIP(c, hipStreamSynchronize(c->stream));
        CKHIP(c, hipStreamSynchronize(h.stream_q));
        used = used || rcnt[0] != 0 || rcnt[6] != 0 || pc[PC_VERTS] != 0 || pc[PC_VOXELS] != 0 || pc[PC_TRIS] != 0;
        if (used) { c->err = "checkpoint: load needs a context on which no map build, update, scan or mesh job has run since immesh_create"; return IMMESH_E_INVAL; }
    }
    {
        const immesh_config &a = hd.cfg, &b = c->cfg;
        const char* f = nullptr;
        if (a.voxel_size != b.voxel_size) f = "voxel_size";
        else if (a.max_layer != b.max_layer) f = "max_layer";
        else if (std::memcmp(a.layer_init, b.layer_init, sizeof(a.layer_init)) != 0) f = "layer_init";
        else if (a.max_points_size != b.max_points_size) f = "max_points_size";
        else if (a.planer_threshold != b.planer_threshold) f = "planer_threshold";
        else if (a.dept_err != b.dept_err) f = "dept_err";
        else if (a.beam_err != b.beam_err) f = "beam_err";
        else if (a.calib_laser != b.calib_laser) f = "calib_laser";
        else if (a.mesh_min_spacing != b.mesh_min_spacing) f = "mesh_min_spacing";
        else if (a.mesh_voxel != b.mesh_voxel) f = "mesh_voxel";
        else if (a.mesh_region != b.mesh_region) f = "mesh_region";
        else if (a.mesh_append_budget != b.mesh_append_budget) f = "mesh_append_budget";
        if (f) { c->err = std::string("checkpoint: ") + f + " of the file differs from the context's (algorithm parameters must be equal)"; return IMMESH_E_INVAL; }
        const uint64_t mine[4] = {c->map.hmask, c->mesh.g_mask, c->mesh.x_mask, c->mesh.th_mask};
        static const char* which[4] = {"registration hash (hmask, from cap_root_voxels)", "dedupe grid (g_mask, from cap_vertices)", "mesh-voxel hash (x_mask, from cap_vertices)",
                                       "triangle hash (th_mask, from cap_triangles)"};
        for (int k = 0; k < 4; k++)
            if (hd.masks[k] != mine[k]) {
                c->err = std::string("checkpoint: size of the ") + which[k] + ": file " + std::to_string(hd.masks[k] + 1) + " slots, context " + std::to_string(mine[k] + 1) + " (table sizes must be equal)";
                return IMMESH_E_INVAL;
            }
        struct Cap { const char* name; int64_t used, cap; };
        const Cap caps[] = {{"cap_nodes", n[CKC_NODES], c->map.cap_nodes}, {"cap_point_chunks", n[CKC_CHUNKS], c->map.cap_chunks}, {"cap_point_chunks (free list)", n[CKC_FREE_READY] + n[CKC_FREE_PENDING], c->map.cap_chunks},
                            {"extension tables (cap_ext, from cap_nodes)", n[CKC_EXT], c->map.cap_ext}, {"leaf chunks (cap_leaf_chunks, from cap_nodes)", n[CKC_LEAF], c->map.cap_leaf_chunks},
                            {"cap_vertices", n[CKC_VERTS], c->mesh.cap_verts}, {"mesh voxels (cap_vertices)", n[CKC_VOXELS], c->mesh.cap_voxels}, {"cap_triangles", n[CKC_TRIS], c->mesh.cap_tris},
                            {"adjacency chunks (cap_adj_chunks, from cap_vertices and cap_triangles)", n[CKC_ADJ], c->mesh.cap_adj_chunks}, {"regions", n[CKC_REGIONS], RG_CAP_REGIONS}};
        for (const Cap& q : caps)
            if (q.used > q.cap) { c->err = std::string("checkpoint: ") + q.name + ": the file uses " + std::to_string(q.used) + ", the context holds " + std::to_string(q.cap); return IMMESH_E_CAPACITY; }
        if (R && R->on && !hd.has_regions) { c->err = "checkpoint: the context's region table is on and the file has no region section"; return IMMESH_E_INVAL; }
        if (hd.has_colour && col && cl_colourer_state(col).cap < n[CKC_VERTS]) { c->err = "checkpoint: the colourer holds fewer vertices than the file"; return IMMESH_E_INVAL; }
    }
    // ---- from here on the context changes
    if (hd.has_regions && (rc = immesh_mesh_regions_enable(c, 1))) { c->err = std::string("checkpoint: region table: ") + immesh_mesh_regions_error(c); return rc; }
    std::unique_lock<std::mutex> lr;
    if (R) lr = std::unique_lock<std::mutex>(R->mu);
    std::lock_guard<std::mutex> lq(h.launch_mu);
    if ((rc = ck_quiesce(c))) return rc;
    hipStream_t s = h.stream_q;
    int64_t tab[CK_N_TABLES] = {0, 0, 0, 0, 0};
    CkHostState hs;
    std::memset(&hs, 0, sizeof(hs));
    {
        std::vector<CkSpec> probe = ck_sections(hd, tab, nullptr, nullptr, nullptr);   // (names only: which entries are the tables' slot lists)
        for (size_t i = 0; i < probe.size(); i++) if (probe[i].table >= 0 && probe[i].part == 0) tab[probe[i].table] = table[i].records;
    }
    const bool with_colour = hd.has_colour && col != nullptr;
    std::vector<CkSpec> specs = ck_sections(hd, tab, c, with_colour ? col : nullptr, &hs);
    CkTableRef tabs[CK_N_TABLES];
    ck_tables(c, tabs);
    uint32_t* d_slots[CK_N_TABLES] = {};
    void* d_ents[CK_N_TABLES] = {};
    const int n_tables = hd.has_regions ? CK_N_TABLES : CK_N_TABLES - 1;
    for (int t = 0; t < n_tables; t++)
        if ((rc = scr.alloc(c, (void**)&d_slots[t], (size_t)tab[t] * 4)) || (rc = scr.alloc(c, &d_ents[t], (size_t)tab[t] * ck_table_entry_bytes(t)))) return rc;
    std::vector<CkPlaced> placed;
    for (size_t i = 0; i < specs.size(); i++) {
        CkSpec& p = specs[i];
        if (p.table >= 0) p.ptr = p.part == 0 ? (char*)d_slots[p.table] : (char*)d_ents[p.table];
        placed.push_back({p, table[i].offset - hd.payload_offset});
    }
    double ms_copy = 0, ms_file = 0;
    if ((rc = scr.staging(c))) return rc;
    if ((rc = ck_stream(c, s, false, scr.fd, hd.payload_offset, hd.file_bytes - hd.payload_offset, placed, scr, &ms_copy, &ms_file))) return rc;
    // ---- checksums of what was placed, then the tables' records into their slots
    const auto t_dev = clk::now();
    std::vector<uint64_t> sums;
    if ((rc = ck_checksums(c, s, placed, scr, sums))) return rc;
    for (size_t i = 0; i < placed.size(); i++)
        if (placed[i].spec.ptr && sums[i] != table[i].checksum) {
            c->err = std::string("checkpoint: checksum mismatch in section ") + placed[i].spec.name + " (the context's maps are undefined now: destroy it)";
            return IMMESH_E_FORMAT;
        }
    int32_t* d_bad = nullptr;
    if ((rc = scr.alloc(c, (void**)&d_bad, 4))) return rc;
    CKHIP(c, hipMemsetAsync(d_bad, 0, 4, s));
    for (int t = 0; t < n_tables; t++) ck_launch_unpack(s, t, tabs[t].ents, tabs[t].n_slots, d_slots[t], d_ents[t], tab[t], d_bad);
    int32_t bad = 0;
    CKHIP(c, hipMemcpyAsync(&bad, d_bad, 4, hipMemcpyDeviceToHost, s));
    CKHIP(c, hipMemcpyAsync(c->h_counters, c->map.counters, 16 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    CKHIP(c, hipStreamSynchronize(s));
    CKHIP(c, hipGetLastError());
    if (bad) { c->err = "checkpoint: " + std::to_string(bad) + " slot indices outside their table (the context's maps are undefined now: destroy it)"; return IMMESH_E_FORMAT; }
    const double ms_dev = ms_since(t_dev);
    // ---- the host's share
    c->cnt = hs.cnt; c->last_n_ds = 0; c->last_reg_pts = nullptr;
    c->map.upd_seq = hs.upd_seq;
    std::memcpy(h.cum, hs.cum, sizeof(h.cum));
    h.seq = hs.seq; h.n_vertices = hs.n_vertices; h.n_live = hs.n_live;
    {
        std::lock_guard<std::mutex> lk(h.mu);   // the mesh job ordinal goes on where the saver's stopped: job sets, world buffers and result sets follow it
        h.submitted = h.completed = h.collected = (long)hs.jobs;
        h.current = 0;
    }
    ck_fill_info(hd, info);
    if (info) { info->has_colour = with_colour ? 1 : 0; info->ms[0] = (float)ms_dev; info->ms[1] = (float)ms_copy; info->ms[2] = (float)ms_file; info->ms[3] = (float)ms_since(t_wall); }
    return 0;
}

}  // extern "C"
