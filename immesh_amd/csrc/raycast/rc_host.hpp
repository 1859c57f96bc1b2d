// The host scaffold of the device modules that own a stream (the caster and its passes, the cloud index and its rules, the renderer, the colourer):
// a buffer that frees itself, the checks more than one entry point makes, the end of a timed span, the point-thinning tail of the two reinforce passes.
// Every refusal is written to the context with the caller's name in front.  Defined in raycast_host.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <utility>
#include "../../../include/immesh_c_api.h"

// ---- a record releases what it holds when it is destroyed, so a buffer is freed by being a member ----------------------------------------------------
struct RcBuf {   // grow-only device buffer
    void* p = nullptr;
    size_t bytes = 0;
    RcBuf() = default;
    RcBuf(const RcBuf&) = delete;
    RcBuf& operator=(const RcBuf&) = delete;
    ~RcBuf() { if (p) (void)hipFree(p); }
};
inline void rc_swap(RcBuf& a, RcBuf& b) {   // two buffers change places (an apply: a result becomes the snapshot)
    std::swap(a.p, b.p);
    std::swap(a.bytes, b.bytes);
}
inline void rc_destroy_events(hipEvent_t* e, int n) {
    for (int i = 0; i < n; i++)
        if (e[i]) (void)hipEventDestroy(e[i]);
}
inline int rc_index_bits(int64_t n) {   // the bits the values 0 .. n - 1 need: the significant bits of a sort over them
    int bits = 1;
    while (bits < 32 && ((int64_t)1 << bits) < n) bits++;
    return bits;
}
// grows b to at least `bytes` (contents are not kept); IMMESH_E_NOMEM with "<who>: hipMalloc(... B) failed" in the context
int rc_grow(immesh_ctx* c, const char* who, RcBuf& b, size_t bytes);
// dst = `bytes` of device memory, unless dst is NULL or nothing is asked for
int rc_fetch(immesh_ctx* c, void* dst, const void* src, size_t bytes);
// the room of a fetch.  rc_cap_negative: "<who>: cap is negative".  rc_cap: that check, then *n_out = n (when given) and, when an output is wanted,
// "<who>: cap <cap> < <n> <noun>" (IMMESH_E_CAPACITY)
int rc_cap_negative(immesh_ctx* c, const char* who, int64_t cap);
int rc_cap(immesh_ctx* c, const char* who, int64_t cap, int64_t n, int64_t* n_out, bool wanted, const char* noun);
// the argument checks more than one entry point makes: "<who>: <none>" unless `have`; "<who>: need 0 < <what>, finite"; "<who>: bad point array" (n
// outside [0, RC_MAX_COUNT], or points without an array); "<who>: need <what> in [0, 2^31 - 2]"; "<who>: <noun> rotation / position is not finite"
// (the twelve values of a pose); a host soup: "<who>: bad vertex / face arrays" (a negative count, more than max_faces faces, a count without its
// array), "<who>: face <i> has vertex index <v> out of range [0, <n_vtx>)"
constexpr int64_t RC_MAX_COUNT = (int64_t)0x7FFFFFFE;
int rc_have(immesh_ctx* c, const char* who, bool have, const char* none);
int rc_positive(immesh_ctx* c, const char* who, const char* what, double v);
int rc_points(immesh_ctx* c, const char* who, const float* pts, int64_t n);
int rc_count_arg(immesh_ctx* c, const char* who, const char* what, int64_t v);
int rc_finite_pose(immesh_ctx* c, const char* who, const char* noun, const double rot[9], const double pos[3]);
int rc_check_soup(immesh_ctx* c, const char* who, int64_t max_faces, const float* vtx, int64_t n_vtx, const int32_t* faces, int64_t n_faces);
// a checked soup into d_vtx / d_faces (grown under `who`), queued on s
int rc_upload_soup(immesh_ctx* c, const char* who, hipStream_t s, RcBuf& d_vtx, RcBuf& d_faces, const float* vtx, int64_t n_vtx, const int32_t* faces,
                   int64_t n_faces);
// The end of a span on s: ev1 recorded, `bytes` of device memory copied to the pinned dst behind it (nothing when bytes == 0), the launches' error
// checked, s idle, *ms = ev0 .. ev1.
int rc_span_end(immesh_ctx* c, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1, float* ms, void* dst = nullptr, const void* src = nullptr, size_t bytes = 0);

// ---- the thinning tail of a reinforce pass (the renderer's pixels, the caster's rays): of n candidates, those with depth[i] >= 0 are points; with
// res > 0 the first point of every cell of that size stays (a hash table of at least 1024 and at least 2 n slots), otherwise all of them
struct RcThin {
    RcBuf pts, cells, keep, koff, slot, tab, out, small;   // candidates: points, cells, keep flags, their scan, table slots; the table; the result, its count
};
// the buffers of n candidates (cells, slot and the table only when res > 0) and the scan's scratch in `temp`; *mask = slots - 1, or 0 without a table
int rc_thin_grow(immesh_ctx* c, const char* who, RcThin& th, RcBuf& temp, int64_t n, float res, uint32_t* mask);
// Behind the owner's producer, which wrote pts, cells and keep: the table's preset and the two hash launches (res > 0), the scan of keep, the
// compaction into out; the count is left in small[0] (the owner ends the span with rc_span_end and reads it back)
int rc_thin_run(immesh_ctx* c, hipStream_t s, RcThin& th, RcBuf& temp, int64_t n, float res, uint32_t mask, const float* depth);
// *n_out = n_points (when given); 0 without an output array or without points; "<who>: cap <cap> < <n> points" (IMMESH_E_CAPACITY); else the copy
int rc_thin_fetch(immesh_ctx* c, const char* who, const RcThin& th, int64_t n_points, float* xyz_out, int64_t cap, int64_t* n_out);
