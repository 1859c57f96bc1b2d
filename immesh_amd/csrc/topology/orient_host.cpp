// Host side of the orientation (include/immesh_topology.h, the Orientation rule): argument checks, grow-only buffers in the caster's RcOrient record,
// the orientation, its fetches and the apply on the caster's stream.  Nothing here is allocated or launched before the first immesh_topology_orient.
// It reads what the analysis left on the device: the marks of the counting faces and the sorted half-edges.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <string>
#include "../host_ctx.hpp"
#include "../../../include/immesh_topology.h"
#include "topology.hpp"

static_assert(sizeof(immesh_orient_stats) == 9 * 8 && offsetof(immesh_orient_stats, n_patches) == 0 && offsetof(immesh_orient_stats, n_orientable) == 8 &&
                  offsetof(immesh_orient_stats, n_nonorientable) == 16 && offsetof(immesh_orient_stats, largest_patch_faces) == 24 &&
                  offsetof(immesh_orient_stats, n_faces_flipped) == 32 && offsetof(immesh_orient_stats, n_faces_nonorientable) == 40 &&
                  offsetof(immesh_orient_stats, n_patches_inverted) == 48 && offsetof(immesh_orient_stats, n_inconsistent_before) == 56 &&
                  offsetof(immesh_orient_stats, n_inconsistent_after) == 64,
              "immesh_orient_stats layout (immesh_amd/capi.py mirrors it)");

namespace {

enum { OS_PATCHES = 0, OS_ORIENTABLE, OS_NONORIENTABLE, OS_LARGEST, OS_FLIPPED, OS_FACES_NONORIENTABLE, OS_INVERTED, OS_BEFORE, OS_AFTER };
constexpr size_t TP_ST_INCONSISTENT = offsetof(immesh_topology_stats, n_inconsistent) / 8;   // its place in RcTopology::st

int ot_grow(immesh_raycaster* r, RcBuf& b, size_t bytes) { return rc_grow(r->ctx, "topology_orient", b, bytes); }

int ot_events(immesh_raycaster* r) {
    immesh_ctx* c = r->ctx;
    for (hipEvent_t& e : r->ot.ev)
        if (!e) HIPCHK(c, hipEventCreate(&e));
    if (!r->ot.h_cnt) HIPCHK(c, hipHostMalloc((void**)&r->ot.h_cnt, OT_COUNTERS * 8));
    return 0;
}

int ot_analysed(immesh_raycaster* r, const char* who) {
    if (!r->built) { r->ctx->err = std::string(who) + ": no hierarchy has been built (immesh_raycast_build_triangles / _build_mesh)"; return IMMESH_E_INVAL; }
    if (!r->tp.have) { r->ctx->err = std::string(who) + ": no analysis since the caster's last build (immesh_topology_analyse)"; return IMMESH_E_INVAL; }
    return 0;
}

int ot_oriented(immesh_raycaster* r, const char* who) {
    const int rc = ot_analysed(r, who);
    if (rc) return rc;
    if (!r->ot.have) { r->ctx->err = std::string(who) + ": no orientation since the last analysis (immesh_topology_orient)"; return IMMESH_E_INVAL; }
    return 0;
}

}  // namespace

extern "C" {

int immesh_topology_orient(immesh_raycaster* r, int32_t mode, const double* viewpoint, immesh_orient_stats* stats) {
    if (!r) return IMMESH_E_INVAL;
    immesh_ctx* c = r->ctx;
    int rc;
    if ((rc = ot_analysed(r, "topology_orient"))) return rc;
    if (mode != IMMESH_ORIENT_FIRST && mode != IMMESH_ORIENT_FEWEST && mode != IMMESH_ORIENT_VIEWPOINT) {
        c->err = "topology_orient: unknown mode " + std::to_string(mode);
        return IMMESH_E_INVAL;
    }
    if (mode == IMMESH_ORIENT_VIEWPOINT) {
        if (!viewpoint) { c->err = "topology_orient: IMMESH_ORIENT_VIEWPOINT needs a viewpoint"; return IMMESH_E_INVAL; }
        for (int k = 0; k < 3; k++)
            if (!(std::fabs(viewpoint[k]) < 0x1p128)) {   // (false for NaN)
                c->err = "topology_orient: the viewpoint is not finite, or 2^128 and more in magnitude";
                return IMMESH_E_INVAL;
            }
    }
    (void)hipSetDevice(c->cfg.device);
    hipStream_t s = r->s;
    const RcTopology& q = r->tp;
    RcOrient& o = r->ot;
    const int64_t nf = r->n_faces, n_bound = q.n_counting, n_half = q.n_half;
    o.have = false;
    if ((rc = ot_events(r))) return rc;
    if ((rc = ot_grow(r, o.cnt, OT_COUNTERS * 8))) return rc;
    if ((rc = ot_grow(r, o.cover, (size_t)nf * 8))) return rc;
    if ((rc = ot_grow(r, o.label, (size_t)nf * 4))) return rc;
    if ((rc = ot_grow(r, o.base, (size_t)nf))) return rc;
    if ((rc = ot_grow(r, o.root, (size_t)nf * 4))) return rc;
    if ((rc = ot_grow(r, o.num, (size_t)nf * 4))) return rc;
    if ((rc = ot_grow(r, o.patch, (size_t)nf * 4))) return rc;
    if ((rc = ot_grow(r, o.flip, (size_t)nf))) return rc;
    if ((rc = ot_grow(r, o.out, (size_t)nf * 12))) return rc;
    if ((rc = ot_grow(r, o.tab, (size_t)n_bound * OT_TABLES * 4))) return rc;
    if ((rc = ot_grow(r, r->tree.temp, exclusive_sum_temp_bytes((int)std::max<int64_t>(nf, 1)) + 256))) return rc;   // the caster's scan scratch
    const int32_t* faces = (const int32_t*)r->faces.p;
    unsigned long long* cnt = (unsigned long long*)o.cnt.p;
    int32_t *cover = (int32_t*)o.cover.p, *label = (int32_t*)o.label.p, *root = (int32_t*)o.root.p, *num = (int32_t*)o.num.p, *patch = (int32_t*)o.patch.p;
    int32_t* tab = (int32_t*)o.tab.p;
    int8_t* base = (int8_t*)o.base.p;
    HIPCHK(c, hipEventRecord(o.ev[0], s));
    HIPCHK(c, hipMemsetAsync(cnt, 0, OT_COUNTERS * 8, s));
    if (nf > 0) {
        if (n_bound > 0) HIPCHK(c, hipMemsetAsync(tab, 0, (size_t)n_bound * OT_TABLES * 4, s));
        ot_launch_init(s, 2 * nf, cover);
        ot_launch_link(s, (const unsigned long long*)q.key_b.p, (const int32_t*)q.val_b.p, n_half, faces, cover, cnt);
        ot_launch_flatten(s, cover, (const int32_t*)q.flag.p, nf, label, base, root);
        exclusive_sum_i32(s, r->tree.temp.p, r->tree.temp.bytes, root, num, (int)nf);
        ot_launch_patches(s, (const float*)r->vtx.p, faces, nf, label, base, root, num, mode, mode == IMMESH_ORIENT_VIEWPOINT ? viewpoint : nullptr, patch,
                          tab, n_bound, cnt);
        ot_launch_inconsistent(s, (const unsigned long long*)q.key_b.p, (const int32_t*)q.val_b.p, n_half, faces, patch, tab, n_bound);
        ot_launch_decide(s, n_bound, mode, tab, cnt);
        ot_launch_flip(s, faces, nf, patch, base, tab, n_bound, (int8_t*)o.flip.p, (int32_t*)o.out.p);
    }
    HIPCHK(c, hipEventRecord(o.ev[1], s));
    unsigned long long* h = o.h_cnt;
    HIPCHK(c, hipMemcpyAsync(h, cnt, OT_COUNTERS * 8, hipMemcpyDeviceToHost, s));   // the one read-back
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(s));
    (void)hipEventElapsedTime(&o.ms[0], o.ev[0], o.ev[1]);
    if (h[OT_ERROR]) {
        c->err = "topology_orient: a union did not finish within its step bound (a defect of the library)";
        return IMMESH_E_INTERNAL;
    }
    int64_t* st = o.st;
    st[OS_PATCHES] = (int64_t)h[OT_N_PATCHES]; st[OS_ORIENTABLE] = (int64_t)h[OT_N_ORIENTABLE]; st[OS_NONORIENTABLE] = (int64_t)h[OT_N_NONORIENTABLE];
    st[OS_LARGEST] = (int64_t)h[OT_LARGEST_PATCH]; st[OS_FLIPPED] = (int64_t)h[OT_N_FLIPPED];
    st[OS_FACES_NONORIENTABLE] = (int64_t)h[OT_N_FACES_NONORIENTABLE]; st[OS_INVERTED] = (int64_t)h[OT_N_INVERTED];
    st[OS_BEFORE] = q.st[TP_ST_INCONSISTENT]; st[OS_AFTER] = (int64_t)h[OT_INCONSISTENT_AFTER];
    o.n_bound = n_bound;
    o.have = true;
    if (stats) std::memcpy(stats, st, sizeof(*stats));
    return 0;
}

int immesh_topology_orient_faces(immesh_raycaster* r, int32_t* patch_out, int8_t* flip_out, int32_t* faces_out) {
    if (!r) return IMMESH_E_INVAL;
    immesh_ctx* c = r->ctx;
    int rc;
    if ((rc = ot_oriented(r, "topology_orient_faces"))) return rc;
    const int64_t nf = r->n_faces;
    if (nf == 0) return 0;
    (void)hipSetDevice(c->cfg.device);
    if (patch_out) HIPCHK(c, hipMemcpy(patch_out, r->ot.patch.p, (size_t)nf * 4, hipMemcpyDeviceToHost));
    if (flip_out) HIPCHK(c, hipMemcpy(flip_out, r->ot.flip.p, (size_t)nf, hipMemcpyDeviceToHost));
    if (faces_out) HIPCHK(c, hipMemcpy(faces_out, r->ot.out.p, (size_t)nf * 12, hipMemcpyDeviceToHost));
    return 0;
}

int immesh_topology_orient_patches(immesh_raycaster* r, int32_t* first_face, int32_t* n_faces, int32_t* orientable, int32_t* n_flipped,
                                   int32_t* n_inconsistent, int64_t cap, int64_t* n_out) {
    if (!r) return IMMESH_E_INVAL;
    immesh_ctx* c = r->ctx;
    int rc;
    if ((rc = ot_oriented(r, "topology_orient_patches"))) return rc;
    if (cap < 0) { c->err = "topology_orient_patches: cap is negative"; return IMMESH_E_INVAL; }
    const RcOrient& o = r->ot;
    const int64_t n = o.st[OS_PATCHES];
    if (n_out) *n_out = n;
    if ((!first_face && !n_faces && !orientable && !n_flipped && !n_inconsistent) || n == 0) return 0;
    if (cap < n) {
        c->err = "topology_orient_patches: cap " + std::to_string(cap) + " < " + std::to_string(n) + " patches";
        return IMMESH_E_CAPACITY;
    }
    (void)hipSetDevice(c->cfg.device);
    const int32_t* tab = (const int32_t*)o.tab.p;
    int32_t* const out[5] = {first_face, n_faces, orientable, n_flipped, n_inconsistent};
    const int which[5] = {OT_FIRST, OT_NFACES, OT_ORIENTABLE, OT_NFLIPPED, OT_NINCONSISTENT};
    for (int k = 0; k < 5; k++)
        if (out[k]) HIPCHK(c, hipMemcpy(out[k], tab + which[k] * o.n_bound, (size_t)n * 4, hipMemcpyDeviceToHost));
    return 0;
}

int immesh_topology_orient_apply(immesh_raycaster* r) {
    if (!r) return IMMESH_E_INVAL;
    immesh_ctx* c = r->ctx;
    int rc;
    if ((rc = ot_oriented(r, "topology_orient_apply"))) return rc;
    (void)hipSetDevice(c->cfg.device);
    hipStream_t s = r->s;
    RcOrient& o = r->ot;
    HIPCHK(c, hipEventRecord(o.ev[2], s));
    if (r->n_faces > 0) HIPCHK(c, hipMemcpyAsync(r->faces.p, o.out.p, (size_t)r->n_faces * 12, hipMemcpyDeviceToDevice, s));
    HIPCHK(c, hipEventRecord(o.ev[3], s));
    HIPCHK(c, hipStreamSynchronize(s));
    (void)hipEventElapsedTime(&o.ms[1], o.ev[2], o.ev[3]);
    // what a successful build discards.  Nothing else the caster keeps depends on the order of a face's vertices: the hierarchy holds boxes and
    // face indices, and the closest-point results of the last query stay readable after a build too.
    r->have_cast = false; r->n_points = 0;
    r->sm.have = false;
    r->tp.have = false;
    o.have = false;
    r->hl.have = false;   // the holes pass read the half-edges as they were wound
    r->sp.have = false;   // a simplification mapped the faces as they were
    r->so.have = false;   // a smoothing pass belongs to the snapshot as it was
    return 0;
}

int immesh_topology_orient_last_timing(immesh_raycaster* r, float* ms) {
    if (!r || !ms) return IMMESH_E_INVAL;
    ms[0] = r->ot.ms[0]; ms[1] = r->ot.ms[1];
    return 0;
}

}  // extern "C"
