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

int ot_grow(immesh_raycaster* r, RcBuf& b, size_t bytes) { return rc_pass_grow(r->ot, b, bytes); }

int ot_oriented(immesh_raycaster* r, const char* who) {
    const int rc = rc_analysed(r, who);
    return rc ? rc : rc_passed(r, who, r->ot, "no orientation since the last analysis (immesh_topology_orient)");
}

}  // namespace

extern "C" {

int immesh_topology_orient(immesh_raycaster* r, int32_t mode, const double* viewpoint, immesh_orient_stats* stats) {
    if (!r) return IMMESH_E_INVAL;
    immesh_ctx* c = r->ctx;
    int rc;
    if ((rc = rc_analysed(r, "topology_orient"))) return rc;
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
    if ((rc = rc_pass_ready(c, s, "topology_orient", o, OT_COUNTERS, OT_COUNTERS))) return rc;
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
    if ((rc = rc_pass_begin(o, 0))) return rc;
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
    if ((rc = rc_pass_end(o, 0, 1, 0, 0, OT_COUNTERS))) return rc;   // the one read-back
    const unsigned long long* h = o.h_cnt;
    if (h[OT_ERROR]) {
        c->err = "topology_orient: a union did not finish within its step bound (a defect of the library)";
        return IMMESH_E_INTERNAL;
    }
    immesh_orient_stats& st = o.st;
    st.n_patches = (int64_t)h[OT_N_PATCHES]; st.n_orientable = (int64_t)h[OT_N_ORIENTABLE]; st.n_nonorientable = (int64_t)h[OT_N_NONORIENTABLE];
    st.largest_patch_faces = (int64_t)h[OT_LARGEST_PATCH]; st.n_faces_flipped = (int64_t)h[OT_N_FLIPPED];
    st.n_faces_nonorientable = (int64_t)h[OT_N_FACES_NONORIENTABLE]; st.n_patches_inverted = (int64_t)h[OT_N_INVERTED];
    st.n_inconsistent_before = q.st.n_inconsistent; st.n_inconsistent_after = (int64_t)h[OT_INCONSISTENT_AFTER];
    o.n_bound = n_bound;
    o.have = true;
    if (stats) *stats = st;
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
    if ((rc = rc_fetch(c, patch_out, r->ot.patch.p, (size_t)nf * 4))) return rc;
    if ((rc = rc_fetch(c, flip_out, r->ot.flip.p, (size_t)nf))) return rc;
    return rc_fetch(c, faces_out, r->ot.out.p, (size_t)nf * 12);
}

int immesh_topology_orient_patches(immesh_raycaster* r, int32_t* first_face, int32_t* n_faces, int32_t* orientable, int32_t* n_flipped,
                                   int32_t* n_inconsistent, int64_t cap, int64_t* n_out) {
    if (!r) return IMMESH_E_INVAL;
    immesh_ctx* c = r->ctx;
    int rc;
    if ((rc = ot_oriented(r, "topology_orient_patches"))) return rc;
    const RcOrient& o = r->ot;
    const int64_t n = o.st.n_patches;
    const bool wanted = first_face || n_faces || orientable || n_flipped || n_inconsistent;
    if ((rc = rc_cap(c, "topology_orient_patches", cap, n, n_out, wanted, "patches"))) return rc;
    if (!wanted || n == 0) return 0;
    (void)hipSetDevice(c->cfg.device);
    const int32_t* tab = (const int32_t*)o.tab.p;
    int32_t* const out[5] = {first_face, n_faces, orientable, n_flipped, n_inconsistent};
    const int which[5] = {OT_FIRST, OT_NFACES, OT_ORIENTABLE, OT_NFLIPPED, OT_NINCONSISTENT};
    for (int k = 0; k < 5; k++)
        if ((rc = rc_fetch(c, out[k], tab + which[k] * o.n_bound, (size_t)n * 4))) return rc;
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
    if ((rc = rc_pass_span(o, 2, 3, 1))) return rc;
    // what a successful build discards, and the hierarchy stays.  Nothing else the caster keeps depends on the order of a face's vertices: the
    // hierarchy holds boxes and face indices, and the closest-point results of the last query stay readable after a build too.
    rc_snapshot_changed(r);
    return 0;
}

int immesh_topology_orient_last_timing(immesh_raycaster* r, float* ms) {
    if (!r || !ms) return IMMESH_E_INVAL;
    ms[0] = r->ot.ms[0]; ms[1] = r->ot.ms[1];
    return 0;
}

}  // extern "C"
