// =====================================================================================================================
// Fast path of the per-voxel triangulation (included by mesh_kernels.hip): neighbourhoods of at most 64 vertices -- every voxel of the
// shipped configurations (mean n_u ~ 31, max ~ 60).  Same algorithm and the same floating-point expressions as mesh_delaunay_voxel
// (sequential-order PCA sums, Morton insertion order, Bowyer-Watson with "cavity = every triangle whose circumdisk contains p"), so the
// face set is identical bit for bit, but laid out for ONE wavefront whose critical path is what bounds the kernel:
//   * vertex i of the neighbourhood lives in lane i; after the Morton ranking the points are moved so that lane s holds the s-th point to
//     insert -- the next point is a v_readlane away, no LDS round trip;
//   * the triangulation lives in REGISTERS: slot s of the (<= 2n-2 <= 126 entry) triangle table is (lane s & 63, set s >> 6); each slot
//     keeps its three vertices' coordinates and the p-independent parts of the in-circle determinant, so the cavity search is ~14 double
//     operations per set and touches no memory;
//   * cavity boundary: each cavity triangle publishes its three directed edges in a 65 x 65 byte table in LDS and looks up their twins
//     (one write + one read round trip instead of an O(edges) search); its FIRST boundary edge is re-triangulated in place (no data
//     movement), the others are handed to freed / new slots through scalar registers (v_readlane -> masked v_mov);
//   * the skinny-face filter decides by comparing the cosine against cos(150 / 57.3) and evaluates acos only within 1e-9 of the threshold;
//   * the fresh faces go into an LDS hash set instead of a sorted list (no bitonic sort); vertex id -> local index is an LDS hash too.
// A voxel the fast path cannot finish (inconsistent predicates leave fewer new triangles than holes, slot table full) is flagged
// (vox_ntris = -1) before anything but the (identical) short axis has been written and redone by mesh_delaunay_general_kernel, which also
// takes the neighbourhoods of 65..256 vertices.  Keeping the general path out of this kernel keeps its LDS footprint at ~20 KB per
// workgroup: LDS capacity is what decides how many workgroups of the three concurrent chains (pose / mesher A / mesher B) fit a CU.
// =====================================================================================================================
#define DF_INF 64
#define DF_ES 66           /* row stride of the directed-edge table (rows / columns 0..64) */
#define DF_OLD_CAP 512
#define DF_XCAP 96           /* boundary edges of one insertion staged through LDS (beyond the one each cavity triangle keeps in place) */
#define DF_EMPTY 0xFFFFFFFFu
// The workgroup IS one wavefront: its LDS operations execute in program order, so the hand-overs through LDS inside the insertion loop need no
// s_barrier and no wait for outstanding global accesses (what __syncthreads() compiles to) -- only the compiler must keep the order.
#define DF_LDS_SYNC() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")
#define DF_COS_LIMIT (-0x1.bb5b0ad0ee9ddp-1)   /* cos(150 / 57.3): acos(x) * 57.3 > 150  <=>  x < this (up to rounding, hence the margin) */

IMD double readlane_d(double x, int k) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(x), k), hi = __builtin_amdgcn_readlane(__double2hiint(x), k);
    return __hiloint2double(hi, lo);
}
IMD unsigned long long readlane_u64(unsigned long long x, int k) {
    const unsigned int lo = (unsigned int)__builtin_amdgcn_readlane((int)(unsigned int)x, k), hi = (unsigned int)__builtin_amdgcn_readlane((int)(unsigned int)(x >> 32), k);
    return ((unsigned long long)hi << 32) | lo;
}
IMD int ff1_u64(unsigned long long x) { return __builtin_ctzll(x); }

// One triangle slot: (v0, v1, v2) counter-clockwise, local vertex indices.  DF_INF only ever sits at v2: the ghost (A, B, inf) closes the
// hull edge A -> B seen from outside.  v0 < 0: empty slot.
struct DfTri {
    int v0, v1, v2;
    double x0, y0, x1, y1;
    double qpx, qpy;   // v1 - v0
    double S, D;       // finite: the two p-independent factors of side_of_oriented_circle; ghost: S = |B - A|^2
};
// Vertex coordinates by local index live in an LDS table (cxy[DF_INF] = (0, 0)): a slot is (re)built from its three INDICES -- three 16-byte LDS
// reads -- instead of moving six doubles through chains of selects (round 2 / early round 3: ~250 of the ~700 instructions of an insertion step).
IMD void df_build(DfTri& t, const int v0, const int v1, const int v2, const double2* __restrict__ cxy) {
    const double2 c0 = cxy[v0], c1 = cxy[v1], c2 = cxy[v2];
    t.v0 = v0; t.v1 = v1; t.v2 = v2;
    t.x0 = c0.x; t.y0 = c0.y; t.x1 = c1.x; t.y1 = c1.y;
    t.qpx = t.x1 - t.x0; t.qpy = t.y1 - t.y0;
    const double rpx = c2.x - t.x0, rpy = c2.y - t.y0;
    const double Sf = rpx * (c2.x - t.x1) + rpy * (c2.y - t.y1);
    const double Df = t.qpx * rpy - t.qpy * rpx;
    const double Sg = t.qpx * t.qpx + t.qpy * t.qpy;
    const bool ghost = v2 == DF_INF;
    t.S = ghost ? Sg : Sf;
    t.D = ghost ? 0.0 : Df;
}
// the triangle (a, b, p) on the cavity's boundary edge a -> b (what mesh_delaunay_voxel stores); ghosts rotated so that inf is last
IMD void df_make(DfTri& t, const int a, const int b, const int p, const double2* __restrict__ cxy) {
    const bool ga = a == DF_INF, gb = b == DF_INF;
    const int v0 = ga ? b : (gb ? p : a), v1 = ga ? p : (gb ? a : b), v2 = (ga || gb) ? DF_INF : p;
    df_build(t, v0, v1, v2, cxy);
}
// dt_in_disk on a register slot: incircle2d(v0, v1, v2, p) > 0, resp. the half-plane test of a ghost -- the same expressions, with
// (qpx, qpy), S and D hoisted out (they do not depend on p)
IMD bool df_in_disk(const DfTri& t, double px, double py) {
    const double tpx = px - t.x0, tpy = py - t.y0;
    const double o = t.qpx * tpy - t.qpy * tpx;
    const double w = tpx * (px - t.x1) + tpy * (py - t.y1);
    const double val = o * t.S - w * t.D;
    const double d = tpx * t.qpx + tpy * t.qpy;
    const bool gin = o > 0 || (o == 0 && d > 0 && d < t.S);
    return t.v0 >= 0 && (t.v2 == DF_INF ? gin : val > 0);
}
// interior angle at P of triangle (P, Q, R) above the 150-"degree" limit of is_face_is_ok ?  (compute_angle: acos(..) * 57.3)
IMD bool df_angle_bad(double px, double py, double qx, double qy, double rx, double ry) {
    const double abx = qx - px, aby = qy - py, acx = rx - px, acy = ry - py;
    const double cosv = (abx * acx + aby * acy) / (sqrt(abx * abx + aby * aby) * sqrt(acx * acx + acy * acy));
    if (cosv < DF_COS_LIMIT - 1e-9 && cosv >= -1.0) return true;   // (below -1 -- three collinear points, rounded -- acos is NaN and the reference's `> 150` is FALSE: the face stays)
    if (cosv > DF_COS_LIMIT + 1e-9) return false;
    return acos(cosv) * 57.3 > 150;   // within the margin, outside [-1, 1] or NaN: the literal expression
}

// Bowyer-Watson over the points held by lanes 0..n-1 in insertion order (li = local vertex index, (sx, sy) = 2-D coordinates); the three
// points of the first triangle sit in lanes 0, L1, L2.  Emits the finite faces that pass the skinny-face filter into the LDS hash set
// `fh` as packed sorted local triplets and returns their number, or -1 when the voxel must take the general path.
// phase timers (IMMESH_DEBUG): accumulated in registers, flushed once per voxel (an atomic per insertion step would dominate what it measures)
#define DF_T(k) do { if (dbg) { const unsigned long long _t = __builtin_readcyclecounter(); tacc[(k) & 7] += _t - tq; tq = _t; } } while (0)
#define DF_FLUSH(base) do { if (dbg && lane == 0) { for (int _k = 0; _k < 8; _k++) if (tacc[_k]) atomicAdd(&dbg[(base) + _k], tacc[_k]); } } while (0)
template <int K>
IMD int df_triangulate(const int n, const int lane, const int li, const double sx, const double sy, const int L1, const int L2, const bool swap12,
                       unsigned char* E, unsigned int* fh, int* xi, const double2* cxy, unsigned long long* dbg, int* sc_degen) {
    unsigned long long tq = dbg ? __builtin_readcyclecounter() : 0;
    unsigned long long tacc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    DfTri T[K];
#pragma unroll
    for (int j = 0; j < K; j++) { T[j].v0 = -1; T[j].v1 = 0; T[j].v2 = 0; T[j].x0 = T[j].y0 = T[j].x1 = T[j].y1 = 0; T[j].qpx = T[j].qpy = T[j].S = T[j].D = 0; }
    {   // first triangle + its three ghosts in slots 0..3 (lanes 0..3 of set 0)
        const int la = swap12 ? L2 : L1, lb = swap12 ? L1 : L2;
        const int i0 = __builtin_amdgcn_readlane(li, 0), i1 = __builtin_amdgcn_readlane(li, la), i2 = __builtin_amdgcn_readlane(li, lb);
        const int w0 = lane == 0 ? i0 : (lane == 1 ? i2 : (lane == 2 ? i0 : i1));
        const int w1 = lane == 0 ? i1 : (lane == 1 ? i1 : (lane == 2 ? i2 : i0));
        const int w2 = lane == 0 ? i2 : DF_INF;
        DfTri t;
        df_build(t, w0, w1, w2, cxy);
        if (lane < 4) T[0] = t;
    }
    int nt = 4;                          // high-water mark of the slot table
    unsigned long long freem[K];         // dead slots below the high-water mark, per set
#pragma unroll
    for (int j = 0; j < K; j++) freem[j] = 0;
    bool bail = false;
    for (int oi = 1; oi < n; oi++) {
        if (oi == L1 || oi == L2) continue;
        const int pi = __builtin_amdgcn_readlane(li, oi);
        const double px = readlane_d(sx, oi), py = readlane_d(sy, oi);
        // ---- cavity: every live triangle whose circumdisk contains p
        bool in[K];
        unsigned long long cm[K];
        int ncav = 0;
        const bool hi = K > 1 && nt > 64;   // the second register set holds something (wave-uniform): until then its share of every phase is skipped
#pragma unroll
        for (int j = 0; j < K; j++) {
            if (j == 0 || hi) { in[j] = df_in_disk(T[j], px, py); cm[j] = __ballot(in[j]); ncav += __popcll(cm[j]); }
            else { in[j] = false; cm[j] = 0; }
        }
        DF_T(16);
        if (ncav == 0) continue;         // duplicate / on every circle: not inserted (counted behind the loop, from Euler's relation)
        // ---- boundary edges: publish the directed edges under this insertion's stamp (oi is unique per insertion of a voxel and never 0: nothing to
        //      clear afterwards; the table is zeroed once per voxel), look up the twins
        const unsigned char stamp = (unsigned char)oi;
#pragma unroll
        for (int j = 0; j < K; j++)
            if (in[j]) { E[T[j].v1 * DF_ES + T[j].v2] = stamp; E[T[j].v2 * DF_ES + T[j].v0] = stamp; E[T[j].v0 * DF_ES + T[j].v1] = stamp; }
        DF_LDS_SYNC();
        bool bd[K][3];
#pragma unroll
        for (int j = 0; j < K; j++) {
            bd[j][0] = bd[j][1] = bd[j][2] = false;
            if (in[j]) { bd[j][0] = E[T[j].v2 * DF_ES + T[j].v1] != stamp; bd[j][1] = E[T[j].v0 * DF_ES + T[j].v2] != stamp; bd[j][2] = E[T[j].v1 * DF_ES + T[j].v0] != stamp; }
        }
        int k0[K];                       // the boundary edge that is re-triangulated in place (3 = none: the slot dies)
        int ndies = 0;                   // cavity triangles without a boundary edge (scalar: from the ballots below)
#pragma unroll
        for (int j = 0; j < K; j++) {
            k0[j] = 3;
            if (j == 0 || hi) {
                k0[j] = bd[j][0] ? 0 : (bd[j][1] ? 1 : (bd[j][2] ? 2 : 3));
                const bool dies = in[j] && k0[j] == 3;   // cavity triangle without a boundary edge: its slot is free for the edges below
                const unsigned long long dm = __ballot(dies);
                ndies += __popcll(dm);
                freem[j] |= dm;
                if (dies) T[j].v0 = -1;
            }
        }
        DF_T(17);
        // ---- the other boundary edges of a cavity triangle go to freed slots first, then to new ones.  They are staged through LDS and taken by
        //      their target slots in parallel (round 2 handed them over one by one through scalar registers: ~700 cycles per edge, half of the
        //      insertion loop).  Which slot an edge lands in does not matter: the face set does not depend on the slot layout.
        //      A slot is rebuilt AT MOST ONCE per insertion -- in place on its first boundary edge (it stays a cavity triangle's slot), or with a staged
        //      edge (a freed slot, or a new one at the high-water mark) -- so the edge is only CHOSEN here and there is one df_make per register set at the
        //      end (round 4; rounds 2-3 rebuilt the takers and the in-place slots in two passes: one LDS round trip + ~30 double operations more per set).
        int ra[K], rb[K];                // the edge (a -> b) slot `lane` of set j is rebuilt on; ra < 0: not rebuilt
#pragma unroll
        for (int j = 0; j < K; j++) {
            ra[j] = -1; rb[j] = 0;
            if (in[j] && k0[j] < 3) {
                const int kk = k0[j];
                ra[j] = kk == 0 ? T[j].v1 : (kk == 1 ? T[j].v2 : T[j].v0); rb[j] = kk == 0 ? T[j].v2 : (kk == 1 ? T[j].v0 : T[j].v1);
            }
        }
        {
            const unsigned long long lt = (1ull << lane) - 1ull;
            int base = 0;
            int myidx[K][2];
#pragma unroll
            for (int j = 0; j < K; j++)
#pragma unroll
                for (int k = 1; k < 3; k++) {
                    myidx[j][k - 1] = -1;
                    if (j == 0 || hi) {
                        const bool ex = bd[j][k] && k0[j] < k;
                        const unsigned long long em = __ballot(ex);
                        myidx[j][k - 1] = ex ? base + __popcll(em & lt) : -1;
                        base += __popcll(em);
                    }
                }
            const int X = base;
            // The triangles that tested in-disk must be ONE disk: |boundary| == |cavity| + 2 (Euler; ghosts close the sphere).  Every cavity triangle that
            // does not die has one boundary edge re-triangulated in place and X counts the others: |boundary| = (ncav - ndies) + X, so the test is
            // X - ndies == 2 -- two scalar values that exist anyway.  On cocircular / collinear input the determinants are rounding noise around zero
            // and the set need not be a disk: the general path then takes the connected part around the triangle that contains p, as the checker does
            // (oracle/orc_delaunay.hpp header).  Never on points in general position (0 of 300 000 insertions of the bench's stream, CPU count).
            if (X - ndies != 2) { bail = true; break; }
            if (X > DF_XCAP) { bail = true; break; }   // (cannot hold at n <= 64: a cavity's boundary has at most n + 1 = 65 vertices, hence edges)
            if (X > 0) {
#pragma unroll
                for (int j = 0; j < K; j++)
#pragma unroll
                    for (int k = 1; k < 3; k++) {
                        const int e = myidx[j][k - 1];
                        if (e >= 0) xi[e] = k == 1 ? (T[j].v2 | (T[j].v0 << 16)) : (T[j].v0 | (T[j].v1 << 16));   // edge k of (v0, v1, v2): k = 1: v2 -> v0, k = 2: v0 -> v1
                    }
                DF_LDS_SYNC();
                // a slot is either a freed one (rank among the freed slots, in slot order) or a new one at the high-water mark -- never both
                const int F0 = __popcll(freem[0]), F1 = hi ? __popcll(freem[K - 1]) : 0, F = F0 + F1;
                const int extra = X > F ? X - F : 0;
                if (nt + extra > 64 * K) { bail = true; break; }   // (cannot hold at n <= 64: the slot table peaks at 2 n - 2 = 126 entries)
#pragma unroll
                for (int f = 0; f < K; f++) {
                    if (f > 0 && !hi && nt + extra <= 64) continue;
                    const unsigned long long fm = (f == 0 || hi) ? freem[f] : 0ull;
                    const int rank = (f == 0 ? 0 : F0) + __popcll(fm & lt);
                    const bool take_f = ((fm >> lane) & 1ull) && rank < X;
                    const int e = f * 64 + lane - nt;
                    const bool take_n = e >= 0 && e < extra;
                    if (take_f || take_n) { const int ab = xi[take_f ? rank : F + e]; ra[f] = ab & 0xFFFF; rb[f] = ab >> 16; }
                    freem[f] = fm & ~__ballot(take_f);
                }
                nt += extra;
                asm volatile("" ::: "memory");   // (LDS operations of one wavefront execute in order: the next insertion's stores cannot pass these loads)
            }
        }
        DF_T(18);
        // ---- the rebuild: every slot that got an edge, once
        const bool hi2 = K > 1 && nt > 64;
#pragma unroll
        for (int j = 0; j < K; j++)
            if ((j == 0 || hi2) && ra[j] >= 0) df_make(T[j], ra[j], rb[j], pi, cxy);
        DF_T(19);
    }
    if (dbg && lane == 0) { atomicAdd(&dbg[15], (unsigned long long)n); if (bail) atomicAdd(&dbg[7], 1ull); }
    if (bail) { DF_FLUSH(16); return -1; }
    {   // points that were NOT inserted (immesh_counters_t::n_degenerate_skips), without a counter carried through the insertion loop (one more live register there
        // cost the launch 29 VGPRs): a triangulation of V finite vertices and the vertex at infinity has 2 V - 2 slots alive (finite + ghost faces)
        int alive = 0;
#pragma unroll
        for (int j = 0; j < K; j++) alive += (int)__popcll(__ballot(T[j].v0 >= 0));
        const int n_skip = n - (alive + 2) / 2;
        if (n_skip > 0 && lane == 0) atomicAdd(sc_degen, n_skip);
    }
    // ---- finite faces that pass the skinny-face filter -> hash set of packed sorted local triplets
    int nf = 0;
#pragma unroll
    for (int j = 0; j < K; j++) {
        bool ok = T[j].v0 >= 0 && T[j].v2 != DF_INF;
        if (ok) {
            const double2 c2 = cxy[T[j].v2];
            ok = !df_angle_bad(T[j].x0, T[j].y0, T[j].x1, T[j].y1, c2.x, c2.y) && !df_angle_bad(T[j].x1, T[j].y1, T[j].x0, T[j].y0, c2.x, c2.y) &&
                 !df_angle_bad(c2.x, c2.y, T[j].x0, T[j].y0, T[j].x1, T[j].y1);
        }
        if (ok) {
            unsigned l0 = (unsigned)T[j].v0, l1 = (unsigned)T[j].v1, l2 = (unsigned)T[j].v2;   // local index order == vertex id order (ids ascending)
            if (l0 > l1) { const unsigned x = l0; l0 = l1; l1 = x; }
            if (l1 > l2) { const unsigned x = l1; l1 = l2; l2 = x; }
            if (l0 > l1) { const unsigned x = l0; l0 = l1; l1 = x; }
            const unsigned int key = (l0 << 20) | (l1 << 10) | l2;
            unsigned int h = (key * 2654435761u) >> 24;
            for (int probe = 0; probe < 256; probe++) {
                if (atomicCAS(&fh[h], DF_EMPTY, key) == DF_EMPTY) break;
                h = (h + 1) & 255;
            }
        }
        nf += __popcll(__ballot(ok));
    }
    DF_T(20);
    DF_FLUSH(16);
    return nf;
}

// PART 0: the whole voxel in one launch (sharded mesher: everything on one stream).
// PART 1 / 2 (round 6): the launch cut in two.  The TRIANGULATION of a neighbourhood (PCA, projection, insertion order, Bowyer-Watson, skinny-face
//   filter: 80 % of the launch) needs nothing but the neighbourhood search's results of its own job -- vertex positions are immutable -- so it runs on a
//   stream of its own right behind phase A (mesh_tri64_kernel) and leaves the fresh faces (the 256-word hash set as it stands), their number and the
//   short axis in per-parity arrays (MeshDev::tri_*).  Only the DIFF against the live triangle set (smoothed positions as this voxel's turn sees them, old
//   set, classification, insertions: mesh_diff64_kernel) has to wait for the previous job's commit on the phase-B stream.  Phase B was the mesher's period
//   (delaunay64 102 + the tail 48 + 13 us of queue gap = the 163 us the whole pipeline ran at, profiles/r06_marks_*.txt); its head is ~20 us now.
template <int PART>
__global__ __launch_bounds__(64) void mesh_delaunay64_kernel(MeshDev m_in) {
    __builtin_amdgcn_s_setprio(MESH_B_PRIO);
    MESH_MARK(m_in, PART == 2 ? 12 : 5);
    MESH_DYN(m_in);
    __shared__ double colb[6][66];                    // per-component columns of the sequential sums
    __shared__ double st_x[64], st_y[64];
    __shared__ int st_i[64];
    __shared__ unsigned int E32[(65 * DF_ES + 8) / 4]; // directed-edge table (bytes): the stamp of the insertion that last published the edge
    __shared__ int ids[64];
    __shared__ unsigned long long idh[128];           // vertex id -> local index: (id << 8 | index), ~0 = empty
    __shared__ double sm[64 * 3];                     // smoothed positions as this voxel's turn in the sequential loop would see them
    __shared__ unsigned int fh[256];                  // fresh faces: packed sorted local triplet, bit 31 = also in the old set
    __shared__ int s_cnt[2];
    __shared__ int old_t[DF_OLD_CAP], old_v1[DF_OLD_CAP], old_v2[DF_OLD_CAP];
    __shared__ unsigned short old_i[DF_OLD_CAP];
    __shared__ int xi[DF_XCAP];                       // staged boundary edges: a | b << 16
    __shared__ double2 cxy[66];                       // 2-D coordinates by local vertex index; [DF_INF] = (0, 0)
    unsigned char* E = (unsigned char*)E32;
    const int lane = threadIdx.x;
    const int n_active = min(m.sc[SC_ACTIVE], m.cap_active);
    for (int r = blockIdx.x; r < n_active; r += gridDim.x) {
    const int n = m.rel_n[r];
    if (n == 0) { if (PART != 1 && lane == 0) m.vox_ntris[r] = 0; continue; }   // sharded mesher: a voxel another rank triangulates (its marks arrive by all-gather)
    if (n > 64) continue;                                           // mesh_delaunay_general_kernel
    if (PART != 2) for (int k = lane; k < (65 * DF_ES + 8) / 4; k += 64) E32[k] = 0;   // directed-edge stamps of this voxel's insertions (mesh_delaunay64.inc: df_triangulate)
    unsigned long long tprev = m.dbg ? __builtin_readcyclecounter() : 0;
    const unsigned long long tvox0 = tprev;
    const int vi = m.act_vox_s[r];
    // ---- vertex `lane` of the neighbourhood: id, position; the dependent gathers of the later phases are started here
    int id = 0, vvox = 0, ahead = -1;
    double p3[3] = {0, 0, 0};
    if (lane < n) {
        id = m.rel_ids[(size_t)r * MV_REL_CAP + lane];
        if (PART != 2) { p3[0] = (double)m.v_pos[(size_t)id * 3 + 0]; p3[1] = (double)m.v_pos[(size_t)id * 3 + 1]; p3[2] = (double)m.v_pos[(size_t)id * 3 + 2]; }
        vvox = m.v_voxel[id];
        if (PART != 1) ahead = m.a_head[id];   // (the live triangle lists belong to the phase-B stream: the previous job's commit edits them)
        ids[lane] = id;
    }
    idh[lane] = ~0ull; idh[lane + 64] = ~0ull;
    if (PART != 2) { fh[lane] = DF_EMPTY; fh[lane + 64] = DF_EMPTY; fh[lane + 128] = DF_EMPTY; fh[lane + 192] = DF_EMPTY; }
    else {   // the fresh faces as mesh_tri64_kernel left them
        const unsigned int* src = m.tri_fh + (size_t)r * 256;
        fh[lane] = src[lane]; fh[lane + 64] = src[lane + 64]; fh[lane + 128] = src[lane + 128]; fh[lane + 192] = src[lane + 192];
    }
    if (lane == 0) { s_cnt[0] = 0; s_cnt[1] = 0; }
    if (PART != 2 && lane < n) { colb[0][lane] = p3[0]; colb[1][lane] = p3[1]; colb[2][lane] = p3[2]; }
    __syncthreads();
    if (lane < n) {
        unsigned int h = ((unsigned int)id * 2654435761u) >> 25;
        const unsigned long long ent = ((unsigned long long)(unsigned int)id << 8) | (unsigned long long)lane;
        for (int probe = 0; probe < 128; probe++) { if (atomicCAS(&idh[h], ~0ull, ent) == ~0ull) break; h = (h + 1) & 127; }
    }
    DBG_T(0);
    int nf = 0;
    bool general = false;
    if (PART == 2) {
        nf = m.tri_nf[r];
        general = nf < 0;
        if (n >= 3 && lane < 3) m.vx_short_axis[(size_t)vi * 3 + lane] = m.tri_axis[(size_t)r * 3 + lane];
    }
    if (PART != 2 && n >= 3) {
        // ---- centre and covariance: sequential sums in vertex order (bit-identical to the CPU path), one lane per component; the loads of a
        //      batch are independent, only the additions are chained
        auto seq_sum = [&](const double* col) {
            double acc = 0;
            int i = 0;
            for (; i + 8 <= n; i += 8) {
                double v[8];
#pragma unroll
                for (int u = 0; u < 8; u++) v[u] = col[i + u];
#pragma unroll
                for (int u = 0; u < 8; u++) acc += v[u];
            }
            for (; i < n; i++) acc += col[i];
            return acc;
        };
        unsigned long long tq = m.dbg ? __builtin_readcyclecounter() : 0;
        unsigned long long tacc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        unsigned long long* dbg = m.dbg;
        double acc = seq_sum(colb[lane < 3 ? lane : 0]);
        acc /= (double)n;
        const double c[3] = {readlane_d(acc, 0), readlane_d(acc, 1), readlane_d(acc, 2)};
        __syncthreads();
        const double d3[3] = {p3[0] - c[0], p3[1] - c[1], p3[2] - c[2]};
        if (lane < n) {
            colb[0][lane] = d3[0] * d3[0]; colb[1][lane] = d3[0] * d3[1]; colb[2][lane] = d3[0] * d3[2];
            colb[3][lane] = d3[1] * d3[1]; colb[4][lane] = d3[1] * d3[2]; colb[5][lane] = d3[2] * d3[2];
        }
        __syncthreads();
        double cv = seq_sum(colb[lane < 6 ? lane : 0]);
        cv /= (double)n;
        const double c00 = readlane_d(cv, 0), c01 = readlane_d(cv, 1), c02 = readlane_d(cv, 2), c11 = readlane_d(cv, 3), c12 = readlane_d(cv, 4), c22 = readlane_d(cv, 5);
        const double cov[9] = {c00, c01, c02, c01, c11, c12, c02, c12, c22};
        DF_T(24);
        double ev[3], U[9];
        sym3_eigen_jacobi(cov, ev, U);  // SelfAdjointEigenSolver::compute, mesh_rec_geometry.cpp:199-200 (eigenvalues ascending)
        DF_T(25);
        int o0 = 0, o1 = 1, o2 = 2;     // stable ascending order of three
        if (ev[o1] < ev[o0]) { const int t = o0; o0 = o1; o1 = t; }
        if (ev[o2] < ev[o1]) { const int t = o1; o1 = o2; o2 = t; if (ev[o1] < ev[o0]) { const int t2 = o0; o0 = o1; o1 = t2; } }
        double sh[3] = {U[0 * 3 + o0], U[1 * 3 + o0], U[2 * 3 + o0]};
        double mid[3] = {U[0 * 3 + o1], U[1 * 3 + o1], U[2 * 3 + o1]};
        {
            const double X0[3] = {readlane_d(d3[0], 0), readlane_d(d3[1], 0), readlane_d(d3[2], 0)};
            const double X1[3] = {readlane_d(d3[0], 1), readlane_d(d3[1], 1), readlane_d(d3[2], 1)};
            if (X0[0] * sh[0] + X0[1] * sh[1] + X0[2] * sh[2] < 0) { sh[0] *= -1; sh[1] *= -1; sh[2] *= -1; }          // :204-207
            if (X1[0] * mid[0] + X1[1] * mid[1] + X1[2] * mid[2] < 0) { mid[0] *= -1; mid[1] *= -1; mid[2] *= -1; }    // :208-211
        }
        double lg[3];
        cross3(sh, mid, lg);
        if (lane == 0) {
            double* const axis_out = PART == 1 ? m.tri_axis + (size_t)r * 3 : m.vx_short_axis + (size_t)vi * 3;   // (PART 1: the voxel record is the phase-B stream's)
            axis_out[0] = sh[0]; axis_out[1] = sh[1]; axis_out[2] = sh[2];
        }
        // ---- 2-D projection
        const double u = d3[0] * lg[0] + d3[1] * lg[1] + d3[2] * lg[2];
        const double v = d3[0] * mid[0] + d3[1] * mid[1] + d3[2] * mid[2];
        double mn0 = lane < n ? u : 1e300, mn1 = lane < n ? v : 1e300, mx0 = lane < n ? u : -1e300, mx1 = lane < n ? v : -1e300;
        mn0 = wave_min_d(mn0); mn1 = wave_min_d(mn1); mx0 = wave_max_d(mx0); mx1 = wave_max_d(mx1);
        const double ext = fmax(mx0 - mn0, mx1 - mn1);
        // ---- insertion order: Morton code over the bounding box, ties by index; rank = number of smaller keys (keys are distinct)
        unsigned long long key = ~0ull;
        if (lane < n) {
            const double f0 = ext > 0 ? (u - mn0) / ext : 0, f1 = ext > 0 ? (v - mn1) / ext : 0;
            const unsigned int q0 = (unsigned int)fmin(65535.0, fmax(0.0, f0 * 65535.0)), q1 = (unsigned int)fmin(65535.0, fmax(0.0, f1 * 65535.0));
            unsigned int code = 0;
#pragma unroll
            for (int b = 0; b < 16; b++) code |= (((q0 >> b) & 1u) << (2 * b)) | (((q1 >> b) & 1u) << (2 * b + 1));
            key = ((unsigned long long)code << 16) | (unsigned long long)lane;
        }
        DF_T(26);
        DF_FLUSH(24);
        DBG_T(1);
        int rank = 0;
        for (int j = 0; j < n; j++) rank += readlane_u64(key, j) < key ? 1 : 0;
        if (lane < n) { st_x[rank] = u; st_y[rank] = v; st_i[rank] = lane; }
        __syncthreads();
        double sx = 0, sy = 0;
        int li = 0;
        if (lane < n) { sx = st_x[lane]; sy = st_y[lane]; li = st_i[lane]; }
        if (lane < n) cxy[li] = make_double2(sx, sy);
        if (lane == 0) cxy[DF_INF] = make_double2(0.0, 0.0);
        DF_LDS_SYNC();
        DBG_T(2);
        // ---- first non-degenerate triangle: point 0, the next distinct point, the next point not collinear with them
        const double x0 = readlane_d(sx, 0), y0 = readlane_d(sy, 0);
        const unsigned long long m1 = __ballot(lane >= 1 && lane < n && (sx != x0 || sy != y0));
        if (m1) {
            const int L1 = ff1_u64(m1);
            const double x1 = readlane_d(sx, L1), y1 = readlane_d(sy, L1);
            const double p0[2] = {x0, y0}, p1[2] = {x1, y1}, ps[2] = {sx, sy};
            const unsigned long long m2 = __ballot(lane >= 1 && lane < n && lane != L1 && orient2d(p0, p1, ps) != 0);
            if (m2) {
                const int L2 = ff1_u64(m2);
                const double p2[2] = {readlane_d(sx, L2), readlane_d(sy, L2)};
                const bool swap12 = orient2d(p0, p1, p2) < 0;
                nf = n <= 33 ? df_triangulate<1>(n, lane, li, sx, sy, L1, L2, swap12, E, fh, xi, cxy, m.dbg, &m.sc[SC_DEGEN]) : df_triangulate<2>(n, lane, li, sx, sy, L1, L2, swap12, E, fh, xi, cxy, m.dbg, &m.sc[SC_DEGEN]);
                if (nf < 0) general = true;
            }
        }
        DBG_T(3);
    }
    if (PART == 1) {
        // ---- hand-over to mesh_diff64_kernel: the hash set as it stands (a kilobyte per voxel), the face count (-1: the general path redoes the voxel)
        unsigned int* dst = m.tri_fh + (size_t)r * 256;
        dst[lane] = fh[lane]; dst[lane + 64] = fh[lane + 64]; dst[lane + 128] = fh[lane + 128]; dst[lane + 192] = fh[lane + 192];
        if (lane == 0) m.tri_nf[r] = general ? -1 : nf;
        if (m.dbg && lane == 0) atomicMax(&m.dbg[14], ((__builtin_readcyclecounter() - tvox0) << 16) | (unsigned long long)n);
        __syncthreads();
        continue;
    }
    if (general) { if (lane == 0) m.vox_ntris[r] = -1; continue; }   // handed to mesh_delaunay_general_kernel (nothing but the short axis has been written)
    // ---- smoothed positions of the neighbourhood (correct_triangle_index reads them)
    if (lane < n) smooth_seen(m, id, r, &sm[lane * 3]);
    __syncthreads();
    DBG_T(4);
    // ---- old = live triangles with all three vertices in the neighbourhood (find_relative_triangulation_combination), via the
    //      min-vertex lists; old \ fresh -> remove, old & fresh -> existing (flip rewritten), fresh \ old -> add
    const double* sa = (PART == 2 && n >= 3) ? m.tri_axis + (size_t)r * 3 : m.vx_short_axis + (size_t)vi * 3;
    const double short_axis[3] = {sa[0], sa[1], sa[2]};
    int* touched = m.vox_tris + (size_t)r * (2 * MV_REL_CAP);
    const unsigned long long wbase = ((unsigned long long)(unsigned int)m.seq << 32) | ((unsigned long long)(unsigned int)r << 1);
    auto local_of = [&](int gid) -> int {   // local index of a vertex id, -1 if it is not in the neighbourhood
        unsigned int h = ((unsigned int)gid * 2654435761u) >> 25;
        for (int probe = 0; probe < 128; probe++) {
            const unsigned long long e = idh[h];
            if (e == ~0ull) return -1;
            if ((int)(e >> 8) == gid) return (int)(e & 0xFF);
            h = (h + 1) & 127;
        }
        return -1;
    };
    auto classify = [&](int t, int i, int g1, int g2) {
        const int l1 = local_of(g1), l2 = local_of(g2);
        if (l1 < 0 || l2 < 0) return;   // not entirely inside this neighbourhood
        const unsigned int key = ((unsigned int)i << 20) | ((unsigned int)l1 << 10) | (unsigned int)l2;
        bool found = false;
        unsigned int h = (key * 2654435761u) >> 24;
        for (int probe = 0; probe < 256; probe++) {
            const unsigned int e = fh[h];
            if (e == DF_EMPTY) break;
            if ((e & 0x7FFFFFFFu) == key) { atomicOr(&fh[h], 0x80000000u); found = true; break; }
            h = (h + 1) & 255;
        }
        if (found) {
            const int fl = flip_of(&sm[i * 3], &sm[l1 * 3], &sm[l2 * 3], sp.cam, short_axis);
            atomicMax(&m.t_word[t], wbase | (unsigned long long)fl);
            touched[atomicAdd(&s_cnt[0], 1)] = t;
        } else if (atomicExch(&m.t_rem_seq[t], m.seq) != m.seq) {
            list_push(m, m.list_rem, SC_REM, t);
        }
    };
    // (1) gather: every lane walks the min-vertex list of its vertex and appends the live triangles to one LDS list ...
    for (int ch = ahead; ch >= 0;) {
        const int4* cp = (const int4*)(m.a_chunks + (size_t)ch * MV_ADJ_STRIDE);
        const int4 q0 = cp[0], q1 = cp[1], q2 = cp[2], q3 = cp[3];   // one 64-byte chunk: 5 x (triangle, v1, v2) + next
        const int e[MV_ADJ_STRIDE] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, q3.x, q3.y, q3.z, q3.w};
#pragma unroll
        for (int sl = 0; sl < MV_ADJ_SLOTS; sl++) {
            if (e[sl * 3] < 0) continue;
            const int pos = atomicAdd(&s_cnt[1], 1);
            if (pos < DF_OLD_CAP) { old_t[pos] = e[sl * 3]; old_v1[pos] = e[sl * 3 + 1]; old_v2[pos] = e[sl * 3 + 2]; old_i[pos] = (unsigned short)lane; }
        }
        ch = e[MV_ADJ_STRIDE - 1];
    }
    __syncthreads();
    // (2) ... then the list is classified with all lanes busy
    const int nold = s_cnt[1];
    if (nold > DF_OLD_CAP) {
        // more live triangles around this voxel than the LDS list holds: classify them straight from the vertex lists (same decisions)
        for (int ch = ahead; ch >= 0; ch = m.a_chunks[(size_t)ch * MV_ADJ_STRIDE + MV_ADJ_STRIDE - 1])
            for (int sl = 0; sl < MV_ADJ_SLOTS; sl++) {
                const int t = m.a_chunks[(size_t)ch * MV_ADJ_STRIDE + sl * 3];
                if (t >= 0) classify(t, lane, m.a_chunks[(size_t)ch * MV_ADJ_STRIDE + sl * 3 + 1], m.a_chunks[(size_t)ch * MV_ADJ_STRIDE + sl * 3 + 2]);
            }
    } else {
        for (int k = lane; k < nold; k += 64) classify(old_t[k], (int)old_i[k], old_v1[k], old_v2[k]);
    }
    __syncthreads();
    DBG_T(5);
    // (3) fresh faces that were not in the old set: insert.  The hash set scatters them unevenly over the lanes (a lane may hold 0..4); each insert
    //     is a chain of dependent global round trips, so they are first compacted into a dense list -- one or two per lane
    unsigned int* addl = (unsigned int*)old_t;   // (the old-triangle list is dead by now)
    {
        int base = 0;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const unsigned int pk = fh[q * 64 + lane];
            const bool is_add = !(pk & 0x80000000u);   // neither empty nor already live
            const unsigned long long mk = __ballot(is_add);
            if (is_add) addl[base + __popcll(mk & ((1ull << lane) - 1ull))] = pk;
            base += __popcll(mk);
        }
        __syncthreads();
        int spare = -1;
        for (int e = lane; e < base; e += 64) {
            const unsigned int pk = addl[e];
            const int la = (int)(pk >> 20), lb = (int)((pk >> 10) & 1023), lc = (int)(pk & 1023);
            const int t = tri_find_or_insert(m, ids[la], ids[lb], ids[lc], &spare);
            if (t < 0) continue;
            const int fl = flip_of(&sm[la * 3], &sm[lb * 3], &sm[lc * 3], sp.cam, short_axis);
            atomicMax(&m.t_word[t], wbase | (unsigned long long)fl);
            touched[atomicAdd(&s_cnt[0], 1)] = (int)((unsigned int)t | TRI_ADD_BIT);
        }
    }
    __syncthreads();
    if (lane == 0) { m.vox_ntris[r] = s_cnt[0]; atomicAdd(&m.sc[SC_TV], nf); }
    __syncthreads();
    DBG_T(6);
    if (PART == 0 && m.dbg && lane == 0) atomicMax(&m.dbg[14], ((__builtin_readcyclecounter() - tvox0) << 16) | (unsigned long long)n);
    }
}
static constexpr auto mesh_tri64_kernel = mesh_delaunay64_kernel<1>;    // (names of their own for the in-library profiler)
static constexpr auto mesh_diff64_kernel = mesh_delaunay64_kernel<2>;
