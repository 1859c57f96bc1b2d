// Vertex colours from camera images for gfx950 (include/immesh_colour.h has the exact contract these kernels implement).
//   mark / compact   RECENT sets: the voxels of MeshDev::recent walked through vx_pts / vx_npts into a flag per vertex, compacted by prefix sum
//                    (ascending vertex id, whatever order the voxels were visited in)
//   select           one lane per candidate, coalesced reads of v_pos: distance, projection and gates, then the sequential "nearer takes the cell" rule
//                    in its order-free form on a dense table of cells -- three passes of integer atomics (min of the float depth's bits, largest index
//                    below it in double, smallest index equal to it), the holders compacted by prefix sum
//   dmin             block reduction + one integer atomicMin per workgroup on the order-preserving bit pattern of the double
//   update           one lane per vertex of the render set: gates, projection, the four 8-bit taps of the interleaved image (served from L2: a
//                    640 x 480 frame is 0.9 MB, the taps of one vertex share at most two lines), update_rgb on the SoA state; integer counters by
//                    one atomic per workgroup, the photometric error as one partial per workgroup (no float atomics: the sum has a fixed order)
// Double arithmetic is written in the contract's order; the library builds with -ffp-contract=off, so nothing is fused.
#include "colour.hpp"

namespace {

__device__ __forceinline__ unsigned long long cl_key(double x) {   // order-preserving: a < b <=> key(a) < key(b)
    const unsigned long long b = (unsigned long long)__double_as_longlong(x);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

struct ClProj { double d[3], u, v; bool front, ok; };

// the contract's Pose + Project for vertex id
__device__ __forceinline__ ClProj cl_project(const ClCam& c, const float* __restrict__ v_pos, int id) {
    ClProj r;
    const double p[3] = {(double)v_pos[3 * (size_t)id], (double)v_pos[3 * (size_t)id + 1], (double)v_pos[3 * (size_t)id + 2]};
    for (int k = 0; k < 3; k++) r.d[k] = p[k] - c.pos[k];
    double pc[3];
    for (int k = 0; k < 3; k++) pc[k] = ((c.rot[k] * p[0] + c.rot[3 + k] * p[1]) + c.rot[6 + k] * p[2]) + c.tc[k];
    r.front = !(pc[2] < 0.001);
    r.u = (pc[0] * c.fx) / pc[2] + c.cx;
    r.v = (pc[1] * c.fy) / pc[2] + c.cy;
    r.ok = r.front && r.u >= c.u_lo && ceil(r.u) < c.u_hi && r.v >= c.v_lo && ceil(r.v) < c.v_hi;
    return r;
}
__device__ __forceinline__ double cl_norm(const double* d) { return sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]); }

__device__ __forceinline__ int cl_r8(double x) {   // saturate_cast<uchar>(double): round half to even, clamp
    const double r = rint(x);
    return r < 0.0 ? 0 : (r > 255.0 ? 255 : (int)r);
}

// getSubPixel<cv::Vec3b>: (u, v) available, so 1 <= floor < cols (rows); a tap one past the image has weight 0 and is read from the last column (row)
__device__ __forceinline__ void cl_sample(const ClCam& c, const uint8_t* __restrict__ img, double u, double v, double* out) {
    const double fr = floor(v), fc = floor(u);
    const double a = v - fr, b = u - fc;
    const int r0 = (int)fr, c0 = (int)fc;
    const int r1 = min(r0 + 1, c.rows - 1), c1 = min(c0 + 1, c.cols - 1);
    const uint8_t* p00 = img + (size_t)r0 * c.stride + 3 * (size_t)c0;
    const uint8_t* p10 = img + (size_t)r1 * c.stride + 3 * (size_t)c0;
    const uint8_t* p01 = img + (size_t)r0 * c.stride + 3 * (size_t)c1;
    const uint8_t* p11 = img + (size_t)r1 * c.stride + 3 * (size_t)c1;
    const double w00 = (1.0 - a) * (1.0 - b), w10 = a * (1.0 - b), w01 = (1.0 - a) * b, w11 = a * b;
    for (int k = 0; k < 3; k++) {
        const int t00 = cl_r8(w00 * (double)p00[k]), t10 = cl_r8(w10 * (double)p10[k]), t01 = cl_r8(w01 * (double)p01[k]), t11 = cl_r8(w11 * (double)p11[k]);
        out[k] = (double)min(min(min(t00 + t10, 255) + t01, 255) + t11, 255);
    }
}

// RGB_pts::update_rgb on vertex id; *first = 1 when the call initialised the vertex
__device__ __forceinline__ int cl_update_rgb(const ClState& st, int id, const double* c, double obs_dis, double sigma, double t, double e, int* first) {
    *first = 0;
    if (c[0] == 0.0 && c[1] == 0.0 && c[2] == 0.0) return 0;
    if (c[0] > 255.0 && c[1] > 255.0 && c[2] > 255.0) return 0;
    const double s_dis = st.obs_dis[id];
    if (s_dis != 0.0 && obs_dis > s_dis * 1.1) return 0;
    const int n = st.n_obs[id];
    if (n == 0) {
        st.last_obs_time[id] = t;
        st.obs_dis[id] = obs_dis;
        st.first_exposure[id] = e;
        for (int k = 0; k < 3; k++) { st.rgb[k][id] = c[k] * e; st.cov[k][id] = sigma; }
        st.n_obs[id] = 1;
        *first = 1;
        return 0;
    }
    const double last = st.last_obs_time[id];
    double first_e = st.first_exposure[id];
    double rgb[3];
    for (int k = 0; k < 3; k++) {
        double cov = st.cov[k][id] + 0.15 * (t - last);
        const double old = cov;
        cov = sqrt(1.0 / (1.0 / cov / cov + 1.0 / sigma / sigma));
        rgb[k] = cov * cov * (st.rgb[k][id] / old / old + c[k] * e / sigma / sigma);
        st.cov[k][id] = cov;
    }
    const double q[3] = {rgb[0] / first_e, rgb[1] / first_e, rgb[2] / first_e};
    double mx = q[0];
    if (q[1] > mx) mx = q[1];
    if (q[2] > mx) mx = q[2];
    if (mx > 255.0)
        for (int k = 0; k < 3; k++) rgb[k] = rgb[k] * 254.999 / mx;
    for (int k = 0; k < 3; k++) st.rgb[k][id] = rgb[k];
    if (obs_dis < s_dis) st.obs_dis[id] = obs_dis;
    st.last_obs_time[id] = t;
    st.n_obs[id] = n + 1;
    st.first_exposure[id] = (first_e * (double)(n + 1) + e) / (double)(n + 2);
    return 1;
}

__global__ void __launch_bounds__(CL_BLOCK) cl_state_init_kernel(ClState st) {
    const int64_t i = (int64_t)blockIdx.x * CL_BLOCK + threadIdx.x;
    if (i >= st.cap) return;
    for (int k = 0; k < 3; k++) { st.rgb[k][i] = 0.0; st.cov[k][i] = 0.0; }
    st.first_exposure[i] = 1.0; st.obs_dis[i] = 0.0; st.last_obs_time[i] = 0.0; st.n_obs[i] = 0;
}

__global__ void cl_counters_init_kernel(ClCounters* cnt, int32_t n_cand, int32_t n_sel) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    cnt->n_cand = n_cand; cnt->n_sel = n_sel;
    cnt->n_hit = cnt->n_first = cnt->n_updated = cnt->pe_count = 0ull;
    cnt->dmin_key = cl_key(3e8);
    cnt->pad = 0ull;
}

// one wavefront per recent voxel (grid-stride): its vertex list has at most 128 entries
__global__ void __launch_bounds__(CL_BLOCK) cl_mark_recent_kernel(const int32_t* __restrict__ recent, const int32_t* __restrict__ n_recent, const int32_t* __restrict__ vx_npts,
                                                                  const int32_t* __restrict__ vx_pts, int vox_cap, int n_vtx, int heads, int32_t* __restrict__ flags) {
    const int lane = threadIdx.x & 63;
    const int n = *n_recent;
    for (int r = (int)((blockIdx.x * CL_BLOCK + threadIdx.x) >> 6); r < n; r += (int)((gridDim.x * CL_BLOCK) >> 6)) {
        const int vi = recent[r];
        const int np = min(vx_npts[vi], vox_cap);
        int lo = 0x7fffffff;
        for (int k = lane; k < np; k += 64) {
            const int id = vx_pts[(size_t)vi * vox_cap + k];
            if (id < 0 || id >= n_vtx) continue;
            if (heads) lo = min(lo, id);
            else flags[id] = 1;
        }
        if (heads) {
            for (int off = 32; off > 0; off >>= 1) lo = min(lo, __shfl_xor(lo, off, 64));
            if (lane == 0 && lo != 0x7fffffff) flags[lo] = 1;
        }
    }
}

__global__ void __launch_bounds__(CL_BLOCK) cl_compact_kernel(const int32_t* __restrict__ flags, const int32_t* __restrict__ off, const int32_t* __restrict__ src, int n,
                                                              int32_t* __restrict__ out, int32_t* __restrict__ n_out) {
    const int i = blockIdx.x * CL_BLOCK + threadIdx.x;
    if (n == 0 && i == 0) *n_out = 0;
    if (i >= n) return;
    const int f = flags[i];
    if (f) out[off[i]] = src ? src[i] : i;
    if (i == n - 1) *n_out = off[i] + (f ? 1 : 0);
}

__global__ void __launch_bounds__(CL_BLOCK) cl_select_min_kernel(ClCam c, const float* __restrict__ v_pos, const int32_t* __restrict__ cand, int n_bound,
                                                                 const ClCounters* __restrict__ cnt, double md, int tab_w, int64_t tab_n, int32_t* __restrict__ cell,
                                                                 double* __restrict__ depth, uint32_t* __restrict__ tab_min) {
    const int i = blockIdx.x * CL_BLOCK + threadIdx.x;
    if (i >= min(n_bound, cnt->n_cand)) return;
    const int id = cand ? cand[i] : i;
    const ClProj p = cl_project(c, v_pos, id);
    const double dep = cl_norm(p.d);
    int32_t ce = -1;
    if (!(dep > c.max_depth) && !(dep < c.min_depth) && p.ok) {
        const int cu = (int)(round(p.u / md) * md), cv = (int)(round(p.v / md) * md);
        const int64_t q = (int64_t)cv * tab_w + cu;
        if (cu >= 0 && cu < tab_w && cv >= 0 && q < tab_n) {   // (always: 1 <= u < cols and the table is md / 2 + 2 wider)
            ce = (int32_t)q;
            atomicMin(&tab_min[q], __float_as_uint((float)dep));   // positive floats order as their bits
        }
    }
    cell[i] = ce;
    depth[i] = dep;
}

__global__ void __launch_bounds__(CL_BLOCK) cl_select_rank_kernel(int n_bound, const ClCounters* __restrict__ cnt, const int32_t* __restrict__ cell,
                                                                  const double* __restrict__ depth, const uint32_t* __restrict__ tab_min, int32_t* __restrict__ tab_hi,
                                                                  uint32_t* __restrict__ tab_lo) {
    const int i = blockIdx.x * CL_BLOCK + threadIdx.x;
    if (i >= min(n_bound, cnt->n_cand)) return;
    const int32_t ce = cell[i];
    if (ce < 0) return;
    const float m = __uint_as_float(tab_min[ce]);
    const double dep = depth[i];
    if (dep < (double)m) atomicMax(&tab_hi[ce], i);
    if ((float)dep == m) atomicMin(&tab_lo[ce], (uint32_t)i);
}

__global__ void __launch_bounds__(CL_BLOCK) cl_select_keep_kernel(int n_bound, const ClCounters* __restrict__ cnt, const int32_t* __restrict__ cell,
                                                                  const int32_t* __restrict__ tab_hi, const uint32_t* __restrict__ tab_lo, int32_t* __restrict__ keep) {
    const int i = blockIdx.x * CL_BLOCK + threadIdx.x;
    if (i >= n_bound) return;
    int k = 0;
    if (i < cnt->n_cand) {
        const int32_t ce = cell[i];
        if (ce >= 0) {
            const int32_t hi = tab_hi[ce];
            k = (hi >= 0 ? hi : (int32_t)tab_lo[ce]) == i;
        }
    }
    keep[i] = k;
}

__global__ void __launch_bounds__(CL_BLOCK) cl_dmin_kernel(ClCam c, const float* __restrict__ v_pos, const int32_t* __restrict__ sel, int n_bound, ClCounters* cnt) {
    __shared__ unsigned long long s_key[CL_BLOCK / 64];
    const int i = blockIdx.x * CL_BLOCK + threadIdx.x;
    unsigned long long key = ~0ull;
    if (i < min(n_bound, cnt->n_sel)) {
        const int id = sel ? sel[i] : i;
        double d[3];
        for (int k = 0; k < 3; k++) d[k] = (double)v_pos[3 * (size_t)id + k] - c.pos[k];
        const double di = (d[0] * c.n[0] + d[1] * c.n[1]) + d[2] * c.n[2];
        if (di == di) key = cl_key(di);
    }
    for (int off = 32; off > 0; off >>= 1) { const unsigned long long o = __shfl_xor(key, off, 64); key = o < key ? o : key; }
    if ((threadIdx.x & 63) == 0) s_key[threadIdx.x >> 6] = key;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < CL_BLOCK / 64; w++) key = s_key[w] < key ? s_key[w] : key;
        // (a look first: once a few workgroups have been through, most find nothing smaller to bring -- 16 k atomics on this one address took 0.19 ms
        // of a 4 M-vertex image; a stale look only costs an atomic that changes nothing)
        if (key < __hip_atomic_load(&cnt->dmin_key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&cnt->dmin_key, key);
    }
}

__device__ __forceinline__ double cl_key_to_double(unsigned long long k) {
    const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double((long long)b);
}

__global__ void __launch_bounds__(CL_BLOCK) cl_update_kernel(ClCam c, int model, const float* __restrict__ v_pos, const int32_t* __restrict__ sel, int n_bound,
                                                             ClCounters* cnt, const uint8_t* __restrict__ img, ClState st, float* __restrict__ uv,
                                                             double* __restrict__ partials) {
    __shared__ double s_pe[CL_BLOCK];
    __shared__ int s_cnt[4];
    if (threadIdx.x < 4) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const int i = blockIdx.x * CL_BLOCK + threadIdx.x;
    double pe = 0.0;
    int hit = 0, first = 0, upd = 0, pe_n = 0;
    if (i < min(n_bound, cnt->n_sel)) {
        const int id = sel ? sel[i] : i;
        const ClProj p = cl_project(c, v_pos, id);
        uv[2 * (size_t)i] = p.front ? (float)p.u : __uint_as_float(0x7fc00000u);
        uv[2 * (size_t)i + 1] = p.front ? (float)p.v : __uint_as_float(0x7fc00000u);
        const double dot = (p.d[0] * c.n[0] + p.d[1] * c.n[1]) + p.d[2] * c.n[2];
        double col[3];
        if (model == 0) {
            const double dmin = cl_key_to_double(cnt->dmin_key);
            const bool skip = (dot - dmin > c.allow) && st.n_obs[id] > 5;
            if (!skip && p.ok) {
                cl_sample(c, img, p.u, p.v, col);
                hit = 1;
                upd = cl_update_rgb(st, id, col, dot, 1.5, c.obs_time, c.inv_exposure, &first);
            }
        } else {
            double dis = cl_norm(p.d);
            double ang = acos(dot / (dis + 0.0001)) * 57.3;
            ang = ang < 5.0 ? 5.0 : ang;
            dis = dis < 1.0 ? 1.0 : dis;
            if (!(ang > 30.0) && p.ok) {
                cl_sample(c, img, p.u, p.v, col);
                hit = 1;
                upd = cl_update_rgb(st, id, col, dis, (1.5 * dis) * ang, c.obs_time, c.inv_exposure, &first);
                if (upd) {
                    const double fe = st.first_exposure[id];
                    const double r[3] = {st.rgb[0][id], st.rgb[1][id], st.rgb[2][id]};
                    const double g[3] = {r[0] / fe, r[1] / fe, r[2] / fe};
                    double gm = g[0];
                    if (g[1] > gm) gm = g[1];
                    if (g[2] > gm) gm = g[2];
                    if (!(gm > 254.0)) {
                        const double rad[3] = {r[0] / c.inv_exposure, r[1] / c.inv_exposure, r[2] / c.inv_exposure};
                        double rm = rad[0];
                        if (rad[1] > rm) rm = rad[1];
                        if (rad[2] > rm) rm = rad[2];
                        if (!(rm > 245.0)) {
                            double err = fabs(cl_norm(col) - cl_norm(rad));
                            if (err > c.max_pe) err = c.max_pe;
                            pe = err;
                            pe_n = 1;
                        }
                    }
                }
            }
        }
    }
    {   // one LDS add per wavefront and counter: the lanes' flags counted by ballot
        const int flag[4] = {hit, first, upd, pe_n};
        for (int k = 0; k < 4; k++) {
            const int n = __popcll(__ballot(flag[k]));
            if ((threadIdx.x & 63) == 0 && n) atomicAdd(&s_cnt[k], n);
        }
    }
    s_pe[threadIdx.x] = pe;
    __syncthreads();
    for (int w = CL_BLOCK / 2; w > 0; w >>= 1) {   // fixed tree: the partial does not depend on scheduling
        if ((int)threadIdx.x < w) s_pe[threadIdx.x] += s_pe[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        partials[blockIdx.x] = s_pe[0];
        if (s_cnt[0]) atomicAdd(&cnt->n_hit, (unsigned long long)s_cnt[0]);
        if (s_cnt[1]) atomicAdd(&cnt->n_first, (unsigned long long)s_cnt[1]);
        if (s_cnt[2]) atomicAdd(&cnt->n_updated, (unsigned long long)s_cnt[2]);
        if (s_cnt[3]) atomicAdd(&cnt->pe_count, (unsigned long long)s_cnt[3]);
    }
}

struct ClStatsOut { long long n_set, n_selected, n_hit, n_first, n_updated, pe_count; double pe_sum, min_dis; };

__global__ void __launch_bounds__(CL_BLOCK) cl_finalize_kernel(int model, const ClCounters* __restrict__ cnt, const double* __restrict__ partials, int n_blocks,
                                                               ClStatsOut* __restrict__ out) {
    __shared__ double s_pe[CL_BLOCK];
    double acc = 0.0;
    for (int b = threadIdx.x; b < n_blocks; b += CL_BLOCK) acc += partials[b];
    s_pe[threadIdx.x] = acc;
    __syncthreads();
    for (int w = CL_BLOCK / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) s_pe[threadIdx.x] += s_pe[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        out->n_set = cnt->n_cand; out->n_selected = cnt->n_sel;
        out->n_hit = (long long)cnt->n_hit; out->n_first = (long long)cnt->n_first; out->n_updated = (long long)cnt->n_updated;
        out->pe_count = (long long)cnt->pe_count;
        out->pe_sum = s_pe[0];
        out->min_dis = model == 0 ? cl_key_to_double(cnt->dmin_key) : 0.0;
    }
}

struct ClStateOut { double rgb[3], cov[3], first_exposure, obs_dis, last_obs_time; int32_t n_obs, pad; };

__global__ void __launch_bounds__(CL_BLOCK) cl_gather_kernel(ClState st, const int32_t* __restrict__ ids, int64_t first, int64_t n,
                                                             uint8_t* __restrict__ out_rgb, ClStateOut* __restrict__ out_state) {
    const int64_t i = (int64_t)blockIdx.x * CL_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int64_t id = ids ? (int64_t)ids[i] : first + i;
    if (id < 0 || id >= st.cap) return;   // (validated on the host)
    const double fe = st.first_exposure[id];
    ClStateOut o;
    for (int k = 0; k < 3; k++) { o.rgb[k] = st.rgb[k][id]; o.cov[k] = st.cov[k][id]; }
    o.first_exposure = fe; o.obs_dis = st.obs_dis[id]; o.last_obs_time = st.last_obs_time[id]; o.n_obs = st.n_obs[id]; o.pad = 0;
    if (out_state) out_state[i] = o;
    if (out_rgb)
        for (int k = 0; k < 3; k++) {
            const double q = o.rgb[k] / fe;
            out_rgb[3 * i + k] = (uint8_t)(q > 255.0 ? 255 : (q > 0.0 ? (int)q : 0));
        }
}

inline unsigned cl_grid(int64_t n) { return (unsigned)((n + CL_BLOCK - 1) / CL_BLOCK); }

}  // namespace

static_assert(sizeof(ClStatsOut) == 64 && sizeof(ClStateOut) == 80, "the C ABI's immesh_colour_stats / immesh_colour_state");

void cl_launch_state_init(hipStream_t s, const ClState& st) {
    if (st.cap > 0) hipLaunchKernelGGL(cl_state_init_kernel, dim3(cl_grid(st.cap)), dim3(CL_BLOCK), 0, s, st);
}
void cl_launch_counters_init(hipStream_t s, ClCounters* cnt, int32_t n_cand, int32_t n_sel) {
    hipLaunchKernelGGL(cl_counters_init_kernel, dim3(1), dim3(64), 0, s, cnt, n_cand, n_sel);
}
void cl_launch_mark_recent(hipStream_t s, const int32_t* recent, const int32_t* n_recent, const int32_t* vx_npts, const int32_t* vx_pts, int vox_cap, int n_vtx,
                           int heads, int32_t* flags) {
    hipLaunchKernelGGL(cl_mark_recent_kernel, dim3(1024), dim3(CL_BLOCK), 0, s, recent, n_recent, vx_npts, vx_pts, vox_cap, n_vtx, heads, flags);
}
void cl_launch_compact(hipStream_t s, const int32_t* flags, const int32_t* off, const int32_t* src, int n, int32_t* out, int32_t* n_out) {
    hipLaunchKernelGGL(cl_compact_kernel, dim3(cl_grid(n > 0 ? n : 1)), dim3(CL_BLOCK), 0, s, flags, off, src, n, out, n_out);
}
void cl_launch_select_min(hipStream_t s, const ClCam& cam, const float* v_pos, const int32_t* cand, int n_bound, const ClCounters* cnt, double md, int tab_w,
                          int64_t tab_n, int32_t* cell, double* depth, uint32_t* tab_min) {
    if (n_bound > 0) hipLaunchKernelGGL(cl_select_min_kernel, dim3(cl_grid(n_bound)), dim3(CL_BLOCK), 0, s, cam, v_pos, cand, n_bound, cnt, md, tab_w, tab_n, cell, depth, tab_min);
}
void cl_launch_select_rank(hipStream_t s, int n_bound, const ClCounters* cnt, const int32_t* cell, const double* depth, const uint32_t* tab_min, int32_t* tab_hi,
                           uint32_t* tab_lo) {
    if (n_bound > 0) hipLaunchKernelGGL(cl_select_rank_kernel, dim3(cl_grid(n_bound)), dim3(CL_BLOCK), 0, s, n_bound, cnt, cell, depth, tab_min, tab_hi, tab_lo);
}
void cl_launch_select_keep(hipStream_t s, int n_bound, const ClCounters* cnt, const int32_t* cell, const int32_t* tab_hi, const uint32_t* tab_lo, int32_t* keep) {
    if (n_bound > 0) hipLaunchKernelGGL(cl_select_keep_kernel, dim3(cl_grid(n_bound)), dim3(CL_BLOCK), 0, s, n_bound, cnt, cell, tab_hi, tab_lo, keep);
}
void cl_launch_dmin(hipStream_t s, const ClCam& cam, const float* v_pos, const int32_t* sel, int n_bound, ClCounters* cnt) {
    if (n_bound > 0) hipLaunchKernelGGL(cl_dmin_kernel, dim3(cl_grid(n_bound)), dim3(CL_BLOCK), 0, s, cam, v_pos, sel, n_bound, cnt);
}
int cl_update_blocks(int n_bound) { return (int)cl_grid(n_bound); }
void cl_launch_update(hipStream_t s, const ClCam& cam, int model, const float* v_pos, const int32_t* sel, int n_bound, ClCounters* cnt, const uint8_t* img,
                      const ClState& st, float* uv, double* partials) {
    if (n_bound > 0) hipLaunchKernelGGL(cl_update_kernel, dim3(cl_grid(n_bound)), dim3(CL_BLOCK), 0, s, cam, model, v_pos, sel, n_bound, cnt, img, st, uv, partials);
}
void cl_launch_finalize(hipStream_t s, int model, const ClCounters* cnt, const double* partials, int n_blocks, void* stats) {
    hipLaunchKernelGGL(cl_finalize_kernel, dim3(1), dim3(CL_BLOCK), 0, s, model, cnt, partials, n_blocks, (ClStatsOut*)stats);
}
void cl_launch_gather(hipStream_t s, const ClState& st, const int32_t* ids, int64_t first, int64_t n, uint8_t* out_rgb, void* out_state) {
    if (n > 0) hipLaunchKernelGGL(cl_gather_kernel, dim3(cl_grid(n)), dim3(CL_BLOCK), 0, s, st, ids, first, n, out_rgb, (ClStateOut*)out_state);
}
