/*
 * ss_refresh.hip -- the map-point refresh: MapPoint::UpdateNormalAndDepth and MapPoint::ComputeDistinctiveDescriptors for every
 * selected point of the context's map (the rule: include/sendslam_orb.h; DESIGN.md "Map-point refresh").  Every step of the rule is
 * the text of ss_refresh_steps.h, which the host twin compiles too.
 *
 *   k_refresh_short    one wave per point row whose list has at most 64 records, four per workgroup, no barrier.  The observations
 *                      are compacted onto the lanes 0 .. n-1 by one cross-lane permute; lane a holds observation a: its term of the
 *                      normal (slot a of the tree, folded by the cross-lane moves of ss_gn.h) and its descriptor in eight registers.
 *                      Observation b's words are wave-uniform reads of lane b; lane a keeps its row of distances in LDS (uint16,
 *                      [b][lane]: no lane reads what another wrote, and consecutive lanes touch consecutive addresses) and finds its
 *                      median by the nine halvings of ss_refresh_select; the winner is a cross-lane minimum of the keys.
 *   k_refresh_long     one workgroup of 256 lanes per longer list.  The observations are compacted in list order into LDS (one word
 *                      each: the descriptor's row of d_desc, from which the keyframe follows); the terms of 256 observations at a
 *                      time go through LDS to wave 0, whose lane s adds slot s in ascending order; the rows of the distance matrix
 *                      are tiled over the lanes, 256 at a time, each lane counting its row against wave-uniform loads of every
 *                      descriptor in each of the nine halvings (no distance is stored); the keys meet in one LDS atomic minimum.
 *   k_refresh_summary  one workgroup per block counts the states its rows' infos hold.
 *
 * Every loop's trip count is wave-uniform; every global write is a plain vector store; there are no global atomics.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "ss_gn.h"
#include "ss_kernels.h"
#include "ss_refresh_steps.h"

namespace {

constexpr int REFRESH_THREADS = 256, REFRESH_WAVES = REFRESH_THREADS / 64;
static_assert(SS_REFRESH_SHORT == 64 && SS_REFRESH_SLOTS == 64, "a short list is one wave's: observation a is lane a and slot a");

struct refresh_args {
    const int32_t *pt_row, *long_pts;
    ss_map_point *points;
    uint8_t *point_desc;
    const int32_t *np, *ref_kf;
    const uint8_t *select, *desc;
    int rows_per_frame;
    const float *ow, *scale;
    int n_levels, lds_n; /* lds_n: the observations the long kernel's LDS holds */
    ss_refresh_info *info;
    ss_refresh_summary *summary;
};

__device__ __forceinline__ void refresh_put(ss_refresh_info *at, const ss_refresh_info &v)
{
    int32_t *o = (int32_t *)at;
    o[0] = v.state, o[1] = v.n_obs, o[2] = v.count, o[3] = v.ref_kf, o[4] = v.level, o[5] = v.best_kf, o[6] = v.best_median, o[7] = 0;
}

__device__ __forceinline__ void refresh_put_geometry(ss_map_point *at, const double sum[3], int n, double dist, const float *scale, int level, int n_levels)
{
    float *o = (float *)at, mn, mx;
    ss_refresh_depth(dist, scale, min(max(level, 0), n_levels - 1), n_levels, &mn, &mx);
    o[3] = ss_refresh_normal(sum[0], n), o[4] = ss_refresh_normal(sum[1], n), o[5] = ss_refresh_normal(sum[2], n);
    o[6] = mn, o[7] = mx;
}

/* the row's block, and whether it is refreshed; the host has checked the tables: the clamps only keep a stray value inside the arrays */
__device__ __forceinline__ bool refresh_row(const ss_covis_tab &m, const refresh_args &a, size_t gp, const ss_map_point &P, int *q)
{
    const int b = (int)(gp / (size_t)m.point_rows), i = (int)(gp - (size_t)b * m.point_rows);
    *q = m.blk_prob[b];
    if (*q < 0 || *q >= m.n_problems) return false;
    return ss_refresh_selected(i, a.np[b], m.point_rows, a.select ? (int)a.select[gp] : 0, P.x, P.y, P.z);
}

template <bool GEO, bool DESC> __global__ __launch_bounds__(REFRESH_THREADS) void k_refresh_short(ss_covis_tab m, refresh_args a)
{
    __shared__ uint16_t dist_lds[DESC ? REFRESH_WAVES * 64 * 64 : 1];
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const size_t NP = (size_t)m.n_blocks * m.point_rows, gp = (size_t)blockIdx.x * REFRESH_WAVES + wave;
    if (gp >= NP) return;
    const int cnt = m.pt_cnt[gp];
    if (cnt > SS_REFRESH_SHORT) return; /* k_refresh_long's */
    const ss_map_point P = a.points[gp];
    int q;
    if (!refresh_row(m, a, gp, P, &q)) {
        if (lane == 0) refresh_put(a.info + gp, ss_refresh_info_none(-1, 0, 0));
        return;
    }
    const int first_kf = m.prob[q].first_kf, off = m.pt_off[gp];
    /* the observations onto the lanes 0 .. n-1, in list order; the other records behind them */
    const uint32_t rec_e = lane < cnt ? m.pt_item[off + lane] : 0u;
    const bool valid = ss_covis_valid(rec_e);
    const unsigned long long vm = __ballot(valid);
    const int n = __popcll(vm), below = __popcll(vm & ((1ull << lane) - 1ull));
    const int dst = valid ? below : n + (lane - below);
    const uint32_t rec = (uint32_t)__builtin_amdgcn_ds_permute(dst * 4, (int)rec_e);
    int row = 0;
    if (DESC) row = __builtin_amdgcn_ds_permute(dst * 4, lane < cnt ? a.pt_row[off + lane] : 0);
    const int count = __shfl(gn_wave_fold(valid ? 1 + ss_covis_stereo(rec_e) : 0), 0);
    if (n == 0) {
        if (lane == 0) refresh_put(a.info + gp, ss_refresh_info_none(1, 0, 0));
        return;
    }
    const bool act = lane < n;
    const int kf = ss_covis_kf(rec), oct = ss_covis_octave(rec);
    const int kfc = min(max(first_kf + kf, 0), m.n_kf - 1);
    ss_refresh_info out = ss_refresh_info_none(0, n, count);
    double sum[3] = {0.0, 0.0, 0.0}, dist = 0.0;
    if (GEO) {
        double t[3], len;
        const bool ok = ss_refresh_term(P.x, P.y, P.z, a.ow + 3 * (size_t)kfc, t, &len);
        const bool bad = __ballot(act && !ok) != 0ull;
#pragma unroll
        for (int c = 0; c < 3; c++) sum[c] = gn_wave_fold(act ? 0.0 + t[c] : 0.0);
        const unsigned long long rm = __ballot(act && ss_refresh_is_ref(rec, a.ref_kf ? a.ref_kf[gp] : -1));
        const int ref_a = rm ? __ffsll((long long)rm) - 1 : 0;
        out.ref_kf = __shfl(kf, ref_a), out.level = __shfl(oct, ref_a), dist = __shfl(len, ref_a);
        if (bad) {
            if (lane == 0) refresh_put(a.info + gp, ss_refresh_info_none(2, n, count));
            return;
        }
    }
    if (DESC) {
        const int rr = min(max(row, 0), a.rows_per_frame - 1);
        const uint4 *dp = (const uint4 *)(a.desc + ((size_t)kfc * a.rows_per_frame + rr) * 32);
        const uint4 w0 = dp[0], w1 = dp[1];
        const uint32_t w[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
        uint16_t *D = dist_lds + wave * 64 * 64 + lane;
        const int nu = __builtin_amdgcn_readfirstlane(n);
        for (int o = 0; o < nu; o++) {
            uint32_t wb[8];
#pragma unroll
            for (int k = 0; k < 8; k++) wb[k] = (uint32_t)__shfl((int)w[k], o);
            D[o * 64] = (uint16_t)ss_refresh_dist(w, wb);
        }
        const int med = ss_refresh_select(ss_refresh_rank(n) + 1, [&](int v) {
            int c = 0;
            for (int o = 0; o < nu; o++) c += (int)D[o * 64] <= v ? 1 : 0;
            return c;
        });
        uint32_t key = act ? ss_refresh_key(med, lane) : 0xffffffffu;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) key = min(key, (uint32_t)__shfl_xor((int)key, d));
        const int win = ss_refresh_key_obs(key);
        out.best_kf = __shfl(kf, win), out.best_median = ss_refresh_key_median(key);
        if (lane == win) {
            uint4 *o = (uint4 *)(a.point_desc + gp * 32);
            o[0] = w0, o[1] = w1;
        }
    }
    if (lane == 0) {
        if (GEO) refresh_put_geometry(a.points + gp, sum, n, dist, a.scale, out.level, a.n_levels);
        refresh_put(a.info + gp, out);
    }
}

/* the head of the long kernel's dynamic LDS: the terms of a chunk and the reference's distance (doubles), then these words, then the
 * observations */
enum { L_COUNT, L_REF_A, L_REF_OCT, L_OCT0, L_BAD, L_BEST, L_WAVE = 8, L_INTS = 16 };
constexpr int LONG_DOUBLES = REFRESH_THREADS * 3 + 1;
constexpr size_t LONG_HEAD = (size_t)LONG_DOUBLES * sizeof(double) + 8 + (size_t)L_INTS * sizeof(uint32_t);
static_assert(LONG_HEAD % 16 == 0, "the observations start on a 16-byte boundary");
constexpr size_t LONG_MAX_LDS = LONG_HEAD + (size_t)SS_GBA_MAX_KF * sizeof(uint32_t);

extern __shared__ __attribute__((aligned(16))) uint8_t refresh_lds[];

template <bool GEO, bool DESC> __global__ __launch_bounds__(REFRESH_THREADS) void k_refresh_long(ss_covis_tab m, refresh_args a)
{
    double *term = (double *)refresh_lds;
    uint32_t *hdr = (uint32_t *)(refresh_lds + (size_t)LONG_DOUBLES * sizeof(double) + 8), *ent = (uint32_t *)(refresh_lds + LONG_HEAD);
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t NP = (size_t)m.n_blocks * m.point_rows;
    const size_t gp = min((size_t)max(a.long_pts[blockIdx.x], 0), NP - 1);
    const ss_map_point P = a.points[gp];
    int q;
    if (!refresh_row(m, a, gp, P, &q)) {
        if (tid == 0) refresh_put(a.info + gp, ss_refresh_info_none(-1, 0, 0));
        return;
    }
    const int first_kf = m.prob[q].first_kf, off = m.pt_off[gp], cnt = min(max(m.pt_cnt[gp], 0), a.lds_n);
    const uint32_t per_kf = DESC ? (uint32_t)a.rows_per_frame : 1u; /* an observation's word: (first_kf + kf) * per_kf + row */
    if (tid < L_INTS) hdr[tid] = (tid == L_REF_A || tid == L_BEST) ? 0xffffffffu : 0u;
    __syncthreads();

    /* the observations in list order, 256 records at a time; the waves' counts of a chunk take two sets in turn */
    const int r = (GEO && a.ref_kf) ? a.ref_kf[gp] : -1;
    int total = 0, chunk = 0, count = 0;
    for (int base = 0; base < cnt; base += REFRESH_THREADS, chunk ^= 1) {
        const int e = base + tid;
        const uint32_t rec = e < cnt ? m.pt_item[off + e] : 0u;
        const bool valid = ss_covis_valid(rec);
        const unsigned long long vote = __ballot(valid);
        if (lane == 0) hdr[L_WAVE + 4 * chunk + wave] = (uint32_t)__popcll(vote);
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int v = 0; v < REFRESH_WAVES; v++) {
            const int x = (int)hdr[L_WAVE + 4 * chunk + v];
            before += v < wave ? x : 0, all += x;
        }
        if (valid) {
            const int pos = total + before + __popcll(vote & ((1ull << lane) - 1ull));
            const uint32_t kfc = (uint32_t)min(max(first_kf + ss_covis_kf(rec), 0), m.n_kf - 1);
            ent[pos] = kfc * per_kf + (DESC ? (uint32_t)min(max(a.pt_row[off + e], 0), a.rows_per_frame - 1) : 0u);
            count += 1 + ss_covis_stereo(rec);
            if (GEO && ss_refresh_is_ref(rec, r)) hdr[L_REF_A] = (uint32_t)pos, hdr[L_REF_OCT] = (uint32_t)ss_covis_octave(rec);
            if (pos == 0) hdr[L_OCT0] = (uint32_t)ss_covis_octave(rec);
        }
        total += all;
    }
    count = gn_wave_fold(count);
    if (lane == 0 && count) atomicAdd(&hdr[L_COUNT], (uint32_t)count);
    __syncthreads();
    const int n = __builtin_amdgcn_readfirstlane(total);
    count = (int)hdr[L_COUNT];
    if (n == 0) {
        if (tid == 0) refresh_put(a.info + gp, ss_refresh_info_none(1, 0, 0));
        return;
    }
    ss_refresh_info out = ss_refresh_info_none(0, n, count);
    double sum[3] = {0.0, 0.0, 0.0};
    if (GEO) {
        const bool given = hdr[L_REF_A] != 0xffffffffu;
        const int ref_a = given ? (int)hdr[L_REF_A] : 0;
        out.level = (int)(given ? hdr[L_REF_OCT] : hdr[L_OCT0]);
        out.ref_kf = (int)(ent[ref_a] / per_kf) - first_kf;
        for (int base = 0; base < n; base += REFRESH_THREADS) {
            const int o = base + tid;
            if (o < n) {
                double t[3], len;
                if (!ss_refresh_term(P.x, P.y, P.z, a.ow + 3 * (size_t)(ent[o] / per_kf), t, &len)) hdr[L_BAD] = 1u;
                term[3 * tid] = t[0], term[3 * tid + 1] = t[1], term[3 * tid + 2] = t[2];
                if (o == ref_a) term[LONG_DOUBLES - 1] = len;
            }
            __syncthreads();
            if (wave == 0) {
#pragma unroll
                for (int j = 0; j < REFRESH_WAVES; j++) {
                    const int s = 64 * j + lane;
                    if (base + s < n) sum[0] = sum[0] + term[3 * s], sum[1] = sum[1] + term[3 * s + 1], sum[2] = sum[2] + term[3 * s + 2];
                }
            }
            __syncthreads();
        }
#pragma unroll
        for (int c = 0; c < 3; c++) sum[c] = gn_wave_fold(sum[c]);
        if (hdr[L_BAD] != 0u) {
            if (tid == 0) refresh_put(a.info + gp, ss_refresh_info_none(2, n, count));
            return;
        }
    }
    if (DESC) {
        uint32_t best = 0xffffffffu;
        const int need = ss_refresh_rank(n) + 1;
        for (int base = 0; base < n; base += REFRESH_THREADS) {
            const int o = base + tid;
            const uint4 *dp = (const uint4 *)(a.desc + (size_t)ent[o < n ? o : 0] * 32);
            const uint4 w0 = dp[0], w1 = dp[1];
            const uint32_t w[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
            const int med = ss_refresh_select(need, [&](int v) {
                int c = 0;
                for (int b = 0; b < n; b++) {
                    const uint32_t *pb = (const uint32_t *)(a.desc + (size_t)__builtin_amdgcn_readfirstlane(ent[b]) * 32);
                    c += ss_refresh_dist(w, pb) <= v ? 1 : 0;
                }
                return c;
            });
            if (o < n) best = min(best, ss_refresh_key(med, o));
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) best = min(best, (uint32_t)__shfl_xor((int)best, d));
        if (lane == 0) atomicMin(&hdr[L_BEST], best);
        __syncthreads();
        const uint32_t key = hdr[L_BEST];
        const uint32_t win = ent[min(ss_refresh_key_obs(key), n - 1)];
        out.best_kf = (int)(win / per_kf) - first_kf, out.best_median = ss_refresh_key_median(key);
        if (tid < 8) ((uint32_t *)(a.point_desc + gp * 32))[tid] = ((const uint32_t *)(a.desc + (size_t)win * 32))[tid];
    }
    if (tid == 0) {
        if (GEO) refresh_put_geometry(a.points + gp, sum, n, term[LONG_DOUBLES - 1], a.scale, out.level, a.n_levels);
        refresh_put(a.info + gp, out);
    }
}

__global__ __launch_bounds__(REFRESH_THREADS) void k_refresh_summary(ss_covis_tab m, refresh_args a)
{
    __shared__ int s[5];
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63;
    if (tid < 5) s[tid] = 0;
    __syncthreads();
    int sel = 0, st0 = 0, st1 = 0, st2 = 0, mx = 0;
    for (int i = tid; i < m.point_rows; i += REFRESH_THREADS) {
        const int32_t *r = (const int32_t *)(a.info + (size_t)b * m.point_rows + i);
        const int state = r[0];
        if (state < 0) continue;
        sel++, st0 += state == 0, st1 += state == 1, st2 += state == 2, mx = max(mx, r[1]);
    }
    sel = gn_wave_fold(sel), st0 = gn_wave_fold(st0), st1 = gn_wave_fold(st1), st2 = gn_wave_fold(st2);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) mx = max(mx, __shfl_xor(mx, d));
    if (lane == 0) atomicAdd(&s[0], sel), atomicAdd(&s[1], st0), atomicAdd(&s[2], st1), atomicAdd(&s[3], st2), atomicMax(&s[4], mx);
    __syncthreads();
    if (tid == 0) {
        const int q = m.blk_prob[b];
        int32_t *o = (int32_t *)(a.summary + b);
        o[0] = SS_OK, o[1] = (q >= 0 && q < m.n_problems) ? ss_covis_clamp_rows(a.np[b], m.point_rows) : 0;
        o[2] = s[0], o[3] = s[1], o[4] = s[2], o[5] = s[3], o[6] = s[4], o[7] = 0;
    }
}

template <bool GEO, bool DESC> int refresh_launch(hipStream_t s, const ss_covis_tab &m, const refresh_args &a, int n_long)
{
    const size_t NP = (size_t)m.n_blocks * m.point_rows;
    hipLaunchKernelGGL((k_refresh_short<GEO, DESC>), dim3((unsigned)((NP + REFRESH_WAVES - 1) / REFRESH_WAVES)), dim3(REFRESH_THREADS), 0, s, m, a);
    if (n_long > 0) {
        auto kernel = k_refresh_long<GEO, DESC>;
        const size_t lds = LONG_HEAD + (size_t)a.lds_n * sizeof(uint32_t);
        if (lds > 48 * 1024) {
            /* only a list of more than some 10 000 records is above the default limit: the attribute is set to the largest once per
             * device and instantiation, not on every launch */
            static std::atomic<uint64_t> granted{0};
            int device = 0;
            (void)hipGetDevice(&device);
            const uint64_t bit = 1ull << (device & 63);
            if (device > 63 || !(granted.load(std::memory_order_relaxed) & bit)) {
                const hipError_t e = hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LONG_MAX_LDS);
                if (e != hipSuccess) return (int)e;
                granted.fetch_or(bit, std::memory_order_relaxed);
            }
        }
        hipLaunchKernelGGL(kernel, dim3((unsigned)n_long), dim3(REFRESH_THREADS), lds, s, m, a);
    }
    hipLaunchKernelGGL(k_refresh_summary, dim3((unsigned)m.n_blocks), dim3(REFRESH_THREADS), 0, s, m, a);
    return (int)hipSuccess;
}

} // namespace

int ssk_refresh(hipStream_t s, const ssk_refresh_call &g)
{
    refresh_args a;
    a.pt_row = g.pt_row, a.long_pts = g.long_pts;
    a.points = g.points, a.point_desc = g.point_desc, a.np = g.np, a.ref_kf = g.ref_kf, a.select = g.select, a.desc = g.desc;
    a.rows_per_frame = g.rows_per_frame, a.ow = g.ow, a.scale = g.scale, a.n_levels = g.n_levels;
    a.lds_n = (std::min(std::max(g.max_cnt, 1), SS_GBA_MAX_KF) + 3) & ~3;
    a.info = g.info, a.summary = g.summary;
    if (g.geometry && g.descriptor) return refresh_launch<true, true>(s, *g.tab, a, g.n_long);
    if (g.geometry) return refresh_launch<true, false>(s, *g.tab, a, g.n_long);
    return refresh_launch<false, true>(s, *g.tab, a, g.n_long);
}
