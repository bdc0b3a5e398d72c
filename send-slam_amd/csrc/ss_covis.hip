/*
 * ss_covis.hip -- covisibility: the neighbour list of a keyframe (KeyFrame::UpdateConnections) or of a tracked frame
 * (Tracking::UpdateLocalKeyFrames) and the redundancy counts of LocalMapping::KeyFrameCulling, from the map's two incidence lists (the
 * rule: include/sendslam_orb.h; DESIGN.md "Covisibility").  Every step of the rule is the text of ss_covis_steps.h, which the host
 * twin compiles too.
 *
 *   k_covis_row   one workgroup per row.  The weight counters of the row's problem live in dynamic LDS.  SS_COVIS_LANES lanes share
 *                 one item of the row (a record of the keyframe's list; SS_COVIS_FRAME_LANES a row of the frame's idx): they walk the item's point
 *                 list, vote with LDS integer atomics (integer addition is order-free: the result does not depend on the schedule)
 *                 and evaluate the item's culling terms in the same visit.  Then the counters of the touched range are compacted,
 *                 in place and in ascending kf, into 32-bit keys (weight << 14 | 16383 - kf), 256 at a time behind a barrier; the
 *                 keys are sorted descending by a bitonic network padded to the next power of two of their count; the first cap
 *                 leave.
 *
 * Every global write is a plain vector store; there are no global atomics and no grid-wide barrier.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "ss_covis_steps.h"
#include "ss_kernels.h"

#ifndef SS_COVIS_LANES
#define SS_COVIS_LANES 8 /* lanes per item of a keyframe row: 1, 4, 8 or 64 (DESIGN.md section 31 holds the table it was chosen on) */
#endif
#ifndef SS_COVIS_FRAME_LANES
#define SS_COVIS_FRAME_LANES 1 /* ... of a frame row, whose items are the rows of idx, most of them no hit */
#endif
#ifndef SS_COVIS_RANGE
#define SS_COVIS_RANGE 1 /* scan only the kf range the votes touched */
#endif

namespace {

static_assert(sizeof(ss_covis_row) == 32 && sizeof(ss_covis_params) == 32 && sizeof(ss_covis_prob) == 16, "the layouts of the header");

constexpr int COVIS_THREADS = 256;
/* the head of the dynamic LDS, ahead of the counters: sums, the touched range, the waves' counts of a chunk (two sets, in turn) */
enum { H_MPS, H_RED, H_LO, H_HI, H_SHARED, H_BEST, H_WAVE = 8, H_INTS = 16 };

struct covis_args {
    int n_rows, cap, lds_n; /* lds_n: the counters the workgroup has, a power of two */
    const int32_t *rows, *src, *idx, *np;
    ss_covis_params p;
    int32_t *nb;
    ss_covis_row *row;
};

constexpr size_t COVIS_MAX_LDS = (size_t)(H_INTS + SS_GBA_MAX_KF) * sizeof(uint32_t);

extern __shared__ __attribute__((aligned(16))) uint32_t covis_lds[];

template <int G, bool RANGE, bool FRAMES> __global__ __launch_bounds__(COVIS_THREADS) void k_covis_row(ss_covis_tab m, covis_args a)
{
    const int r = (int)blockIdx.x, tid = (int)threadIdx.x;
    uint32_t *hdr = covis_lds, *cnt = covis_lds + H_INTS;
    /* the host has checked the row and the tables: the clamps only keep a stray value inside the arrays */
    int kf = 0, block = 0, q;
    if (FRAMES) {
        block = min(max(a.src[r], 0), m.n_blocks - 1);
        q = m.blk_prob[block];
    } else {
        kf = min(max(a.rows ? a.rows[r] : r, 0), m.n_kf - 1);
        q = m.kf_prob[kf];
    }
    const bool owned = q >= 0 && q < m.n_problems;
    const int n_kf = owned ? min(max(m.prob[q].n_kf, 1), a.lds_n) : 0;
    const int self = (FRAMES || !owned) ? -1 : kf - m.prob[q].first_kf;
    for (int j = tid; j < n_kf; j += COVIS_THREADS) cnt[j] = 0u;
    if (tid < H_INTS) hdr[tid] = tid == H_LO ? 0xffffffffu : 0u;
    __syncthreads();

    /* the walk: group g of G lanes takes the items g, g + groups, ... */
    const int lane_in = tid % G, group = tid / G, groups = COVIS_THREADS / G;
    const int n_items = !owned ? 0 : (FRAMES ? ss_covis_clamp_rows(a.np[block], m.point_rows) : max(m.kf_cnt[kf], 0));
    int n_mps = 0, n_red = 0;
    uint32_t lo = 0xffffffffu, hi = 0u;
    for (int t = group; t < n_items; t += groups) {
        size_t gp;
        int place = 0;
        bool live = true;
        if (FRAMES) {
            gp = (size_t)block * m.point_rows + t;
            live = a.idx[(size_t)r * m.point_rows + t] >= 0;
        } else {
            const int32_t *item = m.kf_item + 2 * ((size_t)m.kf_off[kf] + t);
            gp = (size_t)item[0], place = item[1];
        }
        const int off = m.pt_off[gp], len = m.pt_cnt[gp];
        uint32_t own = 0u;
        if (!FRAMES) {
            own = m.pt_item[off + place];
            live = ss_covis_valid(own);
        }
        int count = 0, near = 0;
        if (live)
            for (int e = lane_in; e < len; e += G) {
                const int j = ss_covis_visit(m.pt_item[off + e], self, ss_covis_octave(own), a.p.cull_slack, &count, &near);
                if (j >= 0) {
                    const uint32_t jj = (uint32_t)min(j, n_kf - 1);
                    atomicAdd(&cnt[jj], 1u);
                    lo = min(lo, jj), hi = max(hi, jj);
                }
            }
        if (!FRAMES) {
#pragma unroll
            for (int d = 1; d < G; d <<= 1) count += __shfl_xor(count, d, G), near += __shfl_xor(near, d, G);
            if (live && lane_in == 0) ss_covis_close(own, count, near, a.p.cull_obs, &n_mps, &n_red);
        }
    }
    if (n_mps) atomicAdd(&hdr[H_MPS], (uint32_t)n_mps);
    if (n_red) atomicAdd(&hdr[H_RED], (uint32_t)n_red);
    if (lo <= hi) atomicMin(&hdr[H_LO], lo), atomicMax(&hdr[H_HI], hi);
    __syncthreads();

    /* the summary and the listed counters as keys, in ascending kf, written over the counters: a chunk's keys land at or below
     * the chunk's own counters, which every lane has read before the barrier */
    int s0 = 0, s1 = n_kf;
    if (RANGE) {
        const uint32_t l = hdr[H_LO], h = hdr[H_HI];
        s0 = l <= h ? (int)l : 0, s1 = l <= h ? (int)h + 1 : 0;
    }
    const int lane = tid & 63, wave = tid >> 6;
    int total = 0, n_shared = 0, chunk = 0;
    uint32_t best = 0u;
    for (int base = s0; base < s1; base += COVIS_THREADS, chunk ^= 1) {
        const int j = base + tid;
        const int w = j < s1 ? (int)cnt[j] : 0;
        if (w > 0) n_shared++, best = max(best, ss_covis_key(w, j));
        const bool listed = w >= a.p.min_weight;
        const unsigned long long vote = __ballot(listed);
        if (lane == 0) hdr[H_WAVE + 4 * chunk + wave] = (uint32_t)__popcll(vote);
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int v = 0; v < 4; v++) {
            const int x = (int)hdr[H_WAVE + 4 * chunk + v];
            before += v < wave ? x : 0, all += x;
        }
        if (listed) cnt[total + before + __popcll(vote & ((1ull << lane) - 1ull))] = ss_covis_key(w, j);
        total += all;
    }
    if (n_shared) atomicAdd(&hdr[H_SHARED], (uint32_t)n_shared);
    if (best) atomicMax(&hdr[H_BEST], best);
    __syncthreads();
    best = hdr[H_BEST];
    int n_listed = total;
    if (n_listed == 0 && a.p.fallback != 0 && best != 0u) {
        if (tid == 0) cnt[0] = best;
        n_listed = 1;
    }

    /* sort descending: a bitonic network over the next power of two, the padding below every key (a key's weight is >= 1) */
    int N = 1;
    while (N < n_listed) N <<= 1;
    N = min(N, a.lds_n);
    for (int j = n_listed + tid; j < N; j += COVIS_THREADS) cnt[j] = 0u;
    __syncthreads();
    for (int k = 2; k <= N; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < N / 2; t += COVIS_THREADS) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
                const uint32_t x = cnt[i], y = cnt[l];
                const bool down = (i & k) == 0;
                if ((x < y) == down) cnt[i] = y, cnt[l] = x;
            }
            __syncthreads();
        }

    const int n_written = min(n_listed, a.cap);
    int32_t *nb = a.nb + (size_t)r * a.cap * 2;
    for (int e = tid; e < a.cap; e += COVIS_THREADS) {
        const uint32_t key = e < n_written ? cnt[e] : 0u;
        nb[2 * e] = e < n_written ? ss_covis_key_kf(key) : -1;
        nb[2 * e + 1] = e < n_written ? ss_covis_key_weight(key) : 0;
    }
    if (tid == 0) {
        const int mps = (int)hdr[H_MPS], red = (int)hdr[H_RED];
        int32_t *o = (int32_t *)(a.row + r);
        o[0] = (int)hdr[H_SHARED];
        o[1] = best ? ss_covis_key_weight(best) : 0;
        o[2] = best ? ss_covis_key_kf(best) : -1;
        o[3] = n_listed, o[4] = n_written;
        o[5] = mps, o[6] = red, o[7] = ss_covis_redundant(red, mps, a.p.redundant_th);
    }
}

template <bool FRAMES> int covis_launch(hipStream_t s, const ssk_covis_call &g)
{
    covis_args a;
    a.n_rows = g.n_rows, a.cap = g.cap;
    a.rows = g.rows, a.src = g.src, a.idx = g.idx, a.np = g.np;
    a.p = g.p, a.nb = g.nb, a.row = g.row;
    a.lds_n = 1;
    while (a.lds_n < g.tab->max_kf) a.lds_n <<= 1;
    const size_t lds = (size_t)(H_INTS + a.lds_n) * sizeof(uint32_t); /* 64 KiB + 64 bytes at 16 384 keyframes: two workgroups per CU */
    auto kernel = k_covis_row<FRAMES ? SS_COVIS_FRAME_LANES : SS_COVIS_LANES, SS_COVIS_RANGE != 0, FRAMES>;
    if (lds > 48 * 1024) {
        /* only the largest counter array (16 384 keyframes) is above the default limit: the attribute is set to it once per device
         * and instantiation, not on every launch */
        static std::atomic<uint64_t> granted{0};
        int device = 0;
        (void)hipGetDevice(&device);
        const uint64_t bit = 1ull << (device & 63);
        if (device > 63 || !(granted.load(std::memory_order_relaxed) & bit)) {
            const hipError_t e = hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)COVIS_MAX_LDS);
            if (e != hipSuccess) return (int)e;
            granted.fetch_or(bit, std::memory_order_relaxed);
        }
    }
    hipLaunchKernelGGL(kernel, dim3((unsigned)g.n_rows), dim3(COVIS_THREADS), lds, s, *g.tab, a);
    return (int)hipSuccess;
}

} // namespace

int ssk_covis_kf(hipStream_t s, const ssk_covis_call &g) { return covis_launch<false>(s, g); }
int ssk_covis_frames(hipStream_t s, const ssk_covis_call &g) { return covis_launch<true>(s, g); }
