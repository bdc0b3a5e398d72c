/*
 * ss_unproject.hip -- map points from depth: Frame::UnprojectStereo with the selection of Tracking::StereoInitialization
 * (SS_UNPROJECT_ALL) and of Tracking::CreateNewKeyFrame / UpdateLastFrame (SS_UNPROJECT_CLOSE), the close counts of
 * Tracking::NeedNewKeyFrame (the rule: include/sendslam_orb.h; DESIGN.md "Map points from depth").  Every step is the text of
 * ss_unproject_steps.h, which the host twin compiles too.
 *
 *   k_unproject   one workgroup of SSK_UNPROJECT_CHUNK threads per frame, thread t owns rows t, t + CHUNK, ... (at the most
 *                 UNPROJECT_SLOTS of them, held in registers as the depth's bits or a sentinel that carries the state).
 *                 U-A  one pass over the rows: class, key bits and the frame's counters (ballot-free: a count per thread, one LDS
 *                      atomic per counter and thread)
 *                 U-B  only when fewer rows are processed than are ranked: the bits of the quota-th lowest key by a radix select,
 *                      four passes of eight bits over a 256-bin LDS histogram (k_stereo_cut's scheme); thread 0 walks all 256 bins
 *                      of each pass.  What is left of the rank inside the last bin is the number of rows with exactly these bits
 *                      that are still admitted, lowest row first
 *                 U-C  the rows in ascending chunks (k_tri_compact's scheme, twice per chunk): ballot and prefix sums number the
 *                      rows at the threshold bits, which settles `processed`; one lane per row then forms the map point in
 *                      double; ballot and prefix sums place the created rows, so the compact block is in row order whatever the
 *                      schedule
 *
 * Every floating-point step is a single IEEE operation (-ffp-contract=off).  Every global write is a plain vector store; the
 * counters live in LDS until thread 0 stores the summary.  No loop but the row loop has a trip count that depends on the data.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ss_constants.h"
#include "ss_kernels.h"
#include "ss_unproject_steps.h"

namespace {

constexpr int UNPROJECT_SLOTS = SS_GUIDED_MAX_ROWS / SSK_UNPROJECT_CHUNK;
constexpr int UNPROJECT_WAVES = SSK_UNPROJECT_CHUNK / 64;
constexpr uint32_t UNPROJECT_NONE = 0xFFFFFFF0u; /* NONE + state: a row without a key; the bits of a depth > 0 are <= 0x7F800000 */

static_assert(SS_GUIDED_MAX_ROWS % SSK_UNPROJECT_CHUNK == 0 && SSK_UNPROJECT_CHUNK == 1024, "k_unproject: one row per thread and chunk, 16 waves");
static_assert(sizeof(ss_keypoint) == 24 && sizeof(ss_map_point) == 32 && sizeof(ss_unproject_view) == 168 && sizeof(ss_unproject_params) == 16 &&
                  sizeof(ss_unproject_info) == 4 && sizeof(ss_unproject_summary) == 40,
              "the layouts of the header");

enum { C_DEPTH, C_RANKED, C_CLOSE, C_NOT_FAR, C_TRACKED, C_UNTRACKED, C_PROCESSED, C_CREATED, C_KEPT, C_COUNTERS };

/* the sums of a flag over the waves below this one and over the chunk; wave_n holds one popcount per wave */
__device__ __forceinline__ void chunk_prefix(const int *wave_n, int wave, int *before, int *total)
{
    int b = 0, t = 0;
#pragma unroll
    for (int k = 0; k < UNPROJECT_WAVES; k++) {
        const int n = wave_n[k];
        b += k < wave ? n : 0;
        t += n;
    }
    *before = b, *total = t;
}

/* grid (frames), SSK_UNPROJECT_CHUNK threads; rows <= SS_GUIDED_MAX_ROWS */
__global__ __launch_bounds__(SSK_UNPROJECT_CHUNK) void k_unproject(ssk_unproject_call g)
{
    __shared__ int hist[256];
    __shared__ int cnt[C_COUNTERS];
    __shared__ int wave_n[UNPROJECT_WAVES];
    __shared__ int sel_bin, sel_rank;
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x, rows = g.rows;
    const int lane = tid & 63, wave = tid >> 6;
    const int status = g.frame_error ? g.frame_error[b] : 0;
    const int n = status != 0 ? 0 : ss_unproject_clamp(g.n_kp[b], rows);
    const int n_levels = min(max(g.n_levels, 1), SS_MAX_LEVELS);
    const size_t row0 = (size_t)b * (size_t)rows;
    const ss_keypoint *kp = g.kp + row0;
    const int block = g.depth_src ? g.depth_src[b] : b; /* negative: the frame has no depth plane */
    const uint8_t *depth = g.depth + (int64_t)max(block, 0) * (int64_t)rows * g.depth_stride;
    const uint8_t *has_point = g.has_point ? g.has_point + row0 : nullptr, *outlier = g.outlier ? g.outlier + row0 : nullptr;
    const float close_limit = g.p.close_limit;
    if (tid < 256) hist[tid] = 0;
    if (tid < C_COUNTERS) cnt[tid] = 0;
    __syncthreads();

    /* U-A */
    uint32_t key[UNPROJECT_SLOTS];
    {
        int n_depth = 0, ranked = 0, close = 0, not_far = 0, tracked = 0, untracked = 0;
#pragma unroll
        for (int k = 0; k < UNPROJECT_SLOTS; k++) {
            const int i = k * SSK_UNPROJECT_CHUNK + tid;
            key[k] = UNPROJECT_NONE + SS_UNPROJECT_NO_DEPTH;
            if (i < n) {
                const float d = block >= 0 ? ss_unproject_depth_at(depth, g.depth_stride, i) : -1.0f;
                const int cls = ss_unproject_class(d, kp[i].octave, n_levels);
                n_depth += d > 0.0f;
                if (cls == 0) {
                    key[k] = ss_unproject_bits(d);
                    ranked++;
                    not_far += d <= close_limit;
                    if (d < close_limit) {
                        close++;
                        const bool t = has_point && has_point[i] != 0 && !(outlier && outlier[i] != 0);
                        tracked += t, untracked += !t;
                    }
                } else {
                    key[k] = UNPROJECT_NONE + (uint32_t)cls;
                }
            }
        }
        if (n_depth) atomicAdd(&cnt[C_DEPTH], n_depth);
        if (ranked) atomicAdd(&cnt[C_RANKED], ranked);
        if (close) atomicAdd(&cnt[C_CLOSE], close);
        if (not_far) atomicAdd(&cnt[C_NOT_FAR], not_far);
        if (tracked) atomicAdd(&cnt[C_TRACKED], tracked);
        if (untracked) atomicAdd(&cnt[C_UNTRACKED], untracked);
    }
    __syncthreads();

    /* U-B: every ranked row with bits below t_bits is processed, and the first t_quota rows with exactly t_bits */
    const int n_ranked = cnt[C_RANKED];
    const int quota = ss_unproject_quota(g.p.mode, g.p.max_points, cnt[C_NOT_FAR], n_ranked);
    uint32_t t_bits = UNPROJECT_NONE; /* above every key */
    int t_quota = 0;
    if (quota < n_ranked) { /* uniform; quota >= 1 */
        uint32_t prefix = 0;
        int rank = quota - 1;
#pragma unroll
        for (int pass = 0; pass < 4; pass++) {
            const int shift = 24 - 8 * pass;
#pragma unroll
            for (int k = 0; k < UNPROJECT_SLOTS; k++) {
                const uint32_t v = key[k];
                /* pass 0 takes every key (a shift by 32 is not formed); later a sentinel's upper bytes equal no key's prefix */
                const bool in = pass == 0 ? v < UNPROJECT_NONE : (v >> ((shift + 8) & 31)) == prefix;
                if (in) atomicAdd(&hist[(v >> shift) & 255u], 1);
            }
            __syncthreads();
            if (tid == 0) {
                int acc = 0, bin = 255, left = 0;
                bool found = false;
                for (int h = 0; h < 256; h++) {
                    const int c = hist[h];
                    if (!found && rank < acc + c) found = true, bin = h, left = rank - acc;
                    acc += c;
                }
                sel_bin = bin, sel_rank = left;
            }
            __syncthreads();
            prefix = (prefix << 8) | (uint32_t)sel_bin;
            rank = sel_rank;
            if (tid < 256) hist[tid] = 0;
            __syncthreads();
        }
        t_bits = prefix;
        t_quota = rank + 1;
    }

    /* U-C */
    const ss_unproject_view *view = g.views + b; /* one address per workgroup: read where a point is formed, not held across the chunks */
    int tie_base = 0, point_base = 0, processed_n = 0, created_n = 0, kept_n = 0;
#pragma unroll
    for (int k = 0; k < UNPROJECT_SLOTS; k++) {
        const int c0 = k * SSK_UNPROJECT_CHUNK;
        if (c0 < rows) { /* uniform */
            const int i = c0 + tid;
            const uint32_t v = key[k];
            const bool ranked = v < UNPROJECT_NONE, tie = ranked && v == t_bits;
            const unsigned long long tie_mask = __ballot(tie);
            if (lane == 0) wave_n[wave] = __popcll(tie_mask);
            __syncthreads();
            int before, total;
            chunk_prefix(wave_n, wave, &before, &total);
            const int tie_at = tie_base + before + __popcll(tie_mask & ((1ull << lane) - 1ull));
            tie_base += total;
            __syncthreads(); /* wave_n is rewritten */
            const bool processed = ranked && (v < t_bits || (tie && tie_at < t_quota));
            int state = -1;
            ss_map_point pt = {};
            if (i < n) {
                if (!ranked) state = (int)(v - UNPROJECT_NONE);
                else if (!processed) state = SS_UNPROJECT_FAR;
                else if (has_point && has_point[i] != 0) state = SS_UNPROJECT_KEPT;
                else {
                    const float2 xy = *(const float2 *)(kp + i);
                    union { uint32_t u; float f; } d;
                    d.u = v;
                    const ss_unproject_out r = ss_unproject_point(*view, g.scale, n_levels, xy.x, xy.y, kp[i].octave, d.f);
                    pt = r.point;
                    state = r.ok ? SS_UNPROJECT_CREATED : SS_UNPROJECT_DEGENERATE;
                }
            }
            if (i < rows) g.info[row0 + i].state = state;
            const bool point = state == SS_UNPROJECT_CREATED;
            processed_n += processed, created_n += point, kept_n += state == SS_UNPROJECT_KEPT;
            const unsigned long long mask = __ballot(point);
            if (lane == 0) wave_n[wave] = __popcll(mask);
            __syncthreads();
            chunk_prefix(wave_n, wave, &before, &total);
            if (point) {
                const int pos = point_base + before + __popcll(mask & ((1ull << lane) - 1ull)); /* pos <= i < rows */
                const size_t at = row0 + pos;
                float4 *po = (float4 *)(g.points + at);
                po[0] = make_float4(pt.x, pt.y, pt.z, pt.nx);
                po[1] = make_float4(pt.ny, pt.nz, pt.min_dist, pt.max_dist);
                const uint4 *di = (const uint4 *)(g.desc + (row0 + i) * SS_DESC_BYTES);
                uint4 *dn = (uint4 *)(g.point_desc + at * SS_DESC_BYTES);
                dn[0] = di[0], dn[1] = di[1];
                *(int2 *)(g.point_rows + at * 2) = make_int2(i, -1);
            }
            point_base += total;
            __syncthreads(); /* wave_n is rewritten */
        }
    }
    if (processed_n) atomicAdd(&cnt[C_PROCESSED], processed_n);
    if (created_n) atomicAdd(&cnt[C_CREATED], created_n);
    if (kept_n) atomicAdd(&cnt[C_KEPT], kept_n);
    __syncthreads();
    if (tid == 0) {
        ss_unproject_summary s;
        s.status = status;
        s.n_kp = n;
        s.n_depth = cnt[C_DEPTH];
        s.n_close = cnt[C_CLOSE];
        s.n_not_far = cnt[C_NOT_FAR];
        s.n_processed = cnt[C_PROCESSED];
        s.n_created = cnt[C_CREATED];
        s.n_kept = cnt[C_KEPT];
        s.n_tracked_close = cnt[C_TRACKED];
        s.n_untracked_close = cnt[C_UNTRACKED];
        g.n_points[b] = cnt[C_CREATED];
        g.summary[b] = s;
    }
}

} // namespace

void ssk_unproject(hipStream_t s, const ssk_unproject_call &g)
{
    if (g.n_frames <= 0 || g.rows <= 0) return;
    hipLaunchKernelGGL(k_unproject, dim3((unsigned)g.n_frames), dim3(SSK_UNPROJECT_CHUNK), 0, s, g);
}
