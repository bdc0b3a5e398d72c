/*
 * ss_place.hip -- place recognition: KeyFrameDatabase's inverted file and DetectLoopCandidates / DetectNBestCandidates /
 * DetectRelocalizationCandidates for every query of a call (the rule: include/sendslam_orb.h).  Every step of
 * the rule is the text of ss_place_steps.h and ss_bow_merge.h, which the host twin compiles too.
 *
 * The database (ssk_place_build):
 *   k_place_count    a thread per entry of the stored vectors: integer atomics count every word in range
 *   k_place_scan_*   an exclusive scan over n_words + 1 counts: 2048 per workgroup, the workgroups' sums by one workgroup, the sums
 *                    added back; the last pass also copies each start into the word's cursor
 *   k_place_fill     a thread per entry again: its place is the word's cursor, taken with an integer atomic.  The order inside a
 *                    list therefore changes from run to run; every reader of a list counts, so no result does
 * The queries (ssk_place_query), all of a call in each launch:
 *   k_place_init     a thread per (query, row): the exclusion flags, words = 0, score = -1, no acc*
 *   k_place_connect  a thread per entry of the query's covisibility row: the flags of a connected row, written whole (every store to
 *                    one address writes the same byte)
 *   k_place_vote     a wave per query word walks the word's list, SPLIT workgroups share a list (grid.z), and adds into words[q][r]
 *                    with an integer atomic; excluded rows are passed over
 *   k_place_reduce   a workgroup per query: n_sharing and max_common, then the survivors compacted in ascending row order, 1024 rows
 *                    at a time: ballots and the waves' counts behind a barrier, no atomics, so the order is fixed
 *   k_place_score    a wave per survivor, and per connected row in mode 1: ss_bow_score_wave, rounded to float once
 *   k_place_floor    a thread per query: the minimum score, in list order
 *   k_place_seeds    a lane per survivor: a seed walks its at most nb_cap neighbours and folds acc into acc*[best] as a key of the
 *                    IEEE total order with an integer atomic maximum (ss_place_key says why -0.0 and NaN are safe there)
 *   k_place_final    a workgroup per query: best_acc, the cut or the class counts, then one pass over the survivors per written
 *                    candidate, each picking the largest order key below the last one: the candidate order without a sort
 * The grids of the per-survivor kernels are sized by n_db, the bound the host knows, and stride over the device's count.
 *
 * Every global write is a plain vector store or a vector atomic.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ss_kernels.h"
#include "ss_place_steps.h"

namespace {

static_assert(sizeof(ss_place_params) == 32 && sizeof(ss_place_cand) == 24 && sizeof(ss_place_summary) == 48, "the layouts of the header");

constexpr int PL_SCAN_T = 256, PL_SCAN_PER = 8, PL_SCAN_BLOCK = PL_SCAN_T * PL_SCAN_PER; /* counts of one workgroup of the scan */
constexpr int PL_SUMS_T = 1024;
constexpr int PL_REDUCE_T = 1024; /* 16 waves: their counts of a chunk are one LDS line */
constexpr int PL_FINAL_T = 256;

__device__ __forceinline__ int pl_entry_word(const ssk_place_lists &b, size_t e, int *row)
{
    const int r = (int)(e / (size_t)b.stride), j = (int)(e % (size_t)b.stride);
    *row = r;
    if (j >= ss_place_clamp(b.count[r], b.stride)) return -1;
    const int32_t w = b.word[e];
    return ss_place_word_ok(w, b.n_words) ? w : -1;
}

__global__ __launch_bounds__(256) void k_place_count(ssk_place_lists b)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)b.n_db * b.stride) return;
    int r;
    const int w = pl_entry_word(b, e, &r);
    if (w >= 0) atomicAdd(&b.off[w], 1);
}

/* off[0 .. m) -> the exclusive scan inside each run of PL_SCAN_BLOCK, the run's total into sums */
__global__ __launch_bounds__(PL_SCAN_T) void k_place_scan_block(int32_t *off, int m, int32_t *sums)
{
    __shared__ int32_t part[PL_SCAN_T];
    const int tid = (int)threadIdx.x;
    const size_t base = (size_t)blockIdx.x * PL_SCAN_BLOCK + (size_t)tid * PL_SCAN_PER;
    int32_t v[PL_SCAN_PER], own = 0;
#pragma unroll
    for (int k = 0; k < PL_SCAN_PER; k++) {
        v[k] = base + k < (size_t)m ? off[base + k] : 0;
        own += v[k];
    }
    part[tid] = own;
    __syncthreads();
    for (int d = 1; d < PL_SCAN_T; d <<= 1) {
        const int32_t x = tid >= d ? part[tid - d] : 0;
        __syncthreads();
        part[tid] += x;
        __syncthreads();
    }
    int32_t run = part[tid] - own;
#pragma unroll
    for (int k = 0; k < PL_SCAN_PER; k++) {
        if (base + k < (size_t)m) off[base + k] = run;
        run += v[k];
    }
    if (tid == PL_SCAN_T - 1) sums[blockIdx.x] = part[tid];
}

/* sums[0 .. n) -> their exclusive scan; one workgroup, each thread a run of `per` */
__global__ __launch_bounds__(PL_SUMS_T) void k_place_scan_sums(int32_t *sums, int n)
{
    __shared__ int32_t part[PL_SUMS_T];
    const int tid = (int)threadIdx.x, per = (n + PL_SUMS_T - 1) / PL_SUMS_T;
    const int p0 = min(tid * per, n), p1 = min(p0 + per, n);
    int32_t own = 0;
    for (int p = p0; p < p1; p++) own += sums[p];
    part[tid] = own;
    __syncthreads();
    for (int d = 1; d < PL_SUMS_T; d <<= 1) {
        const int32_t x = tid >= d ? part[tid - d] : 0;
        __syncthreads();
        part[tid] += x;
        __syncthreads();
    }
    int32_t run = part[tid] - own;
    for (int p = p0; p < p1; p++) {
        const int32_t c = sums[p];
        sums[p] = run;
        run += c;
    }
}

__global__ __launch_bounds__(256) void k_place_scan_add(int32_t *off, int m, const int32_t *sums, int32_t *cursor)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)m) return;
    const int32_t v = off[i] + sums[i / PL_SCAN_BLOCK];
    off[i] = v;
    cursor[i] = v;
}

__global__ __launch_bounds__(256) void k_place_fill(ssk_place_lists b)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x, total = (size_t)b.n_db * b.stride;
    if (e >= total) return;
    int r;
    const int w = pl_entry_word(b, e, &r);
    if (w < 0) return;
    const int32_t at = atomicAdd(&b.cursor[w], 1);
    if (at >= 0 && (size_t)at < total) b.list[at] = r; /* the counts and the fill read the same arrays: only a caller who rewrites them in flight gets here */
}

/* ---- the queries ---- */
__device__ __forceinline__ int pl_conn_count(const ssk_place_call &c, int q)
{
    return c.q_nb ? ss_place_clamp(c.q_row[q].n_written, c.q_cap) : 0;
}

__global__ __launch_bounds__(256) void k_place_init(ssk_place_call c)
{
    const int q = (int)blockIdx.y, r = (int)(blockIdx.x * 256 + threadIdx.x);
    if (r == 0) {
        int32_t *st = c.state + 8 * (size_t)q;
#pragma unroll
        for (int k = 0; k < 8; k++) st[k] = 0;
    }
    if (r >= c.db.n_db) return;
    const size_t o = (size_t)q * c.db.n_db + r;
    c.flags[o] = (uint8_t)ss_place_base_flags(c.db, r, c.q_kf[q]);
    c.words[o] = 0;
    c.score[o] = -1.0f;
    c.star[o] = 0u;
}

__global__ __launch_bounds__(256) void k_place_connect(ssk_place_call c)
{
    const int q = (int)blockIdx.y, e = (int)(blockIdx.x * 256 + threadIdx.x);
    if (e >= pl_conn_count(c, q)) return;
    const int j = ss_place_row_of(c.db, c.q_problem[q], c.q_nb[((size_t)q * c.q_cap + e) * 2]);
    if (j >= 0) c.flags[(size_t)q * c.db.n_db + j] = (uint8_t)(ss_place_base_flags(c.db, j, c.q_kf[q]) | SS_PLACE_F_CONNECTED);
}

/* grid (ceil(q_stride / 4), n_q, split) */
__global__ __launch_bounds__(256) void k_place_vote(ssk_place_call c)
{
    const int q = (int)blockIdx.y, t = (int)(blockIdx.x * 4 + (threadIdx.x >> 6)), lane = (int)(threadIdx.x & 63);
    if (t >= ss_place_clamp(c.q_count[q], c.q_stride)) return; /* a whole wave */
    const int32_t w = c.q_word[(size_t)q * c.q_stride + t];
    if (!ss_place_word_ok(w, c.db.n_words)) return;
    const int32_t off = c.db.off[w], len = c.db.off[w + 1] - off;
    const size_t row0 = (size_t)q * c.db.n_db;
    for (int i = (int)blockIdx.z * 64 + lane; i < len; i += (int)gridDim.z * 64) {
        const uint32_t r = (uint32_t)c.db.list[off + i];
        if (r < (uint32_t)c.db.n_db && c.flags[row0 + r] == 0) atomicAdd(&c.words[row0 + r], 1);
    }
}

enum { ST_SHARING, ST_MAX, ST_MIN, ST_SURV, ST_SEEDS, ST_FLOOR }; /* a query's eight words of state */

__global__ __launch_bounds__(PL_REDUCE_T) void k_place_reduce(ssk_place_call c)
{
    __shared__ int sh[2];
    __shared__ int wave_n[2][PL_REDUCE_T / 64];
    const int q = (int)blockIdx.x, tid = (int)threadIdx.x, n_db = c.db.n_db, lane = tid & 63, wave = tid >> 6;
    const size_t row0 = (size_t)q * n_db;
    if (tid < 2) sh[tid] = 0;
    __syncthreads();
    int sharing = 0, mx = 0;
    for (int r = tid; r < n_db; r += PL_REDUCE_T) {
        const int w = c.words[row0 + r];
        sharing += w > 0, mx = max(mx, w);
    }
    if (sharing) atomicAdd(&sh[0], sharing);
    if (mx) atomicMax(&sh[1], mx);
    __syncthreads();
    const int max_common = sh[1], min_common = ss_place_min_common(max_common, c.p.common_ratio);
    int total = 0, chunk = 0;
    for (int base = 0; base < n_db; base += PL_REDUCE_T, chunk ^= 1) {
        const int r = base + tid;
        const bool keep = r < n_db && ss_place_survivor(c.flags[row0 + r], c.words[row0 + r], min_common);
        const unsigned long long vote = __ballot(keep);
        if (lane == 0) wave_n[chunk][wave] = (int)__popcll(vote);
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int v = 0; v < PL_REDUCE_T / 64; v++) {
            const int x = wave_n[chunk][v];
            before += v < wave ? x : 0, all += x;
        }
        if (keep) c.surv[row0 + total + before + (int)__popcll(vote & ((1ull << lane) - 1ull))] = r;
        total += all;
    }
    if (tid == 0) {
        int32_t *st = c.state + 8 * (size_t)q;
        st[ST_SHARING] = sh[0], st[ST_MAX] = max_common, st[ST_MIN] = min_common, st[ST_SURV] = total;
    }
}

/* grid (blocks, n_q): wave g of a query takes the slots g, g + waves, ...: the survivors, then (mode 1) the connected entries */
__global__ __launch_bounds__(256) void k_place_score(ssk_place_call c)
{
    const int q = (int)blockIdx.y, lane = (int)(threadIdx.x & 63), waves = (int)gridDim.x * 4;
    const int n_surv = c.state[8 * (size_t)q + ST_SURV], n_conn = c.p.min_score_mode == 1 ? pl_conn_count(c, q) : 0;
    const size_t row0 = (size_t)q * c.db.n_db;
    const int nq = ss_place_clamp(c.q_count[q], c.q_stride);
    for (int slot = (int)(blockIdx.x * 4 + (threadIdx.x >> 6)); slot < n_surv + n_conn; slot += waves) {
        int r;
        if (slot < n_surv) {
            r = c.surv[row0 + slot];
        } else {
            r = ss_place_row_of(c.db, c.q_problem[q], c.q_nb[((size_t)q * c.q_cap + (slot - n_surv)) * 2]);
            if (r < 0 || (c.flags[row0 + r] & SS_PLACE_F_SKIP)) continue; /* uniform over the wave */
        }
        const double s = ss_bow_score_wave(c.q_word + (size_t)q * c.q_stride, c.q_value + (size_t)q * c.q_stride, nq, c.db.word + (size_t)r * c.db.stride,
                                           c.db.value + (size_t)r * c.db.stride, ss_place_clamp(c.db.count[r], c.db.stride), lane);
        if (lane == 0) c.score[row0 + r] = ss_place_round(s);
    }
}

__global__ __launch_bounds__(64) void k_place_floor(ssk_place_call c)
{
    const int q = (int)(blockIdx.x * 64 + threadIdx.x);
    if (q >= c.n_q) return;
    float m = c.p.min_score;
    if (c.p.min_score_mode == 1) {
        m = 1.0f;
        const int n_conn = pl_conn_count(c, q);
        const size_t row0 = (size_t)q * c.db.n_db;
        for (int e = 0; e < n_conn; e++) {
            const int j = ss_place_row_of(c.db, c.q_problem[q], c.q_nb[((size_t)q * c.q_cap + e) * 2]);
            if (j < 0 || (c.flags[row0 + j] & SS_PLACE_F_SKIP)) continue;
            const float s = c.score[row0 + j];
            if (s < m) m = s;
        }
    }
    ((float *)c.state)[8 * (size_t)q + ST_FLOOR] = m;
}

__global__ __launch_bounds__(256) void k_place_seeds(ssk_place_call c)
{
    const int q = (int)blockIdx.y;
    const int32_t *st = c.state + 8 * (size_t)q;
    const int n_surv = st[ST_SURV], min_common = st[ST_MIN];
    const float floor_s = ((const float *)st)[ST_FLOOR];
    const size_t row0 = (size_t)q * c.db.n_db;
    int seeds = 0;
    for (int slot = (int)(blockIdx.x * 256 + threadIdx.x); slot < n_surv; slot += (int)gridDim.x * 256) {
        const int i = c.surv[row0 + slot];
        const float s = c.score[row0 + i];
        if (!(s >= floor_s)) continue;
        seeds++;
        float acc;
        int best;
        ss_place_group(c.db, i, s, c.nb + (size_t)i * c.nb_cap * 2, c.nb_cap, c.flags + row0, c.words + row0, c.score + row0, min_common, &acc, &best);
        atomicMax(&c.star[row0 + best], ss_place_key(acc));
    }
    if (seeds) atomicAdd(&c.state[8 * (size_t)q + ST_SEEDS], seeds);
}

__device__ __forceinline__ uint64_t pl_wave_max(uint64_t x)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)x, d), hi = (uint32_t)__shfl_xor((int)(uint32_t)(x >> 32), d);
        const uint64_t y = ((uint64_t)hi << 32) | lo;
        x = y > x ? y : x;
    }
    return x;
}

__global__ __launch_bounds__(PL_FINAL_T) void k_place_final(ssk_place_call c)
{
    __shared__ unsigned int top_s;
    __shared__ int count_s[2];
    __shared__ uint64_t pick[2][PL_FINAL_T / 64];
    const int q = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int32_t *st = c.state + 8 * (size_t)q;
    const int n_surv = st[ST_SURV], q_problem = c.q_problem[q];
    const size_t row0 = (size_t)q * c.db.n_db;
    if (tid == 0) top_s = 0u, count_s[0] = count_s[1] = 0;
    __syncthreads();
    uint32_t top = 0u;
    for (int slot = tid; slot < n_surv; slot += PL_FINAL_T) top = max(top, c.star[row0 + c.surv[row0 + slot]]);
    if (top) atomicMax(&top_s, top);
    __syncthreads();
    top = top_s;
    const float best_acc = top ? ss_place_unkey(top) : 0.0f;
    const int none[2] = {0, 0};
    int n0 = 0, n1 = 0;
    for (int slot = tid; slot < n_surv; slot += PL_FINAL_T) {
        const int r = c.surv[row0 + slot];
        const uint32_t key = c.star[row0 + r];
        if (!key) continue;
        const int cls = c.db.row_prob[r] != q_problem ? 1 : 0;
        if (ss_place_wanted(c.p, key, best_acc, cls, none)) (cls ? n1 : n0)++;
    }
    if (n0) atomicAdd(&count_s[0], n0);
    if (n1) atomicAdd(&count_s[1], n1);
    __syncthreads();
    n0 = count_s[0], n1 = count_s[1];
    const int n_candidates = c.p.n_best > 0 ? min(n0, c.p.n_best) + min(n1, c.p.n_best) : n0 + n1;
    const int n_written = min(n_candidates, c.cand_cap);
    ss_place_cand *cand = c.cand + (size_t)q * c.cand_cap;
    uint64_t last = ~0ull;
    int taken[2] = {0, 0};
    for (int k = 0; k < n_written; k++) {
        uint64_t mine = 0ull;
        for (int slot = tid; slot < n_surv; slot += PL_FINAL_T) {
            const int r = c.surv[row0 + slot];
            const uint32_t key = c.star[row0 + r];
            if (!key) continue;
            const uint64_t o = ss_place_order(key, r);
            if (o >= last || o <= mine) continue;
            if (ss_place_wanted(c.p, key, best_acc, c.db.row_prob[r] != q_problem ? 1 : 0, taken)) mine = o;
        }
        mine = pl_wave_max(mine);
        if (lane == 0) pick[k & 1][wave] = mine;
        __syncthreads();
        uint64_t won = 0ull;
#pragma unroll
        for (int v = 0; v < PL_FINAL_T / 64; v++) won = max(won, pick[k & 1][v]);
        if (won == 0ull) break; /* uniform; the counts above say it cannot happen */
        const int r = ss_place_order_row(won), cls = c.db.row_prob[r] != q_problem ? 1 : 0;
        if (tid == 0) cand[k] = ss_place_cand_of(c.db, r, q_problem, c.words + row0, c.score + row0, (uint32_t)(won >> 32));
        taken[cls]++;
        last = won;
    }
    for (int e = n_written + tid; e < c.cand_cap; e += PL_FINAL_T) cand[e] = ss_place_no_cand();
    if (tid == 0) {
        ss_place_summary s;
        s.n_sharing = st[ST_SHARING], s.max_common = st[ST_MAX], s.min_common = st[ST_MIN], s.n_survivors = n_surv, s.n_seeds = st[ST_SEEDS];
        s.min_score = ((const float *)st)[ST_FLOOR], s.best_acc = best_acc;
        s.n_candidates = n_candidates, s.n_written = n_written, s.status = SS_OK;
        s.reserved[0] = s.reserved[1] = 0;
        c.summary[q] = s;
    }
}

} // namespace

size_t ssk_place_scan_sums(int n_words) { return ((size_t)n_words + 1 + PL_SCAN_BLOCK - 1) / PL_SCAN_BLOCK; }

int ssk_place_build(hipStream_t s, const ssk_place_lists &b)
{
    const int m = b.n_words + 1;
    const size_t entries = (size_t)b.n_db * b.stride;
    const unsigned scan_blocks = (unsigned)ssk_place_scan_sums(b.n_words);
    const hipError_t e = hipMemsetAsync(b.off, 0, (size_t)m * sizeof(int32_t), s);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_place_count, dim3((unsigned)((entries + 255) / 256)), dim3(256), 0, s, b);
    hipLaunchKernelGGL(k_place_scan_block, dim3(scan_blocks), dim3(PL_SCAN_T), 0, s, b.off, m, b.sums);
    hipLaunchKernelGGL(k_place_scan_sums, dim3(1), dim3(PL_SUMS_T), 0, s, b.sums, (int)scan_blocks);
    hipLaunchKernelGGL(k_place_scan_add, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s, b.off, m, b.sums, b.cursor);
    hipLaunchKernelGGL(k_place_fill, dim3((unsigned)((entries + 255) / 256)), dim3(256), 0, s, b);
    return (int)hipSuccess;
}

void ssk_place_query(hipStream_t s, const ssk_place_call &c, int stage)
{
    const unsigned n_q = (unsigned)c.n_q, n_db = (unsigned)c.db.n_db;
    /* a list is at most n_db long: one more workgroup per 2048 rows of it, sixteen at the most */
    const unsigned split = min(max((n_db + 2047u) / 2048u, 1u), 16u);
    /* the per-survivor kernels: enough waves (lanes) for every row of a small database, 1024 waves (65 536 lanes) per query else */
    const unsigned conn = c.q_nb ? (unsigned)c.q_cap : 0u;
    const unsigned score_blocks = min((n_db + conn + 3u) / 4u, 256u), seed_blocks = min((n_db + 255u) / 256u, 256u);
    switch (stage) {
    case 0:
        hipLaunchKernelGGL(k_place_init, dim3((n_db + 255u) / 256u, n_q), dim3(256), 0, s, c);
        if (c.q_nb) hipLaunchKernelGGL(k_place_connect, dim3(((unsigned)c.q_cap + 255u) / 256u, n_q), dim3(256), 0, s, c);
        break;
    case 1:
        hipLaunchKernelGGL(k_place_vote, dim3(((unsigned)c.q_stride + 3u) / 4u, n_q, split), dim3(256), 0, s, c);
        break;
    case 2:
        hipLaunchKernelGGL(k_place_reduce, dim3(n_q), dim3(PL_REDUCE_T), 0, s, c);
        break;
    case 3:
        hipLaunchKernelGGL(k_place_score, dim3(score_blocks, n_q), dim3(256), 0, s, c);
        hipLaunchKernelGGL(k_place_floor, dim3((n_q + 63u) / 64u), dim3(64), 0, s, c);
        break;
    case 4:
        hipLaunchKernelGGL(k_place_seeds, dim3(seed_blocks, n_q), dim3(256), 0, s, c);
        break;
    default:
        hipLaunchKernelGGL(k_place_final, dim3(n_q), dim3(PL_FINAL_T), 0, s, c);
        break;
    }
}
