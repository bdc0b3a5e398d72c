/*
 * ss_sim3.hip -- Sim3 from matched map points: Sim3Solver's RANSAC over 3-point Horn alignments, every hypothesis of every pair
 * evaluated at once (the rule: include/sendslam_orb.h; DESIGN.md "Sim3 RANSAC").  Every step of the arithmetic is the text of
 * ss_sim3_steps.h, which the host twins compile too.
 *
 *   S-A  k_sim3_gather  one workgroup per pair walks the query rows in chunks of SSK_SIM3_CHUNK in ascending order: ballot and
 *                       prefix sums number the correspondences (gn_chunk_compact of ss_gn.h), so the numbering is the rule's
 *                       whatever the schedule.  A kept row writes its twelve floats into twelve planes and every row the number of
 *                       its correspondence
 *   S-B  k_sim3_model   one lane per pair and hypothesis: the draws, the model in double with the 4 x 4 arrays in registers, one
 *                       128-byte record; the hypothesis' count is zeroed here, so the call needs no memset
 *   S-C  k_sim3_count   a lane owns one correspondence and keeps its twelve floats in registers across SSK_SIM3_HYP_BLOCK
 *                       hypotheses.  A hypothesis' record is one address per wave (scalar loads); one ballot and popcount per wave
 *                       and hypothesis go to LDS, and the workgroup adds its SSK_SIM3_HYP_BLOCK integer sums to the counts with
 *                       one vector atomic.  Integer sums are order-free
 *   S-D  k_sim3_finish  one workgroup per pair: the first hypothesis over the threshold by a min-reduction, the largest count, then
 *                       the winner once more over the query rows for the flags
 *
 * Every floating-point step is a single IEEE operation (-ffp-contract=off).  Every global write is a plain vector store or a vector
 * atomic.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ss_constants.h"
#include "ss_gn.h"
#include "ss_kernels.h"
#include "ss_sim3_steps.h"
#include "ss_quad.h"

namespace {

static_assert(SSK_SIM3_CHUNK == 1024, "k_sim3_gather: one row per thread and chunk, 16 waves");
static_assert(SSK_SIM3_COUNT_ROWS == 256 && SSK_SIM3_HYP_BLOCK <= 64, "k_sim3_count: one correspondence per thread, the sums in one wave");
static_assert(sizeof(ssk_sim3_model) == 128, "one record, eight float4");

/* plane k of the correspondences of pair b */
__device__ __forceinline__ float *sim3_plane(const ssk_sim3_call &a, int k, int b) { return a.corr + ((size_t)k * a.n_frames + b) * a.rows; }

__device__ __forceinline__ ss_sim3_corr sim3_load_corr(const ssk_sim3_call &a, int b, int n)
{
    ss_sim3_corr c;
    c.x1[0] = sim3_plane(a, 0, b)[n], c.x1[1] = sim3_plane(a, 1, b)[n], c.x1[2] = sim3_plane(a, 2, b)[n];
    c.x2[0] = sim3_plane(a, 3, b)[n], c.x2[1] = sim3_plane(a, 4, b)[n], c.x2[2] = sim3_plane(a, 5, b)[n];
    c.u1 = sim3_plane(a, 6, b)[n], c.v1 = sim3_plane(a, 7, b)[n];
    c.u2 = sim3_plane(a, 8, b)[n], c.v2 = sim3_plane(a, 9, b)[n];
    c.max1 = sim3_plane(a, 10, b)[n], c.max2 = sim3_plane(a, 11, b)[n];
    return c;
}

/* both tests of step 3c */
__device__ __forceinline__ bool sim3_inlier(const ssk_sim3_model *m, const ss_sim3_corr &c, const ss_proj_view *v1, const ss_proj_view *v2)
{
    const float e1 = ss_sim3_err(m->sr12, m->t12, c.x2, v1->fx, v1->fy, v1->cx, v1->cy, c.u1, c.v1);
    const float e2 = ss_sim3_err(m->sr21, m->t21, c.x1, v2->fx, v2->fy, v2->cx, v2->cy, c.u2, c.v2);
    return e1 < c.max1 && e2 < c.max2;
}

/* S-A.  grid (pairs), SSK_SIM3_CHUNK threads; corr_of_row of every row < rows is written */
__global__ __launch_bounds__(SSK_SIM3_CHUNK) void k_sim3_gather(ssk_sim3_call a)
{
    __shared__ int wave_n[SSK_SIM3_CHUNK / 64];
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x, rows = a.rows;
    const gd_frame f = gd_frame_of(a.src, a.frame_error, a.nq, a.nt, rows, b);
    const int n_levels = min(max(a.n_levels, 1), SS_MAX_LEVELS);
    const int t = max(f.t, 0);
    const ss_proj_view *v1 = a.views1 + b, *v2 = a.views2 + b; /* one address per workgroup */
    int base = 0;
    for (int c0 = 0; c0 < rows; c0 += SSK_SIM3_CHUNK) { /* uniform */
        const int i = c0 + tid;
        const size_t o = (size_t)b * rows + i;
        bool keep = false;
        int j = -1, o1 = 0, o2 = 0;
        if (i < f.nq) {
            j = a.idx[o];
            if (j >= 0 && j < f.nt) { /* j < nt <= rows */
                const size_t oj = (size_t)t * rows + j;
                o1 = a.q_kp[o].octave, o2 = a.t_kp[oj].octave;
                keep = o1 >= 0 && o1 < n_levels && o2 >= 0 && o2 < n_levels;
                if (keep && a.q_skip && a.q_skip[o] != 0) keep = false;
                if (keep && a.t_skip && a.t_skip[oj] != 0) keep = false;
            }
        }
        const gn_chunk ch = gn_chunk_compact<SSK_SIM3_CHUNK>(keep, wave_n);
        int pos = -1;
        if (keep) {
            pos = gn_chunk_pos(ch, base); /* pos <= i < rows */
            const ss_map_point *p1 = a.q_xyz + o, *p2 = a.t_xyz + (size_t)t * rows + j;
            const ss_sim3_corr c = ss_sim3_corr_of(*v1, *v2, p1->x, p1->y, p1->z, p2->x, p2->y, p2->z, a.chi2, a.scale[o1], a.scale[o2]);
            sim3_plane(a, 0, b)[pos] = c.x1[0], sim3_plane(a, 1, b)[pos] = c.x1[1], sim3_plane(a, 2, b)[pos] = c.x1[2];
            sim3_plane(a, 3, b)[pos] = c.x2[0], sim3_plane(a, 4, b)[pos] = c.x2[1], sim3_plane(a, 5, b)[pos] = c.x2[2];
            sim3_plane(a, 6, b)[pos] = c.u1, sim3_plane(a, 7, b)[pos] = c.v1;
            sim3_plane(a, 8, b)[pos] = c.u2, sim3_plane(a, 9, b)[pos] = c.v2;
            sim3_plane(a, 10, b)[pos] = c.max1, sim3_plane(a, 11, b)[pos] = c.max2;
        }
        if (i < rows) a.corr_of_row[o] = pos;
        base += ch.total;
        __syncthreads(); /* wave_n is rewritten */
    }
    if (tid == 0) a.n_corr[b] = base;
}

/* S-B.  grid (ceil(max_iterations / 64), pairs), 64 threads */
__global__ __launch_bounds__(64) void k_sim3_model(ssk_sim3_call a)
{
    const int b = (int)blockIdx.y, t = (int)(blockIdx.x * 64 + threadIdx.x);
    if (t >= a.max_iterations) return;
    const int n = min(max(a.n_corr[b], 0), a.rows);
    const size_t at = (size_t)b * a.max_iterations + t;
    a.counts[at] = 0;
    if (ss_sim3_too_few(n, a.min_inliers)) return;
    int pick[3];
    ss_sim3_draw(a.seed, (uint32_t)b, t, n, pick); /* each in 0 .. n-1 */
    float x1[9], x2[9];
#pragma unroll
    for (int k = 0; k < 3; k++) {
#pragma unroll
        for (int i = 0; i < 3; i++) {
            x1[3 * k + i] = sim3_plane(a, i, b)[pick[k]];
            x2[3 * k + i] = sim3_plane(a, 3 + i, b)[pick[k]];
        }
    }
    const ss_sim3_model m = ss_sim3_model_of(x1, x2, a.fix_scale);
    float4 *out = (float4 *)(a.models + at);
    out[0] = make_float4(m.sr12[0], m.sr12[1], m.sr12[2], m.sr12[3]);
    out[1] = make_float4(m.sr12[4], m.sr12[5], m.sr12[6], m.sr12[7]);
    out[2] = make_float4(m.sr12[8], m.t12[0], m.t12[1], m.t12[2]);
    out[3] = make_float4(m.sr21[0], m.sr21[1], m.sr21[2], m.sr21[3]);
    out[4] = make_float4(m.sr21[4], m.sr21[5], m.sr21[6], m.sr21[7]);
    out[5] = make_float4(m.sr21[8], m.t21[0], m.t21[1], m.t21[2]);
    out[6] = make_float4(m.s12, 0.0f, 0.0f, 0.0f);
    out[7] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

/* S-C.  grid (ceil(rows / SSK_SIM3_COUNT_ROWS), ceil(max_iterations / SSK_SIM3_HYP_BLOCK), pairs), SSK_SIM3_COUNT_ROWS threads */
__global__ __launch_bounds__(SSK_SIM3_COUNT_ROWS) void k_sim3_count(ssk_sim3_call a)
{
    __shared__ int cnt[SSK_SIM3_HYP_BLOCK];
    const int b = (int)blockIdx.z, tid = (int)threadIdx.x;
    const int n_corr = min(max(a.n_corr[b], 0), a.rows);
    const int n0 = (int)blockIdx.x * SSK_SIM3_COUNT_ROWS;
    if (ss_sim3_too_few(n_corr, a.min_inliers) || n0 >= n_corr) return; /* uniform */
    const int n = n0 + tid;
    const bool live = n < n_corr;
    const ss_sim3_corr c = sim3_load_corr(a, b, live ? n : 0);
    const ss_proj_view *v1 = a.views1 + b, *v2 = a.views2 + b;
    const int t0 = (int)blockIdx.y * SSK_SIM3_HYP_BLOCK;
    const ssk_sim3_model *models = a.models + (size_t)b * a.max_iterations;
    if (tid < SSK_SIM3_HYP_BLOCK) cnt[tid] = 0;
    __syncthreads();
    for (int h = 0; h < SSK_SIM3_HYP_BLOCK && t0 + h < a.max_iterations; h++) { /* uniform */
        const bool in = live && sim3_inlier(models + t0 + h, c, v1, v2);
        const unsigned long long mask = __ballot(in);
        if ((tid & 63) == 0 && mask != 0ull) atomicAdd(&cnt[h], __popcll(mask));
    }
    __syncthreads();
    if (tid < SSK_SIM3_HYP_BLOCK && t0 + tid < a.max_iterations && cnt[tid] > 0) atomicAdd(a.counts + (size_t)b * a.max_iterations + t0 + tid, cnt[tid]);
}

/* S-D.  grid (pairs), 256 threads; the flag of every row < rows and the result are written */
__global__ __launch_bounds__(256) void k_sim3_finish(ssk_sim3_call a)
{
    __shared__ int s_first, s_best, s_inliers;
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x, rows = a.rows;
    const gd_frame f = gd_frame_of(a.src, a.frame_error, a.nq, a.nt, rows, b);
    const int n_corr = min(max(a.n_corr[b], 0), rows);
    const bool too_few = ss_sim3_too_few(n_corr, a.min_inliers);
    const int none = 0x7FFFFFFF;
    if (tid == 0) s_first = none, s_best = 0, s_inliers = 0;
    __syncthreads();
    if (!too_few) {
        int first = none, best = 0;
        for (int t = tid; t < a.max_iterations; t += 256) {
            const int c = a.counts[(size_t)b * a.max_iterations + t];
            best = max(best, c);
            if (ss_sim3_wins(c, a.min_inliers)) first = min(first, t);
        }
        if (best > 0) atomicMax(&s_best, best);
        if (first != none) atomicMin(&s_first, first);
    }
    __syncthreads();
    const int win = s_first;
    const ssk_sim3_model *m = a.models + (size_t)b * a.max_iterations + (win == none ? 0 : win);
    const ss_proj_view *v1 = a.views1 + b, *v2 = a.views2 + b;
    int mine = 0;
    for (int i = tid; i < rows; i += 256) {
        const size_t o = (size_t)b * rows + i;
        const int n = a.corr_of_row[o];
        uint8_t flag = 0;
        if (win != none && n >= 0 && n < n_corr) flag = sim3_inlier(m, sim3_load_corr(a, b, n), v1, v2) ? 1 : 0;
        a.inlier[o] = flag;
        mine += flag;
    }
    if (mine) atomicAdd(&s_inliers, mine);
    __syncthreads();
    if (tid == 0) {
        ss_sim3_result r;
        for (int k = 0; k < 9; k++) r.sr12[k] = win == none ? 0.0f : m->sr12[k], r.sr21[k] = win == none ? 0.0f : m->sr21[k];
        for (int k = 0; k < 3; k++) r.t12[k] = win == none ? 0.0f : m->t12[k], r.t21[k] = win == none ? 0.0f : m->t21[k];
        r.s12 = win == none ? 0.0f : m->s12;
        r.state = too_few ? 1 : win == none ? 2 : 0;
        r.n_corr = n_corr;
        r.n_inliers = s_inliers;
        r.best_inliers = s_best;
        r.iteration = win == none ? -1 : win;
        r.status = f.status;
        r.reserved = 0;
        a.result[b] = r;
    }
}

} // namespace

void ssk_sim3_gather(hipStream_t s, const ssk_sim3_call &g) { hipLaunchKernelGGL(k_sim3_gather, dim3((unsigned)g.n_frames), dim3(SSK_SIM3_CHUNK), 0, s, g); }

void ssk_sim3_model_launch(hipStream_t s, const ssk_sim3_call &g)
{
    hipLaunchKernelGGL(k_sim3_model, dim3((unsigned)((g.max_iterations + 63) / 64), (unsigned)g.n_frames), dim3(64), 0, s, g);
}

void ssk_sim3_count(hipStream_t s, const ssk_sim3_call &g)
{
    const dim3 grid((unsigned)((g.rows + SSK_SIM3_COUNT_ROWS - 1) / SSK_SIM3_COUNT_ROWS),
                    (unsigned)((g.max_iterations + SSK_SIM3_HYP_BLOCK - 1) / SSK_SIM3_HYP_BLOCK), (unsigned)g.n_frames);
    hipLaunchKernelGGL(k_sim3_count, grid, dim3(SSK_SIM3_COUNT_ROWS), 0, s, g);
}

void ssk_sim3_finish(hipStream_t s, const ssk_sim3_call &g) { hipLaunchKernelGGL(k_sim3_finish, dim3((unsigned)g.n_frames), dim3(256), 0, s, g); }
