/*
 * ss_sim3opt.hip -- Sim3 refinement: the bookkeeping of ORBmatcher::SearchBySim3 and the 7-DoF damped Gauss-Newton of
 * Optimizer::OptimizeSim3 for every loop candidate of a call at once (the rule: include/sendslam_orb.h; DESIGN.md "Sim3
 * refinement").  Every step of the arithmetic is the text of ss_sim3opt_steps.h, which the host twin compiles too.
 *
 *   O-A  k_sim3opt_gather  one workgroup per pair walks the query rows in chunks of SSK_SIM3OPT_CHUNK in ascending order: ballot and
 *                          prefix sums number the correspondences (gn_chunk_compact of ss_gn.h).  A kept row writes its twelve floats
 *                          (X1 and X2 in float32 by the RANSAC's text, both keypoints, both scales) into twelve planes and its query
 *                          row; every other row gets its flag 2 here.  A pair without a usable start keeps nothing
 *   O-B  k_sim3opt_solve   one workgroup of SS_GN_SLOTS threads per pair holds both rounds (its own loop on ss_gn.h).  Thread s owns
 *                          the correspondences s, s + 256, ...: it re-reads their planes every step, adds the e12 terms and then the
 *                          e21 terms into its 35 partial sums in registers (one edge's rows are live at a time) and keeps its
 *                          correspondences' inlier bits in one 64-bit mask.  A wave folds by halving through cross-lane moves, the
 *                          four wave results go through LDS (gn_block_sum of ss_gn.h), and every thread solves the same system, so the
 *                          model needs no broadcast and every branch on it is uniform
 *   O-C  k_sim3_marks      one workgroup per pair: the skip bytes of both searches of SearchBySim3
 *   O-D  k_sim3_mutual     one workgroup per pair: the agreement test of the two searches' results
 *
 * Every floating-point step is a single IEEE operation (-ffp-contract=off).  Every global write is a plain vector store; there is no
 * atomic.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ss_constants.h"
#include "ss_gn.h"
#include "ss_kernels.h"
#include "ss_sim3opt_steps.h"
#include "ss_quad.h"

namespace {

static_assert(SSK_SIM3OPT_CHUNK == 1024, "k_sim3opt_gather: one row per thread and chunk, 16 waves");
static_assert(SS_GN_SLOTS == 256, "k_sim3opt_solve: four waves, one group of 64 slots each");
static_assert(SS_GUIDED_MAX_ROWS <= 64 * SS_GN_SLOTS, "k_sim3opt_solve: a thread's correspondences have one bit each in a 64-bit mask");
static_assert(sizeof(ss_sim3_opt_result) == 272, "fourteen doubles, eight integers, one ss_sim3_result, no padding");
static_assert(sizeof(ss_sim3_opt_params) == 64 && sizeof(ss_sim3_mutual_summary) == 8, "the documented sizes");

/* plane k of the correspondences of pair b */
__device__ __forceinline__ float *opt_plane(const ssk_sim3opt_call &a, int k, int b) { return a.planes + ((size_t)k * a.n_frames + b) * a.rows; }

__device__ __forceinline__ ss_sim3opt_corr opt_load(const ssk_sim3opt_call &a, int b, int n)
{
    const float x1[3] = {opt_plane(a, 0, b)[n], opt_plane(a, 1, b)[n], opt_plane(a, 2, b)[n]};
    const float x2[3] = {opt_plane(a, 3, b)[n], opt_plane(a, 4, b)[n], opt_plane(a, 5, b)[n]};
    return ss_sim3opt_corr_of(x1, x2, opt_plane(a, 6, b)[n], opt_plane(a, 7, b)[n], opt_plane(a, 8, b)[n], opt_plane(a, 9, b)[n], opt_plane(a, 10, b)[n],
                              opt_plane(a, 11, b)[n]);
}

/* the pair's status: the frame's before the start's */
__device__ __forceinline__ int opt_status(const gd_frame &f, const ss_sim3_result &start) { return f.status ? f.status : start.status; }

/* O-A.  grid (pairs), SSK_SIM3OPT_CHUNK threads; the flag of every row < rows that is no correspondence is written */
__global__ __launch_bounds__(SSK_SIM3OPT_CHUNK) void k_sim3opt_gather(ssk_sim3opt_call a)
{
    __shared__ int wave_n[SSK_SIM3OPT_CHUNK / 64];
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x, rows = a.rows;
    const gd_frame f = gd_frame_of(a.src, a.frame_error, a.nq, a.nt, rows, b);
    const int n_levels = min(max(a.n_levels, 1), SS_MAX_LEVELS);
    const int t = max(f.t, 0);
    const ss_proj_view *v1 = a.views1 + b, *v2 = a.views2 + b; /* one address per workgroup */
    const bool usable = ss_sim3opt_start_usable(a.start[b]);
    int base = 0;
    for (int c0 = 0; c0 < rows; c0 += SSK_SIM3OPT_CHUNK) { /* uniform */
        const int i = c0 + tid;
        const size_t o = (size_t)b * rows + i;
        bool keep = false;
        int j = -1, o1 = 0, o2 = 0;
        if (usable && i < f.nq) {
            j = a.idx[o];
            if (j >= 0 && j < f.nt) { /* j < nt <= rows */
                const size_t oj = (size_t)t * rows + j;
                o1 = a.q_kp[o].octave, o2 = a.t_kp[oj].octave;
                keep = o1 >= 0 && o1 < n_levels && o2 >= 0 && o2 < n_levels;
                if (keep && a.q_skip && a.q_skip[o] != 0) keep = false;
                if (keep && a.t_skip && a.t_skip[oj] != 0) keep = false;
            }
        }
        const gn_chunk ch = gn_chunk_compact<SSK_SIM3OPT_CHUNK>(keep, wave_n);
        if (keep) {
            const int pos = gn_chunk_pos(ch, base); /* pos <= i < rows */
            const size_t oj = (size_t)t * rows + j;
            const ss_map_point *p1 = a.q_xyz + o, *p2 = a.t_xyz + oj;
            float x1[3], x2[3];
            ss_sim3_transform(v1->rcw, v1->tcw, p1->x, p1->y, p1->z, x1);
            ss_sim3_transform(v2->rcw, v2->tcw, p2->x, p2->y, p2->z, x2);
            opt_plane(a, 0, b)[pos] = x1[0], opt_plane(a, 1, b)[pos] = x1[1], opt_plane(a, 2, b)[pos] = x1[2];
            opt_plane(a, 3, b)[pos] = x2[0], opt_plane(a, 4, b)[pos] = x2[1], opt_plane(a, 5, b)[pos] = x2[2];
            opt_plane(a, 6, b)[pos] = a.q_kp[o].x, opt_plane(a, 7, b)[pos] = a.q_kp[o].y;
            opt_plane(a, 8, b)[pos] = a.t_kp[oj].x, opt_plane(a, 9, b)[pos] = a.t_kp[oj].y;
            opt_plane(a, 10, b)[pos] = a.scale[o1], opt_plane(a, 11, b)[pos] = a.scale[o2];
            a.row_of[(size_t)b * rows + pos] = i;
        } else if (i < rows) {
            a.flags[o] = 2;
        }
        base += ch.total;
        __syncthreads(); /* wave_n is rewritten */
    }
    if (tid == 0) a.n_corr[b] = base;
}

/* O-B.  grid (pairs), SS_GN_SLOTS threads; the flag of every correspondence's row and the result are written */
__global__ __launch_bounds__(SS_GN_SLOTS) void k_sim3opt_solve(ssk_sim3opt_call a)
{
    __shared__ double part[2][4][SS_SIM3OPT_SUMS];
    __shared__ int part_n[2][4];
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x, rows = a.rows;
    const gd_frame f = gd_frame_of(a.src, a.frame_error, a.nq, a.nt, rows, b);
    const int n = min(max(a.n_corr[b], 0), rows);
    const ss_sim3opt_cams cam = ss_sim3opt_cams_of(a.views1[b], a.views2[b], a.p.chi2);
    const ss_sim3_result start = a.start[b];
    const bool fix = a.p.fix_scale != 0;
    double R[9], t[3], s, R0[9], t0[3], s0;
    const bool usable = ss_sim3opt_start_usable(start);
    const bool start_ok = ss_sim3opt_start(start, fix, R, t, &s);
#pragma unroll
    for (int k = 0; k < 9; k++) R0[k] = R[k];
#pragma unroll
    for (int k = 0; k < 3; k++) t0[k] = t[k];
    s0 = s;
    unsigned long long active = ~0ull; /* bit j: correspondence tid + 256 j is an inlier */
    const int status = opt_status(f, start);
    int state = (status != 0 || !usable) ? 1 : !start_ok ? 2 : n < a.p.min_corr ? 1 : 0;
    int n_in = n, n_removed = 0, steps0 = 0, steps1 = 0, buf = 0;
    double cost = 0.0;
    for (int round = 0; state == 0 && round < 2; round++) { /* everything the loops branch on is the same in every thread */
        const bool robust = round == 0;
        const int iterations = round == 0 ? a.p.iterations0 : n_removed > 0 ? a.p.iterations_more : a.p.iterations_same;
        for (int it = 0; it < iterations; it++) {
            double sum[SS_SIM3OPT_SUMS]; /* this thread's partial sums, then the pair's */
#pragma unroll
            for (int q = 0; q < SS_SIM3OPT_SUMS; q++) sum[q] = 0.0;
            int j = 0;
            for (int k = tid; k < n; k += SS_GN_SLOTS, j++) {
                if (!((active >> j) & 1ull)) continue;
                const ss_sim3opt_corr c = opt_load(a, b, k);
                ss_sim3opt_edge e;
                if (ss_sim3opt_edge12(c, cam, R, t, s, e)) ss_sim3opt_add(e, cam, robust, sum);
                if (ss_sim3opt_edge21(c, cam, R, t, s, e)) ss_sim3opt_add(e, cam, robust, sum);
            }
            gn_block_sum(sum, part, &buf);
            bool small;
            const int rc = ss_sim3opt_step(sum, fix, a.p.lambda, a.p.step_eps, R, t, &s, &small);
            if (rc != 0) {
                state = rc;
                break;
            }
            if (round == 0) steps0++;
            else steps1++;
            if (small) break;
        }
        if (state != 0) break;
        unsigned long long now = 0ull;
        double mine = 0.0;
        int mine_n = 0, j = 0;
        for (int k = tid; k < n; k += SS_GN_SLOTS, j++) {
            if (!((active >> j) & 1ull)) continue; /* a removed correspondence stays removed */
            const ss_sim3opt_corr c = opt_load(a, b, k);
            const double c12 = ss_sim3opt_chi2_12(c, cam, R, t, s), c21 = ss_sim3opt_chi2_21(c, cam, R, t, s);
            if (ss_sim3opt_inlier(cam, c12, c21)) {
                now |= 1ull << j;
                mine = mine + (c12 + c21);
                mine_n++;
            }
        }
        active = now;
        gn_block_sum(&mine, &mine_n, part, part_n, &buf);
        cost = mine, n_in = mine_n;
        if (round == 0) {
            n_removed = n - n_in;
            if (n_in < a.p.min_inliers) state = 3;
        }
    }
    int j = 0;
    for (int k = tid; k < n; k += SS_GN_SLOTS, j++) {
        const int row = a.row_of[(size_t)b * rows + k];
        if (row >= 0 && row < rows) a.flags[(size_t)b * rows + row] = ((active >> j) & 1ull) ? 0 : 1;
    }
    if (tid == 0) {
        ss_sim3_opt_result r;
        ss_sim3opt_record(R, t, s, R0, t0, s0, cost, state, status, n, n_removed, n_in, steps0, steps1, &r);
        a.result[b] = r;
    }
}

/* idx[i] of pair b names a train row */
__device__ __forceinline__ bool marks_valid(const gd_frame &f, int i, int j) { return i < f.nq && j >= 0 && j < f.nt; }

/* O-C.  grid (pairs), 256 threads; skip1 and skip2 of every row < rows are written */
__global__ __launch_bounds__(256) void k_sim3_marks(ssk_sim3_marks_call a)
{
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x, rows = a.rows;
    const gd_frame f = gd_frame_of(a.src, a.frame_error, a.nq, a.nt, rows, b);
    const int t = max(f.t, 0);
    for (int i = tid; i < rows; i += 256) {
        const size_t o = (size_t)b * rows + i;
        const bool own = a.q_skip && a.q_skip[o] != 0;
        a.skip1[o] = (own || marks_valid(f, i, a.idx[o])) ? 1 : 0;
        a.skip2[o] = (a.t_skip && f.t >= 0 && a.t_skip[(size_t)t * rows + i] != 0) ? 1 : 0;
    }
    __syncthreads(); /* the base values are written before any mark */
    for (int i = tid; i < rows; i += 256) {
        const int j = a.idx[(size_t)b * rows + i];
        if (marks_valid(f, i, j)) a.skip2[(size_t)b * rows + j] = 1; /* j < nt <= rows; every store here writes 1 */
    }
}

/* O-D.  grid (pairs), 256 threads; idx_out of every row < rows and the summary are written */
__global__ __launch_bounds__(256) void k_sim3_mutual(ssk_sim3_marks_call a)
{
    __shared__ int cnt[2][4];
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x, rows = a.rows;
    const int lane = tid & 63, wave = tid >> 6;
    const gd_frame f = gd_frame_of(a.src, a.frame_error, a.nq, a.nt, rows, b);
    uint8_t *taken = a.taken + (size_t)b * rows;
    for (int i = tid; i < rows; i += 256) taken[i] = 0;
    __syncthreads();
    for (int i = tid; i < rows; i += 256) {
        const int j = a.idx[(size_t)b * rows + i];
        if (marks_valid(f, i, j)) taken[j] = 1;
    }
    __syncthreads();
    int n_prior = 0, n_new = 0;
    for (int i = tid; i < rows; i += 256) {
        const size_t o = (size_t)b * rows + i;
        const int prior = a.idx[o];
        int out = -1;
        if (marks_valid(f, i, prior)) {
            out = prior;
            n_prior++;
        } else if (i < f.nq) {
            const int j = a.idx12[o];
            if (j >= 0 && j < f.nt && a.idx21[(size_t)b * rows + j] == i && taken[j] == 0) {
                out = j;
                n_new++;
            }
        }
        a.idx_out[o] = out;
    }
    n_prior = gn_wave_fold(n_prior), n_new = gn_wave_fold(n_new);
    if (lane == 0) cnt[0][wave] = n_prior, cnt[1][wave] = n_new;
    __syncthreads();
    if (tid == 0) {
        ss_sim3_mutual_summary s;
        s.n_prior = (cnt[0][0] + cnt[0][1]) + (cnt[0][2] + cnt[0][3]);
        s.n_new = (cnt[1][0] + cnt[1][1]) + (cnt[1][2] + cnt[1][3]);
        a.summary[b] = s;
    }
}

} // namespace

void ssk_sim3opt_gather(hipStream_t s, const ssk_sim3opt_call &g) { hipLaunchKernelGGL(k_sim3opt_gather, dim3((unsigned)g.n_frames), dim3(SSK_SIM3OPT_CHUNK), 0, s, g); }

void ssk_sim3opt_solve(hipStream_t s, const ssk_sim3opt_call &g) { hipLaunchKernelGGL(k_sim3opt_solve, dim3((unsigned)g.n_frames), dim3(SS_GN_SLOTS), 0, s, g); }

void ssk_sim3_marks(hipStream_t s, const ssk_sim3_marks_call &g) { hipLaunchKernelGGL(k_sim3_marks, dim3((unsigned)g.n_frames), dim3(256), 0, s, g); }

void ssk_sim3_mutual(hipStream_t s, const ssk_sim3_marks_call &g) { hipLaunchKernelGGL(k_sim3_mutual, dim3((unsigned)g.n_frames), dim3(256), 0, s, g); }
