/*
 * ss_gba.hip -- global bundle adjustment: the Levenberg-Marquardt of Optimizer::BundleAdjustment over every keyframe and point of
 * a map, its reduced camera system applied matrix-free under preconditioned conjugate gradients, for every map (problem) of a call
 * at once (the rule: include/sendslam_orb.h; DESIGN.md "Global bundle adjustment").  Every step of the arithmetic is the text of
 * ss_gba_steps.h and ss_ba_steps.h, which the host twin compiles too.
 *
 * The host enqueues the fixed schedule of every round, step and PCG iteration without a round trip; a problem's state
 * (ssk_gba_state) lives in device memory, and a kernel whose problem has ended, whose round is over or whose PCG has left returns
 * at once.  One workgroup cannot carry a map's operator, so a PCG iteration is three launches, not a loop inside a workgroup.
 *
 *   A-A  k_gba_gather_kf, k_gba_gather_points, k_gba_gather_state   the starts into both pose buffers, the points widened, their
 *                           flags and the records' bytes, the problem's state
 *   A-B  k_gba_points       one lane per point: its list linearised in ascending kf, V, b, the factor, W per free record
 *   A-C  k_gba_blocks       one workgroup per keyframe: the 53 trees over its list, the damped block's factor, r_k, z_k
 *        k_gba_pcg_init     one workgroup per problem: the pivots' verdict, rho = r.z, the stop value
 *   A-D  k_gba_pcg_points   one lane per point: a_i = sum W^T.p, c_i = V^-1.a_i
 *        k_gba_pcg_kf       one workgroup per keyframe: q_k = U_k.p_k - tree of W.c
 *        k_gba_pcg_step     one workgroup per problem: both dot products, x, r, z, p and the three exits
 *   A-E  k_gba_update_kf, k_gba_update_points   the trial poses, the back-substitution and the trial points
 *   A-F  k_gba_cost         one workgroup per keyframe: the tree of its chi-terms
 *        k_gba_accept       one workgroup per problem: the tree over the keyframes, accept or reject, lambda, the end of a round
 *   A-G  k_gba_classify     per point after a round
 *   A-H  k_gba_finish_points, k_gba_finish_obs, k_gba_finish_kf, k_gba_finish_state   the outputs
 *
 * Every floating-point step is a single IEEE operation (-ffp-contract=off).  Every global write is a plain vector store; there are
 * no atomics and no grid-wide barrier.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ss_gba_steps.h"
#include "ss_gn.h"
#include "ss_kernels.h"

namespace {

static_assert(SS_GN_SLOTS == 256, "four waves, one group of 64 slots each");
static_assert(sizeof(ss_gba_result) == 104 && sizeof(ss_gba_params) == 104 && sizeof(ss_gba_problem) == 32 && sizeof(ss_gba_obs) == 24 && sizeof(ss_gba_rec) == 32,
              "the layouts of the header");

struct gba_prob {
    int k0, n_kf, b0, n_blocks, s0, n_obs;
};

/* the host has checked the table: the clamps only keep a stray value inside the arrays */
__device__ __forceinline__ gba_prob gba_prob_of(const ssk_gba_call &a, int q)
{
    const ss_gba_problem p = a.prob[q];
    gba_prob r;
    r.n_kf = min(max(p.n_kf, 1), a.n_kf);
    r.k0 = min(max(p.first_kf, 0), a.n_kf - r.n_kf);
    r.n_blocks = min(max(p.n_blocks, 0), a.n_blocks);
    r.b0 = min(max(p.first_block, 0), a.n_blocks - r.n_blocks);
    r.n_obs = min(max(p.n_obs, 0), a.n_obs);
    r.s0 = min(max(p.first_obs, 0), a.n_obs - r.n_obs);
    return r;
}

__device__ __forceinline__ bool gba_running(const ssk_gba_call &a, int q) { return a.st[q].ended == 0 && a.st[q].round_over == 0; }

__device__ __forceinline__ int gba_pblocks(const ssk_gba_call &a) { return (a.point_rows + SS_GN_SLOTS - 1) / SS_GN_SLOTS; }

/* a lane of a per-point kernel: workgroup w covers 256 rows of block w / pblocks */
struct gba_lane {
    int b, row, q;
    size_t gp; /* the point's number in the call's arrays */
};

__device__ __forceinline__ gba_lane gba_lane_of(const ssk_gba_call &a)
{
    const int pb = gba_pblocks(a);
    gba_lane l;
    l.b = min((int)blockIdx.x / pb, a.n_blocks - 1);
    l.row = ((int)blockIdx.x % pb) * SS_GN_SLOTS + (int)threadIdx.x;
    const int q = a.blk_prob[l.b];
    l.q = (q >= 0 && q < a.n_problems) ? q : -1;
    l.gp = (size_t)l.b * a.point_rows + min(l.row, a.point_rows - 1);
    return l;
}

/* the point's run of the problem's records, kept inside them */
__device__ __forceinline__ void gba_point_list(const ssk_gba_call &a, const gba_prob &pr, size_t gp, int *off, int *cnt)
{
    *off = min(max(a.pt_off[gp], 0), pr.n_obs);
    *cnt = min(max(a.pt_cnt[gp], 0), pr.n_obs - *off);
}

__device__ __forceinline__ void gba_kf_list(const ssk_gba_call &a, const gba_prob &pr, int k, int *off, int *cnt)
{
    *off = min(max(a.kf_off[k], 0), pr.n_obs);
    *cnt = min(max(a.kf_cnt[k], 0), pr.n_obs - *off);
}

/* item j of keyframe k's list -> the record's number in the call's arrays (the problem has a record: cnt > 0) */
__device__ __forceinline__ size_t gba_kf_item(const ssk_gba_call &a, const gba_prob &pr, int off, int j)
{
    return (size_t)pr.s0 + (size_t)min(max(a.kf_list[(size_t)pr.s0 + off + j], 0), pr.n_obs - 1);
}

__device__ __forceinline__ int gba_rec_kf(const gba_prob &pr, const ss_gba_rec &r) { return pr.k0 + min(max(r.kf, 0), pr.n_kf - 1); }

__device__ __forceinline__ size_t gba_rec_point(const ssk_gba_call &a, const gba_prob &pr, const ss_gba_rec &r)
{
    const int P = pr.n_blocks * a.point_rows;
    return (size_t)pr.b0 * a.point_rows + (size_t)min(max(r.point, 0), P - 1);
}

__device__ __forceinline__ const double *gba_pose(const ssk_gba_call &a, int buf, int k) { return a.pose + ((size_t)buf * a.n_kf + k) * 12; }

__device__ __forceinline__ double *gba_X(const ssk_gba_call &a, int buf, size_t gp)
{
    return a.X + ((size_t)buf * a.n_blocks * a.point_rows + gp) * 3;
}

__device__ __forceinline__ void gba_load_pose(const double *src, double R[9], double t[3])
{
#pragma unroll
    for (int e = 0; e < 9; e++) R[e] = src[e];
#pragma unroll
    for (int e = 0; e < 3; e++) t[e] = src[9 + e];
}

__device__ __forceinline__ ss_pose_cam gba_cam(const ssk_gba_call &a, int k) { return ss_pose_cam_of(a.views[k], a.p.chi2_mono, a.p.chi2_stereo); }

__device__ __forceinline__ ss_pose_obs gba_obs(const ssk_gba_call &a, int buf, size_t gp, const ss_gba_rec &r)
{
    const double *Xp = gba_X(a, buf, gp);
    const double X[3] = {Xp[0], Xp[1], Xp[2]};
    return ss_ba_obs_of(X, ss_gba_meas_of(r));
}

/* the tree of a dot product over the n entries of a problem's vectors: thread s is slot s */
__device__ __forceinline__ double gba_dot(const double *x, const double *y, int n, double (*part)[4][1], int *buf)
{
    double sum[1] = {0.0};
    for (int k = (int)threadIdx.x; k < n; k += SS_GN_SLOTS) sum[0] = sum[0] + x[k] * y[k];
    gn_block_sum(sum, part, buf);
    return sum[0];
}

/* A-A.  grid (keyframes / 256): every keyframe of the call */
__global__ __launch_bounds__(SS_GN_SLOTS) void k_gba_gather_kf(ssk_gba_call a)
{
    const int k = (int)blockIdx.x * SS_GN_SLOTS + (int)threadIdx.x;
    if (k >= a.n_kf) return;
    double R[9], t[3];
    const bool ok = ss_pose_start(a.start + (size_t)12 * k, R, t);
#pragma unroll
    for (int b = 0; b < 2; b++) {
        double *dst = a.pose + ((size_t)b * a.n_kf + k) * 12;
#pragma unroll
        for (int e = 0; e < 9; e++) dst[e] = R[e];
#pragma unroll
        for (int e = 0; e < 3; e++) dst[9 + e] = t[e];
    }
    a.kf_flag[k] = ok ? 1 : 0;
}

/* grid (blocks * pblocks): the flag of every point row, both buffers of the points, the records' bytes, the workgroup's counts */
__global__ __launch_bounds__(SS_GN_SLOTS) void k_gba_gather_points(ssk_gba_call a)
{
    __shared__ int part_n[2][4];
    const gba_lane l = gba_lane_of(a);
    int n_obs = 0, n_stereo = 0, n_active = 0, buf = 0;
    if (l.row < a.point_rows) {
        uint8_t flag = 2;
        double X[3] = {0.0, 0.0, 0.0};
        if (l.q >= 0) {
            const gba_prob pr = gba_prob_of(a, l.q);
            const int np = min(max(a.np[l.b], 0), a.point_rows);
            bool is_point = l.row < np && !(a.p_skip && a.p_skip[l.gp] != 0);
            if (is_point) {
                const ss_map_point p = a.points[l.gp];
                is_point = ss_gn_is_finite((double)p.x) && ss_gn_is_finite((double)p.y) && ss_gn_is_finite((double)p.z);
                if (is_point) X[0] = (double)p.x, X[1] = (double)p.y, X[2] = (double)p.z;
            }
            int off, cnt;
            gba_point_list(a, pr, l.gp, &off, &cnt);
            for (int j = 0; j < cnt; j++) {
                const size_t s = (size_t)pr.s0 + off + j;
                const ss_gba_rec r = a.rec[s];
                const bool good = r.valid != 0 && is_point;
                a.ob[s] = good ? 0 : 2;
                if (good) n_obs++, n_stereo += r.ur > 0.0f ? 1 : 0;
            }
            if (is_point) {
                flag = n_obs < a.p.min_point_obs ? 1 : 0;
                n_active = flag == 0 ? 1 : 0;
            }
        }
        a.pflag[l.gp] = flag;
        a.solved[l.gp] = 0;
#pragma unroll
        for (int e = 0; e < 3; e++) gba_X(a, 0, l.gp)[e] = X[e], gba_X(a, 1, l.gp)[e] = X[e];
    }
    n_obs = gn_block_sum(n_obs, part_n, &buf);
    n_stereo = gn_block_sum(n_stereo, part_n, &buf);
    n_active = gn_block_sum(n_active, part_n, &buf);
    if (threadIdx.x == 0) {
        int32_t *b = a.part + (size_t)blockIdx.x * 4;
        b[0] = n_obs, b[1] = n_stereo, b[2] = n_active, b[3] = 0;
    }
}

/* grid (problems): the counts of the problem's workgroups of points and of its keyframes, the state */
__global__ __launch_bounds__(SS_GN_SLOTS) void k_gba_gather_state(ssk_gba_call a)
{
    __shared__ int part_n[2][4];
    const int q = (int)blockIdx.x, tid = (int)threadIdx.x;
    const gba_prob pr = gba_prob_of(a, q);
    const int pb = gba_pblocks(a);
    int n_obs = 0, n_stereo = 0, n_active = 0, n_free = 0, n_bad = 0, buf = 0;
    for (int w = tid; w < pr.n_blocks * pb; w += SS_GN_SLOTS) {
        const int32_t *c = a.part + ((size_t)pr.b0 * pb + w) * 4;
        n_obs += c[0], n_stereo += c[1], n_active += c[2];
    }
    for (int k = tid; k < pr.n_kf; k += SS_GN_SLOTS) n_free += a.fixed[pr.k0 + k] ? 0 : 1, n_bad += a.kf_flag[pr.k0 + k] ? 0 : 1;
    n_obs = gn_block_sum(n_obs, part_n, &buf);
    n_stereo = gn_block_sum(n_stereo, part_n, &buf);
    n_active = gn_block_sum(n_active, part_n, &buf);
    n_free = gn_block_sum(n_free, part_n, &buf);
    n_bad = gn_block_sum(n_bad, part_n, &buf);
    if (tid != 0) return;
    ssk_gba_state s;
    s.lambda = a.p.lambda, s.cost0 = 0.0, s.cost_before = 0.0, s.rho = 0.0, s.stop = 0.0;
    s.state = n_bad > 0 ? 2 : (n_active == 0 || n_free == 0) ? 1 : 0;
    s.ended = s.state != 0 ? 1 : 0;
    s.round_over = 0, s.cur = 0, s.n_free = n_free;
    s.pcg_live = 0, s.pcg_done = 0, s.pcg_total = 0;
    s.n_obs = n_obs, s.n_stereo = n_stereo, s.n_frozen_max = 0, s.trial_ok = 0;
#pragma unroll
    for (int r = 0; r < 4; r++) s.steps[r] = 0, s.accepted[r] = 0;
    a.st[q] = s;
}

/* A-B.  grid (blocks * pblocks) */
__global__ __launch_bounds__(SS_GN_SLOTS) void k_gba_points(ssk_gba_call a, int round)
{
    __shared__ int part_n[2][4];
    const gba_lane l = gba_lane_of(a);
    if (l.q < 0 || !gba_running(a, l.q)) return; /* uniform */
    const gba_prob pr = gba_prob_of(a, l.q);
    const int cur = a.st[l.q].cur & 1;
    const double lambda = a.st[l.q].lambda;
    const bool robust = round < a.p.robust_rounds;
    int frozen = 0, buf = 0;
    if (l.row < a.point_rows) {
        const bool active = a.pflag[l.gp] == 0;
        double V[SS_BA_V] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, b[3] = {0.0, 0.0, 0.0};
        int off, cnt;
        gba_point_list(a, pr, l.gp, &off, &cnt);
        for (int j = 0; j < cnt; j++) {
            const size_t s = (size_t)pr.s0 + off + j;
            uint8_t took = 0;
            if (active && a.ob[s] == 0) {
                const ss_gba_rec r = a.rec[s];
                const int k = gba_rec_kf(pr, r);
                double R[9], t[3], tV[SS_BA_V], tb[3], tW[SS_BA_W];
                gba_load_pose(gba_pose(a, cur, k), R, t);
                if (ss_ba_lin(gba_obs(a, cur, l.gp, r), gba_cam(a, k), R, t, robust, tV, tb, tW)) {
                    took = 1;
#pragma unroll
                    for (int e = 0; e < SS_BA_V; e++) V[e] = V[e] + tV[e];
#pragma unroll
                    for (int e = 0; e < 3; e++) b[e] = b[e] + tb[e];
                    if (!a.fixed[k]) {
                        double *W = a.W + s * SS_BA_W;
#pragma unroll
                        for (int e = 0; e < SS_BA_W; e++) W[e] = tW[e];
                    }
                }
            }
            a.lin[s] = took;
        }
        uint8_t solved = 0;
        if (active) {
            double L[6];
            if (ss_ba_point_factor(V, b, lambda, L)) {
                solved = 1;
                double *dst = a.Lb + l.gp * 12;
#pragma unroll
                for (int e = 0; e < 6; e++) dst[e] = L[e];
#pragma unroll
                for (int e = 0; e < 3; e++) dst[6 + e] = b[e];
            } else {
                frozen = 1;
            }
        }
        a.solved[l.gp] = solved;
    }
    frozen = gn_block_sum(frozen, part_n, &buf);
    if (threadIdx.x == 0) a.part[(size_t)blockIdx.x * 4] = frozen;
}

/* A-C.  grid (keyframes): thread s is slot s of the 53 trees over the keyframe's list */
__global__ __launch_bounds__(SS_GN_SLOTS) void k_gba_blocks(ssk_gba_call a, int round)
{
    __shared__ double part[2][4][SS_GBA_SUMS];
    const int k = (int)blockIdx.x, tid = (int)threadIdx.x;
    const int q = a.kf_prob[k];
    if (q < 0 || q >= a.n_problems || !gba_running(a, q)) return; /* uniform */
    if (a.fixed[k]) {
        if (tid < 6) {
            const size_t o = (size_t)k * 6 + tid;
            a.x[o] = 0.0, a.r[o] = 0.0, a.z[o] = 0.0, a.pv[o] = 0.0, a.q[o] = 0.0;
        }
        if (tid == 0) a.kf_flag[k] = 1;
        return;
    }
    const gba_prob pr = gba_prob_of(a, q);
    const int cur = a.st[q].cur & 1;
    const double lambda = a.st[q].lambda;
    const bool robust = round < a.p.robust_rounds;
    double R[9], t[3];
    gba_load_pose(gba_pose(a, cur, k), R, t);
    const ss_pose_cam cam = gba_cam(a, k);
    double acc[SS_GBA_SUMS];
#pragma unroll
    for (int e = 0; e < SS_GBA_SUMS; e++) acc[e] = 0.0;
    int off, cnt;
    gba_kf_list(a, pr, k, &off, &cnt);
    for (int j = tid; j < cnt; j += SS_GN_SLOTS) {
        const size_t s = gba_kf_item(a, pr, off, j);
        if (!a.lin[s]) continue;
        const ss_gba_rec r = a.rec[s];
        const size_t gp = gba_rec_point(a, pr, r);
        const bool solved = a.solved[gp] != 0;
        double W[SS_BA_W], L[6], b[3], term[SS_GBA_SUMS];
        if (solved) {
#pragma unroll
            for (int e = 0; e < SS_BA_W; e++) W[e] = a.W[s * SS_BA_W + e];
#pragma unroll
            for (int e = 0; e < 6; e++) L[e] = a.Lb[gp * 12 + e];
#pragma unroll
            for (int e = 0; e < 3; e++) b[e] = a.Lb[gp * 12 + 6 + e];
        }
        ss_gba_block_terms(gba_obs(a, cur, gp, r), cam, R, t, robust, solved, W, L, b, term);
        if (solved) {
#pragma unroll
            for (int e = 0; e < SS_GBA_U; e++) acc[e] = acc[e] + term[e];
        }
#pragma unroll
        for (int e = SS_GBA_U; e < SS_GBA_SUMS; e++) acc[e] = acc[e] + term[e];
    }
    int buf = 0;
    gn_block_sum(acc, part, &buf);
    if (tid != 0) return;
    /* the block, its factor and the vectors of the solve in the workspace: run-time indices stay out of the registers */
    const size_t o = (size_t)k * 6;
    const bool ok = ss_gba_kf_block(acc, lambda, a.U + (size_t)k * SS_BA_DIAG, a.M + (size_t)k * 36, a.r + o);
#pragma unroll
    for (int e = 0; e < 6; e++) a.z[o + e] = a.r[o + e], a.x[o + e] = 0.0, a.q[o + e] = 0.0;
    ss_gn_subst_n(a.M + (size_t)k * 36, 6, 6, a.z + o);
#pragma unroll
    for (int e = 0; e < 6; e++) a.pv[o + e] = a.z[o + e];
    a.kf_flag[k] = ok ? 1 : 0;
}

/* grid (problems): the verdict of the blocks, the most frozen points, rho and the stop value of the solve */
__global__ __launch_bounds__(SS_GN_SLOTS) void k_gba_pcg_init(ssk_gba_call a)
{
    __shared__ double part[2][4][1];
    __shared__ int part_n[2][4];
    const int q = (int)blockIdx.x, tid = (int)threadIdx.x;
    if (!gba_running(a, q)) return; /* uniform */
    const gba_prob pr = gba_prob_of(a, q);
    const int pb = gba_pblocks(a);
    int bad = 0, frozen = 0, buf = 0, buf_n = 0;
    for (int k = tid; k < pr.n_kf; k += SS_GN_SLOTS) bad |= a.kf_flag[pr.k0 + k] ? 0 : 1;
    for (int w = tid; w < pr.n_blocks * pb; w += SS_GN_SLOTS) frozen += a.part[((size_t)pr.b0 * pb + w) * 4];
    frozen = gn_block_sum(frozen, part_n, &buf_n);
    const int any_bad = __syncthreads_or(bad);
    const size_t base = (size_t)pr.k0 * 6;
    const double rho = gba_dot(a.r + base, a.z + base, 6 * pr.n_kf, part, &buf);
    if (tid != 0) return;
    ssk_gba_state *s = a.st + q;
    s->n_frozen_max = max(s->n_frozen_max, frozen);
    s->pcg_done = 0;
    if (any_bad) {
        s->state = 2, s->ended = 1, s->pcg_live = 0;
        return;
    }
    s->rho = rho, s->stop = (a.p.pcg_tol * a.p.pcg_tol) * rho;
    s->pcg_live = 1;
}

/* A-D.  grid (blocks * pblocks): a_i and c_i of every solved point */
__global__ __launch_bounds__(SS_GN_SLOTS) void k_gba_pcg_points(ssk_gba_call a)
{
    const gba_lane l = gba_lane_of(a);
    if (l.q < 0 || !gba_running(a, l.q) || a.st[l.q].pcg_live == 0) return; /* uniform */
    if (l.row >= a.point_rows || !a.solved[l.gp]) return;
    const gba_prob pr = gba_prob_of(a, l.q);
    double c[3] = {0.0, 0.0, 0.0};
    int off, cnt;
    gba_point_list(a, pr, l.gp, &off, &cnt);
    for (int j = 0; j < cnt; j++) {
        const size_t s = (size_t)pr.s0 + off + j;
        if (!a.lin[s]) continue;
        const int k = gba_rec_kf(pr, a.rec[s]);
        if (a.fixed[k]) continue;
        double W[SS_BA_W], p[6];
#pragma unroll
        for (int e = 0; e < SS_BA_W; e++) W[e] = a.W[s * SS_BA_W + e];
#pragma unroll
        for (int e = 0; e < 6; e++) p[e] = a.pv[(size_t)k * 6 + e];
        ss_gba_wt_p(W, p, c);
    }
    double L[6];
#pragma unroll
    for (int e = 0; e < 6; e++) L[e] = a.Lb[l.gp * 12 + e];
    ss_ba_point_subst(L, c);
#pragma unroll
    for (int e = 0; e < 3; e++) a.Lb[l.gp * 12 + 9 + e] = c[e];
}

/* grid (keyframes): q_k of every free keyframe */
__global__ __launch_bounds__(SS_GN_SLOTS) void k_gba_pcg_kf(ssk_gba_call a)
{
    __shared__ double part[2][4][6];
    const int k = (int)blockIdx.x, tid = (int)threadIdx.x;
    const int q = a.kf_prob[k];
    if (q < 0 || q >= a.n_problems || !gba_running(a, q) || a.st[q].pcg_live == 0 || a.fixed[k]) return; /* uniform */
    const gba_prob pr = gba_prob_of(a, q);
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    int off, cnt;
    gba_kf_list(a, pr, k, &off, &cnt);
    for (int j = tid; j < cnt; j += SS_GN_SLOTS) {
        const size_t s = gba_kf_item(a, pr, off, j);
        if (!a.lin[s]) continue;
        const size_t gp = gba_rec_point(a, pr, a.rec[s]);
        if (!a.solved[gp]) continue;
        double W[SS_BA_W], c[3];
#pragma unroll
        for (int e = 0; e < SS_BA_W; e++) W[e] = a.W[s * SS_BA_W + e];
#pragma unroll
        for (int e = 0; e < 3; e++) c[e] = a.Lb[gp * 12 + 9 + e];
#pragma unroll
        for (int e = 0; e < 6; e++) acc[e] = acc[e] + ss_ba_yb_term(W, c, e);
    }
    int buf = 0;
    gn_block_sum(acc, part, &buf);
    if (tid != 0) return;
    double U[SS_BA_DIAG], p[6], up[6];
#pragma unroll
    for (int e = 0; e < SS_BA_DIAG; e++) U[e] = a.U[(size_t)k * SS_BA_DIAG + e];
#pragma unroll
    for (int e = 0; e < 6; e++) p[e] = a.pv[(size_t)k * 6 + e];
    ss_gba_u_p(U, p, up);
#pragma unroll
    for (int e = 0; e < 6; e++) a.q[(size_t)k * 6 + e] = up[e] - acc[e];
}

/* grid (problems): the rest of one iteration over the 6 n_kf vectors of the problem; a thread owns the keyframes tid, tid + 256, ... */
__global__ __launch_bounds__(SS_GN_SLOTS) void k_gba_pcg_step(ssk_gba_call a)
{
    __shared__ double part[2][4][1];
    const int q = (int)blockIdx.x, tid = (int)threadIdx.x;
    if (!gba_running(a, q) || a.st[q].pcg_live == 0) return; /* uniform */
    const gba_prob pr = gba_prob_of(a, q);
    const size_t base = (size_t)pr.k0 * 6;
    const int n6 = 6 * pr.n_kf;
    double *x = a.x + base, *r = a.r + base, *z = a.z + base, *p = a.pv + base;
    const double *qv = a.q + base;
    const double rho = a.st[q].rho, stop = a.st[q].stop;
    const int done = a.st[q].pcg_done;
    int buf = 0;
    const double pq = gba_dot(p, qv, n6, part, &buf); /* its barrier stands between every thread's reads of the state and thread 0's writes */
    if (!(pq > 0.0)) {
        if (tid == 0) a.st[q].pcg_live = 0;
        return;
    }
    const double alpha = rho / pq;
    for (int v = tid; v < pr.n_kf; v += SS_GN_SLOTS) {
#pragma unroll
        for (int e = 0; e < 6; e++) {
            const size_t o = (size_t)v * 6 + e;
            x[o] = x[o] + alpha * p[o], r[o] = r[o] - alpha * qv[o];
            z[o] = r[o];
        }
        if (!a.fixed[pr.k0 + v]) ss_gn_subst_n(a.M + (size_t)(pr.k0 + v) * 36, 6, 6, z + (size_t)v * 6);
    }
    __syncthreads();
    const double rho1 = gba_dot(r, z, n6, part, &buf);
    const bool leave = rho1 <= stop || done + 1 >= a.p.pcg_iterations;
    if (!leave) {
        const double beta = rho1 / rho;
        for (int v = tid; v < pr.n_kf; v += SS_GN_SLOTS) {
#pragma unroll
            for (int e = 0; e < 6; e++) p[(size_t)v * 6 + e] = z[(size_t)v * 6 + e] + beta * p[(size_t)v * 6 + e];
        }
    }
    if (tid != 0) return;
    a.st[q].pcg_done = done + 1;
    if (leave) a.st[q].pcg_live = 0;
    else a.st[q].rho = rho1;
}

/* A-E.  grid (keyframes / 256): the trial pose of every keyframe of a running problem into the other buffer */
__global__ __launch_bounds__(SS_GN_SLOTS) void k_gba_update_kf(ssk_gba_call a)
{
    const int k = (int)blockIdx.x * SS_GN_SLOTS + (int)threadIdx.x;
    if (k >= a.n_kf) return;
    const int q = a.kf_prob[k];
    if (q < 0 || q >= a.n_problems || !gba_running(a, q)) return;
    const int cur = a.st[q].cur & 1;
    double R[9], t[3];
    gba_load_pose(gba_pose(a, cur, k), R, t);
    bool small = true, large = false;
    if (!a.fixed[k]) {
        double dc[6];
#pragma unroll
        for (int e = 0; e < 6; e++) dc[e] = a.x[(size_t)k * 6 + e];
        if (!ss_ba_trial_pose(dc, a.p.step_eps, R, t, &small)) large = true, small = false;
    }
    const bool finite = ss_gn_all_finite(R, t);
    double *dst = a.pose + ((size_t)(cur ^ 1) * a.n_kf + k) * 12;
#pragma unroll
    for (int e = 0; e < 9; e++) dst[e] = R[e];
#pragma unroll
    for (int e = 0; e < 3; e++) dst[9 + e] = t[e];
    a.kf_flag[k] = (uint8_t)((finite ? 1 : 0) | (small ? 2 : 0) | (large ? 4 : 0));
}

/* grid (blocks * pblocks): back-substitution and the trial point */
__global__ __launch_bounds__(SS_GN_SLOTS) void k_gba_update_points(ssk_gba_call a)
{
    const gba_lane l = gba_lane_of(a);
    if (l.q < 0 || !gba_running(a, l.q)) return; /* uniform */
    const gba_prob pr = gba_prob_of(a, l.q);
    const int cur = a.st[l.q].cur & 1;
    bool small = true, finite = true;
    if (l.row < a.point_rows) {
        const double *Xc = gba_X(a, cur, l.gp);
        double X[3] = {Xc[0], Xc[1], Xc[2]};
        if (a.pflag[l.gp] == 0 && a.solved[l.gp]) {
            double L[6], v[3];
#pragma unroll
            for (int e = 0; e < 6; e++) L[e] = a.Lb[l.gp * 12 + e];
#pragma unroll
            for (int e = 0; e < 3; e++) v[e] = -a.Lb[l.gp * 12 + 6 + e];
            int off, cnt;
            gba_point_list(a, pr, l.gp, &off, &cnt);
            for (int j = 0; j < cnt; j++) {
                const size_t s = (size_t)pr.s0 + off + j;
                if (!a.lin[s]) continue;
                const int k = gba_rec_kf(pr, a.rec[s]);
                if (a.fixed[k]) continue;
                double W[SS_BA_W], dc[6];
#pragma unroll
                for (int e = 0; e < SS_BA_W; e++) W[e] = a.W[s * SS_BA_W + e];
#pragma unroll
                for (int e = 0; e < 6; e++) dc[e] = a.x[(size_t)k * 6 + e];
                ss_ba_point_rhs(W, dc, v);
            }
            ss_ba_point_subst(L, v);
#pragma unroll
            for (int e = 0; e < 3; e++) {
                X[e] = X[e] + v[e];
                small = small && fabs(v[e]) < a.p.step_eps;
                finite = finite && ss_gn_is_finite(X[e]);
            }
        }
        double *Xt = gba_X(a, cur ^ 1, l.gp);
        Xt[0] = X[0], Xt[1] = X[1], Xt[2] = X[2];
    }
    const int all_small = __syncthreads_and(small ? 1 : 0);
    const int all_finite = __syncthreads_and(finite ? 1 : 0);
    if (threadIdx.x == 0) {
        int32_t *b = a.part + (size_t)blockIdx.x * 4;
        b[1] = all_small, b[2] = all_finite;
    }
}

/* A-F.  grid (keyframes): the tree of keyframe k's chi-terms under the current (begin) or the trial state.  begin: the cost ahead
 * of a round's first step, which a round that is over does not keep from being formed */
__global__ __launch_bounds__(SS_GN_SLOTS) void k_gba_cost(ssk_gba_call a, int round, int begin)
{
    __shared__ double part[2][4][1];
    const int k = (int)blockIdx.x, tid = (int)threadIdx.x;
    const int q = a.kf_prob[k];
    if (q < 0 || q >= a.n_problems) return;
    if (begin ? a.st[q].ended != 0 : !gba_running(a, q)) return; /* uniform */
    const gba_prob pr = gba_prob_of(a, q);
    const int state = (a.st[q].cur & 1) ^ (begin ? 0 : 1);
    const bool robust = round < a.p.robust_rounds;
    double R[9], t[3];
    gba_load_pose(gba_pose(a, state, k), R, t);
    const ss_pose_cam cam = gba_cam(a, k);
    double sum[1] = {0.0};
    int off, cnt;
    gba_kf_list(a, pr, k, &off, &cnt);
    for (int j = tid; j < cnt; j += SS_GN_SLOTS) {
        const size_t s = gba_kf_item(a, pr, off, j);
        if (a.ob[s] != 0) continue;
        const ss_gba_rec r = a.rec[s];
        const size_t gp = gba_rec_point(a, pr, r);
        if (a.pflag[gp] != 0) continue;
        sum[0] = sum[0] + ss_ba_cost_term(gba_obs(a, state, gp, r), cam, R, t, robust);
    }
    int buf = 0;
    gn_block_sum(sum, part, &buf);
    if (tid == 0) a.cost_k[k] = sum[0];
}

/* grid (problems): the tree over the keyframes' costs, what the update kernels report, then thread 0 decides */
__global__ __launch_bounds__(SS_GN_SLOTS) void k_gba_accept(ssk_gba_call a, int round, int begin)
{
    __shared__ double part[2][4][1];
    const int q = (int)blockIdx.x, tid = (int)threadIdx.x;
    if (begin ? a.st[q].ended != 0 : !gba_running(a, q)) return; /* uniform */
    const gba_prob pr = gba_prob_of(a, q);
    const int pb = gba_pblocks(a);
    double sum[1] = {0.0};
    bool small = true, finite = true, large = false;
    for (int k = tid; k < pr.n_kf; k += SS_GN_SLOTS) {
        sum[0] = sum[0] + a.cost_k[pr.k0 + k];
        const uint8_t f = a.kf_flag[pr.k0 + k];
        finite = finite && (f & 1) != 0, small = small && (f & 2) != 0, large = large || (f & 4) != 0;
    }
    for (int w = tid; w < pr.n_blocks * pb; w += SS_GN_SLOTS) {
        const int32_t *c = a.part + ((size_t)pr.b0 * pb + w) * 4;
        small = small && c[1] != 0, finite = finite && c[2] != 0;
    }
    int buf = 0;
    gn_block_sum(sum, part, &buf); /* its barrier stands between every thread's reads of the state and thread 0's writes */
    const int all_small = __syncthreads_and(small ? 1 : 0);
    const int all_finite = __syncthreads_and(finite ? 1 : 0);
    const int any_large = __syncthreads_or(large ? 1 : 0);
    if (tid != 0) return;
    ssk_gba_state *s = a.st + q; /* updated in place: a copy indexed by the round would live in scratch */
    const double cost = sum[0];
    if (begin) {
        if (!ss_gn_is_finite(cost)) {
            s->state = 2, s->ended = 1;
            return;
        }
        s->cost0 = cost, s->round_over = 0;
        if (round == 0) s->cost_before = cost;
        return;
    }
    s->pcg_total = s->pcg_total + s->pcg_done;
    s->pcg_live = 0;
    if (any_large) {
        s->state = 4, s->ended = 1;
        return;
    }
    const bool accepted = all_finite != 0 && ss_gn_is_finite(cost) && cost <= s->cost0;
    const int r = min(max(round, 0), 3);
    s->steps[r] = s->steps[r] + 1;
    s->lambda = ss_ba_next_lambda(s->lambda, accepted, a.p.lambda_factor, a.p.lambda_min);
    if (!accepted) return;
    s->accepted[r] = s->accepted[r] + 1;
    s->cost0 = cost;
    s->cur = s->cur ^ 1;
    if (all_small) s->round_over = 1;
}

/* A-G.  grid (blocks * pblocks): after a round, under the current state */
__global__ __launch_bounds__(SS_GN_SLOTS) void k_gba_classify(ssk_gba_call a)
{
    const gba_lane l = gba_lane_of(a);
    if (l.q < 0 || a.st[l.q].ended != 0) return; /* uniform */
    if (l.row >= a.point_rows || a.pflag[l.gp] != 0) return;
    const gba_prob pr = gba_prob_of(a, l.q);
    const int cur = a.st[l.q].cur & 1;
    int n = 0, off, cnt;
    gba_point_list(a, pr, l.gp, &off, &cnt);
    for (int j = 0; j < cnt; j++) {
        const size_t s = (size_t)pr.s0 + off + j;
        if (a.ob[s] != 0) continue;
        const ss_gba_rec r = a.rec[s];
        const int k = gba_rec_kf(pr, r);
        double R[9], t[3];
        gba_load_pose(gba_pose(a, cur, k), R, t);
        const ss_pose_cam cam = gba_cam(a, k);
        const ss_pose_obs o = gba_obs(a, cur, l.gp, r);
        if (ss_pose_inlier(o, cam, ss_pose_chi2(o, cam, R, t))) n++;
        else a.ob[s] = 1;
    }
    if (n < a.p.min_point_obs) a.pflag[l.gp] = 1;
}

/* A-H.  grid (blocks * pblocks): the points out, the workgroup's counts */
__global__ __launch_bounds__(SS_GN_SLOTS) void k_gba_finish_points(ssk_gba_call a)
{
    __shared__ int part_n[2][4];
    const gba_lane l = gba_lane_of(a);
    int n_in = 0, n_act = 0, buf = 0;
    if (l.row < a.point_rows) {
        const uint8_t flag = a.pflag[l.gp];
        const int cur = l.q >= 0 ? (a.st[l.q].cur & 1) : 0;
        const double *X = gba_X(a, cur, l.gp);
        double *out = a.out_xyz + l.gp * 3;
#pragma unroll
        for (int e = 0; e < 3; e++) out[e] = flag == 2 ? 0.0 : X[e];
        a.out_pflag[l.gp] = flag;
        n_act = flag == 0 ? 1 : 0;
        if (l.q >= 0) {
            const gba_prob pr = gba_prob_of(a, l.q);
            int off, cnt;
            gba_point_list(a, pr, l.gp, &off, &cnt);
            for (int j = 0; j < cnt; j++) n_in += a.ob[(size_t)pr.s0 + off + j] == 0 ? 1 : 0;
        }
    }
    n_in = gn_block_sum(n_in, part_n, &buf);
    n_act = gn_block_sum(n_act, part_n, &buf);
    if (threadIdx.x == 0) {
        int32_t *b = a.part + (size_t)blockIdx.x * 4;
        b[0] = n_in, b[3] = n_act;
    }
}

/* grid (records / 256): every record's byte in the caller's order */
__global__ __launch_bounds__(SS_GN_SLOTS) void k_gba_finish_obs(ssk_gba_call a)
{
    const int s = (int)blockIdx.x * SS_GN_SLOTS + (int)threadIdx.x;
    if (s >= a.n_obs) return;
    const ss_gba_rec r = a.rec[s];
    a.out_obs[min(max(r.orig, 0), a.n_obs - 1)] = r.kf < 0 ? 2 : a.ob[s];
}

/* grid (keyframes / 256): every keyframe's pose */
__global__ __launch_bounds__(SS_GN_SLOTS) void k_gba_finish_kf(ssk_gba_call a)
{
    const int k = (int)blockIdx.x * SS_GN_SLOTS + (int)threadIdx.x;
    if (k >= a.n_kf) return;
    const int q = a.kf_prob[k];
    const int buf = (q >= 0 && q < a.n_problems) ? (a.st[q].cur & 1) : 0;
    const double *src = gba_pose(a, buf, k);
#pragma unroll
    for (int e = 0; e < 12; e++) a.out_pose[(size_t)k * 12 + e] = src[e];
}

/* grid (problems): the result */
__global__ __launch_bounds__(SS_GN_SLOTS) void k_gba_finish_state(ssk_gba_call a)
{
    __shared__ int part_n[2][4];
    const int q = (int)blockIdx.x, tid = (int)threadIdx.x;
    const gba_prob pr = gba_prob_of(a, q);
    const int pb = gba_pblocks(a);
    int n_in = 0, n_act = 0, buf = 0;
    for (int w = tid; w < pr.n_blocks * pb; w += SS_GN_SLOTS) {
        const int32_t *c = a.part + ((size_t)pr.b0 * pb + w) * 4;
        n_in += c[0], n_act += c[3];
    }
    n_in = gn_block_sum(n_in, part_n, &buf);
    n_act = gn_block_sum(n_act, part_n, &buf);
    if (tid != 0) return;
    const ssk_gba_state s = a.st[q];
    ss_gba_result r;
    r.lambda = s.lambda, r.cost_before = s.cost_before, r.cost_after = s.cost0;
    r.state = s.state, r.status = 0;
    r.n_obs = s.n_obs, r.n_stereo = s.n_stereo, r.n_inliers = n_in, r.n_points_active = n_act, r.n_frozen_max = s.n_frozen_max;
#pragma unroll
    for (int k = 0; k < 4; k++) r.steps[k] = s.steps[k], r.accepted[k] = s.accepted[k];
    r.pcg_iterations = s.pcg_total, r.n_free = s.n_free, r.n_fixed = pr.n_kf - s.n_free;
    r.reserved[0] = 0, r.reserved[1] = 0;
    a.result[q] = r;
}

inline unsigned blocks_of(int n, int per) { return (unsigned)((n + per - 1) / per); }

/* the workgroups of a per-point kernel: 0 when the call has no block of points */
inline unsigned point_groups(const ssk_gba_call &g) { return (unsigned)g.n_blocks * blocks_of(g.point_rows, SS_GN_SLOTS); }

} // namespace

void ssk_gba_gather(hipStream_t s, const ssk_gba_call &g)
{
    hipLaunchKernelGGL(k_gba_gather_kf, dim3(blocks_of(g.n_kf, SS_GN_SLOTS)), dim3(SS_GN_SLOTS), 0, s, g);
    if (point_groups(g)) hipLaunchKernelGGL(k_gba_gather_points, dim3(point_groups(g)), dim3(SS_GN_SLOTS), 0, s, g);
    hipLaunchKernelGGL(k_gba_gather_state, dim3((unsigned)g.n_problems), dim3(SS_GN_SLOTS), 0, s, g);
}

void ssk_gba_cost(hipStream_t s, const ssk_gba_call &g, int round, int begin)
{
    hipLaunchKernelGGL(k_gba_cost, dim3((unsigned)g.n_kf), dim3(SS_GN_SLOTS), 0, s, g, round, begin);
    hipLaunchKernelGGL(k_gba_accept, dim3((unsigned)g.n_problems), dim3(SS_GN_SLOTS), 0, s, g, round, begin);
}

void ssk_gba_points(hipStream_t s, const ssk_gba_call &g, int round)
{
    if (point_groups(g)) hipLaunchKernelGGL(k_gba_points, dim3(point_groups(g)), dim3(SS_GN_SLOTS), 0, s, g, round);
}

void ssk_gba_blocks(hipStream_t s, const ssk_gba_call &g, int round)
{
    hipLaunchKernelGGL(k_gba_blocks, dim3((unsigned)g.n_kf), dim3(SS_GN_SLOTS), 0, s, g, round);
    hipLaunchKernelGGL(k_gba_pcg_init, dim3((unsigned)g.n_problems), dim3(SS_GN_SLOTS), 0, s, g);
}

void ssk_gba_pcg(hipStream_t s, const ssk_gba_call &g)
{
    if (point_groups(g)) hipLaunchKernelGGL(k_gba_pcg_points, dim3(point_groups(g)), dim3(SS_GN_SLOTS), 0, s, g);
    hipLaunchKernelGGL(k_gba_pcg_kf, dim3((unsigned)g.n_kf), dim3(SS_GN_SLOTS), 0, s, g);
    hipLaunchKernelGGL(k_gba_pcg_step, dim3((unsigned)g.n_problems), dim3(SS_GN_SLOTS), 0, s, g);
}

void ssk_gba_update(hipStream_t s, const ssk_gba_call &g)
{
    hipLaunchKernelGGL(k_gba_update_kf, dim3(blocks_of(g.n_kf, SS_GN_SLOTS)), dim3(SS_GN_SLOTS), 0, s, g);
    if (point_groups(g)) hipLaunchKernelGGL(k_gba_update_points, dim3(point_groups(g)), dim3(SS_GN_SLOTS), 0, s, g);
}

void ssk_gba_classify(hipStream_t s, const ssk_gba_call &g)
{
    if (point_groups(g)) hipLaunchKernelGGL(k_gba_classify, dim3(point_groups(g)), dim3(SS_GN_SLOTS), 0, s, g);
}

void ssk_gba_finish(hipStream_t s, const ssk_gba_call &g)
{
    if (point_groups(g)) hipLaunchKernelGGL(k_gba_finish_points, dim3(point_groups(g)), dim3(SS_GN_SLOTS), 0, s, g);
    if (g.n_obs > 0) hipLaunchKernelGGL(k_gba_finish_obs, dim3(blocks_of(g.n_obs, SS_GN_SLOTS)), dim3(SS_GN_SLOTS), 0, s, g);
    hipLaunchKernelGGL(k_gba_finish_kf, dim3(blocks_of(g.n_kf, SS_GN_SLOTS)), dim3(SS_GN_SLOTS), 0, s, g);
    if (g.n_problems > 0) hipLaunchKernelGGL(k_gba_finish_state, dim3((unsigned)g.n_problems), dim3(SS_GN_SLOTS), 0, s, g);
}
