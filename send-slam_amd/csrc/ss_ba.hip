/*
 * ss_ba.hip -- local bundle adjustment: the Schur-reduced Levenberg-Marquardt of Optimizer::LocalBundleAdjustment for every local
 * map (problem) of a call at once (the rule: include/sendslam_orb.h; DESIGN.md "Local bundle adjustment").  Every step of the
 * arithmetic is the text of ss_ba_steps.h, which the host twin compiles too.
 *
 * The host enqueues the fixed schedule of every round and iteration without a round trip; a problem's state (ssk_ba_state) lives
 * in device memory, and a kernel whose problem has ended, or whose round is over, returns at once.
 *
 *   B-A  k_ba_gather, k_ba_gather_points, k_ba_gather_state   the observations' measurements and bytes, the points widened and
 *                       their flags, the start poses and the problem's state
 *   B-B  k_ba_points    one lane per point over (points, problems): V, b and the W of every free keyframe in ascending k, the
 *                       factor of V, Y = W.V^-1; W and Y go to the workspace as planes over the points
 *   B-C  k_ba_blocks    one workgroup of SS_GN_SLOTS threads per block (k, l), k <= l, and problem; thread s is slot s of the tree
 *                       and reads the W and Y of its points for k and l straight from their planes (the dense lin bytes say which
 *                       exist).  A diagonal block sums U, g and Y.b as well
 *   B-D  k_ba_solve     one workgroup per problem: S's triangle into LDS, Cholesky by columns there, one thread per row of a column,
 *                       the two triangular solves, the trial poses
 *   B-E  k_ba_update    per point: back-substitution and the trial point
 *   B-F  k_ba_cost      one workgroup per keyframe and problem: the tree of its chi-terms
 *   B-G  k_ba_accept    one thread per problem: the sum over the keyframes, accept or reject, lambda, the end of a round
 *   B-H  k_ba_classify  per point after a round
 *   B-I  k_ba_finish_points, k_ba_finish   the outputs
 *
 * Every floating-point step is a single IEEE operation (-ffp-contract=off).  Every global write is a plain vector store; there are
 * no atomics.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ss_ba_steps.h"
#include "ss_constants.h"
#include "ss_gn.h"
#include "ss_kernels.h"

namespace {

static_assert(SS_GN_SLOTS == 256, "four waves, one group of 64 slots each");
static_assert(6 * SS_BA_MAX_FREE <= SS_GN_SLOTS, "k_ba_solve: one thread per row");
static_assert(SS_BA_MAX_KF <= 64, "k_ba_gather_state: one thread per keyframe in one wave");
static_assert(sizeof(ss_ba_result) == 88 && sizeof(ss_ba_params) == 96 && sizeof(ss_ba_problem) == 16, "the layouts of the header");
static_assert(sizeof(ssk_ba_meas) == sizeof(ss_ba_meas), "one layout");

#define BA_NS_DIAG (SS_BA_DIAG + 6 + SS_POSE_SUMS)

struct ba_prob {
    int f0, n_kf, n_free, pb;
};

/* the host has checked the table: the clamps only keep a stray value inside the arrays */
__device__ __forceinline__ ba_prob ba_prob_of(const ssk_ba_call &a, int q)
{
    const ss_ba_problem p = a.prob[q];
    ba_prob r;
    r.n_kf = min(max(p.n_kf, 1), min(a.max_kf, a.n_frames));
    r.n_free = min(max(p.n_free, 1), min(a.max_free, r.n_kf));
    r.f0 = min(max(p.first_frame, 0), a.n_frames - r.n_kf);
    r.pb = p.point_block;
    return r;
}

__device__ __forceinline__ bool ba_running(const ssk_ba_call &a, int q) { return a.st[q].ended == 0 && a.st[q].round_over == 0; }

__device__ __forceinline__ int ba_pblocks(const ssk_ba_call &a) { return (a.point_rows + SS_GN_SLOTS - 1) / SS_GN_SLOTS; }

/* the first frame_error of the problem's frames in ascending order, or 0 */
__device__ __forceinline__ int ba_status(const ssk_ba_call &a, const ba_prob &pr)
{
    int status = 0;
    if (a.frame_error)
        for (int k = 0; k < pr.n_kf; k++)
            if (status == 0) status = a.frame_error[pr.f0 + k];
    return status;
}

__device__ __forceinline__ bool ba_is_point(const ssk_ba_call &a, const ba_prob &pr, int status, int i, ss_map_point *out)
{
    const int np = min(max(a.np[pr.pb], 0), a.point_rows);
    if (status != 0 || !(i < np)) return false;
    const size_t o = (size_t)pr.pb * a.point_rows + i;
    if (a.p_skip && a.p_skip[o] != 0) return false;
    const ss_map_point p = a.points[o];
    *out = p;
    return ss_gn_is_finite((double)p.x) && ss_gn_is_finite((double)p.y) && ss_gn_is_finite((double)p.z);
}

/* the poses (buffer `buf`) and cameras of a problem's keyframes into LDS; one barrier */
__device__ __forceinline__ void ba_stage(const ssk_ba_call &a, const ba_prob &pr, int buf, double (*s_pose)[12], ss_pose_cam *s_cam)
{
    for (int k = (int)threadIdx.x; k < pr.n_kf; k += (int)blockDim.x) {
        const double *src = a.pose + ((size_t)buf * a.n_frames + pr.f0 + k) * 12;
#pragma unroll
        for (int e = 0; e < 12; e++) s_pose[k][e] = src[e];
        s_cam[k] = ss_pose_cam_of(a.views[pr.f0 + k], a.p.chi2_mono, a.p.chi2_stereo);
    }
    __syncthreads();
}

__device__ __forceinline__ ss_pose_obs ba_obs(const ssk_ba_call &a, const double *Xq, int f, int i)
{
    const ssk_ba_meas m = a.meas[(size_t)f * a.point_rows + i];
    ss_ba_meas mm;
    mm.u = m.u, mm.v = m.v, mm.ur = m.ur, mm.scale = m.scale;
    const double X[3] = {Xq[(size_t)i * 3], Xq[(size_t)i * 3 + 1], Xq[(size_t)i * 3 + 2]};
    return ss_ba_obs_of(X, mm);
}

__device__ __forceinline__ double *ba_X(const ssk_ba_call &a, int buf, int q) { return a.X + ((size_t)buf * a.n_problems + q) * a.point_rows * 3; }

/* plane e of W (e < 18) and Y (18 <= e < 36) of free keyframe k of problem q */
__device__ __forceinline__ double *ba_wy(const ssk_ba_call &a, int q, int k, int e)
{
    return a.WY + (((size_t)q * a.max_free + k) * 36 + e) * a.point_rows;
}

__device__ __forceinline__ double *ba_lb(const ssk_ba_call &a, int q, int e) { return a.Lb + ((size_t)q * 9 + e) * a.point_rows; }

/* B-A.  grid (pblocks, frames): the measurement and the byte of every (frame, point row) */
__global__ __launch_bounds__(SS_GN_SLOTS) void k_ba_gather(ssk_ba_call a)
{
    const int f = (int)blockIdx.y, i = (int)blockIdx.x * SS_GN_SLOTS + (int)threadIdx.x;
    if (i >= a.point_rows) return;
    const size_t o = (size_t)f * a.point_rows + i;
    const int q = a.frame_prob[f];
    uint8_t byte = 2;
    ssk_ba_meas m = {0.0f, 0.0f, -1.0f, 1.0f};
    if (q >= 0 && q < a.n_problems) {
        const ba_prob pr = ba_prob_of(a, q);
        ss_map_point pt;
        if (ba_is_point(a, pr, ba_status(a, pr), i, &pt)) {
            const int nk = min(max(a.nk[f], 0), a.rows), krow = a.idx[o];
            if (krow >= 0 && krow < nk) {
                const ss_keypoint kp = a.kp[(size_t)f * a.rows + krow];
                const int n_levels = min(max(a.n_levels, 1), SS_MAX_LEVELS);
                if (kp.octave >= 0 && kp.octave < n_levels) {
                    const float right = a.right ? a.right[(size_t)f * a.rows + krow] : 0.0f;
                    m.u = kp.x, m.v = kp.y, m.ur = ss_pose_stored_right(a.p.check_right != 0, a.right != nullptr, right), m.scale = a.scale[kp.octave];
                    byte = 0;
                }
            }
        }
    }
    a.meas[o] = m;
    a.obs[o] = byte;
}

/* grid (pblocks, problems): the flag of every point row, both buffers of the points, the workgroup's counts */
__global__ __launch_bounds__(SS_GN_SLOTS) void k_ba_gather_points(ssk_ba_call a)
{
    __shared__ int part_n[2][4];
    const int q = (int)blockIdx.y, i = (int)blockIdx.x * SS_GN_SLOTS + (int)threadIdx.x;
    const ba_prob pr = ba_prob_of(a, q);
    int n_obs = 0, n_stereo = 0, n_active = 0, buf = 0;
    if (i < a.point_rows) {
        ss_map_point pt;
        const bool is_point = ba_is_point(a, pr, ba_status(a, pr), i, &pt);
        uint8_t flag = 2;
        double X[3] = {0.0, 0.0, 0.0};
        if (is_point) {
            X[0] = (double)pt.x, X[1] = (double)pt.y, X[2] = (double)pt.z;
            for (int k = 0; k < pr.n_kf; k++) {
                const size_t o = (size_t)(pr.f0 + k) * a.point_rows + i;
                if (a.obs[o] == 0) n_obs++, n_stereo += a.meas[o].ur > 0.0f ? 1 : 0;
            }
            flag = n_obs < a.p.min_point_obs ? 1 : 0;
            n_active = flag == 0 ? 1 : 0;
        }
        a.pflag[(size_t)q * a.point_rows + i] = flag;
#pragma unroll
        for (int e = 0; e < 3; e++) ba_X(a, 0, q)[(size_t)i * 3 + e] = X[e], ba_X(a, 1, q)[(size_t)i * 3 + e] = X[e];
    }
    n_obs = gn_block_sum(n_obs, part_n, &buf);
    n_stereo = gn_block_sum(n_stereo, part_n, &buf);
    n_active = gn_block_sum(n_active, part_n, &buf);
    if (threadIdx.x == 0) {
        int32_t *b = a.blk + ((size_t)q * ba_pblocks(a) + blockIdx.x) * 4;
        b[0] = n_obs, b[1] = n_stereo, b[2] = n_active, b[3] = 0;
    }
}

/* grid (problems), 64 threads: the start poses into both buffers, the state */
__global__ __launch_bounds__(64) void k_ba_gather_state(ssk_ba_call a)
{
    const int q = (int)blockIdx.x, k = (int)threadIdx.x;
    const ba_prob pr = ba_prob_of(a, q);
    bool ok = true;
    if (k < pr.n_kf) {
        double R[9], t[3];
        ok = ss_pose_start(a.start + (size_t)12 * (pr.f0 + k), R, t);
#pragma unroll
        for (int b = 0; b < 2; b++) {
            double *dst = a.pose + ((size_t)b * a.n_frames + pr.f0 + k) * 12;
#pragma unroll
            for (int e = 0; e < 9; e++) dst[e] = R[e];
#pragma unroll
            for (int e = 0; e < 3; e++) dst[9 + e] = t[e];
        }
    }
    const bool all_ok = __syncthreads_and(ok ? 1 : 0) != 0;
    if (k != 0) return;
    int n_obs = 0, n_stereo = 0, n_active = 0;
    for (int b = 0; b < ba_pblocks(a); b++) {
        const int32_t *c = a.blk + ((size_t)q * ba_pblocks(a) + b) * 4;
        n_obs += c[0], n_stereo += c[1], n_active += c[2];
    }
    const int status = ba_status(a, pr);
    ssk_ba_state s;
    s.lambda = a.p.lambda, s.cost0 = 0.0, s.cost_before = 0.0;
    s.state = !all_ok ? 2 : n_active == 0 ? 1 : 0;
    s.status = status;
    s.ended = s.state != 0 ? 1 : 0;
    s.round_over = 0, s.cur = 0, s.pose_small = 0, s.pose_finite = 0;
    s.n_obs = n_obs, s.n_stereo = n_stereo, s.n_frozen_max = 0;
#pragma unroll
    for (int r = 0; r < 4; r++) s.steps[r] = 0, s.accepted[r] = 0;
    a.st[q] = s;
}

/* B-B.  grid (pblocks, problems) */
__global__ __launch_bounds__(SS_GN_SLOTS) void k_ba_points(ssk_ba_call a, int round)
{
    __shared__ double s_pose[SS_BA_MAX_KF][12];
    __shared__ ss_pose_cam s_cam[SS_BA_MAX_KF];
    __shared__ int part_n[2][4];
    const int q = (int)blockIdx.y, i = (int)blockIdx.x * SS_GN_SLOTS + (int)threadIdx.x, P = a.point_rows;
    if (!ba_running(a, q)) return; /* uniform */
    const ba_prob pr = ba_prob_of(a, q);
    const int cur = a.st[q].cur & 1;
    const double lambda = a.st[q].lambda;
    const bool robust = round < a.p.robust_rounds;
    ba_stage(a, pr, cur, s_pose, s_cam);
    int frozen = 0, buf = 0;
    if (i < P) {
        const bool active = a.pflag[(size_t)q * P + i] == 0;
        double V[SS_BA_V] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, b[3] = {0.0, 0.0, 0.0};
        unsigned long long took = 0ull; /* bit k: the observation in keyframe k took part */
        for (int k = 0; k < pr.n_kf; k++) {
            const size_t o = (size_t)(pr.f0 + k) * P + i;
            bool part = false;
            if (active && a.obs[o] == 0) {
                double tV[SS_BA_V], tb[3], tW[SS_BA_W];
                part = ss_ba_lin(ba_obs(a, ba_X(a, cur, q), pr.f0 + k, i), s_cam[k], s_pose[k], s_pose[k] + 9, robust, tV, tb, tW);
                if (part) {
#pragma unroll
                    for (int e = 0; e < SS_BA_V; e++) V[e] = V[e] + tV[e];
#pragma unroll
                    for (int e = 0; e < 3; e++) b[e] = b[e] + tb[e];
                    if (k < pr.n_free) {
#pragma unroll
                        for (int e = 0; e < SS_BA_W; e++) ba_wy(a, q, k, e)[i] = tW[e];
                    }
                    took |= 1ull << k;
                }
            }
            a.lin[o] = part ? 1 : 0;
        }
        uint8_t solved = 0;
        if (active) {
            double L[6];
            if (ss_ba_point_factor(V, b, lambda, L)) {
                solved = 1;
#pragma unroll
                for (int e = 0; e < 6; e++) ba_lb(a, q, e)[i] = L[e];
#pragma unroll
                for (int e = 0; e < 3; e++) ba_lb(a, q, 6 + e)[i] = b[e];
                for (int k = 0; k < pr.n_free; k++) {
                    if (!((took >> k) & 1ull)) continue;
                    double W[SS_BA_W], Y[SS_BA_W];
#pragma unroll
                    for (int e = 0; e < SS_BA_W; e++) W[e] = ba_wy(a, q, k, e)[i];
                    ss_ba_coupling(L, W, Y);
#pragma unroll
                    for (int e = 0; e < SS_BA_W; e++) ba_wy(a, q, k, SS_BA_W + e)[i] = Y[e];
                }
            } else {
                frozen = 1;
            }
        }
        a.solved[(size_t)q * P + i] = solved;
    }
    frozen = gn_block_sum(frozen, part_n, &buf);
    if (threadIdx.x == 0) a.blk[((size_t)q * ba_pblocks(a) + blockIdx.x) * 4] = frozen;
}

/* the sums of one block of the reduced system in the tree order */
template <bool DIAG>
__device__ __forceinline__ void ba_block(const ssk_ba_call &a, const ba_prob &pr, int q, int k, int l, bool robust, double lambda, const double *Xq,
                                         const double *pose_k, const ss_pose_cam &cam_k)
{
    constexpr int NS = DIAG ? BA_NS_DIAG : 36;
    __shared__ double part[2][4][NS];
    const int P = a.point_rows, tid = (int)threadIdx.x, n = 6 * pr.n_free;
    const uint8_t *lin_k = a.lin + (size_t)(pr.f0 + k) * P, *lin_l = a.lin + (size_t)(pr.f0 + l) * P, *solved = a.solved + (size_t)q * P;
    double sum[NS];
#pragma unroll
    for (int e = 0; e < NS; e++) sum[e] = 0.0;
    for (int i = tid; i < P; i += SS_GN_SLOTS) {
        if (!lin_k[i] || !lin_l[i]) continue;
        if (solved[i]) {
            double Y[SS_BA_W], W[SS_BA_W];
#pragma unroll
            for (int e = 0; e < SS_BA_W; e++) Y[e] = ba_wy(a, q, k, SS_BA_W + e)[i], W[e] = ba_wy(a, q, l, e)[i];
#pragma unroll
            for (int r = 0; r < 6; r++) {
#pragma unroll
                for (int c = DIAG ? r : 0; c < 6; c++) {
                    const int m = DIAG ? 6 * r - (r * (r - 1)) / 2 + (c - r) : 6 * r + c;
                    sum[m] = sum[m] + ss_ba_c_term(Y, W, r, c);
                }
            }
            if constexpr (DIAG) {
                const double b[3] = {ba_lb(a, q, 6)[i], ba_lb(a, q, 7)[i], ba_lb(a, q, 8)[i]};
#pragma unroll
                for (int r = 0; r < 6; r++) sum[SS_BA_DIAG + r] = sum[SS_BA_DIAG + r] + ss_ba_yb_term(Y, b, r);
            }
        }
        if constexpr (DIAG) {
            double term[SS_POSE_SUMS];
            if (ss_pose_terms(ba_obs(a, Xq, pr.f0 + k, i), cam_k, pose_k, pose_k + 9, robust, term)) {
#pragma unroll
                for (int e = 0; e < SS_POSE_SUMS; e++) sum[SS_BA_DIAG + 6 + e] = sum[SS_BA_DIAG + 6 + e] + term[e];
            }
        }
    }
    int buf = 0;
    gn_block_sum(sum, part, &buf);
    if (tid != 0) return;
    double *A = a.A + (size_t)q * (6 * a.max_free) * (6 * a.max_free);
    if constexpr (DIAG) {
        double U[SS_BA_DIAG], g[6];
        ss_ba_unpack_u(sum + SS_BA_DIAG + 6, lambda, U, g);
#pragma unroll
        for (int r = 0; r < 6; r++) {
#pragma unroll
            for (int c = r; c < 6; c++) {
                const int m = 6 * r - (r * (r - 1)) / 2 + (c - r);
                A[(size_t)(6 * k + r) * n + 6 * k + c] = U[m] - sum[m];
            }
        }
#pragma unroll
        for (int r = 0; r < 6; r++) a.r[(size_t)q * 6 * a.max_free + 6 * k + r] = g[r] - sum[SS_BA_DIAG + r];
    } else {
#pragma unroll
        for (int r = 0; r < 6; r++) {
#pragma unroll
            for (int c = 0; c < 6; c++) A[(size_t)(6 * k + r) * n + 6 * l + c] = 0.0 - sum[6 * r + c];
        }
    }
}

/* B-C.  grid (max_free (max_free + 1) / 2, problems) */
__global__ __launch_bounds__(SS_GN_SLOTS) void k_ba_blocks(ssk_ba_call a, int round)
{
    __shared__ double s_pose[12];
    __shared__ ss_pose_cam s_cam;
    const int q = (int)blockIdx.y;
    if (!ba_running(a, q)) return; /* uniform */
    const ba_prob pr = ba_prob_of(a, q);
    int k = 0, rem = (int)blockIdx.x;
    if (rem >= pr.n_free * (pr.n_free + 1) / 2) return;
    while (k < pr.n_free - 1 && rem >= pr.n_free - k) rem -= pr.n_free - k, k++; /* rem started below the number of pairs */
    const int l = k + rem, cur = a.st[q].cur & 1;
    const bool robust = round < a.p.robust_rounds;
    const double lambda = a.st[q].lambda;
    if (k != l) {
        ba_block<false>(a, pr, q, k, l, robust, lambda, nullptr, nullptr, s_cam);
        return;
    }
    if (threadIdx.x == 0) {
        const double *src = a.pose + ((size_t)cur * a.n_frames + pr.f0 + k) * 12;
#pragma unroll
        for (int e = 0; e < 12; e++) s_pose[e] = src[e];
        s_cam = ss_pose_cam_of(a.views[pr.f0 + k], a.p.chi2_mono, a.p.chi2_stereo);
    }
    __syncthreads();
    ba_block<true>(a, pr, q, k, k, robust, lambda, ba_X(a, cur, q), s_pose, s_cam);
}

/* B-D.  grid (problems), SS_GN_SLOTS threads.  The upper triangle of S is copied into the workgroup's dynamic LDS, packed row by row
 * (row r: its n - r entries from the diagonal on; order 192: 148 224 bytes), and factored there; it holds the factor afterwards:
 * L[i][k] = U[k][i], so thread i walks consecutive addresses.  Column j: thread i >= j subtracts the columns k < j in ascending
 * order, the thread of the pivot stores its square root, the others divide: the text of ss_gn_chol_n, its rows in parallel */
__global__ __launch_bounds__(SS_GN_SLOTS) void k_ba_solve(ssk_ba_call a)
{
    extern __shared__ double s_tri[];
    __shared__ double d[6 * SS_BA_MAX_FREE], prod[6 * SS_BA_MAX_FREE];
    __shared__ int s_bad;
    const int q = (int)blockIdx.x, tid = (int)threadIdx.x;
    if (!ba_running(a, q)) return; /* uniform */
    const ba_prob pr = ba_prob_of(a, q);
    const int n = 6 * pr.n_free, cur = a.st[q].cur & 1;
    const double *G = a.A + (size_t)q * (6 * a.max_free) * (6 * a.max_free);
    /* entry (r, c), r <= c, of the upper triangle */
    auto U = [&](int r, int c) -> double & { return s_tri[r * n - (r * (r - 1)) / 2 + (c - r)]; };
    if (tid == 0) {
        s_bad = 0;
        int frozen = 0;
        for (int b = 0; b < ba_pblocks(a); b++) frozen += a.blk[((size_t)q * ba_pblocks(a) + b) * 4];
        if (frozen > a.st[q].n_frozen_max) a.st[q].n_frozen_max = frozen;
    }
    if (tid < n) d[tid] = -a.r[(size_t)q * 6 * a.max_free + tid];
    for (int r = 0; r < n; r++)
        if (tid >= r && tid < n) U(r, tid) = G[(size_t)r * n + tid];
    __syncthreads();
    for (int j = 0; j < n; j++) {
        double v = 0.0;
        if (tid >= j && tid < n) {
            v = U(j, tid);
            for (int k = 0; k < j; k++) v = v - U(k, tid) * U(k, j);
            if (tid == j) {
                if (!(v > 0.0)) s_bad = 1;
                U(j, j) = sqrt(v);
            }
        }
        __syncthreads();
        if (tid > j && tid < n) U(j, tid) = v / U(j, j);
        __syncthreads();
    }
    if (s_bad) { /* uniform: written before the last barrier */
        if (tid == 0) a.st[q].state = 2, a.st[q].ended = 1;
        return;
    }
    /* forward: d_k is final once the columns before it are taken off; then every later row takes column k off */
    for (int k = 0; k < n; k++) {
        if (tid == k) d[k] = d[k] / U(k, k);
        __syncthreads();
        if (tid > k && tid < n) d[tid] = d[tid] - U(k, tid) * d[k];
    }
    __syncthreads();
    /* backward: row i needs its products in ascending k, so they are formed in parallel and one thread subtracts them in order */
    for (int i = n - 1; i >= 0; i--) {
        if (tid > i && tid < n) prod[tid] = U(i, tid) * d[tid];
        __syncthreads();
        if (tid == 0) {
            double v = d[i];
#pragma unroll 8
            for (int k = i + 1; k < n; k++) v = v - prod[k];
            d[i] = v / U(i, i);
        }
        __syncthreads();
    }
    if (tid < n) a.dc[(size_t)q * 6 * a.max_free + tid] = d[tid];
    /* the trial poses of the free keyframes into the other buffer */
    bool large = false, small = true, finite = true;
    if (tid < pr.n_free) {
        const double *src = a.pose + ((size_t)cur * a.n_frames + pr.f0 + tid) * 12;
        double *dst = a.pose + ((size_t)(cur ^ 1) * a.n_frames + pr.f0 + tid) * 12;
        double R[9], t[3], dc[6];
#pragma unroll
        for (int e = 0; e < 9; e++) R[e] = src[e];
#pragma unroll
        for (int e = 0; e < 3; e++) t[e] = src[9 + e];
#pragma unroll
        for (int e = 0; e < 6; e++) dc[e] = d[6 * tid + e];
        large = !ss_ba_trial_pose(dc, a.p.step_eps, R, t, &small);
        finite = ss_gn_all_finite(R, t);
#pragma unroll
        for (int e = 0; e < 9; e++) dst[e] = R[e];
#pragma unroll
        for (int e = 0; e < 3; e++) dst[9 + e] = t[e];
    }
    const int any_large = __syncthreads_or(large ? 1 : 0);
    const int all_small = __syncthreads_and(small ? 1 : 0);
    const int all_finite = __syncthreads_and(finite ? 1 : 0);
    if (tid != 0) return;
    if (any_large) a.st[q].state = 4, a.st[q].ended = 1;
    a.st[q].pose_small = all_small, a.st[q].pose_finite = all_finite;
}

/* B-E.  grid (pblocks, problems): every point row of the other buffer is written */
__global__ __launch_bounds__(SS_GN_SLOTS) void k_ba_update(ssk_ba_call a)
{
    __shared__ double s_dc[6 * SS_BA_MAX_FREE];
    const int q = (int)blockIdx.y, i = (int)blockIdx.x * SS_GN_SLOTS + (int)threadIdx.x, P = a.point_rows;
    if (!ba_running(a, q)) return; /* uniform */
    const ba_prob pr = ba_prob_of(a, q);
    const int cur = a.st[q].cur & 1;
    if ((int)threadIdx.x < 6 * pr.n_free) s_dc[threadIdx.x] = a.dc[(size_t)q * 6 * a.max_free + threadIdx.x];
    __syncthreads();
    bool small = true, finite = true;
    if (i < P) {
        const double *Xc = ba_X(a, cur, q) + (size_t)i * 3;
        double *Xt = ba_X(a, cur ^ 1, q) + (size_t)i * 3;
        double X[3] = {Xc[0], Xc[1], Xc[2]};
        if (a.pflag[(size_t)q * P + i] == 0 && a.solved[(size_t)q * P + i]) {
            double L[6], v[3];
#pragma unroll
            for (int e = 0; e < 6; e++) L[e] = ba_lb(a, q, e)[i];
#pragma unroll
            for (int e = 0; e < 3; e++) v[e] = -ba_lb(a, q, 6 + e)[i];
            for (int k = 0; k < pr.n_free; k++) {
                if (!a.lin[(size_t)(pr.f0 + k) * P + i]) continue;
                double W[SS_BA_W];
#pragma unroll
                for (int e = 0; e < SS_BA_W; e++) W[e] = ba_wy(a, q, k, e)[i];
                ss_ba_point_rhs(W, s_dc + 6 * k, v);
            }
            ss_ba_point_subst(L, v);
#pragma unroll
            for (int e = 0; e < 3; e++) {
                X[e] = X[e] + v[e];
                small = small && fabs(v[e]) < a.p.step_eps;
                finite = finite && ss_gn_is_finite(X[e]);
            }
        }
        Xt[0] = X[0], Xt[1] = X[1], Xt[2] = X[2];
    }
    const int all_small = __syncthreads_and(small ? 1 : 0);
    const int all_finite = __syncthreads_and(finite ? 1 : 0);
    if (threadIdx.x == 0) {
        int32_t *b = a.blk + ((size_t)q * ba_pblocks(a) + blockIdx.x) * 4;
        b[1] = all_small, b[2] = all_finite;
    }
}

/* B-F.  grid (max_kf, problems): the tree of keyframe k's chi-terms under the current (trial == 0) or the trial state.  begin: the
 * cost ahead of a round's first step, which a round that is over does not keep from being formed */
__global__ __launch_bounds__(SS_GN_SLOTS) void k_ba_cost(ssk_ba_call a, int round, int trial, int begin)
{
    __shared__ double part[2][4][1];
    __shared__ double s_pose[12];
    __shared__ ss_pose_cam s_cam;
    const int q = (int)blockIdx.y, k = (int)blockIdx.x, P = a.point_rows, tid = (int)threadIdx.x;
    if (begin ? a.st[q].ended != 0 : !ba_running(a, q)) return; /* uniform */
    const ba_prob pr = ba_prob_of(a, q);
    if (k >= pr.n_kf) return;
    const int buf_state = (a.st[q].cur & 1) ^ (trial ? 1 : 0), f = pr.f0 + k;
    const bool robust = round < a.p.robust_rounds;
    if (tid == 0) {
        const double *src = a.pose + ((size_t)buf_state * a.n_frames + f) * 12;
#pragma unroll
        for (int e = 0; e < 12; e++) s_pose[e] = src[e];
        s_cam = ss_pose_cam_of(a.views[f], a.p.chi2_mono, a.p.chi2_stereo);
    }
    __syncthreads();
    const double *Xq = ba_X(a, buf_state, q);
    double sum[1] = {0.0};
    for (int i = tid; i < P; i += SS_GN_SLOTS) {
        if (a.pflag[(size_t)q * P + i] != 0 || a.obs[(size_t)f * P + i] != 0) continue;
        sum[0] = sum[0] + ss_ba_cost_term(ba_obs(a, Xq, f, i), s_cam, s_pose, s_pose + 9, robust);
    }
    int buf = 0;
    gn_block_sum(sum, part, &buf);
    if (tid == 0) a.cost_k[(size_t)q * a.max_kf + k] = sum[0];
}

/* B-G.  grid (problems), one thread */
__global__ __launch_bounds__(64) void k_ba_accept(ssk_ba_call a, int round, int begin)
{
    const int q = (int)blockIdx.x;
    if (threadIdx.x != 0) return;
    ssk_ba_state *s = a.st + q; /* updated in place: a copy indexed by the round would live in scratch */
    if (s->ended != 0 || (!begin && s->round_over != 0)) return;
    const ba_prob pr = ba_prob_of(a, q);
    double cost = 0.0;
    for (int k = 0; k < pr.n_kf; k++) cost = cost + a.cost_k[(size_t)q * a.max_kf + k];
    if (begin) {
        if (!ss_gn_is_finite(cost)) {
            s->state = 2, s->ended = 1;
            return;
        }
        s->cost0 = cost, s->round_over = 0;
        if (round == 0) s->cost_before = cost;
        return;
    }
    bool small = s->pose_small != 0, finite = s->pose_finite != 0;
    for (int b = 0; b < ba_pblocks(a); b++) {
        const int32_t *c = a.blk + ((size_t)q * ba_pblocks(a) + b) * 4;
        small = small && c[1] != 0, finite = finite && c[2] != 0;
    }
    const bool accepted = finite && ss_gn_is_finite(cost) && cost <= s->cost0;
    const int r = min(max(round, 0), 3);
    s->steps[r] = s->steps[r] + 1;
    s->lambda = ss_ba_next_lambda(s->lambda, accepted, a.p.lambda_factor, a.p.lambda_min);
    if (!accepted) return;
    s->accepted[r] = s->accepted[r] + 1;
    s->cost0 = cost;
    s->cur = s->cur ^ 1;
    if (small) s->round_over = 1;
}

/* B-H.  grid (pblocks, problems): after a round, under the current state */
__global__ __launch_bounds__(SS_GN_SLOTS) void k_ba_classify(ssk_ba_call a)
{
    __shared__ double s_pose[SS_BA_MAX_KF][12];
    __shared__ ss_pose_cam s_cam[SS_BA_MAX_KF];
    const int q = (int)blockIdx.y, i = (int)blockIdx.x * SS_GN_SLOTS + (int)threadIdx.x, P = a.point_rows;
    if (a.st[q].ended != 0) return; /* uniform */
    const ba_prob pr = ba_prob_of(a, q);
    const int cur = a.st[q].cur & 1;
    ba_stage(a, pr, cur, s_pose, s_cam);
    if (i >= P || a.pflag[(size_t)q * P + i] != 0) return;
    int cnt = 0;
    for (int k = 0; k < pr.n_kf; k++) {
        const size_t o = (size_t)(pr.f0 + k) * P + i;
        if (a.obs[o] != 0) continue;
        const ss_pose_obs ob = ba_obs(a, ba_X(a, cur, q), pr.f0 + k, i);
        if (ss_pose_inlier(ob, s_cam[k], ss_pose_chi2(ob, s_cam[k], s_pose[k], s_pose[k] + 9))) cnt++;
        else a.obs[o] = 1;
    }
    if (cnt < a.p.min_point_obs) a.pflag[(size_t)q * P + i] = 1;
}

/* B-I.  grid (pblocks, problems): the points out, the workgroup's counts */
__global__ __launch_bounds__(SS_GN_SLOTS) void k_ba_finish_points(ssk_ba_call a)
{
    __shared__ int part_n[2][4];
    const int q = (int)blockIdx.y, i = (int)blockIdx.x * SS_GN_SLOTS + (int)threadIdx.x, P = a.point_rows;
    const ba_prob pr = ba_prob_of(a, q);
    const int cur = a.st[q].cur & 1;
    int n_in = 0, n_act = 0, buf = 0;
    if (i < P) {
        const uint8_t flag = a.pflag[(size_t)q * P + i];
        const double *X = ba_X(a, cur, q) + (size_t)i * 3;
        double *out = a.out_xyz + ((size_t)q * P + i) * 3;
#pragma unroll
        for (int e = 0; e < 3; e++) out[e] = flag == 2 ? 0.0 : X[e];
        n_act = flag == 0 ? 1 : 0;
        for (int k = 0; k < pr.n_kf; k++) n_in += a.obs[(size_t)(pr.f0 + k) * P + i] == 0 ? 1 : 0;
    }
    n_in = gn_block_sum(n_in, part_n, &buf);
    n_act = gn_block_sum(n_act, part_n, &buf);
    if (threadIdx.x == 0) {
        int32_t *b = a.blk + ((size_t)q * ba_pblocks(a) + blockIdx.x) * 4;
        b[0] = n_in, b[3] = n_act;
    }
}

/* grid (frames), 64 threads: every frame's pose; workgroup q < n_problems writes problem q's result as well */
__global__ __launch_bounds__(64) void k_ba_finish(ssk_ba_call a)
{
    const int f = (int)blockIdx.x, tid = (int)threadIdx.x;
    const int fq = a.frame_prob[f];
    if (tid == 0) {
        double R[9], t[3];
        if (fq >= 0 && fq < a.n_problems) {
            const double *src = a.pose + ((size_t)(a.st[fq].cur & 1) * a.n_frames + f) * 12;
#pragma unroll
            for (int e = 0; e < 9; e++) R[e] = src[e];
#pragma unroll
            for (int e = 0; e < 3; e++) t[e] = src[9 + e];
        } else {
            (void)ss_pose_start(a.start + (size_t)12 * f, R, t);
        }
        double *dst = a.out_pose + (size_t)12 * f;
#pragma unroll
        for (int e = 0; e < 9; e++) dst[e] = R[e];
#pragma unroll
        for (int e = 0; e < 3; e++) dst[9 + e] = t[e];
    }
    if (tid != 1 || f >= a.n_problems) return;
    const int q = f;
    const ssk_ba_state s = a.st[q];
    int n_in = 0, n_act = 0;
    for (int b = 0; b < ba_pblocks(a); b++) {
        const int32_t *c = a.blk + ((size_t)q * ba_pblocks(a) + b) * 4;
        n_in += c[0], n_act += c[3];
    }
    ss_ba_result r;
    r.lambda = s.lambda, r.cost_before = s.cost_before, r.cost_after = s.cost0;
    r.state = s.state, r.status = s.status;
    r.n_obs = s.n_obs, r.n_stereo = s.n_stereo, r.n_inliers = n_in, r.n_points_active = n_act, r.n_frozen_max = s.n_frozen_max;
#pragma unroll
    for (int k = 0; k < 4; k++) r.steps[k] = s.steps[k], r.accepted[k] = s.accepted[k];
    r.reserved = 0;
    a.result[q] = r;
}

/* grid (pblocks, problems): x, y, z of every row that is a point */
__global__ __launch_bounds__(SS_GN_SLOTS) void k_ba_points_to_block(ssk_ba_block_call a)
{
    const int q = (int)blockIdx.y, i = (int)blockIdx.x * SS_GN_SLOTS + (int)threadIdx.x;
    if (i >= a.point_rows) return;
    const size_t o = (size_t)q * a.point_rows + i;
    if (a.flags[o] == 2) return;
    ss_map_point *p = a.points + (size_t)a.block_of[q] * a.point_rows + i;
    p->x = (float)a.xyz[o * 3], p->y = (float)a.xyz[o * 3 + 1], p->z = (float)a.xyz[o * 3 + 2];
}

inline unsigned pblocks_of(int rows) { return (unsigned)((rows + SS_GN_SLOTS - 1) / SS_GN_SLOTS); }

} // namespace

void ssk_ba_gather(hipStream_t s, const ssk_ba_call &g)
{
    hipLaunchKernelGGL(k_ba_gather, dim3(pblocks_of(g.point_rows), (unsigned)g.n_frames), dim3(SS_GN_SLOTS), 0, s, g);
    hipLaunchKernelGGL(k_ba_gather_points, dim3(pblocks_of(g.point_rows), (unsigned)g.n_problems), dim3(SS_GN_SLOTS), 0, s, g);
    hipLaunchKernelGGL(k_ba_gather_state, dim3((unsigned)g.n_problems), dim3(64), 0, s, g);
}

void ssk_ba_cost(hipStream_t s, const ssk_ba_call &g, int round, int trial)
{
    hipLaunchKernelGGL(k_ba_cost, dim3((unsigned)g.max_kf, (unsigned)g.n_problems), dim3(SS_GN_SLOTS), 0, s, g, round, trial, trial ? 0 : 1);
}

void ssk_ba_accept(hipStream_t s, const ssk_ba_call &g, int round, int begin)
{
    hipLaunchKernelGGL(k_ba_accept, dim3((unsigned)g.n_problems), dim3(64), 0, s, g, round, begin);
}

void ssk_ba_points(hipStream_t s, const ssk_ba_call &g, int round)
{
    hipLaunchKernelGGL(k_ba_points, dim3(pblocks_of(g.point_rows), (unsigned)g.n_problems), dim3(SS_GN_SLOTS), 0, s, g, round);
}

void ssk_ba_blocks(hipStream_t s, const ssk_ba_call &g, int round)
{
    hipLaunchKernelGGL(k_ba_blocks, dim3((unsigned)(g.max_free * (g.max_free + 1) / 2), (unsigned)g.n_problems), dim3(SS_GN_SLOTS), 0, s, g, round);
}

void ssk_ba_solve(hipStream_t s, const ssk_ba_call &g)
{
    const int n = 6 * g.max_free;
    const size_t tri = (size_t)n * (n + 1) / 2 * sizeof(double); /* 148 224 bytes at the most, of the 160 KiB of a workgroup */
    if (tri > 48 * 1024) (void)hipFuncSetAttribute((const void *)k_ba_solve, hipFuncAttributeMaxDynamicSharedMemorySize, (int)tri);
    hipLaunchKernelGGL(k_ba_solve, dim3((unsigned)g.n_problems), dim3(SS_GN_SLOTS), tri, s, g);
}

void ssk_ba_update(hipStream_t s, const ssk_ba_call &g)
{
    hipLaunchKernelGGL(k_ba_update, dim3(pblocks_of(g.point_rows), (unsigned)g.n_problems), dim3(SS_GN_SLOTS), 0, s, g);
}

void ssk_ba_classify(hipStream_t s, const ssk_ba_call &g)
{
    hipLaunchKernelGGL(k_ba_classify, dim3(pblocks_of(g.point_rows), (unsigned)g.n_problems), dim3(SS_GN_SLOTS), 0, s, g);
}

void ssk_ba_finish(hipStream_t s, const ssk_ba_call &g)
{
    hipLaunchKernelGGL(k_ba_finish_points, dim3(pblocks_of(g.point_rows), (unsigned)g.n_problems), dim3(SS_GN_SLOTS), 0, s, g);
    hipLaunchKernelGGL(k_ba_finish, dim3((unsigned)g.n_frames), dim3(64), 0, s, g);
}

void ssk_ba_points_to_block(hipStream_t s, const ssk_ba_block_call &g)
{
    hipLaunchKernelGGL(k_ba_points_to_block, dim3(pblocks_of(g.point_rows), (unsigned)g.n), dim3(SS_GN_SLOTS), 0, s, g);
}
