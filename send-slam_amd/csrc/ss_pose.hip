/*
 * ss_pose.hip -- pose-only optimisation on matched map points: the damped Gauss-Newton of Optimizer::PoseOptimization for every
 * frame of a call at once (the rule: include/sendslam_orb.h; DESIGN.md "Pose-only optimisation").  Every step of the arithmetic is
 * the text of ss_pose_steps.h, which the host twin compiles too.
 *
 *   P-A  k_pose_gather  one workgroup per frame walks the slots in chunks of SSK_POSE_CHUNK in ascending order: ballot and prefix
 *                       sums number the observations (gn_chunk_compact of ss_gn.h), so the numbering is the rule's whatever the
 *                       schedule.  An observation writes its seven floats (X Y Z u v, the right coordinate or -1, the scale of its
 *                       octave) into seven planes and its slot; every other slot gets its flag 2 here
 *   P-B  k_pose_solve   one workgroup of SS_GN_SLOTS threads per frame holds the whole round and step loop.  Thread s owns the
 *                       observations s, s + 256, ...: it re-reads their planes every step (they stay in L2; a frame of 2000 has
 *                       eight per thread), keeps its 26 partial sums in registers and its observations' inlier bits in one 64-bit
 *                       mask.  A wave folds by halving through cross-lane moves, the four wave results go through LDS (two buffers
 *                       in turn: one barrier per tree; gn_block_sum of ss_gn.h), and every thread solves the same 6 x 6 system
 *                       from them, so the pose needs no broadcast and every branch on it is uniform.  Flags and result are
 *                       written at the end
 *
 * Every floating-point step is a single IEEE operation (-ffp-contract=off).  Every global write is a plain vector store.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ss_constants.h"
#include "ss_gn.h"
#include "ss_kernels.h"
#include "ss_pose_steps.h"
#include "ss_quad.h"

namespace {

static_assert(SSK_POSE_CHUNK == 1024, "k_pose_gather: one slot per thread and chunk, 16 waves");
static_assert(SS_GN_SLOTS == 256, "k_pose_solve: four waves, one group of 64 slots each");
static_assert(SS_GUIDED_MAX_ROWS <= 64 * SS_GN_SLOTS, "k_pose_solve: a thread's observations have one bit each in a 64-bit mask");
static_assert(sizeof(ss_pose_result) == 160, "thirteen doubles, fourteen integers, no padding");

/* plane k of the observations of frame b */
__device__ __forceinline__ float *pose_plane(const ssk_pose_call &a, int k, int b) { return a.planes + ((size_t)k * a.n_frames + b) * a.slots; }

__device__ __forceinline__ ss_pose_obs pose_load_obs(const ssk_pose_call &a, int b, int n)
{
    return ss_pose_obs_of(pose_plane(a, 0, b)[n], pose_plane(a, 1, b)[n], pose_plane(a, 2, b)[n], pose_plane(a, 3, b)[n], pose_plane(a, 4, b)[n],
                          pose_plane(a, 5, b)[n], pose_plane(a, 6, b)[n]);
}

/* P-A.  grid (frames), SSK_POSE_CHUNK threads; the flag of every slot that is no observation is written */
__global__ __launch_bounds__(SSK_POSE_CHUNK) void k_pose_gather(ssk_pose_call a)
{
    __shared__ int wave_n[SSK_POSE_CHUNK / 64];
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x, slots = a.slots;
    const gd_points_frame f = gd_points_frame_of(a.src, a.frame_error, a.np, a.nk, a.point_rows, a.rows, b);
    const int n_levels = min(max(a.n_levels, 1), SS_MAX_LEVELS);
    int base = 0;
    for (int c0 = 0; c0 < slots; c0 += SSK_POSE_CHUNK) { /* uniform */
        const int i = c0 + tid;
        const size_t o = (size_t)b * slots + i;
        bool keep = false;
        int prow = -1, krow = -1, octave = 0;
        if (i < slots) {
            const int j = a.idx[o];
            prow = a.idx_by_row ? j : i, krow = a.idx_by_row ? i : j;
            if (prow >= 0 && prow < f.np && krow >= 0 && krow < f.nt) { /* np <= point_rows, nt <= rows */
                octave = a.kp[(size_t)b * a.rows + krow].octave;
                keep = octave >= 0 && octave < n_levels;
                if (keep && a.p_skip && a.p_skip[(size_t)f.pb * a.point_rows + prow] != 0) keep = false;
            }
        }
        const gn_chunk ch = gn_chunk_compact<SSK_POSE_CHUNK>(keep, wave_n);
        if (keep) {
            const int pos = gn_chunk_pos(ch, base); /* pos <= i < slots */
            const ss_map_point *p = a.points + (size_t)f.pb * a.point_rows + prow;
            const ss_keypoint *kp = a.kp + (size_t)b * a.rows + krow;
            const float right = a.right ? a.right[(size_t)b * a.rows + krow] : 0.0f;
            pose_plane(a, 0, b)[pos] = p->x, pose_plane(a, 1, b)[pos] = p->y, pose_plane(a, 2, b)[pos] = p->z;
            pose_plane(a, 3, b)[pos] = kp->x, pose_plane(a, 4, b)[pos] = kp->y;
            pose_plane(a, 5, b)[pos] = ss_pose_stored_right(a.check_right != 0, a.right != nullptr, right);
            pose_plane(a, 6, b)[pos] = a.scale[octave];
            a.slot_of[(size_t)b * slots + pos] = i;
        } else if (i < slots) {
            a.flags[o] = 2;
        }
        base += ch.total;
        __syncthreads(); /* wave_n is rewritten */
    }
    if (tid == 0) a.n_obs[b] = base;
}

/* P-B.  grid (frames), SS_GN_SLOTS threads; the flag of every observation's slot and the result are written */
__global__ __launch_bounds__(SS_GN_SLOTS) void k_pose_solve(ssk_pose_call a)
{
    __shared__ double part[2][4][SS_POSE_SUMS];
    __shared__ int part_n[2][4];
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x, slots = a.slots;
    const gd_points_frame f = gd_points_frame_of(a.src, a.frame_error, a.np, a.nk, a.point_rows, a.rows, b);
    const int n = min(max(a.n_obs[b], 0), slots);
    const ss_pose_cam cam = ss_pose_cam_of(a.views[b], a.chi2_mono, a.chi2_stereo);
    double R[9], t[3], R0[9], t0[3];
    const bool start_ok = ss_pose_start(a.start + (size_t)12 * b, R, t);
#pragma unroll
    for (int k = 0; k < 9; k++) R0[k] = R[k];
#pragma unroll
    for (int k = 0; k < 3; k++) t0[k] = t[k];
    unsigned long long active = ~0ull; /* bit j: observation tid + 256 j is an inlier */
    unsigned long long steps = 0;      /* eight bits per round */
    int state = !start_ok ? 2 : n < a.min_obs ? 1 : 0;
    int n_in = n, buf = 0;
    double cost = 0.0;
    for (int round = 0; state == 0 && round < a.n_rounds; round++) { /* everything the loops branch on is the same in every thread */
        const bool robust = round < a.robust_rounds;
        for (int it = 0; it < a.iterations; it++) {
            double sum[SS_POSE_SUMS]; /* this thread's partial sums, then the frame's */
#pragma unroll
            for (int s = 0; s < SS_POSE_SUMS; s++) sum[s] = 0.0;
            int j = 0;
            for (int k = tid; k < n; k += SS_GN_SLOTS, j++) {
                if (!((active >> j) & 1ull)) continue;
                double term[SS_POSE_SUMS];
                if (!ss_pose_terms(pose_load_obs(a, b, k), cam, R, t, robust, term)) continue;
#pragma unroll
                for (int s = 0; s < SS_POSE_SUMS; s++) sum[s] = sum[s] + term[s];
            }
            gn_block_sum(sum, part, &buf);
            bool small;
            const int rc = ss_pose_step(sum, a.lambda, a.step_eps, R, t, &small);
            if (rc != 0) {
                state = rc;
                break;
            }
            steps += 1ull << (8 * round);
            if (small) break;
        }
        if (state != 0) break;
        unsigned long long now = 0ull;
        double mine = 0.0;
        int mine_n = 0, j = 0;
        for (int k = tid; k < n; k += SS_GN_SLOTS, j++) {
            const ss_pose_obs o = pose_load_obs(a, b, k);
            const double chi2 = ss_pose_chi2(o, cam, R, t);
            if (ss_pose_inlier(o, cam, chi2)) {
                now |= 1ull << j;
                mine = mine + chi2;
                mine_n++;
            }
        }
        active = now;
        gn_block_sum(&mine, &mine_n, part, part_n, &buf);
        cost = mine, n_in = mine_n;
        if (n_in < a.min_obs) state = 3;
    }
    if (!ss_gn_all_finite(R, t)) {
        state = 2;
#pragma unroll
        for (int k = 0; k < 9; k++) R[k] = R0[k];
#pragma unroll
        for (int k = 0; k < 3; k++) t[k] = t0[k];
    }
    int n_stereo = 0, j = 0;
    for (int k = tid; k < n; k += SS_GN_SLOTS, j++) {
        const int slot = a.slot_of[(size_t)b * slots + k];
        if (slot >= 0 && slot < slots) a.flags[(size_t)b * slots + slot] = ((active >> j) & 1ull) ? 0 : 1;
        n_stereo += pose_plane(a, 5, b)[k] > 0.0f ? 1 : 0;
    }
    n_stereo = gn_block_sum(n_stereo, part_n, &buf);
    if (tid == 0) {
        ss_pose_result r;
#pragma unroll
        for (int k = 0; k < 9; k++) r.rcw[k] = R[k];
#pragma unroll
        for (int k = 0; k < 3; k++) r.tcw[k] = t[k];
        r.cost = cost;
        r.state = state;
        r.status = f.status;
        r.n_obs = n;
        r.n_stereo = n_stereo;
        r.n_inliers = n_in;
#pragma unroll
        for (int k = 0; k < 8; k++) r.steps[k] = (int32_t)((steps >> (8 * k)) & 0xFFull);
        r.reserved = 0;
        a.result[b] = r;
    }
}

} // namespace

void ssk_pose_gather(hipStream_t s, const ssk_pose_call &g) { hipLaunchKernelGGL(k_pose_gather, dim3((unsigned)g.n_frames), dim3(SSK_POSE_CHUNK), 0, s, g); }

void ssk_pose_solve(hipStream_t s, const ssk_pose_call &g) { hipLaunchKernelGGL(k_pose_solve, dim3((unsigned)g.n_frames), dim3(SS_GN_SLOTS), 0, s, g); }
