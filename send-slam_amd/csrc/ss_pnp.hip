/*
 * ss_pnp.hip -- a pose from 2D-3D matches with no prior: MLPnPsolver's RANSAC over six-point models as Tracking::Relocalization
 * runs it, every hypothesis of every candidate evaluated at once (the rule: include/sendslam_orb.h; DESIGN.md "PnP RANSAC").  Every
 * step of the arithmetic is the text of ss_pnp_steps.h, which the host twins compile too.
 *
 *   N-A  k_pnp_gather  one workgroup per problem walks the keypoint rows in chunks of SSK_PNP_CHUNK in ascending order: ballot and
 *                      prefix sums number the correspondences (gn_chunk_compact of ss_gn.h), so the numbering is the rule's whatever
 *                      the schedule.  A kept row writes its six floats into six planes, its scale and point row into two more that
 *                      only the model reads, and every row the number of its correspondence
 *   N-B  k_pnp_model   one lane per problem and hypothesis: the draws, the 12 x 12 normal matrix, its factor and the inverse
 *                      iterations in a slice of LDS one lane wide (SS_PNP_WORK doubles, lane-interleaved: no bank conflict, and the
 *                      loops of the factorisation stay rolled without any register array indexed by a variable), Horn's rotation
 *                      and the refinement in registers, one 64-byte record and twelve doubles; the hypothesis' count is zeroed
 *                      here, so the call needs no memset
 *   N-C  k_pnp_count   a lane owns one correspondence and keeps its six floats in registers across SSK_PNP_HYP_BLOCK hypotheses.  A
 *                      hypothesis' record is one address per wave; one ballot and popcount per wave and hypothesis go to LDS, and
 *                      the workgroup adds its SSK_PNP_HYP_BLOCK integer sums to the counts with one vector atomic each.  Integer
 *                      sums are order-free
 *   N-D  k_pnp_finish  one workgroup per problem: the largest count and the smallest t among equals by one max-reduction over
 *                      ss_pnp_key, the selection predicate, then the winner once more over the rows for the flags
 *
 * Every floating-point step is a single IEEE operation (-ffp-contract=off).  Every global write is a plain vector store or a vector
 * atomic.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ss_constants.h"
#include "ss_gn.h"
#include "ss_kernels.h"
#include "ss_pnp_steps.h"
#include "ss_quad.h"

namespace {

static_assert(SSK_PNP_CHUNK == 1024, "k_pnp_gather: one row per thread and chunk, 16 waves");
static_assert(SSK_PNP_COUNT_ROWS == 256 && SSK_PNP_HYP_BLOCK <= 64, "k_pnp_count: one correspondence per thread, the sums in one wave");
static_assert(sizeof(ssk_pnp_model) == 64, "one record, four float4");
static_assert(sizeof(ss_pnp_result) == 128, "twelve doubles, eight integers");
static_assert(SS_GUIDED_MAX_ROWS <= (0x7FFFFFFF / SS_PNP_MAX_ITERATIONS) - 1, "ss_pnp_key fits an int");

/* the work area of one lane: entry k of lane l at work[k * 64 + l] */
struct pnp_work_lds {
    double *p;
    __device__ __forceinline__ double &at(int k) { return p[k * 64]; }
};

/* plane k of the correspondences of problem b */
__device__ __forceinline__ float *pnp_plane(const ssk_pnp_call &a, int k, int b) { return a.corr + ((size_t)k * a.n_frames + b) * a.rows; }

__device__ __forceinline__ ss_pnp_corr pnp_load_corr(const ssk_pnp_call &a, int b, int n)
{
    ss_pnp_corr c;
    c.X[0] = pnp_plane(a, 0, b)[n], c.X[1] = pnp_plane(a, 1, b)[n], c.X[2] = pnp_plane(a, 2, b)[n];
    c.u = pnp_plane(a, 3, b)[n], c.v = pnp_plane(a, 4, b)[n], c.max = pnp_plane(a, 5, b)[n];
    return c;
}

/* the frames of problem b: kf and pb were checked on the host */
struct pnp_frame {
    int kf, pb, status, nk, np;
};
__device__ __forceinline__ pnp_frame pnp_frame_of(const ssk_pnp_call &a, int b)
{
    pnp_frame f;
    f.kf = a.kp_src[b], f.pb = a.point_src[b];
    f.status = a.frame_error ? a.frame_error[f.kf] : 0;
    f.nk = f.status ? 0 : gd_clamp_count(a.nk[f.kf], a.rows);
    f.np = f.status ? 0 : gd_clamp_count(a.np[f.pb], a.point_rows);
    return f;
}

/* N-A.  grid (problems), SSK_PNP_CHUNK threads; corr_of_row of every row < rows is written */
__global__ __launch_bounds__(SSK_PNP_CHUNK) void k_pnp_gather(ssk_pnp_call a)
{
    __shared__ int wave_n[SSK_PNP_CHUNK / 64];
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x, rows = a.rows;
    const pnp_frame f = pnp_frame_of(a, b);
    const int n_levels = min(max(a.n_levels, 1), SS_MAX_LEVELS);
    int base = 0;
    for (int c0 = 0; c0 < rows; c0 += SSK_PNP_CHUNK) { /* uniform */
        const int i = c0 + tid;
        const size_t o = (size_t)b * rows + i;
        bool keep = false;
        int j = -1, octave = 0;
        if (i < f.nk) { /* nk <= rows */
            j = a.idx[o];
            if (j >= 0 && j < f.np) { /* np <= point_rows */
                octave = a.kp[(size_t)f.kf * rows + i].octave;
                keep = octave >= 0 && octave < n_levels;
                if (keep && a.p_skip && a.p_skip[(size_t)f.pb * a.point_rows + j] != 0) keep = false;
            }
        }
        const gn_chunk ch = gn_chunk_compact<SSK_PNP_CHUNK>(keep, wave_n);
        int pos = -1;
        if (keep) {
            pos = gn_chunk_pos(ch, base); /* pos <= i < rows */
            const ss_map_point *p = a.points + (size_t)f.pb * a.point_rows + j;
            const ss_keypoint *kp = a.kp + (size_t)f.kf * rows + i;
            const float s = a.scale[octave];
            pnp_plane(a, 0, b)[pos] = p->x, pnp_plane(a, 1, b)[pos] = p->y, pnp_plane(a, 2, b)[pos] = p->z;
            pnp_plane(a, 3, b)[pos] = kp->x, pnp_plane(a, 4, b)[pos] = kp->y;
            pnp_plane(a, 5, b)[pos] = ss_pnp_max(a.chi2, s);
            a.corr_scale[(size_t)b * rows + pos] = s;
            a.corr_point[(size_t)b * rows + pos] = j;
        }
        if (i < rows) a.corr_of_row[o] = pos;
        base += ch.total;
        __syncthreads(); /* wave_n is rewritten */
    }
    if (tid == 0) a.n_corr[b] = base;
}

/* N-B.  grid (ceil(max_iterations / 64), problems), 64 threads */
__global__ __launch_bounds__(64) void k_pnp_model(ssk_pnp_call a)
{
    __shared__ double work[SS_PNP_WORK * 64];
    const int b = (int)blockIdx.y, t = (int)(blockIdx.x * 64 + threadIdx.x);
    if (t >= a.max_iterations) return;
    const int n = min(max(a.n_corr[b], 0), a.rows);
    const size_t at = (size_t)b * a.max_iterations + t;
    a.counts[at] = 0;
    if (ss_pnp_too_few(n, a.min_inliers)) return;
    int pick[SS_PNP_DRAWS];
    ss_pnp_draw(a.seed, (uint32_t)b, t, n, pick); /* each in 0 .. n-1 */
    float X[3 * SS_PNP_DRAWS], uv[2 * SS_PNP_DRAWS], sc[SS_PNP_DRAWS];
    int row[SS_PNP_DRAWS];
#pragma unroll
    for (int k = 0; k < SS_PNP_DRAWS; k++) {
#pragma unroll
        for (int i = 0; i < 3; i++) X[3 * k + i] = pnp_plane(a, i, b)[pick[k]];
        uv[2 * k] = pnp_plane(a, 3, b)[pick[k]], uv[2 * k + 1] = pnp_plane(a, 4, b)[pick[k]];
        sc[k] = a.corr_scale[(size_t)b * a.rows + pick[k]];
        row[k] = a.corr_point[(size_t)b * a.rows + pick[k]];
    }
    pnp_work_lds w;
    w.p = work + threadIdx.x;
    const ss_pnp_model m = ss_pnp_model_of(X, uv, sc, row, ss_pnp_cam_of(a.views[b]), a.lambda, a.refine_steps, w);
    float4 *out = (float4 *)(a.models + at);
    out[0] = make_float4(m.rf[0], m.rf[1], m.rf[2], m.rf[3]);
    out[1] = make_float4(m.rf[4], m.rf[5], m.rf[6], m.rf[7]);
    out[2] = make_float4(m.rf[8], m.tf[0], m.tf[1], m.tf[2]);
    out[3] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    double2 *pose = (double2 *)(a.poses + at * 12);
    pose[0] = make_double2(m.rcw[0], m.rcw[1]);
    pose[1] = make_double2(m.rcw[2], m.rcw[3]);
    pose[2] = make_double2(m.rcw[4], m.rcw[5]);
    pose[3] = make_double2(m.rcw[6], m.rcw[7]);
    pose[4] = make_double2(m.rcw[8], m.tcw[0]);
    pose[5] = make_double2(m.tcw[1], m.tcw[2]);
}

/* N-C.  grid (ceil(rows / SSK_PNP_COUNT_ROWS), ceil(max_iterations / SSK_PNP_HYP_BLOCK), problems), SSK_PNP_COUNT_ROWS threads */
__global__ __launch_bounds__(SSK_PNP_COUNT_ROWS) void k_pnp_count(ssk_pnp_call a)
{
    __shared__ int cnt[SSK_PNP_HYP_BLOCK];
    const int b = (int)blockIdx.z, tid = (int)threadIdx.x;
    const int n_corr = min(max(a.n_corr[b], 0), a.rows);
    const int n0 = (int)blockIdx.x * SSK_PNP_COUNT_ROWS;
    if (ss_pnp_too_few(n_corr, a.min_inliers) || n0 >= n_corr) return; /* uniform */
    const int n = n0 + tid;
    const bool live = n < n_corr;
    const ss_pnp_corr c = pnp_load_corr(a, b, live ? n : 0);
    const ss_pnp_cam cam = ss_pnp_cam_of(a.views[b]);
    const int t0 = (int)blockIdx.y * SSK_PNP_HYP_BLOCK;
    const ssk_pnp_model *models = a.models + (size_t)b * a.max_iterations;
    if (tid < SSK_PNP_HYP_BLOCK) cnt[tid] = 0;
    __syncthreads();
    for (int h = 0; h < SSK_PNP_HYP_BLOCK && t0 + h < a.max_iterations; h++) { /* uniform */
        const ssk_pnp_model *m = models + t0 + h;
        const bool in = live && ss_pnp_inlier(m->r, m->t, c, cam);
        const unsigned long long mask = __ballot(in);
        if ((tid & 63) == 0 && mask != 0ull) atomicAdd(&cnt[h], __popcll(mask));
    }
    __syncthreads();
    if (tid < SSK_PNP_HYP_BLOCK && t0 + tid < a.max_iterations && cnt[tid] > 0) atomicAdd(a.counts + (size_t)b * a.max_iterations + t0 + tid, cnt[tid]);
}

/* N-D.  grid (problems), 256 threads; the flag of every row < rows and the result are written */
__global__ __launch_bounds__(256) void k_pnp_finish(ssk_pnp_call a)
{
    __shared__ int s_key, s_inliers;
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x, rows = a.rows;
    const pnp_frame f = pnp_frame_of(a, b);
    const int n_corr = min(max(a.n_corr[b], 0), rows);
    const bool too_few = ss_pnp_too_few(n_corr, a.min_inliers);
    if (tid == 0) s_key = -1, s_inliers = 0;
    __syncthreads();
    if (!too_few) {
        int key = -1;
        for (int t = tid; t < a.max_iterations; t += 256) key = max(key, ss_pnp_key(min(max(a.counts[(size_t)b * a.max_iterations + t], 0), rows), t));
        if (key >= 0) atomicMax(&s_key, key);
    }
    __syncthreads();
    const int key = s_key;
    const int best = key < 0 ? 0 : ss_pnp_key_count(key);
    const bool won = key >= 0 && ss_pnp_wins(best, n_corr, a.min_inliers, a.min_ratio);
    const int win = won ? ss_pnp_key_t(key) : 0; /* < max_iterations */
    const ssk_pnp_model *m = a.models + (size_t)b * a.max_iterations + win;
    const ss_pnp_cam cam = ss_pnp_cam_of(a.views[b]);
    int mine = 0;
    for (int i = tid; i < rows; i += 256) {
        const size_t o = (size_t)b * rows + i;
        const int n = a.corr_of_row[o];
        uint8_t flag = 0;
        if (won && n >= 0 && n < n_corr) flag = ss_pnp_inlier(m->r, m->t, pnp_load_corr(a, b, n), cam) ? 1 : 0;
        a.inlier[o] = flag;
        mine += flag;
    }
    if (mine) atomicAdd(&s_inliers, mine);
    __syncthreads();
    if (tid == 0) {
        ss_pnp_result r;
        const double *pose = a.poses + ((size_t)b * a.max_iterations + win) * 12;
        for (int k = 0; k < 9; k++) r.rcw[k] = won ? pose[k] : 0.0;
        for (int k = 0; k < 3; k++) r.tcw[k] = won ? pose[9 + k] : 0.0;
        r.state = too_few ? 1 : won ? 0 : 2;
        r.status = f.status;
        r.n_corr = n_corr;
        r.n_inliers = s_inliers;
        r.best_inliers = best;
        r.iteration = won ? win : -1;
        r.reserved[0] = r.reserved[1] = 0;
        a.result[b] = r;
    }
}

} // namespace

void ssk_pnp_gather(hipStream_t s, const ssk_pnp_call &g) { hipLaunchKernelGGL(k_pnp_gather, dim3((unsigned)g.n_frames), dim3(SSK_PNP_CHUNK), 0, s, g); }

void ssk_pnp_model_launch(hipStream_t s, const ssk_pnp_call &g)
{
    hipLaunchKernelGGL(k_pnp_model, dim3((unsigned)((g.max_iterations + 63) / 64), (unsigned)g.n_frames), dim3(64), 0, s, g);
}

void ssk_pnp_count(hipStream_t s, const ssk_pnp_call &g)
{
    const dim3 grid((unsigned)((g.rows + SSK_PNP_COUNT_ROWS - 1) / SSK_PNP_COUNT_ROWS),
                    (unsigned)((g.max_iterations + SSK_PNP_HYP_BLOCK - 1) / SSK_PNP_HYP_BLOCK), (unsigned)g.n_frames);
    hipLaunchKernelGGL(k_pnp_count, grid, dim3(SSK_PNP_COUNT_ROWS), 0, s, g);
}

void ssk_pnp_finish(hipStream_t s, const ssk_pnp_call &g) { hipLaunchKernelGGL(k_pnp_finish, dim3((unsigned)g.n_frames), dim3(256), 0, s, g); }
