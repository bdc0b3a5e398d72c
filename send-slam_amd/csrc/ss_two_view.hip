/*
 * ss_two_view.hip -- the map from two frames' matches: TwoViewReconstruction::Reconstruct as Tracking::MonocularInitialization runs
 * it, every hypothesis of every initialising pair evaluated at once (the rule: include/sendslam_orb.h; DESIGN.md "Two-view
 * initialisation").  Every step of the arithmetic is the text of ss_two_view_steps.h, which the host twins compile too.
 *
 *   T-A  k_tv_gather  one workgroup per problem walks the rows of frame 1 in chunks of SSK_TV_GATHER_ROWS in ascending order: ballot and
 *                     prefix sums number the correspondences (gn_chunk_compact of ss_gn.h).  A kept row writes its four floats into
 *                     four planes and every row the number of its correspondence.  Then the two sums of the normalisation in the
 *                     rule's tree: a wave folds groups of 64 correspondences, four group sums make a chunk's, the chunks are added in
 *                     ascending order.  The counts of the motion hypotheses are zeroed here, so the call needs no memset
 *   T-B  k_tv_model   one lane per problem and hypothesis: the draws, both 9 x 9 normal matrices in turn in a slice of LDS one lane
 *                     wide (SS_TV_WORK doubles, lane-interleaved), the rank-2 projection in registers, one 256-byte record
 *   T-C  k_tv_score   a lane owns one correspondence and keeps its four coordinates in registers across SSK_TV_HYP_BLOCK hypotheses;
 *                     a hypothesis' record is one address per wave.  Both sums of the workgroup's chunk are folded in the tree and
 *                     written as one partial per (chunk, hypothesis): no floating-point atomic anywhere
 *   T-D  k_tv_select  one workgroup per problem: a lane adds a hypothesis' partials in ascending chunk order, one reduction under
 *                     ss_tv_beats (a total order) finds both winners, the model is chosen, its inliers flagged and counted, and one
 *                     lane decomposes it into the four or eight motion hypotheses
 *   T-E  k_tv_check   a lane per correspondence triangulates and tests an inlier under every motion hypothesis; one ballot and
 *                     popcount per wave and hypothesis go to LDS, the workgroup's integer sums to the counts with one vector atomic
 *                     each.  Integer sums are order-free
 *   T-F  k_tv_finish  one workgroup per problem: the best hypothesis, its good points' cosines as ordered keys in registers, the
 *                     order statistic by a search over the key's 64 bits (one histogram per four bits), the acceptance, then the rows in
 *                     ascending order once more for the flags and the compaction of the points
 *
 * Every floating-point step is a single IEEE operation (-ffp-contract=off).  Every global write is a plain vector store or a vector
 * atomic.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ss_constants.h"
#include "ss_gn.h"
#include "ss_kernels.h"
#include "ss_quad.h"
#include "ss_two_view_steps.h"

namespace {

static_assert(SSK_TV_GATHER_ROWS == 1024, "k_tv_gather, k_tv_finish: one row per thread and chunk, 16 waves");
static_assert(SS_TV_CHUNK == 256 && SS_GN_SLOTS == 256, "k_tv_score: one chunk of the tree per workgroup of four waves");
static_assert(SS_GUIDED_MAX_ROWS == 16 * SSK_TV_GATHER_ROWS, "k_tv_finish keeps a problem's keys in sixteen registers per lane");
static_assert(sizeof(ssk_tv_model) == 256, "27 doubles, two flags, padding");
static_assert(sizeof(ss_two_view_result) == 192 && sizeof(ss_two_view_params) == 64, "the ABI's records");

#define TV_MAX_GROUPS (SS_GUIDED_MAX_ROWS / 64)
#define TV_KEYS (SS_GUIDED_MAX_ROWS / SSK_TV_GATHER_ROWS)

struct tv_work_lds {
    double *p;
    __device__ __forceinline__ double &at(int k) { return p[k * 64]; }
};

__device__ __forceinline__ float *tv_plane(const ssk_tv_call &a, int k, int b) { return a.corr + ((size_t)k * a.n_frames + b) * a.rows; }

struct tv_corr {
    double u1, v1, u2, v2;
};
__device__ __forceinline__ tv_corr tv_load_corr(const ssk_tv_call &a, int b, int n)
{
    tv_corr c;
    c.u1 = (double)tv_plane(a, 0, b)[n], c.v1 = (double)tv_plane(a, 1, b)[n], c.u2 = (double)tv_plane(a, 2, b)[n], c.v2 = (double)tv_plane(a, 3, b)[n];
    return c;
}

/* the frames of problem b: f1 was checked on the host, f2 too unless it is < 0 (no frame 2) */
struct tv_frame {
    int f1, f2, status, n1, n2;
};
__device__ __forceinline__ tv_frame tv_frame_of(const ssk_tv_call &a, int b)
{
    tv_frame f;
    f.f1 = a.kp1_src[b], f.f2 = a.kp2_src[b];
    f.status = 0;
    if (a.frame_error) {
        f.status = a.frame_error[f.f1];
        if (f.status == 0 && f.f2 >= 0) f.status = a.frame_error[f.f2];
    }
    f.n1 = f.status ? 0 : gd_clamp_count(a.n1[f.f1], a.rows);
    f.n2 = (f.status || f.f2 < 0) ? 0 : gd_clamp_count(a.n2[f.f2], a.rows);
    return f;
}

__device__ __forceinline__ int tv_n_corr(const ssk_tv_call &a, int b) { return min(max(a.n_corr[b], 0), a.rows); }

__device__ __forceinline__ ss_tv_norm tv_norm_of(const ssk_tv_choice &c)
{
    ss_tv_norm n;
#pragma unroll
    for (int k = 0; k < 4; k++) n.m[k] = c.norm[k], n.d[k] = c.norm[4 + k];
    return n;
}

/* T-A.  grid (problems), SSK_TV_GATHER_ROWS threads; corr_of_row of every row < rows is written */
__global__ __launch_bounds__(SSK_TV_GATHER_ROWS) void k_tv_gather(ssk_tv_call a)
{
    __shared__ int wave_n[SSK_TV_GATHER_ROWS / 64];
    __shared__ double gsum[TV_MAX_GROUPS][4];
    __shared__ double s_m[4], s_d[4];
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x, rows = a.rows, lane = tid & 63, wave = tid >> 6;
    const tv_frame f = tv_frame_of(a, b);
    const int n_levels = min(max(a.n_levels, 1), SS_MAX_LEVELS);
    int base = 0;
    for (int c0 = 0; c0 < rows; c0 += SSK_TV_GATHER_ROWS) { /* uniform */
        const int i = c0 + tid;
        const size_t o = (size_t)b * rows + i;
        bool keep = false;
        int j = -1;
        if (i < f.n1) { /* n1 <= rows */
            j = a.idx[o];
            if (j >= 0 && j < f.n2) { /* n2 <= rows */
                const int octave = a.kp1[(size_t)f.f1 * rows + i].octave;
                keep = octave >= 0 && octave < n_levels;
            }
        }
        const gn_chunk ch = gn_chunk_compact<SSK_TV_GATHER_ROWS>(keep, wave_n);
        int pos = -1;
        if (keep) {
            pos = gn_chunk_pos(ch, base); /* pos <= i < rows */
            const ss_keypoint *k1 = a.kp1 + (size_t)f.f1 * rows + i, *k2 = a.kp2 + (size_t)f.f2 * rows + j;
            tv_plane(a, 0, b)[pos] = k1->x, tv_plane(a, 1, b)[pos] = k1->y, tv_plane(a, 2, b)[pos] = k2->x, tv_plane(a, 3, b)[pos] = k2->y;
        }
        if (i < rows) a.corr_of_row[o] = pos;
        base += ch.total;
        __syncthreads(); /* wave_n is rewritten */
    }
    const int n = base; /* <= rows <= SS_GUIDED_MAX_ROWS */
    const bool live = !ss_tv_too_few(n);
    const int n_chunks = (n + SS_TV_CHUNK - 1) / SS_TV_CHUNK, n_groups = 4 * n_chunks; /* <= TV_MAX_GROUPS */
    if (live) {
        for (int pass = 0; pass < 2; pass++) { /* uniform */
            for (int g = wave; g < n_groups; g += SSK_TV_GATHER_ROWS / 64) {
                const int k = 64 * g + lane;
#pragma unroll
                for (int c = 0; c < 4; c++) {
                    double x = 0.0;
                    if (k < n) {
                        x = (double)tv_plane(a, c, b)[k];
                        if (pass == 1) x = fabs(x - s_m[c]);
                    }
                    x = gn_wave_fold(x);
                    if (lane == 0) gsum[g][c] = x;
                }
            }
            __syncthreads();
            if (tid < 4) {
                double total = 0.0;
                for (int ch = 0; ch < n_chunks; ch++) {
                    const double v = ss_gn_combine(gsum[4 * ch][tid], gsum[4 * ch + 1][tid], gsum[4 * ch + 2][tid], gsum[4 * ch + 3][tid]);
                    total = ch == 0 ? v : total + v;
                }
                if (pass == 0) s_m[tid] = total / (double)n;
                else s_d[tid] = total / (double)n;
            }
            __syncthreads();
        }
    }
    if (tid == 0) {
        ssk_tv_choice *c = a.choice + b;
        ss_tv_norm nm;
        for (int k = 0; k < 4; k++) nm.m[k] = live ? s_m[k] : 0.0, nm.d[k] = live ? s_d[k] : 0.0;
        for (int k = 0; k < 4; k++) c->norm[k] = nm.m[k], c->norm[4 + k] = nm.d[k];
        c->norm_ok = live && ss_tv_norm_ok(nm) ? 1 : 0;
        for (int k = 0; k < 8; k++) c->good[k] = 0;
        a.n_corr[b] = n;
    }
}

/* T-B.  grid (ceil(max_iterations / 64), problems), 64 threads */
__global__ __launch_bounds__(64) void k_tv_model(ssk_tv_call a)
{
    __shared__ double work[SS_TV_WORK * 64];
    const int b = (int)blockIdx.y, t = (int)(blockIdx.x * 64 + threadIdx.x);
    if (t >= a.p.max_iterations) return;
    const int n = tv_n_corr(a, b);
    const ssk_tv_choice *c = a.choice + b;
    if (ss_tv_too_few(n) || !c->norm_ok) return;
    int pick[SS_TV_DRAWS];
    ss_tv_draw(a.p.seed, (uint32_t)b, t, n, pick); /* each in 0 .. n-1 */
    float uv[4 * SS_TV_DRAWS];
#pragma unroll
    for (int k = 0; k < SS_TV_DRAWS; k++) {
#pragma unroll
        for (int i = 0; i < 4; i++) uv[4 * k + i] = tv_plane(a, i, b)[pick[k]];
    }
    tv_work_lds w;
    w.p = work + threadIdx.x;
    ss_tv_model_of(uv, pick, tv_norm_of(*c), w, a.models[(size_t)b * a.p.max_iterations + t]);
}

/* T-C.  grid (ceil(rows / SS_TV_CHUNK), ceil(max_iterations / SSK_TV_HYP_BLOCK), problems), SS_TV_CHUNK threads */
__global__ __launch_bounds__(SS_TV_CHUNK) void k_tv_score(ssk_tv_call a)
{
    __shared__ double part[2][4][2];
    const int b = (int)blockIdx.z, tid = (int)threadIdx.x, chunk = (int)blockIdx.x;
    const int n = tv_n_corr(a, b);
    const int k0 = chunk * SS_TV_CHUNK;
    if (ss_tv_too_few(n) || !a.choice[b].norm_ok || k0 >= n) return; /* uniform */
    const int k = k0 + tid;
    const bool live = k < n;
    const tv_corr c = tv_load_corr(a, b, live ? k : 0);
    const int t0 = (int)blockIdx.y * SSK_TV_HYP_BLOCK, T = a.p.max_iterations;
    const int chunks = (a.rows + SS_TV_CHUNK - 1) / SS_TV_CHUNK;
    const ssk_tv_model *models = a.models + (size_t)b * T;
    double *partial = a.partial + (((size_t)b * chunks + chunk) * T) * 2;
    int buf = 0;
    for (int h = 0; h < SSK_TV_HYP_BLOCK && t0 + h < T; h++) { /* uniform */
        const ssk_tv_model *m = models + t0 + h;
        double v[2] = {0.0, 0.0}, chi[2];
        bool in;
        if (live && m->ok_h) v[0] = ss_tv_term_h(m->h21, m->h12, c.u1, c.v1, c.u2, c.v2, a.p.chi2_h, &in, chi);
        if (live && m->ok_f) v[1] = ss_tv_term_f(m->f21, c.u1, c.v1, c.u2, c.v2, a.p.chi2_f, a.p.chi2_score, &in, chi);
        gn_block_sum<2>(v, part, &buf);
        if (tid == 0) partial[2 * (t0 + h)] = v[0], partial[2 * (t0 + h) + 1] = v[1];
    }
}

/* T-D.  grid (problems), 256 threads */
__global__ __launch_bounds__(256) void k_tv_select(ssk_tv_call a)
{
    __shared__ double s_sh[256], s_sf[256];
    __shared__ int s_th[256], s_tf[256], s_in;
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x, T = a.p.max_iterations;
    const int n = tv_n_corr(a, b);
    ssk_tv_choice *c = a.choice + b;
    const bool dead = ss_tv_too_few(n) || !c->norm_ok;
    if (dead) { /* uniform */
        if (tid == 0) c->model = 0, c->n_hyp = 0, c->reason = 0, c->n_in = 0, c->t_h = c->t_f = -1, c->score_h = c->score_f = 0.0;
        return;
    }
    const int chunks = (a.rows + SS_TV_CHUNK - 1) / SS_TV_CHUNK, n_chunks = (n + SS_TV_CHUNK - 1) / SS_TV_CHUNK;
    const ssk_tv_model *models = a.models + (size_t)b * T;
    double sh = -1.0, sf = -1.0;
    int th = -1, tf = -1;
    for (int t = tid; t < T; t += 256) {
        double h = 0.0, f = 0.0;
        for (int ch = 0; ch < n_chunks; ch++) {
            const double *p = a.partial + ((((size_t)b * chunks + ch) * T) + t) * 2;
            h = ch == 0 ? p[0] : h + p[0];
            f = ch == 0 ? p[1] : f + p[1];
        }
        if (!models[t].ok_h) h = -1.0;
        if (!models[t].ok_f) f = -1.0;
        if (th < 0 || ss_tv_beats(h, t, sh, th)) sh = h, th = t;
        if (tf < 0 || ss_tv_beats(f, t, sf, tf)) sf = f, tf = t;
    }
    s_sh[tid] = sh, s_th[tid] = th, s_sf[tid] = sf, s_tf[tid] = tf;
    __syncthreads();
    for (int step = 128; step >= 1; step >>= 1) {
        if (tid < step) {
            const int oh = s_th[tid + step], of = s_tf[tid + step];
            if (oh >= 0 && (s_th[tid] < 0 || ss_tv_beats(s_sh[tid + step], oh, s_sh[tid], s_th[tid]))) s_sh[tid] = s_sh[tid + step], s_th[tid] = oh;
            if (of >= 0 && (s_tf[tid] < 0 || ss_tv_beats(s_sf[tid + step], of, s_sf[tid], s_tf[tid]))) s_sf[tid] = s_sf[tid + step], s_tf[tid] = of;
        }
        __syncthreads();
    }
    sh = s_sh[0], th = s_th[0], sf = s_sf[0], tf = s_tf[0];
    const int model = ss_tv_choose(sh, sf, a.p.rh_threshold);
    if (tid == 0) s_in = 0;
    __syncthreads();
    if (model != 0) { /* uniform */
        const ssk_tv_model *m = models + (model == 2 ? th : tf); /* 0 <= th, tf < T: T >= 1 */
        int mine = 0;
        for (int k = tid; k < n; k += 256) {
            const tv_corr q = tv_load_corr(a, b, k);
            bool in;
            double chi[2];
            if (model == 2) ss_tv_term_h(m->h21, m->h12, q.u1, q.v1, q.u2, q.v2, a.p.chi2_h, &in, chi);
            else ss_tv_term_f(m->f21, q.u1, q.v1, q.u2, q.v2, a.p.chi2_f, a.p.chi2_score, &in, chi);
            a.corr_flag[(size_t)b * a.rows + k] = in ? 1 : 0;
            mine += in ? 1 : 0;
        }
        if (mine) atomicAdd(&s_in, mine);
    }
    __syncthreads();
    if (tid == 0) {
        const int n_in = s_in;
        int n_hyp = 0, reason = 0;
        if (model != 0) {
            const ssk_tv_model *m = models + (model == 2 ? th : tf);
            const ss_tv_cam cam = ss_tv_cam_of(a.views[b]);
            double M[9];
#pragma unroll
            for (int k = 0; k < 9; k++) M[k] = model == 2 ? m->h21[k] : m->f21[k];
            if (n_in < SS_TV_DRAWS) reason = 2;
            else {
                n_hyp = model == 2 ? ss_tv_decompose_h(M, cam, c->hyp) : ss_tv_decompose_f(M, cam, c->hyp);
                if (n_hyp == 0) reason = 1;
            }
        }
        c->model = model, c->n_hyp = n_hyp, c->reason = reason, c->n_in = n_in, c->t_h = th, c->t_f = tf, c->score_h = sh, c->score_f = sf;
    }
}

/* T-E.  grid (ceil(rows / 256), problems), 256 threads */
__global__ __launch_bounds__(256) void k_tv_check(ssk_tv_call a)
{
    __shared__ int cnt[SS_TV_MAX_HYP];
    const int b = (int)blockIdx.y, tid = (int)threadIdx.x;
    const int n = tv_n_corr(a, b), k0 = (int)blockIdx.x * 256;
    ssk_tv_choice *c = a.choice + b;
    const bool dead = ss_tv_too_few(n) || !c->norm_ok;
    if (dead || k0 >= n) return; /* uniform */
    const int n_hyp = min(max(c->n_hyp, 0), SS_TV_MAX_HYP);
    if (c->model == 0 || c->reason != 0 || n_hyp == 0) return; /* uniform */
    const int k = k0 + tid;
    const bool live = k < n && a.corr_flag[(size_t)b * a.rows + k] != 0;
    const tv_corr q = tv_load_corr(a, b, k < n ? k : 0);
    const ss_tv_cam cam = ss_tv_cam_of(a.views[b]);
    if (tid < SS_TV_MAX_HYP) cnt[tid] = 0;
    __syncthreads();
    for (int h = 0; h < n_hyp; h++) { /* uniform */
        ss_tv_point pt;
        const bool good = live && ss_tv_check_rt(c->hyp + 12 * h, c->hyp + 12 * h + 9, cam, q.u1, q.v1, q.u2, q.v2, &pt);
        const unsigned long long mask = __ballot(good);
        if ((tid & 63) == 0 && mask != 0ull) atomicAdd(&cnt[h], __popcll(mask));
    }
    __syncthreads();
    if (tid < n_hyp && cnt[tid] > 0) atomicAdd(&c->good[tid], cnt[tid]);
}

/* T-F.  grid (problems), SSK_TV_GATHER_ROWS threads; the flag of every row < rows and the result are written */
__global__ __launch_bounds__(SSK_TV_GATHER_ROWS) void k_tv_finish(ssk_tv_call a)
{
    __shared__ int wave_n[SSK_TV_GATHER_ROWS / 64];
    __shared__ int s_hist[16][16];
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x, rows = a.rows;
    const tv_frame f = tv_frame_of(a, b);
    const int n = tv_n_corr(a, b);
    const ssk_tv_choice *c = a.choice + b;
    const bool too_few = ss_tv_too_few(n);
    const bool dead = too_few || !c->norm_ok;
    const int model = dead ? 0 : c->model, n_hyp = dead ? 0 : min(max(c->n_hyp, 0), SS_TV_MAX_HYP), n_in = dead ? 0 : c->n_in;
    const ss_tv_cam cam = ss_tv_cam_of(a.views[b]);
    int reason = model != 0 ? c->reason : 0;
    int good[SS_TV_MAX_HYP], best = -1, best_good = 0, second_good = 0;
#pragma unroll
    for (int k = 0; k < SS_TV_MAX_HYP; k++) good[k] = (model != 0 && reason == 0 && k < n_hyp) ? min(max(c->good[k], 0), rows) : 0;
    if (model != 0 && reason == 0) ss_tv_pick(good, n_hyp, &best, &best_good, &second_good);
    double R[9], t[3];
#pragma unroll
    for (int k = 0; k < 9; k++) R[k] = best >= 0 ? c->hyp[12 * best + k] : 0.0;
#pragma unroll
    for (int k = 0; k < 3; k++) t[k] = best >= 0 ? c->hyp[12 * best + 9 + k] : 0.0;
    double cosp = 0.0;
    if (tid < 256) s_hist[tid >> 4][tid & 15] = 0;
    __syncthreads();
    if (best >= 0) { /* uniform */
        uint64_t key[TV_KEYS];
        unsigned is_good = 0u;
#pragma unroll
        for (int i = 0; i < TV_KEYS; i++) {
            const int k = i * SSK_TV_GATHER_ROWS + tid;
            key[i] = ~0ull;
            if (k < n && a.corr_flag[(size_t)b * rows + k] != 0) {
                const tv_corr q = tv_load_corr(a, b, k);
                ss_tv_point pt;
                if (ss_tv_check_rt(R, t, cam, q.u1, q.v1, q.u2, q.v2, &pt)) key[i] = ss_tv_key(pt.cosp), is_good |= 1u << i;
            }
        }
        /* the key of rank want - 1 (from 0) among the good points, four bits a step from the top: a histogram of the nibble over the
         * keys that share the bits found so far, then the first nibble at which the count reaches the rank */
        const int want = ss_tv_parallax_index(best_good) + 1;
        uint64_t K = 0;
        int below = 0; /* good keys under the prefix found so far */
        for (int step = 0; step < 16; step++) { /* uniform */
            const int shift = 60 - 4 * step;
#pragma unroll
            for (int i = 0; i < TV_KEYS; i++) {
                const bool same = step == 0 || (key[i] >> (shift + 4)) == (K >> (shift + 4));
                if (((is_good >> i) & 1u) && same) atomicAdd(&s_hist[step][(int)((key[i] >> shift) & 15ull)], 1);
            }
            __syncthreads();
            int nib = 15, cum = below;
#pragma unroll
            for (int j = 14; j >= 0; j--) { /* the smallest nibble whose cumulative count reaches the rank */
                int upto = below;
#pragma unroll
                for (int e = 0; e <= j; e++) upto += s_hist[step][e];
                if (upto >= want) nib = j;
            }
#pragma unroll
            for (int e = 0; e < 15; e++) cum += e < nib ? s_hist[step][e] : 0;
            below = cum;
            K |= (uint64_t)nib << shift;
        }
        cosp = ss_tv_unkey(K);
    }
    if (model != 0 && reason == 0) reason = ss_tv_accept(model, good, n_hyp, best_good, second_good, n_in, cosp, a.p);
    const bool won = model != 0 && reason == 0;
    const int n_levels = min(max(a.n_levels, 1), SS_MAX_LEVELS);
    int base = 0;
    for (int c0 = 0; c0 < rows; c0 += SSK_TV_GATHER_ROWS) { /* uniform */
        const int i = c0 + tid;
        const size_t o = (size_t)b * rows + i;
        const int k = i < rows ? a.corr_of_row[o] : -1;
        const bool is_corr = k >= 0 && k < n;
        uint8_t flag = is_corr ? 1 : 0;
        bool tri = false;
        ss_tv_point pt;
        if (won && is_corr && a.corr_flag[(size_t)b * rows + k] != 0) {
            const tv_corr q = tv_load_corr(a, b, k);
            tri = ss_tv_check_rt(R, t, cam, q.u1, q.v1, q.u2, q.v2, &pt) && ss_tv_triangulated(pt.cosp);
            flag = tri ? 3 : 2;
        }
        const gn_chunk ch = gn_chunk_compact<SSK_TV_GATHER_ROWS>(tri, wave_n);
        if (tri) {
            const int pos = gn_chunk_pos(ch, base); /* pos <= i < rows */
            const int octave = min(max(a.kp1[(size_t)f.f1 * rows + i].octave, 0), n_levels - 1); /* the gather kept the row: in the table; the clamp guards the read only */
            a.points[(size_t)b * rows + pos] = ss_tv_map_point(pt, a.scale[octave], a.scale[n_levels - 1]);
            a.point_rows[2 * ((size_t)b * rows + pos)] = i, a.point_rows[2 * ((size_t)b * rows + pos) + 1] = a.idx[o];
        }
        if (i < rows) a.flag[o] = flag;
        base += ch.total;
        __syncthreads(); /* wave_n is rewritten */
    }
    if (tid == 0) {
        ss_two_view_result r;
        ss_tv_result_clear(&r, n, f.status);
        if (!too_few) {
            r.state = 2;
            if (!dead) {
                r.score_h = c->score_h, r.score_f = c->score_f, r.iteration_h = c->t_h, r.iteration_f = c->t_f;
                if (model != 0) {
                    r.model = model, r.state = won ? 0 : 3, r.reason = reason, r.n_inliers = n_in, r.n_good = best_good, r.cos_parallax = cosp;
                    if (won) {
#pragma unroll
                        for (int k = 0; k < 9; k++) r.r21[k] = R[k];
#pragma unroll
                        for (int k = 0; k < 3; k++) r.t21[k] = t[k];
                        r.n_triangulated = base;
                    }
                }
            }
        }
        a.n_points[b] = base;
        a.result[b] = r;
    }
}

} // namespace

void ssk_tv_gather(hipStream_t s, const ssk_tv_call &g) { hipLaunchKernelGGL(k_tv_gather, dim3((unsigned)g.n_frames), dim3(SSK_TV_GATHER_ROWS), 0, s, g); }

void ssk_tv_model_launch(hipStream_t s, const ssk_tv_call &g)
{
    hipLaunchKernelGGL(k_tv_model, dim3((unsigned)((g.p.max_iterations + 63) / 64), (unsigned)g.n_frames), dim3(64), 0, s, g);
}

void ssk_tv_score(hipStream_t s, const ssk_tv_call &g)
{
    const dim3 grid((unsigned)((g.rows + SS_TV_CHUNK - 1) / SS_TV_CHUNK), (unsigned)((g.p.max_iterations + SSK_TV_HYP_BLOCK - 1) / SSK_TV_HYP_BLOCK),
                    (unsigned)g.n_frames);
    hipLaunchKernelGGL(k_tv_score, grid, dim3(SS_TV_CHUNK), 0, s, g);
}

void ssk_tv_select(hipStream_t s, const ssk_tv_call &g) { hipLaunchKernelGGL(k_tv_select, dim3((unsigned)g.n_frames), dim3(256), 0, s, g); }

void ssk_tv_check(hipStream_t s, const ssk_tv_call &g)
{
    hipLaunchKernelGGL(k_tv_check, dim3((unsigned)((g.rows + 255) / 256), (unsigned)g.n_frames), dim3(256), 0, s, g);
}

void ssk_tv_finish(hipStream_t s, const ssk_tv_call &g) { hipLaunchKernelGGL(k_tv_finish, dim3((unsigned)g.n_frames), dim3(SSK_TV_GATHER_ROWS), 0, s, g); }
