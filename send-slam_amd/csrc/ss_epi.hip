/*
 * ss_epi.hip -- new map points from pairs of keyframes: the epipolar search of ORBmatcher::SearchForTriangulation and the per-match
 * part of LocalMapping::CreateNewMapPoints with MapPoint::UpdateNormalAndDepth (the rule: include/sendslam_orb.h; DESIGN.md
 * "Epipolar search and triangulation").  The train frames are indexed by k_bow_index (ss_bow.hip), one_to_one and the rotation
 * histogram are k_guided_finish (ss_guided.hip), both as they are.
 *
 *   E-A  k_epi_search   k_bow_search's shape: four lanes (a quad) per query row walk the run of the row's node in the train frame's
 *                       index (gd_walk_node, ss_quad.h).  The pair is one address per workgroup (scalar loads); the epipolar line
 *                       a, b, c is evaluated once per row; a couple passes taken flag, octave, epipole and line (ss_epi_steps.h, the
 *                       text the host twin compiles) before its descriptor is loaded.  Only the best key d << 20 | row is folded:
 *                       no second best
 *   E-B  k_epi_summary  one workgroup per pair: the sums of the per-row counters next to what k_guided_finish counted
 *   T-A  k_tri_eval     one thread per query row: steps 1 - 9 in double with the 4 x 4 arrays in registers, the info record, the
 *                       map point of the row into a workspace
 *   T-A' k_tri_stereo_eval     the stereo form of T-A (ss_tri_stereo_eval): depth and right coordinate of both rows from strided planes;
 *                       T-B runs on the mono records it leaves in the workspace; k_tri_stereo_summary adds the rows per mode
 *   T-B  k_tri_compact  one workgroup per pair walks the rows in chunks of SSK_TRI_CHUNK in ascending order: ballot and prefix
 *                       sums place the state-0 rows, so the compact block is in query-row order whatever the schedule
 *
 * Every floating-point step is a single IEEE operation (-ffp-contract=off).  Every global write is a plain vector store.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ss_constants.h"
#include "ss_kernels.h"
#include "ss_epi_steps.h"
#include "ss_quad.h"

namespace {

static_assert(SSK_TRI_CHUNK == 1024, "k_tri_compact: one row per thread and chunk, 16 waves");

/* E-A.  grid (ceil(rows / 64), pairs), 256 threads; every row < rows is written */
__global__ __launch_bounds__(256) void k_epi_search(ssk_guided_call a, ssk_epi_call e)
{
    const int b = (int)blockIdx.y, rows = a.rows;
    const int i = (int)(blockIdx.x * 64 + (threadIdx.x >> 2)), sub = (int)(threadIdx.x & 3);
    const gd_frame f = gd_frame_of(a.src, a.frame_error, a.nq, a.nt, rows, b);
    const ss_epi_pair *w = e.pairs + b; /* one address per workgroup */
    const int n_levels = min(max(e.n_levels, 1), SS_MAX_LEVELS);
    const int t = max(f.t, 0), nt = f.nt;
    bool live = i < f.nq;
    int node = live ? e.q_node[(size_t)b * rows + i] : -1;
    if (live && e.q_taken && e.q_taken[(size_t)b * rows + i] != 0) live = false;
    uint32_t best = GD_NONE, count = 0, geo = 0, near = 0;
    if (live && nt > 0 && node >= 0) {
        const ss_keypoint *qk = a.q_kp + (size_t)b * rows + i;
        const ss_epi_line line = ss_epi_line_of(w->f12, qk->x, qk->y);
        const float ex = w->ex, ey = w->ey;
        const int epipole_test = w->epipole_test;
        const gd_desc q = gd_load_desc(a.q_desc + ((size_t)b * rows + i) * SS_DESC_BYTES);
        const uint8_t *td = a.t_desc + (size_t)t * rows * SS_DESC_BYTES;
        const ss_keypoint *tkp = a.t_kp + (size_t)t * rows;
        const uint8_t *taken = e.t_taken ? e.t_taken + (size_t)t * rows : nullptr;
        const int skip = (a.exclude_same_frame && f.t == b) ? i : -1;
        gd_walk_node(e.index + (size_t)t * rows, min(max(e.n_index[t], 0), rows), node, sub, [&](int row) {
            if (row >= nt || row == skip) return; /* row < nt <= rows: the index was made with the same count */
            if (taken && taken[row] != 0) return;
            count++;
            const ss_keypoint *tk = tkp + row;
            const float2 xy = *(const float2 *)tk;
            if (ss_epi_check(ex, ey, epipole_test, e.coarse, line, e.scale, n_levels, xy.x, xy.y, tk->octave) != 0) return;
            geo++;
            const uint32_t dist = gd_hamming(q, td + (size_t)row * SS_DESC_BYTES);
            if ((int)dist > a.th) return;
            near++;
            best = min(best, (dist << 20) | (uint32_t)row);
        });
    }
    /* fold the quad: all 64 lanes take part */
#pragma unroll
    for (int m = 1; m <= 2; m <<= 1) {
        gd_fold_step(best, count, m);
        geo += (uint32_t)__shfl_xor((int)geo, m);
        near += (uint32_t)__shfl_xor((int)near, m);
    }
    if (i >= rows || sub != 0) return;
    const size_t o = (size_t)b * rows + i;
    a.idx[o] = best == GD_NONE ? -1 : (int)(best & 0xFFFFFu);
    a.d1[o] = (uint16_t)gd_dist_of(best);
    a.n_cand[o] = (int32_t)count;
    e.n_geo[o] = (int32_t)geo;
    e.n_near[o] = (int32_t)near;
}

/* E-B.  grid (pairs), 256 threads, after k_guided_finish */
__global__ __launch_bounds__(256) void k_epi_summary(ssk_guided_call a, ssk_epi_call e)
{
    __shared__ int cnt[2];
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x, rows = a.rows;
    const ss_guided_summary g = a.summary[b];
    const int nq = min(max(g.n_query, 0), rows);
    if (tid < 2) cnt[tid] = 0;
    __syncthreads();
    int geo = 0, near = 0;
    for (int i = tid; i < nq; i += 256) {
        geo += e.n_geo[(size_t)b * rows + i];
        near += e.n_near[(size_t)b * rows + i];
    }
    if (geo) atomicAdd(&cnt[0], geo);
    if (near) atomicAdd(&cnt[1], near);
    __syncthreads();
    if (tid == 0) {
        ss_epi_summary s;
        s.status = g.status;
        s.n_query = g.n_query;
        s.n_train = g.n_train;
        s.n_candidates = g.n_candidates;
        s.n_geometric = cnt[0];
        s.n_near = cnt[1];
        s.n_accepted = g.n_accepted;
        s.n_unique = g.n_unique;
        s.n_final = g.n_final;
        s.rot_bins = g.rot_bins;
        e.summary[b] = s;
    }
}

/* T-A.  grid (ceil(rows / 256), pairs), 256 threads; the info of every row < rows is written, the workspace point of a state-0 row */
__global__ __launch_bounds__(256) void k_tri_eval(ssk_tri_call a)
{
    const int b = (int)blockIdx.y, rows = a.rows;
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= rows) return;
    const gd_frame f = gd_frame_of(a.src, a.frame_error, a.nq, a.nt, rows, b);
    const int n_levels = min(max(a.n_levels, 1), SS_MAX_LEVELS);
    const size_t o = (size_t)b * rows + i;
    const int j = i < f.nq ? a.idx[o] : -1;
    ss_tri_out r = ss_tri_rejected(-1, 0.0, 0.0, 0.0);
    if (j >= 0 && j < f.nt) {
        const ss_keypoint *k1 = a.q_kp + o, *k2 = a.t_kp + (size_t)f.t * rows + j;
        const float2 p1 = *(const float2 *)k1, p2 = *(const float2 *)k2;
        r = ss_tri_eval(a.pairs[b], a.tp, a.scale, n_levels, p1.x, p1.y, k1->octave, p2.x, p2.y, k2->octave);
    }
    a.info[o] = r.info;
    if (r.info.state == 0) {
        float4 *po = (float4 *)(a.tmp + o);
        po[0] = make_float4(r.point.x, r.point.y, r.point.z, r.point.nx);
        po[1] = make_float4(r.point.ny, r.point.nz, r.point.min_dist, r.point.max_dist);
    }
}

/* T-A, stereo form.  As k_tri_eval, with the depth and right coordinate of both rows; the mono record goes to the workspace for T-B */
__global__ __launch_bounds__(256) void k_tri_stereo_eval(ssk_tri_stereo_call c)
{
    const ssk_tri_call &a = c.t;
    const int b = (int)blockIdx.y, rows = a.rows;
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= rows) return;
    const gd_frame f = gd_frame_of(a.src, a.frame_error, a.nq, a.nt, rows, b);
    const int n_levels = min(max(a.n_levels, 1), SS_MAX_LEVELS);
    const size_t o = (size_t)b * rows + i;
    const int j = i < f.nq ? a.idx[o] : -1;
    ss_tri_stereo_out r = ss_tri_stereo_rejected(-1, -1, 0.0, 0.0, 0.0, 0.0, 0.0);
    if (j >= 0 && j < f.nt) {
        const size_t t = (size_t)f.t * rows + j;
        const ss_keypoint *k1 = a.q_kp + o, *k2 = a.t_kp + t;
        const float2 p1 = *(const float2 *)k1, p2 = *(const float2 *)k2;
        ss_tri_stereo_params sp;
        sp.tri = a.tp, sp.chi2_stereo = c.chi2_stereo;
        const float d1 = *(const float *)(c.depth1 + (int64_t)o * c.depth1_stride), u1 = *(const float *)(c.right1 + (int64_t)o * c.right1_stride);
        const float d2 = *(const float *)(c.depth2 + (int64_t)t * c.depth2_stride), u2 = *(const float *)(c.right2 + (int64_t)t * c.right2_stride);
        r = ss_tri_stereo_eval(a.pairs[b], c.rigs[b], sp, a.scale, n_levels, p1.x, p1.y, k1->octave, d1, u1, p2.x, p2.y, k2->octave, d2, u2);
    }
    c.sinfo[o] = r.info;
    ss_tri_info m;
    m.state = r.info.state, m.cos_parallax = r.info.cos_rays, m.err1_sq = r.info.err1_sq, m.err2_sq = r.info.err2_sq;
    a.info[o] = m;
    if (r.info.state == 0) {
        float4 *po = (float4 *)(a.tmp + o);
        po[0] = make_float4(r.point.x, r.point.y, r.point.z, r.point.nx);
        po[1] = make_float4(r.point.ny, r.point.nz, r.point.min_dist, r.point.max_dist);
    }
}

/* T-C, stereo form.  grid (pairs), 256 threads, after T-B: its summary and the state-0 rows per mode */
__global__ __launch_bounds__(256) void k_tri_stereo_summary(ssk_tri_stereo_call c)
{
    __shared__ int cnt[3];
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x, rows = c.t.rows;
    const ss_tri_summary s = c.t.summary[b];
    const int nq = min(max(s.n_query, 0), rows);
    if (tid < 3) cnt[tid] = 0;
    __syncthreads();
    int n0 = 0, n1 = 0, n2 = 0;
    for (int i = tid; i < nq; i += 256) {
        const ss_tri_stereo_info v = c.sinfo[(size_t)b * rows + i];
        if (v.state == 0) n0 += v.mode == 0, n1 += v.mode == 1, n2 += v.mode == 2;
    }
    if (n0) atomicAdd(&cnt[0], n0);
    if (n1) atomicAdd(&cnt[1], n1);
    if (n2) atomicAdd(&cnt[2], n2);
    __syncthreads();
    if (tid == 0) {
        ss_tri_stereo_summary out;
        out.tri = s;
        out.n_mode[0] = cnt[0], out.n_mode[1] = cnt[1], out.n_mode[2] = cnt[2];
        out.reserved = 0;
        c.ssummary[b] = out;
    }
}

/* T-B.  grid (pairs), SSK_TRI_CHUNK threads */
__global__ __launch_bounds__(SSK_TRI_CHUNK) void k_tri_compact(ssk_tri_call a)
{
    __shared__ int wave_n[SSK_TRI_CHUNK / 64];
    __shared__ int cnt[11];
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x, rows = a.rows;
    const int lane = tid & 63, wave = tid >> 6;
    const gd_frame f = gd_frame_of(a.src, a.frame_error, a.nq, a.nt, rows, b);
    if (tid < 11) cnt[tid] = 0;
    __syncthreads();
    int base = 0;
    for (int c0 = 0; c0 < f.nq; c0 += SSK_TRI_CHUNK) { /* uniform */
        const int i = c0 + tid;
        const size_t o = (size_t)b * rows + i;
        const int st = i < f.nq ? a.info[o].state : -1;
        const bool point = st == 0;
        const unsigned long long mask = __ballot(point);
        if (lane == 0) wave_n[wave] = __popcll(mask);
        if (st >= 0 && st <= 10) atomicAdd(&cnt[st], 1);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int k = 0; k < SSK_TRI_CHUNK / 64; k++) {
            const int n = wave_n[k];
            before += k < wave ? n : 0;
            total += n;
        }
        if (point) {
            const int pos = base + before + __popcll(mask & ((1ull << lane) - 1ull)); /* pos <= i < rows */
            const size_t at = (size_t)b * rows + pos;
            const float4 *pi = (const float4 *)(a.tmp + o);
            float4 *po = (float4 *)(a.points + at);
            po[0] = pi[0], po[1] = pi[1];
            const uint4 *di = (const uint4 *)(a.q_desc + o * SS_DESC_BYTES);
            uint4 *dn = (uint4 *)(a.point_desc + at * SS_DESC_BYTES);
            dn[0] = di[0], dn[1] = di[1];
            *(int2 *)(a.point_rows + at * 2) = make_int2(i, a.idx[o]);
        }
        base += total;
        __syncthreads(); /* wave_n is rewritten */
    }
    if (tid == 0) {
        ss_tri_summary s;
        s.status = f.status;
        s.n_query = f.nq;
        s.n_train = f.nt;
        int m = 0;
        for (int k = 0; k < 11; k++) s.n_state[k] = cnt[k], m += cnt[k];
        s.n_matches = m;
        s.n_points = cnt[0];
        a.n_points[b] = cnt[0];
        a.summary[b] = s;
    }
}

} // namespace

void ssk_epi_search(hipStream_t s, const ssk_guided_call &g, const ssk_epi_call &e)
{
    hipLaunchKernelGGL(k_epi_search, dim3((unsigned)((g.rows + 63) / 64), (unsigned)g.n_frames), dim3(256), 0, s, g, e);
}

void ssk_epi_summary(hipStream_t s, const ssk_guided_call &g, const ssk_epi_call &e)
{
    hipLaunchKernelGGL(k_epi_summary, dim3((unsigned)g.n_frames), dim3(256), 0, s, g, e);
}

void ssk_tri_eval(hipStream_t s, const ssk_tri_call &t)
{
    hipLaunchKernelGGL(k_tri_eval, dim3((unsigned)((t.rows + 255) / 256), (unsigned)t.n_frames), dim3(256), 0, s, t);
}

void ssk_tri_stereo_eval(hipStream_t s, const ssk_tri_stereo_call &c)
{
    hipLaunchKernelGGL(k_tri_stereo_eval, dim3((unsigned)((c.t.rows + 255) / 256), (unsigned)c.t.n_frames), dim3(256), 0, s, c);
}

void ssk_tri_stereo_summary(hipStream_t s, const ssk_tri_stereo_call &c)
{
    hipLaunchKernelGGL(k_tri_stereo_summary, dim3((unsigned)c.t.n_frames), dim3(256), 0, s, c);
}

void ssk_tri_compact(hipStream_t s, const ssk_tri_call &t)
{
    hipLaunchKernelGGL(k_tri_compact, dim3((unsigned)t.n_frames), dim3(SSK_TRI_CHUNK), 0, s, t);
}
