/*
 * ss_proj.hip -- map-point projection search: Tracking::SearchLocalPoints, i.e. Frame::isInFrustum, the predicted pyramid level
 * and ORBmatcher::SearchByProjection(Frame&, vector<MapPoint*>&, th) (the rule: include/sendslam_orb.h; DESIGN.md "Projection
 * search").  The train frames are binned by k_guided_index (ss_guided.hip) as they are for guided matching.
 *
 *   P-A  k_proj_search  four lanes (a quad) per map point.  The frame's view is block-uniform and read once; every lane of the
 *                       quad evaluates frustum, level and window itself (ss_proj_steps.h, the text the host twin compiles), then
 *                       the quad walks the cell rows the window meets (gd_walk_window, ss_quad.h), with the taken mask and the
 *                       right-eye test on top.  Best and second best are folded as full keys d << 20 | row, because the octave
 *                       of the second best decides whether the ratio test counts
 *   P-B  k_proj_finish  one workgroup per frame: conflicts by an LDS atomicMin of d1 << 20 | i per train row (gd_settle), the summary
 *
 * Every float step is a single IEEE operation (-ffp-contract=off).  Every global write is a plain vector store.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ss_constants.h"
#include "ss_kernels.h"
#include "ss_layout.h"
#include "ss_proj_steps.h"
#include "ss_quad.h"

namespace {

/* P-A.  grid (ceil(point_rows / 64), frames), 256 threads; every row < point_rows is written */
__global__ __launch_bounds__(256) void k_proj_search(ssk_proj_call a)
{
    const int b = (int)blockIdx.y, prow = a.point_rows, rows = a.rows;
    const int i = (int)(blockIdx.x * 64 + (threadIdx.x >> 2)), sub = (int)(threadIdx.x & 3);
    const gd_points_frame f = gd_points_frame_of(a.src, a.frame_error, a.np, a.nt, prow, a.rows, b);
    const ss_proj_view view = a.views[b]; /* one address per workgroup */
    const bool live = i < f.np;
    ss_proj_point o = ss_proj_rejected(-1);
    if (live) {
        const ss_map_point p = gd_load_point(a.points + (size_t)f.pb * prow + i);
        o = ss_proj_eval(view, p, a.view_cos_limit, a.th, a.far_limit, a.scale, a.n_levels);
    }
    const float x = o.u, y = o.v, r = o.radius;
    const int olo = o.level - 1, ohi = o.level;
    const bool search = live && o.state == 0 && f.nt > 0 && r > 0.0f;
    uint32_t best = GD_NONE, second = GD_NONE, count = 0;
    const ss_keypoint *tkp = a.t_kp + (size_t)b * rows;
    if (search) {
        const gd_desc q = gd_load_desc(a.p_desc + ((size_t)f.pb * prow + i) * SS_DESC_BYTES);
        const uint32_t *cs = a.cell_start + (size_t)b * (GD_CELLS + 1);
        const gd_rec *recs = (const gd_rec *)a.recs + (size_t)b * rows;
        const uint8_t *td = a.t_desc + (size_t)b * rows * SS_DESC_BYTES;
        const uint8_t *taken = a.t_taken ? a.t_taken + (size_t)b * rows : nullptr;
        const float *right = a.check_right ? a.t_right + (size_t)b * rows : nullptr;
        gd_walk_window(cs, recs, a.cols, a.x_max, a.y_max, a.shift, x, y, r, sub, [&](float ex, float ey, int eo, int row) {
            if (eo < olo || eo > ohi) return;
            if (!(fabsf(ex - x) < r) || !(fabsf(ey - y) < r)) return;
            if (taken && taken[row] != 0) return;
            if (right) {
                const float ur = right[row];
                if (ur > 0.0f && !(fabsf(o.u_right - ur) <= r)) return;
            }
            const uint32_t key = (gd_hamming(q, td + (size_t)row * SS_DESC_BYTES) << 20) | (uint32_t)row;
            count++;
            if (key < best) {
                second = best;
                best = key;
            } else {
                second = min(second, key);
            }
        });
    }
    /* fold the quad: all 64 lanes take part.  The lanes hold different rows, so their keys differ: the second best of two lanes
     * is the lowest of the losing best and both seconds */
#pragma unroll
    for (int m = 1; m <= 2; m <<= 1) {
        const uint32_t os = (uint32_t)__shfl_xor((int)second, m);
        second = min(min(second, os), gd_fold_step(best, count, m));
    }
    if (i >= prow || sub != 0) return;
    const uint32_t d1 = gd_dist_of(best), d2 = gd_dist_of(second);
    const int row1 = best == GD_NONE ? -1 : (int)(best & 0xFFFFFu), row2 = second == GD_NONE ? -1 : (int)(second & 0xFFFFFu);
    const int lvl1 = row1 >= 0 ? tkp[row1].octave : -1, lvl2 = row2 >= 0 ? tkp[row2].octave : -1;
    const bool accept = row1 >= 0 && (int)d1 <= a.th_high && !(a.rden != 0 && lvl1 == lvl2 && (int)d1 * a.rden > (int)d2 * a.rnum);
    const size_t at = (size_t)b * prow + i;
    a.idx[at] = accept ? row1 : -1;
    a.d1[at] = (uint16_t)d1;
    a.d2[at] = (uint16_t)d2;
    a.n_cand[at] = (int32_t)count;
    float4 *po = (float4 *)(a.proj + at);
    po[0] = make_float4(o.u, o.v, o.u_right, o.view_cos);
    po[1] = make_float4(o.dist, o.radius, __int_as_float(o.level), __int_as_float(o.state));
}

/* P-B.  grid (frames), GD_FIN threads; thread t owns the point rows t, t + GD_FIN, ... in every pass, so a row's idx is read and
 * rewritten by one thread only */
__global__ __launch_bounds__(GD_FIN) void k_proj_finish(ssk_proj_call a)
{
    __shared__ uint32_t keys[GD_KEY_ROWS];
    __shared__ int cnt[4]; /* in view, candidates, accepted, unique */
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x, prow = a.point_rows;
    const gd_points_frame f = gd_points_frame_of(a.src, a.frame_error, a.np, a.nt, prow, a.rows, b);
    int32_t *idx = a.idx + (size_t)b * prow;
    const uint16_t *d1 = a.d1 + (size_t)b * prow;
    if (tid < 4) cnt[tid] = 0;
    __syncthreads();
    int view = 0, cand = 0, acc = 0;
    for (int i = tid; i < f.np; i += GD_FIN) {
        view += a.proj[(size_t)b * prow + i].state == 0;
        cand += a.n_cand[(size_t)b * prow + i];
        acc += idx[i] >= 0;
    }
    if (view) atomicAdd(&cnt[0], view);
    if (cand) atomicAdd(&cnt[1], cand);
    if (acc) atomicAdd(&cnt[2], acc);
    if (a.one_to_one) gd_settle(keys, d1, f.np, f.nt, tid, [&](int i) { return idx[i]; }, [&](int i, uint32_t) { idx[i] = -1; });
    int uniq = 0;
    for (int i = tid; i < f.np; i += GD_FIN) uniq += idx[i] >= 0;
    if (uniq) atomicAdd(&cnt[3], uniq);
    __syncthreads();
    if (tid == 0) {
        ss_proj_summary s;
        s.status = f.status;
        s.n_points = f.np;
        s.n_train = f.nt;
        s.n_in_view = cnt[0];
        s.n_candidates = cnt[1];
        s.n_accepted = cnt[2];
        s.n_unique = cnt[3];
        s.reserved = 0;
        a.summary[b] = s;
    }
}

} // namespace

void ssk_proj_search(hipStream_t s, const ssk_proj_call &g)
{
    hipLaunchKernelGGL(k_proj_search, dim3((unsigned)((g.point_rows + 63) / 64), (unsigned)g.n_frames), dim3(256), 0, s, g);
}

void ssk_proj_finish(hipStream_t s, const ssk_proj_call &g)
{
    hipLaunchKernelGGL(k_proj_finish, dim3((unsigned)g.n_frames), dim3(GD_FIN), 0, s, g);
}
