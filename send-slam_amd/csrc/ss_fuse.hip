/*
 * ss_fuse.hip -- map-point fusion: ORBmatcher::Fuse(pKF, vpMapPoints, th), its Sim3 form Fuse(pKF, Scw, ...) and the Sim3
 * SearchByProjection(pKF, Scw, vpPoints, vpMatched, th, ratioHamming) (the rule: include/sendslam_orb.h; DESIGN.md "Map-point
 * fusion").  The train frames are binned by k_guided_index (ss_guided.hip) as they are for guided matching and the projection search.
 *
 *   F-A  k_fuse_search  four lanes (a quad) per map point, k_proj_search's shape.  The frame's view is block-uniform and read once;
 *                       every lane of the quad evaluates step 1 itself (ss_fuse_steps.h, the text the host twins compile), then the
 *                       quad walks the cell rows the window meets (gd_walk_window, ss_quad.h).  The record holds x, y, octave and
 *                       row, so the octave, the window and the monocular chi-square need no further load; taken[row] and right[row]
 *                       come next, the 32-byte descriptor only for a row that passed.  Only the best key d << 20 | row is folded
 *   F-B  k_fuse_finish  one workgroup per frame: an occupied row is REPLACE at once; the points that name a free row meet in an LDS
 *                       atomicMin of d1 << 20 | i (gd_settle), the winner is ADD, the others DUPLICATE of the winner; the summary
 *
 * Every float step is a single IEEE operation (-ffp-contract=off).  Every global write is a plain vector store.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ss_constants.h"
#include "ss_fuse_steps.h"
#include "ss_kernels.h"
#include "ss_layout.h"
#include "ss_quad.h"

namespace {

/* F-A.  grid (ceil(point_rows / 64), frames), 256 threads; every row < point_rows is written */
__global__ __launch_bounds__(256) void k_fuse_search(ssk_fuse_call a)
{
    const int b = (int)blockIdx.y, prow = a.point_rows, rows = a.rows;
    const int i = (int)(blockIdx.x * 64 + (threadIdx.x >> 2)), sub = (int)(threadIdx.x & 3);
    const gd_points_frame f = gd_points_frame_of(a.src, a.frame_error, a.np, a.nt, prow, a.rows, b);
    const ss_proj_view view = a.views[b]; /* one address per workgroup */
    const bool live = i < f.np;
    ss_fuse_point o = ss_fuse_rejected(-1);
    if (live) {
        const ss_map_point p = gd_load_point(a.points + (size_t)f.pb * prow + i);
        const int skip = a.p_skip ? a.p_skip[(size_t)b * prow + i] : 0;
        o = ss_fuse_eval(view, p, skip, a.view_cos_limit, a.th, a.scale, a.n_levels);
    }
    const float x = o.u, y = o.v, r = o.radius;
    const bool search = live && o.state == 0 && f.nt > 0 && r > 0.0f;
    uint32_t best = GD_NONE, count = 0;
    if (search) {
        float s_lo, s_hi;
        ss_fuse_scales(a.scale, a.n_levels, o.level, &s_lo, &s_hi);
        const gd_desc q = gd_load_desc(a.p_desc + ((size_t)f.pb * prow + i) * SS_DESC_BYTES);
        const uint32_t *cs = a.cell_start + (size_t)b * (GD_CELLS + 1);
        const gd_rec *recs = (const gd_rec *)a.recs + (size_t)b * rows;
        const uint8_t *td = a.t_desc + (size_t)b * rows * SS_DESC_BYTES;
        const uint8_t *taken = a.t_taken ? a.t_taken + (size_t)b * rows : nullptr;
        const float *right = (a.check_right && a.t_right) ? a.t_right + (size_t)b * rows : nullptr;
        gd_walk_window(cs, recs, a.cols, a.x_max, a.y_max, a.shift, x, y, r, sub, [&](float ex, float ey, int eo, int row) {
            /* row < nt <= rows: k_guided_index wrote it */
            if (ss_fuse_check(o, s_lo, s_hi, ex, ey, eo, row, taken, right, a.chi2_mono, a.chi2_stereo, a.check_right) != 0) return;
            count++;
            best = min(best, (gd_hamming(q, td + (size_t)row * SS_DESC_BYTES) << 20) | (uint32_t)row);
        });
    }
    /* fold the quad: all 64 lanes take part */
#pragma unroll
    for (int m = 1; m <= 2; m <<= 1) gd_fold_step(best, count, m);
    if (i >= prow || sub != 0) return;
    const uint32_t d1 = gd_dist_of(best);
    const size_t at = (size_t)b * prow + i;
    a.idx[at] = (best != GD_NONE && (int)d1 <= a.th_low) ? (int)(best & 0xFFFFFu) : -1;
    a.d1[at] = (uint16_t)d1;
    a.n_cand[at] = (int32_t)count;
    float4 *po = (float4 *)(a.point + at);
    po[0] = make_float4(o.u, o.v, o.u_right, o.dot);
    po[1] = make_float4(o.dist, o.radius, __int_as_float(o.level), __int_as_float(o.state));
}

/* F-B.  grid (frames), GD_FIN threads; thread t owns the point rows t, t + GD_FIN, ... in every loop, so a row's action is written
 * and read again by one thread only */
__global__ __launch_bounds__(GD_FIN) void k_fuse_finish(ssk_fuse_call a)
{
    __shared__ uint32_t keys[GD_KEY_ROWS];
    __shared__ int cnt[5]; /* in view, candidates, add, replace, duplicate */
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x, prow = a.point_rows;
    const gd_points_frame f = gd_points_frame_of(a.src, a.frame_error, a.np, a.nt, prow, a.rows, b);
    const int32_t *idx = a.idx + (size_t)b * prow;
    const uint16_t *d1 = a.d1 + (size_t)b * prow;
    const int32_t *tp = a.t_point ? a.t_point + (size_t)b * a.rows : nullptr;
    ss_fuse_action *act = a.fuse + (size_t)b * prow;
    if (tid < 5) cnt[tid] = 0;
    __syncthreads();
    /* NONE and REPLACE; a point that names a free row is marked ADD until the pass below has found the row's winner */
    int view = 0, cand = 0, n_rep = 0, n_dup = 0;
    for (int i = tid; i < prow; i += GD_FIN) {
        ss_fuse_action o;
        o.action = SS_FUSE_NONE, o.other = -1;
        if (i < f.np) {
            view += a.point[(size_t)b * prow + i].state == 0;
            cand += a.n_cand[(size_t)b * prow + i];
            const int j = idx[i]; /* -1, or a row < nt */
            if (j >= 0) {
                const int id = tp ? tp[j] : -1;
                if (id >= 0) {
                    o.action = SS_FUSE_REPLACE, o.other = id;
                    n_rep++;
                } else {
                    o.action = SS_FUSE_ADD;
                }
            }
        }
        act[i] = o;
    }
    const auto claim = [&](int i) {
        const int j = idx[i];
        return act[i].action == SS_FUSE_ADD ? j : -1;
    };
    const int n_add = gd_settle(keys, d1, f.np, f.nt, tid, claim, [&](int i, uint32_t won) {
        ss_fuse_action o;
        o.action = SS_FUSE_DUPLICATE, o.other = (int32_t)(won & 0xFFFFFu);
        act[i] = o;
        n_dup++;
    });
    if (view) atomicAdd(&cnt[0], view);
    if (cand) atomicAdd(&cnt[1], cand);
    if (n_add) atomicAdd(&cnt[2], n_add);
    if (n_rep) atomicAdd(&cnt[3], n_rep);
    if (n_dup) atomicAdd(&cnt[4], n_dup);
    __syncthreads();
    if (tid == 0) {
        ss_fuse_summary s;
        s.status = f.status;
        s.n_points = f.np;
        s.n_train = f.nt;
        s.n_in_view = cnt[0];
        s.n_candidates = cnt[1];
        s.n_add = cnt[2];
        s.n_replace = cnt[3];
        s.n_duplicate = cnt[4];
        a.summary[b] = s;
    }
}

} // namespace

void ssk_fuse_search(hipStream_t s, const ssk_fuse_call &g)
{
    hipLaunchKernelGGL(k_fuse_search, dim3((unsigned)((g.point_rows + 63) / 64), (unsigned)g.n_frames), dim3(256), 0, s, g);
}

void ssk_fuse_finish(hipStream_t s, const ssk_fuse_call &g)
{
    hipLaunchKernelGGL(k_fuse_finish, dim3((unsigned)g.n_frames), dim3(GD_FIN), 0, s, g);
}
