/*
 * ss_fuse.hip -- map-point fusion: ORBmatcher::Fuse(pKF, vpMapPoints, th), its Sim3 form Fuse(pKF, Scw, ...) and the Sim3
 * SearchByProjection(pKF, Scw, vpPoints, vpMatched, th, ratioHamming) (the rule: include/sendslam_orb.h; DESIGN.md "Map-point
 * fusion").  The train frames are binned by k_guided_index (ss_guided.hip) as they are for guided matching and the projection search.
 *
 *   F-A  k_fuse_search  four lanes (a quad) per map point, k_proj_search's shape.  The frame's view is block-uniform and read once;
 *                       every lane of the quad evaluates step 1 itself (ss_fuse_steps.h, the text the host twins compile), then the
 *                       quad walks the cell rows the window meets.  The record holds x, y, octave and row, so the octave, the window
 *                       and the monocular chi-square need no further load; taken[row] and right[row] come next, the 32-byte
 *                       descriptor only for a row that passed.  Only the best key d << 20 | row is folded
 *   F-B  k_fuse_finish  one workgroup per frame: an occupied row is REPLACE at once; the points that name a free row meet in an LDS
 *                       atomicMin of d1 << 20 | i, the winner is ADD, the others DUPLICATE of the winner; the summary
 *
 * Every float step is a single IEEE operation (-ffp-contract=off).  Every global write is a plain vector store.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ss_constants.h"
#include "ss_fuse_steps.h"
#include "ss_guided_index.h"
#include "ss_kernels.h"
#include "ss_layout.h"

namespace {

/* what the two kernels agree on for frame b: its block of points, its status, both row counts */
struct fu_frame {
    int pb, status, np, nt;
};
__device__ __forceinline__ fu_frame fu_frame_of(const ssk_fuse_call &a, int b)
{
    fu_frame f;
    f.pb = a.src ? a.src[b] : b;
    f.status = a.frame_error ? a.frame_error[b] : 0;
    f.np = f.status ? 0 : gd_clamp_count(a.np[f.pb], a.point_rows);
    f.nt = f.status ? 0 : gd_clamp_count(a.nt[b], a.rows);
    return f;
}

/* F-A.  grid (ceil(point_rows / 64), frames), 256 threads; every row < point_rows is written */
__global__ __launch_bounds__(256) void k_fuse_search(ssk_fuse_call a)
{
    const int b = (int)blockIdx.y, prow = a.point_rows, rows = a.rows;
    const int i = (int)(blockIdx.x * 64 + (threadIdx.x >> 2)), sub = (int)(threadIdx.x & 3);
    const fu_frame f = fu_frame_of(a, b);
    const ss_proj_view view = a.views[b]; /* one address per workgroup */
    const bool live = i < f.np;
    ss_fuse_point o = ss_fuse_rejected(-1);
    if (live) {
        const float4 *pp = (const float4 *)(a.points + (size_t)f.pb * prow + i);
        const float4 pa = pp[0], pb = pp[1];
        ss_map_point p;
        p.x = pa.x, p.y = pa.y, p.z = pa.z, p.nx = pa.w;
        p.ny = pb.x, p.nz = pb.y, p.min_dist = pb.z, p.max_dist = pb.w;
        const int skip = a.p_skip ? a.p_skip[(size_t)b * prow + i] : 0;
        o = ss_fuse_eval(view, p, skip, a.view_cos_limit, a.th, a.scale, a.n_levels);
    }
    const float x = o.u, y = o.v, r = o.radius;
    const bool search = live && o.state == 0 && f.nt > 0 && r > 0.0f;
    uint32_t best = GD_NONE, count = 0;
    if (search) {
        float s_lo, s_hi;
        ss_fuse_scales(a.scale, a.n_levels, o.level, &s_lo, &s_hi);
        const uint4 *qd = (const uint4 *)(a.p_desc + ((size_t)f.pb * prow + i) * SS_DESC_BYTES);
        const uint4 qa = qd[0], qb = qd[1];
        const uint64_t q0 = (uint64_t)qa.x | ((uint64_t)qa.y << 32), q1 = (uint64_t)qa.z | ((uint64_t)qa.w << 32);
        const uint64_t q2 = (uint64_t)qb.x | ((uint64_t)qb.y << 32), q3 = (uint64_t)qb.z | ((uint64_t)qb.w << 32);
        const uint32_t *cs = a.cell_start + (size_t)b * (GD_CELLS + 1);
        const gd_rec *recs = (const gd_rec *)a.recs + (size_t)b * rows;
        const uint8_t *td = a.t_desc + (size_t)b * rows * SS_DESC_BYTES;
        const uint8_t *taken = a.t_taken ? a.t_taken + (size_t)b * rows : nullptr;
        const float *right = (a.check_right && a.t_right) ? a.t_right + (size_t)b * rows : nullptr;
        const int cx0 = gd_bin(x - r, a.x_max, a.shift), cx1 = gd_bin(x + r, a.x_max, a.shift);
        const int cy0 = gd_bin(y - r, a.y_max, a.shift), cy1 = gd_bin(y + r, a.y_max, a.shift);
        for (int cy = cy0; cy <= cy1; cy++) {
            /* the cells cx0 .. cx1 of a grid row are one run of records */
            const uint32_t k0 = cs[cy * a.cols + cx0], k1 = cx1 >= cx0 ? cs[cy * a.cols + cx1 + 1] : k0;
            for (uint32_t k = k0 + (uint32_t)sub; k < k1; k += 4) {
                const uint4 raw = *(const uint4 *)(recs + k);
                const int row = (int)raw.w; /* < nt <= rows: k_guided_index wrote it */
                if (ss_fuse_check(o, s_lo, s_hi, __uint_as_float(raw.x), __uint_as_float(raw.y), (int)raw.z, row, taken, right, a.chi2_mono,
                                  a.chi2_stereo, a.check_right) != 0)
                    continue;
                const uint4 *d = (const uint4 *)(td + (size_t)row * SS_DESC_BYTES);
                const uint4 ta = d[0], tb = d[1];
                const uint32_t dist = (uint32_t)(__popcll(q0 ^ ((uint64_t)ta.x | ((uint64_t)ta.y << 32))) + __popcll(q1 ^ ((uint64_t)ta.z | ((uint64_t)ta.w << 32))) +
                                                 __popcll(q2 ^ ((uint64_t)tb.x | ((uint64_t)tb.y << 32))) + __popcll(q3 ^ ((uint64_t)tb.z | ((uint64_t)tb.w << 32))));
                count++;
                best = min(best, (dist << 20) | (uint32_t)row);
            }
        }
    }
    /* fold the quad: all 64 lanes take part */
#pragma unroll
    for (int m = 1; m <= 2; m <<= 1) {
        const uint32_t ob = (uint32_t)__shfl_xor((int)best, m), oc = (uint32_t)__shfl_xor((int)count, m);
        best = min(best, ob);
        count += oc;
    }
    if (i >= prow || sub != 0) return;
    const uint32_t d1 = best == GD_NONE ? 0xFFFFu : best >> 20;
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
    const fu_frame f = fu_frame_of(a, b);
    const int32_t *idx = a.idx + (size_t)b * prow;
    const uint16_t *d1 = a.d1 + (size_t)b * prow;
    const int32_t *tp = a.t_point ? a.t_point + (size_t)b * a.rows : nullptr;
    ss_fuse_action *act = a.fuse + (size_t)b * prow;
    if (tid < 5) cnt[tid] = 0;
    __syncthreads();
    /* NONE and REPLACE; a point that names a free row is marked ADD until the passes below have found the row's winner */
    int view = 0, cand = 0, n_add = 0, n_rep = 0, n_dup = 0;
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
    for (int base = 0; base < f.nt; base += GD_KEY_ROWS) { /* uniform */
        const int len = min(GD_KEY_ROWS, f.nt - base);
        for (int k = tid; k < len; k += GD_FIN) keys[k] = GD_NONE;
        __syncthreads();
        for (int i = tid; i < f.np; i += GD_FIN) {
            const int j = idx[i] - base;
            if (j >= 0 && j < len && act[i].action == SS_FUSE_ADD) atomicMin(&keys[j], ((uint32_t)d1[i] << 20) | (uint32_t)i);
        }
        __syncthreads();
        for (int i = tid; i < f.np; i += GD_FIN) {
            const int j = idx[i] - base;
            if (j >= 0 && j < len && act[i].action == SS_FUSE_ADD) {
                const uint32_t won = keys[j];
                if (won == (((uint32_t)d1[i] << 20) | (uint32_t)i)) {
                    n_add++;
                } else {
                    ss_fuse_action o;
                    o.action = SS_FUSE_DUPLICATE, o.other = (int32_t)(won & 0xFFFFFu);
                    act[i] = o;
                    n_dup++;
                }
            }
        }
        __syncthreads();
    }
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
