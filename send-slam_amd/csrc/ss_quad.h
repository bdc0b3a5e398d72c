/* ss_quad.h -- the one text of what the quad search kernels and their finishers share (device only).  Four lanes (a quad) serve one
 * query row or map point in k_guided_search (ss_guided.hip), k_bow_search (ss_bow.hip), k_proj_search (ss_proj.hip), k_epi_search
 * (ss_epi.hip) and k_fuse_search (ss_fuse.hip); k_guided_finish, k_proj_finish and k_fuse_finish settle the train rows that several
 * of them name.  Here: the cell record and the binning of k_guided_index, the 32-byte descriptor and its Hamming distance, the key
 * d << 20 | row, the frame rules, the two walks (the cell rows of a window, the run of a node), the fold over the quad and the
 * conflict pass.  What a kernel does with a candidate stays in the kernel.  k_guided_search walks its window and k_guided_finish
 * settles its conflicts in their own text (the same statements; DESIGN.md section 14 says why). */
#ifndef SS_QUAD_H
#define SS_QUAD_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ss_constants.h"
#include "ss_kernels.h"

#define GD_CELLS SSK_GUIDED_MAX_CELLS
#define GD_KEY_ROWS 8192 /* train rows whose conflict keys are in LDS at a time */
#define GD_FIN 1024     /* threads of a finishing kernel */
#define GD_NONE 0xFFFFFFFFu

struct gd_rec { /* 16 bytes: one dwordx4 */
    float x, y;
    int32_t oct, row;
};

/* any float -> a valid cell coordinate: NaN and negatives land in 0, +inf and huge values in the last one; non-decreasing */
__device__ __forceinline__ int gd_bin(float v, float v_max, int shift)
{
    const int c = (int)fminf(fmaxf(v, 0.0f), v_max); /* fmaxf(NaN, 0) is 0 */
    return min(max(c, 0), (int)v_max) >> shift;       /* the bound again on the integer: an index, whatever the float was */
}

__device__ __forceinline__ int gd_clamp_count(int n, int rows) { return min(max(n, 0), rows); }

/* ---- the descriptor ---- */

struct gd_desc {
    uint64_t q0, q1, q2, q3;
};

__device__ __forceinline__ gd_desc gd_load_desc(const uint8_t *row)
{
    const uint4 *qd = (const uint4 *)row;
    const uint4 qa = qd[0], qb = qd[1];
    gd_desc q;
    q.q0 = (uint64_t)qa.x | ((uint64_t)qa.y << 32), q.q1 = (uint64_t)qa.z | ((uint64_t)qa.w << 32);
    q.q2 = (uint64_t)qb.x | ((uint64_t)qb.y << 32), q.q3 = (uint64_t)qb.z | ((uint64_t)qb.w << 32);
    return q;
}

__device__ __forceinline__ uint32_t gd_hamming(uint64_t q0, uint64_t q1, uint64_t q2, uint64_t q3, const uint8_t *row)
{
    const uint4 ta = ((const uint4 *)row)[0], tb = ((const uint4 *)row)[1];
    return (uint32_t)(__popcll(q0 ^ ((uint64_t)ta.x | ((uint64_t)ta.y << 32))) + __popcll(q1 ^ ((uint64_t)ta.z | ((uint64_t)ta.w << 32))) +
                      __popcll(q2 ^ ((uint64_t)tb.x | ((uint64_t)tb.y << 32))) + __popcll(q3 ^ ((uint64_t)tb.z | ((uint64_t)tb.w << 32))));
}
__device__ __forceinline__ uint32_t gd_hamming(const gd_desc &q, const uint8_t *row) { return gd_hamming(q.q0, q.q1, q.q2, q.q3, row); }

/* the distance of a key d << 20 | row */
__device__ __forceinline__ uint32_t gd_dist_of(uint32_t key) { return key == GD_NONE ? 0xFFFFu : key >> 20; }

__device__ __forceinline__ ss_map_point gd_load_point(const ss_map_point *row)
{
    const float4 *pp = (const float4 *)row;
    const float4 pa = pp[0], pb = pp[1];
    ss_map_point p;
    p.x = pa.x, p.y = pa.y, p.z = pa.z, p.nx = pa.w;
    p.ny = pb.x, p.nz = pb.y, p.min_dist = pb.z, p.max_dist = pb.w;
    return p;
}

/* ---- the frame rules: what the kernels of a call agree on for frame b ---- */

/* a pair of frames: its train frame, its status, both row counts */
struct gd_frame {
    int t, status, nq, nt;
};
__device__ __forceinline__ gd_frame gd_frame_of(const int32_t *src, const int32_t *frame_error, const int32_t *nq, const int32_t *nt, int rows, int b)
{
    gd_frame f;
    f.t = src ? src[b] : b;
    f.status = 0;
    if (frame_error) {
        f.status = frame_error[b];
        if (f.status == 0 && f.t >= 0) f.status = frame_error[f.t];
    }
    f.nq = f.status ? 0 : gd_clamp_count(nq[b], rows);
    f.nt = (f.status || f.t < 0) ? 0 : gd_clamp_count(nt[f.t], rows);
    return f;
}

/* a block of map points against a frame: the block, the status, both row counts */
struct gd_points_frame {
    int pb, status, np, nt;
};
__device__ __forceinline__ gd_points_frame gd_points_frame_of(const int32_t *src, const int32_t *frame_error, const int32_t *np, const int32_t *nt,
                                                              int point_rows, int rows, int b)
{
    gd_points_frame f;
    f.pb = src ? src[b] : b;
    f.status = frame_error ? frame_error[b] : 0;
    f.np = f.status ? 0 : gd_clamp_count(np[f.pb], point_rows);
    f.nt = f.status ? 0 : gd_clamp_count(nt[b], rows);
    return f;
}

/* ---- the walks: lane `sub` of the quad takes every fourth candidate ---- */

/* the records of the cells that the window x -+ r, y -+ r meets: visit(ex, ey, octave, row).  The cells cx0 .. cx1 of a grid row are
 * one run of records; a NaN bound can make it empty or reversed */
template <typename F>
__device__ __forceinline__ void gd_walk_window(const uint32_t *cs, const gd_rec *recs, int cols, float x_max, float y_max, int shift, float x, float y,
                                               float r, int sub, const F &visit)
{
    const int cx0 = gd_bin(x - r, x_max, shift), cx1 = gd_bin(x + r, x_max, shift);
    const int cy0 = gd_bin(y - r, y_max, shift), cy1 = gd_bin(y + r, y_max, shift);
    for (int cy = cy0; cy <= cy1; cy++) {
        const uint32_t k0 = cs[cy * cols + cx0], k1 = cx1 >= cx0 ? cs[cy * cols + cx1 + 1] : k0;
        for (uint32_t k = k0 + (uint32_t)sub; k < k1; k += 4) {
            const uint4 raw = *(const uint4 *)(recs + k);
            visit(__uint_as_float(raw.x), __uint_as_float(raw.y), (int)raw.z, (int)raw.w);
        }
    }
}

/* the rows of `node` in a frame's index of m ascending keys node << 32 | row: visit(row) */
template <typename F>
__device__ __forceinline__ void gd_walk_node(const uint64_t *keys, int m, int node, int sub, const F &visit)
{
    int lo = 0, hi = m; /* the first key of the node, if it has any */
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((uint32_t)(keys[mid] >> 32) < (uint32_t)node) lo = mid + 1;
        else hi = mid;
    }
    for (int k = lo + sub; k < m; k += 4) {
        const uint64_t key64 = keys[k];
        if ((uint32_t)(key64 >> 32) != (uint32_t)node) break;
        visit((int)(uint32_t)key64);
    }
}

/* ---- the fold over the quad: all 64 lanes take part ---- */

/* one step, with lane ^ m: the lower key and the sum of the counts stay, the higher key is returned */
__device__ __forceinline__ uint32_t gd_fold_step(uint32_t &best, uint32_t &count, int m)
{
    const uint32_t ob = (uint32_t)__shfl_xor((int)best, m), oc = (uint32_t)__shfl_xor((int)count, m);
    const uint32_t loser = max(best, ob);
    best = min(best, ob);
    count += oc;
    return loser;
}

/* best key, second-best distance and count, the whole fold.  Two lanes fold as two train chunks do: the second best is the minimum
 * over the loser's best and both seconds.  (Not on gd_fold_step: in this order of the three exchanges k_guided_search compiles to the
 * code it had) */
__device__ __forceinline__ void gd_fold_second(uint32_t &best, uint32_t &second, uint32_t &count)
{
#pragma unroll
    for (int m = 1; m <= 2; m <<= 1) {
        const uint32_t ob = (uint32_t)__shfl_xor((int)best, m), os = (uint32_t)__shfl_xor((int)second, m), oc = (uint32_t)__shfl_xor((int)count, m);
        second = min(min(second, os), gd_dist_of(max(best, ob)));
        best = min(best, ob);
        count += oc;
    }
}

/* ---- the conflict pass of a finishing kernel (GD_FIN threads, all of them call it) ---- */

/* Of the nq rows that claim the same one of nt train rows, the lowest d1 << 20 | i wins.  claim(i): the train row that i claims, or
 * -1; lose(i, key): what a loser does, given the winner's key.  Thread t owns the rows t, t + GD_FIN, ... in both; keys: GD_KEY_ROWS
 * words of LDS, the train rows pass through them GD_KEY_ROWS at a time.  Returns how many of this thread's rows won */
template <typename C, typename L>
__device__ __forceinline__ int gd_settle(uint32_t *keys, const uint16_t *d1, int nq, int nt, int tid, C claim, L lose)
{
    int won = 0;
    for (int base = 0; base < nt; base += GD_KEY_ROWS) { /* uniform */
        const int len = min(GD_KEY_ROWS, nt - base);
        for (int k = tid; k < len; k += GD_FIN) keys[k] = GD_NONE;
        __syncthreads();
        for (int i = tid; i < nq; i += GD_FIN) {
            const int j = claim(i) - base;
            if (j >= 0 && j < len && claim(i) >= 0) atomicMin(&keys[j], ((uint32_t)d1[i] << 20) | (uint32_t)i);
        }
        __syncthreads();
        for (int i = tid; i < nq; i += GD_FIN) {
            const int j = claim(i) - base;
            if (j >= 0 && j < len && claim(i) >= 0) {
                const uint32_t top = keys[j];
                if (top == (((uint32_t)d1[i] << 20) | (uint32_t)i)) won++;
                else lose(i, top);
            }
        }
        __syncthreads();
    }
    return won;
}

#endif
