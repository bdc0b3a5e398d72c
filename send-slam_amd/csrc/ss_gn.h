/* ss_gn.h -- the one text of what the gather and solve kernels of the Gauss-Newton problems share (device only; DESIGN.md
 * "Gauss-Newton core"): the compaction of a chunk of rows by ballot and prefix sums (k_sim3_gather in ss_sim3.hip, k_pose_gather in
 * ss_pose.hip, k_sim3opt_gather in ss_sim3opt.hip), the fold of a wave by halving and the sum of a four-wave workgroup through two
 * LDS buffers in turn (k_pose_solve, k_sim3opt_solve, k_sim3_mutual).  The round and step loops stay in the kernels: their rules
 * differ.  The arithmetic of a step is ss_gn_steps.h's. */
#ifndef SS_GN_H
#define SS_GN_H

#include <hip/hip_runtime.h>

#include "ss_gn_steps.h"

/* One chunk of a gather: every thread of the CHUNK (one row each) brings keep; wave_n is the workgroup's LDS array of CHUNK / 64.
 * before: the kept rows of the waves before this one; total: the chunk's count (the same in every thread).  The caller adds total
 * to its running base and puts one barrier before the next chunk: wave_n is rewritten */
struct gn_chunk {
    unsigned long long mask; /* the wave's ballot of keep */
    int before, total;
};

template <int CHUNK> __device__ __forceinline__ gn_chunk gn_chunk_compact(bool keep, int *wave_n)
{
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    gn_chunk c;
    c.mask = __ballot(keep);
    if (lane == 0) wave_n[wave] = __popcll(c.mask);
    __syncthreads();
    c.before = 0, c.total = 0;
#pragma unroll
    for (int k = 0; k < CHUNK / 64; k++) {
        const int n = wave_n[k];
        c.before += k < wave ? n : 0;
        c.total += n;
    }
    return c;
}

/* the number of a kept row, base rows being kept in the chunks before: rows are numbered in ascending order.  Call it inside the
 * branch on keep: formed ahead of it, k_sim3_gather takes 17 more VGPRs (DESIGN.md "Gauss-Newton core") */
__device__ __forceinline__ int gn_chunk_pos(const gn_chunk &c, int base)
{
    return base + c.before + __popcll(c.mask & ((1ull << ((int)threadIdx.x & 63)) - 1ull));
}

/* a[l] += a[l + h], h = 32 .. 1: lane 0 ends with the group's sum */
__device__ __forceinline__ double gn_wave_fold(double v)
{
#pragma unroll
    for (int h = 32; h >= 1; h >>= 1) v = v + __shfl_down(v, h);
    return v;
}

__device__ __forceinline__ int gn_wave_fold(int v)
{
#pragma unroll
    for (int h = 32; h >= 1; h >>= 1) v += __shfl_down(v, h);
    return v;
}

/* The tree of NS sums over a workgroup of SS_GN_SLOTS threads: every wave folds, lane 0 writes its results to part[*buf][wave], one
 * barrier, every thread combines the four.  *buf flips: the next tree writes the other buffer, so one barrier per tree is enough
 * (a wave can be one tree ahead of another, never two) */
template <int NS> __device__ __forceinline__ void gn_block_sum(double (&v)[NS], double (*part)[4][NS], int *buf)
{
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
#pragma unroll
    for (int s = 0; s < NS; s++) v[s] = gn_wave_fold(v[s]);
    if (lane == 0) {
#pragma unroll
        for (int s = 0; s < NS; s++) part[*buf][wave][s] = v[s];
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < NS; s++) v[s] = ss_gn_combine(part[*buf][0][s], part[*buf][1][s], part[*buf][2][s], part[*buf][3][s]);
    *buf ^= 1;
}

/* the same tree for one double and one count in one barrier: the cost and the inliers of a classification */
template <int NS> __device__ __forceinline__ void gn_block_sum(double *v, int *n, double (*part)[4][NS], int (*part_n)[4], int *buf)
{
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const double fv = gn_wave_fold(*v);
    const int fn = gn_wave_fold(*n);
    if (lane == 0) part[*buf][wave][0] = fv, part_n[*buf][wave] = fn;
    __syncthreads();
    *v = ss_gn_combine(part[*buf][0][0], part[*buf][1][0], part[*buf][2][0], part[*buf][3][0]);
    *n = (part_n[*buf][0] + part_n[*buf][1]) + (part_n[*buf][2] + part_n[*buf][3]);
    *buf ^= 1;
}

/* the same tree for one count */
__device__ __forceinline__ int gn_block_sum(int n, int (*part_n)[4], int *buf)
{
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    n = gn_wave_fold(n);
    if (lane == 0) part_n[*buf][wave] = n;
    __syncthreads();
    n = (part_n[*buf][0] + part_n[*buf][1]) + (part_n[*buf][2] + part_n[*buf][3]);
    *buf ^= 1;
    return n;
}

#endif
