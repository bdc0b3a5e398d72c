/* ss_guided_index.h -- what the kernels that read the cell index of k_guided_index (ss_guided.hip, ss_proj.hip) share with it:
 * the record and the binning of a coordinate. */
#ifndef SS_GUIDED_INDEX_H
#define SS_GUIDED_INDEX_H

#include <hip/hip_runtime.h>
#include <stdint.h>

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

#endif
