/*
 * ss_undistort.hip -- Frame's keypoint post-processing: mvKeysUn (Frame::UndistortKeyPoints) and the RGB-D depth lookup
 * (Frame::ComputeStereoFromRGBD).  The rules: include/sendslam_orb.h; DESIGN.md "Undistorted keypoints".  Every step is the text of
 * ss_undistort_steps.h, which the host twins compile too.
 *
 *   k_undistort     one lane per keypoint row, a frame per blockIdx.y.  The frame's camera (eight doubles and the zero-distortion
 *                   flag) is read at an address that depends on blockIdx.y alone: uniform per block.  x and y move as one 8-byte load
 *                   and one 8-byte store; the raw save of the in-place form is one more 8-byte store; the out-of-place form copies
 *                   the other 16 bytes of the record as two 8-byte moves.  Rows at or past the frame's count are not touched.
 *   k_depth_begin   one lane per frame: status and row count of the frame's summary, its two counters cleared.
 *   k_depth         one lane per row of both planes, a frame per blockIdx.y: the sample at the truncated raw position, depth and
 *                   right coordinate, -1.0f for rows without a depth and for rows past the count.  A wave counts its rows with a
 *                   depth and its close rows by ballot; one lane adds them to the summary (integer atomics: exact and order-free).
 *
 * Every global write is a plain vector store or a vector integer atomic; there is no grid-wide barrier.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ss_kernels.h"
#include "ss_undistort_steps.h"

namespace {

static_assert(sizeof(ss_keypoint) == 24 && sizeof(ss_undist_cam) == 72 && sizeof(ss_depth_params) == 16 && sizeof(ss_depth_summary) == 16,
              "the layouts of the header");

constexpr int UNDIST_THREADS = 256;

/* the rows of frame `frame` that count: the told count clamped to 0 .. rows, 0 for a frame whose error is set */
__device__ __forceinline__ int frame_rows(const int32_t *n_kp, const int32_t *frame_error, int frame, int rows)
{
    if (frame_error && frame_error[frame] != 0) return 0;
    return ss_undist_clamp(n_kp[frame], rows);
}

template <bool SAVE_RAW, bool COPY> __global__ __launch_bounds__(UNDIST_THREADS) void k_undistort(ssk_undistort_call g)
{
    const int frame = (int)blockIdx.y, row = (int)(blockIdx.x * UNDIST_THREADS + threadIdx.x);
    if (row >= frame_rows(g.n_kp, g.frame_error, frame, g.rows)) return;
    const ss_undist_cam cam = g.cams[frame];
    const size_t at = (size_t)frame * (size_t)g.rows + (size_t)row;
    /* a record is 24 bytes on a 16-byte aligned base: three 8-byte words, the first is (x, y) */
    const float2 *in = (const float2 *)(g.kp + at);
    const float2 xy = in[0];
    float2 un;
    ss_undist_point(cam, xy.x, xy.y, &un.x, &un.y);
    if (SAVE_RAW) g.raw_xy[at] = xy;
    float2 *out = (float2 *)(g.kp_out + at);
    if (COPY) {
        const float2 w1 = in[1], w2 = in[2];
        out[1] = w1;
        out[2] = w2;
    }
    out[0] = un;
}

__global__ __launch_bounds__(UNDIST_THREADS) void k_depth_begin(ssk_depth_call g)
{
    const int frame = (int)(blockIdx.x * UNDIST_THREADS + threadIdx.x);
    if (frame >= g.n_frames) return;
    ss_depth_summary s;
    s.status = g.frame_error ? g.frame_error[frame] : 0;
    s.n_kp = frame_rows(g.n_kp, g.frame_error, frame, g.rows);
    s.n_depth = s.n_close = 0;
    g.summary[frame] = s;
}

__global__ __launch_bounds__(UNDIST_THREADS) void k_depth(ssk_depth_call g)
{
    const int frame = (int)blockIdx.y, row = (int)(blockIdx.x * UNDIST_THREADS + threadIdx.x);
    const bool live = row < g.rows;
    const size_t at = (size_t)frame * (size_t)g.rows + (size_t)(live ? row : 0);
    bool have = false;
    float d = 0.0f, x_un = 0.0f;
    if (live && row < frame_rows(g.n_kp, g.frame_error, frame, g.rows)) {
        float2 raw;
        if (g.raw_xy) raw = g.raw_xy[at];
        else raw = *(const float2 *)(g.kp_raw + at);
        x_un = ((const float *)(g.kp_un + at))[0];
        have = ss_depth_sample(g.depth + (int64_t)frame * g.frame_stride, g.width, g.height, g.row_stride, g.p.depth_type, g.inv, g.scale_float, raw.x, raw.y, &d);
    }
    float right, depth;
    ss_depth_row(have, d, x_un, g.p.bf, &right, &depth);
    if (live) {
        g.right[at] = right;
        g.depth_out[at] = depth;
    }
    /* depth > 0 only for a row inside the count; a dead lane has depth -1 */
    const bool has_depth = depth > 0.0f, close = has_depth && depth < g.p.close_limit;
    const unsigned long long m_depth = __ballot(has_depth), m_close = __ballot(close);
    if ((threadIdx.x & 63) == 0) {
        if (m_depth) atomicAdd(&g.summary[frame].n_depth, (int32_t)__popcll(m_depth));
        if (m_close) atomicAdd(&g.summary[frame].n_close, (int32_t)__popcll(m_close));
    }
}

} // namespace

void ssk_undistort(hipStream_t s, const ssk_undistort_call &g)
{
    if (g.n_frames <= 0 || g.rows <= 0) return;
    const dim3 grid((unsigned)((g.rows + UNDIST_THREADS - 1) / UNDIST_THREADS), (unsigned)g.n_frames), block(UNDIST_THREADS);
    const bool copy = (const void *)g.kp_out != (const void *)g.kp;
    if (g.raw_xy) hipLaunchKernelGGL((k_undistort<true, false>), grid, block, 0, s, g); /* in place: the caller gives kp_out == kp */
    else if (copy) hipLaunchKernelGGL((k_undistort<false, true>), grid, block, 0, s, g);
    else hipLaunchKernelGGL((k_undistort<false, false>), grid, block, 0, s, g);
}

void ssk_depth(hipStream_t s, const ssk_depth_call &g)
{
    if (g.n_frames <= 0 || g.rows <= 0) return;
    hipLaunchKernelGGL(k_depth_begin, dim3((unsigned)((g.n_frames + UNDIST_THREADS - 1) / UNDIST_THREADS)), dim3(UNDIST_THREADS), 0, s, g);
    const dim3 grid((unsigned)((g.rows + UNDIST_THREADS - 1) / UNDIST_THREADS), (unsigned)g.n_frames);
    hipLaunchKernelGGL(k_depth, grid, dim3(UNDIST_THREADS), 0, s, g);
}
