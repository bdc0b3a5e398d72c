/*
 * ss_rectify.hip -- bilinear remap of raw frames through fixed-point rectification maps: a restatement of
 * cv::remap(INTER_LINEAR, BORDER_CONSTANT 0) on 8-bit pixels (include/sendslam_orb.h "rectification").
 *
 *   k_rectify   one workgroup owns a 128 x 8 destination tile of ONE map; a lane owns four consecutive destination pixels
 *               of a row.  It decodes its four map entries once (four clamped tap positions and four integer weights per
 *               pixel, a tap outside the image weighs 0) and keeps them in registers while it loops over the frames of the
 *               batch that use this map, so the map (6 B per pixel) is read once per map and batch while the pixels (1 - 4 B)
 *               are read once per frame.  Taps are plain byte gathers through the vector cache (16 one-byte load instructions
 *               per lane and gray frame: the instruction rate of the cache's address path bounds that form) or, on a
 *               16-byte aligned source, LDS byte reads of the tile's source bounding box, which is staged per frame by
 *               aligned 16-byte loads: 2.9 x faster on a 128-frame batch of 1280 x 720.  The lane's
 *               4 * channels result bytes leave as whole dwords where the address allows it, as bytes on the right edge and
 *               on unaligned destinations.
 *
 * Integer arithmetic only, exact; every global write is a plain vector store.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "ss_kernels.h"

namespace {

#define RC_TILE_W 128 /* 32 lanes x 4 pixels */
#define RC_TILE_H 8
#define RC_BOX_BYTES 10240 /* LDS of the staged form */

struct rc_groups {
    ssk_rectify_group g[SS_MAX_RECTIFY_MAPS];
};

/* STAGED: the source is 16-byte aligned in every respect (host check), so the bounding box of the taps of the tile, taken from
 * the tile's own entries, is staged in LDS by aligned 16-byte loads and the taps are LDS byte reads; a workgroup whose box does not
 * fit (or is empty) runs the gather loop.  The box of frame i + 1 is loaded into registers while frame i is computed. */
template <int CH, bool STAGED>
__global__ __launch_bounds__(256, CH == 1 ? 7 : 1) void k_rectify(rc_groups groups, const int32_t *__restrict__ order, const uint8_t *__restrict__ src,
                                                 int64_t row_stride, int64_t frame_stride, uint8_t *__restrict__ dst,
                                                 int64_t dst_row_stride, int64_t dst_frame_stride, int w, int h, int pitch)
{
    __shared__ __attribute__((aligned(16))) uint8_t box[STAGED ? RC_BOX_BYTES : 16];
    __shared__ int lim[4];
    const int tid = (int)threadIdx.x;
    const int x0 = (int)blockIdx.x * RC_TILE_W + (tid & 31) * 4;
    const int y = (int)blockIdx.y * RC_TILE_H + (tid >> 5);
    const bool active = x0 < w && y < h;
    if (!STAGED && !active) return;
    const ssk_rectify_group grp = groups.g[blockIdx.z];
    /* rows of the map are `pitch` entries apart, a multiple of 4: a lane's four entries are one aligned 16-byte and one aligned
     * 8-byte load; the entries past the width are "outside" records */
    uint32_t xy[4] = {0x80008000u, 0x80008000u, 0x80008000u, 0x80008000u}, ab[4] = {0, 0, 0, 0};
    if (active) {
        const size_t e = (size_t)y * pitch + x0;
        const uint4 xy4 = *(const uint4 *)(grp.xy + e);
        const uint2 ab2 = *(const uint2 *)(grp.ab + e);
        xy[0] = xy4.x, xy[1] = xy4.y, xy[2] = xy4.z, xy[3] = xy4.w;
        ab[0] = ab2.x & 0xFFFFu, ab[1] = ab2.x >> 16, ab[2] = ab2.y & 0xFFFFu, ab[3] = ab2.y >> 16;
    }
    int cx[4][2], cy[4][2];       /* [pixel][first / second tap column or row], clamped into the image */
    uint32_t off[4][4], wt[4][4]; /* [pixel][tap (y, x), (y, x + 1), (y + 1, x), (y + 1, x + 1)] */
#pragma unroll
    for (int p = 0; p < 4; p++) {
        const int ix = (int)(int16_t)(xy[p] & 0xFFFFu), iy = (int)(int16_t)(xy[p] >> 16);
        const int a = (int)(ab[p] & 31u), b = (int)(ab[p] >> 5);
        const bool vx0 = (unsigned)ix < (unsigned)w, vx1 = (unsigned)(ix + 1) < (unsigned)w;
        const bool vy0 = (unsigned)iy < (unsigned)h, vy1 = (unsigned)(iy + 1) < (unsigned)h;
        /* a tap outside the image reads a clamped, valid address and weighs 0 */
        cx[p][0] = min(max(ix, 0), w - 1), cx[p][1] = min(max(ix + 1, 0), w - 1);
        cy[p][0] = min(max(iy, 0), h - 1), cy[p][1] = min(max(iy + 1, 0), h - 1);
        wt[p][0] = vx0 && vy0 ? (uint32_t)((32 - a) * (32 - b) * 32) : 0u;
        wt[p][1] = vx1 && vy0 ? (uint32_t)(a * (32 - b) * 32) : 0u;
        wt[p][2] = vx0 && vy1 ? (uint32_t)((32 - a) * b * 32) : 0u;
        wt[p][3] = vx1 && vy1 ? (uint32_t)(a * b * 32) : 0u;
    }
    /* the box of the taps that weigh something: bytes [bx0, bx0 + bw) of rows [by0, by0 + bh), bx0 and bw multiples of 16 (the
     * host has checked that the row bytes are one, so the box ends inside the row) */
    int bx0 = 0, by0 = 0, bw = 0, bh = 0;
    bool staged = false;
    if (STAGED) {
        if (tid == 0) lim[0] = lim[2] = INT32_MAX, lim[1] = lim[3] = -1;
        __syncthreads();
        int xl = INT32_MAX, xh = -1, yl = INT32_MAX, yh = -1;
#pragma unroll
        for (int p = 0; p < 4; p++)
#pragma unroll
            for (int t = 0; t < 4; t++)
                if (wt[p][t]) {
                    xl = min(xl, cx[p][t & 1]), xh = max(xh, cx[p][t & 1]);
                    yl = min(yl, cy[p][t >> 1]), yh = max(yh, cy[p][t >> 1]);
                }
        if (xh >= 0) {
            atomicMin(&lim[0], xl), atomicMax(&lim[1], xh);
            atomicMin(&lim[2], yl), atomicMax(&lim[3], yh);
        }
        __syncthreads();
        xl = __builtin_amdgcn_readfirstlane(lim[0]), xh = __builtin_amdgcn_readfirstlane(lim[1]);
        yl = __builtin_amdgcn_readfirstlane(lim[2]), yh = __builtin_amdgcn_readfirstlane(lim[3]);
        if (xh >= 0) {
            bx0 = (xl * CH) & ~15, bw = ((xh + 1) * CH - bx0 + 15) & ~15;
            by0 = yl, bh = yh - yl + 1;
            staged = bw * bh <= RC_BOX_BYTES;
        }
    }
#pragma unroll
    for (int p = 0; p < 4; p++)
#pragma unroll
        for (int t = 0; t < 4; t++) {
            if (staged) /* a tap without weight may lie outside the box: it reads the box's first byte */
                off[p][t] = wt[p][t] ? (uint32_t)((cy[p][t >> 1] - by0) * bw + cx[p][t & 1] * CH - bx0) : 0u;
            else
                off[p][t] = (uint32_t)cy[p][t >> 1] * (uint32_t)row_stride + (uint32_t)cx[p][t & 1] * CH;
        }
    const int n_px = min(4, w - x0);
    uint8_t *const d_row = dst + (size_t)y * dst_row_stride + (size_t)x0 * CH;
    /* the lane's 4 * CH result bytes of one frame: taps through `s` (the frame, or the box), out as dwords where d allows it */
    auto remap = [&](const uint8_t *__restrict__ s, uint8_t *d) __attribute__((always_inline)) {
        uint32_t o[CH] = {};
#pragma unroll
        for (int p = 0; p < 4; p++)
#pragma unroll
            for (int c = 0; c < CH; c++) {
                const uint32_t acc = (uint32_t)s[off[p][0] + c] * wt[p][0] + (uint32_t)s[off[p][1] + c] * wt[p][1] +
                                     (uint32_t)s[off[p][2] + c] * wt[p][2] + (uint32_t)s[off[p][3] + c] * wt[p][3];
                const int k = p * CH + c;
                o[k >> 2] |= ((acc + 16384u) >> 15) << (8 * (k & 3));
            }
        if (n_px == 4 && ((uintptr_t)d & 3) == 0) {
#pragma unroll
            for (int k = 0; k < CH; k++) ((uint32_t *)d)[k] = o[k];
        } else {
#pragma unroll
            for (int k = 0; k < 4 * CH; k++)
                if (k < n_px * CH) d[k] = (uint8_t)(o[k >> 2] >> (8 * (k & 3)));
        }
    };
    if (!staged) {
        if (!active) return;
        for (int i = 0; i < grp.count; i++) {
            const int f = order[grp.first + i];
            remap(src + (size_t)f * frame_stride, d_row + (size_t)f * dst_frame_stride);
        }
        return;
    }
    /* chunk j of the box = 16 bytes at box + 16 j: row j / (bw / 16), column j % (bw / 16); a lane moves chunks tid, tid + 256 and
     * tid + 512 (named registers: an indexed array of them would live in scratch) */
    static_assert(RC_BOX_BYTES <= 3 * 256 * 16, "three chunks per lane cover the box");
    const int cpr = bw >> 4, n_chunks = cpr * bh;
    auto chunk_offset = [&](int j) {
        const int row = j / cpr;
        return (uint32_t)(by0 + row) * (uint32_t)row_stride + (uint32_t)(bx0 + (j - row * cpr) * 16);
    };
    const bool has0 = tid < n_chunks, has1 = tid + 256 < n_chunks, has2 = tid + 512 < n_chunks;
    const uint32_t g0 = chunk_offset(tid), g1 = chunk_offset(tid + 256), g2 = chunk_offset(tid + 512);
    uint4 st0 = {}, st1 = {}, st2 = {};
    for (int i = -1; i < grp.count; i++) {
        if (i >= 0) {
            __syncthreads(); /* the taps of the frame before have been read */
            if (has0) *(uint4 *)(box + 16 * tid) = st0;
            if (has1) *(uint4 *)(box + 16 * (tid + 256)) = st1;
            if (has2) *(uint4 *)(box + 16 * (tid + 512)) = st2;
            __syncthreads();
        }
        if (i + 1 < grp.count) { /* the box of the next frame travels while this one is computed */
            const uint8_t *__restrict__ s = src + (size_t)order[grp.first + i + 1] * frame_stride;
            if (has0) st0 = *(const uint4 *)(s + g0);
            if (has1) st1 = *(const uint4 *)(s + g1);
            if (has2) st2 = *(const uint4 *)(s + g2);
        }
        if (i >= 0 && active) remap(box, d_row + (size_t)order[grp.first + i] * dst_frame_stride);
    }
}

} // namespace

void ssk_rectify_fixed(const float *map_x, const float *map_y, int width, int height, int pitch, uint32_t *xy, uint16_t *ab)
{
    auto fixed = [](float v, int *i, int *f) {
        const float t = v * 32.0f;
        const int32_t s = std::isfinite(t) && t >= -2147483648.0f && t < 2147483648.0f ? (int32_t)rintf(t) : INT32_MIN;
        const int32_t q = s >> 5;
        *i = q < -32768 ? -32768 : q > 32767 ? 32767 : q;
        *f = s & 31;
    };
    for (int y = 0; y < height; y++)
        for (int x = 0; x < pitch; x++) {
            int ix = -32768, iy = -32768, a = 0, b = 0; /* the padding of a row: outside */
            if (x < width) {
                fixed(map_x[(size_t)y * width + x], &ix, &a);
                fixed(map_y[(size_t)y * width + x], &iy, &b);
            }
            xy[(size_t)y * pitch + x] = (uint32_t)(uint16_t)(int16_t)ix | (uint32_t)(uint16_t)(int16_t)iy << 16;
            ab[(size_t)y * pitch + x] = (uint16_t)(a | b << 5);
        }
}

void ssk_rectify(hipStream_t s, const ssk_rectify_group *groups, int n_groups, const int32_t *order, const void *src, int channels,
                 int64_t row_stride, int64_t frame_stride, void *dst, int64_t dst_row_stride, int64_t dst_frame_stride, int w, int h)
{
    rc_groups gr{};
    for (int i = 0; i < n_groups; i++) gr.g[i] = groups[i];
    const dim3 grid((unsigned)((w + RC_TILE_W - 1) / RC_TILE_W), (unsigned)((h + RC_TILE_H - 1) / RC_TILE_H), (unsigned)n_groups);
    const int pitch = ssk_rectify_pitch(w);
    const uint8_t *sp = (const uint8_t *)src;
    uint8_t *dp = (uint8_t *)dst;
    /* staged form: every source row starts 16-byte aligned and is a whole number of 16-byte chunks */
    const bool staged = (((uintptr_t)src | (uintptr_t)row_stride | (uintptr_t)frame_stride | (uintptr_t)((int64_t)w * channels)) & 15) == 0;
#define RC_LAUNCH(CH, ST) \
    k_rectify<CH, ST><<<grid, 256, 0, s>>>(gr, order, sp, row_stride, frame_stride, dp, dst_row_stride, dst_frame_stride, w, h, pitch)
    if (channels == 1) {
        if (staged) RC_LAUNCH(1, true); else RC_LAUNCH(1, false);
    } else if (channels == 3) {
        if (staged) RC_LAUNCH(3, true); else RC_LAUNCH(3, false);
    } else {
        if (staged) RC_LAUNCH(4, true); else RC_LAUNCH(4, false);
    }
#undef RC_LAUNCH
}
