/* ss_fast_queue.h -- the 16-bit entries of k_fast_score's queue (ss_kernels.hip).
 *
 * A thread of the compass test owns four pixels (i = 0 .. 3, columns 4 tx + i) of four rows (half hf, row rr: region row
 * 32 hf + 2 ty + rr) and holds their sixteen verdicts in ONE word: compass_row() leaves the verdicts of a row in bits 8 i + 7,
 * and the row's word goes in shifted right by ftq_shift(hf, rr), so that the verdict of (i, rr, hf) is bit
 *     k = 8 i + 2 hf + rr.
 * An entry holds a position (ly, lx), -1 <= ly, lx <= 64, as
 *     bit 0       r        }
 *     bit 1       f        }  ly + 2 = 2 q + r + 32 f
 *     bits 11-15  q        }
 *     bit 2       FTQ_RING: the position is on the 1-px ring around the region (or one of its four corner pixels), not inside
 *     bits 3-9    lx + 1
 *     bit 10      clear
 * A REGION entry is ftq_code0(ty, tx) + k -- q = ty + 1, lx + 1 = 4 tx + 1 + i (the sum does not leave its field), r = rr, f = hf:
 * the loop that writes the queue adds the index of the bit it found to a constant of its thread and does nothing else.  A RING
 * entry spells its coordinates out in the same fields under FTQ_RING, so phase 2 decodes both kinds with the same six
 * instructions and asks for the kind only where it keeps a corner.  q <= 17, so no entry is FTQ_VOID (0xFFFF). */
#ifndef SS_FAST_QUEUE_H
#define SS_FAST_QUEUE_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define FTQ_HD __host__ __device__ constexpr
#else
#define FTQ_HD constexpr
#endif

#define FTQ_RING 0x4u
#define FTQ_VOID 0xFFFFu

FTQ_HD int ftq_shift(int hf, int rr) { return 7 - (2 * hf + rr); }
FTQ_HD uint32_t ftq_code0(int ty, int tx) { return (uint32_t)(((ty + 1) << 11) | ((4 * tx + 1) << 3)); }
FTQ_HD uint32_t ftq_ring(int ly, int lx)
{
    const int y = ly + 2, f = y >= 32 ? 1 : 0; /* 1 <= y <= 66: q <= 17 */
    return (uint32_t)((((y - 32 * f) >> 1) << 11) | ((lx + 1) << 3) | (f << 1) | (y & 1)) | FTQ_RING;
}

FTQ_HD bool ftq_is_ring(uint32_t e) { return (e & FTQ_RING) != 0; }
FTQ_HD int ftq_lx(uint32_t e) { return (int)((e >> 3) & 0x7Fu) - 1; }
FTQ_HD int ftq_ly(uint32_t e) { return (int)(((e >> 10) | (e & 1u)) + ((e & 2u) << 4)) - 2; } /* bit 10 is clear: e >> 10 is 2 q */

/* every position a block can queue, encoded the way the kernel does it and decoded again */
constexpr bool ftq_region_ok(int ly, int lx)
{
    const int hf = ly >> 5, ty = (ly & 31) >> 1, rr = ly & 1, tx = lx >> 2, i = lx & 3;
    const uint32_t word = (0x80u << (8 * i)) >> ftq_shift(hf, rr); /* the pixel's verdict in the thread's word */
    int k = 0;
    while (!((word >> k) & 1u)) k++;
    const uint32_t e = ftq_code0(ty, tx) + (uint32_t)k;
    return word == (1u << k) && e < FTQ_VOID && !(e & 0x400u) && !ftq_is_ring(e) && ftq_ly(e) == ly && ftq_lx(e) == lx;
}
constexpr bool ftq_ring_ok(int ly, int lx)
{
    const uint32_t e = ftq_ring(ly, lx);
    return e < FTQ_VOID && !(e & 0x400u) && ftq_is_ring(e) && ftq_ly(e) == ly && ftq_lx(e) == lx;
}
constexpr bool ftq_round_trip()
{
    for (int ly = 0; ly < 64; ly++)
        for (int lx = 0; lx < 64; lx++)
            if (!ftq_region_ok(ly, lx)) return false;
    for (int hrows = 32; hrows <= 64; hrows += 32) {
        for (int lx = -1; lx <= 64; lx++) /* the rows above and below, corner pixels included */
            if (!ftq_ring_ok(-1, lx) || !ftq_ring_ok(hrows, lx)) return false;
        for (int ly = 0; ly < hrows; ly++)
            if (!ftq_ring_ok(ly, -1) || !ftq_ring_ok(ly, 64)) return false;
    }
    return true;
}
static_assert(ftq_round_trip(), "queue entries: every region and ring position decodes to itself and none is FTQ_VOID");
/* the four shifts are different, so no two verdicts of a thread share a bit, and none of them is FTQ_RING's */
static_assert(ftq_shift(0, 0) == 7 && ftq_shift(0, 1) == 6 && ftq_shift(1, 0) == 5 && ftq_shift(1, 1) == 4, "bit k = 8 i + 2 hf + rr");

#endif
