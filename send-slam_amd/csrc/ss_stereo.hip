/*
 * ss_stereo.hip -- stereo depth for rectified pairs of one batch (frames 2p = left, 2p + 1 = right): a restatement of
 * ORB-SLAM3's Frame::ComputeStereoMatches on the keypoints, descriptors and unblurred pyramids the extraction left
 * in HBM (DESIGN.md "Stereo depth").
 *
 *   S-A  k_stereo_search   Hamming search over the right keypoints whose row band holds the left keypoint's row,
 *                          octave +-1, u inside the disparity range; four lanes per left keypoint walk a compact
 *                          LDS copy of the right keypoints (ties: lowest index, as the minimum of distance | index)
 *   S-B  k_stereo_refine   11 x 11 byte SAD slid -5 .. +5 px at the left keypoint's octave, parabola fit, disparity
 *                          and depth; a wave per matched keypoint, windows staged as aligned dwords
 *   S-C  k_stereo_cut      median of the accepted SADs per pair (two-pass radix select), the 1.5 * 1.4 * median cut,
 *                          the pair's summary; one block per pair
 *
 * Integer work except the float steps of S-B / S-C, each a single IEEE operation (-ffp-contract=off).  Every global
 * write is a plain vector store.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ss_constants.h"
#include "ss_kernels.h"
#include "ss_layout.h"

namespace {

#define ST_TH_REJECT ((SS_TH_HIGH + SS_TH_LOW) / 2) /* 75 */
#define ST_W 5                                      /* SAD window half size */
#define ST_L 5                                      /* slide range */
#define ST_CHUNK 1024                               /* right keypoints per LDS pass of S-A */
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ void st_wave_sync()
{
    /* lanes of one wave hand data to each other through LDS: program order holds, only the compiler must not move accesses */
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

/* status of pair p: 0, or the error of the eye that voids it (left first) */
__device__ __forceinline__ int pair_status(const int32_t *__restrict__ frame_error, int p)
{
    const int el = frame_error[2 * p], er = frame_error[2 * p + 1];
    return el ? el : er;
}

/* S-A.  grid (ceil(kcap / 64), pairs), 256 threads: four lanes (a quad) per left keypoint row, lane `sub` of the quad takes
 * every fourth group of eight right keypoints; every row < kcap is written.  "d < best in ascending index order" keeps the
 * lowest index among the lowest distances = the minimum of the key d << 20 | index, so the order of the walk is free and
 * the quad's four minima fold into one (indices < kcap < 2^20, d <= 256; the start value is upstream's best = 100, bestR = 0) */
__global__ __launch_bounds__(256) void k_stereo_search(const ss_geom *__restrict__ g, const ss_keypoint *__restrict__ kps,
                                                       const uint8_t *__restrict__ desc, const int32_t *__restrict__ n_kp,
                                                       const int32_t *__restrict__ frame_error, float max_d, float min_d,
                                                       ss_stereo_point *__restrict__ points)
{
    /* per right keypoint of the chunk: first row of its band, rows after the first, octave (16 bits each: image rows fit 12), u */
    __shared__ __attribute__((aligned(16))) uint16_t r_lo[ST_CHUNK];
    __shared__ __attribute__((aligned(16))) uint16_t r_span[ST_CHUNK];
    __shared__ __attribute__((aligned(16))) uint16_t r_oct[ST_CHUNK];
    __shared__ __attribute__((aligned(16))) float r_u[ST_CHUNK];
    const int p = (int)blockIdx.y, kcap = g->kcap;
    const int iL = (int)(blockIdx.x * 64 + (threadIdx.x >> 2)), sub = (int)(threadIdx.x & 3);
    const bool ok_pair = pair_status(frame_error, p) == 0;
    const int nL = ok_pair ? min(n_kp[2 * p], kcap) : 0, nR = ok_pair ? min(n_kp[2 * p + 1], kcap) : 0;
    const ss_keypoint *kL = kps + (size_t)(2 * p) * kcap, *kR = kps + (size_t)(2 * p + 1) * kcap;
    const bool live = iL < nL;
    float uL = 0.f, min_u = 0.f, max_u = -1.f;
    int vi = 0, octL = 0;
    uint64_t dl[4] = {0, 0, 0, 0};
    if (live) {
        const ss_keypoint k = kL[iL];
        uL = k.x;
        vi = (int)k.y;
        octL = k.octave;
        min_u = uL - max_d;
        max_u = uL - min_d;
        const uint4 *d = (const uint4 *)(desc + ((size_t)(2 * p) * kcap + iL) * SS_DESC_BYTES);
        const uint4 a = d[0], b = d[1];
        dl[0] = (uint64_t)a.x | ((uint64_t)a.y << 32);
        dl[1] = (uint64_t)a.z | ((uint64_t)a.w << 32);
        dl[2] = (uint64_t)b.x | ((uint64_t)b.y << 32);
        dl[3] = (uint64_t)b.z | ((uint64_t)b.w << 32);
    }
    const bool search = live && !(max_u < 0.f);
    uint32_t best_key = (uint32_t)SS_TH_HIGH << 20;
    for (int base = 0; base < nR; base += ST_CHUNK) {
        const int cnt = min(ST_CHUNK, nR - base);
        __syncthreads();
        for (int j = (int)threadIdx.x; j < ST_CHUNK; j += 256) {
            int lo = 0xFFFF, span = 0; /* the padding of the last group of eight: no row is inside */
            if (j < cnt) {
                const ss_keypoint k = kR[base + j];
                const float r = 2.0f * g->lv[k.octave].scale;
                lo = max((int)floorf(k.y - r), 0);
                span = min((int)ceilf(k.y + r), 0xFFF) - lo;
                r_u[j] = k.x;
                r_oct[j] = (uint16_t)k.octave;
            }
            r_lo[j] = (uint16_t)lo;
            r_span[j] = (uint16_t)span;
        }
        __syncthreads();
        if (search) {
            /* kcap^2 row tests per pair, ~1 % pass: they are taken eight at a time in packed 16-bit arithmetic.
             * t = (vL - lo) mod 2^16 is <= span exactly for the rows of the band, the saturating t - span is then 0; the
             * octave test |octR - octL| <= 1 is (octR - (octL - 1)) mod 2^16 <= 2 in the same form.  One packed minimum over
             * the eight says whether any passes both.  Everything a group needs (bands, octaves, u) is loaded up front, in
             * one LDS round trip: about four of a wave's 512 candidates pass per step, and a dependent LDS read per passing
             * candidate cost 0.101 against 0.084 ms per 64 pairs of 2000 keypoints */
            const u16x2 vv = {(unsigned short)vi, (unsigned short)vi};
            const u16x2 ov = {(unsigned short)(octL - 1), (unsigned short)(octL - 1)}, two = {2, 2};
            for (int q = sub; 8 * q < cnt; q += 4) {
                const uint4 lo4 = ((const uint4 *)r_lo)[q], sp4 = ((const uint4 *)r_span)[q], oc4 = ((const uint4 *)r_oct)[q];
                const float4 ua = ((const float4 *)r_u)[2 * q], ub = ((const float4 *)r_u)[2 * q + 1];
                const uint32_t lo_w[4] = {lo4.x, lo4.y, lo4.z, lo4.w}, sp_w[4] = {sp4.x, sp4.y, sp4.z, sp4.w}, oc_w[4] = {oc4.x, oc4.y, oc4.z, oc4.w};
                const float u8[8] = {ua.x, ua.y, ua.z, ua.w, ub.x, ub.y, ub.z, ub.w};
                u16x2 over[4];
#pragma unroll
                for (int k = 0; k < 4; k++)
                    over[k] = __builtin_elementwise_sub_sat(vv - __builtin_bit_cast(u16x2, lo_w[k]), __builtin_bit_cast(u16x2, sp_w[k])) |
                              __builtin_elementwise_sub_sat(__builtin_bit_cast(u16x2, oc_w[k]) - ov, two);
                const u16x2 m = __builtin_elementwise_min(__builtin_elementwise_min(over[0], over[1]), __builtin_elementwise_min(over[2], over[3]));
                if (m.x != 0 && m.y != 0) continue;
#pragma unroll
                for (int e = 0; e < 8; e++) {
                    if ((e & 1 ? over[e >> 1].y : over[e >> 1].x) != 0) continue;
                    if (!(u8[e] >= min_u && u8[e] <= max_u)) continue;
                    const int j = 8 * q + e;
                    const uint4 *d = (const uint4 *)(desc + ((size_t)(2 * p + 1) * kcap + base + j) * SS_DESC_BYTES);
                    const uint4 a = d[0], b = d[1];
                    const int dist = __popcll(dl[0] ^ ((uint64_t)a.x | ((uint64_t)a.y << 32))) + __popcll(dl[1] ^ ((uint64_t)a.z | ((uint64_t)a.w << 32))) +
                                     __popcll(dl[2] ^ ((uint64_t)b.x | ((uint64_t)b.y << 32))) + __popcll(dl[3] ^ ((uint64_t)b.z | ((uint64_t)b.w << 32)));
                    best_key = min(best_key, ((uint32_t)dist << 20) | (uint32_t)(base + j));
                }
            }
        }
    }
    /* fold the quad (all 64 lanes take part; a quad's lanes share iL, so `search` is uniform inside it) */
    best_key = min(best_key, (uint32_t)__shfl_xor((int)best_key, 1));
    best_key = min(best_key, (uint32_t)__shfl_xor((int)best_key, 2));
    if (iL >= kcap || sub != 0) return;
    const int best = (int)(best_key >> 20), best_r = (int)(best_key & 0xFFFFFu);
    ss_stereo_point v;
    v.u_right = -1.0f;
    v.depth = -1.0f;
    v.right_idx = -1;
    v.orb_dist = 0xFFFF;
    v.sad = 0xFFFF;
    if (search && best < ST_TH_REJECT) {
        v.right_idx = best_r;
        v.orb_dist = (uint16_t)best;
    }
    points[(size_t)p * kcap + iL] = v;
}

/* S-B.  grid (ceil(kcap / 4), pairs), 256 threads: one wave per left keypoint, waves independent (no block barrier) */
__global__ __launch_bounds__(256) void k_stereo_refine(const ss_geom *__restrict__ g, const ss_keypoint *__restrict__ kps,
                                                       const int32_t *__restrict__ n_kp, const int32_t *__restrict__ frame_error,
                                                       const uint8_t *__restrict__ pyr, const uint8_t *__restrict__ lvl0, int lvl0_pitch,
                                                       int64_t lvl0_fs, float bf, float max_d, float min_d, ss_stereo_point *__restrict__ points)
{
    /* per wave: 11 rows x (4 left + 8 right) staged dwords, then 121 partial sums, then the 11 sums */
    __shared__ uint32_t win_all[4][11 * 12];
    __shared__ uint32_t part_all[4][11 * 11 + 11];
    const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
    const int p = (int)blockIdx.y, kcap = g->kcap;
    const int iL = (int)blockIdx.x * 4 + wave;
    if (pair_status(frame_error, p) != 0) return;
    if (iL >= min(n_kp[2 * p], kcap)) return;
    ss_stereo_point *pt = points + (size_t)p * kcap + iL;
    const ss_stereo_point cur = *pt;
    const int best_r = cur.right_idx;
    if (best_r < 0) return;
    const ss_keypoint kl = kps[(size_t)(2 * p) * kcap + iL];
    const float uL = kl.x, vL = kl.y, uR0 = kps[(size_t)(2 * p + 1) * kcap + best_r].x;
    const int l = kl.octave;
    const ss_level &L = g->lv[l];
    const float sc = L.scale, inv = 1.0f / sc;
    const int su = (int)roundf(uL * inv), sv = (int)roundf(vL * inv), sr = (int)roundf(uR0 * inv);
    const int cols = L.w, rows = L.h;
    /* upstream's test, as written; then the guard: every window column / row must lie inside the level image */
    if (sr + ST_L - ST_W < 0 || sr + ST_L + ST_W + 1 >= cols || sr - ST_L - ST_W < 0 || sr + ST_L + ST_W > cols - 1 || su - ST_W < 0 ||
        su + ST_W > cols - 1 || sv - ST_W < 0 || sv + ST_W > rows - 1)
        return;

    const bool inplace = l == 0 && lvl0 != nullptr; /* level 0 lives in the caller's buffer */
    const int pitch = inplace ? lvl0_pitch : L.pitch;
    const uint8_t *imL = inplace ? lvl0 + (int64_t)(2 * p) * lvl0_fs : pyr + (size_t)(2 * p) * g->block_bytes + L.off;
    const uint8_t *imR = inplace ? lvl0 + (int64_t)(2 * p + 1) * lvl0_fs : pyr + (size_t)(2 * p + 1) * g->block_bytes + L.off;
    const int xl0 = su - ST_W, xr0 = sr - ST_L - ST_W;
    const int sL = xl0 & 3, sR = xr0 & 3;
    const int last_l = (sL + 2 * ST_W) >> 2, last_r = (sR + 2 * ST_W + 2 * ST_L) >> 2; /* last dword holding a window byte: <= 3, <= 5 */
    uint32_t *win = win_all[wave], *part = part_all[wave];
    /* rows are dword aligned (pitch is a multiple of 4) and a loaded dword holds at least one window byte, which the
     * guard placed inside the row: it lies inside the row's pitch */
#pragma unroll
    for (int it = 0; it < 3; it++) {
        const int slot = lane + 64 * it;
        if (slot < 11 * 12) {
            const int r = slot / 12, c = slot - r * 12;
            uint32_t v = 0;
            if (c < 4) {
                if (c <= last_l) v = *(const uint32_t *)(imL + (size_t)(sv - ST_W + r) * pitch + (xl0 & ~3) + 4 * c);
            } else if (c - 4 <= last_r) {
                v = *(const uint32_t *)(imR + (size_t)(sv - ST_W + r) * pitch + (xr0 & ~3) + 4 * (c - 4));
            }
            win[slot] = v;
        }
    }
    st_wave_sync();
#pragma unroll
    for (int it = 0; it < 2; it++) {
        const int t = lane + 64 * it;
        if (t < 121) {
            const int r = t / 11, inc = t - r * 11;
            const uint32_t *w = win + r * 12;
            const uint32_t l0 = __builtin_amdgcn_alignbyte(w[1], w[0], sL), l1 = __builtin_amdgcn_alignbyte(w[2], w[1], sL),
                           l2 = __builtin_amdgcn_alignbyte(w[3], w[2], sL) & 0x00FFFFFFu;
            const int o = sR + inc, i = 4 + (o >> 2), s = o & 3;
            const uint32_t r0 = __builtin_amdgcn_alignbyte(w[i + 1], w[i], s), r1 = __builtin_amdgcn_alignbyte(w[i + 2], w[i + 1], s),
                           r2 = __builtin_amdgcn_alignbyte(w[i + 3], w[i + 2], s) & 0x00FFFFFFu;
            uint32_t sad = __builtin_amdgcn_sad_u8(l0, r0, 0u);
            sad = __builtin_amdgcn_sad_u8(l1, r1, sad);
            sad = __builtin_amdgcn_sad_u8(l2, r2, sad);
            part[t] = sad;
        }
    }
    st_wave_sync();
    if (lane < 11) {
        uint32_t s = 0;
#pragma unroll
        for (int r = 0; r < 11; r++) s += part[r * 11 + lane];
        part[121 + lane] = s;
    }
    st_wave_sync();
    /* the serial tail, uniform over the wave (LDS broadcast reads); lane 0 writes */
    int best_sad = 0x7FFFFFFF, best_inc = 0;
    for (int k = 0; k < 2 * ST_L + 1; k++) {
        const int d = (int)part[121 + k];
        if (d < best_sad) {
            best_sad = d;
            best_inc = k - ST_L;
        }
    }
    float u_right = -1.0f, depth = -1.0f;
    if (best_inc != -ST_L && best_inc != ST_L) {
        const float d1 = (float)part[121 + ST_L + best_inc - 1], d2 = (float)part[121 + ST_L + best_inc], d3 = (float)part[121 + ST_L + best_inc + 1];
        const float num = d1 - d3;
        const float t0 = d1 + d3, t1 = 2.0f * d2, t2 = t0 - t1, den = 2.0f * t2;
        const float delta = num / den; /* 0/0 -> NaN, x/0 -> inf: followed, not special-cased */
        if (!(delta < -1.0f || delta > 1.0f)) {
            const float a0 = (float)sr + (float)best_inc, a1 = a0 + delta;
            float best_u = sc * a1;
            float disp = uL - best_u;
            if (disp >= min_d && disp < max_d) { /* NaN rejects here */
                if (disp <= 0.0f) {
                    disp = 0.01f;
                    best_u = uL - 0.01f;
                }
                depth = bf / disp;
                u_right = best_u;
            }
        }
    }
    if (lane == 0) {
        ss_stereo_point v;
        v.u_right = u_right;
        v.depth = depth;
        v.right_idx = best_r;
        v.orb_dist = cur.orb_dist;
        v.sad = (uint16_t)best_sad; /* <= 121 * 255 */
        *pt = v;
    }
}

/* S-C.  grid (pairs), 256 threads.  Accepted = depth > 0 (bf > 0 and 0 < disparity < maxD).  The median is element
 * [n / 2] of the ascending SADs: a 256-bin histogram of sad >> 7, then a 128-bin one of sad & 127 inside the bin that
 * holds the rank (sad <= 30855 = 241 * 128 + 7) */
__global__ __launch_bounds__(256) void k_stereo_cut(const ss_geom *__restrict__ g, const int32_t *__restrict__ n_kp,
                                                    const int32_t *__restrict__ frame_error, float close_depth,
                                                    ss_stereo_point *__restrict__ points, ss_stereo_summary *__restrict__ summary)
{
    __shared__ int hist[256];
    __shared__ int cnt[4]; /* matched, refined, depth, close */
    __shared__ int sel_bin, sel_rank, median_s;
    const int p = (int)blockIdx.x, kcap = g->kcap, tid = (int)threadIdx.x;
    const int status = pair_status(frame_error, p);
    const int nL = status == 0 ? min(n_kp[2 * p], kcap) : 0, nR = status == 0 ? min(n_kp[2 * p + 1], kcap) : 0;
    ss_stereo_point *pts = points + (size_t)p * kcap;
    hist[tid] = 0;
    if (tid < 4) cnt[tid] = 0;
    if (tid == 0) median_s = -1;
    __syncthreads();
    int matched = 0, refined = 0;
    for (int i = tid; i < nL; i += 256) {
        const ss_stereo_point v = pts[i];
        matched += v.right_idx >= 0;
        if (v.depth > 0.0f) {
            refined++;
            atomicAdd(&hist[v.sad >> 7], 1);
        }
    }
    if (matched) atomicAdd(&cnt[0], matched);
    if (refined) atomicAdd(&cnt[1], refined);
    __syncthreads();
    const int n_ref = cnt[1];
    if (n_ref > 0) { /* uniform */
        if (tid == 0) {
            int rank = n_ref / 2, b = 0;
            while (rank >= hist[b]) rank -= hist[b++];
            sel_bin = b;
            sel_rank = rank;
        }
        __syncthreads();
        const int bin = sel_bin;
        hist[tid] = 0;
        __syncthreads();
        for (int i = tid; i < nL; i += 256) {
            const ss_stereo_point v = pts[i];
            if (v.depth > 0.0f && (v.sad >> 7) == bin) atomicAdd(&hist[v.sad & 127], 1);
        }
        __syncthreads();
        if (tid == 0) {
            int rank = sel_rank, b = 0;
            while (rank >= hist[b]) rank -= hist[b++];
            median_s = bin * 128 + b;
        }
        __syncthreads();
        const float th_dist = (1.5f * 1.4f) * (float)median_s;
        int with_depth = 0, close = 0;
        for (int i = tid; i < nL; i += 256) {
            ss_stereo_point v = pts[i];
            if (!(v.depth > 0.0f)) continue;
            if ((float)v.sad >= th_dist) {
                v.u_right = -1.0f;
                v.depth = -1.0f;
                pts[i] = v;
            } else {
                with_depth++;
                close += v.depth < close_depth;
            }
        }
        if (with_depth) atomicAdd(&cnt[2], with_depth);
        if (close) atomicAdd(&cnt[3], close);
        __syncthreads();
    }
    if (tid == 0) {
        ss_stereo_summary s;
        s.status = status;
        s.n_left = nL;
        s.n_right = nR;
        s.n_matched = cnt[0];
        s.n_refined = cnt[1];
        s.n_depth = cnt[2];
        s.n_close = cnt[3];
        s.sad_median = median_s;
        summary[p] = s;
    }
}

} // namespace

void ssk_stereo_search(hipStream_t s, const ssk_extract_ws &ws, const ss_geom &hg, int n_frames, const ssk_stereo_call &st)
{
    hipLaunchKernelGGL(k_stereo_search, dim3((unsigned)((hg.kcap + 63) / 64), (unsigned)(n_frames / 2)), dim3(256), 0, s, ws.dg, ws.kps, ws.desc,
                       ws.n_kp, st.frame_error ? st.frame_error : ws.frame_error, st.max_d, st.min_d, (ss_stereo_point *)st.points);
}

void ssk_stereo_refine(hipStream_t s, const ssk_extract_ws &ws, const ss_geom &hg, int n_frames, const ss_lvl0 &l0, const ssk_stereo_call &st)
{
    hipLaunchKernelGGL(k_stereo_refine, dim3((unsigned)((hg.kcap + 3) / 4), (unsigned)(n_frames / 2)), dim3(256), 0, s, ws.dg, ws.kps, ws.n_kp,
                       st.frame_error ? st.frame_error : ws.frame_error, ws.pyr, l0.ptr, l0.pitch, l0.frame_stride, st.bf, st.max_d, st.min_d,
                       (ss_stereo_point *)st.points);
}

void ssk_stereo_cut(hipStream_t s, const ssk_extract_ws &ws, const ss_geom &hg, int n_frames, const ssk_stereo_call &st)
{
    hipLaunchKernelGGL(k_stereo_cut, dim3((unsigned)(n_frames / 2)), dim3(256), 0, s, ws.dg, ws.n_kp, st.frame_error ? st.frame_error : ws.frame_error,
                       st.close_depth, (ss_stereo_point *)st.points, (ss_stereo_summary *)st.summary);
}
