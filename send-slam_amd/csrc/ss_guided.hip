/*
 * ss_guided.hip -- guided matching: the descriptor search of ORB-SLAM3's SearchForInitialization / SearchByProjection, which
 * looks inside a pixel window (Frame::GetFeaturesInArea) instead of at every train row, then resolves conflicts and applies
 * the 30-bin rotation histogram (the rule: include/sendslam_orb.h; DESIGN.md "Guided matching").
 *
 *   G-A  k_guided_index   one workgroup per train frame: keypoints binned into square cells (LDS histogram, scan, scatter) ->
 *                         cell_start[] and a cell-sorted array of 16-byte records (x, y, octave, row).  No per-cell capacity;
 *                         the order inside a cell is free, every later choice is a minimum over a key
 *   G-B  k_guided_search  four lanes per query walk the cell rows its window meets; the box and octave tests run on the
 *                         records, descriptors are loaded for candidates only; best key d << 20 | row, second-best distance
 *                         and the candidate count fold over the four lanes with the match kernels' chunk rule
 *   G-C  k_guided_finish  one workgroup per frame: conflicts by an LDS atomicMin of d1 << 20 | i per train row, the 30-bin
 *                         histogram and its three maxima, the final idx and the summary
 *
 * The grid never decides membership: a window's cell rectangle is formed from the correctly rounded x -+ radius, binning is a
 * monotone clamp, and a row that passes the float box test lies between those two bounds.  Every float step is a single
 * IEEE operation (-ffp-contract=off).  Every global write is a plain vector store.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ss_constants.h"
#include "ss_kernels.h"
#include "ss_layout.h"
#include "ss_quad.h"

namespace {

/* G-A.  grid (train frames), 256 threads */
__global__ __launch_bounds__(256) void k_guided_index(ssk_guided_call a)
{
    __shared__ uint32_t cnt[GD_CELLS];
    __shared__ uint32_t part[256];
    const int f = (int)blockIdx.x, tid = (int)threadIdx.x, rows = a.rows;
    const int n = (a.frame_error && a.frame_error[f]) ? 0 : gd_clamp_count(a.nt[f], rows);
    const int n_cells = a.cols * a.grid_rows;
    const ss_keypoint *kp = a.t_kp + (size_t)f * rows;
    uint32_t *cs = a.cell_start + (size_t)f * (GD_CELLS + 1);
    gd_rec *recs = (gd_rec *)a.recs + (size_t)f * rows;
    for (int c = tid; c < n_cells; c += 256) cnt[c] = 0;
    __syncthreads();
    for (int j = tid; j < n; j += 256) {
        const ss_keypoint k = kp[j];
        atomicAdd(&cnt[gd_bin(k.y, a.y_max, a.shift) * a.cols + gd_bin(k.x, a.x_max, a.shift)], 1u);
    }
    __syncthreads();
    /* exclusive scan: thread t owns the cells [t * per, (t + 1) * per) */
    const int per = (n_cells + 255) / 256, c0 = tid * per, c1 = min(c0 + per, n_cells);
    uint32_t own = 0;
    for (int c = c0; c < c1; c++) own += cnt[c];
    part[tid] = own;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        const uint32_t v = tid >= off ? part[tid - off] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    uint32_t base = part[tid] - own;
    for (int c = c0; c < c1; c++) {
        const uint32_t v = cnt[c];
        cnt[c] = base; /* from here on: the next free record of the cell */
        cs[c] = base;
        base += v;
    }
    if (tid == 0) cs[n_cells] = (uint32_t)n;
    __syncthreads();
    for (int j = tid; j < n; j += 256) {
        const ss_keypoint k = kp[j];
        const uint32_t pos = atomicAdd(&cnt[gd_bin(k.y, a.y_max, a.shift) * a.cols + gd_bin(k.x, a.x_max, a.shift)], 1u);
        gd_rec r;
        r.x = k.x;
        r.y = k.y;
        r.oct = k.octave;
        r.row = j;
        recs[pos] = r; /* pos < n: the counts sum to n */
    }
}

/* G-B.  grid (ceil(rows / 64), frames), 256 threads: four lanes (a quad) per query row, lane `sub` takes every fourth record of
 * each cell row of the window (gd_walk_window's walk); every row < rows is written.  Per lane: the lowest key d << 20 | row (= lowest
 * distance, then lowest row, whatever the order of the walk), the second-best distance, the candidate count (gd_fold_second) */
__global__ __launch_bounds__(256) void k_guided_search(ssk_guided_call a)
{
    const int b = (int)blockIdx.y, rows = a.rows;
    const int i = (int)(blockIdx.x * 64 + (threadIdx.x >> 2)), sub = (int)(threadIdx.x & 3);
    const gd_frame f = gd_frame_of(a.src, a.frame_error, a.nq, a.nt, rows, b);
    const bool live = i < f.nq;
    float x = 0.f, y = 0.f, r = 0.f;
    int olo = 0, ohi = -1;
    if (live) {
        if (a.windows) {
            const ss_guided_window w = a.windows[(size_t)b * rows + i];
            x = w.x, y = w.y, r = w.radius;
            olo = w.oct_lo, ohi = w.oct_hi;
        } else {
            const ss_keypoint k = a.q_kp[(size_t)b * rows + i];
            x = k.x, y = k.y;
            r = a.radius_by_octave ? a.radius * a.dg->lv[min(max(k.octave, 0), SS_MAX_LEVELS_ - 1)].scale : a.radius;
            olo = k.octave - a.octave_span, ohi = k.octave + a.octave_span;
        }
    }
    const bool search = live && f.nt > 0 && r > 0.0f && olo <= ohi; /* a NaN radius compares false */
    uint32_t best = GD_NONE, second = 0xFFFFu, count = 0;
    if (search) {
        const gd_desc q = gd_load_desc(a.q_desc + ((size_t)b * rows + i) * SS_DESC_BYTES);
        const uint32_t *cs = a.cell_start + (size_t)f.t * (GD_CELLS + 1);
        const gd_rec *recs = (const gd_rec *)a.recs + (size_t)f.t * rows;
        const uint8_t *td = a.t_desc + (size_t)f.t * rows * SS_DESC_BYTES;
        const int skip = (a.exclude_same_frame && f.t == b) ? i : -1;
        /* gd_walk_window (ss_quad.h) written out: through its functor this kernel's record load compiles to other vector loads */
        const int cx0 = gd_bin(x - r, a.x_max, a.shift), cx1 = gd_bin(x + r, a.x_max, a.shift);
        const int cy0 = gd_bin(y - r, a.y_max, a.shift), cy1 = gd_bin(y + r, a.y_max, a.shift);
        for (int cy = cy0; cy <= cy1; cy++) {
            /* the cells cx0 .. cx1 of a grid row are one run of records; a NaN bound can make it empty or reversed */
            const uint32_t k0 = cs[cy * a.cols + cx0], k1 = cx1 >= cx0 ? cs[cy * a.cols + cx1 + 1] : k0;
            for (uint32_t k = k0 + (uint32_t)sub; k < k1; k += 4) {
                const uint4 raw = *(const uint4 *)(recs + k);
                const float ex = __uint_as_float(raw.x), ey = __uint_as_float(raw.y);
                const int eo = (int)raw.z, row = (int)raw.w;
                if (eo < olo || eo > ohi) continue;
                if (!(fabsf(ex - x) < r) || !(fabsf(ey - y) < r)) continue;
                if (row == skip) continue;
                const uint32_t dist = gd_hamming(q, td + (size_t)row * SS_DESC_BYTES);
                const uint32_t key = (dist << 20) | (uint32_t)row;
                count++;
                if (key < best) {
                    second = min(second, gd_dist_of(best));
                    best = key;
                } else {
                    second = min(second, dist);
                }
            }
        }
    }
    gd_fold_second(best, second, count);
    if (i >= rows || sub != 0) return;
    const uint32_t d1 = gd_dist_of(best), d2 = second;
    const int row = best == GD_NONE ? -1 : (int)(best & 0xFFFFFu);
    const bool accept = row >= 0 && (int)d1 <= a.th && (a.rden == 0 || (int)d1 * a.rden < (int)d2 * a.rnum);
    const size_t o = (size_t)b * rows + i;
    a.idx[o] = accept ? row : -1;
    a.d1[o] = (uint16_t)d1;
    a.d2[o] = (uint16_t)d2;
    a.n_cand[o] = (int32_t)count;
}

/* rot -> bin of the 30-bin histogram, -1 when it falls outside (angles outside [0, 360) or NaN) */
__device__ __forceinline__ int gd_rot_bin(float angle_q, float angle_t, float factor)
{
    float rot = angle_q - angle_t;
    if (rot < 0.0f) rot += 360.0f;
    const float rb = roundf(rot * factor);
    if (!(rb >= 0.0f && rb <= (float)SS_HISTO_LENGTH)) return -1;
    const int bin = (int)rb;
    return bin == SS_HISTO_LENGTH ? 0 : bin;
}

/* G-C.  grid (frames), GD_FIN threads; thread t owns the query rows t, t + GD_FIN, ... in every pass, so a row's idx is read and
 * rewritten by one thread only.  The passes are chains of dependent loads on a nearly empty chip (one workgroup per frame): the
 * wider the workgroup, the fewer links per chain */
__global__ __launch_bounds__(GD_FIN) void k_guided_finish(ssk_guided_call a)
{
    __shared__ uint32_t keys[GD_KEY_ROWS];
    __shared__ int hist[SS_HISTO_LENGTH];
    __shared__ int cnt[4]; /* candidates, accepted, unique, final */
    __shared__ int kept[3];
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x, rows = a.rows;
    const gd_frame f = gd_frame_of(a.src, a.frame_error, a.nq, a.nt, rows, b);
    int32_t *idx = a.idx + (size_t)b * rows;
    const uint16_t *d1 = a.d1 + (size_t)b * rows;
    if (tid < 4) cnt[tid] = 0;
    if (tid < 3) kept[tid] = -1;
    if (tid < SS_HISTO_LENGTH) hist[tid] = 0;
    __syncthreads();
    int cand = 0, acc = 0;
    for (int i = tid; i < f.nq; i += GD_FIN) {
        cand += a.n_cand[(size_t)b * rows + i];
        acc += idx[i] >= 0;
    }
    if (cand) atomicAdd(&cnt[0], cand);
    if (acc) atomicAdd(&cnt[1], acc);
    if (a.one_to_one) { /* gd_settle (ss_quad.h) written out: with the call, the three-maxima block below compiles to more LDS reads */
        for (int base = 0; base < f.nt; base += GD_KEY_ROWS) { /* uniform */
            const int len = min(GD_KEY_ROWS, f.nt - base);
            for (int k = tid; k < len; k += GD_FIN) keys[k] = GD_NONE;
            __syncthreads();
            for (int i = tid; i < f.nq; i += GD_FIN) {
                const int j = idx[i] - base;
                if (j >= 0 && j < len && idx[i] >= 0) atomicMin(&keys[j], ((uint32_t)d1[i] << 20) | (uint32_t)i);
            }
            __syncthreads();
            for (int i = tid; i < f.nq; i += GD_FIN) {
                const int j = idx[i] - base;
                if (j >= 0 && j < len && idx[i] >= 0 && keys[j] != (((uint32_t)d1[i] << 20) | (uint32_t)i)) idx[i] = -1;
            }
            __syncthreads();
        }
    }
    int uniq = 0;
    for (int i = tid; i < f.nq; i += GD_FIN) uniq += idx[i] >= 0;
    if (uniq) atomicAdd(&cnt[2], uniq);
    int fin = uniq;
    if (a.orientation) {
        const float factor = a.orientation == 1 ? SS_ROT_FACTOR_1 : SS_ROT_FACTOR_2;
        const ss_keypoint *qk = a.q_kp + (size_t)b * rows, *tk = a.t_kp + (size_t)max(f.t, 0) * rows;
        for (int i = tid; i < f.nq; i += GD_FIN) {
            const int j = idx[i];
            if (j < 0) continue;
            const int bin = gd_rot_bin(qk[i].angle, tk[j].angle, factor);
            if (bin >= 0) atomicAdd(&hist[bin], 1);
        }
        __syncthreads();
        if (tid == 0) { /* ComputeThreeMaxima */
            int max1 = 0, max2 = 0, max3 = 0, ind1 = -1, ind2 = -1, ind3 = -1;
            for (int k = 0; k < SS_HISTO_LENGTH; k++) {
                const int s = hist[k];
                if (s > max1) {
                    max3 = max2, max2 = max1, max1 = s;
                    ind3 = ind2, ind2 = ind1, ind1 = k;
                } else if (s > max2) {
                    max3 = max2, max2 = s;
                    ind3 = ind2, ind2 = k;
                } else if (s > max3) {
                    max3 = s;
                    ind3 = k;
                }
            }
            const float cut = 0.1f * (float)max1;
            if ((float)max2 < cut) ind2 = ind3 = -1;
            else if ((float)max3 < cut) ind3 = -1;
            kept[0] = ind1, kept[1] = ind2, kept[2] = ind3;
        }
        __syncthreads();
        const int k0 = kept[0], k1 = kept[1], k2 = kept[2];
        fin = 0;
        for (int i = tid; i < f.nq; i += GD_FIN) {
            const int j = idx[i];
            if (j < 0) continue;
            const int bin = gd_rot_bin(qk[i].angle, tk[j].angle, factor);
            if (bin >= 0 && (bin == k0 || bin == k1 || bin == k2)) fin++;
            else idx[i] = -1;
        }
    }
    if (fin) atomicAdd(&cnt[3], fin);
    __syncthreads();
    if (tid == 0) {
        ss_guided_summary s;
        s.status = f.status;
        s.n_query = f.nq;
        s.n_train = f.nt;
        s.n_candidates = cnt[0];
        s.n_accepted = cnt[1];
        s.n_unique = cnt[2];
        s.n_final = cnt[3];
        s.rot_bins = a.orientation ? ((kept[0] & 0xFF) | ((kept[1] & 0xFF) << 8) | ((kept[2] & 0xFF) << 16)) : 0xFFFFFF;
        a.summary[b] = s;
    }
}

} // namespace

/* cells of 32 px, doubled until the grid fits SSK_GUIDED_MAX_CELLS; extents beyond 2^24 px share the last cells (float holds
 * every integer below that, so the clamp bound is exact) */
void ssk_guided_grid(ssk_guided_call &g, int extent_w, int extent_h)
{
    const int w = extent_w < (1 << 24) ? extent_w : (1 << 24), h = extent_h < (1 << 24) ? extent_h : (1 << 24);
    int s = 5;
    while ((int64_t)(((w - 1) >> s) + 1) * (((h - 1) >> s) + 1) > SSK_GUIDED_MAX_CELLS) s++;
    g.shift = s;
    g.cols = ((w - 1) >> s) + 1;
    g.grid_rows = ((h - 1) >> s) + 1;
    g.x_max = (float)(w - 1);
    g.y_max = (float)(h - 1);
}

void ssk_guided_index(hipStream_t s, const ssk_guided_call &g)
{
    hipLaunchKernelGGL(k_guided_index, dim3((unsigned)g.n_frames), dim3(256), 0, s, g);
}

void ssk_guided_search(hipStream_t s, const ssk_guided_call &g)
{
    hipLaunchKernelGGL(k_guided_search, dim3((unsigned)((g.rows + 63) / 64), (unsigned)g.n_frames), dim3(256), 0, s, g);
}

void ssk_guided_finish(hipStream_t s, const ssk_guided_call &g)
{
    hipLaunchKernelGGL(k_guided_finish, dim3((unsigned)g.n_frames), dim3(GD_FIN), 0, s, g);
}
