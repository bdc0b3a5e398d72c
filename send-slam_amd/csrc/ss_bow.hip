/*
 * ss_bow.hip -- bag of words: DBoW2's vocabulary transform (Frame::ComputeBoW), the candidate search of ORBmatcher::SearchByBoW and
 * L1Scoring::score (the rule: include/sendslam_orb.h; DESIGN.md "Bag of words").
 *
 *   B-A  k_bow_descend  eight lanes per descriptor row walk the tree: the row stays in registers, the lanes take the children of
 *                       the current node (32-byte rows, consecutive), the minimum of distance << 8 | child ordinal folds over the
 *                       eight lanes, so the earliest of equally near children wins; no LDS
 *   B-B  k_bow_vector   one workgroup per frame: the keys word << 32 | row of the used rows sorted in LDS, runs turned into
 *                       counts and values (w added to itself), ONE thread walks the norm in ascending word order, everybody
 *                       divides; then the keys node << 32 | row sorted the same way are the frame's node index
 *        k_bow_index    the node index alone, for caller-made nodes
 *   B-C  k_bow_search   four lanes per query: binary search for the run of its node in the train frame's index (gd_walk_node,
 *                       ss_quad.h), then the lane scheme, the fold (gd_fold_second) and the acceptance test of k_guided_search;
 *                       k_guided_finish runs on what it writes
 *   B-D  k_bow_score    one wave per database vector: every lane looks its word up in the query (binary search), the terms of
 *                       the common words are added in ascending order, one double addition at a time
 *
 * Every double step is a single IEEE operation (-ffp-contract=off).  Every global write is a plain vector store.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ss_bow_merge.h"
#include "ss_constants.h"
#include "ss_kernels.h"
#include "ss_quad.h"

namespace {

#define BW_LANES 8      /* lanes per row of k_bow_descend */
#define BW_SORT 16384   /* keys one workgroup sorts: SS_BOW_MAX_ROWS */
#define BW_T 1024       /* threads of k_bow_vector / k_bow_index */
#define BW_PAD 0xFFFFFFFFFFFFFFFFull /* sorts behind every key: a row is < 2^32 - 1 */

static_assert(SS_BOW_MAX_ROWS == BW_SORT, "the LDS sort holds SS_BOW_MAX_ROWS keys");
static_assert(SS_VOCAB_MAX_K <= 256, "a child ordinal has 8 bits of the descent's key");

__device__ __forceinline__ int bw_count(const int32_t *n_rows, const int32_t *frame_error, int f, int rows)
{
    if (frame_error && frame_error[f]) return 0;
    return min(max(n_rows[f], 0), rows);
}

/* B-A.  grid (ceil(rows / 32), frames), 256 threads; every row < rows is written.  The loop is uniform over the wave (a row
 * that has reached its leaf idles), so all 64 lanes take part in every fold; max_depth bounds it whatever the tables hold. */
__global__ __launch_bounds__(256) void k_bow_descend(ssk_bow_voc v, ssk_bow_call c)
{
    const int f = (int)blockIdx.y, rows = c.rows;
    const int i = (int)(blockIdx.x * (256 / BW_LANES) + (threadIdx.x / BW_LANES)), sub = (int)(threadIdx.x % BW_LANES);
    const int n = bw_count(c.n_rows, c.frame_error, f, rows);
    const bool live = i < n;
    uint64_t q0 = 0, q1 = 0, q2 = 0, q3 = 0; /* four words, not a gd_desc: in this form the kernel compiles to the code it had */
    int base = 0, nc = 0;
    if (live) {
        const gd_desc l = gd_load_desc(c.desc + ((size_t)f * rows + i) * SS_DESC_BYTES);
        q0 = l.q0, q1 = l.q1, q2 = l.q2, q3 = l.q3;
        const uint4 root = *(const uint4 *)v.recs;
        base = (int)root.x, nc = (int)root.y;
    }
    const int target = v.L - c.levelsup;
    int depth = 0, word = -1, node = target <= 0 ? 0 : -1;
    bool go = live && nc > 0;
    for (int step = 0; step < v.max_depth; step++) {
        if (!__any(go)) break;
        uint32_t best = GD_NONE;
        if (go)
            for (int ch = sub; ch < nc; ch += BW_LANES)
                best = min(best, (gd_hamming(q0, q1, q2, q3, v.rows + (size_t)(base + ch) * SS_DESC_BYTES) << 8) | (uint32_t)ch);
#pragma unroll
        for (int m = 1; m < BW_LANES; m <<= 1) best = min(best, (uint32_t)__shfl_xor((int)best, m));
        if (go) {
            const uint4 rec = *(const uint4 *)(v.recs + base + (int)(best & 0xFFu)); /* one address per row: a broadcast */
            depth++;
            if (depth == target) node = (int)rec.w;
            base = (int)rec.x, nc = (int)rec.y;
            if (nc == 0) { /* the leaf; shallower than L - levelsup, it is the node itself */
                word = (int)rec.z;
                if (node < 0) node = (int)rec.w;
                go = false;
            }
        }
    }
    if (i >= rows || sub != 0) return;
    const size_t o = (size_t)f * rows + i;
    if (live && word >= 0) {
        const double w = v.weight[word];
        if (!(w > 0.0)) node = -1;
    } else {
        word = node = -1;
    }
    c.word[o] = word;
    c.node[o] = node;
    if (c.node2) c.node2[o] = node;
}

/* bitonic sort of n2 (a power of two <= BW_SORT) keys in LDS, ascending; all BW_T threads call it */
__device__ void bw_sort(uint64_t *a, int n2, int tid)
{
    for (int k = 2; k <= n2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (n2 >> 1); t += BW_T) {
                const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
                const uint64_t x = a[lo], y = a[hi];
                if ((x > y) == ((lo & k) == 0)) a[lo] = y, a[hi] = x;
            }
            __syncthreads();
        }
}

__device__ __forceinline__ int bw_pow2(int n)
{
    int p = 1;
    while (p < n) p <<= 1;
    return p;
}

/* The node index of one frame: the keys node << 32 | row of its rows with node >= 0, ascending -> index[0 .. m), m returned;
 * *distinct = the number of different nodes.  cnt: two shared words.  All BW_T threads call it. */
__device__ int bw_index_frame(uint64_t *a, int *cnt, const int32_t *node, int n, int tid, uint64_t *index, int *distinct)
{
    const int n2 = bw_pow2(n);
    if (tid < 2) cnt[tid] = 0;
    __syncthreads();
    int mine = 0;
    for (int j = tid; j < n2; j += BW_T) {
        const int nd = j < n ? node[j] : -1;
        a[j] = nd >= 0 ? ((uint64_t)(uint32_t)nd << 32) | (uint32_t)j : BW_PAD;
        mine += nd >= 0;
    }
    if (mine) atomicAdd(&cnt[0], mine);
    __syncthreads();
    bw_sort(a, n2, tid);
    const int m = cnt[0];
    int heads = 0;
    for (int p = tid; p < m; p += BW_T) {
        const uint64_t key = a[p];
        heads += p == 0 || (uint32_t)(a[p - 1] >> 32) != (uint32_t)(key >> 32);
        if (index) index[p] = key;
    }
    if (heads) atomicAdd(&cnt[1], heads);
    __syncthreads();
    *distinct = cnt[1];
    return m;
}

/* B-B.  grid (frames), BW_T threads */
__global__ __launch_bounds__(BW_T) void k_bow_vector(ssk_bow_voc v, ssk_bow_call c)
{
    __shared__ uint64_t a[BW_SORT];
    __shared__ uint32_t part[BW_T];
    __shared__ int cnt[2];
    __shared__ double norm_s;
    const int f = (int)blockIdx.x, tid = (int)threadIdx.x, rows = c.rows;
    const int n = bw_count(c.n_rows, c.frame_error, f, rows);
    const int32_t *word = c.word + (size_t)f * rows, *node = c.node + (size_t)f * rows;
    int32_t *bw = c.bow_word + (size_t)f * rows;
    double *bv = c.bow_value + (size_t)f * rows;
    const int n2 = bw_pow2(n);
    if (tid == 0) cnt[0] = 0;
    __syncthreads();
    int mine = 0;
    for (int j = tid; j < n2; j += BW_T) {
        /* w > 0: the descent gave the row a node.  The two arrays are the caller's outputs: a word that is none of the
         * vocabulary's (the caller reused the memory while the call was in flight) must not index the weights */
        const uint32_t wd = j < n ? (uint32_t)word[j] : GD_NONE;
        const bool used = j < n && node[j] >= 0 && wd < (uint32_t)v.n_words;
        a[j] = used ? ((uint64_t)wd << 32) | (uint32_t)j : BW_PAD;
        mine += used;
    }
    if (mine) atomicAdd(&cnt[0], mine);
    __syncthreads();
    bw_sort(a, n2, tid);
    const int m = cnt[0];
    /* thread t owns the sorted positions [t * per, (t + 1) * per): the heads of the runs among them, ranked by an exclusive scan */
    const int per = (n2 + BW_T - 1) / BW_T, p0 = min(tid * per, m), p1 = min(p0 + per, m);
    uint32_t own = 0;
    for (int p = p0; p < p1; p++) own += p == 0 || (uint32_t)(a[p - 1] >> 32) != (uint32_t)(a[p] >> 32);
    part[tid] = own;
    __syncthreads();
    for (int off = 1; off < BW_T; off <<= 1) {
        const uint32_t x = tid >= off ? part[tid - off] : 0;
        __syncthreads();
        part[tid] += x;
        __syncthreads();
    }
    const int n_words = (int)part[BW_T - 1];
    int rank = (int)(part[tid] - own);
    for (int p = p0; p < p1; p++) {
        const uint32_t wd = (uint32_t)(a[p] >> 32);
        if (p != 0 && (uint32_t)(a[p - 1] >> 32) == wd) continue;
        int seen = 1;
        while (p + seen < m && (uint32_t)(a[p + seen] >> 32) == wd) seen++;
        const double w = v.weight[wd];
        double val = w;
        for (int t = 1; t < seen; t++) val += w; /* addWeight, once per further row */
        bw[rank] = (int32_t)wd; /* rank < n_words <= m <= rows */
        bv[rank] = val;
        rank++;
    }
    for (int r = n_words + tid; r < rows; r += BW_T) bw[r] = -1, bv[r] = 0.0;
    __threadfence_block();
    __syncthreads();
    if (tid == 0) { /* normalize(L1): the serial chain is the rule */
        double s = 0.0;
        for (int r = 0; r < n_words; r++) s += fabs(bv[r]);
        norm_s = s;
    }
    __syncthreads();
    const double norm = norm_s;
    if (norm > 0.0)
        for (int r = tid; r < n_words; r += BW_T) bv[r] = bv[r] / norm;
    __syncthreads(); /* the keys are reused */
    int n_nodes = 0;
    const int indexed = bw_index_frame(a, cnt, node, n, tid, c.index ? c.index + (size_t)f * rows : nullptr, &n_nodes);
    if (tid == 0) {
        if (c.n_index) c.n_index[f] = indexed;
        ss_bow_summary s;
        s.status = c.frame_error ? c.frame_error[f] : 0;
        s.n_rows = n;
        s.n_used = m;
        s.n_words = n_words;
        s.n_nodes = n_nodes;
        s.reserved = 0;
        s.norm = norm;
        c.summary[f] = s;
    }
}

__global__ __launch_bounds__(BW_T) void k_bow_index(const int32_t *node, const int32_t *n_rows, const int32_t *frame_error, int rows,
                                                    uint64_t *index, int32_t *n_index)
{
    __shared__ uint64_t a[BW_SORT];
    __shared__ int cnt[2];
    const int f = (int)blockIdx.x, tid = (int)threadIdx.x;
    int distinct = 0;
    const int m = bw_index_frame(a, cnt, node + (size_t)f * rows, bw_count(n_rows, frame_error, f, rows), tid, index + (size_t)f * rows, &distinct);
    if (tid == 0) n_index[f] = m;
}

/* B-C.  grid (ceil(rows / 64), frames), 256 threads: k_guided_search with the run of the query's node in place of the window's
 * cells.  The frame rule (train frame, status, counts) is k_guided_finish's, which reads the same call: gd_frame_of. */
__global__ __launch_bounds__(256) void k_bow_search(ssk_guided_call a, const int32_t *q_node, const uint64_t *index, const int32_t *n_index)
{
    const int b = (int)blockIdx.y, rows = a.rows;
    const int i = (int)(blockIdx.x * 64 + (threadIdx.x >> 2)), sub = (int)(threadIdx.x & 3);
    const gd_frame f = gd_frame_of(a.src, a.frame_error, a.nq, a.nt, rows, b);
    const int t = f.t, nt = f.nt;
    const bool live = i < f.nq;
    const int node = live ? q_node[(size_t)b * rows + i] : -1;
    uint32_t best = GD_NONE, second = 0xFFFFu, count = 0;
    if (live && nt > 0 && node >= 0) {
        const gd_desc q = gd_load_desc(a.q_desc + ((size_t)b * rows + i) * SS_DESC_BYTES);
        const uint8_t *td = a.t_desc + (size_t)t * rows * SS_DESC_BYTES;
        const int skip = (a.exclude_same_frame && t == b) ? i : -1;
        gd_walk_node(index + (size_t)t * rows, min(max(n_index[t], 0), rows), node, sub, [&](int row) {
            if (row >= nt || row == skip) return; /* row < nt: the index was made with the same count */
            const uint32_t dist = gd_hamming(q, td + (size_t)row * SS_DESC_BYTES);
            const uint32_t key = (dist << 20) | (uint32_t)row;
            count++;
            if (key < best) {
                second = min(second, gd_dist_of(best));
                best = key;
            } else {
                second = min(second, dist);
            }
        });
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

/* B-D.  grid (ceil(n_db / 4)), 256 threads: wave w of a block scores database vector 4 * block + w */
__global__ __launch_bounds__(256) void k_bow_score(const int32_t *q_word, const double *q_value, const int32_t *q_count, int q_rows,
                                                   const int32_t *db_word, const double *db_value, const int32_t *db_count, int n_db, int stride,
                                                   double *score)
{
    const int d = (int)(blockIdx.x * 4 + (threadIdx.x >> 6)), lane = (int)(threadIdx.x & 63);
    if (d >= n_db) return; /* a whole wave */
    const int nq = min(max(q_count[0], 0), q_rows), nd = min(max(db_count[d], 0), stride);
    const int32_t *dw = db_word + (size_t)d * stride;
    const double *dv = db_value + (size_t)d * stride;
    const double s = ss_bow_score_wave(q_word, q_value, nq, dw, dv, nd, lane); /* ss_bow_merge.h: the place recognition scores with it too */
    if (lane == 0) score[d] = s;
}

} // namespace

void ssk_bow_descend(hipStream_t s, const ssk_bow_voc &v, const ssk_bow_call &c)
{
    const int per = 256 / BW_LANES;
    hipLaunchKernelGGL(k_bow_descend, dim3((unsigned)((c.rows + per - 1) / per), (unsigned)c.n_frames), dim3(256), 0, s, v, c);
}

void ssk_bow_vector(hipStream_t s, const ssk_bow_voc &v, const ssk_bow_call &c)
{
    hipLaunchKernelGGL(k_bow_vector, dim3((unsigned)c.n_frames), dim3(BW_T), 0, s, v, c);
}

void ssk_bow_index(hipStream_t s, const int32_t *node, const int32_t *n_rows, const int32_t *frame_error, int n_frames, int rows,
                   uint64_t *index, int32_t *n_index)
{
    hipLaunchKernelGGL(k_bow_index, dim3((unsigned)n_frames), dim3(BW_T), 0, s, node, n_rows, frame_error, rows, index, n_index);
}

void ssk_bow_search(hipStream_t s, const ssk_guided_call &g, const int32_t *q_node, const uint64_t *index, const int32_t *n_index)
{
    hipLaunchKernelGGL(k_bow_search, dim3((unsigned)((g.rows + 63) / 64), (unsigned)g.n_frames), dim3(256), 0, s, g, q_node, index, n_index);
}

void ssk_bow_score(hipStream_t s, const int32_t *q_word, const double *q_value, const int32_t *q_count, int q_rows, const int32_t *db_word,
                   const double *db_value, const int32_t *db_count, int n_db, int stride, double *score)
{
    hipLaunchKernelGGL(k_bow_score, dim3((unsigned)((n_db + 3) / 4)), dim3(256), 0, s, q_word, q_value, q_count, q_rows, db_word, db_value,
                       db_count, n_db, stride, score);
}
