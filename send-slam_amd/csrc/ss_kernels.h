/* ss_kernels.h -- host-callable launch wrappers of ss_kernels.hip (all asynchronous on `s`). */
#ifndef SS_KERNELS_H
#define SS_KERNELS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/sendslam_orb.h"
#include "ss_layout.h"
#include "ss_place_steps.h" /* ss_place_db, a member of ssk_place_call */
#include "ss_undistort_steps.h" /* ss_undist_cam, the table of ssk_undistort_call */

/* level 0 read in place from the caller's buffer (ptr != NULL: 1-channel image, 16-byte aligned base, row and frame
 * strides; no k_ingest pass), or from the pyramid block (ptr == NULL) */
struct ss_lvl0 {
    const uint8_t *ptr = nullptr;
    int pitch = 0;
    int64_t frame_stride = 0;
};

/* Every device pointer of an extraction context (ss_layout.h; ss_api.cpp's ws_table is the one place their sizes live).  A
 * wrapper below picks the ones its kernel takes by name. */
struct ssk_extract_ws {
    /* tables uploaded once per geometry */
    ss_geom *dg = nullptr;
    ss_rtab *rtab = nullptr;
    uint32_t *tile_recs = nullptr; /* per-tile records (the FAST kernel's blocks in a launch too small to fill the chip), then its per-block records of two stacked tiles (SS_TILE_REC_WORDS each) */
    uint16_t *cinfo = nullptr;
    uint32_t *cell_units = nullptr;
    /* per-batch buffers, [batch slot][...] */
    uint8_t *pyr = nullptr, *blur = nullptr;
    uint8_t *score = nullptr;                   /* the FAST response map: NULL until ss_debug_fetch(2) asks for it, no kernel reads it */
    uint32_t *tsurv = nullptr, *thdr = nullptr; /* per 64x32 tile: survivor sub-lists and their count words */
    uint32_t *bucket = nullptr;                 /* per cell: NMS survivors, unordered */
    uint32_t *cell_cnt = nullptr;
    uint32_t *cand = nullptr, *qbuf0 = nullptr, *qbuf1 = nullptr;
    ss_qnode *nodes = nullptr;
    int32_t *lists = nullptr;
    uint32_t *sel = nullptr;
    ss_level_state *state = nullptr;
    uint32_t *kp_ref = nullptr;                 /* (reference, record) per output slot */
    /* per slot, between the three launches of ssk_orient_describe: the integer patch moments (m10, m01), then the float
     * (sin, cos) of the keypoint's angle */
    int2 *od_moments = nullptr;
    float2 *od_steer = nullptr;
    int32_t *n_kp = nullptr, *level_counts = nullptr, *frame_error = nullptr;
    ss_keypoint *kps = nullptr;
    uint8_t *desc = nullptr;
    uint8_t *desc_x = nullptr; /* the descriptors as 256 FP4 values (+1 / -1) per row, 128 B: operand of the batch matcher, or NULL */
};

/* The extraction stages of n_frames frames of geometry hg (the host copy of *ws.dg), in launch order. */
/* src -> level 0 in ws.pyr: the gray weights c0, c1, c2 of its channels, its row and frame strides */
void ssk_ingest(hipStream_t s, const ssk_extract_ws &ws, const ss_geom &hg, int n_frames, const void *src, int channels,
                int64_t row_stride, int64_t frame_stride, int c0, int c1, int c2);
/* one pyramid step, by the kernel the launch's size asks for: k_resize_walk (bands of 32 rows, else of 16) where `walk`
 * (= ssk_resize_walk_fits(host geometry, HOST tap tables, level), asked once per geometry) and the launch has at least
 * `wave_slots` waves (SSK_WAVE_SLOTS_PER_CU x the compute units of the context's device: the waves k_resize_walk keeps
 * resident, eight per SIMD), else k_resize_lds, else k_resize; returns which */
enum { SSK_WAVE_SLOTS_PER_CU = 32 };
enum { SSK_RESIZE_DIRECT = 1, SSK_RESIZE_WALK32 = 2, SSK_RESIZE_PAIR = 3, SSK_RESIZE_LDS = 4, SSK_RESIZE_WALK16 = 5 };
bool ssk_resize_walk_fits(const ss_geom &hg, const ss_rtab *host_rtab, int level);
int ssk_resize(hipStream_t s, const ssk_extract_ws &ws, const ss_geom &hg, int n_frames, int level, const ss_lvl0 &l0, bool walk, int64_t wave_slots);
/* levels `level` and `level + 1` in one launch (k_resize_pair), where ssk_resize_pair_fits(host geometry, HOST tap tables)
 * said so */
bool ssk_resize_pair_fits(const ss_geom &hg, const ss_rtab *host_rtab, int level);
void ssk_resize_pair(hipStream_t s, const ssk_extract_ws &ws, const ss_geom &hg, int n_frames, int level, const ss_lvl0 &l0);
/* K2 + K3a + K6a fused: FAST response map (where ws.score exists), in-window NMS into per-tile survivor sub-lists, blurred
 * pyramid -- one staged tile, no global atomics */
void ssk_fast_blur_nms(hipStream_t s, const ssk_extract_ws &ws, const ss_geom &hg, int n_frames, const ss_lvl0 &l0);
/* tile sub-lists -> per-cell buckets + count words (one thread per cell) */
void ssk_bucket_gather(hipStream_t s, const ssk_extract_ws &ws, const ss_geom &hg, int n_frames);
/* K3b: ranks the bucket entries of every cell into upstream's candidate order */
void ssk_cells_emit(hipStream_t s, const ssk_extract_ws &ws, const ss_geom &hg, int n_frames);
void ssk_quadtree(hipStream_t s, const ssk_extract_ws &ws, const ss_geom &hg, int n_frames);
void ssk_slots(hipStream_t s, const ssk_extract_ws &ws, const ss_geom &hg, int n_frames);
void ssk_orient_describe(hipStream_t s, const ssk_extract_ws &ws, const ss_geom &hg, int n_frames, const ss_lvl0 &l0, bool steer_fma);

/* Table form of a matcher call (ss_match_batch_sources_device): query frame b is matched against src[b] (device int32 [n_frames])
 * instead of b + train_frame_shift.  src[b] >= 0: frame src[b] of the batch, the self pair excluded iff src[b] == b; -1: no train
 * (idx -1, d1 / d2 0xFFFF); <= -2: carry frame -2 - src[b], with carry_n[c] rows, at the train's frame stride (carry_p packed
 * 32-byte rows; carry_x expanded rows, needed on operand rows only).  Always the compact kernel forms. */
struct ssk_table {
    const int32_t *src;
    const void *carry_p, *carry_x;
    const int32_t *carry_n;
};
/* One batch or single matcher call, filled by field name.  Its rows are packed 32-byte descriptors (k_match, from
 * SSK_MATCH_MFMA_MIN_QUERIES query rows per frame on k_match_mfma) or, with operand_rows, descriptors expanded to one FP4 value
 * (+1 / -1) per bit (k_match_mfma_x; desc_x of ssk_orient_describe, ssk_expand_desc*: SSK_X_ROW bytes per row, multiples of 32
 * rows allocated). */
#define SSK_X_ROW 128
struct ssk_match_call {
    hipStream_t s = nullptr;
    int n_frames = 1;
    bool operand_rows = false;
    const void *query = nullptr, *train = nullptr;           /* the rows the first launch reads */
    int64_t q_frame_stride = 0, t_frame_stride = 0;          /* packed rows: in 32-bit words; operand rows: in BYTES */
    /* operand rows: the same rows as packed descriptors where the caller has them, frame strides in bytes (the second launch,
     * which recomputes 15 distances per query, then reads a quarter of the bytes; a single chunk finishes in the first) */
    const uint8_t *query_p = nullptr, *train_p = nullptr;
    int64_t qp_frame_stride = 0, tp_frame_stride = 0;
    const int32_t *nq_arr = nullptr, *nt_arr = nullptr;      /* device row counts per frame, or null: nq_fixed / nt_fixed */
    int nq_fixed = 0, nt_fixed = 0;
    int train_frame_shift = 0;                               /* query frame b against train frame b + shift */
    int exclude_self_mode = 0;                               /* 0 never, 1 always, 2 when train frame == query frame */
    int th = 0, rnum = 0, rden = 0;                          /* the acceptance test */
    int out_stride = 0;                                      /* rows per frame of partial, idx, d1, d2 */
    void *partial = nullptr;                                 /* of the bytes ssk_match_plan returned */
    int32_t *idx = nullptr;
    uint16_t *d1 = nullptr, *d2 = nullptr;
    const ssk_table *tab = nullptr;                          /* the table form: exclude_self_mode 2, no shift, counts per frame */
    /* written by ssk_match_plan: the train split (a launch has >> 256 workgroups, local indices fit their bits) and the
     * matrix-core kernel's form, k_match_mfma's NU or k_match_mfma_x compact (1) / pipelined (2) */
    int chunk_len = 0, n_chunks = 0, tiles_per_wave = 1;
};
#define SSK_MATCH_PARTIAL_BYTES 8
/* Plans a call of rows_q query against rows_t train rows per frame (operand rows: reads SENDSLAM_MX_FORM and SENDSLAM_MX_CHUNKS,
 * once).  Returns the bytes of `partial` the launch needs, n_frames * n_chunks * out_stride records (operand rows: always;
 * packed rows: with more than one chunk), or 0. */
size_t ssk_match_plan(ssk_match_call &m, int rows_q, int rows_t);
/* The launches of a planned call: the first kernel and, unless that finished its queries itself, the merge or finish of the
 * chunk partials (one frame with fixed counts and >= 32 chunks: k_match_merge_wide before it or in its place). */
void ssk_match(const ssk_match_call &m);
/* (idx, d1, d2) of a raw match -> ss_match_part records with global rows (row_offset + idx) */
void ssk_pack_partial(hipStream_t s, const int32_t *idx, const uint16_t *d1, const uint16_t *d2, int n, int32_t row_offset,
                      void *part);
/* cross-shard fold: parts [n_parts][nq] in ascending row order -> final outputs (k_match_merge's rule) */
void ssk_match_fold(hipStream_t s, const void *parts, int n_parts, int nq, int th, int rnum, int rden, int32_t *idx,
                    uint16_t *d1, uint16_t *d2);
void ssk_match_fold_strided(hipStream_t s, const void *parts, int64_t part_stride_bytes, int n_parts, int nq, int th, int rnum, int rden,
                            int32_t *idx, uint16_t *d1, uint16_t *d2);
/* pipe match_mode 2: carry frame dst[i] <- batch frame src[i] (packed rows [kcap][32], row count clamped to kcap), i < n <=
 * SSK_CARRY_MAX, one launch */
#define SSK_CARRY_MAX 8
void ssk_carry_gather(hipStream_t s, const void *desc, const int32_t *n_kp, int kcap, const int32_t *dst, const int32_t *src, int n, void *carry,
                      int32_t *carry_n);
/* packed 32-B descriptors -> expanded SSK_X_ROW-byte rows; `out` holds n rounded up to 32 rows */
void ssk_expand_desc(hipStream_t s, const void *packed, int n, void *out);
/* [n_frames][rows][32] packed -> [n_frames][rows rounded up to 32][SSK_X_ROW] */
void ssk_expand_desc_frames(hipStream_t s, const void *packed, int rows, int n_frames, void *out);
/* ss_stereo.hip: stereo depth of the pairs (2p, 2p + 1) of a batch of n_frames (even); points [n_frames / 2][kcap]
 * ss_stereo_point, summary [n_frames / 2] ss_stereo_summary.  search writes every row (right_idx / orb_dist or "none"), refine
 * fills sad / u_right / depth of the matched rows from the unblurred pyramids, cut applies the median test and writes the
 * summaries */
struct ssk_stereo_call {
    float bf = 0, max_d = 0, min_d = 0, close_depth = 0; /* ComputeStereoMatches' constants */
    const int32_t *frame_error = nullptr;                /* in place of ws.frame_error (the stereo test hook), or NULL */
    void *points = nullptr, *summary = nullptr;
};
void ssk_stereo_search(hipStream_t s, const ssk_extract_ws &ws, const ss_geom &hg, int n_frames, const ssk_stereo_call &st);
void ssk_stereo_refine(hipStream_t s, const ssk_extract_ws &ws, const ss_geom &hg, int n_frames, const ss_lvl0 &l0, const ssk_stereo_call &st);
void ssk_stereo_cut(hipStream_t s, const ssk_extract_ws &ws, const ss_geom &hg, int n_frames, const ssk_stereo_call &st);
/* ss_guided.hip: window search of n_frames (query frame, train frame) pairs (DESIGN.md "Guided matching").  Both sides are
 * [frames][rows] arrays of keypoints and packed descriptors with per-frame counts; query frame b is matched against train frame
 * src[b] (device int32 [n_frames]; -1 = no train; NULL = frame b).  index bins the keypoints of each train frame into the cells of a grid (cell_start, recs), search walks the cells a query's window meets and writes the raw best /
 * second best, the accepted index and the candidate count of every row, finish applies the one-to-one and orientation filters
 * and writes the summaries. */
#define SSK_GUIDED_MAX_CELLS 4096 /* grid cells per train frame: their counts and offsets live in one workgroup's LDS */
struct ssk_guided_call {
    int n_frames = 0, rows = 0; /* frames on both sides, rows per frame */
    const ss_keypoint *q_kp = nullptr, *t_kp = nullptr;
    const uint8_t *q_desc = nullptr, *t_desc = nullptr;
    const int32_t *nq = nullptr, *nt = nullptr;
    const int32_t *src = nullptr;
    const int32_t *frame_error = nullptr;       /* per frame of both sides (the batch form: they are the same frames), or NULL */
    int exclude_same_frame = 0;                 /* the pair j == i is no candidate when src[b] == b */
    const ss_guided_window *windows = nullptr;  /* [n_frames][rows], or NULL: the query's own position, radius (* scale[octave]
                                                 * of *dg), octave -+ octave_span */
    const ss_geom *dg = nullptr;
    float radius = 0;
    int radius_by_octave = 0, octave_span = 0;
    int th = 0, rnum = 0, rden = 0, one_to_one = 0, orientation = 0;
    /* the grid (ssk_guided_grid): cells of 1 << shift pixels, cols x grid_rows <= SSK_GUIDED_MAX_CELLS of them; coordinates are
     * clamped to [0, x_max] x [0, y_max] before they are binned */
    int shift = 0, cols = 1, grid_rows = 1;
    float x_max = 0, y_max = 0;
    /* workspace: [n_frames][SSK_GUIDED_MAX_CELLS + 1] cell offsets, [n_frames][rows] 16-byte records,
     * [n_frames][rows] candidate counts */
    uint32_t *cell_start = nullptr;
    void *recs = nullptr;
    int32_t *n_cand = nullptr;
    int32_t *idx = nullptr;
    uint16_t *d1 = nullptr, *d2 = nullptr;
    ss_guided_summary *summary = nullptr;
};
void ssk_guided_grid(ssk_guided_call &g, int extent_w, int extent_h);
void ssk_guided_index(hipStream_t s, const ssk_guided_call &g);
void ssk_guided_search(hipStream_t s, const ssk_guided_call &g);
void ssk_guided_finish(hipStream_t s, const ssk_guided_call &g);
/* ss_proj.hip: map-point projection search (DESIGN.md "Projection search").  Frame b searches the points of block src[b]
 * ([n_blocks][point_rows] map points and descriptors, counts np) in its train frame b ([n_frames][rows] keypoints, descriptors,
 * optional right coordinates and taken flags, counts nt).  The train frames are indexed by ssk_guided_index on a guided call that
 * shares t_kp, nt, frame_error, the grid and the workspace; search evaluates frustum, level and window of every point and walks
 * the cells, finish applies one_to_one and writes the summaries. */
struct ssk_proj_call {
    int n_frames = 0, point_rows = 0, rows = 0;
    const ss_map_point *points = nullptr;
    const uint8_t *p_desc = nullptr;
    const int32_t *np = nullptr;
    const int32_t *src = nullptr;      /* device int32 [n_frames], or NULL: block b */
    const ss_proj_view *views = nullptr; /* device [n_frames] */
    const ss_keypoint *t_kp = nullptr;
    const uint8_t *t_desc = nullptr;
    const int32_t *nt = nullptr;
    const int32_t *frame_error = nullptr; /* per train frame, or NULL */
    const float *t_right = nullptr;       /* [n_frames][rows], or NULL */
    const uint8_t *t_taken = nullptr;     /* [n_frames][rows], or NULL */
    float view_cos_limit = 0, th = 0, far_limit = 0;
    int th_high = 0, rnum = 0, rden = 0, one_to_one = 0, check_right = 0;
    int n_levels = 1;
    float scale[SS_MAX_LEVELS] = {};
    /* the grid and the index of the guided call */
    int shift = 0, cols = 1;
    float x_max = 0, y_max = 0;
    const uint32_t *cell_start = nullptr;
    const void *recs = nullptr;
    int32_t *n_cand = nullptr; /* workspace [n_frames][point_rows] */
    int32_t *idx = nullptr;
    uint16_t *d1 = nullptr, *d2 = nullptr;
    ss_proj_point *proj = nullptr;
    ss_proj_summary *summary = nullptr;
};
void ssk_proj_search(hipStream_t s, const ssk_proj_call &g);
void ssk_proj_finish(hipStream_t s, const ssk_proj_call &g);
/* ss_fuse.hip: map-point fusion (DESIGN.md "Map-point fusion").  The operands of a projection call (blocks of points searched by
 * frames, the train side, the index of the guided call) plus the skip flags of the points ([n_frames][point_rows]) and the map-point
 * ids the train rows already carry ([n_frames][rows]).  search evaluates step 1 of every point, walks the cells and writes the best
 * row, its distance, the candidate count and the ss_fuse_point; finish turns them into one action per point and the summaries. */
struct ssk_fuse_call {
    int n_frames = 0, point_rows = 0, rows = 0;
    const ss_map_point *points = nullptr;
    const uint8_t *p_desc = nullptr;
    const int32_t *np = nullptr;
    const uint8_t *p_skip = nullptr;     /* [n_frames][point_rows], or NULL */
    const int32_t *src = nullptr;        /* device int32 [n_frames], or NULL: block b */
    const ss_proj_view *views = nullptr; /* device [n_frames] */
    const ss_keypoint *t_kp = nullptr;
    const uint8_t *t_desc = nullptr;
    const int32_t *nt = nullptr;
    const int32_t *frame_error = nullptr; /* per train frame, or NULL */
    const float *t_right = nullptr;       /* [n_frames][rows], or NULL */
    const uint8_t *t_taken = nullptr;     /* [n_frames][rows], or NULL */
    const int32_t *t_point = nullptr;     /* [n_frames][rows], or NULL */
    float view_cos_limit = 0, th = 0, chi2_mono = 0, chi2_stereo = 0;
    int th_low = 0, check_right = 0;
    int n_levels = 1;
    float scale[SS_MAX_LEVELS] = {};
    /* the grid and the index of the guided call */
    int shift = 0, cols = 1;
    float x_max = 0, y_max = 0;
    const uint32_t *cell_start = nullptr;
    const void *recs = nullptr;
    int32_t *n_cand = nullptr; /* workspace [n_frames][point_rows] */
    int32_t *idx = nullptr;
    uint16_t *d1 = nullptr;
    ss_fuse_action *fuse = nullptr;
    ss_fuse_point *point = nullptr;
    ss_fuse_summary *summary = nullptr;
};
void ssk_fuse_search(hipStream_t s, const ssk_fuse_call &g);
void ssk_fuse_finish(hipStream_t s, const ssk_fuse_call &g);
/* ss_bow.hip: vocabulary descent, BoW vectors, the node index and search of SearchByBoW, the L1 score (DESIGN.md "Bag of
 * words").  The vocabulary on the device, nodes numbered breadth first (0 = the root) so that a node's children are consecutive:
 * rows [n][32] descriptors, recs [n] ssk_bow_node, weight [n_words] doubles by word id. */
struct ssk_bow_node { /* 16 bytes: one dwordx4 */
    int32_t child_base, n_child; /* n_child 0 = a leaf */
    int32_t word;                /* -1 for an inner node */
    int32_t file_id;             /* the id the text file gives the node */
};
struct ssk_bow_voc {
    const uint8_t *rows = nullptr;
    const ssk_bow_node *recs = nullptr;
    const double *weight = nullptr;
    int L = 0, max_depth = 0, n_words = 0;
};
/* One transform call: [n_frames][rows] descriptors with per-frame counts (frame_error: per frame, or NULL).  descend writes
 * word / node of every row (node2: a second copy, or NULL), vector sorts a frame's words and nodes in LDS and writes the BoW
 * vector, the summary and, where index != NULL, the frame's node index: the keys node << 32 | row of its rows with node >= 0 in
 * ascending order, n_index[frame] of them. */
struct ssk_bow_call {
    int n_frames = 0, rows = 0, levelsup = 0;
    const uint8_t *desc = nullptr;
    const int32_t *n_rows = nullptr, *frame_error = nullptr;
    int32_t *word = nullptr, *node = nullptr, *node2 = nullptr;
    int32_t *bow_word = nullptr;
    double *bow_value = nullptr;
    ss_bow_summary *summary = nullptr;
    uint64_t *index = nullptr;
    int32_t *n_index = nullptr;
};
void ssk_bow_descend(hipStream_t s, const ssk_bow_voc &v, const ssk_bow_call &c);
void ssk_bow_vector(hipStream_t s, const ssk_bow_voc &v, const ssk_bow_call &c);
/* the node index alone, of caller-made nodes [n_frames][rows] with counts n_rows */
void ssk_bow_index(hipStream_t s, const int32_t *node, const int32_t *n_rows, const int32_t *frame_error, int n_frames, int rows,
                   uint64_t *index, int32_t *n_index);
/* fills idx / d1 / d2 / n_cand of a guided call whose candidates are the train rows of the query's node (q_node [n_frames][rows];
 * index / n_index of the train frames); ssk_guided_finish then runs on g as it is */
void ssk_bow_search(hipStream_t s, const ssk_guided_call &g, const int32_t *q_node, const uint64_t *index, const int32_t *n_index);
void ssk_bow_score(hipStream_t s, const int32_t *q_word, const double *q_value, const int32_t *q_count, int q_rows, const int32_t *db_word,
                   const double *db_value, const int32_t *db_count, int n_db, int stride, double *score);
/* ss_epi.hip: epipolar search and triangulation (DESIGN.md "Epipolar search and triangulation").  The search runs on a guided
 * call (operands, counts, src, frame_error, exclude_same_frame, th, one_to_one, orientation, idx, d1, n_cand; d2 is not written
 * and g.summary is a workspace row per pair) plus what follows; ssk_guided_finish then runs on g as it is, and ssk_epi_summary
 * turns its summary and the per-row counters into the ss_epi_summary of every pair. */
struct ssk_epi_call {
    const int32_t *q_node = nullptr;      /* [n_frames][rows] */
    const uint64_t *index = nullptr;      /* the node index of the train frames (ssk_bow_index), n_index keys each */
    const int32_t *n_index = nullptr;
    const uint8_t *q_taken = nullptr, *t_taken = nullptr; /* [n_frames][rows], or NULL */
    const ss_epi_pair *pairs = nullptr;   /* device [n_frames] */
    int coarse = 0, n_levels = 1;
    float scale[SS_MAX_LEVELS] = {};
    int32_t *n_geo = nullptr, *n_near = nullptr; /* workspace [n_frames][rows] */
    ss_epi_summary *summary = nullptr;
};
void ssk_epi_search(hipStream_t s, const ssk_guided_call &g, const ssk_epi_call &e);
void ssk_epi_summary(hipStream_t s, const ssk_guided_call &g, const ssk_epi_call &e);
/* Pair b triangulates the matches idx[b][i] of its query rows with the rows of train frame src[b] (NULL: b).  eval writes info and,
 * into the workspace tmp [n_frames][rows], the map point of every row; compact (one workgroup per pair, SSK_TRI_CHUNK rows at a
 * time, in ascending row order) gathers the state-0 rows into points / point_desc / point_rows, counts them and writes the summary */
#define SSK_TRI_CHUNK 1024
struct ssk_tri_call {
    int n_frames = 0, rows = 0;
    const ss_keypoint *q_kp = nullptr, *t_kp = nullptr;
    const uint8_t *q_desc = nullptr;
    const int32_t *nq = nullptr, *nt = nullptr;
    const int32_t *src = nullptr;
    const int32_t *frame_error = nullptr;
    const int32_t *idx = nullptr;
    const ss_epi_pair *pairs = nullptr; /* device [n_frames] */
    ss_tri_params tp = {};
    int n_levels = 1;
    float scale[SS_MAX_LEVELS] = {};
    ss_map_point *tmp = nullptr;
    ss_tri_info *info = nullptr;
    ss_map_point *points = nullptr;
    uint8_t *point_desc = nullptr;
    int32_t *point_rows = nullptr;
    int32_t *n_points = nullptr;
    ss_tri_summary *summary = nullptr;
};
void ssk_tri_eval(hipStream_t s, const ssk_tri_call &t);
void ssk_tri_compact(hipStream_t s, const ssk_tri_call &t);
/* The stereo form: eval reads the planes of both sides (query row i of pair b at x1 + (b * rows + i) * stride, train row j of frame
 * f = src[b] (NULL: b) at x2 + (f * rows + j) * stride), writes sinfo and, for ssk_tri_compact as it is, the mono record t.info
 * (workspace) and the point into t.tmp; compact writes t.summary (workspace); summary adds the state-0 rows per mode */
struct ssk_tri_stereo_call {
    ssk_tri_call t;
    const uint8_t *depth1 = nullptr, *right1 = nullptr, *depth2 = nullptr, *right2 = nullptr;
    int64_t depth1_stride = 4, right1_stride = 4, depth2_stride = 4, right2_stride = 4;
    const ss_tri_stereo_rig *rigs = nullptr; /* device [n_frames] */
    double chi2_stereo = 0.0;
    ss_tri_stereo_info *sinfo = nullptr;
    ss_tri_stereo_summary *ssummary = nullptr;
};
void ssk_tri_stereo_eval(hipStream_t s, const ssk_tri_stereo_call &c);
void ssk_tri_stereo_summary(hipStream_t s, const ssk_tri_stereo_call &c);
/* ss_sim3.hip: Sim3 from matched map points (DESIGN.md "Sim3 RANSAC").  Pair b solves the matches idx[b][i] of its query rows with
 * the rows of train frame src[b] (NULL: b).  gather (one workgroup per pair, SSK_SIM3_CHUNK rows at a time in ascending order)
 * numbers the correspondences and writes their twelve floats as a structure of arrays (corr: 12 planes of [n_frames][rows]), the
 * number of every query row's correspondence (corr_of_row, -1: none) and N; model (one lane per pair and hypothesis) writes one
 * ssk_sim3_model and zeroes its count; count (a lane per correspondence, SSK_SIM3_COUNT_ROWS of them and SSK_SIM3_HYP_BLOCK
 * hypotheses per workgroup) adds the inliers; finish (one workgroup per pair) selects and writes flags and result */
#define SSK_SIM3_CHUNK 1024
#define SSK_SIM3_COUNT_ROWS 256
#define SSK_SIM3_HYP_BLOCK 32
struct alignas(16) ssk_sim3_model { /* 128 bytes, so that a wave reads one with wide scalar loads */
    float sr12[9], t12[3], sr21[9], t21[3], s12;
    float pad[7];
};
/* the two sides of the pairs of a call: what the Sim3 RANSAC and the Sim3 refinement read of them */
struct ssk_pair_sides {
    int n_frames = 0, rows = 0;
    const ss_map_point *q_xyz = nullptr, *t_xyz = nullptr;
    const ss_keypoint *q_kp = nullptr, *t_kp = nullptr;
    const uint8_t *q_skip = nullptr, *t_skip = nullptr; /* [n_frames][rows], or NULL */
    const int32_t *nq = nullptr, *nt = nullptr;
    const int32_t *src = nullptr;
    const int32_t *frame_error = nullptr;
    const int32_t *idx = nullptr;
    const ss_proj_view *views1 = nullptr, *views2 = nullptr; /* device [n_frames] each */
};
struct ssk_sim3_call : ssk_pair_sides {
    float chi2 = 0;
    int min_inliers = 0, max_iterations = 1, fix_scale = 0;
    uint32_t seed = 0;
    int n_levels = 1;
    float scale[SS_MAX_LEVELS] = {};
    /* workspace */
    float *corr = nullptr;
    int32_t *corr_of_row = nullptr; /* [n_frames][rows] */
    int32_t *n_corr = nullptr;      /* [n_frames] */
    ssk_sim3_model *models = nullptr; /* [n_frames][max_iterations] */
    int32_t *counts = nullptr;        /* [n_frames][max_iterations] */
    uint8_t *inlier = nullptr;
    ss_sim3_result *result = nullptr;
};
void ssk_sim3_gather(hipStream_t s, const ssk_sim3_call &g);
void ssk_sim3_model_launch(hipStream_t s, const ssk_sim3_call &g);
void ssk_sim3_count(hipStream_t s, const ssk_sim3_call &g);
void ssk_sim3_finish(hipStream_t s, const ssk_sim3_call &g);
/* ss_pose.hip: pose-only optimisation (DESIGN.md "Pose-only optimisation").  Frame b optimises its start pose on the observations
 * its slots give: slot i pairs point row i of block src[b] with keypoint row idx[b][i] (idx_by_row: keypoint row i with point row
 * idx[b][i]); slots = idx_by_row ? rows : point_rows.  gather (one workgroup per frame, SSK_POSE_CHUNK slots at a time in ascending
 * order) numbers the observations, writes their seven floats as a structure of arrays (planes: 7 of [n_frames][slots]), the slot of
 * every observation and N, and flag 2 into every other slot; solve (one workgroup per frame) runs every round and step and writes
 * the observations' flags and the result */
#define SSK_POSE_CHUNK 1024
struct ssk_pose_call {
    int n_frames = 0, point_rows = 0, rows = 0, slots = 0;
    const ss_map_point *points = nullptr; /* [n_blocks][point_rows] */
    const uint8_t *p_skip = nullptr;      /* [n_blocks][point_rows], or NULL */
    const int32_t *np = nullptr;
    const int32_t *src = nullptr;         /* device int32 [n_frames] */
    const ss_proj_view *views = nullptr;  /* device [n_frames] */
    const double *start = nullptr;        /* device [n_frames][12] */
    const ss_keypoint *kp = nullptr;      /* [n_frames][rows] */
    const float *right = nullptr;         /* [n_frames][rows], or NULL */
    const int32_t *nk = nullptr;
    const int32_t *frame_error = nullptr; /* per frame, or NULL */
    const int32_t *idx = nullptr;         /* [n_frames][slots] */
    double chi2_mono = 0, chi2_stereo = 0, lambda = 0, step_eps = 0;
    int n_rounds = 1, iterations = 1, robust_rounds = 0, min_obs = 3, check_right = 0, idx_by_row = 0;
    int n_levels = 1;
    float scale[SS_MAX_LEVELS] = {};
    /* workspace */
    float *planes = nullptr;
    int32_t *slot_of = nullptr; /* [n_frames][slots] */
    int32_t *n_obs = nullptr;   /* [n_frames] */
    uint8_t *flags = nullptr;   /* [n_frames][slots] */
    ss_pose_result *result = nullptr;
};
void ssk_pose_gather(hipStream_t s, const ssk_pose_call &g);
void ssk_pose_solve(hipStream_t s, const ssk_pose_call &g);
/* ss_pnp.hip: PnP RANSAC (DESIGN.md "PnP RANSAC").  Problem q solves the matches idx[q][i] of the rows of keypoint frame kp_src[q]
 * with the rows of point block point_src[q].  gather (one workgroup per problem, SSK_PNP_CHUNK rows at a time in ascending order)
 * numbers the correspondences and writes their six floats as a structure of arrays (corr: 6 planes of [n_frames][rows]: X Y Z u v
 * max), the two values only the model reads (corr_scale, corr_point: the keypoint's scale and the point row), the number of every
 * row's correspondence (corr_of_row, -1: none) and N; model (one lane per problem and hypothesis) writes one ssk_pnp_model, the
 * pose's twelve doubles and zeroes its count; count (a lane per correspondence, SSK_PNP_COUNT_ROWS of them and SSK_PNP_HYP_BLOCK
 * hypotheses per workgroup) adds the inliers; finish (one workgroup per problem) selects and writes flags and result */
#define SSK_PNP_CHUNK 1024
#define SSK_PNP_COUNT_ROWS 256
#define SSK_PNP_HYP_BLOCK 32
struct alignas(16) ssk_pnp_model { /* 64 bytes, so that a wave reads one with wide scalar loads */
    float r[9], t[3];
    float pad[4];
};
struct ssk_pnp_call {
    int n_frames = 0, point_rows = 0, rows = 0; /* n_frames: the problems of the call */
    const ss_map_point *points = nullptr; /* [n_blocks][point_rows] */
    const uint8_t *p_skip = nullptr;      /* [n_blocks][point_rows], or NULL */
    const int32_t *np = nullptr;
    const ss_keypoint *kp = nullptr;      /* [n_kp_frames][rows] */
    const int32_t *nk = nullptr;
    const int32_t *frame_error = nullptr; /* per keypoint frame, or NULL */
    const int32_t *kp_src = nullptr, *point_src = nullptr; /* device int32 [n_frames] each */
    const ss_proj_view *views = nullptr;  /* device [n_frames] */
    const int32_t *idx = nullptr;         /* [n_frames][rows] */
    float chi2 = 0, min_ratio = 0;
    double lambda = 0;
    int min_inliers = 0, max_iterations = 1, refine_steps = 0;
    uint32_t seed = 0;
    int n_levels = 1;
    float scale[SS_MAX_LEVELS] = {};
    /* workspace */
    float *corr = nullptr;          /* 6 planes */
    float *corr_scale = nullptr;    /* [n_frames][rows] */
    int32_t *corr_point = nullptr;  /* [n_frames][rows] */
    int32_t *corr_of_row = nullptr; /* [n_frames][rows] */
    int32_t *n_corr = nullptr;      /* [n_frames] */
    ssk_pnp_model *models = nullptr; /* [n_frames][max_iterations] */
    double *poses = nullptr;         /* [n_frames][max_iterations][12] */
    int32_t *counts = nullptr;       /* [n_frames][max_iterations] */
    uint8_t *inlier = nullptr;       /* [n_frames][rows] */
    ss_pnp_result *result = nullptr;
};
void ssk_pnp_gather(hipStream_t s, const ssk_pnp_call &g);
void ssk_pnp_model_launch(hipStream_t s, const ssk_pnp_call &g);
void ssk_pnp_count(hipStream_t s, const ssk_pnp_call &g);
void ssk_pnp_finish(hipStream_t s, const ssk_pnp_call &g);
/* ss_two_view.hip: two-view initialisation (DESIGN.md "Two-view initialisation").  Problem q solves the matches idx[q][i] of the rows
 * of frame kp1_src[q] with the rows of frame kp2_src[q] (< 0: no frame 2).  gather (one workgroup per problem, SSK_TV_GATHER_ROWS rows at a
 * time in ascending order) numbers the correspondences, writes their four floats as a structure of arrays (corr: 4 planes of
 * [n_frames][rows]: u1 v1 u2 v2), the number of every row's correspondence (corr_of_row, -1: none), N and the normalisation; model
 * (one lane per problem and hypothesis) writes one ssk_tv_model; score (a lane per correspondence, SS_TV_CHUNK of them and
 * SSK_TV_HYP_BLOCK hypotheses per workgroup) writes both scores' partial sums per (chunk, hypothesis); select (one workgroup per
 * problem) adds them, picks both winners and the model, flags its inliers and decomposes it; check (a lane per correspondence)
 * counts the good points of every motion hypothesis; finish (one workgroup per problem) accepts and writes flags, points and result */
#define SSK_TV_GATHER_ROWS 1024
#define SSK_TV_HYP_BLOCK 32
struct alignas(16) ssk_tv_model { /* 256 bytes */
    double h21[9], h12[9], f21[9];
    int32_t ok_h, ok_f;
    double pad[4];
};
struct alignas(8) ssk_tv_choice { /* per problem, select -> check and finish */
    double hyp[12 * 8];
    double norm[8];       /* m[4], d[4] */
    double score_h, score_f;
    int32_t norm_ok, model, n_hyp, reason, n_in, t_h, t_f, pad;
    int32_t good[8];
};
struct ssk_tv_call {
    int n_frames = 0, rows = 0; /* n_frames: the problems of the call */
    const ss_keypoint *kp1 = nullptr, *kp2 = nullptr; /* [frames][rows] */
    const int32_t *n1 = nullptr, *n2 = nullptr;
    const int32_t *frame_error = nullptr; /* per frame of either side (the batch form), or NULL */
    const int32_t *kp1_src = nullptr, *kp2_src = nullptr; /* device int32 [n_frames] each */
    const ss_proj_view *views = nullptr;  /* device [n_frames] */
    const int32_t *idx = nullptr;         /* [n_frames][rows] */
    ss_two_view_params p = {};
    int n_levels = 1;
    float scale[SS_MAX_LEVELS] = {};
    /* workspace */
    float *corr = nullptr;          /* 4 planes */
    int32_t *corr_of_row = nullptr; /* [n_frames][rows] */
    uint8_t *corr_flag = nullptr;   /* [n_frames][rows], by correspondence: 1 an inlier of the chosen model */
    int32_t *n_corr = nullptr;      /* [n_frames] */
    ssk_tv_model *models = nullptr; /* [n_frames][max_iterations] */
    double *partial = nullptr;      /* [n_frames][chunks][max_iterations][2] */
    ssk_tv_choice *choice = nullptr; /* [n_frames] */
    /* outputs */
    uint8_t *flag = nullptr;        /* [n_frames][rows] */
    ss_map_point *points = nullptr; /* [n_frames][rows] */
    int32_t *point_rows = nullptr;  /* [n_frames][rows][2] */
    int32_t *n_points = nullptr;
    ss_two_view_result *result = nullptr;
};
void ssk_tv_gather(hipStream_t s, const ssk_tv_call &g);
void ssk_tv_model_launch(hipStream_t s, const ssk_tv_call &g);
void ssk_tv_score(hipStream_t s, const ssk_tv_call &g);
void ssk_tv_select(hipStream_t s, const ssk_tv_call &g);
void ssk_tv_check(hipStream_t s, const ssk_tv_call &g);
void ssk_tv_finish(hipStream_t s, const ssk_tv_call &g);
/* ss_sim3opt.hip: Sim3 refinement (DESIGN.md "Sim3 refinement").  Pair b as for ssk_sim3_call, and start[b], the model it starts
 * from.  gather (one workgroup per pair, SSK_SIM3OPT_CHUNK rows at a time in ascending order) numbers the correspondences, writes
 * their twelve floats as a structure of arrays (planes: 12 of [n_frames][rows]: X1, X2, both keypoints, both scales), the query row
 * of every correspondence and N, and flag 2 into every other row; solve (one workgroup per pair) runs both rounds and writes the
 * correspondences' flags and the result */
#define SSK_SIM3OPT_CHUNK 1024
struct ssk_sim3opt_call : ssk_pair_sides {
    const ss_sim3_result *start = nullptr;                   /* device [n_frames] */
    ss_sim3_opt_params p = {};
    int n_levels = 1;
    float scale[SS_MAX_LEVELS] = {};
    /* workspace */
    float *planes = nullptr;
    int32_t *row_of = nullptr; /* [n_frames][rows] */
    int32_t *n_corr = nullptr; /* [n_frames] */
    uint8_t *flags = nullptr;  /* [n_frames][rows] */
    ss_sim3_opt_result *result = nullptr;
};
void ssk_sim3opt_gather(hipStream_t s, const ssk_sim3opt_call &g);
void ssk_sim3opt_solve(hipStream_t s, const ssk_sim3opt_call &g);
/* ss_ba.hip: local bundle adjustment (DESIGN.md "Local bundle adjustment").  Problem q owns the frames prob[q].first_frame .. of the
 * call and reads block prob[q].point_block; P = point_rows.  Every kernel of the fixed schedule reads its problem's ssk_ba_state and
 * returns at once when the problem has ended or the round is over.  Poses and points are double-buffered: st.cur names the buffer
 * of the current state, the other one takes the trial state, and an accepted step flips cur.  obs and pflag are the caller's
 * output arrays, which carry the rule's bytes from the gather on */
struct ssk_ba_state {
    double lambda, cost0, cost_before;
    int32_t state, status, ended, round_over, cur, pose_small, pose_finite;
    int32_t n_obs, n_stereo, n_frozen_max;
    int32_t steps[4], accepted[4];
};
struct ssk_ba_meas { /* ss_ba_meas of ss_ba_steps.h */
    float u, v, ur, scale;
};
struct ssk_ba_call {
    int n_frames = 0, n_problems = 0, point_rows = 0, rows = 0;
    int max_kf = 0, max_free = 0;          /* the largest of the call's problems */
    const ss_map_point *points = nullptr; /* [n_blocks][point_rows] */
    const uint8_t *p_skip = nullptr;      /* [n_blocks][point_rows], or NULL */
    const int32_t *np = nullptr;
    const ss_keypoint *kp = nullptr;      /* [n_frames][rows] */
    const float *right = nullptr;         /* [n_frames][rows], or NULL */
    const int32_t *nk = nullptr;
    const int32_t *frame_error = nullptr; /* per frame, or NULL */
    const int32_t *idx = nullptr;         /* [n_frames][point_rows] */
    const ss_ba_problem *prob = nullptr;  /* device [n_problems] */
    const int32_t *frame_prob = nullptr;  /* device [n_frames]: the frame's problem, or -1 */
    const ss_proj_view *views = nullptr;  /* device [n_frames] */
    const double *start = nullptr;        /* device [n_frames][12] */
    ss_ba_params p = {};
    int n_levels = 1;
    float scale[SS_MAX_LEVELS] = {};
    /* workspace */
    ssk_ba_meas *meas = nullptr;  /* [n_frames][P] */
    uint8_t *lin = nullptr;       /* [n_frames][P]: the observation took part in this step's linearisation */
    double *pose = nullptr;       /* [2][n_frames][12] */
    double *X = nullptr;          /* [2][n_problems][P][3] */
    double *WY = nullptr;         /* [n_problems][max_free][36][P]: W (18 planes), then Y */
    double *Lb = nullptr;         /* [n_problems][9][P]: a point's factor (6 planes), then b */
    uint8_t *solved = nullptr;    /* [n_problems][P] */
    double *A = nullptr;          /* [n_problems][(6 max_free)^2]: the upper triangle of S, rows of 6 n_free */
    double *r = nullptr;          /* [n_problems][6 max_free] */
    double *dc = nullptr;         /* [n_problems][6 max_free] */
    double *cost_k = nullptr;     /* [n_problems][max_kf] */
    int32_t *blk = nullptr;       /* [n_problems][pblocks][4]: per workgroup of points, what a kernel hands to the next */
    ssk_ba_state *st = nullptr;   /* [n_problems] */
    /* outputs */
    double *out_pose = nullptr, *out_xyz = nullptr;
    uint8_t *pflag = nullptr, *obs = nullptr;
    ss_ba_result *result = nullptr;
};
void ssk_ba_gather(hipStream_t s, const ssk_ba_call &g);                 /* three launches */
void ssk_ba_cost(hipStream_t s, const ssk_ba_call &g, int round, int trial);
void ssk_ba_accept(hipStream_t s, const ssk_ba_call &g, int round, int begin);
void ssk_ba_points(hipStream_t s, const ssk_ba_call &g, int round);
void ssk_ba_blocks(hipStream_t s, const ssk_ba_call &g, int round);
void ssk_ba_solve(hipStream_t s, const ssk_ba_call &g);
void ssk_ba_update(hipStream_t s, const ssk_ba_call &g);
void ssk_ba_classify(hipStream_t s, const ssk_ba_call &g);
void ssk_ba_finish(hipStream_t s, const ssk_ba_call &g);                 /* two launches */
struct ssk_ba_block_call {
    int n = 0, point_rows = 0;
    const double *xyz = nullptr;
    const uint8_t *flags = nullptr;
    const int32_t *block_of = nullptr; /* device [n] */
    ss_map_point *points = nullptr;
};
void ssk_ba_points_to_block(hipStream_t s, const ssk_ba_block_call &g);
/* ss_graph.hip: essential-graph optimisation (DESIGN.md "Essential-graph optimisation").  Problem q owns the keyframes
 * prob[q].first_kf .. and the edges prob[q].first_edge .. of the call; keyframe and edge numbers are the call's everywhere.  Every
 * kernel of the fixed schedule reads its problem's ssk_graph_state and returns at once when the problem has ended.  The Sim3s are
 * double-buffered: st.cur names the buffer of the current state, the other one takes the trial state, an accepted step flips cur */
struct ssk_graph_state {
    double lambda, cost0, cost_before;
    int32_t state, ended, cur, n_free, steps, accepted, pcg, trial_finite;
};
struct ssk_graph_call {
    int n_kf = 0, n_problems = 0, n_edges = 0;
    int max_kf = 0, max_edges = 0;           /* the largest of the call's problems */
    const double *nc = nullptr;             /* [n_kf][13] */
    const double *start = nullptr;          /* [n_kf][13] */
    const uint8_t *fixed = nullptr;         /* [n_kf] */
    const ss_graph_problem *prob = nullptr; /* device [n_problems] */
    const int32_t *edges = nullptr;         /* device [n_edges][2] */
    const int32_t *kf_prob = nullptr;       /* device [n_kf]: the keyframe's problem, or -1 */
    const int32_t *inc_off = nullptr, *inc_cnt = nullptr; /* device [n_kf]: the keyframe's run of inc */
    const int32_t *inc = nullptr;           /* device [2 n_edges]: 2 * edge + side, ascending per keyframe */
    ss_graph_params p = {};
    /* workspace */
    double *S = nullptr;       /* [2][n_kf][13] */
    double *M = nullptr;       /* [n_edges][13] */
    double *err = nullptr;     /* [n_edges][7] */
    double *J = nullptr;       /* [n_edges][14][7]: column c of endpoint `side` at 7 (7 side + c) */
    double *u = nullptr;       /* [n_edges][7] */
    double *L = nullptr;       /* [n_kf][49]: the factor of a free keyframe's damped block */
    double *dd = nullptr, *g = nullptr, *x = nullptr, *r = nullptr, *z = nullptr, *pv = nullptr, *q = nullptr; /* [n_kf][7] each */
    uint8_t *flag = nullptr;   /* [n_kf]: gather: the Sim3s are usable; blocks: every pivot > 0 */
    ssk_graph_state *st = nullptr; /* [n_problems] */
    /* outputs */
    double *out_sim3 = nullptr, *out_pose = nullptr;
    ss_graph_result *result = nullptr;
};
void ssk_graph_gather(hipStream_t s, const ssk_graph_call &g); /* three launches; two without a problem */
void ssk_graph_lin(hipStream_t s, const ssk_graph_call &g);
void ssk_graph_blocks(hipStream_t s, const ssk_graph_call &g);
void ssk_graph_solve(hipStream_t s, const ssk_graph_call &g);
void ssk_graph_cost(hipStream_t s, const ssk_graph_call &g, int begin);
void ssk_graph_finish(hipStream_t s, const ssk_graph_call &g);
struct ssk_graph_points_call {
    int n_blocks = 0, point_rows = 0, n_kf = 0;
    ss_map_point *points = nullptr;
    const int32_t *ref = nullptr;
    const double *nc = nullptr, *sim3 = nullptr;
};
void ssk_graph_points(hipStream_t s, const ssk_graph_points_call &g);
/* ss_gba.hip: global bundle adjustment (DESIGN.md "Global bundle adjustment").  Problem q owns the keyframes prob[q].first_kf ..,
 * the blocks prob[q].first_block .. and the sorted records prob[q].first_obs .. of the call.  Keyframe, point (block * point_rows +
 * row) and record numbers index the call's arrays; what the tables hold (rec.kf, rec.point, the offsets and kf_list) is relative
 * to the problem, as ss_gba_tables builds it.  Every kernel of the fixed schedule reads its problem's ssk_gba_state and returns at
 * once when the problem has ended, its round is over or (the three kernels of a PCG iteration) its PCG has left.  Poses and
 * points are double-buffered as in ss_ba.hip */
struct ss_gba_rec; /* ss_gba_steps.h */
struct ssk_gba_state {
    double lambda, cost0, cost_before, rho, stop;
    int32_t state, ended, round_over, cur, n_free;
    int32_t pcg_live, pcg_done, pcg_total;
    int32_t n_obs, n_stereo, n_frozen_max, trial_ok;
    int32_t steps[4], accepted[4];
};
struct ssk_gba_call {
    int n_kf = 0, n_problems = 0, n_blocks = 0, point_rows = 0, n_obs = 0;
    int max_kf = 0;                        /* the largest of the call's problems */
    const ss_map_point *points = nullptr; /* [n_blocks][point_rows] */
    const uint8_t *p_skip = nullptr;      /* [n_blocks][point_rows], or NULL */
    const int32_t *np = nullptr;          /* [n_blocks] */
    const double *start = nullptr;        /* [n_kf][12] */
    const uint8_t *fixed = nullptr;       /* [n_kf] */
    const ss_gba_problem *prob = nullptr; /* device [n_problems] */
    const int32_t *kf_prob = nullptr;     /* device [n_kf]: the keyframe's problem, or -1 */
    const int32_t *blk_prob = nullptr;    /* device [n_blocks]: the block's problem, or -1 */
    const ss_proj_view *views = nullptr;  /* device [n_kf] */
    const ss_gba_rec *rec = nullptr;      /* device [n_obs]: a problem's records sorted; kf < 0: a record of no problem */
    const int32_t *pt_off = nullptr, *pt_cnt = nullptr; /* device [n_blocks * point_rows]: the point's run of rec */
    const int32_t *kf_off = nullptr, *kf_cnt = nullptr; /* device [n_kf]: the keyframe's run of kf_list */
    const int32_t *kf_list = nullptr;     /* device [n_obs] */
    ss_gba_params p = {};
    /* workspace */
    double *pose = nullptr;    /* [2][n_kf][12] */
    double *X = nullptr;       /* [2][points][3] */
    uint8_t *pflag = nullptr;  /* [points] */
    uint8_t *solved = nullptr; /* [points] */
    uint8_t *ob = nullptr;     /* [n_obs]: the rule's byte of every sorted record */
    uint8_t *lin = nullptr;    /* [n_obs]: the record took part in this step's linearisation */
    double *W = nullptr;       /* [n_obs][18]: the records of free keyframes */
    double *Lb = nullptr;      /* [points][12]: a point's factor (6), b (3), c of the operator (3) */
    double *U = nullptr;       /* [n_kf][21] */
    double *M = nullptr;       /* [n_kf][36]: the factor of a free keyframe's block */
    double *x = nullptr, *r = nullptr, *z = nullptr, *pv = nullptr, *q = nullptr; /* [n_kf][6] each */
    double *cost_k = nullptr;  /* [n_kf] */
    uint8_t *kf_flag = nullptr; /* [n_kf]: gather: the start is finite; blocks: every pivot > 0; update: bit 0 finite, 1 small, 2 too large */
    int32_t *part = nullptr;   /* [n_blocks * pblocks][4]: per workgroup of points, what a kernel hands to the next */
    ssk_gba_state *st = nullptr; /* [n_problems] */
    /* outputs */
    double *out_pose = nullptr, *out_xyz = nullptr;
    uint8_t *out_pflag = nullptr, *out_obs = nullptr;
    ss_gba_result *result = nullptr;
};
void ssk_gba_gather(hipStream_t s, const ssk_gba_call &g);  /* three launches */
void ssk_gba_cost(hipStream_t s, const ssk_gba_call &g, int round, int begin); /* two launches: the keyframes' trees, then the decision */
void ssk_gba_points(hipStream_t s, const ssk_gba_call &g, int round);
void ssk_gba_blocks(hipStream_t s, const ssk_gba_call &g, int round);          /* two launches: the blocks, then the start of the PCG */
void ssk_gba_pcg(hipStream_t s, const ssk_gba_call &g);                        /* one iteration: three launches */
void ssk_gba_update(hipStream_t s, const ssk_gba_call &g);                     /* two launches */
void ssk_gba_classify(hipStream_t s, const ssk_gba_call &g);
void ssk_gba_finish(hipStream_t s, const ssk_gba_call &g);                     /* three launches */
/* ss_covis.hip: covisibility (DESIGN.md "Covisibility").  One workgroup per row: a keyframe row names a keyframe of the map (rows
 * NULL: row r is keyframe r), a frame row the block its hits index (src) and its row of idx.  max_kf, the largest problem of the map,
 * sizes the weight counters in dynamic LDS */
struct ss_covis_tab; /* ss_covis_steps.h */
struct ssk_covis_call {
    const ss_covis_tab *tab = nullptr; /* HOST: the map's tables on the device */
    int n_rows = 0, cap = 0;
    const int32_t *rows = nullptr;     /* device [n_rows] or NULL: keyframe rows */
    const int32_t *src = nullptr;      /* device [n_rows]: the block of a frame row */
    const int32_t *idx = nullptr;      /* device [n_rows][point_rows] */
    const int32_t *np = nullptr;       /* device [n_blocks] */
    ss_covis_params p = {};
    int32_t *nb = nullptr;             /* device [n_rows][cap][2] */
    ss_covis_row *row = nullptr;       /* device [n_rows] */
};
int ssk_covis_kf(hipStream_t s, const ssk_covis_call &g);     /* a hipError_t: the LDS attribute may be refused */
int ssk_covis_frames(hipStream_t s, const ssk_covis_call &g);
/* ss_refresh.hip: the map-point refresh (DESIGN.md "Map-point refresh").  One wave per point row whose list has at most 64 records,
 * one workgroup per longer one (long_pts names them), then one workgroup per block for the summary: three launches */
struct ssk_refresh_call {
    const ss_covis_tab *tab = nullptr; /* HOST: the map's tables on the device */
    const int32_t *pt_row = nullptr;   /* device [records] in the order of pt_item, or NULL (descriptor 0) */
    const int32_t *long_pts = nullptr; /* device [n_long]: block * point_rows + row */
    int n_long = 0, max_cnt = 0;       /* max_cnt: the longest list, which sizes the long kernel's dynamic LDS */
    ss_map_point *points = nullptr;    /* device [n_blocks][point_rows] */
    uint8_t *point_desc = nullptr;     /* device [n_blocks][point_rows][32] */
    const int32_t *np = nullptr;       /* device [n_blocks] */
    const int32_t *ref_kf = nullptr;   /* device [n_blocks][point_rows] or NULL */
    const uint8_t *select = nullptr;   /* device [n_blocks][point_rows] or NULL */
    const uint8_t *desc = nullptr;     /* device [n_kf][rows_per_frame][32] */
    int rows_per_frame = 0;
    const float *ow = nullptr;         /* device [n_kf][3] */
    const float *scale = nullptr;      /* device [n_levels] */
    int n_levels = 0, geometry = 0, descriptor = 0;
    ss_refresh_info *info = nullptr;       /* device [n_blocks][point_rows] */
    ss_refresh_summary *summary = nullptr; /* device [n_blocks] */
};
int ssk_refresh(hipStream_t s, const ssk_refresh_call &g); /* a hipError_t: the LDS attribute may be refused */
/* ss_place.hip: place recognition (DESIGN.md "Place recognition").  The inverted file of a database: count, scan, fill (one memset
 * and five launches); the queries of a call in six stages, so that the caller can time each (stage 0 .. 5: flags, votes, survivors,
 * scores and the minimum score, groups, candidates; ten launches in all) */
struct ssk_place_lists {
    const int32_t *word = nullptr, *count = nullptr; /* device [n_db][stride], [n_db] */
    int n_db = 0, stride = 0, n_words = 0;
    int32_t *off = nullptr;    /* device [n_words + 1]: the counts, then the lists' starts */
    int32_t *cursor = nullptr; /* device [n_words + 1] */
    int32_t *list = nullptr;   /* device [n_db * stride] */
    int32_t *sums = nullptr;   /* device [ssk_place_scan_sums(n_words)] */
};
size_t ssk_place_scan_sums(int n_words);
int ssk_place_build(hipStream_t s, const ssk_place_lists &b); /* a hipError_t */
struct ssk_place_call {
    ss_place_db db; /* device pointers */
    const int32_t *q_word = nullptr, *q_count = nullptr;
    const double *q_value = nullptr;
    int q_stride = 0, n_q = 0, q_cap = 0, nb_cap = 0, cand_cap = 0;
    const int32_t *q_kf = nullptr, *q_problem = nullptr; /* device [n_q] */
    const int32_t *q_nb = nullptr;                       /* device [n_q][q_cap][2] or NULL */
    const ss_covis_row *q_row = nullptr;
    const int32_t *nb = nullptr; /* device [n_db][nb_cap][2] */
    ss_place_params p = {};
    ss_place_cand *cand = nullptr;
    ss_place_summary *summary = nullptr;
    /* [n_q][n_db] each: the caller's d_words / d_score or the workspace's */
    int32_t *words = nullptr;
    float *score = nullptr;
    uint8_t *flags = nullptr;
    uint32_t *star = nullptr; /* acc* as keys of the total order; 0: none */
    int32_t *surv = nullptr;  /* the survivors, ascending */
    int32_t *state = nullptr; /* [n_q][8] */
};
void ssk_place_query(hipStream_t s, const ssk_place_call &c, int stage);
/* ss_undistort.hip: Frame's keypoint post-processing (DESIGN.md "Undistorted keypoints").  One launch: mvKeysUn of every row below
 * its frame's count.  kp_out == kp: only x and y are written; raw_xy != NULL (the in-place form of a batch, kp_out == kp): the raw
 * pairs are saved there first */
struct ssk_undistort_call {
    int n_frames = 0, rows = 0;
    const ss_keypoint *kp = nullptr;       /* device [n_frames][rows] */
    const int32_t *n_kp = nullptr;         /* device [n_frames] */
    const int32_t *frame_error = nullptr;  /* device [n_frames] or NULL */
    const ss_undist_cam *cams = nullptr;   /* device [n_frames] */
    ss_keypoint *kp_out = nullptr;         /* device [n_frames][rows] */
    float2 *raw_xy = nullptr;              /* device [n_frames][rows] or NULL */
};
void ssk_undistort(hipStream_t s, const ssk_undistort_call &g);
/* Two launches: the summaries' heads, then depth and right coordinate of every row.  raw_xy != NULL: the raw positions are read
 * there instead of kp_raw */
struct ssk_depth_call {
    int n_frames = 0, rows = 0, width = 0, height = 0;
    const uint8_t *depth = nullptr; /* device: n_frames frames of frame_stride bytes, rows of row_stride bytes */
    int64_t row_stride = 0, frame_stride = 0;
    ss_depth_params p = {};
    float inv = 1.0f;         /* ss_depth_inv(p.depth_map_factor) */
    bool scale_float = false; /* ss_depth_scales_float(inv) */
    const ss_keypoint *kp_raw = nullptr, *kp_un = nullptr; /* device [n_frames][rows] */
    const float2 *raw_xy = nullptr;
    const int32_t *n_kp = nullptr, *frame_error = nullptr;
    float *right = nullptr, *depth_out = nullptr; /* device [n_frames][rows] */
    ss_depth_summary *summary = nullptr;          /* device [n_frames] */
};
void ssk_depth(hipStream_t s, const ssk_depth_call &g);
/* ss_unproject.hip: map points from depth (DESIGN.md "Map points from depth").  One launch, one workgroup per frame: the counts, the
 * radix select of the threshold key, then the rows in ascending chunks of SSK_UNPROJECT_CHUNK: state, map point and the ordered
 * compaction.  The depth of row i of frame b is at depth + (depth_src[b] * rows + i) * depth_stride (depth_src NULL: block b); a
 * frame whose depth_src is negative reads no depth and has none */
#define SSK_UNPROJECT_CHUNK 1024
struct ssk_unproject_call {
    int n_frames = 0, rows = 0;
    const ss_keypoint *kp = nullptr;          /* device [n_frames][rows] */
    const uint8_t *desc = nullptr;
    const int32_t *n_kp = nullptr, *frame_error = nullptr;
    const uint8_t *depth = nullptr;
    int64_t depth_stride = 4;
    const int32_t *depth_src = nullptr;       /* device [n_frames] or NULL */
    const uint8_t *has_point = nullptr, *outlier = nullptr; /* device [n_frames][rows] or NULL */
    const ss_unproject_view *views = nullptr; /* device [n_frames] */
    ss_unproject_params p = {};
    int n_levels = 1;
    float scale[SS_MAX_LEVELS] = {};
    ss_unproject_info *info = nullptr;
    ss_map_point *points = nullptr;
    uint8_t *point_desc = nullptr;
    int32_t *point_rows = nullptr;
    int32_t *n_points = nullptr;
    ss_unproject_summary *summary = nullptr;
};
void ssk_unproject(hipStream_t s, const ssk_unproject_call &g);
/* The bookkeeping of SearchBySim3 (the rule: include/sendslam_orb.h).  One workgroup per pair: a base pass over the rows, a barrier,
 * a scatter pass in which every store to one address writes the same value.  marks writes skip1 and skip2; mutual marks the train
 * rows that carry a prior match in taken (workspace, [n_frames][rows]) and writes idx_out and the summary */
struct ssk_sim3_marks_call {
    int n_frames = 0, rows = 0;
    const int32_t *idx = nullptr, *idx12 = nullptr, *idx21 = nullptr;
    const uint8_t *q_skip = nullptr, *t_skip = nullptr;
    const int32_t *nq = nullptr, *nt = nullptr;
    const int32_t *src = nullptr;
    const int32_t *frame_error = nullptr;
    uint8_t *skip1 = nullptr, *skip2 = nullptr, *taken = nullptr;
    int32_t *idx_out = nullptr;
    ss_sim3_mutual_summary *summary = nullptr;
};
void ssk_sim3_marks(hipStream_t s, const ssk_sim3_marks_call &g);
void ssk_sim3_mutual(hipStream_t s, const ssk_sim3_marks_call &g);
/* ss_rectify.hip: bilinear remap through fixed-point maps (DESIGN.md "Rectification").  A map on the device is two arrays of
 * height rows, ssk_rectify_pitch(width) entries apart: xy = (uint16)ix | (uint16)iy << 16 and ab = a | b << 5; the entries past the
 * width are "outside" records.  ssk_rectify_fixed is the host conversion of a float map pair into them.  ssk_rectify remaps the
 * frames of n_groups <= SS_MAX_RECTIFY_MAPS groups, group g = the frames order[first .. first + count) (device int32) that
 * share one map; a source frame's rows must span less than 4 GiB (32-bit tap offsets).  A source whose base, strides and row bytes
 * are multiples of 16 takes the form that stages each tile's source box in LDS, any other the byte gathers. */
struct ssk_rectify_group {
    const uint32_t *xy = nullptr;
    const uint16_t *ab = nullptr;
    int32_t first = 0, count = 0;
};
#define SSK_RECTIFY_ENTRY_BYTES 6
inline int ssk_rectify_pitch(int width) { return (width + 3) & ~3; }
void ssk_rectify_fixed(const float *map_x, const float *map_y, int width, int height, int pitch, uint32_t *xy, uint16_t *ab);
void ssk_rectify(hipStream_t s, const ssk_rectify_group *groups, int n_groups, const int32_t *order, const void *src, int channels,
                 int64_t row_stride, int64_t frame_stride, void *dst, int64_t dst_row_stride, int64_t dst_frame_stride, int w, int h);
/* test hook: run the device std::sort restatement on n <= 2048 items (size << 32 | UL.x << 20 | id) */
int ssk_debug_sort(hipStream_t s, uint64_t *d_items, int n);
#define SSK_MATCH_MFMA_MIN_QUERIES 128 /* from this many query rows on, ssk_match runs a matrix-core kernel */
/* database-streaming form for n_query <= 8 and n_train >= 65536: plan (false = not applicable), the HBM-bound kernel,
 * the merge of its per-chunk partials */
bool ssk_match_stream_plan(int nq, int nt, size_t partial_bytes, int *chunk_len, int *n_chunks);
void ssk_match_stream_kernel(hipStream_t s, const void *query, const void *train, int nq, int nt, int chunk_len, int n_chunks,
                             void *partial);
void ssk_match_stream_merge(hipStream_t s, const void *partial, int nq, int n_chunks, int th, int rnum, int rden, int32_t *idx,
                            uint16_t *d1, uint16_t *d2);
#define SSK_STREAM_PARTIAL_MAX (2048 * 8 * SSK_MATCH_PARTIAL_BYTES)

#endif
