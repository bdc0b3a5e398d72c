/*
 * ss_api_search.cpp -- the search family of the C ABI (include/sendslam_orb.h): guided matching, map-point projection search,
 * map-point fusion, the vocabulary and bag of words, epipolar search and triangulation, the Sim3 RANSAC, the pose-only optimisation, the Sim3 refinement,
 * the local bundle adjustment, the PnP RANSAC, the undistortion of keypoints with the image bounds and the RGB-D depth, the map points from depth.  Each has a pairs form on caller arrays, a batch form on the
 * frames of the last extraction and, for some, a host form.  The context and the helpers they share: ss_ctx.h.
 */
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "ss_ctx.h"
#include <new>

#include "ss_ba_steps.h"
#include "ss_graph_steps.h"
#include "ss_gba_steps.h"
#include "ss_epi_steps.h"
#include "ss_fuse_steps.h"
#include "ss_pnp_steps.h"
#include "ss_pose_steps.h"
#include "ss_proj_steps.h"
#include "ss_refresh_steps.h"
#include "ss_sim3_steps.h"
#include "ss_sim3opt_steps.h"
#include "ss_two_view_steps.h"
#include "ss_undistort_steps.h"
#include "ss_unproject_steps.h"

extern "C" {

/* ---- what the forms share ---- */
/* false, with the error set: a batch form (`entry`) before any extraction */
static bool have_batch(ss_ctx *c, const char *entry)
{
    if (c->have_geom && c->last_n_frames > 0) return true;
    fail(c, SS_ERR_STATE, std::string(entry) + ": no batch has been extracted");
    return false;
}

/* The operands of a batch form with a train table: frame b of the last batch against frame src[b] of it */
struct batch_operands {
    int n_frames = 0, kcap = 0;
    const ss_keypoint *kps = nullptr;
    const uint8_t *desc = nullptr;
    const int32_t *n_kp = nullptr, *src = nullptr, *frame_error = nullptr;
};

/* Fills them once the form (`form`: as its messages name it) has checked its own arguments: the capacity, the train table (checked,
 * then on the device; NULL: frame b against b - 1), the frame errors */
static int batch_operands_of(ss_ctx *c, const std::string &form, const int32_t *train_src, batch_operands &o)
{
    const int n = c->last_n_frames, kcap = c->hg.kcap;
    if (kcap > SS_GUIDED_MAX_ROWS) return fail(c, SS_ERR_INVALID_ARG, form + ": kp_capacity " + std::to_string(kcap) + " exceeds SS_GUIDED_MAX_ROWS");
    for (int b = 0; train_src && b < n; b++)
        if (train_src[b] < -1 || train_src[b] >= n)
            return fail(c, SS_ERR_INVALID_ARG, "train_src[" + std::to_string(b) + "] = " + std::to_string(train_src[b]) + " names no frame of the batch (" +
                                                   std::to_string(n) + "); the " + form + " takes no carry frames");
    const int rc = upload_train_src(c, train_src, n);
    if (rc != SS_OK) return rc;
    o.n_frames = n, o.kcap = kcap;
    o.kps = c->ws.kps, o.desc = c->ws.desc, o.n_kp = c->ws.n_kp, o.src = c->train_src.as<int32_t>();
    return flagged_frame_error(c, c->batch_test_flagged, &o.frame_error);
}

/* a guided call (the BoW match and the epipolar search run on one too) on the frames of the batch, none against itself */
static void batch_sides(ssk_guided_call &g, const batch_operands &o)
{
    g.n_frames = o.n_frames, g.rows = o.kcap;
    g.q_kp = g.t_kp = o.kps, g.q_desc = g.t_desc = o.desc, g.nq = g.nt = o.n_kp;
    g.src = o.src, g.frame_error = o.frame_error;
    g.exclude_same_frame = 1;
}

/* ... and on the caller arrays of a pairs form */
static void pairs_sides(ssk_guided_call &g, int n_frames, int rows_per_frame, const void *d_query, const void *d_query_kp, const void *d_n_query,
                        const void *d_train, const void *d_train_kp, const void *d_n_train)
{
    g.n_frames = n_frames, g.rows = rows_per_frame;
    g.q_kp = (const ss_keypoint *)d_query_kp, g.t_kp = (const ss_keypoint *)d_train_kp;
    g.q_desc = (const uint8_t *)d_query, g.t_desc = (const uint8_t *)d_train;
    g.nq = (const int32_t *)d_n_query, g.nt = (const int32_t *)d_n_train;
}

/* the frame (or pair: `counted`) and row counts of a pairs form; n_frames == 0 passes: the form returns SS_OK on it once its other
 * shape checks are through */
static int pairs_shape(ss_ctx *c, const std::string &form, const char *counted, int n_frames, int rows_per_frame)
{
    if (n_frames < 0 || rows_per_frame < 1) return fail(c, SS_ERR_INVALID_ARG, form + ": bad " + counted + " or row count");
    if (rows_per_frame > SS_GUIDED_MAX_ROWS)
        return fail(c, SS_ERR_INVALID_ARG, form + ": rows_per_frame " + std::to_string(rows_per_frame) + " exceeds SS_GUIDED_MAX_ROWS (" +
                                               std::to_string(SS_GUIDED_MAX_ROWS) + ")");
    return SS_OK;
}

/* the pyramid table of the context into a call (`what` heads the message) */
static int context_pyramid(ss_ctx *c, const std::string &what, int *n_levels, float *scale)
{
    if (c->params.n_levels < 1 || c->params.n_levels > SS_MAX_LEVELS || !(c->params.scale_factor > 1.0f))
        return fail(c, SS_ERR_INVALID_ARG, what + ": the context's n_levels / scale_factor give no pyramid table");
    *n_levels = c->params.n_levels;
    ss_scale_table(c->params.scale_factor, *n_levels, scale);
    return SS_OK;
}

/* a call of one workgroup per frame or pair (`counted`: "frames", "pairs") takes 65535 of them */
static int call_count_ok(ss_ctx *c, const std::string &what, int n, const char *counted)
{
    if (n > 65535) return fail(c, SS_ERR_INVALID_ARG, what + ": more than 65535 " + counted + " in one call");
    return SS_OK;
}

/* the sides of the pairs of a Sim3 call on the caller arrays of a pairs form */
static void pairs_sides(ssk_pair_sides &g, int n_pairs, int rows, const void *d_query_xyz, const void *d_query_kp, const void *d_query_skip,
                        const void *d_n_query, const void *d_train_xyz, const void *d_train_kp, const void *d_train_skip, const void *d_n_train,
                        const void *d_idx)
{
    g.n_frames = n_pairs, g.rows = rows;
    g.q_xyz = (const ss_map_point *)d_query_xyz, g.t_xyz = (const ss_map_point *)d_train_xyz;
    g.q_kp = (const ss_keypoint *)d_query_kp, g.t_kp = (const ss_keypoint *)d_train_kp;
    g.q_skip = (const uint8_t *)d_query_skip, g.t_skip = (const uint8_t *)d_train_skip;
    g.nq = (const int32_t *)d_n_query, g.nt = (const int32_t *)d_n_train;
    g.idx = (const int32_t *)d_idx;
}

/* ... and on the frames of the batch */
static void batch_sides(ssk_pair_sides &g, const batch_operands &o, const void *d_xyz, const void *d_skip, const void *d_idx)
{
    g.n_frames = o.n_frames, g.rows = o.kcap;
    g.q_xyz = g.t_xyz = (const ss_map_point *)d_xyz;
    g.q_kp = g.t_kp = o.kps;
    g.q_skip = g.t_skip = (const uint8_t *)d_skip;
    g.nq = g.nt = o.n_kp;
    g.src = o.src, g.frame_error = o.frame_error;
    g.idx = (const int32_t *)d_idx;
}

/* The views of the pairs of g through the staged table `tab`: views1 then views2, each of n_frames.  A pairs form brings both; a
 * batch form brings the frames' views as views1 and views2 NULL: pair b reads the view of its train frame (train_src NULL: b - 1) */
static int pair_views(ss_ctx *c, staged_table &tab, ssk_pair_sides &g, const ss_proj_view *views1, const ss_proj_view *views2, const int32_t *train_src)
{
    const int n = g.n_frames;
    const size_t vb = (size_t)n * sizeof(ss_proj_view);
    const int rc = staged_upload(c, tab, 2 * vb, [&](uint8_t *h) {
        ss_proj_view *v1 = (ss_proj_view *)h, *v2 = (ss_proj_view *)(h + vb);
        memcpy(v1, views1, vb);
        if (views2) memcpy(v2, views2, vb);
        for (int b = 0; !views2 && b < n; b++) {
            const int t = train_src ? train_src[b] : b - 1; /* checked by batch_operands_of; -1: the pair has no train and reads no view */
            v2[b] = views1[t < 0 ? b : t];
        }
    });
    if (rc != SS_OK) return rc;
    g.views1 = tab.as<ss_proj_view>(), g.views2 = tab.as<ss_proj_view>(vb);
    return SS_OK;
}

static void guided_rule(ssk_guided_call &g, const ss_guided_params *p)
{
    g.th = p->th, g.rnum = p->ratio_num, g.rden = p->ratio_den;
    g.one_to_one = p->one_to_one != 0, g.orientation = p->orientation;
}

/* The index of the train frames of ix on the grid: sizes the grid from the extent, carves the index and the candidate counts
 * ([n_frames][cand_rows]) out of c->d_guided_ws, launches k_guided_index as stage `stage` */
static int grid_index(ss_ctx *c, ssk_guided_call &ix, const char *stage, int extent_w, int extent_h, int cand_rows)
{
    ssk_guided_grid(ix, extent_w, extent_h);
    const size_t frames = (size_t)ix.n_frames;
    const int rc = carve_from(c, c->d_guided_ws, [&](carve &w) {
        ix.cell_start = w.take<uint32_t>(frames * (SSK_GUIDED_MAX_CELLS + 1) * sizeof(uint32_t));
        ix.recs = w.take<void>(frames * ix.rows * 16);
        ix.n_cand = w.take<int32_t>(frames * cand_rows * sizeof(int32_t));
    });
    if (rc != SS_OK) return rc;
    const int64_t nt = (int64_t)ix.n_frames * ix.rows, n_cells = (int64_t)ix.cols * ix.grid_rows;
    /* algorithmic bytes: keypoints in, records and cell offsets out */
    stage_timer t(c, stage, nt * ((int64_t)sizeof(ss_keypoint) + 16) + ix.n_frames * (n_cells + 1) * 4);
    ssk_guided_index(c->stream, ix);
    return SS_OK;
}

/* The index of the train nodes a pairs form brings (BoW match, epipolar search): its two pieces of the workspace being carved, then
 * the launch as stage `stage` */
struct node_index {
    uint64_t *index = nullptr;
    int32_t *n_index = nullptr;
};
static void take_node_index(carve &w, node_index &x, const ssk_guided_call &g)
{
    x.index = w.take<uint64_t>((size_t)g.n_frames * g.rows * sizeof(uint64_t));
    x.n_index = w.take<int32_t>((size_t)g.n_frames * sizeof(int32_t));
}
static void index_train_nodes(ss_ctx *c, const char *stage, const ssk_guided_call &g, const int32_t *t_node, const node_index &x)
{
    stage_timer t(c, stage, (int64_t)g.n_frames * g.rows * 12);
    ssk_bow_index(c->stream, t_node, g.nt, nullptr, g.n_frames, g.rows, x.index, x.n_index);
}

/* One array of a host form: `room` bytes of the form's device buffer, at d once io_send has carved it; `bytes` of it come from
 * `in` before the device call and go to `out` after it (either NULL, or bytes 0: no copy) */
struct io_piece {
    const void *in;
    void *out;
    size_t room, bytes;
    uint8_t *d = nullptr;
};
static int io_send(ss_ctx *c, dev_buf<uint8_t> &buf, io_piece *io, int n)
{
    const int rc = carve_from(c, buf, [&](carve &w) {
        for (int k = 0; k < n; k++) io[k].d = w.take<uint8_t>(io[k].room);
    });
    if (rc != SS_OK) return rc;
    for (int k = 0; k < n; k++)
        if (io[k].in && io[k].bytes) HIP_TRY(c, hipMemcpyAsync(io[k].d, io[k].in, io[k].bytes, hipMemcpyHostToDevice, c->stream));
    return SS_OK;
}
static int io_fetch(ss_ctx *c, const io_piece *io, int n)
{
    for (int k = 0; k < n; k++)
        if (io[k].out && io[k].bytes) HIP_TRY(c, hipMemcpyAsync(io[k].out, io[k].d, io[k].bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SS_OK;
}

/* The host form of one pair (ss_sim3, ss_sim3_opt; `what` heads the messages): the checks, the pair's arrays as one pair of `rows`
 * rows on both sides in the form's device buffer `buf`, the pairs form on those pieces (device(io, rows)), the flags and the
 * result back.  others: what else the form needs is there; extra: one more input of the form (the start), or NULL and 0 bytes */
enum { PP_QX, PP_QK, PP_QS, PP_TX, PP_TK, PP_TS, PP_IDX, PP_N, PP_EXTRA, PP_FLAGS, PP_RES, PP_PIECES };
extern "C++" template <class Device>
static int single_pair(ss_ctx *c, const std::string &what, dev_buf<uint8_t> &buf, const ss_map_point *query_xyz, const ss_keypoint *query_kp,
                       const uint8_t *query_skip, int n_query, const ss_map_point *train_xyz, const ss_keypoint *train_kp, const uint8_t *train_skip,
                       int n_train, const int32_t *idx, bool others, const void *extra, size_t extra_bytes, uint8_t *flags, void *result,
                       size_t result_bytes, Device device)
{
    if (n_query < 0 || n_train < 0 || n_query > SS_GUIDED_MAX_ROWS || n_train > SS_GUIDED_MAX_ROWS)
        return fail(c, SS_ERR_INVALID_ARG, what + ": n_query and n_train must be 0 .. SS_GUIDED_MAX_ROWS");
    if (!others || !result || (n_query > 0 && (!query_xyz || !query_kp || !idx || !flags)) || (n_train > 0 && (!train_xyz || !train_kp)))
        return fail(c, SS_ERR_INVALID_ARG, what + ": NULL buffer");
    /* `counts` is on this stack: no return before the stream has read it */
    const size_t rows = (size_t)std::max(std::max(n_query, n_train), 1), nq = (size_t)n_query, nt = (size_t)n_train;
    const size_t kp = sizeof(ss_keypoint), mp = sizeof(ss_map_point);
    const int32_t counts[2] = {n_query, n_train};
    io_piece io[PP_PIECES] = {{query_xyz, nullptr, rows * mp, nq * mp}, {query_kp, nullptr, rows * kp, nq * kp}, {query_skip, nullptr, rows, nq},
                              {train_xyz, nullptr, rows * mp, nt * mp}, {train_kp, nullptr, rows * kp, nt * kp}, {train_skip, nullptr, rows, nt},
                              {idx, nullptr, rows * 4, nq * 4}, {counts, nullptr, sizeof(counts), sizeof(counts)}, {extra, nullptr, extra_bytes, extra_bytes},
                              {nullptr, flags, rows, nq}, {nullptr, result, result_bytes, result_bytes}};
    int rc = io_send(c, buf, io, PP_PIECES);
    if (!query_skip) io[PP_QS].d = nullptr; /* the pairs form takes NULL for "no flags" */
    if (!train_skip) io[PP_TS].d = nullptr;
    if (rc == SS_OK) rc = device(io, (int)rows);
    if (rc != SS_OK) {
        (void)hipStreamSynchronize(c->stream);
        return rc;
    }
    return io_fetch(c, io, PP_PIECES);
}

/* ---- guided matching (csrc/ss_guided.hip) ---- */
static int guided_check_params(ss_ctx *c, const ss_guided_params *p)
{
    if (!p) return fail(c, SS_ERR_INVALID_ARG, "guided match: params is NULL");
    if (p->ratio_num < 0 || p->ratio_num > 32767 || p->ratio_den < 0 || p->ratio_den > 32767)
        return fail(c, SS_ERR_INVALID_ARG, "guided match: ratio_num and ratio_den must be 0 .. 32767 (ratio_den 0 = no ratio test)");
    if (p->orientation < 0 || p->orientation > 2) return fail(c, SS_ERR_INVALID_ARG, "guided match: orientation must be 0, 1 or 2");
    return SS_OK;
}

/* The three launches of a call whose operands, windows and outputs are filled in */
static int guided_run(ss_ctx *c, ssk_guided_call &g, const ss_guided_params *p, int extent_w, int extent_h)
{
    guided_rule(g, p);
    const int rc = grid_index(c, g, "guided_index", extent_w, extent_h, g.rows);
    if (rc != SS_OK) return rc;
    const int64_t nq = (int64_t)g.n_frames * g.rows;
    {
        /* per query: its window (or keypoint), its descriptor, the 12 bytes it writes; the records and descriptors it visits depend
         * on the content and are not counted */
        stage_timer t(c, "guided_search", nq * ((g.windows ? 16 : (int64_t)sizeof(ss_keypoint)) + SS_DESC_BYTES + 12));
        ssk_guided_search(c->stream, g);
    }
    {
        /* idx read and written, d1, the candidate count; the two angles of a surviving match on top when orientation is on */
        stage_timer t(c, "guided_finish", nq * (8 + 2 + 4 + (g.orientation ? 8 : 0)) + g.n_frames * (int64_t)sizeof(ss_guided_summary));
        ssk_guided_finish(c->stream, g);
    }
    HIP_TRY(c, hipGetLastError());
    return SS_OK;
}

int ss_match_guided_pairs_device(ss_ctx *c, const void *d_query, const void *d_query_kp, const void *d_n_query, const void *d_train,
                                 const void *d_train_kp, const void *d_n_train, const void *d_windows, int n_frames, int rows_per_frame,
                                 const ss_guided_params *p, void *d_idx, void *d_d1, void *d_d2, void *d_summary)
{
    if (!c) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    int rc = guided_check_params(c, p);
    if (rc != SS_OK) return rc;
    rc = pairs_shape(c, "guided match", "frame", n_frames, rows_per_frame);
    if (rc != SS_OK) return rc;
    if (p->extent_w <= 0 || p->extent_h <= 0) return fail(c, SS_ERR_INVALID_ARG, "guided match: extent_w and extent_h must be > 0");
    if (n_frames == 0) return SS_OK;
    if (!d_query || !d_query_kp || !d_n_query || !d_train || !d_train_kp || !d_n_train || !d_windows || !d_idx || !d_d1 || !d_d2 || !d_summary)
        return fail(c, SS_ERR_INVALID_ARG, "guided match: NULL buffer");
    ssk_guided_call g;
    pairs_sides(g, n_frames, rows_per_frame, d_query, d_query_kp, d_n_query, d_train, d_train_kp, d_n_train);
    g.windows = (const ss_guided_window *)d_windows;
    g.idx = (int32_t *)d_idx, g.d1 = (uint16_t *)d_d1, g.d2 = (uint16_t *)d_d2;
    g.summary = (ss_guided_summary *)d_summary;
    return guided_run(c, g, p, p->extent_w, p->extent_h);
}

int ss_match_guided_batch_device(ss_ctx *c, const int32_t *train_src, const void *d_windows, const ss_guided_params *p, void *d_idx,
                                 void *d_d1, void *d_d2, void *d_summary)
{
    if (!c) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    if (!have_batch(c, "ss_match_guided_batch_device")) return SS_ERR_STATE;
    int rc = guided_check_params(c, p);
    if (rc != SS_OK) return rc;
    if (!d_idx || !d_d1 || !d_d2 || !d_summary) return fail(c, SS_ERR_INVALID_ARG, "guided match: NULL output buffer");
    batch_operands o;
    rc = batch_operands_of(c, "guided match", train_src, o);
    if (rc != SS_OK) return rc;
    ssk_guided_call g;
    batch_sides(g, o);
    g.windows = (const ss_guided_window *)d_windows;
    g.dg = c->ws.dg;
    g.radius = p->radius, g.radius_by_octave = p->radius_by_octave != 0, g.octave_span = p->octave_span;
    g.idx = (int32_t *)d_idx, g.d1 = (uint16_t *)d_d1, g.d2 = (uint16_t *)d_d2;
    g.summary = (ss_guided_summary *)d_summary;
    return guided_run(c, g, p, c->hg.w, c->hg.h);
}

int ss_match_guided(ss_ctx *c, const uint8_t *query, const ss_keypoint *query_kp, int n_query, const uint8_t *train,
                    const ss_keypoint *train_kp, int n_train, const ss_guided_window *windows, const ss_guided_params *p, int32_t *idx,
                    uint16_t *d1, uint16_t *d2, ss_guided_summary *summary)
{
    if (!c) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    if (n_query < 0 || n_train < 0 || n_query > SS_GUIDED_MAX_ROWS || n_train > SS_GUIDED_MAX_ROWS)
        return fail(c, SS_ERR_INVALID_ARG, "guided match: n_query and n_train must be 0 .. SS_GUIDED_MAX_ROWS");
    if ((n_query > 0 && (!query || !query_kp || !windows || !idx || !d1 || !d2)) || (n_train > 0 && (!train || !train_kp)) || !summary)
        return fail(c, SS_ERR_INVALID_ARG, "guided match: NULL buffer");
    /* one frame of `rows` rows on both sides; `counts` is on this stack: no return before the stream has read it */
    const size_t rows = (size_t)std::max(std::max(n_query, n_train), 1), nq = (size_t)n_query, nt = (size_t)n_train, kp = sizeof(ss_keypoint);
    const int32_t counts[2] = {n_query, n_train};
    enum { QD, TD, QK, TK, WIN, N, IDX, D1, D2, SUM, PIECES };
    io_piece io[PIECES] = {{query, nullptr, rows * 32, nq * 32}, {train, nullptr, rows * 32, nt * 32}, {query_kp, nullptr, rows * kp, nq * kp},
                           {train_kp, nullptr, rows * kp, nt * kp}, {windows, nullptr, rows * sizeof(ss_guided_window), nq * sizeof(ss_guided_window)},
                           {counts, nullptr, sizeof(counts), sizeof(counts)}, {nullptr, idx, rows * 4, nq * 4}, {nullptr, d1, rows * 2, nq * 2},
                           {nullptr, d2, rows * 2, nq * 2}, {nullptr, summary, sizeof(ss_guided_summary), sizeof(ss_guided_summary)}};
    int rc = io_send(c, c->d_guided_io, io, PIECES);
    if (rc == SS_OK)
        rc = ss_match_guided_pairs_device(c, io[QD].d, io[QK].d, io[N].d, io[TD].d, io[TK].d, io[N].d + 4, io[WIN].d, 1, (int)rows, p, io[IDX].d, io[D1].d,
                                          io[D2].d, io[SUM].d);
    if (rc != SS_OK) {
        (void)hipStreamSynchronize(c->stream);
        return rc;
    }
    return io_fetch(c, io, PIECES);
}

/* ---- map-point projection search (csrc/ss_proj.hip, csrc/ss_proj_steps.h) ---- */
/* the message of the first rule p breaks, or NULL; needs no context */
static const char *proj_params_error(const ss_proj_params *p)
{
    if (!p) return "projection search: params is NULL";
    if (!(p->th > 0.0f) || !std::isfinite(p->th)) return "projection search: th must be finite and > 0";
    if (p->view_cos_limit != p->view_cos_limit) return "projection search: view_cos_limit is NaN";
    if (p->th_high < 0 || p->th_high > 256) return "projection search: th_high must be 0 .. 256";
    if (p->ratio_num < 0 || p->ratio_num > 32767 || p->ratio_den < 0 || p->ratio_den > 32767)
        return "projection search: ratio_num and ratio_den must be 0 .. 32767 (ratio_den 0 = no ratio test)";
    return nullptr;
}

int ss_proj_view_init(const ss_camera *cam, const double rcw[9], const double tcw[3], float bf, ss_proj_view *out)
{
    if (!cam || !rcw || !tcw || !out) return SS_ERR_INVALID_ARG;
    for (int k = 0; k < 9; k++) out->rcw[k] = (float)rcw[k];
    for (int k = 0; k < 3; k++) {
        out->tcw[k] = (float)tcw[k];
        out->ow[k] = (float)-((rcw[k] * tcw[0] + rcw[3 + k] * tcw[1]) + rcw[6 + k] * tcw[2]);
    }
    out->fx = (float)cam->fx, out->fy = (float)cam->fy, out->cx = (float)cam->cx, out->cy = (float)cam->cy;
    out->bf = bf;
    out->min_x = 0.0f, out->max_x = (float)cam->width;
    out->min_y = 0.0f, out->max_y = (float)cam->height;
    return SS_OK;
}

int ss_proj_points_host(const ss_proj_view *view, const ss_proj_params *p, const float *scale, int n_levels, const ss_map_point *points,
                        int n, ss_proj_point *out)
{
    if (proj_params_error(p)) return SS_ERR_INVALID_ARG;
    if (!view || !scale || n_levels < 1 || n_levels > SS_MAX_LEVELS || n < 0 || (n > 0 && (!points || !out))) return SS_ERR_INVALID_ARG;
    for (int i = 0; i < n; i++) out[i] = ss_proj_eval(*view, points[i], p->view_cos_limit, p->th, p->far_limit, scale, n_levels);
    return SS_OK;
}

/* What a call of blocks of points searched by frames needs before its search is launched, for the projection search and fusion
 * (Call is ssk_proj_call or ssk_fuse_call; `what` heads the messages): the checks the device forms share, the pyramid table, the
 * staged table of views and block numbers, and the index of the train frames (k_guided_index on a guided call over the same arrays,
 * timed as `index_stage`).  `buffers` says that no operand or output the call needs is NULL.  A call of no frames returns SS_OK and
 * launches nothing: the caller returns with it */
extern "C++" template <class Call>
static int points_call_prepare(ss_ctx *c, Call &g, const std::string &what, const char *index_stage, int n_blocks, const ss_proj_view *views,
                               const int32_t *point_src, bool buffers, bool check_right, int extent_w, int extent_h)
{
    if (g.n_frames < 0 || n_blocks < 0 || g.point_rows < 1 || g.rows < 1) return fail(c, SS_ERR_INVALID_ARG, what + ": bad frame, block or row count");
    if (g.point_rows > SS_GUIDED_MAX_ROWS || g.rows > SS_GUIDED_MAX_ROWS)
        return fail(c, SS_ERR_INVALID_ARG, what + ": point_rows " + std::to_string(g.point_rows) + " / rows_per_frame " + std::to_string(g.rows) +
                                               " exceed SS_GUIDED_MAX_ROWS (" + std::to_string(SS_GUIDED_MAX_ROWS) + ")");
    if (extent_w <= 0 || extent_h <= 0) return fail(c, SS_ERR_INVALID_ARG, what + ": extent_w and extent_h must be > 0");
    int rc = context_pyramid(c, what, &g.n_levels, g.scale);
    if (rc != SS_OK) return rc;
    if (g.n_frames == 0) return SS_OK;
    if (!views) return fail(c, SS_ERR_INVALID_ARG, what + ": views is NULL");
    for (int b = 0; b < g.n_frames; b++) {
        const int pb = point_src ? point_src[b] : b;
        if (pb < 0 || pb >= n_blocks)
            return fail(c, SS_ERR_INVALID_ARG, std::string(point_src ? "point_src[" : "frame [") + std::to_string(b) + "] = " + std::to_string(pb) +
                                                   " names no block of points (" + std::to_string(n_blocks) + ")");
    }
    if (!buffers || !g.points || !g.p_desc || !g.np || !g.t_kp || !g.t_desc || !g.nt || !g.idx || !g.d1 || !g.summary)
        return fail(c, SS_ERR_INVALID_ARG, what + ": NULL buffer");
    if (check_right && !g.t_right) return fail(c, SS_ERR_INVALID_ARG, what + ": check_right needs the right coordinates of the train rows");
    g.check_right = check_right;
    /* the host tables of the call: n_frames views, then n_frames block numbers (point_src NULL: 0, 1, ...) */
    const size_t views_bytes = (size_t)g.n_frames * sizeof(ss_proj_view);
    rc = staged_upload(c, c->proj_tab, views_bytes + (size_t)g.n_frames * sizeof(int32_t), [&](uint8_t *h) {
        memcpy(h, views, views_bytes);
        int32_t *src = (int32_t *)(h + views_bytes);
        for (int b = 0; b < g.n_frames; b++) src[b] = point_src ? point_src[b] : b;
    });
    if (rc != SS_OK) return rc;
    g.views = c->proj_tab.as<ss_proj_view>();
    g.src = c->proj_tab.as<int32_t>(views_bytes);
    ssk_guided_call ix; /* the index alone: train keypoints, counts, errors, grid, workspace */
    ix.n_frames = g.n_frames;
    ix.rows = g.rows;
    ix.t_kp = g.t_kp;
    ix.nt = g.nt;
    ix.frame_error = g.frame_error;
    rc = grid_index(c, ix, index_stage, extent_w, extent_h, g.point_rows);
    if (rc != SS_OK) return rc;
    g.shift = ix.shift, g.cols = ix.cols, g.x_max = ix.x_max, g.y_max = ix.y_max;
    g.cell_start = ix.cell_start, g.recs = ix.recs, g.n_cand = ix.n_cand;
    return SS_OK;
}

/* The three launches of a call whose device operands and outputs are filled in: the index of the train frames, the search, the
 * finish */
static int proj_run(ss_ctx *c, ssk_proj_call &g, int n_blocks, const ss_proj_view *views, const int32_t *point_src, const ss_proj_params *p,
                    int extent_w, int extent_h)
{
    if (const char *msg = proj_params_error(p)) return fail(c, SS_ERR_INVALID_ARG, msg);
    const int rc = points_call_prepare(c, g, "projection search", "proj_index", n_blocks, views, point_src, g.d2 && g.proj, p->check_right != 0, extent_w,
                                       extent_h);
    if (rc != SS_OK || g.n_frames == 0) return rc;
    g.view_cos_limit = p->view_cos_limit, g.th = p->th, g.far_limit = p->far_limit;
    g.th_high = p->th_high, g.rnum = p->ratio_num, g.rden = p->ratio_den;
    g.one_to_one = p->one_to_one != 0;
    const int64_t np = (int64_t)g.n_frames * g.point_rows;
    {
        /* per point: the point, its descriptor, the 44 bytes it writes; the records and descriptors it visits depend on the content */
        stage_timer t(c, "proj_search", np * ((int64_t)sizeof(ss_map_point) + SS_DESC_BYTES + 12 + (int64_t)sizeof(ss_proj_point)));
        ssk_proj_search(c->stream, g);
    }
    {
        stage_timer t(c, "proj_finish", np * (8 + 2 + 4 + 4) + g.n_frames * (int64_t)sizeof(ss_proj_summary));
        ssk_proj_finish(c->stream, g);
    }
    HIP_TRY(c, hipGetLastError());
    return SS_OK;
}

static void proj_outputs(ssk_proj_call &g, void *d_idx, void *d_d1, void *d_d2, void *d_proj, void *d_summary)
{
    g.idx = (int32_t *)d_idx, g.d1 = (uint16_t *)d_d1, g.d2 = (uint16_t *)d_d2;
    g.proj = (ss_proj_point *)d_proj;
    g.summary = (ss_proj_summary *)d_summary;
}

int ss_match_proj_pairs_device(ss_ctx *c, const void *d_points, const void *d_point_desc, const void *d_n_points, int n_blocks, int point_rows,
                               const void *d_train, const void *d_train_kp, const void *d_n_train, const void *d_train_right,
                               const void *d_train_taken, int n_frames, int rows_per_frame, const ss_proj_view *views, const int32_t *point_src,
                               const ss_proj_params *p, void *d_idx, void *d_d1, void *d_d2, void *d_proj, void *d_summary)
{
    if (!c) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    ssk_proj_call g;
    g.n_frames = n_frames;
    g.point_rows = point_rows;
    g.rows = rows_per_frame;
    g.points = (const ss_map_point *)d_points, g.p_desc = (const uint8_t *)d_point_desc, g.np = (const int32_t *)d_n_points;
    g.t_kp = (const ss_keypoint *)d_train_kp, g.t_desc = (const uint8_t *)d_train, g.nt = (const int32_t *)d_n_train;
    g.t_right = (const float *)d_train_right, g.t_taken = (const uint8_t *)d_train_taken;
    proj_outputs(g, d_idx, d_d1, d_d2, d_proj, d_summary);
    return proj_run(c, g, n_blocks, views, point_src, p, p ? p->extent_w : 1, p ? p->extent_h : 1);
}

int ss_match_proj_batch_device(ss_ctx *c, const void *d_points, const void *d_point_desc, const void *d_n_points, int n_blocks, int point_rows,
                               const void *d_train_right, const void *d_train_taken, const ss_proj_view *views, const int32_t *point_src,
                               const ss_proj_params *p, void *d_idx, void *d_d1, void *d_d2, void *d_proj, void *d_summary)
{
    if (!c) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    if (!have_batch(c, "ss_match_proj_batch_device")) return SS_ERR_STATE;
    ssk_proj_call g;
    g.n_frames = c->last_n_frames;
    g.point_rows = point_rows;
    g.rows = c->hg.kcap;
    g.points = (const ss_map_point *)d_points, g.p_desc = (const uint8_t *)d_point_desc, g.np = (const int32_t *)d_n_points;
    g.t_kp = c->ws.kps, g.t_desc = c->ws.desc, g.nt = c->ws.n_kp;
    const int rc = flagged_frame_error(c, c->batch_test_flagged, &g.frame_error);
    if (rc != SS_OK) return rc;
    g.t_right = (const float *)d_train_right, g.t_taken = (const uint8_t *)d_train_taken;
    proj_outputs(g, d_idx, d_d1, d_d2, d_proj, d_summary);
    return proj_run(c, g, n_blocks, views, point_src, p, c->hg.w, c->hg.h);
}

int ss_match_proj(ss_ctx *c, const ss_proj_view *view, const ss_map_point *points, const uint8_t *point_desc, int n_points, const uint8_t *train,
                  const ss_keypoint *train_kp, int n_train, const float *train_right, const uint8_t *train_taken, const ss_proj_params *p,
                  int32_t *idx, uint16_t *d1, uint16_t *d2, ss_proj_point *proj, ss_proj_summary *summary)
{
    if (!c) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    if (n_points < 0 || n_train < 0 || n_points > SS_GUIDED_MAX_ROWS || n_train > SS_GUIDED_MAX_ROWS)
        return fail(c, SS_ERR_INVALID_ARG, "projection search: n_points and n_train must be 0 .. SS_GUIDED_MAX_ROWS");
    if (!view || (n_points > 0 && (!points || !point_desc || !idx || !d1 || !d2)) || (n_train > 0 && (!train || !train_kp)) || !summary)
        return fail(c, SS_ERR_INVALID_ARG, "projection search: NULL buffer");
    /* one block of `pr` points, one train frame of `tr` rows; `counts` is on this stack: no return before the stream has read it */
    const size_t pr = (size_t)std::max(n_points, 1), tr = (size_t)std::max(n_train, 1), np = (size_t)n_points, nt = (size_t)n_train;
    const size_t kp = sizeof(ss_keypoint), mp = sizeof(ss_map_point), pp = sizeof(ss_proj_point);
    const int32_t counts[2] = {n_points, n_train};
    enum { PT, PD, TD, TK, TR, TT, N, IDX, D1, D2, PJ, SUM, PIECES };
    io_piece io[PIECES] = {{points, nullptr, pr * mp, np * mp}, {point_desc, nullptr, pr * 32, np * 32}, {train, nullptr, tr * 32, nt * 32},
                           {train_kp, nullptr, tr * kp, nt * kp}, {train_right, nullptr, tr * 4, nt * 4}, {train_taken, nullptr, tr, nt},
                           {counts, nullptr, sizeof(counts), sizeof(counts)}, {nullptr, idx, pr * 4, np * 4}, {nullptr, d1, pr * 2, np * 2},
                           {nullptr, d2, pr * 2, np * 2}, {nullptr, proj, pr * pp, np * pp},
                           {nullptr, summary, sizeof(ss_proj_summary), sizeof(ss_proj_summary)}};
    int rc = io_send(c, c->d_proj_io, io, PIECES);
    /* a side without rows has no array to pass: its count is 0 and nothing of it is read */
    if (rc == SS_OK)
        rc = ss_match_proj_pairs_device(c, io[PT].d, io[PD].d, io[N].d, 1, (int)pr, io[TD].d, io[TK].d, io[N].d + 4,
                                        (train_right || n_train == 0) ? io[TR].d : nullptr, train_taken ? io[TT].d : nullptr, 1, (int)tr, view, nullptr, p,
                                        io[IDX].d, io[D1].d, io[D2].d, io[PJ].d, io[SUM].d);
    if (rc != SS_OK) {
        (void)hipStreamSynchronize(c->stream);
        return rc;
    }
    return io_fetch(c, io, PIECES);
}

/* ---- map-point fusion (csrc/ss_fuse.hip, csrc/ss_fuse_steps.h) ---- */
/* the message of the first rule p breaks, or NULL; needs no context */
static const char *fuse_params_error(const ss_fuse_params *p)
{
    if (!p) return "fusion: params is NULL";
    if (!(p->th > 0.0f) || !std::isfinite(p->th)) return "fusion: th must be finite and > 0";
    if (p->view_cos_limit != p->view_cos_limit) return "fusion: view_cos_limit is NaN";
    if (p->th_low < 0 || p->th_low > 256) return "fusion: th_low must be 0 .. 256";
    if (p->chi2_mono > 0.0f && p->check_right && (!(p->chi2_stereo > 0.0f) || !std::isfinite(p->chi2_stereo)))
        return "fusion: chi2_stereo must be finite and > 0 when chi2_mono > 0 and check_right is set";
    if (p->reserved[0] != 0 || p->reserved[1] != 0) return "fusion: the reserved fields must be 0";
    return nullptr;
}

int ss_fuse_view_sim3(const ss_camera *cam, const double srcw[9], const double t[3], float bf, ss_proj_view *out)
{
    if (!cam || !srcw || !t || !out) return SS_ERR_INVALID_ARG;
    const double s = sqrt((srcw[0] * srcw[0] + srcw[1] * srcw[1]) + srcw[2] * srcw[2]);
    if (!(s > 0.0) || !std::isfinite(s)) return SS_ERR_INVALID_ARG;
    double r[9], tc[3];
    for (int k = 0; k < 9; k++) r[k] = srcw[k] / s;
    for (int k = 0; k < 3; k++) tc[k] = t[k] / s;
    return ss_proj_view_init(cam, r, tc, bf, out);
}

int ss_fuse_points_host(const ss_proj_view *view, const ss_fuse_params *p, const float *scale, int n_levels, const ss_map_point *points,
                        const uint8_t *skip, int n, ss_fuse_point *out)
{
    if (fuse_params_error(p)) return SS_ERR_INVALID_ARG;
    if (!view || !scale || n_levels < 1 || n_levels > SS_MAX_LEVELS || n < 0 || (n > 0 && (!points || !out))) return SS_ERR_INVALID_ARG;
    for (int i = 0; i < n; i++) out[i] = ss_fuse_eval(*view, points[i], skip ? skip[i] : 0, p->view_cos_limit, p->th, scale, n_levels);
    return SS_OK;
}

int ss_fuse_check_host(const ss_fuse_params *p, const float *scale, int n_levels, const ss_fuse_point *points, const ss_keypoint *kp,
                       const float *right, const uint8_t *taken, int n, uint8_t *out)
{
    if (fuse_params_error(p)) return SS_ERR_INVALID_ARG;
    if (!scale || n_levels < 1 || n_levels > SS_MAX_LEVELS || n < 0 || (n > 0 && (!points || !kp || !out))) return SS_ERR_INVALID_ARG;
    for (int k = 0; k < n; k++) {
        float s_lo, s_hi;
        ss_fuse_scales(scale, n_levels, points[k].level, &s_lo, &s_hi);
        out[k] = (uint8_t)ss_fuse_check(points[k], s_lo, s_hi, kp[k].x, kp[k].y, kp[k].octave, k, taken, right, p->chi2_mono, p->chi2_stereo,
                                        p->check_right != 0);
    }
    return SS_OK;
}

/* The three launches of a fusion call, as proj_run.  The host tables go through the projection search's staged table and the index
 * through guided matching's workspace: all of it is on the context's one stream */
static int fuse_run(ss_ctx *c, ssk_fuse_call &g, int n_blocks, const ss_proj_view *views, const int32_t *point_src, const ss_fuse_params *p,
                    int extent_w, int extent_h)
{
    if (const char *msg = fuse_params_error(p)) return fail(c, SS_ERR_INVALID_ARG, msg);
    const int rc = points_call_prepare(c, g, "fusion", "fuse_index", n_blocks, views, point_src, g.fuse && g.point, p->check_right != 0, extent_w, extent_h);
    if (rc != SS_OK || g.n_frames == 0) return rc;
    g.view_cos_limit = p->view_cos_limit, g.th = p->th;
    g.chi2_mono = p->chi2_mono, g.chi2_stereo = p->chi2_stereo;
    g.th_low = p->th_low;
    const int64_t np = (int64_t)g.n_frames * g.point_rows;
    {
        /* per point: the point, its descriptor, its flag, the 42 bytes it writes; the records and descriptors it visits depend on the
         * content */
        stage_timer t(c, "fuse_search", np * ((int64_t)sizeof(ss_map_point) + SS_DESC_BYTES + (g.p_skip ? 1 : 0) + 10 + (int64_t)sizeof(ss_fuse_point)));
        ssk_fuse_search(c->stream, g);
    }
    {
        /* idx, d1, the candidate count and the state read, the action written; the id of a named row on top */
        stage_timer t(c, "fuse_finish", np * (4 + 2 + 4 + 4 + 8 + (g.t_point ? 4 : 0)) + g.n_frames * (int64_t)sizeof(ss_fuse_summary));
        ssk_fuse_finish(c->stream, g);
    }
    HIP_TRY(c, hipGetLastError());
    return SS_OK;
}

static void fuse_outputs(ssk_fuse_call &g, void *d_idx, void *d_d1, void *d_fuse, void *d_point, void *d_summary)
{
    g.idx = (int32_t *)d_idx, g.d1 = (uint16_t *)d_d1;
    g.fuse = (ss_fuse_action *)d_fuse;
    g.point = (ss_fuse_point *)d_point;
    g.summary = (ss_fuse_summary *)d_summary;
}

int ss_match_fuse_pairs_device(ss_ctx *c, const void *d_points, const void *d_point_desc, const void *d_n_points, int n_blocks, int point_rows,
                               const void *d_point_skip, const void *d_train, const void *d_train_kp, const void *d_n_train,
                               const void *d_train_right, const void *d_train_taken, const void *d_train_point, int n_frames, int rows_per_frame,
                               const ss_proj_view *views, const int32_t *point_src, const ss_fuse_params *p, void *d_idx, void *d_d1, void *d_fuse,
                               void *d_point, void *d_summary)
{
    if (!c) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    ssk_fuse_call g;
    g.n_frames = n_frames;
    g.point_rows = point_rows;
    g.rows = rows_per_frame;
    g.points = (const ss_map_point *)d_points, g.p_desc = (const uint8_t *)d_point_desc, g.np = (const int32_t *)d_n_points;
    g.p_skip = (const uint8_t *)d_point_skip;
    g.t_kp = (const ss_keypoint *)d_train_kp, g.t_desc = (const uint8_t *)d_train, g.nt = (const int32_t *)d_n_train;
    g.t_right = (const float *)d_train_right, g.t_taken = (const uint8_t *)d_train_taken, g.t_point = (const int32_t *)d_train_point;
    fuse_outputs(g, d_idx, d_d1, d_fuse, d_point, d_summary);
    return fuse_run(c, g, n_blocks, views, point_src, p, p ? p->extent_w : 1, p ? p->extent_h : 1);
}

int ss_match_fuse_batch_device(ss_ctx *c, const void *d_points, const void *d_point_desc, const void *d_n_points, int n_blocks, int point_rows,
                               const void *d_point_skip, const void *d_train_right, const void *d_train_taken, const void *d_train_point,
                               const ss_proj_view *views, const int32_t *point_src, const ss_fuse_params *p, void *d_idx, void *d_d1, void *d_fuse,
                               void *d_point, void *d_summary)
{
    if (!c) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    if (!have_batch(c, "ss_match_fuse_batch_device")) return SS_ERR_STATE;
    ssk_fuse_call g;
    g.n_frames = c->last_n_frames;
    g.point_rows = point_rows;
    g.rows = c->hg.kcap;
    g.points = (const ss_map_point *)d_points, g.p_desc = (const uint8_t *)d_point_desc, g.np = (const int32_t *)d_n_points;
    g.p_skip = (const uint8_t *)d_point_skip;
    g.t_kp = c->ws.kps, g.t_desc = c->ws.desc, g.nt = c->ws.n_kp;
    const int rc = flagged_frame_error(c, c->batch_test_flagged, &g.frame_error);
    if (rc != SS_OK) return rc;
    g.t_right = (const float *)d_train_right, g.t_taken = (const uint8_t *)d_train_taken, g.t_point = (const int32_t *)d_train_point;
    fuse_outputs(g, d_idx, d_d1, d_fuse, d_point, d_summary);
    return fuse_run(c, g, n_blocks, views, point_src, p, c->hg.w, c->hg.h);
}

int ss_match_fuse(ss_ctx *c, const ss_proj_view *view, const ss_map_point *points, const uint8_t *point_desc, const uint8_t *point_skip, int n_points,
                  const uint8_t *train, const ss_keypoint *train_kp, int n_train, const float *train_right, const uint8_t *train_taken,
                  const int32_t *train_point, const ss_fuse_params *p, int32_t *idx, uint16_t *d1, ss_fuse_action *fuse, ss_fuse_point *point,
                  ss_fuse_summary *summary)
{
    if (!c) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    if (n_points < 0 || n_train < 0 || n_points > SS_GUIDED_MAX_ROWS || n_train > SS_GUIDED_MAX_ROWS)
        return fail(c, SS_ERR_INVALID_ARG, "fusion: n_points and n_train must be 0 .. SS_GUIDED_MAX_ROWS");
    if (!view || (n_points > 0 && (!points || !point_desc || !idx || !d1 || !fuse)) || (n_train > 0 && (!train || !train_kp)) || !summary)
        return fail(c, SS_ERR_INVALID_ARG, "fusion: NULL buffer");
    /* one block of `pr` points, one train frame of `tr` rows; `counts` is on this stack: no return before the stream has read it */
    const size_t pr = (size_t)std::max(n_points, 1), tr = (size_t)std::max(n_train, 1), np = (size_t)n_points, nt = (size_t)n_train;
    const size_t kp = sizeof(ss_keypoint), mp = sizeof(ss_map_point), fp = sizeof(ss_fuse_point), fa = sizeof(ss_fuse_action);
    const int32_t counts[2] = {n_points, n_train};
    enum { PT, PD, PS, TD, TK, TR, TT, TP, N, IDX, D1, FU, FP, SUM, PIECES };
    io_piece io[PIECES] = {{points, nullptr, pr * mp, np * mp}, {point_desc, nullptr, pr * 32, np * 32}, {point_skip, nullptr, pr, np},
                           {train, nullptr, tr * 32, nt * 32}, {train_kp, nullptr, tr * kp, nt * kp}, {train_right, nullptr, tr * 4, nt * 4},
                           {train_taken, nullptr, tr, nt}, {train_point, nullptr, tr * 4, nt * 4}, {counts, nullptr, sizeof(counts), sizeof(counts)},
                           {nullptr, idx, pr * 4, np * 4}, {nullptr, d1, pr * 2, np * 2}, {nullptr, fuse, pr * fa, np * fa},
                           {nullptr, point, pr * fp, np * fp}, {nullptr, summary, sizeof(ss_fuse_summary), sizeof(ss_fuse_summary)}};
    int rc = io_send(c, c->d_proj_io, io, PIECES);
    /* a side without rows has no array to pass: its count is 0 and nothing of it is read */
    if (rc == SS_OK)
        rc = ss_match_fuse_pairs_device(c, io[PT].d, io[PD].d, io[N].d, 1, (int)pr, point_skip ? io[PS].d : nullptr, io[TD].d, io[TK].d, io[N].d + 4,
                                        (train_right || n_train == 0) ? io[TR].d : nullptr, train_taken ? io[TT].d : nullptr,
                                        train_point ? io[TP].d : nullptr, 1, (int)tr, view, nullptr, p, io[IDX].d, io[D1].d, io[FU].d, io[FP].d,
                                        io[SUM].d);
    if (rc != SS_OK) {
        (void)hipStreamSynchronize(c->stream);
        return rc;
    }
    return io_fetch(c, io, PIECES);
}

/* ---- bag of words (csrc/ss_bow.hip) ---- */
/* The vocabulary tree on the host, indexed by the file's node ids (0 = the root).  parent < own id for every node, so the children
 * of a node in file order are its children in ascending id: children[child_pos[p] .. child_pos[p] + n_child[p]). */
struct ss_vocab {
    int k = 0, L = 0, n_nodes = 0, n_words = 0, max_depth = 0;
    std::vector<int32_t> parent, n_child, child_pos, children, word, depth;
    std::vector<double> weight;
    std::vector<uint8_t> leaf, desc;
};

static int voc_fail(char *err, int err_bytes, const std::string &msg)
{
    if (err && err_bytes > 0) snprintf(err, (size_t)err_bytes, "%s", msg.c_str());
    return SS_ERR_INVALID_ARG;
}

/* checks and links a tree whose parent / leaf / desc / weight arrays are filled for the ids 1 .. n */
static int voc_link(ss_vocab &v, char *err, int err_bytes)
{
    const int n = v.n_nodes;
    if (v.k < 1 || v.k > SS_VOCAB_MAX_K) return voc_fail(err, err_bytes, "vocabulary: k " + std::to_string(v.k) + " is outside 1 .. SS_VOCAB_MAX_K");
    if (v.L < 1 || v.L > SS_VOCAB_MAX_DEPTH) return voc_fail(err, err_bytes, "vocabulary: L " + std::to_string(v.L) + " is outside 1 .. SS_VOCAB_MAX_DEPTH");
    if (n < 1) return voc_fail(err, err_bytes, "vocabulary: no nodes");
    if (n >= SS_VOCAB_MAX_NODES) return voc_fail(err, err_bytes, "vocabulary: more than SS_VOCAB_MAX_NODES nodes");
    v.n_child.assign((size_t)n + 1, 0);
    v.depth.assign((size_t)n + 1, 0);
    v.word.assign((size_t)n + 1, -1);
    v.leaf[0] = 0;
    v.parent[0] = -1;
    v.weight[0] = 0.0;
    for (int id = 1; id <= n; id++) {
        const int p = v.parent[id];
        if (p < 0 || p >= id) return voc_fail(err, err_bytes, "vocabulary: node " + std::to_string(id) + " names parent " + std::to_string(p) + ", which is no earlier node");
        if (v.leaf[p]) return voc_fail(err, err_bytes, "vocabulary: leaf " + std::to_string(p) + " has a child (node " + std::to_string(id) + ")");
        if (++v.n_child[p] > v.k) return voc_fail(err, err_bytes, "vocabulary: node " + std::to_string(p) + " has more than k = " + std::to_string(v.k) + " children");
        v.depth[id] = v.depth[p] + 1;
        if (v.depth[id] > SS_VOCAB_MAX_DEPTH) return voc_fail(err, err_bytes, "vocabulary: node " + std::to_string(id) + " is deeper than SS_VOCAB_MAX_DEPTH");
    }
    v.n_words = v.max_depth = 0;
    for (int id = 1; id <= n; id++) {
        if (v.leaf[id]) {
            v.word[id] = v.n_words++;
            v.max_depth = std::max(v.max_depth, (int)v.depth[id]);
        } else {
            if (v.n_child[id] == 0) return voc_fail(err, err_bytes, "vocabulary: inner node " + std::to_string(id) + " has no children");
            v.weight[id] = 0.0;
        }
    }
    v.child_pos.assign((size_t)n + 2, 0);
    for (int id = 0; id <= n; id++) v.child_pos[id + 1] = v.child_pos[id] + v.n_child[id];
    v.children.assign((size_t)n, 0);
    std::vector<int32_t> fill(v.child_pos.begin(), v.child_pos.end() - 1);
    for (int id = 1; id <= n; id++) v.children[fill[v.parent[id]]++] = id;
    return SS_OK;
}

static void voc_reserve(ss_vocab &v, size_t n)
{
    v.parent.assign(n + 1, 0);
    v.leaf.assign(n + 1, 0);
    v.weight.assign(n + 1, 0.0);
    v.desc.assign((n + 1) * 32, 0);
}

int ss_vocab_from_arrays(int n_nodes, const int32_t *parent, const uint8_t *is_leaf, const uint8_t *desc, const double *weight, int k, int L,
                         ss_vocab **out, char *err, int err_bytes)
{
    if (!out) return voc_fail(err, err_bytes, "vocabulary: out is NULL");
    *out = nullptr;
    if (n_nodes < 1) return voc_fail(err, err_bytes, "vocabulary: no nodes");
    if (n_nodes >= SS_VOCAB_MAX_NODES) return voc_fail(err, err_bytes, "vocabulary: more than SS_VOCAB_MAX_NODES nodes");
    if (!parent || !is_leaf || !desc || !weight) return voc_fail(err, err_bytes, "vocabulary: NULL array");
    ss_vocab *v = new (std::nothrow) ss_vocab;
    if (!v) return SS_ERR_NO_MEMORY;
    v->k = k, v->L = L, v->n_nodes = n_nodes;
    voc_reserve(*v, (size_t)n_nodes);
    for (int i = 0; i < n_nodes; i++) {
        v->parent[i + 1] = parent[i];
        v->leaf[i + 1] = is_leaf[i] != 0;
        v->weight[i + 1] = weight[i];
    }
    memcpy(v->desc.data() + 32, desc, (size_t)n_nodes * 32);
    const int rc = voc_link(*v, err, err_bytes);
    if (rc != SS_OK) {
        delete v;
        return rc;
    }
    *out = v;
    return SS_OK;
}

/* the next blank-separated token of [p, end), or false */
static bool voc_token(const char *&p, const char *end, const char *&tok, size_t &len)
{
    while (p < end && (*p == ' ' || *p == '\t' || *p == '\r')) p++;
    if (p >= end) return false;
    tok = p;
    while (p < end && *p != ' ' && *p != '\t' && *p != '\r') p++;
    len = (size_t)(p - tok);
    return true;
}

/* a decimal integer of at most 9 digits with an optional minus sign, nothing else */
static bool voc_int(const char *tok, size_t len, long &out)
{
    size_t i = 0;
    const bool neg = len > 0 && tok[0] == '-';
    if (neg) i = 1;
    if (i >= len || len - i > 9) return false;
    long v = 0;
    for (; i < len; i++) {
        if (tok[i] < '0' || tok[i] > '9') return false;
        v = v * 10 + (tok[i] - '0');
    }
    out = neg ? -v : v;
    return true;
}

/* a decimal floating-point literal (digits, sign, point, exponent), correctly rounded by strtod */
static bool voc_double(const char *tok, size_t len, double &out)
{
    char buf[64];
    if (len == 0 || len >= sizeof(buf)) return false;
    bool digit = false;
    for (size_t i = 0; i < len; i++) {
        const char ch = tok[i];
        if (ch >= '0' && ch <= '9') digit = true;
        else if (ch != '+' && ch != '-' && ch != '.' && ch != 'e' && ch != 'E') return false;
        buf[i] = ch;
    }
    buf[len] = 0;
    if (!digit) return false;
    char *stop = nullptr;
    out = strtod(buf, &stop);
    return stop == buf + len;
}

int ss_vocab_load_text(const char *path, ss_vocab **out, char *err, int err_bytes)
{
    if (!out) return voc_fail(err, err_bytes, "vocabulary: out is NULL");
    *out = nullptr;
    if (!path) return voc_fail(err, err_bytes, "vocabulary: path is NULL");
    std::string text;
    {
        std::ifstream in(path, std::ios::binary);
        if (!in) return voc_fail(err, err_bytes, std::string("vocabulary: cannot open ") + path);
        std::ostringstream ss;
        ss << in.rdbuf();
        text = ss.str();
    }
    ss_vocab *v = new (std::nothrow) ss_vocab;
    if (!v) return SS_ERR_NO_MEMORY;
    auto bad = [&](long line, const std::string &what) {
        delete v;
        return voc_fail(err, err_bytes, "vocabulary: line " + std::to_string(line) + ": " + what);
    };
    const char *p = text.data(), *const end = p + text.size();
    long line = 0, nodes = 0;
    bool header = false;
    while (p < end) {
        const char *le = (const char *)memchr(p, '\n', (size_t)(end - p));
        if (!le) le = end;
        const char *q = p, *tok = nullptr;
        size_t len = 0;
        p = le < end ? le + 1 : end;
        line++;
        if (!voc_token(q, le, tok, len)) continue; /* a blank line */
        long val[36];
        const int want = header ? 34 : 4; /* integers of the line; a node line ends with the weight */
        int got = 0;
        bool more = false; /* a token behind the integers: tok */
        do {
            if (got == want) {
                more = true;
                break;
            }
            if (!voc_int(tok, len, val[got])) return bad(line, "token " + std::to_string(got + 1) + " is no integer");
            got++;
        } while (voc_token(q, le, tok, len));
        if (got < want || (header && !more)) return bad(line, "truncated: " + std::to_string(got) + " of " + std::to_string(want + (header ? 1 : 0)) + " tokens");
        if (!header) {
            if (more) return bad(line, "more than 4 tokens in the header");
            if (val[2] != 0 || val[3] != 0) return bad(line, "only scoring 0 (L1) with weighting 0 (TF-IDF) is supported");
            v->k = (int)std::min(std::max(val[0], -1L), (long)SS_VOCAB_MAX_K + 1);
            v->L = (int)std::min(std::max(val[1], -1L), (long)SS_VOCAB_MAX_DEPTH + 1);
            header = true;
            /* at most one node per 70 bytes of text: sizes the arrays once */
            voc_reserve(*v, std::min(text.size() / 70 + 16, (size_t)SS_VOCAB_MAX_NODES));
            continue;
        }
        /* tok is the 35th token: the weight */
        double w = 0;
        if (!voc_double(tok, len, w)) return bad(line, "the weight is no number");
        if (voc_token(q, le, tok, len)) return bad(line, "more than 35 tokens");
        if (val[1] != 0 && val[1] != 1) return bad(line, "is_leaf must be 0 or 1");
        const size_t id = (size_t)++nodes;
        if (id >= (size_t)SS_VOCAB_MAX_NODES) return bad(line, "more than SS_VOCAB_MAX_NODES nodes");
        if (id >= v->parent.size()) {
            const size_t cap = v->parent.size() * 2;
            v->parent.resize(cap), v->leaf.resize(cap), v->weight.resize(cap), v->desc.resize(cap * 32);
        }
        for (int b = 0; b < 32; b++) {
            if (val[2 + b] < 0 || val[2 + b] > 255) return bad(line, "descriptor byte " + std::to_string(b) + " is outside 0 .. 255");
            v->desc[id * 32 + b] = (uint8_t)val[2 + b];
        }
        v->parent[id] = (int32_t)std::min(std::max(val[0], -1L), (long)SS_VOCAB_MAX_NODES);
        v->leaf[id] = (uint8_t)val[1];
        v->weight[id] = w;
    }
    if (!header) return bad(line, "no header line");
    v->n_nodes = (int)nodes;
    const int rc = voc_link(*v, err, err_bytes);
    if (rc != SS_OK) {
        delete v;
        return rc;
    }
    *out = v;
    return SS_OK;
}

int ss_vocab_info(const ss_vocab *v, ss_vocab_shape *out)
{
    if (!v || !out) return SS_ERR_INVALID_ARG;
    out->k = v->k, out->L = v->L, out->n_nodes = v->n_nodes, out->n_words = v->n_words, out->max_depth = v->max_depth;
    return SS_OK;
}

int ss_vocab_copy_out(const ss_vocab *v, int32_t *first_child, int32_t *n_children, int32_t *word, double *weight, int32_t *depth)
{
    if (!v) return SS_ERR_INVALID_ARG;
    for (int id = 0; id <= v->n_nodes; id++) {
        if (first_child) first_child[id] = v->n_child[id] ? v->children[v->child_pos[id]] : -1;
        if (n_children) n_children[id] = v->n_child[id];
        if (word) word[id] = v->word[id];
        if (weight) weight[id] = v->weight[id];
        if (depth) depth[id] = v->depth[id];
    }
    return SS_OK;
}

int ss_vocab_destroy(ss_vocab *v)
{
    if (!v) return SS_ERR_INVALID_ARG;
    delete v;
    return SS_OK;
}

int ss_bow_set_vocabulary(ss_ctx *c, const ss_vocab *v)
{
    if (!c) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    if (!v) return fail(c, SS_ERR_INVALID_ARG, "ss_bow_set_vocabulary: voc is NULL");
    /* breadth first: the children of the node at position u take the next n_child positions, in file order */
    const size_t n = (size_t)v->n_nodes + 1;
    std::vector<int32_t> at(n); /* position -> file id */
    std::vector<ssk_bow_node> recs(n);
    std::vector<uint8_t> rows(n * 32);
    std::vector<double> wgt((size_t)v->n_words);
    size_t next = 1;
    at[0] = 0;
    for (size_t u = 0; u < n; u++) {
        const int id = at[u];
        ssk_bow_node &r = recs[u];
        r.child_base = v->n_child[id] ? (int32_t)next : 0;
        r.n_child = v->n_child[id];
        r.word = v->word[id];
        r.file_id = id;
        memcpy(&rows[u * 32], &v->desc[(size_t)id * 32], 32);
        if (r.word >= 0) wgt[(size_t)r.word] = v->weight[id];
        for (int ch = 0; ch < v->n_child[id]; ch++) at[next++] = v->children[v->child_pos[id] + ch];
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->voc = ssk_bow_voc();
    c->bow_frames = 0;
    dev_free(c->d_voc);
    uint8_t *d_rows;
    ssk_bow_node *d_recs;
    double *d_wgt;
    const int rc = carve_from(c, c->d_voc, [&](carve &w) {
        d_rows = w.take<uint8_t>(n * 32);
        d_recs = w.take<ssk_bow_node>(n * sizeof(ssk_bow_node));
        d_wgt = w.take<double>(wgt.size() * sizeof(double) + 8);
    });
    if (rc != SS_OK) return rc;
    HIP_TRY(c, hipMemcpy(d_rows, rows.data(), rows.size(), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(d_recs, recs.data(), recs.size() * sizeof(ssk_bow_node), hipMemcpyHostToDevice));
    if (!wgt.empty()) HIP_TRY(c, hipMemcpy(d_wgt, wgt.data(), wgt.size() * sizeof(double), hipMemcpyHostToDevice));
    c->voc.rows = d_rows;
    c->voc.recs = d_recs;
    c->voc.weight = d_wgt;
    c->voc.L = v->L;
    c->voc.max_depth = v->max_depth;
    c->voc.n_words = v->n_words;
    return SS_OK;
}

/* the two launches of a transform whose arrays are filled in */
static int bow_transform_run(ss_ctx *c, ssk_bow_call &b)
{
    const int64_t nr = (int64_t)b.n_frames * b.rows;
    {
        /* per row: its descriptor and the two ids it writes; the children it visits depend on the tree */
        stage_timer t(c, "bow_descend", nr * (SS_DESC_BYTES + 8));
        ssk_bow_descend(c->stream, c->voc, b);
    }
    {
        /* word and node read (the node twice), the vector and the index written */
        stage_timer t(c, "bow_vector", nr * (12 + 12 + (b.index ? 8 : 0)) + b.n_frames * (int64_t)sizeof(ss_bow_summary));
        ssk_bow_vector(c->stream, c->voc, b);
    }
    HIP_TRY(c, hipGetLastError());
    return SS_OK;
}

int ss_bow_transform_device(ss_ctx *c, const void *d_desc, const void *d_n_rows, int n_frames, int rows_per_frame, int levelsup, void *d_word,
                            void *d_node, void *d_bow_word, void *d_bow_value, void *d_summary)
{
    if (!c) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    if (!c->voc.rows) return fail(c, SS_ERR_STATE, "ss_bow_transform_device: no vocabulary (ss_bow_set_vocabulary)");
    if (n_frames < 0 || rows_per_frame < 1 || levelsup < 0) return fail(c, SS_ERR_INVALID_ARG, "bow transform: bad frame count, row count or levelsup");
    if (rows_per_frame > SS_BOW_MAX_ROWS)
        return fail(c, SS_ERR_INVALID_ARG, "bow transform: rows_per_frame " + std::to_string(rows_per_frame) + " exceeds SS_BOW_MAX_ROWS (" +
                                               std::to_string(SS_BOW_MAX_ROWS) + ")");
    if (n_frames == 0) return SS_OK;
    if (!d_desc || !d_n_rows || !d_word || !d_node || !d_bow_word || !d_bow_value || !d_summary) return fail(c, SS_ERR_INVALID_ARG, "bow transform: NULL buffer");
    ssk_bow_call b;
    b.n_frames = n_frames, b.rows = rows_per_frame, b.levelsup = levelsup;
    b.desc = (const uint8_t *)d_desc, b.n_rows = (const int32_t *)d_n_rows;
    b.word = (int32_t *)d_word, b.node = (int32_t *)d_node;
    b.bow_word = (int32_t *)d_bow_word, b.bow_value = (double *)d_bow_value, b.summary = (ss_bow_summary *)d_summary;
    return bow_transform_run(c, b);
}

/* what a batch transform keeps: [index][nodes][index counts] of n frames of kcap rows; p NULL: only the total */
struct bow_keep {
    uint64_t *index;
    int32_t *node, *n_index;
    size_t total;
};
static bow_keep bow_keep_of(uint8_t *p, int n, int kcap)
{
    carve w(p);
    bow_keep k;
    k.index = w.take<uint64_t>((size_t)n * kcap * sizeof(uint64_t));
    k.node = w.take<int32_t>((size_t)n * kcap * sizeof(int32_t));
    k.n_index = w.take<int32_t>((size_t)n * sizeof(int32_t));
    k.total = w.total();
    return k;
}

int ss_bow_transform_batch_device(ss_ctx *c, int levelsup, void *d_word, void *d_node, void *d_bow_word, void *d_bow_value, void *d_summary)
{
    if (!c) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    if (!c->voc.rows) return fail(c, SS_ERR_STATE, "ss_bow_transform_batch_device: no vocabulary (ss_bow_set_vocabulary)");
    if (!have_batch(c, "ss_bow_transform_batch_device")) return SS_ERR_STATE;
    if (levelsup < 0) return fail(c, SS_ERR_INVALID_ARG, "bow transform: levelsup must be >= 0");
    if (!d_word || !d_node || !d_bow_word || !d_bow_value || !d_summary) return fail(c, SS_ERR_INVALID_ARG, "bow transform: NULL output buffer");
    const int n = c->last_n_frames, kcap = c->hg.kcap;
    if (kcap > SS_BOW_MAX_ROWS) return fail(c, SS_ERR_INVALID_ARG, "bow transform: kp_capacity " + std::to_string(kcap) + " exceeds SS_BOW_MAX_ROWS");
    c->bow_frames = 0;
    const int rc = grow(c, c->d_bow_keep, bow_keep_of(nullptr, n, kcap).total);
    if (rc != SS_OK) return rc;
    const bow_keep keep = bow_keep_of(c->d_bow_keep.p, n, kcap);
    ssk_bow_call b;
    b.n_frames = n, b.rows = kcap, b.levelsup = levelsup;
    b.desc = c->ws.desc, b.n_rows = c->ws.n_kp;
    const int rc1 = flagged_frame_error(c, c->batch_test_flagged, &b.frame_error);
    if (rc1 != SS_OK) return rc1;
    b.word = (int32_t *)d_word, b.node = (int32_t *)d_node, b.node2 = keep.node;
    b.bow_word = (int32_t *)d_bow_word, b.bow_value = (double *)d_bow_value, b.summary = (ss_bow_summary *)d_summary;
    b.index = keep.index, b.n_index = keep.n_index;
    const int rc2 = bow_transform_run(c, b);
    if (rc2 == SS_OK) c->bow_frames = n;
    return rc2;
}

/* The launches of a BoW match whose operands, query nodes and outputs are filled in: the index of the train nodes where the call
 * brings its own (t_node != NULL), the search, then guided matching's finish as it is. */
static int bow_match_run(ss_ctx *c, ssk_guided_call &g, const ss_guided_params *p, const int32_t *q_node, const int32_t *t_node, const uint64_t *index,
                         const int32_t *n_index)
{
    guided_rule(g, p);
    const size_t nr = (size_t)g.n_frames * g.rows;
    node_index own;
    const int rc = carve_from(c, c->d_bow_ws, [&](carve &w) {
        g.n_cand = w.take<int32_t>(nr * sizeof(int32_t));
        if (t_node) take_node_index(w, own, g);
    });
    if (rc != SS_OK) return rc;
    if (t_node) {
        index_train_nodes(c, "bow_index", g, t_node, own);
        index = own.index, n_index = own.n_index;
    }
    {
        /* per query: its node, its descriptor, the 12 bytes it writes; the keys and descriptors of its run depend on the content */
        stage_timer t(c, "bow_search", (int64_t)nr * (4 + SS_DESC_BYTES + 12));
        ssk_bow_search(c->stream, g, q_node, index, n_index);
    }
    {
        stage_timer t(c, "bow_finish", (int64_t)nr * (8 + 2 + 4 + (g.orientation ? 8 : 0)) + g.n_frames * (int64_t)sizeof(ss_guided_summary));
        ssk_guided_finish(c->stream, g);
    }
    HIP_TRY(c, hipGetLastError());
    return SS_OK;
}

int ss_match_bow_pairs_device(ss_ctx *c, const void *d_query, const void *d_query_kp, const void *d_query_node, const void *d_n_query,
                              const void *d_train, const void *d_train_kp, const void *d_train_node, const void *d_n_train, int n_frames,
                              int rows_per_frame, const ss_guided_params *p, void *d_idx, void *d_d1, void *d_d2, void *d_summary)
{
    if (!c) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    int rc = guided_check_params(c, p);
    if (rc != SS_OK) return rc;
    rc = pairs_shape(c, "bow match", "frame", n_frames, rows_per_frame);
    if (rc != SS_OK) return rc;
    if (n_frames == 0) return SS_OK;
    if (!d_query || !d_query_kp || !d_query_node || !d_n_query || !d_train || !d_train_kp || !d_train_node || !d_n_train || !d_idx || !d_d1 || !d_d2 ||
        !d_summary)
        return fail(c, SS_ERR_INVALID_ARG, "bow match: NULL buffer");
    ssk_guided_call g;
    pairs_sides(g, n_frames, rows_per_frame, d_query, d_query_kp, d_n_query, d_train, d_train_kp, d_n_train);
    g.idx = (int32_t *)d_idx, g.d1 = (uint16_t *)d_d1, g.d2 = (uint16_t *)d_d2;
    g.summary = (ss_guided_summary *)d_summary;
    return bow_match_run(c, g, p, (const int32_t *)d_query_node, (const int32_t *)d_train_node, nullptr, nullptr);
}

int ss_match_bow_batch_device(ss_ctx *c, const int32_t *train_src, const ss_guided_params *p, void *d_idx, void *d_d1, void *d_d2, void *d_summary)
{
    if (!c) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    if (!have_batch(c, "ss_match_bow_batch_device")) return SS_ERR_STATE;
    if (c->bow_frames != c->last_n_frames)
        return fail(c, SS_ERR_STATE, "ss_match_bow_batch_device: the last batch has not been through ss_bow_transform_batch_device");
    int rc = guided_check_params(c, p);
    if (rc != SS_OK) return rc;
    if (!d_idx || !d_d1 || !d_d2 || !d_summary) return fail(c, SS_ERR_INVALID_ARG, "bow match: NULL output buffer");
    batch_operands o;
    rc = batch_operands_of(c, "bow match", train_src, o);
    if (rc != SS_OK) return rc;
    const bow_keep keep = bow_keep_of(c->d_bow_keep.p, o.n_frames, o.kcap);
    ssk_guided_call g;
    batch_sides(g, o);
    g.idx = (int32_t *)d_idx, g.d1 = (uint16_t *)d_d1, g.d2 = (uint16_t *)d_d2;
    g.summary = (ss_guided_summary *)d_summary;
    return bow_match_run(c, g, p, keep.node, nullptr, keep.index, keep.n_index);
}

int ss_bow_score_device(ss_ctx *c, const void *d_q_word, const void *d_q_value, const void *d_q_count, int q_rows, const void *d_db_word,
                        const void *d_db_value, const void *d_db_count, int n_db, int stride, void *d_score)
{
    if (!c) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    if (n_db < 0 || stride < 1 || q_rows < 1) return fail(c, SS_ERR_INVALID_ARG, "bow score: bad vector count, stride or query size");
    if (n_db == 0) return SS_OK;
    if (!d_q_word || !d_q_value || !d_q_count || !d_db_word || !d_db_value || !d_db_count || !d_score) return fail(c, SS_ERR_INVALID_ARG, "bow score: NULL buffer");
    {
        /* the allocation of every vector is an upper bound of what is read */
        stage_timer t(c, "bow_score", (int64_t)n_db * ((int64_t)stride * 12 + 12) + (int64_t)q_rows * 12);
        ssk_bow_score(c->stream, (const int32_t *)d_q_word, (const double *)d_q_value, (const int32_t *)d_q_count, q_rows, (const int32_t *)d_db_word,
                      (const double *)d_db_value, (const int32_t *)d_db_count, n_db, stride, (double *)d_score);
    }
    HIP_TRY(c, hipGetLastError());
    return SS_OK;
}

/* ---- epipolar search and triangulation (csrc/ss_epi.hip, csrc/ss_epi_steps.h) ---- */
int ss_epi_pair_init(const ss_camera *cam1, const double rcw1[9], const double tcw1[3], const ss_camera *cam2, const double rcw2[9],
                     const double tcw2[3], ss_epi_pair *out)
{
    if (!cam1 || !rcw1 || !tcw1 || !cam2 || !rcw2 || !tcw2 || !out) return SS_ERR_INVALID_ARG;
    ss_epi_pair &w = *out;
    for (int k = 0; k < 9; k++) w.rcw1[k] = rcw1[k], w.rcw2[k] = rcw2[k];
    for (int k = 0; k < 3; k++) {
        w.tcw1[k] = tcw1[k], w.tcw2[k] = tcw2[k];
        w.ow1[k] = -((rcw1[k] * tcw1[0] + rcw1[3 + k] * tcw1[1]) + rcw1[6 + k] * tcw1[2]);
        w.ow2[k] = -((rcw2[k] * tcw2[0] + rcw2[3 + k] * tcw2[1]) + rcw2[6 + k] * tcw2[2]);
    }
    w.fx1 = cam1->fx, w.fy1 = cam1->fy, w.cx1 = cam1->cx, w.cy1 = cam1->cy, w.invfx1 = 1.0 / cam1->fx, w.invfy1 = 1.0 / cam1->fy;
    w.fx2 = cam2->fx, w.fy2 = cam2->fy, w.cx2 = cam2->cx, w.cy2 = cam2->cy, w.invfx2 = 1.0 / cam2->fx, w.invfy2 = 1.0 / cam2->fy;
    const double *R1 = w.rcw1, *R2 = w.rcw2, *t1 = w.tcw1, *t2 = w.tcw2;
    double R12[3][3], t12[3], E[3][3], G[3][3], F[3][3];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) R12[i][j] = (R1[3 * i] * R2[3 * j] + R1[3 * i + 1] * R2[3 * j + 1]) + R1[3 * i + 2] * R2[3 * j + 2];
    for (int i = 0; i < 3; i++) t12[i] = t1[i] - ((R12[i][0] * t2[0] + R12[i][1] * t2[1]) + R12[i][2] * t2[2]);
    for (int j = 0; j < 3; j++) {
        E[0][j] = t12[1] * R12[2][j] - t12[2] * R12[1][j];
        E[1][j] = t12[2] * R12[0][j] - t12[0] * R12[2][j];
        E[2][j] = t12[0] * R12[1][j] - t12[1] * R12[0][j];
    }
    for (int j = 0; j < 3; j++) {
        G[0][j] = w.invfx1 * E[0][j];
        G[1][j] = w.invfy1 * E[1][j];
        G[2][j] = E[2][j] - (w.cx1 * G[0][j] + w.cy1 * G[1][j]);
    }
    double m = 0.0;
    bool finite = true;
    for (int i = 0; i < 3; i++) {
        F[i][0] = G[i][0] * w.invfx2;
        F[i][1] = G[i][1] * w.invfy2;
        F[i][2] = G[i][2] - (F[i][0] * w.cx2 + F[i][1] * w.cy2);
        for (int j = 0; j < 3; j++) {
            const double v = fabs(F[i][j]);
            if (!(v <= 1.7976931348623157e308)) finite = false;
            else if (v > m) m = v;
        }
    }
    const bool usable = finite && m > 0.0;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) w.f12[3 * i + j] = usable ? (float)(F[i][j] / m) : 0.0f;
    double C2[3];
    for (int i = 0; i < 3; i++) C2[i] = ((R2[3 * i] * w.ow1[0] + R2[3 * i + 1] * w.ow1[1]) + R2[3 * i + 2] * w.ow1[2]) + t2[i];
    const float ex = (float)((w.fx2 * C2[0]) / C2[2] + w.cx2), ey = (float)((w.fy2 * C2[1]) / C2[2] + w.cy2);
    w.epipole_test = (std::isfinite(ex) && std::isfinite(ey)) ? 1 : 0;
    w.ex = w.epipole_test ? ex : 0.0f;
    w.ey = w.epipole_test ? ey : 0.0f;
    return SS_OK;
}

/* the message of the first rule p breaks, or NULL; needs no context */
static const char *epi_params_error(const ss_epi_params *p)
{
    if (!p) return "epipolar search: params is NULL";
    if (p->th < 0 || p->th > 256) return "epipolar search: th must be 0 .. 256";
    if (p->orientation < 0 || p->orientation > 2) return "epipolar search: orientation must be 0, 1 or 2";
    return nullptr;
}

int ss_epi_check_host(const ss_epi_pair *pair, const ss_epi_params *p, const float *scale, int n_levels, const ss_keypoint *kp1,
                      const ss_keypoint *kp2, int n, uint8_t *out)
{
    if (epi_params_error(p)) return SS_ERR_INVALID_ARG;
    if (!pair || !scale || n_levels < 1 || n_levels > SS_MAX_LEVELS || n < 0 || (n > 0 && (!kp1 || !kp2 || !out))) return SS_ERR_INVALID_ARG;
    for (int k = 0; k < n; k++) {
        const ss_epi_line line = ss_epi_line_of(pair->f12, kp1[k].x, kp1[k].y);
        out[k] = (uint8_t)ss_epi_check(pair->ex, pair->ey, pair->epipole_test, p->coarse != 0, line, scale, n_levels, kp2[k].x, kp2[k].y, kp2[k].octave);
    }
    return SS_OK;
}

int ss_triangulate_host(const ss_epi_pair *pair, const ss_tri_params *tp, const float *scale, int n_levels, const ss_keypoint *kp1,
                        const ss_keypoint *kp2, int n, ss_map_point *points, ss_tri_info *info)
{
    if (!pair || !tp || !scale || n_levels < 1 || n_levels > SS_MAX_LEVELS || n < 0 || (n > 0 && (!kp1 || !kp2 || !points || !info))) return SS_ERR_INVALID_ARG;
    for (int k = 0; k < n; k++) {
        const ss_tri_out r = ss_tri_eval(*pair, *tp, scale, n_levels, kp1[k].x, kp1[k].y, kp1[k].octave, kp2[k].x, kp2[k].y, kp2[k].octave);
        points[k] = r.point;
        info[k] = r.info;
    }
    return SS_OK;
}

/* The host pairs of a call -> c->epi_tab, which the search and the triangulation share */
static int upload_epi_pairs(ss_ctx *c, const ss_epi_pair *pairs, int n)
{
    const size_t bytes = (size_t)n * sizeof(ss_epi_pair);
    return staged_upload(c, c->epi_tab, bytes, [&](uint8_t *h) { memcpy(h, pairs, bytes); });
}

/* The launches of a search whose operands, counts and outputs are filled in: the index of the train nodes where the call brings its
 * own (t_node != NULL), the search, guided matching's finish as it is (its summaries go to the workspace), the summaries */
static int epi_match_run(ss_ctx *c, ssk_guided_call &g, ssk_epi_call &e, const ss_epi_pair *pairs, const ss_epi_params *p, const int32_t *t_node)
{
    g.th = p->th, g.rnum = 0, g.rden = 0;
    g.one_to_one = p->one_to_one != 0, g.orientation = p->orientation;
    e.coarse = p->coarse != 0;
    int rc = context_pyramid(c, "epipolar search", &e.n_levels, e.scale);
    if (rc != SS_OK) return rc;
    const size_t nr = (size_t)g.n_frames * g.rows;
    node_index own;
    rc = carve_from(c, c->d_epi_ws, [&](carve &w) {
        g.n_cand = w.take<int32_t>(nr * sizeof(int32_t));
        e.n_geo = w.take<int32_t>(nr * sizeof(int32_t));
        e.n_near = w.take<int32_t>(nr * sizeof(int32_t));
        g.summary = w.take<ss_guided_summary>((size_t)g.n_frames * sizeof(ss_guided_summary));
        if (t_node) take_node_index(w, own, g);
    });
    if (rc != SS_OK) return rc;
    rc = upload_epi_pairs(c, pairs, g.n_frames);
    if (rc != SS_OK) return rc;
    e.pairs = c->epi_tab.as<ss_epi_pair>();
    if (t_node) {
        index_train_nodes(c, "epi_index", g, t_node, own);
        e.index = own.index, e.n_index = own.n_index;
    }
    {
        /* per query: its node, keypoint and descriptor, the 18 bytes it writes; what it visits of its run depends on the content */
        stage_timer t(c, "epi_search", (int64_t)nr * (4 + (int64_t)sizeof(ss_keypoint) + SS_DESC_BYTES + 18));
        ssk_epi_search(c->stream, g, e);
    }
    {
        stage_timer t(c, "epi_finish", (int64_t)nr * (8 + 2 + 4 + 8 + (g.orientation ? 8 : 0)) + g.n_frames * (int64_t)(sizeof(ss_guided_summary) + sizeof(ss_epi_summary)));
        ssk_guided_finish(c->stream, g);
        ssk_epi_summary(c->stream, g, e);
    }
    HIP_TRY(c, hipGetLastError());
    return SS_OK;
}

int ss_match_epi_pairs_device(ss_ctx *c, const void *d_query, const void *d_query_kp, const void *d_query_node, const void *d_query_taken,
                              const void *d_n_query, const void *d_train, const void *d_train_kp, const void *d_train_node,
                              const void *d_train_taken, const void *d_n_train, int n_frames, int rows_per_frame, const ss_epi_pair *pairs,
                              const ss_epi_params *p, void *d_idx, void *d_d1, void *d_summary)
{
    if (!c) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    if (const char *msg = epi_params_error(p)) return fail(c, SS_ERR_INVALID_ARG, msg);
    const int rc = pairs_shape(c, "epipolar search", "pair", n_frames, rows_per_frame);
    if (rc != SS_OK) return rc;
    if (n_frames == 0) return SS_OK;
    if (!d_query || !d_query_kp || !d_query_node || !d_n_query || !d_train || !d_train_kp || !d_train_node || !d_n_train || !pairs || !d_idx || !d_d1 ||
        !d_summary)
        return fail(c, SS_ERR_INVALID_ARG, "epipolar search: NULL buffer");
    ssk_guided_call g;
    pairs_sides(g, n_frames, rows_per_frame, d_query, d_query_kp, d_n_query, d_train, d_train_kp, d_n_train);
    g.idx = (int32_t *)d_idx, g.d1 = (uint16_t *)d_d1;
    ssk_epi_call e;
    e.q_node = (const int32_t *)d_query_node;
    e.q_taken = (const uint8_t *)d_query_taken, e.t_taken = (const uint8_t *)d_train_taken;
    e.summary = (ss_epi_summary *)d_summary;
    return epi_match_run(c, g, e, pairs, p, (const int32_t *)d_train_node);
}

int ss_match_epi_batch_device(ss_ctx *c, const int32_t *train_src, const void *d_taken, const ss_epi_pair *pairs, const ss_epi_params *p,
                              void *d_idx, void *d_d1, void *d_summary)
{
    if (!c) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    if (!have_batch(c, "ss_match_epi_batch_device")) return SS_ERR_STATE;
    if (c->bow_frames != c->last_n_frames)
        return fail(c, SS_ERR_STATE, "ss_match_epi_batch_device: the last batch has not been through ss_bow_transform_batch_device");
    if (const char *msg = epi_params_error(p)) return fail(c, SS_ERR_INVALID_ARG, msg);
    if (!pairs || !d_idx || !d_d1 || !d_summary) return fail(c, SS_ERR_INVALID_ARG, "epipolar search: NULL buffer");
    batch_operands o;
    const int rc = batch_operands_of(c, "epipolar search", train_src, o);
    if (rc != SS_OK) return rc;
    const bow_keep keep = bow_keep_of(c->d_bow_keep.p, o.n_frames, o.kcap);
    ssk_guided_call g;
    batch_sides(g, o);
    g.idx = (int32_t *)d_idx, g.d1 = (uint16_t *)d_d1;
    ssk_epi_call e;
    e.q_node = keep.node;
    e.index = keep.index, e.n_index = keep.n_index;
    e.q_taken = e.t_taken = (const uint8_t *)d_taken;
    e.summary = (ss_epi_summary *)d_summary;
    return epi_match_run(c, g, e, pairs, p, nullptr);
}

/* the two launches of a triangulation whose operands and outputs are filled in */
static int tri_run(ss_ctx *c, ssk_tri_call &t, const ss_epi_pair *pairs, const ss_tri_params *tp)
{
    t.tp = *tp;
    int rc = context_pyramid(c, "epipolar search", &t.n_levels, t.scale);
    if (rc != SS_OK) return rc;
    const size_t nr = (size_t)t.n_frames * t.rows;
    rc = grow(c, c->d_tri_ws, nr * sizeof(ss_map_point));
    if (rc != SS_OK) return rc;
    rc = upload_epi_pairs(c, pairs, t.n_frames);
    if (rc != SS_OK) return rc;
    t.pairs = c->epi_tab.as<ss_epi_pair>();
    t.tmp = (ss_map_point *)c->d_tri_ws.p;
    {
        /* per row: its match, its keypoint and its info; a matched row reads the other keypoint on top */
        stage_timer s(c, "tri_eval", (int64_t)nr * (4 + (int64_t)sizeof(ss_keypoint) + (int64_t)sizeof(ss_tri_info)));
        ssk_tri_eval(c->stream, t);
    }
    {
        /* the states read; what a point moves (its 32 bytes twice, its descriptor twice, its rows) depends on the content */
        stage_timer s(c, "tri_compact", (int64_t)nr * 4 + t.n_frames * (int64_t)(sizeof(ss_tri_summary) + 4));
        ssk_tri_compact(c->stream, t);
    }
    HIP_TRY(c, hipGetLastError());
    return SS_OK;
}

static void tri_outputs(ssk_tri_call &t, void *d_info, void *d_points, void *d_point_desc, void *d_point_rows, void *d_n_points, void *d_summary)
{
    t.info = (ss_tri_info *)d_info;
    t.points = (ss_map_point *)d_points, t.point_desc = (uint8_t *)d_point_desc, t.point_rows = (int32_t *)d_point_rows;
    t.n_points = (int32_t *)d_n_points;
    t.summary = (ss_tri_summary *)d_summary;
}

int ss_triangulate_pairs_device(ss_ctx *c, const void *d_query, const void *d_query_kp, const void *d_n_query, const void *d_train_kp,
                                const void *d_n_train, const void *d_idx, int n_frames, int rows_per_frame, const ss_epi_pair *pairs,
                                const ss_tri_params *tp, void *d_info, void *d_points, void *d_point_desc, void *d_point_rows, void *d_n_points,
                                void *d_summary)
{
    if (!c) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    if (!tp) return fail(c, SS_ERR_INVALID_ARG, "triangulation: params is NULL");
    const int rc = pairs_shape(c, "triangulation", "pair", n_frames, rows_per_frame);
    if (rc != SS_OK) return rc;
    if (n_frames == 0) return SS_OK;
    if (!d_query || !d_query_kp || !d_n_query || !d_train_kp || !d_n_train || !d_idx || !pairs || !d_info || !d_points || !d_point_desc || !d_point_rows ||
        !d_n_points || !d_summary)
        return fail(c, SS_ERR_INVALID_ARG, "triangulation: NULL buffer");
    ssk_tri_call t;
    t.n_frames = n_frames;
    t.rows = rows_per_frame;
    t.q_kp = (const ss_keypoint *)d_query_kp, t.t_kp = (const ss_keypoint *)d_train_kp;
    t.q_desc = (const uint8_t *)d_query;
    t.nq = (const int32_t *)d_n_query, t.nt = (const int32_t *)d_n_train;
    t.idx = (const int32_t *)d_idx;
    tri_outputs(t, d_info, d_points, d_point_desc, d_point_rows, d_n_points, d_summary);
    return tri_run(c, t, pairs, tp);
}

int ss_triangulate_batch_device(ss_ctx *c, const int32_t *train_src, const void *d_idx, const ss_epi_pair *pairs, const ss_tri_params *tp,
                                void *d_info, void *d_points, void *d_point_desc, void *d_point_rows, void *d_n_points, void *d_summary)
{
    if (!c) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    if (!have_batch(c, "ss_triangulate_batch_device")) return SS_ERR_STATE;
    if (!tp) return fail(c, SS_ERR_INVALID_ARG, "triangulation: params is NULL");
    if (!d_idx || !pairs || !d_info || !d_points || !d_point_desc || !d_point_rows || !d_n_points || !d_summary)
        return fail(c, SS_ERR_INVALID_ARG, "triangulation: NULL buffer");
    batch_operands o;
    const int rc = batch_operands_of(c, "triangulation", train_src, o);
    if (rc != SS_OK) return rc;
    ssk_tri_call t;
    t.n_frames = o.n_frames;
    t.rows = o.kcap;
    t.q_kp = t.t_kp = o.kps;
    t.q_desc = o.desc;
    t.nq = t.nt = o.n_kp;
    t.src = o.src;
    t.frame_error = o.frame_error;
    t.idx = (const int32_t *)d_idx;
    tri_outputs(t, d_info, d_points, d_point_desc, d_point_rows, d_n_points, d_summary);
    return tri_run(c, t, pairs, tp);
}

/* ---- the stereo form of the triangulation (k_tri_stereo_eval, ss_tri_stereo_eval) ---- */
int ss_triangulate_stereo_host(const ss_epi_pair *pair, const ss_tri_stereo_rig *rig, const ss_tri_stereo_params *tp, const float *scale, int n_levels,
                               const ss_keypoint *kp1, const ss_keypoint *kp2, const float *depth1, const float *right1, const float *depth2,
                               const float *right2, int n, ss_map_point *points, ss_tri_stereo_info *info)
{
    if (!pair || !rig || !tp || !scale || n_levels < 1 || n_levels > SS_MAX_LEVELS || n < 0 || (n > 0 && (!kp1 || !kp2 || !points || !info))) return SS_ERR_INVALID_ARG;
    const bool planes = depth1 && right1 && depth2 && right2;
    if (!planes && (depth1 || right1 || depth2 || right2)) return SS_ERR_INVALID_ARG; /* all four or none */
    for (int k = 0; k < n; k++) {
        const ss_tri_stereo_out r = ss_tri_stereo_eval(*pair, *rig, *tp, scale, n_levels, kp1[k].x, kp1[k].y, kp1[k].octave, planes ? depth1[k] : -1.0f,
                                                       planes ? right1[k] : -1.0f, kp2[k].x, kp2[k].y, kp2[k].octave, planes ? depth2[k] : -1.0f,
                                                       planes ? right2[k] : -1.0f);
        points[k] = r.point;
        info[k] = r.info;
    }
    return SS_OK;
}

/* the message of the first rule a plane of the stereo form breaks, or NULL */
static const char *tri_plane_error(const void *p, int64_t stride)
{
    if (!p) return "triangulation, stereo form: NULL plane";
    if (stride < 4 || stride % 4 != 0 || stride > ((int64_t)1 << 30)) return "triangulation, stereo form: a plane's stride must be a positive multiple of 4";
    if ((uintptr_t)p % 4 != 0) return "triangulation, stereo form: a plane's pointer must be a multiple of 4";
    return nullptr;
}

/* the three launches of a stereo triangulation whose sides, planes and outputs are filled in */
static int tri_stereo_run(ss_ctx *c, ssk_tri_stereo_call &sc, const ss_epi_pair *pairs, const ss_tri_stereo_rig *rigs, const ss_tri_stereo_params *tp)
{
    ssk_tri_call &t = sc.t;
    t.tp = tp->tri, sc.chi2_stereo = tp->chi2_stereo;
    int rc = context_pyramid(c, "epipolar search", &t.n_levels, t.scale);
    if (rc != SS_OK) return rc;
    const size_t nr = (size_t)t.n_frames * t.rows, n = (size_t)t.n_frames;
    rc = carve_from(c, c->d_tri_ws, [&](carve &w) {
        t.tmp = w.take<ss_map_point>(nr * sizeof(ss_map_point));
        t.info = w.take<ss_tri_info>(nr * sizeof(ss_tri_info));
        t.summary = w.take<ss_tri_summary>(n * sizeof(ss_tri_summary));
    });
    if (rc != SS_OK) return rc;
    /* the pairs, then the rigs */
    const size_t pb = n * sizeof(ss_epi_pair), rb = n * sizeof(ss_tri_stereo_rig);
    rc = staged_upload(c, c->epi_tab, pb + rb, [&](uint8_t *h) {
        memcpy(h, pairs, pb);
        memcpy(h + pb, rigs, rb);
    });
    if (rc != SS_OK) return rc;
    t.pairs = c->epi_tab.as<ss_epi_pair>(), sc.rigs = c->epi_tab.as<ss_tri_stereo_rig>(pb);
    {
        /* per row: its match, its keypoint, both records; a matched row reads the other keypoint and the four plane values on top */
        stage_timer s(c, "tri_stereo_eval", (int64_t)nr * (4 + (int64_t)sizeof(ss_keypoint) + (int64_t)sizeof(ss_tri_info) + (int64_t)sizeof(ss_tri_stereo_info)));
        ssk_tri_stereo_eval(c->stream, sc);
    }
    {
        stage_timer s(c, "tri_compact", (int64_t)nr * 4 + t.n_frames * (int64_t)(sizeof(ss_tri_summary) + 4));
        ssk_tri_compact(c->stream, t);
    }
    {
        stage_timer s(c, "tri_stereo_summary", (int64_t)nr * 8 + t.n_frames * (int64_t)(sizeof(ss_tri_summary) + sizeof(ss_tri_stereo_summary)));
        ssk_tri_stereo_summary(c->stream, sc);
    }
    HIP_TRY(c, hipGetLastError());
    return SS_OK;
}

static void tri_stereo_outputs(ssk_tri_stereo_call &sc, void *d_info, void *d_points, void *d_point_desc, void *d_point_rows, void *d_n_points, void *d_summary)
{
    sc.sinfo = (ss_tri_stereo_info *)d_info;
    sc.t.points = (ss_map_point *)d_points, sc.t.point_desc = (uint8_t *)d_point_desc, sc.t.point_rows = (int32_t *)d_point_rows;
    sc.t.n_points = (int32_t *)d_n_points;
    sc.ssummary = (ss_tri_stereo_summary *)d_summary;
}

int ss_triangulate_stereo_pairs_device(ss_ctx *c, const void *d_query, const void *d_query_kp, const void *d_n_query, const void *d_train_kp,
                                       const void *d_n_train, const void *d_idx, int n_frames, int rows_per_frame, const ss_epi_pair *pairs,
                                       const ss_tri_stereo_rig *rigs, const void *d_depth1, int64_t depth1_stride, const void *d_right1,
                                       int64_t right1_stride, const void *d_depth2, int64_t depth2_stride, const void *d_right2, int64_t right2_stride,
                                       const ss_tri_stereo_params *tp, void *d_info, void *d_points, void *d_point_desc, void *d_point_rows,
                                       void *d_n_points, void *d_summary)
{
    if (!c) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    if (!tp) return fail(c, SS_ERR_INVALID_ARG, "triangulation, stereo form: params is NULL");
    const int rc = pairs_shape(c, "triangulation, stereo form", "pair", n_frames, rows_per_frame);
    if (rc != SS_OK) return rc;
    if (n_frames == 0) return SS_OK;
    if (!d_query || !d_query_kp || !d_n_query || !d_train_kp || !d_n_train || !d_idx || !pairs || !rigs || !d_info || !d_points || !d_point_desc ||
        !d_point_rows || !d_n_points || !d_summary)
        return fail(c, SS_ERR_INVALID_ARG, "triangulation, stereo form: NULL buffer");
    const void *planes[4] = {d_depth1, d_right1, d_depth2, d_right2};
    const int64_t strides[4] = {depth1_stride, right1_stride, depth2_stride, right2_stride};
    for (int k = 0; k < 4; k++)
        if (const char *msg = tri_plane_error(planes[k], strides[k])) return fail(c, SS_ERR_INVALID_ARG, msg);
    ssk_tri_stereo_call sc;
    ssk_tri_call &t = sc.t;
    t.n_frames = n_frames;
    t.rows = rows_per_frame;
    t.q_kp = (const ss_keypoint *)d_query_kp, t.t_kp = (const ss_keypoint *)d_train_kp;
    t.q_desc = (const uint8_t *)d_query;
    t.nq = (const int32_t *)d_n_query, t.nt = (const int32_t *)d_n_train;
    t.idx = (const int32_t *)d_idx;
    sc.depth1 = (const uint8_t *)d_depth1, sc.right1 = (const uint8_t *)d_right1, sc.depth2 = (const uint8_t *)d_depth2, sc.right2 = (const uint8_t *)d_right2;
    sc.depth1_stride = depth1_stride, sc.right1_stride = right1_stride, sc.depth2_stride = depth2_stride, sc.right2_stride = right2_stride;
    tri_stereo_outputs(sc, d_info, d_points, d_point_desc, d_point_rows, d_n_points, d_summary);
    return tri_stereo_run(c, sc, pairs, rigs, tp);
}

int ss_triangulate_stereo_batch_device(ss_ctx *c, const int32_t *train_src, const void *d_idx, const ss_epi_pair *pairs, const ss_tri_stereo_rig *rigs,
                                       const void *d_depth, int64_t depth_stride, const void *d_right, int64_t right_stride,
                                       const ss_tri_stereo_params *tp, void *d_info, void *d_points, void *d_point_desc, void *d_point_rows,
                                       void *d_n_points, void *d_summary)
{
    if (!c) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    if (!have_batch(c, "ss_triangulate_stereo_batch_device")) return SS_ERR_STATE;
    if (!tp) return fail(c, SS_ERR_INVALID_ARG, "triangulation, stereo form: params is NULL");
    if (!d_idx || !pairs || !rigs || !d_info || !d_points || !d_point_desc || !d_point_rows || !d_n_points || !d_summary)
        return fail(c, SS_ERR_INVALID_ARG, "triangulation, stereo form: NULL buffer");
    if (const char *msg = tri_plane_error(d_depth, depth_stride)) return fail(c, SS_ERR_INVALID_ARG, msg);
    if (const char *msg = tri_plane_error(d_right, right_stride)) return fail(c, SS_ERR_INVALID_ARG, msg);
    batch_operands o;
    const int rc = batch_operands_of(c, "triangulation, stereo form", train_src, o);
    if (rc != SS_OK) return rc;
    ssk_tri_stereo_call sc;
    ssk_tri_call &t = sc.t;
    t.n_frames = o.n_frames;
    t.rows = o.kcap;
    t.q_kp = t.t_kp = o.kps;
    t.q_desc = o.desc;
    t.nq = t.nt = o.n_kp;
    t.src = o.src;
    t.frame_error = o.frame_error;
    t.idx = (const int32_t *)d_idx;
    sc.depth1 = sc.depth2 = (const uint8_t *)d_depth, sc.right1 = sc.right2 = (const uint8_t *)d_right;
    sc.depth1_stride = sc.depth2_stride = depth_stride, sc.right1_stride = sc.right2_stride = right_stride;
    tri_stereo_outputs(sc, d_info, d_points, d_point_desc, d_point_rows, d_n_points, d_summary);
    return tri_stereo_run(c, sc, pairs, rigs, tp);
}

/* ---- Sim3 from matched map points (csrc/ss_sim3.hip, csrc/ss_sim3_steps.h) ---- */
/* the message of the first rule p breaks, or NULL; needs no context */
static const char *sim3_params_error(const ss_sim3_params *p)
{
    if (!p) return "sim3: params is NULL";
    if (!(p->chi2 > 0.0f) || !std::isfinite(p->chi2)) return "sim3: chi2 must be finite and > 0";
    if (p->min_inliers < 0) return "sim3: min_inliers must be >= 0";
    if (p->max_iterations < 1 || p->max_iterations > SS_SIM3_MAX_ITERATIONS) return "sim3: max_iterations must be 1 .. SS_SIM3_MAX_ITERATIONS";
    if (p->reserved[0] != 0 || p->reserved[1] != 0 || p->reserved[2] != 0) return "sim3: the reserved fields must be 0";
    return nullptr;
}

static void sim3_model_into(const ss_sim3_model &m, ss_sim3_result *out)
{
    memcpy(out->sr12, m.sr12, sizeof(m.sr12));
    memcpy(out->t12, m.t12, sizeof(m.t12));
    memcpy(out->sr21, m.sr21, sizeof(m.sr21));
    memcpy(out->t21, m.t21, sizeof(m.t21));
    out->s12 = m.s12;
}

int ss_sim3_model_host(const ss_sim3_params *p, const float x1[9], const float x2[9], ss_sim3_result *out)
{
    if (sim3_params_error(p) || !x1 || !x2 || !out) return SS_ERR_INVALID_ARG;
    memset(out, 0, sizeof(*out));
    sim3_model_into(ss_sim3_model_of(x1, x2, p->fix_scale != 0), out);
    out->iteration = -1;
    return SS_OK;
}

int ss_sim3_check_host(const ss_sim3_params *p, const ss_proj_view *view1, const ss_proj_view *view2, const float *scale, int n_levels,
                       const ss_map_point *points1, const ss_keypoint *kp1, const ss_map_point *points2, const ss_keypoint *kp2, int n,
                       const ss_sim3_result *model, uint8_t *out, float *err)
{
    if (sim3_params_error(p)) return SS_ERR_INVALID_ARG;
    if (!view1 || !view2 || !scale || n_levels < 1 || n_levels > SS_MAX_LEVELS || !model || n < 0 || (n > 0 && (!points1 || !kp1 || !points2 || !kp2 || !out)))
        return SS_ERR_INVALID_ARG;
    for (int k = 0; k < n; k++) {
        const int o1 = kp1[k].octave, o2 = kp2[k].octave;
        if (err) err[2 * k] = err[2 * k + 1] = 0.0f;
        if (!(o1 >= 0 && o1 < n_levels && o2 >= 0 && o2 < n_levels)) {
            out[k] = 1;
            continue;
        }
        const ss_sim3_corr c = ss_sim3_corr_of(*view1, *view2, points1[k].x, points1[k].y, points1[k].z, points2[k].x, points2[k].y, points2[k].z,
                                               p->chi2, scale[o1], scale[o2]);
        const float e1 = ss_sim3_err(model->sr12, model->t12, c.x2, view1->fx, view1->fy, view1->cx, view1->cy, c.u1, c.v1);
        const float e2 = ss_sim3_err(model->sr21, model->t21, c.x1, view2->fx, view2->fy, view2->cx, view2->cy, c.u2, c.v2);
        if (err) err[2 * k] = e1, err[2 * k + 1] = e2;
        out[k] = !(e1 < c.max1) ? 2 : !(e2 < c.max2) ? 3 : 0;
    }
    return SS_OK;
}

int ss_sim3_to_view(const ss_camera *cam, const ss_sim3_result *result, const double rcw2[9], const double tcw2[3], float bf, double *srcw_out,
                    double *t_out, ss_proj_view *out)
{
    if (!cam || !result || !rcw2 || !tcw2 || !out || result->state != 0) return SS_ERR_INVALID_ARG;
    double m[9], t[3];
    for (int i = 0; i < 3; i++) {
        const double a0 = result->sr12[3 * i], a1 = result->sr12[3 * i + 1], a2 = result->sr12[3 * i + 2];
        for (int j = 0; j < 3; j++) m[3 * i + j] = (a0 * rcw2[j] + a1 * rcw2[3 + j]) + a2 * rcw2[6 + j];
        t[i] = ((a0 * tcw2[0] + a1 * tcw2[1]) + a2 * tcw2[2]) + (double)result->t12[i];
    }
    if (srcw_out) memcpy(srcw_out, m, sizeof(m));
    if (t_out) memcpy(t_out, t, sizeof(t));
    return ss_fuse_view_sim3(cam, m, t, bf, out);
}

/* The checks the device forms share, the workspace, the views (pair_views), then the four launches of a call whose device operands
 * and outputs are filled in */
static int sim3_run(ss_ctx *c, ssk_sim3_call &g, const ss_sim3_params *p, const ss_proj_view *views1, const ss_proj_view *views2, const int32_t *train_src)
{
    int rc = call_count_ok(c, "sim3", g.n_frames, "pairs");
    if (rc == SS_OK) rc = context_pyramid(c, "sim3", &g.n_levels, g.scale);
    if (rc != SS_OK) return rc;
    g.chi2 = p->chi2, g.min_inliers = p->min_inliers, g.max_iterations = p->max_iterations, g.fix_scale = p->fix_scale != 0, g.seed = p->seed;
    const size_t nr = (size_t)g.n_frames * g.rows, nh = (size_t)g.n_frames * g.max_iterations;
    rc = carve_from(c, c->d_sim3_ws, [&](carve &w) {
        g.corr = w.take<float>(12 * nr * sizeof(float));
        g.corr_of_row = w.take<int32_t>(nr * sizeof(int32_t));
        g.n_corr = w.take<int32_t>((size_t)g.n_frames * sizeof(int32_t));
        g.models = w.take<ssk_sim3_model>(nh * sizeof(ssk_sim3_model));
        g.counts = w.take<int32_t>(nh * sizeof(int32_t));
    });
    if (rc == SS_OK) rc = pair_views(c, c->sim3_tab, g, views1, views2, train_src);
    if (rc != SS_OK) return rc;
    const int64_t np = g.n_frames;
    {
        /* per query row: its match and the number written; a correspondence reads two map points, two octaves and up to two flags
         * and writes its twelve floats */
        stage_timer t(c, "sim3_gather", (int64_t)nr * (4 + 4 + 2 * (int64_t)sizeof(ss_map_point) + 2 * 4 + (g.q_skip ? 1 : 0) + (g.t_skip ? 1 : 0) + 48) + np * 4);
        ssk_sim3_gather(c->stream, g);
    }
    {
        /* per hypothesis: three correspondences' six floats read, one record and one count written */
        stage_timer t(c, "sim3_model", (int64_t)nh * (3 * 24 + (int64_t)sizeof(ssk_sim3_model) + 4));
        ssk_sim3_model_launch(c->stream, g);
    }
    {
        /* every block of hypotheses reads the twelve floats of every correspondence once and its own records; the counts are added */
        const int64_t hb = (g.max_iterations + SSK_SIM3_HYP_BLOCK - 1) / SSK_SIM3_HYP_BLOCK;
        stage_timer t(c, "sim3_count", (int64_t)nr * 48 * hb + (int64_t)nh * ((int64_t)sizeof(ssk_sim3_model) + 4));
        ssk_sim3_count(c->stream, g);
    }
    {
        /* the counts read; per query row its number read and its flag written, an inlier candidate's twelve floats on top */
        stage_timer t(c, "sim3_finish", (int64_t)nh * 4 + (int64_t)nr * (4 + 1 + 48) + np * (int64_t)(sizeof(ssk_sim3_model) + sizeof(ss_sim3_result)));
        ssk_sim3_finish(c->stream, g);
    }
    HIP_TRY(c, hipGetLastError());
    return SS_OK;
}

int ss_sim3_pairs_device(ss_ctx *c, const void *d_query_xyz, const void *d_query_kp, const void *d_query_skip, const void *d_n_query,
                         const void *d_train_xyz, const void *d_train_kp, const void *d_train_skip, const void *d_n_train, const void *d_idx,
                         int n_pairs, int rows, const ss_proj_view *views1, const ss_proj_view *views2, const ss_sim3_params *p, void *d_inlier,
                         void *d_result)
{
    if (!c) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    if (const char *msg = sim3_params_error(p)) return fail(c, SS_ERR_INVALID_ARG, msg);
    const int rc = pairs_shape(c, "sim3", "pair", n_pairs, rows);
    if (rc != SS_OK) return rc;
    if (n_pairs == 0) return SS_OK;
    if (!d_query_xyz || !d_query_kp || !d_n_query || !d_train_xyz || !d_train_kp || !d_n_train || !d_idx || !views1 || !views2 || !d_inlier || !d_result)
        return fail(c, SS_ERR_INVALID_ARG, "sim3: NULL buffer");
    ssk_sim3_call g;
    pairs_sides(g, n_pairs, rows, d_query_xyz, d_query_kp, d_query_skip, d_n_query, d_train_xyz, d_train_kp, d_train_skip, d_n_train, d_idx);
    g.inlier = (uint8_t *)d_inlier, g.result = (ss_sim3_result *)d_result;
    return sim3_run(c, g, p, views1, views2, nullptr);
}

int ss_sim3_batch_device(ss_ctx *c, const int32_t *train_src, const void *d_xyz, const void *d_skip, const void *d_idx, const ss_proj_view *views,
                         const ss_sim3_params *p, void *d_inlier, void *d_result)
{
    if (!c) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    if (!have_batch(c, "ss_sim3_batch_device")) return SS_ERR_STATE;
    if (const char *msg = sim3_params_error(p)) return fail(c, SS_ERR_INVALID_ARG, msg);
    if (!d_xyz || !d_idx || !views || !d_inlier || !d_result) return fail(c, SS_ERR_INVALID_ARG, "sim3: NULL buffer");
    batch_operands o;
    const int rc = batch_operands_of(c, "sim3", train_src, o);
    if (rc != SS_OK) return rc;
    ssk_sim3_call g;
    batch_sides(g, o, d_xyz, d_skip, d_idx);
    g.inlier = (uint8_t *)d_inlier, g.result = (ss_sim3_result *)d_result;
    return sim3_run(c, g, p, views, nullptr, train_src);
}

int ss_sim3(ss_ctx *c, const ss_proj_view *view1, const ss_map_point *query_xyz, const ss_keypoint *query_kp, const uint8_t *query_skip, int n_query,
            const ss_proj_view *view2, const ss_map_point *train_xyz, const ss_keypoint *train_kp, const uint8_t *train_skip, int n_train,
            const int32_t *idx, const ss_sim3_params *p, uint8_t *inlier, ss_sim3_result *result)
{
    if (!c) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    return single_pair(c, "sim3", c->d_sim3_io, query_xyz, query_kp, query_skip, n_query, train_xyz, train_kp, train_skip, n_train, idx, view1 && view2,
                       nullptr, 0, inlier, result, sizeof(ss_sim3_result), [&](const io_piece *io, int rows) {
                           return ss_sim3_pairs_device(c, io[PP_QX].d, io[PP_QK].d, io[PP_QS].d, io[PP_N].d, io[PP_TX].d, io[PP_TK].d, io[PP_TS].d,
                                                       io[PP_N].d + 4, io[PP_IDX].d, 1, rows, view1, view2, p, io[PP_FLAGS].d, io[PP_RES].d);
                       });
}

/* ---- pose-only optimisation (csrc/ss_pose.hip, csrc/ss_pose_steps.h) ---- */
/* the message of the first rule p breaks, or NULL; needs no context */
static const char *pose_params_error(const ss_pose_opt_params *p)
{
    if (!p) return "pose optimisation: params is NULL";
    if (!(p->chi2_mono > 0.0) || !std::isfinite(p->chi2_mono)) return "pose optimisation: chi2_mono must be finite and > 0";
    if (!(p->chi2_stereo > 0.0) || !std::isfinite(p->chi2_stereo)) return "pose optimisation: chi2_stereo must be finite and > 0";
    if (!(p->lambda >= 0.0) || !std::isfinite(p->lambda)) return "pose optimisation: lambda must be finite and >= 0";
    if (!(p->step_eps >= 0.0) || !std::isfinite(p->step_eps)) return "pose optimisation: step_eps must be finite and >= 0";
    if (p->n_rounds < 1 || p->n_rounds > 8) return "pose optimisation: n_rounds must be 1 .. 8";
    if (p->iterations < 1 || p->iterations > 32) return "pose optimisation: iterations must be 1 .. 32";
    if (p->robust_rounds < 0 || p->robust_rounds > 8) return "pose optimisation: robust_rounds must be 0 .. 8";
    if (p->min_obs < 3) return "pose optimisation: min_obs must be >= 3";
    if (p->reserved[0] != 0 || p->reserved[1] != 0) return "pose optimisation: the reserved fields must be 0";
    return nullptr;
}

int ss_pose_opt_host(const ss_proj_view *view, const double *start, const float *scale, int n_levels, const ss_map_point *points,
                     const uint8_t *point_skip, int n_points, const ss_keypoint *kp, const float *right, int n_kp, const int32_t *idx,
                     const ss_pose_opt_params *p, uint8_t *flags, ss_pose_result *result)
{
    if (pose_params_error(p)) return SS_ERR_INVALID_ARG;
    if (!view || !start || !scale || n_levels < 1 || n_levels > SS_MAX_LEVELS || n_points < 0 || n_kp < 0 || !result) return SS_ERR_INVALID_ARG;
    const int slots = p->idx_by_row ? n_kp : n_points;
    if ((n_points > 0 && !points) || (n_kp > 0 && !kp) || (slots > 0 && (!idx || !flags))) return SS_ERR_INVALID_ARG;
    /* step 1 */
    std::vector<ss_pose_obs> obs;
    std::vector<int> slot_of;
    for (int i = 0; i < slots; i++) {
        const int prow = p->idx_by_row ? idx[i] : i, krow = p->idx_by_row ? i : idx[i];
        flags[i] = 2;
        if (!(prow >= 0 && prow < n_points && krow >= 0 && krow < n_kp)) continue;
        const int octave = kp[krow].octave;
        if (!(octave >= 0 && octave < n_levels)) continue;
        if (point_skip && point_skip[prow] != 0) continue;
        const float ur = ss_pose_stored_right(p->check_right != 0, right != nullptr, right ? right[krow] : 0.0f);
        obs.push_back(ss_pose_obs_of(points[prow].x, points[prow].y, points[prow].z, kp[krow].x, kp[krow].y, ur, scale[octave]));
        slot_of.push_back(i);
    }
    const int n = (int)obs.size();
    std::vector<uint8_t> active((size_t)n + 1);
    std::vector<double> slot((size_t)(SS_POSE_SUMS + 1) * SS_GN_SLOTS);
    ss_pose_frame_host(obs.data(), n, ss_pose_cam_of(*view, p->chi2_mono, p->chi2_stereo), start, *p, active.data(), slot.data(), result);
    for (int k = 0; k < n; k++) flags[slot_of[(size_t)k]] = active[(size_t)k] ? 0 : 1;
    return SS_OK;
}

/* The checks the device forms share, the workspace, the host tables (views, block numbers, start poses), then the two launches of
 * a call whose device operands and outputs are filled in */
static int pose_run(ss_ctx *c, ssk_pose_call &g, int n_blocks, const ss_proj_view *views, const double *start_poses, const int32_t *point_src,
                    const ss_pose_opt_params *p)
{
    if (const char *msg = pose_params_error(p)) return fail(c, SS_ERR_INVALID_ARG, msg);
    if (g.n_frames < 0 || n_blocks < 0 || g.point_rows < 1 || g.rows < 1) return fail(c, SS_ERR_INVALID_ARG, "pose optimisation: bad frame, block or row count");
    if (g.point_rows > SS_GUIDED_MAX_ROWS || g.rows > SS_GUIDED_MAX_ROWS)
        return fail(c, SS_ERR_INVALID_ARG, "pose optimisation: point_rows " + std::to_string(g.point_rows) + " / rows_per_frame " + std::to_string(g.rows) +
                                               " exceed SS_GUIDED_MAX_ROWS (" + std::to_string(SS_GUIDED_MAX_ROWS) + ")");
    int rc = call_count_ok(c, "pose optimisation", g.n_frames, "frames");
    if (rc == SS_OK) rc = context_pyramid(c, "pose optimisation", &g.n_levels, g.scale);
    if (rc != SS_OK) return rc;
    if (g.n_frames == 0) return SS_OK;
    if (!views || !start_poses) return fail(c, SS_ERR_INVALID_ARG, "pose optimisation: views or start_poses is NULL");
    for (int b = 0; b < g.n_frames; b++) {
        const int pb = point_src ? point_src[b] : b;
        if (pb < 0 || pb >= n_blocks)
            return fail(c, SS_ERR_INVALID_ARG, std::string(point_src ? "point_src[" : "frame [") + std::to_string(b) + "] = " + std::to_string(pb) +
                                                   " names no block of points (" + std::to_string(n_blocks) + ")");
    }
    if (!g.points || !g.np || !g.kp || !g.nk || !g.idx || !g.flags || !g.result) return fail(c, SS_ERR_INVALID_ARG, "pose optimisation: NULL buffer");
    g.chi2_mono = p->chi2_mono, g.chi2_stereo = p->chi2_stereo, g.lambda = p->lambda, g.step_eps = p->step_eps;
    g.n_rounds = p->n_rounds, g.iterations = p->iterations, g.robust_rounds = p->robust_rounds, g.min_obs = p->min_obs;
    g.check_right = p->check_right != 0, g.idx_by_row = p->idx_by_row != 0;
    g.slots = g.idx_by_row ? g.rows : g.point_rows;
    const size_t ns = (size_t)g.n_frames * g.slots;
    rc = carve_from(c, c->d_pose_ws, [&](carve &w) {
        g.planes = w.take<float>(7 * ns * sizeof(float));
        g.slot_of = w.take<int32_t>(ns * sizeof(int32_t));
        g.n_obs = w.take<int32_t>((size_t)g.n_frames * sizeof(int32_t));
    });
    if (rc != SS_OK) return rc;
    /* the host tables of the call: n_frames views, then n_frames start poses, then n_frames block numbers */
    const size_t vb = (size_t)g.n_frames * sizeof(ss_proj_view), sb = (size_t)g.n_frames * 12 * sizeof(double);
    rc = staged_upload(c, c->pose_tab, vb + sb + (size_t)g.n_frames * sizeof(int32_t), [&](uint8_t *h) {
        memcpy(h, views, vb);
        memcpy(h + vb, start_poses, sb);
        int32_t *src = (int32_t *)(h + vb + sb);
        for (int b = 0; b < g.n_frames; b++) src[b] = point_src ? point_src[b] : b;
    });
    if (rc != SS_OK) return rc;
    g.views = c->pose_tab.as<ss_proj_view>();
    g.start = c->pose_tab.as<double>(vb);
    g.src = c->pose_tab.as<int32_t>(vb + sb);
    {
        /* per slot: its match and its flag or slot number; an observation reads a map point, a keypoint, up to a flag and a right
         * coordinate and writes its seven floats */
        stage_timer t(c, "pose_gather", (int64_t)ns * (4 + 4 + (int64_t)sizeof(ss_map_point) + (int64_t)sizeof(ss_keypoint) + (g.p_skip ? 1 : 0) + (g.right ? 4 : 0) + 28) +
                                            (int64_t)g.n_frames * 4);
        ssk_pose_gather(c->stream, g);
    }
    {
        /* every step and every classification reads the observations' planes once (an upper bound: a round may end early) */
        const int64_t passes = (int64_t)g.n_rounds * (g.iterations + 1);
        stage_timer t(c, "pose_solve", (int64_t)ns * (28 * passes + 4 + 1) + (int64_t)g.n_frames * (int64_t)(sizeof(ss_proj_view) + 96 + sizeof(ss_pose_result)));
        ssk_pose_solve(c->stream, g);
    }
    HIP_TRY(c, hipGetLastError());
    return SS_OK;
}

int ss_pose_opt_pairs_device(ss_ctx *c, const void *d_points, const void *d_point_skip, const void *d_n_points, int n_blocks, int point_rows,
                             const void *d_kp, const void *d_right, const void *d_n_kp, int n_frames, int rows_per_frame, const void *d_idx,
                             const ss_proj_view *views, const double *start_poses, const int32_t *point_src, const ss_pose_opt_params *p,
                             void *d_flags, void *d_result)
{
    if (!c) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    ssk_pose_call g;
    g.n_frames = n_frames, g.point_rows = point_rows, g.rows = rows_per_frame;
    g.points = (const ss_map_point *)d_points, g.p_skip = (const uint8_t *)d_point_skip, g.np = (const int32_t *)d_n_points;
    g.kp = (const ss_keypoint *)d_kp, g.right = (const float *)d_right, g.nk = (const int32_t *)d_n_kp;
    g.idx = (const int32_t *)d_idx;
    g.flags = (uint8_t *)d_flags, g.result = (ss_pose_result *)d_result;
    return pose_run(c, g, n_blocks, views, start_poses, point_src, p);
}

int ss_pose_opt_batch_device(ss_ctx *c, const void *d_points, const void *d_point_skip, const void *d_n_points, int n_blocks, int point_rows,
                             const void *d_right, const void *d_idx, const ss_proj_view *views, const double *start_poses, const int32_t *point_src,
                             const ss_pose_opt_params *p, void *d_flags, void *d_result)
{
    if (!c) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    if (!have_batch(c, "ss_pose_opt_batch_device")) return SS_ERR_STATE;
    ssk_pose_call g;
    g.n_frames = c->last_n_frames, g.point_rows = point_rows, g.rows = c->hg.kcap;
    g.points = (const ss_map_point *)d_points, g.p_skip = (const uint8_t *)d_point_skip, g.np = (const int32_t *)d_n_points;
    g.kp = c->ws.kps, g.right = (const float *)d_right, g.nk = c->ws.n_kp;
    const int rc = flagged_frame_error(c, c->batch_test_flagged, &g.frame_error);
    if (rc != SS_OK) return rc;
    g.idx = (const int32_t *)d_idx;
    g.flags = (uint8_t *)d_flags, g.result = (ss_pose_result *)d_result;
    return pose_run(c, g, n_blocks, views, start_poses, point_src, p);
}

int ss_pose_opt(ss_ctx *c, const ss_proj_view *view, const double *start, const ss_map_point *points, const uint8_t *point_skip, int n_points,
                const ss_keypoint *kp, const float *right, int n_kp, const int32_t *idx, const ss_pose_opt_params *p, uint8_t *flags,
                ss_pose_result *result)
{
    if (!c) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    if (const char *msg = pose_params_error(p)) return fail(c, SS_ERR_INVALID_ARG, msg);
    if (n_points < 0 || n_kp < 0 || n_points > SS_GUIDED_MAX_ROWS || n_kp > SS_GUIDED_MAX_ROWS)
        return fail(c, SS_ERR_INVALID_ARG, "pose optimisation: n_points and n_kp must be 0 .. SS_GUIDED_MAX_ROWS");
    const size_t ns = (size_t)(p->idx_by_row ? n_kp : n_points);
    if (!view || !start || !result || (n_points > 0 && !points) || (n_kp > 0 && !kp) || (ns > 0 && (!idx || !flags)))
        return fail(c, SS_ERR_INVALID_ARG, "pose optimisation: NULL buffer");
    /* one block of `pr` points, one frame of `kr` rows; `counts` is on this stack: no return before the stream has read it */
    const size_t pr = (size_t)std::max(n_points, 1), kr = (size_t)std::max(n_kp, 1), np = (size_t)n_points, nk = (size_t)n_kp;
    const size_t sr = p->idx_by_row ? kr : pr;
    const int32_t counts[2] = {n_points, n_kp};
    enum { PT, PS, KP, RT, IDX, N, FL, RES, PIECES };
    io_piece io[PIECES] = {{points, nullptr, pr * sizeof(ss_map_point), np * sizeof(ss_map_point)}, {point_skip, nullptr, pr, np},
                           {kp, nullptr, kr * sizeof(ss_keypoint), nk * sizeof(ss_keypoint)}, {right, nullptr, kr * 4, nk * 4},
                           {idx, nullptr, sr * 4, ns * 4}, {counts, nullptr, sizeof(counts), sizeof(counts)}, {nullptr, flags, sr, ns},
                           {nullptr, result, sizeof(ss_pose_result), sizeof(ss_pose_result)}};
    int rc = io_send(c, c->d_pose_io, io, PIECES);
    if (rc == SS_OK)
        rc = ss_pose_opt_pairs_device(c, io[PT].d, point_skip ? io[PS].d : nullptr, io[N].d, 1, (int)pr, io[KP].d, right ? io[RT].d : nullptr, io[N].d + 4, 1,
                                      (int)kr, io[IDX].d, view, start, nullptr, p, io[FL].d, io[RES].d);
    if (rc != SS_OK) {
        (void)hipStreamSynchronize(c->stream);
        return rc;
    }
    return io_fetch(c, io, PIECES);
}

/* ---- Sim3 refinement (csrc/ss_sim3opt.hip, csrc/ss_sim3opt_steps.h) ---- */
/* the message of the first rule p breaks, or NULL; needs no context */
static const char *sim3opt_params_error(const ss_sim3_opt_params *p)
{
    if (!p) return "sim3 refinement: params is NULL";
    if (!(p->chi2 > 0.0) || !std::isfinite(p->chi2)) return "sim3 refinement: chi2 must be finite and > 0";
    if (!(p->lambda >= 0.0) || !std::isfinite(p->lambda)) return "sim3 refinement: lambda must be finite and >= 0";
    if (!(p->step_eps >= 0.0) || !std::isfinite(p->step_eps)) return "sim3 refinement: step_eps must be finite and >= 0";
    if (p->iterations0 < 1 || p->iterations0 > 32) return "sim3 refinement: iterations0 must be 1 .. 32";
    if (p->iterations_more < 1 || p->iterations_more > 32) return "sim3 refinement: iterations_more must be 1 .. 32";
    if (p->iterations_same < 1 || p->iterations_same > 32) return "sim3 refinement: iterations_same must be 1 .. 32";
    if (p->min_corr < 3) return "sim3 refinement: min_corr must be >= 3";
    if (p->min_inliers < 0) return "sim3 refinement: min_inliers must be >= 0";
    if (p->reserved[0] != 0 || p->reserved[1] != 0 || p->reserved[2] != 0 || p->reserved[3] != 0) return "sim3 refinement: the reserved fields must be 0";
    return nullptr;
}

int ss_sim3_opt_host(const ss_proj_view *view1, const ss_proj_view *view2, const float *scale, int n_levels, const ss_map_point *query_xyz,
                     const ss_keypoint *query_kp, const uint8_t *query_skip, int n_query, const ss_map_point *train_xyz,
                     const ss_keypoint *train_kp, const uint8_t *train_skip, int n_train, const int32_t *idx, const ss_sim3_result *start,
                     const ss_sim3_opt_params *p, uint8_t *flags, ss_sim3_opt_result *result)
{
    if (sim3opt_params_error(p)) return SS_ERR_INVALID_ARG;
    if (!view1 || !view2 || !scale || n_levels < 1 || n_levels > SS_MAX_LEVELS || n_query < 0 || n_train < 0 || !start || !result) return SS_ERR_INVALID_ARG;
    if ((n_query > 0 && (!query_xyz || !query_kp || !idx || !flags)) || (n_train > 0 && (!train_xyz || !train_kp))) return SS_ERR_INVALID_ARG;
    /* step 1 */
    std::vector<ss_sim3opt_corr> corr;
    std::vector<int> row_of;
    const bool usable = ss_sim3opt_start_usable(*start);
    for (int i = 0; i < n_query; i++) {
        flags[i] = 2;
        const int j = idx[i];
        if (!usable || !(j >= 0 && j < n_train)) continue;
        const int o1 = query_kp[i].octave, o2 = train_kp[j].octave;
        if (!(o1 >= 0 && o1 < n_levels && o2 >= 0 && o2 < n_levels)) continue;
        if ((query_skip && query_skip[i] != 0) || (train_skip && train_skip[j] != 0)) continue;
        float x1[3], x2[3];
        ss_sim3_transform(view1->rcw, view1->tcw, query_xyz[i].x, query_xyz[i].y, query_xyz[i].z, x1);
        ss_sim3_transform(view2->rcw, view2->tcw, train_xyz[j].x, train_xyz[j].y, train_xyz[j].z, x2);
        corr.push_back(ss_sim3opt_corr_of(x1, x2, query_kp[i].x, query_kp[i].y, train_kp[j].x, train_kp[j].y, scale[o1], scale[o2]));
        row_of.push_back(i);
    }
    const int n = (int)corr.size();
    std::vector<uint8_t> active((size_t)n + 1);
    std::vector<double> slot((size_t)(SS_SIM3OPT_SUMS + 1) * SS_GN_SLOTS);
    ss_sim3opt_pair_host(corr.data(), n, ss_sim3opt_cams_of(*view1, *view2, p->chi2), *start, start->status, *p, active.data(), slot.data(), result);
    for (int k = 0; k < n; k++) flags[row_of[(size_t)k]] = active[(size_t)k] ? 0 : 1;
    return SS_OK;
}

int ss_sim3_to_view21(const ss_camera *cam, const ss_sim3_result *result, const double rcw1[9], const double tcw1[3], float bf, double *srcw_out,
                      double *t_out, ss_proj_view *out)
{
    if (!cam || !result || !rcw1 || !tcw1 || !out || result->state != 0) return SS_ERR_INVALID_ARG;
    double m[9], t[3];
    for (int i = 0; i < 3; i++) {
        const double a0 = result->sr21[3 * i], a1 = result->sr21[3 * i + 1], a2 = result->sr21[3 * i + 2];
        for (int j = 0; j < 3; j++) m[3 * i + j] = (a0 * rcw1[j] + a1 * rcw1[3 + j]) + a2 * rcw1[6 + j];
        t[i] = ((a0 * tcw1[0] + a1 * tcw1[1]) + a2 * tcw1[2]) + (double)result->t21[i];
    }
    if (srcw_out) memcpy(srcw_out, m, sizeof(m));
    if (t_out) memcpy(t_out, t, sizeof(t));
    return ss_fuse_view_sim3(cam, m, t, bf, out);
}

/* The checks the device forms share, the workspace, the views (pair_views), then the two launches of a call whose device operands
 * and outputs are filled in */
static int sim3opt_run(ss_ctx *c, ssk_sim3opt_call &g, const ss_sim3_opt_params *p, const ss_proj_view *views1, const ss_proj_view *views2,
                       const int32_t *train_src)
{
    int rc = call_count_ok(c, "sim3 refinement", g.n_frames, "pairs");
    if (rc == SS_OK) rc = context_pyramid(c, "sim3 refinement", &g.n_levels, g.scale);
    if (rc != SS_OK) return rc;
    g.p = *p;
    const size_t nr = (size_t)g.n_frames * g.rows;
    rc = carve_from(c, c->d_sim3opt_ws, [&](carve &w) {
        g.planes = w.take<float>(12 * nr * sizeof(float));
        g.row_of = w.take<int32_t>(nr * sizeof(int32_t));
        g.n_corr = w.take<int32_t>((size_t)g.n_frames * sizeof(int32_t));
    });
    if (rc == SS_OK) rc = pair_views(c, c->sim3opt_tab, g, views1, views2, train_src);
    if (rc != SS_OK) return rc;
    const int64_t np = g.n_frames;
    {
        /* per query row: its match and its flag or row number; a correspondence reads two map points, two keypoints and up to two
         * flags and writes its twelve floats; per pair the start is read and N written */
        stage_timer t(c, "sim3opt_gather", (int64_t)nr * (4 + 4 + 2 * (int64_t)sizeof(ss_map_point) + 2 * (int64_t)sizeof(ss_keypoint) + (g.q_skip ? 1 : 0) +
                                                          (g.t_skip ? 1 : 0) + 48) + np * (int64_t)(sizeof(ss_sim3_result) + 4));
        ssk_sim3opt_gather(c->stream, g);
    }
    {
        /* every step and both classifications read the correspondences' planes once (an upper bound: a round may end early) */
        const int64_t passes = (int64_t)p->iterations0 + std::max(p->iterations_more, p->iterations_same) + 2;
        stage_timer t(c, "sim3opt_solve", (int64_t)nr * (48 * passes + 4 + 1) + np * (int64_t)(2 * sizeof(ss_proj_view) + sizeof(ss_sim3_result) + sizeof(ss_sim3_opt_result)));
        ssk_sim3opt_solve(c->stream, g);
    }
    HIP_TRY(c, hipGetLastError());
    return SS_OK;
}

int ss_sim3_opt_pairs_device(ss_ctx *c, const void *d_query_xyz, const void *d_query_kp, const void *d_query_skip, const void *d_n_query,
                             const void *d_train_xyz, const void *d_train_kp, const void *d_train_skip, const void *d_n_train, const void *d_idx,
                             int n_pairs, int rows, const ss_proj_view *views1, const ss_proj_view *views2, const void *d_start,
                             const ss_sim3_opt_params *p, void *d_flags, void *d_result)
{
    if (!c) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    if (const char *msg = sim3opt_params_error(p)) return fail(c, SS_ERR_INVALID_ARG, msg);
    const int rc = pairs_shape(c, "sim3 refinement", "pair", n_pairs, rows);
    if (rc != SS_OK) return rc;
    if (n_pairs == 0) return SS_OK;
    if (!d_query_xyz || !d_query_kp || !d_n_query || !d_train_xyz || !d_train_kp || !d_n_train || !d_idx || !views1 || !views2 || !d_start || !d_flags ||
        !d_result)
        return fail(c, SS_ERR_INVALID_ARG, "sim3 refinement: NULL buffer");
    ssk_sim3opt_call g;
    pairs_sides(g, n_pairs, rows, d_query_xyz, d_query_kp, d_query_skip, d_n_query, d_train_xyz, d_train_kp, d_train_skip, d_n_train, d_idx);
    g.start = (const ss_sim3_result *)d_start;
    g.flags = (uint8_t *)d_flags, g.result = (ss_sim3_opt_result *)d_result;
    return sim3opt_run(c, g, p, views1, views2, nullptr);
}

int ss_sim3_opt_batch_device(ss_ctx *c, const int32_t *train_src, const void *d_xyz, const void *d_skip, const void *d_idx, const ss_proj_view *views,
                             const void *d_start, const ss_sim3_opt_params *p, void *d_flags, void *d_result)
{
    if (!c) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    if (!have_batch(c, "ss_sim3_opt_batch_device")) return SS_ERR_STATE;
    if (const char *msg = sim3opt_params_error(p)) return fail(c, SS_ERR_INVALID_ARG, msg);
    if (!d_xyz || !d_idx || !views || !d_start || !d_flags || !d_result) return fail(c, SS_ERR_INVALID_ARG, "sim3 refinement: NULL buffer");
    batch_operands o;
    const int rc = batch_operands_of(c, "sim3 refinement", train_src, o);
    if (rc != SS_OK) return rc;
    ssk_sim3opt_call g;
    batch_sides(g, o, d_xyz, d_skip, d_idx);
    g.start = (const ss_sim3_result *)d_start;
    g.flags = (uint8_t *)d_flags, g.result = (ss_sim3_opt_result *)d_result;
    return sim3opt_run(c, g, p, views, nullptr, train_src);
}

int ss_sim3_opt(ss_ctx *c, const ss_proj_view *view1, const ss_map_point *query_xyz, const ss_keypoint *query_kp, const uint8_t *query_skip, int n_query,
                const ss_proj_view *view2, const ss_map_point *train_xyz, const ss_keypoint *train_kp, const uint8_t *train_skip, int n_train,
                const int32_t *idx, const ss_sim3_result *start, const ss_sim3_opt_params *p, uint8_t *flags, ss_sim3_opt_result *result)
{
    if (!c) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    return single_pair(c, "sim3 refinement", c->d_sim3opt_io, query_xyz, query_kp, query_skip, n_query, train_xyz, train_kp, train_skip, n_train, idx,
                       view1 && view2 && start, start, sizeof(ss_sim3_result), flags, result, sizeof(ss_sim3_opt_result), [&](const io_piece *io, int rows) {
                           return ss_sim3_opt_pairs_device(c, io[PP_QX].d, io[PP_QK].d, io[PP_QS].d, io[PP_N].d, io[PP_TX].d, io[PP_TK].d, io[PP_TS].d,
                                                           io[PP_N].d + 4, io[PP_IDX].d, 1, rows, view1, view2, io[PP_EXTRA].d, p, io[PP_FLAGS].d,
                                                           io[PP_RES].d);
                       });
}

/* the two launches of SearchBySim3's bookkeeping: the call's sides are filled in */
static int sim3_marks_run(ss_ctx *c, ssk_sim3_marks_call &g, bool mutual)
{
    if (const int rc = call_count_ok(c, "sim3 marks", g.n_frames, "pairs")) return rc;
    const int64_t nr = (int64_t)g.n_frames * g.rows;
    if (!mutual) {
        /* per row: its match and up to two skip bytes read, two bytes written; a valid match writes one more */
        stage_timer t(c, "sim3opt_marks", nr * (4 + (g.q_skip ? 1 : 0) + (g.t_skip ? 1 : 0) + 2 + 4 + 1) + (int64_t)g.n_frames * 8);
        ssk_sim3_marks(c->stream, g);
    } else {
        const int rc = carve_from(c, c->d_sim3opt_ws, [&](carve &w) { g.taken = w.take<uint8_t>((size_t)nr); });
        if (rc != SS_OK) return rc;
        /* per row: the taken byte written, the prior match read twice and marked, then up to two search results and a taken byte
         * read and the match written */
        stage_timer t(c, "sim3opt_mutual", nr * (1 + 4 + 1 + 4 + 4 + 4 + 1 + 4) + (int64_t)g.n_frames * (8 + (int64_t)sizeof(ss_sim3_mutual_summary)));
        ssk_sim3_mutual(c->stream, g);
    }
    HIP_TRY(c, hipGetLastError());
    return SS_OK;
}

int ss_sim3_marks_pairs_device(ss_ctx *c, const void *d_idx, const void *d_query_skip, const void *d_train_skip, const void *d_n_query,
                               const void *d_n_train, int n_pairs, int rows, void *d_skip1_out, void *d_skip2_out)
{
    if (!c) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    const int rc = pairs_shape(c, "sim3 marks", "pair", n_pairs, rows);
    if (rc != SS_OK) return rc;
    if (n_pairs == 0) return SS_OK;
    if (!d_idx || !d_n_query || !d_n_train || !d_skip1_out || !d_skip2_out) return fail(c, SS_ERR_INVALID_ARG, "sim3 marks: NULL buffer");
    ssk_sim3_marks_call g;
    g.n_frames = n_pairs, g.rows = rows;
    g.idx = (const int32_t *)d_idx, g.q_skip = (const uint8_t *)d_query_skip, g.t_skip = (const uint8_t *)d_train_skip;
    g.nq = (const int32_t *)d_n_query, g.nt = (const int32_t *)d_n_train;
    g.skip1 = (uint8_t *)d_skip1_out, g.skip2 = (uint8_t *)d_skip2_out;
    return sim3_marks_run(c, g, false);
}

int ss_sim3_mutual_pairs_device(ss_ctx *c, const void *d_idx, const void *d_idx12, const void *d_idx21, const void *d_n_query, const void *d_n_train,
                                int n_pairs, int rows, void *d_idx_out, void *d_summary)
{
    if (!c) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    const int rc = pairs_shape(c, "sim3 mutual", "pair", n_pairs, rows);
    if (rc != SS_OK) return rc;
    if (n_pairs == 0) return SS_OK;
    if (!d_idx || !d_idx12 || !d_idx21 || !d_n_query || !d_n_train || !d_idx_out || !d_summary) return fail(c, SS_ERR_INVALID_ARG, "sim3 mutual: NULL buffer");
    ssk_sim3_marks_call g;
    g.n_frames = n_pairs, g.rows = rows;
    g.idx = (const int32_t *)d_idx, g.idx12 = (const int32_t *)d_idx12, g.idx21 = (const int32_t *)d_idx21;
    g.nq = (const int32_t *)d_n_query, g.nt = (const int32_t *)d_n_train;
    g.idx_out = (int32_t *)d_idx_out, g.summary = (ss_sim3_mutual_summary *)d_summary;
    return sim3_marks_run(c, g, true);
}

int ss_sim3_marks_batch_device(ss_ctx *c, const int32_t *train_src, const void *d_idx, const void *d_skip, void *d_skip1_out, void *d_skip2_out)
{
    if (!c) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    if (!have_batch(c, "ss_sim3_marks_batch_device")) return SS_ERR_STATE;
    if (!d_idx || !d_skip1_out || !d_skip2_out) return fail(c, SS_ERR_INVALID_ARG, "sim3 marks: NULL buffer");
    batch_operands o;
    const int rc = batch_operands_of(c, "sim3 marks", train_src, o);
    if (rc != SS_OK) return rc;
    ssk_sim3_marks_call g;
    g.n_frames = o.n_frames, g.rows = o.kcap;
    g.idx = (const int32_t *)d_idx, g.q_skip = g.t_skip = (const uint8_t *)d_skip;
    g.nq = g.nt = o.n_kp, g.src = o.src, g.frame_error = o.frame_error;
    g.skip1 = (uint8_t *)d_skip1_out, g.skip2 = (uint8_t *)d_skip2_out;
    return sim3_marks_run(c, g, false);
}

int ss_sim3_mutual_batch_device(ss_ctx *c, const int32_t *train_src, const void *d_idx, const void *d_idx12, const void *d_idx21, void *d_idx_out,
                                void *d_summary)
{
    if (!c) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    if (!have_batch(c, "ss_sim3_mutual_batch_device")) return SS_ERR_STATE;
    if (!d_idx || !d_idx12 || !d_idx21 || !d_idx_out || !d_summary) return fail(c, SS_ERR_INVALID_ARG, "sim3 mutual: NULL buffer");
    batch_operands o;
    const int rc = batch_operands_of(c, "sim3 mutual", train_src, o);
    if (rc != SS_OK) return rc;
    ssk_sim3_marks_call g;
    g.n_frames = o.n_frames, g.rows = o.kcap;
    g.idx = (const int32_t *)d_idx, g.idx12 = (const int32_t *)d_idx12, g.idx21 = (const int32_t *)d_idx21;
    g.nq = g.nt = o.n_kp, g.src = o.src, g.frame_error = o.frame_error;
    g.idx_out = (int32_t *)d_idx_out, g.summary = (ss_sim3_mutual_summary *)d_summary;
    return sim3_marks_run(c, g, true);
}

/* ---- local bundle adjustment (csrc/ss_ba.hip, csrc/ss_ba_steps.h) ---- */
/* the message of the first rule p breaks, or NULL; needs no context */
static const char *ba_params_error(const ss_ba_params *p)
{
    if (!p) return "local BA: params is NULL";
    if (!(p->chi2_mono > 0.0) || !std::isfinite(p->chi2_mono)) return "local BA: chi2_mono must be finite and > 0";
    if (!(p->chi2_stereo > 0.0) || !std::isfinite(p->chi2_stereo)) return "local BA: chi2_stereo must be finite and > 0";
    if (!(p->lambda >= 0.0) || !std::isfinite(p->lambda)) return "local BA: lambda must be finite and >= 0";
    if (!(p->lambda_factor > 1.0) || !std::isfinite(p->lambda_factor)) return "local BA: lambda_factor must be finite and > 1";
    if (!(p->lambda_min >= 0.0) || !std::isfinite(p->lambda_min)) return "local BA: lambda_min must be finite and >= 0";
    if (!(p->step_eps >= 0.0) || !std::isfinite(p->step_eps)) return "local BA: step_eps must be finite and >= 0";
    if (p->n_rounds < 1 || p->n_rounds > SS_BA_MAX_ROUNDS) return "local BA: n_rounds must be 1 .. 4";
    for (int r = 0; r < p->n_rounds; r++)
        if (p->iterations[r] < 1 || p->iterations[r] > 32) return "local BA: iterations must be 1 .. 32 in every round";
    if (p->robust_rounds < 0 || p->robust_rounds > SS_BA_MAX_ROUNDS) return "local BA: robust_rounds must be 0 .. 4";
    if (p->min_point_obs < 1) return "local BA: min_point_obs must be >= 1";
    if (p->reserved[0] != 0 || p->reserved[1] != 0 || p->reserved[2] != 0 || p->reserved[3] != 0) return "local BA: the reserved fields must be 0";
    return nullptr;
}

/* the message of the rule the shape of problem q breaks (frames and blocks apart), or empty */
static std::string ba_problem_error(const ss_ba_problem &b, int q)
{
    const std::string head = "local BA: problem " + std::to_string(q) + ": ";
    if (b.n_kf < 1 || b.n_kf > SS_BA_MAX_KF) return head + "n_kf " + std::to_string(b.n_kf) + " outside 1 .. SS_BA_MAX_KF (" + std::to_string(SS_BA_MAX_KF) + ")";
    if (b.n_free < 1 || b.n_free > SS_BA_MAX_FREE)
        return head + "n_free " + std::to_string(b.n_free) + " outside 1 .. SS_BA_MAX_FREE (" + std::to_string(SS_BA_MAX_FREE) + ")";
    if (b.n_kf - b.n_free < 1) return head + "n_free " + std::to_string(b.n_free) + " of n_kf " + std::to_string(b.n_kf) + " leaves no fixed keyframe to hold the gauge";
    return std::string();
}

int ss_local_ba_host(const ss_proj_view *views, const double *start, int n_kf, int n_free, const float *scale, int n_levels, const ss_map_point *points,
                     const uint8_t *point_skip, int n_points, const ss_keypoint *kp, const float *right, const int32_t *n_kp, int rows_per_frame,
                     const int32_t *idx, const ss_ba_params *p, double *poses, double *xyz, uint8_t *point_flags, uint8_t *obs_flags, ss_ba_result *result)
{
    if (ba_params_error(p)) return SS_ERR_INVALID_ARG;
    const ss_ba_problem shape = {0, n_kf, n_free, 0};
    if (!ba_problem_error(shape, 0).empty()) return SS_ERR_INVALID_ARG;
    if (!views || !start || !scale || n_levels < 1 || n_levels > SS_MAX_LEVELS || n_points < 0 || rows_per_frame < 1 || !n_kp || !kp || !poses || !result)
        return SS_ERR_INVALID_ARG;
    if (n_points > 0 && (!points || !idx || !xyz || !point_flags || !obs_flags)) return SS_ERR_INVALID_ARG;
    const size_t P = (size_t)n_points;
    std::vector<ss_pose_cam> cam((size_t)n_kf);
    for (int k = 0; k < n_kf; k++) cam[(size_t)k] = ss_pose_cam_of(views[k], p->chi2_mono, p->chi2_stereo);
    std::vector<ss_ba_meas> meas((size_t)n_kf * P + 1);
    std::vector<double> X(P * 3 + 1);
    std::vector<uint8_t> obs((size_t)n_kf * P + 1), pflag(P + 1);
    /* step 1 */
    for (size_t i = 0; i < P; i++) {
        const ss_map_point &pt = points[i];
        const bool is_point = !(point_skip && point_skip[i] != 0) && ss_gn_is_finite((double)pt.x) && ss_gn_is_finite((double)pt.y) && ss_gn_is_finite((double)pt.z);
        pflag[i] = is_point ? 0 : 2;
        X[3 * i] = is_point ? (double)pt.x : 0.0, X[3 * i + 1] = is_point ? (double)pt.y : 0.0, X[3 * i + 2] = is_point ? (double)pt.z : 0.0;
        for (int k = 0; k < n_kf; k++) {
            const size_t o = (size_t)k * P + i;
            const int nk = std::min(std::max(n_kp[k], 0), rows_per_frame), krow = idx[o];
            ss_ba_meas m = {0.0f, 0.0f, -1.0f, 1.0f};
            obs[o] = 2;
            if (is_point && krow >= 0 && krow < nk) {
                const ss_keypoint &kk = kp[(size_t)k * rows_per_frame + krow];
                if (kk.octave >= 0 && kk.octave < n_levels) {
                    m.u = kk.x, m.v = kk.y, m.scale = scale[kk.octave];
                    m.ur = ss_pose_stored_right(p->check_right != 0, right != nullptr, right ? right[(size_t)k * rows_per_frame + krow] : 0.0f);
                    obs[o] = 0;
                }
            }
            meas[o] = m;
        }
    }
    ss_ba_problem_host(n_kf, n_free, n_points, cam.data(), start, meas.data(), *p, obs.data(), X.data(), pflag.data(), poses, result);
    for (size_t i = 0; i < P; i++) {
        point_flags[i] = pflag[i];
        for (int e = 0; e < 3; e++) xyz[3 * i + e] = pflag[i] == 2 ? 0.0 : X[3 * i + e];
    }
    for (size_t o = 0; o < (size_t)n_kf * P; o++) obs_flags[o] = obs[o];
    return SS_OK;
}

/* The checks the device forms share, the workspace, the host tables (start poses, views, problems, the frames' problems), then the
 * fixed schedule of a call whose device operands and outputs are filled in */
static int ba_run(ss_ctx *c, ssk_ba_call &g, int n_blocks, const ss_ba_problem *problems, const ss_proj_view *views, const double *start_poses,
                  const ss_ba_params *p)
{
    if (const char *msg = ba_params_error(p)) return fail(c, SS_ERR_INVALID_ARG, msg);
    if (g.n_frames < 0 || g.n_problems < 0 || n_blocks < 0 || g.point_rows < 1 || g.rows < 1)
        return fail(c, SS_ERR_INVALID_ARG, "local BA: bad frame, problem, block or row count");
    if (g.point_rows > SS_GUIDED_MAX_ROWS || g.rows > SS_GUIDED_MAX_ROWS)
        return fail(c, SS_ERR_INVALID_ARG, "local BA: point_rows " + std::to_string(g.point_rows) + " / rows_per_frame " + std::to_string(g.rows) +
                                               " exceed SS_GUIDED_MAX_ROWS (" + std::to_string(SS_GUIDED_MAX_ROWS) + ")");
    int rc = call_count_ok(c, "local BA", g.n_frames, "frames");
    if (rc == SS_OK) rc = context_pyramid(c, "local BA", &g.n_levels, g.scale);
    if (rc != SS_OK) return rc;
    if (g.n_frames == 0 || g.n_problems == 0) return SS_OK;
    if (!problems || !views || !start_poses) return fail(c, SS_ERR_INVALID_ARG, "local BA: problems, views or start_poses is NULL");
    std::vector<int32_t> frame_prob((size_t)g.n_frames, -1);
    g.max_kf = g.max_free = 0;
    for (int q = 0; q < g.n_problems; q++) {
        const ss_ba_problem &b = problems[q];
        const std::string msg = ba_problem_error(b, q);
        if (!msg.empty()) return fail(c, SS_ERR_INVALID_ARG, msg);
        const std::string head = "local BA: problem " + std::to_string(q) + ": ";
        if (b.first_frame < 0 || b.first_frame > g.n_frames - b.n_kf)
            return fail(c, SS_ERR_INVALID_ARG, head + "frames " + std::to_string(b.first_frame) + " .. + " + std::to_string(b.n_kf) + " lie outside the call's " +
                                                   std::to_string(g.n_frames));
        if (b.point_block < 0 || b.point_block >= n_blocks)
            return fail(c, SS_ERR_INVALID_ARG, head + "point_block " + std::to_string(b.point_block) + " names no block of points (" + std::to_string(n_blocks) + ")");
        for (int k = 0; k < b.n_kf; k++) {
            int32_t &owner = frame_prob[(size_t)(b.first_frame + k)];
            if (owner >= 0) return fail(c, SS_ERR_INVALID_ARG, head + "frame " + std::to_string(b.first_frame + k) + " belongs to problem " + std::to_string(owner) + " already");
            owner = q;
        }
        g.max_kf = std::max(g.max_kf, (int)b.n_kf), g.max_free = std::max(g.max_free, (int)b.n_free);
    }
    if (!g.points || !g.np || !g.kp || !g.nk || !g.idx || !g.out_pose || !g.out_xyz || !g.pflag || !g.obs || !g.result)
        return fail(c, SS_ERR_INVALID_ARG, "local BA: NULL buffer");
    g.p = *p;
    const size_t P = (size_t)g.point_rows, nf = (size_t)g.n_frames, nq = (size_t)g.n_problems, F = (size_t)g.max_free, K = (size_t)g.max_kf;
    const size_t pblocks = (P + SS_GN_SLOTS - 1) / SS_GN_SLOTS;
    rc = carve_from(c, c->d_ba_ws, [&](carve &w) {
        g.meas = w.take<ssk_ba_meas>(nf * P * sizeof(ssk_ba_meas));
        g.lin = w.take<uint8_t>(nf * P);
        g.pose = w.take<double>(2 * nf * 12 * sizeof(double));
        g.X = w.take<double>(2 * nq * P * 3 * sizeof(double));
        g.WY = w.take<double>(nq * F * 36 * P * sizeof(double));
        g.Lb = w.take<double>(nq * 9 * P * sizeof(double));
        g.solved = w.take<uint8_t>(nq * P);
        g.A = w.take<double>(nq * 36 * F * F * sizeof(double));
        g.r = w.take<double>(nq * 6 * F * sizeof(double));
        g.dc = w.take<double>(nq * 6 * F * sizeof(double));
        g.cost_k = w.take<double>(nq * K * sizeof(double));
        g.blk = w.take<int32_t>(nq * pblocks * 4 * sizeof(int32_t));
        g.st = w.take<ssk_ba_state>(nq * sizeof(ssk_ba_state));
    });
    if (rc != SS_OK) return rc;
    /* the host tables of the call: n_frames start poses, n_frames views, n_problems problems, n_frames problem numbers */
    const size_t sb = nf * 12 * sizeof(double), vb = nf * sizeof(ss_proj_view), pb = nq * sizeof(ss_ba_problem);
    rc = staged_upload(c, c->ba_tab, sb + vb + pb + nf * sizeof(int32_t), [&](uint8_t *h) {
        memcpy(h, start_poses, sb);
        memcpy(h + sb, views, vb);
        memcpy(h + sb + vb, problems, pb);
        memcpy(h + sb + vb + pb, frame_prob.data(), nf * sizeof(int32_t));
    });
    if (rc != SS_OK) return rc;
    g.start = c->ba_tab.as<double>();
    g.views = c->ba_tab.as<ss_proj_view>(sb);
    g.prob = c->ba_tab.as<ss_ba_problem>(sb + vb);
    g.frame_prob = c->ba_tab.as<int32_t>(sb + vb + pb);
    /* the stages' bytes: what a launch reads and writes when every slot is an observation of a free keyframe (an upper bound) */
    const int64_t nfP = (int64_t)(nf * P), nqP = (int64_t)(nq * P), iF = (int64_t)F, iK = (int64_t)K, iq = (int64_t)nq;
    {
        stage_timer t(c, "ba_gather", nfP * (4 + 16 + 1) + nqP * (32 + 1 + 48) + (g.p_skip ? nqP : 0));
        ssk_ba_gather(c->stream, g);
    }
    for (int r = 0; r < p->n_rounds; r++) {
        for (int it = -1; it < p->iterations[r]; it++) {
            if (it >= 0) {
                {
                    stage_timer t(c, "ba_points", nqP * (iK * 18 + 24 + iF * 288 + 72 + 2));
                    ssk_ba_points(c->stream, g, r);
                }
                {
                    stage_timer t(c, "ba_blocks", iq * (iF * (iF + 1) / 2) * (int64_t)P * (3 + 288) + iq * 36 * iF * iF * 8);
                    ssk_ba_blocks(c->stream, g, r);
                }
                {
                    stage_timer t(c, "ba_solve", iq * (36 * iF * iF * 8 + 6 * iF * 16 + iF * 192));
                    ssk_ba_solve(c->stream, g);
                }
                {
                    stage_timer t(c, "ba_update", nqP * (2 + 48 + 72 + iF * (1 + 144)));
                    ssk_ba_update(c->stream, g);
                }
            }
            {
                stage_timer t(c, "ba_cost", iq * iK * (int64_t)P * (2 + 16 + 24) + iq * iK * 8);
                ssk_ba_cost(c->stream, g, r, it >= 0 ? 1 : 0);
            }
            {
                stage_timer t(c, "ba_accept", iq * (iK * 8 + (int64_t)sizeof(ssk_ba_state)));
                ssk_ba_accept(c->stream, g, r, it >= 0 ? 0 : 1);
            }
        }
        stage_timer t(c, "ba_classify", nqP * (1 + iK * 17 + 24));
        ssk_ba_classify(c->stream, g);
    }
    {
        stage_timer t(c, "ba_finish", nqP * (1 + 48 + iK) + (int64_t)nf * 96 + iq * (int64_t)sizeof(ss_ba_result));
        ssk_ba_finish(c->stream, g);
    }
    HIP_TRY(c, hipGetLastError());
    return SS_OK;
}

int ss_local_ba_pairs_device(ss_ctx *c, const void *d_points, const void *d_point_skip, const void *d_n_points, int n_blocks, int point_rows,
                             const void *d_kp, const void *d_right, const void *d_n_kp, int n_frames, int rows_per_frame, const void *d_idx,
                             const ss_ba_problem *problems, int n_problems, const ss_proj_view *views, const double *start_poses, const ss_ba_params *p,
                             void *d_poses, void *d_xyz, void *d_point_flags, void *d_obs_flags, void *d_result)
{
    if (!c) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    ssk_ba_call g;
    g.n_frames = n_frames, g.n_problems = n_problems, g.point_rows = point_rows, g.rows = rows_per_frame;
    g.points = (const ss_map_point *)d_points, g.p_skip = (const uint8_t *)d_point_skip, g.np = (const int32_t *)d_n_points;
    g.kp = (const ss_keypoint *)d_kp, g.right = (const float *)d_right, g.nk = (const int32_t *)d_n_kp;
    g.idx = (const int32_t *)d_idx;
    g.out_pose = (double *)d_poses, g.out_xyz = (double *)d_xyz, g.pflag = (uint8_t *)d_point_flags, g.obs = (uint8_t *)d_obs_flags;
    g.result = (ss_ba_result *)d_result;
    return ba_run(c, g, n_blocks, problems, views, start_poses, p);
}

int ss_local_ba_batch_device(ss_ctx *c, const void *d_points, const void *d_point_skip, const void *d_n_points, int n_blocks, int point_rows,
                             const void *d_right, const void *d_idx, const ss_ba_problem *problems, int n_problems, const ss_proj_view *views,
                             const double *start_poses, const ss_ba_params *p, void *d_poses, void *d_xyz, void *d_point_flags, void *d_obs_flags,
                             void *d_result)
{
    if (!c) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    if (!have_batch(c, "ss_local_ba_batch_device")) return SS_ERR_STATE;
    ssk_ba_call g;
    g.n_frames = c->last_n_frames, g.n_problems = n_problems, g.point_rows = point_rows, g.rows = c->hg.kcap;
    g.points = (const ss_map_point *)d_points, g.p_skip = (const uint8_t *)d_point_skip, g.np = (const int32_t *)d_n_points;
    g.kp = c->ws.kps, g.right = (const float *)d_right, g.nk = c->ws.n_kp;
    const int rc = flagged_frame_error(c, c->batch_test_flagged, &g.frame_error);
    if (rc != SS_OK) return rc;
    g.idx = (const int32_t *)d_idx;
    g.out_pose = (double *)d_poses, g.out_xyz = (double *)d_xyz, g.pflag = (uint8_t *)d_point_flags, g.obs = (uint8_t *)d_obs_flags;
    g.result = (ss_ba_result *)d_result;
    return ba_run(c, g, n_blocks, problems, views, start_poses, p);
}

int ss_local_ba(ss_ctx *c, const ss_proj_view *views, const double *start, int n_kf, int n_free, const ss_map_point *points, const uint8_t *point_skip,
                int n_points, const ss_keypoint *kp, const float *right, const int32_t *n_kp, int rows_per_frame, const int32_t *idx, const ss_ba_params *p,
                double *poses, double *xyz, uint8_t *point_flags, uint8_t *obs_flags, ss_ba_result *result)
{
    if (!c) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    if (const char *msg = ba_params_error(p)) return fail(c, SS_ERR_INVALID_ARG, msg);
    const ss_ba_problem problem = {0, n_kf, n_free, 0};
    const std::string msg = ba_problem_error(problem, 0);
    if (!msg.empty()) return fail(c, SS_ERR_INVALID_ARG, msg);
    if (n_points < 0 || n_points > SS_GUIDED_MAX_ROWS || rows_per_frame < 1 || rows_per_frame > SS_GUIDED_MAX_ROWS)
        return fail(c, SS_ERR_INVALID_ARG, "local BA: n_points must be 0 .. SS_GUIDED_MAX_ROWS and rows_per_frame 1 .. SS_GUIDED_MAX_ROWS");
    if (!views || !start || !kp || !n_kp || !poses || !result || (n_points > 0 && (!points || !idx || !xyz || !point_flags || !obs_flags)))
        return fail(c, SS_ERR_INVALID_ARG, "local BA: NULL buffer");
    /* one block of `pr` points, n_kf frames of rows_per_frame rows; `count` is on this stack: no return before the stream has read it */
    const size_t pr = (size_t)std::max(n_points, 1), np = (size_t)n_points, kf = (size_t)n_kf, kr = kf * (size_t)rows_per_frame;
    const int32_t count[1] = {n_points};
    enum { PT, PS, NP, KP, RT, NK, IDX, POSE, XYZ, PF, OF, RES, PIECES };
    io_piece io[PIECES] = {{points, nullptr, pr * sizeof(ss_map_point), np * sizeof(ss_map_point)},
                           {point_skip, nullptr, pr, np},
                           {count, nullptr, sizeof(count), sizeof(count)},
                           {kp, nullptr, kr * sizeof(ss_keypoint), kr * sizeof(ss_keypoint)},
                           {right, nullptr, kr * 4, kr * 4},
                           {n_kp, nullptr, kf * 4, kf * 4},
                           {idx, nullptr, kf * pr * 4, kf * np * 4},
                           {nullptr, poses, kf * 12 * sizeof(double), kf * 12 * sizeof(double)},
                           {nullptr, xyz, pr * 3 * sizeof(double), np * 3 * sizeof(double)},
                           {nullptr, point_flags, pr, np},
                           {nullptr, obs_flags, kf * pr, kf * np},
                           {nullptr, result, sizeof(ss_ba_result), sizeof(ss_ba_result)}};
    int rc = io_send(c, c->d_ba_io, io, PIECES);
    if (rc == SS_OK)
        rc = ss_local_ba_pairs_device(c, io[PT].d, point_skip ? io[PS].d : nullptr, io[NP].d, 1, (int)pr, io[KP].d, right ? io[RT].d : nullptr, io[NK].d, n_kf,
                                      rows_per_frame, io[IDX].d, &problem, 1, views, start, p, io[POSE].d, io[XYZ].d, io[PF].d, io[OF].d, io[RES].d);
    if (rc != SS_OK) {
        (void)hipStreamSynchronize(c->stream);
        return rc;
    }
    return io_fetch(c, io, PIECES);
}

int ss_local_ba_points_to_block(ss_ctx *c, const void *d_xyz, const void *d_point_flags, int n_problems, int point_rows, const int32_t *block_of,
                                void *d_points, int n_blocks)
{
    if (!c) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    if (n_problems < 0 || n_blocks < 0 || point_rows < 1 || point_rows > SS_GUIDED_MAX_ROWS)
        return fail(c, SS_ERR_INVALID_ARG, "local BA points: bad problem, block or row count");
    const int rc0 = call_count_ok(c, "local BA points", n_problems, "problems");
    if (rc0 != SS_OK) return rc0;
    for (int q = 0; q < n_problems; q++) {
        const int b = block_of ? block_of[q] : q;
        if (b < 0 || b >= n_blocks)
            return fail(c, SS_ERR_INVALID_ARG, std::string(block_of ? "block_of[" : "problem [") + std::to_string(q) + "] = " + std::to_string(b) +
                                                   " names no block of points (" + std::to_string(n_blocks) + ")");
    }
    if (n_problems == 0) return SS_OK;
    if (!d_xyz || !d_point_flags || !d_points) return fail(c, SS_ERR_INVALID_ARG, "local BA points: NULL buffer");
    const int rc = staged_upload(c, c->ba_block_tab, (size_t)n_problems * sizeof(int32_t), [&](uint8_t *h) {
        int32_t *t = (int32_t *)h;
        for (int q = 0; q < n_problems; q++) t[q] = block_of ? block_of[q] : q;
    });
    if (rc != SS_OK) return rc;
    ssk_ba_block_call g;
    g.n = n_problems, g.point_rows = point_rows;
    g.xyz = (const double *)d_xyz, g.flags = (const uint8_t *)d_point_flags, g.block_of = c->ba_block_tab.as<int32_t>();
    g.points = (ss_map_point *)d_points;
    {
        stage_timer t(c, "ba_points_to_block", (int64_t)n_problems * point_rows * (1 + 24 + 12));
        ssk_ba_points_to_block(c->stream, g);
    }
    HIP_TRY(c, hipGetLastError());
    return SS_OK;
}

/* ---- essential-graph optimisation (csrc/ss_graph.hip, csrc/ss_graph_steps.h) ---- */
/* the message of the first rule p breaks, or NULL; needs no context */
static const char *graph_params_error(const ss_graph_params *p)
{
    if (!p) return "pose graph: params is NULL";
    if (!(p->lambda >= 0.0) || !std::isfinite(p->lambda)) return "pose graph: lambda must be finite and >= 0";
    if (!(p->lambda_factor > 1.0) || !std::isfinite(p->lambda_factor)) return "pose graph: lambda_factor must be finite and > 1";
    if (!(p->lambda_min >= 0.0) || !std::isfinite(p->lambda_min)) return "pose graph: lambda_min must be finite and >= 0";
    if (!(p->pcg_tol >= 0.0) || !std::isfinite(p->pcg_tol)) return "pose graph: pcg_tol must be finite and >= 0";
    if (p->iterations < 1 || p->iterations > 64) return "pose graph: iterations must be 1 .. 64";
    if (p->pcg_iterations < 1 || p->pcg_iterations > 4096) return "pose graph: pcg_iterations must be 1 .. 4096";
    if (p->reserved != 0) return "pose graph: the reserved field must be 0";
    return nullptr;
}

/* the message of the rule problem q of a call of n_kf keyframes and n_edges edges breaks (overlaps apart), or empty */
static std::string graph_problem_error(const ss_graph_problem &b, int q, int n_kf, int n_edges, const int32_t *edges)
{
    const std::string head = "pose graph: problem " + std::to_string(q) + ": ";
    if (b.n_kf < 1 || b.n_kf > SS_GRAPH_MAX_KF)
        return head + "n_kf " + std::to_string(b.n_kf) + " outside 1 .. SS_GRAPH_MAX_KF (" + std::to_string(SS_GRAPH_MAX_KF) + ")";
    if (b.n_edges < 0 || b.n_edges > SS_GRAPH_MAX_EDGES)
        return head + "n_edges " + std::to_string(b.n_edges) + " outside 0 .. SS_GRAPH_MAX_EDGES (" + std::to_string(SS_GRAPH_MAX_EDGES) + ")";
    if (b.first_kf < 0 || b.first_kf > n_kf - b.n_kf)
        return head + "keyframes " + std::to_string(b.first_kf) + " .. + " + std::to_string(b.n_kf) + " lie outside the call's " + std::to_string(n_kf);
    if (b.first_edge < 0 || b.first_edge > n_edges - b.n_edges)
        return head + "edges " + std::to_string(b.first_edge) + " .. + " + std::to_string(b.n_edges) + " lie outside the call's " + std::to_string(n_edges);
    for (int e = b.first_edge; e < b.first_edge + b.n_edges; e++) {
        const int i = edges[2 * (size_t)e], j = edges[2 * (size_t)e + 1];
        if (i < b.first_kf || i >= b.first_kf + b.n_kf || j < b.first_kf || j >= b.first_kf + b.n_kf)
            return head + "edge " + std::to_string(e) + " (" + std::to_string(i) + ", " + std::to_string(j) + ") names a keyframe outside the problem";
        if (i == j) return head + "edge " + std::to_string(e) + " joins keyframe " + std::to_string(i) + " to itself";
    }
    return std::string();
}

int ss_graph_atan2_host(const double *y, const double *x, int n, double *out)
{
    if (n < 0 || (n > 0 && (!y || !x || !out))) return SS_ERR_INVALID_ARG;
    for (int k = 0; k < n; k++) out[k] = ss_graph_atan2(y[k], x[k]);
    return SS_OK;
}

int ss_graph_ln_host(const double *x, int n, double *out)
{
    if (n < 0 || (n > 0 && (!x || !out))) return SS_ERR_INVALID_ARG;
    for (int k = 0; k < n; k++) out[k] = ss_graph_ln(x[k]);
    return SS_OK;
}

int ss_pose_graph_edge_host(const double *nc_i, const double *nc_j, const double *s_i, const double *s_j, int fixed_i, int fixed_j, int fix_scale, double *e,
                            double *J)
{
    if (!nc_i || !nc_j || !s_i || !s_j || !e || !J) return SS_ERR_INVALID_ARG;
    double M[SS_GRAPH_SIM3];
    ss_graph_measure(nc_i, nc_j, M);
    ss_graph_error(M, s_i, s_j, e);
    const bool fix = fix_scale != 0;
    for (int c = 0; c < 14; c++) ss_graph_column(M, s_i, s_j, c / 7, c % 7, fix, (c < 7 ? fixed_i : fixed_j) != 0 || (fix && c % 7 == 6), J + 7 * c);
    return SS_OK;
}

int ss_pose_graph_host(const double *nc, const double *start, const uint8_t *fixed, int n_kf, const int32_t *edges, int n_edges, const ss_graph_params *p,
                       double *sim3, double *poses, ss_graph_result *result)
{
    if (graph_params_error(p)) return SS_ERR_INVALID_ARG;
    if (!nc || !start || !fixed || !sim3 || !poses || !result || n_edges < 0 || (n_edges > 0 && !edges)) return SS_ERR_INVALID_ARG;
    const ss_graph_problem shape = {0, n_kf, 0, n_edges};
    if (!graph_problem_error(shape, 0, n_kf, n_edges, edges).empty()) return SS_ERR_INVALID_ARG;
    try {
        ss_graph_problem_host(n_kf, n_edges, nc, start, fixed, edges, *p, sim3, result);
    } catch (const std::bad_alloc &) { /* its workspace grows with the caller's counts */
        return SS_ERR_NO_MEMORY;
    }
    for (int v = 0; v < n_kf; v++) ss_graph_pose(sim3 + 13 * (size_t)v, poses + 12 * (size_t)v);
    return SS_OK;
}

/* the checks, the tables and the schedule of ss_pose_graph_device; its host tables grow with the caller's counts and may throw */
static int graph_run(ss_ctx *c, const void *d_nc, const void *d_start, const void *d_fixed, int n_kf, const ss_graph_problem *problems, int n_problems,
                     const int32_t *edges, int n_edges, const ss_graph_params *p, void *d_sim3, void *d_poses, void *d_result)
{
    if (const char *msg = graph_params_error(p)) return fail(c, SS_ERR_INVALID_ARG, msg);
    if (n_kf < 0 || n_problems < 0 || n_edges < 0) return fail(c, SS_ERR_INVALID_ARG, "pose graph: bad keyframe, problem or edge count");
    const int rc0 = call_count_ok(c, "pose graph", n_problems, "problems");
    if (rc0 != SS_OK) return rc0;
    if (n_kf == 0) return SS_OK;
    if ((n_problems > 0 && !problems) || (n_edges > 0 && !edges)) return fail(c, SS_ERR_INVALID_ARG, "pose graph: problems or edges is NULL");
    ssk_graph_call g;
    g.n_kf = n_kf, g.n_problems = n_problems, g.n_edges = n_edges;
    std::vector<int32_t> kf_prob((size_t)n_kf, -1), edge_prob((size_t)n_edges, -1), off((size_t)n_kf, 0), cnt((size_t)n_kf, 0), inc(2 * (size_t)n_edges + 1);
    int inc_at = 0;
    for (int q = 0; q < n_problems; q++) {
        const ss_graph_problem &b = problems[q];
        const std::string msg = graph_problem_error(b, q, n_kf, n_edges, edges);
        if (!msg.empty()) return fail(c, SS_ERR_INVALID_ARG, msg);
        const std::string head = "pose graph: problem " + std::to_string(q) + ": ";
        for (int k = b.first_kf; k < b.first_kf + b.n_kf; k++) {
            if (kf_prob[(size_t)k] >= 0)
                return fail(c, SS_ERR_INVALID_ARG, head + "keyframe " + std::to_string(k) + " belongs to problem " + std::to_string(kf_prob[(size_t)k]) + " already");
            kf_prob[(size_t)k] = q;
        }
        for (int e = b.first_edge; e < b.first_edge + b.n_edges; e++) {
            if (edge_prob[(size_t)e] >= 0)
                return fail(c, SS_ERR_INVALID_ARG, head + "edge " + std::to_string(e) + " belongs to problem " + std::to_string(edge_prob[(size_t)e]) + " already");
            edge_prob[(size_t)e] = q;
        }
        /* the problem's incidence lists in the call's numbers: its run of inc starts at inc_at */
        std::vector<int32_t> local(2 * (size_t)b.n_edges + 1), l_off((size_t)b.n_kf), l_cnt((size_t)b.n_kf), l_inc(2 * (size_t)b.n_edges + 1);
        for (int e = 0; e < 2 * b.n_edges; e++) local[(size_t)e] = edges[2 * (size_t)b.first_edge + e] - b.first_kf;
        ss_graph_incidence(b.n_kf, b.n_edges, local.data(), l_off.data(), l_cnt.data(), l_inc.data());
        for (int k = 0; k < b.n_kf; k++) off[(size_t)(b.first_kf + k)] = inc_at + l_off[(size_t)k], cnt[(size_t)(b.first_kf + k)] = l_cnt[(size_t)k];
        for (int m = 0; m < 2 * b.n_edges; m++) inc[(size_t)(inc_at + m)] = l_inc[(size_t)m] + 2 * b.first_edge;
        inc_at += 2 * b.n_edges;
        g.max_kf = std::max(g.max_kf, (int)b.n_kf), g.max_edges = std::max(g.max_edges, (int)b.n_edges);
    }
    if (!d_nc || !d_start || !d_fixed || !d_sim3 || !d_poses || (n_problems > 0 && !d_result)) return fail(c, SS_ERR_INVALID_ARG, "pose graph: NULL buffer");
    g.nc = (const double *)d_nc, g.start = (const double *)d_start, g.fixed = (const uint8_t *)d_fixed;
    g.out_sim3 = (double *)d_sim3, g.out_pose = (double *)d_poses, g.result = (ss_graph_result *)d_result;
    g.p = *p;
    const size_t K = (size_t)n_kf, E = (size_t)n_edges, nq = (size_t)n_problems;
    int rc = carve_from(c, c->d_graph_ws, [&](carve &w) {
        g.S = w.take<double>(2 * K * 13 * sizeof(double));
        g.M = w.take<double>(E * 13 * sizeof(double));
        g.err = w.take<double>(E * 7 * sizeof(double));
        g.J = w.take<double>(E * 98 * sizeof(double));
        g.u = w.take<double>(E * 7 * sizeof(double));
        g.L = w.take<double>(K * 49 * sizeof(double));
        g.dd = w.take<double>(K * 7 * sizeof(double));
        g.g = w.take<double>(K * 7 * sizeof(double));
        g.x = w.take<double>(K * 7 * sizeof(double));
        g.r = w.take<double>(K * 7 * sizeof(double));
        g.z = w.take<double>(K * 7 * sizeof(double));
        g.pv = w.take<double>(K * 7 * sizeof(double));
        g.q = w.take<double>(K * 7 * sizeof(double));
        g.flag = w.take<uint8_t>(K);
        g.st = w.take<ssk_graph_state>(nq * sizeof(ssk_graph_state));
    });
    if (rc != SS_OK) return rc;
    /* the host tables of the call: the problems, the edges, the keyframes' problems, the incidence lists */
    const size_t pb = (nq * sizeof(ss_graph_problem) + 15) & ~(size_t)15, eb = E * 8, kb = K * 4, ib = 2 * E * 4;
    rc = staged_upload(c, c->graph_tab, pb + eb + 3 * kb + ib + 16, [&](uint8_t *h) {
        if (nq) memcpy(h, problems, nq * sizeof(ss_graph_problem));
        if (E) memcpy(h + pb, edges, eb);
        memcpy(h + pb + eb, kf_prob.data(), kb);
        memcpy(h + pb + eb + kb, off.data(), kb);
        memcpy(h + pb + eb + 2 * kb, cnt.data(), kb);
        if (E) memcpy(h + pb + eb + 3 * kb, inc.data(), ib);
    });
    if (rc != SS_OK) return rc;
    g.prob = c->graph_tab.as<ss_graph_problem>();
    g.edges = c->graph_tab.as<int32_t>(pb);
    g.kf_prob = c->graph_tab.as<int32_t>(pb + eb);
    g.inc_off = c->graph_tab.as<int32_t>(pb + eb + kb);
    g.inc_cnt = c->graph_tab.as<int32_t>(pb + eb + 2 * kb);
    g.inc = c->graph_tab.as<int32_t>(pb + eb + 3 * kb);
    /* the stages' bytes: what a launch reads and writes when every problem runs (an upper bound) */
    const int64_t iK = (int64_t)K, iE = (int64_t)E, iq = (int64_t)nq;
    {
        stage_timer t(c, "graph_gather", iK * (2 * 104 + 2 * 104 + 2) + iE * (8 + 3 * 104) + iq * (int64_t)sizeof(ssk_graph_state));
        ssk_graph_gather(c->stream, g);
    }
    if (n_problems > 0 && g.max_edges > 0) {
        for (int it = -1; it < p->iterations; it++) {
            if (it >= 0) {
                {
                    stage_timer t(c, "graph_lin", iE * 16 * (8 + 3 * 104) + iE * (56 + 784));
                    ssk_graph_lin(c->stream, g);
                }
                {
                    stage_timer t(c, "graph_blocks", 2 * iE * (4 + 392 + 56) + iK * (392 + 112 + 1));
                    ssk_graph_blocks(c->stream, g);
                }
                {
                    stage_timer t(c, "graph_solve", (int64_t)p->pcg_iterations * (iE * (784 + 112 + 56 + 2 * (392 + 56 + 4)) + iK * (392 + 10 * 56)) + iK * (2 * 104 + 56));
                    ssk_graph_solve(c->stream, g);
                }
            }
            stage_timer t(c, "graph_cost", iE * (8 + 3 * 104) + iq * (int64_t)sizeof(ssk_graph_state));
            ssk_graph_cost(c->stream, g, it >= 0 ? 0 : 1);
        }
    }
    {
        stage_timer t(c, "graph_finish", iK * (4 + 104 + 104 + 96) + iq * (int64_t)(sizeof(ssk_graph_state) + sizeof(ss_graph_result)));
        ssk_graph_finish(c->stream, g);
    }
    HIP_TRY(c, hipGetLastError());
    return SS_OK;
}

int ss_pose_graph_device(ss_ctx *c, const void *d_nc, const void *d_start, const void *d_fixed, int n_kf, const ss_graph_problem *problems, int n_problems,
                         const int32_t *edges, int n_edges, const ss_graph_params *p, void *d_sim3, void *d_poses, void *d_result)
{
    if (!c) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    try {
        return graph_run(c, d_nc, d_start, d_fixed, n_kf, problems, n_problems, edges, n_edges, p, d_sim3, d_poses, d_result);
    } catch (const std::bad_alloc &) {
        return fail(c, SS_ERR_NO_MEMORY, "pose graph: no host memory for the tables of the call");
    }
}

int ss_pose_graph(ss_ctx *c, const double *nc, const double *start, const uint8_t *fixed, int n_kf, const int32_t *edges, int n_edges, const ss_graph_params *p,
                  double *sim3, double *poses, ss_graph_result *result)
{
    if (!c) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    if (const char *msg = graph_params_error(p)) return fail(c, SS_ERR_INVALID_ARG, msg);
    if (!nc || !start || !fixed || !sim3 || !poses || !result || n_edges < 0 || (n_edges > 0 && !edges)) return fail(c, SS_ERR_INVALID_ARG, "pose graph: NULL buffer");
    const ss_graph_problem problem = {0, n_kf, 0, n_edges};
    const std::string msg = graph_problem_error(problem, 0, n_kf, n_edges, edges);
    if (!msg.empty()) return fail(c, SS_ERR_INVALID_ARG, msg);
    const size_t K = (size_t)n_kf;
    enum { NC, ST, FX, S3, PO, RES, PIECES };
    io_piece io[PIECES] = {{nc, nullptr, K * 104, K * 104},      {start, nullptr, K * 104, K * 104}, {fixed, nullptr, K, K},
                           {nullptr, sim3, K * 104, K * 104},    {nullptr, poses, K * 96, K * 96},   {nullptr, result, sizeof(ss_graph_result), sizeof(ss_graph_result)}};
    int rc = io_send(c, c->d_graph_io, io, PIECES);
    if (rc == SS_OK) rc = ss_pose_graph_device(c, io[NC].d, io[ST].d, io[FX].d, n_kf, &problem, 1, edges, n_edges, p, io[S3].d, io[PO].d, io[RES].d);
    if (rc != SS_OK) {
        (void)hipStreamSynchronize(c->stream);
        return rc;
    }
    return io_fetch(c, io, PIECES);
}

int ss_pose_graph_points_device(ss_ctx *c, void *d_points, const void *d_ref, int n_blocks, int point_rows, const void *d_nc, const void *d_sim3, int n_kf)
{
    if (!c) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    if (n_blocks < 0 || n_kf < 0 || point_rows < 1 || point_rows > SS_GUIDED_MAX_ROWS)
        return fail(c, SS_ERR_INVALID_ARG, "pose graph points: bad block, row or keyframe count");
    const int rc0 = call_count_ok(c, "pose graph points", n_blocks, "blocks");
    if (rc0 != SS_OK) return rc0;
    if (n_blocks == 0 || n_kf == 0) return SS_OK;
    if (!d_points || !d_ref || !d_nc || !d_sim3) return fail(c, SS_ERR_INVALID_ARG, "pose graph points: NULL buffer");
    ssk_graph_points_call g;
    g.n_blocks = n_blocks, g.point_rows = point_rows, g.n_kf = n_kf;
    g.points = (ss_map_point *)d_points, g.ref = (const int32_t *)d_ref, g.nc = (const double *)d_nc, g.sim3 = (const double *)d_sim3;
    {
        stage_timer t(c, "graph_points", (int64_t)n_blocks * point_rows * (4 + 24 + 208));
        ssk_graph_points(c->stream, g);
    }
    HIP_TRY(c, hipGetLastError());
    return SS_OK;
}

/* ---- global bundle adjustment (csrc/ss_gba.hip, csrc/ss_gba_steps.h) ---- */
/* the message of the first rule p breaks, or NULL; needs no context */
static const char *gba_params_error(const ss_gba_params *p)
{
    if (!p) return "global BA: params is NULL";
    if (!(p->chi2_mono > 0.0) || !std::isfinite(p->chi2_mono)) return "global BA: chi2_mono must be finite and > 0";
    if (!(p->chi2_stereo > 0.0) || !std::isfinite(p->chi2_stereo)) return "global BA: chi2_stereo must be finite and > 0";
    if (!(p->lambda >= 0.0) || !std::isfinite(p->lambda)) return "global BA: lambda must be finite and >= 0";
    if (!(p->lambda_factor > 1.0) || !std::isfinite(p->lambda_factor)) return "global BA: lambda_factor must be finite and > 1";
    if (!(p->lambda_min >= 0.0) || !std::isfinite(p->lambda_min)) return "global BA: lambda_min must be finite and >= 0";
    if (!(p->step_eps >= 0.0) || !std::isfinite(p->step_eps)) return "global BA: step_eps must be finite and >= 0";
    if (!(p->pcg_tol >= 0.0) || !std::isfinite(p->pcg_tol)) return "global BA: pcg_tol must be finite and >= 0";
    if (p->n_rounds < 1 || p->n_rounds > SS_BA_MAX_ROUNDS) return "global BA: n_rounds must be 1 .. 4";
    for (int r = 0; r < p->n_rounds; r++)
        if (p->iterations[r] < 1 || p->iterations[r] > 32) return "global BA: iterations must be 1 .. 32 in every round";
    if (p->robust_rounds < 0 || p->robust_rounds > SS_BA_MAX_ROUNDS) return "global BA: robust_rounds must be 0 .. 4";
    if (p->min_point_obs < 1) return "global BA: min_point_obs must be >= 1";
    if (p->pcg_iterations < 1 || p->pcg_iterations > 256) return "global BA: pcg_iterations must be 1 .. 256";
    if (p->reserved[0] != 0 || p->reserved[1] != 0 || p->reserved[2] != 0) return "global BA: the reserved fields must be 0";
    return nullptr;
}

/* the host tables of a call: what the kernels read besides the caller's device arrays */
struct gba_host_tables {
    std::vector<int32_t> kf_prob, blk_prob, pt_off, pt_cnt, kf_off, kf_cnt, kf_list;
    std::vector<ss_gba_rec> rec;
    int max_kf = 0;
};

/* The shapes and ranges of the problems of a call (`what` heads the messages): the keyframes' and the blocks' problems into kf_prob and
 * blk_prob, the largest n_kf into *max_kf.  The message of the first rule that is broken, or empty */
static std::string problem_ranges(const std::string &what, int n_kf, int n_blocks, int point_rows, const ss_gba_problem *problems, int n_problems, int n_obs,
                                  std::vector<int32_t> &kf_prob, std::vector<int32_t> &blk_prob, int *max_kf)
{
    kf_prob.assign((size_t)n_kf, -1), blk_prob.assign((size_t)n_blocks, -1);
    std::vector<int32_t> rec_prob((size_t)n_obs, -1);
    for (int q = 0; q < n_problems; q++) {
        const ss_gba_problem &b = problems[q];
        const std::string head = what + ": problem " + std::to_string(q) + ": ";
        if (b.n_kf < 1 || b.n_kf > SS_GBA_MAX_KF) return head + "n_kf " + std::to_string(b.n_kf) + " outside 1 .. SS_GBA_MAX_KF (" + std::to_string(SS_GBA_MAX_KF) + ")";
        if (b.n_blocks < 0 || (int64_t)b.n_blocks * point_rows > SS_GBA_MAX_POINTS)
            return head + "n_blocks " + std::to_string(b.n_blocks) + " of " + std::to_string(point_rows) + " rows outside 0 .. SS_GBA_MAX_POINTS (" +
                   std::to_string(SS_GBA_MAX_POINTS) + ") points";
        if (b.n_obs < 0 || b.n_obs > SS_GBA_MAX_OBS) return head + "n_obs " + std::to_string(b.n_obs) + " outside 0 .. SS_GBA_MAX_OBS (" + std::to_string(SS_GBA_MAX_OBS) + ")";
        if (b.reserved[0] != 0 || b.reserved[1] != 0) return head + "the reserved fields must be 0";
        if (b.first_kf < 0 || b.first_kf > n_kf - b.n_kf)
            return head + "keyframes " + std::to_string(b.first_kf) + " .. + " + std::to_string(b.n_kf) + " lie outside the call's " + std::to_string(n_kf);
        if (b.first_block < 0 || b.first_block > n_blocks - b.n_blocks)
            return head + "blocks " + std::to_string(b.first_block) + " .. + " + std::to_string(b.n_blocks) + " lie outside the call's " + std::to_string(n_blocks);
        if (b.first_obs < 0 || b.first_obs > n_obs - b.n_obs)
            return head + "records " + std::to_string(b.first_obs) + " .. + " + std::to_string(b.n_obs) + " lie outside the call's " + std::to_string(n_obs);
        for (int k = b.first_kf; k < b.first_kf + b.n_kf; k++) {
            if (kf_prob[(size_t)k] >= 0) return head + "keyframe " + std::to_string(k) + " belongs to problem " + std::to_string(kf_prob[(size_t)k]) + " already";
            kf_prob[(size_t)k] = q;
        }
        for (int k = b.first_block; k < b.first_block + b.n_blocks; k++) {
            if (blk_prob[(size_t)k] >= 0) return head + "block " + std::to_string(k) + " belongs to problem " + std::to_string(blk_prob[(size_t)k]) + " already";
            blk_prob[(size_t)k] = q;
        }
        for (int m = b.first_obs; m < b.first_obs + b.n_obs; m++) {
            if (rec_prob[(size_t)m] >= 0) return head + "record " + std::to_string(m) + " belongs to problem " + std::to_string(rec_prob[(size_t)m]) + " already";
            rec_prob[(size_t)m] = q;
        }
        *max_kf = std::max(*max_kf, (int)b.n_kf);
    }
    return std::string();
}

/* The shapes and ranges of the problems of a call, then the records of each sorted and both its incidence lists into t.  The message
 * of the first rule that is broken, or empty.  May throw std::bad_alloc: the tables grow with the caller's counts */
static std::string gba_build(int n_kf, int n_blocks, int point_rows, const ss_gba_problem *problems, int n_problems, const ss_gba_obs *obs, int n_obs,
                             const float *scale, int n_levels, bool check_right, gba_host_tables &t)
{
    const size_t NP = (size_t)n_blocks * point_rows;
    t.pt_off.assign(NP, 0), t.pt_cnt.assign(NP, 0), t.kf_off.assign((size_t)n_kf, 0), t.kf_cnt.assign((size_t)n_kf, 0);
    t.kf_list.assign((size_t)n_obs, 0);
    t.rec.resize((size_t)n_obs);
    for (int m = 0; m < n_obs; m++) t.rec[(size_t)m] = ss_gba_rec{-1, -1, 0.0f, 0.0f, -1.0f, 1.0f, m, 0};
    const std::string ranges = problem_ranges("global BA", n_kf, n_blocks, point_rows, problems, n_problems, n_obs, t.kf_prob, t.blk_prob, &t.max_kf);
    if (!ranges.empty()) return ranges;
    /* the ranges stand: now the records of every problem */
    for (int q = 0; q < n_problems; q++) {
        const ss_gba_problem &b = problems[q];
        const std::string head = "global BA: problem " + std::to_string(q) + ": ";
        if (b.n_obs > 0 && !obs) return "global BA: obs is NULL";
        const int P = b.n_blocks * point_rows;
        const size_t p0 = (size_t)b.first_block * point_rows;
        int bad = 0;
        const int why = ss_gba_tables(b.n_kf, P, obs + b.first_obs, b.n_obs, scale, n_levels, check_right, b.first_obs, t.rec.data() + b.first_obs, t.pt_off.data() + p0,
                                      t.pt_cnt.data() + p0, t.kf_off.data() + b.first_kf, t.kf_cnt.data() + b.first_kf, t.kf_list.data() + b.first_obs, &bad);
        if (why != 0) {
            const ss_gba_obs &o = obs[b.first_obs + bad];
            const std::string rec = head + "record " + std::to_string(b.first_obs + bad) + ": ";
            if (why == 1) return rec + "kf " + std::to_string(o.kf) + " outside 0 .. " + std::to_string(b.n_kf - 1);
            if (why == 2) return rec + "point " + std::to_string(o.point) + " outside 0 .. " + std::to_string(P - 1);
            return rec + "the pair (kf " + std::to_string(o.kf) + ", point " + std::to_string(o.point) + ") has a record already";
        }
    }
    return std::string();
}

static int gba_refuse(char *err, int err_bytes, const std::string &msg)
{
    if (err && err_bytes > 0) snprintf(err, (size_t)err_bytes, "%s", msg.c_str());
    return SS_ERR_INVALID_ARG;
}

int ss_global_ba_obs_from_idx_host(const ss_keypoint *kp, const float *right, const int32_t *n_kp, int n_kf, int rows_per_frame, const int32_t *idx, int n_points,
                                   ss_gba_obs *out, int capacity)
{
    if (n_kf < 0 || n_points < 0 || rows_per_frame < 1 || capacity < 0) return SS_ERR_INVALID_ARG;
    if (n_kf > 0 && n_points > 0 && (!kp || !n_kp || !idx)) return SS_ERR_INVALID_ARG;
    int64_t n = 0;
    for (int i = 0; i < n_points; i++)
        for (int k = 0; k < n_kf; k++) {
            const int nk = std::min(std::max(n_kp[k], 0), rows_per_frame), row = idx[(size_t)k * n_points + i];
            if (row < 0 || row >= nk) continue;
            if (out && n < capacity) {
                const ss_keypoint &kk = kp[(size_t)k * rows_per_frame + row];
                out[n] = ss_gba_obs{k, i, kk.x, kk.y, right ? right[(size_t)k * rows_per_frame + row] : -1.0f, kk.octave};
            }
            n++;
        }
    return n > INT32_MAX ? SS_ERR_INVALID_ARG : (int)n;
}

int ss_global_ba_rows_from_idx_host(const int32_t *n_kp, int n_kf, int rows_per_frame, const int32_t *idx, int n_points, int32_t *out, int capacity)
{
    if (n_kf < 0 || n_points < 0 || rows_per_frame < 1 || capacity < 0) return SS_ERR_INVALID_ARG;
    if (n_kf > 0 && n_points > 0 && (!n_kp || !idx)) return SS_ERR_INVALID_ARG;
    int64_t n = 0;
    for (int i = 0; i < n_points; i++)
        for (int k = 0; k < n_kf; k++) {
            const int nk = std::min(std::max(n_kp[k], 0), rows_per_frame), row = idx[(size_t)k * n_points + i];
            if (row < 0 || row >= nk) continue;
            if (out && n < capacity) out[n] = row;
            n++;
        }
    return n > INT32_MAX ? SS_ERR_INVALID_ARG : (int)n;
}

int ss_global_ba_host(const ss_proj_view *views, const double *start, const uint8_t *fixed, int n_kf, const float *scale, int n_levels, const ss_map_point *points,
                      const uint8_t *point_skip, int n_points, const ss_gba_obs *obs, int n_obs, const ss_gba_params *p, double *poses, double *xyz,
                      uint8_t *point_flags, uint8_t *obs_flags, ss_gba_result *result, char *err, int err_bytes)
{
    if (const char *msg = gba_params_error(p)) return gba_refuse(err, err_bytes, msg);
    if (n_points < 0 || n_obs < 0 || n_kf < 0) return gba_refuse(err, err_bytes, "global BA: bad keyframe, point or record count");
    if (!scale || n_levels < 1 || n_levels > SS_MAX_LEVELS) return gba_refuse(err, err_bytes, "global BA: no pyramid table of 1 .. SS_MAX_LEVELS levels");
    if (!views || !start || !fixed || !poses || !result || (n_points > 0 && (!points || !xyz || !point_flags)) || (n_obs > 0 && (!obs || !obs_flags)))
        return gba_refuse(err, err_bytes, "global BA: NULL buffer");
    try {
        const ss_gba_problem shape = {0, n_kf, 0, n_points > 0 ? 1 : 0, 0, n_obs, {0, 0}};
        gba_host_tables t;
        const std::string msg = gba_build(n_kf, shape.n_blocks, std::max(n_points, 1), &shape, 1, obs, n_obs, scale, n_levels, p->check_right != 0, t);
        if (!msg.empty()) return gba_refuse(err, err_bytes, msg);
        const size_t P = (size_t)n_points;
        std::vector<ss_pose_cam> cam((size_t)n_kf);
        for (int k = 0; k < n_kf; k++) cam[(size_t)k] = ss_pose_cam_of(views[k], p->chi2_mono, p->chi2_stereo);
        std::vector<double> X(P * 3 + 1);
        std::vector<uint8_t> pflag(P + 1), ob((size_t)n_obs + 1);
        for (size_t i = 0; i < P; i++) {
            const ss_map_point &pt = points[i];
            const bool is_point = !(point_skip && point_skip[i] != 0) && ss_gn_is_finite((double)pt.x) && ss_gn_is_finite((double)pt.y) && ss_gn_is_finite((double)pt.z);
            pflag[i] = is_point ? 0 : 2;
            X[3 * i] = is_point ? (double)pt.x : 0.0, X[3 * i + 1] = is_point ? (double)pt.y : 0.0, X[3 * i + 2] = is_point ? (double)pt.z : 0.0;
        }
        ss_gba_problem_host(n_kf, n_points, n_obs, cam.data(), start, fixed, t.rec.data(), t.pt_off.data(), t.pt_cnt.data(), t.kf_off.data(), t.kf_cnt.data(),
                            t.kf_list.data(), *p, ob.data(), X.data(), pflag.data(), poses, result);
        for (size_t i = 0; i < P; i++) {
            point_flags[i] = pflag[i];
            for (int e = 0; e < 3; e++) xyz[3 * i + e] = pflag[i] == 2 ? 0.0 : X[3 * i + e];
        }
        for (int s = 0; s < n_obs; s++) obs_flags[t.rec[(size_t)s].orig] = ob[(size_t)s];
    } catch (const std::bad_alloc &) { /* the tables and the workspace grow with the caller's counts */
        return SS_ERR_NO_MEMORY;
    }
    return SS_OK;
}

/* the checks, the tables and the schedule of ss_global_ba_device; its host tables grow with the caller's counts and may throw */
static int gba_run(ss_ctx *c, ssk_gba_call &g, const ss_gba_problem *problems, const ss_gba_obs *obs, const ss_proj_view *views, const ss_gba_params *p)
{
    if (const char *msg = gba_params_error(p)) return fail(c, SS_ERR_INVALID_ARG, msg);
    if (g.n_kf < 0 || g.n_problems < 0 || g.n_blocks < 0 || g.n_obs < 0 || g.point_rows < 1)
        return fail(c, SS_ERR_INVALID_ARG, "global BA: bad keyframe, problem, block, row or record count");
    if (g.point_rows > SS_GUIDED_MAX_ROWS)
        return fail(c, SS_ERR_INVALID_ARG, "global BA: point_rows " + std::to_string(g.point_rows) + " exceeds SS_GUIDED_MAX_ROWS (" + std::to_string(SS_GUIDED_MAX_ROWS) + ")");
    if ((int64_t)g.n_blocks * g.point_rows > INT32_MAX / 4) return fail(c, SS_ERR_INVALID_ARG, "global BA: more than 2^29 point rows in one call");
    int n_levels = 1;
    float scale[SS_MAX_LEVELS];
    int rc = call_count_ok(c, "global BA", g.n_problems, "problems");
    if (rc == SS_OK) rc = context_pyramid(c, "global BA", &n_levels, scale);
    if (rc != SS_OK) return rc;
    if (g.n_kf == 0 || g.n_problems == 0) return SS_OK;
    if (!problems || !views) return fail(c, SS_ERR_INVALID_ARG, "global BA: problems or views is NULL");
    gba_host_tables t;
    const std::string msg = gba_build(g.n_kf, g.n_blocks, g.point_rows, problems, g.n_problems, obs, g.n_obs, scale, n_levels, p->check_right != 0, t);
    if (!msg.empty()) return fail(c, SS_ERR_INVALID_ARG, msg);
    if (!g.start || !g.fixed || !g.out_pose || !g.result || (g.n_blocks > 0 && (!g.points || !g.np || !g.out_xyz || !g.out_pflag)) || (g.n_obs > 0 && !g.out_obs))
        return fail(c, SS_ERR_INVALID_ARG, "global BA: NULL buffer");
    g.p = *p;
    g.max_kf = t.max_kf;
    const size_t K = (size_t)g.n_kf, NP = (size_t)g.n_blocks * g.point_rows, S = (size_t)g.n_obs, nq = (size_t)g.n_problems, B = (size_t)g.n_blocks;
    const size_t groups = B * (((size_t)g.point_rows + SS_GN_SLOTS - 1) / SS_GN_SLOTS);
    rc = carve_from(c, c->d_gba_ws, [&](carve &w) {
        g.pose = w.take<double>(2 * K * 12 * sizeof(double));
        g.X = w.take<double>(2 * NP * 3 * sizeof(double));
        g.pflag = w.take<uint8_t>(NP);
        g.solved = w.take<uint8_t>(NP);
        g.ob = w.take<uint8_t>(S);
        g.lin = w.take<uint8_t>(S);
        g.W = w.take<double>(S * SS_BA_W * sizeof(double));
        g.Lb = w.take<double>(NP * 12 * sizeof(double));
        g.U = w.take<double>(K * SS_BA_DIAG * sizeof(double));
        g.M = w.take<double>(K * 36 * sizeof(double));
        g.x = w.take<double>(K * 6 * sizeof(double));
        g.r = w.take<double>(K * 6 * sizeof(double));
        g.z = w.take<double>(K * 6 * sizeof(double));
        g.pv = w.take<double>(K * 6 * sizeof(double));
        g.q = w.take<double>(K * 6 * sizeof(double));
        g.cost_k = w.take<double>(K * sizeof(double));
        g.kf_flag = w.take<uint8_t>(K);
        g.part = w.take<int32_t>(groups * 4 * sizeof(int32_t));
        g.st = w.take<ssk_gba_state>(nq * sizeof(ssk_gba_state));
    });
    if (rc != SS_OK) return rc;
    /* the host tables of the call, each on a 16-byte boundary: the problems, the views, the keyframes' and the blocks' problems, the
     * keyframes' and the points' runs, the sorted records, the keyframes' lists */
    size_t at = 0;
    auto place = [&](size_t bytes) {
        const size_t o = at;
        at += (bytes + 15) & ~(size_t)15;
        return o;
    };
    const size_t o_prob = place(nq * sizeof(ss_gba_problem)), o_view = place(K * sizeof(ss_proj_view)), o_kfp = place(K * 4), o_blp = place(B * 4), o_kfo = place(K * 4),
                 o_kfc = place(K * 4), o_pto = place(NP * 4), o_ptc = place(NP * 4), o_rec = place(S * sizeof(ss_gba_rec)), o_lst = place(S * 4);
    rc = staged_upload(c, c->gba_tab, at + 16, [&](uint8_t *h) {
        memcpy(h + o_prob, problems, nq * sizeof(ss_gba_problem));
        memcpy(h + o_view, views, K * sizeof(ss_proj_view));
        memcpy(h + o_kfp, t.kf_prob.data(), K * 4);
        if (B) memcpy(h + o_blp, t.blk_prob.data(), B * 4);
        memcpy(h + o_kfo, t.kf_off.data(), K * 4);
        memcpy(h + o_kfc, t.kf_cnt.data(), K * 4);
        if (NP) memcpy(h + o_pto, t.pt_off.data(), NP * 4), memcpy(h + o_ptc, t.pt_cnt.data(), NP * 4);
        if (S) memcpy(h + o_rec, t.rec.data(), S * sizeof(ss_gba_rec)), memcpy(h + o_lst, t.kf_list.data(), S * 4);
    });
    if (rc != SS_OK) return rc;
    g.prob = c->gba_tab.as<ss_gba_problem>(o_prob);
    g.views = c->gba_tab.as<ss_proj_view>(o_view);
    g.kf_prob = c->gba_tab.as<int32_t>(o_kfp), g.blk_prob = c->gba_tab.as<int32_t>(o_blp);
    g.kf_off = c->gba_tab.as<int32_t>(o_kfo), g.kf_cnt = c->gba_tab.as<int32_t>(o_kfc);
    g.pt_off = c->gba_tab.as<int32_t>(o_pto), g.pt_cnt = c->gba_tab.as<int32_t>(o_ptc);
    g.rec = c->gba_tab.as<ss_gba_rec>(o_rec);
    g.kf_list = c->gba_tab.as<int32_t>(o_lst);
    /* the stages' bytes: what a launch reads and writes when every record is an observation of a free keyframe (an upper bound) */
    const int64_t iK = (int64_t)K, iP = (int64_t)NP, iS = (int64_t)S, iq = (int64_t)nq, iG = (int64_t)groups;
    const int64_t state_bytes = iq * (int64_t)sizeof(ssk_gba_state);
    {
        stage_timer tm(c, "gba_gather", iK * (96 + 192 + 1) + iP * (32 + 8 + 48 + 2 + (g.p_skip ? 1 : 0)) + iS * 33 + iG * 32 + state_bytes);
        ssk_gba_gather(c->stream, g);
    }
    for (int r = 0; r < p->n_rounds; r++) {
        for (int it = -1; it < p->iterations[r]; it++) {
            if (it >= 0) {
                {
                    stage_timer tm(c, "gba_points", iP * (8 + 1 + 24 + 72 + 1) + iS * (1 + 32 + 96 + 48 + 1 + 144 + 1) + iG * 4);
                    ssk_gba_points(c->stream, g, r);
                }
                {
                    stage_timer tm(c, "gba_blocks", iS * (4 + 1 + 32 + 1 + 24 + 144 + 72) + iK * (8 + 96 + 48 + 168 + 288 + 5 * 48 + 1 + 48 + 1) + iG * 4 + 2 * state_bytes);
                    ssk_gba_blocks(c->stream, g, r);
                }
                for (int m = 0; m < p->pcg_iterations; m++) {
                    stage_timer tm(c, "gba_pcg", iS * (1 + 32 + 1 + 144 + 48) + iP * (8 + 1 + 48 + 24) + iS * (4 + 1 + 32 + 1 + 144 + 24) + iK * (8 + 168 + 48 + 48) +
                                                     iK * (6 * 48 + 288 + 1) + 2 * state_bytes);
                    ssk_gba_pcg(c->stream, g);
                }
                {
                    stage_timer tm(c, "gba_update", iK * (96 + 48 + 96 + 2) + iP * (8 + 2 + 24 + 72 + 24) + iS * (1 + 32 + 1 + 144 + 48) + iG * 8);
                    ssk_gba_update(c->stream, g);
                }
            }
            stage_timer tm(c, "gba_cost", iK * (8 + 96 + 48 + 8) + iS * (4 + 1 + 32 + 1 + 24) + iK * 9 + iG * 8 + 2 * state_bytes);
            ssk_gba_cost(c->stream, g, r, it >= 0 ? 0 : 1);
        }
        stage_timer tm(c, "gba_classify", iP * (8 + 1 + 24 + 1) + iS * (1 + 32 + 96 + 48 + 1));
        ssk_gba_classify(c->stream, g);
    }
    {
        stage_timer tm(c, "gba_finish", iP * (8 + 1 + 24 + 24 + 1) + iS * (1 + 32 + 1 + 1) + iK * (4 + 96 + 96) + iG * 16 + iq * (int64_t)sizeof(ss_gba_result) + state_bytes);
        ssk_gba_finish(c->stream, g);
    }
    HIP_TRY(c, hipGetLastError());
    return SS_OK;
}

int ss_global_ba_device(ss_ctx *c, const void *d_points, const void *d_point_skip, const void *d_n_points, int n_blocks, int point_rows, const void *d_start,
                        const void *d_fixed, int n_kf, const ss_gba_problem *problems, int n_problems, const ss_gba_obs *obs, int n_obs, const ss_proj_view *views,
                        const ss_gba_params *p, void *d_poses, void *d_xyz, void *d_point_flags, void *d_obs_flags, void *d_result)
{
    if (!c) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    ssk_gba_call g;
    g.n_kf = n_kf, g.n_problems = n_problems, g.n_blocks = n_blocks, g.point_rows = point_rows, g.n_obs = n_obs;
    g.points = (const ss_map_point *)d_points, g.p_skip = (const uint8_t *)d_point_skip, g.np = (const int32_t *)d_n_points;
    g.start = (const double *)d_start, g.fixed = (const uint8_t *)d_fixed;
    g.out_pose = (double *)d_poses, g.out_xyz = (double *)d_xyz, g.out_pflag = (uint8_t *)d_point_flags, g.out_obs = (uint8_t *)d_obs_flags;
    g.result = (ss_gba_result *)d_result;
    try {
        return gba_run(c, g, problems, obs, views, p);
    } catch (const std::bad_alloc &) {
        return fail(c, SS_ERR_NO_MEMORY, "global BA: no host memory for the tables of the call");
    }
}

int ss_global_ba(ss_ctx *c, const ss_proj_view *views, const double *start, const uint8_t *fixed, int n_kf, const ss_map_point *points, const uint8_t *point_skip,
                 int n_points, const ss_gba_obs *obs, int n_obs, const ss_gba_params *p, double *poses, double *xyz, uint8_t *point_flags, uint8_t *obs_flags,
                 ss_gba_result *result)
{
    if (!c) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    if (const char *msg = gba_params_error(p)) return fail(c, SS_ERR_INVALID_ARG, msg);
    if (n_kf < 1 || n_kf > SS_GBA_MAX_KF) return fail(c, SS_ERR_INVALID_ARG, "global BA: problem 0: n_kf " + std::to_string(n_kf) + " outside 1 .. SS_GBA_MAX_KF (" + std::to_string(SS_GBA_MAX_KF) + ")");
    if (n_points < 0 || n_points > SS_GBA_MAX_POINTS || n_obs < 0 || n_obs > SS_GBA_MAX_OBS)
        return fail(c, SS_ERR_INVALID_ARG, "global BA: n_points must be 0 .. SS_GBA_MAX_POINTS and n_obs 0 .. SS_GBA_MAX_OBS");
    if (!views || !start || !fixed || !poses || !result || (n_points > 0 && (!points || !xyz || !point_flags)) || (n_obs > 0 && (!obs || !obs_flags)))
        return fail(c, SS_ERR_INVALID_ARG, "global BA: NULL buffer");
    /* the points as blocks of `pr` rows, the last one short: point i is row i % pr of block i / pr.  `count` is on this stack: no
     * return before the stream has read it */
    const int pr = std::min(std::max(n_points, 1), SS_GUIDED_MAX_ROWS), nb = n_points > 0 ? (n_points + pr - 1) / pr : 0;
    const size_t np = (size_t)n_points, room = (size_t)std::max(nb, 1) * pr, kf = (size_t)n_kf, ns = (size_t)n_obs;
    std::vector<int32_t> count((size_t)std::max(nb, 1), 0);
    for (int b = 0; b < nb; b++) count[(size_t)b] = std::min(pr, n_points - b * pr);
    const ss_gba_problem problem = {0, n_kf, 0, nb, 0, n_obs, {0, 0}};
    enum { PT, PS, NP, ST, FX, POSE, XYZ, PF, OF, RES, PIECES };
    io_piece io[PIECES] = {{points, nullptr, room * sizeof(ss_map_point), np * sizeof(ss_map_point)},
                           {point_skip, nullptr, room, np},
                           {count.data(), nullptr, count.size() * 4, count.size() * 4},
                           {start, nullptr, kf * 96, kf * 96},
                           {fixed, nullptr, kf, kf},
                           {nullptr, poses, kf * 96, kf * 96},
                           {nullptr, xyz, room * 24, np * 24},
                           {nullptr, point_flags, room, np},
                           {nullptr, obs_flags, std::max(ns, (size_t)1), ns},
                           {nullptr, result, sizeof(ss_gba_result), sizeof(ss_gba_result)}};
    int rc = io_send(c, c->d_gba_io, io, PIECES);
    if (rc == SS_OK)
        rc = ss_global_ba_device(c, io[PT].d, point_skip ? io[PS].d : nullptr, io[NP].d, nb, pr, io[ST].d, io[FX].d, n_kf, &problem, 1, obs, n_obs, views, p, io[POSE].d,
                                 io[XYZ].d, io[PF].d, io[OF].d, io[RES].d);
    if (rc != SS_OK) {
        (void)hipStreamSynchronize(c->stream);
        return rc;
    }
    return io_fetch(c, io, PIECES);
}

/* ---- covisibility (csrc/ss_covis.hip, csrc/ss_covis_steps.h) ---- */
/* the message of the first rule p or cap breaks, or NULL; needs no context */
static const char *covis_params_error(const ss_covis_params *p, int cap)
{
    if (!p) return "covis: params is NULL";
    if (p->min_weight < 1) return "covis: min_weight must be >= 1";
    if (p->fallback != 0 && p->fallback != 1) return "covis: fallback must be 0 or 1";
    if (p->cull_obs < 0) return "covis: cull_obs must be >= 0";
    if (p->cull_slack < 0 || p->cull_slack > SS_MAX_LEVELS) return "covis: cull_slack must be 0 .. SS_MAX_LEVELS";
    if (!(p->redundant_th >= 0.0f && p->redundant_th <= 1.0f)) return "covis: redundant_th must be finite and 0 .. 1";
    if (p->reserved[0] != 0 || p->reserved[1] != 0 || p->reserved[2] != 0) return "covis: the reserved fields must be 0";
    if (cap < 1 || cap > SS_COVIS_MAX_NEIGHBOURS) return "covis: cap must be 1 .. SS_COVIS_MAX_NEIGHBOURS (1024)";
    return nullptr;
}

int ss_covis_params_default(ss_covis_params *p)
{
    if (!p) return SS_ERR_INVALID_ARG;
    *p = ss_covis_params{15, 1, 3, 1, 0.9f, {0, 0, 0}};
    return SS_OK;
}

/* the map's tables on the host */
struct covis_host_tables {
    std::vector<ss_covis_prob> prob;
    std::vector<int32_t> kf_prob, blk_prob, pt_off, pt_cnt, kf_off, kf_cnt, kf_item;
    std::vector<uint32_t> pt_item;
    std::vector<int32_t> pt_row, long_pts; /* with rows: each record's keypoint row, in the order of pt_item; the points of a list above one wave's */
    int n_kf = 0, n_blocks = 0, point_rows = 0, max_kf = 0, max_row = -1, max_cnt = 0;
    bool has_rows = false;
    size_t items = 0;
    ss_covis_tab view() const
    {
        ss_covis_tab m;
        m.n_kf = n_kf, m.n_blocks = n_blocks, m.point_rows = point_rows, m.n_problems = (int)prob.size(), m.max_kf = max_kf;
        m.prob = prob.data(), m.kf_prob = kf_prob.data(), m.blk_prob = blk_prob.data();
        m.kf_off = kf_off.data(), m.kf_cnt = kf_cnt.data(), m.pt_off = pt_off.data(), m.pt_cnt = pt_cnt.data();
        m.pt_item = pt_item.data(), m.kf_item = kf_item.data();
        return m;
    }
};

/* The checks of ss_covis_set_map and the lists of every problem into t.  The message of the first rule that is broken, or empty.  May
 * throw std::bad_alloc: the tables grow with the caller's counts */
static std::string covis_build(const ss_gba_problem *problems, int n_problems, int n_kf, int n_blocks, int point_rows, const ss_gba_obs *obs, int n_obs,
                               const uint8_t *cull_skip, bool check_right, int n_levels, covis_host_tables &t, const int32_t *obs_row = nullptr)
{
    if (n_kf < 0 || n_problems < 0 || n_blocks < 0 || n_obs < 0 || point_rows < 1) return "covis: bad keyframe, problem, block, row or record count";
    if (point_rows > SS_GUIDED_MAX_ROWS)
        return "covis: point_rows " + std::to_string(point_rows) + " exceeds SS_GUIDED_MAX_ROWS (" + std::to_string(SS_GUIDED_MAX_ROWS) + ")";
    if ((int64_t)n_blocks * point_rows > INT32_MAX / 4) return "covis: more than 2^29 point rows in one call";
    if (n_kf > SS_COVIS_MAX_MAP_KF) return "covis: n_kf " + std::to_string(n_kf) + " exceeds SS_COVIS_MAX_MAP_KF (" + std::to_string(SS_COVIS_MAX_MAP_KF) + ") keyframes in one call";
    if (n_levels < 1 || n_levels > SS_MAX_LEVELS) return "covis: no pyramid of 1 .. SS_MAX_LEVELS levels";
    if (n_problems > 0 && !problems) return "covis: problems is NULL";
    const std::string ranges = problem_ranges("covis", n_kf, n_blocks, point_rows, problems, n_problems, n_obs, t.kf_prob, t.blk_prob, &t.max_kf);
    if (!ranges.empty()) return ranges;
    const size_t NP = (size_t)n_blocks * point_rows;
    t.n_kf = n_kf, t.n_blocks = n_blocks, t.point_rows = point_rows;
    t.pt_off.assign(NP + 1, 0), t.pt_cnt.assign(NP + 1, 0), t.kf_off.assign((size_t)n_kf + 1, 0), t.kf_cnt.assign((size_t)n_kf + 1, 0);
    t.items = 0;
    for (int q = 0; q < n_problems; q++) t.items += (size_t)problems[q].n_obs;
    t.pt_item.assign(t.items + 1, 0u), t.kf_item.assign(2 * t.items + 2, 0);
    t.prob.resize((size_t)n_problems);
    t.has_rows = obs_row != nullptr;
    t.pt_row.assign(obs_row ? t.items + 1 : 0, 0);
    std::vector<int32_t> from;
    size_t base = 0;
    for (int q = 0; q < n_problems; q++) {
        const ss_gba_problem &b = problems[q];
        t.prob[(size_t)q] = ss_covis_prob{b.first_kf, b.n_kf, b.first_block, b.n_blocks};
        if (b.n_obs > 0 && !obs) return "covis: obs is NULL";
        const int P = b.n_blocks * point_rows;
        const size_t p0 = (size_t)b.first_block * point_rows;
        int bad = 0;
        if (obs_row) from.assign((size_t)b.n_obs + 1, 0);
        const int why = ss_covis_tables(b.n_kf, P, obs + b.first_obs, cull_skip ? cull_skip + b.first_obs : nullptr, b.n_obs, n_levels, check_right, (int)base, (int)p0,
                                        t.pt_off.data() + p0, t.pt_cnt.data() + p0, t.kf_off.data() + b.first_kf, t.kf_cnt.data() + b.first_kf, t.pt_item.data() + base,
                                        t.kf_item.data() + 2 * base, &bad, obs_row ? from.data() : nullptr);
        if (why != 0) {
            const ss_gba_obs &o = obs[b.first_obs + bad];
            const std::string rec = "covis: problem " + std::to_string(q) + ": record " + std::to_string(b.first_obs + bad) + ": ";
            if (why == 1) return rec + "kf " + std::to_string(o.kf) + " outside 0 .. " + std::to_string(b.n_kf - 1);
            if (why == 2) return rec + "point " + std::to_string(o.point) + " outside 0 .. " + std::to_string(P - 1);
            if (why == 3) return rec + "the pair (kf " + std::to_string(o.kf) + ", point " + std::to_string(o.point) + ") has a record already";
            return rec + "keyframe " + std::to_string(o.kf) + " has more than SS_COVIS_MAX_ROW_ITEMS (" + std::to_string(SS_COVIS_MAX_ROW_ITEMS) + ") records";
        }
        for (int s = 0; obs_row && s < b.n_obs; s++) {
            const int m = b.first_obs + from[(size_t)s], row = obs_row[m];
            if (row < 0 || row >= SS_GUIDED_MAX_ROWS)
                return "covis: problem " + std::to_string(q) + ": record " + std::to_string(m) + ": row " + std::to_string(row) + " outside 0 .. SS_GUIDED_MAX_ROWS - 1 (" +
                       std::to_string(SS_GUIDED_MAX_ROWS - 1) + ")";
            t.pt_row[base + (size_t)s] = row;
            t.max_row = std::max(t.max_row, row);
        }
        base += (size_t)b.n_obs;
    }
    for (size_t gp = 0; gp < NP; gp++) {
        t.max_cnt = std::max(t.max_cnt, (int)t.pt_cnt[gp]);
        if (t.pt_cnt[gp] > SS_REFRESH_SHORT) t.long_pts.push_back((int32_t)gp);
    }
    return std::string();
}

/* the checks of a query against the map m (`what` heads the messages); table: the keyframe numbers or, frames, the block numbers */
static std::string covis_query_error(const std::string &what, const ss_covis_tab &m, bool frames, const int32_t *table, int n_rows, const ss_covis_params *p, int cap)
{
    if (const char *msg = covis_params_error(p, cap)) return msg;
    if (n_rows < 0) return what + ": bad row count";
    if (n_rows > 65535) return what + ": more than 65535 rows in one call";
    if (frames && n_rows > 0 && !table) return what + ": point_src is NULL";
    if (!frames && !table && n_rows != 0 && n_rows != m.n_kf)
        return what + ": rows is NULL, so n_rows must be the map's " + std::to_string(m.n_kf) + " keyframes, not " + std::to_string(n_rows);
    const int limit = frames ? m.n_blocks : m.n_kf;
    for (int r = 0; table && r < n_rows; r++)
        if (table[r] < 0 || table[r] >= limit)
            return what + ": row " + std::to_string(r) + ": " + (frames ? "block " : "keyframe ") + std::to_string(table[r]) + " lies outside the map's " + std::to_string(limit);
    return std::string();
}

static int covis_host(bool frames, const ss_gba_problem *problems, int n_problems, int n_kf, int n_blocks, int point_rows, const ss_gba_obs *obs, int n_obs,
                      const uint8_t *cull_skip, int check_right, int n_levels, const int32_t *table, const int32_t *idx, const int32_t *n_points, int n_rows,
                      const ss_covis_params *p, int cap, int32_t *nb, ss_covis_row *row, char *err, int err_bytes)
{
    const std::string what = frames ? "ss_covis_frames_host" : "ss_covis_kf_host";
    try {
        covis_host_tables t;
        std::string msg = covis_build(problems, n_problems, n_kf, n_blocks, point_rows, obs, n_obs, cull_skip, check_right != 0, n_levels, t);
        if (msg.empty() && n_problems == 0) msg = what + ": no map";
        const ss_covis_tab m = t.view();
        if (msg.empty()) msg = covis_query_error(what, m, frames, table, n_rows, p, cap);
        if (msg.empty() && n_rows > 0 && (!nb || !row || (frames && (!idx || !n_points)))) msg = what + ": NULL buffer";
        if (!msg.empty()) return gba_refuse(err, err_bytes, msg);
        std::vector<int32_t> w;
        for (int r = 0; r < n_rows; r++) {
            const int at = table ? table[r] : r;
            ss_covis_row_host(m, frames ? -1 : at, frames ? at : 0, frames ? idx + (size_t)r * point_rows : nullptr, frames ? n_points[at] : 0, *p, cap,
                              nb + (size_t)r * cap * 2, row + r, w);
        }
    } catch (const std::bad_alloc &) {
        return SS_ERR_NO_MEMORY;
    }
    return SS_OK;
}

int ss_covis_kf_host(const ss_gba_problem *problems, int n_problems, int n_kf, int n_blocks, int point_rows, const ss_gba_obs *obs, int n_obs, const uint8_t *cull_skip,
                     int check_right, int n_levels, const int32_t *rows, int n_rows, const ss_covis_params *p, int cap, int32_t *nb, ss_covis_row *row, char *err,
                     int err_bytes)
{
    return covis_host(false, problems, n_problems, n_kf, n_blocks, point_rows, obs, n_obs, cull_skip, check_right, n_levels, rows, nullptr, nullptr, n_rows, p, cap, nb, row,
                      err, err_bytes);
}

int ss_covis_frames_host(const ss_gba_problem *problems, int n_problems, int n_kf, int n_blocks, int point_rows, const ss_gba_obs *obs, int n_obs,
                         const uint8_t *cull_skip, int check_right, int n_levels, const int32_t *idx, const int32_t *n_points, const int32_t *point_src, int n_frames,
                         const ss_covis_params *p, int cap, int32_t *nb, ss_covis_row *row, char *err, int err_bytes)
{
    return covis_host(true, problems, n_problems, n_kf, n_blocks, point_rows, obs, n_obs, cull_skip, check_right, n_levels, point_src, idx, n_points, n_frames, p, cap, nb,
                      row, err, err_bytes);
}

int ss_covis_edges_host(const int32_t *nb, const ss_covis_row *row, const int32_t *row_kf, int n_rows, int cap, int min_weight, int32_t *edges, int capacity)
{
    if (n_rows < 0 || cap < 1 || capacity < 0 || (n_rows > 0 && (!nb || !row || !row_kf))) return SS_ERR_INVALID_ARG;
    int64_t n = 0;
    for (int r = 0; r < n_rows; r++) {
        const int listed = std::min(std::max(row[r].n_written, 0), cap);
        for (int e = 0; e < listed; e++) {
            const int32_t j = nb[((size_t)r * cap + e) * 2], w = nb[((size_t)r * cap + e) * 2 + 1];
            if (j <= row_kf[r] || w < min_weight) continue;
            if (edges && n < capacity) edges[2 * n] = row_kf[r], edges[2 * n + 1] = j;
            n++;
        }
    }
    return n > INT32_MAX ? SS_ERR_INVALID_ARG : (int)n;
}

static int covis_set_map(ss_ctx *c, const ss_gba_problem *problems, int n_problems, int n_kf, int n_blocks, int point_rows, const ss_gba_obs *obs, int n_obs,
                         const uint8_t *cull_skip, int check_right, const int32_t *obs_row)
{
    int n_levels = 1;
    float scale[SS_MAX_LEVELS];
    const int rc = context_pyramid(c, "covis", &n_levels, scale);
    if (rc != SS_OK) return rc;
    covis_host_tables t;
    const std::string msg = covis_build(problems, n_problems, n_kf, n_blocks, point_rows, obs, n_obs, cull_skip, check_right != 0, n_levels, t, obs_row);
    if (!msg.empty()) return fail(c, SS_ERR_INVALID_ARG, msg);
    auto no_map = [&]() {
        c->covis_map = ss_covis_tab();
        c->covis_items = 0;
        c->covis_pt_row = c->covis_long = nullptr;
        c->covis_max_row = -1, c->covis_n_long = c->covis_max_cnt = 0;
    };
    if (n_problems == 0) {
        no_map();
        return SS_OK;
    }
    /* the tables, each on a 16-byte boundary */
    const size_t K = (size_t)n_kf, B = (size_t)n_blocks, NP = B * point_rows, S = t.items, nq = (size_t)n_problems;
    size_t at = 0;
    auto place = [&](size_t bytes) {
        const size_t o = at;
        at += (bytes + 15) & ~(size_t)15;
        return o;
    };
    const size_t o_prob = place(nq * sizeof(ss_covis_prob)), o_kfp = place(K * 4), o_blp = place(B * 4), o_kfo = place(K * 4), o_kfc = place(K * 4), o_pto = place(NP * 4),
                 o_ptc = place(NP * 4), o_pti = place(S * 4), o_kfi = place(S * 8), o_row = place(t.has_rows ? S * 4 : 0), o_long = place(t.long_pts.size() * 4);
    {
        stage_timer tm(c, "covis_upload", (int64_t)at);
        const int up = staged_upload(c, c->covis_tab, at + 16, [&](uint8_t *h) {
            memcpy(h + o_prob, t.prob.data(), nq * sizeof(ss_covis_prob));
            memcpy(h + o_kfp, t.kf_prob.data(), K * 4);
            if (B) memcpy(h + o_blp, t.blk_prob.data(), B * 4);
            memcpy(h + o_kfo, t.kf_off.data(), K * 4);
            memcpy(h + o_kfc, t.kf_cnt.data(), K * 4);
            if (NP) memcpy(h + o_pto, t.pt_off.data(), NP * 4), memcpy(h + o_ptc, t.pt_cnt.data(), NP * 4);
            if (S) memcpy(h + o_pti, t.pt_item.data(), S * 4), memcpy(h + o_kfi, t.kf_item.data(), S * 8);
            if (S && t.has_rows) memcpy(h + o_row, t.pt_row.data(), S * 4);
            if (!t.long_pts.empty()) memcpy(h + o_long, t.long_pts.data(), t.long_pts.size() * 4);
        });
        if (up != SS_OK) {
            no_map(); /* the buffer may have moved */
            return up;
        }
    }
    ss_covis_tab m;
    m.n_kf = n_kf, m.n_blocks = n_blocks, m.point_rows = point_rows, m.n_problems = n_problems, m.max_kf = t.max_kf;
    m.prob = c->covis_tab.as<ss_covis_prob>(o_prob);
    m.kf_prob = c->covis_tab.as<int32_t>(o_kfp), m.blk_prob = c->covis_tab.as<int32_t>(o_blp);
    m.kf_off = c->covis_tab.as<int32_t>(o_kfo), m.kf_cnt = c->covis_tab.as<int32_t>(o_kfc);
    m.pt_off = c->covis_tab.as<int32_t>(o_pto), m.pt_cnt = c->covis_tab.as<int32_t>(o_ptc);
    m.pt_item = c->covis_tab.as<uint32_t>(o_pti), m.kf_item = c->covis_tab.as<int32_t>(o_kfi);
    c->covis_map = m;
    c->covis_items = (int64_t)S;
    c->covis_pt_row = t.has_rows ? c->covis_tab.as<int32_t>(o_row) : nullptr;
    c->covis_long = c->covis_tab.as<int32_t>(o_long);
    c->covis_max_row = t.max_row, c->covis_n_long = (int)t.long_pts.size(), c->covis_max_cnt = t.max_cnt;
    return SS_OK;
}

int ss_covis_set_map_rows(ss_ctx *c, const ss_gba_problem *problems, int n_problems, int n_kf, int n_blocks, int point_rows, const ss_gba_obs *obs, int n_obs,
                          const uint8_t *cull_skip, int check_right, const int32_t *obs_row)
{
    if (!c) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    try {
        return covis_set_map(c, problems, n_problems, n_kf, n_blocks, point_rows, obs, n_obs, cull_skip, check_right, obs_row);
    } catch (const std::bad_alloc &) {
        return fail(c, SS_ERR_NO_MEMORY, "covis: no host memory for the tables of the map");
    }
}

int ss_covis_set_map(ss_ctx *c, const ss_gba_problem *problems, int n_problems, int n_kf, int n_blocks, int point_rows, const ss_gba_obs *obs, int n_obs,
                     const uint8_t *cull_skip, int check_right)
{
    return ss_covis_set_map_rows(c, problems, n_problems, n_kf, n_blocks, point_rows, obs, n_obs, cull_skip, check_right, nullptr);
}

/* the checks, the table and the launch of both device forms */
static int covis_query(ss_ctx *c, const std::string &what, bool frames, const int32_t *table, int n_rows, const ss_covis_params *p, int cap, const void *d_idx,
                       const void *d_n_points, void *d_nb, void *d_row)
{
    const ss_covis_tab &m = c->covis_map;
    if (const char *msg = covis_params_error(p, cap)) return fail(c, SS_ERR_INVALID_ARG, msg);
    if (m.n_kf == 0) return fail(c, SS_ERR_STATE, what + ": no map (ss_covis_set_map)");
    const std::string msg = covis_query_error(what, m, frames, table, n_rows, p, cap);
    if (!msg.empty()) return fail(c, SS_ERR_INVALID_ARG, msg);
    if (n_rows == 0) return SS_OK;
    if (!d_nb || !d_row || (frames && (!d_idx || !d_n_points))) return fail(c, SS_ERR_INVALID_ARG, what + ": NULL buffer");
    ssk_covis_call g;
    g.tab = &m, g.n_rows = n_rows, g.cap = cap, g.p = *p;
    g.idx = (const int32_t *)d_idx, g.np = (const int32_t *)d_n_points;
    g.nb = (int32_t *)d_nb, g.row = (ss_covis_row *)d_row;
    if (table) {
        const int rc = staged_upload(c, c->covis_call_tab, (size_t)n_rows * 4, [&](uint8_t *h) { memcpy(h, table, (size_t)n_rows * 4); });
        if (rc != SS_OK) return rc;
        (frames ? g.src : g.rows) = c->covis_call_tab.as<int32_t>();
    }
    /* the stage's bytes: the row's share of the map's lists (a mean row's; 12 bytes per record, its point's list once more and the
     * point's run), the frame's idx, and the outputs */
    const int64_t out = (int64_t)n_rows * (cap * 8 + 32 + 4);
    hipError_t e;
    if (frames) {
        stage_timer tm(c, "covis_frames", (int64_t)n_rows * m.point_rows * (4 + 8) + out);
        e = (hipError_t)ssk_covis_frames(c->stream, g);
    } else {
        stage_timer tm(c, "covis_kf", c->covis_items * (12 + 8) * n_rows / m.n_kf + out);
        e = (hipError_t)ssk_covis_kf(c->stream, g);
    }
    HIP_TRY(c, e);
    HIP_TRY(c, hipGetLastError());
    return SS_OK;
}

int ss_covis_kf_device(ss_ctx *c, const int32_t *rows, int n_rows, const ss_covis_params *p, int cap, void *d_nb, void *d_row)
{
    if (!c) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    return covis_query(c, "ss_covis_kf_device", false, rows, n_rows, p, cap, nullptr, nullptr, d_nb, d_row);
}

int ss_covis_frames_device(ss_ctx *c, const void *d_idx, const void *d_n_points, const int32_t *point_src, int n_frames, const ss_covis_params *p, int cap, void *d_nb,
                           void *d_row)
{
    if (!c) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    return covis_query(c, "ss_covis_frames_device", true, point_src, n_frames, p, cap, d_idx, d_n_points, d_nb, d_row);
}

int ss_covis(ss_ctx *c, int n_kf, int n_points, const ss_gba_obs *obs, int n_obs, const uint8_t *cull_skip, int check_right, const ss_covis_params *p, int cap,
             int32_t *nb, ss_covis_row *row)
{
    if (!c) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    if (const char *msg = covis_params_error(p, cap)) return fail(c, SS_ERR_INVALID_ARG, msg);
    if (n_points < 0 || n_points > SS_GBA_MAX_POINTS || n_obs < 0) return fail(c, SS_ERR_INVALID_ARG, "covis: n_points must be 0 .. SS_GBA_MAX_POINTS and n_obs >= 0");
    if (!nb || !row) return fail(c, SS_ERR_INVALID_ARG, "ss_covis: NULL buffer");
    /* the points as blocks of `pr` rows, the last one short, as ss_global_ba lays them out */
    const int pr = std::min(std::max(n_points, 1), SS_GUIDED_MAX_ROWS), nblk = n_points > 0 ? (n_points + pr - 1) / pr : 0;
    const ss_gba_problem problem = {0, n_kf, 0, nblk, 0, n_obs, {0, 0}};
    int rc = ss_covis_set_map(c, &problem, 1, n_kf, nblk, pr, obs, n_obs, cull_skip, check_right);
    if (rc != SS_OK) return rc;
    const size_t kf = (size_t)n_kf;
    enum { NB, ROW, PIECES };
    io_piece io[PIECES] = {{nullptr, nb, kf * cap * 8, kf * cap * 8}, {nullptr, row, kf * sizeof(ss_covis_row), kf * sizeof(ss_covis_row)}};
    rc = io_send(c, c->d_covis_io, io, PIECES);
    if (rc == SS_OK) rc = ss_covis_kf_device(c, nullptr, n_kf, p, cap, io[NB].d, io[ROW].d);
    if (rc != SS_OK) {
        (void)hipStreamSynchronize(c->stream);
        return rc;
    }
    return io_fetch(c, io, PIECES);
}

/* ---- map-point refresh (csrc/ss_refresh.hip, csrc/ss_refresh_steps.h) ---- */
/* the message of the first rule p breaks, or NULL; needs no context */
static const char *refresh_params_error(const ss_refresh_params *p)
{
    if (!p) return "refresh: params is NULL";
    if (p->geometry != 0 && p->geometry != 1) return "refresh: geometry must be 0 or 1";
    if (p->descriptor != 0 && p->descriptor != 1) return "refresh: descriptor must be 0 or 1";
    if (p->geometry == 0 && p->descriptor == 0) return "refresh: geometry or descriptor must be set";
    for (int k = 0; k < 6; k++)
        if (p->reserved[k] != 0) return "refresh: the reserved fields must be 0";
    return nullptr;
}

int ss_refresh_params_default(ss_refresh_params *p)
{
    if (!p) return SS_ERR_INVALID_ARG;
    *p = ss_refresh_params{1, 1, {0, 0, 0, 0, 0, 0}};
    return SS_OK;
}

/* the checks of a call against a map of n_kf keyframes whose largest row is max_row (`what` heads the messages), or empty */
static std::string refresh_call_error(const std::string &what, int n_kf, int max_row, int rows_per_frame, const ss_refresh_params *p)
{
    if (p->descriptor == 0) return std::string();
    if (rows_per_frame > SS_GUIDED_MAX_ROWS)
        return what + ": rows_per_frame " + std::to_string(rows_per_frame) + " exceeds SS_GUIDED_MAX_ROWS (" + std::to_string(SS_GUIDED_MAX_ROWS) + ")";
    if (rows_per_frame <= max_row || rows_per_frame < 1)
        return what + ": rows_per_frame " + std::to_string(rows_per_frame) + " is not above the map's largest row " + std::to_string(max_row);
    if ((int64_t)n_kf * rows_per_frame > INT32_MAX) return what + ": n_kf * rows_per_frame exceeds 2^31 - 1 descriptor rows";
    return std::string();
}

int ss_refresh_device(ss_ctx *c, void *d_points, void *d_point_desc, const void *d_n_points, const void *d_ref_kf, const void *d_select, const void *d_desc,
                      int rows_per_frame, const ss_proj_view *views, const ss_refresh_params *p, void *d_info, void *d_summary)
{
    if (!c) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    const std::string what = "ss_refresh_device";
    if (const char *msg = refresh_params_error(p)) return fail(c, SS_ERR_INVALID_ARG, msg);
    const ss_covis_tab &m = c->covis_map;
    if (m.n_kf == 0) return fail(c, SS_ERR_STATE, what + ": no map (ss_covis_set_map_rows)");
    if (p->descriptor != 0 && !c->covis_pt_row) return fail(c, SS_ERR_STATE, what + ": the map was set without rows (ss_covis_set_map_rows), which descriptor needs");
    const std::string msg = refresh_call_error(what, m.n_kf, c->covis_max_row, rows_per_frame, p);
    if (!msg.empty()) return fail(c, SS_ERR_INVALID_ARG, msg);
    if (!d_points || !d_n_points || !views || !d_info || !d_summary || (p->descriptor != 0 && (!d_desc || !d_point_desc))) return fail(c, SS_ERR_INVALID_ARG, what + ": NULL buffer");
    if (m.n_blocks == 0) return SS_OK;
    int n_levels = 1;
    float scale[SS_MAX_LEVELS];
    int rc = context_pyramid(c, "refresh", &n_levels, scale);
    if (rc != SS_OK) return rc;
    /* the tables of the call: every keyframe's ow, then the pyramid's table */
    const size_t K = (size_t)m.n_kf, o_scale = (K * 12 + 15) & ~(size_t)15;
    rc = staged_upload(c, c->refresh_tab, o_scale + SS_MAX_LEVELS * 4, [&](uint8_t *h) {
        for (size_t k = 0; k < K; k++) memcpy(h + 12 * k, views[k].ow, 12);
        memcpy(h + o_scale, scale, sizeof(scale[0]) * (size_t)n_levels);
    });
    if (rc != SS_OK) return rc;
    ssk_refresh_call g;
    g.tab = &m, g.pt_row = c->covis_pt_row, g.long_pts = c->covis_long, g.n_long = c->covis_n_long, g.max_cnt = c->covis_max_cnt;
    g.points = (ss_map_point *)d_points, g.point_desc = (uint8_t *)d_point_desc, g.np = (const int32_t *)d_n_points;
    g.ref_kf = (const int32_t *)d_ref_kf, g.select = (const uint8_t *)d_select, g.desc = (const uint8_t *)d_desc, g.rows_per_frame = rows_per_frame;
    g.ow = c->refresh_tab.as<float>(), g.scale = c->refresh_tab.as<float>(o_scale), g.n_levels = n_levels;
    g.geometry = p->geometry, g.descriptor = p->descriptor;
    g.info = (ss_refresh_info *)d_info, g.summary = (ss_refresh_summary *)d_summary;
    /* the stage's bytes: per record its word of the list, the keyframe's ow (geometry), its row and its descriptor (descriptor); per
     * point row its run, the point and its info, the fields (geometry) or the descriptor (descriptor) written; per block its count
     * and its summary */
    const int64_t NP = (int64_t)m.n_blocks * m.point_rows;
    const int64_t bytes = c->covis_items * (4 + 12 * p->geometry + 36 * p->descriptor) + NP * (8 + 32 + 32 + 20 * p->geometry + 32 * p->descriptor) + (int64_t)m.n_blocks * 36;
    hipError_t e;
    {
        stage_timer tm(c, "refresh", bytes);
        e = (hipError_t)ssk_refresh(c->stream, g);
    }
    HIP_TRY(c, e);
    HIP_TRY(c, hipGetLastError());
    return SS_OK;
}

/* the blocks ss_covis and ss_refresh lay n_points points out in: rows per block, blocks */
static void single_problem_blocks(int n_points, int *pr, int *nblk)
{
    *pr = std::min(std::max(n_points, 1), SS_GUIDED_MAX_ROWS);
    *nblk = n_points > 0 ? (n_points + *pr - 1) / *pr : 0;
}

int ss_refresh(ss_ctx *c, const ss_proj_view *views, int n_kf, ss_map_point *points, uint8_t *point_desc, int n_points, const int32_t *ref_kf, const uint8_t *select,
               const ss_gba_obs *obs, const int32_t *obs_row, int n_obs, int check_right, const uint8_t *desc, int rows_per_frame, const ss_refresh_params *p,
               ss_refresh_info *info, ss_refresh_summary *summary)
{
    if (!c) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    if (const char *msg = refresh_params_error(p)) return fail(c, SS_ERR_INVALID_ARG, msg);
    if (n_points < 1 || n_points > SS_GBA_MAX_POINTS || n_obs < 0 || n_kf < 1) return fail(c, SS_ERR_INVALID_ARG, "refresh: n_points must be 1 .. SS_GBA_MAX_POINTS, n_kf >= 1 and n_obs >= 0");
    if (!views || !points || !info || !summary || (p->descriptor != 0 && (!desc || !point_desc || (n_obs > 0 && !obs_row)))) return fail(c, SS_ERR_INVALID_ARG, "ss_refresh: NULL buffer");
    int pr, nblk;
    single_problem_blocks(n_points, &pr, &nblk);
    const ss_gba_problem problem = {0, n_kf, 0, nblk, 0, n_obs, {0, 0}};
    int rc = ss_covis_set_map_rows(c, &problem, 1, n_kf, nblk, pr, obs, n_obs, nullptr, check_right, p->descriptor != 0 ? obs_row : nullptr);
    if (rc != SS_OK) return rc;
    const std::string msg = refresh_call_error("ss_refresh", n_kf, c->covis_max_row, rows_per_frame, p);
    if (!msg.empty()) return fail(c, SS_ERR_INVALID_ARG, msg);
    std::vector<int32_t> np((size_t)nblk);
    for (int b = 0; b < nblk; b++) np[(size_t)b] = std::min(pr, n_points - b * pr);
    const size_t N = (size_t)n_points, R = (size_t)nblk * pr, D = p->descriptor != 0 ? (size_t)n_kf * rows_per_frame * 32 : 0;
    enum { PTS, PDESC, NPTS, REF, SEL, DESC, INFO, SUM, PIECES };
    io_piece io[PIECES] = {{points, points, R * 32, N * 32},
                           {p->descriptor != 0 ? point_desc : nullptr, p->descriptor != 0 ? point_desc : nullptr, R * 32, N * 32},
                           {np.data(), nullptr, (size_t)nblk * 4, (size_t)nblk * 4},
                           {ref_kf, nullptr, ref_kf ? R * 4 : 0, ref_kf ? N * 4 : 0},
                           {select, nullptr, select ? R : 0, select ? N : 0},
                           {desc, nullptr, D, D},
                           {nullptr, info, R * 32, N * 32},
                           {nullptr, summary, (size_t)nblk * 32, (size_t)nblk * 32}};
    rc = io_send(c, c->d_refresh_io, io, PIECES);
    if (rc == SS_OK)
        rc = ss_refresh_device(c, io[PTS].d, p->descriptor != 0 ? io[PDESC].d : nullptr, io[NPTS].d, ref_kf ? io[REF].d : nullptr, select ? io[SEL].d : nullptr,
                               p->descriptor != 0 ? io[DESC].d : nullptr, rows_per_frame, views, p, io[INFO].d, io[SUM].d);
    if (rc != SS_OK) {
        (void)hipStreamSynchronize(c->stream);
        return rc;
    }
    return io_fetch(c, io, PIECES);
}

int ss_refresh_host(const ss_gba_problem *problems, int n_problems, int n_kf, int n_blocks, int point_rows, const ss_gba_obs *obs, int n_obs, int check_right,
                    const int32_t *obs_row, const float *scale, int n_levels, ss_map_point *points, uint8_t *point_desc, const int32_t *n_points, const int32_t *ref_kf,
                    const uint8_t *select, const uint8_t *desc, int rows_per_frame, const ss_proj_view *views, const ss_refresh_params *p, ss_refresh_info *info,
                    ss_refresh_summary *summary, char *err, int err_bytes)
{
    const std::string what = "ss_refresh_host";
    if (const char *msg = refresh_params_error(p)) return gba_refuse(err, err_bytes, msg);
    if (!scale || n_levels < 1 || n_levels > SS_MAX_LEVELS) return gba_refuse(err, err_bytes, "refresh: no pyramid table of 1 .. SS_MAX_LEVELS levels");
    try {
        covis_host_tables t;
        std::string msg = covis_build(problems, n_problems, n_kf, n_blocks, point_rows, obs, n_obs, nullptr, check_right != 0, n_levels, t, obs_row);
        if (!msg.empty()) return gba_refuse(err, err_bytes, msg);
        if (n_problems == 0 || (p->descriptor != 0 && !obs_row)) {
            (void)gba_refuse(err, err_bytes, n_problems == 0 ? what + ": no map" : what + ": the map has no rows, which descriptor needs");
            return SS_ERR_STATE;
        }
        msg = refresh_call_error(what, n_kf, t.max_row, rows_per_frame, p);
        if (msg.empty() && (!points || !n_points || !views || !info || !summary || (p->descriptor != 0 && (!desc || !point_desc)))) msg = what + ": NULL buffer";
        if (!msg.empty()) return gba_refuse(err, err_bytes, msg);
        const ss_covis_tab m = t.view();
        std::vector<float> ow((size_t)n_kf * 3 + 1);
        for (int k = 0; k < n_kf; k++) memcpy(&ow[(size_t)k * 3], views[k].ow, 12);
        ss_refresh_host_in in;
        in.pt_row = t.pt_row.data(), in.n_points = n_points, in.ref_kf = ref_kf, in.select = select, in.desc = desc, in.rows_per_frame = rows_per_frame;
        in.ow = ow.data(), in.scale = scale, in.n_levels = n_levels, in.geometry = p->geometry, in.descriptor = p->descriptor;
        for (int b = 0; b < n_blocks; b++) {
            for (int i = 0; i < point_rows; i++) ss_refresh_row_host(m, in, b, i, points, point_desc, info);
            ss_refresh_summary_host(m, b, n_points[b], info, summary + b);
        }
    } catch (const std::bad_alloc &) {
        return SS_ERR_NO_MEMORY;
    }
    return SS_OK;
}

/* ---- place recognition (csrc/ss_place.hip, csrc/ss_place_steps.h) ---- */
/* the message of the first rule p breaks, or NULL; needs no context */
static const char *place_params_error(const ss_place_params *p)
{
    if (!p) return "place: params is NULL";
    if (p->min_score_mode != 0 && p->min_score_mode != 1) return "place: min_score_mode must be 0 or 1";
    if (!std::isfinite(p->min_score)) return "place: min_score must be finite";
    if (p->n_best < 0 || p->n_best > SS_PLACE_MAX_CANDIDATES) return "place: n_best must be 0 .. SS_PLACE_MAX_CANDIDATES";
    if (p->scope != 0 && p->scope != 1) return "place: scope must be 0 or 1";
    if (!(p->common_ratio >= 0.0f && p->common_ratio <= 1.0f)) return "place: common_ratio must be 0 .. 1";
    if (!(p->retain_ratio >= 0.0f && p->retain_ratio <= 1.0f)) return "place: retain_ratio must be 0 .. 1";
    if (p->reserved[0] != 0 || p->reserved[1] != 0) return "place: the reserved fields must be 0";
    return nullptr;
}

int ss_place_params_default(ss_place_params *p)
{
    if (!p) return SS_ERR_INVALID_ARG;
    *p = ss_place_params{1, 0.0f, 0, 1, 0.8f, 0.75f, {0, 0}};
    return SS_OK;
}

/* The checks of a database (`what` heads the messages), the rows' problems into row_prob and the problems' (first_kf, n_kf) into
 * prob.  The message of the first rule that is broken, or empty */
static std::string place_db_error(const std::string &what, bool arrays, int n_db, int stride, int n_words, const ss_gba_problem *problems, int n_problems,
                                  std::vector<int32_t> &row_prob, std::vector<int32_t> &prob)
{
    if (n_db < 0 || n_db > SS_PLACE_MAX_DB) return what + ": n_db " + std::to_string(n_db) + " outside 0 .. SS_PLACE_MAX_DB (" + std::to_string(SS_PLACE_MAX_DB) + ")";
    if (stride < 1) return what + ": stride " + std::to_string(stride) + " must be >= 1";
    if ((int64_t)n_db * stride > INT32_MAX) return what + ": n_db * stride must be below 2^31";
    if (n_words < 1 || n_words > SS_VOCAB_MAX_NODES) return what + ": n_words " + std::to_string(n_words) + " outside 1 .. SS_VOCAB_MAX_NODES (" + std::to_string(SS_VOCAB_MAX_NODES) + ")";
    if (n_problems < 0) return what + ": n_problems must be >= 0";
    if (n_problems > 0 && !problems) return what + ": problems is NULL";
    if (n_db > 0 && !arrays) return what + ": db_word, db_value or db_count is NULL";
    row_prob.assign((size_t)n_db, -1), prob.assign((size_t)n_problems * 2 + 2, 0);
    for (int q = 0; q < n_problems; q++) {
        const ss_gba_problem &b = problems[q];
        const std::string head = what + ": problems[" + std::to_string(q) + "]: ";
        if (b.n_kf < 1 || b.n_kf > SS_GBA_MAX_KF) return head + "n_kf " + std::to_string(b.n_kf) + " outside 1 .. SS_GBA_MAX_KF (" + std::to_string(SS_GBA_MAX_KF) + ")";
        if (b.first_kf < 0 || b.first_kf > n_db - b.n_kf)
            return head + "keyframes " + std::to_string(b.first_kf) + " .. + " + std::to_string(b.n_kf) + " lie outside the call's n_db " + std::to_string(n_db);
        for (int k = b.first_kf; k < b.first_kf + b.n_kf; k++) {
            if (row_prob[(size_t)k] >= 0) return head + "keyframe " + std::to_string(k) + " belongs to problem " + std::to_string(row_prob[(size_t)k]) + " already";
            row_prob[(size_t)k] = q;
        }
        prob[(size_t)q * 2] = b.first_kf, prob[(size_t)q * 2 + 1] = b.n_kf;
    }
    return std::string();
}

/* the checks of a call's queries against a database of n_db rows whose problems are row_prob, or empty */
static std::string place_query_error(const std::string &what, int n_db, int n_problems, const int32_t *row_prob, bool vectors, int q_stride, int n_q, const int32_t *q_kf,
                                     const int32_t *q_problem, bool have_q_nb, bool have_q_row, int q_cap, bool have_nb, int nb_cap, const ss_place_params *p, int cand_cap,
                                     bool outputs)
{
    if (const char *msg = place_params_error(p)) return msg;
    if (n_q < 0 || n_q > SS_PLACE_MAX_QUERIES) return what + ": n_q " + std::to_string(n_q) + " outside 0 .. SS_PLACE_MAX_QUERIES (" + std::to_string(SS_PLACE_MAX_QUERIES) + ")";
    if (q_stride < 1) return what + ": q_stride " + std::to_string(q_stride) + " must be >= 1";
    if (cand_cap < 1 || cand_cap > SS_PLACE_MAX_CANDIDATES)
        return what + ": cand_cap " + std::to_string(cand_cap) + " outside 1 .. SS_PLACE_MAX_CANDIDATES (" + std::to_string(SS_PLACE_MAX_CANDIDATES) + ")";
    if (nb_cap < 1 || nb_cap > SS_PLACE_MAX_NEIGHBOURS)
        return what + ": nb_cap " + std::to_string(nb_cap) + " outside 1 .. SS_PLACE_MAX_NEIGHBOURS (" + std::to_string(SS_PLACE_MAX_NEIGHBOURS) + ")";
    if (have_q_nb != have_q_row) return what + ": q_nb and q_row must both be given or both be NULL";
    if (have_q_nb && (q_cap < 1 || q_cap > SS_PLACE_MAX_NEIGHBOURS))
        return what + ": q_cap " + std::to_string(q_cap) + " outside 1 .. SS_PLACE_MAX_NEIGHBOURS (" + std::to_string(SS_PLACE_MAX_NEIGHBOURS) + ")";
    if (n_q == 0) return std::string();
    if (!vectors) return what + ": q_word, q_value or q_count is NULL";
    if (!q_kf) return what + ": q_kf is NULL";
    if (!q_problem) return what + ": q_problem is NULL";
    if (!have_nb) return what + ": nb is NULL";
    if (!outputs) return what + ": cand or summary is NULL";
    for (int q = 0; q < n_q; q++) {
        const std::string head = what + ": query " + std::to_string(q) + ": ";
        if (q_kf[q] < -1 || q_kf[q] >= n_db) return head + "q_kf " + std::to_string(q_kf[q]) + " outside -1 .. n_db - 1 (" + std::to_string(n_db - 1) + ")";
        if (q_problem[q] < 0 || q_problem[q] >= n_problems)
            return head + "q_problem " + std::to_string(q_problem[q]) + " outside the table's " + std::to_string(n_problems) + " problems";
        if (q_kf[q] >= 0 && row_prob[q_kf[q]] != q_problem[q])
            return head + "q_problem " + std::to_string(q_problem[q]) + " contradicts q_kf " + std::to_string(q_kf[q]) + ", a row of problem " + std::to_string(row_prob[q_kf[q]]);
    }
    return std::string();
}

static void place_clear(ss_ctx *c)
{
    c->place_db = ss_place_db();
    c->place_row_prob.clear();
}

static int place_set_database(ss_ctx *c, const void *d_db_word, const void *d_db_value, const void *d_db_count, const void *d_db_skip, int n_db, int stride, int n_words,
                              const ss_gba_problem *problems, int n_problems)
{
    const std::string what = "ss_place_set_database";
    std::vector<int32_t> row_prob, prob;
    const std::string msg = place_db_error(what, d_db_word && d_db_value && d_db_count, n_db, stride, n_words, problems, n_problems, row_prob, prob);
    if (!msg.empty()) return fail(c, SS_ERR_INVALID_ARG, msg);
    if (n_db == 0) {
        place_clear(c);
        return SS_OK;
    }
    place_clear(c); /* from here on the buffers of the database it found may move */
    const size_t o_prob = ((size_t)n_db * 4 + 15) & ~(size_t)15;
    int rc = staged_upload(c, c->place_tab, o_prob + prob.size() * 4, [&](uint8_t *h) {
        memcpy(h, row_prob.data(), (size_t)n_db * 4);
        memcpy(h + o_prob, prob.data(), prob.size() * 4);
    });
    if (rc != SS_OK) return rc;
    ssk_place_lists b;
    b.word = (const int32_t *)d_db_word, b.count = (const int32_t *)d_db_count, b.n_db = n_db, b.stride = stride, b.n_words = n_words;
    const size_t entries = (size_t)n_db * stride, W = (size_t)n_words + 1;
    rc = carve_from(c, c->d_place_lists, [&](carve &w) {
        b.off = w.take<int32_t>(W * 4), b.cursor = w.take<int32_t>(W * 4), b.list = w.take<int32_t>((entries + 1) * 4);
        b.sums = w.take<int32_t>(ssk_place_scan_sums(n_words) * 4);
    });
    if (rc != SS_OK) return rc;
    hipError_t e;
    {
        /* the stage's bytes: every entry's word twice, its row written once, the counts three times and the cursors twice */
        stage_timer tm(c, "place_build", (int64_t)entries * 12 + (int64_t)W * 20);
        e = (hipError_t)ssk_place_build(c->stream, b);
    }
    HIP_TRY(c, e);
    HIP_TRY(c, hipGetLastError());
    ss_place_db &db = c->place_db;
    db.word = b.word, db.value = (const double *)d_db_value, db.count = b.count, db.skip = (const uint8_t *)d_db_skip;
    db.n_db = n_db, db.stride = stride, db.n_words = n_words, db.n_problems = n_problems;
    db.row_prob = c->place_tab.as<int32_t>(), db.prob = c->place_tab.as<int32_t>(o_prob);
    db.off = b.off, db.list = b.list;
    c->place_row_prob.swap(row_prob);
    return SS_OK;
}

int ss_place_set_database(ss_ctx *c, const void *d_db_word, const void *d_db_value, const void *d_db_count, const void *d_db_skip, int n_db, int stride, int n_words,
                          const ss_gba_problem *problems, int n_problems)
{
    if (!c) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    try {
        return place_set_database(c, d_db_word, d_db_value, d_db_count, d_db_skip, n_db, stride, n_words, problems, n_problems);
    } catch (const std::bad_alloc &) {
        return fail(c, SS_ERR_NO_MEMORY, "place: no host memory for the tables of the database");
    }
}

int ss_place_query_device(ss_ctx *c, const void *d_q_word, const void *d_q_value, const void *d_q_count, int q_stride, int n_q, const int32_t *q_kf, const int32_t *q_problem,
                          const void *d_q_nb, const void *d_q_row, int q_cap, const void *d_nb, int nb_cap, const ss_place_params *params, int cand_cap, void *d_cand,
                          void *d_summary, void *d_words, void *d_score)
{
    if (!c) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    const std::string what = "ss_place_query_device";
    if (const char *msg = place_params_error(params)) return fail(c, SS_ERR_INVALID_ARG, msg);
    const ss_place_db &db = c->place_db;
    if (db.n_db == 0) return fail(c, SS_ERR_STATE, what + ": no database (ss_place_set_database)");
    const std::string msg = place_query_error(what, db.n_db, db.n_problems, c->place_row_prob.data(), d_q_word && d_q_value && d_q_count, q_stride, n_q, q_kf, q_problem,
                                              d_q_nb != nullptr, d_q_row != nullptr, q_cap, d_nb != nullptr, nb_cap, params, cand_cap, d_cand && d_summary);
    if (!msg.empty()) return fail(c, SS_ERR_INVALID_ARG, msg);
    if (n_q == 0) return SS_OK;
    const size_t Q = (size_t)n_q, T = Q * (size_t)db.n_db;
    int rc = staged_upload(c, c->place_call_tab, Q * 8, [&](uint8_t *h) {
        memcpy(h, q_kf, Q * 4);
        memcpy(h + Q * 4, q_problem, Q * 4);
    });
    if (rc != SS_OK) return rc;
    ssk_place_call g;
    g.db = db;
    g.q_word = (const int32_t *)d_q_word, g.q_value = (const double *)d_q_value, g.q_count = (const int32_t *)d_q_count;
    g.q_stride = q_stride, g.n_q = n_q, g.q_cap = d_q_nb ? q_cap : 0, g.nb_cap = nb_cap, g.cand_cap = cand_cap;
    g.q_kf = c->place_call_tab.as<int32_t>(), g.q_problem = c->place_call_tab.as<int32_t>(Q * 4);
    g.q_nb = (const int32_t *)d_q_nb, g.q_row = (const ss_covis_row *)d_q_row, g.nb = (const int32_t *)d_nb;
    g.p = *params, g.cand = (ss_place_cand *)d_cand, g.summary = (ss_place_summary *)d_summary;
    g.words = (int32_t *)d_words, g.score = (float *)d_score;
    rc = carve_from(c, c->d_place_ws, [&](carve &w) {
        g.flags = w.take<uint8_t>(T), g.star = w.take<uint32_t>(T * 4), g.surv = w.take<int32_t>(T * 4), g.state = w.take<int32_t>(Q * 32);
        if (!d_words) g.words = w.take<int32_t>(T * 4);
        if (!d_score) g.score = w.take<float>(T * 4);
    });
    if (rc != SS_OK) return rc;
    /* the stages' bytes: the tables each writes or reads whole; the lists and vectors it follows are the data's */
    static const char *const stage_name[6] = {"place_flags", "place_vote", "place_reduce", "place_score", "place_seeds", "place_final"};
    const int64_t table_bytes[6] = {13, 5, 9, 4, 8, 8};
    for (int stage = 0; stage < 6; stage++) {
        stage_timer tm(c, stage_name[stage], (int64_t)T * table_bytes[stage]);
        ssk_place_query(c->stream, g, stage);
    }
    HIP_TRY(c, hipGetLastError());
    return SS_OK;
}

int ss_place(ss_ctx *c, const int32_t *db_word, const double *db_value, const int32_t *db_count, const uint8_t *db_skip, int n_db, int stride, int n_words,
             const ss_gba_problem *problems, int n_problems, const int32_t *q_word, const double *q_value, const int32_t *q_count, int q_stride, int n_q,
             const int32_t *q_kf, const int32_t *q_problem, const int32_t *q_nb, const ss_covis_row *q_row, int q_cap, const int32_t *nb, int nb_cap,
             const ss_place_params *params, int cand_cap, ss_place_cand *cand, ss_place_summary *summary, int32_t *words, float *score)
{
    if (!c) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    const std::string what = "ss_place";
    try {
        std::vector<int32_t> row_prob, prob;
        std::string msg = place_db_error(what, db_word && db_value && db_count, n_db, stride, n_words, problems, n_problems, row_prob, prob);
        if (msg.empty() && n_db == 0) msg = what + ": n_db must be >= 1";
        if (msg.empty())
            msg = place_query_error(what, n_db, n_problems, row_prob.data(), q_word && q_value && q_count, q_stride, n_q, q_kf, q_problem, q_nb != nullptr, q_row != nullptr, q_cap,
                                    nb != nullptr, nb_cap, params, cand_cap, cand && summary);
        if (!msg.empty()) return fail(c, SS_ERR_INVALID_ARG, msg);
        if (n_q == 0) return SS_OK;
        const size_t D = (size_t)n_db * stride, Q = (size_t)n_q, QV = Q * q_stride, T = Q * n_db, QN = q_nb ? Q * q_cap * 8 : 0;
        enum { DW, DV, DC, DS, QW, QVAL, QC, QNB, QROW, NB, CAND, SUM, WORDS, SCORE, PIECES };
        io_piece io[PIECES] = {{db_word, nullptr, D * 4, D * 4},
                               {db_value, nullptr, D * 8, D * 8},
                               {db_count, nullptr, (size_t)n_db * 4, (size_t)n_db * 4},
                               {db_skip, nullptr, db_skip ? (size_t)n_db : 0, db_skip ? (size_t)n_db : 0},
                               {q_word, nullptr, QV * 4, QV * 4},
                               {q_value, nullptr, QV * 8, QV * 8},
                               {q_count, nullptr, Q * 4, Q * 4},
                               {q_nb, nullptr, QN, QN},
                               {q_row, nullptr, q_nb ? Q * sizeof(ss_covis_row) : 0, q_nb ? Q * sizeof(ss_covis_row) : 0},
                               {nb, nullptr, (size_t)n_db * nb_cap * 8, (size_t)n_db * nb_cap * 8},
                               {nullptr, cand, Q * cand_cap * sizeof(ss_place_cand), Q * cand_cap * sizeof(ss_place_cand)},
                               {nullptr, summary, Q * sizeof(ss_place_summary), Q * sizeof(ss_place_summary)},
                               {nullptr, words, words ? T * 4 : 0, words ? T * 4 : 0},
                               {nullptr, score, score ? T * 4 : 0, score ? T * 4 : 0}};
        int rc = io_send(c, c->d_place_io, io, PIECES);
        if (rc == SS_OK) rc = place_set_database(c, io[DW].d, io[DV].d, io[DC].d, db_skip ? io[DS].d : nullptr, n_db, stride, n_words, problems, n_problems);
        if (rc == SS_OK)
            rc = ss_place_query_device(c, io[QW].d, io[QVAL].d, io[QC].d, q_stride, n_q, q_kf, q_problem, q_nb ? io[QNB].d : nullptr, q_nb ? io[QROW].d : nullptr, q_cap, io[NB].d,
                                       nb_cap, params, cand_cap, io[CAND].d, io[SUM].d, words ? io[WORDS].d : nullptr, score ? io[SCORE].d : nullptr);
        if (rc != SS_OK) {
            (void)hipStreamSynchronize(c->stream);
            place_clear(c);
            return rc;
        }
        rc = io_fetch(c, io, PIECES);
        place_clear(c); /* the database's arrays were this call's copies */
        return rc;
    } catch (const std::bad_alloc &) {
        return fail(c, SS_ERR_NO_MEMORY, "place: no host memory for the tables of the database");
    }
}

int ss_place_query_host(const int32_t *db_word, const double *db_value, const int32_t *db_count, const uint8_t *db_skip, int n_db, int stride, int n_words,
                        const ss_gba_problem *problems, int n_problems, const int32_t *q_word, const double *q_value, const int32_t *q_count, int q_stride, int n_q,
                        const int32_t *q_kf, const int32_t *q_problem, const int32_t *q_nb, const ss_covis_row *q_row, int q_cap, const int32_t *nb, int nb_cap,
                        const ss_place_params *params, int cand_cap, ss_place_cand *cand, ss_place_summary *summary, int32_t *words, float *score, char *err, int err_bytes)
{
    const std::string what = "ss_place_query_host";
    try {
        ss_place_host_db h;
        std::string msg = place_db_error(what, db_word && db_value && db_count, n_db, stride, n_words, problems, n_problems, h.row_prob, h.prob);
        if (msg.empty() && n_db == 0) msg = what + ": n_db must be >= 1";
        if (msg.empty())
            msg = place_query_error(what, n_db, n_problems, h.row_prob.data(), q_word && q_value && q_count, q_stride, n_q, q_kf, q_problem, q_nb != nullptr, q_row != nullptr,
                                    q_cap, nb != nullptr, nb_cap, params, cand_cap, cand && summary);
        if (!msg.empty()) return gba_refuse(err, err_bytes, msg);
        ss_place_db &db = h.view;
        db.word = db_word, db.value = db_value, db.count = db_count, db.skip = db_skip;
        db.n_db = n_db, db.stride = stride, db.n_words = n_words, db.n_problems = n_problems;
        db.row_prob = h.row_prob.data(), db.prob = h.prob.data();
        ss_place_build_host(h);
        std::vector<int32_t> w((size_t)n_db);
        std::vector<float> s((size_t)n_db);
        for (int q = 0; q < n_q; q++) {
            const size_t row0 = (size_t)q * n_db;
            ss_place_query_one_host(db, q_word + (size_t)q * q_stride, q_value + (size_t)q * q_stride, ss_place_clamp(q_count[q], q_stride), q_kf[q], q_problem[q],
                                    q_nb ? q_nb + (size_t)q * q_cap * 2 : nullptr, q_nb ? ss_place_clamp(q_row[q].n_written, q_cap) : 0, nb, nb_cap, *params, cand_cap,
                                    cand + (size_t)q * cand_cap, summary + q, words ? words + row0 : w.data(), score ? score + row0 : s.data());
        }
    } catch (const std::bad_alloc &) {
        return SS_ERR_NO_MEMORY;
    }
    return SS_OK;
}

/* ---- undistorted keypoints, image bounds, RGB-D depth (csrc/ss_undistort.hip, csrc/ss_undistort_steps.h) ---- */
int ss_undistort_bounds_host(const ss_camera *cam, float out[4])
{
    if (!cam || !out || cam->width <= 0 || cam->height <= 0) return SS_ERR_INVALID_ARG;
    const ss_undist_cam u = ss_undist_cam_of(*cam);
    if (!ss_undist_cam_finite(u)) return SS_ERR_INVALID_ARG;
    ss_undist_bounds(u, cam->width, cam->height, out);
    return SS_OK;
}

int ss_proj_view_set_bounds(ss_proj_view *view, const ss_camera *cam)
{
    if (!view) return SS_ERR_INVALID_ARG;
    float b[4];
    const int rc = ss_undistort_bounds_host(cam, b);
    if (rc != SS_OK) return rc;
    view->min_x = b[0], view->max_x = b[1], view->min_y = b[2], view->max_y = b[3];
    return SS_OK;
}

int ss_undistort_host(const ss_camera *cam, const ss_keypoint *kp, int n, ss_keypoint *out)
{
    if (!cam || n < 0 || (n > 0 && (!kp || !out))) return SS_ERR_INVALID_ARG;
    if (!ss_undist_focal_ok(cam->fx, cam->fy)) return SS_ERR_INVALID_ARG;
    const ss_undist_cam u = ss_undist_cam_of(*cam);
    for (int i = 0; i < n; i++) {
        ss_keypoint k = kp[i]; /* out may be kp */
        ss_undist_point(u, k.x, k.y, &k.x, &k.y);
        out[i] = k;
    }
    return SS_OK;
}

/* The launch of an undistortion call whose device operands are filled in: the cameras checked and staged, one per frame */
static int undistort_run(ss_ctx *c, ssk_undistort_call &g, const std::string &what, const ss_camera *cams, int n_cams)
{
    if (!cams) return fail(c, SS_ERR_INVALID_ARG, what + ": cams is NULL");
    if (n_cams != 1 && n_cams != g.n_frames) return fail(c, SS_ERR_INVALID_ARG, what + ": n_cams " + std::to_string(n_cams) + " is neither 1 nor n_frames (" + std::to_string(g.n_frames) + ")");
    for (int k = 0; k < n_cams; k++)
        if (!ss_undist_focal_ok(cams[k].fx, cams[k].fy)) return fail(c, SS_ERR_INVALID_ARG, what + ": cams[" + std::to_string(k) + "]: fx and fy must be finite and not 0");
    int rc = call_count_ok(c, what, g.n_frames, "frames");
    if (rc != SS_OK) return rc;
    rc = staged_upload(c, c->undist_tab, (size_t)g.n_frames * sizeof(ss_undist_cam), [&](uint8_t *h) {
        ss_undist_cam *t = (ss_undist_cam *)h;
        for (int b = 0; b < g.n_frames; b++) t[b] = ss_undist_cam_of(cams[n_cams == 1 ? 0 : b]);
    });
    if (rc != SS_OK) return rc;
    g.cams = c->undist_tab.as<ss_undist_cam>();
    {
        /* per row: x and y read and written, the raw save or the rest of the record on top; the counts and the cameras */
        const int64_t per_row = 16 + (g.raw_xy ? 8 : 0) + ((const void *)g.kp_out != (const void *)g.kp ? 32 : 0);
        stage_timer t(c, g.raw_xy ? "undistort_in_place" : "undistort", (int64_t)g.n_frames * g.rows * per_row + g.n_frames * (int64_t)(4 + sizeof(ss_undist_cam)));
        ssk_undistort(c->stream, g);
    }
    HIP_TRY(c, hipGetLastError());
    return SS_OK;
}

int ss_undistort_pairs_device(ss_ctx *c, const void *d_kp, const void *d_n_kp, int n_frames, int rows_per_frame, const ss_camera *cams, int n_cams,
                              void *d_kp_out)
{
    if (!c) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    const std::string what = "ss_undistort_pairs_device";
    const int rc = pairs_shape(c, what, "frame", n_frames, rows_per_frame);
    if (rc != SS_OK) return rc;
    if (n_frames == 0) return SS_OK;
    if (!d_kp || !d_n_kp || !d_kp_out) return fail(c, SS_ERR_INVALID_ARG, what + ": NULL buffer");
    ssk_undistort_call g;
    g.n_frames = n_frames, g.rows = rows_per_frame;
    g.kp = (const ss_keypoint *)d_kp, g.n_kp = (const int32_t *)d_n_kp, g.kp_out = (ss_keypoint *)d_kp_out;
    return undistort_run(c, g, what, cams, n_cams);
}

int ss_undistort_batch_device(ss_ctx *c, const ss_camera *cams, int n_cams, void *d_kp_out)
{
    if (!c) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    const std::string what = "ss_undistort_batch_device";
    if (!have_batch(c, what.c_str())) return SS_ERR_STATE;
    if (!cams) {
        if (!c->calibrated) return fail(c, SS_ERR_NOT_CALIBRATED, what + ": cams is NULL and no calibration has been set");
        cams = &c->cam, n_cams = 1;
    }
    const bool in_place = d_kp_out == nullptr;
    if (in_place && c->batch_undistorted) return fail(c, SS_ERR_STATE, what + ": this batch has been undistorted in place already");
    ssk_undistort_call g;
    g.n_frames = c->last_n_frames, g.rows = c->hg.kcap;
    g.kp = c->ws.kps, g.n_kp = c->ws.n_kp;
    int rc = flagged_frame_error(c, c->batch_test_flagged, &g.frame_error);
    if (rc != SS_OK) return rc;
    if (in_place) {
        rc = raw_xy_buffer(c);
        if (rc != SS_OK) return rc;
        g.kp_out = c->ws.kps, g.raw_xy = c->d_raw_xy;
    } else {
        g.kp_out = (ss_keypoint *)d_kp_out;
    }
    rc = undistort_run(c, g, what, cams, n_cams);
    if (rc == SS_OK && in_place) c->batch_undistorted = true;
    return rc;
}

int ss_get_batch_raw_xy(ss_ctx *c, const float **d_xy)
{
    if (!c || !d_xy) return SS_ERR_INVALID_ARG;
    if (!c->have_geom || c->last_n_frames <= 0 || !c->batch_undistorted)
        return fail(c, SS_ERR_STATE, "ss_get_batch_raw_xy: the current batch has not been undistorted in place");
    *d_xy = (const float *)c->d_raw_xy;
    return SS_OK;
}

int ss_depth_params_from_camera(const ss_camera *cam, int depth_type, ss_depth_params *out)
{
    if (!cam || !out || (depth_type != 0 && depth_type != 1)) return SS_ERR_INVALID_ARG;
    const double bf = cam->baseline * cam->fx;
    out->bf = (float)bf;
    out->depth_map_factor = (float)cam->depth_map_factor;
    out->close_limit = (float)(bf * cam->th_depth / cam->fx);
    out->depth_type = depth_type;
    return SS_OK;
}

/* the message of the first rule the shape of a depth call breaks, or NULL; needs no context */
static const char *depth_shape_error(const ss_depth_params *p, const void *depth, int width, int height, int64_t row_stride, int64_t frame_stride, int n_frames)
{
    if (!p) return "depth: params is NULL";
    if (p->depth_type != 0 && p->depth_type != 1) return "depth: depth_type must be 0 (float32) or 1 (uint16)";
    if (!std::isfinite(p->bf) || !std::isfinite(p->depth_map_factor) || !std::isfinite(p->close_limit)) return "depth: bf, depth_map_factor and close_limit must be finite";
    if (width < 1 || height < 1 || width > (1 << 24) || height > (1 << 24)) return "depth: width and height must be 1 .. 16777216";
    const int64_t sample = p->depth_type == 1 ? 2 : 4;
    if (row_stride < width * sample || (n_frames > 1 && frame_stride < row_stride * (height - 1) + width * sample)) return "depth: strides smaller than the frame";
    if (row_stride > ((int64_t)1 << 40) || frame_stride > ((int64_t)1 << 40)) return "depth: strides above 2^40";
    if (row_stride % sample != 0 || (n_frames > 1 && frame_stride % sample != 0) || (uintptr_t)depth % (uintptr_t)sample != 0)
        return "depth: the base and the strides must be multiples of the sample size";
    return nullptr;
}

int ss_depth_host(const ss_depth_params *p, const void *depth, int width, int height, int64_t row_stride, const ss_keypoint *kp_raw, const ss_keypoint *kp_un,
                  int n, float *right, float *depth_out, ss_depth_summary *summary)
{
    if (!depth || n < 0 || (n > 0 && (!kp_raw || !right || !depth_out))) return SS_ERR_INVALID_ARG;
    if (depth_shape_error(p, depth, width, height, row_stride, 0, 1)) return SS_ERR_INVALID_ARG;
    const float inv = ss_depth_inv(p->depth_map_factor);
    const bool scale_float = ss_depth_scales_float(inv);
    ss_depth_summary s = {SS_OK, n, 0, 0};
    for (int i = 0; i < n; i++) {
        float d = 0.0f;
        const bool have = ss_depth_sample((const uint8_t *)depth, width, height, row_stride, p->depth_type, inv, scale_float, kp_raw[i].x, kp_raw[i].y, &d);
        ss_depth_row(have, d, (kp_un ? kp_un : kp_raw)[i].x, p->bf, &right[i], &depth_out[i]);
        s.n_depth += depth_out[i] > 0.0f;
        s.n_close += depth_out[i] > 0.0f && depth_out[i] < p->close_limit;
    }
    if (summary) *summary = s;
    return SS_OK;
}

/* The two launches of a depth call whose keypoint side is filled in */
static int depth_run(ss_ctx *c, ssk_depth_call &g, const std::string &what, const ss_depth_params *p, const void *d_depth, int width, int height, int64_t row_stride,
                     int64_t frame_stride, void *d_right, void *d_depth_out, void *d_summary)
{
    if (!d_depth || !d_right || !d_depth_out || !d_summary) return fail(c, SS_ERR_INVALID_ARG, what + ": NULL buffer");
    if (const char *msg = depth_shape_error(p, d_depth, width, height, row_stride, frame_stride, g.n_frames)) return fail(c, SS_ERR_INVALID_ARG, what + ": " + msg);
    const int rc = call_count_ok(c, what, g.n_frames, "frames");
    if (rc != SS_OK) return rc;
    g.width = width, g.height = height;
    g.depth = (const uint8_t *)d_depth, g.row_stride = row_stride, g.frame_stride = g.n_frames > 1 ? frame_stride : 0;
    g.p = *p;
    g.inv = ss_depth_inv(p->depth_map_factor), g.scale_float = ss_depth_scales_float(g.inv);
    g.right = (float *)d_right, g.depth_out = (float *)d_depth_out, g.summary = (ss_depth_summary *)d_summary;
    {
        /* per row: the raw pair, the undistorted x, one sample, the two planes; per frame its count and summary */
        const int64_t sample = p->depth_type == 1 ? 2 : 4;
        stage_timer t(c, "depth_lookup", (int64_t)g.n_frames * g.rows * (8 + 4 + sample + 8) + g.n_frames * (int64_t)(4 + sizeof(ss_depth_summary)));
        ssk_depth(c->stream, g);
    }
    HIP_TRY(c, hipGetLastError());
    return SS_OK;
}

int ss_depth_pairs_device(ss_ctx *c, const ss_depth_params *p, const void *d_depth, int width, int height, int64_t row_stride, int64_t frame_stride,
                          const void *d_kp_raw, const void *d_kp_un, const void *d_n_kp, int n_frames, int rows_per_frame, void *d_right, void *d_depth_out,
                          void *d_summary)
{
    if (!c) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    const std::string what = "ss_depth_pairs_device";
    const int rc = pairs_shape(c, what, "frame", n_frames, rows_per_frame);
    if (rc != SS_OK) return rc;
    if (n_frames == 0) return SS_OK;
    if (!d_kp_raw || !d_n_kp) return fail(c, SS_ERR_INVALID_ARG, what + ": NULL buffer");
    ssk_depth_call g;
    g.n_frames = n_frames, g.rows = rows_per_frame;
    g.kp_raw = (const ss_keypoint *)d_kp_raw, g.kp_un = d_kp_un ? (const ss_keypoint *)d_kp_un : g.kp_raw, g.n_kp = (const int32_t *)d_n_kp;
    return depth_run(c, g, what, p, d_depth, width, height, row_stride, frame_stride, d_right, d_depth_out, d_summary);
}

int ss_depth_batch_device(ss_ctx *c, const ss_depth_params *p, const void *d_depth, int width, int height, int64_t row_stride, int64_t frame_stride, void *d_right,
                          void *d_depth_out, void *d_summary)
{
    if (!c) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    const std::string what = "ss_depth_batch_device";
    if (!have_batch(c, what.c_str())) return SS_ERR_STATE;
    ssk_depth_call g;
    g.n_frames = c->last_n_frames, g.rows = c->hg.kcap;
    g.kp_raw = g.kp_un = c->ws.kps, g.n_kp = c->ws.n_kp;
    if (c->batch_undistorted) g.raw_xy = c->d_raw_xy;
    const int rc = flagged_frame_error(c, c->batch_test_flagged, &g.frame_error);
    if (rc != SS_OK) return rc;
    return depth_run(c, g, what, p, d_depth, width, height, row_stride, frame_stride, d_right, d_depth_out, d_summary);
}

/* ---- map points from depth (csrc/ss_unproject.hip, csrc/ss_unproject_steps.h) ---- */
int ss_unproject_view_init(const ss_camera *cam, const double rcw[9], const double tcw[3], ss_unproject_view *out)
{
    if (!cam || !rcw || !tcw || !out) return SS_ERR_INVALID_ARG;
    ss_unproject_view &v = *out;
    for (int k = 0; k < 9; k++) v.rcw[k] = rcw[k];
    for (int k = 0; k < 3; k++) {
        v.tcw[k] = tcw[k];
        v.ow[k] = -((rcw[k] * tcw[0] + rcw[3 + k] * tcw[1]) + rcw[6 + k] * tcw[2]);
    }
    v.fx = cam->fx, v.fy = cam->fy, v.cx = cam->cx, v.cy = cam->cy, v.invfx = 1.0 / cam->fx, v.invfy = 1.0 / cam->fy;
    return SS_OK;
}

/* the message of the first rule the parameters or the depth plane break, or NULL; needs no context */
static const char *unproject_error(const ss_unproject_params *p, const void *depth, int64_t depth_stride)
{
    if (!p) return "unproject: params is NULL";
    if (p->mode != SS_UNPROJECT_ALL && p->mode != SS_UNPROJECT_CLOSE) return "unproject: mode must be SS_UNPROJECT_ALL or SS_UNPROJECT_CLOSE";
    if (p->max_points < 0) return "unproject: max_points must be >= 0";
    if (!std::isfinite(p->close_limit)) return "unproject: close_limit must be finite";
    if (p->reserved != 0) return "unproject: the reserved field must be 0";
    if (depth_stride < 4 || depth_stride % 4 != 0 || depth_stride > ((int64_t)1 << 30)) return "unproject: depth_stride must be a positive multiple of 4";
    if ((uintptr_t)depth % 4 != 0) return "unproject: the depth pointer must be a multiple of 4";
    return nullptr;
}

int ss_unproject_host(const ss_unproject_view *view, const ss_unproject_params *p, const float *scale, int n_levels, const ss_keypoint *kp,
                      const uint8_t *desc, int n, int rows, const void *depth, int64_t depth_stride, const uint8_t *has_point, const uint8_t *outlier,
                      ss_unproject_info *info, ss_map_point *points, uint8_t *point_desc, int32_t *point_rows, int32_t *n_points,
                      ss_unproject_summary *summary)
{
    if (!view || !scale || n_levels < 1 || n_levels > SS_MAX_LEVELS || rows < 0 || rows > SS_GUIDED_MAX_ROWS || !n_points || !summary) return SS_ERR_INVALID_ARG;
    if (rows > 0 && (!kp || !desc || !depth || !info || !points || !point_desc || !point_rows)) return SS_ERR_INVALID_ARG;
    if (unproject_error(p, depth, depth_stride)) return SS_ERR_INVALID_ARG;
    const int nk = ss_unproject_clamp(n, rows);
    ss_unproject_summary s = {SS_OK, nk, 0, 0, 0, 0, 0, 0, 0, 0};
    try {
        std::vector<uint64_t> keys;
        std::vector<int> cls((size_t)nk);
        for (int i = 0; i < nk; i++) {
            const float d = ss_unproject_depth_at((const uint8_t *)depth, depth_stride, i);
            cls[i] = ss_unproject_class(d, kp[i].octave, n_levels);
            s.n_depth += d > 0.0f;
            if (cls[i] != 0) continue;
            keys.push_back(ss_unproject_key(d, i));
            s.n_not_far += d <= p->close_limit;
            if (d < p->close_limit) {
                s.n_close++;
                const bool t = has_point && has_point[i] != 0 && !(outlier && outlier[i] != 0);
                s.n_tracked_close += t, s.n_untracked_close += !t;
            }
        }
        std::sort(keys.begin(), keys.end());
        const int quota = ss_unproject_quota(p->mode, p->max_points, s.n_not_far, (int)keys.size());
        const uint64_t last = quota > 0 ? keys[(size_t)quota - 1] : 0; /* a row is processed iff its key is <= last */
        for (int i = 0; i < rows; i++) {
            int state = -1;
            if (i < nk) {
                const float d = ss_unproject_depth_at((const uint8_t *)depth, depth_stride, i);
                if (cls[i] != 0) state = cls[i];
                else if (!(quota > 0 && ss_unproject_key(d, i) <= last)) state = SS_UNPROJECT_FAR;
                else {
                    s.n_processed++;
                    if (has_point && has_point[i] != 0) {
                        state = SS_UNPROJECT_KEPT;
                        s.n_kept++;
                    } else {
                        const ss_unproject_out r = ss_unproject_point(*view, scale, n_levels, kp[i].x, kp[i].y, kp[i].octave, d);
                        if (r.ok) {
                            state = SS_UNPROJECT_CREATED;
                            points[s.n_created] = r.point;
                            memcpy(point_desc + (size_t)s.n_created * SS_DESC_BYTES, desc + (size_t)i * SS_DESC_BYTES, SS_DESC_BYTES);
                            point_rows[2 * s.n_created] = i, point_rows[2 * s.n_created + 1] = -1;
                            s.n_created++;
                        } else {
                            state = SS_UNPROJECT_DEGENERATE;
                        }
                    }
                }
            }
            info[i].state = state;
        }
    } catch (const std::bad_alloc &) {
        return SS_ERR_NO_MEMORY;
    }
    *n_points = s.n_created;
    *summary = s;
    return SS_OK;
}

/* The launch of an unprojection whose keypoint side is filled in and whose parameters and depth plane the form has checked
 * (unproject_error): the buffers and the depth blocks checked, the views staged, the outputs */
static int unproject_run(ss_ctx *c, ssk_unproject_call &g, const std::string &what, const void *d_depth, int64_t depth_stride, int n_depth_blocks,
                         const int32_t *depth_src, const void *d_has_point, const void *d_outlier, const ss_unproject_view *views, const ss_unproject_params *p, void *d_info, void *d_points,
                         void *d_point_desc, void *d_point_rows, void *d_n_points, void *d_summary)
{
    if (!d_depth || !views || !d_info || !d_points || !d_point_desc || !d_point_rows || !d_n_points || !d_summary)
        return fail(c, SS_ERR_INVALID_ARG, what + ": NULL buffer");
    if (n_depth_blocks < 1) return fail(c, SS_ERR_INVALID_ARG, what + ": n_depth_blocks must be >= 1");
    if (!depth_src && n_depth_blocks < g.n_frames) return fail(c, SS_ERR_INVALID_ARG, what + ": depth_src is NULL and n_depth_blocks is below the frames");
    for (int b = 0; depth_src && b < g.n_frames; b++)
        if (depth_src[b] < -1 || depth_src[b] >= n_depth_blocks)
            return fail(c, SS_ERR_INVALID_ARG, what + ": depth_src[" + std::to_string(b) + "] = " + std::to_string(depth_src[b]) + " names no depth block (" +
                                                   std::to_string(n_depth_blocks) + ")");
    int rc = call_count_ok(c, what, g.n_frames, "frames");
    if (rc != SS_OK) return rc;
    rc = context_pyramid(c, what, &g.n_levels, g.scale);
    if (rc != SS_OK) return rc;
    /* the views, then the depth blocks of the frames */
    const size_t vb = (size_t)g.n_frames * sizeof(ss_unproject_view);
    rc = staged_upload(c, c->unproject_tab, vb + (size_t)g.n_frames * sizeof(int32_t), [&](uint8_t *h) {
        memcpy(h, views, vb);
        int32_t *src = (int32_t *)(h + vb);
        for (int b = 0; b < g.n_frames; b++) src[b] = depth_src ? depth_src[b] : b;
    });
    if (rc != SS_OK) return rc;
    g.views = c->unproject_tab.as<ss_unproject_view>(), g.depth_src = c->unproject_tab.as<int32_t>(vb);
    g.depth = (const uint8_t *)d_depth, g.depth_stride = depth_stride;
    g.has_point = (const uint8_t *)d_has_point, g.outlier = (const uint8_t *)d_outlier;
    g.p = *p;
    g.info = (ss_unproject_info *)d_info;
    g.points = (ss_map_point *)d_points, g.point_desc = (uint8_t *)d_point_desc, g.point_rows = (int32_t *)d_point_rows;
    g.n_points = (int32_t *)d_n_points;
    g.summary = (ss_unproject_summary *)d_summary;
    {
        /* per row: its depth, its octave and its state; what a created row moves (its keypoint, 32 bytes of point, its descriptor
         * twice, its rows) depends on the content; per frame its count, view, point count and summary */
        stage_timer t(c, "unproject", (int64_t)g.n_frames * g.rows * (4 + 4 + 4) +
                                          g.n_frames * (int64_t)(4 + sizeof(ss_unproject_view) + 4 + sizeof(ss_unproject_summary)));
        ssk_unproject(c->stream, g);
    }
    HIP_TRY(c, hipGetLastError());
    return SS_OK;
}

int ss_unproject_pairs_device(ss_ctx *c, const void *d_kp, const void *d_desc, const void *d_n_kp, const void *d_depth, int64_t depth_stride,
                              int n_depth_blocks, const int32_t *depth_src, const void *d_has_point, const void *d_outlier, int n_frames, int rows_per_frame, const ss_unproject_view *views,
                              const ss_unproject_params *p, void *d_info, void *d_points, void *d_point_desc, void *d_point_rows, void *d_n_points,
                              void *d_summary)
{
    if (!c) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    const std::string what = "ss_unproject_pairs_device";
    const int rc = pairs_shape(c, what, "frame", n_frames, rows_per_frame);
    if (rc != SS_OK) return rc;
    if (const char *msg = unproject_error(p, d_depth, depth_stride)) return fail(c, SS_ERR_INVALID_ARG, what + ": " + msg);
    if (n_frames == 0) return SS_OK;
    if (!d_kp || !d_desc || !d_n_kp) return fail(c, SS_ERR_INVALID_ARG, what + ": NULL buffer");
    ssk_unproject_call g;
    g.n_frames = n_frames, g.rows = rows_per_frame;
    g.kp = (const ss_keypoint *)d_kp, g.desc = (const uint8_t *)d_desc, g.n_kp = (const int32_t *)d_n_kp;
    return unproject_run(c, g, what, d_depth, depth_stride, n_depth_blocks, depth_src, d_has_point, d_outlier, views, p, d_info, d_points, d_point_desc, d_point_rows, d_n_points,
                         d_summary);
}

int ss_unproject_batch_device(ss_ctx *c, const void *d_depth, int64_t depth_stride, int n_depth_blocks, const int32_t *depth_src,
                              const void *d_has_point, const void *d_outlier,
                              const ss_unproject_view *views, const ss_unproject_params *p, void *d_info, void *d_points, void *d_point_desc,
                              void *d_point_rows, void *d_n_points, void *d_summary)
{
    if (!c) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    const std::string what = "ss_unproject_batch_device";
    if (!have_batch(c, what.c_str())) return SS_ERR_STATE;
    if (c->hg.kcap > SS_GUIDED_MAX_ROWS) return fail(c, SS_ERR_INVALID_ARG, what + ": kp_capacity " + std::to_string(c->hg.kcap) + " exceeds SS_GUIDED_MAX_ROWS");
    if (const char *msg = unproject_error(p, d_depth, depth_stride)) return fail(c, SS_ERR_INVALID_ARG, what + ": " + msg);
    ssk_unproject_call g;
    g.n_frames = c->last_n_frames, g.rows = c->hg.kcap;
    g.kp = c->ws.kps, g.desc = c->ws.desc, g.n_kp = c->ws.n_kp;
    const int rc = flagged_frame_error(c, c->batch_test_flagged, &g.frame_error);
    if (rc != SS_OK) return rc;
    return unproject_run(c, g, what, d_depth, depth_stride, n_depth_blocks, depth_src, d_has_point, d_outlier, views, p, d_info, d_points, d_point_desc, d_point_rows, d_n_points,
                         d_summary);
}

int ss_unproject(ss_ctx *c, const ss_unproject_view *view, const ss_unproject_params *p, const ss_keypoint *kp, const uint8_t *desc, int n,
                 const void *depth, int64_t depth_stride, const uint8_t *has_point, const uint8_t *outlier, ss_unproject_info *info,
                 ss_map_point *points, uint8_t *point_desc, int32_t *point_rows, int32_t *n_points, ss_unproject_summary *summary)
{
    if (!c) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    const std::string what = "ss_unproject";
    if (n < 0 || n > SS_GUIDED_MAX_ROWS) return fail(c, SS_ERR_INVALID_ARG, what + ": n must be 0 .. SS_GUIDED_MAX_ROWS");
    if (const char *msg = unproject_error(p, depth, depth_stride)) return fail(c, SS_ERR_INVALID_ARG, what + ": " + msg);
    if (!view || !n_points || !summary || (n > 0 && (!kp || !desc || !depth || !info || !points || !point_desc || !point_rows)))
        return fail(c, SS_ERR_INVALID_ARG, what + ": NULL buffer");
    /* one frame of `rows` rows; the depth plane goes up as the caller strides it, so that the device reads what the host would */
    const size_t rows = (size_t)std::max(n, 1), nn = (size_t)n, kb = sizeof(ss_keypoint), stride = (size_t)depth_stride;
    const size_t depth_bytes = nn ? (nn - 1) * stride + 4 : 0;
    const int32_t count = n;
    enum { KP, DESC, DEPTH, HAS, OUT, N, INFO, PTS, PDESC, PROWS, NPTS, SUM, PIECES };
    io_piece io[PIECES] = {{kp, nullptr, rows * kb, nn * kb}, {desc, nullptr, rows * 32, nn * 32}, {depth, nullptr, rows * stride, depth_bytes},
                           {has_point, nullptr, rows, nn}, {outlier, nullptr, rows, nn}, {&count, nullptr, 4, 4},
                           {nullptr, info, rows * sizeof(ss_unproject_info), nn * sizeof(ss_unproject_info)},
                           {nullptr, points, rows * sizeof(ss_map_point), 0}, {nullptr, point_desc, rows * 32, 0}, {nullptr, point_rows, rows * 8, 0},
                           {nullptr, n_points, 4, 4}, {nullptr, summary, sizeof(ss_unproject_summary), sizeof(ss_unproject_summary)}};
    int rc = io_send(c, c->d_unproject_io, io, PIECES);
    if (rc == SS_OK)
        rc = ss_unproject_pairs_device(c, io[KP].d, io[DESC].d, io[N].d, io[DEPTH].d, depth_stride, 1, nullptr, has_point ? io[HAS].d : nullptr,
                                       outlier ? io[OUT].d : nullptr, 1, (int)rows, view, p, io[INFO].d, io[PTS].d, io[PDESC].d, io[PROWS].d, io[NPTS].d,
                                       io[SUM].d);
    if (rc != SS_OK) {
        (void)hipStreamSynchronize(c->stream);
        return rc;
    }
    rc = io_fetch(c, io, PIECES); /* the count first: it sizes the copies of the compact blocks */
    if (rc != SS_OK) return rc;
    const size_t np = (size_t)std::min(std::max(*n_points, 0), n);
    io_piece blocks[3] = {io[PTS], io[PDESC], io[PROWS]};
    blocks[0].bytes = np * sizeof(ss_map_point), blocks[1].bytes = np * 32, blocks[2].bytes = np * 8;
    return io_fetch(c, blocks, 3);
}

/* ---- PnP RANSAC (csrc/ss_pnp.hip, csrc/ss_pnp_steps.h) ---- */
/* the message of the first rule p breaks, or NULL; needs no context */
static const char *pnp_params_error(const ss_pnp_params *p)
{
    if (!p) return "pnp: params is NULL";
    if (!(p->chi2 > 0.0f) || !std::isfinite(p->chi2)) return "pnp: chi2 must be finite and > 0";
    if (!(p->min_ratio >= 0.0f) || !std::isfinite(p->min_ratio)) return "pnp: min_ratio must be finite and >= 0";
    if (!(p->lambda >= 0.0) || !std::isfinite(p->lambda)) return "pnp: lambda must be finite and >= 0";
    if (p->min_inliers < 0) return "pnp: min_inliers must be >= 0";
    if (p->max_iterations < 1 || p->max_iterations > SS_PNP_MAX_ITERATIONS) return "pnp: max_iterations must be 1 .. SS_PNP_MAX_ITERATIONS";
    if (p->refine_steps < 0 || p->refine_steps > SS_PNP_MAX_REFINE) return "pnp: refine_steps must be 0 .. SS_PNP_MAX_REFINE";
    if (p->reserved[0] != 0 || p->reserved[1] != 0) return "pnp: the reserved fields must be 0";
    return nullptr;
}

int ss_pnp_host(const ss_proj_view *view, const float *scale, int n_levels, const ss_map_point *points, const uint8_t *point_skip, int n_points,
                const ss_keypoint *kp, int n_kp, const int32_t *idx, const ss_pnp_params *p, int problem, uint8_t *inlier, ss_pnp_result *result)
{
    if (pnp_params_error(p)) return SS_ERR_INVALID_ARG;
    if (!view || !scale || n_levels < 1 || n_levels > SS_MAX_LEVELS || n_points < 0 || n_kp < 0 || problem < 0 || !result) return SS_ERR_INVALID_ARG;
    if ((n_points > 0 && !points) || (n_kp > 0 && (!kp || !idx || !inlier))) return SS_ERR_INVALID_ARG;
    /* step 1 */
    std::vector<ss_pnp_corr> corr;
    std::vector<float> sc;
    std::vector<int32_t> point, row_of;
    for (int i = 0; i < n_kp; i++) {
        const int j = idx[i], octave = kp[i].octave;
        inlier[i] = 0;
        if (!(j >= 0 && j < n_points) || !(octave >= 0 && octave < n_levels)) continue;
        if (point_skip && point_skip[j] != 0) continue;
        ss_pnp_corr c;
        c.X[0] = points[j].x, c.X[1] = points[j].y, c.X[2] = points[j].z;
        c.u = kp[i].x, c.v = kp[i].y, c.max = ss_pnp_max(p->chi2, scale[octave]);
        corr.push_back(c), sc.push_back(scale[octave]), point.push_back(j), row_of.push_back(i);
    }
    const int n = (int)corr.size();
    std::vector<uint8_t> in((size_t)n + 1);
    ss_pnp_problem_host(corr.data(), sc.data(), point.data(), n, ss_pnp_cam_of(*view), *p, (uint32_t)problem, in.data(), result);
    for (int k = 0; k < n; k++) inlier[row_of[(size_t)k]] = in[(size_t)k];
    return SS_OK;
}

int ss_pnp_model_host(const ss_pnp_params *p, const ss_proj_view *view, const float *xyz, const float *uv, const float *scale6,
                      const int32_t *point_rows6, ss_pnp_result *out)
{
    if (pnp_params_error(p) || !view || !xyz || !uv || !scale6 || !point_rows6 || !out) return SS_ERR_INVALID_ARG;
    memset(out, 0, sizeof(*out));
    int row[SS_PNP_DRAWS];
    for (int k = 0; k < SS_PNP_DRAWS; k++) row[k] = point_rows6[k];
    ss_pnp_work_host w;
    const ss_pnp_model m = ss_pnp_model_of(xyz, uv, scale6, row, ss_pnp_cam_of(*view), p->lambda, p->refine_steps, w);
    memcpy(out->rcw, m.rcw, sizeof(m.rcw));
    memcpy(out->tcw, m.tcw, sizeof(m.tcw));
    out->iteration = -1;
    return SS_OK;
}

int ss_pnp_check_host(const ss_pnp_params *p, const ss_proj_view *view, const float *scale, int n_levels, const ss_map_point *points,
                      const ss_keypoint *kp, int n, const ss_pnp_result *model, uint8_t *out, float *err)
{
    if (pnp_params_error(p)) return SS_ERR_INVALID_ARG;
    if (!view || !scale || n_levels < 1 || n_levels > SS_MAX_LEVELS || !model || n < 0 || (n > 0 && (!points || !kp || !out))) return SS_ERR_INVALID_ARG;
    float r[9], t[3];
    for (int k = 0; k < 9; k++) r[k] = (float)model->rcw[k];
    for (int k = 0; k < 3; k++) t[k] = (float)model->tcw[k];
    const ss_pnp_cam cam = ss_pnp_cam_of(*view);
    for (int k = 0; k < n; k++) {
        const int octave = kp[k].octave;
        if (err) err[k] = 0.0f;
        if (!(octave >= 0 && octave < n_levels)) {
            out[k] = 1;
            continue;
        }
        ss_pnp_corr c;
        c.X[0] = points[k].x, c.X[1] = points[k].y, c.X[2] = points[k].z;
        c.u = kp[k].x, c.v = kp[k].y, c.max = ss_pnp_max(p->chi2, scale[octave]);
        float e;
        out[k] = (uint8_t)ss_pnp_test(r, t, c, cam, &e);
        if (err) err[k] = e;
    }
    return SS_OK;
}

/* The checks the device forms share, the workspace, the host tables (views, then the frame and block numbers), then the four
 * launches of a call whose device operands and outputs are filled in */
static int pnp_run(ss_ctx *c, ssk_pnp_call &g, int n_blocks, int n_kp_frames, const ss_proj_view *views, const int32_t *kp_src, const int32_t *point_src,
                   const ss_pnp_params *p)
{
    if (const char *msg = pnp_params_error(p)) return fail(c, SS_ERR_INVALID_ARG, msg);
    if (g.n_frames < 0 || n_blocks < 0 || n_kp_frames < 0 || g.point_rows < 1 || g.rows < 1)
        return fail(c, SS_ERR_INVALID_ARG, "pnp: bad problem, frame, block or row count");
    if (g.point_rows > SS_GUIDED_MAX_ROWS || g.rows > SS_GUIDED_MAX_ROWS)
        return fail(c, SS_ERR_INVALID_ARG, "pnp: point_rows " + std::to_string(g.point_rows) + " / rows_per_frame " + std::to_string(g.rows) +
                                               " exceed SS_GUIDED_MAX_ROWS (" + std::to_string(SS_GUIDED_MAX_ROWS) + ")");
    int rc = call_count_ok(c, "pnp", g.n_frames, "problems");
    if (rc == SS_OK) rc = context_pyramid(c, "pnp", &g.n_levels, g.scale);
    if (rc != SS_OK) return rc;
    if (g.n_frames == 0) return SS_OK;
    if (!views) return fail(c, SS_ERR_INVALID_ARG, "pnp: views is NULL");
    for (int q = 0; q < g.n_frames; q++) {
        const int kf = kp_src ? kp_src[q] : q, pb = point_src ? point_src[q] : q;
        if (kf < 0 || kf >= n_kp_frames)
            return fail(c, SS_ERR_INVALID_ARG, std::string(kp_src ? "kp_src[" : "problem [") + std::to_string(q) + "] = " + std::to_string(kf) +
                                                   " names no frame of keypoints (" + std::to_string(n_kp_frames) + ")");
        if (pb < 0 || pb >= n_blocks)
            return fail(c, SS_ERR_INVALID_ARG, std::string(point_src ? "point_src[" : "problem [") + std::to_string(q) + "] = " + std::to_string(pb) +
                                                   " names no block of points (" + std::to_string(n_blocks) + ")");
    }
    if (!g.points || !g.np || !g.kp || !g.nk || !g.idx || !g.inlier || !g.result) return fail(c, SS_ERR_INVALID_ARG, "pnp: NULL buffer");
    g.chi2 = p->chi2, g.min_ratio = p->min_ratio, g.lambda = p->lambda;
    g.min_inliers = p->min_inliers, g.max_iterations = p->max_iterations, g.refine_steps = p->refine_steps, g.seed = p->seed;
    const size_t np = (size_t)g.n_frames, nr = np * g.rows, nh = np * g.max_iterations;
    rc = carve_from(c, c->d_pnp_ws, [&](carve &w) {
        g.corr = w.take<float>(6 * nr * sizeof(float));
        g.corr_scale = w.take<float>(nr * sizeof(float));
        g.corr_point = w.take<int32_t>(nr * sizeof(int32_t));
        g.corr_of_row = w.take<int32_t>(nr * sizeof(int32_t));
        g.n_corr = w.take<int32_t>(np * sizeof(int32_t));
        g.models = w.take<ssk_pnp_model>(nh * sizeof(ssk_pnp_model));
        g.poses = w.take<double>(nh * 12 * sizeof(double));
        g.counts = w.take<int32_t>(nh * sizeof(int32_t));
    });
    if (rc != SS_OK) return rc;
    const size_t vb = np * sizeof(ss_proj_view), sb = np * sizeof(int32_t);
    rc = staged_upload(c, c->pnp_tab, vb + 2 * sb, [&](uint8_t *h) {
        memcpy(h, views, vb);
        int32_t *ks = (int32_t *)(h + vb), *ps = (int32_t *)(h + vb + sb);
        for (int q = 0; q < g.n_frames; q++) ks[q] = kp_src ? kp_src[q] : q, ps[q] = point_src ? point_src[q] : q;
    });
    if (rc != SS_OK) return rc;
    g.views = c->pnp_tab.as<ss_proj_view>();
    g.kp_src = c->pnp_tab.as<int32_t>(vb), g.point_src = c->pnp_tab.as<int32_t>(vb + sb);
    {
        /* per row: its match and the number written; a correspondence reads a map point, a keypoint and up to a flag and writes its
         * six floats, its scale and its point row */
        stage_timer t(c, "pnp_gather", (int64_t)nr * (4 + 4 + (int64_t)sizeof(ss_map_point) + (int64_t)sizeof(ss_keypoint) + (g.p_skip ? 1 : 0) + 32) + (int64_t)np * 4);
        ssk_pnp_gather(c->stream, g);
    }
    {
        /* per hypothesis: six correspondences' five floats, scale and row read, one record, twelve doubles and one count written */
        stage_timer t(c, "pnp_model", (int64_t)nh * (SS_PNP_DRAWS * 28 + (int64_t)sizeof(ssk_pnp_model) + 96 + 4));
        ssk_pnp_model_launch(c->stream, g);
    }
    {
        /* every block of hypotheses reads the six floats of every correspondence once and its own records; the counts are added */
        const int64_t hb = (g.max_iterations + SSK_PNP_HYP_BLOCK - 1) / SSK_PNP_HYP_BLOCK;
        stage_timer t(c, "pnp_count", (int64_t)nr * 24 * hb + (int64_t)nh * ((int64_t)sizeof(ssk_pnp_model) + 4));
        ssk_pnp_count(c->stream, g);
    }
    {
        /* the counts read; per row its number read and its flag written, an inlier candidate's six floats on top */
        stage_timer t(c, "pnp_finish", (int64_t)nh * 4 + (int64_t)nr * (4 + 1 + 24) + (int64_t)np * (int64_t)(sizeof(ssk_pnp_model) + 96 + sizeof(ss_pnp_result)));
        ssk_pnp_finish(c->stream, g);
    }
    HIP_TRY(c, hipGetLastError());
    return SS_OK;
}

int ss_pnp_pairs_device(ss_ctx *c, const void *d_points, const void *d_point_skip, const void *d_n_points, int n_blocks, int point_rows, const void *d_kp,
                        const void *d_n_kp, int n_kp_frames, int rows_per_frame, const void *d_idx, int n_problems, const ss_proj_view *views,
                        const int32_t *kp_src, const int32_t *point_src, const ss_pnp_params *p, void *d_inlier, void *d_result)
{
    if (!c) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    ssk_pnp_call g;
    g.n_frames = n_problems, g.point_rows = point_rows, g.rows = rows_per_frame;
    g.points = (const ss_map_point *)d_points, g.p_skip = (const uint8_t *)d_point_skip, g.np = (const int32_t *)d_n_points;
    g.kp = (const ss_keypoint *)d_kp, g.nk = (const int32_t *)d_n_kp;
    g.idx = (const int32_t *)d_idx;
    g.inlier = (uint8_t *)d_inlier, g.result = (ss_pnp_result *)d_result;
    return pnp_run(c, g, n_blocks, n_kp_frames, views, kp_src, point_src, p);
}

int ss_pnp_batch_device(ss_ctx *c, const void *d_points, const void *d_point_skip, const void *d_n_points, int n_blocks, int point_rows,
                        const void *d_idx, int n_problems, const ss_proj_view *views, const int32_t *kp_src, const int32_t *point_src,
                        const ss_pnp_params *p, void *d_inlier, void *d_result)
{
    if (!c) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    if (!have_batch(c, "ss_pnp_batch_device")) return SS_ERR_STATE;
    ssk_pnp_call g;
    g.n_frames = n_problems, g.point_rows = point_rows, g.rows = c->hg.kcap;
    g.points = (const ss_map_point *)d_points, g.p_skip = (const uint8_t *)d_point_skip, g.np = (const int32_t *)d_n_points;
    g.kp = c->ws.kps, g.nk = c->ws.n_kp;
    const int rc = flagged_frame_error(c, c->batch_test_flagged, &g.frame_error);
    if (rc != SS_OK) return rc;
    g.idx = (const int32_t *)d_idx;
    g.inlier = (uint8_t *)d_inlier, g.result = (ss_pnp_result *)d_result;
    return pnp_run(c, g, n_blocks, c->last_n_frames, views, kp_src, point_src, p);
}

int ss_pnp(ss_ctx *c, const ss_proj_view *view, const ss_map_point *points, const uint8_t *point_skip, int n_points, const ss_keypoint *kp, int n_kp,
           const int32_t *idx, const ss_pnp_params *p, uint8_t *inlier, ss_pnp_result *result)
{
    if (!c) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    if (const char *msg = pnp_params_error(p)) return fail(c, SS_ERR_INVALID_ARG, msg);
    if (n_points < 0 || n_kp < 0 || n_points > SS_GUIDED_MAX_ROWS || n_kp > SS_GUIDED_MAX_ROWS)
        return fail(c, SS_ERR_INVALID_ARG, "pnp: n_points and n_kp must be 0 .. SS_GUIDED_MAX_ROWS");
    if (!view || !result || (n_points > 0 && !points) || (n_kp > 0 && (!kp || !idx || !inlier))) return fail(c, SS_ERR_INVALID_ARG, "pnp: NULL buffer");
    /* one block of `pr` points, one frame of `kr` rows; `counts` is on this stack: no return before the stream has read it */
    const size_t pr = (size_t)std::max(n_points, 1), kr = (size_t)std::max(n_kp, 1), np = (size_t)n_points, nk = (size_t)n_kp;
    const int32_t counts[2] = {n_points, n_kp};
    enum { PT, PS, KP, IDX, N, FL, RES, PIECES };
    io_piece io[PIECES] = {{points, nullptr, pr * sizeof(ss_map_point), np * sizeof(ss_map_point)}, {point_skip, nullptr, pr, np},
                           {kp, nullptr, kr * sizeof(ss_keypoint), nk * sizeof(ss_keypoint)}, {idx, nullptr, kr * 4, nk * 4},
                           {counts, nullptr, sizeof(counts), sizeof(counts)}, {nullptr, inlier, kr, nk},
                           {nullptr, result, sizeof(ss_pnp_result), sizeof(ss_pnp_result)}};
    int rc = io_send(c, c->d_pnp_io, io, PIECES);
    if (rc == SS_OK)
        rc = ss_pnp_pairs_device(c, io[PT].d, point_skip ? io[PS].d : nullptr, io[N].d, 1, (int)pr, io[KP].d, io[N].d + 4, 1, (int)kr, io[IDX].d, 1, view,
                                 nullptr, nullptr, p, io[FL].d, io[RES].d);
    if (rc != SS_OK) {
        (void)hipStreamSynchronize(c->stream);
        return rc;
    }
    return io_fetch(c, io, PIECES);
}

/* ---- two-view initialisation (csrc/ss_two_view.hip, csrc/ss_two_view_steps.h) ---- */
/* the message of the first rule p breaks, or NULL; needs no context */
static const char *tv_params_error(const ss_two_view_params *p)
{
    if (!p) return "two_view: params is NULL";
    if (!(p->chi2_h > 0.0) || !std::isfinite(p->chi2_h)) return "two_view: chi2_h must be finite and > 0";
    if (!(p->chi2_f > 0.0) || !std::isfinite(p->chi2_f)) return "two_view: chi2_f must be finite and > 0";
    if (!(p->chi2_score > 0.0) || !std::isfinite(p->chi2_score)) return "two_view: chi2_score must be finite and > 0";
    if (!(p->rh_threshold >= 0.0 && p->rh_threshold <= 1.0)) return "two_view: rh_threshold must be 0 .. 1";
    if (!(p->cos_min_parallax >= -1.0 && p->cos_min_parallax <= 1.0)) return "two_view: cos_min_parallax must be -1 .. 1";
    if (p->min_triangulated < 0) return "two_view: min_triangulated must be >= 0";
    if (p->max_iterations < 1 || p->max_iterations > SS_TWO_VIEW_MAX_ITERATIONS) return "two_view: max_iterations must be 1 .. SS_TWO_VIEW_MAX_ITERATIONS";
    if (p->reserved[0] != 0 || p->reserved[1] != 0 || p->reserved[2] != 0) return "two_view: the reserved fields must be 0";
    return nullptr;
}

int ss_two_view_host(const ss_proj_view *view, const float *scale, int n_levels, const ss_keypoint *kp1, int n_kp1, const ss_keypoint *kp2, int n_kp2,
                     const int32_t *idx, const ss_two_view_params *p, int problem, uint8_t *flag, ss_map_point *points, int32_t *point_rows,
                     int32_t *n_points, ss_two_view_result *result)
{
    if (tv_params_error(p)) return SS_ERR_INVALID_ARG;
    if (!view || !scale || n_levels < 1 || n_levels > SS_MAX_LEVELS || n_kp1 < 0 || n_kp2 < 0 || problem < 0 || !result || !n_points) return SS_ERR_INVALID_ARG;
    if ((n_kp1 > 0 && (!kp1 || !idx || !flag || !points || !point_rows)) || (n_kp2 > 0 && !kp2)) return SS_ERR_INVALID_ARG;
    /* step 1 */
    std::vector<float> corr, s1;
    std::vector<int32_t> row_of;
    for (int i = 0; i < n_kp1; i++) {
        const int j = idx[i], octave = kp1[i].octave;
        flag[i] = 0;
        if (!(j >= 0 && j < n_kp2) || !(octave >= 0 && octave < n_levels)) continue;
        corr.push_back(kp1[i].x), corr.push_back(kp1[i].y), corr.push_back(kp2[j].x), corr.push_back(kp2[j].y);
        s1.push_back(scale[octave]), row_of.push_back(i);
    }
    const int n = (int)row_of.size();
    std::vector<uint8_t> fl((size_t)n + 1);
    std::vector<ss_map_point> pts((size_t)n + 1);
    ss_tv_problem_host(corr.data(), s1.data(), n, ss_tv_cam_of(*view), scale[n_levels - 1], *p, (uint32_t)problem, fl.data(), pts.data(), result);
    int np = 0;
    for (int k = 0; k < n; k++) {
        const int i = row_of[(size_t)k];
        flag[i] = fl[(size_t)k];
        if (fl[(size_t)k] == 3) points[np] = pts[(size_t)k], point_rows[2 * np] = i, point_rows[2 * np + 1] = idx[i], np++;
    }
    *n_points = np;
    return SS_OK;
}

int ss_two_view_model_host(const float *uv, double *h21, double *h12, double *f21, int32_t *ok)
{
    if (!uv || !h21 || !h12 || !f21 || !ok) return SS_ERR_INVALID_ARG;
    const ss_tv_norm nm = ss_tv_normalise_host(uv, SS_TV_DRAWS);
    ss_tv_model m;
    memset(&m, 0, sizeof(m));
    if (ss_tv_norm_ok(nm)) {
        const int pick[SS_TV_DRAWS] = {0, 1, 2, 3, 4, 5, 6, 7};
        ss_tv_work_host w;
        ss_tv_model_of(uv, pick, nm, w, m);
    }
    memcpy(h21, m.h21, sizeof(m.h21)), memcpy(h12, m.h12, sizeof(m.h12)), memcpy(f21, m.f21, sizeof(m.f21));
    ok[0] = m.ok_h, ok[1] = m.ok_f;
    return SS_OK;
}

int ss_two_view_check_host(const ss_two_view_params *p, const ss_proj_view *view, const float *uv, int n, const double *h21, const double *h12,
                           const double *f21, const double *r21, const double *t21, double *chi_h, uint8_t *in_h, double *score_h, double *chi_f,
                           uint8_t *in_f, double *score_f, uint8_t *good, double *cosv, double *xyz)
{
    if (tv_params_error(p)) return SS_ERR_INVALID_ARG;
    if (!view || n < 0 || (n > 0 && !uv)) return SS_ERR_INVALID_ARG;
    const bool do_h = h21 && h12, do_f = f21 != nullptr, do_rt = r21 && t21;
    if ((do_h && (!chi_h || !in_h || !score_h)) || (do_f && (!chi_f || !in_f || !score_f)) || (do_rt && (!good || !cosv || !xyz))) return SS_ERR_INVALID_ARG;
    auto at = [&](int k, int c) { return (double)uv[4 * k + c]; };
    if (do_h)
        *score_h = ss_tv_tree_sum(n, [&](int k) {
            bool in;
            const double v = ss_tv_term_h(h21, h12, at(k, 0), at(k, 1), at(k, 2), at(k, 3), p->chi2_h, &in, chi_h + 2 * k);
            in_h[k] = in ? 1 : 0;
            return v;
        });
    if (do_f)
        *score_f = ss_tv_tree_sum(n, [&](int k) {
            bool in;
            const double v = ss_tv_term_f(f21, at(k, 0), at(k, 1), at(k, 2), at(k, 3), p->chi2_f, p->chi2_score, &in, chi_f + 2 * k);
            in_f[k] = in ? 1 : 0;
            return v;
        });
    const ss_tv_cam cam = ss_tv_cam_of(*view);
    for (int k = 0; do_rt && k < n; k++) {
        ss_tv_point q;
        const bool g = ss_tv_check_rt(r21, t21, cam, at(k, 0), at(k, 1), at(k, 2), at(k, 3), &q);
        good[k] = g ? (ss_tv_triangulated(q.cosp) ? 2 : 1) : 0;
        cosv[k] = q.cosp, xyz[3 * k] = q.X[0], xyz[3 * k + 1] = q.X[1], xyz[3 * k + 2] = q.X[2];
    }
    return SS_OK;
}

int ss_two_view_accept_host(const ss_two_view_params *p, int model, const int32_t *good, int n_hyp, int n_in, double cos_parallax, int32_t *out)
{
    if (tv_params_error(p) || !good || !out || (model != 1 && model != 2) || n_hyp < 1 || n_hyp > SS_TV_MAX_HYP || n_in < 0) return SS_ERR_INVALID_ARG;
    int g[SS_TV_MAX_HYP] = {0}, best, best_good, second_good;
    for (int k = 0; k < n_hyp; k++) g[k] = good[k];
    ss_tv_pick(g, n_hyp, &best, &best_good, &second_good);
    out[0] = ss_tv_accept(model, g, n_hyp, best_good, second_good, n_in, cos_parallax, *p);
    out[1] = best, out[2] = best_good, out[3] = second_good;
    return SS_OK;
}

int ss_two_view_point_tests_host(double cos_parallax, double err_sq, int32_t *out)
{
    if (!out) return SS_ERR_INVALID_ARG;
    out[0] = ss_tv_triangulated(cos_parallax) ? 1 : 0, out[1] = ss_tv_exempt(cos_parallax) ? 1 : 0, out[2] = ss_tv_reprojects(err_sq) ? 1 : 0;
    return SS_OK;
}

int ss_two_view_beats_host(double score, int t, double best, int best_t) { return ss_tv_beats(score, t, best, best_t) ? 1 : 0; }

/* The checks the device forms share, the workspace, the host tables (views, then both sides' frame numbers; src2 entries may be -1
 * when `none_ok`: no frame 2), then the six launches of a call whose device operands and outputs are filled in */
static int tv_run(ss_ctx *c, ssk_tv_call &g, int n_frames1, int n_frames2, const ss_proj_view *views, const int32_t *src1, const int32_t *src2,
                  int default2_shift, bool none_ok, const ss_two_view_params *p)
{
    if (const char *msg = tv_params_error(p)) return fail(c, SS_ERR_INVALID_ARG, msg);
    if (n_frames1 < 0 || n_frames2 < 0) return fail(c, SS_ERR_INVALID_ARG, "two_view: bad frame count");
    int rc = pairs_shape(c, "two_view", "problem", g.n_frames, g.rows);
    if (rc == SS_OK) rc = call_count_ok(c, "two_view", g.n_frames, "problems");
    if (rc == SS_OK) rc = context_pyramid(c, "two_view", &g.n_levels, g.scale);
    if (rc != SS_OK) return rc;
    if (g.n_frames == 0) return SS_OK;
    if (!views) return fail(c, SS_ERR_INVALID_ARG, "two_view: views is NULL");
    for (int q = 0; q < g.n_frames; q++) {
        const int f1 = src1 ? src1[q] : q, f2 = src2 ? src2[q] : q - default2_shift;
        if (f1 < 0 || f1 >= n_frames1)
            return fail(c, SS_ERR_INVALID_ARG, std::string(src1 ? "kp1_src[" : "problem [") + std::to_string(q) + "] = " + std::to_string(f1) +
                                                   " names no frame of side 1 (" + std::to_string(n_frames1) + ")");
        if ((f2 < (none_ok ? -1 : 0)) || f2 >= n_frames2)
            return fail(c, SS_ERR_INVALID_ARG, std::string(src2 ? "kp2_src[" : "problem [") + std::to_string(q) + "] = " + std::to_string(f2) +
                                                   " names no frame of side 2 (" + std::to_string(n_frames2) + ")");
    }
    if (!g.kp1 || !g.n1 || !g.kp2 || !g.n2 || !g.idx || !g.flag || !g.points || !g.point_rows || !g.n_points || !g.result)
        return fail(c, SS_ERR_INVALID_ARG, "two_view: NULL buffer");
    g.p = *p;
    const size_t np = (size_t)g.n_frames, nr = np * g.rows, nh = np * g.p.max_iterations;
    const size_t chunks = ((size_t)g.rows + SS_TV_CHUNK - 1) / SS_TV_CHUNK;
    rc = carve_from(c, c->d_tv_ws, [&](carve &w) {
        g.models = w.take<ssk_tv_model>(nh * sizeof(ssk_tv_model));
        g.partial = w.take<double>(nh * chunks * 2 * sizeof(double));
        g.choice = w.take<ssk_tv_choice>(np * sizeof(ssk_tv_choice));
        g.corr = w.take<float>(4 * nr * sizeof(float));
        g.corr_of_row = w.take<int32_t>(nr * sizeof(int32_t));
        g.n_corr = w.take<int32_t>(np * sizeof(int32_t));
        g.corr_flag = w.take<uint8_t>(nr);
    });
    if (rc != SS_OK) return rc;
    const size_t vb = np * sizeof(ss_proj_view), sb = np * sizeof(int32_t);
    rc = staged_upload(c, c->tv_tab, vb + 2 * sb, [&](uint8_t *h) {
        memcpy(h, views, vb);
        int32_t *s1 = (int32_t *)(h + vb), *s2 = (int32_t *)(h + vb + sb);
        for (int q = 0; q < g.n_frames; q++) s1[q] = src1 ? src1[q] : q, s2[q] = src2 ? src2[q] : q - default2_shift;
    });
    if (rc != SS_OK) return rc;
    g.views = c->tv_tab.as<ss_proj_view>();
    g.kp1_src = c->tv_tab.as<int32_t>(vb), g.kp2_src = c->tv_tab.as<int32_t>(vb + sb);
    const int64_t T = g.p.max_iterations, hb = (T + SSK_TV_HYP_BLOCK - 1) / SSK_TV_HYP_BLOCK;
    {
        /* per row: its match and the number written; a correspondence reads two keypoints and writes its four floats, which the two
         * sums of the normalisation then read twice */
        stage_timer t(c, "tv_gather", (int64_t)nr * (4 + 4 + 2 * (int64_t)sizeof(ss_keypoint) + 16 + 32) + (int64_t)np * (int64_t)sizeof(ssk_tv_choice));
        ssk_tv_gather(c->stream, g);
    }
    {
        /* per hypothesis: eight correspondences' four floats read, one record written */
        stage_timer t(c, "tv_model", (int64_t)nh * (SS_TV_DRAWS * 16 + (int64_t)sizeof(ssk_tv_model)));
        ssk_tv_model_launch(c->stream, g);
    }
    {
        /* every block of hypotheses reads the four floats of every correspondence once and its own records per chunk; two partial
         * sums per chunk and hypothesis are written */
        stage_timer t(c, "tv_score", (int64_t)nr * 16 * hb + (int64_t)nh * (int64_t)chunks * ((int64_t)sizeof(ssk_tv_model) + 16));
        ssk_tv_score(c->stream, g);
    }
    {
        /* the partial sums and the records' flags read; per correspondence its four floats read and its flag written */
        stage_timer t(c, "tv_select", (int64_t)nh * ((int64_t)chunks * 16 + 8) + (int64_t)nr * (16 + 1) + (int64_t)np * (int64_t)(sizeof(ssk_tv_model) + sizeof(ssk_tv_choice)));
        ssk_tv_select(c->stream, g);
    }
    {
        /* per correspondence its flag and four floats; the hypotheses and counts per workgroup */
        stage_timer t(c, "tv_check", (int64_t)nr * (16 + 1) + (int64_t)np * (int64_t)chunks * (int64_t)sizeof(ssk_tv_choice));
        ssk_tv_check(c->stream, g);
    }
    {
        /* twice per correspondence its flag and four floats; per row its number, match and octave read, its flag written, and up to
         * one point and its two rows */
        stage_timer t(c, "tv_finish", (int64_t)nr * (2 * (16 + 1) + 4 + 4 + (int64_t)sizeof(ss_keypoint) + 1 + (int64_t)sizeof(ss_map_point) + 8) +
                                          (int64_t)np * (int64_t)(sizeof(ssk_tv_choice) + sizeof(ss_two_view_result) + 4));
        ssk_tv_finish(c->stream, g);
    }
    HIP_TRY(c, hipGetLastError());
    return SS_OK;
}

int ss_two_view_pairs_device(ss_ctx *c, const void *d_kp1, const void *d_n_kp1, int n_frames1, const void *d_kp2, const void *d_n_kp2, int n_frames2,
                             int rows_per_frame, const void *d_idx, int n_problems, const ss_proj_view *views, const int32_t *kp1_src,
                             const int32_t *kp2_src, const ss_two_view_params *p, void *d_flag, void *d_points, void *d_point_rows, void *d_n_points,
                             void *d_result)
{
    if (!c) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    ssk_tv_call g;
    g.n_frames = n_problems, g.rows = rows_per_frame;
    g.kp1 = (const ss_keypoint *)d_kp1, g.n1 = (const int32_t *)d_n_kp1, g.kp2 = (const ss_keypoint *)d_kp2, g.n2 = (const int32_t *)d_n_kp2;
    g.idx = (const int32_t *)d_idx;
    g.flag = (uint8_t *)d_flag, g.points = (ss_map_point *)d_points, g.point_rows = (int32_t *)d_point_rows, g.n_points = (int32_t *)d_n_points;
    g.result = (ss_two_view_result *)d_result;
    return tv_run(c, g, n_frames1, n_frames2, views, kp1_src, kp2_src, 0, false, p);
}

int ss_two_view_batch_device(ss_ctx *c, const int32_t *train_src, const void *d_idx, int n_problems, const ss_proj_view *views,
                             const ss_two_view_params *p, void *d_flag, void *d_points, void *d_point_rows, void *d_n_points, void *d_result)
{
    if (!c) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    if (!have_batch(c, "ss_two_view_batch_device")) return SS_ERR_STATE;
    if (n_problems != c->last_n_frames) return fail(c, SS_ERR_INVALID_ARG, "two_view: n_problems must be the batch's frame count");
    ssk_tv_call g;
    g.n_frames = n_problems, g.rows = c->hg.kcap;
    g.kp1 = g.kp2 = c->ws.kps, g.n1 = g.n2 = c->ws.n_kp;
    const int rc = flagged_frame_error(c, c->batch_test_flagged, &g.frame_error);
    if (rc != SS_OK) return rc;
    g.idx = (const int32_t *)d_idx;
    g.flag = (uint8_t *)d_flag, g.points = (ss_map_point *)d_points, g.point_rows = (int32_t *)d_point_rows, g.n_points = (int32_t *)d_n_points;
    g.result = (ss_two_view_result *)d_result;
    return tv_run(c, g, c->last_n_frames, c->last_n_frames, views, nullptr, train_src, 1, true, p);
}

int ss_two_view(ss_ctx *c, const ss_proj_view *view, const ss_keypoint *kp1, int n_kp1, const ss_keypoint *kp2, int n_kp2, const int32_t *idx,
                const ss_two_view_params *p, uint8_t *flag, ss_map_point *points, int32_t *point_rows, int32_t *n_points, ss_two_view_result *result)
{
    if (!c) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    if (const char *msg = tv_params_error(p)) return fail(c, SS_ERR_INVALID_ARG, msg);
    if (n_kp1 < 0 || n_kp2 < 0 || n_kp1 > SS_GUIDED_MAX_ROWS || n_kp2 > SS_GUIDED_MAX_ROWS)
        return fail(c, SS_ERR_INVALID_ARG, "two_view: n_kp1 and n_kp2 must be 0 .. SS_GUIDED_MAX_ROWS");
    if (!view || !result || !n_points || (n_kp1 > 0 && (!kp1 || !idx || !flag || !points || !point_rows)) || (n_kp2 > 0 && !kp2))
        return fail(c, SS_ERR_INVALID_ARG, "two_view: NULL buffer");
    /* one frame of `rows` rows on each side; `counts` is on this stack: no return before the stream has read it.  The points and
     * their rows come back whole: rows from n_points on hold what the device buffer held */
    const size_t rows = (size_t)std::max(std::max(n_kp1, n_kp2), 1), n1 = (size_t)n_kp1, n2 = (size_t)n_kp2, kb = sizeof(ss_keypoint);
    const int32_t counts[2] = {n_kp1, n_kp2};
    std::vector<ss_map_point> pts(rows);
    std::vector<int32_t> prow(2 * rows);
    enum { K1, K2, IDX, N, FL, PT, PR, NP, RES, PIECES };
    io_piece io[PIECES] = {{kp1, nullptr, rows * kb, n1 * kb}, {kp2, nullptr, rows * kb, n2 * kb}, {idx, nullptr, rows * 4, n1 * 4},
                           {counts, nullptr, sizeof(counts), sizeof(counts)}, {nullptr, flag, rows, n1},
                           {nullptr, pts.data(), rows * sizeof(ss_map_point), rows * sizeof(ss_map_point)}, {nullptr, prow.data(), rows * 8, rows * 8},
                           {nullptr, n_points, 4, 4}, {nullptr, result, sizeof(ss_two_view_result), sizeof(ss_two_view_result)}};
    int rc = io_send(c, c->d_tv_io, io, PIECES);
    if (rc == SS_OK)
        rc = ss_two_view_pairs_device(c, io[K1].d, io[N].d, 1, io[K2].d, io[N].d + 4, 1, (int)rows, io[IDX].d, 1, view, nullptr, nullptr, p, io[FL].d,
                                      io[PT].d, io[PR].d, io[NP].d, io[RES].d);
    if (rc != SS_OK) {
        (void)hipStreamSynchronize(c->stream);
        return rc;
    }
    rc = io_fetch(c, io, PIECES);
    if (rc != SS_OK) return rc;
    const int np = std::min(std::max(*n_points, 0), n_kp1);
    for (int k = 0; k < np; k++) points[k] = pts[(size_t)k], point_rows[2 * k] = prow[2 * (size_t)k], point_rows[2 * k + 1] = prow[2 * (size_t)k + 1];
    return SS_OK;
}

} /* extern "C" */
