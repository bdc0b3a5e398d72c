/*
 * ss_ctx.h -- private to the sources of the C ABI (ss_api.cpp, ss_api_search.cpp): the context, its buffers and the helpers every
 * entry point is written with.  No kernel source includes it.  The helpers live in ss_detail, which stays out of the dynamic
 * symbol table.
 */
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "../../include/sendslam_orb.h"
#include "ss_constants.h"
#include "ss_covis_steps.h"
#include "ss_geometry.h"
#include "ss_kernels.h"
#include "ss_layout.h"
#include "ss_track.h"

namespace ss_detail __attribute__((visibility("hidden"))) {

struct stage_rec {
    std::string name;
    int64_t bytes = 0;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
    std::vector<float> ms;
};

template <typename T> void dev_free(T *&p)
{
    if (p) (void)hipFree((void *)p);
    p = nullptr;
}

/* a device buffer that grow() enlarges on demand: reads as its pointer */
template <typename T> struct dev_buf {
    T *p = nullptr;
    size_t bytes = 0;
    operator T *() const { return p; }
};
template <typename T> void dev_free(dev_buf<T> &b)
{
    dev_free(b.p);
    b.bytes = 0;
}

/* A host table of a call on its way to the device (staged_upload): written into pinned memory, copied from there on the context's
 * stream; the event marks the end of the last copy.  Both sides are counted in bytes. */
struct staged_table {
    dev_buf<uint8_t> d;
    uint8_t *h = nullptr;
    size_t h_bytes = 0;
    hipEvent_t copied = nullptr;
    template <typename T> const T *as(size_t byte_offset = 0) const { return (const T *)(d.p + byte_offset); }
};

} // namespace ss_detail
using namespace ss_detail;

/* ss_track state of one camera: the tracker, the descriptors of its initialisation reference / previous frame, its own
 * calibration (if it has been sent one) */
struct cam_track {
    int camera_id = 0; /* 0: a free slot */
    bool has_cam = false;
    ss_camera cam{};
    sst_tracker tracker;
    dev_buf<uint8_t> d_ref_desc, d_prev_desc;
    dev_buf<uint8_t> d_ref_desc_x, d_prev_desc_x; /* the same rows as matrix-core operands (128 B each) */
    /* this camera's pose-step calls are numbered: which call's frame the tracker holds as its previous / reference frame, and
     * whether the previous frame's descriptors are still the caller's rows (ss_track_features_matched, prev_ext_n of them) */
    int64_t serial = 0, prev_serial = -1, ref_serial = -1;
    const uint8_t *d_prev_ext = nullptr;
    int prev_ext_n = 0;

    void reset()
    {
        tracker.reset();
        prev_serial = ref_serial = -1;
        d_prev_ext = nullptr;
        prev_ext_n = 0;
    }
    void free_rows()
    {
        dev_free(d_ref_desc);
        dev_free(d_prev_desc);
        dev_free(d_ref_desc_x);
        dev_free(d_prev_desc_x);
    }
};

struct ss_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    ss_orb_params params{};
    std::string err;
    bool calibrated = false;
    bool force_ingest = false; /* SENDSLAM_FORCE_INGEST=1: always copy level 0 into the pyramid block (tests) */
    bool resize_pair[SS_MAX_LEVELS] = {}; /* levels l, l + 1 built by one k_resize_pair launch (checked on the tap tables) */
    bool resize_walk[SS_MAX_LEVELS] = {}; /* level l may be built by k_resize_walk (checked on the tap tables) */
    int64_t wave_slots = 0;    /* resident waves of this context's device at k_resize_walk's occupancy (ss_create): ssk_resize */
    int resize_kernel[SS_MAX_LEVELS] = {}; /* SSK_RESIZE_*: what built level l of the last batch (ss_debug_fetch 5) */
    bool no_desc_x = false;    /* SENDSLAM_MATCH_PACKED=1: batch matches run k_match_mfma on the packed descriptors (A/B tests) */
    ss_camera cam{};
    int cam_id = 0;

    bool have_geom = false;
    ss_geom hg{};
    ss_host_tables tabs;
    ssk_extract_ws ws; /* the device buffers of the extraction: ws_table below lists them with their sizes */

    dev_buf<uint8_t> d_in;
    dev_buf<void> match_partial;
    dev_buf<uint8_t> d_mq, d_mt, d_mout, d_part_tmp;
    dev_buf<uint8_t> d_qx, d_tx; /* caller descriptors expanded to the matrix-core matcher's operand rows */
    staged_table train_src; /* the train table of a batch form (upload_train_src) */
    dev_buf<uint8_t> d_carry_x; /* its carry frames expanded to operand rows */

    /* host results of ss_extract */
    std::vector<ss_keypoint> h_kps;
    std::vector<uint8_t> h_desc;
    std::vector<int32_t> h_err;
    /* ss_extract_stereo: the right eye's host arrays (the left eye uses the set above), the points, their device buffers */
    std::vector<ss_keypoint> h_kps_r;
    std::vector<uint8_t> h_desc_r;
    std::vector<ss_stereo_point> h_stereo;
    dev_buf<uint8_t> d_stereo;
    /* test hooks, SENDSLAM_TEST_STEREO_FLAG=frame,... and SENDSLAM_TEST_FLAG_BATCH=frame,...: the stereo stages / the batch forms
     * of guided matching, bag of words and projection search see those frames of a batch as flagged (frame_error SS_ERR_OVERFLOW,
     * through a copy of the array: flagged_frame_error), the only way to reach the voided-frame rules without overflowing a
     * capacity; n_kp stays as extracted */
    std::vector<int> stereo_test_flagged, batch_test_flagged;
    dev_buf<int32_t> d_test_err;
    /* guided matching: the grid index and candidate counts of a call (grid_index carves them; the projection search uses the same
     * buffer); the host form's device copies */
    dev_buf<uint8_t> d_guided_ws, d_guided_io;
    /* projection search and map-point fusion: the host form's device copies; the views, then the block numbers of a call */
    dev_buf<uint8_t> d_proj_io;
    staged_table proj_tab;
    /* bag of words: the vocabulary on the device (one allocation: rows, records, weights), the node index of a pairs call, and
     * what ss_bow_transform_batch_device keeps of bow_frames frames of the last batch for ss_match_bow_batch_device (nodes, node
     * index, index counts) */
    dev_buf<uint8_t> d_voc, d_bow_ws, d_bow_keep;
    ssk_bow_voc voc;
    int bow_frames = 0;
    /* epipolar search and triangulation: the workspace of each (counters, the finish's summaries, the node index of a pairs call;
     * the uncompacted map points) and the pairs of a call, one table for both */
    dev_buf<uint8_t> d_epi_ws, d_tri_ws;
    staged_table epi_tab;
    /* Sim3 RANSAC: the workspace of a call (correspondences, models, counts), the host form's device copies, the views of a call
     * (views1, then views2) */
    dev_buf<uint8_t> d_sim3_ws, d_sim3_io;
    staged_table sim3_tab;
    /* pose-only optimisation: the workspace of a call (the observations' planes and slots, their counts), the host form's device
     * copies, the tables of a call (views, then block numbers, then start poses) */
    dev_buf<uint8_t> d_pose_ws, d_pose_io;
    staged_table pose_tab;
    /* Sim3 refinement: the workspace of a call (the correspondences' planes and rows, their counts; the taken bytes of the mutual
     * check), the host form's device copies, the views of a call (views1, then views2) */
    dev_buf<uint8_t> d_sim3opt_ws, d_sim3opt_io;
    staged_table sim3opt_tab;
    /* local bundle adjustment: the workspace of a call, the host form's device copies, the tables of a call (problems, the frames'
     * problems, views, start poses; the block numbers of ss_local_ba_points_to_block) */
    dev_buf<uint8_t> d_ba_ws, d_ba_io;
    staged_table ba_tab, ba_block_tab;
    /* essential-graph optimisation: the workspace of a call, the host form's device copies, the tables of a call (problems, edges,
     * the keyframes' problems, the incidence lists) */
    dev_buf<uint8_t> d_graph_ws, d_graph_io;
    staged_table graph_tab;
    /* global bundle adjustment: the workspace of a call, the host form's device copies, the tables of a call (problems, views, the
     * keyframes' and blocks' problems, the sorted records and both incidence lists) */
    dev_buf<uint8_t> d_gba_ws, d_gba_io;
    staged_table gba_tab;
    /* covisibility: the map's tables, kept from ss_covis_set_map until the next one (covis_map points into covis_tab; n_kf == 0: no
     * map), the tables of a query (row or block numbers), the host form's device copies */
    staged_table covis_tab, covis_call_tab;
    ss_covis_tab covis_map;
    int64_t covis_items = 0; /* the records of the map's problems */
    /* the map-point refresh: next to the map's lists, each record's keypoint row in the order of pt_item (NULL: the map was set
     * without rows) with the largest of them, and the points whose list is longer than one wave's (their numbers, their longest
     * list); the tables of a call (every keyframe's ow, then the pyramid's scale table); the host form's device copies */
    const int32_t *covis_pt_row = nullptr, *covis_long = nullptr;
    int covis_max_row = -1, covis_n_long = 0, covis_max_cnt = 0;
    staged_table refresh_tab;
    dev_buf<uint8_t> d_refresh_io;
    dev_buf<uint8_t> d_covis_io;
    /* place recognition: the database ss_place_set_database keeps (place_db points at the caller's arrays, into place_tab, the
     * rows' problems and the problems' ranges, and into d_place_lists, the inverted file; n_db == 0: none), the tables of a query
     * (q_kf, then q_problem), the workspace of a query, the host form's device copies */
    ss_place_db place_db;
    std::vector<int32_t> place_row_prob; /* the host's copy of the rows' problems: a query's q_kf and q_problem are checked on it */
    staged_table place_tab, place_call_tab;
    dev_buf<uint8_t> d_place_lists, d_place_ws, d_place_io;
    /* PnP RANSAC: the workspace of a call (correspondences, models, poses, counts), the host form's device copies, the tables of a
     * call (views, then frame numbers, then block numbers) */
    dev_buf<uint8_t> d_pnp_ws, d_pnp_io;
    staged_table pnp_tab;
    /* two-view initialisation: the workspace of a call (correspondences, models, partial sums, choices), the host form's device
     * copies, the tables of a call (views, then both sides' frame numbers) */
    dev_buf<uint8_t> d_tv_ws, d_tv_io;
    staged_table tv_tab;
    /* rectification: map map_id in its fixed-point form (one allocation each: the xy array, then ab; d == NULL: unset) and the
     * 16-byte aligned buffer ss_extract_stereo_raw remaps both eyes into */
    struct rect_map {
        uint8_t *d = nullptr;
        int w = 0, h = 0;
    } rect_maps[SS_MAX_RECTIFY_MAPS];
    dev_buf<uint8_t> d_rect;

    /* undistortion: the raw (x, y) pairs of the batch, [max_batch][kcap] (a buffer of ws_table, allocated by raw_xy_buffer on first
     * use, freed with the geometry); whether the current batch was undistorted in place (cleared where last_n_frames is set); the
     * cameras of a call */
    float2 *d_raw_xy = nullptr;
    bool batch_undistorted = false;
    staged_table undist_tab;
    /* map points from depth: the views of a call, the host form's device copies */
    staged_table unproject_tab;
    dev_buf<uint8_t> d_unproject_io;

    int last_n_frames = 0;
    ss_lvl0 last_lvl0; /* where level 0 of the last batch lives (ptr == NULL: in the pyramid block) */

    /* ss_track: one state per camera id, slots taken in the order the ids first appear; host geometry buffers */
    cam_track cams[SS_MAX_CAMERAS];
    int n_cams = 0;
    std::vector<float> h_xy;
    std::vector<int32_t> h_oct, h_midx;
    std::vector<uint16_t> h_md1;

    /* SENDSLAM_TRACK_TIMING=1: host seconds of the pose step, printed at ss_destroy (match = enqueue + wait for the device match,
     * geometry = sst_tracker::step, keep = copies of the descriptors the next frame matches against) */
    bool track_timing = false;
    double t_match = 0, t_geom = 0, t_keep = 0;
    int64_t n_tracked = 0;
    bool profile = false;
    std::vector<stage_rec> stages;
    std::vector<hipEvent_t> event_pool;
};

namespace ss_detail __attribute__((visibility("hidden"))) {

/* records msg as the context's last error (c NULL: as ss_create's) and returns code */
int fail(ss_ctx *c, int code, const std::string &msg);

#define HIP_TRY(c, call)                                                                      \
    do {                                                                                      \
        hipError_t e_ = (call);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return fail((c), e_ == hipErrorOutOfMemory ? SS_ERR_NO_MEMORY : SS_ERR_HIP,       \
                        std::string(#call) + ": " + hipGetErrorString(e_));                   \
    } while (0)

inline stage_rec &stage(ss_ctx *c, const char *name)
{
    for (auto &s : c->stages)
        if (s.name == name) return s;
    c->stages.emplace_back();
    c->stages.back().name = name;
    return c->stages.back();
}

inline hipEvent_t get_event(ss_ctx *c)
{
    if (!c->event_pool.empty()) {
        hipEvent_t e = c->event_pool.back();
        c->event_pool.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
}

struct stage_timer {
    ss_ctx *c;
    stage_rec *s = nullptr;
    hipEvent_t a = nullptr, b = nullptr;
    hipStream_t on;
    stage_timer(ss_ctx *ctx, const char *name, int64_t bytes, hipStream_t stream = nullptr)
        : c(ctx), on(stream ? stream : ctx->stream)
    {
        if (!c->profile) return;
        s = &stage(c, name);
        s->bytes = bytes;
        a = get_event(c);
        b = get_event(c);
        (void)hipEventRecord(a, on); /* on the stream the kernel is launched on */
    }
    ~stage_timer()
    {
        if (!s) return;
        (void)hipEventRecord(b, on);
        s->pending.emplace_back(a, b);
    }
};

template <typename T> int grow(ss_ctx *c, dev_buf<T> &b, size_t want)
{
    if (b.bytes >= want) return SS_OK;
    (void)hipStreamSynchronize(c->stream);
    dev_free(b);
    HIP_TRY(c, hipMalloc((void **)&b.p, want));
    b.bytes = want;
    return SS_OK;
}

/* `bytes` of a host table -> t.d on c->stream.  fill(uint8_t *) writes them into the pinned side once the previous call's copy
 * has left it, so the copy is asynchronous and the caller's arrays are free when this returns. */
template <typename Fill> int staged_upload(ss_ctx *c, staged_table &t, size_t bytes, Fill fill)
{
    const int rc = grow(c, t.d, bytes);
    if (rc != SS_OK) return rc;
    if (t.copied) HIP_TRY(c, hipEventSynchronize(t.copied));
    else HIP_TRY(c, hipEventCreateWithFlags(&t.copied, hipEventDisableTiming));
    if (t.h_bytes < bytes) {
        if (t.h) (void)hipHostFree(t.h);
        t.h = nullptr;
        t.h_bytes = 0;
        HIP_TRY(c, hipHostMalloc((void **)&t.h, bytes, hipHostMallocDefault));
        t.h_bytes = bytes;
    }
    fill(t.h);
    HIP_TRY(c, hipMemcpyAsync(t.d, t.h, bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipEventRecord(t.copied, c->stream));
    return SS_OK;
}

inline void staged_free(staged_table &t)
{
    dev_free(t.d);
    if (t.h) (void)hipHostFree(t.h);
    if (t.copied) (void)hipEventDestroy(t.copied);
    t = staged_table();
}

/* A host train table [n] -> c->train_src.  train_src NULL: frame b against frame b - 1, frame 0 without a train. */
int upload_train_src(ss_ctx *c, const int32_t *train_src, int n);

/* The frame_error array a stage of the last batch reads: the extraction's own, or, where a test hook names frames, a copy of it
 * on c->stream in which those frames carry SS_ERR_OVERFLOW. */
int flagged_frame_error(ss_ctx *c, const std::vector<int> &frames, const int32_t **out);

/* c->d_raw_xy, allocated through the workspace's buffer table when it is not there yet (needs the geometry) */
int raw_xy_buffer(ss_ctx *c);

/* Hands out the pieces of one buffer in order, each on a 256-byte boundary.  With a null base it only measures. */
struct carve {
    uint8_t *base;
    size_t at = 0;
    explicit carve(uint8_t *p) : base(p) {}
    template <typename T> T *take(size_t bytes)
    {
        T *piece = base ? (T *)(base + at) : nullptr;
        at += (bytes + 255) & ~(size_t)255;
        return piece;
    }
    size_t total() const { return at; }
};

/* grows b to what layout(carve &) takes, then lets it take its pieces from b: layout runs twice, the first time on a null base */
template <typename Layout> int carve_from(ss_ctx *c, dev_buf<uint8_t> &b, Layout layout)
{
    carve measure(nullptr);
    layout(measure);
    const int rc = grow(c, b, measure.total());
    if (rc != SS_OK) return rc;
    carve pieces(b.p);
    layout(pieces);
    return SS_OK;
}

} // namespace ss_detail
