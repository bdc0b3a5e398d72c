/*
 * ss_api.cpp -- the C ABI of libsendslam_orb.so (include/sendslam_orb.h): the context's life cycle, HBM
 * buffers, the per-batch kernel sequence on ONE HIP stream, the all-pairs matchers, tracking, stereo, rectification,
 * HIP-event stage timing and debug.  The search family is in ss_api_search.cpp; the context and the helpers both
 * sources are written with are in ss_ctx.h.
 *
 * Host-side counterpart of the reference shim's frame branch
 * (/root/reference/slam_backends/orb_slam_3/orbslam3_mono_networked.cc:521-627): same
 * guards and the same log-and-skip error policy, with the ORB-SLAM3 call at :594 replaced
 * by the kernel sequence below.  No CPU fallback exists: every stage runs on the device.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "ss_ctx.h"

namespace {

thread_local std::string g_create_error;

} // namespace

namespace ss_detail {

int fail(ss_ctx *c, int code, const std::string &msg)
{
    if (c) c->err = msg;
    else g_create_error = msg;
    return code;
}

int flagged_frame_error(ss_ctx *c, const std::vector<int> &frames, const int32_t **out)
{
    *out = c->ws.frame_error;
    if (frames.empty()) return SS_OK;
    static const int32_t flagged = SS_ERR_OVERFLOW;
    const int rc = grow(c, c->d_test_err, (size_t)c->last_n_frames * sizeof(int32_t));
    if (rc != SS_OK) return rc;
    HIP_TRY(c, hipMemcpyAsync(c->d_test_err, c->ws.frame_error, (size_t)c->last_n_frames * sizeof(int32_t), hipMemcpyDeviceToDevice, c->stream));
    for (int f : frames)
        if (f >= 0 && f < c->last_n_frames)
            HIP_TRY(c, hipMemcpyAsync(c->d_test_err + f, &flagged, sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    *out = c->d_test_err;
    return SS_OK;
}

int upload_train_src(ss_ctx *c, const int32_t *train_src, int n)
{
    return staged_upload(c, c->train_src, (size_t)n * sizeof(int32_t), [&](uint8_t *h) {
        int32_t *src = (int32_t *)h;
        for (int b = 0; b < n; b++) src[b] = train_src ? train_src[b] : b - 1;
    });
}

} // namespace ss_detail

namespace {

void collect_events(ss_ctx *c)
{
    for (auto &s : c->stages) {
        for (auto &p : s.pending) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, p.first, p.second) == hipSuccess) s.ms.push_back(ms);
            c->event_pool.push_back(p.first);
            c->event_pool.push_back(p.second);
        }
        s.pending.clear();
    }
}

/* The buffers of c->ws in allocation order: the one place where their sizes live.  ensure_geometry, free_geometry_buffers and
 * the first ss_debug_fetch(2) walk it (ws_alloc: one hipMalloc per buffer). */
/* a group is allocated and uploaded in table order, then cleared: with the geometry; desc_x, after that group's clears; score, when
 * ss_debug_fetch(2) first asks for it; raw_xy, when the first in-place undistortion asks for it */
enum ws_when { WS_GEOMETRY, WS_OPERANDS, WS_FIRST_USE, WS_RAW_XY };
struct ws_buf {
    void **p;
    size_t bytes;      /* from the geometry and max_batch; 0: not allocated */
    const void *host;  /* the host table whose host_bytes are uploaded, or NULL */
    size_t host_bytes;
    bool zero;         /* cleared once */
    ws_when when;
};
std::array<ws_buf, 29> ws_table(ss_ctx *c)
{
    ssk_extract_ws &w = c->ws;
    const ss_geom &g = c->hg;
    const ss_host_tables &t = c->tabs;
    const size_t B = (size_t)c->params.max_batch, K = B * g.kcap;
    const size_t rtab = t.rtab.size() * sizeof(ss_rtab), tiles = t.tile_recs.size() * sizeof(uint32_t);
    const size_t cinfo = t.cinfo.size() * sizeof(uint16_t), units = t.cell_units.size() * sizeof(uint32_t);
    /* desc_x: zeroed once, a row that was never written contributes 0 to every dot product (and is masked out anyway) */
    const bool operands = !c->no_desc_x && g.kcap >= SSK_MATCH_MFMA_MIN_QUERIES;
#define WS(m) (void **)&w.m
    return {{
        {WS(dg), sizeof(ss_geom), &g, sizeof(ss_geom)},
        {WS(rtab), std::max<size_t>(t.rtab.size(), 1) * sizeof(ss_rtab), t.rtab.data(), rtab},
        {WS(tile_recs), tiles, t.tile_recs.data(), tiles},
        {WS(pyr), B * g.block_bytes},
        {WS(blur), B * g.block_bytes},
        {WS(score), B * g.block_bytes, nullptr, 0, false, WS_FIRST_USE},
        {WS(cinfo), cinfo, t.cinfo.data(), cinfo},
        {WS(cell_cnt), B * g.n_cells * sizeof(uint32_t)},
        {WS(cand), B * g.cand_total * sizeof(uint32_t)},
        {WS(qbuf0), B * g.cand_total * sizeof(uint32_t)},
        {WS(qbuf1), B * g.cand_total * sizeof(uint32_t)},
        {WS(bucket), B * g.bucket_total * sizeof(uint32_t)},
        {WS(tsurv), B * g.tiles2_total * (size_t)SS_TS_CAP * sizeof(uint32_t)},
        {WS(thdr), B * g.tiles2_total * (size_t)SS_TS_HDR * sizeof(uint32_t)},
        {WS(cell_units), units, t.cell_units.data(), units},
        {WS(nodes), B * g.node_total * sizeof(ss_qnode)},
        {WS(lists), B * g.item_total * 2 * sizeof(int32_t)},
        {WS(sel), B * g.sel_total * sizeof(uint32_t)},
        {WS(state), B * SS_MAX_LEVELS * sizeof(ss_level_state)},
        {WS(kp_ref), K * 2 * sizeof(uint32_t)},
        {WS(od_moments), K * sizeof(int2)},
        {WS(od_steer), K * sizeof(float2)},
        {WS(n_kp), B * sizeof(int32_t), nullptr, 0, true},
        {WS(level_counts), B * SS_MAX_LEVELS * sizeof(int32_t)},
        {WS(frame_error), B * sizeof(int32_t)},
        {WS(kps), K * sizeof(ss_keypoint), nullptr, 0, true},
        {WS(desc), K * SS_DESC_BYTES, nullptr, 0, true},
        {WS(desc_x), operands ? K * SSK_X_ROW : 0, nullptr, 0, true, WS_OPERANDS},
        {(void **)&c->d_raw_xy, K * sizeof(float2), nullptr, 0, false, WS_RAW_XY},
    }};
#undef WS
}

int ws_alloc(ss_ctx *c, ws_when when)
{
    const auto table = ws_table(c);
    for (const ws_buf &b : table) {
        if (b.when != when || !b.bytes) continue;
        HIP_TRY(c, hipMalloc(b.p, b.bytes));
        if (b.host_bytes) HIP_TRY(c, hipMemcpy(*b.p, b.host, b.host_bytes, hipMemcpyHostToDevice));
    }
    for (const ws_buf &b : table)
        if (b.when == when && b.bytes && b.zero) HIP_TRY(c, hipMemset(*b.p, 0, b.bytes));
    return SS_OK;
}

void free_geometry_buffers(ss_ctx *c)
{
    for (const ws_buf &b : ws_table(c)) dev_free(*b.p);
    c->have_geom = false;
}

} // namespace

namespace ss_detail {

int raw_xy_buffer(ss_ctx *c)
{
    if (c->d_raw_xy) return SS_OK;
    return ws_alloc(c, WS_RAW_XY);
}

} // namespace ss_detail

namespace {

int ensure_geometry(ss_ctx *c, int w, int h)
{
    if (c->have_geom && c->hg.w == w && c->hg.h == h) return SS_OK;
    (void)hipStreamSynchronize(c->stream);
    free_geometry_buffers(c);
    std::string msg;
    ss_geom g;
    int rc = ss_build_geometry(c->params, w, h, &g, &c->tabs, &msg);
    if (rc != SS_OK) return fail(c, rc, msg);
    for (int l = 0; l < g.n_levels; l++)
        if (g.lv[l].item_cap > 2048)
            return fail(c, SS_ERR_INVALID_ARG, "n_features too large: per-level quota exceeds 2032");
    c->hg = g;
    {
        /* SENDSLAM_RESIZE_PAIRS=1: two pyramid levels per launch (k_resize_pair: four launches instead of seven, bit-exact).
         * Off by default: alone it takes the same 0.126 ms per 64 frames, with four batches in flight it costs 7.6 % frames/s
         * (31 KB of LDS per block and 10 % more instructions for the overlapping windows) */
        const char *e = getenv("SENDSLAM_RESIZE_PAIRS");
        std::fill(std::begin(c->resize_pair), std::end(c->resize_pair), false); /* flags of the previous geometry do not survive */
        for (int l = 1; l + 1 < g.n_levels && e && atoi(e);)
            if (ssk_resize_pair_fits(g, c->tabs.rtab.data(), l)) { c->resize_pair[l] = true; l += 2; } else l += 1;
    }
    std::fill(std::begin(c->resize_walk), std::end(c->resize_walk), false);
    for (int l = 1; l < g.n_levels; l++) c->resize_walk[l] = ssk_resize_walk_fits(g, c->tabs.rtab.data(), l);
    rc = ws_alloc(c, WS_GEOMETRY);
    if (rc == SS_OK) rc = ws_alloc(c, WS_OPERANDS);
    if (rc != SS_OK) return rc;
    c->have_geom = true;
    c->last_n_frames = 0;
    c->bow_frames = 0;
    c->batch_undistorted = false;
    return SS_OK;
}

int64_t level_px(const ss_geom &g, int l) { return (int64_t)g.lv[l].w * g.lv[l].h; }

/* the per-batch kernel sequence; d_pix is device memory */
int run_extract(ss_ctx *c, const void *d_pix, int n, int channels, int64_t row_stride, int64_t frame_stride, int rgb_flag = -1)
{
    const ss_geom &g = c->hg;
    hipStream_t s = c->stream;
    int64_t all_px = 0;
    for (int l = 0; l < g.n_levels; l++) all_px += level_px(g, l);

    HIP_TRY(c, hipMemsetAsync(c->ws.state, 0, (size_t)n * SS_MAX_LEVELS * sizeof(ss_level_state), s));
    /* A 1-channel image whose base, rows and frames are 16-byte aligned IS pyramid level 0: the kernels read it in
     * place (aligned dword loads work on it as they do on the pyramid block) and the ingest copy is skipped.  The
     * caller's buffer must stay untouched until the batch has finished (it is asynchronous, as before). */
    ss_lvl0 l0;
    if (channels == 1 && ((uintptr_t)d_pix % 16) == 0 && row_stride % 16 == 0 && frame_stride % 16 == 0 &&
        row_stride < (1 << 24) && !c->force_ingest) {
        l0.ptr = (const uint8_t *)d_pix;
        l0.pitch = (int)row_stride;
        l0.frame_stride = frame_stride;
    }
    c->last_lvl0 = l0;
    if (!l0.ptr) {
        int c0 = 0, c1 = 0, c2 = 0;
        if (channels != 1) { /* Camera.RGB: 1 -> byte 0 weighs as R */
            /* rgb_flag: the frame's camera's own Camera.RGB (ss_extract), or -1: the calibration set last */
            const bool rgb = rgb_flag >= 0 ? rgb_flag != 0 : c->calibrated ? c->cam.rgb != 0 : false;
            c0 = rgb ? SS_GRAY_RY : SS_GRAY_BY;
            c1 = SS_GRAY_GY;
            c2 = rgb ? SS_GRAY_BY : SS_GRAY_RY;
        }
        stage_timer t(c, "ingest", n * level_px(g, 0) * (channels + 1));
        ssk_ingest(s, c->ws, g, n, d_pix, channels, row_stride, frame_stride, c0, c1, c2);
    }
    for (int l = 1; l < g.n_levels;) {
        if (c->resize_pair[l]) { /* two pyramid steps, the middle level never read back */
            stage_timer t(c, "resize", n * (level_px(g, l - 1) + level_px(g, l) + level_px(g, l + 1)));
            ssk_resize_pair(s, c->ws, g, n, l, l0);
            c->resize_kernel[l] = c->resize_kernel[l + 1] = SSK_RESIZE_PAIR;
            l += 2;
        } else {
            stage_timer t(c, "resize", n * (level_px(g, l - 1) + level_px(g, l)));
            c->resize_kernel[l] = ssk_resize(s, c->ws, g, n, l, l0, c->resize_walk[l], c->wave_slots);
            l += 1;
        }
    }
    {
        /* algorithmic bytes: read the pyramid once, write the blurred pyramid (the score map and the
         * survivor lists are this design's own intermediates) */
        stage_timer t(c, "fast_blur_nms", n * 2 * all_px);
        ssk_fast_blur_nms(s, c->ws, g, n, l0);
    }
    /* the stages between them take nothing per call */
    static const struct {
        const char *name;
        void (*launch)(hipStream_t, const ssk_extract_ws &, const ss_geom &, int);
    } mid[] = {{"bucket_gather", ssk_bucket_gather}, {"cells_emit", ssk_cells_emit}, {"quadtree", ssk_quadtree}, {"slots", ssk_slots}};
    for (const auto &m : mid) {
        stage_timer t(c, m.name, 0);
        m.launch(s, c->ws, g, n);
    }
    {
        stage_timer t(c, "orient_describe", (int64_t)n * g.n_features * (709 + 512 + 32 + 24));
        ssk_orient_describe(s, c->ws, g, n, l0, c->params.steer_fma != 0);
    }
    HIP_TRY(c, hipGetLastError());
    c->last_n_frames = n;
    c->bow_frames = 0; /* the nodes a BoW transform kept belong to the batch before */
    c->batch_undistorted = false; /* ... and so do the raw pairs an in-place undistortion saved */
    return SS_OK;
}

int check_frame_errors(ss_ctx *c)
{
    const int n = c->last_n_frames;
    if (n <= 0) return SS_OK;
    c->h_err.resize((size_t)n);
    HIP_TRY(c, hipMemcpyAsync(c->h_err.data(), c->ws.frame_error, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < n; i++)
        if (c->h_err[i] != 0)
            return fail(c, SS_ERR_OVERFLOW, "frame " + std::to_string(i) + ": an internal capacity was exceeded (code " +
                                                std::to_string(c->h_err[i]) + "); no result was truncated");
    return SS_OK;
}

/* the frames a test hook names: "frame,frame,..." */
void parse_test_frames(const char *e, std::vector<int> &out)
{
    for (const char *q = e; q && *q;) {
        char *end = nullptr;
        const long f = strtol(q, &end, 10);
        if (end == q) break;
        out.push_back((int)f);
        q = *end == ',' ? end + 1 : end;
    }
}

/* the 8 bytes per query of a match scratch as the matcher's three outputs: idx [n] int32, then d1 [n] and d2 [n] uint16 */
struct match_out {
    int32_t *idx;
    uint16_t *d1, *d2;
};
match_out split_scratch(uint8_t *p, int n) { return {(int32_t *)p, (uint16_t *)(p + (size_t)n * 4), (uint16_t *)(p + (size_t)n * 6)}; }

/* One matcher call on c->stream: plan, grow match_partial to what the plan needs, launch inside a "match" stage of `bytes`
 * algorithmic bytes.  The caller has filled everything but the stream, the partials and the plan. */
int run_match(ss_ctx *c, ssk_match_call &m, int rows_q, int rows_t, int64_t bytes)
{
    m.s = c->stream;
    const int rc = grow(c, c->match_partial, ssk_match_plan(m, rows_q, rows_t));
    if (rc != SS_OK) return rc;
    m.partial = c->match_partial;
    {
        stage_timer t(c, "match", bytes);
        ssk_match(m);
    }
    HIP_TRY(c, hipGetLastError());
    return SS_OK;
}

} // namespace

extern "C" {

/* the ss_track state of camera_id, or NULL when the camera has none yet */
static cam_track *find_camera(ss_ctx *c, int camera_id)
{
    for (int i = 0; i < c->n_cams; i++)
        if (c->cams[i].camera_id == camera_id) return &c->cams[i];
    return nullptr;
}

/* the ss_track state of camera_id: its slot, or a new one while fewer than SS_MAX_CAMERAS ids have been seen */
static int camera_slot(ss_ctx *c, int camera_id, cam_track **out)
{
    for (int i = 0; i < c->n_cams; i++)
        if (c->cams[i].camera_id == camera_id) {
            *out = &c->cams[i];
            return SS_OK;
        }
    if (c->n_cams == SS_MAX_CAMERAS)
        return fail(c, SS_ERR_INVALID_ARG, "camera " + std::to_string(camera_id) + ": this context tracks " + std::to_string(SS_MAX_CAMERAS) +
                                               " cameras already (SS_MAX_CAMERAS)");
    cam_track &ct = c->cams[c->n_cams++];
    ct.camera_id = camera_id;
    *out = &ct;
    return SS_OK;
}

/* the previous frame's rows of a camera are still the caller's (SS_TRACK_DESC_STAYS_VALID): copy them into the camera's own
 * buffers (and their operand form), so that the caller may reuse its rows once this has returned */
static int detach_rows(ss_ctx *c, cam_track &ct)
{
    if (!ct.d_prev_ext) return SS_OK;
    const int n = ct.prev_ext_n;
    int rc = grow(c, ct.d_prev_desc, (size_t)n * SS_DESC_BYTES);
    if (rc != SS_OK) return rc;
    HIP_TRY(c, hipMemcpyAsync(ct.d_prev_desc, ct.d_prev_ext, (size_t)n * SS_DESC_BYTES, hipMemcpyDeviceToDevice, c->stream));
    if (!c->no_desc_x) {
        rc = grow(c, ct.d_prev_desc_x, (size_t)SS_EXPANDED_BYTES(n));
        if (rc != SS_OK) return rc;
        ssk_expand_desc(c->stream, ct.d_prev_ext, n, ct.d_prev_desc_x);
        HIP_TRY(c, hipGetLastError());
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    ct.d_prev_ext = nullptr;
    ct.prev_ext_n = 0;
    return SS_OK;
}

int ss_abi_version(void) { return SS_ABI_VERSION; }

int ss_orb_params_default(ss_orb_params *p)
{
    if (!p) return SS_ERR_INVALID_ARG;
    p->n_features = SS_DEFAULT_NFEATURES;
    p->scale_factor = SS_DEFAULT_SCALE;
    p->n_levels = SS_DEFAULT_NLEVELS;
    p->ini_th_fast = SS_DEFAULT_INI_TH;
    p->min_th_fast = SS_DEFAULT_MIN_TH;
    p->lapping_x0 = SS_DEFAULT_LAPPING_X0;
    p->lapping_x1 = SS_DEFAULT_LAPPING_X1;
    p->max_batch = 1;
    p->steer_fma = 0;
    return SS_OK;
}

int ss_create(int device_ordinal, const ss_orb_params *params, ss_ctx **out)
{
    if (!out) return fail(nullptr, SS_ERR_INVALID_ARG, "ss_create: out is NULL");
    *out = nullptr;
    ss_orb_params p;
    ss_orb_params_default(&p);
    if (params) p = *params;
    if (p.max_batch < 1 || p.max_batch > 4096) return fail(nullptr, SS_ERR_INVALID_ARG, "max_batch out of range (1..4096)");
    int n_dev = 0;
    hipError_t e = hipGetDeviceCount(&n_dev);
    if (e != hipSuccess || n_dev <= 0)
        return fail(nullptr, SS_ERR_NO_DEVICE,
                    std::string("no HIP device: this library has no CPU path (") + hipGetErrorString(e) + ")");
    if (device_ordinal < 0 || device_ordinal >= n_dev)
        return fail(nullptr, SS_ERR_NO_DEVICE, "device ordinal " + std::to_string(device_ordinal) + " out of range");
    HIP_TRY((ss_ctx *)nullptr, hipSetDevice(device_ordinal));
    int n_cus = 0;
    HIP_TRY((ss_ctx *)nullptr, hipDeviceGetAttribute(&n_cus, hipDeviceAttributeMultiprocessorCount, device_ordinal));
    if (n_cus <= 0) return fail(nullptr, SS_ERR_HIP, "device reports no compute units");
    {
        /* validate the parameters on a nominal size now, so a bad parameter fails here */
        ss_geom g;
        ss_host_tables tabs;
        std::string msg;
        int rc = ss_build_geometry(p, 640, 480, &g, &tabs, &msg);
        if (rc == SS_ERR_INVALID_ARG) return fail(nullptr, rc, msg);
    }
    ss_ctx *c = new ss_ctx();
    c->device = device_ordinal;
    c->wave_slots = (int64_t)SSK_WAVE_SLOTS_PER_CU * n_cus;
    c->params = p;
    if (const char *e = getenv("SENDSLAM_FORCE_INGEST")) c->force_ingest = atoi(e) != 0;
    if (const char *e = getenv("SENDSLAM_TRACK_TIMING")) c->track_timing = atoi(e) != 0;
    if (const char *e = getenv("SENDSLAM_MATCH_PACKED")) c->no_desc_x = atoi(e) != 0;
    parse_test_frames(getenv("SENDSLAM_TEST_STEREO_FLAG"), c->stereo_test_flagged);
    parse_test_frames(getenv("SENDSLAM_TEST_FLAG_BATCH"), c->batch_test_flagged);
    hipError_t se = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (se != hipSuccess) {
        delete c;
        return fail(nullptr, SS_ERR_HIP, std::string("hipStreamCreate: ") + hipGetErrorString(se));
    }
    *out = c;
    return SS_OK;
}

int ss_destroy(ss_ctx *c)
{
    if (!c) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    if (c->track_timing && c->n_tracked)
        fprintf(stderr, "ss_track timing over %lld frames: match %.3f ms, geometry %.3f ms, keep %.3f ms per frame\n", (long long)c->n_tracked,
                1e3 * c->t_match / c->n_tracked, 1e3 * c->t_geom / c->n_tracked, 1e3 * c->t_keep / c->n_tracked);
    collect_events(c);
    for (auto e : c->event_pool) (void)hipEventDestroy(e);
    free_geometry_buffers(c);
    dev_free(c->d_in);
    dev_free(c->match_partial);
    dev_free(c->d_mq);
    dev_free(c->d_mt);
    dev_free(c->d_mout);
    dev_free(c->d_part_tmp);
    dev_free(c->d_qx);
    dev_free(c->d_tx);
    staged_free(c->train_src);
    dev_free(c->d_carry_x);
    dev_free(c->d_stereo);
    dev_free(c->d_test_err);
    dev_free(c->d_guided_ws);
    dev_free(c->d_guided_io);
    dev_free(c->d_proj_io);
    staged_free(c->proj_tab);
    dev_free(c->d_voc);
    dev_free(c->d_bow_ws);
    dev_free(c->d_bow_keep);
    dev_free(c->d_epi_ws);
    dev_free(c->d_tri_ws);
    staged_free(c->epi_tab);
    dev_free(c->d_sim3_ws);
    dev_free(c->d_sim3_io);
    staged_free(c->sim3_tab);
    dev_free(c->d_pnp_ws);
    dev_free(c->d_pnp_io);
    staged_free(c->pnp_tab);
    dev_free(c->d_tv_ws);
    dev_free(c->d_tv_io);
    staged_free(c->tv_tab);
    dev_free(c->d_pose_ws);
    dev_free(c->d_pose_io);
    staged_free(c->pose_tab);
    dev_free(c->d_ba_ws);
    dev_free(c->d_ba_io);
    staged_free(c->ba_tab);
    staged_free(c->ba_block_tab);
    dev_free(c->d_graph_ws);
    dev_free(c->d_graph_io);
    staged_free(c->graph_tab);
    dev_free(c->d_gba_ws);
    dev_free(c->d_gba_io);
    staged_free(c->gba_tab);
    staged_free(c->covis_tab);
    staged_free(c->covis_call_tab);
    dev_free(c->d_covis_io);
    staged_free(c->refresh_tab);
    dev_free(c->d_refresh_io);
    staged_free(c->undist_tab);
    staged_free(c->unproject_tab);
    dev_free(c->d_unproject_io);
    staged_free(c->place_tab);
    staged_free(c->place_call_tab);
    dev_free(c->d_place_lists);
    dev_free(c->d_place_ws);
    dev_free(c->d_place_io);
    dev_free(c->d_sim3opt_ws);
    dev_free(c->d_sim3opt_io);
    staged_free(c->sim3opt_tab);
    for (auto &rm : c->rect_maps) dev_free(rm.d);
    dev_free(c->d_rect);
    for (cam_track &ct : c->cams) ct.free_rows();
    (void)hipStreamDestroy(c->stream);
    delete c;
    return SS_OK;
}

const char *ss_last_error(const ss_ctx *c) { return c ? c->err.c_str() : g_create_error.c_str(); }

int ss_set_calibration(ss_ctx *c, int camera_id, const ss_camera *cam)
{
    if (!c) return SS_ERR_INVALID_ARG;
    if (camera_id == 0) return fail(c, SS_ERR_INVALID_ARG, "Calibration message missing camera identifier.");
    if (!cam) return fail(c, SS_ERR_INVALID_ARG, "Calibration message missing structured parameter payload.");
    cam_track *ct = nullptr;
    const int rc = camera_slot(c, camera_id, &ct);
    if (rc != SS_OK) return rc;
    c->cam = *cam;
    c->cam.type[sizeof(c->cam.type) - 1] = 0;
    c->cam_id = camera_id;
    c->calibrated = true;
    /* the reference rebuilds the whole ORB_SLAM3::System on every calibration message (:491-518): the map, the
     * reference frame and the motion model do not survive it -- of this camera; the others keep tracking */
    ct->cam = c->cam;
    ct->has_cam = true;
    ct->reset();
    return SS_OK;
}

/* The image-argument checks of the extraction entry points, in their order of precedence; `no_image` and `small` are the entry
 * point's own wording of the first and the last one.  A single image is one frame of frame_stride row_stride * height. */
static int check_image_args(ss_ctx *c, bool have_pixels, int n_frames, int width, int height, int channels, int64_t row_stride,
                            int64_t frame_stride, bool needs_calibration, const char *no_image, const char *small)
{
    if (!have_pixels || n_frames < 1 || width <= 0 || height <= 0) return fail(c, SS_ERR_BAD_FRAME, no_image);
    if (n_frames > c->params.max_batch) return fail(c, SS_ERR_INVALID_ARG, "n_frames exceeds max_batch of this context");
    if (channels != 1 && channels != 3 && channels != 4) return fail(c, SS_ERR_BAD_FRAME, "unsupported channel count");
    if (needs_calibration && channels != 1 && !c->calibrated)
        return fail(c, SS_ERR_NOT_CALIBRATED, "Received frame before calibration. Ignoring.");
    if (row_stride < (int64_t)width * channels || frame_stride < row_stride * height) return fail(c, SS_ERR_BAD_FRAME, small);
    return SS_OK;
}

/* upload footprint of one host image: the last row of a tight caller buffer ends after width * channels bytes, not after
 * row_stride; frames lie `alloc` (16-byte rounded) apart in d_in */
struct upload_size {
    size_t bytes, alloc;
};
static upload_size upload_footprint(int width, int height, int channels, int row_stride)
{
    return {(size_t)row_stride * (height - 1) + (size_t)width * channels, ((size_t)row_stride * height + 15) & ~(size_t)15};
}

/* frame f's nk keypoints and descriptors -> the host vectors, which *out then points to; the copies are asynchronous on
 * c->stream and out->level_counts is the caller's */
static int fetch_rows(ss_ctx *c, int f, int32_t nk, std::vector<ss_keypoint> &kps, std::vector<uint8_t> &desc, int camera_id, double timestamp,
                      ss_frame_result *out)
{
    const size_t row0 = (size_t)f * c->hg.kcap;
    kps.resize((size_t)std::max(nk, 1));
    desc.resize((size_t)std::max(nk, 1) * SS_DESC_BYTES);
    if (nk > 0) {
        HIP_TRY(c, hipMemcpyAsync(kps.data(), c->ws.kps + row0, (size_t)nk * sizeof(ss_keypoint), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipMemcpyAsync(desc.data(), c->ws.desc + row0 * SS_DESC_BYTES, (size_t)nk * SS_DESC_BYTES, hipMemcpyDeviceToHost, c->stream));
    }
    out->n_keypoints = nk;
    out->camera_id = camera_id;
    out->timestamp = timestamp;
    out->keypoints = kps.data();
    out->descriptors = desc.data();
    return SS_OK;
}

int ss_extract(ss_ctx *c, int camera_id, const uint8_t *pix, int width, int height, int channels, int row_stride,
               double timestamp, ss_frame_result *out)
{
    if (!c || !out) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    if (camera_id == 0) return fail(c, SS_ERR_BAD_FRAME, "Frame message missing camera identifier.");
    int rc = check_image_args(c, pix != nullptr, 1, width, height, channels, row_stride, (int64_t)row_stride * height, true,
                              "Frame message missing binary image data.", "row_stride smaller than a row");
    if (rc == SS_OK) rc = ensure_geometry(c, width, height);
    if (rc != SS_OK) return rc;
    const upload_size up = upload_footprint(width, height, channels, row_stride);
    rc = grow(c, c->d_in, up.alloc);
    if (rc != SS_OK) return rc;
    HIP_TRY(c, hipMemcpyAsync(c->d_in, pix, up.bytes, hipMemcpyHostToDevice, c->stream));
    /* the caller keeps ownership of pix: it is consumed before we return */
    const cam_track *own = find_camera(c, camera_id);
    rc = run_extract(c, c->d_in, 1, channels, row_stride, (int64_t)up.alloc, own && own->has_cam ? (own->cam.rgb != 0) : -1);
    if (rc != SS_OK) return rc;
    int32_t nk = 0;
    HIP_TRY(c, hipMemcpyAsync(&nk, c->ws.n_kp, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(out->level_counts, c->ws.level_counts, SS_MAX_LEVELS * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    rc = check_frame_errors(c); /* synchronises */
    if (rc == SS_OK) rc = fetch_rows(c, 0, nk, c->h_kps, c->h_desc, camera_id, timestamp, out);
    if (rc != SS_OK) return rc;
    if (nk > 0) HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SS_OK;
}

int ss_extract_batch_device(ss_ctx *c, const void *d_pix, int n_frames, int width, int height, int channels,
                            int64_t row_stride, int64_t frame_stride)
{
    if (!c) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    int rc = check_image_args(c, d_pix != nullptr, n_frames, width, height, channels, row_stride, frame_stride, true, "empty batch",
                              "strides smaller than the frame");
    if (rc == SS_OK) rc = ensure_geometry(c, width, height);
    if (rc != SS_OK) return rc;
    return run_extract(c, d_pix, n_frames, channels, row_stride, frame_stride);
}

int ss_get_batch_view(ss_ctx *c, ss_batch_view *out)
{
    if (!c || !out) return SS_ERR_INVALID_ARG;
    if (!c->have_geom || c->last_n_frames <= 0) return fail(c, SS_ERR_STATE, "no batch has been extracted");
    out->n_frames = c->last_n_frames;
    out->kp_capacity = c->hg.kcap;
    out->keypoints = c->ws.kps;
    out->descriptors = c->ws.desc;
    out->n_keypoints = c->ws.n_kp;
    out->level_counts = c->ws.level_counts;
    out->frame_error = c->ws.frame_error;
    return SS_OK;
}

int ss_fetch_frame(ss_ctx *c, int frame, ss_frame_result *out)
{
    if (!c || !out) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    if (!c->have_geom || frame < 0 || frame >= c->last_n_frames) return fail(c, SS_ERR_STATE, "ss_fetch_frame: no such frame");
    int rc = check_frame_errors(c);
    if (rc != SS_OK) return rc;
    int32_t nk = 0;
    HIP_TRY(c, hipMemcpyAsync(&nk, c->ws.n_kp + frame, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(out->level_counts, c->ws.level_counts + (size_t)frame * SS_MAX_LEVELS, SS_MAX_LEVELS * sizeof(int32_t),
                              hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    rc = fetch_rows(c, frame, nk, c->h_kps, c->h_desc, c->cam_id, 0.0, out);
    if (rc != SS_OK) return rc;
    if (nk > 0) HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SS_OK;
}

/* one query set against one train set: one frame, no strides, no count arrays */
static ssk_match_call single_call(const void *d_query, int n_query, const void *d_train, int n_train, int exclude_self, int th, int ratio_num,
                                  int ratio_den, void *d_idx, void *d_d1, void *d_d2)
{
    ssk_match_call m;
    m.query = d_query, m.train = d_train ? d_train : d_query;
    m.nq_fixed = m.out_stride = n_query, m.nt_fixed = n_train;
    m.exclude_self_mode = exclude_self ? 1 : 0;
    m.th = th, m.rnum = ratio_num, m.rden = ratio_den;
    m.idx = (int32_t *)d_idx, m.d1 = (uint16_t *)d_d1, m.d2 = (uint16_t *)d_d2;
    return m;
}

/* the argument guard of a single match on device rows: true when the call ends here, with *rc (an error, or no query to match) */
static bool match_ends(ss_ctx *c, const void *d_query, int n_query, const void *d_train, int n_train, int ratio_num, int ratio_den,
                       const void *d_idx, const void *d_d1, const void *d_d2, int *rc)
{
    *rc = SS_OK;
    if (!c) {
        *rc = SS_ERR_INVALID_ARG;
    } else {
        (void)hipSetDevice(c->device);
        if (n_query < 0 || n_train < 0 || ratio_den <= 0 || ratio_num < 0) *rc = fail(c, SS_ERR_INVALID_ARG, "bad match arguments");
        else if (n_query > 0 && (!d_query || (!d_train && n_train > 0) || !d_idx || !d_d1 || !d_d2)) *rc = fail(c, SS_ERR_INVALID_ARG, "NULL match buffer");
    }
    return *rc != SS_OK || n_query == 0;
}

/* one expanded query set against one expanded train set (any size).  q_packed / t_packed: the same rows as packed descriptors
 * when the caller has them (the finishing launch reads those) */
static int match_expanded(ss_ctx *c, const void *d_query_x, int n_query, const void *d_train_x, int n_train, int th, int ratio_num,
                          int ratio_den, int exclude_self, void *d_idx, void *d_d1, void *d_d2, const uint8_t *q_packed, const uint8_t *t_packed)
{
    int rc;
    if (match_ends(c, d_query_x, n_query, d_train_x, n_train, ratio_num, ratio_den, d_idx, d_d1, d_d2, &rc)) return rc;
    ssk_match_call m = single_call(d_query_x, n_query, d_train_x, n_train, exclude_self, th, ratio_num, ratio_den, d_idx, d_d1, d_d2);
    m.operand_rows = true;
    m.query_p = q_packed, m.train_p = t_packed;
    return run_match(c, m, n_query, std::max(n_train, 1), (int64_t)n_query * SSK_X_ROW + (int64_t)n_train * SSK_X_ROW + (int64_t)n_query * 8);
}

int ss_match_device(ss_ctx *c, const void *d_query, int n_query, const void *d_train, int n_train, int th,
                    int ratio_num, int ratio_den, int exclude_self, void *d_idx, void *d_d1, void *d_d2)
{
    int rc;
    if (match_ends(c, d_query, n_query, d_train, n_train, ratio_num, ratio_den, d_idx, d_d1, d_d2, &rc)) return rc;
    if (n_query <= 8 && n_train >= 65536 && !exclude_self) {
        /* a handful of queries against a large database: stream the database once (HBM-bound) */
        rc = grow(c, c->match_partial, (size_t)SSK_STREAM_PARTIAL_MAX);
        if (rc != SS_OK) return rc;
        int s_len = 0, s_chunks = 0;
        if (ssk_match_stream_plan(n_query, n_train, c->match_partial.bytes, &s_len, &s_chunks)) {
            {
                /* the kernel that reads the database exactly once: timed on its own (bench.py match_stream_roofline) */
                stage_timer t(c, "match_stream_kernel", (int64_t)n_query * 32 + (int64_t)n_train * 32 + (int64_t)s_chunks * n_query * 8);
                ssk_match_stream_kernel(c->stream, d_query, d_train, n_query, n_train, s_len, s_chunks, c->match_partial);
            }
            {
                stage_timer t(c, "match_stream_merge", (int64_t)s_chunks * n_query * 8 + (int64_t)n_query * 8);
                ssk_match_stream_merge(c->stream, c->match_partial, n_query, s_chunks, th, ratio_num, ratio_den, (int32_t *)d_idx,
                                       (uint16_t *)d_d1, (uint16_t *)d_d2);
            }
            HIP_TRY(c, hipGetLastError());
            return SS_OK;
        }
    }
    if (n_query >= SSK_MATCH_MFMA_MIN_QUERIES && n_train > 0 && !c->no_desc_x) {
        /* ONE matrix-core matcher for every entry point: the caller's packed rows are expanded to its operand format
         * (k_expand_desc: 32 -> 128 bytes per row) and k_match_mfma_x runs on them.  SENDSLAM_MATCH_PACKED=1 keeps round 1's
         * k_match_mfma, which expands every tile in every query block through an LDS table. */
        const bool same = d_train == d_query && n_train == n_query;
        rc = grow(c, c->d_qx, (size_t)SS_EXPANDED_BYTES(n_query));
        if (rc == SS_OK && !same) rc = grow(c, c->d_tx, (size_t)SS_EXPANDED_BYTES(n_train));
        if (rc != SS_OK) return rc;
        {
            stage_timer t(c, "expand", ((int64_t)n_query + (same ? 0 : n_train)) * (32 + SSK_X_ROW));
            ssk_expand_desc(c->stream, d_query, n_query, c->d_qx);
            if (!same) ssk_expand_desc(c->stream, d_train, n_train, c->d_tx);
        }
        return match_expanded(c, c->d_qx, n_query, same ? c->d_qx : c->d_tx, n_train, th, ratio_num, ratio_den, exclude_self, d_idx, d_d1, d_d2,
                              (const uint8_t *)d_query, (const uint8_t *)d_train);
    }
    ssk_match_call m = single_call(d_query, n_query, d_train, n_train, exclude_self, th, ratio_num, ratio_den, d_idx, d_d1, d_d2);
    return run_match(c, m, n_query, std::max(n_train, 1), (int64_t)n_query * 32 + (int64_t)n_train * 32 + (int64_t)n_query * 8);
}

int ss_match(ss_ctx *c, const uint8_t *query, int n_query, const uint8_t *train, int n_train, int th, int ratio_num,
             int ratio_den, int exclude_self, int32_t *idx, uint16_t *d1, uint16_t *d2)
{
    if (!c) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    if (n_query < 0 || n_train < 0) return fail(c, SS_ERR_INVALID_ARG, "bad match arguments");
    if (n_query == 0) return SS_OK;
    if (!query || (!train && n_train > 0) || !idx || !d1 || !d2) return fail(c, SS_ERR_INVALID_ARG, "NULL match buffer");
    int rc = grow(c, c->d_mq, (size_t)n_query * 32);
    if (rc == SS_OK) rc = grow(c, c->d_mt, (size_t)std::max(n_train, 1) * 32);
    if (rc == SS_OK) rc = grow(c, c->d_mout, (size_t)n_query * 8);
    if (rc != SS_OK) return rc;
    HIP_TRY(c, hipMemcpyAsync(c->d_mq, query, (size_t)n_query * 32, hipMemcpyHostToDevice, c->stream));
    if (n_train > 0) HIP_TRY(c, hipMemcpyAsync(c->d_mt, train, (size_t)n_train * 32, hipMemcpyHostToDevice, c->stream));
    const match_out o = split_scratch(c->d_mout, n_query);
    rc = ss_match_device(c, c->d_mq, n_query, c->d_mt, n_train, th, ratio_num, ratio_den, exclude_self, o.idx, o.d1, o.d2);
    if (rc != SS_OK) return rc;
    HIP_TRY(c, hipMemcpyAsync(idx, o.idx, (size_t)n_query * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d1, o.d1, (size_t)n_query * 2, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d2, o.d2, (size_t)n_query * 2, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SS_OK;
}

/* the frames of the last batch against frames of the same batch: the extraction's rows, as operands where it wrote them */
static ssk_match_call batch_call(ss_ctx *c, int th, int ratio_num, int ratio_den, void *d_idx, void *d_d1, void *d_d2)
{
    const int kcap = c->hg.kcap;
    ssk_match_call m;
    m.n_frames = c->last_n_frames;
    m.operand_rows = c->ws.desc_x != nullptr;
    m.query = m.train = m.operand_rows ? c->ws.desc_x : c->ws.desc;
    m.q_frame_stride = m.t_frame_stride = m.operand_rows ? (int64_t)kcap * SSK_X_ROW : (int64_t)kcap * 8;
    if (m.operand_rows) {
        m.query_p = m.train_p = c->ws.desc;
        m.qp_frame_stride = m.tp_frame_stride = (int64_t)kcap * SS_DESC_BYTES;
    }
    m.nq_arr = m.nt_arr = c->ws.n_kp;
    m.th = th, m.rnum = ratio_num, m.rden = ratio_den;
    m.out_stride = kcap;
    m.idx = (int32_t *)d_idx, m.d1 = (uint16_t *)d_d1, m.d2 = (uint16_t *)d_d2;
    return m;
}
static int run_batch_match(ss_ctx *c, ssk_match_call &m)
{
    const int64_t nf = c->hg.n_features;
    return run_match(c, m, c->hg.kcap, c->hg.kcap, (int64_t)m.n_frames * (nf * 32 * 2 + nf * 8));
}

int ss_match_batch_device(ss_ctx *c, int mode, int th, int ratio_num, int ratio_den, void *d_idx, void *d_d1, void *d_d2)
{
    if (!c) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    if (!c->have_geom || c->last_n_frames <= 0) return fail(c, SS_ERR_STATE, "no batch has been extracted");
    if ((mode != 0 && mode != 1) || !d_idx || !d_d1 || !d_d2 || ratio_den <= 0) return fail(c, SS_ERR_INVALID_ARG, "bad match arguments");
    ssk_match_call m = batch_call(c, th, ratio_num, ratio_den, d_idx, d_d1, d_d2);
    m.train_frame_shift = mode == 0 ? 0 : -1;
    m.exclude_self_mode = mode == 0 ? 1 : 2;
    return run_batch_match(c, m);
}

int ss_match_batch_sources_device(ss_ctx *c, const int32_t *train_src, const void *d_carry, const void *d_carry_n, int n_carry, int th,
                                  int ratio_num, int ratio_den, void *d_idx, void *d_d1, void *d_d2)
{
    if (!c) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    if (!c->have_geom || c->last_n_frames <= 0) return fail(c, SS_ERR_STATE, "no batch has been extracted");
    if (!train_src || !d_idx || !d_d1 || !d_d2 || ratio_den <= 0 || n_carry < 0 || (n_carry > 0 && (!d_carry || !d_carry_n)))
        return fail(c, SS_ERR_INVALID_ARG, "bad match arguments");
    const int n = c->last_n_frames, kcap = c->hg.kcap;
    for (int b = 0; b < n; b++) {
        const int t = train_src[b];
        if (t >= n || t < -1 - n_carry)
            return fail(c, SS_ERR_INVALID_ARG, "train_src[" + std::to_string(b) + "] = " + std::to_string(t) + " names no frame of the batch (" +
                                                   std::to_string(n) + ") or of the carry (" + std::to_string(n_carry) + ")");
    }
    int rc = upload_train_src(c, train_src, n);
    if (rc != SS_OK) return rc;
    ssk_table tab{c->train_src.as<int32_t>(), d_carry, nullptr, (const int32_t *)d_carry_n};
    if (c->ws.desc_x && n_carry > 0) { /* the carry as operand rows, at the batch's frame stride */
        rc = grow(c, c->d_carry_x, (size_t)n_carry * kcap * SSK_X_ROW);
        if (rc != SS_OK) return rc;
        stage_timer t(c, "expand", (int64_t)n_carry * kcap * (32 + SSK_X_ROW));
        ssk_expand_desc_frames(c->stream, d_carry, kcap, n_carry, c->d_carry_x);
        tab.carry_x = c->d_carry_x;
    }
    ssk_match_call m = batch_call(c, th, ratio_num, ratio_den, d_idx, d_d1, d_d2);
    m.exclude_self_mode = 2;
    m.tab = &tab;
    return run_batch_match(c, m);
}

int ss_match_pairs_device(ss_ctx *c, const void *d_query, const void *d_n_query, const void *d_train, const void *d_n_train,
                          int n_frames, int rows_per_frame, int th, int ratio_num, int ratio_den, void *d_idx, void *d_d1,
                          void *d_d2)
{
    if (!c) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    if (n_frames < 0 || rows_per_frame < 1 || ratio_den <= 0 || ratio_num < 0) return fail(c, SS_ERR_INVALID_ARG, "bad match arguments");
    if (n_frames == 0) return SS_OK;
    if (!d_query || !d_n_query || !d_train || !d_n_train || !d_idx || !d_d1 || !d_d2) return fail(c, SS_ERR_INVALID_ARG, "NULL match buffer");
    ssk_match_call m; /* per-frame counts on both sides, frame b against frame b */
    m.n_frames = n_frames;
    m.nq_arr = (const int32_t *)d_n_query, m.nt_arr = (const int32_t *)d_n_train;
    m.th = th, m.rnum = ratio_num, m.rden = ratio_den;
    m.out_stride = rows_per_frame;
    m.idx = (int32_t *)d_idx, m.d1 = (uint16_t *)d_d1, m.d2 = (uint16_t *)d_d2;
    if (rows_per_frame >= SSK_MATCH_MFMA_MIN_QUERIES && !c->no_desc_x) {
        /* both sides expanded frame by frame ([n_frames][rows rounded up to 32][128 B]), then the batch matcher of the metric
         * path with per-frame counts on both sides */
        const int rows_alloc = (rows_per_frame + 31) & ~31;
        const size_t xb = (size_t)n_frames * rows_alloc * SSK_X_ROW;
        int rc = grow(c, c->d_qx, xb);
        if (rc == SS_OK) rc = grow(c, c->d_tx, xb);
        if (rc != SS_OK) return rc;
        {
            stage_timer t(c, "expand", (int64_t)2 * n_frames * rows_per_frame * (32 + SSK_X_ROW));
            ssk_expand_desc_frames(c->stream, d_query, rows_per_frame, n_frames, c->d_qx);
            ssk_expand_desc_frames(c->stream, d_train, rows_per_frame, n_frames, c->d_tx);
        }
        m.operand_rows = true;
        m.query = c->d_qx, m.train = c->d_tx;
        m.q_frame_stride = m.t_frame_stride = (int64_t)rows_alloc * SSK_X_ROW;
        m.query_p = (const uint8_t *)d_query, m.train_p = (const uint8_t *)d_train;
        m.qp_frame_stride = m.tp_frame_stride = (int64_t)rows_per_frame * SS_DESC_BYTES;
    } else {
        m.query = d_query, m.train = d_train;
        m.q_frame_stride = m.t_frame_stride = (int64_t)rows_per_frame * 8;
        m.nt_fixed = rows_per_frame;
    }
    return run_match(c, m, rows_per_frame, rows_per_frame, (int64_t)n_frames * rows_per_frame * (32 * 2 + 8));
}

/* the pose half of the frame branch: device match against the initial / previous frame's descriptors, then the host
 * geometry (csrc/ss_track.cpp).  d_desc: n rows of 32 bytes in device memory, written on c->stream or complete. */
static int track_step(ss_ctx *c, cam_track &ct, double timestamp, const uint8_t *d_desc, const uint8_t *d_desc_x, const ss_keypoint *kps,
                      int n, ss_pose *out, const int32_t *given_idx = nullptr, const uint16_t *given_d1 = nullptr, int flags = 0)
{
    /* d_desc_x: the same n rows already expanded (the extraction's desc_x), or NULL: expanded here when the matrix-core matcher
     * is going to read them (as the query now, or as the next frames' train set).
     * given_idx / given_d1 (ss_track_features_matched): this frame's matches against the frame of the PREVIOUS call, made by
     * the caller's batch matcher; used when that frame is the one the tracker is about to match against, and then nothing
     * is enqueued on the device for this frame. */
    const bool use_x = !c->no_desc_x && n > 0;
    const int camera_id = ct.camera_id;
    const int64_t serial = ++ct.serial;
    auto expanded = [&]() -> int {
        if (!use_x || d_desc_x) return SS_OK;
        int rcx = grow(c, c->d_qx, (size_t)SS_EXPANDED_BYTES(n));
        if (rcx != SS_OK) return rcx;
        stage_timer t(c, "expand", (int64_t)n * (32 + SSK_X_ROW));
        ssk_expand_desc(c->stream, d_desc, n, c->d_qx);
        d_desc_x = c->d_qx;
        return SS_OK;
    };
    sst_tracker &tr = ct.tracker;
    const ss_camera &cal = ct.has_cam ? ct.cam : c->cam; /* a camera never calibrated: the calibration set last */
    tr.cam = sst_camera{cal.fx, cal.fy, cal.cx, cal.cy, cal.k1, cal.k2, cal.p1, cal.p2};
    tr.scale_factor = c->params.scale_factor;
    c->h_xy.resize((size_t)2 * std::max(n, 1));
    c->h_oct.resize((size_t)std::max(n, 1));
    c->h_midx.assign((size_t)std::max(n, 1), -1);
    c->h_md1.assign((size_t)std::max(n, 1), 0xFFFF);
    for (int i = 0; i < n; i++) {
        c->h_xy[2 * i] = kps[i].x;
        c->h_xy[2 * i + 1] = kps[i].y;
        c->h_oct[i] = kps[i].octave;
    }
    int rc;
    const int want = tr.want_match();
    const auto tm0 = std::chrono::steady_clock::now();
    const int32_t *m_idx = c->h_midx.data();
    const uint16_t *m_d1 = c->h_md1.data();
    if (want != SST_MATCH_NONE && n > 0) {
        const int64_t train_serial = want == SST_MATCH_REF ? ct.ref_serial : ct.prev_serial;
        if (given_idx && given_d1 && train_serial == serial - 1 && tr.n_train() > 0) {
            m_idx = given_idx;
            m_d1 = given_d1;
        } else {
            /* the previous frame's descriptors may still be the caller's (SS_TRACK_DESC_STAYS_VALID): packed rows only */
            const bool prev_ext = want == SST_MATCH_PREV && ct.d_prev_ext != nullptr;
            const uint8_t *train = want == SST_MATCH_REF ? ct.d_ref_desc : prev_ext ? ct.d_prev_ext : ct.d_prev_desc;
            const uint8_t *train_x = want == SST_MATCH_REF ? ct.d_ref_desc_x : prev_ext ? nullptr : ct.d_prev_desc_x;
            rc = grow(c, c->d_mout, (size_t)n * 8);
            if (rc != SS_OK) return rc;
            const match_out o = split_scratch(c->d_mout, n);
            if (use_x && train_x && n >= SSK_MATCH_MFMA_MIN_QUERIES && tr.n_train() > 0) { /* both operands are expanded already */
                rc = expanded();
                if (rc == SS_OK) rc = match_expanded(c, d_desc_x, n, train_x, tr.n_train(), SS_TH_LOW, 9, 10, 0, o.idx, o.d1, o.d2, d_desc, train);
            } else {
                rc = ss_match_device(c, d_desc, n, train, tr.n_train(), SS_TH_LOW, 9, 10, 0, o.idx, o.d1, o.d2);
            }
            if (rc != SS_OK) return rc;
            HIP_TRY(c, hipMemcpyAsync(c->h_midx.data(), o.idx, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, hipMemcpyAsync(c->h_md1.data(), o.d1, (size_t)n * 2, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, hipStreamSynchronize(c->stream));
        }
    }
    sst_pose_out po;
    const auto tg0 = std::chrono::steady_clock::now();
    const int keep = tr.step(n, c->h_xy.data(), c->h_oct.data(), m_idx, m_d1, po);
    const auto tk0 = std::chrono::steady_clock::now();
    struct timing_guard {
        ss_ctx *c;
        std::chrono::steady_clock::time_point a, b, d;
        ~timing_guard()
        {
            if (!c->track_timing) return;
            const auto e = std::chrono::steady_clock::now();
            c->t_match += std::chrono::duration<double>(b - a).count();
            c->t_geom += std::chrono::duration<double>(d - b).count();
            c->t_keep += std::chrono::duration<double>(e - d).count();
            c->n_tracked++;
        }
    } tguard{c, tm0, tg0, tk0};
    /* the caller's rows of the previous frame are never read after this call: a frame kept as the previous one replaces
     * them, and every other outcome leaves the tracker without a previous frame to match against (it matches only in
     * state OK, which is entered through a frame kept as the previous one) */
    ct.d_prev_ext = nullptr;
    ct.prev_ext_n = 0;
    if (keep == SST_KEEP_AS_PREV) {
        ct.prev_serial = serial;
    } else if (keep == SST_KEEP_AS_REF) {
        ct.ref_serial = serial;
    }
    if (keep == SST_KEEP_AS_PREV && n > 0 && (flags & SS_TRACK_DESC_STAYS_VALID)) {
        ct.d_prev_ext = d_desc; /* the caller keeps the rows alive until the next call has returned: nothing to copy */
        ct.prev_ext_n = n;
    } else if (keep != SST_KEEP_NONE && n > 0) {
        dev_buf<uint8_t> &dst = keep == SST_KEEP_AS_REF ? ct.d_ref_desc : ct.d_prev_desc;
        rc = grow(c, dst, (size_t)n * SS_DESC_BYTES);
        if (rc != SS_OK) return rc;
        HIP_TRY(c, hipMemcpyAsync(dst, d_desc, (size_t)n * SS_DESC_BYTES, hipMemcpyDeviceToDevice, c->stream));
        if (use_x) {
            rc = expanded();
            if (rc != SS_OK) return rc;
            dev_buf<uint8_t> &dst_x = keep == SST_KEEP_AS_REF ? ct.d_ref_desc_x : ct.d_prev_desc_x;
            rc = grow(c, dst_x, (size_t)SS_EXPANDED_BYTES(n));
            if (rc != SS_OK) return rc;
            HIP_TRY(c, hipMemcpyAsync(dst_x, d_desc_x, (size_t)SS_EXPANDED_BYTES(n), hipMemcpyDeviceToDevice, c->stream));
        }
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    out->tracking_state = po.state;
    out->camera_id = camera_id;
    out->timestamp = timestamp;
    for (int k = 0; k < 3; k++) out->position[k] = po.pos[k];
    for (int k = 0; k < 4; k++) out->quaternion[k] = po.quat[k];
    out->n_keypoints = n;
    out->n_matches = po.n_matches;
    out->n_inliers = po.n_inliers;
    out->n_map_points = po.n_map_points;
    return SS_OK;
}

static int track_impl(ss_ctx *c, int camera_id, const uint8_t *pix, int width, int height, int channels, int row_stride, double timestamp,
                      ss_pose *out)
{
    if (!out) return SS_ERR_INVALID_ARG;
    if (!c->calibrated) return fail(c, SS_ERR_NOT_CALIBRATED, "Received frame before calibration. Ignoring.");
    /* a new camera is refused before any work when the context has no slot left, and gets its slot only once its frame has
     * been extracted (a frame that fails does not take one) */
    if (camera_id != 0 && !find_camera(c, camera_id) && c->n_cams == SS_MAX_CAMERAS) {
        cam_track *none = nullptr;
        return camera_slot(c, camera_id, &none);
    }
    ss_frame_result res;
    int rc = ss_extract(c, camera_id, pix, width, height, channels, row_stride, timestamp, &res);
    if (rc != SS_OK) return rc;
    cam_track *ct = nullptr;
    rc = camera_slot(c, camera_id, &ct);
    if (rc != SS_OK) return rc;
    /* this frame's descriptors are still in HBM (frame 0 of the batch arrays) */
    return track_step(c, *ct, timestamp, c->ws.desc, c->ws.desc_x, res.keypoints, res.n_keypoints, out);
}

/* the body of ss_track_features_matched, and of ss_track_features (`who`) with no matches and no flags */
static int track_features_impl(ss_ctx *c, const char *who, int camera_id, double timestamp, const void *d_descriptors, const ss_keypoint *keypoints,
                               int n_keypoints, const int32_t *match_idx, const uint16_t *match_d1, int flags, ss_pose *out)
{
    const std::string name = who;
    if (!out || n_keypoints < 0) return SS_ERR_INVALID_ARG;
    if (!c->calibrated) return fail(c, SS_ERR_NOT_CALIBRATED, "Received frame before calibration. Ignoring.");
    if (camera_id == 0) return fail(c, SS_ERR_BAD_FRAME, "Frame message missing camera identifier.");
    if (n_keypoints > 0 && (!d_descriptors || !keypoints)) return fail(c, SS_ERR_INVALID_ARG, name + ": NULL feature arrays");
    if ((match_idx == nullptr) != (match_d1 == nullptr)) return fail(c, SS_ERR_INVALID_ARG, name + ": match_idx and match_d1 go together");
    if (flags & ~SS_TRACK_DESC_STAYS_VALID) return fail(c, SS_ERR_INVALID_ARG, name + ": unknown flag");
    cam_track *ct = nullptr;
    const int rc = camera_slot(c, camera_id, &ct);
    if (rc != SS_OK) return rc;
    return track_step(c, *ct, timestamp, (const uint8_t *)d_descriptors, nullptr, keypoints, n_keypoints, out, match_idx, match_d1, flags);
}

/* SS_TRACK_DESC_STAYS_VALID: the rows a camera refers to are valid until the next pose-step call on the context has
 * returned, whatever its outcome.  Every pose-step entry point therefore copies the rows of the other cameras first, and
 * those of its own camera when it fails (a call that reaches the tracker drops or replaces them, track_step). */
extern "C++" template <typename F> static int pose_call(ss_ctx *c, int camera_id, F &&body)
{
    if (!c) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    for (int i = 0; i < c->n_cams; i++)
        if (c->cams[i].camera_id != camera_id) {
            const int rcd = detach_rows(c, c->cams[i]);
            if (rcd != SS_OK) return rcd;
        }
    const int rc = body();
    if (rc != SS_OK)
        if (cam_track *own = find_camera(c, camera_id)) {
            const std::string why = c->err; /* the call's own error is what the caller sees */
            (void)detach_rows(c, *own);
            c->err = why;
        }
    return rc;
}

int ss_track(ss_ctx *c, int camera_id, const uint8_t *pix, int width, int height, int channels, int row_stride,
             double timestamp, ss_pose *out)
{
    return pose_call(c, camera_id, [&]() { return track_impl(c, camera_id, pix, width, height, channels, row_stride, timestamp, out); });
}

int ss_track_features(ss_ctx *c, int camera_id, double timestamp, const void *d_descriptors, const ss_keypoint *keypoints,
                      int n_keypoints, ss_pose *out)
{
    return pose_call(c, camera_id, [&]() {
        return track_features_impl(c, "ss_track_features", camera_id, timestamp, d_descriptors, keypoints, n_keypoints, nullptr, nullptr, 0, out);
    });
}

int ss_track_features_matched(ss_ctx *c, int camera_id, double timestamp, const void *d_descriptors, const ss_keypoint *keypoints,
                              int n_keypoints, const int32_t *match_idx, const uint16_t *match_d1, int flags, ss_pose *out)
{
    return pose_call(c, camera_id, [&]() {
        return track_features_impl(c, "ss_track_features_matched", camera_id, timestamp, d_descriptors, keypoints, n_keypoints, match_idx, match_d1, flags, out);
    });
}
int ss_expand_descriptors_device(ss_ctx *c, const void *d_packed, int n, void *d_expanded)
{
    if (!c) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    if (n < 0) return fail(c, SS_ERR_INVALID_ARG, "bad descriptor count");
    if (n == 0) return SS_OK;
    if (!d_packed || !d_expanded) return fail(c, SS_ERR_INVALID_ARG, "NULL descriptor buffer");
    stage_timer t(c, "expand", (int64_t)n * (32 + SSK_X_ROW));
    ssk_expand_desc(c->stream, d_packed, n, d_expanded);
    HIP_TRY(c, hipGetLastError());
    return SS_OK;
}

int ss_match_expanded_device(ss_ctx *c, const void *d_query_x, int n_query, const void *d_train_x, int n_train, int th, int ratio_num,
                             int ratio_den, int exclude_self, void *d_idx, void *d_d1, void *d_d2)
{
    return match_expanded(c, d_query_x, n_query, d_train_x, n_train, th, ratio_num, ratio_den, exclude_self, d_idx, d_d1, d_d2, nullptr, nullptr);
}

static int partial_common(ss_ctx *c, bool expanded, const void *d_query, int n_query, const void *d_train, int n_train,
                          int64_t row_offset, void *d_part)
{
    if (!c) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    if (n_query < 0 || n_train < 0 || row_offset < 0 || row_offset + n_train > 0x7FFFFFFFll)
        return fail(c, SS_ERR_INVALID_ARG, "ss_match_partial_device: rows must fit 31 bits");
    if (n_query == 0) return SS_OK;
    if (!d_query || !d_part || (!d_train && n_train > 0)) return fail(c, SS_ERR_INVALID_ARG, "NULL match buffer");
    int rc = grow(c, c->d_part_tmp, (size_t)n_query * 8);
    if (rc != SS_OK) return rc;
    const match_out o = split_scratch(c->d_part_tmp, n_query);
    rc = expanded ? ss_match_expanded_device(c, d_query, n_query, d_train, n_train, -1, 1, 1, 0, o.idx, o.d1, o.d2)
                  : ss_match_device(c, d_query, n_query, d_train, n_train, -1, 1, 1, 0, o.idx, o.d1, o.d2);
    if (rc != SS_OK) return rc;
    ssk_pack_partial(c->stream, o.idx, o.d1, o.d2, n_query, (int32_t)row_offset, d_part);
    HIP_TRY(c, hipGetLastError());
    return SS_OK;
}

int ss_match_partial_expanded_device(ss_ctx *c, const void *d_query_x, int n_query, const void *d_train_x, int n_train,
                                     int64_t row_offset, void *d_part)
{
    return partial_common(c, true, d_query_x, n_query, d_train_x, n_train, row_offset, d_part);
}

int ss_match_partial_device(ss_ctx *c, const void *d_query, int n_query, const void *d_train, int n_train, int64_t row_offset,
                            void *d_part)
{
    return partial_common(c, false, d_query, n_query, d_train, n_train, row_offset, d_part);
}

int ss_match_fold_device(ss_ctx *c, const void *d_parts, int n_parts, int n_query, int th, int ratio_num, int ratio_den,
                         void *d_idx, void *d_d1, void *d_d2)
{
    if (!c) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    if (n_parts < 1 || n_query < 0 || ratio_den <= 0 || ratio_num < 0) return fail(c, SS_ERR_INVALID_ARG, "bad fold arguments");
    if (n_query == 0) return SS_OK;
    if (!d_parts || !d_idx || !d_d1 || !d_d2) return fail(c, SS_ERR_INVALID_ARG, "NULL fold buffer");
    stage_timer t(c, "match_fold", (int64_t)n_parts * n_query * 8 + (int64_t)n_query * 8);
    ssk_match_fold(c->stream, d_parts, n_parts, n_query, th, ratio_num, ratio_den, (int32_t *)d_idx, (uint16_t *)d_d1, (uint16_t *)d_d2);
    HIP_TRY(c, hipGetLastError());
    return SS_OK;
}

int ss_match_fold_strided_device(ss_ctx *c, const void *d_parts, int n_parts, int64_t part_stride_bytes, int n_query, int th,
                                 int ratio_num, int ratio_den, void *d_idx, void *d_d1, void *d_d2)
{
    if (!c) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    if (n_parts < 1 || n_query < 0 || ratio_den <= 0 || ratio_num < 0 || part_stride_bytes % 8 != 0 || part_stride_bytes < (int64_t)n_query * 8)
        return fail(c, SS_ERR_INVALID_ARG, "bad fold arguments");
    if (n_query == 0) return SS_OK;
    if (!d_parts || !d_idx || !d_d1 || !d_d2) return fail(c, SS_ERR_INVALID_ARG, "NULL fold buffer");
    stage_timer t(c, "match_fold", (int64_t)n_parts * n_query * 8 + (int64_t)n_query * 8);
    ssk_match_fold_strided(c->stream, d_parts, part_stride_bytes, n_parts, n_query, th, ratio_num, ratio_den, (int32_t *)d_idx, (uint16_t *)d_d1,
                           (uint16_t *)d_d2);
    HIP_TRY(c, hipGetLastError());
    return SS_OK;
}

int ss_stereo_exchange_match(ss_ctx *c, ss_xchg *x, int peer_rank, int th, int ratio_num, int ratio_den, int32_t *idx, uint16_t *d1,
                             uint16_t *d2, int32_t *n_own, int32_t *n_peer)
{
    if (!c || !x) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    if (!c->have_geom || c->last_n_frames <= 0) return fail(c, SS_ERR_STATE, "ss_stereo_exchange_match: no frame has been extracted");
    if (peer_rank < 0) return fail(c, SS_ERR_INVALID_ARG, "ss_stereo_exchange_match: bad peer rank");
    const int kcap = c->hg.kcap;
    const int64_t blk = (int64_t)kcap * SS_DESC_BYTES;
    const void *segs[2] = {c->ws.desc, c->ws.n_kp};
    const int64_t sizes[2] = {blk, (int64_t)sizeof(int32_t)};
    const void *gathered = nullptr;
    int64_t stride = 0;
    int rc = ss_xchg_allgather(x, c, segs, sizes, 2, &gathered, &stride);
    if (rc != SS_OK) return fail(c, rc, std::string("ss_stereo_exchange_match: ") + ss_xchg_last_error(x));
    rc = grow(c, c->d_mout, (size_t)kcap * 8);
    if (rc != SS_OK) return rc;
    const uint8_t *peer = (const uint8_t *)gathered + (int64_t)peer_rank * stride;
    const match_out o = split_scratch(c->d_mout, kcap);
    rc = ss_match_pairs_device(c, c->ws.desc, c->ws.n_kp, peer, peer + blk, 1, kcap, th, ratio_num, ratio_den, o.idx, o.d1, o.d2);
    if (rc != SS_OK) return rc;
    int32_t counts[2] = {0, 0};
    HIP_TRY(c, hipMemcpyAsync(&counts[0], c->ws.n_kp, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(&counts[1], peer + blk, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    if (idx) HIP_TRY(c, hipMemcpyAsync(idx, o.idx, (size_t)kcap * 4, hipMemcpyDeviceToHost, c->stream));
    if (d1) HIP_TRY(c, hipMemcpyAsync(d1, o.d1, (size_t)kcap * 2, hipMemcpyDeviceToHost, c->stream));
    if (d2) HIP_TRY(c, hipMemcpyAsync(d2, o.d2, (size_t)kcap * 2, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    rc = ss_xchg_status(x);
    if (rc != SS_OK) return fail(c, rc, std::string("ss_stereo_exchange_match: ") + ss_xchg_last_error(x));
    if (n_own) *n_own = counts[0];
    if (n_peer) *n_peer = counts[1];
    return SS_OK;
}

static int stereo_check_params(ss_ctx *c, const ss_stereo_params *p)
{
    if (!p) return fail(c, SS_ERR_INVALID_ARG, "stereo: params is NULL");
    if (!std::isfinite(p->fx) || !std::isfinite(p->baseline) || !std::isfinite(p->th_depth))
        return fail(c, SS_ERR_INVALID_ARG, "stereo: fx, baseline and th_depth must be finite");
    if (!(p->fx > 0.0f)) return fail(c, SS_ERR_INVALID_ARG, "stereo: fx must be > 0");
    if (!(p->baseline > 0.0f)) return fail(c, SS_ERR_INVALID_ARG, "stereo: baseline must be > 0 (a monocular calibration has no depth)");
    return SS_OK;
}

int ss_stereo_batch_device(ss_ctx *c, const ss_stereo_params *p, void *d_points, void *d_summary)
{
    if (!c) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    if (!c->have_geom || c->last_n_frames <= 0) return fail(c, SS_ERR_STATE, "ss_stereo_batch_device: no batch has been extracted");
    int rc = stereo_check_params(c, p);
    if (rc != SS_OK) return rc;
    if (!d_points || !d_summary) return fail(c, SS_ERR_INVALID_ARG, "ss_stereo_batch_device: NULL output buffer");
    if (c->last_n_frames % 2 != 0)
        return fail(c, SS_ERR_INVALID_ARG, "ss_stereo_batch_device: the last batch has " + std::to_string(c->last_n_frames) +
                                               " frames; stereo pairs are frames (2p, 2p + 1) of an even batch");
    const ss_geom &g = c->hg;
    const int n_pairs = c->last_n_frames / 2;
    /* ComputeStereoMatches' constants, one single-precision operation each: mbf, mb = mbf / fx, minD = 0, maxD = mbf / minZ
     * with minZ = mb; Tracking's mThDepth = mbf * ThDepth / fx */
    ssk_stereo_call st;
    st.bf = p->baseline * p->fx;
    const float mb = st.bf / p->fx;
    st.min_d = 0.0f, st.max_d = st.bf / mb;
    const float bt = st.bf * p->th_depth;
    st.close_depth = bt / p->fx;
    st.points = d_points, st.summary = d_summary;
    rc = flagged_frame_error(c, c->stereo_test_flagged, &st.frame_error);
    if (rc != SS_OK) return rc;
    const int64_t nf = g.n_features;
    {
        /* both eyes' keypoints, the left descriptors, ~1 % of the right ones per left keypoint (one row here), the points */
        stage_timer t(c, "stereo_search", (int64_t)n_pairs * (2 * nf * (int64_t)sizeof(ss_keypoint) + 2 * nf * SS_DESC_BYTES + (int64_t)g.kcap * 16));
        ssk_stereo_search(c->stream, c->ws, g, c->last_n_frames, st);
    }
    {
        /* per left keypoint: 11 rows of 11 (left) and 21 (right) pixels, its keypoint, the point read and written */
        stage_timer t(c, "stereo_refine", (int64_t)n_pairs * nf * (11 * (11 + 21) + (int64_t)sizeof(ss_keypoint) + 4 + 2 * 16));
        ssk_stereo_refine(c->stream, c->ws, g, c->last_n_frames, c->last_lvl0, st);
    }
    {
        /* three passes over the points (the second and third mostly hit), one write of the cut ones, the summary */
        stage_timer t(c, "stereo_cut", (int64_t)n_pairs * (nf * 16 * 2 + 32));
        ssk_stereo_cut(c->stream, c->ws, g, c->last_n_frames, st);
    }
    HIP_TRY(c, hipGetLastError());
    return SS_OK;
}

/* frames 0 / 1 of the batch just extracted are one pair: its stereo points, then both eyes' features, the points and the summary
 * to the host (c->d_stereo holds kcap points and the summary); synchronises */
static int stereo_pair_results(ss_ctx *c, const ss_stereo_params &sp, int camera_id, double timestamp, ss_frame_result *out_left,
                               ss_frame_result *out_right, const ss_stereo_point **points, ss_stereo_summary *summary)
{
    uint8_t *d_sum = c->d_stereo + (size_t)c->hg.kcap * sizeof(ss_stereo_point);
    int rc = ss_stereo_batch_device(c, &sp, c->d_stereo, d_sum);
    if (rc != SS_OK) return rc;
    int32_t nk[2] = {0, 0};
    HIP_TRY(c, hipMemcpyAsync(nk, c->ws.n_kp, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(out_left->level_counts, c->ws.level_counts, SS_MAX_LEVELS * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(out_right->level_counts, c->ws.level_counts + SS_MAX_LEVELS, SS_MAX_LEVELS * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(summary, d_sum, sizeof(ss_stereo_summary), hipMemcpyDeviceToHost, c->stream));
    rc = check_frame_errors(c); /* synchronises */
    if (rc != SS_OK) return rc;
    rc = fetch_rows(c, 0, nk[0], c->h_kps, c->h_desc, camera_id, timestamp, out_left);
    if (rc != SS_OK) return rc;
    c->h_stereo.resize((size_t)std::max(nk[0], 1));
    if (nk[0] > 0)
        HIP_TRY(c, hipMemcpyAsync(c->h_stereo.data(), c->d_stereo, (size_t)nk[0] * sizeof(ss_stereo_point), hipMemcpyDeviceToHost, c->stream));
    rc = fetch_rows(c, 1, nk[1], c->h_kps_r, c->h_desc_r, camera_id, timestamp, out_right);
    if (rc != SS_OK) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    *points = c->h_stereo.data();
    return SS_OK;
}

int ss_extract_stereo(ss_ctx *c, int camera_id, const uint8_t *left, const uint8_t *right, int width, int height, int channels,
                      int row_stride, double timestamp, ss_frame_result *out_left, ss_frame_result *out_right,
                      const ss_stereo_point **points, ss_stereo_summary *summary)
{
    if (!c || !out_left || !out_right || !points || !summary) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    if (camera_id == 0) return fail(c, SS_ERR_BAD_FRAME, "Frame message missing camera identifier.");
    /* each eye is a single image here: that the context holds both is checked below, in this entry point's words */
    int rc = check_image_args(c, left && right, 1, width, height, channels, row_stride, (int64_t)row_stride * height, false,
                              "Frame message missing binary image data.", "row_stride smaller than a row");
    if (rc != SS_OK) return rc;
    const cam_track *own = find_camera(c, camera_id);
    if (!own || !own->has_cam)
        return fail(c, SS_ERR_NOT_CALIBRATED, "ss_extract_stereo: camera " + std::to_string(camera_id) + " has no calibration (fx, baseline, th_depth)");
    if (c->params.max_batch < 2) return fail(c, SS_ERR_INVALID_ARG, "ss_extract_stereo: the context needs max_batch >= 2 (both eyes are one batch)");
    ss_stereo_params sp;
    sp.fx = (float)own->cam.fx;
    sp.baseline = (float)own->cam.baseline;
    sp.th_depth = (float)own->cam.th_depth;
    rc = stereo_check_params(c, &sp);
    if (rc == SS_OK) rc = ensure_geometry(c, width, height);
    if (rc != SS_OK) return rc;
    const ss_geom &g = c->hg;
    const upload_size up = upload_footprint(width, height, channels, row_stride);
    rc = grow(c, c->d_in, 2 * up.alloc);
    if (rc == SS_OK) rc = grow(c, c->d_stereo, (size_t)g.kcap * sizeof(ss_stereo_point) + sizeof(ss_stereo_summary));
    if (rc != SS_OK) return rc;
    HIP_TRY(c, hipMemcpyAsync(c->d_in, left, up.bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->d_in + up.alloc, right, up.bytes, hipMemcpyHostToDevice, c->stream));
    rc = run_extract(c, c->d_in, 2, channels, row_stride, (int64_t)up.alloc, own->cam.rgb != 0);
    if (rc != SS_OK) return rc;
    return stereo_pair_results(c, sp, camera_id, timestamp, out_left, out_right, points, summary);
}

/* ---- rectification (csrc/ss_rectify.hip) ---- */
int ss_rectify_build_map(const ss_rectify_model *m, float *map_x, float *map_y)
{
    if (!m || !map_x || !map_y || m->width <= 0 || m->height <= 0 || m->width > 32767 || m->height > 32767) return SS_ERR_INVALID_ARG;
    /* A = K' * R, ir = A^-1 by the adjugate; every step one double operation (-ffp-contract=off) */
    const double kn[3][3] = {{m->fx_new, 0.0, m->cx_new}, {0.0, m->fy_new, m->cy_new}, {0.0, 0.0, 1.0}};
    double a[3][3];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) a[i][j] = kn[i][0] * m->R[j] + kn[i][1] * m->R[3 + j] + kn[i][2] * m->R[6 + j];
    const double det = a[0][0] * (a[1][1] * a[2][2] - a[1][2] * a[2][1]) - a[0][1] * (a[1][0] * a[2][2] - a[1][2] * a[2][0]) +
                       a[0][2] * (a[1][0] * a[2][1] - a[1][1] * a[2][0]);
    if (det == 0.0 || !std::isfinite(det)) return SS_ERR_INVALID_ARG;
    const double d = 1.0 / det;
    const double ir[9] = {(a[1][1] * a[2][2] - a[1][2] * a[2][1]) * d, (a[0][2] * a[2][1] - a[0][1] * a[2][2]) * d,
                          (a[0][1] * a[1][2] - a[0][2] * a[1][1]) * d, (a[1][2] * a[2][0] - a[1][0] * a[2][2]) * d,
                          (a[0][0] * a[2][2] - a[0][2] * a[2][0]) * d, (a[0][2] * a[1][0] - a[0][0] * a[1][2]) * d,
                          (a[1][0] * a[2][1] - a[1][1] * a[2][0]) * d, (a[0][1] * a[2][0] - a[0][0] * a[2][1]) * d,
                          (a[0][0] * a[1][1] - a[0][1] * a[1][0]) * d};
    const double k1 = m->k1, k2 = m->k2, p1 = m->p1, p2 = m->p2, k3 = m->k3;
    for (int i = 0; i < m->height; i++) {
        double _x = i * ir[1] + ir[2], _y = i * ir[4] + ir[5], _w = i * ir[7] + ir[8];
        float *mx = map_x + (size_t)i * m->width, *my = map_y + (size_t)i * m->width;
        for (int j = 0; j < m->width; j++, _x += ir[0], _y += ir[3], _w += ir[6]) {
            const double w = 1.0 / _w, x = _x * w, y = _y * w;
            const double x2 = x * x, y2 = y * y, r2 = x2 + y2, _2xy = 2.0 * x * y;
            const double kr = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2;
            const double xd = x * kr + p1 * _2xy + p2 * (r2 + 2.0 * x2);
            const double yd = y * kr + p1 * (r2 + 2.0 * y2) + p2 * _2xy;
            mx[j] = (float)(m->fx * xd + m->cx);
            my[j] = (float)(m->fy * yd + m->cy);
        }
    }
    return SS_OK;
}

int ss_rectify_set_map(ss_ctx *c, int map_id, const float *map_x, const float *map_y, int width, int height)
{
    if (!c) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    if (map_id < 0 || map_id >= SS_MAX_RECTIFY_MAPS)
        return fail(c, SS_ERR_INVALID_ARG, "ss_rectify_set_map: map_id " + std::to_string(map_id) + " is outside 0 .. " + std::to_string(SS_MAX_RECTIFY_MAPS - 1));
    ss_ctx::rect_map &rm = c->rect_maps[map_id];
    if (!map_x && !map_y && width == 0) { /* drop it, once the remaps that read it have run */
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        dev_free(rm.d);
        rm.w = rm.h = 0;
        return SS_OK;
    }
    if (!map_x || !map_y || width <= 0 || height <= 0 || width > 32767 || height > 32767)
        return fail(c, SS_ERR_INVALID_ARG, "ss_rectify_set_map: two maps of 1 .. 32767 columns and rows are needed (NULL, NULL, width 0 drops the map)");
    const int pitch = ssk_rectify_pitch(width);
    const size_t n = (size_t)pitch * height;
    std::vector<uint32_t> host((n * SSK_RECTIFY_ENTRY_BYTES + 3) / 4); /* xy [n] uint32, then ab [n] uint16 */
    ssk_rectify_fixed(map_x, map_y, width, height, pitch, host.data(), (uint16_t *)(host.data() + n));
    uint8_t *d = nullptr;
    HIP_TRY(c, hipMalloc((void **)&d, n * SSK_RECTIFY_ENTRY_BYTES));
    hipError_t e = hipMemcpy(d, host.data(), n * SSK_RECTIFY_ENTRY_BYTES, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream); /* the map this one replaces may still be read */
    if (e != hipSuccess) {
        dev_free(d);
        return fail(c, SS_ERR_HIP, std::string("ss_rectify_set_map: ") + hipGetErrorString(e));
    }
    dev_free(rm.d);
    rm.d = d, rm.w = width, rm.h = height;
    return SS_OK;
}

/* the checks and the launch of ss_rectify_batch_device; `who` names the entry point in the messages */
static int rectify_run(ss_ctx *c, const std::string &who, const void *d_src, int n, int w, int h, int channels, int64_t row_stride,
                       int64_t frame_stride, const int32_t *map_ids, void *d_dst, int64_t dst_row_stride, int64_t dst_frame_stride)
{
    int rc = check_image_args(c, d_src && d_dst && map_ids, n, w, h, channels, row_stride, frame_stride, false,
                              "rectify: NULL source, destination or map table, or an empty batch", "rectify: source strides smaller than the frame");
    if (rc != SS_OK) return rc;
    const int64_t row_bytes = (int64_t)w * channels, max_stride = (int64_t)1 << 40;
    if (w > 32767 || h > 32767) return fail(c, SS_ERR_INVALID_ARG, who + ": frames larger than 32767 columns or rows");
    if (dst_row_stride < row_bytes || dst_frame_stride < dst_row_stride * h || dst_row_stride > max_stride || dst_frame_stride > max_stride)
        return fail(c, SS_ERR_INVALID_ARG, who + ": destination strides smaller than the frame (or beyond 2^40)");
    if (row_stride > max_stride || frame_stride > max_stride) return fail(c, SS_ERR_INVALID_ARG, who + ": source strides beyond 2^40");
    const int64_t src_span = (h - 1) * row_stride + row_bytes, dst_span = (h - 1) * dst_row_stride + row_bytes;
    if (src_span > (int64_t)UINT32_MAX) return fail(c, SS_ERR_INVALID_ARG, who + ": the rows of a source frame span 4 GiB or more");
    const uintptr_t s0 = (uintptr_t)d_src, s1 = s0 + (uintptr_t)((n - 1) * frame_stride + src_span);
    const uintptr_t d0 = (uintptr_t)d_dst, d1 = d0 + (uintptr_t)((n - 1) * dst_frame_stride + dst_span);
    if (s0 < d1 && d0 < s1) return fail(c, SS_ERR_INVALID_ARG, who + ": source and destination overlap (the remap is not in place)");
    for (int b = 0; b < n; b++) {
        const int id = map_ids[b];
        if (id < 0 || id >= SS_MAX_RECTIFY_MAPS)
            return fail(c, SS_ERR_INVALID_ARG, who + ": map_ids[" + std::to_string(b) + "] = " + std::to_string(id) + " is outside 0 .. " +
                                                   std::to_string(SS_MAX_RECTIFY_MAPS - 1));
        const ss_ctx::rect_map &rm = c->rect_maps[id];
        if (!rm.d) return fail(c, SS_ERR_INVALID_ARG, who + ": map " + std::to_string(id) + " has not been set");
        if (rm.w != w || rm.h != h)
            return fail(c, SS_ERR_INVALID_ARG, who + ": map " + std::to_string(id) + " is " + std::to_string(rm.w) + " x " + std::to_string(rm.h) +
                                                   ", the frames are " + std::to_string(w) + " x " + std::to_string(h));
    }
    /* the frame table grouped by map: a workgroup keeps its tile of ONE map in registers over all the frames that use it */
    std::vector<int32_t> order;
    order.reserve((size_t)n);
    ssk_rectify_group groups[SS_MAX_RECTIFY_MAPS];
    int n_groups = 0;
    const size_t n_entries = (size_t)ssk_rectify_pitch(w) * h;
    for (int id = 0; id < SS_MAX_RECTIFY_MAPS; id++) {
        const int first = (int)order.size();
        for (int b = 0; b < n; b++)
            if (map_ids[b] == id) order.push_back(b);
        if ((int)order.size() == first) continue;
        ssk_rectify_group &g = groups[n_groups++];
        g.xy = (const uint32_t *)c->rect_maps[id].d;
        g.ab = (const uint16_t *)(c->rect_maps[id].d + n_entries * 4);
        g.first = first, g.count = (int)order.size() - first;
    }
    rc = upload_train_src(c, order.data(), n); /* the staged host -> device table of the batch calls */
    if (rc != SS_OK) return rc;
    {
        stage_timer t(c, "rectify", (int64_t)n * w * h * channels * 2 + (int64_t)n_groups * w * h * SSK_RECTIFY_ENTRY_BYTES);
        ssk_rectify(c->stream, groups, n_groups, c->train_src.as<int32_t>(), d_src, channels, row_stride, frame_stride, d_dst, dst_row_stride,
                    dst_frame_stride, w, h);
    }
    HIP_TRY(c, hipGetLastError());
    return SS_OK;
}

int ss_rectify_batch_device(ss_ctx *c, const void *d_src, int n_frames, int width, int height, int channels, int64_t row_stride,
                            int64_t frame_stride, const int32_t *map_ids, void *d_dst, int64_t dst_row_stride, int64_t dst_frame_stride)
{
    if (!c) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    return rectify_run(c, "ss_rectify_batch_device", d_src, n_frames, width, height, channels, row_stride, frame_stride, map_ids, d_dst,
                       dst_row_stride, dst_frame_stride);
}

int ss_extract_stereo_raw(ss_ctx *c, int camera_id, const uint8_t *left, const uint8_t *right, int width, int height, int channels,
                          int row_stride, double timestamp, int map_left, int map_right, const ss_stereo_params *sp,
                          ss_frame_result *out_left, ss_frame_result *out_right, const ss_stereo_point **points, ss_stereo_summary *summary)
{
    if (!c || !out_left || !out_right || !points || !summary) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    if (camera_id == 0) return fail(c, SS_ERR_BAD_FRAME, "Frame message missing camera identifier.");
    int rc = check_image_args(c, left && right, 1, width, height, channels, row_stride, (int64_t)row_stride * height, true,
                              "Frame message missing binary image data.", "row_stride smaller than a row");
    if (rc != SS_OK) return rc;
    if (c->params.max_batch < 2) return fail(c, SS_ERR_INVALID_ARG, "ss_extract_stereo_raw: the context needs max_batch >= 2 (both eyes are one batch)");
    rc = stereo_check_params(c, sp);
    if (rc != SS_OK) return rc;
    const ss_stereo_params params = *sp;
    /* both eyes raw in d_in, remapped into d_rect with rows and frames 16 bytes aligned: a gray pair is level 0 in place */
    const upload_size up = upload_footprint(width, height, channels, row_stride);
    const int64_t rect_row = ((int64_t)width * channels + 15) & ~(int64_t)15, rect_frame = rect_row * height;
    rc = grow(c, c->d_in, 2 * up.alloc);
    if (rc == SS_OK) rc = grow(c, c->d_rect, (size_t)(2 * rect_frame));
    if (rc != SS_OK) return rc;
    HIP_TRY(c, hipMemcpyAsync(c->d_in, left, up.bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->d_in + up.alloc, right, up.bytes, hipMemcpyHostToDevice, c->stream));
    const int32_t ids[2] = {map_left, map_right};
    rc = rectify_run(c, "ss_extract_stereo_raw", c->d_in, 2, width, height, channels, row_stride, (int64_t)up.alloc, ids, c->d_rect, rect_row,
                     rect_frame);
    if (rc == SS_OK) rc = ensure_geometry(c, width, height);
    if (rc == SS_OK) rc = grow(c, c->d_stereo, (size_t)c->hg.kcap * sizeof(ss_stereo_point) + sizeof(ss_stereo_summary));
    if (rc != SS_OK) return rc;
    const cam_track *own = find_camera(c, camera_id);
    rc = run_extract(c, c->d_rect, 2, channels, rect_row, rect_frame, own && own->has_cam ? (own->cam.rgb != 0) : -1);
    if (rc != SS_OK) return rc;
    return stereo_pair_results(c, params, camera_id, timestamp, out_left, out_right, points, summary);
}

int ss_wait_stream(ss_ctx *c, void *hip_stream)
{
    if (!c) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    hipEvent_t e = nullptr;
    HIP_TRY(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    hipError_t r = hipEventRecord(e, (hipStream_t)hip_stream);
    if (r == hipSuccess) r = hipStreamWaitEvent(c->stream, e, 0);
    (void)hipEventDestroy(e); /* destruction is deferred until the event has completed */
    if (r != hipSuccess) return fail(c, SS_ERR_HIP, std::string("ss_wait_stream: ") + hipGetErrorString(r));
    return SS_OK;
}

int ss_track_reset(ss_ctx *c)
{
    if (!c) return SS_ERR_INVALID_ARG;
    /* every camera back to NO_IMAGES_YET; a camera without a calibration of its own gives its slot back */
    int kept = 0;
    for (int i = 0; i < c->n_cams; i++) {
        c->cams[i].reset();
        if (c->cams[i].has_cam) {
            if (kept != i) std::swap(c->cams[kept], c->cams[i]);
            kept++;
        }
    }
    for (int i = kept; i < c->n_cams; i++) {
        cam_track &ct = c->cams[i];
        ct.free_rows();
        ct = cam_track();
    }
    c->n_cams = kept;
    return SS_OK;
}

int ss_track_detach(ss_ctx *c)
{
    if (!c) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    for (int i = 0; i < c->n_cams; i++) {
        const int rc = detach_rows(c, c->cams[i]);
        if (rc != SS_OK) return rc;
    }
    return SS_OK;
}

int ss_synchronize(ss_ctx *c)
{
    if (!c) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    if (c->have_geom && c->last_n_frames > 0) return check_frame_errors(c);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SS_OK;
}

int ss_get_stream(ss_ctx *c, void **hip_stream)
{
    if (!c || !hip_stream) return SS_ERR_INVALID_ARG;
    *hip_stream = (void *)c->stream;
    return SS_OK;
}

int ss_profile_enable(ss_ctx *c, int on)
{
    if (!c) return SS_ERR_INVALID_ARG;
    c->profile = on != 0;
    return SS_OK;
}

int ss_profile_reset(ss_ctx *c)
{
    if (!c) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    collect_events(c);
    for (auto &s : c->stages) s.ms.clear();
    return SS_OK;
}

int ss_stats(ss_ctx *c, ss_stage_stats *out, int max_stages)
{
    if (!c || (!out && max_stages > 0)) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    collect_events(c);
    int n = 0;
    for (auto &s : c->stages) {
        if (n < max_stages) {
            ss_stage_stats &o = out[n];
            memset(&o, 0, sizeof(o));
            snprintf(o.name, sizeof(o.name), "%s", s.name.c_str());
            o.launches = (int64_t)s.ms.size();
            o.algorithmic_bytes = s.bytes;
            if (!s.ms.empty()) {
                std::vector<float> v = s.ms;
                std::sort(v.begin(), v.end());
                double tot = 0;
                for (float x : v) tot += x;
                o.total_ms = tot;
                o.mean_ms = tot / v.size();
                o.median_ms = v[v.size() / 2]; /* the shim's median rule, :661 */
            }
        }
        n++;
    }
    return n;
}

int ss_debug_fetch(ss_ctx *c, int what, int frame, int level, void *dst, int64_t dst_bytes)
{
    if (!c || !dst) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    if (!c->have_geom || frame < 0 || frame >= c->last_n_frames || level < 0 || level >= c->hg.n_levels)
        return fail(c, SS_ERR_INVALID_ARG, "ss_debug_fetch: no such frame / level");
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const ss_geom &g = c->hg;
    const ss_level &L = g.lv[level];
    if (what >= 0 && what <= 2) {
        if (what == 2 && !c->ws.score) {
            /* the response map is not kept in normal operation: allocate it and run the FAST kernel
             * again on the pyramid of the last batch (same kernel, same outputs, plus the map);
             * from now on this context keeps it */
            const int rc = ws_alloc(c, WS_FIRST_USE);
            if (rc != SS_OK) return rc;
            ssk_fast_blur_nms(c->stream, c->ws, g, c->last_n_frames, c->last_lvl0);
            HIP_TRY(c, hipStreamSynchronize(c->stream));
        }
        const uint8_t *base = what == 0 ? c->ws.pyr : what == 1 ? c->ws.blur : c->ws.score;
        const int64_t need = (int64_t)L.w * L.h;
        if (dst_bytes < need) return fail(c, SS_ERR_INVALID_ARG, "ss_debug_fetch: dst too small");
        if (what == 0 && level == 0 && c->last_lvl0.ptr) { /* level 0 was read in place from the caller's buffer */
            HIP_TRY(c, hipMemcpy2D(dst, (size_t)L.w, c->last_lvl0.ptr + (int64_t)frame * c->last_lvl0.frame_stride,
                                   (size_t)c->last_lvl0.pitch, (size_t)L.w, (size_t)L.h, hipMemcpyDeviceToHost));
            return (int)need;
        }
        HIP_TRY(c, hipMemcpy2D(dst, (size_t)L.w, base + (size_t)frame * g.block_bytes + L.off, (size_t)L.pitch,
                               (size_t)L.w, (size_t)L.h, hipMemcpyDeviceToHost));
        return (int)need;
    }
    if (what == 3 || what == 4) {
        ss_level_state st;
        HIP_TRY(c, hipMemcpy(&st, c->ws.state + (size_t)frame * SS_MAX_LEVELS + level, sizeof(st), hipMemcpyDeviceToHost));
        const int n = what == 3 ? st.n_cand : st.n_sel;
        if (dst_bytes < (int64_t)n * 12) return fail(c, SS_ERR_INVALID_ARG, "ss_debug_fetch: dst too small");
        std::vector<uint32_t> packed((size_t)std::max(n, 1));
        const uint32_t *src = what == 3 ? c->ws.cand + (size_t)frame * g.cand_total + L.cand_base
                                        : c->ws.sel + (size_t)frame * g.sel_total + L.sel_base;
        if (n > 0) HIP_TRY(c, hipMemcpy(packed.data(), src, (size_t)n * 4, hipMemcpyDeviceToHost));
        int32_t *o = (int32_t *)dst;
        for (int i = 0; i < n; i++) {
            o[3 * i] = SS_PX(packed[i]);
            o[3 * i + 1] = SS_PY(packed[i]);
            o[3 * i + 2] = SS_PR(packed[i]);
        }
        return n * 12;
    }
    if (what == 5) { /* which kernel built this level of the last batch, and where its level 0 lives */
        if (dst_bytes < 8) return fail(c, SS_ERR_INVALID_ARG, "ss_debug_fetch: dst too small");
        ((int32_t *)dst)[0] = level == 0 ? 0 : c->resize_kernel[level];
        ((int32_t *)dst)[1] = c->last_lvl0.ptr != nullptr;
        return 8;
    }
    return fail(c, SS_ERR_INVALID_ARG, "ss_debug_fetch: unknown selector");
}

} /* extern "C" */

extern "C" int ss_debug_sort(ss_ctx *c, uint64_t *items, int n)
{
    if (!c || (!items && n > 0)) return SS_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    if (n == 0) return SS_OK;
    int rc = grow(c, c->d_mq, (size_t)n * 8);
    if (rc != SS_OK) return rc;
    HIP_TRY(c, hipMemcpyAsync(c->d_mq, items, (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
    if (ssk_debug_sort(c->stream, (uint64_t *)c->d_mq.p, n) != 0) return fail(c, SS_ERR_INVALID_ARG, "ss_debug_sort: n > 2048");
    HIP_TRY(c, hipMemcpyAsync(items, c->d_mq, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SS_OK;
}
