/*
 * sendslam_orb.h -- C ABI of libsendslam_orb.so: the MI355X-native ORB tracking front-end
 * that replaces SEND-SLAM's dockerised ORB-SLAM3 CPU backend for ONE path: per-frame ORB
 * extraction (pyramid, FAST-9 + NMS, quadtree distribution, orientation, rBRIEF) and
 * brute-force Hamming matching with a ratio test.
 *
 * Plain C linkage, plain pointers and sizes, int status (0 = ok, < 0 = ss_status), no
 * exception crosses.  What each entry point replaces in the reference
 * (/root/reference/slam_backends/orb_slam_3/orbslam3_mono_networked.cc unless noted):
 *
 *   ss_create / ss_destroy     make_unique<ORB_SLAM3::System>(voc, yaml, MONOCULAR, false) :511,
 *                              Shutdown :654; ORB parameters = the YAML literals :193-206
 *   ss_set_calibration         the "calibration" message branch :477-519 with the 16 scalars of
 *                              CameraCalibration :59-77 / ParseCameraCalibration :109-137
 *   ss_extract                 the "frame" branch :521-627 up to and inside TrackMonocular :594
 *                              (ORBextractor::operator()), pixels as cv::imdecode leaves them :546
 *   ss_extract_batch_device    same, for a batch of frames already resident in HBM (cameras /
 *                              frame batches shard one per GPU; no counterpart in the reference,
 *                              which handles one camera on one thread :594)
 *   ss_pipe_*                  the same frame branch :521-627 for a STREAM of host frames: pinned ring,
 *                              H2D copy / kernels / D2H copy of different batches overlapped, results in
 *                              host memory -- what the copy at :325 + imdecode :546 + TrackMonocular :594
 *                              do one frame at a time; host half slam_handler.ex:59-88
 *   ss_track_features[_matched] the pose half of TrackMonocular :594 for a frame whose features a pipe
 *                              extracted (front door read-ahead of queued frames)
 *   ss_match_partial_device /  the local and the cross-shard half of a query against a database
 *   ss_match_fold_device       partitioned over GPUs
 *   ss_xchg_*                  the exchange step of configs 4 / 5 (all-gather, broadcast) as direct peer writes; no
 *                              counterpart in the reference (one TCP link :387-388)
 *   ss_match*                  ORBmatcher::DescriptorDistance + best/second-best search inside
 *                              TrackMonocular :594 (all-pairs rule: SURVEY.md Appendix A.6)
 *   ss_track                   TrackMonocular :594 -> Twc, tracking state :596 (bounded monocular
 *                              front-end; the pose SendPosePacket :225-282 ships)
 *   ss_stereo_batch_device /   ORB_SLAM3::Frame::ComputeStereoMatches (the stereo Frame constructor; no counterpart in the
 *   ss_extract_stereo          monocular shim, which only ships th_depth / baseline :59-77)
 *   ss_rectify_* /             cv::initUndistortRectifyMap + cv::remap(INTER_LINEAR) of upstream's stereo examples, which run on every
 *   ss_extract_stereo_raw      frame of both eyes before the extractor (no counterpart in the monocular shim)
 *   ss_match_guided*           ORBmatcher::SearchForInitialization / SearchByProjection on Frame::GetFeaturesInArea (window
 *                              search, conflicts, rotation histogram; the monocular shim reaches them inside TrackMonocular :594)
 *   ss_vocab_* / ss_bow_* /    the ORBvoc.txt argument of the System constructor :511 (DBoW2 TemplatedVocabulary::loadFromTextFile),
 *   ss_match_bow_*             Frame::ComputeBoW, ORBmatcher::SearchByBoW (TrackReferenceKeyFrame, relocalisation) and
 *                              L1Scoring::score (KeyFrameDatabase) inside TrackMonocular :594
 *   ss_proj_* / ss_match_proj* Tracking::SearchLocalPoints: Frame::isInFrustum, MapPoint::PredictScale and
 *                              ORBmatcher::SearchByProjection(Frame&, vector<MapPoint*>&, th) inside TrackMonocular :594
 *   ss_fuse_* / ss_match_fuse* ORBmatcher::Fuse (LocalMapping::SearchInNeighbors), its Sim3 form (LoopClosing::SearchAndFuse) and
 *                              the Sim3 SearchByProjection of the loop and merge candidate check
 *   ss_sim3_opt_* /            the rest of ORBmatcher::SearchBySim3 (the skip marks of its two projection searches and their
 *   ss_sim3_marks_* /          agreement test) and Optimizer::OptimizeSim3 of LoopClosing::DetectCommonRegionsFromBoW, starting from
 *   ss_sim3_mutual_*           the result ss_sim3_* left in device memory
 *   ss_pnp_*                   MLPnPsolver's RANSAC of Tracking::Relocalization: a pose from the 2D-3D matches of SearchByBoW against
 *                              each relocalisation candidate, with no prior
 *   ss_refresh_*               MapPoint::UpdateNormalAndDepth, MapPoint::ComputeDistinctiveDescriptors and MapPoint::Observations()
 *                              over the map ss_covis_set_map_rows keeps: after a fusion, a bundle adjustment or a loop correction
 *   ss_place_*                 KeyFrameDatabase: add / erase, DetectLoopCandidates, DetectNBestCandidates and
 *                              DetectRelocalizationCandidates over an inverted file kept on the device
 *   ss_undistort_* /           the keypoint post-processing of Frame's constructor: UndistortKeyPoints (mvKeysUn; k1 k2 p1 p2 of the
 *   ss_proj_view_set_bounds /  calibration message :125-128), ComputeImageBounds and ComputeStereoFromRGBD (the first reader of
 *   ss_depth_*                 depth_map_factor), so that every family above that takes undistorted keypoints gets them on the device
 *   ss_stats                   vTimesTrack median/mean summary :615-616, :656-664
 *   ss_last_error              the cerr diagnostics of the shim (:457-469, :523-551)
 *
 * Threading: a context is single-threaded (one HIP stream, one camera or one batch in
 * flight); distinct contexts are independent and may live on different devices.  A call
 * that fails leaves the context usable (the shim's log-and-skip policy, :523-551).
 * Every entry point takes longer than 1 ms on first use: NIF callers flag them dirty
 * (INTEGRATION.md).
 *
 * The library has NO CPU fallback: without a usable HIP device ss_create fails with
 * SS_ERR_NO_DEVICE.
 */
#ifndef SENDSLAM_ORB_H
#define SENDSLAM_ORB_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SS_ABI_VERSION 5
#define SS_MAX_LEVELS 16
#define SS_MAX_CAMERAS 8 /* cameras one context tracks (ss_track*), each with its own state */
#define SS_DESC_BYTES 32

typedef enum {
    SS_OK = 0,
    SS_ERR_INVALID_ARG = -1,
    SS_ERR_NO_DEVICE = -2,
    SS_ERR_HIP = -3,
    SS_ERR_TOO_SMALL = -4,      /* image too small for the cell grid at some level */
    SS_ERR_OVERFLOW = -5,       /* an internal capacity was exceeded; nothing was truncated */
    SS_ERR_NOT_CALIBRATED = -6, /* frame before calibration (shim :523-527) */
    SS_ERR_BAD_FRAME = -7,
    SS_ERR_NO_MEMORY = -8,
    SS_ERR_STATE = -9,
    SS_ERR_BUSY = -10 /* ss_pipe_acquire: every slot of the ring is in flight or not yet released */
} ss_status;

typedef struct ss_ctx ss_ctx;

/* ORB parameters.  Defaults are the reference's YAML literals (:193-206): 1250 features,
 * scale 1.2, 8 levels, FAST 20 / 7; lapping area {0, 1000} is ORB-SLAM3's monocular
 * Frame constructor (ExtractORB(0, im, 0, 1000)). */
typedef struct {
    int32_t n_features;
    float scale_factor;
    int32_t n_levels;
    int32_t ini_th_fast;
    int32_t min_th_fast;
    int32_t lapping_x0;
    int32_t lapping_x1;
    int32_t max_batch; /* frames per ss_extract_batch_device call; >= 1 */
    /* How the rotated rBRIEF tap coordinates cvRound(x*b + y*a), cvRound(x*a - y*b) of computeOrbDescriptor are
     * evaluated.  0 (default): as written, every product and the sum rounded.  1: the first product fused into the
     * sum, fma(x, b, y*a) / fma(x, a, -(y*b)) -- what GCC's FMA contraction makes of the expression when upstream is
     * built -O3 -march=native (slam_backends/orb_slam_3/CMakeLists.txt:10-13) on an FMA-capable host.  Which one the
     * reference binary runs is unpinned (tests/golden/ref_dump/README.md); a few descriptor bits per frame depend on it. */
    int32_t steer_fma;
} ss_orb_params;

/* The 16 calibration scalars of the wire protocol (shim :59-77; produced by
 * send_slam/lib/send_slam/slam_handler.ex:209-226). */
typedef struct {
    char type[16]; /* "PinHole" */
    double fx, fy, cx, cy;
    double k1, k2, p1, p2;
    int32_t width, height;
    double fps;
    int32_t rgb; /* Camera.RGB: 1 = byte 0 of a 3-channel pixel is treated as R */
    double th_depth, baseline, depth_map_factor;
} ss_camera;

/* cv::KeyPoint fields the extractor fills */
typedef struct {
    float x, y;     /* level-0 pixel coordinates */
    float size;     /* (int)(31 * scale^octave) */
    float angle;    /* degrees [0, 360) */
    float response; /* FAST score */
    int32_t octave;
} ss_keypoint;

/* Result of ss_extract: host arrays owned by the context, valid until the next call on it */
typedef struct {
    int32_t n_keypoints;
    int32_t camera_id;
    double timestamp;
    const ss_keypoint *keypoints; /* n_keypoints */
    const uint8_t *descriptors;   /* n_keypoints x 32, row-major (CV_8U N x 32) */
    int32_t level_counts[SS_MAX_LEVELS];
} ss_frame_result;

/* Device-resident results of the last ss_extract_batch_device call */
typedef struct {
    int32_t n_frames;
    int32_t kp_capacity;           /* rows per frame in the two arrays below */
    const ss_keypoint *keypoints;  /* device: [n_frames][kp_capacity] */
    const uint8_t *descriptors;    /* device: [n_frames][kp_capacity][32] */
    const int32_t *n_keypoints;    /* device: [n_frames] */
    const int32_t *level_counts;   /* device: [n_frames][SS_MAX_LEVELS] */
    const int32_t *frame_error;    /* device: [n_frames]; 0 or the ss_status of a frame whose capacity was exceeded */
} ss_batch_view;

typedef struct {
    char name[32];
    int64_t launches;
    double total_ms;  /* HIP-event time on the context's stream */
    double mean_ms;   /* per launch */
    double median_ms; /* per launch */
    int64_t algorithmic_bytes; /* per launch of the last shape run */
} ss_stage_stats;

int ss_abi_version(void);
int ss_orb_params_default(ss_orb_params *p);

int ss_create(int device_ordinal, const ss_orb_params *params, ss_ctx **out);
int ss_destroy(ss_ctx *ctx);
/* ctx may be NULL: returns the message of the last failed ss_create on this thread */
const char *ss_last_error(const ss_ctx *ctx);

int ss_set_calibration(ss_ctx *ctx, int camera_id, const ss_camera *cam);

/* Host pixels in, host keypoints/descriptors out; synchronous.  channels 1 (gray), 3 or 4
 * (converted with the calibration's rgb flag, exactly as GrabImageMonocular does);
 * camera_id must be non-zero (shim :528); caller keeps ownership of pix. */
int ss_extract(ss_ctx *ctx, int camera_id, const uint8_t *pix, int width, int height,
               int channels, int row_stride, double timestamp, ss_frame_result *out);

/* n_frames <= max_batch frames already in device memory (row_stride / frame_stride in
 * bytes).  Asynchronous on the context's stream; results stay on the device. */
int ss_extract_batch_device(ss_ctx *ctx, const void *d_pix, int n_frames, int width,
                            int height, int channels, int64_t row_stride,
                            int64_t frame_stride);
int ss_get_batch_view(ss_ctx *ctx, ss_batch_view *out);
/* Copies frame `frame` of the last batch to the context's host arrays (same ownership
 * rule as ss_extract); synchronises the context's stream. */
int ss_fetch_frame(ss_ctx *ctx, int frame, ss_frame_result *out);

/* K7.  idx[i] = index of the accepted best train descriptor or -1; d1/d2 = best and
 * second-best distance (0xFFFF when absent).  Accept iff d1 <= th and d1*ratio_den <
 * d2*ratio_num.  exclude_self skips j == i.  Ties: lowest index.  th < 0 = raw mode: no
 * acceptance test, idx = best index (or -1 when there is no train row): what a shard of a
 * partitioned database reports before the cross-shard merge. */
int ss_match(ss_ctx *ctx, const uint8_t *query, int n_query, const uint8_t *train,
             int n_train, int th, int ratio_num, int ratio_den, int exclude_self,
             int32_t *idx, uint16_t *d1, uint16_t *d2);
/* same with device pointers, asynchronous on the context's stream */
int ss_match_device(ss_ctx *ctx, const void *d_query, int n_query, const void *d_train,
                    int n_train, int th, int ratio_num, int ratio_den, int exclude_self,
                    void *d_idx, void *d_d1, void *d_d2);
/* Matches every frame of the last batch: mode 0 = self-match (exclude j == i), mode 1 =
 * frame b against frame b-1 (frame 0 against itself, excluding j == i).  Outputs are
 * device arrays [n_frames][kp_capacity]; rows >= n_keypoints[b] are idx -1. */
int ss_match_batch_device(ss_ctx *ctx, int mode, int th, int ratio_num, int ratio_den,
                          void *d_idx, void *d_d1, void *d_d2);
/* Matches every frame of the last batch against a train frame named per frame by a table (the table form of
 * ss_match_batch_device, e.g. each frame against the previous frame of its own camera).  train_src is a HOST array
 * [n_frames]; for query frame b, t = train_src[b]:
 *   t >= 0   frame t of the batch (0 <= t < n_frames, earlier or later); the pair j == i is excluded iff t == b;
 *   t == -1  no train: rows < n_keypoints[b] get idx -1 and d1 = d2 = 0xFFFF;
 *   t <= -2  carry frame c = -2 - t (0 <= c < n_carry): d_carry is a device array [n_carry][kp_capacity][32] of packed
 *            descriptors (kp_capacity of ss_get_batch_view) and d_carry_n a device int32 [n_carry] of their row counts
 *            (<= kp_capacity); no self-exclusion.
 * Any other value is SS_ERR_INVALID_ARG.  d_carry / d_carry_n may be NULL when n_carry == 0.  th / ratio and the outputs
 * are those of ss_match_batch_device.  Asynchronous on the context's stream; the table is copied before the call returns,
 * the carry is read by the device (on the matrix-core path it is first expanded into a context buffer). */
int ss_match_batch_sources_device(ss_ctx *ctx, const int32_t *train_src, const void *d_carry, const void *d_carry_n,
                                  int n_carry, int th, int ratio_num, int ratio_den, void *d_idx, void *d_d1,
                                  void *d_d2);

/* n_frames independent (query frame, train frame) pairs in one launch, e.g. the frames of this GPU's eye against the
 * all-gathered frames of the peer eye.  Both sides are device arrays
 * [n_frames][rows_per_frame][32] with per-frame row counts d_n_query / d_n_train (device int32 [n_frames]); outputs
 * are [n_frames][rows_per_frame], rows >= n_query[b] get idx -1 / 0xFFFF.  No self-exclusion. */
int ss_match_pairs_device(ss_ctx *ctx, const void *d_query, const void *d_n_query, const void *d_train,
                          const void *d_n_train, int n_frames, int rows_per_frame, int th, int ratio_num,
                          int ratio_den, void *d_idx, void *d_d1, void *d_d2);

/* Pose of one frame (shim :225-282 SendPosePacket: position + quaternion x y z w of Twc, shipped
 * only in tracking state OK :596).  tracking_state uses ORB_SLAM3::Tracking::eTrackingState values:
 * 0 NO_IMAGES_YET, 1 NOT_INITIALIZED, 2 OK, 4 LOST. */
typedef struct {
    int32_t tracking_state;
    int32_t camera_id;
    double timestamp;
    double position[3];
    double quaternion[4]; /* x y z w */
    int32_t n_keypoints;
    int32_t n_matches;    /* one-to-one matches to the reference / previous frame */
    int32_t n_inliers;    /* triangulated (initialisation) or pose-optimisation inliers */
    int32_t n_map_points; /* keypoints of this frame that carry a 3-D point */
} ss_pose;

/* The whole "frame" branch :521-627 = TrackMonocular :594 for a bounded monocular front-end:
 * ss_extract, device match against the initial / previous frame's descriptors (th 50, ratio
 * 0.9), then host double-precision geometry (csrc/ss_track.h: two-view initialisation, pose-only
 * optimisation, triangulation).  Requires ss_set_calibration (fx fy cx cy k1 k2 p1 p2 are used).
 * No keyframes, local mapping or loop closing.  Relocalisation: the link exists (ss_pnp_*, below);
 * ss_track itself still re-initialises a lost tracker from the next frame. */
int ss_track(ss_ctx *ctx, int camera_id, const uint8_t *pix, int width, int height, int channels,
             int row_stride, double timestamp, ss_pose *out);
/* Several cameras on one context: every camera id gets its own tracker state (reference, previous frame, motion model)
 * and descriptor buffers, up to SS_MAX_CAMERAS ids in the order they first appear; a further id is SS_ERR_INVALID_ARG.
 * ss_set_calibration(camera_id) gives that camera its own calibration (intrinsics, distortion, and for ss_track the
 * RGB order of colour frames) and resets that camera only; a camera that was never sent a calibration uses the
 * calibration set last.  An id takes its slot with its calibration or its first successful pose-step call (a frame
 * that fails extraction takes none).  One camera's frames must arrive in order; frames of different cameras may
 * interleave.  Batch extraction (ss_extract_batch_device, ss_pipe) has no camera ids: its colour frames use the RGB
 * order of the calibration set last, so the cameras of one pipe share one RGB order.
 * ss_track_reset: every camera back to NO_IMAGES_YET (System::Reset / the "terminate" message :462-469); cameras
 * without a calibration of their own give their slots back. */
int ss_track_reset(ss_ctx *ctx);

/* The matrix-core matcher reads descriptors as rows of 256 FP4 values (one per bit, +1 / -1: 128 bytes).  The frames of a
 * batch get that form from the extraction itself; a database that is matched against again and again (loop closure,
 * relocalisation: SURVEY.md section 8(e) config 5) is expanded ONCE: n descriptors of 32 B at d_packed -> rows of 128 B
 * at d_expanded, which must hold n rounded up to a multiple of 32 rows (SS_EXPANDED_BYTES(n)).  ss_match_expanded_device
 * is ss_match_device on two expanded operands (same rule, same outputs, any sizes); ss_match_partial_expanded_device is
 * ss_match_partial_device on them. */
#define SS_EXPANDED_ROW_BYTES 128
#define SS_EXPANDED_BYTES(n) ((((int64_t)(n) + 31) & ~(int64_t)31) * SS_EXPANDED_ROW_BYTES)
int ss_expand_descriptors_device(ss_ctx *ctx, const void *d_packed, int n, void *d_expanded);
int ss_match_expanded_device(ss_ctx *ctx, const void *d_query_x, int n_query, const void *d_train_x, int n_train, int th,
                             int ratio_num, int ratio_den, int exclude_self, void *d_idx, void *d_d1, void *d_d2);
int ss_match_partial_expanded_device(ss_ctx *ctx, const void *d_query_x, int n_query, const void *d_train_x, int n_train,
                                     int64_t row_offset, void *d_part);

/* Pose step alone (ss_track without its ss_extract): the frame's descriptors are n rows of 32 bytes in DEVICE memory
 * (e.g. ss_pipe_result.d_descriptors of a completed slot), its keypoints are host memory.  Same state machine, same
 * match (th 50, ratio 0.9) and geometry as ss_track; frames must arrive in camera order. */
int ss_track_features(ss_ctx *ctx, int camera_id, double timestamp, const void *d_descriptors,
                      const ss_keypoint *keypoints, int n_keypoints, ss_pose *out);

/* ss_track_features for a caller that has matched the frames of a batch against each other already (ss_pipe match_mode 1,
 * ss_match_batch_device mode 1, with th 50 and ratio 9 / 10 -- the pose step's own rule): match_idx / match_d1 are host
 * arrays of n_keypoints entries, this frame's matches against the frame of the PREVIOUS pose-step call FOR THE SAME CAMERA
 * on this context that returned SS_OK (NULL, NULL: none -- also the thing to pass after a call that failed).  They are used when that
 * frame is the one the tracker is about to match against (tracking, or the frame right after a new reference); in every
 * other case the tracker runs its own device match, as ss_track_features does, so the poses are the same either way.  flags: SS_TRACK_DESC_STAYS_VALID = d_descriptors stays valid and unchanged
 * until the next pose-step call on this context has returned (the rows of a pipe slot that is released after its last
 * frame): the tracker then refers to them instead of copying them, and never reads them after that next call has
 * returned (it copies them first where it still needs them, see ss_track_detach).  With both, a tracked frame costs
 * no device work. */
#define SS_TRACK_DESC_STAYS_VALID 1
int ss_track_features_matched(ss_ctx *ctx, int camera_id, double timestamp, const void *d_descriptors,
                              const ss_keypoint *keypoints, int n_keypoints, const int32_t *match_idx,
                              const uint16_t *match_d1, int flags, ss_pose *out);
/* The rows a camera's tracker refers to under SS_TRACK_DESC_STAYS_VALID are copied into the context ("detached") by the
 * next pose-step call for ANOTHER camera (before it returns), dropped by the next call for the SAME camera (which either
 * replaces them or leaves the camera without a previous frame), and copied by ss_track_detach for every camera at once: call it
 * before the memory of those rows is reused or freed (e.g. before releasing a pipe slot whose frames were tracked, even
 * when its last frames were skipped), after which the caller owes nothing.  Poses do not depend on where the rows live. */
int ss_track_detach(ss_ctx *ctx);

/* ---- a database partitioned over GPUs ------------------------------------
 * A shard reports, per query descriptor, ss_match_part = (best distance, second-best distance, GLOBAL row of the
 * best or -1): 8 bytes, the unit every rank all-gathers.  ss_match_partial_device runs the raw local match of
 * n_query device descriptors against this shard's n_train rows (global row = row_offset + local row) and writes
 * d_part[n_query].  ss_match_fold_device folds n_parts such arrays laid out [part][n_query], parts in ASCENDING
 * row order, with the rule the match kernels use across their train chunks (ties keep the lower row; second best =
 * min over the losers' best and everyone's second best), then applies the acceptance test of ss_match.  One
 * launch; asynchronous on the context's stream. */
typedef struct {
    uint16_t d1, d2; /* 0xFFFF = none */
    int32_t row;     /* global row of the best, -1 = none */
} ss_match_part;
int ss_match_partial_device(ss_ctx *ctx, const void *d_query, int n_query, const void *d_train, int n_train,
                            int64_t row_offset, void *d_part);
int ss_match_fold_device(ss_ctx *ctx, const void *d_parts, int n_parts, int n_query, int th, int ratio_num,
                         int ratio_den, void *d_idx, void *d_d1, void *d_d2);
/* same, part p at d_parts + p * part_stride_bytes (a multiple of 8, >= n_query * 8): the layout ss_xchg_allgather leaves */
int ss_match_fold_strided_device(ss_ctx *ctx, const void *d_parts, int n_parts, int64_t part_stride_bytes, int n_query, int th,
                                 int ratio_num, int ratio_den, void *d_idx, void *d_d1, void *d_d2);

/* ---- the exchange step of configs 4 and 5 without PyTorch / RCCL ---------------------------------
 * One process per GPU.  ss_xchg_create is collective: every rank calls it with the same world, max_bytes and rendezvous
 * (the path of a Unix-domain socket rank 0 listens on while the hipIpc handles of the ranks' slabs are swapped); every rank
 * then has every peer's slab mapped -- different GPUs of one node (xGMI) or the same GPU.  A message is ONE hop: each rank
 * stores its block straight into every peer's slab and raises a flag there (csrc/ss_xchg.hip).
 *
 * ss_xchg_allgather: every rank contributes the same number of bytes, as up to 4 device segments laid back to back (each
 * padded to 16 bytes); on return *d_gathered points at [world][*rank_stride] bytes of LOCAL device memory, rank r's
 * block at r * *rank_stride, valid until the second-next message of this exchange.  ss_xchg_broadcast: d_buf of `root` ->
 * d_buf of everybody (in place, like ncclBroadcast).  Both are asynchronous on ctx's stream: enqueue the consumers on the same
 * stream.  Every rank must issue the same sequence of messages.  timeout_ms bounds the rendezvous of ss_xchg_create (0 = 10 s);
 * a message waits at most min(timeout_ms, 10 s).  A peer that does not show up within that limit ends
 * the waiting kernel (it never hangs the GPU) and poisons the exchange: ss_xchg_status / the next call return SS_ERR_STATE.
 * ss_xchg_destroy is collective too (a last flag-only message, so that nobody unmaps memory a peer still writes).
 * The reference has nothing here: one camera, one TCP link (orbslam3_mono_networked.cc:387-388, application.ex:80). */
typedef struct ss_xchg ss_xchg;
int ss_xchg_create(int device_ordinal, int rank, int world, int64_t max_bytes, const char *rendezvous, int timeout_ms,
                   ss_xchg **out);
int ss_xchg_destroy(ss_xchg *x);
/* x may be NULL: message of the last failed ss_xchg_create on this thread */
const char *ss_xchg_last_error(const ss_xchg *x);
int ss_xchg_status(ss_xchg *x);
int ss_xchg_allgather(ss_xchg *x, ss_ctx *ctx, const void *const *d_segments, const int64_t *segment_bytes, int n_segments,
                      const void **d_gathered, int64_t *rank_stride);
int ss_xchg_broadcast(ss_xchg *x, ss_ctx *ctx, int root, void *d_buf, int64_t bytes);
/* Config 4 in one call, for hosts that hold no device memory of their own (the TCP front door with SENDSLAM_SHARD=r/2, the NIF):
 * all-gathers the descriptor block and keypoint count of the frame ctx extracted last (ss_extract / ss_track; frame 0 of a
 * batch) with the peer rank's, matches this eye's descriptors against the peer eye's (th, ratio as in ss_match) and copies
 * idx / d1 / d2 (kp_capacity entries each; any of them may be NULL) to the host.  Both ranks call it once per stereo pair, in
 * lockstep.  *n_own / *n_peer: the two keypoint counts.  Synchronous. */
int ss_stereo_exchange_match(ss_ctx *ctx, ss_xchg *x, int peer_rank, int th, int ratio_num, int ratio_den, int32_t *idx,
                             uint16_t *d1, uint16_t *d2, int32_t *n_own, int32_t *n_peer);

/* ---- stereo depth of rectified pairs (ORB-SLAM3 Frame::ComputeStereoMatches, which the stereo Frame constructor runs right
 * after the two extractions; the reference's shim is monocular, :511 / :594, and ships th_depth / baseline with every
 * calibration, :59-77, without a reader) -----------------------------------------------------------------------------
 * Frames 2p (left) and 2p + 1 (right) of the last batch are pair p.  Per left keypoint: Hamming search over the right
 * keypoints whose row band (+-2 * scale^octave) holds its row, octave +-1, u inside [uL - bf / mb, uL], best < 75; then an
 * 11 x 11 SAD window slid -5 .. +5 px over the right eye's unblurred pyramid at the left keypoint's octave, a parabola fit
 * for the sub-pixel right coordinate, depth = bf / disparity; per pair, points whose SAD is >= 1.5 * 1.4 * the median SAD
 * lose their depth again.  Ties: lowest right index, lowest shift.  Two deviations from upstream: a SAD window that would
 * leave the level image rejects the point (upstream would read outside it), and a pair without an accepted point is left
 * alone (upstream indexes an empty vector).  Input is assumed rectified: distortion coefficients are ignored, as upstream
 * ignores them here (it uses mvKeys); ss_rectify_* below make such a pair from raw frames.  Upstream's stereo constructor extracts both eyes with lapping area {0, 0}: that is
 * the stereo setting of ss_orb_params; the outputs are indexed by left keypoint row, so any lapping works. */
typedef struct {
    float fx, baseline, th_depth; /* Camera.fx, Stereo.b (metres; bf = baseline * fx), Stereo.ThDepth */
} ss_stereo_params;
typedef struct {          /* 16 bytes, one per LEFT keypoint row */
    float u_right;        /* mvuRight: -1 = none */
    float depth;          /* mvDepth:  -1 = none */
    int32_t right_idx;    /* the search's best right keypoint if its distance is < 75, else -1; kept when refinement or the median cut reject */
    uint16_t orb_dist;    /* that distance, 0xFFFF when right_idx < 0 */
    uint16_t sad;         /* best SAD once the 11 sums were formed (kept when later tests or the median cut reject), else 0xFFFF */
} ss_stereo_point;
typedef struct {          /* 32 bytes, one per pair */
    int32_t status;       /* SS_OK, or the ss_status that voided the pair (frame_error of an eye; all its points are "none") */
    int32_t n_left, n_right;
    int32_t n_matched;    /* right_idx >= 0 */
    int32_t n_refined;    /* points with a depth before the median cut */
    int32_t n_depth;      /* depth > 0 after it */
    int32_t n_close;      /* 0 < depth < (bf * th_depth) / fx  (Tracking's mThDepth) */
    int32_t sad_median;   /* -1 when no point was refined */
} ss_stereo_summary;
/* Pairs (2p, 2p + 1) of the last ss_extract_batch_device batch; n_frames must be even (else SS_ERR_INVALID_ARG).
 * d_points: device [n_frames / 2][kp_capacity] ss_stereo_point (rows >= n_left are "none"), d_summary: device [n_frames / 2]
 * ss_stereo_summary.  fx <= 0, baseline <= 0 or a non-finite value: SS_ERR_INVALID_ARG.  Asynchronous on the context's
 * stream; a batch whose level 0 was read in place needs the caller's pixel buffer untouched until this has run. */
int ss_stereo_batch_device(ss_ctx *ctx, const ss_stereo_params *p, void *d_points, void *d_summary);
/* Host pixels of one rectified pair in, both eyes' features and the left eye's stereo points (n_keypoints of out_left
 * entries) out; synchronous.  fx / baseline / th_depth are those of camera_id's own calibration (SS_ERR_NOT_CALIBRATED
 * without one, SS_ERR_INVALID_ARG for baseline <= 0 or a context created with max_batch < 2); pixels as in ss_extract.
 * The result arrays are owned by the context until the next call on it. */
int ss_extract_stereo(ss_ctx *ctx, int camera_id, const uint8_t *left, const uint8_t *right, int width, int height,
                      int channels, int row_stride, double timestamp, ss_frame_result *out_left,
                      ss_frame_result *out_right, const ss_stereo_point **points, ss_stereo_summary *summary);

/* ---- rectification of raw stereo pairs (upstream ORB-SLAM3's stereo examples: cv::initUndistortRectifyMap once per eye, then
 * cv::remap(raw, rect, M1, M2, INTER_LINEAR) on every frame of both eyes before the extractor sees a pixel; neither OpenCV file,
 * imgwarp.cpp / undistort.dispatch.cpp, is in the reference tree: the rule below is this library's own restatement from OpenCV
 * 4.x as recalled, parity with a real OpenCV build unpinned like the rest of the path; tests/rectify_ref.py is the normative
 * statement, reproduced bit for bit) -------------------------------------------------------------------
 * Map builder (double precision, every step one IEEE operation): A = K' * R (each entry summed k = 0, 1, 2 left to right),
 *   ir = A^-1 by the 3 x 3 adjugate (det == 0 or not finite: SS_ERR_INVALID_ARG).  Row i starts at _x = i * ir[1] + ir[2],
 *   _y = i * ir[4] + ir[5], _w = i * ir[7] + ir[8]; column j uses them and then adds ir[0], ir[3], ir[6] (the running sum is
 *   upstream's form, not j * ir[0] + ...).  Per pixel: w = 1 / _w, x = _x * w, y = _y * w, x2 = x * x, y2 = y * y, r2 = x2 + y2,
 *   _2xy = 2 * x * y, kr = 1 + ((k3 * r2 + k2) * r2 + k1) * r2, xd = x * kr + p1 * _2xy + p2 * (r2 + 2 * x2),
 *   yd = y * kr + p1 * (r2 + 2 * y2) + p2 * _2xy, map_x = (float)(fx * xd + cx), map_y = (float)(fy * yd + cy).  The rational
 *   denominator (k4 .. k6), the thin-prism and the tilt terms are not modelled; fisheye models are not either: such callers
 *   hand their own float maps to ss_rectify_set_map.
 * Fixed point, per float32 map value v: t = v * 32.0f; s = (int32)rintf(t), half to even, when t is finite and
 *   -2^31 <= t < 2^31, else INT32_MIN (cvRound on x86-64; the pixel then lies outside every image);
 *   i = clamp(s >> 5, -32768, 32767) (arithmetic shift), f = s & 31.  (ix, a) come from map_x, (iy, b) from map_y.
 * Remap (same size and channel count on both sides, every channel the same weights, constant border 0):
 *   S(y, x) = src[y][x] inside the image, else 0;
 *   acc = S(iy, ix) * (32 - a)(32 - b) * 32 + S(iy, ix + 1) * a(32 - b) * 32 + S(iy + 1, ix) * (32 - a) * b * 32
 *       + S(iy + 1, ix + 1) * a * b * 32;  out = (acc + 16384) >> 15.
 *   The weights sum to 32768, so out <= 255 without a clamp.  OpenCV's table of shorts saturates the entry a = b = 0 to 32767
 *   and moves the missing 1 to another tap; for 8-bit pixels the rounded byte is the same.
 * Widths and heights up to 32767 are accepted, so a saturated i is always outside the image.  R and K' are the caller's
 * stereoRectify output (R1 / R2 and the left 3 x 3 block of P1 / P2); computing them from extrinsics is not part of this. */
#define SS_MAX_RECTIFY_MAPS 16 /* maps one context holds: two eyes for each of SS_MAX_CAMERAS */
typedef struct {
    double fx, fy, cx, cy;     /* raw intrinsics */
    double k1, k2, p1, p2, k3; /* distortion, OpenCV's order */
    double R[9];               /* rectifying rotation, row-major */
    double fx_new, fy_new, cx_new, cy_new;
    int32_t width, height;
} ss_rectify_model;
/* Fills two [height][width] float arrays by the builder above.  Pure host code: no context, no device. */
int ss_rectify_build_map(const ss_rectify_model *m, float *map_x, float *map_y);
/* Converts any float map pair (the builder's or the caller's own) to the fixed-point form and uploads it as map map_id
 * (0 <= map_id < SS_MAX_RECTIFY_MAPS), replacing what was there; another size is allowed.  map_x == map_y == NULL with width 0
 * drops the map.  Synchronises the context's stream: a per-calibration call, not a per-frame one. */
int ss_rectify_set_map(ss_ctx *ctx, int map_id, const float *map_x, const float *map_y, int width, int height);
/* n_frames <= max_batch frames in device memory (strides in bytes, channels 1, 3 or 4), frame b remapped with map map_ids[b]
 * (a HOST table [n_frames], copied before the call returns) into d_dst.  Asynchronous on the context's stream.  Writes exactly
 * width * channels bytes of every destination row and nothing else.  SS_ERR_INVALID_ARG: an id out of range, an unset map, a map
 * whose size differs from the frames', source and destination ranges that overlap, a destination stride smaller than a row /
 * a frame, n_frames > max_batch, a source frame whose rows span 4 GiB or more; a NULL pointer, n_frames < 1 or source strides
 * smaller than the frame are SS_ERR_BAD_FRAME, as in ss_extract_batch_device.  A gray result whose d_dst,
 * dst_row_stride and dst_frame_stride are multiples of 16 is read in place, as level 0, by a following
 * ss_extract_batch_device. */
int ss_rectify_batch_device(ss_ctx *ctx, const void *d_src, int n_frames, int width, int height, int channels,
                            int64_t row_stride, int64_t frame_stride, const int32_t *map_ids, void *d_dst,
                            int64_t dst_row_stride, int64_t dst_frame_stride);
/* ss_extract_stereo on a RAW pair: both eyes are uploaded, remapped on the device (colour included: upstream remaps before the
 * gray conversion too) with maps map_left / map_right into a buffer of the context, then extracted and matched as
 * ss_extract_stereo does.  The stereo parameters are the caller's: after rectification fx is fx_new and the baseline comes from
 * P2, not from the raw calibration, so gray input needs no calibration; colour input follows ss_extract's rule for the RGB
 * order (SS_ERR_NOT_CALIBRATED before any calibration).  Needs a context created with max_batch >= 2. */
int ss_extract_stereo_raw(ss_ctx *ctx, int camera_id, const uint8_t *left, const uint8_t *right, int width, int height,
                          int channels, int row_stride, double timestamp, int map_left, int map_right,
                          const ss_stereo_params *sp, ss_frame_result *out_left, ss_frame_result *out_right,
                          const ss_stereo_point **points, ss_stereo_summary *summary);

/* ---- guided matching: descriptor search inside a pixel window (ORB-SLAM3 ORBmatcher::SearchForInitialization /
 * SearchByProjection on Frame::GetFeaturesInArea; neither source file is in the reference tree: the rule below is this
 * library's own restatement, parity unpinned like the rest of the path) ----------------------------
 * Query row i has a window (x, y, radius, oct_lo, oct_hi).
 *   Candidates: train row j < n_train with oct_lo <= octave_j <= oct_hi, fabsf(x_j - x) < radius and fabsf(y_j - y) < radius
 *     (both strict, every difference one float32 operation on the keypoints' x / y as they are: the membership test inside
 *     GetFeaturesInArea; the device's grid only finds them faster).  A query whose radius is not > 0 (zero, negative, NaN) has
 *     none; oct_lo > oct_hi gives none.
 *   d1 = the lowest distance over the candidates, idx = the lowest j among those, d2 = the lowest distance over the candidates
 *     j != idx (a duplicate gives d2 == d1), 0xFFFF = absent: ss_match's rule, so a window that covers everything gives what
 *     ss_match gives.  d1 / d2 are always these raw values; idx is what survives the tests below, else -1.
 *   Accept iff d1 <= th and (ratio_den == 0 or d1 * ratio_den < d2 * ratio_num).  ratio_den 0 is SearchByProjection (no ratio
 *     test), 9 / 10 with th 50 SearchForInitialization.  0 <= ratio_num, ratio_den <= 32767.
 *   one_to_one: among the accepted queries that name the same train row the one with the lowest d1 << 20 | i keeps it, the
 *     others get -1.  Deviation: upstream resolves such conflicts while it walks the queries in order (vMatchedDistance,
 *     vnMatches21), which depends on that order; this is the order-free form of "the closer one wins, ties to the lower query".
 *   orientation (0 off, 1, 2), on what is left: rot = angle_query - angle_train; if (rot < 0) rot += 360.0f;
 *     bin = (int)roundf(rot * factor) (half away from zero); if (bin == 30) bin = 0.  factor is 1.0f / 30 for 1 (bins 0..12 are
 *     used and 359 degrees lands in bin 12) and 30 / 360.0f for 2: both forms exist upstream, which one the reference binary
 *     runs is unpinned.  Then ComputeThreeMaxima: bins 0..29 scanned with a strict > against max1, max2, max3 in turn; if
 *     (float)max2 < 0.1f * (float)max1 the second and third are dropped, else if (float)max3 < 0.1f * (float)max1 the third.
 *     Matches outside the kept bins get -1; so does a match whose bin is outside 0..29 or NaN, which takes caller-made angles
 *     outside [0, 360) (upstream asserts).  Every step is a single float32 operation. */
#define SS_GUIDED_MAX_ROWS 16384 /* rows per frame: the conflict keys hold a row in 20 bits, a frame's keys one workgroup's LDS */
typedef struct {          /* 16 bytes, one per query row */
    float x, y, radius;
    int16_t oct_lo, oct_hi;
} ss_guided_window;
typedef struct {          /* 40 bytes */
    int32_t th, ratio_num, ratio_den;   /* ratio_den 0 = no ratio test */
    int32_t one_to_one, orientation;    /* orientation 0 / 1 / 2 as above */
    /* only when d_windows == NULL (batch form): the window of a query is its own position, radius `radius`, or radius *
     * scale[octave] of the context's pyramid when radius_by_octave is set, octaves octave -+ octave_span */
    float radius;
    int32_t radius_by_octave, octave_span;
    /* pairs / host form: the image size the coordinates live in; it sizes the index only and never changes a result
     * (coordinates outside it, infinite or NaN are binned into a border cell); <= 0 is SS_ERR_INVALID_ARG.  Batch form: ignored */
    int32_t extent_w, extent_h;
} ss_guided_params;
typedef struct {          /* 32 bytes, one per frame */
    int32_t status;       /* SS_OK, or the ss_status that voided the frame (frame_error of either side: all rows "none", counts 0) */
    int32_t n_query, n_train;
    int32_t n_candidates; /* Hamming distances taken = the sum of the candidate-set sizes */
    int32_t n_accepted, n_unique, n_final; /* after the acceptance test, after one_to_one, after orientation */
    int32_t rot_bins;     /* the kept bins ind1 | ind2 << 8 | ind3 << 16, 0xFF = none; 0xFFFFFF when orientation is off */
} ss_guided_summary;
/* n_frames independent (query frame, train frame) pairs on caller-supplied device arrays laid out like ss_match_pairs_device:
 * descriptors [n_frames][rows_per_frame][32] and keypoints [n_frames][rows_per_frame] (ss_keypoint: x, y, octave of the train
 * side and angle of both sides are read) on both sides, counts d_n_query / d_n_train (device int32 [n_frames], clamped to
 * 0 .. rows_per_frame), d_windows [n_frames][rows_per_frame] ss_guided_window.  Outputs: d_idx (int32) / d_d1 / d_d2 (uint16)
 * [n_frames][rows_per_frame], rows >= n_query get -1 / 0xFFFF, and d_summary [n_frames] ss_guided_summary.  No self-exclusion.
 * rows_per_frame > SS_GUIDED_MAX_ROWS is SS_ERR_INVALID_ARG.  Asynchronous on the context's stream. */
int ss_match_guided_pairs_device(ss_ctx *ctx, const void *d_query, const void *d_query_kp, const void *d_n_query,
                                 const void *d_train, const void *d_train_kp, const void *d_n_train, const void *d_windows,
                                 int n_frames, int rows_per_frame, const ss_guided_params *p, void *d_idx, void *d_d1, void *d_d2,
                                 void *d_summary);
/* The frames of the last ss_extract_batch_device batch.  train_src is a HOST table [n_frames] as in
 * ss_match_batch_sources_device, without the carry: t >= 0 names frame t of the batch (the pair j == i is excluded iff
 * t == b), -1 no train; t <= -2 or t >= n_frames is SS_ERR_INVALID_ARG.  NULL: frame b against frame b - 1, frame 0 without a
 * train.  d_windows: device [n_frames][kp_capacity], or NULL (the windows follow from p, above).  Outputs are
 * [n_frames][kp_capacity] and d_summary [n_frames].  A frame whose frame_error is set, on either side, gets that status and
 * all-none rows, as the stereo stages do.  Asynchronous on the context's stream. */
int ss_match_guided_batch_device(ss_ctx *ctx, const int32_t *train_src, const void *d_windows, const ss_guided_params *p,
                                 void *d_idx, void *d_d1, void *d_d2, void *d_summary);
/* One pair with host pointers in and out (copy in, the pairs form, copy out), synchronous: the counterpart of ss_match.
 * n_query, n_train <= SS_GUIDED_MAX_ROWS; windows has n_query entries. */
int ss_match_guided(ss_ctx *ctx, const uint8_t *query, const ss_keypoint *query_kp, int n_query, const uint8_t *train,
                    const ss_keypoint *train_kp, int n_train, const ss_guided_window *windows, const ss_guided_params *p,
                    int32_t *idx, uint16_t *d1, uint16_t *d2, ss_guided_summary *summary);

/* ---- bag of words: DBoW2's vocabulary tree on the device (TemplatedVocabulary::transform as Frame::ComputeBoW calls it,
 * ORBmatcher::SearchByBoW, L1Scoring::score as KeyFrameDatabase ranks keyframes with it; none of these sources is in the reference
 * tree and no ORBvoc.txt is at hand: the rule below is this library's own restatement from DBoW2 / ORBmatcher.cc as published,
 * parity with the real binary unpinned like the rest of the path; tests/bow_ref.py is the normative statement, reproduced bit
 * for bit) ----------------------------------------------------------------------------------------------
 * Vocabulary: a tree whose root is node 0; node ids are the text file's (line n, from 0, is node n + 1), word ids count the
 *   leaves in file order, a node's children are in file order.  Node and word ids reported by any call are these, whatever the
 *   device layout (breadth first, so that the children of a node are consecutive 32-byte rows).
 * Transform of one descriptor row (transform(feature, id, w, &nid, levelsup)): start at the root, depth 0; until the node is a
 *   leaf go to the child with the lowest Hamming distance (ties: the earliest child, upstream's strict < in a forward scan),
 *   depth += 1, and when depth == L - levelsup remember that node as the row's NODE.  The leaf is the row's WORD, its weight w.
 *   L - levelsup <= 0: the node is 0.  Deviation: a leaf shallower than L - levelsup is the row's node itself (upstream leaves
 *   *nid unwritten there).  A row for which w > 0 is false takes part in nothing: its word is reported, its node is -1.
 * BoW vector of a frame (BowVector::addWeight, normalize(L1)): the distinct words of the rows with w > 0, ascending; the value of
 *   a word seen c times is w, then += w (c - 1) times; norm = the sum of fabs(value) in ascending word order, ONE serial chain of
 *   double additions; if norm > 0.0 every value is divided by it.  Every step is one IEEE double operation.
 * Bounds.  SS_VOCAB_MAX_K: the descent folds the key distance << 8 | child ordinal, so an ordinal has 8 bits (DBoW2 builds k = 10,
 *   OpenCV-style trees up to 32).  SS_VOCAB_MAX_DEPTH: bounds the descent loop, nothing is stored per level (ORBvoc.txt has L = 6).
 *   SS_VOCAB_MAX_NODES: 2^24 nodes are 768 MiB on the device (32-byte row + 16-byte record each); ORBvoc.txt has about 1.08 M.
 *   SS_BOW_MAX_ROWS: a frame's rows are sorted as 64-bit keys in one workgroup's LDS (128 KiB of the CU's 160), and the match
 *   shares ss_match_guided's row bound. */
#define SS_VOCAB_MAX_K 256
#define SS_VOCAB_MAX_DEPTH 32
#define SS_VOCAB_MAX_NODES (1 << 24)
#define SS_BOW_MAX_ROWS SS_GUIDED_MAX_ROWS
typedef struct ss_vocab ss_vocab; /* host object, no device needed */
typedef struct {          /* 20 bytes */
    int32_t k, L;         /* the header's branching factor and depth */
    int32_t n_nodes;      /* nodes without the root = lines of the file; ids 1 .. n_nodes */
    int32_t n_words;      /* leaves */
    int32_t max_depth;    /* of the deepest leaf (the root has depth 0); may differ from L */
} ss_vocab_shape;
/* DBoW2's text format: a header line `k L scoring weighting`, then one line per node `parent_id is_leaf b0 .. b31 weight`
 * (weight through strtod).  Only scoring 0 (L1) and weighting 0 (TF-IDF) are accepted, what ORBvoc.txt declares.  A file that is
 * malformed (truncated line, a byte > 255, a parent id that is not an earlier node, more than k children, an inner node without
 * children, a leaf with children, no node at all, a token that is no number) or exceeds a bound above is SS_ERR_INVALID_ARG with
 * a message in err (err_bytes including the NUL; err may be NULL); a file that cannot be read is SS_ERR_INVALID_ARG too. */
int ss_vocab_load_text(const char *path, ss_vocab **out, char *err, int err_bytes);
/* The same from arrays of n_nodes entries, entry n = node n + 1: parent ids, leaf flags, 32-byte descriptors, weights. */
int ss_vocab_from_arrays(int n_nodes, const int32_t *parent, const uint8_t *is_leaf, const uint8_t *desc, const double *weight,
                         int k, int L, ss_vocab **out, char *err, int err_bytes);
int ss_vocab_info(const ss_vocab *voc, ss_vocab_shape *out);
/* The flattened tree, for tests: arrays of n_nodes + 1 entries indexed by node id (0 = the root): the id of the first child (-1
 * for a leaf), the child count, the word id (-1 for an inner node), the weight (0.0 for an inner node), the depth.  Any pointer
 * may be NULL. */
int ss_vocab_copy_out(const ss_vocab *voc, int32_t *first_child, int32_t *n_children, int32_t *word, double *weight, int32_t *depth);
int ss_vocab_destroy(ss_vocab *voc);
/* Uploads the vocabulary; the context keeps its own device copy (voc may be destroyed afterwards), a second call replaces it.
 * Synchronises the context's stream.  The transform and match calls below return SS_ERR_STATE before the first one. */
int ss_bow_set_vocabulary(ss_ctx *ctx, const ss_vocab *voc);
typedef struct {          /* 32 bytes, one per frame */
    int32_t status;       /* SS_OK, or the frame_error that voided the frame (all rows -1, empty vector) */
    int32_t n_rows;       /* rows transformed */
    int32_t n_used;       /* rows with w > 0 */
    int32_t n_words;      /* distinct words among them = entries of the BoW vector */
    int32_t n_nodes;      /* distinct nodes among them */
    int32_t reserved;     /* 0 */
    double norm;          /* the L1 norm the values were divided by (0.0: nothing was divided) */
} ss_bow_summary;
/* Caller arrays laid out as for ss_match_pairs_device: d_desc [n_frames][rows_per_frame][32], d_n_rows device int32 [n_frames]
 * (clamped to 0 .. rows_per_frame).  Outputs [n_frames][rows_per_frame]: d_word / d_node (int32, -1 past the count), d_bow_word
 * (int32, ascending, -1 past n_words), d_bow_value (double, 0.0 past n_words); d_summary [n_frames] ss_bow_summary.
 * rows_per_frame > SS_BOW_MAX_ROWS or levelsup < 0 is SS_ERR_INVALID_ARG.  Asynchronous on the context's stream, which is a
 * non-blocking one: the outputs are written by one kernel and read again by the next, so they stay allocated and untouched until
 * the call has run (ss_synchronize, or an event on ss_get_stream). */
int ss_bow_transform_device(ss_ctx *ctx, const void *d_desc, const void *d_n_rows, int n_frames, int rows_per_frame, int levelsup,
                            void *d_word, void *d_node, void *d_bow_word, void *d_bow_value, void *d_summary);
/* The frames of the last ss_extract_batch_device batch (rows_per_frame = kp_capacity).  A frame whose frame_error is set gets
 * that status, all rows -1 and an empty vector.  The context keeps the nodes and their index for ss_match_bow_batch_device. */
int ss_bow_transform_batch_device(ss_ctx *ctx, int levelsup, void *d_word, void *d_node, void *d_bow_word, void *d_bow_value,
                                  void *d_summary);
/* SearchByBoW.  The candidates of query row i are the train rows j < n_train with node_j == node_i, node_i >= 0; from there on
 * ss_match_guided's rule word for word (d1 / lowest idx / d2, acceptance, one_to_one, orientation, raw d1 / d2), through the same
 * finishing kernel.  Of p only th, ratio_num, ratio_den, one_to_one and orientation are read; upstream's call is th 50, ratio
 * 7 / 10, orientation on.  Upstream skips keyframe rows without a map point: write -1 into their node.  It also skips frame rows
 * already matched, which is the one_to_one deviation of ss_match_guided.  Arrays as for ss_match_guided_pairs_device, with
 * d_query_node / d_train_node (device int32 [n_frames][rows_per_frame]) in place of the windows; needs no vocabulary. */
int ss_match_bow_pairs_device(ss_ctx *ctx, const void *d_query, const void *d_query_kp, const void *d_query_node, const void *d_n_query,
                              const void *d_train, const void *d_train_kp, const void *d_train_node, const void *d_n_train,
                              int n_frames, int rows_per_frame, const ss_guided_params *p, void *d_idx, void *d_d1, void *d_d2,
                              void *d_summary);
/* The frames and nodes of the last ss_bow_transform_batch_device (SS_ERR_STATE without one on the current batch); train_src and
 * its self-exclusion rule are those of ss_match_guided_batch_device. */
int ss_match_bow_batch_device(ss_ctx *ctx, const int32_t *train_src, const ss_guided_params *p, void *d_idx, void *d_d1, void *d_d2,
                              void *d_summary);
/* L1Scoring::score of one query vector (d_q_word ascending int32 / d_q_value double, q_rows entries allocated, *d_q_count used)
 * against n_db vectors stored [n_db][stride] with a device int32 count each (counts are clamped to the allocation): both
 * ascending lists are walked; for each common word, in ascending order, s += fabs(v - w) - fabs(v) - fabs(w) (v the query's
 * value; three double operations left to right, then the add), s starting at 0.0; score = -s / 2.0 (so -0.0 without a common
 * word); an empty side gives 0.0.  d_score: double [n_db].  Vectors are kept outputs of the transform; needs no vocabulary.
 * Asynchronous on the context's stream. */
int ss_bow_score_device(ss_ctx *ctx, const void *d_q_word, const void *d_q_value, const void *d_q_count, int q_rows,
                        const void *d_db_word, const void *d_db_value, const void *d_db_count, int n_db, int stride, void *d_score);

/* ---- map-point projection search: Tracking::SearchLocalPoints = Frame::isInFrustum followed by
 * ORBmatcher::SearchByProjection(Frame&, vector<MapPoint*>&, th).  Neither upstream source is in the reference tree.  This is the
 * library's own restatement and parity with the real binary stays unpinned, as for the guided and the bag-of-words stages.
 * tests/proj_ref.py is its normative statement; DESIGN.md section 17 --------------------------------------------------------
 * - Every float step is one float32 IEEE operation, left to right as written, with no contraction.
 * - Every test is written in its accepting form, so a NaN fails it.
 * Per frame there is one view, ss_proj_view, all float32: rcw[9] row-major, tcw[3], ow[3]; fx, fy, cx, cy, bf; min_x, max_x,
 * min_y, max_y (upstream's mnMinX and the rest).
 * Per map point there is one ss_map_point of 32 bytes: x y z, nx ny nz (mean viewing direction), min_dist, max_dist.  These are
 * mfMinDistance / mfMaxDistance as stored, before the 0.8 / 1.2 factors.  Each point also has a 32-byte descriptor.
 * 1. Frustum.  The state is the number of the first test that fails; 0 means in view.
 *    1. Test 1: pc = R.P + t, each component ((r0*x + r1*y) + r2*z) + t.  The test is pc.z > 0.
 *    2. Test 2: invz = 1.0f / pc.z; u = fx*pc.x*invz + cx (two products, then the sum); v is formed likewise; the test is
 *       u >= min_x && u <= max_x && v >= min_y && v <= max_y.
 *    3. Test 3: po = P - ow; dist = sqrtf((po.x*po.x + po.y*po.y) + po.z*po.z); the test is
 *       dist >= 0.8f*min_dist && dist <= 1.2f*max_dist.
 *    4. Test 4: view_cos = ((po.x*nx + po.y*ny) + po.z*nz) / dist; the test is view_cos >= view_cos_limit.
 *    5. Test 5 applies only when far_limit > 0.  The test is dist <= far_limit.
 *       Deviation: upstream tests ||pc||, which is the same number in exact arithmetic.
 * 2. Level.  ratio = max_dist / dist.  level is the smallest n in 0 .. n_levels-1 with ratio <= scale[n], else n_levels-1.
 *    scale[] is the context's pyramid table (ss_geometry.cpp).
 *    Deviation: upstream evaluates ceil(logf(ratio) / logScaleFactor) and clamps it.  Checked on the CPU with numpy's float32 log,
 *    scale 1.2 and 8 levels: the sweep was 2 M ratios in [0.3, 5] plus +-3000 ulp around every table entry; the two forms differ
 *    at one value, and that ratio equals a table entry.  (How many ratios differ depends on the float32 log at hand;
 *    tests/test_proj_ref.py repeats the sweep and requires every disagreement to lie within 2 ulp of a table entry.)
 * 3. Window.  r = (view_cos > 0.998f ? 2.5f : 4.0f) * th.  radius = r * scale[level].  u_right = u - bf*invz.
 *    A candidate is a train row j < n_train that passes all of:
 *    - level-1 <= octave_j <= level;
 *    - fabsf(x_j - u) < radius and fabsf(y_j - v) < radius, ss_match_guided's membership test, unchanged;
 *    - if a taken mask is given, taken[j] == 0;
 *    - if check_right is set and right[j] > 0, then fabsf(u_right - right[j]) <= radius.
 * 4. Best and second.  The key is distance << 20 | j.  The best is the lowest key.  The second is the lowest key over the other
 *    candidates.  idx, d1, lvl1 come from the best.  d2, lvl2 come from the second.  With no second candidate, d2 is 0xFFFF and
 *    lvl2 is -1.  Deviation: upstream's bestLevel2 depends on the scan order when seconds tie.
 * 5. Accept iff d1 <= th_high and not (ratio_den != 0 and lvl1 == lvl2 and d1*ratio_den > d2*ratio_num).  Upstream uses 100 and
 *    8 / 10.  Equality accepts, as upstream's bestDist > mfNNratio*bestDist2 does.
 * 6. one_to_one is optional and is ss_match_guided's order-free rule on d1 << 20 | i.  Upstream has none: a later map point
 *    overwrites an earlier one.  With 0, several points may name one row.
 * Outputs per point row: idx is int32, -1 when not accepted.  d1 / d2 are uint16 raw values, 0xFFFF when absent.  ss_proj_point is
 * 32 bytes: u, v, u_right, view_cos, dist, radius, int32 level, int32 state.  When state != 0, the floats are 0.0f and level is
 * -1.  Rows >= n_points get state -1 and "none".
 * Outputs per frame: ss_proj_summary, 32 bytes, holding status, n_points, n_train, n_in_view, n_candidates, n_accepted, n_unique,
 * reserved 0. */
typedef struct {          /* 96 bytes, one per frame */
    float rcw[9], tcw[3], ow[3];
    float fx, fy, cx, cy, bf;
    float min_x, max_x, min_y, max_y;
} ss_proj_view;
typedef struct {          /* 32 bytes, one per map point */
    float x, y, z;
    float nx, ny, nz;
    float min_dist, max_dist;
} ss_map_point;
typedef struct {          /* 32 bytes, one per point row */
    float u, v, u_right, view_cos, dist, radius;
    int32_t level, state;
} ss_proj_point;
typedef struct {          /* 40 bytes */
    float view_cos_limit; /* upstream: 0.5; NaN is SS_ERR_INVALID_ARG */
    float th;             /* the window factor of step 3; must be finite and > 0 */
    float far_limit;      /* test 5; not > 0 (zero, negative, NaN): no test */
    int32_t th_high;      /* 0 .. 256 */
    int32_t ratio_num, ratio_den; /* 0 .. 32767; ratio_den 0 = no ratio test */
    int32_t one_to_one, check_right;
    int32_t extent_w, extent_h;   /* as in ss_guided_params: they size the index only; the batch form ignores them */
} ss_proj_params;
typedef struct {          /* 32 bytes, one per frame */
    int32_t status;       /* SS_OK, or the frame_error that voided the frame (all rows "none", counts 0) */
    int32_t n_points, n_train;
    int32_t n_in_view;    /* points with state 0 */
    int32_t n_candidates; /* Hamming distances taken */
    int32_t n_accepted, n_unique; /* after the acceptance test, after one_to_one */
    int32_t reserved;     /* 0 */
} ss_proj_summary;
/* The view of a camera at pose (rcw row-major, tcw), needs no device: every number rounded to float32 once; ow = -R^T t is formed
 * in double (((r0*t0 + r3*t1) + r6*t2, negated) and then rounded; the bounds are 0 .. width, 0 .. height. */
int ss_proj_view_init(const ss_camera *cam, const double rcw[9], const double tcw[3], float bf, ss_proj_view *out);
/* The host twin of steps 1 - 3 for n points: out[i] is what the device calls write for the point.  scale: n_levels entries,
 * 1 <= n_levels <= SS_MAX_LEVELS.  Needs no device.  p is checked as the device calls check it (SS_ERR_INVALID_ARG). */
int ss_proj_points_host(const ss_proj_view *view, const ss_proj_params *p, const float *scale, int n_levels,
                        const ss_map_point *points, int n, ss_proj_point *out);
/* n_frames frames on caller-supplied device arrays.  Map points: d_points [n_blocks][point_rows] ss_map_point, d_point_desc
 * [n_blocks][point_rows][32], counts d_n_points (device int32 [n_blocks], clamped to 0 .. point_rows).  Train side, as for
 * ss_match_guided_pairs_device: d_train [n_frames][rows_per_frame][32], d_train_kp [n_frames][rows_per_frame] ss_keypoint,
 * d_n_train device int32 [n_frames]; optional (NULL: absent) d_train_right float and d_train_taken uint8, both
 * [n_frames][rows_per_frame].  views: a HOST table of n_frames views.  point_src: a HOST table [n_frames] of block numbers, frame b
 * searches the points of block point_src[b]; NULL: frame b reads block b (then n_blocks >= n_frames).  Both tables are copied
 * before the call returns.  Outputs: d_idx (int32) / d_d1 / d_d2 (uint16) / d_proj (ss_proj_point) [n_frames][point_rows] and
 * d_summary [n_frames] ss_proj_summary.  SS_ERR_INVALID_ARG: either row count above SS_GUIDED_MAX_ROWS, th not > 0 or not finite, a
 * NaN view_cos_limit, th_high outside 0 .. 256, a ratio term outside 0 .. 32767, a point_src entry outside 0 .. n_blocks - 1,
 * extent_w or extent_h <= 0, a NULL buffer.  Asynchronous on the context's stream. */
int ss_match_proj_pairs_device(ss_ctx *ctx, const void *d_points, const void *d_point_desc, const void *d_n_points, int n_blocks,
                               int point_rows, const void *d_train, const void *d_train_kp, const void *d_n_train,
                               const void *d_train_right, const void *d_train_taken, int n_frames, int rows_per_frame,
                               const ss_proj_view *views, const int32_t *point_src, const ss_proj_params *p, void *d_idx, void *d_d1,
                               void *d_d2, void *d_proj, void *d_summary);
/* The same, the train side being the frames of the last ss_extract_batch_device batch (n_frames and kp_capacity are the batch's;
 * d_train_right / d_train_taken are [n_frames][kp_capacity]).  A frame whose frame_error is set gets that status in its summary
 * and all its rows are "none". */
int ss_match_proj_batch_device(ss_ctx *ctx, const void *d_points, const void *d_point_desc, const void *d_n_points, int n_blocks,
                               int point_rows, const void *d_train_right, const void *d_train_taken, const ss_proj_view *views,
                               const int32_t *point_src, const ss_proj_params *p, void *d_idx, void *d_d1, void *d_d2, void *d_proj,
                               void *d_summary);
/* One frame with host pointers in and out (copy in, the pairs form, copy out), synchronous: the counterpart of ss_match_guided.
 * n_points, n_train <= SS_GUIDED_MAX_ROWS; train_right / train_taken may be NULL; proj may be NULL. */
int ss_match_proj(ss_ctx *ctx, const ss_proj_view *view, const ss_map_point *points, const uint8_t *point_desc, int n_points,
                  const uint8_t *train, const ss_keypoint *train_kp, int n_train, const float *train_right,
                  const uint8_t *train_taken, const ss_proj_params *p, int32_t *idx, uint16_t *d1, uint16_t *d2,
                  ss_proj_point *proj, ss_proj_summary *summary);

/* ---- epipolar search and triangulation: ORBmatcher::SearchForTriangulation, then the per-match part of
 * LocalMapping::CreateNewMapPoints with MapPoint::UpdateNormalAndDepth: new map points from (keyframe 1 = query, keyframe 2 =
 * train) pairs.  Neither upstream source is in the reference tree.  This is the library's own restatement and parity with the real
 * binary stays unpinned, as for the guided, bag-of-words and projection stages.  tests/epi_ref.py is its normative statement;
 * DESIGN.md section 18.  An addition to ABI 5: nothing existing changes ---------------------------------------------------------
 * Out of scope: stereo rows in ss_triangulate_* (a row with a right coordinate is treated as monocular there; the stereo parallax,
 * unprojectStereo and the three-term error are ss_triangulate_stereo_*, below),
 * fisheye models (pinhole only; keypoints are taken as undistorted, upstream's mvKeysUn: k1 k2 p1 p2 are not read), the per-pair
 * baseline / median-depth gate of CreateNewMapPoints (the caller decides which pairs to submit), Fuse, culling, the observations
 * bookkeeping and any wiring into ss_track.
 * The pair.  One ss_epi_pair per pair, made on the host by ss_epi_pair_init, handed to the device calls as a HOST table that is
 * copied before the call returns.  It has a float32 part for the search and a double part for the triangulation.
 *   Float32 part.  All of it is formed in double, one IEEE operation per step, then rounded once:
 *   - R12[i][j] = (R1[i][0]*R2[j][0] + R1[i][1]*R2[j][1]) + R1[i][2]*R2[j][2]           (R12 = R1w.R2w^T)
 *   - t12[i] = t1[i] - ((R12[i][0]*t2[0] + R12[i][1]*t2[1]) + R12[i][2]*t2[2])
 *   - E = [t12]x.R12: E[0][j] = t12[1]*R12[2][j] - t12[2]*R12[1][j], E[1][j] = t12[2]*R12[0][j] - t12[0]*R12[2][j],
 *     E[2][j] = t12[0]*R12[1][j] - t12[1]*R12[0][j]
 *   - G = K1^-T.E: G[0][j] = invfx1*E[0][j], G[1][j] = invfy1*E[1][j], G[2][j] = E[2][j] - (cx1*G[0][j] + cy1*G[1][j])
 *   - F = G.K2^-1: F[i][0] = G[i][0]*invfx2, F[i][1] = G[i][1]*invfy2, F[i][2] = G[i][2] - (F[i][0]*cx2 + F[i][1]*cy2)
 *   - f12[3*i + j] = (float)(F[i][j] / m), m the largest |F[i][j]|.  If an entry is not finite or m is 0, f12 is all 0.0f and the
 *     epipolar test fails for every couple (den > 0 is false).  Deviation: upstream does not normalise; the test is scale-free in
 *     exact arithmetic, and the division keeps a*a + b*b away from float32 underflow for short baselines.
 *   - The epipole of camera 1 in image 2: C2[i] = ((R2[i][0]*ow1[0] + R2[i][1]*ow1[1]) + R2[i][2]*ow1[2]) + t2[i];
 *     ex = (float)((fx2*C2[0])/C2[2] + cx2), ey = (float)((fy2*C2[1])/C2[2] + cy2).  epipole_test is 1 iff both are finite after the
 *     rounding; else it is 0, ex = ey = 0.0f are stored and the epipole test is skipped (sideways motion has its epipole at
 *     infinity, no keypoint is near it).
 *   Double part.  rcw, tcw as given, ow[k] = -((r[k]*t[0] + r[3+k]*t[1]) + r[6+k]*t[2]) as in ss_proj_view_init, then
 *   fx, fy, cx, cy, 1.0/fx, 1.0/fy of each camera.
 * The search, for query row i.  The row is live iff i < n_query, node_i >= 0 and it is not taken.  A candidate is a train row
 *   j < n_train, not taken, with node_j == node_i (a VISITED couple).  scale[] is the context's pyramid table, n_levels entries,
 *   sigma2[n] = scale[n]*scale[n] in float32.  Every float step is one float32 operation, left to right, no contraction; every test
 *   is in its accepting form, so a NaN fails it.  A candidate must pass, in this order:
 *   1. Octave: 0 <= octave_j < n_levels (caller-made keypoints may violate it; such a row is no candidate).
 *   2. Epipole, only when epipole_test: dx = ex - x_j, dy = ey - y_j; accept iff dx*dx + dy*dy >= 100.0f * scale[octave_j]
 *      (upstream rejects <).
 *   3. Epipolar line, unless coarse: a = (x_i*f[0] + y_i*f[3]) + f[6], b = (x_i*f[1] + y_i*f[4]) + f[7],
 *      c = (x_i*f[2] + y_i*f[5]) + f[8]; num = (a*x_j + b*y_j) + c; den = a*a + b*b; accept iff den > 0.0f and
 *      num*num/den < 3.84f * sigma2[octave_j].  Deviation: upstream evaluates the right-hand side in double.
 *   4. Distance: Hamming <= th.
 *   The best is the lowest key distance << 20 | j; idx and d1 come from it; there is no second best and no ratio test.
 *   Deviation: upstream keeps the LAST of several equal distances in scan order (dist > bestDist -> continue); here the lowest row
 *   wins, as everywhere in this library.  Then one_to_one and the rotation histogram run through guided matching's finishing kernel,
 *   unchanged (orientation 0 / 1 / 2 as there).  Upstream's vbMatched2 is the ORB-SLAM2 behaviour and ORB-SLAM3 never sets it; here
 *   one_to_one is ss_match_guided's order-free rule, off by default.  Upstream's call: th 50, coarse 0, orientation on.
 *   The counters follow the rule's order, so a descriptor is loaded only for a couple that passed the geometry; the conjunction makes
 *   the winner independent of the order.
 *   Outputs per query row: idx int32 (-1: none), d1 uint16 (raw, 0xFFFF: none); rows >= n_query get -1 / 0xFFFF.
 * The triangulation of query row i with train row j = idx[i]; an entry outside 0 .. n_train - 1 is "no match", state -1.  All steps
 *   are in double, one IEEE operation each, left to right; x, y and scale[] are converted exactly from float32, s_n = scale[n],
 *   sigma2 = s*s in double.  The state is the number of the first failing test, 0 = a map point.  An octave of either row outside
 *   0 .. n_levels - 1 is state 10, tested before step 1.
 *   1. Parallax: xn = ((x - cx)*invfx, (y - cy)*invfy, 1); ray[k] = (R[k]*xn.x + R[3+k]*xn.y) + R[6+k] (R^T.xn) for each side;
 *      cos = ((r1x*r2x + r1y*r2y) + r1z*r2z) / (sqrt((r1x*r1x + r1y*r1y) + r1z*r1z) * sqrt(the same of ray2)); accept iff
 *      cos > 0 && cos < cos_parallax_max.
 *   2. DLT: A[0][c] = xn1.x*P1[2][c] - P1[0][c], A[1][c] = xn1.y*P1[2][c] - P1[1][c], A[2], A[3] the same of side 2 (P = [R|t]);
 *      M[i][j] = ((A[0][i]*A[0][j] + A[1][i]*A[1][j]) + A[2][i]*A[2][j]) + A[3][i]*A[3][j] for i <= j, mirrored.  SS_TRI_SWEEPS
 *      sweeps of cyclic Jacobi on M, V = I, pairs (p, q) in the order (0,1) (0,2) (0,3) (1,2) (1,3) (2,3); a rotation is skipped
 *      iff M[p][q] is exactly 0.0; else theta = (M[q][q] - M[p][p]) / (2.0*M[p][q]), t = (theta >= 0 ? 1.0 : -1.0) /
 *      (fabs(theta) + sqrt(theta*theta + 1.0)), c = 1.0 / sqrt(t*t + 1.0), s = t*c; for k != p, q: M[k][p] = c*M[k][p] - s*M[k][q] and
 *      M[k][q] = s*M[k][p] + c*M[k][q] (both from the old values, mirrored); M[p][p] -= t*M[p][q]; M[q][q] += t*M[p][q];
 *      M[p][q] = 0.0; for every k: V[k][p] = c*V[k][p] - s*V[k][q], V[k][q] = s*V[k][p] + c*V[k][q] (old values).  v is the column
 *      of V at the smallest M[k][k], lowest k on a tie.  Accept iff v[3] is finite and != 0; X = v[0..2] / v[3].  No loop has a trip
 *      count that depends on the data.  Deviation: upstream runs Eigen's float32 JacobiSVD.
 *   3. z1 = ((R1[6]*X0 + R1[7]*X1) + R1[8]*X2) + t1[2] > 0.        4. The same for z2.
 *   5. Reprojection, side 1: u = (fx*x1c)/z1 + cx, v = (fy*y1c)/z1 + cy (x1c, y1c as z1 with rows 0 and 1); eu = u - x, ev = v - y;
 *      err1 = eu*eu + ev*ev; accept iff err1 <= chi2 * sigma2[octave_1].        6. The same for side 2.
 *   7. n1 = X - ow1, d1 = sqrt((n1x*n1x + n1y*n1y) + n1z*n1z); n2, d2 likewise; accept iff d1 > 0 && d2 > 0.
 *   8. Far limit, only when far_limit > 0: d1 < far_limit && d2 < far_limit.
 *   9. Scale: rd = d2/d1, ro = s[o1]/s[o2]; accept iff rd*ratio_factor >= ro && rd <= ro*ratio_factor.
 *   The map point of a state-0 row (UpdateNormalAndDepth, reference keyframe = keyframe 1): position X; normal
 *   (n1[k]/d1 + n2[k]/d2) / 2.0 (upstream does not renormalise either); max_dist = d1*s[o1]; min_dist = max_dist / s[n_levels - 1];
 *   each of the eight numbers rounded to float32 once.  Its descriptor is keyframe 1's row: with two observations
 *   ComputeDistinctiveDescriptors takes the first of a pointer-ordered map, here that is keyframe 1.
 *   ss_tri_info per query row: state, and cos_parallax, err1_sq, err2_sq rounded to float32 once the step that forms them was
 *   reached (whether it passed or not), 0.0f before; a NaN is reported as 0.0f.  Rows >= n_query get state -1 and 0.0f.
 *   Compact outputs, in ascending query row: d_points / d_point_desc / d_point_rows (int32 i, j) / d_n_points.  Rows from n_points
 *   on are not written.  d_points, d_point_desc and d_n_points are exactly the blocks ss_match_proj_pairs_device reads, with
 *   point_rows = rows_per_frame.
 * Alignment of the device buffers of these calls (hipMalloc's and any allocator's 256 bytes satisfy all of them; a sub-view at an
 *   odd offset does not): descriptors, d_points and d_point_desc 16 bytes; keypoints and d_point_rows 8; the rest 4. */
#define SS_TRI_SWEEPS 6
typedef struct {          /* 384 bytes, one per pair */
    float f12[9];
    float ex, ey;
    int32_t epipole_test;
    double rcw1[9], tcw1[3], ow1[3];
    double rcw2[9], tcw2[3], ow2[3];
    double fx1, fy1, cx1, cy1, invfx1, invfy1;
    double fx2, fy2, cx2, cy2, invfx2, invfy2;
} ss_epi_pair;
typedef struct {          /* 16 bytes */
    int32_t th;           /* 0 .. 256; upstream: 50 */
    int32_t coarse;       /* not 0: no epipolar-line test (upstream's bCoarse) */
    int32_t one_to_one, orientation; /* as in ss_guided_params */
} ss_epi_params;
typedef struct {          /* 40 bytes, one per pair */
    int32_t status;       /* SS_OK, or the frame_error that voided the pair (all rows "none", counts 0) */
    int32_t n_query, n_train;
    int32_t n_candidates; /* couples visited: same node, both untaken */
    int32_t n_geometric;  /* couples passing tests 1 - 3 */
    int32_t n_near;       /* couples also passing test 4 */
    int32_t n_accepted, n_unique, n_final; /* rows with a winner, after one_to_one, after orientation */
    int32_t rot_bins;     /* as in ss_guided_summary */
} ss_epi_summary;
typedef struct {          /* 32 bytes */
    double cos_parallax_max; /* upstream: 0.9998 */
    double chi2;             /* upstream: 5.991 */
    double ratio_factor;     /* upstream: 1.5f * scale_factor */
    double far_limit;        /* test 8; not > 0 (zero, negative, NaN): no test */
} ss_tri_params;
typedef struct {          /* 16 bytes, one per query row */
    int32_t state;
    float cos_parallax, err1_sq, err2_sq;
} ss_tri_info;
typedef struct {          /* 64 bytes, one per pair */
    int32_t status;       /* SS_OK, or the frame_error that voided the pair (all rows -1, no point) */
    int32_t n_query, n_train;
    int32_t n_matches;    /* rows whose state is not -1 */
    int32_t n_points;     /* rows of state 0 = n_state[0] */
    int32_t n_state[11];  /* rows per state 0 .. 10 */
} ss_tri_summary;
/* Needs no device.  NULL pointer: SS_ERR_INVALID_ARG.  A pose or camera that is not finite gives a pair that matches nothing. */
int ss_epi_pair_init(const ss_camera *cam1, const double rcw1[9], const double tcw1[3], const ss_camera *cam2, const double rcw2[9],
                     const double tcw2[3], ss_epi_pair *out);
/* Host twins of the steps (the text the kernels compile, csrc/ss_epi_steps.h); neither needs a device.  scale: n_levels entries,
 * 1 <= n_levels <= SS_MAX_LEVELS.  ss_epi_check_host: tests 1 - 3 of the n couples (kp1[k], kp2[k]); out[k] is 0 pass, 1 octave,
 * 2 epipole, 3 line.  ss_triangulate_host: the triangulation of the n couples; points[k] is all 0.0f unless info[k].state == 0. */
int ss_epi_check_host(const ss_epi_pair *pair, const ss_epi_params *p, const float *scale, int n_levels, const ss_keypoint *kp1,
                      const ss_keypoint *kp2, int n, uint8_t *out);
int ss_triangulate_host(const ss_epi_pair *pair, const ss_tri_params *tp, const float *scale, int n_levels, const ss_keypoint *kp1,
                        const ss_keypoint *kp2, int n, ss_map_point *points, ss_tri_info *info);
/* n_frames independent pairs.  The arrays of ss_match_bow_pairs_device, plus d_query_taken / d_train_taken (device uint8
 * [n_frames][rows_per_frame]; not 0 = the row already has a map point; NULL = none is taken) and pairs, a HOST table of n_frames
 * ss_epi_pair.  Outputs d_idx (int32) / d_d1 (uint16) [n_frames][rows_per_frame] and d_summary [n_frames] ss_epi_summary.  Needs no
 * vocabulary.  SS_ERR_INVALID_ARG: rows_per_frame above SS_GUIDED_MAX_ROWS, th outside 0 .. 256, orientation outside 0 .. 2, a NULL
 * required buffer; the context stays usable.  Asynchronous on the context's stream. */
int ss_match_epi_pairs_device(ss_ctx *ctx, const void *d_query, const void *d_query_kp, const void *d_query_node, const void *d_query_taken,
                              const void *d_n_query, const void *d_train, const void *d_train_kp, const void *d_train_node,
                              const void *d_train_taken, const void *d_n_train, int n_frames, int rows_per_frame, const ss_epi_pair *pairs,
                              const ss_epi_params *p, void *d_idx, void *d_d1, void *d_summary);
/* The frames and nodes of the last ss_bow_transform_batch_device (SS_ERR_STATE without one on the current batch).  train_src and its
 * rules are those of ss_match_guided_batch_device (the couple j == i is excluded iff train_src[b] == b; a bad entry is
 * SS_ERR_INVALID_ARG); pairs[b] is the pair (frame b, frame train_src[b]).  d_taken: device uint8 [n_frames][kp_capacity], read for
 * both sides, or NULL.  A frame whose frame_error is set, on either side, gets that status and all-none rows. */
int ss_match_epi_batch_device(ss_ctx *ctx, const int32_t *train_src, const void *d_taken, const ss_epi_pair *pairs, const ss_epi_params *p,
                              void *d_idx, void *d_d1, void *d_summary);
/* Triangulates the matches d_idx (device int32 [n_frames][rows_per_frame], the search's output or the caller's own) of n_frames
 * pairs: keypoints of both sides, the query descriptors, the counts, the HOST table pairs.  Outputs: d_info [n_frames][rows_per_frame]
 * ss_tri_info; the compact d_points (ss_map_point) / d_point_desc ([32]) / d_point_rows (int32 i, j) [n_frames][rows_per_frame],
 * d_n_points int32 [n_frames]; d_summary [n_frames] ss_tri_summary.  The compaction is deterministic.  SS_ERR_INVALID_ARG:
 * rows_per_frame above SS_GUIDED_MAX_ROWS, a NULL buffer.  Asynchronous on the context's stream. */
int ss_triangulate_pairs_device(ss_ctx *ctx, const void *d_query, const void *d_query_kp, const void *d_n_query, const void *d_train_kp,
                                const void *d_n_train, const void *d_idx, int n_frames, int rows_per_frame, const ss_epi_pair *pairs,
                                const ss_tri_params *tp, void *d_info, void *d_points, void *d_point_desc, void *d_point_rows,
                                void *d_n_points, void *d_summary);
/* The same on the frames of the last ss_extract_batch_device batch (rows_per_frame = kp_capacity), frame b against frame
 * train_src[b] (ss_match_guided_batch_device's table; -1: no train, every row -1).  A flagged frame on either side voids the pair. */
int ss_triangulate_batch_device(ss_ctx *ctx, const int32_t *train_src, const void *d_idx, const ss_epi_pair *pairs, const ss_tri_params *tp,
                                void *d_info, void *d_points, void *d_point_desc, void *d_point_rows, void *d_n_points, void *d_summary);
/* The stereo form of the triangulation: LocalMapping::CreateNewMapPoints with its stereo branch.  ss_triangulate_* above are
 * unchanged and keep treating every row as monocular.  The library's own restatement, as the rest of this family: tests/tri_stereo_ref.py
 * is its normative statement and parity with the real binary stays unpinned; DESIGN.md section 35.  An addition to ABI 5.
 * Per side a depth plane and a right-coordinate plane (float32, each a pointer and a byte stride per row, so ss_stereo_point is read in
 * place with stride 16 at &points[0].depth and &points[0].u_right) and, per pair, one ss_tri_stereo_rig on the HOST: bf1, b1, bf2, b2
 * in double, b upstream's mb in metres and bf = b*fx.  ss_tri_stereo_params holds ss_tri_params as it is and chi2_stereo (upstream:
 * 7.8); ss_tri_params itself stays 32 bytes (deviation from "one new number joins it": the existing struct may not change).
 * The rule of a match, in double like steps 1 - 9 above, one IEEE operation per step:
 *   stereo1 = right1 >= 0 (a NaN is mono), stereo2 likewise.  cos_rays is step 1's cos.  cs1 = cs2 = cos_rays + 1.0; if stereo1:
 *   cs1 = (d*d - h*h)/(d*d + h*h) with d = (double)depth1, h = b1/2.0; ELSE IF stereo2: the same for side 2 (upstream's else is kept:
 *   with both sides stereo only cs1 is formed).  cs = min(cs1, cs2).  Deviation: upstream evaluates cos(2*atan2(mb/2, depth)) in float
 *   through libm; the closed form is the same number in exact arithmetic (tests/test_tri_stereo_ref.py sweeps 2 M pairs).
 *   Mode 0, triangulated: iff cos_rays < cs && cos_rays > 0 && (stereo1 || stereo2 || cos_rays < cos_parallax_max); step 2's DLT
 *   unchanged.  Mode 1: else iff stereo1 && cs1 < cs2; X is the unprojection of the row of keyframe 1 (ss_unproject's step 5 position,
 *   the very function).  Mode 2: else iff stereo2 && cs2 < cs1; the same from keyframe 2.  Else state 1, mode -1.
 *   Steps 3 - 9 as above, except that on a stereo side steps 5 / 6 become ur = u - bf*(1.0/z), er = ur - right,
 *   err = (eu*eu + ev*ev) + er*er, accepted iff err <= chi2_stereo * sigma2.  The map point and its descriptor are the mono form's.
 * With both right planes all -1.0f the states, points and compact blocks are those of ss_triangulate_*, byte for byte.
 * ss_tri_stereo_info per query row: state (as above), mode (-1 .. 2; -1 where no mode was chosen), cos_rays, cs1, cs2, err1_sq,
 * err2_sq as floats (0.0f before their step, a NaN as 0.0f).  ss_tri_stereo_summary: ss_tri_summary, then the state-0 rows per mode. */
typedef struct {          /* 32 bytes, one per pair (a HOST table) */
    double bf1, b1, bf2, b2;
} ss_tri_stereo_rig;
typedef struct {          /* 40 bytes */
    ss_tri_params tri;
    double chi2_stereo;   /* upstream: 7.8 */
} ss_tri_stereo_params;
typedef struct {          /* 32 bytes, one per query row */
    int32_t state, mode;
    float cos_rays, cs1, cs2, err1_sq, err2_sq;
    int32_t reserved;     /* 0 */
} ss_tri_stereo_info;
typedef struct {          /* 80 bytes, one per pair */
    ss_tri_summary tri;
    int32_t n_mode[3];    /* rows of state 0 per mode */
    int32_t reserved;     /* 0 */
} ss_tri_stereo_summary;
/* The n couples (kp1[k], kp2[k]) on the host from the text the kernel compiles; depth and right of each side are float [n], or all
 * four NULL (every row mono).  Needs no device.  Refusals as ss_triangulate_host. */
int ss_triangulate_stereo_host(const ss_epi_pair *pair, const ss_tri_stereo_rig *rig, const ss_tri_stereo_params *tp, const float *scale,
                               int n_levels, const ss_keypoint *kp1, const ss_keypoint *kp2, const float *depth1, const float *right1,
                               const float *depth2, const float *right2, int n, ss_map_point *points, ss_tri_stereo_info *info);
/* ss_triangulate_pairs_device with the planes of both sides: the value of query row i of pair b at d_x1 + (b * rows_per_frame + i) *
 * stride, of train row j at d_x2 + (b * rows_per_frame + j) * stride (strides positive multiples of 4, pointers multiples of 4: else
 * SS_ERR_INVALID_ARG, as for a NULL buffer or table).  rigs: a HOST table of n_frames.  d_info [n_frames][rows_per_frame]
 * ss_tri_stereo_info, d_summary [n_frames] ss_tri_stereo_summary; the compact blocks as ss_triangulate_pairs_device.  Asynchronous. */
int ss_triangulate_stereo_pairs_device(ss_ctx *ctx, const void *d_query, const void *d_query_kp, const void *d_n_query, const void *d_train_kp,
                                       const void *d_n_train, const void *d_idx, int n_frames, int rows_per_frame, const ss_epi_pair *pairs,
                                       const ss_tri_stereo_rig *rigs, const void *d_depth1, int64_t depth1_stride, const void *d_right1,
                                       int64_t right1_stride, const void *d_depth2, int64_t depth2_stride, const void *d_right2,
                                       int64_t right2_stride, const ss_tri_stereo_params *tp, void *d_info, void *d_points, void *d_point_desc,
                                       void *d_point_rows, void *d_n_points, void *d_summary);
/* ss_triangulate_batch_device with one pair of planes [n_frames][kp_capacity] that both sides read: row i of frame f at
 * d_x + (f * kp_capacity + i) * stride. */
int ss_triangulate_stereo_batch_device(ss_ctx *ctx, const int32_t *train_src, const void *d_idx, const ss_epi_pair *pairs,
                                       const ss_tri_stereo_rig *rigs, const void *d_depth, int64_t depth_stride, const void *d_right,
                                       int64_t right_stride, const ss_tri_stereo_params *tp, void *d_info, void *d_points, void *d_point_desc,
                                       void *d_point_rows, void *d_n_points, void *d_summary);

/* ---- map-point fusion: ORBmatcher::Fuse(pKF, vpMapPoints, th) of LocalMapping::SearchInNeighbors, Fuse(pKF, Scw, ...) of
 * LoopClosing::SearchAndFuse and SearchByProjection(pKF, Scw, vpPoints, vpMatched, th, ratioHamming) of the loop and merge
 * candidate check.  Neither upstream source is in the reference tree.  This is the library's own restatement and parity with the
 * real binary stays unpinned, as for the guided, bag-of-words, projection and epipolar stages.  tests/fuse_ref.py is its normative
 * statement; DESIGN.md section 19.  An addition to ABI 5: nothing existing changes ---------------------------------------------
 * - Every float step is one float32 IEEE operation, left to right as written, with no contraction.
 * - Every test is written in its accepting form, so a NaN fails it.
 * Inputs.  Per frame: one ss_proj_view, the struct as it is (an SE3 pose through ss_proj_view_init, a Sim3 through
 * ss_fuse_view_sim3: the kernel never sees a Sim3), and the train side of ss_match_proj_*.  Per map point: one ss_map_point, its
 * descriptor and, optionally, skip[frame][i] (uint8; upstream's isBad(), IsInKeyFrame(pKF) and spAlreadyFound).  Per train row, all
 * optional: right[j] (float), taken[j] (uint8: vpMatched[idx] of the Sim3 SearchByProjection), train_point[j] (int32: the caller's
 * id of the map point the row already carries, < 0 for none).
 * 1. The point.  The state is the number of the first failing test, 0 if none fails.  A rejected point gets floats 0.0f and level
 *    -1.  Rows at or past the count get state -1.
 *    1. State 1: skip is given and is non-zero.
 *    2. State 2: pc = R.P + t, formed as in the projection search.  The test is pc.z > 0.
 *       Deviation: upstream rejects z < 0 only, so a point at z == 0 goes on with an infinite invz.
 *    3. State 3: u and v are formed as in the projection search.  The test is u >= min_x && u < max_x && v >= min_y && v < max_y:
 *       KeyFrame::IsInImage, strict at the upper bound (Frame::isInFrustum of the projection search is closed there).
 *    4. State 4: dist is formed as in the projection search.  The test is dist >= 0.8f*min_dist && dist <= 1.2f*max_dist.
 *    5. State 5: dot = (po.x*nx + po.y*ny) + po.z*nz.  The test is dot >= view_cos_limit * dist.  There is no division, as
 *       upstream's PO.dot(Pn) < 0.5*dist3D.
 *    Then level is the projection search's table rule on max_dist / dist; radius = th * scale[level] (its 2.5 / 4.0 factor does
 *    not apply); u_right = u - bf*invz.
 * 2. Candidates.  A candidate is a train row j < n_train that passes, in this order:
 *    1. max(level-1, 0) <= octave_j <= level.  An octave outside the table is never a candidate (test 4 reads scale[octave_j]; the
 *       projection search accepts octave -1 at level 0).
 *    2. fabsf(x_j - u) < radius && fabsf(y_j - v) < radius.
 *    3. If taken is given, taken[j] == 0.
 *    4. Only when chi2_mono > 0: ex = u - x_j, ey = v - y_j, e2 = ex*ex + ey*ey.  If check_right is set and right[j] >= 0:
 *       er = u_right - right[j], e2 = e2 + er*er and the limit is chi2_stereo; otherwise the limit is chi2_mono.  Accept iff
 *       e2 <= limit * (scale[octave_j]*scale[octave_j]).
 *       Deviation, as in the triangulation: upstream multiplies e2 by invLevelSigma2 and rejects on >.
 *    A Hamming distance is taken only for a row that passed all four; n_candidates counts exactly those rows.
 * 3. Best.  The key is distance << 20 | j; the best is the lowest key; d1 is its distance.  The point names row idx iff
 *    d1 <= th_low.  Deviation: at equal distance upstream keeps the first row in its grid scan order.
 * 4. Outcome, one ss_fuse_action per point.  The rule is order-free; upstream walks the points in sequence and mutates the keyframe
 *    as it goes.
 *      SS_FUSE_NONE       no row named                                                                          other -1
 *      SS_FUSE_REPLACE    train_point is given and train_point[idx] >= 0                                        other = that id
 *      SS_FUSE_ADD        the row is free, and this point holds the lowest d1 << 20 | i among the frame's
 *                         points that name the row                                                              other -1
 *      SS_FUSE_DUPLICATE  the row is free, and another point row w holds the lowest key                         other = w, a
 *                                                                                                   point row of the same block
 *    Deviation: every point that names an occupied row gets REPLACE; where one row has several points, upstream fuses the second
 *    with whatever the first left there.
 *    Deviation: upstream lets the first point in order add and fuses later ones into it; here the closest point adds.
 * Outputs per point row: idx int32 (-1: none); d1 uint16 (0xFFFF: no candidate); ss_fuse_action; ss_fuse_point, 32 bytes.
 * Outputs per frame: ss_fuse_summary, 32 bytes. */
#define SS_FUSE_NONE 0
#define SS_FUSE_ADD 1
#define SS_FUSE_REPLACE 2
#define SS_FUSE_DUPLICATE 3
typedef struct {          /* 32 bytes, one per point row */
    float u, v, u_right, dot, dist, radius;
    int32_t level, state;
} ss_fuse_point;
typedef struct {          /* 8 bytes, one per point row */
    int32_t action, other;
} ss_fuse_action;
typedef struct {          /* 40 bytes */
    float view_cos_limit; /* upstream: 0.5; NaN is SS_ERR_INVALID_ARG */
    float th;             /* finite and > 0; upstream: 3.0 in local mapping, 4.0 in SearchAndFuse, 8 in the candidate check */
    float chi2_mono;      /* upstream: 5.99; not > 0 (zero, negative, NaN): no test 2.4, which is the Sim3 forms */
    float chi2_stereo;    /* upstream: 7.8; must be finite and > 0 when both chi2_mono > 0 and check_right */
    int32_t th_low;       /* 0 .. 256; upstream: 50, or 50*ratioHamming */
    int32_t check_right;  /* test 2.4 uses right[j] */
    int32_t extent_w, extent_h; /* as in ss_proj_params */
    int32_t reserved[2];  /* must be 0 */
} ss_fuse_params;
typedef struct {          /* 32 bytes, one per frame */
    int32_t status;       /* SS_OK, or the frame_error that voided the frame (all rows "none", counts 0) */
    int32_t n_points, n_train;
    int32_t n_in_view;    /* points with state 0 */
    int32_t n_candidates; /* Hamming distances taken */
    int32_t n_add, n_replace, n_duplicate;
} ss_fuse_summary;
/* The view of a camera under upstream's Sim3 Scw = [s.R | t], needs no device.  In double, in this order:
 * s = sqrt((m0*m0 + m1*m1) + m2*m2) of row 0 of srcw; R[k] = srcw[k] / s; t[k] = t[k] / s; then exactly ss_proj_view_init(cam, R, t,
 * bf, out).  SS_ERR_INVALID_ARG if s is not finite or not > 0, or a pointer is NULL.  An SE3 caller uses ss_proj_view_init. */
int ss_fuse_view_sim3(const ss_camera *cam, const double srcw[9], const double t[3], float bf, ss_proj_view *out);
/* Host twins of steps 1 and 2 (the text the kernel compiles, csrc/ss_fuse_steps.h); neither needs a device.  scale: n_levels
 * entries, 1 <= n_levels <= SS_MAX_LEVELS.  p is checked as the device calls check it (SS_ERR_INVALID_ARG).
 * ss_fuse_points_host: out[i] is what the device calls write for point i; skip: n flags, or NULL.
 * ss_fuse_check_host: step 2 of the n couples (points[k], kp[k]) with right[k] (NULL: no row has a right coordinate) and
 * taken[k] (NULL: none is taken); out[k] is 0 for a candidate, else the number 1 .. 4 of the first failing test. */
int ss_fuse_points_host(const ss_proj_view *view, const ss_fuse_params *p, const float *scale, int n_levels, const ss_map_point *points,
                        const uint8_t *skip, int n, ss_fuse_point *out);
int ss_fuse_check_host(const ss_fuse_params *p, const float *scale, int n_levels, const ss_fuse_point *points, const ss_keypoint *kp,
                       const float *right, const uint8_t *taken, int n, uint8_t *out);
/* n_frames frames on caller-supplied device arrays: the arrays, HOST tables (views, point_src) and rules of
 * ss_match_proj_pairs_device, plus d_point_skip (uint8 [n_frames][point_rows], NULL: none) and d_train_point (int32
 * [n_frames][rows_per_frame], NULL: every row is free).  Outputs [n_frames][point_rows]: d_idx (int32), d_d1 (uint16), d_fuse
 * (ss_fuse_action), d_point (ss_fuse_point); d_summary [n_frames] ss_fuse_summary.  SS_ERR_INVALID_ARG: either row count above
 * SS_GUIDED_MAX_ROWS, th not > 0 or not finite, a NaN view_cos_limit, th_low outside 0 .. 256, chi2_stereo not finite or not > 0
 * where it is used, a reserved field that is not 0, a point_src entry outside 0 .. n_blocks - 1, extent_w or extent_h <= 0,
 * check_right without d_train_right, a NULL buffer.  Asynchronous on the context's stream. */
int ss_match_fuse_pairs_device(ss_ctx *ctx, const void *d_points, const void *d_point_desc, const void *d_n_points, int n_blocks,
                               int point_rows, const void *d_point_skip, const void *d_train, const void *d_train_kp,
                               const void *d_n_train, const void *d_train_right, const void *d_train_taken, const void *d_train_point,
                               int n_frames, int rows_per_frame, const ss_proj_view *views, const int32_t *point_src,
                               const ss_fuse_params *p, void *d_idx, void *d_d1, void *d_fuse, void *d_point, void *d_summary);
/* The same, the train side being the frames of the last ss_extract_batch_device batch (SS_ERR_STATE without one; n_frames and
 * kp_capacity are the batch's).  A frame whose frame_error is set gets that status in its summary and all its rows are "none". */
int ss_match_fuse_batch_device(ss_ctx *ctx, const void *d_points, const void *d_point_desc, const void *d_n_points, int n_blocks,
                               int point_rows, const void *d_point_skip, const void *d_train_right, const void *d_train_taken,
                               const void *d_train_point, const ss_proj_view *views, const int32_t *point_src, const ss_fuse_params *p,
                               void *d_idx, void *d_d1, void *d_fuse, void *d_point, void *d_summary);
/* One frame with host pointers in and out (copy in, the pairs form, copy out), synchronous.  n_points, n_train <=
 * SS_GUIDED_MAX_ROWS; point_skip, train_right, train_taken and train_point may be NULL; point may be NULL. */
int ss_match_fuse(ss_ctx *ctx, const ss_proj_view *view, const ss_map_point *points, const uint8_t *point_desc, const uint8_t *point_skip,
                  int n_points, const uint8_t *train, const ss_keypoint *train_kp, int n_train, const float *train_right,
                  const uint8_t *train_taken, const int32_t *train_point, const ss_fuse_params *p, int32_t *idx, uint16_t *d1,
                  ss_fuse_action *fuse, ss_fuse_point *point, ss_fuse_summary *summary);

/* ---- Sim3 from matched map points: Sim3Solver (Horn 1987, RANSAC over 3-point alignments) as LoopClosing::
 * DetectCommonRegionsFromBoW uses it on the matches of SearchByBoW.  The upstream source is not in the reference tree.  This is the
 * library's own restatement and parity with the real binary stays unpinned, as for the guided, bag-of-words, projection, epipolar
 * and fusion stages.  tests/sim3_ref.py is its normative statement; DESIGN.md section 20.  An addition to ABI 5: nothing existing
 * changes ------------------------------------------------------------------------------------------------------------------------
 * - Every float32 step is one IEEE operation, left to right as written, with no contraction; so is every double step of the model.
 * - Every test is written in its accepting form, so a NaN fails it.
 * One pair: keyframe 1 is the query with view v1, keyframe 2 the train with view v2 (ss_proj_view; only rcw, tcw, fx, fy, cx, cy
 * are read).  Every keypoint row of either has an ss_map_point (only x, y, z are read), an ss_keypoint (only octave is read) and,
 * optionally, a skip byte (fusion's convention: non-zero = the row has no usable map point).  idx[i] is the train row matched to
 * query row i, or < 0: what ss_match_bow_pairs_device wrote.
 * 1. Correspondences.  Query rows i < n_query in ascending order; (i, j = idx[i]) is kept iff 0 <= j < n_train, neither row is
 *    skipped and both octaves lie in 0 .. n_levels-1.  The kept ones are numbered 0 .. N-1 in that order.  For each, in float32:
 *    X1 = R1.P1 + t1 and X2 = R2.P2 + t2, each component ((r0*x + r1*y) + r2*z) + t; p = project(X, K): invz = 1.0f / X.z,
 *    u = fx*X.x*invz + cx, v = fy*X.y*invz + cy (two products, then the sum); max1 = chi2 * (s1*s1) with s1 = scale[octave_i],
 *    max2 = chi2 * (s2*s2) with s2 = scale[octave_j].  p1 and p2 are the projections of the map points, not the keypoints, as
 *    upstream has it.
 * 2. State 1: N < 3 or N < min_inliers.  There is no model.
 * 3. Hypothesis t, 0 <= t < max_iterations; each is independent of the others.
 *    a. Draws.  Three draws without replacement over the virtual array 0 .. N-1 under upstream's swap-with-last rule: draw k
 *       (0, 1, 2) takes r = mix32(seed, pair, 3t + k) and j = (uint64(r) * (N - k)) >> 32; the value at slot j is drawn, and slot j
 *       then receives the value at slot N-1-k.  mix32, all in uint32: h = (seed ^ pair*0x9E3779B1) + n*0x85EBCA77; h ^= h >> 16;
 *       h *= 0x7FEB352D; h ^= h >> 15; h *= 0x846CA68B; h ^= h >> 16.  pair is the pair's number in the call.
 *    b. Model, in double from the float32 X1, X2 of the three draws a, b, c in draw order.  O = ((a + b) + c) / 3.0 per component;
 *       Pr = P - O; M[i][j] = (Pr2a[i]*Pr1a[j] + Pr2b[i]*Pr1b[j]) + Pr2c[i]*Pr1c[j].  Horn's symmetric N: N00 = (M00 + M11) + M22,
 *       N01 = M12 - M21, N02 = M20 - M02, N03 = M01 - M10, N11 = (M00 - M11) - M22, N12 = M01 + M10, N13 = M20 + M02,
 *       N22 = (M11 - M00) - M22, N23 = M12 + M21, N33 = (M22 - M00) - M11.  SS_TRI_SWEEPS sweeps of the triangulation's rotation
 *       in its order (0,1) (0,2) (0,3) (1,2) (1,3) (2,3), V starting as the identity.  The quaternion (w, x, y, z) is the column of
 *       V at the LARGEST diagonal entry (strict >, so the first index wins a tie), divided by
 *       sqrt(((w*w + x*x) + y*y) + z*z).  R: r00 = 1 - 2*(y*y + z*z), r01 = 2*(x*y - w*z), r02 = 2*(x*z + w*y),
 *       r10 = 2*(x*y + w*z), r11 = 1 - 2*(x*x + z*z), r12 = 2*(y*z - w*x), r20 = 2*(x*z - w*y), r21 = 2*(y*z + w*x),
 *       r22 = 1 - 2*(x*x + y*y).  P3 = R.Pr2, each component (r0*x + r1*y) + r2*z.  Scale: with d(p, q) = (p0*q0 + p1*q1) + p2*q2,
 *       s = ((d(Pr1a, P3a) + d(Pr1b, P3b)) + d(Pr1c, P3c)) / ((d(P3a, P3a) + d(P3b, P3b)) + d(P3c, P3c)), or exactly 1.0 with
 *       fix_scale.  t12 = O1 - s*(R.O2).  The inverse: s21 = 1.0 / s, sR21[i][j] = s21 * R[j][i], t21[i] = -(s21 * ((R[0][i]*t12[0]
 *       + R[1][i]*t12[1]) + R[2][i]*t12[2])).  s*R, t12, s, s21*R^T, t21 are rounded to float32 once.  If any of these 25 floats
 *       is not finite, the model is the zero model: all 25 are 0.0f (no correspondence passes it: invz is infinite and 0*inf is
 *       NaN).
 *    c. Count, in float32.  Correspondence n is an inlier iff both tests pass: with Y = sR12.X2 + t12 (components as in step 1) and
 *       q = project(Y, K1), e1 = (p1.u - q.u)^2 + (p1.v - q.v)^2 (two products, one sum) and e1 < max1; with Y = sR21.X1 + t21 and
 *       q = project(Y, K2), e2 = (q.u - p2.u)^2 + (q.v - p2.v)^2 and e2 < max2.  There is no depth-sign test, as upstream has
 *       none.  count[t] is an integer.
 * 4. Selection.  The winner is the SMALLEST t with count[t] > min_inliers: the model upstream's iterate returns, since nothing
 *    earlier exceeded the threshold and so it is also the best so far.  State 0: the model, inlier[i] = 1 for the query rows of its
 *    inliers, n_inliers, iteration = t.  State 2, no winner: model and flags all 0, iteration -1.  best_inliers = max count[t] in
 *    states 0 and 2, 0 in state 1.
 * Deviations from upstream: the draw stream (DUtils::Random there); R from the quaternion's nine polynomial entries (upstream goes
 * through atan2 and Rodrigues, the same rotation: atan2, sin and cos are not the same bits on host and device); the model in double
 * (float there); max_iterations is the caller's number (upstream shrinks 300 by log(1 - p) / log(1 - eps^3), and log is not
 * portable bit for bit); one call evaluates every t instead of iterate(20) in a loop with an early exit, which selects the same
 * model; chi2 is a parameter (9.210 there); eigenvectors by cyclic Jacobi (cv::eigen there); a non-finite model is the zero model.
 * Outputs per pair: ss_sim3_result, 128 bytes, and inlier uint8 [rows] by QUERY row (every row < rows is written).  A pair with a
 * frame the extraction flagged has that status, state 1 and no correspondences. */
#define SS_SIM3_MAX_ITERATIONS 1024
typedef struct {          /* 32 bytes */
    float chi2;           /* finite and > 0; upstream: 9.210 */
    int32_t min_inliers;  /* >= 0; a model wins with MORE inliers than this; upstream: 20 */
    int32_t max_iterations; /* 1 .. SS_SIM3_MAX_ITERATIONS; upstream: at most 300 */
    int32_t fix_scale;    /* non-zero: s = 1.0 (stereo and RGB-D) */
    uint32_t seed;
    int32_t reserved[3];  /* must be 0 */
} ss_sim3_params;
typedef struct {          /* 128 bytes, one per pair */
    float sr12[9], t12[3], s12; /* X1 = sr12.X2 + t12 (row-major); all 0.0f unless state == 0 */
    float sr21[9], t21[3];      /* the inverse: X2 = sr21.X1 + t21 */
    int32_t state;        /* 0 a model, 1 too few correspondences, 2 no hypothesis over min_inliers */
    int32_t n_corr;       /* N */
    int32_t n_inliers;    /* state 0: count of the winner, else 0 */
    int32_t best_inliers; /* max count[t]; 0 in state 1 */
    int32_t iteration;    /* the winner's t, or -1 */
    int32_t status;       /* SS_OK, or the frame_error that voided the pair */
    int32_t reserved;     /* 0 */
} ss_sim3_result;
/* Host twins of steps 3b and 3c (the text the kernels compile, csrc/ss_sim3_steps.h); neither needs a device.  p is checked as the
 * device calls check it (SS_ERR_INVALID_ARG).
 * ss_sim3_model_host: the model of the triple x1[k], x2[k] (k = 0, 1, 2 in draw order; float32 camera coordinates) into
 * out->sr12 .. out->t21; state 0, iteration -1, the other integers 0.
 * ss_sim3_check_host: steps 1 and 3c of the n couples (points1[k] with kp1[k] under view1, points2[k] with kp2[k] under view2)
 * against the model in `model`; scale: n_levels entries, 1 <= n_levels <= SS_MAX_LEVELS.  out[k]: 0 an inlier, 1 an octave outside
 * the table (not a correspondence), 2 the first test fails, 3 the second.  err (NULL, or 2n floats): e1, e2 of couple k at
 * err[2k], err[2k + 1]; 0.0f where out[k] == 1. */
int ss_sim3_model_host(const ss_sim3_params *p, const float x1[9], const float x2[9], ss_sim3_result *out);
int ss_sim3_check_host(const ss_sim3_params *p, const ss_proj_view *view1, const ss_proj_view *view2, const float *scale, int n_levels,
                       const ss_map_point *points1, const ss_keypoint *kp1, const ss_map_point *points2, const ss_keypoint *kp2, int n,
                       const ss_sim3_result *model, uint8_t *out, float *err);
/* Closes the chain on the host, needs no device: upstream's gScw = gScm * gSmw, the Sim3 that takes the world of keyframe 2's pose
 * (the loop candidate, rcw2 / tcw2) into the camera of keyframe 1 (the current keyframe), as the view ss_match_fuse_* projects the
 * candidate's map points with.  In double from the result's floats: srcw[9] = sr12 . rcw2 (each entry (a0*b0 + a1*b1) + a2*b2),
 * t[k] = ((sr12[3k]*tcw2[0] + sr12[3k+1]*tcw2[1]) + sr12[3k+2]*tcw2[2]) + t12[k]; then exactly ss_fuse_view_sim3(cam, srcw, t, bf,
 * out).  SS_ERR_INVALID_ARG: a NULL pointer, result->state != 0.  srcw_out (9) and t_out (3) receive the Sim3 when not NULL. */
int ss_sim3_to_view(const ss_camera *cam, const ss_sim3_result *result, const double rcw2[9], const double tcw2[3], float bf,
                    double *srcw_out, double *t_out, ss_proj_view *out);
/* n_pairs pairs on caller-supplied device arrays, pair b = query block b against train block b.  d_query_xyz / d_train_xyz
 * [n_pairs][rows] ss_map_point; d_query_kp / d_train_kp [n_pairs][rows] ss_keypoint; d_query_skip / d_train_skip uint8
 * [n_pairs][rows], or NULL; d_n_query / d_n_train device int32 [n_pairs], clamped to 0 .. rows; d_idx int32 [n_pairs][rows].
 * views1 / views2: HOST tables of n_pairs views each, copied before the call returns.  Outputs: d_inlier uint8 [n_pairs][rows],
 * d_result [n_pairs] ss_sim3_result.  SS_ERR_INVALID_ARG: rows above SS_GUIDED_MAX_ROWS, max_iterations outside
 * 1 .. SS_SIM3_MAX_ITERATIONS, min_inliers < 0, chi2 not finite or not > 0, a reserved field that is not 0, a NULL buffer.
 * Asynchronous on the context's stream. */
int ss_sim3_pairs_device(ss_ctx *ctx, const void *d_query_xyz, const void *d_query_kp, const void *d_query_skip, const void *d_n_query,
                         const void *d_train_xyz, const void *d_train_kp, const void *d_train_skip, const void *d_n_train,
                         const void *d_idx, int n_pairs, int rows, const ss_proj_view *views1, const ss_proj_view *views2,
                         const ss_sim3_params *p, void *d_inlier, void *d_result);
/* The same on the frames of the last ss_extract_batch_device batch (SS_ERR_STATE without one; rows = kp_capacity), frame b against
 * frame train_src[b] (ss_match_guided_batch_device's table; -1: no train, state 1): d_xyz [n_frames][kp_capacity] ss_map_point and
 * d_skip (or NULL) hold the map points of every frame's rows, views (HOST, n_frames) the view of every frame: pair b reads
 * views[b] and views[train_src[b]].  A flagged frame on either side voids the pair. */
int ss_sim3_batch_device(ss_ctx *ctx, const int32_t *train_src, const void *d_xyz, const void *d_skip, const void *d_idx,
                         const ss_proj_view *views, const ss_sim3_params *p, void *d_inlier, void *d_result);
/* One pair with host pointers in and out (copy in, the pairs form, copy out), synchronous.  n_query, n_train <=
 * SS_GUIDED_MAX_ROWS; the skip arrays may be NULL; inlier: n_query bytes. */
int ss_sim3(ss_ctx *ctx, const ss_proj_view *view1, const ss_map_point *query_xyz, const ss_keypoint *query_kp, const uint8_t *query_skip,
            int n_query, const ss_proj_view *view2, const ss_map_point *train_xyz, const ss_keypoint *train_kp, const uint8_t *train_skip,
            int n_train, const int32_t *idx, const ss_sim3_params *p, uint8_t *inlier, ss_sim3_result *result);

/* ---- Pose-only optimisation: Optimizer::PoseOptimization (g2o EdgeSE3ProjectXYZOnlyPose and EdgeStereoSE3ProjectXYZOnlyPose) as
 * TrackWithMotionModel, TrackReferenceKeyFrame, TrackLocalMap and Relocalization run it on the matches of a search, for every frame
 * of a call at once.  It is the rule of ss_track's host step (sst_pose_only) with the stereo row added and the order of every sum
 * fixed.  tests/pose_ref.py is its normative statement; DESIGN.md section 21.  An addition to ABI 5: nothing existing changes, and
 * ss_track keeps calling its host step -----------------------------------------------------------------------------------------
 * - All arithmetic is double.  Every step is one IEEE operation, left to right as written, with no contraction.  The only library
 *   function is sqrt: no transcendental appears, because the device's and the host's differ in the last bits.
 * - Every test is written in its accepting form, so a NaN fails it; the one exception is the step-size test of step 3.
 * One frame: a view (ss_proj_view; only fx, fy, cx, cy, bf are read, widened to double), a start pose of twelve doubles (rcw
 * row-major, then tcw), a block of map points (only x, y, z are read) with an optional skip byte each (fusion's convention: non-zero
 * = no usable map point), keypoint rows (x, y, octave; taken as undistorted) with an optional right coordinate each, and idx.
 * 1. Observations.  Slots i = 0 .. slots-1 in ascending order.  idx_by_row == 0: slots = point_rows, slot i is point row i and
 *    idx[i] its keypoint row (what ss_match_proj_* writes).  idx_by_row == 1: slots = rows_per_frame, slot i is keypoint row i and
 *    idx[i] its point row (what ss_match_bow_* writes, with one map point per train row as for ss_sim3_*).  A slot is an observation
 *    iff the point row is in 0 .. n_points-1, the keypoint row in 0 .. n_kp-1, the point's skip byte (if given) is 0 and the
 *    keypoint's octave lies in 0 .. n_levels-1.  Observations are numbered 0 .. N-1 in slot order.  X, Y, Z, u, v are the float32
 *    inputs widened; w = 1.0 / (s*s) with s = (double)scale[octave].  The observation is stereo iff check_right is set, a right array
 *    is given and right[row] > 0; then ur is widened as well.
 * 2. Start.  n0 = sqrt((r0*r0 + r1*r1) + r2*r2), a = row0 / n0; d = (r3*a0 + r4*a1) + r5*a2; b = row1 - d*a; c = b / sqrt((b0*b0 +
 *    b1*b1) + b2*b2); R = [a; c; a x c] with (a x c)0 = a1*c2 - a2*c1 and so on; t as given.  State 1: N < min_obs.
 * 3. A step.  Each active observation (round 0: every one) with z > 0 contributes; P = R.X + t, each component ((r0*X + r1*Y) +
 *    r2*Z) + t; iz = 1.0 / z, iz2 = iz*iz; up = fx*x*iz + cx; rx = u - up, ry = v - (fy*y*iz + cy);
 *    J0 = {x*y*iz2*fx, -(1.0 + x*x*iz2)*fx, y*iz*fx, -iz*fx, 0, x*iz2*fx}, J1 = {(1.0 + y*y*iz2)*fy, -x*y*iz2*fy, -x*iz*fy, 0, -iz*fy,
 *    y*iz2*fy} (products left to right; the unary minus applies to the first factor).  Stereo adds rr = ur - (up - bf*iz) and
 *    J2 = {J0[0] - bf*y*iz2, J0[1] + bf*x*iz2, J0[2], J0[3], 0, J0[5] - bf*iz2}.  e2 = w*(rx*rx + ry*ry), stereo w*((rx*rx + ry*ry) +
 *    rr*rr).  With delta = sqrt(chi2_mono) (stereo: sqrt(chi2_stereo)) the weight is w*delta / sqrt(e2) in a robust round when
 *    e2 > delta*delta, else w.  With wJ = weight*J entry by entry, the term of H_ab is (wJ0[a]*J0[b] + wJ1[a]*J1[b]) + wJ2[a]*J2[b]
 *    and that of g_a (wJ0[a]*rx + wJ1[a]*ry) + wJ2[a]*rr, a row whose entry a or b is the structural 0 above being left out (H34 has
 *    no term and is 0).  The 26 sums (20 of H's upper triangle, 6 of g): slot s of 256 adds the terms of the active contributing
 *    observations k = s, s + 256, ... in ascending order from +0.0, the others are skipped; each group of 64 consecutive slots is
 *    folded by halving (a[l] += a[l + h], h = 32 .. 1), and the four results combine as (r0 + r1) + (r2 + r3).  Solve: H symmetric,
 *    H_aa += lambda*(1.0 + H_aa), b = -g, Cholesky column by column (s = H_jj - sum of squares in ascending k, L_jj = sqrt(s),
 *    L_ij = (H_ij - sum) / L_jj), forward then backward substitution, as chol6_solve of ss_track.cpp spells it.  A pivot that is not
 *    > 0: state 2, the pose stays the one before the step.  exp(delta), delta = (omega, upsilon): q = (w0*w0 + w1*w1) + w2*w2;
 *    q > pi*pi (the double next to it): state 4, the pose stays; a NaN q passes and ends in step 5.  A = sum (-q)^k / (2k+1)!,
 *    B = sum (-q)^k / (2k+2)!, C = sum (-q)^k / (2k+3)!, k = 0 .. 14, Horner from the last term (acc = acc*(-q) + coefficient; the coefficients are the
 *    doubles next to 1/n!, a table of hex-float literals in csrc/ss_pose_steps.h).  The first term left out is below 2^-60 for
 *    q <= pi*pi.  dR = I + A.W + B.W2 and V = I + B.W + C.W2 with W the cross-product matrix of omega and W2 its square written as
 *    W2_ii = -(the two other squares' sum), W2_ij = wi*wj; a diagonal entry is 1.0 + B*W2_ii, an off-diagonal one B*W2_ij -+ A*wk.
 *    dt_i = (V_i0*u0 + V_i1*u1) + V_i2*u2.  Update: R <- dR.R, t <- dR.t + dt, each entry ((a*b + c*d) + e*f) [+ g].  A round ends
 *    after `iterations` steps, or after a step with every |delta_a| < step_eps.
 * 4. After a round.  The chi-square of every observation, outliers included, under the new pose: z > 0 is required, else 1e30; the
 *    projection is formed with / z (up = fx*x/z + cx; stereo: er = ur - (up - bf/z)); chi2 = w*(ex*ex + ey*ey), stereo
 *    w*((ex*ex + ey*ey) + er*er).  An outlier iff not chi2 <= th, th = chi2_mono or chi2_stereo by kind.  The inliers are the next
 *    round's active observations.  cost is the sum of the inliers' chi-squares in the tree order above.  Fewer than min_obs inliers:
 *    state 3, and the frame stops with the pose it has.  Rounds r < robust_rounds are robust.
 * 5. A pose with an entry that is not finite becomes the orthonormalised start pose with state 2 (the identity and zero, should
 *    that one not be finite either), so no NaN bits reach a result.
 * Outputs per frame: ss_pose_result, 160 bytes.  Per slot one byte: 0 inlier, 1 outlier (mvbOutlier), 2 no observation; the flags
 * are those of the last classification that ran, and all 0 before any (then n_inliers = n_obs and cost = 0).  rcw and tcw feed
 * ss_proj_view_init unchanged.
 * Deviations from upstream: robust_rounds defaults to 2, the host step's value (upstream's loop effectively has 3: it switches the
 * kernel off from its third pass on but optimises before it does); the exponential by series (sin and cos there); lambda and the
 * early end of a round are the host step's (g2o's Levenberg-Marquardt adapts lambda and has its own stop test); a point behind the
 * camera takes no part in a step; the order of every sum is fixed; a step above pi ends the frame; keypoints are taken as
 * undistorted.  Against sst_pose_only: the tree of a sum (four interleaved partial sums there), delta*delta in place of the
 * literal 5.991 on the right of the Huber test, a NaN delta does not end a round, and the stereo row. */
typedef struct {          /* 64 bytes */
    double chi2_mono;     /* finite and > 0; upstream: 5.991 */
    double chi2_stereo;   /* finite and > 0; upstream: 7.815 */
    double lambda;        /* finite and >= 0; the host step: 1e-6 */
    double step_eps;      /* finite and >= 0; the host step: 1e-10; 0 runs every step */
    int32_t n_rounds;     /* 1 .. 8; upstream: 4 */
    int32_t iterations;   /* 1 .. 32; upstream: 10 */
    int32_t robust_rounds; /* 0 .. 8; the host step: 2 */
    int32_t min_obs;      /* >= 3; upstream: 3 */
    int32_t check_right;  /* non-zero: a row with right > 0 is a stereo observation */
    int32_t idx_by_row;   /* 0: idx by point row; 1: idx by keypoint row */
    int32_t reserved[2];  /* must be 0 */
} ss_pose_opt_params;
typedef struct {          /* 160 bytes, one per frame */
    double rcw[9], tcw[3];
    double cost;          /* the sum of the inliers' chi-squares after the last round that ended */
    int32_t state;        /* 0 ok, 1 too few observations, 2 not positive definite, 3 too few inliers, 4 step too large */
    int32_t status;       /* SS_OK, or the frame_error that voided the frame (no observations, state 1) */
    int32_t n_obs, n_stereo, n_inliers;
    int32_t steps[8];     /* steps taken in round r */
    int32_t reserved;     /* 0 */
} ss_pose_result;
/* The whole rule on the host from the text the kernels compile (csrc/ss_pose_steps.h), one frame; needs no device.  start: twelve
 * doubles; scale: n_levels entries, 1 <= n_levels <= SS_MAX_LEVELS; skip and right may be NULL; idx and flags have n_points entries
 * (idx_by_row == 0) or n_kp (idx_by_row == 1).  p is checked as the device calls check it (SS_ERR_INVALID_ARG). */
int ss_pose_opt_host(const ss_proj_view *view, const double *start, const float *scale, int n_levels, const ss_map_point *points,
                     const uint8_t *point_skip, int n_points, const ss_keypoint *kp, const float *right, int n_kp, const int32_t *idx,
                     const ss_pose_opt_params *p, uint8_t *flags, ss_pose_result *result);
/* n_frames frames on caller-supplied device arrays.  Map points as for ss_match_proj_pairs_device: d_points [n_blocks][point_rows]
 * ss_map_point, d_point_skip uint8 [n_blocks][point_rows] or NULL, d_n_points device int32 [n_blocks]; point_src a HOST table
 * [n_frames] of block numbers or NULL (frame b reads block b).  Keypoints: d_kp [n_frames][rows_per_frame] ss_keypoint, d_right float
 * [n_frames][rows_per_frame] or NULL, d_n_kp device int32 [n_frames]; counts are clamped to 0 .. their rows.  d_idx int32 and
 * d_flags uint8 are [n_frames][slots].  views (n_frames) and start_poses (n_frames x 12 doubles) are HOST tables, copied before the
 * call returns.  d_result [n_frames] ss_pose_result.  SS_ERR_INVALID_ARG: either row count above SS_GUIDED_MAX_ROWS, a parameter
 * out of its range, a reserved field that is not 0, a point_src entry outside 0 .. n_blocks - 1, a NULL buffer.  Asynchronous on the
 * context's stream. */
int ss_pose_opt_pairs_device(ss_ctx *ctx, const void *d_points, const void *d_point_skip, const void *d_n_points, int n_blocks,
                             int point_rows, const void *d_kp, const void *d_right, const void *d_n_kp, int n_frames, int rows_per_frame,
                             const void *d_idx, const ss_proj_view *views, const double *start_poses, const int32_t *point_src,
                             const ss_pose_opt_params *p, void *d_flags, void *d_result);
/* The same, the keypoints being the frames of the last ss_extract_batch_device batch (SS_ERR_STATE without one; n_frames and
 * rows_per_frame = kp_capacity are the batch's; d_right is [n_frames][kp_capacity] or NULL).  A frame whose frame_error is set gets
 * that status, state 1 and flag 2 in every slot. */
int ss_pose_opt_batch_device(ss_ctx *ctx, const void *d_points, const void *d_point_skip, const void *d_n_points, int n_blocks,
                             int point_rows, const void *d_right, const void *d_idx, const ss_proj_view *views, const double *start_poses,
                             const int32_t *point_src, const ss_pose_opt_params *p, void *d_flags, void *d_result);
/* One frame with host pointers in and out (copy in, the pairs form, copy out), synchronous.  n_points, n_kp <= SS_GUIDED_MAX_ROWS;
 * point_skip and right may be NULL; idx and flags as for ss_pose_opt_host. */
int ss_pose_opt(ss_ctx *ctx, const ss_proj_view *view, const double *start, const ss_map_point *points, const uint8_t *point_skip,
                int n_points, const ss_keypoint *kp, const float *right, int n_kp, const int32_t *idx, const ss_pose_opt_params *p,
                uint8_t *flags, ss_pose_result *result);

/* ---- Sim3 refinement: the rest of ORBmatcher::SearchBySim3 and Optimizer::OptimizeSim3 (g2o EdgeSim3ProjectXYZ and
 * EdgeInverseSim3ProjectXYZ) as LoopClosing::DetectCommonRegionsFromBoW runs them after the RANSAC, for every loop candidate of a
 * call at once.  The upstream source is not in the reference tree.  This is the library's own restatement and parity with the real
 * binary stays unpinned, as for the Sim3 RANSAC.  tests/sim3opt_ref.py is its normative statement; DESIGN.md section 23.  An
 * addition to ABI 5: nothing existing changes ------------------------------------------------------------------------------------
 * - All arithmetic below step 1 is double.  Every step is one IEEE operation, left to right as written, with no contraction.  The
 *   only library function is sqrt.
 * - Every test is written in its accepting form, so a NaN fails it; the one exception is the rotation's step-size test of step 3.
 * One pair: the arrays ss_sim3_* takes (keyframe 1 the query with view v1, keyframe 2 the train with view v2, idx[i] the train row
 * of query row i), and a start: the ss_sim3_result the RANSAC wrote.  A start with state != 0 or status != SS_OK, or a frame the
 * extraction flagged, gives state 1, no correspondences (flag 2 in every row) and that status (the frame's before the start's).
 * 1. Correspondences.  The keep rule and the numbering 0 .. N-1 of ss_sim3_* step 1.  X1 = R1.P1 + t1 and X2 = R2.P2 + t2 in
 *    float32 exactly as that step spells them, then widened.  The observations are the KEYPOINTS (x, y of query row i and of train
 *    row j, float32 widened, taken as undistorted), not the projections the RANSAC compares.  w1 = 1.0 / (s1*s1) with
 *    s1 = (double)scale[octave_i], w2 likewise from octave_j.
 * 2. Start.  s = sqrt((a0*a0 + a1*a1) + a2*a2) over row 0 of the start's sr12 widened, as ss_fuse_view_sim3 reads a scale; with
 *    fix_scale s is exactly 1.0 and is never updated.  R is the Gram-Schmidt rotation of the pose rule's step 2 on sr12's rows,
 *    t = t12.  An entry that is not finite, or s not > 0: state 2 with R = I, t = 0, s = 1.  State 1: N < min_corr.
 * 3. A step.  Every active correspondence (round 0: every one) contributes up to two edges, e12 first.
 *    e12: Y = s.(R.X2) + t, each component s*((r0*x + r1*y) + r2*z) + t.  It takes part iff Y.z > 0.  With (x, y, z) = Y,
 *    iz = 1.0 / z, iz2 = iz*iz: rx = u1 - (fx1*x*iz + cx1), ry = v1 - (fy1*y*iz + cy1); the rows by (omega, upsilon, sigma) are the
 *    pose rule's J0 and J1 under K1 with a seventh entry: J0 = {x*y*iz2*fx, -(1.0 + x*x*iz2)*fx, y*iz*fx, -iz*fx, 0, x*iz2*fx, 0},
 *    J1 = {(1.0 + y*y*iz2)*fy, -x*y*iz2*fy, -x*iz*fy, 0, -iz*fy, y*iz2*fy, 0}.  Y moves by (-[Y]x, I, Y) and a scale about the
 *    camera centre moves no projection, so the sigma entries are the structural 0.  Here a structural 0 is the factor +0.0 and its
 *    products ARE added.  Weight w1.
 *    e21: M[i][j] = (1.0 / s) * R[j][i]; d = X1 - t; Z[i] = (M[i][0]*d0 + M[i][1]*d1) + M[i][2]*d2.  It takes part iff Z.z > 0.  With
 *    (x, y, z) = Z: rx = u2 - (fx2*x*iz + cx2), ry = v2 - (fy2*y*iz + cy2).  X1 = (a, b, g) moves by E = ([X1]x, -I, -X1), then by M:
 *    D[i] = {M[i][1]*g - M[i][2]*b, M[i][2]*a - M[i][0]*g, M[i][0]*b - M[i][1]*a, -M[i][0], -M[i][1], -M[i][2],
 *    -((M[i][0]*a + M[i][1]*b) + M[i][2]*g)}.  With px = fx2*iz, pxz = fx2*x*iz2, py = fy2*iz, pyz = fy2*y*iz2:
 *    J0[c] = pxz*D[2][c] - px*D[0][c], J1[c] = pyz*D[2][c] - py*D[1][c].  Weight w2.
 *    Per edge: e2 = w*(rx*rx + ry*ry); with delta = sqrt(chi2) the weight is wq = w*delta / sqrt(e2) in the robust round when
 *    e2 > delta*delta, else w.  The term of H_ab (a <= b) is (wq*J0[a])*J0[b] + (wq*J1[a])*J1[b], that of g_a
 *    (wq*J0[a])*rx + (wq*J1[a])*ry.  The 35 sums (28 of H's upper triangle row by row, then 7 of g): slot s of 256 adds, from +0.0,
 *    for its active correspondences k = s, s + 256, ... in ascending order first the e12 term, then the e21 term (an edge that
 *    takes no part is skipped); each group of 64 slots folds by halving and the four results combine as (r0 + r1) + (r2 + r3), the
 *    pose rule's tree.  Solve over n = 7 (with fix_scale the leading 6 x 6 and its 6 of g): H_aa += lambda*(1.0 + H_aa), b = -g,
 *    Cholesky and both substitutions as in the pose rule; a pivot that is not > 0: state 2, the model stays.  Retraction of
 *    delta = (omega, upsilon, sigma): dR from the pose rule's series A and B; |omega|^2 > pi*pi (a NaN passes), or not
 *    |sigma| <= 1.0: state 4, the model stays.  ds = sum sigma^k / k!, k = 0 .. 19, Horner from the last term over the pose rule's
 *    table of 1 / n! (the first term left out, 1 / 20!, is below 2^-60); with fix_scale ds is 1.0 and s is not touched.
 *    R <- dR.R (each entry (a*b + c*d) + e*f), t[i] <- ds*((dR[i][0]*t0 + dR[i][1]*t1) + dR[i][2]*t2) + upsilon[i], s <- ds*s.  A
 *    round ends after its number of steps, or after a step with every |delta_a| < step_eps, a < n.
 * 4. Rounds.  Round 0: iterations0 robust steps on every correspondence.  Then every correspondence is classified: chi2_12 =
 *    w1*(ex*ex + ey*ey) with the projection formed with / z (ex = u1 - (fx1*x/z + cx1)), or 1e30 when Y.z is not > 0; chi2_21
 *    likewise.  It is removed iff not (chi2_12 <= chi2 && chi2_21 <= chi2).  n_removed counts these.  Fewer than min_inliers left:
 *    state 3.  Round 1 is not robust and runs on what is left, iterations_more steps if n_removed > 0, else iterations_same.  The
 *    same test then runs on what round 1 ran on (a removed correspondence stays removed, as upstream has deleted its edges) and
 *    gives n_inliers and the flags.  cost is the sum of the inliers' (chi2_12 + chi2_21) in the tree order above.
 * 5. Result.  s.R, t, s and the inverse are formed and rounded to float32 once as ss_sim3_* step 3b forms them (s21 = 1.0 / s).
 *    If R, t, s or one of these 25 floats is not finite, the result is the start of step 2 with state 2, so no NaN bits reach an
 *    output.  The embedded ss_sim3_result carries the floats and state 0 only when the state is 0; otherwise its floats are all
 *    0.0f and its state is the optimisation's.  ss_sim3_to_view, ss_sim3_to_view21 and a later ss_sim3_opt_* call take it unchanged.
 * Flags, one byte per QUERY row < rows, each written exactly once per call: 0 inlier, 1 removed (upstream's vpMatches1[i] = NULL),
 * 2 no correspondence.  They are those of the last classification that ran, and 0 for every correspondence before any.
 * Deviations from upstream: the left increment is applied by a first-order retraction (g2o: the closed-form Sim3 exponential with
 * sin, cos and exp, which are not the same bits on host and device; a stationary point does not depend on the retraction); analytic
 * Jacobians (g2o differentiates these two edges numerically); lambda and the early end of a round are the pose rule's (g2o's
 * Levenberg-Marquardt adapts lambda); an edge with depth not > 0 takes no part in a step and fails the classification; the order of
 * every sum is fixed; a step above pi or |sigma| above 1 ends the pair; chi2 is a parameter (th2 = 10 there) and so are the step
 * counts; keypoints are taken as undistorted; upstream's bAllPoints / covisibility bookkeeping stays with the caller. */
typedef struct {          /* 64 bytes */
    double chi2;          /* finite and > 0; upstream: th2 = 10 */
    double lambda;        /* finite and >= 0; the pose rule: 1e-6 */
    double step_eps;      /* finite and >= 0; 0 runs every step */
    int32_t iterations0;  /* 1 .. 32; upstream: 5 */
    int32_t iterations_more; /* 1 .. 32, round 1 after a removal; upstream: 10 */
    int32_t iterations_same; /* 1 .. 32, round 1 otherwise; upstream: 5 */
    int32_t min_corr;     /* >= 3; upstream: 10 */
    int32_t min_inliers;  /* >= 0; upstream: 10 */
    int32_t fix_scale;    /* non-zero: s = 1.0 and six unknowns (stereo and RGB-D) */
    int32_t reserved[4];  /* must be 0 */
} ss_sim3_opt_params;
typedef struct {          /* 272 bytes, one per pair */
    double r12[9], t12[3], s12; /* X1 = s12 * r12.X2 + t12 */
    double cost;
    int32_t state;        /* 0 ok, 1 no usable start or too few correspondences, 2 not positive definite or not finite, 3 too few inliers, 4 step too large */
    int32_t status;       /* SS_OK, the frame_error that voided the pair, or the start's status */
    int32_t n_corr, n_removed, n_inliers;
    int32_t steps[2];     /* steps taken in round r */
    int32_t reserved;     /* 0 */
    ss_sim3_result model; /* step 5; iteration -1, best_inliers 0, n_inliers as above in state 0 */
} ss_sim3_opt_result;
typedef struct {          /* 8 bytes, one per pair */
    int32_t n_prior;      /* rows that keep their prior match */
    int32_t n_new;        /* rows that gained a mutual match */
} ss_sim3_mutual_summary;
/* The whole rule on the host from the text the kernels compile (csrc/ss_sim3opt_steps.h), one pair; needs no device.  scale:
 * n_levels entries, 1 <= n_levels <= SS_MAX_LEVELS; the skip arrays may be NULL; idx and flags have n_query entries.  p is checked as
 * the device calls check it (SS_ERR_INVALID_ARG). */
int ss_sim3_opt_host(const ss_proj_view *view1, const ss_proj_view *view2, const float *scale, int n_levels, const ss_map_point *query_xyz,
                     const ss_keypoint *query_kp, const uint8_t *query_skip, int n_query, const ss_map_point *train_xyz,
                     const ss_keypoint *train_kp, const uint8_t *train_skip, int n_train, const int32_t *idx, const ss_sim3_result *start,
                     const ss_sim3_opt_params *p, uint8_t *flags, ss_sim3_opt_result *result);
/* n_pairs pairs on caller-supplied device arrays: every array as for ss_sim3_pairs_device, and d_start, a DEVICE array [n_pairs] of
 * ss_sim3_result (ss_sim3_pairs_device's d_result feeds it unchanged).  Outputs: d_flags uint8 [n_pairs][rows], d_result [n_pairs]
 * ss_sim3_opt_result.  SS_ERR_INVALID_ARG: rows above SS_GUIDED_MAX_ROWS, a parameter out of its range, a reserved field that is
 * not 0, a NULL buffer.  Asynchronous on the context's stream. */
int ss_sim3_opt_pairs_device(ss_ctx *ctx, const void *d_query_xyz, const void *d_query_kp, const void *d_query_skip, const void *d_n_query,
                             const void *d_train_xyz, const void *d_train_kp, const void *d_train_skip, const void *d_n_train,
                             const void *d_idx, int n_pairs, int rows, const ss_proj_view *views1, const ss_proj_view *views2,
                             const void *d_start, const ss_sim3_opt_params *p, void *d_flags, void *d_result);
/* The same on the frames of the last ss_extract_batch_device batch, with train_src, d_xyz, d_skip and views as for
 * ss_sim3_batch_device; d_start [n_frames]. */
int ss_sim3_opt_batch_device(ss_ctx *ctx, const int32_t *train_src, const void *d_xyz, const void *d_skip, const void *d_idx,
                             const ss_proj_view *views, const void *d_start, const ss_sim3_opt_params *p, void *d_flags, void *d_result);
/* One pair with host pointers in and out (copy in, the pairs form, copy out), synchronous.  n_query, n_train <=
 * SS_GUIDED_MAX_ROWS; the skip arrays may be NULL; flags: n_query bytes. */
int ss_sim3_opt(ss_ctx *ctx, const ss_proj_view *view1, const ss_map_point *query_xyz, const ss_keypoint *query_kp, const uint8_t *query_skip,
                int n_query, const ss_proj_view *view2, const ss_map_point *train_xyz, const ss_keypoint *train_kp, const uint8_t *train_skip,
                int n_train, const int32_t *idx, const ss_sim3_result *start, const ss_sim3_opt_params *p, uint8_t *flags,
                ss_sim3_opt_result *result);
/* The bookkeeping of SearchBySim3 around its two searches, which are ss_match_fuse_* called twice.  A match idx[i] is VALID iff
 * i < n_query and 0 <= idx[i] < n_train.
 * Marks: d_skip1_out[i] = (query skip byte of row i != 0) || idx[i] is valid; d_skip2_out[j] = (train skip byte of row j != 0) ||
 * some valid idx[i] == j; a skip array that is NULL reads as 0.  Both are uint8 [n_pairs][rows], every row < rows is written, 0 or 1:
 * the point_skip of the search of one keyframe's points in the other and its train_taken in the other direction.
 * Mutual: d_idx12 [n_pairs][rows] is the train row the search found for query row i, d_idx21 [n_pairs][rows] the query row found for
 * train row j.  d_idx_out[i] = idx[i] if that is valid; else j = idx12[i] iff i < n_query, 0 <= j < n_train, idx21[j] == i and no valid
 * idx[i'] == j; else -1.  Every row < rows is written.  d_summary [n_pairs] ss_sim3_mutual_summary.
 * SS_ERR_INVALID_ARG: rows above SS_GUIDED_MAX_ROWS, a NULL buffer (the skip arrays may be NULL).  Asynchronous. */
int ss_sim3_marks_pairs_device(ss_ctx *ctx, const void *d_idx, const void *d_query_skip, const void *d_train_skip, const void *d_n_query,
                               const void *d_n_train, int n_pairs, int rows, void *d_skip1_out, void *d_skip2_out);
int ss_sim3_mutual_pairs_device(ss_ctx *ctx, const void *d_idx, const void *d_idx12, const void *d_idx21, const void *d_n_query,
                                const void *d_n_train, int n_pairs, int rows, void *d_idx_out, void *d_summary);
/* The same on the frames of the last batch: pair b is frame b against frame train_src[b], d_skip (or NULL) [n_frames][kp_capacity]
 * holds every frame's skip bytes, d_skip2_out[b] and d_idx21[b] go by the rows of pair b's train frame.  A flagged frame on either
 * side leaves the pair no valid match. */
int ss_sim3_marks_batch_device(ss_ctx *ctx, const int32_t *train_src, const void *d_idx, const void *d_skip, void *d_skip1_out,
                               void *d_skip2_out);
int ss_sim3_mutual_batch_device(ss_ctx *ctx, const int32_t *train_src, const void *d_idx, const void *d_idx12, const void *d_idx21,
                                void *d_idx_out, void *d_summary);
/* ss_sim3_to_view in the other direction, for the search of keyframe 1's points in keyframe 2: S21.T1w, the Sim3 that takes the
 * world of keyframe 1's pose (rcw1 / tcw1) into the camera of keyframe 2.  In double from the result's floats: srcw = sr21 . rcw1,
 * t[k] = ((sr21[3k]*tcw1[0] + sr21[3k+1]*tcw1[1]) + sr21[3k+2]*tcw1[2]) + t21[k]; then exactly ss_fuse_view_sim3(cam, srcw, t, bf,
 * out).  SS_ERR_INVALID_ARG: a NULL pointer, result->state != 0. */
int ss_sim3_to_view21(const ss_camera *cam, const ss_sim3_result *result, const double rcw1[9], const double tcw1[3], float bf,
                      double *srcw_out, double *t_out, ss_proj_view *out);

/* ---- Local bundle adjustment: Optimizer::LocalBundleAdjustment (g2o EdgeSE3ProjectXYZ and EdgeStereoSE3ProjectXYZ under a
 * Levenberg-Marquardt loop with the points marginalised) as LocalMapping::Run calls it after the map-building chain, for several
 * local maps (problems) of a call at once.  tests/ba_ref.py is its normative statement; DESIGN.md section 25.  An addition to ABI 5:
 * nothing existing changes.  The upstream source is not in the reference tree: parity with the real binary is unpinned, as for the
 * Sim3 refinement -----------------------------------------------------------------------------------------------------------------
 * - All arithmetic is double.  Every step is one IEEE operation, left to right as written, with no contraction.  The only library
 *   function is sqrt.  Every test is written in its accepting form, so a NaN fails it (the step-size test of ss_pose_exp excepted).
 * - Every sum has one fixed order, so ss_local_ba_host and the kernels agree bit for bit.
 * A call has n_frames keyframes (their keypoint rows with an optional right coordinate each, as for ss_pose_opt_*), blocks of map
 * points (only x, y, z are read) with an optional skip byte each, d_idx int32 [n_frames][point_rows] (idx[f][i]: the keypoint row of
 * point row i in keyframe f, or a negative value: a stack of ss_match_proj_* outputs), and a HOST table of problems.  Problem q owns
 * the keyframes first_frame .. first_frame + n_kf - 1 (k = 0 .. n_kf-1 below) and reads the points of block point_block.  The first
 * n_free keyframes are optimised, the others are fixed (upstream's lFixedCameras) and hold the gauge: n_kf - n_free >= 1.  The frame
 * ranges of the problems of a call do not overlap; two problems may read one block of points.
 * 1. Observations and points.  Point row i is a point iff i < n_points, its skip byte (if given) is 0 and x, y, z are finite.  (k, i)
 *    is an observation iff i is a point, 0 <= idx < n_kp of the keyframe and the keypoint's octave lies in 0 .. n_levels-1; u, v are
 *    the float32 keypoint coordinates widened, w = 1.0 / (s*s) with s = (double)scale[octave]; stereo iff check_right is set, a right
 *    array is given and right[row] > 0.  A point is active iff it has at least min_point_obs observations; the others are flagged 1
 *    and never move.  Start poses go through step 2 of the pose-only optimisation (Gram-Schmidt); one that is not finite gives the
 *    problem state 2 at once.  Points are widened to double.  No active point: state 1.
 * 2. Linearisation of an inlier observation (round 0: every one) of an active point under (R, t) of its keyframe and the point X:
 *    x, y, z, iz, iz2, rx, ry, rr, J0, J1, J2, e2 and the Huber weight are those of step 3 of the pose-only optimisation, term by
 *    term (ss_pose_terms); so are the 26 terms of U_k and g_k.  An observation with z > 0 false takes no part in the step.  The
 *    point Jacobian reuses the translation entries of J: with a3 = J0[3], a5 = J0[5], c4 = J1[4], c5 = J1[5], d5 = J2[5] (a3 =
 *    -iz*fx is minus the entry fx*iz of the projection's Jacobian, a5 = x*iz2*fx minus its entry -fx*x*iz2, and so on: Jp =
 *    -Jproj.R), Jp0[b] = a3*R[b] + a5*R[6+b], Jp1[b] = c4*R[3+b] + c5*R[6+b], Jp2[b] = a3*R[b] + d5*R[6+b], b = 0 .. 2.  With
 *    q = the Huber weight, qJp = q*Jp and qJ = q*J entry by entry (J's structural zeros are +0.0 here), the terms are V_ab =
 *    (qJp0[a]*Jp0[b] + qJp1[a]*Jp1[b]) [+ qJp2[a]*Jp2[b]] for a <= b, b_a = (qJp0[a]*rx + qJp1[a]*ry) [+ qJp2[a]*rr], and
 *    W[a][b] = (qJ0[a]*Jp0[b] + qJ1[a]*Jp1[b]) [+ qJ2[a]*Jp2[b]], a = 0 .. 5, b = 0 .. 2 (the bracket: stereo only).
 * 3. Per active point.  V_i (6 sums) and b_i (3) are added over the contributing observations in ascending k from +0.0, fixed
 *    keyframes included; W_ki is kept for every free k.  V_aa += lambda*(1.0 + V_aa), then the column Cholesky of ss_gn_solve<3>.
 *    Y_ki = W_ki.V_i^-1, each row by the two triangular solves.  A point with a pivot that is not > 0 is frozen for this step: its
 *    observations still contribute U and g, it gets no coupling and its delta is 0.
 * 4. Reduced system, for free k <= l.  The entries of U_k (21: H34 is the structural 0), g_k (6), C_kl = sum_i Y_ki.W_li^T (36; the
 *    21 of the upper triangle on the diagonal; an entry is (Y[a][0]*W[b][0] + Y[a][1]*W[b][1]) + Y[a][2]*W[b][2]) and sum_i Y_ki.b_i
 *    (6, the same form) are each summed over the points i in the tree order of the pose-only optimisation: slot s of 256 adds the
 *    points s, s + 256, ... in ascending order from +0.0, skipping those that do not contribute; each group of 64 slots folds by
 *    halving; the four results combine as (r0 + r1) + (r2 + r3).  U_aa += lambda*(1.0 + U_aa); S_kk = U_k - C_kk, S_kl = 0.0 - C_kl
 *    for k < l, r_k = g_k - sum Y.b, one subtraction per entry.
 * 5. Solve S.dc = -r by Cholesky by columns of order 6*n_free (ss_gn_chol_n and ss_gn_subst_n of csrc/ss_gn_steps.h: the text of
 *    ss_gn_solve for a run-time order).  Every inner sum subtracts in ascending k; since each entry's subtractions are sequential in
 *    k, the rows of a column may be computed in parallel, and a right-looking schedule gives the same bits.  A pivot that is not
 *    > 0: state 2, the problem ends, poses and points stay as before the step.
 * 6. Back-substitution and update.  v = -b_i; for every free k with a contributing observation, ascending: v_b = v_b - (((((W[0][b]*
 *    dc[0] + W[1][b]*dc[1]) + W[2][b]*dc[2]) + W[3][b]*dc[3]) + W[4][b]*dc[4]) + W[5][b]*dc[5]); dp_i = V_i^-1.v by the two
 *    triangular solves; X <- X + dp, entry by entry.  Frozen and inactive points are not touched.  Poses: exp(dc_k) and the update
 *    as in the pose-only optimisation; q > pi*pi in any free keyframe: state 4, the problem ends, nothing moves.
 * 7. Accept or reject: the one place the rule departs from the fixed-lambda steps of the pose-only optimisation, because a coupled
 *    problem needs it.  The cost of a state is the sum over k = 0 .. n_kf-1, ascending from +0.0, of the tree sum over the points i
 *    of the chi-terms of the inlier observations (k, i) of active points: the chi-square of step 4 of the pose-only optimisation
 *    (projection formed with / z; 1e30 when z > 0 is false), and in a robust round e2 <= d*d ? e2 : 2.0*d*sqrt(e2) - d*d with d =
 *    sqrt(chi2_mono) or sqrt(chi2_stereo).  A step is accepted iff every entry of the trial poses and points is finite, its cost is
 *    finite and <= the cost before it; then lambda <- max(lambda / lambda_factor, lambda_min).  Otherwise nothing moves and lambda <-
 *    lambda*lambda_factor.  Either way the step counts as an iteration.  A round ends after iterations[r] steps, or after an accepted
 *    step with every |delta| < step_eps, pose and moved-point entries alike.  The cost before the first step of a round is formed
 *    under that round's inliers and robustness; one that is not finite (an input that is not finite) ends the problem in state 2
 *    with the poses and points it has (in round 0: the start) and the costs recorded before.
 * 8. Rounds r = 0 .. n_rounds-1; r < robust_rounds is robust.  The defaults are ORB-SLAM2's schedule: 5 robust iterations,
 *    classification, then 10 plain iterations on the inliers; ORB-SLAM3's single robust round of 10 is n_rounds = 1, iterations[0] =
 *    10, robust_rounds = 1.  After a round every inlier observation of an active point is classified: an outlier iff not chi2 <= th
 *    (chi2_mono or chi2_stereo by kind; the chi-square of step 7 without the Huber form, so a depth that is not positive is an
 *    outlier).  A removed observation stays removed.  A point left with fewer than min_point_obs inliers becomes inactive (flag 1)
 *    and keeps its place.
 * 9. Non-finite results.  Step 7 accepts no state with an entry that is not finite and step 1 ends a problem whose start poses are
 *    not finite (state 2; such a pose is returned as the identity and zero), so no NaN bits reach a result.
 * Outputs.  Per problem one ss_ba_result, 88 bytes.  Per keyframe of the call twelve doubles (rcw row-major, tcw): fixed keyframes
 * and those of no problem get their orthonormalised start.  Per problem and point row three doubles and one flag byte: 0 optimised,
 * 1 too few observations or inliers, 2 not a point (its doubles are +0.0).  Per (keyframe, point row) one byte: 0 inlier, 1
 * outlier, 2 no observation (every row of a keyframe of no problem).  Every output byte is written exactly once per call.
 * Deviations from upstream: g2o's Levenberg-Marquardt scales lambda by its gain ratio and seeds it from the diagonal, here it is
 * multiplied or divided by lambda_factor from the given start; the exponential by series; a point behind a camera takes no part
 * in a step; the order of every sum is fixed; keypoints are taken as undistorted; no map bookkeeping (the caller erases what the
 * flags name). */
#define SS_BA_MAX_KF 64     /* keyframes of a problem */
#define SS_BA_MAX_FREE 32   /* optimised keyframes of a problem: the reduced system has order 192 at the most */
#define SS_BA_MAX_ROUNDS 4
typedef struct {            /* 16 bytes, one per problem (a HOST table) */
    int32_t first_frame, n_kf, n_free, point_block;
} ss_ba_problem;
typedef struct {            /* 96 bytes */
    double chi2_mono;       /* finite and > 0; upstream: 5.991 */
    double chi2_stereo;     /* finite and > 0; upstream: 7.815 */
    double lambda;          /* the first step's; finite and >= 0; default 1e-4 */
    double lambda_factor;   /* finite and > 1; default 10 */
    double lambda_min;      /* finite and >= 0; default 1e-9 */
    double step_eps;        /* finite and >= 0; default 1e-10; 0 runs every step */
    int32_t n_rounds;       /* 1 .. SS_BA_MAX_ROUNDS; default 2 */
    int32_t iterations[4];  /* each 1 .. 32 for r < n_rounds; default 5, 10 */
    int32_t robust_rounds;  /* 0 .. SS_BA_MAX_ROUNDS; default 1 */
    int32_t min_point_obs;  /* >= 1; default 2 */
    int32_t check_right;    /* non-zero: a row with right > 0 is a stereo observation */
    int32_t reserved[4];    /* must be 0 */
} ss_ba_params;
typedef struct {            /* 88 bytes, one per problem */
    double lambda;          /* after the last step */
    double cost_before;     /* the cost ahead of the first step of round 0 */
    double cost_after;      /* the cost of the state returned, under the inliers and robustness of the last round that ran */
    int32_t state;          /* 0 ok, 1 no active point, 2 not positive definite, or a start pose or a cost that is not finite, 4 step too large */
    int32_t status;         /* SS_OK, or the frame_error that voided the problem (state 1) */
    int32_t n_obs, n_stereo; /* observations of points, active or not; the stereo ones among them */
    int32_t n_inliers;      /* observation bytes that are 0 on return */
    int32_t n_points_active; /* point flags that are 0 on return */
    int32_t n_frozen_max;   /* the most points frozen in one step */
    int32_t steps[4];       /* steps taken in round r, rejected ones included */
    int32_t accepted[4];    /* steps accepted in round r */
    int32_t reserved;       /* 0 */
} ss_ba_result;
/* The whole rule on the host from the text the kernels compile (csrc/ss_ba_steps.h), one problem of n_kf keyframes; needs no device.
 * views, start (n_kf x 12 doubles), n_kp are per keyframe; kp and right (or NULL) are [n_kf][rows_per_frame]; idx and obs_flags
 * [n_kf][n_points]; poses n_kf x 12 doubles, xyz n_points x 3 doubles, point_flags n_points bytes.  p is checked as the device calls
 * check it (SS_ERR_INVALID_ARG). */
int ss_local_ba_host(const ss_proj_view *views, const double *start, int n_kf, int n_free, const float *scale, int n_levels,
                     const ss_map_point *points, const uint8_t *point_skip, int n_points, const ss_keypoint *kp, const float *right,
                     const int32_t *n_kp, int rows_per_frame, const int32_t *idx, const ss_ba_params *p, double *poses, double *xyz,
                     uint8_t *point_flags, uint8_t *obs_flags, ss_ba_result *result);
/* n_problems problems on caller-supplied device arrays: map points, keypoints and d_idx as described above (counts are clamped to
 * 0 .. their rows).  problems (n_problems), views (n_frames) and start_poses (n_frames x 12 doubles) are HOST tables, copied before
 * the call returns.  Outputs: d_poses double [n_frames][12], d_xyz double [n_problems][point_rows][3], d_point_flags uint8
 * [n_problems][point_rows], d_obs_flags uint8 [n_frames][point_rows], d_result [n_problems] ss_ba_result.  SS_ERR_INVALID_ARG: a row
 * count above SS_GUIDED_MAX_ROWS, n_kf outside 1 .. SS_BA_MAX_KF, n_free outside 1 .. SS_BA_MAX_FREE, n_free == n_kf, a frame range
 * outside the call or overlapping another, a point_block outside 0 .. n_blocks - 1, a parameter out of its range, a reserved field
 * that is not 0, a NULL buffer.  Without a frame or without a problem the call returns SS_OK and writes nothing.  The context's
 * workspace for a call is dominated by the points' W and Y blocks: n_problems x F x point_rows x 288 bytes, F being the largest
 * n_free of the call (16 problems of 32 free keyframes and 16 384 rows: 2.4 GB; SS_ERR_NO_MEMORY when it cannot be had), so choose
 * point_rows by the local maps, not by the row limit.  The fixed schedule
 * of every round and iteration is enqueued at once; a problem that has ended costs empty launches.  Asynchronous on the context's
 * stream. */
int ss_local_ba_pairs_device(ss_ctx *ctx, const void *d_points, const void *d_point_skip, const void *d_n_points, int n_blocks,
                             int point_rows, const void *d_kp, const void *d_right, const void *d_n_kp, int n_frames, int rows_per_frame,
                             const void *d_idx, const ss_ba_problem *problems, int n_problems, const ss_proj_view *views,
                             const double *start_poses, const ss_ba_params *p, void *d_poses, void *d_xyz, void *d_point_flags,
                             void *d_obs_flags, void *d_result);
/* The same, the keyframes being the frames of the last ss_extract_batch_device batch (SS_ERR_STATE without one; n_frames and
 * rows_per_frame = kp_capacity are the batch's).  A problem with a frame whose frame_error is set gets that status and state 1. */
int ss_local_ba_batch_device(ss_ctx *ctx, const void *d_points, const void *d_point_skip, const void *d_n_points, int n_blocks,
                             int point_rows, const void *d_right, const void *d_idx, const ss_ba_problem *problems, int n_problems,
                             const ss_proj_view *views, const double *start_poses, const ss_ba_params *p, void *d_poses, void *d_xyz,
                             void *d_point_flags, void *d_obs_flags, void *d_result);
/* One problem with host pointers in and out (copy in, the pairs form, copy out), synchronous; the arguments of ss_local_ba_host. */
int ss_local_ba(ss_ctx *ctx, const ss_proj_view *views, const double *start, int n_kf, int n_free, const ss_map_point *points,
                const uint8_t *point_skip, int n_points, const ss_keypoint *kp, const float *right, const int32_t *n_kp,
                int rows_per_frame, const int32_t *idx, const ss_ba_params *p, double *poses, double *xyz, uint8_t *point_flags,
                uint8_t *obs_flags, ss_ba_result *result);
/* Rounds the points of n problems back into blocks of ss_map_point, so that the next ss_match_proj_* reads them: x, y, z of row i of
 * block block_of[q] (a HOST table, or NULL: block q) become (float) of d_xyz[q][i] wherever d_point_flags[q][i] is not 2; nothing
 * else of the block is written.  SS_ERR_INVALID_ARG: a bad count, a block number outside 0 .. n_blocks - 1, a NULL buffer.
 * Asynchronous. */
int ss_local_ba_points_to_block(ss_ctx *ctx, const void *d_xyz, const void *d_point_flags, int n_problems, int point_rows,
                                const int32_t *block_of, void *d_points, int n_blocks);

/* ---- PnP RANSAC: a pose from 2D-3D matches with no prior, MLPnPsolver (Urban et al. 2016) as Tracking::Relocalization runs it on
 * the matches of SearchByBoW against each relocalisation candidate, for every candidate of a call at once.  The upstream source is
 * not in the reference tree.  This is the library's own restatement and parity with the real binary stays unpinned, as for the Sim3
 * RANSAC.  tests/pnp_ref.py is its normative statement; DESIGN.md section 26.  An addition to ABI 5: nothing existing changes -----
 * - Every step is one IEEE operation, left to right as written, with no contraction: float32 in steps 1 and 3e, double in 3b - 3d.
 * - Every test is written in its accepting form, so a NaN fails it.  Division and sqrt are the only library operations.
 * - Host and device agree bit for bit, for any number of problems in a call and in any order.
 * One problem q: the keypoints of a frame (ss_keypoint; x, y, octave are read; taken as undistorted), a block of ss_map_point (x, y,
 * z are read) with an optional skip byte each (fusion's convention), a camera (fx, fy, cx, cy of an ss_proj_view; nothing else of
 * it is read) and idx[i], the point row matched to keypoint row i, or < 0: what ss_match_bow_pairs_device writes, and
 * ss_pose_opt's idx_by_row = 1 form.
 * 1. Correspondences.  Rows i < n_kp in ascending order; (i, j = idx[i]) is kept iff 0 <= j < n_points, point j is not skipped and
 *    0 <= octave_i < n_levels.  The kept ones are numbered 0 .. N-1 in that order.  Each carries six float32 values: X Y Z of the
 *    point, u v of the keypoint and max = chi2 * (s*s) with s = scale[octave_i]; the model reads s and j of its six as well.
 * 2. State 1: N < 6 or N < min_inliers.  There is no model.
 * 3. Hypothesis t, 0 <= t < max_iterations; each is independent of the others.
 *    a. Draws.  Six draws without replacement over the virtual array 0 .. N-1 under the swap-with-last rule of ss_sim3_* step 3a
 *       with its mix32: draw k (0 .. 5) takes r = mix32(seed, q, 6t + k) and j = (uint64(r) * (N - k)) >> 32; the value at slot j
 *       is drawn, and slot j then receives the value at slot N-1-k.  q is the problem's number in the call.
 *    b. Linear model, in double from the float32 inputs widened.  Bearing of draw i: xn = (u - cx) / fx, yn = (v - cy) / fy,
 *       n = sqrt((xn*xn + yn*yn) + 1.0), b_i = (xn / n, yn / n, 1.0 / n).  O = (((((X0 + X1) + X2) + X3) + X4) + X5) / 6.0 per
 *       component, draws in draw order; d_i = (X_i - O, 1.0).  P_i[r][c] = (r == c ? 1.0 : 0.0) - b_ir*b_ic.  The twelve unknowns
 *       are the columns c1 c2 c3 of R^ and then t^: unknown 3a + r is component r of column a.  Entry (3a + r, 3e + c) of the
 *       symmetric H is the sum over the six draws, in draw order starting from the first term, of (d_ia*d_ie) * P_i[r][c]: the
 *       normal matrix of MLPnP's tangent-plane residuals under identity covariance, which does not depend on the choice of
 *       null-space basis, so none is formed.  trace = ((H00 + H11) + ...) + H_11,11 in ascending order; H_kk += 1e-13 * trace.  One
 *       Cholesky by columns (s = H_jj - the squares in ascending k, L_jj = sqrt(s), L_ij = (H_ij - sum in ascending k) / L_jj); a
 *       pivot that is not > 0 makes the model the zero model.  x starts as twelve times 1.0 / sqrt(12.0); six times: forward then
 *       backward substitution on the factor (each entry subtracts in ascending k, then divides by the diagonal), n =
 *       sqrt(((x0*x0 + x1*x1) + ...) + x11*x11), x_k = x_k / n.  The count is fixed; there is no convergence test.  Sign: with
 *       y_i[r] = ((x[r]*d_i0 + x[3+r]*d_i1) + x[6+r]*d_i2) + x[9+r] and f_i = (b_i0*y_i0 + b_i1*y_i1) + b_i2*y_i2, if
 *       ((((f_0 + f_1) + f_2) + f_3) + f_4) + f_5 < 0 all twelve are negated.  Scale: n_a = sqrt((x[3a]*x[3a] + x[3a+1]*x[3a+1]) +
 *       x[3a+2]*x[3a+2]), s = 3.0 / ((n_0 + n_1) + n_2).  R is the rotation nearest to R^: Horn's quaternion exactly as ss_sim3_*
 *       step 3b has it (N, SS_TRI_SWEEPS sweeps, the largest diagonal entry, the nine polynomial entries) with M[i][j] = x[3i + j],
 *       the columns of R^ as Pr1 against the unit vectors as Pr2; it is always a proper rotation.  tcw[r] = s*x[9+r] -
 *       ((R[r][0]*O0 + R[r][1]*O1) + R[r][2]*O2).
 *    c. Refinement on the six: refine_steps plain (non-robust) steps of ss_pose_opt_* step 3 with its own functions: each draw an
 *       observation with w = 1.0 / (s*s) and no right coordinate; each of the 26 sums starts at +0.0 and adds the terms of the draws
 *       with z > 0 in draw order; the solve with `lambda`, the exponential and the update as there.  A step the pose rule refuses
 *       (a pivot not > 0, a step above pi) or that leaves an entry not finite ends the refinement; the hypothesis keeps the pose it
 *       had before that step.  A model that is already the zero model by (d) is not refined.
 *    d. The record.  rcw and tcw in double, and rounded to float32 once.  If any of the twelve floats is not finite, the Cholesky
 *       met a pivot not > 0, the linear pose has an entry that is not finite, or two of the six share a point row, the model is
 *       the zero model, all 0: no correspondence passes it.
 *    e. Count, in float32.  Y = R.X + t, each component ((r0*X + r1*Y) + r2*Z) + t; correspondence n is an inlier iff Y.z > 0 and,
 *       with invz = 1.0f / Y.z, qu = fx*Y.x*invz + cx, qv = fy*Y.y*invz + cy (two products, then the sum),
 *       (u - qu)*(u - qu) + (v - qv)*(v - qv) < max.  count[t] is an integer.
 * 4. Selection.  The winner is the hypothesis with the LARGEST count, the smallest t among equals; it must also satisfy
 *    count >= min_inliers and (float)count >= min_ratio * (float)N.  State 0: the double model, inlier[i] = 1 for the keypoint
 *    rows of its inliers, n_inliers, iteration = t.  State 2, the best hypothesis does not qualify: model and flags all 0,
 *    iteration -1.  best_inliers = max count[t] in states 0 and 2, 0 in state 1.
 * Deviations from upstream: the draw stream (DUtils::Random there); no covariance (identity); no planar branch (upstream switches
 * to nine unknowns only when the points' scatter has rank exactly 2; a planar set here gives an arbitrary finite model, or the zero
 * model, that the count votes down); the scale is the mean of the column norms (a cube root through pow there); the rotation comes
 * from Horn's quaternion (an SVD there); the refinement minimises pixel error with the pose rule's step (five Gauss-Newton steps on
 * tangent-plane residuals there); every hypothesis is evaluated and the best is taken (upstream runs iterate(5) in a loop with an
 * early exit at the first hypothesis over the threshold whose Refine() holds); there is no final refit over all inliers: the
 * ss_pose_opt_* call that follows does that job from result.rcw / tcw; the smallest eigenvector by inverse iteration on a shifted
 * Cholesky factor (an SVD there); max_iterations is the caller's number.
 * Outputs per problem: ss_pnp_result, 128 bytes, and inlier uint8 [rows] by KEYPOINT row (every row < rows is written).  A problem
 * whose keypoint frame the extraction flagged has that status, state 1 and no correspondences. */
#define SS_PNP_MAX_ITERATIONS 1024
#define SS_PNP_MAX_REFINE 16
typedef struct {            /* 40 bytes */
    float chi2;             /* finite and > 0; upstream: 5.991 */
    float min_ratio;        /* finite and >= 0; upstream: 0.5; 0 switches the test off */
    double lambda;          /* finite and >= 0; the pose rule's: 1e-6 */
    int32_t min_inliers;    /* >= 0; upstream: 10 */
    int32_t max_iterations; /* 1 .. SS_PNP_MAX_ITERATIONS; upstream: 300 */
    int32_t refine_steps;   /* 0 .. SS_PNP_MAX_REFINE; upstream: 5 */
    uint32_t seed;
    int32_t reserved[2];    /* must be 0 */
} ss_pnp_params;
typedef struct {            /* 128 bytes, one per problem */
    double rcw[9], tcw[3];  /* all 0.0 unless state == 0; feed ss_proj_view_init and ss_pose_opt_*'s start unchanged */
    int32_t state;          /* 0 a model, 1 too few correspondences, 2 the best hypothesis does not qualify */
    int32_t status;         /* SS_OK, or the frame_error that voided the problem */
    int32_t n_corr;         /* N */
    int32_t n_inliers;      /* state 0: count of the winner, else 0 */
    int32_t best_inliers;   /* max count[t]; 0 in state 1 */
    int32_t iteration;      /* the winner's t, or -1 */
    int32_t reserved[2];    /* 0 */
} ss_pnp_result;
/* Host twins (the text the kernels compile, csrc/ss_pnp_steps.h); none needs a device.  p is checked as the device calls check it
 * (SS_ERR_INVALID_ARG); scale: n_levels entries, 1 <= n_levels <= SS_MAX_LEVELS.
 * ss_pnp_host: the whole rule for one problem whose number in the call is `problem`; point_skip may be NULL; idx and inlier have
 * n_kp entries.
 * ss_pnp_model_host: steps 3b - 3d of one sextuple in draw order: xyz 18 floats, uv 12 floats, scale6 the six keypoints' scales,
 * point_rows6 their point rows, into out->rcw / tcw; state 0, iteration -1, the other integers 0.
 * ss_pnp_check_host: steps 1 and 3e of the n couples (points[k] with kp[k]) against the pose in `model`, rounded to float32 as step
 * 3d rounds it.  out[k]: 0 an inlier, 1 an octave outside the table (not a correspondence), 2 the depth is not > 0, 3 the error
 * is not < max.  err (NULL, or n floats): the squared error, 0.0f where out[k] is 1 or 2. */
int ss_pnp_host(const ss_proj_view *view, const float *scale, int n_levels, const ss_map_point *points, const uint8_t *point_skip,
                int n_points, const ss_keypoint *kp, int n_kp, const int32_t *idx, const ss_pnp_params *p, int problem, uint8_t *inlier,
                ss_pnp_result *result);
int ss_pnp_model_host(const ss_pnp_params *p, const ss_proj_view *view, const float *xyz, const float *uv, const float *scale6,
                      const int32_t *point_rows6, ss_pnp_result *out);
int ss_pnp_check_host(const ss_pnp_params *p, const ss_proj_view *view, const float *scale, int n_levels, const ss_map_point *points,
                      const ss_keypoint *kp, int n, const ss_pnp_result *model, uint8_t *out, float *err);
/* n_problems problems on caller-supplied device arrays.  Map points as for ss_pose_opt_pairs_device: d_points [n_blocks][point_rows]
 * ss_map_point, d_point_skip uint8 [n_blocks][point_rows] or NULL, d_n_points device int32 [n_blocks].  Keypoints: d_kp
 * [n_kp_frames][rows_per_frame] ss_keypoint, d_n_kp device int32 [n_kp_frames]; counts are clamped to 0 .. their rows.  kp_src and
 * point_src: HOST tables [n_problems] of frame and block numbers, or NULL (problem q reads frame q, block q): several candidate
 * keyframes of one lost frame are several problems that share one keypoint frame, with no copies.  d_idx int32 and d_inlier uint8
 * are [n_problems][rows_per_frame].  views (n_problems) is a HOST table, copied before the call returns.  d_result [n_problems]
 * ss_pnp_result.  SS_ERR_INVALID_ARG: either row count above SS_GUIDED_MAX_ROWS, a parameter out of its range, a reserved field
 * that is not 0, a kp_src or point_src entry out of range, a NULL buffer.  Asynchronous on the context's stream. */
int ss_pnp_pairs_device(ss_ctx *ctx, const void *d_points, const void *d_point_skip, const void *d_n_points, int n_blocks, int point_rows,
                        const void *d_kp, const void *d_n_kp, int n_kp_frames, int rows_per_frame, const void *d_idx, int n_problems,
                        const ss_proj_view *views, const int32_t *kp_src, const int32_t *point_src, const ss_pnp_params *p,
                        void *d_inlier, void *d_result);
/* The same, the keypoints being the frames of the last ss_extract_batch_device batch (SS_ERR_STATE without one; n_kp_frames and
 * rows_per_frame = kp_capacity are the batch's).  A problem whose keypoint frame has its frame_error set gets that status, state 1
 * and no correspondences. */
int ss_pnp_batch_device(ss_ctx *ctx, const void *d_points, const void *d_point_skip, const void *d_n_points, int n_blocks, int point_rows,
                        const void *d_idx, int n_problems, const ss_proj_view *views, const int32_t *kp_src, const int32_t *point_src,
                        const ss_pnp_params *p, void *d_inlier, void *d_result);
/* One problem (number 0) with host pointers in and out (copy in, the pairs form, copy out), synchronous.  n_points, n_kp <=
 * SS_GUIDED_MAX_ROWS; point_skip may be NULL; idx and inlier have n_kp entries. */
int ss_pnp(ss_ctx *ctx, const ss_proj_view *view, const ss_map_point *points, const uint8_t *point_skip, int n_points,
           const ss_keypoint *kp, int n_kp, const int32_t *idx, const ss_pnp_params *p, uint8_t *inlier, ss_pnp_result *result);

/* ---- Two-view initialisation: TwoViewReconstruction::Reconstruct as Tracking::MonocularInitialization runs it on the matches of
 * SearchForInitialization (ss_match_guided_*): homography and fundamental-matrix RANSAC, the model choice, the decomposition and
 * CheckRT, for every initialising pair of a call at once.  The upstream source is not in the reference tree.  This is the library's
 * own restatement from the published algorithm and from the host form inside the bounded tracker (sst_two_view, which keeps its own
 * draw stream and is not replaced); parity with the real binary stays unpinned, as for the Sim3 and PnP RANSAC.  tests/two_view_ref.py is
 * its normative statement; csrc/ss_two_view_steps.h is the text kernels and host twins compile; DESIGN.md section 30.  An addition to ABI 5: nothing
 * existing changes -------------------------------------------------------------------------------------------------------------
 * - All arithmetic is double on the float32 coordinates widened.  Every step is one IEEE operation, left to right as written, with
 *   no contraction.  Every test is written in its accepting form, so a NaN fails it.  Division and sqrt are the only library
 *   operations (no acos: the parallax tests are on cosines).
 * - Host and device agree bit for bit, for any number of problems in a call and in any order.
 * One problem q: the keypoints of two frames (ss_keypoint; x, y of both and the octave of frame 1 are read; taken as undistorted),
 * idx[i], the row of frame 2 matched to row i of frame 1, or < 0 (what ss_match_guided_* writes), and one camera for both frames
 * (fx, fy, cx, cy of an ss_proj_view; nothing else of it is read).
 * 1. Correspondences.  Rows i < n1 in ascending order; (i, j = idx[i]) is kept iff 0 <= j < n2 and 0 <= octave_i < n_levels (the
 *    map point's distance range reads that scale).  The kept ones are numbered 0 .. N-1 in that order; each is four float32 values
 *    u1 v1 u2 v2.  N < 8: state 1.
 * 2. Normalisation, per coordinate c of the four: m_c = sum(x) / N, d_c = sum(|x - m_c|) / N.  A sum over the correspondences is
 *    THE TREE: chunks of 256 consecutive correspondences (absent terms +0.0); in a chunk each group of 64 is folded by halving
 *    (a[l] += a[l + h], h = 32 .. 1) and the four group results are combined as (g0 + g1) + (g2 + g3) (ss_gn_tree); the chunk sums
 *    are added in ascending order starting from the first.  A d_c that is not > 0, or a d_c or m_c that is not finite: state 2.
 *    s_c = 1.0 / d_c, the normalised coordinate is (x - m_c) * s_c, T = [[sx, 0, -mx*sx], [0, sy, -my*sy], [0, 0, 1]] per image and
 *    T2^-1 = [[dx, 0, mx], [0, dy, my], [0, 0, 1]] in closed form.
 * 3. Hypothesis t, 0 <= t < max_iterations: eight draws without replacement by the swap-with-last rule of ss_sim3_* step 3a with
 *    eight values of the stream per hypothesis (ss_sim3_draw_k<8>(seed, q, t, N)); H and F share them.
 *    H: each draw gives the rows ra = (0, 0, 0, -u1, -v1, -1, v2*u1, v2*v1, v2) and rb = (u1, v1, 1, 0, 0, 0, -(u2*u1), -(u2*v1),
 *    -u2); entry (i, j), i >= j, of the 9 x 9 normal matrix is the sum over the draws, in draw order from the first term, of
 *    ra_i*ra_j + rb_i*rb_j.  F: one row (u2*u1, u2*v1, u2, v2*u1, v2*v1, v2, u1, v1, 1) per draw, entry (i, j) the sum of r_i*r_j.
 *    The null vector of either as ss_pnp_* step 3b finds its own at order 12: trace in ascending order, 1e-13 * trace added to the
 *    diagonal, one Cholesky by columns, x = nine times 1.0 / 3.0, six inverse iterations each followed by x / sqrt(the sequential
 *    sum of squares); no convergence test.  F is then projected to rank 2: G = F^T.F (entry (i, j) = (F0i*F0j + F1i*F1j) +
 *    F2i*F2j), eight sweeps of cyclic Jacobi over (0,1) (0,2) (1,2) with the rotation of ss_triangulate_* step 2, v the column of
 *    the smallest diagonal entry (the first among equals), F[r][c] -= ((F[r][0]*v0 + F[r][1]*v1) + F[r][2]*v2) * v[c].  H21 =
 *    (T2^-1.Hn).T1, H12 = adj(H21) * (1.0 / det), F21 = (T2^T.Fn).T1, every product entry (a0*b0 + a1*b1) + a2*b2.  A model is the
 *    zero model, of score -1, when an entry is not finite, a pivot was not > 0, |det H21| is not > 1e-300 (H only) or two of the
 *    eight draws coincide.
 * 4. Score over all N correspondences, sigma = 1.  H: with x2 carried into image 1 by H12 and x1 into image 2 by H21 (w = 1.0 /
 *    ((h6*u + h7*v) + h8), then each coordinate times w), chi_a and chi_b the two squared distances; F: chi_a = num^2 / (a^2 + b^2)
 *    of x2 against the line F.x1, chi_b of x1 against F^T.x2.  A term is accepted iff chi <= chi2_h (chi2_f); the correspondence
 *    contributes (chi_a accepted ? th - chi_a : 0.0) + (chi_b accepted ? th - chi_b : 0.0) with th = chi2_h for H and chi2_score
 *    for F, and is an inlier iff both are accepted.  The score is the tree of step 2 over these contributions.
 * 5. Selection, per model: the LARGEST score, the smallest t among equals.  Neither score > 0: state 2.
 * 6. Model choice.  RH = h / (h + f), h and f the two scores, one that is not > 0 taken as 0.0; the homography iff RH >
 *    rh_threshold.  The winner's inlier flags are computed once more; N_in is their count.  N_in < 8: state 3, reason 2.
 * 7. Decomposition in double.  The 3 x 3 SVD: the eigenvalues of A^T.A by the Jacobi of step 3, sorted descending (among equals the
 *    smaller index first), sigma = sqrt (0.0 when the eigenvalue is not > 0); columns 0 and 1 of U are A.v over its length,
 *    column 2 their cross product, negated when its product with A.v2 is < 0.  F: E = (K^T.F).K, t = column 2 of U over its
 *    length, R1 = (U.W).V^T, R2 = (U.W^T).V^T, each negated when its determinant is < 0; the four hypotheses (R1, t) (R2, t)
 *    (R1, -t) (R2, -t).  H: A = (K^-1.H).K, refused (state 3, reason 1) unless d1/d2 >= 1.00001 and d2/d3 >= 1.00001; Faugeras and
 *    Lustman's eight in the order of ReconstructH, R = s.(U.R').V^T with s = det U * det V^T, t = U.t' over its length.
 * 8. CheckRT of every hypothesis over the winner's inliers.  a = (u - cx) / fx, b = (v - cy) / fy for both images; the DLT rows
 *    (-1, 0, a1, 0), (0, -1, b1, 0), a2*P2[2] - P2[0], b2*P2[2] - P2[1] with P2 = [R | t]; the smallest eigenvector of the 4 x 4
 *    exactly as ss_triangulate_* step 2; X = v / v3.  The point is good iff v3 is finite and not 0, X is finite, cos = (X.n2) /
 *    (|X| * |n2|) with n2 = X + R^T.t is finite, (X.z > 0 or cos >= 0.99998), (Y.z > 0 or cos >= 0.99998) with Y = R.X + t, and
 *    both squared reprojection errors ((fx*X.x) / X.z + cx) - u ... are <= 4.0.  n_good counts them; a good point is triangulated
 *    iff cos < 0.99998.  The best hypothesis is the first with the largest n_good; its parallax cosine is the element at index
 *    min(50, n_good - 1) of its good points' cosines in ascending order (an order statistic: -0.0 orders below +0.0).
 * 9. Acceptance, in this order.  F: n_good >= max((int)(0.9 * N_in), min_triangulated), else reason 2; at most one hypothesis with
 *    n_good > 0.7 * best, else reason 3; cos < cos_min_parallax, else reason 4.  H: n_good > min_triangulated and n_good > 0.9 *
 *    N_in, else reason 2; second < 0.75 * best, else reason 3; cos <= cos_min_parallax, else reason 4.  Anything refused: state 3.
 * 10. Outputs.  ss_two_view_result per problem; flag uint8 per row of frame 1 (every row < rows is written): 0 not a
 *    correspondence, 1 an outlier of the chosen model, 2 an inlier that is not triangulated, 3 triangulated.  The triangulated
 *    points in ascending query row as ss_map_point (frame 1 the world; x y z; the normal (X/|X| + n2/|n2|) / 2.0; max_dist = |X| *
 *    scale[octave_i], min_dist = max_dist / scale[n_levels - 1]; each rounded to float32 once), their rows (int32 i, j) and their
 *    count, in the layout ss_triangulate_* writes; rows from n_points on are not written.  In states 1 - 3 r21 and t21 are all
 *    0.0, no flag exceeds 1 and there are no points; the scores, iterations, model, N_in, n_good and cos_parallax keep what the
 *    rule reached.
 * Deviations from upstream: the draw stream (DUtils::Random there); a match whose reference keypoint has an octave outside the
 * pyramid table is no correspondence (upstream takes every match: N can be below the count of valid idx entries);
 * inverse iteration and Jacobi where upstream calls cv::SVD;
 * triangulation in normalised coordinates; cosines instead of degrees (cos_min_parallax is cos 1 degree); rh_threshold is a
 * parameter (upstream's source has 0.50, ss_track 0.45); every hypothesis is scored, as upstream does; a NaN fails every test. */
#define SS_TWO_VIEW_MAX_ITERATIONS 1024
#define SS_TWO_VIEW_COS_1DEG 0.9998476951563913 /* cos(1 degree) */
typedef struct {               /* 64 bytes */
    double chi2_h;             /* finite and > 0; upstream: 5.991 */
    double chi2_f;             /* finite and > 0; upstream: 3.841 */
    double chi2_score;         /* finite and > 0; upstream: 5.991 */
    double rh_threshold;       /* 0 .. 1; upstream: 0.50, ss_track: 0.45 */
    double cos_min_parallax;   /* -1 .. 1; upstream: SS_TWO_VIEW_COS_1DEG */
    int32_t min_triangulated;  /* >= 0; upstream: 50 */
    int32_t max_iterations;    /* 1 .. SS_TWO_VIEW_MAX_ITERATIONS; upstream: 200 */
    uint32_t seed;
    int32_t reserved[3];       /* must be 0 */
} ss_two_view_params;
typedef struct {               /* 192 bytes, one per problem */
    double r21[9], t21[3];     /* all 0.0 unless state == 0; X2 = r21.X1 + t21, |t21| = 1; feed ss_proj_view_init unchanged */
    double score_h, score_f;   /* the best scores; -1.0 when every model was the zero model; 0.0 in state 1 and when step 2 fails */
    double cos_parallax;       /* of the best hypothesis; 0.0 when there was none */
    int32_t state;             /* 0 a map, 1 too few correspondences, 2 no model, 3 the reconstruction was refused */
    int32_t reason;            /* state 3: 1 singular values, 2 too few good points, 3 ambiguous, 4 low parallax; else 0 */
    int32_t status;            /* SS_OK, or the frame_error that voided the problem */
    int32_t model;             /* 1 F, 2 H, 0 none */
    int32_t iteration_h, iteration_f; /* the winners' t, or -1 */
    int32_t n_corr;            /* N */
    int32_t n_inliers;         /* N_in of the chosen model */
    int32_t n_good;            /* of the best hypothesis */
    int32_t n_triangulated;    /* state 0: the points written */
    int32_t reserved[8];       /* 0 */
} ss_two_view_result;
/* Host twins (the text the kernels compile); none needs a device.  p is checked as the device calls check it (SS_ERR_INVALID_ARG).
 * ss_two_view_host: the whole rule for one problem whose number in the call is `problem`; scale: n_levels entries; idx and flag
 * have n_kp1 entries; points and point_rows (2 int32 each) have room for n_kp1 entries; *n_points is written.
 * ss_two_view_model_host: steps 2 and 3 for one octuple: uv 8 x 4 floats (u1 v1 u2 v2) in draw order, normalised by their own mean
 * and deviation (N = 8, the draws 0 .. 7); h21, h12, f21: nine doubles each, all 0.0 for a zero model; ok[2]: H, F.
 * ss_two_view_check_host: steps 4 and 8 of n correspondences (uv n x 4 floats).  Any of h21 + h12, f21, r21 + t21 may be NULL with
 * its outputs: chi_h / chi_f (2 doubles each per correspondence) and in_h / in_f (uint8), score_h / score_f (the tree); good
 * (uint8: 0 not good, 1 good, 2 triangulated), cosv and xyz (3 doubles) under (r21, t21) and the camera of `view`.
 * ss_two_view_accept_host: steps 8 and 9 on counts: good[n_hyp] (n_hyp 1 .. 8) the hypotheses' n_good, model 1 or 2, N_in and the best
 * hypothesis' parallax cosine -> out[0] the reason (0: accepted), out[1] the best hypothesis (-1: none), out[2] its count, out[3] the
 * second count.  ss_two_view_beats_host: step 5's order, 1 iff (score, t) beats (best, best_t).  ss_two_view_point_tests_host: the
 * three tests of step 8 on given numbers: out[0] cos < 0.99998 (triangulated), out[1] cos >= 0.99998 (exempt from the depth tests),
 * out[2] err_sq <= 4.0. */
int ss_two_view_host(const ss_proj_view *view, const float *scale, int n_levels, const ss_keypoint *kp1, int n_kp1, const ss_keypoint *kp2,
                     int n_kp2, const int32_t *idx, const ss_two_view_params *p, int problem, uint8_t *flag, ss_map_point *points,
                     int32_t *point_rows, int32_t *n_points, ss_two_view_result *result);
int ss_two_view_model_host(const float *uv, double *h21, double *h12, double *f21, int32_t *ok);
int ss_two_view_check_host(const ss_two_view_params *p, const ss_proj_view *view, const float *uv, int n, const double *h21, const double *h12,
                           const double *f21, const double *r21, const double *t21, double *chi_h, uint8_t *in_h, double *score_h,
                           double *chi_f, uint8_t *in_f, double *score_f, uint8_t *good, double *cosv, double *xyz);
int ss_two_view_accept_host(const ss_two_view_params *p, int model, const int32_t *good, int n_hyp, int n_in, double cos_parallax,
                            int32_t *out);
int ss_two_view_beats_host(double score, int t, double best, int best_t);
int ss_two_view_point_tests_host(double cos_parallax, double err_sq, int32_t *out);
/* n_problems problems on caller-supplied device arrays.  d_kp1 [n_frames1][rows_per_frame] and d_kp2 [n_frames2][rows_per_frame]
 * ss_keypoint with their device int32 counts (clamped to 0 .. rows); kp1_src and kp2_src: HOST tables [n_problems] of frame
 * numbers, or NULL (problem q reads frame q): one reference frame tried against several current frames is several problems that
 * share it, with no copies.  d_idx int32 and d_flag uint8 are [n_problems][rows_per_frame]; views (n_problems) is a HOST table,
 * copied before the call returns.  d_points (ss_map_point) and d_point_rows (2 int32) are [n_problems][rows_per_frame], d_n_points
 * int32 [n_problems], d_result [n_problems] ss_two_view_result.  SS_ERR_INVALID_ARG: rows above SS_GUIDED_MAX_ROWS, a parameter out
 * of its range, a reserved field that is not 0, a source entry out of range, a NULL buffer.  Asynchronous on the context's stream. */
int ss_two_view_pairs_device(ss_ctx *ctx, const void *d_kp1, const void *d_n_kp1, int n_frames1, const void *d_kp2, const void *d_n_kp2,
                             int n_frames2, int rows_per_frame, const void *d_idx, int n_problems, const ss_proj_view *views,
                             const int32_t *kp1_src, const int32_t *kp2_src, const ss_two_view_params *p, void *d_flag, void *d_points,
                             void *d_point_rows, void *d_n_points, void *d_result);
/* The same, both sides being frames of the last ss_extract_batch_device batch (SS_ERR_STATE without one; n_problems is the batch's
 * frame count and rows_per_frame its kp_capacity): problem q has frame q as its frame 1 and frame train_src[q] as its frame 2
 * (train_src: a HOST table, or NULL: frame q - 1; -1, and frame 0 under NULL: no frame 2, so no correspondences and state 1), as in
 * ss_match_guided_batch_device, whose d_idx it reads.  A problem with a frame whose frame_error is set gets that status, state 1 and
 * no correspondences. */
int ss_two_view_batch_device(ss_ctx *ctx, const int32_t *train_src, const void *d_idx, int n_problems, const ss_proj_view *views,
                             const ss_two_view_params *p, void *d_flag, void *d_points, void *d_point_rows, void *d_n_points, void *d_result);
/* One problem (number 0) with host pointers in and out (copy in, the pairs form, copy out), synchronous; the arguments of
 * ss_two_view_host.  n_kp1, n_kp2 <= SS_GUIDED_MAX_ROWS. */
int ss_two_view(ss_ctx *ctx, const ss_proj_view *view, const ss_keypoint *kp1, int n_kp1, const ss_keypoint *kp2, int n_kp2, const int32_t *idx,
                const ss_two_view_params *p, uint8_t *flag, ss_map_point *points, int32_t *point_rows, int32_t *n_points,
                ss_two_view_result *result);

/* ---- Essential-graph optimisation: Optimizer::OptimizeEssentialGraph (g2o VertexSim3Expmap and EdgeSim3 under Levenberg-Marquardt)
 * as LoopClosing::CorrectLoop calls it once a loop is accepted, for several loops (problems) of a call at once, and the map-point
 * correction that follows it there.  tests/graph_ref.py is its normative statement; DESIGN.md section 28.  An addition to ABI 5:
 * nothing existing changes.  The g2o and ORB-SLAM3 sources are not in the reference tree: parity with the real binary is unpinned,
 * as for the Sim3 refinement and the local bundle adjustment ----------------------------------------------------------------------
 * - All arithmetic is double.  Every step is one IEEE operation, left to right as written, with no contraction.  Division and sqrt
 *   are the only library operations: atan2 and ln are series of csrc/ss_graph_steps.h, the same text on host and device.
 * - Every sum has one fixed order, so ss_pose_graph_host and the kernels agree bit for bit, for any number of problems in a call.
 * A Sim3 S = (R, t, s) maps x to s.R.x + t and is thirteen doubles: R row-major, t, s.  Product A.B = (RA.RB, sA.(RA.tB) + tA,
 * sA.sB), entries (a*b + c*d) + e*f; inverse (R^T, -((1/s).(R^T.t)), 1/s).
 * A call has n_kf keyframes, each with a NON-CORRECTED Sim3 N_v, a START Sim3 S_v and a `fixed` byte, a HOST table of edges (i, j),
 * keyframe numbers of the call, and a HOST table of problems.  Problem q owns the keyframes first_kf .. first_kf + n_kf - 1 and the
 * edges first_edge .. first_edge + n_edges - 1, whose endpoints are keyframes of the problem, i != j; a pair listed twice is two
 * edges.  Neither range overlaps another problem's.  Upstream's vertex and edge sets (spanning tree, loop edges, covisibility >=
 * 100, the new loop connections) are the caller's to choose.  WHICH KEYFRAMES TO FIX: every measurement is formed from the
 * non-corrected Sim3s (step 1), so the measurements alone are a consistent graph whose zero-cost states are S_v = N_v . D for one
 * common D.  A loop correction therefore enters through the fixed keyframes: fix the loop keyframe at its non-corrected pose AND the
 * current keyframe (or its corrected group) at the corrected Sim3s; the edges spread the disagreement over the free keyframes in
 * between.  With the loop keyframe alone fixed at N_m (upstream's choice, which works there because it measures the loop
 * connections from the corrected Sim3s) the optimum is the non-corrected map and the points do not move.
 * 1. Start.  A problem whose N_v or S_v has an entry that is not finite, or s not > 0: state 2.  No free keyframe or no edge: state
 *    1.  The state starts as the S_v as they stand (no orthonormalisation).  M_e = N_j . N_i^-1, formed once.
 * 2. Error of an edge: E = (M_e . S_i) . S_j^-1, e = (omega, upsilon, sigma).  v = (E21 - E12, E02 - E20, E10 - E01) / 2 (each
 *    0.5 * difference), c = 0.5 * (((E00 + E11) + E22) - 1.0), n = sqrt((v0*v0 + v1*v1) + v2*v2), theta = atan2(n, c).  omega =
 *    v * (theta / n); if n < 2^-26: omega = v; if c < 0 and n < 2^-20 (next to pi, where v vanishes): with B = (E + E^T) / 2
 *    entry by entry, d = 1.0 - c and k the largest diagonal entry of E (the first among equals), a_k = sqrt((E_kk - c) / d), a_j =
 *    B_kj / (d * a_k), negated when (a0*v0 + a1*v1) + a2*v2 < 0; omega = a * theta: defined, with no NaN, at theta = pi.  upsilon =
 *    t_E AS IT STANDS, without g2o's W^-1: the counterpart of the retraction below; second order in the error, zero at a consistent
 *    graph.  sigma = ln(s_E).  The information matrix is the identity, as upstream sets it.
 * 3. Retraction by delta = (omega, upsilon, sigma), the Sim3 refinement's: dR of ss_pose_exp, ds its scale series; R <- dR.R, t <-
 *    ds * (dR.t) + upsilon, s <- ds * s.  Refused (state 4, nothing moves): q > pi*pi or |delta_6| > 1.  fix_scale (upstream's
 *    bFixScale for stereo) holds delta_6 = 0 and s as it is.
 * 4. Jacobians are g2o's own for EdgeSim3, which defines none: central differences through the retraction, column a of endpoint
 *    `side` = (e(+h) - e(-h)) / 2h with h = 1e-9 (2h the double next to 2e-9).  Columns of a fixed endpoint, and the scale column
 *    under fix_scale, are +0.0.
 * 5. Per free keyframe v: H_vv = sum J^T.J and g_v = sum J^T.e over its incident (edge, side) pairs in ascending edge number from
 *    +0.0, each entry a seven-term dot product added left to right.  d_a = lambda * (1.0 + H_aa); the preconditioner is the Cholesky
 *    factor (ss_gn_chol_n) of H_vv with H_aa + d_a on its diagonal, order 7 (6 under fix_scale).  A pivot not > 0: state 2.
 * 6. The step solves (H + diag d) delta = -g by preconditioned conjugate gradients, matrix-free: u_e = J_ei.p_i + J_ej.p_j (fourteen
 *    products left to right), q_v = sum J_side^T.u_e in the order of 5, then + d_a * p_a.  x = 0, r = -g, z = M^-1.r, p = z, rho =
 *    r.z, stop = (pcg_tol * pcg_tol) * rho.  Each iteration: q = A.p; pq = p.q; if not pq > 0 the solve ends and keeps x; alpha =
 *    rho / pq; x += alpha * p; r -= alpha * q; z = M^-1.r; rho' = r.z; the solve ends after pcg_iterations iterations or once
 *    rho' <= stop; else beta = rho' / rho, p = z + beta * p.  Every dot product is the tree of the pose-only optimisation over the
 *    7 * n_kf entries in keyframe-major order (slot k mod 256), entries of fixed keyframes and of the held scale being +0.0.
 * 7. Accept or reject, as in the local bundle adjustment: the cost is the tree sum over the edges (slot e mod 256) of e^T.e (seven
 *    squares added left to right).  A step is accepted iff every trial entry is finite and the trial cost is finite and <= the
 *    cost before; then lambda <- max(lambda / lambda_factor, lambda_min), else nothing moves and lambda <- lambda * lambda_factor.
 *    `iterations` steps are taken.  A start cost that is not finite: state 2.
 * Outputs.  Per problem an ss_graph_result, 48 bytes.  Per keyframe of the call thirteen doubles, the Sim3, and twelve doubles, R
 * and t / s (upstream's SetPose), which feed ss_proj_view_init unchanged.  A fixed keyframe, a keyframe of no problem and every
 * keyframe of a problem that ends in state 1, 2 or 4 before its first accepted step return their start bit for bit.
 * Deviations from upstream: upsilon without W^-1; g2o's Levenberg-Marquardt scales lambda by its gain ratio and seeds it from the
 * diagonal, here it is multiplied or divided by lambda_factor from the given start; the linear solve is block-Jacobi PCG to a loose
 * tolerance (a sparse Cholesky there); the exponentials, atan2 and ln by series; the order of every sum is fixed; every edge is
 * measured from the non-corrected Sim3s (upstream measures the loop connections from the corrected ones), so the corrected
 * keyframes are fixed where upstream fixes the loop keyframe alone. */
#define SS_GRAPH_MAX_KF 16384     /* keyframes of a problem */
#define SS_GRAPH_MAX_EDGES 131072 /* edges of a problem */
typedef struct {            /* 16 bytes, one per problem (a HOST table) */
    int32_t first_kf, n_kf, first_edge, n_edges;
} ss_graph_problem;
typedef struct {            /* 48 bytes */
    double lambda;          /* the first step's; finite and >= 0; upstream: 1e-16.  0 is plain Gauss-Newton: the block of a free
                             * keyframe without an edge is then all zero and its pivot ends the problem in state 2 (step 5); with
                             * any lambda > 0 that keyframe stays where it is */
    double lambda_factor;   /* finite and > 1; default 10 */
    double lambda_min;      /* finite and >= 0; default 0 */
    double pcg_tol;         /* finite and >= 0; default 1e-2 */
    int32_t iterations;     /* 1 .. 64; upstream: 20 */
    int32_t pcg_iterations; /* 1 .. 4096; default 128 */
    int32_t fix_scale;      /* non-zero: delta_6 = 0, blocks of order 6 */
    int32_t reserved;       /* must be 0 */
} ss_graph_params;
typedef struct {            /* 48 bytes, one per problem */
    double lambda;          /* after the last step */
    double cost_before, cost_after;
    int32_t state;          /* 0 ok, 1 nothing to optimise, 2 not finite or a pivot not > 0, 4 step too large */
    int32_t n_edges, n_free;
    int32_t steps, accepted; /* steps taken, rejected ones included; steps accepted */
    int32_t pcg_iterations; /* of all steps */
} ss_graph_result;
/* The whole rule on the host from the text the kernels compile (csrc/ss_graph_steps.h), one problem; needs no device.  nc, start:
 * n_kf x 13 doubles; fixed: n_kf bytes; edges: n_edges pairs; sim3 n_kf x 13 and poses n_kf x 12 doubles out.  Arguments are checked
 * as the device calls check them (SS_ERR_INVALID_ARG). */
int ss_pose_graph_host(const double *nc, const double *start, const uint8_t *fixed, int n_kf, const int32_t *edges, int n_edges,
                       const ss_graph_params *p, double *sim3, double *poses, ss_graph_result *result);
/* One edge on the host: its error e (7) under (N_i, N_j, S_i, S_j) and both Jacobian blocks, J [14][7]: column c of endpoint i at
 * J + 7c, of endpoint j at J + 7(7 + c); fixed_i / fixed_j and fix_scale zero columns as step 4 says. */
int ss_pose_graph_edge_host(const double *nc_i, const double *nc_j, const double *s_i, const double *s_j, int fixed_i, int fixed_j,
                            int fix_scale, double *e, double *J);
/* The two series on the host, n values each: out[k] = atan2(y[k], x[k]) for finite y >= 0 and finite x, ln(x[k]) for finite x > 0;
 * NaN outside. */
int ss_graph_atan2_host(const double *y, const double *x, int n, double *out);
int ss_graph_ln_host(const double *x, int n, double *out);
/* n_problems problems on device arrays: d_nc and d_start double [n_kf][13], d_fixed uint8 [n_kf]; problems (n_problems) and edges
 * (int32 [n_edges][2]) are HOST tables, copied (with the incidence lists the host builds from them) before the call returns.
 * Outputs: d_sim3 double [n_kf][13], d_poses double [n_kf][12], d_result [n_problems] ss_graph_result; every byte is written.
 * SS_ERR_INVALID_ARG, with a message: an endpoint outside its problem, i == j, n_kf outside 1 .. SS_GRAPH_MAX_KF or n_edges outside
 * 0 .. SS_GRAPH_MAX_EDGES, a keyframe or edge range outside the call or overlapping another problem's, a parameter out of its
 * range, a reserved field that is not 0, a NULL buffer.  Without a keyframe the call returns SS_OK and writes nothing.  The fixed
 * schedule of every step is enqueued at once; a problem that has ended costs empty launches.  The workspace is dominated by the
 * edges' Jacobians, 784 bytes each.  Asynchronous on the context's stream. */
int ss_pose_graph_device(ss_ctx *ctx, const void *d_nc, const void *d_start, const void *d_fixed, int n_kf,
                         const ss_graph_problem *problems, int n_problems, const int32_t *edges, int n_edges, const ss_graph_params *p,
                         void *d_sim3, void *d_poses, void *d_result);
/* One problem with host pointers in and out (copy in, the device form, copy out), synchronous; the arguments of
 * ss_pose_graph_host. */
int ss_pose_graph(ss_ctx *ctx, const double *nc, const double *start, const uint8_t *fixed, int n_kf, const int32_t *edges,
                  int n_edges, const ss_graph_params *p, double *sim3, double *poses, ss_graph_result *result);
/* The map-point correction of OptimizeEssentialGraph: row i of block b of d_points ([n_blocks][point_rows] ss_map_point) whose
 * d_ref entry (int32 [n_blocks][point_rows]) names keyframe r of the call, 0 <= r < n_kf, gets x <- S_r^-1(N_r(x)) in double from
 * its floats widened: y = s_N * ((R_N.x)) + t_N, x' = (1 / s_S) * (R_S^T.(y - t_S)), rounded to the block's floats; the other 20 bytes
 * of the ss_map_point are left alone (UpdateNormalAndDepth stays with the caller).  Any other r (-1) skips the row.  d_nc and d_sim3
 * are double [n_kf][13]: the call's input and ss_pose_graph_device's output.  SS_ERR_INVALID_ARG: a bad count, point_rows above
 * SS_GUIDED_MAX_ROWS, a NULL buffer.  Asynchronous. */
int ss_pose_graph_points_device(ss_ctx *ctx, void *d_points, const void *d_ref, int n_blocks, int point_rows, const void *d_nc,
                                const void *d_sim3, int n_kf);

/* ---- Global bundle adjustment: Optimizer::GlobalBundleAdjustemnt / BundleAdjustment (the edges of the local bundle adjustment
 * over every keyframe and point of a map, under one Levenberg-Marquardt loop with the points marginalised) as
 * LoopClosing::RunGlobalBundleAdjustment starts it after a loop correction and CreateInitialMapMonocular after the initialisation,
 * for several maps (problems) of a call at once.  tests/gba_ref.py is its normative statement; DESIGN.md section 29.  An addition
 * to ABI 5: nothing existing changes.  The g2o and ORB-SLAM3 sources are not in the reference tree: parity with the real binary is
 * unpinned, as for the Sim3 refinement, the local bundle adjustment and the essential-graph optimisation --------------------------
 * - All arithmetic is double.  Every step is one IEEE operation, left to right as written, with no contraction.  The only library
 *   functions are sqrt and division.  Every test is written in its accepting form, so a NaN fails it (the step-size test of
 *   ss_pose_exp excepted).
 * - Every sum has one fixed order, so ss_global_ba_host and the kernels agree bit for bit, for any number of problems of a call
 *   and whatever the order of the observation records.
 * A call has n_kf keyframes (a start pose and a fixed byte each on the device, a view each in a HOST table: only the camera and bf
 * of a view are read, as in the local bundle adjustment), blocks of map points (only x, y, z are read) with an optional skip byte
 * each, a HOST table of observation records (ss_gba_obs, any order) and a HOST table of problems.  Problem q owns the keyframes
 * first_kf .. first_kf + n_kf - 1, the blocks first_block .. first_block + n_blocks - 1 (its points: P = n_blocks * point_rows,
 * point i = block * point_rows + row relative to first_block) and the records first_obs .. first_obs + n_obs - 1, whose kf and point
 * are relative to the problem.  No two problems share a keyframe, a block or a record.  The host sorts a problem's records by
 * (point, kf) with two stable counting passes and builds both incidence lists from the sorted table: a point's list in ascending
 * kf, a keyframe's list in ascending point.  "List order" below is that order; j is an item's place in its keyframe's list.
 * 1. Observations and points, as step 1 of the local bundle adjustment with the record in the place of the keypoint row.  Point row
 *    i of a block is a point iff i < n_points of the block, its skip byte (if given) is 0 and x, y, z are finite.  A record is an
 *    observation iff its point is a point and its octave lies in 0 .. n_levels-1; u, v are the record's floats widened, w = 1.0 /
 *    (s*s) with s = (double)scale[octave]; stereo iff check_right is set and right > 0.  A point is active iff it has at least
 *    min_point_obs observations; the others are flagged 1 and never move.  Start poses go through step 2 of the pose-only
 *    optimisation (Gram-Schmidt); one that is not finite gives the problem state 2 at once.  Keyframe k is free iff fixed[k] == 0;
 *    no fixed keyframe is required (the damping keeps the system definite, the gauge is the caller's choice; upstream fixes the
 *    first keyframe).  No active point or no free keyframe: state 1.
 * 2. Linearisation: step 2 of the local bundle adjustment, term by term (ss_ba_lin, ss_pose_terms).
 * 3. Per active point: step 3 of the local bundle adjustment over the point's list (ascending kf from +0.0, fixed keyframes
 *    included): V_i, b_i, the damping V_aa += lambda*(1.0 + V_aa), the factor, frozen points.  W_ki is kept for every free k.
 * 4. Per free keyframe k, over its list in list order.  The 26 sums of U_k and g_k (every contributing observation), the 21 of the
 *    upper triangle of C_kk = sum_i Y_ki.W_ki^T and the 6 of sum_i Y_ki.b_i (the contributing observations of solved points; Y_ki =
 *    W_ki.V_i^-1 row by row by the two triangular solves, the entries as in step 4 of the local bundle adjustment) are each a tree
 *    of 256 slots: slot s adds the items j = s, s + 256, ... in ascending j from +0.0, skipping those that do not contribute; each
 *    group of 64 slots folds by halving; the four results combine as (r0 + r1) + (r2 + r3).  U_aa += lambda*(1.0 + U_aa); M_k = U_k
 *    - C_kk, one subtraction per entry, is factored by Cholesky by columns of order 6 (ss_gn_chol_n); r_k = -(g_k - sum Y.b).  A
 *    pivot that is not > 0 in any free keyframe: state 2, the problem ends, nothing moves.  A free keyframe without a contributing
 *    observation has M_k = lambda on the diagonal: it stays where it is for any lambda > 0, and ends the problem under lambda 0.
 * 5. Solve S.dc = r, S = U - W.V^-1.W^T over the free keyframes, by preconditioned conjugate gradients; S is never formed.
 *    The operator q = S.p: per solved point a_i = sum_k W_ki^T.p_k over its free contributing observations in ascending kf from
 *    +0.0 (a_b = a_b + (((((W[0][b]*p[0] + W[1][b]*p[1]) + W[2][b]*p[2]) + W[3][b]*p[3]) + W[4][b]*p[4]) + W[5][b]*p[5])), c_i =
 *    V_i^-1.a_i by the two triangular solves; per free keyframe q_k = U_k.p_k - T_k, entry by entry, with (U.p)_a the six products
 *    of row a added left to right and T_k the tree over the keyframe's list of W_ki.c_i (entry a: (W[a][0]*c[0] + W[a][1]*c[1]) +
 *    W[a][2]*c[2]; the items of solved points that contribute).  So Y.x is W.(V^-1.x) in the operator and (W.V^-1).x in step 4,
 *    on the host and on the device alike.  The loop is that of the essential-graph optimisation: x = 0, z = M^-1.r block by
 *    block, p = z, rho = r.z, stop = (pcg_tol*pcg_tol)*rho; while fewer than pcg_iterations are done: q = S.p, pq = p.q, leave
 *    unless pq > 0 (x kept); alpha = rho / pq; x += alpha*p, r -= alpha*q; one more is done; z = M^-1.r; rho1 = r.z; leave if rho1
 *    <= stop; beta = rho1 / rho; p = z + beta*p; rho = rho1.  Every dot product is the tree over the 6*n_kf entries in
 *    keyframe-major order (entry e in slot e % 256); the entries of fixed keyframes are +0.0.  dc = x.
 * 6. Back-substitution and update: step 6 of the local bundle adjustment over the point's list (v = -b_i, the free contributing
 *    observations in ascending kf, dp_i = V_i^-1.v), the trial poses by exp(dc_k), and q > pi*pi in any free keyframe: state 4.
 * 7. Accept or reject, the lambda schedule and the end of a round: step 7 of the local bundle adjustment.  The cost of a state is
 *    the tree over the keyframes (keyframe k in slot k % 256, ascending) of the tree over each keyframe's list, in list order, of
 *    the chi-terms of the inlier observations of active points.
 * 8. Rounds and classification: step 8 of the local bundle adjustment.  The defaults are upstream's global schedule: one robust
 *    round of 10 iterations.
 * 9. No NaN bits reach a result, as in step 9 of the local bundle adjustment.
 * Outputs.  Per problem one ss_gba_result, 104 bytes.  Per keyframe of the call twelve doubles: fixed keyframes and those of no
 * problem get their orthonormalised start.  Per block and point row three doubles and one flag byte with the local bundle
 * adjustment's meaning (0 optimised, 1 too few observations or inliers, 2 not a point, its doubles +0.0; every row of a block of
 * no problem is flagged 2), in its layout with one block in the place of one problem, so that ss_local_ba_points_to_block with
 * n_problems = n_blocks and block_of = NULL rounds the result back into the map.  Per record, in the caller's order, one byte: 0
 * inlier, 1 outlier, 2 not an observation (every record of no problem).  Every output byte is written exactly once per call.
 * Deviations from upstream: those of the local bundle adjustment; the linear solve is block-Jacobi PCG on the reduced system to a
 * loose tolerance (a sparse Cholesky there); no map bookkeeping and no stop flag. */
#define SS_GBA_MAX_KF 16384       /* keyframes of a problem: SS_GRAPH_MAX_KF, one call's output feeds the other */
#define SS_GBA_MAX_POINTS 1048576 /* n_blocks * point_rows of a problem */
#define SS_GBA_MAX_OBS 4194304    /* observation records of a problem */
typedef struct {            /* 24 bytes, one per observation (a HOST table, any order) */
    int32_t kf;             /* 0 .. n_kf-1, relative to the problem */
    int32_t point;          /* block * point_rows + row, relative to the problem's first block */
    float u, v;             /* the undistorted keypoint */
    float right;            /* > 0: a stereo observation when check_right is set */
    int32_t octave;
} ss_gba_obs;
typedef struct {            /* 32 bytes, one per problem (a HOST table) */
    int32_t first_kf, n_kf, first_block, n_blocks, first_obs, n_obs;
    int32_t reserved[2];    /* must be 0 */
} ss_gba_problem;
typedef struct {            /* 104 bytes */
    double chi2_mono;       /* finite and > 0; upstream: 5.991 */
    double chi2_stereo;     /* finite and > 0; upstream: 7.815 */
    double lambda;          /* the first step's; finite and >= 0; default 1e-4 */
    double lambda_factor;   /* finite and > 1; default 10 */
    double lambda_min;      /* finite and >= 0; default 1e-9 */
    double step_eps;        /* finite and >= 0; default 1e-10; 0 runs every step */
    double pcg_tol;         /* finite and >= 0; default 1e-2 (DESIGN.md section 29 holds the table it was chosen on) */
    int32_t n_rounds;       /* 1 .. SS_BA_MAX_ROUNDS; default 1 */
    int32_t iterations[4];  /* each 1 .. 32 for r < n_rounds; default 10 */
    int32_t robust_rounds;  /* 0 .. SS_BA_MAX_ROUNDS; default 1 */
    int32_t min_point_obs;  /* >= 1; default 2 */
    int32_t check_right;    /* non-zero: a record with right > 0 is a stereo observation */
    int32_t pcg_iterations; /* 1 .. 256 per step; default 64.  Each one is three launches of the fixed schedule */
    int32_t reserved[3];    /* must be 0 */
} ss_gba_params;
typedef struct {            /* 104 bytes, one per problem */
    double lambda;          /* after the last step */
    double cost_before;     /* the cost ahead of the first step of round 0 */
    double cost_after;      /* the cost of the state returned, under the inliers and robustness of the last round that ran */
    int32_t state;          /* 0 ok, 1 no active point or no free keyframe, 2 not positive definite, or a start pose or a cost that is not finite, 4 step too large */
    int32_t status;         /* SS_OK */
    int32_t n_obs, n_stereo; /* observations of points, active or not; the stereo ones among them */
    int32_t n_inliers;      /* observation bytes that are 0 on return */
    int32_t n_points_active; /* point flags that are 0 on return */
    int32_t n_frozen_max;   /* the most points frozen in one step */
    int32_t steps[4];       /* steps taken in round r, rejected ones included */
    int32_t accepted[4];    /* steps accepted in round r */
    int32_t pcg_iterations; /* of all steps */
    int32_t n_free, n_fixed; /* keyframes of the problem */
    int32_t reserved[2];    /* 0 */
} ss_gba_result;
/* The whole rule on the host from the text the kernels compile (csrc/ss_gba_steps.h), one problem of n_kf keyframes, n_points point
 * rows (one block) and n_obs records; needs no device.  views, start (n_kf x 12 doubles) and fixed are per keyframe; poses n_kf x
 * 12 doubles, xyz n_points x 3 doubles, point_flags n_points bytes, obs_flags n_obs bytes in the order of obs.  Arguments are
 * checked as the device call checks them: SS_ERR_INVALID_ARG, and the message in err (err_bytes of it; NULL: none). */
int ss_global_ba_host(const ss_proj_view *views, const double *start, const uint8_t *fixed, int n_kf, const float *scale, int n_levels,
                      const ss_map_point *points, const uint8_t *point_skip, int n_points, const ss_gba_obs *obs, int n_obs,
                      const ss_gba_params *p, double *poses, double *xyz, uint8_t *point_flags, uint8_t *obs_flags,
                      ss_gba_result *result, char *err, int err_bytes);
/* The records of the stack the projection searches leave, in ascending (point, kf) order: one for every idx[k][i] (int32
 * [n_kf][n_points]) with 0 <= idx < n_kp[k] clamped to 0 .. rows_per_frame, with the keypoint's x, y and octave and right[k][row]
 * (right NULL: -1).  kp and right are [n_kf][rows_per_frame], downloaded.  Returns the count and writes at most capacity records
 * (out NULL: counts only); SS_ERR_INVALID_ARG (negative) for a NULL table or a bad count.  Pure host code. */
int ss_global_ba_obs_from_idx_host(const ss_keypoint *kp, const float *right, const int32_t *n_kp, int n_kf, int rows_per_frame,
                                   const int32_t *idx, int n_points, ss_gba_obs *out, int capacity);
/* The keypoint row of each of those records: the same enumeration, the same ascending (point, kf) order, the same clamp and the
 * same return convention, so out[m] is the row of record m of ss_global_ba_obs_from_idx_host's table (the obs_row of
 * ss_covis_set_map_rows).  Pure host code. */
int ss_global_ba_rows_from_idx_host(const int32_t *n_kp, int n_kf, int rows_per_frame, const int32_t *idx, int n_points,
                                    int32_t *out, int capacity);
/* n_problems problems on device arrays: d_points [n_blocks][point_rows] ss_map_point, d_point_skip uint8 [n_blocks][point_rows] or
 * NULL, d_n_points int32 [n_blocks] (clamped to 0 .. point_rows), d_start double [n_kf][12] (ss_pose_graph_device's d_poses feeds
 * it without a round trip), d_fixed uint8 [n_kf].  problems (n_problems), obs (n_obs) and views (n_kf) are HOST tables, copied
 * (sorted, with both incidence lists) before the call returns.  The scale table and n_levels are the context's.  Outputs: d_poses
 * double [n_kf][12], d_xyz double [n_blocks][point_rows][3], d_point_flags uint8 [n_blocks][point_rows], d_obs_flags uint8
 * [n_obs], d_result [n_problems] ss_gba_result.  SS_ERR_INVALID_ARG, with a message: a kf or point outside its problem, a (kf,
 * point) pair twice, n_kf outside 1 .. SS_GBA_MAX_KF, n_blocks * point_rows outside 0 .. SS_GBA_MAX_POINTS or n_obs outside 0 ..
 * SS_GBA_MAX_OBS, a keyframe, block or record range outside the call or overlapping another problem's, a parameter out of its
 * range, a reserved field that is not 0, a NULL buffer, point_rows above SS_GUIDED_MAX_ROWS.  Without a keyframe or without a
 * problem the call returns SS_OK and writes nothing.  The fixed schedule of every round, step and PCG iteration is enqueued at
 * once (7 + 3 * pcg_iterations launches per step); a problem that has ended, or whose PCG has left, costs empty launches.  The
 * context's workspace for a call is dominated by the W blocks, 144 bytes per record (4 194 304 records: 604 MB);
 * SS_ERR_NO_MEMORY when it cannot be had.  Asynchronous on the context's stream. */
int ss_global_ba_device(ss_ctx *ctx, const void *d_points, const void *d_point_skip, const void *d_n_points, int n_blocks,
                        int point_rows, const void *d_start, const void *d_fixed, int n_kf, const ss_gba_problem *problems,
                        int n_problems, const ss_gba_obs *obs, int n_obs, const ss_proj_view *views, const ss_gba_params *p,
                        void *d_poses, void *d_xyz, void *d_point_flags, void *d_obs_flags, void *d_result);
/* One problem with host pointers in and out (copy in, the device form, copy out), synchronous; the arguments of
 * ss_global_ba_host without the message buffer (the message is the context's last error). */
int ss_global_ba(ss_ctx *ctx, const ss_proj_view *views, const double *start, const uint8_t *fixed, int n_kf,
                 const ss_map_point *points, const uint8_t *point_skip, int n_points, const ss_gba_obs *obs, int n_obs,
                 const ss_gba_params *p, double *poses, double *xyz, uint8_t *point_flags, uint8_t *obs_flags, ss_gba_result *result);

/* ---- Covisibility: how many map points two keyframes share, as KeyFrame::UpdateConnections counts it for a keyframe,
 * Tracking::UpdateLocalKeyFrames for a tracked frame and LocalMapping::KeyFrameCulling walks the same two incidence lists for the
 * redundant observations of a keyframe.  tests/covis_ref.py is its normative statement; DESIGN.md section 31.  An addition to ABI
 * 5: nothing existing changes.  All of it is integer counting, so it is order-free and exact; one float comparison closes the
 * culling vote -----------------------------------------------------------------------------------------------------------------
 * The map.  ss_covis_set_map takes the tables ss_global_ba_device takes: problems (ss_gba_problem, HOST) and observation records
 * (ss_gba_obs, HOST, any order; only kf, point, octave and right are read), and optionally one skip byte per record (cull_skip, in
 * the order of obs).  Per problem the host sorts the records by (point, kf) with two stable counting passes and keeps compact
 * lists, 12 bytes per record: a point's list is its run of (kf, octave, stereo bit, skip bit) in ascending kf; a keyframe's list
 * is its run of point numbers in ascending point, each with the record's place in the point's run.  A record is an observation
 * iff its octave lies in 0 .. n_levels-1 of the context; it is stereo iff check_right is set and right > 0.  The context keeps the
 * tables on the device until the next ss_covis_set_map or ss_destroy (the map changes at keyframe rate, frames query it at frame
 * rate); n_problems == 0 clears the map.
 * Weights.  A keyframe row k of problem q: for j != k of the same problem, w(j) is the number of points i for which both (k, i)
 * and (j, i) are observations.  A frame row b: w(j) is the number of hits i whose point (j, i) is an observation; a hit is a row i
 * of d_idx[b] with idx >= 0 (only the sign is read) and i < clamp(d_n_points[point_src[b]], 0, point_rows), its point is
 * (point_src[b] - first_block) * point_rows + i of the block's problem; there is no self exclusion.  A frame whose block, or a
 * keyframe row whose keyframe, belongs to no problem has an empty row.
 * Row summary (ss_covis_row).  n_shared: the j with w > 0.  max_weight, max_kf: the largest w and the lowest j that attains it; 0
 * and -1 with nothing shared.  The listed set is every j with w >= min_weight; if it is empty, fallback is set and max_kf >= 0, it
 * is {max_kf} (UpdateConnections' "no keyframe over the threshold: connect to the best").  n_listed is its size, n_written =
 * min(n_listed, cap).
 * Neighbour list.  d_nb is int32 [n_rows][cap][2]: (kf relative to the problem, weight), weight descending, then kf ascending (a
 * rule of ours: upstream's sort of pair<int, KeyFrame*> breaks ties by pointer); truncation keeps the first cap entries of that
 * order; entries from n_written on are (-1, 0).
 * Culling counts (keyframe rows; a frame row gets zeros): LocalMapping::KeyFrameCulling for keyframe k.  An item (k, i) that is an
 * observation and whose skip bit is 0 is examined and adds 1 to n_mps (the skip bit stands for upstream's depth test, which
 * passes over the point before it is counted).  count(i) is the observations of i plus its stereo ones once more
 * (MapPoint::Observations()); near is the number of observations (j, i), j != k, with octave_j <= octave_k + cull_slack.  An
 * examined item adds 1 to n_redundant iff count(i) > cull_obs and near > cull_obs.  redundant = ((float)n_redundant > redundant_th
 * * (float)n_mps): one float multiply and one compare, uncontracted.  Skip bits do not affect the weights.
 * Deviations from upstream.  A row is what UpdateConnections itself leaves in mvpOrderedConnectedKeyFrames, on a snapshot of the
 * map; its history-dependent side effects on the other keyframes (AddConnection -> UpdateBestCovisibles, which re-sorts every
 * counted keyframe, those under the threshold too) are not modelled: min_weight 1 gives that superset.  The fallback is
 * one-directional.  The culling counts are order-free on the snapshot (upstream removes a culled keyframe's observations before it
 * examines the next; its early break does not change a count's verdict and is not modelled).  With the caller stay: the spanning
 * tree (a new keyframe's parent is entry 0 of its row), children, parents and temporal neighbours in UpdateLocalKeyFrames,
 * applying a culling decision, and bad flags (leave those records out). */
/* records of one keyframe: a weight then fits 18 bits, and (weight << 14) | (16383 - kf) is one exact 32-bit sort key */
#define SS_COVIS_MAX_ROW_ITEMS 262143
#define SS_COVIS_MAX_NEIGHBOURS 1024 /* cap */
#define SS_COVIS_MAX_MAP_KF 1048576  /* keyframes of one ss_covis_set_map call, all its problems and the gaps between them */
typedef struct {            /* 32 bytes */
    int32_t min_weight;     /* >= 1; upstream: 15, and 1 for UpdateLocalKeyFrames */
    int32_t fallback;       /* 0 / 1; default 1 */
    int32_t cull_obs;       /* >= 0; upstream: 3 */
    int32_t cull_slack;     /* 0 .. SS_MAX_LEVELS; upstream: 1 */
    float redundant_th;     /* finite, 0 .. 1; upstream: 0.9 */
    int32_t reserved[3];    /* must be 0 */
} ss_covis_params;
typedef struct {            /* 32 bytes, one per row */
    int32_t n_shared, max_weight, max_kf, n_listed, n_written;
    int32_t n_mps, n_redundant, redundant;
} ss_covis_row;
int ss_covis_params_default(ss_covis_params *p);
/* The map of the context (above).  n_kf keyframes, n_blocks blocks of point_rows point rows and n_obs records in the call; the
 * problems own ranges of each as in ss_global_ba_device, and records of no problem are not read.  SS_ERR_INVALID_ARG, with a
 * message: a kf or point outside its problem, a (kf, point) pair twice, a problem's n_kf outside 1 .. SS_GBA_MAX_KF, its n_blocks *
 * point_rows outside 0 .. SS_GBA_MAX_POINTS or its n_obs outside 0 .. SS_GBA_MAX_OBS, the call's n_kf above SS_COVIS_MAX_MAP_KF or its
 * point rows above 2^29, a range outside the call or overlapping another problem's,
 * a reserved field that is not 0, point_rows above SS_GUIDED_MAX_ROWS, a keyframe with more than SS_COVIS_MAX_ROW_ITEMS records.  A
 * refused call leaves the map it found. */
int ss_covis_set_map(ss_ctx *ctx, const ss_gba_problem *problems, int n_problems, int n_kf, int n_blocks, int point_rows,
                     const ss_gba_obs *obs, int n_obs, const uint8_t *cull_skip, int check_right);
/* The same, and which keypoint row of its keyframe each record is: obs_row is a HOST int32 [n_obs] in the order of obs, or NULL
 * (then this is ss_covis_set_map).  With rows the context keeps one int32 per record next to the points' lists, in their order, and
 * the largest row of the map: what ss_refresh_device needs to find an observation's descriptor.  The covisibility queries do not
 * read them.  One more refusal, SS_ERR_INVALID_ARG with a message that names the record: a row < 0 or >= SS_GUIDED_MAX_ROWS. */
int ss_covis_set_map_rows(ss_ctx *ctx, const ss_gba_problem *problems, int n_problems, int n_kf, int n_blocks, int point_rows,
                          const ss_gba_obs *obs, int n_obs, const uint8_t *cull_skip, int check_right, const int32_t *obs_row);
/* n_rows keyframe rows: rows is a HOST table of call keyframe numbers in any order, duplicates allowed; NULL: every keyframe of
 * the map in order (n_rows must be the map's n_kf).  d_nb int32 [n_rows][cap][2], d_row ss_covis_row [n_rows]; every output byte
 * is written exactly once.  n_rows == 0: SS_OK, nothing written.  SS_ERR_STATE: no map is set.  SS_ERR_INVALID_ARG, with a message:
 * a row outside the map, cap outside 1 .. SS_COVIS_MAX_NEIGHBOURS, a parameter out of its range, a NULL buffer, more than 65535
 * rows.  Asynchronous on the context's stream. */
int ss_covis_kf_device(ss_ctx *ctx, const int32_t *rows, int n_rows, const ss_covis_params *p, int cap, void *d_nb, void *d_row);
/* n_frames frame rows: d_idx int32 [n_frames][point_rows] exactly as ss_match_proj_batch_device writes it, d_n_points int32
 * [n_blocks] of the map's blocks, point_src a HOST table of block numbers.  Otherwise as ss_covis_kf_device. */
int ss_covis_frames_device(ss_ctx *ctx, const void *d_idx, const void *d_n_points, const int32_t *point_src, int n_frames,
                           const ss_covis_params *p, int cap, void *d_nb, void *d_row);
/* One problem of n_kf keyframes and n_points points with host pointers in and out, synchronous: sets the context's map to it
 * (ss_covis_set_map) and returns every keyframe's row: nb int32 [n_kf][cap][2], row [n_kf]. */
int ss_covis(ss_ctx *ctx, int n_kf, int n_points, const ss_gba_obs *obs, int n_obs, const uint8_t *cull_skip, int check_right,
             const ss_covis_params *p, int cap, int32_t *nb, ss_covis_row *row);
/* The whole rule on the host from the text the kernels compile (csrc/ss_covis_steps.h); needs no device.  The map's arguments are
 * ss_covis_set_map's, with the pyramid's n_levels in the place of the context; the query's are the device forms' with host
 * arrays.  Arguments are checked as the device calls check them: SS_ERR_INVALID_ARG, and the message in err (err_bytes of it;
 * NULL: none). */
int ss_covis_kf_host(const ss_gba_problem *problems, int n_problems, int n_kf, int n_blocks, int point_rows, const ss_gba_obs *obs,
                     int n_obs, const uint8_t *cull_skip, int check_right, int n_levels, const int32_t *rows, int n_rows,
                     const ss_covis_params *p, int cap, int32_t *nb, ss_covis_row *row, char *err, int err_bytes);
int ss_covis_frames_host(const ss_gba_problem *problems, int n_problems, int n_kf, int n_blocks, int point_rows, const ss_gba_obs *obs,
                         int n_obs, const uint8_t *cull_skip, int check_right, int n_levels, const int32_t *idx, const int32_t *n_points,
                         const int32_t *point_src, int n_frames, const ss_covis_params *p, int cap, int32_t *nb, ss_covis_row *row,
                         char *err, int err_bytes);
/* The covisibility edges of the table ss_pose_graph_device takes, from downloaded rows: nb [n_rows][cap][2] and row [n_rows] as
 * written above, row_kf [n_rows] the keyframe of each row relative to its problem.  For every row r in ascending r and every entry
 * (j, w) of its list in list order with j > row_kf[r] and w >= min_weight, the pair (row_kf[r], j).  Writes at most capacity pairs
 * (edges int32 [capacity][2]; NULL: counts only) and returns the count of pairs that qualify; SS_ERR_INVALID_ARG (negative) for a
 * NULL table or a bad count.  Pure host code. */
int ss_covis_edges_host(const int32_t *nb, const ss_covis_row *row, const int32_t *row_kf, int n_rows, int cap, int min_weight,
                        int32_t *edges, int capacity);

/* ---- Map-point refresh: MapPoint::UpdateNormalAndDepth and MapPoint::ComputeDistinctiveDescriptors for every selected point of
 * the context's map in one call, with MapPoint::Observations() reported per point: what a triangulation, a fusion, a bundle
 * adjustment or a loop correction leaves stale in the fields the projection search reads (nx, ny, nz, min_dist, max_dist of an
 * ss_map_point and the point's row of d_point_desc).  tests/refresh_ref.py is its normative statement; DESIGN.md section 32.  An
 * addition to ABI 5: nothing existing changes --------------------------------------------------------------------------------------
 * The map is the context's (ss_covis_set_map_rows: the points' lists in ascending kf, and each record's keypoint row).
 * Inputs.  Per block b of a problem q of the map: d_points[b][i] and d_n_points[b] clamped to 0 .. point_rows; views[k].ow of every
 * keyframe of the call (a HOST ss_proj_view table; only ow is read); scale[] and n_levels of the context; optionally d_ref_kf
 * (int32 [n_blocks][point_rows]: the point's reference keyframe relative to its problem) and d_select (uint8
 * [n_blocks][point_rows]); d_desc, uint8 [n_kf][rows_per_frame][32]: the descriptors of the map's keyframes by call keyframe number.
 * Selection.  Row i of block b is refreshed iff the block belongs to a problem, i < n_points, its select byte (if given) is 0 and
 * x, y, z are finite; so the d_point_flags of ss_local_ba_* and ss_global_ba_* (0 = optimised) serve as d_select as they lie.  Any
 * other row has state -1.
 * Observations.  The records of the point's list whose octave lies in 0 .. n_levels-1, in ascending kf, numbered a = 0 .. n-1;
 * count = n + (the stereo ones), MapPoint::Observations().  n == 0: state 1.
 * Geometry (UpdateNormalAndDepth; all in double from the float32 inputs widened, one IEEE operation per step, no contraction).
 * Per observation d = P - ow_k, len = sqrt((dx*dx + dy*dy) + dz*dz); any len that is not > 0 or not finite: state 2.  Per component
 * the sum of the terms d[c] / len is a tree of 64 slots: slot s adds the terms a = s, s + 64, ... in ascending a from +0.0, and the
 * slots fold by halving (one 64-slot group of the global bundle adjustment's trees).  normal[c] = sum[c] / (double)n; upstream does
 * not renormalise.  The reference keyframe is d_ref_kf's entry if it is given and names an observation of the list, otherwise
 * observation 0 (upstream's EraseObservation falls back to mObservations.begin(); our order is kf order, its is pointer order).
 * level = the octave of the reference's record, dist = its len, max_dist = dist * (double)scale[level], min_dist = max_dist /
 * (double)scale[n_levels-1].  Each of the five numbers is rounded to float32 once.  Deviation: upstream runs Eigen float32; this
 * is the triangulation's deviation, so a refreshed point and a triangulated one follow one text.
 * Descriptor (ComputeDistinctiveDescriptors).  Observation a's descriptor is row obs_row of keyframe first_kf + kf of d_desc.
 * D[a][b] is the Hamming distance over all 256 bits, D[a][a] = 0.  median_a is the element of rank (n-1)/2 (integer division;
 * upstream's 0.5*(N-1) truncated) of row a in ascending order, the self distance included.  The winner is the lowest median, the
 * lowest a on a tie: the minimum of median << 14 | a (a < 16384 = SS_GBA_MAX_KF).  Upstream's tie is the first in pointer order: the
 * only deviation.  All of it is integer and order-free.
 * Outputs.  For a state-0 row: nx, ny, nz, min_dist, max_dist of d_points[b][i] if geometry is set, the 32 bytes of
 * d_point_desc[b][i] if descriptor is set.  x, y, z are never written, nor anything of a row whose state is not 0.  d_info
 * [n_blocks][point_rows] ss_refresh_info: ref_kf is the one used, best_kf the winner's keyframe (both relative to the problem);
 * states 1 and 2 carry n_obs and count, state -1 zero counts; ref_kf, level, best_kf and best_median are -1 in a row whose state is
 * not 0, ref_kf and level also with geometry 0 (then state 2 cannot occur), best_* also with descriptor 0.  d_summary [n_blocks]
 * ss_refresh_summary: n_rows is the clamped n_points of a block of a problem (0 for a block of none), n_selected the rows whose
 * state is not -1, then the rows of state 0, 1 and 2, and the largest n_obs.  Every byte of both is written exactly once per call.
 * With the caller stay mnFound / mnVisible, applying a culling decision and bad flags; the fisheye right-eye observations of
 * UpdateNormalAndDepth are not modelled. */
typedef struct {            /* 32 bytes */
    int32_t geometry;       /* 0 / 1; default 1: UpdateNormalAndDepth */
    int32_t descriptor;     /* 0 / 1; default 1: ComputeDistinctiveDescriptors.  At least one must be set */
    int32_t reserved[6];    /* must be 0 */
} ss_refresh_params;
typedef struct {            /* 32 bytes, one per point row */
    int32_t state;          /* 0 refreshed, 1 no observation, 2 a camera centre on the point (or a distance not finite), -1 not selected */
    int32_t n_obs, count;   /* the observations; with the stereo ones once more: MapPoint::Observations() */
    int32_t ref_kf, level;
    int32_t best_kf, best_median;
    int32_t reserved;       /* 0 */
} ss_refresh_info;
typedef struct {            /* 32 bytes, one per block */
    int32_t status;         /* SS_OK */
    int32_t n_rows, n_selected, n_refreshed, n_no_obs, n_degenerate, max_obs;
    int32_t reserved;       /* 0 */
} ss_refresh_summary;
int ss_refresh_params_default(ss_refresh_params *p);
/* Replaces MapPoint::UpdateNormalAndDepth and MapPoint::ComputeDistinctiveDescriptors over the context's map (its n_kf, n_blocks
 * and point_rows).  d_points [n_blocks][point_rows] ss_map_point (read and written), d_point_desc [n_blocks][point_rows][32]
 * (written), d_n_points int32 [n_blocks], d_ref_kf / d_select as above or NULL, d_desc as above, views a HOST table of the map's
 * n_kf views, copied before the call returns; d_info and d_summary as above.  With descriptor 0, d_desc and d_point_desc may be
 * NULL.  Descriptors and points on 16-byte boundaries, as everywhere.  SS_ERR_STATE: no map, or a map set without rows while
 * descriptor is set (a geometry-only call needs no rows).  SS_ERR_INVALID_ARG, with a message: rows_per_frame not above the map's
 * largest row or above SS_GUIDED_MAX_ROWS, n_kf * rows_per_frame above 2^31 - 1, a parameter out of range, a reserved field that is
 * not 0, a NULL buffer that the flags require.  Asynchronous on the context's stream. */
int ss_refresh_device(ss_ctx *ctx, void *d_points, void *d_point_desc, const void *d_n_points, const void *d_ref_kf,
                      const void *d_select, const void *d_desc, int rows_per_frame, const ss_proj_view *views,
                      const ss_refresh_params *p, void *d_info, void *d_summary);
/* One problem of n_kf keyframes and n_points points with host pointers in and out, synchronous: sets the context's map to it with
 * its rows (ss_covis_set_map_rows, the points as blocks of min(n_points, SS_GUIDED_MAX_ROWS) rows, as ss_covis lays them out),
 * refreshes points and point_desc in place and returns info [n_points] and one summary per block.  ref_kf and select [n_points] or
 * NULL; desc [n_kf][rows_per_frame][32]; obs_row [n_obs] (NULL only with descriptor 0). */
int ss_refresh(ss_ctx *ctx, const ss_proj_view *views, int n_kf, ss_map_point *points, uint8_t *point_desc, int n_points,
               const int32_t *ref_kf, const uint8_t *select, const ss_gba_obs *obs, const int32_t *obs_row, int n_obs, int check_right,
               const uint8_t *desc, int rows_per_frame, const ss_refresh_params *p, ss_refresh_info *info, ss_refresh_summary *summary);
/* The whole rule on the host from the text the kernels compile (csrc/ss_refresh_steps.h); needs no device.  The map's arguments
 * are ss_covis_set_map_rows', with the pyramid's table in the place of the context; the rest are ss_refresh_device's with host
 * arrays.  Arguments are checked as the device calls check them: SS_ERR_INVALID_ARG (a map without rows under descriptor:
 * SS_ERR_STATE), and the message in err (err_bytes of it; NULL: none). */
int ss_refresh_host(const ss_gba_problem *problems, int n_problems, int n_kf, int n_blocks, int point_rows, const ss_gba_obs *obs,
                    int n_obs, int check_right, const int32_t *obs_row, const float *scale, int n_levels, ss_map_point *points,
                    uint8_t *point_desc, const int32_t *n_points, const int32_t *ref_kf, const uint8_t *select, const uint8_t *desc,
                    int rows_per_frame, const ss_proj_view *views, const ss_refresh_params *p, ss_refresh_info *info,
                    ss_refresh_summary *summary, char *err, int err_bytes);

/* ---- Place recognition: KeyFrameDatabase (add / erase / DetectLoopCandidates / DetectNBestCandidates /
 * DetectRelocalizationCandidates): from a new keyframe or a lost frame and a database of keyframes' BoW vectors, the few keyframes
 * worth handing to the Sim3 or the PnP stage.  No ORB-SLAM3 source is in the reference tree: this is the library's own restatement,
 * tests/place_ref.py is its normative statement, and parity with the real binary stays unpinned.  DESIGN.md section 33.  An
 * addition to ABI 5: nothing existing changes -----------------------------------------------------------------------------------
 * Database.  n_db BoW vectors as ss_bow_transform_* writes them: d_db_word int32 (ascending, distinct), d_db_value double, both
 * [n_db][stride], d_db_count int32 [n_db] clamped to 0 .. stride: the arrays ss_bow_score_device takes, kept by the caller.  Row r
 * is keyframe r of the call, numbered as ss_covis_set_map numbers them; problems is a HOST table of ss_gba_problem of which only
 * first_kf and n_kf are read (n_kf in 1 .. SS_GBA_MAX_KF, the range inside the call, no keyframe in two problems).  A row's map is
 * its problem; a row of no problem takes part in nothing.  d_db_skip, uint8 [n_db] or NULL, is upstream's erase / isBad: it is read
 * at query time, so erasing a keyframe rebuilds nothing.  The inverted file: for every word 0 .. n_words-1 the rows whose vector
 * holds it within its count; an entry whose word lies outside that range is in no list.  The order inside a list is free:
 * everything that reads a list counts.
 * Query q of n_q: its vector (a row of d_q_word / d_q_value [n_q][q_stride] with d_q_count [n_q]); q_kf[q], HOST: its own database
 * row, or -1 for a frame; q_problem[q], HOST: its map (for q_kf >= 0 that row's problem); optionally its covisibility row as
 * ss_covis_kf_device writes it (d_q_nb int32 [n_q][q_cap][2], d_q_row ss_covis_row [n_q]): the first n_written (clamped to 0 ..
 * q_cap) entries, relative to q_problem, are the connected keyframes; an entry that names no keyframe of that problem is passed
 * over.  NULL covisibility arrays: nothing is connected (the relocalisation form).
 * 1. Shared words.  Row r is excluded iff it is skipped, belongs to no problem, r == q_kf, or it is connected.  words(r) is the
 *    number of the query's words, within its count and in range, whose list holds r.  The sharing set is the non-excluded r with
 *    words(r) > 0; empty: no candidates.
 * 2. Word threshold.  max_common is the largest words(r) of the sharing set, min_common = (int)((float)max_common * common_ratio):
 *    one float multiply, then truncation.  Survivors are the sharing rows with words > min_common.
 * 3. Score.  s(r) = (float) of ss_bow_score_device's double for (query, r), rounded once.  The minimum score: mode 0, min_score;
 *    mode 1 (LoopClosing::DetectLoop), start at 1.0f and, for each connected entry in list order whose row is not skipped, if
 *    s(j) < m then m = s(j).  Seeds are the survivors with s >= the minimum score; none: no candidates.
 * 4. Groups.  d_nb is int32 [n_db][nb_cap][2]: row r holds (kf relative to r's problem, weight), what ss_covis_kf_device writes
 *    with rows == NULL (upstream: cap 10, min_weight 15); an entry with kf < 0 ends the row.  For seed i: acc = s(i), best = i,
 *    best_s = s(i); for each entry j in list order that is a survivor of this query (seed or not): acc += s(j), one float add, and if
 *    s(j) > best_s, strictly, best = j, best_s = s(j).  A listed j that is no survivor contributes nothing (the one deviation:
 *    upstream's DetectNBestCandidates reads a stale score there).
 * 5. Candidates.  acc*(b) is the maximum of acc(i) over the seeds with best(i) == b, best_acc the maximum over all seeds; both
 *    maxima are taken in the IEEE total order (-0.0 below +0.0, a NaN at its fixed place), so they do not depend on a schedule.  The
 *    order is acc* descending in that order, then row ascending (a tie rule of ours: upstream ties by list position).  Threshold
 *    form (n_best == 0): every b with acc*(b) > retain_ratio * best_acc, one float multiply and a strict compare.  N-best form
 *    (n_best > 0): walk the order; the first n_best of the query's own problem are loop candidates (class 0), the first n_best of
 *    other problems merge candidates (class 1).  scope is applied last: 0 keeps only the query's own problem, 1 all; rows of other
 *    maps still count towards max_common and the groups.
 * Outputs per query.  d_cand [n_q][cand_cap] ss_place_cand in the candidate order, entries from n_written on (-1, -1, 0, 0, 0, 0);
 * d_summary [n_q] ss_place_summary (min_score as used, best_acc 0.0 without a seed, n_candidates the size of the set, n_written =
 * min(n_candidates, cand_cap), status SS_OK); optionally d_words int32 [n_q][n_db] (words(r), 0 for excluded rows) and d_score
 * float [n_q][n_db] (s, -1.0f for a row never scored; the connected rows of mode 1 are scored).  Every output byte is written
 * exactly once per call.  Values are expected finite, as the transform writes them; a NaN is ordered, never read as an index. */
#define SS_PLACE_MAX_DB 262144         /* n_db: a query's tables are [n_q][n_db]; below SS_COVIS_MAX_MAP_KF, whose numbering the rows share */
#define SS_PLACE_MAX_QUERIES 256       /* n_q: with SS_PLACE_MAX_DB four 256 MiB tables and one of 64 MiB in the workspace */
#define SS_PLACE_MAX_CANDIDATES 256    /* cand_cap and n_best: each written candidate is one pass of a workgroup over the survivors */
#define SS_PLACE_MAX_NEIGHBOURS 1024   /* nb_cap and q_cap: SS_COVIS_MAX_NEIGHBOURS, the rows ss_covis_kf_device can write */
typedef struct {            /* 32 bytes */
    int32_t min_score_mode; /* 0: min_score; 1: the lowest score of the connected keyframes.  Default 1 */
    float min_score;        /* mode 0; finite */
    int32_t n_best;         /* 0: the threshold form; 1 .. SS_PLACE_MAX_CANDIDATES: the N-best form.  Default 0 */
    int32_t scope;          /* 0: the query's own problem only; 1: all.  Default 1 */
    float common_ratio;     /* 0 .. 1; upstream: 0.8f */
    float retain_ratio;     /* 0 .. 1; upstream: 0.75f */
    int32_t reserved[2];    /* must be 0 */
} ss_place_params;
typedef struct {            /* 24 bytes */
    int32_t kf;             /* the call row */
    int32_t problem;
    int32_t words;
    int32_t cls;            /* the class: 0 own map, 1 other map */
    float score, acc;       /* s and acc* */
} ss_place_cand;
typedef struct {            /* 48 bytes, one per query */
    int32_t n_sharing, max_common, min_common, n_survivors, n_seeds;
    float min_score, best_acc;
    int32_t n_candidates, n_written, status;
    int32_t reserved[2];    /* 0 */
} ss_place_summary;
/* upstream's loop detection: mode 1, the threshold form, every map, 0.8f and 0.75f */
int ss_place_params_default(ss_place_params *p);
/* Builds the inverted file on the device from the caller's device arrays, which are never downloaded: a count of every word with
 * integer atomics, an exclusive scan, a fill through per-word cursors.  The lists are sized by their upper bound n_db * stride,
 * which the host knows, so the whole call is asynchronous on the context's stream: nothing waits for the device (only a workspace
 * that has to grow synchronises, as everywhere).  The context keeps the lists and the caller's pointers until the next call or
 * ss_destroy, so the arrays must stay allocated; their contents are read again by every query (the skip bytes, the vectors of the
 * scored rows).  n_db == 0 clears the database.  SS_ERR_INVALID_ARG, with a message: n_db outside 0 .. SS_PLACE_MAX_DB, stride < 1,
 * n_db * stride not below 2^31, n_words outside 1 .. SS_VOCAB_MAX_NODES, a NULL required buffer, a bad problem table.  A refused call
 * leaves the database it found. */
int ss_place_set_database(ss_ctx *ctx, const void *d_db_word, const void *d_db_value, const void *d_db_count, const void *d_db_skip,
                          int n_db, int stride, int n_words, const ss_gba_problem *problems, int n_problems);
/* The whole rule for n_q queries, enqueued at once on the context's stream with no host synchronisation inside (q_kf and q_problem
 * are HOST tables, copied before the call returns).  d_q_nb and d_q_row both NULL: no covisibility rows (q_cap is ignored); d_words /
 * d_score may be NULL.  n_q == 0: SS_OK, nothing written.  SS_ERR_STATE without a database.  SS_ERR_INVALID_ARG, with a message:
 * n_q outside 0 .. SS_PLACE_MAX_QUERIES, q_stride < 1, cand_cap outside 1 .. SS_PLACE_MAX_CANDIDATES, nb_cap or q_cap outside 1 ..
 * SS_PLACE_MAX_NEIGHBOURS, a NULL required buffer, a q_kf outside -1 .. n_db-1 or a q_problem outside the table, a q_problem that
 * contradicts q_kf, a parameter out of range, a reserved field that is not 0. */
int ss_place_query_device(ss_ctx *ctx, const void *d_q_word, const void *d_q_value, const void *d_q_count, int q_stride, int n_q,
                          const int32_t *q_kf, const int32_t *q_problem, const void *d_q_nb, const void *d_q_row, int q_cap,
                          const void *d_nb, int nb_cap, const ss_place_params *params, int cand_cap, void *d_cand, void *d_summary,
                          void *d_words, void *d_score);
/* One database and its queries with host pointers in and out, synchronous: uploads, ss_place_set_database, ss_place_query_device,
 * downloads.  The context's database is left cleared (its arrays were the call's own copies).  words / score may be NULL. */
int ss_place(ss_ctx *ctx, const int32_t *db_word, const double *db_value, const int32_t *db_count, const uint8_t *db_skip, int n_db,
             int stride, int n_words, const ss_gba_problem *problems, int n_problems, const int32_t *q_word, const double *q_value,
             const int32_t *q_count, int q_stride, int n_q, const int32_t *q_kf, const int32_t *q_problem, const int32_t *q_nb,
             const ss_covis_row *q_row, int q_cap, const int32_t *nb, int nb_cap, const ss_place_params *params, int cand_cap,
             ss_place_cand *cand, ss_place_summary *summary, int32_t *words, float *score);
/* The whole rule on the host from the text the kernels compile (csrc/ss_place_steps.h, csrc/ss_bow_merge.h); needs no device.
 * Arguments are ss_place's and are checked as the device calls check them: SS_ERR_INVALID_ARG, and the message in err (err_bytes
 * of it; NULL: none). */
int ss_place_query_host(const int32_t *db_word, const double *db_value, const int32_t *db_count, const uint8_t *db_skip, int n_db,
                        int stride, int n_words, const ss_gba_problem *problems, int n_problems, const int32_t *q_word,
                        const double *q_value, const int32_t *q_count, int q_stride, int n_q, const int32_t *q_kf,
                        const int32_t *q_problem, const int32_t *q_nb, const ss_covis_row *q_row, int q_cap, const int32_t *nb,
                        int nb_cap, const ss_place_params *params, int cand_cap, ss_place_cand *cand, ss_place_summary *summary,
                        int32_t *words, float *score, char *err, int err_bytes);

/* ---- undistorted keypoints, image bounds, RGB-D depth: what Frame's constructor does to the extractor's keypoints --
 * Frame::UndistortKeyPoints (mvKeysUn), Frame::ComputeImageBounds (mnMinX .. mnMaxY) and Frame::ComputeStereoFromRGBD (mvuRight,
 * mvDepth).  Every search and optimiser above takes its keypoints as undistorted; this family makes them so on the device, so that
 * the batch of a distorted camera stays in HBM from pixels to poses.  No ORB-SLAM3 source is in the reference tree: this is the
 * library's own restatement, oracle/vo_oracle.py::undistort and tests/undistort_ref.py are its normative statement, and parity with
 * the real binary stays unpinned.  DESIGN.md section 34.  An addition to ABI 5: nothing existing changes; ss_track keeps its own
 * host routine, which states the same rule.
 * 1. Undistortion.  Of a camera only fx fy cx cy k1 k2 p1 p2 are read.  If k1 == 0 && k2 == 0 && p1 == 0 && p2 == 0, x and y are
 *    copied bit for bit.  Otherwise, in double, one IEEE operation per step, left to right, no contraction:
 *      x0 = ((double)x - cx) / fx;  y0 = ((double)y - cy) / fy;  x = x0;  y = y0;
 *      five times:  r2 = x*x + y*y;  icdist = 1.0 / (1.0 + (k2*r2 + k1)*r2);
 *                   dx = 2*p1*x*y + p2*(r2 + 2*x*x);  dy = p1*(r2 + 2*y*y) + 2*p2*x*y;
 *                   x = (x0 - dx)*icdist;  y = (y0 - dy)*icdist;
 *      out.x = (float)(x*fx + cx);  out.y = (float)(y*fy + cy);      one rounding each: mvKeysUn is float32
 *    Host and device agree bit for bit on finite input; a non-finite coordinate goes through the same operations.  size, angle,
 *    response and octave are never touched.  Known differences from cv::undistortPoints as published: the rule divides by fx where
 *    OpenCV multiplies by 1/fx; OpenCV's bail-out for icdist < 0 is absent (tests/test_undistort_ref.py shows the denominator
 *    positive over the whole image for its cameras); K is taken in double where upstream holds it in float.
 * 2. Bounds.  All four coefficients zero: 0, width, 0, height.  Otherwise the corners c0 = (0,0), c1 = (w,0), c2 = (0,h),
 *    c3 = (w,h), as floats, go through rule 1, and min_x = min(c0.x, c2.x), max_x = max(c1.x, c3.x), min_y = min(c0.y, c1.y),
 *    max_y = max(c2.y, c3.y).
 * 3. RGB-D depth (Tracking::GrabImageRGBD, then ComputeStereoFromRGBD), all float32, one operation per step:
 *    1. inv = fabsf(depth_map_factor) < 1e-5f ? 1.0f : 1.0f / depth_map_factor.
 *    2. A uint16 sample becomes (float)raw * inv.  A float32 sample is multiplied by inv only when fabsf(inv - 1.0f) > 1e-5f.
 *    3. The sample is taken at column (int)x_raw, row (int)y_raw: truncation of the RAW position, as at<float>(v, u) does.  A
 *       position whose pixel lies outside the frame, or a NaN, has no sample.
 *    4. If d > 0 (a NaN fails): depth = d and right = x_undistorted - bf / d, one division and one subtraction.  Otherwise both
 *       are -1.0f.  Rows at or past a frame's count get -1.0f in both planes.
 *    right is the plane ss_pose_opt_*, ss_local_ba_* and ss_match_proj_* take as d_right / d_train_right. */
typedef struct {            /* 16 bytes */
    float bf;               /* baseline times fx (upstream's mbf); finite */
    float depth_map_factor; /* the calibration's; finite */
    float close_limit;      /* upstream's mThDepth: a depth in (0, close_limit) counts as close; summary only */
    int32_t depth_type;     /* 0: float32 samples, 1: uint16 samples */
} ss_depth_params;
typedef struct {            /* 16 bytes, one per frame */
    int32_t status;         /* SS_OK, or the frame_error that voided the frame (batch form: n_kp 0, every row -1.0f) */
    int32_t n_kp;           /* the count as used, clamped to 0 .. rows_per_frame */
    int32_t n_depth;        /* rows with depth > 0 */
    int32_t n_close;        /* rows with 0 < depth < close_limit */
} ss_depth_summary;
/* Rule 2; needs no device.  SS_ERR_INVALID_ARG: a NULL pointer, width <= 0, height <= 0, a non-finite one of the eight numbers
 * rule 1 reads, fx or fy equal to 0. */
int ss_undistort_bounds_host(const ss_camera *cam, float out[4] /* min_x, max_x, min_y, max_y */);
/* Overwrites the four bound fields of a view, and nothing else of it, with rule 2 of cam: for a view from ss_proj_view_init,
 * ss_fuse_view_sim3, ss_sim3_to_view or ss_sim3_to_view21, all of which set 0 .. width, 0 .. height.  Refusals as above. */
int ss_proj_view_set_bounds(ss_proj_view *view, const ss_camera *cam);
/* Rule 1 for n keypoints on the host from the text the kernel compiles; out may alias kp; other fields are copied.  Needs no
 * device.  SS_ERR_INVALID_ARG: a NULL pointer (n == 0 needs no arrays), n < 0, fx or fy not finite or equal to 0. */
int ss_undistort_host(const ss_camera *cam, const ss_keypoint *kp, int n, ss_keypoint *out);
/* Rule 1 on caller arrays: d_kp [n_frames][rows_per_frame] ss_keypoint, counts d_n_kp (device int32 [n_frames], clamped to 0 ..
 * rows_per_frame).  cams: a HOST table of n_cams cameras, n_cams == 1 (all frames) or n_cams == n_frames, copied before the call
 * returns.  d_kp_out [n_frames][rows_per_frame] may equal d_kp; otherwise whole records are written, every other field copied.
 * Rows at or past a frame's count are not written.  One launch, asynchronous on the context's stream.  SS_ERR_INVALID_ARG: a bad
 * frame or row count, n_cams neither 1 nor n_frames, a NULL buffer or table, fx or fy of a camera not finite or equal to 0. */
int ss_undistort_pairs_device(ss_ctx *ctx, const void *d_kp, const void *d_n_kp, int n_frames, int rows_per_frame,
                              const ss_camera *cams, int n_cams, void *d_kp_out);
/* The same on the frames of the last ss_extract_batch_device batch (SS_ERR_STATE without one; n_frames and kp_capacity are the
 * batch's); a frame whose frame_error is set counts as 0 rows.  cams == NULL: the calibration set last (n_cams is ignored;
 * SS_ERR_NOT_CALIBRATED without one).
 * d_kp_out != NULL: out of place, the batch is left as it is.
 * d_kp_out == NULL: IN PLACE.  The raw (x, y) pairs are first saved into an array of the context ([n_frames][kp_capacity][2]
 * float, allocated on first use, handed out by ss_get_batch_raw_xy), then x and y of the batch's own keypoints are overwritten.
 * From then on every *_batch_device call on that batch, ss_get_batch_view and ss_fetch_frame read mvKeysUn.  A second in-place call
 * on the same batch is SS_ERR_STATE and writes nothing; every new extraction clears the state.
 * ss_stereo_batch_device reads the positions as they are: its row bands and its disparity are those of rectified pairs, whose
 * coefficients are zero, and for zero coefficients the in-place form is a bit copy. */
int ss_undistort_batch_device(ss_ctx *ctx, const ss_camera *cams, int n_cams, void *d_kp_out /* NULL = in place */);
/* The raw pairs the in-place form saved, device [n_frames][kp_capacity][2] float (rows past a frame's count are unspecified);
 * valid until the next extraction.  SS_ERR_STATE while the current batch has not been undistorted in place. */
int ss_get_batch_raw_xy(ss_ctx *ctx, const float **d_xy);
/* bf = (float)(baseline * fx), depth_map_factor = (float) of the calibration's, close_limit = (float)(baseline * fx * th_depth / fx)
 * (upstream's mThDepth = mbf * ThDepth / fx, in double, left to right).  Needs no device.  SS_ERR_INVALID_ARG: a NULL pointer,
 * depth_type not 0 or 1. */
int ss_depth_params_from_camera(const ss_camera *cam, int depth_type, ss_depth_params *out);
/* Rule 3 for the n keypoints of one frame on the host from the text the kernel compiles.  depth: height rows of row_stride bytes,
 * width samples each.  kp_un == NULL: kp_raw serves as both.  right and depth_out are float [n]; summary may be NULL.  Needs no
 * device.  Refusals as for the device forms. */
int ss_depth_host(const ss_depth_params *p, const void *depth, int width, int height, int64_t row_stride, const ss_keypoint *kp_raw,
                  const ss_keypoint *kp_un, int n, float *right, float *depth_out, ss_depth_summary *summary);
/* Rule 3 on caller arrays.  d_depth: n_frames depth frames in device memory, frame b at d_depth + b * frame_stride, its rows
 * row_stride bytes apart (both in bytes, multiples of the sample size, as the base is).  d_kp_raw / d_kp_un
 * [n_frames][rows_per_frame] ss_keypoint, the raw and the undistorted keypoints (d_kp_un == NULL: d_kp_raw serves as both), counts
 * d_n_kp.  Outputs d_right / d_depth_out float [n_frames][rows_per_frame], every row written; d_summary [n_frames]
 * ss_depth_summary, its two counters by integer atomics (exact and order-free).  Two launches, asynchronous on the context's
 * stream.  SS_ERR_INVALID_ARG: a bad frame or row count, width or height outside 1 .. 16777216, strides smaller than the frame or
 * misaligned, depth_type not 0 or 1, bf, depth_map_factor or close_limit not finite, a NULL buffer. */
int ss_depth_pairs_device(ss_ctx *ctx, const ss_depth_params *p, const void *d_depth, int width, int height, int64_t row_stride,
                          int64_t frame_stride, const void *d_kp_raw, const void *d_kp_un, const void *d_n_kp, int n_frames,
                          int rows_per_frame, void *d_right, void *d_depth_out, void *d_summary);
/* The same on the frames of the last ss_extract_batch_device batch (SS_ERR_STATE without one; planes [n_frames][kp_capacity]).  A
 * batch that was undistorted in place: the saved raw pairs give the pixel, the batch's keypoints x_undistorted.  Otherwise the
 * batch's keypoints serve as both.  A frame whose frame_error is set gets that status and no depth. */
int ss_depth_batch_device(ss_ctx *ctx, const ss_depth_params *p, const void *d_depth, int width, int height, int64_t row_stride,
                          int64_t frame_stride, void *d_right, void *d_depth_out, void *d_summary);

/* ---- map points from depth: Frame::UnprojectStereo / KeyFrame::UnprojectStereo, Tracking::StereoInitialization, the close-point
 * rule of Tracking::CreateNewKeyFrame and Tracking::UpdateLastFrame and the close counts of Tracking::NeedNewKeyFrame: from the
 * depth per keypoint that ss_stereo_batch_device and ss_depth_*_device leave on the device to a block of ss_map_point that
 * ss_match_proj_* reads, without a round trip through the host.  No ORB-SLAM3 source is in the reference tree: this is the
 * library's own restatement, tests/unproject_ref.py is its normative statement, and parity with the real binary stays unpinned.
 * DESIGN.md section 35.  An addition to ABI 5: nothing existing changes; ss_triangulate_* keep treating every row as monocular, the
 * stereo form of the triangulation is ss_triangulate_stereo_* (with the epipolar family above).
 * Not built: the inertial 0.9996 parallax variant of the stereo triangulation (ss_triangulate_stereo_* are the plain rule), the order in which upstream numbers the created points (depth order; it affects ids only: a caller sorts the
 * few hundred created rows by depth if it needs that), inserting the points into a map, mnFound / mnVisible, wiring into ss_track
 * or the pipe, fisheye stereo.
 * Inputs per frame: undistorted keypoints and descriptors, a count clamped to 0 .. rows_per_frame, a depth plane (a pointer and
 * a byte stride per row: stride 4 reads the float plane ss_depth_*_device writes, stride 16 with the pointer at &points[0].depth
 * reads ss_stereo_point in place), has_point (uint8 per row, upstream's mvpMapPoints[i] && Observations() >= 1; NULL: no row has a
 * point), outlier (uint8 per row, or NULL) and one ss_unproject_view, made on the host by ss_unproject_view_init and handed to the
 * device calls as a HOST table that is copied before the call returns.  The view holds, in double, rcw and tcw as given, fx fy cx
 * cy, 1.0/fx, 1.0/fy and ow[k] = -((r[k]*t[0] + r[3+k]*t[1]) + r[6+k]*t[2]), as ss_epi_pair_init forms it.
 * The rule.  All arithmetic is in double, one IEEE operation per step, left to right, no contraction, no library function beyond
 * sqrt; every test is in its accepting form, so a NaN fails it.  scale[] is the pyramid table, n_levels entries.
 * 1. Row i is live iff i < n and depth_i > 0; otherwise its state is 3 (a row at or past the count: -1).  A live row whose octave
 *    is outside 0 .. n_levels - 1 has state 4 and takes no part in steps 2 - 6: it has no key and only n_depth counts it.
 * 2. The key of a live row is (uint64)bits(depth_i) << 32 | i: positive floats order as their bits, so this is std::sort on
 *    pair<float, int>.  rank_i is the number of live rows with a lower key; n_not_far the number with depth <= close_limit
 *    (upstream's break test is first > mThDepth); n_close the number with depth < close_limit (NeedNewKeyFrame, ss_depth_summary).
 * 3. SS_UNPROJECT_ALL (StereoInitialization): every live row is processed.  SS_UNPROJECT_CLOSE (CreateNewKeyFrame,
 *    UpdateLastFrame): row i iff rank_i <= max(n_not_far, max_points); upstream's max_points is 100.  This is the closed form of
 *    upstream's loop "nPoints++; if (depth > mThDepth && nPoints > maxPoint) break;" over the sorted pairs
 *    (tests/test_unproject_ref.py compares the two).  A live row that is not processed has state 2.
 * 4. A processed row is created (state 0) iff has_point is NULL or has_point[i] == 0; otherwise it is kept (state 1).
 * 5. The map point of a created row, (x, y) the keypoint and z = (double)depth: xc = ((x - cx)*z)*invfx, yc = ((y - cy)*z)*invfy;
 *    X[k] = ((rcw[k]*xc + rcw[3+k]*yc) + rcw[6+k]*z) + ow[k] (Rwc.xc + Ow); n = X - ow; d = sqrt((n0*n0 + n1*n1) + n2*n2).  The row
 *    has state 5, and no point, unless d > 0 and d is finite.  Normal n/d; max_dist = d*scale[octave]; min_dist = max_dist /
 *    scale[n_levels - 1]; the eight numbers rounded to float32 once each (MapPoint::UpdateNormalAndDepth with one observation).
 *    The descriptor is the row's own.
 * 6. Over the live rows with depth < close_limit: tracked iff has_point[i] != 0 and the row is no outlier (outlier NULL or
 *    outlier[i] == 0), untracked otherwise (NeedNewKeyFrame's nTrackedClose and nNonTrackedClose).
 * Outputs: one ss_unproject_info per row; the compact d_points / d_point_desc / d_point_rows (int32 (i, -1)) / d_n_points of the
 * state-0 rows in ascending row order, byte for byte the layout ss_triangulate_* write and ss_match_proj_pairs_device reads, with
 * the same alignment rules (the depth plane: 4 bytes); rows from n_points on are not written; the compaction is deterministic
 * whatever the schedule.  One ss_unproject_summary per frame; its counters are exact and order-free. */
#define SS_UNPROJECT_ALL 0
#define SS_UNPROJECT_CLOSE 1
#define SS_UNPROJECT_CREATED 0
#define SS_UNPROJECT_KEPT 1
#define SS_UNPROJECT_FAR 2
#define SS_UNPROJECT_NO_DEPTH 3
#define SS_UNPROJECT_OCTAVE 4
#define SS_UNPROJECT_DEGENERATE 5
typedef struct {            /* 168 bytes, one per frame (a HOST table) */
    double rcw[9], tcw[3];
    double fx, fy, cx, cy, invfx, invfy;
    double ow[3];
} ss_unproject_view;
typedef struct {            /* 16 bytes */
    int32_t mode;           /* SS_UNPROJECT_ALL or SS_UNPROJECT_CLOSE */
    int32_t max_points;     /* >= 0; upstream: 100; SS_UNPROJECT_CLOSE only */
    float close_limit;      /* upstream's mThDepth (ss_depth_params_from_camera's close_limit); finite */
    int32_t reserved;       /* 0 */
} ss_unproject_params;
typedef struct {            /* 4 bytes, one per row */
    int32_t state;          /* -1 at or past the count, else SS_UNPROJECT_CREATED .. SS_UNPROJECT_DEGENERATE */
} ss_unproject_info;
typedef struct {            /* 40 bytes, one per frame */
    int32_t status;         /* SS_OK, or the frame_error that voided the frame (batch form: n_kp 0, every row -1, no point) */
    int32_t n_kp;           /* the count as used, clamped to 0 .. rows_per_frame */
    int32_t n_depth;        /* rows with depth > 0 */
    int32_t n_close;        /* live rows with depth < close_limit */
    int32_t n_not_far;      /* live rows with depth <= close_limit */
    int32_t n_processed;    /* states 0, 1 and 5 */
    int32_t n_created;      /* state 0 = n_points */
    int32_t n_kept;         /* state 1 */
    int32_t n_tracked_close, n_untracked_close; /* step 6 */
} ss_unproject_summary;
/* Needs no device.  NULL pointer: SS_ERR_INVALID_ARG.  A pose or camera that is not finite gives state 5 for every created row. */
int ss_unproject_view_init(const ss_camera *cam, const double rcw[9], const double tcw[3], ss_unproject_view *out);
/* The whole rule for one frame on the host from the text the kernel compiles; needs no device.  The arrays have `rows` rows
 * (0 <= rows <= SS_GUIDED_MAX_ROWS), n is the told count (clamped); depth is row 0's, depth_stride bytes to the next.  info gets
 * rows entries, points / point_desc / point_rows their first *n_points.  SS_ERR_INVALID_ARG: as the device forms; 1 <= n_levels <=
 * SS_MAX_LEVELS. */
int ss_unproject_host(const ss_unproject_view *view, const ss_unproject_params *p, const float *scale, int n_levels, const ss_keypoint *kp,
                      const uint8_t *desc, int n, int rows, const void *depth, int64_t depth_stride, const uint8_t *has_point,
                      const uint8_t *outlier, ss_unproject_info *info, ss_map_point *points, uint8_t *point_desc, int32_t *point_rows,
                      int32_t *n_points, ss_unproject_summary *summary);
/* The rule on caller arrays of n_frames frames: d_kp / d_desc [n_frames][rows_per_frame], counts d_n_kp (device int32 [n_frames]),
 * d_has_point / d_outlier uint8 [n_frames][rows_per_frame] or NULL, views a HOST table of n_frames.  The depth planes are
 * n_depth_blocks blocks of rows_per_frame rows: frame b reads block depth_src[b] (a HOST table of n_frames, copied before the call
 * returns; NULL: block b, and n_depth_blocks >= n_frames), the depth of its row i at d_depth + (depth_src[b] * rows_per_frame + i) *
 * depth_stride; depth_src[b] == -1: the frame has no depth plane, nothing is read for it and none of its rows has a depth (the
 * right-eye frames of a stereo batch, whose left eye 2p reads block p of ss_stereo_batch_device's points).  n_depth_blocks and
 * depth_src are this library's addition to the interface first planned for the family (a pointer and a stride alone): without them
 * the batch form would read past the [pairs][kp_capacity] points of a stereo batch for its last right eye.
 * Outputs: d_info [n_frames][rows_per_frame] ss_unproject_info (every row written), the compact blocks [n_frames][rows_per_frame] with d_n_points int32 [n_frames], d_summary [n_frames].  The
 * pyramid table is the context's.  One launch, asynchronous on the context's stream.  SS_ERR_INVALID_ARG: a bad frame or row count
 * (rows_per_frame above SS_GUIDED_MAX_ROWS), a bad mode, max_points < 0, a close_limit that is not finite, reserved not 0, a
 * depth_stride that is not a positive multiple of 4, a depth pointer that is no multiple of 4, n_depth_blocks < 1, a depth_src entry
 * outside -1 .. n_depth_blocks - 1, a NULL required buffer or table; the context stays usable. */
int ss_unproject_pairs_device(ss_ctx *ctx, const void *d_kp, const void *d_desc, const void *d_n_kp, const void *d_depth, int64_t depth_stride,
                              int n_depth_blocks, const int32_t *depth_src, const void *d_has_point, const void *d_outlier, int n_frames, int rows_per_frame, const ss_unproject_view *views,
                              const ss_unproject_params *p, void *d_info, void *d_points, void *d_point_desc, void *d_point_rows,
                              void *d_n_points, void *d_summary);
/* The same on the frames of the last ss_extract_batch_device batch (SS_ERR_STATE without one; rows_per_frame = kp_capacity, which
 * must not exceed SS_GUIDED_MAX_ROWS).  It reads the batch's keypoints as they are: after an in-place ss_undistort_batch_device
 * that is mvKeysUn.  A frame whose frame_error is set gets that status and no rows. */
int ss_unproject_batch_device(ss_ctx *ctx, const void *d_depth, int64_t depth_stride, int n_depth_blocks, const int32_t *depth_src,
                              const void *d_has_point, const void *d_outlier, const ss_unproject_view *views, const ss_unproject_params *p, void *d_info, void *d_points, void *d_point_desc,
                              void *d_point_rows, void *d_n_points, void *d_summary);
/* One frame of n rows (0 .. SS_GUIDED_MAX_ROWS) in host memory, synchronous; outputs as ss_unproject_host's with rows = n. */
int ss_unproject(ss_ctx *ctx, const ss_unproject_view *view, const ss_unproject_params *p, const ss_keypoint *kp, const uint8_t *desc, int n,
                 const void *depth, int64_t depth_stride, const uint8_t *has_point, const uint8_t *outlier, ss_unproject_info *info,
                 ss_map_point *points, uint8_t *point_desc, int32_t *point_rows, int32_t *n_points, ss_unproject_summary *summary);

int ss_synchronize(ss_ctx *ctx);
/* Orders the context's stream after everything enqueued so far on another stream of the same device
 * (hipStream_t; NULL = the legacy default stream): for callers that produce the inputs of a *_device call on their own
 * stream (a collective's output, a decoder) and must not launch the match before they are written. */
int ss_wait_stream(ss_ctx *ctx, void *hip_stream);
/* the hipStream_t every kernel of this context is launched on */
int ss_get_stream(ss_ctx *ctx, void **hip_stream);

/* Per-kernel HIP-event timing on the context's stream (off by default). */
int ss_profile_enable(ss_ctx *ctx, int on);
int ss_profile_reset(ss_ctx *ctx);
/* fills up to max_stages entries, returns the number of stages (or < 0) */
int ss_stats(ss_ctx *ctx, ss_stage_stats *out, int max_stages);

/* Intermediate buffers of the last batch, for stage-by-stage parity tests.  what:
 * 0 pyramid level, 1 blurred level, 2 FAST score map (tight w*h u8 each; no kernel reads the map, so it
 * is not kept in normal operation: the first request allocates it, re-runs the FAST kernel on the last
 * batch's pyramid, and the context keeps it from then on); 3 candidates,
 * 4 quadtree-selected keypoints of a level (int32 triples x, y, response; candidates are
 * relative to the (16,16) border origin, selected are level coordinates); 5 two int32: the kernel that
 * built the level in the last batch (0 level 0, 1 k_resize, 2 / 5 k_resize_walk with bands of 32 / 16 rows,
 * 3 k_resize_pair, 4 k_resize_lds) and whether the batch's level 0 was read in place from the caller's buffer.  Returns the number
 * of bytes written to dst (<= dst_bytes) or < 0. */
int ss_debug_fetch(ss_ctx *ctx, int what, int frame, int level, void *dst, int64_t dst_bytes);
/* Test hook: sorts n <= 2048 items in place with the device's restatement of libstdc++
 * std::sort for ORB-SLAM3's compareNodes.  Item = size << 32 | UL.x << 20 | id (20 bits); the
 * comparator looks at (size, UL.x) only, so the placement of equal keys is what is tested. */
int ss_debug_sort(ss_ctx *ctx, uint64_t *items, int n);

/* ---- pipelined host-memory path ----------------------------------------------------------------------------
 * A pipe owns a ring of `depth` slots.  A slot = pinned host memory for `batch` frames + its own extraction
 * context (HBM buffers, HIP stream) + pinned host memory for the results.  Producer side: ss_pipe_acquire hands out
 * a free slot, the caller decodes / receives / copies frames straight into slot.pixels (frame i at
 * pixels + i * frame_stride, rows of row_stride bytes) and calls ss_pipe_submit; or ss_pipe_submit_frames gathers
 * caller-owned frames into a slot with a few host threads and submits it.  Submission enqueues, on the slot's stream,
 * H2D copy -> extraction (-> match) -> D2H copy of the results and returns at once, so the copies of one batch overlap
 * the kernels of the others.  Consumer side: ss_pipe_wait / ss_pipe_poll return completed batches in submission
 * order; the result arrays are the slot's pinned host memory and stay valid until ss_pipe_release(slot), which puts
 * the slot back into the ring.  A frame that is bad (NULL pointer, camera id 0) or exceeds an internal capacity gets
 * its own status; the other frames of the batch are unaffected (the shim's log-and-skip policy :523-551).
 * One producer thread and one consumer thread (or one thread doing both) per pipe. */
typedef struct ss_pipe ss_pipe;

typedef struct {
    int32_t width, height, channels; /* every frame of the pipe has this shape */
    int32_t batch;                   /* frames per slot, 1..256 */
    int32_t depth;                   /* slots, 2..16 */
    int32_t match_mode;              /* -1 none; 0 self-match; 1 frame b against frame b-1 of the batch (ss_match_batch_device);
                                      * 2 each frame against the previous frame of its own camera (below) */
    int32_t match_th, ratio_num, ratio_den; /* 0 0 0 = the defaults 50, 9, 10 */
    int32_t copy_threads;            /* host threads of ss_pipe_submit_frames; 0 = 4 */
} ss_pipe_config;

typedef struct {
    int32_t slot;
    uint8_t *pixels; /* pinned host memory, batch * frame_stride bytes */
    int64_t row_stride, frame_stride;
} ss_pipe_slot;

typedef struct {
    int32_t slot;
    int32_t n_frames;
    int32_t kp_capacity;          /* rows per frame in the per-keypoint arrays */
    uint64_t sequence;            /* 0, 1, 2 ... in submission order */
    const int32_t *status;        /* [n_frames] SS_OK or the frame's ss_status */
    const int32_t *camera_id;     /* [n_frames] as submitted */
    const double *timestamp;      /* [n_frames] as submitted */
    const int32_t *n_keypoints;   /* [n_frames]; 0 for a frame whose status is not SS_OK */
    const int32_t *level_counts;  /* [n_frames][SS_MAX_LEVELS] */
    const ss_keypoint *keypoints; /* [n_frames][kp_capacity] */
    const uint8_t *descriptors;   /* [n_frames][kp_capacity][32] */
    const int32_t *match_idx;     /* [n_frames][kp_capacity], NULL when match_mode < 0; match_mode 1: all -1 for a frame whose train frame (the one before) is bad */
    const uint16_t *match_d1, *match_d2;
    const void *d_descriptors;    /* DEVICE copy of `descriptors` (same layout), valid until ss_pipe_release */
} ss_pipe_result;

/* cam may be NULL for 1-channel frames (its rgb flag decides the gray weights of 3/4-channel frames) */
int ss_pipe_create(int device_ordinal, const ss_orb_params *params, const ss_camera *cam,
                   const ss_pipe_config *cfg, ss_pipe **out);
int ss_pipe_destroy(ss_pipe *pipe);
/* pipe may be NULL: message of the last failed ss_pipe_create on this thread */
const char *ss_pipe_last_error(const ss_pipe *pipe);
int ss_pipe_acquire(ss_pipe *pipe, ss_pipe_slot *out);
/* camera_ids / timestamps: n_frames entries each, or NULL (camera 1, timestamp 0) */
int ss_pipe_submit(ss_pipe *pipe, int slot, int n_frames, const int32_t *camera_ids, const double *timestamps);
/* frames[i]: caller-owned host image of the pipe's shape with rows of row_stride bytes (NULL = a bad frame);
 * consumed before the call returns.  SS_ERR_BUSY when no slot is free (ss_pipe_last_error is not updated for SS_ERR_BUSY:
 * producers poll it). */
int ss_pipe_submit_frames(ss_pipe *pipe, const uint8_t *const *frames, int n_frames, int64_t row_stride,
                          const int32_t *camera_ids, const double *timestamps);
/* oldest submitted batch: wait blocks until it has completed; poll returns 1 (completed, *out filled), 0 (still
 * running, or nothing submitted) or < 0 */
int ss_pipe_wait(ss_pipe *pipe, ss_pipe_result *out);
int ss_pipe_poll(ss_pipe *pipe, ss_pipe_result *out);
int ss_pipe_release(ss_pipe *pipe, int slot);
/* batches submitted and not yet returned by wait / poll */
int ss_pipe_in_flight(const ss_pipe *pipe);
/* match_mode 2 (several cameras in one stream): a frame's train is the latest earlier frame, in submission order across
 * batches, with the same camera_id and a producer-side status of SS_OK (a NULL frame, camera id 0).  The train table is
 * built at submission (ss_match_batch_sources_device).  A train in an earlier batch comes from the pipe's carry: the last
 * such frame of up to SS_MAX_CAMERAS cameras, updated on the device after each batch's match by one gather launch; a
 * batch's match waits for the previous batch's carry update, extractions of different slots still overlap.  Frames of
 * further cameras get trains inside their batch only.  A submission that fails half-way empties the carry: the next
 * batch's first frame of each camera then has no train.  A frame whose train turns out bad on the device (SS_ERR_OVERFLOW)
 * gets match_idx -1, as in mode 1.
 * ss_pipe_match_sources: for each frame of a returned, unreleased slot of a mode-2 pipe, the (sequence, index in its batch)
 * of the frame it was matched against, or -1 / -1 (no train, or its matches were voided); arrays of n_frames entries.
 * SS_ERR_STATE for another mode or slot state. */
int ss_pipe_match_sources(const ss_pipe *pipe, int slot, int64_t *train_sequence, int32_t *train_frame);
/* Test hook: the next submission fails (SS_ERR_HIP, "injected failure ...") after `after_operations` of its enqueues have
 * been issued.  A submission that fails half-way drains its streams before it returns, leaves the slot ACQUIRED (release or
 * resubmit it) and the pipe usable; ss_pipe_submit_frames frees its slot itself. */
int ss_pipe_debug_inject_failure(ss_pipe *pipe, int after_operations);

#ifdef __cplusplus
}
#endif
#endif
