"""The host-side contract of the search family of the C ABI (guided matching, projection search, bag of words, epipolar search,
triangulation): what each pairs, batch and host entry answers to a broken argument -- the status code, the full message, which of
two broken arguments is reported -- and which stages a call records for ss_stats, how often, with how many algorithmic bytes.
The messages are those of the source; the byte figures are computed here from the formulas next to each stage_timer.  Nothing here
looks at a match: tests/test_guided.py, test_proj.py, test_bow.py and test_epi.py do that."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import epi_cases as EC
import guided_cases as G

pytestmark = pytest.mark.gpu

F, ROWS = 2, 64  # the pairs forms: 2 frames of 64 rows
NAMES = ["synth_t0", "synth_t1"]  # the batch forms: 2 frames of 320 x 240
VOC_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bow", "k3_vocabulary.txt")
MAX = 16384  # SS_GUIDED_MAX_ROWS, SS_BOW_MAX_ROWS
OK, INVALID, STATE = 0, -1, -9
DESC = 32

SIGNATURES = {
    "ss_match_guided_pairs_device": "d_query d_query_kp d_n_query d_train d_train_kp d_n_train d_windows n_frames rows p d_idx d_d1 d_d2 d_summary",
    "ss_match_guided_batch_device": "train_src d_windows p d_idx d_d1 d_d2 d_summary",
    "ss_match_guided": "query query_kp n_query train train_kp n_train windows p idx d1 d2 summary",
    "ss_match_proj_pairs_device": "d_points d_point_desc d_n_points n_blocks point_rows d_train d_train_kp d_n_train d_train_right d_train_taken "
                                  "n_frames rows views point_src p d_idx d_d1 d_d2 d_proj d_summary",
    "ss_match_proj_batch_device": "d_points d_point_desc d_n_points n_blocks point_rows d_train_right d_train_taken views point_src p d_idx d_d1 "
                                  "d_d2 d_proj d_summary",
    "ss_match_proj": "view points point_desc n_points train train_kp n_train train_right train_taken p idx d1 d2 proj summary",
    "ss_bow_transform_device": "d_desc d_n_rows n_frames rows levelsup d_word d_node d_bow_word d_bow_value d_summary",
    "ss_bow_transform_batch_device": "levelsup d_word d_node d_bow_word d_bow_value d_summary",
    "ss_match_bow_pairs_device": "d_query d_query_kp d_query_node d_n_query d_train d_train_kp d_train_node d_n_train n_frames rows p d_idx d_d1 "
                                 "d_d2 d_summary",
    "ss_match_bow_batch_device": "train_src p d_idx d_d1 d_d2 d_summary",
    "ss_bow_score_device": "d_q_word d_q_value d_q_count q_rows d_db_word d_db_value d_db_count n_db stride d_score",
    "ss_match_epi_pairs_device": "d_query d_query_kp d_query_node d_query_taken d_n_query d_train d_train_kp d_train_node d_train_taken d_n_train "
                                 "n_frames rows pairs p d_idx d_d1 d_summary",
    "ss_match_epi_batch_device": "train_src d_taken pairs p d_idx d_d1 d_summary",
    "ss_triangulate_pairs_device": "d_query d_query_kp d_n_query d_train_kp d_n_train d_idx n_frames rows pairs p d_info d_points d_point_desc "
                                   "d_point_rows d_n_points d_summary",
    "ss_triangulate_batch_device": "train_src d_idx pairs p d_info d_points d_point_desc d_point_rows d_n_points d_summary",
}
RATIO = " ratio_num and ratio_den must be 0 .. 32767 (ratio_den 0 = no ratio test)"
NO_FRAME = " names no frame of the batch (2); "


def _too_many(form, rows=MAX + 1):
    return f"{form}: rows_per_frame {rows} exceeds SS_GUIDED_MAX_ROWS ({MAX})"


class Arrays:
    """the operands of every form, on the device and on the host; `keep` holds what the raw pointers point into"""

    def __init__(self, binding, rows):
        import torch
        self.binding, self.rows, self.keep = binding, rows, []
        dev = torch.device("cuda:0")
        kp = np.zeros((F, rows), binding.KP_DTYPE)
        desc = np.zeros((F, rows, DESC), np.uint8)
        for b, name in enumerate(NAMES):
            k, d = G.features(name)
            kp[b, :ROWS], desc[b, :ROWS] = k[:ROWS], d[:ROWS]
        self.host = dict(kp=kp, desc=desc, windows=np.stack([G.own_windows(kp[b]) for b in range(F)]),
                         counts=np.full(F, ROWS, np.int32), node=np.ascontiguousarray(np.broadcast_to(np.arange(rows, dtype=np.int32) % 7, (F, rows))),
                         points=np.zeros((F, rows), binding.MAP_POINT_DTYPE), idx=np.full((F, rows), -1, np.int32))
        self.d = {}
        for name, a in self.host.items():
            t = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(F, -1)).to(dev)
            self.keep.append(t)
            self.d[name] = t.data_ptr()
        scratch = torch.zeros((16, F * rows * 64), dtype=torch.uint8, device=dev)  # one row per output: the largest is 32 bytes a row
        self.keep.append(scratch)
        self.out = [scratch[k].data_ptr() for k in range(16)]
        torch.cuda.synchronize()  # the library's stream does not wait for torch's
        pair = EC.library_pair(binding, EC.pose(None), EC.pose(0))
        self.pairs = (binding.EpiPair * F)(pair, pair)
        cam = binding.Camera(fx=EC.CAM[0], fy=EC.CAM[1], cx=EC.CAM[2], cy=EC.CAM[3], width=G.W, height=G.H)
        view = binding.proj_view(cam, np.eye(3), np.zeros(3))
        self.views = (binding.ProjView * F)(view, view)
        self.h_out = [np.zeros(rows * 64, np.uint8) for _ in range(4)]
        self.guided_summary, self.proj_summary = binding.GuidedSummary(), binding.ProjSummary()

    def guided(self, **kw):
        return self.binding.guided_params(**dict(dict(orientation=1, extent_w=G.W, extent_h=G.H), **kw))

    def proj(self, **kw):
        return self.binding.proj_params(**dict(dict(extent_w=G.W, extent_h=G.H), **kw))

    def good(self, fn):
        """the arguments of a call of `fn` that succeeds"""
        d, o, h = self.d, self.out, self.host
        sides = dict(d_query=d["desc"], d_query_kp=d["kp"], d_n_query=d["counts"], d_train=d["desc"], d_train_kp=d["kp"], d_n_train=d["counts"],
                     d_query_node=d["node"], d_train_node=d["node"], d_query_taken=0, d_train_taken=0, d_train_right=0, d_taken=0, n_frames=F,
                     rows=self.rows, train_src=None)
        outs = dict(d_idx=o[0], d_d1=o[1], d_d2=o[2], d_summary=o[3], d_proj=o[4], d_info=o[4], d_points=o[5], d_point_desc=o[6], d_point_rows=o[7],
                    d_n_points=o[8], d_word=o[4], d_node=o[5], d_bow_word=o[6], d_bow_value=o[7])
        own = {
            "ss_match_guided_pairs_device": dict(d_windows=d["windows"], p=self.guided()),
            "ss_match_guided_batch_device": dict(d_windows=0, p=self.guided(radius=15.0, radius_by_octave=True, octave_span=1)),
            "ss_match_guided": dict(query=h["desc"][0], query_kp=h["kp"][0], n_query=ROWS, train=h["desc"][1], train_kp=h["kp"][1], n_train=ROWS,
                                    windows=h["windows"][0], p=self.guided(), idx=self.h_out[0], d1=self.h_out[1], d2=self.h_out[2],
                                    summary=self.guided_summary),
            "ss_match_proj_pairs_device": dict(d_points=d["points"], d_n_points=d["counts"], n_blocks=F, point_rows=self.rows, views=self.views,
                                               point_src=None, p=self.proj()),
            "ss_match_proj_batch_device": dict(d_points=d["points"], d_n_points=d["counts"], n_blocks=F, point_rows=ROWS, views=self.views,
                                               point_src=None, p=self.proj()),
            "ss_match_proj": dict(view=self.views, points=h["points"][0], point_desc=h["desc"][0], n_points=ROWS, train=h["desc"][1],
                                  train_kp=h["kp"][1], n_train=ROWS, train_right=None, train_taken=None, p=self.proj(), idx=self.h_out[0],
                                  d1=self.h_out[1], d2=self.h_out[2], proj=self.h_out[3], summary=self.proj_summary),
            "ss_bow_transform_device": dict(d_desc=d["desc"], d_n_rows=d["counts"], levelsup=2),
            "ss_bow_transform_batch_device": dict(levelsup=2),
            "ss_match_bow_pairs_device": dict(p=self.guided()),
            "ss_match_bow_batch_device": dict(p=self.guided()),
            "ss_bow_score_device": dict(d_q_word=o[4], d_q_value=o[5], d_q_count=o[6], q_rows=4, d_db_word=o[7], d_db_value=o[8], d_db_count=o[9],
                                        n_db=1, stride=4, d_score=o[10]),
            "ss_match_epi_pairs_device": dict(pairs=self.pairs, p=self.binding.epi_params()),
            "ss_match_epi_batch_device": dict(pairs=self.pairs, p=self.binding.epi_params()),
            "ss_triangulate_pairs_device": dict(d_idx=d["idx"], pairs=self.pairs, p=self.binding.tri_params()),
            "ss_triangulate_batch_device": dict(d_idx=d["idx"], pairs=self.pairs, p=self.binding.tri_params()),
        }[fn]
        if fn.startswith("ss_match_proj"):
            own["d_point_desc"] = d["desc"]
        return dict(dict(sides, **outs), **own)


def _raw(v):
    """a value as ctypes takes it: None is NULL, arrays and structures go by address"""
    if isinstance(v, np.ndarray):
        return v.ctypes.data
    if isinstance(v, C.Array):
        return C.addressof(v)
    if isinstance(v, C.Structure):
        return C.byref(v)
    return v


def call(ctx, arrays, fn, **broken):
    """`fn` with its good arguments but for `broken` -> (status, message); a params field is broken as p__field"""
    args = arrays.good(fn)
    for name, v in broken.items():
        if name.startswith("p__"):
            setattr(args["p"], name[3:], v)
        elif name == "all_buffers_null":
            for k in args:
                if k not in ("n_frames", "rows", "n_blocks", "point_rows", "levelsup", "q_rows", "n_db", "stride", "p"):
                    args[k] = None
        else:
            assert name in args, name
            args[name] = np.asarray(v, np.int32) if name in ("train_src", "point_src") and v is not None else v
    rc = getattr(ctx._lib, fn)(ctx._h, *[_raw(args[name]) for name in SIGNATURES[fn].split()])
    return rc, (ctx.last_error() if rc != OK else "")


def _refused(ctx, arrays, table):
    for fn, broken, code, message in table:
        got = call(ctx, arrays, fn, **broken)
        assert got == (code, message), f"{fn}({broken}): {got} != {(code, message)}"


def _pairs_table(fn, form, what, params, rules="{form}"):
    """what every pairs form shares; `params`: (broken arguments, message) of its params rules, the first of them first; `rules`:
    the form its params rules speak of"""
    no_params = f"{rules.format(form=form)}: params is NULL"
    t = [(fn, dict(p=None), INVALID, no_params)]
    t += [(fn, b, INVALID, m) for b, m in params]
    t += [(fn, dict(n_frames=-1), INVALID, f"{form}: bad {what} or row count"),
          (fn, dict(rows=0), INVALID, f"{form}: bad {what} or row count"),
          (fn, dict(rows=MAX + 1), INVALID, _too_many(form)),
          (fn, dict(d_train_kp=None), INVALID, f"{form}: NULL buffer"),
          (fn, dict(d_summary=None), INVALID, f"{form}: NULL buffer"),
          (fn, dict(n_frames=0, all_buffers_null=True), OK, ""),
          # the order: params, the counts, the rows, the buffers
          (fn, dict(p=None, n_frames=-1), INVALID, no_params),
          (fn, dict(dict(params[0][0]), rows=0), INVALID, params[0][1]),
          (fn, dict(n_frames=-1, rows=MAX + 1), INVALID, f"{form}: bad {what} or row count"),
          (fn, dict(rows=MAX + 1, d_idx=None), INVALID, _too_many(form)),
          (fn, dict(n_frames=0, rows=MAX + 1), INVALID, _too_many(form))]
    return t


GUIDED_RULES = [(dict(p__ratio_num=-1), "guided match:" + RATIO), (dict(p__ratio_den=32768), "guided match:" + RATIO),
                (dict(p__orientation=3), "guided match: orientation must be 0, 1 or 2"),
                (dict(p__ratio_num=40000, p__orientation=-1), "guided match:" + RATIO)]
EPI_RULES = [(dict(p__th=-1), "epipolar search: th must be 0 .. 256"), (dict(p__th=257), "epipolar search: th must be 0 .. 256"),
             (dict(p__orientation=3), "epipolar search: orientation must be 0, 1 or 2"),
             (dict(p__th=300, p__orientation=3), "epipolar search: th must be 0 .. 256")]
PROJ_RULES = [(dict(p__th=0.0), "projection search: th must be finite and > 0"), (dict(p__th=math.inf), "projection search: th must be finite and > 0"),
              (dict(p__view_cos_limit=math.nan), "projection search: view_cos_limit is NaN"),
              (dict(p__th_high=257), "projection search: th_high must be 0 .. 256"), (dict(p__ratio_den=-1), "projection search:" + RATIO),
              (dict(p__th=-1.0, p__th_high=-1), "projection search: th must be finite and > 0")]
PROJ_COUNT = "projection search: bad frame, block or row count"
PROJ_NULL = "projection search: NULL buffer"


def _proj_too_many(point_rows, rows):
    return f"projection search: point_rows {point_rows} / rows_per_frame {rows} exceed SS_GUIDED_MAX_ROWS ({MAX})"


def _proj_shared(fn, rows):
    """what the two device forms of the projection search share (proj_run); `rows`: the rows of a train frame"""
    t = [(fn, dict(p=None), INVALID, "projection search: params is NULL")]
    t += [(fn, b, INVALID, m) for b, m in PROJ_RULES]
    t += [(fn, dict(n_blocks=-1), INVALID, PROJ_COUNT), (fn, dict(point_rows=0), INVALID, PROJ_COUNT),
          (fn, dict(point_rows=MAX + 1), INVALID, _proj_too_many(MAX + 1, rows)),
          (fn, dict(views=None), INVALID, "projection search: views is NULL"),
          (fn, dict(point_src=[0, 2]), INVALID, "point_src[1] = 2 names no block of points (2)"),
          (fn, dict(point_src=[-1, 0]), INVALID, "point_src[0] = -1 names no block of points (2)"),
          (fn, dict(n_blocks=1), INVALID, "frame [1] = 1 names no block of points (1)"),
          (fn, dict(d_points=None), INVALID, PROJ_NULL), (fn, dict(d_proj=None), INVALID, PROJ_NULL),
          (fn, dict(p__check_right=1), INVALID, "projection search: check_right needs the right coordinates of the train rows"),
          # the order: params, the counts, the rows, the views, the blocks, the buffers, the right coordinates
          (fn, dict(p__th=0.0, n_blocks=-1), INVALID, "projection search: th must be finite and > 0"),
          (fn, dict(point_rows=0, views=None), INVALID, PROJ_COUNT),
          (fn, dict(views=None, point_src=[0, 2]), INVALID, "projection search: views is NULL"),
          (fn, dict(point_src=[2, 0], d_points=None), INVALID, "point_src[0] = 2 names no block of points (2)"),
          (fn, dict(d_idx=None, p__check_right=1), INVALID, PROJ_NULL)]
    return t


def _batch_table(fn, form, what):
    """what the batch forms with a train table share, on a batch that is ready for them"""
    return [(fn, dict(p=None), INVALID, f"{form}: params is NULL"),
            (fn, dict(train_src=[0, F]), INVALID, f"train_src[1] = {F}" + NO_FRAME + f"the {what} takes no carry frames"),
            (fn, dict(train_src=[-2, 0]), INVALID, "train_src[0] = -2" + NO_FRAME + f"the {what} takes no carry frames"),
            (fn, dict(train_src=[-1, 0]), OK, ""),
            # the order: params, the outputs, the train table
            (fn, dict(p=None, d_idx=None), INVALID, f"{form}: params is NULL"),
            (fn, dict(p=None, train_src=[5, 5]), INVALID, f"{form}: params is NULL")]


def _extract(ctx):
    import torch
    frames = torch.from_numpy(np.stack([G.frame(n) for n in NAMES])).to("cuda:0")
    ctx.extract_batch_device(frames.data_ptr(), F, G.W, G.H)
    ctx.synchronize()
    return ctx.batch_view().kp_capacity


def test_error_table():
    """one context through its states: fresh, with a vocabulary, with a batch, with the batch transformed"""
    from send_slam_amd import binding
    assert MAX == binding.SS_GUIDED_MAX_ROWS == binding.SS_BOW_MAX_ROWS
    no_batch = ": no batch has been extracted"
    no_transform = ": the last batch has not been through ss_bow_transform_batch_device"
    with binding.OrbContext(0, n_features=G.NF, max_batch=F) as ctx:
        a = Arrays(binding, ROWS)
        # ---- the pairs forms and the host forms need no state
        g, b, e, t = "ss_match_guided_pairs_device", "ss_match_bow_pairs_device", "ss_match_epi_pairs_device", "ss_triangulate_pairs_device"
        _refused(ctx, a, _pairs_table(g, "guided match", "frame", GUIDED_RULES))
        _refused(ctx, a, [(g, dict(p__extent_w=0), INVALID, "guided match: extent_w and extent_h must be > 0"),
                          (g, dict(p__extent_h=-1), INVALID, "guided match: extent_w and extent_h must be > 0"),
                          (g, dict(d_windows=None), INVALID, "guided match: NULL buffer"),
                          (g, dict(rows=MAX + 1, p__extent_w=0), INVALID, _too_many("guided match")),
                          (g, dict(n_frames=0, p__extent_w=0), INVALID, "guided match: extent_w and extent_h must be > 0"),
                          (g, dict(p__extent_h=0, d_query=None), INVALID, "guided match: extent_w and extent_h must be > 0")])
        _refused(ctx, a, _pairs_table(b, "bow match", "frame", GUIDED_RULES, rules="guided match"))
        _refused(ctx, a, [(b, dict(d_query_node=None), INVALID, "bow match: NULL buffer")])
        _refused(ctx, a, _pairs_table(e, "epipolar search", "pair", EPI_RULES))
        _refused(ctx, a, [(e, dict(pairs=None), INVALID, "epipolar search: NULL buffer"), (e, dict(d_train_node=None), INVALID, "epipolar search: NULL buffer")])
        _refused(ctx, a, _pairs_table(t, "triangulation", "pair", [(dict(p=None), "triangulation: params is NULL")]))
        _refused(ctx, a, [(t, dict(pairs=None), INVALID, "triangulation: NULL buffer"), (t, dict(d_idx=None), INVALID, "triangulation: NULL buffer")])
        pp = "ss_match_proj_pairs_device"
        _refused(ctx, a, _proj_shared(pp, ROWS))
        _refused(ctx, a, [(pp, dict(n_frames=-1), INVALID, PROJ_COUNT), (pp, dict(rows=0), INVALID, PROJ_COUNT),
                          (pp, dict(rows=MAX + 1), INVALID, _proj_too_many(ROWS, MAX + 1)),
                          (pp, dict(p__extent_w=0), INVALID, "projection search: extent_w and extent_h must be > 0"),
                          (pp, dict(d_train=None), INVALID, PROJ_NULL),
                          (pp, dict(n_frames=0, all_buffers_null=True), OK, ""),
                          (pp, dict(rows=MAX + 1, p__extent_h=0), INVALID, _proj_too_many(ROWS, MAX + 1)),
                          (pp, dict(n_frames=0, p__extent_h=0), INVALID, "projection search: extent_w and extent_h must be > 0"),
                          (pp, dict(n_frames=0, p=None), INVALID, "projection search: params is NULL")])
        hg, hp = "ss_match_guided", "ss_match_proj"
        counts = "guided match: n_query and n_train must be 0 .. SS_GUIDED_MAX_ROWS"
        _refused(ctx, a, [(hg, dict(n_query=-1), INVALID, counts), (hg, dict(n_train=MAX + 1), INVALID, counts),
                          (hg, dict(query=None), INVALID, "guided match: NULL buffer"), (hg, dict(summary=None), INVALID, "guided match: NULL buffer"),
                          (hg, dict(p=None), INVALID, "guided match: params is NULL"),
                          (hg, dict(p__orientation=3), INVALID, "guided match: orientation must be 0, 1 or 2"),
                          (hg, dict(p__extent_w=0), INVALID, "guided match: extent_w and extent_h must be > 0"),
                          (hg, dict(n_query=-1, p=None), INVALID, counts), (hg, dict(train_kp=None, p=None), INVALID, "guided match: NULL buffer")])
        counts = "projection search: n_points and n_train must be 0 .. SS_GUIDED_MAX_ROWS"
        _refused(ctx, a, [(hp, dict(n_points=-1), INVALID, counts), (hp, dict(n_train=MAX + 1), INVALID, counts),
                          (hp, dict(view=None), INVALID, PROJ_NULL), (hp, dict(points=None), INVALID, PROJ_NULL),
                          (hp, dict(p=None), INVALID, "projection search: params is NULL"),
                          (hp, dict(p__th=0.0), INVALID, "projection search: th must be finite and > 0"),
                          (hp, dict(p__extent_h=0), INVALID, "projection search: extent_w and extent_h must be > 0"),
                          (hp, dict(p__check_right=1), INVALID, "projection search: check_right needs the right coordinates of the train rows"),
                          (hp, dict(n_points=MAX + 1, p=None), INVALID, counts), (hp, dict(summary=None, p=None), INVALID, PROJ_NULL)])
        s = "ss_bow_score_device"
        _refused(ctx, a, [(s, dict(n_db=-1), INVALID, "bow score: bad vector count, stride or query size"),
                          (s, dict(stride=0), INVALID, "bow score: bad vector count, stride or query size"),
                          (s, dict(q_rows=0, d_score=None), INVALID, "bow score: bad vector count, stride or query size"),
                          (s, dict(d_db_count=None), INVALID, "bow score: NULL buffer"), (s, dict(n_db=0, all_buffers_null=True), OK, "")])
        # ---- a fresh context: no vocabulary, no batch
        tp, tb = "ss_bow_transform_device", "ss_bow_transform_batch_device"
        gb, pb, bb, eb, rb = ("ss_match_guided_batch_device", "ss_match_proj_batch_device", "ss_match_bow_batch_device", "ss_match_epi_batch_device",
                              "ss_triangulate_batch_device")
        _refused(ctx, a, [(tp, dict(), STATE, tp + ": no vocabulary (ss_bow_set_vocabulary)"), (tp, dict(n_frames=-1), STATE, tp + ": no vocabulary (ss_bow_set_vocabulary)"),
                          (tb, dict(), STATE, tb + ": no vocabulary (ss_bow_set_vocabulary)")])
        for fn in (gb, pb, bb, eb, rb):
            _refused(ctx, a, [(fn, dict(), STATE, fn + no_batch), (fn, dict(p=None), STATE, fn + no_batch), (fn, dict(d_idx=None), STATE, fn + no_batch)])
        # ---- with a vocabulary
        with binding.Vocabulary.load_text(VOC_PATH) as voc:
            ctx.set_vocabulary(voc)
        too_many = f"bow transform: rows_per_frame {MAX + 1} exceeds SS_BOW_MAX_ROWS ({MAX})"
        _refused(ctx, a, [(tp, dict(n_frames=-1), INVALID, "bow transform: bad frame count, row count or levelsup"),
                          (tp, dict(rows=0), INVALID, "bow transform: bad frame count, row count or levelsup"),
                          (tp, dict(levelsup=-1), INVALID, "bow transform: bad frame count, row count or levelsup"),
                          (tp, dict(rows=MAX + 1), INVALID, too_many), (tp, dict(d_node=None), INVALID, "bow transform: NULL buffer"),
                          (tp, dict(n_frames=0, all_buffers_null=True), OK, ""), (tp, dict(rows=MAX + 1, d_desc=None), INVALID, too_many),
                          (tb, dict(), STATE, tb + no_batch), (tb, dict(levelsup=-1), STATE, tb + no_batch)])
        # ---- with a batch that has not been transformed
        kcap = _extract(ctx)
        a = Arrays(binding, kcap)
        _refused(ctx, a, [(tb, dict(levelsup=-1), INVALID, "bow transform: levelsup must be >= 0"),
                          (tb, dict(d_bow_value=None), INVALID, "bow transform: NULL output buffer"),
                          (tb, dict(levelsup=-1, d_word=None), INVALID, "bow transform: levelsup must be >= 0")])
        for fn in (bb, eb):
            _refused(ctx, a, [(fn, dict(), STATE, fn + no_transform), (fn, dict(p=None), STATE, fn + no_transform),
                              (fn, dict(train_src=[7, 7]), STATE, fn + no_transform)])
        _refused(ctx, a, _batch_table(gb, "guided match", "guided match"))
        _refused(ctx, a, [(gb, b, INVALID, m) for b, m in GUIDED_RULES])
        _refused(ctx, a, [(gb, dict(d_d2=None), INVALID, "guided match: NULL output buffer"),
                          (gb, dict(d_summary=None, train_src=[0, F]), INVALID, "guided match: NULL output buffer")])
        _refused(ctx, a, _batch_table(rb, "triangulation", "triangulation"))
        _refused(ctx, a, [(rb, dict(d_idx=None), INVALID, "triangulation: NULL buffer"), (rb, dict(pairs=None), INVALID, "triangulation: NULL buffer"),
                          (rb, dict(d_n_points=None, train_src=[0, F]), INVALID, "triangulation: NULL buffer")])
        _refused(ctx, a, _proj_shared(pb, kcap))
        # ---- with the batch transformed
        assert call(ctx, a, tb) == (OK, "")
        _refused(ctx, a, _batch_table(bb, "guided match", "bow match"))
        _refused(ctx, a, [(bb, b, INVALID, m) for b, m in GUIDED_RULES])
        _refused(ctx, a, [(bb, dict(d_d1=None), INVALID, "bow match: NULL output buffer"),
                          (bb, dict(d_idx=None, train_src=[-2, 0]), INVALID, "bow match: NULL output buffer")])
        _refused(ctx, a, _batch_table(eb, "epipolar search", "epipolar search"))
        _refused(ctx, a, [(eb, b, INVALID, m) for b, m in EPI_RULES])
        _refused(ctx, a, [(eb, dict(pairs=None), INVALID, "epipolar search: NULL buffer"),
                          (eb, dict(d_summary=None, train_src=[F, 0]), INVALID, "epipolar search: NULL buffer")])
        ctx.synchronize()


# ---- the stages of a call: (name, launches, algorithmic bytes), from the formulas next to each stage_timer --------------------------
def _sizes(binding):
    return dict(kp=binding.KP_DTYPE.itemsize, window=binding.GUIDED_WINDOW_DTYPE.itemsize, point=binding.MAP_POINT_DTYPE.itemsize,
                proj=binding.PROJ_POINT_DTYPE.itemsize, info=binding.TRI_INFO_DTYPE.itemsize, guided=C.sizeof(binding.GuidedSummary),
                proj_sum=C.sizeof(binding.ProjSummary), bow=C.sizeof(binding.BowSummary), epi=C.sizeof(binding.EpiSummary),
                tri=C.sizeof(binding.TriSummary))


def _cells(extent_w, extent_h):
    s = G.grid_shift(extent_w, extent_h)
    return (((extent_w - 1) >> s) + 1) * (((extent_h - 1) >> s) + 1)


def _index_bytes(z, frames, rows, extent):
    """keypoints in, records (16 bytes) and cell offsets out"""
    return frames * rows * (z["kp"] + 16) + frames * (_cells(*extent) + 1) * 4


def guided_stages(z, frames, rows, extent, windows, orientation):
    nq = frames * rows
    return {("guided_index", 1, _index_bytes(z, frames, rows, extent)),
            ("guided_search", 1, nq * ((z["window"] if windows else z["kp"]) + DESC + 12)),
            ("guided_finish", 1, nq * (8 + 2 + 4 + (8 if orientation else 0)) + frames * z["guided"])}


def proj_stages(z, frames, point_rows, rows, extent):
    n = frames * point_rows
    return {("proj_index", 1, _index_bytes(z, frames, rows, extent)), ("proj_search", 1, n * (z["point"] + DESC + 12 + z["proj"])),
            ("proj_finish", 1, n * (8 + 2 + 4 + 4) + frames * z["proj_sum"])}


def transform_stages(z, frames, rows, index):
    nr = frames * rows
    return {("bow_descend", 1, nr * (DESC + 8)), ("bow_vector", 1, nr * (12 + 12 + (8 if index else 0)) + frames * z["bow"])}


def bow_stages(z, frames, rows, own_nodes, orientation):
    nr = frames * rows
    return ({("bow_index", 1, nr * 12)} if own_nodes else set()) | {
        ("bow_search", 1, nr * (4 + DESC + 12)), ("bow_finish", 1, nr * (8 + 2 + 4 + (8 if orientation else 0)) + frames * z["guided"])}


def epi_stages(z, frames, rows, own_nodes, orientation):
    nr = frames * rows
    return ({("epi_index", 1, nr * 12)} if own_nodes else set()) | {
        ("epi_search", 1, nr * (4 + z["kp"] + DESC + 18)),
        ("epi_finish", 1, nr * (8 + 2 + 4 + 8 + (8 if orientation else 0)) + frames * (z["guided"] + z["epi"]))}


def tri_stages(z, frames, rows):
    nr = frames * rows
    return {("tri_eval", 1, nr * (4 + z["kp"] + z["info"])), ("tri_compact", 1, nr * 4 + frames * (z["tri"] + 4))}


def _recorded(binding, forms, batch=False, vocabulary=False):
    """the stages `forms` record on a fresh context that profiles from its first search call on"""
    with binding.OrbContext(0, n_features=G.NF, max_batch=F) as ctx:
        if vocabulary:
            with binding.Vocabulary.load_text(VOC_PATH) as voc:
                ctx.set_vocabulary(voc)
        a = Arrays(binding, _extract(ctx) if batch else ROWS)
        ctx.profile(True)
        for fn, broken in forms:
            assert call(ctx, a, fn, **broken) == (OK, ""), fn
        ctx.synchronize()
        return {(s["name"], s["launches"], s["algorithmic_bytes"]) for s in ctx.stats()}, a.rows


def test_stage_table():
    from send_slam_amd import binding
    z = _sizes(binding)
    assert (z["kp"], z["window"], z["point"], z["proj"], z["info"]) == (24, 16, 32, 32, 16)  # the layouts the formulas were written for
    ext = (G.W, G.H)
    got, _ = _recorded(binding, [("ss_match_guided_pairs_device", {})])
    assert got == guided_stages(z, F, ROWS, ext, True, 1)
    got, _ = _recorded(binding, [("ss_match_guided_pairs_device", dict(p__orientation=0, p__extent_w=5000, p__extent_h=3000))])
    assert got == guided_stages(z, F, ROWS, (5000, 3000), True, 0)
    got, kcap = _recorded(binding, [("ss_match_guided_batch_device", {})], batch=True)
    assert got == guided_stages(z, F, kcap, ext, False, 1)
    got, _ = _recorded(binding, [("ss_match_guided", {})])
    assert got == guided_stages(z, 1, ROWS, ext, True, 1)
    got, _ = _recorded(binding, [("ss_match_proj_pairs_device", {})])
    assert got == proj_stages(z, F, ROWS, ROWS, ext)
    got, kcap = _recorded(binding, [("ss_match_proj_batch_device", {})], batch=True)
    assert got == proj_stages(z, F, ROWS, kcap, ext)
    got, _ = _recorded(binding, [("ss_match_proj", dict(n_points=40))])
    assert got == proj_stages(z, 1, 40, ROWS, ext)
    got, _ = _recorded(binding, [("ss_bow_transform_device", {}), ("ss_match_bow_pairs_device", {})], vocabulary=True)
    assert got == transform_stages(z, F, ROWS, False) | bow_stages(z, F, ROWS, True, 1)
    got, kcap = _recorded(binding, [("ss_bow_transform_batch_device", {}), ("ss_match_bow_batch_device", dict(p__orientation=0))], batch=True, vocabulary=True)
    assert got == transform_stages(z, F, kcap, True) | bow_stages(z, F, kcap, False, 0)
    got, _ = _recorded(binding, [("ss_match_epi_pairs_device", {})])
    assert got == epi_stages(z, F, ROWS, True, 1)
    got, kcap = _recorded(binding, [("ss_bow_transform_batch_device", {}), ("ss_match_epi_batch_device", dict(p__orientation=0))], batch=True, vocabulary=True)
    assert got == transform_stages(z, F, kcap, True) | epi_stages(z, F, kcap, False, 0)
    got, _ = _recorded(binding, [("ss_triangulate_pairs_device", {})])
    assert got == tri_stages(z, F, ROWS)
    got, kcap = _recorded(binding, [("ss_triangulate_batch_device", {})], batch=True)
    assert got == tri_stages(z, F, kcap)
    # twice on one context: the launches add up, the bytes are those of the last call
    got, _ = _recorded(binding, [("ss_match_epi_pairs_device", {}), ("ss_match_epi_pairs_device", dict(p__orientation=0))])
    assert got == {(n, 2, b) for n, _, b in epi_stages(z, F, ROWS, True, 0)}
