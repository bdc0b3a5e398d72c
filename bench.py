#!/usr/bin/env python3
"""bench.py -- frames/s of ORB extract + self-match on synthetic 1280x720 frames, 2000 kp/frame
(BASELINE.json metric, config "1xMI355X: synthetic 1280x720 frames, ORB extract + self-match").

A "step" is one pass of the hot path over ONE BATCH of frames already resident in HBM:
ss_extract_batch_device (pyramid, FAST + NMS, quadtree, orientation, blur, rBRIEF) followed by
ss_match_batch_device (self-match, j == i excluded).  Steps rotate over several DISTINCT device batches
whose total exceeds the 256 MB Infinity Cache, so the frames of a step come from HBM, and over a few
contexts (camera batches in flight, each with its own stream and buffers).  With N GPUs every rank
runs the same steps on its own camera batches (cameras shard one per GPU, no data-path collective):
weak scaling, value = frames all ranks processed / max-over-ranks time.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--batch B]        N > 1 without a launcher: bench.py starts its N ranks itself
    python bench.py ... --dump-outputs DIR                                 also write the last timed step's outputs as DIR/*.npy
    python bench.py ... --full                                             everything listed below as well
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...
    python bench.py --gpus 2 --workload stereo [--exchange native|rccl]    config 4
    python bench.py --gpus N --workload loop_closure [--exchange ...]      config 5

Timing of the metric workload: a plain run times ONE region of EXACTLY K steps, bracketed by barrier +
torch.cuda.synchronize() on both sides and max-reduced over the ranks; value = frames all ranks processed / its time,
ms_per_step = its time / K.  Nothing else runs: set-up, warm-up (W steps, and more until it has lasted 0.5 s), the K
steps, the outputs (--dump-outputs) and the line.
With --full: R rounds of EXACTLY K steps, each bracketed the same way, added until they together time >= 0.5 s whatever K
is (at least 3 rounds); value = units all ranks processed in a round / the MEDIAN round's time; value_spread = min /
median / max over the rounds.  The stereo and loop-closure workloads always time their steps in such rounds.

--dump-outputs DIR (metric workload, rank 0): what the last timed step returned to its caller, the frames of its batch
concatenated in order, as float32 .npy: n_keypoints [F], level_counts [F, 8], keypoints [n, 6] (x, y, size, angle,
response, octave), descriptors [n, 32] (byte values), match_idx / match_d1 / match_d2 [n], frames [F] (the batch indices
of the F frames written: the whole batch, or a fixed sample of it where the whole would exceed 64 MB).  The frames are
seeded and every round of timed steps runs the same steps, so the same arguments give the same inputs on every run.

Rank 0 prints ONE JSON line.  With --full, besides the contract fields it carries
  sustained              (K < 500) one region of 1000 steps, the rate of a pipeline that stays full, with the rate of each 1/25th
  ranks_reported_by_backend  N > 1 (and forced world-1 groups): world size and an all-reduce of ones through the backend
  single_gpu_exchange    N = 1: configs 4 and 5 as child processes at world size 1 -- through a real "nccl" (RCCL) process
                         group (SENDSLAM_BENCH_FORCE_DIST=1) and through the C ABI's own exchange (ss_xchg_*)
  roofline               dominant kernel: ALGORITHMIC bytes per launch / HIP-event mean duration on its own stream
  valu_roofline          the same kernel against the resource that binds it (integer VALU issue)
  match_roofline         the Hamming-match kernel of the metric (2000 x 2000 per frame) against the FP4 MFMA peak
  match_stream_roofline  the Hamming-match kernel in the database-streaming regime (1 and 4 queries against 20 M
                         descriptors = 640 MB): achieved HBM GB/s against the 8 TB/s peak -- the north star's
                         ">= 60 % HBM roofline on the Hamming-match kernel"
  consecutive_frames     the same step with every frame matched against the frame before it in its batch (SURVEY.md 8(d):
                         "frame t vs t + 1"); two pairs checked against the oracle
  host_pipeline          the same step fed from HOST memory through the pinned ring of the C ABI (ss_pipe_*):
                         frames/s and PCIe GB/s, copies overlapped with the kernels.  Never `value`.
  frontdoor              the literal drop-in: this process plays SlamHandler over TCP + MessagePack + PNM against the front
                         door binary (read-ahead 16, pacing off): frames/s, and where the front door's time goes
  kernels                per-stage durations
  cpu_baseline           the CPU oracle (a port: the reference's ORB-SLAM3 cannot be built here) timed on
                         this host on a bounded sample of the same frames, 1 thread like the reference shim
                         (orbslam3_mono_networked.cc:594), plus all cores
Parity: "parity_checked_vs_oracle" compares frames of EVERY context's last timed batch with the oracle = the
committed CPU restatement (parity with the real ORB-SLAM3 binary is unpinned).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for p in (ROOT, os.path.join(ROOT, "send-slam_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

FP4_MFMA_PEAK_OPS = 10.0e15  # dense FP4 MFMA (MI355X_MICROARCH.md "Peak FP6/FP4 MFMA ~10 PF dense"; measured issue rate: profiles/r02_fp4_probe.txt)
INT8_MFMA_PEAK_OPS = 5.0e15  # dense int8 MFMA: the packed-descriptor kernel k_match_mfma (SENDSLAM_LC_PACKED=1)
HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8 TB/s spec (6.3 TB/s achievable)
CACHE_BYTES = 256 << 20  # Infinity Cache: the rotating device batches must exceed it


def make_frames(rank, n_sets, batch, w, h):
    """n_sets x batch DISTINCT frames: set s = scene (rank, s) at time steps 0 .. batch-1 (consecutive frames move
    by (3,-2) px and carry fresh noise).  Every frame has its own seeded generator, so host threads make the same bytes
    as one thread would; the pool is gone before anything forks."""
    from concurrent.futures import ThreadPoolExecutor
    from send_slam_amd import synth
    out = np.empty((n_sets, batch, h, w), np.uint8)
    scenes = [None] * n_sets

    def one_scene(s):
        scenes[s] = synth.scene(1000 * rank + s, w, h)

    def one_frame(st):
        s, t = st
        out[s, t] = synth.frame_from_scene(scenes[s], 1000 * rank + s, w, h, t)
    with ThreadPoolExecutor(max(1, min(16, usable_cores()))) as pool:
        list(pool.map(one_scene, range(n_sets)))
        list(pool.map(one_frame, [(s, t) for s in range(n_sets) for t in range(batch)]))
    return out


_CPU_FRAMES = None


def _cpu_one(args):
    from oracle import orb_oracle as O
    i, nf = args
    frame = _CPU_FRAMES[i]
    p = O.default_params(n_features=nf)
    t0 = time.perf_counter()
    kps, desc, _ = O.extract(frame, p)
    idx, d1, d2 = O.match(desc, desc, 50, 9, 10, exclude_self=True)
    return time.perf_counter() - t0, kps, desc, idx, d1, d2


def _cpu_time_only(args):
    return _cpu_one(args)[0]


def _noop(_):
    return 0


def usable_cores():
    """cores this process may actually use: the affinity mask, cut to the cgroup's CPU quota when there is one (a GPU box
    shows all of the host's cores but grants a share of them)"""
    cores = len(os.sched_getaffinity(0))
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if quota != "max":
            cores = min(cores, max(1, int(float(quota) / float(period) + 0.5)))
    except (OSError, ValueError):
        try:
            q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0:
                cores = min(cores, max(1, int(q / per + 0.5)))
        except (OSError, ValueError):
            pass
    return cores


def cpu_baseline(frames, nf, budget_s=12.0):
    """Oracle timed on host cores BEFORE the GPU is touched (a process pool forks).
    Returns the JSON object and the per-frame oracle outputs for the parity check."""
    import multiprocessing as mp
    from oracle import orb_oracle as O
    global _CPU_FRAMES
    _CPU_FRAMES = frames
    O.build()
    times, outs = [], []
    _cpu_one((0, nf))  # warm-up (page in, first malloc)
    t_start = time.perf_counter()
    for i in range(len(frames)):
        r = _cpu_one((i, nf))
        times.append(r[0])
        outs.append(r[1:])
        if time.perf_counter() - t_start > budget_s / 2 and len(times) >= 5:
            break
    times.sort()
    median = times[len(times) // 2]  # the shim's median rule (orbslam3_mono_networked.cc:661)
    cores = usable_cores()
    all_cores = n_jobs = None
    if cores > 1:
        # >= 4 jobs per core, frames reused round-robin (the workers inherit them by fork: nothing is pickled in),
        # pool started and warmed before the clock starts
        n_jobs = max(4 * cores, int(cores * (budget_s / 2) / max(median, 1e-3)))
        n_jobs = min(n_jobs, 16 * cores)
        jobs = [(i % len(frames), nf) for i in range(n_jobs)]
        with mp.get_context("fork").Pool(cores) as pool:
            pool.map(_noop, range(4 * cores), chunksize=1)
            t0 = time.perf_counter()
            pool.map(_cpu_time_only, jobs, chunksize=1)
            all_cores = n_jobs / (time.perf_counter() - t0)
    obj = {"value": round(1.0 / median, 3), "unit": "frames/s", "cores": 1, "kind": "port",
           "sample": f"{len(times)} of the bench's own 1280x720 frames, extract + self-match, median per frame "
                     f"{median * 1e3:.1f} ms, 1 thread (oracle/orb_oracle.c, -O3)",
           "all_cores_value": None if all_cores is None else round(all_cores, 2), "all_cores": cores,
           "all_cores_sample": None if n_jobs is None else f"{n_jobs} frame jobs over a warmed pool of {cores} processes (affinity mask {len(os.sched_getaffinity(0))}, cgroup quota applied), one frame per job"}
    return obj, outs


def dist_setup(world):
    import torch
    import torch.distributed as dist
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    # rehearsal hooks for a ONE-GPU box (tests / gpurun): SENDSLAM_BENCH_BACKEND=gloo moves the collectives to the
    # CPU, SENDSLAM_BENCH_ONE_DEVICE=1 puts every rank on device 0.
    backend = os.environ.get("SENDSLAM_BENCH_BACKEND", "nccl")
    if os.environ.get("SENDSLAM_BENCH_ONE_DEVICE") == "1":
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29533")
    if use_dist(world):
        import datetime
        tmo = datetime.timedelta(seconds=int(os.environ.get("SENDSLAM_BENCH_DIST_TIMEOUT", "180")))
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev, timeout=tmo)  # RCCL over xGMI
        else:
            dist.init_process_group(backend, rank=rank, world_size=world, timeout=tmo)
    return rank, local_rank, dev, backend


def use_dist(world):
    """a process group exists for every multi-rank run, and at world size 1 under SENDSLAM_BENCH_FORCE_DIST=1: the
    collectives of the stereo / loop-closure steps then run through RCCL ("nccl") on ONE GPU, so that branch has
    executed before an 8-GPU node sees it"""
    return world > 1 or os.environ.get("SENDSLAM_BENCH_FORCE_DIST") == "1"


def backend_world(world, dev, backend):
    """the rank count the backend itself reports: an all-reduce of ones (through RCCL on the GPUs)"""
    import torch
    import torch.distributed as dist
    if not use_dist(world):
        return None
    t = torch.ones(1, dtype=torch.int32, device=dev if backend == "nccl" else "cpu")
    dist.all_reduce(t)
    return {"backend": backend, "world_size": dist.get_world_size(), "allreduce_of_ones": int(t.item())}


def max_over_ranks(elapsed, world, dev, backend):
    import torch
    import torch.distributed as dist
    if not use_dist(world):
        return elapsed
    t = torch.tensor([elapsed], dtype=torch.float64, device=dev if backend == "nccl" else "cpu")
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


MIN_REGION_S = 0.5  # whatever --steps is, the rounds together time at least this long
MIN_WARMUP_S = 0.5  # a plain run's warm-up lasts at least this long: its ONE region then starts on a GPU at speed


def timed_rounds(run_steps, steps, drain, world, dev, backend, max_rounds=400, rounds=0):
    """R rounds of EXACTLY `steps` steps.  Every round is bracketed by barrier + torch.cuda.synchronize() on both sides and
    its time is the MAX over ranks; rounds are added until they together last >= MIN_REGION_S, at least 3, or exactly
    `rounds` of them when it is given.  Returns the list of round times in seconds."""
    import torch
    import torch.distributed as dist
    d = use_dist(world)

    def one():
        if d:
            dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run_steps(steps)
        drain()
        torch.cuda.synchronize()
        if d:
            dist.barrier()
        return max_over_ranks(time.perf_counter() - t0, world, dev, backend)
    # every time in `times` is max-reduced, so every rank sees the same numbers and stops after the same round
    fixed = rounds or int(os.environ.get("SENDSLAM_BENCH_ROUNDS", "0"))
    times = []
    while len(times) < max_rounds:
        times.append(one())
        if fixed:
            if len(times) >= fixed:
                break
        elif len(times) >= 3 and sum(times) >= MIN_REGION_S:
            break
    return times


def round_summary(times, units_per_round, unit):
    """value = the median round's rate; spread over the rounds"""
    srt = sorted(times)
    med = srt[len(srt) // 2]
    return med, {"rounds": len(times), "median": round(units_per_round / med, 2), "min": round(units_per_round / srt[-1], 2),
                 "max": round(units_per_round / srt[0], 2), "unit": unit,
                 "round_ms": {"median": round(med * 1e3, 4), "min": round(srt[0] * 1e3, 4), "max": round(srt[-1] * 1e3, 4)}}


def stage_roofline(stats, name, peak=HBM_PEAK_GBS):
    s = next((x for x in stats if x["name"] == name), None)
    if not s or not s["launches"] or s["mean_ms"] <= 0:
        return None
    gbs = s["algorithmic_bytes"] / (s["mean_ms"] * 1e-3) / 1e9
    return {"kernel": name, "bound": "hbm", "achieved": round(gbs, 1), "peak": peak, "unit": "GB/s", "frac": round(gbs / peak, 4),
            "kernel_ms": round(s["mean_ms"], 5), "launches": s["launches"], "algorithmic_bytes_per_launch": s["algorithmic_bytes"]}


def bench_loop_closure(a):
    """Config 5 of BASELINE.json: query-vs-all Hamming match against a keyframe database partitioned in contiguous slabs
    over the ranks; per query one broadcast, ss_match_partial_device, one all_gather of world x nq x 8 B and
    ss_match_fold_device, all ordered on the context's stream (multi.loop_closure_query_device)."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank, local_rank, dev, backend = dist_setup(world)
    import torch
    import torch.distributed as dist
    from send_slam_amd import binding, multi
    n_db, nq = 10000 * 2000, a.features
    b, e = multi.slab(n_db, world, rank)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1234 + rank)
    db = torch.randint(0, 256, (e - b, 32), dtype=torch.uint8, device=dev, generator=gen)
    query = torch.randint(0, 256, (nq, 32), dtype=torch.uint8, device=dev, generator=gen)
    ctx = binding.OrbContext(local_rank)
    out = (torch.empty(nq, dtype=torch.int32, device=dev), torch.empty(nq, dtype=torch.int16, device=dev),
           torch.empty(nq, dtype=torch.int16, device=dev))
    steps = a.steps if a.steps else 20
    # the keyframe database is static: its slab is expanded once to the matrix-core matcher's operand format (128 B per
    # descriptor: 2.6 GB for the whole database, 320 MB per GPU at 8); SENDSLAM_LC_PACKED=1 keeps the packed rows and
    # the expanding kernel (k_match_mfma<2>) instead
    dbx = None if os.environ.get("SENDSLAM_LC_PACKED") == "1" else multi.expand_database(ctx, db)
    kw = {} if dbx is None else {"db_expanded": dbx, "n_db": e - b}
    xchg = make_exchange(a, binding, rank, world, local_rank, nq * 32)
    if xchg is not None:
        kw["xchg"] = xchg
    _q = multi.loop_closure_query_device
    multi_query = lambda: _q(ctx, query, db, b, out=out, **kw)  # noqa: E731
    for _ in range(max(a.warmup, 1)):
        multi_query()
    ctx.synchronize()
    ctx.profile(True)
    ctx.profile_reset()

    def run_steps(k):
        for _ in range(k):
            multi_query()
    times = timed_rounds(run_steps, steps, ctx.synchronize, world, dev, backend)
    elapsed, spread = round_summary(times, steps, "queries/s")
    stats = ctx.stats()
    ctx.profile(False)
    reported = backend_world(world, dev, backend)
    if rank == 0:
        mk = next((s for s in stats if s["name"] == "match"), None)
        pairs = float(nq) * (e - b)
        roof = None
        if mk and mk["mean_ms"] > 0:
            t = mk["mean_ms"] * 1e-3
            peak = INT8_MFMA_PEAK_OPS if dbx is None else FP4_MFMA_PEAK_OPS
            roof = {"kernel": ("match (k_match_mfma<2>" if dbx is None else "match (k_match_mfma_x on the expanded slab") + " + merge, this rank's slab)", "bound": "mfma", "achieved": float(f"{pairs * 512 / t / 1e12:.4g}"),
                    "peak": peak / 1e12, "unit": "Top/s (int8 MFMA)" if dbx is None else "Top/s (FP4 MFMA, +-1 operands, exact)", "frac": round(pairs * 512 / t / peak, 4),
                    "kernel_ms": round(mk["mean_ms"], 4), "traffic": None}
        print(json.dumps({
            "metric": "loop-closure queries/sec (2000 descriptors vs 10k-keyframe database)", "value": round(steps / elapsed, 3),
            "unit": "queries/s", "n_gpus": world, "steps": steps, "rounds": len(times), "warmup": a.warmup,
            "ms_per_step": round(elapsed / steps * 1e3, 3), "higher_is_better": True, "scaling": "strong",
            "vs_baseline": None, "dtype": "u8", "data": "synthetic",
            "config": {"workload": f"loop closure: {nq}-descriptor query vs {n_db} descriptors (640 MB) sharded over {world} GPU(s), "
                                   "raw local match -> 8-byte records, all_gather, fold kernel", "parallelism": f"db slabs x {world}",
                       "database_format": "packed 32 B rows" if dbx is None else "expanded once to 128 B rows of FP4 +-1 (matrix-core operand)",
                       "exchange": exchange_name(a, world), "backend": backend if use_dist(world) else None},
            "timed_region_s": round(sum(times), 4), "value_spread": spread, "ranks_reported_by_backend": reported,
            "roofline": roof, "kernels": [{"name": s["name"], "mean_ms": round(s["mean_ms"], 5), "launches": s["launches"]} for s in stats],
            "pairs_per_s": float(f"{nq * n_db * steps / elapsed:.4g}")}))
    if xchg is not None:
        xchg.close()
    ctx.close()
    if use_dist(world):
        dist.destroy_process_group()


def exchange_name(a, world):
    if not use_dist(world) and a.exchange != "native":
        return None
    return "native (ss_xchg: peer-mapped slabs, direct writes + flags)" if a.exchange == "native" else "torch.distributed collectives"


def make_exchange(a, binding, rank, world, local_rank, max_bytes):
    """--exchange native: the C ABI's own all-gather (ss_xchg_*: every rank writes its block straight into every peer's
    IPC-mapped slab over xGMI and raises a flag; no PyTorch, no RCCL in the data path).  The rendezvous (a Unix socket
    path) comes from the master port, so every rank derives the same one."""
    if a.exchange != "native":
        return None
    path = os.environ.get("SENDSLAM_XCHG_PATH") or f"/tmp/sendslam_xchg_{os.environ.get('MASTER_PORT', '29533')}_{a.workload}"
    return binding.Exchange(local_rank, rank, world, max_bytes, path, timeout_ms=180000)  # ranks reach this point seconds apart


def bench_stereo(a):
    """Config 4 of BASELINE.json: left / right 1920x1080 cameras on two GPUs.  A step = each rank extracts a batch of
    frames of ITS eye, one all_gather of the fixed-size descriptor blocks ([B][kp_capacity][32] + counts) over xGMI,
    then each rank matches its frames against the peer eye's frames of the same instant (ss_match_pairs_device).
    Everything is ordered on the context's stream; value = stereo pairs per second.  World size 1 is accepted under
    SENDSLAM_BENCH_FORCE_DIST=1 only (one-GPU execution of the same collectives: the "peer" eye is the rank's own)."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != 2 and not (world == 1 and (use_dist(world) or a.exchange == "native")):
        sys.exit("bench.py --workload stereo needs exactly 2 ranks (bench.py --gpus 2 --workload stereo, or torch.distributed.run "
                 "--nproc-per-node 2); world size 1 only with SENDSLAM_BENCH_FORCE_DIST=1")
    rank, local_rank, dev, backend = dist_setup(world)
    import torch
    import torch.distributed as dist
    from send_slam_amd import binding, multi, synth
    w, h, nf, B = 1920, 1080, a.features, (a.batch or 16)
    # the right eye sees the left eye's scene 24 px further left (a fronto-parallel plane)
    sc = synth.scene(4242, w + 64, h)
    frames = np.stack([np.clip(sc[synth._MARGIN + 2 * t:synth._MARGIN + 2 * t + h, synth._MARGIN + 24 * rank + 3 * t:synth._MARGIN + 24 * rank + 3 * t + w], 0, 255).astype(np.uint8)
                       for t in range(B)])
    d_frames = torch.from_numpy(np.ascontiguousarray(frames)).to(dev)
    ctx = binding.OrbContext(local_rank, n_features=nf, max_batch=B)
    ctx.extract_batch_device(d_frames.data_ptr(), B, w, h)
    ctx.synchronize()
    kcap = ctx.batch_view().kp_capacity
    view = ctx.batch_view()

    def dev_tensor(ptr, shape, dtype):
        """torch view of a device array the library owns (no copy)"""
        class _Wrap:
            __cuda_array_interface__ = {"shape": tuple(shape), "typestr": {torch.uint8: "|u1", torch.int32: "<i4"}[dtype],
                                        "data": (ptr, False), "version": 2}
        return torch.as_tensor(_Wrap(), device=dev)
    own_desc = dev_tensor(view.descriptors, (B, kcap, 32), torch.uint8)
    own_n = dev_tensor(view.n_keypoints, (B,), torch.int32)
    gathered_desc = torch.empty((world, B, kcap, 32), dtype=torch.uint8, device=dev)
    gathered_n = torch.empty((world, B), dtype=torch.int32, device=dev)
    o_idx = torch.empty((B, kcap), dtype=torch.int32, device=dev)
    o_d1 = torch.empty((B, kcap), dtype=torch.int16, device=dev)
    o_d2 = torch.empty((B, kcap), dtype=torch.int16, device=dev)
    peer = (world - 1) - rank
    blk = B * kcap * 32
    # native exchange: ONE message per step = the descriptor blocks followed by the B counts
    xchg = make_exchange(a, binding, rank, world, local_rank, blk + 4 * B)

    def step():
        ctx.extract_batch_device(d_frames.data_ptr(), B, w, h)
        if xchg is not None:
            base, stride = xchg.allgather(ctx, [(view.descriptors, blk), (view.n_keypoints, 4 * B)])
            ctx.match_pairs_device(view.descriptors, view.n_keypoints, base + peer * stride, base + peer * stride + blk,
                                   B, kcap, o_idx.data_ptr(), o_d1.data_ptr(), o_d2.data_ptr())
            return
        with multi.on_ctx_stream(ctx, dev):
            if backend == "nccl":
                dist.all_gather_into_tensor(gathered_desc, own_desc)
                dist.all_gather_into_tensor(gathered_n, own_n)
            else:  # CPU rehearsal of the exchange
                ctx.synchronize()
                outs = [torch.empty((B, kcap, 32), dtype=torch.uint8) for _ in range(world)]
                dist.all_gather(outs, own_desc.cpu())
                gathered_desc.copy_(torch.stack(outs))
                outs = [torch.empty((B,), dtype=torch.int32) for _ in range(world)]
                dist.all_gather(outs, own_n.cpu())
                gathered_n.copy_(torch.stack(outs))
            ctx.match_pairs_device(own_desc.data_ptr(), own_n.data_ptr(), gathered_desc[peer].data_ptr(), gathered_n[peer].data_ptr(),
                                   B, kcap, o_idx.data_ptr(), o_d1.data_ptr(), o_d2.data_ptr())

    steps = a.steps if a.steps else 20
    for _ in range(max(a.warmup, 1)):
        step()
    ctx.synchronize()
    ctx.profile(True)
    ctx.profile_reset()

    def run_steps(k):
        for _ in range(k):
            step()
    times = timed_rounds(run_steps, steps, ctx.synchronize, world, dev, backend)
    elapsed, spread = round_summary(times, B * steps, "pairs/s")
    stats = ctx.stats()
    ctx.profile(False)
    reported = backend_world(world, dev, backend)
    # sanity on the measured configuration: most left keypoints find their right-eye partner 24 px away
    n_own = own_n.cpu().numpy()
    idx = o_idx.cpu().numpy()
    matched = float(np.mean([(idx[b, :n_own[b]] >= 0).mean() for b in range(B)]))
    if rank == 0:
        print(json.dumps({
            "metric": "stereo pairs/sec ORB extract + cross-camera match @1920x1080, 2000 kp/eye", "value": round(B * steps / elapsed, 2),
            "unit": "pairs/s", "n_gpus": world, "steps": steps, "rounds": len(times), "warmup": a.warmup, "ms_per_step": round(elapsed / steps * 1e3, 4),
            "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "u8", "data": "synthetic",
            "config": {"workload": f"stereo {w}x{h}: one eye per GPU, batches of {B} frames, all_gather of {B * kcap * 32} B descriptor blocks + counts, "
                                   "cross-eye match" + (" (world size 1: the peer eye is the rank's own)" if world == 1 else ""),
                       "parallelism": f"{world} rank(s), one all_gather per step", "backend": backend if use_dist(world) else None,
                       "exchange": exchange_name(a, world)},
            "timed_region_s": round(sum(times), 4), "value_spread": spread, "ranks_reported_by_backend": reported,
            "roofline": stage_roofline(stats, "fast_blur_nms"),
            "kernels": [{"name": s["name"], "mean_ms": round(s["mean_ms"], 5), "launches": s["launches"]} for s in stats],
            "fraction_of_keypoints_matched_across_eyes": round(matched, 3)}))
    if xchg is not None:
        xchg.close()
    ctx.close()
    if use_dist(world):
        dist.destroy_process_group()


def bench_match_stream(binding, torch, dev, local_rank, launches=24):
    """The Hamming-match kernel in the regime where HBM bounds it (SURVEY.md section 8(d), config 5 with a handful of
    queries): 1 and 4 query descriptors against 20 M database descriptors (640 MB, read exactly once per launch)."""
    n_db = 10000 * 2000
    gen = torch.Generator(device=dev)
    gen.manual_seed(99)
    db = torch.randint(0, 256, (n_db, 32), dtype=torch.uint8, device=dev, generator=gen)
    out = {}
    with binding.OrbContext(local_rank) as ctx:
        for nq in (1, 4):
            q = torch.randint(0, 256, (nq, 32), dtype=torch.uint8, device=dev, generator=gen)
            idx = torch.empty(nq, dtype=torch.int32, device=dev)
            d1 = torch.empty(nq, dtype=torch.int16, device=dev)
            d2 = torch.empty(nq, dtype=torch.int16, device=dev)
            torch.cuda.synchronize()
            for _ in range(3):
                ctx.match_device(q.data_ptr(), nq, db.data_ptr(), n_db, idx.data_ptr(), d1.data_ptr(), d2.data_ptr())
            ctx.synchronize()
            ctx.profile(True)
            ctx.profile_reset()
            t0 = time.perf_counter()
            for _ in range(launches):
                ctx.match_device(q.data_ptr(), nq, db.data_ptr(), n_db, idx.data_ptr(), d1.data_ptr(), d2.data_ptr())
            ctx.synchronize()
            wall = (time.perf_counter() - t0) / launches
            st = ctx.stats()
            ctx.profile(False)
            ks = next(s for s in st if s["name"] == "match_stream_kernel")
            mg = next(s for s in st if s["name"] == "match_stream_merge")
            gbs = ks["algorithmic_bytes"] / (ks["mean_ms"] * 1e-3) / 1e9
            both = ks["mean_ms"] + mg["mean_ms"]
            out[f"{nq}q"] = {"kernel_ms": round(ks["mean_ms"], 4), "achieved_GBps": round(gbs, 1), "frac": round(gbs / HBM_PEAK_GBS, 4),
                             "merge_launch_ms": round(mg["mean_ms"], 4), "with_merge_GBps": round(ks["algorithmic_bytes"] / (both * 1e-3) / 1e9, 1),
                             "host_wall_ms_per_query_batch": round(wall * 1e3, 4), "launches": ks["launches"]}
    del db
    best = max(out.values(), key=lambda v: v["achieved_GBps"])
    traffic = None
    tpath = os.path.join(ROOT, "profiles", "traffic.json")
    if os.path.exists(tpath):
        traffic = json.load(open(tpath)).get("k_match_stream@20M_rows")
    return {"kernel": "k_match_stream (lane = database row, queries in SGPRs)", "bound": "hbm", "achieved": best["achieved_GBps"],
            "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": best["frac"], "traffic": traffic,
            "algorithmic_bytes_per_launch": n_db * 32, "database": "20 000 000 descriptors x 32 B = 640 MB", "by_queries": out}


def bench_host_pipeline(binding, frames_sets, w, h, nf, B, local_rank, depth=4, batches=24):
    """Host frames in, host keypoints / descriptors / matches out through ss_pipe_*: pinned ring of `depth` slots,
    H2D copy, kernels and D2H copy of different batches overlapped.  Two producers: (a) ss_pipe_submit_frames gathers
    the caller's pageable frames into the pinned slot with host threads; (b) the producer writes pinned slots itself
    (acquire / submit: the slots already hold frames; models a decoder or socket that fills pinned memory)."""
    n_sets = frames_sets.shape[0]
    res = {}
    cores = len(os.sched_getaffinity(0))
    with binding.Pipe(local_rank, w, h, batch=B, depth=depth, match_mode=0, copy_threads=int(os.environ.get("SENDSLAM_BENCH_COPY_THREADS", min(8, max(2, cores // 2)))), n_features=nf) as pipe:
        kcap = None

        def drain_one():
            nonlocal kcap
            r = pipe.wait()
            kcap = r["kp_capacity"]
            ok = int((r["status"] == 0).sum())
            nk = int(r["n_keypoints"].sum())
            pipe.release(r["slot"])
            return ok, nk
        for mode in ("submit_frames", "pinned_producer"):
            if mode == "pinned_producer":  # leave real frames in every slot
                slots = []
                for s in range(depth):
                    sl = pipe.acquire()
                    sl[1][:B, :, :w] = frames_sets[s % n_sets]
                    slots.append(sl[0])
                for s in slots:
                    pipe.release(s)
            # warm-up
            for i in range(depth):
                if mode == "submit_frames":
                    assert pipe.submit_batch_array(frames_sets[i % n_sets])
                else:
                    pipe.submit(pipe.acquire()[0], B)
            for _ in range(depth):
                drain_one()
            done = frames_ok = kps = 0
            t0 = time.perf_counter()
            for i in range(batches):
                if pipe.in_flight() == depth:
                    ok, nk = drain_one()
                    frames_ok += ok
                    kps += nk
                    done += 1
                if mode == "submit_frames":
                    assert pipe.submit_batch_array(frames_sets[i % n_sets])
                else:
                    pipe.submit(pipe.acquire()[0], B)
            while pipe.in_flight():
                ok, nk = drain_one()
                frames_ok += ok
                kps += nk
                done += 1
            el = time.perf_counter() - t0
            assert done == batches and frames_ok == batches * B
            h2d = batches * B * w * h
            d2h = batches * B * (kcap * (24 + 32 + 8) + 4 * 18)
            res[mode] = {"frames_per_s": round(batches * B / el, 1), "pcie_h2d_GBps": round(h2d / el / 1e9, 2),
                         "pcie_d2h_GBps": round(d2h / el / 1e9, 2), "batches": batches, "mean_keypoints_per_frame": round(kps / (batches * B), 1)}
    return {"batch": B, "depth": depth, "match": "self-match on the device, results copied back",
            "frames_per_s": res["submit_frames"]["frames_per_s"], "pcie_GBps": round(res["submit_frames"]["pcie_h2d_GBps"] + res["submit_frames"]["pcie_d2h_GBps"], 2),
            "submit_frames": res["submit_frames"], "pinned_producer": res["pinned_producer"],
            "note": "submit_frames = pageable caller frames gathered into the pinned slot by host threads, then H2D; pinned_producer = frames already in the "
                    "pinned slot (PCIe + kernels only)"}


def bench_frontdoor(n_frames=192, readahead=16):
    """The LITERAL drop-in: this process plays SlamHandler (slam_handler.ex:140-156, 275-291: one TCP connection, u32 length +
    MessagePack map per frame with the PPM/PGM file as a bin), the front door binary connects like the container does
    (ORB_SLAM3_WS_PORT), receives, decodes the PNM into pinned slots, extracts on the GPU, tracks, answers.  Pacing off,
    read-ahead 16 (SENDSLAM_NO_PACING=1).  Frames are pre-encoded, so the sender costs one sendall; a "features" message per
    frame tells when each frame has been answered.  Config 1 of BASELINE.json (640x480 colour P6, 1250 features) and the metric's
    frame shape (1280x720 gray P5, 2000 features).  Never `value`."""
    import socket
    import subprocess
    import threading
    import msgpack
    from send_slam_amd import synth, wire
    fd_bin = os.path.join(ROOT, "send-slam_amd", "frontdoor", "sendslam_frontdoor")
    if not os.path.exists(fd_bin):
        return {"error": "front door binary not built"}
    out = {}
    for name, (w, h, ch, nfeat) in {"640x480_P6_1250": (640, 480, 3, 1250), "1280x720_P5_2000": (1280, 720, 1, 2000)}.items():
        n_distinct = 24
        sc = synth.scene(4000, w, h)
        base = [synth.parallax_frame(4000, w, h, t, sc=sc) for t in range(n_distinct)]
        if ch == 3:
            base = [np.repeat(f[:, :, None], 3, axis=2) for f in base]
        order = list(range(n_distinct)) + list(range(n_distinct - 2, 0, -1))  # back and forth: continuous motion
        dims = {"width": w, "height": h, "channels": ch}
        enc = [wire.encode_to_ppm(f) for f in base]
        pk = [wire.build_frame_packet(enc[order[i % len(order)]], dims, camera_id=1, timestamp=1.0 + i / 30.0) for i in range(n_frames)]
        blob = b"".join(pk)
        calib = wire.build_calibration_packet([[0.8 * w, 0, w / 2], [0, 0.8 * w, h / 2], [0, 0, 1]], [0, 0, 0, 0], dims)
        srv = socket.socket(socket.AF_INET, socket.SOCK_STREAM)
        srv.setsockopt(socket.SOL_SOCKET, socket.SO_REUSEADDR, 1)
        srv.bind(("127.0.0.1", 0))
        srv.listen(1)
        env = dict(os.environ, ORB_SLAM3_WS_PORT=str(srv.getsockname()[1]), SENDSLAM_NO_PACING="1", SENDSLAM_READAHEAD=str(readahead),
                   SENDSLAM_EMIT_FEATURES="1", SENDSLAM_TIMING="1", SENDSLAM_TRACK_TIMING="1", SENDSLAM_ORB_NFEATURES=str(nfeat),
                   LD_LIBRARY_PATH=os.path.join(ROOT, "send-slam_amd", "lib") + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
        proc = subprocess.Popen([fd_bin], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        try:
            srv.settimeout(60)
            conn, _ = srv.accept()
            conn.settimeout(120)
            conn.setsockopt(socket.SOL_SOCKET, socket.SO_SNDBUF, 8 << 20)
            stamps, states = [], []

            def reader():
                buf = b""
                while len(stamps) < n_frames:
                    chunk = conn.recv(1 << 16)
                    if not chunk:
                        return
                    pkts, buf = wire.extract_packets(buf + chunk)
                    for p_ in pkts:
                        m = msgpack.unpackb(p_, raw=False)
                        if m.get("type") == "features":
                            stamps.append(time.perf_counter())
                            states.append(m["tracking_state"])
            conn.sendall(calib)
            warm = pk[:readahead]  # first batch: pipe creation, kernel load
            th = threading.Thread(target=reader)
            th.start()
            t0 = time.perf_counter()
            conn.sendall(blob)
            t_sent = time.perf_counter() - t0
            th.join(timeout=180)
            conn.sendall(wire.build_terminate_packet())
            log = proc.communicate(timeout=60)[0]
        finally:
            srv.close()
            if proc.poll() is None:
                proc.kill()
        if len(stamps) < n_frames:
            out[name] = {"error": f"{len(stamps)} of {n_frames} frames answered", "log_tail": log[-400:] if "log" in dir() else ""}
            continue
        # steady state: from the answer of the first read-ahead batch's last frame to the last answer
        k0 = len(warm)
        rate = (n_frames - k0) / (stamps[-1] - stamps[k0 - 1])
        # windows of two batches' worth of consecutive frames that were all tracked (state OK): what a connection sustains
        # away from the (far more expensive) initialisation attempts.  Two batches, not one: the answers of ONE batch come
        # at the tracker's pace alone, whatever the receiving thread needs for the next batch.
        wl = 2 * readahead
        win = sorted(wl / (stamps[i] - stamps[i - wl]) for i in range(max(k0, wl), n_frames)
                     if all(s_ == 2 for s_ in states[i - wl + 1:i + 1]) and stamps[i] > stamps[i - wl])
        tline = next((ln for ln in log.splitlines() if ln.startswith("timing:")), "")
        tok = tline.split()
        tm = {tok[i]: float(tok[i + 1]) for i in range(1, len(tok) - 1, 2)} if tok else {}
        biggest = max((k for k in tm if k != "wall"), key=lambda k: tm[k]) if tm else None
        split = next((ln for ln in log.splitlines() if ln.startswith("ss_track timing")), None)  # SENDSLAM_TRACK_TIMING=1
        out[name] = {"frames_per_s": round(rate, 1), "ms_per_frame": round(1e3 / rate, 4), "frames": n_frames, "read_ahead": readahead,
                     "payload_bytes_per_frame": len(pk[0]), "socket_GBps": round(rate * len(pk[0]) / 1e9, 3),
                     "sender_sendall_s": round(t_sent, 4), "frames_tracking_ok": int(sum(1 for s_ in states if s_ == 2)),
                     "frames_per_s_while_tracking": None if not win else round(win[len(win) // 2], 1),
                     "tracking_states": "".join(str(s_) for s_ in states),
                     "frontdoor_seconds": tm, "largest_share": biggest, "pose_step_split": split}
    return out


def exchange_legs(timeout_s=240):
    import socket
    import subprocess
    res = {}
    for name, args, env_extra in (
            ("loop_closure_rccl_world1", ["--workload", "loop_closure", "--steps", "10", "--warmup", "2"], {"SENDSLAM_BENCH_FORCE_DIST": "1"}),
            ("stereo_rccl_world1", ["--workload", "stereo", "--steps", "10", "--warmup", "2"], {"SENDSLAM_BENCH_FORCE_DIST": "1"}),
            ("loop_closure_native_world1", ["--workload", "loop_closure", "--exchange", "native", "--steps", "10", "--warmup", "2"], {}),
            ("stereo_native_world1", ["--workload", "stereo", "--exchange", "native", "--steps", "10", "--warmup", "2"], {})):
        sock = socket.socket()
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
        sock.close()
        env = dict(os.environ, RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   HSA_ENABLE_IPC_MODE_LEGACY="0", SENDSLAM_BENCH_DIST_TIMEOUT="60", **env_extra)
        env.pop("SENDSLAM_BENCH_BACKEND", None)
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--gpus", "1"] + args, env=env, capture_output=True, text=True,
                               timeout=timeout_s)
            line = next((ln for ln in r.stdout.splitlines() if ln.startswith("{")), None)
            if r.returncode != 0 or line is None:
                res[name] = {"ok": False, "returncode": r.returncode, "stderr_tail": r.stderr[-600:]}
                continue
            j = json.loads(line)
            res[name] = {"ok": True, "value": j["value"], "unit": j["unit"], "ms_per_step": j["ms_per_step"], "rounds": j.get("rounds"),
                         "backend": j["config"].get("backend"), "exchange": j["config"].get("exchange"),
                         "ranks_reported_by_backend": j.get("ranks_reported_by_backend"),
                         "kernels": {k["name"]: k["mean_ms"] for k in j.get("kernels", [])}}
            if "fraction_of_keypoints_matched_across_eyes" in j:
                res[name]["fraction_of_keypoints_matched_across_eyes"] = j["fraction_of_keypoints_matched_across_eyes"]
        except subprocess.TimeoutExpired:
            res[name] = {"ok": False, "error": f"no result within {timeout_s} s"}
    return res


DUMP_LIMIT_BYTES = 64 * 10 ** 6  # --dump-outputs writes at most this much


def dump_outputs(path, ctx, match_out, batch):
    """--dump-outputs: the results of the context's last step as its caller receives them (ss_fetch_frame per frame and the
    step's match arrays), the frames of the batch concatenated in order, as float32 DIR/<name>.npy.  Where the whole batch
    could exceed DUMP_LIMIT_BYTES, a fixed seeded sample of its frames (bounded by the keypoint capacity, not by the
    outputs, so two builds pick the same frames)."""
    from send_slam_amd import binding
    kcap = ctx.batch_view().kp_capacity
    per_frame = kcap * (len(binding.KP_DTYPE.names) + 32 + 3) * 4 + (2 + ctx.params.n_levels) * 4
    n_frames = min(batch, max(1, DUMP_LIMIT_BYTES // per_frame))
    frames = np.arange(batch) if n_frames == batch else np.sort(np.random.default_rng(0).choice(batch, n_frames, replace=False))
    m_idx, m_d1, m_d2 = (t.cpu().numpy() for t in match_out)
    parts = {k: [] for k in ("n_keypoints", "level_counts", "keypoints", "descriptors", "match_idx", "match_d1", "match_d2")}
    for b in frames:
        kps, desc, levels = ctx.fetch_frame(int(b))
        n = len(kps)
        parts["n_keypoints"].append(n)
        parts["level_counts"].append(levels)
        parts["keypoints"].append(np.stack([kps[f].astype(np.float32) for f in binding.KP_DTYPE.names], axis=1))
        parts["descriptors"].append(desc)
        parts["match_idx"].append(m_idx[b, :n])
        parts["match_d1"].append(m_d1[b, :n])
        parts["match_d2"].append(m_d2[b, :n])
    arrays = {"frames": frames, "n_keypoints": np.array(parts.pop("n_keypoints")), "level_counts": np.stack(parts.pop("level_counts"))}
    arrays.update({k: np.concatenate(v) for k, v in parts.items()})
    os.makedirs(path, exist_ok=True)
    for name, arr in arrays.items():
        np.save(os.path.join(path, name + ".npy"), np.ascontiguousarray(arr, dtype=np.float32))


def self_launch(n):
    import signal
    import socket
    import subprocess
    one_device = os.environ.get("SENDSLAM_BENCH_ONE_DEVICE") == "1"
    if not one_device:
        import torch
        have = torch.cuda.device_count()  # no HIP context is created by this call
        if have < n:
            sys.exit(f"bench.py --gpus {n}: this node shows {have} GPU(s)")
    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = sock.getsockname()[1]
    sock.close()
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env))
    rc = 0
    pending = set(range(n))
    while pending:
        for r in sorted(pending):
            code = procs[r].poll()
            if code is None:
                continue
            pending.discard(r)
            if code != 0 and rc == 0:
                rc = code
                for q in pending:  # a rank failed: the others would wait for it in a collective
                    procs[q].send_signal(signal.SIGTERM)
        time.sleep(0.05)
    sys.exit(rc)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=0, help="timed steps (default 1000 for the metric workload: a timed region of about 0.6 s, 20 for the others)")
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--batch", type=int, default=0, help="frames per step (default 128; stereo 16)")
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--features", type=int, default=2000)
    ap.add_argument("--contexts", type=int, default=4, help="camera batches in flight per GPU")
    ap.add_argument("--full", action="store_true",
                    help="metric workload: time rounds of K steps (value = median round) and add everything beside the headline: "
                         "per-kernel events, rooflines, parity against the oracle, the CPU baseline and the other legs")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="metric workload: write the outputs of the last timed step as DIR/<name>.npy (float32)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--timed-only", action="store_true",
                    help="with --full: only warm-up + timed rounds: no isolated pass, database-streaming, host-pipeline, latency or tracking "
                         "extras (what the rocprofv3 --stats runs use, so every launch they average is a launch of the timed loop)")
    ap.add_argument("--profile-extra", default="", choices=["", "match_stream"],
                    help="run ONLY that extra leg (for rocprofv3 of the database-streaming kernel)")
    ap.add_argument("--workload", default="extract_match", choices=["extract_match", "loop_closure", "stereo"],
                    help="extract_match = the BASELINE.json metric (default); stereo = config 4 (2 ranks); loop_closure = config 5: one "
                         "2000-descriptor query against a 10 000-keyframe descriptor database sharded over the ranks (strong scaling)")
    ap.add_argument("--exchange", default="rccl", choices=["rccl", "native"],
                    help="stereo / loop_closure: rccl = torch.distributed collectives (RCCL over xGMI; gloo in rehearsals), native = the C "
                         "ABI's own peer-write all-gather (ss_xchg_*)")
    a = ap.parse_args()

    # python bench.py --gpus N (N > 1) started plainly: this process becomes the launcher.  It starts N ranks of itself
    # BEFORE making any HIP call (device_count() does not initialise the GPU), never exec()s, relays rank 0's JSON line
    # (the children share its stdout) and exits with the first failing rank's code.  Under torch.distributed.run
    # (WORLD_SIZE set) nothing of this runs.
    if "WORLD_SIZE" not in os.environ and a.gpus > 1:
        return self_launch(a.gpus)
    if a.workload == "loop_closure":
        return bench_loop_closure(a)
    if a.workload == "stereo":
        return bench_stereo(a)

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    a.gpus = world
    w, h, nf = a.width, a.height, a.features
    # 128 frames per step: with rounds of few steps (the driver's --steps 20) a round's ramp and the latency tail of its last
    # batches weigh half as much as at 64 (measured at --steps 20: 113.5 k frames/s at 64, 116.3 k at 128; with 300-step rounds
    # 118.2 k and 117.2 k)
    B = a.batch or 128
    steps = a.steps or 1000
    n_ctx = max(1, a.contexts)
    n_sets = max(2, -(-(CACHE_BYTES + (64 << 20)) // (B * w * h)))  # rotating device batches exceed the Infinity Cache
    n_sets = -(-n_sets // n_ctx) * n_ctx if n_sets > n_ctx else n_sets  # every context then meets several sets

    if a.profile_extra == "match_stream":
        import torch
        from send_slam_amd import binding
        rank, local_rank, dev, backend = dist_setup(world)
        print(json.dumps({"match_stream_roofline": bench_match_stream(binding, torch, dev, local_rank)}))
        return

    frames = make_frames(rank, n_sets, B, w, h)
    extras = a.full and not a.timed_only  # the legs beside the timed steps

    cpu_obj, cpu_outs = None, []
    if rank == 0 and a.gpus == 1 and a.full and not a.no_cpu_baseline and not a.profile_extra:
        cpu_obj, cpu_outs = cpu_baseline(frames[0], nf)  # before any HIP call in this process

    import torch
    import torch.distributed as dist
    from send_slam_amd import binding
    rank, local_rank, dev, backend = dist_setup(world)

    # A few camera batches in flight per GPU: step i runs on context i % n (own stream, own HBM
    # buffers), so the latency-bound quadtree of one batch overlaps the dense kernels of the others.
    ctxs = [binding.OrbContext(local_rank, n_features=nf, max_batch=B) for _ in range(n_ctx)]
    ctx = ctxs[0]
    d_sets = [torch.from_numpy(frames[s]).to(dev) for s in range(n_sets)]
    torch.cuda.synchronize()

    # shape the outputs once (kp_capacity is known after the first extraction)
    ctx.extract_batch_device(d_sets[0].data_ptr(), B, w, h)
    ctx.synchronize()
    kcap = ctx.batch_view().kp_capacity
    outs = [(torch.empty((B, kcap), dtype=torch.int32, device=dev), torch.empty((B, kcap), dtype=torch.int16, device=dev),
             torch.empty((B, kcap), dtype=torch.int16, device=dev)) for _ in range(n_ctx)]
    last_set = [0] * n_ctx

    def step(i):
        k = i % n_ctx
        c, (o_idx, o_d1, o_d2) = ctxs[k], outs[k]
        last_set[k] = i % n_sets
        c.extract_batch_device(d_sets[i % n_sets].data_ptr(), B, w, h)
        c.match_batch_device(0, o_idx.data_ptr(), o_d1.data_ptr(), o_d2.data_ptr())

    t_warm = time.perf_counter()
    for i in range(max(a.warmup, n_ctx)):
        step(i)
    for c in ctxs:
        c.synchronize()
    # A plain run times one region, so a short one would otherwise start while the GPU still ramps up (measured at
    # --steps 20 --warmup 5: 2 % below the same region after 0.5 s of steps); --full's median round is past that ramp.
    # The extra steps are warm-up only: the timed steps below are the same steps whatever it took.
    i = max(a.warmup, n_ctx)
    while not a.full and time.perf_counter() - t_warm < MIN_WARMUP_S:
        for _ in range(8 * n_ctx):
            step(i)
            i += 1
        for c in ctxs:
            c.synchronize()

    # --full: per-kernel HIP events on each context's own stream, live over the timed rounds (SENDSLAM_BENCH_NO_EVENTS=1
    # switches them off to measure what they cost)
    live_events = a.full and os.environ.get("SENDSLAM_BENCH_NO_EVENTS") != "1"
    for c in ctxs:
        c.profile(live_events)
        c.profile_reset()
    first_timed = max(a.warmup, n_ctx)
    next_step = [first_timed]  # the step counter runs on after the rounds: contexts and frame sets keep rotating

    def run_steps(k):
        for i in range(next_step[0], next_step[0] + k):
            step(i)
        next_step[0] += k

    def run_round(k):
        next_step[0] = first_timed  # every round runs the same steps: the last one's inputs do not depend on the round count
        run_steps(k)

    def drain():
        for c in ctxs:
            c.synchronize()  # drains the context's stream and checks the per-frame error words
    # A plain run: ONE region of exactly `steps` steps.  --full: R rounds of exactly `steps` steps, together >= 0.5 s
    # whatever --steps is, value = the median round.  Either way bracketed by barrier + synchronize, max-reduced over the ranks.
    times = timed_rounds(run_round, steps, drain, world, dev, backend, rounds=0 if a.full else 1)
    elapsed, spread = round_summary(times, B * steps * world, "frames/s")
    if a.dump_outputs and rank == 0:
        k_last = (first_timed + steps - 1) % n_ctx  # the context of the last timed step: its buffers hold that step's results
        dump_outputs(a.dump_outputs, ctxs[k_last], outs[k_last], B)
    reported = backend_world(world, dev, backend) if a.full else None

    # per-kernel HIP-event statistics of the timed loop (summed over the contexts)
    def merged_stats(cs):
        stats = []
        for c in cs:
            for s_ in c.stats():
                m = next((x for x in stats if x["name"] == s_["name"]), None)
                if m is None:
                    stats.append(dict(s_))
                else:
                    tot = m["total_ms"] + s_["total_ms"]
                    n_l = m["launches"] + s_["launches"]
                    m.update(total_ms=tot, launches=n_l, mean_ms=tot / n_l if n_l else 0.0)
        return stats
    stats = merged_stats(ctxs)
    for c in ctxs:
        c.profile(False)

    # A round of few steps pays the ramp of its first batch and the latency tail of its last one (the quadtree of the
    # last batch runs with nothing beside it).  The rate the pipeline sustains once full: one region of >= 1000 steps,
    # bracketed like a round, with the rate of each 1/25th of it from events recorded on the contexts' streams (no drain
    # in between).  Reported next to `value`, never instead.
    sustained = None
    if extras and steps < 500:
        s_steps, n_chunks = 1000, 25
        ext = [torch.cuda.ExternalStream(c.stream(), device=dev) for c in ctxs]
        chunk_ev = []

        def mark():
            evs = []
            for s_ in ext:
                e = torch.cuda.Event(enable_timing=True)
                e.record(s_)
                evs.append(e)
            chunk_ev.append(evs)
        bounds = [round(s_steps * j / n_chunks) for j in range(n_chunks + 1)]
        if use_dist(world):
            dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        mark()
        for j in range(n_chunks):
            run_steps(bounds[j + 1] - bounds[j])
            mark()
        drain()
        torch.cuda.synchronize()
        if use_dist(world):
            dist.barrier()
        s_el = max_over_ranks(time.perf_counter() - t0, world, dev, backend)
        rates = []
        for j in range(n_chunks):
            # chunk j = from the latest of the start marks to the latest of the end marks over the contexts
            ref = chunk_ev[0][0]
            t_start = max(ref.elapsed_time(e) for e in chunk_ev[j])
            t_end = max(ref.elapsed_time(e) for e in chunk_ev[j + 1])
            if t_end > t_start:
                rates.append((bounds[j + 1] - bounds[j]) * B / ((t_end - t_start) * 1e-3))
        rates.sort()
        sustained = {"value": round(B * s_steps * world / s_el, 2), "unit": "frames/s", "steps": s_steps, "ms_per_step": round(s_el / s_steps * 1e3, 4),
                     "region_s": round(s_el, 4),
                     "chunks": None if not rates else {"n": len(rates), "median": round(rates[len(rates) // 2], 1), "min": round(rates[0], 1),
                                                       "max": round(rates[-1], 1), "unit": "frames/s per rank"}}

    # parity of the measured configuration: EVERY context's last timed batch against the oracle (frame 1 + its own
    # index of that batch: the oracle costs 0.1 s per frame), then all frames of the baseline leg on context 0
    parity = None
    if rank == 0 and a.full and not a.no_cpu_baseline:
        from oracle import orb_oracle as O
        parity = True
        p = O.default_params(n_features=nf)
        for k, c in enumerate(ctxs):
            idx = outs[k][0].cpu().numpy()
            for b in sorted({1 % B, (7 * k + 3) % B}):
                okps, odesc, _ = O.extract(frames[last_set[k], b], p)
                oidx, _, _ = O.match(odesc, odesc, 50, 9, 10, exclude_self=True)
                kps_b, desc_b, _ = c.fetch_frame(b)
                n = len(kps_b)
                parity &= n == len(okps) and kps_b.tobytes() == okps.tobytes()
                parity &= bool(np.array_equal(desc_b, odesc)) and bool(np.array_equal(idx[b, :n], oidx))
        if cpu_outs:
            ctx.extract_batch_device(d_sets[0].data_ptr(), B, w, h)
            ctx.match_batch_device(0, outs[0][0].data_ptr(), outs[0][1].data_ptr(), outs[0][2].data_ptr())
            ctx.synchronize()
            idx = outs[0][0].cpu().numpy()
            for b, (okps, odesc, oidx, od1, od2) in enumerate(cpu_outs):
                kps_b, desc_b, _ = ctx.fetch_frame(b)
                n = len(kps_b)
                parity &= n == len(okps) and kps_b.tobytes() == okps.tobytes()
                parity &= bool(np.array_equal(desc_b, odesc)) and bool(np.array_equal(idx[b, :n], oidx))
        if not parity:
            sys.exit("bench.py: GPU results differ from the oracle on the benchmark frames")

    # The timed region keeps several batches in flight, so a kernel's live event pair also counts the time it waits
    # for its turn next to the other streams' kernels.  A short extra pass on ONE context gives each kernel's duration
    # when it has the GPU to itself -- the number rocprofv3's kernel trace reports for the same kernel -- reported next
    # to the live number, never instead.
    iso = {}
    if extras:
        ctx.profile(True)
        ctx.profile_reset()
        for i in range(2 * n_sets):
            ctx.extract_batch_device(d_sets[i % n_sets].data_ptr(), B, w, h)
            ctx.match_batch_device(0, outs[0][0].data_ptr(), outs[0][1].data_ptr(), outs[0][2].data_ptr())
            ctx.synchronize()
        for s_ in ctx.stats():
            iso[s_["name"]] = s_["mean_ms"]
        ctx.profile(False)

    # The same step with each frame matched against the frame BEFORE it in its batch (the frames of a set are consecutive time
    # steps of one scene: SURVEY.md section 8(d) asks for "frame t vs t + 1" beside the self-match), four batches in
    # flight like the timed region; two pairs checked against the oracle.  Never `value`.
    consecutive = None
    if extras:
        def step_prev(i):
            k = i % n_ctx
            c, (o_idx, o_d1, o_d2) = ctxs[k], outs[k]
            last_set[k] = i % n_sets
            c.extract_batch_device(d_sets[i % n_sets].data_ptr(), B, w, h)
            c.match_batch_device(1, o_idx.data_ptr(), o_d1.data_ptr(), o_d2.data_ptr())
        for i in range(n_ctx):
            step_prev(i)
        drain()
        k_prev = 200
        t1 = time.perf_counter()
        for i in range(n_ctx, n_ctx + k_prev):
            step_prev(i)
        drain()
        el_prev = time.perf_counter() - t1
        k0 = (n_ctx + k_prev - 1) % n_ctx  # the context of the last step: its outputs are that step's
        idx = outs[k0][0].cpu().numpy()
        n_kp, n_matched, ok_prev = 0, 0, True
        prev_desc = None
        for b in range(B):
            kps_b, desc_b, _ = ctxs[k0].fetch_frame(b)
            n = len(kps_b)
            if b >= 1:
                n_kp += n
                n_matched += int((idx[b, :n] >= 0).sum())
                if b <= 2 and not a.no_cpu_baseline:
                    oidx, _, _ = O.match(desc_b, prev_desc, 50, 9, 10, exclude_self=False)
                    ok_prev &= bool(np.array_equal(idx[b, :n], oidx))
            prev_desc = desc_b
        if not ok_prev:
            sys.exit("bench.py: frame-to-previous-frame matches differ from the oracle's")
        consecutive = {"frames_per_s": round(B * k_prev / el_prev, 1), "ms_per_step": round(el_prev / k_prev * 1e3, 4), "steps": k_prev,
                       "match": "frame b against frame b - 1 of its batch (th 50, ratio 0.9), frame 0 against itself",
                       "fraction_of_keypoints_matched": round(n_matched / max(n_kp, 1), 4),
                       "checked_vs_oracle": not a.no_cpu_baseline}

    # Latency path of the drop-in boundary (what the NIF / front door call per camera frame):
    # host pixels in, host keypoints + descriptors out, PCIe copies included.  Never `value`.
    lat = []
    for i in range(12 if extras else 0):
        t1 = time.perf_counter()
        ctx.extract(frames[0, i % B])
        lat.append(time.perf_counter() - t1)
    lat = sorted(lat[2:])
    single_frame_ms = lat[len(lat) // 2] * 1e3 if lat else None

    # Same boundary one step further (ss_track: extraction + match on the GPU, pose geometry on the
    # host) on a parallax sequence, rank 0 only: per-frame time in tracking state OK.  Never `value`.
    track_ms = track_ok = None
    if rank == 0 and extras:
        from send_slam_amd import synth
        cam = binding.Camera(type=b"PinHole", fx=800.0, fy=800.0, cx=w / 2.0, cy=h / 2.0, width=w, height=h, fps=30.0,
                             rgb=1, th_depth=40.0, baseline=0.0, depth_map_factor=1000.0)
        ctx.set_calibration(1, cam)
        sc = synth.scene(1000, w, h)
        tl, states = [], []
        for t in range(14):
            img = synth.parallax_frame(1000, w, h, t, sc=sc)
            t1 = time.perf_counter()
            po = ctx.track(img, 1, t / 30.0)
            dt = time.perf_counter() - t1
            states.append(po["state"])
            if po["state"] == 2 and t > 0 and states[-2] == 2:
                tl.append(dt)
        if tl:
            tl.sort()
            track_ms, track_ok = tl[len(tl) // 2] * 1e3, states.count(2)

    for c in ctxs:
        c.close()
    del d_sets, outs

    match_stream = host_pipe = frontdoor = None
    if rank == 0 and extras:
        torch.cuda.empty_cache()
        match_stream = bench_match_stream(binding, torch, dev, local_rank)
        torch.cuda.empty_cache()
        if world == 1:
            host_pipe = bench_host_pipeline(binding, frames, w, h, nf, B, local_rank)
            if os.environ.get("SENDSLAM_BENCH_NO_FRONTDOOR") != "1":
                try:
                    frontdoor = bench_frontdoor()
                except Exception as ex:  # the leg must never take the metric line down
                    frontdoor = {"error": repr(ex)}

    if use_dist(world):
        dist.destroy_process_group()
    if rank != 0:
        return

    # Configs 4 and 5 on this one GPU, each as a child process (started, never exec'ed into) at world size 1 with a real
    # "nccl" process group: the all_gather / broadcast of their steps go through RCCL, so that branch has executed on the
    # hardware the line was measured on; then the same steps over the C ABI's own exchange.  Never `value`.
    single_gpu_exchange = None
    if world == 1 and extras and os.environ.get("SENDSLAM_BENCH_NO_EXCHANGE_LEGS") != "1":
        single_gpu_exchange = exchange_legs()

    kernels = []
    for s in stats:
        if s["launches"] == 0:
            continue
        gbs = s["algorithmic_bytes"] / (s["mean_ms"] * 1e-3) / 1e9 if s["mean_ms"] > 0 and s["algorithmic_bytes"] else None
        im = iso.get(s["name"])
        kernels.append({"name": s["name"], "launches": s["launches"], "mean_ms": round(s["mean_ms"], 5),
                        "algorithmic_bytes_per_launch": s["algorithmic_bytes"],
                        "achieved_GBps": None if gbs is None else round(gbs, 1),
                        "isolated_mean_ms": None if not im else round(im, 5),
                        "isolated_GBps": None if not im or not s["algorithmic_bytes"] else round(s["algorithmic_bytes"] / (im * 1e-3) / 1e9, 1)})
    with_bytes = [k for k in kernels if k["achieved_GBps"] is not None]
    dom = max(with_bytes, key=lambda k: (k["isolated_mean_ms"] or k["mean_ms"]) * k["launches"]) if with_bytes else None
    stage_kernel = {"fast_blur_nms": "k_fast_score", "match": "k_match_mfma_x", "orient_describe": "k_orient_describe", "resize": "k_resize_lds"}
    prof = {}
    ppath = os.path.join(ROOT, "profiles", "per_frame_counters.json")
    if os.path.exists(ppath):
        prof = json.load(open(ppath)).get(f"{w}x{h}_n{nf}", {})
    roofline = None
    if dom:
        # `achieved` uses the kernel's duration with one batch in flight (HIP events on the launch stream): that is
        # the number rocprofv3's kernel trace reports for the same kernel (profiles/).  HIP events recorded while
        # several streams are in flight also count the time a kernel waits for its turn, so the live event mean is
        # reported separately and is not a kernel duration.
        ach = dom["isolated_GBps"] if dom["isolated_GBps"] else dom["achieved_GBps"]
        per_frame = prof.get(stage_kernel.get(dom["name"], ""), {}).get("hbm_bytes_per_frame")
        roofline = {"kernel": dom["name"], "bound": "hbm", "achieved": ach, "peak": HBM_PEAK_GBS,
                    "unit": "GB/s", "frac": round(ach / HBM_PEAK_GBS, 4), "traffic": None if per_frame is None else int(per_frame * B),
                    "kernel_ms": dom["isolated_mean_ms"] if dom["isolated_GBps"] else dom["mean_ms"],
                    "live_event_ms": dom["mean_ms"], "live_event_GBps": dom["achieved_GBps"],
                    "note": "integer-VALU-bound kernel (DESIGN.md section 5): the HBM fraction is reported because the contract "
                            "asks for it, not because HBM limits it; see valu_roofline"}

    # the Hamming-match kernel (k_match_mfma_x) against the two pipes it uses: the distance of a
    # (query, train) pair is a 256-term contraction of FP4 +-1 values on the matrix cores (512 ops, exact in f32), the
    # best / second-best selection stays on the VALU: the key IS the accumulator, a lane keeps the two smallest minima of its
    # groups of four rows (one instruction per pair), priced with the measured instruction costs (profiles/r01_valu_rates.json).
    match_roofline = None
    mk = next((k for k in kernels if k["name"] == "match"), None)
    rpath = os.path.join(ROOT, "profiles", "r01_valu_rates.json")
    if mk and mk.get("isolated_mean_ms") and os.path.exists(rpath):
        pairs = B * float(nf) ** 2  # the quotas are saturated on these frames (2000 <= n <= 2024)
        t = mk["isolated_mean_ms"] * 1e-3
        rates = json.load(open(rpath))
        c = rates["cycles_per_wave64_instruction_per_simd"]
        # per group of four rows of a lane: v_min3_u32 + v_min_u32 (the group's minimum), v_med3_u32 + v_min_u32 (the two smallest
        # group minima): four instructions per four pairs
        sel = (c["v_min3_u32"] + 2 * c["v_min_u32"] + c["v_med3_u32"]) / 4
        simd_cycles_per_s = rates["cus"] * 4 * rates["clock_mhz"] * 1e6
        valu_floor_ms = pairs / 64 * sel / simd_cycles_per_s * 1e3
        mfma_floor_ms = pairs * 512 / FP4_MFMA_PEAK_OPS * 1e3
        match_roofline = {"kernel": "match (k_match_mfma_x + merge)", "bound": "mfma", "achieved": float(f"{pairs * 512 / t / 1e12:.4g}"),
                          "peak": FP4_MFMA_PEAK_OPS / 1e12, "unit": "Top/s (FP4 MFMA, +-1 operands, exact)", "frac": round(pairs * 512 / t / FP4_MFMA_PEAK_OPS, 4),
                          "kernel_ms": mk["isolated_mean_ms"], "mfma_floor_ms": round(mfma_floor_ms, 4),
                          "valu_select_cycles_per_64_pairs": round(sel, 1), "valu_select_floor_ms": round(valu_floor_ms, 4),
                          "pairs_per_s": float(f"{pairs / t:.4g}"),
                          "note": "the instruction sustains 21-24 ns per 32x32x64 instruction and SIMD beside this kernel's other work "
                                  "(profiles/r03_fp4_rate_probe.txt: ~1.45 GHz under this load), i.e. 5.6-6.4e15 op/s on the chip; four are "
                                  "issued per 32 x 32 x 256 tile (the row index rides in the constant C input)"}

    # the dominant kernel against the resource that bounds it: VALU issue.  Instructions per FRAME from the committed
    # PMC pass (profiles/per_frame_counters.json: SQ_INSTS_VALU of full-batch launches / frames), duration live; peak =
    # the measured issue rate (profiles/r01_peaks.json).
    valu_roofline = None
    pk_path = os.path.join(ROOT, "profiles", "r01_peaks.json")
    if dom and dom.get("isolated_mean_ms") and os.path.exists(pk_path):
        insts = prof.get(stage_kernel.get(dom["name"], ""), {}).get("valu_wave_insts_per_frame")
        if insts:
            peak = json.load(open(pk_path))["xor_popc_lane_ops_per_s"]
            ach = insts * B * 64 / (dom["isolated_mean_ms"] * 1e-3)
            arch_peak = 256 * 4 * 2.4e9 / 2 * 64  # MI355X_MICROARCH.md: a wave64 VALU instruction issues over 2 cycles on a SIMD-32
            valu_roofline = {"kernel": dom["name"], "bound": "int_valu", "achieved": float(f"{ach:.4g}"), "peak": peak,
                             "unit": "lane-ops/s", "frac": round(ach / peak, 4), "valu_wave_instructions_per_launch": int(insts * B),
                             "peak_is": "the measured issue rate of this path's instruction class (v_bcnt / v_perm / v_dot4 / v_pk_*: 4.05 cycles "
                                        "per wave64 instruction and SIMD, profiles/r01_peaks.json)",
                             "architectural_peak": arch_peak, "frac_of_architectural_peak": round(ach / arch_peak, 4),
                             "architectural_peak_is": "2 cycles per wave64 instruction and SIMD at 2.4 GHz, 1024 SIMDs"}

    total_frames = B * steps * world
    out = {
        "metric": "frames/sec ORB extract+match @1280x720, 2000 kp/frame",
        "value": round(total_frames / elapsed, 2), "unit": "frames/s", "n_gpus": world, "steps": steps,
        "warmup": a.warmup, "ms_per_step": round(elapsed / steps * 1e3, 4), "higher_is_better": True,
        "scaling": "weak", "vs_baseline": None, "dtype": "u8", "data": "synthetic",
        "config": {"workload": f"{world}xMI355X: synthetic {w}x{h} frames, ORB extract + self-match, {nf} kp/frame",
                   "frames_per_step_per_gpu": B, "batches_in_flight_per_gpu": n_ctx,
                   "distinct_device_batches_rotated": n_sets, "device_frame_set_bytes": int(n_sets * B * w * h),
                   "n_features": nf, "n_levels": 8, "scale_factor": 1.2,
                   "match": "self-match all-pairs, j==i excluded, TH 50, ratio 9/10",
                   "parallelism": f"one camera batch per GPU x {world}, no collective"},
        "rounds": len(times), "timed_region_s": round(sum(times), 4),
    }
    if not a.full:
        print(json.dumps(out))
        return
    out.update({
        "value_spread": spread, "sustained": sustained,
        "ranks_reported_by_backend": reported, "single_gpu_exchange": single_gpu_exchange,
        "roofline": roofline, "valu_roofline": valu_roofline, "match_roofline": match_roofline,
        "match_stream_roofline": match_stream, "consecutive_frames": consecutive, "host_pipeline": host_pipe, "frontdoor": frontdoor, "kernels": kernels, "cpu_baseline": cpu_obj,
        "parity_checked_vs_oracle": parity,
        "parity_note": "oracle = the committed CPU restatement; parity with the real ORB-SLAM3 binary is unpinned (DESIGN.md section 3)",
        "single_frame_host_to_host_ms": None if single_frame_ms is None else round(single_frame_ms, 3),
        "track_frame_host_to_host_ms": None if track_ms is None else round(track_ms, 3), "track_ok_frames_of_14": track_ok,
    })
    print(json.dumps(out))


if __name__ == "__main__":
    main()
