#!/usr/bin/env python3
"""Benchmark: clouds/s of NDT preprocessing + NDTNetSegmentation forward.

Metric (BASELINE.json): "clouds/sec NDT preprocess+PointNet fwd, 100k pts ->
1000 NDs, batch=16".  One step = one batch of 16 synthetic 100k-point clouds
(SURVEY §8d generator U, float32, resident in HBM before timing) through
``ndt_preprocessing`` (voxel-size bisection, per-voxel ND, KL prune) and the
eval-mode ``NDTNetSegmentation(point_dim=3, num_classes=28, feature_dim=768)``
forward -- the path tools/train.py:67-69 runs each iteration.

Multi-GPU (one process per GPU): every rank processes its own contiguous
shard of 16 clouds (weak scaling, no collective on the data path -- SURVEY
§8e; config C4 at --gpus 8: 128 clouds, 16 per rank); value = all clouds /
max-over-ranks time.  ``--gpus N`` with N > 1 and no WORLD_SIZE in the
environment launches the N ranks itself (torch.distributed.run as a child
process, before this process touches the GPU); under torch.distributed.run
WORLD_SIZE must equal --gpus.  ``--dry-run`` runs the launcher, rendezvous,
shard split and the timing/max-over-ranks logic on CPU (gloo) with no GPU
work (tests/test_bench_launcher.py).

A plain run sets up, settles and warms up, times the --steps steps, writes
the last step's outputs if ``--dump-outputs DIR`` is given, and prints the
JSON line with the headline (metric, value, unit, ms_per_step, dtype, config).
``--full`` then goes on to everything else, each a run of its own after the
timed steps: the other distribution, the PCIe-inclusive rate, the C2 / C3 /
C5 config lines, the stage and chain timing, and

  roofline     -- the dominant kernel stage, achieved vs MI355X peak
  cpu_baseline -- the CPU oracle (sequential C port of the reference core) +
                  torch fp32 CPU forward, timed on a bounded sample (rank 0, N=1)
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(REPO, "ndt-net_amd"))

HBM_PEAK_GBS = 8000.0       # MI355X_MICROARCH.md: HBM3E 8 TB/s (spec)
FP32_MFMA_PEAK_TF = 157.3   # MI355X_MICROARCH.md: FP32 matrix 157.3 TF (dense)
BF16_MFMA_PEAK_TF = 2500.0  # MI355X_MICROARCH.md: BF16 MFMA ~2.5 PF dense (no sparsity)


def pointnet_flops_per_cloud(n: int, F: int, C: int) -> float:
    """2 x the Conv1d/Linear MACs NDTNetSegmentation executes per cloud."""
    pt = (3 * 64 + 64 * 128 + 128 * 1024) + 12 * 64 + (64 * 64 + 64 * 128 + 128 * 1024) \
        + 64 * 128 + 128 * F + (64 + F) * 512 + 512 * 256 + 256 * 128 + 128 * (C + 1)
    fc = (1024 * 512 + 512 * 256 + 256 * 9) + (1024 * 512 + 512 * 256 + 256 * 4096)
    return 2.0 * (pt * n + fc)


def chain_layers(F: int, C: int) -> tuple:
    """The per-point layers each k_pn_chain launch must compute, at their
    unpadded sizes, with the matrix instruction they run on: ((K, N, kind),
    ...) per chain, kind "x6" (fp32-accurate split-bf16: six
    v_mfma_f32_16x16x32_bf16 products per fp32 MAC) or "f32"
    (v_mfma_f32_16x16x4_f32).  The kernels' recomputation of conv1 / conv2 in
    later chains and the zero padding are overhead, not counted."""
    from ndnet.models import pointnet_hip as P
    x6 = "x6" if P.SPLIT_BF16 else "f32"
    nar = x6 if P.X6_NARROW else "f32"
    return (((3, 64, "f32"), (64, 128, nar), (128, 1024, x6)),
            ((12, 64, "f32"), (64, 64, nar), (64, 128, nar), (128, 1024, x6)),
            ((64, 128, x6), (128, F, x6)),
            ((64, 512, x6), (512, 256, x6), (256, 128, x6), (128, C + 1, nar)))


def chain_flops_per_point(F: int, C: int) -> tuple:
    """Algorithmic FLOPs per point of the four k_pn_chain launches (2 K N per layer)."""
    return tuple(2.0 * sum(K * N for K, N, _ in ch) for ch in chain_layers(F, C))


def chain_ideal_s_per_point(F: int, C: int) -> tuple:
    """Seconds per point of each chain at the dense peak of the instructions
    its layers issue: x6 layers at BF16_MFMA_PEAK_TF / 6 (six bf16 products per
    fp32 MAC), f32 layers at FP32_MFMA_PEAK_TF."""
    peak = {"x6": BF16_MFMA_PEAK_TF * 1e12 / 6.0, "f32": FP32_MFMA_PEAK_TF * 1e12}
    return tuple(sum(2.0 * K * N / peak[kind] for K, N, kind in ch) for ch in chain_layers(F, C))


def dump_outputs(dirname: str, out, rank: int, cap_bytes: int = 48 << 20) -> None:
    """--dump-outputs: the last timed step's return value as float32 .npy files,
    whole (16 x 1000 x 29 log-probs: 1.9 MB; config C5's three levels: 6.5 MB).
    ``log_probs.npy``, or ``log_probs_level<i>.npy`` per level with --levels;
    ranks beyond the first add ``.rank<r>`` before the extension.  Shapes whose
    outputs exceed ``cap_bytes`` in all are written as a fixed (seed 0) sample of the
    flattened elements, in index order."""
    os.makedirs(dirname, exist_ok=True)
    outs = out if isinstance(out, list) else [out]
    names = [f"log_probs_level{i}" for i in range(len(outs))] if isinstance(out, list) else ["log_probs"]
    cap = cap_bytes // 4  # float32 elements in all
    total = sum(o.numel() for o in outs)
    for name, o in zip(names, outs):
        a = o.detach().to(torch.float32).cpu().numpy()
        if total > cap:
            keep = np.random.default_rng(0).choice(a.size, size=max(1, a.size * cap // total), replace=False)
            a = a.reshape(-1)[np.sort(keep)]
        tag = f".rank{rank}" if rank else ""
        np.save(os.path.join(dirname, f"{name}{tag}.npy"), a)


def _free_port() -> int:
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as so:
        so.bind(("127.0.0.1", 0))
        return so.getsockname()[1]


def _self_launch(nproc: int) -> int:
    """One rank per GPU as fresh child processes (no GPU call has happened in
    this process: importing torch does not initialise HIP)."""
    import subprocess
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
           os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.run(cmd).returncode


def _dry_run(args, rank: int, world: int) -> None:
    """The multi-rank skeleton on CPU: gloo rendezvous, the shard split, the
    barrier / max-over-ranks timing of --steps no-op steps, the JSON line."""
    import torch.distributed as tdist
    from ndnet import distributed as D
    D.init("gloo")
    start, count = D.shard(args.batch * world, world, rank)
    shards = [None] * world
    if tdist.is_initialized():
        tdist.all_gather_object(shards, (start, count))
    else:
        shards = [(start, count)]
    D.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        pass
    D.barrier()
    elapsed = D.max_over_ranks(max(time.perf_counter() - t0, 1e-9))
    if rank == 0:
        print(json.dumps({"metric": "dry-run (no GPU work)", "n_gpus": world, "steps": args.steps,
                          "global_batch": args.batch * world, "shards": shards,
                          "max_elapsed_s": elapsed}))
    if tdist.is_initialized():
        tdist.destroy_process_group()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also measure everything beside the headline: the other "
                         "distribution, the PCIe-inclusive rate, the C2 / C3 / C5 config lines, stage and chain "
                         "timing with the roofline, the CPU baseline (each still has its own --no-... switch)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step returned (the log-probs a caller of the timed path "
                         "receives) as DIR/<name>.npy, float32")
    ap.add_argument("--no-stream-lines", action="store_true",
                    help="skip the C2 / C3 lines over consecutive batches on several streams")
    ap.add_argument("--settle-ms", type=float, default=300.0,
                    help="untimed replays of the step before the warmup steps (GPU clocks to steady state)")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--points", type=int, default=100_000)
    ap.add_argument("--nds", type=int, default=1000)
    ap.add_argument("--kind", default="U", choices=["U", "L"])
    ap.add_argument("--feature-dim", type=int, default=768)
    ap.add_argument("--classes", type=int, default=28)
    ap.add_argument("--cpu-baseline-seconds", type=float, default=8.0)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--eager", action="store_true", help="launch kernels from Python each step (no HIP graph)")
    ap.add_argument("--no-pipeline", action="store_true",
                    help="one HIP graph per step, NDT then forward of the same batch (no cross-step overlap)")
    ap.add_argument("--levels", default=None,
                    help="config C5: comma-separated NDs per level, e.g. 2000,1000,500 (downsample, then prune; "
                         "a forward per level)")
    ap.add_argument("--no-other", action="store_true", help="skip the other-distribution (U <-> L) timing")
    ap.add_argument("--dist-backend", default="nccl", choices=["nccl", "gloo"],
                    help="process group of the timing barrier / max over ranks (nccl = RCCL)")
    ap.add_argument("--dry-run", action="store_true",
                    help="launcher / shard split / timing skeleton on CPU (gloo), no GPU work")
    args = ap.parse_args()

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(_self_launch(args.gpus))
    from ndnet import distributed as D
    rank, local, world = D.world_from_env()
    if world != args.gpus:
        print(f"bench.py: WORLD_SIZE {world} != --gpus {args.gpus}", file=sys.stderr)
        sys.exit(2)
    if args.dry_run:
        _dry_run(args, rank, world)
        return
    # one GPU per rank; a box with fewer GPUs than ranks (a rehearsal of the
    # multi-rank path on one card, --dist-backend gloo) wraps around
    ndev = max(1, torch.cuda.device_count())
    torch.cuda.set_device(local % ndev)
    dev = torch.device("cuda", local % ndev)
    # RCCL ("nccl") carries only the barrier and the max-over-ranks time: no
    # collective on the data path
    dist = D.init(args.dist_backend, dev)

    from ndnet.models.ndtnet import NDTNetSegmentation
    from ndnet.models import pointnet_hip
    from ndnet.preprocessing.ndtnet_preprocessing import ndt_preprocessing, get_plan
    from ndnet.synthetic import make_batch
    from ndnet import _lib

    B, n, k, F, C = args.batch, args.points, args.nds, args.feature_dim, args.classes
    levels = tuple(int(v) for v in args.levels.split(",")) if args.levels else None
    if levels:
        k = levels[0]  # the stage timing / roofline below cover the first level's downsample + forward
    # this rank's contiguous shard of the job's B * world clouds (cloud i of the
    # job is the SURVEY §8d generator's seed i)
    shard0, shard_n = D.shard(B * world, world, rank)
    assert shard_n == B
    pts = torch.from_numpy(make_batch(args.kind, B, n, seed0=shard0)).to(dev)
    per_dev = -(-world // ndev)
    # ranks sharing one card (the one-card rehearsal): k_front's cloud-major
    # deal keeps any two launches at once deadlock-free (csrc/ndt_front.h), but
    # more ranks per card than that, each with pipelines of its own, could
    # want more k_front workgroups than the chip holds.  Each rank's k_front
    # then takes CUs / (ranks per card x its NDT streams) (pipe_share); the
    # cached plan of the stage lines takes CUs / ranks per card.
    from ndnet.pipeline import PIPE_CU_SHARE, PIPE_CU_SHARE_MULTI

    def pipe_share(ndt_streams: int = 1):
        base = PIPE_CU_SHARE if ndt_streams == 1 else PIPE_CU_SHARE_MULTI
        return None if per_dev == 1 else max(base, ndt_streams) * per_dev
    if per_dev > 1:
        get_plan(B, n, k, -1, dev).set_cu_share(per_dev)
    torch.manual_seed(1234)
    model = NDTNetSegmentation(3, C, F).to(dev).eval()
    with torch.no_grad():
        for m in model.modules():  # non-trivial BN statistics
            if isinstance(m, torch.nn.BatchNorm1d):
                m.running_mean.uniform_(-0.2, 0.2)
                m.running_var.uniform_(0.5, 1.5)

    def eager_step():
        if levels:
            from ndnet.preprocessing.ndtnet_preprocessing import ndt_multiscale
            return [model(p, c) for p, c, _ in ndt_multiscale(levels, pts)]
        p, c, _ = ndt_preprocessing(k, pts)
        return model(p, c)

    if args.eager:
        step = eager_step
    else:
        # the same kernels, launched from one captured HIP graph per step
        from ndnet.pipeline import GraphedSegmentation
        if args.no_pipeline:
            graphed = GraphedSegmentation(model, k, B, n, device=dev, levels=levels)
        else:
            # step i: NDT of batch i on one stream || forward(s) of batch i - 1 on another
            from ndnet.pipeline import PipelinedSegmentation
            graphed = PipelinedSegmentation(model, k, B, n, device=dev, levels=levels, cu_share=pipe_share())
        if hasattr(graphed, "load_resident"):
            graphed.load_resident(pts)
        else:
            graphed.points.copy_(pts)
        step = graphed.replay

    def run_steps(k: int):
        """k steps: the pipeline's event-ordered replays where it has them, else k replays."""
        if not args.eager and hasattr(graphed, "replay_steps"):
            return graphed.replay_steps(k)
        out = None
        for _ in range(k):
            out = step()
        return out

    def run_plan():
        """The NDT plan the timed steps ran (the pipeline's first, else the cached one)."""
        g = None if args.eager else graphed
        return g.plan if g is not None and hasattr(g, "plan") else get_plan(B, n, k, -1, dev)

    def all_run_stats():
        """host_stats() of every plan the timed steps ran (the pipeline's NDT
        streams each have a plan of their own)."""
        g = None if args.eager else graphed
        plans = getattr(g, "plans", None) or [run_plan()]
        return [st for pl in plans for st in pl.host_stats()]

    with torch.no_grad():
        # settle: replay the step for --settle-ms before the W warmup steps, so
        # the timed steps run at the GPU's steady clocks (20 steps of 0.26 ms
        # right after graph capture measured 6% slower than steady state:
        # profiles/r02e_settle.txt); untimed, and every timed step still runs
        # the whole NDT + forward
        t_settle = time.perf_counter()
        n_settle = 0
        while args.settle_ms > 0 and (time.perf_counter() - t_settle) * 1e3 < args.settle_ms:
            out = run_steps(12)
            n_settle += 12
            torch.cuda.synchronize()
        out = run_steps(args.warmup)
        torch.cuda.synchronize()
        D.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = run_steps(args.steps)
        t_enq = time.perf_counter() - t0  # host time to enqueue the K steps (diagnostic)
        torch.cuda.synchronize()
        D.barrier()
        torch.cuda.synchronize()
        elapsed = time.perf_counter() - t0
    elapsed = D.max_over_ranks(elapsed)
    total_clouds = world * B * args.steps
    value = total_clouds / elapsed
    stats = all_run_stats()
    assert all(s.rc == 0 for s in stats), [s.rc for s in stats]
    assert all(torch.isfinite(o).all() for o in (out if isinstance(out, list) else [out]))
    if args.dump_outputs:
        # the last timed step's return value, before anything below replays the step again
        dump_outputs(args.dump_outputs, out, rank)

    if rank == 0:
        line = {
            "metric": ("clouds/sec NDT preprocess+PointNet fwd, 100k pts->1000 NDs, batch=16" if not levels else
                       "clouds/sec NDT multiscale {%s} NDs + PointNet fwd per level, 100k pts, batch=16"
                       % ",".join(map(str, levels))),
            "value": round(value, 2),
            "unit": "clouds/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "settle": {"ms": args.settle_ms, "steps": n_settle},
            "ms_per_step": round(elapsed / args.steps * 1e3, 4),
            "host_enqueue_ms_per_step": round(t_enq / args.steps * 1e3, 4),
            "pipeline_front_share": list(getattr(graphed, "front_share", [])) if not args.eager else None,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": (f"f64 NDT; PointNet fp32-accurate split-bf16x3 (6 products) on {11 if pointnet_hip.X6_NARROW else 7}"
                      " per-point layers, fp32 MFMA on the K=16 first layers and the TNet / seg-bias FC layers"
                      if pointnet_hip.SPLIT_BF16 else "f64 NDT; PointNet fp32 MFMA"),
            "data": f"synthetic {args.kind} clouds (SURVEY 8d), random-init weights",
            "full": args.full,
            "measurement_notes": [
                "U clouds reach exactly k occupied voxels at the accepted size, so their level-1 prune removes "
                "nothing: the run counts the KL events (stats num_events / num_kl) and builds the sorted list only "
                "on demand (ndnet_ndt_set_lazy_list; bit-equal to the eager build by test_lazy_list_equals_eager). "
                "The L line (other_distribution, with --full) times the KL scoring, sort and prune of ~121 pruned "
                "NDs per cloud.",
                "Every ring slot replays one resident batch (bench inputs already in HBM, as the contract asks; "
                "the slots' inputs total ~115 MB, within the 256 MB Infinity Cache); pcie_inclusive (with --full) "
                "streams the batch from pinned host memory instead."] if not levels else None,
            "config": {"workload": (f"batch {B} x {n} pts -> {k} NDs, NDTNetSegmentation F={F} C={C} eval"
                                    if not levels and world == 1 else
                                    f"C4: {B * world} clouds end to end ({n} pts -> {k} NDs -> NDTNetSegmentation "
                                    f"F={F} C={C} eval), {B} per rank over {world} GPUs, contiguous shards"
                                    if not levels else
                                    f"C5: batch {B} x {n} pts -> downsample {levels[0]} -> prune "
                                    f"{' -> '.join(map(str, levels[1:]))}, NDTNetSegmentation F={F} C={C} eval "
                                    f"per level"),
                       "launch": "eager" if args.eager else (
                           "hip graph per step (ndnet.pipeline.GraphedSegmentation)" if args.no_pipeline
                           else f"NDT(batch i) || forward(batch i-1): a hip graph per stage and ring slot "
                                f"({graphed.R} buffers), one NDT stream + {graphed.F} forward streams (step i's "
                                f"forward on stream i % {graphed.F}) ordered by events only, joined once per timed "
                                f"region (ndnet.pipeline.PipelinedSegmentation.replay_steps)"),
                       "global_batch": B * world, "points": n, "nds": k, "parallelism": f"dp{world} (clouds sharded)",
                       "dist_backend": args.dist_backend if world > 1 else None,
                       **({"rehearsal": f"{world} ranks on {ndev} GPU(s)"} if world > ndev else {})},
        }
    if not args.full:
        # the plain run ends here: everything below takes runs of its own (--full)
        if rank == 0:
            print(json.dumps(line))
        if dist:
            torch.distributed.destroy_process_group()
        return

    # ---- the other synthetic distribution on the same graph (SURVEY §8d "also
    # report L"): the L clouds exercise the prune (~128 of ~1128 NDs removed) ----
    other, other_pts = None, None
    if not args.eager and not levels and not args.no_other:
        okind = "L" if args.kind == "U" else "U"
        opts = torch.from_numpy(make_batch(okind, B, n, seed0=shard0)).to(dev)
        # the L clouds' NDT stage (~0.2 ms) outlasts a forward: their pipeline
        # runs two NDT streams, each with a plan of its own (62k vs 56k clouds/s;
        # the U clouds' one NDT stream: profiles/r04_pipe_knobs.txt), unless the
        # NDT streams are set explicitly (NDNET_PIPE_NDT_STREAMS)
        o_graphed, o_ndt_streams = graphed, None
        if (okind == "L" and not args.no_pipeline and hasattr(graphed, "replay_steps")
                and "NDNET_PIPE_NDT_STREAMS" not in os.environ):
            from ndnet.pipeline import PipelinedSegmentation
            o_ndt_streams = 2
            o_graphed = PipelinedSegmentation(model, k, B, n, device=dev, ndt_streams=o_ndt_streams,
                                              cu_share=pipe_share(o_ndt_streams))
        if hasattr(o_graphed, "load_resident"):
            o_graphed.load_resident(opts)
        else:
            o_graphed.points.copy_(opts)

        def o_steps(m: int):
            if hasattr(o_graphed, "replay_steps"):
                return o_graphed.replay_steps(m)
            for _ in range(m):
                o_graphed.replay()

        with torch.no_grad():
            t_s = time.perf_counter()  # the same untimed settle as the headline's
            while args.settle_ms > 0 and (time.perf_counter() - t_s) * 1e3 < min(args.settle_ms, 200.0):
                o_steps(12)
                torch.cuda.synchronize()
            o_steps(max(2, args.warmup))
            torch.cuda.synchronize()
            D.barrier()
            t0 = time.perf_counter()
            o_steps(args.steps)
            torch.cuda.synchronize()
            D.barrier()
            t_o = D.max_over_ranks(time.perf_counter() - t0)
        o_plans = getattr(o_graphed, "plans", None) or [run_plan()]
        o_stats = [st for pl in o_plans for st in pl.host_stats()]
        assert all(st.rc == 0 for st in o_stats), [st.rc for st in o_stats]
        ost = o_plans[0].host_stats()
        other_pts = opts
        other = {"kind": okind, "value": round(total_clouds / t_o, 2), "unit": "clouds/s",
                 "ms_per_step": round(1e3 * t_o / args.steps, 4),
                 "pruned_per_cloud": round(float(np.mean([st.num_nds - k for st in ost])), 1)}
        if o_ndt_streams:
            other["ndt_streams"] = o_ndt_streams
        # free the L pipeline's plans: the stage lines below time the plans a
        # standalone caller has (include/ndnet_amd.h: with fewer live k_front
        # plans than the cloud-major deal's bound, no lane admission)
        del o_plans, o_stats
        if o_graphed is not graphed:
            del o_graphed
            import gc
            gc.collect()
        if hasattr(graphed, "load_resident"):
            graphed.load_resident(pts)
        else:
            graphed.points.copy_(pts)
        with torch.no_grad():
            step()
            step()

    # ---- PCIe-inclusive rate (never `value`): each step first copies the batch
    # from pinned host memory into the graph's input buffer on the same stream, then replays.
    pcie = None
    if not args.eager:
        host_pts = pts.cpu().pin_memory()
        with torch.no_grad():
            graphed.points.copy_(host_pts, non_blocking=True)
            step()
            torch.cuda.synchronize()
            D.barrier()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                graphed.points.copy_(host_pts, non_blocking=True)
                out = step()
            torch.cuda.synchronize()
            t_pcie = D.max_over_ranks(time.perf_counter() - t0)
        pcie = {"value": round(total_clouds / t_pcie, 2), "unit": "clouds/s",
                "ms_per_step": round(1e3 * t_pcie / args.steps, 4),
                "h2d_bytes_per_step": int(host_pts.numel() * 4),
                "how": "pinned host f32 xyz -> HBM copy, then the same graph replay, serialised on one stream"}
        if hasattr(graphed, "replay_streamed"):
            # the serving loop: H2D of batch i+1 on a copy stream overlapped with step i
            with torch.no_grad():
                graphed.points.copy_(host_pts)
                for _ in range(2):
                    graphed.replay_streamed(host_pts)
                torch.cuda.synchronize()
                D.barrier()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    out = graphed.replay_streamed(host_pts)
                torch.cuda.synchronize()
                t_ov = D.max_over_ranks(time.perf_counter() - t0)
            pcie["overlapped"] = {"value": round(total_clouds / t_ov, 2),
                                  "ms_per_step": round(1e3 * t_ov / args.steps, 4),
                                  "how": "PipelinedSegmentation.replay_streamed: ring of input buffers, copy stream"}
    stats = all_run_stats()
    assert all(s.rc == 0 for s in stats), [s.rc for s in stats]
    assert all(torch.isfinite(o).all() for o in (out if isinstance(out, list) else [out]))

    # ---- BASELINE.json configs 2 and 3 as their own lines: the NDT stage alone
    # (16 x 100k -> 1000 NDs) and the forward alone (16 x 1000 x 12-D NDs), each
    # one HIP graph per step over the same resident inputs ----
    config_lines = None
    if not args.eager and not levels:
        def graph_rate(fn):
            side = torch.cuda.Stream(device=dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.no_grad(), torch.cuda.stream(side):
                fn()
                fn()
            torch.cuda.current_stream(dev).wait_stream(side)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.no_grad(), torch.cuda.graph(g):
                fn()
            for _ in range(3):
                g.replay()
            torch.cuda.synchronize()
            D.barrier()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                g.replay()
            torch.cuda.synchronize()
            D.barrier()
            return D.max_over_ranks(time.perf_counter() - t0)
        t_ndt = graph_rate(lambda: ndt_preprocessing(k, pts))
        rows_p, rows_c, _ = ndt_preprocessing(k, pts)
        rows = torch.cat((rows_p, rows_c), dim=2).contiguous()
        t_fwd = graph_rate(lambda: model(rows[..., :3], rows[..., 3:]))
        config_lines = {
            "C2_ndt_only": {"value": round(total_clouds / t_ndt, 2), "unit": "clouds/s",
                            "ms_per_step": round(1e3 * t_ndt / args.steps, 4),
                            "workload": f"batch {B} x {n} pts -> {k} NDs, ndt_preprocessing alone"},
            "C3_forward_only": {"value": round(total_clouds / t_fwd, 2), "unit": "clouds/s",
                                "ms_per_step": round(1e3 * t_fwd / args.steps, 4),
                                "workload": f"batch {B} x {k} x 12-D NDs, NDTNetSegmentation F={F} C={C} eval forward alone"},
        }
        # the same two stages over a stream of batches (round 6: C2 201k vs
        # 167k sequential at CU share 2, 146-158k at share 1; C3 127-130k vs
        # 100-102k, profiles/r06su_stream_lines.txt): consecutive batches on
        # S streams, each stream its own workspace and graph (the NDT stage: a
        # plan per stream; the forward: a pointnet_hip workspace slot per
        # stream), so one batch's latency-bound phases overlap the next one's
        # (the way the headline pipeline overlaps them).  Every step is one
        # whole batch; the lines above replay one graph after another.
        if not args.no_stream_lines and per_dev == 1:
            from ndnet.preprocessing.ndtnet_preprocessing import NdtPlan
            from ndnet.models import pointnet_hip

            def streams_rate(S, body):
                sts = [torch.cuda.Stream(device=dev) for _ in range(S)]
                cur = torch.cuda.current_stream(dev)
                graphs = []
                for i, st in enumerate(sts):
                    st.wait_stream(cur)
                    with torch.no_grad(), torch.cuda.stream(st):
                        body(i)
                        body(i)
                torch.cuda.synchronize()
                for i, st in enumerate(sts):
                    g = torch.cuda.CUDAGraph()
                    with torch.no_grad(), torch.cuda.graph(g, stream=st):
                        body(i)
                    graphs.append(g)
                torch.cuda.synchronize()

                def run(m):
                    for st in sts:
                        st.wait_stream(cur)
                    for s_ in range(m):
                        with torch.cuda.stream(sts[s_ % S]):
                            graphs[s_ % S].replay()
                    for st in sts:
                        cur.wait_stream(st)
                run(3 * S)
                torch.cuda.synchronize()
                D.barrier()
                t0_ = time.perf_counter()
                run(args.steps)
                torch.cuda.synchronize()
                D.barrier()
                return D.max_over_ranks(time.perf_counter() - t0_)

            S_ndt, S_fwd = 2, 3
            splans = [NdtPlan(B, n, k, -1, device=dev) for _ in range(S_ndt)]
            ndt_share = int(os.environ.get("NDNET_STREAMS_NDT_SHARE", "2"))
            if ndt_share > 1:
                for pl in splans:
                    pl.set_cu_share(ndt_share)
            souts = [torch.zeros((B, k, 12), dtype=torch.float32, device=dev) for _ in range(S_ndt)]
            t_ndt_s = streams_rate(S_ndt, lambda i: splans[i].run(pts, None, souts[i], None))
            assert all(st.rc == 0 for pl in splans for st in pl.host_stats())
            assert all(torch.equal(o, rows) for o in souts), "stream-line NDT rows differ from ndt_preprocessing's"

            def fwd_slot(i):
                with pointnet_hip.workspace_slot(i):
                    return model(rows[..., :3], rows[..., 3:])
            t_fwd_s = streams_rate(S_fwd, fwd_slot)
            del splans, souts
            config_lines["C2_ndt_only_streams"] = {
                "value": round(total_clouds / t_ndt_s, 2), "unit": "clouds/s",
                "ms_per_step": round(1e3 * t_ndt_s / args.steps, 4),
                "workload": f"as C2_ndt_only, consecutive batches on {S_ndt} streams (a plan each, CU share {ndt_share})"}
            config_lines["C3_forward_only_streams"] = {
                "value": round(total_clouds / t_fwd_s, 2), "unit": "clouds/s",
                "ms_per_step": round(1e3 * t_fwd_s / args.steps, 4),
                "workload": f"as C3_forward_only, consecutive batches on {S_fwd} streams (a workspace slot each)"}

        # ---- config C5 (BASELINE configs[4], tools/train_multiscale.py): the
        # multiscale step -- downsample to 2000, prune to 1000 and 500, a
        # forward per level -- through the same stream pipeline ----
        c5 = (2000, 1000, 500)
        from ndnet.pipeline import PipelinedSegmentation
        p5 = PipelinedSegmentation(model, c5[0], B, n, device=dev, levels=c5, cu_share=pipe_share())
        p5.load_resident(pts)
        with torch.no_grad():
            t5 = time.perf_counter()
            while (time.perf_counter() - t5) * 1e3 < min(args.settle_ms, 200.0):
                p5.replay_steps(12)
                torch.cuda.synchronize()
            p5.replay_steps(max(2, args.warmup))
            torch.cuda.synchronize()
            D.barrier()
            t5 = time.perf_counter()
            p5.replay_steps(args.steps)
            torch.cuda.synchronize()
            D.barrier()
            t5 = D.max_over_ranks(time.perf_counter() - t5)
        assert all(st.rc == 0 for pl in p5.plans for st in pl.host_stats())
        config_lines["C5_multiscale"] = {
            "value": round(total_clouds / t5, 2), "unit": "clouds/s", "ms_per_step": round(1e3 * t5 / args.steps, 4),
            "front_share": list(p5.front_share),
            "workload": f"batch {B} x {n} pts ({args.kind}) -> downsample {c5[0]} -> prune {c5[1]} -> prune {c5[2]}, "
                        f"NDTNetSegmentation F={F} C={C} eval per level (3 forwards per step), stream pipeline"}
        del p5

    # ---- stage timing (HIP events on the stream the kernels run on) ----
    # Each timed region starts behind a ~2 ms device-side sleep on the same
    # stream, so the host has queued every launch of the region before its
    # first event fires: the events bracket kernel time, not Python launch gaps.
    plan = get_plan(B, n, k, -1, dev)
    stage_names = ["reset+limits", "bisection (15 launches)", "dense ids", "binning", "welford + LU chains",
                   "kl (scores, order, prune, rows)"]
    reps = max(3, min(args.steps, 10))
    sleep_cycles = int(5e6)

    def ndt_stage_ms(points):
        """Per-stage ms of ndt_preprocessing on ``points`` (the plan's events)."""
        _lib.lib().ndnet_ndt_set_timing(plan.handle, 1)
        acc = np.zeros(6)
        with torch.no_grad():
            for _ in range(reps):
                torch.cuda._sleep(sleep_cycles)
                ndt_preprocessing(k, points)
                ms = np.zeros(6, np.float32)
                _lib.lib().ndnet_ndt_stage_ms(plan.handle, ms.ctypes.data)
                acc += ms
        _lib.lib().ndnet_ndt_set_timing(plan.handle, 0)
        return acc / reps

    stage_ms = ndt_stage_ms(pts)
    other_stage_ms = ndt_stage_ms(other_pts) if other_pts is not None else None
    fwd_ms = 0.0
    pointnet_hip.chain_timing = []
    with torch.no_grad():
        p, c, _ = ndt_preprocessing(k, pts)
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda._sleep(sleep_cycles)
            e0.record()
            model(p, c)
            e1.record()
            e1.synchronize()
            fwd_ms += e0.elapsed_time(e1)
    fwd_ms /= reps
    chain_in_fwd_ms = np.zeros(4)
    for i, e0, e1 in pointnet_hip.chain_timing:
        chain_in_fwd_ms[i] += e0.elapsed_time(e1) / reps
    pointnet_hip.chain_timing = None
    # each chain alone, R launches back to back between two events on the
    # launch stream: the per-launch duration rocprofv3's kernel statistics
    # report (the events around each chain inside a forward add that launch's
    # dispatch latency).  The inputs and the workspace are the last forward's;
    # chain D re-arms the max-pool buffer last, as a forward does.
    chain_ms = chain_in_fwd_ms.copy()
    if pointnet_hip.available():
        ws = pointnet_hip._folded(model)["ws"].get((B, k, dev, 0))
        if ws is not None:
            blk = p.as_strided((B, k, 12), (k * 12, 12, 1))
            out_d = torch.empty((B, k, C + 1), device=dev)
            R = 20
            with torch.no_grad():
                for i in range(4):
                    o = out_d if i == 3 else None
                    ws.chain(i, blk, out=o)  # warm
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda._sleep(sleep_cycles)
                    e0.record()
                    for _ in range(R):
                        ws.chain(i, blk, out=o)
                    e1.record()
                    e1.synchronize()
                    chain_ms[i] = e0.elapsed_time(e1) / R
    ndt_ms = float(stage_ms.sum())
    hip_fwd = pointnet_hip.available()
    flops = pointnet_flops_per_cloud(k, F, C) * B
    ndt_bytes = (24.0 * n + 48.0 * k) * B  # fp64 xyz read once + fp32 12-D write
    # The roofline entry is the kernel that holds the most time per step (launch
    # count x duration): the four k_pn_chain launches of a forward taken as one
    # set (they are one kernel, launched once per chain), k_front, k_welford.
    cflops = np.array(chain_flops_per_point(F, C)) * k * B
    cideal = np.array(chain_ideal_s_per_point(F, C)) * k * B  # seconds at the issued instructions' peak
    chains_info = {"ms": [round(float(v), 4) for v in chain_ms],
                   "fp32_equiv_tflops": [round(float(f / (t * 1e-3) / 1e12), 2) if t > 0 else None
                                         for f, t in zip(cflops, chain_ms)],
                   "frac_of_issued_peak": [round(float(i / (t * 1e-3)), 4) if t > 0 else None
                                           for i, t in zip(cideal, chain_ms)],
                   "in_forward_ms": [round(float(v), 4) for v in chain_in_fwd_ms],
                   "in_forward_basis": "events around each chain launch inside a forward (adds its dispatch latency)",
                   "forward_other_ms": round(fwd_ms - float(chain_in_fwd_ms.sum()), 4),
                   "forward_other": "per-cloud FC heads, weight folds and launch boundaries of the forward"}
    # the NDT front (k_reset + k_front: limits, every bisection pass, dense ids
    # and binning in ONE launch) reads the f32 points once into registers and
    # writes them grouped by ND: 12 N in + 12 N out per cloud
    front = plan.path == 2  # k_front: events 1-4 are recorded back to back after it
    if front:
        # events 1-4 follow k_front back to back: their intervals hold no kernel
        stage_names = ["k_front (limits, bisection, dense ids, binning)", "welford + LU chains",
                       "kl (scores, order, prune, rows)"]
        stage_ms = np.array([stage_ms[0], stage_ms[4], stage_ms[5]])
        if other_stage_ms is not None:
            other_stage_ms = np.array([other_stage_ms[0], other_stage_ms[4], other_stage_ms[5]])
    if other is not None and other_stage_ms is not None:
        other["stages_ms"] = {nm: round(float(v), 4) for nm, v in zip(stage_names, other_stage_ms)}
        other["stages_basis"] = "per-stage HIP events around ndt_preprocessing on the other distribution's batch"
    ndt_single = {  # stage index -> (kernel, algorithmic bytes per launch, what)
        0: ("k_front", 24.0 * n * B, "f32 xyz read once + written once grouped by ND (12 N + 12 N per cloud)")
           if front else ("k_limits", 12.0 * n * B, "f32 xyz read once (12 N per cloud)"),
        (1 if front else 4): ("k_welford", 12.0 * n * B + (4 + 24 + 72) * k * B,
                              "grouped f32 xyz read once + count/mean/covariance write per ND"),
    }
    cand = ([("chains", -1, float(chain_ms.sum()))] if hip_fwd else []) + \
           [("ndt", i, float(stage_ms[i])) for i in ndt_single]
    kind, ci, ms = max(cand, key=lambda c: c[2])
    pmc_path = os.path.join(REPO, "profiles", "pmc_traffic.json")
    pmc = {}
    if os.path.exists(pmc_path):
        with open(pmc_path) as f:
            pmc = json.load(f)
    if kind == "chains":
        # fp32-equivalent FLOP/s against the peak of the instructions issued:
        # x6 layers at 2.5 PF / 6, f32 layers at 157.3 TF (chain_ideal_s_per_point)
        achieved = float(cflops.sum()) / (ms * 1e-3) / 1e12
        peak = float(cflops.sum()) / float(cideal.sum()) / 1e12
        roofline = {"kernel": "k_pn_chain (4 launches per forward: chains A-D)", "bound": "mfma",
                    "achieved": round(achieved, 3), "peak": round(peak, 2), "unit": "TFLOP/s",
                    "frac": round(achieved / peak, 4), "traffic": None,
                    "algorithmic": f"{cflops.sum() / 1e9:.3f} fp32-equivalent GFLOP per forward ({B} clouds x {k} "
                                   f"points; 2 K N per point per layer at unpadded sizes)",
                    "peak_basis": "the issued-instruction peak: split-bf16 (x6) layers at BF16 2500 TF / 6 products, "
                                  "f32 layers at 157.3 TF, weighted by each layer's FLOPs",
                    "ms": round(ms, 4), "ms_basis": "sum over chains A-D of the per-launch time of 20 back-to-back "
                                                          "launches of that chain between two events on its stream "
                                                          "(rocprofv3's per-launch duration)",
                    "all_chains": chains_info}
        rows = [pmc.get(f"k_pn_chain {c}") for c in "ABCD"]
        if all(r and "hbm_bytes" in r for r in rows):
            roofline["traffic"] = round(sum(r["hbm_bytes"] for r in rows))
            roofline["traffic_source"] = f"{pmc.get('_source', pmc_path)}: k_pn_chain A-D, sum over the 4 launches " \
                f"of 2 x FETCH_SIZE + WRITE_SIZE"
    else:
        name, nbytes, what = ndt_single[ci]
        achieved = nbytes / (ms * 1e-3) / 1e9
        roofline = {"kernel": name, "bound": "hbm", "achieved": round(achieved, 2), "peak": HBM_PEAK_GBS,
                    "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 5), "traffic": None,
                    "algorithmic": f"{nbytes / 1e6:.2f} MB per launch: {what}", "ms": round(ms, 4),
                    "all_chains": chains_info}
        # HBM bytes per launch of that kernel from the committed rocprofv3 PMC
        # passes (tools/gpu.sh pmc ndt -> tools/pmc_summary.py --json): FETCH_SIZE doubled
        # per MI355X_MICROARCH.md's gfx950 correction, plus WRITE_SIZE
        for kname, row in pmc.items():
            if kname != "_source" and roofline["kernel"].startswith(kname.split("<")[0]) and "hbm_bytes" in row:
                roofline["traffic"] = round(row["hbm_bytes"])
                roofline["traffic_source"] = f"{pmc.get('_source', pmc_path)}: {kname}, " \
                    f"2 x FETCH_SIZE {row['FETCH_SIZE']:.0f} KB + WRITE_SIZE {row['WRITE_SIZE']:.0f} KB per launch"
                break
    # the per-step time of each candidate, and the NDT single kernels beside it
    roofline["per_step_ms"] = {("k_pn_chain x4" if kd == "chains" else ndt_single[i][0]): round(t, 4)
                               for kd, i, t in cand}
    if "k_front" in roofline["per_step_ms"] and front and stage_ms[0] > 0:
        roofline["k_front"] = {"ms": round(float(stage_ms[0]), 4),
                               "algorithmic_gbs": round(24.0 * n * B / (stage_ms[0] * 1e-3) / 1e9, 1),
                               "frac_of_peak": round(24.0 * n * B / (stage_ms[0] * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}
        frow = next((r for kk, r in pmc.items() if kk.startswith("k_front")), None)
        if frow and "hbm_bytes" in frow:
            roofline["k_front"]["pmc_bytes"] = round(frow["hbm_bytes"])
    # the scatter-stage kernel (per-ND Welford over the grouped points) and the
    # MFMA-busy fraction of the four point-MLP chains, from the same PMC passes:
    # busy = SQ_VALU_MFMA_BUSY_CYCLES (MFMA cycles summed over SIMDs) /
    # (GRBM_GUI_ACTIVE (summed over the 8 XCDs) x 128 SIMDs per XCD)
    if pmc:
        wrow = next((r for kk, r in pmc.items() if kk.startswith("k_welford")), None)
        wi = 1 if front else 4
        if wrow and "hbm_bytes" in wrow and stage_ms[wi] > 0:
            wbytes = ndt_single[wi][1]
            roofline["k_welford"] = {"ms": round(float(stage_ms[wi]), 4),
                                     "algorithmic_gbs": round(wbytes / (stage_ms[wi] * 1e-3) / 1e9, 1),
                                     "pmc_bytes": round(wrow["hbm_bytes"]),
                                     "pmc_gbs": round(wrow["hbm_bytes"] / (stage_ms[wi] * 1e-3) / 1e9, 1),
                                     "frac_of_peak": round(wrow["hbm_bytes"] / (stage_ms[wi] * 1e-3) / 1e9
                                                           / HBM_PEAK_GBS, 4)}
        busy, num, den = {}, 0.0, 0.0
        for c in "ABCD":
            row = pmc.get(f"k_pn_chain {c}")
            if row and row.get("GRBM_GUI_ACTIVE") and "SQ_VALU_MFMA_BUSY_CYCLES" in row:
                busy[c] = round(row["SQ_VALU_MFMA_BUSY_CYCLES"] / (row["GRBM_GUI_ACTIVE"] * 128.0), 4)
                num += row["SQ_VALU_MFMA_BUSY_CYCLES"]
                den += row["GRBM_GUI_ACTIVE"] * 128.0
        if busy:
            roofline["all_chains"]["mfma_busy"] = busy
            roofline["all_chains"]["mfma_busy_set"] = round(num / den, 4)
            roofline["all_chains"]["mfma_busy_source"] = (
                f"{pmc.get('_source', pmc_path)}: SQ_VALU_MFMA_BUSY_CYCLES / (GRBM_GUI_ACTIVE x 128 SIMDs per XCD), "
                f"summed over the 4 chains for the set")
    roofline["ndt_end_to_end"] = {"bytes": ndt_bytes, "ms": round(ndt_ms, 4),
                                  "gbs": round(ndt_bytes / (ndt_ms * 1e-3) / 1e9, 2),
                                  "unit": "SURVEY 8d: 24N+48k per cloud over the whole NDT stage"}

    # ---- CPU baseline (rank 0, N = 1), bounded samples of the same workload ----
    #  * reference-faithful: oracle/cpu_ref.c -- the reference core's cost
    #    structure (8 pthreads with a mutex + condvar per voxel, GSL-style heap
    #    traffic per KL call, O(E^2) insertion, -O0), one cloud at a time as
    #    ndtnet_preprocessing.py:27 runs it; calibrated against the reference's
    #    own compiled estimate stage in the build container
    #    (profiles/r02_cpu_ref_calibration.txt);
    #  * all cores: the -O2 oracle, one cloud per thread on every core we use;
    #  * the NDTNetSegmentation forward as torch fp32 on the CPU.
    cpu = None
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        sys.path.insert(0, os.path.join(REPO, "oracle"))
        import oracle as O
        from concurrent.futures import ThreadPoolExecutor
        host = pts.cpu().numpy().astype(np.float64)
        nproc = os.cpu_count() or 1
        cores = min(16, nproc)  # the GPU box's CPU share per GPU (labelled per_gpu_cpu_share)
        budget = args.cpu_baseline_seconds
        t_ref, done = 0.0, 0
        while done < B and t_ref < 0.45 * budget:
            t1 = time.perf_counter()
            _, _, rc = O.cref_downsample(host[done], k)
            t_ref += time.perf_counter() - t1
            assert rc == 0
            done += 1
        # all cores: 2 clouds per thread, one cloud per call
        jobs = [host[i % B] for i in range(2 * cores)]
        t1 = time.perf_counter()
        with ThreadPoolExecutor(cores) as ex:
            rcs = list(ex.map(lambda c: O.legacy_downsample_rows(c, k), jobs))
        t_all = time.perf_counter() - t1
        assert all(r == 0 for r in rcs)
        cpu_model = NDTNetSegmentation(3, C, F).eval()
        cpu_model.load_state_dict({kk: v.cpu() for kk, v in model.state_dict().items()})
        torch.set_num_threads(cores)
        pc = torch.randn(1, k, 3)
        cc = torch.randn(1, k, 9)
        t_fwd, fdone = 0.0, 0
        with torch.no_grad():
            while fdone < 4 and t_fwd < 0.25 * budget:
                t1 = time.perf_counter()
                cpu_model.forward_torch(pc, cc)
                t_fwd += time.perf_counter() - t1
                fdone += 1
        fwd = t_fwd / fdone
        ref_cloud = t_ref / done
        all_cloud = t_all / len(jobs)
        cpu = {"value": round(1.0 / (ref_cloud + fwd), 3), "unit": "clouds/s", "cores": 8, "kind": "port",
               "sample": f"{done} clouds one at a time through oracle/cpu_ref.c (the reference core's structure: "
                         f"8 pthreads, mutex per voxel, -O0; {ref_cloud * 1e3:.1f} ms/cloud) + torch fp32 CPU "
                         f"forward ({cores} threads, {fwd * 1e3:.1f} ms/cloud)",
               "nproc": nproc,
               "calibration": "estimate stage only: cpu_ref / compiled reference estimate stage = 1.08 (U), "
                              "1.15 (L) in the build container (profiles/r02_cpu_ref_calibration.txt); the KL leg "
                              "(GSL calls, kullback_leibler.c:28-127) is uncalibrated: GSL is absent here",
               "per_gpu_cpu_share": {"value": round(1.0 / (all_cloud + fwd), 3), "unit": "clouds/s", "cores": cores,
                                     "sample": f"{len(jobs)} clouds through the -O2 oracle (oracle/ndt_oracle.c), one "
                                               f"cloud per thread on {cores} threads ({all_cloud * 1e3:.2f} ms/cloud "
                                               f"aggregate), + the torch forward ({cores} threads per cloud)",
                                     "note": f"{cores} of the host's {nproc} CPUs: the CPU share the GPU box gives one "
                                             f"GPU (gpurun: 16 per GPU), not every core of the host"}}

    if rank == 0:
        line.update({
            "stages_ms": {nm: round(float(v), 4) for nm, v in zip(stage_names, stage_ms)}
                         | ({"pointnet_fwd": config_lines["C3_forward_only"]["ms_per_step"],
                             "pointnet_fwd_eager": round(fwd_ms, 4)} if config_lines else
                            {"pointnet_fwd": round(fwd_ms, 4)}),
            "roofline": roofline,
            "other_distribution": other,
            "config_lines": config_lines,
            "cpu_baseline": cpu,
            "pcie_inclusive": pcie,
        })
        print(json.dumps(line))
    if dist:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
