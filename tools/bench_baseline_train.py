#!/usr/bin/env python3
"""Time the PointNet baseline's training path on one GPU: the random subsample
(ndnet.preprocessing.RandomSample: ndnet_sample_random_run's five launches), the
one-launch gather (gather_samples) and the graphed BaselineTrainer step.

(a) ``random_sample`` per call at 16 x 100k -> 4096 and 16 x 70k -> 4160 with
    int32 labels: device events around ``--iters`` back-to-back calls replayed
    from one HIP graph, ``--rounds`` rounds after a warm-up, the calls rotating
    over ``--copies`` input buffers.  Beside it, in the same rounds in rotating
    order and from a graph of its own, the same cut composed from capturable
    torch ops: ``torch.rand`` keys, ``topk`` of the S smallest, a sort of the
    picked indices, and the gathers of points (an int64 index expanded to three
    columns) and labels.  It is not bit-equal to the kernels: it only measures
    cost.  Per-kernel times of the HIP call come from one ``rocprofv3
    --kernel-trace`` run of its own (a child process that only makes the
    calls), medians over its launches.
(b) ``gather_samples`` (points only) against the three torch launches of
    ``segment_points_fps`` (index expansion, clamp, ``torch.gather``), and with
    labels against those plus a label gather.
(c) the graphed baseline step (``GraphedBaselineStep`` replays) for ``random`` /
    ``fps`` x ``samples`` / ``points`` at 16 x 100k -> 4096; the eager step
    (``BaselineTrainer(graphs=False).step`` on the host's clock, its two
    ``.item()`` reads included); the stages of a step laid out by hand between
    device events (sampler, rows, histogram, forward + loss + backward, Adam:
    ``eager_stages_us``, their sum is not a timed step); and the NDT
    ``Trainer``'s graphed step on the same batch, measured in the same run.

Nothing is judged: every figure is reported.  Writes JSON (default
profiles/baseline_train.json).  Measures on the GPU only.

    python tools/bench_baseline_train.py [--out profiles/baseline_train.json]
"""
import argparse
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=16)
ap.add_argument("--points", type=int, default=100_000)
ap.add_argument("--samples", type=int, default=4096)
ap.add_argument("--nds", type=int, default=1000, help="the NDT trainer's NDs per cloud")
ap.add_argument("--classes", type=int, default=28)
ap.add_argument("--feature-dim", type=int, default=768)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--iters", type=int, default=48, help="calls per variant and round")
ap.add_argument("--step-iters", type=int, default=20, help="train-step replays per variant and round")
ap.add_argument("--fps-step-iters", type=int, default=3, help="the same for sampler=fps (about 70 ms a step)")
ap.add_argument("--copies", type=int, default=6, help="input buffers the calls rotate over")
ap.add_argument("--no-steps", action="store_true", help="skip (c), the train steps")
ap.add_argument("--no-trace", action="store_true", help="skip the rocprofv3 kernel trace of (a)")
ap.add_argument("--trace-child", action="store_true", help=argparse.SUPPRESS)
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "baseline_train.json"))
a = ap.parse_args()

SAMPLE_SHAPES = ((a.batch, a.points, a.samples), (a.batch, 70_000, 4160))


def kernel_trace():
    """Median microseconds per k_smp_* kernel and shape from a rocprofv3 run of a child that only samples."""
    exe = shutil.which("rocprofv3")
    if exe is None:
        return {"skipped": "rocprofv3 not found"}
    with tempfile.TemporaryDirectory() as d:
        cmd = [exe, "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "run", "--", sys.executable,
               os.path.abspath(__file__), "--trace-child", "--batch", str(a.batch), "--points", str(a.points),
               "--samples", str(a.samples)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        if p.returncode != 0 or not files:
            return {"skipped": f"rocprofv3 exit {p.returncode}", "tail": p.stdout[-400:]}
        rows = {}
        with open(files[0]) as f:
            for r in csv.DictReader(f):
                name = r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
                if name.startswith("k_smp_"):
                    key = (name, int(r["Grid_Size_X"]) if "Grid_Size_X" in r else 0)
                    rows.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1000)
    out = {}
    for (name, grid), v in sorted(rows.items()):
        out.setdefault(name, []).append({"grid_x_threads": grid, "launches": len(v),
                                         "median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2)})
    return out


trace = None
if not a.trace_child and not a.no_trace:
    trace = kernel_trace()  # (before this process opens the GPU)

import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.path.insert(0, os.path.join(REPO, "ndt-net_amd"))
from ndnet.models.ndtnet import NDTNetSegmentation  # noqa: E402
from ndnet.models.pointnet import PointNetSegmentation  # noqa: E402
from ndnet.preprocessing import RandomSample, farthest_point_sample, gather_samples  # noqa: E402
from ndnet.synthetic import make_labelled_batch  # noqa: E402
from ndnet.training import BaselineTrainer, Trainer, point_accuracy_tensor, point_loss  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("bench_baseline_train.py measures on the GPU: none found")
dev = torch.device("cuda", 0)
C, R = a.classes, a.copies


def summary(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3),
            "per_round": [round(x, 3) for x in v]}


def timed(fn, iters, calls=1):
    """Microseconds per call: device events around `iters` back-to-back fn(i), each of which makes `calls` calls."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(iters):
        fn(i)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (iters * calls)


def graphed(fn, iters):
    """`iters` calls of fn(i) captured into one HIP graph, after one eager call on a side stream:
    (replay, 1, iters), a variant of rounds_of."""
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        fn(0)
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for i in range(iters):
            fn(i)
    return (lambda i: g.replay()), 1, iters


def rotate(names, r):
    return names[r % len(names):] + names[:r % len(names)]


def rounds_of(variants, rounds):
    """{name: us per call, summarised over the rounds}: every variant (fn, iters, calls per fn) once per round,
    in rotating order, after one warm-up each."""
    for v in variants.values():
        timed(*v)
    out = {k: [] for k in variants}
    for r in range(rounds):
        for k in rotate(list(variants), r):
            out[k].append(timed(*variants[k]))
    return {k: summary(v) for k, v in out.items()}


def sample_inputs(B, n):
    rng = np.random.default_rng(0)
    pts = [torch.from_numpy(rng.standard_normal((B, n, 3)).astype(np.float32) * 30).to(dev) for _ in range(R)]
    ids = [torch.from_numpy(rng.integers(0, C + 1, (B, n)).astype(np.int32)).to(dev) for _ in range(R)]
    return pts, ids


if a.trace_child:  # under rocprofv3: the calls alone, each shape in turn
    for B, n, S in SAMPLE_SHAPES:
        pts, ids = sample_inputs(B, n)
        s = RandomSample(S, seed=1)
        for i in range(40):
            s(pts[i % R], ids[i % R])
    torch.cuda.synchronize()
    sys.exit(0)

result = {
    "device": torch.cuda.get_device_name(0),
    "rounds": a.rounds, "calls_per_round": a.iters, "step_replays_per_round": a.step_iters,
    "fps_step_replays_per_round": a.fps_step_iters, "buffer_copies": R,
    "units": "microseconds per call or per step (per-round values summarised as median / min / max); hip and torch "
             "calls replayed from one HIP graph each, device events around the replay",
    "torch_sample": "capturable torch ops on the same device: torch.rand keys, topk(S, largest=False), sort of the "
                    "indices, gather of points through an int64 [B, S, 3] index and of labels; not bit-equal, cost only",
    "random_sample": [], "random_sample_kernels": trace,
}

# ---------------------------------------------------------------- (a) random_sample per call
for B, n, S in SAMPLE_SHAPES:
    pts, ids = sample_inputs(B, n)
    s = RandomSample(S, seed=1)
    o_p = torch.empty((B, S, 3), dtype=torch.float32, device=dev)
    o_l, o_i = torch.empty((B, S), dtype=torch.int32, device=dev), torch.empty((B, S), dtype=torch.int32, device=dev)
    o_c = torch.empty((B,), dtype=torch.int32, device=dev)
    keys = torch.empty((B, n), dtype=torch.float32, device=dev)

    def hip(i):
        s(pts[i % R], ids[i % R], out_points=o_p, out_labels=o_l, out_counts=o_c, out_indices=o_i)

    def composed(i):
        keys.uniform_()
        idx = torch.topk(keys, S, dim=1, largest=False, sorted=False).indices
        idx = torch.sort(idx, dim=1).values
        torch.gather(pts[i % R], 1, idx.unsqueeze(2).expand(B, S, 3), out=o_p)
        torch.gather(ids[i % R], 1, idx, out=o_l)

    t = rounds_of({"hip": graphed(hip, a.iters), "torch": graphed(composed, a.iters)}, a.rounds)
    result["random_sample"].append({"batch": B, "points": n, "samples": S, "labels": True, "hip_us": t["hip"],
                                    "torch_us": t["torch"],
                                    "torch_over_hip": round(t["torch"]["median"] / t["hip"]["median"], 2)})
    del pts, ids

# ---------------------------------------------------------------- (b) gather_samples
B, n, S = a.batch, a.points, a.samples
host_pts, host_gt = make_labelled_batch(B, n, C)
d_pts = torch.from_numpy(host_pts).to(dev)
d_ids = torch.from_numpy(host_gt.argmax(-1).astype(np.int32)).to(dev)
del host_gt
idx = RandomSample(S, seed=2)(d_pts)[3]  # any valid indices: the gather's cost does not depend on which
o_p = torch.empty((B, S, 3), dtype=torch.float32, device=dev)
o_l, o_c = torch.empty((B, S), dtype=torch.int32, device=dev), torch.empty((B,), dtype=torch.int32, device=dev)
gi = torch.empty((B, S, 3), dtype=torch.int64, device=dev)
gl = torch.empty((B, S), dtype=torch.int64, device=dev)


def torch_points(i):
    gi.copy_(idx.unsqueeze(2).expand(B, S, 3))
    gi.clamp_(min=0)
    torch.gather(d_pts, 1, gi, out=o_p)


def torch_both(i):
    torch_points(i)
    gl.copy_(idx)
    gl.clamp_(min=0)
    torch.gather(d_ids, 1, gl, out=o_l)


t = rounds_of({
    "hip_points": graphed(lambda i: gather_samples(d_pts, idx, out_points=o_p, out_counts=o_c), a.iters),
    "torch_points": graphed(torch_points, a.iters),
    "hip_points_labels": graphed(lambda i: gather_samples(d_pts, idx, d_ids, out_points=o_p, out_labels=o_l,
                                                          out_counts=o_c), a.iters),
    "torch_points_labels": graphed(torch_both, a.iters)}, a.rounds)
result["gather_samples"] = {"batch": B, "points": n, "samples": S, **{k + "_us": v for k, v in t.items()},
                            "torch_over_hip_points": round(t["torch_points"]["median"] / t["hip_points"]["median"], 2)}

# ---------------------------------------------------------------- (c) the train steps
if not a.no_steps:
    steps = {}
    for sampler in ("random", "fps"):
        for loss in ("samples", "points"):
            torch.manual_seed(0)
            tr = BaselineTrainer(PointNetSegmentation(3, C, a.feature_dim), 1e-3, S, C, dev, ddp=False, graphs=True,
                                 sampler=sampler, loss=loss, seed=3)
            s_p, s_g = tr.graph_inputs(d_pts.shape, d_ids.shape)
            s_p.copy_(d_pts)
            s_g.copy_(d_ids)
            iters = a.step_iters if sampler == "random" else a.fps_step_iters
            t = rounds_of({"graphed": (lambda i: tr.step_graphed(s_p, s_g), iters)}, a.rounds)
            # the stages, laid out by hand on the graphed trainer's model: device events between them, the
            # median over the steps (the label conversion and the .item() reads of a real step are not in it)
            from ndnet import segment
            from ndnet.preprocessing import nearest_sample
            names = ("sampler", "rows", "histogram", "forward_loss_backward", "adam")
            per = {k: [] for k in names}
            for it in range(2 + max(3, iters // 2)):
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(names) + 1)]
                ev[0].record()
                if sampler == "random":
                    smp, slab, scnt, _ = tr.random_sample(d_pts, d_ids)
                else:
                    smp, slab, scnt = gather_samples(d_pts, farthest_point_sample(d_pts, S), d_ids)
                ev[1].record()
                rows = tr._rows_iota(B) if loss == "samples" else nearest_sample(d_pts, smp, sample_counts=scnt)
                ev[2].record()
                hist = segment.row_histogram(rows, slab if loss == "samples" else d_ids, S, C + 1, -1)
                ev[3].record()
                tr.model.train()
                pred = tr.net(smp)
                lv = point_loss(pred, hist)
                tr.opt.zero_grad(set_to_none=True)
                lv.backward()
                point_accuracy_tensor(pred.detach(), hist)
                ev[4].record()
                tr.opt.step()
                ev[5].record()
                torch.cuda.synchronize()
                if it >= 2:
                    for k, name in enumerate(names):
                        per[name].append(ev[k].elapsed_time(ev[k + 1]) * 1e3)
            stages = {k: round(statistics.median(v), 1) for k, v in per.items()}
            # the eager step itself: BaselineTrainer(graphs=False).step, label conversion, torch's Adam and
            # the two .item() reads included, on the host's clock
            torch.manual_seed(0)
            tr_e = BaselineTrainer(PointNetSegmentation(3, C, a.feature_dim), 1e-3, S, C, dev, ddp=False,
                                   sampler=sampler, loss=loss, seed=3)
            eager = []
            for r in range(1 + a.rounds):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(iters):
                    tr_e.step(d_pts, d_ids)
                torch.cuda.synchronize()
                if r:  # (the first round warms up)
                    eager.append((time.perf_counter() - t0) * 1e6 / iters)
            steps[f"{sampler}/{loss}"] = {"graphed_us": t["graphed"], "eager_step_us": summary(eager),
                                          "eager_stages_us": stages,
                                          "eager_stages_sum_us": round(sum(stages.values()), 1),
                                          "clouds_per_s_graphed": round(B / t["graphed"]["median"] * 1e6, 1)}
            del tr, tr_e
            torch.cuda.empty_cache()
    # the NDT trainer's graphed step on the same batch, for context
    torch.manual_seed(0)
    ndt = Trainer(NDTNetSegmentation(3, C, a.feature_dim), 1e-3, a.nds, C, dev, ddp=False, graphs=True, loss="points")
    s_p, s_g = ndt.graph_inputs(d_pts.shape, d_ids.shape)
    s_p.copy_(d_pts)
    s_g.copy_(d_ids)
    t = rounds_of({"graphed": (lambda i: ndt.step_graphed(s_p, s_g), a.step_iters)}, a.rounds)
    result["train_step"] = {"batch": B, "points": n, "samples": S, "classes": C, "feature_dim": a.feature_dim,
                            "clouds": "synthetic L (make_labelled_batch), integer labels", "baseline": steps,
                            "ndt_trainer_graphed_us": {"nds": a.nds, "loss": "points", **t["graphed"]}}

os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
print(json.dumps({k: v for k, v in result.items() if k not in ("units", "torch_sample")}))
