#!/usr/bin/env python3
"""Time PipelinedSegmentation with per-point labels against the pipeline as it
was and against the one-graph-per-batch labelled step.

Shape C2 by default: 16 x 100k points -> 1000 NDs, synthetic U and L clouds
(ndnet.synthetic), the pipelines configured as bench.py configures them (one
NDT stream for U, two for L).  Per cloud kind, in rounds that alternate the
variants (the order rotated by one each round), after a warm-up of each:

* (a) ``plain``: the pipeline with its arguments at their defaults
* (b) ``labels_none``: ``point_labels="none"``
* (c) ``labels_nearest``: ``point_labels="nearest"``
* (d) ``labels_nearest_ragged``: (c) with ``ragged=True`` and counts spread
  evenly over n / 2 .. n
* (c8) ``labels_nearest_u8``: (c) with ``label_dtype=torch.uint8``
  -- each ``replay_steps(--steps)`` (>= 200) on a resident batch, device events
  around the call
* (e) ``streamed_u8``: (c8) under ``replay_streamed`` with pinned host batches
  in and every step's uint8 labels copied back to pinned memory (the
  PCIe-inclusive loop), and ``streamed_plain``: the pipeline as it was under
  ``replay_streamed``; a host clock around ``--steps`` calls ending in a
  device synchronise
* ``graphed_labelled`` / ``graphed_plain``: ``GraphedSegmentation`` with and
  without ``point_labels="nearest"``, one replay per batch (what
  tools/bench_point_labels.py times as ``graph_point_labels``): the labelled
  path without this pipeline
* ``stage_us``: the NDT-stage graph and the forward-stage graph of (a) and (c)
  replayed alone on one stream (no overlap), for reading the step times
* ``label_launch_us``: ``segment.point_labels`` alone as int32 and as uint8,
  --iters launches replayed from one HIP graph, rotating over --copies row
  and label buffers

Reports clouds/s (median, min, max and every round) and the ratio
(c) / graphed_labelled.  No figure is asserted.  Writes JSON (default
profiles/pipeline_labels.json).  Measures on the GPU only.

    python tools/bench_pipeline_labels.py [--out profiles/pipeline_labels.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=16)
ap.add_argument("--points", type=int, default=100_000)
ap.add_argument("--nds", type=int, default=1000)
ap.add_argument("--classes", type=int, default=28)
ap.add_argument("--feature-dim", type=int, default=768)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--steps", type=int, default=240, help="pipeline steps per variant and round")
ap.add_argument("--iters", type=int, default=40, help="isolated label launches per round")
ap.add_argument("--copies", type=int, default=16, help="row / label buffers the isolated launches rotate over")
ap.add_argument("--kinds", default="U,L")
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pipeline_labels.json"))
a = ap.parse_args()
if a.steps < 200:
    sys.exit("at least 200 steps per variant and round")

import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.path.insert(0, os.path.join(REPO, "ndt-net_amd"))
from ndnet import segment  # noqa: E402
from ndnet.models.ndtnet import NDTNetSegmentation  # noqa: E402
from ndnet.pipeline import GraphedSegmentation, PipelinedSegmentation  # noqa: E402
from ndnet.synthetic import make_batch  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("bench_pipeline_labels.py measures on the GPU: none found")
dev = torch.device("cuda", 0)
B, N, K = a.batch, a.points, a.nds
COLS = a.classes + 1


def summary(v, digits=1):
    return {"median": round(statistics.median(v), digits), "min": round(min(v), digits),
            "max": round(max(v), digits), "per_round": [round(x, digits) for x in v]}


def event_us(fn):
    """Microseconds of fn() on the device: events on the caller's stream around it."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3


def host_us(fn):
    """Microseconds of fn() on the host clock, the device idle before and after."""
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e6


def graphed_launches(fn, iters):
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
    return g.replay


result = {
    "shape": {"batch": B, "points": N, "nds": K, "classes": a.classes, "feature_dim": a.feature_dim},
    "device": torch.cuda.get_device_name(0),
    "rounds": a.rounds, "steps_per_round": a.steps, "label_launches_per_round": a.iters, "label_copies": a.copies,
    "units": "clouds_per_s: batch x steps over the time of the timed window, per round (median / min / max); "
             "step_us: the window over its steps; stage_us and label_launch_us: microseconds per replay / launch",
    "timing": "replay_steps and the graphed replays: device events around the window; the streamed loops: a "
              "host clock around the calls, ending in a device synchronise",
    "kinds": {},
}
torch.manual_seed(0)
model = NDTNetSegmentation(3, a.classes, a.feature_dim).to(dev).eval()
for kind in a.kinds.split(","):
    ndt_streams = 2 if kind == "L" else 1  # as bench.py runs the two kinds
    host = make_batch(kind, B, N)
    pts = torch.from_numpy(host).to(dev)
    counts = [int(c) for c in np.linspace(N // 2, N, B).round()]

    def pipe(**kw):
        p = PipelinedSegmentation(model, K, B, N, device=dev, ndt_streams=ndt_streams, **kw)
        p.load_resident(pts, counts if kw.get("ragged") else None)
        return p

    pipes = {"plain": pipe(),
             "labels_none": pipe(point_labels="none"),
             "labels_nearest": pipe(point_labels="nearest"),
             "labels_nearest_ragged": pipe(point_labels="nearest", ragged=True),
             "labels_nearest_u8": pipe(point_labels="nearest", label_dtype=torch.uint8)}
    streamed = {"streamed_plain": pipe(), "streamed_u8": pipe(point_labels="nearest", label_dtype=torch.uint8)}
    graphs = {"graphed_plain": GraphedSegmentation(model, K, B, N, device=dev),
              "graphed_labelled": GraphedSegmentation(model, K, B, N, device=dev, point_labels="nearest")}
    for g in graphs.values():
        g.points.copy_(pts)
    R = pipes["plain"].R
    host_in = [torch.from_numpy(host).pin_memory() for _ in range(2)]
    host_labels = [torch.empty((B, N), dtype=torch.uint8).pin_memory() for _ in range(2)]

    def streamed_loop(p, labelled):
        def run():
            for s in range(a.steps):
                p.replay_streamed(host_in[s % 2], labels_host=host_labels[s % 2] if labelled else None)
        return run

    def graphed_loop(g):
        def run():
            for _ in range(a.steps):
                g.replay()
        return run

    # name -> (timer, callable running a.steps steps)
    variants = {nm: (event_us, (lambda p=p: p.replay_steps(a.steps))) for nm, p in pipes.items()}
    variants["streamed_plain"] = (host_us, streamed_loop(streamed["streamed_plain"], False))
    variants["streamed_u8"] = (host_us, streamed_loop(streamed["streamed_u8"], True))
    for nm, g in graphs.items():
        variants[nm] = (event_us, graphed_loop(g))
    names = list(variants)
    for timer, fn in variants.values():  # warm-up: every shape and graph the windows use
        timer(fn)
    us = {nm: [] for nm in names}
    for r in range(a.rounds):
        for nm in names[r % len(names):] + names[:r % len(names)]:
            timer, fn = variants[nm]
            us[nm].append(timer(fn))
    torch.cuda.synchronize(dev)
    # the labelled pipelines computed what the graphed labelled step computes
    ref = graphs["graphed_labelled"]
    same = {nm: bool(torch.equal(pipes[nm].labels[0], ref.point_labels)) for nm in ("labels_nearest",)}
    u8 = pipes["labels_nearest_u8"].labels[0]
    ref_u8 = torch.where(ref.point_labels < 0, torch.full_like(ref.point_labels, 255), ref.point_labels).to(torch.uint8)
    same["labels_nearest_u8"] = bool(torch.equal(u8, ref_u8))
    streamed["streamed_u8"].labels_copied.synchronize()
    same["streamed_u8_host"] = bool(torch.equal(host_labels[(a.steps - 1) % 2], u8.cpu()))
    rcs_ok = all(st.rc == 0 for p in list(pipes.values()) + list(streamed.values())
                 for plan in p.plans for st in plan.host_stats())

    # the stage graphs alone, back to back on one stream
    stage = {}
    for nm in ("plain", "labels_nearest"):
        p = pipes[nm]
        for what, gs in (("ndt", p.g_ndt), ("fwd", p.g_fwd)):
            def run(gs=gs):
                for s in range(a.steps):
                    gs[s % R].replay()
            event_us(run)
            stage[f"{nm}_{what}"] = summary([event_us(run) / a.steps for _ in range(a.rounds)], 2)

    # the label launches alone
    scores = torch.randn(B, K, COLS, device=dev)
    rows = [ref.point_rows.clone() for _ in range(a.copies)]
    nd_labels = torch.empty((B, K), dtype=torch.int32, device=dev)
    launch = {}
    for nm, dt in (("int32", torch.int32), ("uint8", torch.uint8)):
        outs = [torch.empty((B, N), dtype=dt, device=dev) for _ in range(a.copies)]
        replay = graphed_launches(lambda i, outs=outs: segment.point_labels(
            scores, rows[i % a.copies], out=outs[i % a.copies], nd_labels=nd_labels), a.iters)
        event_us(replay)
        launch[nm] = (replay, outs)
    lus = {nm: [] for nm in launch}
    for r in range(a.rounds):
        for nm in (list(launch) if r % 2 == 0 else list(launch)[::-1]):
            lus[nm].append(event_us(launch[nm][0]) / a.iters)
    per_nd = 4 * B * K * COLS + 4 * B * K
    label_bytes = {"int32": 8 * N * B + per_nd, "uint8": 5 * N * B + per_nd}
    label_launch = {nm: dict(summary(v, 2), algorithmic_bytes=label_bytes[nm],
                             GBps=round(label_bytes[nm] / statistics.median(v) / 1e3, 1)) for nm, v in lus.items()}

    rate = {nm: summary([B * a.steps / (t * 1e-6) for t in v]) for nm, v in us.items()}
    step = {nm: round(statistics.median(v) / a.steps, 2) for nm, v in us.items()}
    ratio = round(rate["labels_nearest"]["median"] / rate["graphed_labelled"]["median"], 3)
    result["kinds"][kind] = {
        "ndt_streams": ndt_streams, "ring": R, "ragged_counts": counts,
        "clouds_per_s": rate, "step_us": step,
        "labels_nearest_over_graphed_labelled": ratio,
        "pipeline_beats_graphed_labelled": bool(ratio > 1.0),
        "stage_us": stage, "label_launch_us": label_launch,
        "labels_equal_graphed": same, "every_cloud_rc_0": bool(rcs_ok),
    }
    print(kind, json.dumps({"step_us": step, "ratio": ratio, "stage_us": {k: v["median"] for k, v in stage.items()},
                            "label_launch_us": {k: v["median"] for k, v in label_launch.items()},
                            "same": same, "rc0": rcs_ok}), flush=True)
    del pipes, streamed, graphs, rows, launch
    torch.cuda.empty_cache()
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
print("wrote", a.out)
