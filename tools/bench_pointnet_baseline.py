#!/usr/bin/env python3
"""Time the PointNet-on-FPS baseline on the GPU (ndnet.models.pointnet,
ndnet.preprocessing.nearest_sample, segment.segment_points_fps).

Every figure is the median over ``--rounds`` timed windows; a window is
``reps`` replays of one captured graph (torch.cuda.graph, one stream) between
two device events, after two eager warm-up calls and one untimed replay.  Where
two versions are compared their windows alternate, round by round, in one
process; minimum and maximum of the rounds are kept beside the median.

* nearest-sample rows at 16 x 100k points -> S = 4096: the HIP kernel
  (ndnet_nearest_sample_run) against the same rows composed from torch ops, a
  loop over chunks of points of ``torch.cdist`` + ``argmin`` (the full
  [16, 100k, 4096] distance matrix is 26 GB and cannot be materialised).  How
  many of the composition's rows equal the kernel's is counted, not required:
  cdist need not round like the definition.
* the baseline eval forward at 16 x 4096 (F = 768, C = 28): the HIP chains
  against ``forward_torch`` on the same GPU.
* the whole baseline step at 16 x 100k -> 4096 samples (FPS, forward, rows,
  labels: ``segment_points_fps`` into preallocated buffers, one graph), its
  stages one by one, and beside them the NDT-Net step figures of
  profiles/pipeline_labels.json (16 x 100k -> 1000 NDs), copied from that file
  as they stand there: another sample count, taken by tools/bench_pipeline_labels.py.

Nothing is fixed in advance: whatever is measured is written, also where the
torch composition wins.  Writes JSON (default profiles/pointnet_baseline.json).
Measures on the GPU only.

    python tools/bench_pointnet_baseline.py [--out profiles/pointnet_baseline.json]
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=16)
ap.add_argument("--points", type=int, default=100_000)
ap.add_argument("--samples", type=int, default=4096)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--cdist-chunk", type=int, default=4000, help="points per cdist call (x batch x samples x 4 bytes)")
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pointnet_baseline.json"))
a = ap.parse_args()

sys.path.insert(0, os.path.join(REPO, "ndt-net_amd"))
import torch  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("bench_pointnet_baseline.py measures on the GPU; none is visible")
from ndnet import segment  # noqa: E402
from ndnet.models.pointnet import PointNetSegmentation  # noqa: E402
from ndnet.preprocessing import farthest_point_sample, nearest_sample  # noqa: E402
from ndnet.synthetic import make_batch  # noqa: E402


def capture(fn):
    """fn twice eagerly on a side stream, then captured there: (graph, fn's result)."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
        fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        out = fn()
    g.replay()
    torch.cuda.synchronize()
    return g, out


def window_us(g, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def compare(graphs: dict, reps: dict, rounds: int) -> dict:
    """us per replay of every graph, the versions' windows alternating round by round."""
    per = {k: [] for k in graphs}
    for _ in range(rounds):
        for k, g in graphs.items():
            per[k].append(window_us(g, reps[k]))
    return {k: {"us_median": round(statistics.median(v), 2), "us_min": round(min(v), 2), "us_max": round(max(v), 2),
                "replays_per_window": reps[k], "rounds": rounds} for k, v in per.items()}


B, n, S = a.batch, a.points, a.samples
res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__,
       "timing": "device events around a window of replays of one captured graph (one stream), after two eager "
                 "calls and one untimed replay; median / min / max over the rounds; compared versions alternate"}
pts = torch.from_numpy(make_batch("U", B, n)).cuda()
with torch.no_grad():
    idx = farthest_point_sample(pts, S).long()
    smp = torch.gather(pts, 1, idx.unsqueeze(2).expand(B, S, 3)).contiguous()

# ---- 1. nearest-sample rows: the kernel against chunked cdist + argmin ----
rows_k = torch.empty((B, n), dtype=torch.int32, device="cuda")
rows_t = torch.empty((B, n), dtype=torch.int64, device="cuda")
chunk = a.cdist_chunk


def torch_rows():
    for i0 in range(0, n, chunk):
        i1 = min(i0 + chunk, n)
        rows_t[:, i0:i1].copy_(torch.cdist(pts[:, i0:i1], smp).argmin(dim=2))
    return rows_t


g_k, _ = capture(lambda: nearest_sample(pts, smp, out=rows_k))
g_t, _ = capture(torch_rows)
t = compare({"hip_kernel": g_k, "torch_cdist_argmin": g_t}, {"hip_kernel": 20, "torch_cdist_argmin": 3}, a.rounds)
pairs = B * n * S
t["hip_kernel"]["pair_evaluations"] = pairs
t["hip_kernel"]["G_pairs_per_s"] = round(pairs / t["hip_kernel"]["us_median"] * 1e-3, 1)
equal = int((rows_t == rows_k.long()).sum())
res["nearest_sample"] = {"batch": B, "points": n, "samples": S, "cdist_chunk_points": chunk, **t,
                         "torch_rows_equal_to_kernel": equal, "rows_total": B * n,
                         "torch_over_kernel": round(t["torch_cdist_argmin"]["us_median"] / t["hip_kernel"]["us_median"], 2),
                         "kernel_beats_torch": t["hip_kernel"]["us_max"] < t["torch_cdist_argmin"]["us_min"]}
del g_t, rows_t

# ---- 2. the eval forward at B x S points ----
torch.manual_seed(0)
model = PointNetSegmentation(3, 28, 768).cuda().eval()
with torch.no_grad():
    g_h, out_h = capture(lambda: model(smp))
    g_f, out_f = capture(lambda: model.forward_torch(smp))
    t = compare({"hip": g_h, "forward_torch": g_f}, {"hip": 50, "forward_torch": 10}, a.rounds)
res["eval_forward"] = {"batch": B, "points": S, "feature_dim": 768, "classes": 28, **t,
                       "max_abs_diff": float((out_h - out_f).abs().max()),
                       "torch_over_hip": round(t["forward_torch"]["us_median"] / t["hip"]["us_median"], 2),
                       "hip_beats_torch": t["hip"]["us_max"] < t["forward_torch"]["us_min"]}
del g_f, out_f

# ---- 3. the whole step: FPS, forward, rows, labels ----
buf = segment.FpsSegmentBuffers(B, n, S, pts.device)
g_step, (labels, log_probs) = capture(lambda: segment.segment_points_fps(model, S, pts, buffers=buf))
g_fps, _ = capture(lambda: farthest_point_sample(pts, S, out=buf.indices, min_dist=buf.min_dist))
g_lab, _ = capture(lambda: segment.point_labels(log_probs, buf.rows, out=buf.labels, nd_labels=buf.nd_labels))
t = compare({"step": g_step, "fps": g_fps, "forward": g_h, "rows": g_k, "labels": g_lab},
            {"step": 3, "fps": 3, "forward": 50, "rows": 20, "labels": 50}, a.rounds)
step = {"batch": B, "points": n, "samples": S, **t,
        "clouds_per_s": round(B / t["step"]["us_median"] * 1e6, 1),
        "labels_assigned": int((labels >= 0).sum()), "labels_total": B * n}
ndt_file = os.path.join(REPO, "profiles", "pipeline_labels.json")
if os.path.exists(ndt_file):
    z = json.load(open(ndt_file))
    step["ndt_net_step_from_profiles_pipeline_labels_json"] = {
        "shape": z["shape"],
        "note": "copied as recorded there (tools/bench_pipeline_labels.py, an earlier session): 1000 NDs per cloud, "
                "not 4096 samples",
        "graphed_labelled_step_us": {k: v["step_us"]["graphed_labelled"] for k, v in z["kinds"].items()},
        "pipelined_labels_nearest_step_us": {k: v["step_us"]["labels_nearest"] for k, v in z["kinds"].items()}}
res["baseline_step"] = step

os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
print(json.dumps(res))
