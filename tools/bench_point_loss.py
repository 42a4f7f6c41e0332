#!/usr/bin/env python3
"""Time the point-level loss (ndnet.segment.row_histogram, the nll_hist
kernels, Trainer(loss="points")) against the same computation composed from
torch ops, and the graphed training step with and without it.

Shape by default: 16 x 100k points -> 1000 NDs, 29 label columns, synthetic U
and L clouds (ndnet.synthetic).  The L labels are the generator's (ground 0,
object clusters 1 + cluster % classes: one ND of a cluster holds ~1.7k points of
one class, the heavy counters); the U labels are slabs along x.  Per kind, after
one labelled ``NdtPlan.run`` and ``point_rows(fill="nearest")``:

(a) ``ndnet_seg_row_hist`` alone, and ``ndnet_tr_nll_hist`` + ``_bwd`` +
    ``ndnet_tr_hist_match_cm`` together: device events around ``--iters``
    back-to-back calls per round replayed from one HIP graph (the time on the
    GPU), ``--rounds`` rounds after a warm-up, the calls rotating over
    ``--copies`` identical input buffers (more than the 256 MB last-level cache
    holds for the histogram's rows and labels).  Each against the torch
    composition on the same device in the same rounds, order rotated:
    ``index_add_`` of ones on a flat int32 table (out-of-range points sent to
    a spare last cell), then the masked product ``where(h != 0, h * logp, 0)``,
    its sum over ``W``, the gradient ``-h / W`` and the matched count by
    ``argmax`` + ``gather``.  The two tables must be equal.
(b) the graphed train step (``GraphedTrainStep`` replays) with
    ``loss="points"`` and ``point_fill`` none / nearest on integer labels,
    against the default ``loss="nds"`` on one-hot labels, same shape, replays
    alternated in the same rounds.

The one condition: the row-histogram kernel is not slower than its torch
composition (``"hist_hip_not_slower"``), for U and for L.  Every other figure
is reported, not judged.  Writes JSON (default profiles/point_loss.json).
Measures on the GPU only.

    python tools/bench_point_loss.py [--out profiles/point_loss.json]
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
ap.add_argument("--nds", type=int, default=1000)
ap.add_argument("--classes", type=int, default=28)
ap.add_argument("--feature-dim", type=int, default=768)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--iters", type=int, default=40, help="kernel calls per variant and round")
ap.add_argument("--baseline-iters", type=int, default=10, help="torch compositions per variant and round")
ap.add_argument("--step-iters", type=int, default=20, help="train-step replays per variant and round")
ap.add_argument("--copies", type=int, default=24, help="identical input buffers the calls rotate over")
ap.add_argument("--kinds", default="U,L")
ap.add_argument("--no-steps", action="store_true", help="skip (b), the graphed train steps")
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "point_loss.json"))
a = ap.parse_args()
if a.rounds * a.iters < 200:
    sys.exit("at least 200 kernel calls per variant (rounds x iters)")

import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.path.insert(0, os.path.join(REPO, "ndt-net_amd"))
from ndnet import _lib, segment, training  # noqa: E402
from ndnet.models.ndtnet import NDTNetSegmentation  # noqa: E402
from ndnet.preprocessing.ndtnet_preprocessing import NdtPlan  # noqa: E402
from ndnet.synthetic import make_batch, make_labelled_batch  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("bench_point_loss.py measures on the GPU: none found")
dev = torch.device("cuda", 0)
B, N, K, R = a.batch, a.points, a.nds, a.copies
C = a.classes
COLS = C + 1
L = _lib.lib()


def summary(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3),
            "per_round": [round(x, 3) for x in v]}


def timed(fn, iters):
    """Microseconds per call of fn(i), device events around `iters` calls."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(iters):
        fn(i)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def graphed(fn, iters):
    """`iters` calls of fn(i) captured into one HIP graph: a replay runs them back to back
    without the host's per-call launch work."""
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
    return lambda i: g.replay()


def labelled(kind):
    """(points [B, N, 3] float32, ids [B, N] int32) on the host."""
    if kind == "L":
        pts, onehot = make_labelled_batch(B, N, C)
        return pts, onehot.argmax(-1).astype(np.int32)
    pts = make_batch(kind, B, N)
    return pts, np.clip(((pts[..., 0] + 10.0) / 20.0 * COLS).astype(np.int32), 0, C)


result = {
    "shape": {"batch": B, "points": N, "nds": K, "classes": C, "columns": COLS, "feature_dim": a.feature_dim},
    "device": torch.cuda.get_device_name(0),
    "rounds": a.rounds, "kernel_calls_per_round": a.iters, "baseline_calls_per_round": a.baseline_iters,
    "step_replays_per_round": a.step_iters, "input_copies": R,
    "units": "microseconds per call (per-round values summarised as median / min / max); hip_*: the calls replayed "
             "from one HIP graph; torch_*: the composition issued from Python, device events around the calls; "
             "step_*: GraphedTrainStep replays",
    "baseline": "torch ops on the same device: index_add_ of ones on a flat int32 table with a spare cell for the "
                "points left out; where(h != 0, h * logp, 0).sum() / W, -h / W, argmax + gather for the matched count",
    "kinds": {},
}
all_ok = True
for kind in a.kinds.split(","):
    host_pts, host_ids = labelled(kind)
    pts = torch.from_numpy(host_pts).to(dev)
    ids = torch.from_numpy(host_ids).to(dev)
    plan = NdtPlan(B, N, K, C, device=dev)
    block = torch.empty((B, K, 12), dtype=torch.float32, device=dev)
    cls = torch.empty((B, K, COLS), dtype=torch.float32, device=dev)
    plan.run(pts, ids, block, cls)
    rows0 = plan.point_rows(pts, block, fill="nearest")
    torch.cuda.synchronize()
    assert all(s.rc == 0 for s in plan.host_stats())
    rows = [rows0.clone() for _ in range(R)]
    labels = [ids.clone() for _ in range(R)]
    tables = [torch.empty((B, K, COLS), dtype=torch.int32, device=dev) for _ in range(R)]
    ones = torch.ones(B * N, dtype=torch.int32, device=dev)
    cloud = (torch.arange(B, device=dev, dtype=torch.int64) * K)[:, None]

    def hip_hist(i):
        segment.row_histogram(rows[i % R], labels[i % R], K, COLS, out=tables[i % R])

    def torch_hist(i):
        r, lb = rows[i % R].long(), labels[i % R].long()
        ok = (r >= 0) & (r < K) & (lb >= 0) & (lb < COLS)
        flat = torch.where(ok, (cloud + r) * COLS + lb, torch.full_like(r, B * K * COLS))
        t = torch.zeros(B * K * COLS + 1, dtype=torch.int32, device=dev)
        t.index_add_(0, flat.view(-1), ones)
        return t[:-1].view(B, K, COLS)

    hip_hist(0)
    hist = tables[0].clone()
    hist_equal = bool(torch.equal(hist, torch_hist(0)))
    heaviest = int(hist.max())

    logp_cm = torch.log_softmax(torch.randn(B, COLS, K, device=dev), 1)
    pred = logp_cm.transpose(1, 2)
    nparts = (B * K + 63) // 64
    part = torch.empty(nparts, dtype=torch.float64, device=dev)
    wsum = torch.empty(1, dtype=torch.int64, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    dloss = torch.ones(1, dtype=torch.float32, device=dev)
    dlogp = torch.empty_like(logp_cm)
    ctr = torch.zeros(3, dtype=torch.int64, device=dev)
    acc = torch.empty((), dtype=torch.float32, device=dev)

    def hip_loss(i):
        st = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(L.ndnet_tr_nll_hist(logp_cm.data_ptr(), hist.data_ptr(), part.data_ptr(), wsum.data_ptr(),
                                       loss.data_ptr(), B, COLS, K, st), "ndnet_tr_nll_hist")
        _lib.check(L.ndnet_tr_nll_hist_bwd(hist.data_ptr(), wsum.data_ptr(), dloss.data_ptr(), dlogp.data_ptr(), B,
                                           COLS, K, st), "ndnet_tr_nll_hist_bwd")
        ctr.zero_()
        _lib.check(L.ndnet_tr_hist_match_cm(logp_cm.data_ptr(), hist.data_ptr(), B, COLS, K, ctr.data_ptr(),
                                            acc.data_ptr(), st), "ndnet_tr_hist_match_cm")

    def torch_loss(i):
        h = hist.float()
        w = hist.sum(dtype=torch.int64).clamp(min=1).float()
        ls = -torch.where(hist != 0, h * pred, torch.zeros((), device=dev)).sum() / w
        grad = -(h / w)
        matched = hist.gather(-1, pred.argmax(-1, keepdim=True)).sum(dtype=torch.int64)
        return ls, grad, matched.float() / w

    hip_loss(0)
    t_ls, t_grad, t_acc = torch_loss(0)
    torch.cuda.synchronize()
    loss_rel = abs(loss.item() - t_ls.item()) / max(abs(t_ls.item()), 1e-30)
    grad_err = (dlogp.transpose(1, 2) - t_grad).abs().max().item()

    variants = {"hip_hist": (graphed(hip_hist, a.iters), 1, a.iters),
                "hip_hist_from_python": (hip_hist, a.iters, 1),
                "torch_hist": (torch_hist, a.baseline_iters, 1),
                "hip_loss": (graphed(hip_loss, a.iters), 1, a.iters),
                "torch_loss": (torch_loss, a.baseline_iters, 1)}
    steps = {}
    if not a.no_steps:
        onehot = torch.nn.functional.one_hot(ids.long(), COLS).float()
        for name, kw, gt in (("step_nds_onehot", {}, onehot),
                             ("step_points_none", {"loss": "points", "point_fill": "none"}, ids),
                             ("step_points_nearest", {"loss": "points", "point_fill": "nearest"}, ids)):
            torch.manual_seed(0)
            tr = training.Trainer(NDTNetSegmentation(3, C, a.feature_dim), 1e-3, K, C, dev, ddp=False, graphs=True,
                                  **kw)
            s_p, s_g = tr.graph_inputs(pts.shape, gt.shape)
            s_p.copy_(pts)
            s_g.copy_(gt)
            g = tr._graph_for(pts.shape, gt.shape)
            steps[name] = tr, g  # (the trainer keeps the graph's tensors alive)
            variants[name] = ((lambda i, g=g: g.graph.replay()), a.step_iters, 1)
        del onehot
    names = list(variants)
    for fn, it, per in variants.values():  # warm-up
        timed(fn, max(2, it // 4))
    us = {nm: [] for nm in names}
    for r in range(a.rounds):
        for nm in names[r % len(names):] + names[:r % len(names)]:  # the order rotated by one each round
            fn, it, per = variants[nm]
            us[nm].append(timed(fn, it) / per)
    res = {nm: summary(v) for nm, v in us.items()}
    med = {nm: res[nm]["median"] for nm in names}
    ok = med["hip_hist"] <= med["torch_hist"]
    all_ok &= ok
    out = {
        "counted_points": int(hist.sum()), "heaviest_counter": heaviest, "nonzero_counters": int((hist != 0).sum()),
        "hist_equals_torch": hist_equal,
        "hist": {"hip_us": med["hip_hist"], "torch_us": med["torch_hist"],
                 "speedup": round(med["torch_hist"] / med["hip_hist"], 2), "hip_not_slower": ok,
                 "hip_from_python_us": med["hip_hist_from_python"],
                 "atomics_per_us": round(int(hist.sum()) / med["hip_hist"], 1)},
        "loss_bwd_match": {"hip_us": med["hip_loss"], "torch_us": med["torch_loss"],
                           "speedup": round(med["torch_loss"] / med["hip_loss"], 2),
                           "loss_rel_diff_to_torch": loss_rel, "grad_max_abs_diff_to_torch": grad_err,
                           "acc_hip": acc.item(), "acc_torch": t_acc.item()},
        "timings_us": res,
    }
    if steps:
        out["graph_step"] = {
            "nds_onehot_us": med["step_nds_onehot"], "points_none_us": med["step_points_none"],
            "points_nearest_us": med["step_points_nearest"],
            "added_none_us": round(med["step_points_none"] - med["step_nds_onehot"], 3),
            "added_nearest_us": round(med["step_points_nearest"] - med["step_nds_onehot"], 3),
            "loss": {nm: steps[nm][1].loss.item() for nm in steps}, "acc": {nm: steps[nm][1].acc.item() for nm in steps}}
    result["kinds"][kind] = out
    print(kind, json.dumps({k: v for k, v in out.items() if k != "timings_us"}), flush=True)
    del steps, variants, rows, labels, tables
    torch.cuda.empty_cache()
result["hist_hip_not_slower"] = bool(all_ok)
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
print("wrote", a.out, "hist_hip_not_slower =", all_ok)
