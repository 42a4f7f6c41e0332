#!/usr/bin/env python3
"""Time the train-time augmentation (ndnet.augment.Augment: ndnet_aug_run's
three launches) against the same transform composed from capturable torch ops,
and the graphed training step with and without it.

Shape by default: 16 x 100k points with int32 labels, synthetic L clouds.

(a) per call, at ``drop`` 0 and 0.2: device events around ``--iters``
    back-to-back calls replayed from one HIP graph, ``--rounds`` rounds after a
    warm-up, the calls rotating over ``--copies`` input and output buffers
    (more than the 256 MB last-level cache holds).  The baseline, in the same
    rounds in rotating order and replayed from a graph of its own: per-cloud
    parameters from ``torch.rand``, the affine map as ``baddbmm``, uniform
    jitter from ``torch.rand``, and with dropout a keep mask compacted per
    cloud with ``cumsum`` + ``scatter`` (points and labels) and summed to the
    new counts, straight into the output buffers (without dropout it writes
    the points only: the labels and counts are the inputs').  It is not
    bit-equal to the kernels: it only measures cost.  The kept share behind
    the byte counts is that of the timed calls themselves, recomputed from
    their steps after the timing.
(b) the graphed train step (``GraphedTrainStep`` replays) at ``loss="points"``
    on integer labels, U and L, with and without ``augment`` (drop 0.2 -- the
    ragged path on device counts -- and drop 0), replays alternated in the same
    rounds; the "without" figure is measured here, on the batch as it is and
    on one augmented batch (the NDT stage's time depends on the pose, and an
    augmented step sees a new pose on every replay).

Bytes: the algorithm reads 16 and writes 16 bytes per kept point (12 of
coordinates, 4 of label) and reads 16 per dropped one; the share of the HBM
peak (8 TB/s) is those bytes over the measured time.  Nothing is judged: every
figure is reported.  Writes JSON (default profiles/augment.json).  Measures on
the GPU only.

    python tools/bench_augment.py [--out profiles/augment.json]
"""
import argparse
import json
import math
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_PEAK_GBS = 8000.0  # HBM3E, spec

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=16)
ap.add_argument("--points", type=int, default=100_000)
ap.add_argument("--nds", type=int, default=1000)
ap.add_argument("--classes", type=int, default=28)
ap.add_argument("--feature-dim", type=int, default=768)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--iters", type=int, default=48, help="calls per variant and round")
ap.add_argument("--step-iters", type=int, default=20, help="train-step replays per variant and round")
ap.add_argument("--copies", type=int, default=12, help="input / output buffers the calls rotate over")
ap.add_argument("--kinds", default="U,L", help="clouds of the train steps")
ap.add_argument("--no-steps", action="store_true", help="skip (b), the graphed train steps")
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "augment.json"))
a = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.path.insert(0, os.path.join(REPO, "ndt-net_amd"))
from ndnet import training  # noqa: E402
from ndnet.augment import Augment  # noqa: E402
from ndnet.models.ndtnet import NDTNetSegmentation  # noqa: E402
from ndnet.synthetic import make_batch, make_labelled_batch  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("bench_augment.py measures on the GPU: none found")
dev = torch.device("cuda", 0)
B, N, K, C, R = a.batch, a.points, a.nds, a.classes, a.copies
CFG = dict(yaw=math.pi, scale=(0.95, 1.05), flip=(0.0, 0.5), shift=(0.2, 0.2, 0.05), jitter=0.01)


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
    """`iters` calls of fn(i) captured into one HIP graph, after one eager call on a side stream."""
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
    return pts, np.clip(((pts[..., 0] + 10.0) / 20.0 * (C + 1)).astype(np.int32), 0, C)


def rotate(names, r):
    return names[r % len(names):] + names[:r % len(names)]


result = {
    "shape": {"batch": B, "points": N, "nds": K, "classes": C, "feature_dim": a.feature_dim},
    "device": torch.cuda.get_device_name(0),
    "config": {k: list(v) if isinstance(v, tuple) else v for k, v in CFG.items()},
    "rounds": a.rounds, "calls_per_round": a.iters, "step_replays_per_round": a.step_iters, "buffer_copies": R,
    "units": "microseconds per call or per step replay (per-round values summarised as median / min / max); "
             "hip_* and torch_*: the calls replayed from one HIP graph each, device events around the replay",
    "baseline": "capturable torch ops on the same device: torch.rand parameters, baddbmm, torch.rand jitter, "
                "keep mask + cumsum + scatter of points and labels, sum for the counts; not bit-equal, cost only",
    "hbm_peak_gbs": HBM_PEAK_GBS,
}

# ---------------------------------------------------------------- (a) per call
host_pts, host_ids = labelled("L")
pts_in = [torch.from_numpy(host_pts).to(dev) for _ in range(R)]
ids_in = [torch.from_numpy(host_ids).to(dev) for _ in range(R)]
pts_out = [torch.empty_like(pts_in[0]) for _ in range(R)]
ids_out = [torch.empty_like(ids_in[0]) for _ in range(R)]
cnt_out = [torch.empty(B, dtype=torch.int32, device=dev) for _ in range(R)]
SQ3 = math.sqrt(3.0)


def torch_aug(drop):
    lo, hi = CFG["scale"]
    shift = torch.tensor(CFG["shift"], device=dev)
    zero, one = torch.zeros(B, device=dev), torch.ones(B, device=dev)
    last_row = torch.full((), N - 1, device=dev, dtype=torch.int64)

    def fn(i):
        p, lb = pts_in[i % R], ids_in[i % R]
        u = torch.rand(B, 8, device=dev)
        th = (2 * u[:, 0] - 1) * CFG["yaw"]
        s = lo + u[:, 1] * (hi - lo)
        fx = torch.where(u[:, 2] < CFG["flip"][0], -one, one)
        fy = torch.where(u[:, 3] < CFG["flip"][1], -one, one)
        c, z = s * torch.cos(th), s * torch.sin(th)
        M = torch.stack([fx * c, fx * -z, zero, fy * z, fy * c, zero, zero, zero, s], 1).view(B, 3, 3)
        t = (2 * u[:, 4:7] - 1) * shift
        if drop == 0.0:  # straight into the output; the labels and counts are the inputs' (no copy charged)
            out = torch.baddbmm(t[:, None, :], p, M.transpose(1, 2), out=pts_out[i % R])
            out += (torch.rand_like(out) * 2 - 1) * (CFG["jitter"] * SQ3)
            return
        out = torch.baddbmm(t[:, None, :], p, M.transpose(1, 2))
        out += (torch.rand_like(out) * 2 - 1) * (CFG["jitter"] * SQ3)
        keep = torch.rand(B, N, device=dev) >= (u[:, 7] * drop)[:, None]
        keep[:, 0] = True
        # straight into the outputs: a dropped point goes to the last row, which lies past the new
        # count whenever a point is dropped (rows from the count on may hold anything)
        dest = torch.where(keep, keep.cumsum(1) - 1, last_row)
        pts_out[i % R].scatter_(1, dest[..., None].expand(-1, -1, 3), out)
        ids_out[i % R].scatter_(1, dest, lb)
        torch.sum(keep, 1, dtype=torch.int32, out=cnt_out[i % R])
    return fn


def hip_aug(aug):
    def fn(i):
        aug(pts_in[i % R], ids_in[i % R], None, out_points=pts_out[i % R], out_labels=ids_out[i % R],
            out_counts=cnt_out[i % R])
    return fn


variants, augs, first_step = {}, {}, {}
for drop in (0.0, 0.2):
    tag = f"drop{drop:g}"
    aug = augs[tag] = Augment(drop=drop, seed=1, **CFG)
    variants[f"hip_{tag}"] = graphed(hip_aug(aug), a.iters)
    variants[f"torch_{tag}"] = graphed(torch_aug(drop), a.iters)
names = list(variants)
for nm in names:
    timed(variants[nm], 2)
for tag, aug in augs.items():
    first_step[tag] = aug.step  # the first timed draw
us = {nm: [] for nm in names}
for r in range(a.rounds):
    for nm in rotate(names, r):
        us[nm].append(timed(variants[nm], 4) / a.iters)  # four replays of a.iters calls each
res = {nm: summary(v) for nm, v in us.items()}
# the share kept by the timed calls themselves: a draw is a function of its step, so the same
# configuration run again over the timed steps keeps the same points
kept_share = {}
for tag, aug in augs.items():
    last_step = aug.step
    probe = Augment(**{k: v for k, v in aug.state_dict().items() if k != "step"})
    probe.step = first_step[tag]
    total = torch.zeros((), dtype=torch.int64, device=dev)
    for _ in range(last_step - first_step[tag]):
        total += probe(pts_in[0], ids_in[0])[2].sum()
    kept_share[tag] = float(total) / ((last_step - first_step[tag]) * B * N)
    assert probe.step == last_step == first_step[tag] + a.rounds * 4 * a.iters
per_call = {}
for drop in (0.0, 0.2):
    tag = f"drop{drop:g}"
    hip, tor = res[f"hip_{tag}"]["median"], res[f"torch_{tag}"]["median"]
    nbytes = B * N * (16 + 16 * kept_share[tag])
    per_call[tag] = {"hip_us": hip, "torch_us": tor, "speedup": round(tor / hip, 2),
                     "kept_share": round(kept_share[tag], 4), "algorithm_bytes": int(nbytes),
                     "hip_gbs": round(nbytes / hip / 1e3, 1),
                     "hip_share_of_hbm_peak": round(nbytes / hip / 1e3 / HBM_PEAK_GBS, 4)}
result["per_call"] = per_call
result["per_call_timings_us"] = res
print("per call", json.dumps(per_call), flush=True)
del variants, pts_in, ids_in, pts_out, ids_out
torch.cuda.empty_cache()

# ---------------------------------------------------------------- (b) the graphed train step
if not a.no_steps:
    result["graph_step"] = {}
    for kind in a.kinds.split(","):
        hp, hi_ = labelled(kind)
        pts, ids = torch.from_numpy(hp).to(dev), torch.from_numpy(hi_).to(dev)
        steps, variants = {}, {}
        # the NDT stage's time depends on the cloud's pose: a plain step on one augmented batch
        # (draw 0 of the drop-0 augmentation) separates that from the augmentation's own launches
        posed = Augment(drop=0.0, seed=1, **CFG)(pts, ids)[0]
        for name, aug in (("plain", None), ("plain_on_augmented", None),
                          ("augment_drop0", Augment(drop=0.0, seed=1, **CFG)),
                          ("augment_drop0.2", Augment(drop=0.2, seed=1, **CFG))):
            torch.manual_seed(0)
            tr = training.Trainer(NDTNetSegmentation(3, C, a.feature_dim), 1e-3, K, C, dev, ddp=False, graphs=True,
                                  loss="points", augment=aug)
            s_p, s_g = tr.graph_inputs(pts.shape, ids.shape)
            s_p.copy_(posed if name == "plain_on_augmented" else pts)
            s_g.copy_(ids)
            g = tr._graph_for(pts.shape, ids.shape)
            steps[name] = tr, g
            variants[name] = (lambda i, g=g: g.graph.replay())
        names = list(variants)
        for nm in names:
            timed(variants[nm], max(2, a.step_iters // 4))
        us = {nm: [] for nm in names}
        for r in range(a.rounds):
            for nm in rotate(names, r):
                us[nm].append(timed(variants[nm], a.step_iters))
        res = {nm: summary(v) for nm, v in us.items()}
        med = {nm: res[nm]["median"] for nm in names}
        result["graph_step"][kind] = {
            "plain_us": med["plain"], "plain_on_augmented_us": med["plain_on_augmented"],
            "augment_drop0_us": med["augment_drop0"],
            "augment_drop0.2_us": med["augment_drop0.2"],
            "added_drop0_us": round(med["augment_drop0"] - med["plain"], 3),
            "added_drop0.2_us": round(med["augment_drop0.2"] - med["plain"], 3),
            "added_drop0_over_plain_on_augmented_us": round(med["augment_drop0"] - med["plain_on_augmented"], 3),
            "loss": {nm: steps[nm][1].loss.item() for nm in steps}, "timings_us": res}
        print(kind, json.dumps({k: v for k, v in result["graph_step"][kind].items() if k != "timings_us"}), flush=True)
        del steps, variants
        torch.cuda.empty_cache()

os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
print("wrote", a.out)
