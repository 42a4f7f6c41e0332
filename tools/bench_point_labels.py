#!/usr/bin/env python3
"""Time the per-point label path (ndnet.segment) against the same computation
composed from torch ops.

Shape C2 by default: 16 x 100k points -> 1000 NDs, synthetic U and L clouds
(ndnet.synthetic).  Per cloud kind, after one ``ndt_preprocessing`` run:

* ``NdtPlan.point_rows`` with fill none and nearest and
  ``segment.point_labels``, each alone: device events around ``--iters``
  back-to-back launches per round (``--rounds`` rounds, >= 200 launches in all,
  after a warm-up), replayed from one HIP graph -- the time on the GPU; a call
  from Python costs more host time than these kernels run, so the same
  launches issued from Python are recorded beside them (``*_from_python``).  The launches rotate over ``--copies`` identical input
  buffers (and as many outputs), more than the 256 MB last-level cache holds,
  so the streams come from HBM.  Achieved bytes/s come from the algorithmic
  bytes: 16 n per cloud for the rows (12 read, 4 written), 8 n + 4 k cols + 4 k
  for the labels.
* the baseline, written here: the same rows from torch ops on the same device
  -- float64 floor-divide voxel keys, ``searchsorted`` on the plan's ``vox``,
  the row table from a cumsum of ``alive``, gathers, and for the fill a chunked
  ``cdist`` / ``argmin`` over the points without a row -- alternated with the
  HIP launches in the same rounds.  (The synthetic clouds meet no worker
  cut-off, so the baseline leaves that rule out.)  Its none rows must equal
  the HIP rows exactly; for nearest the differing points are counted (``cdist``
  rounds differently from the kernel's fp32 formula).
* the ``GraphedSegmentation`` step with and without ``point_labels="nearest"``,
  replays alternated in the same rounds; the difference is reported, not
  bounded.

The one condition: in each of the four cells (U / L x none / nearest) the HIP
path is not slower than the torch composition (``"hip_not_slower"``).  Writes
JSON (default profiles/point_labels.json).  Measures on the GPU only.

    python tools/bench_point_labels.py [--out profiles/point_labels.json]
"""
import argparse
import ctypes
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
ap.add_argument("--iters", type=int, default=40, help="launches per variant and round")
ap.add_argument("--baseline-iters", type=int, default=4, help="torch compositions per variant and round")
ap.add_argument("--copies", type=int, default=16, help="identical input buffers the launches rotate over")
ap.add_argument("--kinds", default="U,L")
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "point_labels.json"))
a = ap.parse_args()
if a.rounds * a.iters < 200:
    sys.exit("at least 200 launches per variant (rounds x iters)")

import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.path.insert(0, os.path.join(REPO, "ndt-net_amd"))
from ndnet import _lib, pipeline, segment  # noqa: E402
from ndnet.models.ndtnet import NDTNetSegmentation  # noqa: E402
from ndnet.preprocessing.ndtnet_preprocessing import NdtPlan  # noqa: E402
from ndnet.synthetic import make_batch  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("bench_point_labels.py measures on the GPU: none found")
dev = torch.device("cuda", 0)
B, N, K, R = a.batch, a.points, a.nds, a.copies
COLS = a.classes + 1


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
    without the host's per-call launch work.  Returns (callable, calls per replay)."""
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


def plan_state(plan, stats):
    """vox (padded with a key above every voxel) and alive of every cloud, on the device."""
    nd_max = max(int(s.num_nds) for s in stats)
    vox = np.full((B, nd_max), 1 << 40, np.int64)
    alive = np.zeros((B, nd_max), bool)
    for b, s in enumerate(stats):
        nd = int(s.num_nds)
        v, al, it = np.zeros(nd, np.uint32), np.zeros(nd, np.uint8), ctypes.c_uint32(0)
        p = lambda x: x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
        rc = _lib.lib().ndnet_ndt_debug_dump(plan.handle, b, None, None, None, None, p(v), None, None, None, None,
                                             None, ctypes.byref(it), p(al))
        _lib.check(rc, "ndnet_ndt_debug_dump")
        vox[b, :nd], alive[b, :nd] = v, al != 0
    return torch.from_numpy(vox).to(dev), torch.from_numpy(alive).to(dev)


def torch_rows(pts, vox, alive, off, vs, ln, nout, nout_h, block, fill):
    """The torch composition: [B, N] int32 rows."""
    n8 = 8 * (N // 8)
    v = torch.floor((pts.double() - off[:, None, :]) / vs[:, None, None]).long()
    ok = ((v >= 0) & (v < ln[:, None, :])).all(2)
    ok[:, n8:] = False
    key = (v[..., 2] * ln[:, None, 1] + v[..., 1]) * ln[:, None, 0] + v[..., 0]
    key = torch.where(ok, key, torch.full_like(key, -1))
    d = torch.searchsorted(vox, key).clamp_(max=vox.shape[1] - 1)
    hit = ok & (torch.gather(vox, 1, d) == key)
    rank = torch.cumsum(alive, 1) - 1
    table = torch.where(alive & (rank < nout[:, None]), rank, torch.full_like(rank, -1))
    rows = torch.where(hit, torch.gather(table, 1, d), torch.full_like(d, -1)).int()
    if fill == "nearest":
        finite = torch.isfinite(pts).all(2)
        for b, nb in enumerate(nout_h):
            if nb == 0:
                continue
            idx = torch.nonzero((rows[b] < 0) & finite[b]).squeeze(1)
            means = block[b, :nb, :3]
            for s in range(0, idx.numel(), 16384):
                part = idx[s:s + 16384]
                rows[b, part] = torch.cdist(pts[b, part], means).argmin(1).int()
    return rows


result = {
    "shape": {"batch": B, "points": N, "nds": K, "classes": a.classes, "feature_dim": a.feature_dim},
    "device": torch.cuda.get_device_name(0),
    "rounds": a.rounds, "launches_per_round": a.iters, "baseline_calls_per_round": a.baseline_iters,
    "input_copies": R,
    "units": "microseconds per call (per-round values summarised as median / min / max); GB/s = algorithmic "
             "bytes over the median; hip_* and labels: the launches replayed from one HIP graph, *_from_python: "
             "issued call by call",
    "baseline": "torch ops on the same device: float64 floor-divide keys, searchsorted on vox, cumsum of alive, "
                "gathers; fill: chunked cdist / argmin over the points without a row",
    "kinds": {},
}
rows_bytes = 16 * N * B
labels_bytes = 8 * N * B + 4 * B * K * COLS + 4 * B * K
torch.manual_seed(0)
model = NDTNetSegmentation(3, a.classes, a.feature_dim).to(dev).eval()
all_ok = True
for kind in a.kinds.split(","):
    host = make_batch(kind, B, N)
    copies = [torch.from_numpy(host).to(dev) for _ in range(R)]
    outs = [torch.empty((B, N), dtype=torch.int32, device=dev) for _ in range(R)]
    pts = copies[0]
    plan = NdtPlan(B, N, K, -1, device=dev)
    block = torch.empty((B, K, 12), dtype=torch.float32, device=dev)
    plan.run(pts, None, block, None)
    torch.cuda.synchronize()
    stats = plan.host_stats()
    assert all(s.rc == 0 for s in stats), [s.rc for s in stats]
    vox, alive = plan_state(plan, stats)
    off = torch.tensor([list(s.offset) for s in stats], dtype=torch.float64, device=dev)
    vs = torch.tensor([s.voxel_size for s in stats], dtype=torch.float64, device=dev)
    ln = torch.tensor([list(s.len) for s in stats], dtype=torch.int64, device=dev)
    nout_h = [min(int(s.num_out), K) for s in stats]
    nout = torch.tensor(nout_h, dtype=torch.int64, device=dev)
    scores = torch.randn(B, K, COLS, device=dev)
    nd_labels = torch.empty((B, K), dtype=torch.int32, device=dev)

    hip = {f: (lambda i, f=f: plan.point_rows(copies[i % R], block, fill=f, out=outs[i % R]))
           for f in ("none", "nearest")}
    base = {f: (lambda i, f=f: torch_rows(copies[i % R], vox, alive, off, vs, ln, nout, nout_h, block, f))
            for f in ("none", "nearest")}
    rows_near = [plan.point_rows(copies[i], block, fill="nearest") for i in range(R)]
    lab_out = [torch.empty((B, N), dtype=torch.int32, device=dev) for _ in range(R)]
    labels = lambda i: segment.point_labels(scores, rows_near[i % R], out=lab_out[i % R], nd_labels=nd_labels)  # noqa: E731

    # agreement of the two computations
    h_none, h_near = hip["none"](0).clone(), hip["nearest"](1).clone()
    t_none, t_near = base["none"](0), base["nearest"](1)
    none_equal = bool(torch.equal(h_none, t_none))
    near_diff = int((h_near != t_near).sum())
    unassigned = int((h_none < 0).sum())

    graphs = {"plain": pipeline.GraphedSegmentation(model, K, B, N, device=dev),
              "point_labels": pipeline.GraphedSegmentation(model, K, B, N, device=dev, point_labels="nearest")}
    for g in graphs.values():
        g.points.copy_(pts)

    # (calls per timed window, launches per call)
    variants = {"hip_none": (graphed(hip["none"], a.iters), 1, a.iters),
                "hip_nearest": (graphed(hip["nearest"], a.iters), 1, a.iters),
                "hip_none_from_python": (hip["none"], a.iters, 1),
                "hip_nearest_from_python": (hip["nearest"], a.iters, 1),
                "torch_none": (base["none"], a.baseline_iters, 1),
                "torch_nearest": (base["nearest"], a.baseline_iters, 1),
                "labels": (graphed(labels, a.iters), 1, a.iters),
                "labels_from_python": (labels, a.iters, 1),
                "graph_plain": (lambda i: graphs["plain"].replay(), a.iters, 1),
                "graph_point_labels": (lambda i: graphs["point_labels"].replay(), a.iters, 1)}
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
    cells = {}
    for f in ("none", "nearest"):
        ok = med[f"hip_{f}"] <= med[f"torch_{f}"]
        all_ok &= ok
        cells[f] = {"hip_us": med[f"hip_{f}"], "torch_us": med[f"torch_{f}"],
                    "speedup": round(med[f"torch_{f}"] / med[f"hip_{f}"], 2), "hip_not_slower": ok,
                    "hip_GBps": round(rows_bytes / med[f"hip_{f}"] / 1e3, 1),
                    "hip_from_python_us": med[f"hip_{f}_from_python"]}
    result["kinds"][kind] = {
        "points_without_a_row": unassigned, "points_without_a_row_share": round(unassigned / (B * N), 4),
        "none_rows_equal_torch": none_equal, "nearest_rows_differing_from_torch": near_diff,
        "cells": cells,
        "labels": {"us": med["labels"], "GBps": round(labels_bytes / med["labels"] / 1e3, 1),
                   "from_python_us": med["labels_from_python"]},
        "graph_step": {"plain_us": med["graph_plain"], "with_point_labels_us": med["graph_point_labels"],
                       "added_us": round(med["graph_point_labels"] - med["graph_plain"], 3)},
        "algorithmic_bytes": {"rows": rows_bytes, "labels": labels_bytes},
        "timings_us": res,
    }
    print(kind, json.dumps({"cells": cells, "labels": result["kinds"][kind]["labels"],
                            "graph_step": result["kinds"][kind]["graph_step"], "none_equal": none_equal,
                            "nearest_diff": near_diff, "unassigned": unassigned}), flush=True)
    del graphs, copies, outs, rows_near, lab_out
    torch.cuda.empty_cache()
result["hip_not_slower_in_every_cell"] = bool(all_ok)
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
print("wrote", a.out, "hip_not_slower_in_every_cell =", all_ok)
