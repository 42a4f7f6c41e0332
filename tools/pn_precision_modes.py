#!/usr/bin/env python3
"""Time and check the precision modes of the eval forward against each other.

One process, F = 768, C = 28, 16 x 1000 NDs by default, every variant warmed,
then the variants alternate round-robin (one round = every variant once, the
order rotated by one each round), so clock and neighbour drift and the place
in the round hit them alike.  Per variant and round:

  * the whole forward launched from Python: device events around
    ``--forwards`` forwards (at this shape the launches, not the kernels, set
    this time);
  * the whole forward replayed from a HIP graph captured in the variant's
    mode: device events around ``--forwards`` replays (the GPU's time);
  * each chain alone: ``--launches`` launches back to back between two device
    events (the per-launch duration a kernel trace reports);
  * each chain inside a forward: ``pointnet_hip.chain_timing`` events around
    every launch (adds the launch's dispatch latency).

Variants are the modes of ``--modes`` (x6, x3, bf16, fp32) run through
``model.precision``.  ``--parent-lib PATH`` adds two more, ``x6@parent`` and
``x6@parent-again``: the same x6 forward through another build of the library
(the parent commit's) loaded beside this one -- the gap between the two is the
spread of a repeated measurement of one build, the bar every other difference
has to clear.  ``--lib PATH`` runs everything on that library instead
(NDNET_AMD_LIB; a build without the reduced modes needs ``--modes x6``).

Also records max |log-prob - float64| and the argmax agreement per variant,
and writes everything as JSON under profiles/.

    python tools/pn_precision_modes.py [--parent-lib PATH] [--out profiles/pn_precision_modes.json]
"""
import argparse
import contextlib
import copy
import ctypes
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ap = argparse.ArgumentParser()
ap.add_argument("--lib", help="library to run instead of this tree's (forwarded to NDNET_AMD_LIB)")
ap.add_argument("--parent-lib", help="a second build of the library, alternated in-process in x6 mode")
ap.add_argument("--modes", default="x6,x3,bf16")
ap.add_argument("--batch", type=int, default=16)
ap.add_argument("--nds", type=int, default=1000)
ap.add_argument("--feature-dim", type=int, default=768)
ap.add_argument("--classes", type=int, default=28)
ap.add_argument("--rounds", type=int, default=10)
ap.add_argument("--forwards", type=int, default=100, help="forwards per variant and round (rounds x forwards >= 200)")
ap.add_argument("--launches", type=int, default=50, help="back-to-back launches per chain, variant and round")
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pn_precision_modes.json"))
a = ap.parse_args()
if a.lib:
    os.environ["NDNET_AMD_LIB"] = os.path.abspath(a.lib)

import torch  # noqa: E402

sys.path.insert(0, os.path.join(REPO, "ndt-net_amd"))
from ndnet import _lib  # noqa: E402
from ndnet.models import pointnet_hip as ph  # noqa: E402
from ndnet.models.ndtnet import NDTNetSegmentation  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("pn_precision_modes.py measures on the GPU: none found")
dev = torch.device("cuda", 0)
this_lib = _lib.lib()
parent = None
if a.parent_lib:
    parent = ctypes.CDLL(os.path.abspath(a.parent_lib))
    for name, (res, args) in {**_lib.EXPORTS, **_lib.POINTNET_EXPORTS, **_lib.TRAIN_EXPORTS}.items():
        fn = getattr(parent, name)
        fn.restype, fn.argtypes = res, args


@contextlib.contextmanager
def library(handle):
    """Every ndnet call inside goes to `handle` (both builds read the same argument blocks)."""
    _lib._lib = handle
    try:
        yield
    finally:
        _lib._lib = this_lib


modes = [s for s in a.modes.split(",") if s]
for s in modes:
    if s not in ph.MODES:
        sys.exit(f"unknown mode {s!r}")
variants = [(s, s, this_lib) for s in modes]
if parent is not None:
    variants += [("x6@parent", "x6", parent), ("x6@parent-again", "x6", parent)]

torch.manual_seed(0)
m = NDTNetSegmentation(3, a.classes, a.feature_dim).to(dev).eval()
B, N = a.batch, a.nds
x = torch.randn(B, N, 12, device=dev)
p, c = x[..., :3], x[..., 3:]
blk = x.as_strided((B, N, 12), (N * 12, 12, 1))
out_d = torch.empty((B, N, a.classes + 1), device=dev)


def event():
    return torch.cuda.Event(enable_timing=True)


def forwards(k):
    e0, e1 = event(), event()
    e0.record()
    for _ in range(k):
        m(p, c)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / k  # us


def chains_alone(ws):
    us = []
    for i in range(4):
        o = out_d if i == 3 else None
        ws.chain(i, blk, out=o)
        e0, e1 = event(), event()
        e0.record()
        for _ in range(a.launches):
            ws.chain(i, blk, out=o)
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3 / a.launches)
    return us


def chains_in_forward(k):
    ph.chain_timing = []
    for _ in range(k):
        m(p, c)
    torch.cuda.synchronize()
    us = [0.0] * 4
    for i, e0, e1 in ph.chain_timing:
        us[i] += e0.elapsed_time(e1) * 1e3 / k
    ph.chain_timing = None
    return us


def replays(g, k):
    e0, e1 = event(), event()
    e0.record()
    for _ in range(k):
        g.replay()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / k  # us


res = {name: {"forward_us": [], "forward_graph_us": [], "chains_alone_us": [], "chains_in_forward_us": []}
       for name, _, _ in variants}
graphs = {}
with torch.no_grad():
    ref64 = copy.deepcopy(m).double().forward_torch(p.double(), c.double())
    for name, mode, handle in variants:  # warm every variant; its error against float64
        m.precision = mode
        with library(handle):
            for _ in range(5):
                out = m(p, c)
            torch.cuda.synchronize()
        res[name]["max_err_vs_float64"] = (out.double() - ref64).abs().max().item()
        res[name]["argmax_agreement"] = (out.argmax(-1) == ref64.argmax(-1)).double().mean().item()
        if name == variants[0][0]:
            first = out.clone()
        res[name]["bit_equal_to_first_variant"] = bool(torch.equal(out, first))
        with library(handle):  # the forward as a graph: it keeps the mode (and the library) it was captured with
            graphs[name] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[name]):
                gout = m(p, c)
            graphs[name].replay()
            torch.cuda.synchronize()
        res[name]["graph_bit_equal_to_eager"] = bool(torch.equal(gout, out))
    ws = ph._folded(m)["ws"][(B, N, dev, 0)]
    for r in range(a.rounds):
        for name, mode, handle in variants[r % len(variants):] + variants[:r % len(variants)]:
            m.precision = mode
            with library(handle):
                forwards(2)
                res[name]["forward_us"].append(forwards(a.forwards))
                replays(graphs[name], 2)
                res[name]["forward_graph_us"].append(replays(graphs[name], a.forwards))
                res[name]["chains_alone_us"].append(chains_alone(ws))
                res[name]["chains_in_forward_us"].append(chains_in_forward(5))
        print(f"round {r + 1}/{a.rounds}", flush=True)
m.precision = None


def summary(v):
    return {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}


report = {"shape": {"batch": B, "nds": N, "feature_dim": a.feature_dim, "classes": a.classes},
          "device": torch.cuda.get_device_name(dev), "library": os.path.relpath(_lib.LIB_PATH, REPO),
          "parent_library": os.path.relpath(a.parent_lib, REPO) if a.parent_lib else None, "rounds": a.rounds, "forwards_per_round": a.forwards,
          "launches_per_round": a.launches, "units": "microseconds; per-round values summarised as median / min / max",
          "variants": {}}
for name, _, _ in variants:
    r = res[name]
    sums = [sum(c4) for c4 in r["chains_alone_us"]]
    report["variants"][name] = {
        "forward_us": summary(r["forward_us"]),
        "forward_graph_us": summary(r["forward_graph_us"]),
        "chain_sum_alone_us": summary(sums),
        "chains_alone_us": [summary([c4[i] for c4 in r["chains_alone_us"]]) for i in range(4)],
        "chains_in_forward_us": [summary([c4[i] for c4 in r["chains_in_forward_us"]]) for i in range(4)],
        "max_err_vs_float64": r["max_err_vs_float64"], "argmax_agreement": r["argmax_agreement"],
        "bit_equal_to_first_variant": r["bit_equal_to_first_variant"],
        "graph_bit_equal_to_eager": r["graph_bit_equal_to_eager"],
        "per_round": {"forward_us": [round(v, 2) for v in r["forward_us"]],
                      "forward_graph_us": [round(v, 2) for v in r["forward_graph_us"]], "chain_sum_alone_us": [round(v, 2) for v in sums]},
    }
if parent is not None:
    pa, pb = report["variants"]["x6@parent"], report["variants"]["x6@parent-again"]
    report["parent_spread_us"] = {
        "what": "|median(x6@parent) - median(x6@parent-again)|: one build measured twice in the same rounds",
        "chain_sum_alone": round(abs(pa["chain_sum_alone_us"]["median"] - pb["chain_sum_alone_us"]["median"]), 2),
        "forward": round(abs(pa["forward_us"]["median"] - pb["forward_us"]["median"]), 2),
        "forward_graph": round(abs(pa["forward_graph_us"]["median"] - pb["forward_graph_us"]["median"]), 2)}
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(report, f, indent=1)
    f.write("\n")
for name, v in report["variants"].items():
    alone = " ".join("%6.1f" % c4["median"] for c4 in v["chains_alone_us"])
    print(f"{name:16s} forward {v['forward_us']['median']:8.1f} us  graphed {v['forward_graph_us']['median']:8.1f} us  chains alone {alone} "
          f"sum {v['chain_sum_alone_us']['median']:7.1f} us  err {v['max_err_vs_float64']:.2e}  "
          f"argmax {100 * v['argmax_agreement']:.2f}%")
if parent is not None:
    print("parent spread:", report["parent_spread_us"])
print("wrote", a.out)
