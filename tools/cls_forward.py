#!/usr/bin/env python3
"""Time and check the eval forward of NDTNetClassification on the HIP path
against the torch composition it replaces.

One process, NDTNetClassification(3, 512, 768) and (3, 40, 768) at 16 x 1000
NDs by default.  ``model(p, c)`` (chains A-C, the per-cloud steps, the head's
two FC launches and ndnet_pn_cls_head_run) is compared with
``model.forward_torch(p, c)`` -- what this call ran before the HIP path
existed, so the baseline.  Every variant is warmed, then the variants
alternate round-robin (one round = every variant once, the order rotated by
one each round), so clock and neighbour drift and the place in the round hit
them alike.  Per variant and round, device events around ``--forwards``
forwards launched from Python (eager) and around ``--forwards`` replays of the
forward captured into a HIP graph.

Also records ndnet_pn_cls_head_run alone (K = 256, 16 clouds, C = 512 and
1000: ``--launches`` launches back to back between two device events, per
round), and the max log-probability error against a float64 forward of both
paths.  Writes everything as JSON under profiles/.  Measures on the GPU only.

    python tools/cls_forward.py [--out profiles/cls_forward.json]
"""
import argparse
import copy
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=16)
ap.add_argument("--nds", type=int, default=1000)
ap.add_argument("--feature-dim", type=int, default=768)
ap.add_argument("--classes", default="512,40")
ap.add_argument("--head-classes", default="512,1000", help="class counts of the head kernel timed alone")
ap.add_argument("--rounds", type=int, default=10)
ap.add_argument("--forwards", type=int, default=50, help="forwards per variant and round")
ap.add_argument("--launches", type=int, default=200, help="back-to-back head launches per round")
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "cls_forward.json"))
a = ap.parse_args()
if a.rounds < 10:
    sys.exit("at least 10 rounds")

import torch  # noqa: E402

sys.path.insert(0, os.path.join(REPO, "ndt-net_amd"))
from ndnet import _lib  # noqa: E402
from ndnet.models import pointnet_hip as ph  # noqa: E402
from ndnet.models.ndtnet import NDTNetClassification  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("cls_forward.py measures on the GPU: none found")
dev = torch.device("cuda", 0)
B, N = a.batch, a.nds
torch.manual_seed(0)
x = torch.randn(B, N, 12, device=dev)
p, c = x[..., :3], x[..., 3:]


def event():
    return torch.cuda.Event(enable_timing=True)


def timed(fn, k):
    e0, e1 = event(), event()
    e0.record()
    for _ in range(k):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / k  # us


def log_err(out, ref64):
    return (out.double().log() - ref64.log()).abs().max().item()


variants = {}  # name -> (eager callable, graph)
report = {"shape": {"batch": B, "nds": N, "feature_dim": a.feature_dim}, "device": torch.cuda.get_device_name(dev),
          "rounds": a.rounds, "forwards_per_round": a.forwards, "launches_per_round": a.launches,
          "units": "microseconds per forward / launch; per-round values summarised as median / min / max",
          "baseline": "model.forward_torch(p, c): the torch composition this call ran before the HIP path",
          "models": {}, "head_alone": {}}
with torch.no_grad():
    for C in [int(s) for s in a.classes.split(",") if s]:
        m = NDTNetClassification(3, C, a.feature_dim).to(dev).eval()
        assert ph.supports_classification(m)
        ref64 = copy.deepcopy(m).double().forward_torch(p.double(), c.double())
        info = {"lowest_float64_probability": ref64.min().item(), "peak_float64_probability": ref64.max().item()}
        for path, fn in (("hip", lambda m=m: m(p, c)), ("torch", lambda m=m: m.forward_torch(p, c))):
            for _ in range(5):
                out = fn()
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                gout = fn()
            g.replay()
            torch.cuda.synchronize()
            info[path] = {"max_log_prob_err_vs_float64": log_err(out, ref64),
                          "max_log_prob_err_vs_float64_graphed": log_err(gout, ref64),
                          "graph_bit_equal_to_eager": bool(torch.equal(gout, out)),
                          "eager_us": [], "graph_us": []}
            variants[(C, path)] = (fn, g)
        report["models"][f"C{C}"] = info
    names = list(variants)
    for r in range(a.rounds):
        for key in names[r % len(names):] + names[:r % len(names)]:
            fn, g = variants[key]
            info = report["models"][f"C{key[0]}"][key[1]]
            timed(fn, 2)
            info["eager_us"].append(timed(fn, a.forwards))
            timed(g.replay, 2)
            info["graph_us"].append(timed(g.replay, a.forwards))
        print(f"round {r + 1}/{a.rounds}", flush=True)

    # the head kernel alone: 16 clouds, K = 256
    heads = {}
    for C in [int(s) for s in a.head_classes.split(",") if s]:
        Cp = (C + 15) // 16 * 16
        h2 = torch.relu(torch.randn(16, 256, device=dev))
        wf = ph._frag(ph._wT(torch.randn(C, 256, device=dev) / 16, 256, Cp))
        bias = ph._bpad(torch.randn(C, device=dev), Cp)
        out = torch.empty(16, C, device=dev)
        st = _lib.stream_ptr(dev)

        def launch(h2=h2, wf=wf, bias=bias, out=out, C=C, Cp=Cp):
            rc = _lib.lib().ndnet_pn_cls_head_run(h2.data_ptr(), 256, wf.data_ptr(), bias.data_ptr(), out.data_ptr(), C,
                                                  None, 0, 16, 256, Cp, C, None, 0, st)
            _lib.check(rc, "ndnet_pn_cls_head_run")
        heads[C] = launch
        report["head_alone"][f"C{C}"] = {"us": []}
    for r in range(a.rounds):
        for C, launch in heads.items():
            timed(launch, 5)
            report["head_alone"][f"C{C}"]["us"].append(timed(launch, a.launches))


def summary(v):
    s = sorted(v)
    return {"median": round(statistics.median(v), 2), "min": round(s[0], 2), "max": round(s[-1], 2),
            "per_round": [round(t, 2) for t in v]}


for name, info in report["models"].items():
    for path in ("hip", "torch"):
        for k in ("eager_us", "graph_us"):
            info[path][k] = summary(info[path][k])
    for k in ("eager_us", "graph_us"):
        info[f"torch_over_hip_{k[:-3]}"] = round(info["torch"][k]["median"] / info["hip"][k]["median"], 3)
for info in report["head_alone"].values():
    info["us"] = summary(info["us"])
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(report, f, indent=1)
    f.write("\n")
for name, info in report["models"].items():
    for path in ("hip", "torch"):
        v = info[path]
        print(f"{name:6s} {path:5s} eager {v['eager_us']['median']:8.1f} us [{v['eager_us']['min']:.1f}, "
              f"{v['eager_us']['max']:.1f}]  graphed {v['graph_us']['median']:8.1f} us [{v['graph_us']['min']:.1f}, "
              f"{v['graph_us']['max']:.1f}]  log-prob err {v['max_log_prob_err_vs_float64']:.2e}")
    print(f"{name:6s} torch / hip: eager {info['torch_over_hip_eager']:.2f}x  graphed {info['torch_over_hip_graph']:.2f}x")
for name, info in report["head_alone"].items():
    print(f"head alone {name}: {info['us']['median']:.2f} us [{info['us']['min']:.2f}, {info['us']['max']:.2f}]")
print("wrote", a.out)
