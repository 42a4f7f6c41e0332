#!/usr/bin/env python3
"""Time packed int16 point input (ndnet.packed) against float32 input.

Shape C2 by default: 16 x 100k points -> 1000 NDs, synthetic U and L clouds
(ndnet.synthetic), the model and the stream counts of
tools/bench_pipeline_labels.py (one NDT stream for U, two for L), one process
on one GPU.  Every group of variants is timed in rounds that alternate them
(the order rotated by one each round) after a warm-up of each; the figures are
median [min, max] over the rounds.

* (a) ``decode``: ``ndnet_pts_unpack_i16`` alone, --iters launches replayed from
  one HIP graph, rotating over --copies input and output buffers, without
  counts (``hip``) and with counts spread evenly over n / 2 .. n
  (``hip_counts``), against the capturable torch composition writing the same
  output buffers (``torch``: ``out.copy_(q); out.mul_(step); out.add_(origin)``,
  three launches); microseconds per decode and achieved bytes/s over the 18
  bytes per decoded point the algorithm needs
* (b) ``streamed``: ``replay_streamed`` from pinned host memory, float32 against
  ``packed=True``, without labels and with ``point_labels="nearest"`` and the
  uint8 labels copied back; a host clock around --steps calls ending in a
  device synchronise
* (c) ``resident``: ``replay_steps(--steps)`` on a resident batch, float32
  against packed, device events around the call: the price of the extra launch
* (d) ``label_disagreement``: the share of the points that get another label
  from the float32 pipeline on the original cloud than from the packed
  pipeline on ``pack_points(original)`` at the default step; recorded, not
  asserted

``conditions`` records, from this run's own medians, whether the HIP decode
beat the torch composition and whether the packed streamed pipeline beat the
float32 one on U without labels.  Writes JSON (default
profiles/packed_input.json).  Measures on the GPU only.

    python tools/bench_packed.py [--out profiles/packed_input.json]
"""
import argparse
import gc
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
ap.add_argument("--iters", type=int, default=64, help="isolated decodes per round")
ap.add_argument("--copies", type=int, default=16, help="input / output buffers the isolated decodes rotate over")
ap.add_argument("--kinds", default="U,L")
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "packed_input.json"))
a = ap.parse_args()
if a.rounds < 5:
    sys.exit("at least 5 rounds")

import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.path.insert(0, os.path.join(REPO, "ndt-net_amd"))
from ndnet.models.ndtnet import NDTNetSegmentation  # noqa: E402
from ndnet.packed import pack_points, unpack  # noqa: E402
from ndnet.pipeline import PipelinedSegmentation  # noqa: E402
from ndnet.synthetic import make_batch  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("bench_packed.py measures on the GPU: none found")
dev = torch.device("cuda", 0)
B, N, K = a.batch, a.points, a.nds


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


def alternate(variants, rounds):
    """name -> [us per round]; variants: name -> (timer, fn).  A warm-up of
    each, then rounds in rotating order."""
    names = list(variants)
    for timer, fn in variants.values():
        timer(fn)
    us = {nm: [] for nm in names}
    for r in range(rounds):
        for nm in names[r % len(names):] + names[:r % len(names)]:
            timer, fn = variants[nm]
            us[nm].append(timer(fn))
    return us


result = {
    "shape": {"batch": B, "points": N, "nds": K, "classes": a.classes, "feature_dim": a.feature_dim},
    "device": torch.cuda.get_device_name(0),
    "rounds": a.rounds, "steps_per_round": a.steps, "decodes_per_round": a.iters, "decode_copies": a.copies,
    "units": "clouds_per_s: batch x steps over the timed window, per round (median / min / max); step_us: the "
             "median window over its steps; decode us: microseconds per decode of the whole batch",
    "timing": "decode and resident: device events around the window; streamed: a host clock around the calls, "
              "ending in a device synchronise",
    "bytes_per_batch": {"float32": 12 * B * N, "packed": 6 * B * N + 16 * B},
    "kinds": {},
}
torch.manual_seed(0)
model = NDTNetSegmentation(3, a.classes, a.feature_dim).to(dev).eval()

# (a) the decode alone
host_u = make_batch("U", B, N)
q_u, qp_u = pack_points(host_u)
counts = [int(c) for c in np.linspace(N // 2, N, B).round()]
qs = [q_u.to(dev) for _ in range(a.copies)]
outs = [torch.empty((B, N, 3), dtype=torch.float32, device=dev) for _ in range(a.copies)]
qp_d = qp_u.to(dev)
cd = torch.tensor(counts, dtype=torch.int32, device=dev)
step_b, origin_b = qp_d[:, None, 3:4].contiguous(), qp_d[:, None, 0:3].contiguous()


def torch_decode(i):
    o = outs[i % a.copies]
    o.copy_(qs[i % a.copies])
    o.mul_(step_b)
    o.add_(origin_b)


decoders = {
    "hip": graphed_launches(lambda i: unpack(qs[i % a.copies], qp_d, out=outs[i % a.copies]), a.iters),
    "hip_counts": graphed_launches(lambda i: unpack(qs[i % a.copies], qp_d, cd, out=outs[i % a.copies]), a.iters),
    "torch": graphed_launches(torch_decode, a.iters),
}
decoders["torch"]()
torch.cuda.synchronize(dev)
same = bool(torch.equal(outs[0], unpack(qs[0], qp_d)))
dus = alternate({nm: (event_us, fn) for nm, fn in decoders.items()}, a.rounds)
dbytes = {"hip": 18 * B * N, "torch": 18 * B * N, "hip_counts": 18 * sum(counts)}
decode = {nm: dict(summary([t / a.iters for t in v], 2), algorithmic_bytes=dbytes[nm],
                   GBps=round(dbytes[nm] / (statistics.median(v) / a.iters) / 1e3, 1)) for nm, v in dus.items()}
decode["torch_equals_hip"] = same
decode["counts"] = counts
result["decode"] = decode
print("decode", json.dumps({nm: decode[nm]["median"] for nm in dus}), "torch == hip:", same, flush=True)
del qs, outs
torch.cuda.empty_cache()

for kind in a.kinds.split(","):
    ndt_streams = 2 if kind == "L" else 1  # as bench.py runs the two kinds
    host = make_batch(kind, B, N)
    q, qp = pack_points(host)
    pts = torch.from_numpy(host).to(dev)

    def pipe(packed, **kw):
        p = PipelinedSegmentation(model, K, B, N, device=dev, ndt_streams=ndt_streams, packed=packed, **kw)
        if packed:
            p.load_resident(q.to(dev), qparams=qp)
        else:
            p.load_resident(pts)
        return p

    u8 = dict(point_labels="nearest", label_dtype=torch.uint8)
    # no cyclic collection while stage graphs are being captured: the previous kind's pipelines are
    # garbage with reference cycles, and destroying their graphs and streams under a capture in
    # progress invalidates it (collected explicitly at the end of each kind instead)
    gc.collect()
    gc.disable()
    resident = {"f32": pipe(False), "packed": pipe(True)}
    streamed = {"f32": pipe(False), "packed": pipe(True), "f32_u8": pipe(False, **u8), "packed_u8": pipe(True, **u8)}
    check = PipelinedSegmentation(model, K, B, N, device=dev, ndt_streams=ndt_streams, **u8)
    gc.enable()
    host_f32 = [torch.from_numpy(host).pin_memory() for _ in range(2)]
    host_q = [q.clone().pin_memory() for _ in range(2)]
    host_qp = [qp.clone().pin_memory() for _ in range(2)]
    host_labels = [torch.empty((B, N), dtype=torch.uint8).pin_memory() for _ in range(2)]

    def streamed_loop(nm):
        p, packed, labelled = streamed[nm], nm.startswith("packed"), nm.endswith("u8")

        def run():
            for s in range(a.steps):
                lb = host_labels[s % 2] if labelled else None
                if packed:
                    p.replay_streamed(host_q[s % 2], None, lb, host_qp[s % 2])
                else:
                    p.replay_streamed(host_f32[s % 2], None, lb)
        return run

    res_us = alternate({nm: (event_us, (lambda p=p: p.replay_steps(a.steps))) for nm, p in resident.items()}, a.rounds)
    str_us = alternate({nm: (host_us, streamed_loop(nm)) for nm in streamed}, a.rounds)
    torch.cuda.synchronize(dev)
    rcs_ok = all(st.rc == 0 for p in list(resident.values()) + list(streamed.values())
                 for plan in p.plans for st in plan.host_stats())
    # (d): the labels of the two labelled pipelines after the same number of steps on the same batch
    lf, lp = streamed["f32_u8"].point_labels, streamed["packed_u8"].point_labels
    differ = float((lf != lp).float().mean())
    unassigned = float((lf == 255).float().mean())
    # ... and, independent of the (untrained) model: how far the NDs themselves move -- every float32
    # ND mean's distance to the nearest ND mean of the packed run (every slot holds the same batch)
    nn = torch.cdist(streamed["f32_u8"].rows[0][0][..., :3], streamed["packed_u8"].rows[0][0][..., :3]).amin(dim=2)
    nd_moved = {"median_m": round(float(nn.median()), 5), "p99_m": round(float(nn.flatten().quantile(0.99)), 5),
                "max_m": round(float(nn.max()), 5), "share_within_1cm": round(float((nn <= 0.01).float().mean()), 4)}
    # the packed pipeline computes what the float32 one computes on the decoded cloud
    check.load_resident(unpack(q.to(dev), qp.to(dev)))
    check.replay_steps(check.R + 1)
    torch.cuda.synchronize(dev)
    exact = bool(torch.equal(check.point_labels, lp))

    def rates(us):
        return ({nm: summary([B * a.steps / (t * 1e-6) for t in v]) for nm, v in us.items()},
                {nm: round(statistics.median(v) / a.steps, 2) for nm, v in us.items()})

    res_rate, res_step = rates(res_us)
    str_rate, str_step = rates(str_us)
    result["kinds"][kind] = {
        "ndt_streams": ndt_streams, "ring": resident["f32"].R,
        "default_step_mm": [round(float(s) * 1e3, 3) for s in qp[:, 3]],
        "resident": {"clouds_per_s": res_rate, "step_us": res_step},
        "streamed": {"clouds_per_s": str_rate, "step_us": str_step,
                     "GBps_in": {nm: round((6 if nm.startswith("packed") else 12) * B * N / str_step[nm] / 1e3, 1)
                                 for nm in str_step}},
        "packed_over_f32": {"resident": round(res_rate["packed"]["median"] / res_rate["f32"]["median"], 3),
                            "streamed": round(str_rate["packed"]["median"] / str_rate["f32"]["median"], 3),
                            "streamed_u8": round(str_rate["packed_u8"]["median"] / str_rate["f32_u8"]["median"], 3)},
        "label_disagreement": {"share_of_points": round(differ, 6), "unassigned_share_f32": round(unassigned, 6),
                               "how": "uint8 nearest-fill labels, float32 pipeline on the original cloud against the "
                                      "packed pipeline on pack_points(original), default step; recorded, not asserted; "
                                      "the model is untrained (seed 0), so its argmax is sensitive to any change of an ND",
                               "nd_mean_to_nearest_packed_nd_mean": nd_moved},
        "packed_labels_equal_f32_on_decoded": exact, "every_cloud_rc_0": bool(rcs_ok),
    }
    print(kind, json.dumps({"resident_us": res_step, "streamed_us": str_step, "differ": differ, "nd_moved": nd_moved, "exact": exact,
                            "rc0": rcs_ok}), flush=True)
    del resident, streamed, check, lf, lp
    gc.collect()
    torch.cuda.synchronize(dev)
    torch.cuda.empty_cache()

hip, tor = result["decode"]["hip"]["median"], result["decode"]["torch"]["median"]
cond = {"hip_decode_faster_than_torch": bool(hip < tor), "hip_over_torch_time": round(hip / tor, 3)}
if "U" in result["kinds"]:
    r = result["kinds"]["U"]["packed_over_f32"]["streamed"]
    cond["packed_streamed_faster_than_f32_on_U"] = bool(r > 1.0)
    cond["packed_over_f32_streamed_U"] = r
result["conditions"] = cond
print("conditions", json.dumps(cond), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
print("wrote", a.out)
