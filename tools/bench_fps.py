#!/usr/bin/env python3
"""Time farthest point sampling (ndnet.preprocessing.farthest_point_sample, the
HIP kernel of include/ndnet_fps.h) on the GPU.

Shape: 16 x 100k float32 points (Gaussian, seeded), one process.

* the kernel at ``--samples`` (default 1024, 8192, 70000): device events around
  one launch, after a warm-up launch of the same shape, ``--repeats`` times;
  median, minimum and maximum, and the time per sample.  The time per sample
  should be flat in S; the spread to judge that against is the
  minimum-to-maximum range of the repeats, reported beside it.
* the same algorithm composed from torch ops on the same GPU at the first S:
  a Python loop over subtract / square / sum, ``torch.minimum``, an indexed
  store and ``argmax`` (at least four launches per sample), timed the same way
  and alternated with the kernel's repeats.  Its per-sample time is reported;
  it is not run to 70000.  How many of its indices equal the kernel's is
  counted, not required: torch's reduction need not round like the definition.
* the numpy oracle (tests/fps_ref.py) on the CPU at S = 256 for one cloud,
  scaled linearly in S and in B to the first S of the batch: an extrapolation,
  marked as one.
* a small shape for the other storage tier (16 x 4096 -> 2048: coordinates in
  LDS), kernel and torch loop.

Writes JSON (default profiles/fps.json).  Measures on the GPU only.

    python tools/bench_fps.py [--out profiles/fps.json]
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
ap.add_argument("--samples", default="1024,8192,70000")
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--oracle-samples", type=int, default=256)
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "fps.json"))
a = ap.parse_args()

sys.path.insert(0, os.path.join(REPO, "ndt-net_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("bench_fps.py measures on the GPU; none is visible")
from fps_ref import fps_ref  # noqa: E402
from ndnet.preprocessing import farthest_point_sample  # noqa: E402


def torch_fps(pts, S):
    """The definition's loop from torch ops (first maximum: torch.argmax)."""
    B, n, _ = pts.shape
    mind = torch.full((B, n), float("inf"), dtype=pts.dtype, device=pts.device)
    idx = torch.empty((B, S), dtype=torch.int64, device=pts.device)
    cur = torch.zeros(B, dtype=torch.int64, device=pts.device)
    ar = torch.arange(B, device=pts.device)
    for t in range(S):
        idx[:, t] = cur
        d = pts - pts[ar, cur][:, None, :]
        d = (d * d).sum(-1)
        mind = torch.minimum(mind, d)
        mind[ar, cur] = -1
        cur = mind.argmax(1)
    return idx


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def summary(ms, S):
    med = statistics.median(ms)
    return {"ms_median": med, "ms_min": min(ms), "ms_max": max(ms), "repeats": len(ms),
            "us_per_sample_median": med * 1e3 / S, "us_per_sample_min": min(ms) * 1e3 / S,
            "us_per_sample_max": max(ms) * 1e3 / S}


def measure(B, n, samples, repeats, with_torch_at):
    pts = torch.from_numpy((np.random.default_rng(0).standard_normal((B, n, 3)) * 20).astype(np.float32)).cuda()
    out = {"batch": B, "points": n, "dtype": "float32", "kernel": {}, "torch_loop": {}}
    for S in samples:
        idx = torch.empty((B, S), dtype=torch.int32, device="cuda")
        md = torch.empty((B, n), dtype=torch.float32, device="cuda")
        run = lambda: farthest_point_sample(pts, S, out=idx, min_dist=md)  # noqa: E731
        timed(run)  # warm-up
        k_ms, t_ms, t_idx = [], [], None
        if S == with_torch_at:
            timed(lambda: torch_fps(pts, min(S, 64)))  # warm-up of every op the loop uses
        for _ in range(repeats):
            k_ms.append(timed(run)[0])
            if S == with_torch_at:
                ms, t_idx = timed(lambda: torch_fps(pts, S))
                t_ms.append(ms)
        out["kernel"][str(S)] = summary(k_ms, S)
        if t_ms:
            out["torch_loop"][str(S)] = summary(t_ms, S)
            out["torch_loop"][str(S)]["indices_equal_to_kernel"] = int((t_idx == idx.long()).sum())
            out["torch_loop"][str(S)]["indices_total"] = B * S
            k, t = out["kernel"][str(S)], out["torch_loop"][str(S)]
            out["kernel_speedup_over_torch_loop"] = t["us_per_sample_median"] / k["us_per_sample_median"]
            out["kernel_beats_torch_loop"] = k["us_per_sample_max"] < t["us_per_sample_min"]
    return out, pts


samples = [int(s) for s in a.samples.split(",")]
res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__}
big, pts = measure(a.batch, a.points, samples, a.repeats, samples[0])
per = [big["kernel"][str(S)]["us_per_sample_median"] for S in samples]
big["us_per_sample_by_samples"] = dict(zip(map(str, samples), per))
big["us_per_sample_max_over_min"] = max(per) / min(per)
res["flagship"] = big

cloud = pts[0].cpu().numpy()
t0 = time.perf_counter()
o_idx, _ = fps_ref(cloud, a.oracle_samples)
o_s = time.perf_counter() - t0
g_idx = farthest_point_sample(pts[:1], a.oracle_samples)[0].cpu().numpy()
res["numpy_oracle_cpu"] = {
    "measured": {"clouds": 1, "points": a.points, "samples": a.oracle_samples, "seconds": o_s,
                 "us_per_sample_per_cloud": o_s * 1e6 / a.oracle_samples},
    "extrapolated_linearly_in_S_and_B": {"clouds": a.batch, "samples": samples[0],
                                         "seconds": o_s * samples[0] / a.oracle_samples * a.batch,
                                         "us_per_sample": o_s * 1e6 / a.oracle_samples * a.batch},
    "indices_equal_to_kernel": bool(np.array_equal(o_idx, g_idx)),
}
small, _ = measure(a.batch, 4096, [2048], a.repeats, 2048)
res["small"] = small

os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
print(json.dumps(res))
