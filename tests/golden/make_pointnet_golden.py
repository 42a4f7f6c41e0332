#!/usr/bin/env python3
"""Generate the PointNet baseline fixtures under tests/golden/ (build container only).

The reference's own Python model (ndnet/models/pointnet.py, imported as
``refndnet.models.pointnet`` through ``make_golden.load_reference``'s
mechanism) with the closed-form weights of ``model_init.deterministic_state``
gives ``out_eval``; this package's CPU forward with the same weights must equal
it bit for bit.  The reference module imports ``ndnet.preprocessing.ndt_legacy``
by its absolute name, which resolves to this package's ``NDT_Sampler``; it
never uses it.  The files hold data only: inputs, the reference module's
outputs, its ``state_dict`` key names and its parameter count.

The first segmentation case also stores a train-mode output at 4 clouds, each
at its own scale and offset as in ``make_golden.model_train_fixture`` (the TNet
heads' BatchNorm1d then divides by a real spread over the clouds).

Run:  python tests/golden/make_pointnet_golden.py
"""
from __future__ import annotations

import importlib
import os

import numpy as np
import torch

from make_golden import HERE, load_reference  # also puts ndt-net_amd and tests/golden on sys.path
from model_init import deterministic_state
from ndnet.models import pointnet as ours_mod

SEG_CASES = [(768, 28, 2, 64), (64, 5, 2, 40)]    # F, C, clouds, points
CLS_CASES = [(768, 512, 2, 64), (64, 5, 2, 40)]
TRAIN_B, TRAIN_N = 4, 64


def _pair(ref_mod, kind: str, F: int, C: int):
    """The reference module and ours with the same deterministic weights."""
    ref = getattr(ref_mod, kind)(3, C, F)
    ref.load_state_dict(deterministic_state(ref.state_dict()))
    ours = getattr(ours_mod, kind)(3, C, F)
    assert list(ours.state_dict().keys()) == list(ref.state_dict().keys())
    ours.load_state_dict(deterministic_state(ours.state_dict()))
    return ref, ours


def main() -> None:
    load_reference()
    ref_mod = importlib.import_module("refndnet.models.pointnet")
    for kind, tag, cases in (("PointNetSegmentation", "seg", SEG_CASES), ("PointNetClassification", "cls", CLS_CASES)):
        for i, (F, C, B, N) in enumerate(cases):
            ref, ours = _pair(ref_mod, kind, F, C)
            rng = np.random.default_rng(11 * F + C + (tag == "cls"))
            pts = rng.uniform(-10, 10, (B, N, 3)).astype(np.float32)
            extra = {}
            with torch.no_grad():
                out_eval = ref.eval()(torch.from_numpy(pts)).numpy()
                out = ours.eval()(torch.from_numpy(pts)).numpy()
                assert np.array_equal(out, out_eval), "the CPU eval forwards differ"
                if tag == "seg" and i == 0:
                    scale = (0.5 + 0.25 * np.arange(TRAIN_B)).reshape(TRAIN_B, 1, 1)
                    shift = rng.uniform(-5, 5, (TRAIN_B, 1, 3))
                    tp = (rng.uniform(-10, 10, (TRAIN_B, TRAIN_N, 3)) * scale + shift).astype(np.float32)
                    out_train = ref.train()(torch.from_numpy(tp)).numpy()
                    _, ours_t = _pair(ref_mod, kind, F, C)  # (fresh running statistics)
                    assert np.array_equal(ours_t.train()(torch.from_numpy(tp)).numpy(), out_train), \
                        "the CPU train forwards differ"
                    extra = dict(points_train=tp, out_train=out_train)
            keys = list(ref.state_dict().keys())
            params = sum(p.numel() for p in ref.parameters())
            name = f"pointnet_{tag}_F{F}_C{C}.npz"
            np.savez_compressed(os.path.join(HERE, name), points=pts, feature_dim=F, num_classes=C, out_eval=out_eval,
                                state_keys=np.array(keys), param_count=params, **extra)
            print("wrote", name, "parameters", params, "out range", float(out_eval.min()), float(out_eval.max()))


if __name__ == "__main__":
    main()
