"""Both eval forwards with the x6 mode's split layers as two fp16 slices (NDNET_PN_SLICES=f16, the default:
ndnet_pn_chain_f16_run) and as three bf16 ones (=bf16: the forward as it was).

Shapes (tests/test_model_fold_products.py's, with its models and inputs): (B, N) = (3, 77) runs every chain
on the 32-point build, (65, 65) on the 64-point build; F = 64, 5 classes.  The default is held to 1e-4 of
``forward_torch`` (tests/test_model_collapse.py's TOL) with the arg-max wherever torch's top two are further
apart than twice that; =bf16 to the output recorded from the parent commit's build, bit for bit
(tests/golden/f16_slices_parent_<build>_<kind>.npy)."""
import os

import numpy as np
import pytest
import torch

from model_init import deterministic_state
from test_model_fold_products import SHAPES, _scores, inputs, model

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL = 1e-4


def _spy(monkeypatch):
    """The argument blocks of the chain launches, in launch order."""
    from ndnet.models import pointnet_hip as ph
    blocks, real = [], ph._run_chain

    def spy(blk, *a, **k):
        blocks.append(blk)
        return real(blk, *a, **k)

    monkeypatch.setattr(ph, "_run_chain", spy)
    return blocks


def _f16_blocks(blocks):
    return [getattr(b, "f16", None) is not None for b in blocks if not hasattr(b, "tail")]


@pytest.mark.gpu
@pytest.mark.parametrize("build", sorted(SHAPES))
@pytest.mark.parametrize("kind", ["seg", "cls"])
def test_default_runs_the_fp16_form_within_tolerance(monkeypatch, kind, build):
    from ndnet.models import pointnet_hip as ph
    assert ph.SLICES == "f16", "the default"
    B, N, seed = SHAPES[build]
    p, c = inputs(B, N, seed)
    blocks = _spy(monkeypatch)
    m = model(kind)
    with torch.no_grad():
        out = m(p, c)
        ref = m.forward_torch(p, c)
    (ws,) = m._hip["ws"].values()
    assert ws.uses_f16()
    # chains A, B and D (a classification model has no D); chain C is the 12 -> F launch, which has no split layer
    assert _f16_blocks(blocks) == [True] * (3 if kind == "seg" else 2)
    fallbacks = ws.take_f16_fallbacks()
    err = (out - ref).abs().max().item()
    print(f"{kind} {build}: |fp16 form - torch fp32| {err:.3e}, fallback tiles {fallbacks}")
    assert out.shape == ref.shape and out.dtype == torch.float32
    assert err < TOL
    assert fallbacks == 0 and ws.take_f16_fallbacks() == 0
    top2 = _scores(kind, ref).topk(2, dim=-1).values
    clear = (top2[..., 0] - top2[..., 1]) > 2 * TOL
    assert bool(clear.any())
    assert torch.equal(_scores(kind, out).argmax(-1)[clear], _scores(kind, ref).argmax(-1)[clear])


@pytest.mark.gpu
@pytest.mark.parametrize("build", sorted(SHAPES))
@pytest.mark.parametrize("kind", ["seg", "cls"])
def test_bf16_slices_equal_the_recorded_output(monkeypatch, kind, build):
    """NDNET_PN_SLICES=bf16 is the default forward as it was, bit for bit (inputs and weights as built here)."""
    from ndnet.models import pointnet_hip as ph
    B, N, seed = SHAPES[build]
    monkeypatch.setattr(ph, "SLICES", "bf16")
    blocks = _spy(monkeypatch)
    p, c = inputs(B, N, seed)
    m = model(kind)
    with torch.no_grad():
        out = m(p, c).cpu().numpy()
    assert not any(_f16_blocks(blocks))
    assert m._hip["W"].frag16 == {} and m._hip["W"].jobs16 == [], "no fp16 planes are built or re-folded for this form"
    want = np.load(os.path.join(GOLDEN, f"f16_slices_parent_{build}_{kind}.npy"))
    assert out.shape == want.shape and out.dtype == want.dtype
    assert np.array_equal(out.view(np.int32), want.view(np.int32))


SWITCHES = ["default", "SLICES=bf16", "COLLAPSE=0", "FOLD_PRODUCTS=0", "BACKBONE=chain", "FOLD_T2=chain", "x3", "bf16",
            "fp32", "many classes", "baseline"]


@pytest.mark.gpu
@pytest.mark.parametrize("setting", SWITCHES)
def test_which_settings_run_the_fp16_form(monkeypatch, setting):
    """Only the x6 mode's default forward: every switch that changes it keeps ndnet_pn_chain_run everywhere."""
    from ndnet.models import pointnet_hip as ph
    from ndnet.models.ndtnet import NDTNetSegmentation
    from ndnet.models.pointnet import PointNetSegmentation
    blocks = _spy(monkeypatch)
    p, c = inputs(3, 77, 5)
    m = model("seg")
    if setting in ph.MODES:
        m.precision = setting
    elif setting == "many classes":  # chain D stays layered past 256 padded classes
        m = NDTNetSegmentation(3, 300, 64)
        m.load_state_dict(deterministic_state(m.state_dict()))
        m = m.cuda().eval()
    elif setting == "baseline":
        m = PointNetSegmentation(3, 28, 64)
        m.load_state_dict(deterministic_state(m.state_dict()))
        m = m.cuda().eval()
    elif setting != "default":
        name, value = setting.split("=")
        attr = {"FOLD_T2": "FOLD_T2_KERNEL"}.get(name, name)
        monkeypatch.setattr(ph, attr, {"0": False, "chain": "chain" if name == "BACKBONE" else False, "bf16": "bf16"}[value])
    with torch.no_grad():
        out = m(p) if setting == "baseline" else m(p, c)
        ref = m.forward_torch(p) if setting == "baseline" else m.forward_torch(p, c)
    (ws,) = m._hip["ws"].values()
    on = setting == "default"
    assert ws.uses_f16() == on
    got = _f16_blocks(blocks)
    assert got == ([True] * 3 if on else [False] * len(got)) and len(got) >= 3
    assert ws.take_f16_fallbacks() == 0
    if setting not in ("x3", "bf16"):  # (the reduced modes' accuracy: tests/test_model_precision.py)
        assert (out - ref).abs().max().item() < TOL


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["seg", "cls"])
def test_captured_graph_replays_equal_to_eager(kind):
    B, N = 3, 77
    m = model(kind)
    p, c = inputs(B, N, 9)
    with torch.no_grad():
        m(p, c)  # fold, workspace and argument blocks
        (ws,) = m._hip["ws"].values()
        assert ws.uses_f16()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = m(p, c)
        for seed in (10, 11):
            p2, c2 = inputs(B, N, seed)
            p.copy_(p2)
            c.copy_(c2)
            g.replay()
            torch.cuda.synchronize()
            got = out.clone()
            assert torch.equal(got, m(p2, c2))
    assert ws.take_f16_fallbacks() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["seg", "cls"])
def test_refold_in_place_is_followed(kind):
    """Weights and running statistics changed and re-folded in place: the fp16 planes and scales follow (same
    tensors, same argument blocks), equal to a fresh fold's, and so does the next forward."""
    from ndnet.models import pointnet_hip as ph
    p, c = inputs(3, 77, 7)
    m = model(kind)
    with torch.no_grad():
        first = m(p, c).clone()
    W = m._hip["W"]
    old = {k: (W.frag16[k].clone(), W.scale16[k].clone()) for k in W.frag16}
    g = torch.Generator(device="cuda").manual_seed(8)
    with torch.no_grad():
        for t in list(m.parameters()) + [b for b in m.buffers() if b.is_floating_point()]:
            t.mul_(1.0 + 0.05 * torch.randn(t.shape, device="cuda", generator=g))
            if t.dim() == 1:
                t.add_(0.01 * torch.rand(t.shape, device="cuda", generator=g))  # running_var stays > 0
        m.feature_extractor.conv2.weight.mul_(4.0)  # one layer's scale moves by two powers of two
        out = m(p, c)
        ref = m.forward_torch(p, c)
    assert m._hip["W"] is W, "the re-fold must be in place"
    assert all(not torch.equal(W.frag16[k].view(torch.int16), old[k][0].view(torch.int16)) for k in old)
    assert any(not torch.equal(W.scale16[k], old[k][1]) for k in old)
    fresh = ph._Folded(m)
    assert fresh.ensure_f16()
    for w, f in zip(W.wide, fresh.wide):
        assert torch.equal(W.frag16[id(w)].view(torch.int16), fresh.frag16[id(f)].view(torch.int16))
        assert torch.equal(W.scale16[id(w)], fresh.scale16[id(f)])
    e_new, e_old = (out - ref).abs().max().item(), (first - ref).abs().max().item()
    print(f"{kind}: after the re-fold {e_new:.3e} from torch fp32; the forward before it {e_old:.3e}")
    assert e_new < TOL and e_old > 10 * TOL
    (ws,) = m._hip["ws"].values()
    assert ws.uses_f16()
