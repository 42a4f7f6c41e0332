"""The precision modes of the eval forward at the model: "x3" and "bf16"
(pointnet_hip.set_precision, NDTNetSegmentation.precision) against a float64
emulation of the same folded forward and against float64 ``forward_torch``.

The emulator is ``segmentation_forward(..., chain=<emulator>)``: the chains
in float64, with the layers that have a split-bf16 copy (``W.frag6``)
truncated as the kernel truncates them (test_pn_precision._emu64: operands
h = bf16(x), m = bf16(x - h); "x3" keeps h h' + h m' + m h', "bf16" h h').
With e_emu = max |emulation - float64| and e_hip = max |HIP - float64| over
the log-probs, every mode is held to  e_emu / 3 <= e_hip <= 3 e_emu + 1e-6
(the factor: the project's allowance for summation order, and the rare
activation whose bf16 rounding flips on an fp32 last-bit difference).

Figures measured on an MI355X: DESIGN.md §3, "Reduced split-bf16 modes"."""
import copy
import os
import subprocess
import sys

import pytest
import torch

from model_init import deterministic_state
from test_pn_precision import _hm

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model(F, C, device="cpu"):
    from ndnet.models.ndtnet import NDTNetSegmentation
    m = NDTNetSegmentation(3, C, F)
    m.load_state_dict(deterministic_state(m.state_dict()))
    return m.to(device).eval()


def _inputs(B, N, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.rand((B, N, 3), device="cuda", generator=g) * 20 - 10,
            torch.randn((B, N, 9), device="cuda", generator=g))


def _emulator(W, mode):
    """pointnet_hip._chain_torch in float64, the layers with a split-bf16 copy reduced to `mode`."""
    def chain(x, n, in_cols, layers, relus, cmode, gmax=None, out=None, out_cols=0, fuse=()):
        h = x[..., :in_cols].double()
        h = torch.nn.functional.pad(h, (0, layers[0][0].shape[-2] - in_cols))
        for i, (w, b) in enumerate(layers):
            bb = (b[:, None, :] if b.dim() == 2 else b).double()
            wk = w[..., : h.shape[-1], :]
            reduced = mode in ("x3", "bf16") and id(w) in W.frag6
            if reduced:
                ah, am = _hm(h.float())
                wh, wm = _hm(wk.float())
                y = torch.matmul(ah, wh)
                if mode == "x3":
                    y = y + torch.matmul(ah, wm) + torch.matmul(am, wh)
                h = y + bb
            else:
                h = torch.matmul(h, wk.double()) + bb
            if relus[i]:
                h = torch.relu(h)
            if reduced:
                h = h.float().double()
        if cmode == 0:
            gmax.copy_(torch.maximum(gmax.double(), h.amax(dim=1)))
        else:
            out.copy_(torch.log_softmax(h[..., :out_cols], dim=2))
    return chain


_shared = {}


def _shape(F, C, B, N):
    """Model, inputs and the float64 forward of one shape, computed once."""
    key = (F, C, B, N)
    if key not in _shared:
        m = _model(F, C, "cuda")
        p, c = _inputs(B, N, F + C + N)
        with torch.no_grad():
            ref64 = copy.deepcopy(m).double().forward_torch(p.double(), c.double())
        _shared[key] = (m, p, c, ref64)
    return _shared[key]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["x3", "bf16"])
@pytest.mark.parametrize("F,C,B,N", [(768, 28, 16, 1000), (64, 5, 3, 77)], ids=["F768-t64", "F64-t32"])
def test_reduced_modes_match_their_emulation(F, C, B, N, mode):
    """16 x 1000 runs the 64-point build, 3 x 77 the 32-point build."""
    from ndnet.models import pointnet_hip as ph
    m, p, c, ref64 = _shape(F, C, B, N)
    assert ph._use_t32(B, N, p.device) == (N == 77)
    try:
        m.precision = mode
        with torch.no_grad():
            out = m(p, c)
            emu = ph.segmentation_forward(m, p, c, chain=_emulator(ph._folded(m)["W"], mode))
            m.precision = "x6"
            x6 = m(p, c)
    finally:
        m.precision = None
    assert out.shape == (B, N, C + 1) and out.dtype == torch.float32
    assert bool(torch.isfinite(out).all())
    lse = torch.logsumexp(out.double(), dim=-1).abs().max().item()
    e_hip = (out.double() - ref64).abs().max().item()
    e_emu = (emu.double() - ref64).abs().max().item()
    e_x6 = (x6.double() - ref64).abs().max().item()
    agree = (out.argmax(-1) == ref64.argmax(-1)).double().mean().item()
    print(f"F={F} C={C} {B}x{N} {mode}: e_hip {e_hip:.3e} e_emu {e_emu:.3e} (x6 {e_x6:.3e}) "
          f"e_hip/e_emu {e_hip / e_emu:.2f} |logsumexp| {lse:.1e} argmax agreement with float64 {100 * agree:.2f}%")
    assert lse <= 1e-5
    assert e_emu / 3 <= e_hip <= 3 * e_emu + 1e-6


@pytest.mark.gpu
def test_precision_attribute_takes_effect_on_the_next_forward():
    """No ``_hip`` reset: the attribute is read at every forward; None returns
    to the module-wide mode, bit for bit; another model never notices."""
    m, p, c, _ = _shape(64, 5, 3, 77)
    other = _model(64, 5, "cuda")
    assert m.precision is None and other.precision is None
    with torch.no_grad():
        before, other_before = m(p, c).clone(), other(p, c).clone()
        cache = m._hip
        try:
            m.precision = "bf16"
            low = m(p, c).clone()
            other_during = other(p, c).clone()
        finally:
            m.precision = None
        after = m(p, c).clone()
    assert m._hip is cache and cache["W"] is m._hip["W"]
    assert not torch.equal(low, before)
    assert (low - before).abs().max().item() > 1e-5  # bf16 level, not a re-ordered x6
    assert torch.equal(after, before)
    assert torch.equal(other_during, other_before) and torch.equal(other_before, before)


@pytest.mark.gpu
def test_graphed_segmentation_keeps_the_mode_it_captured():
    from ndnet.pipeline import GraphedSegmentation
    from ndnet.preprocessing.ndtnet_preprocessing import ndt_preprocessing
    from ndnet.synthetic import make_batch
    B, n, k = 2, 4096, 256
    m = _model(768, 28, "cuda")
    pts = torch.from_numpy(make_batch("U", B, n)).cuda()
    try:
        m.precision = "x3"
        with torch.no_grad():
            p, c, _ = ndt_preprocessing(k, pts)
            eager = m(p, c).clone()
        g = GraphedSegmentation(m, k, B, n)
        m.precision = None  # the graph recorded x3's kernels and argument blocks
        out = g(pts).clone()
        torch.cuda.synchronize()
        with torch.no_grad():
            default = m(p, c).clone()
    finally:
        m.precision = None
    assert torch.equal(out, eager)
    assert not torch.equal(default, eager)


# ---- no GPU ----

def test_set_precision_names():
    from ndnet.models import pointnet_hip as ph
    saved = ph.PRECISION
    try:
        with pytest.raises(ValueError):
            ph.set_precision("x4")
        assert ph.PRECISION == saved
        for name, prec in (("x6", 1), ("fp32", 1), ("x3", 2), ("bf16", 3)):
            ph.set_precision(name)
            assert (ph.PRECISION, ph.X6_PREC, ph.SPLIT_BF16) == (name, prec, name != "fp32")
    finally:
        ph.set_precision(saved)


def test_precision_from_the_environment():
    """NDNET_PN_PRECISION in a fresh process (the module reads it at import)."""
    env = dict(os.environ, NDNET_PN_PRECISION="x3")
    code = ("import sys; sys.path.insert(0, sys.argv[1]); from ndnet.models import pointnet_hip as ph; "
            "print('PRECISION', ph.PRECISION, ph.X6_PREC)")
    r = subprocess.run([sys.executable, "-c", code, os.path.join(REPO, "ndt-net_amd")], env=env,
                       capture_output=True, text=True, check=True)
    assert "PRECISION x3 2" in r.stdout


def test_precision_is_a_plain_attribute():
    from ndnet.models import pointnet_hip as ph
    from ndnet.models.ndtnet import NDTNetSegmentation
    m = NDTNetSegmentation(3, 28, 768)
    assert m.precision is None
    keys, count = list(m.state_dict()), sum(p.numel() for p in m.parameters())
    m.precision = "bf16"
    assert list(m.state_dict()) == keys and not any("precision" in k for k in keys)
    assert sum(p.numel() for p in m.parameters()) == count == 3_366_822
    assert "precision" not in dict(m.named_buffers()) and "precision" not in dict(m.named_parameters())
    assert ph.model_precision(m) == "bf16"
    m.precision = None
    assert ph.model_precision(m) == ph.PRECISION
    m.precision = "x4"
    with pytest.raises(ValueError):
        ph.model_precision(m)
