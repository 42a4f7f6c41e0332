"""Chain C collapsed to one per-cloud 12 -> F layer: the algebra in float64
against the layered chain (``pointnet_hip._chain_torch`` on ``specs[2]``), and
the kernel's fp32 arithmetic, restated on the CPU, against float64 under the
bound the GPU tests hold the kernel to (tests/pool12_ref.py).  No GPU."""
import pytest
import torch

import pool12_ref as R
from model_init import deterministic_state


class _F64(torch.Tensor):
    """``_chain_torch`` takes its input with ``.float()``; this input stays float64."""

    def float(self):
        return self.as_subclass(torch.Tensor).double()


def _chain_c(F, B=3, N=77):
    """A model's chain C after one emulated forward: (x [B,N,12], the layers
    of ``specs[2]`` as (W^T, bias) pairs, its ReLU flags)."""
    from ndnet.models import pointnet_hip as ph
    from ndnet.models.ndtnet import NDTNetSegmentation
    m = NDTNetSegmentation(3, 5, F)
    m.load_state_dict(deterministic_state(m.state_dict()))
    m.eval()
    g = torch.Generator().manual_seed(F)
    p, c = torch.rand((B, N, 3), generator=g) * 20 - 10, torch.randn((B, N, 9), generator=g)
    with torch.no_grad():
        ph.segmentation_forward(m, p, c, chain=ph._chain_torch)  # fills the per-cloud folded conv1 (w1t2, b1t2)
    (ws,) = m._hip["ws"].values()
    in_cols, layers, relus, mode, _ = ws.specs[2]
    assert in_cols == 12 and mode == 0 and len(layers) == 3
    return torch.cat((p, c), dim=2), [(w.clone(), b.clone()) for w, b in layers], relus


@pytest.mark.parametrize("F", [64, 100, 768])
def test_collapse_equals_the_layered_chain_in_float64(F):
    from ndnet.models import pointnet_hip as ph
    x, layers, relus = _chain_c(F)
    assert relus == (0, 0, 0), "the collapse needs a ReLU-free chain C"
    Fp = layers[2][0].shape[1]
    assert Fp == ph._npad(F)
    g_chain = torch.full((x.shape[0], Fp), float("-inf"), dtype=torch.float64)
    ph._chain_torch(x.double().as_subclass(_F64), x.shape[1], 12, [(w.double(), b.double()) for w, b in layers],
                    relus, 0, gmax=g_chain)
    assert g_chain.dtype == torch.float64
    wc, bc = R.collapse(*layers[0], *layers[1], *layers[2])
    g = R.pooled(x.double(), wc, bc)
    err = (g - g_chain).abs().max().item()
    print(f"F={F}: collapsed vs layered chain C in float64 {err:.3e} (|g3| <= {g_chain.abs().max().item():.3g})")
    assert err <= 1e-12
    assert torch.equal(g[:, F:], torch.zeros_like(g[:, F:]))  # the padding columns: zero weights, zero bias


@pytest.mark.parametrize("F", [64, 100, 768])
def test_fp32_form_is_within_its_bound(F):
    x, layers, _ = _chain_c(F)
    wc, bc = R.collapse(*layers[0], *layers[1], *layers[2])
    g64 = R.pooled(x.double(), wc, bc)
    g32 = R.pooled_fp32(x, wc, bc)
    err, lim = (g32.double() - g64).abs(), R.bound(x, wc, g64)
    worst = (err / lim.clamp_min(1e-300))[:, :F].max().item()
    print(f"F={F}: fp32 form vs float64 {err.max().item():.3e}, worst error / bound {worst:.3f}")
    assert bool((err <= lim).all())
    assert torch.equal(g32[:, F:], torch.zeros_like(g32[:, F:]))
