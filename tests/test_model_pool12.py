"""Both eval forwards with chain C as one ``ndnet_pn_pool12_run``
(NDNET_PN_BACKBONE=pool12, the default) and as the layered chain
(NDNET_PN_BACKBONE=chain): against each other and torch's fp32 composition,
which launch each precision mode and glue setting takes, an in-place re-fold,
and a captured graph.  Tolerance: tests/test_model.py's TOL and its
margin-aware argmax."""
import pytest
import torch

from model_init import deterministic_state

TOL = 1e-4
SHAPES = [(3, 77, 64), (16, 1000, 768)]


def _model(kind, F, device="cuda"):
    from ndnet.models.ndtnet import NDTNetClassification, NDTNetSegmentation
    m = NDTNetSegmentation(3, 28, F) if kind == "seg" else NDTNetClassification(3, 40, F)
    m.load_state_dict(deterministic_state(m.state_dict()))
    return m.to(device).eval()


def _inputs(B, N, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.rand((B, N, 3), device="cuda", generator=g) * 20 - 10,
            torch.randn((B, N, 9), device="cuda", generator=g))


def _scores(kind, out):
    """[..., classes]: log-probs of the segmentation model, probabilities [B, C, 1] of the classification model."""
    return out if kind == "seg" else out[:, :, 0]


def _spy(monkeypatch):
    """Counts the launches of the Python wrappers: all per-point launches, and the 12 -> F ones among them."""
    from ndnet.models import pointnet_hip as ph
    count = {"chain": 0, "pool12": 0}
    real_chain, real_pool = ph._run_chain, ph._run_pool12

    def spy_chain(*a, **k):
        count["chain"] += 1
        return real_chain(*a, **k)

    def spy_pool(*a, **k):
        count["pool12"] += 1
        return real_pool(*a, **k)

    monkeypatch.setattr(ph, "_run_chain", spy_chain)
    monkeypatch.setattr(ph, "_run_pool12", spy_pool)
    return count


@pytest.mark.gpu
@pytest.mark.parametrize("B,N,F", SHAPES)
@pytest.mark.parametrize("kind", ["seg", "cls"])
def test_pool12_and_chain_backbones_agree(monkeypatch, kind, B, N, F):
    from ndnet.models import pointnet_hip as ph
    p, c = _inputs(B, N, B + N + F)
    count = _spy(monkeypatch)
    outs = {}
    for backbone in ("pool12", "chain"):
        monkeypatch.setattr(ph, "BACKBONE", backbone)
        m = _model(kind, F)  # a fresh model: argument blocks are cached per model
        count.update(chain=0, pool12=0)
        with torch.no_grad():
            outs[backbone] = m(p, c)
        assert count == {"chain": 4 if kind == "seg" else 3, "pool12": 1 if backbone == "pool12" else 0}
    with torch.no_grad():
        ref = m.forward_torch(p, c)
    top2 = _scores(kind, ref).topk(2, dim=-1).values
    clear = (top2[..., 0] - top2[..., 1]) > 2 * TOL
    d = (outs["pool12"] - outs["chain"]).abs().max().item()
    print(f"{kind} B={B} N={N} F={F}: pool12 vs chain {d:.3e}, vs torch fp32 "
          f"{(outs['pool12'] - ref).abs().max().item():.3e} / {(outs['chain'] - ref).abs().max().item():.3e}")
    assert d < TOL
    for out in outs.values():
        assert out.shape == ref.shape and (out - ref).abs().max().item() < TOL
        assert torch.equal(_scores(kind, out).argmax(-1)[clear], _scores(kind, ref).argmax(-1)[clear])


@pytest.mark.gpu
@pytest.mark.parametrize("mode,pool", [("x6", 1), ("fp32", 1), ("x3", 0), ("bf16", 0)])
def test_reduced_modes_keep_the_chain(monkeypatch, mode, pool):
    """x3 and bf16 are defined layer by layer (their emulation): they run the layered chain C."""
    p, c = _inputs(3, 77, 5)
    count = _spy(monkeypatch)
    m = _model("seg", 64)
    m.precision = mode
    with torch.no_grad():
        out = m(p, c)
        ref = m.forward_torch(p, c)
    assert count == {"chain": 4, "pool12": pool}
    if pool:  # (the reduced modes' accuracy: tests/test_model_precision.py)
        assert (out - ref).abs().max().item() < TOL


@pytest.mark.gpu
def test_fold_t2_in_the_chain_keeps_the_chain(monkeypatch):
    """NDNET_PN_FOLD_T2=chain: chain C's prologue publishes conv1 with t2 folded for chain D, so it must run."""
    from ndnet.models import pointnet_hip as ph
    monkeypatch.setattr(ph, "FOLD_T2_KERNEL", False)
    p, c = _inputs(3, 77, 6)
    count = _spy(monkeypatch)
    m = _model("seg", 64)
    with torch.no_grad():
        out = m(p, c)
        ref = m.forward_torch(p, c)
    assert count == {"chain": 4, "pool12": 0}
    assert (out - ref).abs().max().item() < TOL


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["seg", "cls"])
def test_refold_in_place_is_followed(monkeypatch, kind):
    """Weights and running statistics changed, re-folded in place by ndnet_pn_fold_run: the same argument
    block, and the next forward computes with the new weights (the kernel keeps no product of them)."""
    p, c = _inputs(3, 200, 7)
    count = _spy(monkeypatch)
    m = _model(kind, 100)
    with torch.no_grad():
        first = m(p, c).clone()
    (ws,) = m._hip["ws"].values()
    blk, W = ws.pool12, m._hip["W"]
    assert blk is not None
    g = torch.Generator(device="cuda").manual_seed(8)
    with torch.no_grad():
        for t in list(m.parameters()) + [b for b in m.buffers() if b.is_floating_point()]:
            t.mul_(1.0 + 0.05 * torch.randn(t.shape, device="cuda", generator=g))
            if t.dim() == 1:
                t.add_(0.01 * torch.rand(t.shape, device="cuda", generator=g))  # running_var stays > 0
        out = m(p, c)
        ref = m.forward_torch(p, c)
    assert m._hip["W"] is W and ws.pool12 is blk, "the re-fold must be in place"
    assert count["pool12"] == 2
    e_new, e_old = (out - ref).abs().max().item(), (first - ref).abs().max().item()
    print(f"{kind}: after the re-fold {e_new:.3e} from torch fp32; the forward before it {e_old:.3e}")
    assert e_new < TOL and e_old > 10 * TOL  # the old weights' output is not the new model's


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["seg", "cls"])
def test_captured_graph_replays_equal_to_eager(kind):
    """No allocation but the output and no synchronisation: the forward is captured, and a replay on new
    inputs gives the bits of the eager forward."""
    B, N = 3, 77
    m = _model(kind, 64)
    p, c = _inputs(B, N, 9)
    with torch.no_grad():
        m(p, c)  # fold, workspace and argument blocks
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = m(p, c)
        for seed in (10, 11):
            p2, c2 = _inputs(B, N, seed)
            p.copy_(p2)
            c.copy_(c2)
            g.replay()
            torch.cuda.synchronize()
            got = out.clone()
            assert torch.equal(got, m(p2, c2))
