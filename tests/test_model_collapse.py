"""Both eval forwards with chain B's first two layers collapsed into one
per-cloud 12 -> 64 layer and chain D's into one 12 -> 512 layer
(NDNET_PN_COLLAPSE=1, the default) and layered (NDNET_PN_COLLAPSE=0): against
each other and torch's fp32 composition, which settings take which launch,
the launch counts, the layered launch against the
output recorded before the collapse existed, an in-place re-fold, a captured
graph and two workspace slots on two streams.  Tolerance: tests/test_model.py's
TOL and its margin-aware argmax."""
import os

import numpy as np
import pytest
import torch

from model_init import deterministic_state

TOL = 1e-4
SHAPES = [(3, 77, 64), (16, 1000, 768)]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _model(kind, F, device="cuda", seg_classes=28):
    from ndnet.models.ndtnet import NDTNetClassification, NDTNetSegmentation
    m = NDTNetSegmentation(3, seg_classes, F) if kind == "seg" else NDTNetClassification(3, 40, F)
    m.load_state_dict(deterministic_state(m.state_dict()))
    return m.to(device).eval()


def _inputs(B, N, seed):
    g = torch.Generator().manual_seed(seed)  # on the CPU: the recorded outputs depend on these bits
    return ((torch.rand((B, N, 3), generator=g) * 20 - 10).cuda(), torch.randn((B, N, 9), generator=g).cuda())


def _scores(kind, out):
    return out if kind == "seg" else out[:, :, 0]


def _spy(monkeypatch):
    """Counts the per-point launches and keeps the argument blocks they were given, in launch order."""
    from ndnet.models import pointnet_hip as ph
    seen = {"chain": 0, "pool12": 0, "blocks": []}
    real_chain, real_pool = ph._run_chain, ph._run_pool12

    def spy_chain(blk, *a, **k):
        seen["chain"] += 1
        seen["blocks"].append(blk)
        return real_chain(blk, *a, **k)

    def spy_pool(*a, **k):
        seen["pool12"] += 1
        return real_pool(*a, **k)

    monkeypatch.setattr(ph, "_run_chain", spy_chain)
    monkeypatch.setattr(ph, "_run_pool12", spy_pool)
    return seen


def _chain_b_is_collapsed(seen):
    """Chain B is the forward's second per-point launch: three layers behind a fold prologue, or four."""
    blk = seen["blocks"][1]
    collapsed = blk.num_layers == 3
    assert collapsed or blk.num_layers == 4
    assert bool(blk.fold_t2) == collapsed and bool(blk.fold_bias) == collapsed and blk.x_nonfinite_nan == int(collapsed)
    assert blk.L[0].relu == int(collapsed)
    return collapsed


def _chain_d_is_collapsed(seen):
    """Chain D is a segmentation forward's fourth per-point launch: 12 -> 512 fused into 512 -> 256 and two
    more layers, or conv1 first (five layers)."""
    blk = seen["blocks"][3]
    collapsed = blk.num_layers == 4
    assert collapsed or blk.num_layers == 5
    assert blk.L[0].fuse_next == int(collapsed) and blk.L[1].fuse_next == int(not collapsed)
    assert blk.L[0].N == (512 if collapsed else 64) and blk.x_nonfinite_nan == int(collapsed) and blk.mode == 1
    return collapsed


@pytest.mark.gpu
@pytest.mark.parametrize("B,N,F", SHAPES)
@pytest.mark.parametrize("kind", ["seg", "cls"])
def test_collapsed_and_layered_agree(monkeypatch, kind, B, N, F):
    from ndnet.models import pointnet_hip as ph
    p, c = _inputs(B, N, B + N + F)
    seen = _spy(monkeypatch)
    outs = {}
    for collapse in (True, False):
        monkeypatch.setattr(ph, "COLLAPSE", collapse)
        m = _model(kind, F)  # a fresh model: argument blocks are cached per model
        seen.update(chain=0, pool12=0, blocks=[])
        with torch.no_grad():
            outs[collapse] = m(p, c)
        assert (seen["chain"], seen["pool12"]) == (4 if kind == "seg" else 3, 1), "the launch counts do not change"
        assert _chain_b_is_collapsed(seen) == collapse
        assert kind == "cls" or _chain_d_is_collapsed(seen) == collapse
    with torch.no_grad():
        ref = m.forward_torch(p, c)
    top2 = _scores(kind, ref).topk(2, dim=-1).values
    clear = (top2[..., 0] - top2[..., 1]) > 2 * TOL
    d = (outs[True] - outs[False]).abs().max().item()
    print(f"{kind} B={B} N={N} F={F}: collapsed vs layered {d:.3e}, vs torch fp32 "
          f"{(outs[True] - ref).abs().max().item():.3e} / {(outs[False] - ref).abs().max().item():.3e}")
    assert d < TOL
    for out in outs.values():
        assert out.shape == ref.shape and (out - ref).abs().max().item() < TOL
        assert torch.equal(_scores(kind, out).argmax(-1)[clear], _scores(kind, ref).argmax(-1)[clear])


@pytest.mark.gpu
@pytest.mark.parametrize("setting", ["x6", "x3", "bf16", "fp32", "COLLAPSE=0", "FOLD_T2=chain", "HEAD3=kernel"])
def test_which_settings_collapse(monkeypatch, setting):
    """Only the x6 mode collapses (the others are defined layer by layer, or keep every layer on the fp32
    MFMA); NDNET_PN_FOLD_T2=chain keeps chain D layered (chain C's prologue publishes its layer 0) and
    leaves chain B's collapse in effect; so does NDNET_PN_HEAD3=kernel, for both chains (chain B's fold
    prologue then runs alone)."""
    from ndnet.models import pointnet_hip as ph
    p, c = _inputs(3, 77, 5)
    seen = _spy(monkeypatch)
    m = _model("seg", 64)
    if setting in ph.MODES:
        m.precision = setting
    elif setting == "COLLAPSE=0":
        monkeypatch.setattr(ph, "COLLAPSE", False)
    elif setting == "FOLD_T2=chain":
        monkeypatch.setattr(ph, "FOLD_T2_KERNEL", False)
    else:
        monkeypatch.setattr(ph, "HEAD3_IN_CHAIN", False)
    with torch.no_grad():
        out = m(p, c)
        ref = m.forward_torch(p, c)
    assert _chain_b_is_collapsed(seen) == (setting in ("x6", "FOLD_T2=chain", "HEAD3=kernel"))
    assert _chain_d_is_collapsed(seen) == (setting in ("x6", "HEAD3=kernel"))
    assert bool(seen["blocks"][1].head_h2) == (setting != "HEAD3=kernel")
    if setting not in ("x3", "bf16"):  # (the reduced modes' accuracy: tests/test_model_precision.py)
        assert (out - ref).abs().max().item() < TOL


@pytest.mark.gpu
def test_many_classes_keep_chain_d_layered(monkeypatch):
    """Past 256 padded classes the collapsed chain D's logits and 256-wide planes no longer share an LDS
    region of the 64-point build: chain D stays layered, chain B collapses."""
    from ndnet.models.ndtnet import NDTNetSegmentation
    seen = _spy(monkeypatch)
    m = NDTNetSegmentation(3, 300, 64)
    m.load_state_dict(deterministic_state(m.state_dict()))
    m = m.cuda().eval()
    p, c = _inputs(3, 77, 13)
    with torch.no_grad():
        out = m(p, c)
        ref = m.forward_torch(p, c)
    assert _chain_b_is_collapsed(seen) and not _chain_d_is_collapsed(seen)
    assert (out - ref).abs().max().item() < TOL


@pytest.mark.gpu
def test_baseline_keeps_the_layered_chain(monkeypatch):
    """The points-only baseline's conv1 is a shared layer on transformed points: nothing to collapse."""
    from ndnet.models.pointnet import PointNetSegmentation
    seen = _spy(monkeypatch)
    m = PointNetSegmentation(3, 28, 64)
    m.load_state_dict(deterministic_state(m.state_dict()))
    m = m.cuda().eval()
    p, _ = _inputs(3, 77, 12)
    with torch.no_grad():
        out = m(p)
        ref = m.forward_torch(p)
    assert not _chain_b_is_collapsed(seen)
    assert (out - ref).abs().max().item() < TOL


# The recorded outputs: (3, 77) runs every chain on the 32-point build; (65, 65) has 130 tiles of 64 points,
# past the 32-point build's limit on a 256-CU device, so the 64-point k_pn_chain runs (the build of the
# benchmark's shape), and its 65 clouds give ndnet_pn_fc_mfma_run four full groups of 16 and one of one.
# The wide one has 5 classes: 100 KB.
RECORDED = {"t32": (3, 77, 21, 28, ""), "t64": (65, 65, 22, 5, "64_")}


@pytest.mark.gpu
@pytest.mark.parametrize("build", sorted(RECORDED))
@pytest.mark.parametrize("kind", ["seg", "cls"])
def test_layered_launch_equals_the_recorded_output(monkeypatch, kind, build):
    """NDNET_PN_COLLAPSE=0 is the forward as it was: bit for bit the output recorded from the commit
    before the collapse (tests/golden/collapse_parent_[64_]<kind>.npy; inputs and weights as built here),
    on either tile build."""
    from ndnet.models import pointnet_hip as ph
    B, N, seed, classes, tag = RECORDED[build]
    monkeypatch.setattr(ph, "COLLAPSE", False)
    entries = []
    real = ph._run_chain

    def spy(blk, x, *a, **k):
        entries.append(ph._use_t32(x.shape[0], x.shape[1], x.device))
        return real(blk, x, *a, **k)

    monkeypatch.setattr(ph, "_run_chain", spy)
    p, c = _inputs(B, N, seed)
    m = _model(kind, 64, seg_classes=classes)
    with torch.no_grad():
        out = m(p, c).cpu().numpy()
    assert entries and all(e == (build == "t32") for e in entries), "the shape no longer selects this build"
    want = np.load(os.path.join(GOLDEN, f"collapse_parent_{tag}{kind}.npy"))
    assert out.shape == want.shape and out.dtype == want.dtype
    assert np.array_equal(out.view(np.int32), want.view(np.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["seg", "cls"])
def test_refold_in_place_is_followed(monkeypatch, kind):
    """Weights and running statistics changed, re-folded in place by ndnet_pn_fold_run: the same argument
    block, and chain B's prologue and ndnet_pn_fold_seg_run compose the new weights (no product is kept)."""
    p, c = _inputs(3, 200, 7)
    seen = _spy(monkeypatch)
    m = _model(kind, 100)
    with torch.no_grad():
        first = m(p, c).clone()
    assert _chain_b_is_collapsed(seen) and (kind == "cls" or _chain_d_is_collapsed(seen))
    blk, W, jobs = seen["blocks"][1], m._hip["W"], len(m._hip["W"].jobs)
    g = torch.Generator(device="cuda").manual_seed(8)
    with torch.no_grad():
        for t in list(m.parameters()) + [b for b in m.buffers() if b.is_floating_point()]:
            t.mul_(1.0 + 0.05 * torch.randn(t.shape, device="cuda", generator=g))
            if t.dim() == 1:
                t.add_(0.01 * torch.rand(t.shape, device="cuda", generator=g))  # running_var stays > 0
        seen.update(blocks=[])
        out = m(p, c)
        ref = m.forward_torch(p, c)
    assert m._hip["W"] is W and seen["blocks"][1] is blk and len(W.jobs) == jobs, "the re-fold must be in place"
    e_new, e_old = (out - ref).abs().max().item(), (first - ref).abs().max().item()
    print(f"{kind}: after the re-fold {e_new:.3e} from torch fp32; the forward before it {e_old:.3e}")
    assert e_new < TOL and e_old > 10 * TOL  # the old weights' output is not the new model's


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["seg", "cls"])
def test_captured_graph_replays_equal_to_eager(kind):
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


@pytest.mark.gpu
def test_two_workspace_slots_on_two_streams():
    """Two forwards with no order between them, each in its own workspace slot: the results of the same
    forwards run one after the other."""
    from ndnet.models import pointnet_hip as ph
    m = _model("seg", 64)
    ins = [_inputs(3, 77, 30), _inputs(3, 77, 31)]
    with torch.no_grad():
        want = [m(p, c).clone() for p, c in ins]
        for i, (p, c) in enumerate(ins):  # fold, workspaces and argument blocks of both slots
            with ph.workspace_slot(i):
                m(p, c)
        torch.cuda.synchronize()
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        got = [None, None]
        for i, (p, c) in enumerate(ins):
            with torch.cuda.stream(streams[i]), ph.workspace_slot(i):
                got[i] = m(p, c)
        torch.cuda.synchronize()
    for w, g in zip(want, got):
        assert torch.equal(w, g)
