"""NDTNetClassification: the reference module tree and numerics (CPU), and its
HIP eval forward (chains A-C, the head's two FC launches and
ndnet_pn_cls_head_run) against float64 (GPU).

Error criterion, on log-probabilities against a float64 ``forward_torch`` of a
deep copy: e(x) = max |log x - log p64| over every entry, and the HIP path is
as accurate as torch's fp32 composition:  e(hip) <= 3 e(torch fp32) + 1e-6
(the project's factor for summation order, test_model._forward_checked),
below the project's 1e-4, rows summing to 1 within 1e-5."""
import copy

import numpy as np
import pytest
import torch

from conftest import golden
from model_init import deterministic_state

TOL = 1e-4
FIXTURES = ["ndtnet_cls_F768_C512.npz", "ndtnet_cls_F64_C5.npz"]
SEG_JOBS = 82  # NDTNetSegmentation(3, 28, 768)'s fold jobs before the fold was split (counted on that commit)
SEG_KINDS = "3535353535535353535355353535353535330000000050005000411111111111122222222222111111"  # their kinds, in order


def _model(F, C, device="cpu"):
    from ndnet.models.ndtnet import NDTNetClassification
    m = NDTNetClassification(3, C, F)
    m.load_state_dict(deterministic_state(m.state_dict()))
    return m.to(device).eval()


def _e(p, p64):
    return (p.double().log() - p64.log()).abs().max().item()


def _copy64(m):
    """A float64 copy of the model as it is now.  Before its first HIP forward
    a deepcopy; after it a fresh model with the same state (the folded-weight
    cache holds ctypes argument blocks, which do not copy)."""
    from ndnet.models.ndtnet import NDTNetClassification
    if m._hip is None:
        return copy.deepcopy(m).double()
    twin = NDTNetClassification(m.point_dim, m.num_classes, m.feature_dim).to(next(m.parameters()).device)
    twin.load_state_dict(m.state_dict())
    return twin.double().eval()


def _ref64(m, p, c):
    with torch.no_grad():
        ref64 = _copy64(m).forward_torch(p.double(), c.double())
        e_t = _e(m.forward_torch(p, c), ref64)
    # no entry is left out, so every float64 probability must be one fp32 holds at full precision:
    # 1e-30 is far above fp32's smallest normal (1.2e-38).  The deterministic weights give >= 1e-11,
    # the peaked models (conv3 x 30) down to ~1e-20
    assert ref64.min().item() >= 1e-30
    return ref64, e_t


def _criterion(tag, out, ref64, e_t):
    assert out.shape == ref64.shape and out.dtype == torch.float32
    e_hip = _e(out, ref64)
    rows = (out.double().sum(dim=1) - 1).abs().max().item()
    print(f"{tag}: e_hip {e_hip:.3e} e_torch_fp32 {e_t:.3e} |row sum - 1| {rows:.1e} "
          f"peak {ref64.max().item():.4f} lowest {ref64.min().item():.2e}")
    assert e_hip <= 3 * e_t + 1e-6
    assert e_hip < TOL
    assert rows <= 1e-5
    return e_hip


# ---- no GPU ----

@pytest.mark.parametrize("name", FIXTURES)
def test_torch_forward_matches_reference_fixture(name):
    z = golden(name)
    m = _model(int(z["feature_dim"]), int(z["num_classes"]))
    with torch.no_grad():
        out = m(torch.from_numpy(z["points"]), torch.from_numpy(z["covs"])).numpy()
    assert np.array_equal(out, z["out_eval"])
    assert list(m.state_dict()) == [str(k) for k in z["state_keys"]]
    assert sum(p.numel() for p in m.parameters()) == int(z["param_count"])
    assert int(z["param_count"]) == {768: 3_427_209, 64: 2_844_238}[int(z["feature_dim"])]


@pytest.mark.parametrize("name", FIXTURES)
def test_folded_algebra_cpu(name):
    """The HIP path's folding (BN, t1, t2, the padded head), evaluated with torch ops."""
    from ndnet.models import pointnet_hip as ph
    z = golden(name)
    m = _model(int(z["feature_dim"]), int(z["num_classes"]))
    p, c = torch.from_numpy(z["points"]), torch.from_numpy(z["covs"])
    ref64, e_t = _ref64(m, p, c)
    with torch.no_grad():
        out = ph.classification_forward(m, p, c, chain=ph._chain_torch)
    _criterion(name, out, ref64, e_t)


@pytest.mark.parametrize("F,C", [(100, 40), (1024, 1000), (16, 1)])
def test_folded_algebra_cpu_other_widths(F, C):
    from ndnet.models import pointnet_hip as ph
    m = _model(F, C)
    assert ph.supports_classification(m)
    g = torch.Generator().manual_seed(F + C)
    p, c = torch.rand((2, 77, 3), generator=g) * 20 - 10, torch.randn((2, 77, 9), generator=g)
    ref64, e_t = _ref64(m, p, c)
    with torch.no_grad():
        out = ph.classification_forward(m, p, c, chain=ph._chain_torch)
    assert out.shape == (2, C, 1)
    _criterion(f"F={F} C={C}", out, ref64, e_t)


def test_dispatch_predicate_bounds():
    from ndnet.models import pointnet_hip as ph
    from ndnet.models.ndtnet import NDTNetClassification
    assert ph.supports_classification(NDTNetClassification(3, 1024, 1024))
    assert ph.supports_classification(NDTNetClassification(3, 1, 16))
    assert ph.supports_classification(NDTNetClassification())
    assert not ph.supports_classification(NDTNetClassification(3, 1025, 768))
    assert not ph.supports_classification(NDTNetClassification(3, 512, 1025))


@pytest.mark.parametrize("F,C", [(768, 512), (64, 5), (100, 40)])
def test_fold_jobs_cover_every_tensor_the_forward_reads(F, C):
    """Each job writes exactly its output tensor's elements, and every tensor
    the classification forward reads is either re-folded or a parameter's own
    storage (the head's conv1 / conv2 rows and biases, fc3)."""
    from ndnet.models import pointnet_hip as ph
    m = _model(F, C)
    W = ph._Folded(m)
    assert not W.seg and not hasattr(W, "D_tail") and not hasattr(W, "s1g")
    size = {0: lambda K, N, Kp, Np: Kp * Np, 1: lambda K, N, Kp, Np: Kp * Np, 2: lambda K, N, Kp, Np: 3 * Kp * Np,
            3: lambda K, N, Kp, Np: N * K, 4: lambda K, N, Kp, Np: 9 * K * N, 5: lambda K, N, Kp, Np: Np}
    outs = set()
    for kind, out, layer, bn, k0, K, Kp, Np, eye in W.jobs:
        N = layer.weight.shape[0]
        assert out.is_contiguous() and out.numel() == size[kind](K, N, Kp, Np)
        assert out.dtype == (torch.bfloat16 if kind == 2 else torch.float32)
        assert k0 + K <= layer.weight.shape[1] and (bn is None or bn.num_features == N)
        outs.add(id(out))
    assert len(outs) == len(W.jobs)
    storage = {t.data_ptr() for t in m.parameters()}
    layers = W.A + W.B_tail + [W.C_mid, W.C_tail]
    read = [w for w, _ in layers] + [b for _, b in layers] + [W.t1_basis, W.c1b, W.h3f, W.h3b]
    read += list(W.frag.values()) + list(W.frag6.values()) + list(W.fcf.values())
    for t in (W.t1, W.t2):
        read += [t[k] for k in ("f1", "c1", "f2", "c2", "f3", "c3")]
    for t in read:
        assert id(t) in outs or t.data_ptr() in storage
    for t in (W.h1w, W.h1b, W.h2w, W.h2b, W.h3w):  # aliases of the parameters: nothing to re-fold
        assert t.data_ptr() in storage
    # the head's three fragment-major weights and the padded bias are jobs of their own
    Cp = (C + 15) // 16 * 16
    assert W.h3f.numel() == 256 * Cp and W.h3b.numel() == Cp
    assert W.fcf[id(W.h1w)].numel() == (F + 15) // 16 * 16 * 512 and W.fcf[id(W.h2w)].numel() == 512 * 256
    for t in (W.h3f, W.h3b, W.fcf[id(W.h1w)], W.fcf[id(W.h2w)]):
        assert id(t) in outs


def test_segmentation_fold_jobs_are_unchanged():
    from ndnet.models import pointnet_hip as ph
    from ndnet.models.ndtnet import NDTNetSegmentation
    W = ph._Folded(NDTNetSegmentation(3, 28, 768).eval())
    assert len(W.jobs) == SEG_JOBS
    assert "".join(str(j[0]) for j in W.jobs) == SEG_KINDS


def test_precision_is_a_plain_attribute():
    from ndnet.models import pointnet_hip as ph
    from ndnet.models.ndtnet import NDTNetClassification
    m = NDTNetClassification(3, 512, 768)
    assert m.precision is None and m._hip is None
    keys, count = list(m.state_dict()), sum(p.numel() for p in m.parameters())
    m.precision = "bf16"
    assert list(m.state_dict()) == keys and not any("precision" in k for k in keys)
    assert sum(p.numel() for p in m.parameters()) == count == 3_427_209
    assert "precision" not in dict(m.named_buffers()) and "precision" not in dict(m.named_parameters())
    assert ph.model_precision(m) == "bf16"
    m.precision = None
    assert ph.model_precision(m) == ph.PRECISION
    m.precision = "x4"
    with pytest.raises(ValueError):
        ph.model_precision(m)


# ---- GPU ----

def _nd_inputs(B, N, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.rand((B, N, 3), device="cuda", generator=g) * 20 - 10,
            torch.randn((B, N, 9), device="cuda", generator=g))


def _forward_checked(monkeypatch, m, p, c, chains, torch_calls):
    """model(p, c) on both chain builds against a float64 forward_torch of a
    deep copy (test_model._forward_checked's scheme, on probabilities): which
    path a forward takes, the output's shape and type, the criterion above,
    and the same class wherever float64's top two log-probabilities are more
    than 2e-4 apart."""
    from ndnet.models import pointnet_hip as ph
    ref64, e_t = _ref64(m, p, c)
    count = {"chain": 0, "torch": 0}
    real_chain, real_torch = ph._run_chain, m.forward_torch

    def spy_chain(*a, **k):
        count["chain"] += 1
        return real_chain(*a, **k)

    def spy_torch(*a, **k):
        count["torch"] += 1
        return real_torch(*a, **k)

    monkeypatch.setattr(ph, "_run_chain", spy_chain)
    monkeypatch.setattr(m, "forward_torch", spy_torch)
    B, C = p.shape[0], m.num_classes
    top2 = ref64[:, :, 0].log().topk(2, dim=1).values if C > 1 else None
    for t32 in (False, True):
        monkeypatch.setattr(ph, "_use_t32", lambda b, n, d, f=t32: f)
        count.update(chain=0, torch=0)
        with torch.no_grad():
            out = m(p, c)
        assert (count["chain"], count["torch"]) == (chains, torch_calls)
        assert out.shape == (B, C, 1)
        _criterion("t32" if t32 else "t64", out, ref64, e_t)
        if top2 is not None:
            clear = (top2[:, 0] - top2[:, 1]) > 2 * TOL
            assert torch.equal(out[:, :, 0].argmax(1)[clear], ref64[:, :, 0].argmax(1)[clear])


@pytest.mark.gpu
@pytest.mark.parametrize("B,N", [(2, 77), (3, 130)])
@pytest.mark.parametrize("F,C", [(768, 512), (64, 5), (100, 40), (1024, 1000), (16, 1), (256, 17)])
def test_hip_forward_model_shapes(monkeypatch, F, C, B, N):
    """Three chain launches and no torch composition: the kernels run."""
    from ndnet.models import pointnet_hip as ph
    m = _model(F, C, "cuda")
    assert ph.supports_classification(m)
    _forward_checked(monkeypatch, m, *_nd_inputs(B, N, F + C + N), chains=3, torch_calls=0)


@pytest.mark.gpu
@pytest.mark.parametrize("B,N", [(2, 77), (3, 130)])
@pytest.mark.parametrize("F,C", [(768, 512), (64, 5)])
def test_hip_forward_peaked_distribution(monkeypatch, F, C, B, N):
    """conv3's weights x 30: peak probabilities 0.89 .. 0.9998 (0.004 and 0.36
    with the weights as they are), the lowest ones 1e-13 .. 1e-20."""
    m = _model(F, C, "cuda")
    with torch.no_grad():
        m.conv3.weight.mul_(30.0)
    _forward_checked(monkeypatch, m, *_nd_inputs(B, N, F + C + N), chains=3, torch_calls=0)


@pytest.mark.gpu
@pytest.mark.parametrize("F,C", [(768, 2000), (2048, 40)])
def test_hip_forward_outside_the_bounds(monkeypatch, F, C):
    """Widths the kernels do not take run the torch composition; nothing raises."""
    from ndnet.models import pointnet_hip as ph
    m = _model(F, C, "cuda")
    assert not ph.supports_classification(m)
    _forward_checked(monkeypatch, m, *_nd_inputs(3, 130, F + C), chains=0, torch_calls=1)


@pytest.mark.gpu
def test_head_rearms_the_max_pool_buffer():
    """A second forward on smaller inputs in the same workspace: a buffer that
    was not re-armed would keep the first forward's larger maxima."""
    m = _model(64, 5, "cuda")
    p1, c1 = _nd_inputs(3, 130, 11)
    p2, c2 = 0.1 * p1, 0.1 * c1
    ref64, e_t = _ref64(m, p2, c2)
    with torch.no_grad():
        m(p1, c1)
        (ws,) = m._hip["ws"].values()
        assert bool((ws.gbuf == float("-inf")).all())
        out = m(p2, c2)
        assert list(m._hip["ws"].values()) == [ws]
        assert bool((ws.gbuf == float("-inf")).all())
    _criterion("second forward", out, ref64, e_t)


@pytest.mark.gpu
def test_hip_forward_two_head_chunks(monkeypatch):
    """17 clouds: the head runs as two chunks (16 + 1) of every launch."""
    m = _model(64, 5, "cuda")
    _forward_checked(monkeypatch, m, *_nd_inputs(17, 40, 17), chains=3, torch_calls=0)


@pytest.mark.gpu
def test_hip_forward_on_ndt_rows():
    """End to end: ndt_preprocessing rows (views of one [B,k,12] block) into the model."""
    from ndnet.preprocessing.ndtnet_preprocessing import ndt_preprocessing
    from ndnet.synthetic import make_batch
    m = _model(768, 512, "cuda")
    pts = torch.from_numpy(make_batch("L", 4, 20_000)).cuda()
    p, c, _ = ndt_preprocessing(500, pts)
    assert not p.is_contiguous()
    pc, cc = p.contiguous(), c.contiguous()
    ref64, e_t = _ref64(m, pc, cc)
    with torch.no_grad():
        out = m(p, c)
    _criterion("ndt rows", out, ref64, e_t)


def _perturb(m, seed, versions=True, params=True):
    """Scales every parameter (``params``) and moves every BatchNorm's running
    statistics; ``versions=False`` writes through ``.data`` (no version bump:
    what a replayed training graph does to the weights)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    with torch.no_grad():
        for t in (list(m.parameters()) if params else []) + [b for b in m.buffers() if b.is_floating_point()]:
            d = t if versions else t.data
            d.mul_(1.0 + 0.05 * torch.randn(t.shape, device="cuda", generator=g))
            if t.dim() == 1:
                d.add_(0.01 * torch.rand(t.shape, device="cuda", generator=g))  # running_var stays > 0


@pytest.mark.gpu
@pytest.mark.parametrize("F,C", [(768, 512), (64, 5)])
def test_refold_in_place_equals_fresh_fold(F, C):
    from ndnet.models import pointnet_hip as ph
    m = _model(F, C, "cuda")
    p, c = _nd_inputs(3, 130, F + C)
    with torch.no_grad():
        before = m(p, c).clone()
    cache = m._hip
    W, ws = cache["W"], dict(cache["ws"])
    assert W.jobs is not None and len(W.jobs) > 60
    _perturb(m, 1)
    with torch.no_grad():
        out = m(p, c)
    assert m._hip is cache and cache["W"] is W and cache["ws"] == ws, "re-fold must be in place"
    fresh = ph._Folded(m)
    bad = []
    for j, f in zip(W.jobs, fresh.jobs):
        a, b = j[1], f[1]
        assert a.shape == b.shape and a.dtype == b.dtype and j[0] == f[0]
        if not torch.equal(a, b):
            bad.append((j[0], tuple(a.shape), (a.float() - b.float()).abs().max().item()))
    assert not bad, bad
    ref64, e_t = _ref64(m, p, c)
    _criterion("after the re-fold", out, ref64, e_t)
    assert _e(before, ref64) > 10 * TOL  # the old weights' output is somewhere else


@pytest.mark.gpu
def test_mode_switch_refolds():
    """A replayed training graph changes weights without bumping versions: the
    mode switch (train() -> eval()) marks the fold stale, so the next eval
    forward re-folds; without a mode switch the fold is kept
    (test_model.test_mode_switch_refolds_weights_changed_without_versions)."""
    m = _model(64, 5, "cuda")
    p, c = _nd_inputs(3, 130, 5)
    with torch.no_grad():
        first = m(p, c).clone()
        W = m._hip["W"]
        m.train()
        _perturb(m, 2, versions=False)
        m.eval()
        out = m(p, c).clone()
    assert m._hip["W"] is W
    ref64, e_t = _ref64(m, p, c)
    _criterion("after train() / eval()", out, ref64, e_t)
    assert _e(first, ref64) > 10 * TOL
    with torch.no_grad():
        # running statistics only: the weights the forward reads unfolded (the head's
        # conv1 / conv2, fc3: pointnet_hip._Folded keeps the parameters) would change it anyway
        _perturb(m, 3, versions=False, params=False)
        kept = m(p, c)   # no mode switch, no version bump: the previous fold
    assert torch.equal(kept, out)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["x3", "bf16"])
def test_reduced_modes_match_their_emulation(mode):
    from ndnet.models import pointnet_hip as ph
    from test_model_precision import _emulator
    m = _model(64, 5, "cuda")
    p, c = _nd_inputs(3, 77, 64 + 5 + 77)
    ref64, _ = _ref64(m, p, c)
    with torch.no_grad():
        default = m(p, c).clone()
        try:
            m.precision = mode
            out = m(p, c).clone()
            emu = ph.classification_forward(m, p, c, chain=_emulator(ph._folded(m)["W"], mode))
            m.precision = "x6"
            x6 = m(p, c).clone()
        finally:
            m.precision = None
        after = m(p, c).clone()
    assert out.shape == (3, 5, 1) and bool(torch.isfinite(out).all())
    e_hip, e_emu = _e(out, ref64), _e(emu, ref64)
    print(f"{mode}: e_hip {e_hip:.3e} e_emu {e_emu:.3e} (x6 {_e(x6, ref64):.3e})")
    assert e_hip <= 3 * e_emu + 1e-6
    if mode == "bf16":
        assert (out - x6).abs().max().item() > 1e-6
    assert torch.equal(after, default)


@pytest.mark.gpu
def test_graphed_classification_replays_the_eager_result():
    from ndnet.pipeline import GraphedSegmentation
    from ndnet.preprocessing.ndtnet_preprocessing import ndt_preprocessing
    from ndnet.synthetic import make_batch
    B, n, k = 2, 4096, 256
    m = _model(768, 512, "cuda")
    pts = torch.from_numpy(make_batch("U", B, n)).cuda()
    with torch.no_grad():
        p, c, _ = ndt_preprocessing(k, pts)
        eager = m(p, c).clone()
    g = GraphedSegmentation(m, k, B, n)
    out = g(pts).clone()
    assert out.shape == (B, 512, 1) and torch.equal(out, eager)
    with torch.no_grad():
        m.conv3.bias.add_(torch.linspace(-1, 1, 512, device="cuda"))  # in place: the next replay follows
        m.feature_extractor.conv2.weight.mul_(1.1)
    out2 = g(pts).clone()
    with torch.no_grad():
        eager2 = m(p, c).clone()
    assert torch.equal(out2, eager2) and not torch.equal(out2, out)


@pytest.mark.gpu
def test_pipelined_classification_steps_equal_sequential_batches():
    """test_pipelined_steps_equal_sequential_batches's scheme with a classifier."""
    from ndnet.pipeline import GraphedSegmentation, PipelinedSegmentation
    from ndnet.synthetic import make_batch
    m = _model(768, 512, "cuda")
    batches = [torch.from_numpy(make_batch("L", 4, 20_000, seed0=10 * i)).cuda() for i in range(3)]
    ref = GraphedSegmentation(m, 400, 4, 20_000)
    expect = [ref(b).clone() for b in batches]
    pipe = PipelinedSegmentation(m, 400, 4, 20_000)
    outs = []
    for b in batches + [batches[-1]]:
        pipe.points.copy_(b)
        outs.append(pipe.replay().clone())
    torch.cuda.synchronize()
    for i in range(3):
        assert expect[i].shape == (4, 512, 1)
        assert torch.equal(outs[i + 1], expect[i]), f"batch {i}"
    assert not torch.equal(expect[0], expect[1])
