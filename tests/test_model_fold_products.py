"""Both eval forwards with chain C's 12 -> F launch run from the fold's composed tail
(NDNET_PN_FOLD_PRODUCTS=1, the default) and from the layers (=0): the default against a float64
forward of the layered model, which settings take which entry point, =0 against the output
recorded from the commit before the composed tail existed, and the product tensors as jobs of the
device fold table -- their values against float64 products of the folded fp32 tensors, and an
in-place re-fold followed by them and by the next forward.

Shapes (tests/test_model_collapse.py's): (B, N) = (3, 77) runs every chain on the 32-point build,
(65, 65) on the 64-point build (130 tiles, five groups of clouds for the FC kernels); F = 64, 5
classes.  Bound (tests/test_pn_chain.py's): e_hip <= 3 e_t + 1e-6 * max |float64|, e_t the error of
torch's fp32 forward of the same model on the device; the arg-max must agree wherever float64's top
two are further apart than that bound."""
import copy
import os

import numpy as np
import pytest
import torch

from model_init import deterministic_state

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F, CLASSES = 64, 5
SHAPES = {"t32": (3, 77, 21), "t64": (65, 65, 22)}  # build: (B, N, input seed)


def model(kind, F=F, device="cuda"):
    from ndnet.models.ndtnet import NDTNetClassification, NDTNetSegmentation
    m = NDTNetSegmentation(3, CLASSES, F) if kind == "seg" else NDTNetClassification(3, CLASSES, F)
    m.load_state_dict(deterministic_state(m.state_dict()))
    return m.to(device).eval()


def inputs(B, N, seed):
    g = torch.Generator().manual_seed(seed)  # on the CPU: the recorded outputs depend on these bits
    return ((torch.rand((B, N, 3), generator=g) * 20 - 10).cuda(), torch.randn((B, N, 9), generator=g).cuda())


def _scores(kind, out):
    return out if kind == "seg" else out[:, :, 0]


def _spy(monkeypatch):
    """The per-point launches in order: the chain argument blocks, the 12 -> F blocks, and which tile build ran."""
    from ndnet.models import pointnet_hip as ph
    seen = {"chains": [], "pool12": [], "t32": []}
    real_chain, real_pool = ph._run_chain, ph._run_pool12

    def spy_chain(blk, x, *a, **k):
        seen["chains"].append(blk)
        seen["t32"].append(ph._use_t32(x.shape[0], x.shape[1], x.device))
        return real_chain(blk, x, *a, **k)

    def spy_pool(blk, *a, **k):
        seen["pool12"].append(blk)
        return real_pool(blk, *a, **k)

    monkeypatch.setattr(ph, "_run_chain", spy_chain)
    monkeypatch.setattr(ph, "_run_pool12", spy_pool)
    return seen


@pytest.mark.gpu
@pytest.mark.parametrize("build", sorted(SHAPES))
@pytest.mark.parametrize("kind", ["seg", "cls"])
def test_default_against_float64(monkeypatch, kind, build):
    B, N, seed = SHAPES[build]
    p, c = inputs(B, N, seed)
    m = model(kind)
    with torch.no_grad():
        ref64 = copy.deepcopy(m).double().forward_torch(p.double(), c.double())
        e_t = (m.forward_torch(p, c).double() - ref64).abs().max().item()
    seen = _spy(monkeypatch)
    with torch.no_grad():
        out = m(p, c)
    assert all(t == (build == "t32") for t in seen["t32"]), "the shape no longer selects this build"
    assert len(seen["chains"]) == (4 if kind == "seg" else 3) and len(seen["pool12"]) == 1
    assert seen["pool12"][0].tail, "the default runs ndnet_pn_pool12_tail_run"
    scale = ref64.abs().max().item()
    bound = 3 * e_t + 1e-6 * scale
    e_hip = (out.double() - ref64).abs().max().item()
    print(f"{kind} {build}: e_hip {e_hip:.3e} e_torch_fp32 {e_t:.3e} max|f64| {scale:.3g} bound {bound:.3e}")
    assert out.shape == ref64.shape and out.dtype == torch.float32
    assert e_hip <= bound
    s64 = _scores(kind, ref64)
    top2 = s64.topk(2, dim=-1).values
    clear = (top2[..., 0] - top2[..., 1]) > bound
    assert bool(clear.any())
    assert torch.equal(_scores(kind, out).argmax(-1)[clear], s64.argmax(-1)[clear])


SETTINGS = {  # setting -> (12 -> F launches, from the composed tail)
    "default": (1, True), "fp32": (1, True), "FOLD_PRODUCTS=0": (1, False), "x3": (0, False), "bf16": (0, False),
    "COLLAPSE=0": (1, False), "BACKBONE=chain": (0, False), "FOLD_T2=chain": (0, False), "HEAD3=kernel": (1, True),
}


@pytest.mark.gpu
@pytest.mark.parametrize("setting", sorted(SETTINGS))
def test_which_settings_run_the_composed_tail(monkeypatch, setting):
    from ndnet.models import pointnet_hip as ph
    p, c = inputs(3, 77, 5)
    seen = _spy(monkeypatch)
    m = model("seg")
    if setting in ph.MODES:
        m.precision = setting
    elif setting != "default":
        name, value = setting.split("=")
        attr = {"FOLD_T2": "FOLD_T2_KERNEL", "HEAD3": "HEAD3_IN_CHAIN"}.get(name, name)
        monkeypatch.setattr(ph, attr, {"0": False, "chain": "chain" if name == "BACKBONE" else False,
                                       "kernel": False}[value])
    with torch.no_grad():
        out = m(p, c)
        ref = m.forward_torch(p, c)
    launches, tail = SETTINGS[setting]
    assert len(seen["pool12"]) == launches and len(seen["chains"]) == 4
    assert [blk.tail for blk in seen["pool12"]] == [tail] * launches
    (ws,) = m._hip["ws"].values()
    assert ws.uses_tail() == tail
    if setting not in ("x3", "bf16"):  # (the reduced modes' accuracy: tests/test_model_precision.py)
        assert (out - ref).abs().max().item() < 1e-4


@pytest.mark.gpu
@pytest.mark.parametrize("build", sorted(SHAPES))
@pytest.mark.parametrize("kind", ["seg", "cls"])
def test_switched_off_equals_the_recorded_output(monkeypatch, kind, build):
    """NDNET_PN_FOLD_PRODUCTS=0 is the forward as it was: bit for bit the output recorded from the parent
    commit's build (tests/golden/fold_products_parent_<build>_<kind>.npy; inputs and weights as built here)."""
    from ndnet.models import pointnet_hip as ph
    B, N, seed = SHAPES[build]
    monkeypatch.setattr(ph, "FOLD_PRODUCTS", False)
    seen = _spy(monkeypatch)
    p, c = inputs(B, N, seed)
    m = model(kind)
    with torch.no_grad():
        out = m(p, c).cpu().numpy()
    assert seen["t32"] and all(t == (build == "t32") for t in seen["t32"]), "the shape no longer selects this build"
    assert [blk.tail for blk in seen["pool12"]] == [False]
    want = np.load(os.path.join(GOLDEN, f"fold_products_parent_{build}_{kind}.npy"))
    assert out.shape == want.shape and out.dtype == want.dtype
    assert np.array_equal(out.view(np.int32), want.view(np.int32))


def _products_checked(W, ph, label):
    """W23 and b23 against float64 products of the folded fp32 tensors they are made of: within the
    rounding of a 128-term float64 sum, and bit for bit the host's restatement of the job."""
    (w_mid, b_mid), (w_tail, b_tail) = W.C_mid, W.C_tail
    w64 = w_mid.double() @ w_tail.double()
    b64 = b_mid.double() @ w_tail.double() + b_tail.double()
    lim_w = 129 * 2.0 ** -53 * (w_mid.double().abs() @ w_tail.double().abs())
    lim_b = 130 * 2.0 ** -53 * (b_mid.double().abs() @ w_tail.double().abs() + b_tail.double().abs())
    e_w, e_b = (W.W23 - w64).abs(), (W.b23 - b64).abs()
    print(f"{label}: W23 off by {e_w.max().item():.3e}, b23 by {e_b.max().item():.3e} (|W23| <= {w64.abs().max().item():.3g})")
    assert bool((e_w <= lim_w).all()) and bool((e_b <= lim_b).all())
    assert torch.equal(W.W23, ph._prod64(w_mid, w_tail))
    assert torch.equal(W.b23, ph._prod64(b_mid[None, :], w_tail, b_tail).reshape(-1))
    assert torch.equal(W.W23[:, W.F:], torch.zeros_like(W.W23[:, W.F:])) and not bool(W.b23[W.F:].any())


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["seg", "cls"])
def test_refold_in_place_recomputes_the_products(monkeypatch, kind):
    """Parameters and running statistics changed in place: ndnet_pn_fold_run rewrites W23 and b23 (jobs of
    the device table, behind the tensors they multiply) in the same storage, the workspace and the argument
    block stay the objects they were, and the next forward computes with the new products."""
    from ndnet.models import pointnet_hip as ph
    p, c = inputs(3, 200, 7)
    seen = _spy(monkeypatch)
    m = model(kind, F=100)
    with torch.no_grad():
        first = m(p, c).clone()
    (ws,) = m._hip["ws"].values()
    W, blk = m._hip["W"], seen["pool12"][0]
    assert blk.tail and blk is ws.pool12 and W._dev_jobs is None, "the first fold is the host's"
    _products_checked(W, ph, f"{kind} first fold")
    ptrs = (W.W23.data_ptr(), W.b23.data_ptr())
    old_w23, old_b23 = W.W23.clone(), W.b23.clone()
    g = torch.Generator(device="cuda").manual_seed(8)
    with torch.no_grad():
        for t in list(m.parameters()) + [b for b in m.buffers() if b.is_floating_point()]:
            t.mul_(1.0 + 0.05 * torch.randn(t.shape, device="cuda", generator=g))
            if t.dim() == 1:
                t.add_(0.01 * torch.rand(t.shape, device="cuda", generator=g))  # running_var stays > 0
        out = m(p, c)
        ref = m.forward_torch(p, c)
    assert m._hip["W"] is W and W._dev_jobs is not None, "the re-fold must be the device table's, in place"
    assert list(m._hip["ws"].values()) == [ws] and ws.pool12 is blk and seen["pool12"] == [blk, blk]
    assert (W.W23.data_ptr(), W.b23.data_ptr()) == ptrs and blk.tensors[2] is W.W23 and blk.tensors[3] is W.b23
    assert W._dev_jobs.numel() == (len(W.jobs) + len(W.products)) * ph.ctypes.sizeof(ph._FoldJob)
    _products_checked(W, ph, f"{kind} re-fold")
    assert not torch.equal(W.W23, old_w23) and not torch.equal(W.b23, old_b23)
    e_new, e_old = (out - ref).abs().max().item(), (first - ref).abs().max().item()
    print(f"{kind}: after the re-fold {e_new:.3e} from torch fp32; the forward before it {e_old:.3e}")
    assert e_new < 1e-4 and e_old > 1e-3  # the old weights' output is not the new model's
    # a fresh fold of the changed model (the host's) holds the same bits as the device's re-fold
    fresh = ph._Folded(m)
    assert torch.equal(fresh.W23, W.W23) and torch.equal(fresh.b23, W.b23)


@pytest.mark.gpu
def test_captured_graph_replays_equal_to_eager():
    B, N = 3, 77
    m = model("seg")
    p, c = inputs(B, N, 9)
    with torch.no_grad():
        m(p, c)  # fold, workspace and argument blocks
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
