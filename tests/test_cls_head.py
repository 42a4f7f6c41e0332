"""ndnet_pn_cls_head_run at the C ABI: the classification head's last layer
and its softmax in one launch (include/ndnet_pointnet.h).

Error criterion, on log-probabilities against a float64 evaluation p64 of the
same inputs: e(x) = max |log x - log p64| over EVERY entry (the inputs keep
every float64 probability above 1e-11, far from fp32 underflow), and the
kernel must be as accurate as torch's fp32 addmm + softmax:
    e(hip) <= 3 e(torch fp32) + 1e-6
(the project's factor for summation order, tests/test_model.py).  Rows sum to
1 within 1e-5.  Logits: within 1e-5 max(1, |logit|max) of torch.addmm."""
import ctypes

import pytest
import torch

from test_code_objects import _code_objects, _kernel_meta

K = 256
SENTINEL = -7.0
SHAPES = [(16, 512), (1, 1), (5, 40), (3, 17), (7, 10), (16, 1000), (16, 1024), (17, 40), (33, 10)]


def _inputs(batch, C):
    g = torch.Generator().manual_seed(batch * 1000 + C)
    x = torch.relu(torch.randn(batch, K, generator=g))
    w = torch.randn(C, K, generator=g) * 4 / K ** 0.5
    b = torch.randn(C, generator=g)
    return x, w, b


_refs = {}


def _case(batch, C, shift=None):
    """Inputs on the GPU, the fragmented padded weights, float64 probabilities
    and torch's fp32 results of one case, computed once.  shift: None, "all"
    (bias += 100) or "one" (one class's bias set to +90)."""
    from ndnet.models import pointnet_hip as ph
    key = (batch, C, shift)
    if key not in _refs:
        x, w, b = _inputs(batch, C)
        if shift == "all":
            b = b + 100.0
        elif shift == "one":
            b = b.clone()
            b[C // 3] = 90.0
        N = (C + 15) // 16 * 16
        p64 = torch.softmax(torch.addmm(b.double(), x.double(), w.double().t()), dim=1)
        assert p64.min().item() >= 1e-11 or shift == "one"  # "one": see test_large_logits
        xd, wd, bd = x.cuda(), w.cuda(), b.cuda()
        lg32 = torch.addmm(bd, xd, wd.t())
        p32 = torch.softmax(lg32, dim=1)
        wf = ph._frag(ph._wT(wd, K, N))
        _refs[key] = dict(x=xd, wf=wf, bias=ph._bpad(bd, N), N=N, p64=p64, lg32=lg32.cpu(), p32=p32.cpu())
    return _refs[key]


def _run(z, batch, C, logits=True, clear=None, clear_count=0):
    """One launch into sentinel-filled buffers with ld = N + 8 and two spare rows."""
    from ndnet import _lib
    N = z["N"]
    probs = torch.full((batch + 2, N + 8), SENTINEL, device="cuda")
    lg = torch.full((batch + 2, N + 8), SENTINEL, device="cuda") if logits else None
    rc = _lib.lib().ndnet_pn_cls_head_run(z["x"].data_ptr(), z["x"].stride(0), z["wf"].data_ptr(), z["bias"].data_ptr(),
                                          probs.data_ptr(), probs.stride(0), lg.data_ptr() if logits else None,
                                          lg.stride(0) if logits else 0, batch, K, N, C,
                                          clear.data_ptr() if clear is not None else None, clear_count,
                                          _lib.stream_ptr(probs.device))
    assert rc == 0
    torch.cuda.synchronize()
    return probs.cpu(), (lg.cpu() if logits else None)


def _e(p, p64):
    return (p.double().log() - p64.log()).abs().max().item()


def _check_probs(tag, probs, z, batch, C):
    p = probs[:batch, :C]
    assert bool(torch.isfinite(p).all()) and bool((p >= 0).all())
    e_hip, e_t = _e(p, z["p64"]), _e(z["p32"], z["p64"])
    rows = (p.double().sum(dim=1) - 1).abs().max().item()
    print(f"{tag}: e_hip {e_hip:.3e} e_torch_fp32 {e_t:.3e} |row sum - 1| {rows:.1e} "
          f"peak {z['p64'].max().item():.4f} lowest {z['p64'].min().item():.2e}")
    assert e_hip <= 3 * e_t + 1e-6
    assert rows <= 1e-5
    # nothing past the classes or the batch is written
    assert bool((probs[:batch, C:] == SENTINEL).all()) and bool((probs[batch:] == SENTINEL).all())


# ---- no GPU: the built library ----

def test_argument_validation():
    """-20 before any launch (a launch without a GPU would give -21)."""
    from ndnet import _lib
    fn = _lib.lib().ndnet_pn_cls_head_run
    buf = (ctypes.c_float * 64)()
    a = ctypes.addressof(buf) // 16 * 16 + 16  # non-NULL, 16-byte aligned; never dereferenced

    def call(**kw):
        d = dict(inp=a, ld_in=256, wf=a, bias=a, probs=a, ld_probs=64, logits=None, ld_logits=0, batch=4, K=256,
                 N=48, out_cols=40, clear=None, clear_count=0)
        d.update(kw)
        return fn(d["inp"], d["ld_in"], d["wf"], d["bias"], d["probs"], d["ld_probs"], d["logits"], d["ld_logits"],
                  d["batch"], d["K"], d["N"], d["out_cols"], d["clear"], d["clear_count"], None)

    bad = [dict(inp=None), dict(wf=None), dict(bias=None), dict(probs=None), dict(K=8, ld_in=8),
           dict(K=272, ld_in=272), dict(N=1040, out_cols=1040, ld_probs=1040), dict(N=24, out_cols=20),
           dict(out_cols=0), dict(out_cols=49), dict(batch=0), dict(ld_in=252), dict(ld_probs=39),
           dict(logits=a, ld_logits=39), dict(inp=a + 4), dict(wf=a + 8), dict(ld_in=258),
           dict(clear=None, clear_count=5), dict(clear=a, clear_count=-1)]
    for kw in bad:
        assert call(**kw) == -20, kw


def test_code_object_has_no_scratch_or_spills(tmp_path):
    meta = {k: v for k, v in _kernel_meta(_code_objects(tmp_path)).items() if "k_pn_cls_head" in k}
    assert len(meta) == 1, sorted(meta)
    (m,) = meta.values()
    assert m["private_segment_fixed_size"] == 0
    assert m["vgpr_spill_count"] == 0


# ---- GPU ----

@pytest.mark.gpu
@pytest.mark.parametrize("batch,C", SHAPES)
def test_sweep(batch, C):
    z = _case(batch, C)
    probs, lg = _run(z, batch, C)
    bound = 1e-5 * max(1.0, z["lg32"].abs().max().item())
    d = (lg[:batch, :C] - z["lg32"]).abs().max().item()
    print(f"batch {batch} C {C}: |logits - addmm| {d:.2e} (bound {bound:.2e}), "
          f"logit range {(z['lg32'].max() - z['lg32'].min()).item():.1f}")
    assert d <= bound
    assert bool((lg[:batch, C:] == SENTINEL).all()) and bool((lg[batch:] == SENTINEL).all())
    _check_probs(f"batch {batch} C {C}", probs, z, batch, C)
    if C == 1:
        assert bool((probs[:batch, 0] == 1.0).all())
    again, none = _run(z, batch, C, logits=False)
    assert none is None and torch.equal(again, probs)  # logits = NULL: the same probabilities, bit for bit


@pytest.mark.gpu
@pytest.mark.parametrize("shift", ["all", "one"])
def test_large_logits(shift):
    """A softmax without the max subtraction overflows here (exp(100)).  With
    one class 90 above the rest the other float64 probabilities are 1e-42 ..
    1e-44, in fp32's denormal range: no entry is left out, so there the
    criterion holds the kernel to whatever torch's fp32 softmax keeps of them
    (a value flushed to 0 has an infinite log-probability error)."""
    z = _case(5, 40, shift)
    probs, lg = _run(z, 5, 40)
    assert lg[:5, :40].max().item() > 88.0
    _check_probs(f"large logits ({shift})", probs, z, 5, 40)


@pytest.mark.gpu
def test_clear():
    z = _case(5, 40)
    buf = torch.ones(5004, device="cuda")
    probs, _ = _run(z, 5, 40, clear=buf, clear_count=5003)
    assert bool((buf[:5003] == float("-inf")).all()) and buf[5003].item() == 1.0
    plain, _ = _run(z, 5, 40, clear=None, clear_count=0)
    assert torch.equal(plain, probs)
    # a range that starts off a 16-byte boundary, and one shorter than a float4
    buf = torch.ones(5004, device="cuda")
    _run(z, 5, 40, clear=buf[1:], clear_count=5002)
    assert buf[0].item() == 1.0 and bool((buf[1:5003] == float("-inf")).all()) and buf[5003].item() == 1.0
    buf = torch.ones(8, device="cuda")
    _run(z, 5, 40, clear=buf[2:], clear_count=3)
    assert buf.tolist() == [1.0, 1.0] + [float("-inf")] * 3 + [1.0] * 3
    # two workgroups share the range
    z = _case(17, 40)
    buf = torch.ones(5004, device="cuda")
    _run(z, 17, 40, clear=buf, clear_count=5003)
    assert bool((buf[:5003] == float("-inf")).all()) and buf[5003].item() == 1.0


@pytest.mark.gpu
def test_deterministic():
    z = _case(16, 512)
    a, la = _run(z, 16, 512)
    b, lb = _run(z, 16, 512)
    assert torch.equal(a, b) and torch.equal(la, lb)
