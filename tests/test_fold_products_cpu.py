"""Chain C's composed tail (NDNET_PN_FOLD_PRODUCTS, ``pointnet_hip.FOLD_PRODUCTS``): W23 = W2'^T W3'^T
and b23 = b2' W3'^T + b3' as the fold keeps them, in float64 against the layered chain C of
``pointnet_hip._chain_torch`` (deterministic weights, and BatchNorm statistics moved away from
them); the host's restatement of an NDNET_FOLD_PROD job; which tensors are product jobs; the job
list rules of ``ndnet_pn_fold_prepare`` and the argument rules of ``ndnet_pn_pool12_tail_run`` on
host memory (nothing rejected is launched); and the ctypes mirror of the new struct fields and entry
point against include/ndnet_pointnet.h.  No GPU."""
import ctypes
import os
import re

import pytest
import torch

import pool12_ref as R
from model_init import deterministic_state

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ndnet_pointnet.h")


class _F64(torch.Tensor):
    """``_chain_torch`` takes its input with ``.float()``; this input stays float64."""

    def float(self):
        return self.as_subclass(torch.Tensor).double()


def _seg(F, perturb):
    from ndnet.models.ndtnet import NDTNetSegmentation
    m = NDTNetSegmentation(3, 5, F)
    m.load_state_dict(deterministic_state(m.state_dict()))
    if perturb:  # running statistics and affine terms of every BatchNorm, away from the deterministic ones
        g = torch.Generator().manual_seed(F + 1)
        with torch.no_grad():
            for mod in m.modules():
                if isinstance(mod, torch.nn.BatchNorm1d):
                    mod.running_mean.add_(0.3 * torch.randn(mod.running_mean.shape, generator=g))
                    mod.running_var.mul_(0.5 + torch.rand(mod.running_var.shape, generator=g))
                    mod.weight.mul_(1.0 + 0.2 * torch.randn(mod.weight.shape, generator=g))
                    mod.bias.add_(0.1 * torch.randn(mod.bias.shape, generator=g))
    return m.eval()


@pytest.mark.parametrize("perturb", [False, True], ids=["deterministic", "moved-statistics"])
@pytest.mark.parametrize("F", [64, 100, 768])
def test_composed_tail_equals_the_layered_chain_in_float64(F, perturb):
    from ndnet.models import pointnet_hip as ph
    B, N = 3, 77
    m = _seg(F, perturb)
    g = torch.Generator().manual_seed(F)
    p, c = torch.rand((B, N, 3), generator=g) * 20 - 10, torch.randn((B, N, 9), generator=g)
    with torch.no_grad():
        ph.segmentation_forward(m, p, c, chain=ph._chain_torch)  # fills the per-cloud folded conv1 (w1t2, b1t2)
    (ws,) = m._hip["ws"].values()
    W = ws.W
    in_cols, layers, relus, mode, _ = ws.specs[2]
    assert in_cols == 12 and mode == 0 and relus == (0, 0, 0) and len(layers) == 3
    Fp = ph._npad(F)
    assert W.W23.shape == (64, Fp) and W.b23.shape == (Fp,) and W.W23.dtype == W.b23.dtype == torch.float64
    x = torch.cat((p, c), dim=2).double()
    g_chain = torch.full((B, Fp), float("-inf"), dtype=torch.float64)
    ph._chain_torch(x.as_subclass(_F64), N, 12, [(w.double(), b.double()) for w, b in layers], relus, 0, gmax=g_chain)
    assert g_chain.dtype == torch.float64
    (w0, b0) = layers[0]
    wc = w0.double() @ W.W23               # [B, 12, Fp]
    bc = b0.double() @ W.W23 + W.b23       # [B, Fp]
    got = R.pooled(x, wc, bc)
    scale = g_chain.abs().max().item()
    err = (got - g_chain).abs().max().item()
    print(f"F={F} perturb={perturb}: composed tail vs layered chain C in float64 {err:.3e} (|g3| <= {scale:.3g})")
    assert err <= 1e-12 * max(scale, 1.0)
    assert torch.equal(got[:, F:], torch.zeros_like(got[:, F:]))  # the padding columns: zero weights, zero bias
    # ... and against the other association, the one ndnet_pn_pool12_run forms
    wc_l, bc_l = R.collapse(*layers[0], *layers[1], *layers[2])
    assert (wc - wc_l).abs().max().item() <= 1e-13 * max(wc_l.abs().max().item(), 1.0)
    assert (bc - bc_l).abs().max().item() <= 1e-13 * max(bc_l.abs().max().item(), 1.0)


def test_prod64_is_the_ascending_float64_sum():
    """``_prod64`` (the host's first fold of a product tensor) is an NDNET_FOLD_PROD job's arithmetic: the
    exact products summed in float64 with k ascending, the bias row last."""
    from ndnet.models import pointnet_hip as ph
    g = torch.Generator().manual_seed(3)
    a, rhs, bias = torch.randn((5, 37), generator=g), torch.randn((37, 48), generator=g), torch.randn(48, generator=g)
    want = torch.zeros((5, 48), dtype=torch.float64)
    for r in range(5):
        for n in range(0, 48, 7):
            acc = 0.0
            for k in range(37):
                acc = acc + float(a[r, k]) * float(rhs[k, n])  # Python floats: IEEE double, one rounding per operation
            want[r, n] = acc + float(bias[n])
    got = ph._prod64(a, rhs, bias)
    assert got.dtype == torch.float64 and got.shape == (5, 48)
    assert torch.equal(got[:, ::7], want[:, ::7])
    assert torch.equal(ph._prod64(a, rhs) + bias.double(), got)
    lim = 38 * 2.0 ** -53 * (a.double().abs() @ rhs.double().abs() + bias.double().abs())
    assert bool(((got - (a.double() @ rhs.double() + bias.double())).abs() <= lim).all())


def test_products_are_jobs_of_their_own():
    """The composed tail's two tensors are product jobs behind ``jobs`` (whose list stays as it was);
    the points-only baseline, which never runs the 12 -> F launch, has none."""
    from ndnet.models import pointnet_hip as ph
    from ndnet.models.pointnet import PointNetSegmentation
    W = ph._Folded(_seg(100, False))
    assert [id(p[0]) for p in W.products] == [id(W.W23), id(W.b23)]
    (o1, a1, r1, c1), (o2, a2, r2, c2) = W.products
    assert a1 is W.C_mid[0] and r1 is W.C_tail[0] and c1 is None
    assert a2 is W.c2b and r2 is W.C_tail[0] and c2 is W.C_tail[1]
    outs = {id(j[1]) for j in W.jobs}
    assert all(id(t) in outs for t in (a1, r1, a2, c2)), "every factor is itself re-folded"
    assert not any(id(p[0]) in outs for p in W.products) and all(j[0] <= 5 for j in W.jobs)
    m = PointNetSegmentation(3, 5, 64)
    m.load_state_dict(deterministic_state(m.state_dict()))
    Wb = ph._Folded(m.eval())
    assert Wb.products == [] and not hasattr(Wb, "W23")


# ---- the job list rules (ndnet_pn_fold_prepare is host code) ----

def _jobs(kinds, **edit):
    """A job list over host memory: kind 0 (WT) jobs of a 4 x 8 layer and kind 6 (PROD) jobs of 4 x 8 times 8 x 16."""
    from ndnet import _lib
    from ndnet.models import pointnet_hip as ph
    t = dict(w=torch.zeros(4, 8), rhs=torch.zeros(8, 16), bias=torch.zeros(16), out=torch.zeros(4, 16, dtype=torch.float64))
    arr = (ph._FoldJob * len(kinds))()
    for J, kind in zip(arr, kinds):
        J.kind, J.w, J.out, J.N, J.K, J.ld = kind, t["w"].data_ptr(), t["out"].data_ptr(), 4, 8, 8
        J.Kp, J.Np = (8, 16) if kind == 6 else (8, 4)
        if kind == 6:
            J.rhs, J.bias, J.out_f64 = t["rhs"].data_ptr(), t["bias"].data_ptr(), 1
            for k, v in edit.items():
                setattr(J, k, v)
    blocks = ctypes.c_int64(-1)
    rc = _lib.lib().ndnet_pn_fold_prepare(arr, len(arr), ctypes.byref(blocks))
    return rc, blocks.value, [J.block0 for J in arr], t


def test_prepare_takes_product_jobs_last_and_counts_their_blocks():
    rc, blocks, block0, _ = _jobs([0, 0, 6, 6])
    assert rc == 0 and block0 == [0, 1, 2, 3]
    assert blocks & 0xFFFFFFFF == 4 and blocks >> 32 == 2  # the list's workgroups, and the product jobs' among them
    rc, blocks, _, _ = _jobs([0, 0])
    assert rc == 0 and blocks == 2                        # no product job: the value is what it always was
    rc, blocks, _, _ = _jobs([6])
    assert rc == 0 and blocks & 0xFFFFFFFF == 1 and blocks >> 32 == 1


@pytest.mark.parametrize("case", ["a job of another kind behind a product", "rhs missing", "out_f64 = 2", "Np = 0",
                                  "a BatchNorm on a product", "K = 0", "ld < K"])
def test_prepare_rejects_invalid_product_jobs(case):
    one = torch.zeros(4)
    edits = {"rhs missing": dict(rhs=None), "out_f64 = 2": dict(out_f64=2), "Np = 0": dict(Np=0),
             "a BatchNorm on a product": dict(gamma=one.data_ptr(), beta=one.data_ptr(), mean=one.data_ptr(),
                                              var=one.data_ptr()),
             "K = 0": dict(K=0), "ld < K": dict(ld=7)}
    if case in edits:
        assert _jobs([0, 6], **edits[case])[0] == -20
    else:
        assert _jobs([6, 0])[0] == -20
    assert _jobs([0, 6])[0] == 0


def test_pool12_tail_invalid_arguments_are_rejected_before_any_launch():
    from ndnet import _lib
    buf = (ctypes.c_double * 16)()
    p = ctypes.addressof(buf)
    ok = dict(x=p, x_ld=12, n=10, w0f=p, w0_stride=1024, b0=p, b0_stride=64, w23=p, b23=p, Fp=128, gmax=p, gmax_ld=128,
              batch=2)
    bad = [dict(x=None), dict(w0f=None), dict(b0=None), dict(w23=None), dict(b23=None), dict(gmax=None), dict(x_ld=8),
           dict(x_ld=13), dict(n=0), dict(w0_stride=960), dict(b0_stride=32), dict(Fp=0), dict(Fp=100), dict(Fp=48),
           dict(gmax_ld=127), dict(batch=0), dict(batch=65536), dict(w23=p + 4), dict(b23=p + 4)]
    for edit in bad:
        a = {**ok, **edit}
        rc = _lib.lib().ndnet_pn_pool12_tail_run(a["x"], a["x_ld"], a["n"], a["w0f"], a["w0_stride"], a["b0"],
                                                 a["b0_stride"], a["w23"], a["b23"], a["Fp"], a["gmax"], a["gmax_ld"],
                                                 a["batch"], None)
        assert rc == -20, edit


# ---- the ctypes mirror against the header ----

def _header_text():
    with open(HEADER) as f:
        return re.sub(r"/\*.*?\*/", "", re.sub(r"//[^\n]*", "", f.read()), flags=re.S)


_SCALARS = dict(int32_t=ctypes.c_int32, int64_t=ctypes.c_int64, float=ctypes.c_float, int=ctypes.c_int)


def _ctype(decl):
    """The ctypes type of one C declarator's type part: any pointer is a c_void_p."""
    if "*" in decl:
        return ctypes.c_void_p
    return _SCALARS[decl.replace("const", "").split()[0]]


def test_fold_job_mirror_matches_the_header():
    from ndnet.models import pointnet_hip as ph
    text = _header_text()
    body = re.search(r"typedef\s+struct\s+ndnet_pn_fold_job\s*\{(.*?)\}\s*ndnet_pn_fold_job\s*;", text, re.S).group(1)
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        ctype, names = re.fullmatch(r"((?:const\s+)?\w+)\s*(.*)", decl, re.S).groups()
        for name in (n.strip() for n in names.split(",")):
            fields.append((name.lstrip("* "), ctypes.c_void_p if name.startswith("*") else _SCALARS[ctype]))
    assert fields == list(ph._FoldJob._fields_)
    names = [f[0] for f in fields]
    assert names[-4:] == ["block0", "rhs", "out_f64", "reserved1"], "the new fields follow the released ones"
    assert ph._FoldJob.rhs.offset == ph._FoldJob.block0.offset + 8
    assert ctypes.sizeof(ph._FoldJob) == ph._FoldJob.rhs.offset + 16
    kinds = {k: int(v) for k, v in re.findall(r"#define\s+(NDNET_FOLD_\w+)\s+(\d+)\s*$", text, re.M)}
    assert kinds["NDNET_FOLD_PROD"] == 6 and sorted(kinds.values()) == list(range(7))


def test_pool12_tail_binding_matches_the_header():
    from ndnet import _lib
    text = _header_text()
    protos = {}
    for name in ("ndnet_pn_pool12_run", "ndnet_pn_pool12_tail_run"):
        ret, args = re.search(r"(\w+)\s+%s\s*\((.*?)\)\s*;" % name, text, re.S).groups()
        protos[name] = (ret, [a.strip() for a in args.split(",")])
    ret, args = protos["ndnet_pn_pool12_tail_run"]
    fn = getattr(_lib.lib(), "ndnet_pn_pool12_tail_run")
    assert ret == "int" and fn.restype is ctypes.c_int
    assert [_ctype(a.rsplit(None, 1)[0] + ("*" if "*" in a else "")) for a in args] == list(fn.argtypes)
    arg_names = [a.replace("*", " ").split()[-1] for a in args]
    assert arg_names == ["x", "x_ld", "num_points", "w0f", "w0_stride", "b0", "b0_stride", "w23", "b23", "Fp", "gmax",
                         "gmax_ld", "batch", "stream"]
    # the layered entry keeps its arguments
    old = [a.replace("*", " ").split()[-1] for a in protos["ndnet_pn_pool12_run"][1]]
    assert old == ["x", "x_ld", "num_points", "w0f", "w0_stride", "b0", "b0_stride", "w_mid", "b_mid", "w_tail", "b_tail",
                   "F", "Fp", "gmax", "gmax_ld", "batch", "stream"]
    assert len(_lib.lib().ndnet_pn_pool12_run.argtypes) == len(old)
