"""Chain D with the seg head's conv1 collapsed into its first layer, piece by
piece at the C ABI: ndnet_pn_fold_seg_run (the per-cloud 12 -> N2 weights and
bias), ndnet_pn_fc_mfma_bias_run (the FC layer with a bias row per cloud), and
the chain block P = 16 -> N1 (prec 0, per-cloud weights and bias, ReLU,
fuse_next) into Q = N1 -> N2 split-bf16 -- the direct form of the 16-wave
64-point build at N2 = 256, the generic fused pair elsewhere -- against float64
under tests/test_pn_chain.py's bound (3 x torch-fp32's own error + 1e-6 x
scale), also with fewer input columns and with Q in the reduced split-bf16
modes; rows holding a NaN or an infinity against the layered launch; and the
-20 cases of both new entries on host memory."""
import ctypes
import math

import pytest
import torch

from test_pn_chain import (BUILDS, F32, NAN_BITS, X6, _Case, _gen, _kept, _layer, _nd_rows, _padded, _ph, _report,
                           _rows16, _sentinel)
from test_pn_precision import MODES as REDUCED_MODES
from test_pn_precision import _Case as _ReducedCase

ERR_ARG = -20


def _lib():
    from ndnet import _lib
    return _lib


# ---- ndnet_pn_fold_seg_run ----

@pytest.mark.gpu
@pytest.mark.parametrize("pads", [0, 1], ids=["tight", "padded"])
@pytest.mark.parametrize("N2", [64, 512])
@pytest.mark.parametrize("batch", [1, 3, 17])
def test_fold_seg_against_float64(batch, N2, pads):
    """outf / outb bit-equal to ndnet_pn_fold_t2_run's; wd[b] = (outf[b] as 12 x 64) s1aT and bd[b] = outb[b]
    s1aT + s1b against float64 from those fp32 values.  Strides with NaN pads, sentinel-filled outputs:
    only the documented elements are written (rows 12..15 of wd and every pad keep their bits)."""
    L, ph = _lib(), _ph()
    g = _gen(7000 + batch + N2 + pads)
    w1_stride, t2_ld, wd_stride, bd_stride = 1024 + 64 * pads, 4096 + 4 * pads, 16 * N2 + 32 * pads, N2 + 5 * pads
    w = torch.randn(batch, 12, 64, generator=g) / math.sqrt(12)
    b1, t2 = torch.randn(64, generator=g) * 0.5, torch.randn(batch, 64, 64, generator=g) / 8.0
    s1aT, s1b = torch.randn(64, N2, generator=g) / 8.0, torch.randn(N2, generator=g) * 0.5
    w16 = torch.full((batch, 16, 64), float("nan"))
    w16[:, :12] = w
    win, t2in = _padded(ph._frag(w16), w1_stride).cuda(), _padded(t2.view(batch, 4096), t2_ld).cuda()
    b1d, sd, sbd = b1.cuda(), s1aT.cuda(), s1b.cuda()
    outf, outb = _sentinel(batch * 1024 + 64), _sentinel(batch * 64 + 64)
    wd, bd = _sentinel(batch, wd_stride), _sentinel(batch, bd_stride)
    st = L.stream_ptr(win.device)
    rc = L.lib().ndnet_pn_fold_seg_run(win.data_ptr(), w1_stride, b1d.data_ptr(), t2in.data_ptr(), t2_ld, outf.data_ptr(),
                                       outb.data_ptr(), sd.data_ptr(), sbd.data_ptr(), N2, wd.data_ptr(), wd_stride,
                                       bd.data_ptr(), bd_stride, batch, st)
    assert rc == 0
    kf, kb = _sentinel(batch * 1024 + 64), _sentinel(batch * 64 + 64)
    rc = L.lib().ndnet_pn_fold_t2_run(win.data_ptr(), w1_stride, b1d.data_ptr(), t2in.data_ptr(), t2_ld, kf.data_ptr(),
                                      kb.data_ptr(), batch, st)
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(outf.view(torch.int32), kf.view(torch.int32)), "outf differs from ndnet_pn_fold_t2_run's"
    assert torch.equal(outb.view(torch.int32), kb.view(torch.int32)), "outb differs from ndnet_pn_fold_t2_run's"
    assert _kept(wd[:, 16 * N2:]) and _kept(bd[:, N2:]), "pads were written"
    rows = ph._frag(torch.arange(16.0)[:, None].expand(16, N2).contiguous())
    got_w = wd[:, : 16 * N2].cpu()
    assert _kept(got_w[:, rows >= 12]), "rows 12..15 of wd were written"
    # float64 from the fp32 values just written (outf holds them fragment-major: undo it through the row/column maps)
    cols = ph._frag(torch.arange(64.0)[None, :].expand(16, 64).contiguous()).long()
    r64 = _rows16(64).long()
    w1t2 = torch.zeros(batch, 16, 64)
    w1t2[:, r64, cols] = outf[: batch * 1024].view(batch, 1024).cpu()
    w1t2, b1t2 = w1t2[:, :12], outb[: batch * 64].view(batch, 64).cpu()
    assert torch.isfinite(w1t2).all() and torch.isfinite(b1t2).all()
    wd_ref = w1t2.double() @ s1aT.double()
    bd_ref = b1t2.double() @ s1aT.double() + s1b.double()
    e_w = (torch.matmul(w1t2.cuda(), sd).double().cpu() - wd_ref).abs().max().item()
    e_b = (torch.addmm(sbd, b1t2.cuda(), sd).double().cpu() - bd_ref).abs().max().item()
    bad, name = [], f"fold_seg batch={batch} N2={N2} pads={pads}"
    ref16 = torch.nn.functional.pad(wd_ref, (0, 0, 0, 4))
    _report(name + " wd", got_w[:, rows < 12].double(), ph._frag(ref16)[:, rows < 12], e_w, bad)
    _report(name + " bd", bd[:, :N2].double().cpu(), bd_ref, e_b, bad)
    assert not bad, bad
    # bit-identical from run to run
    wd2, bd2 = _sentinel(batch, wd_stride), _sentinel(batch, bd_stride)
    rc = L.lib().ndnet_pn_fold_seg_run(win.data_ptr(), w1_stride, b1d.data_ptr(), t2in.data_ptr(), t2_ld, outf.data_ptr(),
                                       outb.data_ptr(), sd.data_ptr(), sbd.data_ptr(), N2, wd2.data_ptr(), wd_stride,
                                       bd2.data_ptr(), bd_stride, batch, st)
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(wd.view(torch.int32), wd2.view(torch.int32)) and torch.equal(bd.view(torch.int32), bd2.view(torch.int32))


def _fold_seg_call(edit):
    L = _lib()
    shapes = dict(w1f=(2, 1024), b1=(64,), t2=(2, 4096), outf=(2, 1024), outb=(2, 64), s1aT=(64, 128), s1b=(128,),
                  wd=(2, 16 * 128), bd=(2, 128))
    t = {k: torch.zeros(*s) for k, s in shapes.items()}
    a = {k: v.data_ptr() for k, v in t.items()}
    a.update(w1_stride=1024, t2_ld=4096, N2=128, wd_stride=16 * 128, bd_stride=128, batch=2)
    edit(a)
    return L.lib().ndnet_pn_fold_seg_run(a["w1f"], a["w1_stride"], a["b1"], a["t2"], a["t2_ld"], a["outf"], a["outb"],
                                         a["s1aT"], a["s1b"], a["N2"], a["wd"], a["wd_stride"], a["bd"], a["bd_stride"],
                                         a["batch"], None)


FOLD_SEG_ARG_CASES = {f"NULL {k}": (lambda k: lambda a: a.update({k: None}))(k)
                      for k in ("w1f", "b1", "t2", "outf", "outb", "s1aT", "s1b", "wd", "bd")}
FOLD_SEG_ARG_CASES.update({
    "batch 0": lambda a: a.update(batch=0),
    "batch 65536": lambda a: a.update(batch=65536),
    "w1_stride < 1024": lambda a: a.update(w1_stride=1020),
    "t2_ld < 4096": lambda a: a.update(t2_ld=4092),
    "t2_ld % 4": lambda a: a.update(t2_ld=4098),
    "t2 misaligned": lambda a: a.update(t2=a["t2"] + 4),
    "s1aT misaligned": lambda a: a.update(s1aT=a["s1aT"] + 8),
    "N2 0": lambda a: a.update(N2=0),
    "N2 % 64": lambda a: a.update(N2=96),
    "wd_stride < 16 N2": lambda a: a.update(wd_stride=16 * 128 - 4),
    "bd_stride < N2": lambda a: a.update(bd_stride=127),
})


@pytest.mark.parametrize("case", sorted(FOLD_SEG_ARG_CASES))
def test_fold_seg_rejects_inconsistent_arguments(case):
    assert _fold_seg_call(FOLD_SEG_ARG_CASES[case]) == ERR_ARG


# ---- ndnet_pn_fc_mfma_bias_run ----

def _fc_bias_launch(x, wf, bias, bias_ld, batch, K, N, relu, entry="ndnet_pn_fc_mfma_bias_run"):
    L = _lib()
    out = _sentinel(batch, N + 3)
    args = (x.data_ptr(), x.stride(0), wf.data_ptr(), bias.data_ptr()) + ((bias_ld,) if "bias" in entry else ()) + \
        (out.data_ptr(), N + 3, batch, K, N, relu, L.stream_ptr(x.device))
    assert getattr(L.lib(), entry)(*args) == 0
    torch.cuda.synchronize()
    assert _kept(out[:, N:])
    return out[:, :N]


@pytest.mark.gpu
@pytest.mark.parametrize("batch", [1, 5, 16])
@pytest.mark.parametrize("K,N", [(64, 64), (768, 512), (112, 48)])
def test_fc_bias_rows(batch, K, N):
    """Stride 0 is ndnet_pn_fc_mfma_run bit for bit (column blocks per workgroup 1 and 4 by the dispatch
    rule); a bias row per cloud (rows of N + 8 floats, NaN pads) against float64."""
    ph = _ph()
    g = _gen(7100 + batch + K + N)
    x = torch.relu(torch.randn(batch, K, generator=g) + 1.0)
    w, b = torch.randn(N, K, generator=g) / math.sqrt(K), torch.randn(N, generator=g) * 0.5
    rows = torch.randn(batch, N, generator=g) * 0.5
    xd, wf = _padded(x, K + 4).cuda(), ph._frag(w.t().contiguous().cuda())
    for relu in (0, 1):
        old = _fc_bias_launch(xd, wf, b.cuda(), 0, batch, K, N, relu, entry="ndnet_pn_fc_mfma_run")
        new = _fc_bias_launch(xd, wf, b.cuda(), 0, batch, K, N, relu)
        assert torch.equal(old.view(torch.int32), new.view(torch.int32)), "stride 0 differs from ndnet_pn_fc_mfma_run"
        pre = x.double() @ w.double().t() + rows.double()
        ref = torch.relu(pre) if relu else pre
        t = torch.matmul(x.cuda(), w.cuda().t()) + rows.cuda()
        e_t = ((torch.relu(t) if relu else t).double().cpu() - ref).abs().max().item()
        got = _fc_bias_launch(xd, wf, _padded(rows, N + 8).cuda(), N + 8, batch, K, N, relu)
        bad = []
        _report(f"fc bias rows batch={batch} K={K} N={N} relu={relu}", got.double().cpu(), ref, e_t, bad)
        assert not bad, bad


def _fc_bias_call(edit):
    L = _lib()
    x, wf, b, out = (torch.zeros(*s) for s in ((2, 16), (16 * 32,), (2, 40), (2, 32)))
    a = dict(x=x.data_ptr(), ld_in=16, wf=wf.data_ptr(), b=b.data_ptr(), bias_ld=40, out=out.data_ptr(), ld_out=32,
             batch=2, K=16, N=32)
    edit(a)
    return L.lib().ndnet_pn_fc_mfma_bias_run(a["x"], a["ld_in"], a["wf"], a["b"], a["bias_ld"], a["out"], a["ld_out"],
                                             a["batch"], a["K"], a["N"], 0, None)


FC_BIAS_ARG_CASES = {
    "0 < bias_ld < N": lambda a: a.update(bias_ld=31),
    "bias_ld < 0": lambda a: a.update(bias_ld=-32),
    "NULL bias": lambda a: a.update(b=None),
    "NULL out": lambda a: a.update(out=None),
    "batch > 16": lambda a: a.update(batch=17),
    "K % 16": lambda a: a.update(K=8),
    "N % 16": lambda a: a.update(N=24),
    "ld_in < K": lambda a: a.update(ld_in=12),
    "ld_out < N": lambda a: a.update(ld_out=28),
    "in misaligned": lambda a: a.update(x=a["x"] + 4),
}


@pytest.mark.parametrize("case", sorted(FC_BIAS_ARG_CASES))
def test_fc_bias_rejects_inconsistent_arguments(case):
    assert _fc_bias_call(FC_BIAS_ARG_CASES[case]) == ERR_ARG


# ---- the chain block ----

B = 3


def _p_layer(g, N1, relu=1):
    """P: per-cloud W^T [B][16][N1] (12 rows used) and a bias row per cloud."""
    wT = torch.zeros(B, 16, N1)
    wT[:, :12] = torch.randn(B, 12, N1, generator=g) / math.sqrt(12)
    return dict(wT=wT, b=torch.randn(B, N1, generator=g) * 0.5, K=16, N=N1, prec=F32, relu=relu, fuse=True)


@pytest.mark.gpu
@pytest.mark.parametrize("N2", [64, 128, 256])
@pytest.mark.parametrize("N1", [64, 128, 512])
def test_chain_d_block(N1, N2):
    """P = 16 -> N1 (one, two and eight chunks) fused into Q = N1 -> N2 split-bf16, then N2 -> 64 split-bf16,
    pooled.  N2 = 256 takes the direct form in the 64-point build (no input tile), the others and the
    32-point build the generic fused pair.  Points 1, 40, 64, 65, 130."""
    for N in (1, 40, 64, 65, 130):
        g = _gen(7200 + N1 + N2 + N)
        layers = [_p_layer(g, N1), _layer(g, N1, N2, X6, 1), _layer(g, N2, 64, X6, 0)]
        c = _Case(_nd_rows(B, N, g), 12, layers, 0)
        assert c.ch.L[0].fuse_next == 1 and c.ch.L[0].w_cloud_stride == 16 * N1 and c.ch.L[0].bias_cloud_stride == N1
        c.check(f"chain D block N1={N1} N2={N2} N={N}")


@pytest.mark.gpu
@pytest.mark.parametrize("in_cols", [3, 7, 9])
def test_chain_d_block_fewer_input_columns(in_cols):
    """in_cols below 12, ending inside a 4-column piece of the row (3: the first piece, 7 and 9: later ones,
    the pieces past them not loaded): the input rows carry all 12 values and P all 12 weight rows, so a
    column past in_cols that is not zeroed shows against float64, which reads in_cols columns.  The direct
    form (N2 = 256, 64-point build) and the generic pair (32-point build), one tile and a tail."""
    for N in (40, 65):
        g = _gen(7400 + in_cols + N)
        layers = [_p_layer(g, 512), _layer(g, 512, 256, X6, 1), _layer(g, 256, 64, X6, 0)]
        x = _nd_rows(B, N, g)
        assert x[..., in_cols:].abs().min() > 0 and layers[0]["wT"][:, in_cols:12].abs().min() > 0
        _Case(x, in_cols, layers, 0).check(f"chain D block in_cols={in_cols} N={N}")


@pytest.mark.gpu
@pytest.mark.parametrize("prec", REDUCED_MODES)
def test_chain_d_block_reduced_modes(prec):
    """Q in the "x3" and "bf16" modes (ndnet_pn_layer.prec 2, 3; k_pn_chain<3>, <1>) behind the direct
    P = 16 -> 512: tests/test_pn_precision.py's float64 emulator and its two-sided bound, both builds."""
    g = _gen(7500 + prec)
    layers = [_layer(g, 16, 512, F32, 1, k_used=12, fuse=True), _layer(g, 512, 256, prec, 1), _layer(g, 256, 64, prec, 0)]
    _ReducedCase(_nd_rows(B, 77, g), 12, layers, 0).check(f"chain D block prec {prec}")


def _launch(ch, entry, gmax):
    L = _lib()
    gmax.fill_(float("-inf"))
    rc = getattr(L.lib(), entry)(ctypes.byref(ch), B, L.stream_ptr(gmax.device))
    assert rc == 0, f"{entry} returned {rc}"
    torch.cuda.synchronize()
    return gmax.cpu()


@pytest.mark.gpu
def test_nonfinite_rows_equal_the_layered_launch():
    """As tests/test_collapse_chain_b.py's: rows with NaN, +inf and -inf in a mean and in a covariance column.
    Layered: conv1 (16 -> 64 per cloud, no ReLU), 64 -> 512 split-bf16 with a bias row per cloud and ReLU
    fused into 512 -> 256, 256 -> 64.  Collapsed: 16 -> 512 on the fp32 MFMA with x_nonfinite_nan.  Integer
    operands: exact up to the first ReLU, the same layers on the same values after it -- bit-equal."""
    ph = _ph()
    N = 70
    g = _gen(7300)
    ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=g).float()  # noqa: E731
    x = ri(-3, 3, B, N, 12)
    bad = torch.zeros(B, N, dtype=torch.bool)
    rows = iter([3, 17, 33, 47, 64, 69])
    for col in (1, 7):
        for v in (float("nan"), float("inf"), float("-inf")):
            r = next(rows)
            x[:, r, col] = v
            bad[:, r] = True
    x[1, 5, 0], x[1, 5, 8] = float("inf"), float("-inf")
    bad[1, 5] = True
    w0 = torch.nn.functional.pad(ri(-4, 4, B, 12, 64), (0, 0, 0, 4))        # conv1 per cloud [B][16][64]
    b0 = ri(-3, 3, B, 64)
    s, cvec = ri(-1, 1, 64, 512), ri(-5, 5, B, 512)                          # the seg head's conv1[:, :64]^T, its bias rows
    tail = [(ri(-1, 1, 512, 256) * (torch.rand(512, 256, generator=g) < 0.1), ri(-2, 2, 256)),
            (ri(-1, 1, 256, 64) * (torch.rand(256, 64, generator=g) < 0.2), ri(-2, 2, 64))]
    wd = torch.matmul(w0.double(), s.double())                               # [B][16][512]
    bd = torch.matmul(b0.double()[:, None, :], s.double())[:, 0] + cvec.double()
    xf = torch.where(bad[..., None], torch.zeros(()), x).double()
    y0 = torch.matmul(xf, w0[:, :12].double()) + b0.double()[:, None, :]
    y1 = torch.matmul(y0, s.double()) + cvec.double()[:, None, :]
    assert max(y0.abs().max(), y1.abs().max(), 3 * wd.abs().sum(dim=1).max() + bd.abs().max()) < 2 ** 24, "exact in fp32"
    h = torch.relu(y1)
    h[bad] = 0.0
    assert (torch.matmul(h, tail[0][0].double().abs()) + 2).max() < 2 ** 24
    h = torch.relu(torch.matmul(h, tail[0][0].double()) + tail[0][1].double())
    assert (torch.matmul(h, tail[1][0].double().abs()) + 2).max() < 2 ** 24
    ref = (torch.matmul(h, tail[1][0].double()) + tail[1][1].double()).amax(dim=1)
    dev = lambda t: t.float().cuda()  # noqa: E731
    xd, b0d, cd, bdd = dev(x), dev(b0), dev(cvec), dev(bd)
    w0f, wdf = ph._frag(w0).cuda(), ph._frag(wd.float()).cuda()
    x6 = [(ph._frag_x6(w).cuda(), 0, dev(b), w.shape[0], w.shape[1], X6) for w, b in tail]
    p6 = (ph._frag_x6(s).cuda(), 0, cd, 64, 512, X6)
    forms = {"layered": ([(w0f, 1024, b0d, 16, 64), p6] + x6, (0, 1, 1, 0), (1,), 0),
             "collapsed": ([(wdf, 16 * 512, bdd, 16, 512)] + x6, (1, 1, 0), (0,), 1)}
    outs = {}
    for form, (layers, relus, fuse, flag) in forms.items():
        gmax = torch.empty(B, 64, device="cuda")
        ch = ph._build_chain(N, 12, layers, relus, 0, gmax=gmax, fuse=fuse)
        ch.x, ch.x_nonfinite_nan = xd.data_ptr(), flag
        outs[form] = [_launch(ch, entry, gmax) for entry in BUILDS]
    for i, entry in enumerate(BUILDS):
        lay, col = outs["layered"][i], outs["collapsed"][i]
        print(f"{entry[9:]}: layered vs float64 {(lay.double() - ref).abs().max().item():.3e}, "
              f"collapsed vs layered {(col - lay).abs().max().item():.3e}")
        assert torch.isfinite(lay).all(), "the layered launch drops the non-finite rows"
        assert torch.equal(col.view(torch.int32), lay.view(torch.int32)), f"{entry}: collapsed differs from layered"
        assert torch.equal(lay.double(), ref), f"{entry}: such a row leaves the first ReLU as zeros"
