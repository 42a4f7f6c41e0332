"""Chain B's collapsed argument block through the C ABI (ndnet_pn_chain_run and
ndnet_pn_chain_run_t32): the head prologue, then the fold prologue with a
shared matrix (fold_ld = 0) and the folded layer's bias (fold_bias), layer 0 =
relu(x (W1f[b] M) + (b1 M + bM)), then 64 -> 128 and 128 -> 1024 split-bf16,
max-pooled -- against the same layers in float64 under tests/test_pn_chain.py's
bound (3 x torch-fp32's own error + 1e-6 x scale), what the head prologue
publishes included; and rows holding a NaN or an infinity against the layered
launch (conv1, the 64 -> 64 split-bf16 layer, ...) on the same inputs, with
small integer operands so that both forms are exact up to the first ReLU."""
import ctypes

import pytest
import torch

from test_pn_chain import BUILDS, F32, NAN_BITS, X6, _Case, _gen, _Head, _layer, _nd_rows, _ph

B = 3


def _attach_fold(ch, keep, b0, m, mb, flag=0):
    """Layer 0 keeps conv1's own bias b0; the prologue folds (m, mb) through it."""
    keep += [b0, m, mb]
    ch.L[0].bias, ch.L[0].bias_cloud_stride = b0.data_ptr(), 0
    ch.fold_t2, ch.fold_ld, ch.fold_bias, ch.x_nonfinite_nan = m.data_ptr(), 0, mb.data_ptr(), flag


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1, 63, 64, 65, 130])
def test_collapsed_chain_b_block(N):
    seed = 4100 + N
    g = _gen(seed)
    hd = _Head(g, B, 256, 12, 64)  # t1, W1f[b] = t1[b] @ basis in float64 (w_ref) and torch fp32 (w_t)
    b0, m, mb = torch.randn(64, generator=g) * 0.5, torch.randn(64, 64, generator=g) / 8.0, torch.randn(64, generator=g) * 0.5
    w_ref = hd.w_ref @ m.double()                                    # [B][16][64], rows 12..15 zero
    b_ref = b0.double() @ m.double() + mb.double()
    md = m.cuda()
    dev = (torch.matmul(hd.w_t, md), torch.addmv(mb.cuda(), md.t(), b0.cuda()))
    l0 = dict(wT=w_ref, b=b_ref, K=16, N=64, prec=F32, relu=1, fuse=False, dev=dev)
    layers = [l0, _layer(g, 64, 128, X6, 1), _layer(g, 128, 1024, X6, 1)]
    x = _nd_rows(B, N, g)
    c = _Case(x, 12, layers, 0)
    hd.attach(c)
    _attach_fold(c.ch, c.keep, b0.cuda(), md, mb.cuda())
    # the output, head_t1 and the published plain W1f[b] against float64, both builds
    hd.check(c, f"collapsed B N={N}")
    # ... and the publication bit for bit what the head prologue alone publishes
    alone = _Head(_gen(seed), B, 256, 12, 64)  # the same operands
    a = _Case(x, 12, [alone.layer0(_gen(1), 0), _layer(_gen(2), 64, 128, X6, 1), _layer(_gen(3), 128, 64, F32, 0)], 0)
    alone.attach(a)
    for entry in BUILDS:
        for h in (hd, alone):
            h.wbuf.view(torch.int32).fill_(NAN_BITS)
        c.run(entry)
        a.run(entry)
        assert torch.equal(hd.wbuf.view(torch.int32), alone.wbuf.view(torch.int32)), f"{entry}: published W1f differs"
        assert torch.equal(hd.t1.view(torch.int32), alone.t1.view(torch.int32))


def _launch(ch, entry, gmax):
    from ndnet import _lib
    gmax.fill_(float("-inf"))
    rc = getattr(_lib.lib(), entry)(ctypes.byref(ch), B, _lib.stream_ptr(gmax.device))
    assert rc == 0, f"{entry} returned {rc}"
    torch.cuda.synchronize()
    return gmax.cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("with_head", [True, False], ids=["head", "no-head"])
def test_nonfinite_rows_equal_the_layered_launch(with_head):
    """Rows with NaN, +inf and -inf in a mean column (1) and a covariance column (7), among finite rows, in
    two 64-point (three 32-point) tiles.  The layered launch is the reference: bit-equal pooled outputs.
    Integer operands keep both forms exact up to the first ReLU, and from there on they run the same
    layers on the same values.  The float64 model of it: such a row leaves that ReLU as zeros."""
    ph = _ph()
    N = 70
    g = _gen(4300 + with_head)
    ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=g).float()  # noqa: E731
    x = ri(-3, 3, B, N, 12)
    bad_rows = {}
    rows = iter([3, 17, 33, 47, 64, 69])
    for col in (1, 7):
        for v in (float("nan"), float("inf"), float("-inf")):
            r = next(rows)
            x[:, r, col] = v
            bad_rows[r] = (col, v)
    x[1, 5, 0], x[1, 5, 8] = float("inf"), float("-inf")  # two in one row, opposite signs
    bad = torch.zeros(B, N, dtype=torch.bool)
    bad[:, list(bad_rows)] = True
    bad[1, 5] = True
    # conv1 per cloud: through the head prologue (t1 = h2 @ w3^T + b3, W1f = t1 @ basis), or given
    h2 = ri(0, 2, B, 256) * (torch.rand(B, 256, generator=g) < 0.1)
    w3, b3 = ri(-1, 1, 9, 256), ri(-2, 2, 9)
    basis = ri(-1, 1, 9, 12 * 64) * (torch.rand(9, 12 * 64, generator=g) < 0.3)
    t1 = h2.double() @ w3.double().t() + b3.double()
    w1 = torch.nn.functional.pad((t1 @ basis.double()).view(B, 12, 64), (0, 0, 0, 4))  # [B][16][64] float64
    b0, m, mb = ri(-2, 2, 64), ri(-1, 1, 64, 64), ri(-3, 3, 64)
    tail = [(ri(-1, 1, 64, 128), ri(-2, 2, 128)), (ri(-1, 1, 128, 256) * (torch.rand(128, 256, generator=g) < 0.2),
                                                   ri(-2, 2, 256))]
    # float64: exactness up to the first ReLU, and the expected maxima
    xf = torch.where(bad[..., None], torch.zeros(()), x).double()
    y0 = torch.matmul(xf, w1[:, :12]) + b0.double()
    y1 = torch.matmul(y0, m.double()) + mb.double()
    wc = torch.matmul(w1[:, :12].abs(), m.double().abs())
    assert y0.abs().max() < 2 ** 24 and y1.abs().max() < 2 ** 24 and (3 * wc.sum(dim=1)).max() < 2 ** 24, "exact in fp32"
    h = torch.relu(y1)
    h[bad] = 0.0
    assert (torch.matmul(h, tail[0][0].double().abs()) + 2).max() < 2 ** 24
    h = torch.relu(torch.matmul(h, tail[0][0].double()) + tail[0][1].double())
    assert (torch.matmul(h, tail[1][0].double().abs()) + 2).max() < 2 ** 24  # every partial sum is an exact integer
    ref = (torch.matmul(h, tail[1][0].double()) + tail[1][1].double()).amax(dim=1)
    dev = lambda t: t.float().cuda()  # noqa: E731
    keep = [dev(t) for t in (x, h2, w3, b3, basis, b0, m, mb)]
    xd, h2d, w3d, b3d, basisd, b0d, md, mbd = keep
    w1f = ph._frag(w1.float()).cuda()  # [B][1024] (the head prologue overwrites it with the same values)
    t1d = torch.empty(B, 9, device="cuda")
    x6 = [(ph._frag_x6(w).cuda(), 0, dev(b), w.shape[0], w.shape[1], X6) for w, b in [(m, mb)] + tail]
    keep += [w1f, t1d, x6]
    conv1 = (w1f, 1024, b0d, 16, 64)
    outs = {}
    for form, layers, relus in (("layered", [conv1] + x6, (0, 1, 1, 0)), ("collapsed", [conv1] + x6[1:], (1, 1, 0))):
        gmax = torch.empty(B, 256, device="cuda")
        ch = ph._build_chain(N, 12, layers, relus, 0, gmax=gmax)
        ch.x = xd.data_ptr()
        if with_head:
            ch.head_h2, ch.head_ld, ch.head_K = h2d.data_ptr(), 256, 256
            ch.head_w3, ch.head_b3, ch.head_basis = w3d.data_ptr(), b3d.data_ptr(), basisd.data_ptr()
            ch.head_kin, ch.head_nout, ch.head_t1 = 12, 64, t1d.data_ptr()
        if form == "collapsed":
            _attach_fold(ch, keep, b0d, md, mbd, flag=1)
        outs[form] = [_launch(ch, entry, gmax) for entry in BUILDS]
    for i, entry in enumerate(BUILDS):
        lay, col = outs["layered"][i], outs["collapsed"][i]
        print(f"{entry[9:]}: layered vs float64 {(lay.double() - ref).abs().max().item():.3e}, "
              f"collapsed vs layered {(col - lay).abs().max().item():.3e}")
        assert torch.isfinite(lay).all(), "the layered launch drops the non-finite rows"
        assert torch.equal(col.view(torch.int32), lay.view(torch.int32)), f"{entry}: collapsed differs from layered"
        assert torch.equal(lay.double(), ref), f"{entry}: such a row leaves the first ReLU as zeros"
