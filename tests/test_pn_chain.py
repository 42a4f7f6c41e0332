"""The fused point-MLP chain kernel (ndnet_pn_chain_run, ndnet_pn_chain_run_t32:
include/ndnet_pointnet.h) driven directly, layer shapes and argument blocks
the model never uses included, against the same layers evaluated in float64.

Bound of every comparison: with e_hip = max |HIP - float64| and e_t = the
error of ``pointnet_hip._chain_torch`` in fp32 on the same device against the
same float64 result,  e_hip <= 3 e_t + 1e-6 max |float64 result|  (the
factor covers summation order only; a split-bf16 layer that lost a plane sits
near 2^-16 relative).  Every case runs on both builds (64-point tiles, 16
waves; 32-point tiles, 8 waves).  Inputs are on the scale of NDT rows: means
within +-10, covariance entries of both signs spanning 1e-4 .. 60.  The two
optional prologues (head_*, fold_t2) are checked the same way, what they
publish included, with torch's fp32 addmm / matmul of the fold as e_t."""
import ctypes
import math

import pytest
import torch

BUILDS = ("ndnet_pn_chain_run", "ndnet_pn_chain_run_t32")
F32, X6 = 0, 1
NAN_BITS = 0x7FC0BEEF  # the sentinel of columns the kernel must not touch


def _ph():
    from ndnet.models import pointnet_hip as ph
    return ph


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _nd_rows(B, N, g, x_ld=12):
    """[B][N][x_ld] rows like ndt_preprocessing's: 3 means, then covariance entries."""
    x = torch.empty(B, N, x_ld)
    x[..., :3] = torch.rand(B, N, 3, generator=g) * 20 - 10
    mag = torch.exp(torch.rand(B, N, x_ld - 3, generator=g) * (math.log(60.0) - math.log(1e-4)) + math.log(1e-4))
    sign = (torch.rand(B, N, x_ld - 3, generator=g) < 0.5).float() * 2 - 1
    x[..., 3:] = mag * sign
    return x


def _layer(g, K, N, prec=F32, relu=1, k_used=None, n_used=None, fuse=False):
    """One layer: plain W^T [K][N] (rows past k_used and columns past n_used
    zero: the padding), random weights scaled by 1 / sqrt(k_used)."""
    k_used, n_used = k_used or K, n_used or N
    wT = torch.zeros(K, N)
    wT[:k_used, :n_used] = torch.randn(k_used, n_used, generator=g) / math.sqrt(k_used)
    b = torch.zeros(N)
    b[:n_used] = torch.randn(n_used, generator=g) * 0.5
    return dict(wT=wT, b=b, K=K, N=N, prec=prec, relu=relu, fuse=fuse)


def _ref64(x, in_cols, layers, mode, out_cols):
    """The chain in float64 (CPU): the padded weights, amax over the points
    (every row of x is a valid point), log_softmax over out_cols."""
    h = torch.nn.functional.pad(x[..., :in_cols].double(), (0, layers[0]["K"] - in_cols))
    for L in layers:
        w, b = L["wT"].double(), L["b"].double()
        h = torch.matmul(h, w) + (b[:, None, :] if b.dim() == 2 else b)
        if L["relu"]:
            h = torch.relu(h)
    return h.amax(dim=1) if mode == 0 else torch.log_softmax(h[..., :out_cols], dim=2)


class _Case:
    """Device operands, argument block and both references of one chain."""

    def __init__(self, x, in_cols, layers, mode, out_cols=0, gmax_extra=0):
        ph = _ph()
        self.x = x.cuda()
        self.mode, self.out_cols, self.layers = mode, out_cols, layers
        B, N, _ = x.shape
        self.B, self.N, self.n_last = B, N, layers[-1]["N"]
        self.ref = _ref64(x, in_cols, layers, mode, out_cols)
        # "dev": the layer as torch computes it in fp32 on the device, where wT / b are its float64 reference
        dev_layers = [L["dev"] if "dev" in L else (L["wT"].cuda(), L["b"].cuda()) for L in layers]
        # torch fp32 on the device
        if mode == 0:
            t = torch.full((B, self.n_last), float("-inf"), device="cuda")
            ph._chain_torch(self.x, N, in_cols, dev_layers, [L["relu"] for L in layers], 0, gmax=t)
        else:
            t = torch.empty((B, N, out_cols), device="cuda")
            ph._chain_torch(self.x, N, in_cols, dev_layers, [L["relu"] for L in layers], 1, out=t, out_cols=out_cols)
        self.e_t = (t.double().cpu() - self.ref).abs().max().item()
        self.scale = self.ref.abs().max().item()
        # the argument block
        self.keep, hip = [], []
        for L, (w, b) in zip(layers, dev_layers):
            if L["prec"] == X6:
                f = ph._frag_x6(w)
                stride = 0
            else:
                f = ph._frag(w)
                stride = f.stride(0) if f.dim() == 2 else 0
            self.keep += [f, b]
            hip.append((f, stride, b, L["K"], L["N"], L["prec"]))
        self.gmax_ld = self.n_last + gmax_extra
        self.gmax = torch.empty((B, self.gmax_ld), device="cuda") if mode == 0 else None
        self.out = torch.empty((B, N, out_cols), device="cuda") if mode == 1 else None
        self.ch = ph._build_chain(N, in_cols, hip, [L["relu"] for L in layers], mode, gmax=self.gmax,
                                  out_cols=out_cols, fuse=tuple(i for i, L in enumerate(layers) if L["fuse"]))
        self.ch.x, self.ch.x_ld = self.x.data_ptr(), self.x.stride(1)
        self.ch.out = self.out.data_ptr() if mode == 1 else None

    def run(self, entry):
        """One launch of `entry`; the result on the CPU in float64."""
        from ndnet import _lib
        if self.mode == 0:
            self.gmax.fill_(float("-inf"))
            if self.gmax_ld > self.n_last:
                self.gmax[:, self.n_last:].view(torch.int32).fill_(NAN_BITS)
        else:
            self.out.fill_(float("nan"))
        rc = getattr(_lib.lib(), entry)(ctypes.byref(self.ch), self.B, _lib.stream_ptr(self.x.device))
        assert rc == 0, f"{entry} returned {rc}"
        torch.cuda.synchronize()
        if self.mode == 0:
            if self.gmax_ld > self.n_last:
                extra = self.gmax[:, self.n_last:].view(torch.int32)
                assert bool((extra == NAN_BITS).all()), "columns past N of gmax were written"
            return self.gmax[:, : self.n_last].double().cpu()
        return self.out.double().cpu()

    def check(self, name, cols=None):
        """Both builds against float64 under the bound; `cols`: also per named
        column subset, each with its own scale and torch error (mode 0)."""
        bad = []
        for entry in BUILDS:
            got = self.run(entry)
            assert torch.isfinite(got).all(), f"{name} {entry}: non-finite output"
            e_hip = (got - self.ref).abs().max().item()
            bound = 3 * self.e_t + 1e-6 * self.scale
            print(f"{name} {entry[9:]}: e_hip {e_hip:.3e} e_t {self.e_t:.3e} scale {self.scale:.3e} "
                  f"ratio {e_hip / max(self.e_t, 1e-300):.2f}")
            if not e_hip <= bound:
                bad.append((name, entry, e_hip, self.e_t, self.scale))
            for cname, (idx, e_t_c) in (cols or {}).items():
                e_c = (got[:, idx] - self.ref[:, idx]).abs().max().item()
                s_c = self.ref[:, idx].abs().max().item()
                print(f"  {cname}: e_hip {e_c:.3e} e_t {e_t_c:.3e} scale {s_c:.3e}")
                if not e_c <= 3 * e_t_c + 1e-6 * s_c:
                    bad.append((name, entry, cname, e_c, e_t_c, s_c))
        assert not bad, bad


def _tail_chain(g, last_relu=1, zero_bias=False):
    """16 -> 64 (layer 0 on the VALU), 64 -> 128 x6, 128 -> 256 x6."""
    layers = [_layer(g, 16, 64, F32, 1, k_used=12), _layer(g, 64, 128, X6, 1), _layer(g, 128, 256, X6, last_relu)]
    if zero_bias:
        layers[0]["b"].zero_()
        layers[1]["b"].zero_()
    return layers


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 130])
def test_point_count_tails(N):
    """One tile, the tile boundaries of both builds, several tiles with a ragged tail."""
    g = _gen(100 + N)
    _Case(_nd_rows(3, N, g), 12, _tail_chain(g), 0).check(f"tails N={N}")


@pytest.mark.gpu
@pytest.mark.parametrize("N", [17, 65])
def test_pool_negative_and_mixed_sign_maxima(N):
    """The pool epilogue's float atomic max (signed max / unsigned min) and its
    row masking, isolated: no ReLU on the pooled layer; every third column has
    a bias of -50 (its maximum over the points is negative), another third a
    bias of 0 and tiny one-signed weights on the ReLU'd input (maxima within
    1e-3 of 0, of both signs).  Layers 0 and 1 have no bias, so a padded row of
    the tail tile is exactly `bias` in the pooled layer: above every real row
    of the tiny negative columns, and it must not win.  gmax has 64 more
    columns than the layer; they keep their bits."""
    g = _gen(200 + N)
    layers = _tail_chain(g, last_relu=0, zero_bias=True)
    wT, b = layers[2]["wT"], layers[2]["b"]
    neg, tiny, rest = (torch.arange(c, 256, 3) for c in (0, 1, 2))
    b[neg] = -50.0
    b[tiny] = 0.0
    csign = (torch.arange(tiny.numel()) % 2).float() * 2 - 1
    wT[:, tiny] = wT[:, tiny].abs() * 2e-6 * csign
    c = _Case(_nd_rows(3, N, g), 12, layers, 0, gmax_extra=64)
    assert (c.ref[:, neg] < 0).all(), "the -50 columns' maxima are negative"
    t = c.ref[:, tiny]
    assert (t.abs() < 1e-3).all() and (t < 0).any() and (t > 0).any(), "tiny maxima of both signs"
    # torch's fp32 error per column subset
    ph = _ph()
    tt = torch.full((3, 256), float("-inf"), device="cuda")
    ph._chain_torch(c.x, N, 12, [(L["wT"].cuda(), L["b"].cuda()) for L in layers], (1, 1, 0), 0, gmax=tt)
    et = (tt.double().cpu() - c.ref).abs()
    cols = {n: (i, et[:, i].max().item()) for n, i in (("bias -50", neg), ("tiny", tiny), ("plain", rest))}
    c.check(f"negmax N={N}", cols)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["single", "wide_input", "three_cols"])
def test_mfma_layer0(case):
    """Layer 0 from an LDS input tile on the fp32 MFMA (every chain that is
    not 16 -> 64 followed by another layer), all fp32 layers."""
    g = _gen({"single": 301, "wide_input": 302, "three_cols": 303}[case])
    if case == "single":
        c = _Case(_nd_rows(3, 77, g), 12, [_layer(g, 16, 64, F32, 1, k_used=12)], 0)
    elif case == "wide_input":
        layers = [_layer(g, 32, 128, F32, 1, k_used=20), _layer(g, 128, 64, F32, 0)]
        c = _Case(_nd_rows(3, 77, g, x_ld=32), 20, layers, 0)
        assert c.ch.x_ld == 32
    else:
        layers = [_layer(g, 16, 128, F32, 1, k_used=3), _layer(g, 128, 32, F32, 0, n_used=17)]
        c = _Case(_nd_rows(3, 77, g), 3, layers, 1, out_cols=17)
    c.check(f"mfma0 {case}")


@pytest.mark.gpu
@pytest.mark.parametrize("prec", [F32, X6], ids=["fp32", "x6"])
@pytest.mark.parametrize("N", [32, 64, 128, 256, 512, 768, 1024])
def test_pooled_layer_widths(N, prec):
    """Every plain_layer split as the pooled last layer (K = 128, no ReLU)."""
    g = _gen(400 + N + prec)
    layers = [_layer(g, 16, 64, F32, 1, k_used=12), _layer(g, 64, 128, prec, 1), _layer(g, 128, N, prec, 0)]
    _Case(_nd_rows(3, 77, g), 12, layers, 0).check(f"width N={N} {'x6' if prec else 'fp32'}")


@pytest.mark.gpu
@pytest.mark.parametrize("tail", [False, True], ids=["pooled", "then_softmax"])
@pytest.mark.parametrize("pp,qp", [(F32, F32), (X6, X6), (X6, F32)], ids=["fp32-fp32", "x6-x6", "x6-fp32"])
@pytest.mark.parametrize("n1,n2", [(128, 64), (256, 128), (512, 256)])
def test_fused_pairs(n1, n2, pp, qp, tail):
    """P 64 -> n1 produced in 64-column chunks into Q n1 -> n2, last (pooled)
    or followed by a 32-wide layer and log_softmax."""
    g = _gen(500 + n1 + 2 * pp + qp + 4 * tail)
    layers = [_layer(g, 16, 64, F32, 1, k_used=12), _layer(g, 64, n1, pp, 1, fuse=True), _layer(g, n1, n2, qp, 1)]
    if tail:
        layers.append(_layer(g, n2, 32, qp, 0, n_used=29))
    c = _Case(_nd_rows(3, 77, g), 12, layers, 1 if tail else 0, out_cols=29 if tail else 0)
    c.check(f"fused {n1}-{n2} P{pp} Q{qp} tail={tail}")


@pytest.mark.gpu
def test_per_cloud_weights_and_bias():
    """Layer 0 with per-cloud weights (stride 1024), layer 1 with per-cloud
    weights at a padded stride and a per-cloud bias (stride N): the three
    clouds' operands differ by a factor of two each, so a wrong cloud index is
    a factor of two in the result."""
    ph = _ph()
    g = _gen(600)
    l0, l1, l2 = _layer(g, 16, 64, F32, 1, k_used=12), _layer(g, 64, 128, F32, 1), _layer(g, 128, 64, F32, 0)
    scale = torch.tensor([1.0, 2.0, 4.0])
    l0["wT"] = l0["wT"][None] * scale[:, None, None]
    l1["wT"] = l1["wT"][None] * scale.flip(0)[:, None, None]
    l1["b"] = l1["b"][None] * scale[:, None]
    c = _Case(_nd_rows(3, 77, g), 12, [l0, l1, l2], 0)
    assert c.ch.L[0].w_cloud_stride == 1024 and c.ch.L[1].bias_cloud_stride == 128
    # layer 1's weights again at a stride past their size
    f1 = ph._frag(l1["wT"].cuda())
    padded = torch.full((3, f1.shape[1] + 64), float("nan"), device="cuda")
    padded[:, : f1.shape[1]] = f1
    c.ch.L[1].w, c.ch.L[1].w_cloud_stride = padded.data_ptr(), padded.stride(0)
    c.check("per-cloud")
    assert (c.ref[1] - c.ref[0]).abs().max() > 1.0  # the clouds' results do differ


def _softmax_inputs(oc, variant):
    """(x, layers) of one log_softmax case, on the CPU."""
    g = _gen(700 + oc)
    n = _ph()._npad(oc)
    layers = [_layer(g, 16, 64, F32, 1, k_used=12), _layer(g, 64, 128, X6, 1), _layer(g, 128, n, X6, 0, n_used=oc)]
    x = _nd_rows(3, 33, g)
    if variant == "range90":  # logits reaching about +-90: exp() of them unshifted overflows
        h = torch.nn.functional.pad(x.double(), (0, 4))
        for L in layers[:2]:
            h = torch.relu(h @ L["wT"].double() + L["b"].double())
        top = (h @ layers[2]["wT"].double() + layers[2]["b"].double())[..., :oc].abs().max().item()
        layers[2]["wT"] *= 90.0 / top
        layers[2]["b"] *= 90.0 / top
    if variant == "pad100":  # padded columns must not enter the sum
        layers[2]["b"][oc:] = 100.0
    return x, layers


def _softmax_case(oc, variant, case=None):
    x, layers = _softmax_inputs(oc, variant)
    return (case or _Case)(x, 12, layers, 1, out_cols=oc)


@pytest.mark.gpu
@pytest.mark.parametrize("oc,variant", [(oc, v) for v in ("plain", "range90", "pad100")
                                        for oc in (1, 2, 16, 17, 29, 32, 33, 64, 301)
                                        if not (v == "pad100" and oc in (32, 64))])  # no padded column there
def test_log_softmax_widths(oc, variant):
    """log_softmax over 1 .. 301 columns (one to many columns per lane), logits
    reaching +-90, and padded columns with a bias of +100 outside the sum."""
    c = _softmax_case(oc, variant)
    if variant == "range90" and oc > 1:
        assert c.scale > 80
    c.check(f"softmax oc={oc} {variant}")


@pytest.mark.gpu
@pytest.mark.parametrize("count", [8, 2500])
def test_clear_rearms_exactly_its_range(count):
    g = _gen(800)
    c = _Case(_nd_rows(3, 33, g), 12, _tail_chain(g), 0)
    buf = torch.arange(count + 8, dtype=torch.float32, device="cuda") + 1
    c.ch.clear, c.ch.clear_count = buf.data_ptr(), count
    for entry in BUILDS:
        buf.copy_(torch.arange(count + 8, dtype=torch.float32) + 1)
        c.run(entry)
        assert bool((buf[:count] == float("-inf")).all())
        assert torch.equal(buf[count:].cpu(), torch.arange(count, count + 8, dtype=torch.float32) + 1)
    c.check("clear")


# ---- the two optional prologues (head_*: TNet(3)'s tail; fold_t2: TNet(64)'s transform through layer 0) ----

def _sentinel(*shape):
    t = torch.empty(*shape, dtype=torch.float32, device="cuda")
    t.view(torch.int32).fill_(NAN_BITS)
    return t


def _kept(t):
    return bool((t.contiguous().view(torch.int32) == NAN_BITS).all())


def _padded(x, ld):
    """[rows][ld] with x in the first columns and NaN in the pad."""
    out = torch.full((x.shape[0], ld), float("nan"))
    out[:, : x.shape[1]] = x
    return out


def _rows16(nout):
    """The row k of every position of a fragment-major [16][nout] layer."""
    return _ph()._frag(torch.arange(16.0)[:, None].expand(16, nout).contiguous())


def _report(name, got, ref, e_t, bad):
    """The bound of this file on one published tensor; prints e_hip, e_t and the ratio."""
    e_hip = (got - ref).abs().max().item()
    scale = ref.abs().max().item()
    print(f"{name}: e_hip {e_hip:.3e} e_t {e_t:.3e} scale {scale:.3e} ratio {e_hip / max(e_t, 1e-300):.2f}")
    if not (bool(torch.isfinite(got).all()) and e_hip <= 3 * e_t + 1e-6 * scale):
        bad.append((name, e_hip, e_t, scale))


def _run_checked(c, name, entry, bad):
    """One launch of `entry`: the chain's output against float64 under the bound."""
    got = c.run(entry)
    _report(f"{name} {entry[9:]} out", got, c.ref, c.e_t, bad)


def _head_parts(g, B, head_K, kin, nout):
    """The head prologue's operands and float64 results on the CPU: (h2, w3, b3, basis, t1, W0^T [B][16][nout])."""
    h2 = torch.relu(torch.randn(B, head_K, generator=g) + 1.0)
    w3, b3 = torch.randn(9, head_K, generator=g) / math.sqrt(head_K), torch.randn(9, generator=g) * 0.5
    basis = torch.randn(9, kin * nout, generator=g) / 3.0
    t1_ref = h2.double() @ w3.double().t() + b3.double()
    w_ref = torch.nn.functional.pad((t1_ref @ basis.double()).view(B, kin, nout), (0, 0, 0, 16 - kin))
    assert (t1_ref[1:] - t1_ref[:-1]).abs().amax(dim=1).min() > 1e-3  # the clouds differ
    return h2, w3, b3, basis, t1_ref, w_ref


class _Head:
    """The head prologue's operands for B clouds: h2 (non-negative, rows of
    head_K + 4 floats with NaN pads), W3, b3 and a dense basis [9][kin * nout]
    (not the model's 0/1 structure: a wrong a, k or n index shows); t1 and
    layer 0's per-cloud W^T [B][16][nout] (rows kin..15 zero) in float64 and
    as torch computes them in fp32 on the device."""

    def __init__(self, g, B, head_K, kin, nout):
        self.B, self.K, self.kin, self.nout, self.ld = B, head_K, kin, nout, head_K + 4
        h2, w3, b3, basis, self.t1_ref, self.w_ref = _head_parts(g, B, head_K, kin, nout)
        pad = (0, 0, 0, 16 - kin)
        self.h2, self.w3, self.b3, self.basis = _padded(h2, self.ld).cuda(), w3.cuda(), b3.cuda(), basis.cuda()
        t1_t = torch.addmm(self.b3, h2.cuda(), self.w3.t())
        self.w_t = torch.nn.functional.pad(torch.matmul(t1_t, self.basis).view(B, kin, nout), pad)
        self.e_t1 = (t1_t.double().cpu() - self.t1_ref).abs().max().item()
        self.e_w = (self.w_t.double().cpu() - self.w_ref).abs().max().item()

    def layer0(self, g, relu=1):
        L = _layer(g, 16, self.nout, F32, relu)
        L.update(wT=self.w_ref, dev=(self.w_t, L["b"].cuda()))
        return L

    def attach(self, c):
        """Points chain `c` at the prologue: layer 0's per-cloud weights are a
        sentinel-filled buffer with 64 floats of pad per cloud."""
        self.size = 16 * self.nout
        self.wbuf, self.t1 = _sentinel(self.B, self.size + 64), _sentinel(self.B * 9 + 7)
        ch = c.ch
        ch.L[0].w, ch.L[0].w_cloud_stride = self.wbuf.data_ptr(), self.wbuf.stride(0)
        ch.head_h2, ch.head_ld, ch.head_K = self.h2.data_ptr(), self.ld, self.K
        ch.head_w3, ch.head_b3, ch.head_basis = self.w3.data_ptr(), self.b3.data_ptr(), self.basis.data_ptr()
        ch.head_kin, ch.head_nout, ch.head_t1 = self.kin, self.nout, self.t1.data_ptr()

    def check(self, c, name):
        """Both builds: the output, head_t1 and the published layer 0 against float64."""
        bad = []
        rows = _rows16(self.nout)
        for entry in BUILDS:
            self.wbuf.view(torch.int32).fill_(NAN_BITS)
            self.t1.view(torch.int32).fill_(NAN_BITS)
            _run_checked(c, name, entry, bad)
            assert _kept(self.t1[self.B * 9:]) and _kept(self.wbuf[:, self.size:]), f"{entry}: pads were written"
            _report(f"{name} {entry[9:]} t1", self.t1[: self.B * 9].view(self.B, 9).double().cpu(), self.t1_ref,
                    self.e_t1, bad)
            w = self.wbuf[:, : self.size].cpu()
            _report(f"{name} {entry[9:]} L[0].w", w.double(), _ph()._frag(self.w_ref), self.e_w, bad)
            assert bool((w[:, rows >= self.kin] == 0).all()), f"{entry}: rows kin..15 are not exactly 0"
        assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1, 33, 130])
@pytest.mark.parametrize("kin", [12, 3])
@pytest.mark.parametrize("head_K", [256, 64, 100])
def test_head_prologue_valu_layer0(head_K, kin, N):
    """head_* with layer 0 on the VALU (16 -> 64, 64 -> 128 x6, 128 -> 64,
    pooled): head_K 256 is the one-float4-per-lane path, 64 and 100 the strided
    loop; kin = in_cols = 12 and 3.  The whole thing in float64: t1, W0[b], the
    chain.  Only the cloud's first workgroup publishes L[0].w[b]."""
    g = _gen(900 + head_K + kin + N)
    hd = _Head(g, 3, head_K, kin, 64)
    layers = [hd.layer0(g), _layer(g, 64, 128, X6, 1), _layer(g, 128, 64, F32, 0)]
    c = _Case(_nd_rows(3, N, g), kin, layers, 0)
    hd.attach(c)
    hd.check(c, f"head valu K={head_K} kin={kin} N={N}")


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1, 33, 130])
@pytest.mark.parametrize("case", ["single", "nout128", "kin16"])
def test_head_prologue_mfma_layer0(case, N):
    """head_* with layer 0 on the MFMA path, where every workgroup stores layer
    0's weights to memory and its layer 0 loads them back after a workgroup
    barrier: a one-layer chain 16 -> 64; 16 -> 128 (head_nout = 128), 128 ->
    64; and in_cols = x_ld = kin = 16 (16 -> 64, 64 -> 64).  All pooled."""
    g = _gen(950 + N + {"single": 0, "nout128": 1000, "kin16": 2000}[case])
    if case == "single":
        hd = _Head(g, 3, 256, 12, 64)
        layers, x, in_cols = [hd.layer0(g)], _nd_rows(3, N, g), 12
    elif case == "nout128":
        hd = _Head(g, 3, 100, 12, 128)
        layers, x, in_cols = [hd.layer0(g), _layer(g, 128, 64, F32, 0)], _nd_rows(3, N, g), 12
    else:
        hd = _Head(g, 3, 64, 16, 64)
        layers, x, in_cols = [hd.layer0(g), _layer(g, 64, 64, F32, 0)], _nd_rows(3, N, g, x_ld=16), 16
    c = _Case(x, in_cols, layers, 0)
    assert c.ch.x_ld == x.shape[2]
    hd.attach(c)
    hd.check(c, f"head mfma {case} N={N}")


def _fold_parts(seed, N, prec1):
    """The fold_t2 prologue's operands for 3 clouds on the CPU: (w0 [3][12][64], b0, t2 [3][64][64], the folded
    layer 0 in float64 -- W0' [3][16][64], b0' [3][64] --, the layers after it, x)."""
    g = _gen(seed)
    w0 = torch.randn(3, 12, 64, generator=g) / math.sqrt(12)
    b0, t2 = torch.randn(64, generator=g) * 0.5, torch.randn(3, 64, 64, generator=g) / 8.0
    w_ref = torch.nn.functional.pad(w0.double() @ t2.double(), (0, 0, 0, 4))
    b_ref = b0.double() @ t2.double()                                   # [B][64]
    assert (b_ref[1:] - b_ref[:-1]).abs().amax(dim=1).min() > 1e-3      # the clouds differ
    tail = [_layer(g, 64, 128, prec1, 1), _layer(g, 128, 64, F32, 0)]
    return w0, b0, t2, w_ref, b_ref, tail, _nd_rows(3, N, g)


class _Fold:
    """The fold_t2 prologue's operands for 3 clouds: a per-cloud layer 0 (W0^T
    [12][64] in a K = 16 fragment, bias b0) and a dense t2 per cloud in rows
    of fold_ld floats (NaN pads); chain 16 -> 64, 64 -> 128 (prec1), 128 ->
    64, pooled.  float64: layer 0 is W0'[b] = W0^T[b] t2[b], b0'[b] = b0^T
    t2[b], its relu flag applied after."""

    def __init__(self, seed, N, relu0, prec1, fold_ld, prefill=None, case=None):
        ph = _ph()
        B = self.B = 3
        w0, b0, t2, self.w_ref, self.b_ref, tail, self.x = _fold_parts(seed, N, prec1)
        pad = (0, 0, 0, 4)
        self.w0f = ph._frag(torch.nn.functional.pad(w0, pad)).cuda()             # [B][1024]
        self.b0, t2d = b0.cuda(), t2.cuda()
        self.t2, self.fold_ld = _padded(t2.view(B, 4096), fold_ld).cuda(), fold_ld
        w_t = torch.nn.functional.pad(torch.matmul(w0.cuda(), t2d), pad)
        b_t = torch.matmul(self.b0, t2d)
        self.e_w = (w_t.double().cpu() - self.w_ref).abs().max().item()
        self.e_b = (b_t.double().cpu() - self.b_ref).abs().max().item()
        l0 = dict(wT=self.w_ref, b=self.b_ref, K=16, N=64, prec=F32, relu=relu0, fuse=False, dev=(w_t, b_t))
        self.layers = [l0] + tail
        c = self.c = (case or _Case)(self.x, 12, self.layers, 0)
        # the HIP chain: the untransformed layer 0 and t2
        L0 = c.ch.L[0]
        L0.w, L0.w_cloud_stride, L0.bias, L0.bias_cloud_stride = self.w0f.data_ptr(), 1024, self.b0.data_ptr(), 0
        c.ch.fold_t2, c.ch.fold_ld = self.t2.data_ptr(), fold_ld
        self.prefill = prefill
        self.out_w, self.out_b = torch.empty(B, 1024, device="cuda"), torch.empty(B * 64 + 8, device="cuda")
        if prefill is not None:
            c.ch.fold_out_w, c.ch.fold_out_b = self.out_w.data_ptr(), self.out_b.data_ptr()

    def run(self, name, entry, bad):
        """One launch: the output and, when published, fold_out_w / fold_out_b
        against float64; rows 12..15 of fold_out_w keep their pre-fill."""
        self.out_w.view(torch.int32).fill_(self.prefill or 0)
        self.out_b.view(torch.int32).fill_(NAN_BITS)
        _run_checked(self.c, name, entry, bad)
        if self.prefill is None:
            return
        rows = _rows16(64)
        w = self.out_w.cpu()
        assert bool((w[:, rows >= 12].contiguous().view(torch.int32) == self.prefill).all()), "rows 12..15 were written"
        assert _kept(self.out_b[self.B * 64:])
        _report(f"{name} {entry[9:]} fold_out_w", w[:, rows < 12].double(), _ph()._frag(self.w_ref)[:, rows < 12],
                self.e_w, bad)
        _report(f"{name} {entry[9:]} fold_out_b", self.out_b[: self.B * 64].view(self.B, 64).double().cpu(), self.b_ref,
                self.e_b, bad)

    def kernel(self):
        """ndnet_pn_fold_t2_run on the same operands: (outf, outb) on the CPU."""
        from ndnet import _lib
        outf, outb = torch.zeros(self.B, 1024, device="cuda"), torch.zeros(self.B, 64, device="cuda")
        rc = _lib.lib().ndnet_pn_fold_t2_run(self.w0f.data_ptr(), 1024, self.b0.data_ptr(), self.t2.data_ptr(),
                                             self.fold_ld, outf.data_ptr(), outb.data_ptr(), self.B,
                                             _lib.stream_ptr(outf.device))
        assert rc == 0
        torch.cuda.synchronize()
        return outf.cpu(), outb.cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1, 33, 130])
@pytest.mark.parametrize("fold_ld", [4096, 4160])
@pytest.mark.parametrize("prec1", [F32, X6], ids=["fp32", "x6"])
@pytest.mark.parametrize("relu0", [0, 1])
def test_fold_t2_prologue(relu0, prec1, fold_ld, N):
    """fold_t2 with fold_out_w / fold_out_b: x_t2 = t2[b]^T (W0 x + b0) carried
    through the chain, layer 0 without a ReLU (the model's case) and with one,
    layer 1 reading fp32 rows or the bf16 planes layer 0 writes.  The published
    tensors against float64 and, within the same bound (not bit-equal: FMAs in
    one, the MFMA in the other), against ndnet_pn_fold_t2_run's."""
    f = _Fold(1100 + 8 * N + 4 * relu0 + 2 * prec1 + fold_ld, N, relu0, prec1, fold_ld, prefill=NAN_BITS)
    kf, kb = f.kernel()
    rows = _rows16(64) < 12
    name, bad = f"fold relu0={relu0} prec1={prec1} ld={fold_ld} N={N}", []
    for entry in BUILDS:
        f.run(name, entry, bad)
        d_w = (f.out_w.cpu()[:, rows] - kf[:, rows]).abs().max().item()
        d_b = (f.out_b[: 3 * 64].view(3, 64).cpu() - kb).abs().max().item()
        print(f"{name} {entry[9:]}: |published - fold_t2_run| W {d_w:.3e} (e_t {f.e_w:.3e}) b {d_b:.3e} (e_t {f.e_b:.3e})")
        if not d_w <= 3 * f.e_w + 1e-6 * f.w_ref.abs().max().item():
            bad.append((name, entry, "W against the kernel", d_w, f.e_w))
        if not d_b <= 3 * f.e_b + 1e-6 * f.b_ref.abs().max().item():
            bad.append((name, entry, "b against the kernel", d_b, f.e_b))
    assert not bad, bad


@pytest.mark.gpu
def test_fold_t2_prologue_without_publication():
    """fold_out_w and fold_out_b NULL: the chain folds t2 for itself only."""
    f = _Fold(1200, 130, 0, X6, 4096)
    bad = []
    for entry in BUILDS:
        f.run("fold unpublished", entry, bad)
    assert not bad, bad


@pytest.mark.gpu
def test_fold_t2_publication_feeds_a_second_chain():
    """As chain D after chain C: a second chain runs the published W0'[b] and
    b0'[b] as a plain per-cloud layer 0 (rows 12..15 zero-initialised, and
    still zero after) and matches float64; once per build of the publisher."""
    f = _Fold(1300, 130, 0, X6, 4096, prefill=0)
    d = _Case(f.x, 12, f.layers, 0)
    L0 = d.ch.L[0]
    L0.w, L0.w_cloud_stride, L0.bias, L0.bias_cloud_stride = f.out_w.data_ptr(), 1024, f.out_b.data_ptr(), 64
    assert not d.ch.fold_t2
    bad = []
    for entry in BUILDS:
        f.run("fold publisher", entry, bad)
        d.check(f"consumer of {entry[9:]}")
    assert not bad, bad


# ---- argument checks: rejected before any HIP call, so these run without a GPU ----

def _arg_block(edit, device="cpu"):
    """A valid 4-layer block (16 -> 64, 64 -> 128 fused into 128 -> 64 x6, 64 -> 32 x6, log_softmax),
    changed by `edit(spec)`; returns what both entry points answer.  Over host memory by default:
    a rejected block is never launched."""
    from ndnet import _lib
    ph = _ph()
    dims = [(16, 64, F32), (64, 128, F32), (128, 64, X6), (64, 32, X6)]
    bufs = [(torch.zeros(K * N * 2, device=device), torch.zeros(N, device=device)) for K, N, _ in dims]
    hip = [(w, 0, b, K, N, p) for (w, b), (K, N, p) in zip(bufs, dims)]
    x, out = torch.zeros(2, 5, 12, device=device), torch.zeros(2, 5, 29, device=device)
    spec = dict(n=5, in_cols=12, layers=hip, relus=[1, 1, 1, 0], mode=1, gmax=None, out_cols=29, fuse=(1,))
    spec = edit(spec) or spec
    ch = ph._build_chain(spec["n"], spec["in_cols"], spec["layers"], spec["relus"][: len(spec["layers"])],
                         spec["mode"], gmax=spec["gmax"], out_cols=spec["out_cols"], fuse=spec["fuse"])
    ch.x, ch.out = x.data_ptr(), out.data_ptr()
    for k, v in spec.get("set", {}).items():
        setattr(ch, k, v)
    rcs = [getattr(_lib.lib(), e)(ctypes.byref(ch), 2, None) for e in BUILDS]
    if device != "cpu":
        torch.cuda.synchronize()
    del bufs
    return rcs


def _with_layer(i, **kw):
    def edit(spec):
        w, s, b, K, N, p = spec["layers"][i]
        d = dict(K=K, N=N, prec=p)
        d.update(kw)
        spec["layers"] = list(spec["layers"])
        spec["layers"][i] = (w, s, b, d["K"], d["N"], d["prec"])
    return edit


def _mode0_without_gmax(spec):
    spec.update(mode=0, out_cols=0, layers=spec["layers"][:3])


def _fused_into_512(spec):
    # 64 -> 128 fused into a 512-wide layer (128 -> 512 fp32, then 512 -> 32)
    L = spec["layers"]
    spec["layers"] = [L[0], L[1], L[2][:3] + (128, 512, F32), L[3][:3] + (512, 32, F32)]


def _narrow(spec):
    spec["set"] = {"max_width": 24}  # region 0 holds the 32-wide logits (and the 16-wide input)


ARG_CASES = {
    "x6 layer 0": lambda s: (_with_layer(0, K=32, prec=X6)(s), s.update(in_cols=12))[1],
    "x6 K % 32": lambda s: (_with_layer(1, N=64)(s), _with_layer(2, K=48)(s), s.update(fuse=()))[2],
    "x6 K != previous N": _with_layer(3, K=128),
    "max_width too small": _narrow,
    "out_cols > last N": lambda s: s.update(out_cols=33),
    "mode 0 without gmax": _mode0_without_gmax,
    "fused into N = 512": _fused_into_512,
    "fuse_next on the last layer": lambda s: s.update(fuse=(1, 3)),
}


@pytest.mark.gpu
def test_unedited_argument_block_is_accepted():
    """The block the rejected ones are one edit away from is itself valid (it runs, on zeros)."""
    assert _arg_block(lambda spec: None, device="cuda") == [0, 0]


@pytest.mark.parametrize("case", sorted(ARG_CASES))
def test_inconsistent_argument_blocks_are_rejected(case, capfd):
    """NDNET_ERR_ARG (-20) from both entry points, before anything is launched."""
    assert _arg_block(ARG_CASES[case]) == [-20, -20]
    assert capfd.readouterr().err.count("invalid argument") == 2


def _head_block(edit, device="cpu"):
    """A valid chain with the head prologue (16 -> 64 per cloud, 64 -> 128, pooled; head_K = 256, kin 12),
    changed by `edit(ch, tensors)`; returns what both entry points answer.  Over host memory by default."""
    from ndnet import _lib
    ph = _ph()
    shapes = dict(w0=(2, 1024), b0=(64,), w1=(64 * 128,), b1=(128,), x=(2, 5, 12), gmax=(2, 128), h2=(2, 256),
                  w3=(9, 256), b3=(9,), basis=(9, 12 * 64), t1=(2, 9))
    t = {k: torch.zeros(*s, device=device) for k, s in shapes.items()}
    ch = ph._build_chain(5, 12, [(t["w0"], 1024, t["b0"], 16, 64), (t["w1"], 0, t["b1"], 64, 128)], [1, 1], 0,
                         gmax=t["gmax"])
    ch.x = t["x"].data_ptr()
    ch.head_h2, ch.head_ld, ch.head_K = t["h2"].data_ptr(), 256, 256
    ch.head_w3, ch.head_b3, ch.head_basis = t["w3"].data_ptr(), t["b3"].data_ptr(), t["basis"].data_ptr()
    ch.head_kin, ch.head_nout, ch.head_t1 = 12, 64, t["t1"].data_ptr()
    edit(ch, t)
    rcs = [getattr(_lib.lib(), e)(ctypes.byref(ch), 2, None) for e in BUILDS]
    if device != "cpu":
        torch.cuda.synchronize()
    return rcs


def _set(name, value):
    return lambda ch, t: setattr(ch, name, value)


def _layer0_k32(ch, t):  # a valid two-k-group layer 0 otherwise: region 0 widened for its input
    ch.L[0].K, ch.max_width = 32, 32


def _layer0_n128(ch, t):  # a 128-wide layer 0 (and layer 1 reading it) with head_nout left at 64
    ch.L[0].N, ch.L[1].K, ch.max_width2 = 128, 128, 128


HEAD_ARG_CASES = {
    "NULL head_w3": _set("head_w3", None),
    "NULL head_b3": _set("head_b3", None),
    "NULL head_basis": _set("head_basis", None),
    "NULL head_t1": _set("head_t1", None),
    "head_K < 1": _set("head_K", 0),
    "head_ld < head_K": lambda ch, t: (setattr(ch, "head_K", 100), setattr(ch, "head_ld", 96)),
    "head_kin < 1": _set("head_kin", 0),
    "head_kin > 16": _set("head_kin", 17),
    "L[0].K != 16": _layer0_k32,
    "head_nout != L[0].N": _set("head_nout", 128),
    "L[0].N != head_nout": _layer0_n128,
    "w_cloud_stride < 16 head_nout": lambda ch, t: setattr(ch.L[0], "w_cloud_stride", 512),
    "shared layer 0": lambda ch, t: setattr(ch.L[0], "w_cloud_stride", 0),
    "head_K 256, head_h2 misaligned": lambda ch, t: (setattr(ch, "head_h2", t["h2"].data_ptr() + 4), setattr(ch, "head_ld", 260)),
    "head_K 256, head_w3 misaligned": lambda ch, t: setattr(ch, "head_w3", t["w3"].data_ptr() + 8),
    "head_K 256, head_ld % 4": _set("head_ld", 258),
}


@pytest.mark.gpu
def test_unedited_head_block_is_accepted():
    assert _head_block(lambda ch, t: None, device="cuda") == [0, 0]


@pytest.mark.parametrize("case", sorted(HEAD_ARG_CASES))
def test_inconsistent_head_blocks_are_rejected(case, capfd):
    """NDNET_ERR_ARG (-20) from both entry points, before anything is launched."""
    assert _head_block(HEAD_ARG_CASES[case]) == [-20, -20]
    assert capfd.readouterr().err.count("invalid argument") == 2
