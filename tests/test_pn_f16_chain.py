"""The fp16 two-slice form of the chain kernel (ndnet_pn_chain_f16_run, ndnet_pn_chain_f16_run_t32:
include/ndnet_pointnet.h) driven directly, on chains shaped like the default forward's A, B (collapsed)
and D (collapsed), with tests/test_pn_chain.py's inputs, references and bound.  B is the real collapsed
block of tests/test_collapse_chain_b.py: the head prologue (head_*), then the fold prologue with a shared
matrix and the folded layer's bias, layer 0 = relu(x (W1f[b] M) + (b1 M + bM)), and x_nonfinite_nan in the
window case as the model sets it -- so a fallback tile runs both prologues twice, and what the head
prologue publishes is compared too.

  e_hip <= 3 e_t + 1e-6 max |float64 result|,  e_t the error of torch's fp32 chain on the device.

Every case runs on both tile builds, at 3 x 65 and 2 x 130 points (one full 64-point tile and a one-point
tail; two full tiles and a two-point tail; 32-point tiles alike).  The window cases build their inputs so
that the tiles' maxima sit where the case needs them, checked in float64 before anything is launched; the
expected number of fallback tiles comes from that float64 evaluation, never from the kernel."""
import ctypes
import math

import pytest
import torch

from test_collapse_chain_b import _attach_fold
from test_pn_chain import F32, NAN_BITS, X6, _Case, _gen, _Head, _layer, _nd_rows, _report

F16_BUILDS = (("ndnet_pn_chain_f16_run", 64), ("ndnet_pn_chain_f16_run_t32", 32))
BF16_ENTRY = {64: "ndnet_pn_chain_run", 32: "ndnet_pn_chain_run_t32"}
SHAPES = [(3, 65), (2, 130)]
LO, HI = 2.0 ** -4, 2.0 ** 11  # the window of a split layer's input tile: max |v| in [LO, HI), or all zero


def _ph():
    from ndnet.models import pointnet_hip as ph
    return ph


def _chain_layers(shape, g, zero_bias=False):
    """(in_cols, layers, mode, out_cols) of a chain shaped like the default forward's."""
    if shape == "A":    # TNet(3): 3 -> 64 on the VALU, 64 -> 128, 128 -> 1024, max over points
        spec = (3, [_layer(g, 16, 64, F32, 1, k_used=3), _layer(g, 64, 128, X6, 1), _layer(g, 128, 1024, X6, 1)], 0, 0)
    elif shape == "B":  # (built by _b_parts / _b_layers below: layer 0 is per cloud, from the prologues)
        raise ValueError(shape)
    else:               # D collapsed: 12 -> 512 fused into 512 -> 256, 256 -> 128, 128 -> 29 (of 64), log-softmax
        spec = (12, [_layer(g, 16, 512, F32, 1, k_used=12, fuse=True), _layer(g, 512, 256, X6, 1),
                     _layer(g, 256, 128, X6, 1), _layer(g, 128, 64, X6, 0, n_used=29)], 1, 29)
    if zero_bias:
        for L in spec[1]:
            L["b"].zero_()
    return spec


class _F16Case(_Case):
    """tests/test_pn_chain.py's case with the fp16 block beside its chain block."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        ph = _ph()
        self.ext = ph._F16()
        self.counter = torch.zeros(1, dtype=torch.int32, device="cuda")
        self.ext.fallbacks = self.counter.data_ptr()
        for l, L in enumerate(self.layers):
            if L["prec"] == X6:
                planes, scale = ph._frag_f16(L["wT"].cuda())
                self.keep += [planes, scale]
                self.ext.w16[l], self.ext.scale[l] = planes.data_ptr(), scale.data_ptr()

    def run_f16(self, entry):
        """One launch of the fp16 form; (result in float64 on the CPU, the float32 result, fallback tiles)."""
        from ndnet import _lib
        if self.mode == 0:
            self.gmax.fill_(float("-inf"))
        else:
            self.out.fill_(float("nan"))
        rc = getattr(_lib.lib(), entry)(ctypes.byref(self.ch), ctypes.byref(self.ext), self.B, _lib.stream_ptr(self.x.device))
        assert rc == 0, f"{entry} returned {rc}"
        n = _lib.lib().ndnet_pn_take_f16_fallbacks(self.counter.data_ptr(), _lib.stream_ptr(self.x.device))
        assert n >= 0 and int(self.counter.item()) == 0, "the counter is handed over and reset"
        got = (self.gmax[:, : self.n_last] if self.mode == 0 else self.out).clone()
        return got.double().cpu(), got, n

    def run_bf16(self, entry):
        self.run(entry)
        return (self.gmax[:, : self.n_last] if self.mode == 0 else self.out).clone()


def _b_parts(g, B, zero_bias=False, same_clouds=False):
    """The operands of chain B collapsed for B clouds: the head prologue's (t1 = h2 @ w3^T + b3, W1f[b] = t1[b] @
    basis), conv1's bias b0, the folded layer (M, bM) and the shared tail 64 -> 128, 128 -> 1024.
    same_clouds: every cloud has cloud 0's h2 row, so that one scaling of M serves all of them."""
    hd = _Head(g, B, 256, 12, 64)
    if same_clouds:
        hd.h2.copy_(hd.h2[:1].expand_as(hd.h2))
        hd.t1_ref, hd.w_ref, hd.w_t = (t[:1].expand_as(t).clone() for t in (hd.t1_ref, hd.w_ref, hd.w_t))
    b0, m, mb = torch.randn(64, generator=g) * 0.5, torch.randn(64, 64, generator=g) / 8.0, torch.randn(64, generator=g) * 0.5
    tail = [_layer(g, 64, 128, X6, 1), _layer(g, 128, 1024, X6, 1)]
    if zero_bias:
        b0.zero_()
        mb.zero_()
        for L in tail:
            L["b"].zero_()
    return dict(hd=hd, b0=b0, m=m, mb=mb, tail=tail)


def _b_layers(p, clouds=slice(None)):
    """The chain's layers from the parts as they are now (layer 0 composed per cloud, in float64 and as torch
    computes it in fp32 on the device), for the clouds `clouds`."""
    hd, b0, m, mb = p["hd"], p["b0"], p["m"], p["mb"]
    md = m.cuda()
    dev = (torch.matmul(hd.w_t, md)[clouds], torch.addmv(mb.cuda(), md.t(), b0.cuda()))
    l0 = dict(wT=(hd.w_ref @ m.double())[clouds], b=b0.double() @ m.double() + mb.double(), K=16, N=64, prec=F32,
              relu=1, fuse=False, dev=dev)
    return [l0] + p["tail"]


def _b_attach(c, p, flag):
    p["hd"].attach(c)
    _attach_fold(c.ch, c.keep, p["b0"].cuda(), p["m"].cuda(), p["mb"].cuda(), flag)


def _b_published(hd):
    """What the head prologue published, after a launch: (t1, W1f) clones; the sentinels are set again."""
    out = (hd.t1.clone(), hd.wbuf.clone())
    hd.t1.view(torch.int32).fill_(NAN_BITS)
    hd.wbuf.view(torch.int32).fill_(NAN_BITS)
    return out


def _tile_maxima(x, in_cols, layers, tile, nonfinite_nan=0):
    """Per cloud and tile of `tile` rows (zero rows past the cloud's last point, as the kernel stages them):
    the maximum |v| of every split layer's input tile, in float64, with the kernel's rules for what is not
    finite: fmaxf's ReLU turns a NaN into 0, and the maximum keeps a NaN or an infinity it meets.
    -> {layer index: [B][tiles]}."""
    B, N, _ = x.shape
    T = (N + tile - 1) // tile
    h = torch.zeros(B, T * tile, layers[0]["K"], dtype=torch.float64)
    xin = x[..., :in_cols].double()
    if nonfinite_nan:
        xin = torch.where(torch.isfinite(xin), xin, torch.full_like(xin, float("nan")))
    h[:, :N, :in_cols] = xin
    out = {}
    for l, L in enumerate(layers):
        if L["prec"] == X6:
            a = h.abs().reshape(B, T, tile * h.shape[-1])
            m = a.nan_to_num(nan=float("inf")).amax(dim=2)  # a NaN is outside the window, as an infinity is
            out[l] = m
        h = torch.matmul(h, L["wT"].double()) + L["b"].double()
        if L["relu"]:
            h = torch.where(h > 0, h, torch.zeros_like(h))
    return out


def _fallback_tiles(maxima):
    """[B][tiles] bool: the tiles with a split layer's input outside the window."""
    bad = None
    for m in maxima.values():
        b = ~((m == 0) | ((m >= LO) & (m < HI)))
        bad = b if bad is None else bad | b
    return bad


@pytest.mark.gpu
@pytest.mark.parametrize("B,N", SHAPES)
@pytest.mark.parametrize("shape", ["A", "B", "D"])
def test_accuracy_against_float64(shape, B, N):
    """NDT-like rows: the test_pn_chain.py bound, no fallback tile, and the bf16 form's error beside it."""
    g = _gen(700 + 10 * "ABD".index(shape) + N)
    parts = _b_parts(g, B) if shape == "B" else None
    in_cols, layers, mode, out_cols = (12, _b_layers(parts), 0, 0) if parts else _chain_layers(shape, g)
    x = _nd_rows(B, N, g)
    c = _F16Case(x, in_cols, layers, mode, out_cols)
    if parts:
        _b_attach(c, parts, 0)
    for tile in (64, 32):
        assert not bool(_fallback_tiles(_tile_maxima(x, in_cols, layers, tile)).any()), "inputs meant to stay in the window"
    bound = 3 * c.e_t + 1e-6 * c.scale
    bad = []
    for entry, tile in F16_BUILDS:
        got, _, fallbacks = c.run_f16(entry)
        e_bf16 = (c.run_bf16(BF16_ENTRY[tile]).double().cpu() - c.ref).abs().max().item()
        e_f16 = (got - c.ref).abs().max().item()
        print(f"chain {shape} {B}x{N} tile {tile}: e_f16 {e_f16:.3e} e_bf16_x6 {e_bf16:.3e} e_t {c.e_t:.3e} "
              f"scale {c.scale:.3e} bound {bound:.3e} fallbacks {fallbacks}")
        assert torch.isfinite(got).all()
        if not e_f16 <= bound or fallbacks != 0:
            bad.append((entry, e_f16, bound, fallbacks))
        if parts:  # what the head prologue published, against float64 as tests/test_pn_chain.py holds it
            hd = parts["hd"]
            _b_published(hd)  # (the bf16 launch's)
            c.run_f16(entry)
            t1, w = _b_published(hd)
            _report(f"chain B tile {tile} t1", t1[: B * 9].view(B, 9).double().cpu(), hd.t1_ref, hd.e_t1, bad)
            _report(f"chain B tile {tile} L[0].w", w[:, : hd.size].double().cpu(), _ph()._frag(hd.w_ref), hd.e_w, bad)
    assert not bad, bad


def _edge_scales(base, in_cols, mats, target=1.05 * LO):
    """mats: (W^T in float64, relu, feeds a split layer) per layer -> the factor of each layer's weights that
    puts row 0's maximum at its output at `target` (1.05 * 2^-4) where that output is a split layer's input
    (else 1)."""
    h = torch.nn.functional.pad(base[:, :in_cols].double(), (0, mats[0][0].shape[0] - in_cols))
    out = []
    for w, relu, feeds in mats:
        o = torch.matmul(h, w)
        o = torch.relu(o) if relu else o
        s = target / o[0].abs().max().item() if feeds else 1.0
        out.append(s)
        h = o * s
    return out


def _lower_edge_case(shape, B, N, g, target=1.05 * LO):
    """Zero biases (the chain is then positively homogeneous), rows of period 32 -- so every tile of either
    build holds the same rows, the ragged tail a prefix of them -- whose row 0 is 8 times the others, and
    each layer's weights rescaled so that row 0's maximum at its output is `target`, 1.05 * 2^-4: every split
    layer's tile maximum then sits just above the window's lower edge (the caller checks it), most elements
    below 2^-6.  (tests/test_pn_f16_shapes.py puts them below the upper edge with target = 0.9 * 2^11.)"""
    base = _nd_rows(1, 32, g)[0]
    base[1:] *= 0.125
    x = base[torch.arange(N) % 32].unsqueeze(0).repeat(B, 1, 1).contiguous()
    if shape == "B":
        # the real collapsed block: the clouds share one h2 row (one scaling then serves all of them), and
        # the folded matrix M carries layer 0's factor -- the composed W1f[b] M produces the first windowed tensor
        parts = _b_parts(g, B, zero_bias=True, same_clouds=True)
        tail = parts["tail"]
        mats = [(parts["hd"].w_ref[0] @ parts["m"].double(), 1, True), (tail[0]["wT"].double(), 1, True),
                (tail[1]["wT"].double(), 1, False)]
        s = _edge_scales(base, 12, mats, target)
        parts["m"] *= s[0]
        tail[0]["wT"] *= s[1]
        return x, 12, _b_layers(parts), 0, 0, parts
    in_cols, layers, mode, out_cols = _chain_layers(shape, g, zero_bias=True)
    feeds = [l + 1 < len(layers) and layers[l + 1]["prec"] == X6 for l in range(len(layers))]
    for L, s in zip(layers, _edge_scales(base, in_cols, [(L["wT"].double(), L["relu"], f) for L, f in zip(layers, feeds)], target)):
        L["wT"] *= s
    return x, in_cols, layers, mode, out_cols, None


@pytest.mark.gpu
@pytest.mark.parametrize("B,N", SHAPES)
@pytest.mark.parametrize("shape", ["A", "B", "D"])
def test_lower_edge_keeps_subnormal_slices(shape, B, N):
    """Tile maxima just above 2^-4, most elements below 2^-6: their low slices are fp16 subnormals, which the
    MFMA must keep for the bound to hold -- and it must hold in the fp16 form itself (no fallback tile)."""
    g = _gen(800 + 10 * "ABD".index(shape) + N)
    x, in_cols, layers, mode, out_cols, parts = _lower_edge_case(shape, B, N, g)
    for tile in (64, 32):
        mx = _tile_maxima(x, in_cols, layers, tile)
        for l, m in mx.items():
            assert bool(((m >= 1.01 * LO) & (m <= 1.2 * LO)).all()), (l, tile, m)
    # most elements of the split layers' inputs are below 2^-6
    h = torch.nn.functional.pad(x[..., :in_cols].double(), (0, layers[0]["K"] - in_cols))
    small = []
    for L in layers:
        if L["prec"] == X6:
            small.append((h.abs() < 2.0 ** -6).double().mean().item())
        h = torch.matmul(h, L["wT"].double())
        h = torch.relu(h) if L["relu"] else h
    assert all(s > 0.5 for s in small), small
    c = _F16Case(x, in_cols, layers, mode, out_cols)
    if parts:
        _b_attach(c, parts, 0)
    bound = 3 * c.e_t + 1e-6 * c.scale
    bad = []
    for entry, tile in F16_BUILDS:
        got, _, fallbacks = c.run_f16(entry)
        e_f16 = (got - c.ref).abs().max().item()
        print(f"lower edge {shape} {B}x{N} tile {tile}: e_f16 {e_f16:.3e} e_t {c.e_t:.3e} scale {c.scale:.3e} "
              f"bound {bound:.3e} below 2^-6 {[round(s, 2) for s in small]} fallbacks {fallbacks}")
        if not e_f16 <= bound or fallbacks != 0:
            bad.append((entry, e_f16, bound, fallbacks))
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["A", "B", "D"])
def test_tiles_outside_the_window_fall_back_bit_for_bit(shape):
    """Four clouds of 65 points, zero biases: cloud 0 untouched; cloud 1 times 3e4 (past 2^11 from layer 0 on);
    cloud 2 times 1e-6 (below 2^-4, not zero); cloud 3 with a NaN row and, in every tile of either build, a
    row with one infinity.  The fallback tiles are those the float64 evaluation puts outside the window,
    counted; a cloud all of whose tiles fell back equals the bf16 launch bit for bit; cloud 0 keeps the bound."""
    g = _gen(900 + "ABD".index(shape))
    B, N = 4, 65
    parts = _b_parts(g, B, zero_bias=True) if shape == "B" else None
    in_cols, layers, mode, out_cols = (12, _b_layers(parts), 0, 0) if parts else _chain_layers(shape, g, zero_bias=True)
    x = _nd_rows(B, N, g)
    x[1] *= 3e4
    x[2] *= 1e-6
    x[3, 5, 1] = float("nan")
    for r in (3, 40, 64):
        x[3, r, 0] = float("inf")
    nan_flag = 1 if shape == "B" else 0  # chain B collapsed sets x_nonfinite_nan: such rows enter layer 0 as NaN
    # references of the finite cloud 0
    c = _F16Case(x[:1], in_cols, _b_layers(parts, slice(0, 1)) if parts else layers, mode, out_cols)
    # the four-cloud launch: the case's argument blocks over all clouds (no reference of the non-finite rows is needed)
    finite = x.clone()
    finite[3] = x[0]
    full = _F16Case(finite, in_cols, layers, mode, out_cols)
    full.x.copy_(x.cuda())
    if parts:
        _b_attach(full, parts, nan_flag)
    full.ch.x_nonfinite_nan = nan_flag
    for entry, tile in F16_BUILDS:
        want_bad = _fallback_tiles(_tile_maxima(x, in_cols, layers, tile, nan_flag))
        assert not bool(want_bad[0].any()) and bool(want_bad[1].all()) and bool(want_bad[2].all())
        if not nan_flag:
            assert bool(want_bad[3].all()), "an infinity in every tile of cloud 3"
        if parts:
            _b_published(parts["hd"])
        got64, got, fallbacks = full.run_f16(entry)
        pub_f16 = _b_published(parts["hd"]) if parts else None
        ref_bf16 = full.run_bf16(BF16_ENTRY[tile])
        if parts:
            # both prologues ran twice in the fallen-back tiles: t1 and the published W1f[b] of every cloud
            # (pads included) are the bf16 launch's, bit for bit
            for a, b_ in zip(pub_f16, _b_published(parts["hd"])):
                assert torch.equal(a.view(torch.int32), b_.view(torch.int32)), "the head prologue's publication differs"
            assert not bool((pub_f16[0][: B * 9].view(torch.int32) == NAN_BITS).any())
        print(f"window {shape} tile {tile}: fallback tiles {fallbacks}, expected {int(want_bad.sum())} "
              f"of {want_bad.numel()} ({want_bad.sum(dim=1).tolist()} per cloud)")
        assert fallbacks == int(want_bad.sum())
        for b in range(1, B):
            if bool(want_bad[b].all()):
                assert torch.equal(got[b].view(torch.int32), ref_bf16[b].view(torch.int32)), f"cloud {b}"
        e0 = (got64[0] - c.ref[0]).abs().max().item()
        assert e0 <= 3 * c.e_t + 1e-6 * c.scale, (e0, c.e_t, c.scale)


@pytest.mark.gpu
def test_fold_on_the_device_equals_the_host_restatement():
    """ndnet_pn_fold16_run against ``_frag_f16`` on the CPU, bit for bit: a layer with BatchNorm and column
    offset, an unpadded one, one whose maximum is an exact power of two, an all-zero one."""
    from ndnet import _lib
    ph = _ph()
    g = _gen(31)
    cases = []
    w = torch.randn(100, 70, generator=g) * 0.2                      # N = 100 rows, ld 70, columns 6 .. 69 used
    bn = (torch.rand(100, generator=g) + 0.5, torch.rand(100, generator=g) + 0.5, 1e-5)
    cases.append((w, bn, 6, 64, 64, 128))
    cases.append((torch.randn(64, 128, generator=g) * 3.0, None, 0, 128, 128, 64))
    p2 = torch.randn(32, 32, generator=g).clamp(-1, 1) * 0.25
    p2[3, 4] = 0.5
    cases.append((p2, None, 0, 32, 32, 32))
    cases.append((torch.zeros(16, 32), None, 0, 32, 32, 16))
    arr = (ph._Fold16Job * len(cases))()
    keep = []
    for J, (w, bn, k0, K, Kp, Np) in zip(arr, cases):
        wd = w.cuda()
        out = torch.full((Kp * Np * 2,), float("nan"), dtype=torch.float16, device="cuda")
        part, scale = torch.zeros(16, device="cuda"), torch.zeros(1, device="cuda")
        keep.append((wd, out, part, scale))
        J.w, J.out, J.partial, J.scale = wd.data_ptr(), out.data_ptr(), part.data_ptr(), scale.data_ptr()
        J.N, J.K, J.ld, J.k0, J.Kp, J.Np = w.shape[0], K, w.shape[1], k0, Kp, Np
        if bn is not None:
            gam, var = bn[0].cuda(), bn[1].cuda()
            keep.append((gam, var))
            J.gamma, J.var, J.eps = gam.data_ptr(), var.data_ptr(), bn[2]
    units = ctypes.c_int64()
    assert _lib.lib().ndnet_pn_fold16_check(arr, len(arr), ctypes.byref(units)) == 0
    assert units.value == 64 * 128 // 8
    dev_jobs = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda()
    assert _lib.lib().ndnet_pn_fold16_run(dev_jobs.data_ptr(), len(arr), units.value, _lib.stream_ptr(dev_jobs.device)) == 0
    torch.cuda.synchronize()
    outs = [k for k in keep if len(k) == 4]
    for (w, bn, k0, K, Kp, Np), (_, out, _, scale) in zip(cases, outs):
        fw = w[:, k0:k0 + K].cuda()
        if bn is not None:
            # pointnet_hip._bn_fold, operation by operation, on the device as the model's first fold runs it
            # (the fold kernels restate torch's device arithmetic; the CPU's division differs in the last bit)
            fw = fw * (bn[0].cuda() / torch.sqrt(bn[1].cuda() + bn[2]))[:, None]
        want, wscale = ph._frag_f16(ph._wT(fw, Kp, Np).cpu())
        assert torch.equal(scale.cpu(), wscale), (scale, wscale)
        got = out.cpu()
        diff = (got.view(torch.int16) != want.view(torch.int16)).nonzero().flatten()
        assert diff.numel() == 0, ((K, Np), diff.numel(), diff[:4].tolist(), got[diff[:4]].tolist(), want[diff[:4]].tolist())
    assert float(outs[2][3]) == 2.0 ** -14 and float(outs[3][3]) == 1.0  # 0.5 * 2^14 = 2^13; the all-zero layer: s = 0
