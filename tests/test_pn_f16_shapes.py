"""The fp16 two-slice form of the chain kernel (ndnet_pn_chain_f16_run, ndnet_pn_chain_f16_run_t32) on every
layer split, fused pair, prologue and window edge the launcher accepts: tests/test_pn_chain.py's matrix of
shapes driven through the fp16 entries (part A: everything stays inside the window), and the window itself
(part B: tiles below the upper edge, exactly on both edges, all zero, mixed within a cloud, outside only at a
deep layer or at a fused pair's second layer).

  e_hip <= 3 e_t + 1e-6 max |float64 result|,  e_t the error of torch's fp32 chain on the device

is the bound of every accuracy comparison, as in tests/test_pn_chain.py and tests/test_pn_f16_chain.py; a tile
outside the window must equal the bf16 launch (ndnet_pn_chain_run, ndnet_pn_chain_run_t32) bit for bit.  Every
case runs on both tile builds and prints ``<family> <case> tile <T>: e_f16 e_t scale ratio fallbacks``.

The inputs of every case are built on the CPU by the ``_in_*`` functions, which also state what the case
relies on: which tiles fall back (evaluated in float64 with ``_tile_maxima``, never taken from the kernel) and
that every tile maximum lies at least 1% from both window edges (B2, whose values are exact in fp32, apart).
``test_inputs_sit_where_the_cases_need_them`` asserts those claims without a GPU, so that a changed seed
cannot silently turn an in-window case into an all-fallback one; every GPU test asserts them again before it
launches anything."""
import ctypes
import math

import pytest
import torch

from test_pn_chain import (F32, NAN_BITS, X6, _Fold, _fold_parts, _gen, _Head, _head_parts, _kept, _layer,
                           _nd_rows, _report, _rows16, _run_checked, _softmax_case, _softmax_inputs, _tail_chain)
from test_pn_f16_chain import (BF16_ENTRY, F16_BUILDS, HI, LO, SHAPES, _chain_layers, _F16Case, _fallback_tiles,
                               _lower_edge_case, _tile_maxima)

F16_TILE = dict(F16_BUILDS)
TILES = (64, 32)


def _ph():
    from ndnet.models import pointnet_hip as ph
    return ph


# ---- the inputs of every case, on the CPU, with what the case relies on ----

class _In:
    """x, the chain and what is expected of its tiles: `expect` is "in" (no tile falls back), "all" (every tile
    does), a list of the clouds all of whose tiles fall back (no tile of another does), or a function of
    (fallback tiles [B][T], maxima {layer: [B][T]}, tile size) that asserts for itself."""

    def __init__(self, x, in_cols, layers, mode=0, out_cols=0, expect="in", exact_edges=False, **extra):
        self.x, self.in_cols, self.layers, self.mode, self.out_cols = x, in_cols, layers, mode, out_cols
        self.expect, self.exact_edges = expect, exact_edges
        self.__dict__.update(extra)


def _maxima(x, in_cols, layers, tile):
    """``_tile_maxima`` with a per-cloud bias [B][N] shaped for its rows."""
    return _tile_maxima(x, in_cols, [dict(L, b=L["b"][:, None, :]) if L["b"].dim() == 2 else L for L in layers], tile)


def _claims(inp):
    """Asserts, in float64, what the case relies on; -> {tile size: fallback tiles [B][T] (bool)}."""
    out = {}
    for tile in TILES:
        mx = _maxima(inp.x, inp.in_cols, inp.layers, tile)
        assert mx, "a chain with a split layer"
        bad = _fallback_tiles(mx)
        if not inp.exact_edges:
            for l, m in mx.items():
                near = ((m >= 0.99 * LO) & (m <= 1.01 * LO)) | ((m >= 0.99 * HI) & (m <= 1.01 * HI))
                assert not bool(near.any()), ("a tile maximum within 1% of a window edge", l, tile, m[near])
        e = inp.expect
        if e == "in":
            assert not bool(bad.any()), ("inputs meant to stay in the window", tile, {l: (m.min().item(), m.max().item()) for l, m in mx.items()})
        elif e == "all":
            assert bool(bad.all()), ("every tile meant to fall back", tile, bad)
        elif isinstance(e, list):
            for b in range(bad.shape[0]):
                assert bool(bad[b].all() if b in e else not bad[b].any()), (tile, b, bad)
        else:
            e(bad, mx, tile)
        out[tile] = bad
    return out


def _in_a1(N):
    g = _gen(100 + N)
    x = _nd_rows(3, N, g)
    return _In(x, 12, _tail_chain(g))


def _in_a2(N):
    """tests/test_pn_chain.py's test_pool_negative_and_mixed_sign_maxima, operand for operand."""
    g = _gen(200 + N)
    layers = _tail_chain(g, last_relu=0, zero_bias=True)
    wT, b = layers[2]["wT"], layers[2]["b"]
    neg, tiny, rest = (torch.arange(c, 256, 3) for c in (0, 1, 2))
    b[neg] = -50.0
    b[tiny] = 0.0
    csign = (torch.arange(tiny.numel()) % 2).float() * 2 - 1
    wT[:, tiny] = wT[:, tiny].abs() * 2e-6 * csign
    return _In(_nd_rows(3, N, g), 12, layers, neg=neg, tiny=tiny, rest=rest)


def _in_a3(W):
    g = _gen(401 + W)
    layers = [_layer(g, 16, 64, F32, 1, k_used=12), _layer(g, 64, 128, X6, 1), _layer(g, 128, W, X6, 0)]
    return _In(_nd_rows(3, 77, g), 12, layers)


def _fused_layers(g, n1, n2):
    return [_layer(g, 16, 64, F32, 1, k_used=12), _layer(g, 64, n1, F32, 1, fuse=True), _layer(g, n1, n2, X6, 1),
            _layer(g, n2, 32, X6, 0, n_used=29)]


def _in_a4(n1, n2):
    g = _gen(505 + n1)
    layers = _fused_layers(g, n1, n2)
    return _In(_nd_rows(3, 77, g), 12, layers, 1, 29)


def _in_a5():
    g = _gen(302)
    layers = [_layer(g, 32, 128, F32, 1, k_used=20), _layer(g, 128, 64, X6, 0)]
    return _In(_nd_rows(3, 77, g, x_ld=32), 20, layers)


def _in_a6(oc, variant):
    x, layers = _softmax_inputs(oc, variant)
    return _In(x, 12, layers, 1, oc)


def _in_a7():
    """tests/test_pn_chain.py's test_per_cloud_weights_and_bias with layer 1 split: its weights shared (the form
    rejects per-cloud split weights), its bias per cloud; layer 0's weights per cloud."""
    g = _gen(600)
    l0, l1, l2 = _layer(g, 16, 64, F32, 1, k_used=12), _layer(g, 64, 128, X6, 1), _layer(g, 128, 64, F32, 0)
    scale = torch.tensor([1.0, 2.0, 4.0])
    l0["wT"] = l0["wT"][None] * scale[:, None, None]
    l1["b"] = l1["b"][None] * scale[:, None]
    return _In(_nd_rows(3, 77, g), 12, [l0, l1, l2])


def _in_a8(scaled):
    g = _gen(800)
    x = _nd_rows(3, 33, g)
    layers = _tail_chain(g)
    return _In(x * 3e4 if scaled else x, 12, layers, expect="all" if scaled else "in")


FOLD_CASES = [(N, ld) for N in (1, 130) for ld in (4096, 4160)]


def _fold_seed(N, fold_ld):
    return 1100 + 8 * N + 2 * X6 + fold_ld  # tests/test_pn_chain.py's, relu0 = 0 (the model's case)


def _in_a9_fold(N, fold_ld, scaled):
    w0, b0, t2, w_ref, b_ref, tail, x = _fold_parts(_fold_seed(N, fold_ld), N, X6)
    l0 = dict(wT=w_ref, b=b_ref, K=16, N=64, prec=F32, relu=0, fuse=False)
    if scaled:
        x[1] *= 3e4
    return _In(x, 12, [l0] + tail, expect=[1] if scaled else "in")


def _head_seed(N):
    return 950 + N + 1000  # tests/test_pn_chain.py's "nout128"


def _in_a9_head(N, scaled):
    g = _gen(_head_seed(N))
    w_ref = _head_parts(g, 3, 100, 12, 128)[5]
    l0 = _layer(g, 16, 128, F32, 1)
    l0["wT"] = w_ref
    layers = [l0, _layer(g, 128, 64, X6, 0)]
    x = _nd_rows(3, N, g)
    if scaled:
        x[1] *= 3e4
    return _In(x, 12, layers, expect=[1] if scaled else "in")


def _in_b1(shape, B, N):
    # (seeds at which row 0, the scaled one, carries every tile's maximum at every split layer: asserted below)
    g = _gen(1040 + 10 * "ABD".index(shape) + N)
    x, in_cols, layers, mode, out_cols, _ = _lower_edge_case(shape, B, N, g, target=0.9 * HI)

    def expect(bad, mx, tile):
        for l, m in mx.items():
            assert bool(((m >= 0.8 * HI) & (m <= 0.99 * HI)).all()), (l, tile, m)
        assert not bool(bad.any())
    return _In(x, in_cols, layers, mode, out_cols, expect=expect)


def _edge_values():
    lo, hi, zero = torch.tensor(LO, dtype=torch.float32), torch.tensor(HI, dtype=torch.float32), torch.tensor(0.0)
    return [lo, torch.nextafter(lo, zero), torch.nextafter(hi, zero), hi]  # inside, outside, inside, outside


def _single_split(g, copy0=False, zero_bias=False, relu1=1):
    """16 -> 64 on the VALU, 64 -> 128 split, pooled: one window.  copy0: layer 0 copies its 12 input columns."""
    l0, l1 = _layer(g, 16, 64, F32, 1, k_used=12), _layer(g, 64, 128, X6, relu1)
    if copy0:
        l0["wT"].zero_()
        l0["wT"][torch.arange(12), torch.arange(12)] = 1.0
    if copy0 or zero_bias:
        l0["b"].zero_()
    return [l0, l1]


def _in_b2():
    g = _gen(1100)
    layers = _single_split(g, copy0=True)
    ms = _edge_values()
    x = torch.rand(4, 65, 12, generator=g)
    for b, m in enumerate(ms):
        x[b] *= m / 2
        x[b, :, 0] = m

    def expect(bad, mx, tile):
        # the copy is exact: every tile's maximum is the cloud's m, bit for bit
        assert torch.equal(mx[1], torch.stack(ms).double()[:, None].expand_as(mx[1]))
        assert ms[1].item() < LO and ms[1].item() > LO * (1 - 2.0 ** -23) and ms[2].item() < HI and ms[2].item() > HI * (1 - 2.0 ** -23)
        assert bad.tolist() == [[b in (1, 3)] * bad.shape[1] for b in range(4)]
    return _In(x, 12, layers, expect=expect, exact_edges=True)


def _in_b3(variant):
    g = _gen(1200)
    layers = _single_split(g, zero_bias=True, relu1=0 if variant == "bias" else 1)
    if variant == "zero":
        layers[1]["b"].zero_()
    x = _nd_rows(3, 65, g)
    x[0] = 0.0
    x[0, ::7, 1] = -0.0
    x[0, 3, 5:9] = -0.0
    x[1, 64] = 0.0

    def expect(bad, mx, tile):
        m = mx[1]
        assert bool((m[0] == 0).all()) and float(m[1, -1]) == 0.0 and bool((m[1, :-1] > 0).all()) and bool((m[2] > 0).all())
        assert not bool(bad.any())
    return _In(x, 12, layers, expect=expect)


def _in_b4(shape):
    g = _gen(1300 + "AD".index(shape))
    in_cols, layers, mode, out_cols = _chain_layers(shape, g, zero_bias=True)
    x = _nd_rows(3, 130, g)
    x[1, 64:128] *= 1e-6

    def expect(bad, mx, tile):
        want = torch.zeros_like(bad)
        want[1, 64 // tile: 128 // tile] = True
        assert torch.equal(bad, want), (tile, bad)
    return _In(x, in_cols, layers, mode, out_cols, expect=expect)


def _push_out(x, in_cols, layers, scaled, target):
    """Multiplies layer `scaled`'s weights (zero biases: its output scales with them) so that split layer
    `target`'s input maxima, over the tiles of both builds, sit inside [2^12, 2^13]; asserts that they do and
    that every split layer before `target` keeps its input in the window.  Random rows spread the tiles' maxima
    over more than the factor of two one weight factor can serve (a two-row tail tile sits 8 times below a full
    one), so x is first evened out, in place: the chain is positively homogeneous, and each 32-row tile's rows
    are scaled to the tiles' geometric mean at `target` -- factors of a few, which the earlier layers' windows,
    asserted too, have room for."""
    m = _maxima(x, in_cols, layers, 32)[target]
    c = (m.log().mean().exp() / m).float()
    x *= c.repeat_interleave(32, dim=1)[:, : x.shape[1], None]
    mx = [_maxima(x, in_cols, layers, tile)[target] for tile in TILES]
    lo, hi = min(m.min().item() for m in mx), max(m.max().item() for m in mx)
    assert lo > 0 and hi / lo < 1.001, ("the tiles' maxima were meant to agree", lo, hi)
    layers[scaled]["wT"] *= math.sqrt(2.0 ** 12 * 2.0 ** 13 / (lo * hi))

    def expect(bad, mx, tile):
        for l, m in mx.items():
            if l < target:
                assert bool(((m >= 1.01 * LO) & (m <= 0.99 * HI)).all()), (l, tile, m)
        m = mx[target]
        assert bool(((m >= 1.01 * 2.0 ** 12) & (m <= 0.99 * 2.0 ** 13)).all()), (target, tile, m)
        assert bool(bad.all())
    return expect


def _in_b5(shape):
    g = _gen(1400 + "AD".index(shape))
    if shape == "A":
        in_cols, layers, mode, out_cols = 12, _tail_chain(g, zero_bias=True), 0, 0
        layers[2]["b"].zero_()
    else:
        in_cols, layers, mode, out_cols = _chain_layers("D", g, zero_bias=True)
    x = _nd_rows(3, 130, g)
    last = len(layers) - 1
    return _In(x, in_cols, layers, mode, out_cols, expect=_push_out(x, in_cols, layers, last - 1, last))


def _in_b6(n1, n2):
    g = _gen(1500 + n1)
    layers = _fused_layers(g, n1, n2)
    for L in layers:
        L["b"].zero_()
    x = _nd_rows(3, 77, g)
    return _In(x, 12, layers, 1, 29, expect=_push_out(x, 12, layers, 1, 2))


TAIL_N = [1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 130]
WIDTHS = [32, 64, 128, 256, 512, 768, 1024]
PAIRS = [(128, 64), (256, 128), (512, 256)]
SOFTMAX = [(oc, v) for v in ("plain", "range90", "pad100") for oc in (1, 2, 16, 17, 29, 32, 33, 64, 301)]
EDGE_CASES = [(s, B, N) for s in "AD" for B, N in SHAPES]

ALL_INPUTS = ([("A1", _in_a1, (N,)) for N in TAIL_N] + [("A2", _in_a2, (N,)) for N in (17, 65)]
              + [("A3", _in_a3, (W,)) for W in WIDTHS] + [("A4", _in_a4, p) for p in PAIRS] + [("A5", _in_a5, ())]
              + [("A6", _in_a6, c) for c in SOFTMAX] + [("A7", _in_a7, ())] + [("A8", _in_a8, (s,)) for s in (False, True)]
              + [("A9 fold", _in_a9_fold, c + (s,)) for c in FOLD_CASES for s in (False, True)]
              + [("A9 head", _in_a9_head, (N, s)) for N in (1, 130) for s in (False, True)]
              + [("B1", _in_b1, c) for c in EDGE_CASES] + [("B2", _in_b2, ())] + [("B3", _in_b3, (v,)) for v in ("zero", "bias")]
              + [("B4", _in_b4, (s,)) for s in "AD"] + [("B5", _in_b5, (s,)) for s in "AD"] + [("B6", _in_b6, p) for p in PAIRS])


def test_inputs_sit_where_the_cases_need_them():
    """Every case's inputs, in float64 on the CPU: the tiles that fall back are the ones the case names (none
    in part A but the scaled variants of A8 and A9), every tile maximum is at least 1% from both edges, and
    B2's are the four fp32 values at the edges exactly.  Part A's split layers see maxima of about 3.9 .. 580."""
    lo, hi = float("inf"), 0.0
    for fam, build, args in ALL_INPUTS:
        inp = build(*args)
        bad = _claims(inp)
        print(f"{fam} {args}: fallback tiles {[int(bad[t].sum()) for t in TILES]} of {[bad[t].numel() for t in TILES]}")
        if fam.startswith("A") and inp.expect == "in":
            for tile in TILES:
                for m in _maxima(inp.x, inp.in_cols, inp.layers, tile).values():
                    lo, hi = min(lo, m.min().item()), max(hi, m.max().item())
    print(f"part A, in-window cases: tile maxima {lo:.3g} .. {hi:.3g}")
    assert 16 * LO < lo and hi < HI / 2, (lo, hi)  # well inside: nothing in part A passes by falling back


def test_pooled_fused_pair_is_rejected():
    """A4's chain without its tail -- the fp32 64 -> n1 produced in chunks into a pooled split n1 -> n2 -- would
    max-pool before the second layer's window is known: NDNET_ERR_ARG from both entries, on host memory."""
    from ndnet import _lib
    ph = _ph()
    for n1, n2 in PAIRS:
        dims = [(16, 64, F32), (64, n1, F32), (n1, n2, X6)]
        bufs = [(torch.zeros(K * N * 2), torch.zeros(N)) for K, N, _ in dims]
        ch = ph._build_chain(5, 12, [(w, 0, b, K, N, p) for (w, b), (K, N, p) in zip(bufs, dims)], [1, 1, 1], 0,
                             gmax=torch.zeros(2, n2), fuse=(1,))
        x, planes, scale, counter = torch.zeros(2, 5, 12), torch.zeros(n1 * n2), torch.ones(1), torch.zeros(1, dtype=torch.int32)
        ch.x = x.data_ptr()
        ext = ph._F16()
        ext.w16[2], ext.scale[2], ext.fallbacks = planes.data_ptr(), scale.data_ptr(), counter.data_ptr()
        for entry, tile in F16_BUILDS:
            assert getattr(_lib.lib(), entry)(ctypes.byref(ch), ctypes.byref(ext), 2, None) == -20, (entry, n1, n2)


# ---- the device side ----

class _ShapeCase(_F16Case):
    """tests/test_pn_f16_chain.py's case whose ``run`` takes either form's entry: an fp16 entry is launched with
    the sentinels of ``_Case.run`` (columns past N of gmax keep their bits, `out` starts as NaN), its fallback
    tiles go to ``self.fallbacks`` and the counter must read 0 afterwards.  ``self.last`` keeps the fp32 result
    of the latest launch for comparisons bit for bit."""

    def __init__(self, x, in_cols, layers, mode, out_cols=0, gmax_extra=0):
        super().__init__(x, in_cols, layers, mode, out_cols, gmax_extra)
        self.in_cols, self.fallbacks = in_cols, None

    def _result(self):
        return (self.gmax[:, : self.n_last] if self.mode == 0 else self.out).clone()

    def run(self, entry):
        if entry not in F16_TILE:
            got = super().run(entry)
            self.last = self._result()
            return got
        from ndnet import _lib
        if self.mode == 0:
            self.gmax.fill_(float("-inf"))
            if self.gmax_ld > self.n_last:
                self.gmax[:, self.n_last:].view(torch.int32).fill_(NAN_BITS)
        else:
            self.out.fill_(float("nan"))
        stream = _lib.stream_ptr(self.x.device)
        rc = getattr(_lib.lib(), entry)(ctypes.byref(self.ch), ctypes.byref(self.ext), self.B, stream)
        assert rc == 0, f"{entry} returned {rc}"
        self.fallbacks = _lib.lib().ndnet_pn_take_f16_fallbacks(self.counter.data_ptr(), stream)
        assert self.fallbacks >= 0 and int(self.counter.item()) == 0, "the counter is handed over and reset"
        if self.mode == 0 and self.gmax_ld > self.n_last:
            assert bool((self.gmax[:, self.n_last:].view(torch.int32) == NAN_BITS).all()), "columns past N of gmax were written"
        self.last = self._result()
        return self.last.double().cpu()

    def torch32(self):
        """torch's fp32 chain on the device again (the run behind e_t), in float64 on the CPU."""
        dev = [L["dev"] if "dev" in L else (L["wT"].cuda(), L["b"].cuda()) for L in self.layers]
        relus = [L["relu"] for L in self.layers]
        if self.mode == 0:
            t = torch.full((self.B, self.n_last), float("-inf"), device="cuda")
            _ph()._chain_torch(self.x, self.N, self.in_cols, dev, relus, 0, gmax=t)
        else:
            t = torch.empty((self.B, self.N, self.out_cols), device="cuda")
            _ph()._chain_torch(self.x, self.N, self.in_cols, dev, relus, 1, out=t, out_cols=self.out_cols)
        return t.double().cpu()


def _case(inp, **kw):
    return _ShapeCase(inp.x, inp.in_cols, inp.layers, inp.mode, inp.out_cols, **kw)


def _bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _check(name, c, want, cols=None):
    """Both fp16 builds: the fallback tiles counted are the float64 evaluation's, the result is finite and
    within the bound; `cols` as in ``_Case.check``."""
    bad = []
    bound = 3 * c.e_t + 1e-6 * c.scale
    for entry, tile in F16_BUILDS:
        got = c.run(entry)
        n_want = int(want[tile].sum())
        e = (got - c.ref).abs().max().item()
        print(f"{name} tile {tile}: e_f16 {e:.3e} e_t {c.e_t:.3e} scale {c.scale:.3e} ratio {e / max(c.e_t, 1e-300):.2f} "
              f"fallbacks {c.fallbacks} expected {n_want}")
        if not (bool(torch.isfinite(got).all()) and e <= bound) or c.fallbacks != n_want:
            bad.append((name, entry, e, c.e_t, c.scale, c.fallbacks, n_want))
        for cname, (idx, e_t_c) in (cols or {}).items():
            e_c = (got[:, idx] - c.ref[:, idx]).abs().max().item()
            s_c = c.ref[:, idx].abs().max().item()
            print(f"{name} tile {tile} {cname}: e_f16 {e_c:.3e} e_t {e_t_c:.3e} scale {s_c:.3e} ratio {e_c / max(e_t_c, 1e-300):.2f}")
            if not e_c <= 3 * e_t_c + 1e-6 * s_c:
                bad.append((name, entry, cname, e_c, e_t_c, s_c))
    assert not bad, bad


def _check_all_fall_back(name, c, want):
    """Both builds: every tile falls back (counted) and the result is the bf16 launch's, bit for bit."""
    for entry, tile in F16_BUILDS:
        assert bool(want[tile].all())
        c.run(entry)
        got = c.last
        c.run(BF16_ENTRY[tile])
        print(f"{name} tile {tile}: fallbacks {c.fallbacks} expected {want[tile].numel()}, bit for bit against the bf16 launch")
        assert c.fallbacks == want[tile].numel(), (entry, c.fallbacks)
        assert _bits_equal(got, c.last), f"{name} {entry}: differs from the bf16 launch"
        assert bool(torch.isfinite(got).all())


# ---- part A: shapes that stay inside the window ----

@pytest.mark.gpu
@pytest.mark.parametrize("N", TAIL_N)
def test_a1_point_count_tails(N):
    """One tile, the tile boundaries of both builds, several tiles with a ragged tail."""
    inp = _in_a1(N)
    _check(f"A1 tails N={N}", _case(inp), _claims(inp))


@pytest.mark.gpu
@pytest.mark.parametrize("N", [17, 65])
def test_a2_pool_negative_and_mixed_sign_maxima(N):
    """The pooled split layer without a ReLU: fma(acc, 2^-4 2^-s, bias) into the float atomic max with negative
    maxima (bias -50) and maxima within 1e-3 of 0 of both signs, the padded rows of the tail tile (exactly
    `bias` there, above the tiny negative columns' real rows) not winning, and 64 more gmax columns keeping
    their bits.  The bound holds per column subset too, each with its own scale and torch error."""
    inp = _in_a2(N)
    want = _claims(inp)
    c = _case(inp, gmax_extra=64)
    assert (c.ref[:, inp.neg] < 0).all(), "the -50 columns' maxima are negative"
    t = c.ref[:, inp.tiny]
    assert (t.abs() < 1e-3).all() and (t < 0).any() and (t > 0).any(), "tiny maxima of both signs"
    et = (c.torch32() - c.ref).abs()
    cols = {n: (i, et[:, i].max().item()) for n, i in (("bias -50", inp.neg), ("tiny", inp.tiny), ("plain", inp.rest))}
    _check(f"A2 negmax N={N}", c, want, cols)


@pytest.mark.gpu
@pytest.mark.parametrize("W", WIDTHS)
def test_a3_pooled_layer_widths(W):
    """Every plain_layer split of either build as the pooled last layer, two planes in, no ReLU (K = 128)."""
    inp = _in_a3(W)
    _check(f"A3 width W={W}", _case(inp), _claims(inp))


@pytest.mark.gpu
@pytest.mark.parametrize("n1,n2", PAIRS)
def test_a4_generic_fused_pairs(n1, n2):
    """An fp32 P that is not layer 0 (64 -> n1, in 64-column chunks) into a split Q n1 -> n2 -- fused_pair<1 | 2 |
    4> by Q's width --, then n2 -> 29 of 32 split and log_softmax."""
    inp = _in_a4(n1, n2)
    _check(f"A4 fused {n1}-{n2}", _case(inp), _claims(inp))


@pytest.mark.gpu
def test_a5_mfma_layer0_feeds_a_split_layer():
    """Layer 0 from the LDS input tile on the fp32 MFMA (32 -> 128, 20 input columns of 32): its plain_layer
    epilogue writes the two planes and the window word of the split 128 -> 64 behind it."""
    inp = _in_a5()
    c = _case(inp)
    assert c.ch.x_ld == 32 and c.ch.in_cols == 20
    _check("A5 mfma0 wide_input", c, _claims(inp))


@pytest.mark.gpu
@pytest.mark.parametrize("oc,variant", SOFTMAX)
def test_a6_log_softmax_widths(oc, variant):
    """log_softmax from a split last layer over 1 .. 301 columns, logits reaching +-90, padded columns with a
    bias of +100 outside the sum (at 32 and 64 columns there is no padded one: the plain case again)."""
    inp = _in_a6(oc, variant)
    c = _softmax_case(oc, variant, case=_ShapeCase)
    assert torch.equal(c.x.cpu(), inp.x)
    if variant == "range90" and oc > 1:
        assert c.scale > 80
    _check(f"A6 softmax oc={oc} {variant}", c, _claims(inp))


@pytest.mark.gpu
def test_a7_per_cloud_operands():
    """A per-cloud bias (stride N) on a split layer, behind per-cloud fp32 layer-0 weights at stride 1024 and
    then at a padded stride; the clouds' operands differ by factors of two, so a wrong cloud index shows."""
    inp = _in_a7()
    want = _claims(inp)
    c = _case(inp)
    assert c.ch.L[0].w_cloud_stride == 1024 and c.ch.L[1].bias_cloud_stride == 128 and c.ch.L[1].w_cloud_stride == 0
    _check("A7 per-cloud stride 1024", c, want)
    f0 = _ph()._frag(inp.layers[0]["wT"].cuda())
    padded = torch.full((3, f0.shape[1] + 64), float("nan"), device="cuda")
    padded[:, : f0.shape[1]] = f0
    c.ch.L[0].w, c.ch.L[0].w_cloud_stride = padded.data_ptr(), padded.stride(0)
    _check("A7 per-cloud stride 1088", c, want)
    assert (c.ref[1] - c.ref[0]).abs().max() > 1.0  # the clouds' results do differ


@pytest.mark.gpu
@pytest.mark.parametrize("scaled", [False, True], ids=["in_window", "all_fall_back"])
@pytest.mark.parametrize("count", [8, 2500])
def test_a8_clear_rearms_exactly_its_range(count, scaled):
    """clear / clear_count from the fp16 body and, with the inputs times 3e4, from the re-run of a tile that fell
    back: exactly `count` floats are -inf afterwards, the 8 behind them keep their values."""
    inp = _in_a8(scaled)
    want = _claims(inp)
    c = _case(inp)
    fresh = torch.arange(count + 8, dtype=torch.float32) + 1
    buf = fresh.cuda()
    c.ch.clear, c.ch.clear_count = buf.data_ptr(), count
    for entry, tile in F16_BUILDS:
        buf.copy_(fresh)
        c.run(entry)
        assert c.fallbacks == int(want[tile].sum())
        assert bool((buf[:count] == float("-inf")).all())
        assert torch.equal(buf[count:].cpu(), fresh[count:])
    if scaled:
        _check_all_fall_back(f"A8 clear {count} x3e4", c, want)
    else:
        _check(f"A8 clear {count}", c, want)


def _published_equal(name, c, tile, entry, want, buffers, base):
    """The scaled variant of a prologue case: cloud 1 falls back in every tile, so the prologue runs twice
    there.  What it published for every cloud (`buffers`, pads and sentinels included) is the bf16 launch's bit
    for bit; cloud 1's result is the bf16 launch's, the other clouds' the unscaled fp16 launch's (`base`)."""
    for t in buffers:
        t.view(torch.int32).fill_(NAN_BITS)
    c.run(entry)
    got, pub = c.last, [t.clone() for t in buffers]
    n = c.fallbacks
    for t in buffers:
        t.view(torch.int32).fill_(NAN_BITS)
    c.run(BF16_ENTRY[tile])
    print(f"{name} tile {tile}: fallbacks {n} expected {int(want[tile].sum())}, publication bit for bit against the bf16 launch")
    assert n == int(want[tile].sum())
    for a, b_ in zip(pub, buffers):
        assert _bits_equal(a, b_), f"{name} {entry}: the prologue's publication differs from the bf16 launch's"
    assert _bits_equal(got[1], c.last[1]), f"{name} {entry}: the fallen-back cloud differs from the bf16 launch"
    assert _bits_equal(got[[0, 2]], base[[0, 2]]), f"{name} {entry}: an untouched cloud changed"


@pytest.mark.gpu
@pytest.mark.parametrize("N,fold_ld", FOLD_CASES)
def test_a9_fold_t2_prologue(N, fold_ld):
    """fold_t2 with per-cloud t2 and publication ahead of a split layer 1: the chain's output, fold_out_w and
    fold_out_b within the bound, rows 12..15 and the pads kept (``_Fold.run``); then cloud 1 times 3e4."""
    inp = _in_a9_fold(N, fold_ld, False)
    want = _claims(inp)
    f = _Fold(_fold_seed(N, fold_ld), N, 0, X6, fold_ld, prefill=NAN_BITS, case=_ShapeCase)
    assert torch.equal(f.x, inp.x) and all(torch.equal(a["wT"], b_["wT"]) for a, b_ in zip(f.layers, inp.layers))
    name, bad, base = f"A9 fold ld={fold_ld} N={N}", [], {}
    for entry, tile in F16_BUILDS:
        f.run(name, entry, bad)
        print(f"{name} tile {tile}: fallbacks {f.c.fallbacks} expected 0")
        assert f.c.fallbacks == 0 == int(want[tile].sum())
        base[tile] = f.c.last
    assert not bad, bad
    scaled = _in_a9_fold(N, fold_ld, True)
    want = _claims(scaled)
    f.c.x.copy_(scaled.x.cuda())
    for entry, tile in F16_BUILDS:
        _published_equal(name + " cloud 1 x3e4", f.c, tile, entry, want, [f.out_w, f.out_b], base[tile])


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1, 130])
def test_a9_head_prologue_mfma_layer0(N):
    """head_* with layer 0 on the MFMA path (16 -> 128 per cloud, every workgroup stores and reloads it) ahead of
    a split 128 -> 64: the output, t1 and the published L[0].w within the bound, pads kept, rows kin..15 exactly
    zero (``_Head.check``'s assertions); then cloud 1 times 3e4."""
    inp = _in_a9_head(N, False)
    want = _claims(inp)
    g = _gen(_head_seed(N))
    hd = _Head(g, 3, 100, 12, 128)
    layers = [hd.layer0(g), _layer(g, 128, 64, X6, 0)]
    x = _nd_rows(3, N, g)
    assert torch.equal(x, inp.x) and all(torch.equal(a["wT"], b_["wT"]) for a, b_ in zip(layers, inp.layers))
    c = _ShapeCase(x, 12, layers, 0)
    hd.attach(c)
    name, bad, base, rows = f"A9 head nout128 N={N}", [], {}, _rows16(hd.nout)
    for entry, tile in F16_BUILDS:
        hd.wbuf.view(torch.int32).fill_(NAN_BITS)
        hd.t1.view(torch.int32).fill_(NAN_BITS)
        _run_checked(c, name, entry, bad)
        print(f"{name} tile {tile}: fallbacks {c.fallbacks} expected 0")
        assert c.fallbacks == 0 == int(want[tile].sum())
        base[tile] = c.last
        assert _kept(hd.t1[hd.B * 9:]) and _kept(hd.wbuf[:, hd.size:]), f"{entry}: pads were written"
        _report(f"{name} {entry[9:]} t1", hd.t1[: hd.B * 9].view(hd.B, 9).double().cpu(), hd.t1_ref, hd.e_t1, bad)
        w = hd.wbuf[:, : hd.size].cpu()
        _report(f"{name} {entry[9:]} L[0].w", w.double(), _ph()._frag(hd.w_ref), hd.e_w, bad)
        assert bool((w[:, rows >= hd.kin] == 0).all()), f"{entry}: rows kin..15 are not exactly 0"
    assert not bad, bad
    scaled = _in_a9_head(N, True)
    want = _claims(scaled)
    c.x.copy_(scaled.x.cuda())
    for entry, tile in F16_BUILDS:
        _published_equal(name + " cloud 1 x3e4", c, tile, entry, want, [hd.t1, hd.wbuf], base[tile])


# ---- part B: the window itself ----

@pytest.mark.gpu
@pytest.mark.parametrize("shape,B,N", EDGE_CASES)
def test_b1_upper_edge(shape, B, N):
    """Every split layer's tile maximum at 0.9 * 2^11 (``_lower_edge_case`` aimed below the upper edge): 16 v
    reaches 2^15 in the high plane, which fp16 holds; no tile falls back and the bound holds."""
    inp = _in_b1(shape, B, N)
    _check(f"B1 upper edge {shape} {B}x{N}", _case(inp), _claims(inp))


@pytest.mark.gpu
def test_b2_exact_edges():
    """One window (layer 0 copies its input, exactly): tile maxima of 2^-4 and the fp32 value below 2^11 are
    inside, the fp32 value below 2^-4 and 2^11 itself are outside.  The outside clouds' tiles are counted and
    equal the bf16 launch bit for bit; the inside clouds keep the bound."""
    inp = _in_b2()
    want = _claims(inp)
    full = _case(inp)
    c = _ShapeCase(inp.x[[0, 2]], inp.in_cols, inp.layers, 0)  # the references of the clouds inside
    bound = 3 * c.e_t + 1e-6 * c.scale
    bad = []
    for entry, tile in F16_BUILDS:
        got = full.run(entry)
        raw, n = full.last, full.fallbacks
        full.run(BF16_ENTRY[tile])
        e = (got[[0, 2]] - c.ref).abs().max().item()
        print(f"B2 exact edges tile {tile}: e_f16 {e:.3e} e_t {c.e_t:.3e} scale {c.scale:.3e} ratio {e / max(c.e_t, 1e-300):.2f} "
              f"fallbacks {n} expected {int(want[tile].sum())} ({want[tile].sum(dim=1).tolist()} per cloud)")
        if n != int(want[tile].sum()) or not e <= bound:
            bad.append((entry, n, e, bound))
        for b in (1, 3):
            if not _bits_equal(raw[b], full.last[b]):
                bad.append((entry, f"cloud {b} differs from the bf16 launch"))
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["zero", "bias"])
def test_b3_all_zero_tiles(variant):
    """A cloud of zero rows (some -0.0) and a cloud whose tail tile is one zero row: a maximum of 0 is inside the
    window.  The zero cloud's pooled row is layer 1's bias exactly -- zero behind a ReLU, or nonzero without."""
    inp = _in_b3(variant)
    want = _claims(inp)
    c = _case(inp)
    _check(f"B3 zero tiles {variant}", c, want)
    b1 = inp.layers[1]["b"]
    assert bool(b1.any()) == (variant == "bias")
    for entry, tile in F16_BUILDS:
        c.run(entry)
        assert torch.equal(c.last[0].cpu(), b1), f"{entry}: the zero cloud's row is not the bias"


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["A", "D"])
def test_b4_mixed_clouds(shape):
    """Rows 64..127 of cloud 1 (of 130) times 1e-6: those tiles fall back, the cloud's other tiles do not.  A
    (pooled): the cloud's maximum over both kinds of tile keeps the bound.  D (log_softmax): the rows of fallen-
    back tiles are the bf16 launch's bit for bit, the other rows keep the bound (with torch's error on them)."""
    inp = _in_b4(shape)
    want = _claims(inp)
    c = _case(inp)
    if inp.mode == 0:
        _check(f"B4 mixed {shape}", c, want)
        return
    err_t = (c.torch32() - c.ref).abs()
    bad = []
    for entry, tile in F16_BUILDS:
        got = c.run(entry)
        raw, n = c.last, c.fallbacks
        c.run(BF16_ENTRY[tile])
        fell = want[tile].repeat_interleave(tile, dim=1)[:, : c.N]  # [B][N]: the row's tile fell back
        assert 0 < int(fell.sum()) < fell.numel()
        e, e_t = (got - c.ref).abs()[~fell].max().item(), err_t[~fell].max().item()
        scale = c.ref[~fell].abs().max().item()
        print(f"B4 mixed {shape} tile {tile}: e_f16 {e:.3e} e_t {e_t:.3e} scale {scale:.3e} ratio {e / max(e_t, 1e-300):.2f} "
              f"fallbacks {n} expected {int(want[tile].sum())}")
        if n != int(want[tile].sum()) or not e <= 3 * e_t + 1e-6 * scale or not bool(torch.isfinite(got).all()):
            bad.append((entry, n, e, e_t, scale))
        if not _bits_equal(raw[fell.cuda()], c.last[fell.cuda()]):
            bad.append((entry, "rows of fallen-back tiles differ from the bf16 launch"))
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["A", "D"])
def test_b5_only_the_deepest_split_layer_outside(shape):
    """The last split layer's input at 2^12 .. 2^13, every earlier one in the window: the tile is found out late,
    after fp16 layers ran, and still leaves nothing behind -- pooled maxima (A) and rows (D) are the bf16
    launch's bit for bit."""
    inp = _in_b5(shape)
    _check_all_fall_back(f"B5 deep layer {shape}", _case(inp), _claims(inp))


@pytest.mark.gpu
@pytest.mark.parametrize("n1,n2", PAIRS)
def test_b6_only_a_fused_second_layer_outside(n1, n2):
    """A4's chain with the fused pair's second layer alone outside: its input arrives chunk by chunk and is
    tested only after the pair closes."""
    inp = _in_b6(n1, n2)
    _check_all_fall_back(f"B6 fused {n1}-{n2}", _case(inp), _claims(inp))
