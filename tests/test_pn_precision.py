"""The reduced split-bf16 modes of the chain kernel at the C ABI
(ndnet_pn_layer.prec 2 = "x3": h h' + h m' + m h'; prec 3 = "bf16": h h';
include/ndnet_pointnet.h), on both builds, against a float64 emulator.

The emulator (``_emu64``) takes, for a reduced layer, the fp32 activations
the previous layer produced and the fp32 W^T, forms h = bf16(x) and
m = bf16(x - h) of both (round to nearest even: torch's bfloat16 cast), sums
the mode's kept products in float64, adds the bias, applies ReLU and rounds
to fp32; prec 0 layers are plain float64 as in ``test_pn_chain._ref64``.

With ref = the untruncated float64 chain, e_emu = max |emu - ref|,
e_hip = max |HIP - ref| and e_t, scale as in test_pn_chain.py, every case is
held to
    e_emu / 3 <= e_hip <= 3 e_emu + 3 e_t + 1e-6 scale.
The factor 3 is the project's allowance for summation order
(test_pn_chain.py:5-9); it also covers the rare activation whose bf16
rounding flips on an fp32 last-bit difference.  The lower half shows that
terms were really dropped (e_emu is > 15x the fp32 level in both modes); the
upper half that none was lost besides (a kernel without, say, h m' sits
40-400x above 3 e_emu at these shapes).

Figures measured on an MI355X: DESIGN.md §3, "Reduced split-bf16 modes"."""
import ctypes

import pytest
import torch

from test_pn_chain import BUILDS, F32, X6, _arg_block, _gen, _layer, _nd_rows, _ph, _ref64, _with_layer

X3, BF16 = 2, 3
MODES = [pytest.param(X3, id="x3"), pytest.param(BF16, id="bf16")]
# the dropped terms of one product, relative to |a| |w|: from |x - h| <= 2^-9 |x| and
# |x - h - m| <= 2^-18 |x| (round to nearest even)
C_DROP = {X3: 3.02 * 2.0 ** -18, BF16: 2.0 ** -8 + 2.0 ** -18}


def _hm(x32):
    """fp32 -> its bf16 planes h and m, as float64."""
    h = x32.to(torch.bfloat16).float()
    m = (x32 - h).to(torch.bfloat16).float()
    return h.double(), m.double()


def _emu64(x, in_cols, layers, mode, out_cols):
    """The chain with its reduced layers' products truncated as the kernel
    truncates them, everything else in float64."""
    h = torch.nn.functional.pad(x[..., :in_cols].double(), (0, layers[0]["K"] - in_cols))
    for L in layers:
        b = L["b"].double()
        if L["prec"] in (X3, BF16):
            ah, am = _hm(h.float())
            wh, wm = _hm(L["wT"])
            y = torch.matmul(ah, wh)
            if L["prec"] == X3:
                y = y + torch.matmul(ah, wm) + torch.matmul(am, wh)
            h = y + b
        else:
            h = torch.matmul(h, L["wT"].double()) + b
        if L["relu"]:
            h = torch.relu(h)
        if L["prec"] in (X3, BF16):
            h = h.float().double()
    return h.amax(dim=1) if mode == 0 else torch.log_softmax(h[..., :out_cols], dim=2)


class _Case:
    """Device operands, the argument block and the three references (float64,
    emulator, torch fp32 on the device) of one chain; built once per case."""

    def __init__(self, x, in_cols, layers, mode, out_cols=0):
        ph = _ph()
        self.x = x.cuda()
        self.mode, self.out_cols, self.layers = mode, out_cols, layers
        B, N, _ = x.shape
        self.B, self.N, self.n_last = B, N, layers[-1]["N"]
        self.ref = _ref64(x, in_cols, layers, mode, out_cols)
        self.emu = _emu64(x, in_cols, layers, mode, out_cols)
        self.e_emu = (self.emu - self.ref).abs().max().item()
        relus = [L["relu"] for L in layers]
        dev_layers = [(L["wT"].cuda(), L["b"].cuda()) for L in layers]
        if mode == 0:
            t = torch.full((B, self.n_last), float("-inf"), device="cuda")
            ph._chain_torch(self.x, N, in_cols, dev_layers, relus, 0, gmax=t)
        else:
            t = torch.empty((B, N, out_cols), device="cuda")
            ph._chain_torch(self.x, N, in_cols, dev_layers, relus, 1, out=t, out_cols=out_cols)
        self.e_t = (t.double().cpu() - self.ref).abs().max().item()
        self.scale = self.ref.abs().max().item()
        self.keep, hip = [], []
        for L, (w, b) in zip(layers, dev_layers):
            f = ph._frag_x6(w) if L["prec"] else ph._frag(w)  # one layout for prec 1, 2 and 3
            self.keep += [f, b]
            hip.append((f, 0, b, L["K"], L["N"], L["prec"]))
        self.gmax = torch.empty((B, self.n_last), device="cuda") if mode == 0 else None
        self.out = torch.empty((B, N, out_cols), device="cuda") if mode == 1 else None
        self.ch = ph._build_chain(N, in_cols, hip, relus, mode, gmax=self.gmax, out_cols=out_cols,
                                  fuse=tuple(i for i, L in enumerate(layers) if L["fuse"]))
        self.ch.x, self.ch.x_ld = self.x.data_ptr(), self.x.stride(1)
        self.ch.out = self.out.data_ptr() if mode == 1 else None

    def run(self, entry):
        from ndnet import _lib
        if self.mode == 0:
            self.gmax.fill_(float("-inf"))
        else:
            self.out.fill_(float("nan"))
        rc = getattr(_lib.lib(), entry)(ctypes.byref(self.ch), self.B, _lib.stream_ptr(self.x.device))
        assert rc == 0, f"{entry} returned {rc}"
        torch.cuda.synchronize()
        return (self.gmax if self.mode == 0 else self.out).double().cpu()

    def check(self, name, elementwise=None):
        """Both builds inside the sandwich; `elementwise`: also |HIP - ref| <=
        elementwise + 3 e_t + 1e-6 scale in every element."""
        bad = []
        for entry in BUILDS:
            got = self.run(entry)
            assert torch.isfinite(got).all(), f"{name} {entry}: non-finite output"
            err = (got - self.ref).abs()
            e_hip = err.max().item()
            slack = 3 * self.e_t + 1e-6 * self.scale
            print(f"{name} {entry[9:]}: e_hip {e_hip:.3e} e_emu {self.e_emu:.3e} e_t {self.e_t:.3e} "
                  f"scale {self.scale:.3e} e_hip/e_emu {e_hip / max(self.e_emu, 1e-300):.2f}")
            if not self.e_emu / 3 <= e_hip <= 3 * self.e_emu + slack:
                bad.append((name, entry, "sandwich", e_hip, self.e_emu, self.e_t, self.scale))
            if elementwise is not None:
                over = (err - (elementwise + slack)).max().item()
                print(f"  elementwise: max (err - bound) {over:.3e}, max err / bound "
                      f"{(err / (elementwise + slack)).max().item():.2f}")
                if not over <= 0:
                    bad.append((name, entry, "elementwise", over))
        assert not bad, bad


def _three_layers(g, prec, N):
    """16 -> 64 fp32 (layer 0 on the VALU), 64 -> 128 in the mode with ReLU, 128 -> N in the mode, pooled."""
    return [_layer(g, 16, 64, F32, 1, k_used=12), _layer(g, 64, 128, prec, 1), _layer(g, 128, N, prec, 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("prec", MODES)
@pytest.mark.parametrize("N", [64, 128, 1024])
def test_single_reduced_layer(N, prec):
    """16 -> 64 fp32, then one layer 64 -> N in the mode, pooled, no ReLU: the
    sandwich, and the rigorous bound of the dropped terms in every element --
    c (|a| |W|), |a| the float64 activations, the maximum over the points of
    each column (a maximum moves by at most the largest error under it)."""
    g = _gen(1100 + N + prec)
    layers = [_layer(g, 16, 64, F32, 1, k_used=12), _layer(g, 64, N, prec, 0)]
    x = _nd_rows(3, 77, g)
    c = _Case(x, 12, layers, 0)
    a = torch.relu(torch.nn.functional.pad(x.double(), (0, 4)) @ layers[0]["wT"].double() + layers[0]["b"].double())
    aw = (a.abs() @ layers[1]["wT"].double().abs()).amax(dim=1)  # [B][N]
    print(f"emulation / rigorous bound: {((c.emu - c.ref).abs() / (C_DROP[prec] * aw)).max().item():.2f}")
    c.check(f"single N={N} prec {prec}", elementwise=C_DROP[prec] * aw)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", MODES)
@pytest.mark.parametrize("N", [32, 64, 128, 256, 512, 768, 1024])
def test_pooled_layer_widths(N, prec):
    """Every plain_layer split as the pooled last layer (K = 128, no ReLU), the
    two-column-block form at 512 and 1024 included, behind the two-step 64 -> 128."""
    g = _gen(1200 + N + prec)
    _Case(_nd_rows(3, 77, g), 12, _three_layers(g, prec, N), 0).check(f"width N={N} prec {prec}")


@pytest.mark.gpu
@pytest.mark.parametrize("prec", MODES)
@pytest.mark.parametrize("points", [1, 17, 33, 65])
def test_point_tails(points, prec):
    g = _gen(1300 + points + prec)
    _Case(_nd_rows(3, points, g), 12, _three_layers(g, prec, 256), 0).check(f"tails {points} prec {prec}")


@pytest.mark.gpu
@pytest.mark.parametrize("prec", MODES)
@pytest.mark.parametrize("tail", [False, True], ids=["pooled", "then_softmax"])
@pytest.mark.parametrize("n1,n2", [(128, 64), (256, 128), (512, 256)])
def test_fused_pairs(n1, n2, tail, prec):
    """P 64 -> n1 in the mode produced in 64-column chunks into Q n1 -> n2 in
    the mode (512 -> 256: the software-pipelined pair of the 64-point build),
    pooled, or followed by a 32-wide layer in the mode and log_softmax."""
    g = _gen(1400 + n1 + 4 * tail + prec)
    layers = [_layer(g, 16, 64, F32, 1, k_used=12), _layer(g, 64, n1, prec, 1, fuse=True), _layer(g, n1, n2, prec, 1)]
    if tail:
        layers.append(_layer(g, n2, 32, prec, 0, n_used=29))
    c = _Case(_nd_rows(3, 77, g), 12, layers, 1 if tail else 0, out_cols=29 if tail else 0)
    c.check(f"fused {n1}-{n2} tail={tail} prec {prec}")


@pytest.mark.gpu
@pytest.mark.parametrize("prec", MODES)
def test_reduced_mode_is_not_a_silent_x6(prec):
    """K = 128, N = 1024: the mode's result differs from a prec 1 run of the same block."""
    g = _gen(1500 + prec)
    c = _Case(_nd_rows(3, 77, g), 12, _three_layers(g, prec, 1024), 0)
    for entry in BUILDS:
        got = c.run(entry)
        for l in (1, 2):
            c.ch.L[l].prec = X6
        x6 = c.run(entry)
        for l in (1, 2):
            c.ch.L[l].prec = prec
        differing = int((got != x6).sum())
        print(f"{entry[9:]} prec {prec}: {differing} of {got.numel()} elements differ from x6, "
              f"max |diff| {(got - x6).abs().max().item():.3e}")
        assert differing >= 1


# ---- argument checks: rejected before any HIP call, so these run without a GPU ----

def _all_split(prec, then=None):
    """The valid block of test_pn_chain._arg_block with both split layers at `prec`, then `then(spec)`."""
    def edit(spec):
        _with_layer(2, prec=prec)(spec)
        _with_layer(3, prec=prec)(spec)
        if then is not None:
            then(spec)
    return edit


def _layer0_split(spec):
    _with_layer(0, K=32, prec=X3)(spec)
    spec.update(in_cols=12)


def _k48(spec):
    _with_layer(1, N=64)(spec)
    _with_layer(2, K=48)(spec)
    spec.update(fuse=())


ARG_CASES = {
    "prec 1 and prec 2 in one chain": _with_layer(3, prec=X3),
    "prec 4": _all_split(4),
    "prec 2 on layer 0": _all_split(X3, _layer0_split),
    "prec 3 with K = 48": _all_split(BF16, _k48),
}


@pytest.mark.parametrize("case", sorted(ARG_CASES))
def test_inconsistent_precision_blocks_are_rejected(case, capfd):
    """NDNET_ERR_ARG (-20) from both entry points, before anything is launched."""
    assert _arg_block(ARG_CASES[case]) == [-20, -20]
    assert capfd.readouterr().err.count("invalid argument") == 2


@pytest.mark.gpu
def test_uniform_prec_2_block_is_accepted():
    """The block the rejected ones are edits of, all split layers at prec 2, is valid (it runs, on zeros)."""
    assert _arg_block(_all_split(X3), device="cuda") == [0, 0]
