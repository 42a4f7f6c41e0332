"""ndnet_pn_pool12_run (chain C as one per-cloud 12 -> F layer) at the C ABI,
against float64 (tests/pool12_ref.py).

Per column the kernel is held to 15 * 2^-24 * max_n sum_k |x_nk| |Wc_kf| +
2^-23 |g3| (``pool12_ref.bound``: twelve FMAs, Wc rounded once, the bias and
its addition) and, over all columns, to three times the error of torch's
layered fp32 chain C on the same input plus 1e-6 (the allowance of
tests/test_model_precision.py)."""
import ctypes

import pytest
import torch

import pool12_ref as R

NAN_BITS = 0x7FC0BEEF  # sentinel of what the kernel must neither read nor write
# one point; odd N, several clouds; Fp > F; the workload; Fp = 32 (half a workgroup's columns); more than 1024 points
SHAPES = [(1, 1, 64), (3, 77, 64), (2, 130, 100), (16, 1000, 768), (2, 33, 16), (1, 1100, 64)]
_cases = {}


def _ph():
    from ndnet.models import pointnet_hip as ph
    return ph


def _sentinel(*shape):
    return torch.full(shape, NAN_BITS, dtype=torch.int32, device="cuda").view(torch.float32)


def _rows(x, x_ld):
    """x [B,N,12] as rows of x_ld floats, the columns past 12 a NaN sentinel."""
    out = _sentinel(x.shape[0], x.shape[1], x_ld)
    out[..., :12] = x
    return out


class _Case:
    """One shape's inputs (on the GPU), float64 reference and torch fp32 error, made once."""

    def __init__(self, B, N, F, integers=False):
        ph = _ph()
        self.B, self.N, self.F, self.Fp = B, N, F, ph._npad(F)
        g = torch.Generator().manual_seed(1000 * B + N + F)

        def rnd(*shape, scale=1.0):
            if integers:  # small integers: every product and sum below is exact in fp32 and in three bf16 planes
                return torch.randint(-1, 2, shape, generator=g).float()
            return torch.randn(shape, generator=g) * scale

        w_tail, b_tail = torch.zeros(128, self.Fp), torch.zeros(self.Fp)
        w_tail[:, :F], b_tail[:F] = rnd(128, F, scale=128 ** -0.5), rnd(F, scale=0.1)
        t = dict(w0=rnd(B, 12, 64, scale=0.3), b0=rnd(B, 64, scale=0.1), w_mid=rnd(64, 128, scale=0.125),
                 b_mid=rnd(128, scale=0.1), w_tail=w_tail, b_tail=b_tail)
        x = torch.cat((torch.rand((B, N, 3), generator=g) * 20 - 10, torch.randn((B, N, 9), generator=g)), dim=2)
        self.x = (torch.randint(-3, 4, (B, N, 12), generator=g).float() if integers else x).cuda()
        for k, v in t.items():
            setattr(self, k, v.cuda())
        self.w0f = ph._frag(torch.nn.functional.pad(self.w0, (0, 0, 0, 4)))  # [B, 1024]: K padded 12 -> 16
        assert self.w0f.shape == (B, 1024)
        self.layers = [(self.w0, self.b0), (self.w_mid, self.b_mid), (self.w_tail, self.b_tail)]
        self.ref = None

    def reference(self):
        if self.ref is None:
            ph = _ph()
            wc, bc = R.collapse(self.w0, self.b0, self.w_mid, self.b_mid, self.w_tail, self.b_tail)
            g64 = R.pooled(self.x.double(), wc, bc)
            g32 = torch.full((self.B, self.Fp), float("-inf"), device="cuda")
            ph._chain_torch(self.x, self.N, 12, self.layers, (0, 0, 0), 0, gmax=g32)  # torch's layered fp32 chain C
            self.ref = (g64, R.bound(self.x, wc, g64), (g32.double() - g64).abs().max().item())
        return self.ref

    def run(self, x_ld=12, x=None):
        """The launch into the g3 slice of a sentinel-filled max-pool buffer -> the whole buffer."""
        from ndnet import _lib
        xr = _rows(self.x if x is None else x, x_ld)
        gbuf = _sentinel(self.B, 2048 + self.Fp)
        g3 = gbuf[:, 2048:]
        rc = _lib.lib().ndnet_pn_pool12_run(xr.data_ptr(), x_ld, self.N, self.w0f.data_ptr(), 1024, self.b0.data_ptr(),
                                            64, self.w_mid.data_ptr(), self.b_mid.data_ptr(), self.w_tail.data_ptr(),
                                            self.b_tail.data_ptr(), self.F, self.Fp, g3.data_ptr(), gbuf.stride(0),
                                            self.B, _lib.stream_ptr(xr.device))
        _lib.check(rc, "ndnet_pn_pool12_run")
        torch.cuda.synchronize()
        return gbuf


def _case(B, N, F, integers=False):
    key = (B, N, F, integers)
    if key not in _cases:
        _cases[key] = _Case(B, N, F, integers)
    return _cases[key]


@pytest.mark.gpu
@pytest.mark.parametrize("x_ld", [12, 16])
@pytest.mark.parametrize("B,N,F", SHAPES)
def test_pool12_against_float64(B, N, F, x_ld):
    c = _case(B, N, F)
    g64, lim, e_t = c.reference()
    gbuf = c.run(x_ld)
    g3 = gbuf[:, 2048:]
    err = (g3.double() - g64).abs()
    e_new = err.max().item()
    print(f"B={B} N={N} F={F} x_ld={x_ld}: e_new {e_new:.3e} e_torch32 {e_t:.3e} "
          f"worst error / bound {(err / lim.clamp_min(1e-300))[:, :F].max().item():.3f}")
    assert bool((err <= lim).all())
    assert e_new <= 3 * e_t + 1e-6
    # the padding columns F .. Fp - 1 (the FC kernels read them): exactly 0.0, no -0
    assert torch.equal(g3[:, F:].view(torch.int32), torch.zeros_like(g3[:, F:], dtype=torch.int32))
    # nothing outside the slice is written
    assert torch.equal(gbuf[:, :2048].view(torch.int32), _sentinel(B, 2048).view(torch.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("B,N,F", [(3, 77, 64), (16, 1000, 768)])
def test_two_runs_are_bit_equal(B, N, F):
    c = _case(B, N, F)
    a, b = c.run(), c.run()
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("split", [1, 0], ids=["x6", "fp32"])
def test_nan_and_inf_rows_as_the_chain_c_launch(split):
    """One NaN row, one +-Inf row and one all-NaN cloud: g3 bit-equal to the
    layered chain-C launch on the same inputs.  Small integer weights and
    inputs make every product and sum of both exact (|y| < 2^24; a layer's
    activations fit three bf16 planes), so the two agree to the bit wherever
    they treat the rows alike: a NaN never wins the maximum, a row with an
    infinity takes no part, a cloud without a usable row stays at -inf, and
    the padding columns (F = 100 in 128) are 0 or -inf with the rest."""
    ph = _ph()
    B, N, F = 3, 77, 100
    c = _case(B, N, F, integers=True)
    x = c.x.clone()
    x[0, 5, 3] = float("nan")
    x[0, 9, 0], x[0, 9, 7] = float("inf"), float("-inf")
    x[2] = float("nan")
    # without the special rows the two launches must already agree (the data is exact in both)
    got = {}
    for name, xin in (("plain", c.x), ("special", x)):
        gchain = torch.full((B, 2048 + c.Fp), float("-inf"), device="cuda")  # the chain's atomic maxima need it armed
        fr = ph._frag_x6 if split else ph._frag
        layers = [(c.w0f, c.w0f.stride(0), c.b0, 16, 64), (fr(c.w_mid), 0, c.b_mid, 64, 128, split),
                  (fr(c.w_tail), 0, c.b_tail, 128, c.Fp, split)]
        ch = ph._build_chain(N, 12, layers, (0, 0, 0), 0, gmax=gchain[:, 2048:])
        ph._run_chain(ch, xin.contiguous())
        g3 = c.run(12, xin)[:, 2048:]
        torch.cuda.synchronize()
        got[name] = g3
        assert torch.equal(g3.view(torch.int32), gchain[:, 2048:].contiguous().view(torch.int32)), name
    s = got["special"]
    assert bool(torch.isinf(s[2]).all()) and bool((s[2] < 0).all())          # the all-NaN cloud
    assert bool(torch.isfinite(s[:2]).all())                                  # NaN / Inf rows never reach g3
    assert torch.equal(s[1], got["plain"][1])
    wc, bc = R.collapse(c.w0, c.b0, c.w_mid, c.b_mid, c.w_tail, c.b_tail)
    keep = [n for n in range(N) if n not in (5, 9)]
    assert torch.equal(s[0].double(), R.pooled(c.x[:1, keep].double(), wc[:1], bc[:1])[0])  # exact: the other 75 rows


def test_invalid_arguments_are_rejected_before_any_launch():
    """-20 for every argument the header rules out (nothing is launched, so no GPU is needed)."""
    from ndnet import _lib
    buf = (ctypes.c_float * 16)()
    p = ctypes.addressof(buf)
    ok = dict(x=p, x_ld=12, n=10, w0f=p, w0_stride=1024, b0=p, b0_stride=64, w_mid=p, b_mid=p, w_tail=p, b_tail=p,
              F=100, Fp=128, gmax=p, gmax_ld=128, batch=2)
    bad = [dict(x=None), dict(w0f=None), dict(b0=None), dict(w_mid=None), dict(b_mid=None), dict(w_tail=None),
           dict(b_tail=None), dict(gmax=None), dict(x_ld=8), dict(x_ld=13), dict(n=0), dict(w0_stride=960),
           dict(b0_stride=32), dict(F=0), dict(F=129), dict(Fp=100), dict(gmax_ld=127), dict(batch=0),
           dict(batch=65536)]
    for edit in bad:
        a = {**ok, **edit}
        rc = _lib.lib().ndnet_pn_pool12_run(a["x"], a["x_ld"], a["n"], a["w0f"], a["w0_stride"], a["b0"], a["b0_stride"],
                                            a["w_mid"], a["b_mid"], a["w_tail"], a["b_tail"], a["F"], a["Fp"],
                                            a["gmax"], a["gmax_ld"], a["batch"], None)
        assert rc == -20, edit
