"""ndnet_pn_pool12_tail_run (chain C's 12 -> F launch from the fold's composed tail W23, b23) at the C
ABI, against float64 of the LAYERED chain C (x W0[b] + b0[b], w_mid, w_tail, the maximum over the
points: tests/pool12_ref.py), never against the kernel or the composed tail themselves.

Shapes: n in {1, 15, 16, 17, 130} points (one point, one short of a 16-point tile, the tile, one past
it, nine tiles over the 16 waves) times model widths F in {32, 64, 96, 768}, padded by the project's
rule to Fp = 32 (half of a workgroup's 64 columns), 64 (one workgroup), 128 (two, the second ragged:
columns 96 .. 127 are padding) and 768 (the workload's twelve).  A padded width of 96 itself is no
width the kernels take: both entries reject it.  B = 3 clouds with their own W0[b], b0[b]; cloud 0
carries a NaN row and cloud 1 a row with +inf and -inf, which take no part in the maximum (with one
point those two clouds keep no row and every column is -inf).  The launch writes the g3 slice of a
buffer of NaN sentinels whose rows are longer than Fp.

Bounds.  Per column 15 * 2^-24 * max_n sum_k |x_nk| |Wc_kf| + 2^-23 |g3| (``pool12_ref.bound``:
twelve FMAs, Wc rounded once from a float64 product, the bias and its addition), and over all
columns e_hip <= 3 e_t + 1e-6 * max |float64|, e_t the error of torch's layered fp32 chain C on the
same rows on the device (tests/test_pn_chain.py's criterion).

ndnet_pn_pool12_run on the same inputs must return the bits it returned before the composed tail
existed: tests/golden/pool12_parent_entry.npz, recorded from the parent commit's build."""
import os

import numpy as np
import pytest
import torch

import pool12_ref as R

NAN_BITS = 0x7FC0BEEF  # sentinel of what the kernel must neither read nor write
POINTS = [1, 15, 16, 17, 130]
WIDTHS = [32, 64, 96, 768]
B = 3
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pool12_parent_entry.npz")
_cases = {}


def _ph():
    from ndnet.models import pointnet_hip as ph
    return ph


def _sentinel(*shape):
    return torch.full(shape, NAN_BITS, dtype=torch.int32, device="cuda").view(torch.float32)


class Case:
    """One shape's inputs (made on the CPU: the recording depends on their bits), float64 reference of
    the layered chain on the rows that count, and torch's fp32 error on the same rows; made once."""

    def __init__(self, n, F):
        ph = _ph()
        self.n, self.F, self.Fp = n, F, ph._npad(F)
        g = torch.Generator().manual_seed(7000 + 10 * n + F)

        def rnd(*shape, scale=1.0):
            return torch.randn(shape, generator=g) * scale

        w_tail, b_tail = torch.zeros(128, self.Fp), torch.zeros(self.Fp)
        w_tail[:, :F], b_tail[:F] = rnd(128, F, scale=128 ** -0.5), rnd(F, scale=0.1)
        t = dict(w0=rnd(B, 12, 64, scale=0.3), b0=rnd(B, 64, scale=0.1), w_mid=rnd(64, 128, scale=0.125),
                 b_mid=rnd(128, scale=0.1), w_tail=w_tail, b_tail=b_tail)
        x = torch.cat((torch.rand((B, n, 3), generator=g) * 20 - 10, torch.randn((B, n, 9), generator=g)), dim=2)
        self.keep = [list(range(n)) for _ in range(B)]
        r0, r1 = min(5, n - 1), min(9, n - 1)
        x[0, r0, 3] = float("nan")
        x[1, r1, 0], x[1, r1, 7] = float("inf"), float("-inf")
        self.keep[0].remove(r0)
        self.keep[1].remove(r1)
        self.x = x.cuda()
        for k, v in t.items():
            setattr(self, k, v.cuda())
        self.w0f = ph._frag(torch.nn.functional.pad(self.w0, (0, 0, 0, 4)))  # [B, 1024]: K padded 12 -> 16
        self.ref = None

    def reference(self):
        """(g64 [B, Fp], per-column bound, e_t, max |float64|): a cloud without a usable row is -inf."""
        if self.ref is None:
            ph = _ph()
            wc, bc = R.collapse(self.w0, self.b0, self.w_mid, self.b_mid, self.w_tail, self.b_tail)
            g64 = torch.full((B, self.Fp), float("-inf"), dtype=torch.float64, device="cuda")
            lim = torch.zeros_like(g64)
            e_t = 0.0
            for b in range(B):
                if not self.keep[b]:
                    continue
                xb = self.x[b:b + 1, self.keep[b]]
                g64[b] = R.pooled(xb.double(), wc[b:b + 1], bc[b:b + 1])[0]
                lim[b] = R.bound(xb, wc[b:b + 1], g64[b:b + 1])[0]
                g32 = torch.full((1, self.Fp), float("-inf"), device="cuda")
                layers = [(self.w0[b:b + 1], self.b0[b:b + 1]), (self.w_mid, self.b_mid), (self.w_tail, self.b_tail)]
                ph._chain_torch(xb, xb.shape[1], 12, layers, (0, 0, 0), 0, gmax=g32)  # torch's layered fp32 chain C
                e_t = max(e_t, (g32.double() - g64[b:b + 1]).abs().max().item())
            finite = g64[torch.isfinite(g64)]
            self.ref = (g64, lim, e_t, finite.abs().max().item() if finite.numel() else 0.0)
        return self.ref

    def run(self, tail, x_ld=12):
        """One launch into the g3 slice of a sentinel-filled max-pool buffer -> the whole buffer."""
        from ndnet import _lib
        ph = _ph()
        xr = _sentinel(B, self.n, x_ld)
        xr[..., :12] = self.x
        gbuf = _sentinel(B, 2048 + self.Fp + 32)
        g3 = gbuf[:, 2048:2048 + self.Fp]
        head = (xr.data_ptr(), x_ld, self.n, self.w0f.data_ptr(), 1024, self.b0.data_ptr(), 64)
        if tail:
            w23 = ph._prod64(self.w_mid, self.w_tail)
            b23 = ph._prod64(self.b_mid[None, :], self.w_tail, self.b_tail).reshape(-1)
            rc = _lib.lib().ndnet_pn_pool12_tail_run(*head, w23.data_ptr(), b23.data_ptr(), self.Fp, g3.data_ptr(),
                                                     gbuf.stride(0), B, _lib.stream_ptr(xr.device))
        else:
            rc = _lib.lib().ndnet_pn_pool12_run(*head, self.w_mid.data_ptr(), self.b_mid.data_ptr(),
                                                self.w_tail.data_ptr(), self.b_tail.data_ptr(), self.F, self.Fp,
                                                g3.data_ptr(), gbuf.stride(0), B, _lib.stream_ptr(xr.device))
        _lib.check(rc, "ndnet_pn_pool12_tail_run" if tail else "ndnet_pn_pool12_run")
        torch.cuda.synchronize()
        return gbuf


def case(n, F):
    if (n, F) not in _cases:
        _cases[(n, F)] = Case(n, F)
    return _cases[(n, F)]


def _check_pads(c, gbuf):
    pads = torch.cat((gbuf[:, :2048], gbuf[:, 2048 + c.Fp:]), dim=1)
    assert torch.equal(pads.view(torch.int32), _sentinel(*pads.shape).view(torch.int32)), "written outside the slice"


@pytest.mark.gpu
@pytest.mark.parametrize("F", WIDTHS)
@pytest.mark.parametrize("n", POINTS)
def test_tail_entry_against_float64(n, F):
    c = case(n, F)
    g64, lim, e_t, scale = c.reference()
    gbuf = c.run(tail=True, x_ld=16 if n % 2 else 12)
    g3 = gbuf[:, 2048:2048 + c.Fp]
    live = torch.isfinite(g64)
    assert bool(torch.isfinite(g3[live]).all()), "a NaN or an infinite row reached the maximum"
    err = torch.where(live, (g3.double() - g64).abs(), torch.zeros_like(g64))
    e_hip = err.max().item()
    worst = (err / lim.clamp_min(1e-300))[:, :F][live[:, :F]]
    print(f"n={n} F={F} Fp={c.Fp}: e_hip {e_hip:.3e} e_torch32 {e_t:.3e} max|f64| {scale:.3g} "
          f"worst error / bound {worst.max().item() if worst.numel() else 0.0:.3f}")
    assert bool((err <= lim).all())
    assert e_hip <= 3 * e_t + 1e-6 * scale
    # a cloud with no usable row: -inf in every column, padding included (as the chain's pooled epilogue)
    assert bool((g3[~live] == float("-inf")).all())
    for b in range(B):
        assert bool(live[b].all()) == bool(c.keep[b]) and bool(live[b].any()) == bool(c.keep[b])
        if c.keep[b]:  # the padding columns F .. Fp - 1 (the FC kernels read them): exactly 0.0, no -0
            assert torch.equal(g3[b, F:].view(torch.int32), torch.zeros(c.Fp - F, dtype=torch.int32, device="cuda"))
    _check_pads(c, gbuf)


@pytest.mark.gpu
@pytest.mark.parametrize("n,F", [(17, 96), (130, 768)])
def test_two_runs_are_bit_equal(n, F):
    c = case(n, F)
    assert torch.equal(c.run(True).view(torch.int32), c.run(True).view(torch.int32))


@pytest.mark.gpu
def test_layered_entry_returns_the_recorded_bits():
    """ndnet_pn_pool12_run, same arguments, on every shape above: the parent commit's output, bit for bit."""
    want = np.load(GOLDEN)
    diff = 0
    for n in POINTS:
        for F in WIDTHS:
            c = case(n, F)
            gbuf = c.run(tail=False)
            got = gbuf[:, 2048:2048 + c.Fp].cpu().numpy()
            rec = want[f"n{n}_F{F}"]
            assert got.shape == rec.shape and got.dtype == rec.dtype
            assert np.array_equal(got.view(np.int32), rec.view(np.int32)), (n, F)
            _check_pads(c, gbuf)
            new = c.run(tail=True)[:, 2048:2048 + c.Fp].cpu().numpy()
            diff += int((new.view(np.int32) != got.view(np.int32)).sum())
    print(f"elements in which the two entries differ (the order of the float64 sums): {diff}")


@pytest.mark.gpu
def test_rejected_padded_width():
    """Fp = 96 is neither 32 nor a multiple of 64: -20 from both entries, nothing launched."""
    from ndnet import _lib
    c = case(16, 96)
    z = torch.zeros(64 * 96, dtype=torch.float64, device="cuda")
    g = _sentinel(B, 96)
    head = (c.x.data_ptr(), 12, c.n, c.w0f.data_ptr(), 1024, c.b0.data_ptr(), 64)
    assert _lib.lib().ndnet_pn_pool12_tail_run(*head, z.data_ptr(), z.data_ptr(), 96, g.data_ptr(), 96, B, None) == -20
    assert _lib.lib().ndnet_pn_pool12_run(*head, c.w_mid.data_ptr(), c.b_mid.data_ptr(), c.w_tail.data_ptr(),
                                          c.b_tail.data_ptr(), 96, 96, g.data_ptr(), 96, B, None) == -20
    torch.cuda.synchronize()
    assert torch.equal(g.view(torch.int32), _sentinel(B, 96).view(torch.int32))
