"""The train-mode kernels (include/ndnet_train.h) called at the C ABI through
``ndnet._lib.lib()``, path by path, against the same operation in float64.

Reference of every numeric comparison: the operation written out in float64
torch.  Baseline e_t: the error of torch's own fp32 op (``torch.bmm``,
``F.batch_norm(training=True)`` with autograd, ``F.linear``, ``log_softmax``,
``torch.max(x, 2)``) on the same device against that float64 result.  Bound,
per output tensor:  max |hip - ref64| <= FACTOR e_t + 1e-6 max |ref64|  (max-abs:
one wrong element fails), FACTOR = 3 as in test_pn_chain.py (summation order
only) unless the table below says otherwise and why.  Every case prints
``RATIO <family> <case>: e_hip e_t scale ratio`` before it asserts.

Reductions that accumulate in double and round once (chan_sum, row_sum,
BatchNorm's dgamma / dbeta / dbias, the FC db) equal the float64 sum S of the
same fp32 terms up to one fp32 rounding:  |out - S| <= 2^-23 |S| + 2^-40 sum |x|.

Every output lies between two pads of NAN_BITS words that must stay untouched
(rows past M, columns N..ldc, the gap columns of sum_parts_2d, elements past
numel in Adam, pool rows past B).

The NDNET_TR_* switches are read once per process: the ``*_child_*`` tests run
the relevant cases of this file again in a fresh child per group of switches."""
import ctypes
import math
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

NAN_BITS = 0x7FC0BEEF  # the sentinel of words a kernel must not touch
PAD = 256              # sentinel words on either side of every buffer
EPS, MOM = 1e-5, 0.1

# factor of e_t in the bound, per kernel family (3: summation order only)
FACTOR = {"gemm": 3.0, "sum_parts": 3.0, "bn": 3.0, "fc": 3.0, "softmax": 3.0, "nll": 3.0, "transform": 3.0,
          "adam": 3.0,
          # BatchNorm's backward over B = 2 rows: xhat = +-s with 1 - s^2 = eps invstd^2, and
          # dpre = gamma invstd (g0 - g1) / 2 (1 - s^2) is what is left of terms 1 / (eps invstd^2) ~ 1e3 .. 1e5
          # times larger: torch and the kernel both return that cancellation's rounding noise, and the ratio
          # of two noises is not a matter of summation order.  Measured: up to 20.8 (B2 K1024 N1), e_hip
          # within 5e-3 of the tensor's scale (the existing suite's tolerance at B = 2); 64 = 3 x that.
          "fc_b2_bwd": 64.0,
          # dgamma over B = 2 rows is s (g0 - g1) with s = d / sqrt(d^2 + eps), d = (y0 - y1) / 2: no
          # cancellation, but ds/dd = eps / (d^2 + eps)^1.5 reaches 1 / sqrt(eps) = 316 where d^2 ~ eps, so in
          # a channel whose two rows nearly agree the forward's rounding error in y (a K-term fp32 dot product,
          # ~1e-7 |y|, different in torch's F.linear and in the kernel) is amplified a few hundred times and is
          # the whole of the tensor's maximum error.  e_hip / e_t is then the ratio of two implementations' y
          # errors in that one channel.  Measured: 7.33 once (B2 K1024 N65, e_hip 5.8e-6 of the scale), every
          # other B = 2 dgamma within 3; 24 = 3 x that.  At B >= 3 dgamma keeps the factor 3.
          "fc_b2_dgamma": 24.0}


@pytest.fixture(autouse=True)
def _need_gpu(request):
    if request.node.get_closest_marker("gpu") and not torch.cuda.is_available():
        pytest.skip("no GPU")


def _L():
    from ndnet import _lib
    return _lib


def _lib():
    return _L().lib()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _gen(seed):
    return torch.Generator().manual_seed(seed)


class Buf:
    """n 4-byte words of device memory between two pads of NAN_BITS, the words
    themselves NAN_BITS until written; `off` words of extra offset (off = 1: a
    base that is not 16-byte aligned)."""

    def __init__(self, n, dtype=torch.float32, off=0, device="cuda"):
        self.n, self.lo = n, PAD + off
        self.raw = torch.full((PAD + off + n + PAD,), NAN_BITS, dtype=torch.int32, device=device)
        self.words = self.raw[self.lo:self.lo + n]
        self.t = self.words.view(dtype)
        self.ptr = self.t.data_ptr()

    @classmethod
    def of(cls, x, off=0):
        x = x.contiguous()
        b = cls(x.numel() * x.element_size() // 4, x.dtype, off, x.device)
        b.t.copy_(x.reshape(-1))
        return b

    def surround_ok(self):
        return bool((self.raw[:self.lo] == NAN_BITS).all()) and bool((self.raw[self.lo + self.n:] == NAN_BITS).all())

    def written(self):
        return not bool((self.words == NAN_BITS).any())


def _guards(bufs, what):
    for name, b in bufs.items():
        if b is not None:
            assert b.surround_ok(), f"{what}: words outside {name} were written"


def _cmp(fam, name, hip, ref, t32, bad):
    """e_hip <= FACTOR e_t + 1e-6 max |ref|; prints the figures, appends a failure to `bad`."""
    hip, ref, t32 = hip.double(), ref.double(), t32.double()
    assert hip.shape == ref.shape == t32.shape, (name, hip.shape, ref.shape, t32.shape)
    fin = bool(torch.isfinite(hip).all())
    e_hip = (hip - ref).abs().max().item() if fin else float("inf")
    e_t = (t32 - ref).abs().max().item()
    scale = ref.abs().max().item()
    print(f"RATIO {fam} {name}: e_hip {e_hip:.3e} e_t {e_t:.3e} scale {scale:.3e} "
          f"ratio {e_hip / e_t if e_t > 0 else (0.0 if e_hip == 0 else float('inf')):.2f}"
          f"{' (below 1e-6 scale)' if e_hip <= 1e-6 * scale else ''}")
    if not e_hip <= FACTOR[fam] * e_t + 1e-6 * scale:
        bad.append((name, e_hip, e_t, scale))


def _sum_once(name, out, S, sabs, bad):
    """out == the float64 sum S of the same fp32 terms, rounded once: 2^-23 |S| + 2^-40 sum |x|."""
    out, S, sabs = out.double(), S.double(), sabs.double()
    err = (out - S).abs()
    lim = 2.0 ** -23 * S.abs() + 2.0 ** -40 * sabs
    worst = (err - lim).max().item()
    print(f"SUM {name}: max err {err.max().item():.3e}, max (err - bound) {worst:.3e}")
    if not bool((err <= lim).all()):
        bad.append((name, "sum-once", err.max().item(), worst))


# ---------------------------------------------------------------- BatchNorm

def _first_max(z):
    """amax over the points and the smallest index that attains it (z [B][C][N])."""
    N = z.shape[2]
    m = z.amax(2, keepdim=True)
    idx = torch.where(z == m, torch.arange(N, device=z.device), N).amin(2)
    return m.squeeze(2), idx


def _bn_plain(y, gamma, beta):
    mu = y.mean((0, 2))
    var = ((y - mu[None, :, None]) ** 2).mean((0, 2))
    inv = 1.0 / torch.sqrt(var + EPS)
    return (y - mu[None, :, None]) * inv[None, :, None] * gamma[None, :, None] + beta[None, :, None], mu, var, inv


def _bn_inputs(B, C, N, relu, pool, seed):
    """y with a scale and offset per channel, gamma of both signs, every eighth
    channel (from 2) with gamma 0.01 and beta -5 (every z < 0); pool mode: two or
    three equal planted extremes per (cloud, channel); relu: no float64 z within
    1e-4 max |z| of zero."""
    g = _gen(seed)
    y = torch.randn(B, C, N, generator=g) * (0.5 + 3 * torch.rand(1, C, 1, generator=g))
    y = y + 2 * torch.randn(1, C, 1, generator=g)
    gamma = (0.5 + torch.rand(C, generator=g)) * torch.where(torch.arange(C) % 2 == 1, -1.0, 1.0)
    beta = 0.5 * torch.randn(C, generator=g)
    low = torch.arange(C) % 8 == 2
    gamma[low], beta[low] = 0.01, -5.0
    pts = None
    if pool:
        pts = sorted({5, 1500, N - 1}) if N > 1501 else sorted({5 % N, 6 % N, N - 1})
        ext = torch.where(gamma[None, :] > 0, y.amax(2) + 0.5, y.amin(2) - 0.5)
        y[:, :, pts] = ext[:, :, None]
    y, gamma, beta = y.cuda(), gamma.cuda(), beta.cuda()
    if relu:
        std = y.std((0, 2)) if B * N > 1 else torch.ones(C, device="cuda")
        for _ in range(10):
            z = _bn_plain(y.double(), gamma.double(), beta.double())[0]
            near = z.abs() < 1e-4 * z.abs().max()
            if not bool(near.any()):
                break
            away = torch.where(z >= 0, 1.0, -1.0) * torch.sign(gamma.double())[None, :, None]
            y = torch.where(near, y + (0.02 * away * std[None, :, None]).float(), y)
        z = _bn_plain(y.double(), gamma.double(), beta.double())[0]
        assert not bool((z.abs() < 1e-4 * z.abs().max()).any()), "inputs: a float64 z at rounding level of zero"
    return y, gamma, beta, pts


def _bn_ref(y, gamma, beta, rm, rv, relu, pool, dz, dtype, idx=None):
    """Forward and backward of the block in `dtype`, written out (float64: the reference)."""
    B, C, N = y.shape
    M = B * N
    y = y.to(dtype).requires_grad_()
    gamma, beta = gamma.to(dtype).requires_grad_(), beta.to(dtype).requires_grad_()
    z, mu, var, inv = _bn_plain(y, gamma, beta)
    if relu:
        z = torch.relu(z)
    r = {}
    if pool:
        if idx is None:
            idx = _first_max(z.detach())[1]
        r["idx"] = idx
        out = z.gather(2, idx[:, :, None]).squeeze(2)
    else:
        out = z
    out.backward(dz.to(dtype))
    unb = var * M / (M - 1) if M > 1 else var
    r.update(out=out.detach(), mean=mu.detach(), invstd=inv.detach(),
             rmean=(1 - MOM) * rm.to(dtype) + MOM * mu.detach(),
             rvar=(1 - MOM) * rv.to(dtype) + MOM * unb.detach(), dy=y.grad, dgamma=gamma.grad, dbeta=beta.grad)
    return r


def _bn_torch(y, gamma, beta, rm, rv, relu, pool, dz, idx):
    """torch's fp32 ops: F.batch_norm(training=True) with autograd, torch.max(x, 2)."""
    y = y.clone().requires_grad_()
    gamma, beta = gamma.clone().requires_grad_(), beta.clone().requires_grad_()
    rm, rv = rm.clone(), rv.clone()
    z = F.batch_norm(y, rm, rv, gamma, beta, True, MOM, EPS)
    if relu:
        z = torch.relu(z)
    if pool:
        out = torch.max(z, 2)[0].detach()
        z.gather(2, idx[:, :, None]).squeeze(2).backward(dz)  # the gradient at the reference's (first) maximum
    else:
        out = z.detach()
        z.backward(dz)
    var, mean = torch.var_mean(y.detach(), (0, 2), unbiased=False)
    return dict(out=out, mean=mean, invstd=torch.rsqrt(var + EPS), rmean=rm, rvar=rv, dy=y.grad, dgamma=gamma.grad,
                dbeta=beta.grad)


def _bn_hip(y, gamma, beta, rm, rv, relu, pool, dz, offs):
    B, C, N = y.shape
    lib = _lib()
    b = dict(y=Buf.of(y, offs.get("y", 0)), z=None if pool else Buf(B * C * N, off=offs.get("z", 0)),
             pool=Buf(B * C) if pool else None, idx=Buf(B * C, torch.int32) if pool else None,
             mean=Buf(C), invstd=Buf(C), rmean=Buf.of(rm), rvar=Buf.of(rv), gamma=Buf.of(gamma), beta=Buf.of(beta),
             nbt=Buf.of(torch.tensor([7], dtype=torch.int64, device="cuda")),
             dz=Buf.of(dz, offs.get("dz", 0)), dy=Buf(B * C * N, off=offs.get("dy", 0)), dgamma=Buf(C), dbeta=Buf(C),
             dbias=Buf(C))
    p = lambda k: b[k].ptr if b[k] is not None else None  # noqa: E731
    rc = lib.ndnet_tr_bn_fwd(p("y"), p("z"), p("mean"), p("invstd"), p("rmean"), p("rvar"), p("gamma"), p("beta"), B, C,
                             N, EPS, MOM, relu, p("pool"), p("idx"), p("nbt"), _st())
    assert rc == 0, f"bn_fwd returned {rc}"
    rc = lib.ndnet_tr_bn_bwd(p("dz"), p("y"), p("mean"), p("invstd"), p("gamma"), p("beta"), p("dy"), p("dgamma"),
                             p("dbeta"), p("dbias"), B, C, N, relu, p("idx"), _st())
    assert rc == 0, f"bn_bwd returned {rc}"
    torch.cuda.synchronize()
    _guards(b, "bn")
    for k in ("z", "pool", "idx", "mean", "invstd", "dy", "dgamma", "dbeta", "dbias"):
        assert b[k] is None or b[k].written(), f"bn: {k} not fully written"
    assert int(b["nbt"].t[0]) == 8, "batches_tracked += 1"
    r = {k: b[k].t.clone() for k in ("mean", "invstd", "rmean", "rvar", "dgamma", "dbeta", "dbias")}
    r["dy"] = b["dy"].t.view(B, C, N).clone()
    if pool:
        r["out"], r["idx"] = b["pool"].t.view(B, C).clone(), b["idx"].t.view(B, C).clone().long()
    else:
        r["out"] = b["z"].t.view(B, C, N).clone()
    return r


# name: (B, N, word offsets of y / z / dy / dz, pool mode too)
BN_WALKS = {
    "vector_cached": (2, 36, {}, True),
    "scalar_cached_N37": (2, 37, {}, True),
    "scalar_cached_N1": (3, 1, {}, True),
    "scalar_cached_B70_N3": (70, 3, {}, False),
    "scalar_cached_y_misaligned": (2, 36, {"y": 1}, True),
    "scalar_cached_z_dy_misaligned": (2, 36, {"z": 1, "dy": 1}, True),
    "dz_misaligned_fallback": (2, 36, {"dz": 1}, False),
    "uncached_N5464": (3, 5464, {}, True),
    "uncached_N5463": (3, 5463, {}, True),
    "boundary_16384": (4, 4096, {}, True),
    "pool_B64_N5": (64, 5, {}, True),
    "pool_B1": (1, 36, {}, True),
}
BN_CASES = [(w, C, relu, pool) for w in BN_WALKS for C in (3, 512) for relu in (0, 1) for pool in (0, 1)
            if (BN_WALKS[w][3] or not pool) and not (w.startswith("pool_") and not pool)]


@pytest.mark.gpu
@pytest.mark.parametrize("walk,C,relu,pool", BN_CASES, ids=[f"{w}-C{C}-relu{r}-pool{p}" for w, C, r, p in BN_CASES])
def test_bn_fwd_bwd(walk, C, relu, pool):
    """k_tr_bn_fwd / k_tr_bn_bwd, every path: the vector cached walk; the scalar
    cached walk, by N (N % 4 != 0) and by alignment (y, or z and dy, 4 bytes
    into a buffer); the backward's dz-misaligned fallback; the uncached plain and
    pooled walk (B N just above 16384, N % 4 == 0 and != 0: the running maximum
    flushed when the cloud changes, grad_at in pool mode) and the boundary
    B N = 16384; on both workgroup sizes (C = 3: 1024 threads, C = 512: 512
    threads); gamma of both signs, ReLU on and off.  Pool mode has planted
    first-maximum ties (two or three equal extremes per cloud and channel in
    different threads, float4s and strides of the walk: pool_idx = the smallest,
    dy gets the pooled gradient there only), a channel whose every z <= 0 under
    ReLU (pool 0.0, index 0, zero gradient) and all-negative without (the
    ordered-key encoding of negative floats), B = 64 and B = 1.  All outputs:
    z or pool + pool_idx, mean, invstd, running statistics (unbiased variance),
    batches_tracked, dy, dgamma, dbeta against float64; dgamma / dbeta / dbias
    as sums rounded once of the kernel's own terms.  (In pool mode there is no
    z, so `scalar_cached_z_dy_misaligned` takes the vector walk forward and the
    scalar walk only backward, through dy; `scalar_cached_y_misaligned` is scalar
    both ways.)"""
    B, N, offs, _ = BN_WALKS[walk]
    seed = 1000 + sorted(BN_WALKS).index(walk) * 8 + (C > 3) * 4 + relu * 2 + pool
    y, gamma, beta, pts = _bn_inputs(B, C, N, relu, pool, seed)
    g = _gen(seed + 1)
    rm, rv = torch.randn(C, generator=g).cuda(), (0.5 + torch.rand(C, generator=g)).cuda()
    dz = torch.randn((B, C) if pool else (B, C, N), generator=g).cuda()
    ref = _bn_ref(y, gamma, beta, rm, rv, relu, pool, dz, torch.float64)
    tt = _bn_torch(y, gamma, beta, rm, rv, relu, pool, dz, ref.get("idx"))
    hip = _bn_hip(y, gamma, beta, rm, rv, relu, pool, dz, offs)
    name = f"{walk} C={C} relu={relu} pool={pool}"
    bad = []
    low = (torch.arange(C) % 8 == 2).cuda()
    if pool:
        assert torch.equal(hip["idx"], ref["idx"]), f"{name}: pool_idx is not the first maximum"
        if N > 2:  # (under ReLU a cloud whose planted z is <= 0 pools the plateau of zeros: index 0)
            planted = (ref["idx"] == pts[0]) | (ref["out"] == 0 if relu else False)
            assert bool(planted[:, ~low].all()), "the planted ties are the maxima"
        if relu:
            assert bool((hip["out"][:, low] == 0).all()) and bool((hip["idx"][:, low] == 0).all())
            assert bool((hip["dy"][:, low] == 0).all()), "a channel with every z <= 0 gets no gradient"
        else:
            assert bool((hip["out"][:, low] < 0).all()), "all-negative channels pool a negative value"
        # the pooled gradient reaches the first maximum only: everywhere else dy = -scale (k1 + xhat k2),
        # which the float64 dy pins; a second copy of dz at another tie would be an O(|dz|) error there
    for k in ("out", "mean", "invstd", "rmean", "rvar", "dy", "dgamma", "dbeta"):
        _cmp("bn", f"{name} {k}", hip[k], ref[k], tt[k], bad)
    # the kernel's own terms, recomputed with one rounding per operation as bn_apply does
    m, i = hip["mean"][None, :, None], hip["invstd"][None, :, None]
    pre = ((y - m) * i) * gamma[None, :, None] + beta[None, :, None]
    if not pool:  # the mask is the sign of the forward's own output (test_bn_relu_mask_is_the_forward_sign)
        gk = torch.where(hip["out"] > 0, dz, torch.zeros_like(dz)) if relu else dz.clone()
    else:  # the pooled gradient at the forward's index, masked there (z at a planted maximum is far from 0)
        gk = torch.zeros_like(y).scatter_(2, hip["idx"][:, :, None], dz[:, :, None])
        if relu:
            gk = torch.where(pre > 0, gk, torch.zeros_like(gk))
    xh = ((y - m) * i).double()
    _sum_once(f"{name} dbeta", hip["dbeta"], gk.double().sum((0, 2)), gk.double().abs().sum((0, 2)), bad)
    gx = gk.double() * xh
    _sum_once(f"{name} dgamma", hip["dgamma"], gx.sum((0, 2)), gx.abs().sum((0, 2)), bad)
    _sum_once(f"{name} dbias", hip["dbias"], hip["dy"].double().sum((0, 2)), hip["dy"].double().abs().sum((0, 2)), bad)
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize("C", [3, 512])
@pytest.mark.parametrize("walk", ["vector_cached", "scalar_cached_N37", "uncached_N5463"])
def test_bn_relu_mask_is_the_forward_sign(walk, C):
    """The backward's ReLU mask recomputed from y equals the forward's output
    sign: with dz = 1 and relu = 1, dbeta[c] == (z_hip[c] > 0).sum() exactly,
    for the vector, the scalar cached and the uncached walk, both workgroup sizes."""
    B, N, offs, _ = BN_WALKS[walk]
    y, gamma, beta, _ = _bn_inputs(B, C, N, 0, 0, 77 + C)
    hip = _bn_hip(y, gamma, beta, torch.zeros(C).cuda(), torch.ones(C).cuda(), 1, 0, torch.ones(B, C, N).cuda(), offs)
    assert torch.equal(hip["dbeta"], (hip["out"] > 0).sum((0, 2)).float())


# ---------------------------------------------------------------- GEMM

def _operand(X, kmajor, pad, off):
    """X [nb][rows][k] stored k-major ([rows][k + pad]) or not ([k][rows + pad]), NaN in the pad columns."""
    S = X if kmajor else X.transpose(1, 2)
    nb, r, c = S.shape
    full = torch.full((nb, r, c + pad), float("nan"), device=X.device)
    full[:, :, :c] = S
    return Buf.of(full, off), c + pad, r * (c + pad)


def _gemm_run(Al, Bl, ak, bk, pad=0, off=0, ldc_pad=0, bias=None, sbias=0, cpp=1, nchunks=1, kchunk=None):
    """Al [batch or 1][M][K] (1: shared, sAz = 0), Bl [batch][K][N] -> the parts [parts][M][N]."""
    batch, K, N = Bl.shape
    M = Al.shape[1]
    a, lda, sAz = _operand(Al, ak, pad, off)
    b, ldb, sBz = _operand(Bl.transpose(1, 2), bk, pad, off)
    if Al.shape[0] == 1:
        sAz = 0
    parts, ldc = -(-batch // cpp) * nchunks, N + ldc_pad
    c = Buf(parts * M * ldc)
    bb = Buf.of(bias) if bias is not None else None
    rc = _lib().ndnet_tr_gemm(a.ptr, b.ptr, c.ptr, bb.ptr if bb else None, sbias, M, N, K, lda, ldb, ldc, sAz, sBz,
                              M * ldc, batch, cpp, int(ak), int(bk), nchunks, kchunk or K, _st())
    assert rc == 0, f"gemm returned {rc}"
    cw = c.words.view(parts, M, ldc)
    flags = torch.stack([(c.raw[:c.lo] == NAN_BITS).all(), (c.raw[c.lo + c.n:] == NAN_BITS).all(),
                         (cw[:, :, N:] == NAN_BITS).all(), ~(cw[:, :, :N] == NAN_BITS).any()])
    return c.t.view(parts, M, ldc)[:, :, :N], flags.all(), c


def _gemm_figures(got, ref, t32, An, Bn):
    """[e_hip, e_t, scale, max |err| / (|A_m| |B_n|)] as a device tensor."""
    err = (got.double() - ref).abs()
    return torch.stack([err.max(), (t32.double() - ref).abs().max(), ref.abs().max(), (err / (An * Bn + 1e-300)).max()])


def _gemm_verdict(fam, rows, oks):
    """rows: [(name, figures tensor)]; oks: sentinel flags.  One transfer, then print and assert."""
    fig = torch.stack([f for _, f in rows]).cpu()
    oks = torch.stack(oks).cpu()
    bad = []
    for (name, _), (e_hip, e_t, scale, rel), ok in zip(rows, fig.tolist(), oks.tolist()):
        print(f"RATIO {fam} {name}: e_hip {e_hip:.3e} e_t {e_t:.3e} scale {scale:.3e} "
              f"ratio {e_hip / e_t if e_t > 0 else (0.0 if e_hip == 0 else float('inf')):.2f} rel {rel:.2e}"
              f"{' (below 1e-6 scale)' if e_hip <= 1e-6 * scale else ''}")
        if not (e_hip <= FACTOR[fam] * e_t + 1e-6 * scale and rel <= 1e-5 and ok):
            bad.append((name, e_hip, e_t, scale, rel, "sentinels ok" if ok else "SENTINEL WRITTEN OR OUTPUT UNWRITTEN"))
    assert not bad, bad[:20]


def _ab(batch, M, N, K, seed, shared=False):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(1 if shared else batch, M, K, device="cuda", generator=g),
            torch.randn(batch, K, N, device="cuda", generator=g))


LAYOUTS = [(True, False), (False, False), (True, True), (False, True)]
LAYOUT_IDS = ["a_kmajor", "neither", "both_kmajor", "b_kmajor_only"]
# NDNET_TR_WIDE_MIN=1 (the child of test_child_wide_tiles): every M, N >= 128 runs the 128 x 128 tile kernel
WIDE = os.environ.get("NDNET_TR_WIDE_MIN") == "1"
GRID_MN = (128, 129, 191, 256) if WIDE else (1, 63, 64, 65)
GRID_K = (1, 3, 4, 15, 16, 17, 31, 32, 33, 65)


def _grid_options(M, N, K, batch):
    """(pad, base offset, shared weight, bias kind, ldc - N) of one grid point, each from its own
    bits of a hash of (M, N, K, batch), so no option is tied to K, to batch or to another option."""
    h = (M * 73856093) ^ (N * 19349663) ^ (K * 83492791) ^ (batch * 2654435761)
    h = (h * 0x9E3779B1 + 0x7F4A7C15) & 0xFFFFFFFF
    h ^= h >> 15
    return (0, 3, 5)[h % 3], (h >> 4) & 1, (h >> 7) % 4 == 0, (h >> 11) % 3, (0, 3, 4)[(h >> 17) % 3]


def test_gemm_grid_options_are_independent():
    """Every K and every batch of the tail grid meets every pad, both base alignments, a shared weight,
    every bias form and every ldc; batch = 3 meets a misaligned base with ldc > N."""
    for mn in ((1, 63, 64, 65), (128, 129, 191, 256)):
        seen = {}
        for M in mn:
            for N in mn:
                for K in GRID_K:
                    for batch in (1, 3):
                        o = _grid_options(M, N, K, batch)
                        for key in (("K", K), ("batch", batch)):
                            seen.setdefault(key, [set() for _ in o])
                            for sset, v in zip(seen[key], o):
                                sset.add(v)
                        if batch == 3 and o[1] == 1 and o[4] > 0:
                            seen["b3 off ldc"] = True
        for key, sets in seen.items():
            if key != "b3 off ldc":
                assert [len(x) for x in sets] == [3, 2, 2, 3, 3], (key, sets)
        assert seen.get("b3 off ldc")


@pytest.mark.gpu
@pytest.mark.parametrize("ak,bk", LAYOUTS, ids=LAYOUT_IDS)
def test_gemm_tile_and_k_tails(ak, bk):
    """The four layouts (a_kmajor, b_kmajor) -- `!a_kmajor, b_kmajor` included --
    over M, N in {1, 63, 64, 65} (128 x 128 tile tails with NDNET_TR_WIDE_MIN=1:
    {128, 129, 191, 256}), K in {1 .. 65} around the 16- and 32-deep steps,
    batch 1 and 3; per grid point, from independent bits of a hash: lda / ldb larger than the extent and not multiples
    of 4 with bases 4 bytes into a buffer (tile_load's / x6_load's element-wise
    fallback next to the 16-byte load), ldc > N, sAz = 0 (a shared weight), a
    shared and a per-cloud bias (sbias = M)."""
    rows, oks, i = [], [], 0
    for M in GRID_MN:
        for N in GRID_MN:
            for K in GRID_K:
                for batch in (1, 3):
                    i += 1
                    pad, off, shared, bias_kind, ldc_pad = _grid_options(M, N, K, batch)
                    Al, Bl = _ab(batch, M, N, K, i, shared)
                    bias = None if bias_kind == 0 else torch.randn(
                        batch if bias_kind == 2 else 1, M, device="cuda",
                        generator=torch.Generator(device="cuda").manual_seed(9000 + i))
                    got, ok, _ = _gemm_run(Al, Bl, ak, bk, pad, off, ldc_pad, bias, M if bias_kind == 2 else 0)
                    A64, B64 = Al.double().expand(batch, M, K), Bl.double()
                    ref, t32 = torch.bmm(A64, B64), torch.bmm(Al.expand(batch, M, K), Bl)
                    if bias is not None:
                        ref, t32 = ref + bias.double()[:, :, None], t32 + bias[:, :, None]
                    An, Bn = A64.norm(dim=2)[:, :, None], B64.norm(dim=1)[:, None, :]
                    if bias is not None:  # the bias is added in fp32: its rounding scales with |bias| too
                        An, Bn = An * Bn + bias.double().abs()[:, :, None], torch.ones_like(Bn)
                    rows.append((f"M{M} N{N} K{K} b{batch} pad{pad} off{off} ldc+{ldc_pad} bias{bias_kind} "
                                 f"shared{int(shared)}", _gemm_figures(got, ref, t32, An, Bn)))
                    oks.append(ok)
    _gemm_verdict("gemm", rows, oks)


def _sum_parts(c, count, nparts):
    out = Buf(count)
    rc = _lib().ndnet_tr_sum_parts(c.ptr, out.ptr, count, nparts, _st())
    assert rc == 0
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("ak,bk", LAYOUTS, ids=LAYOUT_IDS)
def test_gemm_split_k(ak, bk):
    """Split-K: a last chunk shorter than kchunk, kchunk not a multiple of 32,
    clouds_per_part not dividing batch; the parts summed by ndnet_tr_sum_parts
    against the whole product."""
    rows, oks = [], []
    for batch, M, N, K, nchunks, kchunk, cpp in [(3, 65, 63, 100, 3, 48, 1), (2, 64, 65, 100, 5, 20, 1),
                                                 (5, 63, 64, 33, 1, 33, 2), (5, 65, 65, 70, 2, 40, 3)] + (
                                                     [(5, 129, 191, 70, 2, 40, 3)] if WIDE else []):
        Al, Bl = _ab(batch, M, N, K, K + cpp)
        got, ok, c = _gemm_run(Al, Bl, ak, bk, pad=3, off=1, cpp=cpp, nchunks=nchunks, kchunk=kchunk)
        tot = _sum_parts(c, M * N, got.shape[0])
        torch.cuda.synchronize()
        assert tot.surround_ok() and tot.written()
        ref = torch.bmm(Al.double(), Bl.double()).sum(0)
        t32 = torch.bmm(Al, Bl).sum(0)
        scale = (Al.double().norm(dim=2)[:, :, None] * Bl.double().norm(dim=1)[:, None, :]).sum(0)
        rows.append((f"M{M} N{N} K{K} b{batch} chunks {nchunks}x{kchunk} cpp{cpp}",
                     _gemm_figures(tot.t.view(M, N), ref, t32, scale, torch.ones_like(scale))))
        oks.append(ok)
    _gemm_verdict("gemm", rows, oks)


@pytest.mark.gpu
@pytest.mark.parametrize("ak,bk", LAYOUTS, ids=LAYOUT_IDS)
def test_gemm_wide_tile_on_the_default_process(ak, bk):
    """128 x 128 tile tails: M = 129, N = 130, K = 7 and 40, batch = 128 gives
    2 * 2 * 128 = 512 workgroups, the default threshold of the 128 x 128 kernel
    (both operands k-major run split-bf16 unless NDNET_TR_X6=0); ldc > N, base
    offsets and a per-cloud bias."""
    rows, oks = [], []
    for K in (7, 40):
        Al, Bl = _ab(128, 129, 130, K, K)
        bias = torch.randn(128, 129, device="cuda", generator=torch.Generator(device="cuda").manual_seed(K + 1))
        got, ok, _ = _gemm_run(Al, Bl, ak, bk, pad=3, off=1, ldc_pad=3, bias=bias, sbias=129)
        ref = torch.bmm(Al.double(), Bl.double()) + bias.double()[:, :, None]
        t32 = torch.bmm(Al, Bl) + bias[:, :, None]
        An, Bn = Al.double().norm(dim=2)[:, :, None], Bl.double().norm(dim=1)[:, None, :]
        An, Bn = An * Bn + bias.double().abs()[:, :, None], torch.ones_like(Bn)
        rows.append((f"wide M129 N130 K{K} b128", _gemm_figures(got, ref, t32, An, Bn)))
        oks.append(ok)
    _gemm_verdict("gemm", rows, oks)


@pytest.mark.gpu
@pytest.mark.parametrize("nparts", [1, 2, 31, 32, 33, 65])
def test_sum_parts(nparts):
    """ndnet_tr_sum_parts / _2d on their own: 1 .. 65 parts (more than 32 parts:
    the second round of the part loop), a count that is not a multiple of 256,
    ldo > cols with the gap columns untouched; the sum in part order, so equal
    bit for bit to the same fp32 additions in sequence."""
    rows_, cols, ldo = 27, 37, 41
    count = rows_ * cols  # 999
    g = _gen(nparts)
    part = (torch.randn(nparts, count, generator=g) * 10.0 ** torch.randint(-3, 4, (nparts, 1), generator=g)).cuda()
    seq = part[0].clone()
    for p in range(1, nparts):
        seq = seq + part[p]
    pb = Buf.of(part)
    out = _sum_parts(pb, count, nparts)
    o2 = Buf(rows_ * ldo)
    assert _lib().ndnet_tr_sum_parts_2d(pb.ptr, o2.ptr, rows_, cols, ldo, nparts, _st()) == 0
    torch.cuda.synchronize()
    assert out.surround_ok() and out.written() and o2.surround_ok()
    w2 = o2.words.view(rows_, ldo)
    assert bool((w2[:, cols:] == NAN_BITS).all()), "gap columns of sum_parts_2d were written"
    assert torch.equal(out.t, seq), "not the parts in order"
    assert torch.equal(o2.t.view(rows_, ldo)[:, :cols].reshape(-1), seq)
    bad = []
    _cmp("sum_parts", f"nparts={nparts}", out.t, part.double().sum(0), part.sum(0), bad)
    assert not bad, bad


KT_CASES = [(True, False, 65, 63, 33, 3), (False, False, 64, 65, 65, 1), (False, True, 63, 64, 31, 3),
            (True, False, 129, 130, 40, 128), (False, False, 129, 130, 7, 128)]


@pytest.mark.gpu
def test_gemm_dump_for_kt_comparison(tmp_path):
    """A few fp32-kernel products (64 x 64 and 128 x 128 tiles) saved to
    NDNET_TR_TEST_DUMP for test_child_kt16_is_bit_identical.  That variable belongs
    to this test alone (the library does not read it): it carries the path to the
    child, named so because a child gets no variable outside NDNET_TR_*."""
    outs = []
    for ak, bk, M, N, K, batch in KT_CASES:
        Al, Bl = _ab(batch, M, N, K, M + K)
        got, ok, _ = _gemm_run(Al, Bl, ak, bk)
        assert bool(ok)
        outs.append(got.cpu().clone())
    torch.save(outs, os.environ.get("NDNET_TR_TEST_DUMP") or str(tmp_path / "dump.pt"))


# ---------------------------------------------------------------- FC heads

def _fc_ref(x, W, b, gamma, beta, relu, eye, dz, dtype, rm=None, rv=None):
    """Linear (+ identity) [+ BatchNorm1d over the rows + ReLU], forward and backward, written out in `dtype`."""
    B, N = x.shape[0], W.shape[0]
    x, W, b = (t.to(dtype).requires_grad_() for t in (x, W, b))
    y = x @ W.t() + b
    if eye:
        d = torch.zeros(N, dtype=dtype, device=x.device)
        d[[n for n in range(min(N, eye * eye)) if n % (eye + 1) == 0]] = 1.0
        y = y + d
    y.retain_grad()
    r = {}
    if gamma is not None:
        gamma, beta = gamma.to(dtype).requires_grad_(), beta.to(dtype).requires_grad_()
        mu = y.mean(0)
        var = ((y - mu) ** 2).mean(0)
        inv = 1.0 / torch.sqrt(var + EPS)
        z = (y - mu) * inv * gamma + beta
        if relu:
            z = torch.relu(z)
        unb = var * B / (B - 1) if B > 1 else var
        r.update(mean=mu.detach(), invstd=inv.detach(), rmean=(1 - MOM) * rm.to(dtype) + MOM * mu.detach(),
                 rvar=(1 - MOM) * rv.to(dtype) + MOM * unb.detach())
    else:
        z = y
    z.backward(dz.to(dtype))
    r.update(y=y.detach(), z=z.detach(), dpre=y.grad, dW=W.grad, db=b.grad, dx=x.grad)
    if gamma is not None:
        r.update(dgamma=gamma.grad, dbeta=beta.grad)
    return r


def _fc_torch(x, W, b, gamma, beta, relu, eye, dz, rm=None, rv=None):
    """torch's fp32 ops: F.linear, F.batch_norm(training=True), autograd."""
    N = W.shape[0]
    x, W, b = (t.clone().requires_grad_() for t in (x, W, b))
    y = F.linear(x, W, b)
    if eye:
        d = torch.zeros(N, device=x.device)
        d[[n for n in range(min(N, eye * eye)) if n % (eye + 1) == 0]] = 1.0
        y = y + d
    y.retain_grad()
    r = {}
    if gamma is not None:
        gamma, beta = gamma.clone().requires_grad_(), beta.clone().requires_grad_()
        rm, rv = rm.clone(), rv.clone()
        z = F.batch_norm(y, rm, rv, gamma, beta, True, MOM, EPS)
        if relu:
            z = torch.relu(z)
        var, mean = torch.var_mean(y.detach(), 0, unbiased=False)
        r.update(mean=mean, invstd=torch.rsqrt(var + EPS), rmean=rm, rvar=rv)
    else:
        z = y
    z.backward(dz)
    r.update(y=y.detach(), z=z.detach(), dpre=y.grad, dW=W.grad, db=b.grad, dx=x.grad)
    if gamma is not None:
        r.update(dgamma=gamma.grad, dbeta=beta.grad)
    return r


def _fc_inputs(B, K, N, bn, relu, seed):
    g = _gen(seed)
    x = torch.randn(B, K, generator=g).cuda()
    W = (torch.randn(N, K, generator=g) / math.sqrt(K)).cuda()
    b = (0.3 * torch.randn(N, generator=g)).cuda()
    dz = torch.randn(B, N, generator=g).cuda()
    if not bn:
        return x, W, b, None, None, dz, None, None
    gamma = ((0.5 + torch.rand(N, generator=g)) * torch.where(torch.arange(N) % 2 == 1, -1.0, 1.0)).cuda()
    beta = (0.5 * torch.randn(N, generator=g)).cuda()
    rm, rv = torch.randn(N, generator=g).cuda(), (0.5 + torch.rand(N, generator=g)).cuda()
    if relu:  # no float64 z within 1e-4 max |z| of zero: shift beta of the channels that have one
        for it in range(20):
            y = x.double() @ W.double().t() + b.double()
            mu = y.mean(0)
            z = (y - mu) / torch.sqrt(((y - mu) ** 2).mean(0) + EPS) * gamma.double() + beta.double()
            near = (z.abs() < 1e-4 * z.abs().max()).any(0)
            if not bool(near.any()):
                break
            beta = torch.where(near, beta + 0.013 * (it + 1), beta)
        else:
            raise AssertionError("inputs: a float64 z at rounding level of zero")
    return x, W, b, gamma, beta, dz, rm, rv


def _fc_hip(x, W, b, gamma, beta, relu, eye, dz, rm, rv, ldw_mode, nulls=()):
    """fc_fwd then fc_bwd_w then fc_bwd_x (one split).  ldw_mode: 0: ldw = 0 (= K); 4: ldw = K + 4;
    64: W and dW are the column slice [:, 64:] of an [N][K + 64] matrix."""
    lib = _lib()
    B, K = x.shape
    N = W.shape[0]
    bn = gamma is not None
    ldw = 0 if ldw_mode == 0 else K + ldw_mode
    col0 = 64 if ldw_mode == 64 else 0
    wide = K + ldw_mode
    Wf = torch.full((N, wide), float("nan"), device="cuda")
    Wf[:, col0:col0 + K] = W
    bufs = dict(x=Buf.of(x), W=Buf.of(Wf), b=Buf.of(b), y=Buf(B * N) if bn else None, z=Buf(B * N),
                mean=Buf(N) if bn else None, invstd=Buf(N) if bn else None, rmean=Buf.of(rm) if bn else None,
                rvar=Buf.of(rv) if bn else None, gamma=Buf.of(gamma) if bn else None, beta=Buf.of(beta) if bn else None,
                nbt=Buf.of(torch.tensor([7], dtype=torch.int64, device="cuda")) if bn else None, dz=Buf.of(dz),
                dpre=Buf(B * N), dW=Buf(N * wide), db=Buf(N), dgamma=Buf(N) if bn else None,
                dbeta=Buf(N) if bn else None, dx=Buf(B * K))
    p = lambda k: None if (bufs[k] is None or k in nulls) else bufs[k].ptr  # noqa: E731
    wp, dwp = bufs["W"].ptr + 4 * col0, (None if "dW" in nulls else bufs["dW"].ptr + 4 * col0)
    rc = lib.ndnet_tr_fc_fwd(p("x"), wp, p("b"), p("y"), p("z"), p("mean"), p("invstd"), p("rmean"), p("rvar"),
                             p("gamma"), p("beta"), B, K, N, ldw, EPS, MOM, relu, eye, p("nbt"), _st())
    assert rc == 0, f"fc_fwd returned {rc}"
    rc = lib.ndnet_tr_fc_bwd_w(p("dz"), p("x"), p("y"), p("mean"), p("invstd"), p("gamma"), p("beta"), p("dpre"), dwp,
                               p("db"), p("dgamma"), p("dbeta"), B, K, N, ldw, relu, _st())
    assert rc == 0, f"fc_bwd_w returned {rc}"
    if "dpre" not in nulls and N <= 256:
        rc = lib.ndnet_tr_fc_bwd_x(p("dpre"), wp, p("dx"), None, B, K, N, ldw, 1, _st())
        assert rc == 0, f"fc_bwd_x returned {rc}"
    torch.cuda.synchronize()
    _guards(bufs, "fc")
    dWw = bufs["dW"].words.view(N, wide)
    if "dW" not in nulls:
        assert not bool((dWw[:, col0:col0 + K] == NAN_BITS).any()), "dW not fully written"
    assert bool((dWw[:, :col0] == NAN_BITS).all()) and bool((dWw[:, col0 + K:] == NAN_BITS).all()), \
        "columns of dW outside the slice were written"
    for k in nulls:
        assert bool((bufs[k].words == NAN_BITS).all())
    if bn:
        assert int(bufs["nbt"].t[0]) == 8
    r = {k: bufs[k].t.clone() for k in ("mean", "invstd", "rmean", "rvar", "db", "dgamma", "dbeta")
         if bufs[k] is not None}
    for k in ("y", "z", "dpre"):
        if bufs[k] is not None:
            r[k] = bufs[k].t.view(B, N).clone()
    r["dW"] = bufs["dW"].t.view(N, wide)[:, col0:col0 + K].clone()
    r["dx"] = bufs["dx"].t.view(B, K).clone()
    return r


def _fc_check(name, B, K, N, bn, relu, eye, ldw_mode, seed, bad):
    x, W, b, gamma, beta, dz, rm, rv = _fc_inputs(B, K, N, bn, relu, seed)
    ref = _fc_ref(x, W, b, gamma, beta, relu, eye, dz, torch.float64, rm, rv)
    tt = _fc_torch(x, W, b, gamma, beta, relu, eye, dz, rm, rv)
    hip = _fc_hip(x, W, b, gamma, beta, relu, eye, dz, rm, rv, ldw_mode)
    # under BatchNorm db's float64 value is 0 and both sides are rounding noise: only the sum-once bound below
    keys = ["z", "dpre", "dW"] + (["y", "mean", "invstd", "rmean", "rvar", "dgamma", "dbeta"] if bn else ["db"])
    if N <= 256:
        keys.append("dx")
    for k in keys:
        fam = "fc"
        if bn and B == 2:
            fam = "fc_b2_bwd" if k in ("dpre", "dW", "dx") else "fc_b2_dgamma" if k == "dgamma" else "fc"
        _cmp(fam, f"{name} {k}", hip[k], ref[k], tt[k], bad)
    _sum_once(f"{name} db", hip["db"], hip["dpre"].double().sum(0), hip["dpre"].double().abs().sum(0), bad)


FC_B = (1, 2, 3, 15, 16)
FC_K = (4, 8, 252, 260, 1024, 2048)
FC_N = (1, 7, 8, 9, 65)


@pytest.mark.gpu
@pytest.mark.parametrize("bn", [False, True], ids=["linear", "bn_relu"])
def test_fc_heads_shapes(bn):
    """fc_fwd, fc_bwd_w, fc_bwd_x with and without gamma: B in {1 (no gamma), 2,
    3, 15, 16}, K in {4, 8, 252, 260 (not multiples of 256), 1024, 2048 with
    B = 8: K > 1024 FC, the second round of the f0 loop}, N in {1, 7, 8, 9, 65}
    (N < 8, N not a multiple of the 8 waves) and N = 2057 > 2048 (the channel
    loop strides the grid); ldw = 0, `ldw > K` as K + 4 and as the column slice
    [:, 64:] of an [N][K + 64] matrix (the columns outside the slice keep the
    sentinel in dW); eye in {0, 3, 64}: exactly the diagonal entries get + 1."""
    bad, i = [], 0
    for K in FC_K:
        for B in FC_B:
            if bn and B == 1:
                continue
            Bk = min(B, 8) if K == 2048 else B
            for N in FC_N + ((2057,) if (K == 8 and B in (3, 16)) else ()):
                i += 1
                relu = int(bn and i % 3 != 0)
                eye = 0 if bn else (0, 3, 64)[i % 3]
                ldw_mode = (0, 4, 64)[(i + i // 3) % 3]
                _fc_check(f"B{Bk} K{K} N{N} relu{relu} eye{eye} ldw+{ldw_mode}", Bk, K, N, bn, relu, eye, ldw_mode,
                          3000 + i, bad)
    assert not bad, bad[:20]


@pytest.mark.gpu
@pytest.mark.parametrize("eye", [3, 64])
def test_fc_eye_adds_one_on_the_diagonal_only(eye):
    """eye x eye transform: with zero x, y = bias + 1 exactly at n % (eye + 1) == 0, n < eye^2, bias elsewhere."""
    N = eye * eye + 5
    b = torch.randn(N, generator=_gen(eye)).cuda()
    x, W = torch.zeros(2, 8).cuda(), torch.randn(N, 8, generator=_gen(1)).cuda()
    hip = _fc_hip(x, W, b, None, None, 0, eye, torch.zeros(2, N).cuda(), None, None, 4)
    diag = torch.tensor([float(n < eye * eye and n % (eye + 1) == 0) for n in range(N)]).cuda()
    assert torch.equal(hip["z"], (b + diag)[None, :].expand(2, N))
    assert int(diag.sum()) == eye


@pytest.mark.gpu
@pytest.mark.parametrize("N,nsplit", [(257, 2), (257, 3), (512, 2), (512, 3), (7, 1), (7, 2), (7, 3)])
def test_fc_bwd_x_splits(N, nsplit):
    """nsplit in {1, 2, 3} with N = 257, 512, 7 (uneven nsplit: the boundaries
    are floor(N s / nsplit)); every partial against the float64 product over its
    channel range, dx equal bit for bit to the partials added in split order;
    ldw > K."""
    B, K, ldw = 5, 260, 264
    g = _gen(N * 4 + nsplit)
    dpre, W = torch.randn(B, N, generator=g).cuda(), torch.full((N, ldw), float("nan")).cuda()
    W[:, :K] = torch.randn(N, K, generator=g).cuda() / math.sqrt(N)
    d, w, dx, part = Buf.of(dpre), Buf.of(W), Buf(B * K), Buf(nsplit * B * K)
    rc = _lib().ndnet_tr_fc_bwd_x(d.ptr, w.ptr, dx.ptr, part.ptr if nsplit > 1 else None, B, K, N, ldw, nsplit, _st())
    assert rc == 0
    torch.cuda.synchronize()
    assert dx.surround_ok() and dx.written() and part.surround_ok()
    bad = []
    Wk = W[:, :K]
    _cmp("fc", f"bwd_x N{N} nsplit{nsplit} dx", dx.t.view(B, K), dpre.double() @ Wk.double(), dpre @ Wk, bad)
    if nsplit > 1:
        assert part.written()
        pv = part.t.view(nsplit, B, K)
        seq = pv[0].clone()
        for s in range(nsplit):
            n0, n1 = N * s // nsplit, N * (s + 1) // nsplit
            _cmp("fc", f"bwd_x N{N} nsplit{nsplit} part{s}", pv[s], dpre[:, n0:n1].double() @ Wk[n0:n1].double(),
                 dpre[:, n0:n1] @ Wk[n0:n1], bad)
            if s:
                seq = seq + pv[s]
        assert torch.equal(seq.reshape(-1), dx.t), "dx is not the partials in split order"
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize("null", ["dpre", "dW", "db", "dgamma", "dbeta"])
def test_fc_bwd_w_null_outputs(null):
    """Each output of fc_bwd_w passed as NULL in turn: accepted, the others unchanged bit for bit."""
    args = _fc_inputs(3, 260, 9, True, 1, 42)
    x, W, b, gamma, beta, dz, rm, rv = args
    full = _fc_hip(x, W, b, gamma, beta, 1, 0, dz, rm, rv, 4)
    part = _fc_hip(x, W, b, gamma, beta, 1, 0, dz, rm, rv, 4, nulls=(null,))
    for k in ("dpre", "dW", "db", "dgamma", "dbeta"):
        if k != null:
            assert torch.equal(full[k], part[k]), k


@pytest.mark.gpu
def test_fc_relu_mask_is_the_forward_sign():
    """dz = 1, relu = 1: dbeta[n] == (z_hip[:, n] > 0).sum() exactly."""
    for B, K, N in ((2, 8, 65), (15, 260, 9), (16, 1024, 65)):
        x, W, b, gamma, beta, _, rm, rv = _fc_inputs(B, K, N, True, 0, B + K)
        hip = _fc_hip(x, W, b, gamma, beta, 1, 0, torch.ones(B, N).cuda(), rm, rv, 0)
        assert torch.equal(hip["dbeta"], (hip["z"] > 0).sum(0).float())


# ---------------------------------------------------------------- log_softmax, loss, accuracy

LSM_C = (1, 2, 29, 31, 32)
LSM_BN = ((1, 1), (1, 63), (2, 33), (3, 1000))


def _logits(B, C, N, variant, seed):
    g = _gen(seed)
    x = torch.randn(B, C, N, generator=g)
    if variant == "range90":
        x = x * (90.0 / x.abs().max())
    if variant == "ahead104":  # one class ahead by more than 104: the others' exp underflows
        lead = torch.randint(0, C, (B, 1, N), generator=g)
        x = x.scatter_add(1, lead, torch.full((B, 1, N), 120.0))
    return x.cuda()


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["plain", "range90", "ahead104"])
@pytest.mark.parametrize("C", LSM_C)
def test_log_softmax_c_fwd_bwd(C, variant):
    """log_softmax over C = 1 and C = 32 classes (and 2, 29, 31) at (B, N) =
    (1, 1), (1, 63), (2, 33), (3, 1000) -- the tail workgroup, a cloud boundary
    inside a workgroup --, logits to +-90 and one class ahead by more than 104;
    the backward against float64 autograd."""
    bad = []
    for B, N in LSM_BN:
        x = _logits(B, C, N, variant, C * 7 + N)
        dy = torch.randn(B, C, N, generator=_gen(N)).cuda()
        xb, ob, dyb, dxb = Buf.of(x), Buf(B * C * N), Buf.of(dy), Buf(B * C * N)
        assert _lib().ndnet_tr_log_softmax_c(xb.ptr, ob.ptr, B, C, N, _st()) == 0
        assert _lib().ndnet_tr_log_softmax_c_bwd(ob.ptr, dyb.ptr, dxb.ptr, B, C, N, _st()) == 0
        torch.cuda.synchronize()
        assert ob.surround_ok() and ob.written() and dxb.surround_ok() and dxb.written()
        x64 = x.double().requires_grad_()
        ref = torch.log_softmax(x64, 1)
        ref.backward(dy.double())
        x32 = x.clone().requires_grad_()
        t32 = torch.log_softmax(x32, 1)
        t32.backward(dy)
        if variant == "range90" and C > 1:
            assert ref.abs().max().item() > 80
        _cmp("softmax", f"C{C} B{B} N{N} {variant} fwd", ob.t.view(B, C, N), ref.detach(), t32.detach(), bad)
        _cmp("softmax", f"C{C} B{B} N{N} {variant} bwd", dxb.t.view(B, C, N), x64.grad, x32.grad, bad)
    assert not bad, bad


def _onehot(B, N, C, seed, empty=True):
    g = _gen(seed)
    gt = F.one_hot(torch.randint(0, C, (B, N), generator=g), C).float()
    if empty and N > 4:
        gt[0, 1:N:7] = 0.0  # rows without a class
    return gt.cuda()


@pytest.mark.gpu
@pytest.mark.parametrize("C", LSM_C)
def test_nll_onehot_fwd_bwd(C):
    """nll_onehot and its gradient at the log_softmax shapes: rows without a
    class, `part` sized exactly ceil(B N / 64) doubles with the sentinel after
    it, dloss != 1."""
    bad = []
    for B, N in LSM_BN:
        logp = torch.log_softmax(_logits(B, C, N, "plain", C + N), 1)
        gt = _onehot(B, N, C, C * N)
        nparts = (B * N + 63) // 64
        dloss = torch.tensor([3.0], device="cuda")
        lb, gb, part, loss, dl, dlogp = Buf.of(logp), Buf.of(gt), Buf(2 * nparts, torch.float64), Buf(1), \
            Buf.of(dloss), Buf(B * C * N)
        assert _lib().ndnet_tr_nll_onehot(lb.ptr, gb.ptr, part.ptr, loss.ptr, B, C, N, _st()) == 0
        assert _lib().ndnet_tr_nll_onehot_bwd(gb.ptr, dl.ptr, dlogp.ptr, B, C, N, _st()) == 0
        torch.cuda.synchronize()
        assert part.surround_ok() and part.written() and loss.surround_ok() and dlogp.surround_ok() and dlogp.written()
        l64 = logp.double().requires_grad_()
        ref = -(gt.double() * l64.transpose(1, 2)).sum(-1).mean()
        (ref * 3.0).backward()
        l32 = logp.clone().requires_grad_()
        t32 = -(gt * l32.transpose(1, 2)).sum(-1).mean()
        (t32 * 3.0).backward()
        _cmp("nll", f"C{C} B{B} N{N} loss", loss.t, ref.detach().reshape(1), t32.detach().reshape(1), bad)
        _cmp("nll", f"C{C} B{B} N{N} grad", dlogp.t.view(B, C, N), l64.grad, l32.grad, bad)
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize("C", LSM_C)
def test_argmax_match_both_layouts(C):
    """argmax_match_cm (pred [B][C][N]) and argmax_match (pred [rows][cols])
    against torch.argmax with a planted NaN, an exact tie and an all-equal row:
    ctr[0] the matches, ctr[1] == the grid size, acc == ctr[0] / (B N) exactly,
    acc = NULL accepted."""
    for B, N in LSM_BN:
        g = _gen(C * 31 + N)
        pred = torch.randn(B, N, C, generator=g)  # [B][N][C]
        pts = B * N
        if pts >= 3 and C > 1:
            pred[0, 0, C // 2] = float("nan")
            pred[0, 1, C - 1] = pred[0, 1].max()  # an exact tie: the first index wins
            pred[-1, N - 1, :] = 0.25             # an all-equal row: class 0
        want = pred.argmax(-1)
        gt = F.one_hot(torch.where(torch.rand(B, N, generator=g) < 0.5, want, torch.randint(0, C, (B, N), generator=g)),
                       C).float()
        if pts >= 3 and C > 1:
            for b_, n_ in ((0, 0), (0, 1), (-1, N - 1)):  # the planted rows count as matches
                gt[b_, n_] = F.one_hot(want[b_, n_], C)
        count = int((pred.argmax(-1) == gt.argmax(-1)).sum())
        cm = Buf.of(pred.transpose(1, 2).contiguous().cuda())
        rm_, gb = Buf.of(pred.cuda()), Buf.of(gt.cuda())
        for with_acc in (True, False):
            ctr, acc = Buf.of(torch.zeros(2, dtype=torch.int32, device="cuda")), Buf(1)
            rc = _lib().ndnet_tr_argmax_match_cm(cm.ptr, gb.ptr, B, C, N, ctr.ptr, acc.ptr if with_acc else None, _st())
            assert rc == 0
            torch.cuda.synchronize()
            assert ctr.surround_ok() and acc.surround_ok()
            assert ctr.t.tolist() == [count, (pts + 63) // 64], (C, B, N, ctr.t.tolist(), count)
            if with_acc:
                want_acc = (torch.tensor(float(count)) / torch.tensor(float(pts))).item()
                assert acc.t.item() == want_acc
            else:
                assert not acc.written()
        cnt = Buf.of(torch.zeros(1, dtype=torch.int32, device="cuda"))
        assert _lib().ndnet_tr_argmax_match(rm_.ptr, gb.ptr, pts, C, cnt.ptr, _st()) == 0
        torch.cuda.synchronize()
        assert cnt.surround_ok() and cnt.t.item() == count


# ---------------------------------------------------------------- the small kernels

def _mixed(shape, seed):
    """Values of mixed sign and scale, 10^-6 .. 10^6."""
    g = _gen(seed)
    return (torch.randn(shape, generator=g) * 10.0 ** (torch.rand(shape, generator=g) * 12 - 6)).cuda()


@pytest.mark.gpu
@pytest.mark.parametrize("B,N", [(1, 1), (27, 19), (20, 1000), (3, 63), (3, 64), (3, 65)])
def test_chan_sum(B, N):
    """chan_sum at B N in {1, 513, 20000} and N in {1, 63, 64, 65, 1000}: the float64 sum rounded once."""
    C = 5
    x = _mixed((B, C, N), B + N)
    xb, out = Buf.of(x), Buf(C)
    assert _lib().ndnet_tr_chan_sum(xb.ptr, out.ptr, B, C, N, _st()) == 0
    torch.cuda.synchronize()
    assert out.surround_ok() and out.written()
    bad = []
    _sum_once(f"chan_sum B{B} N{N}", out.t, x.double().sum((0, 2)), x.double().abs().sum((0, 2)), bad)
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize("rows", [1, 6, 7])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 1000])
def test_row_sum(rows, N):
    """row_sum with rows % 4 != 0 (a workgroup holds four rows) and N around the wave: the float64 sum rounded once."""
    x = _mixed((rows, N), rows * 1000 + N)
    xb, out = Buf.of(x), Buf(rows)
    assert _lib().ndnet_tr_row_sum(xb.ptr, out.ptr, rows, N, _st()) == 0
    torch.cuda.synchronize()
    assert out.surround_ok() and out.written()
    bad = []
    _sum_once(f"row_sum rows{rows} N{N}", out.t, x.double().sum(1), x.double().abs().sum(1), bad)
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize("pld,eld", [(3, 9), (12, 12), (5, 11)])
def test_point_transform_fwd_bwd(pld, eld):
    """point_transform and its backward at N in {1, 255, 256, 257, 1025, 2049}
    (N > 1024 transform backward: the second round of the point loop), B = 3,
    separate arrays with padded rows and both views of one [B][N][12] array."""
    B, bad = 3, []
    for N in (1, 255, 256, 257, 1025, 2049):
        g = _gen(N + pld)
        t = torch.randn(B, 3, 3, generator=g).cuda()
        p = (torch.rand(B, N, 3, generator=g) * 20 - 10).cuda()
        cv = torch.randn(B, N, 9, generator=g).cuda()
        dx = torch.randn(B, 12, N, generator=g).cuda()
        if pld == 12:  # one [B][N][12] array: points in columns 0-2, the covariance in 3-11
            rows = Buf.of(torch.cat([p, cv], 2))
            pp, ep, keep = rows.ptr, rows.ptr + 12, rows
        else:
            pf, ef = torch.full((B, N, pld), float("nan")).cuda(), torch.full((B, N, eld), float("nan")).cuda()
            pf[..., :3], ef[..., :9] = p, cv
            keep = (Buf.of(pf), Buf.of(ef))
            pp, ep = keep[0].ptr, keep[1].ptr
        tb, xb, dxb, dtb = Buf.of(t), Buf(B * 12 * N), Buf.of(dx), Buf(B * 9)
        assert _lib().ndnet_tr_point_transform(tb.ptr, pp, pld, ep, eld, xb.ptr, B, N, _st()) == 0
        assert _lib().ndnet_tr_point_transform_bwd(dxb.ptr, pp, pld, ep, eld, dtb.ptr, B, N, _st()) == 0
        torch.cuda.synchronize()
        assert xb.surround_ok() and xb.written() and dtb.surround_ok() and dtb.written()

        def run(dtype):
            tt = t.to(dtype).requires_grad_()
            xp = torch.bmm(tt, p.to(dtype).transpose(1, 2))                                    # [B][3][N]
            xc = torch.bmm(tt, cv.to(dtype).view(B, N, 3, 3).permute(0, 2, 1, 3).reshape(B, 3, N * 3))  # [B][3][(n, k)]
            xc = xc.view(B, 3, N, 3).permute(0, 1, 3, 2).reshape(B, 9, N)                       # row 3 i + k
            x = torch.cat([xp, xc], 1)
            x.backward(dx.to(dtype))
            return x.detach(), tt.grad

        (x64, dt64), (x32, dt32) = run(torch.float64), run(torch.float32)
        _cmp("transform", f"pld{pld} eld{eld} N{N} x", xb.t.view(B, 12, N), x64, x32, bad)
        _cmp("transform", f"pld{pld} eld{eld} N{N} dt", dtb.t.view(B, 3, 3), dt64, dt32, bad)
        del keep
    assert not bad, bad


ADAM_NUMEL = (1, 255, 4095, 4096, 4097, 8193)


def _adam_call(n, ps, gs, ms, vs, ss, numel, lr, wd):
    arr = lambda xs: (ctypes.c_void_p * len(xs))(*xs)  # noqa: E731
    return _lib().ndnet_tr_adam(n, arr(ps), arr(gs), arr(ms), arr(vs), arr(ss), (ctypes.c_int64 * len(numel))(*numel),
                                lr, 0.9, 0.999, 1e-8, wd, _st())


@pytest.mark.gpu
@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("n", [1, 32, 33, 129])
def test_adam(n, wd):
    """ndnet_tr_adam with n in {1, 32, 33, 129} tensors (n > 128 Adam: the second
    steps launch; n > 32: the second update launch) of 1 .. 8193 elements (a
    tensor that crosses a 4096-element chunk by one), three steps, weight decay
    on and off: against torch's fused capturable Adam with the existing test's
    tolerances, and against a float64 transcription of the header's update
    under the e_t bound; nothing past numel is written.  (The kernel follows
    torch's double-precision roundings: on an MI355X every parameter and moment
    came out equal to torch's bit for bit; a tensor that differs is printed.)"""
    numel = [ADAM_NUMEL[i % len(ADAM_NUMEL)] for i in range(n)]
    g = _gen(n)
    p0 = [torch.randn(k, generator=g).cuda() for k in numel]
    P, Mo, V, S = [Buf.of(p) for p in p0], [Buf.of(torch.zeros_like(p)) for p in p0], \
        [Buf.of(torch.zeros_like(p)) for p in p0], [Buf.of(torch.zeros(1).cuda()) for _ in p0]
    lr = torch.tensor(1e-3, device="cuda")
    qs = [p.clone().requires_grad_() for p in p0]
    opt = torch.optim.Adam(qs, lr=lr.clone(), weight_decay=wd, capturable=True, fused=True)
    p64, m64, v64 = [p.double() for p in p0], [torch.zeros_like(p).double() for p in p0], \
        [torch.zeros_like(p).double() for p in p0]
    lr64 = lr.double()
    for step in range(1, 4):
        grads = [(torch.randn(k, generator=g) * 10.0 ** (i % 5 - 2)).cuda() for i, k in enumerate(numel)]
        G = [Buf.of(x) for x in grads]
        rc = _adam_call(n, [b.ptr for b in P], [b.ptr for b in G], [b.ptr for b in Mo], [b.ptr for b in V],
                        [b.ptr for b in S], numel, lr.data_ptr(), wd)
        assert rc == 0
        torch.cuda.synchronize()
        for q, x in zip(qs, grads):
            q.grad = x.clone()
        opt.step()
        for i, x in enumerate(grads):
            gi = x.double() + wd * p64[i] if wd else x.double()
            m64[i] = 0.9 * m64[i] + (1 - 0.9) * gi
            v64[i] = 0.999 * v64[i] + (1 - 0.999) * gi * gi
            denom = v64[i].sqrt() / math.sqrt(1 - 0.999 ** step) + 1e-8
            p64[i] = p64[i] - (lr64 / (1 - 0.9 ** step)) * m64[i] / denom
    torch.cuda.synchronize()
    bad = []
    for i, q in enumerate(qs):
        for b in (P[i], Mo[i], V[i], S[i]):
            assert b.surround_ok(), f"tensor {i}: written past numel"
        assert S[i].t.item() == 3.0
        dv = (V[i].t != opt.state[q]["exp_avg_sq"]).sum().item()
        if dv or (P[i].t != q.detach()).any():
            print(f"ADAM bits n{n} wd{wd} tensor {i} numel {numel[i]}: v differs in {dv}, p in "
                  f"{(P[i].t != q.detach()).sum().item()}, m in {(Mo[i].t != opt.state[q]['exp_avg']).sum().item()}")
        torch.testing.assert_close(P[i].t, q.detach(), rtol=1e-6, atol=1e-7, msg=f"tensor {i} wd {wd}")
        torch.testing.assert_close(V[i].t, opt.state[q]["exp_avg_sq"], rtol=1e-6, atol=0)
    # one comparison over all tensors of a size class (the bound is per output tensor; figures per size)
    for k in sorted(set(numel)):
        ix = [i for i, kk in enumerate(numel) if kk == k]
        cat = lambda xs: torch.cat([xs[i].reshape(-1) for i in ix])  # noqa: E731
        _cmp("adam", f"n{n} wd{wd} numel{k} p", cat([b.t for b in P]), cat(p64), cat([q.detach() for q in qs]), bad)
        _cmp("adam", f"n{n} wd{wd} numel{k} m", cat([b.t for b in Mo]), cat(m64),
             cat([opt.state[q]["exp_avg"] for q in qs]), bad)
        _cmp("adam", f"n{n} wd{wd} numel{k} v", cat([b.t for b in V]), cat(v64),
             cat([opt.state[q]["exp_avg_sq"] for q in qs]), bad)
    assert not bad, bad


@pytest.mark.gpu
def test_adam_rejected_call_changes_nothing():
    """One bad numel among 40 valid tensors: -20, and every step counter,
    parameter and moment keeps its bits (every tensor is validated before the
    first launch)."""
    n = 40
    g = _gen(40)
    mk = lambda: [Buf.of(torch.randn(100, generator=g).cuda()) for _ in range(n)]  # noqa: E731
    P, G, Mo, V = mk(), mk(), mk(), mk()
    S = [Buf.of(torch.full((1,), 2.0).cuda()) for _ in range(n)]
    before = [[b.raw.clone() for b in grp] for grp in (P, Mo, V, S)]
    numel = [100] * n
    numel[37] = 0
    lr = torch.tensor(1e-3, device="cuda")
    args = ([b.ptr for b in P], [b.ptr for b in G], [b.ptr for b in Mo], [b.ptr for b in V], [b.ptr for b in S])
    assert _adam_call(n, *args, numel, lr.data_ptr(), 0.0) == -20
    torch.cuda.synchronize()
    for grp, old in zip((P, Mo, V, S), before):
        for b, o in zip(grp, old):
            assert torch.equal(b.raw, o)
    numel[37] = 100
    assert _adam_call(n, *args, numel, lr.data_ptr(), 0.0) == 0
    torch.cuda.synchronize()
    assert all(s.t.item() == 3.0 for s in S)


# ---------------------------------------------------------------- argument checks
# A rejected call launches nothing, so the rejections run over host memory without a GPU.

ARG_ORDER = {
    "ndnet_tr_gemm": "A B C bias sbias M N K lda ldb ldc sAz sBz sCz batch cpp ak bk nchunks kchunk",
    "ndnet_tr_sum_parts_2d": "part out rows cols ldo nparts",
    "ndnet_tr_bn_fwd": "y z mean invstd rmean rvar gamma beta B C N eps mom relu pool pool_idx nbt",
    "ndnet_tr_bn_bwd": "dz y mean invstd gamma beta dy dgamma dbeta dbias B C N relu pool_idx",
    "ndnet_tr_fc_fwd": "x W bias y z mean invstd rmean rvar gamma beta B K N ldw eps mom relu eye nbt",
    "ndnet_tr_fc_bwd_w": "dz x y mean invstd gamma beta dpre dW db dgamma dbeta B K N ldw relu",
    "ndnet_tr_fc_bwd_x": "dpre W dx part B K N ldw nsplit",
    "ndnet_tr_log_softmax_c": "x out B C N",
    "ndnet_tr_log_softmax_c_bwd": "y dy dx B C N",
    "ndnet_tr_nll_onehot": "logp gt part loss B C N",
    "ndnet_tr_nll_onehot_bwd": "gt dloss dlogp B C N",
    "ndnet_tr_argmax_match_cm": "pred gt B C N ctr acc",
    "ndnet_tr_point_transform": "t pts pld extra eld x B N",
    "ndnet_tr_point_transform_bwd": "dx pts pld extra eld dt B N",
    "ndnet_tr_adam": "n params grads exp_avg exp_avg_sq steps numel lr beta1 beta2 eps wd",
}
P_ = "P"  # a pointer argument: replaced by its own zeroed 64 KiB buffer


def _bases():
    """The valid calls the rejections are one edit away from: name -> (entry point, arguments)."""
    gemm = dict(A=P_, B=P_, C=P_, bias=None, sbias=0, M=8, N=8, K=8, lda=8, ldb=8, ldc=8, sAz=64, sBz=64, sCz=64,
                batch=2, cpp=1, ak=1, bk=0, nchunks=1, kchunk=8)
    bn = dict(y=P_, z=P_, mean=P_, invstd=P_, rmean=P_, rvar=P_, gamma=P_, beta=P_, B=2, C=2, N=4, eps=EPS, mom=MOM,
              relu=1, pool=None, pool_idx=None, nbt=P_)
    bnb = dict(dz=P_, y=P_, mean=P_, invstd=P_, gamma=P_, beta=P_, dy=P_, dgamma=P_, dbeta=P_, dbias=P_, B=2, C=2, N=4,
               relu=1, pool_idx=P_)
    fc = dict(x=P_, W=P_, bias=P_, y=None, z=P_, mean=None, invstd=None, rmean=None, rvar=None, gamma=None, beta=None,
              B=2, K=8, N=4, ldw=0, eps=EPS, mom=MOM, relu=0, eye=0, nbt=None)
    fcg = dict(fc, y=P_, mean=P_, invstd=P_, rmean=P_, rvar=P_, gamma=P_, beta=P_, relu=1, nbt=P_)
    fcw = dict(dz=P_, x=P_, y=None, mean=None, invstd=None, gamma=None, beta=None, dpre=P_, dW=P_, db=P_, dgamma=None,
               dbeta=None, B=2, K=8, N=4, ldw=0, relu=0)
    fcx = dict(dpre=P_, W=P_, dx=P_, part=None, B=2, K=8, N=4, ldw=0, nsplit=1)
    bcn = dict(B=2, C=4, N=5)
    return {
        "gemm": ("ndnet_tr_gemm", gemm),
        "gemm chunks": ("ndnet_tr_gemm", dict(gemm, nchunks=2, kchunk=4)),
        "gemm groups": ("ndnet_tr_gemm", dict(gemm, cpp=2)),
        "sum_parts_2d": ("ndnet_tr_sum_parts_2d", dict(part=P_, out=P_, rows=2, cols=4, ldo=4, nparts=2)),
        "bn_fwd": ("ndnet_tr_bn_fwd", bn),
        "bn_fwd pool": ("ndnet_tr_bn_fwd", dict(bn, z=None, pool=P_, pool_idx=P_)),
        "bn_bwd pool": ("ndnet_tr_bn_bwd", bnb),
        "fc_fwd": ("ndnet_tr_fc_fwd", fc),
        "fc_fwd gamma": ("ndnet_tr_fc_fwd", fcg),
        "fc_bwd_w": ("ndnet_tr_fc_bwd_w", fcw),
        "fc_bwd_x": ("ndnet_tr_fc_bwd_x", fcx),
        "fc_bwd_x split": ("ndnet_tr_fc_bwd_x", dict(fcx, part=P_, nsplit=2)),
        "log_softmax": ("ndnet_tr_log_softmax_c", dict(x=P_, out=P_, **bcn)),
        "log_softmax_bwd": ("ndnet_tr_log_softmax_c_bwd", dict(y=P_, dy=P_, dx=P_, **bcn)),
        "nll": ("ndnet_tr_nll_onehot", dict(logp=P_, gt=P_, part=P_, loss=P_, **bcn)),
        "nll_bwd": ("ndnet_tr_nll_onehot_bwd", dict(gt=P_, dloss=P_, dlogp=P_, **bcn)),
        "argmax_match_cm": ("ndnet_tr_argmax_match_cm", dict(pred=P_, gt=P_, ctr=P_, acc=P_, **bcn)),
        "point_transform": ("ndnet_tr_point_transform", dict(t=P_, pts=P_, pld=3, extra=P_, eld=9, x=P_, B=2, N=5)),
        "point_transform_bwd": ("ndnet_tr_point_transform_bwd",
                                dict(dx=P_, pts=P_, pld=3, extra=P_, eld=9, dt=P_, B=2, N=5)),
        "adam": ("ndnet_tr_adam", dict(n=2, params="PP", grads="PP", exp_avg="PP", exp_avg_sq="PP", steps="PP",
                                       numel=(16, 16), lr=P_, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.0)),
    }


OFF4 = "P+4"   # a pointer 4 bytes into its buffer (not 16-byte aligned)
# name: (base, edits)
REJECTED = {
    "gemm: bias with nchunks > 1": ("gemm chunks", dict(bias=P_)),
    "gemm: bias with clouds_per_part > 1": ("gemm groups", dict(bias=P_)),
    "gemm: chunks not covering K": ("gemm chunks", dict(kchunk=3)),
    "gemm: a chunk starting outside K": ("gemm chunks", dict(nchunks=3)),
    "gemm: clouds_per_part > batch": ("gemm", dict(cpp=3)),
    "gemm: ldc < N": ("gemm", dict(ldc=7)),
    "gemm: grid z > 65535": ("gemm", dict(batch=65536)),
    "sum_parts_2d: ldo < cols": ("sum_parts_2d", dict(ldo=3)),
    "bn_fwd: pool without pool_idx": ("bn_fwd pool", dict(pool_idx=None)),
    "bn_fwd: pool with B = 65": ("bn_fwd pool", dict(B=65)),
    "bn_fwd: neither z nor pool": ("bn_fwd", dict(z=None)),
    "bn_bwd: pool with B = 65": ("bn_bwd pool", dict(B=65)),
    "fc_fwd: B = 17": ("fc_fwd", dict(B=17)),
    "fc_fwd: K % 4 != 0": ("fc_fwd", dict(K=6)),
    "fc_fwd: ldw < K": ("fc_fwd", dict(ldw=4)),
    "fc_fwd: ldw % 4 != 0": ("fc_fwd", dict(ldw=10)),
    "fc_fwd: misaligned x": ("fc_fwd", dict(x=OFF4)),
    "fc_fwd: misaligned W": ("fc_fwd", dict(W=OFF4)),
    "fc_fwd: B K > 16384": ("fc_fwd", dict(K=8196)),
    "fc_fwd: gamma without y": ("fc_fwd gamma", dict(y=None)),
    "fc_fwd: gamma without mean": ("fc_fwd gamma", dict(mean=None)),
    "fc_fwd: gamma without invstd": ("fc_fwd gamma", dict(invstd=None)),
    "fc_fwd: gamma without beta": ("fc_fwd gamma", dict(beta=None)),
    "fc_fwd: relu without gamma": ("fc_fwd", dict(relu=1)),
    "fc_fwd: batches_tracked without gamma": ("fc_fwd", dict(nbt=P_)),
    "fc_bwd_w: relu without gamma": ("fc_bwd_w", dict(relu=1)),
    "fc_bwd_w: misaligned dW": ("fc_bwd_w", dict(dW=OFF4)),
    "fc_bwd_x: nsplit > N": ("fc_bwd_x split", dict(nsplit=5)),
    "fc_bwd_x: a split wider than 256 channels": ("fc_bwd_x", dict(N=257)),
    "fc_bwd_x: nsplit > 1 without part": ("fc_bwd_x split", dict(part=None)),
    "log_softmax: C = 33": ("log_softmax", dict(C=33)),
    "log_softmax_bwd: C = 33": ("log_softmax_bwd", dict(C=33)),
    "nll: C = 33": ("nll", dict(C=33)),
    "nll_bwd: C = 33": ("nll_bwd", dict(C=33)),
    "argmax_match_cm: C = 33": ("argmax_match_cm", dict(C=33)),
    "point_transform: pld = 2": ("point_transform", dict(pld=2)),
    "point_transform: eld = 8": ("point_transform", dict(eld=8)),
    "point_transform_bwd: pld = 2": ("point_transform_bwd", dict(pld=2)),
    "point_transform_bwd: eld = 8": ("point_transform_bwd", dict(eld=8)),
    "adam: n = 0": ("adam", dict(n=0)),
    "adam: a NULL step pointer": ("adam", dict(steps="P0")),
    "adam: numel = 0": ("adam", dict(numel=(16, 0))),
}


def _arg_call(base, edits, device):
    fn, args = _bases()[base]
    args = dict(args, **edits)
    keep, vals = [], []

    def buf():
        keep.append(torch.zeros(16384, device=device))
        return keep[-1].data_ptr()

    for k in ARG_ORDER[fn].split():
        v = args[k]
        if v == P_:
            v = buf()
        elif v == OFF4:
            v = buf() + 4
        elif v in ("PP", "P0"):
            v = (ctypes.c_void_p * 2)(buf(), buf() if v == "PP" else None)
            keep.append(v)
        elif k == "numel":
            v = (ctypes.c_int64 * 2)(*v)
            keep.append(v)
        vals.append(v)
    rc = getattr(_lib(), fn)(*vals, None)
    if device != "cpu":
        torch.cuda.synchronize()
    del keep
    return rc


@pytest.mark.parametrize("case", sorted(REJECTED))
def test_inconsistent_arguments_are_rejected(case):
    """NDNET_ERR_ARG (-20) for every documented rejection, before anything is launched (host memory, no GPU)."""
    assert _arg_call(*REJECTED[case], "cpu") == -20


@pytest.mark.gpu
@pytest.mark.parametrize("base", sorted(_bases()))
def test_unedited_arguments_are_accepted(base):
    """The call each rejection is one edit away from is itself valid: it returns 0 on the GPU (over zeros)."""
    assert _arg_call(base, {}, "cuda") == 0


# ---------------------------------------------------------------- variant builds in child processes

def _child(env_extra, select, timeout=420):
    """This file's GPU cases matching `select` (never the *_child_* tests) in a fresh process with only
    NDNET_TR_* variables added."""
    assert all(k.startswith("NDNET_TR_") for k in env_extra)
    env = dict(os.environ, **env_extra)
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider", __file__, "-m", "gpu",
                        "-k", f"({select}) and not child"], env=env, capture_output=True, text=True, timeout=timeout,
                       cwd=os.path.dirname(os.path.abspath(__file__)))
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    return r


@pytest.mark.gpu
def test_child_wide_tiles():
    """NDNET_TR_WIDE_MIN=1 with NDNET_TR_X6=0: the 128 x 128 tile tails, M, N in
    {128, 129, 191, 256} over the k tails, all four layouts on the fp32 kernel."""
    _child({"NDNET_TR_WIDE_MIN": "1", "NDNET_TR_X6": "0"}, "test_gemm_tile or test_gemm_split or test_gemm_wide")


@pytest.mark.gpu
def test_child_kt16_is_bit_identical(tmp_path):
    """NDNET_TR_KT=1 (16-deep k steps) with NDNET_TR_BN1024=0 (512-thread
    BatchNorm workgroups for every C): the GEMM and BatchNorm cases again, and
    the header's "same sums in the same order": the products of a KT=1 child and
    of a default child are equal bit for bit."""
    a, b = str(tmp_path / "kt16.pt"), str(tmp_path / "kt32.pt")
    _child({"NDNET_TR_KT": "1", "NDNET_TR_BN1024": "0", "NDNET_TR_TEST_DUMP": a}, "test_gemm or test_bn or test_sum")
    _child({"NDNET_TR_TEST_DUMP": b}, "test_gemm_dump")
    for x, y in zip(torch.load(a), torch.load(b)):
        assert torch.equal(x, y)


@pytest.mark.gpu
def test_child_x6_all_bn1024_everywhere():
    """NDNET_TR_X6=all (every layout on the split-bf16 kernel) with NDNET_TR_BN1024=2 (1024 threads for C = 512 too)."""
    _child({"NDNET_TR_X6": "all", "NDNET_TR_BN1024": "2"}, "test_gemm or test_bn")


@pytest.mark.gpu
def test_child_x6_off_gemm64():
    """NDNET_TR_X6=0 (both operands k-major on the fp32 kernel) with NDNET_TR_GEMM64=1 (64 x 64 tiles only)."""
    _child({"NDNET_TR_X6": "0", "NDNET_TR_GEMM64": "1"}, "test_gemm")
