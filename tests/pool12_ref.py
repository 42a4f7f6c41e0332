"""Chain C as one per-cloud 12 -> F layer, restated in torch (the reference
of tests/test_pool12_cpu.py, tests/test_pn_pool12.py).

conv1 (with t1 and t2 folded: per-cloud W0 [B,12,64], b0 [B,64]), conv2
(w_mid [64,128], b_mid) and conv3 (w_tail [128,Fp], b_tail) have no ReLU
between them (ndtnet.py:149-161), so

  g3[b] = max_n (x[b,n] Wc[b]) + bc[b],
  Wc[b] = W0[b] w_mid w_tail,  bc[b] = (b0[b] w_mid + b_mid) w_tail + b_tail.
"""
import torch

U = 2.0 ** -24  # fp32 unit roundoff


def collapse(w0, b0, w_mid, b_mid, w_tail, b_tail):
    """(Wc [B,12,Fp], bc [B,Fp]) in float64."""
    w0, b0, w_mid, b_mid, w_tail, b_tail = (t.double() for t in (w0, b0, w_mid, b_mid, w_tail, b_tail))
    wc = w0 @ w_mid @ w_tail
    bc = (b0 @ w_mid + b_mid) @ w_tail + b_tail
    return wc, bc


def pooled(x, wc, bc):
    """max over the points of x[..., :12] Wc, plus bc, in the dtype of wc."""
    return (x[..., :12].to(wc.dtype) @ wc).amax(dim=1) + bc


def bound(x, wc64, g64):
    """Per column: 15 * 2^-24 * max_n sum_k |x_nk| |Wc_kf| + 2^-23 |g3|.

    Twelve rounded products / FMAs and Wc's one rounding are 13 u S with
    S = sum_k |x_k| |Wc_k|; the rounded bias is off by u |bc| <= u (|g3| + S)
    and its addition by u |g3|: 14 u S + 2 u |g3|, under the 15 u S + 2 u |g3|
    the tests hold the kernel to."""
    s = (x[..., :12].double().abs() @ wc64.abs()).amax(dim=1)
    return 15 * U * s + 2 * U * g64.abs()


def _fma32(a, b, c):
    """fl32(a * b + c) for fp32 values held in float64: the product is exact
    in float64 (48 bits), the sum is rounded to 53 bits and then to 24."""
    return (a * b + c).float().double()


def pooled_fp32(x, wc64, bc64):
    """The kernel's arithmetic on the CPU: Wc and bc rounded once to fp32,
    twelve fp32 FMAs per point and column with k ascending from 0, the maximum
    over the points, the bias added to the maximum.  Returns float32."""
    wc = wc64.float().double()
    xs = x[..., :12].float().double()
    acc = torch.zeros(xs.shape[0], xs.shape[1], wc.shape[2], dtype=torch.float64)
    for k in range(12):
        acc = _fma32(xs[:, :, k:k + 1], wc[:, k:k + 1, :], acc)
    return (acc.amax(dim=1) + bc64.float().double()).float()
