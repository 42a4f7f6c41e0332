"""The per-cloud eval kernels between the chains (include/ndnet_pointnet.h:
ndnet_pn_fc_run, ndnet_pn_fc_mfma_run, ndnet_pn_head3_run,
ndnet_pn_fold_t2_run) driven directly at the C ABI, at shapes, strides and
batch sizes the model never uses, against the same operation in float64.

Bound of every comparison, as in test_pn_chain.py: with e_hip = max |HIP -
float64| and e_t = the error of the same operation in torch fp32 on the same
device (addmm / matmul + relu) against the same float64 result,
e_hip <= 3 e_t + 1e-6 max |float64 result|.  Every case prints e_hip, e_t
and their ratio.  Activations are non-negative with exact zeros (as after a
ReLU), weights randn / sqrt(K), biases 0.5 randn; pad columns of the inputs
hold NaN and outputs are pre-filled with a NaN bit pattern that everything
outside the result must keep."""
import itertools
import math

import pytest
import torch

from test_pn_chain import _gen, _kept, _padded, _ph, _report, _sentinel  # NAN_BITS-filled buffers, the bound

ERR_ARG = -20


def _lib():
    from ndnet import _lib
    return _lib


def _acts(g, *shape):
    """Non-negative activations, about one in six exactly zero."""
    return torch.relu(torch.randn(*shape, generator=g) + 1.0)


def _clouds_differ(pre):
    """Every two clouds' rows differ by far more than the bound (about 1e-6)."""
    d = (pre[:, None, :] - pre[None, :, :]).abs().amax(dim=2)
    d.fill_diagonal_(float("inf"))
    return bool((d > 1e-4).all())


# ---- the FC layers: ndnet_pn_fc_run (k_pn_fc, k_pn_fc_split<2>, <4>) and ndnet_pn_fc_mfma_run ----

def _fc_operands(g, batch, K, N):
    """CPU operands of one FC layer and its float64 pre-activations."""
    x, w, b = _acts(g, batch, K), torch.randn(N, K, generator=g) / math.sqrt(K), torch.randn(N, generator=g) * 0.5
    return x, w, b, x.double() @ w.double().t() + b.double()


def _fc_launch(entry, x, wdev, b, batch, K, N, relu, ld_in, ld_out):
    """One launch over an input of exactly `batch` rows with NaN pad columns;
    the result [batch][N] in float64 after the check of out's pad columns."""
    L = _lib()
    xin, bd = _padded(x, ld_in).cuda(), b.cuda()
    out = _sentinel(batch, ld_out)
    rc = getattr(L.lib(), entry)(xin.data_ptr(), ld_in, wdev.data_ptr(), bd.data_ptr(), out.data_ptr(), ld_out,
                                 batch, K, N, relu, L.stream_ptr(xin.device))
    assert rc == 0, f"{entry} returned {rc}"
    torch.cuda.synchronize()
    assert _kept(out[:, N:]), "columns N..ld_out of out were written"
    return out[:, :N].double().cpu()


def _fc_torch_error(x, w, b, relu, ref):
    t = torch.addmm(b.cuda(), x.cuda(), w.cuda().t())
    return ((torch.relu(t) if relu else t).double().cpu() - ref).abs().max().item()


FC_K = [4, 12, 252, 256, 260, 512, 768, 1024, 1028, 2048]
FC_N = [1, 2, 3, 5, 9]
FC_BATCH = [1, 7, 16]


def _fc_cases(K):
    """Every N tail with every batch; relu and the padded strides alternate
    so that each N meets both values of each."""
    g = _gen(1000 + K)
    for i, (N, batch) in enumerate(itertools.product(FC_N, FC_BATCH)):
        relu, pad = (i + i // 3) % 2, (i // 2) % 2
        yield (N, batch, relu, pad) + _fc_operands(g, batch, K, N)


def test_fc_cases_have_both_signs_and_distinct_clouds():
    """What the GPU test below relies on, checked on the float64 references:
    pre-activations of both signs in every case of five columns or more (and
    over each K's cases together), clouds that differ, and for every N both
    ReLU settings and both stride settings."""
    for K in FC_K:
        seen, signs = set(), [False, False]
        for N, batch, relu, pad, x, w, b, pre in _fc_cases(K):
            seen.add((N, relu))
            seen.add((N, "pad", pad))
            signs = [signs[0] or bool((pre < 0).any()), signs[1] or bool((pre > 0).any())]
            if N >= 5:  # a column's sign is mostly that of its bias and weight sum: the signs differ across columns
                assert (pre < 0).any() and (pre > 0).any(), (K, N, batch)
            if batch > 1 and N >= 2:
                assert _clouds_differ(pre), (K, N, batch)
            assert (x == 0).any() or x.numel() < 64
        assert all(signs)
        assert all((N, r) in seen and (N, "pad", r) in seen for N in FC_N for r in (0, 1))


@pytest.mark.gpu
@pytest.mark.parametrize("K", FC_K)
def test_fc_gemv_against_float64(K):
    """ndnet_pn_fc_run: K = 256 the one-wave kernel by the dispatch rule, 512
    k_pn_fc_split<2>, 1024 k_pn_fc_split<4>, every other K the generic loop
    (4: one float4, lanes 1..63 idle; 260: a second pass with one lane; 768:
    three passes).  N = 1, 2, 3, 5, 9: the 4- and 2-outputs-per-workgroup tails
    and the clamp on odd N.  ld_in = K, ld_out = N and ld_in = K + 4, ld_out =
    N + 3."""
    bad = []
    for N, batch, relu, pad, x, w, b, pre in _fc_cases(K):
        ref = torch.relu(pre) if relu else pre
        got = _fc_launch("ndnet_pn_fc_run", x, w.cuda(), b, batch, K, N, relu, K + 4 * pad, N + 3 * pad)
        _report(f"fc K={K} N={N} batch={batch} relu={relu} pad={pad}", got, ref, _fc_torch_error(x, w, b, relu, ref), bad)
    assert not bad, bad


def _fc_mfma_case(seed, batch, K, N, relu, bad, ld_in=None, ld_out=None):
    """One ndnet_pn_fc_mfma_run launch against float64; returns its result."""
    x, w, b, pre = _fc_operands(_gen(seed), batch, K, N)
    assert (pre < 0).any() and (pre > 0).any()
    assert batch == 1 or _clouds_differ(pre)
    ref = torch.relu(pre) if relu else pre
    wf = _ph()._frag(w.t().contiguous().cuda())
    got = _fc_launch("ndnet_pn_fc_mfma_run", x, wf, b, batch, K, N, relu, ld_in or K + 4, ld_out or N + 3)
    _report(f"fc_mfma K={K} N={N} batch={batch} relu={relu}", got, ref, _fc_torch_error(x, w, b, relu, ref), bad)
    return got, (x, wf, b)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [16, 48, 112, 128, 144, 1024])
def test_fc_mfma_k_group_split(K):
    """K / 16 = 1, 3, 7, 8, 9, 64 k-groups over the 8 waves: below 8 some waves
    own none and still add a (zero) partial tile; 9 splits unevenly.  Rows of
    ld_in = K + 4 floats with NaN pads, ld_out = N + 3."""
    bad = []
    for i, (N, batch) in enumerate(itertools.product([16, 48], [1, 5, 16])):
        _fc_mfma_case(2000 + K + i, batch, K, N, (i + i // 3) % 2, bad)
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize("K,N,blocks", [(512, 1024, 2), (272, 1024, 2), (256, 2048, 4), (1024, 512, 1)])
def test_fc_mfma_column_block_widths(K, N, blocks):
    """Column blocks per workgroup by fc_mfma_cbw (4, else 2, while N / 16 /
    blocks >= 32 workgroups remain and ceil(K / 128) * blocks <= 8 fragments
    per wave): (512, 1024) and (272, 1024) run two blocks (64 / 4 = 16
    workgroups would be too few for four), (256, 2048) four, (1024, 512) one
    (8 k-groups per wave leave room for no second block).  Each against
    float64; then the same layer as 512-column slices, which run one block
    per workgroup: bit-identical to the single launch."""
    L = _lib()
    bad = []
    batch, relu = (16, 0) if K != 272 else (5, 1)
    got, (x, wf, b) = _fc_mfma_case(3000 + K + N, batch, K, N, relu, bad, ld_in=K, ld_out=N)
    assert not bad, bad
    if N == 512:
        return
    xd, bd = x.cuda(), b.cuda()
    sliced = _sentinel(batch, N)
    for s in range(N // 512):
        rc = L.lib().ndnet_pn_fc_mfma_run(xd.data_ptr(), K, wf.data_ptr() + 4 * K * 512 * s, bd.data_ptr() + 4 * 512 * s,
                                          sliced.data_ptr() + 4 * 512 * s, N, batch, K, 512, relu, L.stream_ptr(xd.device))
        assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(sliced.double().cpu(), got), f"{blocks} blocks per workgroup differ from one"


# ---- ndnet_pn_head3_run ----

H3_K = [1, 63, 64, 65, 256, 300]
H3_KIN = [3, 12, 16]
H3_NOUT = [16, 64, 128, 320]
H3_BATCH = [1, 3, 16]
# every nout with every kin, twice; K, batch and the stride of h2 rotate at different periods
H3_CASES = [(H3_K[(i + i // 6) % 6], kin, nout, H3_BATCH[(i + r + i // 3) % 3], (i + r) % 2)
            for r in range(2) for i, (nout, kin) in enumerate(itertools.product(H3_NOUT, H3_KIN))]


def test_head3_cases_cover_the_parameters():
    """Every nout meets every kin, batch and stride; every K and kin both strides; every kin every batch."""
    pairs = lambda i, j: {(c[i], c[j]) for c in H3_CASES}  # noqa: E731
    assert pairs(1, 2) == set(itertools.product(H3_KIN, H3_NOUT))
    assert pairs(2, 3) == set(itertools.product(H3_NOUT, H3_BATCH)) and pairs(2, 4) == set(itertools.product(H3_NOUT, (0, 1)))
    assert pairs(0, 4) == set(itertools.product(H3_K, (0, 1))) and pairs(1, 4) == set(itertools.product(H3_KIN, (0, 1)))
    assert pairs(1, 3) == set(itertools.product(H3_KIN, H3_BATCH))


def _head3_operands(g, batch, K, kin, nout):
    """h2, W3, b3, a dense basis; float64 t1 [batch][9] and W [batch][kin][nout]."""
    h2 = _acts(g, batch, K)
    if K == 1:  # one activation per cloud: distinct values, a single exact zero (two zeros are two equal clouds)
        h2 = torch.rand(batch, 1, generator=g) * 2 + 0.1
        h2[0] = 0.0
    w3, b3 = torch.randn(9, K, generator=g) / math.sqrt(K), torch.randn(9, generator=g) * 0.5
    basis = torch.randn(9, kin * nout, generator=g) / 3.0
    t1 = h2.double() @ w3.double().t() + b3.double()
    return h2, w3, b3, basis, t1, (t1 @ basis.double()).view(batch, kin, nout)


def _frag16(w):
    """[batch][kin][nout] -> fragment-major with K padded to 16 (zero rows)."""
    return _ph()._frag(torch.nn.functional.pad(w, (0, 0, 0, 16 - w.shape[1])))


@pytest.mark.gpu
@pytest.mark.parametrize("K,kin,nout,batch,pad", H3_CASES)
def test_head3_against_float64(K, kin, nout, batch, pad):
    """t1 = h2 @ W3^T + b3 and W[k][n] = sum_a t1[a] basis[a][k nout + n] in
    the fragment layout (K padded to 16): nout 128 and 320 run the loop past
    the first 1024 positions; the basis is dense, so a wrong a, k or n shows.
    Rows kin..15 are exactly 0 and nothing past batch * 16 * nout floats (or
    batch * 9 of t1) is written."""
    L = _lib()
    h2, w3, b3, basis, t1_ref, w_ref = _head3_operands(_gen(4000 + 7 * K + kin + nout + batch), batch, K, kin, nout)
    assert batch == 1 or _clouds_differ(t1_ref)
    ld_h = K + 5 * pad
    dev = [t.cuda() for t in (_padded(h2, ld_h), w3, b3, basis)]
    total = batch * 16 * nout
    t1, w1f = _sentinel(batch * 9 + 7), _sentinel(total + 64)
    rc = L.lib().ndnet_pn_head3_run(dev[0].data_ptr(), ld_h, dev[1].data_ptr(), dev[2].data_ptr(), dev[3].data_ptr(),
                                    t1.data_ptr(), w1f.data_ptr(), batch, K, kin, nout, L.stream_ptr(t1.device))
    assert rc == 0
    torch.cuda.synchronize()
    assert _kept(t1[batch * 9:]) and _kept(w1f[total:]), "written past the result"
    # torch fp32 on the device
    t1_t = torch.addmm(dev[2], h2.cuda(), dev[1].t())
    w_t = torch.matmul(t1_t, dev[3]).view(batch, kin, nout)
    bad = []
    name = f"head3 K={K} kin={kin} nout={nout} batch={batch} pad={pad}"
    _report(name + " t1", t1[: batch * 9].view(batch, 9).double().cpu(), t1_ref,
            (t1_t.double().cpu() - t1_ref).abs().max().item(), bad)
    got = w1f[:total].view(batch, 16 * nout).cpu()
    _report(name + " w1f", got.double(), _frag16(w_ref), (w_t.double().cpu() - w_ref).abs().max().item(), bad)
    rows = _frag16(torch.arange(16.0)[None, :, None].expand(1, 16, nout))[0]
    assert bool((got[:, rows >= kin] == 0).all()), "rows kin..15 are not exactly 0"
    assert not bad, bad


# ---- ndnet_pn_fold_t2_run ----

@pytest.mark.gpu
@pytest.mark.parametrize("t2_ld", [4096, 4100])
@pytest.mark.parametrize("w1_stride", [1024, 1088])
@pytest.mark.parametrize("batch", [1, 3, 17])
def test_fold_t2_against_float64(batch, w1_stride, t2_ld):
    """outf[b] = W1'^T[b] (12 x 64) @ t2[b] in the K = 16 fragment layout and
    outb[b] = b1^T t2[b]; t2 dense per cloud.  Rows 12..15 of the input hold
    NaN (ignored) and rows 12..15 of outf keep their bits; batch 17 is past
    the 16 of the other per-cloud kernels."""
    L = _lib()
    g = _gen(5000 + batch + w1_stride + t2_ld)
    w = torch.randn(batch, 12, 64, generator=g) / math.sqrt(12)
    b1 = torch.randn(64, generator=g) * 0.5
    t2 = torch.randn(batch, 64, 64, generator=g) / 8.0
    wf_ref, b_ref = w.double() @ t2.double(), b1.double() @ t2.double()
    assert batch == 1 or _clouds_differ(b_ref)
    w16 = torch.full((batch, 16, 64), float("nan"))
    w16[:, :12] = w
    win = _padded(_ph()._frag(w16), w1_stride).cuda()
    t2in = _padded(t2.view(batch, 4096), t2_ld).cuda()
    b1d = b1.cuda()
    outf, outb = _sentinel(batch * 1024 + 64), _sentinel(batch * 64 + 64)
    rc = L.lib().ndnet_pn_fold_t2_run(win.data_ptr(), w1_stride, b1d.data_ptr(), t2in.data_ptr(), t2_ld,
                                      outf.data_ptr(), outb.data_ptr(), batch, L.stream_ptr(win.device))
    assert rc == 0
    torch.cuda.synchronize()
    assert _kept(outf[batch * 1024:]) and _kept(outb[batch * 64:]), "written past the result"
    rows = _frag16(torch.arange(16.0)[None, :, None].expand(1, 16, 64))[0]
    got = outf[: batch * 1024].view(batch, 1024).cpu()
    assert _kept(got[:, rows >= 12]), "rows 12..15 of outf were written"
    wd, td = w.cuda(), t2.cuda()
    e_w = (torch.matmul(wd, td).double().cpu() - wf_ref).abs().max().item()
    e_b = (torch.matmul(b1d, td).double().cpu() - b_ref).abs().max().item()
    bad = []
    name = f"fold_t2 batch={batch} w1_stride={w1_stride} t2_ld={t2_ld}"
    _report(name + " outf", got[:, rows < 12].double(), _frag16(wf_ref)[:, rows < 12], e_w, bad)
    _report(name + " outb", outb[: batch * 64].view(batch, 64).double().cpu(), b_ref, e_b, bad)
    assert not bad, bad


# ---- argument checks: rejected before any launch, so these run without a GPU ----

def _fc_call(edit, device="cpu"):
    """A valid ndnet_pn_fc_run (batch 2, K 8, N 3, rows of 12 and 5 floats), changed by `edit(args)`."""
    L = _lib()
    x, w, b, out = (torch.zeros(*s, device=device) for s in ((2, 12), (3, 8), (3,), (2, 5)))
    a = dict(x=x.data_ptr(), ld_in=12, w=w.data_ptr(), b=b.data_ptr(), out=out.data_ptr(), ld_out=5, batch=2, K=8, N=3)
    edit(a)
    rc = L.lib().ndnet_pn_fc_run(a["x"], a["ld_in"], a["w"], a["b"], a["out"], a["ld_out"], a["batch"], a["K"], a["N"],
                                 1, None)
    if device != "cpu":
        torch.cuda.synchronize()
    return rc


FC_ARG_CASES = {
    "ld_in < K": lambda a: a.update(ld_in=4),
    "ld_out < N": lambda a: a.update(ld_out=2),
    "ld_in % 4": lambda a: a.update(ld_in=10),
    "K % 4": lambda a: a.update(K=6),
    "batch > 16": lambda a: a.update(batch=17),
    "in misaligned": lambda a: a.update(x=a["x"] + 4),
    "NULL out": lambda a: a.update(out=None),
}


@pytest.mark.parametrize("case", sorted(FC_ARG_CASES))
def test_fc_run_rejects_inconsistent_arguments(case):
    assert _fc_call(FC_ARG_CASES[case]) == ERR_ARG


@pytest.mark.gpu
def test_fc_run_accepts_the_unedited_call():
    assert _fc_call(lambda a: None, device="cuda") == 0


def _head3_call(edit, device="cpu"):
    """A valid ndnet_pn_head3_run (batch 2, K 8 in rows of 12, kin 3, nout 16), changed by `edit(args)`."""
    L = _lib()
    h2, w3, b3, basis, t1, w1f = (torch.zeros(*s, device=device) for s in ((2, 12), (9, 8), (9,), (9, 48), (2, 9), (2, 256)))
    a = dict(h2=h2.data_ptr(), ld_h=12, w3=w3.data_ptr(), b3=b3.data_ptr(), basis=basis.data_ptr(), t1=t1.data_ptr(),
             w1f=w1f.data_ptr(), batch=2, K=8, kin=3, nout=16)
    edit(a)
    rc = L.lib().ndnet_pn_head3_run(a["h2"], a["ld_h"], a["w3"], a["b3"], a["basis"], a["t1"], a["w1f"], a["batch"],
                                    a["K"], a["kin"], a["nout"], None)
    if device != "cpu":
        torch.cuda.synchronize()
    return rc


HEAD3_ARG_CASES = {
    "ld_h < K": lambda a: a.update(ld_h=7),
    "kin > 16": lambda a: a.update(kin=17),
    "kin < 1": lambda a: a.update(kin=0),
    "nout % 16": lambda a: a.update(nout=24),
    "K < 1": lambda a: a.update(K=0),
    "NULL basis": lambda a: a.update(basis=None),
}


@pytest.mark.parametrize("case", sorted(HEAD3_ARG_CASES))
def test_head3_run_rejects_inconsistent_arguments(case):
    assert _head3_call(HEAD3_ARG_CASES[case]) == ERR_ARG


@pytest.mark.gpu
def test_head3_run_accepts_the_unedited_call():
    assert _head3_call(lambda a: None, device="cuda") == 0
