"""The point-level loss on the GPU: the row histogram (ndnet_seg_row_hist)
against ``np.add.at`` and against the labelled NDT run's own per-voxel classes
and counts, the loss / gradient / accuracy kernels (ndnet_tr_nll_hist[_bwd],
ndnet_tr_hist_match_cm) at the C ABI against float64 and integer references,
their identity with the evaluation stack (``point_labels`` + ``confusion``), and
the trainer with ``loss="points"``, eager and graphed, on a ragged batch.

Numeric bound, as the "nll" family of tests/test_train_kernels.py:
max |hip - ref64| <= 3 e_t + 1e-6 max |ref64| with e_t the error of the same
formula in fp32 torch on the same device.  Integer results are exact.  Every C
ABI output lies between two pads of NAN_BITS words that must stay untouched."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FC0BEEF  # the sentinel of words a kernel must not touch
PAD = 256              # sentinel words on either side of every buffer
FACTOR = 3.0
INT32_MIN = -2 ** 31


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _lib():
    from ndnet import _lib
    return _lib.lib()


def _st():
    return torch.cuda.current_stream().cuda_stream


class Buf:
    """n 4-byte words of device memory between two pads of NAN_BITS, the words
    themselves NAN_BITS until written (as tests/test_train_kernels.py has it)."""

    def __init__(self, n, dtype=torch.float32, device="cuda"):
        self.n, self.lo = n, PAD
        self.raw = torch.full((PAD + n + PAD,), NAN_BITS, dtype=torch.int32, device=device)
        self.words = self.raw[self.lo:self.lo + n]
        self.t = self.words.view(dtype)
        self.ptr = self.t.data_ptr()

    @classmethod
    def of(cls, x):
        x = x.contiguous()
        b = cls(x.numel() * x.element_size() // 4, x.dtype, x.device)
        b.t.copy_(x.reshape(-1))
        return b

    def surround_ok(self):
        return bool((self.raw[:self.lo] == NAN_BITS).all()) and bool((self.raw[self.lo + self.n:] == NAN_BITS).all())

    def written(self):
        return not bool((self.words == NAN_BITS).any())


def _cmp(name, hip, ref, t32, bad):
    """e_hip <= FACTOR e_t + 1e-6 max |ref|; prints the figures, appends a failure to `bad`."""
    hip, ref, t32 = hip.double(), ref.double(), t32.double()
    assert hip.shape == ref.shape == t32.shape, (name, hip.shape, ref.shape, t32.shape)
    fin = bool(torch.isfinite(hip).all())
    e_hip = (hip - ref).abs().max().item() if fin else float("inf")
    e_t = (t32 - ref).abs().max().item()
    scale = ref.abs().max().item()
    print(f"RATIO nll_hist {name}: e_hip {e_hip:.3e} e_t {e_t:.3e} scale {scale:.3e}")
    if not e_hip <= FACTOR * e_t + 1e-6 * scale:
        bad.append((name, e_hip, e_t, scale))


# ---------------------------------------------------------------- 1: the histogram against np.add.at

def _np_hist(rows, labels, k, cols, ignore):
    B = rows.shape[0]
    h = np.zeros((B, k, cols), np.int32)
    ok = (rows >= 0) & (rows < k) & (labels >= 0) & (labels < cols) & (labels != ignore)
    b = np.broadcast_to(np.arange(B)[:, None], rows.shape)
    np.add.at(h, (b[ok], rows[ok], labels[ok]), 1)
    return h


def _hip_hist(rows, labels, k, cols, ignore):
    """ndnet_seg_row_hist into a garbage-filled table between sentinels."""
    B, n = rows.shape
    rb, lb = Buf.of(torch.from_numpy(rows).cuda()), Buf.of(torch.from_numpy(labels).cuda())
    hb = Buf(B * k * cols, torch.int32)
    hb.t.copy_(torch.randint(-1000, 1000, (B * k * cols,), dtype=torch.int32, device="cuda"))
    assert _lib().ndnet_seg_row_hist(rb.ptr, lb.ptr, B, n, k, cols, ignore, hb.ptr, _st()) == 0
    torch.cuda.synchronize()
    assert hb.surround_ok() and rb.surround_ok() and lb.surround_ok(), "words outside the table were written"
    return hb.t.view(B, k, cols).cpu().numpy()


HIST_SHAPES = [(1, 1, 1, 1), (2, 63, 5, 2), (3, 4097, 128, 29), (2, 5000, 1000, 29), (2, 3000, 7, 65),
               (1, 2000, 3, 301)]


@pytest.mark.parametrize("shape", HIST_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_row_hist_equals_np_add_at(shape):
    B, n, k, cols = shape
    rng = np.random.default_rng(sum(shape))
    for ignore in (-1, cols // 2):
        rows = rng.integers(-1, k + 1, (B, n)).astype(np.int32)       # -1 and k among them
        labels = rng.integers(-1, cols + 1, (B, n)).astype(np.int32)  # -1 and cols among them
        if n >= 8:
            rows[0, :3] = (-1, k, INT32_MIN)
            rows[-1, 3:8] = k - 1
            labels[-1, 3:6] = (-1, cols, cols // 2)
            labels[-1, 6:8] = (0, cols - 1)
        want = _np_hist(rows, labels, k, cols, ignore)
        got = _hip_hist(rows, labels, k, cols, ignore)
        assert np.array_equal(got, want), (shape, ignore)
        if n >= 8:
            assert 0 < int(want.sum()) < B * n
    # (1, 1, 1, 1): the one point counted, and left out
    if shape == (1, 1, 1, 1):
        one = np.zeros((1, 1), np.int32)
        assert _hip_hist(one, one, 1, 1, -1).tolist() == [[[1]]]
        assert _hip_hist(one, one, 1, 1, 0).tolist() == [[[0]]]
        assert _hip_hist(one - 1, one, 1, 1, -1).tolist() == [[[0]]]


def test_row_hist_every_point_in_one_cell_and_python_wrapper():
    from ndnet import segment
    B, n, k, cols = 2, 5000, 1000, 29
    rows, labels = np.full((B, n), 7, np.int32), np.full((B, n), 3, np.int32)
    want = np.zeros((B, k, cols), np.int32)
    want[:, 7, 3] = n
    assert np.array_equal(_hip_hist(rows, labels, k, cols, -1), want)
    assert not _hip_hist(rows, labels, k, cols, 3).any()
    # the wrapper: a new table, and `out` overwritten whole
    r, l_ = torch.from_numpy(rows).cuda(), torch.from_numpy(labels).cuda()
    h = segment.row_histogram(r, l_, k, cols)
    assert h.dtype == torch.int32 and h.shape == (B, k, cols) and np.array_equal(h.cpu().numpy(), want)
    out = torch.full((B, k, cols), 99, dtype=torch.int32, device="cuda")
    assert segment.row_histogram(r, l_, k, cols, ignore_label=5, out=out) is out
    assert np.array_equal(out.cpu().numpy(), want)


def test_row_hist_is_capturable():
    """No allocation and no synchronisation: the call, its clearing included, replays from a graph."""
    from ndnet import segment
    B, n, k, cols = 2, 3000, 50, 6
    rng = np.random.default_rng(5)
    rows = torch.from_numpy(rng.integers(-1, k, (B, n)).astype(np.int32)).cuda()
    labels = torch.from_numpy(rng.integers(0, cols, (B, n)).astype(np.int32)).cuda()
    out = torch.empty((B, k, cols), dtype=torch.int32, device="cuda")
    segment.row_histogram(rows, labels, k, cols, out=out)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        segment.row_histogram(rows, labels, k, cols, out=out)
    for seed in (6, 7):  # new inputs and garbage in the table before every replay
        r2 = rng.integers(-1, k, (B, n)).astype(np.int32)
        rows.copy_(torch.from_numpy(r2))
        out.fill_(seed)
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), _np_hist(r2, labels.cpu().numpy(), k, cols, -1))


# ---------------------------------------------------------------- 2: the histogram against the labelled run

K = 128
N4K, COUNTS8 = 4096, (4096, 2003, 3001, 1024, 640, 129, 1025, 2048)


@functools.lru_cache(maxsize=None)
def _cloud(kind, n_max, seed):
    from ndnet.synthetic import lidar_cloud, uniform_cloud
    a = {"U": uniform_cloud, "L": lidar_cloud}[kind](n_max, seed)
    a.setflags(write=False)
    return a


def _padded(kind, n_max, counts, seed0=0, pad=np.nan):
    """[B, n_max, 3] float32: cloud b = the first counts[b] points of cloud (n_max, seed0 + b), the rest `pad`."""
    pts = np.stack([_cloud(kind, n_max, seed0 + b) for b in range(len(counts))]).copy()
    for b, c in enumerate(counts):
        pts[b, c:] = pad
    return pts


def _nd_n_alive(plan, cloud, nd):
    from ndnet import _lib
    nd_n, alive, it = np.zeros(nd, np.uint32), np.zeros(nd, np.uint8), ctypes.c_uint32(0)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    rc = _lib.lib().ndnet_ndt_debug_dump(plan.handle, cloud, p(nd_n), None, None, None, None, None, None, None, None,
                                         None, ctypes.byref(it), p(alive))
    assert rc == 0
    return nd_n, alive


@pytest.mark.parametrize("kind", ["U", "L"])
def test_row_hist_equals_the_labelled_runs_voxel_classes_and_counts(kind):
    from ndnet import segment
    from ndnet.preprocessing.ndtnet_preprocessing import NdtPlan
    ncls, B = 5, 8
    labels = np.stack([np.random.default_rng(100 + b).integers(0, 6, N4K) for b in range(B)]).astype(np.int32)
    d_pts = torch.from_numpy(_padded(kind, N4K, COUNTS8)).cuda()
    d_counts = torch.tensor(COUNTS8, dtype=torch.int32, device="cuda")
    paths = (1, 2) if NdtPlan(B, N4K, K, -1).path == 2 else (1,)
    tables = []
    for path in paths:
        for fill in (5, 0):  # the padding's labels
            lb = labels.copy()
            for b, c in enumerate(COUNTS8):
                lb[b, c:] = fill
            plan = NdtPlan(B, N4K, K, ncls)
            plan.set_path(path)
            d_lb = torch.from_numpy(lb).cuda()
            block = torch.empty((B, K, 12), dtype=torch.float32, device="cuda")
            cls = torch.empty((B, K, ncls + 1), dtype=torch.float32, device="cuda")
            plan.run(d_pts, d_lb, block, cls, counts=d_counts)
            rows = plan.point_rows(d_pts, fill="none", counts=d_counts)
            hist = segment.row_histogram(rows, d_lb, K, ncls + 1).cpu().numpy()
            torch.cuda.synchronize()
            plan.raise_sync_failures()
            stats, onehot = plan.host_stats(), cls.cpu().numpy()
            for b, s in enumerate(stats):
                assert s.rc == 0, (path, b)
                nout = min(int(s.num_out), K)
                assert nout > 0
                # np.argmax: the first maximum, as k_welford_q picks the class of a voxel
                assert np.array_equal(hist[b, :nout].argmax(1), onehot[b, :nout].argmax(1)), (path, fill, b)
                nd_n, alive = _nd_n_alive(plan, b, int(s.num_nds))
                assert np.array_equal(hist[b, :nout].sum(1), nd_n[alive != 0][:nout]), (path, fill, b)
                assert not hist[b, nout:].any(), (path, fill, b)
            tables.append(hist)
    assert all(np.array_equal(tables[0], t) for t in tables[1:])  # either padding label, either path
    assert (tables[0] > 0).sum(2).max() >= 2  # mixed voxels exist: the argmax check says something


# ---------------------------------------------------------------- 3: nll_hist forward and backward

LSM_C = (1, 2, 29, 31, 32)
LSM_BN = ((1, 1), (1, 63), (2, 33), (3, 1000))


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _table(B, N, C, seed, hi=9):
    """Counts in 0 .. hi - 1, about half of the cells and some whole rows empty."""
    g = _gen(seed)
    h = torch.randint(0, hi, (B, N, C), generator=g, dtype=torch.int32)
    h[torch.rand(B, N, C, generator=g) < 0.5] = 0
    if N > 4:
        h[0, 1:N:7] = 0  # rows without a point
    return h


def _loss_formula(logp_cm, hist, dtype):
    """-(sum of h logp over the non-zero counts) / W in `dtype`, W == 0 -> 0; returns (loss, d(3 loss)/dlogp)."""
    l_ = logp_cm.detach().to(dtype).clone().requires_grad_()
    h = hist.transpose(1, 2)  # [B][C][N] as logp
    terms = torch.where(h != 0, h.to(dtype) * l_, torch.zeros((), dtype=dtype, device=l_.device))
    W = int(hist.sum(dtype=torch.int64))
    loss = -terms.sum() / max(W, 1)
    (loss * 3.0).backward()
    return loss.detach().reshape(1), l_.grad


def _nll_case(name, logp, hist, bad):
    B, C, N = logp.shape
    nparts = (B * N + 63) // 64
    W = int(hist.sum(dtype=torch.int64))
    lb, hb, part, ws, loss, dl, dlogp = Buf.of(logp), Buf.of(hist), Buf(2 * nparts, torch.float64), \
        Buf(2, torch.int64), Buf(1), Buf.of(torch.tensor([3.0], device="cuda")), Buf(B * C * N)
    assert _lib().ndnet_tr_nll_hist(lb.ptr, hb.ptr, part.ptr, ws.ptr, loss.ptr, B, C, N, _st()) == 0
    assert _lib().ndnet_tr_nll_hist_bwd(hb.ptr, ws.ptr, dl.ptr, dlogp.ptr, B, C, N, _st()) == 0
    torch.cuda.synchronize()
    for nm, b in (("part", part), ("wsum", ws), ("loss", loss), ("dlogp", dlogp), ("hist", hb), ("logp", lb)):
        assert b.surround_ok(), f"{name}: words outside {nm} were written"
    assert part.written() and dlogp.written() and loss.written()
    assert ws.t.item() == W, (name, ws.t.item(), W)
    ref, gref = _loss_formula(logp, hist, torch.float64)
    t32, g32 = _loss_formula(logp, hist, torch.float32)
    assert bool(torch.isfinite(ref).all()) and bool(torch.isfinite(gref).all())
    _cmp(f"{name} loss", loss.t, ref, t32, bad)
    _cmp(f"{name} grad", dlogp.t.view(B, C, N), gref, g32, bad)
    return loss.t.clone(), dlogp.t.view(B, C, N).clone()


@pytest.mark.parametrize("C", LSM_C)
def test_nll_hist_fwd_bwd(C):
    """The loss and its gradient with dloss = 3, `part` sized exactly ceil(B N /
    64) doubles with the sentinel after it: tables with empty rows, a -inf
    log-prob under a zero count, W == 0, and W above 2^24."""
    bad = []
    for B, N in LSM_BN:
        logp = torch.log_softmax(torch.randn(B, C, N, generator=_gen(C + N)), 1).cuda()
        hist = _table(B, N, C, C * N).cuda()
        _nll_case(f"C{C} B{B} N{N}", logp, hist, bad)
        # a -inf log-prob under a zero count adds 0 to the loss and gets a zero gradient
        masked = logp.clone()
        zero = (hist == 0).transpose(1, 2)
        masked[zero] = float("-inf")
        loss, grad = _nll_case(f"C{C} B{B} N{N} -inf", masked, hist, bad)
        assert bool((grad[zero] == 0).all())
        # W == 0: loss 0 and an all-zero gradient, whatever the log-probs hold
        loss, grad = _nll_case(f"C{C} B{B} N{N} W0", masked, torch.zeros_like(hist), bad)
        assert loss.item() == 0.0 and bool((grad == 0).all())
    # W = 70 000 per cell: above 2^24 from 240 cells on, where an fp32 W is no longer exact
    B, N = LSM_BN[-1]
    logp = torch.log_softmax(torch.randn(B, C, N, generator=_gen(C)), 1).cuda()
    hist = torch.full((B, N, C), 70_000, dtype=torch.int32, device="cuda")
    hist[1, 5:N:3] = 0
    assert int(hist.sum(dtype=torch.int64)) > 2 ** 24
    _nll_case(f"C{C} B{B} N{N} 70000", logp, hist, bad)
    assert not bad, bad


# ---------------------------------------------------------------- 4: hist_match

def _first_argmax(pred):
    """The first maximum of the last axis, NaN counting as a maximum (torch.argmax), in numpy."""
    p = pred.numpy()
    nan = np.isnan(p)
    return np.where(nan.any(-1), nan.argmax(-1), np.where(nan, -np.inf, p).argmax(-1))


@pytest.mark.parametrize("C", LSM_C)
def test_hist_match_against_an_integer_reference(C):
    """ctr[0] the matched points, ctr[1] = W (both beyond 32 bits at the largest
    shape), ctr[2] == the grid size, acc == float(matched) / float(W) exactly,
    acc = NULL accepted; a planted NaN, an exact tie and an all-equal row."""
    for B, N in LSM_BN:
        g = _gen(C * 31 + N)
        pred = torch.randn(B, N, C, generator=g)  # [B][N][C]
        pts = B * N
        if pts >= 3 and C > 1:
            pred[0, 0, C // 2] = float("nan")
            pred[0, 1, C - 1] = pred[0, 1].max()  # an exact tie: the first index wins
            pred[-1, N - 1, :] = 0.25             # an all-equal row: class 0
        hist = torch.randint(0, 2 ** 31 - 1, (B, N, C), generator=g, dtype=torch.int32)
        hist[torch.rand(B, N, C, generator=g) < 0.3] = 0
        am = _first_argmax(pred)
        assert np.array_equal(am, pred.argmax(-1).numpy())
        h64 = hist.numpy().astype(np.int64)
        matched, W = int(np.take_along_axis(h64, am[..., None], -1).sum()), int(h64.sum())
        if pts >= 3000:
            assert W > 2 ** 32 and matched > 2 ** 32
        cm, hb = Buf.of(pred.transpose(1, 2).contiguous().cuda()), Buf.of(hist.cuda())
        for with_acc in (True, False):
            ctr, acc = Buf.of(torch.zeros(3, dtype=torch.int64, device="cuda")), Buf(1)
            rc = _lib().ndnet_tr_hist_match_cm(cm.ptr, hb.ptr, B, C, N, ctr.ptr, acc.ptr if with_acc else None, _st())
            assert rc == 0
            torch.cuda.synchronize()
            assert ctr.surround_ok() and acc.surround_ok() and hb.surround_ok() and cm.surround_ok()
            assert ctr.t.tolist() == [matched, W, (pts + 63) // 64], (C, B, N, ctr.t.tolist(), matched, W)
            if with_acc:
                want = (np.float32(matched) / np.float32(W)) if W else np.float32(0)
                assert acc.t.item() == float(want), (C, B, N)
            else:
                assert not acc.written()
    # W == 0: acc 0
    ctr, acc = Buf.of(torch.zeros(3, dtype=torch.int64, device="cuda")), Buf(1)
    zb = Buf.of(torch.zeros_like(hist).cuda())
    assert _lib().ndnet_tr_hist_match_cm(cm.ptr, zb.ptr, B, C, N, ctr.ptr, acc.ptr, _st()) == 0
    torch.cuda.synchronize()
    assert ctr.t.tolist()[:2] == [0, 0] and acc.t.item() == 0.0


# ---------------------------------------------------------------- 5: identity with the evaluation stack

@pytest.mark.parametrize("kind", ["U", "L"])
def test_point_loss_is_the_nll_of_what_segment_points_predicts(kind):
    from ndnet import segment, training
    from ndnet.preprocessing.ndtnet_preprocessing import ndt_preprocessing
    C, B = 28, len(COUNTS8)
    cols = C + 1
    pts = torch.from_numpy(_padded(kind, N4K, COUNTS8)).cuda()
    ndt_preprocessing(K, pts, counts=list(COUNTS8))
    rows = segment.point_rows(pts, "nearest")  # the last run's plan, block and counts
    rng = np.random.default_rng(9)
    labels_h = rng.integers(-2, cols + 2, (B, N4K)).astype(np.int32)  # out-of-range ids among them
    labels = torch.from_numpy(labels_h).cuda()
    logp_cm = torch.log_softmax(torch.randn(B, cols, K, generator=_gen(3)), 1).cuda()
    pred = logp_cm.transpose(1, 2)  # the model's output: a [B, k, C + 1] view of [B, C + 1, k]
    hist = segment.row_histogram(rows, labels, K, cols)
    assert training._hist_on_hip(pred, hist)
    loss = training.point_loss(pred, hist)
    t32 = training.point_loss_torch(pred, hist)
    # float64 mean of -logp[b, row, label] over the counted points
    rows_h, lp = rows.cpu().numpy(), pred.cpu().numpy().astype(np.float64)
    for b, c in enumerate(COUNTS8):
        assert (rows_h[b, :c] >= 0).all() and (rows_h[b, c:] == -1).all()
    ok = (rows_h >= 0) & (labels_h >= 0) & (labels_h < cols)
    b_idx = np.broadcast_to(np.arange(B)[:, None], rows_h.shape)
    nll = -lp[b_idx[ok], rows_h[ok], labels_h[ok]]
    assert nll.size == int(hist.sum()) > 0
    bad = []
    _cmp(f"{kind} point_loss", loss.reshape(1).cpu(), torch.tensor([nll.mean()]), t32.reshape(1).cpu(), bad)
    assert not bad, bad
    # the matched points are the trace of the point-level confusion matrix
    ctr = torch.zeros(3, dtype=torch.int64, device="cuda")
    assert _lib().ndnet_tr_hist_match_cm(logp_cm.data_ptr(), hist.data_ptr(), B, cols, K, ctr.data_ptr(), None,
                                         _st()) == 0
    conf = segment.confusion(segment.point_labels(pred.contiguous(), rows), labels, C)
    assert int(ctr[0]) == int(conf.diagonal().sum()) > 0
    assert int(ctr[1]) == int(conf.sum()) == nll.size
    acc = training.point_accuracy_tensor(pred, hist)
    assert acc.item() == float(np.float32(int(ctr[0])) / np.float32(int(ctr[1])))


# ---------------------------------------------------------------- 6, 7: the trainer

TB, TN, TK, TC = 2, 20_000, 500, 28
TCOUNTS = (20_000, 12_345)


def _model(seed):
    from ndnet.models.ndtnet import NDTNetSegmentation
    torch.manual_seed(seed)
    return NDTNetSegmentation(3, TC, 768)


@functools.lru_cache(maxsize=None)
def _batch(seed0, counts=TCOUNTS, pad=np.nan, pad_label=0):
    """(points [B, n, 3] float32, one-hot [B, n, C + 1] float32, ids [B, n] int64) on the CPU, padded past counts."""
    from ndnet.synthetic import make_labelled_batch
    pts, gt = make_labelled_batch(TB, TN, TC, seed0=seed0)
    pts, gt = pts.copy(), gt.copy()
    ids = gt.argmax(-1)
    for b, c in enumerate(counts):
        pts[b, c:] = pad
        ids[b, c:] = pad_label
        gt[b, c:] = 0.0
        if 0 <= pad_label <= TC:
            gt[b, c:, pad_label] = 1.0
    return torch.from_numpy(pts), torch.from_numpy(gt), torch.from_numpy(ids)


def _trainer(seed, **kw):
    from ndnet.training import Trainer
    dev = torch.device("cuda", 0)
    return Trainer(_model(seed), 1e-3, TK, TC, dev, ddp=False, **kw)


def _grads(tr):
    return [p.grad.detach().clone() for p in tr.model.parameters()]


@pytest.mark.parametrize("fill", ["nearest", "none"])
def test_trainer_point_loss_eager(fill, monkeypatch):
    from ndnet import training
    pts, gt, ids = _batch(31)
    counts = list(TCOUNTS)
    t_hip = _trainer(4, loss="points", point_fill=fill)
    l_hip, a_hip = t_hip.step(pts, ids, counts=counts)
    g_hip = _grads(t_hip)
    assert np.isfinite(l_hip) and 0.0 <= a_hip <= 1.0
    # the same step on the torch composition of the loss
    t_ref = _trainer(4, loss="points", point_fill=fill)
    with monkeypatch.context() as m:
        m.setattr(training, "point_loss", training.point_loss_torch)
        l_ref, a_ref = t_ref.step(pts, ids, counts=counts)
    g_ref = _grads(t_ref)
    print(f"TRAINER {fill}: loss hip {l_hip!r} torch {l_ref!r} acc {a_hip!r} {a_ref!r}")
    assert abs(l_hip - l_ref) <= 1e-5 * max(1.0, abs(l_ref)), (l_hip, l_ref)
    scale = max(g.abs().max().item() for g in g_ref)
    assert scale > 0
    for (name, _), a, b in zip(t_hip.model.named_parameters(), g_hip, g_ref):
        assert (a - b).abs().max().item() <= 1e-4 * scale, name
    # a one-hot gt gives the same bits as its integer ids: the step's inputs and what it returns
    t_oh = _trainer(4, loss="points", point_fill=fill)
    for a, b in zip(t_oh.nds_and_targets(pts, gt, counts), t_hip.nds_and_targets(pts, ids, counts)):
        assert torch.equal(a, b)
    assert t_oh.step(pts, gt, counts=counts) == (l_hip, a_hip)
    # garbage in the padding, points and labels, changes nothing
    pts2, _, ids2 = _batch(31, pad=1e30, pad_label=777)
    assert not torch.equal(ids2, ids)
    t_pad = _trainer(4, loss="points", point_fill=fill)
    for a, b in zip(t_pad.nds_and_targets(pts2, ids2.int(), counts), t_hip.nds_and_targets(pts, ids, counts)):
        assert torch.equal(a, b)
    assert t_pad.step(pts2, ids2.int(), counts=torch.tensor(counts)) == (l_hip, a_hip)
    # the eval step returns the same two figures from the eval forward, and updates nothing
    before = [p.detach().clone() for p in t_hip.model.parameters()]
    l_ev, a_ev = t_hip.step(pts, ids, train=False, counts=counts)
    assert np.isfinite(l_ev) and 0.0 <= a_ev <= 1.0
    assert all(torch.equal(a, b) for a, b in zip(before, t_hip.model.parameters()))


def test_trainer_nd_loss_takes_ids_and_counts():
    pts, gt, ids = _batch(31)
    counts = list(TCOUNTS)
    t_oh, t_id = _trainer(6), _trainer(6)
    assert t_oh.loss == "nds"
    r_oh = t_oh.step(pts, gt, counts=counts)
    r_id = t_id.step(pts, ids, counts=counts)
    assert r_oh == r_id and np.isfinite(r_oh[0])
    for a, b in zip(t_oh.nds_and_targets(pts, gt, counts)[:3], t_id.nds_and_targets(pts, ids, counts)[:3]):
        assert torch.equal(a, b)
    # counts matter: the whole clouds give another loss
    full, gt_full, _ = _batch(31, counts=(TN, TN))
    assert _trainer(6).step(full, gt_full) != r_oh


def test_trainer_point_loss_graphed():
    """Three replays of one captured step (labels -> labelled NDT -> rows ->
    histogram -> train forward -> point loss -> backward -> Adam) with different
    counts and labels, each against the eager step from the same weights."""
    from ndnet.training import point_loss
    dev = torch.device("cuda", 0)
    t_g = _trainer(9, graphs=True, loss="points", point_fill="nearest")
    t_e = _trainer(9, graphs=True, loss="points", point_fill="nearest")
    m_g, m_e = t_g.model, t_e.model
    cases = [(20, TCOUNTS), (21, (9_999, 20_000)), (22, (TN, TN))]
    for i, (seed0, counts) in enumerate(cases):
        pts, _, ids = _batch(seed0, counts=counts, pad_label=TC + 5 + i)
        pts, ids = pts.to(dev), ids.to(dev)
        d_counts = torch.tensor(counts, dtype=torch.int32, device=dev)
        with torch.no_grad():  # the eager side starts from the graph side's weights
            for a, b in zip(m_e.parameters(), m_g.parameters()):
                a.copy_(b)
            for a, b in zip(m_e.buffers(), m_g.buffers()):
                a.copy_(b)
        pcl, covs, _, hist = t_e.nds_and_targets(pts, ids, d_counts)
        m_e.train()
        t_e.opt.zero_grad(set_to_none=True)
        l_e = point_loss(m_e(pcl, covs), hist)
        l_e.backward()
        if i == 1:  # the graph's own input buffers, filled in place: replayed with no copy
            s_p, s_g, s_c = t_g.graph_inputs(pts.shape, ids.shape, counts=True)
            assert s_g.dtype == torch.int32 and s_c.dtype == torch.int32 and s_c.shape == (TB,)
            s_p.copy_(pts)
            s_g.copy_(ids)
            s_c.copy_(d_counts)
            l_g, a_g = t_g.step_graphed(s_p, s_g, s_c)
        else:
            l_g, a_g = t_g.step_graphed(pts, ids, list(counts) if i == 0 else d_counts)
        print(f"GRAPHED {i}: loss graph {l_g.item()!r} eager {l_e.item()!r} acc {a_g.item()!r}")
        assert abs(l_g.item() - l_e.item()) <= 1e-5 * max(1.0, abs(l_e.item())), (i, l_g.item(), l_e.item())
        assert 0.0 <= a_g.item() <= 1.0
        scale = max(q.grad.abs().max().item() for q in m_e.parameters())
        for (name, a), b in zip(m_g.named_parameters(), m_e.parameters()):
            assert (a.grad - b.grad).abs().max().item() <= 1e-4 * scale, (i, name)
    assert len(t_g._graphed) == 1
    # counts go with a ragged capture only, and the fixed-size key is as it was
    with pytest.raises(ValueError, match="counts"):
        t_g._graphed[next(iter(t_g._graphed))](pts, ids)
