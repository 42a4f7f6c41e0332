"""The random subsample on the GPU (ndnet_sample_random_run, ndnet_sample_gather_run)
against the numpy oracle of tests/sample_ref.py: exact equality of indices,
points, labels and counts.  Every output lies between two pads of sentinel
words that must stay untouched."""
import numpy as np
import pytest
import torch

import sample_ref as R

pytestmark = pytest.mark.gpu

SENT = 0x7FC0BEEF
PAD = 256


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


class Out:
    """The four output buffers of a call, each between two pads of sentinel words."""

    def __init__(self, B, S, labels=True):
        self.raw = {}
        self.points = self._make("points", (B, S, 3), torch.float32)
        self.labels = self._make("labels", (B, S), torch.int32) if labels else None
        self.counts = self._make("counts", (B,), torch.int32)
        self.indices = self._make("indices", (B, S), torch.int32)

    def _make(self, name, shape, dtype):
        n = int(np.prod(shape))
        raw = self.raw[name] = torch.full((PAD + n + PAD,), SENT, dtype=torch.int32, device="cuda")
        return raw[PAD:PAD + n].view(dtype).view(shape)

    def kw(self):
        return dict(out_points=self.points, out_labels=self.labels, out_counts=self.counts, out_indices=self.indices)

    def pads_ok(self):
        return all(bool((r[:PAD] == SENT).all()) and bool((r[-PAD:] == SENT).all()) for r in self.raw.values())


def _batch(B, n, seed, counts=None, pad=np.nan, pad_label=0):
    rng = np.random.default_rng(seed)
    pts = rng.standard_normal((B, n, 3)).astype(np.float32) * 10
    lab = rng.integers(0, 20, (B, n)).astype(np.int32)
    if counts is not None:
        for b, c in enumerate(counts):
            pts[b, c:] = pad
            lab[b, c:] = pad_label
    return pts, lab


def _run(sampler, pts, lab, counts, fill=-1, **kw):
    """One call into sentinel-guarded buffers -> numpy (points, labels, counts, indices)."""
    B, n, _ = pts.shape
    out = Out(B, sampler.n_samples, lab is not None)
    d_lab = torch.from_numpy(lab).cuda() if lab is not None else None
    res = sampler(torch.from_numpy(pts).cuda(), d_lab, counts, fill_label=fill, **out.kw(), **kw)
    torch.cuda.synchronize()
    assert out.pads_ok(), "words outside an output were written"
    assert res[0] is out.points and res[2] is out.counts and res[3] is out.indices
    return tuple(None if t is None else t.cpu().numpy() for t in res)


def _same(got, want, what=""):
    for name, g, w in zip(("points", "labels", "counts", "indices"), got, want):
        if w is None:
            assert g is None, (what, name)
        else:
            assert g.dtype == w.dtype and np.array_equal(g.view(np.int32), w.view(np.int32)), (what, name)


# ---------------------------------------------------------------- the small ragged batch

N, COUNTS = 2500, (2500, 1, 1500)  # three tiles, the last partial; one point; two tiles


@pytest.mark.parametrize("key_bits", [32, 12, 4, 1])
@pytest.mark.parametrize("S", [1, 7, 1024, 2499, 2500])
def test_small_ragged_batch_equals_the_oracle(S, key_bits):
    from ndnet.preprocessing import RandomSample
    pts, lab = _batch(3, N, 5, COUNTS)
    junk_p, junk_l = _batch(3, N, 5, COUNTS, pad=1e30, pad_label=777)
    s = RandomSample(S, seed=11, stream=2, key_bits=key_bits)
    for step, fill in ((0, -1), (6, 31)):
        want = R.sample(11, 2, pts, lab, COUNTS, S, step, key_bits, fill)
        assert want[2].tolist() == [min(c, S) for c in COUNTS]
        if S > 1:  # cloud 1 (and cloud 2 at S = 2499, 2500) has filler rows
            assert want[3][1, 1:].tolist() == [-1] * (S - 1) and (want[1][1, 1:] == fill).all()
        for p, l_, counts in ((pts, lab, list(COUNTS)), (junk_p, junk_l, torch.tensor(COUNTS)),
                              (pts, None, torch.tensor(COUNTS, dtype=torch.int32, device="cuda"))):
            s.step = step
            got = _run(s, p, l_, counts, fill)
            _same(got, want if l_ is not None else (want[0], None, want[2], want[3]), (S, key_bits, step))
        assert s.step == step + 1
    # without counts: every cloud whole
    full_p, full_l = _batch(3, N, 6)
    s.step = 3
    _same(_run(s, full_p, full_l, None), R.sample(11, 2, full_p, full_l, None, S, 3, key_bits), "whole")


@pytest.mark.parametrize("key_bits", [1, 4])
def test_tie_quota_splits_a_tie_class_across_tiles(key_bits):
    """S = 1024 of 2500 at 1 and at 4 key bits: the threshold's tie class is cut,
    #{key < tau} < S < #{key <= tau}, and its members lie in more than one tile."""
    from ndnet.preprocessing import RandomSample
    S, step = 1024, None
    for cand in range(64):
        key = R.keys(3, 0, 0, N, cand, key_bits)
        _, tau, below, ties = R.choose_threshold(key, S)
        tiles = np.unique(np.nonzero(key == tau)[0] // R.TILE)
        taken = np.nonzero(key == tau)[0][:S - below]
        if below < S < below + ties and len(tiles) > 1 and len(np.unique(taken // R.TILE)) > 1 \
                and (key_bits == 1 or below > 0):
            step = cand
            break
    assert step is not None
    pts, lab = _batch(1, N, 8)
    s = RandomSample(S, seed=3, stream=0, key_bits=key_bits)
    s.step = step
    _same(_run(s, pts, lab, None), R.sample(3, 0, pts, lab, None, S, step, key_bits), (key_bits, step))


@pytest.mark.parametrize("n,S", [(1, 1), (1024, 1024), (1025, 1024), (1025, 1), (1025, 1025)])
def test_edges(n, S):
    from ndnet.preprocessing import RandomSample
    pts, lab = _batch(2, n, n + S)
    s = RandomSample(S, seed=1, stream=0)
    _same(_run(s, pts, lab, None), R.sample(1, 0, pts, lab, None, S, 0), (n, S))
    counts = [n, max(1, n // 2)]
    _same(_run(s, pts, lab, counts), R.sample(1, 0, pts, lab, counts, S, 1), (n, S, "ragged"))


def test_production_shape():
    from ndnet.preprocessing import RandomSample
    B, n, S = 2, 70_000, 4160
    counts = [70_000, 51_234]
    pts, lab = _batch(B, n, 2, counts)
    s = RandomSample(S, seed=2024)
    s.step = (1 << 35) + 7  # both words of the step reach the counter
    _same(_run(s, pts, lab, counts), R.sample(2024, 0, pts, lab, counts, S, (1 << 35) + 7), "production")


def test_a_threshold_bin_too_large_for_lds_is_read_again():
    """320 000 points at 32 bits: the bin of the keys' top 8 bits that holds the
    threshold has more than NDNET_SAMPLE_LIST keys, so every further pass reads
    the cloud's keys again instead of the list in LDS."""
    from ndnet.preprocessing import RandomSample
    n, S = 320_000, 4096
    key = R.keys(5, 0, 0, n, 0)
    tau = np.sort(key)[S - 1]
    assert int((key >> 24 == tau >> 24).sum()) > R.LIST
    pts, lab = _batch(1, n, 4)
    _same(_run(RandomSample(S, seed=5, stream=0), pts, lab, None), R.sample(5, 0, pts, lab, None, S, 0), "rescan")


# ---------------------------------------------------------------- the counter

def test_counter_streams_and_state():
    from ndnet.preprocessing import RandomSample, random_sample
    pts, lab = _batch(2, 3000, 9)
    d_pts, d_lab = torch.from_numpy(pts).cuda(), torch.from_numpy(lab).cuda()
    S = 300
    want = [R.sample(4, 0, pts, lab, None, S, k) for k in range(3)]
    s = RandomSample(S, seed=4)
    assert s.step == 0
    _same(_run(s, pts, lab, None), want[0], "step 0")
    _same(_run(s, pts, lab, None), want[1], "step 1")
    assert s.step == 2
    # advance=False leaves the counter and repeats the draw
    _same(_run(s, pts, lab, None, advance=False), want[2], "no advance")
    assert s.step == 2
    _same(_run(s, pts, lab, None), want[2], "the same draw")
    assert s.step == 3
    # a counter of the caller's: the sampler's own stays
    mine = torch.tensor([1], dtype=torch.int64, device="cuda")
    _same(_run(s, pts, lab, None, step=mine, advance=False), want[1], "step=")
    assert mine.item() == 1 and s.step == 3
    _same(_run(s, pts, lab, None, step=mine), want[1], "step= advancing")
    assert mine.item() == 2 and s.step == 3
    # another stream, another draw; the default stream is 0 outside torch.distributed
    other = RandomSample(S, seed=4, stream=1)
    got = _run(other, pts, lab, None)
    _same(got, R.sample(4, 1, pts, lab, None, S, 0), "stream 1")
    assert not np.array_equal(got[3], want[0][3])
    # the state round trip repeats the next draw
    s.step = 1
    t = RandomSample(7)
    t.load_state_dict(s.state_dict())
    _same(_run(t, pts, lab, None), want[1], "resumed")
    # the one-shot form
    res = random_sample(d_pts, S, d_lab, seed=4, step=2)
    _same(tuple(r.cpu().numpy() for r in res), want[2], "random_sample")
    # independent of an augmentation with the same seed: its keep draw (purpose 2) is not the key
    import aug_ref
    assert not np.array_equal(aug_ref.point_words(aug_ref.Config(seed=4), 0, 3000, 0)[6], R.keys(4, 0, 0, 3000, 0))


def test_captured_call_draws_anew_at_every_replay():
    """Captured once, replayed three times: steps k, k + 1, k + 2, with other
    counts before every replay -- scratch left by one replay must not reach the
    next (the histograms are cleared by the call itself)."""
    from ndnet.preprocessing import RandomSample
    B, n, S, k = 2, 5000, 640, 10
    pts, lab = _batch(B, n, 12)
    d_pts, d_lab = torch.from_numpy(pts).cuda(), torch.from_numpy(lab).cuda()
    d_counts = torch.tensor([n, n], dtype=torch.int32, device="cuda")
    s = RandomSample(S, seed=6)
    out = Out(B, S)
    s(d_pts, d_lab, d_counts, **out.kw())  # (the work buffer and the counter exist before the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        s(d_pts, d_lab, d_counts, **out.kw())
    s.step = k
    for r, counts in enumerate(([n, 3000], [700, n], [n, 300])):
        d_counts.copy_(torch.tensor(counts, dtype=torch.int32))
        for t in (out.points, out.labels, out.counts, out.indices):
            t.view(torch.int32).fill_(-12345)
        g.replay()
        torch.cuda.synchronize()
        got = tuple(t.cpu().numpy() for t in (out.points, out.labels, out.counts, out.indices))
        _same(got, R.sample(6, 0, pts, lab, counts, S, k + r), ("replay", r))
        assert out.pads_ok()
    assert s.step == k + 3


def test_one_scratch_grows_to_the_largest_batch_and_a_captured_one_stays():
    """Ragged batches padded to another length on every call share one work
    buffer, sized for the largest seen; the buffer a captured call reads stays
    alive when a larger batch replaces it, and the replay is still the oracle's."""
    from ndnet.preprocessing import RandomSample
    S = 200
    s = RandomSample(S, seed=8)
    sizes = []
    for step, n in enumerate((3000, 2100, 2999, 1024)):
        pts, lab = _batch(2, n, 20 + n)
        _same(_run(s, pts, lab, None), R.sample(8, 0, pts, lab, None, S, step), n)
        sizes.append(next(iter(s._work.values())).numel())
        assert len(s._work) == 1
    assert sizes == [sizes[0]] * 4 and not s._captured
    pts, lab = _batch(2, 3000, 30)
    d_pts, d_lab = torch.from_numpy(pts).cuda(), torch.from_numpy(lab).cuda()
    out = Out(2, S)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        s(d_pts, d_lab, **out.kw())
    assert len(s._captured) == 1 and s._captured[0].numel() == sizes[0]
    big_p, big_l = _batch(2, 9000, 31)
    s.step = 50
    _same(_run(s, big_p, big_l, None), R.sample(8, 0, big_p, big_l, None, S, 50), "larger")
    assert len(s._work) == 1 and next(iter(s._work.values())).numel() > sizes[0] and len(s._captured) == 1
    junk = [torch.full((sizes[0],), -1, dtype=torch.int64, device="cuda") for _ in range(8)]  # (would land on a freed buffer)
    s.step = 60
    g.replay()
    torch.cuda.synchronize()
    got = tuple(t.cpu().numpy() for t in (out.points, out.labels, out.counts, out.indices))
    _same(got, R.sample(8, 0, pts, lab, None, S, 60), "replay after growth")
    assert out.pads_ok() and all(bool((j == -1).all()) for j in junk)


# ---------------------------------------------------------------- gather_samples

def test_gather_samples_against_the_oracle_and_the_torch_gather():
    from ndnet.preprocessing import farthest_point_sample, gather_samples
    B, n, S = 2, 3000, 600
    counts = [3000, 250]  # cloud 1 is short: its FPS indices end in -1
    pts, lab = _batch(B, n, 14, counts)
    d_pts, d_lab = torch.from_numpy(pts).cuda(), torch.from_numpy(lab).cuda()
    idx = farthest_point_sample(d_pts, S, counts=counts)
    idx_h = idx.cpu().numpy()
    assert (idx_h[1, 250:] == -1).all() and (idx_h[1, :250] >= 0).all()
    for fill in (-1, 42):
        p, l_, c = gather_samples(d_pts, idx, d_lab, fill_label=fill)
        wp, wl, wc = R.gather(pts, lab, idx_h, fill)
        assert np.array_equal(p.cpu().numpy().view(np.int32), wp.view(np.int32))
        assert np.array_equal(l_.cpu().numpy(), wl) and c.tolist() == wc.tolist() == [600, 250]
    # segment_points_fps's composition: the int64 expansion, the clamp and torch.gather
    gi = idx.unsqueeze(2).expand(B, S, 3).long().clamp_(min=0)
    assert torch.equal(p, torch.gather(d_pts, 1, gi))
    valid = idx >= 0
    assert torch.equal(l_[valid], torch.gather(d_lab, 1, idx.long().clamp(min=0))[valid])
    # without labels, into given buffers
    out = Out(B, S, labels=False)
    p2, l2, c2 = gather_samples(d_pts, idx, out_points=out.points, out_counts=out.counts)
    torch.cuda.synchronize()
    assert l2 is None and p2 is out.points and torch.equal(p2, p) and torch.equal(c2, c) and out.pads_ok()
    # hand-made indices: out of range on either side, the extremes, a repeated index
    hand = np.array([[0, n - 1, n, -1, 5, 5, 2 ** 31 - 1, -2 ** 31, n + 7]] * B, np.int32)
    hand[1, 0] = 299
    out = Out(B, hand.shape[1])
    p, l_, c = gather_samples(d_pts, torch.from_numpy(hand).cuda(), d_lab, fill_label=-9, out_points=out.points,
                              out_labels=out.labels, out_counts=out.counts)
    torch.cuda.synchronize()
    wp, wl, wc = R.gather(pts, lab, hand, -9)
    assert out.pads_ok() and c.tolist() == wc.tolist() == [4, 4]
    assert np.array_equal(p.cpu().numpy().view(np.int32), wp.view(np.int32)) and np.array_equal(l_.cpu().numpy(), wl)
