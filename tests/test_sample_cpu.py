"""The random subsample, the parts that need no GPU: the definition's two forms
against each other, its uniformity, the keys' distinctness at full width, the
C ABI's argument checks (nothing is launched), the wrappers' own checks and the
BaselineTrainer's constructor."""
import ctypes

import numpy as np
import pytest
import torch

import sample_ref as R


@pytest.mark.parametrize("key_bits", [32, 4, 1])
@pytest.mark.parametrize("m,S", [(2500, 1), (2500, 7), (2500, 1024), (2500, 2499), (1500, 1024), (5, 1024)])
def test_threshold_form_equals_lexsort_form(key_bits, m, S):
    for step in (0, 3, (1 << 40) + 5):
        key = R.keys(9, 2, 1, m, step, key_bits)
        assert key.dtype == np.uint32 and key.shape == (m,) and int(key.max()) < 1 << key_bits
        a = R.choose(key, S)
        b, tau, below, ties = R.choose_threshold(key, S)
        assert np.array_equal(a, b)
        assert len(a) == min(m, S) and len(set(a.tolist())) == len(a)
        assert (np.diff(a) > 0).all() and a.min() >= 0 and a.max() < m
        if m > S:
            assert below < S <= below + ties
            assert (key[a] <= tau).all() and (np.delete(key, a) >= tau).all()


def test_inclusion_is_uniform():
    """Seed 7, stream 0, cloud 0, n = 64, S = 16, steps 0 .. 3999: every index is
    chosen 1000 times within 4.5 sigma, sigma = sqrt(4000 * 1/4 * 3/4) (the
    definition itself gives at most 2.37 sigma here)."""
    n, S, steps = 64, 16, 4000
    hits = np.zeros(n, np.int64)
    for step in range(steps):
        idx = R.choose(R.keys(7, 0, 0, n, step), S)
        assert len(idx) == S
        hits[idx] += 1
    sigma = np.sqrt(steps * 0.25 * 0.75)
    dev = np.abs(hits - steps * S / n) / sigma
    print(f"UNIFORM max deviation {dev.max():.2f} sigma")
    assert hits.sum() == steps * S and dev.max() <= 4.5


def test_no_key_collisions_at_full_width():
    assert len(np.unique(R.keys(0, 0, 0, 100_000, 0))) == 100_000
    # not a property of the definition: 100 000 draws from 2^32 values hold n^2 / 2^33 = 1.16 equal
    # pairs on average, and seed 4 has three -- there the index decides, as at any narrower key
    assert len(np.unique(R.keys(4, 0, 0, 100_000, 0))) == 99_997
    # the sampler's keys are not the augmentation's: purpose 3 against 0 .. 2 on the same counter
    from aug_ref import counter, philox
    mine = R.keys(0, 0, 0, 1000, 0)
    for purpose in (0, 1, 2):
        assert not np.array_equal(mine, philox(*counter(np.arange(1000), 0, 0, purpose), 0, 0)[0])


def test_oracle_filler_rows_and_gather():
    rng = np.random.default_rng(1)
    pts = rng.standard_normal((2, 40, 3)).astype(np.float32)
    lab = rng.integers(0, 9, (2, 40)).astype(np.int32)
    p, l_, c, i = R.sample(3, 0, pts, lab, [40, 5], 8, step=2, fill_label=-7)
    assert c.tolist() == [8, 5] and i[1].tolist() == [0, 1, 2, 3, 4, -1, -1, -1]
    assert np.array_equal(p[1, 5:], np.repeat(pts[1, :1], 3, 0)) and l_[1, 5:].tolist() == [-7] * 3
    assert np.array_equal(p[0], pts[0, i[0]]) and np.array_equal(l_[0], lab[0, i[0]])
    gp, gl, gc = R.gather(pts, lab, i, fill_label=-7)
    assert np.array_equal(gp, p) and np.array_equal(gl, l_) and np.array_equal(gc, c)


# ---------------------------------------------------------------- the C ABI's argument checks

E = -20
# addresses that are never dereferenced (every case is refused before any launch), far enough apart
PTS, LAB, CNT, STEP, WORK, OPTS, OLAB, OCNT, OIDX, IDX = (0x10_0000_0000 * (k + 1) for k in range(10))


def _cfg(key_bits=32):
    from ndnet import _lib
    c = _lib.SampleConfig()
    c.seed, c.stream, c.key_bits = 1, 0, key_bits
    return c


def _random_args(**kw):
    a = dict(cfg=ctypes.byref(_cfg()), pts=PTS, lab=LAB, cnt=CNT, B=2, n=100, S=10, fill=-1, adv=1, step=STEP,
             work=WORK, opts=OPTS, olab=OLAB, ocnt=OCNT, oidx=OIDX, st=None)
    a.update(kw)
    return tuple(a.values())


def test_random_run_argument_checks_launch_nothing():
    from ndnet import _lib
    f = _lib.lib().ndnet_sample_random_run
    assert _lib.NDNET_ERR_ARG == E
    for bad in ("cfg", "pts", "step", "work", "opts", "ocnt"):
        assert f(*_random_args(**{bad: None})) == E, bad
    assert f(*_random_args(lab=None)) == E    # labels out without labels in
    assert f(*_random_args(olab=None)) == E   # labels in without labels out
    for kw in (dict(B=0), dict(B=-1), dict(B=65536), dict(n=0), dict(n=1 << 31), dict(n=1 << 40, S=1 << 40),
               dict(S=0), dict(S=101)):
        assert f(*_random_args(**kw)) == E, kw
    for kb in (0, -1, 33):
        assert f(*_random_args(cfg=ctypes.byref(_cfg(kb)))) == E, kb
    # an output over an input or over another output (ranges, not just equal pointers)
    assert f(*_random_args(opts=PTS)) == E
    assert f(*_random_args(opts=PTS + 12 * 2 * 100 - 4)) == E
    assert f(*_random_args(opts=PTS - 12 * 2 * 10 + 4)) == E
    assert f(*_random_args(olab=LAB + 400)) == E
    assert f(*_random_args(oidx=LAB)) == E
    assert f(*_random_args(ocnt=CNT + 4)) == E
    assert f(*_random_args(oidx=OLAB + 4 * 2 * 10 - 4)) == E
    assert f(*_random_args(ocnt=STEP)) == E
    # the scratch, ndnet_sample_work_bytes(2, 100) bytes: no output, input or counter inside it
    nbytes = _lib.lib().ndnet_sample_work_bytes(2, 100)
    assert f(*_random_args(opts=WORK + nbytes - 4)) == E
    assert f(*_random_args(oidx=WORK - 4 * 2 * 10 + 4)) == E
    assert f(*_random_args(ocnt=WORK + 16)) == E
    assert f(*_random_args(work=PTS + 8)) == E
    assert f(*_random_args(work=STEP - nbytes + 8)) == E
    assert f(*_random_args(work=LAB - nbytes + 4)) == E
    assert _lib.lib().ndnet_sample_work_bytes(0, 10) == 0 and _lib.lib().ndnet_sample_work_bytes(1, 1 << 31) == 0
    # head 16; per cloud tau, quota, 256 bins and 2 words per tile, rounded up to 16 bytes; per cloud n keys
    # rounded up to 4; 4 bytes each
    assert _lib.lib().ndnet_sample_work_bytes(3, 2500) == 16 + 4 * (3 * (2 + 256 + 2 * 3) + 3 * 2500)
    assert _lib.lib().ndnet_sample_work_bytes(3, 2501) == 16 + 4 * (3 * (2 + 256 + 2 * 3) + 3 * 2504)
    assert _lib.lib().ndnet_sample_work_bytes(1, 5) == 16 + 4 * (260 + 8)


def _gather_args(**kw):
    a = dict(pts=PTS, lab=LAB, idx=IDX, B=2, n=100, S=10, fill=-1, opts=OPTS, olab=OLAB, ocnt=OCNT, st=None)
    a.update(kw)
    return tuple(a.values())


def test_gather_run_argument_checks_launch_nothing():
    from ndnet import _lib
    f = _lib.lib().ndnet_sample_gather_run
    for bad in ("pts", "idx", "opts", "ocnt"):
        assert f(*_gather_args(**{bad: None})) == E, bad
    assert f(*_gather_args(lab=None)) == E and f(*_gather_args(olab=None)) == E
    for kw in (dict(B=0), dict(B=65536), dict(n=0), dict(n=1 << 31), dict(S=0), dict(S=1 << 31)):
        assert f(*_gather_args(**kw)) == E, kw
    assert f(*_gather_args(opts=PTS + 12)) == E
    assert f(*_gather_args(olab=IDX)) == E
    assert f(*_gather_args(ocnt=OLAB)) == E


# ---------------------------------------------------------------- the wrappers' checks

def test_random_sample_checks_come_before_the_gpu():
    from ndnet.preprocessing import RandomSample, random_sample  # noqa: F401
    pts = torch.zeros((2, 16, 3))
    lab = torch.zeros((2, 16), dtype=torch.int64)
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match="n_samples"):
            RandomSample(bad)
    with pytest.raises(ValueError, match="seed"):
        RandomSample(4, seed=-1)
    with pytest.raises(ValueError, match="stream"):
        RandomSample(4, stream=1 << 32)
    with pytest.raises(ValueError, match="key_bits"):
        RandomSample(4, key_bits=0)
    s = RandomSample(4, seed=5)
    with pytest.raises(ValueError, match="float32"):
        s(pts.double())
    with pytest.raises(ValueError, match=r"\[B, n, 3\]"):
        s(pts[0])
    with pytest.raises(ValueError, match=r"\[B, n, 3\]"):
        s(torch.zeros((2, 16, 4)))
    with pytest.raises(ValueError, match="n_samples"):
        RandomSample(17)(pts)
    with pytest.raises(ValueError, match="labels"):
        s(pts, lab.float())
    with pytest.raises(ValueError, match="labels"):
        s(pts, lab[:, :8])
    with pytest.raises(ValueError, match="out_labels"):
        s(pts, out_labels=torch.zeros((2, 4), dtype=torch.int32))
    with pytest.raises(ValueError, match="counts"):
        s(pts, counts=[16])
    with pytest.raises(ValueError, match="count"):
        s(pts, counts=[16, 0])
    with pytest.raises(ValueError, match="count"):
        s(pts, counts=torch.tensor([17, 3]))
    with pytest.raises(ValueError, match="out_points"):
        s(pts, out_points=torch.zeros((2, 5, 3)))
    with pytest.raises(ValueError, match="out_indices"):
        s(pts, out_indices=torch.zeros((2, 4), dtype=torch.int64))
    with pytest.raises(ValueError, match="step"):
        s(pts, step=torch.zeros(1, dtype=torch.int32))
    with pytest.raises(ValueError, match="step"):
        s.step = 1 << 62
    # the state travels without a device
    s.step = 41
    t = RandomSample(9)
    t.load_state_dict(s.state_dict())
    assert (t.n_samples, t.seed, t.stream, t.key_bits, t.step) == (4, 5, None, 32, 41)
    assert s.resolve_stream() == 0 and s.config().key_bits == 32
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):  # valid arguments, no GPU: no CPU fallback
            s(pts, lab, counts=[16, 3])


def test_gather_samples_checks_come_before_the_gpu():
    from ndnet.preprocessing import gather_samples
    pts = torch.zeros((2, 16, 3))
    idx = torch.zeros((2, 4), dtype=torch.int32)
    with pytest.raises(ValueError, match="float32"):
        gather_samples(pts.half(), idx)
    with pytest.raises(ValueError, match="indices"):
        gather_samples(pts, idx.long())
    with pytest.raises(ValueError, match="indices"):
        gather_samples(pts, idx[:1])
    with pytest.raises(ValueError, match="indices"):
        gather_samples(pts, idx[0])
    with pytest.raises(ValueError, match="labels"):
        gather_samples(pts, idx, torch.zeros((2, 16)))
    with pytest.raises(ValueError, match="out_labels"):
        gather_samples(pts, idx, out_labels=torch.zeros((2, 4), dtype=torch.int32))
    with pytest.raises(ValueError, match="out_counts"):
        gather_samples(pts, idx, out_counts=torch.zeros((3,), dtype=torch.int32))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):
            gather_samples(pts, idx)


def test_baseline_trainer_refuses_unknown_modes_before_the_gpu():
    from ndnet.models.pointnet import PointNetSegmentation
    from ndnet.training import BaselineTrainer
    model = PointNetSegmentation(3, 4, 64)
    cpu = torch.device("cpu")
    with pytest.raises(ValueError, match="sampler"):
        BaselineTrainer(model, 1e-3, 64, 4, cpu, sampler="grid")
    with pytest.raises(ValueError, match="loss"):
        BaselineTrainer(model, 1e-3, 64, 4, cpu, loss="nds")
    with pytest.raises(ValueError, match="augment"):
        BaselineTrainer(model, 1e-3, 64, 4, cpu, augment=object())
    with pytest.raises(ValueError, match="n_samples"):
        BaselineTrainer(model, 1e-3, 0, 4, cpu)
    with pytest.raises(ValueError, match="graphs"):
        BaselineTrainer(model, 1e-3, 64, 4, cpu, graphs=True)
    tr = BaselineTrainer(model, 1e-3, 64, 4, cpu, ddp=False, seed=3)
    assert (tr.sampler, tr.loss, tr.random_sample.seed, tr.random_sample.n_samples) == ("random", "samples", 3, 64)
    tr.set_epoch(19)
    assert tr.opt.param_groups[0]["lr"] == 0.5e-3

