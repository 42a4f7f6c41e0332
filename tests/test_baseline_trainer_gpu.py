"""``ndnet.training.BaselineTrainer`` on the GPU: the eager step against the torch
composition on the oracles' samples, the ignore label, the eval step, the
captured step against the eager one, the augmentation's counts reaching the
sampler, and a learning check.

The model widths, B, n and the class count are those of ``_trainer`` /
``_batch`` in tests/test_point_loss_gpu.py, with S = 512 samples; so are the
tolerances: the loss within 1e-5 max(1, |ref|), every gradient within 1e-4 of
the largest reference gradient."""
import functools

import numpy as np
import pytest
import torch

import sample_ref as R
from fps_ref import fps_ref
from nearest_ref import nearest_ref

pytestmark = pytest.mark.gpu

TB, TN, TC, TS = 2, 20_000, 28, 512
TCOUNTS = (20_000, 12_345)
SEED = 5  # the trainer's sampler seed


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _model(seed):
    from ndnet.models.pointnet import PointNetSegmentation
    torch.manual_seed(seed)
    return PointNetSegmentation(3, TC, 768)


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
    from ndnet.training import BaselineTrainer
    return BaselineTrainer(_model(seed), 1e-3, TS, TC, torch.device("cuda", 0), ddp=False, seed=SEED, **kw)


def _grads(model):
    return [p.grad.detach().clone() for p in model.parameters()]


@functools.lru_cache(maxsize=None)
def _fps_indices(seed0, counts):
    pts = _batch(seed0, counts)[0].numpy()
    return np.stack([fps_ref(pts[b], TS, counts[b])[0] for b in range(TB)])


def _ref_front(pts, ids, counts, sampler, loss, step, ignore=-1, fps_idx=None):
    """The oracles' samples and the np.add.at histogram: (samples [B, S, 3], hist [B, S, C + 1] int32, sample counts)."""
    pts, ids = np.asarray(pts, np.float32), np.asarray(ids).astype(np.int32)
    if sampler == "random":
        smp, slab, scnt, _ = R.sample(SEED, 0, pts, ids, counts, TS, step)
    else:
        smp, slab, scnt = R.gather(pts, ids, fps_idx)
    hist = np.zeros((TB, TS, TC + 1), np.int32)
    for b in range(TB):
        if loss == "samples":
            rows, labels = np.arange(TS), slab[b]
        else:
            rows, labels = nearest_ref(pts[b], smp[b], counts[b], int(scnt[b]))[0], ids[b]
        ok = (rows >= 0) & (labels >= 0) & (labels <= TC) & (labels != ignore)
        np.add.at(hist[b], (rows[ok], labels[ok]), 1)
    return smp, hist, scnt


def _ref_step(seed, smp, hist):
    """forward_torch in train mode on the samples, point_loss_torch, backward: (loss, gradients)."""
    from ndnet.training import point_loss_torch
    m = _model(seed).cuda().train()
    loss = point_loss_torch(m.forward_torch(torch.from_numpy(smp).cuda()), torch.from_numpy(hist).cuda())
    loss.backward()
    return loss.item(), _grads(m)


def _close(tag, l_hip, g_hip, l_ref, g_ref, names):
    print(f"{tag}: loss hip {l_hip!r} ref {l_ref!r}")
    assert abs(l_hip - l_ref) <= 1e-5 * max(1.0, abs(l_ref)), (tag, l_hip, l_ref)
    scale = max(g.abs().max().item() for g in g_ref)
    assert scale > 0
    for name, a, b in zip(names, g_hip, g_ref):
        assert (a - b).abs().max().item() <= 1e-4 * scale, (tag, name)


@pytest.mark.parametrize("sampler", ["random", "fps"])
@pytest.mark.parametrize("loss", ["samples", "points"])
def test_eager_step_against_the_torch_composition(loss, sampler):
    pts, gt, ids = _batch(31)
    counts = list(TCOUNTS)
    fps_idx = _fps_indices(31, TCOUNTS) if sampler == "fps" else None
    t_hip = _trainer(4, sampler=sampler, loss=loss)
    names = [n for n, _ in t_hip.model.named_parameters()]
    l_hip, a_hip = t_hip.step(pts, ids, counts=counts)
    g_hip = _grads(t_hip.model)
    assert np.isfinite(l_hip) and 0.0 <= a_hip <= 1.0
    smp, hist, scnt = _ref_front(pts.numpy(), ids.numpy(), counts, sampler, loss, 0, fps_idx=fps_idx)
    assert int(hist.sum()) == (2 * TS if loss == "samples" else sum(TCOUNTS))
    l_ref, g_ref = _ref_step(4, smp, hist)
    _close(f"EAGER {loss} {sampler}", l_hip, g_hip, l_ref, g_ref, names)
    # the front is the oracles', bit for bit; and the second draw is step 1
    got = t_hip.samples_and_targets(pts, ids, counts)
    smp1, hist1, scnt1 = _ref_front(pts.numpy(), ids.numpy(), counts, sampler, loss, 1, fps_idx=fps_idx)
    assert np.array_equal(got[0].cpu().numpy(), smp1) and np.array_equal(got[1].cpu().numpy(), hist1)
    assert got[2].tolist() == scnt1.tolist() == [TS, TS]
    assert t_hip.random_sample.step == (2 if sampler == "random" else 0)
    # a one-hot gt gives the same bits as its integer ids
    t_oh = _trainer(4, sampler=sampler, loss=loss)
    assert t_oh.step(pts, gt, counts=counts) == (l_hip, a_hip)
    # garbage in the padding, points and labels, changes nothing
    pts2, _, ids2 = _batch(31, pad=1e30, pad_label=777)
    assert not torch.equal(ids2, ids)
    t_pad = _trainer(4, sampler=sampler, loss=loss)
    assert t_pad.step(pts2, ids2.int(), counts=torch.tensor(counts)) == (l_hip, a_hip)


@pytest.mark.parametrize("sampler", ["random", "fps"])
@pytest.mark.parametrize("loss", ["samples", "points"])
def test_ignore_label_carries_no_weight(loss, sampler):
    pts, _, ids = _batch(32)
    counts = list(TCOUNTS)
    fps_idx = _fps_indices(32, TCOUNTS) if sampler == "fps" else None
    ignore = int(torch.bincount(ids[0, :TCOUNTS[0]]).argmax())  # a class the batch does hold
    t_hip = _trainer(7, sampler=sampler, loss=loss, ignore_label=ignore)
    l_hip, _ = t_hip.step(pts, ids, counts=counts)
    smp, hist, _ = _ref_front(pts.numpy(), ids.numpy(), counts, sampler, loss, 0, ignore=ignore, fps_idx=fps_idx)
    _, full, _ = _ref_front(pts.numpy(), ids.numpy(), counts, sampler, loss, 0, fps_idx=fps_idx)
    assert not hist[:, :, ignore].any() and full[:, :, ignore].any()
    assert np.array_equal(np.delete(hist, ignore, 2), np.delete(full, ignore, 2))
    l_ref, g_ref = _ref_step(7, smp, hist)
    _close(f"IGNORE {loss} {sampler}", l_hip, _grads(t_hip.model), l_ref, g_ref, [n for n, _ in t_hip.model.named_parameters()])
    # and it is not the loss of the whole batch
    assert abs(_ref_step(7, smp, full)[0] - l_ref) > 1e-3


@pytest.mark.parametrize("sampler", ["random", "fps"])
def test_eval_step_is_deterministic_and_updates_nothing(sampler):
    from ndnet import segment
    pts, _, ids = _batch(33)
    counts = list(TCOUNTS)
    tr = _trainer(8, sampler=sampler, loss="points")
    tr.step(pts, ids, counts=counts)  # one training step first: the counter stands at 1
    state = [t.detach().clone() for t in list(tr.model.parameters()) + list(tr.model.buffers())]
    first = tr.step(pts, ids, train=False, counts=counts)
    second = tr.step(pts, ids, train=False, counts=counts)
    assert first == second and np.isfinite(first[0]) and 0.0 <= first[1] <= 1.0
    assert all(torch.equal(a, b) for a, b in zip(state, list(tr.model.parameters()) + list(tr.model.buffers())))
    assert tr.random_sample.step == (1 if sampler == "random" else 0)
    if sampler == "random":
        assert tr._eval_step.item() == 1 << 61
    # the mean NLL of every labelled point under its nearest sample's eval-mode prediction
    d_pts = pts.cuda()
    if sampler == "random":
        smp = R.sample(SEED, 0, pts.numpy(), None, counts, TS, 1 << 61)[0]
        with torch.no_grad():
            logp = tr.model.eval()(torch.from_numpy(smp).cuda())
        rows = np.stack([nearest_ref(pts.numpy()[b], smp[b], counts[b])[0] for b in range(TB)])
    else:
        buf = segment.FpsSegmentBuffers(TB, TN, TS, d_pts.device)
        _, logp = segment.segment_points_fps(tr.model.eval(), TS, d_pts, counts=counts, buffers=buf)
        rows = buf.rows.cpu().numpy()
    lp, ids_h = logp.cpu().numpy().astype(np.float64), ids.numpy()
    ok = rows >= 0
    b_idx = np.broadcast_to(np.arange(TB)[:, None], rows.shape)
    nll = -lp[b_idx[ok], rows[ok], ids_h[ok]]
    assert nll.size == sum(TCOUNTS)
    print(f"EVAL {sampler}: loss {first[0]!r} mean nll {nll.mean()!r}")
    assert abs(first[0] - nll.mean()) <= 1e-5 * max(1.0, abs(nll.mean()))
    acc = (lp.argmax(-1)[b_idx[ok], rows[ok]] == ids_h[ok]).mean()
    assert abs(first[1] - acc) <= 1e-6


@pytest.mark.parametrize("sampler", ["random", "fps"])
@pytest.mark.parametrize("loss", ["samples", "points"])
def test_graphed_step_against_the_eager_step(loss, sampler):
    """Three replays of one captured step with different counts and labels, each
    against the eager step from the same weights and the same sampler step;
    replay i is draw i."""
    from ndnet.training import point_loss
    dev = torch.device("cuda", 0)
    t_g = _trainer(9, graphs=True, sampler=sampler, loss=loss)
    t_e = _trainer(9, graphs=True, sampler=sampler, loss=loss)
    m_g, m_e = t_g.model, t_e.model
    cases = [(20, TCOUNTS), (21, (9_999, 20_000)), (22, (TN, 300))]  # 300 < S: filler rows in the last
    for i, (seed0, counts) in enumerate(cases):
        pts, _, ids = _batch(seed0, counts=counts, pad_label=TC + 5 + i)
        pts, ids = pts.to(dev), ids.to(dev)
        d_counts = torch.tensor(counts, dtype=torch.int32, device=dev)
        with torch.no_grad():  # the eager side starts from the graph side's weights
            for a, b in zip(m_e.parameters(), m_g.parameters()):
                a.copy_(b)
            for a, b in zip(m_e.buffers(), m_g.buffers()):
                a.copy_(b)
        t_e.random_sample.step = i
        smp, hist, scnt = t_e.samples_and_targets(pts, ids, d_counts)
        m_e.train()
        t_e.opt.zero_grad(set_to_none=True)
        l_e = point_loss(m_e(smp), hist)
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
        g = t_g._graph_for(pts.shape, ids.shape, True)
        assert torch.equal(g.buffers.samples, smp) and torch.equal(g.buffers.hist, hist)
        assert g.buffers.sample_counts.tolist() == scnt.tolist() == [min(c, TS) for c in counts]
        print(f"GRAPHED {loss} {sampler} {i}: loss graph {l_g.item()!r} eager {l_e.item()!r} acc {a_g.item()!r}")
        assert abs(l_g.item() - l_e.item()) <= 1e-5 * max(1.0, abs(l_e.item())), (i, l_g.item(), l_e.item())
        assert 0.0 <= a_g.item() <= 1.0
        scale = max(q.grad.abs().max().item() for q in m_e.parameters())
        for (name, a), b in zip(m_g.named_parameters(), m_e.parameters()):
            assert (a.grad - b.grad).abs().max().item() <= 1e-4 * scale, (i, name)
        assert t_g.random_sample.step == (i + 1 if sampler == "random" else 0)
    assert len(t_g._graphed) == 1  # one graph serves all counts
    with pytest.raises(ValueError, match="counts"):
        t_g._graphed[next(iter(t_g._graphed))](pts, ids)
    # a trainer captures one step: another batch shape, label form or no counts is refused, nothing captured
    for bad in ((pts[:, :TN - 8], ids[:, :TN - 8], d_counts.clamp(max=TN - 8)), (pts, ids, None),
                (pts, torch.nn.functional.one_hot(ids.clamp(0, TC).long(), TC + 1).float(), d_counts)):
        with pytest.raises(ValueError, match="one batch shape"):
            t_g.step_graphed(*bad)
    assert len(t_g._graphed) == 1 and t_g.random_sample.step == (3 if sampler == "random" else 0)


@pytest.mark.parametrize("sampler", ["random", "fps"])
@pytest.mark.parametrize("loss", ["samples", "points"])
def test_replays_around_eval_steps_equal_the_eager_steps(loss, sampler):
    """A training script's sequence -- replays, validation steps (the eval chains
    fold the weights the replays changed), replays again -- against an eager
    trainer taken through the same sequence from the same weights: every
    training loss and every validation figure (which the weights of all the
    steps before it decide)."""
    dev = torch.device("cuda", 0)
    t_g = _trainer(12, graphs=True, sampler=sampler, loss=loss)
    t_e = _trainer(12, graphs=True, sampler=sampler, loss=loss)  # (HipAdam on both sides; stepped eagerly)
    seq = [("train", 26, TCOUNTS), ("train", 27, (TN, 9_000)), ("val", 28, (15_000, TN)), ("val", 26, TCOUNTS),
           ("train", 28, (15_000, TN)), ("train", 26, (400, TN)), ("val", 27, (TN, 9_000)), ("train", 27, (TN, 9_000))]
    for i, (mode, seed0, counts) in enumerate(seq):
        pts, _, ids = _batch(seed0, counts=counts)
        pts, ids = pts.to(dev), ids.to(dev)
        d_counts = torch.tensor(counts, dtype=torch.int32)
        if mode == "val":
            got, want = t_g.step(pts, ids, train=False, counts=d_counts), t_e.step(pts, ids, train=False, counts=d_counts)
        else:
            got = t_g.step(pts, ids, counts=d_counts)  # (a replay)
            smp, hist, _ = t_e.samples_and_targets(pts, ids, d_counts)
            want = t_e.step_on_samples(smp, hist)
        print(f"SEQUENCE {loss} {sampler} {i} {mode}: graphed {got!r} eager {want!r}")
        assert abs(got[0] - want[0]) <= 1e-5 * max(1.0, abs(want[0])), (i, mode, got, want)
        # the two sides differ by rounding, which can flip the argmax of a near-tied row; a row carries
        # about 1 / (B S) = 1 / 1024 of the weight under either loss: ten such rows
        assert abs(got[1] - want[1]) <= 0.01, (i, mode, got, want)
    assert len(t_g._graphed) == 1
    assert t_g.random_sample.step == t_e.random_sample.step == (5 if sampler == "random" else 0)


def test_graphed_step_feeds_the_augmentations_counts_to_the_sampler():
    """Augment(drop=0.2) in front, sharing the sampler's seed: after replay r the
    sampler's counts and indices are the oracle chain's -- aug_ref.augment's kept
    counts at augmentation step r into sample_ref at sampler step r."""
    import aug_ref
    from ndnet.augment import Augment
    dev = torch.device("cuda", 0)
    aug = Augment(yaw=0.5, drop=0.2, jitter=0.01, seed=SEED)
    tr = _trainer(10, graphs=True, loss="points", augment=aug)
    cfg = aug_ref.Config.of(aug)
    cases = [(23, (20_000, 560)), (24, (530, 20_000)), (25, (20_000, 20_000))]
    short = 0
    for r, (seed0, counts) in enumerate(cases):
        pts, _, ids = _batch(seed0, counts=counts)
        loss, acc = tr.step_graphed(pts.to(dev), ids.to(dev), list(counts))
        assert np.isfinite(loss.item()) and 0.0 <= acc.item() <= 1.0
        _, _, kept, _, _ = aug_ref.augment(cfg, pts.numpy(), None, counts, r)
        m = [len(k) for k in kept]
        assert all(a < c for a, c in zip(m, counts))  # the dropout did drop
        want = np.full((TB, TS), -1, np.int32)
        for b in range(TB):
            idx = R.choose(R.keys(SEED, 0, b, m[b], r), TS)
            want[b, :len(idx)] = idx
        g = tr._graph_for(pts.shape, ids.shape, True)
        assert g.buffers.sample_counts.tolist() == [min(v, TS) for v in m], (r, m)
        assert np.array_equal(g.buffers.indices.cpu().numpy(), want), r
        short += sum(v < TS for v in m)
    assert short >= 1  # a cloud the augmentation left shorter than S was among them
    assert aug.step == 3 and tr.random_sample.step == 3


def test_twenty_graphed_steps_lower_the_loss():
    """The pieces are connected: the loss on one batch falls over twenty replays."""
    from ndnet.synthetic import make_labelled_batch
    dev = torch.device("cuda", 0)
    pts, gt = make_labelled_batch(TB, TN, TC, seed0=40)
    pts, ids = torch.from_numpy(pts).to(dev), torch.from_numpy(gt.argmax(-1)).to(dev).int()
    tr = _trainer(11, graphs=True)
    losses = [tr.step_graphed(pts, ids)[0].item() for _ in range(20)]
    print("LEARNING", " ".join(f"{v:.3f}" for v in losses))
    assert all(np.isfinite(losses)) and np.mean(losses[-5:]) < losses[0]
    assert tr.random_sample.step == 20
