"""The trainer with ``augment=``: the augmented eager step equals a plain
trainer's step on the separately augmented batch (both losses), the eval step
never augments, one-hot labels give the same bits as ids, and the captured step
draws a new augmentation on every replay.  Shapes and tolerances are those of
tests/test_point_loss_gpu.py (loss 1e-5 relative, gradients 1e-4 of the largest
gradient)."""
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TB, TN, TK, TC = 2, 20_000, 500, 28
TCOUNTS = (20_000, 12_345)


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


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


def _aug(drop=0.3, seed=12):
    from ndnet.augment import Augment
    return Augment(yaw=math.pi, scale=(0.95, 1.05), flip=(0.0, 0.5), shift=(0.2, 0.2, 0.05), jitter=0.01, drop=drop,
                   seed=seed)


def _same_weights(a, b):
    return all(torch.equal(p, q) for p, q in zip(a.model.parameters(), b.model.parameters())) and \
        all(torch.equal(p, q) for p, q in zip(a.model.buffers(), b.model.buffers()))


@pytest.mark.parametrize("loss", ["nds", "points"])
@pytest.mark.parametrize("drop,ragged", [(0.3, True), (0.3, False), (0.0, True), (0.0, False)])
def test_augmented_eager_step_equals_the_step_on_the_augmented_batch(loss, drop, ragged):
    dev = torch.device("cuda", 0)
    counts = list(TCOUNTS) if ragged else None
    pts, gt, ids = _batch(31) if ragged else _batch(31, counts=(TN, TN))
    A, A2 = _aug(drop), _aug(drop)
    t_aug, t_ref = _trainer(4, loss=loss, augment=A), _trainer(4, loss=loss)
    assert A.stream == 0  # no process group: resolved to 0 by the trainer
    for step in range(2):
        got = t_aug.step(pts, ids, counts=counts)
        p2, l2, c2 = A2(pts.to(dev), ids.to(dev), counts)
        if drop == 0.0:
            assert c2.tolist() == (counts or [TN, TN])
        else:
            assert all(1 <= k < m for k, m in zip(c2.tolist(), counts or [TN, TN]))
        want = t_ref.step(p2, l2, counts=c2)
        print(f"AUG EAGER {loss} drop {drop} ragged {ragged} step {step}: {got!r} kept {c2.tolist()}")
        assert got == want and np.isfinite(got[0])
        assert _same_weights(t_aug, t_ref)
        assert A.step == A2.step == step + 1
    if drop == 0.0 and not ragged:
        # whole clouds and no dropout: the augmented step stayed on the fixed-size path
        pcl = t_aug.nds_and_targets(pts, ids, None, augment=True)[0]
        from ndnet.preprocessing.ndtnet_preprocessing import ndt_preprocessing
        assert ndt_preprocessing.last_counts is None and pcl.shape == (TB, TK, 3)
    # the eval step never augments: the plain trainer's figures, the counter where it was
    before = A.step
    assert t_aug.step(pts, ids, train=False, counts=counts) == t_ref.step(pts, ids, train=False, counts=counts)
    assert A.step == before
    # without augment=True nds_and_targets is what it was
    for a, b in zip(t_aug.nds_and_targets(pts, ids, counts), t_ref.nds_and_targets(pts, ids, counts)):
        assert (a is None and b is None) or torch.equal(a, b)
    assert A.step == before


@pytest.mark.parametrize("loss", ["nds", "points"])
def test_one_hot_labels_give_the_same_bits_as_ids(loss):
    pts, gt, ids = _batch(31)
    counts = list(TCOUNTS)
    t_oh, t_id = _trainer(6, loss=loss, augment=_aug()), _trainer(6, loss=loss, augment=_aug())
    r_oh, r_id = t_oh.step(pts, gt, counts=counts), t_id.step(pts, ids, counts=counts)
    assert r_oh == r_id and np.isfinite(r_id[0])
    assert _same_weights(t_oh, t_id)
    t_oh.augment.step = t_id.augment.step = 7
    for a, b in zip(t_oh.nds_and_targets(pts, gt, counts, augment=True),
                    t_id.nds_and_targets(pts, ids, counts, augment=True)):
        assert (a is None and b is None) or torch.equal(a, b)


def test_graphed_step_draws_a_new_augmentation_on_every_replay():
    """Three replays of one captured augmented step, each against the eager
    augmented step from the same weights and the same counter."""
    from ndnet.training import point_loss
    dev = torch.device("cuda", 0)
    A_g, A_e = _aug(0.3), _aug(0.3)
    t_g = _trainer(9, graphs=True, loss="points", augment=A_g)
    t_e = _trainer(9, graphs=True, loss="points", augment=A_e)
    m_g, m_e = t_g.model, t_e.model
    cases = [(20, TCOUNTS), (21, (9_999, 20_000)), (22, (TN, TN))]
    xforms = []
    for i, (seed0, counts) in enumerate(cases):
        pts, _, ids = _batch(seed0, counts=counts, pad_label=TC + 5 + i)
        pts, ids = pts.to(dev), ids.to(dev)
        d_counts = torch.tensor(counts, dtype=torch.int32, device=dev)
        if i == 0:
            t_g._graph_for(pts.shape, ids.shape, True)  # build: warm-up, capture, roll-back
            assert A_g.step == 0, "the warm-up's draws were not rolled back"
        with torch.no_grad():  # the eager side starts from the graph side's weights
            for a, b in zip(m_e.parameters(), m_g.parameters()):
                a.copy_(b)
            for a, b in zip(m_e.buffers(), m_g.buffers()):
                a.copy_(b)
        assert A_e.step == A_g.step == i
        pcl, covs, _, hist = t_e.nds_and_targets(pts, ids, d_counts, augment=True)
        x_e = A_e.xform.clone()
        m_e.train()
        t_e.opt.zero_grad(set_to_none=True)
        l_e = point_loss(m_e(pcl, covs), hist)
        l_e.backward()
        l_g, a_g = t_g.step_graphed(pts, ids, d_counts)
        print(f"AUG GRAPHED {i}: loss graph {l_g.item()!r} eager {l_e.item()!r} acc {a_g.item()!r}")
        assert abs(l_g.item() - l_e.item()) <= 1e-5 * max(1.0, abs(l_e.item())), (i, l_g.item(), l_e.item())
        assert 0.0 <= a_g.item() <= 1.0
        scale = max(q.grad.abs().max().item() for q in m_e.parameters())
        for (name, a), b in zip(m_g.named_parameters(), m_e.parameters()):
            assert (a.grad - b.grad).abs().max().item() <= 1e-4 * scale, (i, name)
        assert torch.equal(A_g.xform, x_e)  # the replay drew the eager step's matrices
        xforms.append(A_g.xform.clone())
    assert not torch.equal(xforms[0], xforms[1]) and not torch.equal(xforms[1], xforms[2])
    assert len(t_g._graphed) == 1
    assert A_g.step == A_e.step == 3
