"""The PointNet-on-FPS baseline on the GPU: the HIP eval forward of
``ndnet.models.pointnet`` against the reference's fixtures, torch fp32 and
float64; its precision modes, re-fold and train mode; and
``segment.segment_points_fps`` end to end, eager and captured.

Bounds are the NDT models': test_model.TOL = 1e-4 on log-probs with
e_hip <= 3 e_torch + 1e-6 against float64, test_model_cls's criterion for the
probabilities, test_model_precision's  e_emu / 3 <= e_hip <= 3 e_emu + 1e-6 for
the reduced modes, test_train_hip's whole-model tolerances for train mode."""
import copy

import numpy as np
import pytest
import torch

from conftest import golden
from fps_ref import fps_ref
from model_init import deterministic_state
from nearest_ref import nearest_ref

TOL = 1e-4  # test_model.TOL, test_model_cls.TOL
SEG = ["pointnet_seg_F768_C28.npz", "pointnet_seg_F64_C5.npz"]
CLS = ["pointnet_cls_F768_C512.npz", "pointnet_cls_F64_C5.npz"]


def _model(F, C, device="cuda", kind="seg", dtype=torch.float32):
    from ndnet.models.pointnet import PointNetClassification, PointNetSegmentation
    m = (PointNetSegmentation if kind == "seg" else PointNetClassification)(3, C, F)
    m.load_state_dict(deterministic_state(m.state_dict()))
    return m.to(device=device, dtype=dtype).eval()


def _points(B, N, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.rand((B, N, 3), device="cuda", generator=g) * 20 - 10


_shared = {}


def _shape(F, C, B, N):
    """Model, points and the float64 forward of one shape, computed once."""
    key = (F, C, B, N)
    if key not in _shared:
        m, p = _model(F, C), _points(B, N, F + C + N)
        with torch.no_grad():
            ref64 = _model(F, C, dtype=torch.float64).forward_torch(p.double())
        _shared[key] = (m, p, ref64)
    return _shared[key]


def _spy_chains(monkeypatch):
    from ndnet.models import pointnet_hip as ph
    calls, real = [], ph._run_chain
    monkeypatch.setattr(ph, "_run_chain", lambda *a, **k: calls.append(1) or real(*a, **k))
    return calls


@pytest.mark.gpu
@pytest.mark.parametrize("name", SEG)
def test_hip_forward_matches_reference_fixture(monkeypatch, name):
    from ndnet.models import pointnet_hip as ph
    assert ph.available(), "the HIP forward must be built (no silent fallback)"
    z = golden(name)
    m = _model(int(z["feature_dim"]), int(z["num_classes"]))
    calls = _spy_chains(monkeypatch)
    with torch.no_grad():
        out = m(torch.from_numpy(z["points"]).cuda()).cpu().numpy()
    assert len(calls) == 4, "the eval forward must run the four HIP chains"
    err = np.abs(out - z["out_eval"]).max()
    print(f"{name}: HIP vs the reference's out_eval {err:.3e}")
    assert out.shape == z["out_eval"].shape and err < TOL


@pytest.mark.gpu
@pytest.mark.parametrize("name", CLS)
def test_hip_classification_matches_reference_fixture(monkeypatch, name):
    """test_model_cls's criterion: log-probabilities as close to float64 as
    torch's own fp32 forward is (factor 3), within 1e-4, rows summing to 1."""
    z = golden(name)
    F, C = int(z["feature_dim"]), int(z["num_classes"])
    m, m64 = _model(F, C, kind="cls"), _model(F, C, kind="cls", dtype=torch.float64)
    p = torch.from_numpy(z["points"]).cuda()
    calls = _spy_chains(monkeypatch)
    with torch.no_grad():
        out = m(p)
        ref64 = m64.forward_torch(p.double())
        e_t = (m.forward_torch(p).double().log() - ref64.log()).abs().max().item()
    assert len(calls) == 3 and out.shape == (2, C, 1) and out.dtype == torch.float32
    e_hip = (out.double().log() - ref64.log()).abs().max().item()
    e_fix = np.abs(np.log(out.cpu().numpy().astype(np.float64)) - np.log(z["out_eval"].astype(np.float64))).max()
    rows = (out.double().sum(dim=1) - 1).abs().max().item()
    print(f"{name}: e_hip {e_hip:.3e} e_torch_fp32 {e_t:.3e} vs out_eval {e_fix:.3e} |row sum - 1| {rows:.1e}")
    assert e_hip <= 3 * e_t + 1e-6
    assert e_hip < TOL and e_fix < TOL
    assert rows <= 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("B,N", [(3, 100), (2, 4160)])
def test_hip_forward_matches_torch_fp32(B, N):
    """A ragged tile tail on the 32-point build, and 65 tiles of the 64-point build."""
    from ndnet.models import pointnet_hip as ph
    m = _model(768, 28)
    p = _points(B, N, B * 1000 + N)
    with torch.no_grad():
        out = m(p)
        ref = m.forward_torch(p)
        emu = ph.segmentation_forward(m, p, None, chain=ph._chain_torch)
    assert out.shape == (B, N, 29)
    print(f"{B}x{N}: HIP vs torch fp32 {(out - ref).abs().max().item():.3e}, vs emulation "
          f"{(out - emu).abs().max().item():.3e}")
    assert (out - ref).abs().max().item() < TOL
    assert (out - emu).abs().max().item() < TOL
    top2 = ref.topk(2, dim=-1).values
    clear = (top2[..., 0] - top2[..., 1]) > 2 * TOL
    assert torch.equal(out.argmax(-1)[clear], ref.argmax(-1)[clear])


@pytest.mark.gpu
def test_hip_forward_is_as_close_to_float64_as_torch_fp32():
    m, p, ref64 = _shape(768, 28, 2, 256)
    with torch.no_grad():
        out = m(p)
        e_t = (m.forward_torch(p).double() - ref64).abs().max().item()
    e_hip = (out.double() - ref64).abs().max().item()
    print(f"e_hip {e_hip:.3e} e_torch_fp32 {e_t:.3e}")
    assert e_hip <= 3 * e_t + 1e-6
    assert e_hip < TOL


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["x3", "bf16"])
@pytest.mark.parametrize("F,C,B,N", [(768, 28, 2, 256), (64, 5, 3, 77)], ids=["F768", "F64"])
def test_reduced_modes_match_their_emulation(F, C, B, N, mode):
    from test_model_precision import _emulator
    from ndnet.models import pointnet_hip as ph
    m, p, ref64 = _shape(F, C, B, N)
    try:
        m.precision = mode
        with torch.no_grad():
            out = m(p)
            emu = ph.segmentation_forward(m, p, None, chain=_emulator(ph._folded(m)["W"], mode))
            m.precision = "x6"
            x6 = m(p)
    finally:
        m.precision = None
    assert out.shape == (B, N, C + 1) and out.dtype == torch.float32 and bool(torch.isfinite(out).all())
    lse = torch.logsumexp(out.double(), dim=-1).abs().max().item()
    e_hip = (out.double() - ref64).abs().max().item()
    e_emu = (emu.double() - ref64).abs().max().item()
    d_x6 = (out - x6).abs().max().item()
    print(f"F={F} C={C} {B}x{N} {mode}: e_hip {e_hip:.3e} e_emu {e_emu:.3e} |mode - x6| {d_x6:.3e} |logsumexp| {lse:.1e}")
    assert lse <= 1e-5
    assert e_emu / 3 <= e_hip <= 3 * e_emu + 1e-6
    assert d_x6 > 0
    with torch.no_grad():
        assert torch.equal(m(p), x6)  # back in the module-wide mode, bit for bit


@pytest.mark.gpu
def test_mode_switch_refolds_changed_weights_in_place():
    """test_model.test_mode_switch_refolds_weights_changed_without_versions for the baseline."""
    from test_model import _perturb
    m = _model(64, 5)
    p = _points(2, 100, 9)
    with torch.no_grad():
        first = m(p).clone()
        W = m._hip["W"]
        m.train()
        _perturb(m, 2, versions=False)
        m.eval()
        out = m(p)
        ref = m.forward_torch(p)
    assert m._hip["W"] is W, "the re-fold is in place (ndnet_pn_fold_run), not a rebuild"
    assert (out - ref).abs().max().item() < TOL and (out - first).abs().max().item() > 1e-3
    with torch.no_grad():
        _perturb(m, 3, versions=False, params=False)
        kept = m(p)   # no mode switch, no version bump: the previous fold
    assert torch.equal(kept, out)


@pytest.mark.gpu
def test_train_forward_backward_matches_torch(monkeypatch):
    """Train mode at B = 4, N = 64 (the fixture's train input): every block on
    the HIP train kernels, log-probs, running statistics and every parameter
    gradient against the torch composition, with the tolerances of
    test_train_hip.test_segmentation_train_forward_backward_matches_torch."""
    from ndnet.models import ndtnet, train_hip
    from ndnet.training import segmentation_loss
    z = golden(SEG[0])
    model = _model(768, 28).train()
    ref_model = copy.deepcopy(model)
    f64_model = copy.deepcopy(model).double()
    pts = torch.from_numpy(z["points_train"]).cuda()
    calls = []
    for name, tag in (("conv_bn_act", 1), ("conv_bn_act_pool", 2), ("seg_conv1", 1), ("fc_bn_act", 3), ("transform_t", 4)):
        real = getattr(train_hip, name)
        monkeypatch.setattr(train_hip, name, lambda *a, _r=real, _t=tag, **k: calls.append(_t) or _r(*a, **k))
    out = model(pts)
    # 3 + 3 TNet blocks (the last of each pooled), 3 PointNet (conv3 pooled), 3 seg head + conv4;
    # 3 + 3 TNet FC layers; one x^T t2
    assert calls.count(1) + calls.count(2) == 13 and calls.count(2) == 3
    assert calls.count(3) == 6 and calls.count(4) == 1
    monkeypatch.setattr(ndtnet, "_TRAIN_TORCH", True)
    ref = ref_model(pts)
    assert len(calls) == 20
    f64 = f64_model(pts.double())
    e_fix = np.abs(out.detach().cpu().numpy() - z["out_train"]).max()
    e_hip = (out.double() - f64).abs().max().item()
    e_torch = (ref.double() - f64).abs().max().item()
    print(f"vs the reference's out_train {e_fix:.3e}; vs float64: HIP {e_hip:.3e}, torch fp32 {e_torch:.3e}; "
          f"HIP vs torch {(out - ref).abs().max().item():.3e}")
    torch.testing.assert_close(out, ref, rtol=1e-4, atol=1e-4)
    assert e_hip <= 2 * e_torch + 1e-6, (e_hip, e_torch)
    for (n, b1), b2 in zip(model.named_buffers(), ref_model.buffers()):
        if b1.dtype.is_floating_point:
            torch.testing.assert_close(b1, b2, rtol=1e-4, atol=1e-5, msg=n)
        else:
            assert torch.equal(b1, b2), n
    gt = torch.nn.functional.one_hot(torch.randint(0, 29, (4, 64), device="cuda"), 29).float()
    segmentation_loss(out, gt).backward()
    segmentation_loss(ref, gt).backward()
    segmentation_loss(f64, gt.double()).backward()
    for (n, p1), p2, p3 in zip(model.named_parameters(), ref_model.parameters(), f64_model.parameters()):
        assert p1.grad is not None, n
        ref_norm = p3.grad.norm().item()
        e_h = (p1.grad.double() - p3.grad).norm().item() / max(ref_norm, 1e-30)
        e_t = (p2.grad.double() - p3.grad).norm().item() / max(ref_norm, 1e-30)
        print(f"{n:45s} rel err vs float64: HIP {e_h:.2e} torch fp32 {e_t:.2e}")
        if n.endswith("bias") and "conv" in n and not n.startswith("conv4"):
            continue  # conv biases ahead of a BatchNorm have gradient sum(dy) ~ 0: rounding only
        assert e_h <= max(3 * e_t, 1e-4), (n, e_h, e_t)


def _scan_batch(seed, counts):
    """B = 2 ragged scans padded to 3000 points, NaN in the padding."""
    g = torch.Generator().manual_seed(seed)
    pts = torch.rand((2, 3000, 3), generator=g) * torch.tensor([80.0, 80.0, 6.0]) - torch.tensor([40.0, 40.0, 2.0])
    for b, c in enumerate(counts):
        pts[b, c:] = float("nan")
    return pts.cuda(), torch.tensor(counts, dtype=torch.int32, device="cuda")


def _check_end_to_end(m, pts, counts, labels, log_probs, buf):
    S = 256
    p_np, c_np = pts.cpu().numpy(), counts.cpu().numpy()
    idx = buf.indices.cpu().numpy()
    rows = buf.rows.cpu().numpy()
    for b in range(2):
        assert np.array_equal(idx[b], fps_ref(p_np[b], S, int(c_np[b]))[0]), b
        smp = p_np[b][idx[b]]
        assert np.array_equal(buf.samples[b].cpu().numpy(), smp)
        assert np.array_equal(rows[b], nearest_ref(p_np[b], smp, int(c_np[b]))[0]), b
    assert labels.dtype == torch.int32 and labels.shape == (2, 3000) and log_probs.shape == (2, S, 6)
    cls = log_probs.argmax(-1).cpu().numpy()
    want = np.where(rows >= 0, np.take_along_axis(cls, np.maximum(rows, 0), axis=1), -1)
    assert np.array_equal(labels.cpu().numpy(), want)
    for b in range(2):
        assert (want[b, c_np[b]:] == -1).all() and (want[b, :c_np[b]] >= 0).all()
    with torch.no_grad():
        assert (log_probs - m.forward_torch(buf.samples)).abs().max().item() < TOL


@pytest.mark.gpu
def test_segment_points_fps_end_to_end_and_captured():
    from ndnet import segment
    m = _model(64, 5)
    pts, counts = _scan_batch(1, [3000, 1777])
    labels, log_probs = segment.segment_points_fps(m, 256, pts, counts=counts)
    # (the eager call's own buffers are not returned: run it again into buffers to look inside)
    buf = segment.FpsSegmentBuffers(2, 3000, 256, pts.device)
    labels_b, log_probs_b = segment.segment_points_fps(m, 256, pts, counts=counts, buffers=buf)
    assert labels_b is buf.labels and torch.equal(labels_b, labels) and torch.equal(log_probs_b, log_probs)
    _check_end_to_end(m, pts, counts, labels, log_probs, buf)
    # counts as a list; no counts at all on the full cloud
    l2, _ = segment.segment_points_fps(m, 256, pts, counts=[3000, 1777])
    assert torch.equal(l2, labels)
    l3, _ = segment.segment_points_fps(m, 256, pts[:1])
    assert torch.equal(l3, labels[:1])
    # point-level IoU of labels made from the rows themselves: 1 for every class present
    conf = segment.confusion(labels, labels.clone(), m.num_classes)
    per_class, mean = segment.iou(conf)
    present = torch.bincount(labels[labels >= 0].long(), minlength=6) > 0
    assert bool(present.any()) and bool((per_class[present] == 1).all()) and mean.item() == 1.0
    assert int(conf.sum()) == 3000 + 1777

    # ---- the same sequence captured once, on one stream, replayed on a second batch ----
    pts2, counts2 = _scan_batch(2, [2500, 3000])
    eager_labels, eager_lp = segment.segment_points_fps(m, 256, pts2, counts=counts2)
    eager_labels, eager_lp = eager_labels.clone(), eager_lp.clone()
    static_pts, static_counts = pts.clone(), counts.clone()
    cbuf = segment.FpsSegmentBuffers(2, 3000, 256, pts.device)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        segment.segment_points_fps(m, 256, static_pts, counts=static_counts, buffers=cbuf)  # warm-up
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        g_labels, g_lp = segment.segment_points_fps(m, 256, static_pts, counts=static_counts, buffers=cbuf)
    graph.replay()
    assert torch.equal(g_labels, labels) and torch.equal(g_lp, log_probs)
    static_pts.copy_(pts2)
    static_counts.copy_(counts2)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(g_labels, eager_labels) and torch.equal(g_lp, eager_lp)
    assert (g_labels[0, 2500:] == -1).all() and (g_labels[0, :2500] >= 0).all()


@pytest.mark.gpu
def test_segment_points_fps_with_clouds_shorter_than_n_samples():
    """Counts 600, 100 and 1 at n_samples = 256: a short cloud's indices end in -1, the model's
    input repeats its point 0 there, and those copies stand for no point -- every row lies
    below min(count, n_samples).  The full cloud beside them is scored as when it is alone."""
    from ndnet import segment
    B, n, S, counts = 3, 600, 256, [600, 100, 1]
    m = _model(64, 5)
    g = torch.Generator().manual_seed(3)
    pts = torch.rand((B, n, 3), generator=g) * torch.tensor([80.0, 80.0, 6.0]) - torch.tensor([40.0, 40.0, 2.0])
    for b, c in enumerate(counts):
        pts[b, c:] = float("nan")
    pts = pts.cuda()
    d_counts = torch.tensor(counts, dtype=torch.int32, device="cuda")
    labels, log_probs = segment.segment_points_fps(m, S, pts, counts=d_counts)
    buf = segment.FpsSegmentBuffers(B, n, S, pts.device)
    labels_b, log_probs_b = segment.segment_points_fps(m, S, pts, counts=d_counts, buffers=buf)
    assert labels_b is buf.labels and torch.equal(labels_b, labels) and torch.equal(log_probs_b, log_probs)
    assert labels.dtype == torch.int32 and labels.shape == (B, n) and log_probs.shape == (B, S, 6)

    p_np = pts.cpu().numpy()
    idx, rows, samples = buf.indices.cpu().numpy(), buf.rows.cpu().numpy(), buf.samples.cpu().numpy()
    assert buf.sample_counts.tolist() == [256, 100, 1]
    for b, c in enumerate(counts):
        ms = min(c, S)
        assert np.array_equal(idx[b], fps_ref(p_np[b], S, c)[0]), b
        assert (idx[b, :ms] >= 0).all() and (idx[b, ms:] == -1).all()
        assert np.array_equal(samples[b], p_np[b][np.maximum(idx[b], 0)]), b
        assert np.array_equal(samples[b, ms:], np.broadcast_to(p_np[b, 0], (S - ms, 3)))  # its first point, repeated
        assert np.array_equal(rows[b], nearest_ref(p_np[b], samples[b], c, ms)[0]), b
        assert (rows[b, :c] >= 0).all() and (rows[b, :c] < ms).all() and (rows[b, c:] == -1).all()
    cls = log_probs.argmax(-1).cpu().numpy()
    want = np.where(rows >= 0, np.take_along_axis(cls, np.maximum(rows, 0), axis=1), -1)
    got = labels.cpu().numpy()
    assert np.array_equal(got, want)
    for b, c in enumerate(counts):
        assert (got[b, :c] >= 0).all() and (got[b, c:] == -1).all()
    with torch.no_grad():
        assert (log_probs - m.forward_torch(buf.samples)).abs().max().item() < TOL
    # a short neighbour does not leak into the full cloud
    l0, lp0 = segment.segment_points_fps(m, S, pts[:1], counts=[600])
    e = (log_probs[0] - lp0[0]).abs().max().item()
    print(f"cloud 0 beside short clouds vs alone: log-probs differ by {e:.3e}")
    assert e < TOL and bool(torch.isfinite(log_probs).all())


@pytest.mark.gpu
def test_ndt_model_is_untouched_by_a_baseline_forward():
    """Workspaces are cached per model: an NDTNetSegmentation forward before and
    after a baseline forward of the same (B, N) gives identical bits."""
    from ndnet.models.ndtnet import NDTNetSegmentation
    ndt = NDTNetSegmentation(3, 5, 64)
    ndt.load_state_dict(deterministic_state(ndt.state_dict()))
    ndt = ndt.cuda().eval()
    base = _model(64, 5)
    g = torch.Generator(device="cuda").manual_seed(5)
    p = torch.rand((2, 100, 3), device="cuda", generator=g) * 20 - 10
    c = torch.randn((2, 100, 9), device="cuda", generator=g)
    with torch.no_grad():
        before = ndt(p, c).clone()
        b1 = base(p).clone()
        after = ndt(p, c).clone()
        b2 = base(p)
    assert torch.equal(before, after) and torch.equal(b1, b2)
    assert (before - ndt.forward_torch(p, c)).abs().max().item() < TOL
