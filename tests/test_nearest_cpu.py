"""The PointNet-on-FPS baseline, the parts that need no GPU: the numpy oracle
of the nearest-sample rows against plain loops, ``nearest_sample``'s own
checks, and ``ndnet.models.pointnet`` on the CPU against the reference's
fixtures (make_pointnet_golden.py)."""
import numpy as np
import pytest
import torch

from conftest import golden
from model_init import deterministic_state
from nearest_ref import lattice_case, nearest_loops, nearest_ref, transform3_ref

SEG = ["pointnet_seg_F768_C28.npz", "pointnet_seg_F64_C5.npz"]
CLS = ["pointnet_cls_F768_C512.npz", "pointnet_cls_F64_C5.npz"]


def _model(name, z=None):
    from ndnet.models.pointnet import PointNetClassification, PointNetSegmentation
    z = golden(name) if z is None else z
    cls = PointNetSegmentation if "_seg_" in name else PointNetClassification
    m = cls(3, int(z["num_classes"]), int(z["feature_dim"]))
    m.load_state_dict(deterministic_state(m.state_dict()))
    return m.eval()


def _same(a, b):
    (r1, d1), (r2, d2) = a, b
    return np.array_equal(r1, r2) and np.array_equal(d1, d2, equal_nan=True)


def test_oracle_forms_agree_on_the_lattice():
    pts, smp = lattice_case()
    assert pts.shape == (512, 3) and smp.shape == (37, 3)
    rows, dist = nearest_ref(pts, smp, chunk=100)
    assert _same((rows, dist), nearest_loops(pts, smp))
    assert rows.min() >= 0 and np.array_equal(dist, np.round(dist))  # small integers
    # ties are there and go to the smaller index: another sample at the same distance never has a smaller one
    d_all = ((pts[:, None, :] - smp[None, :, :]) ** 2).sum(-1)
    tied = (d_all == dist[:, None]).sum(1) > 1
    assert tied.sum() >= 100  # (of 512 points)
    assert np.array_equal(rows, np.argmax(d_all == dist[:, None], axis=1))
    # a point that is itself a sample: distance 0
    assert (dist == 0).sum() == 37


def test_oracle_forms_agree_on_a_random_case():
    rng = np.random.default_rng(4)
    pts = rng.uniform(-50, 50, (90, 3)).astype(np.float32)
    smp = rng.uniform(-50, 50, (21, 3)).astype(np.float32)
    smp[13] = smp[5]              # a duplicate: the smaller index wins
    pts[7] = smp[13]
    pts[3, 1] = np.nan
    pts[4, 0] = np.inf
    smp[2, 2] = np.nan            # never chosen
    smp[9, 0] = -np.inf
    for count, sc in ((None, None), (61, 14), (1, 1), (0, 21), (90, 0), (200, -5)):
        a, b = nearest_ref(pts, smp, count, sc, chunk=32), nearest_loops(pts, smp, count, sc)
        assert _same(a, b), (count, sc)
    rows, dist = nearest_ref(pts, smp)
    assert rows[3] == -1 and rows[4] == -1 and np.isinf(dist[3]) and np.isinf(dist[4])
    assert rows[7] == 5 and dist[7] == 0
    assert 2 not in rows and 9 not in rows and 13 not in rows
    rows, dist = nearest_ref(pts, np.full((4, 3), np.nan, np.float32))
    assert (rows == -1).all() and np.isinf(dist).all()


def test_transform_oracle_clamps_like_nan_to_num():
    p = np.array([[1, 2, 3], [np.inf, 1, 1], [-np.inf, 1, 1], [np.inf, -np.inf, 0], [3e38, 3e38, 0]], np.float32)
    t = np.array([[1, 0, 0], [1, 1, 0], [0, 0, 2]], np.float32)
    want = torch.nan_to_num(torch.from_numpy(p) @ torch.from_numpy(t).T, nan=0.0).numpy()
    assert np.array_equal(transform3_ref(p, t), want)


def test_wrapper_checks_come_before_the_gpu(monkeypatch):
    from ndnet import _lib
    from ndnet.preprocessing import nearest_sample
    pts, smp = torch.zeros((2, 16, 3)), torch.zeros((2, 5, 3))
    with monkeypatch.context() as mp:
        def no_gpu_work():
            raise AssertionError("GPU work before the argument check")
        mp.setattr(_lib, "require_gpu", no_gpu_work)
        for bad in ((pts[0], smp), (pts, smp[0]), (torch.zeros((2, 16, 4)), smp), (pts, torch.zeros((2, 5, 2))),  # rank, width
                    (pts.double(), smp), (pts, smp.half()), (pts.int(), smp),                                   # dtype
                    (pts, torch.zeros((3, 5, 3))), (pts, torch.zeros((1, 5, 3)))):                              # batch size
            with pytest.raises(ValueError):
                nearest_sample(*bad)
        with pytest.raises(ValueError, match="clouds"):
            nearest_sample(pts, torch.zeros((3, 5, 3)))
        i32, f32 = torch.zeros((2, 16), dtype=torch.int32), torch.zeros((2, 16))
        for kw in (dict(out=torch.zeros((2, 15), dtype=torch.int32)), dict(out=torch.zeros((2, 16), dtype=torch.int64)),
                   dict(out=f32), dict(out=torch.zeros((2, 16), dtype=torch.int32, device="meta")),
                   dict(dist=torch.zeros((2, 17))), dict(dist=torch.zeros((16, 2))), dict(dist=f32.double()),
                   dict(dist=i32), dict(dist=torch.zeros((2, 16), device="meta")),
                   dict(out=i32, dist=torch.zeros((2, 16, 1))),
                   dict(counts=[16, 16, 16]), dict(sample_counts=torch.tensor([[5, 5]]))):
            with pytest.raises(ValueError):
                nearest_sample(pts, smp, **kw)
    with pytest.raises(RuntimeError):  # valid arguments, CPU tensors: no CPU fallback
        nearest_sample(pts, smp, counts=[16, 3], sample_counts=[5, 1], out=i32, dist=f32)


@pytest.mark.parametrize("name", SEG + CLS)
def test_state_keys_and_parameter_counts_match_the_fixtures(name):
    z = golden(name)
    m = _model(name, z)
    assert list(m.state_dict().keys()) == [str(k) for k in z["state_keys"]]
    assert sum(p.numel() for p in m.parameters()) == int(z["param_count"])


def test_constructor_defaults_are_the_references():
    from ndnet.models.pointnet import PointNet, PointNetClassification, PointNetSegmentation
    s, c, f = PointNetSegmentation(), PointNetClassification(), PointNet()
    assert (s.point_dim, s.num_classes, s.feature_dim) == (3, 16, 768)
    assert (c.point_dim, c.num_classes, c.feature_dim) == (3, 512, 768)
    assert (f.point_dim, f.feature_dim) == (3, 768) and f.t1.in_dim == 3 and f.t2.in_dim == 64
    assert s.conv1.in_channels == 768 + 64 and s.conv4.out_channels == 17 and f.conv1.in_channels == 3


@pytest.mark.parametrize("name", SEG + CLS)
def test_cpu_eval_forward_equals_the_reference_bit_for_bit(name):
    z = golden(name)
    m = _model(name, z)
    with torch.no_grad():
        out = m(torch.from_numpy(z["points"])).numpy()
    assert out.shape == z["out_eval"].shape and np.array_equal(out, z["out_eval"])


def test_cpu_train_forward_equals_the_reference_bit_for_bit():
    """The bound of test_model.test_torch_train_forward_matches_reference_b16_fixture: equality."""
    z = golden(SEG[0])
    m = _model(SEG[0], z).train()
    with torch.no_grad():
        out = m(torch.from_numpy(z["points_train"])).numpy()
    assert z["points_train"].shape == (4, 64, 3) and np.array_equal(out, z["out_train"])


@pytest.mark.parametrize("name", [SEG[1], CLS[1], SEG[0]])
def test_folded_algebra_cpu(name):
    """The HIP path's folding for the baseline (BN, the transform as a step of
    its own, conv1 shared, t2 through conv1, split seg head), evaluated with
    torch ops."""
    from ndnet.models import pointnet_hip as ph
    z = golden(name)
    m = _model(name, z)
    fwd = ph.segmentation_forward if "_seg_" in name else ph.classification_forward
    with torch.no_grad():
        out = fwd(m, torch.from_numpy(z["points"]), None, chain=ph._chain_torch).numpy()
    assert np.abs(out - z["out_eval"]).max() < 1e-5
    W = m._hip["W"]
    assert W.baseline and W.t1_basis is None and W.jobs is not None
    assert not any(kind == 4 for kind, *_ in W.jobs)  # no NDNET_FOLD_BASIS job


def test_fold_jobs_pass_the_library_check():
    """ndnet_pn_fold_prepare (host code) takes the baseline's job list, the
    K = 16 fragment copy of the 3-input conv1 among it."""
    import ctypes
    from ndnet import _lib
    from ndnet.models import pointnet_hip as ph
    m = _model(SEG[1])
    W = ph._Folded(m)
    arr = (ph._FoldJob * len(W.jobs))()
    seen = False
    for J, (kind, out, layer, bn, k0, K, Kp, Np, eye) in zip(arr, W.jobs):
        J.kind, J.out, J.N, J.K, J.ld, J.k0 = kind, out.data_ptr(), layer.weight.shape[0], K, layer.weight.shape[1], k0
        J.Kp, J.Np, J.eye = Kp, Np, eye
        J.bias = layer.bias.data_ptr()
        J.w = layer.weight.data_ptr()
        if bn is not None:
            J.gamma, J.beta = bn.weight.data_ptr(), bn.bias.data_ptr()
            J.mean, J.var, J.eps = bn.running_mean.data_ptr(), bn.running_var.data_ptr(), bn.eps
        seen |= kind == 1 and layer is m.feature_extractor.conv1 and (K, Kp, Np) == (3, 16, 64)
    assert seen
    blocks = ctypes.c_int64()
    assert _lib.lib().ndnet_pn_fold_prepare(arr, len(arr), ctypes.byref(blocks)) == 0 and blocks.value > 0


def test_dispatch_sends_cpu_training_and_grad_inputs_to_forward_torch(monkeypatch):
    m = _model(SEG[1])
    calls = []
    real = m.forward_torch
    monkeypatch.setattr(m, "forward_torch", lambda p: (calls.append(1), real(p))[1])
    pts = torch.from_numpy(golden(SEG[1])["points"])
    assert not m._hip_eval_points(pts)                       # a CPU tensor
    with torch.no_grad():
        m(pts)
    assert len(calls) == 1
    cuda_like = type("T", (), dict(is_cuda=True, requires_grad=False))()  # a device tensor's flags, no device needed
    with torch.no_grad():
        assert m._hip_eval(cuda_like, cuda_like)             # eval, no autograd, on a GPU: the HIP path
        m.train()
        assert not m._hip_eval(cuda_like, cuda_like)         # a training model
        m.eval()
    grad_in = type("T", (), dict(is_cuda=True, requires_grad=True))()
    for p in m.parameters():
        p.requires_grad_(False)
    assert m._hip_eval(cuda_like, cuda_like)                 # grad enabled, nothing requires it
    assert not m._hip_eval(grad_in, grad_in)                 # a grad-requiring input
    m.train()
    out = m(pts)                                             # train mode on the CPU: forward_torch
    assert len(calls) == 2 and out.shape == (2, 40, 6)
