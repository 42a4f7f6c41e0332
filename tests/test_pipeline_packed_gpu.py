"""packed=True through the graphed and pipelined surfaces: log-probs, points'
rows and labels are bit-equal to the float32 path fed the oracle-decoded clouds
(tests/packed_ref.py), batch by batch.

Every ring slot holds a different batch (U and L clouds in turn, distinct
seeds) with its own qparams -- each cloud's own origin and default step -- so a
decode with another slot's qparams, or of another slot's input, cannot pass;
the tests first check that consecutive slots' qparams and rows differ.
n = 20 003: a cloud's q starts 16-byte aligned only for b = 0, and the n % 8
tail's 3 points per cloud go to the fill."""
import numpy as np
import pytest

import packed_ref as R

pytestmark = pytest.mark.gpu

B, N_PTS, K = 4, 20_003, 400
SLOTS = 6  # the largest ring the tests build: F, N = 3, 2


def _model(F=64, C=5, seed=3):
    import torch
    from ndnet.models.ndtnet import NDTNetSegmentation
    torch.manual_seed(seed)
    m = NDTNetSegmentation(3, C, F).cuda().eval()
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm1d):
                mod.running_mean.uniform_(-0.2, 0.2)
                mod.running_var.uniform_(0.5, 1.5)
    return m


def _kind(j):
    return "L" if j % 2 else "U"


def _counts(j, variant):
    """Counts in n / 2 .. n for slot j: a cloud at n, one with count % 8 != 0."""
    rng = np.random.default_rng(50 * j + variant)
    c = rng.integers(N_PTS // 2, N_PTS + 1, B)
    c[(j + variant) % B] = N_PTS
    c[(j + variant + 1) % B] = N_PTS // 2 + 3 + 8 * j + 16 * variant
    return [int(x) for x in c]


_packed_cache = {}


def _packed_batch(j, variant=None):
    """Slot j's batch as (q, qparams, counts or None, decoded float32): packed
    by pack_points -- at the default step, or for the second ragged variant at
    1.5 times it -- and decoded by the oracle, the padding of a ragged batch
    set to NaN in the decoded cloud (it is never read)."""
    from ndnet.packed import pack_points
    from ndnet.synthetic import make_batch
    if (j, variant) not in _packed_cache:
        pts = make_batch(_kind(j), B, N_PTS, seed0=100 * j + 7)
        pts = pts + np.float32(3.0) * np.array([j + 1, -2 * j - 1, 0.25 * j], np.float32)  # every slot its own origin
        counts = None if variant is None else _counts(j, variant)
        step = None
        if variant == 1:
            step = pack_points(pts, counts)[1][:, 3].numpy().astype(np.float64) * 1.5
        q, qp = pack_points(pts, counts, step)
        dec = R.decode(q.numpy(), qp.numpy())
        if counts is not None:
            for b in range(B):
                dec[b, counts[b]:] = np.nan
        _packed_cache[(j, variant)] = (q, qp, counts, dec)
    return _packed_cache[(j, variant)]


_ref_cache = {}


def _reference(fill, variant=None):
    """Per batch j < SLOTS: (log-probs, rows, labels) of the float32
    GraphedSegmentation on the oracle-decoded cloud, computed once and shared."""
    import torch
    from ndnet.pipeline import GraphedSegmentation
    key = (fill, variant)
    if key not in _ref_cache:
        g = GraphedSegmentation(_model(), K, B, N_PTS, point_labels=fill, ragged=variant is not None)
        assert g.points.dtype == torch.float32 and g.qparams is None
        ref = []
        for j in range(SLOTS):
            _, _, counts, dec = _packed_batch(j, variant)
            out = g(torch.from_numpy(dec).cuda(), counts)
            ref.append((out.clone(), g.point_rows.clone(), g.point_labels.clone()))
        torch.cuda.synchronize()
        _ref_cache[key] = ref
    return _ref_cache[key]


def _preconditions(ref, R_, variant=None):
    import torch
    for j in range(R_):
        a, b = _packed_batch(j, variant), _packed_batch((j + 1) % R_, variant)
        assert not torch.equal(a[1], b[1]) and not torch.equal(a[0], b[0]), j   # qparams and q differ slot to slot
        assert bool((a[1][:, 3] != b[1][:, 3]).all()) and bool((a[1][:, :3] != b[1][:, :3]).all()), j
        assert not torch.equal(ref[j][1], ref[(j + 1) % R_][1]), j
        assert not torch.equal(ref[j][0], ref[(j + 1) % R_][0]), j


def _load(pipe, variant=None):
    import torch
    for j in range(pipe.R):
        q, qp, counts, _ = _packed_batch(j, variant)
        pipe.inputs[j].copy_(q)
        pipe.qparam_bufs[j].copy_(qp)
        if counts is not None:
            pipe.count_bufs[j].copy_(torch.tensor(counts, dtype=torch.int32))


def _run_and_compare(pipe, ref, labels_of=lambda t: t):
    """R single steps, then 2 R free-running ones; every slot against the
    reference of the batch before it."""
    import torch
    R_ = pipe.R
    singles = []
    for s in range(R_):
        assert pipe.points.data_ptr() == pipe.inputs[s].data_ptr()
        assert pipe.qparams.data_ptr() == pipe.qparam_bufs[s].data_ptr()
        out = pipe.replay()
        singles.append((out.clone(), pipe.point_labels.clone()))
    torch.cuda.synchronize()
    for s in range(1, R_):  # (step 0's forward ran on the warm-up rows)
        assert torch.equal(singles[s][0], ref[s - 1][0]), f"step {s}: log-probs"
        assert torch.equal(singles[s][1], labels_of(ref[s - 1][2])), f"step {s}: labels"
    pipe.replay_steps(2 * R_)
    torch.cuda.synchronize()
    for j in range(R_):
        assert torch.equal(pipe.out[j], ref[(j - 1) % R_][0]), f"slot {j}: log-probs"
        assert torch.equal(pipe.labels[j], labels_of(ref[(j - 1) % R_][2])), f"slot {j}: labels"
        assert torch.equal(pipe.point_rows[j], ref[j][1]), f"slot {j}: rows"
    for plan in pipe.plans:
        assert all(st.rc == 0 for st in plan.host_stats())


@pytest.mark.parametrize("fill,fwd_streams,ndt_streams", [("none", 1, 1), ("nearest", 3, 2)])
def test_packed_pipeline_equals_float32_on_decoded_batches(fill, fwd_streams, ndt_streams):
    import torch
    from ndnet.pipeline import PipelinedSegmentation
    ref = _reference(fill)
    pipe = PipelinedSegmentation(_model(), K, B, N_PTS, fwd_streams=fwd_streams, ndt_streams=ndt_streams,
                                 point_labels=fill, packed=True)
    assert pipe.R <= SLOTS and len(pipe.inputs) == len(pipe.qparam_bufs) == pipe.R
    assert len(pipe._decoded) == ndt_streams and pipe.counts is None
    assert all(t.dtype == torch.int16 for t in pipe.inputs)
    assert all(t.dtype == torch.float32 and t.shape == (B, 4) for t in pipe.qparam_bufs)
    _preconditions(ref, pipe.R)
    _load(pipe)
    _run_and_compare(pipe, ref)


def test_packed_ragged_pipeline_takes_new_counts_and_qparams():
    """Counts in n / 2 .. n per cloud and slot; then the same stage graphs
    with a second set of counts, q and qparams (1.5 times the step)."""
    import torch
    from ndnet.pipeline import PipelinedSegmentation
    pipe = PipelinedSegmentation(_model(), K, B, N_PTS, fwd_streams=3, ndt_streams=2, point_labels="nearest",
                                 ragged=True, packed=True)
    for variant in (0, 1):
        ref = _reference("nearest", variant)
        _preconditions(ref, pipe.R, variant)
        _load(pipe, variant)
        _run_and_compare(pipe, ref)
        for j in range(pipe.R):  # the padding points of batch j - 1: no label
            c = _counts((j - 1) % pipe.R, variant)
            for b in range(B):
                assert bool((pipe.labels[j][b, c[b]:] == -1).all()) and bool((pipe.labels[j][b, :c[b]] >= 0).all())
    assert not torch.equal(_packed_batch(0, 0)[1], _packed_batch(0, 1)[1])
    assert not torch.equal(_reference("nearest", 0)[0][0], _reference("nearest", 1)[0][0])
    # load_resident: every slot one batch, its counts and its qparams
    q, qp, counts, _ = _packed_batch(1, 1)
    pipe.load_resident(q.cuda(), counts, qp)
    pipe.replay_steps(pipe.R + 1)
    torch.cuda.synchronize()
    for j in range(pipe.R):
        assert torch.equal(pipe.out[j], _reference("nearest", 1)[1][0]), f"resident slot {j}"
        assert torch.equal(pipe.point_rows[j], _reference("nearest", 1)[1][1]), f"resident slot {j}"
    with pytest.raises(ValueError, match="int16"):
        pipe.load_resident(torch.zeros((B, N_PTS, 3)), counts, qp)
    with pytest.raises(ValueError, match="qparams"):
        pipe.load_resident(q, counts)


def test_packed_streamed_uint8_labels():
    """The PCIe-inclusive loop: int16 batches, their counts and qparams from
    pinned host memory, every step's uint8 labels copied back."""
    import torch
    from ndnet.pipeline import PipelinedSegmentation

    def as_u8(t):
        return torch.where(t < 0, torch.full_like(t, 255), t).to(torch.uint8)

    ref = _reference("nearest", 0)
    pipe = PipelinedSegmentation(_model(), K, B, N_PTS, point_labels="nearest", ragged=True, label_dtype=torch.uint8,
                                 packed=True)
    _preconditions(ref, pipe.R, 0)
    host, counts, qps = [], [], []
    for i in range(4):
        q, qp, c, _ = _packed_batch(i, 0)
        host.append(q.clone().pin_memory())
        qps.append(qp.clone().pin_memory())
        counts.append(torch.tensor(c, dtype=torch.int32).pin_memory())
    assert host[0].dtype == torch.int16 and host[0].numel() * 2 * 2 == B * N_PTS * 3 * 4  # half the float32 bytes
    labels_host = [torch.full((B, N_PTS), 77, dtype=torch.uint8).pin_memory() for _ in range(5)]
    pipe.points.copy_(host[0])
    pipe.counts.copy_(counts[0])
    pipe.qparams.copy_(qps[0])
    outs = []
    for i in range(5):
        nxt = min(i + 1, 3)
        outs.append(pipe.replay_streamed(host[nxt], counts[nxt], labels_host[i], qps[nxt]).clone())
        pipe.labels_copied.synchronize()
        if i:
            assert torch.equal(labels_host[i], as_u8(ref[i - 1][2]).cpu()), f"streamed batch {i - 1}: labels"
    torch.cuda.synchronize()
    for i in range(4):
        assert torch.equal(outs[i + 1], ref[i][0]), f"streamed batch {i}: log-probs"
    with pytest.raises(ValueError, match="int16"):
        pipe.replay_streamed(host[0].float(), counts[0], None, qps[0])
    with pytest.raises(ValueError, match="qparams"):
        pipe.replay_streamed(host[0], counts[0])


def test_packed_levels_pipeline_equals_float32_levels():
    import torch
    from ndnet.pipeline import GraphedSegmentation, PipelinedSegmentation
    levels = (400, 200, 100)
    m = _model()
    pipe = PipelinedSegmentation(m, levels[0], B, N_PTS, levels=levels, ragged=True, packed=True)
    R_ = pipe.R
    g = GraphedSegmentation(m, levels[0], B, N_PTS, levels=levels, ragged=True)
    expect = []
    for j in range(R_):
        _, _, counts, dec = _packed_batch(j, 0)
        expect.append([o.clone() for o in g(torch.from_numpy(dec).cuda(), counts)])
    for j in range(R_):
        for lv in range(3):
            assert not torch.equal(expect[j][lv], expect[(j + 1) % R_][lv])
    _load(pipe, 0)
    for _ in range(R_):
        pipe.replay()
    pipe.replay_steps(2 * R_)
    torch.cuda.synchronize()
    for j in range(R_):
        for lv in range(3):
            assert torch.equal(pipe.out[j][lv], expect[(j - 1) % R_][lv]), f"slot {j} level {lv}"


def test_packed_graphed_equals_eager_unpack_and_segment_points():
    import torch
    from ndnet.packed import unpack
    from ndnet.pipeline import GraphedSegmentation
    from ndnet.segment import segment_points
    m = _model()
    g = GraphedSegmentation(m, K, B, N_PTS, point_labels="nearest", ragged=True, packed=True)
    assert g.points.dtype == torch.int16 and g.qparams.shape == (B, 4) and g.counts.tolist() == [N_PTS] * B
    plain = GraphedSegmentation(m, K, B, N_PTS, point_labels="nearest", packed=True)
    seen = []
    for j, variant in ((0, 0), (1, 0), (2, 1), (3, None)):
        q, qp, counts, dec = _packed_batch(j, variant)
        qd, qpd = q.cuda(), qp.cuda()
        x = unpack(qd, qpd)
        assert np.array_equal(x.cpu().numpy(), R.decode(q.numpy(), qp.numpy()))
        labels, log_probs = segment_points(m, K, x, "nearest", counts=counts)
        graph = g if variant is not None else plain
        out = graph(qd, counts, qparams=qpd) if counts is not None else graph(qd, qparams=qpd)
        torch.cuda.synchronize()
        assert torch.equal(out, log_probs), (j, variant)
        assert torch.equal(graph.point_labels, labels), (j, variant)
        seen.append(out.clone())
    assert not torch.equal(seen[0], seen[1])
    with pytest.raises(ValueError, match="int16"):
        g(torch.zeros((B, N_PTS, 3), device="cuda"), qparams=qpd)
    with pytest.raises(ValueError, match="qparams"):
        g(qd)
    with pytest.raises(ValueError, match="packed=True"):
        GraphedSegmentation(m, K, B, N_PTS)(x, qparams=qpd)
