"""PipelinedSegmentation with point_labels / ragged / label_dtype: every step's
log-probs and per-point labels, single-step and free-running, are bit-equal to
the one-graph-per-batch path (GraphedSegmentation(point_labels=, ragged=)) on
the batch before it.

Every ring slot holds a different batch (U and L clouds in turn, distinct
seeds), and every test first checks that consecutive batches' rows differ and
that an L batch leaves >= 1% of its real points without a row under
fill="none": with those, rows of the wrong batch (taken after the plan moved
on, or routed through the wrong slot) cannot pass.  n = 20 003 leaves the
n % 8 tail's 3 points per cloud to the fill."""
import numpy as np
import pytest

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


def _batch(j, n=N_PTS):
    from ndnet.synthetic import make_batch
    return make_batch(_kind(j), B, n, seed0=100 * j + 7)


def _counts(j, variant=0):
    """Counts in n / 2 .. n for slot j: a cloud at n, one with count % 8 != 0."""
    rng = np.random.default_rng(50 * j + variant)
    c = rng.integers(N_PTS // 2, N_PTS + 1, B)
    c[(j + variant) % B] = N_PTS
    c[(j + variant + 1) % B] = N_PTS // 2 + 3 + 8 * j + 16 * variant  # 10 004 + a multiple of 8: % 8 = 4
    assert any(int(x) % 8 for x in c)
    return [int(x) for x in c]


def _ragged_batch(j, variant=0):
    pts, c = _batch(j), _counts(j, variant)
    for b in range(B):
        pts[b, c[b]:] = np.nan
    return pts, c


_cache = {}


def _reference(fill, ragged_variant=None):
    """Per batch j < SLOTS: (log-probs, rows, labels) of the graphed path,
    computed once per (fill, counts) and shared."""
    import torch
    from ndnet.pipeline import GraphedSegmentation
    key = (fill, ragged_variant)
    if key not in _cache:
        g = GraphedSegmentation(_model(), K, B, N_PTS, point_labels=fill, ragged=ragged_variant is not None)
        ref = []
        for j in range(SLOTS):
            if ragged_variant is None:
                out = g(torch.from_numpy(_batch(j)).cuda())
            else:
                pts, c = _ragged_batch(j, ragged_variant)
                out = g(torch.from_numpy(pts).cuda(), c)
            ref.append((out.clone(), g.point_rows.clone(), g.point_labels.clone()))
        torch.cuda.synchronize()
        _cache[key] = ref
    return _cache[key]


def _preconditions(ref, R, ragged_variant=None):
    """Stale or misrouted rows must show: consecutive batches' rows (and
    labels) differ, and an L batch has >= 1% of its real points at -1 under
    fill="none"."""
    import torch
    for j in range(R):
        assert not torch.equal(ref[j][1], ref[(j + 1) % R][1]), j
        assert not torch.equal(ref[j][2], ref[(j + 1) % R][2]), j
    none = _reference("none", ragged_variant)
    worst = 0.0
    for j in range(R):
        if _kind(j) != "L":
            continue
        real = sum(_counts(j, ragged_variant)) if ragged_variant is not None else B * N_PTS
        unassigned = int((none[j][1] < 0).sum()) - (B * N_PTS - real)  # the padding is at -1 too
        worst = max(worst, unassigned / real)
    assert worst >= 0.01, worst


def _load(pipe, variant=None):
    import torch
    for j in range(pipe.R):
        if variant is None:
            pipe.inputs[j].copy_(torch.from_numpy(_batch(j)))
        else:
            pts, c = _ragged_batch(j, variant)
            pipe.inputs[j].copy_(torch.from_numpy(pts))
            pipe.count_bufs[j].copy_(torch.tensor(c, dtype=torch.int32))


def _run_and_compare(pipe, ref, labels_of=lambda t: t):
    """R single steps, then 2 R free-running ones; every slot against the
    reference of the batch before it."""
    import torch
    R = pipe.R
    singles = []
    for s in range(R):
        out = pipe.replay()
        assert pipe.point_labels.data_ptr() == pipe.labels[s].data_ptr()
        singles.append((out.clone(), pipe.point_labels.clone()))
    torch.cuda.synchronize()
    for s in range(1, R):  # (step 0's forward ran on the warm-up rows)
        assert torch.equal(singles[s][0], ref[s - 1][0]), f"step {s}: log-probs"
        assert torch.equal(singles[s][1], labels_of(ref[s - 1][2])), f"step {s}: labels"
    last = pipe.replay_steps(2 * R)
    torch.cuda.synchronize()
    assert last.data_ptr() == pipe.out[R - 1].data_ptr()
    for j in range(R):
        assert torch.equal(pipe.out[j], ref[(j - 1) % R][0]), f"slot {j}: log-probs"
        assert torch.equal(pipe.labels[j], labels_of(ref[(j - 1) % R][2])), f"slot {j}: labels"
        assert torch.equal(pipe.point_rows[j], ref[j][1]), f"slot {j}: rows"
    for plan in pipe.plans:
        assert all(st.rc == 0 for st in plan.host_stats())


@pytest.mark.parametrize("fwd_streams,ndt_streams", [(1, 1), (3, 2)])
@pytest.mark.parametrize("fill", ["none", "nearest"])
def test_labels_and_log_probs_equal_graphed_batches(fill, fwd_streams, ndt_streams):
    from ndnet.pipeline import PipelinedSegmentation
    ref = _reference(fill)
    pipe = PipelinedSegmentation(_model(), K, B, N_PTS, fwd_streams=fwd_streams, ndt_streams=ndt_streams,
                                 point_labels=fill)
    assert pipe.R <= SLOTS and len(pipe.labels) == len(pipe.point_rows) == pipe.R and pipe.counts is None
    _preconditions(ref, pipe.R)
    _load(pipe)
    _run_and_compare(pipe, ref)
    if fill == "none":
        assert any(int((lb < 0).sum()) for lb in pipe.labels)


@pytest.mark.parametrize("fill,fwd_streams,ndt_streams", [("none", 1, 1), ("nearest", 3, 2)])
def test_ragged_labels_equal_graphed_ragged_batches(fill, fwd_streams, ndt_streams):
    """Counts in n / 2 .. n per cloud and slot, NaN padding; then the same stage
    graphs with a second set of counts."""
    import torch
    from ndnet.pipeline import PipelinedSegmentation
    pipe = PipelinedSegmentation(_model(), K, B, N_PTS, fwd_streams=fwd_streams, ndt_streams=ndt_streams,
                                 point_labels=fill, ragged=True)
    assert [c.tolist() for c in pipe.count_bufs] == [[N_PTS] * B] * pipe.R
    assert pipe.counts.data_ptr() == pipe.count_bufs[0].data_ptr()
    for variant in (0, 1):
        ref = _reference(fill, variant)
        _preconditions(ref, pipe.R, variant)
        _load(pipe, variant)
        _run_and_compare(pipe, ref)
        for j in range(pipe.R):  # the padding points of batch j - 1: no label
            c = _counts((j - 1) % pipe.R, variant)
            for b in range(B):
                assert bool((pipe.labels[j][b, c[b]:] == -1).all())
                if fill == "nearest":
                    assert bool((pipe.labels[j][b, :c[b]] >= 0).all())
    assert not torch.equal(_reference(fill, 0)[0][2], _reference(fill, 1)[0][2])
    with pytest.raises(ValueError, match="count"):
        pipe.load_resident(pipe.inputs[0], [N_PTS + 1] * B)
    with pytest.raises(ValueError, match="shape"):
        pipe.load_resident(pipe.inputs[0], [N_PTS] * (B + 1))


def test_ragged_levels_equal_graphed_ragged_levels():
    import torch
    from ndnet.pipeline import GraphedSegmentation, PipelinedSegmentation
    levels = (400, 200, 100)
    m = _model()
    pipe = PipelinedSegmentation(m, levels[0], B, N_PTS, levels=levels, ragged=True)
    assert pipe.labels is None and pipe.point_rows is None
    R = pipe.R
    g = GraphedSegmentation(m, levels[0], B, N_PTS, levels=levels, ragged=True)
    expect = []
    for j in range(R):
        pts, c = _ragged_batch(j)
        expect.append([o.clone() for o in g(torch.from_numpy(pts).cuda(), c)])
    for j in range(R):
        for lv in range(3):
            assert not torch.equal(expect[j][lv], expect[(j + 1) % R][lv])
    _load(pipe, 0)
    for _ in range(R):
        pipe.replay()
    pipe.replay_steps(2 * R)
    torch.cuda.synchronize()
    for j in range(R):
        for lv in range(3):
            assert torch.equal(pipe.out[j][lv], expect[(j - 1) % R][lv]), f"slot {j} level {lv}"
    # load_resident fills every slot with one batch and its counts
    pts, c = _ragged_batch(1)
    pipe.load_resident(torch.from_numpy(pts).cuda(), c)
    pipe.replay_steps(R + 1)
    torch.cuda.synchronize()
    for j in range(R):
        for lv in range(3):
            assert torch.equal(pipe.out[j][lv], expect[1][lv]), f"resident slot {j} level {lv}"


def test_uint8_labels_resident_and_streamed():
    """label_dtype=torch.uint8: the int32 pipeline's labels with 255 for -1;
    then the PCIe-inclusive loop over 4 ragged host batches, every step's
    labels copied to pinned memory beside the compute."""
    import torch
    from ndnet.pipeline import PipelinedSegmentation

    def as_u8(t):
        return torch.where(t < 0, torch.full_like(t, 255), t).to(torch.uint8)

    ref = _reference("nearest", 0)
    m = _model()
    p32 = PipelinedSegmentation(m, K, B, N_PTS, point_labels="nearest", ragged=True)
    p8 = PipelinedSegmentation(m, K, B, N_PTS, point_labels="nearest", ragged=True, label_dtype=torch.uint8)
    R = p8.R
    _preconditions(ref, R, 0)
    assert p8.labels[0].dtype == torch.uint8 and p32.labels[0].dtype == torch.int32
    for pipe in (p32, p8):
        _load(pipe, 0)
    _run_and_compare(p32, ref)
    _run_and_compare(p8, ref, labels_of=as_u8)
    for j in range(R):
        assert torch.equal(p8.labels[j], as_u8(p32.labels[j])), j
        assert bool((p8.labels[j] == 255).any())  # the padding
        assert torch.equal(p8.out[j], p32.out[j])
    # streamed: replay i runs batch i and streams batch i + 1 in; its labels are batch i - 1's
    host, counts = [], []
    for i in range(4):
        pts, c = _ragged_batch(i)
        host.append(torch.from_numpy(pts).pin_memory())
        counts.append(torch.tensor(c, dtype=torch.int32).pin_memory())
    labels_host = [torch.full((B, N_PTS), 77, dtype=torch.uint8).pin_memory() for _ in range(5)]
    p8.points.copy_(host[0])
    p8.counts.copy_(counts[0])
    outs = []
    for i in range(5):
        nxt = min(i + 1, 3)
        outs.append(p8.replay_streamed(host[nxt], counts[nxt], labels_host[i]).clone())
        p8.labels_copied.synchronize()
        if i:
            assert torch.equal(labels_host[i], as_u8(ref[i - 1][2]).cpu()), f"streamed batch {i - 1}: labels"
    torch.cuda.synchronize()
    for i in range(4):
        assert torch.equal(outs[i + 1], ref[i][0]), f"streamed batch {i}: log-probs"
    with pytest.raises(ValueError, match="count"):
        p8.replay_streamed(host[0], torch.zeros(B, dtype=torch.int32))
    with pytest.raises(ValueError, match="pinned"):
        p8.replay_streamed(host[0], labels_host=torch.zeros((B, N_PTS), dtype=torch.int32).pin_memory())


def test_defaults_build_no_label_ring():
    """The arguments at their defaults: the pipeline as it was."""
    import torch
    from ndnet.pipeline import GraphedSegmentation, PipelinedSegmentation
    from ndnet.synthetic import make_batch
    n = 20_000
    m = _model()
    pipe = PipelinedSegmentation(m, K, B, n)
    assert pipe.labels is None and pipe.point_rows is None and pipe.point_labels is None
    assert pipe.counts is None and pipe.count_bufs is None and pipe.labels_copied is None
    R = pipe.R
    batches = [torch.from_numpy(make_batch(_kind(j), B, n, seed0=100 * j + 7)).cuda() for j in range(R)]
    g = GraphedSegmentation(m, K, B, n)
    expect = [g(b).clone() for b in batches]
    for j in range(R):
        pipe.inputs[j].copy_(batches[j])
    for _ in range(R):
        pipe.replay()
    pipe.replay_steps(2 * R)
    torch.cuda.synchronize()
    for j in range(R):
        assert torch.equal(pipe.out[j], expect[(j - 1) % R]), f"slot {j}"
    with pytest.raises(ValueError, match="ragged"):
        pipe.load_resident(batches[0], [n] * B)
    with pytest.raises(ValueError, match="point_labels"):
        pipe.replay_streamed(batches[0].cpu().pin_memory(),
                             labels_host=torch.zeros((B, n), dtype=torch.int32).pin_memory())
