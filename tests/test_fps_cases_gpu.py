"""k_fps at its internal boundaries (the cases of fps_cases.py, whose
preconditions test_fps_cases_cpu.py asserts on the oracle) against the numpy
oracle, through test_fps_gpu's own runner and checker: the indices equal the
oracle's, min_dist equals it bit for bit over [0, m), is untouched past m, and
the sentinel margins around both outputs are untouched."""
import numpy as np
import pytest

import fps_cases as FC
from test_fps_gpu import SENT, _bits, _check, _gpu

# (the cases are shared read-only arrays: torch.from_numpy remarks on that, and nothing writes them)
pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:The given NumPy array is not writable")]

DTYPES = list(FC.DTYPES)


def _run(case, dtype):
    return _check((case.name, dtype), case.points, case.S, case.counts, case.start)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", range(6))
def test_chunk_edges(k, dtype):
    """n at C T - 1, C T, C T + 1, C T + T, C T + T + 1 and 2 C T + 1 with the picks forced
    into the tail chunk's last slab and onto the last lane of the slab before it."""
    case = FC.chunk_edge(FC.chunk_edge_sizes(dtype)[k], dtype)
    idx, md = _run(case, dtype)
    assert set(case.marks) <= set(idx[0].tolist()) and (md[0, list(case.marks)] == -1).all()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", range(3))
def test_tier_edges_with_the_lone_point_picked(k, dtype):
    case = FC.tier_edge_marked(FC.tier_edge_sizes(dtype)[k], dtype)
    idx, md = _run(case, dtype)
    assert set(case.marks) <= set(idx[0].tolist()) and (md[0, list(case.marks)] == -1).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_spill_tier(dtype):
    """Most picks past REG_POINTS: the spill loop's picked-point arm, its unrolled body, its
    remainder slab and its partial slab all decide samples."""
    case = FC.spill(dtype)
    idx, _ = _run(case, dtype)
    assert int((idx[0] >= FC.sizes(dtype).REG).sum()) >= 32


@pytest.mark.parametrize("dtype", DTYPES)
def test_spill_tier_ragged(dtype):
    """Four workgroups of one launch that end in different tiers."""
    case = FC.spill_ragged(dtype)
    idx, _ = _run(case, dtype)
    assert idx[:, 0].tolist() == case.start
    for b, c in enumerate(case.counts):
        assert (idx[b] >= 0).all() and (idx[b] < c).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_cross_tier_ties(dtype):
    case = FC.cross_tier_ties(dtype)
    idx, md = _run(case, dtype)
    picked = set(idx[0].tolist())
    for a, b in case.pairs:
        assert a in picked and b not in picked and md[0, a] == -1 and md[0, b] == 0, (a, b)


@pytest.mark.parametrize("kind,dtype", [(k, d) for k, ds in FC.DEGENERATE.items() for d in ds])
def test_degenerate_clouds(kind, dtype):
    case = FC.degenerate(kind, dtype)
    idx, _ = _run(case, dtype)
    if kind in ("identical", "nan"):
        assert idx[0].tolist() == list(range(case.S))


@pytest.mark.parametrize("dtype", DTYPES)
def test_short_clouds_and_counts_below_one(dtype):
    """Clouds shorter than n_samples (the -1 fill's stride runs) and counts of 0 and -3, which
    the header clamps to 1: the launch with the counts and starts as given must equal, byte for
    byte, the launch with them clamped on the host, which _check holds against the oracle (its
    m is then 1 for those clouds: min_dist[1:] stays untouched)."""
    case = FC.short(dtype)
    B = len(case.counts)
    m, s = zip(*(FC.effective(case, b) for b in range(B)))
    assert min(case.counts) < 1 and min(m) == 1
    idx, md = _check((case.name, dtype), case.points, case.S, list(m), list(s))
    raw_idx, raw_md = _gpu(case.points, case.S, case.counts, case.start)
    assert np.array_equal(raw_idx, idx) and np.array_equal(_bits(raw_md), _bits(md))
    for b in range(B):
        assert (idx[b, m[b]:] == -1).all() and (idx[b, :min(m[b], case.S)] >= 0).all()
        assert (raw_md[b, m[b]:] == SENT).all()
    assert [int((idx[b] == -1).sum()) for b in range(B)] == [800, 1499, 0, 0, 1499, 1499]


@pytest.mark.parametrize("dtype", DTYPES)
def test_more_clouds_than_compute_units(dtype):
    import torch
    case = FC.many_clouds(dtype)
    assert len(case.counts) > torch.cuda.get_device_properties(0).multi_processor_count
    idx, _ = _run(case, dtype)
    assert idx[:, 0].tolist() == case.start and (idx >= 0).all()
