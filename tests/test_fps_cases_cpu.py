"""The cases of fps_cases.py are what they claim to be, on the numpy oracle
alone: the oracle agrees with plain loops where a cloud is small enough, and
every precondition that makes the matching GPU test (test_fps_cases_gpu.py)
meaningful holds -- every marked point is picked, of every duplicate pair the
smaller index and never the larger, the spill case picks mostly in the spill
tier, the short clouds leave the stated numbers of -1.  These are conditions
on the inputs: if a later change to a header constant breaks one, this file
says so instead of the GPU test going quiet."""
import numpy as np
import pytest

import fps_cases as FC
from fps_ref import fps_loops, fps_ref

DTYPES = list(FC.DTYPES)


def _oracle(case, b=0):
    m, s = FC.effective(case, b)
    return fps_ref(case.points[b], case.S, m, s)


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint8), b[1].view(np.uint8))


def test_header_constants_and_sizes():
    import test_fps_gpu
    assert FC.header_constants() == test_fps_gpu._header_constants()
    assert {"THREADS", "LDS_POINTS_F32", "LDS_POINTS_F64", "REG_POINTS_F32", "REG_POINTS_F64", "CHUNK_SLABS_F32",
            "CHUNK_SLABS_F64"} <= set(FC.H)
    for dtype in DTYPES:
        z = FC.sizes(dtype)
        # what the kernel's static_asserts require, and what the cases' geometry assumes
        assert z.REG % (z.C * z.T) == 0 and z.LDS % z.T == 0 and z.T % 64 == 0
        assert 2 * z.C * z.T + 1 < z.LDS < z.REG and z.T > 64 and z.C >= 2
        assert len(set(FC.chunk_edge_sizes(dtype))) == 6
        n = FC.spill_size(dtype)
        assert (n - z.REG) // z.T == 5 and (n - z.REG) % z.T == 3
        for a, b in FC.tie_pairs(dtype):
            assert 0 < a < b < n


def test_builders_are_seeded_and_read_only():
    a = FC.chunk_edge(FC.chunk_edge_sizes("float32")[0], "float32")
    FC.chunk_edge.cache_clear()
    b = FC.chunk_edge(FC.chunk_edge_sizes("float32")[0], "float32")
    assert a.points is not b.points and np.array_equal(a.points, b.points) and a.marks == b.marks
    with pytest.raises(ValueError):
        a.points[0, 0, 0] = 1.0
    f32, f64 = FC.many_clouds("float32"), FC.many_clouds("float64")
    assert f32.points.dtype == np.float32 and f64.points.dtype == np.float64 and f32.counts == f64.counts


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", range(6))
def test_chunk_edge_marks_are_picked(k, dtype):
    n = FC.chunk_edge_sizes(dtype)[k]
    case = FC.chunk_edge(n, dtype)
    z = FC.sizes(dtype)
    assert case.points.shape == (1, n, 3) and n - 1 in case.marks and 2 <= len(case.marks) <= 3
    # the marks sit in the last slab and on the last lane of the slab before it
    assert {i // z.T for i in case.marks} == {(n - 1) // z.T, (n - 1) // z.T - 1}
    idx, _ = _oracle(case)
    assert set(case.marks) <= set(idx.tolist())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", range(3))
def test_tier_edge_marks_are_picked(k, dtype):
    n = FC.tier_edge_sizes(dtype)[k]
    case = FC.tier_edge_marked(n, dtype)
    assert case.points.shape == (1, n, 3) and case.marks == (n - 2, n - 1)
    idx, _ = _oracle(case)
    assert set(case.marks) <= set(idx.tolist())


@pytest.mark.parametrize("dtype", DTYPES)
def test_spill_picks_mostly_in_the_spill_tier(dtype):
    z = FC.sizes(dtype)
    case = FC.spill(dtype)
    n = case.points.shape[1]
    idx, _ = _oracle(case)
    in_spill = int((idx >= z.REG).sum())
    print(f"spill {dtype}: {in_spill} of {case.S} picks at indices >= REG")
    assert idx[0] == n - 2 and in_spill >= 32
    # the picks reach the unrolled slabs, the remainder slab and the partial slab
    slabs = {(int(i) - z.REG) // z.T for i in idx if i >= z.REG}
    assert slabs == set(range(6))


@pytest.mark.parametrize("dtype", DTYPES)
def test_spill_ragged_ends_in_four_places(dtype):
    z = FC.sizes(dtype)
    case = FC.spill_ragged(dtype)
    n = case.points.shape[1]
    assert case.counts == [n, z.REG + 1, z.REG, z.REG - z.T + 1] and case.start == [n - 2, z.REG, 0, 5]
    base = FC.spill(dtype).points[0]
    for b, c in enumerate(case.counts):
        assert np.array_equal(case.points[b, :c], base[:c]) and np.isnan(case.points[b, c:]).all()
        idx, _ = _oracle(case, b)
        assert idx[0] == case.start[b] and (idx >= 0).all() and (idx < c).all()
    assert np.array_equal(_oracle(case, 0)[0], _oracle(FC.spill(dtype))[0])


@pytest.mark.parametrize("dtype", DTYPES)
def test_cross_tier_ties_pick_the_smaller_index(dtype):
    case = FC.cross_tier_ties(dtype)
    assert len(case.pairs) == 8
    idx, mind = _oracle(case)
    picked = set(idx.tolist())
    for a, b in case.pairs:
        assert np.array_equal(case.points[0, a], case.points[0, b])
        assert a in picked and b not in picked, (a, b)
        assert mind[a] == -1 and mind[b] == 0
        # both members tied exactly on the trip that took a: the larger index was as far
        t = idx.tolist().index(a)
        _, before = fps_ref(case.points[0], t)
        assert before[a] == before[b] == before.max() and int(np.argmax(before)) == a


@pytest.mark.parametrize("kind,dtype", [(k, d) for k, ds in FC.DEGENERATE.items() for d in ds])
def test_degenerate_oracle_agrees_with_loops(kind, dtype):
    case = FC.degenerate(kind, dtype)
    assert case.points.shape == (1, 1500, 3) and case.S == 600 and case.points.dtype == np.dtype(dtype)
    got = _oracle(case)
    assert _same(got, fps_loops(case.points[0], case.S))
    idx, mind = got
    if kind in ("identical", "nan"):
        assert idx.tolist() == list(range(600))
        assert (mind[:600] == -1).all() and (mind[600:] == (0 if kind == "identical" else np.inf)).all()
    elif kind == "overflow":
        assert set(np.abs(case.points).ravel().tolist()) == {float(np.float32(1e20))}
        assert set(mind.tolist()) <= {-1.0, 0.0, float("inf")} and len(set(idx.tolist())) == 600
    else:
        rest = np.delete(mind, idx)
        assert (rest > 0).all() and (rest < 3).all() and len(set(idx.tolist())) == 600


@pytest.mark.parametrize("dtype", DTYPES)
def test_short_clouds_leave_the_stated_fill(dtype):
    case = FC.short(dtype)
    assert case.points.shape == (6, 2000, 3) and case.S == 1500
    assert [FC.effective(case, b) for b in range(6)] == [(700, 0), (1, 0), (1500, 1499), (2000, 5), (1, 0), (1, 0)]
    fill = []
    for b in range(6):
        m, s = FC.effective(case, b)
        got = _oracle(case, b)
        if m <= 700:
            assert _same(got, fps_loops(case.points[b], case.S, m, s))
        idx, mind = got
        fill.append(int((idx == -1).sum()))
        assert idx[0] == s and (idx[:min(m, case.S)] >= 0).all() and (idx[m:] == -1).all() and len(mind) == m
    assert fill == [800, 1499, 0, 0, 1499, 1499]
    assert np.isnan(case.points[4, 0]).all() and np.isnan(case.points[5, 0]).all()  # the point that is read


@pytest.mark.parametrize("dtype", DTYPES)
def test_many_clouds_oracle_agrees_with_loops(dtype):
    case = FC.many_clouds(dtype)
    B = len(case.counts)
    assert case.points.shape == (300, 100, 3) and case.S == 16
    assert min(case.counts) == 16 and max(case.counts) == 100 and len(set(case.counts)) > 50
    assert len({case.points[b, :16].tobytes() for b in range(B)}) == B  # every cloud different
    for b in range(B):
        m, s = FC.effective(case, b)
        assert (m, s) == (case.counts[b], case.start[b]) and np.isnan(case.points[b, m:]).all()
        got = _oracle(case, b)
        assert _same(got, fps_loops(case.points[b], case.S, m, s))
        assert got[0][0] == s and len(set(got[0].tolist())) == 16 and (got[0] < m).all()
