"""ndnet_pts_unpack_i16 (include/ndnet_packed.h) against the numpy oracle
(tests/packed_ref.py), bit for bit: every n in 1..33 and 1023, 1024, 1025,
20 003, B in {1, 3}, q offset by 0..7 int16 and the output by 0..3 floats (the
16-byte groups, the misaligned heads, the tails and the 4-byte-store path),
with and without counts, between sentinel pads that must stay untouched.

The inputs hold -32768, 32767 and 0, steps 0.00313 / 0.0217 and non-zero
origins: test_packed_cpu.py checks that an fma-form decode differs from the
oracle on >= 1% of exactly these inputs."""
import numpy as np
import pytest

import packed_ref as R

pytestmark = pytest.mark.gpu

PAD = 16                  # sentinel floats on either side of every output
SENTINEL = 0x7FC0DEAD     # a NaN payload no decode produces
SMALL, LARGE = tuple(range(1, 34)), (1023, 1024, 1025, 20_003)


def _count_sets(B, n):
    """name -> counts (None: the NULL pointer); as the device reads them."""
    mixed = [0, n // 2, n][:B] if B > 1 else [0]
    sets = {"null": None, "ones": [1] * B, "full": [n] * B, "mixed": mixed,
            "over": ([n + 5, n, -3][:B] if B > 1 else [n + 5])}
    if B == 1:
        sets["half"] = [n // 2]
    return sets


def _expected(dec, counts, n):
    """The output region as uint32: the decoded points up to each (clamped)
    count, the sentinel everywhere else."""
    B = dec.shape[0]
    exp = np.full((B, n, 3), SENTINEL, np.uint32)
    for b in range(B):
        m = n if counts is None else min(max(int(counts[b]), 0), n)
        exp[b, :m] = dec[b, :m].view(np.uint32)
    return exp.reshape(-1)


def _run_shape(B, n):
    import torch
    from ndnet import _lib
    f = _lib.lib().ndnet_pts_unpack_i16
    dev = torch.device("cuda", 0)
    q, qp = R.kernel_case(B, n)
    dec = R.decode(q, qp)
    sets = _count_sets(B, n)
    E = 3 * n * B
    region = E + 2 * PAD + 4                                   # pads, and room for the float offset
    cases = [(qo, oo, name) for qo in range(8) for oo in range(4) for name in sets]
    # 16-byte aligned bases (torch's allocator gives 256): the offsets below are the misalignment
    q_dev = torch.zeros(E + 8 + 8, dtype=torch.int16, device=dev)
    out = torch.full((len(cases), region + (-region) % 4), SENTINEL, dtype=torch.int32, device=dev)
    assert q_dev.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0 and out.stride(0) % 4 == 0
    qp_dev = torch.from_numpy(qp).to(dev)
    counts_dev = {k: None if v is None else torch.tensor(v, dtype=torch.int32, device=dev) for k, v in sets.items()}
    q_flat = torch.from_numpy(q.reshape(-1)).to(dev)
    stream = _lib.stream_ptr(dev)
    last_qo = None
    for ci, (qo, oo, name) in enumerate(cases):
        if qo != last_qo:
            q_dev.zero_()
            q_dev[qo:qo + E].copy_(q_flat)
            last_qo = qo
        c = counts_dev[name]
        rc = f(q_dev.data_ptr() + 2 * qo, qp_dev.data_ptr(), B, n, c.data_ptr() if c is not None else None,
               out[ci].data_ptr() + 4 * (PAD + oo), stream)
        assert rc == 0
    got = out.cpu().numpy().view(np.uint32)
    for ci, (qo, oo, name) in enumerate(cases):
        exp = np.full(out.shape[1], SENTINEL, np.uint32)
        exp[PAD + oo:PAD + oo + E] = _expected(dec, sets[name], n)
        assert np.array_equal(got[ci], exp), (B, n, qo, oo, name, np.flatnonzero(got[ci] != exp)[:8] - PAD - oo)
    # as floats too, the full decode
    full = [ci for ci, (qo, oo, name) in enumerate(cases) if name == "null"]
    for ci in full:
        oo = cases[ci][1]
        assert np.array_equal(got[ci][PAD + oo:PAD + oo + E].view(np.float32), dec.reshape(-1))


@pytest.mark.parametrize("B", [1, 3])
def test_small_clouds_equal_the_oracle_at_every_offset(B):
    for n in SMALL:
        _run_shape(B, n)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n", LARGE)
def test_large_clouds_equal_the_oracle_at_every_offset(B, n):
    _run_shape(B, n)


def test_unpack_wrapper_counts_out_and_streams():
    """ndnet.packed.unpack: fresh and given outputs, counts as a list and as a
    device tensor, a non-default stream."""
    import torch
    from ndnet.packed import unpack
    B, n = 3, 1025
    q, qp = R.kernel_case(B, n, seed=1)
    dec = R.decode(q, qp)
    qd, qpd = torch.from_numpy(q).cuda(), torch.from_numpy(qp).cuda()
    x = unpack(qd, qpd)
    assert x.dtype == torch.float32 and x.shape == (B, n, 3)
    assert np.array_equal(x.cpu().numpy(), dec)
    counts = [1, 700, n]
    for c in (counts, torch.tensor(counts), torch.tensor(counts, device="cuda")):
        out = torch.full((B, n, 3), -7.0, device="cuda")
        assert unpack(qd, qpd, c, out=out) is out
        got = out.cpu().numpy()
        for b in range(B):
            assert np.array_equal(got[b, :counts[b]], dec[b, :counts[b]]) and (got[b, counts[b]:] == -7.0).all()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    out = torch.zeros((B, n, 3), device="cuda")
    with torch.cuda.stream(side):
        unpack(qd, qpd, out=out)
    side.synchronize()
    assert np.array_equal(out.cpu().numpy(), dec)
    with pytest.raises(ValueError, match="count"):
        unpack(qd, qpd, [1, 700, n + 1])


def test_captured_decode_follows_q_and_qparams_in_place():
    """A graph of the decode replayed after q, qparams and the counts change in
    place: nothing is baked into the capture but the pointers."""
    import torch
    from ndnet.packed import unpack
    B, n = 3, 20_003
    dev = torch.device("cuda", 0)
    qd = torch.zeros((B, n, 3), dtype=torch.int16, device=dev)
    qpd = torch.zeros((B, 4), device=dev)
    cd = torch.full((B,), n, dtype=torch.int32, device=dev)
    out = torch.full((B, n, 3), -7.0, device=dev)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        unpack(qd, qpd, cd, out=out)
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        unpack(qd, qpd, cd, out=out)
    seen = []
    for seed, counts in ((0, [n, n, n]), (1, [n, 5, n // 2]), (2, [n - 1, n, 8])):
        q, qp = R.kernel_case(B, n, seed)
        out.fill_(-7.0)
        qd.copy_(torch.from_numpy(q))
        qpd.copy_(torch.from_numpy(qp))
        cd.copy_(torch.tensor(counts, dtype=torch.int32))
        g.replay()
        got, dec = out.cpu().numpy(), R.decode(q, qp)
        for b in range(B):
            assert np.array_equal(got[b, :counts[b]], dec[b, :counts[b]]), (seed, b)
            assert (got[b, counts[b]:] == -7.0).all(), (seed, b)
        seen.append(dec)
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])
