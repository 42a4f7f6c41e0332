"""Seeded case generators for the per-function tests of the NDT device
arithmetic (csrc/ndt_device.h, csrc/ndt_log.h): tests/test_ndt_device_cpu.py
shows with the oracle alone that each corpus reaches the branches it is meant
to reach, tests/test_ndt_device_gpu.py runs the device functions on it.

The generators are numpy on the host; the references at the end call the
CPU oracle.  Results are cached, shared by the tests and read-only.
"""
import ctypes
import functools

import numpy as np

from test_ndt_gpu import _lu_cases

KEY_INVALID = 0xFFFFFFFF  # voxel_key / orc_voxel_keys: out of grid
KEY_REDO = 0xFFFFFFFE     # voxel_key_f32: left to the double path
WAVE = 64

LOG_TAB_LO, LOG_TAB_HI = 91, 181  # NDNET_LOG_TAB_LO / _HI (csrc/ndt_log_table.h)
LOG_SPLIT_MANT = 0x6A09E667F3BCD  # ndnet_log's sqrt(2) split of the mantissa


def _ro(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


def _from_bits(b):
    return np.asarray(b, dtype=np.uint64).view(np.float64)


def _step_ulps(x, k):
    """x moved by k units in the last place (finite positive x, small k)."""
    return (np.asarray(x, np.float64).view(np.int64) + np.int64(k)).view(np.float64)


# --------------------------------------------------------------------- log

@functools.lru_cache(maxsize=None)
def log_cases(seed=3):
    """~20k inputs of ndnet_log: the mixture of test_portable_log_correctly_rounded,
    both sides of every table-index boundary (idx +- 0.5) / 128 within 2 ulp at
    several exponents, the sqrt(2) split mantissa and its neighbours, all-ones
    and all-zero mantissas at every exponent, subnormals down to 5e-324, and
    the specials (+-0, negatives, +inf, NaN) at the end."""
    rng = np.random.default_rng(seed)
    parts = [np.exp(rng.uniform(-700, 700, 6000)), rng.uniform(0.5, 2.0, 6000), 1 + rng.normal(0, 1e-9, 1000),
             np.array([1.0, 2.0, 0.5, 1e-310, 5e-324, 1.7976931348623157e308])]
    edges = np.array([(i + h) / 128.0 for i in range(LOG_TAB_LO, LOG_TAB_HI + 1) for h in (-0.5, 0.5)])
    near = np.concatenate([_step_ulps(edges, k) for k in (-2, -1, 0, 1, 2)])
    for e in (0, 1, -1, 37, -500, 1000, -1021):
        parts.append(np.ldexp(near, e))
    parts.append(np.ldexp(near, -1060))  # subnormal after scaling: the e == 0 branch, then the table edge
    exps = np.array([1, 2, 400, 1022, 1023, 1024, 1500, 2045, 2046], np.uint64)
    for dm in (-1, 0, 1):
        parts.append(_from_bits((exps << np.uint64(52)) | np.uint64(LOG_SPLIT_MANT + dm)))
    all_e = np.arange(1, 2047, dtype=np.uint64) << np.uint64(52)
    parts.append(_from_bits(all_e))                                   # all-zero mantissas
    parts.append(_from_bits(all_e | np.uint64(0x000FFFFFFFFFFFFF)))   # all-ones mantissas
    k = np.arange(0, 52, dtype=np.uint64)
    sub = np.concatenate([np.uint64(1) << k, (np.uint64(1) << (k + np.uint64(1))) - np.uint64(1),
                          np.array([1, 2, 3, LOG_SPLIT_MANT - 1, LOG_SPLIT_MANT, LOG_SPLIT_MANT + 1], np.uint64),
                          rng.integers(1, 1 << 52, 600, dtype=np.uint64)])
    parts.append(_from_bits(sub))
    parts.append(np.array([0.0, -0.0, -1.0, -5e-324, -1e300, -np.inf, np.inf, np.nan]))
    return _ro(np.concatenate(parts))


def log_positive_finite(x):
    """Mask of the inputs a decimal reference can take: 0 < x < inf."""
    return (x > 0) & np.isfinite(x)


# ---------------------------------------------------------------- KL pairs

def _spd(rng, n):
    a = rng.normal(size=(n, 3, 3))
    return a @ a.transpose(0, 2, 1)


def _sample_cov(rng, m, lattice):
    """Population covariance of m samples (rank <= m - 1: near-singular for m <= 3)."""
    x = rng.integers(-300, 301, size=(m, 3)).astype(np.float64) / 128.0 if lattice else rng.normal(size=(m, 3))
    d = x - x.mean(axis=0)
    return d.T @ d / m


@functools.lru_cache(maxsize=None)
def kl_pair_cases(seed=5):
    """(P [n][9], Q [n][9]): matrix pairs for one KL event each.  Every family
    of _lu_cases on both sides and against itself; diagonal and block-diagonal
    covariances (an axis-aligned lattice cloud's), with entries exactly 1 and
    exact zeros; covariances of 2..5 samples; scales 1e-150..1e150 per side,
    so the determinant ratio under- and overflows and goes subnormal; a
    negative determinant on one side or both; an infinite entry at each
    position of Q, P or both; -0.0 entries."""
    rng = np.random.default_rng(seed)
    A = _lu_cases(seed).reshape(-1, 3, 3)
    P, Q = [], []

    def add(p, q):
        P.append(np.asarray(p, np.float64).reshape(-1, 3, 3))
        Q.append(np.asarray(q, np.float64).reshape(-1, 3, 3))

    add(A, A[rng.permutation(len(A))])   # every family against every other
    add(A[::4], A[::4])                  # P = Q
    # diagonal covariances: lattice variances (k / 128^2 multiples), some entries exactly 1, some 0
    d = rng.integers(1, 4000, size=(600, 3)).astype(np.float64) / 16384.0
    d[rng.random((600, 3)) < 0.15] = 1.0
    d[rng.random((600, 3)) < 0.04] = 0.0
    D = np.zeros((600, 3, 3))
    D[:, [0, 1, 2], [0, 1, 2]] = d
    D[::3, 0, 1] = -0.0
    D[1::3, 2, 0] = -0.0
    add(D, D[rng.permutation(600)])
    add(D[:150], D[:150])
    add(D[150:450], _spd(rng, 300))
    add(_spd(rng, 300), D[150:450])
    # one zero off-diagonal block: a 2x2 covariance and a lone axis, in each of the three arrangements
    B = np.zeros((600, 3, 3))
    for i in range(600):
        lone = i % 3
        pair = [a for a in range(3) if a != lone]
        x = rng.integers(-200, 201, size=(rng.integers(3, 9), 2)).astype(np.float64) / 128.0
        c = (x - x.mean(axis=0)).T @ (x - x.mean(axis=0)) / len(x)
        B[i][np.ix_(pair, pair)] = c
        B[i, lone, lone] = 1.0 if i % 5 == 0 else rng.integers(1, 4000) / 16384.0
    add(B, B[rng.permutation(600)])
    add(B[:300], _spd(rng, 300))
    add(_spd(rng, 300), B[300:])
    # covariances of 2..5 samples
    few = np.array([_sample_cov(rng, 2 + i % 4, i % 2 == 0) for i in range(800)])
    add(few, few[rng.permutation(800)])
    add(few[:400], _spd(rng, 400))
    add(_spd(rng, 400), few[400:])
    # scales per side
    ea, eb = rng.uniform(-150, 150, 1500), rng.uniform(-150, 150, 1500)
    add(_spd(rng, 1500) * (10.0 ** ea)[:, None, None], _spd(rng, 1500) * (10.0 ** eb)[:, None, None])
    eq = rng.uniform(-80, -25, 200)      # det_q / det_p ~ 1e-315: subnormal
    add(_spd(rng, 200) * (10.0 ** (eq + 105))[:, None, None], _spd(rng, 200) * (10.0 ** eq)[:, None, None])
    # negative determinants: one row negated on P, on Q, on both
    neg = np.diag([1.0, 1.0, -1.0])
    s1, s2 = _spd(rng, 300), _spd(rng, 300)
    add(neg @ s1[:100], s2[:100])
    add(s1[100:200], neg @ s2[100:200])
    add(neg @ s1[200:], neg @ s2[200:])
    # an infinite entry at each position (U gets an infinite diagonal, the inverse an exact 0)
    for pos in range(9):
        r, c = divmod(pos, 3)
        g, h = _spd(rng, 60), _spd(rng, 60)
        gi, hi = g.copy(), h.copy()
        gi[:, r, c] = np.inf
        hi[:, r, c] = np.inf
        hi[::2, r, c] = -np.inf
        add(g[:20], hi[:20])       # Q alone
        add(gi[20:40], hi[20:40])  # both: an inf in P next to a zero of the inverse
        add(gi[40:], h[40:])       # P alone
    # -0.0 entries
    z = rng.normal(size=(300, 3, 3))
    z[rng.random((300, 3, 3)) < 0.25] = -0.0
    add(z, z[rng.permutation(300)])
    add(z[:100], _spd(rng, 100))
    P = np.concatenate(P).reshape(-1, 9)
    Q = np.concatenate(Q).reshape(-1, 9)
    return _ro(P), _ro(Q)


# -------------------------------------------------------------- voxel keys

def _bisection_midpoints(count):
    lo, hi, out = 0.01, 30.0, []
    for i in range(count):  # the search's own midpoints, halving downwards then upwards
        mid = (lo + hi) / 2
        out.append(mid)
        if i % 3 == 2:
            lo = mid
        else:
            hi = mid
    return out


def voxel_grids():
    """(off[3] float-exact, len[3] <= 64, vs) of every test grid."""
    f = lambda *v: np.array([float(np.float32(x)) for x in v])  # noqa: E731
    mids = _bisection_midpoints(5)
    return [
        (f(0.0, 0.0, 0.0), (64, 64, 64), 0.25),
        (f(-8.0, -8.0, -8.0), (64, 17, 33), 0.25),
        (f(-3.25, 1.1, -0.3), (64, 63, 7), 0.01),
        (f(-71.3, -0.007, 12.6), (33, 64, 1), 0.1),
        (f(5.7, -2.9, -100.1), (19, 2, 64), 0.3),
        (f(-1.05, -41.0, 0.6), (64, 64, 5), 1.0 / 3.0),
        (f(999999.9, -2.5, 17.0), (64, 3, 40), 30.0),
        (f(-17.2, 3.3, -0.9), (11, 64, 29), mids[0]),
        (f(0.37, -55.5, 2.2), (64, 23, 31), mids[1]),
        (f(-0.11, 0.93, -7.7), (47, 5, 64), mids[3]),
        (f(2.6, -2.6, 0.05), (64, 64, 64), mids[4]),
    ]


def _axis_boundaries(off, ln, vs, f32):
    """(coordinates, kind) on one axis: kind 0 = an in-range multiple or its
    neighbours, 1 = the far face and past it, 2 = below off / huge / special
    (the double run only).  For the float run every value is rounded to
    float32 and the neighbours are float32 neighbours."""
    ft = np.float32 if f32 else np.float64
    m = np.arange(ln + 1, dtype=np.float64)
    mul = (off + m * vs).astype(ft)
    rep = np.empty(ln + 1)
    c = off
    for i in range(ln + 1):
        rep[i] = c
        c = c + vs
    rep = rep.astype(ft)
    face = ft(off + ln * vs)
    vals = [mul, rep, np.nextafter(mul, ft(-np.inf)), np.nextafter(mul, ft(np.inf)), np.full(4, off, ft)]
    kinds = [np.where(m < ln, 0, 1)] * 4 + [np.zeros(4, int)]
    far = np.array([face, np.nextafter(face, ft(np.inf)), np.nextafter(face, ft(-np.inf)), face + ft(vs),
                    face * ft(1 + 1e-6) + ft(1e-6), off + (ln + 0.5) * vs, off + 1000.0 * vs], ft)
    vals.append(far)
    kinds.append(np.ones(len(far), int))
    if not f32:
        low = np.array([off - vs, np.nextafter(off, -np.inf), off - 0.5 * vs, off - (2.0 ** 31 + 1) * vs,
                        off - 2.0 ** 32 * vs, off - 2.0 ** 31 * vs, off - (2.0 ** 32 - 1) * vs,
                        off + 2.0 ** 63 * vs, off + 2.0 ** 64 * vs, off - 2.0 ** 63 * vs, off - 2.0 ** 64 * vs,
                        off + 2.0 ** 31 * vs, off + 2.0 ** 32 * vs, off + (2.0 ** 32 + 1) * vs,
                        1e300, -1e300, np.inf, -np.inf, np.nan])
        vals.append(low)
        kinds.append(np.full(len(low), 2))
    else:  # huge and special values a float point can hold (none below off)
        big = np.array([off + 2.0 ** 31 * vs, off + 2.0 ** 63 * vs, off + 2.0 ** 64 * vs, 3e38, np.inf, np.nan], ft)
        vals.append(big)
        kinds.append(np.full(len(big), 2))
    v = np.concatenate(vals).astype(np.float64)
    k = np.concatenate(kinds)
    if f32:  # (rounding to float32 is monotone and off is a float, so only nextafter can go below off)
        keep = ~(v < off)
        v, k = v[keep], k[keep]
    return v, k


def _voxel_points(rng, off, ln, vs, f32):
    """Random and boundary points of one grid; boundary points have the case
    on one axis and random in-grid coordinates on the others."""
    def rand(n):
        p = off + rng.random((n, 3)) * (np.array(ln) * vs)
        return p.astype(np.float32).astype(np.float64) if f32 else p

    bnd, kind = [], []
    for a in range(3):
        with np.errstate(over="ignore"):
            v, k = _axis_boundaries(off[a], ln[a], vs, f32)
        p = rand(len(v))
        p[:, a] = v
        bnd.append(p)
        kind.append(k)
    return rand, np.concatenate(bnd), np.concatenate(kind)


def _waves(rng, rand, bnd, kind):
    """Order the points wave by wave of 64: all-random waves, all-boundary
    waves, then waves with a single boundary case in lane 0, 63 or 31.
    Returns (points, family) with family -1 = random, else the boundary kind."""
    order = rng.permutation(len(bnd))
    bnd, kind = bnd[order], kind[order]
    pts, fam = [rand(8 * WAVE)], [np.full(8 * WAVE, -1)]
    full = max(0, (len(bnd) - 48) // WAVE) * WAVE  # whole all-boundary waves; the other 48 .. 111 one to a wave
    pts.append(bnd[:full])
    fam.append(kind[:full])
    for j, i in enumerate(range(full, len(bnd))):
        w = rand(WAVE)
        f = np.full(WAVE, -1)
        lane = (0, 63, 31)[j % 3]
        w[lane] = bnd[i]
        f[lane] = kind[i]
        pts.append(w)
        fam.append(f)
    pts.append(rand(4 * WAVE + 37))  # all-random again, and a ragged last wave
    fam.append(np.full(4 * WAVE + 37, -1))
    return np.concatenate(pts), np.concatenate(fam)


@functools.lru_cache(maxsize=None)
def voxel_cases(seed=7):
    """Per grid: dict(off, len, vs, points [n][3] float64, family [n],
    f32 [n]).  The first part of `points` is the double run (random doubles,
    every boundary family, points below off, huge magnitudes, inf, NaN); the
    second, flagged f32, the same families in float32 (rounded, with float32
    neighbours) without the below-off ones: where the float screen's
    preconditions hold.  family is
    -1 for a random point, 0 / 1 / 2 for a boundary point (in-range multiple /
    far face / below-off, huge or special)."""
    out = []
    for g, (off, ln, vs) in enumerate(voxel_grids()):
        rng = np.random.default_rng([seed, g])
        parts, fams, f32s = [], [], []
        for f32 in (False, True):
            rand, bnd, kind = _voxel_points(rng, off, ln, vs, f32)
            p, f = _waves(rng, rand, bnd, kind)
            pad = (-len(p)) % WAVE  # the float run starts on a wave of its own
            if pad and not f32:
                p, f = np.concatenate([p, rand(pad)]), np.concatenate([f, np.full(pad, -1)])
            parts.append(p)
            fams.append(f)
            f32s.append(np.full(len(p), f32))
        out.append(dict(off=_ro(off), len=tuple(ln), vs=float(vs), points=_ro(np.concatenate(parts)),
                        family=_ro(np.concatenate(fams)), f32=_ro(np.concatenate(f32s))))
    return tuple(out)


def f32_screen_decided(points, off, ln, vs):
    """The definition of voxel_key_f32's screen (csrc/ndt_device.h) in numpy
    float32: True where every axis has |frac(q) - 1/2| < half_tol."""
    off32 = off.astype(np.float32)
    inv32 = np.float32(1.0 / vs)
    half_tol = np.float32(0.5) - np.float32(max(ln)) * np.float32(2.0 ** -19)
    q = (points.astype(np.float32) - off32) * inv32
    assert q.dtype == np.float32
    return (np.abs(q - np.floor(q) - np.float32(0.5)) < half_tol).all(axis=1)


# ---------------------------------------------------------------- division

DIV_HARD = slice(1 << 16, (1 << 16) + 40000)  # where div_cases puts the midpoint cases


def _div_midpoint_cases(rng, pow2):
    """(m, n): 53-bit integers m and odd counts n whose quotient, scaled into
    [2^52, 2^53), lies 1 / (2 n) from the midpoint of two doubles: the
    hardest roundings a division by n has."""
    count = DIV_HARD.stop - DIV_HARD.start
    ns = [int(v) for v in pow2 if v % 2 == 1 and v > 1]
    ms, out_n, tries = [], [], 0
    while len(ms) < count:
        tries += 1  # (a draw whose range [lo, hi) holds no m of the residue is dropped)
        n = ns[(tries // 4) % len(ns)] if tries % 4 == 0 else int(rng.integers(1, 1 << 21)) * 2 + 1
        a = n.bit_length() - int(rng.integers(0, 2))  # Q = m 2^a / n
        lo = max(1 << 52, -((-(n << 52)) >> a))        # Q >= 2^52
        hi = min(1 << 53, -((-(n << 53)) >> a))        # Q < 2^53
        res = ((n + int(rng.choice((-1, 1)))) // 2) * pow(2, -a, n) % n  # m 2^a = (n +- 1) / 2 (mod n)
        m = lo + (res - lo) % n
        m += n * int(rng.integers(0, max(1, (hi - m + n - 1) // n)))
        if lo <= m < hi:
            ms.append(m)
            out_n.append(n)
    return np.array(ms, np.uint64), np.array(out_n, np.uint64)


@functools.lru_cache(maxsize=None)
def div_cases(seed=11):
    """(t float64 [N], n uint32 [N]), N ~ 10^6: counts 1 .. 2^22 and the powers
    of two up to 2^31 with their neighbours; t of both signs with exponents
    over the whole range div_fast admits (2^-969 < |t| < 2^900), mantissas
    random, few-bit and next to a power of two; t = +-0; t an exact multiple
    of n; and in DIV_HARD quotients next to a rounding midpoint."""
    rng = np.random.default_rng(seed)
    N = 1 << 20
    pow2 = np.array(sorted({max(1, (1 << k) + d) for k in range(32) for d in (-1, 0, 1)}), np.uint64)
    n = rng.integers(1, (1 << 22) + 1, N, dtype=np.uint64)
    sel = rng.random(N) < 0.25
    n[sel] = pow2[rng.integers(0, len(pow2), sel.sum())]
    n[:len(pow2)] = pow2
    n[len(pow2):len(pow2) + 4096] = np.arange(1, 4097)
    kind = rng.integers(0, 8, N)
    mant = rng.integers(0, 1 << 52, N, dtype=np.uint64)                                     # random
    few = (rng.integers(0, 1 << 16, N, dtype=np.uint64) | np.uint64(1)).astype(np.float64)  # few significant bits
    few = (np.frexp(few)[0] * 2).view(np.uint64) & np.uint64((1 << 52) - 1)
    mant = np.where(kind == 0, few, mant)
    mant = np.where(kind == 1, rng.integers(0, 16, N, dtype=np.uint64), mant)               # just above 2^e
    mant = np.where(kind == 2, np.uint64((1 << 52) - 1) - rng.integers(0, 16, N, dtype=np.uint64), mant)  # just below
    e = rng.integers(-968, 900, N)  # 2^e <= |t| < 2^(e+1)
    e[:64] = -968
    e[64:128] = 899
    t = np.ldexp(_from_bits(mant | np.uint64(0x3FF0000000000000)), e)
    mult = kind == 3  # exact multiples of n, scaled by a power of two
    m = rng.integers(1, 1 << 21, N).astype(np.float64)
    t = np.where(mult, np.ldexp(m * n.astype(np.float64), rng.integers(-900, 840, N)), t)
    hm, hn = _div_midpoint_cases(rng, pow2)
    hs = DIV_HARD
    n[hs] = hn
    t[hs] = np.ldexp(hm.astype(np.float64), rng.integers(-968 - 52, 899 - 52, len(hm)))
    t = np.where(rng.random(N) < 0.5, -t, t)
    t[-2000:-1000] = 0.0
    t[-1000:] = -0.0
    assert (np.abs(t[t != 0]) > 2.0 ** -969).all() and (np.abs(t) < 2.0 ** 900).all()
    return _ro(t), _ro(n.astype(np.uint32))


# -------------------------------------------------------------------- keys

@functools.lru_cache(maxsize=None)
def key_cases(seed=13):
    """Doubles without NaN: the log corpus, both zeros, the smallest and
    largest subnormal and normal of each sign, +-inf, duplicates, and a few
    thousand random bit patterns."""
    rng = np.random.default_rng(seed)
    x = log_cases()
    ext = _from_bits(np.array([0x1, 0x000FFFFFFFFFFFFF, 0x0010000000000000, 0x7FEFFFFFFFFFFFFF], np.uint64))
    bits = rng.integers(0, 1 << 64, 6000, dtype=np.uint64)
    r = _from_bits(bits)
    allv = np.concatenate([x, -x, ext, -ext, [0.0, -0.0, np.inf, -np.inf], [0.0, -0.0, 1.5, 1.5, -1.5, -0.0, 0.0], r])
    return _ro(allv[~np.isnan(allv)])


# ------------------------------------------------- references (the oracle)

def ref_log(x):
    import oracle as O
    y = np.zeros(len(x))
    O.lib().orc_portable_log_many(O._ptr(np.ascontiguousarray(x)), O._ptr(y), ctypes.c_uint64(len(x)))
    return y


@functools.lru_cache(maxsize=None)
def ref_log_cases():
    return _ro(ref_log(log_cases()))


@functools.lru_cache(maxsize=None)
def ref_kl_pairs():
    """(score [n], flag [n], inv [n][9]) of kl_pair_cases by orc_kl_pairs."""
    import oracle as O
    P, Q = kl_pair_cases()
    n = len(P)
    score, flag, inv = np.zeros(n), np.zeros(n, np.uint32), np.zeros((n, 9))
    O.lib().orc_kl_pairs(O._ptr(P), O._ptr(Q), ctypes.c_uint64(n), O._ptr(score), O._ptr(flag), O._ptr(inv))
    return _ro(score), _ro(flag), _ro(inv)


def ref_lu(A):
    """(LU [n][9], perm [n][3], signum [n]) of one gsl_linalg_LU_decomp each (orc_lu_chain, one step)."""
    import oracle as O
    n = len(A)
    st, ps, fl = np.zeros((n, 1, 9)), np.zeros((n, 1), np.uint32), np.zeros((n, 1), np.uint32)
    O.lib().orc_lu_chain(O._ptr(np.ascontiguousarray(A)), ctypes.c_uint64(n), ctypes.c_int(1), O._ptr(st), O._ptr(ps),
                         O._ptr(fl))
    ps = ps[:, 0]
    perm = np.stack([ps & 3, (ps >> 2) & 3, (ps >> 4) & 3], axis=1)
    return st[:, 0], perm, np.where(ps & 0x100, -1, 1)


def ref_voxel_keys(case):
    import oracle as O
    pts = case["points"]
    key = np.zeros(len(pts), np.uint32)
    ln = np.array(case["len"], np.int32)
    O.lib().orc_voxel_keys(O._ptr(pts), ctypes.c_uint64(len(pts)), O._ptr(case["off"]), O._ptr(ln),
                           ctypes.c_double(case["vs"]), O._ptr(key))
    return key


@functools.lru_cache(maxsize=None)
def ref_voxel_cases():
    return tuple(_ro(ref_voxel_keys(c)) for c in voxel_cases())
