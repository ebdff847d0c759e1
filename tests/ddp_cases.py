"""Restatements for the distributed-DP kernels (csrc/ddp.h, csrc/ddp.hip; the format: include/fedfr_hip.h, "THE DISCRETE NOISE STREAM").

* ``attempt`` / ``sample``: the discrete Gaussian sampler in numpy float64, one operation per line in the order of ``dgauss_attempt``, on
  the Philox words of tests/dp_cases.py (block (offset + e) * 64 + a for attempt a of element e).  ``fedfr_dgauss_fill`` is held to
  ``sample`` BIT FOR BIT, with ONE accepted deviation: ``log`` and ``exp`` are the device library's there and numpy's here, and the two may
  differ in the last place.  ``sample`` therefore also says, per element, whether any decision it took was AMBIGUOUS:
    floor    -t log(U1) lies within 64 ulp of an integer;
    accept   |U2 - p| <= 64 ulp(p).
  A test asserts that no element of its inputs is ambiguous (a property of its seeds, checked on the CPU too) and then exact equality.
* ``pmf`` / ``chi2_cells``: the exact probability mass function exp(-y^2 / 2 sigma^2) / Z and the cells of the goodness-of-fit test.
* ``clip_factor``: min(1, C / ||xi - x||) in float64 from the float32 differences, rounded to float32 once (fedfr_fedopt_sqnorm, k = 1,
  w = 1).  The device sums the squares in another order, so its factor may differ by an ulp: the SECOND accepted deviation (a test then
  feeds the device's own factor to ``mask_dp_u32`` and holds the factor itself to 2 ulp).
* ``mask_dp_u32``: ``fedfr_secagg_mask_dp``: secagg_cases.encode32 at coef = factor 2^f, the exact sum of the squared codes mod 2^64, the
  noise of the stream (seed, round, NOISE_STREAM) and secagg_cases.stream_sum, mod 2^32.

Nothing here imports the package."""
import math

import numpy as np

import dp_cases as D
import secagg_cases as S

f32, f64, u32, u64, i32, i64 = np.float32, np.float64, np.uint32, np.uint64, np.int32, np.int64
ATTEMPTS = 64
NOISE_STREAM = 0x44444750                    # "DDGP": the stream_id of the clients' noise shares
SIGMA_MIN, SIGMA_MAX = 16.0, 2.0 ** 26
TAIL = 37                                    # |Y| <= TAIL t: U1 >= 2^-53 and 53 ln 2 = 36.74
AMBIGUOUS_ULPS = 64.0


def params(sigma):
    """(t, s2t, c) as the host forms them: t = floor(sigma) + 1, s2t = (sigma sigma) / t, c = -1 / (2 (sigma sigma))"""
    sigma = f64(sigma)
    t = np.floor(sigma) + f64(1.0)
    s2 = sigma * sigma
    return t, s2 / t, f64(-1.0) / (f64(2.0) * s2)


def attempt(w, sigma):
    """w: [m, 4] uint32 words -> (accepted [m] bool, value [m] int64, ambiguous [m] bool)"""
    t, s2t, c = params(sigma)
    w0, w1, w2, w3 = (w[:, q].astype(u64) for q in range(4))
    m1 = (w0 << u64(21)) | (w1 >> u64(11))
    m2 = (w2 << u64(21)) | (w3 >> u64(11))
    u1 = (m1 + u64(1)).astype(f64) * f64(2.0 ** -53)      # exact: an integer <= 2^53 times a power of two
    u2 = m2.astype(f64) * f64(2.0 ** -53)
    neg = (w1 & u64(1)) != 0
    prod = -t * np.log(u1)
    g = np.floor(prod)
    d = g - s2t
    dd = d * d
    p = np.exp(dd * c)
    accepted = ~(neg & (g == 0)) & (u2 < p)
    value = np.where(neg, -g, g).astype(i64)
    ambiguous = (np.abs(prod - np.rint(prod)) <= AMBIGUOUS_ULPS * np.spacing(np.abs(prod))) | (np.abs(u2 - p) <= AMBIGUOUS_ULPS * np.spacing(p))
    return accepted, value, ambiguous


def sample(n, seed, rnd, sid, offset, sigma):
    """(values [n] int64, attempts [n] (0 = exhausted), ambiguous [n] bool, exhausted count): element j is element offset + j of the stream"""
    assert SIGMA_MIN <= sigma <= SIGMA_MAX and offset + n <= 2 ** 58
    values, attempts, ambiguous = np.zeros(n, i64), np.zeros(n, np.int32), np.zeros(n, bool)
    pending = np.arange(n)
    for a in range(ATTEMPTS):
        if pending.size == 0:
            break
        blk = (pending.astype(u64) + u64(offset)) * u64(ATTEMPTS) + u64(a)
        w = np.stack(D.philox4x32_10((blk & D.MASK, blk >> u64(32), int(rnd) & 0xFFFFFFFF, sid), (int(seed) & 0xFFFFFFFF, int(seed) >> 32)), axis=1)
        ok, val, amb = attempt(w, sigma)
        ambiguous[pending] |= amb
        values[pending[ok]], attempts[pending[ok]] = val[ok], a + 1
        pending = pending[~ok]
    return values, attempts, ambiguous, int(pending.size)


def as_u32(values):
    """int64 values as the uint32 words the kernels write (mod 2^32)"""
    return (values & i64(0xFFFFFFFF)).astype(u32)


# ---- the target -------------------------------------------------------------------------------------------------------------------------
def pmf(sigma, half_width=None):
    """(support y = -W ... W, P(y)) of N_Z(0, sigma^2), W = ceil(12 sigma) by default (the mass beyond is below 1e-31)"""
    W = int(math.ceil(12 * sigma)) if half_width is None else int(half_width)
    y = np.arange(-W, W + 1, dtype=f64)
    p = np.exp(-y * y / (2.0 * f64(sigma) ** 2))
    return y.astype(i64), p / p.sum()


def pmf_moments(sigma):
    """(variance, fourth central moment) of N_Z(0, sigma^2) from the pmf (the mean is 0 by symmetry)"""
    y, p = pmf(sigma)
    yf = y.astype(f64)
    return float(np.sum(p * yf ** 2)), float(np.sum(p * yf ** 4))


def chi2_cells(sigma, cells=None):
    """Upper edges (inclusive, ascending integers) of the cells of the goodness-of-fit test and their probabilities.  ``cells`` None: one
    cell per integer |y| <= 4 sigma and ONE tail cell (both tails together, index -1).  Otherwise ``cells`` equal-probability cells over
    the integers, cut at the quantiles of the pmf (a cell is never empty of mass)."""
    y, p = pmf(sigma)
    if cells is None:
        W = int(math.floor(4 * sigma))
        inside = np.abs(y) <= W
        return y[inside], np.concatenate([p[inside], [p[~inside].sum()]])
    cdf = np.cumsum(p)
    cut = np.searchsorted(cdf, np.arange(1, cells) / float(cells))      # index of the last integer of each cell but the last
    edges = np.concatenate([y[cut], [y[-1]]])
    prob = np.diff(np.concatenate([[0.0], cdf[cut], [1.0]]))
    return edges, prob


def chi2(values, sigma, cells=None):
    """(chi-square statistic, degrees of freedom) of ``values`` against the pmf"""
    edges, prob = chi2_cells(sigma, cells)
    if cells is None:
        W = int(edges[-1])
        inside = np.abs(values) <= W
        obs = np.concatenate([np.bincount((values[inside] + W).astype(i64), minlength=2 * W + 1), [np.count_nonzero(~inside)]])
    else:
        obs = np.bincount(np.searchsorted(edges, values, side="left"), minlength=cells)
        assert obs.size == cells, "a value beyond 12 sigma"
    exp = prob * values.size
    return float(np.sum((obs - exp) ** 2 / exp)), prob.size - 1


# ---- fedfr_secagg_mask_dp ---------------------------------------------------------------------------------------------------------------
def clip_factor(x, xi, clip):
    """fp32(min(1, clip / ||xi - x||)): fp32 differences, fp64 squares and sum, as fedfr_fedopt_sqnorm with k = 1, w = 1.  A norm that is
    0 or NaN leaves the factor at 1, an infinite one gives 0 (the kernel's own cases)"""
    with np.errstate(over="ignore", invalid="ignore"):
        d = (xi - x).astype(f64)
        s = float(np.sum(d * d))
    c = 1.0
    if clip > 0 and s > 0.0:
        r = float(f32(clip)) / math.sqrt(s)
        c = c * (r if r < 1.0 else 1.0)
    return f32(c)


def mask_dp_u32(x, xi, factor, frac_bits, limit, seed, rnd, offset, sigma, streams):
    """(y as uint32, sum of the squared codes mod 2^64 as a Python int, (saturated, nonfinite, exhausted), ambiguous [n] bool)"""
    coef = f32(factor) * f32(2.0 ** frac_bits)
    assert coef.dtype == f32
    q, sat, bad = S.encode32(x, xi, coef, limit)
    sq = _sq_mod64(q)
    noise, _, amb, exhausted = sample(q.size, seed, rnd, NOISE_STREAM, offset, sigma)
    with np.errstate(over="ignore"):
        y = q.view(u32) + as_u32(noise) + S.stream_sum(q.size, streams)
    return y, sq, (sat, bad, exhausted), amb


# ---- the inputs of the GPU tests: stated here so that tests/test_ddp_cpu.py can hold their seeds to "no ambiguous decision" too ------------
FILL_SEED, FILL_ROUND = 0x1234567890ABCDEF, 3
FILL_SIGMAS = (16.0, 1000.5, 2.0 ** 18.3)
FILL_SIZES = S.SMALL_SIZES + (1 << 16,)
FILL_OFFSET = (1 << 40) + 7                  # a non-zero offset whose block index (offset + e) * 64 needs the high counter word
MASK_SEED, MASK_ROUND, MASK_SIGMA, MASK_FRAC = 0x0FEDCBA987654321, 5, 100.25, 24
MASK_SIZES = (5, 16, 17, 4100)
MASK_LIMIT = S.code_limit(8) - TAIL * (int(MASK_SIGMA) + 1)      # L' of K = 8 at MASK_SIGMA
MASK_KINDS = ("planted", "binds", "free")


def mask_inputs(n, kind):
    """(x, xi, clip, limit) float32 inputs of one mask_dp case:
    planted   secagg_cases.planted_inputs at coef 2^24: elements that saturate at both ends, a NaN, +-inf, rounding ties.  The norm is NaN,
              which leaves the clip factor at 1 (the kernel's own case): nothing is clipped and the clamp L' does the work
    binds     ordinary updates and one large element; ||xi - x|| is about 0.5 and clip = 0.25, so the factor is about 0.5; the limit is
              2^21, which the large element (0.25 2^24 after the clip) passes: it saturates
    free      ordinary updates of norm about 1e-3 sqrt(n) under clip = 10: the factor is exactly 1"""
    if kind == "planted":
        x, xi = S.planted_inputs(n, f32(2.0 ** MASK_FRAC), MASK_LIMIT)
        return x, xi, 1.0, MASK_LIMIT
    g = np.random.default_rng(1000 + n)
    x = (g.standard_normal(n) * 0.05).astype(f32)
    xi = (x + g.standard_normal(n).astype(f32) * f32(1e-3)).astype(f32)
    if kind == "binds":
        xi[1] = x[1] + f32(0.5)
        return x, xi, 0.25, 1 << 21
    assert kind == "free"
    return x, xi, 10.0, MASK_LIMIT


def _sq_mod64(q):
    """sum q^2 mod 2^64 for a long vector: q^2 < 2^62 is exact in uint64, and uint64 addition wraps"""
    q2 = q.astype(i64) * q.astype(i64)
    with np.errstate(over="ignore"):
        return int(np.sum(q2.astype(u64), dtype=u64))
