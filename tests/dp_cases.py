"""Restatements for the differential-privacy kernels (csrc/dp.h, csrc/dp.hip; the format: include/fedfr_hip.h, "THE NOISE STREAM").

* ``philox4x32_10`` / ``words``: Philox4x32-10 in numpy integer arithmetic and the stream's indexing (key = seed halves, counter =
  (blk low, blk high, round low, stream_id), element e = lane e % 4 of block e / 4).  ``fedfr_philox_fill`` is held to ``words`` BIT FOR BIT.
* ``gauss64``: the Box-Muller formula in float64 from the exact u1, u2 of those words: what ``fedfr_gaussian_fill`` approximates in fp32.
* ``run32``: ``fedfr_dp_multi`` in float32, one operation per line, on top of tests/fedopt_cases.py, with the noise values z passed in
  (read back from ``fedfr_gaussian_fill``: the kernel is documented to add those very bits).
* ``quadrature_rdp``: the Renyi divergence of the subsampled Gaussian mechanism by direct trapezoid quadrature, against which the
  accountant's closed form is checked.

Nothing here imports the package."""
import numpy as np

import fedopt_cases as F

f32, f64, u32, u64 = np.float32, np.float64, np.uint32, np.uint64
KINDS = dict(F.KINDS, PLAIN=4)
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = u64(0xFFFFFFFF)
GRID_WRAP = F.GRID_CAP * 256 * 4 + 5        # 2 097 157: one element behind what 2048 blocks cover in one grid-stride pass
TAIL_BOUND = float(np.sqrt(48 * np.log(2)))  # |z| of u1 = 2^-24


def philox4x32_10(ctr, key):
    """ctr: four uint32 arrays (or scalars), key: two; returns the four output words as uint32 arrays"""
    c = [np.atleast_1d(np.asarray(a, dtype=u64)) & MASK for a in ctr]
    k = [np.atleast_1d(np.asarray(a, dtype=u64)) & MASK for a in key]
    for _ in range(10):
        p0, p1 = u64(M0) * c[0], u64(M1) * c[2]              # 32 x 32 -> 64 bits: exact in uint64
        c = [(p1 >> u64(32)) ^ c[1] ^ k[0], p1 & MASK, (p0 >> u64(32)) ^ c[3] ^ k[1], p0 & MASK]
        k = [(k[0] + u64(W0)) & MASK, (k[1] + u64(W1)) & MASK]
    return [a.astype(u32) for a in c]


def blocks(nblk, seed, rnd, sid, blk0):
    """[nblk, 4] words of blocks blk0 .. blk0 + nblk - 1"""
    b = np.arange(nblk, dtype=u64) + u64(blk0)
    out = philox4x32_10((b & MASK, b >> u64(32), int(rnd) & 0xFFFFFFFF, sid), (int(seed) & 0xFFFFFFFF, int(seed) >> 32))
    return np.stack(out, axis=1)


def words(n, seed, rnd, sid, offset=0):
    """what fedfr_philox_fill writes: word offset + j for j < n"""
    assert offset % 4 == 0
    return blocks((n + 3) // 4, seed, rnd, sid, offset // 4).reshape(-1)[:n]


def gauss64(n, seed, rnd, sid, offset=0):
    """the standard normal values of the stream in float64: pairs (r_a, r_b) = lanes (0, 1) and (2, 3) of every block"""
    w = blocks((n + 3) // 4, seed, rnd, sid, offset // 4).reshape(-1, 2)
    u1 = ((w[:, 0] >> u32(8)).astype(f64) + 1.0) * 2.0 ** -24
    u2 = (w[:, 1] >> u32(8)).astype(f64) * 2.0 ** -24
    rad = np.sqrt(-2.0 * np.log(u1))
    z = np.stack([rad * np.cos(2.0 * np.pi * u2), rad * np.sin(2.0 * np.pi * u2)], axis=1)
    return z.reshape(-1)[:n]


# ---- fedfr_dp_multi, float32, one operation per line ----------------------------------------------------------------------------------
def noisy_delta32(x, xs, coef, noise_std, z):
    d = F.delta32(x, xs, coef)
    if noise_std > 0:
        t = f32(noise_std) * z
        d = d + t
    assert d.dtype == f32
    return d


def step32(kind, x, m, v, d, h):
    """(m', v', x'); m' and v' are None where the kind has none"""
    if kind == "PLAIN":
        return None, None, x + d
    return F.step32(kind, x, m, v, d, h)


def run32(kind, x, xs, coef, m, v, h, noise_std, z):
    return step32(kind, x, m, v, noisy_delta32(x, xs, coef, noise_std, z), h)


def noise_std32(noise_multiplier, clip_norm, wmax):
    """fp32(noise_multiplier) * fp32(clip_norm) * fp32(max_i w_i), in that order, in fp32 (privacy.GaussianMechanism.noise_std)"""
    return (f32(noise_multiplier) * f32(clip_norm)) * f32(wmax)


# ---- the accountant's yardstick ----------------------------------------------------------------------------------------------------------
def quadrature_rdp(q, sigma, alpha, points=4_000_001):
    """D_alpha((1 - q) N(0, s^2) + q N(1, s^2) || N(0, s^2)) = log(E_{N(0, s^2)} [(1 - q + q exp((2 x - 1) / (2 s^2)))^alpha]) / (alpha - 1) by the trapezoid
    rule on [-40 s, 40 s + alpha]; the integrand is formed in logs"""
    lo, hi = -40.0 * sigma, 40.0 * sigma + alpha
    x = np.linspace(lo, hi, points)
    logp0 = -x * x / (2 * sigma * sigma) - 0.5 * np.log(2 * np.pi * sigma * sigma)
    logratio = np.logaddexp(np.log1p(-q), np.log(q) + (2 * x - 1) / (2 * sigma * sigma))
    y = np.exp(logp0 + alpha * logratio)
    integral = float(np.sum((y[1:] + y[:-1]) * 0.5)) * ((hi - lo) / (points - 1))      # (not x[1] - x[0]: that difference carries 1e-10 of cancellation)
    return np.log(integral) / (alpha - 1)


def epsilon_by_hand(q, sigma, rounds, delta, orders=range(2, 257)):
    """min over integer orders of T rdp(alpha) + log(1 / delta) / (alpha - 1), rdp by the binomial sum in plain floats (math.comb is exact)"""
    import math
    best = math.inf
    for a in orders:
        if q == 1.0:
            r = a / (2 * sigma * sigma)
        else:
            terms = [math.log(math.comb(a, i)) + (a - i) * math.log1p(-q) + (i * math.log(q) if i else 0.0) + (i * i - i) / (2 * sigma * sigma)
                     for i in range(a + 1)]
            mx = max(terms)
            r = (mx + math.log(sum(math.exp(t - mx) for t in terms))) / (a - 1)
        best = min(best, rounds * r + math.log(1 / delta) / (a - 1))
    return best
