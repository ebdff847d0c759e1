"""Inputs and references for the robust-aggregation kernels (csrc/robust.hip: robust_trimmed_mean_kernel, robust_pairdist_kernel,
robust_krum_select_kernel).  The formulas are the ones include/fedfr_hip.h states for fedfr_robust_trimmed_mean / _pairdist / _krum_select.

* ``trimmed32``: a numpy float32 restatement of the trimmed mean.  ORDER: a stable argsort on the uint32 key of every value (``key``: bits u
  of a non-NaN value -> u ^ (sign ? 0xFFFFFFFF : 0x80000000); every NaN -> 0xFFFFFFFF, so NaN sorts last and -0 < +0).  ARITHMETIC: the kept
  values s_b .. s_{k-1-b} are added in ascending order starting from s_b, one float32 addition per line, then ONE float32 division by
  float32(kept count).  numpy's float32 + and / are single correctly rounded IEEE operations, as the kernel's are, so the kernel is held
  to this BIT FOR BIT (NaN where this is NaN).
* ``pairdist64``: D[i][j] = sum_e (double) (x_i[e] - x_j[e] in float32)^2, numpy's fp64 dot product.  The terms are exact (a float32 squared has 48
  bits) and non-negative, so ANY summation order of n of them is within (n - 1) 2^-53 (relative) of the exact sum; two orders differ by at
  most twice that: ``pairdist_bound`` = n 2^-52 D.
* ``krum_ref``: Krum / Multi-Krum scores and selection from a distance matrix.

Nothing here imports the package.
"""
import functools

import numpy as np

f32, f64 = np.float32, np.float64
GRID_CAP = 2048                     # the launchers' grid cap (fedavg_multi's rule)
SIZES = (1, 3, 4, 5, 1023, 4103, GRID_CAP * 256 * 4 + 5)      # tail only, below / at / above one float4, around one block, grid-stride wrap + tail
BIG = SIZES[-1]
KS_TRIM = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32)
KS_TRIM_BIG = (3, 8, 17)            # the k the largest n runs at
KS_DIST = (2, 3, 8, 9, 16, 32)
MAX_K = 32
U = 2.0 ** -24                      # fp32 unit roundoff


def grid(n):
    """blocks of 256 threads the launchers use for n elements: min(ceil((n / 4 + 1) / 256), 2048)"""
    return min((n // 4 + 1 + 255) // 256, GRID_CAP)


def trims(k):
    """the b of the tests: 0, 1 and the median's (k - 1) // 2, where 2 b < k"""
    return sorted({b for b in (0, 1, (k - 1) // 2) if 2 * b < k})


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def key(a):
    """the uint32 sort key of float32 values: a total order on bit patterns, every NaN last"""
    u = bits(np.asarray(a, dtype=f32))
    k = u ^ np.where(u >> 31 != 0, np.uint32(0xFFFFFFFF), np.uint32(0x80000000))
    return np.where((u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000), np.uint32(0xFFFFFFFF), k).astype(np.uint32)


def _freeze(arrays):
    for a in arrays:
        a.flags.writeable = False
    return tuple(arrays)


@functools.lru_cache(maxsize=8)
def inputs(n, k, tag=0.0):
    """closed-form client states x_0 .. x_{k-1}: one sine base plus a per-client sine whose amplitude grows with the client index (so the
    pairwise distances, and with them the Krum scores, are well separated).  Computed once per argument set, shared, read-only."""
    j = np.arange(n, dtype=f64)
    base = 0.5 * np.sin(0.37 * j + 0.1 + tag)
    return _freeze([(base + 0.02 * (1.0 + 0.25 * i) * np.sin(0.091 * (i + 1) * j + 0.5 * i + 0.3 + tag)).astype(f32) for i in range(k)])


@functools.lru_cache(maxsize=8)
def spiked(n, k):
    """``inputs`` with the spikes a robust rule exists for (k >= 5): client 0 is all NaN (both signs, two payloads), client 1 is +-inf,
    client 2 is +-1e30; at every coordinate j % 3 == 1 the remaining clients are EXACTLY equal, at j % 3 == 2 they hold only +-0 in signs
    that differ from client to client and coordinate to coordinate."""
    assert k >= 5
    xs = [a.copy() for a in inputs(n, k)]
    j = np.arange(n)
    nan = np.array([0x7FC00000, 0xFFC00001, 0x7F800001], dtype=np.uint32).view(f32)
    xs[0][:] = nan[j % 3]
    xs[1][:] = np.where(j % 2 == 0, np.inf, -np.inf).astype(f32)
    xs[2][:] = np.where((j // 2) % 2 == 0, 1e30, -1e30).astype(f32)
    for i in range(3, k):
        xs[i][j % 3 == 1] = xs[3][j % 3 == 1]
        z = np.where((i * (j + 1) + j // 3) % 2 == 0, f32(0.0), f32(-0.0)).astype(f32)
        xs[i][j % 3 == 2] = z[j % 3 == 2]
    return _freeze(xs)


@functools.lru_cache(maxsize=8)
def signed_zeros(n, k):
    """every client holds only +-0, in mixed signs: coordinates with all -0, all +0 and every mixture occur"""
    j = np.arange(n)
    return _freeze([np.where((j >> (i % 8)) % 2 == 0, f32(-0.0), f32(0.0)).astype(f32) for i in range(k)])      # (j % 256 == 0: all -0)


_SORTED = []                        # [(the arrays themselves, their sorted stack)]: the last few, so that every b of a case shares one sort


def _sorted(xs):
    for held, S in _SORTED:
        if len(held) == len(xs) and all(a is b for a, b in zip(held, xs)):
            return S
    X = np.stack(xs)
    order = np.argsort(key(X), axis=0, kind="stable")
    S = np.take_along_axis(X, order, axis=0)
    S.flags.writeable = False
    if all(not a.flags.writeable for a in xs):      # (only arrays that cannot change under the cache)
        _SORTED.append((tuple(xs), S))
        del _SORTED[:-3]
    return S


def trimmed32(xs, b, b_hi=None):
    """the float32 restatement: drop the b smallest and b_hi (default b) largest values of every coordinate, add the rest in ascending order
    (one float32 addition per line, starting from the first kept value), divide once by float32(kept count)"""
    k = len(xs)
    b_hi = b if b_hi is None else b_hi
    assert b >= 0 and b_hi >= 0 and b + b_hi < k
    S = _sorted(tuple(xs))
    assert S.dtype == f32
    with np.errstate(invalid="ignore", over="ignore"):
        acc = S[b].copy()
        for j in range(b + 1, k - b_hi):
            acc = acc + S[j]
        out = acc / f32(k - b - b_hi)
    assert out.dtype == f32
    return out


def trimmed64(xs, b):
    """(mean of the kept values, sum of their magnitudes) in fp64, for finite inputs"""
    S = np.sort(np.stack(xs).astype(f64), axis=0)
    kept = S[b:len(xs) - b]
    return kept.sum(axis=0) / (len(xs) - 2 * b), np.abs(kept).sum(axis=0)


def same_bits_or_nan(got, ref):
    """indices at which ``got`` is neither bit-equal to ``ref`` nor NaN where ``ref`` is NaN"""
    ok = (bits(got) == bits(ref)) | (np.isnan(got) & np.isnan(ref))
    return np.flatnonzero(~ok)


# ---- pairwise distances and Krum -----------------------------------------------------------------------------------------------------------
def pairdist64(xs):
    k = len(xs)
    D = np.zeros((k, k), dtype=f64)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(k):
            for j in range(i + 1, k):
                d = (xs[i] - xs[j]).astype(f64)
                D[i, j] = D[j, i] = np.dot(d, d)
    return D


def pairdist_bound(n, D):
    return n * 2.0 ** -52 * D


def krum_ref(D, f, m):
    """(score [k] fp64, selected [k] int32 0/1): score_i = the k - f - 2 smallest D[i][j], j != i, added in ascending order (a distance that is
    not finite counts as +inf); the m lowest scores are selected, ties to the lower index"""
    k = D.shape[0]
    assert k >= 2 * f + 3 and 1 <= m <= k - f
    E = np.where(np.isfinite(D), D, np.inf)
    score = np.zeros(k, dtype=f64)
    for i in range(k):
        row = np.sort(np.delete(E[i], i))
        s = f64(0.0)
        for v in row[:k - f - 2]:
            s = s + v
        score[i] = s
    order = sorted(range(k), key=lambda i: (score[i], i))
    sel = np.zeros(k, dtype=np.int32)
    sel[order[:m]] = 1
    return score, sel


# (n, k, f, m) of the selection tests on ``krum_inputs``: Krum and Multi-Krum, one and two launches' worth of clients, a tiled k
KRUM_CASES = ((4103, 5, 1, 1), (4103, 5, 1, 4), (1023, 8, 2, 6), (4103, 9, 3, 1), (4103, 16, 3, 13), (1023, 32, 7, 25), (BIG, 8, 2, 6))


@functools.lru_cache(maxsize=8)
def krum_inputs(n, k, f):
    """``inputs`` whose LAST f clients are planted outliers: one +-1e30, the others the honest state plus an offset of 3 + i"""
    xs = [a.copy() for a in inputs(n, k)]
    j = np.arange(n)
    for i in range(k - f, k):
        if i == k - 1:
            xs[i][:] = np.where(j % 2 == 0, 1e30, -1e30).astype(f32)
        else:
            xs[i][:] = (xs[i].astype(f64) + 3.0 + i).astype(f32)
    return _freeze(xs)


def score_gap(score, m):
    """(gap between the m-th and (m+1)-th lowest score, the (m+1)-th lowest score)"""
    s = np.sort(score)
    return (s[m] - s[m - 1], s[m]) if m < len(s) else (np.inf, np.inf)
