"""References for the clip and the Gaussian mechanism on compressed and top-k uploads (csrc/compress.hip: delta_sqnorm_kernel,
delta_aggregate_dp_kernel; csrc/sparse.hip: sparse_sqnorm_kernel, sparse_aggregate_dp_kernel; the formats: include/fedfr_hip.h), on top of
the restatements that exist (compress_cases, sparse_cases, dp_cases, fedopt_cases).

* ``delta_terms`` / ``delta_sqnorm``: per block of 32 elements S_b = sum q^2 as an integer and T_b = S_b 4^(eb - 127) as the fp64 number
  it is EXACTLY (``math.ldexp`` of an integer below 2^20: no rounding; ``t_b_exact`` states the same in Python integers and Fractions);
  the squared norm is ``math.fsum`` of those: the correctly rounded sum, whatever the order.
* ``sparse_sqnorm``: ``math.fsum`` of float(val)^2, each square exact in fp64 (48 significant bits, exponent range of fp32 doubled).
* ``violations``: entries whose index is >= n or not above the entry before.
* ``tolerance(B)`` = B 2^-52, relative: B - 1 fp64 additions of non-negative terms are off by at most (B - 1) 2^-53 relative to the sum
  whatever their order (each addition rounds a partial sum that is at most the total), so the tolerance leaves a factor two.
* ``delta_dp`` / ``sparse_dp`` / the ``*_chained_dp``: the existing aggregates with ws := the coefficients the device formed, then
  s + fp32(noise_std) z before the base, z passed in (read back from fedfr_gaussian_fill, as tests/test_dp_gpu.py feeds its restatement).

Nothing here imports the package."""
import math
from fractions import Fraction

import numpy as np

import compress_cases as Q
import sparse_cases as S

f32, f64 = np.float32, np.float64
WS = [f32(w) for w in (0.21, 0.07, 0.13, 0.09, 0.17, 0.11, 0.08, 0.14)]
SEED, ROUND, SID = 987 | 654 << 32, 5, 3
NOISE_STD = f32(0.0125)


def tolerance(terms):
    return max(int(terms), 1) * 2.0 ** -52


def t_b_exact(s_b, eb):
    """S_b 4^(eb - 127) as a Fraction, from Python integers"""
    return Fraction(int(s_b)) * Fraction(4) ** (int(eb) - 127)


def t_b_fp64(s_b, eb):
    """the same as the kernel forms it: double(S_b) times the fp64 power of four (both factors exact, so is the product if the claim holds)"""
    return float(int(s_b)) * math.ldexp(1.0, 2 * (int(eb) - 127))


def delta_terms(codes, scales, bits, n):
    """(T_b as fp64 [blocks], any scale byte 255) of one upload; elements at index >= n are not counted (``unpack`` drops them)"""
    q = Q.unpack(codes, bits, n).astype(np.int64)
    nb = Q.scale_bytes(n)
    pad = np.zeros(nb * Q.BLOCK, dtype=np.int64)
    pad[:n] = q * q
    s_b = pad.reshape(nb, Q.BLOCK).sum(axis=1)                    # integers: exact
    eb = np.asarray(scales[:nb], dtype=np.int64)
    assert s_b.max(initial=0) <= 32 * 128 * 128
    t = np.ldexp(s_b.astype(f64), 2 * (np.minimum(eb, 254) - 127))      # exact: a 20-bit integer times 2^-254 .. 2^254
    return t, bool(np.any(eb == 255))


def delta_sqnorm(codes, scales, bits, n):
    """the correctly rounded squared norm of the dequantised upload; NaN if a block carries the reserved scale byte"""
    t, bad = delta_terms(codes, scales, bits, n)
    return float("nan") if bad else math.fsum(t.tolist())


def sparse_sqnorm(val):
    v = np.asarray(val, dtype=f32).astype(f64)
    return math.fsum((v * v).tolist())


def violations(idx, n):
    i = np.asarray(idx).astype(np.int64)
    bad = i >= n
    bad[1:] |= i[1:] <= i[:-1]
    return int(bad.sum())


def rel_err(got, ref):
    if ref == 0.0:
        return 0.0 if got == 0.0 else math.inf
    return abs(got - ref) / ref


# ---- made-up uploads -----------------------------------------------------------------------------------------------------------------------
def quantized_uploads(n, k, bits, tag=0.0):
    """[(codes, scales)] of the k sine client states of compress_cases.inputs through the numpy quantiser"""
    x, xs = Q.inputs(n, k, tag=tag)
    return [Q.quantize(x, xi, None, bits)[:2] for xi in xs]


def hashed_uploads(n, k, bits, top=254):
    """k uploads whose bytes are integer hashes (every code value occurs, -128 / -8 included), scale bytes 100 .. 140 with a 0 and a ``top``
    here and there: no NaN block.  (At top = 254 a code beyond +-1 dequantises to an fp32 infinity, which the quantiser never sends:
    its scale bytes end at 252.  The norm pass works on the integers and stays finite: the block term is defined for every byte.)"""
    out = []
    for i in range(k):
        j = np.arange(Q.code_bytes(bits, n), dtype=np.uint64)
        codes = (((j * np.uint64(2654435761) + np.uint64(40503 * i + 17)) >> np.uint64(9)) & np.uint64(0xFF)).astype(np.uint8)
        b = np.arange(Q.scale_bytes(n), dtype=np.int64)
        scales = (100 + (b * 7 + 3 * i) % 41).astype(np.uint8)
        scales[(b + i) % 61 == 7] = 0
        scales[(b + 5 * i) % 67 == 11] = top
        out.append((codes, scales))
    return out


# ---- the aggregates with device coefficients and noise -----------------------------------------------------------------------------------
def _noised(s, base, noise_std, z):
    with np.errstate(invalid="ignore", over="ignore"):
        if noise_std > 0:
            t = f32(noise_std) * z
            assert t.dtype == f32
            s = s + t
        out = s if base is None else base + s
    assert out.dtype == f32
    return out


def delta_dp(dst, base, uploads, coef, bits, n, accumulate, noise_std=0.0, z=None):
    """one LAST pass of fedfr_delta_aggregate_dp (a pass that is not the last is compress_cases.aggregate with base None)"""
    return _noised(Q.aggregate(dst, None, uploads, coef, bits, n, accumulate), base, noise_std, z)


def delta_chained_dp(x, uploads, coef, bits, n, noise_std=0.0, z=None, with_base=True):
    """the chain of server.FedCompressed with ``clip``: groups of 8, the noise and x on the last pass only = one ascending loop, then the noise"""
    return _noised(Q.chained(x, uploads, coef, bits, n, with_base=False), x if with_base else None, noise_std, z)


def sparse_dp(dst, base, uploads, coef, n, accumulate, noise_std=0.0, z=None):
    return _noised(S.aggregate(dst, None, uploads, coef, n, accumulate), base, noise_std, z)


def sparse_chained_dp(x, uploads, coef, n, noise_std=0.0, z=None, with_base=True):
    return _noised(S.chained(x, uploads, coef, n, with_base=False), x if with_base else None, noise_std, z)
