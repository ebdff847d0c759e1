"""Restatement of distributed differential privacy on 16-bit narrow words (csrc/ddp_narrow.hip; the format: include/fedfr_hip.h, "NARROW
WORDS UNDER DISTRIBUTED DP"), from the restatements of its parts and from nothing else:

    secagg_narrow_cases.rotate32            v = 2^-6 H (D (xi - x)) on the padded vector
    secagg_narrow_cases.encode_narrow32     the stochastic encoder at coef = fl(factor 2^f), the DEVICE's clip factor, clamped at ``limit``
    ddp_cases.sample                        the discrete Gaussian of the stream (noise seed, round, NOISE_STREAM) on ALL n_pad elements:
                                            element e is position e of the padded rotated vector (the padding carries noise)
    secagg_narrow_cases.pack                code + noise mod 2^16, two fields to a word
    secagg_narrow_cases.stream_sum_fields   the k ChaCha20 streams, field-wise

``mask_narrow_dp`` is ``fedfr_secagg_mask_narrow_dp``; the two accepted deviations are those of tests/ddp_cases.py (last-place log / exp,
flagged per element as AMBIGUOUS; the clip factor, for which a test feeds the device's own).  The inputs of the GPU tests are stated here
so that tests/test_ddp_narrow_cpu.py can hold their seeds to "no ambiguous decision" without a GPU.

Nothing here imports the package."""
import numpy as np

import ddp_cases as X
import dp_cases as D  # noqa: F401   (the Philox restatement under both samplers)
import secagg_cases as S
import secagg_narrow_cases as N

f32, f64, u32, i32, i64 = np.float32, np.float64, np.uint32, np.int32, np.int64
BITS = 16
FIELD_MAX = 2 ** 15 - 1
EPS_FP, EPS_ROT = 2.0 ** -22, 13 * 2.0 ** -24      # privacy.DistributedDiscreteGaussian's, restated


def codes(x, xi, factor, frac_bits, limit, rot_seed, priv_seed, rnd):
    """(codes int32 [n_pad], saturated, nonfinite) at the clip factor ``factor`` (float32)"""
    coef = f32(factor) * f32(2.0 ** frac_bits)
    assert coef.dtype == f32 and x.dtype == xi.dtype == f32
    with np.errstate(over="ignore", invalid="ignore"):
        u = xi - x
    v = N.rotate32(u, rot_seed, rnd)
    return N.encode_narrow32(v, coef, limit, N.draws(v.size, priv_seed, rnd))


def noise(n_pad, seed, rnd, offset, sigma):
    """(values int64 [n_pad], ambiguous [n_pad], exhausted count) of the clients' noise stream"""
    values, _, ambiguous, exhausted = X.sample(n_pad, seed, rnd, X.NOISE_STREAM, offset, sigma)
    return values, ambiguous, exhausted


def mask_narrow_dp(x, xi, factor, frac_bits, limit, rot_seed, priv_seed, rnd, noise_seed, noise_rnd, noise_offset, sigma, streams, counter0=0):
    """(y uint32 [n_pad / 2], sum of the squared codes mod 2^64 as a Python int, (saturated, nonfinite, exhausted), ambiguous [n_pad] bool)"""
    q, sat, bad = codes(x, xi, factor, frac_bits, limit, rot_seed, priv_seed, rnd)
    sq = X._sq_mod64(q)
    z, amb, exhausted = noise(q.size, noise_seed, noise_rnd, noise_offset, sigma)
    w = N.pack(q.astype(i64) + z, BITS)
    y = N.field_add(w, N.stream_sum_fields(w.size, streams, BITS, counter0), BITS)
    return y, sq, (sat, bad, exhausted), amb


def delta_int(clip, frac_bits, n):
    """the mechanism's L2 sensitivity at 16 bits, restated: C 2^f (1 + EPS_FP) (1 + EPS_ROT) + sqrt(n_pad)"""
    return clip * 2.0 ** frac_bits * (1.0 + EPS_FP) * (1.0 + EPS_ROT) + np.sqrt(float(N.padded_count(n)))


# ---- the inputs of the GPU tests ------------------------------------------------------------------------------------------------------------
SIZES = N.SIZES                              # one padded block from a single element, a block less one, exact, one more, ragged past three
KINDS = ("planted", "binds", "free", "zero")
ROT_SEED, PRIV_SEED, RND = 0xC0FFEE_0000_0002, 0xFEED_FACE_CAFE_F00D, 6
NOISE_SEED, NOISE_ROUND = 0x0BADC0DE_1234_5678, 11
NOISE_OFFSET = (1 << 40) + 7                 # a non-zero offset whose block index (offset + e) * 64 needs the high counter word
FRAC = 12
SIGMA = {"planted": 16.0, "binds": 100.25, "free": 16.0, "zero": 100.25}      # the sampler's smallest sigma, and a non-integer one
LIMIT = {"planted": 511, "binds": 12, "free": 511, "zero": 511}


def inputs(n, kind):
    """(x, xi, clip, limit, sigma) float32 inputs of one case:
    planted   the blocks of secagg_narrow_cases.planted_inputs at coef 2^12 and limit 511 under a clip that never binds; the first block is
              of another kind at every size, so that over SIZES a padded block is non-finite (n = 1: +inf, the clip factor is 0 and every
              product NaN), saturating (4095), all-zero (4096), ordinary and ties (4097), and the largest size holds a NaN block (the
              norm is NaN: the factor stays 1), a saturating and a zero one
    binds     ordinary updates and one large element: ||xi - x|| is about 0.5 and clip = 0.25, so the factor is about 0.5.  The rotation
              spreads the large element over its block, +-16 on every coordinate at 2^12: under the limit 12 the whole block saturates
    free      ordinary updates of norm about 1e-3 sqrt(n) under clip = 10: the factor is exactly 1
    zero      xi = x: every code is 0 and a field is the noise (and the masks) alone"""
    if kind == "planted":
        x, xi = N.planted_inputs(n, f32(2.0 ** FRAC), LIMIT[kind], first=SIZES.index(n) + 2)
        return x, xi, 1e3, LIMIT[kind], SIGMA[kind]
    g = np.random.default_rng(2000 + n)
    x = (g.standard_normal(n) * 0.05).astype(f32)
    xi = (x + g.standard_normal(n).astype(f32) * f32(1e-3)).astype(f32)
    if kind == "binds":
        xi[min(1, n - 1)] = x[min(1, n - 1)] + f32(0.5)
        return x, xi, 0.25, LIMIT[kind], SIGMA[kind]
    if kind == "zero":
        return x, x.copy(), 1.0, LIMIT[kind], SIGMA[kind]
    assert kind == "free"
    return x, xi, 10.0, LIMIT[kind], SIGMA[kind]
