"""Restatements for the narrow secure-aggregation kernels (csrc/secagg_narrow.h, csrc/secagg_narrow.hip; the format: include/fedfr_hip.h,
"NARROW WORDS"), on top of the ChaCha20 restatement of secagg_cases.py and the Philox restatement of dp_cases.py.

* ``sign_bits`` / ``hadamard32`` / ``rotate32`` / ``rotate_back32``: the public signs D (bit e % 32 of word e / 32 of the Philox stream
  (rotation seed, round, SIGN_SID)), the unnormalised Walsh-Hadamard butterfly on blocks of 4096 in float32, LEVEL BY LEVEL in the order
  h = 1, 2, 4, ..., 2048 (one fp32 addition or subtraction per output), and v = 2^-6 H (D u) / u' = D (2^-6 H s).  ``fedfr_rht_fill`` is held
  to these BIT FOR BIT.  ``rotate64`` is the same in float64: the yardstick of ROTATION_BOUND.
* ``encode_narrow32``: t = v coef, fl = floor(t), q = clamp(fl + [r 2^-24 < t - fl], -L, L) with r the top 24 bits of word e of the private
  stream (private seed, round, ROUND_SID); a non-finite t gives 0.  Counters as in secagg_cases.encode32.
* ``pack`` / ``unpack``: element e is field e % F of word e / F, little end first, F = 32 / bits.
* ``field_add`` / ``field_sub``: addition and subtraction of every field mod 2^bits THROUGH NUMPY'S OWN uint8 / uint16 ARITHMETIC (a view of the
  words; little-endian hosts), and ``swar_add`` / ``swar_sub``: the kernels' formulas on whole words, held to the former in the CPU tests.
* ``mask_narrow`` / ``aggregate_narrow``: ``fedfr_secagg_mask_narrow`` and ``fedfr_secagg_aggregate_narrow`` in ONE order (field-wise addition
  is associative and commutative: every chaining must give these bits).

ROTATION_BOUND.  Every level is one fp32 addition or subtraction per output, fl(a +- b) = (a +- b)(1 + d), |d| <= u = 2^-24, and never
a product, so after the 12 levels an output of H (D x) is sum_e +-x_e prod (1 + d) with 12 factors on every path: it is within
((1 + u)^12 - 1) ||x||_1 = 12 u ||x||_1 (first order) of the exact value.  The 2^-6 scale is exact and ||x||_1 <= sqrt(4096) ||x||_2 =
64 ||x||_2, so an element of v is within 12 u ||x||_2 of the fp64 rotation; the bound keeps 12.5 u for the second-order terms.  It is
derived, not measured.

Nothing here imports the package."""
import sys

import numpy as np

import dp_cases as D
import secagg_cases as S

f32, f64, u32, i32, i64 = np.float32, np.float64, np.uint32, np.int32, np.int64
assert sys.byteorder == "little"
BLOCK = 4096
SIGN_SID = 0x52485444                        # "RHTD"
ROUND_SID = 0x53525244                       # "SRRD"
SIZES = (1, 4095, 4096, 4097, 3 * 4096 + 17)
ROTATION_BOUND = 12.5 * 2.0 ** -24           # times ||u_block||_2, per element


def padded_count(n):
    return (n + BLOCK - 1) // BLOCK * BLOCK


def code_limit(K, bits):
    return (2 ** (bits - 1) - 1) // K


def sign_bits(n_pad, seed, rnd):
    """bool [n_pad]: element e is negated where bit e % 32 of word e / 32 of the stream is 1"""
    assert n_pad % BLOCK == 0
    w = D.words(n_pad // 32, seed, rnd, SIGN_SID)
    return ((w[:, None] >> np.arange(32, dtype=u32)[None, :]) & u32(1)).astype(bool).reshape(-1)


def _butterfly(v):
    """H on the last axis (4096) of v, level by level; the dtype of v is kept"""
    shape = v.shape
    h = 1
    while h < BLOCK:
        w = v.reshape(-1, BLOCK // (2 * h), 2, h)
        a, b = w[:, :, 0, :], w[:, :, 1, :]
        v = np.stack([a + b, a - b], axis=2).reshape(shape)
        h *= 2
    return v


def hadamard32(v):
    assert v.dtype == f32 and v.shape[-1] == BLOCK
    with np.errstate(over="ignore", invalid="ignore"):
        out = _butterfly(v)
    assert out.dtype == f32
    return out


def pad32(u):
    out = np.zeros(padded_count(u.size), dtype=f32)
    out[:u.size] = u
    return out


def rotate32(u, seed, rnd):
    """v = 2^-6 H (D u) on the padded vector, float32 [n_pad]"""
    assert u.dtype == f32
    p = pad32(u)
    p = np.where(sign_bits(p.size, seed, rnd), -p, p)
    with np.errstate(over="ignore", invalid="ignore"):
        return (hadamard32(p.reshape(-1, BLOCK)) * f32(2.0 ** -6)).reshape(-1)


def rotate_back32(s, seed, rnd):
    """u' = D (2^-6 H s), float32 [n_pad]; s is padded the same way"""
    assert s.dtype == f32
    p = pad32(s)
    with np.errstate(over="ignore", invalid="ignore"):
        r = (hadamard32(p.reshape(-1, BLOCK)) * f32(2.0 ** -6)).reshape(-1)
    return np.where(sign_bits(p.size, seed, rnd), -r, r)


def rotate64(u, seed, rnd):
    p = np.zeros(padded_count(u.size), dtype=f64)
    p[:u.size] = u
    p = np.where(sign_bits(p.size, seed, rnd), -p, p)
    return (_butterfly(p.reshape(-1, BLOCK)) * 2.0 ** -6).reshape(-1)


def draws(n_pad, seed, rnd):
    """word e of the private stream, e < n_pad"""
    return D.words(n_pad, seed, rnd, ROUND_SID)


def encode_narrow32(v, coef, limit, r):
    """(codes as int32, saturated, nonfinite); v float32 (rotated), r uint32 draws of the same length"""
    assert v.dtype == f32 and r.dtype == u32 and v.shape == r.shape
    with np.errstate(over="ignore", invalid="ignore"):
        t = v * f32(coef)
        assert t.dtype == f32
        finite = np.isfinite(t)
        t0 = np.where(finite, t, f32(0))
        fl = np.floor(t0)
        frac = t0 - fl                                   # one fp32 subtraction
        assert frac.dtype == f32
        uu = (r >> u32(8)).astype(f32) * f32(2.0 ** -24)  # exact
        inc = uu < frac
    q = np.clip(fl.astype(f64) + inc, -limit, limit).astype(i64)
    q = np.where(finite, q, 0)
    saturated = int(np.count_nonzero(finite & (np.abs(q) == limit)))
    return q.astype(i32), saturated, int(np.count_nonzero(~finite))


def pack(q, bits):
    """int codes [n_pad] -> uint32 words [n_pad bits / 32]"""
    F = 32 // bits
    f = (np.asarray(q).astype(i64) & ((1 << bits) - 1)).reshape(-1, F)
    w = np.zeros(f.shape[0], dtype=i64)
    for c in range(F):
        w |= f[:, c] << (bits * c)
    return w.astype(u32)


def unpack(w, bits):
    """uint32 words -> the fields as signed int64 [len(w) 32 / bits]"""
    assert w.dtype == u32
    F = 32 // bits
    f = (w.astype(i64)[:, None] >> (bits * np.arange(F, dtype=i64))[None, :]) & ((1 << bits) - 1)
    f = np.where(f >= 1 << (bits - 1), f - (1 << bits), f)
    return f.reshape(-1)


def _view(w, bits):
    return np.ascontiguousarray(w).view(np.uint8 if bits == 8 else np.uint16)


def field_add(a, b, bits):
    with np.errstate(over="ignore"):
        return (_view(a, bits) + _view(b, bits)).view(u32)


def field_sub(a, b, bits):
    with np.errstate(over="ignore"):
        return (_view(a, bits) - _view(b, bits)).view(u32)


def _hi(bits):
    return u32(0x80808080 if bits == 8 else 0x80008000)


def swar_add(a, b, bits):
    """the kernels' word formula (csrc/secagg_narrow.h, Fields::add)"""
    H = _hi(bits)
    with np.errstate(over="ignore"):
        return ((a & ~H) + (b & ~H)) ^ ((a ^ b) & H)


def swar_sub(a, b, bits):
    H = _hi(bits)
    with np.errstate(over="ignore"):
        return ((a | H) - (b & ~H)) ^ ((a ^ ~b) & H)


def stream_sum_fields(nwords, streams, bits, counter0=0):
    """the field-wise signed sum of the streams' words counter0 * 16 ... over ``streams`` = [(key, nonce, sign)]"""
    tot = np.zeros(nwords, dtype=u32)
    for key, nonce, sign in streams:
        assert sign in (1, -1)
        m = S.words(nwords, key, counter0, nonce)
        tot = field_add(tot, m, bits) if sign > 0 else field_sub(tot, m, bits)
    return tot


def codes_narrow(x, xi, coef, K, bits, rot_seed, priv_seed, rnd):
    """(codes int32 [n_pad], saturated, nonfinite) of one client"""
    assert x.dtype == xi.dtype == f32
    with np.errstate(over="ignore", invalid="ignore"):
        u = xi - x
    v = rotate32(u, rot_seed, rnd)
    return encode_narrow32(v, coef, code_limit(K, bits), draws(v.size, priv_seed, rnd))


def mask_narrow(x, xi, coef, K, bits, rot_seed, priv_seed, rnd, streams, counter0=0):
    """(y uint32 [n_pad bits / 32], saturated, nonfinite, the codes)"""
    q, sat, bad = codes_narrow(x, xi, coef, K, bits, rot_seed, priv_seed, rnd)
    w = pack(q, bits)
    return field_add(w, stream_sum_fields(w.size, streams, bits, counter0), bits), sat, bad, q


def decode_narrow(S_words, bits, frac_bits, rescale, rot_seed, rnd, n, x=None):
    s = unpack(S_words, bits).astype(f32) * f32(2.0 ** -frac_bits)
    d = rotate_back32(s, rot_seed, rnd)[:n] * f32(rescale)
    assert d.dtype == f32
    return d if x is None else x + d


def aggregate_narrow(x, ys, streams, bits, frac_bits, rescale, rot_seed, rnd, n, counter0=0):
    """out as float32 [n]; ``x`` may be None"""
    nwords = padded_count(n) * bits // 32
    s = np.zeros(nwords, dtype=u32)
    for y in ys:
        assert y.dtype == u32 and y.size == nwords
        s = field_add(s, y, bits)
    s = field_add(s, stream_sum_fields(nwords, streams, bits, counter0), bits)
    return decode_narrow(s, bits, frac_bits, rescale, rot_seed, rnd, n, x)


KINDS = ("ordinary", "ties", "nonfinite", "saturating", "zero")


def planted_inputs(n, coef, limit, first=0, seed=3, scale=1e-3):
    """(x, xi) float32 of length n.  Rotation block b is of kind KINDS[(b + first) % 5]:
      ordinary     x_i - x of size ``scale``, both signs
      ties         x = 0 and x_i = a e_0 with a coef / 64 = 2.5: every rotated element is +-2.5 exactly, a draw away from 2 or 3 (-3 or -2)
      nonfinite    an ordinary block with a NaN and an inf in it: every element of the rotated block is non-finite
      saturating   x = 0 and x_i = a e_0 with a coef / 64 = 4 limit: every code is clamped
      zero         x_i = x: every code is 0
    (a ragged last block is planted the same way as far as it reaches)"""
    g = np.random.default_rng(seed)
    x = (g.standard_normal(n) * 0.05).astype(f32)
    xi = (x + g.standard_normal(n).astype(f32) * f32(scale)).astype(f32)
    for b in range(padded_count(n) // BLOCK):
        lo, hi = b * BLOCK, min(n, (b + 1) * BLOCK)
        kind = KINDS[(b + first) % 5]
        if kind == "ties":
            x[lo:hi], xi[lo:hi] = 0, 0
            xi[lo] = 2.5 * 64 / float(coef)
        elif kind == "nonfinite":
            xi[lo] = np.nan
            xi[hi - 1] = np.inf
        elif kind == "saturating":
            x[lo:hi], xi[lo:hi] = 0, 0
            xi[lo] = -4.0 * limit * 64 / float(coef)
        elif kind == "zero":
            xi[lo:hi] = x[lo:hi]
    return x, xi
