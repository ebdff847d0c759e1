"""Inputs and references for the compressed-upload kernels (csrc/compress.hip: delta_quantize_kernel, delta_aggregate_kernel).  The format is
the one include/fedfr_hip.h states for fedfr_delta_quantize / fedfr_delta_aggregate.

* ``quantize``: a numpy float32 restatement of the format, step by step: v = (x_i - x) + e (two float32 operations), the block maximum on
  the integer image of |v| (NaN and inf order above every finite value), the scale byte from the exponent field, the code as
  clip(rint(v 2^(127 - eb))) (np.rint is round-half-to-even), the pack, dq = float32(q) 2^(eb - 127) and e' = v - dq (one float32
  subtraction).  Every scale is a power of two, so the only roundings are the ones named here and numpy's float32 operations are single
  correctly rounded IEEE operations, as the kernel's are: the kernel is held to this BIT FOR BIT.
* ``aggregate``: s = (accumulate ? dst + w_0 dq_0 : w_0 dq_0), s = s + w_i dq_i ascending, out = base ? base + s : s; one float32 multiply
  and one float32 add per line.

Nothing here imports the package.
"""
import functools

import numpy as np

f32, f64 = np.float32, np.float64
BLOCK = 32                          # elements per scale byte
EPT = 8                             # elements per thread of both kernels
CHUNK = 64 * EPT                    # elements per wave and loop iteration of the quantiser
GRID_CAP = 2048
SIZES = (1, 3, 31, 32, 33, 63, 64, 1023, 4103)      # below / at / above one block and two; below one wave chunk; several chunks + a tail
BIG = GRID_CAP * 256 * EPT + 37     # the capped grid with every thread at work, a wrap onto the first ones, and a tail
BITS = (8, 4)
U = 2.0 ** -24                      # fp32 unit roundoff


def grid(n):
    """blocks of 256 threads both launchers use: min(ceil((n / 8 + 1) / 256), 2048)"""
    return min((n // EPT + 1 + 255) // 256, GRID_CAP)


def qmax(bits):
    return (1 << (bits - 1)) - 1


def code_bytes(bits, n):
    return (n * bits + 7) // 8


def scale_bytes(n):
    return (n + BLOCK - 1) // BLOCK


def bits_of(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits_or_nan(got, ref):
    """indices at which ``got`` is neither bit-equal to ``ref`` nor NaN where ``ref`` is NaN"""
    ok = (bits_of(got) == bits_of(ref)) | (np.isnan(got) & np.isnan(ref))
    return np.flatnonzero(~ok)


def _freeze(arrays):
    for a in arrays:
        a.flags.writeable = False
    return tuple(arrays)


def scale_of(eb):
    """float32 2^(eb - 127) per scale byte: subnormal at 0, NaN at the reserved 255"""
    eb = np.asarray(eb, dtype=np.uint32)
    u = np.where(eb == 0, np.uint32(0x00400000), np.where(eb == 255, np.uint32(0x7FC00000), eb << np.uint32(23))).astype(np.uint32)
    return u.view(f32)


def pack(q, bits):
    """codes [n] (int) -> the code bytes"""
    q = np.asarray(q, dtype=np.int32).reshape(-1)
    if bits == 8:
        return q.astype(np.int8).view(np.uint8).copy()
    nib = (q & 15).astype(np.uint8)
    if nib.size % 2:
        nib = np.concatenate([nib, np.zeros(1, np.uint8)])      # a missing last element is 0
    return (nib[0::2] | (nib[1::2] << 4)).astype(np.uint8)


def unpack(codes, bits, n):
    """the code bytes -> codes [n] int32"""
    codes = np.asarray(codes, dtype=np.uint8)
    if bits == 8:
        return codes[:n].view(np.int8).astype(np.int32)
    nib = np.empty(codes.size * 2, dtype=np.int32)
    nib[0::2] = codes & 15
    nib[1::2] = codes >> 4
    return (((nib ^ 8) - 8))[:n].astype(np.int32)              # two's-complement nibbles


def value_to_send(x, xi, e=None):
    with np.errstate(invalid="ignore", over="ignore"):
        d = xi - x
        v = d if e is None else d + e
    assert v.dtype == f32
    return v


def quantize(x, xi, e, bits):
    """(codes uint8, scales uint8, new residual float32 or None, nonfinite block count, info) for float32 arrays x, xi and the residual e
    (None: no error feedback).  ``info`` holds the unpacked pieces for the law tests, per element: v, q, eb, scale, the saturated and the
    non-finite-block flags, and e' (also without feedback: what the client would have kept)."""
    assert x.dtype == f32 and xi.dtype == f32 and (e is None or e.dtype == f32)
    n, nb, qm = x.size, scale_bytes(x.size), qmax(bits)
    v = value_to_send(x, xi, e)
    V = np.zeros(nb * BLOCK, dtype=f32)
    V[:n] = v                                                    # elements past n count as 0
    V = V.reshape(nb, BLOCK)
    m = (bits_of(V) & np.uint32(0x7FFFFFFF)).max(axis=1)
    bad = m >= np.uint32(0x7F800000)
    ef = (m >> np.uint32(23)).astype(np.int64)
    eb = np.where(bad, 255, np.clip(ef - (bits - 2), 0, 254)).astype(np.int64)
    inv = np.where(bad, np.uint32(0), ((254 - np.minimum(eb, 254)).astype(np.uint32) << np.uint32(23))).astype(np.uint32).view(f32)
    scale = scale_of(eb)
    Vs = np.where(bad[:, None], f32(0.0), V).astype(f32)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        prod = Vs * inv[:, None]
        assert prod.dtype == f32
        r = np.rint(prod)
        q = np.clip(r, -qm, qm).astype(np.int32)
        dq = q.astype(f32) * scale[:, None]
        assert dq.dtype == f32
        en = np.where(bad[:, None], f32(0.0), Vs - dq).astype(f32)
    sat = (np.abs(r) > qm) & ~bad[:, None]
    info = {"v": v, "q": q.reshape(-1)[:n], "eb": np.repeat(eb, BLOCK)[:n], "scale": np.repeat(scale, BLOCK)[:n], "sat": sat.reshape(-1)[:n],
            "bad": np.repeat(bad, BLOCK)[:n], "e_new": en.reshape(-1)[:n].copy()}
    codes = pack(q.reshape(-1)[:n], bits)
    assert codes.size == code_bytes(bits, n)
    return codes, eb.astype(np.uint8), (None if e is None else en.reshape(-1)[:n].copy()), int(bad.sum()), info


def dequantize(codes, scales, bits, n):
    """dq [n] float32: float32(q) 2^(eb - 127), NaN for the blocks with scale byte 255"""
    q = unpack(codes, bits, n)
    s = np.repeat(scale_of(scales), BLOCK)[:n]
    with np.errstate(invalid="ignore"):
        dq = q.astype(f32) * s
    assert dq.dtype == f32
    return dq


def aggregate(dst, base, uploads, ws, bits, n, accumulate):
    """the float32 restatement of fedfr_delta_aggregate; ``uploads`` = [(codes, scales)], ``ws`` the weights, ``dst`` the previous content
    (read when ``accumulate``), ``base`` an array or None"""
    s = None
    with np.errstate(invalid="ignore", over="ignore"):
        for i, ((codes, scales), w) in enumerate(zip(uploads, ws)):
            term = f32(w) * dequantize(codes, scales, bits, n)
            if i == 0:
                s = (dst + term) if accumulate else term
            else:
                s = s + term
        out = s if base is None else base + s
    assert out.dtype == f32
    return out


def chained(x, uploads, ws, bits, n, with_base=True):
    """x + sum_i w_i dq_i as server.FedCompressed chains it: groups of 8, ``accumulate`` from the second group on, ``base`` = x on the last"""
    acc = np.zeros(n, dtype=f32)
    for c0 in range(0, len(uploads), 8):
        last = c0 + 8 >= len(uploads)
        acc = aggregate(acc, x if (last and with_base) else None, uploads[c0:c0 + 8], ws[c0:c0 + 8], bits, n, c0 > 0)
    return acc


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=8)
def inputs(n, k, tag=0.0):
    """(x, (x_0 .. x_{k-1})) in closed form: a sine global state of magnitude 0.5 and client states that differ from it by per-client sines
    whose amplitude (~0.02) swells and fades along the buffer, so that the blocks span a few octaves of scale.  Shared, read-only."""
    j = np.arange(n, dtype=f64)
    x = (0.5 * np.sin(0.37 * j + 0.1 + tag)).astype(f32)
    env = 0.02 * (0.05 + np.sin(0.0113 * j + tag) ** 2)
    xs = [(x.astype(f64) + env * (1.0 + 0.25 * i) * np.sin(0.091 * (i + 1) * j + 0.5 * i + 0.3 + tag)).astype(f32) for i in range(k)]
    return _freeze([x])[0], _freeze(xs)


@functools.lru_cache(maxsize=8)
def residual(n, tag=0.0):
    """a made-up residual of the size a few rounds leave (|e| ~ 1e-4)"""
    j = np.arange(n, dtype=f64)
    return _freeze([(1e-4 * np.sin(0.77 * j + 1.3 + tag)).astype(f32)])[0]


def _edge_block_list(bits):
    """15 blocks of 32 (x, x_i) pairs; x = 0 except where a block needs the subtraction itself"""
    qm = qmax(bits)
    s = f32(2.0 ** -10)                                          # the scale of the saturation and tie blocks (eb = 117)
    j = np.arange(BLOCK)
    wave = (0.3 * np.sin(0.9 * j + 0.2)).astype(f32)            # |.| <= 0.3
    z = np.zeros(BLOCK, dtype=f32)
    blocks = []

    def add(xi, x=None):
        xi = np.asarray(xi, dtype=f32)
        assert xi.size == BLOCK
        blocks.append((z.copy() if x is None else np.asarray(x, dtype=f32), xi))

    add(z)                                                       # 1  all zero: eb = 0, codes 0
    b = wave.copy(); b[5] = 1.0; b[17] = -0.5                    # 2  amax an exact power of two
    add(b)
    edge = f32((qm + 0.5) * s)                                   # (qmax + 1/2) scale: exactly representable
    below = np.nextafter(edge, f32(0.0))
    b = (wave * s * f32(qm)).astype(f32); b[3] = below; b[9] = -below      # 3  amax just below the saturation edge: rounds to qmax, not saturated
    add(b)
    top = np.nextafter(f32(2.0 ** (bits - 1)) * s, f32(0.0))
    b = (wave * s * f32(qm)).astype(f32); b[0] = edge; b[1] = -edge; b[2] = top; b[30] = -top; b[31] = below      # 4  at the edge (tie to qmax + 1: saturates) and up to the octave's end
    add(b)
    ties = np.array([0.5, 1.5, 2.5, 3.5, 4.5, 5.5, -0.5, -1.5, -2.5, -3.5, -4.5, -5.5], dtype=f32) * s      # 5  .5 ties, both parities and signs
    b = np.zeros(BLOCK, dtype=f32); b[:12] = ties; b[12:24] = ties[::-1]; b[24] = f32(1.5 * 2.0 ** (bits - 2)) * s; b[25:] = (wave[25:] * s)
    add(b)
    add(np.where(j % 3 == 0, f32(-0.0), f32(0.0)))              # 6  +-0 only
    b = wave.copy(); b[j % 4 == 1] = f32(-0.0); b[j % 4 == 3] = f32(0.0)      # 7  +-0 among ordinary values
    add(b)
    sub = np.array([1e-44, -3e-45, 1e-40, -1e-40, 5e-39, -5e-39, 1e-38, -1e-38, 4.4e-39, 1.4e-45], dtype=f32)      # 8  subnormals: eb = 0, codes 0, +-1, +-2
    b = np.zeros(BLOCK, dtype=f32); b[:10] = sub; b[10:20] = -sub; b[20:30] = sub[::-1]
    assert np.all(np.abs(b) < f32(1.1754944e-38))
    add(b)
    b = (wave * f32(6e-38)).astype(f32); b[7] = f32(2e-38)       # 9  the smallest normal exponents: Ef - (bits - 2) < 0 clamps to eb = 0
    add(b)
    b = (wave * f32(1e39 / 3.0 * 3e-1)).astype(f32); b[0] = f32(3e38); b[1] = f32(-3e38); b[2] = f32(3.4028235e38); b[3] = f32(1e38)      # 10 near the top of the range: Ef = 254
    add(b)
    xo, xio = (wave * f32(0.1)).astype(f32), (wave * f32(0.2)).astype(f32)      # 11 x_i - x overflows to +-inf in two elements
    xo[4], xio[4], xo[20], xio[20] = f32(-3e38), f32(3e38), f32(3e38), f32(-3e38)
    add(xio, xo)
    b = wave.copy(); b[11] = np.array([0x7FC00000], dtype=np.uint32).view(f32)[0]      # 12 a NaN, positive sign
    add(b)
    add((wave * f32(0.5)).astype(f32))                           # 13 a finite block between two non-finite ones
    b = wave.copy(); b[0] = np.array([0xFFC00001], dtype=np.uint32).view(f32)[0]; b[31] = np.array([0x7F800001], dtype=np.uint32).view(f32)[0]      # 14 NaNs, negative sign / another payload
    add(b)
    b = wave.copy(); b[6] = f32(np.inf); b[7] = f32(-np.inf)     # 15 infinities
    add(b)
    assert len(blocks) == 15
    return blocks


@functools.lru_cache(maxsize=16)
def edge_blocks(bits, short=1, copies=2):
    """(x, x_i): ``copies`` times the 15 edge blocks, then a short last block of ``short`` elements (1 or 31).  copies = 2: 992 elements, the
    first 512 (all 15 kinds) on the quantiser's whole-chunk path; copies = 1: 481 elements, every block on its partial-chunk path."""
    blocks = _edge_block_list(bits) * copies
    j = np.arange(short)
    xs = [b[0] for b in blocks] + [np.zeros(short, dtype=f32)]
    xis = [b[1] for b in blocks] + [(0.25 * np.cos(0.7 * j + 0.4)).astype(f32)]
    x, xi = _freeze([np.concatenate(xs), np.concatenate(xis)])
    assert x.size == 15 * BLOCK * copies + short and (copies * 15 * BLOCK + 31 < CHUNK if copies == 1 else copies * 15 * BLOCK >= CHUNK + 15 * BLOCK - BLOCK)
    return x, xi
