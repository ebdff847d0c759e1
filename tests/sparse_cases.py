"""Inputs and references for the top-k upload kernels (csrc/sparse.hip: the topk_* kernels, sparse_aggregate_kernel).  The format is the one
include/fedfr_hip.h states for fedfr_topk_sparsify / fedfr_sparse_aggregate.

* ``sparsify``: a numpy restatement of the format: v = (x_i - x) + e (two float32 operations), key = bits(v) & 0x7FFFFFFF, the selected
  set = the first ``keep`` elements in (key descending, index ascending) order (a STABLE argsort of -key), sent in ascending index order
  with their values bit for bit; e' = v with +0 at the sent and at the non-finite positions.  Nothing rounds after v is formed and the
  selection is exact, so the kernels are held to this BIT FOR BIT.
* ``aggregate``: s = accumulate ? dst : +0, then s[idx_i] = s[idx_i] + w_i val_i for ascending i (one float32 multiply, one float32 add),
  out = base ? base + s : s.

Nothing here imports the package.
"""
import functools

import numpy as np

from compress_cases import bits_of, inputs, residual, same_bits_or_nan, value_to_send  # noqa: F401  (re-used by the tests)

f32, f64 = np.float32, np.float64
EPT = 8                             # elements per lane of the sparsify passes
WAVE = 64 * EPT                     # elements per wave
TILE = 4 * WAVE                     # elements per workgroup and loop iteration (one count pair per tile)
GRID_CAP = 2048
AGG_TILE = 4096                     # elements per LDS tile of the aggregate
AGG_STEP = 256                      # entries of one upload the aggregate reads per step
BIG = GRID_CAP * 256 * EPT + 37     # the capped grid, a wrap onto the first workgroup, and a partial tile
U = 2.0 ** -24
INF_KEY = 0x7F800000
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1, 3 * TILE + 5)
AGG_SIZES = (1, 2, AGG_TILE - 1, AGG_TILE, AGG_TILE + 1, 3 * AGG_TILE + 5)


def keeps_for(n):
    """keep in {1, 2, ceil(n / 100), n / 2, n - 1, n}, those that lie in 1..n, ascending and distinct"""
    return sorted({k for k in (1, 2, -(-n // 100), n // 2, n - 1, n) if 1 <= k <= n})


def keep_count(n, ratio):
    return min(n, max(1, int(np.ceil(ratio * n))))


def keys(v):
    return bits_of(v) & np.uint32(0x7FFFFFFF)


def f32_of_bits(u):
    return np.ascontiguousarray(np.asarray(u, dtype=np.uint32)).view(f32)


def select(v, keep):
    """the selected indices, ascending"""
    return np.sort(np.argsort(-keys(v).astype(np.int64), kind="stable")[:keep])


def threshold(v, keep):
    """(T, r): the keep-th largest key and how many elements with key == T are sent"""
    k = keys(v)
    T = np.sort(k)[k.size - keep]
    return int(T), int(keep - np.count_nonzero(k > T))


def positions(v, keep):
    """the position law evaluated directly: for every element of S its place #{key > T, index < j} + min(#{key == T, index < j}, r), and S
    itself as a mask"""
    k = keys(v)
    T, r = threshold(v, keep)
    gt, eq = k > T, k == T
    gb = np.cumsum(gt) - gt                                       # exclusive counts
    eb = np.cumsum(eq) - eq
    sel = gt | (eq & (eb < r))
    return (gb + np.minimum(eb, r))[sel], sel


def select_by_threshold(v, keep):
    """the same set from the threshold law, in O(n) (np.partition): {key > T} and the r lowest-index elements with key == T.  For the inputs
    of tens of millions of elements, where the stable argsort of ``select`` takes seconds; tests/test_sparse_cpu.py holds the two equal."""
    k = keys(v)
    T = np.partition(k, k.size - keep)[k.size - keep]
    r = keep - np.count_nonzero(k > T)
    return np.sort(np.concatenate([np.flatnonzero(k > T), np.flatnonzero(k == T)[:r]]))


def sparsify(x, xi, e, keep, fast=False):
    """(idx uint32 [keep], val float32 [keep], new residual (what a client without feedback would have kept, if ``e`` is None), the number
    of non-finite elements of v, v)"""
    assert x.dtype == f32 and xi.dtype == f32 and (e is None or e.dtype == f32) and 1 <= keep <= x.size
    v = value_to_send(x, xi, e)
    idx = select_by_threshold(v, keep) if fast else select(v, keep)
    bad = keys(v) >= np.uint32(INF_KEY)
    en = v.copy()
    en[idx] = f32(0.0)
    en[bad] = f32(0.0)
    return idx.astype(np.uint32), v[idx].copy(), en, int(bad.sum()), v


def scatter(idx, val, n):
    out = np.zeros(n, dtype=f32)
    out[idx] = val
    return out


def aggregate(dst, base, uploads, ws, n, accumulate):
    """the float32 restatement of fedfr_sparse_aggregate; ``uploads`` = [(idx, val)], ``dst`` the previous content (read when ``accumulate``)"""
    s = dst.copy() if accumulate else np.zeros(n, dtype=f32)
    assert s.dtype == f32
    with np.errstate(invalid="ignore", over="ignore"):
        for (idx, val), w in zip(uploads, ws):
            term = f32(w) * val
            assert term.dtype == f32
            s[idx] = s[idx] + term
        out = s if base is None else base + s
    assert out.dtype == f32
    return out


def chained(x, uploads, ws, n, with_base=True):
    """x + sum_i w_i sparse_i as server.FedSparse chains it: groups of 8, ``accumulate`` from the second group on, ``base`` = x on the last"""
    acc = np.zeros(n, dtype=f32)
    for c0 in range(0, len(uploads), 8):
        last = c0 + 8 >= len(uploads)
        acc = aggregate(acc, x if (last and with_base) else None, uploads[c0:c0 + 8], ws[c0:c0 + 8], n, c0 > 0)
    return acc


# ---- constructed key patterns ------------------------------------------------------------------------------------------------------------
PN = 3 * TILE + 5                   # three whole tiles and a partial one
QNAN_POS, QNAN_NEG, QNAN_PAYLOAD = 0x7FC00000, 0xFFC00001, 0x7FC12345      # quiet NaNs: a subtraction hands their bits on unchanged
TIE_POSITIONS = (3, 10, 77, WAVE + 5, WAVE + 300, TILE + 1, TILE + WAVE + 1, 2 * TILE - 1, 2 * TILE + 9, 3 * TILE + 2)
TIE_VALUE, ABOVE_VALUE = f32(0.5), f32(1.0)
ABOVE_POSITIONS = (0, 64, WAVE - 1, TILE, 2 * TILE + 8, 3 * TILE + 4)
# r and where it puts the cut: (a) inside wave 0 of tile 0, (b) at that wave's end, (c) at tile 0's end, (d) every tie is sent
TIE_CUTS = (("inside a wave", 2), ("at a wave boundary", 3), ("at a tile boundary", 5), ("every tie", len(TIE_POSITIONS)))


def _signs(j):
    return ((j * 2654435761) >> 7 & 1).astype(np.uint32) << np.uint32(31)


@functools.lru_cache(maxsize=1)
def patterns():
    """[(name, v float32 [PN], keep)]: read-only.  Fed to the kernel as x = 0, x_i = v (v - 0 == v bit for bit)."""
    j = np.arange(PN, dtype=np.int64)
    sg = _signs(j)
    out = []

    def add(name, key, keep, signed=True):
        v = f32_of_bits(np.asarray(key, dtype=np.uint32) | (sg if signed else np.uint32(0)))
        v.flags.writeable = False
        out.append((name, v, keep))

    add("top digit only", ((1 + (j * 7) % 2039) << 20), PN // 100)                       # 2039 distinct top digits, all finite
    add("middle digit only", (0x3F8 << 20) | (((j * 13) % 1024) << 10), PN // 10)
    add("lowest digit only", (0x3F8 << 20) | (5 << 10) | ((j * 29) % 1024), PN // 10)
    add("all ties", np.full(PN, 0x3E800000), PN // 3)                                    # |v| = 0.25, signs alternate
    add("all zeros", np.zeros(PN, dtype=np.int64), 100)                                  # +-0
    add("subnormals only", 1 + (j * 2654435761) % 0x7FFFFF, PN // 100)
    add("one exponent", (120 << 23) | ((j * 2654435761) % (1 << 23)), PN // 100)         # the hot bin: 2^-7 <= |v| < 2^-6
    base = (0.01 * np.sin(0.37 * j + 0.2)).astype(f32)
    for what, r in TIE_CUTS:
        v = base.copy()
        v[list(TIE_POSITIONS)] = TIE_VALUE
        v[list(TIE_POSITIONS[1::2])] = -TIE_VALUE
        v[list(ABOVE_POSITIONS)] = ABOVE_VALUE
        v.flags.writeable = False
        out.append(("tie cut " + what, v, len(ABOVE_POSITIONS) + r))
    nf = base.copy()
    at = [5, WAVE + 1, TILE - 1, TILE + 700, 2 * TILE + 3, 3 * TILE + 1, 3 * TILE + 4]
    nf[at] = f32_of_bits([QNAN_POS, QNAN_NEG, INF_KEY, INF_KEY | 0x80000000, QNAN_PAYLOAD, QNAN_NEG, INF_KEY])
    nf.flags.writeable = False
    out.append(("non-finite, fewer than keep", nf, 40))
    out.append(("non-finite, more than keep", nf, 4))
    return tuple(out)


@functools.lru_cache(maxsize=2)
def big_case():
    """(x, x_i, e, keep) at n = BIG with NaNs planted in the first and the last tile; shared, read-only"""
    x, xs = inputs(BIG, 1)
    xi = xs[0].copy()
    xi[[5, 6, BIG - 3]] = f32_of_bits([QNAN_POS, QNAN_NEG, QNAN_PAYLOAD])
    xi.flags.writeable = False
    return x, xi, residual(BIG), -(-BIG // 100)


@functools.lru_cache(maxsize=4)
def big_reference(feedback):
    x, xi, e, keep = big_case()
    out = sparsify(x, xi, e if feedback else None, keep, fast=True)
    for a in out:
        if isinstance(a, np.ndarray):
            a.flags.writeable = False
    return out


# ---- made-up uploads for the aggregate ---------------------------------------------------------------------------------------------------
def _vals(idx, i):
    return (0.3 * np.sin(0.61 * idx.astype(f64) + 0.9 * i + 0.2)).astype(f32)


@functools.lru_cache(maxsize=16)
def uploads(n, shape, k=8):
    """k uploads [(idx uint32 ascending and unique, val float32)] over n elements, read-only.  ``shape``:
    "multiples"  client i holds the multiples of i + 1 (client 0: keep = n): the overlaps follow a fixed pattern, the keeps differ
    "one tile"   every entry inside the second aggregate tile (or the only one)
    "ends"       indices 0 and n - 1 only
    "gaps"       entries further apart than a tile, different offsets per client
    "single"     keep = 1, another index per client"""
    out = []
    for i in range(k):
        if shape == "multiples":
            idx = np.arange(0, n, i + 1)
        elif shape == "one tile":
            lo = AGG_TILE if n > AGG_TILE else 0
            idx = np.arange(lo + i, min(lo + AGG_TILE, n), 3 + i)
            idx = idx if idx.size else np.array([n - 1])
        elif shape == "ends":
            idx = np.unique(np.array([0, n - 1]))
        elif shape == "gaps":
            idx = np.arange((37 * i) % n, n, AGG_TILE + 513 + 64 * i)
        elif shape == "single":
            idx = np.array([(i * 2654435761) % n])
        else:
            raise ValueError(shape)
        idx = idx.astype(np.uint32)
        val = _vals(idx, i)
        assert idx.size >= 1 and np.all(np.diff(idx.astype(np.int64)) > 0) and idx[-1] < n
        idx.flags.writeable = False
        val.flags.writeable = False
        out.append((idx, val))
    return tuple(out)


UPLOAD_SHAPES = ("multiples", "one tile", "ends", "gaps", "single")
