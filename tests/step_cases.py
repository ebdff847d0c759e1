"""Inputs, case tables, restated launch rules, plain references and check functions for the direct tests of the kernels that run on every
step and had only spot checks: momentum SGD (csrc/optim.hip: sgd_kernel, both instantiations), fedavg_axpy, the PartialFC selection
(pfc_topk / pfc_topk_wide, pfc_positive, pfc_remap, rows gather / scatter), the head helpers (csrc/head.hip: contrastive, sgemm_colflag,
class_accumulate, roc_histogram) and the input path (csrc/ew.hip: preprocess_u8, pad_input_nhwc).  tests/test_step_kernels_gpu.py runs
the kernels against what is here; tests/test_step_cases_cpu.py proves the exact cases admissible, holds the toleranced formulas at fp32 in
the kernels' operation order to a QUARTER of their tolerance, checks the tables against the restated launch rules and shows one mutant per
check that the check rejects.  Nothing here touches the GPU library or imports the oracle.

Exactness and tolerance rules.
  SGD           bit-exact against ``sgd_ref``, a numpy restatement of sgd_one operation by operation: d = fma(wd, p, g); b = first ? d :
                fl(fl(buf mu) + d); p' = fma(-lr, b, p).  ``fma32`` is an exact fp32 fused multiply-add: the product of two fp32 values is
                exact in float64, the sum is rounded to float64 and then to fp32; the two roundings differ from one only where the float64
                sum sits exactly on an fp32 tie (low 29 mantissa bits == 2^28) or below the fp32 normal range, and those elements are
                recomputed with fractions.Fraction.  The O(1) hyper-parameters (lr 0.61, mu 0.9, wd 0.37) are what makes a bit comparison
                sharp: at wd = 5e-4 an unfused weight decay changes almost nothing.  The 16-bit shadow equals p'.to(storage dtype).
  fedavg_axpy   bit-exact: fl(d + fl(w s)).
  selection     exact index sets (stable descending argsort), exact counts, exact searchsorted, exact row copies.
  contrastive   float64 formula + autograd, each norm clamped at 1e-8.  row_loss: TOL["loss"] against max(1, |ref|).  dx: TOL["grad"] per
                row against that row's max |ref| — except rows whose gradient cancels BY CONSTRUCTION (every row at D == 1, where cos is
                +-1 and its derivative zero, and the g == l row, where the two terms are equal and opposite): there the reference is 0 and
                a correct fp32 kernel leaves the rounding of its three terms, so the denominator is the row's max_i (|kg g_i| + |kl l_i| +
                |kx x_i|), the sum of |terms| the other suites use for cancelling sums.  Inputs with 0 < ||x|| < 1e-8 are OUTSIDE the
                contract (the kernel differentiates through the clamp as if it were not there; torch gives the clamp a zero derivative):
                none is fed.  An all-zero x row is inside it: both give dx = kg g + kl l.  The "underflow" row: with T >= 0.07 and
                |cos| <= 1, (pos - neg) <= 28.6, which expf itself survives (3.9e-13); what vanishes is expf(neg - pos) against 1 in the
                logsumexp, so row_loss is 0 in fp32 and 2e-12 in float64 — inside TOL["loss"] of max(1, |ref|) — and dx is carried by
                p1 = expf(neg - lse) alone.  The row is conditioned (l = -g + an orthogonal part) so that dx does not vanish with it.
  colflag       exact tier: small-integer operands, K max|a| max|b| < 2^24, alpha a power of two: every score is exact in any order.
  class_accumulate  bit-equal to the stated order (per class, per 1024-row slice, sequential fp32 from 0, then added to sums) and within
                TOL["fwd"] of float64 per element against |sums| + sum |terms|.
  roc           features on a 1/8 grid: every dot product is a multiple of 1/64 and exact in any order, (s + 1) * 1000 is exact in float64.
  input path    bit-exact."""
import functools
import math
from fractions import Fraction

import numpy as np
import torch

import fedopt_cases as fc
import head_cases as hc
import tail_cases as tc

f32, f64 = np.float32, np.float64
TOL, TINY, SENTINEL, uniform = hc.TOL, hc.TINY, hc.SENTINEL, hc.uniform
Q, check = tc.Q, tc.check                                  # per COLUMN: con_check hands dx over transposed, so that a column is one of its rows
pfc_rand_order = tc.pfc_rand_order
cdiv = tc.cdiv


def bits32(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.int32)


def same32(got, want, what="", nan_ok=False):
    """bit equality of two fp32 arrays; a NaN equals only the same NaN — nan_ok: any NaN (a payload is not part of a contract)"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, "%s: shape %s != %s" % (what, got.shape, want.shape)
    bad = bits32(got) != bits32(want)
    if nan_ok:
        bad &= ~(np.isnan(got) & np.isnan(want))
    assert not bad.any(), "%s: %d of %d elements differ, first at %d" % (what, int(bad.sum()), bad.size, int(np.flatnonzero(bad.reshape(-1))[0]))


def same_int(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and np.array_equal(got, want), "%s: %d entries differ" % (
        what, int((got != want).sum()) if got.shape == want.shape else -1)


# ================================================================================================ SGD
SGD_GRID_CAP = 4096                                        # optim.hip: optim_sgd and optim_fedavg_axpy — blocks of 256 threads, one float4 each
SGD_WRAP_N = SGD_GRID_CAP * 256 * 4 + 7                    # the grid-stride loop's second round (two float4) plus a tail of three
SGD_N = [1, 2, 3, 4, 5, 7, 1023, 1024, 1025, 4103, SGD_WRAP_N]
SGD_HYPER = (0.61, 0.9, 0.37)                              # (lr, mu, wd): the bit-exact tier
SGD_HYPER_PRODUCT = (0.1, 0.9, 5e-4)                       # what training runs with
SGD_SCALE = 2.0 ** -8                                      # the buffer holds gradient / grad_scale; the kernel multiplies by grad_scale
SGD_MUTANTS = ("unfused_wd", "fused_momentum", "unfused_update")


def sgd_grid(n):
    """blocks the launcher uses: min(ceil((n / 4 + 1) / 256), 4096)"""
    return min(cdiv(n // 4 + 1, 256), SGD_GRID_CAP)


def sgd_wraps(n):
    return n // 4 > sgd_grid(n) * 256


def sgd_tail_only(n):
    return n < 4


def round_fraction_f32(q):
    """the fp32 nearest to the rational q, ties to even"""
    if q == 0:
        return f32(0.0)
    x = f32(float(q))
    best, bd = None, None
    for c in (x, np.nextafter(x, f32(np.inf)), np.nextafter(x, f32(-np.inf))):
        if not np.isfinite(c):
            continue
        d = abs(Fraction(float(c)) - q)
        if bd is None or d < bd or (d == bd and (int(np.asarray(c, f32).view(np.int32)) & 1) == 0):
            best, bd = c, d
    return best


FMA_TIE_MASK, FMA_TIE = np.uint64((1 << 29) - 1), np.uint64(1 << 28)


def fma_risky(s):
    """where rounding the float64 sum s to fp32 may differ from rounding the exact sum once"""
    with np.errstate(all="ignore"):
        return np.isfinite(s) & (((s.view(np.uint64) & FMA_TIE_MASK) == FMA_TIE) | ((np.abs(s) < 2.0 ** -126) & (s != 0)))


def fma32(a, b, c, exact_all=False, stats=None):
    """fl32(a b + c) with ONE rounding.  exact_all: every finite element through fractions.Fraction (what the CPU file compares with)"""
    a, b, c = np.broadcast_arrays(np.atleast_1d(np.asarray(a, f32)), np.atleast_1d(np.asarray(b, f32)), np.atleast_1d(np.asarray(c, f32)))
    with np.errstate(all="ignore"):
        s = a.astype(f64) * b.astype(f64) + c.astype(f64)
        r = s.astype(f32)
    idx = np.flatnonzero(np.isfinite(s).reshape(-1) if exact_all else fma_risky(s).reshape(-1))
    if stats is not None:
        stats.append(int(idx.size))
    if idx.size:
        fa, fb, fcc, fr = a.reshape(-1), b.reshape(-1), c.reshape(-1), r.reshape(-1)
        for i in idx:
            fr[i] = round_fraction_f32(Fraction(float(fa[i])) * Fraction(float(fb[i])) + Fraction(float(fcc[i])))
    return r


def sgd_ref(p, g, buf, lr, mu, wd, first, gs=None, mutant=None):
    """one call of sgd_kernel in numpy: (p', buf', g', overflow).  gs: the UNSCALE instantiation (g' = fl(g gs), elements whose g' is not
    finite keep p and buf — 0 on the first step — and set the word).  mutant: one of SGD_MUTANTS or "bad_updates_momentum\""""
    lr, mu, wd = f32(lr), f32(mu), f32(wd)
    p, g = np.asarray(p, f32), np.asarray(g, f32)
    b0 = np.zeros_like(p) if first else np.asarray(buf, f32)
    with np.errstate(all="ignore"):
        if gs is not None:
            g = g * f32(gs)
        d = (wd * p + g) if mutant == "unfused_wd" else fma32(wd, p, g)
        if first:
            b = d
        elif mutant == "fused_momentum":
            b = fma32(b0, mu, d)
        else:
            b = (b0 * mu) + d
        pn = (p - lr * b) if mutant == "unfused_update" else fma32(-lr, b, p)
        assert d.dtype == f32 and b.dtype == f32 and pn.dtype == f32
        ovf = 0
        if gs is not None:
            bad = ~np.isfinite(g)
            pn = np.where(bad, p, pn)
            if mutant != "bad_updates_momentum":
                b = np.where(bad, b0, b)
            ovf = int(bad.any())
    return pn.astype(f32), b.astype(f32), g, ovf


@functools.lru_cache(maxsize=None)
def sgd_inputs(n):
    """(p, g): uniform, the gradient a quarter of the parameters' range (read-only, shared)"""
    p, g = uniform((n,), 4000 + n % 9973).numpy(), (uniform((n,), 4001 + n % 9973) * 0.25).numpy()
    p.setflags(write=False)
    g.setflags(write=False)
    return p, g


@functools.lru_cache(maxsize=None)
def sgd_two_steps(n, hyper=SGD_HYPER):
    """[(p1, buf1), (p2, buf2)]: first = 1, then first = 0 with a second gradient, on the same buffers"""
    p, g = sgd_inputs(n)
    lr, mu, wd = hyper
    p1, b1, _, _ = sgd_ref(p, g, None, lr, mu, wd, 1)
    p2, b2, _, _ = sgd_ref(p1, sgd_second_grad(n), b1, lr, mu, wd, 0)
    return (p1, b1), (p2, b2)


@functools.lru_cache(maxsize=None)
def sgd_second_grad(n):
    g = (uniform((n,), 4002 + n % 9973) * 0.25).numpy()
    g.setflags(write=False)
    return g


def sgd_bad_positions(n):
    """where the non-finite gradients go: element 0, the float4 body, the scalar tail, n - 1 and, at the wrap size, the second
    grid-stride round (float4 index >= grid * 256)"""
    pos = {0, n - 1}
    if n >= 12:
        pos |= {5, 10}
    if n % 4 and n >= 4:
        pos.add(n // 4 * 4)
    if sgd_wraps(n):
        pos.add(4 * sgd_grid(n) * 256 + 2)
    return sorted(pos)


def sgd_bad_values(k):
    return np.array([np.inf, -np.inf, np.nan] * k, dtype=f32)[:k]


# ---- the 16-bit shadow
def shadow_ref(p, s16):
    return torch.from_numpy(np.array(p, dtype=f32)).to(s16)


def shadow_mutant(p, s16, kind):
    """"truncate": rounded toward zero; "flush": results below the smallest normal become zero"""
    t = torch.from_numpy(np.array(p, dtype=f32))
    r = t.to(s16)
    if kind == "truncate":
        over = (r.float().abs() > t.abs()) & torch.isfinite(t)
        return torch.where(over, (r.view(torch.int16) - 1).view(s16), r)            # one step toward zero (sign-magnitude)
    tiny = torch.finfo(s16).tiny
    return torch.where(r.float().abs() < tiny, torch.zeros_like(r), r)


def shadow_plants(s16):
    """parameters to plant, as fp32: values that round to a 16-bit subnormal (one of them an exact tie to zero), round-to-even ties both
    ways and, for fp16, magnitudes above 65504 (the first that rounds to inf, the last that does not)"""
    if s16 == torch.float16:
        v = [2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -25, 3 * 2.0 ** -25, -(2.0 ** -25), 1023.5 * 2.0 ** -24, 5.75 * 2.0 ** -20,
             1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 2.0 ** -11), 1 + 2.0 ** -11 + 2.0 ** -23,
             65520.0, -65520.0, 65519.996, 1e5]
    else:
        v = [2.0 ** -133, 2.0 ** -134, 1.5 * 2.0 ** -134, 3 * 2.0 ** -134, -(2.0 ** -134), 5.75 * 2.0 ** -130, 2.0 ** -127,
             1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 1 + 2.0 ** -8 + 2.0 ** -23]
    return np.array(v, dtype=f64).astype(f32)


def shadow_plant_case(s16, j):
    """(p, g, body, tail): n = 4 L + 3; every planted value sits once in the float4 body (positions 4 ...: all four lanes) and values
    3 j ... 3 j + 2 sit in the scalar tail.  g = -fl(wd p) there, so the weight decay cancels to its rounding residue and the new p is the
    planted value again — which the CPU file asserts from the reference, not from this sentence"""
    v = shadow_plants(s16)
    L = len(v)
    n = 4 * L + 3
    p, g = (uniform((n,), 4100 + j) * 0.5).numpy(), (uniform((n,), 4200 + j) * 0.25).numpy()
    body = np.arange(4, 4 + L)
    tail = np.arange(4 * L, 4 * L + 3)
    tv = np.array([v[(3 * j + t) % L] for t in range(3)], dtype=f32)
    p[body], p[tail] = v, tv
    wd = f32(SGD_HYPER[2])
    for idx in (body, tail):
        g[idx] = -(wd * p[idx])
    return p, g, body, tail


def shadow_plant_calls(s16):
    return cdiv(len(shadow_plants(s16)), 3)


# ================================================================================================ fedavg_axpy
AXPY_N = list(fc.SIZES) + [SGD_GRID_CAP * 256 * 4 + 5]
AXPY_W = (0.3, 0.45)


def axpy_ref(dst, src, w, accumulate):
    d = np.asarray(dst, f32) if accumulate else np.zeros_like(src)
    t = f32(w) * np.asarray(src, f32)
    r = d + t
    assert t.dtype == f32 and r.dtype == f32
    return r


# ================================================================================================ PartialFC selection
TOPK_WIDE_MIN_N = 8192                                     # optim.hip: optim_pfc_topk — the wide kernel needs n >= 8192 and a 16-byte-aligned perm
TOPK_CHUNK = 16384                                         # the wide kernel's chunk: 1024 threads x 16 consecutive values
TOPK_ROUND = 1024                                          # the narrow kernel's compaction round
TOPK_N = [1, 2, 1023, 1024, 1025, 8191, 8192, 8193, 16383, 16384, 16385, 2 * 16384 + 3, 85000]
TOPK_PATTERN_N = [1025, 8191, 8192, 8193, 2 * 16384 + 3]   # the value patterns: both sides of the dispatch boundary, one and three chunks
TOPK_MARKS = 50


def topk_is_wide(aligned, n):
    return bool(aligned) and n >= TOPK_WIDE_MIN_N


def topk_ks(n):
    return sorted(k for k in {1, 2, n - 1, n, max(1, n // 3)} if 1 <= k <= n)


def _ints(n, seed, hi):
    return np.random.default_rng(seed).integers(0, hi, n)


def _pat_rand(n):
    return pfc_rand_order(n, 11, n % 5)


def _pat_levels(n):
    return (_ints(n, 61 + n, 5).astype(f32) * f32(0.125) + f32(0.125)).astype(f32)


def _pat_equal(n):
    return np.full(n, 0.375, f32)


def _pat_zero(n):
    return np.zeros(n, f32)


def _pat_marks(n):
    v = _pat_rand(n).copy()
    v[np.random.default_rng(62 + n).permutation(n)[:min(n, TOPK_MARKS)]] = 2.0
    return v


def _pat_low10(n):
    """0.5 + j 2^-24, j < 1024: the values share their upper 22 bits — only the THIRD radix pass separates them"""
    return (f32(0.5) + _ints(n, 63 + n, 1024).astype(f32) * f32(2.0 ** -24)).astype(f32)


def _pat_mid11(n):
    """0.5 + (j << 10) 2^-24, j < 2048: the first pass sees one bin, the SECOND decides, the third sees equal digits"""
    return (f32(0.5) + (_ints(n, 64 + n, 2048) * 1024).astype(f32) * f32(2.0 ** -24)).astype(f32)


TOPK_PATTERNS = {"rand": _pat_rand, "levels": _pat_levels, "equal": _pat_equal, "zero": _pat_zero, "marks": _pat_marks, "low10": _pat_low10,
                 "mid11": _pat_mid11}


def topk_tie_case(n, edge):
    """the k-th value tied at positions edge - 2 ... edge + 2, G larger values elsewhere: k = G + 2 cuts the tie between edge - 1 and
    edge, k = G + 3 one later.  Returns (values, [k, k + 1])"""
    assert n >= edge + 3
    v = (_pat_rand(n) * f32(0.25)).astype(f32)                          # < 0.25
    big = np.random.default_rng(65 + n + edge).permutation(n)[:min(40, n // 4)]
    v[big] = 0.75
    tie = np.arange(edge - 2, edge + 3)
    v[tie] = 0.5
    G = int((v > 0.5).sum())
    return v, [G + 2, G + 3]


TOPK_TIE_CASES = [(2 * 16384 + 3, TOPK_CHUNK), (16384 + 3, TOPK_CHUNK), (8193, TOPK_ROUND), (8191, TOPK_ROUND), (1027, TOPK_ROUND)]


def topk_ref(v, k, mutant=None):
    """sorted(argsort(descending, stable)[:k]).  mutants: "last_tied" takes the LAST of the tied values; "no_third_pass" compares only the
    upper 22 bits"""
    v = np.asarray(v, f32)
    n = v.size
    if mutant == "last_tied":
        order = n - 1 - np.argsort(-v[::-1], kind="stable")
    elif mutant == "no_third_pass":
        order = np.argsort(-(v.view(np.int32) >> 10).astype(np.int64), kind="stable")
    else:
        order = np.argsort(-v.astype(f64), kind="stable")
    return np.sort(order[:k]).astype(np.int64)


def topk_npos(v):
    return int((np.asarray(v) == f32(2.0)).sum())


POSITIVE_N = [1, 1023, 1024, 1025, 5000]


def positive_cases(n):
    """{name: perm}: no positive, all positive, positives only at 0 and n - 1"""
    base = (_pat_rand(n) * f32(0.5)).astype(f32)
    ends = base.copy()
    ends[[0, n - 1]] = 2.0
    return {"none": base, "all": np.full(n, 2.0, f32), "ends": ends}


REMAP_N, REMAP_K = [1, 255, 256, 257], [1, 2, 1000]


def remap_inputs(n, k):
    """(labels, sorted index): labels -1 (untouched), present in the index, and absent from it: below, between and ABOVE every entry"""
    g = np.random.default_rng(70 + 7 * n + k)
    index = np.sort(g.permutation(3 * k + 5)[:k]).astype(np.int64) + 2
    lab = g.integers(0, int(index[-1]) + 3, n).astype(np.int64)
    special = [int(index[-1]) + 1, -1, int(index[0]), 0, int(index[-1])]
    lab[:min(n, len(special))] = special[:n]
    return lab, index


def remap_ref(label, index, side="left"):
    out = label.copy()
    m = label >= 0
    out[m] = np.searchsorted(index, label[m], side=side)
    return out


ROWS_K, ROWS_D = [1, 3, 4, 5, 101], [4, 8, 252, 256, 260, 512]
ROWS_PER_BLOCK, ROW_LANES = 4, 64                          # rows_kernel and contrastive_kernel: one 64-lane wave per row, four rows per block
ROWS_TABLE = 37
ROWS_BAD = (-1, ROWS_TABLE, 10 ** 9)


def rows_index(k):
    """k indices into a table of ROWS_TABLE rows, distinct where valid; as many of (negative, == nrows, 10^9) as fit are planted"""
    idx = np.random.default_rng(80 + k).permutation(ROWS_TABLE)[np.arange(k) % ROWS_TABLE].astype(np.int64)
    if k > ROWS_TABLE:
        idx[ROWS_TABLE:-1] = -5                              # a table row at most once: the scatter is then order-free
        idx[-1] = idx[1]                                     # (row 1 is handed to a bad index below; the LAST row stays valid)
    for j, b in enumerate(ROWS_BAD[:max(0, k - 1)]):         # rows 1, 2, 3: row 0 and, from k = 5, the last row stay valid
        idx[1 + j] = b
    return idx


def rows_valid(idx, nrows=ROWS_TABLE):
    return (idx >= 0) & (idx < nrows)


def rows_gather_ref(table, idx, k=None, fill=np.nan):
    """dst[i] = table[idx[i]] for the first k entries with a valid index; every other row (the guard rows behind k too) keeps ``fill``"""
    k = len(idx) if k is None else k
    out = np.full((len(idx), table.shape[1]), fill, f32)
    ok = rows_valid(idx, len(table)) & (np.arange(len(idx)) < k)
    out[ok] = table[idx[ok]]
    return out


def rows_scatter_ref(table, src, idx, k=None):
    k = len(idx) if k is None else k
    out = table.copy()
    ok = rows_valid(idx, len(table)) & (np.arange(len(idx)) < k)
    out[idx[ok]] = src[ok]
    return out


def chain_ref(num_local, num_sample, label, class_start, seed, step, weight, mom):
    """what partial_fc.py does with these calls: draw, localize (marks 2.0), top-k — or, with more positives than samples, the positives
    — remap, gather; the caller's edit (w -> -w, m -> m / 2, both exact); scatter.  Returns a dict of every intermediate"""
    perm = pfc_rand_order(num_local, seed, step)
    loc, perm_t = tc.pfc_localize_ref(torch.from_numpy(label), class_start, num_local, torch.from_numpy(perm))
    perm, loc = perm_t.numpy(), loc.numpy()
    index = topk_ref(perm, num_sample)
    npos = topk_npos(perm)
    if npos > num_sample:
        index = np.flatnonzero(perm == f32(2.0)).astype(np.int64)
    lab = remap_ref(loc, index)
    sub_w, sub_m = weight[index], mom[index]
    w2, m2 = weight.copy(), mom.copy()
    w2[index], m2[index] = -sub_w, sub_m * f32(0.5)
    return {"perm": perm, "index": index, "npos": npos, "label": lab, "sub_w": sub_w, "sub_m": sub_m, "weight": w2, "mom": m2}


CHAIN_CASES = [(8200, 820, 64, False), (2000, 200, 64, False), (8200, 16, 64, True), (2000, 16, 64, True)]     # (num_local, num_sample, batch, positives win)


def chain_labels(num_local, batch, class_start):
    g = np.random.default_rng(90 + num_local)
    lab = class_start + g.permutation(num_local)[:batch].astype(np.int64)                 # distinct classes of this shard
    lab[::8] = class_start - 1 - np.arange(len(lab[::8]))                                  # some outside it
    lab[1] = class_start + num_local
    return lab


# ================================================================================================ contrastive
CON_B, CON_D, CON_T = [1, 3, 4, 5, 9], [1, 63, 64, 65, 96, 512], [0.5, 0.07]
CON_EPS = 1e-8
CON_SPECIAL = ("x_eq_g", "x_eq_neg_g", "g_eq_l", "x_zero", "underflow")       # rows 0 ... 4 as far as B reaches


def con_inputs(B, D):
    s = 5000 + 31 * B + D
    x, g, l = uniform((B, D), s), uniform((B, D), s + 1), uniform((B, D), s + 2)
    cancel = torch.zeros(B, dtype=torch.bool)
    if D == 1:
        cancel[:] = True
    for r, kind in enumerate(CON_SPECIAL[:B]):
        if kind == "x_eq_g":
            x[r] = g[r]
        elif kind == "x_eq_neg_g":
            x[r] = -g[r]
        elif kind == "g_eq_l":
            l[r] = g[r]
            cancel[r] = True
        elif kind == "x_zero":
            x[r] = 0.0
        else:
            x[r] = g[r]
            l[r] = -g[r] + 0.5 * uniform((D,), s + 3)          # cos(x, l) near -1 but l keeps a part orthogonal to x (D > 1)
    return x, g, l, cancel


def con_ref(x, g, l, T, cancel, dt=torch.float64):
    """{"row_loss": Q, "dx": Q (held transposed, [D][B])}: CE([cos(x, g) / T, cos(x, l) / T], 0) per row, dx = d mean / dx by autograd; every norm clamped at 1e-8"""
    x = x.to(dt).requires_grad_(True)
    g, l = g.to(dt), l.to(dt)
    B = x.shape[0]
    nx, ng, nl = (t.norm(dim=1).clamp_min(CON_EPS) for t in (x, g, l))
    cg, cl = (x * g).sum(1) / (nx * ng), (x * l).sum(1) / (nx * nl)
    pos, neg = cg / T, cl / T
    loss = torch.logsumexp(torch.stack([pos, neg], 1), 1) - pos
    loss.mean().backward()
    dx = x.grad
    with torch.no_grad():
        w = torch.softmax(torch.stack([pos, neg], 1), 1)[:, 1] / T / B
        kg, kl, kx = -w / (nx * ng), w / (nx * nl), (w * cg - w * cl) / (nx * nx)
        terms = (kg[:, None] * g).abs() + (kl[:, None] * l).abs() + (kx[:, None] * x).abs()
        scale = torch.where(cancel, terms.amax(1), dx.abs().amax(1)).to(torch.float64)
    loss = loss.detach()
    return {"row_loss": Q(loss, "loss", loss.abs().clamp_min(1.0)), "dx": Q(dx.t(), "grad", scale)}


def con_check(got, ref, key, what="", frac=1.0, out=None):
    """tail_cases.check on row_loss [B] or dx [B][D]: dx goes in TRANSPOSED, so the columns the check takes its maxima over are dx's rows
    (a row is what one wave produces); the figure that goes to ``out`` is a fraction of the tolerance"""
    g = got.detach().to("cpu")
    check(g.t() if key == "dx" else g, ref[key], what, frac, out)


def _wave_sum(v):
    """[B][64] lane partials -> [B]: the butterfly of a 64-lane wave in fp32"""
    while v.shape[1] > 1:
        h = v.shape[1] // 2
        v = v[:, :h] + v[:, h:]
    return v[:, 0]


def con_kernel_order(x, g, l, T, mutant=None):
    """the kernel's arithmetic at fp32: 64 lane partials over i, i + 64, ..., the wave sum, the closed-form gradient.
    mutant "row_ge": the last row is not computed (NaN); "lanes": the lanes above D % 64 of the last trip are dropped"""
    B, D = x.shape
    f = torch.float32
    pad = cdiv(D, 64) * 64 - D

    def lanes(a, b):
        pr = torch.nn.functional.pad(a * b, (0, pad)).view(B, -1, 64)
        if mutant == "lanes" and D > 64:
            pr = pr[:, :-1]
        acc = torch.zeros(B, 64, dtype=f)
        for t in range(pr.shape[1]):
            acc = acc + pr[:, t]
        return _wave_sum(acc)

    eps, inv_t = torch.tensor(CON_EPS, dtype=f), torch.tensor(1.0, dtype=f) / torch.tensor(T, dtype=f)
    nx, ng, nl = (torch.maximum(torch.sqrt(lanes(a, a)), eps) for a in (x, g, l))
    cg, cl = lanes(x, g) / (nx * ng), lanes(x, l) / (nx * nl)
    pos, neg = cg * inv_t, cl * inv_t
    mx = torch.maximum(pos, neg)
    lse = mx + torch.log(torch.exp(pos - mx) + torch.exp(neg - mx))
    w = torch.exp(neg - lse) * inv_t / torch.tensor(float(B), dtype=f)
    kg, kl, kx = -w / (nx * ng), w / (nx * nl), (w * cg - w * cl) / (nx * nx)
    dx = kg[:, None] * g + kl[:, None] * l + kx[:, None] * x
    loss = lse - pos
    if mutant == "row_ge":
        loss, dx = loss.clone(), dx.clone()
        loss[-1], dx[-1] = math.nan, math.nan
    assert dx.dtype == f and loss.dtype == f
    return {"row_loss": loss, "dx": dx}


# ================================================================================================ colflag
CF_M, CF_N, CF_K = [1, 37, 65], [1, 63, 64, 65, 130], [1, 15, 16, 17, 96, 100]
CF_ALPHA = 0.25
CF_AMAX, CF_BMAX = 2, 1
CF_TILE = 64


def cf_admissible(K):
    return K * CF_AMAX * CF_BMAX < 2 ** 24


def cf_operands(M, N, K):
    """a [M][K] in {1, 2}, b [N][K] in {-1, 0, 1}; every third column of the score matrix is all -1 (its scores are -sum_k a <= -K < 0)"""
    g = torch.Generator().manual_seed(6000 + 131 * M + 17 * N + K)
    a = torch.randint(1, CF_AMAX + 1, (M, K), generator=g).to(torch.float32)
    b = torch.randint(-CF_BMAX, CF_BMAX + 1, (N, K), generator=g).to(torch.float32)
    b[::3] = -1.0
    return a, b


def cf_scores(a, b, row_mask=True):
    """alpha a b^T in float64 (exact).  row_mask False: the mutant that also sees the zero rows padding M to the 64-row tile"""
    s = CF_ALPHA * (a.double() @ b.double().t())
    if not row_mask and a.shape[0] % CF_TILE:
        s = torch.cat([s, torch.zeros(CF_TILE - a.shape[0] % CF_TILE, s.shape[1], dtype=torch.float64)])
    return s


def cf_thresholds(a, b):
    """{name: thr}, every one an ATTAINED score (exact in fp32): the largest (nothing is flagged), the median of the column maxima, the
    largest score of the all-negative columns and the median of their maxima (negative: the padded zero rows would exceed them)"""
    s = cf_scores(a, b)
    colmax = s.amax(0)
    neg = colmax[::3]
    out = {"max": float(s.max()), "median": float(colmax.sort().values[len(colmax) // 2]),
           "neg_max": float(neg.max()), "neg_median": float(neg.sort().values[len(neg) // 2])}
    assert all(float(np.float32(t)) == t for t in out.values()) and out["neg_max"] < 0
    return out


def cf_flags(a, b, thr, ge=False, row_mask=True):
    s = cf_scores(a, b, row_mask)
    return ((s >= thr) if ge else (s > thr)).any(0).to(torch.uint8)


# ================================================================================================ class_accumulate
CA_B, CA_D, CA_C = [1, 7, 1024, 1025, 2500], [1, 64, 255, 256, 257, 512], [1, 5, 33]
CA_SLICE = 1024
CA_BAD = (-1, None, 10 ** 12)                              # None: the class count C itself


def ca_labels(B, C):
    """label vectors: random classes with -1, C and 10^12 planted (B == 1: one vector per kind, and a valid one)"""
    bad = [C if b is None else b for b in CA_BAD]
    if B < 7:
        return [np.array([v], dtype=np.int64) for v in [C - 1] + bad]
    lab = np.random.default_rng(7000 + B + C).integers(0, C, B).astype(np.int64)
    if C == 33:
        lab[lab % 4 == 1] = 0                                # classes 1, 5, 9, ... have no row at all
    lab[[1, B // 2, B - 1]] = bad
    return [lab]


def ca_inputs(B, D, C):
    s = 7100 + B + 3 * D + C
    return uniform((B, D), s).numpy(), uniform((C, D), s + 1).numpy(), np.random.default_rng(s).integers(0, 5, C).astype(f32)


def _pairwise(a):
    while a.shape[0] > 1:
        if a.shape[0] % 2:
            a = np.concatenate([a, np.zeros((1,) + a.shape[1:], f32)])
        a = a[0::2] + a[1::2]
    return a[0]


def ca_order(x, label, sums, counts, mutant=None):
    """the kernel's order in numpy fp32: per class, per 1024-row slice of the batch, a sequential sum in batch order from 0, then added to
    sums; counts += the slice's row count.  mutant "pairwise": the slice sum as a tree"""
    sums, counts = sums.copy(), counts.copy()
    B = len(label)
    for c in range(len(counts)):
        for b0 in range(0, B, CA_SLICE):
            rows = b0 + np.flatnonzero(label[b0:b0 + CA_SLICE] == c)
            if rows.size == 0:
                continue
            s = _pairwise(x[rows]) if mutant == "pairwise" else np.cumsum(x[rows], axis=0, dtype=f32)[-1]
            sums[c] = sums[c] + s
            counts[c] = counts[c] + f32(rows.size)
    assert sums.dtype == f32 and counts.dtype == f32
    return sums, counts


def ca_ref64(x, label, sums):
    """(float64 sums, |sums| + sum |terms|)"""
    C = len(sums)
    ok = (label >= 0) & (label < C)
    r, s = sums.astype(f64), np.abs(sums).astype(f64)
    np.add.at(r, label[ok], x[ok].astype(f64))
    np.add.at(s, label[ok], np.abs(x[ok]).astype(f64))
    return r, s


def ca_check(got_s, got_c, x, label, sums, counts, what="", frac=1.0, out=None, order=True):
    r, s = ca_ref64(x, label, sums)
    err = np.abs(got_s.astype(f64) - r) / (s + TINY)
    worst = float(np.nan_to_num(err, nan=np.inf).max()) / TOL["fwd"]
    if out is not None:
        out.append((what, "fwd", worst))
    assert worst <= frac, "%s: class sums are %.3g of the tolerance from float64" % (what, worst)
    if order:
        ws, wc = ca_order(x, label, sums, counts)
        same32(got_s, ws, what + " sums vs the stated order")
        same32(got_c, wc, what + " counts")
        absent = ~np.isin(np.arange(len(counts)), label)
        same32(got_s[absent], sums[absent], what + " sums of classes with no row")


# ================================================================================================ ROC histogram
ROC_N, ROC_D, ROC_NBIN = 130, [1, 15, 17, 20], 4002
ROC_T = [1, 64, 65, ROC_N]


def roc_inputs(D):
    """features k / 8: |k| <= 12 at D == 1 (|dot| up to 2.25: both clamps), |k| <= 3 otherwise (dots between about -2 and 2)"""
    g = np.random.default_rng(8000 + D)
    kmax = 12 if D == 1 else 3
    return (g.integers(-kmax, kmax + 1, (ROC_N, D)) / 8.0).astype(f32), g.integers(0, 5, ROC_N).astype(np.int64)


def roc_ref(feat, label, T):
    """roc_slot in float64 numpy: bin = clamp(trunc((s + 1) * 1000), 0, 2000); slot 2 bin + (labels differ)"""
    N = len(feat)
    s = feat.astype(f64) @ feat.astype(f64).T
    a, b = np.meshgrid(np.arange(N), np.arange(N), indexing="ij")
    m = (a < b) & (a < T)
    bins = np.clip(np.trunc((s[m] + 1.0) * 1000.0), 0, 2000).astype(np.int64)
    slot = 2 * bins + (label[a[m]] != label[b[m]])
    return np.bincount(slot, minlength=ROC_NBIN).astype(np.uint64)


# ================================================================================================ input path
PRE_GRID_CAP, PAD_GRID_CAP = 8192, 16384                   # ew.hip: blocks of 256 threads, one pixel / one group of eight channels each
PRE_SHAPES = [(4, 64, 1), (4, 32, 2), (3, 5, 111), (2, 3, 112)]          # (B, H, W): W odd, even, one
PRE_WRAP = (3, 840, 840)
PRE_FLIPS = ("null", "zeros", "ones", "mixed")


def pre_input(B, H, W):
    """uint8 [B][H][W][3]: pixel i holds (7 i + 85 c) mod 256 in channel c — every byte value in every channel once B H W >= 256"""
    i = np.arange(B * H * W, dtype=np.int64)[:, None]
    return ((7 * i + 85 * np.arange(3)[None]) % 256).astype(np.uint8).reshape(B, H, W, 3)


def pre_flip(B, kind):
    return {"null": None, "zeros": np.zeros(B, np.uint8), "ones": np.ones(B, np.uint8), "mixed": (np.arange(B) % 2).astype(np.uint8) * 3}[kind]


def pre_ref(u8, flip):
    """torchvision's ToTensor + Normalize(0.5, 0.5) on the CPU, the flagged images mirrored"""
    t = torch.from_numpy(u8).permute(0, 3, 1, 2).float().div(255).sub(0.5).div(0.5)
    if flip is not None:
        t = torch.where(torch.from_numpy(flip != 0)[:, None, None, None], t.flip(3), t)
    return t.contiguous()


PAD_CC = [(3, 64), (1, 8), (8, 8), (3, 8), (64, 64), (5, 16)]
PAD_HW = [1, 7, 400]
PAD_WRAP = (2, 3, 262150, 64)                              # (B, C, HW, Cpad): B HW Cpad / 8 = 4 194 400 groups > 16384 x 256


def pad_ref(x, Cpad, s16, mutant=None):
    """[B][C][HW] fp32 -> [B][HW][Cpad] 16-bit, exact zeros in the pad channels.  mutant "copy0": the pad channels repeat channel 0"""
    B, C, HW = x.shape
    out = torch.zeros(B, HW, Cpad, dtype=s16)
    out[:, :, :C] = x.permute(0, 2, 1).to(s16)
    if mutant == "copy0" and Cpad > C:
        out[:, :, C:] = x[:, 0, :, None].to(s16)
    return out
