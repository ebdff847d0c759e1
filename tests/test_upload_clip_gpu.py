"""The clip and the Gaussian mechanism on compressed and top-k uploads, on the GPU: fedfr_delta_sqnorm / fedfr_sparse_sqnorm against the
correctly rounded sums of tests/upload_clip_cases.py (relative error <= B 2^-52, B the number of terms), their coefficients against
fedopt_cases.clip_coef on the device's own sums, determinism on a NaN-filled workspace, what lies behind n, the violation counter;
fedfr_delta_aggregate_dp / fedfr_sparse_aggregate_dp bit for bit against the existing restatements with ws := the device's coefficients and
the noise read back from fedfr_gaussian_fill; argument errors with sentinels behind every output; and the Python surface
(server.UploadClip, FedCompressed / FedSparse with clip and mech, Server.train with clip_uploads)."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import compress_cases as Q  # noqa: E402
import dp_cases as D  # noqa: E402
import fedopt_cases as F  # noqa: E402
import sparse_cases as S  # noqa: E402
import test_compress_gpu as TC  # noqa: E402   (its synthetic states and tiny world: helpers, not tests)
import upload_clip_cases as U  # noqa: E402

from fedfr_amd import _C, compress, privacy, server  # noqa: E402

DEV = torch.device("cuda:0")
f32, f64 = np.float32, np.float64
SENT, SENT_D, SENT_I = -777.25, -777.25, 0x7A5A5A5A
GUARD = 16
G, N, ptr, ptrs_of = TC.G, TC.N, TC.ptr, TC.ptrs_of
bits_of = Q.bits_of


def wvec(ws):
    return (C.c_float * len(ws))(*[float(w) for w in ws])


@functools.lru_cache(maxsize=None)
def z_of(n, seed=U.SEED, rnd=U.ROUND, sid=U.SID, offset=0):
    """the n standard normal values of the stream as the device draws them (std = 1: 0 + 1 * z), read back once and shared"""
    out = torch.empty(n, device=DEV)
    assert _C.lib().fedfr_gaussian_fill(ptr(out), n, seed, rnd, sid, offset, 1.0, 0, _C.stream()) == 0, _C.last_error()
    z = N(out)
    z.flags.writeable = False
    return z


class Norms:
    """sq / coef / violations with sentinels behind them and a workspace of exactly the size the library asks for (+ a guard)"""

    def __init__(self, k, m):
        self.k = k
        self.need = int(_C.lib().fedfr_upload_sqnorm_workspace_bytes(k, m))
        assert self.need == k * Q.grid(m) * 8
        self.wsp = torch.full((self.need // 8 + GUARD,), SENT_D, dtype=torch.float64, device=DEV)
        self.reset()

    def reset(self, workspace_fill=None):
        self.sq = torch.full((self.k + GUARD,), SENT_D, dtype=torch.float64, device=DEV)
        self.coef = torch.full((self.k + GUARD,), SENT, dtype=torch.float32, device=DEV)
        self.viol = torch.full((self.k + GUARD,), SENT_I, dtype=torch.int32, device=DEV)
        self.viol[:self.k] = 0
        if workspace_fill is not None:
            self.wsp[:self.need // 8] = workspace_fill

    def read(self, what):
        torch.cuda.synchronize()
        sq, coef, viol, w = N(self.sq), N(self.coef), N(self.viol), N(self.wsp)
        assert np.all(sq[self.k:] == SENT_D) and np.all(coef[self.k:] == f32(SENT)) and np.all(viol[self.k:] == SENT_I), what + ": wrote behind an output"
        assert np.all(w[self.need // 8:] == SENT_D), what + ": wrote behind the workspace"
        return sq[:self.k].copy(), coef[:self.k].copy(), viol[:self.k].copy()


def delta_sqnorm(o, dups, ws, bits, n, clip, what=""):
    rc = _C.lib().fedfr_delta_sqnorm(ptrs_of([u[0] for u in dups]), ptrs_of([u[1] for u in dups]), wvec(ws), len(dups), bits, n, float(clip), ptr(o.sq),
                                     ptr(o.coef), ptr(o.wsp), o.need, _C.stream())
    assert rc == 0, _C.last_error()
    return o.read(what)[:2]


def sparse_sqnorm(o, dups, ws, n, clip, what=""):
    keeps = (C.c_size_t * len(dups))(*[u[2] for u in dups])
    rc = _C.lib().fedfr_sparse_sqnorm(ptrs_of([u[0] for u in dups]), ptrs_of([u[1] for u in dups]), keeps, wvec(ws), len(dups), n, float(clip), ptr(o.sq),
                                      ptr(o.coef), ptr(o.viol), ptr(o.wsp), o.need, _C.stream())
    assert rc == 0, _C.last_error()
    return o.read(what)


def same64(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def check_norm_pass(run, refs, terms, ws, what):
    """the common law of both norm passes.  ``run(clip, workspace_fill)`` -> (sq, coef); ``refs``: the correctly rounded sums (NaN: the
    upload carries a NaN block); ``terms``: B per upload"""
    k = len(refs)
    sq0, coef0 = run(0.0, None)
    assert np.array_equal(bits_of(coef0), bits_of(np.array(ws[:k], dtype=f32))), what + ": clip = 0 must return the weights"
    for i, (ref, b) in enumerate(zip(refs, terms)):
        if math.isnan(ref):
            assert math.isnan(sq0[i]), (what, i)
            continue
        err = U.rel_err(float(sq0[i]), ref)
        print("%s upload %d: sq %.17g, rel err %.3g of %.3g allowed" % (what, i, sq0[i], err, U.tolerance(b)))
        assert err <= U.tolerance(b), (what, i, sq0[i], ref)
    finite = sq0[np.isfinite(sq0)]
    if finite.size == 0 or finite.max() == 0.0:
        return sq0, coef0
    clip = f32(0.75 * math.sqrt(finite.max()))
    sq1, coef1 = run(clip, None)
    sq2, coef2 = run(clip, float("nan"))                                  # the second run: on a workspace full of NaN
    assert same64(sq1, sq0) and same64(sq2, sq1) and np.array_equal(bits_of(coef2), bits_of(coef1)), what + ": two runs differ"
    want = F.clip_coef(sq1, ws[:k], clip)
    w32 = np.array(ws[:k], dtype=f32)
    for i in range(k):
        if math.isnan(sq1[i]) or sq1[i] == 0.0:
            assert bits_of(coef1[i:i + 1])[0] == bits_of(w32[i:i + 1])[0], (what, i)      # the comparison fails: coef = w
        else:
            assert abs(float(coef1[i]) - float(want[i])) <= float(np.spacing(want[i])), (what, i, coef1[i], want[i])
    top = int(np.nanargmax(np.where(np.isfinite(sq1), sq1, -1.0)))
    assert coef1[top] < w32[top], what + ": the largest upload was not clipped"
    return sq1, coef1


# ---- fedfr_delta_sqnorm ------------------------------------------------------------------------------------------------------------------
def dev_codes(ups):
    return [(G(c), G(s)) for c, s in ups]


def check_delta_sqnorm(ups, bits, n, what):
    dups, k = dev_codes(ups), len(ups)
    o = Norms(k, n)

    def run(clip, fill):
        o.reset(fill)
        return delta_sqnorm(o, dups, U.WS[:k], bits, n, clip, what)
    out = check_norm_pass(run, [U.delta_sqnorm(c, s, bits, n) for c, s in ups], [Q.scale_bytes(n)] * k, U.WS, what)
    for (dc, ds), (c, s) in zip(dups, ups):
        assert np.array_equal(N(dc), c) and np.array_equal(N(ds), s)        # read, never written
    return out


@pytest.mark.parametrize("k", [1, 3, 8])
@pytest.mark.parametrize("n", Q.SIZES)
@pytest.mark.parametrize("bits", Q.BITS)
def test_delta_sqnorm_against_the_correctly_rounded_sum(bits, n, k):
    """the sine client states through the numpy quantiser; below / at / above one and two blocks, units of 8 that end before, at and behind n"""
    sq, _ = check_delta_sqnorm(U.quantized_uploads(n, k, bits), bits, n, "sine bits=%d n=%d k=%d" % (bits, n, k))
    assert np.all(sq > 0)


@pytest.mark.parametrize("bits", Q.BITS)
def test_delta_sqnorm_grid_stride_wrap(bits):
    """n = 2048 * 256 * 8 + 37: the capped grid, the wrap onto the first threads, and a last unit of 5 elements; the tolerance is 3e-11"""
    n = Q.BIG
    assert Q.grid(n) == Q.GRID_CAP and 2e-11 < U.tolerance(Q.scale_bytes(n)) < 4e-11
    check_delta_sqnorm(U.quantized_uploads(n, 2, bits), bits, n, "sine bits=%d BIG" % bits)


@pytest.mark.parametrize("short,copies", [(1, 2), (31, 1)])
@pytest.mark.parametrize("bits", Q.BITS)
def test_delta_sqnorm_edge_blocks(bits, short, copies):
    """the quantiser's edge blocks: as they are (NaN blocks: sq is NaN and coef = w) and with the reserved scale byte replaced by 0 and 180
    (finite: held to the tolerance; the ends of the range themselves: the next test)"""
    x, xi = Q.edge_blocks(bits, short, copies)
    n = x.size
    codes, scales = Q.quantize(x, xi, None, bits)[:2]
    assert np.count_nonzero(scales == 255) >= 4
    o = Norms(1, n)
    sq, coef = delta_sqnorm(o, dev_codes([(codes, scales)]), U.WS[:1], bits, n, 0.5, "edge")
    assert math.isnan(sq[0]) and bits_of(coef)[0] == bits_of(np.array(U.WS[:1]))[0]
    ends = scales.copy()
    ends[scales == 255] = np.where(np.arange(np.count_nonzero(scales == 255)) % 2 == 0, 0, 180).astype(np.uint8)
    ends[ends > 200] = 200                                                    # (the block at the top of the fp32 range: a clip of its size would not fit fp32)
    hashed = U.hashed_uploads(n, 1, bits)[0][0]                               # (the NaN blocks' codes are 0: give those blocks something to count)
    check_delta_sqnorm([(codes, ends), (hashed, ends)], bits, n, "edge, finite, bits=%d short=%d" % (bits, short))


@pytest.mark.parametrize("bits", Q.BITS)
def test_delta_sqnorm_zero_extreme_codes_and_what_lies_behind_n(bits):
    n = 4103
    zero = (np.zeros(Q.code_bytes(bits, n), dtype=np.uint8), np.full(Q.scale_bytes(n), 130, dtype=np.uint8))
    o = Norms(2, n)
    one = U.quantized_uploads(n, 1, bits)[0]
    sq, coef = delta_sqnorm(o, dev_codes([zero, one]), U.WS[:2], bits, n, 1e-6, "zero")
    assert sq[0] == 0.0 and not np.signbit(sq[0]) and bits_of(coef)[0] == bits_of(np.array(U.WS[:1]))[0] and coef[1] < U.WS[1]
    # the most negative code, which the quantiser never produces: counted as 128^2 / 8^2, what the aggregate would apply
    lowest = (np.full(Q.code_bytes(bits, n), 0x80 if bits == 8 else 0x88, dtype=np.uint8), np.full(Q.scale_bytes(n), 127, dtype=np.uint8))
    if bits == 4:
        lowest[0][-1] = 0x08                                                  # (n is odd: the pad nibble stays 0 here)
    o = Norms(1, n)
    sq, _ = delta_sqnorm(o, dev_codes([lowest]), U.WS[:1], bits, n, 0.0, "lowest code")
    assert sq[0] == n * float(1 << (bits - 1)) ** 2 == U.delta_sqnorm(*lowest, bits, n)
    # the two ends of the scale range on every block: 4^-127 and 4^127 (the sum stays inside fp64; a clip of its size would not fit fp32)
    for eb in (0, 254):
        ends = (U.hashed_uploads(n, 1, bits)[0][0], np.full(Q.scale_bytes(n), eb, dtype=np.uint8))
        o = Norms(1, n)
        sq, coef = delta_sqnorm(o, dev_codes([ends]), U.WS[:1], bits, n, 0.0, "eb=%d" % eb)
        assert 0 < sq[0] < np.inf and U.rel_err(float(sq[0]), U.delta_sqnorm(*ends, bits, n)) <= U.tolerance(Q.scale_bytes(n)) and coef[0] == U.WS[0], (bits, eb)
    # garbage behind n: (a) the pad nibble of an odd 4-bit n; (b) a last block padded with non-zero codes up to 32 (the buffer is longer than
    # ceil(n bits / 8)); (c) n a multiple of 8 but not of 32: whole units of the last block lie behind n.  sq is what it is with zeros there
    for m in (37, 40, 1001):
        codes, scales = U.hashed_uploads(m, 1, bits)[0]
        nb = Q.scale_bytes(m)
        clean = np.zeros(nb * 32 * bits // 8, dtype=np.uint8)
        clean[:codes.size] = codes
        if bits == 4 and m % 2:
            clean[codes.size - 1] &= 0x0F
        dirty = np.full(nb * 32 * bits // 8, 0x7F, dtype=np.uint8)
        dirty[:codes.size] = codes
        if bits == 4 and m % 2:
            dirty[codes.size - 1] |= 0x70
        o = Norms(2, m)
        sq, _ = delta_sqnorm(o, dev_codes([(clean, scales), (dirty, scales)]), U.WS[:2], bits, m, 0.0, "behind n")
        assert sq[0] == sq[1] > 0 and U.rel_err(float(sq[0]), U.delta_sqnorm(codes, scales, bits, m)) <= U.tolerance(nb), (bits, m)


# ---- fedfr_sparse_sqnorm -----------------------------------------------------------------------------------------------------------------
def dev_sparse(ups):
    """(idx, val, keep) on the device; an upload without entries still has a buffer (the entry point refuses a null pointer)"""
    return [(G(np.concatenate([i, np.zeros(4, np.uint32)]).view(np.int32)), G(np.concatenate([v, np.full(4, 9.0, f32)])), i.size) for i, v in ups]


def check_sparse_sqnorm(ups, n, what):
    dups, k = dev_sparse(ups), len(ups)
    o = Norms(k, max(i.size for i, _ in ups))

    def run(clip, fill):
        o.reset(fill)
        sq, coef, viol = sparse_sqnorm(o, dups, U.WS[:k], n, clip, what)
        assert np.all(viol == 0), (what, viol)
        return sq, coef
    return check_norm_pass(run, [U.sparse_sqnorm(v) for _, v in ups], [i.size for i, _ in ups], U.WS, what)


@pytest.mark.parametrize("shape", S.UPLOAD_SHAPES)
@pytest.mark.parametrize("n", S.AGG_SIZES)
def test_sparse_sqnorm_against_the_correctly_rounded_sum(n, shape):
    """k = 1 and k = 8 with the differing keeps of the shapes, one upload of the eight without entries (sq = 0, coef = w)"""
    ups = list(S.uploads(n, shape))
    check_sparse_sqnorm(ups[:1], n, "%s n=%d k=1" % (shape, n))
    ups[3] = (ups[3][0][:0], ups[3][1][:0])
    sq, coef = check_sparse_sqnorm(ups, n, "%s n=%d k=8" % (shape, n))
    assert sq[3] == 0.0 and coef[3] == U.WS[3]


def test_sparse_sqnorm_many_blocks():
    """keep = n / 3 at n = 2048 * 256 * 8 + 37: several hundred workgroups, each thread several entries; and non-finite values: NaN in, NaN out"""
    n = S.BIG
    idx = np.arange(0, n, 3).astype(np.uint32)
    val = S._vals(idx, 1)
    sq, _ = check_sparse_sqnorm([(idx, val), (idx[:7], val[:7])], n, "every third of BIG")
    bad = val.copy()
    bad[12345] = np.nan
    o = Norms(1, idx.size)
    sq, coef, viol = sparse_sqnorm(o, dev_sparse([(idx, bad)]), U.WS[:1], n, 0.5, "NaN")
    assert math.isnan(sq[0]) and coef[0] == U.WS[0] and viol[0] == 0


def test_sparse_sqnorm_counts_violations_exactly():
    """one duplicate, one descending pair and one index = n per upload, placed inside a wave, at the boundary between two waves, between two
    workgroups (entry 256 belongs to the first thread of the second workgroup and looks back at the last thread of the first) and at the
    last entry; the counter is ADDED to, and the norms do not depend on the indices"""
    n, keep = 20000, 5000
    assert Q.grid(keep) >= 2
    base = (np.arange(keep) * 3).astype(np.uint32)
    val = S._vals(base, 0)
    ups, want = [], []
    for dup, desc, at_n in ((100, 300, keep - 1), (64, 256, 4097), (256, 63, keep - 1), (255, 2, 512)):
        idx = base.copy()
        idx[dup] = idx[dup - 1]                                               # a duplicate: idx_e == idx_(e-1)
        idx[desc] = idx[desc - 1] - 1                                         # a descending pair (the entry behind it ascends again)
        idx[at_n] = n                                                         # out of range (and above its neighbours' indices: one violation,
        ups.append((idx, val))                                                #  plus one where the entry behind it is now "not ascending")
        want.append(U.violations(idx, n))
    assert want == [3 + (1 if a < keep - 1 else 0) for a in (keep - 1, 4097, keep - 1, 512)]
    dups = dev_sparse(ups + [(base, val)])
    o = Norms(5, keep)
    o.viol[:5] = torch.tensor([0, 10, 0, 0, 7], dtype=torch.int32)
    sq, _, viol = sparse_sqnorm(o, dups, U.WS[:5], n, 1.0, "violations")
    assert viol.tolist() == [want[0], 10 + want[1], want[2], want[3], 7]
    assert all(same64(sq[i:i + 1], sq[4:5]) for i in range(4))


# ---- fedfr_delta_aggregate_dp ------------------------------------------------------------------------------------------------------------
def delta_dp(buf, base_ptr, dups, coef_t, bits, n, accumulate, last, std, offset=0, stream=(U.SEED, U.ROUND, U.SID)):
    rc = _C.lib().fedfr_delta_aggregate_dp(ptr(buf), base_ptr, ptrs_of([u[0] for u in dups]), ptrs_of([u[1] for u in dups]), ptr(coef_t), len(dups), bits,
                                           n, accumulate, last, float(std), *stream, offset, _C.stream())
    assert rc == 0, _C.last_error()
    torch.cuda.synchronize()


def sparse_dp(buf, base_ptr, dups, coef_t, n, accumulate, last, std, offset=0, stream=(U.SEED, U.ROUND, U.SID)):
    keeps = (C.c_size_t * len(dups))(*[u[2] for u in dups])
    rc = _C.lib().fedfr_sparse_aggregate_dp(ptr(buf), base_ptr, ptrs_of([u[0] for u in dups]), ptrs_of([u[1] for u in dups]), keeps, ptr(coef_t), len(dups),
                                            n, accumulate, last, float(std), *stream, offset, _C.stream())
    assert rc == 0, _C.last_error()
    torch.cuda.synchronize()


def agg_uploads(n, k, bits):
    """hashed uploads whose dq are finite in fp32, and one NaN block in the second upload where there are blocks enough"""
    ups = U.hashed_uploads(n, k, bits, top=240)
    if k > 1 and Q.scale_bytes(n) > 20:
        ups[1][1][17] = 255
    return ups


def device_coef(ups, bits, n, k):
    """the coefficients as the norm pass leaves them on the device (a clip that bites), as a tensor with a guard, and as numpy"""
    dups = dev_codes(ups[:k]) if bits else dev_sparse(ups[:k])
    o = Norms(k, n if bits else max(i.size for i, _ in ups[:k]))
    sq = (delta_sqnorm(o, dups, U.WS[:k], bits, n, 0.0) if bits else sparse_sqnorm(o, dups, U.WS[:k], n, 0.0))[0]
    fin = sq[np.isfinite(sq)]
    clip = f32(0.75 * math.sqrt(fin.max())) if fin.size and fin.max() > 0 else f32(1.0)
    o.reset()
    coef = (delta_sqnorm(o, dups, U.WS[:k], bits, n, clip) if bits else sparse_sqnorm(o, dups, U.WS[:k], n, clip))[1]
    return dups, o.coef, coef


def check_dp_aggregate(bits, n, ks, ups, what, accumulates=(0, 1), bases=("null", "distinct", "dst"), stds=(0.0, U.NOISE_STD)):
    """bits = 0: the sparse pair of entry points.  Every k x noise off / on x accumulate x base against the restatement with ws := the
    device's coefficients; the noise-free call on the fp32 weights against the existing entry point, bit for bit"""
    j = np.arange(n, dtype=f64)
    dst0 = (0.4 * np.sin(0.77 * j + 1.3)).astype(f32)
    x = (0.5 * np.sin(0.37 * j + 0.1)).astype(f32)
    xd, d0 = G(x), G(dst0)
    z = z_of(n)
    for k in ks:
        dups, coef_t, coef = device_coef(ups, bits, n, k)
        for std in stds:
            for accumulate in accumulates:
                for base in bases:
                    buf = torch.full((n + GUARD,), SENT, dtype=torch.float32, device=DEV)
                    buf[:n] = d0
                    bp = {"null": None, "distinct": ptr(xd), "dst": ptr(buf)}[base]
                    bn = {"null": None, "distinct": x, "dst": dst0}[base]
                    if bits:
                        delta_dp(buf, bp, dups, coef_t, bits, n, accumulate, 1, std)
                        ref = U.delta_dp(dst0, bn, ups[:k], coef, bits, n, accumulate, std, z)
                    else:
                        sparse_dp(buf, bp, dups, coef_t, n, accumulate, 1, std)
                        ref = U.sparse_dp(dst0, bn, ups[:k], coef, n, bool(accumulate), std, z)
                    got = N(buf)
                    tag = "%s n=%d k=%d std=%g accumulate=%d base=%s" % (what, n, k, std, accumulate, base)
                    assert np.all(got[n:] == f32(SENT)), tag + ": wrote behind dst"
                    bad = Q.same_bits_or_nan(got[:n], ref)
                    assert bad.size == 0, "%s: %d of %d elements differ, first at %d: %r vs %r" % (tag, bad.size, n, bad[0], got[bad[0]], ref[bad[0]])
        # noise_std = 0 and coef = the fp32 weights: the existing entry point's bits; and a pass that is not the last draws nothing
        wt = G(np.array(U.WS[:k], dtype=f32))
        a = torch.full((n + GUARD,), SENT, dtype=torch.float32, device=DEV)
        b, c = a.clone(), a.clone()
        if bits:
            delta_dp(a, ptr(xd), dups, wt, bits, n, 0, 1, 0.0)
            delta_dp(c, ptr(xd), dups, wt, bits, n, 0, 0, U.NOISE_STD)
            rc = _C.lib().fedfr_delta_aggregate(ptr(b), ptr(xd), ptrs_of([u[0] for u in dups]), ptrs_of([u[1] for u in dups]), wvec(U.WS[:k]), k, bits, n, 0,
                                                _C.stream())
        else:
            sparse_dp(a, ptr(xd), dups, wt, n, 0, 1, 0.0)
            sparse_dp(c, ptr(xd), dups, wt, n, 0, 0, U.NOISE_STD)
            keeps = (C.c_size_t * k)(*[u[2] for u in dups])
            rc = _C.lib().fedfr_sparse_aggregate(ptr(b), ptr(xd), ptrs_of([u[0] for u in dups]), ptrs_of([u[1] for u in dups]), keeps, wvec(U.WS[:k]), k, n, 0,
                                                 _C.stream())
        assert rc == 0, _C.last_error()
        torch.cuda.synchronize()
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(c.view(torch.int32), b.view(torch.int32)), (what, n, k)
    assert np.array_equal(bits_of(N(xd)), bits_of(x))


@pytest.mark.parametrize("n", Q.SIZES)
@pytest.mark.parametrize("bits", Q.BITS)
def test_delta_aggregate_dp_bit_identical_to_the_restatement(bits, n):
    check_dp_aggregate(bits, n, (1, 3, 8), agg_uploads(n, 8, bits), "hashed")


@pytest.mark.parametrize("bits", Q.BITS)
def test_delta_aggregate_dp_grid_stride_wrap(bits):
    n = Q.BIG
    check_dp_aggregate(bits, n, (3,), agg_uploads(n, 3, bits), "BIG", accumulates=(1,), bases=("distinct",), stds=(U.NOISE_STD,))


@pytest.mark.parametrize("k", [9, 17])
@pytest.mark.parametrize("bits", Q.BITS)
def test_delta_aggregate_dp_chained(bits, k):
    """chains of 9 and 17 uploads: every pass is given the chain's noise arguments, only the last draws, and the result is the
    restatement's single ascending loop, then the noise, then x"""
    n = 4103
    ups = agg_uploads(n, k, bits)
    dups = dev_codes(ups)
    ws = [f32(1.0 / (3 + i)) for i in range(k)]
    coef_t = torch.full((k + GUARD,), SENT, dtype=torch.float32, device=DEV)
    sq_t = torch.empty(k, dtype=torch.float64, device=DEV)
    o = Norms(8, n)
    for c0 in range(0, k, 8):
        g = dups[c0:c0 + 8]
        rc = _C.lib().fedfr_delta_sqnorm(ptrs_of([u[0] for u in g]), ptrs_of([u[1] for u in g]), wvec(ws[c0:c0 + 8]), len(g), bits, n, 20.0,
                                         ptr(sq_t) + 8 * c0, ptr(coef_t) + 4 * c0, ptr(o.wsp), o.need, _C.stream())
        assert rc == 0, _C.last_error()
    torch.cuda.synchronize()
    coef = N(coef_t)[:k]
    assert np.all(N(coef_t)[k:] == f32(SENT)) and np.any(coef[np.isfinite(N(sq_t))] < np.array(ws, dtype=f32)[np.isfinite(N(sq_t))])
    x = (0.5 * np.sin(0.37 * np.arange(n, dtype=f64) + 0.1)).astype(f32)
    xd = G(x)
    for std in (0.0, U.NOISE_STD):
        buf = torch.full((n + GUARD,), SENT, dtype=torch.float32, device=DEV)
        for c0 in range(0, k, 8):
            last = c0 + 8 >= k
            rc = _C.lib().fedfr_delta_aggregate_dp(ptr(buf), ptr(xd) if last else None, ptrs_of([u[0] for u in dups[c0:c0 + 8]]),
                                                   ptrs_of([u[1] for u in dups[c0:c0 + 8]]), ptr(coef_t) + 4 * c0, len(dups[c0:c0 + 8]), bits, n,
                                                   1 if c0 else 0, 1 if last else 0, float(std), U.SEED, U.ROUND, U.SID, 0, _C.stream())
            assert rc == 0, _C.last_error()
        torch.cuda.synchronize()
        got = N(buf)
        assert np.all(got[n:] == f32(SENT))
        assert Q.same_bits_or_nan(got[:n], U.delta_chained_dp(x, ups, coef, bits, n, std, z_of(n))).size == 0, (bits, k, std)


def test_the_noise_of_an_element_depends_on_its_index_alone():
    """uploads of zeros, so the output IS noise_std z: the same for k = 1 and k = 8, for one workgroup and for many (n against a prefix of a
    longer buffer), for the compressed and the sparse kernel, on the vector path and in the tail; an offset shifts the stream"""
    short, long_ = 1023, 70001
    std = U.NOISE_STD
    outs = {}
    for n, k in ((short, 1), (long_, 8)):
        zero = [(np.zeros(Q.code_bytes(8, n), dtype=np.uint8), np.full(Q.scale_bytes(n), 120, dtype=np.uint8))] * k
        empty = [(np.zeros(0, np.uint32), np.zeros(0, f32))] * k
        coef_t = G(np.array(U.WS[:k], dtype=f32))
        for name, off in (("delta", 0), ("sparse", 0), ("delta+8", 8)):
            buf = torch.full((n + GUARD,), SENT, dtype=torch.float32, device=DEV)
            if name == "sparse":
                sparse_dp(buf, None, dev_sparse(empty), coef_t, n, 0, 1, std, off)
            else:
                delta_dp(buf, None, dev_codes(zero), coef_t, 8, n, 0, 1, std, off)
            outs[name, n] = N(buf)
            assert np.all(outs[name, n][n:] == f32(SENT))
    ref = f32(0.0) + f32(std) * z_of(long_ + 8)
    for name, off in (("delta", 0), ("sparse", 0), ("delta+8", 8)):
        assert np.array_equal(bits_of(outs[name, long_][:long_]), bits_of(ref[off:off + long_])), name
        assert np.array_equal(bits_of(outs[name, short][:short]), bits_of(outs[name, long_][:short])), name
    assert not np.array_equal(outs["delta", short][:short], outs["delta+8", short][:short])


# ---- fedfr_sparse_aggregate_dp -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", S.UPLOAD_SHAPES)
@pytest.mark.parametrize("n", S.AGG_SIZES)
def test_sparse_aggregate_dp_bit_identical_to_the_restatement(n, shape):
    check_dp_aggregate(0, n, (1, 8), list(S.uploads(n, shape)), shape)


def test_sparse_aggregate_dp_grid_stride_wrap():
    """n = 2048 * 256 * 8 + 37: every workgroup walks a tile, the last one a partial tile; the noise reaches every element"""
    n = S.BIG
    ups = list(S.uploads(n, "gaps", 1)) + [(np.arange(0, n, 3).astype(np.uint32), S._vals(np.arange(0, n, 3).astype(np.uint32), 1))]
    check_dp_aggregate(0, n, (2,), ups, "BIG", accumulates=(1,), bases=("distinct",), stds=(U.NOISE_STD,))


@pytest.mark.parametrize("k", [9, 17])
def test_sparse_aggregate_dp_chained(k):
    n = 3 * S.AGG_TILE + 5
    ups = (S.uploads(n, "multiples") + S.uploads(n, "gaps") + S.uploads(n, "one tile"))[:k]
    dups = dev_sparse(ups)
    ws = [f32(1.0 / (3 + i)) for i in range(k)]
    coef_t = torch.full((k + GUARD,), SENT, dtype=torch.float32, device=DEV)
    sq_t = torch.empty(k, dtype=torch.float64, device=DEV)
    viol = torch.zeros(k, dtype=torch.int32, device=DEV)
    o = Norms(8, n)
    for c0 in range(0, k, 8):
        g = dups[c0:c0 + 8]
        keeps = (C.c_size_t * len(g))(*[u[2] for u in g])
        rc = _C.lib().fedfr_sparse_sqnorm(ptrs_of([u[0] for u in g]), ptrs_of([u[1] for u in g]), keeps, wvec(ws[c0:c0 + 8]), len(g), n, 2.0,
                                          ptr(sq_t) + 8 * c0, ptr(coef_t) + 4 * c0, ptr(viol) + 4 * c0, ptr(o.wsp), o.need, _C.stream())
        assert rc == 0, _C.last_error()
    torch.cuda.synchronize()
    coef = N(coef_t)[:k]
    assert int(viol.abs().sum()) == 0 and np.any(coef < np.array(ws, dtype=f32)) and np.all(N(coef_t)[k:] == f32(SENT))
    x = (0.5 * np.sin(0.37 * np.arange(n, dtype=f64) + 0.1)).astype(f32)
    xd = G(x)
    for std in (0.0, U.NOISE_STD):
        buf = torch.full((n + GUARD,), SENT, dtype=torch.float32, device=DEV)
        for c0 in range(0, k, 8):
            last = c0 + 8 >= k
            g = dups[c0:c0 + 8]
            keeps = (C.c_size_t * len(g))(*[u[2] for u in g])
            rc = _C.lib().fedfr_sparse_aggregate_dp(ptr(buf), ptr(xd) if last else None, ptrs_of([u[0] for u in g]), ptrs_of([u[1] for u in g]), keeps,
                                                    ptr(coef_t) + 4 * c0, len(g), n, 1 if c0 else 0, 1 if last else 0, float(std), U.SEED, U.ROUND, U.SID, 0,
                                                    _C.stream())
            assert rc == 0, _C.last_error()
        torch.cuda.synchronize()
        got = N(buf)
        assert np.all(got[n:] == f32(SENT))
        assert np.array_equal(bits_of(got[:n]), bits_of(U.sparse_chained_dp(x, ups, coef, n, std, z_of(n)))), (k, std)


# ---- argument errors ---------------------------------------------------------------------------------------------------------------------
def test_argument_errors_launch_nothing():
    """one case per refusal, on device buffers: every output stays at its sentinel (tests/test_upload_clip_cpu.py walks every argument)"""
    n, k = 1023, 2
    ups = dev_codes(U.hashed_uploads(n, k, 8))
    sp = dev_sparse(list(S.uploads(n, "multiples", k)))
    o = Norms(k, n)
    out = torch.full((n + GUARD,), SENT, dtype=torch.float32, device=DEV)
    coef_in = G(np.array(U.WS[:4], dtype=f32))
    lib = _C.lib()
    ws = wvec(U.WS[:8])
    cs, ss = ptrs_of([u[0] for u in ups]), ptrs_of([u[1] for u in ups])
    ix, vs = ptrs_of([u[0] for u in sp]), ptrs_of([u[1] for u in sp])
    keeps = (C.c_size_t * k)(*[u[2] for u in sp])
    nan = float("nan")

    def refused(rc, word, code=-1):
        assert rc == code and word in _C.last_error(), (rc, _C.last_error())

    st = _C.stream()
    dn, sn, da, sa = lib.fedfr_delta_sqnorm, lib.fedfr_sparse_sqnorm, lib.fedfr_delta_aggregate_dp, lib.fedfr_sparse_aggregate_dp
    refused(dn(cs, ss, ws, k, 8, n, 1.0, None, ptr(o.coef), ptr(o.wsp), o.need, st), "null")
    refused(dn(cs, ss, ws, 9, 8, n, 1.0, ptr(o.sq), ptr(o.coef), ptr(o.wsp), o.need, st), "k=9")
    refused(dn(cs, ss, ws, k, 6, n, 1.0, ptr(o.sq), ptr(o.coef), ptr(o.wsp), o.need, st), "bits=6")
    refused(dn(ptrs_of([ups[0][0], None]), ss, ws, k, 8, n, 1.0, ptr(o.sq), ptr(o.coef), ptr(o.wsp), o.need, st), "code buffer 1 is null")
    refused(dn(cs, ss, ws, k, 8, n, 1.0, ptr(o.sq) + 4, ptr(o.coef), ptr(o.wsp), o.need, st), "aligned")
    refused(dn(cs, ss, ws, k, 8, n, nan, ptr(o.sq), ptr(o.coef), ptr(o.wsp), o.need, st), "NaN")
    refused(dn(cs, ss, ws, k, 8, n, 1.0, ptr(o.sq), ptr(o.coef), ptr(o.wsp), o.need - 1, st), "workspace", code=-3)
    refused(sn(ix, vs, keeps, ws, k, n, 1.0, ptr(o.sq), ptr(o.coef), None, ptr(o.wsp), o.need, st), "null")
    refused(sn(ix, vs, keeps, ws, 0, n, 1.0, ptr(o.sq), ptr(o.coef), ptr(o.viol), ptr(o.wsp), o.need, st), "k=0")
    refused(sn(ix, vs, (C.c_size_t * k)(n + 1, 1), ws, k, n, 1.0, ptr(o.sq), ptr(o.coef), ptr(o.viol), ptr(o.wsp), o.need, st), "upload 0")
    refused(sn((C.c_void_p * 2)(ptr(sp[0][0]), ptr(sp[1][0]) + 4), vs, keeps, ws, k, n, 1.0, ptr(o.sq), ptr(o.coef), ptr(o.viol), ptr(o.wsp), o.need, st), "aligned")
    refused(sn(ix, vs, keeps, ws, k, n, nan, ptr(o.sq), ptr(o.coef), ptr(o.viol), ptr(o.wsp), o.need, st), "NaN")
    refused(sn(ix, vs, keeps, ws, k, n, 1.0, ptr(o.sq), ptr(o.coef), ptr(o.viol), ptr(o.wsp), 8, st), "workspace", code=-3)
    noise = (0.5, 1, 2, 3, 0)
    refused(da(ptr(out), None, cs, ss, None, k, 8, n, 0, 1, *noise, st), "null")
    refused(da(ptr(out), None, cs, ss, ptr(coef_in), 9, 8, n, 0, 1, *noise, st), "k=9")
    refused(da(ptr(out), None, cs, ss, ptr(coef_in), k, 2, n, 0, 1, *noise, st), "bits=2")
    refused(da(ptr(out) + 8, None, cs, ss, ptr(coef_in), k, 8, n, 0, 1, *noise, st), "aligned")
    refused(da(ptr(out), None, cs, ss, ptr(coef_in) + 2, k, 8, n, 0, 1, *noise, st), "coef")
    refused(da(ptr(out), None, cs, ss, ptr(coef_in), k, 8, n, 0, 1, -0.5, 1, 2, 3, 0, st), "noise_std")
    refused(da(ptr(out), None, cs, ss, ptr(coef_in), k, 8, n, 0, 1, float("inf"), 1, 2, 3, 0, st), "noise_std")
    refused(da(ptr(out), None, cs, ss, ptr(coef_in), k, 8, n, 0, 1, 0.5, 1, 2, 3, 2, st), "offset 2")
    refused(sa(None, None, ix, vs, keeps, ptr(coef_in), k, n, 0, 1, *noise, st), "null")
    refused(sa(ptr(out), None, ix, vs, keeps, ptr(coef_in), 9, n, 0, 1, *noise, st), "k=9")
    refused(sa(ptr(out), None, ptrs_of([sp[0][0], None]), vs, keeps, ptr(coef_in), k, n, 0, 1, *noise, st), "index buffer 1 is null")
    refused(sa(ptr(out), ptr(out) + 4, ix, vs, keeps, ptr(coef_in), k, n, 0, 1, *noise, st), "aligned")
    refused(sa(ptr(out), None, ix, vs, keeps, ptr(coef_in), k, n, 0, 1, nan, 1, 2, 3, 0, st), "noise_std")
    refused(sa(ptr(out), None, ix, vs, keeps, ptr(coef_in), k, n, 0, 1, 0.5, 1, 2, 3, 7, st), "offset 7")
    assert da(ptr(out), None, cs, ss, ptr(coef_in), k, 8, 0, 0, 1, *noise, st) == 0      # n = 0: a no-op
    sq, coef, viol = o.read("refused calls")
    assert np.all(sq == SENT_D) and np.all(coef == f32(SENT)) and np.all(viol == 0) and np.all(N(o.wsp) == SENT_D)
    assert float(out.min()) == SENT == float(out.max())


# ---- the Python surface ------------------------------------------------------------------------------------------------------------------
NP = TC.NP
OPT_KINDS = (None, "AVGM", "ADAGRAD", "ADAM", "YOGI")


def _opt(kind, clip_norm=0.0):
    return None if kind is None else server.ServerOptimizer(kind, lr=0.5, beta1=0.75, beta2=0.9, tau=1e-2, clip_norm=clip_norm)


def check_round_function(sparse, kind, with_mech):
    k = 9
    g, models = TC.synthetic_states(k)
    sizes = TC.sizes_of(k)
    ws = TC.weights32(sizes)
    x = N(g.flat[0])
    if sparse:
        ups = [compress.TopKCompressor(0.1).compress(g, m) for m in models]
        rups = [(N(u.idx).view(np.uint32), N(u.val)) for u in ups]
        refs, terms = [U.sparse_sqnorm(v) for _, v in rups], [i.size for i, _ in rups]
    else:
        bits = 4 if with_mech else 8
        ups = [compress.DeltaCompressor(bits).compress(g, m) for m in models]
        rups = [(N(u.codes), N(u.scales)) for u in ups]
        refs, terms = [U.delta_sqnorm(c, s, bits, NP) for c, s in rups], [Q.scale_bytes(NP)] * k
    clip_norm = float(f32(0.75 * math.sqrt(max(refs))))
    clip = server.UploadClip(clip_norm)
    mech = privacy.GaussianMechanism(1.5, clip_norm, seed=U.SEED, stream_id=U.SID) if with_mech else None
    if mech is not None:
        mech.round = 11
    opt = _opt(kind, clip_norm if kind == "YOGI" else 0.0)                    # (an optimiser that clips at the same norm is accepted)
    fed = server.FedSparse if sparse else server.FedCompressed
    out = fed(g, ups, sizes, opt, clip=clip, mech=mech)
    avg = server.FedPavg(models, sizes)
    torch.cuda.synchronize()
    sq, coef = N(clip.last_update_sqnorm), N(clip.last_coef)
    assert sq.dtype == f64 and coef.dtype == f32 and sq.shape == coef.shape == (k,) and clip.last_coef.is_cuda
    for i in range(k):
        assert U.rel_err(float(sq[i]), refs[i]) <= U.tolerance(terms[i]), i
    want = F.clip_coef(sq, ws, clip_norm)
    assert np.all(np.abs(coef.astype(f64) - want.astype(f64)) <= np.spacing(want).astype(f64)) and np.any(coef < np.array(ws)) and np.any(coef == np.array(ws))
    if sparse:
        assert N(clip.last_violations).tolist() == [0] * k and clip.last_violations.dtype == torch.int32
    else:
        assert clip.last_violations is None
    std, z = 0.0, None
    if mech is not None:
        assert mech.round == 12                                               # one call, one round of the stream
        std = D.noise_std32(1.5, clip_norm, max(ws))
        assert std == f32(mech.noise_std(ws))
        z = z_of(NP, U.SEED, 11, U.SID)
    if sparse:
        ref = U.sparse_chained_dp(x, rups, coef, NP, std, z, with_base=opt is None)
    else:
        ref = U.delta_chained_dp(x, rups, coef, bits, NP, std, z, with_base=opt is None)
    if opt is None:
        assert np.array_equal(bits_of(N(out.flat[0])), bits_of(ref))
    else:
        ref_opt = _opt(kind)
        P = torch.empty(NP, dtype=torch.float32, device=DEV)
        ref_opt.apply_delta(P, g.flat[0], G(ref))
        torch.cuda.synchronize()
        assert torch.equal(out.flat[0], P) and torch.equal(opt.m, ref_opt.m) and opt.rounds == 1 and float(opt.m.abs().max()) > 0
        assert (opt.v is None and ref_opt.v is None) or torch.equal(opt.v, ref_opt.v)
    assert np.array_equal(bits_of(N(g.flat[0])), bits_of(x))                 # the global state is read, never written
    assert torch.equal(out.flat[1], avg.flat[1]) and torch.equal(out.flat[2], avg.flat[2])      # statistics and counters: outside clip and mechanism
    if mech is not None and opt is None:                                      # and the noise is really there, at its size
        plain = U.sparse_chained_dp(x, rups, coef, NP) if sparse else U.delta_chained_dp(x, rups, coef, bits, NP)
        d = N(out.flat[0]).astype(f64) - plain.astype(f64)
        assert 0.9 * float(std) < d.std() < 1.1 * float(std)


@pytest.mark.parametrize("with_mech", [False, True])
@pytest.mark.parametrize("kind", OPT_KINDS)
def test_fedcompressed_with_clip_and_mechanism(kind, with_mech):
    check_round_function(False, kind, with_mech)


@pytest.mark.parametrize("with_mech", [False, True])
@pytest.mark.parametrize("kind", OPT_KINDS)
def test_fedsparse_with_clip_and_mechanism(kind, with_mech):
    check_round_function(True, kind, with_mech)


def test_clip_none_is_the_path_of_today():
    """clip=None, mech=None: the entry points of today (the new ones are not called) and its bits"""
    k = 9
    g, models = TC.synthetic_states(k)
    ups = [compress.DeltaCompressor(8).compress(g, m) for m in models]
    sps = [compress.TopKCompressor(0.1).compress(g, m) for m in models]
    a, b = server.FedCompressed(g, ups, TC.sizes_of(k)), server.FedSparse(g, sps, TC.sizes_of(k))
    real = _C.call
    called = []

    def spy(name, *args):
        called.append(name)
        return real(name, *args)
    try:
        _C.call = spy
        a2 = server.FedCompressed(g, ups, TC.sizes_of(k), None, clip=None, mech=None)
        b2 = server.FedSparse(g, sps, TC.sizes_of(k), None, clip=None, mech=None)
    finally:
        _C.call = real
    assert torch.equal(a.flat[0], a2.flat[0]) and torch.equal(b.flat[0], b2.flat[0])
    assert "fedfr_delta_aggregate" in called and "fedfr_sparse_aggregate" in called and not any("_dp" in c or "sqnorm" in c for c in called)


# ---- Server.train ------------------------------------------------------------------------------------------------------------------------
def test_server_train_clips_compressed_uploads(monkeypatch):
    """compress_bits=8, clip_norm, clip_uploads=True, FedAvg: the installed parameters are the restatement on the recorded uploads with the
    device's coefficients (data-size weights), every client was clipped, and the norms the round read back are the uploads' own"""
    clip_norm = 2e-3
    srv, clients = TC._tiny_world("FedAvg", 2, compress_bits=8, clip_norm=clip_norm, clip_uploads=True)
    rec = []
    real = server.FedCompressed

    def recording(global_state, updates, weights, server_opt=None, **kw):
        out = real(global_state, updates, weights, server_opt, **kw)
        rec.append((N(global_state.flat[0]), [(N(u.codes), N(u.scales)) for u in updates], list(weights), server_opt, kw))
        return out
    monkeypatch.setattr(server, "FedCompressed", recording)
    monkeypatch.setattr(server, "FedPavg", lambda *a: pytest.fail("FedPavg was called on the compressed path"))
    assert np.isfinite(srv.train())
    torch.cuda.synchronize()
    xg, ups, weights, opt, kw = rec[0]
    n = xg.size
    assert weights == [300, 100] and opt is None and kw["clip"] is srv.upload_clip and kw["mech"] is None and srv.upload_clip.clip_norm == clip_norm
    assert srv.dp_epsilon is None and srv.dp_accountant is None
    ws = TC.weights32(weights)
    sq, coef = N(srv.upload_clip.last_update_sqnorm), N(srv.upload_clip.last_coef)
    assert srv.upload_sqnorms == sq.tolist() and srv.upload_coefs == [float(c) for c in coef] and srv.upload_violations is None
    for i, (c, s) in enumerate(ups):
        assert U.rel_err(float(sq[i]), U.delta_sqnorm(c, s, 8, n)) <= U.tolerance(Q.scale_bytes(n)), i
    want = F.clip_coef(sq, ws, clip_norm)
    assert np.all(np.abs(coef.astype(f64) - want.astype(f64)) <= np.spacing(want).astype(f64)) and np.all(coef < np.array(ws))
    got = N(srv.federated_model.flat_state()[0])
    for w in TC._windows(n):
        wu = [(c[w], s[w.start // 32:(w.stop + 31) // 32]) for c, s in ups]
        ref = U.delta_chained_dp(xg[w], wu, coef, 8, w.stop - w.start)
        assert np.array_equal(bits_of(got[w]), bits_of(ref)), w


def test_server_train_topk_uploads_under_dp(monkeypatch):
    """topk_ratio=0.05, clip_norm, dp_noise_multiplier=1.0, dp_seed, clip_uploads=True: two rounds whose installed parameters are the
    restatement on the recorded uploads (uniform weights, the device's coefficients, the round's noise), dp_epsilon is the accountant run
    by hand; then a client whose upload carries a NaN, and one whose indices repeat: each voids its round (RuntimeError naming the client,
    the global model untouched, nothing accounted)"""
    clip_norm, seed = 2e-3, 2024
    srv, clients = TC._tiny_world("FedAvg", 2, topk_ratio=0.05, clip_norm=clip_norm, dp_noise_multiplier=1.0, dp_seed=seed, clip_uploads=True)
    rec = []
    real = server.FedSparse

    def recording(global_state, updates, weights, server_opt=None, **kw):
        rnd = kw["mech"].round
        out = real(global_state, updates, weights, server_opt, **kw)
        rec.append((N(global_state.flat[0]), [(N(u.idx).view(np.uint32), N(u.val)) for u in updates], list(weights), rnd, kw))
        return out
    monkeypatch.setattr(server, "FedSparse", recording)
    monkeypatch.setattr(server, "FedDP", lambda *a, **k: pytest.fail("FedDP was called on the top-k path"))
    n = srv.federated_model.flat_state()[0].numel()
    for r in range(2):
        assert np.isfinite(srv.train())
        srv.step_round()
        torch.cuda.synchronize()
        xg, ups, weights, rnd, kw = rec[r]
        assert weights == [1.0, 1.0] and rnd == r and kw["clip"] is srv.upload_clip and kw["mech"] is srv.dp_mech
        assert srv.dp_mech.seed == seed and srv.dp_mech.round == r + 1 and srv.dp_mech.clip_norm == clip_norm
        sq, coef = N(srv.upload_clip.last_update_sqnorm), N(srv.upload_clip.last_coef)
        assert srv.upload_violations == [0, 0] and srv.upload_sqnorms == sq.tolist()
        for i, (idx, val) in enumerate(ups):
            assert idx.size == S.keep_count(n, 0.05) and U.rel_err(float(sq[i]), U.sparse_sqnorm(val)) <= U.tolerance(idx.size), i
        want = F.clip_coef(sq, [f32(0.5)] * 2, clip_norm)
        assert np.all(np.abs(coef.astype(f64) - want.astype(f64)) <= np.spacing(want).astype(f64)) and np.all(coef < f32(0.5))
        std = D.noise_std32(1.0, clip_norm, 0.5)
        ref = U.sparse_chained_dp(xg, ups, coef, n, std, z_of(n, seed, r, 0))
        got = N(srv.federated_model.flat_state()[0])
        assert np.array_equal(bits_of(got), bits_of(ref)), "global parameters after round %d" % r
        assert srv.dp_epsilon == pytest.approx(D.epsilon_by_hand(1.0, 1.0, r + 1, 1e-5), rel=1e-12)
        assert srv.dp_accountant.steps == r + 1 and srv.dp_accountant.q == 1.0
    assert not np.array_equal(z_of(4096, seed, 0, 0), z_of(4096, seed, 1, 0))
    before = N(srv.federated_model.flat_state()[0]).copy()
    eps = srv.dp_epsilon
    for poison, word in ((lambda u: u.val.__setitem__(3, float("nan")), "squared norm nan"),
                         (lambda u: u.idx.__setitem__(1, int(u.idx[0])), "not ascending")):
        victim = clients[1]
        real_get = victim.get_sparse_update

        def poisoned(*a, _real=real_get, _poison=poison, **k):
            u = _real(*a, **k)
            _poison(u)
            return u
        monkeypatch.setattr(victim, "get_sparse_update", poisoned)
        with pytest.raises(RuntimeError, match=r"client %s .*%s.*the round is void" % (getattr(victim, "cid", 1), word)):
            srv.train()
        monkeypatch.setattr(victim, "get_sparse_update", real_get)
        torch.cuda.synchronize()
        assert np.array_equal(bits_of(N(srv.federated_model.flat_state()[0])), bits_of(before))
        assert srv.dp_accountant.steps == 2 and srv.dp_epsilon == eps
