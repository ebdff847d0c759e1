"""Top-k sparsified client uploads, the part that needs no GPU: the laws the format promises hold for the numpy restatement of
tests/sparse_cases.py (which the kernels are held to bit for bit on the GPU), the constructed inputs hit what they were built for, the C
ABI carries the new entry points with their host-side checks, no new kernel uses scratch memory, and the Python surface refuses what it
cannot serve before any client trains."""
import ctypes as C
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import sparse_cases as S
from conftest import REPO

f32, f64 = np.float32, np.float64
NEW_SYMBOLS = ("fedfr_topk_workspace_bytes", "fedfr_topk_sparsify", "fedfr_sparse_aggregate")


@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__ as ge
    ge.build()
    from fedfr_amd import _C
    return _C


def law_inputs():
    """[(name, x, x_i, e or None, keep)]: the sine states with and without a residual at several keeps, and every constructed pattern"""
    n = 3 * S.TILE + 5
    x, xs = S.inputs(n, 3)
    out = []
    for keep in S.keeps_for(n):
        out.append(("sine keep=%d" % keep, x, xs[1], None, keep))
        out.append(("sine+residual keep=%d" % keep, x, xs[2], S.residual(n), keep))
    for name, v, keep in S.patterns():
        out.append((name, np.zeros(v.size, dtype=f32), v, None, keep))
        out.append((name + " + 0 residual", np.zeros(v.size, dtype=f32), v, np.zeros(v.size, dtype=f32), keep))
    return out


# ---- laws of the restatement -------------------------------------------------------------------------------------------------------------
def test_restatement_laws():
    """threshold law (S = {key > T} + the r lowest-index elements with key == T, and the O(n) form of it selects the same set), position
    law, idx strictly ascending, values bit for bit, exact conservation scatter(idx, val) + e' == v wherever v is finite, e' = +0 at the
    sent and the non-finite elements, the counter = the non-finite elements"""
    for name, x, xi, e, keep in law_inputs():
        n = x.size
        idx, val, en, nbad, v = S.sparsify(x, xi, e, keep)
        assert idx.dtype == np.uint32 and idx.size == keep == val.size and np.all(np.diff(idx.astype(np.int64)) > 0) and idx[-1] < n, name
        key = S.keys(v)
        T, r = S.threshold(v, keep)
        assert 1 <= r <= np.count_nonzero(key == T) and np.count_nonzero(key > T) + r == keep, name
        sel = np.zeros(n, dtype=bool)
        sel[idx] = True
        assert np.all(sel[key > T]) and not np.any(sel[key < T]), name
        assert np.array_equal(np.flatnonzero(sel & (key == T)), np.flatnonzero(key == T)[:r]), name      # the r LOWEST-index ties
        assert np.array_equal(S.select_by_threshold(v, keep), idx), name
        pos, mask = S.positions(v, keep)
        assert np.array_equal(mask, sel) and np.array_equal(pos, np.arange(keep)), name                 # the position law lands idx[t] at t
        assert np.array_equal(S.bits_of(val), S.bits_of(v)[idx]), name
        bad = key >= S.INF_KEY
        assert nbad == int(bad.sum()) == int((~np.isfinite(v)).sum()), name
        assert np.all(S.bits_of(en)[sel | bad] == 0), name                                              # +0, not -0
        assert np.array_equal(S.bits_of(en)[~(sel | bad)], S.bits_of(v)[~(sel | bad)]), name
        fin = ~bad & (v != 0)
        assert np.array_equal(S.bits_of(S.scatter(idx, val, n) + en)[fin], S.bits_of(v)[fin]), name    # exact: one of the two terms is +0
        assert np.all(np.isfinite(en)), name


def test_constructed_inputs_hit_what_they_are_for():
    pats = {name: (v, keep) for name, v, keep in S.patterns()}
    assert S.PN == 3 * S.TILE + 5

    def digits(v):
        k = S.keys(v).astype(np.int64)
        return k >> 20, (k >> 10) & 1023, k & 1023

    d1, d2, d3 = digits(pats["top digit only"][0])
    assert len(set(d1)) == 2039 and d1.max() < (S.INF_KEY >> 20) and not d2.any() and not d3.any()
    d1, d2, d3 = digits(pats["middle digit only"][0])
    assert len(set(d1)) == 1 and len(set(d2)) == 1024 and not d3.any()
    d1, d2, d3 = digits(pats["lowest digit only"][0])
    assert len(set(d1)) == 1 and len(set(d2)) == 1 and len(set(d3)) == 1024
    v, keep = pats["all ties"]
    assert len(set(S.keys(v))) == 1 and np.any(np.signbit(v)) and np.any(~np.signbit(v)) and np.array_equal(S.select(v, keep), np.arange(keep))
    v, keep = pats["all zeros"]
    assert not S.keys(v).any() and np.any(np.signbit(v)) and np.array_equal(S.select(v, keep), np.arange(keep))
    v, _ = pats["subnormals only"]
    assert np.all(S.keys(v) > 0) and np.all(S.keys(v) < 0x00800000)
    v, _ = pats["one exponent"]
    assert len(set(S.keys(v) >> 23)) == 1 and len(set(S.keys(v) >> 20)) == 8                           # one octave: 8 bins of the top digit
    T = int(S.bits_of(np.array([S.TIE_VALUE]))[0])
    ties = np.array(S.TIE_POSITIONS)
    for what, r in S.TIE_CUTS:
        v, keep = pats["tie cut " + what]
        assert S.threshold(v, keep) == (T, r) and np.array_equal(np.flatnonzero(S.keys(v) == T), ties)
        idx = S.select(v, keep)
        sent = np.intersect1d(idx, ties)
        assert np.array_equal(sent, ties[:r]) and np.all(np.isin(S.ABOVE_POSITIONS, idx))
    last_a, first_a = ties[2 - 1], ties[2]
    assert last_a // S.WAVE == first_a // S.WAVE == 0                                                   # (a) the cut lies inside wave 0
    assert ties[3 - 1] // S.WAVE == 0 and ties[3] // S.WAVE == 1 and ties[3] // S.TILE == 0             # (b) between wave 0 and wave 1 of tile 0
    assert ties[5 - 1] // S.TILE == 0 and ties[5] // S.TILE == 1                                        # (c) between tile 0 and tile 1
    assert ties[-1] >= 3 * S.TILE                                                                       # (d) the last tie is in the partial tile
    assert len({p // S.WAVE for p in S.TIE_POSITIONS}) >= 6
    v, keep = pats["non-finite, fewer than keep"]
    bad = np.flatnonzero(~np.isfinite(v))
    assert bad.size == 7 > 4 and keep > bad.size and np.all(np.isin(bad, S.select(v, keep)))
    assert np.any(np.isnan(v) & np.signbit(v)) and np.any(np.isnan(v) & ~np.signbit(v)) and np.any(np.isposinf(v)) and np.any(np.isneginf(v))
    v, keep = pats["non-finite, more than keep"]
    idx, _, en, nbad, _ = S.sparsify(np.zeros(v.size, dtype=f32), v, None, keep)
    assert np.all(np.isnan(v[idx])) and nbad == 7 and np.all(np.isfinite(en)) and np.all(S.bits_of(en)[bad] == 0)      # NaN orders above inf; the unsent infinities leave no residual
    x, xi, e, keep = S.big_case()
    assert x.size == S.BIG == S.GRID_CAP * S.TILE + 37 and keep == -(-S.BIG // 100) and np.isnan(xi[5]) and np.isnan(xi[S.BIG - 3])


def test_error_feedback_telescopes():
    """Four rounds with the same x and x_i, the residual carried: sum_t sent_t + e_4 equals 4 d, d = fl(x_i - x), up to the float32 rounding
    of the additions fl(d + e_{t-1}) alone.

    Derivation.  v_t = fl(d + e_{t-1}) = d + e_{t-1} + rho_t with |rho_t| <= U |v_t| (U = 2^-24: one rounding, relative to the result).
    The format gives sent_t + e_t = v_t EXACTLY (one of the two is +0).  Summing over t = 1..R with e_0 = 0:
        sum_t sent_t = sum_t (d + e_{t-1} + rho_t - e_t) = R d - e_R + sum_t rho_t,
    so |sum_t sent_t + e_R - R d| = |sum_t rho_t| <= U sum_t |v_t|.  The left side is evaluated in fp64 and the bound is asserted as it
    stands, with nothing added for that evaluation: the left side adds six float32 values (24-bit significands; 4 d is exact) that lie within a few
    octaves of each other, which fp64 adds exactly."""
    R = 4
    n = 3 * S.TILE + 5
    x, xs = S.inputs(n, 2)
    xi = xs[1]
    d = S.value_to_send(x, xi).astype(f64)
    keep = S.keep_count(n, 0.01)
    e = np.zeros(n, dtype=f32)
    total, vsum = np.zeros(n, dtype=f64), np.zeros(n, dtype=f64)
    for _ in range(R):
        idx, val, e, nbad, v = S.sparsify(x, xi, e, keep)
        assert nbad == 0
        sent = S.scatter(idx, val, n).astype(f64)
        total += sent
        vsum += np.abs(v.astype(f64))
    lhs = total + e.astype(f64) - R * d
    bound = S.U * vsum
    print("worst |telescoped error| / bound %.3f" % float(np.max(np.abs(lhs) / np.maximum(bound, 1e-300))))
    assert np.all(np.abs(lhs) <= bound)
    assert np.any(e != 0)
    # without feedback the same entries are sent every round and everything else never: the feedback is what the bound is about
    idx0, val0, _, _, _ = S.sparsify(x, xi, None, keep)
    drift = np.abs(R * S.scatter(idx0, val0, n).astype(f64) - R * d)
    assert np.max(drift) > 100 * np.max(np.abs(lhs))


def test_aggregate_restatement_matches_fp64_on_exact_weights():
    """weights that are powers of two make every product exact, so the float32 loop differs from the fp64 sum by its additions alone: the
    first (to +0) is exact, each later one rounds once, by at most U times its result, and every partial result is at most
    (1 + U)^2 M with M = sum_i |w_i val_i|: at most 2 U M (1 + 2 U) for three uploads; with accumulate and base two more additions
    round and the partial results are bounded by 2 |x| + M"""
    n = S.AGG_TILE + 7
    ups = S.uploads(n, "multiples", 3)
    ws = [0.5, 0.25, 0.25]
    got = S.aggregate(None, None, ups, ws, n, False)
    ref = sum(w * S.scatter(i, v, n).astype(f64) for (i, v), w in zip(ups, ws))
    mag = sum(w * np.abs(S.scatter(i, v, n).astype(f64)) for (i, v), w in zip(ups, ws))
    assert np.all(np.abs(got.astype(f64) - ref) <= 2 * S.U * mag * (1 + 2 * S.U))
    x = (0.5 * np.sin(0.37 * np.arange(n))).astype(f32)
    acc = S.aggregate(x.copy(), x, ups, ws, n, True)                          # accumulate and base both in use
    assert np.all(np.abs(acc.astype(f64) - (2 * x.astype(f64) + ref)) <= 4 * S.U * (2 * np.abs(x.astype(f64)) + mag) * (1 + 4 * S.U))
    ch = S.chained(x, ups * 3, [1.0 / 9] * 9, n)                              # 9 uploads: two groups
    one = S.aggregate(np.zeros(n, dtype=f32), x, ups * 3, [1.0 / 9] * 9, n, False)      # the same ascending loop in one go
    assert np.array_equal(S.bits_of(ch), S.bits_of(one))
    for shape in S.UPLOAD_SHAPES:                                             # the made-up uploads are what their names say
        for m in S.AGG_SIZES:
            for i, (idx, val) in enumerate(S.uploads(m, shape)):
                assert idx.dtype == np.uint32 and val.dtype == f32 and idx.size == val.size >= 1
    assert S.uploads(S.AGG_SIZES[-1], "multiples")[0][0].size == S.AGG_SIZES[-1]      # keep = n
    assert len({u[0].size for u in S.uploads(S.AGG_SIZES[-1], "multiples")}) == 8      # a different keep per client
    assert np.all(np.diff(S.uploads(S.AGG_SIZES[-1], "gaps")[0][0].astype(np.int64)) > S.AGG_TILE)
    assert all(u[0].size == 1 for u in S.uploads(S.AGG_SIZES[-1], "single"))
    assert all(np.all(u[0] // S.AGG_TILE == 1) for u in S.uploads(S.AGG_SIZES[-1], "one tile"))


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_header_ctypes_table_and_library_carry_the_symbols(built_lib):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "fedfr_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(fedfr_[a-z0-9_]+)\s*\(", src))
    out = subprocess.run(["nm", "-D", "--defined-only", built_lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = set(re.findall(r"\sT\s+(fedfr_[a-z0-9_]+)", out))
    for s in NEW_SYMBOLS:
        assert s in declared and s in built_lib.SIGNATURES and s in exported, s


def test_workspace_bytes_is_monotone_and_aligned(built_lib):
    lib = built_lib.lib()
    sizes = sorted(set(S.SIZES + (0, 2047, 2049, 4096, 65156160, S.BIG, 2 ** 31 - 1)))
    for fb in (0, 1):
        prev = 0
        for n in sizes:
            b = lib.fedfr_topk_workspace_bytes(n, fb)
            assert b % 16 == 0 and b >= prev > -1, (n, fb, b)
            assert b >= 8 * (-(-n // S.TILE)) + (0 if fb else 4 * n)          # a count pair per tile; without feedback the n values
            prev = b
    for n in sizes:                                                           # with feedback the values live in the residual
        assert lib.fedfr_topk_workspace_bytes(n, 0) - lib.fedfr_topk_workspace_bytes(n, 1) == (4 * n + 15) // 16 * 16
    assert lib.fedfr_topk_workspace_bytes(65156160, 1) < 1 << 20


def _aligned(nbytes, off=0):
    """(keep-alive array, address) of a host buffer whose address is 16-byte aligned plus ``off``"""
    raw = np.zeros(nbytes + 32, dtype=np.uint8)
    a = raw.ctypes.data
    return raw, (a + 15) // 16 * 16 + off


def test_argument_errors_are_host_side(built_lib):
    """every refused call returns FEDFR_ERR_ARG with a message naming the function (and the offending value) BEFORE any HIP call: host
    pointers serve, no GPU is needed, and nothing is written.  n = 0 with keep = 0 is a no-op."""
    lib = built_lib.lib()
    err_arg = int(re.search(r"#define FEDFR_ERR_ARG \((-?\d+)\)", open(os.path.join(REPO, "include", "fedfr_hip.h")).read()).group(1))
    n = 64
    keep = [_aligned(4 * n) for _ in range(8)]
    x, xi, e, idx, val, ws, dst, cnt = [a for _, a in keep]
    vp = C.c_void_p

    def refused(rc, *words):
        assert rc == err_arg, rc
        msg = lib.fedfr_last_error_string().decode()
        for w in words:
            assert w in msg, msg

    sp = lib.fedfr_topk_sparsify
    refused(sp(None, xi, e, n, 4, idx, val, cnt, ws, None), "topk_sparsify", "null")
    refused(sp(x, None, e, n, 4, idx, val, cnt, ws, None), "topk_sparsify", "null")
    refused(sp(x, xi, e, n, 4, None, val, cnt, ws, None), "topk_sparsify", "null")
    refused(sp(x, xi, e, n, 4, idx, None, cnt, ws, None), "topk_sparsify", "null")
    refused(sp(x, xi, e, n, 4, idx, val, cnt, None, None), "topk_sparsify", "null")
    refused(sp(x, xi, e, n, 0, idx, val, cnt, ws, None), "topk_sparsify", "keep=0")
    refused(sp(x, xi, None, n, n + 1, idx, val, None, ws, None), "topk_sparsify", "keep=%d" % (n + 1))
    refused(sp(x, xi, e, 0, 1, idx, val, cnt, ws, None), "topk_sparsify", "keep=1")
    for big in (2 ** 31, 2 ** 31 + 5, 2 ** 40):
        refused(sp(x, xi, e, big, 4, idx, val, cnt, ws, None), "topk_sparsify", "2^31", "n=%d" % big)
    for args in ((x + 4, xi, e, idx, val, ws), (x, xi + 8, e, idx, val, ws), (x, xi, e + 4, idx, val, ws), (x, xi, e, idx + 4, val, ws),
                 (x, xi, e, idx, val + 8, ws), (x, xi, None, idx, val, ws + 4)):
        a = args
        refused(sp(a[0], a[1], a[2], n, 4, a[3], a[4], cnt, a[5], None), "topk_sparsify", "aligned")
    refused(sp(x, xi, e, n, 4, idx, val, cnt + 2, ws, None), "topk_sparsify", "aligned")
    assert sp(x, xi, e, 0, 0, idx, val, cnt, ws, None) == 0                   # n = 0, keep = 0: nothing to do, nothing launched
    assert sp(x, xi, None, 0, 0, idx, val, None, ws, None) == 0

    aggr = lib.fedfr_sparse_aggregate
    wv = (C.c_float * 9)(*([0.125] * 9))
    ks = (C.c_size_t * 9)(*([4] * 9))

    def arr(ps):
        return (vp * max(len(ps), 1))(*ps)

    ii, vv = arr([idx] * 9), arr([val] * 9)
    for k in (0, 9, -1, 100):
        refused(aggr(dst, None, ii, vv, ks, wv, k, n, 0, None), "sparse_aggregate", "k=%d" % k)
    refused(aggr(None, None, ii, vv, ks, wv, 2, n, 0, None), "sparse_aggregate", "null")
    refused(aggr(dst, None, None, vv, ks, wv, 2, n, 0, None), "sparse_aggregate", "null")
    refused(aggr(dst, None, ii, None, ks, wv, 2, n, 0, None), "sparse_aggregate", "null")
    refused(aggr(dst, None, ii, vv, None, wv, 2, n, 0, None), "sparse_aggregate", "null")
    refused(aggr(dst, None, ii, vv, ks, None, 2, n, 0, None), "sparse_aggregate", "null")
    refused(aggr(dst, None, arr([idx, None, idx]), vv, ks, wv, 3, n, 0, None), "sparse_aggregate", "index buffer 1 is null")
    refused(aggr(dst, None, ii, arr([val, val, None]), ks, wv, 3, n, 0, None), "sparse_aggregate", "value buffer 2 is null")
    refused(aggr(dst, None, ii, vv, (C.c_size_t * 2)(4, n + 1), wv, 2, n, 0, None), "sparse_aggregate", "upload 1", "keep=%d" % (n + 1))
    refused(aggr(dst, None, ii, vv, ks, wv, 2, 2 ** 31, 0, None), "sparse_aggregate", "2^31")
    refused(aggr(dst + 4, None, ii, vv, ks, wv, 2, n, 0, None), "sparse_aggregate", "aligned")
    refused(aggr(dst, x + 8, ii, vv, ks, wv, 2, n, 0, None), "sparse_aggregate", "aligned")
    refused(aggr(dst, x, arr([idx, idx + 4]), vv, ks, wv, 2, n, 1, None), "sparse_aggregate", "aligned")
    refused(aggr(dst, x, ii, arr([val + 8, val]), ks, wv, 2, n, 1, None), "sparse_aggregate", "aligned")
    assert aggr(dst, x, ii, vv, (C.c_size_t * 8)(), wv, 8, 0, 1, None) == 0    # n = 0
    for raw, _ in keep:
        assert not raw.any()                                                  # nothing was written


def test_sparse_kernels_use_no_scratch_memory(built_lib):
    """every kernel of csrc/sparse.hip (zero, 2 first passes, 2 digit passes, 2 selects, count, scan, 2 emits, K = 1..8 aggregates; both
    storage builds): a lane's eight elements and an upload's cursors are registers, so scratch memory would mean an array indexed at run time"""
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(REPO, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    ks = kr.kernels(built_lib.LIB_PATH)
    bf16 = os.path.join(os.path.dirname(built_lib.LIB_PATH), "libfedfr_hip_bf16.so")
    if os.path.exists(bf16) and os.path.basename(built_lib.LIB_PATH) != "libfedfr_hip_bf16.so":
        ks.update({"bf16:" + k: v for k, v in kr.kernels(bf16).items()})
    builds = 2 if any(k.startswith("bf16:") for k in ks) else 1
    tk = {n: r for n, r in ks.items() if re.match(r"(bf16:)?_Z\d+topk_[a-z0-9]+_kernel", n)}      # (the mangled name STARTS with topk_: not pfc_topk_kernel)
    ag = {n: r for n, r in ks.items() if "sparse_aggregate_kernel" in n}
    assert len(tk) == 11 * builds and len(ag) == 8 * builds, (sorted(tk), len(ag))
    bad = [(n, r) for n, r in list(tk.items()) + list(ag.items()) if r["scratch"]]
    assert not bad, bad


# ---- Python surface ----------------------------------------------------------------------------------------------------------------------
def test_keep_count_edges():
    from fedfr_amd import compress
    assert compress.keep_count(100, 0.01) == 1 and compress.keep_count(101, 0.01) == 2 and compress.keep_count(100, 1) == 100
    assert compress.keep_count(100, 1.0) == 100 and compress.keep_count(3, 1e-9) == 1 and compress.keep_count(1, 0.5) == 1
    assert compress.keep_count(65156160, 0.01) == 651562 and compress.keep_count(65156160, 0.001) == 65157
    assert compress.keep_count(10, np.float32(0.5)) == 5
    for n in (1, 7, 4103, 65156160):
        for ratio in (0.001, 0.01, 0.05, 0.5, 1.0):
            assert compress.keep_count(n, ratio) == S.keep_count(n, ratio)
    for bad in (0, 0.0, -0.01, 1.0001, 2, float("nan"), float("inf"), "0.01", None, True):
        with pytest.raises(ValueError, match=re.escape(repr(bad))):
            compress.keep_count(100, bad)


def test_topk_compressor_and_fedsparse_refuse_what_they_cannot_serve(built_lib):
    from fedfr_amd import compress, server
    from fedfr_amd.client import FlatStateDict
    for bad in (0, -1, 1.5, "0.01", None, True, float("nan")):
        with pytest.raises(ValueError, match="topk_ratio"):
            compress.TopKCompressor(bad)
    comp = compress.TopKCompressor()
    assert comp.ratio == 0.01 and comp.error_feedback and comp.residual is None and comp.workspace is None
    cpu = FlatStateDict.from_flat((torch.zeros(8), torch.zeros(0), torch.zeros(0, dtype=torch.int64)), [], [])
    with pytest.raises(RuntimeError, match="GPU"):
        comp.compress(cpu, cpu)                                               # FlatStateDicts, but not on the GPU
    with pytest.raises(RuntimeError, match="FlatStateDict"):
        comp.compress({"w": torch.zeros(8)}, cpu)
    with pytest.raises(RuntimeError, match="FlatStateDict"):
        comp.compress(cpu, {"w": torch.zeros(8)})
    assert comp.residual is None and comp.workspace is None                   # nothing was allocated for a refused call

    def upload(n=8, keep=2, idx_dtype=torch.int32, val_dtype=torch.float32):
        return compress.SparseDelta(torch.zeros(keep, dtype=idx_dtype), torch.zeros(keep, dtype=val_dtype), n, keep, torch.zeros(3),
                                    torch.zeros(2, dtype=torch.int64), torch.zeros(1, dtype=torch.int32))
    up = upload()
    assert up.nbytes == 16 + 12 + 16 and up.dense_nbytes == 32 + 12 + 16 and up.ratio == up.nbytes / up.dense_nbytes and up.nonfinite_count() == 0
    with pytest.raises(RuntimeError, match="FlatStateDict"):
        server.FedSparse({"w": torch.zeros(8)}, [up], [1.0])
    with pytest.raises(RuntimeError, match="SparseDelta"):
        server.FedSparse(cpu, [cpu], [1.0])
    with pytest.raises(RuntimeError, match="SparseDelta"):
        server.FedSparse(cpu, [], [])
    with pytest.raises(RuntimeError, match="weights"):
        server.FedSparse(cpu, [up, up], [1.0])
    with pytest.raises(ValueError, match="clip_norm"):
        server.FedSparse(cpu, [up], [1.0], server.ServerOptimizer("AVGM", clip_norm=1.0))
    with pytest.raises(ValueError, match="robust"):
        server.FedSparse(cpu, [up], [1.0], server.RobustAggregator("CoordMedian"))
    with pytest.raises(RuntimeError, match="GPU"):
        server.FedSparse(cpu, [up], [1.0])


def test_fedsparse_refuses_mixed_sizes_and_wrong_dtypes(monkeypatch):
    """the checks of the uploads themselves come behind the device check of the global state; with that one stubbed they can be reached
    without a GPU, and nothing is launched"""
    from fedfr_amd import _C, compress, server
    from fedfr_amd.client import FlatStateDict
    monkeypatch.setattr(server, "_check_states", lambda *a: None)
    monkeypatch.setattr(_C, "call", lambda *a: pytest.fail("a kernel was launched for a refused call"))
    cpu = FlatStateDict.from_flat((torch.zeros(8), torch.zeros(0), torch.zeros(0, dtype=torch.int64)), [], [])

    def upload(n=8, keep=2, idx_dtype=torch.int32, val_dtype=torch.float32, entries=None):
        entries = keep if entries is None else entries
        return compress.SparseDelta(torch.zeros(entries, dtype=idx_dtype), torch.zeros(entries, dtype=val_dtype), n, keep, torch.zeros(0),
                                    torch.zeros(0, dtype=torch.int64), torch.zeros(1, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="9 parameters among updates for 8"):
        server.FedSparse(cpu, [upload(), upload(n=9)], [1.0, 1.0])
    with pytest.raises(RuntimeError, match="9 entries for 8 parameters"):
        server.FedSparse(cpu, [upload(keep=9)], [1.0])
    with pytest.raises(RuntimeError, match="idx must be a contiguous int32"):
        server.FedSparse(cpu, [upload(idx_dtype=torch.int64)], [1.0])
    with pytest.raises(RuntimeError, match="val must be a contiguous float32"):
        server.FedSparse(cpu, [upload(val_dtype=torch.float64)], [1.0])
    with pytest.raises(RuntimeError, match="idx must be a contiguous int32 tensor of 2 entries"):
        server.FedSparse(cpu, [upload(entries=3)], [1.0])


def test_server_train_refuses_topk_settings_before_any_client_trains():
    from fedfr_amd import server

    def world(aggr, nclients, **extra):
        class Args:
            network, loss, local_epoch, output_dir, BCE_local, aggr_alg = "iresnet18", "CosFace", 1, "/tmp", False, aggr

        for k_, v_ in extra.items():
            setattr(Args, k_, v_)

        class NeverTrains:
            cid = 0

            def __getattr__(self, name):
                raise AssertionError("a client was touched (%s): the round has started" % name)

            def __setattr__(self, name, value):
                raise AssertionError("a client was touched (%s): the round has started" % name)
        return server.Server([NeverTrains() for _ in range(nclients)], None, Args, device=torch.device("cpu"))

    for kind in sorted(server.ROBUST_ALG_KINDS):
        with pytest.raises(ValueError, match=r"topk_ratio=0.01.*%s" % kind):
            world(kind, 5, topk_ratio=0.01).train()                           # a robust rule needs whole states
    for aggr in ("FedAvg", "FedAdam"):
        with pytest.raises(ValueError, match=r"topk_ratio=0.05.*clip_norm=2.5"):
            world(aggr, 3, topk_ratio=0.05, clip_norm=2.5).train()
    for bits in (4, 8):
        with pytest.raises(ValueError, match=r"topk_ratio=0.01.*compress_bits=%d" % bits):
            world("FedAvg", 3, topk_ratio=0.01, compress_bits=bits).train()
    for bad in (-0.01, 1.5, 2, "0.01", float("nan"), True):
        with pytest.raises(ValueError, match=r"topk_ratio.*%s" % re.escape(repr(bad))):
            world("FedAvg", 3, topk_ratio=bad).train()
    for aggr, extra in (("FedAvg", {"topk_ratio": 0.01}), ("FedProx", {"topk_ratio": 1.0}), ("FedAvgM", {"topk_ratio": 0.001, "clip_norm": 0.0}),
                        ("FedYogi", {"topk_ratio": 0.5, "error_feedback": False}), ("FedAvg", {"topk_ratio": 0, "clip_norm": 2.5}),
                        ("CoordMedian", {"topk_ratio": 0}), ("FedAvg", {"topk_ratio": None}), ("FedAvg", {"topk_ratio": 0.0, "compress_bits": 8})):
        with pytest.raises(AssertionError, match="the round has started"):    # served: the round starts (and meets the stub)
            world(aggr, 3, **extra).train()
