"""CPU-side proof that tests/tail_cases.py asks for what a correct kernel can deliver and for nothing less: the same formulas at fp32 in the
kernels' operation order stay within a QUARTER of every tolerance; every exact case is admissible; the case tables agree with the restated
dispatch rules; and for each check one mutant of the kernel's arithmetic — an off-by-one row group, a dropped K tail, the biased variance in
place of the unbiased one, the wrong mask field, a skipped slab — is rejected by it."""
import numpy as np
import pytest
import torch

import tail_cases as T

f32, f64 = T.f32, T.f64
S16 = [torch.float16, torch.bfloat16]


def rejected(fn, *a, **k):
    with pytest.raises(AssertionError):
        fn(*a, **k)


# ------------------------------------------------------------------------------------------------ BatchNorm1d
def test_bn1d_table_covers_every_value_and_both_instantiations():
    Bs, Cs = {b for b, _ in T.BN_SHAPES}, {c for _, c in T.BN_SHAPES}
    assert Bs == {1, 2, 7, 8, 9, 127, 128, 129, 200} and Cs == {8, 64, 72, 100, 512}
    assert T.bn_uses_cache(128) and not T.bn_uses_cache(129)
    assert {T.bn_uses_cache(b) for b in Bs} == {True, False}
    assert all(T.bn_ldt(b) > b and T.bn_ldt(b) % 8 == 0 for b in Bs)


@pytest.mark.parametrize("B,C", T.BN_SHAPES)
def test_bn1d_fp32_in_kernel_order_holds_a_quarter_of_the_tolerance(B, C):
    i = T.BnInputs(B, C)
    for training in (True, False):
        for ug, ub in ((1, 1), (0, 1), (1, 0), (0, 0)):
            ref, got = T.bn_fwd_ref(i, training, ug, ub), T.bn_fwd_kernel_order(i, training, ug, ub)
            for k, q in ref.items():
                T.check(got[k], q, "fwd %s" % k, frac=0.25)
            want = (i.beta if ub else torch.zeros(C))[T.BN_CONST_COL]
            if training:                      # the constant column: y == beta exactly, rstd == 1 / sqrt(eps) to fp32
                assert bool((got["y"][:, T.BN_CONST_COL] == want).all())
                assert abs(float(got["save_rstd"][T.BN_CONST_COL]) * np.sqrt(np.float64(np.float32(T.BN_EPS))) - 1.0) < 2.0 ** -23
    for frozen in (False, True):
        for ug in (1, 0):
            ref, got = T.bn_bwd_ref(i, ug, frozen), T.bn_bwd_kernel_order(i, ug, frozen)
            for k, q in ref.items():
                T.check(got[k], q, "bwd %s" % k, frac=0.25)
    if B == 1:
        assert bool((T.bn_bwd_ref(i, 1, False)["dx"].value == 0).all())


def test_bn1d_b2_conditioning_is_what_the_docstring_says():
    i = T.BnInputs(2, 64)
    var = i.x.double().var(0, unbiased=False)
    assert float(var.max()) <= 1.6e-5 and T.BN_EPS / (float(var.max()) + T.BN_EPS) > 0.38


def test_bn1d_mutants_are_rejected():
    i = T.BnInputs(9, 512)                                   # the ninth row is the second of row group 0; row 7 is the only one of group 7
    ref = T.bn_fwd_ref(i, True, 1, 1)
    good, rg, biased = (T.bn_fwd_kernel_order(i, True, 1, 1, m) for m in (None, "row_group", "biased"))
    for k in ("y", "save_mean", "save_rstd", "rm", "rv"):
        T.check(good[k], ref[k], k)
        rejected(T.check, rg[k], ref[k], k)
    rejected(T.check, biased["rv"], ref["rv"], "rv")          # (1 - 1 / 9) of the variance: 1.1e-2 of rv
    for k in ("y", "save_mean", "save_rstd", "rm"):
        T.check(biased[k], ref[k], k)
    i = T.BnInputs(200, 8)
    bref, bad = T.bn_bwd_ref(i, 1, False), T.bn_bwd_kernel_order(i, 1, False, "row_group")
    for k in ("dx", "dbeta", "dx_colsum"):
        rejected(T.check, bad[k], bref[k], k)
    # a 16-bit side output strided by B instead of ldt, or rounded twice, is not the rounding of dx
    dx = T.bn_bwd_kernel_order(i, 1, False)["dx"]
    for s16 in S16:
        rejected(T.same16, (dx * (1 + 2.0 ** -9)).to(s16), dx.to(s16))


# ------------------------------------------------------------------------------------------------ slabs
def test_slab_table_reaches_both_kernels_and_every_loop():
    wide = [c for c in T.SLAB_CASES if T.slabs_wide(*c)]
    narrow = [c for c in T.SLAB_CASES if not T.slabs_wide(*c)]
    assert {ns for ns, _ in narrow} == {1, 2, 15, 16} and {ns for ns, _ in wide} == {16, 17, 31, 32, 33, 40, 128}
    assert (16, 4 * 65536) in wide and (16, 4 * 65536 + 4) in narrow
    assert any(n // 4 > 2 * T.SLAB_GRID_CAP * 256 for _, n in narrow)
    assert all(n % 4 == 0 for _, n in T.SLAB_CASES)
    assert {T.slabs_wide(ns, n) for ns, n, _ in T.SLAB_BIAS_CASES} == {True, False} == {T.slabs_wide(*c) for c in T.SLAB_PAIR_CASES}
    assert {bn for _, _, bn in T.SLAB_BIAS_CASES} == {4, 512}


@pytest.mark.parametrize("nsplit,n", [c for c in T.SLAB_CASES if c[0] * c[1] < 2 ** 23])
def test_slab_order_holds_a_quarter_and_a_skipped_slab_is_rejected(nsplit, n):
    slabs = T.slab_inputs(nsplit, n)
    got = T.slab_sum_order(slabs)
    T.slab_check(got, slabs, frac=0.25)
    if nsplit > 1:
        rejected(T.slab_check, T.slab_sum_order(slabs, skip=nsplit - 1), slabs)
        rejected(T.slab_check, T.slab_sum_order(slabs, skip=nsplit // 2), slabs)
    if nsplit >= 17:                                          # the other kernel's order is a different rounding somewhere: the restatement is sharp
        fold = slabs[0].copy()
        for s in range(1, nsplit):
            fold = fold + slabs[s]
        assert T.slabs_wide(nsplit, n) and not np.array_equal(fold, got) or n <= 4


def test_slab_bias_goes_to_element_mod_bias_n():
    for nsplit, n, bias_n in T.SLAB_BIAS_CASES:
        slabs, bias = T.slab_inputs(nsplit, n), T.slab_bias(bias_n)
        T.slab_check(T.slab_sum_order(slabs, bias), slabs, bias, frac=0.25)
        rejected(T.slab_check, T.slab_sum_order(slabs, np.roll(bias, 1)), slabs, bias)
        rejected(T.slab_check, T.slab_sum_order(slabs), slabs, bias)


# ------------------------------------------------------------------------------------------------ dropout
def test_dropout_restatement_keep_rate_and_independence():
    n = 200704
    for p in T.DROPOUT_P:
        thr = T.dropout_thr(p)
        keep = 1.0 - thr / 65536.0
        assert 0 <= keep - (1.0 - float(np.float32(p))) < 2.0 ** -16     # thr is p * 65536 rounded down: the keep rate exceeds 1 - p by less than 2^-16
        sigma = np.sqrt(keep * (1 - keep) / n)
        for seed in T.DROPOUT_SEEDS:
            masks = [T.dropout_mask(n, p, seed, st) for st in T.DROPOUT_STEPS]
            for m in masks:
                assert set(np.unique(m)) <= {0, 1}
                assert abs(m.mean() - keep) < 4 * sigma, (p, seed, m.mean(), keep)
            agree = keep * keep + (1 - keep) ** 2
            s2 = np.sqrt(agree * (1 - agree) / n)
            assert abs((masks[0] == masks[1]).mean() - agree) < 4 * s2
    assert abs((T.dropout_mask(n, 0.4, 0, 0) == T.dropout_mask(n, 0.4, 0, 1)).mean() - 0.52) < 2e-3
    for nn in T.DROPOUT_N:
        assert np.array_equal(T.dropout_mask(n, 0.4, 100, 7)[:nn], T.dropout_mask(nn, 0.4, 100, 7))      # a pure function of (seed, step, index)


def test_dropout_wrong_mask_field_is_rejected():
    for n in T.DROPOUT_N:
        good = T.dropout_mask(n, 0.5, 100, 1)
        assert not np.array_equal(T.dropout_mask(n, 0.5, 100, 1, field_shift=1), good)
        assert not np.array_equal(T.dropout_mask(n, 0.5, 100, 2), good) and not np.array_equal(T.dropout_mask(n, 0.5, 101, 1), good)
    for s16 in S16:
        x = T.dropout_values(4104, s16)
        m = T.dropout_mask(4104, 0.4, 0, 0)
        want = T.dropout_fwd_expect(x, m, 0.4)
        assert bool((want[torch.from_numpy(m == 0)].view(torch.int16) == 0).all()) and bool((want[torch.from_numpy(m == 1)] != 0).all())
        rejected(T.same16, T.dropout_fwd_expect(x, T.dropout_mask(4104, 0.4, 0, 0, field_shift=1), 0.4), want)
        # a scale applied in the storage type (1 / (1 - p) rounded to 16 bits first) is not storage(x * inv_keep)
        rejected(T.same16, (x.float() * float(torch.tensor(float(T.dropout_inv_keep(0.4))).to(s16))).to(s16) * torch.from_numpy(m).to(s16), want)
    assert T.DROPOUT_N_FWD_BIG // 8 > T.DROPOUT_GRID_CAP * 256 and T.DROPOUT_N_BWD_BIG // 4 > T.DROPOUT_GRID_CAP * 256


# ------------------------------------------------------------------------------------------------ layout, casts, shadows
def test_layout_and_cast_cases():
    assert any(hw % 64 for _, _, hw in T.NHWC_SHAPES) and any(c % 64 for _, c, _ in T.NHWC_SHAPES) and (2, 512, 49) in T.NHWC_SHAPES
    x = T.uniform((2, 66, 49), 5)
    for s16 in S16:
        y = T.nhwc_ref(x, s16)
        assert y.shape == (2, 49, 66) and float(y[1, 48, 65]) == float(x[1, 65, 48].to(s16))
        rejected(T.same16, T.nhwc_ref(x.roll(1, 2), s16), y)
    assert T.CAST_N[0] < 16 and T.CAST_N[1] == 8 and T.CAST_N[2] % 8 and T.CAST_N[3] // 8 + 1 > T.CAST_GRID_CAP * 256 and T.CAST_N[3] % 8
    e = T.cast_edge_values()
    assert bool(torch.isnan(e).sum() == 1) and bool(torch.isinf(e).any())
    h, b = e.to(torch.float16), e.to(torch.bfloat16)
    assert bool(torch.isinf(h[e == 65520.0]).all()) and float(h[e == torch.tensor(65519.996, dtype=f32)][0]) == 65504.0
    assert float(h[7]) == 1.0 and float(h[8]) == 1 + 2.0 ** -9 and float(b[11]) == 1.0 and float(b[12]) == 1 + 2.0 ** -6      # ties go to even
    assert bool((h[e.abs() == 2.0 ** -25] == 0).all()) and float(h[e == 1.5 * 2.0 ** -25][0]) == 2.0 ** -24
    assert bool(torch.isinf(b[-8:][[0, 1, 4, 5]]).all()) and bool(torch.isfinite(b[-8:][[2, 3, 6, 7]]).all())
    x = T.cast_input(77)
    for s16 in S16:
        # truncation instead of round-to-nearest-even is rejected
        trunc = (x.view(torch.int32) & -65536).view(f32).to(s16) if s16 == torch.bfloat16 else (x.view(torch.int32) & -8192).view(f32).to(s16)
        rejected(T.same16, trunc, x.to(s16))
    w = T.uniform((64, 3, 3, 128), 6)
    for s16 in S16:
        d = T.dgrad_shadow_ref(w, s16)
        assert d.shape == (128, 3, 3, 64) and float(d[5, 0, 2, 7]) == float(w[7, 2, 0, 5].to(s16))
    lay, total = T.shadow_layout([("conv1.weight", 0, 0, 0, (64, 3, 3, 3)), ("layer1.0.conv1.weight", 0, 0, 1732, (64, 64, 3, 3)),
                                  ("layer1.0.bn1.weight", 1, 0, 100, (64, 0, 0, 0)), ("layer1.0.downsample.0.weight", 0, 0, 9000, (128, 64, 1, 1))], 20003)
    assert lay == [("layer1.0.conv1.weight", 1732, 20008, 64, 64, 3), ("layer1.0.downsample.0.weight", 9000, 20008 + 36864, 128, 64, 1)]
    assert total == 20008 + 36864 + 8192


# ------------------------------------------------------------------------------------------------ plain GEMMs
def test_gemm_tables_agree_with_the_restated_dispatch_rules():
    for (M, N, K), want in T.NT_ROWS:
        assert T.nt_expected(M, N, K) == want, ((M, N, K), T.nt_expected(M, N, K))
        assert K % 8 == 0 and N % 4 == 0 and T.gemm_exact_admissible(K)
    assert sorted({s for _, (s, _) in T.NT_ROWS}) == [0, 1, 2, 3, 17]
    assert sum(1 for (M, N, K), _ in T.NT_ROWS if K % 64) >= 5
    M, N, K = 7, 132, 584                                     # the second split: K-steps 5..9, the last one 8 columns wide
    per = T.cdiv(T.cdiv(K, 64), 2)
    assert per == 5 and K - per * 64 < per * 64 and K % 64 == 8
    assert T.nt_expected(1024, 1024, 4104, nt_glds=0) == (2, 4)
    for (Kp, NI, NJ), slot in T.TN_ROWS:
        assert T.tn_expected_slot(NI, NJ) == slot and NI % 8 == 0 and NJ % 8 == 0 and T.gemm_exact_admissible(Kp)
    assert sorted(s for _, s in T.TN_ROWS) == [4, 5, 6, 7] and sum(1 for (Kp, _, _), _ in T.TN_ROWS if Kp == 1) == 2


@pytest.mark.parametrize("s16", S16)
@pytest.mark.parametrize("M,N,K", [r for r, _ in T.NT_ROWS])
def test_gemm_fp32_holds_a_quarter_and_a_dropped_k_tail_is_rejected(M, N, K, s16):
    rows = min(M, 48)                                         # the leading rows: the bound is per element, the inputs are i.i.d.
    splits = T.gemm_nt_pick_splits(M, N, K)
    for exact in (True, False):
        a, b = T.gemm_operands(rows, N, K, exact, s16, 11)
        assert torch.equal(a.to(s16).to(f32), a) and torch.equal(b.to(s16).to(f32), b)
        ref, S = T.gemm_ref(a, b)
        if exact:
            assert float(S.max()) < 2 ** 24
        got = a @ b.t()                                       # fp32, in whatever order the host library takes: the kernels' order is as arbitrary
        T.gemm_check(got, ref, S, K, splits, exact, frac=0.25)
        if K % 64:
            bad, _ = T.gemm_ref(a, b, f32, k_drop=K % 64)
            rejected(T.gemm_check, bad, ref, S, K, splits, exact)


@pytest.mark.parametrize("s16", S16)
@pytest.mark.parametrize("Kp,NI,NJ", [r for r, _ in T.TN_ROWS])
def test_gemm_tn_fp32_holds_a_quarter_and_a_dropped_row_is_rejected(Kp, NI, NJ, s16):
    nj = min(NJ, 512)
    for exact in (True, False):
        p, q = T.gemm_operands(NI, nj, Kp, exact, s16, 12)    # [NI][Kp], [NJ][Kp]: the transposes of the kernel's operands
        ref, S = T.gemm_ref(p, q)
        T.gemm_check(p @ q.t(), ref, S, Kp, 1, exact, frac=0.25)
        bad, _ = T.gemm_ref(p, q, f32, k_drop=1)
        rejected(T.gemm_check, bad, ref, S, Kp, 1, exact)


# ------------------------------------------------------------------------------------------------ the four small entry points
def test_small_entry_point_restatements():
    src, acc = T.fedavg_i64_inputs(257)
    assert int(src[0]) == 2 ** 24 + 1 and float(np.float32(src[0])) != float(src[0])          # the conversion rounds
    v, tr = T.fedavg_i64_order(acc, src, 0.3, True)
    v0, _ = T.fedavg_i64_order(acc, src, 0.3, False)
    exact = acc.astype(np.float64) + np.float64(np.float32(0.3)) * src.astype(np.float64)
    assert np.all(np.abs(v - exact) <= 3 * 2.0 ** -24 * (np.abs(exact) + acc)) and np.all(tr == np.trunc(v)) and not np.array_equal(v, v0)
    assert np.any(v != (acc.astype(np.float64) + 0.3 * src).astype(np.float32))                 # one rounding is not three
    r0, r1 = T.pfc_rand_order(4099, 5, 0), T.pfc_rand_order(4099, 5, 1)
    assert r0.dtype == np.float32 and r0.min() >= 0 and r0.max() < 1 and not np.array_equal(r0, r1)
    assert abs(r0.mean() - 0.5) < 4 * np.sqrt(1 / 12 / 4099) and len(np.unique(r0)) > 4000
    lab = torch.tensor([9, 10, 14, 15, 12, -1], dtype=torch.int64)
    out, perm = T.pfc_localize_ref(lab, 10, 5, torch.zeros(5))
    assert out.tolist() == [-1, 0, 4, -1, 2, -1] and perm.tolist() == [2.0, 0.0, 2.0, 0.0, 2.0]
