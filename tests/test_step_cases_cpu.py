"""CPU-side proof that tests/step_cases.py asks for what a correct kernel can deliver and for nothing less: the toleranced formulas at fp32
in the kernels' operation order stay within a QUARTER of their tolerance; every exact case is admissible (the integer bound of colflag,
the planted shadow values in both storage types, the 1/8 grid of the ROC features, the fused multiply-add's Fraction fallback); the case
tables reach what they claim under the restated launch and dispatch rules; and one mutant per check is rejected by it."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import step_cases as S

f32, f64 = S.f32, S.f64
S16 = [torch.float16, torch.bfloat16]


def rejected(fn, *a, **k):
    with pytest.raises(AssertionError):
        fn(*a, **k)


def differ(a, b):
    return int((S.bits32(a) != S.bits32(b)).sum())


# ------------------------------------------------------------------------------------------------ SGD
def test_fma32_rounds_once_and_the_fallback_agrees():
    # a b = 1 + 2^-24 exactly (16777217 = 24929 x 673), c = 2^-80: the float64 sum loses c and sits on the fp32 tie, which rounds DOWN to 1;
    # the exact sum is above the tie and rounds UP
    a, b, c = f32(24929 * 2.0 ** -24), f32(673.0), f32(2.0 ** -80)
    assert Fraction(float(a)) * Fraction(float(b)) == 1 + Fraction(1, 2 ** 24)
    with np.errstate(all="ignore"):
        naive = f32(f64(a) * f64(b) + f64(c))
    assert naive == f32(1.0)
    stats = []
    assert S.fma32(a, b, c, stats=stats)[0] == f32(1 + 2.0 ** -23) and stats == [1]
    assert S.fma32(a, b, -c)[0] == f32(1.0)
    # below the fp32 normal range the second rounding is at another bit: also through the fallback
    assert S.fma32(f32(2.0 ** -100), f32(2.0 ** -40), f32(2.0 ** -149))[0] == f32(2.0 ** -140 + 2.0 ** -149)
    # on ordinary draws the fast path and the all-Fraction path agree bit for bit, and the fallback is (almost) never taken
    p, g = S.sgd_inputs(4103)
    stats = []
    fast = S.fma32(f32(0.37), p, g, stats=stats)
    S.same32(fast, S.fma32(f32(0.37), p, g, exact_all=True), "fma32")
    assert stats[0] <= 2
    for q in (Fraction(1, 3), Fraction(-5, 7), 1 + Fraction(1, 2 ** 24), 1 + Fraction(3, 2 ** 24), Fraction(1, 2 ** 149) / 2):
        r = S.round_fraction_f32(q)
        lo, hi = np.nextafter(r, f32(-np.inf)), np.nextafter(r, f32(np.inf))
        assert all(abs(Fraction(float(r)) - q) <= abs(Fraction(float(o)) - q) for o in (lo, hi))
    assert S.round_fraction_f32(1 + Fraction(1, 2 ** 24)) == f32(1.0) and S.round_fraction_f32(1 + Fraction(3, 2 ** 24)) == f32(1 + 2.0 ** -22)


def test_sgd_table_has_a_wrapping_size_a_tail_only_size_and_every_remainder():
    assert S.sgd_grid(S.SGD_WRAP_N) == S.SGD_GRID_CAP and S.sgd_wraps(S.SGD_WRAP_N) and not S.sgd_wraps(S.SGD_GRID_CAP * 256 * 4 - 4)
    assert [n for n in S.SGD_N if S.sgd_wraps(n)] == [S.SGD_WRAP_N] and S.SGD_WRAP_N % 4 == 3
    assert {n for n in S.SGD_N if S.sgd_tail_only(n)} == {1, 2, 3}
    assert {n % 4 for n in S.SGD_N} == {0, 1, 2, 3} and any(S.sgd_grid(n) > 1 for n in S.SGD_N if not S.sgd_wraps(n))
    assert S.sgd_grid(1023) == 1 and S.sgd_grid(1024) == 2                                  # n / 4 + 1 work items: 1024 is the first second block
    assert [n for n in S.AXPY_N if S.sgd_wraps(n)] == [S.SGD_GRID_CAP * 256 * 4 + 5] and any(n < 4 for n in S.AXPY_N)
    wrap_pos = S.sgd_bad_positions(S.SGD_WRAP_N)
    assert 0 in wrap_pos and S.SGD_WRAP_N - 1 in wrap_pos and any(q // 4 >= S.SGD_GRID_CAP * 256 and q < S.SGD_WRAP_N // 4 * 4 for q in wrap_pos)
    assert any(q >= S.SGD_WRAP_N // 4 * 4 for q in wrap_pos) and any(0 < q < 4 * 256 for q in wrap_pos)


@pytest.mark.parametrize("n", [1023, 4103])
def test_sgd_rounding_order_mutants_are_rejected(n):
    """with O(1) hyper-parameters each mutant changes hundreds of elements; at the product's weight decay the unfused one changes none"""
    p, g = S.sgd_inputs(n)
    lr, mu, wd = S.SGD_HYPER
    (p1, b1), (p2, b2) = S.sgd_two_steps(n)
    g2 = S.sgd_second_grad(n)
    for m in S.SGD_MUTANTS:
        mp1, mb1, _, _ = S.sgd_ref(p, g, None, lr, mu, wd, 1, mutant=m)
        mp2, mb2, _, _ = S.sgd_ref(p1, g2, b1, lr, mu, wd, 0, mutant=m)
        changed = differ(mp1, p1) + differ(mb1, b1) + differ(mp2, p2) + differ(mb2, b2)
        assert changed >= 100, (m, changed)
        rejected(S.same32, np.concatenate([mp1, mb1, mp2, mb2]), np.concatenate([p1, b1, p2, b2]))
    if n == 4103:
        lr, mu, wd = S.SGD_HYPER_PRODUCT
        a = S.sgd_ref(p, g, None, lr, mu, wd, 1)
        b = S.sgd_ref(p, g, None, lr, mu, wd, 1, mutant="unfused_wd")
        assert differ(a[0], b[0]) + differ(a[1], b[1]) < 20                                 # why the bit-exact tier does not use these


def test_sgd_scaled_reference_skips_and_a_momentum_updating_skip_is_rejected():
    n = 1025
    p, g = S.sgd_inputs(n)
    lr, mu, wd = S.SGD_HYPER
    (p1, b1), (p2, b2) = S.sgd_two_steps(n)
    gs = S.SGD_SCALE
    scaled = (g / f32(gs)).astype(f32)                                                     # a power of two: exact
    cp, cb, cg, ovf = S.sgd_ref(p, scaled, None, lr, mu, wd, 1, gs=gs)
    S.same32(cp, p1), S.same32(cb, b1), S.same32(cg, g)
    assert ovf == 0
    pos = S.sgd_bad_positions(n)
    assert 0 in pos and n - 1 in pos and n // 4 * 4 in pos and any(0 < q < n // 4 * 4 for q in pos)
    g2 = (S.sgd_second_grad(n) / f32(gs)).astype(f32)
    g2[pos] = S.sgd_bad_values(len(pos))
    for first, (p0, b0, want_p, want_b) in ((1, (p, None, p1, b1)), (0, (p1, b1, p2, b2))):
        gin = g2 if not first else np.where(np.isin(np.arange(n), pos), g2, scaled)
        bp, bb, bg, ovf = S.sgd_ref(p0, gin, b0, lr, mu, wd, first, gs=gs)
        keep = np.ones(n, bool)
        keep[pos] = False
        assert ovf == 1 and not np.isfinite(bg[pos]).any()
        S.same32(bp[pos], p0[pos]), S.same32(bb[pos], np.zeros(len(pos), f32) if first else b0[pos])
        S.same32(bp[keep], want_p[keep]), S.same32(bb[keep], want_b[keep])
        mp, mb, _, _ = S.sgd_ref(p0, gin, b0, lr, mu, wd, first, gs=gs, mutant="bad_updates_momentum")
        S.same32(mp, bp)
        rejected(S.same32, mb, bb)


@pytest.mark.parametrize("s16", S16, ids=["fp16", "bf16"])
def test_planted_shadow_values_come_out_of_the_reference_and_hit_their_edges(s16):
    v = S.shadow_plants(s16)
    fi = torch.finfo(s16)
    r = torch.from_numpy(v).to(s16)
    sub = (r.float().abs() < fi.tiny)
    assert int((sub & (r != 0)).sum()) >= 3 and int((sub & (r == 0)).sum()) >= 2            # subnormal results, and ties that reach zero
    # exact ties: the value is midway between its two neighbours in the storage type (the one toward zero, and that one's successor)
    lo = S.shadow_mutant(v, s16, "truncate")
    hi = (lo.view(torch.int16) + 1).view(s16)
    av = torch.from_numpy(v).double().abs()
    ties = torch.isfinite(hi.double()) & (av - lo.double().abs() == hi.double().abs() - av) & (lo.double().abs() != av)
    assert int(ties.sum()) >= 6 and int((ties & (r.double().abs() > av)).sum()) >= 2 and int((ties & (r.double().abs() < av)).sum()) >= 2, ties
    assert bool((r.view(torch.int16)[ties] & 1 == 0).all())                                 # ... and goes to the even one
    if s16 == torch.float16:
        assert int(torch.isinf(r).sum()) == 3 and float(torch.from_numpy(v)[~torch.isinf(r)].abs().max()) > 65504
    seen_tail, tail_shows = set(), set()
    for j in range(S.shadow_plant_calls(s16)):
        p, g, body, tail = S.shadow_plant_case(s16, j)
        assert len(p) % 4 == 3 and body.max() < len(p) // 4 * 4 <= tail.min() and {int(b) % 4 for b in body} == {0, 1, 2, 3}
        pn, _, _, _ = S.sgd_ref(p, g, None, *S.SGD_HYPER, 1)
        S.same32(pn[body], v, "planted body")                                              # the new p IS the planted value
        S.same32(pn[tail], p[tail], "planted tail")
        seen_tail |= {float(t) for t in p[tail]}
        good = S.shadow_ref(pn, s16)
        for kind in ("truncate", "flush"):
            rejected(S.tc.same16, S.shadow_mutant(pn, s16, kind), good)
            rejected(S.tc.same16, S.shadow_mutant(pn, s16, kind)[body], good[body])         # the body alone shows it,
            if not torch.equal(S.tc.bits16(S.shadow_mutant(pn, s16, kind)[tail]), S.tc.bits16(good[tail])):
                tail_shows.add(kind)                                                        # and so does the tail of some call
    assert seen_tail == {float(t) for t in v} and tail_shows == {"truncate", "flush"}


def test_axpy_is_two_roundings():
    src, dst = S.uniform((4103,), 1).numpy(), S.uniform((4103,), 2).numpy()
    two = S.axpy_ref(dst, src, 0.3, True)
    fused = S.fma32(f32(0.3), src, dst)
    assert differ(two, fused) >= 100
    S.same32(S.axpy_ref(np.full(7, np.nan, f32), src[:7], 0.3, False), f32(0.3) * src[:7])


# ------------------------------------------------------------------------------------------------ PartialFC selection
def test_topk_tables_sit_on_both_sides_of_every_boundary():
    W, CH, R = S.TOPK_WIDE_MIN_N, S.TOPK_CHUNK, S.TOPK_ROUND
    assert {W - 1, W, W + 1, CH - 1, CH, CH + 1, 2 * CH + 3, R - 1, R, R + 1, 1, 2, 85000} <= set(S.TOPK_N)
    assert not S.topk_is_wide(True, W - 1) and S.topk_is_wide(True, W) and not S.topk_is_wide(False, 85000)
    for tab in (S.TOPK_N, S.TOPK_PATTERN_N, [n for n, _ in S.TOPK_TIE_CASES]):
        assert {S.topk_is_wide(True, n) for n in tab} == {True, False}
    assert any(n > 2 * CH for n in S.TOPK_PATTERN_N) and any(n > R and not S.topk_is_wide(True, n) for n in S.TOPK_PATTERN_N)
    for n in S.TOPK_N:
        assert {1, n} <= set(S.topk_ks(n)) and (n < 3 or n - 1 in S.topk_ks(n)) and all(1 <= k <= n for k in S.topk_ks(n))
    assert {e for _, e in S.TOPK_TIE_CASES} == {CH, R}
    assert any(e == CH and S.topk_is_wide(True, n) for n, e in S.TOPK_TIE_CASES) and any(e == R and n < W for n, e in S.TOPK_TIE_CASES)


def test_topk_patterns_force_the_pass_they_name():
    for n in S.TOPK_PATTERN_N:
        lo, mid = S.TOPK_PATTERNS["low10"](n).view(np.int32), S.TOPK_PATTERNS["mid11"](n).view(np.int32)
        assert len(np.unique(lo >> 10)) == 1 and len(np.unique(lo & 1023)) > 500
        assert len(np.unique(mid >> 21)) == 1 and len(np.unique(mid & 1023)) == 1 and len(np.unique((mid >> 10) & 2047)) > 500
        assert not S.TOPK_PATTERNS["zero"](n).view(np.int32).any()
        r = S.TOPK_PATTERNS["rand"](n)
        assert np.array_equal(r, np.round(r * 2 ** 24) / 2 ** 24) and r.min() >= 0 and r.max() < 1
        assert S.topk_npos(S.TOPK_PATTERNS["marks"](n)) == S.TOPK_MARKS > 2
        assert len(np.unique(S.TOPK_PATTERNS["levels"](n))) == 5


def test_topk_mutants_are_rejected():
    for n, edge in S.TOPK_TIE_CASES:
        v, ks = S.topk_tie_case(n, edge)
        a, b = S.topk_ref(v, ks[0]), S.topk_ref(v, ks[1])
        tie = np.arange(edge - 2, edge + 3)
        assert np.array_equal(np.intersect1d(a, tie), tie[:2]) and np.array_equal(np.intersect1d(b, tie), tie[:3])      # the cut falls at edge, then one later
        for k in ks:
            rejected(S.same_int, S.topk_ref(v, k, "last_tied"), S.topk_ref(v, k))
    for n in S.TOPK_PATTERN_N:
        v = S.TOPK_PATTERNS["low10"](n)
        k = n // 3
        rejected(S.same_int, S.topk_ref(v, k, "no_third_pass"), S.topk_ref(v, k))
        v = S.TOPK_PATTERNS["mid11"](n)
        S.same_int(S.topk_ref(v, k, "no_third_pass"), S.topk_ref(v, k))                     # (there the second pass has already decided)
        eq = S.topk_ref(S.TOPK_PATTERNS["equal"](n), k)
        assert np.array_equal(eq, np.arange(k)) and np.array_equal(S.topk_ref(S.TOPK_PATTERNS["zero"](n), k), np.arange(k))


def test_remap_and_rows_tables_and_mutants():
    for n in S.REMAP_N:
        for k in S.REMAP_K:
            lab, index = S.remap_inputs(n, k)
            assert np.all(np.diff(index) > 0) and lab[0] > index[-1] and S.remap_ref(lab, index)[0] == k     # absent and above all: the value k
            want = S.remap_ref(lab, index)
            assert np.array_equal(want[lab < 0], lab[lab < 0])
            m = lab >= 0
            assert np.array_equal(want[m], torch.searchsorted(torch.from_numpy(index), torch.from_numpy(lab[m])).numpy())
            if n >= 3:
                assert lab[1] == -1 and np.isin(lab[2], index)
                rejected(S.same_int, S.remap_ref(lab, index, side="right"), want)
    assert {n % 256 for n in S.REMAP_N} >= {0, 1, 255}
    assert {k % S.ROWS_PER_BLOCK for k in S.ROWS_K} == {0, 1, 3} and min(S.ROWS_K) < S.ROWS_PER_BLOCK < max(S.ROWS_K)
    assert {(d // 4) % S.ROW_LANES for d in S.ROWS_D} >= {0, 1, 63} and min(S.ROWS_D) == 4 and any(d // 4 > S.ROW_LANES for d in S.ROWS_D)
    table = S.uniform((S.ROWS_TABLE, 8), 3).numpy()
    for k in S.ROWS_K:
        idx = S.rows_index(k)
        ok = S.rows_valid(idx)
        assert ok[0] and (k < 5 or ok[-1]) and len(np.unique(idx[ok])) == int(ok.sum())
        if k >= 4:
            assert set(S.ROWS_BAD) <= set(idx.tolist())
        full = np.concatenate([idx, np.zeros(3, np.int64)])                                # guard entries behind the k indices: valid row numbers
        want = S.rows_gather_ref(table, full, k)
        assert np.isnan(want[k:]).all() and np.isnan(want[:k][~ok]).all() and not np.isnan(want[:k][ok]).any()
        rejected(S.same32, S.rows_gather_ref(table, full, k + 1), want)                     # `row > k`: one row too many
        src = S.uniform((len(full), 8), 4).numpy()
        rejected(S.same32, S.rows_scatter_ref(table, src, full, k + 1), S.rows_scatter_ref(table, src, full, k))
    for n in S.POSITIVE_N:
        c = S.positive_cases(n)
        assert S.topk_npos(c["none"]) == 0 and S.topk_npos(c["all"]) == n and S.topk_npos(c["ends"]) == min(n, 2)
    assert {n % 1024 for n in S.POSITIVE_N} >= {0, 1, 1023}


def test_chain_cases_take_both_branches_on_both_kernels():
    for nl, ns, batch, pos_win in S.CHAIN_CASES:
        lab = S.chain_labels(nl, batch, 1000)
        w, m = S.uniform((nl, 8), 5).numpy(), S.uniform((nl, 8), 6).numpy()
        c = S.chain_ref(nl, ns, lab, 1000, 7, 3, w, m)
        inside = (lab >= 1000) & (lab < 1000 + nl)
        assert 0 < inside.sum() < batch and c["npos"] == inside.sum() and (c["npos"] > ns) == pos_win
        assert len(c["index"]) == (c["npos"] if pos_win else ns)
        assert np.array_equal(c["index"][c["label"][inside]], lab[inside] - 1000)           # every positive is in the sample, at its remapped place
        assert np.array_equal(c["label"][~inside], np.full(int((~inside).sum()), -1))
        touched = np.zeros(nl, bool)
        touched[c["index"]] = True
        S.same32(c["weight"][~touched], w[~touched]), S.same32(c["weight"][touched], -w[touched])
    assert {S.topk_is_wide(True, nl) for nl, _, _, _ in S.CHAIN_CASES} == {True, False}


# ------------------------------------------------------------------------------------------------ head helpers
@pytest.mark.parametrize("T", S.CON_T)
@pytest.mark.parametrize("B", S.CON_B)
def test_contrastive_fp32_in_kernel_order_holds_a_quarter(B, T):
    for D in S.CON_D:
        x, g, l, cancel = S.con_inputs(B, D)
        assert not bool(((x.norm(dim=1) > 0) & (x.norm(dim=1) < 1e-6)).any())               # nothing near the clamp except the exact zero row
        ref, got = S.con_ref(x, g, l, T, cancel), S.con_kernel_order(x, g, l, T)
        for k in ("row_loss", "dx"):
            S.con_check(got[k], ref, k, "contrastive[%d,%d,%g] %s" % (B, D, T, k), frac=0.25)
        assert bool(torch.isfinite(ref["dx"].value).all())
        if B >= 3:
            assert abs(float(ref["row_loss"].value[2]) - float(np.log(2.0))) <= 2.0 ** -52     # g == l: log 2 to the last bit of float64
        if B >= 4:
            xd, gd, ld = x[3].double(), g[3].double(), l[3].double()
            assert float(xd.abs().max()) == 0
            w = 0.5 / T / B
            want = (-w / (S.CON_EPS * gd.norm())) * gd + (w / (S.CON_EPS * ld.norm())) * ld  # dx = kg g + kl l
            assert float((ref["dx"].value[:, 3] - want).abs().max()) <= 1e-12 * float(want.abs().max())
        if B >= 5 and D > 1 and T == 0.07:
            assert 0 < float(ref["row_loss"].value[4]) < 2.0 ** -25 and float(got["row_loss"][4]) == 0.0      # vanishes against 1 in fp32
            assert float(ref["dx"].value[:, 4].abs().max()) > 0


def test_contrastive_tables_and_mutants():
    assert {b % S.ROWS_PER_BLOCK for b in S.CON_B} == {0, 1, 3} and min(S.CON_B) < S.ROWS_PER_BLOCK < max(S.CON_B)
    assert {d % S.ROW_LANES for d in S.CON_D} >= {0, 1, 63} and min(S.CON_D) < S.ROW_LANES < max(S.CON_D) and max(S.CON_B) >= len(S.CON_SPECIAL)
    x, g, l, cancel = S.con_inputs(5, 96)
    ref = S.con_ref(x, g, l, 0.07, cancel)
    for m in ("row_ge", "lanes"):
        bad = S.con_kernel_order(x, g, l, 0.07, m)
        rejected(S.con_check, bad["row_loss"], ref, "row_loss")
        rejected(S.con_check, bad["dx"], ref, "dx")
    # the per-row denominator: an error of 1e-3 of ONE small row passes against the batch's largest gradient and fails against its own
    good = S.con_kernel_order(x, g, l, 0.07)
    big = ref["dx"].value.abs().amax(0)
    r = int(torch.where(cancel, torch.full_like(big, np.inf), big).argmin())              # (not a row whose reference is zero by construction)
    assert float(big[r]) * 100 < float(big.max())
    hurt = good["dx"].clone()
    hurt[r] *= 1.001
    S.con_check(good["dx"], ref, "dx")
    assert float((hurt.double() - ref["dx"].value.t()).abs().max() / big.max()) < S.TOL["grad"]
    rejected(S.con_check, hurt, ref, "dx")


def test_colflag_cases_are_exact_and_the_mutants_are_rejected():
    assert all(S.cf_admissible(K) for K in S.CF_K) and float(np.log2(S.CF_ALPHA)).is_integer()
    assert {k % 16 for k in S.CF_K} >= {0, 1, 15} and all(m % S.CF_TILE for m in S.CF_M) and {n % 64 for n in S.CF_N} >= {0, 1, 63}
    for M in S.CF_M:
        for N in S.CF_N:
            for K in (1, 17, 100):
                a, b = S.cf_operands(M, N, K)
                assert float(a.abs().max()) <= S.CF_AMAX and float(b.abs().max()) <= S.CF_BMAX and float(a.min()) >= 1
                s32 = (S.CF_ALPHA * (a @ b.t())).double()
                assert torch.equal(s32, S.cf_scores(a, b))                                  # exact at fp32, whatever the order
                thr = S.cf_thresholds(a, b)
                for name, t in thr.items():
                    want = S.cf_flags(a, b, t)
                    assert bool((S.cf_scores(a, b) == t).any())                             # attained
                    rejected(S.same_int, S.cf_flags(a, b, t, ge=True).numpy(), want.numpy())
                    if t < 0:                                                               # the padded zero rows exceed a negative threshold
                        assert not bool(want[0]) and bool(S.cf_flags(a, b, t, row_mask=False).all())
                        if not bool(want.all()):
                            rejected(S.same_int, S.cf_flags(a, b, t, row_mask=False).numpy(), want.numpy())
                assert not bool(S.cf_flags(a, b, thr["max"]).any())
                assert not bool(S.cf_flags(a, b, thr["neg_max"])[::3].all()) or N == 1


@pytest.mark.parametrize("B", S.CA_B)
def test_class_accumulate_order_holds_a_quarter_and_pairwise_is_rejected(B):
    for D in ((1, 64, 257) if B > 1024 else S.CA_D):
        for C in S.CA_C:
            x, sums, counts = S.ca_inputs(B, D, C)
            for lab in S.ca_labels(B, C):
                gs, gc = S.ca_order(x, lab, sums, counts)
                S.ca_check(gs, gc, x, lab, sums, counts, frac=0.25)
                ok = (lab >= 0) & (lab < C)
                assert np.array_equal(gc, counts + np.bincount(lab[ok], minlength=C).astype(f32))
                if B >= 7:
                    assert {-1, C, 10 ** 12} <= set(lab.tolist())
                if B >= 1024 and C <= 5:
                    ps, pc = S.ca_order(x, lab, sums, counts, "pairwise")
                    rejected(S.ca_check, ps, pc, x, lab, sums, counts)
                    S.ca_check(ps, pc, x, lab, sums, counts, order=False)                   # (a different order, not a wrong sum)
    assert any(b > S.CA_SLICE for b in S.CA_B) and S.CA_SLICE in S.CA_B and {d % 256 for d in S.CA_D} >= {0, 1, 255}
    absent = ~np.isin(np.arange(33), S.ca_labels(1025, 33)[0])
    assert absent.sum() >= 8


def test_roc_features_are_exact_and_sit_on_bin_edges():
    assert {d % 16 for d in S.ROC_D} >= {1, 15} and {1, 64, 65, S.ROC_N} == set(S.ROC_T) and S.ROC_N > 128
    clamped = [0, 0]
    for D in S.ROC_D:
        f, lab = S.roc_inputs(D)
        assert np.array_equal(f * 8, np.round(f * 8))
        s = f.astype(f64) @ f.astype(f64).T
        assert np.array_equal(s * 64, np.round(s * 64)) and np.abs(s).max() < 2 ** 10      # multiples of 1/64: exact in any order
        v = (s + 1.0) * 1000.0
        assert np.array_equal(v * 8, np.round(v * 8))                                      # (s + 1) * 1000 = k * 15.625 exactly
        iu = np.triu_indices(S.ROC_N, 1)
        assert int((v[iu] == np.round(v[iu])).sum()) > 50                                  # scores exactly on bin edges
        clamped[0] += int((s[iu] < -1).sum())
        clamped[1] += int((s[iu] > 1).sum())
        for T in S.ROC_T:
            h = S.roc_ref(f, lab, T)
            assert int(h.sum()) == T * (T - 1) // 2 + T * (S.ROC_N - T)
    assert min(clamped) > 0                                                                # both clamps are reached


# ------------------------------------------------------------------------------------------------ input path
def test_input_path_tables_and_mutants():
    for B, H, W in S.PRE_SHAPES + [S.PRE_WRAP]:
        u8 = S.pre_input(B, H, W)
        assert all(len(np.unique(u8[..., c])) == 256 for c in range(3))
    assert {W for _, _, W in S.PRE_SHAPES} == {1, 2, 111, 112}
    B, H, W = S.PRE_WRAP
    assert B * H * W > S.PRE_GRID_CAP * 256 and all(b * h * w <= S.PRE_GRID_CAP * 256 for b, h, w in S.PRE_SHAPES)
    u8 = S.pre_input(3, 5, 111)
    plain, mixed = S.pre_ref(u8, None), S.pre_ref(u8, S.pre_flip(3, "mixed"))
    assert torch.equal(plain, S.pre_ref(u8, S.pre_flip(3, "zeros"))) and torch.equal(plain.flip(3), S.pre_ref(u8, S.pre_flip(3, "ones")))
    assert torch.equal(mixed[0], plain[0]) and torch.equal(mixed[1], plain[1].flip(2)) and not torch.equal(mixed[1], plain[1])
    assert float(plain.min()) == -1.0 and float(plain.max()) == 1.0
    # a multiplication by 1 / 255 in place of the division is another fp32 number for some bytes
    alt = torch.from_numpy(u8).permute(0, 3, 1, 2).float().mul(1.0 / 255).sub(0.5).div(0.5)
    assert not torch.equal(alt, plain)
    Bw, Cw, HWw, Cpw = S.PAD_WRAP
    assert Bw * HWw * (Cpw // 8) > S.PAD_GRID_CAP * 256 and Bw * HWw * Cpw * 2 < 70e6
    assert {(3, 64), (1, 8), (8, 8), (3, 8), (64, 64), (5, 16)} == set(S.PAD_CC) and S.PAD_HW == [1, 7, 400]
    for s16 in S16:
        x = S.uniform((2, 3, 7), 9)
        x[0, 0] = torch.tensor([1 + 2.0 ** -11, 1 + 2.0 ** -8, 65520.0, 2.0 ** -25, -0.0, 1.0, 0.5])
        good = S.pad_ref(x, 8, s16)
        assert bool((good[:, :, 3:].view(torch.int16) == 0).all())
        rejected(S.tc.same16, S.pad_ref(x, 8, s16, "copy0"), good)
        S.tc.same16(S.pad_ref(x[:, :, :], 8, s16)[:, :, :3], x.permute(0, 2, 1).contiguous().to(s16))
