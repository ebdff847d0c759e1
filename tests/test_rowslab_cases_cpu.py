"""CPU checks of tests/rowslab_cases.py, the references of test_rowslab_fwd_gpu.py.  (1) Precision: the float32 evaluation of every reference
formula in the kernels' order of operations, taken before the final store, stays within a QUARTER of the tolerance the kernels get against
float64.  (Two exceptions, both stated where they apply: a column sum whose whole chain is 11 additions gets a half, _frac; and the eval-mode coefficients: their tolerance is k fp32 roundings with k = 3 ... 6 counted off the
expression, the fp32 evaluation makes those very roundings and is held to the whole tolerance.)  (2) Admissibility of the exact tier at the real
shapes.  (3) The tables against the restated geometry: every shape reaches the branch it is listed for.  (4) Sensitivity: each listed corruption
of the operation moves the float64 reference beyond the tolerance."""
import pytest
import torch

import rowslab_cases as K

f32, f64 = K.f32, K.f64
S16 = [torch.float16, torch.bfloat16]
IDS = ["fp16", "bf16"]


def _frac(chain):
    """share of a column sum's tolerance the fp32 evaluation in the workgroup's own order may use: a quarter — a half where the chain is so short
    (C = 2048: 8 rows of one thread + 1 + 2 = 11) that the roundings the evaluation really makes, 8 of the 11 counted, cannot average out"""
    return 0.25 if chain >= 16 else 0.5


def _stored(v, s16):
    return K.r16(v.to(f32), s16)


# ------------------------------------------------------------------------------------------------ tables and geometry
def test_row_slab_tables_reach_their_branches():
    want = {8: (1, 256, 0), 24: (3, 85, 1), 64: (8, 32, 0), 96: (12, 21, 4), 512: (64, 4, 0), 2048: (256, 1, 0)}
    for table, blocks in ((K.apply_table(), K.APPLY_BLOCKS), (K.prelu_table(), K.PRELU_BLOCKS)):
        seen = {}
        for row in table:
            C, kind, M = row[:3]
            g = K.geometry(M, C, blocks)
            assert (g["tpr"], g["rpp"], g["idle"]) == want[C]
            rpp = g["rpp"]
            seen.setdefault(C, set()).add(kind)
            if kind == "slab_grows":
                assert C == 512 and g["slab"] == 36 > 8 * rpp and M == blocks * 32 + 1 and g["grid"] > 1 and M * C < 17.5e6
                continue
            assert g["slab"] == 8 * rpp
            if kind == "lt_rpp":
                assert (M < rpp or rpp == 1) and g["grid"] == 1 and K.trips(M, rpp) == (0, 1)
            elif kind == "rem_only":
                assert M == 3 * rpp - 1 and K.trips(M, rpp) == (0, 3 if rpp > 1 else 2)
            elif kind == "two_trips":
                assert M == 8 * rpp and g["grid"] == 1 and K.trips(M, rpp) == (2, 0)
            elif kind == "slab_plus1":
                assert g["grid"] == 2 and g["last"] == 1
            else:
                n = int(kind[4:])
                assert g["grid"] == n and n & 7 and 0 < g["last"] < g["slab"] and (rpp == 1 or g["last"] % rpp)
                assert K.trips(g["last"], rpp)[0] >= 1 and K.trips(g["last"], rpp)[1] >= 1
                assert sorted(K.xcd_remap(i, n) for i in range(n)) == list(range(n))            # the remainder path of xcd_remap is a bijection
                assert [K.xcd_remap(i, n) for i in range(n)] != list(range(n)) or n < 8
        assert all(seen[C] >= set(K.m_kinds(C)) for C in K.CHANNELS) and "slab_grows" in seen[512]
    ap = K.apply_table()
    for C in K.CHANNELS:
        rows = [r for r in ap if r[0] == C]
        assert {("x2" in K.VARIANTS[r[3]], r[4]) for r in rows} == {(a, b) for a in (False, True) for b in (False, True)}      # all four <X2, STATS>
        assert {r[3] for r in rows} == set(K.VARIANTS)
    for v in K.VARIANTS:
        assert {r[1] for r in ap if r[3] == v} >= set(K.m_kinds(64))
    for n in ("sc1", "sh1", "alpha", "sc2", "sh2"):
        assert any(n in ops for ops in K.VARIANTS.values()) and any(n not in ops and ("x2" in ops or n in ("sc1", "sh1", "alpha")) for ops in K.VARIANTS.values())
    for C in K.CHANNELS:
        assert {(r[3], r[4]) for r in K.prelu_table() if r[0] == C} == {(a, b) for a in (False, True) for b in (False, True)}
    for C, hw, B, v, stats in K.nchw_table():
        g = K.geometry(B * hw, C, K.APPLY_BLOCKS)
        assert g["grid"] >= 3 and (hw == 1 or g["slab"] % hw) and B >= 3
    assert {(r[0], r[1]) for r in K.nchw_table()} == {(C, hw) for C in (96, 512) for hw in (1, 5, 49)}
    for M, C in K.APPLY_ERRORS:
        assert M <= 0 or C % 8 or C // 8 > K.EW_THREADS
    for C, M, bias in K.LEGACY_TABLE:
        assert K.geometry(M, C, K.PRELU_BLOCKS)["grid"] >= 3


def test_finalize_tables_and_who_hands_over_more_than_1024_rows():
    """The finalize table straddles fin8_accumulate's 128 row groups (two rows per trip) and reaches colsum_stage_kernel's second and ragged third
    trip.  Which producers hand a finalize more than 1024 rows at the bench batch (128 x 112 x 112): only those whose row count grows with M — the
    stem conv's statistics rows; bn_apply / prelu_bwd_pass rows are capped by max_blocks."""
    P = K.FIN_P
    assert {K.FIN_RG - 1, K.FIN_RG, K.FIN_RG + 1, 2 * K.FIN_RG - 1, 2 * K.FIN_RG, 2 * K.FIN_RG + 1, 1024} <= set(P)
    trips = lambda p: -(-p // (K.STAGE_S * 32))     # noqa: E731   `row += S * 32` from row = slice + S rg: rows per trip of one workgroup
    assert [trips(p) for p in P if p > 1024] == [1, 1, 2, 3] and 4097 % (K.STAGE_S * 32) == 1
    assert 2 * 8 < 32 and -(-2 * 24 // 32) == 2 and 2 * 24 % 32 == 16          # W = 16 < 32; a half-empty second column block
    seen = {(p, c) for p, c, _, _ in K.finalize_table()}
    assert seen >= {(p, c) for p in P for c in K.FIN_C}
    assert {n for r in K.finalize_table() for n in r[3]} == {"gamma", "beta", "running"} and {r[2] for r in K.finalize_table()} == {"M", "one", "large"}
    assert K.stem_stat_rows(128, 112, 112) == 25088 > 1024
    for hw, C in ((112, 64), (56, 64), (56, 128), (28, 128), (28, 256), (14, 256), (14, 512), (7, 512)):
        M = 128 * hw * hw
        assert K.geometry(M, C, K.APPLY_BLOCKS)["grid"] <= 1024 and K.geometry(M, C, K.PRELU_BLOCKS)["grid"] <= 512
    print("rows handed to bn_finalize at batch 128: stem", K.stem_stat_rows(128, 112, 112), "| bn_apply <= 1024 | prelu_bwd_pass <= 512")
    for name, ent in K.multi_tables().items():
        lay = K.MultiLayout(ent)
        blk0, blocks = lay.blocks()
        assert 1 <= len(ent) <= K.MAX_PRELU_FIN and blocks == sum(e[1] // 8 for e in ent) and all(o % 16 == 0 for o in lay.rows_off)
    big = K.multi_tables()["n64"]
    assert len(big) == K.MAX_PRELU_FIN and len({e[1] for e in big}) >= 4 and len({e[0] for e in big}) >= 6
    assert any(e[2] == 3 for e in big) and any(not e[3] for e in big) and any(e[1] == 8 for e in big)     # C = 8: the first workgroup of an entry is its last
    assert K.EvalCase(K.MAX_BN_EVAL).n == K.MAX_BN_EVAL and set(K.EvalCase(K.MAX_BN_EVAL).C) == set(K.EVAL_C)
    assert 264 > 256 and 520 > 2 * 256


# ------------------------------------------------------------------------------------------------ 1. bn_apply
def _apply_rows(C):
    return [r for r in K.apply_table() if r[0] == C and r[1] != "slab_grows"]


@pytest.mark.parametrize("C", K.CHANNELS + ("grows", "nchw"))
def test_apply_exact_tier_is_admissible(C):
    """Every intermediate is a multiple of 2^-7 below 2^10 (exact in fp32 in any order, fused or not), y equals its own rounding in BOTH storage
    types, and per statistics row and channel all terms are multiples of one quantum q (q^2 for the squares) with sum |terms| < 2^24 quanta:
    every partial sum is then representable and the fp32 sums are exact whatever their order."""
    if C == "grows":
        rows = [r for r in K.apply_table() if r[1] == "slab_grows"]
    elif C == "nchw":
        rows = [(c, "nchw", B * hw, v, st) for c, hw, B, v, st in K.nchw_table()]
    else:
        rows = _apply_rows(C)
    for Cc, kind, M, v, stats in rows:
        c = K.ApplyCase(Cc, M, v, stats, torch.float16, True)
        assert torch.equal(c.x.to(torch.bfloat16).to(f64), c.x.to(f64)) and float(c.x.abs().max()) <= 2.0
        z, a, w = c.parts(f64)
        for t in (z, a) + (() if w is None else (w,)):
            assert bool(((t * 128) == (t * 128).round()).all()) and float(t.abs().max()) < 2 ** 10
        y = c.y()[0]
        for s16 in S16:
            assert torch.equal(_stored(y, s16).to(f64), y), c.name
        assert torch.equal(c.y(f32)[0].to(f64), y)
        if "alpha" in c.has and "sh1" in c.has and M > 40:
            assert bool((z[:, K.TIE::8] == 0).any())                                    # exact ties
        ay = y.abs()
        q = torch.full((Cc,), 2.0 ** -7, dtype=f64)                                     # per channel: the largest power of two dividing every y
        for e in range(-6, 4):
            ok = ((y / 2.0 ** e) == (y / 2.0 ** e).round()).all(0)
            q = torch.where(ok, torch.full_like(q, 2.0 ** e), q)
        assert bool(((y / q) == (y / q).round()).all()), c.name
        g = c.g
        assert float((K.slab_sums(ay, g["slab"], g["grid"]) / q).max()) < 2 ** 24, c.name
        assert float((K.slab_sums(y * y, g["slab"], g["grid"]) / (q * q)).max()) < 2 ** 24, c.name


@pytest.mark.parametrize("s16", S16, ids=IDS)
@pytest.mark.parametrize("C", K.CHANNELS)
def test_apply_tolerance_tier(C, s16):
    for Cc, kind, M, v, stats in _apply_rows(C) + ([(c, "nchw", B * hw, vv, st) for c, hw, B, vv, st in K.nchw_table() if c == C]):
        c = K.ApplyCase(Cc, M, v, stats, s16, False)
        z = c.z()
        assert bool(((z == 0) | (z.abs() >= K.ZMIN)).all()), c.name
        assert torch.equal(c.z(f32) > 0, z > 0), c.name                               # the mask is the same in every precision
        q = c.y_q()
        assert bool(((q.value == 0) | (q.value.abs() >= K.YMIN)).all()), c.name
        if c.op["alpha"] is not None:
            assert float(c.op["alpha"].abs().max()) <= 1.0                            # K_APPLY counts the slope's product on the bound of z
            assert bool((z[:, K.TIE] == 0).any()) or M < 1
        K.check(c.y(f32)[0], q, c.name + " y fp32", 0.25)
        if v == "ident":
            assert torch.equal(_stored(q.value, s16), c.x)
        if c.op["alpha"] is not None:
            flat = int((z.abs() * (c.eff("sc1", f64) != 0)).argmax())
            flip = (flat // Cc, flat % Cc)
            assert K.exceeds(c.y(f64, flip=flip)[0], q), c.name + ": a flipped PReLU mask"
            if M * Cc >= 64:
                assert K.exceeds(c.y(f64, neighbour_slope=True)[0], q), c.name + ": the neighbouring channel's slope"
                assert K.exceeds(c.y(f64, bias_after=True)[0], q), c.name + ": the shift added behind the mask"
        y16 = _stored(q.value, s16)
        sq = c.stats_q(y16)
        K.check(c.stats_q(y16, f32).value, sq, c.name + " stats fp32", _frac(c.chain))
        assert K.exceeds(c.stats_q(y16, f64, drop=M // 2).value, sq), c.name + ": a row dropped from a statistics column"
        assert K.exceeds(c.stats_q(y16, f64, drop=M - 1).value, sq), c.name + ": the last pixel of the last slab omitted"
        if c.g["grid"] > 1:
            assert K.exceeds(c.stats_q(y16, f64, gid=K.gid_neighbour(M, c.g["slab"])).value, sq), c.name + ": a pixel counted in the neighbouring slab's row"
        if Cc >= 96 and M >= 8 and v != "ident":
            assert K.exceeds(c.stats_q(q.value).value, sq), c.name + ": a statistics row summed from the unrounded y"
    if C == 96:
        y = K.uniform((7 * 49, 96), 5)
        assert not torch.equal(K.nchw(y, 49, swap=11), K.nchw(y, 49)) and torch.equal(K.nchw(y, 49)[2, 5], y[2 * 49:3 * 49, 5])


# ------------------------------------------------------------------------------------------------ 2. bn_finalize
@pytest.mark.parametrize("C", K.FIN_C)
def test_finalize_reference(C):
    shown = []
    for P, Cc, kind, null in [r for r in K.finalize_table() if r[1] == C]:
        c = K.FinalizeCase(P, Cc, kind, null)
        live = [j for j in range(Cc) if j != K.CONST]
        srt = c.rows[:, :, live].sort(0).values
        assert P == 1 or bool((srt[1:] != srt[:-1]).all()), c.name + ": rows pairwise different"
        assert float(((c.rows.to(f64) - c.rows64).abs() / c.rows64.abs().clamp_min(1e-30)).max()) <= 16 * K.U24 and c.rows.shape == (P, 2, Cc)
        q = c.outputs()
        share = dict(c.stage_over_store)
        kq = c.outputs("kernel")
        for n in q:
            K.check(kq[n].value, q[n], c.name + " " + n + " kernel order", 0.25)
        x0 = q["rstd"].value
        if c.count == c.M:
            assert abs(float(x0[K.CONST]) * K.EPS32 ** 0.5 - 1.0) < 1e-6              # variance clamped at 0: rstd = 1 / sqrt(eps)
        if c.count == c.M and P >= 127:
            mean, rstd = q["mean"].value, q["rstd"].value
            assert 30.0 < abs(float(mean[K.FAR] * rstd[K.FAR])) < 34.0 + 40.0 / P ** 0.5
        if "running" not in c.null and kind == "M" and P > 1:
            assert K.exceeds(c.outputs(biased=True)["rv"].value, q["rv"]), c.name + ": the biased variance in the running update"
        if P > 1:
            bad = c.outputs(drop_row=P // 2)
            assert any(K.exceeds(bad[n].value, q[n]) for n in q), c.name + ": a row dropped"
        if c.staged:
            bad = c.outputs(drop_slice=K.STAGE_S - 1)
            assert all(K.exceeds(bad[n].value, q[n]) for n in ("mean", "rstd", "scale") if not (n == "scale" and "gamma" not in c.null and Cc <= K.ZERO)), c.name
            if c.count == c.M:
                assert share["rstd"] > 100.0, share        # the staged slices' fp32 rounding dominates the 32 sigma channel's tolerance
                shown.append((P, Cc, round(share["rstd"]), round(share["scale"])))
    print("tolerance of (rstd, scale) on the 32 sigma channel in units of its fp32 store, P > 1024:", shown)
    r = K.exact_fin_rows(257, C).to(f64)
    assert torch.equal(r.cumsum(0), r.cumsum(0).round()) and float(r.abs().sum(0).max()) < 2 ** 53


# ------------------------------------------------------------------------------------------------ 3. prelu_bwd_pass
@pytest.mark.parametrize("s16", S16, ids=IDS)
@pytest.mark.parametrize("C", K.CHANNELS)
def test_prelu_pass_reference(C, s16):
    rows = [r for r in K.prelu_table() if r[0] == C and r[1] != "slab_grows"] + [(c, "legacy", M, False, b) for c, M, b in K.LEGACY_TABLE if c == C]
    for Cc, kind, M, add, bias in rows:
        c = K.PreluCase(Cc, M, add, bias, s16)
        g16 = c.gsum()
        x = c.x.to(f64)
        z = x if c.bias is None else x + c.bias.to(f64)
        z32 = c.x.to(f32) if c.bias is None else c.x.to(f32) + c.bias
        assert bool((z[c.keep] == 0).all()) and bool(c.keep.any()) and float(z[~c.keep].abs().min()) >= K.ZMIN, c.name
        assert torch.equal(z32 <= 0, z <= 0), c.name
        q = c.dz_q(g16)
        assert bool(((q.value == 0) | (q.value.abs() >= K.RMIN)).all()), c.name
        K.check(c.dz_q(g16, f32).value, q, c.name + " dz fp32", 0.25)
        rq = c.rows_q(g16)
        K.check(c.rows_q(g16, f32).value, rq, c.name + " rows fp32", _frac(c.chain))
        mid = (M // 2, 9 % Cc)
        flat = int((g16.to(f64).abs() * (~c.keep)).argmax())
        flip = (flat // Cc, flat % Cc)
        assert K.exceeds(c.dz_q(g16, flip=flip).value, q) and K.exceeds(c.rows_q(g16, flip=flip).value, rq), c.name + ": a flipped mask"
        assert K.exceeds(c.dz_q(g16, tie_positive=True).value, q), c.name + ": the tie z == 0 taken as positive"
        assert K.exceeds(c.rows_q(g16, dalpha_positive=True).value, rq), c.name + ": dalpha summed over z > 0"
        if M * Cc >= 64:
            assert K.exceeds(c.dz_q(g16, neighbour_slope=True).value, q), c.name + ": the neighbouring channel's slope"
            if bias:
                assert K.exceeds(c.dz_q(g16, bias_after=True).value, q), c.name + ": bias added after the mask"
        assert K.exceeds(c.rows_q(g16, drop=mid[0]).value, rq) and K.exceeds(c.rows_q(g16, drop=M - 1).value, rq), c.name + ": a row dropped / the last pixel omitted"
        if c.g["grid"] > 1:
            assert K.exceeds(c.rows_q(g16, gid=K.gid_neighbour(M, c.g["slab"])).value, rq), c.name + ": a pixel counted in the neighbouring slab's row"
        if add:                                         # the ADD pass IS the plain pass on its own gsum: one formula, one stored g
            assert torch.equal(g16, (c.dy.float() + c.add.float()).to(s16))


# ------------------------------------------------------------------------------------------------ 4. prelu_bwd_finalize
def test_prelu_finalize_reference():
    for P in K.PFIN_P:
        for C in K.PFIN_C:
            rows = K.prelu_rows(P, C)
            q = K.prelu_fin_q(rows)
            k = K.prelu_fin_q(rows.flip(0))
            for i in range(2):
                K.check(k[i].value, q[i], "prelu_finalize[P=%d,C=%d] reversed" % (P, C), 0.25)
            if P > 1:
                bad = rows.clone()
                bad[P // 2] = 0
                assert all(K.exceeds(K.prelu_fin_q(bad)[i].value, q[i]) for i in range(2))
    r3 = K.prelu_rows(5, 8, 3)
    assert bool(torch.isnan(r3[:, 2]).all()) and bool(torch.isfinite(K.prelu_fin_q(r3)[0].value).all())


# ------------------------------------------------------------------------------------------------ 5. bn_eval_coeffs
@pytest.mark.parametrize("n", [1, K.MAX_BN_EVAL])
def test_eval_coeffs_reference(n):
    c = K.EvalCase(n)
    assert any(g < 0 for g in c.g_off) or n == 1
    for i in range(n):
        q, k = c.entry(i), c.entry(i, f32)
        for name in q:
            K.check(k[name].value, q[name], "%s entry %d %s fp32" % (c.name, i, name), 1.0)
        rv = c.bufs[c.rv_off[i]: c.rv_off[i] + c.C[i]]
        assert float(rv.min()) <= 1.0001e-6 and float(rv.max()) >= 999.0
