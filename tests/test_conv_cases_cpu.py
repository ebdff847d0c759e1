"""CPU checks of tests/conv_cases.py, the references of test_conv_branches_gpu.py.  (1) conv_ref in float64 IS F.conv2d and its autograd
(stride 2, 1x1, B > 1).  (2) The table's literal profile slots and row counts are what the restated dispatch rules give, and the batch sizes sit on
the thresholds they claim.  (3) Every exact case of the table is admissible (conditions a, b, c of conv_cases.py) at its REAL shape, on the tensors
the GPU test builds, and its epilogue is exact in fp32 in both orders of the affine, with and without fma.  (4) Tolerance tier: the float32
evaluation in plausible kernel orders (per tap, 64-channel chunks, split-K slabs added last, one partial row per tile, the kernels' algebraic form
of the BatchNorm-backward rows) stays within a quarter of EVERY tolerance formula.  (5) Mutants: each corruption of the reference differs from it in
at least one bit in the exact tier, and those that move a conv output also exceed the tolerance tier's bound; a 16-bit store that truncates
exceeds it too, and so does an eval epilogue that rounds affine + identity once instead of twice.  (6) The library's own kernel selector
(gemm.hip: gemm_nt_plan, asked through the host-only fedfr_conv2d_plan) agrees with the restated rules on the table and on a sweep across every threshold."""
import contextlib
import ctypes
import itertools

import pytest
import torch
import torch.nn.functional as F

import conv_cases as K

f32, f64 = K.f32, K.f64
S16 = [torch.float16, torch.bfloat16]
IDS = ["fp16", "bf16"]
TABLE = K.table(256)


# ------------------------------------------------------------------------------------------------ 1. the reference
@pytest.mark.parametrize("B,H,Cin,Cout,k,s", [(2, 6, 8, 16, 3, 1), (3, 8, 16, 8, 3, 2), (2, 6, 8, 8, 1, 1), (2, 8, 8, 24, 1, 2), (1, 5, 4, 4, 3, 1)])
def test_conv_ref_is_conv2d(B, H, Cin, Cout, k, s):
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, H, H, Cin, generator=g, dtype=f64)
    w = torch.randn(Cout, k, k, Cin, generator=g, dtype=f64)
    dy = torch.randn(B, H // s if H % s == 0 else (H + 1) // s, H // s if H % s == 0 else (H + 1) // s, Cout, generator=g, dtype=f64)
    xn, wn = x.permute(0, 3, 1, 2).clone().requires_grad_(True), w.permute(0, 3, 1, 2).clone().requires_grad_(True)
    y = F.conv2d(xn, wn, None, s, 1 if k == 3 else 0)
    assert y.shape[2] == dy.shape[1]
    y.backward(dy.permute(0, 3, 1, 2))
    r = K.conv_ref(x, w, s, f64, "cpu", dy=dy, want=("y", "dx", "dw"))
    for got, ref in ((r["y"], y.detach().permute(0, 2, 3, 1)), (r["dx"], xn.grad.permute(0, 2, 3, 1)), (r["dw"], wn.grad.permute(0, 2, 3, 1))):
        assert float((got - ref).abs().max()) <= 1e-12 * (1 + float(ref.abs().max()))
    # S is the same sum over |terms|
    ra = K.conv_ref(x.abs(), w.abs(), s, f64, "cpu", dy=dy.abs(), want=("y", "dx", "dw"))
    for n in ("y", "dx", "dw"):
        assert float((r["S" + n] - ra[n]).abs().max()) <= 1e-12 * (1 + float(ra[n].abs().max()))
    # the float32 orders compute the same thing
    r32 = K.conv_ref(x.float(), w.float(), s, f32, "cpu", dy=dy.float(), want=("y", "dx", "dw"), chunk=4, slabs=2)
    for n in ("y", "dx", "dw"):
        assert float((r32[n].double() - r[n]).abs().max()) <= 1e-4 * (1 + float(r[n].abs().max()))


# ------------------------------------------------------------------------------------------------ 2. geometry
def test_table_slots_follow_the_dispatch_rules():
    assert len({r.id for r in TABLE}) == len(TABLE) >= 90
    for r in TABLE:
        assert K.expected_slot(r) == r.slot, r.id
    assert {r.slot for r in TABLE} >= {0, 1, 2, 3, 4, 5, 6, 7, 12, 13, 14, 15, 16, 17}
    for r in TABLE:                                   # ... and so do the literal statistics / partial row counts (gemm_nt_plan, launch_glds, launch_c64p)
        assert K.expected_rows(r) == r.rows, (r.id, r.rows, K.expected_rows(r))


def test_batches_sit_on_the_thresholds():
    bm = K.nt_bm
    assert (bm(124 * 196, 256), bm(125 * 196, 256)) == (64, 128)            # 14x14, two output tiles
    assert (bm(250 * 196, 128), bm(251 * 196, 128)) == (64, 128)            # 14x14, one output tile: ceil(49 000 / 128) = 383
    assert (bm(62 * 784, 128), bm(63 * 784, 128)) == (64, 128)              # 28x28
    assert (bm(15 * 3136, 64), bm(16 * 3136, 64), bm(15 * 3136, 128), bm(16 * 3136, 128)) == (64, 128, 64, 128)
    assert (bm(3 * 12544, 64), bm(4 * 12544, 64)) == (64, 128)              # 112x112
    assert (bm(63 * 784, 128), bm(16 * 3136, 64)) == (128, 128)             # the 1x1 rows of slots 0 and 1
    assert K.c64p_batches(56, 256) == (1, 19, 37) and K.c64p_batches(112, 256) == (1, 5, 10)
    for W, (b0, b1, b2) in ((56, K.c64p_batches(56, 256)), (112, K.c64p_batches(112, 256))):
        t = W * W // 224
        assert b1 * t > 256 >= (b1 - 1) * t and K.conv_c64p_grid(b1 * W * W, 256) < b1 * t
        per = K.cdiv(b2 * t, 256)
        assert (b2 * t) % per != 0 and K.conv_c64p_grid(b2 * W * W, 256) == K.cdiv(b2 * t, per)      # a short last workgroup
    assert K.conv_c64p_grid(3136, 256) == 14                                # one tile per workgroup
    assert (4 * 63) % 2 == 0 and K.fused_rows(63 * 784, 28) == 126 and K.fused_rows(63 * 784, 28, 1) == 252
    # gemm_nt_glds: 64-row shapes taken up to 128-row tiles only where the statistics rows agree
    assert not K.nt_glds_up(147, True) and K.nt_glds_up(147, False) and K.nt_glds_up(196, True) and K.nt_glds_up(80, True) and K.nt_glds_up(588, True)
    assert K.nt_glds_applies(512, 4608) and not K.nt_glds_applies(128, 576) and not K.nt_glds_applies(512, 4608, par=True) and not K.nt_glds_applies(64, 4608)
    # nine-tap kernel: one stage -> one split; 5 stages on 2 splits (3 + 2); every width
    assert K.wgrad9_pick_splits(196, 256, 2304, 14) == 1 and K.wgrad9_pick_splits(5 * 196, 128, 1152, 14) == 2 and K.w9_stages(5 * 196, 14) == 5
    assert [K.w9_stages(W * W, W) for W in (14, 28, 56, 112)] == [1, 4, 16, 64]
    assert K.wgrad_slot_splits(3, 14, 64, 192, 3, 1)[0] == 16 and 192 % 64 == 0 and (192 // 32) % 2 == 0 and (64 // 32) % 2 == 0


# ------------------------------------------------------------------------------------------------ 3. admissibility of the exact tier
def _exact_fp32_affine(x, sc, sh, mean, rstd, gamma, beta):
    """z in fp32 as x sc + sh and as (x - mean) rstd gamma + beta, with and without fma, equals float64"""
    zd = x.to(f64) * sc.to(f64) + sh.to(f64)
    forms = [x * sc + sh, (x.to(f64) * sc.to(f64) + sh.to(f64)).to(f32)]
    if mean is not None:
        forms += [(x - mean) * rstd * gamma + beta, (((x - mean) * rstd).to(f64) * gamma.to(f64) + beta.to(f64)).to(f32)]
        assert torch.equal(((x.to(f64) - mean.to(f64)) * rstd.to(f64) * gamma.to(f64) + beta.to(f64)), zd)
    return all(torch.equal(f.to(f64), zd) for f in forms)


def _exact_rows():
    seen, outl = set(), []
    for r in TABLE:
        for tier in r.tiers:
            key = (r.op, r.shape, tier, r.prelu)
            if tier != "tol" and key not in seen:
                seen.add(key)
                outl.append((r, tier))
    return sorted(outl, key=lambda t: (t[0].shape, t[1]))      # rows of one geometry together: their reference is computed once


@pytest.mark.parametrize("s16", S16, ids=IDS)
def test_exact_cases_are_admissible(s16):
    """every exact case of the table at its REAL shape, on the very tensors the GPU test builds: no image, element or column left out"""
    last_key, r = None, None
    for row, tier in _exact_rows():
        c = K.ConvCase(*row.shape, tier, s16)
        kind = "dw" if row.op.startswith("wgrad") else ("y" if row.op.startswith("fwd") else "dx")
        key = (kind, row.shape, tier)
        if key != last_key:
            if kind == "y":
                x, w = c.fwd()
                r = K.conv_ref(x, w, c.s, f64, "cpu", want=("y",))
            elif kind == "dx":
                dy, w = c.bwd()
                r = K.conv_ref(torch.zeros(c.B, c.H, c.H, c.Cin), w, c.s, f64, "cpu", dy=dy, want=("dx",))
            else:
                r = {}
                for seed in (0, 100) if row.op == "wgrad_pair" else (0,):
                    x, dy = c.wg(seed)
                    r[seed] = K.conv_ref(x, torch.zeros(c.Cout, c.k, c.k, c.Cin), c.s, f64, "cpu", dy=dy, want=("dw",))
            last_key = key
        q = c.quantum(kind)
        if kind == "dw":        # fp32 result: conditions (a) and "a whole number of quanta"
            for g in r.values():
                assert K.admissible_out(g["dw"], g["Sdw"], q), row.id
                assert float(g["dw"].abs().max()) > 0
            continue
        ref, S = r[kind].reshape(-1, r[kind].shape[-1]), r["S" + kind].reshape(-1, r[kind].shape[-1])
        assert K.admissible_out(ref, S, q, s16), (row.id, tier, float(ref.abs().max()) / q)          # (a) and (b), every element
        zeros = float((ref == 0).double().mean())
        assert zeros < 0.9 and (zeros > 0.01 or tier == "multi"), (row.id, tier, zeros)               # sparse tiers: exact zeros and non-zeros both occur
        M, C = ref.shape
        if row.op == "fwd_stats" or (row.op == "fwd" and row.rows is not None):       # (c): whole columns over all M rows
            _, mag = K.stats_of(ref)
            assert K.admissible_col(mag, q * q), row.id
        elif row.op == "fwd_moments":
            other = K.moments_other(M, C, True, s16)
            assert K.is_representable(other, s16)
            _, mag = K.moments(ref, other)
            assert K.admissible_col(mag, q * min(q, 0.5)), row.id
        elif row.op == "dgrad_bnbwd":
            par = K.BnPar(C, True, 60)
            assert float(par.gamma.min()) < 0 and bool((par.gamma == 0).any())
            bx, keep = K.bn_input(M, C, par, True, s16, 61)
            assert K.is_representable(bx, s16)
            assert _exact_fp32_affine(bx, par.sc, par.sh, par.mean, par.rstd, par.gamma, par.beta), row.id
            z = bx.to(f64) * par.sc.to(f64) + par.sh.to(f64)
            assert bool(keep.any()) and bool((z[keep] == 0).all())                                    # the ties: z == 0, masked
            assert bool(((bx == 0) & (par.sh == 0) & (par.sc > 0)).any())                             # ... and x == +0 on a zero threshold
            val, mag = K.bnbwd_rows(ref, bx, par, row.prelu)
            # quanta per row: dz in q / 4 (alpha = 1/4); (dz x - mean dz) rstd in q / 4 / 2 / 2; sc dx x + sh dx in q / 8 (sc down to 1/4 on x in halves, sh in eighths)
            for i, qq in enumerate((q / 4, q / 16, q / 8)):
                assert K.admissible_col(mag[i], qq), (row.id, i, float(mag[i].max()) / qq)
            v32, _ = K.bnbwd_rows(ref.to(f32), bx, par, row.prelu, f32)
            assert torch.equal(v32.to(f64), val), row.id                                              # and in fp32 on these rows
        elif row.op == "dgrad_papply":
            for with_bias in (True, False):
                ax, bias, alpha = K.papply_operands(M, C, True, s16, with_bias)
                dz, val, mag = K.papply_ref(ref, ax, bias, alpha)
                assert K.is_representable(ax, s16) and K.is_representable(dz, s16) and K.admissible_col(mag, q / 4 / 2), row.id
                zf = ax if bias is None else ax + bias
                assert torch.equal(zf.to(f64), ax.to(f64) + (0 if bias is None else bias.to(f64))) and bool((zf[::7, K.TIE::16] == 0).all())
        elif row.op == "fwd_epi":
            ep = K.EpiPar(C, True, s16, 50)
            add = K.epi_add(M, C, ep, True, s16)
            assert K.is_representable(add, s16)
            assert _exact_fp32_affine(ref.to(f32), ep.scale, ep.shift, None, None, None, None), row.id
            for alpha in (False, True):
                y0, ya, _ = K.epilogue_ref(ref, S, ep, alpha, add)
                for y in (y0, ya):
                    assert K.is_representable(y, s16), (row.id, alpha)
                    y2 = y * ep.scale2.to(f64) + ep.shift2.to(f64)
                    assert K.is_representable(y2, s16), (row.id, alpha)
                    assert torch.equal((y.to(f32) * ep.scale2 + ep.shift2).to(f64), y2)


# ------------------------------------------------------------------------------------------------ 4. tolerance tier: reachable by a correct fp32 kernel
def _tiles32(t, C, tile=196):
    """fp32 sums over tiles of 196 pixels (one partial row each), as [tiles][C]"""
    return t.to(f32).reshape(-1, tile, C).sum(1)


def _rows64(*parts):
    return torch.stack([p.to(f64).sum(0) for p in parts])


@pytest.mark.parametrize("s16", S16, ids=IDS)
def test_tolerances_hold_for_fp32_in_kernel_orders(s16):
    """every tolerance formula of conv_cases.py against the float32 evaluation in kernel order, at a quarter.  The bounds are element-wise formulas,
    so each geometry of the table is taken with two images (one on the 56x56 / 112x112 maps)."""
    shapes = sorted({r.shape[1:] for r in TABLE if "tol" in r.tiers})
    for H, Cin, Cout, k, s in shapes:
        c = K.ConvCase(2 if H <= 28 else 1, H, Cin, Cout, k, s, "tol", s16)
        x, w = c.fwd()
        dy, wb = c.bwd()
        xg, dyg = c.wg()
        r64 = K.conv_ref(x, w, s, f64, "cpu", want=("y",))
        b64 = K.conv_ref(x, wb, s, f64, "cpu", dy=dy, want=("dx",))
        g64 = K.conv_ref(xg, w, s, f64, "cpu", dy=dyg, want=("dw",))
        if s16 == torch.float16:
            assert float(r64["y"].abs().max()) < 6e4 and float(b64["dx"].abs().max()) < 6e4, c.name
        Ky = k * k * Cin
        qy = c.out16_q(r64["y"], r64["Sy"], Ky)
        qx = c.out16_q(b64["dx"], b64["Sdx"], k * k * Cout)
        qw = c.dw_q(g64["dw"], g64["Sdw"], 2)
        for chunk, slabs in ((0, 1), (64, 2)):
            y32 = K.conv_ref(x, w, s, f32, "cpu", want=("y",), chunk=chunk)["y"]
            K.check(y32, qy, c.name + " y fp32", 0.25)
            K.check(K.conv_ref(x, wb, s, f32, "cpu", dy=dy, want=("dx",), chunk=chunk)["dx"], qx, c.name + " dx fp32", 0.25)
            K.check(K.conv_ref(xg, w, s, f32, "cpu", dy=dyg, want=("dw",), slabs=slabs)["dw"], qw, c.name + " dw fp32", 0.25)
        # a store that truncates instead of rounding to nearest-even exceeds the bound (the coherent channels see it)
        assert K.exceeds(K.trunc16(r64["y"], s16), qy) and K.exceeds(K.trunc16(b64["dx"], s16), qx), c.name
        assert not K.exceeds(K.r16(r64["y"].to(f32), s16), qy) and not K.exceeds(K.r16(b64["dx"].to(f32), s16), qx), c.name
        # statistics rows of the stored output in fp32, 112 pixels per row
        y16 = K.r16(r64["y"].to(f32), s16).reshape(-1, Cout)
        val, mag = K.stats_of(y16)
        M = y16.shape[0]
        pad = torch.zeros(K.cdiv(M, 112) * 112 - M, Cout)
        v = torch.cat([y16.to(f32), pad]).reshape(-1, 112, Cout)
        K.check(_rows64(v.sum(1), (v * v).sum(1)), K.stats_q(val, mag, M, K.cdiv(M, 112)), c.name + " stats fp32", 0.25)
        if k != 3 or s != 1 or M % 196:
            continue
        # ---- the epilogues of the 3x3 / stride-1 kernels, one partial row per 196-pixel tile
        rows = M // 196
        yf = y16.to(f32)
        of = K.moments_other(M, Cout, False, s16)
        val, mag = K.moments(y16, of)
        K.check(_rows64(_tiles32(yf, Cout), _tiles32(yf * of, Cout), _tiles32(yf * yf, Cout)), K.moments_q(val, mag, M, rows), c.name + " moments fp32", 0.25)
        # eval epilogue: y, y with the identity path, y2
        ep = K.EpiPar(Cout, False, s16, 50)
        add = K.epi_add(M, Cout, ep, False, s16)
        a32 = y32.reshape(M, Cout)
        for alpha in (False, True):
            y0, ya, emag = K.epilogue_ref(r64["y"].reshape(M, Cout), r64["Sy"].reshape(M, Cout), ep, alpha, add)
            y0_32 = K.fma(a32, ep.scale, ep.shift, f32)
            if alpha:
                y0_32 = torch.where(y0_32 > 0, y0_32, y0_32 * ep.alpha)
            K.check(y0_32, K.epi_y_q(s16, y0, emag, Ky), c.name + " epilogue y fp32", 0.25)
            y0_16 = K.r16(y0_32, s16)
            qa = K.epi_yadd_q(s16, y0_16, add)
            K.check(y0_16.to(f32) + add, qa, c.name + " epilogue y + add fp32", 0.25)
            assert K.exceeds(K.r16(ya.to(f32), s16), qa), c.name + ": a single rounding of affine + identity must show"
            ys = K.r16(y0_16.to(f32) + add, s16)
            q2 = K.epi_y2_q(s16, ys, ep.scale2, ep.shift2)
            K.check(K.fma(ys.to(f32), ep.scale2, ep.shift2, f32), q2, c.name + " epilogue y2 fp32 fma", 0.25)
            K.check(ys.to(f32) * ep.scale2 + ep.shift2, q2, c.name + " epilogue y2 fp32", 0.25)
        # BatchNorm-backward rows in the kernels' form, PReLU-apply sums
        dx16 = K.r16(b64["dx"].to(f32), s16).reshape(-1, Cin)
        d = dx16.to(f32)
        par = K.BnPar(Cin, False, 60)
        bx, _ = K.bn_input(M, Cin, par, False, s16, 61)
        for prelu in (False, True):
            val, mag = K.bnbwd_rows(dx16, bx, par, prelu)
            t0, t1 = _tiles32(d, Cin), _tiles32(d * bx, Cin)
            t2 = torch.zeros_like(t0)
            if prelu:
                pos = torch.where(K.fma(bx, par.sc, par.sh, f32) <= 0, torch.zeros_like(d), d)
                sp, spx = _tiles32(pos, Cin), _tiles32(pos * bx, Cin)
                sn, snx = t0 - sp, t1 - spx
                t0, t1, t2 = sp + par.alpha * sn, spx + par.alpha * snx, par.sc * snx + par.sh * sn
            K.check(_rows64(t0, par.rstd * (t1 - par.mean * t0), t2), K.bnbwd_q(val, mag, M, rows), c.name + " bn-backward rows fp32", 0.25)
        for with_bias in (True, False):
            ax, bias, alpha_t = K.papply_operands(M, Cin, False, s16, with_bias)
            _, val, mag = K.papply_ref(dx16, ax, bias, alpha_t)
            z = ax if bias is None else ax + bias
            neg = z <= 0
            K.check(_rows64(_tiles32(torch.where(neg, d * alpha_t, d), Cin), _tiles32(torch.where(neg, d * z, torch.zeros_like(d)), Cin)),
                    K.papply_q(val, mag, M, rows), c.name + " prelu-apply sums fp32", 0.25)


# ------------------------------------------------------------------------------------------------ 5. mutants
def _differs(a, b):
    return not torch.equal(a.to(f64), b.to(f64))


@pytest.mark.parametrize("s16", S16, ids=IDS)
def test_mutants_show(s16):
    for tier in ("sparse", "multi", "tol"):
        c = K.ConvCase(3, 14, 128, 128, 3, 1, tier, s16)
        x, w = c.fwd()
        r = K.conv_ref(x, w, 1, f64, "cpu", want=("y",))
        y = r["y"]
        q = c.out16_q(y, r["Sy"], 9 * 128)
        muts = {"tap dropped at a border pixel": K.mut_drop_tap(y, x, w), "tap read from the neighbouring image": K.mut_cross_image(y, x, w),
                "tap wrapped to the next row": K.mut_wrap_row(y, x, w), "64-channel chunk dropped for one tile": K.mut_drop_chunk(y, x, w),
                "last pixel of the last tile omitted": K.mut_last_pixel(y)}
        for what, m in muts.items():
            assert _differs(m, y), (tier, what)
            if tier == "tol":
                assert K.exceeds(m, q), what
        # one row missing from a statistics column (of the stored output)
        y16 = K.r16(y.to(f32), s16).reshape(-1, 128)
        val, mag = K.stats_of(y16)
        for drop in (5, y16.shape[0] - 1):
            assert bool((y16[drop] != 0).any())
            assert _differs(K.stats_of(y16, drop=drop)[0], val), (tier, drop)
        if tier != "tol":
            other = K.dyadic(tuple(y16.shape), (0.5, -0.5, 1, -1, 2, 0), 1.0, 77)
            assert _differs(K.moments(y16, other, drop=5)[0], K.moments(y16, other)[0])
            par = K.BnPar(128, True)
            bx, _ = K.bn_input(y16.shape[0], 128, par, True, s16, 61)
            for prelu in (False, True):
                assert _differs(K.bnbwd_rows(y16, bx, par, prelu, drop=5)[0], K.bnbwd_rows(y16, bx, par, prelu)[0])
        # weight gradient: a split-K slab (one image) not added; the two layers of a pair swapped
        xa, dya = c.wg(0)
        xb, dyb = c.wg(100)
        z = torch.zeros(128, 3, 3, 128)
        ga = K.conv_ref(xa, z, 1, f64, "cpu", dy=dya, want=("dw",))
        gb = K.conv_ref(xb, z, 1, f64, "cpu", dy=dyb, want=("dw",))
        assert _differs(ga["dw"], gb["dw"]), tier
        slab = K.mut_drop_slab(ga["dw"], xa, dya, 1)
        assert _differs(slab, ga["dw"]), tier
        if tier == "tol":
            assert K.exceeds(slab, c.dw_q(ga["dw"], ga["Sdw"], 2)) and K.exceeds(gb["dw"], c.dw_q(ga["dw"], ga["Sdw"], 2))
        # stride-2 dgrad: one output-parity class with another class's taps
        c2 = K.ConvCase(2, 8, 64, 128, 3, 2, tier, s16)
        dy, wb = c2.bwd()
        b = K.conv_ref(torch.zeros(2, 8, 8, 64), wb, 2, f64, "cpu", dy=dy, want=("dx",))
        m = K.mut_parity(b["dx"], dy, wb)
        assert _differs(m, b["dx"]), tier
        if tier == "tol":
            assert K.exceeds(m, c2.out16_q(b["dx"], b["Sdx"], 9 * 128))
    # the 6x6 -> 3x3 case: the four parity classes have 1, 2, 2 and 4 taps, fewer at every border
    cnt = K.conv_ref(torch.zeros(1, 6, 6, 1), torch.ones(1, 3, 3, 1), 2, f64, "cpu", dy=torch.ones(1, 3, 3, 1), want=("dx",))["dx"][0, :, :, 0]
    assert cnt[0::2, 0::2].unique().tolist() == [1.0] and sorted(cnt[1::2, 1::2].unique().tolist()) == [1.0, 2.0, 4.0]
    assert sorted(cnt[0::2, 1::2].unique().tolist()) == [1.0, 2.0] and sorted(cnt[1::2, 0::2].unique().tolist()) == [1.0, 2.0]


# ------------------------------------------------------------------------------------------------ 6. the library's selector against the restated rules
@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__ as ge
    ge.build()
    from fedfr_amd import _C
    return _C


def _plan(lib, B, H, Cin, Cout, k, s, dgrad, want):
    out = [ctypes.c_int(-1) for _ in range(5)]
    rc = lib.fedfr_conv2d_plan(B, H, Cin, Cout, k, s, dgrad, want, *[ctypes.byref(v) for v in out])
    assert rc == 0, (rc, lib.fedfr_last_error_string(), (B, H, Cin, Cout, k, s, dgrad, want))
    return out[0].value, out[1].value, out[2].value, out[3].value, bool(out[4].value)


def test_plan_query_agrees_with_the_restated_rules(built_lib):
    """fedfr_conv2d_plan (no device: the persistent kernel is planned for 256 compute units) == conv_cases.plan_expected: slot, stat_rows,
    stat_rows_live, part_rows and out_epilogue, for every NT row of the table under its options and for the sweep of the issue."""
    _C, lib = built_lib, built_lib.lib()
    names = ("conv_c64p", "conv28_tpw2", "nt_glds", "dgrad_parity")

    def scope(vals):
        st = contextlib.ExitStack()
        for n, v in zip(names, vals):
            st.enter_context(_C.option_scope(n, v))
        return st

    # ---- the table: the plan gives each row's literal slot and row count
    nrows = 0
    for r in TABLE:
        if r.op.startswith("wgrad"):
            continue
        B, H, Cin, Cout, k, s = r.shape
        dgrad, want = int(r.op.startswith("dgrad")), K.ROW_WANT[r.op]
        opts = tuple(r.opt(n, d) for n, d in zip(names, (1, 2, 4, 2)))
        with scope(opts):
            got = _plan(lib, B, H, Cin, Cout, k, s, dgrad, want)
            assert got == K.plan_expected(B, H, Cin, Cout, k, s, dgrad, want, 256, *opts), (r.id, got)
            assert got[0] == r.slot, (r.id, got)
            if r.op in ("fwd_moments", "dgrad_bnbwd", "dgrad_papply"):
                assert got[3] == r.rows, (r.id, got)
            if r.op == "fwd_epi":
                assert got[4] and got[4] == K.conv_epilogue_ok(H, Cin, Cout, B * H * H, k, s), (r.id, got)
            if r.rows is not None and r.op in ("fwd", "fwd_stats"):      # (a plain "fwd" row with a row count is launched once more with statistics)
                live = _plan(lib, B, H, Cin, Cout, k, s, 0, K.WANT_STATS)
                assert live[2] == r.rows and live[1] == K.nt_stat_rows(B * (H // s) ** 2, Cout), (r.id, live)
        nrows += 1
    assert nrows >= 70
    # ---- the sweep: both sides of every batch threshold of test_batches_sit_on_the_thresholds, every option value, every want an op admits
    batches = sorted({124, 125, 250, 251, 62, 63, 15, 16, 3, 4} | set(K.c64p_batches(56, 256)) | set(K.c64p_batches(112, 256)))
    chans = (64, 128, 192, 256, 512)
    ops = [(dgrad, k, w) for dgrad in (0, 1) for k in (3, 1) for w in K.plan_wants(dgrad, k)]
    seen_slots, ncases = set(), 0
    for opts in itertools.product((0, 1), (0, 1, 2), (0, 4, 12), (0, 2)):
        with scope(opts):
            for H, s in itertools.product((7, 14, 28, 56, 112), (1, 2)):
                if H % s:                                   # (7x7 / stride 2 is no geometry of the library: conv_args_ok)
                    continue
                for Cin, Cout, B, (dgrad, k, want) in itertools.product(chans, chans, batches, ops):
                    got = _plan(lib, B, H, Cin, Cout, k, s, dgrad, want)
                    assert got == K.plan_expected(B, H, Cin, Cout, k, s, dgrad, want, 256, *opts), ((B, H, Cin, Cout, k, s, dgrad, want), opts, got)
                    if want & K.WANT_EPILOGUE:              # a launch that asks for the output epilogue: the persistent kernel steps aside
                        assert got[4] == K.conv_epilogue_ok(H, Cin, Cout, B * (H // s) ** 2, k, s)
                    seen_slots.add(got[0])
                    ncases += 1
    assert seen_slots == {0, 1, 2, 3, 12, 13, 15, 17} and ncases > 10 ** 6
    # what the entry point refuses: epilogues of the other direction, reductions of a 1x1 conv, a geometry the library has none of
    out = [ctypes.byref(ctypes.c_int()) for _ in range(5)]
    for bad in ((4, 14, 128, 128, 3, 1, 0, K.WANT_BNBWD), (4, 14, 128, 128, 3, 1, 1, K.WANT_STATS), (4, 14, 128, 128, 1, 1, 0, K.WANT_MOMENTS),
                (4, 7, 128, 128, 3, 2, 0, 0), (4, 14, 128, 128, 3, 1, 0, 32)):
        assert lib.fedfr_conv2d_plan(*bad, *out) == -1 and b"conv2d" in lib.fedfr_last_error_string(), bad
