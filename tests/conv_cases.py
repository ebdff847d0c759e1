"""Inputs, float64 references, tolerances and dispatch geometry for the direct tests of the convolution kernels (tests/test_conv_branches_gpu.py),
in the manner of stem_cases.py.  Nothing here touches the GPU library or imports the oracle.

Two tiers.

EXACT.  Inputs are few-bit dyadic numbers, so that every fp32 partial sum a kernel can form — whatever its tiling, K order, split-K or
regrouping — is an exact number, and the 16-bit result is exact too: the kernels must reproduce the float64 reference BIT FOR BIT.  A case is
admissible only if (the CPU test asserts all three for every case of the GPU table, no element excluded)
  (a) S / quantum < 2^24 for every output, S = sum |terms|: every fp32 partial sum in any order is exact;
  (b) every 16-bit result equals its own rounding to the storage type (11 significant bits fp16, 8 bf16);
  (c) for statistics / moment / BatchNorm-backward rows the whole-column sum of |terms| over all M rows stays below 2^24 quanta, which is
      sufficient for every grouping of the rows into partial rows.
Generators: "sparse" (x in {+-1, +-2}, w in {+-1}, density sqrt(terms / K) for both: |y| stays below 64, bf16-exact; what everything with
statistics uses) and "multi" (more mantissa bits for y / dx / dw alone: x in {+-1, +-2, +-3, 5, -7} / 4, w in {+-1, +-2, +-3, +-5} / 8 under
fp16; {+-1, +-2, +-3} / 4 and / 8 at the sparse density under bf16, whose 8 bits hold no more).  The epilogue operands (mean, rstd, gamma, beta,
alpha, scale, shift) are powers of two and small multiples of 1/4, with a negative gamma, a zero gamma and an exact z == 0 tie (masked): every
epilogue in the table — BatchNorm-backward rows, raw moments, the eval-mode affine + PReLU + identity + second output, the PReLU-apply — is
exact in fp32 in every order the kernels may use (x sc + sh or (x - mean) rstd gamma + beta, with and without fma: asserted), so NO quantity
had to move to the tolerance tier for that reason.

TOLERANCE.  Ordinary seeded inputs (gradients carry the fp16 loss scale 256), for what exactness cannot see: rounding mode, accumulation
precision, double rounding.  Every tolerance is element-wise and a formula of u16, 2^-24, a chain length and S = sum |terms|:
  16-bit conv output   u16 |ref| + (K + 2) 2^-24 S
  eval epilogue's y    the conv output's bound through the affine, + its two fp32 roundings (epi_y_q)
  ... with identity    round16(STORED y0 + add): u16 |ref| + 2^-24 |ref| (+ 2^-25 under fp16, its subnormal spacing) against the y0 the launch
                       without the identity path stored — the documented double rounding; a single rounding exceeds it (epi_yadd_q)
  ... second output    round16(STORED y scale2 + shift2): u16 |ref| + 2 2^-24 sum |terms| (+ 2^-25 under fp16) (epi_y2_q)
  fp32 weight gradient (Kp + splits + 2) 2^-24 S
  partial rows         (L + 2) 2^-24 sum |terms|, L = the most pixels one partial row covers (the rows are added in float64 by the test)
  rows the kernels form as rstd (sum dz x - mean sum dz) or sc sum + sh sum: the same with the |terms| of THAT form, L + 4
All of them are functions of this module (out16_q, dw_q, stats_q, moments_q, bnbwd_q, papply_q, epi_*_q); the CPU test holds the float32 evaluation
in kernel order to a quarter of each.
Output channels 0..15 of the weights are non-negative and the activations mostly positive, so that there S ~ |ref| and the bound sees the
rounding mode of the store (truncation instead of round-to-nearest-even exceeds it).

conv_ref is ONE plain function for forward, dgrad, wgrad and S: nine shifted [M][Cin] @ [Cin][Cout] matmuls at the given dtype, so that it runs
in float64 on the GPU through torch.matmul as well (there is no float64 convolution to call).  Layouts are the library's: activations NHWC,
weights KRSC."""
import math

import torch

from stem_cases import GSCALE, Q, U24, check, err_over_tol, exceeds, f32, f64, fma, nudge_from_zero, r16, u16, uniform  # noqa: F401

TWO24 = 2.0 ** 24


def mant_bits(s16):
    return 11 if s16 == torch.float16 else 8


def cdiv(a, b):
    return -(-a // b)


# ================================================================================================ dispatch geometry (restated from csrc)
def nt_bn(N):
    return 64 if N <= 64 else 128


def nt_bm(M, N):
    """gemm.hip: nt_bm — 128-row tiles unless that leaves fewer than 384 of them"""
    return 128 if cdiv(M, 128) * cdiv(N, nt_bn(N)) >= 384 else 64


def nt_generic_slot(M, N):
    """gemm.hip: prof_slot(false, BM, BN) — profile slots 0..3 = gemm_nt tiles <128,128> <128,64> <64,128> <64,64>"""
    return (0 if nt_bm(M, N) == 128 else 2) + (0 if nt_bn(N) == 128 else 1)


def nt_glds_applies(N, K, par=False, epilogue=False, nt_glds=4):
    """gemm_nt_glds.hip: gemm_nt_glds_applies with one split — the ring pays from 16 K-steps of 64 (option value + 8: every shape)"""
    pays = bool(nt_glds & 8) or (not par and cdiv(K, 64) >= 16)
    return (nt_glds & 7) > 0 and N > 64 and pays and not epilogue


def nt_glds_up(M, stats, nt_glds=4):
    """gemm_nt_glds.hip: launch_nt_glds `up` — a 64-row shape on 128-row tiles when both tilings agree on the statistics row count"""
    return (nt_glds & 7) >= 3 and (not stats or cdiv(M, 64) == 2 * cdiv(M, 128))


def conv_epilogue_ok(W, C, N, M, ksize, stride):
    """gemm.hip: gemm_nt_plan, out_epilogue of a launch that asks for it — the 3x3 / stride-1 shapes on a plain LDS-DMA instantiation"""
    if ksize != 3 or stride != 1 or W <= 0 or M % (W * W) or nt_bm(M, N) != 128:
        return False
    if W == 112:
        return C == 64 and N == 64
    if W == 56:
        return (C == 64 and N in (64, 128)) or (C == 128 and N == 64)
    if W in (14, 28):
        return N % 128 == 0 and C % 128 == 0
    return False


def conv_c64p_grid(M, cus):
    """conv_c64p.hip: c64p_deal — 224-pixel tiles dealt out evenly to at most one workgroup per CU"""
    ntiles = M // 224
    per_wg = cdiv(ntiles, min(ntiles, cus))
    return cdiv(ntiles, per_wg)


def nt_stat_rows(M, N):
    """gemm.hip: gemm_nt_stat_rows — rows of the statistics buffer (ceil(M / BM) * WM)"""
    bm = nt_bm(M, N)
    wm = 2 if bm == 128 else (2 if N <= 64 else 1)
    return cdiv(M, bm) * wm


def nt_stat_rows_live(M, N, C, W, ksize, stride, cus, conv_c64p=1, conv28_tpw2=2):
    """gemm.hip: gemm_nt_plan, stat_rows_live of a forward launch with statistics — the leading rows that carry data (the rest are zero filler)"""
    if W in (14, 28) and conv_epilogue_ok(W, C, N, M, ksize, stride):
        return M // 196 // 2 if (W == 28 and conv28_tpw2 and (M // 196) % 2 == 0) else M // 196 * 2
    if conv_c64p and ksize == 3 and stride == 1 and C == 64 and N == 64 and W in (56, 112) and M % (W * W) == 0:
        return 2 * conv_c64p_grid(M, cus)
    return nt_stat_rows(M, N)


def conv3x3_slot(M, W, C, N, fused=False, stats=False, epilogue=False, conv_c64p=1, nt_glds=4, bmom=False):
    """gemm.hip: nt_pick for a 3x3 / stride-1 / pad-1 conv whose GEMM has K = 9 C and N output columns (forward: C = cin, N = cout;
    dgrad: C = cout, N = cin).  fused: a BatchNorm-backward / moment / PReLU-apply reduction is asked for (bpart); bmom: it is one of the
    latter two (GemmNT::bmom != 0).  Returns the profile slot."""
    if conv_c64p and C == 64 and N == 64 and W in (56, 112) and not (fused and stats) and not epilogue and not bmom:
        return 15
    if nt_bm(M, N) == 128:
        if W == 112 and C == 64 and N == 64 and not fused:
            return 15
        if W == 56 and not fused and (C, N) in ((64, 64), (64, 128), (128, 64)):
            return 15
        if W in (14, 28) and N % 128 == 0 and C % 128 == 0:
            return 12 if W == 14 else 13
    if nt_glds_applies(N, 9 * C, epilogue=epilogue or fused, nt_glds=nt_glds):
        return 17
    return nt_generic_slot(M, N)


def w9_lg(W):
    return {14: 0, 28: 1, 56: 2, 112: 3}.get(W, -1)


def wgrad9_shape_ok(Kp, NI, NJ, C, W, stride):
    """wgrad9.hip: wgrad9_shape_ok"""
    return stride == 1 and w9_lg(W) >= 0 and C > 0 and C % 64 == 0 and NI % 32 == 0 and NJ == 9 * C and Kp % (W * W) == 0


def w9_stages(Kp, W):
    """wgrad9.hip: w9_stages — 14 x 14 sub-images"""
    return (Kp // (W * W)) << (2 * w9_lg(W))


def _whole_splits(stages, splits):
    splits = max(1, min(splits, stages // 2 if stages // 2 > 0 else 1))
    per = cdiv(stages, splits)
    return cdiv(stages, per)


def wgrad9_pick_splits(Kp, NI, NJ, W):
    """wgrad9.hip: wgrad9_pick_splits — ~256 workgroups, at least two stages per split"""
    return _whole_splits(w9_stages(Kp, W), max(1, 256 // ((NI // 32) * (NJ // 9 // 64))))


def wgrad9p_pick_splits(Kp, NI, NJ, W):
    """wgrad9p.hip: wgrad9p_pick_splits — 2 layers x tiles x splits ~ 256 workgroups"""
    return _whole_splits(w9_stages(Kp, W), max(1, 128 // ((NI // 64) * (NJ // 9 // 64))))


def tn_glds_shape_ok(NI, NJ, C):
    """gemm_tn_glds.hip: gemm_tn_glds_shape_ok (conv gather mode)"""
    return NI % 128 == 0 and NJ % 128 == 0 and C % 128 == 0


def tn_glds_pick_splits(Kp, NI, NJ):
    """gemm_tn_glds.hip: gemm_tn_glds_pick_splits"""
    tiles, ksteps = (NI // 128) * (NJ // 128), cdiv(Kp, 64)
    best, best_cost = 1, -1
    for s in range(1, min(64, ksteps // 4 + 1) + 1):
        per = cdiv(ksteps, s)
        if cdiv(ksteps, per) != s:
            continue
        cost = cdiv(tiles * s, 256) * (per + 8)
        if best_cost < 0 or cost < best_cost:
            best, best_cost = s, cost
    return best


def tn_generic_pick_splits(Kp, NI, NJ):
    """gemm.hip: tn_pick_splits_for (register-staged kernel, 416 workgroups aimed for, >= 4 K-steps per split)"""
    ti, tj = (64 if NI <= 64 else 128), (64 if NJ <= 64 else 128)
    tiles, ksteps = cdiv(NI, ti) * cdiv(NJ, tj), cdiv(Kp, 64)
    splits = min(cdiv(416, tiles), ksteps)
    while splits > 1 and ksteps // splits < 4:
        splits -= 1
    splits = max(splits, 1)
    return cdiv(ksteps, cdiv(ksteps, splits))


def tn_generic_slot(NI, NJ):
    """gemm.hip: prof_slot(true, TI, TJ) with gemm_tn_tiles — slots 4..7"""
    return 4 + (0 if NI > 64 else 2) + (0 if NJ > 64 else 1)


def wgrad_slot_splits(B, H, Cin, Cout, k, s, wgrad9=1, tn_glds=2, tn_use_tr=1):
    """gemm.hip: gemm_tn_pick_splits + gemm_tn_launch — (profile slot, K-splits) of one weight gradient"""
    Ho = H // s
    Kp, NI, NJ = B * Ho * Ho, Cout, k * k * Cin
    if wgrad9 and tn_use_tr and k == 3 and wgrad9_shape_ok(Kp, NI, NJ, Cin, Ho, s):
        return 16, wgrad9_pick_splits(Kp, NI, NJ, Ho)
    if tn_glds and tn_glds_shape_ok(NI, NJ, Cin):
        # (gemm_tn_pick_splits asks gemm_tn_glds_applies alone; gemm_tn_launch takes the LDS-DMA kernel only with transpose reads)
        return (14 if tn_use_tr else tn_generic_slot(NI, NJ)), tn_glds_pick_splits(Kp, NI, NJ)
    return tn_generic_slot(NI, NJ), tn_generic_pick_splits(Kp, NI, NJ)


# ================================================================================================ the reference
def _taps(H, k, stride):
    """per filter row r: (r, first output row, end output row, first input row) of the outputs whose tap r lands inside the image"""
    pad, Ho = (1 if k == 3 else 0), H // stride
    for r in range(k):
        o0 = max(0, cdiv(pad - r, stride))
        o1 = min(Ho, (H - 1 - r + pad) // stride + 1)
        yield r, o0, o1, o0 * stride + r - pad


def conv_ref(x, w, stride, dtype, device, dy=None, want=("y",), chunk=0, slabs=1):
    """x [B][H][H][Cin] (NHWC), w [Cout][k][k][Cin] (KRSC), dy [B][Ho][Ho][Cout], pad = k // 2.  Returns a dict with the quantities in `want`:
    "y" [B][Ho][Ho][Cout], "dx" [B][H][H][Cin], "dw" [Cout][k][k][Cin], each with its sum of |terms| under "S" + name.  chunk: the K side
    in channel chunks of that size, chunk-major (an accumulation order for the float32 evaluation); slabs: the weight gradient as that many
    groups of images, added last (split-K)."""
    B, H, _, Cin = x.shape
    Cout, k = w.shape[0], w.shape[1]
    Ho = H // stride
    xd, wd = x.to(device, dtype), w.to(device, dtype)
    dyd = None if dy is None else dy.to(device, dtype)
    xa, wa = xd.abs(), wd.abs()
    dya = None if dyd is None else dyd.abs()
    out = {}
    z = lambda *s: torch.zeros(s, dtype=dtype, device=device)  # noqa: E731
    if "y" in want:
        out["y"], out["Sy"] = z(B, Ho, Ho, Cout), z(B, Ho, Ho, Cout)
    if "dx" in want:
        out["dx"], out["Sdx"] = z(B, H, H, Cin), z(B, H, H, Cin)
    if "dw" in want:
        out["dw"], out["Sdw"] = z(Cout, k, k, Cin), z(Cout, k, k, Cin)
    cks = [(0, Cin)] if not chunk else [(c, min(c + chunk, Cin)) for c in range(0, Cin, chunk)]
    cko = [(0, Cout)] if not chunk else [(c, min(c + chunk, Cout)) for c in range(0, Cout, chunk)]
    groups = [(b * B // slabs, (b + 1) * B // slabs) for b in range(slabs)]
    for r, oh0, oh1, ih0 in _taps(H, k, stride):
        for s, ow0, ow1, iw0 in _taps(H, k, stride):
            if oh1 <= oh0 or ow1 <= ow0:
                continue
            hs = slice(ih0, ih0 + (oh1 - oh0 - 1) * stride + 1, stride)
            ws = slice(iw0, iw0 + (ow1 - ow0 - 1) * stride + 1, stride)
            if "y" in want:
                for c0, c1 in cks:
                    out["y"][:, oh0:oh1, ow0:ow1] += xd[:, hs, ws, c0:c1] @ wd[:, r, s, c0:c1].t()
                out["Sy"][:, oh0:oh1, ow0:ow1] += xa[:, hs, ws] @ wa[:, r, s].t()
            if "dx" in want:
                for c0, c1 in cko:
                    out["dx"][:, hs, ws] += dyd[:, oh0:oh1, ow0:ow1, c0:c1] @ wd[c0:c1, r, s]
                out["Sdx"][:, hs, ws] += dya[:, oh0:oh1, ow0:ow1] @ wa[:, r, s]
            if "dw" in want:
                for b0, b1 in groups:
                    if b1 > b0:
                        out["dw"][:, r, s] += dyd[b0:b1, oh0:oh1, ow0:ow1].reshape(-1, Cout).t() @ xd[b0:b1, hs, ws].reshape(-1, Cin)
                out["Sdw"][:, r, s] += dya[:, oh0:oh1, ow0:ow1].reshape(-1, Cout).t() @ xa[:, hs, ws].reshape(-1, Cin)
    return out


def tap_term(x, w, r, s, c0=0, c1=None):
    """the contribution of filter tap (r, s), channels c0:c1, of a 3x3 / stride-1 conv to every output pixel: [B][H][H][Cout] (float64, CPU)"""
    B, H, _, Cin = x.shape
    c1 = Cin if c1 is None else c1
    xp = torch.zeros(B, H + 2, H + 2, c1 - c0, dtype=f64)
    xp[:, 1:-1, 1:-1] = x[..., c0:c1].to(f64)
    return xp[:, r:r + H, s:s + H] @ w[:, r, s, c0:c1].to(f64).t()


# ================================================================================================ inputs
def dyadic(shape, vals, density, seed):
    """elements drawn from `vals` with probability `density`, else 0 (float32)"""
    g = torch.Generator().manual_seed(seed)
    pick = torch.tensor(vals, dtype=f32)[torch.randint(len(vals), shape, generator=g)]
    return torch.where(torch.rand(shape, generator=g) < density, pick, torch.zeros(()))


def cyc(vals, C, shift=0):
    return torch.tensor([vals[(i + shift) % len(vals)] for i in range(C)], dtype=f32)


SPARSE_X, SPARSE_W = (1, -1, 2, -2), (1, -1)
TIE = 3                     # the channel with gamma = rstd = 1, mean = 0, beta = -1/2 (z = x - 1/2) and x = 1/2 in every 7th row: z == 0, masked


def exact_sets(kind, s16, K):
    """(x values, w values, density, quantum of a product) of an exact generator for a sum over K"""
    if kind.startswith("sparse"):                          # "sparse": 24 non-zero terms per output on average; "sparseN": N
        return SPARSE_X, SPARSE_W, min(0.5, math.sqrt(float(kind[6:] or 24) / K)), 1.0
    if s16 == torch.float16:
        xv = [v / 4.0 for v in (1, -1, 2, -2, 3, -3, 5, -7)]
        wv = [v / 8.0 for v in (1, -1, 2, -2, 3, -3, 5, -5)]
        return xv, wv, min(0.4, math.sqrt(200.0 / K)), 1.0 / 32
    xv = [v / 4.0 for v in (1, -1, 2, -2, 3, -3)]
    wv = [v / 8.0 for v in (1, -1, 2, -2, 3, -3)]
    return xv, wv, min(0.5, math.sqrt(24.0 / K)), 1.0 / 32


class BnPar:
    """per-channel operands of a BatchNorm(+PReLU) backward reduction in front of a dgrad, all dyadic in the exact tier: gamma cycles through
    (1, -1, 0, 1/2, 2), rstd through (1, 1/2, 2), mean through (0, 1/2, -1/2, 1), beta through (0, 1/4, -1/4, -1/2); alpha = 1/4; channel TIE (and every
    16th after it) has z = x - 1/2.  Channels with mean = beta = 0 have shift == 0: every x == 0 of the input is a z == 0 tie there as well (what found the
    -0 threshold of epi_mfma.h)"""

    def __init__(self, C, exact, seed=0):
        if exact:
            self.gamma, self.rstd = cyc((1, -1, 0, 0.5, 2), C), cyc((1, 0.5, 2), C)
            self.mean, self.beta = cyc((0, 0.5, -0.5, 1), C), cyc((0, 0.25, -0.25, -0.5), C)
            self.alpha = torch.full((C,), 0.25)
            for t in (self.gamma, self.rstd):
                t[TIE::16] = 1.0
            self.mean[TIE::16], self.beta[TIE::16] = 0.0, -0.5
        else:
            self.gamma = uniform((C,), seed) * 0.2 + 1.0
            self.gamma[1::8] *= -1.0
            self.gamma[2::8] = 0.0
            self.rstd = uniform((C,), seed + 1) * 0.2 + 1.0
            self.mean, self.beta = uniform((C,), seed + 2) * 0.2, uniform((C,), seed + 3) * 0.3
            self.beta[2::8] = 0.05
            self.alpha = uniform((C,), seed + 4) * 0.1 + 0.25
            self.gamma[TIE::16], self.rstd[TIE::16], self.mean[TIE::16], self.beta[TIE::16] = 1.0, 1.0, 0.0, -0.5
        self.sc = (self.gamma.to(f64) * self.rstd.to(f64)).to(f32)
        self.sh = (self.beta.to(f64) - self.mean.to(f64) * self.sc.to(f64)).to(f32)


def bn_input(M, C, par, exact, s16, seed, ties=True):
    """the BatchNorm input bx [M][C]: quarters-free dyadic values (exact), or ordinary values moved off the PReLU threshold (tolerance);
    rows 0, 7, 14, ... of the TIE channels sit exactly on it"""
    if exact:
        bx = dyadic((M, C), (0.5, -0.5, 1, -1, 1.5, -1.5, 2, 0), 1.0, seed)
    else:
        bx = r16(uniform((M, C), seed) * 1.5 + 0.2, s16).to(f32)
    keep = torch.zeros(M, C, dtype=torch.bool)
    if ties:
        keep[::7, TIE::16] = True
        bx[keep] = 0.5
    if not exact:
        bx = nudge_from_zero(r16(bx, s16), par.sc, par.sh, s16, keep).to(f32)
    return bx, keep


def bnbwd_rows(dx, bx, par, prelu, dt=f64, drop=None):
    """the three column sums (sum dz, sum dz xhat, sum dx z over z <= 0) of a STORED dx [M][C] against bx, and the sum of |terms| of each in
    the form the kernels use: row 1 as rstd (sum dz x - mean sum dz), row 2 as sc sum dx x + sh sum dx over the masked elements.
    drop: a row left out (the corruption)"""
    d, x = dx.to(dt), bx.to(dt)
    g, r, mu, be, al = (t.to(d.device, dt) for t in (par.gamma, par.rstd, par.mean, par.beta, par.alpha))
    xhat = (x - mu) * r
    if prelu:
        z = g * xhat + be
        neg = z <= 0
        dz = torch.where(neg, d * al, d)
        t2 = torch.where(neg, d * z, torch.zeros_like(d))
        sc, sh = g * r, be - mu * g * r
        a2 = torch.where(neg, (d * x).abs() * sc.abs() + d.abs() * sh.abs(), torch.zeros_like(d))
    else:
        dz, t2, a2 = d, torch.zeros_like(d), torch.zeros_like(d)
    t = [dz, dz * xhat, t2]
    a = [dz.abs(), ((dz * x).abs() + dz.abs() * mu.abs()) * r, a2]
    if drop is not None:
        t = [v.clone() for v in t]
        for v in t:
            v[drop] = 0
    return torch.stack([v.sum(0) for v in t]), torch.stack([v.sum(0) for v in a])


def papply_ref(dx, ax, bias, alpha, dt=f64):
    """sphnet's PReLU-apply on a dgrad result dx [M][C]: z = ax + bias, dz = dx (z <= 0 ? alpha : 1); rows (sum dz, sum dx z over z <= 0)"""
    d, x = dx.to(dt), ax.to(dt)
    z = x + (0 if bias is None else bias.to(d.device, dt))
    neg = z <= 0
    dz = torch.where(neg, d * alpha.to(d.device, dt), d)
    t2 = torch.where(neg, d * z, torch.zeros_like(d))
    return dz, torch.stack([dz.sum(0), t2.sum(0)]), torch.stack([dz.abs().sum(0), t2.abs().sum(0)])


def moments(y, other, dt=f64, drop=None):
    """raw moments (sum y, sum y other, sum y y) of a STORED y [M][C] and the sums of |terms|"""
    yv, o = y.to(dt), other.to(dt)
    t = [yv, yv * o, yv * yv]
    if drop is not None:
        t = [v.clone() for v in t]
        for v in t:
            v[drop] = 0
    return torch.stack([v.sum(0) for v in t]), torch.stack([v.abs().sum(0) for v in t])


class EpiPar:
    """operands of the eval-mode output epilogue: y = prelu_alpha(acc scale + shift) (+ add); y2 = y scale2 + shift2.  Exact tier: powers of
    two and quarters sized to the storage type's mantissa (bf16: halves and integers, alpha = 1/2)"""

    def __init__(self, C, exact, s16, seed=0):
        if exact and s16 == torch.float16:
            self.scale, self.shift = cyc((1, 0.5, 2, -1), C), cyc((0, 0.25, -0.5, 1, -0.25), C)
            self.alpha = torch.full((C,), 0.25)
            self.scale2, self.shift2 = cyc((1, 2, -1), C), cyc((0, 0.5, -0.25, 1), C)
            self.add_vals = (0, 0.25, -0.25, 0.5, -0.5, 1)
        elif exact:
            self.scale, self.shift = cyc((1, -1, 2), C), cyc((0, 1, -1, 2), C)
            self.alpha = torch.full((C,), 0.5)
            self.scale2, self.shift2 = cyc((1, 2, -1), C), cyc((0, 1, -1), C)
            self.add_vals = (0, 0.5, -0.5, 1, -1)
        else:
            self.scale, self.shift = uniform((C,), seed) * 0.2 + 0.05, uniform((C,), seed + 1) * 0.5
            self.scale[1::8] *= -1.0
            self.alpha = uniform((C,), seed + 2) * 0.1 + 0.25
            self.scale2, self.shift2 = uniform((C,), seed + 3) * 0.3 + 1.0, uniform((C,), seed + 4) * 0.3
            self.add_vals = None


def epilogue_ref(acc, Sacc, ep, alpha, add, dt=f64):
    """y before its 16-bit store(s): (prelu(acc scale + shift), the same + add or None) and the |terms| of the affine"""
    a = acc.to(dt)
    sc, sh = ep.scale.to(a.device, dt), ep.shift.to(a.device, dt)
    y0 = a * sc + sh
    mag = Sacc.to(dt) * sc.abs()
    if alpha:
        al = ep.alpha.to(a.device, dt)
        mag = torch.where(y0 > 0, mag, mag * al)
        y0 = torch.where(y0 > 0, y0, y0 * al)
    return y0, (None if add is None else y0 + add.to(a.device, dt)), mag


# ================================================================================================ cases
class ConvCase:
    """one conv geometry with its inputs for one tier.  tier: "sparse" | "sparse6" | "multi" (exact) or "tol".  Tensors are float32 holding
    values the storage type represents exactly: x [B][H][H][Cin], w [Cout][k][k][Cin], dy [B][Ho][Ho][Cout]."""

    def __init__(self, B, H, Cin, Cout, k, s, tier, s16, seed=0):
        self.B, self.H, self.Cin, self.Cout, self.k, self.s, self.tier, self.s16, self.seed = B, H, Cin, Cout, k, s, tier, s16, seed
        self.Ho = H // s
        self.exact = tier != "tol"
        self.M_out, self.M_in = B * self.Ho * self.Ho, B * H * H
        self.name = "conv[%d,%d,%d->%d,k%d,s%d,%s]" % (B, H, Cin, Cout, k, s, tier)

    # ---- forward operands (K = k k Cin), dgrad operands (K = k k Cout), weight-gradient operands (K = output pixels)
    def fwd(self):
        K = self.k * self.k * self.Cin
        if self.exact:
            xv, wv, p, _ = exact_sets(self.tier, self.s16, K)
            return dyadic((self.B, self.H, self.H, self.Cin), xv, p, self.seed + 1), dyadic((self.Cout, self.k, self.k, self.Cin), wv, p, self.seed + 2)
        x = r16(uniform((self.B, self.H, self.H, self.Cin), self.seed + 1, -0.1, 1.0), self.s16).to(f32)
        w = uniform((self.Cout, self.k, self.k, self.Cin), self.seed + 2) * 0.1
        w[:16] = w[:16].abs() * (0.5 + torch.arange(16.0) / 32).reshape(16, 1, 1, 1)       # coherent output channels: S ~ |y| there, at 16 different scales
        return x, r16(w, self.s16).to(f32)

    def bwd(self):
        K = self.k * self.k * self.Cout
        if self.exact:
            xv, wv, p, _ = exact_sets(self.tier, self.s16, K)
            return dyadic((self.B, self.Ho, self.Ho, self.Cout), xv, p, self.seed + 3), dyadic((self.Cout, self.k, self.k, self.Cin), wv, p, self.seed + 4)
        dy = r16(uniform((self.B, self.Ho, self.Ho, self.Cout), self.seed + 3, -0.1, 1.0) * GSCALE, self.s16).to(f32)
        w = uniform((self.Cout, self.k, self.k, self.Cin), self.seed + 4) * 0.1
        w[..., :16] = w[..., :16].abs() * (0.5 + torch.arange(16.0) / 32)                      # coherent input channels: S ~ |dx| there
        return dy, r16(w, self.s16).to(f32)

    def wg(self, seed=0):
        if self.exact:
            xv, wv, p, _ = exact_sets("multi" if self.tier == "multi" else "sparse", self.s16, self.M_out)
            return (dyadic((self.B, self.H, self.H, self.Cin), xv, p, self.seed + seed + 5),
                    dyadic((self.B, self.Ho, self.Ho, self.Cout), wv, p, self.seed + seed + 6))
        x = r16(uniform((self.B, self.H, self.H, self.Cin), self.seed + seed + 5, -0.25, 1.0), self.s16).to(f32)
        dy = r16(uniform((self.B, self.Ho, self.Ho, self.Cout), self.seed + seed + 6) * GSCALE, self.s16).to(f32)
        return x, dy

    def quantum(self, which):
        K = {"y": self.k * self.k * self.Cin, "dx": self.k * self.k * self.Cout, "dw": self.M_out}[which]
        kind = self.tier if which != "dw" else ("multi" if self.tier == "multi" else "sparse")
        return exact_sets(kind, self.s16, K)[3]

    # ---- tolerances
    def out16_q(self, ref, S, K):
        """a 16-bit conv output: u16 |ref| + (K + 2) 2^-24 S"""
        return Q(ref, u16(self.s16) * ref.abs().to("cpu", f64) + (K + 2) * U24 * S.to("cpu", f64))

    def dw_q(self, ref, S, splits):
        """an fp32 weight gradient: (Kp + splits + 2) 2^-24 S"""
        return Q(ref, (self.M_out + splits + 2) * U24 * S.to("cpu", f64))


def floor16(s16):
    """what u16 |ref| does not cover of a 16-bit store: below 2^-14 fp16 rounds to multiples of 2^-24, half that spacing (results that land there by
    cancellation cannot be kept out of an affine of ordinary inputs); nothing for bf16, whose exponent range is fp32's"""
    return 2.0 ** -25 if s16 == torch.float16 else 0.0


def rows_q(val, mag, L, extra=2):
    """partial rows added in float64: (L + extra) 2^-24 sum |terms|, L = the most pixels one partial row covers"""
    return Q(val, (L + extra) * U24 * mag.to("cpu", f64))


def rows_L(M, rows):
    """chain length of a partial row: no row of the kernels' layouts covers more than twice the mean row's pixels"""
    return 2 * cdiv(M, rows)


def stats_q(val, mag, M, rows):
    """(sum, sum of squares) rows of the 16-bit output"""
    return rows_q(val, mag, rows_L(M, rows))


def moments_q(val, mag, M, rows):
    """raw-moment rows (sum y, sum y other, sum y y)"""
    return rows_q(val, mag, rows_L(M, rows))


def bnbwd_q(val, mag, M, rows):
    """BatchNorm-backward rows: the kernels form row 1 as rstd (sum dz x - mean sum dz) and row 2 as sc sum + sh sum from fp32 sums: two more
    roundings than a plain sum (L + 4), on the |terms| of THAT form (bnbwd_rows returns them)"""
    return rows_q(val, mag, rows_L(M, rows), 4)


def papply_q(val, mag, M, rows):
    """PReLU-apply rows (sum dz, sum dy z over z <= 0): plain fp32 sums of one product each"""
    return rows_q(val, mag, rows_L(M, rows))


def epi_y_q(s16, y0, mag, Kc):
    """the eval epilogue's y = round16(prelu(acc scale + shift)): the conv output's bound through the affine (mag = S |scale| (alpha)), and the
    affine's own two fp32 roundings"""
    y0 = y0.to("cpu", f64)
    m = mag.to("cpu", f64)
    return Q(y0, u16(s16) * y0.abs() + (Kc + 2) * U24 * m + 2 * U24 * (y0.abs() + m))


def epi_yadd_q(s16, y0_16, add):
    """with the identity path y = round16(y0 + add) of the STORED 16-bit y0 (the value the launch without `add` stores): one fp32 sum of two
    16-bit values, rounded once more — a kernel that adds to the unrounded affine instead misses this bound by up to u16 |y0|"""
    ref = y0_16.to("cpu", f64) + add.to("cpu", f64)
    return Q(ref, u16(s16) * ref.abs() + U24 * ref.abs() + floor16(s16))


def epi_y2_q(s16, y16, sc2, sh2):
    """the second output y2 = round16(y scale2 + shift2) of the STORED y: one fp32 affine and one 16-bit rounding"""
    yd, a, b = y16.to("cpu", f64), sc2.to("cpu", f64), sh2.to("cpu", f64)
    ref = yd * a + b
    return Q(ref, u16(s16) * ref.abs() + 2 * U24 * ((yd * a).abs() + b.abs()) + floor16(s16))


# ---- the epilogue operands of a case (the GPU test and the CPU test build the same ones)
def moments_other(M, C, exact, s16):
    return dyadic((M, C), (0.5, -0.5, 1, -1, 2, 0), 1.0, 77) if exact else r16(uniform((M, C), 77) * 1.3 + 0.25, s16).to(f32)


def epi_add(M, C, ep, exact, s16):
    return dyadic((M, C), ep.add_vals, 1.0, 78) if exact else r16(uniform((M, C), 78) * 1.5, s16).to(f32)


def papply_operands(M, C, exact, s16, with_bias):
    """(act_x [M][C], bias or None, alpha) of a PReLU-apply dgrad; exact tier: rows 0, 7, ... of the TIE channels have z == 0"""
    alpha = torch.full((C,), 0.25) if exact else uniform((C,), 70) * 0.1 + 0.25
    bias_t = cyc((0, 0.5, -0.5, 1), C) if exact else uniform((C,), 71) * 0.3
    bias = bias_t if with_bias else None
    if exact:
        ax = dyadic((M, C), (0.5, -0.5, 1, -1, 1.5, -1.5, 2, 0), 1.0, 72)
        ax[::7, TIE::16] = -float(bias_t[TIE]) if with_bias else 0.0
    else:
        ax = r16(uniform((M, C), 72) * 1.5 + 0.2, s16)
        ax = nudge_from_zero(ax, torch.ones(C), bias if with_bias else torch.zeros(C), s16).to(f32)
    return ax, bias, alpha


def stats_of(y16, dt=f64, drop=None):
    """(sum, sum of squares) per channel of a STORED y [M][C] and the sums of |terms|"""
    v = y16.to(dt)
    if drop is not None:
        v = v.clone()
        v[drop] = 0
    return torch.stack([v.sum(0), (v * v).sum(0)]), torch.stack([v.abs().sum(0), (v * v).sum(0)])


def trunc16(t, s16):
    """t rounded TOWARD ZERO to the storage type (the corruption of a store's rounding mode)"""
    t = t.to(f64)
    mb = mant_bits(s16)
    e = torch.floor(torch.log2(t.abs().clamp_min(1e-300)))
    q = torch.pow(torch.tensor(2.0, dtype=f64), e - (mb - 1))
    return torch.trunc(t / q) * q


def is_representable(t, s16):
    t = t.to("cpu", f64)
    return bool((t.to(f32).to(s16).to(f64) == t).all())


# ---- admissibility of an exact case (conditions a, b, c)
def admissible_out(ref, S, quantum, s16=None):
    """(a) every S below 2^24 quanta and every value a whole number of quanta; (b) with s16, every value representable in it"""
    r, Sv = ref.to("cpu", f64), S.to("cpu", f64)
    n = r / quantum
    ok = bool((n == n.round()).all()) and float(Sv.max()) / quantum < TWO24
    return ok and (s16 is None or is_representable(r, s16))


def admissible_col(mag, quantum, scale=1.0):
    """(c) whole-column sums of |terms| (times `scale`, when they were taken over a part of the rows) below 2^24 quanta"""
    return float(mag.to("cpu", f64).max()) * scale / quantum < TWO24


# ================================================================================================ mutants (on float64 reference values, CPU)
def mut_drop_tap(y, x, w):
    """tap (0, 0) dropped at the pixel (row 1, last column) of image 0 — a right-border pixel"""
    H = x.shape[1]
    o = y.clone()
    o[0, 1, H - 1] -= x[0, 0, H - 2].to(f64) @ w[:, 0, 0].to(f64).t()
    return o


def mut_cross_image(y, x, w):
    """tap row 0 of the top row of image 1 reads the last row of image 0 instead of the padding"""
    o = y.clone()
    o[1, 0, 1:-1] += x[0, -1, 1:-1].to(f64) @ w[:, 0, 1].to(f64).t()
    return o


def mut_wrap_row(y, x, w):
    """tap column 2 of the pixels in the last column reads the first pixel of the next row instead of the padding"""
    o = y.clone()
    o[:, :-1, -1] += x[:, 1:, 0].to(f64) @ w[:, 1, 2].to(f64).t()
    return o


def mut_drop_chunk(y, x, w, rows=128):
    """the centre tap's first 64-channel chunk dropped for the first tile of `rows` output pixels"""
    o = y.clone()
    t = tap_term(x, w, 1, 1, 0, 64).reshape(-1, y.shape[-1])
    o.reshape(-1, y.shape[-1])[:rows] -= t[:rows]
    return o


def mut_last_pixel(y):
    o = y.clone()
    o[-1, -1, -1] = 0
    return o


def mut_parity(dx, dy, w):
    """stride-2 dgrad: the (even, even) output class computed with the taps of the (even, odd) class"""
    o = dx.clone()
    d, wv = dy.to(f64), w.to(f64)
    nxt = torch.zeros_like(d)
    nxt[:, :, :-1] = d[:, :, 1:]
    o[:, 0::2, 0::2] = nxt @ wv[:, 1, 0] + d @ wv[:, 1, 2]
    return o


def mut_drop_slab(dw, x, dy, b, stride=1):
    """the weight gradient without image b (one split-K slab not added)"""
    one = conv_ref(x[b:b + 1], torch.zeros(dy.shape[-1], dw.shape[1], dw.shape[1], x.shape[-1]), stride, f64, "cpu", dy=dy[b:b + 1], want=("dw",))
    return dw - one["dw"]


# ================================================================================================ the case table of the GPU test
class Row:
    """one row: the entry point (op), the geometry (B, H, Cin, Cout, k, s), option switches, the profile slot that must count `launches`
    launches (and no other GEMM slot any), the partial / statistics row count where the op leaves rows, and the tiers it runs in"""

    def __init__(self, op, shape, slot, launches=1, opts=(), rows=None, tiers=("sparse", "tol"), prelu=False):
        self.op, self.shape, self.slot, self.launches, self.opts, self.rows, self.tiers, self.prelu = op, shape, slot, launches, tuple(opts), rows, tiers, prelu
        self.id = "%s%s-%s%s" % (op, "+prelu" if prelu else "", "x".join(str(v) for v in shape), "".join("-%s=%d" % o for o in self.opts))

    def opt(self, name, default):
        return dict(self.opts).get(name, default)


PLAIN = ("multi", "tol")        # y / dx / dw alone: the generator with more mantissa bits
SMALL = ("sparse6", "tol")      # epilogues that multiply the result again, and the longest columns: fewer terms per output


def fused_rows(M, W, conv28_tpw2=2):
    """conv_glds_impl.h: launch_glds — one partial row per 196-pixel tile, per PAIR of tiles on the two-tiles 28x28 kernel
    (gemm.hip: nt_pick)"""
    return M // 392 if (W == 28 and conv28_tpw2 >= 2 and (M // 196) % 2 == 0) else M // 196


def c64p_batches(W, cus):
    """(one tile per workgroup, the smallest batch with more tiles than CUs, the next one whose last workgroup is short)"""
    per_img = W * W // 224
    b1 = cus // per_img + 1
    b2 = b1 + 1
    while (b2 * per_img) % cdiv(b2 * per_img, cus) == 0:
        b2 += 1
    return 1, b1, b2


def table(cus=256):
    T = []
    add = lambda *a, **k: T.append(Row(*a, **k))  # noqa: E731

    def lds_dma_family(shape, slot, stats_rows, frows, opts=(), ops=("fwd", "fwd_stats", "fwd_moments", "fwd_epi", "dgrad", "dgrad_bnbwd", "dgrad_bnbwd+", "dgrad_papply")):
        for op in ops:
            if op in ("fwd", "dgrad"):
                add(op, shape, slot, opts=opts, tiers=PLAIN)
            elif op == "fwd_stats":
                add(op, shape, slot, opts=opts, rows=stats_rows)
            elif op == "fwd_epi":
                add(op, shape, slot, launches=8, opts=opts, tiers=SMALL)
            elif op == "dgrad_bnbwd+":
                add("dgrad_bnbwd", shape, slot, opts=opts, rows=frows, tiers=SMALL, prelu=True)
            else:                                           # (the PReLU-apply runs with and without a bias)
                add(op, shape, slot, launches=2 if op == "dgrad_papply" else 1, opts=opts, rows=frows, tiers=SMALL)

    # ---- 14x14, conv3x3_glds<14> (slot 12): 128-row tiles from B = 125 (ceil(24 500 / 128) * 2 = 384); an odd batch beside it
    for B in (125, 131):
        lds_dma_family((B, 14, 256, 256, 3, 1), 12, 2 * B, B)
    add("fwd", (125, 14, 128, 256, 3, 1), 12, tiers=PLAIN)            # one input chunk pair, two output tiles
    add("dgrad", (125, 14, 128, 256, 3, 1), 17, tiers=PLAIN)          # its dgrad has N = 128: 192 tiles, 64-row shape -> gemm_nt_glds
    add("fwd", (251, 14, 256, 128, 3, 1), 12, tiers=PLAIN)            # N = 128 needs ceil(M / 128) >= 384: B = 251 (B = 250 leaves 383)
    add("dgrad", (251, 14, 256, 128, 3, 1), 12, tiers=PLAIN)          # C = 128 -> N = 256: the other chunk count
    # ---- 28x28, conv3x3_glds<28> (slot 13): from B = 63; 4 B tiles, always even: the two-tiles kernels by default, the one-tile ones by option
    s28 = (63, 28, 128, 128, 3, 1)
    lds_dma_family(s28, 13, 126, 126)
    lds_dma_family(s28, 13, 504, 252, opts=(("conv28_tpw2", 0),))          # one tile per workgroup everywhere
    lds_dma_family(s28, 13, 126, 252, opts=(("conv28_tpw2", 1),))          # two tiles only in the forward launches with statistics
    # ---- 56x56 (from B = 16) and 112x112 (from B = 4) on the LDS-DMA kernels (slot 15); 64 -> 64 only with the persistent kernel off
    for shp, opts in (((16, 56, 64, 128, 3, 1), ()), ((16, 56, 128, 64, 3, 1), ()), ((16, 56, 64, 64, 3, 1), (("conv_c64p", 0),)),
                      ((4, 112, 64, 64, 3, 1), (("conv_c64p", 0),))):
        lds_dma_family(shp, 15, nt_stat_rows(shp[0] * shp[1] * shp[1], shp[3]), None, opts=opts, ops=("fwd", "fwd_stats", "fwd_epi", "dgrad"))
    add("dgrad_bnbwd", (16, 56, 64, 64, 3, 1), 1, opts=(("conv_c64p", 0),), rows=0, tiers=SMALL, prelu=True)      # no fused LDS-DMA kernel there: generic <128,64>, caller reduces
    # ---- the persistent 64-channel kernel (slot 15; told from the kernels above by its row counts): plain, STATS, BWD = 1, BWD = 2
    for W in (56, 112):
        for B in c64p_batches(W, cus)[(0 if W == 56 else 1):]:
            shp, g = (B, W, 64, 64, 3, 1), conv_c64p_grid(B * W * W, cus)
            add("fwd", shp, 15, rows=2 * g)                  # (sparse tier: the row check needs condition c; a plain launch leaves no rows: the test launches the shape once more with statistics, see run_fwd)
            add("fwd_stats", shp, 15, rows=2 * g)
            tiers = SMALL if B * W * W < 100000 else ("sparse1", "tol")       # the longest columns: condition (c) needs still smaller gradients
            add("dgrad_bnbwd", shp, 15, rows=g, tiers=tiers)
            add("dgrad_bnbwd", shp, 15, rows=g, tiers=tiers, prelu=True)
    # ---- gemm_nt_glds (slot 17): 3x3 with >= 16 K-steps that no conv kernel takes; nt_glds = 0 / 1 are the register-staged kernel / 64-row ring tiles
    s7 = (3, 7, 512, 512, 3, 1)                                        # M = 147: ragged; with statistics 3 rows of 64 != 2 x 2: NOT taken up to 128-row tiles
    add("fwd", s7, 17, tiers=PLAIN)
    add("dgrad", s7, 17, tiers=PLAIN)
    for o, slot in (((), 17), ((("nt_glds", 0),), 2), ((("nt_glds", 1),), 17)):
        add("fwd_stats", s7, slot, opts=o, rows=3)
    add("fwd_stats", (4, 7, 512, 512, 3, 1), 17, rows=4)              # M = 196: 4 rows either way: taken up
    s8 = (5, 8, 512, 512, 3, 2)                                        # stride-2 forward, M = 80
    for o, slot in (((), 17), ((("nt_glds", 0),), 2), ((("nt_glds", 1),), 17)):
        add("fwd", s8, slot, opts=o, tiers=PLAIN)
    add("fwd_stats", s8, 17, rows=2)
    add("fwd_stats", (3, 28, 128, 256, 3, 2), 17, rows=10)             # M = 588, 18 K-steps
    add("fwd_stats", (125, 28, 128, 256, 3, 2), 17, rows=384)          # 128-row shape (192 x 2 tiles)
    add("fwd_stats", (2, 16, 64, 128, 3, 2), 2, rows=2)                # 9 K-steps: the ring does not pay -> generic <64,128>
    # ---- generic gemm_nt tiles (slots 0..3): short K
    for shp, sf, sd in (((63, 56, 64, 128, 1, 2), 0, 1), ((16, 56, 64, 64, 1, 1), 1, 1), ((3, 14, 128, 256, 1, 2), 2, 2), ((2, 14, 64, 64, 3, 1), 3, 3)):
        add("fwd_stats", shp, sf, rows=nt_stat_rows(shp[0] * (shp[1] // shp[5]) ** 2, shp[3]))
        add("dgrad", shp, sd, tiers=PLAIN)
    # ---- stride-2 3x3 dgrad by output-parity class: one launch (2), four (1), the plain zero-inserted GEMM (0)
    for shp, s2, s0 in (((2, 16, 64, 128, 3, 2), 3, 3), ((5, 8, 512, 512, 3, 2), 2, 17), ((1, 6, 64, 64, 3, 2), 3, 3)):
        add("dgrad", shp, s2, tiers=PLAIN)
        add("dgrad", shp, s2, launches=4, opts=(("dgrad_parity", 1),), tiers=PLAIN)
        add("dgrad", shp, s0, opts=(("dgrad_parity", 0),), tiers=PLAIN)
    # ---- weight gradients: nine-tap kernel (slot 16) on every width; splits == 1 (one stage), a stage count the splits do not divide; Cout = 64, 192
    for shp in ((1, 14, 256, 256, 3, 1), (1, 28, 128, 128, 3, 1), (1, 56, 64, 64, 3, 1), (1, 112, 64, 64, 3, 1), (5, 14, 128, 128, 3, 1),
                (3, 14, 64, 64, 3, 1), (3, 14, 64, 192, 3, 1)):
        add("wgrad", shp, 16, tiers=PLAIN)
    for shp in ((24, 14, 128, 128, 3, 1), (16, 28, 128, 128, 3, 1), (3, 56, 64, 64, 3, 1), (5, 14, 128, 128, 3, 1)):
        add("wgrad_pair", shp, 16, tiers=PLAIN)
    sp = (24, 14, 128, 128, 3, 1)
    add("wgrad_pair", sp, 16, launches=2, opts=(("wgrad9p", 0),), tiers=PLAIN)
    # (the switches wgrad9p_bg and wgrad_pair_reduce act inside the network's backward pass only — the W9PJob of wgrad9p.hip —: no entry point reaches them, no row)
    sg = (8, 14, 256, 256, 3, 1)
    add("wgrad", sg, 14, opts=(("wgrad9", 0),), tiers=PLAIN)                    # gemm_tn_glds, eight waves
    add("wgrad", sg, 14, opts=(("wgrad9", 0), ("tn_glds", 1)), tiers=PLAIN)     # four waves
    add("wgrad", sg, 4, opts=(("wgrad9", 0), ("tn_glds", 0)), tiers=PLAIN)      # register-staged <128,128>
    add("wgrad", sg, 4, opts=(("tn_use_tr", 0),), tiers=PLAIN)                  # scalar LDS fragments: neither nine-tap nor LDS-DMA kernel
    add("wgrad", (5, 8, 512, 512, 3, 2), 14, tiers=PLAIN)
    add("wgrad", (3, 14, 128, 256, 1, 2), 14, tiers=PLAIN)
    for shp, slot in (((2, 16, 64, 128, 3, 2), 4), ((2, 14, 64, 128, 1, 1), 5), ((2, 14, 128, 64, 1, 1), 6), ((2, 14, 64, 64, 1, 1), 7)):
        add("wgrad", shp, slot, tiers=PLAIN)
        add("wgrad", shp, slot, opts=(("tn_use_tr", 0),), tiers=PLAIN)
    return T


def expected_rows(row, cus=256):
    """the statistics / partial row count the restated rules give a row that leaves rows (None otherwise)"""
    B, H, Cin, Cout, k, s = row.shape
    Ho = H // s
    c64p, tpw2 = row.opt("conv_c64p", 1), row.opt("conv28_tpw2", 2)
    if row.op == "fwd_stats" or (row.op == "fwd" and row.rows is not None):
        return nt_stat_rows_live(B * Ho * Ho, Cout, Cin, H, k, s, cus, c64p, tpw2)
    if row.op in ("fwd_moments", "dgrad_bnbwd", "dgrad_papply"):
        M = B * H * H
        C, N = (Cin, Cout) if row.op == "fwd_moments" else (Cout, Cin)
        if row.op == "dgrad_bnbwd" and c64p and C == 64 and N == 64 and H in (56, 112):
            return conv_c64p_grid(M, cus)
        if H in (14, 28) and conv_epilogue_ok(H, C, N, M, k, s):
            return fused_rows(M, H, tpw2)
        return 0
    return None


def expected_slot(row, cus=256):
    """the slot the restated dispatch rules give a row (the CPU test holds the table's literal slots to it)"""
    B, H, Cin, Cout, k, s = row.shape
    Ho = H // s
    if row.op.startswith("wgrad"):
        return wgrad_slot_splits(B, H, Cin, Cout, k, s, row.opt("wgrad9", 1), row.opt("tn_glds", 2), row.opt("tn_use_tr", 1))[0]
    c64p, ntg = row.opt("conv_c64p", 1), row.opt("nt_glds", 4)
    if row.op.startswith("fwd"):
        M, N, C, W = B * Ho * Ho, Cout, Cin, H
        if k == 3 and s == 1:
            return conv3x3_slot(M, W, C, N, fused=row.op == "fwd_moments", stats=row.op == "fwd_stats", epilogue=row.op == "fwd_epi", conv_c64p=c64p, nt_glds=ntg,
                                bmom=row.op == "fwd_moments")
        return 17 if nt_glds_applies(N, k * k * C, nt_glds=ntg) else nt_generic_slot(M, N)
    # dgrad: GEMM over K = k k Cout with N = Cin
    if k == 1:
        return nt_generic_slot(B * Ho * Ho, Cin)
    if s == 1:
        return conv3x3_slot(B * H * H, H, Cout, Cin, fused=row.op != "dgrad", conv_c64p=c64p, nt_glds=ntg, bmom=row.op == "dgrad_papply")
    par = row.opt("dgrad_parity", 2)
    if par:
        return nt_generic_slot(B * H * H // 4, Cin)
    return 17 if nt_glds_applies(Cin, 9 * Cout, nt_glds=ntg) else nt_generic_slot(B * H * H, Cin)


# want bits of fedfr_conv2d_plan (include/fedfr_hip.h)
WANT_STATS, WANT_BNBWD, WANT_MOMENTS, WANT_PAPPLY, WANT_EPILOGUE = 1, 2, 4, 8, 16
ROW_WANT = {"fwd": 0, "fwd_stats": WANT_STATS, "fwd_moments": WANT_MOMENTS, "fwd_epi": WANT_EPILOGUE, "dgrad": 0, "dgrad_bnbwd": WANT_BNBWD,
            "dgrad_papply": WANT_PAPPLY}


def plan_wants(dgrad, k):
    """the `want` values fedfr_conv2d_plan admits: the reductions exist for 3x3 convs only"""
    if dgrad:
        return (0, WANT_BNBWD, WANT_PAPPLY) if k == 3 else (0,)
    return (0, WANT_STATS, WANT_MOMENTS, WANT_EPILOGUE) if k == 3 else (0, WANT_STATS, WANT_EPILOGUE)


def plan_expected(B, H, Cin, Cout, k, s, dgrad, want, cus=256, conv_c64p=1, conv28_tpw2=2, nt_glds=4, dgrad_parity=2):
    """what fedfr_conv2d_plan must answer — (profile slot, stat_rows, stat_rows_live, part_rows, out_epilogue) — put together from the
    restated rules above alone.  The row counts are those of the GEMM problem that is launched: a 1x1 dgrad at the output resolution, a
    stride-2 3x3 dgrad under dgrad_parity as one output-parity class (a quarter of the pixels)."""
    Ho = H // s
    stats, bnbwd, mom, pap, epi = (bool(want & b) for b in (WANT_STATS, WANT_BNBWD, WANT_MOMENTS, WANT_PAPPLY, WANT_EPILOGUE))
    fused, par = bnbwd or mom or pap, False
    if not dgrad:
        M, N, C, K, same = B * Ho * Ho, Cout, Cin, k * k * Cin, k == 3 and s == 1
    elif k == 1:
        M, N, C, K, same = B * Ho * Ho, Cin, Cout, Cout, False
    else:
        M, N, C, K, same = B * H * H, Cin, Cout, 9 * Cout, s == 1
        par = s == 2 and dgrad_parity > 0
        M = M // 4 if par else M
    if same:
        slot = conv3x3_slot(M, H, C, N, fused=fused, stats=stats, epilogue=epi, conv_c64p=conv_c64p, nt_glds=nt_glds, bmom=mom or pap)
    else:
        slot = 17 if nt_glds_applies(N, K, par=par, epilogue=epi or fused, nt_glds=nt_glds) else nt_generic_slot(M, N)
    rows = nt_stat_rows(M, N)
    c64p = same and slot == 15 and conv_c64p and C == 64 and N == 64 and not epi           # (with the output epilogue: the LDS-DMA kernel)
    two28 = slot == 13 and conv28_tpw2 and (M // 196) % 2 == 0 and not epi and (conv28_tpw2 >= 2 or (stats and not fused))
    live, part = rows, 0
    if c64p:
        live, part = 2 * conv_c64p_grid(M, cus), conv_c64p_grid(M, cus) if bnbwd else 0
    elif slot in (12, 13) and fused:
        part = M // 196 // (2 if two28 and not stats else 1)
    elif slot in (12, 13):
        live = M // 196 // 2 if two28 else M // 196 * 2
    # out_epilogue is a property of the CHOSEN kernel: a launch that asks for the epilogue gets conv_epilogue_ok; one that does not may run on
    # the persistent 64-channel kernel or the two-tiles 28x28 kernel (both without it: False) — the kernels the dispatch chose for such launches before the plan existed
    out_epi = same and conv_epilogue_ok(H, C, N, M, 3, 1) and not fused and not c64p and not two28
    return slot, rows, live, part, out_epi
