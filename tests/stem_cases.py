"""Inputs and fp64 references for the direct tests of the end of the backward pass: the stem conv (forward, weight gradient plain and
with the BatchNorm + PReLU backward fused in) and the row-slab BatchNorm backward chain (csrc/stem.hip, csrc/bn_rowslab.hip), in the manner of head_cases.py.

Every reference is a plain torch formula evaluated at ``dtype``.  The float64 evaluation is what the kernels are held to
(tests/test_stem_chain_gpu.py); the float32 evaluation is the same formula in the kernels' order of operations (the 16-bit roundings the
kernels make on the way in, hi + lo split of the stem input, per-workgroup partial sums) and tests/test_stem_cases_cpu.py holds it to a
QUARTER of every tolerance.  That file also proves every tolerance tight enough: one row dropped from a column sum, one PReLU mask
flipped, the last pixel omitted, a tap shifted across an image border each move the fp64 reference by more than the tolerance.  Nothing
here imports the oracle.

A reference quantity is a ``Q``: value and an ELEMENT-WISE tolerance, both float64.  Every tolerance is a formula of u16 (the unit
roundoff of the 16-bit storage type: 2^-11 fp16, 2^-8 bf16), 2^-24 and a chain length or a sum of |terms| — none is a measured number.

Conditioning of the inputs (asserted by the CPU test, no element is ever excluded from a comparison):
  * gradients carry the fp16 library's loss scale (256), so that no 16-bit RESULT falls below 2^-11 in magnitude unless it is an exact zero
    (fp16 has no relative precision under 2^-14; elements that would land there get their incoming gradient moved by 1.0);
  * no PReLU pre-activation z = x sc + sh is closer to zero than 1e-3 (offending 16-bit x are moved to the next values that are not),
    except the deliberate exact ties: channel TIE has sc = 1, sh = -0.5 and x = 0.5 in every third row, z == 0, which counts as masked;
  * channel NEG has a negative gamma, channel ZERO gamma == 0 (dx == 0 exactly there).
  * the weight-gradient cases have a few loud pixels (every 64th, the last one, one at an image border) on a background 64 times
    quieter, as gradient maps do: the sum of |terms| the bound is made of then stays small enough for the bound to see ONE pixel.
"""
import math

import torch
import torch.nn.functional as F

f32, f64 = torch.float32, torch.float64
U24 = 2.0 ** -24
GSCALE = 256.0              # the fp16 library's loss scale
ZMIN = 1e-3                 # no |z| below this (ties excepted)
RMIN = 2.0 ** -11           # no 16-bit result below this (exact zeros excepted)
EPS = 1e-5
NEG, ZERO, TIE, NTIE = 1, 2, 3, 5      # special channels
EW_THREADS = 256


def u16(s16):
    return 2.0 ** -11 if s16 == torch.float16 else 2.0 ** -8


def uniform(shape, seed, lo=-1.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g, dtype=f32) * (hi - lo) + lo


def r16(t, s16):
    return t.to(f32).to(s16)


class Q:
    """one reference quantity: value and element-wise tolerance (float64, broadcastable)"""

    def __init__(self, value, tol):
        self.value, self.tol = value.detach().to("cpu", f64), torch.as_tensor(tol).detach().to("cpu", f64)


def err_over_tol(got, q):
    """max over elements of |got - ref| / tol (0 / 0 counts as 0, x / 0 as inf, NaN as inf)"""
    g = got.detach().to("cpu", f64).reshape(q.value.shape)
    e = (g - q.value).abs()
    r = e / q.tol.expand_as(e)
    r = torch.where(e == 0, torch.zeros_like(r), r)
    return float(torch.nan_to_num(r, nan=math.inf).max()) if r.numel() else 0.0


def check(got, q, what, frac=1.0, out=None):
    r = err_over_tol(got, q)
    if out is not None:
        out.append((what, r))
    assert r <= frac, "%s: error is %.3g of its tolerance (allowed %.3g)" % (what, r, frac)


def exceeds(val, q):
    """whether a corrupted reference value lies outside the tolerance somewhere"""
    return err_over_tol(val, q) > 1.0


# ------------------------------------------------------------------------------------------------ geometry (formulas of csrc/bn_rowslab.hip and csrc/stem.hip)
def rows_per_pass(C):
    return EW_THREADS // (C >> 3)


def slab_rows(M, C, max_blocks):
    """bn_rowslab.hip slab_rows: max(8 rpp, ceil(M / max_blocks)) rounded up to a multiple of rpp = 256 / (C / 8)"""
    rpp = rows_per_pass(C)
    rows = max(rpp * 8, -(-M // max_blocks))
    return -(-rows // rpp) * rpp


def colsum_chain(slab, C):
    """longest fp32 addition chain of one workgroup's column sum (ew_block_colsum): rows per thread, then xor-shuffles within the wave and
    4 wave rows in LDS when C / 8 is a power of two <= 64, else rpp rows in LDS; + 2 for the roundings of the term itself"""
    tpr, rpp = C >> 3, rows_per_pass(C)
    shfl = tpr <= 64 and (tpr & (tpr - 1)) == 0
    return slab // rpp + (int(math.log2(64 // tpr)) if shfl else 0) + (EW_THREADS // 64 if shfl else rpp) + 2


def stem_px_per_block(M, sw_px=128):
    """stem.hip stem_px_per_block: ceil(M / 1024) rounded up to whole stages of SW_PX pixels"""
    return max(sw_px, -(-(-(-M // 1024)) // sw_px) * sw_px)


def slab_sum(t, slab, dt):
    """column sum of t [M][C]: float64 plainly, float32 as the kernels do it (one fp32 sum per slab of rows, the slabs added in fp64)"""
    if dt == f64:
        return t.sum(0)
    M = t.shape[0]
    P = -(-M // slab)
    pad = torch.zeros((P * slab - M,) + t.shape[1:], dtype=t.dtype)
    return torch.cat([t, pad]).reshape(P, slab, -1).sum(1).to(f64).sum(0)


def fma(a, b, c, dt):
    """a * b + c with one rounding at float32 (the kernels' contracted form); plain at float64"""
    if dt == f64:
        return a * b + c
    return (a.to(f64) * b.to(f64) + c.to(f64)).to(f32)


def nudge_from_zero(x, sc, sh, s16, keep=None):
    """moves the 16-bit x whose z = x sc + sh lies within ZMIN of zero to the nearest 16-bit values for which it does not (``keep``: a
    mask of deliberate ties left alone)"""
    x = x.clone()
    scd, shd = sc.to(f64), sh.to(f64)
    for k in range(1, 40):
        z = x.to(f64) * scd + shd
        bad = (z.abs() < 1.5 * ZMIN) & (scd != 0)
        if keep is not None:
            bad &= ~keep
        if not bool(bad.any()):
            break
        step = (2.0 * ZMIN * k / scd.abs().clamp_min(1e-30)).expand_as(z)
        away = torch.where(z * scd >= 0, 1.0, -1.0)
        x = torch.where(bad, r16((x.to(f64) + away * step).to(f32), s16), x)
    return x


# ================================================================================================ stem forward
STEM_FWD_SHAPES = [(2, 16), (3, 112), (1, 32), (3, 37), (33, 127)]       # the last two: ragged last tile / second trip of the tile loop


def stem_taps(x, wrap=False):
    """im2col of x [B][3][H][W] (3x3, pad 1) -> [M][27], column k = (kh * 3 + kw) * 3 + ci as the KRSC weights are laid out.  wrap: the
    corruption — tap (kh, kw) = (1, 2) of the pixels in the last column reads the first pixel of the next row instead of the padding"""
    B, _, H, W = x.shape
    col = F.unfold(x, 3, padding=1).reshape(B, 3, 9, H * W).permute(0, 3, 2, 1).reshape(B * H * W, 27).contiguous()
    if wrap:
        nxt = torch.zeros_like(x)
        nxt[:, :, :-1, W - 1] = x[:, :, 1:, 0]
        col = col.clone()
        col[:, 15:18] += nxt.permute(0, 2, 3, 1).reshape(-1, 3)
    return col


class StemFwdCase:
    def __init__(self, B, HW, s16):
        self.name, self.B, self.HW, self.M, self.s16 = "stem_fwd[%d,%d]" % (B, HW), B, HW, B * HW * HW, s16
        self.x = uniform((B, 3, HW, HW), 3)
        self.w = uniform((64, 3, 3, 3), 4) * 0.2
        self.w_krsc = self.w.permute(0, 2, 3, 1).contiguous()

    def y(self, dt=f64, wrap=False):
        """conv of the 16-bit-rounded x and w (the kernel rounds both for the MFMA): [M][64]"""
        xr, wr = r16(self.x, self.s16).to(dt), r16(self.w_krsc, self.s16).to(dt)
        return stem_taps(xr, wrap) @ wr.reshape(64, 27).t()

    def y_q(self, y):
        """per pixel row: max_c |got - ref| <= (u16 + 2^-20) max_c |ref|"""
        return Q(y, (u16(self.s16) + 2.0 ** -20) * y.abs().amax(1, keepdim=True))

    def stats_q(self, y16, dt=f64, drop=None):
        """the statistics rows [rows][2][64] of a STORED y: one row per 64 pixels (a wave's share of a 256-pixel tile), pixels beyond M
        count nothing; 64 values are summed, so each row is held to 64 * 2^-24 * sum |terms|.  drop: a pixel left out (corruption)"""
        rows = -(-self.M // 256) * 4
        v = torch.zeros(rows * 64, 64, dtype=dt)
        v[: self.M] = y16.to("cpu", dt)
        if drop is not None:
            v[drop] = 0
        v = v.reshape(rows, 64, 64)
        val = torch.stack([v.sum(1), (v * v).sum(1)], 1)
        vd = v.to(f64)
        return Q(val, 64 * U24 * torch.stack([vd.abs().sum(1), (vd * vd).sum(1)], 1))


# ================================================================================================ stem weight gradient
STEM_WGRAD_SHAPES = [(11, 112), (53, 50), (1, 10)]      # two exact stages per workgroup / ragged last stage + short last workgroup / one ragged stage


def loud_pixels(B, HW):
    M = B * HW * HW
    loud = torch.zeros(M, dtype=torch.bool)
    if M <= 4096:                                       # a short sum sees one pixel anyway; with two loud terms the bf16 hi + lo split (2^-18 of x at worst) alone takes a third of 2^-17
        loud[:] = True
    loud[63::64] = True
    loud[M - 1] = True
    loud[(HW // 2) * HW + HW - 1] = True                # image 0, middle row, last column: the pixel whose right-hand taps are padding
    return loud


class BnParams:
    """per-channel inputs of one BatchNorm (+PReLU) backward over x [M][C]: saved statistics of x, gamma / beta with the special
    channels, slopes, and the forward's (scale, shift) with the exact-tie channel"""

    def __init__(self, x, seed, tie):
        C = x.shape[1]
        xd = x.to(f64)
        self.mean = xd.mean(0).to(f32)
        self.rstd = (1.0 / torch.sqrt(xd.var(0, unbiased=False) + EPS)).to(f32)
        self.gamma = uniform((C,), seed) * 0.2 + 1.0
        self.gamma[NEG] = -self.gamma[NEG]
        self.gamma[ZERO] = 0.0
        self.beta = uniform((C,), seed + 1) * 0.1
        self.beta[ZERO] = 0.05
        self.alpha = uniform((C,), seed + 2) * 0.1 + 0.25
        self.sc = (self.gamma.to(f64) * self.rstd.to(f64)).to(f32)
        self.sh = (self.beta.to(f64) - self.mean.to(f64) * self.sc.to(f64)).to(f32)
        if tie is not None:
            self.sc[tie], self.sh[tie] = 1.0, -0.5


def make_bn(x, seed, tie, keep, s16, prelu):
    """(x, BnParams): with a PReLU, x is first moved off the mask threshold and the statistics are those of the x that is returned"""
    p = BnParams(x, seed, tie)
    if prelu:
        x = nudge_from_zero(x, p.sc, p.sh, s16, keep)
        p = BnParams(x, seed, tie)
    return x, p


def tie_rows(M, C, tie, phase):
    keep = torch.zeros(M, C, dtype=torch.bool)
    keep[phase::3, tie] = True
    return keep


def bn_terms(dy, x, p, alpha, dt):
    """dz = dy prelu'(z) and the three per-element terms of the backward sums (dz | dz xhat | dy z over z <= 0), in the kernel's order"""
    dyv, xv = dy.to(dt), x.to(dt)
    if alpha:
        z = fma(xv, p.sc.to(dt), p.sh.to(dt), dt)
        neg = z <= 0
        dz = torch.where(neg, dyv * p.alpha.to(dt), dyv)
        t2 = torch.where(neg, dyv * z, torch.zeros_like(z))
    else:
        neg, dz, t2 = None, dyv, torch.zeros_like(dyv)
    t1 = dz * (xv - p.mean.to(dt)) * p.rstd.to(dt)       # the kernel multiplies the finished sum by rstd: the same terms
    return dz, neg, (dz, t1, t2)


def bn_coef(S0, S1, p, count):
    """bn_bwd_finalize8_kernel: a = fl32(gamma rstd), A = -a rstd S1 / count, B = a (rstd mean S1 / count - S0 / count)"""
    g, r, mu = p.gamma.to(f64), p.rstd.to(f64), p.mean.to(f64)
    a = (g * r).to(f32).to(f64)
    cb, cc = S0.to(f64) / count, S1.to(f64) / count
    return torch.stack([a, -a * cc * r, a * (cc * r * mu - cb)])


def bn_coef_tol(coef, tS0, tS1, p, count):
    """what the tolerances of the two sums (tS0, tS1) and the fp32 stores leave of coef"""
    g, r, mu = p.gamma.to(f64).abs(), p.rstd.to(f64), p.mean.to(f64).abs()
    a = (g * r)
    return torch.stack([2 * U24 * a, a * r * tS1 / count + 2 * U24 * coef[1].abs(), a * (r * mu * tS1 + tS0) / count + 2 * U24 * (coef[1].abs() * mu + coef[2].abs())])


def bn_dx(coef, dz, x, dt, extra=None):
    """dx = a dz + (A x + B) (+ addend) as the kernels evaluate it, and |a dz| + |A x| + |B| (+ |addend|)"""
    c = coef.to(dt)
    xv = x.to(dt)
    o = fma(c[0], dz, fma(c[1], xv, c[2].expand_as(xv), dt), dt)
    mag = (c[0] * dz).abs().to(f64) + (c[1] * xv).abs().to(f64) + c[2].abs().to(f64)
    if extra is not None:
        o = o + extra.to(dt)
        mag = mag + extra.abs().to(f64)
    return o, mag


def dx_q(o, mag, s16, unconditioned=False):
    """a stored 16-bit dx: u16 |ref| + 2^-22 (|a dz| + |A x| + |B|).  unconditioned: the inputs are another kernel's output, so results below
    2^-14 cannot be kept out; there fp16 rounds to multiples of 2^-24 and u16 |ref| is not its error: half that spacing, 2^-25, is added
    (nothing for bf16, whose exponent range is fp32's)"""
    o = o.to(f64)
    floor = 2.0 ** -25 if (unconditioned and s16 == torch.float16) else 0.0
    return Q(o, u16(s16) * o.abs() + 2.0 ** -22 * mag + floor)


class StemWgradCase:
    """x [B][3][HW][HW] fp32, the gradient wrt the stem's ACTIVATION dy [M][64] (16 bit), the conv output x0 [M][64] (16 bit) and the
    stem's BatchNorm + PReLU.  plain form: the weight gradient of (x, dz) for a given 16-bit dz; fused form: dz = bn_prelu_backward(dy, x0)"""

    def __init__(self, B, HW, s16):
        self.name, self.B, self.HW, self.M, self.s16 = "stem_wgrad[%d,%d]" % (B, HW), B, HW, B * HW * HW, s16
        M = self.M
        self.x = uniform((B, 3, HW, HW), 13)
        self.loud = loud_pixels(B, HW)
        amp = torch.where(self.loud, 1.0, 2.0 ** -6)[:, None] * GSCALE
        self.ppb = stem_px_per_block(M)
        self.nblk = -(-M // self.ppb)
        # longest fp32 chain: (stages per workgroup) x 4 k-steps of 32 pixels, + the nblk partial results of the reduce kernel
        self.L = (self.ppb // 128) * 4 + self.nblk
        self.x0 = r16(uniform((M, 64), 14) * 2 + 0.3, s16)
        self.keep = tie_rows(M, 64, TIE, 0)
        self.x0[self.keep] = 0.5
        self.x0, self.p = make_bn(self.x0, 15, TIE, self.keep, s16, True)
        self.dy = r16(uniform((M, 64), 16) * amp, s16)
        self.slab = slab_rows(M, 64, 512)                 # the reduce pass (kEwReduceBlocks)
        for _ in range(3):                                # keep every stored dz0 away from fp16's subnormals
            o = self.dz0(self.coef()).value
            bad = (o.abs() < 2 * RMIN) & (self.p.gamma != 0)
            if not bool(bad.any()):
                break
            self.dy = torch.where(bad, r16(self.dy.to(f32) + torch.where(self.dy >= 0, 1.0, -1.0), s16), self.dy)

    # ---- the stem's BatchNorm + PReLU backward
    def sums(self, dt=f64):
        _, _, t = bn_terms(self.dy, self.x0, self.p, True, dt)
        return [slab_sum(v, self.slab, dt) for v in t]

    def sums_q(self, dt=f64):
        _, _, t = bn_terms(self.dy, self.x0, self.p, True, f64)
        ch = colsum_chain(self.slab, 64)
        return [Q(s, ch * U24 * v.abs().sum(0) + U24 * s.abs()) for s, v in zip(self.sums(dt), t)]

    def coef(self, dt=f64):
        s = self.sums(dt)
        return bn_coef(s[0], s[1], self.p, float(self.M)).to(f32)

    def coef_q(self, dt=f64):
        s = self.sums_q(f64)
        c = bn_coef(s[0].value, s[1].value, self.p, float(self.M))
        return Q(bn_coef(*self.sums(dt)[:2], self.p, float(self.M)), bn_coef_tol(c, s[0].tol, s[1].tol, self.p, float(self.M)))

    def dz0(self, coef, dt=f64, flip=None):
        """the stored d(conv output) for GIVEN fp32 coefficients (the kernel's own when a kernel is checked).  flip: (px, c) whose mask is inverted"""
        dz, neg, _ = bn_terms(self.dy, self.x0, self.p, True, dt)
        if flip is not None:
            dz = dz.clone()
            dz[flip] = self.dy[flip].to(dt) * (1.0 if bool(neg[flip]) else self.p.alpha[flip[1]].to(dt))
        return dx_q(*bn_dx(coef, dz, self.x0, dt), self.s16)

    # ---- the weight gradient of a given 16-bit dz [M][64]: [64][27] in KRSC order
    def dw(self, dz16, dt=f64, wrap=False, drop=None, extra_sigma=0.0):
        """float64: the plain sum over pixels of dz x col with the fp32 x.  float32: x split into a 16-bit high and low part, one fp32 sum
        per workgroup, the workgroups added in fp64 — the kernel's order.  Tolerance per weight element:
        (2^-17 + L 2^-24) sum |dz col| (+ extra_sigma * u16 * sqrt(sum (dz col)^2) where the operand was rounded to 16 bits on the way)"""
        col = stem_taps(self.x, wrap)
        d = dz16.to("cpu", f64).clone()
        if drop is not None:
            d[drop] = 0
        if dt == f64:
            val = d.t() @ col.to(f64)
        else:
            hi = r16(col, self.s16).to(f32)
            c2 = hi + r16(col - hi, self.s16).to(f32)
            P, n = self.nblk, self.ppb
            dp, cp = torch.zeros(P * n, 64), torch.zeros(P * n, 27)
            dp[: self.M], cp[: self.M] = d.to(f32), c2
            val = torch.bmm(dp.reshape(P, n, 64).transpose(1, 2), cp.reshape(P, n, 27)).to(f64).sum(0)
        ad, ac = dz16.to("cpu", f64).abs(), col.to(f64).abs()
        tol = (2.0 ** -17 + self.L * U24) * (ad.t() @ ac)
        if extra_sigma:
            tol = tol + extra_sigma * u16(self.s16) * torch.sqrt((ad * ad).t() @ (ac * ac))
        return Q(val, tol)

    def plain_dz(self):
        """a 16-bit dz for the plain form: the stored dz0 of the fp64 coefficients"""
        return r16(self.dz0(self.coef()).value.to(f32), self.s16)


# ================================================================================================ row-slab BatchNorm backward
APPLY_BLOCKS, REDUCE_BLOCKS = 768, 512               # kEwBwdApplyBlocks, kEwReduceBlocks


class BnBwdCase:
    """one call of the row-slab chain: variant = 4 alpha | 2 next | 1 add, or 8 (next BatchNorm with a PReLU behind it)"""

    def __init__(self, M, C, variant, s16, up=None, frozen=False, ties=True):
        self.M, self.C, self.variant, self.s16, self.up, self.frozen = M, C, variant, s16, up, frozen
        self.name = "bn_bwd_rowslab[M=%d,C=%d,v=%d%s%s]" % (M, C, variant, ",add_up" if up else "", ",frozen" if frozen else "")
        self.alpha = variant != 8 and bool(variant & 4)
        self.nx_mode = 2 if variant == 8 else (1 if variant & 2 else 0)
        self.has_add = variant != 8 and bool(variant & 1)
        self.count = math.inf if frozen else float(M)
        self.slab_red, self.slab_app = slab_rows(M, C, REDUCE_BLOCKS), slab_rows(M, C, APPLY_BLOCKS)
        self.P_red, self.P_app = -(-M // self.slab_red), -(-M // self.slab_app)
        self.x = r16(uniform((M, C), 21) * 2 + 0.3, s16)
        self.keep = tie_rows(M, C, TIE, 0) if ties else torch.zeros(M, C, dtype=torch.bool)
        if self.alpha:
            self.x[self.keep] = 0.5
        self.x, self.p = make_bn(self.x, 22, TIE if ties else None, self.keep, s16, self.alpha)
        self.dy = r16(uniform((M, C), 25) * GSCALE, s16)
        self.add = r16(uniform((M, C), 26) * GSCALE, s16) if self.has_add else None
        self.add_up = None
        self.extra = None if self.add is None else self.add.to(f64)
        if up:
            B, H, W = up
            assert B * H * W == M and H % 2 == 0 and W % 2 == 0
            self.add_up = r16(uniform((B, H // 2, W // 2, C), 27) * GSCALE, s16)
            e = torch.zeros(B, H, W, C, dtype=f64)
            e[:, ::2, ::2] = self.add_up.to(f64)
            self.extra = e.reshape(M, C) + (0 if self.extra is None else self.extra)
        if self.nx_mode:
            self.nx = r16(uniform((M, C), 28) * 2 - 0.2, s16)
            self.nkeep = tie_rows(M, C, NTIE, 1) if ties else torch.zeros(M, C, dtype=torch.bool)
            if self.nx_mode == 2:
                self.nx[self.nkeep] = 0.5
            self.nx, self.np = make_bn(self.nx, 29, NTIE if ties else None, self.nkeep, s16, self.nx_mode == 2)
        for _ in range(3):
            o = self.dx(self.coef()).value
            bad = (o.abs() < 2 * RMIN) & (self.p.gamma != 0)
            if not bool(bad.any()):
                break
            self.dy = torch.where(bad, r16(self.dy.to(f32) + torch.where(self.dy >= 0, 1.0, -1.0), s16), self.dy)

    def terms(self, dt=f64):
        return bn_terms(self.dy, self.x, self.p, self.alpha, dt)[2]

    def sums(self, dt=f64, drop=None, flip=None):
        dz, neg, t = bn_terms(self.dy, self.x, self.p, self.alpha, dt)
        t = [v.clone() for v in t]
        if drop is not None:
            for v in t:
                v[drop] = 0
        if flip is not None:                              # one mask inverted
            dyv, xv = self.dy[flip].to(dt), self.x[flip].to(dt)
            c = flip[1]
            z = xv * self.p.sc[c].to(dt) + self.p.sh[c].to(dt)
            was = bool(neg[flip])
            nd = dyv if was else dyv * self.p.alpha[c].to(dt)
            t[0][flip], t[1][flip], t[2][flip] = nd, nd * (xv - self.p.mean[c].to(dt)) * self.p.rstd[c].to(dt), (0.0 if was else dyv * z)
        return [slab_sum(v, self.slab_red, dt) for v in t]

    def sums_q(self, dt=f64):
        """dbeta, dgamma, dalpha: (chain of one reduce workgroup) 2^-24 sum |terms| + the fp32 store"""
        ch = colsum_chain(self.slab_red, self.C)
        return [Q(s, ch * U24 * v.abs().sum(0) + U24 * s.abs()) for s, v in zip(self.sums(dt), self.terms(f64))]

    def coef(self, dt=f64):
        s = self.sums(dt)
        return bn_coef(s[0], s[1], self.p, self.count).to(f32)

    def coef_q(self, dt=f64):
        s = self.sums_q(f64)
        c = bn_coef(s[0].value, s[1].value, self.p, self.count)
        return Q(bn_coef(*self.sums(dt)[:2], self.p, self.count), bn_coef_tol(c, s[0].tol, s[1].tol, self.p, self.count))

    def dx(self, coef, dt=f64, flip=None):
        """the stored dx for GIVEN fp32 coefficients"""
        dz, neg, _ = bn_terms(self.dy, self.x, self.p, self.alpha, dt)
        if flip is not None:
            dz = dz.clone()
            dz[flip] = self.dy[flip].to(dt) * (1.0 if bool(neg[flip]) else self.p.alpha[flip[1]].to(dt))
        return dx_q(*bn_dx(coef, dz, self.x, dt, self.extra), self.s16)

    def next_sums_q(self, dx16, dt=f64, drop=None, flip=None):
        """the next BatchNorm's rows summed over the workgroups, of a STORED dx (the kernel reduces what it stored): (sum dz, sum dz xhat,
        sum dx z over z <= 0) with the next PReLU (variant 8), (sum dx, sum dx xhat, 0) without; chain of one apply workgroup"""
        dzn, neg, t = bn_terms(dx16.to("cpu"), self.nx, self.np, self.nx_mode == 2, dt)
        t = [v.clone() for v in t]
        if drop is not None:
            for v in t:
                v[drop] = 0
        if flip is not None:
            d, xv, c = dx16.to("cpu")[flip].to(dt), self.nx[flip].to(dt), flip[1]
            z = xv * self.np.sc[c].to(dt) + self.np.sh[c].to(dt)
            was = bool(neg[flip])
            nd = d if was else d * self.np.alpha[c].to(dt)
            t[0][flip], t[1][flip], t[2][flip] = nd, nd * (xv - self.np.mean[c].to(dt)) * self.np.rstd[c].to(dt), (0.0 if was else d * z)
        ch = colsum_chain(self.slab_app, self.C)
        return [Q(slab_sum(v, self.slab_app, dt), ch * U24 * v.to(f64).abs().sum(0)) for v in t]


def bn_bwd_cases(s16):
    out = [BnBwdCase(3000, 64, v, s16) for v in (2, 3, 6, 7, 8)]            # 12 slabs of 256 rows, the last of 184: unrolled and tail loop
    out += [BnBwdCase(250037, 64, v, s16) for v in (7, 8)]                  # the slab comes from M / 768 (352 rows), not the minimum
    out += [BnBwdCase(1000, 96, v, s16) for v in (3, 8)]                    # rpp = 21: four idle threads, column sum through LDS only
    out += [BnBwdCase(777, 512, v, s16) for v in (6, 8)]                    # rpp = 4, a whole wave per row: no shuffle step
    out += [BnBwdCase(3 * 34 * 34, 64, 8, s16, up=(3, 34, 34)), BnBwdCase(3 * 34 * 34, 64, 2, s16, up=(3, 34, 34))]
    out += [BnBwdCase(3000, 64, 8, s16, frozen=True)]
    return out


# ================================================================================================ the chain as a unit
class ChainCase:
    """first block's bn1 backward (variant 8 with add_up) -> rows -> finalize of the STEM's BatchNorm (coef_only) -> fused stem weight
    gradient, against the float64 gradient of prelu(bn(conv(x))) for the gradient the first step stored.  B = 3, HW = 34."""

    def __init__(self, s16, B=3, HW=34):
        self.B, self.HW, self.M, self.s16 = B, HW, B * HW * HW, s16
        self.first = BnBwdCase(self.M, 64, 8, s16, up=(B, HW, HW), ties=False)     # (sc, sh) are the BatchNorm's own: autograd is the reference
        self.sw = StemWgradCase.__new__(StemWgradCase)
        s = self.sw
        s.name, s.B, s.HW, s.M, s.s16 = "chain[%d,%d]" % (B, HW), B, HW, self.M, s16
        s.x = uniform((B, 3, HW, HW), 13)
        s.ppb = stem_px_per_block(s.M)
        s.nblk = -(-s.M // s.ppb)
        s.L = (s.ppb // 128) * 4 + s.nblk
        s.x0, s.p, s.keep = self.first.nx, self.first.np, self.first.nkeep       # the stem's conv output and BatchNorm ARE the first step's "next"
        s.slab = self.first.slab_app

    def reference(self, g16):
        """float64 autograd of prelu(bn(conv(x))) wrt (conv weight [64][27] KRSC, gamma, beta, alpha) for the stored upstream gradient
        g16 [M][64]; the conv output takes the stored 16-bit values (straight-through), the BatchNorm measures its statistics itself"""
        s = self.sw
        w = torch.zeros(64, 27, dtype=f64, requires_grad=True)
        ga, be, al = (t.to(f64).clone().requires_grad_(True) for t in (s.p.gamma, s.p.beta, s.p.alpha))
        conv = stem_taps(s.x.to(f64)) @ w.t()
        x0 = conv + (s.x0.to(f64) - conv).detach()
        mu, var = x0.mean(0), x0.var(0, unbiased=False)
        z = (x0 - mu) / torch.sqrt(var + EPS) * ga + be
        z = torch.where(self.mask_z() <= 0, z * al, z)      # the forward's own mask, sign of x0 sc + sh (no |z| < 1e-3: the same in every precision)
        z.backward(g16.to("cpu", f64))
        return w.grad, ga.grad, be.grad, al.grad

    def mask_z(self):
        s = self.sw
        return s.x0.to(f64) * s.p.sc.to(f64) + s.p.sh.to(f64)
