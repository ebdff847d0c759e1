"""Inputs, case tables and fp64 references for the direct tests of the row-slab FORWARD BatchNorm passes and the sphnet PReLU passes that ride on
the same mapping (csrc/bn_rowslab.hip: bn_apply_kernel<X2, STATS>, colsum_stage_kernel + bn_finalize8_kernel, prelu_bwd_pass_kernel<ADD>,
prelu_rows_finalize_kernel / _multi_kernel; csrc/ew.hip: bn_eval_coeffs_multi_kernel), in the manner of stem_cases.py, whose helpers (Q, check,
err_over_tol, u16, slab_rows, rows_per_pass, colsum_chain, the conditioning rules ZMIN / RMIN / GSCALE and the special channels NEG / ZERO / TIE)
are used, not copied.

Every reference is a plain torch formula written from the operation's definition and evaluated at float64 (what tests/test_rowslab_fwd_gpu.py
holds the kernels to) or at float32 in the kernels' order of operations (what tests/test_rowslab_cases_cpu.py holds to a QUARTER of every
tolerance, taken before the final store).  No tolerance is a measured number: each is a formula of u16 (2^-11 fp16 / 2^-8 bf16), 2^-24, 2^-53, a
chain length restated from the kernel (and said which loop it mirrors) and a sum of |terms|.  No element is excluded from any comparison.

Geometry restated from bn_rowslab.hip / ew_rowslab.h: a thread owns 8 channels, tpr = C / 8 threads cover a row, rpp = 256 // tpr rows per pass
(256 - rpp tpr threads idle), a workgroup walks one slab = max(8 rpp, ceil(M / max_blocks)) rounded up to rpp rows, kEwUnroll = 4 rows of a thread
are in flight per unrolled trip and the rest go through the remainder loop; workgroup i takes slab xcd_remap(i, grid).

Two tiers for bn_apply.  EXACT: x, x2 are multiples of 1/8 in [-2, 2] and the per-channel operands are powers of two and quarters (PAT: a
negative scale, a zero scale, exact z == 0 ties among them), so every fp32 intermediate is exact in either affine order, with or without fma, y
equals its own 16-bit rounding in BOTH storage types, and every statistics row is an exact sum (the CPU test proves it at the real shapes: all
partial sums are multiples of one quantum and sum |terms| stays below 2^24 quanta).  TOLERANCE: seeded inputs conditioned as in stem_cases (no
|z| < ZMIN except exact zeros, no stored y below fp16's normal range except exact zeros)."""
import math

import torch

import stem_cases as S
from stem_cases import (EPS, EW_THREADS, GSCALE, NEG, RMIN, TIE, U24, ZERO, ZMIN, Q, check, colsum_chain, err_over_tol, exceeds, f32, f64, fma,  # noqa: F401
                        nudge_from_zero, r16, rows_per_pass, slab_rows, tie_rows, u16, uniform)

U53 = 2.0 ** -53
APPLY_BLOCKS, PRELU_BLOCKS = 1024, 512          # max_blocks of ew_bn_apply / ew_prelu_bwd_pass (and kEwReduceBlocks of the legacy two-pass form)
UNROLL = 4                                      # kEwUnroll
FIN_RG, STAGE_S, STAGE_MIN_P = 128, 64, 1025    # fin8_accumulate's row groups; colsum_stage_kernel's slices, taken when P > 1024
MAX_PRELU_FIN, MAX_BN_EVAL = 64, 160            # kMaxPreluFin, kMaxBnEvalEntries
YMIN = 2.0 ** -13                               # no stored forward result below this (fp16 is normal down to 2^-14) unless it is an exact zero
CHANNELS = (8, 24, 64, 96, 512, 2048)
CONST, FAR = 4, 5                               # finalize: a constant channel (variance clamped at 0) and one with |mean| = 32 sigma
MOMENTUM = float(torch.tensor(0.1, dtype=f32))  # the fp32 value the kernel promotes to double
EPS32 = float(torch.tensor(EPS, dtype=f32))


# ================================================================================================ geometry
def geometry(M, C, max_blocks):
    tpr, rpp = C >> 3, rows_per_pass(C)
    slab = slab_rows(M, C, max_blocks)
    grid = -(-M // slab)
    return dict(tpr=tpr, rpp=rpp, idle=EW_THREADS - rpp * tpr, slab=slab, grid=grid, last=M - (grid - 1) * slab)


def trips(rows, rpp):
    """(unrolled trips, remainder trips) of the thread in row 0 of a pass over a slab of ``rows`` rows: the streaming loops of bn_apply_kernel /
    prelu_bwd_pass_kernel (`m + 3 rpp < mend` four rows at a time, then one at a time)"""
    n = -(-rows // rpp)
    return n // UNROLL, n % UNROLL


def xcd_remap(i, nwg):
    """common.h xcd_remap: workgroup i of nwg -> logical slab (XCD x = i % 8 streams a contiguous range of slabs)"""
    q, r, x, loc = nwg >> 3, nwg & 7, i & 7, i >> 3
    return (x * (q + 1) if x < r else r * (q + 1) + (x - r) * q) + loc


def m_kinds(C):
    """the row counts every channel count is run at (slab at its minimum, 8 rpp, for both max_blocks)"""
    rpp = rows_per_pass(C)
    slab, tail = 8 * rpp, 5 * rpp + (rpp + 1) // 2          # the tail: one unrolled trip, a remainder trip and (rpp > 1) a partial pass
    return {"lt_rpp": max(1, rpp - 1), "rem_only": 3 * rpp - 1, "two_trips": 8 * rpp, "slab_plus1": slab + 1, "grid3": 2 * slab + tail,
            "grid9": 8 * slab + tail, "grid13": 12 * slab + tail}


def slab_sums(t, slab, grid, gid=None):
    """[grid][...]: the sum of t [M][...] over each slab's rows, at t's dtype.  gid: another row -> slab assignment (a corruption)"""
    M = t.shape[0]
    if gid is not None:
        return t.new_zeros((grid,) + t.shape[1:]).index_add_(0, gid, t)
    if grid * slab > M:
        t = torch.cat([t, t.new_zeros((grid * slab - M,) + t.shape[1:])])
    return t.reshape((grid, slab) + t.shape[1:]).sum(1)


def slab_sums_kernel(a, b, slab, grid, rpp):
    """[grid][C]: the fp32 column sum of a (b None) or of a b over each slab's rows AS A WORKGROUP FORMS IT: thread row rl adds its rows
    rl, rl + rpp, ... in turn (`s += r`, or the contracted `q += r * r`: one rounding per step), then the rpp partial sums are added in turn"""
    M, C = a.shape
    pad = grid * slab - M

    def shape(t):
        t = t.to(f32)
        if pad:
            t = torch.cat([t, t.new_zeros(pad, C)])
        return t.reshape(grid, slab // rpp, rpp, C)
    a = shape(a)
    b = None if b is None else shape(b)
    acc = torch.zeros(grid, rpp, C, dtype=f32)
    for s in range(slab // rpp):
        acc = acc + a[:, s] if b is None else (a[:, s].to(f64) * b[:, s].to(f64) + acc.to(f64)).to(f32)
    t = torch.zeros(grid, C, dtype=f32)
    for r in range(rpp):
        t = t + acc[:, r]
    return t


def affine(C, seed):
    """per-channel (scale, shift, slope) of a BatchNorm + PReLU as a forward pass holds them (gamma rstd, beta - mean gamma rstd for statistics
    mean 0.3, variance 4/3: those of the x below), with stem_cases' special channels: NEG, ZERO, and TIE (scale 1, shift -0.5)"""
    gamma = uniform((C,), seed) * 0.2 + 1.0
    gamma[NEG] = -gamma[NEG]
    gamma[ZERO] = 0.0
    beta = uniform((C,), seed + 1) * 0.1
    beta[ZERO] = 0.05
    sc = (gamma.to(f64) / math.sqrt(4.0 / 3.0 + EPS)).to(f32)
    sh = (beta.to(f64) - 0.3 * sc.to(f64)).to(f32)
    sc[TIE], sh[TIE] = 1.0, -0.5
    return sc, sh, uniform((C,), seed + 2) * 0.1 + 0.25


def gid_neighbour(M, slab):
    """the first pixel of the second slab counted in the first slab's row"""
    gid = torch.arange(M) // slab
    gid[slab] = 0
    return gid


# ================================================================================================ 1. bn_apply
# operands present (every other pointer is NULL).  sc1 / sh1 / alpha / sc2 / sh2 are each present and absent somewhere; x2 absent = <X2 = false>
VARIANTS = {
    "bn": ("sc1", "sh1"),                               # a BatchNorm alone (bn1 of a block, bn2 in front of the flatten)
    "bn_prelu": ("sc1", "sh1", "alpha"),                # BatchNorm + PReLU (stem, bn2 of a block)
    "sph": ("sh1", "alpha"),                            # sphnet: y = prelu(c + bias)
    "sph_x2": ("sh1", "alpha", "x2"),                   # ... + identity
    "ds": ("sc1", "sh1", "x2", "sc2", "sh2"),           # downsample block: bn3(c2) + bn_ds(d)
    "res": ("sc1", "sh1", "alpha", "x2"),               # BatchNorm + PReLU + identity
    "ident": (),                                        # net_forward on a lone block: statistics of x1, y == x1 bit for bit
    "sc_only": ("sc1", "x2", "sc2"),                    # both shifts NULL
}
K_APPLY = 6     # fp32 roundings of bn_apply_kernel's statement, without fma: x sc1 | + sh1 | alpha * | x2 sc2 | + sh2 | the final add (with fma: 4)

# exact tier: (sc1, sh1, alpha, sc2, sh2) of channel c = PAT[c % 8]; 1 = NEG (negative scales), 2 = ZERO (zero scales), 3 = TIE (z == 0 where x == 0.5)
PAT = [(1.0, 0.25, 0.5, 1.0, -0.5), (-1.0, 0.5, 0.25, -1.0, 0.25), (0.0, -0.25, 0.5, 0.0, 0.5), (1.0, -0.5, 0.5, 1.0, 0.0),
       (2.0, -1.0, 0.5, 0.5, 1.0), (0.5, 0.75, 0.5, 1.0, -0.25), (1.0, 0.0, 1.0, 1.0, 0.0), (-0.5, -0.25, 2.0, -2.0, 0.5)]


def apply_table():
    """(C, kind, M, variant, stats): per channel count every row-count kind with three of the eight variants, rotated so that every variant meets
    every kind and every channel count; + the case whose slab grows past 8 rpp"""
    names, out = list(VARIANTS), []
    for iC, C in enumerate(CHANNELS):
        for k, (kind, M) in enumerate(m_kinds(C).items()):
            for j, v in enumerate(names):
                if (j + k) % 3 == iC % 3:
                    out.append((C, kind, M, v, v == "ident" or (j + k + iC) % 2 == 0))
    out.append((512, "slab_grows", APPLY_BLOCKS * 32 + 1, "bn_prelu", True))
    return out


def nchw_table():
    """(C, hw, B, variant, stats): M = B hw with slab edges inside an image (hw > 1)"""
    out = []
    for C, sizes in ((96, {1: 400, 5: 70, 49: 7}), (512, {1: 70, 5: 15, 49: 3})):
        for hw, B in sizes.items():
            out += [(C, hw, B, "bn", False), (C, hw, B, "res", True), (C, hw, B, "sph_x2", False)]
    return out


APPLY_ERRORS = [(100, 2056), (100, 12), (0, 64)]       # (M, C): C / 8 > 256 threads, C % 8, no rows


class ApplyCase:
    def __init__(self, C, M, variant, stats, s16, exact, seed=101):
        self.C, self.M, self.variant, self.stats, self.s16, self.exact = C, M, variant, stats, s16, exact
        self.name = "bn_apply[%s,M=%d,C=%d,%s%s]" % ("exact" if exact else "tol", M, C, variant, ",stats" if stats else "")
        self.has = set(VARIANTS[variant])
        self.g = geometry(M, C, APPLY_BLOCKS)
        self.chain = self.g["slab"] // self.g["rpp"] + self.g["rpp"] + 2      # bn_apply_kernel: s[j] += over slab / rpp rows, then `for r < rpp: t += red[r W + i]`; + 2: r r and its own term
        x2 = "x2" in self.has
        v = {}
        if exact:
            g = torch.Generator().manual_seed(seed)
            self.x = (torch.randint(-16, 17, (M, C), generator=g).to(f32) / 8).to(s16)
            self.x2 = (torch.randint(-16, 17, (M, C), generator=g).to(f32) / 8).to(s16) if x2 else None
            pat = torch.tensor(PAT, dtype=f32)[torch.arange(C) % 8]
            for i, n in enumerate(("sc1", "sh1", "alpha", "sc2", "sh2")):
                v[n] = pat[:, i].contiguous()
        else:
            alpha = "alpha" in self.has
            x = r16(uniform((M, C), seed) * 2 + 0.3, s16)
            keep = tie_rows(M, C, TIE, 0) if alpha else torch.zeros(M, C, dtype=torch.bool)
            x[keep] = 0.5
            psc, psh, palpha = affine(C, seed + 1)
            sc = psc if "sc1" in self.has else torch.ones(C)
            sh = torch.zeros(C)
            if "sh1" in self.has:
                sh = psh if "sc1" in self.has else uniform((C,), seed + 4) * 0.5
                sh[TIE] = -0.5
            if alpha:
                assert float(sc[TIE]) == 1.0 and float(sh[TIE]) == -0.5
            self.x = nudge_from_zero(x, sc, sh, s16, keep)         # (with or without a PReLU: y = z there, and a stored y keeps away from fp16's subnormals)
            v.update(sc1=sc, sh1=sh, alpha=palpha)
            self.x2 = None
            if x2:
                self.x2 = r16(uniform((M, C), seed + 5) * 2 - 0.2, s16)
                sc2, sh2, _ = affine(C, seed + 6)
                sc2[TIE], sh2[TIE] = 0.75, 0.125
                v.update(sc2=sc2 if "sc2" in self.has else torch.ones(C), sh2=sh2 if "sh2" in self.has else torch.zeros(C))
        self.op = {n: (v[n].to(f32).contiguous() if n in self.has else None) for n in ("sc1", "sh1", "alpha", "sc2", "sh2")}
        if not exact and x2:
            for _ in range(4):                                    # cancellation of the two branches: keep the stored sum out of fp16's subnormals
                y = self.y()[0]
                bad = (y.abs() < 2 * RMIN) & (y != 0)
                if not bool(bad.any()):
                    break
                self.x2 = torch.where(bad, r16(self.x2.to(f32) + 0.25, s16), self.x2)

    def eff(self, n, dt):
        dflt = 1.0 if n in ("sc1", "sc2") else 0.0
        return self.op[n].to(dt) if self.op[n] is not None else torch.full((self.C,), dflt, dtype=dt)

    def z(self, dt=f64):
        return fma(self.x.to(dt), self.eff("sc1", dt), self.eff("sh1", dt), dt)

    def parts(self, dt=f64):
        """(z, prelu(z), x2 sc2 + sh2 or None)"""
        z = self.z(dt)
        a = z if self.op["alpha"] is None else torch.where(z > 0, z, self.op["alpha"].to(dt) * z)
        w = None if self.x2 is None else fma(self.x2.to(dt), self.eff("sc2", dt), self.eff("sh2", dt), dt)
        return z, a, w

    def y(self, dt=f64, flip=None, neighbour_slope=False, bias_after=False):
        """(y before the 16-bit store, |x sc1| + |sh1| + |x2 sc2| + |sh2|).  Corruptions: flip = (m, c) whose PReLU mask is inverted;
        the slopes of channel c + 1; the shift added behind the PReLU"""
        z, a, w = self.parts(dt)
        if self.op["alpha"] is not None:
            al = self.op["alpha"].to(dt)
            if neighbour_slope:
                al = al.roll(-1)
            if bias_after:
                z0 = self.x.to(dt) * self.eff("sc1", dt)
                a = torch.where(z0 > 0, z0, al * z0) + self.eff("sh1", dt)
            else:
                a = torch.where(z > 0, z, al * z)
            if flip is not None:
                a = a.clone()
                a[flip] = al[flip[1]] * z[flip] if bool(z[flip] > 0) else z[flip]
        o = a if w is None else a + w
        mag = (self.x.to(f64) * self.eff("sc1", f64)).abs() + self.eff("sh1", f64).abs()
        if w is not None:
            mag = mag + (self.x2.to(f64) * self.eff("sc2", f64)).abs() + self.eff("sh2", f64).abs()
        return o, mag

    def y_q(self, **kw):
        o, mag = self.y(f64, **kw)
        return Q(o, u16(self.s16) * o.abs() + K_APPLY * U24 * mag)

    def stats_q(self, y16, dt=f64, drop=None, gid=None):
        """rows [grid][2][C] of a STORED y (the kernel unpacks what it packed): sum r | sum r r over each slab's rows"""
        v = y16.to("cpu", dt)
        if drop is not None:
            v = v.clone()
            v[drop] = 0
        g = self.g
        if dt == f32:
            val = torch.stack([slab_sums_kernel(v, None, g["slab"], g["grid"], g["rpp"]), slab_sums_kernel(v, v, g["slab"], g["grid"], g["rpp"])], 1)
        else:
            val = torch.stack([slab_sums(v, g["slab"], g["grid"], gid), slab_sums(v * v, g["slab"], g["grid"], gid)], 1)
        vd = y16.to("cpu", f64)
        return Q(val, self.chain * U24 * torch.stack([slab_sums(vd.abs(), g["slab"], g["grid"]), slab_sums(vd * vd, g["slab"], g["grid"])], 1))


def nchw(y, hw, swap=None):
    """[B hw][C] -> the flatten order [B][C][hw] bn_apply_kernel stores with nchw_hw = hw.  swap = pixel whose image index is exchanged with the next image's (corruption)"""
    B, C = y.shape[0] // hw, y.shape[1]
    t = y.reshape(B, hw, C).permute(0, 2, 1).contiguous()
    if swap is not None:
        t[0, :, swap], t[1, :, swap] = t[1, :, swap].clone(), t[0, :, swap].clone()
    return t


# ================================================================================================ 2. bn_finalize
FIN_P = (1, 2, 127, 128, 129, 255, 256, 257, 1024, 1025, 2048, 2049, 4097)
FIN_C = (8, 24, 64, 512)
FIN_NULLS = ((), ("gamma",), ("beta",), ("running",), ("gamma", "beta", "running"))
BENCH_COUNT = 128 * 112 * 112


def finalize_table():
    """(P, C, count kind, null operands)"""
    out = []
    for iP, P in enumerate(FIN_P):
        for iC, C in enumerate(FIN_C):
            out.append((P, C, "large" if (iP + iC) % 4 == 3 else "M", FIN_NULLS[(iP + 2 * iC) % 5]))
    out += [(1, 8, "one", ()), (1, 64, "one", ("gamma",))]
    return out


def fin_chain64(P):
    """longest fp64 addition chain of fin8_accumulate: two adds per trip of `r += 2 FIN_RG`, 16 LDS entries per lane, 3 xor steps; + 3 for ic, the product and the difference"""
    return 2 * -(-P // (2 * FIN_RG)) + FIN_RG // 8 + 3 + 3


def make_distinct(rows, fixed):
    """rows [P][nv][C] with the few fp32 values that coincide within a column moved up by one ulp each (channel ``fixed`` is left alone: a
    constant input's rows repeat), so that no two rows of a column can be exchanged unnoticed"""
    rows = rows.clone()
    inf = torch.tensor(float("inf"))
    for _ in range(16):
        srt, idx = rows.sort(0)
        dup = srt[1:] == srt[:-1]
        dup[:, :, fixed] = False
        if not bool(dup.any()):
            break
        mask = torch.zeros_like(rows, dtype=torch.bool).scatter_(0, idx[1:], dup)
        rows = torch.where(mask, torch.nextafter(rows, inf), rows)
    return rows


class FinalizeCase:
    """rows [P][2][C] are the INPUT: fp64 (sum x, sum x x) over uneven row ranges (1, 2, 3, 1, ... pixels) of an fp64 x, rounded to fp32 once"""

    def __init__(self, P, C, count_kind="M", null=(), seed=201):
        self.P, self.C, self.null = P, C, set(null)
        self.name = "bn_finalize[P=%d,C=%d,count=%s,null=%s]" % (P, C, count_kind, "+".join(null) or "-")
        sizes = 1 + torch.arange(P) % 3
        M = int(sizes.sum())
        x = (uniform((M, C), seed) * math.sqrt(3.0)).to(f64) + (uniform((C,), seed + 1) * 0.5).to(f64)       # sigma = 1
        x[:, CONST] = 0.5
        x[:, FAR] += 32.0
        seg = torch.repeat_interleave(torch.arange(P), sizes)
        self.rows64 = torch.stack([torch.zeros(P, C, dtype=f64).index_add_(0, seg, x), torch.zeros(P, C, dtype=f64).index_add_(0, seg, x * x)], 1)
        self.rows = make_distinct(self.rows64.to(f32), CONST)
        self.M = M
        self.count = {"M": float(M), "one": 1.0, "large": float(BENCH_COUNT)}[count_kind]
        assert self.count >= M
        self.gamma = uniform((C,), seed + 2) * 0.2 + 1.0
        self.gamma[NEG] = -self.gamma[NEG]
        self.gamma[ZERO] = 0.0
        self.beta = uniform((C,), seed + 3) * 0.1
        self.rm0, self.rv0 = uniform((C,), seed + 4) * 0.1, uniform((C,), seed + 5) * 0.2 + 1.0
        self.staged = P >= STAGE_MIN_P

    def sums(self, order="plain", drop_row=None, drop_slice=None):
        """(S, Q, stage term of S, stage term of Q): fp64 column sums of the fp32 rows.  order = "kernel": as the launches add them (P > 1024: slice
        s = rows s, s + 64, ... summed in fp64 and rounded to fp32 ONCE by colsum_stage_kernel, then the 64 slices in fp64; else the rows reversed)"""
        r = self.rows.to(f64)
        if drop_row is not None:
            r = r.clone()
            r[drop_row] = 0
        zero = torch.zeros(self.C, dtype=f64)
        if not self.staged:
            t = (r.flip(0) if order == "kernel" else r).sum(0)
            return t[0], t[1], zero, zero
        sl = torch.zeros(STAGE_S, 2, self.C, dtype=f64).index_add_(0, torch.arange(self.P) % STAGE_S, r)
        if drop_slice is not None:
            sl[drop_slice] = 0
        term = U24 * sl.abs().sum(0)
        t = sl.to(f32).to(f64).sum(0) if order == "kernel" else sl.sum(0)
        return t[0], t[1], term[0], term[1]

    def outputs(self, order="plain", biased=False, **kw):
        """the six outputs {name: Q} from bn_math.h's expressions (bn_fwd_coef, bn_running_update) at float64, BEFORE the fp32 store"""
        Ssum, Qsum, dS, dQ = self.sums(order, **kw)
        C, count, ic = self.C, self.count, 1.0 / self.count
        g = torch.ones(C, dtype=f64) if "gamma" in self.null else self.gamma.to(f64)
        b = torch.zeros(C, dtype=f64) if "beta" in self.null else self.beta.to(f64)
        mean = Ssum * ic
        ex2 = Qsum * ic
        var = (ex2 - mean * mean).clamp_min(0.0)
        rstd = 1.0 / torch.sqrt(var + EPS32)
        unb = var if (biased or count <= 1.0) else var * count / (count - 1.0)
        val = dict(scale=g * rstd, shift=b - mean * g * rstd, mean=mean, rstd=rstd)
        # first order: d mean, d var (fp64 chain on sum | sumsq ic + mean^2, + the staged slices' single fp32 rounding), d rstd = rstd^3 d var / 2 (+ 4 ulp: two Newton steps)
        c64 = fin_chain64(STAGE_S if self.staged else self.P) * U53
        dmean = c64 * mean.abs() + dS * ic
        dvar = c64 * (ex2 + mean * mean) + dQ * ic + 2 * mean.abs() * dS * ic
        drstd = 0.5 * rstd ** 3 * dvar + 4 * U53 * rstd
        tol = dict(scale=g.abs() * drstd, shift=g.abs() * (mean.abs() * drstd + rstd * dmean) + 2 * U53 * (b.abs() + (mean * g * rstd).abs()),
                   mean=dmean, rstd=drstd)
        if "running" not in self.null:
            val["rm"] = (1.0 - MOMENTUM) * self.rm0.to(f64) + MOMENTUM * mean
            val["rv"] = (1.0 - MOMENTUM) * self.rv0.to(f64) + MOMENTUM * unb
            f = 1.0 if count <= 1.0 else count / (count - 1.0)
            tol["rm"] = MOMENTUM * dmean + 2 * U53 * val["rm"].abs()
            tol["rv"] = MOMENTUM * f * dvar + 2 * U53 * val["rv"].abs()
        # what the staged slices' rounding allows on the 32 sigma channel, in units of the value's own fp32 store
        self.stage_over_store = {n: float(tol[n][FAR] / (U24 * val[n][FAR].abs())) for n in val} if self.staged else {}
        return {n: Q(val[n], tol[n] + U24 * val[n].abs()) for n in val}        # + the fp32 store of the value


def exact_fin_rows(P, C, seed=251):
    """rows whose every partial sum is an exact fp64 integer: the six outputs cannot depend on the order of the rows"""
    g = torch.Generator().manual_seed(seed)
    s = torch.randint(-8, 9, (P, C), generator=g)
    return torch.stack([s, s * s + torch.randint(1, 9, (P, C), generator=g)], 1).to(f32)


def stem_stat_rows(B, H, W):
    """stem.hip ew_stem_stat_rows"""
    return -(-(B * H * W) // 256) * 4


# ================================================================================================ 3. prelu_bwd_pass
def prelu_table():
    """(C, kind, M, add, bias): two of the four operand forms per shape, all four per channel count; + the case whose slab grows"""
    out = []
    for iC, C in enumerate(CHANNELS):
        for k, (kind, M) in enumerate(m_kinds(C).items()):
            a, b = (k + iC) % 2 == 0, (k // 2 + iC) % 2 == 0
            out += [(C, kind, M, a, b), (C, kind, M, not a, not b)]
    out.append((512, "slab_grows", PRELU_BLOCKS * 32 + 1, True, True))
    return out


LEGACY_TABLE = [(64, 2 * 256 + 176, True), (96, 2 * 168 + 116, False), (512, 77, True)]     # (C, M, bias): fedfr_bias_prelu_bwd


class PreluCase:
    """g = dy (+ add, rounded to 16 bits); z = x + bias; dz = g (z > 0 ? 1 : alpha); rows = (sum of the unrounded dz | sum g z over z <= 0) per slab"""

    def __init__(self, C, M, add, bias, s16, seed=301):
        self.C, self.M, self.s16 = C, M, s16
        self.name = "prelu_bwd_pass[M=%d,C=%d%s%s]" % (M, C, ",add" if add else "", ",bias" if bias else "")
        self.g = geometry(M, C, PRELU_BLOCKS)
        self.chain = colsum_chain(self.g["slab"], C)        # ew_block_colsum: the shuffle form when C / 8 is a power of two <= 64, else rpp rows in LDS (C = 24, 96, 2048)
        self.bias = None
        if bias:
            self.bias = uniform((C,), seed + 1) * 0.5
            self.bias[TIE] = -0.5
        self.alpha = uniform((C,), seed + 2) * 0.1 + 0.25
        x = r16(uniform((M, C), seed) * 2 + 0.3, s16)
        self.keep = tie_rows(M, C, TIE, 0)
        x[self.keep] = 0.5 if bias else 0.0
        self.x = nudge_from_zero(x, torch.ones(C), self.bias if bias else torch.zeros(C), s16, self.keep)
        self.dy = r16(uniform((M, C), seed + 3) * GSCALE, s16)
        self.add = r16(uniform((M, C), seed + 4) * GSCALE, s16) if add else None
        for _ in range(4):                                  # no stored dz in fp16's subnormals
            o = self.dz_q(self.gsum()).value
            bad = (o.abs() < 2 * RMIN) & (o != 0)
            if not bool(bad.any()):
                break
            self.dy = torch.where(bad, r16(self.dy.to(f32) + torch.where(self.dy >= 0, 1.0, -1.0), s16), self.dy)

    def gsum(self):
        """what the ADD pass stores: the fp32 sum rounded to 16 bits (bit for bit); dy itself without an addend"""
        return self.dy if self.add is None else (self.dy.float() + self.add.float()).to(self.s16)

    def terms(self, g16, dt=f64, flip=None, tie_positive=False, bias_after=False, neighbour_slope=False, dalpha_positive=False):
        """(dz, g z over z <= 0) per element from a STORED g.  Corruptions: one mask inverted | z < 0 instead of z <= 0 | the mask taken from x
        alone | the slopes of channel c + 1 | the slope gradient gathered over z > 0"""
        g, x = g16.to("cpu", dt), self.x.to(dt)
        z = x if self.bias is None else x + self.bias.to(dt)
        neg = (x <= 0) if bias_after else ((z < 0) if tie_positive else (z <= 0))
        if flip is not None:
            neg = neg.clone()
            neg[flip] = ~neg[flip]
        al = self.alpha.to(dt)
        if neighbour_slope:
            al = al.roll(-1)
        dz = torch.where(neg, g * al, g)
        gz = torch.where(~neg if dalpha_positive else neg, g * z, torch.zeros_like(z))
        return dz, gz

    def dz_q(self, g16, dt=f64, **kw):
        dz = self.terms(g16, dt, **kw)[0]
        d = dz.to(f64)
        return Q(dz, u16(self.s16) * d.abs() + 2 * U24 * d.abs())

    def rows_q(self, g16, dt=f64, drop=None, gid=None, **kw):
        """rows [grid][2][C]"""
        t = [v.clone() for v in self.terms(g16, dt, **kw)]
        if drop is not None:
            for v in t:
                v[drop] = 0
        s, n = self.g["slab"], self.g["grid"]
        if dt == f32:                                       # dz is rounded, then added; g z is contracted into the accumulation
            x = self.x.to(f32)
            z = x if self.bias is None else x + self.bias
            gm = torch.where(z <= 0, g16.to("cpu", f32), torch.zeros_like(z))
            val = torch.stack([slab_sums_kernel(t[0], None, s, n, self.g["rpp"]), slab_sums_kernel(gm, z, s, n, self.g["rpp"])], 1)
        else:
            val = torch.stack([slab_sums(v, s, n, gid) for v in t], 1)
        mag = torch.stack([slab_sums(v.abs(), s, n) for v in self.terms(g16, f64)], 1)
        return Q(val, self.chain * U24 * mag)

    def grads_q(self, g16):
        """dbias, dalpha of the legacy two-pass form: its reduce rows (the same slabs: kEwReduceBlocks = 512) added in fp64, + the fp32 store"""
        q = self.rows_q(g16)
        v, t = q.value.sum(0), q.tol.sum(0)
        return Q(v[0], t[0] + U24 * v[0].abs()), Q(v[1], t[1] + U24 * v[1].abs())


# ================================================================================================ 4. prelu_bwd_finalize (+ multi)
PFIN_P = (1, 2, 127, 128, 129, 255, 256, 257, 600)
PFIN_C = (8, 64, 512)


def prelu_rows(P, C, nv=2, seed=401):
    """input rows [P][nv][C]: pairwise different; the third statistic of a fused dgrad epilogue's rows is never read: NaN"""
    r = uniform((P, nv, C), seed + 7 * P + C) * GSCALE
    if nv == 3:
        r[:, 2] = float("nan")
    return r


def prelu_fin_q(rows):
    """(dbias, dalpha): the fp64 sum of the rows, one fp32 rounding, + 2^-53 P sum |rows| for the fp64 additions"""
    P = rows.shape[0]
    r = rows[:, :2].to(f64)
    v, mag = r.sum(0), r.abs().sum(0)
    return [Q(v[i], U24 * v[i].abs() + U53 * P * mag[i]) for i in range(2)]


def multi_tables():
    """{name: [(P, C, nv_row, has dbias)]}"""
    Cs, Ps = (8, 64, 8, 512, 24, 8, 96, 64), (1, 2, 127, 128, 129, 256, 257, 300, 5)
    big = [(Ps[i % len(Ps)], Cs[i % len(Cs)], 3 if i % 5 == 2 else 2, i % 3 != 1) for i in range(MAX_PRELU_FIN)]
    return {"n1": [(129, 64, 2, True)], "n2": [(255, 8, 2, True), (3, 512, 3, False)], "n64": big}


class MultiLayout:
    """one `base` byte range holding every entry's rows (16-byte aligned, NaN in between) and one `grads` float range with NaN guard bands"""

    def __init__(self, entries, seed=451):
        self.entries = entries
        self.rows, self.rows_off, self.dbias_off, self.dalpha_off = [], [], [], []
        nb, ng = 4, 8                                        # floats
        for i, (P, C, nv, has_b) in enumerate(entries):
            self.rows.append(prelu_rows(P, C, nv, seed + i))
            self.rows_off.append(nb * 4)
            nb += P * nv * C + 4 * (1 + i % 3)
            if has_b:
                self.dbias_off.append(ng)
                ng += C + 8
            else:
                self.dbias_off.append(-1)
            self.dalpha_off.append(ng)
            ng += C + 8 * (1 + i % 2)
        self.base = torch.full((nb,), float("nan"), dtype=f32)
        for r, off in zip(self.rows, self.rows_off):
            self.base[off // 4: off // 4 + r.numel()] = r.reshape(-1)
        self.n_grads = ng
        self.named = torch.zeros(ng, dtype=torch.bool)
        for (P, C, nv, has_b), bo, ao in zip(entries, self.dbias_off, self.dalpha_off):
            if has_b:
                self.named[bo: bo + C] = True
            self.named[ao: ao + C] = True

    def blocks(self):
        """(blk0, blocks) as net_sph.inc fin_add fills PreluFinTable: C / 8 workgroups per entry, in order"""
        b0, out = 0, []
        for P, C, nv, has_b in self.entries:
            out.append(b0)
            b0 += C // 8
        return out, b0


# ================================================================================================ 5. bn_eval_coeffs
EVAL_C = (8, 64, 264, 520)          # 264: the second blockIdx.y; 520: the second trip of the grid-stride loop (2 x 256 channels per trip)
K_EVAL = dict(rstd=3, scale=4, shift=6)   # fp32 roundings: rv + eps | sqrtf | 1 / . ; * g ; shift: those, rm g, the product, the final add — on |b| + |rm g rstd|


class EvalCase:
    def __init__(self, n, seed=501):
        self.n = n
        self.C = [EVAL_C[(i + n) % 4] for i in range(n)] if n > 1 else [520]
        self.name = "bn_eval_coeffs[n=%d]" % n
        self.g_off, self.b_off, self.rm_off, self.rv_off, self.save_off = [], [], [], [], []
        npar, nbuf, nsave = 3, 5, 8
        for i, C in enumerate(self.C):
            if i % 3 == 1:
                self.g_off.append(-1)                           # weight reads as 1
            else:
                self.g_off.append(npar)
                npar += C
            self.b_off.append(npar)
            npar += C + i % 2
            self.rm_off.append(nbuf)
            self.rv_off.append(nbuf + C)
            nbuf += 2 * C + 1
            self.save_off.append(nsave)
            nsave += 4 * C + 8
        self.params = uniform((npar,), seed) * 0.5 + torch.where(torch.arange(npar) % 7 == 0, -1.0, 1.0)       # weights and biases of both signs
        self.bufs = uniform((nbuf,), seed + 1)
        self.n_save = nsave
        self.named = torch.zeros(nsave, dtype=torch.bool)
        for i, C in enumerate(self.C):
            rv = 10.0 ** (uniform((C,), seed + 2 + i) * 4.5 - 1.5)                # 1e-6 ... 1e3
            rv[0], rv[-1] = 1e-6, 1e3
            self.bufs[self.rv_off[i]: self.rv_off[i] + C] = rv
            self.named[self.save_off[i]: self.save_off[i] + 4 * C] = True

    def entry(self, i, dt=f64):
        """(scale, shift, mean, rstd) of entry i as {name: Q}: float64 of the stated fp32 expressions; dt = float32: the expressions in fp32"""
        C = self.C[i]
        rv, rm = self.bufs[self.rv_off[i]: self.rv_off[i] + C].to(dt), self.bufs[self.rm_off[i]: self.rm_off[i] + C].to(dt)
        g = torch.ones(C, dtype=dt) if self.g_off[i] < 0 else self.params[self.g_off[i]: self.g_off[i] + C].to(dt)
        b = self.params[self.b_off[i]: self.b_off[i] + C].to(dt)
        eps = torch.tensor(EPS32, dtype=dt)
        rstd = 1.0 / torch.sqrt(rv + eps)
        scale = g * rstd
        shift = b - rm * g * rstd
        d = lambda t: t.to(f64)     # noqa: E731
        return dict(scale=Q(scale, K_EVAL["scale"] * U24 * d(scale).abs()), shift=Q(shift, K_EVAL["shift"] * U24 * (d(b).abs() + d(rm * g * rstd).abs())),
                    mean=Q(rm, torch.zeros(C, dtype=f64)), rstd=Q(rstd, K_EVAL["rstd"] * U24 * d(rstd)))
