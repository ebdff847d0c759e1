"""Inputs, geometry mirror and fp64 references for the direct tests of the channel-sliced BatchNorm passes (csrc/bn_sliced.hip) behind
fedfr_bn_apply_sliced, fedfr_bn_apply2_sliced and fedfr_bn_bwd_sliced, in the manner of stem_cases.py, whose ``Q`` / ``check`` machinery,
parameter builders and BatchNorm-backward formulas are imported, not repeated.

Every reference is a plain torch formula evaluated at ``dtype``: float64 is what the kernels are held to (tests/test_bn_sliced_gpu.py),
float32 is the same formula in the kernels' order of operations (16-bit inputs, per-thread accumulation over the passes of a pixel group,
the xor-shuffle / wave tree, fp64 fan-in of fp32 rows, fp32 coefficient stores, contracted fma forms of bn_math.h) and
tests/test_bn_sliced_cases_cpu.py holds it to a QUARTER of every tolerance; that file also shows every tolerance tight (a row dropped,
doubled or clamped wrongly, a pixel lost or attributed to the neighbouring group, a flipped mask, count - 1, a biased running variance,
a dropped covariance, the wrong statistic, the neighbour's slope).  Nothing here imports the GPU library or the oracle.

THE STATISTICS OF AN OPERATION ARE THE SUM OF THE PARTIAL ROWS IT IS GIVEN.  The rows are an input: fp64 column sums of distinct, uneven
row ranges of the tensor, rounded once to fp32 (``partial_rows``), then made pairwise different in every channel and statistic
(``make_distinct``: equal values, e.g. of one-pixel rows, are moved by multiples of 2^-22 of the largest).  The reference sums those fp32
rows in fp64, so a producer's error never enters a tolerance and every single row counts.

Tolerances (element-wise, none a measured number):
  * a coefficient the kernel derives in fp64 from given rows and stores as fp32: COEF_ULPS 2^-24 of its own magnitude — of the magnitudes of
    the terms that cancel for shift, B, the derived mean / variance and the running statistics.  Derivation: everything up to the store is fp64
    (error ~2^-52 of those magnitudes), the store rounds by at most 2^-24 |v|, and the QUARTER rule of the CPU test then asks for 4;
  * a sum a workgroup accumulates in fp32: chain 2^-24 sum |terms|, chain = passes per thread (ceil(ppg / 64)) + 4 xor-shuffle steps + the 4
    wave rows + the roundings of the term itself (``*_CHAIN_EXTRA``);
  * a stored 16-bit result: stem_cases.dx_q, u16 |ref| + 2^-22 sum |terms|, for coefficients that are GIVEN (the kernel's own scale / shift
    where it returns them; where it does not — the backward pass — the fp32 rounding of the fp64 coefficients of the given rows, and one unit
    in the last place of each, stem_cases.bn_coef_tol with exact sums, is added through |dz|, |x| and 1).

Conditioning (asserted by the CPU test, no element is ever excluded): stem_cases' rules (loss scale on gradients, no |z| under ZMIN but for
exact ties, no 16-bit result under RMIN unless exactly 0) and the special channels NEG (gamma < 0), ZERO (gamma == 0), TIE (backward only,
where (sc, sh) are inputs: sc = 1, sh = -0.5, x = 0.5 in every third pixel), CONST (x == 0.5 in every pixel; its rows carry fractional
pixel counts so that they differ, and the first row's sum of squares is lowered by 2^-10 so that E[x^2] - mean^2 < 0: the variance must
clamp at 0, rstd = 1 / sqrt(eps)) and BIG (|mean| = 32 standard deviations: x sc + sh and E[x^2] - mean^2 cancel).

Not reachable through the C ABI: the frozen-BatchNorm form of the backward pass (count = HUGE_VAL, set by net.hip) — fedfr_bn_bwd_sliced
fixes count = M.  It stays with test_freeze_bn_vs_reference (tests/test_e2e_gpu.py).
"""
import torch

from stem_cases import (NEG, TIE, ZERO, GSCALE, RMIN, ZMIN, U24, BnParams, Q, bn_coef, bn_coef_tol, bn_dx, bn_terms, check,  # noqa: F401
                        dx_q, err_over_tol, exceeds, f32, f64, fma, make_bn, nudge_from_zero, r16, tie_rows, u16, uniform)

CONST, BIG = 4, 6                                    # further special channels (stem_cases: NEG, ZERO, TIE = 1, 2, 3)
CONST_X, CONST_BETA = 0.5, 0.0625
COEF_ULPS = 4
MOM = float(torch.tensor(0.1, dtype=f32))            # the ABI takes momentum and eps as float
EPSF = float(torch.tensor(1e-5, dtype=f32))

# ------------------------------------------------------------------------------------------------ geometry (formulas of csrc/bn_sliced.hip)
SW, NTH, PXP = 32, 256, 64                           # channels per slice, threads, pixels per pass
MAX_PASSES, BWD_PASSES = 13, 26                      # kMaxPasses, g_bn_sliced_bwd_passes
RG = {2: 16, 3: 10}                                  # FanIn<NV>::RG = 256 / (8 NV): row groups of the fan-in
FL_FWD, FL_BWD2, FL_BWD3 = 16, 8, 13                 # kFwdFL, kBwdFL2, kBwdFL3: rows per thread (wide: twice)
NARROW = {"fwd": FL_FWD * RG[2], "bwd2": FL_BWD2 * RG[2], "bwd3": FL_BWD3 * RG[3]}       # 256, 128, 130
NPRE, UAPPLY = 3, 2                                  # backward apply: passes in flight before the prologue, then chunks of two
SUM_TREE = 4 + 4                                     # xor-shuffle steps 4, 8, 16, 32 and the four wave rows (counted as stem_cases.colsum_chain counts them)


def sliced_geometry(M, C, backward=False):
    """(G, ppg): pixel groups and pixels per group"""
    g = max(1, 256 // (C // SW))
    per = -(-(-(-M // g)) // 8) * 8
    per = min(per, (BWD_PASSES if backward else MAX_PASSES) * PXP)
    return -(-M // per), per


def sliced_ok(M, C, P, backward=False):
    if C < 64 or C > 1024 or C % SW or M < 256:
        return False
    if M * C > 14 * 1000 * 1000 or M > 128 * MAX_PASSES * PXP:
        return False
    return 0 < P <= (2 * NARROW["bwd2"] if backward else NARROW["fwd"])


def apply2_ok(M, C, P):
    return sliced_ok(M, C, 1) and 0 < P <= 2 * NARROW["bwd3"]


def xcd_remap(i, nwg):
    q, r, x, loc = nwg >> 3, nwg & 7, i & 7, i >> 3
    return (x * (q + 1) if x < r else r * (q + 1) + (x - r) * q) + loc


def passes(ppg):
    return -(-ppg // PXP)


def fwd_np(ppg):
    return 7 if ppg <= 7 * PXP else MAX_PASSES


def apply_variant(M, C, x2):
    return "bn_apply_s<NP=%d,X2=%d>" % (fwd_np(sliced_geometry(M, C)[1]), int(bool(x2)))


def apply2_variant(M, C, P):
    return "bn_apply2_s<NP=%d,FL=%d>" % (fwd_np(sliced_geometry(M, C)[1]), FL_BWD3 * (2 if P > NARROW["bwd3"] else 1))


def bwd_variant(P, alpha, nx, add):
    """(variant number 4 alpha | 2 next | 1 add, FX, name) of bn_bwd_apply_s_kernel"""
    v = (4 if alpha else 0) | (2 if nx else 0) | (1 if add else 0)
    fx = 2 if P > NARROW["bwd3" if alpha else "bwd2"] else 1
    return v, fx, "bn_bwd_apply_s<v=%d(%s),FX=%d>" % (v, ",".join(n for n, f in (("alpha", alpha), ("next", nx), ("add", add)) if f) or "plain", fx)


def bwd_apply_chunks(ppg):
    """chunks of UAPPLY passes the backward apply pass streams after its NPRE prefetched passes"""
    return -(-max(0, passes(ppg) - NPRE) // UAPPLY)


def bwd_reduce_chunks(ppg, alpha):
    return -(-passes(ppg) // (2 if alpha else 4))


# ------------------------------------------------------------------------------------------------ partial rows
def row_bounds(M, P):
    """P distinct, uneven, non-empty row ranges that cover [0, M): sizes in the proportion 1 : 3 : 2 : 1 : 3 : 2 ..."""
    assert 0 < P <= M
    w = [1 + (r * 5) % 3 for r in range(P)]
    W, acc, b = sum(w), 0, [0]
    for r in range(P):
        acc += w[r]
        b.append(min(max(M * acc // W, b[-1] + 1), M - (P - 1 - r)))
    assert b[-1] == M
    return b


def partial_rows(cols, bounds):
    """[P][len(cols)][C] fp32: the fp64 column sums of the row ranges, rounded once"""
    b = torch.tensor(bounds)
    out = []
    for t in cols:
        cs = torch.cat([torch.zeros(1, t.shape[1], dtype=f64), t.to(f64).cumsum(0)])
        out.append(cs[b[1:]] - cs[b[:-1]])
    return torch.stack(out, 1).to(f32)


def const_rows(bounds, values):
    """rows of a channel that is constant: fractional pixel counts n_r = size_r + (r - (P - 1) / 2) / 512 (pairwise different, sum M exactly)
    times the per-pixel value of each statistic; [P][len(values)] float64"""
    P = len(bounds) - 1
    n = torch.tensor([bounds[r + 1] - bounds[r] + (r - (P - 1) / 2.0) / 512.0 for r in range(P)], dtype=f64)
    return torch.stack([n * v for v in values], 1)


def pairwise_distinct(rows, nv=None):
    v = rows[:, :nv].sort(0)[0]
    return not bool((v[1:] == v[:-1]).any())


def make_distinct(rows, fixed=(), nv=None):
    """spreads every run of L equal values of one (statistic, channel) symmetrically, to v + (2 i - (L - 1)) step, i = 0 .. L - 1, step = 2^-22 (two fp32
    steps) of the column's largest magnitude (+ 2^-6): the column's total stays what it was (the channel with |mean| = 32 sigma would turn a shifted
    total into a different variance).  ``fixed``: channels left alone (constructed distinct); nv: statistics that are read"""
    rows = rows.clone()
    sub = rows[:, :nv]
    P = sub.shape[0]
    i = torch.arange(P).reshape(-1, 1, 1).expand_as(sub)
    for it in range(16):
        v, idx = sub.sort(0)
        first = torch.ones_like(v, dtype=torch.bool)
        first[1:] = v[1:] != v[:-1]
        last = torch.ones_like(v, dtype=torch.bool)
        last[:-1] = first[1:]
        for c in fixed:
            first[:, :, c] = last[:, :, c] = True
        if bool(first.all()):
            break
        start = torch.where(first, i, torch.zeros_like(i)).cummax(0)[0]
        end = torch.where(last, i, torch.full_like(i, P - 1)).flip(0).cummin(0)[0].flip(0)
        step = 2.0 ** -22 * (v.abs().amax(0, keepdim=True) + 2.0 ** -6)
        sub.scatter_(0, idx, v + (2 * (i - start) - (end - start)).to(f32) * step)
    return rows


def row_variants(rows):
    """the corruptions of a fan-in: (name, rows) — one row dropped, one counted twice, the last replaced by a repeat of the one before"""
    P = rows.shape[0]
    out = [("row dropped", torch.cat([rows[: P // 2], rows[P // 2 + 1:]])), ("row twice", torch.cat([rows, rows[P // 2: P // 2 + 1]]))]
    if P > 1:
        out.append(("last row = the one before", torch.cat([rows[:-1], rows[-2:-1]])))
    return out


# ------------------------------------------------------------------------------------------------ a workgroup's sums
def group_sum(terms, M, ppg, dt, gid=None, scale=None):
    """[G][C] per term: the sum over each pixel group.  terms: tensors [M][C], or pairs (a, b) that are accumulated as acc = fma(a, b, acc).
    float64: plain (gid: a pixel -> group map, -1 = not counted, for the corruptions).  float32: the kernel's order — thread pl = pixel % 64
    of the group adds its pixels pass by pass, then the binary tree over the 64 pixel lanes (xor-shuffles 4 .. 32, (w0 + w1) + (w2 + w3)).
    scale: per term, None or a per-channel factor each thread applies to its sum before the tree (rstd)"""
    G = -(-M // ppg)
    if dt == f64:
        if gid is None:
            gid = torch.arange(M) // ppg
        keep = gid >= 0
        out = []
        for t in terms:
            v = t[0].to(f64) * t[1].to(f64) if isinstance(t, tuple) else t.to(f64)
            out.append(torch.zeros(G, v.shape[1], dtype=f64).index_add_(0, gid[keep], v[keep]))
        return [o if scale is None or scale[i] is None else o * scale[i].to(f64) for i, o in enumerate(out)]
    npass = passes(ppg)
    j = torch.arange(npass * PXP).reshape(1, -1)
    m = torch.arange(G).reshape(G, 1) * ppg + j
    m = torch.where((j < ppg) & (m < M), m, torch.full_like(m, M))          # beyond the group or the tensor: the zero row appended below
    m = m.reshape(-1)

    def padded(t):
        t = t.to(f32)
        return torch.cat([t, torch.zeros(1, t.shape[1])])[m].reshape(G, npass, PXP, -1)

    out = []
    for i, t in enumerate(terms):
        if isinstance(t, tuple):
            a, b = padded(t[0]), padded(t[1])
            acc = torch.zeros(G, PXP, a.shape[-1])
            for u in range(npass):
                acc = fma(a[:, u], b[:, u], acc, f32)
        else:
            a = padded(t)
            acc = torch.zeros(G, PXP, a.shape[-1])
            for u in range(npass):
                acc = acc + a[:, u]
        if scale is not None and scale[i] is not None:
            acc = acc * scale[i].to(f32)
        while acc.shape[1] > 1:
            acc = acc[:, 0::2] + acc[:, 1::2]
        out.append(acc[:, 0])
    return out


def gid_last_pixel_lost(M, ppg):
    g = torch.arange(M) // ppg
    g[M - 1] = -1
    return g


def gid_boundary_moved(M, ppg):
    """the first pixel of group 1 counted in group 0's row"""
    g = torch.arange(M) // ppg
    g[ppg] = 0
    return g


# ------------------------------------------------------------------------------------------------ forward coefficients
def fwd_coef(rows, count, gamma, beta, rm, rv, i2=1, unbiased=True):
    """bn_fwd_coef + bn_running_update on the fp64 sum of the given fp32 rows (statistic 0 = sum x, i2 = sum x^2): a dict of Q.  All fp64 up
    to one fp32 store each: COEF_ULPS 2^-24 of |value| (mean, rstd, scale), of |beta| + |mean gamma rstd| (shift), of the blended terms with
    the variance as E[x^2] + mean^2, the two that cancel (running statistics)"""
    S = rows.to(f64).sum(0)
    mean, e2 = S[0] / count, S[i2] / count
    var = (e2 - mean * mean).clamp_min(0.0)
    rstd = 1.0 / torch.sqrt(var + EPSF)
    g, b = gamma.to(f64), beta.to(f64)
    t = COEF_ULPS * U24
    out = {"mean": Q(mean, t * mean.abs()), "rstd": Q(rstd, t * rstd), "scale": Q(g * rstd, t * (g * rstd).abs()),
           "shift": Q(b - mean * g * rstd, t * (b.abs() + (mean * g * rstd).abs()))}
    if rm is not None:
        k = count / (count - 1.0) if unbiased else 1.0
        out["rm"] = Q((1.0 - MOM) * rm.to(f64) + MOM * mean, t * ((1.0 - MOM) * rm.to(f64).abs() + MOM * mean.abs()))
        out["rv"] = Q((1.0 - MOM) * rv.to(f64) + MOM * var * k, t * ((1.0 - MOM) * rv.to(f64).abs() + MOM * k * (e2.abs() + mean * mean)))
    out["_var"], out["_S"] = var, S
    return out


def stored32(q):
    """what a correct kernel stores for an fp64-derived coefficient: the fp32 rounding"""
    return q.value.to(f32)


def special_x(M, C, seed, s16, const=True):
    x = r16(uniform((M, C), seed) * 2 + 0.3, s16)
    x[:, BIG] = r16(4.0 + 0.2165 * uniform((M,), seed + 1), s16)      # sigma = 0.2165 / sqrt(3) = 1 / 8: |mean| = 32 sigma
    if const:
        x[:, CONST] = CONST_X
    return x


def params(x, seed, tie=None, gamma=True, beta=True, const=True, zero_beta=None):
    """stem_cases.BnParams of x, with beta[CONST] large enough for z = beta to stay off the mask threshold, or with the default values of a null
    gamma / beta; (sc, sh) follow"""
    p = BnParams(x, seed, None)
    if not gamma:
        p.gamma = torch.ones_like(p.gamma)
    if not beta:
        p.beta = torch.zeros_like(p.beta)
    elif const:
        p.beta[CONST] = CONST_BETA
    if zero_beta is not None:
        p.beta[ZERO] = zero_beta
    p.sc = (p.gamma.to(f64) * p.rstd.to(f64)).to(f32)
    p.sh = (p.beta.to(f64) - p.mean.to(f64) * p.sc.to(f64)).to(f32)
    if tie is not None:
        p.sc[tie], p.sh[tie] = 1.0, -0.5
    return p


# ================================================================================================ bn_apply_sliced
class FwdCase:
    """y = r16(prelu?(x1 sc + sh) (+ x2)), the coefficient set from P given rows [2][C], the statistics rows of the stored y.
    null: names of the optional vectors passed as NULL ("gamma", "beta", "rm")"""
    kind = "apply"

    def __init__(self, M, C, P, s16, prelu=False, x2=False, stats=True, null=()):
        self.M, self.C, self.P, self.s16, self.prelu, self.has_x2, self.stats, self.null = M, C, P, s16, prelu, x2, stats, tuple(null)
        self.G, self.ppg = sliced_geometry(M, C)
        self.variant = apply_variant(M, C, x2)
        self.name = "apply[%dx%d,P=%d%s%s%s%s]" % (M, C, P, ",prelu" if prelu else "", ",x2" if x2 else "", ",stats" if stats else "",
                                                 "".join(",null_" + n for n in self.null))
        self.const = "beta" not in self.null                  # z = beta in the constant channel: a null beta would put it ON the threshold
        kw = dict(gamma="gamma" not in self.null, beta="beta" not in self.null, const=self.const)
        x = special_x(M, C, 31, s16, self.const)
        p = params(x, 33, **kw)
        if prelu or not x2:                                   # |z| >= 6e-3: off the threshold, and alpha z (alpha >= 0.15) no 16-bit result under RMIN
            x = nudge_from_zero(x, p.sc / 4, p.sh / 4, s16)
            p = params(x, 33, **kw)
        self.x, self.p = x, p
        self.gamma, self.beta = (p.gamma if kw["gamma"] else None), (p.beta if kw["beta"] else None)
        self.rm = self.rv = None
        if "rm" not in self.null:
            self.rm, self.rv = uniform((C,), 36) * 0.1, uniform((C,), 37) * 0.1 + 1.0
        self.count = float(M)
        self.bounds = row_bounds(M, P)
        xd = x.to(f64)
        rows = partial_rows([xd, xd * xd], self.bounds)
        if self.const:
            cr = const_rows(self.bounds, [CONST_X, CONST_X * CONST_X])
            cr[0, 1] -= 2.0 ** -10
            rows[:, :, CONST] = cr.to(f32)
        self.rows = make_distinct(rows, fixed=(CONST,) if self.const else ())
        self.x2 = r16(uniform((M, C), 38), s16) if x2 else None
        if x2:
            sc, sh = stored32(self.coef()["scale"]), stored32(self.coef()["shift"])
            for _ in range(3):
                o = self.y(sc, sh).value
                bad = (o.abs() < 2 * RMIN) & (o != 0)
                if not bool(bad.any()):
                    break
                self.x2 = torch.where(bad, r16(self.x2.to(f32) + torch.where(self.x2 >= 0, 1.0, -1.0), s16), self.x2)

    def coef(self, rows=None, count=None, unbiased=True):
        return fwd_coef(self.rows if rows is None else rows, self.count if count is None else count, self.p.gamma, self.p.beta, self.rm, self.rv,
                        unbiased=unbiased)

    def y(self, sc, sh, dt=f64, flip=None, neighbour_slope=False):
        """the stored y for GIVEN fp32 (scale, shift): fma, the PReLU product, the addend — dx_q's form over |x sc| + |sh| (+ |x2|)"""
        xv, s, h = self.x.to(dt), sc.to("cpu", dt), sh.to("cpu", dt)
        z = fma(xv, s, h.expand_as(xv), dt)
        o = z
        if self.prelu:
            al = self.p.alpha.roll(1) if neighbour_slope else self.p.alpha
            pos = z > 0
            if flip is not None:
                pos = pos.clone()
                pos[flip] = ~pos[flip]
            o = torch.where(pos, z, al.to(dt) * z)
        mag = (xv * s).abs().to(f64) + h.abs().to(f64)
        if self.has_x2:
            o = o + self.x2.to(dt)
            mag = mag + self.x2.abs().to(f64)
        return dx_q(o, mag, self.s16)

    def z(self, sc, sh, dt=f64):
        xv = self.x.to(dt)
        return fma(xv, sc.to(dt), sh.to(dt).expand_as(xv), dt)

    def stats_q(self, y16, dt=f64, gid=None):
        """the G statistics rows [G][2][C] of a STORED y (sum y, sum y^2 per pixel group): chain = passes + tree + 1 (the product's rounding
        inside the fma)"""
        y = y16.to("cpu")
        s = group_sum([y, (y, y)], self.M, self.ppg, dt, gid)
        yd = y.to(f64)
        a = group_sum([yd.abs(), yd * yd], self.M, self.ppg, f64)
        return Q(torch.stack(s, 1), (passes(self.ppg) + SUM_TREE + 1) * U24 * torch.stack(a, 1))


# ================================================================================================ bn_apply2_sliced
class Apply2Case:
    """out = r16(x1 sc + sh + x2), y2 = r16(out nsc + nsh): the first coefficient set from P rows [3][C] = (sum x1, sum x1 x2, sum x1^2), the
    second from the DERIVED statistics of out"""
    kind = "apply2"

    def __init__(self, M, C, P, s16):
        self.M, self.C, self.P, self.s16 = M, C, P, s16
        self.G, self.ppg = sliced_geometry(M, C)
        self.variant = apply2_variant(M, C, P)
        self.name = "apply2[%dx%d,P=%d]" % (M, C, P)
        self.count = float(M)
        self.x = special_x(M, C, 41, s16)
        # beta = 2^-4 in the ZERO and CONST channels, where out = beta + x2: exact in 16 bits for nearly every element.  With 0.05 every element
        # of a binade of x2 is rounded the same way and the MEASURED mean moves by a third of its bound — no error of a kernel, but no quarter either
        self.p = params(self.x, 43, zero_beta=CONST_BETA)
        self.rm, self.rv = uniform((C,), 46) * 0.1, uniform((C,), 47) * 0.1 + 1.0
        self.nrm, self.nrv = uniform((C,), 48) * 0.1, uniform((C,), 49) * 0.1 + 1.0
        self.x2 = r16(uniform((M, C), 50) * 1.3 + 0.25, s16)
        self.bounds = row_bounds(M, P)
        for it in range(8):                                    # no stored out or y2 under RMIN: their x2 moves by 1.0 (and the statistics follow)
            self._finish()
            c1 = self.coef()
            sc, sh = stored32(c1["scale"]), stored32(c1["shift"])
            o = self.out(sc, sh)
            c2 = self.second(sc, sh)
            o16 = r16(o.value.to(f32), s16)
            y2 = self.y2(o16, stored32(c2["nscale"]), stored32(c2["nshift"])).value
            bad = ((o.value.abs() < 2 * RMIN) & (o.value != 0)) | ((y2.abs() < 2 * RMIN) & (y2 != 0))
            if not bool(bad.any()):
                break
            self.x2 = torch.where(bad, r16(self.x2.to(f32) + torch.where(self.x2 >= 0, 1.0, -1.0), s16), self.x2)
        self._finish()

    def _finish(self):
        """everything that follows from (x1, x2): the saved statistics of x2, the next BatchNorm's parameters, the rows"""
        x1, x2 = self.x.to(f64), self.x2.to(f64)
        self.x2_mean64, self.x2_var64 = x2.mean(0), x2.var(0, unbiased=False)
        self.xmean = self.x2_mean64.to(f32)
        self.xrstd = (1.0 / torch.sqrt(self.x2_var64 + EPSF)).to(f32)
        self.np = params(x2, 51, const=False)                  # gamma / beta of the next BatchNorm (its NEG and ZERO channels included)
        cols = [x1, x1 * x2, x1 * x1]
        self.exact_S = torch.stack([c.sum(0) for c in cols])
        rows = partial_rows(cols, self.bounds)
        cr = const_rows(self.bounds, [CONST_X, 1.0, CONST_X * CONST_X])
        cr[:, 1] = cr[:, 1] * CONST_X * self.xmean[CONST].to(f64)
        cr[0, 2] -= 2.0 ** -10
        rows[:, :, CONST] = cr.to(f32)
        self.rows = make_distinct(rows, fixed=(CONST,))

    def coef(self, rows=None, count=None, unbiased=True):
        return fwd_coef(self.rows if rows is None else rows, self.count if count is None else count, self.p.gamma, self.p.beta, self.rm, self.rv,
                        i2=2, unbiased=unbiased)

    def second(self, sc, sh, rows=None, count=None, unbiased=True, with_cov=True, exact=False):
        """the statistics of out = sc x1 + sh + x2 by the kernel's formulas, with the GIVEN fp32 (sc, sh), and the next BatchNorm's
        coefficient set.  exact: from the tensors' own fp64 sums and x2 statistics instead of the rows and the fp32 (x2_mean, x2_rstd).
        Each is fp64 up to its fp32 store: COEF_ULPS 2^-24 of the magnitudes of its terms"""
        count = self.count if count is None else count
        S = self.exact_S if exact else (self.rows if rows is None else rows).to(f64).sum(0)
        mean, e2 = S[0] / count, S[2] / count
        var = (e2 - mean * mean).clamp_min(0.0)
        if exact:
            mx, vx = self.x2_mean64, self.x2_var64
        else:
            mx, xr = self.xmean.to(f64), self.xrstd.to(f64)
            vx = (1.0 / (xr * xr) - EPSF).clamp_min(0.0)
        cov = S[1] / count - mean * mx
        s, h = sc.to("cpu", f64), sh.to("cpu", f64)
        omean = s * mean + h + mx
        ovar = (s * s * var + vx + (2.0 * s * cov if with_cov else 0.0)).clamp_min(0.0)
        orstd = 1.0 / torch.sqrt(ovar + EPSF)
        g, b = self.np.gamma.to(f64), self.np.beta.to(f64)
        t = COEF_ULPS * U24
        k = count / (count - 1.0) if unbiased else 1.0
        m_om = (s * mean).abs() + h.abs() + mx.abs()
        m_ov = s * s * (e2.abs() + mean * mean) + vx + 2.0 * s.abs() * ((S[1] / count).abs() + (mean * mx).abs())
        return {"nmean": Q(omean, t * m_om), "nrstd": Q(orstd, t * orstd), "nscale": Q(g * orstd, t * (g * orstd).abs()),
                "nshift": Q(b - omean * g * orstd, t * (b.abs() + m_om * (g * orstd).abs())),
                "nrm": Q((1.0 - MOM) * self.nrm.to(f64) + MOM * omean, t * ((1.0 - MOM) * self.nrm.to(f64).abs() + MOM * m_om)),
                "nrv": Q((1.0 - MOM) * self.nrv.to(f64) + MOM * ovar * k, t * ((1.0 - MOM) * self.nrv.to(f64).abs() + MOM * k * m_ov)),
                "_ovar": ovar}

    def out(self, sc, sh, dt=f64):
        xv, s, h = self.x.to(dt), sc.to("cpu", dt), sh.to("cpu", dt)
        o = fma(xv, s, h.expand_as(xv), dt) + self.x2.to(dt)
        return dx_q(o, (xv * s).abs().to(f64) + h.abs().to(f64) + self.x2.abs().to(f64), self.s16)

    def y2(self, out16, nsc, nsh, dt=f64):
        """from the STORED out: an element of out one 16-bit step off is not charged to y2"""
        ov, s, h = out16.to("cpu", dt), nsc.to("cpu", dt), nsh.to("cpu", dt)
        return dx_q(fma(ov, s, h.expand_as(ov), dt), (ov * s).abs().to(f64) + h.abs().to(f64), self.s16)

    def measured(self, out16, sc, sh):
        """the looser pair: derived nmean / nrstd against the statistics MEASURED on the stored out.  An element of the stored out differs from
        the exact sc x1 + sh + x2 by at most d_i = its own tolerance (16-bit rounding + fp32 evaluation), so the measured mean moves by at
        most mean(d) (~ u16 mean |out|) and the measured variance by at most 2 mean(|out - m| d) + mean(d^2); to that the distance between
        the statistics derived from the GIVEN rows and from the tensors' exact fp64 sums is added (the rows are fp32, were made distinct and carry
        the constant channel's lowered sum of squares), and the fp32 stores.  rstd: the larger change of (v + eps)^-1/2 over v -+ that bound"""
        o = out16.to("cpu", f64)
        d = self.out(sc, sh).tol
        m, v = o.mean(0), o.var(0, unbiased=False)
        given, exact = self.second(sc, sh), self.second(sc, sh, exact=True)
        dm = d.mean(0) + (given["nmean"].value - exact["nmean"].value).abs() + COEF_ULPS * U24 * m.abs()
        dv = 2.0 * ((o - m).abs() * d).mean(0) + (d * d).mean(0) + (given["_ovar"] - exact["_ovar"]).abs()
        f = lambda t: 1.0 / torch.sqrt(t.clamp_min(0.0) + EPSF)      # noqa: E731
        r = f(v)
        dr = torch.maximum((f(v - dv) - r).abs(), (f(v + dv) - r).abs()) + COEF_ULPS * U24 * r
        return {"nmean": Q(m, dm), "nrstd": Q(r, dr)}


# ================================================================================================ bn_bwd_sliced
RED_CHAIN_EXTRA = 3      # dz = dy alpha, x - mean (or z), and the final multiplication by rstd
NEXT_CHAIN_EXTRA = 2     # x - mean and the final multiplication by rstd


class BwdCase:
    """variant = 4 alpha | 2 next | 1 add.  rows_in = 0: the entry point runs its reduce pass (G rows, left in ``partials``); rows_in = P > 0:
    external rows, the exact fp64 sums of P uneven row ranges rounded to fp32.  null: parameter-gradient outputs passed as NULL"""
    kind = "bwd"

    def __init__(self, M, C, variant, s16, rows_in=0, null=()):
        self.M, self.C, self.v, self.s16, self.rows_in, self.null = M, C, variant, s16, rows_in, tuple(null)
        self.alpha, self.has_nx, self.has_add = bool(variant & 4), bool(variant & 2), bool(variant & 1)
        self.G, self.ppg = sliced_geometry(M, C, True)
        self.P = rows_in if rows_in > 0 else self.G
        self.nv = 3 if self.alpha else 2
        _, self.fx, self.variant = bwd_variant(self.P, self.alpha, self.has_nx, self.has_add)
        self.name = "bwd[%dx%d,v=%d,%s%s]" % (M, C, variant, "P=%d" % rows_in if rows_in else "own rows", "".join(",null_" + n for n in self.null))
        self.count = float(M)
        x = special_x(M, C, 61, s16)
        self.keep = tie_rows(M, C, TIE, 0) if self.alpha else torch.zeros(M, C, dtype=torch.bool)
        if self.alpha:
            x[self.keep] = 0.5
        p = params(x, 62, TIE if self.alpha else None)
        if self.alpha:
            x = nudge_from_zero(x, p.sc, p.sh, s16, self.keep)
            p = params(x, 62, TIE)
        self.x, self.p = x, p
        # a gradient with a mean (B = -a mean(dz) is then no rounding-size term: ``count`` shows); the constant channel's rstd is 316: its
        # gradient is 2^-9 of the others' so that dx stays inside fp16
        dy = (uniform((M, C), 65) + 0.25) * GSCALE
        dy[:, CONST] *= 2.0 ** -9
        self.dy = r16(dy, s16)
        self.add = r16(uniform((M, C), 66) * GSCALE, s16) if self.has_add else None
        self.extra = None if self.add is None else self.add.to(f64)
        if self.has_nx:
            self.nx = special_x(M, C, 68, s16, const=False)
            self.np = params(self.nx, 69, const=False)
        self.bounds = row_bounds(M, self.P) if rows_in > 0 else None
        self._terms64, self._frozen = None, False
        for _ in range(8):
            self.rows = self._external_rows() if rows_in > 0 else None
            o = self.dx(self.given_rows()).value
            bad = (o.abs() < 2 * RMIN) & (o != 0)
            if not bool(bad.any()):
                break
            step = (self.dy.to(f32).abs() * 2.0 ** -6).clamp_min(1.0)        # at least two bf16 steps: 1.0 alone is rounded away above 256
            self.dy = torch.where(bad, r16(self.dy.to(f32) + torch.where(self.dy >= 0, step, -step), s16), self.dy)
        self.rows = self._external_rows() if rows_in > 0 else None
        self._frozen = True

    def terms(self, dt=f64, flip=None, neighbour_slope=False):
        """(dz, [t0, t1 without rstd as a pair, t2 as a pair]) in the kernel's order: acc1 = fma(dz, x - mean, acc1), acc2 = fma(dy, z, acc2)"""
        plain = dt == f64 and flip is None and not neighbour_slope
        if plain and self._terms64 is not None:
            return self._terms64
        p = self.p
        dyv, xv = self.dy.to(dt), self.x.to(dt)
        if self.alpha:
            z = fma(xv, p.sc.to(dt), p.sh.to(dt).expand_as(xv), dt)
            neg = z <= 0
            if flip is not None:
                neg = neg.clone()
                neg[flip] = ~neg[flip]
            al = (p.alpha.roll(1) if neighbour_slope else p.alpha).to(dt)
            dz = torch.where(neg, dyv * al, dyv)
            t2 = (torch.where(neg, dyv, torch.zeros_like(dyv)), z)
        else:
            dz, t2 = dyv, (torch.zeros_like(dyv), torch.zeros_like(dyv))
        out = dz, [dz, (dz, xv - p.mean.to(dt)), t2]
        if plain and self._frozen:                             # the float64 terms of the finished case are computed once
            self._terms64 = out
        return out

    def reduce_rows(self, dt=f64, gid=None, flip=None, neighbour_slope=False):
        """[G][3][C]: what the reduce pass leaves (sum dz | rstd sum dz (x - mean) | sum dy z over z <= 0)"""
        _, t = self.terms(dt, flip, neighbour_slope)
        return torch.stack(group_sum(t, self.M, self.ppg, dt, gid, scale=[None, self.p.rstd, None]), 1)

    def reduce_rows_q(self, dt=f64):
        """chain = passes + tree + RED_CHAIN_EXTRA, times 2^-24 sum |terms| of the group (rstd |dz (x - mean)| for the second)"""
        _, t = self.terms(f64)
        a = group_sum([t[0].abs(), (t[1][0] * t[1][1]).abs(), (t[2][0] * t[2][1]).abs()], self.M, self.ppg, f64)
        a[1] = a[1] * self.p.rstd.to(f64)
        return Q(self.reduce_rows(dt), (passes(self.ppg) + SUM_TREE + RED_CHAIN_EXTRA) * U24 * torch.stack(a, 1))

    def _external_rows(self):
        dz, t = self.terms(f64)
        cols = [t[0], t[1][0] * t[1][1] * self.p.rstd.to(f64), t[2][0] * t[2][1]]
        rows = partial_rows(cols, self.bounds)
        return make_distinct(rows, nv=self.nv)

    def given_rows(self):
        """the rows the apply pass is given in the reference computation: the external ones, or the fp32 rounding of the fp64 reduce rows"""
        return self.rows if self.rows_in > 0 else self.reduce_rows().to(f32)

    def grads_q(self, rows, second=1):
        """dbeta, dgamma, dalpha = the fp64 sums of the given rows, stored as fp32: COEF_ULPS 2^-24 of their magnitude.  second: the statistic
        read as the second sum (2: the corruption)"""
        S = rows.to("cpu", f64).sum(0)
        t = COEF_ULPS * U24
        return {"dbeta": Q(S[0], t * S[0].abs()), "dgamma": Q(S[second], t * S[second].abs()), "dalpha": Q(S[2], t * S[2].abs())}

    def dx(self, rows, dt=f64, count=None, second=1, flip=None, neighbour_slope=False):
        """the stored dx for GIVEN rows: coefficients (stem_cases.bn_coef, rounded to fp32 as the kernel holds them) from their fp64 sums;
        dx_q + one unit in the last place of each coefficient (bn_coef_tol with exact sums) through |dz|, |x|, 1: the kernel multiplies by
        1 / count where bn_coef divides"""
        S = rows.to("cpu", f64).sum(0)
        cnt = self.count if count is None else count
        c64 = bn_coef(S[0], S[second], self.p, cnt)
        dz, _ = self.terms(dt, flip, neighbour_slope)
        o, mag = bn_dx(c64.to(f32), dz, self.x, dt, self.extra)
        q = dx_q(o, mag, self.s16)
        zero = torch.zeros_like(S[0])
        tc = bn_coef_tol(c64, zero, zero, self.p, cnt)
        return Q(q.value, q.tol + tc[0] * dz.abs().to(f64) + tc[1] * self.x.to(f64).abs() + tc[2])

    def next_rows_q(self, dx16, dt=f64, gid=None):
        """the G rows [G][3][C] for the next BatchNorm backward, of a STORED dx: (sum dx, nrstd sum dx (nx - nmean), exactly 0);
        chain = passes + tree + NEXT_CHAIN_EXTRA"""
        d = dx16.to("cpu")
        xm = self.nx.to(dt) - self.np.mean.to(dt)
        s = group_sum([d, (d.to(dt), xm)], self.M, self.ppg, dt, gid, scale=[None, self.np.rstd])
        dd = d.to(f64)
        a = group_sum([dd.abs(), (dd * (self.nx.to(f64) - self.np.mean.to(f64))).abs()], self.M, self.ppg, f64)
        a[1] = a[1] * self.np.rstd.to(f64)
        zero = torch.zeros_like(s[0])
        return Q(torch.stack(s + [zero], 1), (passes(self.ppg) + SUM_TREE + NEXT_CHAIN_EXTRA) * U24 * torch.stack(a + [zero.to(f64)], 1))


# ================================================================================================ case tables
# (M, C): (forward G, ppg, pixels in the last group, grid) and (backward G, ppg, last) — written by hand from sliced_geometry; the CPU test holds
# the mirror to them, the GPU test holds the library's row queries to the mirror
GEOMETRY = {
    (256, 64): ((32, 8, 8, 64), (32, 8, 8)),
    (257, 64): ((33, 8, 1, 66), (33, 8, 1)),
    (264, 96): ((33, 8, 8, 99), (33, 8, 8)),
    (300, 160): ((38, 8, 4, 190), (38, 8, 4)),
    (897, 128): ((57, 16, 1, 228), (57, 16, 1)),
    (1793, 512): ((15, 120, 113, 240), (15, 120, 113)),
    (1536, 1024): ((8, 192, 192, 256), (8, 192, 192)),
    (1537, 1024): ((8, 200, 137, 256), (8, 200, 137)),
    (2049, 1024): ((8, 264, 201, 256), (8, 264, 201)),
    (2561, 1024): ((8, 328, 265, 256), (8, 328, 265)),
    (3584, 1024): ((8, 448, 448, 256), (8, 448, 448)),
    (3585, 1024): ((8, 456, 393, 256), (8, 456, 393)),
    (6657, 1024): ((9, 832, 1, 288), (8, 840, 777)),
    (13313, 1024): ((17, 832, 1, 544), (9, 1664, 1)),
}

FWD_TABLE = {}
APPLY2_TABLE = {}
BWD_TABLE = {}


def _fwd(M, C, P, **kw):
    c = dict(M=M, C=C, P=P, **kw)
    FWD_TABLE["f%02d" % len(FWD_TABLE)] = c


def _bwd(M, C, v, rows_in=0, null=()):
    BWD_TABLE["b%02d" % len(BWD_TABLE)] = dict(M=M, C=C, variant=v, rows_in=rows_in, null=null)


# ---- forward: shapes (special channels at a small and a multi-pass shape: every row has them)
_fwd(256, 64, 7, prelu=True, x2=True, stats=True)
_fwd(257, 64, 3, stats=True)
_fwd(264, 96, 5, prelu=True, stats=True)
_fwd(300, 160, 9, x2=True, stats=True)
_fwd(897, 128, 8, prelu=True, x2=True, stats=False)
_fwd(1793, 512, 15, x2=True, stats=True)
_fwd(3584, 1024, 16, prelu=True, x2=True, stats=True)
_fwd(3585, 1024, 17, prelu=True, stats=True)
_fwd(6657, 1024, 64, x2=True, stats=True)
_fwd(13313, 1024, 98, stats=True)
# ---- forward: the other seven flag combinations
for _f in range(7):
    _fwd(264, 96, 4, prelu=bool(_f & 4), x2=bool(_f & 2), stats=bool(_f & 1))
# ---- forward: null optional vectors
for _n in (("gamma",), ("beta",), ("rm",), ("gamma", "beta", "rm")):
    _fwd(256, 64, 6, prelu=True, x2=True, stats=True, null=_n)
# ---- forward: fan-in edges (RG = 16 row groups x FL = 16)
FWD_FANIN = (1, 15, 16, 17, 255, 256)
for _p in FWD_FANIN:
    _fwd(264, 96, _p, stats=True)

# ---- apply2: shapes, then the fan-in edges (RG = 10, narrow FL = 13 -> 130 rows, wide 260)
APPLY2_FANIN = (1, 10, 130, 131, 260)
for _i, (_m, _c, _p) in enumerate([(256, 64, 5), (257, 64, 3), (300, 160, 7), (897, 128, 8), (1793, 512, 9), (3584, 1024, 19), (3585, 1024, 21), (3585, 1024, 200)]
                                  + [(264, 96, p) for p in APPLY2_FANIN]):
    APPLY2_TABLE["a%02d" % _i] = dict(M=_m, C=_c, P=_p)

# ---- backward: all eight variants, with rows from the own reduce pass and with external rows
for _v in range(8):
    _bwd(256, 64, _v)
    _bwd(256, 64, _v, rows_in=5)
# ---- backward: shapes
_bwd(257, 64, 7)
_bwd(264, 96, 6)
_bwd(300, 160, 3)
_bwd(897, 128, 5)
_bwd(1793, 512, 2)
_bwd(1536, 1024, 7)
_bwd(1537, 1024, 4, rows_in=8)
_bwd(2049, 1024, 1)
_bwd(2561, 1024, 6)
_bwd(6657, 1024, 5)
_bwd(13313, 1024, 2)
# ---- backward: null parameter gradients
for _n in (("dgamma",), ("dbeta",), ("dalpha",), ("dgamma", "dbeta", "dalpha")):
    _bwd(256, 64, 7, null=_n)
# ---- backward: fan-in edges without PReLU (RG = 16, FL = 8 -> 128 rows narrow) and with (RG = 10, FL = 13 -> 130)
BWD_FANIN2, BWD_FANIN3 = (1, 16, 17, 128, 129, 256), (1, 10, 11, 130, 131, 256)
for _p in BWD_FANIN2:
    _bwd(264, 96, 0, rows_in=_p)
for _p in BWD_FANIN3:
    _bwd(264, 96, 4, rows_in=_p)

# rejections: (entry point, M, C, P) that must return an error (P: rows given; for bwd rows_in, 0 = own reduce pass)
REJECT = [("apply", 255, 64, 4), ("apply", 256, 48, 4), ("apply", 256, 1056, 4), ("apply", 256, 80, 4), ("apply", 13672, 1024, 4),
          ("apply", 256, 64, 0), ("apply", 256, 64, 257),
          ("apply2", 255, 64, 4), ("apply2", 256, 48, 4), ("apply2", 256, 1056, 4), ("apply2", 256, 80, 4), ("apply2", 13672, 1024, 4),
          ("apply2", 256, 64, 0), ("apply2", 264, 96, 261),
          ("bwd", 255, 64, 0), ("bwd", 256, 48, 0), ("bwd", 256, 1056, 0), ("bwd", 256, 80, 0), ("bwd", 13672, 1024, 0), ("bwd", 256, 64, 257)]

def row_info(kind, key):
    """what a table row is for, from the mirror alone (no tensors): geometry, rows given, the instantiation its launcher picks"""
    r = {"apply": FWD_TABLE, "apply2": APPLY2_TABLE, "bwd": BWD_TABLE}[kind][key]
    M, C = r["M"], r["C"]
    G, ppg = sliced_geometry(M, C, kind == "bwd")
    info = dict(M=M, C=C, G=G, ppg=ppg, last=M - (G - 1) * ppg, grid=G * (C // SW), passes=passes(ppg))
    if kind == "apply":
        info.update(P=r["P"], kernel=apply_variant(M, C, r.get("x2", False)))
    elif kind == "apply2":
        info.update(P=r["P"], kernel=apply2_variant(M, C, r["P"]))
    else:
        v = r["variant"]
        P = r["rows_in"] or G
        info.update(P=P, own_rows=r["rows_in"] == 0, kernel=bwd_variant(P, bool(v & 4), bool(v & 2), bool(v & 1))[2],
                    reduce_kernel=None if r["rows_in"] else "bn_bwd_reduce_s<ALPHA=%d,U=%d>" % (bool(v & 4), 2 if v & 4 else 4),
                    apply_chunks=bwd_apply_chunks(ppg), reduce_chunks=bwd_reduce_chunks(ppg, bool(v & 4)))
    return info


_CACHE = {}


def case(kind, key, s16):
    """the case of a table row, built once per storage type"""
    k = (kind, key, s16)
    if k not in _CACHE:
        if kind == "apply":
            _CACHE[k] = FwdCase(s16=s16, **FWD_TABLE[key])
        elif kind == "apply2":
            _CACHE[k] = Apply2Case(s16=s16, **APPLY2_TABLE[key])
        else:
            _CACHE[k] = BwdCase(s16=s16, **BWD_TABLE[key])
    return _CACHE[k]


def drop(kind, key, s16):
    _CACHE.pop((kind, key, s16), None)
