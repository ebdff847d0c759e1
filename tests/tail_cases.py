"""Inputs, case tables, tolerance rules, restated dispatch rules and plain references for the direct tests of the network tail — the kernels
between the last residual block and the embedding (csrc/ew.hip: BatchNorm1d, split-K slab reduction, dropout, NCHW -> NHWC, the 16-bit cast,
the dgrad weight shadows), the plain-mode GEMMs of the fc layer (fedfr_gemm_nt / fedfr_gemm_tn, mode == 0) and four small aggregation /
PartialFC entry points.  tests/test_tail_kernels_gpu.py runs the kernels against what is here; tests/test_tail_cases_cpu.py holds the same
formulas at fp32, in the kernels' operation order, to a QUARTER of every tolerance, proves the exact cases admissible and shows one mutant per
check that the check rejects.  Nothing here touches the GPU library or imports the oracle.

References are float64 torch / numpy formulas written from the operation's definition: F.batch_norm and autograd, permute, .to(dtype), a
matrix product, a sum.  Where a kernel's contract is an ORDER or a HASH (the slab sums, the dropout mask, the PartialFC random numbers, the
int64 counter average) the contract is restated in numpy and the kernel must match it bit for bit.

Tolerances.  The project's fp32 levels (head_cases.TOL) against float64: forward quantities 1e-5, gradients 1e-4.
  BatchNorm1d   errors PER COLUMN (a column is what one thread group produces), max_b |got - ref| / den.  den = max_b |ref| for y and dx;
                for everything that is a sum whose terms cancel, den = the column's sum of |terms|: save_mean (sum |x| / B), the running
                statistics ((1 - m) |old| + m |new|), dbeta (sum |dy|) and dx_colsum (sum |dx|; analytically ZERO in training mode).
                Conditioning of the inputs: with B == 2 a training-mode BatchNorm maps every column to +-(1 - e), so dx is all cancellation,
                of relative size eps / (var + eps): the B == 2 inputs have a spread of 2^-8 (var <= 1.6e-5, eps = 1e-5), which keeps that
                factor above 0.38 — with unit spread it is 3e-5 and NO fp32 kernel holds 1e-4 of max |dx|; their running mean lives at the
                same scale, or the eval-mode y of two nearly equal rows would be one cancelling value per column.  B == 1: dx == 0 exactly.
                The 16-bit side outputs are the rounding of the kernel's own fp32 dx, bit for bit.
  slab sums     bit-equal to the numpy restatement of each kernel's order, and within 1e-5 of the float64 sum per row, a row being the four
                consecutive outputs one thread produces (den = max |ref| of the row).
  plain GEMMs   exact tier: small-integer operands (exact in fp16 and bf16), K max|a| max|b| < 2^24, so every fp32 partial sum in any
                tile, split or slab order is exact: bit-equal to the float64 product.  Tolerance tier: uniform operands, element-wise
                (K + splits + 2) 2^-24 S with S = sum |terms|, the weight-gradient level of conv_cases (dw_q); an element-wise bound is
                never weaker than a per-row one, and the figure reported is the worst row's.
  everything else (dropout, layout, casts, shadows, the four small entry points) is bit-exact."""
import math

import numpy as np
import torch
import torch.nn.functional as F

import head_cases as hc

f32, f64 = torch.float32, torch.float64
TOL = hc.TOL
TINY = hc.TINY
SENTINEL = hc.SENTINEL
U24 = 2.0 ** -24
uniform = hc.uniform


def cdiv(a, b):
    return -(-a // b)


class Q:
    """one reference quantity: value, tolerance kind ("fwd" | "grad") and, optionally, the per-column denominators"""

    def __init__(self, value, kind, scale=None):
        self.value, self.kind, self.scale = value.detach(), kind, None if scale is None else scale.detach()


def col_err(got, ref, scale=None):
    """per-column max_b |got - ref| / (den + TINY); a [C] vector is one row: every element is a column of its own.  NaN where got is NaN"""
    g, r = got.detach().to("cpu", f64), ref.detach().to("cpu", f64)
    assert g.shape == r.shape, (g.shape, r.shape)
    if g.dim() == 1:
        g, r = g[None], r[None]
    den = r.abs().amax(0) if scale is None else scale.to("cpu", f64).reshape(-1)
    return (g - r).abs().amax(0) / (den + TINY)


def check(got, q, what="", frac=1.0, out=None):
    """assert ``got`` is within ``frac`` of the tolerance of ``q`` in every column; the worst figure (as a fraction of the tolerance) goes to ``out``"""
    err = col_err(got, q.value, q.scale)
    tol = TOL[q.kind]
    worst = float(torch.nan_to_num(err, nan=math.inf).max()) / tol if err.numel() else 0.0
    if out is not None:
        out.append((what, q.kind, worst))
    assert bool((err <= tol * frac).all()), "%s: %s error is %.3g of its tolerance (allowed %.3g), column %d" % (
        what, q.kind, worst, frac, int(torch.nan_to_num(err, nan=1e300).argmax()))


# ================================================================================================ BatchNorm1d
BN_MOMENTUM, BN_EPS = 0.1, 1e-5            # csrc/net.hip: kBnMomentum, kBnEps (passed to the kernels as fp32)
BN_CACHE_ROWS = 128                        # ew.hip: BN1D_NR * BN1D_RG — up to here the rows are held in registers
BN_ROW_GROUPS = 8                          # ew.hip: BN1D_RG
BN_SHAPES = [(1, 8), (2, 64), (7, 72), (8, 100), (9, 512), (127, 100), (128, 72), (129, 64), (200, 8), (128, 512), (129, 100)]
BN_CONST_COL, BN_CONST = 3, 0.75           # a constant column: var == 0, y == beta exactly, rstd == 1 / sqrt(eps)
BN_NEG_COL = 1                             # a negative gamma
_EPS32, _MOM32 = float(np.float32(BN_EPS)), float(np.float32(BN_MOMENTUM))


def bn_uses_cache(B):
    return B <= BN_CACHE_ROWS


def bn_ldt(B):
    """net.hip: the transposed 16-bit gradient is strided by B rounded up to 8 — plus 8, so that ldt > B in every case"""
    return (B + 7) // 8 * 8 + 8


class BnInputs:
    def __init__(self, B, C):
        s = 1000 + 13 * B + C
        self.B, self.C = B, C
        if B == 2:
            x = uniform((B, C), s) * 2.0 ** -8                      # see the module docstring: the conditioning of dx at B == 2
        else:
            x = uniform((B, C), s) + uniform((C,), s + 1, -0.5, 0.5)[None]
        x[:, BN_CONST_COL] = BN_CONST
        self.x, self.dy = x, uniform((B, C), s + 2)
        self.gamma, self.beta = uniform((C,), s + 3, 0.5, 1.5), uniform((C,), s + 4)
        self.gamma[BN_NEG_COL] = -0.75
        self.rm, self.rv = uniform((C,), s + 5, -0.5, 0.5) * (2.0 ** -8 if B == 2 else 1.0), uniform((C,), s + 6, 0.5, 1.5)
        # what the forward pass saves for the backward one, rounded to fp32 from float64 (not taken from the kernel)
        xd = x.double()
        mu = xd.mean(0)
        self.save_mean = mu.float()
        self.save_rstd = (1.0 / torch.sqrt(((xd - mu) ** 2).mean(0) + _EPS32)).float()
        self.eval_rstd = (1.0 / torch.sqrt(self.rv.double() + _EPS32)).float()


def bn_fwd_ref(i, training, use_gamma, use_beta, dt=f64):
    """F.batch_norm at ``dt``; B == 1 in training mode, which F.batch_norm refuses, from the definition with the biased variance in the
    running update (the kernel's documented fall-back: there is no unbiased variance of one value)"""
    x = i.x.to(dt)
    g, b = (i.gamma.to(dt) if use_gamma else None), (i.beta.to(dt) if use_beta else None)
    rm, rv = i.rm.to(dt).clone(), i.rv.to(dt).clone()
    m_abs = None
    if training:
        mean = x.mean(0)
        var = ((x - mean) ** 2).mean(0)
        m_abs = x.abs().mean(0)
        if i.B > 1:
            y = F.batch_norm(x, rm, rv, g, b, True, _MOM32, _EPS32)
        else:
            y = (x - mean) / torch.sqrt(var + _EPS32) * (g if use_gamma else 1.0) + (b if use_beta else 0.0)
            rm, rv = (1 - _MOM32) * rm + _MOM32 * mean, (1 - _MOM32) * rv + _MOM32 * var
    else:
        y = F.batch_norm(x, rm, rv, g, b, False, 0.0, _EPS32)
        mean, var = rm, rv
    if training:
        # var == 0 by construction: xhat == 0 and y == beta by definition (the float64 mean of B equal numbers carries 1e-16 of them, which
        # rstd = 316 and a missing beta would turn into the column's whole value)
        y = y.clone()
        y[:, BN_CONST_COL] = b[BN_CONST_COL] if use_beta else 0.0
    rstd = 1.0 / torch.sqrt(var + _EPS32)
    out = {"y": Q(y, "fwd"), "save_mean": Q(mean, "fwd", m_abs), "save_rstd": Q(rstd, "fwd")}
    if training:
        new_var = (rv - (1 - _MOM32) * i.rv.to(dt)).abs()
        out["rm"] = Q(rm, "fwd", (1 - _MOM32) * i.rm.to(dt).abs() + _MOM32 * m_abs)
        out["rv"] = Q(rv, "fwd", (1 - _MOM32) * i.rv.to(dt).abs() + new_var)
    return out


def bn_fwd_kernel_order(i, training, use_gamma, use_beta, mutant=None):
    """the forward kernel's own arithmetic: float64 sums, fp32 statistics, y = (x - mean) * rstd * g + b in fp32.
    mutant "row_group": the last of the eight row groups is left out of the sums; "biased": running_var takes the biased variance"""
    x = i.x
    g = i.gamma if use_gamma else torch.ones(i.C)
    b = i.beta if use_beta else torch.zeros(i.C)
    rm, rv = i.rm.clone(), i.rv.clone()
    if training:
        xs = x.double()
        if mutant == "row_group":
            xs = xs[torch.arange(i.B) % BN_ROW_GROUPS != BN_ROW_GROUPS - 1]
        mu = xs.sum(0) / i.B
        v = ((xs - mu) ** 2).sum(0)
        mean, rstd = mu.float(), (1.0 / torch.sqrt(v / i.B + _EPS32)).float()
        unb = v / (i.B - 1) if (i.B > 1 and mutant != "biased") else v / i.B
        rm = ((1.0 - _MOM32) * rm.double() + _MOM32 * mu).float()
        rv = ((1.0 - _MOM32) * rv.double() + _MOM32 * unb).float()
    else:
        mean, rstd = rm, (1.0 / torch.sqrt(rv + torch.tensor(BN_EPS, dtype=f32))).to(f32)
    y = (x - mean) * rstd * g + b
    return {"y": y, "save_mean": mean, "save_rstd": rstd, "rm": rm, "rv": rv}


def bn_bwd_stats(i, frozen):
    """(mean, rstd) fp32 the backward kernel is handed: the batch statistics, or — frozen — the running ones"""
    return (i.rm, i.eval_rstd) if frozen else (i.save_mean, i.save_rstd)


def bn_bwd_ref(i, use_gamma, frozen, dt=f64):
    """autograd through F.batch_norm (training mode) or through the affine of the saved constants (frozen: dx = gamma rstd dy)"""
    x = i.x.to(dt).requires_grad_(True)
    dy = i.dy.to(dt)
    g = i.gamma.to(dt) if use_gamma else None
    if frozen:
        mean, rstd = (t.to(dt) for t in bn_bwd_stats(i, True))
        y = (x - mean) * rstd * (g if use_gamma else 1.0)
    elif i.B > 1:
        y = F.batch_norm(x, None, None, g, None, True, 0.0, _EPS32)
    else:
        mean = x.mean(0, keepdim=True)
        y = (x - mean) / torch.sqrt(((x - mean) ** 2).mean(0) + _EPS32) * (g if use_gamma else 1.0)
    (y * dy).sum().backward()
    dx = x.grad
    return {"dx": Q(dx, "grad"), "dbeta": Q(dy.sum(0), "grad", dy.abs().sum(0)), "dx_colsum": Q(dx.sum(0), "grad", dx.abs().sum(0))}


def bn_bwd_kernel_order(i, use_gamma, frozen, mutant=None):
    """the backward kernel's own arithmetic: float64 column sums of fp32 terms, dx = (g rstd) (dy - m1 - xhat m2) in fp32.
    mutant "row_group": the last of the eight row groups is left out of the sums"""
    mean, rstd = bn_bwd_stats(i, frozen)
    g = i.gamma if use_gamma else torch.ones(i.C)
    xh = (i.x - mean) * rstd
    keep = torch.arange(i.B) % BN_ROW_GROUPS != BN_ROW_GROUPS - 1 if mutant == "row_group" else torch.ones(i.B, dtype=torch.bool)
    s1 = i.dy.double()[keep].sum(0)
    s2 = (i.dy.double() * xh.double())[keep].sum(0)
    m1 = torch.zeros(i.C) if frozen else (s1 / i.B).float()
    m2 = torch.zeros(i.C) if frozen else (s2 / i.B).float()
    dx = (g * rstd) * (i.dy - m1 - xh * m2)
    return {"dx": dx, "dbeta": s1.float(), "dx_colsum": dx.double()[keep].sum(0).float()}


# ================================================================================================ split-K slab reduction
SLAB_WIDE_MIN_SPLITS, SLAB_WIDE_MAX_N4 = 16, 65536          # ew.hip: reduce_slabs_launch
SLAB_GRID_CAP = 2048                                        # narrow kernel: blocks of 256 float4


def slabs_wide(nsplit, n):
    return nsplit >= SLAB_WIDE_MIN_SPLITS and n // 4 <= SLAB_WIDE_MAX_N4


# (nsplit, n): one slab, the narrow fold, 16 (two slabs per lane), a ragged lane, 31 / 32 / 33 around the first group of four, one group plus a
# tail, four groups; both sides of the n4 <= 65536 switch at nsplit = 16; the narrow kernel on its third trip around the capped grid
SLAB_CASES = [(1, 4), (2, 1028), (15, 4100), (16, 4), (17, 132), (31, 260), (32, 260), (33, 260), (40, 516), (128, 36864),
              (16, 4 * SLAB_WIDE_MAX_N4), (16, 4 * SLAB_WIDE_MAX_N4 + 4), (2, 4 * (2 * SLAB_GRID_CAP * 256 + 37))]
SLAB_BIAS_CASES = [(ns, 1536, bn) for ns in (2, 17) for bn in (4, 512)]          # (nsplit, n, bias_n) on both kernels
SLAB_PAIR_CASES = [(2, 1028), (33, 260)]                                         # the two-pair launch on both kernels


def slab_inputs(nsplit, n, seed=0):
    return uniform((nsplit, n), 7000 + 31 * nsplit + n % 9973 + seed).numpy()


def slab_bias(bias_n):
    return uniform((bias_n,), 7100 + bias_n).numpy()


def _bias_tile(bias, n):
    return np.tile(bias, cdiv(n, len(bias)))[:n]                                 # element e takes bias[e % bias_n]


def slab_sum_order(slabs, bias=None, skip=None):
    """the kernels' stated order in numpy fp32.  Narrow: ascending left fold.  Wide: lane q takes the slabs q, q + 8, ... — in groups of four
    as (b0 + b1) + (b2 + b3) while four remain, then one at a time — and the eight lanes meet in ascending order.  skip: a slab left out (mutant)"""
    nsplit, n = slabs.shape
    live = [s for s in range(nsplit) if s != skip]
    if slabs_wide(nsplit, n):
        lanes = []
        for q in range(8):
            a = np.zeros(n, np.float32)
            s = q
            while s + 24 < nsplit:
                b = [slabs[t] if t in live else np.zeros(n, np.float32) for t in (s, s + 8, s + 16, s + 24)]
                a = a + ((b[0] + b[1]) + (b[2] + b[3]))
                s += 32
            while s < nsplit:
                if s in live:
                    a = a + slabs[s]
                s += 8
            lanes.append(a)
        a = lanes[0]
        for k in range(1, 8):
            a = a + lanes[k]
    else:
        a = slabs[0].copy() if 0 in live else np.zeros(n, np.float32)
        for s in range(1, nsplit):
            if s in live:
                a = a + slabs[s]
    if bias is not None:
        a = a + _bias_tile(bias, n)
    assert a.dtype == np.float32
    return a


def slab_sum_ref(slabs, bias=None):
    r = slabs.astype(np.float64).sum(0)
    return r + _bias_tile(bias, slabs.shape[1]) if bias is not None else r


def slab_check(got, slabs, bias=None, what="", frac=1.0, out=None):
    """bit-equal to the order restatement AND within 1e-5 of float64 per row of four"""
    got = np.asarray(got)
    ref = slab_sum_ref(slabs, bias).reshape(-1, 4)
    err = np.abs(got.astype(np.float64).reshape(-1, 4) - ref).max(1) / (np.abs(ref).max(1) + TINY)
    worst = float(np.nan_to_num(err, nan=np.inf).max()) / TOL["fwd"]
    if out is not None:
        out.append((what, "fwd", worst))
    assert worst <= frac, "%s: slab sum is %.3g of its tolerance from float64" % (what, worst)
    assert np.array_equal(got, slab_sum_order(slabs, bias)), "%s: not bit-equal to the stated summation order" % what


# ================================================================================================ dropout
M64 = (1 << 64) - 1
DROPOUT_P = [0.1, 0.4, 0.5, 0.9]
DROPOUT_SEEDS = [0, 100, 2 ** 63 + 5]
DROPOUT_STEPS = [0, 1, 7]
DROPOUT_GRID_CAP = 4096                                     # blocks of 256 threads; a thread takes 8 (forward) or 4 (backward) elements
DROPOUT_N = [8, 4104]
DROPOUT_N_FWD_BIG = 8 * (DROPOUT_GRID_CAP * 256 + 300)
DROPOUT_N_BWD_BIG = 4 * (DROPOUT_GRID_CAP * 256 + 300)


def splitmix64(x):
    """the splitmix64 finaliser on a uint64 array (arithmetic modulo 2^64)"""
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def dropout_thr(p):
    return int(np.float32(p) * np.float32(65536.0))


def dropout_key(seed, step):
    return (seed * 0x100000001B3 + step * 0x9E3779B1) & M64


def dropout_mask(n, p, seed, step, field_shift=0):
    """element e is kept (1) iff field e % 4 (16 bits) of splitmix64(key ^ (e / 4)) >= thr.  field_shift: the wrong field (mutant)"""
    e = np.arange(n, dtype=np.uint64)
    h = splitmix64(np.uint64(dropout_key(seed, step)) ^ (e >> np.uint64(2)))
    field = (h >> (((e + np.uint64(field_shift)) & np.uint64(3)) * np.uint64(16))) & np.uint64(0xFFFF)
    return (field >= np.uint64(dropout_thr(p))).astype(np.uint8)


def dropout_inv_keep(p):
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def dropout_values(n, s16, seed=0):
    """16-bit values with no zeros (a dropped element is +0: it must be told from a kept one)"""
    x = uniform((n,), 8000 + seed, 0.25, 2.0) * torch.where(uniform((n,), 8001 + seed) < 0, -1.0, 1.0)
    return x.to(s16)


def dropout_fwd_expect(x16, mask, p):
    """storage(x * 1 / (1 - p)) in fp32 where kept, +0 where dropped"""
    y = (x16.float() * float(dropout_inv_keep(p))).to(x16.dtype)
    return torch.where(torch.from_numpy(mask.astype(bool)), y, torch.zeros_like(y))


def dropout_bwd_expect(dx, mask, p):
    y = dx * float(dropout_inv_keep(p))
    return torch.where(torch.from_numpy(mask.astype(bool)), y, torch.zeros_like(y))


# ================================================================================================ layout and casts
NHWC_SHAPES = [(1, 2, 1), (2, 66, 49), (3, 64, 64), (1, 130, 65), (2, 512, 49)]      # (B, C, HW): ragged 64-pixel and 64-channel tiles
CAST_GRID_CAP = 4096
CAST_N = [13, 8, 72 + 5, 8 * (CAST_GRID_CAP * 256 + 100) + 5]                        # scalar tail only / vector only / both / past the grid cap


def nhwc_ref(x, s16):
    B, C, HW = x.shape
    return x.permute(0, 2, 1).contiguous().to(s16)


def bits16(t):
    return t.contiguous().view(torch.int16)


def cast_edge_values():
    """fp32 values at the rounding edges of both storage types: ties (to even, both ways), the largest finite values and the first that
    round to inf, subnormals of the target and of fp32, +-0, +-inf and a quiet NaN"""
    v = [0.0, -0.0, 1.0, -1.0, math.inf, -math.inf, math.nan,
         1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1 + 2.0 ** -11 + 2.0 ** -23, -(1 + 2.0 ** -11),          # fp16 ties at 1 (down, up), just above a tie
         1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -23, -(1 + 3 * 2.0 ** -8),          # bf16 ties at 1
         65504.0, 65519.996, 65520.0, -65520.0, 65536.0, 1e5,                                        # fp16: max, below / at the tie to inf, beyond
         2.0 ** -14, 2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -25, -(2.0 ** -25), 3 * 2.0 ** -25, 2.0 ** -26, 1023.5 * 2.0 ** -24,   # fp16 subnormals
         2.0 ** -126, 2.0 ** -127, 2.0 ** -133, 2.0 ** -134, 1.5 * 2.0 ** -134, -(2.0 ** -134), 2.0 ** -149, -(2.0 ** -149)]   # fp32 / bf16 subnormals
    t = torch.tensor(v, dtype=f64).to(f32)
    big = torch.tensor([0x7F7FFFFF, 0x7F7F8000, 0x7F7F7FFF, 0x7F7F0000], dtype=torch.int32).view(f32)   # bf16: rounds to inf / tie to inf / below / max
    return torch.cat([t, big, -big])


def cast_input(n, seed=0):
    """n fp32 values: the edge values first (as far as they fit), then random BIT PATTERNS (every exponent, subnormals, infs), NaNs replaced
    by ordinary numbers — a NaN's payload is not part of the contract; the quiet NaN among the edge values is compared as a NaN"""
    g = torch.Generator().manual_seed(9000 + seed)
    x = torch.randint(-2 ** 31, 2 ** 31 - 1, (n,), generator=g, dtype=torch.int64).to(torch.int32).view(f32).clone()
    x = torch.where(torch.isnan(x), torch.full_like(x, 0.3), x)
    e = cast_edge_values()[:n]
    x[:e.numel()] = e
    return x


def same16(got, ref, what=""):
    """bit equality of two 16-bit tensors; a NaN matches a NaN"""
    got, ref = got.cpu(), ref.cpu()
    gn, rn = torch.isnan(got.float()), torch.isnan(ref.float())
    ok = torch.equal(gn, rn) and torch.equal(bits16(got)[~gn], bits16(ref)[~rn])
    assert ok, "%s: not bit-equal (%d elements differ)" % (what, int(((bits16(got) != bits16(ref)) & ~(gn & rn)).sum()))


def shadow_layout(tensors, trainable_count):
    """csrc/net.h: the shadow buffer is the 16-bit mirror of the trainable parameters, then — from the next multiple of 8 — the dgrad-layout
    copy [Cin][taps, flipped][Cout] of every block conv in state_dict order.  tensors: (name, kind, region, offset, shape) per entry;
    returns [(name, w_off, wd_off, Cout, Cin, R)] and the total element count"""
    off = (trainable_count + 7) // 8 * 8
    out = []
    for name, kind, region, offset, shape in tensors:
        if kind == 0 and region == 0 and name.startswith("layer"):
            cout, cin, r = shape[0], shape[1], shape[2]
            out.append((name, offset, off, cout, cin, r))
            off += cin * r * r * cout
    return out, off


def dgrad_shadow_ref(w_krsc, s16):
    """KRSC [Cout][R][S][Cin] -> [Cin][R][S][Cout] with both taps flipped, rounded to the storage type"""
    return w_krsc.flip(1, 2).permute(3, 1, 2, 0).contiguous().to(s16)


# ================================================================================================ plain GEMMs
def nt_bn(N):
    return 64 if N <= 64 else 128


def nt_bm(M, N):
    """gemm.hip: nt_bm — 128-row tiles unless that leaves fewer than 384 of them"""
    return 128 if cdiv(M, 128) * cdiv(N, nt_bn(N)) >= 384 else 64


def gemm_nt_pick_splits(M, N, K):
    """gemm.hip: gemm_nt_pick_splits — 512 workgroups aimed for, at least four K-steps of 64 per split, no empty trailing split"""
    tiles = cdiv(M, nt_bm(M, N)) * cdiv(N, nt_bn(N))
    ksteps = cdiv(K, 64)
    splits = max(min(cdiv(512, tiles), ksteps // 4), 1)
    return cdiv(ksteps, cdiv(ksteps, splits))


def gemm_nt_glds_applies(N, K, splits, nt_glds=4):
    """gemm_nt_glds.hip: gemm_nt_glds_applies for a plain problem — the ring kernel pays from 16 K-steps per workgroup"""
    pays = bool(nt_glds & 8) or cdiv(cdiv(K, 64), splits) >= 16
    return (nt_glds & 7) > 0 and N > 64 and pays


def nt_expected(M, N, K, nt_glds=4):
    """(profile slot, K-splits) of fedfr_gemm_nt: slot 17 = the ring kernel, 0..3 = gemm_nt tiles <128,128> <128,64> <64,128> <64,64>"""
    splits = gemm_nt_pick_splits(M, N, K)
    if gemm_nt_glds_applies(N, K, splits, nt_glds):
        return 17, splits
    return (0 if nt_bm(M, N) == 128 else 2) + (0 if nt_bn(N) == 128 else 1), splits


def tn_expected_slot(NI, NJ):
    """gemm.hip: gemm_tn_tiles + prof_slot — 4..7 = gemm_tn tiles <128,128> <128,64> <64,128> <64,64>; a plain problem is one launch, one split"""
    return 4 + (0 if NI > 64 else 2) + (0 if NJ > 64 else 1)


SLAB_SLOT = 25                                              # ew.hip: the profile slot of the slab reduction
# (M, N, K) -> (slot, splits) the row is there for (test_tail_cases_cpu holds the restated rules to this table)
NT_ROWS = [((1, 132, 72), (2, 1)),                          # <64,128>, one K-step and a tail of 8
           ((65, 4, 8), (3, 1)),                            # <64,64>, two row tiles, K below one step
           ((2945, 2048, 72), (0, 1)),                      # <128,128>: 24 x 16 = 384 tiles
           ((49025, 60, 72), (1, 1)),                       # <128,64>: 384 tiles, N not a multiple of 8
           ((7, 132, 584), (2, 2)),                         # two splits of five K-steps, the second ending in the tail
           ((4, 512, 25088), (2, 98)),                      # the fc forward: 98 splits through the wide slab reduction
           ((1024, 1024, 4104), (17, 4))]                   # the ring kernel (17 K-steps per workgroup), K tail
TN_ROWS = [((1, 512, 64), 5), ((1, 8, 25088), 6), ((129, 72, 136), 4), ((200, 8, 64), 7)]      # (Kp, NI, NJ) -> slot; Kp = 1: a one-image batch


def gemm_operands(rows, cols, K, exact, s16, seed):
    """[rows][K] and [cols][K] fp32 values representable in the storage type: small integers (exact tier) or rounded uniform numbers"""
    g = torch.Generator().manual_seed(seed)
    if exact:
        a = torch.randint(-2, 3, (rows, K), generator=g).to(f32)
        b = torch.randint(-1, 2, (cols, K), generator=g).to(f32)
    else:
        a = (torch.rand((rows, K), generator=g) * 2 - 1).to(s16).to(f32)
        b = (torch.rand((cols, K), generator=g) * 2 - 1).to(s16).to(f32)
    return a, b


GEMM_EXACT_AMAX, GEMM_EXACT_BMAX = 2, 1


def gemm_exact_admissible(K):
    """every partial sum of every output, in any order, is an integer below 2^24"""
    return K * GEMM_EXACT_AMAX * GEMM_EXACT_BMAX < 2 ** 24


def gemm_ref(a, b, dt=f64, k_drop=0):
    """C[m][n] = sum_k a[m][k] b[n][k] and S = sum_k |a||b| (runs on whatever device the operands are on).  k_drop: columns left off (mutant)"""
    K = a.shape[1] - k_drop
    a, b = a[:, :K].to(dt), b[:, :K].to(dt)
    return a @ b.t(), a.abs() @ b.abs().t()


def gemm_row_ratio(got, ref, S, K, splits):
    """per row, max_n |got - ref| / ((K + splits + 2) 2^-24 S); 0 / 0 = 0, NaN = inf"""
    e = (got.to(f64) - ref).abs()
    r = e / ((K + splits + 2) * U24 * S)
    r = torch.where(e == 0, torch.zeros_like(r), r)
    return torch.nan_to_num(r, nan=math.inf).amax(1)


def gemm_check(got, ref, S, K, splits, exact, what="", frac=1.0, out=None):
    if exact:
        assert torch.equal(got.to(f64), ref), "%s: not bit-equal to the float64 product (%d elements differ)" % (what, int((got.to(f64) != ref).sum()))
        return
    r = gemm_row_ratio(got, ref, S, K, splits)
    worst = float(r.max())
    if out is not None:
        out.append((what, "gemm", worst))
    assert worst <= frac, "%s: error is %.3g of its tolerance (allowed %.3g), row %d" % (what, worst, frac, int(r.argmax()))


# ================================================================================================ the four small entry points
def fedavg_i64_order(acc, src, w, accumulate):
    """acc (+)= w * float(src), every step rounded to fp32: the conversion (counters above 2^24 round), the product, the sum; then the
    truncation toward zero back to int64"""
    s = src.astype(np.float32)
    t = np.float32(w) * s
    v = (acc if accumulate else np.zeros_like(acc)) + t
    assert v.dtype == np.float32
    return v, np.trunc(v).astype(np.int64)


def fedavg_i64_inputs(n):
    g = np.random.default_rng(50 + n)
    src = g.integers(0, 2 ** 24, n, dtype=np.int64)
    special = np.array([2 ** 24 + 1, 2 ** 24 + 3, 2 ** 31 + 129, 123456789, 2 ** 40 + 2 ** 16 + 1, 7, 0], dtype=np.int64)
    src[:min(n, len(special))] = special[:n]
    return src, g.random(n, dtype=np.float32) * np.float32(1000.0)


def pfc_rand_order(n, seed, step):
    """perm[i] = (top 32 bits of splitmix64(seed * 0x100000001B3 + step * 0x9E3779B1 + i * 0xD6E8FEB86659FD93) >> 8) * 2^-24"""
    with np.errstate(over="ignore"):
        i = np.arange(n, dtype=np.uint64)
        h = splitmix64(np.uint64(dropout_key(seed, step)) + i * np.uint64(0xD6E8FEB86659FD93))
    return ((h >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)


def pfc_localize_ref(label, class_start, num_local, perm):
    """partial_fc.py:91-98: labels of this shard become local ids and mark perm[id] = 2.0, the rest become -1"""
    loc = label - class_start
    ok = (loc >= 0) & (loc < num_local)
    out = torch.where(ok, loc, torch.full_like(loc, -1))
    if perm is not None:
        perm = perm.clone()
        perm[out[ok]] = 2.0
    return out, perm
