"""Inputs and references for the direct tests of the fp32 head kernels (csrc/head.hip).

Every case is a ``Case``: seeded (or closed-form) fp32 inputs plus ``ref(dtype)``, the operation written as a plain torch formula on those
inputs converted to ``dtype``.  ``ref(torch.float64)`` is the answer the kernels are held to (tests/test_head_kernels_gpu.py);
``ref(torch.float32)`` is the same formula at the kernels' own precision, which tests/test_host_cpu.py holds to a QUARTER of every
tolerance: the inputs are conditioned well enough for a correct fp32 kernel to pass, and the tolerances hide nothing.  Nothing here
imports the oracle: the formulas come from the reference's definitions (F.normalize, losses.py, F.cross_entropy, partial_fc.py, the BCE
comment block of head.hip), not from the project's own restatement of them.

Tolerances (the project's fp32 head levels, against fp64): forward quantities and exact-fp32 GEMM results 1e-5, gradients 1e-4, scalar
losses 1e-5 * max(1, |ref|).  The error of a matrix is taken PER ROW, max_c |got - ref| / (max_c |ref| + 1e-30), never over the whole
tensor, so a wrong row of small magnitude cannot hide behind a large one; an element of a vector with one entry per row (inv, row_max,
row_sum) is a row of its own.  Two per-row scalars are single elements of a row whose other elements the kernel never stores, and are
measured against that row's maximum like any other element of it: prob_t = p[row][label] against max_c p[row] (a target probability may
be 1e-60: exp() in fp32 cannot carry a relative error there, and no fp32 softmax has one), and dmul = d logit / d cos at the target
against max(|dmul|, s), s being that derivative at every other column (ArcFace's crosses zero where th + m = pi).
"""
import math

import torch

f32, f64 = torch.float32, torch.float64
TOL = {"fwd": 1e-5, "grad": 1e-4, "loss": 1e-5}
TINY = 1e-30
EPS = 1e-12                 # F.normalize's eps
FLOOR = 1e-30               # PartialFC's clamp_min on the target probability
SENTINEL = -777.25          # what ld padding is filled with before a call


def uniform(shape, seed, lo=-1.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g, dtype=f32) * (hi - lo) + lo


class Q:
    """one reference quantity: value, tolerance kind ("fwd" | "grad" | "loss" | "exact") and, optionally, the per-row denominators"""

    def __init__(self, value, kind, scale=None):
        self.value, self.kind, self.scale = value, kind, scale


class Case:
    def __init__(self, name, inputs, ref):
        self.name, self.inputs, self._ref = name, inputs, ref

    def ref(self, dtype=f64):
        return self._ref(dtype)


def _rows(t):
    t = t.detach().to("cpu", f64)
    if t.dim() == 0:
        return t.reshape(1, 1)
    if t.dim() == 1:
        return t.reshape(-1, 1)
    return t.reshape(-1, t.shape[-1])


def row_err(got, ref, scale=None):
    """per-row max_c |got - ref| / (max_c |ref| + TINY) (``scale``: the denominators, one per row); NaN where got is NaN"""
    g, r = _rows(got), _rows(ref)
    assert g.shape == r.shape, (g.shape, r.shape)
    den = r.abs().amax(1) if scale is None else scale.detach().to("cpu", f64).reshape(-1)
    return (g - r).abs().amax(1) / (den + TINY)


def check(got, q, what="", frac=1.0, out=None):
    """assert ``got`` equals reference quantity ``q`` within ``frac`` of its tolerance; prints the figure first when ``out`` is a list"""
    ref = q.value
    if q.kind == "exact":
        ok = torch.equal(got.detach().cpu().to(ref.dtype).reshape(ref.shape), ref)
        assert ok, "%s: not equal" % what
        return
    if q.kind == "loss":
        g, r = _rows(got).reshape(-1), _rows(ref).reshape(-1)
        fin = torch.isfinite(r)
        assert torch.equal(g[~fin], r[~fin]), "%s: non-finite entries differ" % what
        err = ((g[fin] - r[fin]).abs() / r[fin].abs().clamp_min(1.0))
    else:
        err = row_err(got, ref, q.scale)
    worst = float(err.max()) if err.numel() else 0.0
    if out is not None:
        out.append((what, q.kind, worst))
    tol = TOL[q.kind] * frac
    assert bool((err <= tol).all()), "%s: %s error %.3g > %.3g (row %d)" % (what, q.kind, worst, tol, int(torch.nan_to_num(err, nan=1e300).argmax()))


def label_sets(R, C):
    """label vectors that together hold the four kinds every case needs: -1, C (the first value out of range), C - 1 and 0"""
    kinds = [-1, C, C - 1, 0]
    if R >= 4:
        g = torch.Generator().manual_seed(7 * R + C)
        rest = torch.randint(0, C, (R - 4,), generator=g).tolist()
        return [torch.tensor(kinds + rest, dtype=torch.int64)]
    n = -(-4 // R)
    return [torch.tensor([kinds[(i * R + j) % 4] for j in range(R)], dtype=torch.int64) for i in range(n)]


# ------------------------------------------------------------------------------------------------ normalise
NORM_SHAPES = [(1, 1), (3, 63), (5, 64), (7, 65), (4, 512), (9, 513), (6, 1100)]


def normalize_ref(x, dtype):
    x = x.to(dtype)
    eps = torch.tensor(EPS, dtype=f32).to(dtype)
    inv = 1.0 / torch.sqrt((x * x).sum(1)).clamp_min(eps)
    return {"xn": Q(x * inv[:, None], "fwd"), "inv": Q(inv, "fwd")}


def normalize_case(R, D):
    x = uniform((R, D), 100 + D) * 3.0
    if R >= 3:
        x[1] = 0.0                                        # -> xn == 0, inv == 1 / eps exactly
        x[2] = 1e-20 * torch.sign(x[2] + 1e-3)            # -> the clamp (||x|| < eps), not inf
    return Case("normalize[%d,%d]" % (R, D), {"x": x}, lambda dt: normalize_ref(x, dt))


def normalize_bwd_case(R, D, nslab, beta):
    x = uniform((R, D), 200 + D).double() * 3.0
    n = x.norm(dim=1)
    xn, inv = (x / n[:, None]).float(), (1.0 / n).float()
    slabs = uniform((nslab, R, D), 300 + D + nslab)
    dx_old = uniform((R, D), 400 + D)

    def ref(dt):
        g = slabs[0].to(dt)
        for k in range(1, nslab):
            g = g + slabs[k].to(dt)
        a, iv = xn.to(dt), inv.to(dt)
        dx = iv[:, None] * (g - a * (a * g).sum(1, keepdim=True))
        return {"dx": Q(dx + beta * dx_old.to(dt) if beta != 0 else dx, "grad")}
    return Case("normalize_bwd[%d,%d,nslab=%d,beta=%g]" % (R, D, nslab, beta), {"xn": xn, "inv": inv, "slabs": slabs, "dx_old": dx_old}, ref)


# ------------------------------------------------------------------------------------------------ margin + softmax + gradient
MARGIN_CFGS = [(30.0, 0.4, 0), (64.0, 0.4, 0), (30.0, 0.4, 1), (64.0, 0.5, 1)]
SOFTMAX_C = [1, 2, 255, 256, 257, 1000, 1024, 1025, 4096, 4097]


def _margin_cos(t, m, arc):
    return math.cos(math.acos(t) + m) if arc else t - m


def softmax_inputs(R, C, cfg, label, seed=0):
    """cosines uniform in [-0.95, 0.95].  ArcFace m = 0.5: the target of the row labelled C - 1 is -0.95 (th + m > pi, negative
    d logit / d cos).  C == 2 in closed form: the other column sits within 0.05 of the target's margined cosine, or p_target would be 1 to
    fp32 precision and the gradient row all rounding error — an ill-conditioned input, not a kernel property."""
    s, m, arc = cfg
    cos = uniform((R, C), 500 + 3 * C + R + seed, -0.95, 0.95)
    for r in range(R):
        y = int(label[r])
        if not 0 <= y < C:
            continue
        if arc and m == 0.5 and y == C - 1:
            cos[r, y] = -0.95
        if C == 2:
            t = float(cos[r, y]) if (arc and m == 0.5 and y == C - 1) else 0.5 + 0.02 * r
            cos[r, y] = t
            mc, d = _margin_cos(float(cos[r, y]), m, arc), (0.03 if r % 2 else -0.05)
            cos[r, 1 - y] = mc + (abs(d) if mc + d < -0.95 else d)
    return cos


def softmax_ref(cos, label, cfg, inv_batch, dtype):
    s, m, arc = cfg
    x = cos.to(dtype)
    R, C = x.shape
    valid = (label >= 0) & (label < C)
    idx = label.clamp(0, C - 1)
    onehot = torch.zeros(R, C, dtype=torch.bool)
    onehot[valid, idx[valid]] = True
    if arc:
        th = torch.acos(x)
        logits = s * torch.cos(torch.where(onehot, th + m, th))
        tht = th.gather(1, idx[:, None])[:, 0]
        dm = s * torch.sin(tht + m) / torch.sin(tht)
    else:
        logits = s * (x - m * onehot.to(dtype))
        dm = torch.full((R,), s, dtype=dtype)
    dmul = torch.where(valid, dm, torch.full_like(dm, s))
    mx = logits.amax(1)
    e = torch.exp(logits - mx[:, None])
    sm = e.sum(1)
    p = e / sm[:, None]
    zero = torch.zeros(R, dtype=dtype)
    prob_t = torch.where(valid, p.gather(1, idx[:, None])[:, 0], zero)
    num = torch.where(valid, e.gather(1, idx[:, None])[:, 0], zero)
    mul = torch.where(onehot, dmul[:, None].expand(R, C), torch.full_like(x, s))
    grad = (p - onehot.to(dtype)) * inv_batch * mul
    zt = logits.gather(1, idx[:, None])[:, 0]
    nll = torch.where(valid, (mx - zt) + torch.log(sm), torch.full_like(mx, float("inf")))
    ratio_loss = -torch.log((num / sm).clamp_min(torch.tensor(FLOOR, dtype=f32).to(dtype))).mean()
    return {"logits": Q(logits, "fwd"), "row_max": Q(mx, "fwd"), "row_sum": Q(sm, "fwd"),
            "dmul": Q(dmul, "grad", scale=dmul.abs().clamp_min(s)), "prob_t": Q(prob_t, "fwd", scale=p.amax(1)),
            "grad": Q(grad, "grad"), "nll_t": Q(nll, "loss"),
            "num": Q(num, "fwd", scale=e.amax(1)), "ratio_loss": Q(ratio_loss, "loss"), "valid": Q(valid, "exact")}


def softmax_cases(C, cfg):
    out = []
    for R in (1, 5):
        for i, lab in enumerate(label_sets(R, C)):
            cos = softmax_inputs(R, C, cfg, lab)
            out.append(Case("softmax[C=%d,R=%d,set%d,s=%g,m=%g,arc=%d]" % ((C, R, i) + cfg), {"cos": cos, "label": lab, "cfg": cfg, "inv_batch": 1.0 / R},
                            lambda dt, cos=cos, lab=lab, R=R: softmax_ref(cos, lab, cfg, 1.0 / R, dt)))
    return out


SHARDED_R = [1, 70, 300]
SHARDED_CFGS = [(64.0, 0.4, 0), (30.0, 0.4, 1)]


def sharded_case(R, cfg):
    """one shard of the class-sharded softmax: labels already localised, -1 = the row's class lives on another rank.  Row 0 under s = 64
    CosFace: target cosine -0.9 against +0.9 elsewhere, a gap of 140.8 — its numerator underflows fp32 and the loss is -log(floor)."""
    C = 130
    g = torch.Generator().manual_seed(900 + R)
    lab = torch.randint(0, C, (R,), generator=g)
    lab[1::3] = -1
    cos = uniform((R, C), 910 + R, -0.95, 0.95)
    if cfg[0] == 64.0:
        lab[0] = 5
        cos[0, 5], cos[0, 6] = -0.9, 0.9
    return Case("sharded[R=%d,s=%g,arc=%d]" % (R, cfg[0], cfg[2]), {"cos": cos, "label": lab, "cfg": cfg, "inv_batch": 1.0 / R},
                lambda dt: softmax_ref(cos, lab, cfg, 1.0 / R, dt))


def ce_case():
    """dense cross-entropy on s = 64 CosFace logits; row 0 is badly mislabelled: target cosine -0.9, another class +0.9, so the target
    logit is 140.8 below the row maximum and its softmax probability (8e-62) is 0 in fp32"""
    R, C, s, m = 4, 300, 64.0, 0.4
    lab = torch.tensor([5, 17, C - 1, 0])
    cos = uniform((R, C), 77, -0.95, 0.95)
    cos[0, 5], cos[0, 6] = -0.9, 0.9
    onehot = torch.zeros(R, C)
    onehot[torch.arange(R), lab] = 1.0
    logits = ((cos - m * onehot) * s).contiguous()

    def ref(dt):
        z = logits.to(dt)
        lse = torch.logsumexp(z, 1)
        loss = (lse - z.gather(1, lab[:, None])[:, 0]).mean()
        grad = (torch.softmax(z, 1) - onehot.to(dt)) / R
        return {"loss": Q(loss, "loss"), "grad": Q(grad, "grad")}
    return Case("dense_ce[s=64,gap=140.8]", {"logits": logits, "label": lab, "cos": cos}, ref)


# ------------------------------------------------------------------------------------------------ small reductions
REDUCE_N = [1, 63, 64, 255, 256, 257, 1000]
COLSUM_SHAPES = [(1, 1), (7, 63), (128, 65), (3, 1000)]


def nll_mean_case(n, floor):
    p = torch.pow(10.0, uniform((n,), 600 + n, -6.0, 0.0))
    if floor > 0:
        p[0] = 0.0                                         # -> -log(floor)

    def ref(dt):
        return {"loss": Q(-torch.log(p.to(dt).clamp_min(torch.tensor(floor, dtype=f32).to(dt))).mean(), "loss")}
    return Case("nll_mean[n=%d,floor=%g]" % (n, floor), {"p": p, "floor": floor}, ref)


def sum_scale_case(n, scale):
    x = uniform((n,), 610 + n, 0.0, 2.0)
    return Case("sum_scale[n=%d,scale=%g]" % (n, scale), {"x": x, "scale": scale},
                lambda dt: {"out": Q(x.to(dt).sum() * torch.tensor(scale, dtype=f32).to(dt), "loss")})


def colsum_case(R, C):
    x = uniform((R, C), 620 + C)
    return Case("colsum[%d,%d]" % (R, C), {"x": x}, lambda dt: {"out": Q(x.to(dt).sum(0, keepdim=True), "fwd")})


# ------------------------------------------------------------------------------------------------ margin backward
MARGIN_BWD_SHAPES = [(1, 1), (5, 257), (3, 1000)]


def margin_bwd_cases(R, C):
    s = 30.0
    out = []
    for i, lab in enumerate(label_sets(R, C)):
        dlogits = uniform((R, C), 700 + C + i)
        dmul = uniform((R,), 710 + C + i, -1.5, 1.5) * s * 0.7          # differs from s in every row, sign included

        def ref(dt, dlogits=dlogits, dmul=dmul, lab=lab):
            onehot = torch.zeros(R, C, dtype=torch.bool)
            v = (lab >= 0) & (lab < C)
            onehot[v, lab[v]] = True
            return {"dcos": Q(dlogits.to(dt) * torch.where(onehot, dmul.to(dt)[:, None].expand(R, C), torch.full((R, C), s, dtype=dt)), "grad")}
        out.append(Case("margin_bwd[%d,%d,set%d]" % (R, C, i), {"dlogits": dlogits, "dmul": dmul, "label": lab, "s": s}, ref))
    return out


# ------------------------------------------------------------------------------------------------ BCE head
BCE_SHAPES = [(1, 1), (5, 255), (3, 257), (2, 1000)]
BCE_M, BCE_R, BCE_LOSS_SCALE = 0.4, 30.0, 2.0


def bce_cases(B, C, t, lam):
    """z = r (g(cos) -/+ m) + bias with g(x) = 2 ((x + 1) / 2)^t - 1, gt = (label == c), dz/dcos = r t ((x + 1) / 2)^(t - 1);
    row_loss = sum_c (gt ? (lam / r) log(1 + e^-z + 1e-8) : ((1 - lam) / r) log(1 + e^z + 1e-8)), dz = d(loss_scale * mean_b row_loss) / dz,
    dcos = dz * dz/dcos.  The loss kernel is fed the fp64 reference's logits rounded to fp32, so each kernel answers for itself."""
    m, r, ls = BCE_M, BCE_R, BCE_LOSS_SCALE
    out = []
    for i, lab in enumerate(label_sets(B, C)):
        cos = uniform((B, C), 800 + C + i, -0.99, 0.99)
        bias = uniform((C,), 810 + C, -0.5, 0.5)
        pos = torch.zeros(B, C, dtype=torch.bool)
        v = (lab >= 0) & (lab < C)
        pos[v, lab[v]] = True

        def logits(dt, cos=cos, bias=bias, pos=pos):
            hb = (cos.to(dt) + 1.0) * 0.5
            pw1 = hb ** (t - 1.0)
            g = 2.0 * pw1 * hb - 1.0
            return r * torch.where(pos, g - m, g + m) + bias.to(dt), r * t * pw1
        z_in, dzdcos_in = (a.float() for a in logits(f64))

        def ref(dt, pos=pos, logits=logits, z_in=z_in, dzdcos_in=dzdcos_in):
            z, dzdcos = logits(dt)
            zz = z_in.to(dt)
            e = torch.exp(torch.where(pos, -zz, zz))
            w = torch.where(pos, torch.full_like(zz, lam / r), torch.full_like(zz, (1.0 - lam) / r))
            le = w * torch.log(1.0 + e + 1e-8)
            dz = w * torch.where(pos, -e, e) / (1.0 + e + 1e-8) * (ls / B)
            return {"z": Q(z, "fwd"), "gt": Q(pos.to(torch.uint8), "exact"), "dzdcos": Q(dzdcos, "grad"), "row_loss": Q(le.sum(1), "loss"),
                    "dz": Q(dz, "grad"), "dcos": Q(dz * dzdcos_in.to(dt), "grad")}
        out.append(Case("bce[%d,%d,set%d,t=%g,lam=%g]" % (B, C, i, t, lam),
                        {"cos": cos, "bias": bias, "label": lab, "z": z_in, "dzdcos": dzdcos_in, "gt": pos.to(torch.uint8), "t": float(t), "lam": lam}, ref))
    return out


# ------------------------------------------------------------------------------------------------ GEMM
GEMM_MN = (65, 67)
GEMM_K = [1, 3, 127, 128, 129]
GEMM_LAYOUTS = [(False, False), (False, True), (True, False), (True, True)]
# (alpha, beta, bias, ld padding)
GEMM_OPTIONS = [(1.0, 0.0, False, 0), (1.0, 0.0, True, 0), (1.0, 0.5, False, 0), (-2.0, 0.0, False, 0), (1.0, 0.0, False, 5), (-2.0, 0.5, True, 5)]


def gemm_case(M, N, K, ta, tb, alpha, beta, use_bias, k_range=None):
    """alpha * op(A) @ op(B) (+ bias) (+ beta * C_old); a [K, M] if ta else [M, K], b [N, K] if tb else [K, N] (row-major storage)"""
    seed = 1000 + 7 * K + 2 * ta + tb
    a = uniform((K, M) if ta else (M, K), seed)
    b = uniform((N, K) if tb else (K, N), seed + 1)
    bias, c_old = uniform((N,), seed + 2), uniform((M, N), seed + 3)
    lo, hi = k_range if k_range is not None else (0, K)

    def ref(dt):
        A = (a.t() if ta else a).to(dt)[:, lo:hi]
        Bm = (b.t() if tb else b).to(dt)[lo:hi]
        c = alpha * (A @ Bm)
        if use_bias:
            c = c + bias.to(dt)
        if beta != 0:
            c = c + beta * c_old.to(dt)
        return {"c": Q(c, "fwd")}
    name = "gemm[%dx%dx%d,ta=%d,tb=%d,alpha=%g,beta=%g,bias=%d,k=%d:%d]" % (M, N, K, ta, tb, alpha, beta, use_bias, lo, hi)
    return Case(name, {"a": a, "b": b, "bias": bias, "c_old": c_old}, ref)


SPLITK = dict(M=65, N=67, K=300, splits=3, alpha=-2.0)


def splitk_chunk(K, splits):
    return -(-(-(-K // splits)) // 32) * 32


def splitk_cases(tb):
    M, N, K, splits, alpha = (SPLITK[k] for k in ("M", "N", "K", "splits", "alpha"))
    kc = splitk_chunk(K, splits)
    return [gemm_case(M, N, K, False, tb, alpha, 0.0, False, (z * kc, min(K, (z + 1) * kc))) for z in range(splits)]


# ------------------------------------------------------------------------------------------------ everything (the CPU conditioning test)
def all_cases():
    for R, D in NORM_SHAPES:
        yield normalize_case(R, D)
        for nslab in (1, 2, 5):
            for beta in (0.0, 1.0, -0.5):
                yield normalize_bwd_case(R, D, nslab, beta)
    for C in SOFTMAX_C:
        for cfg in MARGIN_CFGS:
            yield from softmax_cases(C, cfg)
    for R in SHARDED_R:
        for cfg in SHARDED_CFGS:
            yield sharded_case(R, cfg)
    yield ce_case()
    for n in REDUCE_N:
        yield nll_mean_case(n, 0.0)
        yield nll_mean_case(n, FLOOR)
        yield sum_scale_case(n, 1.0 / n)
        yield sum_scale_case(n, -3.0)
    for R, C in COLSUM_SHAPES:
        yield colsum_case(R, C)
    for R, C in MARGIN_BWD_SHAPES:
        yield from margin_bwd_cases(R, C)
    for B, C in BCE_SHAPES:
        for t in (1, 3):
            for lam in (0.5, 0.9):
                yield from bce_cases(B, C, t, lam)
    M, N = GEMM_MN
    for K in GEMM_K:
        for ta, tb in GEMM_LAYOUTS:
            for alpha, beta, use_bias, _ in GEMM_OPTIONS:
                yield gemm_case(M, N, K, ta, tb, alpha, beta, use_bias)
    for tb in (False, True):
        yield from splitk_cases(tb)
