"""Inputs and references for the reweighted rules (csrc/reweight.hip: reweight_step_kernel, reweight_weights_kernel): the geometric median
(RFA) and centred clipping.  The formulas are the ones include/fedfr_hip.h states for fedfr_reweight_step / fedfr_reweight_weights.

* ``step32``: a numpy float32 restatement of the step pass.  delta_i = x_i - z; acc = z; for i ascending, where beta_i != 0:
  acc = acc + beta_i * delta_i (one float32 multiply, one float32 add); z' = acc; then D_i = sum_e (double) (x_i[e] - z'[e] in float32)^2
  for EVERY client, numpy's fp64 dot product.  numpy's float32 - * + are single correctly rounded IEEE operations, as the kernel's are, so the
  kernel's z' is held to this BIT FOR BIT; its D_i to ``robust_cases.pairdist_bound`` (the terms are exact and non-negative).
* ``weights64``: the weights kernel, operation by operation in fp64 (sqrt, /, max, min and the ascending sum are single correctly rounded
  operations on both sides), each beta rounded to float32 once: held bit for bit.
* ``round32``: a round as the server runs it (distance-only pass, then R weighted steps) on step32 / weights64.
* ``round64``: the same round with every quantity in fp64 and no rounding of the weights: the reference of the conditioning check.

Nothing here imports the package.
"""
import numpy as np

import robust_cases as R

f32, f64 = np.float32, np.float64
GEOMEDIAN, CCLIP = 0, 1
RULES = {"GeoMedian": GEOMEDIAN, "CenteredClip": CCLIP}
U = 2.0 ** -24                      # fp32 unit roundoff
# (n, k, f) of the conditioning check and of the chain tests: ``krum_inputs`` (the last f clients are planted outliers, one of them +-1e30)
ROUND_CASES = ((4103, 5, 1), (1023, 8, 2), (4103, 16, 3), (1023, 32, 7))
ROUND_ITERS = (1, 3, 8)


def base(n, tag=0.0):
    """z0 of the tests: the sine base of ``robust_cases.inputs`` (the global parameters the clients trained from), float32, read-only"""
    j = np.arange(n, dtype=f64)
    z = (0.5 * np.sin(0.37 * j + 0.1 + tag)).astype(f32)
    z.flags.writeable = False
    return z


def sqdist64(xs, z):
    """D_i = sum_e (double) (x_i[e] - z[e] in float32)^2"""
    out = np.zeros(len(xs), dtype=f64)
    with np.errstate(invalid="ignore", over="ignore"):
        for i, x in enumerate(xs):
            e = (x - z).astype(f64)
            out[i] = np.dot(e, e)
    return out


def step32(z, xs, beta=None):
    """(z', D): one step pass.  ``beta`` None is the distance-only mode (z' is z itself)"""
    assert z.dtype == f32 and all(x.dtype == f32 for x in xs)
    if beta is None:
        return z, sqdist64(xs, z)
    beta = np.asarray(beta, dtype=f32)
    acc = z.copy()
    with np.errstate(invalid="ignore", over="ignore"):
        for i, x in enumerate(xs):
            if beta[i] != 0:                       # a SELECT: a skipped client's NaN / inf never reaches acc
                t = beta[i] * (x - z)
                acc = acc + t
    assert acc.dtype == f32
    return acc, sqdist64(xs, acc)


def weights64(rule, D, alpha, param, tau=None):
    """(beta float32 [k], S, tau, number of finite clients) from the squared distances D.  ``param``: nu (GeoMedian), tau or 0 = auto
    (CenteredClip); auto takes ``tau`` if given (a later slot of the round) and else the lower median of the finite d_i (slot 0)"""
    D, alpha = np.asarray(D, dtype=f64), np.asarray(alpha, dtype=f64)
    k = D.size
    fin = np.isfinite(D)
    nf = int(fin.sum())
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        d = np.where(fin, np.sqrt(np.where(fin, D, 0.0)), np.inf)
        beta = np.zeros(k, dtype=f32)
        S = f64(0.0)
        if rule == CCLIP:
            if param == 0.0:
                if tau is None:
                    tau = float(np.sort(d[fin])[(nf - 1) // 2]) if nf else 0.0
            else:
                tau = float(param)
            for i in range(k):
                if fin[i]:
                    q = f64(tau) / d[i]
                    r = f64(1.0) if d[i] == 0.0 else (q if q < 1.0 else f64(1.0))
                    beta[i] = f32(alpha[i] * r)
                S = S + f64(beta[i])
            return beta, float(S), tau, nf
        w = np.zeros(k, dtype=f64)
        for i in range(k):
            if fin[i]:
                w[i] = alpha[i] / (d[i] if d[i] > param else f64(param))
            S = S + w[i]
        if S > 0.0:
            beta = (w / S).astype(f32)
    return beta, float(S), None, nf


def round32(z0, xs, alpha, rule, iters, param):
    """the round of the server: (z, D history (iters + 1) x k, beta history iters x k, tau)"""
    k = len(xs)
    Dh, Bh = np.zeros((iters + 1, k), dtype=f64), np.zeros((iters, k), dtype=f32)
    z, Dh[0] = step32(z0, xs)
    tau = None
    for s in range(iters):
        Bh[s], _, tau, _ = weights64(rule, Dh[s], alpha, param, tau)
        z, Dh[s + 1] = step32(z, xs, Bh[s])
    return z, Dh, Bh, tau


def round64(z0, xs, alpha, rule, iters, param):
    """the same round in fp64 throughout (states, centre, distances, weights): the exact iteration up to fp64 rounding.  Clients that are
    not finite in fp64 get weight 0, as in the kernels"""
    X = [x.astype(f64) for x in xs]
    alpha = np.asarray(alpha, dtype=f64)
    z = z0.astype(f64)
    tau = None
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for s in range(iters):
            D = np.array([np.dot(x - z, x - z) for x in X])
            fin = np.isfinite(D)
            d = np.where(fin, np.sqrt(np.where(fin, D, 0.0)), np.inf)
            if rule == CCLIP:
                if tau is None:
                    tau = float(param) if param != 0.0 else (float(np.sort(d[fin])[(int(fin.sum()) - 1) // 2]) if fin.any() else 0.0)
                b = np.where(fin, alpha * np.where(d == 0.0, 1.0, np.minimum(1.0, tau / np.where(d == 0.0, 1.0, d))), 0.0)
            else:
                w = np.where(fin, alpha / np.maximum(param, d), 0.0)
                b = w / w.sum() if w.sum() > 0 else w
            acc = z.copy()
            for i in range(len(X)):
                if b[i] != 0:
                    acc = acc + b[i] * (X[i] - z)
            z = acc
    return z


def honest_scale(z0, xs, nhonest):
    """max |x| over the centre and the honest clients: the magnitude the rounding of a step is relative to (a planted +-1e30 client enters a
    step only through beta_i (x_i - z), a term of the honest magnitude: its weight is ~ 1 / |x_i - z|)"""
    return float(max(np.abs(z0).max(), max(np.abs(x).max() for x in xs[:nhonest])))
