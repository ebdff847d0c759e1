"""Inputs and references for the server-optimiser kernels (csrc/optim.hip: fedopt_sqnorm_kernel, fedopt_multi_kernel).

Two forms of the same formulas (include/fedfr_hip.h, the fedfr_fedopt_multi comment):

* ``delta32`` / ``step32``: a numpy float32 restatement, ONE operation per line in the kernel's order.  numpy's float32 + - * / sqrt are
  single correctly rounded IEEE operations, as the kernel's are (nothing is contracted into an fma), so the kernel is held to these
  BIT FOR BIT (tests/test_fedopt_gpu.py).
* ``delta64`` / ``step64``: the formulas evaluated in float64 on the same fp32 inputs and fp32 hyper-parameters.

``fp64_bound`` is the tolerance of the fp32 result against the fp64 one on ``inputs(..., same_sign=True)``:
(k + 16) 2^-24 (|x| + |u| + |m| + sum_i |coef_i d_i|), u the applied step.  tests/test_fedopt_cpu.py shows that the restatement alone meets
it on exactly the inputs the GPU test uses: the inputs are conditioned for it (client deltas and m share one sign per element, so neither
Delta nor m' cancels) and the bound hides nothing a correct fp32 kernel would not produce.  Nothing here imports the package.
"""
import functools

import numpy as np

f32, f64 = np.float32, np.float64
KINDS = {"AVGM": 0, "ADAGRAD": 1, "ADAM": 2, "YOGI": 3}
GRID_CAP = 2048                     # the launchers' grid cap (fedavg_multi's rule)
SIZES = (1, 3, 4, 5, 1023, 4103, GRID_CAP * 256 * 4 + 5)      # tail only, < one float4, one float4, float4 + tail, < / > one block, grid-stride wrap + tail
KS = (1, 2, 3, 8)
U = 2.0 ** -24                      # fp32 unit roundoff


def grid(n):
    """blocks of 256 threads the launchers use for n elements: min(ceil((n / 4 + 1) / 256), 2048)"""
    return min((n // 4 + 1 + 255) // 256, GRID_CAP)


def hyper(lr=1.0, beta1=0.9, beta2=0.99, tau=1e-3):
    """(lr, beta1, 1 - beta1, beta2, 1 - beta2, tau) in fp32, (1 - beta) formed in fp32: what the host passes to the kernel"""
    lr, b1, b2, tau = f32(lr), f32(beta1), f32(beta2), f32(tau)
    return lr, b1, f32(1) - b1, b2, f32(1) - b2, tau


def weights(k):
    """dataset-size weights n_i / sum n, rounded to fp32 as the host does"""
    sizes = [300.0 + 37.0 * ((5 * i) % 7) for i in range(k)]
    return [f32(s / sum(sizes)) for s in sizes]


@functools.lru_cache(maxsize=None)
def inputs(n, k, tau=1e-3, same_sign=False, tag=0.0):
    """closed-form (x, [x_1..x_k], m, v): sin-type, v >= tau^2.  same_sign: every client's delta and m carry the sign s_j of element j.
    Computed once per argument set and shared (read-only arrays)."""
    j = np.arange(n, dtype=f64)
    x = (0.5 * np.sin(0.37 * j + 0.1 + tag)).astype(f32)
    s = np.where(np.sin(0.77 * j + 0.3) >= 0, 1.0, -1.0)
    xs = []
    for i in range(k):
        if same_sign:
            d = s * 0.05 * (0.2 + np.abs(np.sin(0.091 * (i + 1) * j + 0.5 * i + 0.3 + tag)))
        else:
            d = 0.05 * np.sin(0.091 * (i + 1) * j + 0.5 * i + 0.3 + tag)       # (no client's delta is zero at j = 0)
        xs.append((x.astype(f64) + d).astype(f32))
    if same_sign:
        m = (s * 0.02 * (0.1 + np.abs(np.sin(0.53 * j + 0.7)))).astype(f32)
    else:
        m = (0.02 * np.sin(0.53 * j + 0.7)).astype(f32)
    t = f32(tau)
    v = (f64(t * t) + 1e-3 * (1.0 + np.sin(0.29 * j + 1.1))).astype(f32)
    v = np.maximum(v, t * t)
    for a in [x, m, v] + xs:
        a.flags.writeable = False
    return x, tuple(xs), m, v


# ---- float32, one operation per line --------------------------------------------------------------------------------------------------
def delta32(x, xs, coef, start=None):
    d = np.zeros_like(x) if start is None else start.copy()
    for xi, c in zip(xs, coef):
        t = xi - x
        t = f32(c) * t
        d = d + t
    return d


def step32(kind, x, m, v, d, h):
    """(m', v', x') of one step; v' is None for AVGM"""
    lr, b1, c1, b2, c2, tau = h
    assert all(a.dtype == f32 for a in (x, m, d)) and all(type(a) is f32 for a in h)
    if kind == "AVGM":
        t = b1 * m
        m1 = t + d
        u = lr * m1
        return m1, None, x + u
    t = b1 * m
    g = c1 * d
    m1 = t + g
    d2 = d * d
    if kind == "ADAGRAD":
        v1 = v + d2
    elif kind == "ADAM":
        a = b2 * v
        b = c2 * d2
        v1 = a + b
    else:
        e = v - d2
        sg = np.sign(e).astype(f32)
        b = c2 * d2
        b = b * sg
        v1 = v - b
    num = lr * m1
    r = np.sqrt(v1)
    den = r + tau
    u = num / den
    x1 = x + u
    assert m1.dtype == f32 and v1.dtype == f32 and x1.dtype == f32
    return m1, v1, x1


def run32(kind, x, xs, coef, m, v, h):
    return step32(kind, x, m, v, delta32(x, xs, coef), h)


# ---- float64 evaluation of the same formulas ---------------------------------------------------------------------------------------------
def delta64(x, xs, coef):
    """(Delta, sum_i |coef_i d_i|) in fp64 from the fp32 inputs"""
    x = x.astype(f64)
    d, mag = np.zeros_like(x), np.zeros_like(x)
    for xi, c in zip(xs, coef):
        t = f64(c) * (xi.astype(f64) - x)
        d, mag = d + t, mag + np.abs(t)
    return d, mag


def step64(kind, x, m, v, d, h):
    """(m', v', x', u) in fp64; u = the applied step"""
    lr, b1, c1, b2, c2, tau = (f64(a) for a in h)
    x, m, d = x.astype(f64), m.astype(f64), d.astype(f64)
    if kind == "AVGM":
        m1 = b1 * m + d
        u = lr * m1
        return m1, None, x + u, u
    v = v.astype(f64)
    m1 = b1 * m + c1 * d
    d2 = d * d
    if kind == "ADAGRAD":
        v1 = v + d2
    elif kind == "ADAM":
        v1 = b2 * v + c2 * d2
    else:
        v1 = v - c2 * d2 * np.sign(v - d2)
    u = lr * m1 / (np.sqrt(v1) + tau)
    return m1, v1, x + u, u


def fp64_bound(k, x, m, u, mag):
    return (k + 16) * U * (np.abs(x.astype(f64)) + np.abs(u) + np.abs(m.astype(f64)) + mag)


# ---- update norms and clipped coefficients ---------------------------------------------------------------------------------------------------
def sqnorm(x, xs):
    """sq_i = sum_j (double) (x_i[j] - x[j] in fp32)^2, summed in fp64 (numpy's pairwise order)"""
    return np.array([np.sum((xi - x).astype(f64) ** 2) for xi in xs], dtype=f64)


def clip_coef64(sq, ws, clip):
    """w_i min(1, clip / sqrt(sq_i)) in fp64 (clip <= 0 or sq_i == 0: w_i)"""
    out = []
    for s, w in zip(sq, ws):
        c = f64(w)
        if clip > 0 and s > 0:
            c = c * min(1.0, f64(f32(clip)) / np.sqrt(s))
        out.append(c)
    return np.array(out, dtype=f64)


def clip_coef(sq, ws, clip):
    return clip_coef64(sq, ws, clip).astype(f32)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)
