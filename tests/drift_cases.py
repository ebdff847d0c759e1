"""Restatements, inputs and mutants for the drift terms of the SGD kernels (include/fedfr_hip.h: DRIFT TERMS) — FedProx's proximal pull and
SCAFFOLD's control-variate correction — and for SCAFFOLD's end-of-round pass.  tests/test_drift_cpu.py proves the restatements sharp and the
algorithm right; tests/test_drift_gpu.py holds the kernels, the trainers and the server rounds to them.  Nothing here touches the GPU library.

  drift_ref             one call of sgd_kernel<UNSCALE, ANCHOR, CORR> in numpy, every operation one fp32 rounding (step_cases.fma32):
                            d0 = fma(wd, p, g); d1 = anchor ? fma(a, fsub(p, anchor), d0) : d0; d = corr ? fadd(d1, corr) : d1;
                            buf = first ? d : fadd(fmul(buf, mu), d); p = fma(-lr, buf, p)
                        with the guard of the UNSCALE instantiations (gs given): an element whose unscaled gradient is not finite keeps p and buf.
  scaffold_control_ref  t = fsub(x, y); cn = fma(inv_mass, t, -corr); dc = fsub(cn, c_i); c_i = cn  (corr None reads as +0.0)
  step_mass             sum_k lr_k (1 - mu^k) / (1 - mu) in fp64: the weight heavy-ball momentum gives the gradients of a run
  quad_*                three clients with diagonal quadratic losses, for whole SCAFFOLD / FedAvg rounds driven by the restatements"""
import functools

import numpy as np

import step_cases as S

f32, f64 = np.float32, np.float64
U = 2.0 ** -24                                             # unit roundoff of fp32

DRIFT_A = 0.43                                             # the proximal coefficient of the bit-exact tier: O(1), like S.SGD_HYPER
DRIFT_MUTANTS = ("prox_before_wd", "unfused_prox", "corr_subtracted", "corr_after_momentum")
KINDS = {"anchor": (True, False), "corr": (False, True), "both": (True, True)}          # x guarded or not = the six new instantiations


def drift_ref(p, g, buf, lr, mu, wd, first, anchor=None, a=0.0, corr=None, gs=None, mutant=None):
    """(p', buf', g', overflow) of one kernel call.  mutant: one of DRIFT_MUTANTS"""
    lr, mu, wd, a = f32(lr), f32(mu), f32(wd), f32(a)
    p, g = np.asarray(p, f32), np.asarray(g, f32)
    b0 = np.zeros_like(p) if first else np.asarray(buf, f32)
    with np.errstate(all="ignore"):
        if gs is not None:
            g = g * f32(gs)
        if anchor is not None and mutant == "prox_before_wd":
            d1 = S.fma32(wd, p, S.fma32(a, p - np.asarray(anchor, f32), g))
        else:
            d1 = S.fma32(wd, p, g)
            if anchor is not None:
                t = p - np.asarray(anchor, f32)
                d1 = (d1 + a * t) if mutant == "unfused_prox" else S.fma32(a, t, d1)
        d = d1
        late = None
        if corr is not None:
            c = np.asarray(corr, f32)
            if mutant == "corr_subtracted":
                d = d1 - c
            elif mutant == "corr_after_momentum":
                late = c
            else:
                d = d1 + c
        b = d if first else (b0 * mu) + d
        pn = S.fma32(-lr, b if late is None else b + late, p)
        assert d.dtype == f32 and b.dtype == f32 and pn.dtype == f32
        ovf = 0
        if gs is not None:
            bad = ~np.isfinite(g)
            pn, b = np.where(bad, p, pn), np.where(bad, b0, b)
            ovf = int(bad.any())
    return pn.astype(f32), b.astype(f32), g, ovf


def drift_ref64(p, g, buf, lr, mu, wd, first, anchor=None, a=0.0, corr=None):
    """the same formula evaluated in fp64 from the fp32 inputs and fp32 hyper-parameters: (p', buf')"""
    lr, mu, wd, a = (f64(f32(v)) for v in (lr, mu, wd, a))
    p, g = np.asarray(p, f64), np.asarray(g, f64)
    d = wd * p + g
    if anchor is not None:
        d = d + a * (p - np.asarray(anchor, f64))
    if corr is not None:
        d = d + np.asarray(corr, f64)
    b = d if first else np.asarray(buf, f64) * mu + d
    return p - lr * b, b


@functools.lru_cache(maxsize=None)
def drift_inputs(n):
    """(anchor, corr): the anchor near the parameters of S.sgd_inputs(n) (p - anchor is a quarter of p's range), corr like a gradient"""
    p, _ = S.sgd_inputs(n)
    anchor = (p + (S.uniform((n,), 4003 + n % 9973) * 0.25).numpy()).astype(f32)
    corr = (S.uniform((n,), 4004 + n % 9973) * 0.25).numpy()
    anchor.setflags(write=False)
    corr.setflags(write=False)
    return anchor, corr


@functools.lru_cache(maxsize=None)
def drift_two_steps(n, kind, hyper=S.SGD_HYPER):
    """[(p1, buf1), (p2, buf2)] for kind in KINDS: first = 1, then first = 0 with S.sgd_second_grad(n), on the same buffers"""
    p, g = S.sgd_inputs(n)
    anchor, corr = drift_inputs(n)
    has_a, has_c = KINDS[kind]
    kw = {"anchor": anchor if has_a else None, "a": DRIFT_A if has_a else 0.0, "corr": corr if has_c else None}
    lr, mu, wd = hyper
    p1, b1, _, _ = drift_ref(p, g, None, lr, mu, wd, 1, **kw)
    p2, b2, _, _ = drift_ref(p1, S.sgd_second_grad(n), b1, lr, mu, wd, 0, **kw)
    return (p1, b1), (p2, b2)


# ================================================================================================ SCAFFOLD's end-of-round pass
CONTROL_GRID_CAP = 2048                                    # multi_state.h: multi_state_grid — blocks of 256 threads, one float4 each
CONTROL_N = [1, 3, 4, 5, 1023, 1025, CONTROL_GRID_CAP * 256 * 4 + 7]      # the last: the second round of that grid rule, plus a tail of three


def scaffold_control_ref(ci, x, y, corr, inv_mass, mutant=None):
    """(c_i', dc).  mutant "corr_added": cn = fma(inv_mass, t, +corr); "unfused": cn = fl(fl(inv_mass t) - corr)"""
    ci, x, y = (np.asarray(v, f32) for v in (ci, x, y))
    r = np.zeros_like(x) if corr is None else np.asarray(corr, f32)
    t = x - y
    if mutant == "unfused":
        cn = f32(inv_mass) * t - r
    else:
        cn = S.fma32(f32(inv_mass), t, r if mutant == "corr_added" else -r)
    dc = cn - ci
    assert t.dtype == f32 and cn.dtype == f32 and dc.dtype == f32
    return cn, dc


@functools.lru_cache(maxsize=None)
def control_inputs(n):
    """(c_i, x, y, corr), read-only: y a trained copy of x a few learning rates away"""
    ci, x = (S.uniform((n,), 4010 + n % 9973) * 0.25).numpy(), S.uniform((n,), 4011 + n % 9973).numpy()
    y = (x + (S.uniform((n,), 4012 + n % 9973) * 0.125).numpy()).astype(f32)
    corr = (S.uniform((n,), 4013 + n % 9973) * 0.25).numpy()
    for v in (ci, x, y, corr):
        v.setflags(write=False)
    return ci, x, y, corr


CONTROL_MASS = 0.4524                                      # a step mass of the size four steps at lr 0.05, mu 0.9 give


def step_mass(lrs, mu, mutant=None):
    """sum_k lr_k (1 - mu^k) / (1 - mu), k = 1 ... len(lrs), in fp64.  mutant "k_lr": sum_k lr_k, SCAFFOLD's K lr (right at mu = 0 only)"""
    mu = float(mu)
    if mutant == "k_lr":
        return float(sum(float(lr) for lr in lrs))
    return float(sum(float(lr) * sum(mu ** j for j in range(k)) for k, lr in enumerate(lrs, start=1)))


def inv_mass32(mass):
    return f32(1.0 / float(mass))


# ================================================================================================ whole rounds on diagonal quadratics
# f_i(w) = 1/2 sum_j a_ij (w_j - b_ij)^2, three clients, equal weights.  grad f_i = a_i (w - b_i): fl(a_i fl(w - b_i)) in the fp32 restatement
QUAD_CLIENTS, QUAD_DIM, QUAD_STEPS = 3, 64, 4
QUAD_LR, QUAD_MU = 0.05, 0.9


@functools.lru_cache(maxsize=None)
def quad_problem():
    """(a [3][D] in [0.25, 1], b [3][D] in [-1, 1]), fp32; the curvatures differ between the clients (that is the heterogeneity FedAvg drifts on)"""
    g = np.random.default_rng(4020)
    a = g.uniform(0.25, 1.0, (QUAD_CLIENTS, QUAD_DIM)).astype(f32)
    b = g.uniform(-1.0, 1.0, (QUAD_CLIENTS, QUAD_DIM)).astype(f32)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


def quad_fixed_point():
    """(w*, c_i = grad f_i(w*), c = mean c_i) rounded to fp32 from their fp64 values: w* = sum a_i b_i / sum a_i minimises sum f_i"""
    a, b = (v.astype(f64) for v in quad_problem())
    w = (a * b).sum(0) / a.sum(0)
    ci = a * (w - b)
    return w.astype(f32), ci.astype(f32), ci.mean(0).astype(f32)


def quad_round32(x, c, cis, scaffold=True, mass_mutant=None, lr=QUAD_LR, mu=QUAD_MU, steps=QUAD_STEPS):
    """one round in the fp32 restatements: every client runs ``steps`` momentum steps of drift_ref from x (corr = c - c_i under SCAFFOLD),
    then scaffold_control_ref; the server averages the models as fedavg_multi does (d = fl(d + fl(w y_i)), ascending i, from 0) and adds
    (1 / N) sum dc_i to c the same way.  Returns (x', c', [c_i'], [y_i])"""
    a, b = quad_problem()
    ys, new_ci, dcs = [], [], []
    inv = inv_mass32(step_mass([lr] * steps, mu, mass_mutant))
    for i in range(QUAD_CLIENTS):
        corr = (np.asarray(c, f32) - np.asarray(cis[i], f32)) if scaffold else None
        p, buf = np.asarray(x, f32), None
        for k in range(steps):
            g = a[i] * (p - b[i])
            assert g.dtype == f32
            p, buf, _, _ = drift_ref(p, g, buf, lr, mu, 0.0, k == 0, corr=corr)
        ys.append(p)
        if scaffold:
            cn, dc = scaffold_control_ref(cis[i], x, p, corr, inv)
            new_ci.append(cn)
            dcs.append(dc)
    w = f32(1.0 / QUAD_CLIENTS)
    xn = np.zeros_like(ys[0])
    for y in ys:
        xn = S.axpy_ref(xn, y, w, True)
    cn = np.asarray(c, f32)
    for dc in dcs:
        cn = S.axpy_ref(cn, dc, w, True)
    return xn, cn, new_ci, ys


def quad_round64(x, c, cis, lr=QUAD_LR, mu=QUAD_MU, steps=QUAD_STEPS):
    """the same SCAFFOLD round evaluated in fp64 from the same fp32 inputs and fp32 constants, carrying beside every fp64 value a bound on
    what the fp32 restatement's roundings can have put between itself and that value (first order in U, magnitudes taken from the fp64
    values and inflated by 1 + 2^-10 to cover the second order):
        t = fl(p - b):        e_t = e_p + U |t|            g = fl(a t):          e_g = a e_t + U |g|
        d = fl(g + corr):     e_d = e_g + U |d|            (fma(0, p, g) = g: the weight decay is off)
        m = fl(buf mu):       e_m = mu e_buf + U |m|        buf = fl(m + d):     e_buf = e_m + e_d + U |buf|   (first step: buf = d)
        p = fma(-lr, buf, p): e_p = e_p + lr e_buf + U |p|
        control pass:         t = fl(x - y): e_y + U |t|;  cn = fma(inv, t, -corr): inv e_t + U |cn|
        server:               per client fl(w y): w e_y + U |w y|, then the running sum: + U |sum|
    corr = fl(c - c_i) is formed once in fp32 on both sides and enters exactly.  Returns (x', e_x, [c_i'], [e_ci])"""
    a, b = (v.astype(f64) for v in quad_problem())
    lr64, mu64 = f64(f32(lr)), f64(f32(mu))
    inv = f64(inv_mass32(step_mass([lr] * steps, mu)))
    infl = 1.0 + 2.0 ** -10
    w = f64(f32(1.0 / QUAD_CLIENTS))
    x64 = np.asarray(x, f64)
    xn, e_x = np.zeros_like(x64), np.zeros_like(x64)
    out_ci, out_e = [], []
    for i in range(QUAD_CLIENTS):
        corr = (np.asarray(c, f32) - np.asarray(cis[i], f32)).astype(f64)
        p, e_p = x64.copy(), np.zeros_like(x64)
        buf, e_buf = None, None
        for k in range(steps):
            t = p - b[i]
            e_t = e_p + U * np.abs(t) * infl
            g = a[i] * t
            e_g = a[i] * e_t + U * np.abs(g) * infl
            d = g + corr
            e_d = e_g + U * np.abs(d) * infl
            if k == 0:
                buf, e_buf = d, e_d
            else:
                m = buf * mu64
                e_m = mu64 * e_buf + U * np.abs(m) * infl
                buf = m + d
                e_buf = e_m + e_d + U * np.abs(buf) * infl
            p = p - lr64 * buf
            e_p = e_p + lr64 * e_buf + U * np.abs(p) * infl
        t = x64 - p
        cn = inv * t - corr
        out_ci.append(cn)
        out_e.append(inv * (e_p + U * np.abs(t) * infl) + U * np.abs(cn) * infl)
        xn = xn + w * p
        e_x = e_x + w * e_p + U * np.abs(w * p) * infl + U * np.abs(xn) * infl
    return xn, e_x, out_ci, out_e
