"""The restatements of tests/drift_cases.py are the arithmetic the header states (DRIFT TERMS), sharp enough to reject every mutant, and the
algorithm they drive is SCAFFOLD: the step mass undoes heavy-ball momentum exactly, and the minimiser of the summed loss with c_i = grad f_i
there is a fixed point of the round, where FedAvg drifts.  No GPU."""
import numpy as np
import pytest

import drift_cases as Dc
import step_cases as S
from fedfr_amd import client

f32, f64 = np.float32, np.float64
N = 4103
LR, MU, WD = S.SGD_HYPER


def _kw(kind):
    anchor, corr = Dc.drift_inputs(N)
    has_a, has_c = Dc.KINDS[kind]
    return {"anchor": anchor if has_a else None, "a": Dc.DRIFT_A if has_a else 0.0, "corr": corr if has_c else None}


@pytest.mark.parametrize("first", [1, 0])
def test_drift_ref_without_terms_is_sgd_ref(first):
    p, g = S.sgd_inputs(N)
    buf = None if first else S.sgd_two_steps(N)[0][1]
    for gs in (None, S.SGD_SCALE):
        gin = g if gs is None else (g / f32(gs)).astype(f32)
        if gs is not None:
            gin[[0, 5, N - 1]] = S.sgd_bad_values(3)
        want = S.sgd_ref(p, gin, buf, LR, MU, WD, first, gs=gs)
        got = Dc.drift_ref(p, gin, buf, LR, MU, WD, first, gs=gs)
        for w, g_, what in zip(want[:3], got[:3], ("p", "buf", "g")):
            S.same32(g_, w, "drift_ref without terms, %s" % what, nan_ok=True)
        assert want[3] == got[3]


@pytest.mark.parametrize("kind", sorted(Dc.KINDS))
def test_drift_ref_is_within_four_roundings_of_fp64(kind):
    """two chained steps against the fp64 evaluation of the same formula from the same fp32 state: per step at most four fp32 roundings
    reach buf (d0, the subtraction, d1, d — or d and the two of the momentum) and one more p, each at most 2^-24 of a magnitude below
    M = max(|p|, |g|, |buf|, |corr|, ...) <= 4 here; the bound asserted is 4 roundings of M on p (lr < 1 scales buf's) and 5 on buf"""
    p, g = S.sgd_inputs(N)
    kw = _kw(kind)
    p1, b1, _, _ = Dc.drift_ref(p, g, None, LR, MU, WD, 1, **kw)
    q1, c1 = Dc.drift_ref64(p, g, None, LR, MU, WD, 1, **kw)
    M = 4.0
    assert max(np.abs(q1).max(), np.abs(c1).max()) < M
    assert np.abs(p1 - q1).max() <= 4 * Dc.U * M and np.abs(b1 - c1).max() <= 5 * Dc.U * M
    g2 = S.sgd_second_grad(N)
    p2, b2, _, _ = Dc.drift_ref(p1, g2, b1, LR, MU, WD, 0, **kw)
    q2, c2 = Dc.drift_ref64(p1, g2, b1, LR, MU, WD, 0, **kw)
    assert max(np.abs(q2).max(), np.abs(c2).max()) < M
    assert np.abs(p2 - q2).max() <= 4 * Dc.U * M and np.abs(b2 - c2).max() <= 5 * Dc.U * M


@pytest.mark.parametrize("mutant", Dc.DRIFT_MUTANTS)
def test_every_drift_mutant_differs_on_the_shared_inputs(mutant):
    """on the inputs the GPU test feeds: the mutant's (p, buf) after the two chained steps is not the restatement's"""
    p, g = S.sgd_inputs(N)
    (p1, b1), (p2, b2) = Dc.drift_two_steps(N, "both")
    kw = _kw("both")
    m1 = Dc.drift_ref(p, g, None, LR, MU, WD, 1, mutant=mutant, **kw)
    m2 = Dc.drift_ref(p1, S.sgd_second_grad(N), b1, LR, MU, WD, 0, mutant=mutant, **kw)
    differs = [not np.array_equal(S.bits32(m), S.bits32(w)) for m, w in ((m1[0], p1), (m1[1], b1), (m2[0], p2), (m2[1], b2))]
    assert any(differs[:2]) and any(differs[2:]), (mutant, differs)


@pytest.mark.parametrize("mutant", ["corr_added", "unfused"])
def test_scaffold_control_mutants_differ(mutant):
    ci, x, y, corr = Dc.control_inputs(1025)
    inv = Dc.inv_mass32(Dc.CONTROL_MASS)
    cn, dc = Dc.scaffold_control_ref(ci, x, y, corr, inv)
    mn, md = Dc.scaffold_control_ref(ci, x, y, corr, inv, mutant=mutant)
    assert not np.array_equal(S.bits32(cn), S.bits32(mn)) and not np.array_equal(S.bits32(dc), S.bits32(md))
    c0, d0 = Dc.scaffold_control_ref(ci, x, y, None, inv)
    S.same32(c0, Dc.scaffold_control_ref(ci, x, y, np.zeros_like(x), inv)[0], "a null corr reads as +0.0")
    S.same32(d0, c0 - ci, "dc = cn - c_i")


def _lrs(K):
    """a learning rate that changes mid-run (a tenth from the second half on)"""
    return [0.1 if k < (K + 1) // 2 else 0.01 for k in range(K)]


@pytest.mark.parametrize("mu", [0.0, 0.9])
@pytest.mark.parametrize("K", [1, 2, 8])
def test_step_mass_recovers_a_constant_gradient(K, mu):
    """a linear loss (gradient g0 whatever p is, wd = 0) run through drift_ref for K momentum steps: (x - y) / mass = g0 to relative 1e-5
    (at most 8 steps of 3 roundings of 2^-24 each: 1.5e-6); the trainer's running sum (client.step_mass_term) is the restated mass; K lr
    misses at mu = 0.9 as soon as there is a second step"""
    x = S.uniform((257,), 4030).numpy()
    g0 = (S.uniform((257,), 4031).numpy() * f32(0.25) + f32(0.5)).astype(f32)            # in [0.25, 0.75]: relative errors are meaningful
    lrs = _lrs(K)
    p, buf = x, None
    mass = 0.0
    for k, lr in enumerate(lrs):
        p, buf, _, _ = Dc.drift_ref(p, g0, buf, lr, mu, 0.0, k == 0)
        mass += client.step_mass_term(lr, mu, k + 1)
    assert abs(mass - Dc.step_mass(lrs, mu)) <= 1e-15 * mass
    rec = (x.astype(f64) - p.astype(f64)) / mass
    assert np.abs(rec / g0 - 1.0).max() <= 1e-5
    cn, _ = Dc.scaffold_control_ref(np.zeros_like(x), x, p, None, Dc.inv_mass32(mass))
    assert np.abs(cn / g0 - 1.0).max() <= 1e-5
    wrong = (x.astype(f64) - p.astype(f64)) / Dc.step_mass(lrs, mu, "k_lr")
    if mu == 0.0 or K == 1:
        assert np.abs(wrong / g0 - 1.0).max() <= 1e-5
    else:
        assert np.abs(wrong / g0 - 1.0).min() > 1e-2                                   # (mass / K lr - 1: 0.08 at K = 2, 1.5 at K = 8)


def test_step_mass_term_and_prox_mu_checks():
    assert client.step_mass_term(0.1, 0.0, 7) == 0.1
    assert abs(client.step_mass_term(0.1, 0.9, 3) - 0.1 * (1 + 0.9 + 0.81)) < 1e-16
    assert client.check_prox_mu(None, "t") == 0.0 and client.check_prox_mu(0, "t") == 0.0 and client.check_prox_mu(0.01, "t") == 0.01
    for bad in (-0.1, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="prox_mu"):
            client.check_prox_mu(bad, "t")
    assert client.DriftTerms() == (None, 0.0, None)


def test_scaffold_fixed_point_and_fedavg_drift():
    """three clients, heterogeneous diagonal quadratics, four momentum steps: started at the minimiser w* of sum f_i with c_i = grad f_i(w*)
    and c = their mean, the SCAFFOLD round of the fp32 restatements stays where its fp64 evaluation stays — inside that evaluation's own
    fp32 rounding bound (drift_cases.quad_round64; printed below: a few 1e-7) — and that evaluation itself moves off w* by no more than the
    rounding of w* and c_i to fp32 allows (the fixed point is exact only in exact arithmetic).  A FedAvg round from the same point moves
    away by more than 100 times the bound: with c_i != 0 every client runs towards its own minimum, and the curvatures differ."""
    w, cis, c = Dc.quad_fixed_point()
    x32, c32, ci32, _ = Dc.quad_round32(w, c, list(cis))
    x64, e_x, ci64, e_ci = Dc.quad_round64(w, c, list(cis))
    bound = float(e_x.max())
    drift32 = float(np.abs(x32.astype(f64) - w).max())
    print("SCAFFOLD: |x' - w*| = %.3g (fp32), %.3g (fp64); |x'32 - x'64| = %.3g; rounding bound %.3g"
          % (drift32, float(np.abs(x64 - w).max()), float(np.abs(x32 - x64).max()), bound))
    assert bound < 1e-5
    assert (np.abs(x32.astype(f64) - x64) <= e_x).all()
    for i in range(Dc.QUAD_CLIENTS):
        assert (np.abs(ci32[i].astype(f64) - ci64[i]) <= e_ci[i]).all()
        # c_i stays grad f_i(w*): the fp64 round returns it up to the fp32 rounding of the inputs (|w*|, |c_i| < 2: a few 2^-24, through
        # a gain of at most a_i mass / mass + 1 <= 2) plus the bound
        assert np.abs(ci64[i] - cis[i]).max() <= 16 * Dc.U + float(e_ci[i].max())
    assert float(np.abs(x64 - w).max()) <= 16 * Dc.U
    assert float(np.abs(c32.astype(f64) - c).max()) <= 3 * float(max(e.max() for e in e_ci)) + 16 * Dc.U
    xa, _, _, ys = Dc.quad_round32(w, c, list(cis), scaffold=False)
    moved = float(np.abs(xa.astype(f64) - w).max())
    print("FedAvg: |x' - w*| = %.3g = %.0f x the bound" % (moved, moved / bound))
    assert moved > 100 * bound and moved > 100 * drift32
