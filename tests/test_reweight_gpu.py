"""Reweighted aggregation on the GPU: fedfr_reweight_step / fedfr_reweight_weights through the C ABI against the restatements of
tests/reweight_cases.py (the new centre and the weights bit for bit, the squared distances within the derived fp64 summation bound), whole
rounds replayed step by step from the kernels' own intermediate results and held to the fp64 iteration within the bound
tests/test_reweight_cpu.py conditions, argument errors, and the Python surface (server.FedReweighted, Server.train with
aggr_alg="GeoMedian" / "CenteredClip")."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import reweight_cases as W  # noqa: E402
import robust_cases as R  # noqa: E402
from oracle import ref_cpu as O  # noqa: E402

from fedfr_amd import _C, client, server  # noqa: E402

DEV = torch.device("cuda:0")
f32, f64 = np.float32, np.float64
SENT = -777.25
GUARD = 4                                      # sentinel elements behind a buffer (it stays 16-byte aligned in front of them)


def G(a):
    return torch.from_numpy(np.array(a)).to(DEV)          # (a copy: the shared inputs are read-only arrays)


def N(t):
    return t.detach().cpu().numpy()


def sent(n, dtype=torch.float32):
    return torch.full((n,), SENT, dtype=dtype, device=DEV)


def ptr(t):
    return None if t is None else t.data_ptr()


def ptrs_of(ts):
    return (C.c_void_p * max(len(ts), 1))(*[ptr(t) for t in ts])


def new_ws(k, n, fill=SENT):
    nws = _C.lib().fedfr_reweight_workspace_bytes(k, n)
    assert nws == 8 * k * R.grid(n)
    return torch.full((nws // 8,), fill, dtype=torch.float64, device=DEV)


def step(dst, z, xs, beta, wsp, n=None, k=None, ws_bytes=None):
    """fedfr_reweight_step on device tensors; returns the return code"""
    n = z.numel() if n is None else n
    return _C.lib().fedfr_reweight_step(ptr(dst), ptr(z), ptrs_of(xs), ptr(beta), len(xs) if k is None else k, n, ptr(wsp),
                                        (0 if wsp is None else wsp.numel() * 8) if ws_bytes is None else ws_bytes, _C.stream())


def weights(rule, alpha, param, slot, iters, k, n, wsp, hd, hb, info, ws_bytes=None):
    al = None if alpha is None else (C.c_double * len(alpha))(*[float(a) for a in alpha])
    return _C.lib().fedfr_reweight_weights(rule, al, float(param), slot, iters, k, n, ptr(wsp),
                                           (0 if wsp is None else wsp.numel() * 8) if ws_bytes is None else ws_bytes, ptr(hd), ptr(hb), ptr(info),
                                           _C.stream())


def finished_D(k, n, wsp):
    """the squared distances a step left in ``wsp``, finished by the weights kernel (ascending block order)"""
    hd, hb, info = sent(k + 1, torch.float64), sent(k + 1), sent(5, torch.float64)
    assert weights(W.GEOMEDIAN, [1.0 / k] * k, 1e-6, 0, 1, k, n, wsp, hd, hb, info) == 0, _C.last_error()
    torch.cuda.synchronize()
    assert N(hd)[k] == SENT and N(hb)[k] == f32(SENT) and N(info)[4] == SENT
    return N(hd)[:k]


def some_beta(k):
    """weights of mixed size with exact zeros among them (clients 1 and k - 2, where there are that many)"""
    b = ((np.arange(k) % 5 + 1.0) / (3.0 * k)).astype(f32)
    if k > 2:
        b[1] = 0.0
        b[k - 2] = 0.0
    return b


def check_D(D, xs, z, n, what):
    ref = W.sqdist64(xs, z)
    fin = np.isfinite(ref)
    assert np.array_equal(np.isfinite(D), fin), (what, D, ref)
    err = np.abs(D[fin] - ref[fin])
    assert np.all(err <= R.pairdist_bound(n, ref[fin])), (what, float(np.max(err / np.maximum(R.pairdist_bound(n, ref[fin]), 1e-300))))


def check_step(xs, z, beta, what):
    """out of place, then in place: z' bit for bit the restatement's, the guard behind dst untouched, every D_i within the bound of numpy's
    distances to the kernel's own z', sources and beta read only"""
    n, k = z.size, len(xs)
    xd, bd = [G(a) for a in xs], G(beta)
    ref, _ = W.step32(z, xs, beta)
    for inplace in (False, True):
        zd = sent(n + GUARD)
        zd[:n] = G(z)
        buf = zd if inplace else sent(n + GUARD)
        wsp = new_ws(k, n, float("nan"))
        assert step(buf[:n], zd[:n], xd, bd, wsp) == 0, _C.last_error()
        torch.cuda.synchronize()
        got = N(buf)
        assert np.all(got[n:] == f32(SENT)), "%s k=%d n=%d: wrote behind dst" % (what, k, n)
        bad = R.same_bits_or_nan(got[:n], ref)
        assert bad.size == 0, "%s k=%d n=%d inplace=%d: %d of %d elements differ, first at %d: %r vs %r" % (
            what, k, n, inplace, bad.size, n, bad[0], got[bad[0]], ref[bad[0]])
        if not inplace:
            assert np.array_equal(R.bits(N(zd)[:n]), R.bits(z))               # z is read, not written
        check_D(finished_D(k, n, wsp), xs, got[:n], n, "%s k=%d n=%d inplace=%d" % (what, k, n, inplace))
    for a, t in zip(xs, xd):
        assert np.array_equal(R.bits(N(t)), R.bits(a))
    assert np.array_equal(N(bd), beta)


# ---- the step pass -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.SIZES[:-1])
@pytest.mark.parametrize("k", [1, 2, 3, 8, 16, 17, 32])
def test_step_bit_identical_to_the_restatement(k, n):
    """tail only, below / at / above one vector, around one block; K <= 16 on float4, K >= 17 on float2; weights with exact zeros among them"""
    check_step(R.inputs(n, k), W.base(n), some_beta(k), "sine")


@pytest.mark.parametrize("k", [3, 17])
def test_step_grid_stride_wrap(k):
    """n = 2048 * 256 * 4 + 5: every thread of the capped grid wraps (twice on the float2 path) and the scalar tail follows"""
    check_step(R.inputs(R.BIG, k), W.base(R.BIG), some_beta(k), "sine")


@pytest.mark.parametrize("n", [1, 5, 4103])
@pytest.mark.parametrize("k", [1, 3, 8, 17, 32])
def test_distance_only_pass_writes_nothing_but_the_workspace(k, n):
    xs, z = R.inputs(n, k), W.base(n)
    xd = [G(a) for a in xs]
    zd = sent(n + GUARD)
    zd[:n] = G(z)
    wsp = new_ws(k, n, float("nan"))
    assert step(None, zd[:n], xd, None, wsp) == 0, _C.last_error()            # beta may be null in this mode
    D = finished_D(k, n, wsp)
    check_D(D, xs, z, n, "distance-only k=%d n=%d" % (k, n))
    junk = sent(k)                                                            # and is not read when given
    junk.fill_(float("nan"))
    assert step(None, zd[:n], xd, junk, wsp) == 0, _C.last_error()
    assert np.array_equal(finished_D(k, n, wsp).view(np.uint64), D.view(np.uint64))      # the same bits on a second run
    got = N(zd)
    assert np.array_equal(R.bits(got[:n]), R.bits(z)) and np.all(got[n:] == f32(SENT))
    for a, t in zip(xs, xd):
        assert np.array_equal(R.bits(N(t)), R.bits(a))


@pytest.mark.parametrize("k", [5, 8, 17])
def test_a_client_with_weight_zero_does_not_change_the_centre_by_a_bit(k):
    """clients 0, 1, 2 hold NaN (both signs, several payloads), +-inf and +-1e30 and have beta = 0: z' is bit for bit what the remaining
    clients alone give; their own D_i is not finite (NaN, inf) or huge (1e30) and nobody else's is"""
    n = 4103
    xs, z = R.spiked(n, k), W.base(n)
    beta = ((np.arange(k) % 3 + 1.0) / (2.0 * k)).astype(f32)
    beta[:3] = 0.0
    check_step(xs, z, beta, "spiked")
    ref, D = W.step32(z, xs, beta)
    alone, _ = W.step32(z, xs[3:], beta[3:])
    assert np.array_equal(R.bits(ref), R.bits(alone)) and np.all(np.isfinite(ref))
    assert not np.isfinite(D[0]) and not np.isfinite(D[1]) and D[2] > 1e60 and np.all(np.isfinite(D[2:])) and np.all(D[3:] < 1e3)


@pytest.mark.parametrize("k", [3, 17])
def test_all_weights_zero_keep_the_centre_signed_zeros_included(k):
    n = 1023
    z = W.base(n).copy()
    z[::3] = R.signed_zeros(n, 1)[0][::3]                                     # -0 and +0 among the values
    assert np.signbit(z[z == 0]).any() and not np.signbit(z[z == 0]).all()
    xs = R.inputs(n, k)
    ref, _ = W.step32(z, xs, np.zeros(k, dtype=f32))
    assert np.array_equal(R.bits(ref), R.bits(z))
    check_step(xs, z, np.zeros(k, dtype=f32), "all zero")
    check_step(xs, z, np.array([-0.0] * k, dtype=f32), "all minus zero")      # -0 == 0: skipped as well


# ---- the weights kernel ------------------------------------------------------------------------------------------------------------------
D_CASES = (
    [4.0, 0.25, 9.0, 1.0, 2.25],
    [4.0, np.inf, 0.0, np.nan, 1.0],
    [0.0, 0.0, 0.0],
    [5e-324, 1e-310, 3.0, 1e-30],                                             # subnormal squared distances
    [np.nan, 7.0, np.inf],                                                    # one finite client only
    [np.nan, np.inf, np.nan, np.inf],                                         # nothing finite
    [1e300, 1e-300, 1.0],
    [float(i * i + 1) * 0.37 for i in range(32)],
    [2.0],
)


def run_weights(rule, D, alpha, param, slot=0, iters=2, info0=None):
    """the weights kernel on squared distances given from the host: n = 1 is a grid of one block, so the workspace [k][1] IS D"""
    k = len(D)
    wsp = G(np.asarray(D, dtype=f64))
    hd, hb = sent((iters + 1) * k + 1, torch.float64), sent(iters * k + 1)
    info = sent(5, torch.float64) if info0 is None else G(np.asarray(list(info0) + [SENT], dtype=f64))
    assert weights(rule, alpha, param, slot, iters, k, 1, wsp, hd, hb, info) == 0, _C.last_error()
    torch.cuda.synchronize()
    return N(hd), N(hb), N(info)


@pytest.mark.parametrize("case", range(len(D_CASES)))
def test_weights_bit_identical_to_the_restatement(case):
    D = np.asarray(D_CASES[case], dtype=f64)
    k = D.size
    alphas = [[1.0 / k] * k, [(i % 4 + 1.0) / (2.5 * k) for i in range(k)]]
    for alpha in alphas:
        for rule, param in ((W.GEOMEDIAN, 1e-6), (W.GEOMEDIAN, 0.5), (W.CCLIP, 0.0), (W.CCLIP, 0.75), (W.CCLIP, 1e-3)):
            beta, S, tau, nf = W.weights64(rule, D, alpha, param)
            hd, hb, info = run_weights(rule, D, alpha, param)
            what = (case, rule, param)
            assert np.array_equal(R.bits(hb[:k]), R.bits(beta)), (what, hb[:k], beta)
            assert np.all(hb[k:] == f32(SENT)) and np.all(hd[k:] == SENT) and info[4] == SENT      # slot 0 only, nothing behind
            fin = np.isfinite(D)                                              # the history holds D itself (a NaN stays a NaN, an inf an inf)
            assert np.array_equal(hd[:k][fin], D[fin]) and np.array_equal(np.isnan(hd[:k]), np.isnan(D)) and np.array_equal(np.isinf(hd[:k]), np.isinf(D))
            assert np.array([info[1]]).view(np.uint64)[0] == np.array([S]).view(np.uint64)[0], (what, info[1], S)
            assert info[2] == (1.0 if nf == 0 else 0.0) and info[3] == nf, (what, info)
            if rule == W.CCLIP:
                assert np.array([info[0]]).view(np.uint64)[0] == np.array([tau], dtype=f64).view(np.uint64)[0], (what, info[0], tau)
            else:
                assert info[0] == SENT


def test_weights_slots_keep_the_rounds_tau_and_the_flag():
    D0, D1 = [4.0, 0.25, 9.0, 1.0, 2.25], [16.0, 1.0, 0.04, np.nan, 100.0]
    k, alpha = 5, [0.2] * 5
    _, _, info = run_weights(W.CCLIP, D0, alpha, 0.0)
    assert info[0] == 1.5 and info[2] == 0.0                                  # the lower median of (2, 0.5, 3, 1, 1.5)
    beta, S, tau, nf = W.weights64(W.CCLIP, D1, alpha, 0.0, tau=1.5)
    hd, hb, info1 = run_weights(W.CCLIP, D1, alpha, 0.0, slot=1, info0=info[:4])
    assert info1[0] == 1.5 and info1[2] == 0.0 and info1[3] == 4
    assert np.array_equal(R.bits(hb[k:2 * k]), R.bits(beta)) and np.all(hb[:k] == f32(SENT)) and np.all(hd[:k] == SENT)
    hd, hb, info2 = run_weights(W.CCLIP, D1, alpha, 0.0, slot=2, info0=info1[:4])          # slot == iters: distances, no weights
    assert np.all(hb == f32(SENT)) and np.array_equal(hd[2 * k:3 * k][[0, 1, 2, 4]], np.asarray(D1)[[0, 1, 2, 4]])
    _, _, info3 = run_weights(W.GEOMEDIAN, [np.nan] * 3, [1 / 3] * 3, 1e-6, slot=1, info0=[0.0, 1.0, 0.0, 3.0])
    assert info3[2] == 1.0 and info3[3] == 0                                  # a later slot without a finite client sets the flag
    _, _, info4 = run_weights(W.GEOMEDIAN, [1.0] * 3, [1 / 3] * 3, 1e-6, slot=1, info0=[0.0, 1.0, 1.0, 0.0])
    assert info4[2] == 1.0                                                    # and it stays set for the round
    _, _, info5 = run_weights(W.GEOMEDIAN, [1.0] * 3, [1 / 3] * 3, 1e-6, slot=0, info0=[0.0, 1.0, 1.0, 0.0])
    assert info5[2] == 0.0                                                    # slot 0 starts a round


# ---- whole rounds through the C ABI ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule,param", [(W.GEOMEDIAN, 1e-6), (W.CCLIP, 0.0)])
@pytest.mark.parametrize("n,k,f", [(4103, 5, 1), (1023, 8, 2), (4103, 17, 3)])
def test_round_replayed_from_the_kernels_own_steps(n, k, f, rule, param):
    """R = 3 on ``krum_inputs``; z is snapshotted after every step.  Each step is replayed from the kernel's own previous (z, D): beta bit
    for bit, z bit for bit, D within the bound.  The final z is within (R + 1)(k + 3) 2^-24 max|x| of the fp64 iteration (the restatement
    stays within a quarter of that: tests/test_reweight_cpu.py), and the +-1e30 client has not moved it."""
    iters = 3
    xs, z0, alpha = R.krum_inputs(n, k, f), W.base(n), [1.0 / k] * k
    xd, zd = [G(a) for a in xs], G(z0)
    wsp = new_ws(k, n, float("nan"))
    hd, hb, info = sent((iters + 1) * k, torch.float64), sent(iters * k), sent(4, torch.float64)
    snaps = []
    for slot in range(iters + 1):
        rc = step(None, zd, xd, None, wsp) if slot == 0 else step(zd, zd, xd, hb[(slot - 1) * k:slot * k], wsp)
        assert rc == 0, _C.last_error()
        assert weights(rule, alpha, param, slot, iters, k, n, wsp, hd, hb, info) == 0, _C.last_error()
        snaps.append(zd.clone())
    torch.cuda.synchronize()
    Dh, Bh, inf_ = N(hd).reshape(iters + 1, k), N(hb).reshape(iters, k), N(info)
    zs = [N(s) for s in snaps]
    assert np.array_equal(R.bits(zs[0]), R.bits(z0)) and inf_[2] == 0.0 and inf_[3] == k
    tau = None
    for s in range(iters + 1):
        check_D(Dh[s], xs, zs[s], n, "slot %d" % s)
        if s == iters:
            break
        beta, _, tau, _ = W.weights64(rule, Dh[s], alpha, param, tau)
        assert np.array_equal(R.bits(Bh[s]), R.bits(beta)), (s, Bh[s], beta)
        ref, _ = W.step32(zs[s], xs, Bh[s])
        assert np.array_equal(R.bits(zs[s + 1]), R.bits(ref)), "step %d" % (s + 1)
    if rule == W.CCLIP:
        assert inf_[0] == tau == float(np.sort(np.sqrt(Dh[0]))[(k - 1) // 2])
    z64 = W.round64(z0, xs, alpha, rule, iters, param)
    bound = (iters + 1) * (k + 3) * W.U * W.honest_scale(z0, xs, k - f)
    err = float(np.abs(zs[-1].astype(f64) - z64).max())
    print("n=%d k=%d rule=%d: error / bound %.3f" % (n, k, rule, err / bound))
    assert err <= bound
    honest = np.mean([x.astype(f64) for x in xs[:k - f]], axis=0)
    assert np.linalg.norm(zs[-1].astype(f64) - honest) <= 0.02 * np.sqrt(n)


# ---- argument errors -----------------------------------------------------------------------------------------------------------------------
def test_reweight_argument_errors_launch_nothing():
    """every bad argument is one the host-side checks refuse before a launch: negative return code, a message, outputs untouched"""
    n, k = 1023, 5
    xs = R.inputs(n, k)
    xd = [G(a) for a in xs]
    zd = G(W.base(n))
    out = sent(n + GUARD)
    dst = out[:n]
    beta = sent(k + 3)
    wsp = new_ws(k, n)

    def refused(rc, word):
        assert rc < 0
        assert word in _C.last_error(), _C.last_error()

    refused(step(dst, None, xd, beta, wsp, n=n), "reweight_step")
    refused(step(dst, zd, xd, beta, None), "reweight_step")
    refused(step(dst, zd, xd, beta, wsp, n=0), "reweight_step")
    refused(step(dst, zd, [], beta, wsp), "k=0")
    refused(step(dst, zd, xd * 6 + xd[:3], beta, wsp), "k=33")
    refused(step(dst, zd, xd, None, wsp), "beta")                             # a step that writes needs its weights
    refused(step(dst, zd, [xd[0], None, xd[2]], beta, wsp), "client state 1 is null")
    refused(step(dst, zd, xd * 2 + [None] + xd, beta, new_ws(16, n)), "client state 10 is null")
    refused(step(out[1:n + 1], zd, xd, beta, wsp), "aligned")
    refused(step(dst, zd[1:], xd, beta, wsp, n=n - 1), "aligned")
    refused(step(dst, zd, [xd[0], xd[1][1:], xd[2]], beta, wsp, n=n - 1), "aligned")
    lib = _C.lib()
    pp = ptrs_of(xd)
    refused(lib.fedfr_reweight_step(dst.data_ptr(), zd.data_ptr(), pp, beta.data_ptr() + 2, k, n, wsp.data_ptr(), wsp.numel() * 8, _C.stream()), "4-byte")
    refused(lib.fedfr_reweight_step(dst.data_ptr(), zd.data_ptr(), pp, beta.data_ptr(), k, n, wsp.data_ptr() + 4, wsp.numel() * 8 - 8, _C.stream()), "8-byte")
    refused(lib.fedfr_reweight_step(dst.data_ptr(), zd.data_ptr(), None, beta.data_ptr(), k, n, wsp.data_ptr(), wsp.numel() * 8, _C.stream()), "reweight_step")
    refused(step(xd[2], zd, xd, beta, wsp), "overlaps client state 2")        # dst is a source
    refused(step(xd[2][4:], zd, xd, beta, wsp, n=n - 4), "overlaps")          # dst inside a source
    refused(step(zd[4:], zd, xd, beta, wsp, n=n - 4), "overlaps z")           # in place means dst == z
    refused(step(dst, zd, xd, beta, wsp[:-1]), "workspace")
    assert step(dst, zd, xd, beta, wsp[:-1]) == -3                            # FEDFR_ERR_WORKSPACE
    assert step(None, zd, xd, None, wsp[:-1]) == -3
    hd, hb, info = sent(3 * k, torch.float64), sent(2 * k), sent(4, torch.float64)
    al = [1.0 / k] * k
    refused(weights(W.GEOMEDIAN, None, 1e-6, 0, 2, k, n, wsp, hd, hb, info), "reweight_weights")
    refused(weights(W.GEOMEDIAN, al, 1e-6, 0, 2, k, n, None, hd, hb, info), "reweight_weights")
    refused(weights(W.GEOMEDIAN, al, 1e-6, 0, 2, k, n, wsp, None, hb, info), "reweight_weights")
    refused(weights(W.GEOMEDIAN, al, 1e-6, 0, 2, k, n, wsp, hd, None, info), "reweight_weights")
    refused(weights(W.GEOMEDIAN, al, 1e-6, 0, 2, k, n, wsp, hd, hb, None), "reweight_weights")
    refused(weights(W.GEOMEDIAN, al, 1e-6, 0, 2, k, 0, wsp, hd, hb, info), "reweight_weights")
    refused(weights(W.GEOMEDIAN, al, 1e-6, 0, 2, 0, n, wsp, hd, hb, info), "k=0")
    refused(weights(W.GEOMEDIAN, al * 7, 1e-6, 0, 2, 33, n, wsp, hd, hb, info), "k=33")
    refused(weights(2, al, 1e-6, 0, 2, k, n, wsp, hd, hb, info), "rule 2")
    refused(weights(-1, al, 1e-6, 0, 2, k, n, wsp, hd, hb, info), "rule -1")
    refused(weights(W.GEOMEDIAN, al, 1e-6, 3, 2, k, n, wsp, hd, hb, info), "slot=3")
    refused(weights(W.GEOMEDIAN, al, 1e-6, -1, 2, k, n, wsp, hd, hb, info), "slot=-1")
    refused(weights(W.GEOMEDIAN, al, 1e-6, 0, 0, k, n, wsp, hd, hb, info), "iters=0")
    refused(weights(W.GEOMEDIAN, al, 0.0, 0, 2, k, n, wsp, hd, hb, info), "nu")
    refused(weights(W.GEOMEDIAN, al, float("nan"), 0, 2, k, n, wsp, hd, hb, info), "nu")
    refused(weights(W.CCLIP, al, -1.0, 0, 2, k, n, wsp, hd, hb, info), "tau")
    refused(weights(W.CCLIP, al, float("inf"), 0, 2, k, n, wsp, hd, hb, info), "tau")
    refused(weights(W.CCLIP, [0.2, -0.1, 0.2, 0.2, 0.2], 0.0, 0, 2, k, n, wsp, hd, hb, info), "alpha 1")
    refused(weights(W.CCLIP, [0.2, 0.2, 0.2, float("nan"), 0.2], 0.0, 0, 2, k, n, wsp, hd, hb, info), "alpha 3")
    refused(weights(W.CCLIP, al, 0.0, 0, 2, k, n, wsp[:-1], hd, hb, info), "workspace")
    assert weights(W.CCLIP, al, 0.0, 0, 2, k, n, wsp[:-1], hd, hb, info) == -3
    cal = (C.c_double * k)(*al)
    for d_off, b_off, i_off in ((4, 0, 0), (0, 2, 0), (0, 0, 4)):
        refused(lib.fedfr_reweight_weights(0, cal, 1e-6, 0, 2, k, n, wsp.data_ptr(), wsp.numel() * 8, hd.data_ptr() + d_off, hb.data_ptr() + b_off,
                                           info.data_ptr() + i_off, _C.stream()), "aligned")
    torch.cuda.synchronize()
    for t in (out, beta, wsp, hd, hb, info):
        assert float(t.min()) == SENT == float(t.max())
    assert np.array_equal(R.bits(N(zd)), R.bits(W.base(n)))
    for a, t in zip(xs, xd):
        assert np.array_equal(N(t), a)


# ---- server.FedReweighted ----------------------------------------------------------------------------------------------------------------
def synthetic_states(k, tag=0.0):
    """k FlatStateDicts over made-up flat tensors: 4103 parameters, 1026 running statistics (means, then variances >= 0), 7 counters (as
    in tests/test_robust_gpu.py); and the global state they were trained from (the sine base as parameters)"""
    ps = R.inputs(4103, k, tag=tag)
    j = np.arange(513, dtype=f64)

    def state(p, i):
        mean = 0.3 * np.sin(0.21 * j + i)
        var = 0.5 + 0.4 * np.sin(0.13 * j + 0.7 * i) ** 2
        b = np.concatenate([mean, var]).astype(f32)
        c = torch.arange(7, dtype=torch.int64) * 3 + 11 * i + 1
        return client.FlatStateDict.from_flat((G(p), G(b), c.to(DEV)), [], [])
    return state(W.base(4103, tag=tag), -1), [state(ps[i], i) for i in range(k)]


def flat_np(sd):
    return [N(t) for t in sd.flat]


def expected_stats(agg, glob, models):
    """``_average_stats`` at the read-back weights: the clients with a non-zero final weight and, for CenteredClip, the global state"""
    ws = agg.stats_weights()
    srcs = list(models) + ([glob] if agg.kind == "CenteredClip" else [])
    assert len(ws) == len(srcs) and all(w >= 0 for w in ws) and abs(sum(ws) - 1.0) <= len(ws) * 2.0 ** -23
    kept = [(m, w) for m, w in zip(srcs, ws) if w != 0]
    return server._average_stats([m for m, _ in kept], [w for _, w in kept])[0]


@pytest.mark.parametrize("kind,kw", [("GeoMedian", {}), ("CenteredClip", {}), ("CenteredClip", {"tau": 0.5, "iters": 2}), ("GeoMedian", {"iters": 1})])
@pytest.mark.parametrize("k", [5, 17])
def test_fedreweighted_survives_poisoned_clients_where_fedpavg_does_not(kind, kw, k):
    """client 2 returns NaN everywhere, client 4 +-1e30 parameters: FedPavg of the states is not finite; the reweighted rule returns finite,
    honest-sized parameters, which are the restatement's steps at the read-back weights bit for bit; the read-back weights are the
    restatement's at the read-back distances; the statistics equal ``_average_stats`` at the final weights with running_var >= 0; the
    counters take FedPavg's path"""
    glob, models = synthetic_states(k)
    models[2].flat[0].fill_(float("nan"))
    models[2].flat[1].fill_(float("nan"))
    p4 = models[4].flat[0]
    p4.copy_(1e30 * torch.where(torch.arange(p4.numel(), device=DEV) % 2 == 0, 1.0, -1.0))
    models[4].flat[1].fill_(1e30)
    sizes = [100.0 + 37.0 * ((5 * i) % 7) for i in range(k)]
    agg = server.ReweightedAggregator(kind, **kw)
    out = server.FedReweighted(glob, models, sizes, agg)
    avg = server.FedPavg(models, sizes)
    torch.cuda.synchronize()
    assert isinstance(out, client.FlatStateDict) and not bool(torch.isfinite(avg.flat[0]).all())
    iters = agg.iters
    assert agg.last_dist.shape == (iters + 1, k) and agg.last_weights.shape == (iters, k) and agg.last_weights.dtype == f32
    assert (agg.last_tau is None) == (kind == "GeoMedian")
    xs, z0 = [flat_np(m)[0] for m in models], flat_np(glob)[0]
    z, tau = z0, None
    rule, param = W.RULES[kind], (agg.nu if kind == "GeoMedian" else (agg.tau or 0.0))
    for s in range(iters):
        beta, _, tau, nf = W.weights64(rule, agg.last_dist[s] ** 2, [1.0 / k] * k, param, tau)
        assert nf == k - 1 and agg.last_weights[s][2] == 0 and not np.isfinite(agg.last_dist[s][2])
        # (last_dist is sqrt(D): squaring it back loses a bit of D, so the weights are compared to 2 ulp, not bit for bit -- that is the chain test's)
        assert np.all(np.abs(agg.last_weights[s].astype(f64) - beta.astype(f64)) <= 2.0 ** -22 * np.abs(beta.astype(f64)))
        z, _ = W.step32(z, xs, agg.last_weights[s])
    if kind == "CenteredClip":
        assert agg.last_tau == tau
    got = N(out.flat[0])
    assert np.array_equal(R.bits(got), R.bits(z)) and np.all(np.isfinite(got)) and float(np.abs(got).max()) < 2.0
    assert agg.last_dist[-1][4] > 1e30 and 0 < agg.last_weights[-1][4] < 1e-30       # the 1e30 client is weighted by 1 / its distance
    assert torch.equal(out.flat[1], expected_stats(agg, glob, models))
    assert bool(torch.isfinite(out.flat[1]).all()) and float(out.flat[1][513:].min()) >= 0.0
    assert torch.equal(out.flat[2], avg.flat[2]) and out.flat[2].dtype == torch.float32
    for m, x in zip(models, xs):                                              # the states are read, never written
        assert np.array_equal(R.bits(N(m.flat[0])), R.bits(x))
    assert np.array_equal(R.bits(N(glob.flat[0])), R.bits(z0))


def test_fedreweighted_keeps_its_buffers_and_repeats_itself():
    glob, models = synthetic_states(8)
    agg = server.ReweightedAggregator("GeoMedian")
    a = server.FedReweighted(glob, models, [1.0] * 8, agg)
    ws_ptr, hist_ptr, d1 = agg._ws.buf.data_ptr(), agg._hist.data_ptr(), agg.last_dist.copy()
    b = server.FedReweighted(glob, models, [1.0] * 8, agg)
    assert agg._ws.buf.data_ptr() == ws_ptr and agg._hist.data_ptr() == hist_ptr
    assert torch.equal(a.flat[0], b.flat[0]) and torch.equal(a.flat[1], b.flat[1]) and np.array_equal(d1, agg.last_dist)
    assert abs(float(agg.last_weights[-1].astype(f64).sum()) - 1.0) <= 8 * 2.0 ** -24


@pytest.mark.parametrize("kind", ["GeoMedian", "CenteredClip"])
def test_fedreweighted_without_a_finite_client_raises(kind):
    glob, models = synthetic_states(3)
    for m, v in zip(models, (float("nan"), float("inf"), float("nan"))):
        m.flat[0].fill_(v)
    with pytest.raises(RuntimeError, match="no client sent a finite state"):
        server.FedReweighted(glob, models, [1.0] * 3, server.ReweightedAggregator(kind))


# ---- Server.train ------------------------------------------------------------------------------------------------------------------------
def _tiny_world(aggr, nc, **extra):
    """``nc`` clients on the smallest backbone and batch of tests/test_robust_gpu.py's Server.train tests (iresnet18, B = 4, two steps each)"""
    class Args:
        network, loss, local_epoch, output_dir, BCE_local, aggr_alg = "iresnet18", "CosFace", 1, "/tmp", False, aggr

    for k_, v_ in extra.items():
        setattr(Args, k_, v_)

    class DS:
        ID_base = 0

    class Loader(list):
        dataset = DS()

    class Data:
        train_class_sizes = [10] * nc
        train_dataset_sizes = [300, 100, 250, 120, 200][:nc]
        train_loaders = [Loader([(O.closed_form_images(4, tag=float(c * 2 + s)), O.closed_form_labels(4, 10, tag=c + s))
                                 for s in range(2)]) for c in range(nc)]

    from fedfr_amd.config import config as cfg
    cfg.lr = 0.01
    torch.manual_seed(20)
    clients = [client.Client(c, Args, Data, device=DEV) for c in range(nc)]
    srv = server.Server(clients, Data, Args, device=DEV)
    srv.federated_model.load_state_dict(O.closed_form_state_dict(O.IRESNET_LAYERS["iresnet18"], tag=2.0))
    return srv


@pytest.mark.parametrize("aggr,extra", [("GeoMedian", {}), ("CenteredClip", {"cclip_iters": 2})])
def test_server_train_equals_fedreweighted_called_directly(monkeypatch, aggr, extra):
    """one round, 3 clients: the loaded global parameters and running statistics are FedReweighted of the recorded global and client
    states, bit for bit"""
    srv = _tiny_world(aggr, 3, **extra)
    rec = []
    real = server.FedReweighted

    def copy_of(sd):
        return client.FlatStateDict.from_flat(tuple(t.clone() for t in sd.flat), sd.table, sd.layers)

    def recording(global_state, models, weights, agg):
        rec.append((copy_of(global_state), [copy_of(m) for m in models], list(weights)))
        return real(global_state, models, weights, agg)
    monkeypatch.setattr(server, "FedReweighted", recording)
    assert np.isfinite(srv.train())
    torch.cuda.synchronize()
    agg = srv.reweight_agg
    assert len(rec) == 1 and len(rec[0][1]) == 3 and agg.kind == aggr and srv.robust_agg is None and srv.server_opt is None
    assert agg.iters == (3 if aggr == "GeoMedian" else 2) and agg.last_dist.shape == (agg.iters + 1, 3)
    assert np.all(agg.last_dist[0] > 0) and np.all(np.isfinite(agg.last_dist))   # the clients' update norms: they trained
    glob, models, weights = rec[0]
    direct = real(glob, models, weights, server.ReweightedAggregator(aggr, iters=agg.iters))
    torch.cuda.synchronize()
    got = srv.federated_model.flat_state()
    for r in (0, 1):
        assert torch.equal(got[r], direct.flat[r]), "region %d" % r
    assert not torch.equal(got[0], glob.flat[0])
