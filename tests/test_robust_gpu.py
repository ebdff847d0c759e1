"""Robust aggregation on the GPU: fedfr_robust_trimmed_mean / _pairdist / _krum_select through the C ABI against the restatements of
tests/robust_cases.py (the trimmed mean bit for bit, the distances within the derived fp64 summation bound, the selection exactly),
argument errors, and the Python surface (server.FedRobust, Server.train with aggr_alg="CoordMedian" / "MultiKrum")."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import robust_cases as R  # noqa: E402
from oracle import ref_cpu as O  # noqa: E402

from fedfr_amd import _C, client, server  # noqa: E402

DEV = torch.device("cuda:0")
f32, f64 = np.float32, np.float64
SENT = -777.25
GUARD = 4                                      # sentinel elements behind dst (the buffer stays 16-byte aligned in front of them)


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


def tmean(dst, srcs, trim, n=None, k=None):
    """fedfr_robust_trimmed_mean on device tensors; returns the return code"""
    n = srcs[0].numel() if n is None else n
    return _C.lib().fedfr_robust_trimmed_mean(ptr(dst), ptrs_of(srcs), len(srcs) if k is None else k, trim, n, _C.stream())


def pairdist(xs, dist, wsp, n=None, k=None, ws_bytes=None):
    n = xs[0].numel() if n is None else n
    return _C.lib().fedfr_robust_pairdist(ptrs_of(xs), len(xs) if k is None else k, n, ptr(dist), ptr(wsp),
                                          (0 if wsp is None else wsp.numel() * 8) if ws_bytes is None else ws_bytes, _C.stream())


def krum(dist, k, f, m, score, sel):
    return _C.lib().fedfr_robust_krum_select(ptr(dist), k, f, m, ptr(score), ptr(sel), _C.stream())


def check_trimmed(xs, bs, what):
    """the kernel at every b of ``bs`` against the restatement: bit for bit (NaN where it is NaN), the guard behind dst untouched"""
    n, k = xs[0].size, len(xs)
    xd = [G(a) for a in xs]
    for b in bs:
        ref = R.trimmed32(xs, b)
        buf = sent(n + GUARD)
        assert tmean(buf[:n], xd, b) == 0, _C.last_error()
        torch.cuda.synchronize()
        got = N(buf)
        assert np.all(got[n:] == f32(SENT)), "%s k=%d n=%d b=%d: wrote behind dst" % (what, k, n, b)
        bad = R.same_bits_or_nan(got[:n], ref)
        assert bad.size == 0, "%s k=%d n=%d b=%d: %d of %d elements differ, first at %d: %r vs %r" % (
            what, k, n, b, bad.size, n, bad[0], got[bad[0]], ref[bad[0]])
    for a, t in zip(xs, xd):                               # the sources are read, never written
        assert np.array_equal(R.bits(N(t)), R.bits(a))


# ---- trimmed mean ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.SIZES[:-1])
@pytest.mark.parametrize("k", R.KS_TRIM)
def test_trimmed_mean_bit_identical_to_the_restatement(k, n):
    """tail only, below / at / above one float4, below and above one block; b = 0, 1 and the median's; K <= 16 on float4, K >= 17 on float2"""
    check_trimmed(R.inputs(n, k), R.trims(k), "sine")


@pytest.mark.parametrize("k", R.KS_TRIM_BIG)
def test_trimmed_mean_grid_stride_wrap(k):
    """n = 2048 * 256 * 4 + 5: every thread of the capped grid wraps (twice on the float2 path) and the scalar tail follows"""
    check_trimmed(R.inputs(R.BIG, k), R.trims(k), "sine")


def test_trimmed_mean_every_client_count():
    """every instantiation K = 1 .. 32 (each its own sorting network) at the median's trim and at b = 0 (the whole sorted sum)"""
    for k in range(1, R.MAX_K + 1):
        check_trimmed(R.inputs(1023, k), sorted({0, (k - 1) // 2}), "sine")


@pytest.mark.parametrize("k", [5, 8, 9, 17])
def test_trimmed_mean_spiked_inputs(k):
    """a NaN client (both signs, several payloads), a +-inf client, a +-1e30 client, exactly equal clients, +-0 in mixed signs: the order is
    the documented total order on bit patterns, so even the sign of a zero result is the restatement's.  b = 0 keeps the NaN (NaN result),
    b = 1 trims it (and meets the infinities), b = 2 trims NaN and inf on top and leaves 1e30 where it is not trimmed below."""
    xs = R.spiked(4103, k)
    bs = sorted({0, 1, 2, (k - 1) // 2})
    check_trimmed(xs, bs, "spiked")
    assert np.all(np.isnan(R.trimmed32(xs, 0)))
    if k >= 8:                                             # 3 spikes <= b: the median sees the honest clients only
        assert np.all(np.isfinite(R.trimmed32(xs, (k - 1) // 2))) and np.all(np.abs(R.trimmed32(xs, (k - 1) // 2)) < 1.0)
    check_trimmed(R.signed_zeros(4103, k), bs, "signed zeros")


# ---- pairwise distances ------------------------------------------------------------------------------------------------------------------
def run_pairdist(xs, fill=0.0):
    k, n = len(xs), xs[0].numel()
    nws = _C.lib().fedfr_robust_pairdist_workspace_bytes(k, n)
    assert nws == 8 * (k * (k - 1) // 2) * R.grid(n)
    wsp = torch.full((nws // 8,), fill, dtype=torch.float64, device=DEV)
    dist = sent(k * k + 1, torch.float64)
    assert pairdist(xs, dist, wsp) == 0, _C.last_error()
    torch.cuda.synchronize()
    out = N(dist)
    assert out[k * k] == SENT                              # nothing behind the matrix
    return out[:k * k].reshape(k, k)


@pytest.mark.parametrize("n", R.SIZES)
@pytest.mark.parametrize("k", R.KS_DIST)
def test_pairdist(k, n):
    """|D - pairdist64| <= n 2^-52 D (the terms are exact and non-negative: any order of n of them is within (n - 1) 2^-53; twice that for
    two orders); symmetric, zero diagonal; a second run on a workspace full of NaN gives the same bits.  k <= 13 is one launch (float4 loads to
    k = 8, float2 above), 16 / 32 are tiled (diagonal groups of 8 and the 8 x 8 cross tiles between them)."""
    xs = R.inputs(n, k)
    ref = R.pairdist64(xs)
    xd = [G(a) for a in xs]
    D = run_pairdist(xd)
    err = np.abs(D - ref)
    off = ~np.eye(k, dtype=bool)
    print("k=%d n=%d: worst error / bound %.3f" % (k, n, float(np.max(err[off] / np.maximum(R.pairdist_bound(n, ref)[off], 1e-300)))))
    assert np.all(err <= R.pairdist_bound(n, ref))
    assert np.array_equal(D, D.T) and np.all(np.diag(D) == 0.0) and np.all(D[off] > 0.0)
    D2 = run_pairdist(xd, fill=float("nan"))
    assert np.array_equal(D2.view(np.uint64), D.view(np.uint64))


@pytest.mark.parametrize("k", [10, 11, 12, 13, 14, 15, 17, 23, 25])
def test_pairdist_around_the_one_launch_threshold_and_partial_groups(k):
    """k = 13 is the last client count served by one launch, 14 the first tiled one (8 + 6); 15, 17, 23, 25: cross tiles 8 x 7, 8 x 1 and
    a last group of one state (no diagonal launch); n below and above one block with a tail"""
    for n in (5, 4103):
        xs = R.inputs(n, k)
        ref = R.pairdist64(xs)
        D = run_pairdist([G(a) for a in xs])
        assert np.all(np.abs(D - ref) <= R.pairdist_bound(n, ref))
        assert np.array_equal(D, D.T) and np.all(np.diag(D) == 0.0)


@pytest.mark.parametrize("k,bad", [(3, 1), (9, 4), (13, 12), (16, 11)])
def test_pairdist_nan_client_poisons_its_row_and_column_only(k, bad):
    n = 4103
    xs = [a.copy() for a in R.inputs(n, k)]
    xs[bad][:] = np.nan
    ref = R.pairdist64([a for i, a in enumerate(xs) if i != bad])
    D = run_pairdist([G(a) for a in xs])
    keep = [i for i in range(k) if i != bad]
    assert not np.any(np.isfinite(D[bad, keep])) and not np.any(np.isfinite(D[keep, bad])) and D[bad, bad] == 0.0
    sub = D[np.ix_(keep, keep)]
    assert np.all(np.isfinite(sub)) and np.all(np.abs(sub - ref) <= R.pairdist_bound(n, ref))


# ---- Krum / Multi-Krum selection ---------------------------------------------------------------------------------------------------------
def run_krum(D, f, m):
    k = D.shape[0]
    dd = G(np.ascontiguousarray(D, dtype=f64).reshape(-1))
    score, sel = sent(k + 1, torch.float64), torch.full((k + 1,), -7, dtype=torch.int32, device=DEV)
    assert krum(dd, k, f, m, score, sel) == 0, _C.last_error()
    torch.cuda.synchronize()
    assert N(score)[k] == SENT and N(sel)[k] == -7
    return N(score)[:k], N(sel)[:k]


@pytest.mark.parametrize("n,k,f,m", R.KRUM_CASES)
def test_krum_select_on_the_kernels_own_distances(n, k, f, m):
    """selected == krum_ref of the kernel's distances exactly, scores within 1e-15 k (relative; the same ascending fp64 sums); and, because
    tests/test_robust_cpu.py shows the m-th and (m+1)-th score 10^6 distance bounds apart, == krum_ref of the numpy distances as well:
    the planted outliers (the last f clients) are rejected"""
    xs = R.krum_inputs(n, k, f)
    D = run_pairdist([G(a) for a in xs])
    score, sel = run_krum(D, f, m)
    rscore, rsel = R.krum_ref(D, f, m)
    assert np.array_equal(sel, rsel), (sel, rsel)
    assert np.all(np.abs(score - rscore) <= 1e-15 * k * rscore), (score, rscore)
    assert np.array_equal(sel, R.krum_ref(R.pairdist64(xs), f, m)[1])
    assert sel.sum() == m and not sel[k - f:].any()


def test_krum_select_ties_and_non_finite_rows():
    D = np.array([[0, 1, 1, 9, 9], [1, 0, 1, 9, 9], [1, 1, 0, 9, 9], [9, 9, 9, 0, 1], [9, 9, 9, 1, 0]], dtype=f64)
    score, sel = run_krum(D, 1, 1)                          # clients 0, 1, 2 tie at 2.0: the lowest index wins
    assert score.tolist() == [2.0, 2.0, 2.0, 10.0, 10.0] and sel.tolist() == [1, 0, 0, 0, 0]
    assert run_krum(D, 1, 2)[1].tolist() == [1, 1, 0, 0, 0]
    assert run_krum(D[::-1, ::-1].copy(), 1, 1)[1].tolist() == [0, 0, 1, 0, 0]      # the clients reversed: scores 10, 10, 2, 2, 2
    E = D.copy()
    E[0, :] = E[:, 0] = np.nan                              # a client that sent NaN: never selected while m finite ones exist
    E[0, 0] = 0.0
    score, sel = run_krum(E, 1, 4)
    rscore, rsel = R.krum_ref(E, 1, 4)
    assert np.isinf(score[0]) and np.all(np.isfinite(score[1:])) and sel.tolist() == rsel.tolist() == [0, 1, 1, 1, 1]
    E[1, 2] = E[2, 1] = -np.inf                             # -inf is not finite either: +inf, not a bargain
    score, sel = run_krum(E, 1, 2)
    assert np.array_equal(sel, R.krum_ref(E, 1, 2)[1]) and sel[0] == 0 and np.all(score >= 0)
    k = 32                                                  # the largest k, every row in use
    rng = np.random.RandomState(3)
    A = rng.rand(k, k)
    Dk = A + A.T
    np.fill_diagonal(Dk, 0.0)
    score, sel = run_krum(Dk, 7, 25)
    rscore, rsel = R.krum_ref(Dk, 7, 25)
    assert np.array_equal(sel, rsel) and np.all(np.abs(score - rscore) <= 1e-15 * k * rscore)


# ---- argument errors -----------------------------------------------------------------------------------------------------------------------
def test_robust_argument_errors_launch_nothing():
    """every bad argument is one the host-side checks refuse before a launch: negative return code, a message, outputs untouched"""
    n, k = 1023, 5
    xs = R.inputs(n, k)
    xd = [G(a) for a in xs]
    out = sent(n + GUARD)
    dst = out[:n]

    def refused(rc, word):
        assert rc < 0
        assert word in _C.last_error(), _C.last_error()

    refused(tmean(None, xd, 1), "robust_trimmed_mean")
    refused(tmean(dst, xd, 1, n=0), "robust_trimmed_mean")
    refused(tmean(dst, [], 0, n=n), "k=0")
    refused(tmean(dst, xd * 7, 1), "k=35")
    refused(tmean(dst, xd * 6 + xd[:3], 1), "k=33")
    refused(tmean(dst, xd, -1), "trim=-1")
    refused(tmean(dst, xd, 3), "trim=3")                                      # 2 b >= k
    refused(tmean(dst, xd[:4], 2), "trim=2")
    refused(tmean(dst, xd[:1], 1), "trim=1")
    refused(tmean(dst, [xd[0], None, xd[2]], 1), "null")
    refused(tmean(dst, xd * 2 + [None] + xd, 1), "source 10 is null")             # a null entry in the middle of a k > 8 array
    refused(tmean(dst, [xd[0], xd[1][1:], xd[2]], 1, n=n - 1), "aligned")
    refused(tmean(out[1:n + 1], xd, 1), "aligned")
    refused(tmean(xd[2], xd, 1), "overlaps")                                  # dst is a source
    refused(tmean(xd[2][4:], xd, 1, n=n - 4), "overlaps")                     # dst inside a source
    refused(_C.lib().fedfr_robust_trimmed_mean(dst.data_ptr(), None, k, 1, n, _C.stream()), "robust_trimmed_mean")
    npairs = k * (k - 1) // 2
    wsp = torch.full((npairs * R.grid(n),), SENT, dtype=torch.float64, device=DEV)
    dist = sent(k * k, torch.float64)
    refused(pairdist(xd, None, wsp), "robust_pairdist")
    refused(pairdist(xd, dist, None), "robust_pairdist")
    refused(pairdist(xd, dist, wsp, n=0), "robust_pairdist")
    refused(pairdist(xd[:1], dist, wsp), "k=1")
    refused(pairdist(xd * 7, dist, wsp), "k=35")
    refused(pairdist([xd[0], None], dist, wsp), "null")
    big_ws = torch.full((120 * R.grid(n),), SENT, dtype=torch.float64, device=DEV)
    big_dist = sent(16 * 16, torch.float64)
    refused(pairdist(xd * 2 + [None] + xd, big_dist, big_ws), "client state 10 is null")
    lib = _C.lib()
    pp = ptrs_of(xd)
    refused(lib.fedfr_robust_pairdist(pp, k, n, dist.data_ptr() + 4, wsp.data_ptr(), wsp.numel() * 8, _C.stream()), "8-byte")
    refused(lib.fedfr_robust_pairdist(pp, k, n, dist.data_ptr(), wsp.data_ptr() + 4, wsp.numel() * 8 - 8, _C.stream()), "8-byte")
    refused(pairdist([a[1:] for a in xd], dist, wsp, n=n - 1), "aligned")
    refused(pairdist(xd, dist, wsp[:-1]), "workspace")
    assert pairdist(xd, dist, wsp[:-1]) == -3                                 # FEDFR_ERR_WORKSPACE
    refused(_C.lib().fedfr_robust_pairdist(None, k, n, dist.data_ptr(), wsp.data_ptr(), wsp.numel() * 8, _C.stream()), "robust_pairdist")
    score, sel = sent(k, torch.float64), torch.full((k,), -7, dtype=torch.int32, device=DEV)
    dm = G(R.pairdist64(xs).reshape(-1))
    refused(krum(None, k, 1, 1, score, sel), "robust_krum_select")
    refused(krum(dm, k, 1, 1, None, sel), "robust_krum_select")
    refused(krum(dm, k, 1, 1, score, None), "robust_krum_select")
    refused(krum(dm, k, 2, 1, score, sel), "f=2")                             # k < 2 f + 3
    refused(krum(dm, k, -1, 1, score, sel), "f=-1")
    refused(krum(dm, 2, 0, 1, score, sel), "k=2")
    refused(krum(dm, 33, 1, 1, score, sel), "k=33")
    refused(krum(dm, k, 1, 0, score, sel), "m=0")
    refused(krum(dm, k, 1, 5, score, sel), "m=5")                             # m > k - f
    for d_off, s_off, l_off in ((4, 0, 0), (0, 4, 0), (0, 0, 2)):              # dist / score 8-byte, selected 4-byte aligned
        refused(lib.fedfr_robust_krum_select(dm.data_ptr() + d_off, k, 1, 1, score.data_ptr() + s_off, sel.data_ptr() + l_off, _C.stream()),
                "aligned")
    torch.cuda.synchronize()
    assert float(out.min()) == SENT == float(out.max()) and float(dist.min()) == SENT == float(dist.max())
    assert float(big_ws.min()) == SENT == float(big_ws.max()) and float(big_dist.min()) == SENT == float(big_dist.max())
    assert float(wsp.min()) == SENT == float(wsp.max()) and float(score.min()) == SENT == float(score.max()) and int(sel.max()) == -7 == int(sel.min())
    for a, t in zip(xs, xd):
        assert np.array_equal(N(t), a)


# ---- server.FedRobust ---------------------------------------------------------------------------------------------------------------------
def synthetic_states(k, tag=0.0):
    """k FlatStateDicts over made-up flat tensors: 4103 parameters, 1026 running statistics (means, then variances >= 0), 7 counters"""
    ps = R.inputs(4103, k, tag=tag)
    j = np.arange(513, dtype=f64)
    out = []
    for i in range(k):
        mean = 0.3 * np.sin(0.21 * j + i)
        var = 0.5 + 0.4 * np.sin(0.13 * j + 0.7 * i) ** 2
        b = np.concatenate([mean, var]).astype(f32)
        c = torch.arange(7, dtype=torch.int64) * 3 + 11 * i + 1
        out.append(client.FlatStateDict.from_flat((G(ps[i]), G(b), c.to(DEV)), [], []))
    return out


def flat_np(sd):
    return [N(t) for t in sd.flat]


@pytest.mark.parametrize("kind,k,kw,b_expected", [("CoordMedian", 3, {}, 1), ("CoordMedian", 8, {}, 3), ("TrimmedMean", 10, {}, 1),
                                                  ("TrimmedMean", 5, {"trim": 2}, 2), ("TrimmedMean", 17, {"trim_ratio": 0.25}, 4)])
def test_fedrobust_coordinate_wise(kind, k, kw, b_expected):
    """parameters and running statistics bit-equal to the restatement (unweighted), counters equal to FedPavg's (data-size weights)"""
    models = synthetic_states(k)
    sizes = [100.0 + 37.0 * ((5 * i) % 7) for i in range(k)]
    agg = server.RobustAggregator(kind, **kw)
    out = server.FedRobust(models, sizes, agg)
    avg = server.FedPavg(models, sizes)
    torch.cuda.synchronize()
    b = agg.trim_count(k)
    assert b == b_expected
    assert isinstance(out, client.FlatStateDict)
    for r in (0, 1):
        ref = R.trimmed32([flat_np(m)[r] for m in models], b)
        assert np.array_equal(R.bits(N(out.flat[r])), R.bits(ref)), (kind, k, r)
    assert float(out.flat[1][513:].min()) >= 0.0                              # running_var stays >= 0
    assert torch.equal(out.flat[2], avg.flat[2]) and out.flat[2].dtype == torch.float32
    assert agg.last_selected is None


@pytest.mark.parametrize("poison", ["nan", "1e30"])
@pytest.mark.parametrize("kind", ["CoordMedian", "TrimmedMean"])
def test_fedrobust_survives_a_poisoned_client_where_fedpavg_does_not(kind, poison):
    """one of 5 clients returns NaN (or +-1e30) everywhere: FedPavg of the states is not finite (or ~1e29), the robust rule returns the
    restatement's finite, honest-sized result bit for bit.  (Cannot pass without the feature: nothing else in the server survives it.)"""
    k = 5
    models = synthetic_states(k)
    p, b, c = models[2].flat
    if poison == "nan":
        p.fill_(float("nan"))
        b.fill_(float("nan"))
    else:
        sign = torch.where(torch.arange(p.numel(), device=DEV) % 2 == 0, 1.0, -1.0)
        p.copy_(1e30 * sign)
        b.copy_(1e30 * sign[:b.numel()])
    sizes = [100.0] * k
    agg = server.RobustAggregator(kind, trim=1)
    out = server.FedRobust(models, sizes, agg)
    avg = server.FedPavg(models, sizes)
    torch.cuda.synchronize()
    bb = agg.trim_count(k)
    for r in (0, 1):
        got = N(out.flat[r])
        ref = R.trimmed32([flat_np(m)[r] for m in models], bb)
        assert np.array_equal(R.bits(got), R.bits(ref))
        assert np.all(np.isfinite(got)) and float(np.abs(got).max()) < 2.0
        worst = N(avg.flat[r])
        assert (not np.all(np.isfinite(worst))) if poison == "nan" else float(np.abs(worst).max()) > 1e28
    assert float(out.flat[1][513:].min()) >= 0.0


@pytest.mark.parametrize("kind,k,f,m", [("Krum", 5, 1, None), ("MultiKrum", 5, 1, None), ("MultiKrum", 9, 2, 4), ("MultiKrum", 17, 3, None)])
def test_fedrobust_krum(kind, k, f, m):
    """the selection is krum_ref's on the kernel's distances (which are within the bound of numpy's); the result is FedPavg of the selected
    states with unit weights, bit for bit, counters included; a poisoned client (NaN, the last one) is never selected"""
    models = synthetic_states(k)
    models[k - 1].flat[0].fill_(float("nan"))
    if f >= 2:
        models[0].flat[0].mul_(-40.0)                                         # and a finite outlier, where f covers both
    sizes = [100.0 + i for i in range(k)]
    agg = server.RobustAggregator(kind, num_byzantine=f, multi_m=m)
    out = server.FedRobust(models, sizes, agg)
    torch.cuda.synchronize()
    mm = agg.select_count(k)
    assert mm == (1 if kind == "Krum" else (m or k - f))
    xs = [flat_np(s)[0] for s in models]
    ref = R.pairdist64(xs[:-1])
    D = agg.last_dist
    assert D.shape == (k, k) and np.all(np.abs(D[:-1, :-1] - ref) <= R.pairdist_bound(4103, ref)) and not np.any(np.isfinite(D[-1, :-1]))
    rscore, rsel = R.krum_ref(D, f, mm)
    assert agg.last_selected == [int(i) for i in np.flatnonzero(rsel)] and len(agg.last_selected) == mm
    assert k - 1 not in agg.last_selected and (f < 2 or 0 not in agg.last_selected)
    assert np.all(np.abs(agg.last_scores[:-1] - rscore[:-1]) <= 1e-15 * k * rscore[:-1]) and np.isinf(agg.last_scores[-1])
    expect = server.FedPavg([models[i] for i in agg.last_selected], [1.0] * mm)
    torch.cuda.synchronize()
    for a, e in zip(out.flat, expect.flat):
        assert torch.equal(a, e)
    assert bool(torch.isfinite(out.flat[0]).all())


def test_fedrobust_krum_without_enough_finite_clients_raises():
    k = 5
    models = synthetic_states(k)
    for i in (1, 3):
        models[i].flat[0].fill_(float("nan"))                                 # 3 finite clients, each with 2 finite neighbours: k - f - 2 = 2 -> scores finite
    agg = server.RobustAggregator("MultiKrum", num_byzantine=1)              # m = 4 > 3 clients with a finite score
    with pytest.raises(RuntimeError, match="not finite"):
        server.FedRobust(models, [1.0] * k, agg)
    assert server.FedRobust(models, [1.0] * k, server.RobustAggregator("MultiKrum", num_byzantine=1, multi_m=3)) is not None


# ---- Server.train ------------------------------------------------------------------------------------------------------------------------
def _tiny_world(aggr, nc, **extra):
    """``nc`` clients on the smallest backbone and batch of tests/test_fedopt_gpu.py's Server.train tests (iresnet18, B = 4, two steps each)"""
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


def _record_fedrobust(monkeypatch):
    rec = []
    real = server.FedRobust

    def recording(models, weights, agg):
        rec.append(([flat_np(m) for m in models], list(weights)))
        return real(models, weights, agg)
    monkeypatch.setattr(server, "FedRobust", recording)
    return rec


def test_server_train_coord_median(monkeypatch):
    """one round, 3 clients, aggr_alg="CoordMedian": the loaded global parameters and running statistics are the restatement (the middle
    value of the three recorded client states, coordinate by coordinate), bit for bit"""
    srv = _tiny_world("CoordMedian", 3)
    rec = _record_fedrobust(monkeypatch)
    assert np.isfinite(srv.train())
    torch.cuda.synchronize()
    assert len(rec) == 1 and len(rec[0][0]) == 3 and srv.robust_agg.kind == "CoordMedian" and srv.server_opt is None
    states, weights = rec[0]
    assert len(weights) == 3 and not np.array_equal(states[0][0], states[1][0])
    got = srv.federated_model.flat_state()
    for r in (0, 1):
        ref = R.trimmed32([s[r] for s in states], 1)
        assert np.array_equal(R.bits(N(got[r])), R.bits(ref)), "region %d" % r


def test_server_train_multi_krum(monkeypatch):
    """one round, 5 clients, aggr_alg="MultiKrum", f = 1: the kernel's distances are within the bound of numpy's, the selection is
    krum_ref's on them, and the loaded global parameters are the unit-weight mean of the 4 selected recorded states in FedPavg's fp32
    order (acc = 0; acc = acc + 0.25 x_i, ascending i), bit for bit"""
    srv = _tiny_world("MultiKrum", 5, num_byzantine=1)
    rec = _record_fedrobust(monkeypatch)
    assert np.isfinite(srv.train())
    torch.cuda.synchronize()
    agg = srv.robust_agg
    states, _ = rec[0]
    xs = [s[0] for s in states]
    ref = R.pairdist64(xs)
    assert np.all(np.abs(agg.last_dist - ref) <= R.pairdist_bound(xs[0].size, ref))
    _, rsel = R.krum_ref(agg.last_dist, 1, 4)
    assert agg.last_selected == [int(i) for i in np.flatnonzero(rsel)] and len(agg.last_selected) == 4
    got = srv.federated_model.flat_state()
    w = f32(1.0 / 4)
    for r in (0, 1):
        acc = np.zeros_like(states[0][r])
        for i in agg.last_selected:
            t = w * states[i][r]
            acc = acc + t
        assert np.array_equal(R.bits(N(got[r])), R.bits(acc)), "region %d" % r
