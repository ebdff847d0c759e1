"""Top-k sparsified client uploads on the GPU: fedfr_topk_sparsify / fedfr_sparse_aggregate through the C ABI against the restatement of
tests/sparse_cases.py, bit for bit (indices, values as uint32 images, residual, counter), with sentinel guards behind every output and the
workspace; and the Python surface (compress.TopKCompressor, server.FedSparse, Server.train with topk_ratio).  No test here feeds unsorted
or out-of-range indices to the aggregate: its in-tile guard is checked by reading the code (csrc/sparse.hip), not by running what a wrong
kernel would turn into an out-of-bounds write."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import sparse_cases as S  # noqa: E402
from oracle import ref_cpu as O  # noqa: E402

from fedfr_amd import _C, client, compress, server  # noqa: E402

DEV = torch.device("cuda:0")
f32, f64 = np.float32, np.float64
SENT = -777.25
SENT_I = 0x7A5A5A5A
GUARD = 16                                     # sentinel elements behind every output


def G(a):
    return torch.from_numpy(np.array(a)).to(DEV)          # (a copy: the shared inputs are read-only arrays)


def N(t):
    return t.detach().cpu().numpy()


def ptr(t):
    return None if t is None else t.data_ptr()


def ptrs_of(ts):
    return (C.c_void_p * max(len(ts), 1))(*[ptr(t) for t in ts])


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


class Sparsifier:
    """x, x_i and (with ``e``) the residual on the device, each output and the workspace with sentinels behind it"""

    def __init__(self, x, xi, e):
        self.x, self.xi, self.n = x, xi, x.size
        self.xd, self.xid = G(x), G(xi)
        self.ed = None
        if e is not None:
            self.ed = torch.full((self.n + GUARD,), SENT, dtype=torch.float32, device=DEV)
            self.ed[:self.n] = G(e)
        self.wsb = int(_C.lib().fedfr_topk_workspace_bytes(self.n, 1 if e is not None else 0))
        assert self.wsb % 16 == 0
        self.ws = torch.full((self.wsb // 4 + GUARD,), SENT_I, dtype=torch.int32, device=DEV)

    def run(self, keep):
        """one fedfr_topk_sparsify call; (idx, val, counter) as numpy after checking the guards"""
        n = self.n
        idx = torch.full((keep + GUARD,), SENT_I, dtype=torch.int32, device=DEV)
        val = torch.full((keep + GUARD,), SENT, dtype=torch.float32, device=DEV)
        cnt = torch.tensor([0, -7], dtype=torch.int32, device=DEV)
        rc = _C.lib().fedfr_topk_sparsify(ptr(self.xd), ptr(self.xid), ptr(self.ed), n, keep, ptr(idx), ptr(val), ptr(cnt), ptr(self.ws), _C.stream())
        assert rc == 0, _C.last_error()
        torch.cuda.synchronize()
        i, v, k, w = N(idx), N(val), N(cnt), N(self.ws)
        tag = "n=%d keep=%d" % (n, keep)
        assert np.all(i[keep:] == SENT_I) and np.all(v[keep:] == f32(SENT)) and k[1] == -7, tag + ": wrote behind idx, val or the counter"
        assert np.all(w[self.wsb // 4:] == SENT_I), tag + ": wrote behind the workspace"
        if self.ed is not None:
            assert np.all(N(self.ed)[n:] == f32(SENT)), tag + ": wrote behind the residual"
        return i[:keep].view(np.uint32), v[:keep], int(k[0])

    def inputs_untouched(self):
        assert np.array_equal(bits(N(self.xd)), bits(self.x)) and np.array_equal(bits(N(self.xid)), bits(self.xi))      # read, never written


def check_sparsify(x, xi, e, keeps, what):
    """one call per entry of ``keeps`` on ONE residual buffer (with ``e``: the rounds of one client) against the restatement carried the same way"""
    sp = Sparsifier(x, xi, e)
    er = e
    for rnd, keep in enumerate(keeps):
        ridx, rval, ren, rbad, _ = S.sparsify(x, xi, er, keep)
        idx, val, bad = sp.run(keep)
        tag = "%s n=%d keep=%d feedback=%s round %d" % (what, x.size, keep, e is not None, rnd)
        d = np.flatnonzero(idx != ridx)
        assert d.size == 0, "%s: %d indices differ, first at %d: %d vs %d" % (tag, d.size, d[0], idx[d[0]], ridx[d[0]])
        d = np.flatnonzero(bits(val) != bits(rval))
        assert d.size == 0, "%s: %d values differ, first at %d: %#x vs %#x" % (tag, d.size, d[0], bits(val)[d[0]], bits(rval)[d[0]])
        assert bad == rbad, "%s: counter %d vs %d" % (tag, bad, rbad)
        if e is not None:
            er = ren
            got = N(sp.ed)[:x.size]
            d = np.flatnonzero(bits(got) != bits(er))
            assert d.size == 0, "%s: %d residuals differ, first at %d: %r vs %r" % (tag, d.size, d[0], got[d[0]], er[d[0]])
    sp.inputs_untouched()


# ---- fedfr_topk_sparsify -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", S.SIZES)
def test_sparsify_bit_identical_to_the_restatement(n):
    """below / at / above one wave and one tile, several tiles and a partial one; keep in {1, 2, ceil(n / 100), n / 2, n - 1, n}; without
    feedback (v in the workspace), and with it: every keep in turn on ONE residual buffer, so each call after the first runs on the
    residual the one before it left (the in-place update)"""
    x, xs = S.inputs(n, 2)
    keeps = S.keeps_for(n)
    check_sparsify(x, xs[0], None, keeps, "sine")
    check_sparsify(x, xs[1], S.residual(n), keeps[::-1], "sine")
    check_sparsify(x, xs[1], np.zeros(n, dtype=f32), [keeps[len(keeps) // 2]] * 2, "sine from a zero residual")


@pytest.mark.parametrize("case", range(len(S.patterns())), ids=[p[0] for p in S.patterns()])
def test_sparsify_constructed_key_patterns(case):
    """keys that differ in one digit only, all ties, +-0, subnormals, one exponent, tie cuts inside a wave / at a wave boundary / at a tile
    boundary / taking every tie, NaNs of both signs and infinities (fewer and more than keep).  What each is for: tests/test_sparse_cpu.py"""
    name, v, keep = S.patterns()[case]
    x = np.zeros(v.size, dtype=f32)
    check_sparsify(x, v, None, [keep], name)
    check_sparsify(x, v, np.zeros(v.size, dtype=f32), [keep, keep], name)


@pytest.mark.parametrize("feedback", [False, True])
def test_sparsify_grid_stride_wrap(feedback):
    """n = 2048 * 256 * 8 + 37 with keep = ceil(n / 100): the capped grid, workgroup 0 wraps onto the partial tile 2048 (non-adjacent tiles in
    one workgroup); NaNs in the first and the last tile: the counter is 3, from different workgroups' passes"""
    x, xi, e, keep = S.big_case()
    assert -(-S.BIG // S.TILE) == S.GRID_CAP + 1 and S.BIG % S.TILE == 37
    ridx, rval, ren, rbad, _ = S.big_reference(feedback)
    sp = Sparsifier(x, xi, e if feedback else None)
    idx, val, bad = sp.run(keep)
    assert rbad == 3 and bad == 3
    assert np.array_equal(idx, ridx) and np.array_equal(bits(val), bits(rval))
    if feedback:
        assert np.array_equal(bits(N(sp.ed)[:S.BIG]), bits(ren))
    sp.inputs_untouched()


# ---- fedfr_sparse_aggregate --------------------------------------------------------------------------------------------------------------
WS = [f32(w) for w in (0.21, 0.07, 0.13, 0.09, 0.17, 0.11, 0.08, 0.14)]


def run_aggregate(buf, base_ptr, dev_ups, ws, n, accumulate):
    k = len(dev_ups)
    keeps = (C.c_size_t * k)(*[u[0].numel() for u in dev_ups])
    wv = (C.c_float * k)(*[float(w) for w in ws])
    rc = _C.lib().fedfr_sparse_aggregate(ptr(buf), base_ptr, ptrs_of([u[0] for u in dev_ups]), ptrs_of([u[1] for u in dev_ups]), keeps, wv, k, n,
                                         accumulate, _C.stream())
    assert rc == 0, _C.last_error()
    torch.cuda.synchronize()


def check_aggregate(n, ups, ks, what, accumulates=(0, 1), bases=("null", "distinct", "dst")):
    """every k of ``ks`` x accumulate 0 / 1 x base null / distinct / equal to dst against the restatement, bit for bit (NaN where it is NaN)"""
    dev = [(G(i.view(np.int32)), G(v)) for i, v in ups[:max(ks)]]
    j = np.arange(n, dtype=f64)
    dst0 = (0.4 * np.sin(0.77 * j + 1.3)).astype(f32)
    x = (0.5 * np.sin(0.37 * j + 0.1)).astype(f32)
    xd, d0 = G(x), G(dst0)
    for k in ks:
        for accumulate in accumulates:
            for base in bases:
                buf = torch.full((n + GUARD,), SENT, dtype=torch.float32, device=DEV)
                buf[:n] = d0
                run_aggregate(buf, {"null": None, "distinct": ptr(xd), "dst": ptr(buf)}[base], dev[:k], WS[:k], n, accumulate)
                got = N(buf)
                tag = "%s n=%d k=%d accumulate=%d base=%s" % (what, n, k, accumulate, base)
                assert np.all(got[n:] == f32(SENT)), tag + ": wrote behind dst"
                ref = S.aggregate(dst0, {"null": None, "distinct": x, "dst": dst0}[base], ups[:k], WS[:k], n, bool(accumulate))
                bad = S.same_bits_or_nan(got[:n], ref)
                assert bad.size == 0, "%s: %d of %d elements differ, first at %d: %r vs %r" % (tag, bad.size, n, bad[0], got[bad[0]], ref[bad[0]])
    assert np.array_equal(bits(N(xd)), bits(x))                              # read, never written: base and the uploads
    for (di, dv), (i, v) in zip(dev, ups):
        assert np.array_equal(N(di).view(np.uint32), i) and np.array_equal(bits(N(dv)), bits(v))


@pytest.mark.parametrize("shape", S.UPLOAD_SHAPES)
@pytest.mark.parametrize("n", S.AGG_SIZES)
def test_aggregate_bit_identical_to_the_restatement(n, shape):
    """k = 1, 2, 3, 8; accumulate 0 and 1; base null, distinct and equal to dst (in place); below / at / above one tile and several tiles with
    a partial one; uploads that overlap in a fixed pattern with keep = n among them and a different keep per client, entries in one tile
    only, at both ends only, further apart than a tile, and keep = 1"""
    check_aggregate(n, S.uploads(n, shape), (1, 2, 3, 8), shape)


def test_aggregate_many_tiles_per_workgroup():
    """n = 2048 * 4096 * 2 + 4099: the capped grid with two or three tiles per workgroup, so the workgroups walk their uploads from tile to
    tile, and the last workgroup goes from whole tiles to the partial one (its threads reuse the LDS tile without a barrier between a
    tile's output and the next one's initialisation: csrc/sparse.hip says why that is safe); a dense upload (every third element: five to
    six steps per tile) beside a sparse one; once with accumulate and base in use, once with neither (nothing to wait for before the next
    tile's initialisation)"""
    n = S.GRID_CAP * S.AGG_TILE * 2 + S.AGG_TILE + 3
    ups = S.uploads(n, "multiples", 3)[2:] + S.uploads(n, "gaps", 1)
    check_aggregate(n, ups, (2,), "multiples of 3 + gaps", accumulates=(1,), bases=("distinct",))
    check_aggregate(n, ups, (2,), "multiples of 3 + gaps", accumulates=(0,), bases=("null",))


@pytest.mark.parametrize("k", [9, 17])
def test_aggregate_chained(k):
    """more than 8 uploads: calls of 8 chained with accumulate, base on the last call only, as server.FedSparse does it"""
    n = 3 * S.AGG_TILE + 5
    ups = (S.uploads(n, "multiples") + S.uploads(n, "gaps") + S.uploads(n, "one tile"))[:k]
    ws = [f32(1.0 / (3 + i)) for i in range(k)]
    x = (0.5 * np.sin(0.37 * np.arange(n, dtype=f64) + 0.1)).astype(f32)
    xd = G(x)
    dev = [(G(i.view(np.int32)), G(v)) for i, v in ups]
    buf = torch.full((n + GUARD,), SENT, dtype=torch.float32, device=DEV)
    for c0 in range(0, k, 8):
        run_aggregate(buf, ptr(xd) if c0 + 8 >= k else None, dev[c0:c0 + 8], ws[c0:c0 + 8], n, 1 if c0 else 0)
    got = N(buf)
    assert np.all(got[n:] == f32(SENT))
    assert np.array_equal(bits(got[:n]), bits(S.chained(x, ups, ws, n)))


def test_aggregate_nan_and_signed_zeros_follow_the_law():
    """a NaN value reaches exactly its own element; val = -0 adds as +0 + w (-0) = +0; base = -0 under an untouched element gives
    -0 + +0 = +0 and under accumulate with dst = -0 gives -0 + -0 = -0"""
    n = S.AGG_TILE + 77
    idx = np.array([3, 500, S.AGG_TILE - 1, S.AGG_TILE, n - 1], dtype=np.uint32)
    val = np.array([0.5, np.nan, -0.0, -0.0, 0.25], dtype=f32)
    idx2 = np.array([3, S.AGG_TILE], dtype=np.uint32)
    val2 = np.array([-0.0, 1.5], dtype=f32)
    ups = [(idx, val), (idx2, val2)]
    base = np.full(n, -0.0, dtype=f32)
    base[10:20] = 1.0
    dst0 = np.full(n, -0.0, dtype=f32)
    dev = [(G(i.view(np.int32)), G(v)) for i, v in ups]
    bd = G(base)
    for accumulate in (0, 1):
        buf = torch.full((n + GUARD,), SENT, dtype=torch.float32, device=DEV)
        buf[:n] = G(dst0)
        run_aggregate(buf, ptr(bd), dev, WS[:2], n, accumulate)
        got = N(buf)[:n]
        ref = S.aggregate(dst0, base, ups, WS[:2], n, bool(accumulate))
        assert S.same_bits_or_nan(got, ref).size == 0
        assert np.flatnonzero(np.isnan(got)).tolist() == [500]
        assert bits(got)[S.AGG_TILE - 1] == (0x80000000 if accumulate else 0) and bits(got)[7] == (0x80000000 if accumulate else 0)
        assert got[3] == f32(WS[0] * f32(0.5)) and got[12] == 1.0


def test_argument_errors_launch_nothing():
    n = 1023
    x, xs = S.inputs(n, 1)
    xd, xid = G(x), G(xs[0])
    idx = torch.full((n + GUARD,), SENT_I, dtype=torch.int32, device=DEV)
    val = torch.full((n + GUARD,), SENT, dtype=torch.float32, device=DEV)
    out = torch.full((n + GUARD,), SENT, dtype=torch.float32, device=DEV)
    ws = torch.full((int(_C.lib().fedfr_topk_workspace_bytes(n, 0)) // 4,), SENT_I, dtype=torch.int32, device=DEV)
    lib = _C.lib()

    def refused(rc, word):
        assert rc == -1 and word in _C.last_error(), (rc, _C.last_error())

    st = _C.stream()
    refused(lib.fedfr_topk_sparsify(ptr(xd), ptr(xid), None, n, 0, ptr(idx), ptr(val), None, ptr(ws), st), "keep=0")
    refused(lib.fedfr_topk_sparsify(ptr(xd), ptr(xid), None, n, n + 1, ptr(idx), ptr(val), None, ptr(ws), st), "keep=%d" % (n + 1))
    refused(lib.fedfr_topk_sparsify(ptr(xd), ptr(xid), None, 2 ** 31, 5, ptr(idx), ptr(val), None, ptr(ws), st), "2^31")
    refused(lib.fedfr_topk_sparsify(ptr(xd), None, None, n, 5, ptr(idx), ptr(val), None, ptr(ws), st), "null")
    refused(lib.fedfr_topk_sparsify(ptr(xd), ptr(xid), None, n, 5, ptr(idx), ptr(val), None, None, st), "null")
    refused(lib.fedfr_topk_sparsify(ptr(xd), ptr(xid), ptr(out) + 4, n, 5, ptr(idx), ptr(val), None, ptr(ws), st), "aligned")
    refused(lib.fedfr_topk_sparsify(ptr(xd), ptr(xid), None, n, 5, ptr(idx) + 8, ptr(val), None, ptr(ws), st), "aligned")
    assert lib.fedfr_topk_sparsify(ptr(xd), ptr(xid), ptr(out), 0, 0, ptr(idx), ptr(val), None, ptr(ws), st) == 0      # n = 0, keep = 0: a no-op
    keeps = (C.c_size_t * 9)(*([5] * 9))
    wv = (C.c_float * 9)(*([0.125] * 9))
    refused(lib.fedfr_sparse_aggregate(ptr(out), None, ptrs_of([idx] * 9), ptrs_of([val] * 9), keeps, wv, 9, n, 0, st), "k=9")
    refused(lib.fedfr_sparse_aggregate(ptr(out), None, ptrs_of([idx, None]), ptrs_of([val, val]), keeps, wv, 2, n, 0, st), "index buffer 1 is null")
    refused(lib.fedfr_sparse_aggregate(ptr(out), None, ptrs_of([idx, idx]), ptrs_of([val, None]), keeps, wv, 2, n, 0, st), "value buffer 1 is null")
    refused(lib.fedfr_sparse_aggregate(ptr(out) + 8, None, ptrs_of([idx]), ptrs_of([val]), keeps, wv, 1, n, 0, st), "aligned")
    refused(lib.fedfr_sparse_aggregate(ptr(out), None, ptrs_of([idx]), ptrs_of([val]), (C.c_size_t * 1)(n + 1), wv, 1, n, 0, st), "keep=%d" % (n + 1))
    assert lib.fedfr_sparse_aggregate(ptr(out), ptr(xd), ptrs_of([idx]), ptrs_of([val]), (C.c_size_t * 1)(0), wv, 1, 0, 0, st) == 0      # n = 0: a no-op
    torch.cuda.synchronize()
    assert float(out.min()) == SENT == float(out.max()) and float(val.min()) == SENT == float(val.max())
    assert int(idx.min()) == SENT_I == int(idx.max()) and int(ws.min()) == SENT_I == int(ws.max())


# ---- the Python surface ------------------------------------------------------------------------------------------------------------------
NP = 4103


def synthetic_states(k, tag=0.0, stats=True):
    """(global state, k client states) as FlatStateDicts over made-up flat tensors: 4103 parameters, 1026 running statistics (means, then
    variances >= 0) and 7 counters per state (none of either with ``stats`` off: a backbone without BatchNorm)"""
    x, ps = S.inputs(NP, k, tag=tag)
    j = np.arange(513, dtype=f64)

    def state(p, i):
        if not stats:
            return client.FlatStateDict.from_flat((G(p), torch.zeros(0, device=DEV), torch.zeros(0, dtype=torch.int64, device=DEV)), [], [])
        mean = 0.3 * np.sin(0.21 * j + i)
        var = 0.5 + 0.4 * np.sin(0.13 * j + 0.7 * i) ** 2
        c = torch.arange(7, dtype=torch.int64) * 3 + 11 * i + 1
        return client.FlatStateDict.from_flat((G(p), G(np.concatenate([mean, var]).astype(f32)), c.to(DEV)), [], [])
    return state(x, -1), [state(p, i) for i, p in enumerate(ps)]


def sizes_of(k):
    return [100.0 + 37.0 * ((5 * i) % 7) for i in range(k)]


def weights32(sizes):
    tot = sum(sizes)
    return [f32(s / tot) for s in sizes]


def test_topk_compressor_carries_its_residual_over_three_rounds():
    g, _ = synthetic_states(1)
    x = N(g.flat[0])
    ratio = 0.05
    keep = S.keep_count(NP, ratio)
    assert compress.keep_count(NP, ratio) == keep == 206
    comp = compress.TopKCompressor(ratio)
    plain = compress.TopKCompressor(ratio, error_feedback=False)
    e = np.zeros(NP, dtype=f32)
    for r in range(3):
        _, (m,) = synthetic_states(1, tag=0.5 * r)                            # the client's state of round r
        up = comp.compress(g, m)
        idx, val, e, bad, _ = S.sparsify(x, N(m.flat[0]), e, keep)
        assert np.array_equal(N(up.idx).view(np.uint32), idx) and np.array_equal(bits(N(up.val)), bits(val)) and up.nonfinite_count() == bad == 0, r
        assert np.array_equal(bits(N(comp.residual)), bits(e)) and np.any(e != 0), r
        up0 = plain.compress(g, m)                                            # no feedback: nothing carried
        idx0, val0, _, _, _ = S.sparsify(x, N(m.flat[0]), None, keep)
        assert np.array_equal(N(up0.idx).view(np.uint32), idx0) and np.array_equal(bits(N(up0.val)), bits(val0)) and plain.residual is None
        assert up.stats is m.flat[1] and up.counters is m.flat[2] and up.keep == keep and up.n == NP
    comp.reset()
    assert comp.residual is None
    up = comp.compress(g, m)
    idx, val, e, _, _ = S.sparsify(x, N(m.flat[0]), np.zeros(NP, dtype=f32), keep)
    assert np.array_equal(N(up.idx).view(np.uint32), idx) and np.array_equal(bits(N(comp.residual)), bits(e))
    assert up.nbytes == 8 * keep + 1026 * 4 + 7 * 8 and up.dense_nbytes == NP * 4 + 1026 * 4 + 7 * 8 and up.ratio == up.nbytes / up.dense_nbytes
    g0, (m0,) = synthetic_states(1, stats=False)                              # no statistics: 8 bytes per kept parameter against 4 per parameter
    up = compress.TopKCompressor(ratio).compress(g0, m0)
    assert up.ratio == 8 * keep / (4 * NP)
    with pytest.raises(RuntimeError, match="reset"):
        comp.compress(client.FlatStateDict.from_flat((g.flat[0][:64].clone(), g.flat[1], g.flat[2]), [], []),
                      client.FlatStateDict.from_flat((m.flat[0][:64].clone(), m.flat[1], m.flat[2]), [], []))


def restated_uploads(x, xs, keep):
    return [S.sparsify(x, xi, np.zeros(x.size, dtype=f32), keep)[:2] for xi in xs]


@pytest.mark.parametrize("opt", [False, True])
@pytest.mark.parametrize("k", [3, 9])
def test_fedsparse(k, opt):
    """parameters bit-equal to the restatement chained as the code chains it (groups of 8, x added by the last pass); with a
    ServerOptimizer("AVGM") the result is apply_delta on the restated delta (the chained sum WITHOUT x), momentum included; statistics and
    counters bit-equal to FedPavg's"""
    g, models = synthetic_states(k)
    sizes = sizes_of(k)
    ups = [compress.TopKCompressor(0.1).compress(g, m) for m in models]
    sopt = server.ServerOptimizer("AVGM", lr=0.5, beta1=0.75) if opt else None
    out = server.FedSparse(g, ups, sizes, sopt)
    avg = server.FedPavg(models, sizes)
    torch.cuda.synchronize()
    assert isinstance(out, client.FlatStateDict)
    x, xs = N(g.flat[0]), [N(m.flat[0]) for m in models]
    rups = restated_uploads(x, xs, S.keep_count(NP, 0.1))
    for u, (i, v) in zip(ups, rups):
        assert np.array_equal(N(u.idx).view(np.uint32), i) and np.array_equal(bits(N(u.val)), bits(v))
    ref = S.chained(x, rups, weights32(sizes), NP, with_base=not opt)
    if opt:
        ref_opt = server.ServerOptimizer("AVGM", lr=0.5, beta1=0.75)
        P = torch.empty(NP, dtype=torch.float32, device=DEV)
        ref_opt.apply_delta(P, g.flat[0], G(ref))
        torch.cuda.synchronize()
        assert torch.equal(out.flat[0], P) and torch.equal(sopt.m, ref_opt.m) and sopt.rounds == 1 and float(sopt.m.abs().max()) > 0
    else:
        assert np.array_equal(bits(N(out.flat[0])), bits(ref)), k
    assert np.array_equal(bits(N(g.flat[0])), bits(x))                        # the global state is read, never written
    assert torch.equal(out.flat[1], avg.flat[1]) and torch.equal(out.flat[2], avg.flat[2]) and out.flat[2].dtype == torch.float32


def test_a_poisoned_client_shows_in_its_element_only():
    """one NaN in one client's state: always sent, NaN in that element of the aggregate and nowhere else, a counter of 1, and a finite
    residual (+0 there)"""
    k, at = 4, 1000
    g, models = synthetic_states(k)
    models[2].flat[0][at] = float("nan")
    comps = [compress.TopKCompressor(0.01) for _ in range(k)]
    ups = [c.compress(g, m) for c, m in zip(comps, models)]
    out = server.FedSparse(g, ups, sizes_of(k))
    torch.cuda.synchronize()
    assert [u.nonfinite_count() for u in ups] == [0, 0, 1, 0]
    got = N(out.flat[0])
    assert np.flatnonzero(np.isnan(got)).tolist() == [at]
    e = N(comps[2].residual)
    assert np.all(np.isfinite(e)) and bits(e)[at] == 0 and np.any(e != 0)


# ---- Server.train ------------------------------------------------------------------------------------------------------------------------
def _tiny_world(aggr, nc, **extra):
    """``nc`` clients on the smallest backbone and batch of the Server.train tests of tests/test_compress_gpu.py (iresnet18, B = 4, two steps each)"""
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
    return srv, clients


def test_server_train_with_topk_uploads(monkeypatch):
    """two rounds, two clients, topk_ratio = 0.01: after each round the global parameters equal the restatement applied to the recorded
    client states (sparsified against the global state the round started from, residuals carried per client, data-size weights), and the
    second round runs on non-zero residuals that differ between the clients"""
    ratio = 0.01
    srv, clients = _tiny_world("FedAvg", 2, topk_ratio=ratio)
    rec = []
    real = server.FedSparse

    def recording(global_state, updates, weights, server_opt=None):
        assert server_opt is None
        rec.append((N(global_state.flat[0]), [N(c.backbone_state_dict.flat[0]) for c in clients], list(weights), [u.nbytes for u in updates],
                    [u.dense_nbytes for u in updates]))
        return real(global_state, updates, weights, server_opt)
    monkeypatch.setattr(server, "FedSparse", recording)
    monkeypatch.setattr(server, "FedPavg", lambda *a: pytest.fail("FedPavg was called on the sparse path"))
    monkeypatch.setattr(server, "FedCompressed", lambda *a, **k: pytest.fail("FedCompressed was called on the sparse path"))
    n = srv.federated_model.flat_state()[0].numel()
    keep = S.keep_count(n, ratio)
    es = [np.zeros(n, dtype=f32) for _ in clients]
    x_prev = N(srv.federated_model.flat_state()[0])
    for r in range(2):
        assert np.isfinite(srv.train())
        srv.step_round()
        torch.cuda.synchronize()
        xg, xs, weights, sent, dense = rec[r]
        assert np.array_equal(bits(xg), bits(x_prev)), "round %d was sparsified against another global state" % r
        assert weights == [300, 100] and not np.array_equal(xs[0], xs[1])
        assert all(s < 0.03 * d for s, d in zip(sent, dense))                 # 8 bytes for 1 % of the parameters + the statistics as they are
        ups = []
        for i in range(2):
            idx, val, es[i], nbad, _ = S.sparsify(xg, xs[i], es[i], keep, fast=True)
            assert nbad == 0
            ups.append((idx, val))
            assert np.array_equal(bits(N(clients[i].sparsifier.residual)), bits(es[i])), (r, i)
        got = N(srv.federated_model.flat_state()[0])
        assert np.array_equal(bits(got), bits(S.chained(xg, ups, weights32(weights), n))), "round %d" % r
        if r == 0:
            assert np.any(es[0] != 0) and np.any(es[1] != 0) and not np.array_equal(es[0], es[1])
        x_prev = got
    assert len(rec) == 2 and all(c.sparsifier.ratio == ratio and c.sparsifier.error_feedback for c in clients)


def test_server_train_without_topk_ratio_is_untouched(monkeypatch):
    """topk_ratio unset: FedPavg is called as before, FedSparse is not, no client grows a sparsifier, and the new global state is FedPavg of
    the client states, bit for bit"""
    calls = []
    real = server.FedPavg
    monkeypatch.setattr(server, "FedPavg", lambda models, weights: (calls.append(([N(m.flat[0]) for m in models], list(weights))), real(models, weights))[1])
    monkeypatch.setattr(server, "FedSparse", lambda *a, **k: pytest.fail("FedSparse was called with topk_ratio unset"))
    srv, clients = _tiny_world("FedAvg", 2)
    assert np.isfinite(srv.train())
    torch.cuda.synchronize()
    assert len(calls) == 1 and not any(hasattr(c, "sparsifier") for c in clients)
    xs, weights = calls[0]
    ws = weights32(weights)
    with np.errstate(invalid="ignore"):
        ref = ws[0] * xs[0]
        ref = ref + ws[1] * xs[1]
    assert np.array_equal(bits(N(srv.federated_model.flat_state()[0])), bits(ref))
