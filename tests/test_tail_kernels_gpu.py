"""The network tail kernel by kernel through the C ABI on raw pointers: BatchNorm1d forward / backward, the split-K slab reductions, dropout,
NCHW -> NHWC, the 16-bit cast, the dgrad weight shadows (single and the whole-network launch), the plain-mode GEMMs of the fc layer and four
small aggregation / PartialFC entry points — against the float64 references and numpy restatements of tests/tail_cases.py (which
tests/test_tail_cases_cpu.py proves admissible and sharp).  Before every call the outputs hold NaN (16-bit and integer buffers: a fill
pattern) and every ld padding, gap and guard band a sentinel; afterwards the padding is intact and every value that is due is a number
within its tolerance, or the exact bits.  Each figure is printed, as a fraction of its tolerance, before it is asserted (pytest -s).  The
storage type is the loaded library's (_C.storage_dtype()): the file runs unchanged on the fp16 and the bf16 build, and
tests/test_bf16_build_gpu.py runs it on the latter."""
import contextlib
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import tail_cases as T  # noqa: E402
from conftest import REPO  # noqa: E402
from fedfr_amd import _C  # noqa: E402

NAN = float("nan")
f32, f64 = torch.float32, torch.float64
GUARD = 256
FILL16 = 0x5555                      # what 16-bit and byte outputs hold before a call (fp16 85.3, bf16 1.5e13: no value a test expects)


def dev():
    return torch.device("cuda:0")


def S16():
    return _C.storage_dtype()


def D(t):
    return t.to(dev()).contiguous()


def galloc(n, dtype=f32):
    """(buffer, view of the first n): an output pre-filled with NaN (fp32) or the fill pattern, with a guard band behind it"""
    if dtype == f32:
        buf = torch.full((n + GUARD,), NAN, dtype=f32, device=dev())
    elif dtype == torch.uint8:
        buf = torch.full((n + GUARD,), 0x55, dtype=torch.uint8, device=dev())
    else:
        buf = torch.full((n + GUARD,), FILL16, dtype=torch.int16, device=dev()).view(dtype)
    return buf, buf[:n]


def guard_ok(buf):
    g = buf[-GUARD:]
    if buf.dtype == f32:
        return bool(torch.isnan(g).all())
    if buf.dtype == torch.uint8:
        return bool((g == 0x55).all())
    return bool((g.view(torch.int16) == FILL16).all())


def run(name, *args):
    _C.call(name, *args, _C.stream())
    torch.cuda.synchronize()


def show(figs):
    for what, kind, worst in figs:
        print("%-90s %-5s %.3g of tol" % (what, kind, worst))


def chk(got, q, what):
    figs = []
    try:
        T.check(got, q, what, out=figs)
    finally:
        show(figs)


def slot_counts():
    out = {}
    for s in range(32):
        ms, n, fl = C.c_double(0), C.c_longlong(0), C.c_double(0)
        _C.call("fedfr_profile_read", s, C.byref(ms), C.byref(n), C.byref(fl))
        if n.value:
            out[s] = n.value
    return out


@contextlib.contextmanager
def launches(expected, what):
    """profiling on; afterwards exactly the expected profile slots have counted the expected launches"""
    _C.call("fedfr_profile_enable", 1)
    try:
        yield
        torch.cuda.synchronize()
        counts = slot_counts()
    finally:
        _C.call("fedfr_profile_enable", 0)
    assert counts == expected, "%s: launches per profile slot %s, expected %s" % (what, counts, expected)


def err_code(name):
    return int(re.search(r"#define %s \((-?\d+)\)" % name, open(os.path.join(REPO, "include", "fedfr_hip.h")).read()).group(1))


def same_bits32(got, want, what):
    assert torch.equal(got.cpu().view(torch.int32), want.cpu().view(torch.int32)), "%s: not bit-equal" % what


# ------------------------------------------------------------------------------------------------ BatchNorm1d
@pytest.mark.parametrize("B,C", T.BN_SHAPES)
def test_bn1d_fwd(B, C):
    """training and eval mode, gamma / beta / the saved statistics each present and NULL: y, save_mean, save_rstd and the updated running
    statistics per column against F.batch_norm in float64; the constant column gives y == beta exactly and rstd == 1 / sqrt(eps)"""
    i = T.BnInputs(B, C)
    x, gamma, beta = D(i.x), D(i.gamma), D(i.beta)
    for training in (1, 0):
        for ug, ub, save in ((1, 1, 1), (0, 1, 1), (1, 0, 1), (0, 0, 1), (1, 1, 0)):
            ref = T.bn_fwd_ref(i, bool(training), ug, ub)
            what = "bn1d_fwd[%d,%d]:train=%d:gamma=%d:beta=%d:save=%d:" % (B, C, training, ug, ub, save)
            (ybuf, y), (mbuf, sm), (rbuf, sr) = galloc(B * C), galloc(C), galloc(C)
            (rmbuf, rm), (rvbuf, rv) = galloc(C), galloc(C)
            rm.copy_(D(i.rm))
            rv.copy_(D(i.rv))
            run("fedfr_bn1d_fwd", x.data_ptr(), y.data_ptr(), B, C, gamma.data_ptr() if ug else None, beta.data_ptr() if ub else None,
                rm.data_ptr(), rv.data_ptr(), T.BN_MOMENTUM, T.BN_EPS, training, sm.data_ptr() if save else None, sr.data_ptr() if save else None)
            y = y.view(B, C)
            chk(y, ref["y"], what + "y")
            if save:
                chk(sm, ref["save_mean"], what + "save_mean")
                chk(sr, ref["save_rstd"], what + "save_rstd")
            else:
                assert bool(torch.isnan(sm).all()) and bool(torch.isnan(sr).all())
            if training:
                chk(rm, ref["rm"], what + "running_mean")
                chk(rv, ref["rv"], what + "running_var")
                want = float(i.beta[T.BN_CONST_COL]) if ub else 0.0
                assert bool((y[:, T.BN_CONST_COL] == want).all()), what + "constant column: y != beta"
                if save:
                    r = float(sr[T.BN_CONST_COL]) * float(np.sqrt(np.float64(np.float32(T.BN_EPS))))
                    print("%-90s rstd sqrt(eps) - 1 = %.3g" % (what + "constant column", r - 1.0))
                    assert abs(r - 1.0) < 2.0 ** -23
            else:
                assert torch.equal(rm.cpu(), i.rm) and torch.equal(rv.cpu(), i.rv), what + "eval mode touched the running statistics"
                if save:
                    assert torch.equal(sm.cpu(), i.rm)
            assert all(guard_ok(b) for b in (ybuf, mbuf, rbuf, rmbuf, rvbuf)), what + "wrote behind an output"
    assert torch.equal(x.cpu(), i.x)


@pytest.mark.parametrize("B,C", T.BN_SHAPES)
def test_bn1d_bwd(B, C):
    """training and frozen mode, gamma present and NULL, every optional output present and NULL: dx per column against autograd in float64,
    dbeta and dx_colsum against their sums of |terms|, the 16-bit outputs == the rounding of the kernel's own dx, dxbt strided by ldt > B
    with its padding columns untouched"""
    i = T.BnInputs(B, C)
    s16, ldt = S16(), T.bn_ldt(B)
    x, dy, gamma = D(i.x), D(i.dy), D(i.gamma)
    for frozen in (0, 1):
        mean, rstd = (D(t) for t in T.bn_bwd_stats(i, bool(frozen)))
        for ug in (1, 0):
            ref = T.bn_bwd_ref(i, ug, bool(frozen))
            what = "bn1d_bwd[%d,%d]:frozen=%d:gamma=%d:" % (B, C, frozen, ug)
            (dxbuf, dx), (dbbuf, dbeta), (csbuf, colsum) = galloc(B * C), galloc(C), galloc(C)
            (hbuf, dxb), (tbuf, dxbt) = galloc(B * C, s16), galloc(C * ldt, s16)
            run("fedfr_bn1d_bwd", dy.data_ptr(), x.data_ptr(), dx.data_ptr(), B, C, gamma.data_ptr() if ug else None, mean.data_ptr(),
                rstd.data_ptr(), dbeta.data_ptr(), colsum.data_ptr(), dxb.data_ptr(), dxbt.data_ptr(), ldt, frozen)
            dx = dx.view(B, C)
            chk(dx, ref["dx"], what + "dx")
            chk(dbeta, ref["dbeta"], what + "dbeta")
            chk(colsum, ref["dx_colsum"], what + "dx_colsum")
            want16 = dx.to(s16)
            T.same16(dxb.view(B, C), want16, what + "dx 16-bit")
            t = dxbt.view(C, ldt)
            T.same16(t[:, :B], want16.t().contiguous(), what + "dx 16-bit transposed")
            assert bool((t[:, B:].contiguous().view(torch.int16) == FILL16).all()), what + "dxbt padding columns written"
            assert all(guard_ok(b) for b in (dxbuf, dbbuf, csbuf, hbuf, tbuf)), what + "wrote behind an output"
            if B == 1 and not frozen:
                assert bool((dx == 0).all()) and bool((colsum == 0).all())
            # every optional output left out: the same dx
            dx2buf, dx2 = galloc(B * C)
            run("fedfr_bn1d_bwd", dy.data_ptr(), x.data_ptr(), dx2.data_ptr(), B, C, gamma.data_ptr() if ug else None, mean.data_ptr(),
                rstd.data_ptr(), None, None, None, None, 0, frozen)
            assert torch.equal(dx2.view(B, C), dx) and guard_ok(dx2buf)


# ------------------------------------------------------------------------------------------------ slab reduction
def _slab_run(slabs, bias=None, bias_n=0, second=None):
    nsplit, n = slabs.shape
    sd = torch.from_numpy(slabs).to(dev())
    dbuf, dst = galloc(n)
    bd = torch.from_numpy(bias).to(dev()) if bias is not None else None
    if second is not None:
        sd1 = torch.from_numpy(second).to(dev())
        d1buf, dst1 = galloc(n)
    with launches({T.SLAB_SLOT: 1}, "reduce_slabs[%d,%d]" % (nsplit, n)):
        _C.call("fedfr_reduce_slabs", dst.data_ptr(), sd.data_ptr(), nsplit, n, bd.data_ptr() if bd is not None else None, bias_n,
                dst1.data_ptr() if second is not None else None, sd1.data_ptr() if second is not None else None, _C.stream())
    assert guard_ok(dbuf) and np.array_equal(sd.cpu().numpy(), slabs)
    if second is not None:
        assert guard_ok(d1buf) and np.array_equal(sd1.cpu().numpy(), second)
        return dst.cpu().numpy(), dst1.cpu().numpy()
    return dst.cpu().numpy()


@pytest.mark.parametrize("nsplit,n", T.SLAB_CASES)
def test_reduce_slabs(nsplit, n):
    """both kernels at every loop structure of the lane schedule, both sides of the width switch, the capped grid's third trip: bit-equal to
    the stated order and within 1e-5 per row of float64"""
    slabs = T.slab_inputs(nsplit, n)
    figs = []
    try:
        T.slab_check(_slab_run(slabs), slabs, what="reduce_slabs[%d,%d]:%s" % (nsplit, n, "wide" if T.slabs_wide(nsplit, n) else "narrow"), out=figs)
    finally:
        show(figs)


def test_reduce_slabs_bias_and_pair():
    figs = []
    try:
        for nsplit, n, bias_n in T.SLAB_BIAS_CASES:
            slabs, bias = T.slab_inputs(nsplit, n), T.slab_bias(bias_n)
            T.slab_check(_slab_run(slabs, bias, bias_n), slabs, bias, what="reduce_slabs[%d,%d]:bias_n=%d" % (nsplit, n, bias_n), out=figs)
        for nsplit, n in T.SLAB_PAIR_CASES:
            s0, s1 = T.slab_inputs(nsplit, n), T.slab_inputs(nsplit, n, seed=1)
            assert not np.array_equal(s0, s1)
            g0, g1 = _slab_run(s0, second=s1)
            T.slab_check(g0, s0, what="reduce_slabs[%d,%d]:pair 0" % (nsplit, n), out=figs)
            T.slab_check(g1, s1, what="reduce_slabs[%d,%d]:pair 1" % (nsplit, n), out=figs)
    finally:
        show(figs)
    # half a second pair, or a bias with one, is an argument error and nothing is written
    sd = torch.zeros(8, device=dev())
    dbuf, dst = galloc(4)
    for args in ((None, 0, dst.data_ptr(), None), (None, 0, None, sd.data_ptr()), (sd.data_ptr(), 4, dst.data_ptr(), sd.data_ptr())):
        with pytest.raises(RuntimeError):
            _C.call("fedfr_reduce_slabs", dst.data_ptr(), sd.data_ptr(), 2, 4, *args, _C.stream())
    torch.cuda.synchronize()
    assert bool(torch.isnan(dbuf).all())


# ------------------------------------------------------------------------------------------------ dropout
def _dropout_fwd(n, p, seed, step, what):
    s16 = S16()
    x16 = T.dropout_values(n, s16, seed=n % 97)
    tbuf, t = galloc(n, s16)
    mbuf, mask = galloc(n, torch.uint8)
    t.copy_(D(x16))
    run("fedfr_dropout_fwd", t.data_ptr(), mask.data_ptr(), n, p, seed, step)
    want = T.dropout_mask(n, p, seed, step)
    got = mask.cpu().numpy()
    assert np.array_equal(got, want), "%s: %d mask bytes differ from the restatement" % (what, int((got != want).sum()))
    T.same16(t, T.dropout_fwd_expect(x16, want, p), what + ":values")
    assert guard_ok(tbuf) and guard_ok(mbuf), what + ": wrote behind an output"


@pytest.mark.parametrize("p", T.DROPOUT_P)
def test_dropout_fwd_mask_is_the_restated_function_of_seed_step_index(p):
    """the mask bytes equal the numpy restatement exactly and the values are storage(x * 1 / (1 - p)) or +0"""
    for seed in T.DROPOUT_SEEDS:
        for step in T.DROPOUT_STEPS:
            for n in T.DROPOUT_N:
                _dropout_fwd(n, p, seed, step, "dropout_fwd[n=%d,p=%g,seed=%d,step=%d]" % (n, p, seed, step))


def test_dropout_fwd_beyond_the_grid_cap():
    _dropout_fwd(T.DROPOUT_N_FWD_BIG, 0.4, 100, 7, "dropout_fwd[n=%d]" % T.DROPOUT_N_FWD_BIG)


@pytest.mark.parametrize("n", T.DROPOUT_N + [T.DROPOUT_N_BWD_BIG])
def test_dropout_bwd_applies_the_same_bytes(n):
    for p in (T.DROPOUT_P if n < 10 ** 6 else [0.4]):
        m = T.dropout_mask(n, p, 100, 1)
        g = T.uniform((n,), 8100 + n % 89)
        dbuf, dx = galloc(n)
        dx.copy_(D(g))
        md = torch.from_numpy(m).to(dev())
        run("fedfr_dropout_bwd", dx.data_ptr(), md.data_ptr(), n, p)
        same_bits32(dx, T.dropout_bwd_expect(g, m, p), "dropout_bwd[n=%d,p=%g]" % (n, p))
        assert guard_ok(dbuf) and np.array_equal(md.cpu().numpy(), m)


# ------------------------------------------------------------------------------------------------ layout and casts
@pytest.mark.parametrize("B,C,HW", T.NHWC_SHAPES)
def test_nchw_to_nhwc16(B, C, HW):
    x = T.uniform((B, C, HW), 300 + C + HW)
    obuf, out = galloc(B * HW * C, S16())
    xd = D(x)
    run("fedfr_nchw_to_nhwc16", xd.data_ptr(), out.data_ptr(), B, C, HW)
    T.same16(out.view(B, HW, C), T.nhwc_ref(x, S16()), "nchw_to_nhwc16[%d,%d,%d]" % (B, C, HW))
    assert guard_ok(obuf)


@pytest.mark.parametrize("n", T.CAST_N)
def test_cast_f32_to_storage(n):
    """the cast behind fedfr_weight_shadows with the dgrad shadow NULL: the scalar tail, the vector body, both, and past the grid cap, on the
    rounding edges and on random bit patterns, bit-exact against the CPU cast"""
    x = T.cast_input(n, seed=n % 7)
    xd = D(x)
    obuf, out = galloc(n, S16())
    run("fedfr_weight_shadows", xd.data_ptr(), out.data_ptr(), None, n, 1, 1)
    T.same16(out, x.to(S16()), "cast[n=%d]" % n)
    assert guard_ok(obuf) and torch.equal(xd.cpu().view(torch.int32), x.view(torch.int32))


def _net_tensors(lib, h):
    q = C.c_longlong()
    assert lib.fedfr_net_query(h, _C.Q_NUM_TENSORS, C.byref(q)) == 0
    out = []
    for i in range(q.value):
        name = C.create_string_buffer(128)
        kind, region, ndim, off, shape = C.c_int(), C.c_int(), C.c_int(), C.c_longlong(), (C.c_int * 4)()
        _C.call("fedfr_net_tensor_info", h, i, name, 128, C.byref(kind), C.byref(region), C.byref(off), C.byref(ndim), shape)
        out.append((name.value.decode(), kind.value, region.value, off.value, tuple(shape)))
    return out


def test_prepare_weights_equals_per_conv_shadows():
    """the whole-network shadow launch (a binary search over the by-value table per workgroup) on a small plan: every block conv's dgrad
    shadow and forward mirror equal the per-conv entry point bit for bit, the mirror equals the cast, nothing else is written"""
    lib, s16 = _C.lib(), S16()
    h = lib.fedfr_net_create((C.c_int * 4)(1, 1, 1, 1), 1, 16, 64)
    assert h
    try:
        q = C.c_longlong()
        vals = {}
        for k in (_C.Q_PARAM_COUNT, _C.Q_TRAINABLE_COUNT, _C.Q_SHADOW_COUNT):
            assert lib.fedfr_net_query(h, k, C.byref(q)) == 0
            vals[k] = q.value
        nparam, ntrain, nshadow = vals[_C.Q_PARAM_COUNT], vals[_C.Q_TRAINABLE_COUNT], vals[_C.Q_SHADOW_COUNT]
        layout, total = T.shadow_layout(_net_tensors(lib, h), ntrain)
        assert total == nshadow and len(layout) == 12
        params = T.uniform((nparam,), 77) * 0.1
        pd = D(params)
        sbuf, shadow = galloc(nshadow, s16)
        run("fedfr_net_prepare_weights", h, pd.data_ptr(), shadow.data_ptr(), 1)
        T.same16(shadow[:ntrain], params[:ntrain].to(s16), "forward mirror")
        first = layout[0][2]
        assert bool((shadow[ntrain:first].view(torch.int16) == FILL16).all()) and guard_ok(sbuf)
        for name, w_off, wd_off, cout, cin, r in layout:
            n = cout * r * r * cin
            w = pd[w_off:w_off + n].clone()
            (bbuf, wb), (dbuf, wdb) = galloc(n, s16), galloc(n, s16)
            run("fedfr_weight_shadows", w.data_ptr(), wb.data_ptr(), wdb.data_ptr(), cout, r, cin)
            T.same16(shadow[w_off:w_off + n], wb, name + ": forward mirror")
            T.same16(shadow[wd_off:wd_off + n], wdb, name + ": dgrad shadow")
            T.same16(wdb.view(cin, r, r, cout), T.dgrad_shadow_ref(params[w_off:w_off + n].view(cout, r, r, cin), s16), name + ": dgrad shadow vs permute")
            assert guard_ok(bbuf) and guard_ok(dbuf)
        # the mirror left to the caller (fwd_shadow_too = 0): only the dgrad region is written
        s2buf, shadow2 = galloc(nshadow, s16)
        run("fedfr_net_prepare_weights", h, pd.data_ptr(), shadow2.data_ptr(), 0)
        assert bool((shadow2[:first].view(torch.int16) == FILL16).all()) and guard_ok(s2buf)
        assert torch.equal(shadow2[first:].view(torch.int16), shadow[first:].view(torch.int16))
    finally:
        lib.fedfr_net_destroy(h)


# ------------------------------------------------------------------------------------------------ plain GEMMs
@pytest.mark.parametrize("exact", [True, False], ids=["exact", "tol"])
@pytest.mark.parametrize("row", T.NT_ROWS, ids=lambda r: "x".join(map(str, r[0])))
def test_gemm_nt_plain_rows(row, exact):
    """fedfr_gemm_nt per tile, with K tails, two and 98 splits and the ring kernel: the profile slot and the launch counts, the result
    bit-equal to float64 (small integers) and within the weight-gradient bound per element (uniform), a workspace of exactly the size
    needed with an untouched guard band behind it, one byte less an error before anything is launched"""
    (M, N, K), _ = row
    slot, splits = T.nt_expected(M, N, K, _C.get_option("nt_glds"))
    s16 = S16()
    a, b = T.gemm_operands(M, N, K, exact, s16, 21)
    ad, bd = D(a.to(s16)), D(b.to(s16))
    assert torch.equal(ad.float().cpu(), a) and torch.equal(bd.float().cpu(), b)
    ref, S = T.gemm_ref(ad, bd)
    ws_bytes = splits * M * N * 4 if splits > 1 else 0
    wbuf, ws = galloc(ws_bytes // 4)
    cbuf, c = galloc(M * N)
    what = "gemm_nt[%d,%d,%d]:%s" % (M, N, K, "exact" if exact else "tol")
    expected = {slot: 1, T.SLAB_SLOT: 1} if splits > 1 else {slot: 1}
    with launches(expected, what):
        _C.call("fedfr_gemm_nt", ad.data_ptr(), bd.data_ptr(), c.data_ptr(), ws.data_ptr() if splits > 1 else None, ws_bytes, M, N, K, _C.stream())
    figs = []
    try:
        T.gemm_check(c.view(M, N), ref, S, K, splits, exact, what, out=figs)
    finally:
        show(figs)
    assert guard_ok(cbuf) and guard_ok(wbuf), what + ": wrote behind an output"
    if splits > 1:
        assert not bool(torch.isnan(ws).any())                 # every slab element was written: the workspace is read as splits x M x N
        c.fill_(NAN)
        rc = _C.lib().fedfr_gemm_nt(ad.data_ptr(), bd.data_ptr(), c.data_ptr(), ws.data_ptr(), ws_bytes - 1, M, N, K, _C.stream())
        torch.cuda.synchronize()
        assert rc == err_code("FEDFR_ERR_WORKSPACE") and "workspace" in _C.last_error() and bool(torch.isnan(c).all())


@pytest.mark.parametrize("use_tr", [1, 0])
@pytest.mark.parametrize("exact", [True, False], ids=["exact", "tol"])
@pytest.mark.parametrize("row", T.TN_ROWS, ids=lambda r: "x".join(map(str, r[0])))
def test_gemm_tn_plain_rows(row, exact, use_tr):
    """fedfr_gemm_tn on each of its four tiles with both LDS read forms, Kp = 1 (a one-image batch) and Kp across two K-steps"""
    (Kp, NI, NJ), slot = row
    s16 = S16()
    pt, qt = T.gemm_operands(NI, NJ, Kp, exact, s16, 22)           # [NI][Kp], [NJ][Kp]
    pd, qd = D(pt.t().contiguous().to(s16)), D(qt.t().contiguous().to(s16))
    ref, S = T.gemm_ref(pd.t(), qd.t())
    cbuf, c = galloc(NI * NJ)
    what = "gemm_tn[%d,%d,%d]:%s:tr=%d" % (Kp, NI, NJ, "exact" if exact else "tol", use_tr)
    with _C.option_scope("tn_use_tr", use_tr):
        with launches({slot: 1}, what):
            _C.call("fedfr_gemm_tn", pd.data_ptr(), qd.data_ptr(), c.data_ptr(), Kp, NI, NJ, _C.stream())
    figs = []
    try:
        T.gemm_check(c.view(NI, NJ), ref, S, Kp, 1, exact, what, out=figs)
    finally:
        show(figs)
    assert guard_ok(cbuf), what + ": wrote behind its output"


# ------------------------------------------------------------------------------------------------ the four small entry points
@pytest.mark.parametrize("n", [1, 257])
def test_fedavg_i64(n):
    """accumulate and overwrite, with and without the truncated copy, counters above 2^24: the three fp32 roundings of the restatement"""
    src, acc0 = T.fedavg_i64_inputs(n)
    sd = torch.from_numpy(src).to(dev())
    for accumulate in (1, 0):
        for trunc in (1, 0):
            abuf, acc = galloc(n)
            acc.copy_(torch.from_numpy(acc0).to(dev()) if accumulate else torch.full((n,), NAN))
            out = torch.full((n + 8,), -12345, dtype=torch.int64, device=dev())
            run("fedfr_fedavg_i64", acc.data_ptr(), sd.data_ptr(), 0.3, n, accumulate, out.data_ptr() if trunc else None)
            v, tr = T.fedavg_i64_order(acc0, src, 0.3, bool(accumulate))
            assert np.array_equal(acc.cpu().numpy(), v), "fedavg_i64[n=%d,acc=%d]" % (n, accumulate)
            assert np.array_equal(out[:n].cpu().numpy(), tr if trunc else np.full(n, -12345)) and bool((out[n:] == -12345).all())
            assert guard_ok(abuf) and np.array_equal(sd.cpu().numpy(), src)


def test_pfc_rand():
    for n in (1, 255, 4099):
        arrs = []
        for seed, step in ((5, 0), (5, 1), (2 ** 63 + 5, 7)):
            pbuf, perm = galloc(n)
            run("fedfr_pfc_rand", perm.data_ptr(), n, seed, step)
            got = perm.cpu().numpy()
            assert np.array_equal(got, T.pfc_rand_order(n, seed, step)) and got.min() >= 0 and got.max() < 1 and guard_ok(pbuf)
            arrs.append(got)
        assert n == 1 or not np.array_equal(arrs[0], arrs[1])


def test_pfc_localize():
    start, nl = 1000, 300
    edge = [start - 1, start, start + nl - 1, start + nl, -1, 0]
    lab = torch.tensor(edge + torch.randint(0, 2000, (600,), generator=torch.Generator().manual_seed(3)).tolist(), dtype=torch.int64)
    n = lab.numel()
    for with_perm in (1, 0):
        ld = torch.full((n + 8,), -99, dtype=torch.int64, device=dev())
        ld[:n] = D(lab)
        pbuf, perm = galloc(nl)
        perm.fill_(0.5)
        run("fedfr_pfc_localize", ld.data_ptr(), n, start, nl, perm.data_ptr() if with_perm else None)
        want, wperm = T.pfc_localize_ref(lab, start, nl, torch.full((nl,), 0.5) if with_perm else None)
        assert torch.equal(ld[:n].cpu(), want) and want[:4].tolist() == [-1, 0, nl - 1, -1] and bool((ld[n:] == -99).all())
        assert torch.equal(perm.cpu(), wperm if with_perm else torch.full((nl,), 0.5)) and guard_ok(pbuf)


def test_pfc_positive():
    for n, pos in ((3000, []), (3000, [2999]), (3000, None), (1, [0]), (1024, None), (1025, [0, 1023, 1024])):
        perm = torch.rand(n, generator=torch.Generator().manual_seed(n)) * 0.999
        if pos is None:
            pos = torch.nonzero(torch.rand(n, generator=torch.Generator().manual_seed(n + 1)) < 0.3).flatten().tolist()
        perm[pos] = 2.0
        want = torch.nonzero(perm == 2).flatten()
        index = torch.full((n + 8,), -7, dtype=torch.int64, device=dev())
        count = torch.full((2,), -7, dtype=torch.int32, device=dev())
        pd = D(perm)
        run("fedfr_pfc_positive", pd.data_ptr(), n, index.data_ptr(), count.data_ptr())
        k = int(count[0])
        assert k == want.numel() and int(count[1]) == -7
        assert torch.equal(index[:k].cpu(), want) and bool((index[k:] == -7).all())
