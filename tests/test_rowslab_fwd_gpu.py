"""Direct float64 parity of the row-slab FORWARD BatchNorm passes and the sphnet PReLU passes, kernel by kernel through the C ABI:
fedfr_bn_apply (all four <X2, STATS> instantiations, every operand present and NULL, the nchw_hw store), fedfr_bn_finalize (both sides of its
row-group loop and the staged column sum behind P > 1024), fedfr_prelu_bwd_pass (<ADD> and plain), fedfr_prelu_bwd_finalize / _multi,
fedfr_bn_eval_coeffs and the legacy fedfr_bias_prelu_bwd.  Inputs, tables, float64 references and tolerances: tests/rowslab_cases.py
(tests/test_rowslab_cases_cpu.py proves the tolerances reachable and tight enough to see one row, one pixel, one mask, one slope).

Every output holds NaN before the call, geometry is asserted from the library's own row queries (a retune of the slab sizes fails here instead
of skipping a path), the worst error / tolerance per quantity is printed, and the storage type is the loaded library's (_C.storage_dtype()):
the file runs unchanged on the fp16 and on the bf16 build, and test_bf16_build_in_a_child_process runs it on the latter."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

import rowslab_cases as K
from fedfr_amd import _C

pytestmark = pytest.mark.gpu
f32, f64 = K.f32, K.f64
NAN = float("nan")
WORST = {}


def dev():
    return torch.device("cuda:0")


def S16():
    return _C.storage_dtype()


def d(t):
    return None if t is None else t.contiguous().to(dev())


def nan(shape, dtype=f32):
    return torch.full(shape, NAN, dtype=dtype, device=dev())


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int16)


def all_nan(*ts):
    return all(bool(torch.isnan(t.float()).all()) for t in ts)


def chk(got, q, key, name):
    r = K.err_over_tol(got, q)
    WORST[key] = max(WORST.get(key, 0.0), r)
    assert r <= 1.0, "%s %s: error is %.3g of its tolerance" % (name, key, r)


def report(prefix):
    print("worst error / tolerance [%s]:" % str(S16()).split(".")[-1], {k: round(v, 4) for k, v in sorted(WORST.items()) if k.startswith(prefix)})


def rc_of(name, *args):
    rc = getattr(_C.lib(), name)(*args)
    torch.cuda.synchronize()
    return rc


# ------------------------------------------------------------------------------------------------ 1. fedfr_bn_apply
def bn_apply(c, nchw_hw=0):
    M, C = c.M, c.C
    rows = _C.lib().fedfr_bn_apply_stat_rows(M, C)
    assert rows == c.g["grid"], (rows, c.g)
    k = {n: d(t) for n, t in c.op.items()}
    x1, x2 = d(c.x), d(c.x2)
    y = nan((M, C), S16())
    stats = nan((rows, 2, C)) if c.stats else None
    _C.call("fedfr_bn_apply", x1.data_ptr(), _C.ptr(k["sc1"]), _C.ptr(k["sh1"]), _C.ptr(k["alpha"]), _C.ptr(x2), _C.ptr(k["sc2"]), _C.ptr(k["sh2"]),
            y.data_ptr(), M, C, nchw_hw, _C.ptr(stats), _C.stream())
    torch.cuda.synchronize()
    return y.cpu(), None if stats is None else stats.cpu()


def _apply_cases(C, exact):
    for Cc, kind, M, v, stats in K.apply_table():
        if Cc == C and kind != "slab_grows":
            yield K.ApplyCase(Cc, M, v, stats, S16(), exact)


def _check_apply(c, y, stats):
    if c.exact:
        ref = c.y()[0]
        assert torch.equal(y.to(f64), ref), "%s: y differs in %d elements" % (c.name, int((y.to(f64) != ref).sum()))
        if stats is not None:
            sq = c.stats_q(y)
            assert torch.equal(stats.to(f64), sq.value), "%s: statistics rows differ, max %.3g" % (c.name, float((stats.to(f64) - sq.value).abs().max()))
    else:
        chk(y, c.y_q(), "bn_apply y", c.name)
        if stats is not None:
            chk(stats, c.stats_q(y), "bn_apply stats rows", c.name)       # against the stored y that came back
    if c.variant == "ident":
        assert torch.equal(bits(y), bits(c.x)), c.name


@pytest.mark.parametrize("tier", ["exact", "tol"])
@pytest.mark.parametrize("C", K.CHANNELS)
def test_bn_apply(C, tier):
    """Every table row of one channel count: exact tier torch.equal on y and on every statistics row; tolerance tier y element-wise and each
    statistics row against the sums of the STORED y over that slab's rows."""
    try:
        for c in _apply_cases(C, tier == "exact"):
            y, stats = bn_apply(c)
            _check_apply(c, y, stats)
    finally:
        report("bn_apply")


@pytest.mark.parametrize("tier", ["exact", "tol"])
def test_bn_apply_slab_grows(tier):
    """C = 512, M = 1024 x 32 + 1: ceil(M / 1024) = 33 rows exceed the minimum slab of 32 and are rounded up to 36"""
    Cc, kind, M, v, stats = [r for r in K.apply_table() if r[1] == "slab_grows"][0]
    c = K.ApplyCase(Cc, M, v, stats, S16(), tier == "exact")
    assert c.g["slab"] == 36 and _C.lib().fedfr_bn_apply_stat_rows(M, Cc) == -(-M // 36)
    try:
        y, st = bn_apply(c)
        _check_apply(c, y, st)
    finally:
        report("bn_apply")


@pytest.mark.parametrize("C", [96, 512])
def test_bn_apply_nchw(C):
    """nchw_hw in {1, 5, 49}: the flatten-order store equals the permuted nchw_hw = 0 result of the same call BIT FOR BIT, statistics rows included;
    the nchw_hw = 0 result itself is held to the tolerance tier"""
    try:
        for Cc, hw, B, v, stats in K.nchw_table():
            if Cc != C:
                continue
            for exact in (True, False):
                c = K.ApplyCase(Cc, B * hw, v, stats, S16(), exact)
                y0, s0 = bn_apply(c)
                _check_apply(c, y0, s0)
                y1, s1 = bn_apply(c, nchw_hw=hw)
                assert torch.equal(bits(y1).reshape(B, Cc, hw), bits(K.nchw(y0, hw))), c.name + " nchw_hw=%d" % hw
                if stats:
                    assert torch.equal(s1, s0), c.name
    finally:
        report("bn_apply")


def test_bn_apply_refuses_bad_shapes():
    for M, C in K.APPLY_ERRORS:
        n = max(M, 1) * max(C, 8)
        x, y, st, v = torch.zeros(n, dtype=S16(), device=dev()), nan((n,), S16()), nan((2 * n,)), torch.ones(max(C, 8), device=dev())
        rc = rc_of("fedfr_bn_apply", x.data_ptr(), v.data_ptr(), v.data_ptr(), None, None, None, None, y.data_ptr(), M, C, 0, st.data_ptr(), _C.stream())
        assert rc != 0 and b"bn_apply" in _C.lib().fedfr_last_error_string() and all_nan(y, st), (M, C, rc)


# ------------------------------------------------------------------------------------------------ 2. fedfr_bn_finalize
FIN_OUT = ("scale", "shift", "mean", "rstd")


def bn_finalize(rows, C, count, gamma, beta, rm0, rv0, tmp="auto"):
    P = rows.shape[0]
    out = {n: nan((C,)) for n in FIN_OUT}
    if rm0 is not None:
        out["rm"], out["rv"] = d(rm0).clone(), d(rv0).clone()
    t = nan((K.STAGE_S * 2 * C,)) if tmp == "auto" else tmp
    r, g, b = d(rows), d(gamma), d(beta)
    rc = rc_of("fedfr_bn_finalize", r.data_ptr(), P, C, float(count), _C.ptr(g), _C.ptr(b), _C.ptr(out.get("rm")), _C.ptr(out.get("rv")), K.MOMENTUM,
               K.EPS32, *[out[n].data_ptr() for n in FIN_OUT], _C.ptr(t), _C.stream())
    return rc, {n: v.cpu() for n, v in out.items()}, t


@pytest.mark.parametrize("C", K.FIN_C)
def test_bn_finalize(C):
    """The rows are inputs (fp64 sums of uneven row ranges, rounded once): the six outputs against the float64 value of bn_math.h's expressions on
    the summed rows — one fp32 store each, the fp64 cancellation, and behind P > 1024 the staged slices' one fp32 rounding."""
    try:
        for P, Cc, kind, null in K.finalize_table():
            if Cc != C:
                continue
            c = K.FinalizeCase(P, Cc, kind, null)
            run = "running" not in c.null
            rc, out, tmp = bn_finalize(c.rows, Cc, c.count, None if "gamma" in c.null else c.gamma, None if "beta" in c.null else c.beta,
                                       c.rm0 if run else None, c.rv0 if run else None)
            assert rc == 0, _C.last_error()
            assert all_nan(tmp) == (P <= 1024)                             # the staged sum is taken exactly when P > 1024
            q = c.outputs()
            assert set(q) == set(out)
            for n in q:
                chk(out[n], q[n], "bn_finalize %s%s" % (n, " staged" if c.staged else ""), c.name)
            if c.count == c.M:
                one = 1.0 / float(torch.tensor(K.EPS32, dtype=f64).sqrt())
                assert abs(float(out["rstd"][K.CONST]) / one - 1.0) <= 2.0 ** -23  # variance clamped at 0: rstd == 1 / sqrt(eps) to one fp32 ulp
            if c.staged and c.count == c.M:
                print("%s: the staged slices allow %.0f fp32 roundings of rstd on the 32 sigma channel" % (c.name, c.stage_over_store["rstd"]))
    finally:
        report("bn_finalize")


def test_bn_finalize_row_order_and_errors():
    """P <= 1024, rows whose every partial sum is exact: forward and reversed row order give the same six outputs bit for bit.  P > 1024 without tmp
    and C % 8 != 0 are argument errors that leave every output untouched."""
    for P, C in ((127, 8), (257, 24), (1024, 64), (300, 512)):
        rows = K.exact_fin_rows(P, C)
        c = K.FinalizeCase(2, C)
        a = bn_finalize(rows, C, 3.0 * P, c.gamma, c.beta, c.rm0, c.rv0)
        b = bn_finalize(rows.flip(0), C, 3.0 * P, c.gamma, c.beta, c.rm0, c.rv0)
        assert a[0] == 0 and b[0] == 0
        for n in a[1]:
            assert torch.equal(a[1][n], b[1][n]) and bool(torch.isfinite(a[1][n]).all()), (P, C, n)
    c = K.FinalizeCase(1025, 8)
    rc, out, _ = bn_finalize(c.rows, 8, c.count, c.gamma, c.beta, None, None, tmp=None)
    assert rc != 0 and b"tmp" in _C.lib().fedfr_last_error_string() and all_nan(*out.values())
    rows = torch.zeros(4, 2, 12)
    rc, out, tmp = bn_finalize(rows, 12, 8.0, None, None, None, None)
    assert rc != 0 and all_nan(tmp, *out.values())


# ------------------------------------------------------------------------------------------------ 3. fedfr_prelu_bwd_pass
def prelu_pass(c, dy, add, want_gsum=True):
    M, C = c.M, c.C
    rows = _C.lib().fedfr_prelu_bwd_rows(M, C)
    assert rows == c.g["grid"], (rows, c.g)
    k = [d(dy), d(add), d(c.x), d(c.bias), d(c.alpha)]
    gsum, dz, r = nan((M, C), S16()) if want_gsum else None, nan((M, C), S16()), nan((rows, 2, C))
    rc = rc_of("fedfr_prelu_bwd_pass", *[_C.ptr(t) for t in k], M, C, _C.ptr(gsum), dz.data_ptr(), r.data_ptr(), _C.stream())
    return rc, None if gsum is None else gsum.cpu(), dz.cpu(), r.cpu()


def _check_prelu(c):
    rc, gsum, dz, rows = prelu_pass(c, c.dy, c.add)
    assert rc == 0, _C.last_error()
    if c.add is None:
        assert all_nan(gsum)                                              # nothing to store without an addend
        g16 = c.dy
    else:
        assert torch.equal(bits(gsum), bits((c.dy.float() + c.add.float()).to(S16()))), c.name + ": gsum"
        g16 = gsum
    chk(dz, c.dz_q(g16), "prelu_bwd_pass dz", c.name)
    chk(rows, c.rows_q(g16), "prelu_bwd_pass rows" + (" (shuffle path)" if c.g["tpr"] <= 64 and c.g["tpr"] & (c.g["tpr"] - 1) == 0 else " (LDS path)"), c.name)
    if c.add is not None:                                                 # the ADD pass IS the plain pass run on its own gsum
        rc2, _, dz2, rows2 = prelu_pass(c, gsum, None, want_gsum=False)
        assert rc2 == 0 and torch.equal(bits(dz2), bits(dz)) and torch.equal(rows2, rows), c.name + ": ADD pass != plain pass on its gsum"


@pytest.mark.parametrize("C", K.CHANNELS)
def test_prelu_bwd_pass(C):
    try:
        for Cc, kind, M, add, bias in K.prelu_table():
            if Cc == C and kind != "slab_grows":
                _check_prelu(K.PreluCase(Cc, M, add, bias, S16()))
    finally:
        report("prelu_bwd_pass")


def test_prelu_bwd_pass_slab_grows_and_errors():
    Cc, kind, M, add, bias = [r for r in K.prelu_table() if r[1] == "slab_grows"][0]
    c = K.PreluCase(Cc, M, add, bias, S16())
    assert c.g["slab"] == 36 and _C.lib().fedfr_prelu_bwd_rows(M, Cc) == -(-M // 36)
    try:
        _check_prelu(c)
    finally:
        report("prelu_bwd_pass")
    c = K.PreluCase(64, 300, True, True, S16())
    rc, gsum, dz, rows = prelu_pass(c, c.dy, c.add, want_gsum=False)      # an addend without gsum
    assert rc != 0 and b"prelu_bwd_pass" in _C.lib().fedfr_last_error_string() and all_nan(dz, rows)


@pytest.mark.parametrize("C,M,bias", K.LEGACY_TABLE)
def test_legacy_bias_prelu_bwd(C, M, bias):
    """fedfr_bias_prelu_bwd (reduce pass, fp64 finalize, apply pass with the coefficients (1, 0, 0)) against the same float64 references: dx at the
    one-pass form's tolerance, dbias / dalpha at its rows' tolerance summed (+ the fp32 store)"""
    c = K.PreluCase(C, M, False, bias, S16())
    P = _C.lib().fedfr_bn_bwd_rows(M, C)
    assert P == c.g["grid"]
    part, coef, db, da, dx = nan((P, 3, C)), nan((3, C)), nan((C,)), nan((C,)), nan((M, C), S16())
    k = [d(c.dy), d(c.x), d(c.bias), d(c.alpha)]
    _C.call("fedfr_bias_prelu_bwd", *[_C.ptr(t) for t in k], M, C, part.data_ptr(), coef.data_ptr(), db.data_ptr(), da.data_ptr(), None, dx.data_ptr(),
            _C.stream())
    torch.cuda.synchronize()
    try:
        chk(dx, c.dz_q(c.dy), "bias_prelu_bwd dx", c.name)
        qb, qa = c.grads_q(c.dy)
        chk(db, qb, "bias_prelu_bwd dbias", c.name)
        chk(da, qa, "bias_prelu_bwd dalpha", c.name)
    finally:
        report("bias_prelu_bwd")


# ------------------------------------------------------------------------------------------------ 4. fedfr_prelu_bwd_finalize (+ multi)
def prelu_finalize(rows, want=(True, True)):
    P, nv, C = rows.shape
    assert nv == 2
    r = d(rows)
    out = [nan((C,)) if w else None for w in want]
    rc = rc_of("fedfr_prelu_bwd_finalize", r.data_ptr(), P, C, _C.ptr(out[0]), _C.ptr(out[1]), _C.stream())
    assert rc == 0, _C.last_error()
    return [None if o is None else o.cpu() for o in out]


def test_prelu_bwd_finalize():
    try:
        for i, P in enumerate(K.PFIN_P):
            for C in K.PFIN_C:
                rows = K.prelu_rows(P, C)
                q = K.prelu_fin_q(rows)
                want = [(True, True), (True, False), (False, True)][(i + C // 8) % 3]         # either output NULL
                got = prelu_finalize(rows, want)
                for j, n in enumerate(("dbias", "dalpha")):
                    if want[j]:
                        chk(got[j], q[j], "prelu_bwd_finalize " + n, "P=%d C=%d" % (P, C))
    finally:
        report("prelu_bwd_finalize")


@pytest.mark.parametrize("name", ["n1", "n2", "n64"])
def test_prelu_bwd_finalize_multi(name):
    """Entry by entry torch.equal to the single finalize (one fin8_accumulate serves both); a third statistic of NaN is never read; every float of
    `grads` outside the named ranges is untouched"""
    ent = K.multi_tables()[name]
    lay = K.MultiLayout(ent)
    n = len(ent)
    base, grads = d(lay.base), nan((lay.n_grads,))
    arr = lambda t, v: (t * n)(*v)      # noqa: E731
    rc = rc_of("fedfr_prelu_bwd_finalize_multi", base.data_ptr(), grads.data_ptr(), n, arr(ctypes.c_ulonglong, lay.rows_off), arr(ctypes.c_longlong, lay.dbias_off),
               arr(ctypes.c_longlong, lay.dalpha_off), arr(ctypes.c_int, [e[0] for e in ent]), arr(ctypes.c_int, [e[1] for e in ent]),
               arr(ctypes.c_int, [e[2] for e in ent]), _C.stream())
    assert rc == 0, _C.last_error()
    g = grads.cpu()
    assert bool(torch.isnan(g[~lay.named]).all()) and bool(torch.isfinite(g[lay.named]).all())
    try:
        for (P, C, nv, has_b), rows, bo, ao in zip(ent, lay.rows, lay.dbias_off, lay.dalpha_off):
            single = prelu_finalize(rows[:, :2].contiguous())
            q = K.prelu_fin_q(rows)
            if has_b:
                assert torch.equal(g[bo: bo + C], single[0]), (P, C, nv)
            assert torch.equal(g[ao: ao + C], single[1]), (P, C, nv)
            chk(g[ao: ao + C], q[1], "prelu_bwd_finalize_multi dalpha", "P=%d C=%d nv=%d" % (P, C, nv))
    finally:
        report("prelu_bwd_finalize")


def test_prelu_bwd_finalize_multi_refuses_bad_tables():
    base, grads = torch.zeros(4096, device=dev()), nan((4096,))
    for n, C in ((0, 8), (K.MAX_PRELU_FIN + 1, 8), (1, 12)):
        m = max(n, 1)
        arr = lambda t, v: (t * m)(*([v] * m))      # noqa: E731
        rc = rc_of("fedfr_prelu_bwd_finalize_multi", base.data_ptr(), grads.data_ptr(), n, arr(ctypes.c_ulonglong, 0), arr(ctypes.c_longlong, -1),
                   arr(ctypes.c_longlong, 0), arr(ctypes.c_int, 2), arr(ctypes.c_int, C), arr(ctypes.c_int, 2), _C.stream())
        assert rc != 0 and b"prelu_bwd_finalize_multi" in _C.lib().fedfr_last_error_string() and all_nan(grads), (n, C)


# ------------------------------------------------------------------------------------------------ 5. fedfr_bn_eval_coeffs
@pytest.mark.parametrize("n", [1, K.MAX_BN_EVAL])
def test_bn_eval_coeffs(n):
    c = K.EvalCase(n)
    params, bufs, save = d(c.params), d(c.bufs), nan((c.n_save,))
    arr = lambda v: (ctypes.c_int * n)(*v)      # noqa: E731
    rc = rc_of("fedfr_bn_eval_coeffs", params.data_ptr(), bufs.data_ptr(), save.data_ptr(), n, arr(c.C), arr(c.g_off), arr(c.b_off), arr(c.rm_off),
               arr(c.rv_off), arr(c.save_off), K.EPS32, _C.stream())
    assert rc == 0, _C.last_error()
    s = save.cpu()
    assert bool(torch.isnan(s[~c.named]).all()) and bool(torch.isfinite(s[c.named]).all())
    try:
        for i in range(n):
            C, o = c.C[i], c.save_off[i]
            q = c.entry(i)
            for j, name in enumerate(("scale", "shift", "mean", "rstd")):
                chk(s[o + j * C: o + (j + 1) * C], q[name], "bn_eval_coeffs " + name, "%s entry %d" % (c.name, i))
            assert torch.equal(s[o + 2 * C: o + 3 * C], c.bufs[c.rm_off[i]: c.rm_off[i] + C])
    finally:
        report("bn_eval_coeffs")
    if n == 1:
        rc = rc_of("fedfr_bn_eval_coeffs", params.data_ptr(), bufs.data_ptr(), save.data_ptr(), K.MAX_BN_EVAL + 1, arr(c.C), arr(c.g_off), arr(c.b_off),
                   arr(c.rm_off), arr(c.rv_off), arr(c.save_off), K.EPS32, _C.stream())
        assert rc != 0 and b"bn_eval_coeffs" in _C.lib().fedfr_last_error_string()


# ------------------------------------------------------------------------------------------------ the bf16 build
def test_bf16_build_in_a_child_process():
    """this file again under FEDFR_HIP_LIB_NAME=libfedfr_hip_bf16.so (a fresh process: the library is chosen at import)"""
    if S16() != torch.float16:
        pytest.skip("this process already runs on the bf16 build")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert os.path.exists(os.path.join(root, "fedfr_amd", "libfedfr_hip_bf16.so")), "libfedfr_hip_bf16.so is not built (make -C fedfr_amd/csrc bf16)"
    env = dict(os.environ, FEDFR_HIP_LIB_NAME="libfedfr_hip_bf16.so")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-s", "-p", "no:cacheprovider", "-k", "not child_process"],
                       env=env, capture_output=True, text=True, timeout=900, cwd=root)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "bfloat16" in r.stdout and "float16]" not in r.stdout.replace("bfloat16]", "")      # it really was the bf16 build
    print("\n".join(t[t.index("worst error"):] for t in r.stdout.splitlines() if "worst error" in t))
