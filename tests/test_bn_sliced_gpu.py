"""Direct float64 parity of the channel-sliced BatchNorm passes (csrc/bn_sliced.hip), one entry point at a time through the C ABI:
fedfr_bn_apply_sliced, fedfr_bn_apply2_sliced, fedfr_bn_bwd_sliced and the *_rows / *_ok queries.  Inputs, float64 references, element-wise
tolerances and the table of shapes: tests/bn_sliced_cases.py (tests/test_bn_sliced_cases_cpu.py proves every tolerance reachable by a correct
fp32 kernel with a factor of four to spare, and tight enough to see one row, one pixel, one mask).  Each table row records the kernel
instantiation it is for; the geometry it relies on is asserted against the library's own queries, so a retune fails here instead of silently
leaving a branch untested.  Every output holds NaN before a call.  The worst error / tolerance of every quantity is printed before it is
asserted (pytest -s) and collected per instantiation (test_zz_margins prints the table).  The storage type is the loaded library's
(_C.storage_dtype()): the file runs unchanged on the fp16 and the bf16 build, and tests/test_bf16_build_gpu.py runs it on the latter."""
import pytest
import torch

import bn_sliced_cases as S
from fedfr_amd import _C

pytestmark = pytest.mark.gpu
f32, f64 = S.f32, S.f64
NAN = float("nan")
MARGINS = {}           # (entry point, instantiation, where the rows came from, fp32 or 16-bit quantity) -> worst error / tolerance seen


def dev():
    return torch.device("cuda:0")


def S16():
    return _C.storage_dtype()


def d(t):
    return None if t is None else t.contiguous().to(dev())


def nan(*shape, dtype=f32):
    return torch.full(shape, NAN, dtype=dtype, device=dev())


STORED16 = (" y", " dx", " out", " y2")     # quantities rounded to 16 bits on the way out: their margin is the rounding itself, up to 1


RAN = {"bwd": 0}       # backward tests that came this far (test_zz_margins asks for the whole table only after the whole file)


def note(out, entry, variant, rows="given rows"):
    for what, r in out:
        k = (entry, variant, rows, "16-bit" if what.endswith(STORED16) else "fp32")
        MARGINS[k] = max(MARGINS.get(k, 0.0), r)


def assert_geometry(M, C):
    fw, bw = S.GEOMETRY[(M, C)]
    lib = _C.lib()
    assert lib.fedfr_bn_sliced_rows(M, C, 0) == fw[0] == S.sliced_geometry(M, C)[0], (M, C)
    assert lib.fedfr_bn_sliced_rows(M, C, 1) == bw[0] == S.sliced_geometry(M, C, True)[0], (M, C)


# ------------------------------------------------------------------------------------------------ the three calls
def run_apply(c, gamma=None, beta=None, stats=None, rows=None, stats_buf=None, rc=False, P=None):
    """one fedfr_bn_apply_sliced call on the case's tensors; gamma / beta: override what the case passes (a tensor instead of NULL)"""
    M, C = c.M, c.C
    rows = c.rows if rows is None else rows
    P = rows.shape[0] if P is None else P
    k = dict(part=d(rows), gamma=d(c.gamma if gamma is None else gamma), beta=d(c.beta if beta is None else beta), rm=d(c.rm), rv=d(c.rv),
             x=d(c.x), alpha=d(c.p.alpha) if c.prelu else None, x2=d(c.x2))
    o = dict(scale=nan(C), shift=nan(C), mean=nan(C), rstd=nan(C), y=nan(M, C, dtype=S16()), rm=k["rm"], rv=k["rv"])
    want = c.stats if stats is None else stats
    o["stats"] = (nan(c.G, 2, C) if stats_buf is None else stats_buf) if want else None
    g = lambda n: _C.ptr(k[n])        # noqa: E731
    code = _C.lib().fedfr_bn_apply_sliced(g("part"), P, float(M), g("gamma"), g("beta"), g("rm"), g("rv"), S.MOM, S.EPSF, o["scale"].data_ptr(),
                                          o["shift"].data_ptr(), o["mean"].data_ptr(), o["rstd"].data_ptr(), g("x"), g("alpha"), g("x2"),
                                          o["y"].data_ptr(), M, C, _C.ptr(o["stats"]), _C.stream())
    torch.cuda.synchronize()
    if rc:
        return code, o
    _C.check(code, "fedfr_bn_apply_sliced")
    return o


def run_apply2(c, rows=None, rc=False, P=None):
    M, C = c.M, c.C
    rows = c.rows if rows is None else rows
    P = rows.shape[0] if P is None else P
    k = [d(t) for t in (rows, c.p.gamma, c.p.beta, c.xmean, c.xrstd, c.np.gamma, c.np.beta, c.x, c.x2)]
    o = dict(rm=d(c.rm), rv=d(c.rv), nrm=d(c.nrm), nrv=d(c.nrv), out=nan(M, C, dtype=S16()), y2=nan(M, C, dtype=S16()))
    for n in ("scale", "shift", "mean", "rstd", "nscale", "nshift", "nmean", "nrstd"):
        o[n] = nan(C)
    p = lambda n: o[n].data_ptr()     # noqa: E731
    code = _C.lib().fedfr_bn_apply2_sliced(k[0].data_ptr(), P, float(M), S.MOM, S.EPSF, k[1].data_ptr(), k[2].data_ptr(), p("rm"), p("rv"),
                                           p("scale"), p("shift"), p("mean"), p("rstd"), k[3].data_ptr(), k[4].data_ptr(), k[5].data_ptr(),
                                           k[6].data_ptr(), p("nrm"), p("nrv"), p("nscale"), p("nshift"), p("nmean"), p("nrstd"), k[7].data_ptr(),
                                           k[8].data_ptr(), p("out"), p("y2"), M, C, _C.stream())
    torch.cuda.synchronize()
    if rc:
        return code, o
    _C.check(code, "fedfr_bn_apply2_sliced")
    return o


def run_bwd(c, rows=None, nx=None, npart=None, rc=False):
    """one fedfr_bn_bwd_sliced call.  rows: [P][3][C] given rows (rows_in = P), None = the reduce pass fills NaN-filled partials; nx: False
    to leave the next-BatchNorm reduction out of a case that has one"""
    M, C = c.M, c.C
    with_nx = c.has_nx if nx is None else nx
    k = dict(dy=d(c.dy), x=d(c.x), mean=d(c.p.mean), rstd=d(c.p.rstd), gamma=d(c.p.gamma), alpha=d(c.p.alpha) if c.alpha else None, sc=d(c.p.sc),
             sh=d(c.p.sh), add=d(c.add), nx=d(c.nx) if with_nx else None, nmean=d(c.np.mean) if with_nx else None,
             nrstd=d(c.np.rstd) if with_nx else None)
    o = dict(part=nan(c.G, 3, C) if rows is None else d(rows), dx=nan(M, C, dtype=S16()))
    for n in ("dgamma", "dbeta", "dalpha"):
        o[n] = None if n in c.null or (n == "dalpha" and not c.alpha) else nan(C)
    o["npart"] = (nan(c.G, 3, C) if npart is None else npart) if with_nx else None
    g = lambda n: _C.ptr(k[n])        # noqa: E731
    code = _C.lib().fedfr_bn_bwd_sliced(g("dy"), g("x"), g("mean"), g("rstd"), g("gamma"), g("alpha"), g("sc"), g("sh"), M, C, o["part"].data_ptr(),
                                        0 if rows is None else rows.shape[0], _C.ptr(o["dgamma"]), _C.ptr(o["dbeta"]), _C.ptr(o["dalpha"]), g("add"),
                                        o["dx"].data_ptr(), g("nx"), g("nmean"), g("nrstd"), _C.ptr(o["npart"]), _C.stream())
    torch.cuda.synchronize()
    if rc:
        return code, o
    _C.check(code, "fedfr_bn_bwd_sliced")
    return o


def same(a, b, names, what):
    for n in names:
        if a[n] is None and b[n] is None:
            continue
        assert not bool(torch.isnan(a[n].float()).any()), (what, n)
        assert torch.equal(a[n], b[n]), "%s: %s differs by up to %g" % (what, n, float((a[n].double() - b[n].double()).abs().max()))


# ================================================================================================ bn_apply_sliced
@pytest.mark.parametrize("key", list(S.FWD_TABLE))
def test_apply(key):
    c = S.case("apply", key, S16())
    M, C = c.M, c.C
    assert_geometry(M, C)
    assert _C.lib().fedfr_bn_sliced_ok(M, C, c.P, 0) == 1
    r = run_apply(c)
    out = []
    try:
        cq = c.coef()
        for n in ["mean", "rstd", "scale", "shift"] + (["rm", "rv"] if c.rm is not None else []):
            S.check(r[n], cq[n], c.name + " " + n, out=out)
        S.check(r["y"], c.y(r["scale"].cpu(), r["shift"].cpu()), c.name + " y", out=out)
        if c.stats:
            S.check(r["stats"], c.stats_q(r["y"].cpu()), c.name + " stats rows", out=out)
    finally:
        print(c.variant, out)
        note(out, "bn_apply_sliced", c.variant)
    # statistics rows requested or not: the same tensor and coefficients
    if M <= 4096:
        same(r, run_apply(c, stats=not c.stats), ["y", "scale", "shift", "mean", "rstd", "rm", "rv"], c.name + " with / without stats rows")
    # a null optional vector = the vector of its default values
    if "gamma" in c.null or "beta" in c.null:
        r1 = run_apply(c, gamma=torch.ones(C) if "gamma" in c.null else None, beta=torch.zeros(C) if "beta" in c.null else None)
        same(r, r1, ["y", "scale", "shift", "mean", "rstd", "rm", "rv", "stats"], c.name + " null vector vs default values")
    if M > 4096:
        S.drop("apply", key, S16())


# ================================================================================================ bn_apply2_sliced
@pytest.mark.parametrize("key", list(S.APPLY2_TABLE))
def test_apply2(key):
    c = S.case("apply2", key, S16())
    M, C = c.M, c.C
    assert_geometry(M, C)
    assert _C.lib().fedfr_bn_apply2_sliced_ok(M, C, c.P) == 1
    r = run_apply2(c)
    out = []
    try:
        cq = c.coef()
        for n in ("mean", "rstd", "scale", "shift", "rm", "rv"):
            S.check(r[n], cq[n], c.name + " " + n, out=out)
        sc, sh = r["scale"].cpu(), r["shift"].cpu()
        dq = c.second(sc, sh)
        for n in ("nmean", "nrstd", "nscale", "nshift", "nrm", "nrv"):
            S.check(r[n], dq[n], c.name + " " + n, out=out)
        S.check(r["out"], c.out(sc, sh), c.name + " out", out=out)
        o16 = r["out"].cpu()
        S.check(r["y2"], c.y2(o16, r["nscale"].cpu(), r["nshift"].cpu()), c.name + " y2", out=out)
        mq = c.measured(o16, sc, sh)
        for n in ("nmean", "nrstd"):
            S.check(r[n], mq[n], c.name + " derived vs measured " + n, out=out)
    finally:
        print(c.variant, out)
        note(out, "bn_apply2_sliced", c.variant)
    if M > 4096:
        S.drop("apply2", key, S16())


# ================================================================================================ bn_bwd_sliced
def _check_bwd(c, r, rows, out, tag=""):
    gq = c.grads_q(rows)
    for n in ("dbeta", "dgamma", "dalpha"):
        if r[n] is not None:
            S.check(r[n], gq[n], c.name + tag + " " + n, out=out)
    S.check(r["dx"], c.dx(rows), c.name + tag + " dx", out=out)
    if c.has_nx:
        S.check(r["npart"], c.next_rows_q(r["dx"].cpu()), c.name + tag + " next rows", out=out)
        assert float(r["npart"][:, 2].abs().max()) == 0.0


@pytest.mark.parametrize("key", list(S.BWD_TABLE))
def test_bwd(key):
    c = S.case("bwd", key, S16())
    M, C = c.M, c.C
    assert_geometry(M, C)
    assert _C.lib().fedfr_bn_sliced_ok(M, C, c.P, 1) == 1
    names = ["dx", "dgamma", "dbeta", "dalpha", "npart"]
    out = []
    if c.rows_in > 0:
        rows = c.rows.clone()
        if not c.alpha:
            rows[:, 2] = NAN                                   # two statistics are read: the third of every row must not be touched
        r = run_bwd(c, rows=rows)
        try:
            _check_bwd(c, r, c.rows, out)
        finally:
            print(c.variant, out)
            note(out, "bn_bwd_sliced", c.variant, "rows_in > 0")
    else:
        r = run_bwd(c)
        try:
            S.check(r["part"], c.reduce_rows_q(), c.name + " reduce rows", out=out)
            rows = r["part"].cpu()
            _check_bwd(c, r, rows, out)
        finally:
            print(c.variant, out)
            note(out, "bn_bwd_sliced", c.variant, "rows_in = 0")
        # the rows the first call left, given to a second call: the same dx, parameter gradients and next rows, bit for bit
        r2 = run_bwd(c, rows=rows)
        same(r, r2, names, c.name + " rows_in = 0 vs rows_in = G")
        out2 = []
        _check_bwd(c, r2, rows, out2, " (rows_in = G)")
        note(out2, "bn_bwd_sliced", c.variant, "rows_in > 0")
    if c.has_nx and M <= 4096:                                 # next rows requested or not: the same dx and parameter gradients
        same(r, run_bwd(c, rows=rows, nx=False), names[:4], c.name + " with / without next rows")
    if M > 4096:
        S.drop("bwd", key, S16())
    RAN["bwd"] += 1


# ================================================================================================ narrow and wide fan-in agree bit for bit
def _grid_rows(P, C, seed):
    """rows of exactly representable values (multiples of 1/8, |v| <= 8): their fp64 sum is exact in every order"""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-64, 65, (P, 3, C), generator=g).to(f32) / 8


@pytest.mark.parametrize("key,alpha", [("b31", False), ("b37", True)])
def test_bwd_wide_fan_in_equals_narrow(key, alpha):
    """100 rows on a 1/8 grid go through the narrow instantiation; the same rows followed by 100 rows of zeros, 200 > 128 / 130, through the wide one
    (FX = 2): the totals are the same numbers, so are dx and the parameter gradients"""
    c = S.case("bwd", key, S16())
    assert c.alpha == alpha and (c.M, c.C) == (264, 96)
    rows = _grid_rows(100, c.C, 5)
    wide = torch.cat([rows, torch.zeros_like(rows)])
    assert S.bwd_variant(100, alpha, False, False)[1] == 1 and S.bwd_variant(200, alpha, False, False)[1] == 2
    a, b = run_bwd(c, rows=rows), run_bwd(c, rows=wide)
    same(a, b, ["dx", "dgamma", "dbeta", "dalpha"], c.name + " narrow vs wide fan-in")
    out = []
    _check_bwd(c, b, wide, out, " (wide, grid rows)")
    print(S.bwd_variant(200, alpha, False, False)[2], out)
    note(out, "bn_bwd_sliced", S.bwd_variant(200, alpha, False, False)[2], "rows_in > 0")


def test_apply2_wide_fan_in_equals_narrow():
    """x1, x2 on a 1/8 grid: 100 partial rows that are exact sums (narrow, FL = 13), the same followed by 100 zero rows (wide, FL = 26)"""
    c = S.case("apply2", "a08", S16())
    M, C = c.M, c.C
    assert (M, C) == (264, 96)
    g = torch.Generator().manual_seed(7)
    x1, x2 = (torch.randint(-16, 17, (M, C), generator=g).to(f64) / 8 for _ in range(2))
    cols = [x1, x1 * x2, x1 * x1]
    rows = S.partial_rows(cols, S.row_bounds(M, 100))
    assert torch.equal(rows.to(f64).sum(0), torch.stack([t.sum(0) for t in cols]))             # exact: no order of summation changes the totals
    keep = (c.x, c.x2)
    c.x, c.x2 = S.r16(x1.to(f32), S16()), S.r16(x2.to(f32), S16())
    try:
        assert torch.equal(c.x.to(f64), x1) and torch.equal(c.x2.to(f64), x2)
        assert S.apply2_variant(M, C, 100).endswith("FL=13>") and S.apply2_variant(M, C, 200).endswith("FL=26>")
        a, b = run_apply2(c, rows=rows), run_apply2(c, rows=torch.cat([rows, torch.zeros_like(rows)]))
    finally:
        c.x, c.x2 = keep
    same(a, b, ["out", "y2", "scale", "shift", "mean", "rstd", "nscale", "nshift", "nmean", "nrstd", "rm", "rv", "nrm", "nrv"], "apply2 narrow vs wide fan-in")


# ================================================================================================ rejections
def _all_nan(o, names):
    return all(o[n] is None or bool(torch.isnan(o[n].float()).all()) for n in names)


class _Shape:
    """the smallest stand-in for a case that run_* accept: tensors of the right size, nothing computed"""

    def __init__(self, kind, M, C, P):
        s16 = S16()
        self.M, self.C, self.P = M, C, P
        self.G = max(1, S.sliced_geometry(M, max(C, 32) // 32 * 32, kind == "bwd")[0])
        z = lambda *s: torch.zeros(*s)     # noqa: E731
        self.x = self.x2 = self.dy = self.nx = torch.zeros(M, C, dtype=s16)
        self.rows = z(max(P, 1), 3 if kind != "apply" else 2, C)
        self.gamma = self.beta = self.rm = self.rv = self.nrm = self.nrv = self.xmean = self.xrstd = z(C) + 1
        self.p = self.np = self
        self.alpha_ = z(C)
        self.mean = self.rstd = self.sc = self.sh = z(C) + 1
        self.prelu = self.alpha = self.has_add = False
        self.has_nx, self.stats, self.add, self.null = True, True, None, ()


@pytest.mark.parametrize("kind,M,C,P", S.REJECT)
def test_rejected_shapes(kind, M, C, P):
    """an error, not a result: non-zero return code, the entry point named, every output still NaN"""
    c = _Shape(kind, M, C, P)
    lib = _C.lib()
    if kind == "apply":
        assert lib.fedfr_bn_sliced_ok(M, C, P, 0) == 0
        code, o = run_apply(c, P=P, rc=True)
        names, entry = ["scale", "shift", "mean", "rstd", "y", "stats"], "bn_apply_sliced"
    elif kind == "apply2":
        assert lib.fedfr_bn_apply2_sliced_ok(M, C, P) == 0
        code, o = run_apply2(c, P=P, rc=True)
        names, entry = ["scale", "shift", "mean", "rstd", "nscale", "nshift", "nmean", "nrstd", "out", "y2"], "bn_apply2_sliced"
    else:
        assert lib.fedfr_bn_sliced_ok(M, C, P or c.G, 1) == 0
        code, o = run_bwd(c, rows=c.rows if P else None, rc=True)
        names, entry = ["dx", "dgamma", "dbeta", "npart"] + ([] if P else ["part"]), "bn_bwd_sliced"
    assert code != 0 and entry in _C.last_error(), (code, _C.last_error())
    assert _all_nan(o, names)


def test_rejected_aliasing_rows():
    """output rows that overlap the input rows: the workgroups of one launch read and write them in no order"""
    c = S.case("apply", "f00", S16())
    rows = torch.cat([c.rows, torch.zeros(c.G, 2, c.C)])       # room for the G output rows in the same buffer
    part = d(rows)
    M, C = c.M, c.C
    k = [d(t) for t in (c.gamma, c.beta, c.x, c.p.alpha, c.x2)]
    o = dict(scale=nan(C), shift=nan(C), mean=nan(C), rstd=nan(C), y=nan(M, C, dtype=S16()))
    code = _C.lib().fedfr_bn_apply_sliced(part.data_ptr(), c.P, float(M), k[0].data_ptr(), k[1].data_ptr(), None, None, S.MOM, S.EPSF, o["scale"].data_ptr(),
                                          o["shift"].data_ptr(), o["mean"].data_ptr(), o["rstd"].data_ptr(), k[2].data_ptr(), k[3].data_ptr(),
                                          k[4].data_ptr(), o["y"].data_ptr(), M, C, part.data_ptr() + 4 * 2 * C * (c.P - 1), _C.stream())
    torch.cuda.synchronize()
    assert code != 0 and "bn_apply_sliced" in _C.last_error() and _all_nan(o, list(o)) and torch.equal(part.cpu(), rows)
    b = S.case("bwd", "b15", S16())                             # variant 7 with external rows
    assert b.has_nx and b.rows_in > 0
    buf = d(torch.cat([b.rows, torch.zeros(b.G, 3, b.C)]))      # the first output row would be the last input row
    before = buf.clone()
    k = dict(dy=d(b.dy), x=d(b.x), mean=d(b.p.mean), rstd=d(b.p.rstd), gamma=d(b.p.gamma), alpha=d(b.p.alpha), sc=d(b.p.sc), sh=d(b.p.sh), add=d(b.add),
             nx=d(b.nx), nmean=d(b.np.mean), nrstd=d(b.np.rstd))
    o = dict(dx=nan(b.M, b.C, dtype=S16()), dgamma=nan(b.C), dbeta=nan(b.C), dalpha=nan(b.C))
    g = lambda n: k[n].data_ptr()     # noqa: E731
    code = _C.lib().fedfr_bn_bwd_sliced(g("dy"), g("x"), g("mean"), g("rstd"), g("gamma"), g("alpha"), g("sc"), g("sh"), b.M, b.C, buf.data_ptr(), b.rows_in,
                                        o["dgamma"].data_ptr(), o["dbeta"].data_ptr(), o["dalpha"].data_ptr(), g("add"), o["dx"].data_ptr(), g("nx"),
                                        g("nmean"), g("nrstd"), buf.data_ptr() + 4 * 3 * b.C * (b.rows_in - 1), _C.stream())
    torch.cuda.synchronize()
    assert code != 0 and "bn_bwd" in _C.last_error() and "sliced" in _C.last_error(), _C.last_error()
    assert _all_nan(o, list(o)) and torch.equal(buf, before)


# ================================================================================================ the margins
def test_zz_margins():
    """the worst error / tolerance per entry point and instantiation, for the log; the instantiations no older test launches are among them"""
    for k in sorted(MARGINS):
        print("%-18s %-46s %-12s %-7s %.3f" % (k + (MARGINS[k],)))
    if RAN["bwd"] < len(S.BWD_TABLE):                     # a selection of this file's tests was run: the table below is not complete
        return
    seen = {(k[1], k[2]) for k in MARGINS}
    v = lambda n, fx: S.bwd_variant(200 if fx == 2 else 5, bool(n & 4), bool(n & 2), bool(n & 1))[2]     # noqa: E731
    for need in ((v(5, 1), "rows_in = 0"), (v(6, 1), "rows_in = 0"), (v(5, 1), "rows_in > 0"), (v(6, 1), "rows_in > 0"), (v(0, 2), "rows_in > 0"),
                 (v(4, 2), "rows_in > 0")):
        assert need in seen, need
    assert all(m <= 1.0 for m in MARGINS.values())
