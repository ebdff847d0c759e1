"""Direct float64 parity of the end of the backward pass, kernel by kernel through the C ABI: the stem conv forward at shapes with a ragged
last tile and a second trip of its tile loop, the stem weight gradient (plain and with the BatchNorm + PReLU backward fused in) with
several stages per workgroup, a ragged last stage and a short last workgroup, the row-slab BatchNorm backward chain with everything the
network passes to it (variants 2, 3, 6, 7, 8, add_up, a frozen BatchNorm, rows left by a producing pass, coef_only), and the three as the
unit the training step runs.  Inputs, float64 references and tolerances: tests/stem_cases.py (tests/test_stem_cases_cpu.py proves the
tolerances reachable by a correct fp32 kernel and tight enough to see one row, one mask, one pixel, one tap).  Geometry is asserted
from the library's own row / size queries: a retune of the slab sizes or the stage size fails here instead of skipping a path.

The fused stem weight gradient is held to equal bn_bwd_apply + the plain form BIT FOR BIT (test_stem_wgrad_plain_and_fused asserts
torch.equal at every shape), as ew.h / stem.hip state: both kernels call the same expression (bn_math.h: bn_bwd_dx), a dz + (A x0 + B), on the same operands, the
library is built with -ffp-contract=on (contraction within a statement only), and both round the result to the same 16 bits."""

import pytest
import torch

import stem_cases as K
from fedfr_amd import _C

pytestmark = pytest.mark.gpu
f32, f64 = K.f32, K.f64


def dev():
    return torch.device("cuda:0")


def S16():
    return _C.storage_dtype()


def d(t):
    return None if t is None else t.contiguous().to(dev())


def rowslab(dy, x, p, M, C, count, alpha=False, part=None, rows_in=0, coef_only=0, add=None, add_up=None, H=0, nx=None, npar=None, nalpha=False,
            npart_alias=False):
    """one fedfr_bn_bwd_rowslab call as net.hip's bn_bwd makes it: the forward's (sc, sh) always given"""
    dv = dev()
    k = dict(dy=d(dy), x=d(x), mean=d(p.mean), rstd=d(p.rstd), gamma=d(p.gamma), beta=d(p.beta), alpha=d(p.alpha) if alpha else None, sc=d(p.sc),
             sh=d(p.sh), add=d(add), add_up=d(add_up), nx=d(nx))
    P_red, P_app = _C.lib().fedfr_bn_bwd_rows(M, C), _C.lib().fedfr_bn_bwd_apply_rows(M, C)
    if part is None:
        part = torch.full((max(P_red, P_app), 3, C), float("nan"), device=dv)
    out = dict(part=part, coef=torch.full((3, C), float("nan"), device=dv), dx=torch.full((M, C), float("nan"), dtype=S16(), device=dv))
    for n in ("dg", "db", "da"):
        out[n] = torch.full((C,), float("nan"), device=dv)
    if nx is not None:
        out["npart"] = part if npart_alias else torch.full((P_app, 3, C), float("nan"), device=dv)
        k.update(nmean=d(npar.mean), nrstd=d(npar.rstd), nsc=d(npar.sc) if nalpha else None, nsh=d(npar.sh) if nalpha else None,
                 nalpha=d(npar.alpha) if nalpha else None)
    g = lambda n: _C.ptr(k.get(n))    # noqa: E731
    _C.call("fedfr_bn_bwd_rowslab", g("dy"), g("x"), g("mean"), g("rstd"), g("gamma"), g("beta"), g("alpha"), g("sc"), g("sh"), M, C, float(count),
            part.data_ptr(), rows_in, coef_only, out["coef"].data_ptr(), out["dg"].data_ptr(), out["db"].data_ptr(),
            out["da"].data_ptr() if alpha else None, g("add"), g("add_up"), H, out["dx"].data_ptr(), g("nx"), g("nmean"), g("nrstd"),
            _C.ptr(out.get("npart")), g("nsc"), g("nsh"), g("nalpha"), _C.stream())
    torch.cuda.synchronize()
    return out


def stem_wgrad(c, dz=None, fused=None):
    """fedfr_stem_wgrad on a 16-bit dz, or fedfr_stem_wgrad_fused on (dy_act, x0, coef, sc, sh, alpha): dw [64][27]"""
    dv = dev()
    nbytes = _C.lib().fedfr_stem_wgrad_ws_bytes(c.B, c.HW)
    assert nbytes == c.nblk * 2048 * 4, (nbytes, c.nblk)
    ws = torch.full((nbytes // 4,), float("nan"), device=dv)
    dw = torch.full((64, 27), float("nan"), device=dv)
    x = d(c.x)
    if fused is None:
        dzd = d(dz)
        _C.call("fedfr_stem_wgrad", x.data_ptr(), dzd.data_ptr(), dw.data_ptr(), ws.data_ptr(), c.B, c.HW, _C.stream())
    else:
        dy, x0, coef, p = fused
        keep = [d(dy), d(x0), d(coef), d(p.sc), d(p.sh), d(p.alpha)]
        _C.call("fedfr_stem_wgrad_fused", x.data_ptr(), *[t.data_ptr() for t in keep], dw.data_ptr(), ws.data_ptr(), c.B, c.HW, _C.stream())
    torch.cuda.synchronize()
    return dw


# ------------------------------------------------------------------------------------------------ a. stem forward
@pytest.mark.parametrize("B,HW", K.STEM_FWD_SHAPES)
def test_stem_forward(B, HW):
    """y per pixel row to u16 + 2^-20 of the row's maximum; every statistics row against the sums of the 64 STORED pixels it covers (the
    rows of a ragged tile count only real pixels).  (3, 37): M % 256 = 11, odd W; (33, 127): 2080 tiles on 2048 workgroups, M % 256 = 33."""
    c = K.StemFwdCase(B, HW, S16())
    M = c.M
    ntiles = -(-M // 256)                              # ew_stem_fwd: tiles of 256 pixels on min(ntiles, 2048) workgroups
    rows = _C.lib().fedfr_stem_stat_rows(B, HW)
    assert rows == ntiles * 4
    if (B, HW) == (3, 37):
        assert M % 256 != 0 and HW % 2 == 1
    if (B, HW) == (33, 127):
        assert ntiles > 2048 and M % 256 != 0
    y = torch.full((M, 64), float("nan"), dtype=S16(), device=dev())
    stats = torch.full((rows, 2, 64), float("nan"), device=dev())
    xd, wd = d(c.x), d(c.w_krsc)
    _C.call("fedfr_stem_fwd", xd.data_ptr(), wd.data_ptr(), y.data_ptr(), stats.data_ptr(), B, HW, _C.stream())
    torch.cuda.synchronize()
    out = []
    try:
        K.check(y, c.y_q(c.y()), c.name + " y", out=out)
        K.check(stats, c.stats_q(y.cpu()), c.name + " stats", out=out)
    finally:
        print(out)


# ------------------------------------------------------------------------------------------------ b + c. stem weight gradient
@pytest.mark.parametrize("B,HW", K.STEM_WGRAD_SHAPES)
def test_stem_wgrad_plain_and_fused(B, HW):
    """The stem's BatchNorm + PReLU backward through the row-slab chain (its sums, coef and the stored dz0 against float64), then the
    weight gradient of that dz0 by the plain kernel and by the fused kernel from (dy, x0, coef): each within
    (2^-17 + L 2^-24) sum |dz col| of the float64 gradient PER WEIGHT ELEMENT, and the two equal bit for bit."""
    c = K.StemWgradCase(B, HW, S16())
    M = c.M
    stages = c.ppb // 128                              # SW_PX = 128 pixels per stage, ppb from stem.hip's stem_px_per_block (the workspace query confirms nblk)
    if (B, HW) == (11, 112):
        assert stages == 2 and M % c.ppb == 0
    elif (B, HW) == (53, 50):
        assert stages == 2 and M - (c.nblk - 1) * c.ppb == 128 + 20
    else:
        assert stages == 1 and c.nblk == 1 and M < 128
    assert c.L == stages * 4 + c.nblk
    assert _C.lib().fedfr_bn_bwd_rows(M, 64) == -(-M // c.slab)
    out = []
    try:
        r = rowslab(c.dy, c.x0, c.p, M, 64, M, alpha=True)
        for got, q, what in zip((r["db"], r["dg"], r["da"]), c.sums_q(), ("dbeta", "dgamma", "dalpha")):
            K.check(got, q, c.name + " " + what, out=out)
        K.check(r["coef"], c.coef_q(), c.name + " coef", out=out)
        coef = r["coef"].cpu()
        K.check(r["dx"], c.dz0(coef), c.name + " dz0", out=out)
        dz0 = r["dx"].cpu()
        q = c.dw(dz0)
        plain = stem_wgrad(c, dz=dz0)
        K.check(plain, q, c.name + " dw plain", out=out)
        fused = stem_wgrad(c, fused=(c.dy, c.x0, coef, c.p))
        K.check(fused, q, c.name + " dw fused", out=out)
        assert torch.equal(plain, fused), "fused and two-kernel form differ: max %.3g" % float((plain - fused).abs().max())
    finally:
        print(out)


# ------------------------------------------------------------------------------------------------ d. row-slab apply variants
def _check_rowslab(c, r, out):
    for got, q, what in zip((r["db"], r["dg"], r["da"]), c.sums_q(), ("dbeta", "dgamma", "dalpha")[: 3 if c.alpha else 2]):
        K.check(got, q, c.name + " " + what, out=out)
    K.check(r["coef"], c.coef_q(), c.name + " coef", out=out)
    coef = r["coef"].cpu()
    K.check(r["dx"], c.dx(coef), c.name + " dx", out=out)
    if c.frozen:                                       # an infinite count: dx = a dz exactly (one fp32 product, rounded to 16 bits)
        assert float(coef[1:].abs().max()) == 0.0
        assert torch.equal(r["dx"].cpu(), K.r16(coef[0] * c.dy.to(f32), c.s16))
    if c.nx_mode:
        nq = c.next_sums_q(r["dx"].cpu())
        rows = r["npart"].double().sum(0).cpu()
        for i in range(3):
            K.check(rows[i], nq[i], c.name + " next rows %d" % i, out=out)
        if c.nx_mode == 1:
            assert float(r["npart"][:, 2].abs().max()) == 0.0


@pytest.mark.parametrize("s", ["small", "big", "c96", "c512", "add_up", "frozen"])
def test_bn_bwd_rowslab(s):
    """Variants 2, 3, 6, 7, 8 of bn_bwd_apply_kernel behind fedfr_bn_bwd_rowslab: dx element-wise, dgamma / dbeta / dalpha / coef, and the next
    BatchNorm's rows (summed over the workgroups) against float64 sums of the STORED dx.  After every variant 8 the rows feed a second call
    (rows_in > 0: no reduce pass) that is the next BatchNorm's own backward."""
    cases = K.bn_bwd_cases(S16())
    sel = {"small": cases[0:5], "big": cases[5:7], "c96": cases[7:9], "c512": cases[9:11], "add_up": cases[11:13], "frozen": cases[13:14]}[s]
    out = []
    try:
        for c in sel:
            M, C = c.M, c.C
            P = _C.lib().fedfr_bn_bwd_apply_rows(M, C)
            assert P == c.P_app and _C.lib().fedfr_bn_bwd_rows(M, C) == c.P_red       # slab = max(8 rpp, ceil(M / 768 | 512)) rounded up to rpp rows
            rpp, last = K.rows_per_pass(C), M - (P - 1) * c.slab_app
            if s == "small":
                assert (c.slab_app, P, last) == (256, 12, 184) and rpp == 32       # 184 = 5 x 32 + 24: two unrolled trips, a tail trip, a partial one
            if s == "big":
                assert c.slab_app == 352 > 8 * rpp and P > 1
            if s == "c96":
                assert rpp == 21 and rpp * (C // 8) < 256
            if s == "c512":
                assert rpp == 4 and C // 8 == 64
            r = rowslab(c.dy, c.x, c.p, M, C, c.count, alpha=c.alpha, add=c.add, add_up=c.add_up, H=c.up[1] if c.up else 0,
                        nx=c.nx if c.nx_mode else None, npar=c.np if c.nx_mode else None, nalpha=c.nx_mode == 2)
            _check_rowslab(c, r, out)
            if c.nx_mode == 2:
                # the rows as a producing pass's: the next BatchNorm (+PReLU) backward without its reduce pass
                dx1 = r["dx"].cpu()
                r2 = rowslab(dx1, c.nx, c.np, M, C, float(M), alpha=True, part=r["npart"], rows_in=P)
                nq = c.next_sums_q(dx1)
                for got, q, what in zip((r2["db"], r2["dg"], r2["da"]), nq, ("dbeta", "dgamma", "dalpha")):
                    K.check(got, K.Q(q.value, q.tol + K.U24 * q.value.abs()), c.name + " rows_in " + what, out=out)
                coef2 = r2["coef"].cpu()
                dzn = K.bn_terms(dx1, c.nx, c.np, True, f64)[0]
                K.check(r2["dx"], K.dx_q(*K.bn_dx(coef2, dzn, c.nx, f64), c.s16, unconditioned=True), c.name + " rows_in dx", out=out)
    finally:
        print(out)


# ------------------------------------------------------------------------------------------------ e. the chain as a unit
def test_first_block_to_stem_chain():
    """bn1 of the first block (variant 8 with add_up) leaves the rows [P][3][64]; fedfr_bn_bwd_rowslab(rows_in = P, coef_only) turns them into
    coef and the stem BatchNorm's parameter gradients; fedfr_stem_wgrad_fused consumes coef.  Against float64 autograd of prelu(bn(conv(x)))
    for the gradient the first step stored.  Bounds: the parameter gradients as the rows (+ 4 roundings of the fp32 statistics the kernels
    are given); the weight gradient (2^-17 + L 2^-24) sum |dz0 col| + 4 u16 sqrt(sum (dz0 col)^2) (four standard deviations of the
    independent 16-bit roundings of the operand dz0, which is never stored) + what the tolerance of coef leaves of dz0, through |col|."""
    ch = K.ChainCase(S16())
    c, s = ch.first, ch.sw
    M = c.M
    P = _C.lib().fedfr_bn_bwd_apply_rows(M, 64)
    assert P == c.P_app and P > 1
    out = []
    try:
        r = rowslab(c.dy, c.x, c.p, M, 64, c.count, add_up=c.add_up, H=c.up[1], nx=c.nx, npar=c.np, nalpha=True, npart_alias=True)
        _check_rowslab(c, r, out)
        dx1 = r["dx"].cpu()
        r2 = rowslab(dx1, c.nx, c.np, M, 64, float(M), alpha=True, part=r["npart"], rows_in=P, coef_only=1)
        assert bool(torch.isnan(r2["dx"].float()).all())                     # coef_only: no apply pass ran
        dw = stem_wgrad(s, fused=(dx1, s.x0, r2["coef"].cpu(), s.p))
        rw, rg, rb, ra = ch.reference(dx1)
        nq = c.next_sums_q(dx1)
        chain = K.colsum_chain(c.slab_app, 64)
        tS = [q.tol * (1 + 4.0 / chain) + K.U24 * q.value.abs() for q in nq]
        K.check(r2["db"], K.Q(rb, tS[0]), "chain dbeta", out=out)
        K.check(r2["dg"], K.Q(rg, tS[1]), "chain dgamma", out=out)
        K.check(r2["da"], K.Q(ra, tS[2]), "chain dalpha", out=out)
        coef = K.bn_coef(rb, rg, s.p, float(M))
        tc = K.bn_coef_tol(coef, tS[0], tS[1], s.p, float(M))
        K.check(r2["coef"], K.Q(coef, tc), "chain coef", out=out)
        dzn = K.bn_terms(dx1, s.x0, s.p, True, f64)[0]
        dz0, mag = K.bn_dx(coef, dzn, s.x0, f64)
        ddz = tc[0] * dzn.abs() + tc[1] * s.x0.to(f64).abs() + tc[2] + 2.0 ** -22 * mag
        q = s.dw(dz0, f64, extra_sigma=4.0)
        K.check(dw, K.Q(rw, q.tol + ddz.t() @ K.stem_taps(s.x).to(f64).abs()), "chain dw", out=out)
        assert float((q.value - rw).abs().max()) <= 1e-5 * float(rw.abs().max())          # the formula IS the autograd gradient (up to the fp32 statistics it is given)
    finally:
        print(out)
