"""Every branch of the convolution kernels, kernel by kernel through the C ABI, against a float64 reference: one table (conv_cases.table) of
entry point x geometry x option switches.  Every row asserts WHICH kernel served it — the profile slot that counted the launch, no other GEMM
slot counting any, and the partial / statistics row count where slot 15 alone does not tell the persistent 64-channel kernel from the LDS-DMA
ones — so that a retuned dispatch rule fails here instead of quietly moving a shape to the generic kernel.

Each row runs in two tiers (tests/conv_cases.py; tests/test_conv_cases_cpu.py proves the exact cases admissible and both instruments sharp):
  exact      dyadic inputs on which fp32 accumulation is exact in any order: y / dx / dz / dw must equal the float64 result BIT FOR BIT and the
             float64 sums of the partial rows must equal the reference sums exactly — all option variants of a shape are thereby bit-equal
             to each other as well;
  tolerance  ordinary inputs, element-wise bounds made of u16, 2^-24, a chain length and sum |terms|.
Outputs and partial buffers are pre-filled with NaN and a guard band behind each must stay NaN.  The float64 references are plain torch
matmuls on the GPU, computed once per (geometry, tier) and shared by the rows that need them.

To add a conv kernel or change a dispatch rule: add or edit rows of the table, not a new ad-hoc test."""
import contextlib
import ctypes as C
from collections import OrderedDict

import pytest
import torch

import conv_cases as K
from fedfr_amd import _C

pytestmark = pytest.mark.gpu
f32, f64 = K.f32, K.f64
CUS = torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256
TABLE = K.table(CUS)
GUARD = 4096
GEMM_SLOTS = range(18)


def dev():
    return torch.device("cuda:0")


def S16():
    return _C.storage_dtype()


def to16(t):
    """a float32 tensor of exactly representable values as a contiguous 16-bit device tensor"""
    h = t.to(S16())
    assert torch.equal(h.to(f32), t), "test input is not representable in the storage type"
    return h.contiguous().to(dev())


def galloc(shape, dtype):
    """(buffer, view): a NaN-filled output of `shape` with a NaN guard band behind it"""
    n = 1
    for v in shape:
        n *= v
    buf = torch.full((n + GUARD,), float("nan"), dtype=dtype, device=dev())
    return buf, buf[:n].view(*shape)


def guard_ok(buf, what):
    assert bool(torch.isnan(buf[-GUARD:].float()).all()), what + ": wrote behind its output"


def slot_counts():
    out = {}
    for s in GEMM_SLOTS:
        ms, n, fl = C.c_double(0), C.c_longlong(0), C.c_double(0)
        _C.call("fedfr_profile_read", s, C.byref(ms), C.byref(n), C.byref(fl))
        if n.value:
            out[s] = n.value
    return out


@contextlib.contextmanager
def served_by(row, launches=None):
    """option switches of the row on, profiling on; afterwards exactly the row's slot has counted the launches"""
    with contextlib.ExitStack() as st:
        for name, val in row.opts:
            st.enter_context(_C.option_scope(name, val))
        _C.call("fedfr_profile_enable", 1)
        try:
            yield
            torch.cuda.synchronize()
            counts = slot_counts()
        finally:
            _C.call("fedfr_profile_enable", 0)
    assert counts == {row.slot: row.launches if launches is None else launches}, "%s: launches per profile slot %s" % (row.id, counts)


# ------------------------------------------------------------------------------------------------ references, once per (geometry, tier)
_cache = OrderedDict()


def cached(key, make):
    if key in _cache:
        _cache.move_to_end(key)
        return _cache[key]
    while len(_cache) >= 6:
        _cache.popitem(last=False)
    _cache[key] = make()
    return _cache[key]


def fwd_ref(c):
    def make():
        x, w = c.fwd()
        r = K.conv_ref(x, w, c.s, f64, dev(), want=("y",))
        return dict(x=to16(x), w=to16(w), y=r["y"].reshape(c.M_out, c.Cout), S=r["Sy"].reshape(c.M_out, c.Cout), K=c.k * c.k * c.Cin)
    return cached(("fwd", c.name, c.s16), make)


def bwd_ref(c):
    def make():
        dy, w = c.bwd()
        r = K.conv_ref(torch.zeros(c.B, c.H, c.H, c.Cin), w, c.s, f64, dev(), dy=dy, want=("dx",))
        dx, S = r["dx"], r["Sdx"]
        if c.k == 1:                                        # the library's 1x1 dgrad leaves the compact result at the output resolution
            dx, S = dx[:, ::c.s, ::c.s].contiguous(), S[:, ::c.s, ::c.s].contiguous()
        wf = w.contiguous().to(dev())
        wd = torch.empty(c.Cin, c.k, c.k, c.Cout, dtype=S16(), device=dev())
        _C.call("fedfr_weight_shadows", wf.data_ptr(), None, wd.data_ptr(), c.Cout, c.k, c.Cin, _C.stream())
        torch.cuda.synchronize()
        return dict(dy=to16(dy), wd=wd, dx=dx.reshape(-1, c.Cin), S=S.reshape(-1, c.Cin), K=c.k * c.k * c.Cout)
    return cached(("bwd", c.name, c.s16), make)


def wg_ref(c, seed):
    def make():
        x, dy = c.wg(seed)
        r = K.conv_ref(x, torch.zeros(c.Cout, c.k, c.k, c.Cin), c.s, f64, dev(), dy=dy, want=("dw",))
        return dict(x=to16(x), dy=to16(dy), dw=r["dw"], S=r["Sdw"])
    return cached(("wg", c.name, c.s16, seed), make)


def vec(t):
    return t.contiguous().to(dev())


def same_bits(got, ref, what):
    g = got.double()
    assert torch.equal(g, ref.to(g.device).reshape(g.shape)), "%s: not bit-equal to float64 (%d elements differ, max |diff| %.3g)" % (
        what, int((g != ref.reshape(g.shape)).sum()), float((g - ref.reshape(g.shape)).abs().nan_to_num(nan=float("inf")).max()))


def check16(c, got, ref, S, Kc, what, out):
    if c.exact:
        same_bits(got, ref, what)
    else:
        K.check(got, c.out16_q(ref, S, Kc), what, out=out)


def check_rows(c, got_rows, val, q, what, out):
    """float64 sum of the partial rows against the reference column sums (q: the tolerance tier's bound, from conv_cases)"""
    g = got_rows.double().sum(0)
    if c.exact:
        same_bits(g, val, what)
    else:
        K.check(g, q, what, out=out)


# ------------------------------------------------------------------------------------------------ the ops
def run_fwd(row, c, out):
    B, H, Cin, Cout, k, s = row.shape
    r = fwd_ref(c)
    stats_on = row.op == "fwd_stats"
    ybuf, y = galloc((c.M_out, Cout), S16())
    nrows = _C.lib().fedfr_conv2d_stat_rows(B, c.Ho, Cout)
    assert nrows == K.nt_stat_rows(c.M_out, Cout)
    sbuf, stats = galloc((nrows, 2, Cout), f32)
    with served_by(row):
        _C.call("fedfr_conv2d_fwd", r["x"].data_ptr(), r["w"].data_ptr(), y.data_ptr(), stats.data_ptr() if stats_on else None, B, H, Cin, Cout, k, s, _C.stream())
    guard_ok(ybuf, row.id + " y")
    guard_ok(sbuf, row.id + " stats")
    check16(c, y, r["y"], r["S"], r["K"], row.id + " y", out)
    if not stats_on:
        assert bool(torch.isnan(stats).all())
        if row.rows is None:
            return
        # slot 15 does not tell the persistent kernel from the LDS-DMA ones and a plain launch leaves no rows: the same shape under the same switches
        # once more WITH statistics (conv_c64p_applies does not look at them) must leave the persistent kernel's row count
        with served_by(row, 1):
            _C.call("fedfr_conv2d_fwd", r["x"].data_ptr(), r["w"].data_ptr(), y.data_ptr(), stats.data_ptr(), B, H, Cin, Cout, k, s, _C.stream())
        # (the LDS-DMA kernels fill all nrows rows of the 128-pixel tiling: theirs would not end at the persistent kernel's two rows per workgroup)
        assert row.rows < nrows and float(stats[row.rows:].abs().sum()) == 0.0 and float(stats[row.rows - 2:row.rows].abs().sum()) > 0.0, row.id + ": not the persistent kernel's rows"
        val, mag = K.stats_of(y)
        check_rows(c, stats[:row.rows], val, K.stats_q(val, mag, c.M_out, row.rows), row.id + " stats", out)
        return
    live = row.rows
    assert 0 < live <= nrows and float(stats[live:].abs().sum()) == 0.0, row.id + ": rows beyond the live ones must be zeros"
    val, mag = K.stats_of(y)                                 # of the STORED y (== the reference in the exact tier)
    check_rows(c, stats[:live], val, K.stats_q(val, mag, c.M_out, live), row.id + " stats", out)


def run_fwd_moments(row, c, out):
    B, H, Cin, Cout, k, s = row.shape
    r = fwd_ref(c)
    M = c.M_out
    od = to16(K.moments_other(M, Cout, c.exact, c.s16))
    ybuf, y = galloc((M, Cout), S16())
    pbuf, part = galloc((M // 196 + 1, 3, Cout), f32)
    rows = C.c_int(-1)
    with served_by(row):
        _C.call("fedfr_conv2d_fwd_moments", r["x"].data_ptr(), r["w"].data_ptr(), y.data_ptr(), B, H, Cin, Cout, od.data_ptr(), part.data_ptr(), C.byref(rows), _C.stream())
    guard_ok(ybuf, row.id + " y")
    guard_ok(pbuf, row.id + " rows")
    assert rows.value == row.rows, (rows.value, row.rows)
    assert bool(torch.isnan(part[rows.value:]).all())
    check16(c, y, r["y"], r["S"], r["K"], row.id + " y", out)
    val, mag = K.moments(y, od)
    check_rows(c, part[:rows.value], val, K.moments_q(val, mag, M, rows.value), row.id + " moments", out)


def run_fwd_epi(row, c, out):
    B, H, Cin, Cout, k, s = row.shape
    r = fwd_ref(c)
    M = c.M_out
    ep = K.EpiPar(Cout, c.exact, c.s16, 50)
    addd = to16(K.epi_add(M, Cout, ep, c.exact, c.s16))
    sc, sh, al, sc2, sh2 = (vec(t) for t in (ep.scale, ep.shift, ep.alpha, ep.scale2, ep.shift2))
    y0_16 = {}                                               # the stored y of the launches without the identity path, per alpha
    with served_by(row):
        for combo in range(8):                               # (the launches without `add` come first)
            alpha, add, two = bool(combo & 1), bool(combo & 2), bool(combo & 4)
            what = "%s[alpha=%d,add=%d,y2=%d]" % (row.id, alpha, add, two)
            ybuf, y = galloc((M, Cout), S16())
            y2buf, y2 = galloc((M, Cout), S16())
            _C.call("fedfr_conv2d_fwd_epilogue", r["x"].data_ptr(), r["w"].data_ptr(), y.data_ptr(), sc.data_ptr(), sh.data_ptr(), al.data_ptr() if alpha else None,
                    addd.data_ptr() if add else None, y2.data_ptr() if two else None, sc2.data_ptr(), sh2.data_ptr(), B, H, Cin, Cout, _C.stream())
            torch.cuda.synchronize()
            guard_ok(ybuf, what + " y")
            guard_ok(y2buf, what + " y2")
            y0, ya, mag = K.epilogue_ref(r["y"], r["S"], ep, alpha, addd if add else None)
            ref = ya if add else y0
            if c.exact:
                same_bits(y, ref, what + " y")
            elif not add:
                K.check(y, K.epi_y_q(c.s16, y0, mag, r["K"]), what + " y", out=out)
                y0_16[alpha] = y
            else:   # the documented double rounding: round16(stored y0 + add)
                K.check(y, K.epi_yadd_q(c.s16, y0_16[alpha], addd), what + " y", out=out)
            if two:                                          # of the STORED y
                if c.exact:
                    same_bits(y2, y.double() * sc2.double() + sh2.double(), what + " y2")
                else:
                    K.check(y2, K.epi_y2_q(c.s16, y, sc2, sh2), what + " y2", out=out)
            else:
                assert bool(torch.isnan(y2.float()).all())


def dgrad_plain(c, r, shape):
    B, H, Cin, Cout, k, s = shape
    rowsd = r["dx"].shape[0]
    buf, dx = galloc((rowsd, Cin), S16())
    _C.call("fedfr_conv2d_dgrad", r["dy"].data_ptr(), r["wd"].data_ptr(), dx.data_ptr(), B, H, Cin, Cout, k, s, _C.stream())
    torch.cuda.synchronize()
    return buf, dx


def run_dgrad(row, c, out):
    r = bwd_ref(c)
    with served_by(row):
        buf, dx = dgrad_plain(c, r, row.shape)
    guard_ok(buf, row.id + " dx")
    check16(c, dx, r["dx"], r["S"], r["K"], row.id + " dx", out)


def run_dgrad_bnbwd(row, c, out):
    B, H, Cin, Cout, k, s = row.shape
    r = bwd_ref(c)
    M = c.M_in
    par = K.BnPar(Cin, c.exact, 60)
    bx, _ = K.bn_input(M, Cin, par, c.exact, c.s16, 61)
    bxd = to16(bx)
    mean, rstd, gamma, beta, alpha = (vec(t) for t in (par.mean, par.rstd, par.gamma, par.beta, par.alpha))
    buf, dx = galloc((M, Cin), S16())
    pbuf, part = galloc((max(K.cdiv(M, 128), M // 196 + 1), 3, Cin), f32)
    rows = C.c_int(-1)
    with served_by(row):
        _C.call("fedfr_conv2d_dgrad_bnbwd", r["dy"].data_ptr(), r["wd"].data_ptr(), dx.data_ptr(), B, H, Cin, Cout, k, s, bxd.data_ptr(), mean.data_ptr(),
                rstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(), alpha.data_ptr() if row.prelu else None, part.data_ptr(), C.byref(rows), _C.stream())
    guard_ok(buf, row.id + " dx")
    guard_ok(pbuf, row.id + " rows")
    assert rows.value == row.rows, (rows.value, row.rows)
    assert bool(torch.isnan(part[rows.value:]).all())
    check16(c, dx, r["dx"], r["S"], r["K"], row.id + " dx", out)
    if rows.value:
        val, mag = K.bnbwd_rows(dx, bxd, par, row.prelu)     # of the STORED dx
        check_rows(c, part[:rows.value], val, K.bnbwd_q(val, mag, M, rows.value), row.id + " rows", out)


def run_dgrad_papply(row, c, out):
    B, H, Cin, Cout, k, s = row.shape
    r = bwd_ref(c)
    M = c.M_in
    _, dx16 = dgrad_plain(c, r, row.shape)                   # the plain dgrad's stored result: what the epilogue applies the PReLU to
    with served_by(row):
        for with_bias in (True, False):
            what = row.id + ("[bias]" if with_bias else "[no bias]")
            ax, bias, alpha_t = K.papply_operands(M, Cin, c.exact, c.s16, with_bias)
            axd, al = to16(ax), vec(alpha_t)
            bd = None if bias is None else vec(bias)
            buf, dz = galloc((M, Cin), S16())
            pbuf, part = galloc((M // 196 + 1, 3, Cin), f32)
            rows = C.c_int(-1)
            _C.call("fedfr_conv2d_dgrad_papply", r["dy"].data_ptr(), r["wd"].data_ptr(), dz.data_ptr(), B, H, Cin, Cout, axd.data_ptr(), _C.ptr(bd), al.data_ptr(),
                    part.data_ptr(), C.byref(rows), _C.stream())
            torch.cuda.synchronize()
            guard_ok(buf, what + " dz")
            guard_ok(pbuf, what + " rows")
            assert rows.value == row.rows, (rows.value, row.rows)
            assert bool(torch.isnan(part[rows.value:]).all())
            dzr, val, mag = K.papply_ref(r["dx"] if c.exact else dx16, axd, bd, al)
            if c.exact:
                same_bits(dz, dzr, what + " dz")
            else:   # one fp32 product of the stored dgrad result, rounded once: the same bits as the two-kernel form
                neg = (axd.float() + (0 if bd is None else bd)) <= 0
                assert torch.equal(dz, torch.where(neg, dx16.float() * al, dx16.float()).to(S16())), what + ": dz is not round16(dx * prelu')"
            check_rows(c, part[:rows.value, 0:2], val, K.papply_q(val, mag, M, rows.value), what + " sums", out)
            assert torch.equal(part[:rows.value, 1], part[:rows.value, 2])
    check16(c, dx16, r["dx"], r["S"], r["K"], row.id + " dx", out)


def run_wgrad(row, c, out):
    B, H, Cin, Cout, k, s = row.shape
    r = wg_ref(c, 0)
    nbytes = _C.lib().fedfr_conv2d_wgrad_ws_bytes(B, H, Cin, Cout, k, s)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev())
    buf, dw = galloc((Cout, k, k, Cin), f32)
    slot, splits = K.wgrad_slot_splits(B, H, Cin, Cout, k, s, row.opt("wgrad9", 1), row.opt("tn_glds", 2), row.opt("tn_use_tr", 1))
    assert slot == row.slot
    with served_by(row):
        _C.call("fedfr_conv2d_wgrad", r["x"].data_ptr(), r["dy"].data_ptr(), dw.data_ptr(), ws.data_ptr(), nbytes, B, H, Cin, Cout, k, s, _C.stream())
    guard_ok(buf, row.id + " dw")
    if c.exact:
        same_bits(dw, r["dw"], row.id + " dw")
    else:
        K.check(dw, c.dw_q(r["dw"], r["S"], splits), row.id + " dw", out=out)


def run_wgrad_pair(row, c, out):
    B, H, Cin, Cout, k, s = row.shape
    ra, rb = wg_ref(c, 0), wg_ref(c, 100)
    nbytes = 2 * _C.lib().fedfr_conv2d_wgrad_ws_bytes(B, H, Cin, Cout, k, s)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev())
    bufa, dwa = galloc((Cout, k, k, Cin), f32)
    bufb, dwb = galloc((Cout, k, k, Cin), f32)
    Kp, NI, NJ = c.M_out, Cout, k * k * Cin
    splits = K.wgrad9p_pick_splits(Kp, NI, NJ, c.Ho) if row.opt("wgrad9p", 1) else K.wgrad9_pick_splits(Kp, NI, NJ, c.Ho)
    with served_by(row):
        _C.call("fedfr_conv2d_wgrad_pair", ra["x"].data_ptr(), ra["dy"].data_ptr(), dwa.data_ptr(), rb["x"].data_ptr(), rb["dy"].data_ptr(), dwb.data_ptr(),
                ws.data_ptr(), nbytes, B, H, Cin, Cout, k, s, _C.stream())
    for buf, dw, r, what in ((bufa, dwa, ra, " dw a"), (bufb, dwb, rb, " dw b")):
        guard_ok(buf, row.id + what)
        if c.exact:
            same_bits(dw, r["dw"], row.id + what)
        else:
            K.check(dw, c.dw_q(r["dw"], r["S"], splits), row.id + what, out=out)
    assert not torch.equal(ra["dw"], rb["dw"])               # (swapped layers would show)


RUN = {"fwd": run_fwd, "fwd_stats": run_fwd, "fwd_moments": run_fwd_moments, "fwd_epi": run_fwd_epi, "dgrad": run_dgrad, "dgrad_bnbwd": run_dgrad_bnbwd,
       "dgrad_papply": run_dgrad_papply, "wgrad": run_wgrad, "wgrad_pair": run_wgrad_pair}


@pytest.mark.parametrize("row", TABLE, ids=[r.id for r in TABLE])
def test_conv_branch(row):
    out = []
    try:
        for tier in row.tiers:
            RUN[row.op](row, K.ConvCase(*row.shape, tier, S16()), out)
    finally:
        print("RATIOS", row.id, out)


def test_unsupported_shapes_are_refused_on_the_host():
    """the two kernel-level entry points refuse what no kernel with their epilogue serves, with an error code and before any launch"""
    lib = _C.lib()
    one = torch.zeros(64, device=dev())
    p = one.data_ptr()
    rows = C.c_int(-1)
    _C.call("fedfr_profile_enable", 1)
    try:
        for B, H, Cin, Cout in ((124, 14, 256, 256), (125, 14, 64, 64), (2, 7, 512, 512), (15, 56, 64, 128)):
            assert lib.fedfr_conv2d_fwd_epilogue(p, p, p, p, p, None, None, None, None, None, B, H, Cin, Cout, _C.stream()) == -4, (B, H, Cin, Cout)
            assert b"conv2d_fwd_epilogue" in lib.fedfr_last_error_string()
        for B, H, Cin, Cout in ((124, 14, 256, 256), (16, 56, 64, 64), (125, 14, 64, 64)):
            assert lib.fedfr_conv2d_dgrad_papply(p, p, p, B, H, Cin, Cout, p, None, p, p, C.byref(rows), _C.stream()) == -4, (B, H, Cin, Cout)
            assert rows.value == 0 and b"conv2d_dgrad_papply" in lib.fedfr_last_error_string()
        torch.cuda.synchronize()
        assert slot_counts() == {}
    finally:
        _C.call("fedfr_profile_enable", 0)
