"""The per-step kernels one by one through the C ABI on raw pointers: momentum SGD (plain and loss-scaled), fedavg_axpy, the PartialFC
selection (top-k on both kernels, positives, remap, row gather / scatter and the whole chain), the head helpers (contrastive, colflag,
class_accumulate, the ROC histogram) and the input path (preprocess_u8, pad_input_nhwc) — against the restatements and float64 references
of tests/step_cases.py (which tests/test_step_cases_cpu.py proves admissible and sharp).  Before every call the outputs hold NaN (16-bit,
byte and integer buffers: a fill pattern) with a guard band behind every buffer; afterwards the guard is intact and every value that is
due is the exact bits, or a number within its tolerance.  Each toleranced figure is printed, as a fraction of its tolerance, before it is
asserted (pytest -s).  The storage type is the loaded library's (_C.storage_dtype()): the file runs unchanged on the fp16 and the bf16
build, and tests/test_bf16_build_gpu.py runs it on the latter."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import step_cases as S  # noqa: E402
import tail_cases as T  # noqa: E402
from fedfr_amd import _C  # noqa: E402

NAN = float("nan")
f32 = torch.float32
GUARD = 256
FILL16 = 0x5555                      # what 16-bit and byte outputs hold before a call (fp16 85.3, bf16 1.5e13: no value a test expects)
IFILL = -7                           # what integer outputs hold


def dev():
    return torch.device("cuda:0")


def S16():
    return _C.storage_dtype()


def D(t):
    if isinstance(t, np.ndarray):
        t = torch.from_numpy(np.array(t))
    return t.to(dev()).contiguous()


def galloc(n, dtype=f32, off=0):
    """(buffer, view of n elements from ``off``): NaN (fp32), the fill pattern (16-bit, bytes) or IFILL (integers), a guard band behind"""
    if dtype == f32:
        buf = torch.full((off + n + GUARD,), NAN, dtype=f32, device=dev())
    elif dtype == torch.uint8:
        buf = torch.full((off + n + GUARD,), 0x55, dtype=torch.uint8, device=dev())
    elif dtype in (torch.int64, torch.int32):
        buf = torch.full((off + n + GUARD,), IFILL, dtype=dtype, device=dev())
    else:
        buf = torch.full((off + n + GUARD,), FILL16, dtype=torch.int16, device=dev()).view(dtype)
    return buf, buf[off:off + n]


def untouched(t):
    if t.dtype == f32:
        return bool(torch.isnan(t).all())
    if t.dtype == torch.uint8:
        return bool((t == 0x55).all())
    if t.dtype in (torch.int64, torch.int32):
        return bool((t == IFILL).all())
    return bool((t.view(torch.int16) == FILL16).all())


def guard_ok(buf):
    return untouched(buf[-GUARD:])


def loaded(src, dtype=f32, off=0):
    """an in / out buffer holding ``src``, with the guard band behind it"""
    src = torch.from_numpy(np.array(src)) if isinstance(src, np.ndarray) else src
    buf, v = galloc(src.numel(), dtype, off)
    v.copy_(src.reshape(-1).to(dev()))
    return buf, v


def run(name, *args):
    _C.call(name, *args, _C.stream())
    torch.cuda.synchronize()


def rc_of(name, *args):
    rc = getattr(_C.lib(), name)(*args, _C.stream())
    torch.cuda.synchronize()
    return rc


def show(figs):
    for what, kind, worst in figs:
        print("%-90s %-5s %.3g of tol" % (what, kind, worst))


def npy(t):
    return t.detach().cpu().numpy()


# ------------------------------------------------------------------------------------------------ SGD
def _sgd(p, g, buf, shadow, n, hyper, first, scaled=None):
    lr, mu, wd = hyper
    sp = shadow.data_ptr() if shadow is not None else None
    if scaled is None:
        run("fedfr_sgd_step", p.data_ptr(), g.data_ptr(), buf.data_ptr(), sp, n, lr, mu, wd, first)
    else:
        gs, word = scaled
        run("fedfr_sgd_step_scaled", p.data_ptr(), g.data_ptr(), buf.data_ptr(), sp, n, lr, mu, wd, first, gs, word.data_ptr() if word is not None else None)


def _sgd_two_steps(n, hyper, with_shadow, what):
    """first = 1 on a NaN momentum buffer, then first = 0 with another gradient, on the same buffers: p, buf and the shadow bit for bit,
    the gradient buffer bit-unchanged"""
    p, g = S.sgd_inputs(n)
    g2 = S.sgd_second_grad(n)
    lr, mu, wd = hyper
    if hyper == S.SGD_HYPER:
        (p1, b1), (p2, b2) = S.sgd_two_steps(n)
    else:
        p1, b1, _, _ = S.sgd_ref(p, g, None, lr, mu, wd, 1)
        p2, b2, _, _ = S.sgd_ref(p1, g2, b1, lr, mu, wd, 0)
    (pb, pd), (gb, gd), (bb, bd) = loaded(p), loaded(g), galloc(n)
    sb, sd = galloc(n, S16()) if with_shadow else (None, None)
    for step, (gin, wp, wb) in enumerate(((g, p1, b1), (g2, p2, b2))):
        if step:
            gd.copy_(D(gin))
        _sgd(pd, gd, bd, sd, n, hyper, 1 - step)
        w = "%s step %d " % (what, step + 1)
        S.same32(npy(pd), wp, w + "p")
        S.same32(npy(bd), wb, w + "buf")
        S.same32(npy(gd), gin, w + "gradient (must be unchanged)")
        if with_shadow:
            T.same16(sd, S.shadow_ref(wp, S16()), w + "shadow")
            assert guard_ok(sb), w + "wrote behind the shadow"
        assert guard_ok(pb) and guard_ok(gb) and guard_ok(bb), w + "wrote behind a buffer"


@pytest.mark.parametrize("n", S.SGD_N)
def test_sgd_two_steps_bit_exact(n):
    for with_shadow in (1, 0):
        _sgd_two_steps(n, S.SGD_HYPER, with_shadow, "sgd[n=%d,shadow=%d]" % (n, with_shadow))


@pytest.mark.parametrize("hyper", [(0.61, 0.0, 0.37), (0.61, 0.9, 0.0), S.SGD_HYPER_PRODUCT], ids=["mu=0", "wd=0", "product"])
def test_sgd_hyper_parameter_cases(hyper):
    for n in (7, 4103):
        _sgd_two_steps(n, hyper, 1, "sgd[n=%d,%s]" % (n, hyper))


def test_sgd_shadow_is_the_cast_on_planted_subnormals_ties_and_overflow():
    """the float4 body (pack_bf2) and the scalar tail (f2bf) on parameters that round to 16-bit subnormals, exact ties and, fp16, past
    65504: the shadow is p'.to(storage dtype) bit for bit"""
    s16 = S16()
    for j in range(S.shadow_plant_calls(s16)):
        p, g, body, tail = S.shadow_plant_case(s16, j)
        n = len(p)
        want, wb, _, _ = S.sgd_ref(p, g, None, *S.SGD_HYPER, 1)
        (pb, pd), (gb, gd), (bb, bd), (sb, sd) = loaded(p), loaded(g), galloc(n), galloc(n, s16)
        _sgd(pd, gd, bd, sd, n, S.SGD_HYPER, 1)
        S.same32(npy(pd), want, "planted[%d] p" % j)
        S.same32(npy(bd), wb, "planted[%d] buf" % j)
        ws = S.shadow_ref(want, s16)
        T.same16(sd, ws, "planted[%d] shadow" % j)
        if s16 == torch.float16:
            assert bool(torch.isinf(sd[torch.from_numpy(body).to(dev())]).any())
        assert all(guard_ok(b) for b in (pb, gb, bb, sb))


def test_sgd_on_a_sub_buffer_touches_nothing_on_either_side():
    n, off = 1025, 8                                                   # 32 bytes into the fp32 allocations, 16 into the shadow
    p, g = S.sgd_inputs(n)
    (p1, b1), _ = S.sgd_two_steps(n)
    big = []
    for src in (p, g, None):
        t = torch.full((off + n + GUARD,), S.SENTINEL, dtype=f32, device=dev())
        if src is not None:
            t[off:off + n] = D(src)
        big.append(t)
    sh = torch.full((off + n + GUARD,), FILL16, dtype=torch.int16, device=dev()).view(S16())
    pd, gd, bd = (t[off:off + n] for t in big)
    assert all(v.data_ptr() % 16 == 0 for v in (pd, gd, bd, sh[off:]))
    _sgd(pd, gd, bd, sh[off:off + n], n, S.SGD_HYPER, 1)
    S.same32(npy(pd), p1, "sub-buffer p")
    S.same32(npy(bd), b1, "sub-buffer buf")
    S.same32(npy(gd), g, "sub-buffer gradient")
    T.same16(sh[off:off + n], S.shadow_ref(p1, S16()), "sub-buffer shadow")
    for t in big:
        assert bool((t[:off] == S.SENTINEL).all()) and bool((t[off + n:] == S.SENTINEL).all())
    assert bool((sh[:off].view(torch.int16) == FILL16).all()) and bool((sh[off + n:].view(torch.int16) == FILL16).all())


def _word(v):
    buf, w = galloc(1, torch.int32)
    w.fill_(v)
    return buf, w


@pytest.mark.parametrize("n", [1, 5, 1025, 4103])
def test_sgd_scaled_clean_gradient_is_the_plain_step(n):
    """grad_scale = 2^-8 on a gradient buffer holding g * 2^8: identical bits to the plain restatement on two steps, the gradient buffer
    reads g afterwards, the overflow word stays 0 — or stays 1 where it already held 1 — and a NULL word changes nothing"""
    p, g = S.sgd_inputs(n)
    (p1, b1), (p2, b2) = S.sgd_two_steps(n)
    gs = S.SGD_SCALE
    for preset, with_word in ((0, True), (1, True), (0, False)):
        (pb, pd), (gb, gd), (bb, bd), (sb, sd) = loaded(p), loaded((g / np.float32(gs)).astype(np.float32)), galloc(n), galloc(n, S16())
        wbuf, word = _word(preset)
        what = "sgd_scaled[n=%d,word=%d,%s] " % (n, preset, "word" if with_word else "NULL")
        for step, (gin, wp, wb) in enumerate(((g, p1, b1), (S.sgd_second_grad(n), p2, b2))):
            if step:
                gd.copy_(D((gin / np.float32(gs)).astype(np.float32)))
            _sgd(pd, gd, bd, sd, n, S.SGD_HYPER, 1 - step, (gs, word if with_word else None))
            S.same32(npy(pd), wp, what + "p")
            S.same32(npy(bd), wb, what + "buf")
            S.same32(npy(gd), gin, what + "unscaled gradient")
            T.same16(sd, S.shadow_ref(wp, S16()), what + "shadow")
            assert int(word[0]) == preset, what + "overflow word"
        assert all(guard_ok(b) for b in (pb, gb, bb, sb, wbuf))


@pytest.mark.parametrize("first", [1, 0])
@pytest.mark.parametrize("n", [1, 2, 3, 5, 7, 1025, 4103, S.SGD_WRAP_N])
def test_sgd_scaled_skips_non_finite_elements(n, first):
    """inf, -inf and NaN planted at element 0, in the body, in the tail, at n - 1 and (wrap size) in the second grid-stride round: those
    elements keep p and buf (0 on the first step), their shadow is the rounding of the unchanged p, the word is 1, every other element
    is what the clean step gives"""
    p, g = S.sgd_inputs(n)
    (p1, b1), (p2, b2) = S.sgd_two_steps(n)
    gs = S.SGD_SCALE
    pos = S.sgd_bad_positions(n)
    p0, b0, gin, clean_p, clean_b = (p, None, g, p1, b1) if first else (p1, b1, S.sgd_second_grad(n), p2, b2)
    gin = (gin / np.float32(gs)).astype(np.float32)
    gin[pos] = S.sgd_bad_values(len(pos))
    wp, wb, wg, wovf = S.sgd_ref(p0, gin, b0, *S.SGD_HYPER, first, gs=gs)
    assert wovf == 1
    (pb, pd), (gb, gd), (sb, sd) = loaded(p0), loaded(gin), galloc(n, S16())
    bb, bd = galloc(n) if first else loaded(b0)
    wbuf, word = _word(0)
    _sgd(pd, gd, bd, sd, n, S.SGD_HYPER, first, (gs, word))
    what = "sgd_scaled[n=%d,first=%d] " % (n, first)
    gp, gbuf = npy(pd), npy(bd)
    S.same32(gp, wp, what + "p")
    S.same32(gbuf, wb, what + "buf")
    S.same32(npy(gd), wg, what + "unscaled gradient", nan_ok=True)
    S.same32(gp[pos], p0[pos], what + "p of the skipped elements")
    S.same32(gbuf[pos], np.zeros(len(pos), np.float32) if first else b0[pos], what + "buf of the skipped elements")
    keep = np.ones(n, bool)
    keep[pos] = False
    S.same32(gp[keep], clean_p[keep], what + "p of the others")
    S.same32(gbuf[keep], clean_b[keep], what + "buf of the others")
    T.same16(sd, S.shadow_ref(wp, S16()), what + "shadow")
    assert int(word[0]) == 1, what + "overflow word"
    assert all(guard_ok(b) for b in (pb, gb, bb, sb, wbuf))
    if n == 1025:                                                       # the same with no word to set: same arithmetic, no fault
        (pb, pd), (gb, gd), (sb, sd) = loaded(p0), loaded(gin), galloc(n, S16())
        bb, bd = galloc(n) if first else loaded(b0)
        _sgd(pd, gd, bd, sd, n, S.SGD_HYPER, first, (gs, None))
        S.same32(npy(pd), wp, what + "p, NULL word")
        S.same32(npy(bd), wb, what + "buf, NULL word")


def test_sgd_argument_errors_write_nothing():
    n = 64
    bufs = [torch.full((n + 8,), 0.5, dtype=f32, device=dev()) for _ in range(3)]
    sh = torch.full((n + 8,), FILL16, dtype=torch.int16, device=dev())
    for bad in range(3):
        ptrs = [(b[1:] if i == bad else b).data_ptr() for i, b in enumerate(bufs)]
        for name, extra in (("fedfr_sgd_step", ()), ("fedfr_sgd_step_scaled", (0.5, None))):
            rc = rc_of(name, *ptrs, sh.data_ptr(), n, 0.1, 0.9, 0.0, 1, *extra)
            assert rc < 0 and "sgd" in _C.last_error(), (name, rc, _C.last_error())
    for name, extra in (("fedfr_sgd_step", ()), ("fedfr_sgd_step_scaled", (0.5, None))):
        rc = rc_of(name, *[b.data_ptr() for b in bufs], sh.data_ptr(), 0, 0.1, 0.9, 0.0, 1, *extra)
        assert rc < 0 and "sgd" in _C.last_error()
    assert all(bool((b == 0.5).all()) for b in bufs) and bool((sh == FILL16).all())


# ------------------------------------------------------------------------------------------------ fedavg_axpy
@pytest.mark.parametrize("n", S.AXPY_N)
def test_fedavg_axpy_bit_exact(n):
    """accumulate = 0 onto a NaN-filled destination, then accumulate = 1: fl(d + fl(w s)) bit for bit"""
    s0, s1 = S.uniform((n,), 300 + n % 997).numpy(), S.uniform((n,), 301 + n % 997).numpy()
    dbuf, dst = galloc(n)
    sd0, sd1 = D(s0), D(s1)
    run("fedfr_fedavg_axpy", dst.data_ptr(), sd0.data_ptr(), S.AXPY_W[0], n, 0)
    want = S.axpy_ref(None, s0, S.AXPY_W[0], False)
    S.same32(npy(dst), want, "axpy[n=%d] overwrite" % n)
    run("fedfr_fedavg_axpy", dst.data_ptr(), sd1.data_ptr(), S.AXPY_W[1], n, 1)
    S.same32(npy(dst), S.axpy_ref(want, s1, S.AXPY_W[1], True), "axpy[n=%d] accumulate" % n)
    assert guard_ok(dbuf) and np.array_equal(npy(sd0), s0) and np.array_equal(npy(sd1), s1)


# ------------------------------------------------------------------------------------------------ PartialFC selection
class _Perm:
    """the values on the device, 16-byte aligned or — as a view one float into a larger buffer — not: the view forces the narrow kernel"""

    def __init__(self, v, aligned):
        n = len(v)
        self.buf = torch.full((n + 4 + GUARD,), NAN, dtype=f32, device=dev())
        self.view = self.buf[0:n] if aligned else self.buf[1:n + 1]
        assert (self.view.data_ptr() % 16 == 0) == bool(aligned)
        self.view.copy_(D(v))
        self.v, self.n = v, n

    def topk(self, k, what, with_npos=True):
        ibuf, index = galloc(k, torch.int64)
        nbuf, npos = galloc(1, torch.int32)
        run("fedfr_pfc_topk", self.view.data_ptr(), self.n, k, index.data_ptr(), npos.data_ptr() if with_npos else None)
        S.same_int(npy(index), S.topk_ref(self.v, k), what)
        assert guard_ok(ibuf) and guard_ok(nbuf), what + ": wrote behind an output"
        if with_npos:
            assert int(npos[0]) == S.topk_npos(self.v), what + ": count of 2.0 values"
        else:
            assert untouched(npos), what + ": wrote through a NULL count"
        assert np.array_equal(npy(self.view), self.v), what + ": the values changed"


def _topk_all(v, ks, what):
    for aligned in (1, 0):
        pm = _Perm(v, aligned)
        for k in ks:
            pm.topk(k, "%s k=%d %s" % (what, k, "wide" if S.topk_is_wide(aligned, len(v)) else "narrow"))


@pytest.mark.parametrize("n", S.TOPK_N)
def test_pfc_topk_sizes_on_both_kernels(n):
    _topk_all(S.TOPK_PATTERNS["rand"](n), S.topk_ks(n), "topk[rand,n=%d]" % n)


@pytest.mark.parametrize("name", [k for k in S.TOPK_PATTERNS if k != "rand"])
def test_pfc_topk_value_patterns(name):
    """tied levels, all equal, all zero (the bin == 0 fallback), more marks than k, and values only the third / only the second radix
    pass can separate, on both sides of the dispatch boundary"""
    for n in S.TOPK_PATTERN_N:
        _topk_all(S.TOPK_PATTERNS[name](n), S.topk_ks(n), "topk[%s,n=%d]" % (name, n))


@pytest.mark.parametrize("n,edge", S.TOPK_TIE_CASES)
def test_pfc_topk_tie_cut_at_a_chunk_boundary(n, edge):
    v, ks = S.topk_tie_case(n, edge)
    _topk_all(v, ks, "topk[tie at %d,n=%d]" % (edge, n))


def test_pfc_topk_without_a_count():
    v = S.TOPK_PATTERNS["marks"](S.TOPK_WIDE_MIN_N)
    for aligned in (1, 0):
        _Perm(v, aligned).topk(len(v) // 3, "topk[npos NULL,aligned=%d]" % aligned, with_npos=False)


@pytest.mark.parametrize("n", S.POSITIVE_N)
def test_pfc_positive(n):
    for name, perm in S.positive_cases(n).items():
        want = np.flatnonzero(perm == np.float32(2.0))
        ibuf, index = galloc(n, torch.int64)
        cbuf, count = galloc(1, torch.int32)
        pd = D(perm)
        run("fedfr_pfc_positive", pd.data_ptr(), n, index.data_ptr(), count.data_ptr())
        k = int(count[0])
        assert k == len(want), "positive[n=%d,%s]: count %d != %d" % (n, name, k, len(want))
        S.same_int(npy(index[:k]), want, "positive[n=%d,%s]" % (n, name))
        assert untouched(index[k:]) and guard_ok(ibuf) and guard_ok(cbuf)


@pytest.mark.parametrize("n", S.REMAP_N)
def test_pfc_remap(n):
    for k in S.REMAP_K:
        lab, index = S.remap_inputs(n, k)
        lbuf, ld = loaded(lab, torch.int64)
        idx = D(index)
        run("fedfr_pfc_remap", ld.data_ptr(), n, idx.data_ptr(), k)
        S.same_int(npy(ld), S.remap_ref(lab, index), "remap[n=%d,k=%d]" % (n, k))
        assert guard_ok(lbuf) and np.array_equal(npy(idx), index)


@pytest.mark.parametrize("k", S.ROWS_K)
def test_rows_gather_and_scatter(k):
    """rows of D floats; negative, == table_rows and 10^9 indices are skipped: in gather those destination rows keep their NaN, in scatter
    no table row changes.  Three valid index entries sit behind the k that count: a launch that ran one row too far would copy it"""
    R = S.ROWS_TABLE
    full = np.concatenate([S.rows_index(k), np.zeros(3, np.int64)])
    idx = D(full)
    for Dm in S.ROWS_D:
        table, src = S.uniform((R, Dm), 500 + Dm).numpy(), S.uniform((len(full), Dm), 501 + Dm).numpy()
        what = "rows[k=%d,D=%d] " % (k, Dm)
        tbuf, td = loaded(table)
        dbuf, dst = galloc(len(full) * Dm)
        run("fedfr_rows_gather", dst.data_ptr(), td.data_ptr(), idx.data_ptr(), k, Dm, R)
        S.same32(npy(dst).reshape(len(full), Dm), S.rows_gather_ref(table, full, k), what + "gather", nan_ok=True)
        S.same32(npy(td).reshape(R, Dm), table, what + "gather changed the table")
        assert guard_ok(dbuf) and guard_ok(tbuf)
        sd = D(src)
        run("fedfr_rows_scatter", td.data_ptr(), sd.data_ptr(), idx.data_ptr(), k, Dm, R)
        S.same32(npy(td).reshape(R, Dm), S.rows_scatter_ref(table, src, full, k), what + "scatter")
        assert guard_ok(tbuf) and np.array_equal(npy(sd), src) and np.array_equal(npy(idx), full)


def test_rows_argument_errors_write_nothing():
    tbuf, td = loaded(S.uniform((4, 8), 1).numpy())
    dbuf, dst = galloc(32)
    idx = D(np.zeros(4, np.int64))
    for name in ("fedfr_rows_gather", "fedfr_rows_scatter"):
        a, b = (dst, td) if name.endswith("gather") else (td, dst)
        assert rc_of(name, a.data_ptr(), b.data_ptr(), idx.data_ptr(), 2, 6, 4) < 0 and "rows" in _C.last_error()
        assert rc_of(name, a.data_ptr(), b.data_ptr(), idx.data_ptr(), 0, 8, 4) < 0 and "rows" in _C.last_error()
    assert untouched(dst) and guard_ok(tbuf)


@pytest.mark.parametrize("num_local,num_sample,batch,pos_win", S.CHAIN_CASES)
def test_partial_fc_sampling_chain(num_local, num_sample, batch, pos_win):
    """rand -> localize -> topk (-> positive) -> remap -> gather -> edit -> scatter, as partial_fc.py issues them, against the numpy
    restatement of the same steps: on the wide and on the narrow top-k kernel, and with more positives than samples"""
    start, seed, step, Dm = 1000, 12345, 3, 8
    lab = S.chain_labels(num_local, batch, start)
    w, m = S.uniform((num_local, Dm), 600).numpy(), S.uniform((num_local, Dm), 601).numpy()
    ref = S.chain_ref(num_local, num_sample, lab, start, seed, step, w, m)
    assert (ref["npos"] > num_sample) == pos_win
    pbuf, perm = galloc(num_local)
    lbuf, ld = loaded(lab, torch.int64)
    (wbuf, wd), (mbuf, md) = loaded(w), loaded(m)
    run("fedfr_pfc_rand", perm.data_ptr(), num_local, seed, step)
    run("fedfr_pfc_localize", ld.data_ptr(), batch, start, num_local, perm.data_ptr())
    S.same32(npy(perm), ref["perm"], "chain perm")
    ibuf, index = galloc(num_sample, torch.int64)
    nbuf, npos = galloc(1, torch.int32)
    run("fedfr_pfc_topk", perm.data_ptr(), num_local, num_sample, index.data_ptr(), npos.data_ptr())
    assert int(npos[0]) == ref["npos"] and guard_ok(ibuf)
    if int(npos[0]) > num_sample:
        ibuf, index = galloc(int(npos[0]), torch.int64)
        run("fedfr_pfc_positive", perm.data_ptr(), num_local, index.data_ptr(), npos.data_ptr())
        assert int(npos[0]) == ref["npos"]
    k = index.numel()
    S.same_int(npy(index), ref["index"], "chain index")
    run("fedfr_pfc_remap", ld.data_ptr(), batch, index.data_ptr(), k)
    S.same_int(npy(ld), ref["label"], "chain labels")
    (swb, sw), (smb, sm) = galloc(k * Dm), galloc(k * Dm)
    run("fedfr_rows_gather", sw.data_ptr(), wd.data_ptr(), index.data_ptr(), k, Dm, num_local)
    run("fedfr_rows_gather", sm.data_ptr(), md.data_ptr(), index.data_ptr(), k, Dm, num_local)
    S.same32(npy(sw).reshape(k, Dm), ref["sub_w"], "chain sub_weight")
    S.same32(npy(sm).reshape(k, Dm), ref["sub_m"], "chain sub_weight_mom")
    sw.neg_()
    sm.mul_(0.5)
    run("fedfr_rows_scatter", md.data_ptr(), sm.data_ptr(), index.data_ptr(), k, Dm, num_local)
    run("fedfr_rows_scatter", wd.data_ptr(), sw.data_ptr(), index.data_ptr(), k, Dm, num_local)
    S.same32(npy(wd).reshape(num_local, Dm), ref["weight"], "chain weight")
    S.same32(npy(md).reshape(num_local, Dm), ref["mom"], "chain weight_mom")
    assert all(guard_ok(b) for b in (pbuf, lbuf, wbuf, mbuf, ibuf, nbuf, swb, smb))


# ------------------------------------------------------------------------------------------------ head helpers
@pytest.mark.parametrize("B", S.CON_B)
def test_contrastive(B):
    """row_loss and dx against float64 + autograd per row, with the special rows (x == g, x == -g, g == l, x == 0, the vanishing
    exponential); dx == NULL gives the same row_loss bits and writes nothing"""
    figs = []
    try:
        for Dm in S.CON_D:
            x, g, l, cancel = S.con_inputs(B, Dm)
            xd, gd, ld = D(x), D(g), D(l)
            for temp in S.CON_T:
                ref = S.con_ref(x, g, l, temp, cancel)
                what = "contrastive[%d,%d,T=%g] " % (B, Dm, temp)
                (lb, loss), (db, dx) = galloc(B), galloc(B * Dm)
                run("fedfr_contrastive", xd.data_ptr(), gd.data_ptr(), ld.data_ptr(), B, Dm, temp, loss.data_ptr(), dx.data_ptr())
                S.con_check(loss, ref, "row_loss", what + "row_loss", out=figs)
                S.con_check(dx.view(B, Dm), ref, "dx", what + "dx", out=figs)
                assert guard_ok(lb) and guard_ok(db), what + "wrote behind an output"
                l2b, loss2 = galloc(B)
                run("fedfr_contrastive", xd.data_ptr(), gd.data_ptr(), ld.data_ptr(), B, Dm, temp, loss2.data_ptr(), None)
                S.same32(npy(loss2), npy(loss), what + "row_loss with dx == NULL")
                assert guard_ok(l2b)
            assert torch.equal(xd.cpu(), x) and torch.equal(gd.cpu(), g) and torch.equal(ld.cpu(), l)
    finally:
        worst = {}
        for what, kind, v in figs:
            key = what.split("] ")[1]
            if key not in worst or not v <= worst[key][2]:
                worst[key] = (what, kind, v)
        show(worst.values())


@pytest.mark.parametrize("M", S.CF_M)
def test_sgemm_colflag_exact(M):
    """small-integer operands: every score is exact, so the flags equal (alpha a b^T > thr).any(0) with NO exclusion band — at thresholds
    that ARE attained scores (strict >), and at negative ones, where a padded zero row would flag every column"""
    for N in S.CF_N:
        for K in S.CF_K:
            a, b = S.cf_operands(M, N, K)
            layouts = (("row-major", D(a), D(b), (K, 1, 1, K)), ("k-major", D(a.t().contiguous()), D(b.t().contiguous()), (1, M, N, 1)))
            for name, thr in S.cf_thresholds(a, b).items():
                want = S.cf_flags(a, b, thr).numpy()
                for lname, ad, bd, (sam, sak, sbk, sbn) in layouts:
                    fbuf, flags = galloc(N, torch.uint8)
                    flags.zero_()
                    run("fedfr_sgemm_colflag", ad.data_ptr(), bd.data_ptr(), M, N, K, sam, sak, sbk, sbn, S.CF_ALPHA, thr, flags.data_ptr())
                    S.same_int(npy(flags), want, "colflag[%d,%d,%d] thr=%s (%g) %s" % (M, N, K, name, thr, lname))
                    assert guard_ok(fbuf)


@pytest.mark.parametrize("B", S.CA_B)
def test_class_accumulate_is_the_stated_order(B):
    """bit-equal to the per-class, per-1024-row-slice sequential fp32 sum added to the running sums; labels -1, C and 10^12 ignored; classes
    with no row bit-unchanged; within TOL["fwd"] of float64 against |sums| + sum |terms|"""
    figs = []
    try:
        for Dm in S.CA_D:
            for Cn in S.CA_C:
                x, sums, counts = S.ca_inputs(B, Dm, Cn)
                xd = D(x)
                for li, lab in enumerate(S.ca_labels(B, Cn)):
                    (sb, sd), (cb, cd) = loaded(sums), loaded(counts)
                    ld = D(lab)
                    run("fedfr_class_accumulate", xd.data_ptr(), ld.data_ptr(), B, Dm, Cn, sd.data_ptr(), cd.data_ptr())
                    S.ca_check(npy(sd).reshape(Cn, Dm), npy(cd), x, lab, sums, counts, "class_accumulate[%d,%d,%d]#%d" % (B, Dm, Cn, li), out=figs)
                    assert guard_ok(sb) and guard_ok(cb) and np.array_equal(npy(ld), lab)
    finally:
        show([max(figs, key=lambda f: f[2] if f[2] == f[2] else np.inf)] if figs else [])


@pytest.mark.parametrize("Dm", S.ROC_D)
def test_roc_histogram_on_bin_edges_and_clamps(Dm):
    """features on a 1/8 grid (exact dots, many exactly on bin edges, |dot| > 1 into the clamped bins 0 and 2000), D not a multiple of
    the K step, T at 1, 64, 65 and N: the float64 restatement of roc_slot, bin for bin"""
    f, lab = S.roc_inputs(Dm)
    fd, ld = D(f), D(lab)
    for Tn in S.ROC_T:
        hist = torch.zeros(S.ROC_NBIN + GUARD, dtype=torch.int64, device=dev())
        hist[S.ROC_NBIN:] = IFILL
        run("fedfr_roc_histogram", fd.data_ptr(), ld.data_ptr(), S.ROC_N, Dm, Tn, hist.data_ptr())
        got = npy(hist[:S.ROC_NBIN]).astype(np.uint64)
        assert int(got.sum()) == Tn * (Tn - 1) // 2 + Tn * (S.ROC_N - Tn)
        S.same_int(got, S.roc_ref(f, lab, Tn), "roc[D=%d,T=%d]" % (Dm, Tn))
        assert guard_ok(hist)


# ------------------------------------------------------------------------------------------------ input path
def _preprocess(B, H, W, kind):
    u8 = S.pre_input(B, H, W)
    flip = S.pre_flip(B, kind)
    ud = D(u8)
    fdv = D(flip) if flip is not None else None
    obuf, out = galloc(B * 3 * H * W)
    run("fedfr_preprocess_u8", ud.data_ptr(), fdv.data_ptr() if fdv is not None else None, out.data_ptr(), B, H, W)
    S.same32(npy(out).reshape(B, 3, H, W), S.pre_ref(u8, flip).numpy(), "preprocess_u8[%d,%d,%d,%s]" % (B, H, W, kind))
    assert guard_ok(obuf) and np.array_equal(npy(ud), u8)


@pytest.mark.parametrize("B,H,W", S.PRE_SHAPES)
def test_preprocess_u8_bit_exact(B, H, W):
    for kind in S.PRE_FLIPS:
        _preprocess(B, H, W, kind)


def test_preprocess_u8_beyond_the_grid_cap():
    _preprocess(*S.PRE_WRAP, "mixed")


def _pad(B, Cn, HW, Cpad):
    s16 = S16()
    x = S.uniform((B, Cn, HW), 700 + Cn + HW)
    edge = torch.tensor([1 + 2.0 ** -11, 1 + 2.0 ** -8, 2.0 ** -25, -0.0, 65520.0, 1 + 3 * 2.0 ** -11])
    x.view(-1)[:min(x.numel(), len(edge))] = edge[:x.numel()]
    xd = D(x)
    obuf, out = galloc(B * HW * Cpad, s16)
    run("fedfr_pad_input_nhwc", xd.data_ptr(), out.data_ptr(), B, Cn, HW, Cpad)
    got = out.view(B, HW, Cpad).cpu()
    what = "pad_input_nhwc[%d,%d,%d,%d]" % (B, Cn, HW, Cpad)
    T.same16(got, S.pad_ref(x, Cpad, s16), what)
    assert bool((got[:, :, Cn:].contiguous().view(torch.int16) == 0).all()), what + ": pad channels are not +0"
    assert guard_ok(obuf) and torch.equal(xd.cpu().view(torch.int32), x.view(torch.int32))


@pytest.mark.parametrize("Cn,Cpad", S.PAD_CC)
def test_pad_input_nhwc(Cn, Cpad):
    for HW in S.PAD_HW:
        for B in (1, 3):
            _pad(B, Cn, HW, Cpad)


def test_pad_input_nhwc_beyond_the_grid_cap():
    _pad(*S.PAD_WRAP)


def test_pad_input_nhwc_argument_errors_write_nothing():
    x = D(S.uniform((1, 16, 4), 1))
    obuf, out = galloc(4 * 16, S16())
    assert rc_of("fedfr_pad_input_nhwc", x.data_ptr(), out.data_ptr(), 1, 3, 4, 12) < 0 and "pad_input_nhwc" in _C.last_error()
    assert rc_of("fedfr_pad_input_nhwc", x.data_ptr(), out.data_ptr(), 1, 16, 4, 8) < 0 and "pad_input_nhwc" in _C.last_error()
    assert untouched(obuf)
