"""Every fp32 head kernel (csrc/head.hip) through the C ABI on raw pointers — so that ld, beta, bias and slab strides are reachable —
against the plain fp64 formulas of tests/head_cases.py, at the smallest shapes that select each code path.  Before every call the
outputs are NaN and any ld padding or slab gap holds a sentinel; after it the padding is intact and every value that is due is a number
within the head's tolerance of fp64 (per row: see head_cases).  The head is fp32 in the fp16- and the bf16-storage library alike:
nothing here depends on the storage type."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import head_cases as hc  # noqa: E402
from fedfr_amd import _C, ops  # noqa: E402

NAN = float("nan")
f32 = torch.float32


def dev():
    return torch.device("cuda:0")


def D(t):
    return t.to(dev()).contiguous()


def nans(*shape):
    return torch.full(shape, NAN, dtype=f32, device=dev())


def padded(t, pad):
    """[R, C + pad] on the device: t in the first C columns, the sentinel in the rest"""
    R, C = t.shape
    buf = torch.full((R, C + pad), hc.SENTINEL, dtype=f32, device=dev())
    buf[:, :C] = D(t)
    return buf


def pad_intact(buf, C):
    return bool((buf[:, C:] == hc.SENTINEL).all())


def run(name, *args):
    _C.call(name, *args, _C.stream())
    torch.cuda.synchronize()


def chk(got, q, what):
    """hc.check with the figure printed before it is asserted (pytest -s shows them)"""
    figs = []
    try:
        hc.check(got, q, what, out=figs)
    finally:
        for f in figs:
            print("%-100s %-5s %.3g" % f)


# ------------------------------------------------------------------------------------------------ normalise
@pytest.mark.parametrize("R,D_", hc.NORM_SHAPES)
def test_normalize_rows(R, D_):
    """R not a multiple of the four rows of a block, D around the wave width and the 512 threshold; an all-zero row (xn == 0,
    inv == 1 / eps exactly), a row of magnitude 1e-20 (the clamp, not inf), and each output left out in turn."""
    case = hc.normalize_case(R, D_)
    ref = case.ref()
    x = D(case.inputs["x"])
    xn, inv = nans(R, D_), nans(R)
    run("fedfr_normalize_rows", x.data_ptr(), xn.data_ptr(), inv.data_ptr(), R, D_, hc.EPS)
    chk(xn, ref["xn"], case.name + ":xn")
    chk(inv, ref["inv"], case.name + ":inv")
    if R >= 3:
        inv_eps = torch.tensor(1.0) / torch.tensor(hc.EPS, dtype=f32)
        assert bool((xn[1] == 0).all()) and float(inv[1]) == float(inv_eps)
        assert float(inv[2]) == float(inv_eps) and bool(torch.isfinite(xn[2]).all())
    inv2, xn2 = nans(R), nans(R, D_)
    run("fedfr_normalize_rows", x.data_ptr(), None, inv2.data_ptr(), R, D_, hc.EPS)
    run("fedfr_normalize_rows", x.data_ptr(), xn2.data_ptr(), None, R, D_, hc.EPS)
    assert torch.equal(inv2, inv) and torch.equal(xn2, xn)


@pytest.mark.parametrize("R,D_", hc.NORM_SHAPES)
def test_normalize_rows_bwd(R, D_):
    """both templates (D <= 512 keeps the row in registers with clamped loads; D > 512 walks it) at every combination of slab count,
    slab stride (tight and padded) and beta (0 = overwrite a NaN-filled dx, else accumulate onto a random one)"""
    for nslab in (1, 2, 5):
        for beta in (0.0, 1.0, -0.5):
            case = hc.normalize_bwd_case(R, D_, nslab, beta)
            ref = case.ref()["dx"]
            xn, inv = D(case.inputs["xn"]), D(case.inputs["inv"])
            for gap in (0, 13):
                stride = R * D_ + gap
                slabs = torch.full((nslab, stride), hc.SENTINEL, dtype=f32, device=dev())
                slabs[:, :R * D_] = D(case.inputs["slabs"]).reshape(nslab, R * D_)
                dx = D(case.inputs["dx_old"]).clone() if beta != 0 else nans(R, D_)
                run("fedfr_normalize_rows_bwd_slabs", xn.data_ptr(), inv.data_ptr(), slabs.data_ptr(), nslab, stride, dx.data_ptr(), R, D_, beta)
                chk(dx, ref, "%s:gap=%d" % (case.name, gap))
                assert pad_intact(slabs, R * D_)
            if nslab == 1:
                dx = D(case.inputs["dx_old"]).clone() if beta != 0 else nans(R, D_)
                g = D(case.inputs["slabs"][0])
                run("fedfr_normalize_rows_bwd", xn.data_ptr(), inv.data_ptr(), g.data_ptr(), dx.data_ptr(), R, D_, beta)
                chk(dx, ref, case.name + ":plain")


# ------------------------------------------------------------------------------------------------ margin + softmax + gradient
def _invalid_rows(case):
    lab, C = case.inputs["label"], case.inputs["cos"].shape[1]
    return D((lab < 0) | (lab >= C))


@pytest.mark.parametrize("cfg", hc.MARGIN_CFGS)
@pytest.mark.parametrize("C", hc.SOFTMAX_C)
def test_softmax_chain_vs_fp64(C, cfg):
    """fedfr_margin_rowmax -> fedfr_exp_rowsum -> fedfr_softmax_grad, every intermediate against fp64: ld == C and ld > C, labels -1, C,
    C - 1 and 0, CosFace / ArcFace at s = 30 and 64, an ArcFace target past th + m = pi"""
    s, m, arc = cfg
    for case in hc.softmax_cases(C, cfg):
        ref = case.ref()
        R = case.inputs["cos"].shape[0]
        lab = D(case.inputs["label"])
        bad = _invalid_rows(case)
        for pad in (0, 3):
            ldz = C + pad
            z = padded(case.inputs["cos"], pad)
            row_max, row_sum, dmul, z_t, prob_t, nll_t = (nans(R) for _ in range(6))
            what = "%s:ld=%d:" % (case.name, ldz)
            run("fedfr_margin_rowmax", z.data_ptr(), lab.data_ptr(), R, C, ldz, s, m, arc, row_max.data_ptr(), dmul.data_ptr(), z_t.data_ptr())
            chk(z[:, :C], ref["logits"], what + "logits")
            chk(row_max, ref["row_max"], what + "row_max")
            chk(dmul, ref["dmul"], what + "dmul")
            assert bool((dmul[bad] == s).all()) and pad_intact(z, C)
            run("fedfr_exp_rowsum", z.data_ptr(), R, C, ldz, row_max.data_ptr(), row_sum.data_ptr())
            chk(row_sum, ref["row_sum"], what + "row_sum")
            assert pad_intact(z, C) and not bool(torch.isnan(z[:, :C]).any())
            run("fedfr_softmax_grad", z.data_ptr(), lab.data_ptr(), R, C, ldz, row_sum.data_ptr(), dmul.data_ptr(), s, case.inputs["inv_batch"],
                prob_t.data_ptr(), row_max.data_ptr(), z_t.data_ptr(), nll_t.data_ptr())
            chk(prob_t, ref["prob_t"], what + "prob_t")
            chk(z[:, :C], ref["grad"], what + "grad")
            chk(nll_t, ref["nll_t"], what + "nll_t")
            assert bool((prob_t[bad] == 0).all()) and pad_intact(z, C)


@pytest.mark.parametrize("cfg", hc.MARGIN_CFGS)
@pytest.mark.parametrize("C", hc.SOFTMAX_C)
def test_softmax_ce_fused_vs_fp64(C, cfg):
    """fedfr_softmax_ce_fused against fp64 (not against the chain): C across 256 (one / two columns per thread), 1024 and 4096 (the
    columns-per-thread instantiations), ld > C, and the cosines arriving as 1 or 3 slabs with a gap between them"""
    s, m, arc = cfg
    for case in hc.softmax_cases(C, cfg):
        ref = case.ref()
        cos = case.inputs["cos"]
        R = cos.shape[0]
        lab = D(case.inputs["label"])
        bad = _invalid_rows(case)
        p0, p1 = cos * 0.5, cos * 0.25
        parts3 = [p0, p1, cos - (p0 + p1)]
        assert torch.equal((parts3[0] + parts3[1]) + parts3[2], cos)            # the kernel's own summation order gives the cosines back exactly
        for pad in (0, 3):
            for parts in ([cos], parts3):
                nslab, ldz = len(parts), C + pad
                stride = R * ldz + (7 if nslab > 1 else 0)
                buf = torch.full((nslab, stride), hc.SENTINEL, dtype=f32, device=dev())
                for q, part in enumerate(parts):
                    buf[q, :R * ldz].view(R, ldz)[:, :C] = D(part)
                before = buf.clone()
                prob_t, nll_t = nans(R), nans(R)
                what = "%s:ld=%d:nslab=%d:" % (case.name, ldz, nslab)
                run("fedfr_softmax_ce_fused", buf.data_ptr(), lab.data_ptr(), R, C, ldz, s, m, arc, case.inputs["inv_batch"], prob_t.data_ptr(), nslab,
                    stride, nll_t.data_ptr())
                g = buf[0, :R * ldz].view(R, ldz)
                chk(g[:, :C], ref["grad"], what + "grad")
                chk(prob_t, ref["prob_t"], what + "prob_t")
                chk(nll_t, ref["nll_t"], what + "nll_t")
                assert bool((prob_t[bad] == 0).all()) and pad_intact(g, C)
                assert torch.equal(buf[1:], before[1:]) and torch.equal(buf[0, R * ldz:], before[0, R * ldz:])
                # the loss may be left out
                buf.copy_(before)
                prob2 = nans(R)
                run("fedfr_softmax_ce_fused", buf.data_ptr(), lab.data_ptr(), R, C, ldz, s, m, arc, case.inputs["inv_batch"], prob2.data_ptr(), nslab,
                    stride, None)
                assert torch.equal(prob2, prob_t) and torch.equal(buf[0, :R * ldz].view(R, ldz)[:, :C], g[:, :C])


@pytest.mark.parametrize("cfg", hc.SHARDED_CFGS)
@pytest.mark.parametrize("R", hc.SHARDED_R)
def test_sharded_softmax_vs_fp64(R, cfg):
    """one shard of the PartialFC form with the identity as the all-reduce: fedfr_exp_rowsum_target's [row sums | target numerators]
    (exactly 0 where the class lives elsewhere), fedfr_softmax_grad on them, fedfr_nll_mean_ratio with the 1e-30 floor — which the row
    whose numerator underflows hits, as the reference's clamp_min(1e-30) does"""
    s, m, arc = cfg
    case = hc.sharded_case(R, cfg)
    ref = case.ref()
    C = case.inputs["cos"].shape[1]
    lab = D(case.inputs["label"])
    bad = _invalid_rows(case)
    for pad in (0, 3):
        ldz = C + pad
        z = padded(case.inputs["cos"], pad)
        row_max, dmul, prob_t, sums2, loss = nans(R), nans(R), nans(R), nans(2 * R), nans(1)
        what = "%s:ld=%d:" % (case.name, ldz)
        run("fedfr_margin_rowmax", z.data_ptr(), lab.data_ptr(), R, C, ldz, s, m, arc, row_max.data_ptr(), dmul.data_ptr(), None)
        run("fedfr_exp_rowsum_target", z.data_ptr(), lab.data_ptr(), R, C, ldz, row_max.data_ptr(), sums2.data_ptr())
        chk(sums2[:R], ref["row_sum"], what + "sums2[:R]")
        chk(sums2[R:], ref["num"], what + "sums2[R:]")
        assert bool((sums2[R:][bad] == 0).all()) and pad_intact(z, C)
        run("fedfr_softmax_grad", z.data_ptr(), lab.data_ptr(), R, C, ldz, sums2.data_ptr(), dmul.data_ptr(), s, case.inputs["inv_batch"],
            prob_t.data_ptr(), None, None, None)
        chk(z[:, :C], ref["grad"], what + "grad")
        chk(prob_t, ref["prob_t"], what + "prob_t")
        run("fedfr_nll_mean_ratio", sums2[R:].data_ptr(), sums2.data_ptr(), R, hc.FLOOR, loss.data_ptr())
        chk(loss, ref["ratio_loss"], what + "loss")
        if s == 64.0:
            assert float(sums2[R] / sums2[0]) < hc.FLOOR          # row 0: the numerator underflowed; the floor is what keeps the loss finite
        assert pad_intact(z, C)


def test_dense_ce_loss_where_the_target_probability_underflows():
    """ops.cross_entropy on s = 64 CosFace logits whose row 0 has its target 140.8 below the row maximum: softmax probability 8e-62, 0 in
    fp32.  F.cross_entropy returns the finite gap, and so must the dense loss (it is taken in the log domain, (row max - target logit) +
    log(row sum), by the chain and by the fused kernel alike; -log(max(p_target, 0)) gave inf here).  The gradient is the reference's."""
    case = hc.ce_case()
    ref = case.ref()
    logits = D(case.inputs["logits"]).requires_grad_(True)
    lab = D(case.inputs["label"])
    loss = ops.cross_entropy(logits, lab)
    loss.backward()
    torch.cuda.synchronize()
    print("dense CE loss %.9g (fp64 %.9g)" % (float(loss.detach()), float(ref["loss"].value)))
    assert bool(torch.isfinite(loss))
    chk(loss.detach(), ref["loss"], case.name + ":loss")
    chk(logits.grad, ref["grad"], case.name + ":grad")
    # the fused trainer's form of the same loss: the margin applied in the kernel, (cos - m) * s in fp32, which is how the logits were made
    R = logits.shape[0]
    _, g, nll_t = ops.softmax_ce_fused(D(case.inputs["cos"])[None].clone(), lab, 64.0, 0.4, False, 1.0 / R, nll=True)
    chk(ops.nll_rows_mean(nll_t), ref["loss"], case.name + ":fused loss")
    chk(g * (1.0 / 64.0), ref["grad"], case.name + ":fused grad / s")


# ------------------------------------------------------------------------------------------------ small reductions
@pytest.mark.parametrize("n", hc.REDUCE_N)
def test_nll_mean_and_sum_scale(n):
    """one-block reductions below one wave, between 64 and 256, above 256"""
    for floor in (0.0, hc.FLOOR):
        case = hc.nll_mean_case(n, floor)
        p, loss = D(case.inputs["p"]), nans(1)
        run("fedfr_nll_mean", p.data_ptr(), n, floor, loss.data_ptr())
        chk(loss, case.ref()["loss"], case.name)
    for scale in (1.0 / n, -3.0):
        case = hc.sum_scale_case(n, scale)
        x, out = D(case.inputs["x"]), nans(1)
        run("fedfr_sum_scale", x.data_ptr(), n, scale, out.data_ptr())
        chk(out, case.ref()["out"], case.name)


@pytest.mark.parametrize("R,C", hc.COLSUM_SHAPES)
def test_colsum_f32(R, C):
    case = hc.colsum_case(R, C)
    x, out = D(case.inputs["x"]), nans(1, C)
    run("fedfr_colsum_f32", x.data_ptr(), R, C, out.data_ptr())
    chk(out, case.ref()["out"], case.name)


@pytest.mark.parametrize("R,C", hc.MARGIN_BWD_SHAPES)
def test_margin_bwd(R, C):
    """dcos = dlogits * (dmul[row] at the target, s elsewhere) with a dmul that is not s; out-of-range labels have no target column"""
    for case in hc.margin_bwd_cases(R, C):
        i = case.inputs
        dl, dm, lab, out = D(i["dlogits"]), D(i["dmul"]), D(i["label"]), nans(R, C)
        run("fedfr_margin_bwd", dl.data_ptr(), lab.data_ptr(), dm.data_ptr(), i["s"], R, C, out.data_ptr())
        chk(out, case.ref()["dcos"], case.name)


# ------------------------------------------------------------------------------------------------ BCE head
@pytest.mark.parametrize("lam", [0.5, 0.9])
@pytest.mark.parametrize("t", [1, 3])
@pytest.mark.parametrize("B,C", hc.BCE_SHAPES)
def test_bce_logits_and_loss(B, C, t, lam):
    """C not a multiple of the block, t != 1, labels -1 and C (no positive column); every optional output requested and left out in turn"""
    m, r, ls = hc.BCE_M, hc.BCE_R, hc.BCE_LOSS_SCALE
    for case in hc.bce_cases(B, C, t, lam):
        ref, i = case.ref(), case.inputs
        cos, bias, lab = D(i["cos"]), D(i["bias"]), D(i["label"])
        for want_gt, want_d in ((1, 1), (0, 1), (1, 0), (0, 0)):
            z, dzdcos = nans(B, C), nans(B, C)
            gt = torch.full((B, C), 255, dtype=torch.uint8, device=dev())
            run("fedfr_bce_logits", cos.data_ptr(), lab.data_ptr(), bias.data_ptr(), B, C, m, r, float(t), z.data_ptr(),
                gt.data_ptr() if want_gt else None, dzdcos.data_ptr() if want_d else None)
            what = "%s:gt=%d:dzdcos=%d:" % (case.name, want_gt, want_d)
            chk(z, ref["z"], what + "z")
            if want_gt:
                chk(gt, ref["gt"], what + "gt")
            else:
                assert bool((gt == 255).all())
            if want_d:
                chk(dzdcos, ref["dzdcos"], what + "dzdcos")
            else:
                assert bool(torch.isnan(dzdcos).all())
        z_in, gt_in, dzdcos_in = D(i["z"]), D(i["gt"]), D(i["dzdcos"])
        for want_dz, want_dcos in ((1, 1), (0, 1), (1, 0), (0, 0)):
            dz, dcos, row_loss = nans(B, C), nans(B, C), nans(B)
            run("fedfr_bce_loss", z_in.data_ptr(), gt_in.data_ptr(), dzdcos_in.data_ptr() if want_dcos else None, B, C, r, lam, ls,
                dz.data_ptr() if want_dz else None, dcos.data_ptr() if want_dcos else None, row_loss.data_ptr())
            what = "%s:dz=%d:dcos=%d:" % (case.name, want_dz, want_dcos)
            chk(row_loss, ref["row_loss"], what + "row_loss")
            if want_dz:
                chk(dz, ref["dz"], what + "dz")
            else:
                assert bool(torch.isnan(dz).all())
            if want_dcos:
                chk(dcos, ref["dcos"], what + "dcos")
            else:
                assert bool(torch.isnan(dcos).all())


# ------------------------------------------------------------------------------------------------ GEMM
def _strides(M, N, K, ta, tb):
    return ((1, M) if ta else (K, 1)) + ((1, K) if tb else (N, 1))


@pytest.mark.parametrize("ta,tb", hc.GEMM_LAYOUTS)
@pytest.mark.parametrize("K", hc.GEMM_K)
def test_sgemm_options(K, ta, tb):
    """fedfr_sgemm's bias, beta (onto a random C), alpha and ldc > N, alone and together, in all four stride layouts at K on both sides
    of 128 (the k depth of a stage switches there) and K = 1, 3 (a single ragged stage)"""
    M, N = hc.GEMM_MN
    sam, sak, sbk, sbn = _strides(M, N, K, ta, tb)
    for alpha, beta, use_bias, pad in hc.GEMM_OPTIONS:
        case = hc.gemm_case(M, N, K, ta, tb, alpha, beta, use_bias)
        i = case.inputs
        a, b, bias = D(i["a"]), D(i["b"]), D(i["bias"])
        c = padded(i["c_old"] if beta != 0 else torch.full((M, N), NAN), pad)
        run("fedfr_sgemm", a.data_ptr(), b.data_ptr(), c.data_ptr(), M, N, K, sam, sak, sbk, sbn, N + pad, alpha, beta,
            bias.data_ptr() if use_bias else None)
        chk(c[:, :N], case.ref()["c"], "%s:ldc=%d" % (case.name, N + pad))
        assert pad_intact(c, N)


@pytest.mark.parametrize("tb", [False, True])
def test_sgemm_splitk_ldc_and_slab_stride(tb):
    """split-K slabs with ldc > N and slab_stride > M * ldc: every slab is alpha * the product over its own k range, the padding columns
    and the gaps between the slabs are not written; a split that would leave an empty k range is an error"""
    M, N, K, splits, alpha = (hc.SPLITK[k] for k in ("M", "N", "K", "splits", "alpha"))
    cases = hc.splitk_cases(tb)
    a, b = D(cases[0].inputs["a"]), D(cases[0].inputs["b"])
    sam, sak, sbk, sbn = _strides(M, N, K, False, tb)
    ldc = N + 5
    stride = M * ldc + 11
    buf = torch.full((splits, stride), hc.SENTINEL, dtype=f32, device=dev())
    for z in range(splits):
        buf[z, :M * ldc].view(M, ldc)[:, :N] = NAN
    run("fedfr_sgemm_splitk", a.data_ptr(), b.data_ptr(), buf.data_ptr(), M, N, K, sam, sak, sbk, sbn, ldc, alpha, splits, stride)
    for z, case in enumerate(cases):
        slab = buf[z, :M * ldc].view(M, ldc)
        chk(slab[:, :N], case.ref()["c"], "splitk:" + case.name)
        assert pad_intact(slab, N) and bool((buf[z, M * ldc:] == hc.SENTINEL).all())
    assert hc.splitk_chunk(64, 3) * 2 >= 64
    with pytest.raises(RuntimeError):
        _C.call("fedfr_sgemm_splitk", a.data_ptr(), b.data_ptr(), buf.data_ptr(), M, N, 64, sam, sak, sbk, sbn, ldc, alpha, 3, stride, _C.stream())
    torch.cuda.synchronize()
    assert bool((buf[:, M * ldc:] == hc.SENTINEL).all())


# ------------------------------------------------------------------------------------------------ argument validation
def test_ldz_below_C_is_an_error():
    """ldz < C would make rows overlap: rejected on the host, before any launch, by every kernel that takes an ldz"""
    R, C = 3, 40
    z = torch.zeros(R, C, device=dev())
    lab = torch.zeros(R, dtype=torch.int64, device=dev())
    v, w, sums2 = torch.ones(R, device=dev()), torch.ones(R, device=dev()), torch.ones(2 * R, device=dev())
    st = _C.stream()
    with pytest.raises(RuntimeError):
        _C.call("fedfr_exp_rowsum", z.data_ptr(), R, C, C - 1, v.data_ptr(), w.data_ptr(), st)
    with pytest.raises(RuntimeError):
        _C.call("fedfr_exp_rowsum_target", z.data_ptr(), lab.data_ptr(), R, C, C - 1, v.data_ptr(), sums2.data_ptr(), st)
    with pytest.raises(RuntimeError):
        _C.call("fedfr_softmax_grad", z.data_ptr(), lab.data_ptr(), R, C, C - 1, v.data_ptr(), w.data_ptr(), 30.0, 1.0 / R, sums2.data_ptr(),
                None, None, None, st)
    with pytest.raises(RuntimeError):
        _C.call("fedfr_margin_rowmax", z.data_ptr(), lab.data_ptr(), R, C, C - 1, 30.0, 0.4, 0, v.data_ptr(), w.data_ptr(), None, st)
    with pytest.raises(RuntimeError):
        _C.call("fedfr_softmax_ce_fused", z.data_ptr(), lab.data_ptr(), R, C, C - 1, 30.0, 0.4, 0, 1.0 / R, v.data_ptr(), 1, 0, None, st)
    torch.cuda.synchronize()
    assert bool((z == 0).all())


@pytest.mark.parametrize("R,C,arc,nslab", [(9, 257, False, 2), (5, 3000, True, 3), (4, 300, False, 1)])
def test_log_domain_row_loss_is_bit_identical_in_the_chain_and_the_fused_kernel(R, C, arc, nslab):
    """the per-row loss is the same expression on the same row max, row sum and target logit in both forms, labels outside [0, C) included"""
    parts = D(hc.uniform((nslab, R, C), 3) * (0.9 / nslab))
    total = parts[0].clone()
    for q in range(1, nslab):
        total += parts[q]
    lab = D(torch.tensor(([-1, C, C - 1, 0] + list(range(5, 5 + R)))[:R]))
    p_ref, g_ref, n_ref = ops.softmax_ce_grad(total.clone(), lab, 64.0, 0.4, arc, 1.0 / R, nll=True)
    p_got, g_got, n_got = ops.softmax_ce_fused(parts.clone(), lab, 64.0, 0.4, arc, 1.0 / R, nll=True)
    torch.cuda.synchronize()
    assert torch.equal(p_got, p_ref) and torch.equal(g_got, g_ref) and torch.equal(n_got, n_ref)
    assert bool(torch.isinf(n_got[:2]).all()) and bool(torch.isfinite(n_got[2:]).all())
    assert torch.equal(ops.nll_rows_mean(n_got), ops.nll_rows_mean(n_ref))
