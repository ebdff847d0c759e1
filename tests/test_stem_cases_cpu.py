"""CPU checks of tests/stem_cases.py, the references of test_stem_chain_gpu.py.  (1) Precision: the float32 evaluation of every
reference formula, in the kernels' order of operations, stays within a QUARTER of the tolerance the kernels get against float64 — a correct
fp32 kernel passes, and the tolerances hide nothing.  (2) Sensitivity: one row dropped from a column sum, one PReLU mask flipped, the
last pixel omitted, a tap shifted across an image border each move the float64 reference beyond the tolerance.  (3) Conditioning: no
PReLU pre-activation within 1e-3 of zero except the exact ties, no 16-bit result below 2^-11 except exact zeros."""
import pytest
import torch

import stem_cases as K

f32, f64 = K.f32, K.f64
S16 = [torch.float16, torch.bfloat16]


def _stored(q, s16):
    return K.r16(q.value.to(f32), s16)


@pytest.mark.parametrize("s16", S16, ids=["fp16", "bf16"])
@pytest.mark.parametrize("B,HW", K.STEM_FWD_SHAPES)
def test_stem_forward_reference(B, HW, s16):
    c = K.StemFwdCase(B, HW, s16)
    y = c.y()
    q = c.y_q(y)
    K.check(c.y(f32), q, c.name + " y fp32", 0.25)
    assert K.exceeds(c.y(f64, wrap=True), q), "a tap read across the image border must show"
    y16 = K.r16(y.to(f32), s16)
    sq = c.stats_q(y16)
    K.check(c.stats_q(y16, f32).value, sq, c.name + " stats fp32", 0.25)
    assert K.exceeds(c.stats_q(y16, f64, drop=c.M // 2).value, sq) and K.exceeds(c.stats_q(y16, f64, drop=c.M - 1).value, sq)
    if c.M % 256:                                     # the rows of the ragged tile count only real pixels: those beyond are exact zeros
        assert float(sq.value[-(-c.M // 64):].abs().max() if -(-c.M // 64) < sq.value.shape[0] else 0.0) == 0.0


def _check_masks(x, p, keep, what):
    z = x.to(f64) * p.sc.to(f64) + p.sh.to(f64)
    assert bool((z[keep] == 0).all()), what
    assert float(z[~keep & (p.sc != 0).expand_as(keep)].abs().min()) >= K.ZMIN, what
    zf = K.fma(x.to(f32), p.sc, p.sh, f32)
    assert torch.equal(zf <= 0, z <= 0), what         # the mask is the same in every precision: no element needs excluding


@pytest.mark.parametrize("s16", S16, ids=["fp16", "bf16"])
@pytest.mark.parametrize("B,HW", K.STEM_WGRAD_SHAPES)
def test_stem_wgrad_reference(B, HW, s16):
    c = K.StemWgradCase(B, HW, s16)
    assert bool(c.keep.any()) and c.p.gamma[K.NEG] < 0 and c.p.gamma[K.ZERO] == 0
    _check_masks(c.x0, c.p, c.keep, c.name)
    coef = c.coef()
    for a, b, what in zip(c.sums(f32), c.sums_q(), ("sum dz", "sum dz xhat", "sum dy z")):
        K.check(a, b, c.name + " " + what, 0.25)
    K.check(c.coef_q(f32).value, c.coef_q(), c.name + " coef fp32", 0.25)
    q0 = c.dz0(coef)
    live = (c.p.gamma != 0).expand_as(q0.value)
    assert float(q0.value[live].abs().min()) >= K.RMIN and float(q0.value[~live].abs().max()) == 0.0
    K.check(c.dz0(coef, f32).value, q0, c.name + " dz0 fp32", 0.25)
    loudpx = int(torch.nonzero(c.loud)[len(torch.nonzero(c.loud)) // 2])
    flat = int((c.dy.to(f64).abs() * (c.p.gamma != 0)).argmax())            # the mask that is flipped: where the gradient is largest
    flip = (flat // 64, flat % 64)
    assert K.exceeds(c.dz0(coef, f64, flip=flip).value, q0), "one flipped mask must show in dz0"
    dz = _stored(q0, s16)
    for sigma in (0.0, 4.0):                         # the plain bound, and the one with the operand's 16-bit rounding added
        q = c.dw(dz, f64, extra_sigma=sigma)
        K.check(c.dw(dz, f32).value, q, c.name + " dw fp32", 0.25)
        assert K.exceeds(c.dw(dz, f64, drop=loudpx).value, q), "one pixel dropped"
        assert K.exceeds(c.dw(dz, f64, drop=c.M - 1).value, q), "the last pixel of the last stage omitted"
        assert K.exceeds(c.dw(dz, f64, wrap=True).value, q), "a tap read across the image border"
        dzf = _stored(c.dz0(coef, f64, flip=flip), s16)
        assert K.exceeds(c.dw(dzf, f64).value, q), "one flipped mask must show in the weight gradient"


@pytest.mark.parametrize("s16", S16, ids=["fp16", "bf16"])
def test_bn_bwd_rowslab_references(s16):
    for c in K.bn_bwd_cases(s16) + [K.ChainCase(s16).first]:
        M, C = c.M, c.C
        assert c.p.gamma[K.NEG] < 0 and c.p.gamma[K.ZERO] == 0
        if c.alpha:
            _check_masks(c.x, c.p, c.keep, c.name)
        sq = c.sums_q()
        for a, b, what in zip(c.sums(f32), sq, ("dbeta", "dgamma", "dalpha")):
            K.check(a, b, c.name + " " + what, 0.25)
        mid, last, ch = M // 2 + 1, M - 1, 9
        n_sums = 3 if c.alpha else 2
        for i in range(n_sums):
            assert K.exceeds(c.sums(f64, drop=mid)[i], sq[i]) and K.exceeds(c.sums(f64, drop=last)[i], sq[i]), (c.name, i)
        if c.alpha:
            fl = c.sums(f64, flip=(mid, ch))
            assert all(K.exceeds(fl[i], sq[i]) for i in range(3)), c.name
        K.check(c.coef_q(f32).value, c.coef_q(), c.name + " coef fp32", 0.25)
        coef = c.coef()
        q = c.dx(coef)
        live = (c.p.gamma != 0).expand_as(q.value)
        assert float(q.value[live].abs().min()) >= K.RMIN, c.name
        if c.extra is None:
            assert float(q.value[~live].abs().max()) == 0.0
        K.check(c.dx(coef, f32).value, q, c.name + " dx fp32", 0.25)
        if c.alpha:
            assert K.exceeds(c.dx(coef, f64, flip=(mid, ch)).value, q), c.name
        if c.frozen:                                  # an infinite count: A = B = 0, dx = a dz
            assert float(coef[1:].abs().max()) == 0.0
        if c.nx_mode:
            if c.nx_mode == 2:
                _check_masks(c.nx, c.np, c.nkeep, c.name + " next")
            dx16 = _stored(q, s16)
            nq = c.next_sums_q(dx16)
            n32 = c.next_sums_q(dx16, f32)
            for i in range(3):
                K.check(n32[i].value, nq[i], c.name + " next sum %d fp32" % i, 0.25)
            for i in range(3 if c.nx_mode == 2 else 2):
                assert K.exceeds(c.next_sums_q(dx16, f64, drop=mid)[i].value, nq[i]), (c.name, i)
                assert K.exceeds(c.next_sums_q(dx16, f64, drop=last)[i].value, nq[i]), (c.name, i)
            if c.nx_mode == 2:
                fl = c.next_sums_q(dx16, f64, flip=(mid, ch))
                assert all(K.exceeds(fl[i].value, nq[i]) for i in range(3)), c.name
            else:
                assert float(nq[2].value.abs().max()) == 0.0


def test_geometry_formulas():
    """the shapes reach what they are meant to reach (the GPU test asserts the same against the library's own row queries)"""
    assert K.slab_rows(3000, 64, K.APPLY_BLOCKS) == 256 and -(-3000 // 256) == 12 and 3000 - 11 * 256 == 184
    assert K.slab_rows(250037, 64, K.APPLY_BLOCKS) == 352 > 8 * K.rows_per_pass(64)
    assert K.rows_per_pass(96) == 21 and 21 * 12 == 252 and K.rows_per_pass(512) == 4
    assert (K.stem_px_per_block(11 * 112 * 112), K.stem_px_per_block(53 * 50 * 50), K.stem_px_per_block(100)) == (256, 256, 128)
    assert 11 * 112 * 112 % 256 == 0 and 53 * 50 * 50 % 256 == 128 + 20
    assert -(-33 * 127 * 127 // 256) > 2048 and 33 * 127 * 127 % 256 and 3 * 37 * 37 % 256
