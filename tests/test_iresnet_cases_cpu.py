"""tests/iresnet_cases.py proven on the CPU before a GPU sees it:
  * the restated dispatch (conv kernel selector, BatchNorm row counts and sliced predicates, weight-gradient splits) against the library's host
    functions for every block shape of iresnet18 / 50 / 100 and of the (1, 1, 3, 1) carry net at every batch 1 .. 256;
  * the carry rule: iresnet18 has NO carrying paired launch at any batch (a pair's slabs are always flushed by the downsample block in front of it), the
    (1, 1, 3, 1) net has one from the batch case_batches() computes;
  * a miniature stack — a downsample block and two identity blocks behind it on an 8 x 8 map, evaluated here in plain float32 torch with 16-bit
    stores at the kernels' rounding points, in every combination of the plan's alternatives (bn_apply2 or separate passes, rows from the dgrad
    accumulator or from the stored tensor) — passes `compare` with every ratio < 1 in both storage types;
  * planted faults: each pushes the comparison named for it above 1 while every other comparison stays below;
  * the miniature stack carries the network's tail too (bn2, flatten, fc, features and their backward), so every comparison of `compare` but the
    stem's runs here."""
import ctypes as C

import pytest
import torch

import bn_sliced_cases as BS
import conv_cases as K
import iresnet_cases as IC
import rowslab_cases as RS
import stem_cases as S
from stem_cases import f32, f64

MINI = (8, 32, (64,))                       # input side, input channels, planes: layer1.0 32 -> 64 stride 2 with downsample, layer1.1, layer1.2 64 -> 64 at 4 x 4
MINI_LAYERS = (3,)
MINI_B = 2


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from fedfr_amd import _C
    return _C.lib()


# ================================================================================================ dispatch against the library
def block_shapes():
    seen = []
    for layers in list(IC.LAYERS.values()) + [IC.CARRY_LAYERS]:
        for b in IC.build_blocks(layers, 112):
            k = (b.cin, b.cout, b.stride, b.hin, b.has_ds)
            if k not in seen:
                seen.append(k)
    return seen


def test_restated_dispatch_agrees_with_the_library_for_every_block_shape_and_batch(lib):
    shapes = block_shapes()
    assert len(shapes) == 8                                   # per stage: the downsample block and the identity block
    out5 = [C.c_int() for _ in range(5)]

    def plan(B, hin, cin, cout, k, s, dgrad, want):
        assert lib.fedfr_conv2d_plan(B, hin, cin, cout, k, s, dgrad, want, *[C.byref(v) for v in out5]) == 0, lib.fedfr_last_error_string()
        return tuple(v.value for v in out5[:4]) + (bool(out5[4].value),)
    for B in range(1, 257):
        net = IC.Net(IC.LAYERS["iresnet18"], B)
        for cin, cout, stride, hin, ds in shapes:
            hout = hin // stride
            Mi, Mo = B * hin * hin, B * hout * hout
            for a in ((hin, cin, cout, 3, 1, 0, K.WANT_STATS), (hin, cout, cout, 3, stride, 0, K.WANT_STATS), (hin, cin, cout, 3, 1, 1, 0),
                      (hin, cin, cout, 3, 1, 1, K.WANT_BNBWD), (hin, cout, cout, 3, stride, 1, 0), (hin, cout, cout, 3, stride, 1, K.WANT_BNBWD)):
                assert plan(B, *a) == net.plan(*a), (B, a)
            if not ds:
                a = (hin, cout, cout, 3, 1, 0, K.WANT_MOMENTS)
                assert plan(B, *a) == net.plan(*a), (B, a)
            else:
                for a in ((hin, cin, cout, 1, stride, 0, K.WANT_STATS), (hin, cin, cout, 1, stride, 1, 0)):
                    assert plan(B, *a) == net.plan(*a), (B, a)
            assert lib.fedfr_conv2d_stat_rows(B, hout, cout) == K.nt_stat_rows(Mo, cout)
            for M, Cc in ((Mi, cin), (Mi, cout), (Mo, cout)):
                for bw in (0, 1):
                    G = BS.sliced_geometry(M, Cc, bool(bw))[0]
                    assert lib.fedfr_bn_sliced_rows(M, Cc, bw) == G, (M, Cc, bw)
                    for P in (1, G, 128, 129, 256, 257, 260, 261):
                        assert bool(lib.fedfr_bn_sliced_ok(M, Cc, P, bw)) == BS.sliced_ok(M, Cc, P, bool(bw)), (M, Cc, P, bw)
                assert lib.fedfr_bn_bwd_rows(M, Cc) == K.cdiv(M, S.slab_rows(M, Cc, S.REDUCE_BLOCKS))
                assert lib.fedfr_bn_bwd_apply_rows(M, Cc) == K.cdiv(M, S.slab_rows(M, Cc, S.APPLY_BLOCKS))
                assert lib.fedfr_bn_apply_stat_rows(M, Cc) == RS.geometry(M, Cc, RS.APPLY_BLOCKS)["grid"]
                assert lib.fedfr_prelu_bwd_rows(M, Cc) == RS.geometry(M, Cc, RS.PRELU_BLOCKS)["grid"]
            # the split-K slabs of every weight gradient fit the workspace the library sizes for the shape
            blk = IC.Block(0, "", cin, cout, stride, hin, ds)
            for which, (ci, co, k, s) in ((2, (cout, cout, 3, stride)), (1, (cin, cout, 3, 1))) + (((0, (cin, cout, 1, stride)),) if ds else ()):
                sp = net.wgrad(blk, which)[1]
                assert sp >= 1 and lib.fedfr_conv2d_wgrad_ws_bytes(B, hin, ci, co, k, s) >= (sp if sp > 1 else 0) * co * k * k * ci * 4, (B, which)


def test_carry_rule_iresnet18_never_carries_the_chosen_net_does():
    for B in range(1, 257):
        net = IC.Net(IC.LAYERS["iresnet18"], B)
        carries, red = net.wgrad_walk()
        assert carries == [] and red == net.wgrad_walk(bg=False)[1], B          # wgrad9p_bg is inert on iresnet18
    cases = IC.case_batches()
    carry_cases = [(l, B) for l, B in cases if l == IC.CARRY_LAYERS]
    assert len(carry_cases) == 2
    for l, B in carry_cases:
        net = IC.Net(l, B)
        carries, red = net.wgrad_walk()
        assert carries and all(not net.blocks[i].has_ds for i in carries), (B, carries)
        assert net.wgrad_walk(bg=False)[1] == red + 2 * len(carries)           # every carry takes two stand-alone reductions away
    first = carry_cases[0][1]
    assert not IC.Net(IC.CARRY_LAYERS, first - 1).wgrad_walk()[0] and first > 1
    # the computed thresholds are where the restated rules flip
    L18 = IC.LAYERS["iresnet18"]
    bs = [B for l, B in cases if l == L18]
    assert bs[:2] == [1, 5] and 128 in bs and len(set(bs)) == len(bs)
    for B in bs[2:]:
        assert B > 5
    assert IC.pair_reduce_case() in cases and IC.pair_reduce_case()[0] == L18


# ================================================================================================ the miniature stack in float32
def fma32(a, b, c):
    return S.fma(a.to(f32), b.to(f32), c.to(f32).expand_as(a), f32)


def fwd_coef32(S0, S1, M, gamma, beta, rm0, rv0):
    """bn_fwd_coef + bn_running_update on fp32 rows: fp64 up to one fp32 store each -> (save [4][C], running_mean, running_var)"""
    mean, e2 = S0.to(f32).to(f64) / M, S1.to(f32).to(f64) / M
    return coef_from(mean, (e2 - mean * mean).clamp_min(0.0), M, gamma, beta, rm0, rv0)


def coef_from(mean, var, M, gamma, beta, rm0, rv0):
    rstd = 1.0 / torch.sqrt(var + BS.EPSF)
    g, b = gamma.to(f64), beta.to(f64)
    k = M / (M - 1.0)
    save = torch.stack([g * rstd, b - mean * g * rstd, mean, rstd]).to(f32)
    return save, ((1.0 - BS.MOM) * rm0.to(f64) + BS.MOM * mean).to(f32), ((1.0 - BS.MOM) * rv0.to(f64) + BS.MOM * var * k).to(f32)


def evaluate(net, s16, fault=None):
    """the miniature stack's forward and backward pass in float32 with 16-bit stores where the kernels store; fault: a planted error (see the test)"""
    B, scale = net.B, (S.GSCALE if s16 == torch.float16 else 1.0)
    r16 = lambda t: t.to(f32).to(s16)  # noqa: E731
    T = dict(par={}, grad={}, buf0={}, buf={}, save={}, blk=[], cap=[None] * len(net.blocks))
    seed = [100]

    def rnd(shape, lo=-1.0, hi=1.0):
        seed[0] += 1
        return S.uniform(shape, seed[0], lo, hi)
    for b in net.blocks:
        p = b.prefix
        for _, n, c in b.bns():
            T["par"][n + ".weight"], T["par"][n + ".bias"] = rnd((c,), 0.8, 1.2), rnd((c,), -0.1, 0.1)
            T["par"][n + ".weight"][1] *= -1.0
            T["buf0"][n] = (rnd((c,), -0.1, 0.1), rnd((c,), 0.9, 1.1))
        T["par"][p + "conv1.weight"] = rnd((b.cout, 3, 3, b.cin)) * 0.1
        T["par"][p + "conv2.weight"] = rnd((b.cout, 3, 3, b.cout)) * 0.1
        T["par"][p + "prelu.weight"] = rnd((b.cout,), 0.15, 0.35)
        if b.has_ds:
            T["par"][p + "downsample.0.weight"] = rnd((b.cout, 1, 1, b.cin)) * 0.2
    w16 = lambda n: T["par"][n].to(s16)  # noqa: E731
    conv = lambda x, w, s, **kw: K.conv_ref(x, w, s, f32, "cpu", **kw)  # noqa: E731

    def bn_train(name, x2d):
        xd = x2d.to(f64)
        M = x2d.shape[0]
        T["save"][name], rm, rv = fwd_coef32(xd.sum(0), (xd * xd).sum(0), M, T["par"][name + ".weight"], T["par"][name + ".bias"], *T["buf0"][name])
        T["buf"][name] = (rm, rv)
        return T["save"][name]
    # ---------------------------------------------------------------- forward
    x = r16(rnd((B, net.hin, net.hin, net.blocks[0].cin)) * 2 + 0.3)
    a1_ready = None
    for b in net.blocks:
        p, t = b.prefix, {"x": x}
        Mi, Mo = B * b.hin * b.hin, B * b.hout * b.hout
        x2 = x.reshape(Mi, b.cin)
        if a1_ready is None:
            sv = bn_train(p + "bn1", x2)
            t["a1"] = r16(fma32(x2, sv[0], sv[1])).reshape(x.shape)
        else:
            t["a1"] = a1_ready
        t["c1"] = r16(conv(t["a1"], w16(p + "conv1.weight"), 1)["y"])
        c1 = t["c1"].reshape(Mi, b.cout)
        sv = bn_train(p + "bn2", c1)
        z = fma32(c1, sv[0], sv[1])
        t["a2"] = r16(torch.where(z <= 0, T["par"][p + "prelu.weight"] * z, z)).reshape(t["c1"].shape)
        t["c2"] = r16(conv(t["a2"], w16(p + "conv2.weight"), b.stride)["y"])
        c2 = t["c2"].reshape(Mo, b.cout)
        sv3 = bn_train(p + "bn3", c2)
        o = fma32(c2, sv3[0], sv3[1])
        if b.has_ds:
            t["d"] = r16(conv(x, w16(p + "downsample.0.weight"), b.stride)["y"])
            d = t["d"].reshape(Mo, b.cout)
            svd = bn_train(p + "downsample.1", d)
            o = o + fma32(d, svd[0], svd[1])
        else:
            o = o + x2.to(f32)
        out = r16(o)
        if fault == "out_row" and b.idx == 1:                # one pixel row of the last image taken from its neighbour
            out[-1] = out[-2]
        t["out"] = out.reshape(B, b.hout, b.hout, b.cout)
        a1_ready = None
        if net.xmom(b):                                      # bn_apply2: the next block's bn1 from conv2's moments and this block's saved bn1 statistics
            nb = net.blocks[b.idx + 1]
            n1 = nb.prefix + "bn1"
            cd, xd = c2.to(f64), x2.to(f64)
            rows = torch.stack([cd.sum(0), (cd * xd).sum(0), (cd * cd).sum(0)]).to(f32).to(f64)
            mean, e2 = rows[0] / Mo, rows[2] / Mo
            var = (e2 - mean * mean).clamp_min(0.0)
            xs = T["save"][p + "bn1"]
            mx = xs[2].to(f64)
            vx = (1.0 / (xs[3].to(f64) ** 2) - BS.EPSF).clamp_min(0.0)
            s, h = sv3[0].to(f64), sv3[1].to(f64)
            cov = rows[1] / Mo - mean * mx
            omean, ovar = s * mean + h + mx, (s * s * var + vx + 2.0 * s * cov).clamp_min(0.0)
            T["save"][n1], rm, rv = coef_from(omean, ovar, Mo, T["par"][n1 + ".weight"], T["par"][n1 + ".bias"], *T["buf0"][n1])
            T["buf"][n1] = (rm, rv)
            use = T["save"][p + "bn1"] if fault == "a1_coef" else T["save"][n1]          # the fault: this block's bn1 coefficients
            a1_ready = r16(fma32(out, use[0], use[1])).reshape(t["out"].shape)
        T["blk"].append(t)
        x = t["out"]
    last = net.blocks[-1]
    Mf, F = B * net.hw, net.F
    if net.tail:                                             # bn2 -> NCHW flatten -> fc -> features (BatchNorm1d), as net_forward's tail
        T["par"]["bn2.weight"], T["par"]["bn2.bias"], T["buf0"]["bn2"] = rnd((net.C,), 0.8, 1.2), rnd((net.C,), -0.1, 0.1), (rnd((net.C,), -0.1, 0.1), rnd((net.C,), 0.9, 1.1))
        o2 = x.reshape(Mf, net.C)
        sv = bn_train("bn2", o2)
        T["t"] = r16(RS.nchw(fma32(o2, sv[0], sv[1]), net.hw).reshape(B, net.fc_in))
        T["par"]["fc.weight"], T["par"]["fc.bias"] = rnd((F, net.fc_in)) * 0.05, rnd((F,)) * 0.05
        T["yfc"] = T["t"].to(f32) @ w16("fc.weight").to(f32).t() + T["par"]["fc.bias"]
        T["par"]["features.weight"], T["par"]["features.bias"] = rnd((F,), 0.8, 1.2), rnd((F,), -0.1, 0.1)
        T["buf0"]["features"] = (rnd((F,), -0.1, 0.1), rnd((F,), 0.9, 1.1))
        yd = T["yfc"].to(f64)
        mu = yd.mean(0)
        var = ((yd - mu) ** 2).mean(0)
        T["fsave"] = torch.stack([mu, 1.0 / torch.sqrt(var + BS.EPSF)]).to(f32)
        T["buf"]["features"] = (((1.0 - BS.MOM) * T["buf0"]["features"][0].to(f64) + BS.MOM * mu).to(f32),
                                ((1.0 - BS.MOM) * T["buf0"]["features"][1].to(f64) + BS.MOM * var * B / (B - 1.0)).to(f32))
        T["feats"] = (T["yfc"] - T["fsave"][0]) * T["fsave"][1] * T["par"]["features.weight"] + T["par"]["features.bias"]
    # ---------------------------------------------------------------- backward
    if net.tail:
        T["dfeats"] = dfe = rnd((B, F)) * scale
        xh = (T["yfc"] - T["fsave"][0]) * T["fsave"][1]
        S1, S2 = dfe.to(f64).sum(0), (dfe.to(f64) * xh.to(f64)).sum(0)
        T["grad"]["features.bias"] = S1.to(f32)
        dy = (T["par"]["features.weight"] * T["fsave"][1]) * (dfe - (S1 / B).to(f32) - xh * (S2 / B).to(f32))
        T["grad"]["fc.bias"] = dy.to(f64).sum(0).to(f32)
        dyb = r16(dy).to(f32)
        T["grad"]["fc.weight"] = dyb.t() @ T["t"].to(f32)
        dx = dyb @ w16("fc.weight").to(f32)                  # [B][C hw] in NCHW order -> NHWC
        T["gt"] = r16(dx.reshape(Mf, net.C) if fault == "gt_nchw" else dx.reshape(B, net.C, net.hw).permute(0, 2, 1).reshape(Mf, net.C))
        g = None                                             # bn2's backward, below, forms the gradient entering the last block
    else:
        g = r16((rnd((B * last.hout * last.hout, last.cout)) + 0.1) * scale)

    def bn_bwd(name, dy_sum, dy_apply, x2d, alpha, extra, drop_rows=None):
        """sums from dy_sum (the stored tensor or the dgrad accumulator), dx from the stored dy_apply: returns the stored dx"""
        sv = T["save"][name]
        M = x2d.shape[0]
        pp = IC.BnP(T["par"][name + ".weight"], T["par"][name + ".bias"], sv)
        dyv, xv = dy_sum.to(f64), x2d.to(f64)
        neg = None
        if alpha is not None:
            z = fma32(x2d, sv[0], sv[1])
            neg = z <= 0
            dz, t2 = torch.where(neg, dyv * alpha.to(f64), dyv), torch.where(neg, dyv * z.to(f64), torch.zeros_like(dyv))
        else:
            dz, t2 = dyv, torch.zeros_like(dyv)
        t1 = dz * (xv - sv[2].to(f64)) * sv[3].to(f64)
        if drop_rows is not None:                            # the fault: one partial-statistics row left out of the dgamma sum
            t1 = t1.clone()
            t1[drop_rows] = 0
        S0, S1, S2 = dz.sum(0).to(f32), t1.sum(0).to(f32), t2.sum(0).to(f32)
        T["grad"][name + ".bias"], T["grad"][name + ".weight"] = S0, S1
        coef = S.bn_coef(S0, S1, pp, float(M)).to(f32)
        da = dy_apply.to(f32)
        dza = da if alpha is None else torch.where(neg, da * alpha, da)
        return r16(S.bn_dx(coef, dza, x2d, f32, extra)[0]), S2

    def slabs(x_, dy_, s, which):
        """a split-K weight gradient: one slab per image group, added last; the faults drop one slab / add one twice"""
        w = torch.zeros(dy_.shape[-1], 3 if which else 1, 3 if which else 1, x_.shape[-1], dtype=s16)
        parts = [conv(x_[i:i + 1], w, s, dy=dy_[i:i + 1], want=("dw",))["dw"] for i in range(B)]
        if fault == "slab_drop" and which == 2:
            parts = parts[:-1]
        if fault == "slab_twice" and which == 1:
            parts = parts + parts[-1:]
        return sum(parts[1:], parts[0])
    if net.tail:
        g, _ = bn_bwd("bn2", T["gt"], T["gt"], T["blk"][last.idx]["out"].reshape(Mf, net.C), None, None)
    for b in reversed(net.blocks):
        p, t, c = b.prefix, T["blk"][b.idx], {"g": g}
        Mi, Mo = B * b.hin * b.hin, B * b.hout * b.hout
        faulty_pair = b.idx == 2                               # the pair whose slabs the next paired launch (block 1) carries
        drop = slice(0, Mo // 4) if (fault == "dgamma_row" and b.idx == 1) else None
        dc2, _ = bn_bwd(p + "bn3", g, g, t["c2"].reshape(Mo, b.cout), None, None, drop)
        c["dc2"] = dc2.reshape(t["c2"].shape)
        acc = conv(t["a2"], w16(p + "conv2.weight"), b.stride, dy=c["dc2"], want=("dx",))["dx"]
        c["da2"] = r16(acc)
        src = acc if net.fused_rows(b, 2) else c["da2"]
        dc1, S2 = bn_bwd(p + "bn2", src.reshape(Mi, b.cout), c["da2"].reshape(Mi, b.cout), t["c1"].reshape(Mi, b.cout), T["par"][p + "prelu.weight"], None)
        T["grad"][p + "prelu.weight"] = S2
        c["dc1"] = dc1.reshape(t["c1"].shape)
        extra = g.to(f32)
        if b.has_ds:
            dd, _ = bn_bwd(p + "downsample.1", g, g, t["d"].reshape(Mo, b.cout), None, None)
            c["dd"] = dd.reshape(t["d"].shape)
            wd = w16(p + "downsample.0.weight").to(f32).reshape(b.cout, b.cin)
            c["dxd"] = r16(dd.to(f32) @ wd).reshape(B, b.hout, b.hout, b.cin)
            T["grad"][p + "downsample.0.weight"] = conv(t["x"], w16(p + "downsample.0.weight"), b.stride, dy=c["dd"], want=("dw",), slabs=B)["dw"]
            e = torch.zeros(B, b.hin, b.hin, b.cin)
            o0 = 1 if fault == "dxd_odd" else 0              # the fault: scattered to the odd pixels
            e[:, o0::2, o0::2] = c["dxd"].to(f32)
            extra = e.reshape(Mi, b.cin)
        if faulty_pair:
            T["grad"][p + "conv2.weight"] = slabs(t["a2"], c["dc2"], b.stride, 2)
            T["grad"][p + "conv1.weight"] = slabs(t["a1"], c["dc1"], 1, 1)
        else:
            T["grad"][p + "conv2.weight"] = conv(t["a2"], w16(p + "conv2.weight"), b.stride, dy=c["dc2"], want=("dw",), slabs=B)["dw"]
            T["grad"][p + "conv1.weight"] = conv(t["a1"], w16(p + "conv1.weight"), 1, dy=c["dc1"], want=("dw",), slabs=B)["dw"]
        acc = conv(t["a1"], w16(p + "conv1.weight"), 1, dy=c["dc1"], want=("dx",))["dx"]
        c["da1"] = r16(acc)
        src = acc if net.fused_rows(b, 1) else c["da1"]
        if fault == "no_shortcut" and b.idx == 2:            # the fault: the last image leaves without its shortcut addend
            extra = extra.clone()
            extra[-(b.hin * b.hin):] = 0
        gin, _ = bn_bwd(p + "bn1", src.reshape(Mi, b.cin), c["da1"].reshape(Mi, b.cin), t["x"].reshape(Mi, b.cin), None, extra)
        T["cap"][b.idx] = c
        g = gin
    T["gin0"] = g
    return T


def mini_net(xmom, fused):
    net = IC.Net(MINI_LAYERS, MINI_B, mini=MINI, F=64)
    net.tail = True
    net.mini_xmom, net.mini_fused, net.mini_splits, net.mini_carry = set(xmom), set(fused), MINI_B, {1}
    return net


FUSED_ALL = {(i, w) for i in range(3) for w in (1, 2)}


@pytest.mark.parametrize("s16", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("xmom,fused", [((), ()), ((1,), ()), ((1,), FUSED_ALL), ((), {(1, 2), (2, 1)})], ids=["plain", "xmom", "xmom+fused", "mixed"])
def test_miniature_stack_passes_every_comparison(s16, xmom, fused):
    net = mini_net(xmom, fused)
    assert [b.has_ds for b in net.blocks] == [True, False, False] and net.wgrad_walk() == ([1], 2 + 3)
    T = evaluate(net, s16)
    info = {}
    res = list(IC.compare(net, T, s16, "cpu", info=info))
    assert len(res) == 8 + 12 + sum(37 + 12 * b.has_ds for b in net.blocks), len(res)      # bn2 / t / yfc, features / fc / bn2 backward / last g, the blocks
    bad = [(w, r) for w, r in res if not r < 1.0]
    print("ambiguous PReLU elements: %d; worst: %s" % (info["ambiguous"], sorted(res, key=lambda wr: -wr[1])[:4]))
    assert not bad, bad


FAULTS = {                                   # fault -> the comparisons that must see it (every other one stays below 1)
    "out_row": {"out[1]"},
    "dgamma_row": {"layer1.1.bn3 dgamma"},
    "a1_coef": {"a1[2]"},
    "no_shortcut": {"gin[2]"},
    "dxd_odd": {"gin[0]"},
    "slab_drop": {"layer1.2.conv2 dw"},
    "slab_twice": {"layer1.2.conv1 dw"},
    "gt_nchw": {"gt"},                       # the fc's input gradient left in NCHW order
}


@pytest.mark.parametrize("s16", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_planted_faults_are_caught_by_the_comparison_named_for_them(s16, fault):
    net = mini_net((1,), FUSED_ALL)
    res = dict(IC.compare(net, evaluate(net, s16, fault), s16, "cpu"))
    over = {w for w, r in res.items() if not r <= 1.0}
    assert over == FAULTS[fault], (fault, {w: res[w] for w in over | FAULTS[fault]})


def _stem_reduction(M, s16, seed):
    """(ratio of the stem BatchNorm's backward sums taken from the UNROUNDED gradient, the same from the stored one) against compare's reference,
    which sums the STORED 16-bit gradient — what the kernels reduce (stem_cases.BnBwdCase.next_sums_q)"""
    scale = S.GSCALE if s16 == torch.float16 else 1.0
    c0 = (S.uniform((M, 64), seed) * 2 + 0.3).to(s16)
    xd = c0.to(f64)
    gamma, beta = S.uniform((64,), seed + 1, 0.8, 1.2), S.uniform((64,), seed + 2, -0.1, 0.1)
    save, _, _ = fwd_coef32(xd.sum(0), (xd * xd).sum(0), M, gamma, beta, torch.zeros(64), torch.ones(64))
    p, alpha = IC.BnP(gamma, beta, save), S.uniform((64,), seed + 3, 0.15, 0.35)
    g = (S.uniform((M, 64), seed + 4) + 0.1) * scale              # the gradient before its 16-bit store
    z, mag = IC.affine(c0, p.sc, p.sh)
    neg, amb = IC.prelu_side(c0, p.sc, p.sh, z, mag)
    val, tol = IC.bwd_sums(g.to(s16).to(f64), c0, p, alpha, IC.Net.chain_bwd(M, 64, "next"), neg, amb)
    unrounded, _ = IC.bwd_sums(g.to(f64), c0, p, alpha, 1, neg, amb)
    stored32 = torch.stack([v.to(f32).to(f64) for v in val])
    return float(((unrounded - val).abs() / tol).max()), float(((stored32 - val).abs() / tol).max())


@pytest.mark.parametrize("s16", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_stem_reduction_from_the_unrounded_gradient_is_rejected_where_it_can_be_evaluated(s16):
    """The stem BatchNorm's reduction rides in the first block's bn1 pass and sums the gradient that pass STORED (bn_rowslab.hip), so compare's reference
    sums the stored gradient.  Summing the unrounded value instead differs by a random walk of M independent 16-bit roundings, about
    u16 sqrt(sum g^2 / 3) per column, against the bound chain 2^-24 sum |g|: the ratio falls as 1 / (chain sqrt(M)).  Asserted here: the formula
    REJECTS that fault at a 34 x 34 map in both storage types, and the ratio falls with M (fp16, the product's batch 16, M = 200 704, where it is
    still above 1).  Not asserted, because M = 1.6 million is no CPU test: by that scaling the bound would stop telling the two apart somewhere
    above batch 16 — a limit of any bound that admits a correct kernel's fp32 accumulation; the 16-bit rounding of that gradient is held by
    `gin[0]` itself, element by element, at every batch."""
    small, own = _stem_reduction(3 * 34 * 34, s16, 700)
    assert own < 0.25 and small > 1.0, (small, own)
    if s16 == torch.float16:
        big, own = _stem_reduction(16 * 112 * 112, s16, 710)
        print("unrounded-gradient stem reduction, error / bound: %.3g at M = %d, %.3g at M = %d" % (small, 3 * 34 * 34, big, 16 * 112 * 112))
        assert own < 0.25 and big < small, (big, small, own)
