"""The instruments of tests/test_sphnet_units_gpu.py, proved here without a GPU (tests/sphnet_cases.py).

On a miniature stack with the wiring of a sphnet — a padded 3 -> 64 stage head into an 8x8 map, one residual block of 64 channels, a stride-2 head into a
second stage, the NCHW-flat last activation and the fc — a float32 / 16-bit evaluation in the kernels' order is held to the float64 references:
  * taken BEFORE each final 16-bit store and without the intermediate stores of the two double-rounded quantities, it stays within a QUARTER of
    every bound;
  * as stored, with either arrangement of the rounding points (the dgrad epilogue applying u1's PReLU backward, or dt1 stored and multiplied by a
    second pass), it stays within every bound;
  * each planted fault moves at least one stored quantity outside its bound.
The computed case batches and the per-unit slot tables for them are asserted as literals: a retuned dispatch rule shows up here."""
import pytest
import torch

import conv_cases as K
import rowslab_cases as RS
import sphnet_cases as SC
from stem_cases import GSCALE, f32, uniform

MINI = ((1, 0), (3, 64, 64), 16, 32)
S16 = (torch.float16, torch.bfloat16)


def mini_inputs(net, s16):
    P = dict(x=uniform((net.B, 3, net.hin, net.hin), 1), w=[], b=[], a=[])
    for u in net.units:
        w = uniform((u.cout, 3, 3, u.cin_real), 10 + u.idx) * (0.3 if u.cin_real == 3 else 0.06)
        w[:16] = w[:16].abs()                               # coherent output channels: S ~ |ref| there, the bound sees the rounding mode of a store
        P["w"].append(w)
        P["b"].append(uniform((u.cout,), 30 + u.idx) * 0.3 if u.bias else None)
        P["a"].append(uniform((u.cout,), 50 + u.idx) * 0.1 + 0.25)
    P["fcw"], P["fcb"] = uniform((net.F, net.fc_in), 70) * 0.05, uniform((net.F,), 71) * 0.1
    P["dfeats"] = uniform((net.B, net.F), 72) * (GSCALE if s16 == torch.float16 else 1.0)
    return P


def evaluate(net, P, s16, fused, mut=None):
    """(T, G): the stored tensors of a float32 / 16-bit evaluation in kernel order, and the float32 values before their final stores (the two
    double-rounded quantities without their intermediate store).  fused: u1's PReLU backward in conv2's dgrad epilogue.  mut: a planted fault"""
    B, U = net.B, net.units
    f = lambda t: t.to(f32)  # noqa: E731
    T = dict(P, inp=[], c=[], t=[], dz=[None] * len(U), dw=[None] * len(U), db=[None] * len(U), da=[None] * len(U), cap={})
    G = dict(inp=[], c=[], t=[], dz=[None] * len(U), dw=T["dw"], db=T["db"], da=[None] * len(U), cap={})
    T["xin"] = G["xin"] = SC.pad_input_ref(P["x"], s16)
    w16 = [SC.w16_of(u, P["w"][u.idx], s16) for u in U]
    cur = T["xin"]
    for u in U:
        i = u.idx
        T["inp"].append(cur)
        cf = K.conv_ref(cur, w16[i], u.stride, f32, "cpu", want=("y",))["y"]
        c = cf.to(s16)
        z = f(c) if P["b"][i] is None else f(c) + P["b"][i]
        y = torch.where(z > 0, z, P["a"][i] * z)
        if u.ident is not None:
            y = y + f(cur if mut == "identity_from_u1" else T["inp"][u.ident])
        t = K.trunc16(y, s16).to(s16) if (mut == "truncated_store" and u.kind == "u1") else y.to(s16)
        if u is U[-1]:
            nchw = lambda v: (v.reshape(B, -1) if mut == "left_nhwc" else RS.nchw(v.reshape(-1, u.cout), net.hw).reshape(B, -1))  # noqa: E731
            y, t = nchw(y), nchw(t)
        T["c"].append(c), T["t"].append(t), G["c"].append(cf), G["t"].append(y)
        cur = t
    flat, fw = f(T["t"][-1]), f(P["fcw"].to(s16))
    T["feats"] = G["feats"] = flat @ fw.t() + P["fcb"]
    dfe16 = f(P["dfeats"].to(s16))
    T["dfcb"] = G["dfcb"] = P["dfeats"].sum(0)
    T["dfcw"] = G["dfcw"] = dfe16.t() @ flat
    last = U[-1]
    gf = (dfe16 @ fw).reshape(B, net.C, net.hw).permute(0, 2, 1).reshape(B, last.hout, last.hout, net.C)
    g16 = gf.to(s16)
    dgrad = lambda u, dz: K.conv_ref(torch.zeros(B, u.hin, u.hin, u.cin), w16[u.idx], u.stride, f32, "cpu", dy=dz, want=("dx",))["dx"]  # noqa: E731
    for u in reversed(U):
        i = u.idx
        if u.kind != "u1":
            T["cap"][i], G["cap"][i] = g16, gf
            z = f(T["c"][i]) if P["b"][i] is None else f(T["c"][i]) + P["b"][i]
            neg = (f(T["c"][i]) <= 0) if mut == "bias_not_in_sign" else (z <= 0)
            dzf = torch.where(neg, f(g16) * P["a"][i], f(g16))
            T["dz"][i], G["dz"][i] = dzf.to(s16), dzf
            if u.bias:
                T["db"][i] = dzf.reshape(-1, u.cout).sum(0)
            T["da"][i] = G["da"][i] = torch.where(~neg if mut == "dalpha_over_positive" else neg, f(g16) * z, torch.zeros_like(z)).reshape(-1, u.cout).sum(0)
        if u.kind == "u2":
            dtf = dgrad(u, T["dz"][i])
            c1, a1 = f(T["c"][i - 1]), P["a"][i - 1]
            d = torch.where(c1 <= 0, a1.expand_as(c1), torch.ones_like(c1))
            G["dz"][i - 1] = dtf * d
            dt = dtf if fused else f(dtf.to(s16))
            T["dz"][i - 1] = (dt * d).to(s16)
            G["da"][i - 1] = torch.where(c1 <= 0, dtf * c1, torch.zeros_like(c1)).reshape(-1, u.cout).sum(0)
            T["da"][i - 1] = torch.where(c1 <= 0, dt * c1, torch.zeros_like(c1)).reshape(-1, u.cout).sum(0)
            daf = dgrad(U[i - 1], T["dz"][i - 1])
            gf = f(g16) + daf
            g16 = g16 if mut == "pending_not_added" else (f(g16) + f(daf.to(s16))).to(s16)
        elif u.kind == "head" and i > 0:
            gf = dgrad(u, T["dz"][i])
            g16 = gf.to(s16)
        dw = K.conv_ref(T["inp"][i], torch.zeros(u.cout, 3, 3, u.cin), u.stride, f32, "cpu", dy=T["dz"][i], want=("dw",), slabs=net.mini_splits)["dw"]
        T["dw"][i] = dw[..., 1:u.cin_real + 1] if (mut == "unpad_shifted" and u.cin_real != u.cin) else dw[..., :u.cin_real]
    return T, G


MUTANTS = ("identity_from_u1", "pending_not_added", "bias_not_in_sign", "dalpha_over_positive", "unpad_shifted", "left_nhwc", "truncated_store")


@pytest.mark.parametrize("s16", S16, ids=("fp16", "bf16"))
def test_miniature_evaluation_within_bounds_and_every_planted_fault_found(s16):
    net = SC.Net(0, 2, mini=MINI)
    assert [u.kind for u in net.units] == ["head", "u1", "u2", "head"] and net.units[0].cin == 64 and net.units[0].cin_real == 3
    assert [u.idx for u in net.captured()] == [3, 2, 0]
    P = mini_inputs(net, s16)
    names = None
    for fused in (True, False):
        net.mini_fused = fused
        T, G = evaluate(net, P, s16, fused)
        # ("... vs stored dz" has the stored, rounded dz in its REFERENCE: it is held to its whole bound below, like every stored quantity)
        pre = {k: v for k, v in SC.compare(net, T, s16, "cpu", got=G) if "vs stored" not in k}
        worst = max(pre.items(), key=lambda kv: kv[1])
        assert worst[1] <= 0.25, ("before the final store", fused, worst)
        stored = dict(SC.compare(net, T, s16, "cpu"))
        worst = max(stored.items(), key=lambda kv: kv[1])
        assert worst[1] <= 1.0, ("as stored", fused, worst)
        names = sorted(stored)
    # every tensor of every unit is among the comparisons
    for i in range(4):
        assert {"c[%d]" % i, "t[%d]" % i, "dz[%d]" % i, "weight grad[%d]" % i, "prelu grad[%d]" % i} <= set(names)
    assert {"xin", "feats", "fc.bias grad", "fc.weight grad", "cap[3] (fc dx)", "cap[2]", "cap[0]", "bias grad[0]", "bias grad[3]"} <= set(names)
    net.mini_fused = False
    for mut in MUTANTS:
        T, _ = evaluate(net, P, s16, False, mut)
        out = dict(SC.compare(net, T, s16, "cpu"))
        over = sorted(k for k, v in out.items() if v > 1.0)
        assert over, "planted fault not found: " + mut
        print("%-22s -> %s" % (mut, ", ".join(over)))


def test_unit_table():
    for type_, n in ((20, 20), (64, 62)):        # 4 stage heads + 2 units per block (8 / 29 blocks)
        net = SC.Net(type_, 8)
        assert len(net.units) == n
        assert [u.hout for u in net.units if u.kind == "head"] == [56, 28, 14, 7]
        assert all((u.ident == u.idx - 1) == (u.kind == "u2") for u in net.units)
        assert all(u.bias == (u.kind == "head") for u in net.units)
        assert net.tensor_names()[0] == ("layer1.0.weight", (64, 3, 3, 3)) and net.tensor_names()[-2] == ("fc.weight", (512, 25088))
    assert [n for n, _ in SC.Net(20, 8).tensor_names()][3:7] == ["layer1.2.conv1.weight", "layer1.2.prelu1.weight", "layer1.2.conv2.weight", "layer1.2.prelu2.weight"]


def slots(net):
    return ([net.fwd_slot(u) for u in net.units], [net.dgrad_slot(u) for u in net.units], [net.wgrad_slot_splits(u) for u in net.units],
            [int(net.dgrad_prelu_ok(u)) for u in net.units if u.kind == "u2"])


def test_case_batches_and_slot_tables_are_these_literals():
    """28x28 / 128 channels: ceil(63 * 784 / 128) = 386 >= 384 tiles (380 at 62); 14x14 / 256: ceil(125 * 196 / 128) * 2 = 384 (380 at 124)"""
    assert SC.first_fused_batch(20, 1) == 63 and SC.first_fused_batch(20, 2) == 125
    assert not any(SC.Net(20, 62).dgrad_prelu_ok(u) for u in SC.Net(20, 62).units if u.kind == "u2")
    assert SC.first_fused_batch(20, 0) is None and SC.first_fused_batch(20, 3) is None       # 64 channels; a 7x7 map
    assert SC.case_batches() == [(20, 1), (20, 5), (20, 63), (20, 125), (20, 128), (64, 64)]
    # sphere20 unit order: head1 b | head2 b b | head3 b b b b | head4 b
    fwd, dg, wg, fu = slots(SC.Net(20, 1))
    assert fwd == [3, 15, 15, 2, 17, 17, 17, 17, 17, 17, 17, 17, 17, 17, 17, 17, 17, 17, 17, 17]
    assert dg == [None, 15, 15, 3, 17, 17, 17, 17, 2, 17, 17, 17, 17, 17, 17, 17, 17, 2, 17, 17]
    assert fu == [0] * 8
    fwd5, dg5, wg5, fu5 = slots(SC.Net(20, 5))
    assert (fwd5, dg5, fu5) == (fwd, dg, fu)
    assert [s for s, _ in wg] == [s for s, _ in wg5] == [6, 16, 16, 4, 16, 16, 16, 16, 14, 16, 16, 16, 16, 16, 16, 16, 16, 14, 14, 14]
    fwd, dg, wg, fu = slots(SC.Net(20, 63))
    assert fwd == [1, 15, 15, 0, 13, 13, 13, 13, 17, 17, 17, 17, 17, 17, 17, 17, 17, 17, 17, 17]
    assert dg == [None, 15, 15, 1, 13, 13, 13, 13, 2, 17, 17, 17, 17, 17, 17, 17, 17, 2, 17, 17]
    assert fu == [0, 1, 1, 0, 0, 0, 0, 0]
    for B in (125, 128):
        fwd, dg, wg, fu = slots(SC.Net(20, B))
        assert fwd == [1, 15, 15, 0, 13, 13, 13, 13, 17, 12, 12, 12, 12, 12, 12, 12, 12, 17, 17, 17]
        assert dg == [None, 15, 15, 1, 13, 13, 13, 13, 2, 12, 12, 12, 12, 12, 12, 12, 12, 2, 17, 17]
        assert fu == [0, 1, 1, 1, 1, 1, 1, 0]
    n64 = SC.Net(64, 64)
    fwd, dg, wg, fu = slots(n64)
    assert fu == [0] * 3 + [1] * 7 + [0] * 16 + [0] * 3
    assert [sp for _, sp in wg[23:55]] == [8] * 32           # the 14x14 stage: 8 slabs per layer, summed by the next paired launch
    assert n64.forward_counts() == {1: 1, 15: 6, 0: 1, 13: 14, 17: 40, 2: 1}
    assert n64.backward_counts()[0] == {4: 2, 6: 2, 15: 6, 16: 26, 1: 1, 13: 14, 2: 2, 14: 8, 17: 38}
    assert n64.backward_counts()[1:] == (7, 26)             # the fused epilogue serves the 28x28 blocks; the paired kernel all but the three 7x7 blocks
    assert SC.Net(20, 128).forward_counts() == {1: 1, 15: 2, 0: 1, 13: 4, 17: 4, 12: 8, 2: 1}
    assert SC.Net(20, 128).backward_counts() == ({4: 3, 6: 1, 15: 2, 16: 7, 1: 1, 13: 4, 2: 2, 14: 4, 12: 8, 17: 2}, 6, 7)
    assert SC.Net(20, 63).backward_counts() == ({4: 2, 6: 2, 15: 2, 16: 7, 1: 1, 13: 4, 2: 2, 14: 4, 17: 10}, 2, 7)
    assert SC.Net(20, 1).forward_counts() == SC.Net(20, 5).forward_counts() == {3: 1, 15: 2, 2: 2, 17: 16}
    assert SC.Net(20, 1).backward_counts()[0] == SC.Net(20, 5).backward_counts()[0] == {4: 2, 6: 2, 15: 2, 16: 7, 3: 1, 17: 14, 2: 2, 14: 4}
    assert SC.Net(20, 5).backward_counts()[1:] == (0, 7)
