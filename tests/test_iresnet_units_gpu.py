"""The iresnet plan (csrc/net.hip: net_forward with training = 1, net_backward) block by block against float64, through the raw C ABI:
fedfr_net_create(layers4, B, 112, 512), fedfr_net_prepare_weights, fedfr_net_forward, fedfr_net_backward2 on the test's own parameter, buffer,
shadow, arena, workspace, gradient and capture buffers, with fedfr_net_debug_capture at detail level 1 and fedfr_net_bn_info for the saved rows.

The cases (tests/iresnet_cases.py case_batches, every batch but 1, 5 and 128 computed from the restated thresholds): iresnet18 at a one-image plan
(Bp = 8 padding, single-split paired weight gradients, row-slab BatchNorm at 14x14), a ragged batch, the first batch with the 56x56 64 <-> 128 convs on
the LDS-DMA kernel and the odd batch behind it, the last batch whose 56x56 BatchNorms run channel-sliced, the first batch with the 28x28 convs on the
LDS-DMA kernels (odd: one tile per workgroup) and the even one behind it (two tiles, fuse_bnbwd28), the first batch with the 14x14 convs on them
(fused BatchNorm-backward epilogue, fwd_xmom), the bench batch; and a (1, 1, 3, 1) net — consecutive identity blocks at 14x14 — at the first batch at
which a paired weight-gradient launch CARRIES the previous pair's slab sums and at the first 14x14 LDS-DMA batch (fwd_xmom and fuse_bnred_next between
identity blocks).  Per case:
  * every comparison of iresnet_cases.compare stays <= 1 (every element, every reference float64 and fed with the run's own stored operands);
  * the profile counters of the forward and of the backward pass equal forward_counts() / backward_counts(), BatchNorm launches included;
  * the guard bands behind shadow, arena, workspace, gradient, capture, buffer and feats buffers stay untouched; arena and workspace start from a
    large finite sentinel and a second run from another sentinel gives the same bits in every output and every inspected tensor;
  * capture level 0 and level 1, and single-stream and dual-stream backward, give the same bits in every gradient;
  * on the (1, 1, 3, 1) cases wgrad9p_bg = 0 gives bit-identical gradients and the counters show two stand-alone reductions more per carry;
  * on the first case in which it changes the launch sequence (iresnet_cases.pair_reduce_case: the 7x7 identity block's weight gradients run
    split-K), wgrad_pair_reduce = 0 — two reduction launches for its two slab sets instead of one — and ALL of compare is run again on that state:
    every comparison stays <= 1.
The profile counters cover the GEMM slots, the BatchNorm apply / reduce / finalize slots (20 - 24: a fused pass that quietly fell back to separate
ones would show) and the slab reductions (25).  At B = 1 BatchNorm1d's backward is exactly zero, so that case holds the backward pass's launches and
bits, not its values.  The float64 references run on the GPU through torch.matmul, block by block."""
import ctypes as C
import functools
import re
import time

import pytest
import torch

import iresnet_cases as IC
from fedfr_amd import _C
from oracle import ref_cpu as R
from plan_harness import CUS, SENTINELS, Guarded, act_info, dev, query, slot_counts, tensor_table

pytestmark = pytest.mark.gpu
f32 = torch.float32
F = 512
CAP_KEYS = ("g", "dc2", "da2", "dc1", "dd", "dxd", "da1")


@functools.lru_cache(maxsize=2)
def state(layers):
    return R.closed_form_state_dict(layers, tag=1.0)


def bn_info(h):
    out = []
    for i in range(query(h, _C.Q_NUM_BN)):
        name, c, off = C.create_string_buffer(64), C.c_int(), C.c_longlong()
        _C.call("fedfr_net_bn_info", h, i, name, 64, C.byref(c), C.byref(off))
        out.append((name.value.decode(), c.value, off.value))
    return out


@pytest.mark.parametrize("layers,B", IC.case_batches(), ids=lambda v: "".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_iresnet_plan_block_by_block(layers, B):
    t0 = time.time()
    s16 = _C.storage_dtype()
    net = IC.Net(layers, B, cus=CUS)
    h = _C.lib().fedfr_net_create((C.c_int * 4)(*layers), B, 112, F)
    assert h
    try:
        run_case(net, h, s16, 256.0 if s16 == torch.float16 else 1.0, t0)
    finally:
        _C.call("fedfr_net_debug_capture", None, 0)
        _C.call("fedfr_net_debug_capture_detail", 0)
        _C.call("fedfr_profile_enable", 0)
        _C.lib().fedfr_net_destroy(h)


def run_case(net, h, s16, scale, t0):
    B, blocks = net.B, net.blocks
    # ---- the block table against the plan's own inventory
    table = tensor_table(h)
    assert [(n, s) for n, s, _, _ in table] == net.tensor_names()
    bns = bn_info(h)
    assert [(n, c) for n, c, _ in bns] == net.bn_table()
    ntrain, nparam, nbuf = query(h, _C.Q_TRAINABLE_COUNT), query(h, _C.Q_PARAM_COUNT), query(h, _C.Q_BUFFER_COUNT)
    assert query(h, _C.Q_FC_IN) == net.fc_in
    # ---- buffers
    sd = state(net.layers4)
    params, bufs0 = torch.zeros(nparam, dtype=f32), torch.zeros(nbuf, dtype=f32)
    for name, shape, off, region in table:
        if region == 2:
            continue
        v = sd[name]
        (params if region == 0 else bufs0)[off:off + v.numel()] = (v.permute(0, 2, 3, 1) if v.dim() == 4 else v).reshape(-1)      # conv weights KRSC
    params, bufs0 = params.to(dev()), bufs0.to(dev())
    bufs = Guarded(nbuf * 4)
    shadow = Guarded(query(h, _C.Q_SHADOW_COUNT) * 2)
    shadow.view(torch.uint8).zero_()
    act, ws, grads, feats = Guarded(query(h, _C.Q_ACT_BYTES)), Guarded(query(h, _C.Q_WS_BYTES)), Guarded(ntrain * 4), Guarded(B * F * 4)
    elems = [C.c_longlong(), C.c_longlong()]
    for lv in (0, 1):
        _C.call("fedfr_net_debug_capture_elems", h, lv, C.byref(elems[lv]))
    cap = Guarded(elems[1].value * 2)
    x = R.closed_form_images(B, tag=4.0).to(dev())
    dfe = (R.closed_form((B, F), 0.37, 0.9, 1.0) * scale).to(dev())
    A16, W16, G32, CAP16, BUF32 = act.view(s16), ws.view(s16), grads.view(f32), cap.view(s16), bufs.view(f32)
    foff = query(h, _C.Q_ACT_FLOAT_OFF_BYTES)
    AF = act.view(torch.uint8)[foff:].view(f32)
    # ---- where everything lives
    offs = {n: (o, s, r) for n, s, o, r in table}

    def par_view(src, name):
        o, shape, _ = offs[name]
        n = 1
        for d in shape:
            n *= d
        v = src[o:o + n]
        return v.view(shape[0], shape[2], shape[3], shape[1]) if len(shape) == 4 else v.view(shape)

    def a16(which_block, which, shape):
        off, rows, ch = act_info(h, which_block, which)
        n = 1
        for d in shape:
            n *= d
        assert rows * ch == n, (which_block, which, rows, ch, shape)
        return A16[off:off + n].view(shape)
    T = dict(x=x, par={}, grad={}, buf0={}, buf={}, save={}, blk=[], cap=[None] * len(blocks))
    for name, shape, off, region in table:
        if region == 0:
            T["par"][name] = par_view(params, name)
            if off < ntrain:
                T["grad"][name] = par_view(G32, name)
    for name, ch, so in bns:
        rm, rv = offs[name + ".running_mean"][0], offs[name + ".running_var"][0]
        T["buf0"][name] = (bufs0[rm:rm + ch].clone(), bufs0[rv:rv + ch].clone())
        T["buf"][name] = (BUF32[rm:rm + ch], BUF32[rv:rv + ch])
        T["save"][name] = AF[so:so + 4 * ch].view(4, ch)
    T["c0"], T["a0"] = a16(-1, 0, (B, 112, 112, 64)), a16(-1, 1, (B, 112, 112, 64))
    T["t"] = a16(-1, 2, (B, net.fc_in))
    yo = bns[-1][2] + 4 * bns[-1][1] + 4 * F                 # behind the features' BatchNorm1d rows (include/fedfr_hip.h, fedfr_net_bn_info)
    T["yfc"] = AF[yo:yo + B * F].view(B, F)
    T["fsave"] = AF[yo + B * F:yo + B * F + 2 * F].view(2, F)
    T["feats"], T["dfeats"] = feats.view(f32).view(B, F), dfe
    rm, rv = offs["features.running_mean"][0], offs["features.running_var"][0]
    T["buf0"]["features"], T["buf"]["features"] = (bufs0[rm:rm + F].clone(), bufs0[rv:rv + F].clone()), (BUF32[rm:rm + F], BUF32[rv:rv + F])
    for b in blocks:
        si, so_ = (B, b.hin, b.hin), (B, b.hout, b.hout)
        t = dict(x=a16(b.idx, 0, si + (b.cin,)), a1=a16(b.idx, 1, si + (b.cin,)), c1=a16(b.idx, 2, si + (b.cout,)), a2=a16(b.idx, 3, si + (b.cout,)),
                 c2=a16(b.idx, 4, so_ + (b.cout,)), out=a16(b.idx, 6, so_ + (b.cout,)))
        if b.has_ds:
            t["d"] = a16(b.idx, 5, so_ + (b.cout,))
        T["blk"].append(t)
    Mf = B * net.hw
    T["gt"] = CAP16[:Mf * net.C].view(Mf, net.C)            # level 1 opens with the gradient wrt the network's bn2 output
    o, g_at = Mf * net.C, {}
    for b in reversed(blocks):
        g_at[b.idx] = o
        si, so_ = (B, b.hin, b.hin), (B, b.hout, b.hout)
        shapes = dict(g=so_ + (b.cout,), dc2=so_ + (b.cout,), da2=si + (b.cout,), dc1=si + (b.cout,), dd=so_ + (b.cout,), dxd=so_ + (b.cin,), da1=si + (b.cin,))
        c = {}
        for k in CAP_KEYS:
            if k in ("dd", "dxd") and not b.has_ds:
                continue
            n = 1
            for d in shapes[k]:
                n *= d
            c[k] = CAP16[o:o + n].view(shapes[k])
            o += n
        T["cap"][b.idx] = c
    T["gin0"] = CAP16[o:o + B * 112 * 112 * 64].view(B, 112, 112, 64)
    g_at[-1] = o
    assert o + B * 112 * 112 * 64 == elems[1].value
    inspected = [T["c0"], T["a0"], T["t"], T["yfc"], feats.view(f32), G32, BUF32, AF[:bns[-1][2] + 4 * bns[-1][1]]] + [v for t in T["blk"] for v in t.values()]

    def run(sentinel, aux, level=1):
        """one training forward + backward from a sentinel-filled arena / workspace; returns the profile counters of the two passes"""
        A16.fill_(sentinel), W16.fill_(sentinel)
        grads.view(torch.uint8).fill_(0x7B), CAP16.fill_(sentinel), feats.view(torch.uint8).fill_(0x7B)
        BUF32.copy_(bufs0)
        st = _C.stream()
        _C.call("fedfr_net_prepare_weights", h, params.data_ptr(), shadow.ptr(), 1, st)
        _C.call("fedfr_profile_enable", 1)
        _C.call("fedfr_net_forward", h, x.data_ptr(), params.data_ptr(), bufs.ptr(), shadow.ptr(), act.ptr(), ws.ptr(), feats.ptr(), 1, st)
        torch.cuda.synchronize()
        fc = slot_counts()
        _C.call("fedfr_profile_enable", 1)
        _C.call("fedfr_net_debug_capture_detail", level)
        _C.call("fedfr_net_debug_capture", cap.ptr(), elems[level].value)
        _C.call("fedfr_net_backward2", h, x.data_ptr(), dfe.data_ptr(), params.data_ptr(), shadow.ptr(), act.ptr(), ws.ptr(), grads.ptr(), st,
                aux.cuda_stream if aux is not None else None)
        torch.cuda.synchronize()
        bc = slot_counts()
        _C.call("fedfr_profile_enable", 0)
        _C.call("fedfr_net_debug_capture", None, 0)
        _C.call("fedfr_net_debug_capture_detail", 0)
        for g, what in ((shadow, "shadow"), (act, "arena"), (ws, "workspace"), (grads, "gradients"), (cap, "capture buffer"), (feats, "feats"), (bufs, "buffers")):
            assert g.guard_ok(), "wrote behind the " + what
        return fc, bc

    counted = lambda c: {s: n for s, n in c.items() if s < 18 or 20 <= s <= 25}  # noqa: E731  (GEMMs, BatchNorm passes and finalizes, slab reductions)
    aux = torch.cuda.Stream()
    fc, bc = run(SENTINELS[0], aux)
    problems = []
    if counted(fc) != net.forward_counts():
        problems.append(("forward launches per profile slot", counted(fc), net.forward_counts()))
    if counted(bc) != net.backward_counts():
        problems.append(("backward launches per profile slot", counted(bc), net.backward_counts()))
    snap = [t.clone() for t in inspected]
    cap_snap = CAP16.clone()
    # ---- another sentinel, the single-stream backward, capture level 0: the same bits everywhere
    for sentinel, a, level, what in ((SENTINELS[1], aux, 1, "a second run from another sentinel"), (SENTINELS[1], None, 1, "the single-stream backward"),
                                     (SENTINELS[0], aux, 0, "capture level 0")):
        fc2, bc2 = run(sentinel, a, level)
        assert (fc2, bc2) == (fc, bc), what
        for i, (t, s) in enumerate(zip(inspected, snap)):
            assert torch.equal(t, s), "%s changed the bits of inspected tensor %d" % (what, i)
        if level == 1:
            assert torch.equal(CAP16, cap_snap), what + " changed the bits of a captured gradient"
        else:                                               # level 0: the gradient entering every block and the one leaving the first, back to back
            o = 0
            for i, n in [(b.idx, T["cap"][b.idx]["g"].numel()) for b in reversed(blocks)] + [(-1, T["gin0"].numel())]:
                assert torch.equal(CAP16[o:o + n], cap_snap[g_at[i]:g_at[i] + n]), "capture level 0: the gradient entering block %d" % i
                o += n
            assert o == elems[0].value
    carries = net.wgrad_walk()[0]
    if net.layers4 == IC.CARRY_LAYERS:
        assert carries, "the case was chosen for its carrying launch"
        with _C.option_scope("wgrad9p_bg", 0):
            _, bc0 = run(SENTINELS[1], aux)
        assert torch.equal(G32, snap[5]), "wgrad9p_bg = 0 changed the bits of a gradient"
        if bc0.get(25, 0) != bc.get(25, 0) + 2 * len(carries) or counted(bc0) != net.backward_counts(bg=False):
            problems.append(("wgrad9p_bg = 0: stand-alone reductions", counted(bc0), net.backward_counts(bg=False)))
    else:
        assert not carries
    fc, bc = run(SENTINELS[0], aux)                          # the state the comparisons read
    del snap, cap_snap
    t1 = time.time()
    worst, n, amb = check_all(net, T, s16, problems)
    want_n = 8 + 8 + 4 + 12 + sum(37 + 12 * b.has_ds for b in blocks)      # stem, bn2 / t / yfc, stem backward, features / fc / bn2 / last g, the blocks
    if n != want_n:
        problems.append(("comparisons", n, want_n))
    print("iresnet%s B=%d: %d comparisons, %d elements with an open PReLU side; setup and plan runs %.1f s, references %.1f s; worst error / bound per "
          "family: %s" % ("".join(map(str, net.layers4)), B, n, amb, t1 - t0, time.time() - t1, ", ".join("%s %.3g" % kv for kv in sorted(worst.items()))))
    if (net.layers4, B) == IC.pair_reduce_case():            # the 7x7 identity block's two slab sets reduced by two launches instead of one
        with _C.option_scope("wgrad_pair_reduce", 0):
            _, bcr = run(SENTINELS[1], aux)
        if counted(bcr) != net.backward_counts(pair_reduce=False):
            problems.append(("wgrad_pair_reduce = 0: launches per profile slot", counted(bcr), net.backward_counts(pair_reduce=False)))
        assert bcr.get(25, 0) > bc.get(25, 0)
        w2, n2, _ = check_all(net, T, s16, problems)         # ALL comparisons again, on the state that run left
        print("    wgrad_pair_reduce = 0: all %d comparisons again, worst %.3g; weight gradients %s" %
              (n2, max(w2.values()), ", ".join("%s %.3g" % kv for kv in sorted(w2.items()) if kv[0].endswith("dw"))))
    assert not problems, problems[:12]


def check_all(net, T, s16, problems):
    """every comparison; returns (worst ratio per family, number of comparisons, elements with an open PReLU side)"""
    fam, n, info = {}, 0, {}
    for what, r in IC.compare(net, T, s16, dev(), info=info):
        n += 1
        k = re.sub(r"^layer\d+\.\d+\.", "", what.split("[")[0])        # layerL.i.bn3 dgamma -> bn3 dgamma
        fam[k] = max(fam.get(k, 0.0), r)
        if not r <= 1.0:
            problems.append((what, r))
    return fam, n, info["ambiguous"]
