"""The sphnet plan (csrc/net_sph.inc) unit by unit against float64, through the raw C ABI: fedfr_net_create_sphere, fedfr_net_query,
fedfr_net_prepare_weights, fedfr_net_forward, fedfr_net_backward2 on the test's own parameter, shadow, arena, workspace, gradient and capture buffers.

Per case (tests/sphnet_cases.py case_batches: sphere20 at a one-image plan, a ragged batch, the two computed thresholds from which the 28x28 and the
14x14 stage run on the LDS-DMA kernels with the fused PReLU-backward epilogue, and the bench batch; sphere64 once, for the long 14x14 stage whose paired
weight-gradient launches carry the previous pair's slab sums):
  * every comparison of sphnet_cases.compare — each unit's conv output, activation, dz, weight / bias / slope gradient, every captured gradient, the
    padded input, the NCHW-flat last activation, feats and the fc gradients — every element, each reference fed with the pass's own stored operands;
  * the profile counters of the forward and of the backward pass equal the per-slot launch counts the restated dispatch rules predict; the streaming
    passes (slot 20 forward, slot 22 backward) show that the fused epilogue took over exactly the PReLU passes it is meant to;
  * guard bands behind the arena, workspace, gradient and capture buffers stay untouched; arena and workspace start from a large FINITE sentinel (a
    halo load of neighbouring memory that is discarded arithmetically is legitimate), and a second run from another sentinel gives the same bits in every
    output and every inspected tensor;
  * single-stream (aux_stream = NULL) and dual-stream backward give the same bits.
The float64 references run on the GPU through torch.matmul, once per case."""
import functools
import time

import pytest
import torch

import sphnet_cases as SC
from fedfr_amd import _C
from oracle import ref_cpu as R
from plan_harness import CUS, SENTINELS, Guarded, act_info, dev, query, slot_counts, tensor_table

pytestmark = pytest.mark.gpu
f32 = torch.float32


@functools.lru_cache(maxsize=2)
def state(type_):
    return R.sphere_state_dict(type_, tag=1.0)


@pytest.mark.parametrize("type_,B", SC.case_batches(), ids=lambda v: str(v))
def test_sphnet_plan_unit_by_unit(type_, B):
    t0 = time.time()
    s16 = _C.storage_dtype()
    scale = 256.0 if s16 == torch.float16 else 1.0
    net = SC.Net(type_, B, cus=CUS)
    h = _C.lib().fedfr_net_create_sphere(type_, B)
    assert h
    try:
        run_case(net, h, s16, scale, t0)
    finally:
        _C.call("fedfr_net_debug_capture", None, 0)
        _C.call("fedfr_profile_enable", 0)
        _C.lib().fedfr_net_destroy(h)


def run_case(net, h, s16, scale, t0):
    type_, B, U = net.type, net.B, net.units
    # ---- the unit table against the plan's own inventory, the row counts against the library's
    table = tensor_table(h)
    assert [(n, s) for n, s, _, _ in table] == net.tensor_names()
    assert all(r == 0 for _, _, _, r in table) and query(h, _C.Q_BUFFER_COUNT) == 0
    offs = {n: o for n, _, o, _ in table}
    ntrain = query(h, _C.Q_TRAINABLE_COUNT)
    assert query(h, _C.Q_PARAM_COUNT) == ntrain and query(h, _C.Q_FC_IN) == net.fc_in
    for u in U:
        assert _C.lib().fedfr_prelu_bwd_rows(B * u.hout * u.hout, u.cout) == net.prelu_rows(u)
    # ---- buffers
    sd = state(type_)
    params = torch.zeros(ntrain, dtype=f32)
    for name, shape, off, _ in table:
        v = sd[name]
        params[off:off + v.numel()] = (v.permute(0, 2, 3, 1) if v.dim() == 4 else v).reshape(-1)      # conv weights KRSC
    params = params.to(dev())
    shadow = Guarded(query(h, _C.Q_SHADOW_COUNT) * 2)
    shadow.view(torch.uint8).zero_()                        # (the alignment gaps between its regions are never written)
    act, ws = Guarded(query(h, _C.Q_ACT_BYTES)), Guarded(query(h, _C.Q_WS_BYTES))
    grads = Guarded(ntrain * 4)
    caps = net.captured()
    cap = Guarded(sum(B * u.hout * u.hout * u.cout for u in caps) * 2)
    x = R.closed_form_images(B, tag=4.0).to(dev())
    dfe = (R.closed_form((B, 512), 0.37, 0.9, 1.0) * scale).to(dev())
    feats = Guarded(B * 512 * 4)
    A16, W16, G32, CAP16 = act.view(s16), ws.view(s16), grads.view(f32), cap.view(s16)
    # ---- where everything lives
    where = {}
    for u in U:
        where[u.idx] = [act_info(h, u.idx, w) for w in range(4)]
        (io, ir, ic), (co, cr, cc), (to, tr, tc), (zo, zr, zc) = where[u.idx]
        assert (ir, ic) == (B * u.hin * u.hin, u.cin) and (cr, cc) == (tr, tc) == (zr, zc) == (B * u.hout * u.hout, u.cout)

    def a16(off, n, shape):
        return A16[off:off + n].view(shape)
    T = dict(x=x, fcw=params[offs["fc.weight"]:offs["fc.weight"] + 512 * net.fc_in].view(512, net.fc_in), fcb=params[offs["fc.bias"]:offs["fc.bias"] + 512],
             feats=feats.view(f32).view(B, 512), dfeats=dfe, w=[], b=[], a=[], inp=[], c=[], t=[], dz=[], dw=[], db=[], da=[], cap={})
    T["dfcw"], T["dfcb"] = G32[offs["fc.weight"]:offs["fc.weight"] + 512 * net.fc_in].view(512, net.fc_in), G32[offs["fc.bias"]:offs["fc.bias"] + 512]
    T["xin"] = a16(where[0][0][0], B * 112 * 112 * 64, (B, 112, 112, 64))
    for u in U:
        (io, ir, ic), (co, cr, cc), (to, _, _), (zo, _, _) = where[u.idx]
        wn, nw = u.conv + ".weight", u.cout * 9 * u.cin_real
        pa = offs[u.prelu + ".weight"]
        for key, src in (("w", params), ("dw", G32)):
            T[key].append(src[offs[wn]:offs[wn] + nw].view(u.cout, 3, 3, u.cin_real))
        for key, src in (("b", params), ("db", G32)):
            T[key].append(src[offs[u.conv + ".bias"]:offs[u.conv + ".bias"] + u.cout] if u.bias else None)
        for key, src in (("a", params), ("da", G32)):
            T[key].append(src[pa:pa + u.cout])
        T["inp"].append(a16(io, ir * ic, (B, u.hin, u.hin, u.cin)))
        T["c"].append(a16(co, cr * cc, (B, u.hout, u.hout, u.cout)))
        T["t"].append(a16(to, cr * cc, (B, net.fc_in) if u is U[-1] else (B, u.hout, u.hout, u.cout)))      # the last unit's t is stored NCHW-flat
        T["dz"].append(W16[zo:zo + cr * cc].view(B, u.hout, u.hout, u.cout))
    o = 0
    for u in caps:
        n = B * u.hout * u.hout * u.cout
        T["cap"][u.idx] = CAP16[o:o + n].view(B, u.hout, u.hout, u.cout)
        o += n
    inspected = [T["xin"], T["feats"], G32] + T["c"] + T["t"] + T["dz"] + [CAP16]

    def run(sentinel, aux):
        """one forward + backward from a sentinel-filled arena / workspace; returns the profile counters of the two passes"""
        A16.fill_(sentinel), W16.fill_(sentinel)
        grads.view(torch.uint8).fill_(0x7B), CAP16.fill_(sentinel), feats.view(torch.uint8).fill_(0x7B)
        st = _C.stream()
        _C.call("fedfr_net_prepare_weights", h, params.data_ptr(), shadow.ptr(), 1, st)
        _C.call("fedfr_profile_enable", 1)
        _C.call("fedfr_net_forward", h, x.data_ptr(), params.data_ptr(), None, shadow.ptr(), act.ptr(), ws.ptr(), feats.ptr(), 1, st)
        torch.cuda.synchronize()
        fc = slot_counts()
        _C.call("fedfr_profile_enable", 1)
        _C.call("fedfr_net_debug_capture", cap.ptr(), cap.n // 2)
        _C.call("fedfr_net_backward2", h, x.data_ptr(), dfe.data_ptr(), params.data_ptr(), shadow.ptr(), act.ptr(), ws.ptr(), grads.ptr(), st,
                aux.cuda_stream if aux is not None else None)
        torch.cuda.synchronize()
        bc = slot_counts()
        _C.call("fedfr_profile_enable", 0)
        _C.call("fedfr_net_debug_capture", None, 0)
        for g, what in ((shadow, "shadow"), (act, "arena"), (ws, "workspace"), (grads, "gradients"), (cap, "capture buffer"), (feats, "feats")):
            assert g.guard_ok(), "wrote behind the " + what
        return fc, bc

    aux = torch.cuda.Stream()
    fc, bc = run(SENTINELS[0], aux)
    # ---- which kernels served the passes
    want_b, fused, paired = net.backward_counts()
    gemm = lambda c: {s: n for s, n in c.items() if s < 18}  # noqa: E731
    assert gemm(fc) == net.forward_counts(), ("forward launches per profile slot", gemm(fc), net.forward_counts())
    assert gemm(bc) == want_b, ("backward launches per profile slot", gemm(bc), want_b)
    nblocks = sum(u.kind == "u2" for u in U)
    assert fc.get(20) == len(U), fc                          # one streaming activation pass per unit
    assert bc.get(22) == len(U) - fused, (bc, fused)         # one PReLU-backward pass per unit, but for the u1 the dgrad epilogue served
    assert fused == sum(net.dgrad_prelu_ok(u) for u in U if u.kind == "u2") and paired == sum(net.pair_ok(u) for u in U if u.kind == "u2") <= nblocks
    snap = [t.clone() for t in inspected]
    # ---- another sentinel, then single-stream: the same bits everywhere
    for sentinel, a, what in ((SENTINELS[1], aux, "a second run from another sentinel"), (SENTINELS[1], None, "the single-stream backward")):
        fc2, bc2 = run(sentinel, a)
        assert (fc2, bc2) == (fc, bc), what
        for i, (t, s) in enumerate(zip(inspected, snap)):
            assert torch.equal(t, s), "%s changed the bits of inspected tensor %d" % (what, i)
    del snap
    t1 = time.time()
    # ---- every comparison, every element
    fam, bad, n = {}, [], 0
    for what, r in SC.compare(net, T, s16, dev()):
        n += 1
        k = what.split("[")[0].split(" (")[0]
        fam[k] = max(fam.get(k, 0.0), r)
        if not r <= 1.0:
            bad.append((what, r))
    # per unit c, t, dz, weight and slope gradient; xin, feats, the fc's two gradients; every captured gradient; two bias comparisons per stage head
    assert n == 5 * len(U) + 4 + len(caps) + 2 * 4, n
    print("sphere%d B=%d: %d comparisons; setup and plan runs %.1f s, references %.1f s; worst error / bound per family: %s" %
          (type_, B, n, t1 - t0, time.time() - t1, ", ".join("%s %.3g" % kv for kv in sorted(fam.items()))))
    assert not bad, ("error / bound", bad[:12], len(bad))
