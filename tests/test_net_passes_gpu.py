"""The C ABI entry of a fused BatchNorm-backward pass and the plan run the SAME function (csrc/ew.h: ew_bn_bwd_sliced / ew_bn_bwd_rowslab), so
fed with the plan's own tensors the entry must give the plan's bits.  A lone-block plan (fedfr_block_create) runs one training forward + backward
with fedfr_net_debug_capture at detail level 1; the entry then gets the captured gradient g entering the block, the block's c2 (fedfr_net_act_info),
bn3's saved rows (fedfr_net_bn_info) and gamma / beta from the tensor table, and its dx / dgamma / dbeta are compared BITWISE with the captured dc2
and the plan's gradient buffer (neither form uses floating-point atomics).  Two cases, the smallest that take each form; the fedfr_bn_sliced_ok
value that selects the form is asserted first, so a moved threshold fails here instead of testing one form twice."""
import ctypes as C

import pytest
import torch

from fedfr_amd import _C
from plan_harness import Guarded, act_info, dev, query, tensor_table

pytestmark = pytest.mark.gpu
f32 = torch.float32


@pytest.mark.parametrize("cin,cout,stride,hin,B,sliced", [(256, 256, 1, 14, 2, 1), (512, 512, 1, 7, 2, 0)], ids=["sliced-256x14", "rowslab-512x7"])
def test_bn3_backward_entry_gives_the_plans_bits(cin, cout, stride, hin, B, sliced):
    lib, s16 = _C.lib(), _C.storage_dtype()
    M, Cc = B * (hin // stride) ** 2, cout
    assert lib.fedfr_bn_sliced_ok(M, Cc, lib.fedfr_bn_sliced_rows(M, Cc, 1), 1) == sliced
    h = lib.fedfr_block_create(cin, cout, stride, hin, B)
    assert h
    try:
        table = {n: (s, o) for n, s, o, _ in tensor_table(h)}
        gen = torch.Generator().manual_seed(7)
        params = torch.zeros(query(h, _C.Q_PARAM_COUNT), dtype=f32)
        bufs = torch.zeros(query(h, _C.Q_BUFFER_COUNT), dtype=f32)
        for name, (shape, off) in table.items():
            n = 1
            for d in shape:
                n *= d
            if name.endswith("conv1.weight") or name.endswith("conv2.weight"):
                params[off:off + n] = torch.randn(n, generator=gen) * (2.0 / (9 * shape[1])) ** 0.5
            elif name.endswith("prelu.weight"):
                params[off:off + n] = 0.25
            elif name.endswith(".weight"):
                params[off:off + n] = 1.0 + 0.2 * torch.randn(n, generator=gen)
            elif name.endswith(".bias"):
                params[off:off + n] = 0.1 * torch.randn(n, generator=gen)
            elif name.endswith("running_var"):
                bufs[off:off + n] = 1.0
        params, bufs = params.to(dev()), bufs.to(dev())
        x = torch.randn(B, cin, hin, hin, generator=gen).to(dev())
        dy = torch.randn(B, cout, hin // stride, hin // stride, generator=gen).to(dev())
        shadow = torch.zeros(query(h, _C.Q_SHADOW_COUNT), dtype=s16, device=dev())
        act, ws = Guarded(query(h, _C.Q_ACT_BYTES)), Guarded(query(h, _C.Q_WS_BYTES))
        grads = torch.zeros(query(h, _C.Q_PARAM_COUNT), dtype=f32, device=dev())
        elems = C.c_longlong()
        _C.call("fedfr_net_debug_capture_elems", h, 1, C.byref(elems))
        cap = torch.zeros(elems.value, dtype=s16, device=dev())
        st = _C.stream()
        _C.call("fedfr_net_prepare_weights", h, params.data_ptr(), shadow.data_ptr(), 1, st)
        _C.call("fedfr_net_forward", h, x.data_ptr(), params.data_ptr(), bufs.data_ptr(), shadow.data_ptr(), act.ptr(), ws.ptr(), None, 1, st)
        _C.call("fedfr_net_debug_capture_detail", 1)
        _C.call("fedfr_net_debug_capture", cap.data_ptr(), cap.numel())
        _C.call("fedfr_net_backward2", h, None, dy.data_ptr(), params.data_ptr(), shadow.data_ptr(), act.ptr(), ws.ptr(), grads.data_ptr(), st, None)
        torch.cuda.synchronize()
        assert act.guard_ok() and ws.guard_ok()
        # ---- the plan's own tensors: level 1 opens a block with g, dc2; bn3 is the block's third BatchNorm
        g, dc2 = cap[:M * Cc], cap[M * Cc:2 * M * Cc]
        off, rows, ch = act_info(h, 0, 4)
        assert (rows, ch) == (M, Cc)
        c2 = act.view(s16)[off:off + M * Cc]
        name, c, so = C.create_string_buffer(64), C.c_int(), C.c_longlong()
        _C.call("fedfr_net_bn_info", h, 2, name, 64, C.byref(c), C.byref(so))
        assert (name.value, c.value) == (b"bn3", Cc)
        save = act.view(torch.uint8)[query(h, _C.Q_ACT_FLOAT_OFF_BYTES):].view(f32)[so.value:so.value + 4 * Cc].view(4, Cc)      # scale, shift, mean, rstd
        go, bo = table["bn3.weight"][1], table["bn3.bias"][1]
        gamma, beta = params[go:go + Cc], params[bo:bo + Cc]
        # ---- the entry, rows_in = 0, no addend, no next BatchNorm, count = M, into the test's own buffers
        dx = torch.zeros(M * Cc, dtype=s16, device=dev())
        dgamma, dbeta = torch.zeros(Cc, dtype=f32, device=dev()), torch.zeros(Cc, dtype=f32, device=dev())
        p = lambda t: t.data_ptr()  # noqa: E731
        if sliced:
            part = torch.zeros(lib.fedfr_bn_sliced_rows(M, Cc, 1) * 3 * Cc, dtype=f32, device=dev())
            _C.call("fedfr_bn_bwd_sliced", p(g), p(c2), p(save[2]), p(save[3]), p(gamma), None, p(save[0]), p(save[1]), M, Cc, p(part), 0, p(dgamma),
                    p(dbeta), None, None, p(dx), None, None, None, None, st)
        else:
            part = torch.zeros(lib.fedfr_bn_bwd_rows(M, Cc) * 3 * Cc, dtype=f32, device=dev())
            coef = torch.zeros(3 * Cc, dtype=f32, device=dev())
            _C.call("fedfr_bn_bwd_rowslab", p(g), p(c2), p(save[2]), p(save[3]), p(gamma), p(beta), None, p(save[0]), p(save[1]), M, Cc, float(M),
                    p(part), 0, 0, p(coef), p(dgamma), p(dbeta), None, None, None, 0, p(dx), None, None, None, None, None, None, None, st)
        torch.cuda.synchronize()
        assert float(dc2.float().abs().max()) > 0 and float(grads[go:go + Cc].abs().max()) > 0      # the plan wrote something to compare with
        assert torch.equal(dx.view(torch.int16), dc2.view(torch.int16)), "dx differs from the plan's dc2"
        assert torch.equal(dgamma.view(torch.int32), grads[go:go + Cc].view(torch.int32)), "dgamma differs from the plan's"
        assert torch.equal(dbeta.view(torch.int32), grads[bo:bo + Cc].view(torch.int32)), "dbeta differs from the plan's"
    finally:
        _C.call("fedfr_net_debug_capture", None, 0)
        _C.call("fedfr_net_debug_capture_detail", 0)
        lib.fedfr_net_destroy(h)
