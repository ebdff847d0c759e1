"""The fused BottleBlock kernels (csrc/bottle.hip) through the C ABI on raw pointers, against the fp64 formula of tests/bottle_cases.py.
Shapes: one row, a partial row tile, more than one 64-row tile with a ragged tail, and batch sums that cross the weight-gradient tiles'
k-step of 32 (B = 130, 257).  Every output is NaN-filled before the call; tolerances and the kink rule are those of bottle_cases.py."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

import bottle_cases as bc  # noqa: E402
from bottle_cases import f32  # noqa: E402

from fedfr_amd import _C  # noqa: E402

DEV = torch.device("cuda:0")
NAN = float("nan")


def _ptrs(ts):
    return (ctypes.c_void_p * bc.N_PARAMS)(*[t.data_ptr() for t in ts])


def run(c, want_dx=True):
    """forward + backward of case ``c`` through the C ABI -> {"y", "h1", "h2", "dx" (None without), "grads"} on the host"""
    lib = _C.lib()
    B, D = c.B, c.D
    x, dy = c.x.to(DEV), c.dy.to(DEV)
    params = [p.to(DEV) for p in c.params]
    h1, h2, y, dx = (torch.full((B, D), NAN, dtype=f32, device=DEV) for _ in range(4))
    grads = [torch.full_like(p, NAN) for p in params]
    st = _C.stream()
    _C.check(lib.fedfr_bottle_forward(x.data_ptr(), _ptrs(params), B, D, h1.data_ptr(), h2.data_ptr(), y.data_ptr(), st), "bottle_forward")
    nbytes = lib.fedfr_bottle_workspace_bytes(B, D)
    assert nbytes > 0
    ws = torch.full((nbytes // 4,), NAN, dtype=f32, device=DEV)
    _C.check(lib.fedfr_bottle_backward(x.data_ptr(), _ptrs(params), h1.data_ptr(), h2.data_ptr(), dy.data_ptr(), B, D,
                                       dx.data_ptr() if want_dx else None, _ptrs(grads), ws.data_ptr(), nbytes, st), "bottle_backward")
    torch.cuda.synchronize()
    return {"y": y.cpu(), "h1": h1.cpu(), "h2": h2.cpu(), "dx": dx.cpu() if want_dx else None, "grads": [g.cpu() for g in grads]}


@pytest.mark.parametrize("B,D", bc.SHAPES)
def test_forward_and_backward_vs_fp64(B, D):
    c = bc.case(B, D)
    out = []
    try:
        c.check(run(c), out=out)
    finally:
        for what, kind, worst in out:
            print("%-40s %-4s %.3g" % (what, kind, worst))


@pytest.mark.parametrize("B,D", [(2, 64), (130, 512)])
def test_null_dx_and_a_second_run_give_the_same_bits(B, D):
    c = bc.case(B, D)
    a, b, n = run(c), run(c), run(c, want_dx=False)
    for k in ("y", "h1", "h2", "dx"):
        assert torch.equal(a[k], b[k]), k
    for i in range(bc.N_PARAMS):
        assert torch.equal(a["grads"][i], b["grads"][i]), ("second run", bc.PARAM_KEYS[i])
        assert torch.equal(a["grads"][i], n["grads"][i]), ("dx = null", bc.PARAM_KEYS[i])


def test_unsupported_shapes_return_an_error_string():
    lib = _C.lib()
    t = torch.zeros(4096, dtype=f32, device=DEV)
    p = _ptrs([t] * bc.N_PARAMS)
    for B, D in ((4, 96), (4, 32), (4, 576), (0, 64)):
        assert lib.fedfr_bottle_workspace_bytes(B, D) == 0
        assert lib.fedfr_bottle_forward(t.data_ptr(), p, B, D, t.data_ptr(), t.data_ptr(), t.data_ptr(), _C.stream()) < 0
        assert b"bottle_forward" in lib.fedfr_last_error_string() and str(D).encode() in lib.fedfr_last_error_string()
        assert lib.fedfr_bottle_backward(t.data_ptr(), p, t.data_ptr(), t.data_ptr(), t.data_ptr(), B, D, None, p, t.data_ptr(), 1 << 20,
                                         _C.stream()) < 0
        assert b"bottle_backward" in lib.fedfr_last_error_string()
    # a workspace that is too small is refused before anything is launched
    assert lib.fedfr_bottle_backward(t.data_ptr(), p, t.data_ptr(), t.data_ptr(), t.data_ptr(), 4, 64, None, p, t.data_ptr(), 16, _C.stream()) < 0
    assert b"workspace" in lib.fedfr_last_error_string()
    torch.cuda.synchronize()
