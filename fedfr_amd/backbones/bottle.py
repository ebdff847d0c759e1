"""BottleBlock: the four-branch bottleneck MLP with a residual that the personalised head uses as its converter when
``converter_layer != 1`` (reference backbones/bottle.py:11-47, client.py:35-36).

    h1_g = leaky(x W1_g^T + b1_g)      g = 0..3, W1_g [H, D], H = D / bottle_rate
    h2_g = leaky(h1_g W2_g^T + b2_g)   W2_g [H, H]
    y    = x + [h2_0 | h2_1 | h2_2 | h2_3] W3^T + b3

Forward and backward each run as two fused HIP launches (csrc/bottle.hip) behind one ``torch.autograd.Function``; there is no
eager path.  The state-dict keys are the reference's: ``br{1..4}.{0,2}.{weight,bias}`` and ``concat_fc.{weight,bias}`` (the
reference's branches are ``nn.Sequential(Linear, LeakyReLU, Linear, LeakyReLU)``: entries 0 and 2 own parameters)."""
from __future__ import annotations

import ctypes

import torch
import torch.nn as nn

from .. import _C

f32 = torch.float32
N_PARAMS = 18       # br1..br4 x (first weight, first bias, second weight, second bias), concat_fc weight and bias: the C ABI's order


def _pointers(tensors):
    return (ctypes.c_void_p * N_PARAMS)(*[t.data_ptr() for t in tensors])


def _gpu(t, name):
    t = t.detach()
    return _C.require_gpu_tensor(t if t.is_contiguous() else t.contiguous(), f32, name)


def bottle_forward(x, params):
    """(y, h1, h2) of the fused forward; x [B, D] and the 18 parameters are fp32 device tensors."""
    B, D = x.shape
    h1, h2, y = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
    _C.call("fedfr_bottle_forward", x.data_ptr(), _pointers(params), B, D, h1.data_ptr(), h2.data_ptr(), y.data_ptr(), _C.stream())
    return y, h1, h2


def bottle_backward(x, params, h1, h2, dy, need_dx=True):
    """(dx or None, the 18 parameter gradients) of the fused backward."""
    B, D = x.shape
    dx = torch.empty_like(x) if need_dx else None
    grads = [torch.empty_like(p) for p in params]
    nbytes = _C.lib().fedfr_bottle_workspace_bytes(B, D)
    ws = torch.empty(max(nbytes, 4) // 4, dtype=f32, device=x.device)
    _C.call("fedfr_bottle_backward", x.data_ptr(), _pointers(params), h1.data_ptr(), h2.data_ptr(), dy.data_ptr(), B, D, _C.ptr(dx),
            _pointers(grads), ws.data_ptr(), nbytes, _C.stream())
    return dx, grads


class _BottleFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, *params):
        if x.dim() != 2:
            raise RuntimeError("fedfr_amd BottleBlock: input must be [batch, features] (got %s)" % (tuple(x.shape),))
        x = _gpu(x, "x")
        params = [_gpu(p, "BottleBlock parameter %d" % i) for i, p in enumerate(params)]
        y, h1, h2 = bottle_forward(x, params)
        ctx.save_for_backward(x, h1, h2, *params)         # dropped at once under torch.no_grad(): the eval paths keep no state
        return y

    @staticmethod
    def backward(ctx, dy):
        x, h1, h2, *params = ctx.saved_tensors
        dx, grads = bottle_backward(x, params, h1, h2, _gpu(dy, "dy"), need_dx=ctx.needs_input_grad[0])
        return (dx, *grads)


class _Affine(nn.Module):
    """weight [out, in] and bias [out] of one nn.Linear of the reference, initialised like it"""

    def __init__(self, in_dim, out_dim):
        super().__init__()
        ref = nn.Linear(in_dim, out_dim)                  # throw-away: consumes the RNG exactly as the reference's layer does
        self.weight, self.bias = nn.Parameter(ref.weight.detach().clone()), nn.Parameter(ref.bias.detach().clone())


class _Branch(nn.Module):
    """parameters of one ``Sequential(Linear, LeakyReLU, Linear, LeakyReLU)`` under its keys ``0`` and ``2``"""

    def __init__(self, in_dim, branch_dim):
        super().__init__()
        self.add_module("0", _Affine(in_dim, branch_dim))
        self.add_module("2", _Affine(branch_dim, branch_dim))


class BottleBlock(nn.Module):
    def __init__(self, in_dim, bottle_rate):
        super().__init__()
        if bottle_rate != 4 or in_dim % 64 or not 64 <= in_dim <= 512:
            raise ValueError("fedfr_amd BottleBlock: in_dim must be a multiple of 64 in [64, 512] and bottle_rate 4 (got %r, %r): "
                             "the fused kernels cover nothing else" % (in_dim, bottle_rate))
        self.in_dim, self.bottle_rate = in_dim, bottle_rate
        branch_dim = in_dim // bottle_rate
        for g in range(1, 5):                             # the reference's construction order: br1..br4, then concat_fc
            setattr(self, "br%d" % g, _Branch(in_dim, branch_dim))
        self.concat_fc = _Affine(branch_dim * 4, in_dim)

    def forward(self, x):
        return _BottleFn.apply(x, *self.parameters())
