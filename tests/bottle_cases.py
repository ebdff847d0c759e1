"""Inputs and references for the direct tests of the fused BottleBlock kernels (csrc/bottle.hip), in the style of head_cases.py.

The block, for x [B, D], H = D / 4, branch g = 0..3, leaky(z) = z if z > 0 else 0.01 z:
    z1_g = x W1_g^T + b1_g,  h1_g = leaky(z1_g)          W1_g [H, D]
    z2_g = h1_g W2_g^T + b2_g,  h2_g = leaky(z2_g)       W2_g [H, H]
    y = x + [h2_0|h2_1|h2_2|h2_3] W3^T + b3              W3 [D, D]
``forward`` / ``backward`` below are that formula and its hand-derived gradient as plain torch expressions in a chosen dtype; the fp64
evaluation is what the kernels are held to, and tests/test_bottle_cpu.py pins it to the values captured from the reference module
(tests/golden/bce_bottle.npz) and holds the fp32 evaluation to a QUARTER of every tolerance.  Parameters are the 18 tensors in the C
ABI's order: br1..br4 x (first weight, first bias, second weight, second bias), then concat_fc weight and bias.

Tolerances (head_cases.TOL, against fp64): y, h1, h2 1e-5 per row; gradients 1e-4 — dx per row, every row of a weight or bias gradient
against the LARGEST row of the same tensor: a unit whose upstream gradient nearly cancels over the batch has no relative accuracy in fp32
under any summation order.

The kink.  fp32 and fp64 can disagree on the sign of a pre-activation that is almost 0, and leaky' then differs by 0.99.  The reference
backward uses the fp64 signs everywhere except where |z| < KINK * (max |z| of that row of the [B, D] pre-activation matrix); there it
takes the sign of the activation the code under test returned.  Such elements may be at most KINK_SHARE of a case's pre-activations, and
none at all in the cases with B <= 33 (``kink_masks`` + test_bottle_cpu.py: a property of the fp64 reference and the inputs alone).
"""
import functools

import torch

from head_cases import Q, TOL, check, uniform, f32, f64  # noqa: F401

SLOPE = 0.01
SHAPES = [(1, 64), (2, 64), (17, 512), (33, 512), (130, 512), (257, 512)]
KINK, KINK_SHARE = 1e-5, 1e-4
N_PARAMS = 18
PARAM_KEYS = ["br%d.%d.%s" % (g, l, n) for g in (1, 2, 3, 4) for l in (0, 2) for n in ("weight", "bias")] + ["concat_fc.weight", "concat_fc.bias"]


def param_shapes(D):
    H = D // 4
    return [s for _ in range(4) for s in ((H, D), (H,), (H, H), (H,))] + [(D, D), (D,)]


def closed_form(shape, a, b, scale):
    """scale * sin(a i + b) over the flattened index, computed in fp64 (no RNG: the golden generator uses the same values)"""
    n = 1
    for s in shape:
        n *= int(s)
    return (scale * torch.sin(a * torch.arange(n, dtype=f64) + b)).to(f32).reshape(tuple(shape))


def golden_params(D=512):
    """the BottleBlock parameters of the golden fixtures: amplitudes 2 / sqrt(fan_in), incommensurate frequencies"""
    out = []
    for i, s in enumerate(param_shapes(D)):
        fan_in = s[1] if len(s) == 2 else out[-1].shape[1]          # a bias follows its weight
        out.append(closed_form(s, 0.37 + 0.0613 * i, 0.11 * i, 2.0 / fan_in ** 0.5))
    return out


def forward(x, params, dt):
    """-> z1, h1, z2, h2 (each [B, D], branch g in columns g H .. (g + 1) H) and y"""
    x = x.to(dt)
    P = [p.to(dt) for p in params]
    z1 = torch.cat([x @ P[4 * g].t() + P[4 * g + 1] for g in range(4)], 1)
    h1 = torch.where(z1 > 0, z1, SLOPE * z1)
    H = x.shape[1] // 4
    z2 = torch.cat([h1[:, g * H:(g + 1) * H] @ P[4 * g + 2].t() + P[4 * g + 3] for g in range(4)], 1)
    h2 = torch.where(z2 > 0, z2, SLOPE * z2)
    y = x + h2 @ P[16].t() + P[17]
    return z1, h1, z2, h2, y


def backward(x, params, h1, h2, pos1, pos2, dy, dt):
    """dx and the 18 parameter gradients from dy; pos1 / pos2: where the pre-activations count as > 0 (leaky' = 1, else 0.01)"""
    x, dy, h1, h2 = x.to(dt), dy.to(dt), h1.to(dt), h2.to(dt)
    P = [p.to(dt) for p in params]
    H = x.shape[1] // 4
    one, sl = torch.ones((), dtype=dt), torch.full((), SLOPE, dtype=dt)
    grads = [None] * N_PARAMS
    grads[16], grads[17] = dy.t() @ h2, dy.sum(0)
    dz2 = (dy @ P[16]) * torch.where(pos2, one, sl)
    dx = dy.clone()
    for g in range(4):
        c = slice(g * H, (g + 1) * H)
        grads[4 * g + 2], grads[4 * g + 3] = dz2[:, c].t() @ h1[:, c], dz2[:, c].sum(0)
        dz1 = (dz2[:, c] @ P[4 * g + 2]) * torch.where(pos1[:, c], one, sl)
        grads[4 * g], grads[4 * g + 1] = dz1.t() @ x, dz1.sum(0)
        dx = dx + dz1 @ P[4 * g]
    return dx, grads


class BottleCase:
    def __init__(self, B, D):
        self.B, self.D, self.name = B, D, "bottle[%d,%d]" % (B, D)
        seed = 19000 + 31 * B + D        # chosen with the kink condition in view: min |z| / row max is 1.8e-5 at B = 17 and 33
        self.x, self.dy = uniform((B, D), seed), uniform((B, D), seed + 1)
        self.params = []
        for i, s in enumerate(param_shapes(D)):
            fan_in = s[1] if len(s) == 2 else self.params[-1].shape[1]
            self.params.append(uniform(s, seed + 2 + i) / fan_in ** 0.5)

    @functools.lru_cache(maxsize=None)
    def fwd(self, dt=f64):
        return forward(self.x, self.params, dt)

    def kink_masks(self):
        """where the fp64 pre-activations are too close to 0 for their sign to be a property of the inputs"""
        z1, _, z2, _, _ = self.fwd(f64)
        return tuple(z.abs() < KINK * z.abs().amax(1, keepdim=True) for z in (z1, z2))

    def ref(self, h1_got, h2_got):
        """{name: Q} in fp64; h1_got / h2_got: the activations the code under test returned (their signs are used at the kinks only)"""
        z1, h1, z2, h2, y = self.fwd(f64)
        k1, k2 = self.kink_masks()
        pos1 = torch.where(k1, h1_got.detach().cpu() > 0, z1 > 0)
        pos2 = torch.where(k2, h2_got.detach().cpu() > 0, z2 > 0)
        dx, grads = backward(self.x, self.params, h1, h2, pos1, pos2, self.dy, f64)
        out = {"y": Q(y, "fwd"), "h1": Q(h1, "fwd"), "h2": Q(h2, "fwd"), "dx": Q(dx, "grad")}
        for i, g in enumerate(grads):
            rows = g if g.dim() == 2 else g.reshape(-1, 1)
            out["d_" + PARAM_KEYS[i]] = Q(g, "grad", scale=torch.full((rows.shape[0],), float(rows.abs().amax(1).max()), dtype=f64))
        return out

    def check(self, got, frac=1.0, out=None):
        """``got``: {"y", "h1", "h2", "dx", "grads": [18]} of the code under test, all finite"""
        ref = self.ref(got["h1"], got["h2"])
        for k in ("y", "h1", "h2", "dx"):
            assert bool(torch.isfinite(got[k]).all()), "%s %s: non-finite values (an output element was not written)" % (self.name, k)
            check(got[k], ref[k], "%s %s" % (self.name, k), frac, out)
        for i, g in enumerate(got["grads"]):
            assert bool(torch.isfinite(g).all()), "%s d_%s: non-finite values" % (self.name, PARAM_KEYS[i])
            check(g, ref["d_" + PARAM_KEYS[i]], "%s d_%s" % (self.name, PARAM_KEYS[i]), frac, out)


@functools.lru_cache(maxsize=None)
def case(B, D):
    return BottleCase(B, D)
