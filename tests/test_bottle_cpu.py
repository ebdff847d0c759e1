"""CPU-side checks of the BottleBlock converter: the test formula of tests/bottle_cases.py is pinned to the reference and is conditioned
well enough for a correct fp32 kernel to pass (tests/test_bottle_kernels_gpu.py), and the Python surface has the reference's keys and
initial values.  Nothing here needs a GPU."""
import numpy as np
import pytest
import torch

from conftest import load_golden

import bottle_cases as bc
from bottle_cases import f32, f64

from fedfr_amd import backbones, client
from fedfr_amd.callbacks import portable_state_dict


def T(a):
    return torch.from_numpy(np.asarray(a))


def maxrel(a, b):
    a, b = a.detach().double(), T(b).double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


@pytest.mark.parametrize("B,D", bc.SHAPES)
def test_fp32_formula_is_within_a_quarter_of_every_tolerance(B, D):
    """the plain fp32 evaluation stands in for a kernel: the inputs leave a correct fp32 implementation 4x of room everywhere"""
    c = bc.case(B, D)
    z1, h1, z2, h2, y = bc.forward(c.x, c.params, f32)
    dx, grads = bc.backward(c.x, c.params, h1, h2, z1 > 0, z2 > 0, c.dy, f32)
    out = []
    try:
        c.check({"y": y, "h1": h1, "h2": h2, "dx": dx, "grads": grads}, frac=0.25, out=out)
    finally:
        print(c.name, "worst fwd %.3g, worst grad %.3g" % (max([e for _, k, e in out if k == "fwd"], default=0.0),
                                                         max([e for _, k, e in out if k == "grad"], default=0.0)))


@pytest.mark.parametrize("B,D", bc.SHAPES)
def test_kink_condition_of_the_fp64_reference(B, D):
    """pre-activations whose sign is not a property of the inputs: at most KINK_SHARE of a case, none in the cases with B <= 33"""
    k1, k2 = bc.case(B, D).kink_masks()
    n = int(k1.sum()) + int(k2.sum())
    print("bottle[%d,%d]: %d of %d pre-activations inside the kink band" % (B, D, n, 2 * B * D))
    assert n <= bc.KINK_SHARE * 2 * B * D
    if B <= 33:
        assert n == 0


def test_fp64_formula_reproduces_the_reference():
    """bce_bottle.npz holds the reference BottleBlock's output for the closed-form x and parameters, the gradient that reached it, and the
    gradients autograd produced from it: the formula of bottle_cases.py gives the same at 1e-6"""
    from oracle import ref_cpu as R
    g = load_golden("bce_bottle")
    x = R.closed_form((int(g["B"]), 512), 0.113, 0.2, 1.0)
    params = bc.golden_params(512)
    z1, h1, z2, h2, y = bc.forward(x, params, f64)
    assert maxrel(y, g["conv_out"]) < 1e-6
    dx, grads = bc.backward(x, params, h1, h2, z1 > 0, z2 > 0, T(g["d_conv_out"]), f64)
    assert maxrel(dx, g["dx"]) < 1e-6
    by_key = dict(zip(bc.PARAM_KEYS, grads))
    for k in ("br1.0.weight", "br3.2.weight", "concat_fc.weight"):
        assert maxrel(by_key[k][:8, :64], g["d_" + k + "_slice"]) < 1e-6, k
    for k, v in by_key.items():
        assert abs(float(v.norm()) - float(g["norm_d_" + k])) < 1e-6 * float(g["norm_d_" + k]), k
        if k.endswith("bias"):
            assert maxrel(v, g["d_" + k]) < 1e-6, k


def test_bce_module_with_a_bottleblock_constructs_with_the_reference_keys():
    g = load_golden("bce_bottle")
    mod = client.BCE_module(512, 10, 2)
    assert isinstance(mod.converter, backbones.BottleBlock)
    assert list(mod.state_dict().keys()) == [str(k) for k in g["keys"]]
    assert [k for k, _ in mod.converter.named_parameters()] == bc.PARAM_KEYS          # the C ABI's pointer order
    assert [tuple(p.shape) for p in mod.converter.parameters()] == bc.param_shapes(512)
    assert isinstance(client.BCE_module(512, 10, 1).converter, torch.nn.Sequential)     # converter_layer == 1 is unchanged


def test_initial_values_are_the_references_under_the_same_seed():
    g = load_golden("bottle_init")
    torch.manual_seed(100)
    sd = backbones.BottleBlock(512, 4).state_dict()
    assert sorted(sd) == sorted(g.files)
    for k, v in sd.items():
        assert torch.equal(v[:8, :8] if v.dim() == 2 else v[:8], T(g[k])), k


def test_reference_keyed_state_dict_round_trips():
    sd = {"weight": torch.zeros(10, 512), "bias": torch.zeros(10)}
    sd.update({"converter." + k: p for k, p in zip(bc.PARAM_KEYS, bc.golden_params(512))})
    mod = client.BCE_module(512, 10, 2)
    mod.load_state_dict(sd, strict=True)
    out = portable_state_dict(mod)
    assert list(out) == list(mod.state_dict())
    for k, v in sd.items():
        assert torch.equal(out[k], v) and out[k].device.type == "cpu" and out[k].is_contiguous(), k


def test_unsupported_shapes_are_errors():
    for in_dim, rate in ((512, 2), (96, 4), (1024, 4)):
        with pytest.raises(ValueError):
            backbones.BottleBlock(in_dim, rate)
