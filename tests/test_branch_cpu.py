"""CPU-side checks of the fused branch head (csrc/branch.hip): the test inputs are conditioned for a correct fp32 kernel (the fp32 evaluation
of every reference formula is within a QUARTER of every tolerance of its fp64 evaluation), and the new entry points are declared in
include/fedfr_hip.h and listed in fedfr_amd/_C.py with the same number of arguments."""
import os
import re

import pytest
import torch

import branch_cases as BC
from conftest import REPO
from head_cases import check, f32, f64

NEW_SYMBOLS = ["fedfr_bce_fused_workspace_bytes", "fedfr_bce_fused", "fedfr_branch_dfeats", "fedfr_branch_workspace_bytes", "fedfr_branch_head"]


def _quarter(case):
    r32, r64 = case.ref(f32), case.ref(f64)
    assert set(r32) == set(r64)
    for k, q in r64.items():
        assert bool(torch.isfinite(q.value).all()), "%s %s: the fp64 reference is not finite" % (case.name, k)
        check(r32[k].value, q, "%s %s" % (case.name, k), frac=0.25)


@pytest.mark.parametrize("case", BC.bce_fused_cases(), ids=lambda c: c.name)
def test_bce_fused_inputs_are_conditioned_for_fp32(case):
    _quarter(case)


@pytest.mark.parametrize("case", BC.branch_cases(), ids=lambda c: c.name)
def test_branch_head_inputs_are_conditioned_for_fp32(case):
    _quarter(case)


def test_cases_cover_the_parameter_table():
    cs = BC.branch_cases()
    assert {c.B for c in cs} == {1, 2, 5, 130}
    assert {c.n_class for c in cs} == {1, 3, 100}
    assert {255, 256, 4096, 4097} <= {c.C for c in cs} and any(c.C == c.n_class for c in cs)
    assert {(c.conv, c.detach, c.con) for c in cs} == {(k, d, n) for k in (0, 1, 2) for d in (False, True) for n in (False, True)}
    for conv in (0, 1, 2):                                   # both sides of the split-K rule for every converter kind
        assert {256 <= c.C <= 4096 for c in cs if c.conv == conv} == {False, True}
    big = [c for c in cs if c.B >= 5]
    assert any(int(c.label[0]) == 0 and int(c.label[1]) == c.n_class - 1 and int(c.label[3]) == c.C - 1 for c in big)
    assert any(c.n_class in c.label.tolist() for c in big if c.C > c.n_class)         # the first public identity: an all-negative BCE row
    assert all(bool((c.feats[1] == 0).all()) for c in cs if c.B >= 2)
    assert all(bool((c.bce_b > 0).any()) and bool((c.bce_b < 0).any()) for c in cs if c.conv and c.n_class >= 3)
    # no BottleBlock pre-activation of the small cases sits on a kink (bottle_cases' rule); the large ones keep their share below the limit
    for c in cs:
        if c.conv == BC.CONV_BOTTLE:
            n = sum(int(k.sum()) for k in c.kink_masks())
            assert n == 0 if c.B <= 33 else n <= BC.bottle_cases.KINK_SHARE * 2 * c.B * BC.D, (c.name, n)


def test_edge_cosines_are_plus_and_minus_one():
    """the BCE weight rows built from the fp64 forward of the converter give cos = +1 (the target) and -1 to fp32 rounding"""
    for c in BC.branch_cases():
        if not (c.conv and c.B >= 5 and c.n_class >= 2):
            continue
        y = c.converter(c.feats.to(f64), [p.to(f64) for p in c.conv_params])[0]
        cos = torch.nn.functional.normalize(y, dim=1) @ torch.nn.functional.normalize(c.bce_w.to(f64), dim=1).t()
        kp = int(c.label[2])
        assert abs(float(cos[2, kp]) - 1.0) < 1e-6 and abs(float(cos[3, (kp + 1) % c.n_class]) + 1.0) < 1e-6, c.name


def test_new_symbols_declared_with_matching_arity():
    from fedfr_amd import _C
    src = open(os.path.join(REPO, "include", "fedfr_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NEW_SYMBOLS:
        m = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, src)
        assert m, "%s is not declared in include/fedfr_hip.h" % name
        assert name in _C.SIGNATURES, "%s is missing from fedfr_amd/_C.py" % name
        assert len(m.group(1).split(",")) == len(_C.SIGNATURES[name][1]), name
