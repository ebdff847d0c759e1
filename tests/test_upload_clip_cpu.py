"""The clip and the Gaussian mechanism on compressed and top-k uploads, the part that needs no GPU: the exactness claim behind the norm of
a compressed upload (T_b = S_b 4^(eb - 127) is an fp64 number for every scale byte and every S_b), the references of
tests/upload_clip_cases.py against plain fp64 arithmetic, the C ABI (symbols, the workspace rule, every argument error on host pointers:
they are all reported before anything is launched), no scratch memory in the new kernels, and the Python surface: what
``server.UploadClip``, ``FedCompressed`` / ``FedSparse`` and ``Server.train`` refuse, in which order, and what ``clip_uploads`` lets through."""
import ctypes as C
import importlib.util
import math
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest
import torch

import compress_cases as Q
import sparse_cases as S
import upload_clip_cases as U
from conftest import REPO

f32, f64 = np.float32, np.float64
NEW_SYMBOLS = ("fedfr_upload_sqnorm_workspace_bytes", "fedfr_delta_sqnorm", "fedfr_sparse_sqnorm", "fedfr_delta_aggregate_dp",
               "fedfr_sparse_aggregate_dp")


@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__ as ge
    ge.build()
    from fedfr_amd import _C
    return _C


# ---- the exactness claim -----------------------------------------------------------------------------------------------------------------
def test_block_term_is_exact_in_fp64_for_every_scale_byte():
    """all 255 scale bytes x the extreme S_b (0, 1, the largest of either width, odd values with 19 and 20 significant bits): the fp64
    product double(S_b) 4^(eb - 127) equals the rational number, and lies inside the normal range (no underflow at eb = 0, no overflow at
    eb = 254)"""
    s_max8, s_max4 = 32 * 128 * 128, 32 * 8 * 8
    for eb in range(255):
        for s_b in (0, 1, 2, 3, 49, s_max4 - 1, s_max4, 127 * 127, 2 ** 19 - 1, 2 ** 19 + 1, s_max8 - 1, s_max8):
            t = U.t_b_fp64(s_b, eb)
            assert Fraction(t) == U.t_b_exact(s_b, eb), (s_b, eb)
            assert s_b == 0 or 2.0 ** -254 <= t <= 2.0 ** 274
    # and the vectorised form the GPU tests use agrees with it
    codes = np.full(64, 0x80, dtype=np.uint8)                               # -128 everywhere: two blocks of S_b = 32 * 128^2
    t, bad = U.delta_terms(codes, np.array([0, 254], dtype=np.uint8), 8, 64)
    assert not bad and [Fraction(v) for v in t.tolist()] == [U.t_b_exact(s_max8, 0), U.t_b_exact(s_max8, 254)]
    assert U.delta_terms(codes, np.array([255, 3], dtype=np.uint8), 8, 64)[1] and math.isnan(U.delta_sqnorm(codes, np.array([255, 3], dtype=np.uint8), 8, 64))


@pytest.mark.parametrize("bits", Q.BITS)
def test_reference_norm_is_the_norm_of_the_dequantised_upload(bits):
    """fsum of the exact block terms against the fp64 sum of dq^2 of the existing restatement (each dq is an fp32 number, its square exact in
    fp64); elements behind n are not counted: the pad nibble of an odd 4-bit n and garbage in the bytes behind it change nothing"""
    for n in Q.SIZES:
        for codes, scales in U.quantized_uploads(n, 2, bits) + U.hashed_uploads(n, 2, bits, top=240):      # (240: every dq is finite in fp32)
            ref = U.delta_sqnorm(codes, scales, bits, n)
            dq = Q.dequantize(codes, scales, bits, n).astype(f64)
            assert U.rel_err(math.fsum((dq * dq).tolist()), ref) == 0.0, (bits, n)
            if bits == 4 and n % 2:
                dirty = codes.copy()
                dirty[-1] |= 0x70
                assert U.delta_sqnorm(dirty, scales, bits, n) == ref
            assert U.delta_sqnorm(np.concatenate([codes, np.full(40, 0x7F, dtype=np.uint8)]), scales, bits, n) == ref
    assert U.delta_sqnorm(np.array([0x80], dtype=np.uint8), np.array([127], dtype=np.uint8), 8, 1) == 128.0 ** 2
    assert U.delta_sqnorm(np.array([0x88], dtype=np.uint8), np.array([127], dtype=np.uint8), 4, 2) == 2 * 8.0 ** 2


def test_sparse_references():
    v = np.array([3e-30, -2.5, 1e19, 1.17549435e-38, -0.0], dtype=f32)
    assert U.sparse_sqnorm(v) == math.fsum([float(a) ** 2 for a in v.tolist()]) and U.sparse_sqnorm(v[:0]) == 0.0
    assert U.violations(np.array([0, 5, 9], dtype=np.uint32), 10) == 0
    assert U.violations(np.array([0, 5, 5, 9], dtype=np.uint32), 10) == 1      # a duplicate
    assert U.violations(np.array([0, 7, 6, 9], dtype=np.uint32), 10) == 1      # a descending pair (the entry behind it ascends again)
    assert U.violations(np.array([0, 5, 10], dtype=np.uint32), 10) == 1        # index = n
    assert U.violations(np.array([10], dtype=np.uint32), 10) == 1 and U.violations(np.array([], dtype=np.uint32), 10) == 0
    for n in S.AGG_SIZES:
        for shape in S.UPLOAD_SHAPES:
            assert all(U.violations(i, n) == 0 for i, _ in S.uploads(n, shape))


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_header_ctypes_table_and_library_carry_the_symbols(built_lib):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "fedfr_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(fedfr_[a-z0-9_]+)\s*\(", src))
    out = subprocess.run(["nm", "-D", "--defined-only", built_lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = set(re.findall(r"\sT\s+(fedfr_[a-z0-9_]+)", out))
    for s in NEW_SYMBOLS:
        assert s in declared and s in built_lib.SIGNATURES and s in exported, s
    lib = built_lib.lib()
    for m in (0, 1, 7, 8, 2047, 2048, 65156160, Q.BIG):
        for k in range(1, 9):
            assert lib.fedfr_upload_sqnorm_workspace_bytes(k, m) == k * Q.grid(m) * 8
        for k in (0, 9, -1):
            assert lib.fedfr_upload_sqnorm_workspace_bytes(k, m) == 0


def _aligned(nbytes, off=0):
    raw = np.zeros(nbytes + 32, dtype=np.uint8)
    a = raw.ctypes.data
    return raw, (a + 15) // 16 * 16 + off


def test_argument_errors_are_host_side(built_lib):
    """every refused call returns FEDFR_ERR_ARG (a short workspace: FEDFR_ERR_WORKSPACE) with a message naming the function BEFORE any HIP
    call: host pointers serve, no GPU is needed, and nothing is written"""
    lib = built_lib.lib()
    hdr = open(os.path.join(REPO, "include", "fedfr_hip.h")).read()
    err_arg = int(re.search(r"#define FEDFR_ERR_ARG \((-?\d+)\)", hdr).group(1))
    err_ws = int(re.search(r"#define FEDFR_ERR_WORKSPACE \((-?\d+)\)", hdr).group(1))
    n = 64
    keep = [_aligned(4 * n) for _ in range(4)] + [_aligned(n) for _ in range(2)] + [_aligned(64) for _ in range(4)]
    dst, x, val, idx, codes, scales, sq, coef, viol, wsp = [a for _, a in keep]
    vp = C.c_void_p

    def refused(rc, *words, code=err_arg):
        assert rc == code, rc
        msg = lib.fedfr_last_error_string().decode()
        for w in words:
            assert w in msg, msg

    def arr(ps):
        return (vp * max(len(ps), 1))(*ps)

    ws = (C.c_float * 9)(*([0.125] * 9))
    nan, inf = float("nan"), float("inf")
    cs, ss = arr([codes] * 9), arr([scales] * 9)
    dn = lib.fedfr_delta_sqnorm
    for bits in (0, 5, 16):
        refused(dn(cs, ss, ws, 2, bits, n, 1.0, sq, coef, wsp, 64, None), "delta_sqnorm", "bits=%d" % bits)
    for k in (0, 9, -1):
        refused(dn(cs, ss, ws, k, 8, n, 1.0, sq, coef, wsp, 64, None), "delta_sqnorm", "k=%d" % k)
    for a in ((None, ss, ws, sq, coef, wsp), (cs, None, ws, sq, coef, wsp), (cs, ss, None, sq, coef, wsp), (cs, ss, ws, None, coef, wsp),
              (cs, ss, ws, sq, None, wsp), (cs, ss, ws, sq, coef, None)):
        refused(dn(a[0], a[1], a[2], 2, 8, n, 1.0, a[3], a[4], a[5], 64, None), "delta_sqnorm", "null")
    refused(dn(arr([codes, None]), ss, ws, 2, 8, n, 1.0, sq, coef, wsp, 64, None), "delta_sqnorm", "code buffer 1 is null")
    refused(dn(cs, arr([scales, None]), ws, 2, 4, n, 1.0, sq, coef, wsp, 64, None), "delta_sqnorm", "scale buffer 1 is null")
    refused(dn(arr([codes, codes + 8]), ss, ws, 2, 8, n, 1.0, sq, coef, wsp, 64, None), "delta_sqnorm", "aligned")
    refused(dn(cs, ss, ws, 2, 8, n, 1.0, sq + 4, coef, wsp, 64, None), "delta_sqnorm", "aligned")
    refused(dn(cs, ss, ws, 2, 8, n, 1.0, sq, coef + 2, wsp, 64, None), "delta_sqnorm", "aligned")
    refused(dn(cs, ss, ws, 2, 8, n, 1.0, sq, coef, wsp + 4, 64, None), "delta_sqnorm", "aligned")
    refused(dn(cs, ss, ws, 2, 8, n, nan, sq, coef, wsp, 64, None), "delta_sqnorm", "NaN")
    refused(dn(cs, ss, ws, 2, 8, 0, 1.0, sq, coef, wsp, 64, None), "delta_sqnorm", "n must be positive")
    refused(dn(cs, ss, ws, 2, 8, n, 1.0, sq, coef, wsp, 15, None), "delta_sqnorm", "workspace of 15 bytes, 16 needed", code=err_ws)

    ix, vs = arr([idx] * 9), arr([val] * 9)
    keeps = (C.c_size_t * 9)(*([16] * 9))
    sn = lib.fedfr_sparse_sqnorm
    for k in (0, 9, -1):
        refused(sn(ix, vs, keeps, ws, k, n, 1.0, sq, coef, viol, wsp, 64, None), "sparse_sqnorm", "k=%d" % k)
    for a in ((None, vs, keeps, ws, sq, coef, viol, wsp), (ix, None, keeps, ws, sq, coef, viol, wsp), (ix, vs, None, ws, sq, coef, viol, wsp),
              (ix, vs, keeps, None, sq, coef, viol, wsp), (ix, vs, keeps, ws, None, coef, viol, wsp), (ix, vs, keeps, ws, sq, None, viol, wsp),
              (ix, vs, keeps, ws, sq, coef, None, wsp), (ix, vs, keeps, ws, sq, coef, viol, None)):
        refused(sn(a[0], a[1], a[2], a[3], 2, n, 1.0, a[4], a[5], a[6], a[7], 64, None), "sparse_sqnorm", "null")
    refused(sn(arr([idx, None]), vs, keeps, ws, 2, n, 1.0, sq, coef, viol, wsp, 64, None), "sparse_sqnorm", "index buffer 1 is null")
    refused(sn(ix, arr([val, None]), keeps, ws, 2, n, 1.0, sq, coef, viol, wsp, 64, None), "sparse_sqnorm", "value buffer 1 is null")
    refused(sn(ix, vs, (C.c_size_t * 2)(16, n + 1), ws, 2, n, 1.0, sq, coef, viol, wsp, 64, None), "sparse_sqnorm", "upload 1", "keep=%d" % (n + 1))
    refused(sn(ix, vs, keeps, ws, 2, 1 << 31, 1.0, sq, coef, viol, wsp, 64, None), "sparse_sqnorm", "2^31")
    refused(sn(ix, vs, (C.c_size_t * 2)(0, 0), ws, 2, 0, 1.0, sq, coef, viol, wsp, 64, None), "sparse_sqnorm", "n must be positive")
    refused(sn(arr([idx, idx + 4]), vs, keeps, ws, 2, n, 1.0, sq, coef, viol, wsp, 64, None), "sparse_sqnorm", "aligned")
    refused(sn(ix, arr([val + 8, val]), keeps, ws, 2, n, 1.0, sq, coef, viol, wsp, 64, None), "sparse_sqnorm", "aligned")
    refused(sn(ix, vs, keeps, ws, 2, n, 1.0, sq + 4, coef, viol, wsp, 64, None), "sparse_sqnorm", "aligned")
    refused(sn(ix, vs, keeps, ws, 2, n, 1.0, sq, coef, viol + 2, wsp, 64, None), "sparse_sqnorm", "aligned")
    refused(sn(ix, vs, keeps, ws, 2, n, nan, sq, coef, viol, wsp, 64, None), "sparse_sqnorm", "NaN")
    refused(sn(ix, vs, keeps, ws, 2, n, 1.0, sq, coef, viol, wsp, 8, None), "sparse_sqnorm", "workspace of 8 bytes, 16 needed", code=err_ws)

    noise = (0.5, 1, 2, 3, 0)
    da = lib.fedfr_delta_aggregate_dp
    for bits in (0, 6):
        refused(da(dst, None, cs, ss, coef, 2, bits, n, 0, 1, *noise, None), "delta_aggregate_dp", "bits=%d" % bits)
    for k in (0, 9):
        refused(da(dst, None, cs, ss, coef, k, 8, n, 0, 1, *noise, None), "delta_aggregate_dp", "k=%d" % k)
    for a in ((None, cs, ss, coef), (dst, None, ss, coef), (dst, cs, None, coef), (dst, cs, ss, None)):
        refused(da(a[0], None, a[1], a[2], a[3], 2, 8, n, 0, 1, *noise, None), "delta_aggregate_dp", "null")
    refused(da(dst, None, arr([codes, None]), ss, coef, 2, 8, n, 0, 1, *noise, None), "delta_aggregate_dp", "code buffer 1 is null")
    refused(da(dst + 4, None, cs, ss, coef, 2, 8, n, 0, 1, *noise, None), "delta_aggregate_dp", "aligned")
    refused(da(dst, x + 8, cs, ss, coef, 2, 8, n, 0, 1, *noise, None), "delta_aggregate_dp", "aligned")
    refused(da(dst, None, cs, ss, coef + 2, 2, 8, n, 0, 1, *noise, None), "delta_aggregate_dp", "coef", "aligned")
    for std in (-0.5, nan, inf):
        refused(da(dst, None, cs, ss, coef, 2, 8, n, 0, 1, std, 1, 2, 3, 0, None), "delta_aggregate_dp", "noise_std")
        refused(da(dst, None, cs, ss, coef, 2, 8, n, 0, 0, std, 1, 2, 3, 0, None), "delta_aggregate_dp", "noise_std")      # (a pass that does not draw, too)
    for off in (1, 2, 3, 6):
        refused(da(dst, None, cs, ss, coef, 2, 8, n, 0, 1, 0.5, 1, 2, 3, off, None), "delta_aggregate_dp", "offset %d" % off)
    assert da(dst, x, cs, ss, coef, 8, 8, 0, 1, 1, *noise, None) == 0       # n = 0: a no-op

    sa = lib.fedfr_sparse_aggregate_dp
    for k in (0, 9):
        refused(sa(dst, None, ix, vs, keeps, coef, k, n, 0, 1, *noise, None), "sparse_aggregate_dp", "k=%d" % k)
    for a in ((None, ix, vs, keeps, coef), (dst, None, vs, keeps, coef), (dst, ix, None, keeps, coef), (dst, ix, vs, None, coef), (dst, ix, vs, keeps, None)):
        refused(sa(a[0], None, a[1], a[2], a[3], a[4], 2, n, 0, 1, *noise, None), "sparse_aggregate_dp", "null")
    refused(sa(dst, None, arr([idx, None]), vs, keeps, coef, 2, n, 0, 1, *noise, None), "sparse_aggregate_dp", "index buffer 1 is null")
    refused(sa(dst, None, ix, vs, (C.c_size_t * 2)(n + 1, 1), coef, 2, n, 0, 1, *noise, None), "sparse_aggregate_dp", "upload 0")
    refused(sa(dst, None, ix, vs, keeps, coef, 2, 1 << 31, 0, 1, *noise, None), "sparse_aggregate_dp", "2^31")
    refused(sa(dst + 8, None, ix, vs, keeps, coef, 2, n, 0, 1, *noise, None), "sparse_aggregate_dp", "aligned")
    refused(sa(dst, None, ix, vs, keeps, coef + 1, 2, n, 0, 1, *noise, None), "sparse_aggregate_dp", "coef", "aligned")
    for std in (-1.0, nan, inf):
        refused(sa(dst, None, ix, vs, keeps, coef, 2, n, 0, 1, std, 1, 2, 3, 0, None), "sparse_aggregate_dp", "noise_std")
    refused(sa(dst, None, ix, vs, keeps, coef, 2, n, 0, 1, 0.5, 1, 2, 3, 5, None), "sparse_aggregate_dp", "offset 5")
    assert sa(dst, x, ix, vs, keeps, coef, 2, 0, 1, 1, 0.5, 1, 2, 3, 0, None) == err_arg      # keeps[i] > n = 0 comes first
    assert sa(dst, x, ix, vs, (C.c_size_t * 2)(0, 0), coef, 2, 0, 1, 1, *noise, None) == 0    # n = 0: a no-op
    for raw, _ in keep:
        assert not raw.any()                                                 # nothing was written


def test_new_kernels_use_no_scratch_memory(built_lib):
    """2 widths x K = 1..8 norm passes, K = 1..8 sparse norm passes, and the aggregates' shells with device coefficients, with and without
    noise; both storage builds.  The existing shells keep their counts (tests/test_compress_cpu.py, tests/test_sparse_cpu.py)"""
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(REPO, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    ks = kr.kernels(built_lib.LIB_PATH)
    bf16 = os.path.join(os.path.dirname(built_lib.LIB_PATH), "libfedfr_hip_bf16.so")
    if os.path.exists(bf16) and os.path.basename(built_lib.LIB_PATH) != "libfedfr_hip_bf16.so":
        ks.update({"bf16:" + k: v for k, v in kr.kernels(bf16).items()})
    builds = 2 if any(k.startswith("bf16:") for k in ks) else 1
    want = {"delta_sqnorm_kernel": 16, "sparse_sqnorm_kernel": 8, "delta_aggregate_dp_kernel": 32, "sparse_aggregate_dp_kernel": 16}
    for name, count in want.items():
        mine = {n: r for n, r in ks.items() if name in n}
        assert len(mine) == count * builds, (name, len(mine))
        bad = [(n, r) for n, r in mine.items() if r["scratch"]]
        assert not bad, bad
        assert max(r["vgpr"] for r in mine.values()) <= 128, name            # at least two waves per SIMD


# ---- Python surface ----------------------------------------------------------------------------------------------------------------------
def test_upload_clip_and_the_round_functions_refuse_in_order(built_lib):
    from fedfr_amd import compress, privacy, server
    from fedfr_amd.client import FlatStateDict
    for bad in (0, 0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="clip_norm"):
            server.UploadClip(bad)
    clip = server.UploadClip(2.5)
    assert clip.clip_norm == 2.5 and clip.last_update_sqnorm is None and clip.last_coef is None and clip.last_violations is None
    cpu = FlatStateDict.from_flat((torch.zeros(8), torch.zeros(0), torch.zeros(0, dtype=torch.int64)), [], [])
    cd = compress.CompressedDelta(torch.zeros(8, dtype=torch.uint8), torch.zeros(1, dtype=torch.uint8), 8, 8, torch.zeros(3), torch.zeros(2, dtype=torch.int64),
                                  torch.zeros(1, dtype=torch.int32))
    sd = compress.SparseDelta(torch.zeros(2, dtype=torch.int32), torch.zeros(2), 8, 2, torch.zeros(3), torch.zeros(2, dtype=torch.int64),
                              torch.zeros(1, dtype=torch.int32))
    mech = privacy.GaussianMechanism(1.0, 2.5, seed=7)
    for fed, up, noun in ((server.FedCompressed, cd, "CompressedDelta"), (server.FedSparse, sd, "SparseDelta")):
        # the head's order is kept: state, uploads, weights, robust rule, the optimiser's clip; the new refusals follow; the GPU comes last
        with pytest.raises(RuntimeError, match="FlatStateDict"):
            fed({"w": torch.zeros(8)}, [up], [1.0], clip=clip, mech=mech)
        with pytest.raises(RuntimeError, match=noun):
            fed(cpu, [cpu], [1.0], clip=clip, mech=mech)
        with pytest.raises(RuntimeError, match="weights"):
            fed(cpu, [up, up], [1.0], clip=clip, mech=mech)
        with pytest.raises(ValueError, match="robust"):
            fed(cpu, [up], [1.0], server.RobustAggregator("CoordMedian"), clip=clip, mech=mech)
        with pytest.raises(ValueError, match="clip_norm > 0 needs per-client norms"):      # today's sentence, without clip
            fed(cpu, [up], [1.0], server.ServerOptimizer("AVGM", clip_norm=2.5))
        with pytest.raises(ValueError, match="clip_norm > 0 needs per-client norms"):
            fed(cpu, [up], [1.0], server.ServerOptimizer("AVGM", clip_norm=2.5), mech=mech)      # (before "mech needs clip")
        with pytest.raises(ValueError, match="must be a server.UploadClip"):
            fed(cpu, [up], [1.0], clip=2.5)
        with pytest.raises(ValueError, match=r"optimiser clips at 1\.5.*clip_norm=2\.5"):
            fed(cpu, [up], [1.0], server.ServerOptimizer("ADAM", clip_norm=1.5), clip=clip)
        with pytest.raises(ValueError, match="mech needs clip"):
            fed(cpu, [up], [1.0], mech=mech)
        with pytest.raises(ValueError, match=r"clipped at 2\.5.*sensitivity bound is clip_norm=1\.0"):
            fed(cpu, [up], [1.0], clip=clip, mech=privacy.GaussianMechanism(1.0, 1.0, seed=7))
        for opt in (None, server.ServerOptimizer("AVGM"), server.ServerOptimizer("YOGI", clip_norm=2.5),
                    server.ServerOptimizer("ADAM", clip_norm=float(np.float32(2.5)))):
            with pytest.raises(RuntimeError, match="GPU"):                   # served as far as a machine without a GPU can tell
                fed(cpu, [up], [1.0], opt, clip=clip, mech=mech)
        with pytest.raises(RuntimeError, match="GPU"):
            fed(cpu, [up], [1.0], clip=clip)
        with pytest.raises(TypeError):
            fed(cpu, [up], [1.0], None, clip)                                 # keyword-only
    assert mech.round == 0                                                    # no refused call advanced the stream


def _world(aggr, nclients, **extra):
    from fedfr_amd import server

    class Args:
        network, loss, local_epoch, output_dir, BCE_local, aggr_alg = "iresnet18", "CosFace", 1, "/tmp", False, aggr

    for k_, v_ in extra.items():
        setattr(Args, k_, v_)

    class NeverTrains:
        cid = 0

        def __getattr__(self, name):
            raise AssertionError("a client was touched (%s): the round has started" % name)

        def __setattr__(self, name, value):
            raise AssertionError("a client was touched (%s): the round has started" % name)
    return server.Server([NeverTrains() for _ in range(nclients)], None, Args, device=torch.device("cpu"))


OLD_SENTENCES = (
    ({"compress_bits": 8, "clip_norm": 2.5}, r"compress_bits=8 cannot be combined with clip_norm=2\.5: the clip needs per-client norms of the "
                                             r"dequantised deltas, which are not provided"),
    ({"topk_ratio": 0.05, "clip_norm": 2.5}, r"topk_ratio=0\.05 cannot be combined with clip_norm=2\.5: the clip needs per-client norms of the deltas, "
                                             r"which are not provided"),
    ({"compress_bits": 4, "clip_norm": 2.5, "dp_noise_multiplier": 1.0},
     r"dp_noise_multiplier=1\.0 cannot be combined with compress_bits=4: the clip needs per-client norms of the dequantised deltas, which are not provided"),
    ({"topk_ratio": 0.05, "clip_norm": 2.5, "dp_noise_multiplier": 1.0},
     r"dp_noise_multiplier=1\.0 cannot be combined with topk_ratio=0\.05: the clip needs per-client norms of the deltas, which are not provided"),
)


@pytest.mark.parametrize("case", range(len(OLD_SENTENCES)))
def test_without_clip_uploads_every_old_sentence_is_still_raised(case):
    extra, sentence = OLD_SENTENCES[case]
    for off in ({}, {"clip_uploads": False}, {"clip_uploads": None}, {"clip_uploads": 0}):
        for aggr in ("FedAvg", "FedAdam"):
            with pytest.raises(ValueError, match="Server.train: " + sentence):
                _world(aggr, 3, **extra, **off).train()


@pytest.mark.parametrize("case", range(len(OLD_SENTENCES)))
def test_with_clip_uploads_the_round_starts(case):
    """the four pairings are served: the stub world gets as far as touching a client"""
    extra, _ = OLD_SENTENCES[case]
    for aggr in ("FedAvg", "FedProx", "FedAvgM", "FedYogi"):
        with pytest.raises(AssertionError, match="the round has started"):
            _world(aggr, 3, **extra, clip_uploads=True).train()
    with pytest.raises(AssertionError, match="the round has started"):       # without a clip_norm the setting has nothing to do: today's round
        _world("FedAvg", 3, **{k: v for k, v in extra.items() if k == "compress_bits" or k == "topk_ratio"}, clip_uploads=True).train()


def test_what_clip_uploads_still_refuses_and_in_which_order():
    dp = {"clip_norm": 2.5, "dp_noise_multiplier": 1.0}
    on = {"clip_uploads": True, "clip_norm": 2.5}
    with pytest.raises(ValueError, match=r"clip_uploads needs compress_bits or topk_ratio"):
        _world("FedAvg", 3, **on).train()
    with pytest.raises(ValueError, match=r"clip_uploads needs compress_bits or topk_ratio"):
        _world("FedAdam", 3, clip_uploads=True, **dp).train()
    with pytest.raises(ValueError, match=r"clip_uploads cannot be combined with secure_aggregation: .*masks hide"):
        _world("FedAvg", 3, secure_aggregation=True, compress_bits=8, **on).train()
    with pytest.raises(ValueError, match=r"clip_uploads cannot be combined with secure_aggregation"):      # before "needs compress_bits or topk_ratio"
        _world("FedAvg", 3, secure_aggregation=True, **on).train()
    for kind in ("TrimmedMean", "CoordMedian", "Krum", "MultiKrum"):
        with pytest.raises(ValueError, match=r"compress_bits=8 cannot be combined with aggr_alg='%s': a robust rule needs whole client states" % kind):
            _world(kind, 5, compress_bits=8, **on).train()
        with pytest.raises(ValueError, match=r"topk_ratio=0\.05 cannot be combined with aggr_alg='%s': a robust rule needs whole client states" % kind):
            _world(kind, 5, topk_ratio=0.05, **on).train()
        with pytest.raises(ValueError, match=r"dp_noise_multiplier=1\.0 cannot be combined with aggr_alg='%s': a robust rule provides no per-client" % kind):
            _world(kind, 5, compress_bits=8, clip_uploads=True, **dp).train()       # the mechanism's refusal comes before the format's
    with pytest.raises(ValueError, match=r"dp_noise_multiplier=1\.0 cannot be combined with return_all"):
        _world("FedAvg", 3, topk_ratio=0.05, return_all=True, clip_uploads=True, **dp).train()
    with pytest.raises(ValueError, match=r"topk_ratio=0\.05 cannot be combined with compress_bits=8: quantising the kept values is not provided"):
        _world("FedAvg", 3, topk_ratio=0.05, compress_bits=8, **on).train()
    with pytest.raises(ValueError, match=r"topk_ratio=0\.05 cannot be combined with compress_bits=8"):
        _world("FedAvg", 3, topk_ratio=0.05, compress_bits=8, clip_uploads=True, **dp).train()
    with pytest.raises(ValueError, match=r"dp_noise_multiplier=1\.0 needs clip_norm > 0"):
        _world("FedAvg", 3, compress_bits=8, clip_uploads=True, dp_noise_multiplier=1.0).train()
    with pytest.raises(ValueError, match=r"compress_bits.*5"):
        _world("FedAvg", 3, compress_bits=5, **on).train()
