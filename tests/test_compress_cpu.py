"""Compressed client uploads (8 / 4-bit block-scaled deltas with error feedback), the part that needs no GPU: the laws the format
promises hold for the numpy restatement of tests/compress_cases.py (which the kernels are held to bit for bit on the GPU), the C ABI
carries the new entry points with their host-side checks, no ``delta_`` kernel uses scratch memory, and the Python surface refuses what
it cannot serve before any client trains."""
import ctypes as C
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import compress_cases as Q
from conftest import REPO

f32, f64 = np.float32, np.float64
NEW_SYMBOLS = ("fedfr_delta_code_bytes", "fedfr_delta_scale_bytes", "fedfr_delta_quantize", "fedfr_delta_aggregate")


@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__ as ge
    ge.build()
    from fedfr_amd import _C
    return _C


def law_inputs(bits):
    """[(name, x, x_i, e or None)]: the sine states with and without a residual, the edge blocks on both paths and with both short blocks"""
    x, xs = Q.inputs(4103, 3)
    out = [("sine", x, xs[1], None), ("sine+residual", x, xs[2], Q.residual(4103))]
    for short, copies in ((1, 2), (31, 2), (1, 1), (31, 1)):
        ex, exi = Q.edge_blocks(bits, short, copies)
        out.append(("edge short=%d copies=%d" % (short, copies), ex, exi, None))
        out.append(("edge+0 residual short=%d copies=%d" % (short, copies), ex, exi, np.zeros(ex.size, dtype=f32)))
    return out


# ---- laws of the restatement -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", Q.BITS)
def test_restatement_laws(bits):
    """dq + e' == v exactly on finite blocks; |e'| <= scale / 2 unless saturated and < scale always; codes within +-qmax; scale byte 255
    exactly for the non-finite blocks, with +0 residual and zero codes there; eb <= 252 on every finite block; sizes as the format says"""
    qm = Q.qmax(bits)
    for name, x, xi, e in law_inputs(bits):
        n = x.size
        codes, scales, en, nbad, info = Q.quantize(x, xi, e, bits)
        assert (en is None) == (e is None) and (en is None or np.array_equal(Q.bits_of(en), Q.bits_of(info["e_new"]))), name
        en = info["e_new"]
        assert codes.size == (n * bits + 7) // 8 and scales.size == (n + 31) // 32, name
        v, q, bad, scale = info["v"], info["q"], info["bad"], info["scale"]
        assert np.all(np.abs(q) <= qm), name
        fin_block = ~np.isfinite(v.astype(f64))                              # per element; per block below
        nb = scales.size
        pad = np.zeros(nb * 32, dtype=bool)
        pad[:n] = fin_block
        block_bad = pad.reshape(nb, 32).any(axis=1)
        assert np.array_equal(scales == 255, block_bad), name
        assert nbad == int(block_bad.sum()), name
        assert np.all(scales[~block_bad] <= 252), name
        assert np.all(q[bad] == 0) and np.all(Q.bits_of(en[bad]) == 0), name      # +0, not -0
        dq = Q.dequantize(codes, scales, bits, n)
        assert np.all(np.isnan(dq[bad])) and np.all(np.isfinite(dq[~bad])), name
        ok = ~bad
        # (evaluated in fp64, where this sum of two float32 values is exact: dq is at most 2^(bits-1) scales, and e' = v - dq is a multiple
        # of ulp(v) >= 2^-25 scale wherever dq is not 0)
        assert np.array_equal(dq[ok].astype(f64) + en[ok].astype(f64), v[ok].astype(f64)), name
        s64 = scale[ok].astype(f64)
        ae = np.abs(en[ok].astype(f64))
        assert np.all(ae < s64), name
        unsat = ~info["sat"][ok]
        assert np.all(ae[unsat] <= s64[unsat] / 2), name
        assert np.all(np.abs(v[ok][info["sat"][ok]].astype(f64)) >= (qm + 0.5) * s64[info["sat"][ok]]), name      # only these saturate


@pytest.mark.parametrize("bits", Q.BITS)
def test_edge_blocks_hit_what_they_are_for(bits):
    """the 15 kinds of block produce the scale bytes, codes and flags they were built for (so the GPU comparison covers those paths)"""
    qm = Q.qmax(bits)
    x, xi = Q.edge_blocks(bits, 1, 2)
    codes, scales, _, nbad, info = Q.quantize(x, xi, None, bits)
    q, sat, v = info["q"].reshape(-1)[:30 * 32].reshape(30, 32), info["sat"][:30 * 32].reshape(30, 32), info["v"][:30 * 32].reshape(30, 32)
    eb = scales[:15].astype(int)
    assert np.array_equal(scales[:15], scales[15:30])                        # the second copy is the first
    assert eb[0] == 0 and not q[0].any()                                     # all zero
    assert eb[1] == 127 - (bits - 2) and q[1, 5] == 2 ** (bits - 2)          # amax = 1.0 = 2^(bits-2) scales
    assert eb[2] == 117 and q[2, 3] == qm and q[2, 9] == -qm and not sat[2].any()      # just below the edge
    assert eb[3] == 117 and sat[3, 0] and sat[3, 1] and sat[3, 2] and sat[3, 30] and not sat[3, 31] and q[3, 0] == qm and q[3, 1] == -qm
    assert eb[4] == 117 and q[4, :12].tolist() == [0, 2, 2, 4, 4, 6, 0, -2, -2, -4, -4, -6]      # ties go to the even neighbour
    assert eb[5] == 0 and not q[5].any() and np.any(np.signbit(v[5])) and np.any(~np.signbit(v[5]))
    assert eb[7] == 0 and sorted(set(q[7].tolist())) == [-2, -1, 0, 1, 2]      # subnormals: codes up to +-2 at scale 2^-127
    assert eb[8] == 0 and q[8].any()                                         # clamped at 0
    assert eb[9] == 254 - (bits - 2) and np.abs(q[9]).max() >= 2 ** (bits - 2)
    assert eb[10] == 255 and np.isinf(v[10, 4]) and np.isinf(v[10, 20]) and eb[11] == 255 and eb[12] < 255 and eb[13] == 255 and eb[14] == 255
    assert nbad == 8
    assert Q.edge_blocks(bits, 31, 1)[0].size == 15 * 32 + 31 < Q.CHUNK      # every block on the partial-chunk path


def test_pack_unpack_round_trip():
    rng = np.random.RandomState(5)
    for bits in Q.BITS:
        qm = Q.qmax(bits)
        for n in (1, 2, 3, 31, 33, 4103):                                    # odd n: the last 4-bit byte holds one code and a zero nibble
            q = rng.randint(-qm, qm + 1, size=n).astype(np.int32)
            q[:min(n, 2)] = [qm, -qm][:min(n, 2)]
            by = Q.pack(q, bits)
            assert by.dtype == np.uint8 and by.size == Q.code_bytes(bits, n)
            assert np.array_equal(Q.unpack(by, bits, n), q)
            if bits == 4 and n % 2:
                assert by[-1] >> 4 == 0
    assert Q.pack([-1, 7, -7], 4).tolist() == [0x7F, 0x09] and Q.pack([-1, 127, -127], 8).tolist() == [0xFF, 0x7F, 0x81]


@pytest.mark.parametrize("bits", Q.BITS)
def test_error_feedback_telescopes(bits):
    """Five rounds with the same x and x_i, the residual carried: sum_t dq_t + e_5 equals 5 d, d = fl(x_i - x), up to the float32 rounding
    of the additions fl(d + e_{t-1}) alone.

    Derivation.  v_t = fl(d + e_{t-1}) = d + e_{t-1} + rho_t with |rho_t| <= U |v_t| (U = 2^-24: one rounding, relative to the result).
    The format gives dq_t + e_t = v_t EXACTLY (a finite block).  Summing over t = 1..T with e_0 = 0:
        sum_t dq_t = sum_t (d + e_{t-1} + rho_t - e_t) = T d - e_T + sum_t rho_t,
    so |sum_t dq_t + e_T - T d| = |sum_t rho_t| <= U sum_t |v_t|.  The test evaluates the left side in fp64, whose own rounding adds at
    most (T + 2) 2^-53 times the sum of the magnitudes added."""
    T = 5
    x, xs = Q.inputs(4103, 2)
    xi = xs[1]
    d = Q.value_to_send(x, xi).astype(f64)
    e = np.zeros(x.size, dtype=f32)
    total, vsum, mags = np.zeros(x.size, dtype=f64), np.zeros(x.size, dtype=f64), np.zeros(x.size, dtype=f64)
    for _ in range(T):
        codes, scales, e, nbad, info = Q.quantize(x, xi, e, bits)
        assert nbad == 0
        dq = Q.dequantize(codes, scales, bits, x.size).astype(f64)
        total += dq
        mags += np.abs(dq)
        vsum += np.abs(info["v"].astype(f64))
    lhs = total + e.astype(f64) - T * d
    bound = Q.U * vsum + (T + 2) * 2.0 ** -53 * (mags + np.abs(e.astype(f64)) + T * np.abs(d))
    print("bits=%d: worst |telescoped error| / bound %.3f" % (bits, float(np.max(np.abs(lhs) / np.maximum(bound, 1e-300)))))
    assert np.all(np.abs(lhs) <= bound)
    assert np.any(e != 0)
    # without feedback the same five rounds drift by five times the one-round error: the feedback is what the bound is about
    c0, s0, _, _, _ = Q.quantize(x, xi, None, bits)
    drift = np.abs(T * Q.dequantize(c0, s0, bits, x.size).astype(f64) - T * d)
    assert np.max(drift) > 100 * np.max(np.abs(lhs))


def test_aggregate_restatement_matches_fp64_on_exact_weights():
    """weights that are powers of two make every product exact: the float32 chain equals the fp64 sum wherever no addition rounds"""
    n = 1023
    x, xs = Q.inputs(n, 3)
    ups = [Q.quantize(x, a, None, 8)[:2] for a in xs]
    ws = [0.5, 0.25, 0.25]
    got = Q.aggregate(None, None, ups, ws, 8, n, False)
    ref = sum(w * Q.dequantize(c, s, 8, n).astype(f64) for (c, s), w in zip(ups, ws))
    assert np.all(np.abs(got.astype(f64) - ref) <= 2 * Q.U * np.abs(ref) + 1e-300)
    acc = Q.aggregate(x.copy(), x, ups, ws, 8, n, True)                       # accumulate and base both in use
    assert np.all(np.abs(acc.astype(f64) - (2 * x.astype(f64) + ref)) <= 4 * Q.U * (2 * np.abs(x.astype(f64)) + np.abs(ref)) + 1e-300)
    ch = Q.chained(x, ups * 3, [1.0 / 9] * 9, 8, n)                           # 9 uploads: two groups
    assert np.all(np.isfinite(ch))


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_header_ctypes_table_and_library_carry_the_symbols_and_byte_counts(built_lib):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "fedfr_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(fedfr_[a-z0-9_]+)\s*\(", src))
    out = subprocess.run(["nm", "-D", "--defined-only", built_lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = set(re.findall(r"\sT\s+(fedfr_[a-z0-9_]+)", out))
    for s in NEW_SYMBOLS:
        assert s in declared and s in built_lib.SIGNATURES and s in exported, s
    lib = built_lib.lib()
    for n in Q.SIZES + (0, 2, 64, 65, 65156160, Q.BIG):
        assert lib.fedfr_delta_scale_bytes(n) == Q.scale_bytes(n) == (n + 31) // 32
        for bits in Q.BITS:
            assert lib.fedfr_delta_code_bytes(bits, n) == Q.code_bytes(bits, n)
        for bits in (0, 1, 2, 5, 16, -4):
            assert lib.fedfr_delta_code_bytes(bits, n) == 0
    n = 65156160                                                             # iresnet100: 8.25 and 4.25 bits per parameter
    assert (lib.fedfr_delta_code_bytes(8, n) + lib.fedfr_delta_scale_bytes(n)) * 8 == int(8.25 * n)
    assert (lib.fedfr_delta_code_bytes(4, n) + lib.fedfr_delta_scale_bytes(n)) * 8 == int(4.25 * n)


def _aligned(nbytes, off=0):
    """(keep-alive array, address) of a host buffer whose address is 16-byte aligned plus ``off``"""
    raw = np.zeros(nbytes + 32, dtype=np.uint8)
    a = raw.ctypes.data
    return raw, (a + 15) // 16 * 16 + off


def test_argument_errors_are_host_side(built_lib):
    """every refused call returns FEDFR_ERR_ARG with a message naming the function (and the offending value) BEFORE any HIP call: host
    pointers serve, no GPU is needed, and nothing is written.  n = 0 with valid arguments is a no-op."""
    lib = built_lib.lib()
    err_arg = int(re.search(r"#define FEDFR_ERR_ARG \((-?\d+)\)", open(os.path.join(REPO, "include", "fedfr_hip.h")).read()).group(1))
    n = 64
    keep = [_aligned(4 * n) for _ in range(4)] + [_aligned(n) for _ in range(3)]
    x, xi, e, dst, codes, scales, cnt = [a for _, a in keep]
    vp = C.c_void_p

    def refused(rc, *words):
        assert rc == err_arg, rc
        msg = lib.fedfr_last_error_string().decode()
        for w in words:
            assert w in msg, msg

    quant = lib.fedfr_delta_quantize
    for bits in (0, 5, 16, -8):
        refused(quant(x, xi, e, codes, scales, bits, n, cnt, None), "delta_quantize", "bits=%d" % bits)
    refused(quant(None, xi, e, codes, scales, 8, n, cnt, None), "delta_quantize", "null")
    refused(quant(x, None, e, codes, scales, 8, n, cnt, None), "delta_quantize", "null")
    refused(quant(x, xi, e, None, scales, 4, n, cnt, None), "delta_quantize", "null")
    refused(quant(x, xi, e, codes, None, 4, n, cnt, None), "delta_quantize", "null")
    for args in ((x + 4, xi, e, codes, scales), (x, xi + 8, e, codes, scales), (x, xi, e + 4, codes, scales), (x, xi, e, codes + 4, scales),
                 (x, xi, e, codes, scales + 1), (x, xi, None, codes + 8, scales)):
        refused(quant(*args, 8, n, cnt, None), "delta_quantize", "aligned")
    refused(quant(x, xi, e, codes, scales, 8, n, cnt + 2, None), "delta_quantize", "aligned")
    assert quant(x, xi, e, codes, scales, 8, 0, cnt, None) == 0              # n = 0: nothing to do, nothing launched
    assert quant(x, xi, None, codes, scales, 4, 0, None, None) == 0

    aggr = lib.fedfr_delta_aggregate
    ws = (C.c_float * 9)(*([0.125] * 9))

    def arr(ps):
        return (vp * max(len(ps), 1))(*ps)

    cs, ss = arr([codes] * 9), arr([scales] * 9)
    for bits in (0, 6, 32):
        refused(aggr(dst, None, cs, ss, ws, 2, bits, n, 0, None), "delta_aggregate", "bits=%d" % bits)
    for k in (0, 9, -1, 100):
        refused(aggr(dst, None, cs, ss, ws, k, 8, n, 0, None), "delta_aggregate", "k=%d" % k)
    refused(aggr(None, None, cs, ss, ws, 2, 8, n, 0, None), "delta_aggregate", "null")
    refused(aggr(dst, None, None, ss, ws, 2, 8, n, 0, None), "delta_aggregate", "null")
    refused(aggr(dst, None, cs, None, ws, 2, 8, n, 0, None), "delta_aggregate", "null")
    refused(aggr(dst, None, cs, ss, None, 2, 8, n, 0, None), "delta_aggregate", "null")
    refused(aggr(dst, None, arr([codes, None, codes]), ss, ws, 3, 8, n, 0, None), "delta_aggregate", "code buffer 1 is null")
    refused(aggr(dst, None, cs, arr([scales, scales, None]), ws, 3, 4, n, 0, None), "delta_aggregate", "scale buffer 2 is null")
    refused(aggr(dst + 4, None, cs, ss, ws, 2, 8, n, 0, None), "delta_aggregate", "aligned")
    refused(aggr(dst, x + 8, cs, ss, ws, 2, 8, n, 0, None), "delta_aggregate", "aligned")
    refused(aggr(dst, x, arr([codes, codes + 4]), ss, ws, 2, 8, n, 1, None), "delta_aggregate", "aligned")
    assert aggr(dst, x, cs, ss, ws, 8, 8, 0, 1, None) == 0                   # n = 0
    assert aggr(dst, None, arr([codes, codes]), arr([scales + 1, scales + 3]), ws, 2, 4, 0, 0, None) == 0      # scale bytes need no alignment here
    for raw, _ in keep:
        assert not raw.any()                                                 # nothing was written


def test_delta_kernels_use_no_scratch_memory(built_lib):
    """every ``delta_`` kernel (2 widths x feedback on / off quantisers, 2 widths x K = 1..8 aggregates; both storage builds): the eight
    elements of a lane are registers and the kernels are bandwidth-bound, so scratch memory would mean an array indexed at run time"""
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(REPO, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    ks = kr.kernels(built_lib.LIB_PATH)
    bf16 = os.path.join(os.path.dirname(built_lib.LIB_PATH), "libfedfr_hip_bf16.so")
    if os.path.exists(bf16) and os.path.basename(built_lib.LIB_PATH) != "libfedfr_hip_bf16.so":
        ks.update({"bf16:" + k: v for k, v in kr.kernels(bf16).items()})
    builds = 2 if any(k.startswith("bf16:") for k in ks) else 1
    dq = {n: r for n, r in ks.items() if "delta_quantize_kernel" in n}
    da = {n: r for n, r in ks.items() if "delta_aggregate_kernel" in n}
    assert len(dq) == 4 * builds and len(da) == 16 * builds, (len(dq), len(da))
    bad = [(n, r) for n, r in list(dq.items()) + list(da.items()) if r["scratch"]]
    assert not bad, bad
    assert max(r["vgpr"] for r in list(dq.values()) + list(da.values())) <= 128      # at least two waves per SIMD


# ---- Python surface ----------------------------------------------------------------------------------------------------------------------
def test_compressor_and_fedcompressed_refuse_what_they_cannot_serve(built_lib):
    from fedfr_amd import compress, server
    from fedfr_amd.client import FlatStateDict
    for bad in (0, 2, 5, 16, "8", None, 8.0, True):
        with pytest.raises(ValueError, match="compress_bits"):
            compress.DeltaCompressor(bad)
    comp = compress.DeltaCompressor()
    assert comp.bits == 8 and comp.error_feedback and comp.residual is None
    cpu = FlatStateDict.from_flat((torch.zeros(8), torch.zeros(0), torch.zeros(0, dtype=torch.int64)), [], [])
    with pytest.raises(RuntimeError, match="GPU"):
        comp.compress(cpu, cpu)                                               # FlatStateDicts, but not on the GPU
    with pytest.raises(RuntimeError, match="FlatStateDict"):
        comp.compress({"w": torch.zeros(8)}, cpu)
    with pytest.raises(RuntimeError, match="FlatStateDict"):
        comp.compress(cpu, {"w": torch.zeros(8)})
    assert comp.residual is None                                              # nothing was allocated for a refused call
    up = compress.CompressedDelta(torch.zeros(8, dtype=torch.uint8), torch.zeros(1, dtype=torch.uint8), 8, 8, torch.zeros(3), torch.zeros(2, dtype=torch.int64),
                                  torch.zeros(1, dtype=torch.int32))
    assert up.nbytes == 8 + 1 + 12 + 16 and up.dense_nbytes == 32 + 12 + 16 and up.ratio == up.nbytes / up.dense_nbytes and up.nonfinite_count() == 0
    with pytest.raises(RuntimeError, match="FlatStateDict"):
        server.FedCompressed({"w": torch.zeros(8)}, [up], [1.0])
    with pytest.raises(RuntimeError, match="CompressedDelta"):
        server.FedCompressed(cpu, [cpu], [1.0])
    with pytest.raises(RuntimeError, match="CompressedDelta"):
        server.FedCompressed(cpu, [], [])
    with pytest.raises(RuntimeError, match="weights"):
        server.FedCompressed(cpu, [up, up], [1.0])
    with pytest.raises(ValueError, match="clip_norm"):
        server.FedCompressed(cpu, [up], [1.0], server.ServerOptimizer("AVGM", clip_norm=1.0))
    with pytest.raises(ValueError, match="robust"):
        server.FedCompressed(cpu, [up], [1.0], server.RobustAggregator("CoordMedian"))
    with pytest.raises(RuntimeError, match="GPU"):
        server.FedCompressed(cpu, [up], [1.0])


def test_server_train_refuses_compression_settings_before_any_client_trains():
    from fedfr_amd import server

    def world(aggr, nclients, **extra):
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

    for kind in sorted(server.ROBUST_ALG_KINDS):
        with pytest.raises(ValueError, match=r"compress_bits=8.*%s" % kind):
            world(kind, 5, compress_bits=8).train()                           # a robust rule needs whole states
    for aggr in ("FedAvg", "FedAdam"):
        with pytest.raises(ValueError, match=r"compress_bits=4.*clip_norm=2.5"):
            world(aggr, 3, compress_bits=4, clip_norm=2.5).train()
    for bad in (1, 2, 3, 5, 16, 32, -8, "8", 8.0):
        with pytest.raises(ValueError, match=r"compress_bits.*%s" % re.escape(repr(bad))):
            world("FedAvg", 3, compress_bits=bad).train()
    for aggr, extra in (("FedAvg", {"compress_bits": 8}), ("FedProx", {"compress_bits": 4}), ("FedAvgM", {"compress_bits": 8, "clip_norm": 0.0}),
                        ("FedYogi", {"compress_bits": 4, "error_feedback": False}), ("FedAvg", {"compress_bits": 0, "clip_norm": 2.5}),
                        ("CoordMedian", {"compress_bits": 0}), ("FedAvg", {"compress_bits": None})):
        with pytest.raises(AssertionError, match="the round has started"):    # served: the round starts (and meets the stub)
            world(aggr, 3, **extra).train()
