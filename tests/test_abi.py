"""CPU-side checks of the drop-in boundary: the C-ABI library builds/loads without a GPU and exports exactly the
symbols include/fedfr_hip.h declares; the ctypes table in fedfr_amd/_C.py covers all of them."""
import os
import re
import subprocess

import pytest

from conftest import REPO

HEADER = os.path.join(REPO, "include", "fedfr_hip.h")


def header_symbols():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(fedfr_[a-z0-9_]+)\s*\(", src)))


@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__ as ge
    ge.build()
    from fedfr_amd import _C
    return _C


def test_header_and_ctypes_table_agree(built_lib):
    syms = header_symbols()
    assert len(syms) >= 45
    assert sorted(built_lib.SIGNATURES.keys()) == syms


def test_library_exports_every_declared_symbol(built_lib):
    out = subprocess.run(["nm", "-D", "--defined-only", built_lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = set(re.findall(r"\sT\s+(fedfr_[a-z0-9_]+)", out))
    missing = [s for s in header_symbols() if s not in exported]
    assert not missing, missing
    lib = built_lib.lib()
    assert lib.fedfr_version() >= 100
    assert lib.fedfr_last_error_string() is not None


def test_plan_layout_matches_reference_inventory(built_lib):
    """The C plan (host-only code, runs on CPU) reproduces the reference's parameter inventory."""
    import ctypes as C
    lib = built_lib.lib()
    for layers, ntens, nparam, nbuf in (((3, 13, 30, 3), 925, 65156160, 69786), ((3, 4, 14, 3), 475, 43590848, 38223)):
        h = lib.fedfr_net_create((C.c_int * 4)(*layers), 128, 112, 512)
        assert h
        q = C.c_longlong()
        def query(k):
            assert lib.fedfr_net_query(h, k, C.byref(q)) == 0
            return q.value
        assert query(built_lib.Q_NUM_TENSORS) == ntens
        assert query(built_lib.Q_PARAM_COUNT) == nparam
        assert query(built_lib.Q_BUFFER_COUNT) + query(built_lib.Q_NBT_COUNT) == nbuf
        assert query(built_lib.Q_FC_IN) == 25088
        assert query(built_lib.Q_ACT_BYTES) < 16 * 2 ** 30 and query(built_lib.Q_WS_BYTES) < 4 * 2 ** 30    # fits 288 GB easily
        lib.fedfr_net_destroy(h)
    # bad arguments are reported through the error string, not a crash
    assert not lib.fedfr_net_create((C.c_int * 4)(2, 2, 2, 2), 0, 112, 512)
    assert b"net_create" in lib.fedfr_last_error_string()
    assert lib.fedfr_set_option(b"no_such_option", 1) != 0
    # fedfr_bn_finalize serves C % 8 == 0 only, like every other [M][C] entry point: C = 12 is an argument error (checked before any HIP call)
    buf = (C.c_float * 64)()
    err_arg = int(re.search(r"#define FEDFR_ERR_ARG \((-?\d+)\)", open(HEADER).read()).group(1))
    assert lib.fedfr_bn_finalize(buf, 2, 12, 8.0, buf, buf, None, None, 0.1, 1e-5, buf, buf, buf, buf, None, None) == err_arg
    msg = lib.fedfr_last_error_string()
    assert b"bn_finalize" in msg and b"12" in msg, msg


def test_rowslab_test_wrappers_check_their_tables_on_the_host(built_lib):
    """The by-value tables of fedfr_prelu_bwd_finalize_multi (1 ... 64 entries, C % 8 == 0) and fedfr_bn_eval_coeffs (1 ... 160 entries) are
    filled and checked on the host before any HIP call, and the row queries are the restated slab formula (tests/rowslab_cases.py)."""
    import ctypes as C
    import rowslab_cases as K
    lib = built_lib.lib()
    err_arg = int(re.search(r"#define FEDFR_ERR_ARG \((-?\d+)\)", open(HEADER).read()).group(1))
    buf = (C.c_float * 64)()
    for n, ch in ((0, 8), (K.MAX_PRELU_FIN + 1, 8), (1, 12)):
        m = max(n, 1)
        rc = lib.fedfr_prelu_bwd_finalize_multi(buf, buf, n, (C.c_ulonglong * m)(), (C.c_longlong * m)(), (C.c_longlong * m)(), (C.c_int * m)(*[2] * m),
                                                (C.c_int * m)(*[ch] * m), (C.c_int * m)(*[2] * m), None)
        assert rc == err_arg and b"prelu_bwd_finalize_multi" in lib.fedfr_last_error_string(), (n, ch)
    one = (C.c_int * 1)(8)
    for n in (0, K.MAX_BN_EVAL + 1):
        assert lib.fedfr_bn_eval_coeffs(buf, buf, buf, n, one, one, one, one, one, one, 1e-5, None) == err_arg
        assert b"bn_eval_coeffs" in lib.fedfr_last_error_string()
    assert lib.fedfr_prelu_bwd_pass(buf, buf, buf, None, buf, 100, 64, None, buf, buf, None) == err_arg        # an addend without gsum
    assert lib.fedfr_prelu_bwd_finalize(buf, 2, 12, buf, buf, None) == err_arg
    for M, ch in ((1, 8), (3000, 64), (1000, 96), (777, 512), (512 * 32 + 1, 512), (100, 2048), (128 * 112 * 112, 64)):
        assert lib.fedfr_prelu_bwd_rows(M, ch) == K.geometry(M, ch, K.PRELU_BLOCKS)["grid"]
        assert lib.fedfr_bn_apply_stat_rows(M, ch) == K.geometry(M, ch, K.APPLY_BLOCKS)["grid"]
    # the producers that hand fedfr_bn_finalize more than 1024 rows at the bench batch (128): the stem conv and the 128-pixel-tiled conv epilogues of the
    # 56x56 and 28x28 maps (stride-2 3x3 and 1x1 downsample convs); bn_apply / prelu_bwd_pass rows are capped at 1024 / 512
    assert lib.fedfr_stem_stat_rows(128, 112) == K.stem_stat_rows(128, 112, 112) == 25088
    assert [lib.fedfr_conv2d_stat_rows(128, hw, c) for hw, c in ((56, 64), (28, 128), (14, 256), (7, 512))] == [6272, 1568, 392, 98]


def test_documented_options_exist_and_unknown_ones_are_errors(built_lib):
    """Every switch the header's fedfr_set_option comment names is one the library accepts (host-only state: no GPU needed), an unknown
    name is an error with a message, and setting a switch to its documented default is harmless."""
    src = open(HEADER).read()
    doc = src[src.index("Kernel-choice switches"):src.index("int fedfr_set_option")]
    names = sorted(set(re.findall(r'"([a-z0-9_]+)"', doc)))
    assert len(names) >= 15 and "nt_glds" in names and "bn_sliced" in names
    lib = built_lib.lib()
    opts = built_lib.options()                       # {name: (value, default)} from fedfr_option_info: the library's own table
    assert set(names) == set(opts), ("the header's comment and the library's option table must list the same switches", sorted(set(names) ^ set(opts)))
    for n in names:
        assert lib.fedfr_set_option(n.encode(), opts[n][1]) == 0, n          # setting a switch to its default is harmless
    assert built_lib.options_non_default() == {} or os.environ.get("FEDFR_OPTIONS")
    assert "dbg_skip" not in opts                    # wrong-results switches exist only in -DFEDFR_DEBUG builds
    assert lib.fedfr_set_option(b"no_such_option", 1) != 0
    assert b"no_such_option" in lib.fedfr_last_error_string() or len(lib.fedfr_last_error_string()) > 0


def test_hot_kernels_do_not_spill(built_lib):
    """No instantiation of the hot kernels may use scratch memory (= register spills): they are shared templates, several sit at the
    256-register limit, and an edit that pushes one over it passes every parity test while costing 50 % of that kernel's time (round 3: a
    new epilogue branch in conv_glds_impl.h took the two-tiles 28x28 conv from 254 VGPRs to 256 + 128 B of scratch per lane, 34 -> 51 us,
    +0.85 ms per step).  Read from the code objects inside the built library (tools/kernel_resources.py): no GPU needed."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(REPO, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    ks = kr.kernels(built_lib.LIB_PATH)
    bf16 = os.path.join(os.path.dirname(built_lib.LIB_PATH), "libfedfr_hip_bf16.so")      # the bf16-storage build of the same kernels: same rule
    if os.path.exists(bf16) and os.path.basename(built_lib.LIB_PATH) != "libfedfr_hip_bf16.so":
        ks.update({"bf16:" + k: v for k, v in kr.kernels(bf16).items()})
    assert len(ks) > 100, len(ks)
    hot = ("conv3x3_glds_kernel", "conv3x3_c64p_kernel", "wgrad9_kernel", "wgrad9p_kernel", "gemm_nt_glds_kernel", "gemm_tn_glds",
           "gemm_nt_kernel", "bn_apply_s_kernel", "bn_bwd_reduce_s_kernel", "bn_bwd_apply_s_kernel", "bn_apply_kernel", "bn_bwd_reduce_kernel",
           "bn_bwd_apply_kernel", "sgd_kernel", "stem_fwd_kernel", "stem_wgrad_mfma_kernel", "prelu_bwd_pass_kernel", "fedavg_multi_kernel")
    seen = {h: 0 for h in hot}
    bad = []
    for name, r in ks.items():
        for h in hot:
            if h in name:
                seen[h] += 1
                if r["scratch"]:
                    bad.append((name, r))
    assert all(seen.values()), [h for h, n in seen.items() if not n]
    assert not bad, bad


def test_sphere_plan_selectors_and_fp32_path_refusal(built_lib):
    """Host-only: fedfr_net_act_info on a sphnet plan answers per UNIT (forward order: stage head, then u1, u2 of each block) with the selectors 0 input,
    1 c, 2 t, 3 dz and refuses everything else with a message; the fp32 validation path has no sphnet plan — its size queries return 0 and its
    forward / backward refuse a sphere plan before any layout computation or launch (dummy host pointers: the calls fail their checks first)."""
    import ctypes as C
    import sphnet_cases as SC
    lib = built_lib.lib()
    err_arg = int(re.search(r"#define FEDFR_ERR_ARG \((-?\d+)\)", open(HEADER).read()).group(1))
    off, rows, ch = C.c_longlong(), C.c_int(), C.c_int()

    def info(h, block, which):
        rc = lib.fedfr_net_act_info(h, block, which, C.byref(off), C.byref(rows), C.byref(ch))
        return rc, off.value, rows.value, ch.value
    for type_, B in ((20, 5), (64, 1)):
        h = lib.fedfr_net_create_sphere(type_, B)
        assert h
        net = SC.Net(type_, B)
        prev_t, seen = None, set()
        for u in net.units:
            i0, c, t, dz = (info(h, u.idx, w) for w in range(4))
            assert (i0[0], c[0], t[0], dz[0]) == (0, 0, 0, 0)
            assert i0[2:] == (B * u.hin * u.hin, u.cin), (u.idx, i0)             # the stem input is the padded 64-channel image
            assert c[2:] == t[2:] == dz[2:] == (B * u.hout * u.hout, u.cout)
            assert i0[1] == (0 if prev_t is None else prev_t)                    # a unit reads the activation in front of it
            assert c[1] % 8 == 0 and t[1] >= c[1] + c[2] * c[3] and dz[1] % 128 == 0
            assert not {c[1], t[1]} & seen
            seen |= {c[1], t[1]}
            prev_t = t[1]
        for block, which in ((-1, 0), (-1, 2), (len(net.units), 0), (0, 4), (0, -1), (3, 7)):
            assert info(h, block, which)[0] == err_arg, (block, which)
            assert b"net_act_info" in lib.fedfr_last_error_string()
        assert lib.fedfr_net_f32_arena_floats(h) == 0 and lib.fedfr_net_f32_ws_floats(h) == 0
        buf = (C.c_float * 64)()
        assert lib.fedfr_net_f32_forward(h, buf, buf, buf, buf, buf, buf, 1, None) == err_arg
        assert b"net_f32_forward" in lib.fedfr_last_error_string() and b"sphnet" in lib.fedfr_last_error_string()
        assert lib.fedfr_net_f32_backward(h, buf, buf, buf, buf, buf, None) == err_arg
        assert b"net_f32_backward" in lib.fedfr_last_error_string() and b"sphnet" in lib.fedfr_last_error_string()
        lib.fedfr_net_destroy(h)


def test_debug_capture_detail_and_bn_info_are_host_only_and_check_their_arguments(built_lib):
    """Host-only: fedfr_net_debug_capture_elems sizes the capture buffer of either detail level from the block table, fedfr_net_bn_info lists the 2-D
    BatchNorms in state_dict order with the offsets of their save rows; bad levels, indices, null pointers and sphnet plans are argument errors with a message."""
    import ctypes as C
    import iresnet_cases as IC
    lib = built_lib.lib()
    err_arg = int(re.search(r"#define FEDFR_ERR_ARG \((-?\d+)\)", open(HEADER).read()).group(1))
    q, c, off, name = C.c_longlong(), C.c_int(), C.c_longlong(), C.create_string_buffer(64)
    for layers, B in (((2, 2, 2, 2), 5), ((1, 1, 3, 1), 2)):
        h = lib.fedfr_net_create((C.c_int * 4)(*layers), B, 112, 512)
        assert h
        net = IC.Net(layers, B)
        want0 = sum(B * b.hout * b.hout * b.cout for b in net.blocks) + B * 112 * 112 * 64
        want1 = want0 + B * net.hw * net.C + sum(B * (b.hout * b.hout * b.cout + 2 * b.hin * b.hin * b.cout + b.hin * b.hin * b.cin +
                                 (b.hout * b.hout * (b.cout + b.cin) if b.has_ds else 0)) for b in net.blocks)
        for level, want in ((0, want0), (1, want1)):
            assert lib.fedfr_net_debug_capture_elems(h, level, C.byref(q)) == 0 and q.value == want, (level, q.value, want)
        for level in (-1, 2):
            assert lib.fedfr_net_debug_capture_elems(h, level, C.byref(q)) == err_arg and b"net_debug_capture_elems" in lib.fedfr_last_error_string()
            assert lib.fedfr_net_debug_capture_detail(level) == err_arg and b"net_debug_capture_detail" in lib.fedfr_last_error_string()
        assert lib.fedfr_net_debug_capture_elems(h, 0, None) == err_arg and lib.fedfr_net_debug_capture_elems(None, 0, C.byref(q)) == err_arg
        assert lib.fedfr_net_debug_capture_detail(1) == 0 and lib.fedfr_net_debug_capture_detail(0) == 0
        table = net.bn_table()
        assert lib.fedfr_net_query(h, built_lib.Q_NUM_BN, C.byref(q)) == 0 and q.value == len(table)
        want_off = 0
        for i, (n, ch) in enumerate(table):
            assert lib.fedfr_net_bn_info(h, i, name, 64, C.byref(c), C.byref(off)) == 0
            assert (name.value.decode(), c.value, off.value) == (n, ch, want_off), (i, name.value, c.value, off.value)
            want_off += 4 * ch
        assert lib.fedfr_net_query(h, built_lib.Q_ACT_FLOAT_OFF_BYTES, C.byref(q)) == 0 and q.value % 256 == 0 and q.value > 0
        assert lib.fedfr_net_query(h, built_lib.Q_ACT_BYTES, C.byref(off)) == 0 and q.value + 4 * (want_off + 4 * 512 + B * 512 + 2 * 512) <= off.value
        for i in (-1, len(table)):
            assert lib.fedfr_net_bn_info(h, i, name, 64, C.byref(c), C.byref(off)) == err_arg and b"net_bn_info" in lib.fedfr_last_error_string()
        assert lib.fedfr_net_bn_info(h, 0, None, 64, C.byref(c), C.byref(off)) == err_arg
        assert lib.fedfr_net_bn_info(h, 0, name, 0, C.byref(c), C.byref(off)) == err_arg
        assert lib.fedfr_net_bn_info(h, 0, name, 64, None, C.byref(off)) == err_arg
        lib.fedfr_net_destroy(h)
    h = lib.fedfr_net_create_sphere(20, 2)
    assert h
    assert lib.fedfr_net_query(h, built_lib.Q_NUM_BN, C.byref(q)) == 0 and q.value == 0
    assert lib.fedfr_net_bn_info(h, 0, name, 64, C.byref(c), C.byref(off)) == err_arg and b"sphnet" in lib.fedfr_last_error_string()
    assert lib.fedfr_net_debug_capture_elems(h, 0, C.byref(q)) == err_arg and b"sphnet" in lib.fedfr_last_error_string()
    lib.fedfr_net_destroy(h)


def test_sphnet_refuses_the_fp32_validation_switch(built_lib):
    """`validation_fp32` is IResNet's: a sphnet raises when it is set, before the library is ever called with a sphere plan."""
    from fedfr_amd import backbones
    m = backbones.sphnet(type=20)
    assert m.validation_fp32 is False
    m.validation_fp32 = False
    with pytest.raises(NotImplementedError, match="validation"):
        m.validation_fp32 = True
    assert m.validation_fp32 is False
