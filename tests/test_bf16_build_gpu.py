"""The direct kernel parity files, again, on the bf16 build (libfedfr_hip_bf16.so: the same kernels under -DFEDFR_FP16=0).

Those files take their storage type from the loaded library, their case modules have bf16 branches and their CPU proofs
are parametrised over both types — but the library is chosen at import, so the `-m gpu` run itself only ever loads the fp16 one.  Each row
of BF16_FILES is run here in a fresh child process that loads the bf16 library (tests/bf16_child.py): the same tests at the same shapes,
against the same float64 references, at the bounds the modules' formulas give for u16 = 2^-8.  This is what holds the bf16-only device code
to a per-kernel bound: prelu_pos's fp32-FMA threshold form (epi_mfma.h), the 0x3f80 `ones` fragments, the bf16 MFMA of wgrad9p.hip,
gemm_dev.h and stem.hip, f2bf / pack_bf2 / unpack8 of common.h, and the loss-scale-1 paths.

tests/test_host_cpu.py::test_every_storage_typed_gpu_file_runs_on_bf16 keeps the table complete: a GPU test file that reads the storage type
must stand in BF16_FILES, COVERED_ELSEWHERE or EXCLUDED."""
import pytest

import bf16_child

pytestmark = pytest.mark.gpu

# The eight children add more than a quarter of the suite's time, so the children leave out the tests that touch no
# 16-bit storage at all: the same device code in both libraries.  Step file: the PartialFC selection (pfc_*: fp32 scores, integer indices),
# the fp32 row gather / scatter and the sampling chain built from them, the fp32 head helpers (contrastive, sgemm_colflag, class_accumulate,
# the ROC histogram) and fedavg_axpy (fp32 flat parameters).  Tail file: reduce_slabs (fp32 slabs), fedavg_i64 (integer buffers) and the
# PartialFC helpers pfc_rand / pfc_localize / pfc_positive (Philox words, integer labels).
STEP_K = ("not pfc_ and not rows_ and not partial_fc and not contrastive and not sgemm_colflag and not class_accumulate "
          "and not roc_histogram and not fedavg_axpy")
TAIL_K = "not reduce_slabs and not fedavg_i64 and not pfc_"

# file: (-k expression or "", timeout_s).  One child per row.  timeout_s = 3 x the file's wall time alone on the fp16 library, rounded up to
# the next 30 s, at least 120 s (a cold code-object load, and bf16's slower epilogue form).  Wall times of one run of each file alone on one
# MI355X, interpreter start included:
BF16_FILES = {
    "test_conv_branches_gpu.py": ("", 120),     # 138 tests: fp16 35.0 s, bf16 34.9 s
    "test_bn_sliced_gpu.py": ("", 120),         # 108 tests: fp16 19.3 s, bf16 18.1 s
    "test_tail_kernels_gpu.py": (TAIL_K, 120),  #  89 tests: fp16  5.2 s, bf16  5.5 s; 70 of them in the child
    "test_stem_chain_gpu.py": ("", 150),        #  15 tests: fp16 47.9 s, bf16 49.2 s
    "test_step_kernels_gpu.py": (STEP_K, 120),  # 119 tests: fp16  6.2 s, bf16  5.9 s; 50 of them in the child
    "test_sphnet_units_gpu.py": ("", 120),      #   6 tests: fp16 18.1 s, bf16 18.3 s
    "test_iresnet_units_gpu.py": ("", 120),     #  11 tests: fp16 38.3 s, bf16 36.7 s
    "test_net_passes_gpu.py": ("", 120),        #   2 tests: fp16  4.7 s, bf16  3.8 s
}

# files that read the storage type and are held on the bf16 build by a child of their own
COVERED_ELSEWHERE = {
    "test_rowslab_fwd_gpu.py": "test_bf16_build_in_a_child_process runs the file itself on the bf16 library",
    "test_e2e_gpu.py": "test_bf16_build_reference_parity_subset runs its reference-parity tests on the bf16 library",
    "test_block_gpu.py": "test_e2e_gpu.py::test_bf16_build_reference_parity_subset runs its block fixtures on the bf16 library",
}

# files that read the storage type and are NOT run on the bf16 build, each with its reason
EXCLUDED = {
    "test_kernels_gpu.py": "the older vs_torch layer: every entry point it calls has a direct float64 test in a BF16_FILES row or in "
                           "test_rowslab_fwd_gpu.py, except fedfr_sgemm and fedfr_fedavg_multi, which are fp32 only",
    "test_drift_gpu.py": "fp32 drift terms; the 16-bit mirror its SGD kernels write is the one store of sgd_kernel<UNSCALE, ANCHOR, CORR> that "
                         "test_step_kernels_gpu.py holds to the cast bit for bit (planted ties and subnormals) on both builds; the file "
                         "passed on the bf16 library when this table was written (81 tests, 43 s: too long for what it would add)",
    "test_multirank_gpu.py": "whole FedAvg rounds on thread ranks: it reads the storage type only to pick the bound between two summation orders",
}


@pytest.mark.parametrize("name", list(BF16_FILES), ids=[n[len("test_"):-len("_gpu.py")] for n in BF16_FILES])
def test_direct_file_on_the_bf16_build(name):
    k, timeout_s = BF16_FILES[name]
    bf16_child.run_on_bf16([name], k, timeout_s)
