"""Compressed client uploads with error feedback (a build extension: the reference's clients hand over full fp32 states).

A client sends ``Q(x_i - x + e_i)`` — 8- or 4-bit codes with one shared power-of-two scale byte per 32 parameters, the OCP microscaling
layout — and keeps the quantisation error ``e_i`` for the next round: 8.25 or 4.25 bits per parameter instead of 32.  The format is fixed
in include/fedfr_hip.h (``fedfr_delta_quantize``); the kernels are csrc/compress.hip; ``server.FedCompressed`` aggregates the uploads.
The BN running statistics and ``num_batches_tracked`` counters travel uncompressed (69,786 values for iresnet100): they are statistics,
not optimisation variables — the stance ``server.FedOpt`` takes.  Not provided: fp8 element types, top-k sparsification, and the RCCL
path (an all-gather of eight 8.25-bit payloads moves about what the ring all-reduce of one fp32 state already moves, so
``server.fedavg_all_reduce`` gains nothing at world 8 and is left alone)."""
from __future__ import annotations

from typing import Optional

import torch

from . import _C

f32 = torch.float32
COMPRESS_BITS = (4, 8)


def check_bits(bits, who: str = "compress") -> int:
    """``bits`` as an int; ValueError naming the value unless it is 4 or 8"""
    if isinstance(bits, bool) or not isinstance(bits, int) or bits not in COMPRESS_BITS:
        raise ValueError("%s: compress_bits must be 4 or 8 (got %r)" % (who, bits))
    return bits


class CompressedDelta:
    """One client's upload: ``codes`` and ``scales`` (uint8 device tensors in the format of include/fedfr_hip.h), ``bits``, the parameter
    count ``n``, the client's BN running statistics ``stats`` (fp32) and ``counters`` (int64) uncompressed, and ``nonfinite_blocks``: a
    DEVICE int32 holding the number of 32-element blocks whose value to send was NaN or infinite (they dequantise to NaN); it is read
    back only when ``nonfinite_count()`` is asked for.  ``table`` / ``layers`` describe the state the upload belongs to (FlatStateDict)."""

    def __init__(self, codes, scales, bits, n, stats, counters, nonfinite_blocks, table=None, layers=None):
        self.codes, self.scales, self.bits, self.n = codes, scales, int(bits), int(n)
        self.stats, self.counters, self.nonfinite_blocks = stats, counters, nonfinite_blocks
        self.table, self.layers = table, layers

    @property
    def nbytes(self) -> int:
        """bytes of the upload: codes, scale bytes, running statistics and counters"""
        return (self.codes.numel() + self.scales.numel() + self.stats.numel() * self.stats.element_size()
                + self.counters.numel() * self.counters.element_size())

    @property
    def dense_nbytes(self) -> int:
        """bytes of the fp32 state this upload replaces"""
        return 4 * self.n + self.stats.numel() * self.stats.element_size() + self.counters.numel() * self.counters.element_size()

    @property
    def ratio(self) -> float:
        return self.nbytes / self.dense_nbytes

    def nonfinite_count(self) -> int:
        """the counter, read back (a host synchronisation)"""
        return int(self.nonfinite_blocks.item())


class DeltaCompressor:
    """The compressor of ONE client.  It owns the client's residual ``e`` (flat fp32 on the device, allocated as zeros on first use to the
    parameter count, updated in place by every ``compress``; ``reset()`` drops it) when ``error_feedback`` is on; without it nothing is
    carried between rounds."""

    def __init__(self, bits: int = 8, error_feedback: bool = True):
        self.bits = check_bits(bits, "DeltaCompressor")
        self.error_feedback = bool(error_feedback)
        self.residual: Optional[torch.Tensor] = None

    def reset(self):
        self.residual = None

    def compress(self, global_state, client_state) -> CompressedDelta:
        """Q(x_i - x + e) of the PARAMETERS of ``client_state`` against ``global_state`` (GPU ``FlatStateDict``s) in one kernel pass that
        also leaves the new residual in place; statistics and counters are carried as they are."""
        from .client import FlatStateDict
        from .server import _check_states
        if not all(isinstance(s, FlatStateDict) and s.flat is not None for s in (global_state, client_state)):
            raise RuntimeError("fedfr_amd.DeltaCompressor: the global and the client state must be FlatStateDicts (client.flat_state_dict)")
        x, (xi, stats, counters) = global_state.flat[0], client_state.flat
        _check_states(x, [xi], "DeltaCompressor")
        n, dev = x.numel(), x.device
        if self.error_feedback:
            if self.residual is not None and (self.residual.numel() != n or self.residual.device != dev):
                raise RuntimeError("fedfr_amd.DeltaCompressor: the residual holds %d elements on %s, the parameters %d on %s; reset() first"
                                   % (self.residual.numel(), self.residual.device, n, dev))
            if self.residual is None:
                self.residual = torch.zeros(n, dtype=f32, device=dev)
        lib = _C.lib()
        codes = torch.empty(int(lib.fedfr_delta_code_bytes(self.bits, n)), dtype=torch.uint8, device=dev)
        scales = torch.empty(int(lib.fedfr_delta_scale_bytes(n)), dtype=torch.uint8, device=dev)
        bad = torch.zeros(1, dtype=torch.int32, device=dev)
        if n:
            _C.call("fedfr_delta_quantize", x.data_ptr(), xi.data_ptr(), _C.ptr(self.residual) if self.error_feedback else None, codes.data_ptr(),
                    scales.data_ptr(), self.bits, n, bad.data_ptr(), _C.stream())
        return CompressedDelta(codes, scales, self.bits, n, stats, counters, bad, client_state.table, client_state.layers)
