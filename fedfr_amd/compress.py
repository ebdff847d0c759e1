"""Compressed client uploads with error feedback (a build extension: the reference's clients hand over full fp32 states).

Two formats, both fixed in include/fedfr_hip.h, both with the residual of what was not sent kept by the client for the next round:

* block-scaled codes (``DeltaCompressor``): a client sends ``Q(x_i - x + e_i)`` — 8- or 4-bit codes with one shared power-of-two scale
  byte per 32 parameters, the OCP microscaling layout: 8.25 or 4.25 bits per parameter instead of 32 (``fedfr_delta_quantize``,
  csrc/compress.hip; ``server.FedCompressed`` aggregates the uploads).
* top-k sparsification (``TopKCompressor``): a client sends the ``keep`` largest-magnitude entries of ``x_i - x + e_i`` as sorted
  (index, value) pairs — 8 bytes per kept parameter, 0.08 bytes per parameter at 1 % — found by an exact radix select on the device
  (``fedfr_topk_sparsify``, csrc/sparse.hip; ``server.FedSparse`` aggregates the uploads).

The BN running statistics and ``num_batches_tracked`` counters travel uncompressed (69,786 values for iresnet100): they are statistics,
not optimisation variables — the stance ``server.FedOpt`` takes.  The server can clip either kind of upload by its norm as it will be
applied, and add the Gaussian mechanism's noise to the clipped sum (``server.UploadClip``, the ``clip`` / ``mech`` arguments of
``server.FedCompressed`` / ``server.FedSparse``, ``clip_uploads`` in ``Server.train``); the client's residual still follows what was
SENT, not what the clip let through.  Not provided: a clip on the client before quantisation, norms under secure aggregation (the masks
hide them by design), fp8 element types, quantising the kept values of a top-k upload, delta-coding its indices, and the RCCL path (an
all-gather of eight 8.25-bit payloads moves about what the ring all-reduce of one fp32 state already moves, so
``server.fedavg_all_reduce`` gains nothing at world 8 and is left alone)."""
from __future__ import annotations

import math
import numbers
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


# ---- top-k sparsification: csrc/sparse.hip --------------------------------------------------------------------------------------------------
def keep_count(n: int, ratio) -> int:
    """entries a top-k upload of ``n`` parameters holds at ``ratio``: min(n, max(1, ceil(ratio n))) for 0 < ratio <= 1; ValueError naming
    the value otherwise"""
    if isinstance(ratio, bool) or not isinstance(ratio, numbers.Real) or not (0.0 < float(ratio) <= 1.0):      # (NaN fails the comparison)
        raise ValueError("keep_count: topk_ratio must be a number in (0, 1] (got %r)" % (ratio,))
    return min(int(n), max(1, int(math.ceil(float(ratio) * int(n)))))


class SparseDelta:
    """One client's top-k upload: ``idx`` (int32 device tensor holding the uint32 indices, strictly ascending) and ``val`` (fp32, the values
    at those indices bit for bit), ``keep`` entries of ``n`` parameters, the client's BN running statistics ``stats`` (fp32) and
    ``counters`` (int64) uncompressed, and ``nonfinite``: a DEVICE int32 holding the number of ELEMENTS of the value to send that were
    NaN or infinite (they order above every finite value, so they are sent first); it is read back only when ``nonfinite_count()`` is
    asked for.  ``table`` / ``layers`` describe the state the upload belongs to (FlatStateDict)."""

    def __init__(self, idx, val, n, keep, stats, counters, nonfinite, table=None, layers=None):
        self.idx, self.val, self.n, self.keep = idx, val, int(n), int(keep)
        self.stats, self.counters, self.nonfinite = stats, counters, nonfinite
        self.table, self.layers = table, layers

    def _side_bytes(self) -> int:
        return self.stats.numel() * self.stats.element_size() + self.counters.numel() * self.counters.element_size()

    @property
    def nbytes(self) -> int:
        """bytes of the upload: 8 per kept entry, running statistics and counters"""
        return 8 * self.keep + self._side_bytes()

    @property
    def dense_nbytes(self) -> int:
        """bytes of the fp32 state this upload replaces"""
        return 4 * self.n + self._side_bytes()

    @property
    def ratio(self) -> float:
        return self.nbytes / self.dense_nbytes

    def nonfinite_count(self) -> int:
        """the counter, read back (a host synchronisation)"""
        return int(self.nonfinite.item())


class TopKCompressor:
    """The top-k compressor of ONE client.  It owns the client's residual ``e`` (flat fp32 on the device, allocated as zeros on first use to
    the parameter count, updated in place by every ``compress``; ``reset()`` drops it) when ``error_feedback`` is on, and the workspace of
    the selection (kept between rounds; without feedback it also holds the n values to select from)."""

    def __init__(self, ratio: float = 0.01, error_feedback: bool = True):
        keep_count(1, ratio)                                                  # ValueError naming the value
        self.ratio = float(ratio)
        self.error_feedback = bool(error_feedback)
        self.residual: Optional[torch.Tensor] = None
        self.workspace: Optional[torch.Tensor] = None

    def reset(self):
        self.residual = None

    def compress(self, global_state, client_state) -> SparseDelta:
        """the ``keep_count(n, ratio)`` largest-magnitude entries of x_i - x + e of the PARAMETERS of ``client_state`` against
        ``global_state`` (GPU ``FlatStateDict``s), stream-ordered with no host synchronisation; the new residual is left in place;
        statistics and counters are carried as they are."""
        from .client import FlatStateDict
        from .server import _check_states
        if not all(isinstance(s, FlatStateDict) and s.flat is not None for s in (global_state, client_state)):
            raise RuntimeError("fedfr_amd.TopKCompressor: the global and the client state must be FlatStateDicts (client.flat_state_dict)")
        x, (xi, stats, counters) = global_state.flat[0], client_state.flat
        _check_states(x, [xi], "TopKCompressor")
        n, dev = x.numel(), x.device
        if n >= 2 ** 31:
            raise RuntimeError("fedfr_amd.TopKCompressor: %d parameters; the indices of an upload are 31-bit" % n)
        if self.error_feedback:
            if self.residual is not None and (self.residual.numel() != n or self.residual.device != dev):
                raise RuntimeError("fedfr_amd.TopKCompressor: the residual holds %d elements on %s, the parameters %d on %s; reset() first"
                                   % (self.residual.numel(), self.residual.device, n, dev))
            if self.residual is None:
                self.residual = torch.zeros(n, dtype=f32, device=dev)
        keep = keep_count(n, self.ratio) if n else 0
        idx = torch.empty(keep, dtype=torch.int32, device=dev)
        val = torch.empty(keep, dtype=f32, device=dev)
        bad = torch.zeros(1, dtype=torch.int32, device=dev)
        if n:
            need = int(_C.lib().fedfr_topk_workspace_bytes(n, 1 if self.error_feedback else 0))
            if self.workspace is None or self.workspace.numel() < need or self.workspace.device != dev:
                self.workspace = torch.empty(need, dtype=torch.uint8, device=dev)
            _C.call("fedfr_topk_sparsify", x.data_ptr(), xi.data_ptr(), _C.ptr(self.residual) if self.error_feedback else None, n, keep,
                    idx.data_ptr(), val.data_ptr(), bad.data_ptr(), self.workspace.data_ptr(), _C.stream())
        return SparseDelta(idx, val, n, keep, stats, counters, bad, client_state.table, client_state.layers)
