"""Server side of the federated loop (reference server.py:25-46, :265-338): dataset-size-weighted
averaging of client models, as HIP kernels over flat buffers (single process) or one RCCL all-reduce over
xGMI when every client is its own rank (one client = one MI355X); the spread-out step on the clients' class centres
(reference server.py:48-63, :340-371) on one fused HIP kernel; and the round's 1:1 verification of the global model with its
checkpoints (reference server.py:135-148).  Build extensions beyond the reference's FedAvg, one module-level round function each: the
server optimisers (``FedOpt``), the robust rules (``FedRobust``, ``FedReweighted``), client-level differential privacy (``FedDP``; privacy.py), and the
rounds from UPLOADS instead of states: 8 / 4-bit and top-k deltas with error feedback (``FedCompressed``, ``FedSparse``; compress.py),
optionally clipped by their norm as the server applies them and noised by the Gaussian mechanism (``UploadClip``),
pairwise-masked fixed-point updates (``FedSecAgg``; secagg.py) and those with the clients' own clip and discrete Gaussian noise
(``FedSecAggDP``).  What these share exists once: the chained delta step (``ServerOptimizer._chain``), the head, the tail and the masked
sum of a round from uploads (``_upload_round_head``, ``_upload_round_tail``, ``_masked_sum``).  ``Server.train`` runs a round in four
stages: settings and refusals, local training, the uploads, the aggregation."""
from __future__ import annotations

import copy
import ctypes
import logging
import random
from collections import OrderedDict
from types import SimpleNamespace
from typing import List, Sequence

import numpy as np
import torch

from . import _C, backbones
from .client import FlatStateDict, flat_state_dict

f32 = torch.float32


def _axpy(dst: torch.Tensor, src: torch.Tensor, w: float, accumulate: bool):
    _C.call("fedfr_fedavg_axpy", dst.data_ptr(), src.data_ptr(), float(np.float32(w)), dst.numel(), 1 if accumulate else 0,
            _C.stream())


def _check_states(x: torch.Tensor, xs: Sequence[torch.Tensor], what: str):
    """RuntimeError unless ``x`` and every tensor of ``xs`` are same-shape contiguous fp32 tensors on one GPU: what the multi-state kernels
    (csrc/multi_state.h) take as raw pointers"""
    if not x.is_cuda:
        raise RuntimeError("fedfr_amd.%s: state tensors must be on the GPU (no CPU fallback)" % what)
    for t in [x] + list(xs):
        if t.numel() != x.numel() or t.dtype != f32 or not t.is_contiguous() or t.device != x.device:
            raise RuntimeError("fedfr_amd.%s: states must be same-shape contiguous fp32 tensors on one device" % what)


class _Workspace:
    """the fp64 device buffer a kernel keeps its per-block partial sums in: grown on demand, kept between calls"""

    def __init__(self):
        self.buf = None

    def ensure(self, nbytes: int, dev):
        """(pointer, size in bytes) of at least ``nbytes`` on ``dev``"""
        if self.buf is None or self.buf.numel() * 8 < nbytes or self.buf.device != dev:
            self.buf = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=dev)
        return self.buf.data_ptr(), self.buf.numel() * 8


def _normalised(weights: Sequence[float]) -> List[float]:
    """w_i / Σw: the reference's ``weights[i] / sum(weights)`` (server.py:27)"""
    tot = sum(weights)
    return [w / tot for w in weights]


def _f32_vector(ws: Sequence[float]):
    """``ws`` rounded to fp32, as the ctypes array a kernel entry point takes its ≤ 8 weights in"""
    return (_C.f32 * len(ws))(*[float(np.float32(w)) for w in ws])


def _multi(dst: torch.Tensor, srcs: Sequence[torch.Tensor], ws: Sequence[float], accumulate: bool):
    """dst (+)= Σ_i ws[i]·srcs[i] over ≤ 8 same-shape contiguous fp32 tensors in one kernel (csrc/optim.hip: fedavg_multi_kernel)."""
    _check_states(dst, srcs, "FedPavg")
    _C.call("fedfr_fedavg_multi", dst.data_ptr(), _C.ptr_array(srcs), _f32_vector(ws), len(srcs), dst.numel(), 1 if accumulate else 0, _C.stream())


def _client_weights(what: str, models: List[dict], weights: Sequence[float], also=()) -> List[float]:
    """The n_i / Σn of the client states ``models``; RuntimeError unless they (and the states in ``also``) are FlatStateDicts that hold their
    flat buffers and there is one weight per client.  That the buffers are on the GPU is checked where they reach a kernel."""
    if not models or not all(isinstance(m, FlatStateDict) and m.flat is not None for m in list(also) + list(models)):
        raise RuntimeError("fedfr_amd.%s: the %sclient states must be FlatStateDicts (client.flat_state_dict)"
                           % (what, "global and the " if also else ""))
    if len(weights) != len(models):
        raise RuntimeError("fedfr_amd.%s: %d weights for %d client states" % (what, len(weights), len(models)))
    return _normalised(weights)


def _average_stats(models: List[dict], ws: Sequence[float], stats_rule=None):
    """(Bf, N) of a flat aggregate: the BN running statistics as Σ_i ws[i]·stats_i, ≤ 8 clients per pass of ``_multi`` in ascending order
    (or ``stats_rule(Bf, [stats_i])`` where the rule has its own), and the ``num_batches_tracked`` counters as the float
    Σ_i ws[i]·float(counter_i), ascending i: what the reference loop computes for these entries (F9)."""
    _, b0, n0 = models[0].flat
    Bf = torch.empty_like(b0)
    N = torch.empty(n0.numel(), dtype=f32, device=b0.device)
    if Bf.numel():                                  # (sphnet has no BatchNorm: no running statistics, no counters)
        if stats_rule is not None:
            stats_rule(Bf, [m.flat[1] for m in models])
        else:
            for c0 in range(0, len(models), 8):
                _multi(Bf, [m.flat[1] for m in models[c0:c0 + 8]], ws[c0:c0 + 8], c0 > 0)
    for i, (m, w) in enumerate(zip(models, ws)):
        n = m.flat[2]
        if n.numel():
            _C.call("fedfr_fedavg_i64", N.data_ptr(), n.data_ptr(), float(np.float32(w)), n.numel(), 1 if i else 0, None, _C.stream())
    return Bf, N


def FedPavg(models: List[dict], weights: Sequence[float]):
    """Σ_i (n_i/Σn)·sd_i[k] for every key k (reference server.py:25-34).

    Same op order as the reference (ascending client index, fp32 mul then add), so float entries are
    bit-identical to it.  int64 ``num_batches_tracked`` entries come back as float32, like the reference (F9).
    Fast path: FlatStateDicts → one pass over up to 8 clients' flat states (3 launches per 8 clients + one per counter vector); generic path: one kernel per key per client.
    """
    if models and all(isinstance(m, FlatStateDict) and m.flat is not None for m in models):
        ws = _client_weights("FedPavg", models, weights)
        P = torch.empty_like(models[0].flat[0])
        # up to 8 client states per pass (fedfr_fedavg_multi: every state read once, the aggregate written once; same op order and
        # roundings as one axpy per client, so still bit-identical to the reference loop)
        for c0 in range(0, len(models), 8):
            _multi(P, [m.flat[0] for m in models[c0:c0 + 8]], ws[c0:c0 + 8], c0 > 0)
        return FlatStateDict.from_flat((P, *_average_stats(models, ws)), models[0].table, models[0].layers)
    ws = _normalised(weights)
    aggr = OrderedDict()
    for name in models[0]:
        t0 = models[0][name]
        if not t0.is_cuda:
            raise RuntimeError("fedfr_amd.FedPavg: tensor '%s' is on %s; move state_dicts to the GPU" % (name, t0.device))
        if t0.is_floating_point():
            acc = torch.empty(t0.shape, dtype=f32, device=t0.device)
            for i, (m, w) in enumerate(zip(models, ws)):
                _axpy(acc, m[name].contiguous(), w, i > 0)
        else:
            acc = torch.empty(t0.shape, dtype=f32, device=t0.device)
            for i, (m, w) in enumerate(zip(models, ws)):
                src = m[name].contiguous().view(-1)
                _C.call("fedfr_fedavg_i64", acc.data_ptr(), src.data_ptr(), float(np.float32(w)), src.numel(), 1 if i else 0, None,
                        _C.stream())
        aggr[name] = acc
    return aggr


# ---- server optimisers (Reddi et al., "Adaptive Federated Optimization"): csrc/optim.hip fedopt_sqnorm_kernel / fedopt_multi_kernel
FEDOPT_KINDS = {"AVGM": 0, "ADAGRAD": 1, "ADAM": 2, "YOGI": 3}
FEDOPT_PLAIN = 4                       # x' = x + Δ, no moments (DP-FedAvg proper): fedfr_dp_multi only
AGGR_ALG_KINDS = {"FedAvgM": "AVGM", "FedAdagrad": "ADAGRAD", "FedAdam": "ADAM", "FedYogi": "YOGI"}


class ServerOptimizer:
    """State and hyper-parameters of one server optimiser over the flat parameter buffer: ``kind`` "AVGM" (server momentum), "ADAGRAD",
    "ADAM" or "YOGI" (the ``aggr_alg`` spellings "FedAvgM", "FedAdagrad", "FedAdam", "FedYogi" are accepted too).  ``m`` (and ``v`` for the
    adaptive kinds) are flat fp32 device tensors, allocated on first use to the parameter count (m = 0, v = tau^2, no bias correction, as in
    the paper), kept across rounds, dropped by ``reset()``.  ``clip_norm`` > 0 scales a client whose update norm ||x_i - x|| exceeds it down
    to that norm before aggregation.  ``last_update_sqnorm`` (fp64) and ``last_coef`` (fp32) hold the last round's squared update norms and
    aggregation coefficients, one per client, ON THE DEVICE: nothing reads them back unless the caller does.  (1 - beta) is formed in fp32, which is what the kernel and its restatement
    (tests/fedopt_cases.py) multiply by."""

    def __init__(self, kind, lr=1.0, beta1=0.9, beta2=0.99, tau=1e-3, clip_norm=0.0):
        self.kind = self._kind(kind)
        self.lr, self.beta1, self.beta2, self.tau, self.clip_norm = float(lr), float(beta1), float(beta2), float(tau), float(clip_norm)
        if not (self.tau > 0.0) and self.adaptive:
            raise ValueError("ServerOptimizer: tau must be positive for the adaptive kinds (got %r)" % (tau,))
        if self.clip_norm < 0.0 or self.clip_norm != self.clip_norm:
            raise ValueError("ServerOptimizer: clip_norm must be >= 0 (got %r)" % (clip_norm,))
        self.reset()

    @staticmethod
    def _kind(kind):
        k = AGGR_ALG_KINDS.get(kind, kind)
        if k not in FEDOPT_KINDS:
            raise ValueError("ServerOptimizer: kind must be one of %s or %s (got %r)" % (sorted(FEDOPT_KINDS), sorted(AGGR_ALG_KINDS), kind))
        return k

    @property
    def adaptive(self) -> bool:
        return self.kind != "AVGM"

    def reset(self):
        self.m = self.v = None
        self.rounds = 0
        self.last_update_sqnorm = self.last_coef = None
        self._scratch, self._ws = None, _Workspace()

    def hyper(self):
        """(lr, beta1, 1 - beta1, beta2, 1 - beta2, tau) as the fp32 values the kernel receives."""
        g = np.float32
        return tuple(float(t) for t in (g(self.lr), g(self.beta1), g(1) - g(self.beta1), g(self.beta2), g(1) - g(self.beta2), g(self.tau)))

    def _ensure(self, like: torch.Tensor):
        if self.m is not None and (self.m.numel() != like.numel() or self.m.device != like.device):
            raise RuntimeError("fedfr_amd.ServerOptimizer: the moments hold %d elements on %s, the parameters %d on %s; reset() first"
                               % (self.m.numel(), self.m.device, like.numel(), like.device))
        if self.m is None:
            self.m = torch.zeros(like.numel(), dtype=f32, device=like.device)
        if self.adaptive and self.v is None:
            t = np.float32(self.tau)
            self.v = torch.full((like.numel(),), float(t * t), dtype=f32, device=like.device)

    def coefficients(self, x: torch.Tensor, xs: Sequence[torch.Tensor], ws: Sequence[float]) -> torch.Tensor:
        """coef_i = w_i min(1, clip_norm / ||x_i - x||) as a DEVICE tensor (fedfr_fedopt_sqnorm: one pass over x and ≤ 8 client states
        at a time, no host synchronisation); the squared norms stay in ``last_update_sqnorm``."""
        _check_states(x, xs, "ServerOptimizer")
        n, dev = x.numel(), x.device
        sq = torch.empty(len(xs), dtype=torch.float64, device=dev)
        coef = torch.empty(len(xs), dtype=f32, device=dev)
        wsp = self._ws.ensure(int(_C.lib().fedfr_fedopt_sqnorm_workspace_bytes(min(8, len(xs)), n)), dev)
        for c0 in range(0, len(xs), 8):
            grp = xs[c0:c0 + 8]
            _C.call("fedfr_fedopt_sqnorm", x.data_ptr(), _C.ptr_array(grp), _f32_vector(ws[c0:c0 + 8]), len(grp), n, float(np.float32(self.clip_norm)),
                    sq.data_ptr() + 8 * c0, coef.data_ptr() + 4 * c0, *wsp, _C.stream())
        self.last_update_sqnorm, self.last_coef = sq, coef
        return coef

    def apply(self, x_out: torch.Tensor, x: torch.Tensor, xs: Sequence[torch.Tensor], coef: torch.Tensor):
        """x_out = x + step(Σ_i coef_i (x_i - x)) and the moment update (fedfr_fedopt_multi; ``x_out`` may be ``x``).  More than 8 client
        states chain passes through a scratch Δ buffer, bit-identical to one ascending loop; only the last pass touches m, v and x_out."""
        _check_states(x, list(xs) + [x_out], "ServerOptimizer")
        if coef.numel() != len(xs) or coef.dtype != f32 or coef.device != x.device or not coef.is_contiguous():
            raise RuntimeError("fedfr_amd.ServerOptimizer: coef must be a contiguous fp32 device tensor with one entry per client state")
        self._chain(x_out, x, xs, coef)

    def _chain(self, x_out, x, xs, coef, noise=None, plain=False):
        """THE chained delta step: ≤ 8 client states per pass, ascending; the last pass applies the step.  Through fedfr_fedopt_multi, or
        with ``noise`` = (noise_std, seed, round, stream_id, offset), given to every pass, through fedfr_dp_multi, whose last pass adds
        noise_std·z to Δ.  ``plain`` (with ``noise`` only): the kind FEDOPT_PLAIN, x_out = x + Δ, no moments, no round counted."""
        if not plain:
            self._ensure(x)
        n = x.numel()
        entry, noise = ("fedfr_fedopt_multi", ()) if noise is None else ("fedfr_dp_multi", tuple(noise))
        if len(xs) > 8 and (self._scratch is None or self._scratch.numel() != n or self._scratch.device != x.device):
            self._scratch = torch.empty(n, dtype=f32, device=x.device)      # the Δ buffer a chain runs through: kept between rounds
        for c0 in range(0, len(xs), 8):
            grp = xs[c0:c0 + 8]
            _C.call(entry, FEDOPT_PLAIN if plain else FEDOPT_KINDS[self.kind], x_out.data_ptr(), x.data_ptr(), _C.ptr_array(grp), coef.data_ptr() + 4 * c0,
                    len(grp), n, None if plain else self.m.data_ptr(), self.v.data_ptr() if self.adaptive and not plain else None,
                    self._scratch.data_ptr() if len(xs) > 8 else None, 1 if c0 == 0 else 0, 1 if c0 + 8 >= len(xs) else 0, *self.hyper(), *noise, _C.stream())
        if not plain:
            self.rounds += 1

    def _pass(self, x_out, x, xi, coef, scratch, first, last):
        _C.call("fedfr_fedopt_multi", FEDOPT_KINDS[self.kind], _C.ptr(x_out), x.data_ptr(), _C.ptr_array([xi]), coef.data_ptr(), 1, x.numel(),
                _C.ptr(self.m) if last else None, _C.ptr(self.v) if last and self.adaptive else None, scratch.data_ptr(), first, last,
                *self.hyper(), _C.stream())

    def weighted_delta(self, dst: torch.Tensor, x: torch.Tensor, xi: torch.Tensor, w: float):
        """dst = w (x_i - x), the term one client adds to Δ, with the two roundings it has inside ``apply`` (a first, non-last pass of
        fedfr_fedopt_multi whose Δ buffer is ``dst``; ``dst`` may be ``xi``).  Moments and parameters are not touched."""
        _check_states(x, [xi, dst], "ServerOptimizer")
        self._pass(None, x, xi, torch.tensor([w], dtype=f32, device=x.device), dst, 1, 0)

    def apply_delta(self, x_out: torch.Tensor, x: torch.Tensor, delta: torch.Tensor):
        """x_out = x + step(Δ) and the moment update for a Δ that already exists (``x_out`` may be ``delta`` or ``x``): the last pass of a
        chain, whose one remaining "client" is x itself and adds 1 (x - x) = 0."""
        _check_states(x, [delta, x_out], "ServerOptimizer")
        self._ensure(x)
        self._pass(x_out, x, x, torch.ones(1, dtype=f32, device=x.device), delta, 0, 1)
        self.rounds += 1

    def state_dict(self) -> dict:
        return {"kind": self.kind, "lr": self.lr, "beta1": self.beta1, "beta2": self.beta2, "tau": self.tau, "clip_norm": self.clip_norm,
                "rounds": self.rounds, "m": None if self.m is None else self.m.clone(), "v": None if self.v is None else self.v.clone()}

    def load_state_dict(self, sd: dict):
        kind = self._kind(sd["kind"])
        for name in ("m", "v"):
            t = sd.get(name)
            if t is not None and (not isinstance(t, torch.Tensor) or t.dtype != f32 or t.dim() != 1):
                raise ValueError("ServerOptimizer.load_state_dict: '%s' must be a flat fp32 tensor or None" % name)
        if sd.get("m") is not None and sd.get("v") is not None and sd["m"].numel() != sd["v"].numel():
            raise ValueError("ServerOptimizer.load_state_dict: m and v differ in length")
        self.reset()
        self.kind = kind
        self.lr, self.beta1, self.beta2, self.tau, self.clip_norm = (float(sd[k]) for k in ("lr", "beta1", "beta2", "tau", "clip_norm"))
        self.rounds = int(sd["rounds"])
        self.m = None if sd.get("m") is None else sd["m"].clone().contiguous()
        self.v = None if sd.get("v") is None or not self.adaptive else sd["v"].clone().contiguous()


def FedOpt(global_state, models: List[dict], weights: Sequence[float], opt: ServerOptimizer):
    """One server-optimiser round: the PARAMETERS of the new global state are x + step(Σ_i c_i (x_i - x)) with x = ``global_state``'s
    parameters, c_i = (n_i/Σn) min(1, clip_norm / ||x_i - x||) and the step of ``opt`` (two streaming kernels: per-client norms and
    coefficients, then the update with ≤ 8 client states per pass).  BN running statistics and ``num_batches_tracked`` are statistics,
    not optimisation variables: they are averaged exactly as ``FedPavg`` averages them (same kernels, order and float counters).
    Only GPU ``FlatStateDict``s are accepted."""
    ws = _client_weights("FedOpt", models, weights, also=[global_state])
    x, xs = global_state.flat[0], [m.flat[0] for m in models]
    _check_states(x, xs, "FedOpt")
    P = torch.empty_like(x)
    opt.apply(P, x, xs, opt.coefficients(x, xs, ws))
    return FlatStateDict.from_flat((P, *_average_stats(models, ws)), models[0].table, models[0].layers)


# ---- client-level differential privacy: csrc/dp.hip dp_multi_kernel (the clip: fedopt_sqnorm_kernel; mechanism and accounting: privacy.py)
def FedDP(global_state, models: List[dict], weights: Sequence[float], mech, opt: ServerOptimizer = None):
    """One DP-FedAvg round: the PARAMETERS of the new global state are x + step(Σ_i c_i (x_i - x) + noise_std z) with x = ``global_state``'s
    parameters, c_i = w_i min(1, clip_norm / ||x_i - x||) (``ServerOptimizer.coefficients``, as ``FedOpt``), w_i = ``weights[i]`` / Σ weights,
    noise_std = ``mech.noise_std(w)`` and z the standard normal values of ``mech``'s device stream at its current round
    (``privacy.GaussianMechanism``; the round counter advances by one per call).  ``opt=None``: step(Δ) = Δ, DP-FedAvg proper, no moments;
    otherwise the step and the moments of ``opt`` (its ``clip_norm`` must be the mechanism's).  One streaming kernel, fedfr_dp_multi: the
    noise is drawn and added inside the pass that reads the client states, ≤ 8 per pass; more chain through a scratch Δ buffer and the last
    pass alone adds the noise.  BN running statistics and ``num_batches_tracked`` are averaged exactly as ``FedOpt`` averages them,
    UN-NOISED: they are outside the mechanism.  Only GPU ``FlatStateDict``s are accepted."""
    ws = _client_weights("FedDP", models, weights, also=[global_state])
    x, xs = global_state.flat[0], [m.flat[0] for m in models]
    _check_states(x, xs, "FedDP")
    if opt is not None and np.float32(opt.clip_norm) != np.float32(mech.clip_norm):
        raise ValueError("FedDP: the server optimiser clips at %r, the mechanism's sensitivity bound is clip_norm=%r" % (opt.clip_norm, mech.clip_norm))
    clipper = opt
    if clipper is None:                                # the clip's workspace and the chain's scratch live with the mechanism
        clipper = getattr(mech, "_clipper", None)
        if clipper is None or clipper.clip_norm != mech.clip_norm:
            clipper = mech._clipper = ServerOptimizer("AVGM", clip_norm=mech.clip_norm)
    coef = clipper.coefficients(x, xs, ws)
    P = torch.empty_like(x)
    std = mech.noise_std([float(np.float32(w)) for w in ws])
    clipper._chain(P, x, xs, coef, noise=(std, mech.seed, mech.round, mech.stream_id, 0), plain=opt is None)
    mech.advance()
    return FlatStateDict.from_flat((P, *_average_stats(models, ws)), models[0].table, models[0].layers)


# ---- robust aggregation: csrc/robust.hip robust_trimmed_mean_kernel / robust_pairdist_kernel / robust_krum_select_kernel
ROBUST_ALG_KINDS = {"TrimmedMean", "CoordMedian", "Krum", "MultiKrum"}
ROBUST_MAX_CLIENTS = 32


class RobustAggregator:
    """One robust aggregation rule over the clients' flat states.  ``kind``: "TrimmedMean" (coordinate-wise mean of what is left after the
    b smallest and b largest values of every coordinate are dropped; b = ``trim`` if given, else floor(``trim_ratio`` k)), "CoordMedian"
    (b = (k - 1) // 2: the middle value or the mean of the middle two; ``trim`` / ``trim_ratio`` are ignored), "Krum" (the ONE client
    whose k - f - 2 nearest neighbours are nearest, f = ``num_byzantine``) or "MultiKrum" (the plain mean of the m best-scored clients,
    m = ``multi_m`` or k - f).  ``last_selected`` (ascending client indices), ``last_scores`` and ``last_dist`` (host numpy arrays) hold
    the last Krum round for logging; they are None for the coordinate-wise kinds.  At most 32 clients: an order statistic (and a
    selection) cannot be chained over groups of clients the way a sum can."""

    def __init__(self, kind, trim_ratio=0.1, trim=None, num_byzantine=1, multi_m=None):
        if kind not in ROBUST_ALG_KINDS:
            raise ValueError("RobustAggregator: kind must be one of %s (got %r)" % (sorted(ROBUST_ALG_KINDS), kind))
        self.kind = kind
        self.trim_ratio = float(trim_ratio)
        self.trim = None if trim is None else int(trim)
        self.num_byzantine = int(num_byzantine)
        self.multi_m = None if multi_m is None else int(multi_m)
        if not 0.0 <= self.trim_ratio < 0.5:
            raise ValueError("RobustAggregator: trim_ratio must be in [0, 0.5) (got %r)" % (trim_ratio,))
        if self.trim is not None and self.trim < 0:
            raise ValueError("RobustAggregator: trim must be >= 0 (got %r)" % (trim,))
        if self.num_byzantine < 0:
            raise ValueError("RobustAggregator: num_byzantine must be >= 0 (got %r)" % (num_byzantine,))
        if self.multi_m is not None and self.multi_m < 1:
            raise ValueError("RobustAggregator: multi_m must be >= 1 (got %r)" % (multi_m,))
        self.last_selected = self.last_scores = self.last_dist = None
        self._ws = _Workspace()

    @property
    def coordinate_wise(self) -> bool:
        return self.kind in ("TrimmedMean", "CoordMedian")

    def trim_count(self, k: int) -> int:
        """b for k clients (the coordinate-wise kinds)"""
        if self.kind == "CoordMedian":
            return (k - 1) // 2
        return self.trim if self.trim is not None else int(np.floor(self.trim_ratio * k))

    def select_count(self, k: int) -> int:
        """m for k clients (the Krum kinds)"""
        if self.kind == "Krum":
            return 1
        return self.multi_m if self.multi_m is not None else k - self.num_byzantine

    def validate(self, k: int):
        """ValueError for a client count this rule cannot serve"""
        if k < 1:
            raise ValueError("RobustAggregator(%s): no client states" % self.kind)
        if k > ROBUST_MAX_CLIENTS:
            raise ValueError("RobustAggregator(%s): %d clients, at most %d in one aggregation" % (self.kind, k, ROBUST_MAX_CLIENTS))
        if self.coordinate_wise:
            b = self.trim_count(k)
            if 2 * b >= k:
                raise ValueError("RobustAggregator(%s): trimming %d values at each end leaves nothing of %d clients (needs 2 b < k)"
                                 % (self.kind, b, k))
        else:
            f, m = self.num_byzantine, self.select_count(k)
            if k < 2 * f + 3:
                raise ValueError("RobustAggregator(%s): %d clients with num_byzantine = %d (needs k >= 2 f + 3)" % (self.kind, k, f))
            if not 1 <= m <= k - f:
                raise ValueError("RobustAggregator(%s): selecting m = %d of %d clients with num_byzantine = %d (needs 1 <= m <= k - f)"
                                 % (self.kind, m, k, f))

    def trimmed_mean(self, dst: torch.Tensor, srcs: Sequence[torch.Tensor]):
        """dst = the coordinate-wise trimmed mean of ``srcs`` at this rule's b (fedfr_robust_trimmed_mean: one pass, every state read once)"""
        k = len(srcs)
        self.validate(k)
        _check_states(dst, srcs, "FedRobust")
        _C.call("fedfr_robust_trimmed_mean", dst.data_ptr(), _C.ptr_array(srcs), k, self.trim_count(k), dst.numel(), _C.stream())

    def select(self, xs: Sequence[torch.Tensor]) -> List[int]:
        """Krum / Multi-Krum: the ascending indices of the selected states.  Distances and scores are computed on the device
        (fedfr_robust_pairdist, fedfr_robust_krum_select) into one buffer; then the host reads ``selected``, ``score`` and the distance
        matrix (kept as ``last_dist`` for logging) back in ONE blocking copy of 2 k + k^2 doubles: THE one synchronisation of a robust
        round (against a round of ~100 ms or more), needed because the
        choice of the states to average is made by the host.  RuntimeError if a selected score is not finite (fewer than m clients have
        k - f - 2 finite neighbours: nothing trustworthy to select)."""
        k = len(xs)
        self.validate(k)
        _check_states(xs[0], xs, "FedRobust")
        n, dev = xs[0].numel(), xs[0].device
        wsp = self._ws.ensure(int(_C.lib().fedfr_robust_pairdist_workspace_bytes(k, n)), dev)
        # one device buffer of 2 k + k^2 doubles: [score | selected (k int32 in the first half of k doubles) | dist], so that ONE copy brings all back
        out = torch.zeros(2 * k + k * k, dtype=torch.float64, device=dev)
        score, sel, dist = out[:k], out[k:2 * k], out[2 * k:]
        _C.call("fedfr_robust_pairdist", _C.ptr_array(xs), k, n, dist.data_ptr(), *wsp, _C.stream())
        _C.call("fedfr_robust_krum_select", dist.data_ptr(), k, self.num_byzantine, self.select_count(k), score.data_ptr(), sel.data_ptr(),
                _C.stream())
        host = out.cpu().numpy()                                    # the synchronisation: one blocking copy
        flags = host[k:2 * k].view(np.int32)[:k]
        self.last_scores, self.last_dist = host[:k].copy(), host[2 * k:].reshape(k, k).copy()
        self.last_selected = [int(i) for i in np.flatnonzero(flags)]
        if not all(np.isfinite(self.last_scores[i]) for i in self.last_selected):
            raise RuntimeError("fedfr_amd.FedRobust(%s): the score of a selected client is not finite (scores %s): fewer than %d clients "
                               "sent finite states" % (self.kind, self.last_scores.tolist(), self.select_count(k)))
        return self.last_selected


def FedRobust(models: List[dict], weights: Sequence[float], agg: RobustAggregator):
    """One robust aggregation of GPU ``FlatStateDict``s.
    TrimmedMean / CoordMedian: the parameters and the BN running statistics each go through the coordinate-wise rule, UNWEIGHTED (the
    data sizes are client-reported: weighting by them would hand a poisoning client its weight back); every kept value of a
    ``running_var`` is >= 0, so the result is.  The ``num_batches_tracked`` counters take ``FedPavg``'s path (data-size weights, float).
    Krum / MultiKrum: distances over the PARAMETER buffer, selection, then ``FedPavg`` of the selected states with unit weights (the
    existing kernels: bit-identical to calling it so).  One host synchronisation, in ``RobustAggregator.select``."""
    ws = _client_weights("FedRobust", models, weights)
    agg.validate(len(models))
    if not agg.coordinate_wise:
        chosen = agg.select([m.flat[0] for m in models])
        return FedPavg([models[i] for i in chosen], [1.0] * len(chosen))
    P = torch.empty_like(models[0].flat[0])
    agg.trimmed_mean(P, [m.flat[0] for m in models])
    return FlatStateDict.from_flat((P, *_average_stats(models, ws, agg.trimmed_mean)), models[0].table, models[0].layers)


# ---- reweighted aggregation: csrc/reweight.hip reweight_step_kernel / reweight_weights_kernel
REWEIGHT_ALG_KINDS = {"GeoMedian", "CenteredClip"}


class ReweightedAggregator:
    """One reweighted rule over the clients' flat states.  ``kind``: "GeoMedian" (the geometric median by RFA, the smoothed Weiszfeld
    iteration: weights alpha_i / max(``nu``, d_i), normalised) or "CenteredClip" (weights alpha_i min(1, ``tau`` / d_i); ``tau`` None or
    "auto": the lower median of the clients' finite update norms of the round), d_i the distance of client i to the current centre;
    ``iters`` weighted steps from the global parameters.  After a round ``last_dist`` ((iters + 1) x k: the distances before the first step
    -- the clients' update norms -- and after every step), ``last_weights`` (iters x k: the weights of every step) and ``last_tau`` (None
    for "GeoMedian") hold what the one blocking copy of the round brought back, for logging.  The workspace and the history buffer are
    kept across rounds.  At most 32 clients."""

    def __init__(self, kind, iters=3, nu=1e-6, tau=None):
        if kind not in REWEIGHT_ALG_KINDS:
            raise ValueError("ReweightedAggregator: kind must be one of %s (got %r)" % (sorted(REWEIGHT_ALG_KINDS), kind))
        self.kind = kind
        if isinstance(iters, bool) or not isinstance(iters, (int, np.integer)) or not 1 <= iters <= 64:
            raise ValueError("ReweightedAggregator: iters must be an integer in 1 ... 64 (got %r)" % (iters,))
        self.iters = int(iters)
        self.nu = float(nu)
        if not (self.nu > 0 and np.isfinite(self.nu)):
            raise ValueError("ReweightedAggregator: nu must be a positive finite number (got %r)" % (nu,))
        if tau is None or (isinstance(tau, str) and tau == "auto"):
            self.tau = None
        else:
            if isinstance(tau, (str, bool)) or not (float(tau) > 0 and np.isfinite(float(tau))):
                raise ValueError("ReweightedAggregator: tau must be a positive finite number, None or 'auto' (got %r)" % (tau,))
            self.tau = float(tau)
        self.last_dist = self.last_weights = self.last_tau = None
        self._ws = _Workspace()
        self._hist = None

    def validate(self, k: int):
        """ValueError for a client count this rule cannot serve"""
        if k < 1:
            raise ValueError("ReweightedAggregator(%s): no client states" % self.kind)
        if k > ROBUST_MAX_CLIENTS:
            raise ValueError("ReweightedAggregator(%s): %d clients, at most %d in one aggregation" % (self.kind, k, ROBUST_MAX_CLIENTS))

    def aggregate(self, z0: torch.Tensor, xs: Sequence[torch.Tensor], alpha: Sequence[float]) -> torch.Tensor:
        """The new centre (a new tensor) after ``iters`` weighted steps from ``z0`` over the states ``xs`` with prior weights ``alpha``:
        iters + 1 passes of fedfr_reweight_step (the first distance-only, the second out of place from ``z0``, the rest in place) with
        fedfr_reweight_weights behind each, back to back on one stream; then ONE blocking copy of the history ((iters + 1) k distances,
        iters k weights, tau, the no-finite-client flag): the one synchronisation of the round.  RuntimeError if no client was finite or
        the final distance of a weighted client is not."""
        from . import ops
        k, R = len(xs), self.iters
        self.validate(k)
        _check_states(z0, xs, "FedReweighted")
        if len(alpha) != k:
            raise RuntimeError("fedfr_amd.FedReweighted: %d prior weights for %d client states" % (len(alpha), k))
        n, dev = z0.numel(), z0.device
        self._ws.ensure(ops.reweight_workspace_bytes(k, n), dev)
        nd, nb = (R + 1) * k + 4, (R * k + 1) // 2                 # [D history | info | beta history (fp32, two per double)]
        if self._hist is None or self._hist.numel() != nd + nb or self._hist.device != dev:
            self._hist = torch.zeros(nd + nb, dtype=torch.float64, device=dev)
        hist_d, info, hist_b = self._hist[:(R + 1) * k], self._hist[(R + 1) * k:nd], self._hist[nd:].view(f32)
        param = self.nu if self.kind == "GeoMedian" else (self.tau or 0.0)
        P = torch.empty_like(z0)
        for slot in range(R + 1):
            if slot == 0:
                ops.reweight_step(None, z0, xs, None, self._ws.buf)
            else:
                ops.reweight_step(P, z0 if slot == 1 else P, xs, hist_b[(slot - 1) * k:slot * k], self._ws.buf)
            ops.reweight_weights(self.kind, alpha, param, slot, R, k, n, self._ws.buf, hist_d, hist_b, info)
        host = self._hist.cpu().numpy()                            # the synchronisation: one blocking copy
        with np.errstate(invalid="ignore"):
            self.last_dist = np.sqrt(host[:(R + 1) * k].reshape(R + 1, k))
        self.last_weights = host[nd:].view(np.float32)[:R * k].reshape(R, k).copy()
        self.last_tau = float(host[(R + 1) * k]) if self.kind == "CenteredClip" else None
        if host[(R + 1) * k + 2] != 0.0:
            raise RuntimeError("fedfr_amd.FedReweighted(%s): no client sent a finite state (distances %s)" % (self.kind, self.last_dist[0].tolist()))
        used = self.last_weights[R - 1] != 0
        if not np.all(np.isfinite(self.last_dist[R][used])):
            raise RuntimeError("fedfr_amd.FedReweighted(%s): the final distance of a weighted client is not finite (distances %s, weights %s)"
                               % (self.kind, self.last_dist[R].tolist(), self.last_weights[R - 1].tolist()))
        return P

    def stats_weights(self) -> List[float]:
        """the convex weights the BN running statistics are combined with after a round: the final weights, and for "CenteredClip" one
        more, 1 - sum(beta) >= 0, for the global state's statistics"""
        ws = [float(b) for b in self.last_weights[-1]]
        if self.kind == "CenteredClip":
            ws.append(max(0.0, 1.0 - sum(ws)))
        return ws


def FedReweighted(global_state, models: List[dict], weights: Sequence[float], agg: ReweightedAggregator):
    """One reweighted aggregation of GPU ``FlatStateDict``s (GeoMedian / CenteredClip): ``agg.iters`` weighted steps over the PARAMETER
    buffer from ``global_state``'s parameters with UNWEIGHTED priors alpha_i = 1 / k (the data sizes are client-reported: see
    ``FedRobust``).  The BN running statistics are a convex combination, ``_average_stats`` at the final weights (for CenteredClip with
    1 - sum(beta) on the global state's; a client whose final weight is 0 is left out, as the step pass skips it), so a ``running_var``
    stays >= 0; the ``num_batches_tracked`` counters take ``FedPavg``'s path
    (data-size weights, float).  One host synchronisation, in ``ReweightedAggregator.aggregate``."""
    ws = _client_weights("FedReweighted", models, weights, also=[global_state])
    k = len(models)
    agg.validate(k)
    P = agg.aggregate(global_state.flat[0], [m.flat[0] for m in models], [1.0 / k] * k)
    sw = agg.stats_weights()
    extra = [global_state.flat[1]] if agg.kind == "CenteredClip" else []

    def stats_rule(Bf, stats):      # what _average_stats does with the clients whose final weight is not zero (a skipped client's NaN must not reach 0 * NaN)
        kept = [(t, w) for t, w in zip(list(stats) + extra, sw) if w != 0]
        for c0 in range(0, len(kept), 8):
            _multi(Bf, [t for t, _ in kept[c0:c0 + 8]], [w for _, w in kept[c0:c0 + 8]], c0 > 0)
    return FlatStateDict.from_flat((P, *_average_stats(models, ws, stats_rule)), models[0].table, models[0].layers)


# ---- compressed uploads: csrc/compress.hip delta_quantize_kernel (client side, compress.py) / delta_aggregate_kernel
class _StatsOnly:
    """what ``_average_stats`` reads of a client state, for an upload that carries no fp32 parameters"""

    def __init__(self, stats, counters):
        self.flat = (None, stats, counters)


def _upload_round_head(what, global_state, uploads, is_upload, noun, expected, weights, server_opt, robust_why, clip_refusal, clip=None, mech=None):
    """What every round from uploads refuses, in this order: a global state that is no FlatStateDict with its flat buffers; uploads that
    are empty or not all ``is_upload`` (``noun``: "updates" / "uploads", ``expected``: what they must be); another number of ``weights``
    (None: the round takes none); a robust rule (``robust_why``); a server optimiser that clips (``clip_refusal``: the sentence that says
    why not) unless ``clip`` (an ``UploadClip``) measures the uploads at the optimiser's own clip_norm; a ``clip`` that is no
    ``UploadClip`` or clips elsewhere than the optimiser; a ``mech`` without ``clip``, or whose sensitivity bound is another clip_norm;
    global parameters off the GPU.  Returns those parameters and the weights, normalised (``weights`` None: uniform)."""
    if not isinstance(global_state, FlatStateDict) or global_state.flat is None:
        raise RuntimeError("fedfr_amd.%s: the global state must be a FlatStateDict (client.flat_state_dict)" % what)
    if not uploads or not all(is_upload(u) for u in uploads):
        raise RuntimeError("fedfr_amd.%s: the client %s must be %s" % (what, noun, expected))
    if weights is not None and len(weights) != len(uploads):
        raise RuntimeError("fedfr_amd.%s: %d weights for %d client %s" % (what, len(weights), len(uploads), noun))
    if isinstance(server_opt, (RobustAggregator, ReweightedAggregator)):
        raise ValueError("%s: a robust rule (%s) needs whole client states, %s" % (what, server_opt.kind, robust_why))
    if server_opt is not None and server_opt.clip_norm > 0 and clip is None:
        raise ValueError("%s: %s" % (what, clip_refusal))
    if clip is not None:
        if not isinstance(clip, UploadClip):
            raise ValueError("%s: clip must be a server.UploadClip (got %r)" % (what, clip))
        if server_opt is not None and server_opt.clip_norm > 0 and np.float32(server_opt.clip_norm) != np.float32(clip.clip_norm):
            raise ValueError("%s: the server optimiser clips at %r, the uploads are clipped at clip_norm=%r" % (what, server_opt.clip_norm, clip.clip_norm))
    if mech is not None:
        if clip is None:
            raise ValueError("%s: mech needs clip: the clip of the uploads is the sensitivity bound of the mechanism" % what)
        if np.float32(clip.clip_norm) != np.float32(mech.clip_norm):
            raise ValueError("%s: the uploads are clipped at %r, the mechanism's sensitivity bound is clip_norm=%r" % (what, clip.clip_norm, mech.clip_norm))
    x = global_state.flat[0]
    _check_states(x, [], what)
    return x, _normalised(weights if weights is not None else [1.0] * len(uploads))


class UploadClip:
    """The clip of a round from compressed or top-k uploads: what ``ServerOptimizer.coefficients`` is for fp32 states.  ``clip_norm`` > 0
    scales an upload whose norm AS THE SERVER WILL APPLY IT (the dequantised codes, the scattered entries) exceeds it down to that norm.
    One pass over <= 8 uploads at a time that reads their bytes once and no fp32 state (fedfr_delta_sqnorm, fedfr_sparse_sqnorm), no host
    synchronisation: after a call ``last_update_sqnorm`` (fp64), ``last_coef`` (fp32, w_i min(1, clip_norm / norm_i)) and, for top-k
    uploads, ``last_violations`` (int32: entries whose index is out of range or not ascending, without which alone the norm is the
    scattered vector's) hold one value per upload ON THE DEVICE; nothing reads them back unless the caller does.  Owns the workspace of
    the norm pass."""

    def __init__(self, clip_norm):
        self.clip_norm = float(clip_norm)
        if not self.clip_norm > 0.0:                   # (NaN fails the comparison too)
            raise ValueError("UploadClip: clip_norm must be > 0 (got %r)" % (clip_norm,))
        self._ws = _Workspace()
        self.last_update_sqnorm = self.last_coef = self.last_violations = None

    def _outputs(self, k: int, dev, violations: bool):
        self.last_update_sqnorm = torch.zeros(k, dtype=torch.float64, device=dev)
        self.last_coef = torch.empty(k, dtype=f32, device=dev)
        self.last_violations = torch.zeros(k, dtype=torch.int32, device=dev) if violations else None
        return self.last_update_sqnorm, self.last_coef, self.last_violations

    def compressed(self, updates, ws: Sequence[float], bits: int, n: int, dev) -> torch.Tensor:
        """coef as a DEVICE tensor for the ``compress.CompressedDelta``s ``updates`` (checked by the caller) at weights ``ws``"""
        sq, coef, _ = self._outputs(len(updates), dev, False)
        if n == 0:                                     # nothing to measure: sq = 0, coef = w
            coef.copy_(torch.tensor([float(np.float32(w)) for w in ws], dtype=f32))
            return coef
        wsp = self._ws.ensure(int(_C.lib().fedfr_upload_sqnorm_workspace_bytes(min(8, len(updates)), n)), dev)
        for c0 in range(0, len(updates), 8):
            grp = updates[c0:c0 + 8]
            _C.call("fedfr_delta_sqnorm", _C.ptr_array([u.codes for u in grp]), _C.ptr_array([u.scales for u in grp]), _f32_vector(ws[c0:c0 + 8]), len(grp),
                    bits, n, float(np.float32(self.clip_norm)), sq.data_ptr() + 8 * c0, coef.data_ptr() + 4 * c0, *wsp, _C.stream())
        return coef

    def sparse(self, updates, ws: Sequence[float], n: int, dev) -> torch.Tensor:
        """coef as a DEVICE tensor for the ``compress.SparseDelta``s ``updates`` (checked by the caller) at weights ``ws``"""
        sq, coef, viol = self._outputs(len(updates), dev, True)
        if n == 0:
            coef.copy_(torch.tensor([float(np.float32(w)) for w in ws], dtype=f32))
            return coef
        wsp = self._ws.ensure(int(_C.lib().fedfr_upload_sqnorm_workspace_bytes(min(8, len(updates)), max(u.keep for u in updates))), dev)
        for c0 in range(0, len(updates), 8):
            grp = updates[c0:c0 + 8]
            keeps = (ctypes.c_size_t * len(grp))(*[u.keep for u in grp])
            _C.call("fedfr_sparse_sqnorm", _C.ptr_array([u.idx for u in grp]), _C.ptr_array([u.val for u in grp]), keeps, _f32_vector(ws[c0:c0 + 8]), len(grp),
                    n, float(np.float32(self.clip_norm)), sq.data_ptr() + 8 * c0, coef.data_ptr() + 4 * c0, viol.data_ptr() + 4 * c0, *wsp, _C.stream())
        return coef


def _upload_noise(mech, ws):
    """(noise_std, seed, round, stream_id, offset) of a chain of ``_dp`` aggregates: ``mech``'s stream at its current round, or no noise"""
    if mech is None:
        return (0.0, 0, 0, 0, 0)
    return (mech.noise_std([float(np.float32(w)) for w in ws]), mech.seed, mech.round, mech.stream_id, 0)


def _upload_round_tail(global_state, P: torch.Tensor, x: torch.Tensor, uploads, ws: Sequence[float], server_opt):
    """The new global state of a round from uploads: ``P`` holds x + the aggregate, or with ``server_opt`` the aggregate alone, which then
    is the pseudo-gradient Δ of ``server_opt.apply_delta`` (in place); the BN running statistics and counters the uploads carry in the clear
    are averaged with ``ws`` exactly as ``FedPavg`` averages them."""
    if server_opt is not None:
        server_opt.apply_delta(P, x, P)
    stats = _average_stats([_StatsOnly(u.stats, u.counters) for u in uploads], ws)
    return FlatStateDict.from_flat((P, *stats), global_state.table, global_state.layers)


def FedCompressed(global_state, updates, weights: Sequence[float], server_opt=None, *, clip=None, mech=None):
    """One round from compressed uploads (``compress.CompressedDelta``, all of one width): the PARAMETERS of the new global state are
    x + Σ_i (n_i/Σn)·dq_i with x = ``global_state``'s parameters and dq_i the dequantised upload of client i (fedfr_delta_aggregate: ≤ 8
    uploads per pass, every code and scale byte read once; more clients chain passes with ``accumulate``, and x is added by the last pass
    only, so the sum has the roundings of one ascending loop).  With ``server_opt`` (a ``ServerOptimizer``) the same sum WITHOUT x is the
    pseudo-gradient Δ and goes through ``server_opt.apply_delta``; ``clip_norm`` > 0 raises ``ValueError`` (the clip needs per-client norms
    of the dequantised deltas: not provided).  BN running statistics and ``num_batches_tracked`` arrive uncompressed and are averaged
    exactly as ``FedPavg`` averages them.  A block a client sent as non-finite is NaN in the result, as it would be with fp32 uploads.
    Only a GPU ``FlatStateDict`` is accepted as ``global_state``.
    ``clip`` (an ``UploadClip``): the weights become c_i = (n_i/Σn) min(1, clip_norm / ||dq_i||), formed on the device from the codes
    and scale bytes (fedfr_delta_sqnorm) and read from there by the same chain (fedfr_delta_aggregate_dp); a ``server_opt`` that clips
    must clip at the same norm.  ``mech`` (a ``privacy.GaussianMechanism`` of that clip_norm; needs ``clip``): the last pass adds
    ``mech.noise_std(w)`` z of the mechanism's stream at its current round to the sum before x (or before ``server_opt``'s step), and the
    round counter advances by one.  BN running statistics and counters stay outside the clip and the mechanism."""
    from .compress import CompressedDelta
    x, ws = _upload_round_head("FedCompressed", global_state, updates, lambda u: isinstance(u, CompressedDelta), "updates",
                               "CompressedDeltas (Client.get_compressed_update)", weights, server_opt, "not compressed uploads",
                               "clip_norm > 0 needs per-client norms of the dequantised deltas, which compressed uploads do not provide; use "
                               "FedOpt on uncompressed states", clip, mech)
    n, bits = x.numel(), updates[0].bits
    lib = _C.lib()
    for u in updates:
        if u.bits != bits or u.n != n:
            raise RuntimeError("fedfr_amd.FedCompressed: an update of %d bits and %d parameters among updates of %d bits for %d parameters"
                               % (u.bits, u.n, bits, n))
        for t, need, what in ((u.codes, lib.fedfr_delta_code_bytes(bits, n), "codes"), (u.scales, lib.fedfr_delta_scale_bytes(n), "scales")):
            if t.dtype != torch.uint8 or t.numel() != need or t.device != x.device or not t.is_contiguous():
                raise RuntimeError("fedfr_amd.FedCompressed: %s must be a contiguous uint8 tensor of %d bytes on %s" % (what, need, x.device))
    P = torch.empty_like(x)
    for c0 in range(0, len(updates), 8):
        grp = updates[c0:c0 + 8]
        last = c0 + 8 >= len(updates)
        if n:
            base = x.data_ptr() if last and server_opt is None else None
            if clip is None:
                _C.call("fedfr_delta_aggregate", P.data_ptr(), base, _C.ptr_array([u.codes for u in grp]), _C.ptr_array([u.scales for u in grp]),
                        _f32_vector(ws[c0:c0 + 8]), len(grp), bits, n, 1 if c0 > 0 else 0, _C.stream())
            else:
                if c0 == 0:
                    coef, noise = clip.compressed(updates, ws, bits, n, x.device), _upload_noise(mech, ws)
                _C.call("fedfr_delta_aggregate_dp", P.data_ptr(), base, _C.ptr_array([u.codes for u in grp]), _C.ptr_array([u.scales for u in grp]),
                        coef.data_ptr() + 4 * c0, len(grp), bits, n, 1 if c0 > 0 else 0, 1 if last else 0, *noise, _C.stream())
    if mech is not None:
        mech.advance()
    return _upload_round_tail(global_state, P, x, updates, ws, server_opt)


# ---- secure aggregation: csrc/secagg.hip secagg_mask_kernel (client side, secagg.py) / secagg_aggregate_kernel
def _masked_sum(what, x: torch.Tensor, uploads, recovery_streams, frac_bits: int, rescale: float, add_x: bool, mismatch: str, bits: int = 32) -> torch.Tensor:
    """(``add_x``: x +) float(int32(S)) 2^-``frac_bits`` ``rescale`` as a new tensor, S = Σ_i y_i + Σ_r sign_r m_r mod 2^32 over the masked
    ``uploads`` and the ``recovery_streams`` (fedfr_secagg_aggregate: ≤ 8 uploads and ≤ 32 streams per pass; more chain passes through an
    integer buffer, and the last pass alone scales and adds x).  RuntimeError for an upload of other fraction bits or parameter count
    (``mismatch``: the sentence, the upload's two numbers left open) or whose ``y`` is not n contiguous int32 words on x's device.
    ``bits`` = 8 or 16: the uploads are NARROW WORDS (secagg.py), all of that width and of one public rotation; S is the FIELD-WISE sum mod
    2^bits of their padded_count(n) bits / 32 packed words and the streams, and the last pass turns the rotation back
    (fedfr_secagg_aggregate_narrow, chained in the same way): x + rescale D 2^-6 H (S 2^-``frac_bits``)."""
    from .secagg import padded_count, stream_arrays
    n = x.numel()
    words = n if bits == 32 else padded_count(n) * bits // 32
    for u in uploads:
        if u.frac_bits != frac_bits or u.n != n:
            raise RuntimeError("fedfr_amd.%s: %s" % (what, mismatch % (u.frac_bits, u.n)))
        if u.bits != bits:
            raise RuntimeError("fedfr_amd.%s: an upload of %d-bit words among uploads of %d-bit words" % (what, u.bits, bits))
        if bits != 32 and (u.rotation_seed, u.round) != (uploads[0].rotation_seed, uploads[0].round):
            raise RuntimeError("fedfr_amd.%s: an upload rotated with (seed %d, round %d) among uploads rotated with (seed %d, round %d)"
                               % (what, u.rotation_seed, u.round, uploads[0].rotation_seed, uploads[0].round))
        if u.y.dtype != torch.int32 or u.y.numel() != words or u.y.device != x.device or not u.y.is_contiguous():
            raise RuntimeError("fedfr_amd.%s: y must be a contiguous int32 tensor of %d words on %s" % (what, words, x.device))
    streams = list(recovery_streams)
    passes = max((len(uploads) + 7) // 8, (len(streams) + 31) // 32)
    acc = torch.empty(words, dtype=torch.int32, device=x.device) if passes > 1 else None
    P = torch.empty_like(x)
    for p in range(passes):
        grp, sgrp = uploads[8 * p:8 * p + 8], streams[32 * p:32 * p + 32]
        last = p == passes - 1
        keys, nonces, signs = stream_arrays(sgrp)
        if n and bits == 32:
            _C.call("fedfr_secagg_aggregate", P.data_ptr(), x.data_ptr() if last and add_x else None, _C.ptr(acc),
                    _C.ptr_array([u.y for u in grp]), len(grp), keys, nonces, signs, len(sgrp), frac_bits, rescale, n, 1 if p == 0 else 0,
                    1 if last else 0, _C.stream())
        elif n:
            _C.call("fedfr_secagg_aggregate_narrow", P.data_ptr(), x.data_ptr() if last and add_x else None, _C.ptr(acc),
                    _C.ptr_array([u.y for u in grp]), len(grp), bits, uploads[0].rotation_seed, uploads[0].round, keys, nonces, signs, len(sgrp), 0,
                    frac_bits, rescale, n, 1 if p == 0 else 0, 1 if last else 0, _C.stream())
    return P


def FedSecAgg(global_state, uploads, weights: Sequence[float], recovery_streams, rescale: float = 1.0, server_opt=None, bits=None):
    """One round from masked uploads (``secagg.MaskedUpdate``, all of one ``frac_bits``): the PARAMETERS of the new global state are
    x + float(int32(S)) 2^-f rescale with x = ``global_state``'s parameters and S = Σ_i y_i + Σ_r sign_r m_r mod 2^32 over the uploads
    and the ``recovery_streams`` ([(8 key words, 3 nonce words, sign)], ``secagg.SecAggServer.recovery_streams``), which cancel what the
    uploads' masks leave (fedfr_secagg_aggregate: ≤ 8 uploads and ≤ 32 streams per pass, every upload word read once; more chain passes
    through an integer buffer, and x is added by the last pass only.  Addition mod 2^32 has one result whatever the order).  ``rescale`` is
    fp32(1 / Σ of the survivors' public weights), 1.0 when nobody dropped (``secagg.survivor_rescale``).  With ``server_opt`` (a
    ``ServerOptimizer``) the same sum WITHOUT x is the pseudo-gradient Δ and goes through ``server_opt.apply_delta``; ``clip_norm`` > 0
    raises ``ValueError`` (the clip needs per-client norms, which masked uploads hide by design).  BN running statistics and
    ``num_batches_tracked`` arrive UNMASKED and are averaged over the uploads with ``weights`` exactly as ``FedPavg`` averages them.  Only a
    GPU ``FlatStateDict`` is accepted as ``global_state``.
    The width of the words is read from the uploads (``MaskedUpdate.bits``): all must have one, and with ``bits`` (the server's setting) that
    one.  At 8 or 16 bits the uploads are NARROW WORDS (secagg.py): S is the field-wise sum mod 2^bits of the packed words, and the
    parameters are x + rescale D 2^-6 H (S 2^-f), the rotation turned back (fedfr_secagg_aggregate_narrow); everything behind the sum is the
    same."""
    from .secagg import MaskedUpdate, check_bits
    if bits is not None:
        bits = check_bits(bits, "FedSecAgg")
    width = {u.bits for u in uploads if isinstance(u, MaskedUpdate)}
    if len(width) > 1:
        raise RuntimeError("fedfr_amd.FedSecAgg: uploads of different widths (%s bits): all clients of a round encode at one width" % sorted(width))
    if bits is not None and width and width != {bits}:
        raise RuntimeError("fedfr_amd.FedSecAgg: uploads of %d-bit words, the server expects %d-bit words" % (width.pop(), bits))
    rescale = float(np.float32(rescale))
    if not (np.isfinite(rescale) and rescale >= 1.0):
        raise ValueError("FedSecAgg: rescale is fp32(1 / sum of the survivors' weights), a finite number >= 1 (got %r)" % (rescale,))
    x, ws = _upload_round_head("FedSecAgg", global_state, uploads, lambda u: isinstance(u, MaskedUpdate), "uploads",
                               "MaskedUpdates (Client.get_masked_update)", weights, server_opt, "which masked uploads hide",
                               "clip_norm > 0 needs per-client norms of the updates, which masked uploads hide by design")
    frac_bits = uploads[0].frac_bits
    P = _masked_sum("FedSecAgg", x, uploads, recovery_streams, frac_bits, rescale, server_opt is None,
                    "an upload of %%d fraction bits and %%d parameters among uploads of %d bits for %d parameters" % (frac_bits, x.numel()),
                    **({} if uploads[0].bits == 32 else {"bits": uploads[0].bits}))
    return _upload_round_tail(global_state, P, x, uploads, ws, server_opt)


# ---- distributed differential privacy: csrc/ddp.hip ddp_mask_kernel (client side, secagg.py) / secagg_aggregate_kernel
def FedSecAggDP(global_state, uploads, recovery_streams, mech, server_opt=None):
    """One round from the uploads of ``secagg.SecAggClient.mask_dp`` (clipped, noised, masked; all of ``mech``, a
    ``privacy.DistributedDiscreteGaussian``): ``FedSecAgg``'s sum S through the same kernel (fedfr_secagg_aggregate, chained in the same
    way), with every client at weight 1 and rescale = fp32(1 / number of uploads): the PARAMETERS are x + float(int32(S)) 2^-f rescale, the
    MEAN of the clipped updates plus the noise of all uploads, or that mean as the pseudo-gradient of ``server_opt``.  (``FedSecAgg``
    itself takes a rescale >= 1 only, the reciprocal of a sum of public weights.)  BN running statistics and ``num_batches_tracked``
    arrive UNMASKED and are averaged uniformly, outside the mechanism.  At least ``mech.threshold`` uploads are required: with fewer the
    sum carries less noise than the accountant is told.
    A mechanism of 16-bit words (``mech.bits`` = 16) takes the NARROW WORDS of ``mask_dp`` at that width: S is the FIELD-WISE sum mod 2^16
    of the packed words and the streams, and the parameters are x + rescale D 2^-6 H (S 2^-f), the rotation turned back
    (fedfr_secagg_aggregate_narrow, unchanged: no new server kernel).  All uploads must be of that width and of one public rotation.  A
    field whose integer sum leaves +-32767 wraps: post-processing of the noised sum, expected ``mech.wrap_bound`` times per round."""
    from .privacy import DistributedDiscreteGaussian
    from .secagg import MaskedUpdate
    # the mechanism's own checks come first: what follows them reads the mechanism
    if not isinstance(mech, DistributedDiscreteGaussian):
        raise RuntimeError("fedfr_amd.FedSecAggDP: mech must be a privacy.DistributedDiscreteGaussian")
    if uploads and not mech.threshold <= len(uploads) <= mech.participants:
        raise ValueError("FedSecAggDP: %d uploads, the mechanism needs %d to %d (its threshold and its participants)"
                         % (len(uploads), mech.threshold, mech.participants))
    x, ws = _upload_round_head("FedSecAggDP", global_state, uploads, lambda u: isinstance(u, MaskedUpdate) and u.sqnorm is not None, "uploads",
                               "the MaskedUpdates of SecAggClient.mask_dp (Client.get_masked_update with dp=...)", None, server_opt,
                               "which masked uploads hide", "the clients have clipped their own updates at %g; a server optimiser with clip_norm > 0 "
                               "needs per-client norms, which masked uploads hide by design" % mech.clip_norm)
    mismatch = "an upload of %%d fraction bits and %%d parameters under a mechanism of %d bits for %d parameters (the state has %d)" \
        % (mech.frac_bits, mech.n, x.numel())
    if x.numel() != mech.n:
        raise RuntimeError("fedfr_amd.FedSecAggDP: %s" % (mismatch % (uploads[0].frac_bits, uploads[0].n)))
    P = _masked_sum("FedSecAggDP", x, uploads, recovery_streams, mech.frac_bits, float(np.float32(1.0 / len(uploads))), server_opt is None, mismatch,
                    **({} if mech.bits == 32 else {"bits": mech.bits}))
    return _upload_round_tail(global_state, P, x, uploads, ws, server_opt)


# ---- top-k uploads: csrc/sparse.hip topk_* kernels (client side, compress.py) / sparse_aggregate_kernel
def FedSparse(global_state, updates, weights: Sequence[float], server_opt=None, *, clip=None, mech=None):
    """One round from top-k uploads (``compress.SparseDelta``): the PARAMETERS of the new global state are x + Σ_i (n_i/Σn)·sparse_i with
    x = ``global_state``'s parameters and sparse_i the scattered upload of client i (fedfr_sparse_aggregate: ≤ 8 uploads per pass, x read
    and the result written once, no float atomics; the sorted entries are walked 256 at a time, so an entry is loaded again for every
    tile of 4096 elements its step reaches into; more clients chain passes with ``accumulate``, and x is added by the last pass only, so
    the sum has the roundings of one ascending loop).  The uploads may hold different numbers of entries.  With ``server_opt`` (a
    ``ServerOptimizer``) the same sum WITHOUT x is the pseudo-gradient Δ and goes through ``server_opt.apply_delta``; ``clip_norm`` > 0
    raises ``ValueError`` (the clip needs per-client norms of the deltas: not provided).  BN running statistics and
    ``num_batches_tracked`` arrive uncompressed and are averaged exactly as ``FedPavg`` averages them.  An element a client sent as
    non-finite is NaN in the result, as it would be with fp32 uploads.  Only a GPU ``FlatStateDict`` is accepted as ``global_state``.
    ``clip`` (an ``UploadClip``) and ``mech`` (a ``privacy.GaussianMechanism``): as in ``FedCompressed``, through fedfr_sparse_sqnorm and
    fedfr_sparse_aggregate_dp.  The noise is dense: every parameter receives it, not only the ones an upload touches.  The norm is the
    scattered vector's only if no entry breaks the format: ``clip.last_violations`` counts those per upload, and a caller who relies on
    the bound must read it (``Server.train`` does, and voids the round)."""
    from .compress import SparseDelta
    x, ws = _upload_round_head("FedSparse", global_state, updates, lambda u: isinstance(u, SparseDelta), "updates",
                               "SparseDeltas (Client.get_sparse_update)", weights, server_opt, "not top-k uploads",
                               "clip_norm > 0 needs per-client norms of the deltas, which top-k uploads do not provide; use FedOpt on uncompressed "
                               "states", clip, mech)
    n = x.numel()
    for u in updates:
        if u.n != n:
            raise RuntimeError("fedfr_amd.FedSparse: an update for %d parameters among updates for %d parameters" % (u.n, n))
        if not 0 <= u.keep <= n:
            raise RuntimeError("fedfr_amd.FedSparse: an update of %d entries for %d parameters" % (u.keep, n))
        for t, dt, what in ((u.idx, torch.int32, "idx"), (u.val, f32, "val")):
            if t.dtype != dt or t.numel() != u.keep or t.device != x.device or not t.is_contiguous():
                raise RuntimeError("fedfr_amd.FedSparse: %s must be a contiguous %s tensor of %d entries on %s"
                                   % (what, str(dt).replace("torch.", ""), u.keep, x.device))
    P = torch.empty_like(x)
    for c0 in range(0, len(updates), 8):
        grp = updates[c0:c0 + 8]
        last = c0 + 8 >= len(updates)
        keeps = (ctypes.c_size_t * len(grp))(*[u.keep for u in grp])
        if n:
            base = x.data_ptr() if last and server_opt is None else None
            if clip is None:
                _C.call("fedfr_sparse_aggregate", P.data_ptr(), base, _C.ptr_array([u.idx for u in grp]), _C.ptr_array([u.val for u in grp]), keeps,
                        _f32_vector(ws[c0:c0 + 8]), len(grp), n, 1 if c0 > 0 else 0, _C.stream())
            else:
                if c0 == 0:
                    coef, noise = clip.sparse(updates, ws, n, x.device), _upload_noise(mech, ws)
                _C.call("fedfr_sparse_aggregate_dp", P.data_ptr(), base, _C.ptr_array([u.idx for u in grp]), _C.ptr_array([u.val for u in grp]), keeps,
                        coef.data_ptr() + 4 * c0, len(grp), n, 1 if c0 > 0 else 0, 1 if last else 0, *noise, _C.stream())
    if mech is not None:
        mech.advance()
    return _upload_round_tail(global_state, P, x, updates, ws, server_opt)


def FedAvg_on_FC(pretrain_fc, models, weights, p):
    """reference server.py:36-46."""
    ws = _normalised(weights)
    m0 = models[0].contiguous()
    if not m0.is_cuda:
        raise RuntimeError("fedfr_amd.FedAvg_on_FC: tensors must be on the GPU")
    aggr = torch.empty_like(m0)
    for i, (m, w) in enumerate(zip(models, ws)):
        _axpy(aggr, m.contiguous(), w, i > 0)
    if p == 1:
        return aggr
    out = torch.empty_like(aggr)
    _axpy(out, pretrain_fc.contiguous(), 1 - p, False)
    _axpy(out, aggr, p, True)
    return out


def _i64_scale(acc: torch.Tensor, src: torch.Tensor, w: float):
    _C.call("fedfr_fedavg_i64", acc.data_ptr(), src.data_ptr(), float(np.float32(w)), src.numel(), 0, None, _C.stream())


def _i64_trunc(acc: torch.Tensor, dst: torch.Tensor):
    """dst (int64) = trunc(acc) — load_state_dict's float -> int64 copy of the averaged num_batches_tracked (F9)."""
    _C.call("fedfr_fedavg_i64", acc.data_ptr(), dst.data_ptr(), 0.0, dst.numel(), 1, dst.data_ptr(), _C.stream())


def exchange_data_sizes(data_size: float, comm) -> float:
    """Σ n_j over the ranks (one tiny all-reduce + host read).  Run it when the sizes become known — at round start, off the exchange
    path — and hand the result to ``fedavg_all_reduce``; ranks that know every client's size in advance skip it."""
    dev = torch.device("cuda", torch.cuda.current_device()) if getattr(comm, "needs_device_tensors", False) else torch.device("cpu")
    t = torch.tensor([float(data_size)], dtype=torch.float64, device=dev)
    t = comm.all_reduce(t, "sum")
    return float(t.item())


def fedavg_all_reduce(backbone, data_size: float, total_size: float, comm=None, _axpy=_axpy, _i64=_i64_scale, _trunc=_i64_trunc,
                      server_opt=None, prev_params=None, dp=None):
    """One client per rank: the FedAvg of a round as ONE collective (replaces the CPU loop of server.py:25-34 and the state_dict
    hand-offs of server.py:286,311).  The local state — parameters, BN running statistics and a float image of the
    ``num_batches_tracked`` counters, which are slices of one fp32 tensor (``IResNet.exchange_buffer``) — is scaled in place by the
    pre-agreed weight n_i / Σn (the reference's ``weights[i] / sum(weights)``, server.py:27) and SUM-all-reduced in place over
    RCCL/xGMI: 261 MB for iresnet100, no packing copies, no host synchronisation.  The counters are truncated back to int64 as
    ``load_state_dict`` does (F9).  The summation ORDER is the collective's (a ring), not the reference's ascending client index: results
    agree with ``FedPavg`` to fp32 rounding, not bit for bit.
    ``comm``: fedfr_amd.comm communicator (default: the torch.distributed world).  ``_axpy`` / ``_i64`` / ``_trunc`` are the HIP
    kernels (injectable only so the plumbing can be exercised by the gloo CPU test).
    ``server_opt`` (a ``ServerOptimizer``) with ``prev_params`` = x (the caller's copy of the flat parameters taken BEFORE local
    training): the PARAMETER slice enters the exchange as w_i (x_i - x), formed in place with the roundings ``FedOpt`` gives that term, so
    after the all-reduce every rank holds Δ = Σ w_i (x_i - x) there (running statistics and counters: the plain mean, as without an
    optimiser); each rank then applies the optimiser's step to it in place (``fedfr_fedopt_multi``) and keeps its own, replicated copy of
    the moments.  Still ONE collective.  Under a communicator that adds in ascending rank order the result is ``FedOpt`` of the same client
    states bit for bit, otherwise to the fp32 rounding of the collective's order.  ``server_opt.clip_norm > 0`` raises ``ValueError``: on
    this path the clip would have to be applied by every rank to its OWN delta before the exchange (one more norm pass per rank) — a
    different algorithm from the clip ``FedOpt`` applies inside one aggregation, and not provided here.  ``dp`` (a
    ``privacy.GaussianMechanism``) raises ``ValueError`` for the same reason: the mechanism needs that clip; use ``FedDP``."""
    from .comm import TorchDistComm
    if dp is not None:
        raise ValueError("fedavg_all_reduce: differential privacy is not supported on the all-reduce path (it needs every rank's own delta "
                         "clipped before the exchange, a different algorithm); use FedDP")
    if isinstance(server_opt, (RobustAggregator, ReweightedAggregator)):
        raise ValueError("fedavg_all_reduce: a robust rule (%s) is not a sum and cannot ride a sum-all-reduce (every rank would need every "
                         "state: an all-gather, not provided here); use %s"
                         % (server_opt.kind, "FedRobust" if isinstance(server_opt, RobustAggregator) else "FedReweighted"))
    if server_opt is not None:
        if server_opt.clip_norm > 0:
            raise ValueError("fedavg_all_reduce: clip_norm > 0 is not supported on the all-reduce path (clipping a rank's own delta before "
                             "the exchange is a different algorithm); use FedOpt")
        if prev_params is None:
            raise ValueError("fedavg_all_reduce: server_opt needs prev_params (the flat parameters before local training)")
    if comm is None:
        comm = TorchDistComm()
    state, nbt_f, nbt = backbone.exchange_buffer()
    w = float(data_size) / float(total_size)
    # params + running stats = everything in front of the counter image.  Storage offsets, not pointer differences: a backbone without
    # BatchNorm counters (sphnet) has an EMPTY image, and data_ptr() of an empty tensor is 0 on torch >= 2.x
    n_float = nbt_f.storage_offset() - state.storage_offset()
    assert 0 <= n_float <= state.numel(), "exchange_buffer: the counter image is not a slice of the state tensor"
    fl = state[:n_float]
    if server_opt is None:
        _axpy(fl, fl, w, False)
    else:
        params = state[:backbone.flat_state()[0].numel()]
        stats = fl[params.numel():]
        if stats.numel() and stats.data_ptr() % 16:
            raise RuntimeError("fedavg_all_reduce: server_opt needs the running statistics 16-byte aligned inside the exchange buffer "
                               "(parameter count %d is not a multiple of 4)" % params.numel())
        server_opt.weighted_delta(params, prev_params, params, w)
        if stats.numel():
            _axpy(stats, stats, w, False)
    if nbt.numel():
        _i64(nbt_f, nbt, w)
    comm.all_reduce(state, "sum")                  # THE exchange of the round
    if nbt.numel():
        _trunc(nbt_f, nbt)
    if server_opt is not None:
        server_opt.apply_delta(params, prev_params, params)
    backbone.mark_weights_dirty()
    return w


def _spreadout_mean(mode) -> bool:
    if mode not in ("sum", "mean"):
        # the reference leaves the unreduced vector in `loss` for any other mode and fails later, in backward()
        raise ValueError("SpreadOut: mode must be 'sum' or 'mean' (got %r)" % (mode,))
    return mode == "mean"


class SpreadOut_Module(torch.nn.Module):
    """reference server.py:48-63: the Parameter ``FC`` [N, D] and ``forward()`` = sum ('sum') or mean ('mean') over the N (N - 1)
    off-diagonal pairs of relu(cos(FC_i, FC_j) - margin) ** 2.  ``loss.backward()`` and ``torch.optim.SGD`` work on it as on the
    reference's module; the loss and its gradient come from one fused HIP pass (``ops.SpreadOutFn``) that never holds the N x N cosine
    matrix.  ``local`` is unused, as in the reference."""

    def __init__(self, all_FC, margin=0.7, local=False, mode='sum'):
        super().__init__()
        _spreadout_mean(mode)
        self.FC = torch.nn.Parameter(all_FC)
        self.margin = margin
        self.mode = mode

    def forward(self):
        from .ops import SpreadOutFn
        return SpreadOutFn.apply(self.FC, float(self.margin), _spreadout_mean(self.mode))


class Server(object):
    """Round driver (reference server.py:68-133, :265-338): clients are trained sequentially in one process (as the
    reference does, server.py:283) and averaged with ``FedPavg``; with ``args.add_pretrained_data`` every client trains on
    local + public identities (``Client.train_with_public_data``) and, with ``args.return_all``, the public class centres
    are averaged with ``FedAvg_on_FC`` (server.py:316-327).  With ``server.pretrained_label`` set (``Initialize_pretrain_FC``)
    every round starts with the public-set embedding sweep (``Generate_pretrain_feats``) and the clients mine hard negatives
    from it (``Client.choose_hard_negative_2``), as server.py:272-275 / :294-304 do."""

    def __init__(self, clients, data, args, device=None):
        self.data = data
        self.clients = clients
        self.args = args
        self.num_client = len(clients)
        self.local_epoch = args.local_epoch
        self.global_epoch = 0
        self.global_round = 0
        self.device = device if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.federated_model = getattr(backbones, args.network)(False, dropout=0, fp16=True).to(self.device)
        self.current_client_list = list(range(self.num_client))
        self.logger = logging.getLogger("FL_face.server")
        self.public_train_loader = getattr(data, "public_train_loader", None)
        self.public_test_loader = getattr(data, "public_test_loader", self.public_train_loader)
        self.pretrained_label = None                 # [N_public] identity of every public image
        self.pretrained_feats = None                 # [N_public, 512] normalised embeddings (hard-negative mining)
        self.pretrained_fc = None                    # [n_public, 512] class centres of the public identities (server.py:182-240)
        self.pretrain_fc = None                      # where the reference stores the FedAvg'd public centres (server.py:325, see train())
        self.callback_local_veri = None              # local 1:1 verification (server.py:105-108): see enable_local_verification()
        self.local_candidates = []
        self.server_opt = None                       # ServerOptimizer of aggr_alg FedAvgM / FedAdagrad / FedAdam / FedYogi (built in train())
        self.robust_agg = None                       # RobustAggregator of aggr_alg TrimmedMean / CoordMedian / Krum / MultiKrum (built in train())
        self.reweight_agg = None                     # ReweightedAggregator of aggr_alg GeoMedian / CenteredClip (built in train())
        self.dp_mech = self.dp_accountant = None     # privacy.GaussianMechanism / RDPAccountant of dp_noise_multiplier > 0 (built in train())
        self.dp_epsilon = None                       # the (epsilon, dp_delta) guarantee after the rounds aggregated so far
        self.upload_clip = None                      # the UploadClip of clip_uploads (built in train()) and what the last round read of it
        self.upload_sqnorms = self.upload_coefs = self.upload_violations = None
        self.dp_last_sqnorms = None                  # distributed_dp: the survivors' sums of squared codes of the last round (each <= delta_int^2)
        self.scaffold_c = None                       # aggr_alg SCAFFOLD: the server's control variate c, fp32 [n_train] on the device (None = still zero)
        self.secagg_rng = None                       # n -> n random bytes for the secure-aggregation secrets (None: os.urandom)

    def enable_local_verification(self, callback, candidates=None):
        """reference server.py:105-108: ``callback`` (``eval_local.CallBack_LocalVerifi``) is handed to the clients whose ``cid`` is a
        "local candidate" — by default up to ten, ``sorted(np.random.permutation(num_client)[:10])``, drawn here and not in
        ``__init__`` so that a server without local verification consumes no random numbers for it."""
        self.callback_local_veri = callback
        if candidates is None:
            candidates = sorted(list(np.random.permutation(self.num_client)[:10]))
        self.local_candidates = [int(c) for c in candidates]
        self.logger.info('Local Veri Candidates %s' % (self.local_candidates,))

    # ---- public-set inference sweeps (reference server.py:182-263)
    def _eval_backbone(self):
        from .client import shared_backbone
        bb = shared_backbone(self.args.network, self.device, 0)       # the process-wide resident instance (one set of arenas)
        bb.load_state_dict(flat_state_dict(self.federated_model))
        return bb.eval()

    @torch.no_grad()
    @_C.on_device(lambda self: self.device)
    def Generate_pretrain_feats(self):
        """normalised embeddings of the whole public set under the current global model (server.py:242-263); stays on the GPU."""
        from .client import embed_dataset
        feats, _ = embed_dataset(self._eval_backbone(), self.public_test_loader, self.device, normalize=True)
        return feats

    @torch.no_grad()
    @_C.on_device(lambda self: self.device)
    def Initialize_pretrain_FC(self, only_labels=False):
        """(init_matrix [n_public_ID, 512], raw_labels [N]) — per-identity mean embedding of the public set (server.py:182-240).
        The reference's optional .pth cache (load_pth / save_pth) is checkpoint I/O, outside this path."""
        from .client import class_centers
        if only_labels:
            return None, torch.cat([torch.as_tensor(l) for _, l in self.public_test_loader]).to(torch.int64)
        n_id = self.public_test_loader.dataset.num_classes
        init_matrix, raw_labels = class_centers(self._eval_backbone(), self.public_test_loader, n_id, self.device,
                                                getattr(self, "norm_before_avg", getattr(self.args, "norm_before_avg", True)))
        return init_matrix, raw_labels.cpu()

    @_C.on_device(lambda self: self.device)
    def train(self):
        """One round (reference server.py:265-338) in four stages: the settings and everything they refuse, local training, the clients'
        uploads, the aggregation; then the new global state is installed.  Returns the clients' mean training loss."""
        s = self._round_settings()
        order = self._train_clients(s)
        up = self._collect_uploads(s, order)
        if s.return_all:                                                                         # server.py:316-327
            # Reference quirk kept: the averaged public centres are assigned to `self.pretrain_fc` — a misspelling of
            # `self.pretrained_fc` (server.py:325 vs :121-124, :295) — so the clients of the NEXT round still receive the initial
            # centres.  `args.feedback_public_fc = True` (a build extension, off by default) feeds the average back.
            self.pretrain_fc = FedAvg_on_FC(self.pretrained_fc, up.models_fc, up.data_sizes, p=1.0)
            if getattr(self.args, "feedback_public_fc", False):
                self.pretrained_fc = self.pretrain_fc
        self.federated_model.load_state_dict(self._aggregate(s, order, up))
        # the round / epoch counters belong to the driver, as in the reference (train.py:87-88): call step_round() after train()
        return self.avg_loss

    def _round_settings(self):
        """Stage 1: ``self.args`` read once, and every combination of settings that cannot be served refused, BEFORE a round of client
        training is spent on it (no client is touched here).  Builds ``self.robust_agg`` and the distributed-DP mechanism; returns the
        resolved values as one record (what is off is 0 / False / None)."""
        a = self.args
        aggr_alg = getattr(a, "aggr_alg", "FedAvg")
        dp_sigma = float(getattr(a, "dp_noise_multiplier", 0) or 0)          # client-level differential privacy (a build extension): absent or 0 = off
        clip_norm = float(getattr(a, "clip_norm", 0.0) or 0.0)
        ddp_on = bool(getattr(a, "distributed_dp", False))                   # the noise added by the CLIENTS under secure aggregation: absent or False = off
        compress_bits = getattr(a, "compress_bits", 0) or 0                  # compressed uploads (a build extension): absent or 0 = off
        topk_ratio = getattr(a, "topk_ratio", 0) or 0                        # top-k uploads (a build extension): absent or 0 = off
        secagg_on = bool(getattr(a, "secure_aggregation", False))            # secure aggregation (a build extension): absent or False = off
        return_all = bool(getattr(a, "return_all", False))
        clip_uploads = bool(getattr(a, "clip_uploads", False))               # the clip (and DP noise) ON compressed / top-k uploads: absent or False = off
        dp_delta = ddp_mech = secagg_frac_bits = secagg_threshold = None     # (resolved below where their feature is on)
        secagg_bits, secagg_rotation_seed = getattr(a, "secagg_bits", None), 0   # narrow masked uploads (a build extension): absent or 32 = one word per parameter
        ddp_wrap = getattr(a, "ddp_wrap_sigmas", None)                       # distributed DP at 16-bit words (kappa, the wrap headroom): absent or None = off
        if secagg_bits is not None:
            from .secagg import check_bits
            secagg_bits = check_bits(secagg_bits, "Server.train")
            if not secagg_on:
                raise ValueError("Server.train: secagg_bits=%d needs secure_aggregation: it is the width of a masked upload's codes" % (secagg_bits,))
            if ddp_on and secagg_bits != 32 and ddp_wrap is None:
                raise ValueError("Server.train: secagg_bits=%d cannot be combined with distributed_dp: discrete Gaussian noise in a ring of %d "
                                 "bits needs its own sensitivity and wrap-around analysis, which is not provided%s"
                                 % (secagg_bits, secagg_bits, " (set ddp_wrap_sigmas to opt into the 16-bit analysis: INTEGRATION.md section 21)"
                                    if secagg_bits == 16 else ""))
        if ddp_wrap is not None:                                             # the opt-in to distributed DP at 16-bit words: what it cannot serve
            from .privacy import DistributedDiscreteGaussian
            if not ddp_on:
                raise ValueError("Server.train: ddp_wrap_sigmas=%r needs distributed_dp: it is the wrap headroom of the clients' noise shares"
                                 % (ddp_wrap,))
            if secagg_bits == 8:
                raise ValueError("Server.train: secagg_bits=8 cannot be combined with distributed_dp: %s" % DistributedDiscreteGaussian.WHY_NOT_8)
            if secagg_bits != 16:
                raise ValueError("Server.train: ddp_wrap_sigmas=%r needs secagg_bits=16: at 32-bit words the clamp keeps every sum inside the "
                                 "word and nothing wraps" % (ddp_wrap,))
        secagg_drop = []
        robust_like = aggr_alg in ROBUST_ALG_KINDS or aggr_alg in REWEIGHT_ALG_KINDS      # the rules that need whole client states in the clear
        if aggr_alg not in ("FedAvg", "FedProx", "SCAFFOLD") and aggr_alg not in AGGR_ALG_KINDS and not robust_like:      # before a round of client training is spent on it
            raise ValueError("Server.train: unknown aggr_alg %r (FedAvg, FedProx, SCAFFOLD, %s, %s, %s)"
                             % (aggr_alg, ", ".join(AGGR_ALG_KINDS), ", ".join(sorted(ROBUST_ALG_KINDS)), ", ".join(sorted(REWEIGHT_ALG_KINDS))))
        from .client import check_prox_mu
        prox_mu = check_prox_mu(getattr(a, "prox_mu", 0), "Server.train")   # FedProx's proximal coefficient (client-side): absent or 0 = off, whatever aggr_alg is
        scaffold = aggr_alg == "SCAFFOLD"
        if scaffold:                                                         # the control updates travel in the clear and unclipped, beside whole states
            why = "the clients' control updates travel in the clear and unclipped"
            if secagg_on:
                raise ValueError("Server.train: aggr_alg='SCAFFOLD' cannot be combined with secure_aggregation: %s" % why)
            if compress_bits:
                raise ValueError("Server.train: aggr_alg='SCAFFOLD' cannot be combined with compress_bits=%r: %s" % (compress_bits, why))
            if topk_ratio:
                raise ValueError("Server.train: aggr_alg='SCAFFOLD' cannot be combined with topk_ratio=%r: %s" % (topk_ratio, why))
            if dp_sigma:
                raise ValueError("Server.train: aggr_alg='SCAFFOLD' cannot be combined with dp_noise_multiplier=%r: %s" % (dp_sigma, why))
            if clip_norm > 0:
                raise ValueError("Server.train: aggr_alg='SCAFFOLD' cannot be combined with clip_norm=%r: %s" % (clip_norm, why))
            if return_all:
                raise ValueError("Server.train: aggr_alg='SCAFFOLD' cannot be combined with return_all: %s, and the public class centres "
                                 "have no control variate" % why)
            if float(getattr(a, "server_lr", 1.0)) != 1.0:
                raise ValueError("Server.train: aggr_alg='SCAFFOLD' runs with the global step size 1 (got server_lr=%r): another one is not "
                                 "provided" % (a.server_lr,))
        if clip_uploads:                                                     # what the setting itself cannot serve; the pairings follow below
            if secagg_on:
                raise ValueError("Server.train: clip_uploads cannot be combined with secure_aggregation: the clip needs per-client norms of the "
                                 "uploads, which masks hide by design")
            if not compress_bits and not topk_ratio:
                raise ValueError("Server.train: clip_uploads needs compress_bits or topk_ratio: it clips compressed and top-k uploads; fp32 "
                                 "states are clipped by clip_norm with a server optimiser or dp_noise_multiplier")
        if ddp_on:
            if not secagg_on:
                raise ValueError("Server.train: distributed_dp needs secure_aggregation: the clients' noise shares protect only a sum that "
                                 "nobody sees in parts")
            if not dp_sigma:
                raise ValueError("Server.train: distributed_dp needs dp_noise_multiplier > 0 (got %r)" % (getattr(a, "dp_noise_multiplier", 0),))
            if not bool(getattr(a, "dp_uniform_weights", True)):
                raise ValueError("Server.train: distributed_dp needs dp_uniform_weights on: every client encodes at weight 1, the weight the "
                                 "sensitivity bound is stated for")
        if dp_sigma:                                                         # what cannot be served: before anybody trains
            if not (dp_sigma > 0 and np.isfinite(dp_sigma)):
                raise ValueError("Server.train: dp_noise_multiplier must be a finite number >= 0 (got %r)" % (a.dp_noise_multiplier,))
            if not clip_norm > 0:
                raise ValueError("Server.train: dp_noise_multiplier=%r needs clip_norm > 0: the clip is the sensitivity bound of the mechanism"
                                 % (dp_sigma,))
            if robust_like:
                raise ValueError("Server.train: dp_noise_multiplier=%r cannot be combined with aggr_alg=%r: a robust rule provides no per-client "
                                 "norms to clip" % (dp_sigma, aggr_alg))
            if compress_bits and not clip_uploads:
                raise ValueError("Server.train: dp_noise_multiplier=%r cannot be combined with compress_bits=%d: the clip needs per-client norms "
                                 "of the dequantised deltas, which are not provided" % (dp_sigma, compress_bits))
            if topk_ratio and not clip_uploads:
                raise ValueError("Server.train: dp_noise_multiplier=%r cannot be combined with topk_ratio=%r: the clip needs per-client norms of "
                                 "the deltas, which are not provided" % (dp_sigma, topk_ratio))
            if return_all:
                raise ValueError("Server.train: dp_noise_multiplier=%r cannot be combined with return_all: the averaged public class centres "
                                 "would be released un-noised" % (dp_sigma,))
            if not ddp_on and self.dp_accountant is not None and self.dp_accountant.sigma != dp_sigma:
                raise ValueError("Server.train: dp_noise_multiplier=%r after rounds accounted at %r: the accountant composes rounds of one noise "
                                 "multiplier (set server.dp_accountant yourself to continue)" % (dp_sigma, self.dp_accountant.sigma))
            dp_delta = float(getattr(a, "dp_delta", 1e-5))
            if not 0.0 < dp_delta < 1.0:
                raise ValueError("Server.train: dp_delta must be in (0, 1) (got %r)" % (dp_delta,))
        if aggr_alg in ROBUST_ALG_KINDS:                   # a client count the rule cannot serve: also before anybody trains
            if getattr(self, "robust_agg", None) is None or self.robust_agg.kind != aggr_alg:      # one aggregator per server (it keeps the distance workspace)
                self.robust_agg = RobustAggregator(aggr_alg, trim_ratio=getattr(a, "trim_ratio", 0.1), num_byzantine=getattr(a, "num_byzantine", 1),
                                                   multi_m=getattr(a, "multi_krum_m", None))
            self.robust_agg.validate(len(self.current_client_list))
        if aggr_alg in REWEIGHT_ALG_KINDS:                 # the same for the reweighted rules (the aggregator keeps workspace and history)
            want = dict(iters=getattr(a, "rfa_iters" if aggr_alg == "GeoMedian" else "cclip_iters", 3), nu=getattr(a, "rfa_nu", 1e-6),
                        tau=getattr(a, "cclip_tau", None))
            if getattr(self, "reweight_agg", None) is None or self.reweight_agg.kind != aggr_alg or self._reweight_settings != want:
                self.reweight_agg = ReweightedAggregator(aggr_alg, **want)      # one aggregator per server and setting
                self._reweight_settings = want
            self.reweight_agg.validate(len(self.current_client_list))
        if compress_bits:                                                    # what cannot be served: also before anybody trains
            from .compress import check_bits
            check_bits(compress_bits, "Server.train")
            if robust_like:
                raise ValueError("Server.train: compress_bits=%d cannot be combined with aggr_alg=%r: a robust rule needs whole client states"
                                 % (compress_bits, aggr_alg))
            if clip_norm > 0 and not clip_uploads:
                raise ValueError("Server.train: compress_bits=%d cannot be combined with clip_norm=%r: the clip needs per-client norms of the "
                                 "dequantised deltas, which are not provided" % (compress_bits, a.clip_norm))
        if topk_ratio:                                                       # the same: before anybody trains
            from .compress import keep_count
            try:
                keep_count(1, topk_ratio)
            except ValueError:
                raise ValueError("Server.train: topk_ratio must be a number in (0, 1] (got %r)" % (topk_ratio,)) from None
            if compress_bits:
                raise ValueError("Server.train: topk_ratio=%r cannot be combined with compress_bits=%d: quantising the kept values is not provided"
                                 % (topk_ratio, compress_bits))
            if robust_like:
                raise ValueError("Server.train: topk_ratio=%r cannot be combined with aggr_alg=%r: a robust rule needs whole client states"
                                 % (topk_ratio, aggr_alg))
            if clip_norm > 0 and not clip_uploads:
                raise ValueError("Server.train: topk_ratio=%r cannot be combined with clip_norm=%r: the clip needs per-client norms of the "
                                 "deltas, which are not provided" % (topk_ratio, a.clip_norm))
        if secagg_on:                                                        # the same: before anybody trains
            from .secagg import MAX_PARTICIPANTS, check_frac_bits
            K = len(self.current_client_list)
            if robust_like:
                raise ValueError("Server.train: secure_aggregation cannot be combined with aggr_alg=%r: a robust rule needs whole client states, "
                                 "which masked uploads hide" % (aggr_alg,))
            if compress_bits:
                raise ValueError("Server.train: secure_aggregation cannot be combined with compress_bits=%d: masking compressed uploads is not "
                                 "provided" % (compress_bits,))
            if topk_ratio:
                raise ValueError("Server.train: secure_aggregation cannot be combined with topk_ratio=%r: masking sparse uploads is not provided"
                                 % (topk_ratio,))
            if dp_sigma and not ddp_on:
                raise ValueError("Server.train: secure_aggregation cannot be combined with dp_noise_multiplier=%r: distributed differential "
                                 "privacy is not provided" % (dp_sigma,))
            if clip_norm > 0 and not ddp_on:
                raise ValueError("Server.train: secure_aggregation cannot be combined with clip_norm=%r: the clip needs per-client norms of the "
                                 "updates, which masked uploads hide by design" % (a.clip_norm,))
            if return_all:
                raise ValueError("Server.train: secure_aggregation cannot be combined with return_all: the public class centres would travel "
                                 "in the clear")
            if not 2 <= K <= MAX_PARTICIPANTS:
                raise ValueError("Server.train: secure_aggregation needs 2 to %d participants (got %d)" % (MAX_PARTICIPANTS, K))
            secagg_frac_bits = check_frac_bits(getattr(a, "secagg_frac_bits", 24), "Server.train")
            if secagg_bits in (8, 16):
                from .secagg import check_rotation_seed
                secagg_rotation_seed = check_rotation_seed(getattr(a, "secagg_rotation_seed", 0), "Server.train")      # public: shared by all clients and the server
            secagg_threshold = getattr(a, "secagg_threshold", None)
            if secagg_threshold is None:
                secagg_threshold = K // 2 + 1
            if isinstance(secagg_threshold, bool) or not isinstance(secagg_threshold, (int, np.integer)) or not 2 <= secagg_threshold <= K:
                raise ValueError("Server.train: secagg_threshold must be an integer in 2 ... %d, the number of participants (got %r)"
                                 % (K, secagg_threshold))
            secagg_drop = sorted(set(int(d) for d in (getattr(a, "secagg_drop", None) or ())))
            if any(d not in self.current_client_list for d in secagg_drop):
                raise ValueError("Server.train: secagg_drop=%r names clients that do not take part in this round (%s)"
                                 % (secagg_drop, list(self.current_client_list)))
            if K - len(secagg_drop) < secagg_threshold:
                raise ValueError("Server.train: secagg_drop=%r leaves %d of %d uploads, fewer than secagg_threshold=%d: the round could not be "
                                 "recovered" % (secagg_drop, K - len(secagg_drop), K, secagg_threshold))
            if ddp_on:                                                       # the mechanism's arithmetic, and what it refuses: also before anybody trains
                from .privacy import DistributedDiscreteGaussian
                ddp_mech = DistributedDiscreteGaussian(dp_sigma, clip_norm, secagg_frac_bits, K, int(secagg_threshold),
                                                       int(self.federated_model.flat_state()[0].numel()),
                                                       **({} if ddp_wrap is None else {"bits": 16, "wrap_sigmas": ddp_wrap}))
                if self.dp_accountant is not None and (self.dp_accountant.q, self.dp_accountant.sigma) != (1.0, ddp_mech.z_eff):
                    raise ValueError("Server.train: distributed_dp at an effective noise multiplier of %r after rounds accounted at %r (q = %g): "
                                     "the accountant composes rounds of one mechanism (set server.dp_accountant yourself to continue)"
                                     % (ddp_mech.z_eff, self.dp_accountant.sigma, self.dp_accountant.q))
        return SimpleNamespace(aggr_alg=aggr_alg, dp_sigma=dp_sigma, clip_norm=clip_norm, dp_delta=dp_delta, ddp_on=ddp_on, ddp_mech=ddp_mech,
                               compress_bits=compress_bits, topk_ratio=topk_ratio, feedback=bool(getattr(a, "error_feedback", True)),
                               secagg_on=secagg_on, secagg_frac_bits=secagg_frac_bits, secagg_threshold=secagg_threshold, secagg_drop=secagg_drop,
                               secagg_bits=secagg_bits or 32, secagg_rotation_seed=secagg_rotation_seed,
                               public=bool(getattr(a, "add_pretrained_data", False)), return_all=return_all,
                               clip_uploads=clip_uploads and clip_norm > 0, prox_mu=prox_mu, scaffold=scaffold)

    def _train_clients(self, s) -> List[int]:
        """Stage 2: every client of ``current_client_list`` receives the global model and trains, one after another or
        ``args.parallel_clients`` at a time; returns the clients in the order they are aggregated in."""
        from .config import config as cfg
        mine = s.public and bool(getattr(self.args, "choose_hard_negative", True)) and self.public_test_loader is not None \
            and self.pretrained_label is not None
        if mine:                                                                                 # server.py:272-275
            self.pretrained_feats = self.Generate_pretrain_feats()
        if getattr(self.args, "adaptive_local_epoch", False) and self.global_round != 0:        # server.py:277-280
            self.local_epoch = max(4, self.local_epoch - 2)
            cfg.train_decay = max(1, int(3 / 4 * self.local_epoch))

        def run_client(i, slot=0):
            c = self.clients[i]
            c.slot = slot
            c.backbone_state_dict = flat_state_dict(self.federated_model)       # "server sends backbone"
            c.local_epoch = self.local_epoch
            if s.scaffold or getattr(c, "scaffold_on", False):                  # "server sends c" (None while it is still zero)
                c.scaffold_on, c.scaffold_c = s.scaffold, self.scaffold_c if s.scaffold else None
            veri = {}                                                           # server.py:291-298: candidates train with the local test
            if self.callback_local_veri is not None and c.cid in self.local_candidates:
                veri = {"callback_verification": self.callback_local_veri}
            if s.public:
                if self.pretrained_fc is None:
                    raise RuntimeError("Server.train: add_pretrained_data needs server.pretrained_fc ([n_public, 512] class centres)")
                c.train_with_public_data(self.global_epoch, public_train_loader=self.public_train_loader,
                                         pretrained_fc=self.pretrained_fc, choose_hard_negative=mine,
                                         pretrained_label=self.pretrained_label, pretrained_feats=self.pretrained_feats, **veri)
            else:
                c.train(self.global_epoch, **veri)

        par = max(1, int(getattr(self.args, "parallel_clients", 1)))
        order = list(self.current_client_list)
        if par == 1:
            for i in order:
                run_client(i)
        else:
            # The clients of a round are independent (the reference trains them one after another, server.py:283); one client's step
            # is a dependent chain of ~1250 short kernels that leaves CUs idle between launches.  `par` clients train CONCURRENTLY on
            # this GPU, each on its own HIP stream pair and resident backbone (measured: 2 clients = +20 % images/s on iresnet100 at
            # B = 128; 3 regress).  Kernels are deterministic and clients share no state, so the round's result is identical to the sequential
            # round with the same kernel selection (the paired weight-gradient kernel below: otherwise equal up to fp32 summation order).
            import threading
            # Kernel selection is the lone client's (the paired weight-gradient kernel has been the default since round 3).  No kernel of the library
            # waits for another workgroup of its own launch (round 5 removed the one option that did, bn_fuse_bwd), so grids of several clients may
            # compete for the CUs freely.
            main = torch.cuda.current_stream(self.device)
            streams = getattr(self, "_client_streams", None)
            if streams is None or len(streams) < par:
                streams = self._client_streams = [torch.cuda.Stream(device=self.device, priority=-1) for _ in range(par)]
            for w0 in range(0, len(order), par):
                errs = []

                def target(i, slot):
                    try:
                        torch.cuda.set_device(self.device)
                        streams[slot].wait_stream(main)
                        with torch.cuda.stream(streams[slot]):
                            run_client(i, slot)
                        streams[slot].synchronize()
                    except BaseException as e:      # noqa: BLE001 — re-raised in the caller's thread
                        errs.append(e)
                ts = [threading.Thread(target=target, args=(i, k), daemon=True) for k, i in enumerate(order[w0: w0 + par])]
                for t in ts:
                    t.start()
                for t in ts:
                    t.join()
                if errs:
                    raise errs[0]
        return order

    def _collect_uploads(self, s, order):
        """Stage 3: what every client of ``order`` sends: its state, or its compressed / top-k / masked update against ``global_state``
        (after the key and share rounds of secure aggregation), its data size and, under ``return_all``, the public class centres.  Sets
        ``self.avg_loss``.  Returns one record; ``global_state``, ``sa_server`` and ``public_w`` are None where the round has no use for them."""
        up = SimpleNamespace(models=[], models_fc=[], data_sizes=[], global_state=None, sa_server=None, public_w=None)
        losses_ = []
        if s.compress_bits or s.topk_ratio or s.secagg_on:
            up.global_state = flat_state_dict(self.federated_model)           # what the round started from: the clients trained on copies
        if s.secagg_on:                                                       # rounds 0 to 2 of the protocol: keys, shares, public weights
            from .secagg import SecAggServer
            up.sa_server = SecAggServer(order, s.secagg_threshold, self.global_round)
            for i in order:
                sa = self.clients[i].secagg_client(i, s.secagg_frac_bits, self.secagg_rng)
                if (sa.bits, sa.rotation_seed) != (s.secagg_bits, s.secagg_rotation_seed):      # (32-bit words: nothing to tell the client)
                    sa.set_width(s.secagg_bits, s.secagg_rotation_seed)
                up.sa_server.register(i, sa.begin_round(self.global_round))
            for i in order:
                up.sa_server.deliver_shares(i, self.clients[i].secagg.make_shares(order, s.secagg_threshold))
            up.public_w = _normalised([self.clients[i].get_data_size() for i in order])      # w_i = n_i / Σn: public, the factor each client encodes with
            if s.ddp_on:
                up.public_w = [1.0] * len(order)                              # distributed DP: every client at weight 1, the mean is taken by the rescale
        for pos, i in enumerate(order):
            losses_.append(self.clients[i].get_train_loss())
            if s.secagg_on:                                                   # "client sends its masked fixed-point update"
                up.models.append(self.clients[i].get_masked_update(up.global_state, up.public_w[pos], order, up.sa_server.public_keys, self.global_round,
                                                                   **({"dp": s.ddp_mech} if s.ddp_on else {})))
            elif s.compress_bits:                                             # "client sends Q(x_i - x + e_i)" and keeps e_i
                up.models.append(self.clients[i].get_compressed_update(up.global_state, s.compress_bits, s.feedback))
            elif s.topk_ratio:                                                # "client sends the largest entries of x_i - x + e_i" and keeps the rest
                up.models.append(self.clients[i].get_sparse_update(up.global_state, s.topk_ratio, s.feedback))
            else:
                up.models.append(self.clients[i].get_model())
            if s.return_all:
                up.models_fc.append(self.clients[i].get_global_fc().to(self.device))
                self.clients[i].fc_module.remove_pretrain()
            up.data_sizes.append(self.clients[i].get_data_size())
        self.avg_loss = sum(losses_) / len(losses_)
        return up

    def _report_uploads(self, label, uploads, tail, senders, counters, warning, clip=None):
        """The log lines of a round from uploads: "``label``: N bytes from K clients, ... of the D bytes of fp32 states``tail``" over all
        ``uploads``; then ``counters`` (one small device tensor per aggregated upload, of the clients ``senders``) in ONE copy, the round's one
        read of them, and ``warning`` % (client, the counters it names) where one of those is not 0.  Returns the counters as lists.
        With ``clip`` (the round's ``UploadClip``) the same copy brings its squared norms, coefficients and, for top-k, violation counts
        (as fp64, which holds all of them exactly): they are logged per client and left on ``self.upload_sqnorms`` / ``upload_coefs`` /
        ``upload_violations`` (None where the clip counts none)."""
        sent, dense = sum(u.nbytes for u in uploads), sum(u.dense_nbytes for u in uploads)
        self.logger.info('%s: %d bytes from %d clients, %.4f of the %d bytes of fp32 states%s' % (label, sent, len(uploads), sent / dense, dense, tail))
        table = torch.stack([c.reshape(-1) for c in counters])
        if clip is not None:
            extra = [clip.last_update_sqnorm, clip.last_coef.double()] + ([] if clip.last_violations is None else [clip.last_violations.double()])
            table = torch.cat([table.double(), torch.stack(extra, dim=1)], dim=1)
        rows = table.cpu().tolist()
        if clip is not None:
            ncnt = counters[0].numel()
            self.upload_sqnorms, self.upload_coefs = [r[ncnt] for r in rows], [r[ncnt + 1] for r in rows]
            self.upload_violations = None if clip.last_violations is None else [int(r[ncnt + 2]) for r in rows]
            rows = [[int(v) for v in r[:ncnt]] for r in rows]
            for pos, i in enumerate(senders):
                self.logger.info('Client %s: squared upload norm %.9g, coefficient %.9g (clip_norm %g)'
                                 % (getattr(self.clients[i], "cid", i), self.upload_sqnorms[pos], self.upload_coefs[pos], clip.clip_norm))
        shown = warning.count('%d')
        for i, row in zip(senders, rows):
            if any(v > 0 for v in row[:shown]):
                self.logger.warning(warning % (getattr(self.clients[i], "cid", i), *row[:shown]))
        return rows

    def _aggregate(self, s, order, up):
        """Stage 4: the round's new global state from what ``_collect_uploads`` gathered, by the path the settings select; logs what the
        uploads cost and carried, and accounts the privacy spent."""
        if s.aggr_alg in AGGR_ALG_KINDS and getattr(self, "server_opt", None) is None:
            # server optimiser (a build extension: the reference's flag runs FedAvg only): one optimiser per server, moments kept across rounds
            a = self.args
            self.server_opt = ServerOptimizer(s.aggr_alg, lr=getattr(a, "server_lr", 1.0), beta1=getattr(a, "server_momentum", 0.9),
                                              beta2=getattr(a, "server_beta2", 0.99), tau=getattr(a, "server_tau", 1e-3),
                                              clip_norm=0.0 if s.ddp_on else getattr(a, "clip_norm", 0.0))      # (distributed DP: the clients clip)
        opt = self.server_opt if s.aggr_alg in AGGR_ALG_KINDS else None
        models, data_sizes, aggr_alg = up.models, up.data_sizes, s.aggr_alg
        if s.compress_bits or s.topk_ratio:
            clip, mech, weights = self._upload_clip(s, data_sizes)
            extra = {} if clip is None else {"clip": clip, "mech": mech}       # (clip_uploads off: today's call, argument for argument)
            if s.compress_bits:
                aggr_state_dict = FedCompressed(up.global_state, models, weights, opt, **extra)
                self._report_uploads('Compressed uploads (%d bits%s)' % (s.compress_bits, ", error feedback" if s.feedback else ""), models, '', order,
                                     [u.nonfinite_blocks for u in models], 'Client %s sent %d non-finite blocks (NaN in the aggregate there)', clip)
            else:
                aggr_state_dict = FedSparse(up.global_state, models, weights, opt, **extra)
                self._report_uploads('Top-k uploads (ratio %g%s)' % (s.topk_ratio, ", error feedback" if s.feedback else ""), models, '', order,
                                     [u.nonfinite for u in models], 'Client %s sent %d non-finite elements (NaN in the aggregate there)', clip)
            if clip is not None:
                self._check_clipped_uploads(order, mech is not None)
            if mech is not None:
                self._dp_account(s.dp_sigma, s.clip_norm, s.dp_delta)
        elif s.secagg_on:
            from .secagg import survivor_rescale
            keep = [pos for pos, i in enumerate(order) if i not in s.secagg_drop]      # (a dropped client's upload is discarded after masking)
            survivors, kept = [order[pos] for pos in keep], [models[pos] for pos in keep]
            streams = up.sa_server.recovery_streams(survivors)
            if s.ddp_on:
                aggr_state_dict = FedSecAggDP(up.global_state, kept, streams, s.ddp_mech, opt)
            else:
                aggr_state_dict = FedSecAgg(up.global_state, kept, [data_sizes[pos] for pos in keep], streams, survivor_rescale(up.public_w, keep), opt,
                                            **({} if s.secagg_bits == 32 else {"bits": s.secagg_bits}))
            bad = self._report_uploads('Masked uploads (%d fraction bits, threshold %d%s)'
                                       % (s.secagg_frac_bits, s.secagg_threshold, "" if s.secagg_bits == 32 else ", %d-bit words" % s.secagg_bits), models,
                                       '; %d dropped, %d recovery streams' % (len(models) - len(keep), len(streams)), survivors,
                                       [u.code_counters for u in kept],
                                       'Client %s sent %d saturated and %d non-finite elements (clamped to the code range / sent as 0)')
            if s.ddp_on:
                self._account_distributed_dp(s.ddp_mech, survivors, [row[2] for row in bad], kept, s.dp_delta, sum(row[0] for row in bad))
        elif s.dp_sigma:
            aggr_state_dict = self._aggregate_dp(models, data_sizes, aggr_alg, s.dp_sigma, s.clip_norm, s.dp_delta)
        elif aggr_alg in ("FedAvg", "FedProx"):
            aggr_state_dict = FedPavg(models, data_sizes)
        elif s.scaffold:
            aggr_state_dict = FedPavg(models, data_sizes)                      # global step size 1: the new model is today's FedAvg
            self._scaffold_update_c([self.clients[i].get_control_update() for i in order])
        elif aggr_alg in AGGR_ALG_KINDS:
            aggr_state_dict = FedOpt(flat_state_dict(self.federated_model), models, data_sizes, opt)
        elif aggr_alg in REWEIGHT_ALG_KINDS:
            # geometric median / centred clipping (a build extension): iters + 1 fused passes from the global parameters, one host synchronisation
            agg = self.reweight_agg
            aggr_state_dict = FedReweighted(flat_state_dict(self.federated_model), models, data_sizes, agg)
            if agg.last_tau is not None:
                self.logger.info('%s: tau %.9g (%s), %d steps' % (aggr_alg, agg.last_tau, "auto" if agg.tau is None else "given", agg.iters))
            for pos, i in enumerate(order):
                self.logger.info('Client %s: update norm %.9g, final distance %.9g, final weight %.9g'
                                 % (getattr(self.clients[i], "cid", i), agg.last_dist[0][pos], agg.last_dist[-1][pos], agg.last_weights[-1][pos]))
        else:
            # ROBUST_ALG_KINDS (nothing else passed the check above).  Robust aggregation (a build extension): trimmed mean / median per
            # coordinate, or Krum's selection (one host synchronisation)
            aggr_state_dict = FedRobust(models, data_sizes, self.robust_agg)
            if not self.robust_agg.coordinate_wise:
                kept = set(self.robust_agg.last_selected)
                cid = [getattr(self.clients[i], "cid", i) for i in order]
                self.logger.info('%s kept clients %s, rejected clients %s' % (aggr_alg, [cid[j] for j in sorted(kept)],
                                                                               [cid[j] for j in range(len(order)) if j not in kept]))
        return aggr_state_dict

    def _scaffold_update_c(self, dcs):
        """SCAFFOLD: c += (1 / N) sum_{i in S} dc_i over this round's clients S, N = all clients of the server: ``fedfr_fedavg_multi`` in
        accumulate mode, up to 8 control updates per pass.  Logs what the round's uploads cost."""
        if any(dc is None for dc in dcs):
            raise RuntimeError("Server.train: aggr_alg='SCAFFOLD' needs every client's control update (Client.get_control_update)")
        if self.scaffold_c is None:
            self.scaffold_c = torch.zeros_like(dcs[0])
        w = 1.0 / len(self.clients)
        for c0 in range(0, len(dcs), 8):
            _multi(self.scaffold_c, dcs[c0:c0 + 8], [w] * len(dcs[c0:c0 + 8]), True)
        n = self.scaffold_c.numel()
        self.logger.info('SCAFFOLD uploads: %d bytes from %d clients, 2 x %d bytes each (the parameters and the control update of %d '
                         'elements, both fp32, in the clear)' % (2 * 4 * n * len(dcs), len(dcs), 4 * n, n))

    def _account_distributed_dp(self, mech, survivors, exhausted, uploads, delta, saturated=0):
        """what ``distributed_dp`` checks and accounts after the round's aggregation (the counters have been read): a sampler that ran out
        of attempts and an upload beyond the sensitivity bound are errors (the round's result is not installed); then the accountant's
        step at q = 1 and the guaranteed noise multiplier, and ``self.dp_epsilon``.  At 16-bit words the sensitivity bound is deterministic
        (the rotation's norm bound plus sqrt(n_pad) of rounding), so the second check can only fire on a bug: it stays as the guard; the
        log then also names the width, kappa, the expected wrapped coordinates and the ``saturated`` codes of the round."""
        for cid, nex in zip(survivors, exhausted):
            if nex > 0:
                raise RuntimeError("Server.train: the noise sampler of client %s ran out of attempts on %d elements (they carry no noise): the "
                                   "round is void" % (getattr(self.clients[cid], "cid", cid), nex))
        sq = [int(v) & ((1 << 64) - 1) for v in torch.cat([u.sqnorm for u in uploads]).cpu().tolist()]
        bound = mech.delta_int * mech.delta_int
        for cid, v in zip(survivors, sq):
            if v > bound:
                raise RuntimeError("Server.train: the codes of client %s have squared norm %d, beyond the sensitivity bound delta_int^2 = %.6g of "
                                   "the mechanism: the round is void" % (getattr(self.clients[cid], "cid", cid), v, bound))
        self.dp_last_sqnorms = sq
        acc = self.dp_accountant
        if acc is None:
            acc = self.dp_accountant = mech.accountant()
        acc.step()
        self.dp_epsilon = acc.epsilon(delta)
        self.logger.info('Distributed differential privacy: (epsilon, delta) = (%.4f, %g) after %d rounds; guaranteed noise multiplier z_eff = %.6g '
                         '(asked %g; sigma_int %.6g per client, delta_int %.6g, threshold %d), realised %.6g with %d uploads; accounted at q = 1 '
                         'whatever the sampling rate (the amplification bound is proven for the continuous Gaussian only)'
                         % (self.dp_epsilon, delta, acc.steps, mech.z_eff, mech.noise_multiplier, mech.sigma_int, mech.delta_int, mech.threshold,
                            mech.realised_multiplier(len(survivors)), len(survivors)))
        if mech.bits != 32:
            self.logger.info('Distributed differential privacy at %d-bit words: %d bytes of packed words per upload (2 x n_pad = 2 x %d); code clamp '
                             '%d = %.3g standard deviations of a rotated coordinate (coordinate_sigmas); wrap headroom kappa = %g: expected wrapped '
                             'coordinates per round wrap_bound = %.3g (post-processing of the noised sum: accuracy, not privacy); %d saturated '
                             'codes among the %d uploads'
                             % (mech.bits, 2 * mech.n_pad, mech.n_pad, mech.code_limit, mech.coordinate_sigmas, mech.wrap_sigmas, mech.wrap_bound,
                                saturated, len(survivors)))

    def _upload_clip(self, s, data_sizes):
        """(clip, mech, weights) of a round from compressed or top-k uploads: (None, None, ``data_sizes``) unless ``clip_uploads`` is on; then
        the server's ``UploadClip`` (one per server and clip_norm: it keeps the workspace), and under ``dp_noise_multiplier`` > 0 the
        mechanism and the weights of ``_aggregate_dp``"""
        if not s.clip_uploads:
            return None, None, data_sizes
        clip = getattr(self, "upload_clip", None)
        if clip is None or clip.clip_norm != s.clip_norm:
            clip = self.upload_clip = UploadClip(s.clip_norm)
        if not s.dp_sigma:
            return clip, None, data_sizes
        return clip, self._dp_mechanism(s.dp_sigma, s.clip_norm), self._dp_weights(data_sizes)

    def _check_clipped_uploads(self, order, dp: bool):
        """what ``clip_uploads`` checks after the round's one read (``_report_uploads``), before the state is installed or the round
        accounted: a top-k upload with entries out of range or out of order does not have the norm the clip measured, and under DP an
        upload whose norm is not finite was not clipped at all (its coefficient is its weight): either voids the round"""
        for i, nv in zip(order, self.upload_violations or []):
            if nv > 0:
                raise RuntimeError("Server.train: the top-k upload of client %s holds %d entries whose index is out of range or not ascending; "
                                   "the clip measured another vector than the server applies and bounds nothing: the round is void"
                                   % (getattr(self.clients[i], "cid", i), nv))
        if dp:
            for i, sq in zip(order, self.upload_sqnorms):
                if not np.isfinite(sq):
                    raise RuntimeError("Server.train: the upload of client %s has squared norm %r: it was not clipped, so the sensitivity bound of "
                                       "the mechanism does not hold: the round is void" % (getattr(self.clients[i], "cid", i), sq))

    def _dp_mechanism(self, sigma, clip_norm):
        """the server's Gaussian mechanism (one per server: it holds the round counter of the noise stream), renewed when the settings change"""
        import secrets
        from .privacy import GaussianMechanism
        if self.dp_mech is None or (self.dp_mech.noise_multiplier, self.dp_mech.clip_norm) != (sigma, clip_norm):
            seed = getattr(self.args, "dp_seed", None)
            rnd = 0 if self.dp_mech is None else self.dp_mech.round
            self.dp_mech = GaussianMechanism(sigma, clip_norm, secrets.randbits(64) if seed is None else seed)
            self.dp_mech.round = rnd
        return self.dp_mech

    def _dp_weights(self, data_sizes):
        """the weights of a round under the central mechanism: uniform unless ``dp_uniform_weights`` is off (then a warning)"""
        uniform = bool(getattr(self.args, "dp_uniform_weights", True))
        if not uniform:
            self.logger.warning('dp_uniform_weights is off: data-size weights are client-reported; the sensitivity bound clip_norm * max w_i '
                                'holds for the weights of this round only')
        return [1.0] * len(data_sizes) if uniform else data_sizes

    def _aggregate_dp(self, models, data_sizes, aggr_alg, sigma, clip_norm, delta):
        """the round's aggregation under ``dp_noise_multiplier`` > 0: ``FedDP`` with the server's mechanism, then the accountant's step
        (``_dp_account``)."""
        opt = self.server_opt if aggr_alg in AGGR_ALG_KINDS else None
        out = FedDP(flat_state_dict(self.federated_model), models, self._dp_weights(data_sizes), self._dp_mechanism(sigma, clip_norm), opt)
        self._dp_account(sigma, clip_norm, delta)
        return out

    def _dp_account(self, sigma, clip_norm, delta):
        """the accountant's step for one round of the central mechanism and the (epsilon, delta) after the rounds so far, on
        ``self.dp_epsilon``.  q = len(current_client_list) / num_client; the rate only ever grows in the accountant (rdp is monotone in q,
        so the largest rate of the run bounds every round)."""
        from .privacy import RDPAccountant
        q = len(self.current_client_list) / float(self.num_client)
        acc = self.dp_accountant
        if acc is None or q > acc.q:
            steps = 0 if acc is None else acc.steps
            acc = self.dp_accountant = RDPAccountant(q, sigma)
            acc.steps = steps
        acc.step()
        self.dp_epsilon = acc.epsilon(delta)
        self.logger.info('Differential privacy: (epsilon, delta) = (%.4f, %g) after %d rounds (noise multiplier %g, clip_norm %g, q = %g)'
                         % (self.dp_epsilon, delta, acc.steps, sigma, clip_norm, acc.q))

    @torch.no_grad()
    @_C.on_device(lambda self: self.device)
    def SpreadOut(self, sp_iter=5, mode='sum'):
        """reference server.py:340-371: the class centres of the round's clients, stacked in ``current_client_list`` order, take ``sp_iter``
        SGD steps (lr = 10 cfg.lr, momentum 0.9, cfg.weight_decay) on the spread-out loss at margin 0.4 and go back to the clients.
        Per iteration: normalise -> fused loss + gradient kernel -> normalise backward -> SGD kernel, no autograd graph, one host read
        for the logged loss (the reference's ``loss.item()``).  Every client gets an independent tensor on the device and in the dtype its
        ``fc`` had.  The reference slices the result at ``idx * num_classes``, which is right only while all clients hold the same number
        of classes; the slices here follow running offsets, identical in that case."""
        from . import ops
        from .config import config as cfg
        assert self.current_client_list is not None
        mean = _spreadout_mean(mode)
        fcs = [self.clients[i].fc_module.fc.data for i in self.current_client_list]
        FC = torch.cat([t.detach().to(device=self.device, dtype=f32) for t in fcs], dim=0).contiguous()
        self.logger.info('=====Collect FC and cat to a big matrix=====')
        mom = torch.empty_like(FC)
        lr, wd = float(cfg.lr) * 10, float(cfg.weight_decay)
        self.logger.info('=====SpreadOut Module Create=====')
        for it in range(sp_iter):
            fn, inv = ops.normalize_rows(FC)
            loss, dfn, _ = ops.spreadout_loss_grad(fn, 0.4, mean)
            self.logger.info('- SP iter %d Loss :  %.5e , Start backward' % (it, loss.item()))
            ops.sgd_step(FC, ops.normalize_rows_bwd(fn, inv, dfn), mom, None, FC.numel(), lr, 0.9, wd, it == 0)
        o = 0
        for i, old in zip(self.current_client_list, fcs):
            n = old.shape[0]
            self.clients[i].fc_module.fc.data = FC[o:o + n].to(device=old.device, dtype=old.dtype, copy=True)
            o += n
        self.logger.info('=====Update FC in partial FC module=====')

    @torch.no_grad()
    @_C.on_device(lambda self: self.device)
    def test(self):
        """reference server.py:135-148: 1:1 verification of the global model on ``cfg.val_targets`` (``callbacks.CallBackVerification``:
        fused k-fold kernel, sets resident on the GPU), in eval mode through the resident shared backbone; ``backbone.pth`` when this
        round is the best of the last target so far and ``global_round`` > 0, ``backbone_<round>.pth`` always.  The callbacks and
        ``output_dir`` come from ``args`` / ``cfg`` on the first call."""
        import os
        from .callbacks import CallBackModelCheckpoint, CallBackVerification, portable_state_dict
        from .config import config as cfg
        if getattr(self, "callback_verification", None) is None:
            self.output_dir = getattr(self, "output_dir", None) or getattr(self.args, "output_dir", "./")
            os.makedirs(self.output_dir, exist_ok=True)
            self.callback_verification = CallBackVerification(1, 0, cfg.val_targets, cfg.val_rec, self.num_client)
            self.callback_checkpoint = CallBackModelCheckpoint(0, self.output_dir)
        self.federated_model.eval()
        bb = self._eval_backbone()
        self.callback_verification(self.global_round, bb, None, th=0)
        bb.eval()                                   # the callback leaves its backbone in train mode, as the reference's does
        self.federated_model.eval()
        if self.callback_verification.highest_acc_list[-1][0] == self.global_round:
            self.callback_checkpoint(self.global_round, self.federated_model, None)
            self.logger.info('Save server model, epoch %d model...' % (self.global_round))
        if self.global_round >= 0 and self.global_round % 1 == 0:
            torch.save(portable_state_dict(self.federated_model), os.path.join(self.output_dir, "backbone_%d.pth" % self.global_round))

    def step_round(self):
        """What the reference driver does after every ``server.train()`` (train.py:87-88)."""
        self.global_epoch += self.local_epoch
        self.global_round += 1
