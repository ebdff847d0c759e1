"""Client-level differential privacy for the federated rounds (DP-FedAvg: McMahan, Ramage, Talwar, Zhang, "Learning Differentially Private
Recurrent Language Models", 2018): the Gaussian mechanism's parameters and round counter (``GaussianMechanism``) and the privacy accounting
(``RDPAccountant``).  The clip is the server optimisers' (``ServerOptimizer.coefficients``: fedfr_fedopt_sqnorm), the noise is drawn and
added on the device inside the aggregation pass (``server.FedDP``: fedfr_dp_multi; the generator: csrc/dp.h).  Nothing here touches the GPU.

WHAT THE GUARANTEE COVERS, and what it does not:
  * the flat PARAMETER vector of the released global model.  BN running statistics and ``num_batches_tracked`` are averaged un-noised and are
    outside the mechanism;
  * Box-Muller on a 24-bit u1 truncates the noise at sqrt(48 ln 2) = 5.77 standard deviations, and fp32 noise carries the known
    floating-point-DP caveats (Mironov, "On Significance of the Least Significant Bits for Differential Privacy", 2012);
  * the accountant's amplification by sampling assumes POISSON sampling of the clients at rate q, which a driver's fixed-size sampling is not."""
from __future__ import annotations

import math

import numpy as np

MASK64 = (1 << 64) - 1


class GaussianMechanism:
    """The Gaussian mechanism of one run: noise N(0, (noise_multiplier * clip_norm * max_i w_i)^2) on the aggregated update, whose
    sensitivity to one client is clip_norm * max_i w_i once every client delta is clipped to ``clip_norm`` and weighted by w_i.  ``seed``
    (64 bits) and ``stream_id`` (32 bits) name the device noise stream; the round counter ``round`` is its third coordinate and advances by
    one per aggregation (``advance``), so every round draws fresh noise and a resumed run (``state_dict`` / ``load_state_dict``) draws what
    the uninterrupted run would have drawn."""

    def __init__(self, noise_multiplier, clip_norm, seed, stream_id=0):
        self.noise_multiplier, self.clip_norm = float(noise_multiplier), float(clip_norm)
        if not (self.noise_multiplier >= 0.0 and math.isfinite(self.noise_multiplier)):
            raise ValueError("GaussianMechanism: noise_multiplier must be finite and >= 0 (got %r)" % (noise_multiplier,))
        if not (self.clip_norm > 0.0 and math.isfinite(self.clip_norm)):
            raise ValueError("GaussianMechanism: clip_norm must be finite and > 0: without a clip there is no sensitivity bound (got %r)"
                             % (clip_norm,))
        self.seed = int(seed) & MASK64
        self.stream_id = int(stream_id)
        if not 0 <= self.stream_id < 1 << 32:
            raise ValueError("GaussianMechanism: stream_id must fit 32 bits (got %r)" % (stream_id,))
        self.round = 0
        self._clipper = None            # server.FedDP without a ServerOptimizer keeps its clip workspace and chain scratch here

    def noise_std(self, ws) -> float:
        """fp32(noise_multiplier) * fp32(clip_norm) * fp32(max_i w_i), multiplied in that order in fp32: the value the kernel receives"""
        g = np.float32
        return float((g(self.noise_multiplier) * g(self.clip_norm)) * g(max(ws)))

    def advance(self):
        self.round += 1

    def state_dict(self) -> dict:
        return {"noise_multiplier": self.noise_multiplier, "clip_norm": self.clip_norm, "seed": self.seed, "stream_id": self.stream_id,
                "round": self.round}

    def load_state_dict(self, sd: dict):
        self.seed, self.round = int(sd["seed"]) & MASK64, int(sd["round"])
        if self.round < 0:
            raise ValueError("GaussianMechanism.load_state_dict: round must be >= 0 (got %r)" % (sd["round"],))
        for name in ("noise_multiplier", "clip_norm"):
            if name in sd:
                setattr(self, name, float(sd[name]))
        if "stream_id" in sd:
            self.stream_id = int(sd["stream_id"])


def _logsumexp(terms):
    mx = max(terms)
    return mx + math.log(sum(math.exp(t - mx) for t in terms))


class RDPAccountant:
    """Renyi-DP accounting of the Poisson-subsampled Gaussian mechanism (Mironov, Talwar, Zhang, "Renyi Differential Privacy of the Sampled
    Gaussian Mechanism", 2019) at the integer orders alpha = 2 .. 256, composed additively over rounds:
        rdp(alpha) = 1 / (alpha - 1) * log sum_{i = 0 .. alpha} C(alpha, i) (1 - q)^(alpha - i) q^i exp((i^2 - i) / (2 sigma^2))      (q < 1)
        rdp(alpha) = alpha / (2 sigma^2)                                                                                             (q = 1)
        epsilon(delta) = min_alpha [T rdp(alpha) + log(1 / delta) / (alpha - 1)]
    with q the sampling rate, sigma the noise multiplier and T the rounds counted by ``step()``.  Pure Python floats; the sum goes through
    log-sum-exp, the binomial coefficients are exact integers (math.comb)."""

    ORDERS = tuple(range(2, 257))

    def __init__(self, sampling_rate, noise_multiplier):
        self.q, self.sigma = float(sampling_rate), float(noise_multiplier)
        if not 0.0 < self.q <= 1.0:
            raise ValueError("RDPAccountant: sampling_rate must be in (0, 1] (got %r)" % (sampling_rate,))
        if not (self.sigma > 0.0 and math.isfinite(self.sigma)):
            raise ValueError("RDPAccountant: noise_multiplier must be finite and > 0 (got %r)" % (noise_multiplier,))
        self.steps = 0
        self._rdp = {}

    def rdp(self, alpha: int) -> float:
        """the Renyi divergence of order ``alpha`` (an integer >= 2) of ONE round"""
        a = int(alpha)
        if a != alpha or a < 2:
            raise ValueError("RDPAccountant.rdp: alpha must be an integer >= 2 (got %r)" % (alpha,))
        if a not in self._rdp:
            s2 = 2.0 * self.sigma * self.sigma
            if self.q == 1.0:
                self._rdp[a] = a / s2
            else:
                lq, l1q = math.log(self.q), math.log1p(-self.q)
                terms = [math.log(math.comb(a, i)) + (a - i) * l1q + i * lq + (i * i - i) / s2 for i in range(a + 1)]
                self._rdp[a] = _logsumexp(terms) / (a - 1)
        return self._rdp[a]

    def step(self, rounds: int = 1):
        self.steps += int(rounds)

    def epsilon(self, delta: float, rounds=None) -> float:
        """the (epsilon, delta) guarantee after ``rounds`` rounds (default: the rounds counted so far)"""
        if not 0.0 < delta < 1.0:
            raise ValueError("RDPAccountant.epsilon: delta must be in (0, 1) (got %r)" % (delta,))
        T = self.steps if rounds is None else int(rounds)
        ld = math.log(1.0 / delta)
        return min(T * self.rdp(a) + ld / (a - 1) for a in self.ORDERS)

    def state_dict(self) -> dict:
        return {"sampling_rate": self.q, "noise_multiplier": self.sigma, "steps": self.steps}

    def load_state_dict(self, sd: dict):
        if float(sd["sampling_rate"]) != self.q or float(sd["noise_multiplier"]) != self.sigma:
            self.q, self.sigma, self._rdp = float(sd["sampling_rate"]), float(sd["noise_multiplier"]), {}
        self.steps = int(sd["steps"])
