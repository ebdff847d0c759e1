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


class DistributedDiscreteGaussian:
    """The arithmetic of the distributed discrete Gaussian mechanism (Kairouz, Liu, Steinke, "The Distributed Discrete Gaussian Mechanism
    for Federated Learning with Secure Aggregation", ICML 2021) on the fixed-point words of secure aggregation: ``participants`` K clients
    each clip their update to ``clip_norm`` C, encode it at ``frac_bits`` f, add integer Gaussian noise of
        sigma_int = z C 2^f / sqrt(T)
    (z = ``noise_multiplier``, T = ``threshold``: the fewest uploads a round can be recovered from, so the unmasked sum always carries at
    least the noise z C 2^f whoever dropped) and mask the result (``secagg.SecAggClient.mask_dp``: fedfr_secagg_mask_dp).  In the integers:
        delta_int  = C 2^f (1 + EPS_FP) + sqrt(n) / 2     the L2 sensitivity: the clipped, scaled update (EPS_FP bounds the fp32 rounding of the
                                                          clip factor and of the product) plus the rounding to
                                                          the nearest integer of ``n`` coordinates
        code_limit = L(K) - 37 (floor(sigma_int) + 1)     the clamp of a code: |noise| <= 37 (floor(sigma_int) + 1) always, so code +
                                                          noise stays inside L(K) = (2^31 - 1) // K and the sum of K of them inside int32
        z_eff      = sqrt(T) sigma_int / delta_int        the noise multiplier the mechanism GUARANTEES (below z by the rounding term)
        tau        = 10 sum_{k=1}^{T-1} exp(-2 pi^2 sigma_int^2 k / (k + 1))     how far a sum of T discrete Gaussians is from one (DDG, Theorem 1)
    ``ValueError`` when sigma_int is outside the sampler's [16, 2^26], when code_limit < delta_int (a clipped update would be clamped), or
    when tau n >= 1e-12 (at sigma_int >= 16 tau underflows to 0 in fp64); the message names the ``secagg_frac_bits`` that would work.  One
    round is then (delta_int / (sqrt(T) sigma_int))^2 / 2-zCDP, which is RDP(alpha) = alpha / (2 z_eff^2): ``accountant()`` returns
    ``RDPAccountant(1.0, z_eff)``.  Rounds are accounted at q = 1 whatever the sampling rate: valid and conservative (the amplification
    bound of ``RDPAccountant`` is proven for the continuous Gaussian only).

    ``bits=16, wrap_sigmas=kappa`` is the same mechanism on the NARROW WORDS of secure aggregation (``SecAggClient(bits=16).mask_dp``:
    fedfr_secagg_mask_narrow_dp): the clipped update is rotated block by block, rounded STOCHASTICALLY with the client's private draws,
    noised and summed field-wise in Z / 2^16.  With n_pad = padded_count(n), the coordinates of the rotated vector (after the rotation
    every coordinate of the padded last block carries the update: every one gets noise and counts toward the sensitivity):
        sigma_int  = z C 2^f / sqrt(T)                                unchanged
        delta_int  = C 2^f (1 + EPS_FP) (1 + EPS_ROT) + sqrt(n_pad)   the rotation is orthogonal; EPS_ROT bounds what its twelve fp32 butterfly
                                                                      levels and the product with the coefficient add to the L2 NORM (DESIGN.md
                                                                      section 3.31); stochastic rounding moves each of the n_pad coordinates by
                                                                      less than 1.  The paper's worst-case bound (c + gamma sqrt(d))^2: no
                                                                      conditional re-rounding.  The clamp only shrinks a code
        code_limit = (32767 - ceil(kappa sigma_int sqrt(K))) // K     |sum of K codes| <= K code_limit, and the sum of K noises passes
                                                                      kappa sigma_int sqrt(K) with probability <= 2 exp(-kappa^2 / 2) per
                                                                      coordinate (a discrete Gaussian is sigma-sub-Gaussian: Canonne, Kamath,
                                                                      Steinke 2020), so a field of the unmasked sum wraps at most that often
        wrap_bound = n_pad 2 exp(-kappa^2 / 2)                        the expected number of wrapped coordinates per round (an attribute)
        coordinate_sigmas = 64 code_limit / (C 2^f)                   code_limit does NOT bound a rotated coordinate: this is how many of its
                                                                      sub-Gaussian standard deviations (scale C 2^f / 64) fit inside the clamp;
                                                                      saturated codes are counted and logged
        tau, z_eff                                                    the formulas above, tau held against n_pad
    A wrapped field is POST-PROCESSING of the noised integer sum (reduction mod 2^16 is a ring homomorphism: the sum of the reduced uploads
    is the reduction of the integer sum): it costs accuracy, never privacy.  ``ValueError`` for sigma_int outside the sampler's range,
    code_limit < 1 or tau n_pad >= 1e-12 (with the ``secagg_frac_bits`` that would work), for ``bits=16`` without ``wrap_sigmas`` (finite,
    >= 1), for ``wrap_sigmas`` at 32 bits (nothing wraps there), and for ``bits=8``.  Each step of ``secagg_frac_bits`` doubles C 2^f and
    sigma_int, so only a few values fit between the sampler's smallest sigma and the wrap headroom."""

    EPS_FP = 2.0 ** -22
    EPS_ROT = 13 * 2.0 ** -24                        # (1 + 2^-24)^13 - 1 to first order: 12 butterfly levels and one product
    SIGMA_MIN, SIGMA_MAX = 16.0, 2.0 ** 26
    TAIL = 37                                        # |noise| <= TAIL (floor(sigma_int) + 1): U1 >= 2^-53 and 53 ln 2 < 37
    FIELD_MAX = 2 ** 15 - 1                          # the largest value of a 16-bit field
    WHY_NOT_8 = ("8-bit words cannot carry distributed differential privacy: the sampler's smallest sigma_int, 16, times any wrap_sigmas >= 1 "
                 "and sqrt(2) for the fewest participants already fills most of the +-127 of a field; use secagg_bits=16")

    def __init__(self, noise_multiplier, clip_norm, frac_bits, participants, threshold, n, bits=32, wrap_sigmas=None):
        from .secagg import MAX_PARTICIPANTS, check_bits, check_frac_bits, padded_count
        who = "DistributedDiscreteGaussian"
        self.bits = check_bits(bits, who)
        if self.bits == 8:
            raise ValueError("%s: %s" % (who, self.WHY_NOT_8))
        if self.bits == 32 and wrap_sigmas is not None:
            raise ValueError("%s: wrap_sigmas=%r belongs to 16-bit words: at 32 bits the clamp keeps every sum inside the word and nothing wraps"
                             % (who, wrap_sigmas))
        if self.bits == 16:
            if wrap_sigmas is None:
                raise ValueError("%s: 16-bit words need wrap_sigmas (ddp_wrap_sigmas): how many standard deviations of the summed noise the "
                                 "fields keep free, which sets the code clamp and the expected number of wrapped coordinates" % who)
            if isinstance(wrap_sigmas, bool) or not isinstance(wrap_sigmas, (int, float, np.integer, np.floating)) \
                    or not (math.isfinite(wrap_sigmas) and wrap_sigmas >= 1.0):
                raise ValueError("%s: wrap_sigmas must be a finite number >= 1 (got %r)" % (who, wrap_sigmas))
        self.wrap_sigmas = None if wrap_sigmas is None else float(wrap_sigmas)
        self.noise_multiplier, self.clip_norm = float(noise_multiplier), float(clip_norm)
        if not (self.noise_multiplier > 0.0 and math.isfinite(self.noise_multiplier)):
            raise ValueError("%s: noise_multiplier must be finite and > 0 (got %r)" % (who, noise_multiplier))
        if not (self.clip_norm > 0.0 and math.isfinite(self.clip_norm)):
            raise ValueError("%s: clip_norm must be finite and > 0: without a clip there is no sensitivity bound (got %r)" % (who, clip_norm))
        self.frac_bits = check_frac_bits(frac_bits, who)
        for name, v, lo, hi in (("participants", participants, 2, MAX_PARTICIPANTS), ("threshold", threshold, 2, participants),
                                ("n", n, 1, None)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < lo or (hi is not None and v > hi):
                raise ValueError("%s: %s must be an integer in %d ... %s (got %r)" % (who, name, lo, "" if hi is None else hi, v))
        self.participants, self.threshold, self.n = int(participants), int(threshold), int(n)
        self.n_pad = padded_count(self.n) if self.bits == 16 else self.n      # the coordinates that carry noise
        ok = [f for f in range(8, 31) if self._refusal(f) is None]
        why = self._refusal(self.frac_bits)
        if why is not None:
            hint = ("secagg_frac_bits in %d ... %d would work" % (ok[0], ok[-1])) if ok else "no secagg_frac_bits in 8 ... 30 would work"
            more = "" if self.bits == 32 else ", bits=%d, wrap_sigmas=%g" % (self.bits, self.wrap_sigmas)
            raise ValueError("%s: %s (noise_multiplier=%g, clip_norm=%g, secagg_frac_bits=%d, participants=%d, threshold=%d, n=%d%s): %s"
                             % (who, why, self.noise_multiplier, self.clip_norm, self.frac_bits, self.participants, self.threshold, self.n, more, hint))
        self.sigma_int, self.delta_int, self.code_limit, self.tau = self._numbers(self.frac_bits)
        self.z_eff = math.sqrt(self.threshold) * self.sigma_int / self.delta_int
        # (32 bits: the clamp keeps code + noise inside the word, nothing wraps, and no coordinate is rotated)
        self.wrap_bound = 0.0 if self.bits == 32 else self.n_pad * 2.0 * math.exp(-self.wrap_sigmas ** 2 / 2.0)
        self.coordinate_sigmas = None if self.bits == 32 else 64.0 * self.code_limit / (self.clip_norm * 2.0 ** self.frac_bits)

    def _numbers(self, f):
        from .secagg import code_limit
        scale = self.clip_norm * 2.0 ** f
        sigma = self.noise_multiplier * scale / math.sqrt(self.threshold)
        tau = 10.0 * sum(math.exp(-2.0 * math.pi ** 2 * sigma * sigma * k / (k + 1.0)) for k in range(1, self.threshold))
        if self.bits == 16:
            delta = scale * (1.0 + self.EPS_FP) * (1.0 + self.EPS_ROT) + math.sqrt(self.n_pad)
            headroom = int(math.ceil(self.wrap_sigmas * min(sigma, 2.0 ** 40) * math.sqrt(self.participants)))
            return sigma, delta, (self.FIELD_MAX - headroom) // self.participants, tau
        delta = scale * (1.0 + self.EPS_FP) + math.sqrt(self.n) / 2.0
        limit = code_limit(self.participants) - self.TAIL * (int(math.floor(min(sigma, 2.0 ** 40))) + 1)
        return sigma, delta, limit, tau

    def _refusal(self, f):
        sigma, delta, limit, tau = self._numbers(f)
        if not self.SIGMA_MIN <= sigma <= self.SIGMA_MAX:
            return "sigma_int = %.6g is outside the sampler's range [16, 2^26]" % sigma
        if self.bits == 16:
            if limit < 1:
                return ("the code clamp (32767 - ceil(%g x %.6g x sqrt(%d))) // %d = %d is below 1: the noise headroom leaves no room for codes "
                        "in a 16-bit field" % (self.wrap_sigmas, sigma, self.participants, self.participants, limit))
        elif limit < delta:
            return "the code clamp L' = %d is below the sensitivity delta_int = %.6g: clipped updates would be clamped" % (limit, delta)
        if tau * self.n_pad >= 1e-12:
            return "the sum of %d discrete Gaussians of sigma_int = %.6g is not close to one (tau n = %.3g >= 1e-12)" % (self.threshold, sigma, tau * self.n_pad)
        return None

    def realised_multiplier(self, survivors: int) -> float:
        """the multiplier of a round in which ``survivors`` >= threshold uploads arrived: sqrt(survivors / T) z_eff (not accounted: the
        accountant keeps the guaranteed z_eff)"""
        return math.sqrt(survivors / float(self.threshold)) * self.z_eff

    def accountant(self) -> "RDPAccountant":
        return RDPAccountant(1.0, self.z_eff)

    def same_as(self, other) -> bool:
        keys = ("noise_multiplier", "clip_norm", "frac_bits", "participants", "threshold", "n", "bits", "wrap_sigmas")
        return isinstance(other, DistributedDiscreteGaussian) and all(getattr(self, k) == getattr(other, k) for k in keys)


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
