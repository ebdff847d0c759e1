"""Secure aggregation of client updates (Bonawitz et al., "Practical Secure Aggregation for Privacy-Preserving Machine Learning", CCS
2017): every client uploads its update as 32-bit fixed-point words under pairwise masks (which cancel between any two clients whose
uploads both arrive) and a self mask (which the server removes once it knows the upload arrived), so the server learns only the SUM of
the updates.  The masks are ChaCha20 key streams generated on the device inside the pass that encodes the update
(``fedfr_secagg_mask``) and, for the recovery streams, inside the pass that sums the uploads (``fedfr_secagg_aggregate``,
``server.FedSecAgg``); the format is stated in include/fedfr_hip.h, "THE MASK STREAM".

This module is the host side of the protocol, in pure Python and numpy: X25519 key agreement (RFC 7748), key derivation with SHA-256,
Shamir secret sharing over GF(2^8), and the bookkeeping of a round (``SecAggClient``, ``SecAggServer``).

WHAT THIS IS AND IS NOT.  It is the SEMI-HONEST protocol in a ONE-PROCESS simulation, built so that the arithmetic, the kernels and the
dropout recovery run end to end:
  * shares are handed over inside the process; they are not encrypted to their recipients;
  * there is no authentication of public keys, no consistency-check round and no defence against a malicious server (the one invariant a
    semi-honest server must keep is enforced: it never reconstructs both the secret key and the self seed of the same client);
  * the integer arithmetic on Python numbers is not constant-time;
  * BN running statistics and ``num_batches_tracked`` travel in the clear, the stance ``compress.py`` and ``server.FedDP`` already take;
  * the RCCL path (``server.fedavg_all_reduce``) is left alone, and combining with compression or with top-k uploads is not provided.

DISTRIBUTED DIFFERENTIAL PRIVACY.  With a ``privacy.DistributedDiscreteGaussian`` every client clips its own update, adds its own share of
integer Gaussian noise to the codes and masks the result (``SecAggClient.mask_dp``: fedfr_secagg_mask_dp, one pass); the sum the server
unmasks then carries the noise of all surviving clients, and nobody ever holds an un-noised sum.  The sampler and its stream are stated in
include/fedfr_hip.h, "THE DISCRETE NOISE STREAM"; what the guarantee covers: DESIGN.md section 3.27.

NARROW WORDS.  ``SecAggClient(..., bits=8 or 16)`` uploads n_pad b / 8 bytes instead of 4 n: the update is rotated block by block with a
PUBLIC random sign flip and a Walsh-Hadamard transform (so that no coordinate is large), rounded STOCHASTICALLY to b-bit codes with the
client's private draws (so that the codes are unbiased), packed 32 / b to a word and masked and summed FIELD-WISE mod 2^b
(``fedfr_secagg_mask_narrow`` / ``fedfr_secagg_aggregate_narrow``; the format: include/fedfr_hip.h, "NARROW WORDS"; how to choose
``frac_bits``: INTEGRATION.md section 19).  ``bits=32`` is the path above, unchanged.  Distributed DP is provided at 16-bit words
(``mask_dp`` with a mechanism of ``bits=16``: fedfr_secagg_mask_narrow_dp; the analysis: INTEGRATION.md section 21), not at 8.
"""
from __future__ import annotations

import hashlib
import os
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

MAX_PARTICIPANTS = 32                # one launch adds at most 32 streams: 31 pair masks and the self mask
PURPOSE_PAIR, PURPOSE_SELF = 0, 1    # the third nonce word
_KEY_TAG = b"fedfr_amd.secagg.pairwise-mask.v1"

Rng = Callable[[int], bytes]         # n -> n random bytes (os.urandom by default; a seeded numpy Generator's ``.bytes`` in tests)


# ---- X25519 (RFC 7748 section 5) on Python integers ---------------------------------------------------------------------------------------
_P = 2 ** 255 - 19
_A24 = 121665
BASE_POINT = (9).to_bytes(32, "little")


def x25519(k: bytes, u: bytes) -> bytes:
    """the X25519 function: scalar ``k`` (32 bytes, clamped here) times the point with u-coordinate ``u`` (32 bytes), as 32 bytes"""
    if len(k) != 32 or len(u) != 32:
        raise ValueError("x25519: the scalar and the u-coordinate are 32 bytes each (got %d and %d)" % (len(k), len(u)))
    kb = bytearray(k)
    kb[0] &= 248
    kb[31] &= 127
    kb[31] |= 64
    kn = int.from_bytes(kb, "little")
    ub = bytearray(u)
    ub[31] &= 127
    x1 = int.from_bytes(ub, "little") % _P
    x2, z2, x3, z3, swap = 1, 0, x1, 1, 0
    for t in range(254, -1, -1):
        kt = (kn >> t) & 1
        if swap ^ kt:
            x2, x3, z2, z3 = x3, x2, z3, z2
        swap = kt
        a, b = (x2 + z2) % _P, (x2 - z2) % _P
        aa, bb = a * a % _P, b * b % _P
        e = (aa - bb) % _P
        da, cb = (x3 - z3) * a % _P, (x3 + z3) * b % _P
        x3 = (da + cb) ** 2 % _P
        z3 = x1 * (da - cb) ** 2 % _P
        x2 = aa * bb % _P
        z2 = e * (aa + _A24 * e) % _P
    if swap:
        x2, z2 = x3, z3
    return (x2 * pow(z2, _P - 2, _P) % _P).to_bytes(32, "little")


def keypair(rng: Optional[Rng] = None) -> Tuple[bytes, bytes]:
    """(secret key, public key): 32 random bytes and their X25519 product with the base point"""
    sk = (rng or os.urandom)(32)
    return sk, x25519(sk, BASE_POINT)


def derive_key(shared: bytes, i: int, j: int) -> Tuple[int, ...]:
    """the ChaCha20 key of the pair mask between clients ``i`` and ``j`` from their X25519 shared secret: SHA-256 over a fixed tag, the
    secret and the ORDERED pair of ids (so both ends derive the same key), as 8 little-endian words"""
    lo, hi = (i, j) if i <= j else (j, i)
    d = hashlib.sha256(_KEY_TAG + bytes(shared) + int(lo).to_bytes(8, "little") + int(hi).to_bytes(8, "little")).digest()
    return key_words(d)


def key_words(b: bytes) -> Tuple[int, ...]:
    """32 bytes as the 8 little-endian key words of the mask stream"""
    if len(b) != 32:
        raise ValueError("key_words: a ChaCha20 key is 32 bytes (got %d)" % len(b))
    return tuple(int.from_bytes(b[4 * q:4 * q + 4], "little") for q in range(8))


def round_nonce(round: int, purpose: int) -> Tuple[int, int, int]:
    """the protocol nonce: (round low 32 bits, round high 32 bits, purpose)"""
    return int(round) & 0xFFFFFFFF, (int(round) >> 32) & 0xFFFFFFFF, int(purpose)


# ---- Shamir secret sharing, byte-wise over GF(2^8) with the polynomial x^8 + x^4 + x^3 + x + 1 (0x11B) ------------------------------------
def _gf_tables():
    exp, log, v = np.zeros(510, np.int64), np.zeros(256, np.int64), 1
    for e in range(255):
        exp[e], log[v] = v, e
        d = v << 1
        v ^= d ^ 0x11B if d & 0x100 else d              # times the generator 3 = x + 1
    exp[255:] = exp[:255]
    return exp, log


_EXP, _LOG = _gf_tables()


def _gf_mul(a, b):
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    return np.where((a == 0) | (b == 0), 0, _EXP[_LOG[a] + _LOG[b]])


def _gf_inv(a: int) -> int:
    if a == 0:
        raise ZeroDivisionError("GF(2^8): 0 has no inverse")
    return int(_EXP[255 - _LOG[a]])


Share = Tuple[int, int, bytes]       # (x-coordinate 1 ... k, threshold t, one byte of the polynomial's value per byte of the secret)


def shamir_split(secret: bytes, k: int, t: int, rng: Optional[Rng] = None) -> List[Share]:
    """``k`` shares of ``secret``, any ``t`` of which give it back and any t - 1 of which say nothing about it: per byte a random
    polynomial of degree t - 1 with the byte as its constant term, evaluated at x = 1 ... k"""
    if not (1 <= t <= k <= 255):
        raise ValueError("shamir_split: need 1 <= t <= k <= 255 (got k=%r, t=%r)" % (k, t))
    rng = rng or os.urandom
    n = len(secret)
    coef = np.empty((t, n), np.int64)
    coef[0] = np.frombuffer(bytes(secret), np.uint8)
    if t > 1:
        coef[1:] = np.frombuffer(rng((t - 1) * n), np.uint8).reshape(t - 1, n)
    shares = []
    for x in range(1, k + 1):
        y = coef[t - 1].copy()
        for d in range(t - 2, -1, -1):                  # Horner
            y = _gf_mul(y, x) ^ coef[d]
        shares.append((x, t, y.astype(np.uint8).tobytes()))
    return shares


def shamir_combine(shares: Sequence[Share]) -> bytes:
    """the secret of ``shares`` (Lagrange interpolation at 0); ValueError for fewer shares than the threshold they carry, for duplicate
    x-coordinates, or for shares that do not belong together"""
    if not shares:
        raise ValueError("shamir_combine: no shares")
    t, n = shares[0][1], len(shares[0][2])
    if any(s[1] != t or len(s[2]) != n for s in shares):
        raise ValueError("shamir_combine: shares of different thresholds or lengths")
    xs = [int(s[0]) for s in shares]
    if len(set(xs)) != len(xs):
        raise ValueError("shamir_combine: duplicate x-coordinates %s" % sorted(xs))
    if any(not 1 <= x <= 255 for x in xs):
        raise ValueError("shamir_combine: x-coordinates must be 1 ... 255 (got %s)" % sorted(xs))
    if len(shares) < t:
        raise ValueError("shamir_combine: %d shares, the threshold is %d" % (len(shares), t))
    use = list(shares)[:t]
    out = np.zeros(n, np.int64)
    for xj, _, yj in use:
        lj = 1
        for xm, _, _ in use:
            if xm != xj:
                lj = int(_gf_mul(lj, _gf_mul(xm, _gf_inv(xm ^ xj))))
        out ^= _gf_mul(np.frombuffer(yj, np.uint8), lj)
    return out.astype(np.uint8).tobytes()


# ---- the round --------------------------------------------------------------------------------------------------------------------------
Stream = Tuple[Tuple[int, ...], Tuple[int, int, int], int]      # (8 key words, 3 nonce words, sign +1 / -1)


WIDTHS = (8, 16, 32)                 # bits of a code on the wire
ROTATION_BLOCK = 4096                # elements of one rotation block of the narrow widths


def check_bits(bits, who: str) -> int:
    if isinstance(bits, bool) or not isinstance(bits, (int, np.integer)) or int(bits) not in WIDTHS:
        raise ValueError("%s: secagg_bits must be 8, 16 or 32 (got %r)" % (who, bits))
    return int(bits)


def check_rotation_seed(seed, who: str) -> int:
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < 2 ** 64:
        raise ValueError("%s: secagg_rotation_seed must be an integer in 0 ... 2^64 - 1 (got %r)" % (who, seed))
    return int(seed)


def code_limit(participants: int, bits: int = 32) -> int:
    """L = (2^(bits-1) - 1) // K: the sum of K codes in [-L, L] cannot leave the signed range of ``bits`` bits"""
    return (2 ** (int(bits) - 1) - 1) // int(participants)


def padded_count(n: int) -> int:
    """n_pad: ``n`` rounded up to whole rotation blocks (the narrow widths encode, mask and sum n_pad elements)"""
    return (int(n) + ROTATION_BLOCK - 1) // ROTATION_BLOCK * ROTATION_BLOCK


def code_coef(weight: float, frac_bits: int) -> float:
    """c_i = fp32(fp32(w_i) 2^f), the factor of the encoding (exact: a power-of-two scaling)"""
    return float(np.float32(np.float32(weight) * np.float32(2.0 ** frac_bits)))


def check_frac_bits(frac_bits, who: str) -> int:
    if isinstance(frac_bits, bool) or not isinstance(frac_bits, (int, np.integer)) or not 8 <= int(frac_bits) <= 30:
        raise ValueError("%s: secagg_frac_bits must be an integer in 8 ... 30 (got %r)" % (who, frac_bits))
    return int(frac_bits)


def stream_arrays(streams: Sequence[Stream]):
    """(keys [k][8], nonces [k][3], signs [k]) as the ctypes HOST arrays of the C entry points"""
    import ctypes as C
    k = len(streams)
    keys = (C.c_uint * (8 * k))(*[w for s in streams for w in s[0]])
    nonces = (C.c_uint * (3 * k))(*[w for s in streams for w in s[1]])
    signs = (C.c_int * k)(*[int(s[2]) for s in streams])
    return keys, nonces, signs


def pair_sign(i: int, j: int) -> int:
    """the sign client ``i`` gives the mask it shares with ``j``: +1 for j > i, -1 for j < i (the two ends cancel)"""
    return 1 if j > i else -1


class MaskedUpdate:
    """One client's upload: ``y`` (an int32 device tensor holding the uint32 words y_i of include/fedfr_hip.h), the parameter count ``n``,
    ``frac_bits``, the client's BN running statistics ``stats`` (fp32) and ``counters`` (int64) UNMASKED, and ``code_counters``: a DEVICE
    int32 pair {saturated, nonfinite} — elements whose code hit +-L, elements whose scaled value was NaN or infinite (sent as 0) — read
    back only when ``saturated_count()`` / ``nonfinite_count()`` are asked for.  ``table`` / ``layers`` describe the state the upload
    belongs to (FlatStateDict).  An upload of ``SecAggClient.mask_dp`` carries a third counter, {..., exhausted} (elements whose noise
    sampler ran out of attempts: an error), and ``sqnorm``: a DEVICE int64 holding the exact sum of its squared codes mod 2^64, taken
    before the noise (``sqnorm_value()``), which the server holds against the mechanism's sensitivity.
    ``bits`` is the width of a code: 32 (one word per parameter), or 8 / 16, where ``y`` holds padded_count(n) bits / 32 PACKED words of the
    rotated update and ``rotation_seed`` / ``round`` name the public rotation the server needs to turn the sum back (both public; with them
    the counters cover the padded_count(n) rotated elements)."""

    def __init__(self, y, n, frac_bits, stats, counters, code_counters, table=None, layers=None, sqnorm=None, bits=32, rotation_seed=0, round=0):
        self.y, self.n, self.frac_bits = y, int(n), int(frac_bits)
        self.stats, self.counters, self.code_counters = stats, counters, code_counters
        self.table, self.layers, self.sqnorm = table, layers, sqnorm
        self.bits, self.rotation_seed, self.round = int(bits), int(rotation_seed), int(round)

    @property
    def nbytes(self) -> int:
        """bytes of the upload: masked words, running statistics and counters"""
        return 4 * self.y.numel() + self.stats.numel() * self.stats.element_size() + self.counters.numel() * self.counters.element_size()

    @property
    def dense_nbytes(self) -> int:
        """bytes of the fp32 state this upload replaces"""
        return 4 * self.n + self.stats.numel() * self.stats.element_size() + self.counters.numel() * self.counters.element_size()

    def saturated_count(self) -> int:
        """the counter, read back (a host synchronisation)"""
        return int(self.code_counters[0].item())

    def nonfinite_count(self) -> int:
        return int(self.code_counters[1].item())

    def exhausted_count(self) -> int:
        """the third counter of a ``mask_dp`` upload (0 for a plain one), read back"""
        return int(self.code_counters[2].item()) if self.code_counters.numel() > 2 else 0

    def sqnorm_value(self):
        """the sum of the squared codes as a Python integer in [0, 2^64), read back; None for a plain upload"""
        return None if self.sqnorm is None else int(self.sqnorm.item()) & ((1 << 64) - 1)


class SecAggClient:
    """The protocol state of ONE client.  ``begin_round`` draws a fresh X25519 key pair and a 32-byte self seed b_i; ``make_shares`` hands
    out Shamir shares of the secret key and of b_i, one pair per participant; ``mask`` makes the upload.  With ``bits`` = 8 or 16 the upload
    is one of NARROW WORDS (the module's docstring): ``rotation_seed`` is the public seed all clients and the server share, and
    ``begin_round`` also draws the 64-bit seed of the client's private rounding draws."""

    def __init__(self, cid: int, frac_bits: int = 24, rng: Optional[Rng] = None, bits: int = 32, rotation_seed: int = 0):
        self.cid, self.frac_bits, self.rng = int(cid), check_frac_bits(frac_bits, "SecAggClient"), rng
        self.rounding_seed = None       # the 64-bit seed of the client's rounding draws of the round (narrow widths): drawn in begin_round, never sent
        self.set_width(bits, rotation_seed)
        self.round = None
        self.secret_key = self.public_key = self.self_seed = None
        self.noise_seed = None          # the 64-bit seed of the client's noise share of the round (mask_dp): drawn here, never sent
        self._clipper = None            # mask_dp keeps the workspace of its norm pass here

    def set_width(self, bits: int = 32, rotation_seed: int = 0):
        """the width of the codes (8, 16 or 32) and, for the narrow ones, the public rotation seed; takes effect at the next ``begin_round``"""
        self.bits = check_bits(bits, "SecAggClient")
        self.rotation_seed = check_rotation_seed(rotation_seed, "SecAggClient")
        return self

    def begin_round(self, round: int) -> bytes:
        """fresh secrets for ``round``; returns the public key"""
        self.round = int(round)
        self.secret_key, self.public_key = keypair(self.rng)
        self.self_seed = (self.rng or os.urandom)(32)
        # (drawn behind the secrets of the 32-bit path and at the narrow widths only: that path draws what it always drew)
        self.rounding_seed = int.from_bytes((self.rng or os.urandom)(8), "little") if self.bits != 32 else None
        return self.public_key

    def make_shares(self, participants: Sequence[int], threshold: int) -> Dict[int, Tuple[Share, Share]]:
        """{holder: (share of the secret key, share of b_i)}: participant number p of ``participants`` holds x-coordinate p + 1"""
        if self.secret_key is None:
            raise RuntimeError("SecAggClient.make_shares: begin_round first")
        sk = shamir_split(self.secret_key, len(participants), threshold, self.rng)
        bs = shamir_split(self.self_seed, len(participants), threshold, self.rng)
        return {int(h): (sk[p], bs[p]) for p, h in enumerate(participants)}

    def streams(self, participants: Sequence[int], public_keys: Dict[int, bytes], round: int) -> List[Stream]:
        """the client's streams of ``round``: one pair mask per peer (ascending position in ``participants``), then its self mask"""
        if self.secret_key is None or self.round != int(round):
            raise RuntimeError("SecAggClient: the secrets at hand are those of round %r, not of round %r; begin_round first" % (self.round, round))
        if self.cid not in participants:
            raise ValueError("SecAggClient: client %d is not among the participants %s" % (self.cid, list(participants)))
        out = []
        for j in participants:
            if j != self.cid:
                out.append((derive_key(x25519(self.secret_key, public_keys[j]), self.cid, j), round_nonce(round, PURPOSE_PAIR), pair_sign(self.cid, j)))
        out.append((key_words(self.self_seed), round_nonce(round, PURPOSE_SELF), 1))
        return out

    def mask(self, global_state, client_state, weight: float, participants: Sequence[int], public_keys: Dict[int, bytes], round: int) -> MaskedUpdate:
        """The masked upload of the PARAMETERS of ``client_state`` against ``global_state`` (GPU ``FlatStateDict``s): ONE call of
        fedfr_secagg_mask, which reads both states once and writes the words once.  ``weight`` is the client's public w_i = n_i / sum n;
        statistics and counters are carried as they are."""
        import torch
        from . import _C
        from .client import FlatStateDict
        from .server import _check_states
        if not all(isinstance(s, FlatStateDict) and s.flat is not None for s in (global_state, client_state)):
            raise RuntimeError("fedfr_amd.SecAggClient: the global and the client state must be FlatStateDicts (client.flat_state_dict)")
        K = len(participants)
        if not 2 <= K <= MAX_PARTICIPANTS or len(set(participants)) != K:
            raise ValueError("SecAggClient.mask: 2 to %d distinct participants (got %d: %s)" % (MAX_PARTICIPANTS, K, list(participants)))
        if not 0.0 < float(weight) <= 1.0:
            raise ValueError("SecAggClient.mask: the weight n_i / sum n must be in (0, 1] (got %r)" % (weight,))
        x, (xi, stats, counters) = global_state.flat[0], client_state.flat
        _check_states(x, [xi], "SecAggClient")
        n, dev = x.numel(), x.device
        keys, nonces, signs = stream_arrays(self.streams(participants, public_keys, round))
        cc = torch.zeros(2, dtype=torch.int32, device=dev)
        if self.bits != 32:
            # NARROW WORDS: ONE call of fedfr_secagg_mask_narrow (rotation, stochastic rounding, packing and masks in one pass)
            if self.rounding_seed is None:
                raise RuntimeError("SecAggClient.mask: the secrets at hand were drawn for 32-bit words; set_width(...) and begin_round again")
            y = torch.empty(padded_count(n) * self.bits // 32, dtype=torch.int32, device=dev)
            if n:
                _C.call("fedfr_secagg_mask_narrow", y.data_ptr(), x.data_ptr(), xi.data_ptr(), code_coef(weight, self.frac_bits), K, self.bits,
                        self.rotation_seed, self.rounding_seed, int(round) & 0xFFFFFFFF, keys, nonces, signs, K, 0, n, cc.data_ptr(), _C.stream())
            return MaskedUpdate(y, n, self.frac_bits, stats, counters, cc, client_state.table, client_state.layers, bits=self.bits,
                                rotation_seed=self.rotation_seed, round=int(round) & 0xFFFFFFFF)
        y = torch.empty(n, dtype=torch.int32, device=dev)
        if n:
            _C.call("fedfr_secagg_mask", y.data_ptr(), x.data_ptr(), xi.data_ptr(), code_coef(weight, self.frac_bits), code_limit(K), keys, nonces,
                    signs, K, n, cc.data_ptr(), _C.stream())
        return MaskedUpdate(y, n, self.frac_bits, stats, counters, cc, client_state.table, client_state.layers)


    def mask_dp(self, global_state, client_state, participants: Sequence[int], public_keys: Dict[int, bytes], round: int, mech) -> MaskedUpdate:
        """``mask`` under distributed differential privacy (``mech``: a ``privacy.DistributedDiscreteGaussian`` of this round's K, T, n and
        this client's ``frac_bits``), at weight 1: the norm pass (fedfr_fedopt_sqnorm, which leaves min(1, C / ||x_i - x||) ON THE DEVICE),
        then ONE call of fedfr_secagg_mask_dp, which clips, encodes at the clamp ``mech.code_limit``, sums the squared codes, adds the
        client's noise share of sigma_int and the masks.  No host synchronisation in between.  The 64-bit noise seed is drawn from
        ``rng`` per call and stays here (``noise_seed``: the client knows its own share, nobody else does).
        A client of 16-bit words takes a mechanism of 16-bit words (``DistributedDiscreteGaussian(..., bits=16, wrap_sigmas=kappa)``): the
        norm pass, then ONE call of fedfr_secagg_mask_narrow_dp, and the upload is padded_count(n) / 2 packed words with the rotation
        seed and the round the server turns the sum back with; its counters and ``sqnorm`` cover all padded_count(n) rotated coordinates,
        every one of which carries noise.  A mechanism and a client of different widths raise ``ValueError``, and so do 8-bit words."""
        import torch
        from . import _C
        from .client import FlatStateDict
        from .privacy import DistributedDiscreteGaussian
        from .server import ServerOptimizer, _check_states
        if not all(isinstance(s, FlatStateDict) and s.flat is not None for s in (global_state, client_state)):
            raise RuntimeError("fedfr_amd.SecAggClient: the global and the client state must be FlatStateDicts (client.flat_state_dict)")
        if not isinstance(mech, DistributedDiscreteGaussian):
            raise RuntimeError("fedfr_amd.SecAggClient.mask_dp: mech must be a privacy.DistributedDiscreteGaussian (got %r)" % (type(mech).__name__,))
        if self.bits == 8:
            raise ValueError("SecAggClient.mask_dp: distributed differential privacy at %d-bit words is not provided: %s"
                             % (self.bits, DistributedDiscreteGaussian.WHY_NOT_8))
        if mech.bits != self.bits:
            raise ValueError("SecAggClient.mask_dp: a mechanism of %d-bit words meets a client of %d-bit words (set_width, or "
                             "DistributedDiscreteGaussian(bits=..., wrap_sigmas=...))" % (mech.bits, self.bits))
        K = len(participants)
        if not 2 <= K <= MAX_PARTICIPANTS or len(set(participants)) != K:
            raise ValueError("SecAggClient.mask_dp: 2 to %d distinct participants (got %d: %s)" % (MAX_PARTICIPANTS, K, list(participants)))
        x, (xi, stats, counters) = global_state.flat[0], client_state.flat
        _check_states(x, [xi], "SecAggClient")
        n, dev = x.numel(), x.device
        if (mech.participants, mech.frac_bits, mech.n) != (K, self.frac_bits, n):
            raise ValueError("SecAggClient.mask_dp: the mechanism is one of %d participants, %d fraction bits and %d parameters; this upload has %d, %d "
                             "and %d" % (mech.participants, mech.frac_bits, mech.n, K, self.frac_bits, n))
        keys, nonces, signs = stream_arrays(self.streams(participants, public_keys, round))
        if self._clipper is None or self._clipper.clip_norm != mech.clip_norm:
            self._clipper = ServerOptimizer("AVGM", clip_norm=mech.clip_norm)
        self.noise_seed = int.from_bytes((self.rng or os.urandom)(8), "little")
        cc = torch.zeros(3, dtype=torch.int32, device=dev)
        sq = torch.zeros(1, dtype=torch.int64, device=dev)
        if self.bits == 16:
            # NARROW WORDS UNDER DISTRIBUTED DP: the norm pass, then ONE call of fedfr_secagg_mask_narrow_dp (clip, rotation, stochastic
            # rounding, the sum of the squared codes, the noise of all n_pad rotated coordinates mod 2^16, packing and masks)
            if self.rounding_seed is None:
                raise RuntimeError("SecAggClient.mask_dp: the secrets at hand were drawn for 32-bit words; set_width(...) and begin_round again")
            y = torch.empty(padded_count(n) // 2, dtype=torch.int32, device=dev)
            if n:
                coef = self._clipper.coefficients(x, [xi], [1.0])
                _C.call("fedfr_secagg_mask_narrow_dp", y.data_ptr(), x.data_ptr(), xi.data_ptr(), coef.data_ptr(), self.frac_bits, mech.code_limit, 16,
                        self.rotation_seed, self.rounding_seed, int(round) & 0xFFFFFFFF, self.noise_seed, int(round) & 0xFFFFFFFF, 0, mech.sigma_int,
                        keys, nonces, signs, K, 0, n, cc.data_ptr(), sq.data_ptr(), _C.stream())
            return MaskedUpdate(y, n, self.frac_bits, stats, counters, cc, client_state.table, client_state.layers, sqnorm=sq, bits=16,
                                rotation_seed=self.rotation_seed, round=int(round) & 0xFFFFFFFF)
        y = torch.empty(n, dtype=torch.int32, device=dev)
        if n:
            coef = self._clipper.coefficients(x, [xi], [1.0])
            _C.call("fedfr_secagg_mask_dp", y.data_ptr(), x.data_ptr(), xi.data_ptr(), coef.data_ptr(), self.frac_bits, mech.code_limit, self.noise_seed,
                    int(round) & 0xFFFFFFFF, 0, mech.sigma_int, keys, nonces, signs, K, n, cc.data_ptr(), sq.data_ptr(), _C.stream())
        return MaskedUpdate(y, n, self.frac_bits, stats, counters, cc, client_state.table, client_state.layers, sqnorm=sq)


class SecAggServer:
    """The server's side of ONE round over ``participants`` (distinct integer ids) at ``threshold`` t: it collects the public keys and the
    shares, and after the uploads turns the shares the SURVIVORS hold into the recovery streams.  It raises when fewer than t clients
    survive, and it refuses to reconstruct both the secret key and the self seed of the same client: with both it could unmask that
    client's upload (the protocol's one invariant)."""

    def __init__(self, participants: Sequence[int], threshold: int, round: int = 0):
        self.participants = [int(p) for p in participants]
        K = len(self.participants)
        if len(set(self.participants)) != K or not 2 <= K <= MAX_PARTICIPANTS:
            raise ValueError("SecAggServer: 2 to %d distinct participants (got %d: %s)" % (MAX_PARTICIPANTS, K, self.participants))
        if isinstance(threshold, bool) or not isinstance(threshold, (int, np.integer)) or not 2 <= threshold <= K:
            raise ValueError("SecAggServer: the threshold must be an integer in 2 ... %d (got %r)" % (K, threshold))
        self.threshold, self.round = int(threshold), int(round)
        self.public_keys: Dict[int, bytes] = {}
        self._held: Dict[int, Dict[int, Tuple[Share, Share]]] = {p: {} for p in self.participants}      # holder -> owner -> (sk share, b share)
        self._reconstructed: Dict[int, str] = {}

    def register(self, cid: int, public_key: bytes):
        if cid not in self._held:
            raise ValueError("SecAggServer: client %r is not a participant of this round" % (cid,))
        self.public_keys[int(cid)] = bytes(public_key)

    def deliver_shares(self, owner: int, shares: Dict[int, Tuple[Share, Share]]):
        """route ``owner``'s shares to their holders (in this simulation the holders' mailboxes live here; a share is only ever read
        through a holder that survived)"""
        if sorted(shares) != sorted(self.participants):
            raise ValueError("SecAggServer: client %r must hand one share pair to every participant" % (owner,))
        for holder, pair in shares.items():
            self._held[holder][int(owner)] = pair

    def _reconstruct(self, owner: int, what: str, survivors: Sequence[int]) -> bytes:
        other = self._reconstructed.get(owner)
        if other is not None and other != what:
            raise RuntimeError("SecAggServer: asked for the %s of client %d after its %s: with both the server could unmask the client's upload"
                               % (what, owner, other))
        shares = [self._held[h][owner][0 if what == "secret key" else 1] for h in survivors if owner in self._held[h]]
        if len(shares) < self.threshold:
            raise RuntimeError("SecAggServer: %d shares of client %d's %s from %d survivors, the threshold is %d"
                               % (len(shares), owner, what, len(survivors), self.threshold))
        self._reconstructed[owner] = what
        return shamir_combine(shares)

    def reconstruct_secret_key(self, owner: int, survivors: Sequence[int]) -> bytes:
        return self._reconstruct(int(owner), "secret key", survivors)

    def reconstruct_self_seed(self, owner: int, survivors: Sequence[int]) -> bytes:
        return self._reconstruct(int(owner), "self seed", survivors)

    def recovery_streams(self, survivors: Sequence[int]) -> List[Stream]:
        """What the sum of the survivors' uploads still carries, with the sign that cancels it: minus the self mask of every survivor
        (from its b_i), and the pair masks between every survivor and every dropped client (from the dropped client's secret key)."""
        survivors = [int(s) for s in survivors]
        if len(set(survivors)) != len(survivors) or any(s not in self._held for s in survivors):
            raise ValueError("SecAggServer: the survivors %s are not distinct participants of %s" % (survivors, self.participants))
        if len(survivors) < self.threshold:
            raise RuntimeError("SecAggServer: %d survivors, the threshold is %d: the round cannot be recovered" % (len(survivors), self.threshold))
        missing = [p for p in self.participants if p not in self.public_keys]
        if missing:
            raise RuntimeError("SecAggServer: no public key of clients %s" % missing)
        out: List[Stream] = []
        for i in survivors:
            out.append((key_words(self.reconstruct_self_seed(i, survivors)), round_nonce(self.round, PURPOSE_SELF), -1))
        for d in self.participants:
            if d in survivors:
                continue
            sk = self.reconstruct_secret_key(d, survivors)
            for i in survivors:
                out.append((derive_key(x25519(sk, self.public_keys[i]), i, d), round_nonce(self.round, PURPOSE_PAIR), -pair_sign(i, d)))
        return out


def survivor_rescale(weights: Sequence[float], survivors: Sequence[int]) -> float:
    """fp32(1 / sum of the survivors' w_i), exactly 1.0 when nobody dropped; ``weights`` are the public w_i of ALL participants"""
    if len(survivors) == len(weights):
        return 1.0
    return float(np.float32(1.0 / sum(float(weights[s]) for s in survivors)))
