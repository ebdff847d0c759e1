// Distributed differential privacy under secure aggregation (Kairouz, Liu, Steinke, "The Distributed Discrete Gaussian Mechanism for
// Federated Learning with Secure Aggregation", ICML 2021; see ddp.hip): the discrete Gaussian sampler, written ONCE here for every kernel
// that draws from it, and the host entry points.
//
// THE SAMPLER.  The target is N_Z(0, sigma^2), P(y) ~ exp(-y^2 / 2 sigma^2) on the integers, 16 <= sigma <= 2^26 given in fp64.  It is the
// rejection scheme of Canonne, Kamath, Steinke ("The Discrete Gaussian for Differential Privacy", NeurIPS 2020, Algorithm 3): a discrete
// Laplace proposal of scale t = floor(sigma) + 1, thinned to the Gaussian, with the probabilities evaluated in fp64.
//
// THE DISCRETE NOISE STREAM.  Attempt a = 0 ... 63 of element e = offset + j of the logical stream (seed, round, stream_id) takes ALL FOUR
// words (w0, w1, w2, w3) of the Philox4x32-10 block of dp.h with
//   key     = (seed low 32 bits, seed high 32 bits)
//   counter = (blk low 32, blk high 32, round low 32, stream_id),  blk = e * 64 + a as a 64-bit number
// so a value depends on (seed, round, stream_id, e) and on nothing else: not on the grid, not on the lane, not on how many attempts a
// neighbour needed.  One attempt, every operation one fp64 rounding (DGauss holds the three constants, formed on the host):
//   U1 = double((w0 2^21 + (w1 >> 11)) + 1) 2^-53 in (0, 1]   (exact);   B = w1 & 1
//   G  = floor(fl(-t log(U1)))                                 (a geometric magnitude: P(G = g) ~ exp(-g / t));  |G| <= 37 t since U1 >= 2^-53
//   reject if B == 1 and G == 0 (zero is proposed once);  Y = B ? -G : G
//   U2 = double(w2 2^21 + (w3 >> 11)) 2^-53 in [0, 1)          (exact)
//   d  = fl(G - s2t),  s2t = fl(fl(sigma sigma) / t);   p = exp(fl(fl(d d) c)),  c = fl(-1 / fl(2 fl(sigma sigma)))
//   accept iff U2 < p
// The first accepted attempt is the value; after 64 rejections (about 10^-40 per element at an acceptance rate of 0.76) the value is 0 and
// the caller counts the element as exhausted.  tests/ddp_cases.py restates the words bit for bit and the formula operation by operation;
// log and exp are the library's fp64 functions, which may differ from another library's in the last place (the tests' one accepted
// deviation, see there).
#pragma once
#include "dp.h"
#include "secagg.h"
#include <cmath>

constexpr int DGAUSS_ATTEMPTS = 64;
constexpr unsigned DDP_NOISE_STREAM = 0x44444750u;      // "DDGP": the stream_id of the clients' noise shares (include/fedfr_hip.h)

struct DGauss {       // the constants of one sigma
  double t;           // floor(sigma) + 1
  double s2t;         // sigma^2 / t
  double c;           // -1 / (2 sigma^2)
};
static inline DGauss dgauss_params(double sigma) {
  const double t = std::floor(sigma) + 1.0, s2 = sigma * sigma;
  return DGauss{t, s2 / t, -1.0 / (2.0 * s2)};
}
// the stream whose block of (element e, attempt a) is dp_words(s, e * 64 + a)
static inline DpStream dgauss_stream(unsigned long long seed, unsigned long long round, unsigned sid, unsigned long long offset) {
  return DpStream{(unsigned)seed, (unsigned)(seed >> 32), (unsigned)round, sid, offset * (unsigned long long)DGAUSS_ATTEMPTS};
}

// one attempt from the four words of its block: accepted?, and the value mod 2^32 (|Y| <= 37 t < 2^32)
__device__ __forceinline__ bool dgauss_attempt(const uint4& w, const DGauss& g, unsigned& y) {
  const unsigned long long m1 = ((unsigned long long)w.x << 21) | (unsigned long long)(w.y >> 11);
  const unsigned long long m2 = ((unsigned long long)w.z << 21) | (unsigned long long)(w.w >> 11);
  const double u1 = __dmul_rn((double)(m1 + 1ull), 0x1p-53);
  const double u2 = __dmul_rn((double)m2, 0x1p-53);
  const bool neg = (w.y & 1u) != 0u;
  const double G = __builtin_floor(__dmul_rn(-g.t, log(u1)));
  const double d = __dsub_rn(G, g.s2t);
  const double p = exp(__dmul_rn(__dmul_rn(d, d), g.c));
  const unsigned mag = (unsigned)(unsigned long long)G;
  y = neg ? 0u - mag : mag;
  return !(neg && G == 0.0) && u2 < p;
}

// THE QUEUE.  A lane owns `cnt` <= 16 elements, elem(i) their indices in the buffer, and works through them as a queue: every trip of the
// loop is ONE attempt of the lane's current element, and an accepted (or exhausted) element makes room for the next one.  The wave leaves
// the loop when its slowest lane has emptied its queue, after max over the lanes of the SUM of 16 attempt counts (16 x 1.31 on average,
// about 28 for the slowest of 64 lanes) instead of the sum of 16 maxima (16 x 3.7) that one element per trip would cost: the two fp64
// transcendentals of a trip run with most lanes active.  The values go to out[i * 64 + lane], the wave's LDS strip (a dynamically indexed
// register array would live in scratch); a lane reads back only what it wrote itself, so no barrier is needed.  Returns the number of
// exhausted elements.
template <class Elem>
__device__ __forceinline__ int dgauss_queue(unsigned* __restrict__ out, int lane, int cnt, const DpStream& s, const DGauss& g, Elem&& elem) {
  int i = 0, a = 0, exhausted = 0;
  while (__builtin_amdgcn_ballot_w64(i < cnt) != 0ull) {
    if (i < cnt) {
      unsigned y;
      const bool ok = dgauss_attempt(dp_words(s, (unsigned long long)elem(i) * DGAUSS_ATTEMPTS + (unsigned)a), g, y);
      if (ok || a == DGAUSS_ATTEMPTS - 1) {
        out[i * 64 + lane] = ok ? y : 0u;
        exhausted += ok ? 0 : 1;
        ++i;
        a = 0;
      } else {
        ++a;
      }
    }
  }
  return exhausted;
}

// what every entry point that draws n elements behind `offset` checks first
static inline int dgauss_args(const char* who, double sigma, size_t n, unsigned long long offset) {
  FEDFR_REQUIRE(sigma >= 16.0 && sigma <= 0x1p26, "%s: sigma must be in [16, 2^26] (sigma=%g)", who, sigma);      // (NaN fails both)
  FEDFR_REQUIRE(offset <= (1ull << 58) && n <= (1ull << 58) - offset,
                "%s: offset + n must not pass 2^58: 64 blocks per element in a 64-bit block index (offset=%llu, n=%zu)", who, offset, n);
  return FEDFR_OK;
}

int ddp_dgauss_fill(int* dst, size_t n, unsigned long long seed, unsigned long long round, unsigned stream_id, unsigned long long offset,
                    double sigma, int* exhausted, hipStream_t st);
int ddp_secagg_mask_dp(unsigned* y, const float* x, const float* xi, const float* clip_coef, int frac_bits, int limit,
                       unsigned long long noise_seed, unsigned long long noise_round, unsigned long long noise_offset, double sigma,
                       const unsigned* keys, const unsigned* nonces, const int* signs, int k, size_t n, int* counters,
                       unsigned long long* sqnorm, hipStream_t st);
// ddp_narrow.hip: the same mechanism on the 16-bit NARROW WORDS of secagg_narrow.h
int ddp_secagg_mask_narrow_dp(unsigned* y, const float* x, const float* xi, const float* clip_coef, int frac_bits, int limit, int bits,
                              unsigned long long rotation_seed, unsigned long long private_seed, unsigned long long round,
                              unsigned long long noise_seed, unsigned long long noise_round, unsigned long long noise_offset, double sigma,
                              const unsigned* keys, const unsigned* nonces, const int* signs, int k, unsigned counter0, size_t n, int* counters,
                              unsigned long long* sqnorm, hipStream_t st);
