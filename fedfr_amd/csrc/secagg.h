// Secure aggregation (Bonawitz et al., "Practical Secure Aggregation for Privacy-Preserving Machine Learning", CCS 2017) on the flat
// parameter buffer (see secagg.hip): the mask generator, written ONCE here for every kernel that draws from it, and the host entry points.
//
// THE MASK STREAM.  The generator is the ChaCha20 block function of RFC 8439 section 2.3: state words 0-3 the constants, 4-11 the key as 8
// little-endian words, 12 the block counter, 13-15 three nonce words; 10 double rounds, then the input state is added.  Element e of the
// stream (key, counter0, nonce[3]) is word e % 16 of block counter0 + e / 16, so a value depends on (key, nonce, counter0, e) and on
// nothing else: not on the grid, not on the number of streams a launch adds, not on how passes are chained.  The counter is ONE 32-bit
// word: the entries refuse a call whose last block would pass 2^32 - 1.  tests/secagg_cases.py restates the words bit for bit.
#pragma once
#include "common.h"

constexpr int SECAGG_MAX_STREAMS = 32;      // streams per launch
constexpr int SECAGG_MAX_UPLOADS = 8;       // uploads per aggregate pass
constexpr int SECAGG_EPT = 16;              // elements per lane: one ChaCha20 block

// up to 32 streams as ONE kernel argument (12 words each, 1.5 KB): wave-uniform, read through scalar loads
struct MaskStreams {
  unsigned key[SECAGG_MAX_STREAMS][8];
  unsigned nonce[SECAGG_MAX_STREAMS][3];
  int sign[SECAGG_MAX_STREAMS];             // +1 / -1
};
struct ChaChaStream {                       // one stream with its first block (fedfr_chacha20_fill)
  unsigned key[8];
  unsigned counter0;
  unsigned nonce[3];
};

__device__ __forceinline__ unsigned chacha_rotl(unsigned v, int r) { return (v << r) | (v >> (32 - r)); }      // one v_alignbit_b32
__device__ __forceinline__ void chacha_quarter(unsigned& a, unsigned& b, unsigned& c, unsigned& d) {
  a += b; d ^= a; d = chacha_rotl(d, 16);
  c += d; b ^= c; b = chacha_rotl(b, 12);
  a += b; d ^= a; d = chacha_rotl(d, 8);
  c += d; b ^= c; b = chacha_rotl(b, 7);
}
// the 16 words of block `counter` of the stream (key, nonce).  key and nonce are wave-uniform (SGPRs); only word 12 differs between lanes.
__device__ __forceinline__ void chacha_block(const unsigned* key, unsigned counter, unsigned n0, unsigned n1, unsigned n2, unsigned (&w)[16]) {
  const unsigned s[16] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u, key[0], key[1], key[2], key[3],
                          key[4],      key[5],      key[6],      key[7],      counter, n0,     n1,     n2};
#pragma unroll
  for (int i = 0; i < 16; ++i) w[i] = s[i];
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    chacha_quarter(w[0], w[4], w[8], w[12]);
    chacha_quarter(w[1], w[5], w[9], w[13]);
    chacha_quarter(w[2], w[6], w[10], w[14]);
    chacha_quarter(w[3], w[7], w[11], w[15]);
    chacha_quarter(w[0], w[5], w[10], w[15]);
    chacha_quarter(w[1], w[6], w[11], w[12]);
    chacha_quarter(w[2], w[7], w[8], w[13]);
    chacha_quarter(w[3], w[4], w[9], w[14]);
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) w[i] += s[i];
}
// acc[0 .. 16) += sum over the k streams of sign_s * (block `counter` of stream s), mod 2^32.  The loop over the streams stays a loop (one
// copy of the 10 double rounds in the code, whatever k); the sign is wave-uniform: a scalar branch.
__device__ __forceinline__ void chacha_add_streams(unsigned (&acc)[16], const MaskStreams& ms, int k, unsigned counter) {
#pragma unroll 1
  for (int s = 0; s < k; ++s) {
    unsigned w[16];
    chacha_block(ms.key[s], counter, ms.nonce[s][0], ms.nonce[s][1], ms.nonce[s][2], w);
    if (ms.sign[s] > 0) {
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[i] += w[i];
    } else {
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[i] -= w[i];
    }
  }
}

int secagg_chacha20_fill(unsigned* dst, size_t n, const unsigned* key, unsigned counter0, const unsigned* nonce, hipStream_t st);
int secagg_mask(unsigned* y, const float* x, const float* xi, float coef, int limit, const unsigned* keys, const unsigned* nonces,
                const int* signs, int k, size_t n, int* counters, hipStream_t st);
int secagg_aggregate(float* out, const float* x, unsigned* acc, const unsigned* const* ys, int ku, const unsigned* keys,
                     const unsigned* nonces, const int* signs, int k, int frac_bits, float rescale, size_t n, int first, int last,
                     hipStream_t st);
