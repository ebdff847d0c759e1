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
#include "multi_state.h"

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

// ---- shared by the kernels of secagg.hip and ddp.hip: the exchange, the encoder and the host-side checks, written ONCE -----------------
typedef unsigned uvec4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uvec4 ld_once_u4(const unsigned* p, size_t i) { return __builtin_nontemporal_load(reinterpret_cast<const uvec4*>(p) + i); }

constexpr int SECAGG_WPB = MULTI_STATE_BLOCK / 64;          // waves per workgroup
constexpr int SECAGG_CHUNK = 64 * SECAGG_EPT;               // elements per wave and loop iteration: 64 blocks = 256 16-byte slots
static_assert(MULTI_STATE_BLOCK % 64 == 0, "whole waves");

// THE EXCHANGE.  The generator leaves lane L of a wave with the 16 words of block L: slots 4 L + j, j < 4, of the wave's chunk of 256
// 16-byte slots, 64 B apart from lane to lane.  Memory wants lane L on slot 64 h + L, h < 4: one contiguous KiB per instruction.  The wave
// passes its 4 KiB through LDS: block layout in, memory layout out.  Slot s lives at s ^ ((s >> 4) & 3): the block-layout writes of 8
// neighbouring lanes then fall on 4 bank groups instead of 2, and every memory-layout ds_read_b128 lane group reads 16 distinct
// slots of a 256-byte bank row.  One wave owns the buffer: no workgroup barrier, only the wave's own program order.
__device__ __forceinline__ int xch_slot(int s) { return s ^ ((s >> 4) & 3); }
__device__ __forceinline__ void block_to_memory_layout(uvec4* __restrict__ buf, unsigned (&m)[16], int lane) {
#pragma unroll
  for (int j = 0; j < 4; ++j) buf[xch_slot(4 * lane + j)] = uvec4{m[4 * j], m[4 * j + 1], m[4 * j + 2], m[4 * j + 3]};
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
  for (int h = 0; h < 4; ++h) {
    const uvec4 v = buf[xch_slot(64 * h + lane)];
    m[4 * h] = v.x; m[4 * h + 1] = v.y; m[4 * h + 2] = v.z; m[4 * h + 3] = v.w;
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");      // (the next iteration's writes stay behind these reads)
  __builtin_amdgcn_wave_barrier();
}

// One element's code: d = xi - x, t = d coef, q = clamp(rint(t), -limit, limit); a t that is NaN or infinite gives 0.  rint(t) is an
// integer-valued float: below 2^31 in magnitude it converts exactly, and beyond that it is past every limit.
__device__ __forceinline__ unsigned secagg_encode(float xi, float x, float coef, int limit, int& saturated, int& nonfinite) {
  const float t = __fmul_rn(__fsub_rn(xi, x), coef);
  const bool finite = __builtin_fabsf(t) < __builtin_inff();
  const float r = __builtin_rintf(t);      // round half to even
  const float rc = __builtin_fminf(__builtin_fmaxf(finite ? r : 0.f, -0x1p31f), 0x1.fffffep30f);      // inside int32: the conversion is exact
  int q = min(max((int)rc, -limit), limit);
  q = r >= 0x1p31f ? limit : q;                                                                        // (inf and NaN: finite is false)
  q = finite ? q : 0;
  saturated += (finite && (q == limit || q == -limit)) ? 1 : 0;
  nonfinite += finite ? 0 : 1;
  return (unsigned)q;
}

// the one 32-bit block counter: the last block of n elements from counter0 on must not pass 2^32 - 1
static inline int counter_fits(const char* who, size_t n, unsigned counter0) {
  const unsigned long long last = (unsigned long long)counter0 + (unsigned long long)((n - 1) / SECAGG_EPT);
  FEDFR_REQUIRE(last <= 0xFFFFFFFFull, "%s: the 32-bit block counter overflows (counter0=%u, n=%zu: last block %llu > 4294967295)", who, counter0, n,
                last);
  return FEDFR_OK;
}
// keys [k][8], nonces [k][3], signs [k] (HOST arrays) -> the kernel argument
static inline int mask_streams_fill(MaskStreams& ms, const char* who, const unsigned* keys, const unsigned* nonces, const int* signs, int k) {
  FEDFR_REQUIRE(k >= 0 && k <= SECAGG_MAX_STREAMS, "%s: 0 to %d streams per call (k=%d)", who, SECAGG_MAX_STREAMS, k);
  FEDFR_REQUIRE(k == 0 || (keys && nonces && signs), "%s: null pointer (keys=%p nonces=%p signs=%p) with k=%d", who, (const void*)keys,
                (const void*)nonces, (const void*)signs, k);
  for (int s = 0; s < k; ++s) {
    FEDFR_REQUIRE(signs[s] == 1 || signs[s] == -1, "%s: sign %d is %d, not +1 or -1", who, s, signs[s]);
    for (int i = 0; i < 8; ++i) ms.key[s][i] = keys[8 * s + i];
    for (int i = 0; i < 3; ++i) ms.nonce[s][i] = nonces[3 * s + i];
    ms.sign[s] = signs[s];
  }
  return FEDFR_OK;
}

int secagg_chacha20_fill(unsigned* dst, size_t n, const unsigned* key, unsigned counter0, const unsigned* nonce, hipStream_t st);
int secagg_mask(unsigned* y, const float* x, const float* xi, float coef, int limit, const unsigned* keys, const unsigned* nonces,
                const int* signs, int k, size_t n, int* counters, hipStream_t st);
int secagg_aggregate(float* out, const float* x, unsigned* acc, const unsigned* const* ys, int ku, const unsigned* keys,
                     const unsigned* nonces, const int* signs, int k, int frac_bits, float rescale, size_t n, int first, int last,
                     hipStream_t st);
