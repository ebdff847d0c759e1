// Client-level differential privacy on the flat parameter buffer (see dp.hip): the counter-based noise generator, written ONCE here for
// every kernel that draws from it, and the host entry points.
//
// THE STREAM.  Element e = offset + j of the logical stream (seed, round, stream_id) takes lane e % 4 of the Philox4x32-10 block with
//   key     = (seed low 32 bits, seed high 32 bits)
//   counter = (blk low 32, blk high 32, round low 32, stream_id),  blk = e / 4 as a 64-bit number
// so a value depends on (seed, round, stream_id, e) and on nothing else: not on the grid, not on the number of client states a launch
// reads, not on how many passes a chain takes.  Lanes (0, 1) and (2, 3) are Box-Muller pairs (dp_gauss_pair).  tests/dp_cases.py restates
// the words bit for bit and the Gaussian formula in fp64.
#pragma once
#include "common.h"

struct DpStream {                 // one logical stream as a kernel argument
  unsigned k0, k1;                // the key: seed low, seed high
  unsigned round, sid;            // counter words 2 and 3
  unsigned long long blk0;        // offset / 4: the block of the buffer's element 0
};
static inline DpStream dp_stream(unsigned long long seed, unsigned long long round, unsigned sid, unsigned long long offset) {
  return DpStream{(unsigned)seed, (unsigned)(seed >> 32), (unsigned)round, sid, offset / 4};
}

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3"; the Random123 constants) of block blk0 + b
__device__ __forceinline__ uint4 dp_words(const DpStream& s, unsigned long long b) {
  const unsigned long long blk = s.blk0 + b;
  unsigned c0 = (unsigned)blk, c1 = (unsigned)(blk >> 32), c2 = s.round, c3 = s.sid, k0 = s.k0, k1 = s.k1;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;            // (the bump after the last round is dead code)
    k1 += 0xBB67AE85u;
  }
  return make_uint4(c0, c1, c2, c3);
}
// One Box-Muller pair from two words.  u1 = ((ra >> 8) + 1) 2^-24 in (0, 1] and u2 = (rb >> 8) 2^-24 in [0, 1) are exact in fp32; the
// angle goes through the pi-scaled functions, so 2 u2 (exact) is their argument and no product with pi is rounded.  |z| <= sqrt(48 ln 2).
// Every product is an explicit single rounding: both kernels that call this get the same bits whatever surrounds the call.
__device__ __forceinline__ void dp_gauss_pair(unsigned ra, unsigned rb, float& z_even, float& z_odd) {
  const float u1 = __fmul_rn((float)((ra >> 8) + 1u), 0x1p-24f);
  const float u2 = __fmul_rn((float)(rb >> 8), 0x1p-24f);
  const float rad = __builtin_sqrtf(__fmul_rn(-2.f, logf(u1)));
  const float a = __fmul_rn(2.f, u2);
  z_even = __fmul_rn(rad, cospif(a));
  z_odd = __fmul_rn(rad, sinpif(a));
}
// the four standard normal values of block blk0 + b
__device__ __forceinline__ float4 dp_gauss4(const DpStream& s, unsigned long long b) {
  const uint4 w = dp_words(s, b);
  float4 z;
  dp_gauss_pair(w.x, w.y, z.x, z.y);
  dp_gauss_pair(w.z, w.w, z.z, z.w);
  return z;
}
__device__ __forceinline__ float lane_of(const float4& z, int lane) { return lane == 0 ? z.x : (lane == 1 ? z.y : (lane == 2 ? z.z : z.w)); }
__device__ __forceinline__ unsigned lane_of(const uint4& w, int lane) { return lane == 0 ? w.x : (lane == 1 ? w.y : (lane == 2 ? w.z : w.w)); }

int dp_philox_fill(unsigned* dst, size_t n, unsigned long long seed, unsigned long long round, unsigned stream_id, unsigned long long offset,
                   hipStream_t st);
int dp_gaussian_fill(float* dst, size_t n, unsigned long long seed, unsigned long long round, unsigned stream_id, unsigned long long offset,
                     float std, int accumulate, hipStream_t st);
int dp_multi(int kind, float* x_out, const float* x, const float* const* xs, const float* coef, int k, size_t n, float* m, float* v,
             float* scratch, int first, int last, float lr, float beta1, float one_minus_beta1, float beta2, float one_minus_beta2, float tau,
             float noise_std, unsigned long long seed, unsigned long long round, unsigned stream_id, unsigned long long offset, hipStream_t st);
