// Compressed client uploads with error feedback: a client sends Q(x_i - x + e_i) as 8- or 4-bit codes with ONE shared power-of-two scale
// byte per 32 elements (the OCP microscaling layout) and keeps the quantisation error e_i; the server adds up to 8 dequantised uploads per
// pass.  The format is stated in include/fedfr_hip.h (fedfr_delta_quantize) and restated in numpy in tests/compress_cases.py; every scale
// is a power of two, so scaling and rescaling are exact and both kernels are held to that restatement bit for bit.  Both go on the
// streaming skeleton of multi_state.h: its launch rule in the 8-elements-per-thread variant, dispatch_int, read-once loads, a vector loop
// followed by a tail.  Every fp32 operation is an explicit single-rounding intrinsic (the build contracts a*b+c otherwise).
// For the server's clip (and the Gaussian mechanism on top of it) there are two more entry points at the end: delta_sqnorm measures <= 8
// uploads from their codes and scale bytes alone and leaves the clipped weights on the device, delta_aggregate_dp is the aggregate with its
// weights read from there and the noise of dp.h added inside the last pass.
//
// LANE MAPPING.  A lane owns 8 consecutive elements: two 16-byte loads per fp32 input, and its codes leave as one dword (4 bits) or one
// 8-byte store (8 bits).  A block of 32 elements is 4 adjacent lanes, so the block maximum is two xor steps inside a quad (on the integer
// image of |v|: NaN and inf order above every finite value, so the same maximum finds the non-finite blocks).  A wave covers 512 elements = 16
// blocks; their 16 scale bytes are packed by two more xor steps inside a row of 16 lanes and stored as ONE 16-byte store by lane 0.
#include "compress.h"
#include "dp.h"            // DpStream, dp_gauss4: the noise of fedfr_delta_aggregate_dp's last pass
#include "multi_state.h"
#include "optim.h"         // optim_fedopt_sqnorm_final: the last step of the norm pass
#include <cmath>

constexpr int DELTA_EPT = 8;                      // elements per lane
constexpr int DELTA_CHUNK = 64 * DELTA_EPT;       // elements per wave and loop iteration: 512 = 16 blocks of 32
static_assert(MULTI_STATE_BLOCK % 64 == 0 && DELTA_CHUNK % 32 == 0, "whole waves, whole blocks per wave");

struct DeltaWeights {      // the weights of up to 8 uploads as one kernel argument
  float w[8];
};

__device__ __forceinline__ float f32_of_bits(unsigned u) { return __builtin_bit_cast(float, u); }
// 2^(eb - 127) for the scale byte eb: subnormal at eb = 0, NaN at the reserved eb = 255 (a non-finite block dequantises to NaN)
__device__ __forceinline__ float delta_scale(unsigned eb) { return f32_of_bits(eb == 0u ? 0x00400000u : (eb == 255u ? 0x7FC00000u : eb << 23)); }
template <class T>
__device__ __forceinline__ T ld_once_as(const unsigned char* p, size_t i) { return __builtin_nontemporal_load(reinterpret_cast<const T*>(p) + i); }

// ---------------------------------------------------------------------------------------------------------
// quantise.  One wave, one chunk of 512 elements starting at element 512 c.  FULL: the whole chunk lies inside n (16-byte loads, dword-or-
// wider stores); !FULL: the last, partial chunk (guarded 4-byte loads, elements past n count as 0 and are never stored; guarded stores).
// The arithmetic between loads and stores is the same code.
// ---------------------------------------------------------------------------------------------------------
template <int BITS, bool FB, bool FULL>
__device__ __forceinline__ void delta_quantize_chunk(const float* __restrict__ x, const float* __restrict__ xi, float* __restrict__ resid,
                                                     unsigned char* __restrict__ codes, unsigned char* __restrict__ scales, size_t n,
                                                     int* __restrict__ bad_blocks, size_t c, int lane) {
  constexpr int QMAX = (1 << (BITS - 1)) - 1;
  const size_t e0 = c * DELTA_CHUNK + (size_t)lane * DELTA_EPT;      // this lane's first element
  float v[DELTA_EPT];
  if (FULL) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const fvec<4> a = ld_once<4>(xi, e0 / 4 + h), b = ld_once<4>(x, e0 / 4 + h);
      fvec<4> r = {0.f, 0.f, 0.f, 0.f};
      if (FB) r = ld_once<4>(resid, e0 / 4 + h);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float d = __fsub_rn(a[q], b[q]);
        v[4 * h + q] = FB ? __fadd_rn(d, r[q]) : d;
      }
    }
  } else {
#pragma unroll
    for (int j = 0; j < DELTA_EPT; ++j) {
      v[j] = 0.f;
      if (e0 + j < n) {
        const float d = __fsub_rn(xi[e0 + j], x[e0 + j]);
        v[j] = FB ? __fadd_rn(d, resid[e0 + j]) : d;
      }
    }
  }
  // block maximum of |v| as integers: the four lanes of a quad hold one block
  unsigned m = 0u;
#pragma unroll
  for (int j = 0; j < DELTA_EPT; ++j) m = max(m, __builtin_bit_cast(unsigned, v[j]) & 0x7FFFFFFFu);
  m = max(m, (unsigned)__shfl_xor((int)m, 1, 64));
  m = max(m, (unsigned)__shfl_xor((int)m, 2, 64));
  const bool bad = m >= 0x7F800000u;                                  // a NaN or an infinity in the block
  const int ef = (int)(m >> 23);
  const unsigned eb = bad ? 255u : (unsigned)max(ef - (BITS - 2), 0);      // <= 252 for a finite block
  const float inv = f32_of_bits(bad ? 0u : (254u - eb) << 23);        // 2^(127 - eb): a normal number for every eb <= 252
  const float scale = delta_scale(eb);
  int q[DELTA_EPT];
  float e[DELTA_EPT];
#pragma unroll
  for (int j = 0; j < DELTA_EPT; ++j) {
    const float vj = bad ? 0.f : v[j];                                // (a non-finite block: codes 0, residual +0)
    const int r = (int)__builtin_rintf(__fmul_rn(vj, inv));           // round half to even; |v inv| < 2^(BITS - 1)
    q[j] = min(max(r, -QMAX), QMAX);
    e[j] = bad ? 0.f : __fsub_rn(vj, __fmul_rn((float)q[j], scale));
  }
  if (bad && (lane & 3) == 0 && bad_blocks && (FULL || e0 < n)) atomicAdd(bad_blocks, 1);
  if (FULL) {
    if (FB) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const fvec<4> o = {e[4 * h], e[4 * h + 1], e[4 * h + 2], e[4 * h + 3]};
        vec_at<4>(resid, e0 / 4 + h) = o;
      }
    }
    if (BITS == 4) {
      unsigned w = 0u;
#pragma unroll
      for (int j = 0; j < DELTA_EPT; ++j) w |= ((unsigned)q[j] & 15u) << (4 * j);
      reinterpret_cast<unsigned*>(codes)[e0 / 8] = w;
    } else {
      uint2 w = make_uint2(0u, 0u);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        w.x |= ((unsigned)q[j] & 255u) << (8 * j);
        w.y |= ((unsigned)q[4 + j] & 255u) << (8 * j);
      }
      reinterpret_cast<uint2*>(codes)[e0 / 8] = w;
    }
    // the wave's 16 scale bytes: quad g = lane / 4 holds the byte of block g; rows of 16 lanes assemble dword g / 4, lane 0 stores all four
    unsigned u = eb << (8 * ((lane >> 2) & 3));
    u |= (unsigned)__shfl_xor((int)u, 4, 64);
    u |= (unsigned)__shfl_xor((int)u, 8, 64);
    uint4 s;
    s.x = (unsigned)__builtin_amdgcn_readlane((int)u, 0);
    s.y = (unsigned)__builtin_amdgcn_readlane((int)u, 16);
    s.z = (unsigned)__builtin_amdgcn_readlane((int)u, 32);
    s.w = (unsigned)__builtin_amdgcn_readlane((int)u, 48);
    if (lane == 0) reinterpret_cast<uint4*>(scales)[c] = s;
  } else {
#pragma unroll
    for (int j = 0; j < DELTA_EPT; ++j) {
      if (e0 + j < n) {
        if (FB) resid[e0 + j] = e[j];
        if (BITS == 8) codes[e0 + j] = (unsigned char)((unsigned)q[j] & 255u);
      }
    }
    if (BITS == 4) {
#pragma unroll
      for (int p = 0; p < DELTA_EPT / 2; ++p)      // (a missing last element has v = 0: its nibble is 0)
        if (e0 + 2 * p < n) codes[e0 / 2 + p] = (unsigned char)(((unsigned)q[2 * p] & 15u) | (((unsigned)q[2 * p + 1] & 15u) << 4));
    }
    if ((lane & 3) == 0 && e0 < n) scales[e0 / 32] = (unsigned char)eb;
  }
}

// vector loop: the n / 512 whole chunks, grid-stride by WAVES; tail: the last, partial chunk, by the wave whose turn it would be
template <int BITS, bool FB>
__global__ __launch_bounds__(MULTI_STATE_BLOCK) void delta_quantize_kernel(const float* __restrict__ x, const float* __restrict__ xi, float* __restrict__ resid,
                                                                           unsigned char* __restrict__ codes, unsigned char* __restrict__ scales, size_t n,
                                                                           int* __restrict__ bad_blocks) {
  constexpr int WPB = MULTI_STATE_BLOCK / 64;
  const int lane = threadIdx.x & 63;
  const size_t nwaves = (size_t)gridDim.x * WPB, wave = (size_t)blockIdx.x * WPB + (threadIdx.x >> 6);
  const size_t nfull = n / DELTA_CHUNK;
  for (size_t c = wave; c < nfull; c += nwaves) delta_quantize_chunk<BITS, FB, true>(x, xi, resid, codes, scales, n, bad_blocks, c, lane);
  if (n % DELTA_CHUNK != 0 && wave == nfull % nwaves) delta_quantize_chunk<BITS, FB, false>(x, xi, resid, codes, scales, n, bad_blocks, nfull, lane);
}

size_t delta_code_bytes(int bits, size_t n) { return bits == 4 || bits == 8 ? (n * (size_t)bits + 7) / 8 : 0; }
size_t delta_scale_bytes(size_t n) { return (n + 31) / 32; }

int delta_quantize(const float* x, const float* xi, float* resid, void* codes, unsigned char* scales, int bits, size_t n, int* nonfinite_blocks,
                   hipStream_t st) {
  FEDFR_REQUIRE(bits == 4 || bits == 8, "delta_quantize: bits must be 4 or 8 (bits=%d)", bits);
  FEDFR_REQUIRE(x && xi && codes && scales, "delta_quantize: null pointer (x=%p xi=%p codes=%p scales=%p)", (const void*)x, (const void*)xi, codes, (void*)scales);
  FEDFR_REQUIRE((((uintptr_t)x | (uintptr_t)xi | (uintptr_t)resid | (uintptr_t)codes | (uintptr_t)scales) & 15) == 0,
                "delta_quantize: x, xi, resid, codes and scales must be 16-byte aligned");
  FEDFR_REQUIRE(((uintptr_t)nonfinite_blocks & 3) == 0, "delta_quantize: nonfinite_blocks must be 4-byte aligned");
  if (n == 0) return FEDFR_OK;
  unsigned char* cb = static_cast<unsigned char*>(codes);
  const int grid = multi_state_grid_per<DELTA_EPT>(n);
  dispatch_int<0, 3>((bits == 8 ? 2 : 0) + (resid ? 1 : 0), [&](auto vc) {
    constexpr int V = decltype(vc)::value;
    hipLaunchKernelGGL((delta_quantize_kernel<(V & 2) ? 8 : 4, (V & 1) != 0>), dim3(grid), dim3(MULTI_STATE_BLOCK), 0, st, x, xi, resid, cb, scales, n,
                       nonfinite_blocks);
  });
  FEDFR_LAUNCH_CHECK("delta_quantize");
  return FEDFR_OK;
}

// ---------------------------------------------------------------------------------------------------------
// aggregate: s = (accumulate ? dst + w_0 dq_0 : w_0 dq_0), s = s + w_i dq_i ascending i, dst = base ? base + s : s.  dq = float(q) 2^(eb - 127).
// A lane owns 8 elements again: one dword (4 bits) or 8 bytes (8 bits) of codes and one scale byte per upload (the 4 lanes of a block read
// the same byte: one 16-byte segment per wave and upload), two 16-byte accesses for each of dst and base.
// ---------------------------------------------------------------------------------------------------------
template <int BITS>
__device__ __forceinline__ int delta_code(const unsigned (&w)[2], int j) {      // element j of a lane's 8, sign-extended
  if (BITS == 4) return (int)(w[0] << (28 - 4 * j)) >> 28;
  return (int)(w[j >> 2] << (24 - 8 * (j & 3))) >> 24;
}

// The body of the aggregate, written ONCE for the two shells below: w[] are the K weights wherever they came from; with NOISE, noise_std z of
// the stream rs is added to s before base (the host selects NOISE only for the last pass of a chain with noise_std > 0).  A lane's 8
// elements 8 u .. 8 u + 7 are the Philox blocks 2 u and 2 u + 1 of the buffer (rs.blk0 = offset / 4), an element i of the tail is lane i % 4
// of block i / 4: the value depends on the element's index alone.
template <int K, int BITS, bool NOISE>
__device__ __forceinline__ void delta_aggregate_body(float* dst, const float* base, const BytePtrs<8>& codes, const BytePtrs<8>& scales, const float (&wt)[K],
                                                     size_t n, int accumulate, float noise_std, const DpStream& rs, size_t t, size_t stride) {
  const size_t n8 = n / DELTA_EPT;
  for (size_t u = t; u < n8; u += stride) {
    unsigned cw[K][2];
    unsigned eb[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      if (BITS == 4) {
        cw[k][0] = ld_once_as<unsigned>(codes.src[k], u);
        cw[k][1] = 0u;
      } else {
        typedef unsigned u32x2_t __attribute__((ext_vector_type(2)));
        const u32x2_t w = ld_once_as<u32x2_t>(codes.src[k], u);
        cw[k][0] = w.x;
        cw[k][1] = w.y;
      }
      eb[k] = scales.src[k][u >> 2];
    }
    float s[DELTA_EPT] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (accumulate) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const fvec<4> d = vec_at<4>(dst, 2 * u + h);
#pragma unroll
        for (int q = 0; q < 4; ++q) s[4 * h + q] = d[q];
      }
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const float sc = delta_scale(eb[k]);
#pragma unroll
      for (int j = 0; j < DELTA_EPT; ++j) {
        const float term = __fmul_rn(wt[k], __fmul_rn((float)delta_code<BITS>(cw[k], j), sc));
        s[j] = (k == 0 && !accumulate) ? term : __fadd_rn(s[j], term);
      }
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      fvec<4> o = {s[4 * h], s[4 * h + 1], s[4 * h + 2], s[4 * h + 3]};
      if (NOISE) {
        const float4 z = dp_gauss4(rs, 2 * u + h);
        o[0] = __fadd_rn(o[0], __fmul_rn(noise_std, z.x));
        o[1] = __fadd_rn(o[1], __fmul_rn(noise_std, z.y));
        o[2] = __fadd_rn(o[2], __fmul_rn(noise_std, z.z));
        o[3] = __fadd_rn(o[3], __fmul_rn(noise_std, z.w));
      }
      if (base) {
        const fvec<4> b = vec_at<4>(base, 2 * u + h);
#pragma unroll
        for (int q = 0; q < 4; ++q) o[q] = __fadd_rn(b[q], o[q]);
      }
      vec_at<4>(dst, 2 * u + h) = o;
    }
  }
  for (size_t i = n8 * DELTA_EPT + t; i < n; i += stride) {
    float s = accumulate ? dst[i] : 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const unsigned byte = codes.src[k][BITS == 4 ? i >> 1 : i];
      const int q = BITS == 4 ? (int)(byte << (28 - 4 * (int)(i & 1))) >> 28 : (int)(byte << 24) >> 24;
      const float term = __fmul_rn(wt[k], __fmul_rn((float)q, delta_scale(scales.src[k][i >> 5])));
      s = (k == 0 && !accumulate) ? term : __fadd_rn(s, term);
    }
    if (NOISE) s = __fadd_rn(s, __fmul_rn(noise_std, lane_of(dp_gauss4(rs, i >> 2), (int)(i & 3))));
    dst[i] = base ? __fadd_rn(base[i], s) : s;
  }
}

// the shell of fedfr_delta_aggregate: the weights travel by value
template <int K, int BITS>
__global__ __launch_bounds__(MULTI_STATE_BLOCK) void delta_aggregate_kernel(float* dst, const float* base, BytePtrs<8> codes, BytePtrs<8> scales, DeltaWeights wt,
                                                                            size_t n, int accumulate) {
  float w[K];
#pragma unroll
  for (int k = 0; k < K; ++k) w[k] = wt.w[k];
  delta_aggregate_body<K, BITS, false>(dst, base, codes, scales, w, n, accumulate, 0.f, DpStream{}, (size_t)blockIdx.x * blockDim.x + threadIdx.x,
                                       (size_t)gridDim.x * blockDim.x);
}
// the shell of fedfr_delta_aggregate_dp: the weights are what a norm pass left on the device, read once per thread
template <int K, int BITS, bool NOISE>
__global__ __launch_bounds__(MULTI_STATE_BLOCK) void delta_aggregate_dp_kernel(float* dst, const float* base, BytePtrs<8> codes, BytePtrs<8> scales,
                                                                               const float* __restrict__ coef, size_t n, int accumulate, float noise_std, DpStream rs) {
  float w[K];
#pragma unroll
  for (int k = 0; k < K; ++k) w[k] = coef[k];
  delta_aggregate_body<K, BITS, NOISE>(dst, base, codes, scales, w, n, accumulate, noise_std, rs, (size_t)blockIdx.x * blockDim.x + threadIdx.x,
                                       (size_t)gridDim.x * blockDim.x);
}

// what both entry points check and fill; `wname`: how the entry point calls its weights
static int delta_aggregate_args(const char* who, const char* wname, BytePtrs<8>& cp, BytePtrs<8>& sp, float* dst, const float* base, const void* const* codes,
                                const unsigned char* const* scales, const float* w, int k, int bits) {
  FEDFR_REQUIRE(bits == 4 || bits == 8, "%s: bits must be 4 or 8 (bits=%d)", who, bits);
  FEDFR_REQUIRE(k >= 1 && k <= 8, "%s: 1 to 8 uploads per call (k=%d)", who, k);
  FEDFR_REQUIRE(dst && codes && scales && w, "%s: null pointer (dst=%p codes=%p scales=%p %s=%p)", who, (void*)dst, (const void*)codes, (const void*)scales,
                wname, (const void*)w);
  uintptr_t al = (uintptr_t)dst | (uintptr_t)base, al_s = 0;      // (null: no bits)
  FEDFR_TRY(byte_ptrs_fill(cp, codes, k, who, "code buffer", al));
  FEDFR_TRY(byte_ptrs_fill(sp, reinterpret_cast<const void* const*>(scales), k, who, "scale buffer", al_s));
  FEDFR_REQUIRE((al & 15) == 0, "%s: dst, base and the code buffers must be 16-byte aligned", who);
  return FEDFR_OK;
}

int delta_aggregate(float* dst, const float* base, const void* const* codes, const unsigned char* const* scales, const float* ws, int k, int bits,
                    size_t n, int accumulate, hipStream_t st) {
  BytePtrs<8> cp{}, sp{};
  FEDFR_TRY(delta_aggregate_args("delta_aggregate", "ws", cp, sp, dst, base, codes, scales, ws, k, bits));
  DeltaWeights wt{};
  for (int i = 0; i < k; ++i) wt.w[i] = ws[i];
  if (n == 0) return FEDFR_OK;
  accumulate = accumulate ? 1 : 0;
  const int grid = multi_state_grid_per<DELTA_EPT>(n);
  dispatch_int<0, 1>(bits == 8 ? 1 : 0, [&](auto bc) {
    dispatch_int<1, 8>(k, [&](auto kc) {
      hipLaunchKernelGGL((delta_aggregate_kernel<decltype(kc)::value, decltype(bc)::value ? 8 : 4>), dim3(grid), dim3(MULTI_STATE_BLOCK), 0, st, dst, base, cp, sp,
                         wt, n, accumulate);
    });
  });
  FEDFR_LAUNCH_CHECK("delta_aggregate");
  return FEDFR_OK;
}

// Every pass of a chain is given the chain's (noise_std, seed, round, stream_id, offset); only the last one draws, and the entry point keeps
// no state to hold the others to it (as dp_multi).
int delta_aggregate_dp(float* dst, const float* base, const void* const* codes, const unsigned char* const* scales, const float* coef, int k, int bits,
                       size_t n, int accumulate, int last, float noise_std, unsigned long long seed, unsigned long long round, unsigned stream_id,
                       unsigned long long offset, hipStream_t st) {
  BytePtrs<8> cp{}, sp{};
  FEDFR_TRY(delta_aggregate_args("delta_aggregate_dp", "coef", cp, sp, dst, base, codes, scales, coef, k, bits));
  FEDFR_REQUIRE(((uintptr_t)coef & 3) == 0, "delta_aggregate_dp: coef must be 4-byte aligned");
  FEDFR_REQUIRE(std::isfinite(noise_std) && noise_std >= 0.f, "delta_aggregate_dp: noise_std must be finite and >= 0 (got %g)", (double)noise_std);
  FEDFR_REQUIRE(offset % 4 == 0, "delta_aggregate_dp: offset %llu is not a multiple of 4", offset);
  if (n == 0) return FEDFR_OK;
  accumulate = accumulate ? 1 : 0;
  const int grid = multi_state_grid_per<DELTA_EPT>(n);
  const DpStream rs = dp_stream(seed, round, stream_id, offset);
  dispatch_int<0, 3>((bits == 8 ? 2 : 0) + (last && noise_std > 0.f ? 1 : 0), [&](auto vc) {
    constexpr int V = decltype(vc)::value;
    dispatch_int<1, 8>(k, [&](auto kc) {
      hipLaunchKernelGGL((delta_aggregate_dp_kernel<decltype(kc)::value, (V & 2) ? 8 : 4, (V & 1) != 0>), dim3(grid), dim3(MULTI_STATE_BLOCK), 0, st, dst, base,
                         cp, sp, coef, n, accumulate, noise_std, rs);
    });
  });
  FEDFR_LAUNCH_CHECK("delta_aggregate_dp");
  return FEDFR_OK;
}

// ---------------------------------------------------------------------------------------------------------
// squared norms of <= 8 uploads as the server will apply them: sq_i = sum_j dq_i[j]^2, from the codes and scale bytes alone.  A lane owns 8
// elements again (one dword or 8 bytes of codes); the four lanes of a quad hold one block of 32, whose S_b = sum q^2 is an INTEGER (<= 32 * 128^2)
// formed by two xor steps, and whose T_b = double(S_b) 4^(eb - 127) is EXACT in fp64 for eb = 0..254 (a 20-bit integer times a power of two inside
// 2^-254 .. 2^254; eb = 255: NaN).  The quad's first lane adds T_b to its fp64 sum, one rounding per block, in its grid-stride order; then
// block_partial_d and fedopt_sqnorm_final_kernel (optim.hip): the fixed order of fedopt_sqnorm, no atomics, every partial written by its block.
// ONE loop over the ceil(n / 8) units, quad-uniform (a quad enters while its first unit exists: the shuffles see all four lanes).  WHOLE: the
// quad's block lies inside n, and the K code words and scale bytes are loaded before anything is computed (K independent loads in flight);
// !WHOLE: the last, short block, whose units are read byte by byte and whose elements at index >= n are dropped, so nothing is read behind
// ceil(n bits / 8) code bytes and whatever a client left in the pad nibble or behind n is not counted.
// ---------------------------------------------------------------------------------------------------------
template <int K, int BITS, bool WHOLE>
__device__ __forceinline__ void delta_sqnorm_unit(const BytePtrs<8>& codes, const BytePtrs<8>& scales, size_t n, size_t u, double (&acc)[K]) {
  const size_t e0 = u * DELTA_EPT;
  unsigned cw[K][2];
  unsigned eb[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    cw[k][0] = cw[k][1] = 0u;
    if (WHOLE) {
      if (BITS == 4) {
        cw[k][0] = ld_once_as<unsigned>(codes.src[k], u);
      } else {
        typedef unsigned u32x2_t __attribute__((ext_vector_type(2)));
        const u32x2_t w = ld_once_as<u32x2_t>(codes.src[k], u);
        cw[k][0] = w.x;
        cw[k][1] = w.y;
      }
    } else {
#pragma unroll
      for (int b = 0; b < BITS; ++b) {      // byte b of the unit holds the elements from e0 + b (8 / BITS) on: read only if one of them is below n
        if (e0 + (size_t)b * (8 / BITS) < n) cw[k][b >> 2] |= (unsigned)codes.src[k][u * BITS + b] << (8 * (b & 3));
      }
    }
    eb[k] = scales.src[k][u >> 2];      // (u / 4 < ceil(n / 32): the quad's first unit exists)
  }
#pragma unroll
  for (int k = 0; k < K; ++k) {
    int sb = 0;
#pragma unroll
    for (int j = 0; j < DELTA_EPT; ++j) {
      const int q = (WHOLE || e0 + j < n) ? delta_code<BITS>(cw[k], j) : 0;
      sb += q * q;
    }
    sb += __shfl_xor(sb, 1, 64);
    sb += __shfl_xor(sb, 2, 64);
    // 4^(eb - 127) = 2^(2 eb - 254): the fp64 exponent field 2 eb + 769 (769 .. 1277 for eb <= 254); eb = 255: a quiet NaN
    const double f = __hiloint2double(eb[k] == 255u ? 0x7FF80000 : (int)((2u * eb[k] + 769u) << 20), 0);
    // (double)sb * f is exact, so a contracted fma rounds as the separate multiply and add do: once, in the sum
    if ((threadIdx.x & 3) == 0) acc[k] += (double)sb * f;
  }
}

template <int K, int BITS>
__global__ __launch_bounds__(MULTI_STATE_BLOCK) void delta_sqnorm_kernel(BytePtrs<8> codes, BytePtrs<8> scales, size_t n, double* __restrict__ part) {
  __shared__ double red[4][8];
  double acc[K];
#pragma unroll
  for (int k = 0; k < K; ++k) acc[k] = 0.0;
  const size_t stride = (size_t)gridDim.x * blockDim.x, t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t nunits = (n + DELTA_EPT - 1) / DELTA_EPT;
  for (size_t u = t; (u & ~(size_t)3) < nunits; u += stride) {
    if (((u | 3) + 1) * DELTA_EPT <= n) delta_sqnorm_unit<K, BITS, true>(codes, scales, n, u, acc);      // (the same for the four lanes of a quad)
    else delta_sqnorm_unit<K, BITS, false>(codes, scales, n, u, acc);
  }
  block_partial_d<K>(acc, red, part, [](int k) { return k; });
}

size_t upload_sqnorm_ws_bytes(int k, size_t m) {
  if (k < 1 || k > 8) return 0;
  return (size_t)k * multi_state_grid_per<DELTA_EPT>(m) * sizeof(double);
}

int delta_sqnorm(const void* const* codes, const unsigned char* const* scales, const float* ws, int k, int bits, size_t n, float clip, double* sq,
                 float* coef, void* wsp, size_t ws_bytes, hipStream_t st) {
  FEDFR_REQUIRE(bits == 4 || bits == 8, "delta_sqnorm: bits must be 4 or 8 (bits=%d)", bits);
  FEDFR_REQUIRE(k >= 1 && k <= 8, "delta_sqnorm: 1 to 8 uploads per call (k=%d)", k);
  FEDFR_REQUIRE(codes && scales && ws && sq && coef && wsp, "delta_sqnorm: null pointer (codes=%p scales=%p ws=%p sq=%p coef=%p workspace=%p)", (const void*)codes,
                (const void*)scales, (const void*)ws, (void*)sq, (void*)coef, wsp);
  FEDFR_REQUIRE(n > 0, "delta_sqnorm: n must be positive");
  FEDFR_REQUIRE(clip == clip, "delta_sqnorm: clip is NaN");
  BytePtrs<8> cp{}, sp{};
  uintptr_t al = 0, al_s = 0;
  FEDFR_TRY(byte_ptrs_fill(cp, codes, k, "delta_sqnorm", "code buffer", al));
  FEDFR_TRY(byte_ptrs_fill(sp, reinterpret_cast<const void* const*>(scales), k, "delta_sqnorm", "scale buffer", al_s));
  FEDFR_REQUIRE((al & 15) == 0, "delta_sqnorm: the code buffers must be 16-byte aligned");
  FEDFR_REQUIRE((((uintptr_t)sq | (uintptr_t)wsp) & 7) == 0 && ((uintptr_t)coef & 3) == 0, "delta_sqnorm: sq / workspace must be 8-byte, coef 4-byte aligned");
  const int grid = multi_state_grid_per<DELTA_EPT>(n);
  if (ws_bytes < (size_t)k * grid * sizeof(double)) {
    fedfr_set_error("delta_sqnorm: workspace of %zu bytes, %zu needed", ws_bytes, (size_t)k * grid * sizeof(double));
    return FEDFR_ERR_WORKSPACE;
  }
  double* part = reinterpret_cast<double*>(wsp);
  dispatch_int<0, 1>(bits == 8 ? 1 : 0, [&](auto bc) {
    dispatch_int<1, 8>(k, [&](auto kc) {
      hipLaunchKernelGGL((delta_sqnorm_kernel<decltype(kc)::value, decltype(bc)::value ? 8 : 4>), dim3(grid), dim3(MULTI_STATE_BLOCK), 0, st, cp, sp, n, part);
    });
  });
  FEDFR_LAUNCH_CHECK("delta_sqnorm");
  return optim_fedopt_sqnorm_final(part, grid, k, ws, clip, sq, coef, st);
}
