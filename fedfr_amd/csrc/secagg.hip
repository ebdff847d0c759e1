// Secure aggregation on the flat parameter buffer: a client uploads its fixed-point update under pairwise and self masks, and the server,
// which removes the masks of the uploads it received with the recovery streams, learns only the sum.  The format (mask stream, encoding,
// masked upload, aggregate) is stated in include/fedfr_hip.h and restated in numpy in tests/secagg_cases.py; everything between the fp32
// encoding and the final conversion is integer arithmetic mod 2^32, so all three kernels are held to that restatement bit for bit:
//   chacha20_fill_kernel          the raw words of one stream: the part that pins the generator (secagg.h)
//   secagg_mask_kernel            y = encode(xi - x) + sum_s sign_s m_s, one pass: x and xi read once, y written once
//   secagg_aggregate_kernel<KU>   S = (first ? 0 : acc) + sum of KU uploads + sum_r sign_r m_r;  last ? out = (x +) float(S) 2^-f rescale : acc = S
// On the streaming skeleton of multi_state.h in its 16-elements-per-thread variant.  The generator's natural mapping is one ChaCha20 block
// = 16 consecutive elements per lane, which puts a lane's four 16-byte accesses 64 B apart and a wave's access on 64 separate segments;
// mask and aggregate therefore touch memory in the contiguous layout and pass only the generated words through LDS (THE EXCHANGE below):
// measured against the direct mapping in DESIGN.md section 3.26.  The streams are wave-uniform kernel arguments; the kernels are
// integer-VALU-bound from about 3 streams upward.
#include "secagg.h"
#include "multi_state.h"
#include <cmath>

__global__ __launch_bounds__(MULTI_STATE_BLOCK) void chacha20_fill_kernel(unsigned* __restrict__ dst, size_t n, ChaChaStream cs) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const size_t nb = n / SECAGG_EPT, nball = (n + SECAGG_EPT - 1) / SECAGG_EPT;
  for (size_t b = (size_t)blockIdx.x * blockDim.x + threadIdx.x; b < nball; b += stride) {
    unsigned w[16];
    chacha_block(cs.key, cs.counter0 + (unsigned)b, cs.nonce[0], cs.nonce[1], cs.nonce[2], w);
    if (b < nb) {
#pragma unroll
      for (int h = 0; h < 4; ++h) reinterpret_cast<uvec4*>(dst)[4 * b + h] = uvec4{w[4 * h], w[4 * h + 1], w[4 * h + 2], w[4 * h + 3]};
    } else {
#pragma unroll
      for (int j = 0; j < SECAGG_EPT; ++j)
        if (b * SECAGG_EPT + j < n) dst[b * SECAGG_EPT + j] = w[j];
    }
  }
}

// Whole chunks of 1024 elements go wave by wave in the memory layout (lane L: 16-byte slots 64 h + L): codes there, the sum of the streams
// generated in the block layout and passed through the exchange (not at all when k = 0).  The n % 1024 elements behind them (up to 63
// whole blocks and a partial one) go lane by lane in the block layout with guarded accesses.
__global__ __launch_bounds__(MULTI_STATE_BLOCK) void secagg_mask_kernel(unsigned* __restrict__ y, const float* __restrict__ x, const float* __restrict__ xi,
                                                                        float coef, int limit, MaskStreams ms, int k, size_t n,
                                                                        int* __restrict__ counters) {
  __shared__ uvec4 xch[SECAGG_WPB][SECAGG_CHUNK / 4];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const size_t nwaves = (size_t)gridDim.x * SECAGG_WPB, wave = (size_t)blockIdx.x * SECAGG_WPB + wv;
  const size_t nchunk = n / SECAGG_CHUNK;
  int saturated = 0, nonfinite = 0;
  for (size_t c = wave; c < nchunk; c += nwaves) {
    const size_t v0 = c * (SECAGG_CHUNK / 4) + lane;      // this lane's first 16-byte slot
    unsigned q[16];
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      const fvec<4> a = ld_once<4>(xi, v0 + 64 * h), b = ld_once<4>(x, v0 + 64 * h);
#pragma unroll
      for (int j = 0; j < 4; ++j) q[4 * h + j] = secagg_encode(a[j], b[j], coef, limit, saturated, nonfinite);
    }
    if (k > 0) {
      unsigned m[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) m[j] = 0u;
      chacha_add_streams(m, ms, k, (unsigned)(c * 64 + lane));
      block_to_memory_layout(xch[wv], m, lane);
#pragma unroll
      for (int j = 0; j < 16; ++j) q[j] += m[j];
    }
#pragma unroll
    for (int h = 0; h < 4; ++h) reinterpret_cast<uvec4*>(y)[v0 + 64 * h] = uvec4{q[4 * h], q[4 * h + 1], q[4 * h + 2], q[4 * h + 3]};
  }
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const size_t nball = (n + SECAGG_EPT - 1) / SECAGG_EPT;
  for (size_t b = nchunk * 64 + (size_t)blockIdx.x * blockDim.x + threadIdx.x; b < nball; b += stride) {
    unsigned q[16];
#pragma unroll
    for (int j = 0; j < SECAGG_EPT; ++j) {
      const size_t e = b * SECAGG_EPT + j;
      q[j] = 0u;
      if (e < n) q[j] = secagg_encode(xi[e], x[e], coef, limit, saturated, nonfinite);
    }
    chacha_add_streams(q, ms, k, (unsigned)b);
#pragma unroll
    for (int j = 0; j < SECAGG_EPT; ++j)
      if (b * SECAGG_EPT + j < n) y[b * SECAGG_EPT + j] = q[j];
  }
  if (counters) {
    if (saturated) atomicAdd(counters, saturated);
    if (nonfinite) atomicAdd(counters + 1, nonfinite);
  }
}

// The same two loops.  out may be x (both are touched by the same lane, read before write); acc is read when !first, written when !last
template <int KU>
__global__ __launch_bounds__(MULTI_STATE_BLOCK) void secagg_aggregate_kernel(float* out, const float* x, unsigned* acc, BytePtrs<SECAGG_MAX_UPLOADS> ys,
                                                                             MaskStreams ms, int k, float scale, float rescale, size_t n, int first,
                                                                             int last) {
  __shared__ uvec4 xch[SECAGG_WPB][SECAGG_CHUNK / 4];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const size_t nwaves = (size_t)gridDim.x * SECAGG_WPB, wave = (size_t)blockIdx.x * SECAGG_WPB + wv;
  const size_t nchunk = n / SECAGG_CHUNK;
  for (size_t c = wave; c < nchunk; c += nwaves) {
    const size_t v0 = c * (SECAGG_CHUNK / 4) + lane;
    unsigned s[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) s[j] = 0u;
    if (!first) {
#pragma unroll
      for (int h = 0; h < 4; ++h) {
        const uvec4 a = reinterpret_cast<const uvec4*>(acc)[v0 + 64 * h];
#pragma unroll
        for (int j = 0; j < 4; ++j) s[4 * h + j] = a[j];
      }
    }
#pragma unroll
    for (int u = 0; u < KU; ++u) {
#pragma unroll
      for (int h = 0; h < 4; ++h) {
        const uvec4 a = ld_once_u4(reinterpret_cast<const unsigned*>(ys.src[u]), v0 + 64 * h);
#pragma unroll
        for (int j = 0; j < 4; ++j) s[4 * h + j] += a[j];
      }
    }
    if (k > 0) {
      unsigned m[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) m[j] = 0u;
      chacha_add_streams(m, ms, k, (unsigned)(c * 64 + lane));
      block_to_memory_layout(xch[wv], m, lane);
#pragma unroll
      for (int j = 0; j < 16; ++j) s[j] += m[j];
    }
    if (!last) {
#pragma unroll
      for (int h = 0; h < 4; ++h) reinterpret_cast<uvec4*>(acc)[v0 + 64 * h] = uvec4{s[4 * h], s[4 * h + 1], s[4 * h + 2], s[4 * h + 3]};
      continue;
    }
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      fvec<4> o;
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = __fmul_rn(__fmul_rn((float)(int)s[4 * h + j], scale), rescale);
      if (x) {
        const fvec<4> xv = vec_at<4>(x, v0 + 64 * h);
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = __fadd_rn(xv[j], o[j]);
      }
      vec_at<4>(out, v0 + 64 * h) = o;
    }
  }
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const size_t nball = (n + SECAGG_EPT - 1) / SECAGG_EPT;
  for (size_t b = nchunk * 64 + (size_t)blockIdx.x * blockDim.x + threadIdx.x; b < nball; b += stride) {
    unsigned s[16];
#pragma unroll
    for (int j = 0; j < SECAGG_EPT; ++j) {
      const size_t e = b * SECAGG_EPT + j;
      s[j] = 0u;
      if (e < n) {
        if (!first) s[j] = acc[e];
#pragma unroll
        for (int u = 0; u < KU; ++u) s[j] += reinterpret_cast<const unsigned*>(ys.src[u])[e];
      }
    }
    chacha_add_streams(s, ms, k, (unsigned)b);
#pragma unroll
    for (int j = 0; j < SECAGG_EPT; ++j) {
      const size_t e = b * SECAGG_EPT + j;
      if (e >= n) continue;
      if (!last) acc[e] = s[j];
      else {
        const float d = __fmul_rn(__fmul_rn((float)(int)s[j], scale), rescale);
        out[e] = x ? __fadd_rn(x[e], d) : d;
      }
    }
  }
}

int secagg_chacha20_fill(unsigned* dst, size_t n, const unsigned* key, unsigned counter0, const unsigned* nonce, hipStream_t st) {
  FEDFR_REQUIRE(dst && key && nonce, "chacha20_fill: null pointer (dst=%p key=%p nonce=%p)", (void*)dst, (const void*)key, (const void*)nonce);
  FEDFR_REQUIRE(((uintptr_t)dst & 15) == 0, "chacha20_fill: dst (%p) must be 16-byte aligned", (void*)dst);
  if (n == 0) return FEDFR_OK;
  FEDFR_TRY(counter_fits("chacha20_fill", n, counter0));
  ChaChaStream cs{};
  for (int i = 0; i < 8; ++i) cs.key[i] = key[i];
  for (int i = 0; i < 3; ++i) cs.nonce[i] = nonce[i];
  cs.counter0 = counter0;
  hipLaunchKernelGGL(chacha20_fill_kernel, dim3(multi_state_grid_per<SECAGG_EPT>(n)), dim3(MULTI_STATE_BLOCK), 0, st, dst, n, cs);
  FEDFR_LAUNCH_CHECK("chacha20_fill");
  return FEDFR_OK;
}

int secagg_mask(unsigned* y, const float* x, const float* xi, float coef, int limit, const unsigned* keys, const unsigned* nonces,
                const int* signs, int k, size_t n, int* counters, hipStream_t st) {
  FEDFR_REQUIRE(y && x && xi, "secagg_mask: null pointer (y=%p x=%p xi=%p)", (void*)y, (const void*)x, (const void*)xi);
  FEDFR_REQUIRE(limit >= 1, "secagg_mask: limit must be >= 1 (limit=%d)", limit);
  MaskStreams ms{};
  FEDFR_TRY(mask_streams_fill(ms, "secagg_mask", keys, nonces, signs, k));
  FEDFR_REQUIRE((((uintptr_t)y | (uintptr_t)x | (uintptr_t)xi) & 15) == 0, "secagg_mask: y (%p), x (%p) and xi (%p) must be 16-byte aligned", (void*)y,
                (const void*)x, (const void*)xi);
  FEDFR_REQUIRE(((uintptr_t)counters & 3) == 0, "secagg_mask: counters (%p) must be 4-byte aligned", (void*)counters);
  if (n == 0) return FEDFR_OK;
  FEDFR_TRY(counter_fits("secagg_mask", n, 0u));
  hipLaunchKernelGGL(secagg_mask_kernel, dim3(multi_state_grid_per<SECAGG_EPT>(n)), dim3(MULTI_STATE_BLOCK), 0, st, y, x, xi, coef, limit, ms, k, n, counters);
  FEDFR_LAUNCH_CHECK("secagg_mask");
  return FEDFR_OK;
}

int secagg_aggregate(float* out, const float* x, unsigned* acc, const unsigned* const* ys, int ku, const unsigned* keys, const unsigned* nonces,
                     const int* signs, int k, int frac_bits, float rescale, size_t n, int first, int last, hipStream_t st) {
  FEDFR_REQUIRE(ku >= 0 && ku <= SECAGG_MAX_UPLOADS, "secagg_aggregate: 0 to %d uploads per call (ku=%d)", SECAGG_MAX_UPLOADS, ku);
  MaskStreams ms{};
  FEDFR_TRY(mask_streams_fill(ms, "secagg_aggregate", keys, nonces, signs, k));
  FEDFR_REQUIRE(k + ku > 0, "secagg_aggregate: nothing to add (ku=%d, k=%d)", ku, k);
  FEDFR_REQUIRE(ku == 0 || ys, "secagg_aggregate: null pointer (ys=%p) with ku=%d", (const void*)ys, ku);
  FEDFR_REQUIRE(frac_bits >= 8 && frac_bits <= 30, "secagg_aggregate: frac_bits must be 8 to 30 (frac_bits=%d)", frac_bits);
  FEDFR_REQUIRE(std::isfinite(rescale), "secagg_aggregate: rescale must be finite (rescale=%g)", (double)rescale);
  first = first ? 1 : 0;
  last = last ? 1 : 0;
  FEDFR_REQUIRE((first && last) || acc, "secagg_aggregate: a chained pass (first=%d last=%d) needs acc", first, last);
  FEDFR_REQUIRE(!last || out, "secagg_aggregate: the last pass (last=%d) needs out", last);
  BytePtrs<SECAGG_MAX_UPLOADS> yp{};
  uintptr_t al = (uintptr_t)out | (uintptr_t)x | (uintptr_t)acc;      // (null: no bits)
  FEDFR_TRY(byte_ptrs_fill(yp, reinterpret_cast<const void* const*>(ys), ku, "secagg_aggregate", "upload", al));
  FEDFR_REQUIRE((al & 15) == 0, "secagg_aggregate: out (%p), x (%p), acc (%p) and the uploads must be 16-byte aligned", (void*)out, (const void*)x,
                (void*)acc);
  if (n == 0) return FEDFR_OK;
  FEDFR_TRY(counter_fits("secagg_aggregate", n, 0u));
  const float scale = std::ldexp(1.0f, -frac_bits);
  dispatch_int<0, SECAGG_MAX_UPLOADS>(ku, [&](auto kc) {
    hipLaunchKernelGGL((secagg_aggregate_kernel<decltype(kc)::value>), dim3(multi_state_grid_per<SECAGG_EPT>(n)), dim3(MULTI_STATE_BLOCK), 0, st, out,
                       last ? x : nullptr, acc, yp, ms, k, scale, rescale, n, first, last);
  });
  FEDFR_LAUNCH_CHECK("secagg_aggregate");
  return FEDFR_OK;
}
