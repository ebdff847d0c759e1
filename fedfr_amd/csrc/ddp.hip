// Distributed differential privacy under secure aggregation: every client adds its own share of integer Gaussian noise to its clipped
// fixed-point update BEFORE masking it, so the sum the server unmasks carries the noise of the mechanism and no party ever holds an
// un-noised sum (the distributed discrete Gaussian of Kairouz, Liu, Steinke, ICML 2021).  The sampler and its stream are stated in ddp.h
// and include/fedfr_hip.h and restated in numpy in tests/ddp_cases.py; the encoding, the masks and the layout of the pass are those of
// secagg.hip (secagg.h):
//   dgauss_fill_kernel     the bare noise values of one stream: the part that pins the sampler
//   ddp_mask_kernel        y = encode((xi - x) clip_coef 2^f) + noise + sum_s sign_s m_s, one pass: x and xi read once, y written once, and
//                          the exact integer sum of the squared codes (taken before the noise) for the sensitivity check
// Per element the pass spends 1.31 attempts on average, each one Philox block, one fp64 log and one fp64 exp: it is bound by the fp64
// transcendentals, not by memory (measured in DESIGN.md section 3.27).  The loop over the attempts is THE QUEUE of ddp.h.
#include "ddp.h"
#include <cmath>

__global__ __launch_bounds__(MULTI_STATE_BLOCK) void dgauss_fill_kernel(unsigned* __restrict__ dst, size_t n, DpStream ns, DGauss g,
                                                                        int* __restrict__ exhausted_out) {
  __shared__ unsigned nz[SECAGG_WPB][SECAGG_CHUNK];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const size_t nball = (n + SECAGG_EPT - 1) / SECAGG_EPT;
  int exhausted = 0;
  for (size_t b = (size_t)blockIdx.x * blockDim.x + threadIdx.x; b < nball; b += stride) {
    const size_t e0 = b * SECAGG_EPT;
    const int cnt = n - e0 < (size_t)SECAGG_EPT ? (int)(n - e0) : SECAGG_EPT;
    exhausted += dgauss_queue(nz[wv], lane, cnt, ns, g, [&](int i) { return e0 + i; });
#pragma unroll
    for (int i = 0; i < SECAGG_EPT; ++i)
      if (i < cnt) dst[e0 + i] = nz[wv][i * 64 + lane];
  }
  if (exhausted) atomicAdd(exhausted_out, exhausted);
}

// The two loops of secagg_mask_kernel.  A lane draws the noise of its 16 elements first (the queue, into the wave's LDS strip), then
// encodes them, squares the codes, adds the noise and the masks.  In the memory layout of the whole chunks the lane's value i = 4 h + j
// is element 1024 c + 256 h + 4 lane + j; in the block layout of the tail it is element 16 b + i.
__global__ __launch_bounds__(MULTI_STATE_BLOCK) void ddp_mask_kernel(unsigned* __restrict__ y, const float* __restrict__ x, const float* __restrict__ xi,
                                                                     const float* __restrict__ clip_coef, float scale, int limit, DpStream ns, DGauss g,
                                                                     MaskStreams ms, int k, size_t n, int* __restrict__ counters,
                                                                     unsigned long long* __restrict__ sqnorm) {
  __shared__ uvec4 xch[SECAGG_WPB][SECAGG_CHUNK / 4];
  __shared__ unsigned nz[SECAGG_WPB][SECAGG_CHUNK];
  __shared__ unsigned long long red[SECAGG_WPB];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const size_t nwaves = (size_t)gridDim.x * SECAGG_WPB, wave = (size_t)blockIdx.x * SECAGG_WPB + wv;
  const size_t nchunk = n / SECAGG_CHUNK;
  const float coef = __fmul_rn(clip_coef[0], scale);      // min(1, C / ||xi - x||) 2^f: a power-of-two scaling, exact
  int saturated = 0, nonfinite = 0, exhausted = 0;
  unsigned long long sq = 0ull;
  for (size_t c = wave; c < nchunk; c += nwaves) {
    const size_t v0 = c * (SECAGG_CHUNK / 4) + lane;      // this lane's first 16-byte slot
    const size_t e0 = c * SECAGG_CHUNK + 4 * lane;
    exhausted += dgauss_queue(nz[wv], lane, 16, ns, g, [&](int i) { return e0 + (size_t)(i >> 2) * 256 + (i & 3); });
    unsigned q[16];
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      const fvec<4> a = ld_once<4>(xi, v0 + 64 * h), b = ld_once<4>(x, v0 + 64 * h);
#pragma unroll
      for (int j = 0; j < 4; ++j) q[4 * h + j] = secagg_encode(a[j], b[j], coef, limit, saturated, nonfinite);
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const long long qi = (int)q[i];
      sq += (unsigned long long)(qi * qi);
      q[i] += nz[wv][i * 64 + lane];
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
    const size_t e0 = b * SECAGG_EPT;
    const int cnt = n - e0 < (size_t)SECAGG_EPT ? (int)(n - e0) : SECAGG_EPT;
    exhausted += dgauss_queue(nz[wv], lane, cnt, ns, g, [&](int i) { return e0 + i; });
    unsigned q[16];
#pragma unroll
    for (int j = 0; j < SECAGG_EPT; ++j) {
      q[j] = 0u;
      if (j < cnt) {
        q[j] = secagg_encode(xi[e0 + j], x[e0 + j], coef, limit, saturated, nonfinite);
        const long long qi = (int)q[j];
        sq += (unsigned long long)(qi * qi);
        q[j] += nz[wv][j * 64 + lane];
      }
    }
    chacha_add_streams(q, ms, k, (unsigned)b);
#pragma unroll
    for (int j = 0; j < SECAGG_EPT; ++j)
      if (j < cnt) y[e0 + j] = q[j];
  }
  if (counters) {
    if (saturated) atomicAdd(counters, saturated);
    if (nonfinite) atomicAdd(counters + 1, nonfinite);
    if (exhausted) atomicAdd(counters + 2, exhausted);
  }
  // the sum of the squared codes: lanes (shuffles), waves (LDS), then ONE 64-bit atomic add per workgroup.  Integer addition mod 2^64 has
  // one result whatever the order
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sq += __shfl_xor(sq, o, 64);
  if (lane == 0) red[wv] = sq;
  __syncthreads();
  if (threadIdx.x == 0 && sqnorm) {
    unsigned long long s = 0ull;
#pragma unroll
    for (int w = 0; w < SECAGG_WPB; ++w) s += red[w];
    if (s) atomicAdd(sqnorm, s);
  }
}

int ddp_dgauss_fill(int* dst, size_t n, unsigned long long seed, unsigned long long round, unsigned stream_id, unsigned long long offset,
                    double sigma, int* exhausted, hipStream_t st) {
  FEDFR_REQUIRE(dst && exhausted, "dgauss_fill: null pointer (dst=%p exhausted=%p)", (void*)dst, (void*)exhausted);
  FEDFR_REQUIRE(((uintptr_t)dst & 15) == 0 && ((uintptr_t)exhausted & 3) == 0, "dgauss_fill: dst (%p) must be 16-byte, exhausted (%p) 4-byte aligned",
                (void*)dst, (void*)exhausted);
  FEDFR_TRY(dgauss_args("dgauss_fill", sigma, n, offset));
  if (n == 0) return FEDFR_OK;
  hipLaunchKernelGGL(dgauss_fill_kernel, dim3(multi_state_grid_per<SECAGG_EPT>(n)), dim3(MULTI_STATE_BLOCK), 0, st, reinterpret_cast<unsigned*>(dst), n,
                     dgauss_stream(seed, round, stream_id, offset), dgauss_params(sigma), exhausted);
  FEDFR_LAUNCH_CHECK("dgauss_fill");
  return FEDFR_OK;
}

int ddp_secagg_mask_dp(unsigned* y, const float* x, const float* xi, const float* clip_coef, int frac_bits, int limit, unsigned long long noise_seed,
                       unsigned long long noise_round, unsigned long long noise_offset, double sigma, const unsigned* keys, const unsigned* nonces,
                       const int* signs, int k, size_t n, int* counters, unsigned long long* sqnorm, hipStream_t st) {
  FEDFR_REQUIRE(y && x && xi && clip_coef, "secagg_mask_dp: null pointer (y=%p x=%p xi=%p clip_coef=%p)", (void*)y, (const void*)x, (const void*)xi,
                (const void*)clip_coef);
  FEDFR_REQUIRE(frac_bits >= 8 && frac_bits <= 30, "secagg_mask_dp: frac_bits must be 8 to 30 (frac_bits=%d)", frac_bits);
  FEDFR_REQUIRE(limit >= 1, "secagg_mask_dp: code_limit must be >= 1 (code_limit=%d)", limit);
  FEDFR_TRY(dgauss_args("secagg_mask_dp", sigma, n, noise_offset));
  MaskStreams ms{};
  FEDFR_TRY(mask_streams_fill(ms, "secagg_mask_dp", keys, nonces, signs, k));
  FEDFR_REQUIRE((((uintptr_t)y | (uintptr_t)x | (uintptr_t)xi) & 15) == 0, "secagg_mask_dp: y (%p), x (%p) and xi (%p) must be 16-byte aligned", (void*)y,
                (const void*)x, (const void*)xi);
  FEDFR_REQUIRE(((uintptr_t)clip_coef & 3) == 0 && ((uintptr_t)counters & 3) == 0 && ((uintptr_t)sqnorm & 7) == 0,
                "secagg_mask_dp: clip_coef (%p) and counters (%p) must be 4-byte, sqnorm (%p) 8-byte aligned", (const void*)clip_coef, (void*)counters,
                (void*)sqnorm);
  if (n == 0) return FEDFR_OK;
  FEDFR_TRY(counter_fits("secagg_mask_dp", n, 0u));
  hipLaunchKernelGGL(ddp_mask_kernel, dim3(multi_state_grid_per<SECAGG_EPT>(n)), dim3(MULTI_STATE_BLOCK), 0, st, y, x, xi, clip_coef,
                     std::ldexp(1.0f, frac_bits), limit, dgauss_stream(noise_seed, noise_round, DDP_NOISE_STREAM, noise_offset), dgauss_params(sigma), ms, k,
                     n, counters, sqnorm);
  FEDFR_LAUNCH_CHECK("secagg_mask_dp");
  return FEDFR_OK;
}
