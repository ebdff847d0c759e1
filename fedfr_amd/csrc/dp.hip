// Client-level DP-FedAvg (McMahan et al., "Learning Differentially Private Recurrent Language Models") on the flat parameter buffer: the
// Gaussian mechanism's noise fused into the server optimisers' streaming pass.  The clip is fedopt_sqnorm's (optim.hip); here:
//   philox_fill_kernel     the raw words of the noise stream (dp.h), the part a host restatement reproduces bit for bit
//   gaussian_fill_kernel   dst (+)= std z
//   dp_multi_kernel<K, KIND>   the shell of fedopt_pass (fedopt_step.h) WITH noise: Delta += noise_std z before the step of the LAST pass, and
//                          the kind FEDOPT_PLAIN (x' = x + Delta, no moments).  optim.hip's fedopt_multi_kernel is the shell without noise;
//                          the noise is dp_gauss4 (dp.h), so this kernel and gaussian_fill round alike.
// All on the skeleton of multi_state.h: one thread per float4 = one Philox block, grid-stride, then the n % 4 tail, whose elements are the
// leading lanes of the block behind the last whole one.
#include "dp.h"
#include "optim.h"
#include "multi_state.h"
#include "fedopt_step.h"
#include <cmath>

__global__ __launch_bounds__(MULTI_STATE_BLOCK) void philox_fill_kernel(unsigned* __restrict__ dst, size_t n, DpStream rs) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const size_t n4 = n / 4;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) reinterpret_cast<uint4*>(dst)[i] = dp_words(rs, i);
  for (size_t i = n4 * 4 + (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) dst[i] = lane_of(dp_words(rs, n4), (int)(i & 3));
}

__global__ __launch_bounds__(MULTI_STATE_BLOCK) void gaussian_fill_kernel(float* __restrict__ dst, size_t n, DpStream rs, float sd, int accumulate) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const size_t n4 = n / 4;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    float4 d = accumulate ? reinterpret_cast<float4*>(dst)[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 z = dp_gauss4(rs, i);
    d.x = __fadd_rn(d.x, __fmul_rn(sd, z.x));
    d.y = __fadd_rn(d.y, __fmul_rn(sd, z.y));
    d.z = __fadd_rn(d.z, __fmul_rn(sd, z.z));
    d.w = __fadd_rn(d.w, __fmul_rn(sd, z.w));
    reinterpret_cast<float4*>(dst)[i] = d;
  }
  for (size_t i = n4 * 4 + (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const float d = accumulate ? dst[i] : 0.f;
    dst[i] = __fadd_rn(d, __fmul_rn(sd, lane_of(dp_gauss4(rs, n4), (int)(i & 3))));
  }
}

static int fill_args(const char* who, const void* dst, size_t n, unsigned long long offset) {
  FEDFR_REQUIRE(dst && n > 0, "%s: bad args", who);
  FEDFR_REQUIRE(((uintptr_t)dst & 15) == 0, "%s: the buffer must be 16-byte aligned", who);
  FEDFR_REQUIRE(offset % 4 == 0, "%s: offset %llu is not a multiple of 4", who, offset);
  return FEDFR_OK;
}
int dp_philox_fill(unsigned* dst, size_t n, unsigned long long seed, unsigned long long round, unsigned stream_id, unsigned long long offset,
                   hipStream_t st) {
  FEDFR_TRY(fill_args("philox_fill", dst, n, offset));
  hipLaunchKernelGGL(philox_fill_kernel, dim3(multi_state_grid(n)), dim3(MULTI_STATE_BLOCK), 0, st, dst, n, dp_stream(seed, round, stream_id, offset));
  FEDFR_LAUNCH_CHECK("philox_fill");
  return FEDFR_OK;
}
int dp_gaussian_fill(float* dst, size_t n, unsigned long long seed, unsigned long long round, unsigned stream_id, unsigned long long offset,
                     float sd, int accumulate, hipStream_t st) {
  FEDFR_TRY(fill_args("gaussian_fill", dst, n, offset));
  FEDFR_REQUIRE(std::isfinite(sd), "gaussian_fill: std is not finite");
  hipLaunchKernelGGL(gaussian_fill_kernel, dim3(multi_state_grid(n)), dim3(MULTI_STATE_BLOCK), 0, st, dst, n, dp_stream(seed, round, stream_id, offset), sd,
                     accumulate ? 1 : 0);
  FEDFR_LAUNCH_CHECK("gaussian_fill");
  return FEDFR_OK;
}

// the pass with noise: fedopt_pass (fedopt_step.h; first / last / scratch, the aliasing rules and the wave-uniform noise test: see there)
template <int K, int KIND>
__global__ __launch_bounds__(MULTI_STATE_BLOCK) void dp_multi_kernel(float* xo, const float* x, StatePtrs<8> p, const float* __restrict__ coef, float* __restrict__ m,
                                                                     float* __restrict__ v, float* scratch, size_t n, int first, int last, FedoptHyper h,
                                                                     float noise_std, DpStream rs) {
  fedopt_pass<K, KIND, true>(xo, x, p, coef, m, v, scratch, n, first, last, h, noise_std, rs, (size_t)blockIdx.x * blockDim.x + threadIdx.x,
                             (size_t)gridDim.x * blockDim.x);
}

// The checks of optim_fedopt_multi (fedopt_pass_args, with FEDOPT_PLAIN admitted), and: noise_std finite and >= 0, offset % 4 == 0.  A chain's
// passes must all be given the chain's (noise_std, seed, round, stream_id, offset): only the last one draws, but the entry point keeps no
// state to hold the others to it.  noise_std == 0 with one of fedopt_multi's four kinds IS fedopt_multi: routed there, so the bits are its own.
int dp_multi(int kind, float* x_out, const float* x, const float* const* xs, const float* coef, int k, size_t n, float* m, float* v,
             float* scratch, int first, int last, float lr, float beta1, float one_minus_beta1, float beta2, float one_minus_beta2, float tau,
             float noise_std, unsigned long long seed, unsigned long long round, unsigned stream_id, unsigned long long offset, hipStream_t st) {
  FEDFR_REQUIRE(kind >= FEDOPT_AVGM && kind <= FEDOPT_PLAIN, "dp_multi: unknown optimiser kind %d", kind);      // (under this name, before the routing)
  FEDFR_REQUIRE(std::isfinite(noise_std) && noise_std >= 0.f, "dp_multi: noise_std must be finite and >= 0 (got %g)", (double)noise_std);
  FEDFR_REQUIRE(offset % 4 == 0, "dp_multi: offset %llu is not a multiple of 4", offset);
  if (noise_std == 0.f && kind != FEDOPT_PLAIN) {
    return optim_fedopt_multi(kind, x_out, x, xs, coef, k, n, m, v, scratch, first, last, lr, beta1, one_minus_beta1, beta2, one_minus_beta2, tau, st);
  }
  FedoptPassArgs a;
  FEDFR_TRY(fedopt_pass_args("dp_multi", FEDOPT_PLAIN, a, kind, x_out, x, xs, coef, k, n, m, v, scratch, first, last, lr, beta1, one_minus_beta1, beta2,
                             one_minus_beta2, tau));
  const DpStream rs = dp_stream(seed, round, stream_id, offset);
  dispatch_int<FEDOPT_AVGM, FEDOPT_PLAIN>(kind, [&](auto kindc) {
    dispatch_int<1, 8>(k, [&](auto kc) {
      hipLaunchKernelGGL((dp_multi_kernel<decltype(kc)::value, decltype(kindc)::value>), dim3(multi_state_grid(n)), dim3(MULTI_STATE_BLOCK), 0, st, x_out, x, a.p,
                         coef, m, v, scratch, n, a.first, a.last, a.h, noise_std, rs);
    });
  });
  FEDFR_LAUNCH_CHECK("dp_multi");
  return FEDFR_OK;
}
