// HBM-bound flat-buffer kernels: fused momentum-SGD (+bf16 weight shadow), FedAvg scale/accumulate,
// PartialFC sampling (counter-based RNG, radix top-k select, ordered compaction), row gather/scatter.
// Reference semantics: torch.optim.SGD as used in client.py:335,527-529; server.py:25-46; partial_fc.py:89-116.
#include "optim.h"
#include "gemm_dev.h"   // ProfScope
#include "multi_state.h"
#include "fedopt_step.h"

// ---------------------------------------------------------------------------------------------------------
// SGD: g += wd*p ; buf = first ? g : mu*buf + g ; p -= lr*buf ; optional bf16 shadow of the new p.
// Op order / fusion mirrors torch's vectorised CPU kernels (alpha-adds are fmadd, mul_ then add_ are two roundings).
// ---------------------------------------------------------------------------------------------------------
// DRIFT TERMS (include/fedfr_hip.h): with ANCHOR the proximal pull a (p - x) of FedProx, with CORR the control-variate correction c - c_i of
// SCAFFOLD, both added to the decayed gradient BEFORE the momentum: d1 = fma(a, fsub(p, x), d0); d = fadd(d1, corr).  Without them (the two
// instantiations training has always run) the function is the three operations it has always been.
template <bool ANCHOR, bool CORR>
__device__ __forceinline__ float sgd_one(float p, float g, float& buf, float lr, float mu, float wd, int first, float a, float x, float c) {
  float d = fmaf(wd, p, g);                                        // grad.add(param, alpha=wd)   (fmadd in torch)
  if (ANCHOR) d = fmaf(a, __fsub_rn(p, x), d);
  if (CORR) d = __fadd_rn(d, c);
  const float b = first ? d : __fadd_rn(__fmul_rn(buf, mu), d);    // buf.mul_(mu).add_(d)        (two roundings)
  buf = b;
  return fmaf(-lr, b, p);                                          // param.add_(buf, alpha=-lr)  (fmadd in torch)
}

// vector i / element i of a drift stream (anchor, corr): read-only, re-read every step of the round.  FEDFR_DRIFT_LD_ONCE selects the
// non-temporal load (multi_state.h: ld_once); which of the two is kept and why: DESIGN.md section 3.30
#ifndef FEDFR_DRIFT_LD_ONCE
#define FEDFR_DRIFT_LD_ONCE 0
#endif
__device__ __forceinline__ float4 drift_ld4(const float* __restrict__ s, size_t i) {
#if FEDFR_DRIFT_LD_ONCE
  const fvec<4> v = ld_once<4>(s, i);
  return make_float4(v.x, v.y, v.z, v.w);
#else
  return reinterpret_cast<const float4*>(s)[i];
#endif
}
__device__ __forceinline__ float drift_ld1(const float* __restrict__ s, size_t i) {
#if FEDFR_DRIFT_LD_ONCE
  return __builtin_nontemporal_load(s + i);
#else
  return s[i];
#endif
}

// UNSCALE: the gradient buffer holds gs^-1 x the gradient (static loss scale of the fp16-storage build); the kernel multiplies by gs
// (a power of two: exact) and stores the true gradient back, so the buffer reads like p.grad afterwards.  Overflow guard (what
// torch.cuda.amp.GradScaler.step does for the reference's fp16 path, client.py:394-396, without its host synchronisation): an element whose
// gradient is not finite is NOT updated (parameter, momentum and mirror keep their values; on the first step its momentum starts at 0) and
// *ovf is set, so one overflowing pass cannot poison the weights; the host reads the word when it next synchronises and lowers the scale.
// ANCHOR / CORR: one more read-only stream each (anchor with its coefficient prox); the guard looks at the gradient alone, whatever they hold.
template <bool UNSCALE, bool ANCHOR, bool CORR>
__global__ __launch_bounds__(256) void sgd_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ buf,
                                                  bf16_t* __restrict__ shadow, size_t n, float lr, float mu, float wd, int first, float gs,
                                                  unsigned* __restrict__ ovf, const float* __restrict__ anchor, float prox,
                                                  const float* __restrict__ corr) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const size_t n4 = n / 4;
  bool bad = false;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    float4 pv = reinterpret_cast<float4*>(p)[i];
    float4 gv = reinterpret_cast<const float4*>(g)[i];
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 xv = ANCHOR ? drift_ld4(anchor, i) : zero;
    const float4 cv = CORR ? drift_ld4(corr, i) : zero;
    if (UNSCALE) {
      gv.x *= gs; gv.y *= gs; gv.z *= gs; gv.w *= gs;
      reinterpret_cast<float4*>(g)[i] = gv;
    }
    float4 bv = first ? make_float4(0.f, 0.f, 0.f, 0.f) : reinterpret_cast<float4*>(buf)[i];
    if (UNSCALE) {
      const float4 p0 = pv, b0 = bv;
      pv.x = sgd_one<ANCHOR, CORR>(pv.x, gv.x, bv.x, lr, mu, wd, first, prox, xv.x, cv.x);
      pv.y = sgd_one<ANCHOR, CORR>(pv.y, gv.y, bv.y, lr, mu, wd, first, prox, xv.y, cv.y);
      pv.z = sgd_one<ANCHOR, CORR>(pv.z, gv.z, bv.z, lr, mu, wd, first, prox, xv.z, cv.z);
      pv.w = sgd_one<ANCHOR, CORR>(pv.w, gv.w, bv.w, lr, mu, wd, first, prox, xv.w, cv.w);
      if (!isfinite(gv.x)) { pv.x = p0.x; bv.x = b0.x; bad = true; }
      if (!isfinite(gv.y)) { pv.y = p0.y; bv.y = b0.y; bad = true; }
      if (!isfinite(gv.z)) { pv.z = p0.z; bv.z = b0.z; bad = true; }
      if (!isfinite(gv.w)) { pv.w = p0.w; bv.w = b0.w; bad = true; }
    } else {
      pv.x = sgd_one<ANCHOR, CORR>(pv.x, gv.x, bv.x, lr, mu, wd, first, prox, xv.x, cv.x);
      pv.y = sgd_one<ANCHOR, CORR>(pv.y, gv.y, bv.y, lr, mu, wd, first, prox, xv.y, cv.y);
      pv.z = sgd_one<ANCHOR, CORR>(pv.z, gv.z, bv.z, lr, mu, wd, first, prox, xv.z, cv.z);
      pv.w = sgd_one<ANCHOR, CORR>(pv.w, gv.w, bv.w, lr, mu, wd, first, prox, xv.w, cv.w);
    }
    reinterpret_cast<float4*>(p)[i] = pv;
    reinterpret_cast<float4*>(buf)[i] = bv;
    if (shadow) {
      uint2 o;
      o.x = pack_bf2(pv.x, pv.y);
      o.y = pack_bf2(pv.z, pv.w);
      reinterpret_cast<uint2*>(shadow)[i] = o;
    }
  }
  for (size_t i = n4 * 4 + (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    float b = first ? 0.f : buf[i];
    float gi = g[i];
    if (UNSCALE) { gi *= gs; g[i] = gi; }
    const float p0 = p[i], b0 = b;
    float v = sgd_one<ANCHOR, CORR>(p0, gi, b, lr, mu, wd, first, prox, ANCHOR ? drift_ld1(anchor, i) : 0.f, CORR ? drift_ld1(corr, i) : 0.f);
    if (UNSCALE && !isfinite(gi)) { v = p0; b = b0; bad = true; }
    p[i] = v;
    buf[i] = b;
    if (shadow) shadow[i] = f2bf(v);
  }
  if (UNSCALE && bad && ovf) *ovf = 1u;          // (every writer stores the same value)
}

// THE route to each of the eight instantiations: (guarded, anchor, corr) -> sgd_kernel<...>.  anchor / corr null: today's two kernels
int optim_sgd(float* p, float* g, float* buf, bf16_t* shadow, size_t n, float lr, float mu, float wd, int first,
              hipStream_t st, float gscale, unsigned* overflow, const float* anchor, float prox, const float* corr) {
  FEDFR_REQUIRE(p && g && buf && n > 0, "sgd: bad args");
  FEDFR_REQUIRE((((uintptr_t)p | (uintptr_t)g | (uintptr_t)buf) & 15) == 0, "sgd: buffers must be 16-byte aligned");
  FEDFR_REQUIRE((((uintptr_t)anchor | (uintptr_t)corr) & 15) == 0, "sgd: anchor / corr must be 16-byte aligned");
  FEDFR_REQUIRE(anchor ? (prox != 0.f && prox - prox == 0.f) : prox == 0.f, "sgd: the proximal coefficient (%g) and the anchor go together", (double)prox);
  const size_t work = n / 4 + 1;
  const int grid = (int)((work + 255) / 256 > 4096 ? 4096 : (work + 255) / 256);
  const bool unscale = gscale != 1.f || overflow != nullptr;
  ProfScope prof(26, (double)n * (first ? 16.0 : 20.0) + (shadow ? 2.0 * n : 0.0) + (unscale ? 4.0 * n : 0.0) + (anchor ? 4.0 * n : 0.0) +
                         (corr ? 4.0 * n : 0.0), st);      // p, g (, buf, anchor, corr) read; p, buf (, bf16 mirror, unscaled g) written
  dispatch_int<0, 7>((unscale ? 1 : 0) | (anchor ? 2 : 0) | (corr ? 4 : 0), [&](auto kc) {
    constexpr int V = decltype(kc)::value;
    constexpr bool U = (V & 1) != 0;
    hipLaunchKernelGGL((sgd_kernel<U, (V & 2) != 0, (V & 4) != 0>), dim3(grid), dim3(256), 0, st, p, g, buf, shadow, n, lr, mu, wd, first,
                       U ? gscale : 1.f, U ? overflow : (unsigned*)nullptr, anchor, prox, corr);
  });
  FEDFR_LAUNCH_CHECK("sgd");
  return FEDFR_OK;
}

// SCAFFOLD's end-of-round pass (option II of Karimireddy et al.): with x the round's global parameters, y the client's trained ones, corr the
// c - c_i it trained with (null: +0.0) and inv_mass = fl32(1 / step_mass),
//   t = fsub(x, y);  cn = fma(inv_mass, t, -corr);  dc = fsub(cn, c_i);  c_i = cn
// one pass, one rounding per operation, on the streaming skeleton of multi_state.h (x, y, corr are read once)
template <bool CORR>
__global__ __launch_bounds__(MULTI_STATE_BLOCK) void scaffold_control_kernel(float* __restrict__ ci, float* __restrict__ dc, const float* __restrict__ x,
                                                                            const float* __restrict__ y, const float* __restrict__ corr,
                                                                            float inv_mass, size_t n) {
  for_each_vec_then_tail<4>(n, [&](auto width, size_t i) {
    constexpr int W = decltype(width)::value;
    const fvec<W> xv = ld_once<W>(x, i), yv = ld_once<W>(y, i);
    fvec<W> cv = vec_at<W>(ci, i), dv;
    fvec<W> rv;
    if constexpr (CORR) rv = ld_once<W>(corr, i);
#pragma unroll
    for (int c = 0; c < W; ++c) {
      float r = 0.f;
      if constexpr (CORR) r = rv[c];
      const float cn = fmaf(inv_mass, __fsub_rn(xv[c], yv[c]), -r);
      dv[c] = __fsub_rn(cn, cv[c]);
      cv[c] = cn;
    }
    vec_at<W>(ci, i) = cv;
    vec_at<W>(dc, i) = dv;
  });
}
int optim_scaffold_control(float* ci, float* dc, const float* x, const float* y, const float* corr, float inv_mass, size_t n, hipStream_t st) {
  FEDFR_REQUIRE(ci && dc && x && y && n > 0, "scaffold_control: bad args");
  FEDFR_REQUIRE(ci != dc, "scaffold_control: c_i and dc must be two buffers");
  FEDFR_REQUIRE((((uintptr_t)ci | (uintptr_t)dc | (uintptr_t)x | (uintptr_t)y | (uintptr_t)corr) & 15) == 0, "scaffold_control: buffers must be 16-byte aligned");
  FEDFR_REQUIRE(inv_mass > 0.f && inv_mass - inv_mass == 0.f, "scaffold_control: inv_mass must be a positive finite number (got %g)", (double)inv_mass);
  if (corr) hipLaunchKernelGGL(scaffold_control_kernel<true>, dim3(multi_state_grid(n)), dim3(MULTI_STATE_BLOCK), 0, st, ci, dc, x, y, corr, inv_mass, n);
  else hipLaunchKernelGGL(scaffold_control_kernel<false>, dim3(multi_state_grid(n)), dim3(MULTI_STATE_BLOCK), 0, st, ci, dc, x, y, corr, inv_mass, n);
  FEDFR_LAUNCH_CHECK("scaffold_control");
  return FEDFR_OK;
}

// ---------------------------------------------------------------------------------------------------------
// FedAvg: dst = (accumulate ? dst : 0) + w * src, fp32, explicit op order (server.py:27-33: tmp += w_i * m_i)
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void fedavg_axpy_kernel(float* __restrict__ dst, const float* __restrict__ src, float w,
                                                          size_t n, int accumulate) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const size_t n4 = n / 4;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    const float4 s = reinterpret_cast<const float4*>(src)[i];
    float4 d = accumulate ? reinterpret_cast<float4*>(dst)[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    d.x = __fadd_rn(d.x, __fmul_rn(w, s.x));
    d.y = __fadd_rn(d.y, __fmul_rn(w, s.y));
    d.z = __fadd_rn(d.z, __fmul_rn(w, s.z));
    d.w = __fadd_rn(d.w, __fmul_rn(w, s.w));
    reinterpret_cast<float4*>(dst)[i] = d;
  }
  for (size_t i = n4 * 4 + (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const float d = accumulate ? dst[i] : 0.f;
    dst[i] = __fadd_rn(d, __fmul_rn(w, src[i]));
  }
}
int optim_fedavg_axpy(float* dst, const float* src, float w, size_t n, int accumulate, hipStream_t st) {
  FEDFR_REQUIRE(dst && src && n > 0, "fedavg_axpy: bad args");
  FEDFR_REQUIRE((((uintptr_t)dst | (uintptr_t)src) & 15) == 0, "fedavg_axpy: buffers must be 16-byte aligned");
  const size_t work = n / 4 + 1;
  const int grid = (int)((work + 255) / 256 > 4096 ? 4096 : (work + 255) / 256);
  hipLaunchKernelGGL(fedavg_axpy_kernel, dim3(grid), dim3(256), 0, st, dst, src, w, n, accumulate);
  FEDFR_LAUNCH_CHECK("fedavg_axpy");
  return FEDFR_OK;
}

// FedAvg over up to 8 client states in ONE pass: dst = (accumulate ? dst : 0) + w_0 * src_0 + w_1 * src_1 + ... in ascending client order with
// the same two roundings per term as fedavg_axpy_kernel, so the result is bit-identical to k sequential axpy launches (server.py:27-33) while
// every state is read once and the aggregate is written once: (k + 1) x n x 4 B instead of (3k - 1) x n x 4 B.
struct StateWeights {      // the weights of up to 8 states as one kernel argument
  float w[8];
};
// Two explicit loops on float4, not for_each_vec_then_tail / fvec<4>: this kernel is the yardstick of all the others, and only this form
// compiles to the instruction stream it has always had (either other form reschedules the vector loop; the callable cost 2 % at k = 8).
template <int K>
__global__ __launch_bounds__(MULTI_STATE_BLOCK) void fedavg_multi_kernel(float* __restrict__ dst, StatePtrs<8> p, StateWeights wt, size_t n, int accumulate) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const size_t n4 = n / 4;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    float4 s[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const fvec<4> v = ld_once<4>(p.src[k], i);
      s[k] = make_float4(v.x, v.y, v.z, v.w);
    }
    float4 d = accumulate ? reinterpret_cast<float4*>(dst)[i] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int k = 0; k < K; ++k) {
      d.x = __fadd_rn(d.x, __fmul_rn(wt.w[k], s[k].x));
      d.y = __fadd_rn(d.y, __fmul_rn(wt.w[k], s[k].y));
      d.z = __fadd_rn(d.z, __fmul_rn(wt.w[k], s[k].z));
      d.w = __fadd_rn(d.w, __fmul_rn(wt.w[k], s[k].w));
    }
    reinterpret_cast<float4*>(dst)[i] = d;
  }
  for (size_t i = n4 * 4 + (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    float d = accumulate ? dst[i] : 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) d = __fadd_rn(d, __fmul_rn(wt.w[k], p.src[k][i]));
    dst[i] = d;
  }
}
int optim_fedavg_multi(float* dst, const float* const* srcs, const float* ws, int k, size_t n, int accumulate, hipStream_t st) {
  FEDFR_REQUIRE(dst && srcs && ws && n > 0 && k >= 1 && k <= 8, "fedavg_multi: bad args (k=%d)", k);
  StatePtrs<8> p{};
  StateWeights wt{};
  uintptr_t al = (uintptr_t)dst;
  FEDFR_TRY(state_ptrs_fill(p, srcs, k, "fedavg_multi", "source", al));
  for (int i = 0; i < k; ++i) wt.w[i] = ws[i];
  FEDFR_REQUIRE((al & 15) == 0, "fedavg_multi: buffers must be 16-byte aligned");
  dispatch_int<1, 8>(k, [&](auto kc) {
    hipLaunchKernelGGL(fedavg_multi_kernel<decltype(kc)::value>, dim3(multi_state_grid(n)), dim3(MULTI_STATE_BLOCK), 0, st, dst, p, wt, n, accumulate);
  });
  FEDFR_LAUNCH_CHECK("fedavg_multi");
  return FEDFR_OK;
}

// int64 counters (num_batches_tracked): acc_f32 (+)= w * float(src) ; optional final truncation back to int64
__global__ void fedavg_i64_kernel(float* acc, const long long* src, float w, int n, int accumulate, long long* out_trunc) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float d = accumulate ? acc[i] : 0.f;
  const float v = __fadd_rn(d, __fmul_rn(w, (float)src[i]));
  acc[i] = v;
  if (out_trunc) out_trunc[i] = (long long)v;
}
int optim_fedavg_i64(float* acc, const long long* src, float w, int n, int accumulate, long long* out_trunc, hipStream_t st) {
  FEDFR_REQUIRE(acc && src && n > 0, "fedavg_i64: bad args");
  hipLaunchKernelGGL(fedavg_i64_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, st, acc, src, w, n, accumulate, out_trunc);
  FEDFR_LAUNCH_CHECK("fedavg_i64");
  return FEDFR_OK;
}

// ---------------------------------------------------------------------------------------------------------
// Server optimisers (Reddi et al., "Adaptive Federated Optimization"): FedAvgM / FedAdagrad / FedAdam / FedYogi on the flat parameter
// buffer, with a per-client update-norm clip.  Two streaming passes on the skeleton fedavg_multi_kernel uses (multi_state.h):
//   fedopt_sqnorm_kernel<K>       sq_i = sum_j (x_i[j] - x[j])^2 per client (fp32 subtract, fp64 square and sum; no atomics: one fp64
//                                 partial per client and block, added in ascending block order by fedopt_sqnorm_final_kernel, which also forms
//                                 coef_i = w_i min(1, clip / sqrt(sq_i)) on the device: no host synchronisation between the two passes)
//   fedopt_multi_kernel<K, KIND>  Delta = sum_i coef_i (x_i - x) (ascending i: subtract, multiply, add = three roundings per client), then the
//                                 moment and parameter update of KIND: the shell of fedopt_pass (fedopt_step.h) without noise; dp.hip's
//                                 dp_multi_kernel is the shell with it.  Every fp32 operation is an explicit single-rounding intrinsic (the build
//                                 contracts a*b+c otherwise), so tests/fedopt_cases.py restates the pass operation by operation.
// The square root is __builtin_sqrtf, not __fsqrt_rn: this toolchain's __fsqrt_rn is the bare v_sqrt_f32 (1 ulp), while hipcc's default
// (-fhip-fp32-correctly-rounded-divide-sqrt) expands __builtin_sqrtf and the division behind __fdiv_rn to correctly rounded sequences.
// ---------------------------------------------------------------------------------------------------------
// (the kinds, FedoptHyper, the per-element step, the pass body and the host's argument check: fedopt_step.h, shared with dp.hip)

template <int K>
__global__ __launch_bounds__(MULTI_STATE_BLOCK) void fedopt_sqnorm_kernel(const float* __restrict__ x, StatePtrs<8> p, size_t n, double* __restrict__ part) {
  __shared__ double red[4][8];
  double acc[K];
#pragma unroll
  for (int k = 0; k < K; ++k) acc[k] = 0.0;
  for_each_vec_then_tail<4>(n, [&](auto width, size_t i) {
    constexpr int W = decltype(width)::value;
    fvec<W> s[K];
#pragma unroll
    for (int k = 0; k < K; ++k) s[k] = ld_once<W>(p.src[k], i);
    const fvec<W> xv = ld_once<W>(x, i);
#pragma unroll
    for (int k = 0; k < K; ++k) {
#pragma unroll
      for (int c = 0; c < W; ++c) {
        // the square of an fp32 value is exact in fp64 (48 bits): fma(d, d, acc) == acc + d * d with ONE rounding either way
        const double d = (double)__fsub_rn(s[k][c], xv[c]);
        acc[k] = __fma_rn(d, d, acc[k]);
      }
    }
  });
  // lanes, waves: block_partial_d; blocks: fedopt_sqnorm_final_kernel, ascending block.  All three orders are fixed
  block_partial_d<K>(acc, red, part, [](int k) { return k; });
}
// one block, wave i owns client i: its `grid` partials are added in ascending block order (ordered_partial_sum), coef_i is formed in fp64 and
// rounded to fp32 once.
__global__ __launch_bounds__(512) void fedopt_sqnorm_final_kernel(const double* __restrict__ part, int grid, int k, StateWeights wt, float clip,
                                                                  double* __restrict__ sq, float* __restrict__ coef) {
  const int i = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (i >= k) return;
  const double s = ordered_partial_sum(part + (size_t)i * grid, grid, lane);
  if (lane != 0) return;
  sq[i] = s;
  double c = (double)wt.w[i];
  if (clip > 0.f && s > 0.0) {
    const double r = (double)clip / sqrt(s);
    c = c * (r < 1.0 ? r : 1.0);
  }
  coef[i] = (float)c;
}
// THE launch of that kernel, for every squared-norm pass of the library (optim.h)
int optim_fedopt_sqnorm_final(const double* part, int grid, int k, const float* ws, float clip, double* sq, float* coef, hipStream_t st) {
  StateWeights wt{};
  for (int i = 0; i < k; ++i) wt.w[i] = ws[i];
  hipLaunchKernelGGL(fedopt_sqnorm_final_kernel, dim3(1), dim3(512), 0, st, part, grid, k, wt, clip, sq, coef);
  FEDFR_LAUNCH_CHECK("fedopt_sqnorm_final");
  return FEDFR_OK;
}
size_t optim_fedopt_sqnorm_ws_bytes(int k, size_t n) {
  if (k < 1 || k > 8 || n == 0) return 0;
  return (size_t)k * multi_state_grid(n) * sizeof(double);
}
int optim_fedopt_sqnorm(const float* x, const float* const* xs, const float* ws, int k, size_t n, float clip, double* sq, float* coef,
                        void* wsp, size_t ws_bytes, hipStream_t st) {
  FEDFR_REQUIRE(x && xs && ws && sq && coef && wsp && n > 0 && k >= 1 && k <= 8, "fedopt_sqnorm: bad args (k=%d)", k);
  FEDFR_REQUIRE(clip == clip, "fedopt_sqnorm: clip is NaN");
  StatePtrs<8> p{};
  uintptr_t al = (uintptr_t)x;
  FEDFR_TRY(state_ptrs_fill(p, xs, k, "fedopt_sqnorm", "client state", al));
  FEDFR_REQUIRE((al & 15) == 0, "fedopt_sqnorm: parameter buffers must be 16-byte aligned");
  FEDFR_REQUIRE((((uintptr_t)sq | (uintptr_t)wsp) & 7) == 0 && ((uintptr_t)coef & 3) == 0, "fedopt_sqnorm: sq / workspace must be 8-byte, coef 4-byte aligned");
  const int grid = multi_state_grid(n);
  if (ws_bytes < (size_t)k * grid * sizeof(double)) {
    fedfr_set_error("fedopt_sqnorm: workspace of %zu bytes, %zu needed", ws_bytes, (size_t)k * grid * sizeof(double));
    return FEDFR_ERR_WORKSPACE;
  }
  double* part = reinterpret_cast<double*>(wsp);
  dispatch_int<1, 8>(k, [&](auto kc) {
    hipLaunchKernelGGL(fedopt_sqnorm_kernel<decltype(kc)::value>, dim3(grid), dim3(MULTI_STATE_BLOCK), 0, st, x, p, n, part);
  });
  FEDFR_LAUNCH_CHECK("fedopt_sqnorm");
  return optim_fedopt_sqnorm_final(part, grid, k, ws, clip, sq, coef, st);
}

// the pass without noise: fedopt_pass (fedopt_step.h; first / last / scratch and the aliasing rules: see there)
template <int K, int KIND>
__global__ __launch_bounds__(MULTI_STATE_BLOCK) void fedopt_multi_kernel(float* xo, const float* x, StatePtrs<8> p, const float* __restrict__ coef, float* __restrict__ m,
                                                           float* __restrict__ v, float* scratch, size_t n, int first, int last,
                                                           FedoptHyper h) {
  fedopt_pass<K, KIND, false>(xo, x, p, coef, m, v, scratch, n, first, last, h, 0.f, DpStream{}, (size_t)blockIdx.x * blockDim.x + threadIdx.x,
                              (size_t)gridDim.x * blockDim.x);
}
int optim_fedopt_multi(int kind, float* x_out, const float* x, const float* const* xs, const float* coef, int k, size_t n, float* m, float* v,
                       float* scratch, int first, int last, float lr, float beta1, float one_minus_beta1, float beta2, float one_minus_beta2,
                       float tau, hipStream_t st) {
  FedoptPassArgs a;
  FEDFR_TRY(fedopt_pass_args("fedopt_multi", FEDOPT_YOGI, a, kind, x_out, x, xs, coef, k, n, m, v, scratch, first, last, lr, beta1, one_minus_beta1, beta2,
                             one_minus_beta2, tau));
  dispatch_int<FEDOPT_AVGM, FEDOPT_YOGI>(kind, [&](auto kindc) {
    dispatch_int<1, 8>(k, [&](auto kc) {
      hipLaunchKernelGGL((fedopt_multi_kernel<decltype(kc)::value, decltype(kindc)::value>), dim3(multi_state_grid(n)), dim3(MULTI_STATE_BLOCK), 0, st, x_out, x, a.p,
                         coef, m, v, scratch, n, a.first, a.last, a.h);
    });
  });
  FEDFR_LAUNCH_CHECK("fedopt_multi");
  return FEDFR_OK;
}

// ---------------------------------------------------------------------------------------------------------
// PartialFC sampling
// ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned hash_u32(unsigned long long x) {   // splitmix64 finaliser
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  x ^= x >> 31;
  return (unsigned)(x >> 32);
}
__global__ void pfc_rand_kernel(float* perm, int n, unsigned long long seed, unsigned long long step) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) perm[i] = (float)(hash_u32(seed * 0x100000001B3ull + step * 0x9E3779B1ull + (unsigned long long)i * 0xD6E8FEB86659FD93ull) >> 8) * (1.0f / 16777216.0f);
}
int optim_pfc_rand(float* perm, int n, unsigned long long seed, unsigned long long step, hipStream_t st) {
  FEDFR_REQUIRE(perm && n > 0, "pfc_rand: bad args");
  hipLaunchKernelGGL(pfc_rand_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, st, perm, n, seed, step);
  FEDFR_LAUNCH_CHECK("pfc_rand");
  return FEDFR_OK;
}

// labels -> local ids (or -1); perm[local] = 2.0 for positives (partial_fc.py:91-98)
__global__ void pfc_localize_kernel(long long* label, int n, long long class_start, int num_local, float* perm) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const long long l = label[i] - class_start;
  if (l >= 0 && l < num_local) {
    label[i] = l;
    if (perm) perm[l] = 2.0f;
  } else {
    label[i] = -1;
  }
}
int optim_pfc_localize(long long* label, int n, long long class_start, int num_local, float* perm, hipStream_t st) {
  FEDFR_REQUIRE(label && n > 0 && num_local > 0, "pfc_localize: bad args");
  hipLaunchKernelGGL(pfc_localize_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, st, label, n, class_start, num_local, perm);
  FEDFR_LAUNCH_CHECK("pfc_localize");
  return FEDFR_OK;
}

// Top-k of non-negative floats as an index set in ascending index order == sort(topk(perm,k).indices).
// One 1024-thread block: 3-pass radix select (11+11+10 bits) for the k-th largest value, then ordered compaction.
__device__ __forceinline__ int block_excl_scan_1024(int v, int* sh, int& total) {
  // sh: 17 ints.  returns exclusive prefix of v over the block; total = block sum
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int x = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int y = __shfl_up(x, o, 64);
    if (lane >= o) x += y;
  }
  if (lane == 63) sh[w] = x;
  __syncthreads();
  if (threadIdx.x == 0) {
    int run = 0;
    for (int i = 0; i < 16; ++i) {
      const int t = sh[i];
      sh[i] = run;
      run += t;
    }
    sh[16] = run;
  }
  __syncthreads();
  const int res = sh[w] + x - v;
  total = sh[16];
  __syncthreads();
  return res;
}

// The digit of the kk-th largest candidate: the highest bin whose count, added to the counts of the bins above it, reaches kk (bin 0 if none
// does).  Block-parallel (1024 threads, nb = 1024 or 2048 bins, descending bin order through one block scan): a single thread walking up to 2 048
// LDS words in a dependent chain was ~70 us per pass at n = 85 000 (round 5 trace).  Ends with a barrier; *s_prefix / *s_k are then visible.
__device__ __forceinline__ void pfc_select_bin(const int* hist, int nb, int kk, unsigned prefix, int shift, int* sh, unsigned* s_prefix, int* s_k) {
  const int per = nb >> 10;                              // bins per thread (1 or 2), thread t owns bins nb - 1 - per t ... downwards
  const int top = nb - 1 - per * (int)threadIdx.x;
  int mine = 0;
  for (int q = 0; q < per; ++q) mine += hist[top - q];
  int total;
  int above = block_excl_scan_1024(mine, sh, total);     // candidates in the bins above this thread's
  for (int q = 0; q < per; ++q) {
    const int bin = top - q, h = hist[bin];
    if (above < kk && (above + h >= kk || bin == 0)) {
      *s_prefix = prefix | ((unsigned)bin << shift);
      *s_k = kk - above;
    }
    above += h;
  }
  __syncthreads();
}

__global__ __launch_bounds__(1024) void pfc_topk_kernel(const float* __restrict__ perm, int n, int k, long long* __restrict__ index,
                                                        int* __restrict__ npos_out) {
  __shared__ int hist[2048];
  __shared__ int sh[17];
  __shared__ unsigned s_prefix;
  __shared__ int s_k;
  const unsigned* bits = reinterpret_cast<const unsigned*>(perm);
  const int tid = threadIdx.x;
  unsigned prefix = 0;     // selected high bits so far
  int kk = k;              // how many still to take from the current candidate set
  const int shifts[3] = {21, 10, 0};
  const int widths[3] = {11, 11, 10};
  unsigned mask_hi = 0;    // mask of bits already fixed
  for (int pass = 0; pass < 3; ++pass) {
    const int nb = 1 << widths[pass];
    for (int i = tid; i < nb; i += 1024) hist[i] = 0;
    __syncthreads();
    for (int i = tid; i < n; i += 1024) {
      const unsigned b = bits[i];
      if ((b & mask_hi) == prefix) atomicAdd(&hist[(b >> shifts[pass]) & (nb - 1)], 1);
    }
    __syncthreads();
    pfc_select_bin(hist, nb, kk, prefix, shifts[pass], sh, &s_prefix, &s_k);
    prefix = s_prefix;
    kk = s_k;
    mask_hi |= (unsigned)(nb - 1) << shifts[pass];
    __syncthreads();
  }
  // prefix == bit pattern T of the k-th largest value; take all > T and the first kk of == T (index order)
  const unsigned T = prefix;
  int base = 0, eq_taken = 0, npos = 0;
  for (int c0 = 0; c0 < n; c0 += 1024) {
    const int i = c0 + tid;
    const unsigned b = i < n ? bits[i] : 0u;
    const int gt = (i < n && b > T) ? 1 : 0;
    const int eq = (i < n && b == T) ? 1 : 0;
    int tot_eq, tot_sel;
    const int eq_rank = block_excl_scan_1024(eq, sh, tot_eq);
    const int sel = gt | (eq && (eq_taken + eq_rank) < kk ? 1 : 0);
    const int pos = block_excl_scan_1024(sel, sh, tot_sel);
    if (sel) index[base + pos] = i;
    if (i < n && b == 0x40000000u) ++npos;     // 2.0f marks a positive class
    base += tot_sel;
    eq_taken += tot_eq;
  }
  if (npos_out) {
    int tot;
    (void)block_excl_scan_1024(npos, sh, tot);
    if (tid == 0) *npos_out = tot;
  }
}
// The same selection with WIDE, prefetched loads (round 5).  The kernel above walks the n values four times (three histogram passes + the
// compaction) with ONE dependent 4-byte global load per thread and iteration: at n = 85 000 that is 4 x 83 L2 round trips = 319 us of the 930 us
// PartialFC head (profiles/r05_pfc_head_trace_v1.txt).  Here a thread owns NPT CONSECUTIVE values of every chunk of 1024 NPT (fetched as 16-byte
// loads, the next chunk's in flight while this one is counted), so a pass is n / (1024 NPT) round trips and the ordered compaction needs one
// pair of block scans per chunk instead of one per 1024 values: same radix select, same index set.  The histogram is kept in NCOPY copies
// (lane l adds to copy l % NCOPY, rows padded to 2049 words so that the copies of a bin sit in different banks): the values are uniform draws,
// so half of them share ONE 11-bit digit in the first pass, and 64 lanes adding to one LDS word are served one after the other (the
// single-copy form of this kernel: 256 us).
template <int NPT, int NCOPY>
__global__ __launch_bounds__(1024) void pfc_topk_wide_kernel(const float* __restrict__ perm, int n, int k, long long* __restrict__ index,
                                                             int* __restrict__ npos_out) {
  extern __shared__ int hcopies[];                      // [NCOPY][2049]
  __shared__ int hist[2048];
  __shared__ int sh[17];
  int* const myhist = hcopies + (threadIdx.x % NCOPY) * 2049;
  __shared__ unsigned s_prefix;
  __shared__ int s_k;
  static_assert(NPT % 4 == 0, "16-byte loads");
  const int tid = threadIdx.x;
  constexpr int CH = 1024 * NPT;
  const int nch = (n + CH - 1) / CH;
  auto load = [&](int c, unsigned (&v)[NPT]) {            // values [c CH + tid NPT, + NPT); beyond n: 0 with ok() false
#pragma unroll
    for (int j = 0; j < NPT / 4; ++j) {
      const int i = c * CH + tid * NPT + 4 * j;
      uint4 q = make_uint4(0u, 0u, 0u, 0u);
      if (i + 3 < n) q = *reinterpret_cast<const uint4*>(perm + i);
      else {
        const unsigned* b = reinterpret_cast<const unsigned*>(perm);
        if (i < n) q.x = b[i];
        if (i + 1 < n) q.y = b[i + 1];
        if (i + 2 < n) q.z = b[i + 2];
      }
      v[4 * j] = q.x; v[4 * j + 1] = q.y; v[4 * j + 2] = q.z; v[4 * j + 3] = q.w;
    }
  };
  unsigned prefix = 0, mask_hi = 0;
  int kk = k;
  const int shifts[3] = {21, 10, 0};
  const int widths[3] = {11, 11, 10};
  unsigned cur[NPT], nxt[NPT];
  for (int pass = 0; pass < 3; ++pass) {
    const int nb = 1 << widths[pass];
    for (int i = tid; i < NCOPY * 2049; i += 1024) hcopies[i] = 0;
    load(0, cur);
    __syncthreads();
    for (int c = 0; c < nch; ++c) {
      if (c + 1 < nch) load(c + 1, nxt);
      const int nv = n - (c * CH + tid * NPT);
#pragma unroll
      for (int j = 0; j < NPT; ++j)
        if (j < nv && (cur[j] & mask_hi) == prefix) atomicAdd(&myhist[(cur[j] >> shifts[pass]) & (nb - 1)], 1);
#pragma unroll
      for (int j = 0; j < NPT; ++j) cur[j] = nxt[j];
    }
    __syncthreads();
    for (int i = tid; i < nb; i += 1024) {              // the copies of a bin, summed
      int t = 0;
#pragma unroll
      for (int q = 0; q < NCOPY; ++q) t += hcopies[q * 2049 + i];
      hist[i] = t;
    }
    __syncthreads();
    pfc_select_bin(hist, nb, kk, prefix, shifts[pass], sh, &s_prefix, &s_k);
    prefix = s_prefix;
    kk = s_k;
    mask_hi |= (unsigned)(nb - 1) << shifts[pass];
    __syncthreads();
  }
  // prefix == bit pattern T of the k-th largest value; take all > T and the first kk of == T (index order)
  const unsigned T = prefix;
  int base = 0, eq_taken = 0, npos = 0;
  load(0, cur);
  for (int c = 0; c < nch; ++c) {
    if (c + 1 < nch) load(c + 1, nxt);
    const int i0 = c * CH + tid * NPT, nv = n - i0;
    int n_gt = 0, n_eq = 0;
#pragma unroll
    for (int j = 0; j < NPT; ++j) {
      n_gt += (j < nv && cur[j] > T) ? 1 : 0;
      n_eq += (j < nv && cur[j] == T) ? 1 : 0;
      npos += (j < nv && cur[j] == 0x40000000u) ? 1 : 0;     // 2.0f marks a positive class
    }
    int tot_eq, tot_gt;
    int eq_before = eq_taken + block_excl_scan_1024(n_eq, sh, tot_eq);
    const int gt_before = block_excl_scan_1024(n_gt, sh, tot_gt);
    // selected elements in front of this thread: `base` from earlier chunks (their > T and taken == T), this chunk's predecessors' > T, and of
    // all == T in front of it the first kk — minus those already counted in `base`
    int pos = base + gt_before + (min(eq_before, kk) - min(eq_taken, kk));
#pragma unroll
    for (int j = 0; j < NPT; ++j) {
      const bool gt = j < nv && cur[j] > T, eq = j < nv && cur[j] == T;
      if (gt || (eq && eq_before < kk)) index[pos++] = i0 + j;
      eq_before += eq ? 1 : 0;
    }
    base += tot_gt + (min(eq_taken + tot_eq, kk) - min(eq_taken, kk));
    eq_taken += tot_eq;
#pragma unroll
    for (int j = 0; j < NPT; ++j) cur[j] = nxt[j];
  }
  if (npos_out) {
    int tot;
    (void)block_excl_scan_1024(npos, sh, tot);
    if (tid == 0) *npos_out = tot;
  }
}
int optim_pfc_topk(const float* perm, int n, int k, long long* index, int* npos_out, hipStream_t st) {
  FEDFR_REQUIRE(perm && index && n > 0 && k > 0 && k <= n, "pfc_topk: bad args (k=%d n=%d)", k, n);
  if ((reinterpret_cast<size_t>(perm) & 15) == 0 && n >= 8192) {
    constexpr int NCOPY = 16;
    constexpr size_t lds = (size_t)NCOPY * 2049 * sizeof(int);
    static PerDeviceOnce attr_once;     // hipFuncSetAttribute is per device
    attr_once.run([&] {
      hipFuncSetAttribute(reinterpret_cast<const void*>(&pfc_topk_wide_kernel<16, NCOPY>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    });
    hipLaunchKernelGGL((pfc_topk_wide_kernel<16, NCOPY>), dim3(1), dim3(1024), lds, st, perm, n, k, index, npos_out);
  } else hipLaunchKernelGGL(pfc_topk_kernel, dim3(1), dim3(1024), 0, st, perm, n, k, index, npos_out);      // (small or unaligned shards: the 4-byte form)
  FEDFR_LAUNCH_CHECK("pfc_topk");
  return FEDFR_OK;
}

// positives only (num_sample < #positives branch, partial_fc.py:101-102): ordered compaction of perm == 2.0
__global__ __launch_bounds__(1024) void pfc_positive_kernel(const float* __restrict__ perm, int n, long long* __restrict__ index,
                                                            int* __restrict__ count) {
  __shared__ int sh[17];
  int base = 0;
  for (int c0 = 0; c0 < n; c0 += 1024) {
    const int i = c0 + threadIdx.x;
    const int sel = (i < n && perm[i] == 2.0f) ? 1 : 0;
    int tot;
    const int pos = block_excl_scan_1024(sel, sh, tot);
    if (sel) index[base + pos] = i;
    base += tot;
  }
  if (threadIdx.x == 0) *count = base;
}
int optim_pfc_positive(const float* perm, int n, long long* index, int* count, hipStream_t st) {
  FEDFR_REQUIRE(perm && index && count && n > 0, "pfc_positive: bad args");
  hipLaunchKernelGGL(pfc_positive_kernel, dim3(1), dim3(1024), 0, st, perm, n, index, count);
  FEDFR_LAUNCH_CHECK("pfc_positive");
  return FEDFR_OK;
}

// label[i] = searchsorted(index, label[i]) for label != -1 (partial_fc.py:104)
__global__ void pfc_remap_kernel(long long* label, int n, const long long* __restrict__ index, int k) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const long long l = label[i];
  if (l < 0) return;
  int lo = 0, hi = k;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (index[mid] < l) lo = mid + 1; else hi = mid;
  }
  label[i] = lo;
}
int optim_pfc_remap(long long* label, int n, const long long* index, int k, hipStream_t st) {
  FEDFR_REQUIRE(label && index && n > 0 && k > 0, "pfc_remap: bad args");
  hipLaunchKernelGGL(pfc_remap_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, st, label, n, index, k);
  FEDFR_LAUNCH_CHECK("pfc_remap");
  return FEDFR_OK;
}

// row gather / scatter (fp32 rows of D floats, D % 4 == 0), one wave per row
__global__ __launch_bounds__(256) void rows_kernel(float* __restrict__ dst, const float* __restrict__ src,
                                                   const long long* __restrict__ index, int k, int D, int scatter, int nrows) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= k) return;
  const long long r = index[row];
  if (r < 0 || r >= nrows) return;                     // never touch memory outside the indexed table
  const float4* s = reinterpret_cast<const float4*>(src + (scatter ? (size_t)row : (size_t)r) * D);
  float4* d = reinterpret_cast<float4*>(dst + (scatter ? (size_t)r : (size_t)row) * D);
  for (int i = lane; i < D / 4; i += 64) d[i] = s[i];
}
int optim_rows(float* dst, const float* src, const long long* index, int k, int D, int scatter, int nrows, hipStream_t st) {
  FEDFR_REQUIRE(dst && src && index && k > 0 && D > 0 && (D & 3) == 0 && nrows > 0, "rows gather/scatter: bad args");
  hipLaunchKernelGGL(rows_kernel, dim3(ceil_div(k, 4)), dim3(256), 0, st, dst, src, index, k, D, scatter, nrows);
  FEDFR_LAUNCH_CHECK("rows");
  return FEDFR_OK;
}
