// The delta-step pass of the server optimisers, written ONCE for optim.hip (fedopt_multi_kernel) and dp.hip (dp_multi_kernel): the
// per-element step (fedopt_one), the two loops in which the order of the sum over the clients lives (fedopt_pass), and the host check of the
// arguments the two entry points share (fedopt_pass_args).  The two kernels are __global__ shells around fedopt_pass, so they round alike by
// construction (tests/fedopt_cases.py restates the pass operation by operation).
#pragma once
#include "common.h"
#include "dp.h"            // DpStream, dp_gauss4: the noise of a last pass
#include "multi_state.h"

// FEDOPT_PLAIN (x' = x + Delta, no moments: DP-FedAvg) is reachable through dp_multi alone
enum { FEDOPT_AVGM = 0, FEDOPT_ADAGRAD = 1, FEDOPT_ADAM = 2, FEDOPT_YOGI = 3, FEDOPT_PLAIN = 4 };
struct FedoptHyper {
  float lr, b1, omb1, b2, omb2, tau;      // omb1 = 1 - beta1, omb2 = 1 - beta2: formed by the host in fp32
};

template <int KIND>
__device__ __forceinline__ void fedopt_one(float d, float x, float& m, float& v, float& xo, const FedoptHyper& h) {
  if (KIND == FEDOPT_PLAIN) {
    xo = __fadd_rn(x, d);
    return;
  }
  if (KIND == FEDOPT_AVGM) {
    m = __fadd_rn(__fmul_rn(h.b1, m), d);
    xo = __fadd_rn(x, __fmul_rn(h.lr, m));
    return;
  }
  m = __fadd_rn(__fmul_rn(h.b1, m), __fmul_rn(h.omb1, d));
  const float d2 = __fmul_rn(d, d);
  if (KIND == FEDOPT_ADAGRAD) v = __fadd_rn(v, d2);
  if (KIND == FEDOPT_ADAM) v = __fadd_rn(__fmul_rn(h.b2, v), __fmul_rn(h.omb2, d2));
  if (KIND == FEDOPT_YOGI) {
    const float e = __fsub_rn(v, d2);
    const float sg = e > 0.f ? 1.f : (e < 0.f ? -1.f : 0.f);      // sign(0) = 0
    v = __fsub_rn(v, __fmul_rn(__fmul_rn(h.omb2, d2), sg));
  }
  xo = __fadd_rn(x, __fdiv_rn(__fmul_rn(h.lr, m), __fadd_rn(__builtin_sqrtf(v), h.tau)));
}

// One pass: Delta = (first ? 0 : scratch) + sum_k coef[k] (x_k - x), ascending k, three roundings per client.  Not last: Delta goes to scratch
// and m, v, xo are untouched.  Last: with NOISE and noise_std > 0, Delta += noise_std z (a wave-uniform test, so a pass without noise pays one
// branch and 0 * z is never added); then the step of KIND on m (, v) and xo.  xo may be x; scratch may be a client state on a non-last pass and
// xo on the last one (every thread reads index i of each before it writes index i).  t and stride are the caller's global thread index and
// grid size in threads: a __global__ function knows its block size to be uniform, a __device__ function reads blockDim.x per lane.
// Two explicit loops, not for_each_vec_then_tail: through that callable 23 of the 32 instantiations need 4-11 more VGPRs.
template <int K, int KIND, bool NOISE>
__device__ __forceinline__ void fedopt_pass(float* xo, const float* x, const StatePtrs<8>& p, const float* __restrict__ coef, float* __restrict__ m,
                                            float* __restrict__ v, float* scratch, size_t n, int first, int last, const FedoptHyper& h,
                                            float noise_std, const DpStream& rs, size_t t, size_t stride) {
  constexpr bool HAS_M = KIND != FEDOPT_PLAIN, HAS_V = HAS_M && KIND != FEDOPT_AVGM;
  const size_t n4 = n / 4;
  const bool noisy = NOISE && last && noise_std > 0.f;
  float c[K];
#pragma unroll
  for (int k = 0; k < K; ++k) c[k] = coef[k];
  for (size_t i = t; i < n4; i += stride) {
    fvec<4> s[K];
#pragma unroll
    for (int k = 0; k < K; ++k) s[k] = ld_once<4>(p.src[k], i);
    const float4 xv = reinterpret_cast<const float4*>(x)[i];
    float4 d = first ? make_float4(0.f, 0.f, 0.f, 0.f) : reinterpret_cast<const float4*>(scratch)[i];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      d.x = __fadd_rn(d.x, __fmul_rn(c[k], __fsub_rn(s[k].x, xv.x)));
      d.y = __fadd_rn(d.y, __fmul_rn(c[k], __fsub_rn(s[k].y, xv.y)));
      d.z = __fadd_rn(d.z, __fmul_rn(c[k], __fsub_rn(s[k].z, xv.z)));
      d.w = __fadd_rn(d.w, __fmul_rn(c[k], __fsub_rn(s[k].w, xv.w)));
    }
    if (!last) {
      reinterpret_cast<float4*>(scratch)[i] = d;
      continue;
    }
    if (noisy) {
      const float4 z = dp_gauss4(rs, i);
      d.x = __fadd_rn(d.x, __fmul_rn(noise_std, z.x));
      d.y = __fadd_rn(d.y, __fmul_rn(noise_std, z.y));
      d.z = __fadd_rn(d.z, __fmul_rn(noise_std, z.z));
      d.w = __fadd_rn(d.w, __fmul_rn(noise_std, z.w));
    }
    float4 mv = HAS_M ? reinterpret_cast<const float4*>(m)[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    float4 vv = HAS_V ? reinterpret_cast<const float4*>(v)[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    float4 o;
    fedopt_one<KIND>(d.x, xv.x, mv.x, vv.x, o.x, h);
    fedopt_one<KIND>(d.y, xv.y, mv.y, vv.y, o.y, h);
    fedopt_one<KIND>(d.z, xv.z, mv.z, vv.z, o.z, h);
    fedopt_one<KIND>(d.w, xv.w, mv.w, vv.w, o.w, h);
    if (HAS_M) reinterpret_cast<float4*>(m)[i] = mv;
    if (HAS_V) reinterpret_cast<float4*>(v)[i] = vv;
    reinterpret_cast<float4*>(xo)[i] = o;
  }
  for (size_t i = n4 * 4 + t; i < n; i += stride) {
    const float xv = x[i];
    float d = first ? 0.f : scratch[i];
#pragma unroll
    for (int k = 0; k < K; ++k) d = __fadd_rn(d, __fmul_rn(c[k], __fsub_rn(p.src[k][i], xv)));
    if (!last) {
      scratch[i] = d;
      continue;
    }
    if (noisy) d = __fadd_rn(d, __fmul_rn(noise_std, lane_of(dp_gauss4(rs, n4), (int)(i & 3))));
    float mv = HAS_M ? m[i] : 0.f, vv = HAS_V ? v[i] : 0.f, o;
    fedopt_one<KIND>(d, xv, mv, vv, o, h);
    if (HAS_M) m[i] = mv;
    if (HAS_V) v[i] = vv;
    xo[i] = o;
  }
}

// What a launch of either shell takes beyond the caller's own pointers: the checked client states, the hyper-parameters, first / last as 0 / 1
struct FedoptPassArgs {
  StatePtrs<8> p;
  FedoptHyper h;
  int first, last;
};
// The argument check of the entry point `who` ("fedopt_multi", "dp_multi"), whose kinds are FEDOPT_AVGM .. max_kind; fills `a`.  The last
// pass needs the moments its kind has; m and v must be aligned for every kind but FEDOPT_PLAIN, which reads neither.
static inline int fedopt_pass_args(const char* who, int max_kind, FedoptPassArgs& a, int kind, const float* x_out, const float* x, const float* const* xs,
                                   const float* coef, int k, size_t n, const float* m, const float* v, const float* scratch, int first, int last, float lr,
                                   float beta1, float one_minus_beta1, float beta2, float one_minus_beta2, float tau) {
  FEDFR_REQUIRE(kind >= FEDOPT_AVGM && kind <= max_kind, "%s: unknown optimiser kind %d", who, kind);
  FEDFR_REQUIRE(x && xs && coef && n > 0 && k >= 1 && k <= 8, "%s: bad args (k=%d)", who, k);
  a.first = first ? 1 : 0;
  a.last = last ? 1 : 0;
  const bool has_m = kind != FEDOPT_PLAIN, has_v = has_m && kind != FEDOPT_AVGM;
  FEDFR_REQUIRE((a.first && a.last) || scratch, "%s: a chained pass (first=%d last=%d) needs the scratch buffer", who, a.first, a.last);
  FEDFR_REQUIRE(!a.last || (x_out && (!has_m || m) && (!has_v || v)), "%s: the last pass needs x_out%s%s", who, has_m ? ", m" : "", has_v ? " and v" : "");
  a.p = StatePtrs<8>{};
  uintptr_t al = (uintptr_t)x | (uintptr_t)x_out | (uintptr_t)scratch;      // (null: no bits)
  if (has_m) al |= (uintptr_t)m | (uintptr_t)v;
  FEDFR_TRY(state_ptrs_fill(a.p, xs, k, who, "client state", al));
  FEDFR_REQUIRE((al & 15) == 0, "%s: buffers must be 16-byte aligned", who);
  FEDFR_REQUIRE(((uintptr_t)coef & 3) == 0, "%s: coef must be 4-byte aligned", who);
  a.h = FedoptHyper{lr, beta1, one_minus_beta1, beta2, one_minus_beta2, tau};
  return FEDFR_OK;
}
