// The per-element step of the server optimisers, shared by optim.hip (fedopt_multi_kernel) and dp.hip (dp_multi_kernel): one definition, so
// that the two kernels round alike (tests/fedopt_cases.py restates it operation by operation).
#pragma once
#include "common.h"

// FEDOPT_PLAIN is dp.hip's alone (x' = x + Delta, no moments: DP-FedAvg); fedopt_one does not know it
enum { FEDOPT_AVGM = 0, FEDOPT_ADAGRAD = 1, FEDOPT_ADAM = 2, FEDOPT_YOGI = 3, FEDOPT_PLAIN = 4 };
struct FedoptHyper {
  float lr, b1, omb1, b2, omb2, tau;      // omb1 = 1 - beta1, omb2 = 1 - beta2: formed by the host in fp32
};

template <int KIND>
__device__ __forceinline__ void fedopt_one(float d, float x, float& m, float& v, float& xo, const FedoptHyper& h) {
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
