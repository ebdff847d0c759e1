// The BatchNorm algebra, written once: every kernel that derives coefficients from statistics or applies them per element (the finalize kernels and
// row-slab passes of bn_rowslab.hip, the channel-sliced passes of bn_sliced.hip, the fused stem weight gradient of stem.hip) calls these helpers, so
// fused and unfused passes agree bit for bit because they run the same expressions, not copies of them (tests/test_kernels_gpu.py:
// test_sliced_and_finalize_coefficients_agree_bitwise, tests/test_stem_chain_gpu.py; tests/test_bn_sliced_gpu.py holds every sliced pass to the fp64
// value of these expressions on the partial rows it is given, tests/bn_sliced_cases.py restates them).  The library is built with -ffp-contract=on: which products fuse
// into an FMA is decided per source expression, so the statement structure and operand order below ARE the arithmetic.
#pragma once
#include "common.h"

// 1 / sqrt(v) in fp64 (v > 0): the hardware estimate + two Newton steps.  `1.0 / sqrt(v)` is a square-root and a divide sequence — ~70 dependent
// fp64 operations — on the critical path of EVERY BatchNorm pass (each workgroup derives its coefficients itself, bn_sliced.hip), and so were the
// divisions by the pixel count: the helpers take its reciprocal `ic`, which the sliced passes form while their loads are in flight.
__device__ __forceinline__ double bn_rsqrt(double v) {
  double y = __builtin_amdgcn_rsq(v);
  y = y * (1.5 - 0.5 * v * y * y);
  y = y * (1.5 - 0.5 * v * y * y);
  return y;
}

// ---- forward: statistics -> coefficients ------------------------------------------------------------------------------------------
struct BnFwdCoef {
  double mean, var, rstd;     // batch statistics (biased variance, clamped at 0)
  float scale, shift;         // y = x scale + shift
};
__device__ __forceinline__ BnFwdCoef bn_fwd_coef(double sum, double sumsq, double ic, float eps, float gamma, float beta) {
  BnFwdCoef k;
  k.mean = sum * ic;
  double var = sumsq * ic - k.mean * k.mean;
  if (var < 0.0) var = 0.0;
  k.var = var;
  k.rstd = bn_rsqrt(var + (double)eps);
  k.scale = (float)((double)gamma * k.rstd);
  k.shift = (float)((double)beta - k.mean * (double)gamma * k.rstd);
  return k;
}
// running statistics (torch semantics: the running variance takes the unbiased batch variance); rm0 / rv0 = their values before the step
__device__ __forceinline__ void bn_running_update(const BnFwdCoef& k, double count, float momentum, float rm0, float rv0, float* rm, float* rv) {
  const double unb = count > 1.0 ? k.var * count / (count - 1.0) : k.var;
  *rm = (float)((1.0 - momentum) * (double)rm0 + momentum * k.mean);
  *rv = (float)((1.0 - momentum) * (double)rv0 + momentum * unb);
}

// ---- backward: sums -> coefficients ------------------------------------------------------------------------------------------------
// dx = a dz + A x + B  (== a (dz - mean(dz) - xhat mean(dz xhat)), xhat = (x - mean) rstd), from t1 = sum dz and t2 = sum dz xhat:
//   a = gamma rstd, A = -a rstd mean(dz xhat), B = a (rstd mean mean(dz xhat) - mean(dz))
struct BnBwdCoef {
  float a, A, B;
};
// (gamma, rstd, mean arrive as the fp32 values they are stored as: the compiler then forms a, the fp32-rounded product, with one fp32 multiply)
__device__ __forceinline__ BnBwdCoef bn_bwd_coef(double t1, double t2, double ic, float gamma, float rstd, float mean) {
  const double g = (double)gamma, r = (double)rstd, mu = (double)mean;
  const double a = (double)(float)(g * r), cb = t1 * ic, cc = t2 * ic;
  BnBwdCoef k;
  k.a = (float)a;
  k.A = (float)(-a * cc * r);
  k.B = (float)(a * (cc * r * mu - cb));
  return k;
}

// ---- backward: per element ----------------------------------------------------------------------------------------------------------
// PReLU pre-activation z = G x + H with the forward's (scale, shift): the same expression as the forward pass, so the mask is the forward's
__device__ __forceinline__ float bn_preact(float x, float G, float H) { return x * G + H; }
// gradient wrt the pre-activation of a PReLU with slope alpha
__device__ __forceinline__ float bn_masked_dz(float dy, float z, float alpha) {
  float dz = dy;
  if (z <= 0.f) dz = dy * alpha;
  return dz;
}
__device__ __forceinline__ float bn_dx(float a, float dz, float A, float x, float B) { return a * dz + (A * x + B); }
// dx of one element of a BatchNorm (+ PReLU when ALPHA; G, H, alpha are not read otherwise) from its coefficients
template <bool ALPHA>
__device__ __forceinline__ float bn_bwd_dx(float dy, float x, const float& G, const float& H, const float& alpha, float a, float A, float B) {
  float dz = dy;
  if (ALPHA) dz = bn_masked_dz(dy, bn_preact(x, G, H), alpha);
  return bn_dx(a, dz, A, x, B);
}
// masked dz of a PReLU, and the element's share of the slope's gradient: s_dyz += dy z over z <= 0
__device__ __forceinline__ float bn_prelu_dz(float dy, float z, float alpha, float& s_dyz) {
  if (z <= 0.f) s_dyz += dy * z;
  return bn_masked_dz(dy, z, alpha);
}
// one element's share of the two sums every BatchNorm backward needs: s_dz += dz, s_dzx += dz (x - mean) (scaled by rstd once, at the end = sum dz xhat)
__device__ __forceinline__ void bn_bwd_sums(float dz, float x, float mean, float& s_dz, float& s_dzx) {
  s_dz += dz;
  s_dzx += dz * (x - mean);
}
// ... of a BatchNorm followed by a PReLU when ALPHA: three sums (G, H, alpha, s_dyz are not touched otherwise)
template <bool ALPHA>
__device__ __forceinline__ void bn_bwd_sums(float dy, float x, float mean, const float& G, const float& H, const float& alpha, float& s_dz, float& s_dzx, float& s_dyz) {
  float dz = dy;
  if (ALPHA) dz = bn_prelu_dz(dy, bn_preact(x, G, H), alpha, s_dyz);
  bn_bwd_sums(dz, x, mean, s_dz, s_dzx);
}
