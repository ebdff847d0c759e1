// Reweighted aggregation over k flat fp32 client states: the geometric median (RFA, the smoothed Weiszfeld iteration of Pillutla, Kakade and
// Harchaoui, 2019) and centred clipping (Karimireddy, He and Jaggi, 2021).  Both are "weights from the distances to the current centre, one
// weighted step, repeat": R iterations are R + 1 HBM-bound streaming passes on the skeleton of multi_state.h with a single-block kernel in
// between, back to back on one stream.
//   reweight_step_kernel<K, V, WRITE>   one pass over the k states and the centre: the new centre AND the k squared distances to it (fp64)
//   reweight_weights_kernel             the blocks' partials in ascending order, then the next weights from the distances, one block
//
// ARITHMETIC CONTRACT (include/fedfr_hip.h states it for the callers; tests/reweight_cases.py restates it in numpy and the kernels are held
// to it: z' and beta bit for bit, D within the fp64 summation bound).  x_0 .. x_{k-1} the states, z the centre, beta k fp32 weights in
// device memory.  Per element, every operation a single correctly rounded fp32 operation (__fsub_rn / __fmul_rn / __fadd_rn: the build
// contracts a * b + c otherwise):
//   delta_i = x_i - z
//   acc = z;  for i ascending:  beta_i != 0 ?  acc = acc + beta_i * delta_i  :  acc       (a SELECT: a skipped client's NaN / inf never reaches acc)
//   z' = acc                                                                            (WRITE == false: z' = z, beta is not read, nothing is stored)
//   e_i = x_i - z'   for every client, the skipped ones included
//   D_i = fma((double) e_i, (double) e_i, D_i)      (the square of an fp32 value is exact in fp64: one rounding per term)
// The x_i stay in registers between the two halves (as the keys do in robust_trimmed_mean_kernel): every state is read ONCE per pass.  D_i:
// lanes by the shuffle tree, waves in ascending order (block_partial_d), one partial per client and block in the workspace [k][grid]; the blocks
// are added in ascending order by reweight_weights_kernel (ordered_partial_sum).  No atomics: two runs give the same bits.
// z' may be written over z: a thread reads the elements it owns before it writes them and nobody else touches them.
// WEIGHTS, fp64, each beta rounded to fp32 once; d_i = sqrt(D_i); a client whose D_i is not finite gets 0; alpha_i the prior weights:
//   geometric median:  w_i = alpha_i / max(nu, d_i);  S = w_0 + ... + w_{k-1} ascending;  beta_i = (float) (w_i / S)
//   centred clipping:  beta_i = (float) (alpha_i * min(1, tau / d_i)), d_i == 0 -> alpha_i;  tau given, or the lower median of the finite d_i of
//                      the round's first (distance-only) pass, kept in info[0] for the rest of the round
#include "reweight.h"
#include "multi_state.h"
#include "../../include/fedfr_hip.h"

// ---------------------------------------------------------------------------------------------------------
// the step pass.  V floats per lane and load: 4 for K <= 16 (64 state registers at K = 16), 2 for K = 17 .. 32 (64 at K = 32), beside 2 K
// registers of fp64 accumulators.  dst and z may be the same buffer: neither is __restrict__.
// ---------------------------------------------------------------------------------------------------------
template <int K, int V, bool WRITE>
__global__ __launch_bounds__(MULTI_STATE_BLOCK) void reweight_step_kernel(float* dst, const float* z, StatePtrs<K> p, const float* __restrict__ beta,
                                                                          size_t n, double* __restrict__ part) {
  __shared__ double red[4][K];
  double acc[K];
  float b[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    acc[k] = 0.0;
    b[k] = WRITE ? beta[k] : 0.f;      // (uniform: scalar loads)
  }
  for_each_vec_then_tail<V>(n, [&](auto width, size_t i) {
    constexpr int W = decltype(width)::value;
    fvec<W> x[K];
#pragma unroll
    for (int k = 0; k < K; ++k) x[k] = ld_once<W>(p.src[k], i);      // all K loads in flight
    const fvec<W> zv = vec_at<W>(z, i);
    fvec<W> zn = zv;
    if constexpr (WRITE) {
#pragma unroll
      for (int c = 0; c < W; ++c) {
        float a = zv[c];
#pragma unroll
        for (int k = 0; k < K; ++k) {
          const float t = __fadd_rn(a, __fmul_rn(b[k], __fsub_rn(x[k][c], zv[c])));
          a = b[k] != 0.f ? t : a;
        }
        zn[c] = a;
      }
      vec_at<W>(dst, i) = zn;
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
#pragma unroll
      for (int c = 0; c < W; ++c) {
        const double e = (double)__fsub_rn(x[k][c], zn[c]);
        acc[k] = __fma_rn(e, e, acc[k]);
      }
    }
  });
  block_partial_d<K>(acc, red, part, [](int k) { return k; });
}

size_t reweight_ws_bytes(int k, size_t n) {
  if (k < 1 || k > 32 || n == 0) return 0;
  return (size_t)k * multi_state_grid(n) * sizeof(double);
}

// the workspace both calls share: [k][grid] doubles, 8-byte aligned
static int reweight_check_ws(const char* who, const void* wsp, size_t ws_bytes, int k, size_t n) {
  FEDFR_REQUIRE(((uintptr_t)wsp & 7) == 0, "%s: workspace must be 8-byte aligned", who);
  const size_t need = reweight_ws_bytes(k, n);
  if (ws_bytes < need) {
    fedfr_set_error("%s: workspace of %zu bytes, %zu needed", who, ws_bytes, need);
    return FEDFR_ERR_WORKSPACE;
  }
  return FEDFR_OK;
}

int reweight_step(float* dst, const float* z, const float* const* xs, const float* beta, int k, size_t n, void* wsp, size_t ws_bytes, hipStream_t st) {
  FEDFR_REQUIRE(z && xs && wsp && n > 0, "reweight_step: bad args");
  FEDFR_REQUIRE(k >= 1 && k <= 32, "reweight_step: k must be 1..32 (k=%d)", k);
  FEDFR_REQUIRE(!dst || beta, "reweight_step: a step that writes the centre needs beta");
  StatePtrs<32> all{};
  uintptr_t al = (uintptr_t)dst | (uintptr_t)z;
  FEDFR_TRY(state_ptrs_fill(all, xs, k, "reweight_step", "client state", al));
  FEDFR_REQUIRE((al & 15) == 0, "reweight_step: dst, z and the client states must be 16-byte aligned");
  FEDFR_REQUIRE(((uintptr_t)beta & 3) == 0, "reweight_step: beta must be 4-byte aligned");
  if (dst) {
    FEDFR_REQUIRE(dst == z || z + n <= dst || dst + n <= z, "reweight_step: dst overlaps z (in place means dst == z)");
    for (int i = 0; i < k; ++i) FEDFR_REQUIRE(xs[i] + n <= dst || dst + n <= xs[i], "reweight_step: dst overlaps client state %d", i);
  }
  FEDFR_TRY(reweight_check_ws("reweight_step", wsp, ws_bytes, k, n));
  double* part = reinterpret_cast<double*>(wsp);
  dispatch_int<1, 32>(k, [&](auto kc) {
    constexpr int K = decltype(kc)::value;
    constexpr int V = K <= 16 ? 4 : 2;
    StatePtrs<K> p;      // CAP = K: the kernel argument is no larger than the states it names
    for (int i = 0; i < K; ++i) p.src[i] = all.src[i];
    if (dst) hipLaunchKernelGGL((reweight_step_kernel<K, V, true>), dim3(multi_state_grid(n)), dim3(MULTI_STATE_BLOCK), 0, st, dst, z, p, beta, n, part);
    else hipLaunchKernelGGL((reweight_step_kernel<K, V, false>), dim3(multi_state_grid(n)), dim3(MULTI_STATE_BLOCK), 0, st, dst, z, p, beta, n, part);
  });
  FEDFR_LAUNCH_CHECK("reweight_step");
  return FEDFR_OK;
}

// ---------------------------------------------------------------------------------------------------------
// the weights: one block of 16 waves, wave w adds the partials of clients w and w + 16 in ascending block order (ordered_partial_sum); then
// thread 0 forms the k weights serially (k <= 32: a few hundred fp64 operations).  Everything indexed at run time lives in LDS.
// ---------------------------------------------------------------------------------------------------------
struct ReweightAlpha {      // the prior weights of up to 32 clients as one kernel argument
  double a[32];
};
__global__ __launch_bounds__(1024) void reweight_weights_kernel(const double* __restrict__ part, int grid, int k, ReweightAlpha al, int rule, double param,
                                                                int slot, int iters, double* __restrict__ hist_d, float* __restrict__ hist_beta,
                                                                double* __restrict__ info) {
  __shared__ double D[32], A[32], dd[32], wv[32];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int i = w; i < k; i += 16) {      // (uniform per wave)
    const double s = ordered_partial_sum(part + (size_t)i * grid, grid, lane);
    if (lane == 0) D[i] = s;
  }
  if (threadIdx.x < 32) {
    double a = 0.0;
#pragma unroll
    for (int j = 0; j < 32; ++j) a = (int)threadIdx.x == j ? al.a[j] : a;      // (constant indices into the kernel argument)
    A[threadIdx.x] = a;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  const double inf = __longlong_as_double(0x7FF0000000000000ll);
  unsigned fin = 0u;
  int nf = 0;
  for (int i = 0; i < k; ++i) {
    const double v = D[i];
    hist_d[(size_t)slot * k + i] = v;
    const bool ok = isfinite(v);
    dd[i] = ok ? sqrt(v) : inf;
    fin |= ok ? 1u << i : 0u;
    nf += ok ? 1 : 0;
  }
  double tau = param, S = 0.0;
  if (rule == FEDFR_REWEIGHT_CCLIP) {
    if (param == 0.0) {      // auto: the lower median of the first pass's finite distances, kept for the round
      if (slot == 0) {
        const int target = (nf - 1) / 2;
        for (int i = 0; i < k; ++i) {
          if (!((fin >> i) & 1u)) continue;
          int rank = 0;
          for (int j = 0; j < k; ++j) rank += ((fin >> j) & 1u) && (dd[j] < dd[i] || (dd[j] == dd[i] && j < i)) ? 1 : 0;
          if (rank == target) tau = dd[i];
        }
      } else {
        tau = info[0];
      }
    }
    info[0] = tau;
    for (int i = 0; i < k; ++i) {
      float bi = 0.f;
      if ((fin >> i) & 1u) {
        const double q = tau / dd[i];
        const double r = dd[i] == 0.0 ? 1.0 : (q < 1.0 ? q : 1.0);
        bi = (float)(A[i] * r);
      }
      S += (double)bi;
      if (slot < iters) hist_beta[(size_t)slot * k + i] = bi;
    }
  } else {
    for (int i = 0; i < k; ++i) {
      const double wi = (fin >> i) & 1u ? A[i] / (dd[i] > param ? dd[i] : param) : 0.0;
      wv[i] = wi;
      S += wi;
    }
    if (slot < iters) {
      for (int i = 0; i < k; ++i) hist_beta[(size_t)slot * k + i] = S > 0.0 ? (float)(wv[i] / S) : 0.f;
    }
  }
  info[1] = S;
  if (slot == 0) info[2] = nf == 0 ? 1.0 : 0.0;
  else if (nf == 0) info[2] = 1.0;
  info[3] = (double)nf;
}

int reweight_weights(int rule, const double* alpha, double param, int slot, int iters, int k, size_t n, const void* wsp, size_t ws_bytes, double* hist_d,
                     float* hist_beta, double* info, hipStream_t st) {
  FEDFR_REQUIRE(alpha && wsp && hist_d && hist_beta && info && n > 0, "reweight_weights: bad args");
  FEDFR_REQUIRE(k >= 1 && k <= 32, "reweight_weights: k must be 1..32 (k=%d)", k);
  FEDFR_REQUIRE(rule == FEDFR_REWEIGHT_GEOMEDIAN || rule == FEDFR_REWEIGHT_CCLIP, "reweight_weights: unknown rule %d", rule);
  FEDFR_REQUIRE(iters >= 1 && slot >= 0 && slot <= iters, "reweight_weights: slot must be 0..iters, iters >= 1 (slot=%d iters=%d)", slot, iters);
  if (rule == FEDFR_REWEIGHT_GEOMEDIAN)
    FEDFR_REQUIRE(param > 0.0 && param - param == 0.0, "reweight_weights: nu must be a positive finite number (got %g)", param);
  else
    FEDFR_REQUIRE(param >= 0.0 && param - param == 0.0, "reweight_weights: tau must be a positive finite number or 0 for auto (got %g)", param);
  ReweightAlpha al{};
  for (int i = 0; i < k; ++i) {
    FEDFR_REQUIRE(alpha[i] >= 0.0 && alpha[i] - alpha[i] == 0.0, "reweight_weights: alpha %d must be a finite number >= 0 (got %g)", i, alpha[i]);
    al.a[i] = alpha[i];
  }
  FEDFR_REQUIRE((((uintptr_t)hist_d | (uintptr_t)info) & 7) == 0 && ((uintptr_t)hist_beta & 3) == 0,
                "reweight_weights: hist_d / info must be 8-byte, hist_beta 4-byte aligned");
  FEDFR_TRY(reweight_check_ws("reweight_weights", wsp, ws_bytes, k, n));
  hipLaunchKernelGGL(reweight_weights_kernel, dim3(1), dim3(1024), 0, st, reinterpret_cast<const double*>(wsp), multi_state_grid(n), k, al, rule, param,
                     slot, iters, hist_d, hist_beta, info);
  FEDFR_LAUNCH_CHECK("reweight_weights");
  return FEDFR_OK;
}
