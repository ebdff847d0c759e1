// LFW-style k-fold 1:1 verification (reference eval/verification.py: test :262-281, evaluate, calculate_roc, calculate_val): everything
// between the embeddings and the accuracy bookkeeping in ONE pass over the two embedding sets.
//
// verif_pair_kernel<float | double>: one wave per pair p (rows 2p and 2p + 1), 16-byte loads, all arithmetic fp64:
//   s = (double)emb0[r] + (double)emb1[r] (emb1 NULL: no flip test), divided by sqrt(sum s^2) as sklearn.preprocessing.normalize does (a
//   zero row stays zero; normalize = 0: rows taken as they are, calculate_roc's own contract), dist = sum (a - b)^2.  For each ascending
//   threshold table: k0 = #{k : thr[k] <= dist}, so np.less(dist, thr[k]) holds exactly for k >= k0; k0 starts from a guess (dist scaled
//   by the table's span) and is walked against the table itself until thr[k0 - 1] <= dist < thr[k0], so the result is a property of the
//   table alone.  A NaN dist lands in bin T (never accepted) and sets status bit 1.  The fp64 L2 norms of the raw rows of both sets are
//   summed on the way (xnorm).
// Folds are the contiguous ranges of KFold(n_splits, shuffle=False); a workgroup serves pairs of ONE fold, so its histogram
// [2][Ta + 1] + [2][Tb + 1] of 32-bit counters lives in LDS and only its non-zero bins reach memory, by integer global atomics (order-free).
// The norm sums go wave -> workgroup -> workspace slot; verif_norm_reduce_kernel adds the slots in a fixed order: no float atomics,
// two launches give the same bits.
#include <cfloat>
#include "head.h"

namespace {

constexpr int kMaxD = 1024;
constexpr int kJ = kMaxD / 256;          // float4 pieces of a row per lane
constexpr int kMaxBins = 16000;          // 2 (Ta + 1) + 2 (Tb + 1) 32-bit counters: at most 64 000 bytes of dynamic LDS
constexpr int kChunk = 32;               // pairs of one workgroup (8 per wave) while the grid stays under kMaxWgs
constexpr int kMaxWgs = 4096;

struct FoldGrid {
  int chunk, wpf;                        // pairs per workgroup, workgroups per fold
};

FoldGrid fold_grid(int P, int nfolds) {
  const int longest = ceil_div(P, nfolds);
  FoldGrid g;
  g.chunk = std::max(kChunk, ceil_div(longest, std::max(1, kMaxWgs / nfolds)));
  g.wpf = ceil_div(longest, g.chunk);
  return g;
}

// k0 = #{k : thr[k] <= d} of an ascending table (d not NaN)
__device__ __forceinline__ int first_above(const double* __restrict__ thr, int T, double d) {
  const double lo = thr[0], span = thr[T - 1] - lo;
  double g = span > 0.0 ? (d - lo) / span * (double)(T - 1) : 0.0;
  g = g < 0.0 ? 0.0 : g > (double)T ? (double)T : g;
  int k = (int)g;
  while (k < T && thr[k] <= d) ++k;
  while (k > 0 && thr[k - 1] > d) --k;
  return k;
}

// four consecutive elements of a row as doubles, by 16-byte loads
__device__ __forceinline__ void load4(const float* p, double* v) {
  const float4 x = *reinterpret_cast<const float4*>(p);
  v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
}
__device__ __forceinline__ void load4(const double* p, double* v) {
  const double2 x = *reinterpret_cast<const double2*>(p), y = *reinterpret_cast<const double2*>(p + 2);
  v[0] = x.x; v[1] = x.y; v[2] = y.x; v[3] = y.y;
}

template <typename T>
__global__ __launch_bounds__(256) void verif_pair_kernel(const T* __restrict__ emb0, const T* __restrict__ emb1, int normalize,
                                                         const unsigned char* __restrict__ issame, int P, int D, int nfolds, int chunk,
                                                         int wpf, const double* __restrict__ thr_a, int Ta, const double* __restrict__ thr_b,
                                                         int Tb, unsigned long long* __restrict__ counts_a,
                                                         unsigned long long* __restrict__ counts_b, double* __restrict__ dist_out,
                                                         double* __restrict__ part_norm, int* __restrict__ status) {
  extern __shared__ unsigned hist[];     // [2][Ta + 1] then [2][Tb + 1]
  __shared__ double sNorm[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int na = 2 * (Ta + 1), nb = thr_b ? 2 * (Tb + 1) : 0;
  for (int i = tid; i < na + nb; i += 256) hist[i] = 0u;
  __syncthreads();

  const int fold = blockIdx.x / wpf, part = blockIdx.x % wpf;
  const int q = P / nfolds, r = P % nfolds;
  const int f0 = fold * q + min(fold, r), f1 = f0 + q + (fold < r ? 1 : 0);      // KFold(shuffle=False): the first P % nfolds folds are longer
  const int p0 = f0 + part * chunk, p1 = min(p0 + chunk, f1);

  double norm_sum = 0.0;
  for (int p = p0 + wave; p < p1; p += 4) {
    double s[2][kJ][4];
    double ss[2] = {0.0, 0.0}, raw0 = 0.0, raw1 = 0.0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const size_t row = (size_t)(2 * p + h) * D;
#pragma unroll
      for (int j = 0; j < kJ; ++j) {
        const int d = 4 * (lane + 64 * j);             // D % 4 == 0: a piece is inside the row or past its end as a whole
        double xv[4] = {0.0, 0.0, 0.0, 0.0}, yv[4] = {0.0, 0.0, 0.0, 0.0};
        if (d < D) {
          load4(emb0 + row + d, xv);
          if (emb1) load4(emb1 + row + d, yv);
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const double v = xv[t] + yv[t];
          s[h][j][t] = v;
          ss[h] += v * v;
          raw0 += xv[t] * xv[t];
          raw1 += yv[t] * yv[t];
        }
      }
      raw0 = wave_sum_d(raw0);
      raw1 = wave_sum_d(raw1);
      norm_sum += sqrt(raw0);
      if (emb1) norm_sum += sqrt(raw1);
      raw0 = raw1 = 0.0;
      ss[h] = sqrt(wave_sum_d(ss[h]));
      if (!normalize || ss[h] < 10.0 * DBL_EPSILON) ss[h] = 1.0;   // sklearn normalize (_handle_zeros_in_scale): a zero row stays zero
    }
    double dd = 0.0;
#pragma unroll
    for (int j = 0; j < kJ; ++j)
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const double e = s[0][j][t] / ss[0] - s[1][j][t] / ss[1];
        dd += e * e;
      }
    dd = wave_sum_d(dd);
    if (lane == 0) {
      if (dist_out) dist_out[p] = dd;
      const int same = issame[p] ? 1 : 0;
      const bool bad = dd != dd;
      if (bad) atomicOr(status, 1);
      atomicAdd(&hist[same * (Ta + 1) + (bad ? Ta : first_above(thr_a, Ta, dd))], 1u);
      if (thr_b) atomicAdd(&hist[na + same * (Tb + 1) + (bad ? Tb : first_above(thr_b, Tb, dd))], 1u);
    }
  }
  if (lane == 0) sNorm[wave] = norm_sum;               // every lane holds the same sum (xor butterfly)
  __syncthreads();
  if (tid == 0) part_norm[blockIdx.x] = ((sNorm[0] + sNorm[1]) + sNorm[2]) + sNorm[3];
  for (int i = tid; i < na + nb; i += 256) {
    const unsigned c = hist[i];
    if (!c) continue;
    if (i < na) atomicAdd(&counts_a[(size_t)fold * na + i], (unsigned long long)c);
    else atomicAdd(&counts_b[(size_t)fold * nb + (i - na)], (unsigned long long)c);
  }
}

__global__ __launch_bounds__(256) void verif_norm_reduce_kernel(const double* __restrict__ part_norm, int n, double* __restrict__ norm_sum) {
  __shared__ double sN[256];
  const int tid = threadIdx.x;
  double v = 0.0;
  for (int i = tid; i < n; i += 256) v += part_norm[i];
  sN[tid] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) sN[tid] += sN[tid + s];
    __syncthreads();
  }
  if (tid == 0) *norm_sum = sN[0];
}

}  // namespace

size_t verif_workspace_bytes(int P, int nfolds) {
  if (P < 1 || nfolds < 1 || nfolds > P) return 0;
  return (size_t)nfolds * fold_grid(P, nfolds).wpf * sizeof(double);
}

int verif_fold_counts(const void* emb0, const void* emb1, int fp64_input, int normalize, const unsigned char* issame, int P, int D,
                      int nfolds, const double* thr_a, int Ta, const double* thr_b, int Tb, unsigned long long* counts_a,
                      unsigned long long* counts_b, double* dist, double* norm_sum, int* status, void* ws, size_t ws_bytes, hipStream_t st) {
  FEDFR_REQUIRE(emb0 && issame && thr_a && counts_a && norm_sum && status,
                "verif_fold_counts: null pointer (emb0, issame, thr_a, counts_a, norm_sum and status are required)");
  FEDFR_REQUIRE(!thr_b || counts_b, "verif_fold_counts: null pointer (a second threshold table needs counts_b)");
  FEDFR_REQUIRE((fp64_input == 0 || fp64_input == 1) && (normalize == 0 || normalize == 1),
                "verif_fold_counts: fp64_input = %d and normalize = %d must be 0 or 1", fp64_input, normalize);
  FEDFR_REQUIRE(P >= 1, "verif_fold_counts: P = %d must be >= 1", P);
  FEDFR_REQUIRE(D >= 4 && D <= kMaxD && D % 4 == 0, "verif_fold_counts: D = %d must be a multiple of 4 in [4, %d]", D, kMaxD);
  FEDFR_REQUIRE(nfolds >= 1 && nfolds <= P, "verif_fold_counts: nfolds = %d must be in [1, P = %d]", nfolds, P);
  FEDFR_REQUIRE(Ta >= 1 && (!thr_b || Tb >= 1), "verif_fold_counts: threshold tables must not be empty (Ta = %d, Tb = %d)", Ta, Tb);
  const long long bins = 2ll * (Ta + 1) + (thr_b ? 2ll * (Tb + 1) : 0ll);
  FEDFR_REQUIRE(bins <= kMaxBins, "verif_fold_counts: Ta = %d, Tb = %d need %lld counters per workgroup (limit %d)", Ta, thr_b ? Tb : 0, bins,
                kMaxBins);
  FEDFR_REQUIRE(((uintptr_t)emb0 | (uintptr_t)emb1) % 16 == 0, "verif_fold_counts: the embeddings must be 16-byte aligned");
  const size_t need = verif_workspace_bytes(P, nfolds);
  if (!ws || ws_bytes < need) {
    fedfr_set_error("verif_fold_counts: workspace of %zu bytes, %zu needed", ws ? ws_bytes : (size_t)0, need);
    return FEDFR_ERR_WORKSPACE;
  }
  const FoldGrid g = fold_grid(P, nfolds);
  const int nwg = nfolds * g.wpf;
  if (hipMemsetAsync(counts_a, 0, (size_t)nfolds * 2 * (Ta + 1) * sizeof(unsigned long long), st) != hipSuccess ||
      (thr_b && hipMemsetAsync(counts_b, 0, (size_t)nfolds * 2 * (Tb + 1) * sizeof(unsigned long long), st) != hipSuccess)) {
    fedfr_set_error("verif_fold_counts: hipMemsetAsync of the count tables failed");
    return FEDFR_ERR_HIP;
  }
  const size_t lds = (size_t)bins * sizeof(unsigned);
  if (fp64_input)
    hipLaunchKernelGGL(verif_pair_kernel<double>, dim3(nwg), dim3(256), lds, st, static_cast<const double*>(emb0),
                       static_cast<const double*>(emb1), normalize, issame, P, D, nfolds, g.chunk, g.wpf, thr_a, Ta, thr_b, Tb, counts_a,
                       counts_b, dist, static_cast<double*>(ws), status);
  else
    hipLaunchKernelGGL(verif_pair_kernel<float>, dim3(nwg), dim3(256), lds, st, static_cast<const float*>(emb0),
                       static_cast<const float*>(emb1), normalize, issame, P, D, nfolds, g.chunk, g.wpf, thr_a, Ta, thr_b, Tb, counts_a,
                       counts_b, dist, static_cast<double*>(ws), status);
  FEDFR_LAUNCH_CHECK("verif_pair");
  hipLaunchKernelGGL(verif_norm_reduce_kernel, dim3(1), dim3(256), 0, st, static_cast<const double*>(ws), nwg, norm_sum);
  FEDFR_LAUNCH_CHECK("verif_norm_reduce");
  return FEDFR_OK;
}
