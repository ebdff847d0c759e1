// IJB-C template evaluation (reference ijbc_all.py): everything after the forward pass of jobs 1:1 on the GPU.
//
// ijbc_image_norm_kernel     optional (use_norm_score=False, :523-528): fp32 L2 norm of every image row, in numpy's summation order.
// ijbc_template_pool_kernel  image features -> template features (image2template_feature_11/_1n, :225-298), one workgroup per template,
//                            one thread per feature dimension: fp32 sums in the reference's order (media mean, then sum over medias),
//                            then the fp64 normalisation (sklearn normalize for 1:1, the explicit divide for 1:N).
// ijbc_pair_kernel           fp64 dot of two gathered template rows per pair (verification, :300-326) in numpy's pairwise order, fused
//                            with the ROC counts: every score is binary-searched in the sorted distinct genuine scores and counted in an
//                            LDS histogram of 32-bit integers (impostors strictly between two genuine values), plus integer global
//                            atomics for the rare exact ties.  Per-workgroup histograms are written to a workspace slab and summed by
//                            ijbc_count_reduce_kernel: no floating-point atomics, the counts are run-to-run identical.
//
// numpy sums a contiguous row pairwise (loops_utils.h pairwise_sum): n < 8 sequentially from 0; n <= 128 in 8 strided accumulators,
// combined ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then the n % 8 tail in order; larger n split in halves (rounded down to a multiple of 8).
// pw_sum reproduces that for D < 8, D <= 128 and D = 256, 512, 1024 (whole 128-blocks, a balanced tree): one lane per accumulator and
// xor shuffles for the tree.  Products and sums must round separately, so contraction is off in this file.
#include <cfloat>
#include "head.h"

#pragma clang fp contract(off)

namespace {

constexpr int kMaxD = 1024;
constexpr int kMaxGenuine = 40000;    // distinct genuine scores: an LDS histogram of kMaxGenuine + 1 uint32 fits the 160 KB of a workgroup
constexpr int kPairWgs = 512;         // pair-kernel workgroups (2 per CU)

__host__ __device__ inline int pw_lanes(int D) { return D < 8 ? 1 : D <= 128 ? 8 : 8 * (D / 128); }
inline bool pw_supported(int D) { return D >= 1 && (D <= 128 || D == 256 || D == 512 || D == 1024); }

// numpy's pairwise sum of term(0) ... term(D-1), computed by the pw_lanes(D) lanes of an aligned lane group (sub = lane index in the
// group).  Every lane of the wave must call it; every lane of a group returns the group's sum.
template <typename T, typename F>
__device__ __forceinline__ T pw_sum(F term, int D, int sub) {
  if (D < 8) {
    T r = 0;
    for (int i = 0; i < D; ++i) r += term(i);
    return r;
  }
  const int L = pw_lanes(D), bl = D <= 128 ? D : 128, n8 = bl - bl % 8;
  const int base = (sub >> 3) * bl, j = sub & 7;
  T r = term(base + j);
  for (int i = 8; i < n8; i += 8) r += term(base + i + j);
  for (int m = 1; m < L; m <<= 1) r += __shfl_xor(r, m);      // 1, 2, 4: the 8-accumulator tree; 8, 16, 32: the halves of D
  for (int i = n8; i < bl; ++i) r += term(i);                 // the tail (D <= 128 only: one block)
  return r;
}

__global__ __launch_bounds__(256) void ijbc_image_norm_kernel(const float* __restrict__ f, int N, int D, int W, float* __restrict__ norm) {
  const int L = pw_lanes(D), per_wave = 64 / L, lane = threadIdx.x & 63;
  const int sub = lane & (L - 1), slot = lane / L;
  const long long nwaves = (long long)gridDim.x * 4, wave = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  for (long long i0 = wave * per_wave; i0 < N; i0 += nwaves * per_wave) {
    const long long i = i0 + slot, ic = i < N ? i : N - 1;
    const float* r = f + ic * W;
    const float s = pw_sum<float>([&](int d) {
      const float x = W == D ? r[d] : r[d] + r[D + d];
      return x * x;
    }, D, sub);
    if (i < N && sub == 0) norm[i] = sqrtf(s);
  }
}

// status bits: 1 = bad CSR / image index, 2 = pair template id without a row, 4 = genuine score missing from the genuine table,
// 8 = a non-finite score
__global__ __launch_bounds__(256) void ijbc_template_pool_kernel(const float* __restrict__ f, int N, int D, int W, const float* __restrict__ face,
                                                                 const float* __restrict__ inorm, const int* __restrict__ t_off,
                                                                 const int* __restrict__ m_off, const int* __restrict__ img, int M, int NI,
                                                                 int mode, float* __restrict__ raw, double* __restrict__ out,
                                                                 int* __restrict__ status) {
  constexpr int J = kMaxD / 256;
  __shared__ double sv[kMaxD];
  __shared__ double snorm;
  const int t = blockIdx.x, tid = threadIdx.x;
  auto xval = [&](int im, int d) -> float {
    const float* r = f + (size_t)im * W;
    float x = W == D ? r[d] : r[d] + r[D + d];      // F1: the two halves added (:515-521)
    if (inorm) x = x / inorm[im];                   // N1 off: images normalised first (:523-528)
    if (face) x = x * face[im];                     // D1: faceness-weighted (:530-533)
    return x;
  };
  float acc[J];
#pragma unroll
  for (int j = 0; j < J; ++j) acc[j] = 0.f;
  const int mb = t_off[t], me = t_off[t + 1];
  bool ok = 0 <= mb && mb <= me && me <= M;
  for (int m = mb; ok && m < me; ++m) {
    const int ib = m_off[m], ie = m_off[m + 1];
    if (!(0 <= ib && ib < ie && ie <= NI)) {
      ok = false;
      break;
    }
    float ms[J];
    for (int k = ib; k < ie; ++k) {
      const int im = img[k];
      if (im < 0 || im >= N) {
        ok = false;
        break;
      }
#pragma unroll
      for (int j = 0; j < J; ++j) {
        const int d = tid + 256 * j;
        if (d < D) {
          const float x = xval(im, d);
          ms[j] = k == ib ? x : ms[j] + x;          // np.mean(axis=0) on float32: the sum in image order ...
        }
      }
    }
    if (!ok) break;
    const float cnt = (float)(ie - ib);
#pragma unroll
    for (int j = 0; j < J; ++j) {
      if (ie - ib > 1) ms[j] = ms[j] / cnt;         // ... divided once by the count; a single-image media is the image itself
      acc[j] = m == mb ? ms[j] : acc[j] + ms[j];    // np.sum(media_norm_feats, 0): medias in order
    }
  }
  if (!ok && tid == 0) atomicOr(status, 1);
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int d = tid + 256 * j;
    if (d < D) {
      if (!ok) acc[j] = 0.f;
      if (raw) raw[(size_t)t * D + d] = acc[j];
      sv[d] = (double)acc[j];
    }
  }
  __syncthreads();
  if (tid < 64) {
    const double s = pw_sum<double>([&](int d) { return sv[d] * sv[d]; }, D, tid & (pw_lanes(D) - 1));
    if (tid == 0) {
      double n = sqrt(s);
      if (mode == 0 && n < 10.0 * DBL_EPSILON) n = 1.0;   // sklearn normalize: _handle_zeros_in_scale
      snorm = n;
    }
  }
  __syncthreads();
  const double n = snorm;
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int d = tid + 256 * j;
    if (d < D) out[(size_t)t * D + d] = sv[d] / n;
  }
}

// k = number of genuine values above s (gv descending); an impostor equal to gv[k] counts in eq, otherwise in the bin between gv[k-1]
// and gv[k] (k = 0: above all, k = G: below all).  counts layout: [0, G] between-bins, [G+1, 2G] impostors equal, [2G+1, 3G] genuine.
__device__ __forceinline__ void roc_count(double s, bool genuine, const double* __restrict__ gv, int G, unsigned* hist,
                                          unsigned long long* __restrict__ counts, int* __restrict__ status) {
  if (!isfinite(s)) {                               // roc_curve rejects non-finite scores
    atomicOr(status, 8);
    return;
  }
  int lo = 0, hi = G;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (gv[mid] > s) lo = mid + 1;
    else hi = mid;
  }
  const bool eq = lo < G && gv[lo] == s;
  if (genuine) {
    if (eq) atomicAdd(&counts[2 * G + 1 + lo], 1ull);
    else atomicOr(status, 4);
  } else if (eq) {
    atomicAdd(&counts[G + 1 + lo], 1ull);
  } else {
    atomicAdd(&hist[lo], 1u);
  }
}

__device__ __forceinline__ void hist_init(unsigned* hist, int G) {
  for (int i = threadIdx.x; i <= G; i += blockDim.x) hist[i] = 0u;
  __syncthreads();
}

__device__ __forceinline__ void hist_flush(const unsigned* hist, int G, unsigned* __restrict__ slab) {
  __syncthreads();
  for (int i = threadIdx.x; i <= G; i += blockDim.x) slab[(size_t)blockIdx.x * (G + 1) + i] = hist[i];
}

__global__ __launch_bounds__(256) void ijbc_pair_kernel(const double* __restrict__ feat, int T, int D, const int* __restrict__ lut,
                                                        long long lut_n, const long long* __restrict__ p1, const long long* __restrict__ p2,
                                                        long long P, double* __restrict__ score, const long long* __restrict__ label,
                                                        const double* __restrict__ gv, int G, unsigned* __restrict__ slab,
                                                        unsigned long long* __restrict__ counts, int* __restrict__ status) {
  extern __shared__ unsigned hist[];
  if (gv) hist_init(hist, G);
  const int L = pw_lanes(D), per_wave = 64 / L, lane = threadIdx.x & 63;
  const int sub = lane & (L - 1), slot = lane / L;
  const long long nwaves = (long long)gridDim.x * 4, wave = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  for (long long p0 = wave * per_wave; p0 < P; p0 += nwaves * per_wave) {
    const long long p = p0 + slot;
    const bool valid = p < P;
    int r1 = -1, r2 = -1;
    if (valid) {
      const long long a = p1[p], b = p2[p];
      r1 = (a >= 0 && a < lut_n) ? lut[a] : -1;
      r2 = (b >= 0 && b < lut_n) ? lut[b] : -1;
    }
    const bool ok = valid && r1 >= 0 && r1 < T && r2 >= 0 && r2 < T;
    const double* x = feat + (size_t)(ok ? r1 : 0) * D;
    const double* y = feat + (size_t)(ok ? r2 : 0) * D;
    const double s = pw_sum<double>([&](int d) { return x[d] * y[d]; }, D, sub);   // np.sum(feat1 * feat2, -1)
    if (valid && sub == 0) {
      if (ok) {
        if (score) score[p] = s;
        if (gv) roc_count(s, label[p] == 1, gv, G, hist, counts, status);
      } else {
        if (score) score[p] = __longlong_as_double(0x7ff8000000000000ll);
        atomicOr(status, 2);
      }
    }
  }
  if (gv) hist_flush(hist, G, slab);
}

__global__ __launch_bounds__(256) void ijbc_roc_count_kernel(const double* __restrict__ score, const long long* __restrict__ label, long long P,
                                                             const double* __restrict__ gv, int G, unsigned* __restrict__ slab,
                                                             unsigned long long* __restrict__ counts, int* __restrict__ status) {
  extern __shared__ unsigned hist[];
  hist_init(hist, G);
  for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < P; p += (long long)gridDim.x * 256)
    roc_count(score[p], label[p] == 1, gv, G, hist, counts, status);
  hist_flush(hist, G, slab);
}

__global__ __launch_bounds__(256) void ijbc_count_reduce_kernel(const unsigned* __restrict__ slab, int nwg, int G,
                                                                unsigned long long* __restrict__ counts) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i > G) return;
  unsigned long long s = 0ull;
  for (int w = 0; w < nwg; ++w) s += slab[(size_t)w * (G + 1) + i];
  counts[i] += s;
}

int count_wgs(long long P) { return (int)std::max(1LL, std::min<long long>(kPairWgs, (P + 255) / 256)); }   // small P (the genuine pass): many short workgroups

// the histogram may exceed the default 64 KB of dynamic LDS
void allow_big_lds() {
  static PerDeviceOnce attr_once;     // hipFuncSetAttribute is per device
  attr_once.run([&] {
    const int lds = (kMaxGenuine + 1) * (int)sizeof(unsigned);
    hipFuncSetAttribute(reinterpret_cast<const void*>(&ijbc_pair_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    hipFuncSetAttribute(reinterpret_cast<const void*>(&ijbc_roc_count_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  });
}

int roc_finish(unsigned* slab, int nwg, int G, unsigned long long* counts, hipStream_t st) {
  hipLaunchKernelGGL(ijbc_count_reduce_kernel, dim3(ceil_div(G + 1, 256)), dim3(256), 0, st, slab, nwg, G, counts);
  FEDFR_LAUNCH_CHECK("ijbc_count_reduce");
  return FEDFR_OK;
}

}  // namespace

size_t ijbc_template_pool_workspace_bytes(int N, int norm_images) { return norm_images ? align_up((size_t)std::max(N, 1) * sizeof(float), 256) : 0; }

int ijbc_template_pool(const float* feats, int N, int D, int flip, const float* face, int norm_images, const int* t_off, int T,
                       const int* m_off, int M, const int* img, int NI, int mode, float* raw, double* out, void* ws, size_t ws_bytes,
                       int* status, hipStream_t st) {
  FEDFR_REQUIRE(feats && t_off && m_off && img && out && status, "template_pool: null pointer (feats, t_off, m_off, img, out and status are required)");
  FEDFR_REQUIRE(N > 0 && T > 0 && M > 0 && NI > 0, "template_pool: bad sizes (N = %d, T = %d, M = %d, NI = %d)", N, T, M, NI);
  FEDFR_REQUIRE(pw_supported(D) && D <= kMaxD, "template_pool: D = %d unsupported (D <= 128 or D in {256, 512, 1024})", D);
  FEDFR_REQUIRE(mode == 0 || mode == 1, "template_pool: mode = %d must be 0 (sklearn normalize) or 1 (explicit divide)", mode);
  const size_t need = ijbc_template_pool_workspace_bytes(N, norm_images);
  FEDFR_REQUIRE(!norm_images || (ws && ws_bytes >= need), "template_pool: workspace of %zu bytes, %zu needed", ws_bytes, need);
  const int W = flip ? 2 * D : D;
  float* inorm = nullptr;
  if (norm_images) {
    inorm = static_cast<float*>(ws);
    const int L = pw_lanes(D), rows_per_wg = 4 * (64 / L);
    hipLaunchKernelGGL(ijbc_image_norm_kernel, dim3(std::min(ceil_div(N, rows_per_wg), 4096)), dim3(256), 0, st, feats, N, D, W, inorm);
    FEDFR_LAUNCH_CHECK("ijbc_image_norm");
  }
  hipLaunchKernelGGL(ijbc_template_pool_kernel, dim3(T), dim3(256), 0, st, feats, N, D, W, face, inorm, t_off, m_off, img, M, NI, mode, raw,
                     out, status);
  FEDFR_LAUNCH_CHECK("ijbc_template_pool");
  return FEDFR_OK;
}

size_t ijbc_roc_workspace_bytes(long long P, int G) {
  if (P < 1 || G < 1) return 0;
  return (size_t)count_wgs(P) * (G + 1) * sizeof(unsigned);
}

static int roc_args(long long P, const long long* label, const double* gv, int G, unsigned long long* counts, void* ws, size_t ws_bytes,
                    const char* who) {
  FEDFR_REQUIRE(label && gv && counts, "%s: counting needs label, genuine table and counts", who);
  FEDFR_REQUIRE(G >= 1 && G <= kMaxGenuine, "%s: G = %d distinct genuine scores outside [1, %d]", who, G, kMaxGenuine);
  const size_t need = ijbc_roc_workspace_bytes(P, G);
  FEDFR_REQUIRE(ws && ws_bytes >= need, "%s: workspace of %zu bytes, %zu needed", who, ws_bytes, need);
  return FEDFR_OK;
}

int ijbc_pair_scores_roc(const double* feats, int T, int D, const int* lut, long long lut_n, const long long* p1, const long long* p2,
                         long long P, double* score, const long long* label, const double* gv, int G, unsigned long long* counts, void* ws,
                         size_t ws_bytes, int* status, hipStream_t st) {
  FEDFR_REQUIRE(feats && lut && p1 && p2 && status, "pair_scores_roc: null pointer (feats, lut, p1, p2 and status are required)");
  FEDFR_REQUIRE(T > 0 && lut_n > 0 && P > 0, "pair_scores_roc: bad sizes (T = %d, lut_n = %lld, P = %lld)", T, lut_n, P);
  FEDFR_REQUIRE(pw_supported(D), "pair_scores_roc: D = %d unsupported (D <= 128 or D in {256, 512, 1024})", D);
  FEDFR_REQUIRE(score || gv, "pair_scores_roc: neither score nor counts requested");
  if (gv) FEDFR_TRY(roc_args(P, label, gv, G, counts, ws, ws_bytes, "pair_scores_roc"));
  allow_big_lds();
  const int nwg = count_wgs(P);
  const size_t lds = gv ? (size_t)(G + 1) * sizeof(unsigned) : 0;
  hipLaunchKernelGGL(ijbc_pair_kernel, dim3(nwg), dim3(256), lds, st, feats, T, D, lut, lut_n, p1, p2, P, score, label, gv, G,
                     static_cast<unsigned*>(ws), counts, status);
  FEDFR_LAUNCH_CHECK("ijbc_pair");
  return gv ? roc_finish(static_cast<unsigned*>(ws), nwg, G, counts, st) : FEDFR_OK;
}

int ijbc_roc_counts(const double* score, const long long* label, long long P, const double* gv, int G, unsigned long long* counts, void* ws,
                    size_t ws_bytes, int* status, hipStream_t st) {
  FEDFR_REQUIRE(score && status, "roc_counts: null pointer (score and status are required)");
  FEDFR_REQUIRE(P > 0, "roc_counts: P = %lld must be > 0", P);
  FEDFR_TRY(roc_args(P, label, gv, G, counts, ws, ws_bytes, "roc_counts"));
  allow_big_lds();
  const int nwg = count_wgs(P);
  hipLaunchKernelGGL(ijbc_roc_count_kernel, dim3(nwg), dim3(256), (size_t)(G + 1) * sizeof(unsigned), st, score, label, P, gv, G,
                     static_cast<unsigned*>(ws), counts, status);
  FEDFR_LAUNCH_CHECK("ijbc_roc_count");
  return roc_finish(static_cast<unsigned*>(ws), nwg, G, counts, st);
}
