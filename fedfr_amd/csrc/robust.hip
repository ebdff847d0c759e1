// Robust aggregation over k flat fp32 client states: HBM-bound streaming passes on the skeleton of multi_state.h (as fedavg_multi_kernel / fedopt_sqnorm_kernel, optim.hip).
//   robust_trimmed_mean_kernel<K, V>   coordinate-wise trimmed mean (Yin et al., 2018); trim = (K - 1) / 2 is the coordinate-wise median
//   robust_pairdist_kernel<TA, TB>     all pairwise squared distances of the states, fp64, no atomics
//   robust_krum_select_kernel          Krum / Multi-Krum scores and selection (Blanchard et al., 2017) from the distance matrix, one block
//
// ORDER of the trimmed mean: a total order on bit patterns.  A value with bits u that is not a NaN has the unsigned key
// u ^ (sign ? 0xFFFFFFFF : 0x80000000): -inf < ... < -0 < +0 < ... < +inf.  Every NaN (either sign, any payload) has key 0xFFFFFFFF and sorts
// last, so a client that sends NaN is trimmed first.  Keys are sorted ascending, s_0 <= ... <= s_{K-1}.
// ARITHMETIC of the trimmed mean: acc = s_b; acc = acc + s_j for j = b + 1 .. K - 1 - b in ascending order, one fp32 rounding each (__fadd_rn);
// dst = acc / (float)(K - 2 b), one correctly rounded division (__fdiv_rn, see the note on division in optim.hip).  A key 0xFFFFFFFF that is
// kept decodes to a NaN and makes the result NaN.  tests/robust_cases.py restates exactly this and the kernel is held to it bit for bit.
// The sort is a compile-time compare-exchange network on the key registers (Batcher's merge exchange, valid for every K: 19 exchanges at K = 8,
// 63 at K = 16, 191 at K = 32), each exchange a v_min_u32 / v_max_u32 pair per component; nothing is indexed by a runtime value, so nothing
// lives in scratch memory.  `trim` is a runtime argument: the kept range is chosen with selects on the unrolled sum.
#include "robust.h"
#include "robust_net.h"
#include "multi_state.h"
#include <utility>

// ---------------------------------------------------------------------------------------------------------
// trimmed mean / median
// ---------------------------------------------------------------------------------------------------------
template <int V>
__device__ __forceinline__ void robust_cmpex(unsigned (&lo)[V], unsigned (&hi)[V]) {
#pragma unroll
  for (int c = 0; c < V; ++c) {
    const unsigned x = lo[c], y = hi[c];
    lo[c] = min(x, y);
    hi[c] = max(x, y);
  }
}
template <int K, int V, size_t... I>
__device__ __forceinline__ void robust_sort(unsigned (&key)[K][V], std::index_sequence<I...>) {
  constexpr RobustNet<K> net = robust_make_net<K>();
  (robust_cmpex<V>(key[net.a[I]], key[net.b[I]]), ...);      // every index is a constant: the keys stay in registers
}
__device__ __forceinline__ unsigned robust_key(float v) {
  const unsigned u = __float_as_uint(v);
  const unsigned k = u ^ ((unsigned)((int)u >> 31) | 0x80000000u);
  return (u & 0x7FFFFFFFu) > 0x7F800000u ? 0xFFFFFFFFu : k;
}
__device__ __forceinline__ float robust_unkey(unsigned k) {      // (0xFFFFFFFF -> 0x7FFFFFFF, a NaN)
  return __uint_as_float(k ^ ((unsigned)((int)~k >> 31) | 0x80000000u));
}
// sum of the sorted values b .. K - 1 - b in ascending order, starting FROM s_b (0 + s_b would turn -0 into +0), then one division
template <int K, int V>
__device__ __forceinline__ float robust_kept_mean(const unsigned (&key)[K][V], int c, int b, float cnt) {
  float acc = 0.f;
#pragma unroll
  for (int j = 0; j < K; ++j) {
    const float v = robust_unkey(key[j][c]);
    const float t = __fadd_rn(acc, v);
    acc = j == b ? v : (j > b && j < K - b ? t : acc);
  }
  return __fdiv_rn(acc, cnt);
}
// V floats per lane and load: 4 for K <= 16 (64 key registers at K = 16), 2 for K = 17 .. 32 (64 key registers at K = 32).  dst aliases no source.
// Two explicit loops, not for_each_vec_then_tail: through the callable most K need 30-60 more VGPRs (K = 8: 41 -> 88) and lose occupancy
// (profiles/multi_state_resources_v1.txt).
template <int K, int V>
__global__ __launch_bounds__(MULTI_STATE_BLOCK) void robust_trimmed_mean_kernel(float* __restrict__ dst, StatePtrs<K> p, size_t n, int b) {
  typedef fvec<V> vec;
  constexpr auto seq = std::make_index_sequence<robust_make_net<K>().n>{};
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const size_t nv = n / V;
  const float cnt = (float)(K - 2 * b);
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += stride) {
    vec v[K];
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = ld_once<V>(p.src[k], i);      // all K loads in flight
    __builtin_amdgcn_sched_barrier(0);      // keep the K loads together in front of their first use (at some K the scheduler otherwise waits for each in turn)
    unsigned key[K][V];
#pragma unroll
    for (int k = 0; k < K; ++k) {
#pragma unroll
      for (int c = 0; c < V; ++c) key[k][c] = robust_key(v[k][c]);
    }
    robust_sort<K, V>(key, seq);
    vec o;
#pragma unroll
    for (int c = 0; c < V; ++c) o[c] = robust_kept_mean<K, V>(key, c, b, cnt);
    reinterpret_cast<vec*>(dst)[i] = o;
  }
  for (size_t i = nv * V + (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    unsigned key[K][1];
#pragma unroll
    for (int k = 0; k < K; ++k) key[k][0] = robust_key(p.src[k][i]);
    robust_sort<K, 1>(key, seq);
    dst[i] = robust_kept_mean<K, 1>(key, 0, b, cnt);
  }
}
int robust_trimmed_mean(float* dst, const float* const* srcs, int k, int trim, size_t n, hipStream_t st) {
  FEDFR_REQUIRE(dst && srcs && n > 0, "robust_trimmed_mean: bad args");
  FEDFR_REQUIRE(k >= 1 && k <= 32, "robust_trimmed_mean: k must be 1..32: an order statistic cannot be chained over groups of clients (k=%d)", k);
  FEDFR_REQUIRE(trim >= 0 && trim <= (k - 1) / 2, "robust_trimmed_mean: trim must satisfy 0 <= 2 trim < k (trim=%d k=%d)", trim, k);
  StatePtrs<32> all{};
  uintptr_t al = (uintptr_t)dst;
  FEDFR_TRY(state_ptrs_fill(all, srcs, k, "robust_trimmed_mean", "source", al));
  for (int i = 0; i < k; ++i) FEDFR_REQUIRE(srcs[i] + n <= dst || dst + n <= srcs[i], "robust_trimmed_mean: dst overlaps source %d", i);
  FEDFR_REQUIRE((al & 15) == 0, "robust_trimmed_mean: buffers must be 16-byte aligned");
  dispatch_int<1, 32>(k, [&](auto kc) {
    constexpr int K = decltype(kc)::value;
    StatePtrs<K> p;      // CAP = K: the kernel argument is no larger than the states it names
    for (int i = 0; i < K; ++i) p.src[i] = all.src[i];
    hipLaunchKernelGGL((robust_trimmed_mean_kernel<K, (K <= 16 ? 4 : 2)>), dim3(multi_state_grid(n)), dim3(MULTI_STATE_BLOCK), 0, st, dst, p, n, trim);
  });
  FEDFR_LAUNCH_CHECK("robust_trimmed_mean");
  return FEDFR_OK;
}

// ---------------------------------------------------------------------------------------------------------
// Pairwise squared distances D[i][j] = sum_e (double) (x_i[e] - x_j[e] in fp32)^2: fp32 subtract, exact fp64 square, fp64 sum (one rounding per
// term: fma(d, d, acc)).  No atomics: one fp64 partial per pair and block in the workspace ([k (k - 1) / 2][grid]); lanes by a fixed shuffle tree,
// waves in ascending order through LDS, blocks in ascending order by robust_pairdist_final_kernel: two runs give the same bits.
// TB == 0: the TA (TA - 1) / 2 pairs among TA states (float4 loads to TA = 8, float2 above).  TA = 13 (78 accumulators = 156 registers, 254 VGPRs,
// no scratch) is the largest that stays inside the 256 architectural registers (TA = 14 compiles to 256 VGPRs + 34 AGPRs of copies at one wave per
// SIMD): k <= 13 is ONE launch that reads every state once.  More clients are cut into groups of 8: one TB == 0 launch per group and one TB > 0
// launch per pair of groups (the 8 x TB pairs between them, float2 loads, <= 64 accumulators, 16 distinct states).
// Two explicit loops, not for_each_vec_then_tail: through the callable <5, 0> and <6, 0> need 30 and 58 more VGPRs and lose occupancy.
// ---------------------------------------------------------------------------------------------------------
__host__ __device__ static inline int robust_pair_index(int i, int j, int k) {      // i < j: row-major upper triangle
  return i * k - i * (i + 1) / 2 + (j - i - 1);
}
template <int TA, int TB>
__global__ __launch_bounds__(MULTI_STATE_BLOCK) void robust_pairdist_kernel(StatePtrs<16> pa, StatePtrs<8> pb, size_t n, int a0, int b0, int k,
                                                              double* __restrict__ part) {
  constexpr bool CROSS = TB > 0;
  constexpr int P = CROSS ? TA * TB : TA * (TA - 1) / 2;
  constexpr int V = (CROSS || TA > 8) ? 2 : 4;
  constexpr int NB = CROSS ? TB : 1;
  typedef fvec<V> vec;
  __shared__ double red[4][P];
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const size_t nv = n / V;
  double acc[P];
#pragma unroll
  for (int q = 0; q < P; ++q) acc[q] = 0.0;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += stride) {
    vec sa[TA], sb[NB];
#pragma unroll
    for (int a = 0; a < TA; ++a) sa[a] = ld_once<V>(pa.src[a], i);
    if (CROSS) {
#pragma unroll
      for (int b = 0; b < NB; ++b) sb[b] = ld_once<V>(pb.src[b], i);
    }
#pragma unroll
    for (int a = 0; a < TA; ++a) {
#pragma unroll
      for (int b = CROSS ? 0 : a + 1; b < (CROSS ? TB : TA); ++b) {
        const int q = CROSS ? a * TB + b : robust_pair_index(a, b, TA);
        const vec y = CROSS ? sb[CROSS ? b : 0] : sa[CROSS ? 0 : b];
#pragma unroll
        for (int c = 0; c < V; ++c) {
          const double d = (double)__fsub_rn(sa[a][c], y[c]);
          acc[q] = __fma_rn(d, d, acc[q]);
        }
      }
    }
  }
  for (size_t i = nv * V + (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    float sa[TA], sb[NB];
#pragma unroll
    for (int a = 0; a < TA; ++a) sa[a] = pa.src[a][i];
    if (CROSS) {
#pragma unroll
      for (int b = 0; b < NB; ++b) sb[b] = pb.src[b][i];
    }
#pragma unroll
    for (int a = 0; a < TA; ++a) {
#pragma unroll
      for (int b = CROSS ? 0 : a + 1; b < (CROSS ? TB : TA); ++b) {
        const int q = CROSS ? a * TB + b : robust_pair_index(a, b, TA);
        const double d = (double)__fsub_rn(sa[a], CROSS ? sb[CROSS ? b : 0] : sa[CROSS ? 0 : b]);
        acc[q] = __fma_rn(d, d, acc[q]);
      }
    }
  }
  block_partial_d<P>(acc, red, part, [&](int q) {      // the row of the workspace: the pair's index among all k states
    int a = 0, b = 0;
    if (CROSS) {
      a = q / NB;
      b = q % NB;
    } else {
      while (robust_pair_index(a + 1, a + 2, TA) <= q && a + 2 < TA) ++a;      // the row of the upper triangle that holds q
      b = a + 1 + (q - robust_pair_index(a, a + 1, TA));
    }
    return robust_pair_index(a0 + a, (CROSS ? b0 : a0) + b, k);
  });
}
// one wave per pair: its `grid` partials are added in ascending block order (ordered_partial_sum).  Writes D[i][j] and D[j][i]; the k waves
// after the last pair write the zero diagonal.
__global__ __launch_bounds__(256) void robust_pairdist_final_kernel(const double* __restrict__ part, int grid, int k, double* __restrict__ dist) {
  const int gw = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int npairs = k * (k - 1) / 2;
  if (gw >= npairs) {
    if (gw < npairs + k && lane == 0) dist[(size_t)(gw - npairs) * k + (gw - npairs)] = 0.0;
    return;
  }
  const double s = ordered_partial_sum(part + (size_t)gw * grid, grid, lane);
  if (lane != 0) return;
  int i = 0;
  while (i + 2 < k && robust_pair_index(i + 1, i + 2, k) <= gw) ++i;
  const int j = i + 1 + (gw - robust_pair_index(i, i + 1, k));
  dist[(size_t)i * k + j] = s;
  dist[(size_t)j * k + i] = s;
}
size_t robust_pairdist_ws_bytes(int k, size_t n) {
  if (k < 2 || k > 32 || n == 0) return 0;
  return (size_t)(k * (k - 1) / 2) * multi_state_grid(n) * sizeof(double);
}
int robust_pairdist(const float* const* xs, int k, size_t n, double* dist, void* wsp, size_t ws_bytes, hipStream_t st) {
  FEDFR_REQUIRE(xs && dist && wsp && n > 0, "robust_pairdist: bad args");
  FEDFR_REQUIRE(k >= 2 && k <= 32, "robust_pairdist: k must be 2..32 (k=%d)", k);
  StatePtrs<32> all{};
  uintptr_t al = 0;
  FEDFR_TRY(state_ptrs_fill(all, xs, k, "robust_pairdist", "client state", al));
  FEDFR_REQUIRE((al & 15) == 0, "robust_pairdist: client states must be 16-byte aligned");
  FEDFR_REQUIRE((((uintptr_t)dist | (uintptr_t)wsp) & 7) == 0, "robust_pairdist: dist / workspace must be 8-byte aligned");
  const int grid = multi_state_grid(n);
  const size_t need = (size_t)(k * (k - 1) / 2) * grid * sizeof(double);
  if (ws_bytes < need) {
    fedfr_set_error("robust_pairdist: workspace of %zu bytes, %zu needed", ws_bytes, need);
    return FEDFR_ERR_WORKSPACE;
  }
  double* part = reinterpret_cast<double*>(wsp);
  constexpr int ONE = 13;                      // the largest diagonal tile: up to here one launch, beyond it groups of 8
  const int gs = k <= ONE ? ONE : 8, ng = (k + gs - 1) / gs;
  for (int ga = 0; ga < ng; ++ga) {
    const int a0 = gs * ga, ta = k - a0 < gs ? k - a0 : gs;
    StatePtrs<16> pa{};
    StatePtrs<8> pb{};
    for (int a = 0; a < ta; ++a) pa.src[a] = all.src[a0 + a];
    dispatch_int<2, ONE>(ta, [&](auto tc) {      // (a last group of one state has no pair of its own)
      hipLaunchKernelGGL((robust_pairdist_kernel<decltype(tc)::value, 0>), dim3(grid), dim3(MULTI_STATE_BLOCK), 0, st, pa, pb, n, a0, a0, k, part);
    });
    for (int gb = ga + 1; gb < ng; ++gb) {      // (only with groups of 8, and ga is not the last group here: ta == 8)
      const int b0 = gs * gb, tb = k - b0 < gs ? k - b0 : gs;
      for (int b = 0; b < tb; ++b) pb.src[b] = all.src[b0 + b];
      dispatch_int<1, 8>(tb, [&](auto tc) {
        hipLaunchKernelGGL((robust_pairdist_kernel<8, decltype(tc)::value>), dim3(grid), dim3(MULTI_STATE_BLOCK), 0, st, pa, pb, n, a0, b0, k, part);
      });
    }
  }
  FEDFR_LAUNCH_CHECK("robust_pairdist");
  const int npairs = k * (k - 1) / 2;
  hipLaunchKernelGGL(robust_pairdist_final_kernel, dim3(ceil_div(npairs + k, 4)), dim3(256), 0, st, part, grid, k, dist);
  FEDFR_LAUNCH_CHECK("robust_pairdist_final");
  return FEDFR_OK;
}

// ---------------------------------------------------------------------------------------------------------
// Krum / Multi-Krum: score_i = the k - f - 2 smallest D[i][j], j != i, added in ascending order in fp64 (a distance that is not finite counts as
// +inf); the m lowest scores are selected, ties to the lower client index.  One block, thread i owns client i; the rows live in LDS (a per-thread
// row indexed at run time would be scratch memory).
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void robust_krum_select_kernel(const double* __restrict__ dist, int k, int f, int m, double* __restrict__ score,
                                                                int* __restrict__ selected) {
  __shared__ double row[32][33];
  __shared__ double sc[32];
  const int i = threadIdx.x;
  const double inf = __longlong_as_double(0x7FF0000000000000ll);
  double s = 0.0;
  if (i < k) {
    for (int j = 0; j < k; ++j) {
      const double v = dist[(size_t)i * k + j];
      row[i][j] = isfinite(v) ? v : inf;
    }
    unsigned used = 1u << i;
    for (int t = 0; t < k - f - 2; ++t) {
      int best = -1;
      double bv = inf;
      for (int j = 0; j < k; ++j) {
        const double v = row[i][j];
        if (!((used >> j) & 1u) && (best < 0 || v < bv)) {
          best = j;
          bv = v;
        }
      }
      used |= 1u << best;
      s += bv;
    }
    sc[i] = s;
    score[i] = s;
  }
  __syncthreads();
  if (i < k) {
    int r = 0;
    for (int j = 0; j < k; ++j) {
      const double sj = sc[j];
      r += (sj < s || (sj == s && j < i)) ? 1 : 0;
    }
    selected[i] = r < m ? 1 : 0;
  }
}
int robust_krum_select(const double* dist, int k, int f, int m, double* score, int* selected, hipStream_t st) {
  FEDFR_REQUIRE(dist && score && selected, "robust_krum_select: bad args");
  FEDFR_REQUIRE(k >= 3 && k <= 32 && f >= 0 && f <= (k - 3) / 2, "robust_krum_select: needs 2 f + 3 <= k <= 32 (k=%d f=%d)", k, f);
  FEDFR_REQUIRE(m >= 1 && m <= k - f, "robust_krum_select: m must be 1..k - f (m=%d k=%d f=%d)", m, k, f);
  FEDFR_REQUIRE((((uintptr_t)dist | (uintptr_t)score) & 7) == 0 && ((uintptr_t)selected & 3) == 0,
                "robust_krum_select: dist / score must be 8-byte, selected 4-byte aligned");
  hipLaunchKernelGGL(robust_krum_select_kernel, dim3(1), dim3(64), 0, st, dist, k, f, m, score, selected);
  FEDFR_LAUNCH_CHECK("robust_krum_select");
  return FEDFR_OK;
}
