// Grouped pair histogram: the pairwise ROC histogram of head.hip (roc_hist_kernel; reference roc_cuda.py:14-30 calc_ROC after the
// target-first reordering of :127-134) for G disjoint target sets in ONE pass over the unordered pairs of a feature matrix — what the
// reference's "all clients" 1:1 evaluation (local_all.py:303-335) gets from G runs of roc_cuda.py on the same features.
//
// Row i has a group g[i] in [-1, G) (-1: a target of nobody).  For every unordered pair {a, b}, a != b:
//   bin = int((<f_a, f_b> + 1) * 1000), fp64 dot product of the fp32 features, clamped to [0, 2000]; column = label[a] == label[b] ? 0 : 1;
//   the pair is counted in hist[g[a]] if g[a] >= 0, and in hist[g[b]] if g[b] >= 0 and g[b] != g[a].
// hist[c] is therefore what roc_hist_kernel returns for group c's rows first: every pair with at least one row in c, once.
//
// Layout: the host hands in a row-index array of n_tiles * 64 slots in which every group starts at a multiple of 64 (padding slots -1,
// ungrouped rows last) and the group of every 64-slot tile.  The kernel gathers feature rows through the index (no reordered copy of the
// matrix); each 64-slot side of a 64 x 64 pair tile belongs to one group, so ALL pairs of a tile go to the same one or two histograms:
// one LDS-private 4002-counter histogram per workgroup is enough, flushed with 64-bit integer atomics to one or two global histograms
// (order-free: deterministic).  The grid is 1-D over the tile pairs (ta <= tb) with ta a grouped tile: tiles below the diagonal and
// tiles between two ungrouped sides are never launched.  No workgroup waits for another.
// Tile arithmetic (64 x 64, 2 x 2 waves of 32 x 32, v_mfma_f64_16x16x4_f64, BK = 16, double-buffered k-major LDS rows with the XOR
// swizzle) and the accumulator layout are roc_hist_kernel's: every dot product is the same fp64 number there and here.
#include "head.h"

namespace {

typedef __attribute__((ext_vector_type(4))) double f64x4_t;
constexpr int BK = 16, LD = 80, NBIN = 4002;

__global__ __launch_bounds__(256) void roc_hist_groups_kernel(const float* __restrict__ feat, const long long* __restrict__ label,
                                                              const int* __restrict__ row_index, const int* __restrict__ tile_group, int N,
                                                              int D, int n_tiles, int G, unsigned long long* __restrict__ hist) {
  __shared__ float sA[2][BK][LD], sB[2][BK][LD];
  __shared__ unsigned lh[NBIN];
  __shared__ int sRow[2][64];                                  // feature row of every slot of the two sides, -1 = padding
  __shared__ long long sLab[2][64];
  // linear index -> (ta, tb), ta <= tb < n_tiles: row ta of the triangle starts at S(ta) = ta * n - ta (ta - 1) / 2
  const long long idx = blockIdx.x, n2 = 2LL * n_tiles + 1;
  int ta = (int)(((double)n2 - sqrt((double)(n2 * n2 - 8 * idx))) * 0.5);
  ta = ta < 0 ? 0 : (ta > n_tiles - 1 ? n_tiles - 1 : ta);
  auto start = [&](long long t) { return t * n_tiles - t * (t - 1) / 2; };
  while (ta + 1 < n_tiles && start(ta + 1) <= idx) ++ta;      // (the fp64 root is off by at most one row)
  while (ta > 0 && start(ta) > idx) --ta;
  const int tb = ta + (int)(idx - start(ta));
  if (tb >= n_tiles) return;
  int ga = tile_group[ta], gb = tile_group[tb];
  ga = (ga >= 0 && ga < G) ? ga : -1;
  gb = (gb >= 0 && gb < G) ? gb : -1;
  if (ga < 0 && gb < 0) return;                                // workgroup-uniform: no pair of this tile has a target row
  const int h0 = ga >= 0 ? ga : gb, h1 = (ga >= 0 && gb >= 0 && gb != ga) ? gb : -1;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  for (int i = tid; i < NBIN; i += 256) lh[i] = 0u;
  if (tid < 128) {
    const int side = tid >> 6, s = tid & 63;
    int r = row_index[(size_t)(side ? tb : ta) * 64 + s];
    r = (r >= 0 && r < N) ? r : -1;
    sRow[side][s] = r;
    sLab[side][s] = r >= 0 ? label[r] : 0;
  }
  int rowa[4], rowb[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {                                // this thread's four rows of either side (the same for every k-step)
    const int m = (tid + 256 * i) >> 4;
    int r = row_index[(size_t)ta * 64 + m];
    rowa[i] = (r >= 0 && r < N) ? r : -1;
    r = row_index[(size_t)tb * 64 + m];
    rowb[i] = (r >= 0 && r < N) ? r : -1;
  }
  float ra[4], rb[4];
  auto load = [&](int k0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int gk = k0 + ((tid + 256 * i) & 15);              // features are row-major: k fastest
      ra[i] = (rowa[i] >= 0 && gk < D) ? feat[(size_t)rowa[i] * D + gk] : 0.f;
      rb[i] = (rowb[i] >= 0 && gk < D) ? feat[(size_t)rowb[i] * D + gk] : 0.f;
    }
  };
  auto store = [&](int buf) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int e = tid + 256 * i, k = e & 15, m = e >> 4;
      sA[buf][k][m ^ ((k >> 1) << 1)] = ra[i];
      sB[buf][k][m ^ ((k >> 1) << 1)] = rb[i];
    }
  };
  f64x4_t acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = (f64x4_t){0.0, 0.0, 0.0, 0.0};
  const int nk = ceil_div(D, BK);
  load(0);
  store(0);
  __syncthreads();
  const int l15 = lane & 15, lg = lane >> 4;
  for (int kt = 0; kt < nk; ++kt) {
    const int buf = kt & 1;
    if (kt + 1 < nk) load((kt + 1) * BK);
#pragma unroll
    for (int k4 = 0; k4 < BK; k4 += 4) {
      double fa[2], fb[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int kk = k4 + lg, sw = (kk >> 1) << 1;
        fa[i] = (double)sA[buf][kk][(wm * 32 + i * 16 + l15) ^ sw];
        fb[i] = (double)sB[buf][kk][(wn * 32 + i * 16 + l15) ^ sw];
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[i], fb[j], acc[i][j], 0, 0, 0);
    }
    if (kt + 1 < nk) store(buf ^ 1);
    __syncthreads();
  }
  // f64 16x16x4 accumulator layout: register q of lane l holds D[row = 4 q + (l >> 4)][col = l & 15]
  const bool diag = ta == tb;                                  // within a diagonal tile every pair shows up twice: keep slot a < slot b
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int sb = wn * 32 + j * 16 + l15;
    const bool vb = sRow[1][sb] >= 0;
    const long long lb = sLab[1][sb];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int sa = wm * 32 + i * 16 + q * 4 + lg;
        if (vb && sRow[0][sa] >= 0 && (!diag || sa < sb)) {
          int bin = (int)((acc[i][j][q] + 1.0) * 1000.0);           // truncation, as int() in the reference
          bin = bin < 0 ? 0 : (bin > 2000 ? 2000 : bin);             // (the reference would write out of bounds instead)
          atomicAdd(&lh[2 * bin + (sLab[0][sa] == lb ? 0 : 1)], 1u);
        }
      }
  }
  __syncthreads();
  unsigned long long* const o0 = hist + (size_t)h0 * NBIN;
  unsigned long long* const o1 = h1 >= 0 ? hist + (size_t)h1 * NBIN : nullptr;
  for (int i = tid; i < NBIN; i += 256)
    if (lh[i]) {
      atomicAdd(&o0[i], (unsigned long long)lh[i]);
      if (o1) atomicAdd(&o1[i], (unsigned long long)lh[i]);
    }
}

}  // namespace

int head_roc_histogram_groups(const float* feat, const long long* label, int N, int D, const int* row_index, const int* tile_group,
                              int n_tiles, int G, int* tile_group_dev, unsigned long long* hist, hipStream_t st) {
  FEDFR_REQUIRE(feat && label && row_index && tile_group && tile_group_dev && hist, "roc_histogram_groups: null pointer");
  FEDFR_REQUIRE(N > 0, "roc_histogram_groups: N = %d must be >= 1", N);
  FEDFR_REQUIRE(D > 0, "roc_histogram_groups: D = %d must be >= 1", D);
  FEDFR_REQUIRE(G > 0, "roc_histogram_groups: G = %d must be >= 1", G);
  FEDFR_REQUIRE(n_tiles > 0 && n_tiles <= (1 << 24), "roc_histogram_groups: n_tiles = %d outside [1, 2^24]", n_tiles);
  int grouped = 0;                                             // tiles [0, grouped) hold every tile that has a group
  for (int t = 0; t < n_tiles; ++t) {
    FEDFR_REQUIRE(tile_group[t] >= -1 && tile_group[t] < G, "roc_histogram_groups: tile %d has group id %d outside [-1, G = %d)", t,
                  tile_group[t], G);
    if (tile_group[t] >= 0) grouped = t + 1;
  }
  if (grouped == 0) return FEDFR_OK;                           // nobody has a target: every histogram stays as it is
  const long long blocks = (long long)grouped * n_tiles - (long long)grouped * (grouped - 1) / 2;
  FEDFR_REQUIRE(blocks < (1LL << 31), "roc_histogram_groups: %lld tile pairs exceed one grid", blocks);
  if (hipMemcpyAsync(tile_group_dev, tile_group, (size_t)n_tiles * sizeof(int), hipMemcpyHostToDevice, st) != hipSuccess) {
    fedfr_set_error("roc_histogram_groups: %s", hipGetErrorString(hipGetLastError()));
    return FEDFR_ERR_HIP;
  }
  hipLaunchKernelGGL(roc_hist_groups_kernel, dim3((unsigned)blocks), dim3(256), 0, st, feat, label, row_index, tile_group_dev, N, D,
                     n_tiles, G, hist);
  FEDFR_LAUNCH_CHECK("roc_histogram_groups");
  return FEDFR_OK;
}
