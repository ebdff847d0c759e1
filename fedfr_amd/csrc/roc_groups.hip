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
// The tile (tile64.h, fp64 accumulation, BK = 16) and the histogram slot (roc_slot, head.h) are roc_hist_kernel's: every dot product is the
// same fp64 number there and here.
#include "head.h"
#include "tile64.h"

namespace {

constexpr int BK = 16;

__global__ __launch_bounds__(256) void roc_hist_groups_kernel(const float* __restrict__ feat, const long long* __restrict__ label,
                                                              const int* __restrict__ row_index, const int* __restrict__ tile_group, int N,
                                                              int D, int n_tiles, int G, unsigned long long* __restrict__ hist) {
  __shared__ tile64::Lds<BK> s;
  __shared__ unsigned lh[ROC_NBIN];
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
  const int tid = threadIdx.x;
  for (int i = tid; i < ROC_NBIN; i += 256) lh[i] = 0u;
  if (tid < 128) {
    const int side = tid >> 6, sl = tid & 63;
    int r = row_index[(size_t)(side ? tb : ta) * 64 + sl];
    r = (r >= 0 && r < N) ? r : -1;
    sRow[side][sl] = r;
    sLab[side][sl] = r >= 0 ? label[r] : 0;
  }
  int rowa[4], rowb[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {                                // this thread's four rows of either side (the same for every k-step)
    int m, k;
    tile64::elem<BK>(true, i, m, k);
    int r = row_index[(size_t)ta * 64 + m];
    rowa[i] = (r >= 0 && r < N) ? r : -1;
    r = row_index[(size_t)tb * 64 + m];
    rowb[i] = (r >= 0 && r < N) ? r : -1;
  }
  float ra[4], rb[4];
  auto row = [&](int r, int gk) { return (r >= 0 && gk < D) ? feat[(size_t)r * D + gk] : 0.f; };   // features are row-major: k fastest
  auto load = [&](int k0) {
    tile64::load<BK>(ra, true, [&](int, int k, int i) { return row(rowa[i], k0 + k); });
    tile64::load<BK>(rb, true, [&](int, int k, int i) { return row(rowb[i], k0 + k); });
  };
  auto store = [&](int buf) {
    tile64::store(s, 0, buf, true, ra);
    tile64::store(s, 1, buf, true, rb);
  };
  f64x4_t acc[2][2];
  tile64::zero(acc);
  tile64::k_loop<BK>(s, acc, 0, D, load, store);
  const bool diag = ta == tb;                                  // within a diagonal tile every pair shows up twice: keep slot a < slot b
  struct Col { bool valid; long long label; };
  tile64::for_each(
      acc, [&](int sb) { return Col{sRow[1][sb] >= 0, sLab[1][sb]}; },
      [&](int sa, int sb, double v, const Col& c) {
        if (c.valid && sRow[0][sa] >= 0 && (!diag || sa < sb)) atomicAdd(&lh[roc_slot(v, sLab[0][sa] == c.label)], 1u);
      });
  __syncthreads();
  unsigned long long* const o0 = hist + (size_t)h0 * ROC_NBIN;
  unsigned long long* const o1 = h1 >= 0 ? hist + (size_t)h1 * ROC_NBIN : nullptr;
  for (int i = tid; i < ROC_NBIN; i += 256)
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
