// 1:N identification read-out (reference local_all.py:142-176 `evaluation`, driven per client by :274-297): one positive score per query
// and the exact top-K of the negative scores of every column segment (one segment per client gallery), the query x gallery similarity
// matrix never written to memory.
//
// ident_tile_kernel, grid (X, S): workgroup (x, s) walks the 64-row query tiles x, x + X, ... and, for each, the columns of segment s in
// 64-wide chunks.  A chunk is one 64 x 64 tile of tile64.h with fp64 accumulation (roc_hist_kernel's): every score is the same fp64 number
// whichever workgroup computes it.  Epilogue: a positive pair (qid[q] >= 0 and qid[q] == gid[c]) writes pos[q]; a negative that beats the
// workgroup's running K-th bound goes to the LDS candidate buffer of topk_cand.h.  The workgroup ends with its sorted top-K (and its negative count) in a
// workspace slab; ident_merge_kernel (one workgroup per segment) runs the same buffer over the segment's X slabs.  The result is the top-K
// multiset itself (ties included) and no floating-point atomics are used: the output does not depend on the order workgroups run in.
#include <algorithm>
#include "head.h"
#include "tile64.h"
#include "topk_cand.h"

namespace {

constexpr int kMaxK = 1024;           // fedfr_ident_topk's K limit (FAR 1e-3 up to ~1M queries)
constexpr int kCap = 4096;            // LDS candidates per workgroup (32 KB); > kMaxK, so a cut always keeps room for new ones
constexpr int kTileWgs = 3072;        // tile-kernel workgroups over all segments: 256 CUs x 3 resident x 4 rounds

struct Cand {                         // the candidate buffer of topk_cand.h in static LDS
  double v[kCap];
  CandHdr h;
};

__global__ __launch_bounds__(256) void ident_tile_kernel(const float* __restrict__ query, const long long* __restrict__ qid, int Q,
                                                         const float* __restrict__ gallery, const long long* __restrict__ gid, int D,
                                                         const long long* __restrict__ seg, int K, double* __restrict__ pos,
                                                         double* __restrict__ slab, unsigned long long* __restrict__ slab_negs) {
  constexpr int BK = 16;
  __shared__ tile64::Lds<BK> t;
  __shared__ Cand c;
  CandHdr& h = c.h;
  double* const cv = c.v;
  const int s = blockIdx.y, X = gridDim.x;
  const int c_beg = (int)seg[s], c_end = (int)seg[s + 1];
  const int tid = threadIdx.x;
  cand_init(h);
  __syncthreads();
  unsigned long long negs = 0ull;
  const int ntile = ceil_div(Q, 64);
  for (int tq = blockIdx.x; tq < ntile; tq += X) {
    const int a0 = tq * 64;
    for (int b0 = c_beg; b0 < c_end; b0 += 64) {
      float ra[4], rb[4];
      auto load = [&](int k0) {
        tile64::load<BK>(ra, true, [&](int m, int k, int) { return (a0 + m < Q && k0 + k < D) ? query[(size_t)(a0 + m) * D + k0 + k] : 0.f; });
        tile64::load<BK>(rb, true, [&](int m, int k, int) { return (b0 + m < c_end && k0 + k < D) ? gallery[(size_t)(b0 + m) * D + k0 + k] : 0.f; });
      };
      auto store = [&](int buf) {
        tile64::store(t, 0, buf, true, ra);
        tile64::store(t, 1, buf, true, rb);
      };
      f64x4_t acc[2][2];
      tile64::zero(acc);
      tile64::k_loop<BK>(t, acc, 0, D, load, store);
      double v[16];
      unsigned pend = 0u;
      int r = 0;                      // position in the walk: a constant once the walk is unrolled
      tile64::for_each(
          acc, [&](int n) { return b0 + n < c_end ? gid[b0 + n] : -1; },
          [&](int m, int n, double x, long long gb) {
            const int a = a0 + m, b = b0 + n;
            v[r] = x;
            if (a < Q && b < c_end) {
              const long long qa = qid[a];
              if (qa >= 0 && qa == gb) {
                pos[a] = x;
              } else {
                ++negs;
                pend |= 1u << r;
              }
            }
            ++r;
          });
      cand_offer<kCap>(h, cv, v, pend, K);
    }
  }
  atomicAdd(&h.negs, negs);
  __syncthreads();
  cand_cut<kCap>(h, cv, K);
  const size_t o = (size_t)s * X + blockIdx.x;
  for (int i = tid; i < K; i += 256) slab[o * K + i] = i < h.n ? cv[i] : -INFINITY;
  if (tid == 0) slab_negs[o] = h.negs;
}

// segment s: the top-K of its X sorted slabs (-inf entries are padding and never enter) and the sum of their negative counts
__global__ __launch_bounds__(256) void ident_merge_kernel(const double* __restrict__ slab, const unsigned long long* __restrict__ slab_negs,
                                                          int X, int K, double* __restrict__ topk, long long* __restrict__ neg_count) {
  __shared__ Cand c;
  CandHdr& h = c.h;
  double* const cv = c.v;
  const int s = blockIdx.x, tid = threadIdx.x;
  cand_init(h);
  __syncthreads();
  unsigned long long negs = 0ull;
  for (int x = tid; x < X; x += 256) negs += slab_negs[(size_t)s * X + x];
  atomicAdd(&h.negs, negs);
  const double* src = slab + (size_t)s * X * K;
  const long long total = (long long)X * K;
  for (long long base = 0; base < total; base += 256 * 16) {
    double v[16];
    unsigned pend = 0u;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const long long e = base + i * 256 + tid;
      v[i] = e < total ? src[e] : -INFINITY;
      if (e < total) pend |= 1u << i;
    }
    cand_offer<kCap>(h, cv, v, pend, K);
  }
  __syncthreads();
  cand_cut<kCap>(h, cv, K);
  for (int i = tid; i < K; i += 256) topk[(size_t)s * K + i] = i < h.n ? cv[i] : -INFINITY;
  if (tid == 0) neg_count[s] = (long long)h.negs;
}

int ident_grid_x(int Q, int S) { return std::min(ceil_div(Q, 64), std::max(1, ceil_div(kTileWgs, S))); }

}  // namespace

size_t ident_workspace_bytes(int Q, int S, int K) {
  if (Q < 1 || S < 1 || K < 1) return 0;
  const size_t slabs = (size_t)ident_grid_x(Q, S) * S;
  return align_up((size_t)(S + 1) * sizeof(long long), 256) + align_up(slabs * sizeof(unsigned long long), 256) + slabs * K * sizeof(double);
}

int ident_topk(const float* query, const long long* qid, int Q, const float* gallery, const long long* gid, int G, int D,
               const long long* seg, int S, int K, double* pos, double* neg_topk, long long* neg_count, void* ws, size_t ws_bytes,
               hipStream_t st) {
  FEDFR_REQUIRE(query && qid && gallery && gid && seg && pos && neg_topk && neg_count, "ident_topk: null pointer");
  FEDFR_REQUIRE(Q > 0 && G > 0 && S > 0 && S <= 65535, "ident_topk: bad sizes (Q = %d, G = %d, S = %d)", Q, G, S);
  FEDFR_REQUIRE(D >= 1, "ident_topk: D = %d must be >= 1", D);
  FEDFR_REQUIRE(K >= 1 && K <= kMaxK, "ident_topk: K = %d outside [1, %d]", K, kMaxK);
  FEDFR_REQUIRE(seg[0] == 0 && seg[S] == G, "ident_topk: segments must start at column 0 and end at G = %d", G);
  for (int s = 0; s < S; ++s) FEDFR_REQUIRE(seg[s + 1] > seg[s], "ident_topk: segment %d is empty", s);
  const size_t need = ident_workspace_bytes(Q, S, K);
  FEDFR_REQUIRE(ws && ws_bytes >= need, "ident_topk: workspace of %zu bytes, %zu needed", ws_bytes, need);
  const int X = ident_grid_x(Q, S);
  char* w = static_cast<char*>(ws);
  long long* dseg = reinterpret_cast<long long*>(w);
  w += align_up((size_t)(S + 1) * sizeof(long long), 256);
  unsigned long long* slab_negs = reinterpret_cast<unsigned long long*>(w);
  w += align_up((size_t)X * S * sizeof(unsigned long long), 256);
  double* slab = reinterpret_cast<double*>(w);
  if (hipMemcpyAsync(dseg, seg, (size_t)(S + 1) * sizeof(long long), hipMemcpyHostToDevice, st) != hipSuccess ||
      hipMemsetAsync(pos, 0xff, (size_t)Q * sizeof(double), st) != hipSuccess) {           // all-ones bytes: NaN = "no positive"
    fedfr_set_error("ident_topk: %s", hipGetErrorString(hipGetLastError()));
    return FEDFR_ERR_HIP;
  }
  hipLaunchKernelGGL(ident_tile_kernel, dim3(X, S), dim3(256), 0, st, query, qid, Q, gallery, gid, D, dseg, K, pos, slab, slab_negs);
  FEDFR_LAUNCH_CHECK("ident_tile");
  hipLaunchKernelGGL(ident_merge_kernel, dim3(S), dim3(256), 0, st, slab, slab_negs, X, K, neg_topk, neg_count);
  FEDFR_LAUNCH_CHECK("ident_merge");
  return FEDFR_OK;
}
