// 1:N identification read-out (reference local_all.py:142-176 `evaluation`, driven per client by :274-297): one positive score per query
// and the exact top-K of the negative scores of every column segment (one segment per client gallery), the query x gallery similarity
// matrix never written to memory.
//
// ident_tile_kernel, grid (X, S): workgroup (x, s) walks the 64-row query tiles x, x + X, ... and, for each, the columns of segment s in
// 64-wide chunks.  A chunk is one 64 x 64 tile of v_mfma_f64_16x16x4_f64 on the fp32 features widened to fp64 (the K loop of
// roc_hist_kernel, head.hip): every score is the same fp64 number whichever workgroup computes it.  Epilogue: a positive pair (qid[q] >= 0
// and qid[q] == gid[c]) writes pos[q]; a negative that beats the workgroup's running K-th bound goes to an LDS candidate buffer, which a
// descending bitonic sort cuts back to K entries whenever it fills.  The workgroup ends with its sorted top-K (and its negative count) in a
// workspace slab; ident_merge_kernel (one workgroup per segment) runs the same buffer over the segment's X slabs.  The result is the top-K
// multiset itself (ties included) and no floating-point atomics are used: the output does not depend on the order workgroups run in.
#include <algorithm>
#include "head.h"

namespace {

constexpr int kMaxK = 1024;           // fedfr_ident_topk's K limit (FAR 1e-3 up to ~1M queries)
constexpr int kCap = 4096;            // LDS candidates per workgroup (32 KB); > kMaxK, so a cut always keeps room for new ones
constexpr int kTileWgs = 3072;        // tile-kernel workgroups over all segments: 256 CUs x 3 resident x 4 rounds
typedef __attribute__((ext_vector_type(4))) double f64x4_t;

struct Cand {
  double v[kCap];
  double thr;                         // a value <= thr cannot enter the top-K (K values >= thr are held)
  int n;                              // candidates written (may run past kCap while a chunk overflows)
  unsigned long long negs;
};

__device__ __forceinline__ void cand_init(Cand& c) {
  if (threadIdx.x == 0) {
    c.n = 0;
    c.thr = -INFINITY;
    c.negs = 0ull;
  }
}

// Sort c.v[0, n) descending (padded with -inf to a power of two >= 64), keep min(n, K) of it and raise thr to the K-th value.  Called by
// the whole workgroup after a barrier that follows the last write to c.
__device__ void cand_cut(Cand& c, int K) {
  const int tid = threadIdx.x;
  const int n = min(c.n, kCap);
  int n2 = 64;
  while (n2 < n) n2 <<= 1;
  for (int i = n + tid; i < n2; i += 256) c.v[i] = -INFINITY;
  __syncthreads();
  for (int k = 2; k <= n2; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < (n2 >> 1); i += 256) {
        const int lo = ((i & ~(j - 1)) << 1) | (i & (j - 1)), hi = lo + j;
        const double a = c.v[lo], b = c.v[hi];
        if ((lo & k) == 0 ? a < b : a > b) {
          c.v[lo] = b;
          c.v[hi] = a;
        }
      }
      __syncthreads();
    }
  if (tid == 0) {
    const int m = min(n, K);
    c.n = m;
    if (m == K) c.thr = c.v[K - 1];
  }
  __syncthreads();
}

// Offer this thread's values v[i] (bit i of pend set) to the buffer; every thread of the workgroup calls it (it holds barriers).  Values
// that find the buffer full stay pending across a cut.
template <int NV>
__device__ __forceinline__ void cand_offer(Cand& c, const double (&v)[NV], unsigned pend, int K) {
  for (;;) {
    const double thr = c.thr;
#pragma unroll
    for (int i = 0; i < NV; ++i)
      if ((pend >> i) & 1u) {
        if (v[i] > thr) {
          const int s = atomicAdd(&c.n, 1);
          if (s < kCap) {
            c.v[s] = v[i];
            pend &= ~(1u << i);
          }
        } else {
          pend &= ~(1u << i);
        }
      }
    if (!__syncthreads_or(pend != 0u)) return;
    cand_cut(c, K);
  }
}

__global__ __launch_bounds__(256) void ident_tile_kernel(const float* __restrict__ query, const long long* __restrict__ qid, int Q,
                                                         const float* __restrict__ gallery, const long long* __restrict__ gid, int D,
                                                         const long long* __restrict__ seg, int K, double* __restrict__ pos,
                                                         double* __restrict__ slab, unsigned long long* __restrict__ slab_negs) {
  constexpr int BK = 16, LD = 80;
  __shared__ float sA[2][BK][LD], sB[2][BK][LD];
  __shared__ Cand c;
  const int s = blockIdx.y, X = gridDim.x;
  const int c_beg = (int)seg[s], c_end = (int)seg[s + 1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, l15 = lane & 15, lg = lane >> 4;
  cand_init(c);
  __syncthreads();
  unsigned long long negs = 0ull;
  const int ntile = ceil_div(Q, 64), nk = ceil_div(D, BK);
  for (int t = blockIdx.x; t < ntile; t += X) {
    const int a0 = t * 64;
    for (int b0 = c_beg; b0 < c_end; b0 += 64) {
      float ra[4], rb[4];
      auto load = [&](int k0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int e = tid + 256 * i, k = e & 15, m = e >> 4;
          const int ga = a0 + m, gb = b0 + m, gk = k0 + k;
          ra[i] = (ga < Q && gk < D) ? query[(size_t)ga * D + gk] : 0.f;
          rb[i] = (gb < c_end && gk < D) ? gallery[(size_t)gb * D + gk] : 0.f;
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
      load(0);
      store(0);                       // the previous chunk's K loop ended on a barrier after its last LDS read
      __syncthreads();
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
      double v[16];
      unsigned pend = 0u;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int b = b0 + wn * 32 + j * 16 + l15;
        const long long gb = b < c_end ? gid[b] : -1;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int a = a0 + wm * 32 + i * 16 + q * 4 + lg, r = (j * 2 + i) * 4 + q;
            v[r] = acc[i][j][q];
            if (a < Q && b < c_end) {
              const long long qa = qid[a];
              if (qa >= 0 && qa == gb) {
                pos[a] = v[r];
              } else {
                ++negs;
                pend |= 1u << r;
              }
            }
          }
      }
      cand_offer(c, v, pend, K);
    }
  }
  atomicAdd(&c.negs, negs);
  __syncthreads();
  cand_cut(c, K);
  const size_t o = (size_t)s * X + blockIdx.x;
  for (int i = tid; i < K; i += 256) slab[o * K + i] = i < c.n ? c.v[i] : -INFINITY;
  if (tid == 0) slab_negs[o] = c.negs;
}

// segment s: the top-K of its X sorted slabs (-inf entries are padding and never enter) and the sum of their negative counts
__global__ __launch_bounds__(256) void ident_merge_kernel(const double* __restrict__ slab, const unsigned long long* __restrict__ slab_negs,
                                                          int X, int K, double* __restrict__ topk, long long* __restrict__ neg_count) {
  __shared__ Cand c;
  const int s = blockIdx.x, tid = threadIdx.x;
  cand_init(c);
  __syncthreads();
  unsigned long long negs = 0ull;
  for (int x = tid; x < X; x += 256) negs += slab_negs[(size_t)s * X + x];
  atomicAdd(&c.negs, negs);
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
    cand_offer(c, v, pend, K);
  }
  __syncthreads();
  cand_cut(c, K);
  for (int i = tid; i < K; i += 256) topk[(size_t)s * K + i] = i < c.n ? c.v[i] : -INFINITY;
  if (tid == 0) neg_count[s] = (long long)c.negs;
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
