// IJB-C job 1:N read-out (reference ijbc_all.py:367-427 `evaluation`): the fp64 form of ident.hip for one gallery.  Per query the score of
// its own gallery row (pos) and the number of other columns that score higher / equal (rank_gt / rank_eq: top-k hit iff rank_gt < k), and
// over all queries the exact top-K (K <= 4096) of the negative scores; the query x gallery matrix is never written to memory.
//
// ident64_tile_kernel<CAP>, CAP > 0 (sweep 1): a work item is a 64-row query tile x a group of 8 column chunks; workgroup x takes items
// x, x + X, ...  A chunk is one 64 x 64 tile of v_mfma_f64_16x16x4_f64 on fp64 operand tiles (its own LDS layout, below) under the pipeline,
// the MFMA step and the accumulator walk of tile64.h: k ascending in steps of 4, zero-padded to a multiple of 16, so a score is the same fp64
// number whichever workgroup computes it and, on fp32-representable features, the number ident.hip computes.  Epilogue as there: column
// mask[q] writes pos[q], every other score that beats the workgroup's running K-th bound goes to the LDS candidate buffer of topk_cand.h at
// CAP entries.  ident64_merge_kernel<CAP> runs the same buffer over the X sorted slabs.  CAP = 4096 for K <= 1024, 8192 (64 KiB) above.
// ident64_tile_kernel<0> (sweep 2) recomputes the tiles and counts each row's scores against the pos of sweep 1: 8 rows x 2 counters per
// lane, summed per item in LDS and added to rank_gt / rank_eq with integer atomics.  pos[q] is not known when sweep 1 meets the first
// columns of row q; keeping a per-row list of "maybe above" scores instead would need Q x (unbounded) storage for hard probes, so the
// ranks cost a second 2 Q G D flop: at IJB-C size 71 GFLOP, about a millisecond of the matrix cores.
// No floating-point atomics anywhere: every output is independent of the order workgroups run in.
//
// LDS (all of it dynamic, 16-byte aligned): operand tiles [2 buffers][64 rows][16 + 2 k] fp64 for A and B = 36 KiB; the row pitch of 18
// doubles puts the 32 lanes of a ds_read_b64 group (16 rows x 2 k) on 32 distinct bank pairs.  Sweep 1 adds the candidates: 68 KiB in all
// at CAP 4096 (2 workgroups per CU), 100 KiB at CAP 8192 (1 per CU); sweep 2 adds 512 B of counters (its 180 VGPRs allow 2 per CU).
#include <algorithm>
#include "head.h"
#include "tile64.h"
#include "topk_cand.h"

namespace {

constexpr int kMaxK = 4096;           // fedfr_ident_rank_topk's K limit: ceil(Q * 0.1) for up to 40 960 probes
constexpr int kChunks = 8;            // 64-column chunks per work item
constexpr int BK = 16, LDK = BK + 2;  // K step and LDS row pitch in doubles
constexpr int kTileBytes = 2 * 2 * 64 * LDK * (int)sizeof(double);
constexpr int kRankWgs = 1024;        // sweep 2: 256 CUs x 2 resident x 2 rounds

static_assert(sizeof(CandHdr) <= 32, "the candidates start 32 bytes after the header");

constexpr int cand_bytes(int cap) { return 32 + cap * (int)sizeof(double); }
constexpr int cap_for(int K) { return K <= 1024 ? 4096 : 8192; }                 // capacity well above K: a cut always leaves room
inline int topk_wgs(int K) { return K <= 1024 ? 512 : 256; }                     // sweep 1: 256 CUs x resident workgroups

// status bits: 1 = a non-finite score, 2 = a mask entry outside [-1, G)
__global__ __launch_bounds__(256) void ident64_init_kernel(const long long* __restrict__ mask, int Q, int G, double* __restrict__ pos,
                                                           int* __restrict__ rank_gt, int* __restrict__ rank_eq, int* __restrict__ status) {
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= Q) return;
  const long long m = mask[q];
  if (m < -1 || m >= G) atomicOr(status, 2);
  const int r = (m >= 0 && m < G) ? 0 : -1;
  pos[q] = __longlong_as_double(0x7ff8000000000000ll);        // NaN = "no positive"; sweep 1 overwrites the rows that have one
  rank_gt[q] = r;
  rank_eq[q] = r;
}

template <int CAP>
__global__ __launch_bounds__(256) void ident64_tile_kernel(const double* __restrict__ query, int Q, const double* __restrict__ gallery, int G,
                                                           int D, const long long* __restrict__ mask, int K, double* pos,
                                                           double* __restrict__ slab, unsigned long long* __restrict__ slab_negs,
                                                           int* __restrict__ rank_gt, int* __restrict__ rank_eq, int* __restrict__ status) {
  constexpr bool RANK = CAP == 0;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* sA = reinterpret_cast<double*>(smem);               // [2][64][LDK]
  double* sB = sA + 2 * 64 * LDK;
  CandHdr& h = *reinterpret_cast<CandHdr*>(smem + kTileBytes);
  double* cv = reinterpret_cast<double*>(smem + kTileBytes + 32);
  int* sCnt = reinterpret_cast<int*>(smem + kTileBytes);      // [64][2] (sweep 2)
  const int tid = threadIdx.x, wm = tile64::wm(), wn = tile64::wn(), l15 = tile64::l15(), lg = tile64::lg();
  if (RANK) {
    if (tid < 128) sCnt[tid] = 0;
  } else {
    cand_init(h);
  }
  __syncthreads();
  unsigned long long negs = 0ull;
  bool bad = false;
  const int ntile = ceil_div(Q, 64), ncg = ceil_div(G, 64 * kChunks);
  const long long items = (long long)ntile * ncg;
  for (long long w = blockIdx.x; w < items; w += gridDim.x) {
    const int a0 = (int)(w / ncg) * 64, c_beg = (int)(w % ncg) * 64 * kChunks, c_end = min(G, c_beg + 64 * kChunks);
    // this lane's 8 rows a0 + row_f64(i, q), kept at index i * 4 + q
    int ma[8];
    double pa[8];
    int gt[8], eq[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const int a = a0 + tile64::row_f64(r >> 2, r & 3);
      const long long m = a < Q ? mask[a] : -1;
      ma[r] = (m >= 0 && m < G) ? (int)m : -1;
      if (RANK) {
        pa[r] = a < Q ? pos[a] : 0.0;
        gt[r] = eq[r] = 0;
      }
    }
    for (int b0 = c_beg; b0 < c_end; b0 += 64) {
      double ra[4], rb[4];
      auto load = [&](int k0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int e = tid + 256 * i, k = e & 15, m = e >> 4;
          const int ga = a0 + m, gb = b0 + m, gk = k0 + k;
          ra[i] = (ga < Q && gk < D) ? query[(size_t)ga * D + gk] : 0.0;
          rb[i] = (gb < c_end && gk < D) ? gallery[(size_t)gb * D + gk] : 0.0;
        }
      };
      auto store = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int e = tid + 256 * i, k = e & 15, m = e >> 4;
          sA[(buf * 64 + m) * LDK + k] = ra[i];
          sB[(buf * 64 + m) * LDK + k] = rb[i];
        }
      };
      f64x4_t acc[2][2];
      tile64::zero(acc);
      // the previous chunk's K loop ended on a barrier after its last LDS read
      tile64::pipeline<BK>(0, D, load, store, [&](int buf) {
#pragma unroll
        for (int k4 = 0; k4 < BK; k4 += 4) {
          double fa[2], fb[2];
#pragma unroll
          for (int i = 0; i < 2; ++i) {
            fa[i] = sA[(buf * 64 + wm * 32 + i * 16 + l15) * LDK + k4 + lg];
            fb[i] = sB[(buf * 64 + wn * 32 + i * 16 + l15) * LDK + k4 + lg];
          }
          tile64::mma(fa, fb, acc);
        }
      });
      double v[16];
      unsigned pend = 0u;
      int r = 0;                      // position in the walk (order j, i, q): a constant once the walk is unrolled; r & 7 = i * 4 + q
      tile64::for_each(acc, [&](int m, int n, double x) {
        const int a = a0 + m, b = b0 + n, r8 = r & 7;
        v[r] = x;
        if (a < Q && b < c_end) {
          if (RANK) {
            if (ma[r8] >= 0 && ma[r8] != b) {
              gt[r8] += x > pa[r8] ? 1 : 0;
              eq[r8] += x == pa[r8] ? 1 : 0;
            }
          } else {
            if (!isfinite(x)) bad = true;
            if (ma[r8] == b) {
              pos[a] = x;
            } else {
              ++negs;
              pend |= 1u << r;
            }
          }
        }
        ++r;
      });
      if constexpr (!RANK) cand_offer<CAP>(h, cv, v, pend, K);
    }
    if (RANK) {
      // the item's counts: LDS sum over the 32 lanes that share a row, then one integer atomic per row and counter
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        const int row = tile64::row_f64(r >> 2, r & 3);
        if (gt[r]) atomicAdd(&sCnt[row * 2], gt[r]);
        if (eq[r]) atomicAdd(&sCnt[row * 2 + 1], eq[r]);
      }
      __syncthreads();
      if (tid < 128) {
        const int n = sCnt[tid], a = a0 + (tid >> 1);
        if (n && a < Q) atomicAdd((tid & 1) ? &rank_eq[a] : &rank_gt[a], n);
        sCnt[tid] = 0;
      }
      __syncthreads();
    }
  }
  if constexpr (!RANK) {
    if (bad) atomicOr(status, 1);
    atomicAdd(&h.negs, negs);
    __syncthreads();
    cand_cut<CAP>(h, cv, K);
    const size_t o = blockIdx.x;
    for (int i = tid; i < K; i += 256) slab[o * K + i] = i < h.n ? cv[i] : -INFINITY;
    if (tid == 0) slab_negs[o] = h.negs;
  }
}

// the top-K of the X sorted slabs (-inf entries are padding and never enter) and the sum of their negative counts
template <int CAP>
__global__ __launch_bounds__(256) void ident64_merge_kernel(const double* __restrict__ slab, const unsigned long long* __restrict__ slab_negs,
                                                            int X, int K, double* __restrict__ topk, long long* __restrict__ neg_count) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  CandHdr& h = *reinterpret_cast<CandHdr*>(smem);
  double* cv = reinterpret_cast<double*>(smem + 32);
  const int tid = threadIdx.x;
  cand_init(h);
  __syncthreads();
  unsigned long long negs = 0ull;
  for (int x = tid; x < X; x += 256) negs += slab_negs[x];
  atomicAdd(&h.negs, negs);
  const long long total = (long long)X * K;
  for (long long base = 0; base < total; base += 256 * 16) {
    double v[16];
    unsigned pend = 0u;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const long long e = base + i * 256 + tid;
      v[i] = e < total ? slab[e] : -INFINITY;
      if (e < total) pend |= 1u << i;
    }
    cand_offer<CAP>(h, cv, v, pend, K);
  }
  __syncthreads();
  cand_cut<CAP>(h, cv, K);
  for (int i = tid; i < K; i += 256) topk[i] = i < h.n ? cv[i] : -INFINITY;
  if (tid == 0) *neg_count = (long long)h.negs;
}

long long work_items(int Q, int G) { return (long long)ceil_div(Q, 64) * ceil_div(G, 64 * kChunks); }
int topk_grid(int Q, int G, int K) { return (int)std::min<long long>(work_items(Q, G), topk_wgs(K)); }

// the kernels ask for more than the default 64 KiB of dynamic LDS
void allow_big_lds() {
  static PerDeviceOnce attr_once;     // hipFuncSetAttribute is per device
  attr_once.run([&] {
    hipFuncSetAttribute(reinterpret_cast<const void*>(&ident64_tile_kernel<4096>), hipFuncAttributeMaxDynamicSharedMemorySize,
                        kTileBytes + cand_bytes(4096));
    hipFuncSetAttribute(reinterpret_cast<const void*>(&ident64_tile_kernel<8192>), hipFuncAttributeMaxDynamicSharedMemorySize,
                        kTileBytes + cand_bytes(8192));
    hipFuncSetAttribute(reinterpret_cast<const void*>(&ident64_merge_kernel<8192>), hipFuncAttributeMaxDynamicSharedMemorySize,
                        cand_bytes(8192));
  });
}

}  // namespace

size_t ident_rank_workspace_bytes(int Q, int G, int K) {
  if (Q < 1 || G < 1 || K < 1 || K > kMaxK) return 0;
  const size_t X = topk_grid(Q, G, K);
  return align_up(X * sizeof(unsigned long long), 256) + X * K * sizeof(double);
}

int ident_rank_topk(const double* query, int Q, const double* gallery, int G, int D, const long long* mask, int K, double* pos,
                    double* neg_topk, long long* neg_count, int* rank_gt, int* rank_eq, void* ws, size_t ws_bytes, int* status,
                    hipStream_t st) {
  FEDFR_REQUIRE(query && gallery && mask && pos && neg_topk && neg_count && rank_gt && rank_eq && status, "ident_rank_topk: null pointer");
  FEDFR_REQUIRE(Q > 0 && G > 0, "ident_rank_topk: bad sizes (Q = %d, G = %d)", Q, G);
  FEDFR_REQUIRE(D >= 1, "ident_rank_topk: D = %d must be >= 1", D);
  FEDFR_REQUIRE(K >= 1 && K <= kMaxK, "ident_rank_topk: K = %d outside [1, %d]", K, kMaxK);
  const size_t need = ident_rank_workspace_bytes(Q, G, K);
  FEDFR_REQUIRE(ws && ws_bytes >= need, "ident_rank_topk: workspace of %zu bytes, %zu needed", ws_bytes, need);
  const int X = topk_grid(Q, G, K);
  char* w = static_cast<char*>(ws);
  unsigned long long* slab_negs = reinterpret_cast<unsigned long long*>(w);
  double* slab = reinterpret_cast<double*>(w + align_up((size_t)X * sizeof(unsigned long long), 256));
  allow_big_lds();
  hipLaunchKernelGGL(ident64_init_kernel, dim3(ceil_div(Q, 256)), dim3(256), 0, st, mask, Q, G, pos, rank_gt, rank_eq, status);
  FEDFR_LAUNCH_CHECK("ident64_init");
  if (cap_for(K) == 4096) {
    hipLaunchKernelGGL(ident64_tile_kernel<4096>, dim3(X), dim3(256), kTileBytes + cand_bytes(4096), st, query, Q, gallery, G, D, mask, K, pos,
                       slab, slab_negs, rank_gt, rank_eq, status);
    FEDFR_LAUNCH_CHECK("ident64_tile");
    hipLaunchKernelGGL(ident64_merge_kernel<4096>, dim3(1), dim3(256), cand_bytes(4096), st, slab, slab_negs, X, K, neg_topk, neg_count);
  } else {
    hipLaunchKernelGGL(ident64_tile_kernel<8192>, dim3(X), dim3(256), kTileBytes + cand_bytes(8192), st, query, Q, gallery, G, D, mask, K, pos,
                       slab, slab_negs, rank_gt, rank_eq, status);
    FEDFR_LAUNCH_CHECK("ident64_tile");
    hipLaunchKernelGGL(ident64_merge_kernel<8192>, dim3(1), dim3(256), cand_bytes(8192), st, slab, slab_negs, X, K, neg_topk, neg_count);
  }
  FEDFR_LAUNCH_CHECK("ident64_merge");
  const int R = (int)std::min<long long>(work_items(Q, G), kRankWgs);
  hipLaunchKernelGGL(ident64_tile_kernel<0>, dim3(R), dim3(256), kTileBytes + 512, st, query, Q, gallery, G, D, mask, K, pos, slab, slab_negs,
                     rank_gt, rank_eq, status);
  FEDFR_LAUNCH_CHECK("ident64_rank");
  return FEDFR_OK;
}
