// Spread-out regulariser of the class centres (reference server.py:48-63 SpreadOut_Module.forward and its autograd backward), fused:
//   S = Fn Fn^T,  H_ij = max(S_ij - margin, 0) for i != j, H_ii = 0,  loss = c * sum_ij H_ij^2,  dFn = 4c * H Fn
// on row-normalised Fn [N][D] fp32, c = 1 ('sum') or 1 / (N (N - 1)) ('mean').  S and H are never written to memory: N = 85 000 would be 29 GB.
//
// spreadout_tile_kernel: workgroup b owns rows [64 b, 64 b + 64) of dFn and walks the 64-column tiles of S in ascending order.
//   First product: the 64 x 64 x D tile of tile64.h with fp32 accumulation (sgemm's exact fp32 FMA chain over k ascending, BK = 16), both
//   operands read from Fn with 16-byte loads and this kernel's own thread-to-element map.
//   Epilogue on the accumulators: hinge, diagonal and out-of-range entries zeroed by global index, sum h^2 (fp64 per lane) and the count of
//   S_ij > margin.  A tile with no active element (workgroup-uniform: __syncthreads_or) ends there: at margin 0.4 that is almost every tile.
//   Second product, active tiles only: the hinge tile goes to LDS (pitch 66: the A-fragment read of 16 rows x 2 k lands on 32 banks) with a
//   4-bit mask of the 16-row groups and a 16-bit mask of the 4-column groups that hold an active element; wave w owns the 16-wide column
//   chunks w, w + 4, ... of D and adds H_tile * Fn_J to its part of dFn with the hinge tile as the MFMA A operand, only over the marked row
//   groups and k groups (the others are exact zeros).  The running sum lives in dFn itself: every element is read and written by the one lane
//   that owns it (a fixed map), so program order alone orders it, the rows stay in the L2 between two active tiles, and D up to 1024 needs
//   no more registers than D = 4.  A row group that never met an active tile is never read: it is stored as zeros at the end, where the
//   touched ones are scaled by 4c.
// spreadout_reduce_kernel: one workgroup adds the per-row-block fp64 loss partials and counts in a fixed order.
// No floating-point atomics; every dFn element is accumulated by one owner over ascending column tiles: two launches are bit-identical.
#include "head.h"
#include "tile64.h"

namespace {

constexpr int BM = 64, BN = 64, BK = 16;
constexpr int HP = 66;                                 // pitch of the hinge tile in floats
constexpr int kMaxD = 1024;

__global__ __launch_bounds__(256) void spreadout_tile_kernel(const float* __restrict__ fn, int N, int D, float margin, float scale,
                                                             float* dfn, double* __restrict__ part_loss,
                                                             long long* __restrict__ part_active) {
  __shared__ tile64::Lds<BK> t;
  __shared__ float sH[BM * HP];
  __shared__ unsigned sMask[2];                        // [0]: 16-row groups, [1]: 4-column groups of the hinge tile with an active element
  __shared__ double sLoss[4];
  __shared__ long long sCnt[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = tile64::l15(), lg = tile64::lg();
  const int i0 = blockIdx.x * BM;
  const int lm = tid >> 2, lk = (tid & 3) * 4;         // this thread's 16-byte piece of a 64 x 16 operand tile: row lm, k lk .. lk + 3
  const int nchunk = ceil_div(D, 16);
  if (tid < 2) sMask[tid] = 0u;
  double loss = 0.0;
  long long cnt = 0;
  unsigned touched = 0u;                               // row groups of this block whose dFn rows hold a running sum (workgroup-uniform)

  for (int j0 = 0; j0 < N; j0 += BN) {
    float4 ra, rb;
    auto load = [&](int k0) {
      const int gk = k0 + lk;                          // D % 4 == 0: a piece is inside the row or past its end as a whole
      ra = (i0 + lm < N && gk < D) ? *reinterpret_cast<const float4*>(fn + (size_t)(i0 + lm) * D + gk) : make_float4(0.f, 0.f, 0.f, 0.f);
      rb = (j0 + lm < N && gk < D) ? *reinterpret_cast<const float4*>(fn + (size_t)(j0 + lm) * D + gk) : make_float4(0.f, 0.f, 0.f, 0.f);
    };
    auto store = [&](int buf) {
      const float va[4] = {ra.x, ra.y, ra.z, ra.w}, vb[4] = {rb.x, rb.y, rb.z, rb.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        t.put(0, buf, lk + e, lm, va[e]);
        t.put(1, buf, lk + e, lm, vb[e]);
      }
    };
    f32x4_t acc[2][2];
    tile64::zero(acc);
    tile64::k_loop<BK>(t, acc, 0, D, load, store);     // the previous tile ended on a barrier after its last LDS read
    auto hinge = [&](int m, int n, float sv, bool& on) {   // H of element (m, n) of the tile; diagonal and out-of-range entries by global index
      on = i0 + m < N && j0 + n < N && i0 + m != j0 + n && sv > margin;
      return on ? sv - margin : 0.f;
    };
    unsigned rmask = 0u, kmask = 0u;
    tile64::for_each(acc, [&](int m, int n, float sv) {
      bool on;
      const float h = hinge(m, n, sv, on);
      if (on) {
        loss += (double)h * (double)h;
        ++cnt;
        rmask |= 1u << (m >> 4);
        kmask |= 1u << (n >> 2);
      }
    });
    if (!__syncthreads_or(rmask != 0u)) continue;
    if (rmask) {
      atomicOr(&sMask[0], rmask);
      atomicOr(&sMask[1], kmask);
    }
    tile64::for_each(acc, [&](int m, int n, float sv) {
      bool on;
      sH[m * HP + n] = hinge(m, n, sv, on);
    });
    __syncthreads();
    const unsigned rows = sMask[0], ks = sMask[1];
    for (int c = wave; c < nchunk; c += 4) {
      const int d = c * 16 + l15;
      const bool dok = d < D;
      float fb[16];
#pragma unroll
      for (int g = 0; g < 16; ++g) {
        const int j = j0 + g * 4 + lg;
        fb[g] = ((ks >> g) & 1u) && dok && j < N ? fn[(size_t)j * D + d] : 0.f;
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (!((rows >> r) & 1u)) continue;
        f32x4_t o = (f32x4_t){0.f, 0.f, 0.f, 0.f};
        if ((touched >> r) & 1u) {
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int m = i0 + r * 16 + lg * 4 + q;
            if (m < N && dok) o[q] = dfn[(size_t)m * D + d];
          }
        }
#pragma unroll
        for (int g = 0; g < 16; ++g)
          if ((ks >> g) & 1u) o = __builtin_amdgcn_mfma_f32_16x16x4f32(sH[(r * 16 + l15) * HP + g * 4 + lg], fb[g], o, 0, 0, 0);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int m = i0 + r * 16 + lg * 4 + q;
          if (m < N && dok) dfn[(size_t)m * D + d] = o[q];
        }
      }
    }
    touched |= rows;
    __syncthreads();
    if (tid < 2) sMask[tid] = 0u;                      // next atomicOr comes after the barriers of the next tile's K loop
  }

  // dFn = 4c * running sum; rows that met no active tile were never written
  for (int c = wave; c < nchunk; c += 4) {
    const int d = c * 16 + l15;
    if (d >= D) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int m = i0 + r * 16 + lg * 4 + q;
        if (m < N) {
          float* p = dfn + (size_t)m * D + d;
          *p = ((touched >> r) & 1u) ? scale * *p : 0.f;
        }
      }
  }
  loss = wave_sum_d(loss);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
  if (lane == 0) {
    sLoss[wave] = loss;
    sCnt[wave] = cnt;
  }
  __syncthreads();
  if (tid == 0) {
    part_loss[blockIdx.x] = ((sLoss[0] + sLoss[1]) + sLoss[2]) + sLoss[3];
    part_active[blockIdx.x] = sCnt[0] + sCnt[1] + sCnt[2] + sCnt[3];
  }
}

__global__ __launch_bounds__(256) void spreadout_reduce_kernel(const double* __restrict__ part_loss, const long long* __restrict__ part_active,
                                                               int nb, double c, float* __restrict__ loss, long long* __restrict__ active) {
  __shared__ double sL[256];
  __shared__ long long sC[256];
  const int tid = threadIdx.x;
  double l = 0.0;
  long long n = 0;
  for (int i = tid; i < nb; i += 256) {
    l += part_loss[i];
    n += part_active[i];
  }
  sL[tid] = l;
  sC[tid] = n;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) {
      sL[tid] += sL[tid + s];
      sC[tid] += sC[tid + s];
    }
    __syncthreads();
  }
  if (tid == 0) {
    *loss = (float)(c * sL[0]);
    if (active) *active = sC[0];
  }
}

}  // namespace

size_t spreadout_workspace_bytes(int N, int D) {
  if (N < 2 || D < 4 || D > kMaxD || D % 4) return 0;
  return align_up((size_t)ceil_div(N, BM) * sizeof(double), 256) + (size_t)ceil_div(N, BM) * sizeof(long long);
}

int spreadout_grad(const float* fn, int N, int D, float margin, int mean, float* dfn, float* loss, long long* active, void* ws, size_t ws_bytes,
                   hipStream_t st) {
  FEDFR_REQUIRE(fn && dfn && loss, "spreadout_grad: null pointer");
  FEDFR_REQUIRE(N >= 2, "spreadout_grad: N = %d must be >= 2", N);
  FEDFR_REQUIRE(D >= 4 && D <= kMaxD && D % 4 == 0, "spreadout_grad: D = %d must be a multiple of 4 in [4, %d]", D, kMaxD);
  FEDFR_REQUIRE(mean == 0 || mean == 1, "spreadout_grad: mean = %d must be 0 (sum) or 1 (mean)", mean);
  const size_t need = spreadout_workspace_bytes(N, D);
  if (!ws || ws_bytes < need) {
    fedfr_set_error("spreadout_grad: workspace of %zu bytes, %zu needed", ws ? ws_bytes : (size_t)0, need);
    return FEDFR_ERR_WORKSPACE;
  }
  const int nb = ceil_div(N, BM);
  double* part_loss = static_cast<double*>(ws);
  long long* part_active = reinterpret_cast<long long*>(static_cast<char*>(ws) + align_up((size_t)nb * sizeof(double), 256));
  const double c = mean ? 1.0 / ((double)N * (double)(N - 1)) : 1.0;
  hipLaunchKernelGGL(spreadout_tile_kernel, dim3(nb), dim3(256), 0, st, fn, N, D, margin, (float)(4.0 * c), dfn, part_loss, part_active);
  FEDFR_LAUNCH_CHECK("spreadout_tile");
  hipLaunchKernelGGL(spreadout_reduce_kernel, dim3(1), dim3(256), 0, st, part_loss, part_active, nb, c, loss, active);
  FEDFR_LAUNCH_CHECK("spreadout_reduce");
  return FEDFR_OK;
}
