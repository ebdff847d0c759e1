// BottleBlock converter of the personalised head (reference backbones/bottle.py, client.py:25-36 with converter_layer != 1), fp32:
//   h1_g = leaky(x W1_g^T + b1_g)   W1_g [H][D], H = D / 4, g = 0..3
//   h2_g = leaky(h1_g W2_g^T + b2_g) W2_g [H][H]
//   y    = x + [h2_0|h2_1|h2_2|h2_3] W3^T + b3,  W3 [D][D]
// h1 and h2 are stored [B][D] with branch g in columns g H .. (g + 1) H (the concatenation W3 consumes); the pre-activations never are:
// slope 0.01 > 0, so h > 0 exactly when z > 0 and the backward takes leaky' from the sign of the stored activation (0.01 at 0, as torch).
//
// Two launches forward, two backward.  Every kernel is built from ONE masked 64x64 tile GEMM: the tile of tile64.h with fp32 accumulation (the
// k-ordered exact fp32 FMA chain of head.hip's sgemm); the block is launch-bound (1.18 MFLOP per row), so what matters is the launch count:
//   fwd 1  grid (row tiles, 4 branches): h1_g tile, barrier, h2_g tile from the block's own h1_g rows
//   fwd 2  grid (D / 64, row tiles):     y
//   bwd 1  grid (row tiles, 4 branches): dz2_g = (dy W3[:, g]) * leaky'(h2_g), barrier, dz1_g = (dz2_g W2_g) * leaky'(h1_g) -> workspace
//   bwd 2  one grid over the tiles of dW3, the four dW2_g, the four dW1_g (K = the whole batch in one workgroup, ascending: no cross-
//          workgroup sum, no atomics; the tile of column block 0 also sums its bias gradient in a fixed order) and of dx = dy + dz1 W1
// Parameters and gradients stay the 18 separate tensors: br1..br4 x (W1, b1, W2, b2), then W3, b3.
#include "head.h"
#include "tile64.h"

namespace {
constexpr int BK = 32;
constexpr float SLOPE = 0.01f;                    // nn.LeakyReLU()
using Smem = tile64::Lds<BK>;
using tile64::zero;

struct BottleP {
  const float* x;
  const float* dy;
  float* h1;
  float* h2;
  float* y;
  float* dz1;
  float* dz2;
  float* dx;
  const float* w[18];
  float* g[18];
  int B, D, H;
};

// acc[m][n] += sum_{k < K} A[m * sam + k * sak] * B[k * sbk + n * sbn] for m < min(64, mrem), n < min(64, nrem); rows and columns past the
// limits read as 0.  Every thread of the block calls it; on return all waves are past the last read of the LDS tiles.
__device__ __forceinline__ void tile_gemm(Smem& s, f32x4_t (&acc)[2][2], const float* A, long long sam, long long sak, int mrem, const float* B,
                                          long long sbk, long long sbn, int nrem, int K) {
  const bool akf = sak == 1, bkf = sbn != 1;      // which operand is k-fastest in memory (uniform)
  float ra[BK / 4], rb[BK / 4];
  auto load = [&](int k0) {
    tile64::load<BK>(ra, akf, [&](int m, int k, int) { return (m < mrem && k0 + k < K) ? A[m * sam + (k0 + k) * sak] : 0.f; });
    tile64::load<BK>(rb, bkf, [&](int n, int k, int) { return (n < nrem && k0 + k < K) ? B[(k0 + k) * sbk + n * sbn] : 0.f; });
  };
  auto store = [&](int buf) {
    tile64::store(s, 0, buf, akf, ra);
    tile64::store(s, 1, buf, bkf, rb);
  };
  tile64::k_loop<BK>(s, acc, 0, K, load, store);
}

// f(m, n, v) for every accumulator element of the tile inside the limits
template <class F>
__device__ __forceinline__ void for_each(const f32x4_t (&acc)[2][2], int mrem, int nrem, F f) {
  tile64::for_each(acc, [&](int m, int n, float v) {
    if (m < mrem && n < nrem) f(m, n, v);
  });
}

__device__ __forceinline__ float leaky(float z) { return z > 0.f ? z : SLOPE * z; }
__device__ __forceinline__ float dleaky(float h) { return h > 0.f ? 1.f : SLOPE; }

// ---- forward 1: h1_g and h2_g of one row tile --------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void bottle_fwd_branch_kernel(BottleP p) {
  __shared__ Smem s;
  const int g = blockIdx.y, D = p.D, H = p.H, m0 = blockIdx.x * 64, mrem = p.B - m0;
  const float *w1 = p.w[4 * g], *b1 = p.w[4 * g + 1], *w2 = p.w[4 * g + 2], *b2 = p.w[4 * g + 3];
  const size_t row0 = (size_t)m0 * D + (size_t)g * H;          // (first row of the tile, first column of branch g) in h1 / h2
  f32x4_t acc[2][2];
#pragma unroll 1
  for (int n0 = 0; n0 < H; n0 += 64) {
    zero(acc);
    tile_gemm(s, acc, p.x + (size_t)m0 * D, D, 1, mrem, w1 + (size_t)n0 * D, 1, D, H - n0, D);
    for_each(acc, mrem, H - n0, [&](int m, int n, float v) { p.h1[row0 + (size_t)m * D + n0 + n] = leaky(v + b1[n0 + n]); });
  }
  __syncthreads();                                             // the block's own h1 rows, written above, are the next A operand
#pragma unroll 1
  for (int n0 = 0; n0 < H; n0 += 64) {
    zero(acc);
    tile_gemm(s, acc, p.h1 + row0, D, 1, mrem, w2 + (size_t)n0 * H, 1, H, H - n0, H);
    for_each(acc, mrem, H - n0, [&](int m, int n, float v) { p.h2[row0 + (size_t)m * D + n0 + n] = leaky(v + b2[n0 + n]); });
  }
}

// ---- forward 2: y = x + h2 W3^T + b3 -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void bottle_fwd_out_kernel(BottleP p) {
  __shared__ Smem s;
  const int D = p.D, n0 = blockIdx.x * 64, m0 = blockIdx.y * 64, mrem = p.B - m0;
  const float *w3 = p.w[16], *b3 = p.w[17];
  f32x4_t acc[2][2];
  zero(acc);
  tile_gemm(s, acc, p.h2 + (size_t)m0 * D, D, 1, mrem, w3 + (size_t)n0 * D, 1, D, D - n0, D);
  for_each(acc, mrem, D - n0, [&](int m, int n, float v) {
    const size_t o = (size_t)(m0 + m) * D + n0 + n;
    p.y[o] = p.x[o] + (v + b3[n0 + n]);
  });
}

// ---- backward 1: dz2_g and dz1_g of one row tile ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void bottle_bwd_branch_kernel(BottleP p) {
  __shared__ Smem s;
  const int g = blockIdx.y, D = p.D, H = p.H, m0 = blockIdx.x * 64, mrem = p.B - m0;
  const float *w2 = p.w[4 * g + 2], *w3 = p.w[16];
  const size_t row0 = (size_t)m0 * D + (size_t)g * H;
  f32x4_t acc[2][2];
#pragma unroll 1
  for (int n0 = 0; n0 < H; n0 += 64) {                         // d concat[:, g] = dy W3[:, g H ..]
    zero(acc);
    tile_gemm(s, acc, p.dy + (size_t)m0 * D, D, 1, mrem, w3 + (size_t)g * H + n0, D, 1, H - n0, D);
    for_each(acc, mrem, H - n0, [&](int m, int n, float v) {
      const size_t o = row0 + (size_t)m * D + n0 + n;
      p.dz2[o] = v * dleaky(p.h2[o]);
    });
  }
  __syncthreads();                                             // the block's own dz2 rows are the next A operand
#pragma unroll 1
  for (int n0 = 0; n0 < H; n0 += 64) {                         // d h1_g = dz2_g W2_g
    zero(acc);
    tile_gemm(s, acc, p.dz2 + row0, D, 1, mrem, w2 + n0, H, 1, H - n0, H);
    for_each(acc, mrem, H - n0, [&](int m, int n, float v) {
      const size_t o = row0 + (size_t)m * D + n0 + n;
      p.dz1[o] = v * dleaky(p.h1[o]);
    });
  }
}

// ---- backward 2: every weight-gradient tile (+ bias sums) and every dx tile in one grid -------------------------------------------------
// dW[o][i] = sum_b dO[b][co + o] * X[b][ci + i] (dO, X: [B][D] row-major), o < M, i < N; tile (ti, tj); db[o] = sum_b dO[b][co + o] by the
// tiles with tj == 0: four interleaved partial sums (b = q, q + 4, ...), added q ascending
__device__ __forceinline__ void wgrad_tile(Smem& s, const BottleP& p, const float* dO, const float* X, int M, int N, int ti, int tj,
                                           float* dW, int ldw, float* db) {
  const int D = p.D, mo = ti * 64, no = tj * 64;
  f32x4_t acc[2][2];
  zero(acc);
  tile_gemm(s, acc, dO + mo, 1, D, M - mo, X + no, D, 1, N - no, p.B);
  for_each(acc, M - mo, N - no, [&](int m, int n, float v) { dW[(size_t)(mo + m) * ldw + no + n] = v; });
  if (tj != 0) return;                                         // uniform over the block
  const int c = threadIdx.x & 63, q = threadIdx.x >> 6;
  float sum = 0.f;
  if (mo + c < M)
    for (int b = q; b < p.B; b += 4) sum += dO[(size_t)b * D + mo + c];
  s.t[0][0][q][c] = sum;                                       // tile_gemm has returned: the LDS tiles are free
  __syncthreads();
  if (q == 0 && mo + c < M) db[mo + c] = ((s.t[0][0][0][c] + s.t[0][0][1][c]) + s.t[0][0][2][c]) + s.t[0][0][3][c];
}

__global__ __launch_bounds__(256) void bottle_bwd_tiles_kernel(BottleP p) {
  __shared__ Smem s;
  const int D = p.D, H = p.H, nD = D / 64, nH = ceil_div(H, 64);
  int t = blockIdx.x;
  if (t < nD * nD) {                                           // dW3 = dy^T h2, db3
    wgrad_tile(s, p, p.dy, p.h2, D, D, t / nD, t % nD, p.g[16], D, p.g[17]);
    return;
  }
  t -= nD * nD;
  if (t < 4 * nH * nH) {                                       // dW2_g = dz2_g^T h1_g, db2_g
    const int g = t / (nH * nH), r = t % (nH * nH);
    wgrad_tile(s, p, p.dz2 + (size_t)g * H, p.h1 + (size_t)g * H, H, H, r / nH, r % nH, p.g[4 * g + 2], H, p.g[4 * g + 3]);
    return;
  }
  t -= 4 * nH * nH;
  if (t < 4 * nH * nD) {                                       // dW1_g = dz1_g^T x, db1_g
    const int g = t / (nH * nD), r = t % (nH * nD);
    wgrad_tile(s, p, p.dz1 + (size_t)g * H, p.x, H, D, r / nD, r % nD, p.g[4 * g], D, p.g[4 * g + 1]);
    return;
  }
  t -= 4 * nH * nD;                                            // dx = dy + sum_g dz1_g W1_g (the grid has these tiles only when dx != null)
  const int m0 = (t / nD) * 64, n0 = (t % nD) * 64, mrem = p.B - m0;
  f32x4_t acc[2][2];
  zero(acc);
#pragma unroll 1
  for (int g = 0; g < 4; ++g) tile_gemm(s, acc, p.dz1 + (size_t)m0 * D + (size_t)g * H, D, 1, mrem, p.w[4 * g] + n0, D, 1, D - n0, H);
  for_each(acc, mrem, D - n0, [&](int m, int n, float v) {
    const size_t o = (size_t)(m0 + m) * D + n0 + n;
    p.dx[o] = p.dy[o] + v;
  });
}

int check_shape(const char* what, int B, int D) {
  FEDFR_REQUIRE(B >= 1 && D >= 64 && D <= 512 && D % 64 == 0,
                "%s: B = %d, D = %d unsupported (B >= 1, D a multiple of 64 in [64, 512], bottle_rate 4)", what, B, D);
  return FEDFR_OK;
}
}  // namespace

size_t bottle_workspace_bytes(int B, int D) {
  if (B < 1 || D < 64 || D > 512 || D % 64 != 0) return 0;
  return (size_t)2 * B * D * sizeof(float);                    // dz1, dz2
}

int bottle_forward(const float* x, const float* const* params, int B, int D, float* h1, float* h2, float* y, hipStream_t st) {
  FEDFR_TRY(check_shape("bottle_forward", B, D));
  FEDFR_REQUIRE(x && params && h1 && h2 && y, "bottle_forward: null pointer");
  BottleP p{};
  p.x = x; p.h1 = h1; p.h2 = h2; p.y = y; p.B = B; p.D = D; p.H = D / 4;
  for (int i = 0; i < 18; ++i) {
    FEDFR_REQUIRE(params[i], "bottle_forward: params[%d] is null", i);
    p.w[i] = params[i];
  }
  const int rt = ceil_div(B, 64);
  hipLaunchKernelGGL(bottle_fwd_branch_kernel, dim3(rt, 4), dim3(256), 0, st, p);
  FEDFR_LAUNCH_CHECK("bottle_fwd_branch");
  hipLaunchKernelGGL(bottle_fwd_out_kernel, dim3(D / 64, rt), dim3(256), 0, st, p);
  FEDFR_LAUNCH_CHECK("bottle_fwd_out");
  return FEDFR_OK;
}

int bottle_backward(const float* x, const float* const* params, const float* h1, const float* h2, const float* dy, int B, int D, float* dx,
                    float* const* grads, void* ws, size_t ws_bytes, hipStream_t st) {
  FEDFR_TRY(check_shape("bottle_backward", B, D));
  FEDFR_REQUIRE(x && params && h1 && h2 && dy && grads && ws, "bottle_backward: null pointer");
  if (ws_bytes < bottle_workspace_bytes(B, D)) {
    fedfr_set_error("bottle_backward: workspace of %zu bytes, %zu needed", ws_bytes, bottle_workspace_bytes(B, D));
    return FEDFR_ERR_WORKSPACE;
  }
  BottleP p{};
  p.x = x; p.dy = dy; p.h1 = const_cast<float*>(h1); p.h2 = const_cast<float*>(h2); p.dx = dx; p.B = B; p.D = D; p.H = D / 4;
  p.dz1 = static_cast<float*>(ws);
  p.dz2 = p.dz1 + (size_t)B * D;
  for (int i = 0; i < 18; ++i) {
    FEDFR_REQUIRE(params[i] && grads[i], "bottle_backward: params[%d] or grads[%d] is null", i, i);
    p.w[i] = params[i];
    p.g[i] = grads[i];
  }
  const int rt = ceil_div(B, 64), nD = D / 64, nH = ceil_div(p.H, 64);
  hipLaunchKernelGGL(bottle_bwd_branch_kernel, dim3(rt, 4), dim3(256), 0, st, p);
  FEDFR_LAUNCH_CHECK("bottle_bwd_branch");
  const int tiles = nD * nD + 4 * nH * nH + 4 * nH * nD + (dx ? rt * nD : 0);
  hipLaunchKernelGGL(bottle_bwd_tiles_kernel, dim3(tiles), dim3(256), 0, st, p);
  FEDFR_LAUNCH_CHECK("bottle_bwd_tiles");
  return FEDFR_OK;
}
