// The project's one 64 x 64 tile of the float-operand GEMM on the 16x16x4 MFMAs: a 256-thread workgroup, 2 x 2 waves of 32 x 32, operands staged
// k-major through double-buffered LDS, k ascending in steps of 4 (fp32 accumulation: one exact fp32 FMA chain per element; fp64 accumulation
// of the operands widened exactly: the same fp64 number in every kernel that uses this header).  Device-only, everything inlined; the caller
// supplies the global fetch and the epilogue.  Users: sgemm_kernel and roc_hist_kernel (head.hip), roc_hist_groups_kernel, ident_tile_kernel,
// spreadout_tile_kernel (first product), the bottle kernels; ident64.hip takes the pipeline and the fp64 walk around its own fp64 operand tiles.
#pragma once
#include "common.h"

namespace tile64 {

constexpr int LD = 80;                // LDS row pitch in floats

// Operand tiles [A / B][buffer][k][m].  Element (k, m) sits at column m ^ ((k >> 1) << 1).  LD % 32 == 16 puts rows k and k + 1 on the two
// halves of the 32 banks and the XOR moves every further row pair by two banks: the 64 lanes of a fragment read (16 m x 4 k) and the 64 lanes
// of either store map (16 k x 4 m, or 64 m of one k) fall on distinct banks within each 32-lane service group: no conflicts.
template <int BK>
struct Lds {
  float t[2][2][BK][LD];
  __device__ __forceinline__ void put(int op, int buf, int k, int m, float v) { t[op][buf][k][m ^ ((k >> 1) << 1)] = v; }
  __device__ __forceinline__ float get(int op, int buf, int k, int m) const { return t[op][buf][k][m ^ ((k >> 1) << 1)]; }
};

// this thread's place in the 2 x 2 wave grid and in its wave's 16 x 4 MFMA lane grid
__device__ __forceinline__ int wm() { return (int)threadIdx.x >> 7; }
__device__ __forceinline__ int wn() { return ((int)threadIdx.x >> 6) & 1; }
__device__ __forceinline__ int l15() { return (int)threadIdx.x & 15; }
__device__ __forceinline__ int lg() { return ((int)threadIdx.x & 63) >> 4; }

// ---- operand staging: the 64 x BK elements of one operand stage, BK / 4 per thread, slot i of thread tid is element e = tid + 256 i ----------
// kfast (memory is k-fastest): k = e % BK, m = e / BK; otherwise m = e % 64, k = e / 64.  A uniform runtime branch where the caller's flag is one.
template <int BK>
__device__ __forceinline__ void elem(bool kfast, int i, int& m, int& k) {
  const int e = (int)threadIdx.x + 256 * i;
  if (kfast) { k = e & (BK - 1); m = e / BK; } else { m = e & 63; k = e >> 6; }
}
// r[i] = fetch(m, k, i): the caller masks and addresses (m, k are tile-local, k within the stage)
template <int BK, class F>
__device__ __forceinline__ void load(float (&r)[BK / 4], bool kfast, F fetch) {
#pragma unroll
  for (int i = 0; i < BK / 4; ++i) {
    int m, k;
    elem<BK>(kfast, i, m, k);
    r[i] = fetch(m, k, i);
  }
}
template <int BK>
__device__ __forceinline__ void store(Lds<BK>& s, int op, int buf, bool kfast, const float (&r)[BK / 4]) {
#pragma unroll
  for (int i = 0; i < BK / 4; ++i) {
    int m, k;
    elem<BK>(kfast, i, m, k);
    s.put(op, buf, k, m, r[i]);
  }
}

// ---- one BK stage of MFMAs, k ascending --------------------------------------------------------------------------------------------------
__device__ __forceinline__ void zero(f32x4_t (&acc)[2][2]) {
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
}
__device__ __forceinline__ void zero(f64x4_t (&acc)[2][2]) {
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = (f64x4_t){0.0, 0.0, 0.0, 0.0};
}
__device__ __forceinline__ void mma(const float (&fa)[2], const float (&fb)[2], f32x4_t (&acc)[2][2]) {
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[i], fb[j], acc[i][j], 0, 0, 0);
}
__device__ __forceinline__ void mma(const double (&fa)[2], const double (&fb)[2], f64x4_t (&acc)[2][2]) {
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[i], fb[j], acc[i][j], 0, 0, 0);
}
// fp32 accumulation
template <int BK>
__device__ __forceinline__ void mma_stage(const Lds<BK>& s, int buf, f32x4_t (&acc)[2][2]) {
#pragma unroll
  for (int k4 = 0; k4 < BK; k4 += 4) {
    float fa[2], fb[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      fa[i] = s.get(0, buf, k4 + lg(), wm() * 32 + i * 16 + l15());
      fb[i] = s.get(1, buf, k4 + lg(), wn() * 32 + i * 16 + l15());
    }
    mma(fa, fb, acc);
  }
}
// fp64 accumulation of the float fragments, widened (exactly) as they leave LDS
template <int BK>
__device__ __forceinline__ void mma_stage(const Lds<BK>& s, int buf, f64x4_t (&acc)[2][2]) {
#pragma unroll
  for (int k4 = 0; k4 < BK; k4 += 4) {
    double fa[2], fb[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      fa[i] = (double)s.get(0, buf, k4 + lg(), wm() * 32 + i * 16 + l15());
      fb[i] = (double)s.get(1, buf, k4 + lg(), wn() * 32 + i * 16 + l15());
    }
    mma(fa, fb, acc);
  }
}

// ---- the pipelined K loop over [kbeg, kend) in stages of BK: ld(k0) fetches stage k0 into the caller's registers, st(buf) writes them to LDS
// buffer buf, step(buf) issues the stage's MFMAs.  Every thread of the workgroup calls it; it ends on a barrier behind the last LDS read, so the
// next call may store at once.
template <int BK, class Load, class Store, class Step>
__device__ __forceinline__ void pipeline(int kbeg, int kend, Load ld, Store st, Step step) {
  const int nk = ceil_div(kend - kbeg, BK);
  ld(kbeg);
  st(0);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int buf = kt & 1;
    if (kt + 1 < nk) ld(kbeg + (kt + 1) * BK);
    step(buf);
    if (kt + 1 < nk) st(buf ^ 1);
    __syncthreads();
  }
}
template <int BK, class Acc, class Load, class Store>
__device__ __forceinline__ void k_loop(const Lds<BK>& s, Acc (&acc)[2][2], int kbeg, int kend, Load ld, Store st) {
  pipeline<BK>(kbeg, kend, ld, st, [&](int buf) { mma_stage(s, buf, acc); });
}

// ---- accumulator layouts: element q of block (i, j) of this lane is D[row(i, q)][col(j)] of the 64 x 64 tile --------------------------------
// fp32 16x16x4: register q of lane l holds D[row = 4 (l >> 4) + q][col = l & 15]
__device__ __forceinline__ int row_f32(int i, int q) { return wm() * 32 + i * 16 + lg() * 4 + q; }
// fp64 16x16x4 (differs from the fp32 form; a mix-up is silent): register q of lane l holds D[row = 4 q + (l >> 4)][col = l & 15]
__device__ __forceinline__ int row_f64(int i, int q) { return wm() * 32 + i * 16 + q * 4 + lg(); }
__device__ __forceinline__ int col(int j) { return wn() * 32 + j * 16 + l15(); }

// f(m, n, value) for the lane's 16 elements, m and n tile-local; order i, j, q (a caller that sums what it sees depends on it)
template <class F>
__device__ __forceinline__ void for_each(const f32x4_t (&acc)[2][2], F f) {
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int q = 0; q < 4; ++q) f(row_f32(i, q), col(j), acc[i][j][q]);
}
// fp64: order j, i, q, and c = percol(n) is evaluated once per column and handed to f(m, n, value, c)
template <class C, class F>
__device__ __forceinline__ void for_each(const f64x4_t (&acc)[2][2], C percol, F f) {
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const auto c = percol(col(j));
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int q = 0; q < 4; ++q) f(row_f64(i, q), col(j), acc[i][j][q], c);
  }
}
template <class F>
__device__ __forceinline__ void for_each(const f64x4_t (&acc)[2][2], F f) {
  for_each(acc, [](int) { return 0; }, [&](int m, int n, double v, int) { f(m, n, v); });
}

}  // namespace tile64
