// The streaming skeleton of the kernels that read up to K flat fp32 states once each and write one result (optim.hip: fedavg_multi,
// fedopt_sqnorm, fedopt_multi; robust.hip: robust_trimmed_mean, robust_pairdist): launch rule, pointer-array argument and its host check,
// read-once loads, the vector-then-tail element loop, instantiation dispatch, and the fixed-order fp64 reduction lanes -> waves -> blocks.
// compress.hip (delta_quantize, delta_aggregate: block-scaled integer codes of x_i - x) goes on the same skeleton with 8 elements per thread:
// multi_state_grid_per<8> and BytePtrs below are its variants of the launch rule and of the pointer array.
#pragma once
#include "common.h"
#include <type_traits>

// THE launch rule of the family: blocks of MULTI_STATE_BLOCK threads (the loop and the reduction below are written for that size), one block
// per 256 float4s (+ 1 so that a tail-only n still gets a block), 2048 at the most
constexpr int MULTI_STATE_BLOCK = 256;
static inline int multi_state_grid(size_t n) {
  const size_t blocks = (n / 4 + 1 + MULTI_STATE_BLOCK - 1) / MULTI_STATE_BLOCK;
  return (int)(blocks > 2048 ? 2048 : blocks);
}
// the variant of the rule for a kernel whose threads take PER elements each instead of one float4 (compress.hip: 8): one block per 256 units
// of PER elements (+ 1), 2048 at the most
template <int PER>
static inline int multi_state_grid_per(size_t n) {
  const size_t blocks = (n / PER + 1 + MULTI_STATE_BLOCK - 1) / MULTI_STATE_BLOCK;
  return (int)(blocks > 2048 ? 2048 : blocks);
}

// up to CAP device pointers as ONE kernel argument
template <int CAP>
struct StatePtrs {
  const float* src[CAP];
};
// p.src[0 .. k) = srcs[0 .. k); refuses a null entry ("<who>: <what> <i> is null"); ORs the addresses into `al` for the caller's alignment check
template <int CAP>
static inline int state_ptrs_fill(StatePtrs<CAP>& p, const float* const* srcs, int k, const char* who, const char* what, uintptr_t& al) {
  for (int i = 0; i < k; ++i) {
    FEDFR_REQUIRE(srcs[i] != nullptr, "%s: %s %d is null", who, what, i);
    p.src[i] = srcs[i];
    al |= (uintptr_t)srcs[i];
  }
  return FEDFR_OK;
}

// the same for up to CAP byte buffers (compress.hip: the codes and the scale bytes of compressed uploads)
template <int CAP>
struct BytePtrs {
  const unsigned char* src[CAP];
};
template <int CAP>
static inline int byte_ptrs_fill(BytePtrs<CAP>& p, const void* const* srcs, int k, const char* who, const char* what, uintptr_t& al) {
  for (int i = 0; i < k; ++i) {
    FEDFR_REQUIRE(srcs[i] != nullptr, "%s: %s %d is null", who, what, i);
    p.src[i] = static_cast<const unsigned char*>(srcs[i]);
    al |= (uintptr_t)srcs[i];
  }
  return FEDFR_OK;
}

// f(std::integral_constant<int, k>) for the run-time k in LO .. HI (nothing outside: the callers have checked the range)
template <int LO, int HI, class F>
static inline void dispatch_int(int k, F&& f) {
  if constexpr (LO <= HI) {
    if (k == LO) f(std::integral_constant<int, LO>{});
    else dispatch_int<LO + 1, HI>(k, f);
  }
}

template <int W>
using fvec = float __attribute__((ext_vector_type(W)));
// vector i of W floats of a buffer
template <int W>
__device__ __forceinline__ fvec<W>& vec_at(float* p, size_t i) { return reinterpret_cast<fvec<W>*>(p)[i]; }
template <int W>
__device__ __forceinline__ const fvec<W>& vec_at(const float* p, size_t i) { return reinterpret_cast<const fvec<W>*>(p)[i]; }
// the same of a state that is read exactly once: non-temporal
template <int W>
__device__ __forceinline__ fvec<W> ld_once(const float* p, size_t i) { return __builtin_nontemporal_load(&vec_at<W>(p, i)); }

// body(width, i): grid-stride over the n / V whole vectors with width = integral_constant<V> and i the VECTOR index, then over the n % V
// elements behind them with width = integral_constant<1> and i the ELEMENT index; a kernel's arithmetic is written once, for any width.
// Used by fedopt_sqnorm_kernel ONLY: the other four kernels of the family lose registers or time through the callable and keep two explicit
// loops.  A new kernel of the family starts here and leaves on the same evidence.
template <int V, class F>
__device__ __forceinline__ void for_each_vec_then_tail(size_t n, F&& body) {
  // (the builtin, not blockDim.x: outside a __global__ function the compiler does not know the block size to be uniform and reads it per lane)
  const unsigned bs = __builtin_amdgcn_workgroup_size_x();
  const size_t stride = (size_t)gridDim.x * bs, t = (size_t)blockIdx.x * bs + threadIdx.x, nv = n / V;
  for (size_t i = t; i < nv; i += stride) body(std::integral_constant<int, V>{}, i);
  for (size_t i = nv * V + t; i < n; i += stride) body(std::integral_constant<int, 1>{}, i);
}

// P per-thread fp64 sums of a block -> part[row_of(q)][blockIdx.x], in a FIXED order: lanes by the xor-shuffle tree of wave_sum_d,
// the four waves through LDS as ((w0 + w1) + w2) + w3.  No atomics: ordered_partial_sum adds the blocks
template <int P, int PR, class RowOf>
__device__ __forceinline__ void block_partial_d(const double (&acc)[P], double (&red)[4][PR], double* __restrict__ part, RowOf&& row_of) {
  static_assert(P <= PR && P <= MULTI_STATE_BLOCK && MULTI_STATE_BLOCK == 4 * 64, "one LDS column and one thread per sum, four waves");
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < P; ++q) {
    const double t = wave_sum_d(acc[q]);
    if (lane == 0) red[w][q] = t;
  }
  __syncthreads();
  if ((int)threadIdx.x < P) {
    const int q = threadIdx.x;
    part[(size_t)row_of(q) * gridDim.x + blockIdx.x] = ((red[0][q] + red[1][q]) + red[2][q]) + red[3][q];
  }
}
// row[0] + row[1] + ... + row[grid - 1] in ascending order, by ONE wave, the sum in every lane.  A lone thread walking the row pays a memory
// round trip per handful of partials (measured: ~0.1 ms of a 0.54 ms call at grid = 2048); here the wave fetches 256 partials at a time, one per
// lane and load, and every lane adds them in order out of the lanes' registers (v_readlane), so the serial part is the chain of `grid` fp64
// additions and nothing else.  Slots past `grid` hold 0.0: s + 0.0 == s bit for bit (s >= +0).
__device__ __forceinline__ double ordered_partial_sum(const double* __restrict__ row, int grid, int lane) {
  double s = 0.0;
  for (int b0 = 0; b0 < grid; b0 += 256) {
    double p[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int b = b0 + 64 * q + lane;
      p[q] = b < grid ? row[b] : 0.0;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int lo = __double2loint(p[q]), hi = __double2hiint(p[q]);
#pragma unroll
      for (int j = 0; j < 64; ++j) s += __hiloint2double(__builtin_amdgcn_readlane(hi, j), __builtin_amdgcn_readlane(lo, j));
    }
  }
  return s;
}
