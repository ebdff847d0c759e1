// Top-k sparsified client uploads with error feedback: a client sends the `keep` largest-magnitude entries of v = x_i - x + e_i as sorted
// (index, value) pairs and keeps the rest as e_i; the server adds up to 8 such uploads per pass.  The format is stated in
// include/fedfr_hip.h (fedfr_topk_sparsify) and restated in numpy in tests/sparse_cases.py.  Nothing is rounded after v is formed and the
// selection is exact, so both kernels are held to that restatement bit for bit.
//
// SELECTION.  key = bits(v) & 0x7FFFFFFF orders by magnitude as an integer.  The keep-th largest key T is found by a radix select over three
// digits of 11 / 10 / 10 bits from the top: a histogram pass per digit over the elements whose higher digits equal the prefix chosen so far,
// and a one-workgroup kernel that picks the digit's bin from the histogram.  T and r = keep - #{key > T} never leave the device.  Then a
// pass counts (#key > T, #key == T) per tile, one workgroup scans the tile counts, and an emit pass ranks every element inside its tile
// (ballots inside a wave, LDS across the four waves) and writes it to its place.  NO kernel waits for another workgroup of its own launch
// (Server.train's parallel_clients mode relies on that): every dependency is a kernel boundary.  Histograms are integer sums (LDS atomics
// per wave, then global atomics): order-free.  There are no float atomics.
//
// LANE MAPPING (as compress.hip).  A lane owns 8 consecutive elements (two 16-byte accesses), a wave 512, a workgroup of 4 waves one TILE of
// 2048; workgroups take tiles grid-stride.  The last, partial tile goes through the same code with guarded 4-byte accesses.
#include "sparse.h"
#include "dp.h"            // DpStream, dp_gauss4: the noise of fedfr_sparse_aggregate_dp's last pass
#include "multi_state.h"
#include "optim.h"         // optim_fedopt_sqnorm_final: the last step of the norm pass
#include <cmath>

constexpr int TOPK_EPT = 8;                               // elements per lane
constexpr int TOPK_WAVE = 64 * TOPK_EPT;                  // elements per wave
constexpr int TOPK_WPB = MULTI_STATE_BLOCK / 64;          // waves per workgroup
constexpr int TOPK_TILE = TOPK_WPB * TOPK_WAVE;           // elements per workgroup and loop iteration: 2048
constexpr int TOPK_GRID_CAP = 2048;
constexpr int TOPK_BINS1 = 2048, TOPK_BINS23 = 1024;      // 31-bit keys = 11 + 10 + 10 bits
constexpr int TOPK_SCAN_BLOCK = 1024, TOPK_SCAN_PER = 8;  // the one-workgroup scan of the tile counts
static_assert(MULTI_STATE_BLOCK == 256 && TOPK_TILE == 2048, "four waves, 2048 elements per tile (tests/sparse_cases.py mirrors these)");

// the head of the workspace: the select state, then the three histograms, then one (#key > T, #key == T) pair per tile (scanned in place);
// without error feedback the n values v follow (with it they live in the residual buffer)
struct TopkState {
  unsigned prefix;      // the digits chosen so far; after the third select: T
  unsigned krem;        // how many of the elements under that prefix are still to be taken; after the third select: r
  unsigned pad[2];
};
constexpr size_t TOPK_OFF_HIST1 = sizeof(TopkState);
constexpr size_t TOPK_OFF_HIST2 = TOPK_OFF_HIST1 + 4 * TOPK_BINS1;
constexpr size_t TOPK_OFF_HIST3 = TOPK_OFF_HIST2 + 4 * TOPK_BINS23;
constexpr size_t TOPK_OFF_TILES = TOPK_OFF_HIST3 + 4 * TOPK_BINS23;
static_assert(TOPK_OFF_TILES % 16 == 0, "the tile counts start 16-byte aligned");

__host__ __device__ static inline size_t topk_tiles(size_t n) { return (n + TOPK_TILE - 1) / TOPK_TILE; }
static inline size_t topk_head_bytes(size_t n) { return align_up(TOPK_OFF_TILES + 8 * topk_tiles(n), 16); }
size_t topk_workspace_bytes(size_t n, int feedback) { return topk_head_bytes(n) + (feedback ? 0 : align_up(4 * n, 16)); }

__device__ __forceinline__ unsigned topk_key(float v) { return __builtin_bit_cast(unsigned, v) & 0x7FFFFFFFu; }
// how many lanes below this one have their bit set in the ballot m
__device__ __forceinline__ unsigned lanes_below(unsigned long long m) {
  return __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}
__device__ __forceinline__ unsigned wave_sum_u(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += (unsigned)__shfl_xor((int)v, o, 64);
  return v;
}

// a lane's 8 values of the tile that starts at element t0 (FULL: the whole tile lies inside n); elements past n read as +0 and are flagged
// invalid by the callers (e0 + j < n)
template <bool FULL>
__device__ __forceinline__ void topk_load(const float* __restrict__ vb, size_t e0, size_t n, float (&v)[TOPK_EPT]) {
  if (FULL) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const fvec<4> a = vec_at<4>(vb, e0 / 4 + h);
#pragma unroll
      for (int q = 0; q < 4; ++q) v[4 * h + q] = a[q];
    }
  } else {
#pragma unroll
    for (int j = 0; j < TOPK_EPT; ++j) v[j] = e0 + j < n ? vb[e0 + j] : 0.f;
  }
}

__global__ __launch_bounds__(MULTI_STATE_BLOCK) void topk_zero_kernel(unsigned* __restrict__ head, int words) {
  const int i = blockIdx.x * MULTI_STATE_BLOCK + threadIdx.x;
  if (i < words) head[i] = 0u;
}

// the four waves' private histograms -> the global one (zero bins cost nothing: real deltas fill a few dozen)
template <int BINS>
__device__ __forceinline__ void topk_flush_hist(unsigned (&lh)[TOPK_WPB][BINS], unsigned* __restrict__ hist) {
  __syncthreads();
  for (int b = threadIdx.x; b < BINS; b += MULTI_STATE_BLOCK) {
    const unsigned s = lh[0][b] + lh[1][b] + lh[2][b] + lh[3][b];
    if (s) atomicAdd(&hist[b], s);
  }
}

// ---------------------------------------------------------------------------------------------------------
// pass 1: v = (x_i - x) + e, stored (in place over e with FB, else into the workspace), the histogram of the top 11 key bits, and the count
// of non-finite elements
// ---------------------------------------------------------------------------------------------------------
template <bool FB, bool FULL>
__device__ __forceinline__ void topk_pass1_tile(const float* __restrict__ x, const float* __restrict__ xi, float* vb, size_t n, size_t e0,
                                                unsigned* lh, unsigned& bad) {
  float v[TOPK_EPT];
  if (FULL) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const fvec<4> a = ld_once<4>(xi, e0 / 4 + h), b = ld_once<4>(x, e0 / 4 + h);
      fvec<4> r = {0.f, 0.f, 0.f, 0.f};
      if (FB) r = vec_at<4>(vb, e0 / 4 + h);
      fvec<4> o;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float d = __fsub_rn(a[q], b[q]);
        o[q] = v[4 * h + q] = FB ? __fadd_rn(d, r[q]) : d;
      }
      vec_at<4>(vb, e0 / 4 + h) = o;
    }
  } else {
#pragma unroll
    for (int j = 0; j < TOPK_EPT; ++j) {
      v[j] = 0.f;
      if (e0 + j < n) {
        const float d = __fsub_rn(xi[e0 + j], x[e0 + j]);
        v[j] = FB ? __fadd_rn(d, vb[e0 + j]) : d;
        vb[e0 + j] = v[j];
      }
    }
  }
#pragma unroll
  for (int j = 0; j < TOPK_EPT; ++j) {
    if (FULL || e0 + j < n) {
      const unsigned key = topk_key(v[j]);
      atomicAdd(&lh[key >> 20], 1u);
      bad += key >= 0x7F800000u ? 1u : 0u;
    }
  }
}

template <bool FB>
__global__ __launch_bounds__(MULTI_STATE_BLOCK) void topk_hist1_kernel(const float* __restrict__ x, const float* __restrict__ xi, float* vb, size_t n,
                                                                       unsigned* __restrict__ hist, int* __restrict__ nonfinite) {
  __shared__ unsigned lh[TOPK_WPB][TOPK_BINS1];      // a histogram per wave: 32 KB
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int b = threadIdx.x; b < TOPK_WPB * TOPK_BINS1; b += MULTI_STATE_BLOCK) (&lh[0][0])[b] = 0u;
  __syncthreads();
  const size_t ntiles = topk_tiles(n);
  unsigned bad = 0u;
  for (size_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const size_t e0 = t * TOPK_TILE + (size_t)w * TOPK_WAVE + (size_t)lane * TOPK_EPT;
    if ((t + 1) * TOPK_TILE <= n) topk_pass1_tile<FB, true>(x, xi, vb, n, e0, lh[w], bad);
    else topk_pass1_tile<FB, false>(x, xi, vb, n, e0, lh[w], bad);
  }
  topk_flush_hist<TOPK_BINS1>(lh, hist);
  bad = wave_sum_u(bad);
  if (lane == 0 && bad && nonfinite) atomicAdd(nonfinite, (int)bad);
}

// passes 2 and 3: the histogram of the next 10 key bits of the elements whose bits from SHIFT up equal the prefix chosen so far
template <int SHIFT>
__global__ __launch_bounds__(MULTI_STATE_BLOCK) void topk_histn_kernel(const float* __restrict__ vb, size_t n, const TopkState* __restrict__ state,
                                                                       unsigned* __restrict__ hist) {
  __shared__ unsigned lh[TOPK_WPB][TOPK_BINS23];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int b = threadIdx.x; b < TOPK_WPB * TOPK_BINS23; b += MULTI_STATE_BLOCK) (&lh[0][0])[b] = 0u;
  __syncthreads();
  const unsigned prefix = state->prefix;
  const size_t ntiles = topk_tiles(n);
  for (size_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const size_t e0 = t * TOPK_TILE + (size_t)w * TOPK_WAVE + (size_t)lane * TOPK_EPT;
    const bool full = (t + 1) * TOPK_TILE <= n;
    float v[TOPK_EPT];
    if (full) topk_load<true>(vb, e0, n, v);
    else topk_load<false>(vb, e0, n, v);
#pragma unroll
    for (int j = 0; j < TOPK_EPT; ++j) {
      const unsigned key = topk_key(v[j]);
      if ((full || e0 + j < n) && (key >> SHIFT) == prefix) atomicAdd(&lh[w][(key >> (SHIFT - 10)) & (TOPK_BINS23 - 1)], 1u);
    }
  }
  topk_flush_hist<TOPK_BINS23>(lh, hist);
}

// ---------------------------------------------------------------------------------------------------------
// inclusive scan of one unsigned pair per thread over a workgroup of NW waves (shuffles inside a wave, LDS across); `total` = the sum
// ---------------------------------------------------------------------------------------------------------
template <int NW>
__device__ __forceinline__ uint2 block_scan_incl(uint2 v, uint2 (&wt)[NW], uint2& total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned ax = (unsigned)__shfl_up((int)v.x, o, 64), ay = (unsigned)__shfl_up((int)v.y, o, 64);
    if (lane >= o) {
      v.x += ax;
      v.y += ay;
    }
  }
  __syncthreads();      // (wt may still be read from the previous use)
  if (lane == 63) wt[w] = v;
  __syncthreads();
  total = make_uint2(0u, 0u);
#pragma unroll
  for (int q = 0; q < NW; ++q) {
    const uint2 s = wt[q];
    if (q < w) {
      v.x += s.x;
      v.y += s.y;
    }
    total.x += s.x;
    total.y += s.y;
  }
  return v;
}

// one workgroup: the bin of this digit.  Thread t owns BINS / 256 bins counted from the TOP; the bin b with
// #{bins above b} < krem <= #{bins above b} + hist[b] holds the krem-th largest key under the prefix (exactly one bin does: the elements
// under the prefix are at least krem).  first: the state is (prefix 0, krem = keep).
template <int LOGB>
__global__ __launch_bounds__(MULTI_STATE_BLOCK) void topk_select_kernel(const unsigned* __restrict__ hist, TopkState* __restrict__ state, unsigned keep, int first) {
  constexpr int BINS = 1 << LOGB, PER = BINS / MULTI_STATE_BLOCK;
  __shared__ uint2 wt[TOPK_WPB];
  const unsigned prefix = first ? 0u : state->prefix, krem = first ? keep : state->krem;
  unsigned h[PER], s = 0u;
#pragma unroll
  for (int q = 0; q < PER; ++q) {
    h[q] = hist[BINS - 1 - ((int)threadIdx.x * PER + q)];
    s += h[q];
  }
  uint2 total;
  const uint2 inc = block_scan_incl<TOPK_WPB>(make_uint2(s, 0u), wt, total);      // (the barriers inside order the reads above before the write below)
  unsigned above = inc.x - s;
#pragma unroll
  for (int q = 0; q < PER; ++q) {
    if (above < krem && krem <= above + h[q]) {
      state->prefix = (prefix << LOGB) | (unsigned)(BINS - 1 - ((int)threadIdx.x * PER + q));
      state->krem = krem - above;
    }
    above += h[q];
  }
}

// bit j of gt / eq: element j of the lane's 8 lies inside n and has key > T / key == T
__device__ __forceinline__ void topk_flags(const float (&v)[TOPK_EPT], size_t e0, size_t n, bool full, unsigned T, unsigned& gt, unsigned& eq) {
  gt = eq = 0u;
#pragma unroll
  for (int j = 0; j < TOPK_EPT; ++j) {
    const unsigned key = topk_key(v[j]);
    const bool ok = full || e0 + j < n;
    gt |= (ok && key > T ? 1u : 0u) << j;
    eq |= (ok && key == T ? 1u : 0u) << j;
  }
}

// the count pass: cnt[tile] = (#key > T, #key == T)
__global__ __launch_bounds__(MULTI_STATE_BLOCK) void topk_count_kernel(const float* __restrict__ vb, size_t n, const TopkState* __restrict__ state,
                                                                       uint2* __restrict__ cnt) {
  __shared__ unsigned wc[2][TOPK_WPB];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const unsigned T = state->prefix;
  const size_t ntiles = topk_tiles(n);
  int par = 0;
  for (size_t t = blockIdx.x; t < ntiles; t += gridDim.x, par ^= 1) {
    const size_t e0 = t * TOPK_TILE + (size_t)w * TOPK_WAVE + (size_t)lane * TOPK_EPT;
    const bool full = (t + 1) * TOPK_TILE <= n;
    float v[TOPK_EPT];
    if (full) topk_load<true>(vb, e0, n, v);
    else topk_load<false>(vb, e0, n, v);
    unsigned gt, eq;
    topk_flags(v, e0, n, full, T, gt, eq);
    const unsigned c = wave_sum_u((unsigned)__builtin_popcount(gt) | ((unsigned)__builtin_popcount(eq) << 16));      // <= 512 each: 16 bits hold it
    if (lane == 0) wc[par][w] = c;
    __syncthreads();      // (wc is double-buffered: the next iteration writes the other half, the one after it comes behind this barrier's successor)
    if (threadIdx.x == 0) {
      unsigned g = 0u, e = 0u;
#pragma unroll
      for (int q = 0; q < TOPK_WPB; ++q) {
        g += wc[par][q] & 0xFFFFu;
        e += wc[par][q] >> 16;
      }
      cnt[t] = make_uint2(g, e);
    }
  }
}

// one workgroup: cnt[tile] becomes the exclusive prefix sum of the pairs, 1024 x 8 tiles per step, the carry in registers
__global__ __launch_bounds__(TOPK_SCAN_BLOCK) void topk_scan_kernel(uint2* __restrict__ cnt, size_t ntiles) {
  __shared__ uint2 wt[TOPK_SCAN_BLOCK / 64];
  uint2 carry = make_uint2(0u, 0u);
  for (size_t base = 0; base < ntiles; base += (size_t)TOPK_SCAN_BLOCK * TOPK_SCAN_PER) {
    const size_t i0 = base + (size_t)threadIdx.x * TOPK_SCAN_PER;
    uint2 c[TOPK_SCAN_PER], s = make_uint2(0u, 0u);
#pragma unroll
    for (int q = 0; q < TOPK_SCAN_PER; ++q) {
      c[q] = i0 + q < ntiles ? cnt[i0 + q] : make_uint2(0u, 0u);
      s.x += c[q].x;
      s.y += c[q].y;
    }
    uint2 total;
    const uint2 inc = block_scan_incl<TOPK_SCAN_BLOCK / 64>(s, wt, total);
    uint2 run = make_uint2(carry.x + inc.x - s.x, carry.y + inc.y - s.y);
#pragma unroll
    for (int q = 0; q < TOPK_SCAN_PER; ++q) {
      if (i0 + q < ntiles) cnt[i0 + q] = run;
      run.x += c[q].x;
      run.y += c[q].y;
    }
    carry.x += total.x;
    carry.y += total.y;
  }
}

// the emit pass.  An element j of S lands at #{key > T, index < j} + min(#{key == T, index < j}, r); the counts before j are the tile's
// scanned pair + the waves before this one (LDS) + the lanes before this one (ballots) + the lane's own earlier elements.
template <bool FB>
__global__ __launch_bounds__(MULTI_STATE_BLOCK) void topk_emit_kernel(float* vb, size_t n, const TopkState* __restrict__ state, const uint2* __restrict__ cnt,
                                                                      unsigned* __restrict__ idx, float* __restrict__ val, unsigned keep) {
  __shared__ uint2 wc[2][TOPK_WPB];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const unsigned T = state->prefix, r = state->krem;
  const size_t ntiles = topk_tiles(n);
  int par = 0;
  for (size_t t = blockIdx.x; t < ntiles; t += gridDim.x, par ^= 1) {
    const size_t e0 = t * TOPK_TILE + (size_t)w * TOPK_WAVE + (size_t)lane * TOPK_EPT;
    const bool full = (t + 1) * TOPK_TILE <= n;
    float v[TOPK_EPT];
    if (full) topk_load<true>(vb, e0, n, v);
    else topk_load<false>(vb, e0, n, v);
    unsigned gt, eq;
    topk_flags(v, e0, n, full, T, gt, eq);
    // lanes before this one and the wave's total: a lane's 8 elements are consecutive, so the lane's count is what the lanes behind it skip
    unsigned g = 0u, e = 0u, wg = 0u, we = 0u;
#pragma unroll
    for (int j = 0; j < TOPK_EPT; ++j) {
      const unsigned long long mg = __ballot((gt >> j) & 1u), me = __ballot((eq >> j) & 1u);
      g += lanes_below(mg);
      e += lanes_below(me);
      wg += (unsigned)__popcll(mg);
      we += (unsigned)__popcll(me);
    }
    if (lane == 0) wc[par][w] = make_uint2(wg, we);
    __syncthreads();
    const uint2 tile0 = cnt[t];
    g += tile0.x;
    e += tile0.y;
#pragma unroll
    for (int q = 0; q < TOPK_WPB - 1; ++q) {
      if (q < w) {
        g += wc[par][q].x;
        e += wc[par][q].y;
      }
    }
#pragma unroll
    for (int j = 0; j < TOPK_EPT; ++j) {
      const bool isg = (gt >> j) & 1u, ise = (eq >> j) & 1u;
      const bool sel = isg || (ise && e < r);
      if (sel) {
        const unsigned at = g + min(e, r);
        if (at < keep) {      // (always: the position law maps S onto 0 .. keep - 1; the guard keeps a wrong T or r inside the buffers)
          idx[at] = (unsigned)(e0 + j);
          val[at] = v[j];
        }
      }
      // e' = +0 where the element was sent or is not finite; everywhere else v is e' already
      if (FB && (sel || ((full || e0 + j < n) && topk_key(v[j]) >= 0x7F800000u))) vb[e0 + j] = 0.f;
      g += isg ? 1u : 0u;
      e += ise ? 1u : 0u;
    }
  }
}

int topk_sparsify(const float* x, const float* xi, float* resid, size_t n, size_t keep, unsigned* idx, float* val, int* nonfinite, void* ws,
                  hipStream_t st) {
  FEDFR_REQUIRE(x && xi && idx && val && ws, "topk_sparsify: null pointer (x=%p xi=%p idx=%p val=%p ws=%p)", (const void*)x, (const void*)xi, (void*)idx,
                (void*)val, ws);
  FEDFR_REQUIRE((((uintptr_t)x | (uintptr_t)xi | (uintptr_t)resid | (uintptr_t)idx | (uintptr_t)val | (uintptr_t)ws) & 15) == 0,
                "topk_sparsify: x, xi, resid, idx, val and ws must be 16-byte aligned");
  FEDFR_REQUIRE(((uintptr_t)nonfinite & 3) == 0, "topk_sparsify: nonfinite must be 4-byte aligned");
  FEDFR_REQUIRE(n < ((size_t)1 << 31), "topk_sparsify: n must be below 2^31 (n=%zu)", n);
  if (n == 0 && keep == 0) return FEDFR_OK;
  FEDFR_REQUIRE(keep >= 1 && keep <= n, "topk_sparsify: keep must be in 1..n (keep=%zu n=%zu)", keep, n);
  unsigned char* wb = static_cast<unsigned char*>(ws);
  TopkState* state = reinterpret_cast<TopkState*>(wb);
  unsigned* hist1 = reinterpret_cast<unsigned*>(wb + TOPK_OFF_HIST1);
  unsigned* hist2 = reinterpret_cast<unsigned*>(wb + TOPK_OFF_HIST2);
  unsigned* hist3 = reinterpret_cast<unsigned*>(wb + TOPK_OFF_HIST3);
  uint2* cnt = reinterpret_cast<uint2*>(wb + TOPK_OFF_TILES);
  float* vb = resid ? resid : reinterpret_cast<float*>(wb + topk_head_bytes(n));
  const size_t ntiles = topk_tiles(n);
  const dim3 grid((unsigned)(ntiles > TOPK_GRID_CAP ? TOPK_GRID_CAP : ntiles)), block(MULTI_STATE_BLOCK), one(1);
  const int words = (int)(TOPK_OFF_TILES / 4);
  hipLaunchKernelGGL(topk_zero_kernel, dim3((words + MULTI_STATE_BLOCK - 1) / MULTI_STATE_BLOCK), block, 0, st, reinterpret_cast<unsigned*>(wb), words);
  if (resid) hipLaunchKernelGGL(topk_hist1_kernel<true>, grid, block, 0, st, x, xi, vb, n, hist1, nonfinite);
  else hipLaunchKernelGGL(topk_hist1_kernel<false>, grid, block, 0, st, x, xi, vb, n, hist1, nonfinite);
  hipLaunchKernelGGL(topk_select_kernel<11>, one, block, 0, st, hist1, state, (unsigned)keep, 1);
  hipLaunchKernelGGL(topk_histn_kernel<20>, grid, block, 0, st, vb, n, state, hist2);
  hipLaunchKernelGGL(topk_select_kernel<10>, one, block, 0, st, hist2, state, 0u, 0);
  hipLaunchKernelGGL(topk_histn_kernel<10>, grid, block, 0, st, vb, n, state, hist3);
  hipLaunchKernelGGL(topk_select_kernel<10>, one, block, 0, st, hist3, state, 0u, 0);
  hipLaunchKernelGGL(topk_count_kernel, grid, block, 0, st, vb, n, state, cnt);
  hipLaunchKernelGGL(topk_scan_kernel, one, dim3(TOPK_SCAN_BLOCK), 0, st, cnt, ntiles);
  if (resid) hipLaunchKernelGGL(topk_emit_kernel<true>, grid, block, 0, st, vb, n, state, cnt, idx, val, (unsigned)keep);
  else hipLaunchKernelGGL(topk_emit_kernel<false>, grid, block, 0, st, vb, n, state, cnt, idx, val, (unsigned)keep);
  FEDFR_LAUNCH_CHECK("topk_sparsify");
  return FEDFR_OK;
}

// ---------------------------------------------------------------------------------------------------------
// aggregate: s = accumulate ? dst : +0; s = s + w_i val_i[t] at j = idx_i[t], ascending i; dst = base ? base + s : s.
// A workgroup owns a CONTIGUOUS range of tiles of 4096 elements and keeps one tile of s in LDS.  Per upload it finds the first entry of its
// range once (a binary search by one lane per upload) and from there walks the sorted entries: 256 entries per step, one per thread; an
// entry is applied only if its index lies inside the tile, the in-tile entries are counted (a ballot per wave, LDS across), and the count
// moves the upload's cursor.  Indices are unique inside an upload, so the LDS adds of one step need no atomics; the barrier that publishes
// the count also orders upload i before upload i + 1.  For ANY index content every read of idx / val stays below keep_i and every LDS
// access inside the tile: an unsorted or out-of-range upload gives an unspecified sum, never an out-of-bounds access.
// BARRIERS.  (1) Between a tile's initialisation of s and the first adds: the barrier behind the first loads.  (2) Between upload i and
// upload i + 1, and between the last adds and the output: the barrier of every step.  (3) Between a tile's output and the NEXT tile's
// initialisation there is none, and none is needed: in both phases, and in whole and partial tiles alike, thread tid touches exactly the
// float4s at (q 256 + tid) 4, so what a thread overwrites early is what it has read itself; any other thread's adds into those positions
// come behind barrier (1) of the next tile, which no thread passes before all have finished their output.  The count words wc are double
// buffered: a word is rewritten two steps later, behind the barrier of the step between.
// A step loads 256 entries of an upload and keeps those inside the tile; the others are loaded again for the next tile, so an entry is
// loaded about 256 / (entries per tile) times in all: 6 times at 1 % density, by the same workgroup within microseconds (where those
// re-reads are served from has not been measured).
// ---------------------------------------------------------------------------------------------------------
constexpr int SAGG_TILE = 4096;
constexpr int SAGG_PER = SAGG_TILE / MULTI_STATE_BLOCK / 4;      // float4s per thread and tile
struct SparseUploads {
  const unsigned* idx[8];
  const float* val[8];
  unsigned keep[8];
  float w[8];
};

// The body, written ONCE for the two shells below it: wt[] are the K weights wherever they came from (up.w is not read here); with NOISE,
// noise_std z of the stream rs is added to EVERY element of the tile before base (the host selects NOISE only for the last pass of a chain
// with noise_std > 0).  A thread's float4 at element ts + pos is Philox block (ts + pos) / 4 of the buffer: the value depends on the
// element's index alone.
template <int K, bool NOISE>
__device__ __forceinline__ void sparse_aggregate_body(float* dst, const float* base, const SparseUploads& up, const float (&wt)[K], unsigned n, int accumulate,
                                                      float noise_std, const DpStream& rs) {
  __shared__ float s[SAGG_TILE];
  __shared__ unsigned start[8];
  __shared__ unsigned wc[2][TOPK_WPB];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const unsigned ntiles = (n + SAGG_TILE - 1) / SAGG_TILE;
  const unsigned t0 = (unsigned)((unsigned long long)blockIdx.x * ntiles / gridDim.x), t1 = (unsigned)(((unsigned long long)blockIdx.x + 1) * ntiles / gridDim.x);
  if (tid < K) {      // the first entry with idx >= the range's first element (a select chain: the pointer arrays stay in registers)
    const unsigned* p = up.idx[0];
    unsigned hi = up.keep[0];
#pragma unroll
    for (int i = 1; i < K; ++i) {
      if (tid == i) {
        p = up.idx[i];
        hi = up.keep[i];
      }
    }
    const unsigned first = t0 * SAGG_TILE;
    unsigned lo = 0u;
    while (lo < hi) {
      const unsigned mid = lo + (hi - lo) / 2;
      if (p[mid] < first) lo = mid + 1;
      else hi = mid;
    }
    start[tid] = lo;
  }
  __syncthreads();
  unsigned cur[K];
#pragma unroll
  for (int i = 0; i < K; ++i) cur[i] = start[i];
  int par = 0;
  for (unsigned t = t0; t < t1; ++t) {
    const unsigned ts = t * SAGG_TILE, te = min(ts + SAGG_TILE, n);
    const bool full = te - ts == SAGG_TILE;
    // thread tid owns the float4s at (q 256 + tid) 4, q = 0..3, of the tile: it alone initialises them here and reads them in the output phase
    // below, in the whole and in the partial tile alike
#pragma unroll
    for (int q = 0; q < SAGG_PER; ++q) {
      const int pos = (q * MULTI_STATE_BLOCK + tid) * 4;
      fvec<4> d = {0.f, 0.f, 0.f, 0.f};
      if (accumulate) {
        if (full) {
          d = vec_at<4>(dst, (size_t)(ts + pos) / 4);
        } else {
#pragma unroll
          for (int c = 0; c < 4; ++c) d[c] = ts + pos + c < te ? dst[ts + pos + c] : 0.f;
        }
      }
      *reinterpret_cast<fvec<4>*>(&s[pos]) = d;
    }
    unsigned bi[K];
    float bv[K];
#pragma unroll
    for (int i = 0; i < K; ++i) {      // the first step of every upload: K independent loads in flight
      const unsigned p = cur[i] + tid;
      const bool in = p < up.keep[i];
      bi[i] = in ? up.idx[i][p] : 0xFFFFFFFFu;
      bv[i] = in ? up.val[i][p] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < K; ++i) {
      unsigned ix = bi[i];
      float vv = bv[i];
      bool more;
      do {
        const bool inr = ix >= ts && ix < te;      // (the filler 0xFFFFFFFF is never inside: te <= n < 2^31)
        if (inr) s[ix - ts] = __fadd_rn(s[ix - ts], __fmul_rn(wt[i], vv));
        const unsigned long long m = __ballot(inr);
        if (lane == 0) wc[par][w] = (unsigned)__popcll(m);
        __syncthreads();
        const unsigned c = wc[par][0] + wc[par][1] + wc[par][2] + wc[par][3];
        par ^= 1;
        cur[i] += c;
        more = c == MULTI_STATE_BLOCK;             // a step that was in-tile throughout: the tile may hold more of this upload
        if (more) {
          const unsigned p = cur[i] + tid;
          const bool in = p < up.keep[i];
          ix = in ? up.idx[i][p] : 0xFFFFFFFFu;
          vv = in ? up.val[i][p] : 0.f;
        }
      } while (more);
    }
    // output: every load (LDS and base) before the first store, so that they are in flight together: dst may equal base, but a thread's
    // stores touch only the positions it has loaded itself
    fvec<4> o[SAGG_PER];
#pragma unroll
    for (int q = 0; q < SAGG_PER; ++q) o[q] = *reinterpret_cast<const fvec<4>*>(&s[(q * MULTI_STATE_BLOCK + tid) * 4]);
    if (NOISE) {
#pragma unroll
      for (int q = 0; q < SAGG_PER; ++q) {
        const unsigned e = ts + (unsigned)(q * MULTI_STATE_BLOCK + tid) * 4;
        if (e < te) {      // (a float4 that lies behind n altogether is never stored)
          const float4 z = dp_gauss4(rs, e / 4);
          o[q][0] = __fadd_rn(o[q][0], __fmul_rn(noise_std, z.x));
          o[q][1] = __fadd_rn(o[q][1], __fmul_rn(noise_std, z.y));
          o[q][2] = __fadd_rn(o[q][2], __fmul_rn(noise_std, z.z));
          o[q][3] = __fadd_rn(o[q][3], __fmul_rn(noise_std, z.w));
        }
      }
    }
    if (base) {
      fvec<4> b[SAGG_PER];
#pragma unroll
      for (int q = 0; q < SAGG_PER; ++q) {
        const int pos = (q * MULTI_STATE_BLOCK + tid) * 4;
        if (full) {
          b[q] = vec_at<4>(base, (size_t)(ts + pos) / 4);
        } else {
#pragma unroll
          for (int c = 0; c < 4; ++c) b[q][c] = ts + pos + c < te ? base[ts + pos + c] : 0.f;
        }
      }
#pragma unroll
      for (int q = 0; q < SAGG_PER; ++q) {
#pragma unroll
        for (int c = 0; c < 4; ++c) o[q][c] = __fadd_rn(b[q][c], o[q][c]);
      }
    }
#pragma unroll
    for (int q = 0; q < SAGG_PER; ++q) {
      const int pos = (q * MULTI_STATE_BLOCK + tid) * 4;
      if (full) {
        vec_at<4>(dst, (size_t)(ts + pos) / 4) = o[q];
      } else {
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (ts + pos + c < te) dst[ts + pos + c] = o[q][c];
      }
    }
  }
}

// the shell of fedfr_sparse_aggregate: the weights travel by value, inside `up`
template <int K>
__global__ __launch_bounds__(MULTI_STATE_BLOCK) void sparse_aggregate_kernel(float* dst, const float* base, SparseUploads up, unsigned n, int accumulate) {
  float w[K];
#pragma unroll
  for (int i = 0; i < K; ++i) w[i] = up.w[i];
  sparse_aggregate_body<K, false>(dst, base, up, w, n, accumulate, 0.f, DpStream{});
}
// the shell of fedfr_sparse_aggregate_dp: the weights are what a norm pass left on the device, read once per thread
template <int K, bool NOISE>
__global__ __launch_bounds__(MULTI_STATE_BLOCK) void sparse_aggregate_dp_kernel(float* dst, const float* base, SparseUploads up, const float* __restrict__ coef, unsigned n,
                                                                                int accumulate, float noise_std, DpStream rs) {
  float w[K];
#pragma unroll
  for (int i = 0; i < K; ++i) w[i] = coef[i];
  sparse_aggregate_body<K, NOISE>(dst, base, up, w, n, accumulate, noise_std, rs);
}

// what both aggregates and the norm pass check of their uploads, and fill; `w` (the weights, `wname`) may be a device pointer: not read here
static int sparse_uploads_fill(const char* who, const char* wname, SparseUploads& up, uintptr_t& al, const unsigned* const* idx, const float* const* val,
                               const size_t* keeps, const float* w, int k, size_t n) {
  FEDFR_REQUIRE(k >= 1 && k <= 8, "%s: 1 to 8 uploads per call (k=%d)", who, k);
  FEDFR_REQUIRE(idx && val && keeps && w, "%s: null pointer (idx=%p val=%p keeps=%p %s=%p)", who, (const void*)idx, (const void*)val, (const void*)keeps, wname,
                (const void*)w);
  FEDFR_REQUIRE(n < ((size_t)1 << 31), "%s: n must be below 2^31 (n=%zu)", who, n);
  for (int i = 0; i < k; ++i) {
    FEDFR_REQUIRE(idx[i] != nullptr, "%s: index buffer %d is null", who, i);
    FEDFR_REQUIRE(val[i] != nullptr, "%s: value buffer %d is null", who, i);
    FEDFR_REQUIRE(keeps[i] <= n, "%s: upload %d holds more entries than there are elements (keep=%zu n=%zu)", who, i, keeps[i], n);
    up.idx[i] = idx[i];
    up.val[i] = val[i];
    up.keep[i] = (unsigned)keeps[i];
    al |= (uintptr_t)idx[i] | (uintptr_t)val[i];
  }
  return FEDFR_OK;
}

int sparse_aggregate_dp(float* dst, const float* base, const unsigned* const* idx, const float* const* val, const size_t* keeps, const float* coef,
                        int k, size_t n, int accumulate, int last, float noise_std, unsigned long long seed, unsigned long long round,
                        unsigned stream_id, unsigned long long offset, hipStream_t st) {
  SparseUploads up{};
  uintptr_t al = 0;
  FEDFR_REQUIRE(dst, "sparse_aggregate_dp: null pointer (dst=%p)", (void*)dst);
  FEDFR_TRY(sparse_uploads_fill("sparse_aggregate_dp", "coef", up, al, idx, val, keeps, coef, k, n));
  FEDFR_REQUIRE((((uintptr_t)dst | (uintptr_t)base | al) & 15) == 0, "sparse_aggregate_dp: dst, base and the index and value buffers must be 16-byte aligned");
  FEDFR_REQUIRE(((uintptr_t)coef & 3) == 0, "sparse_aggregate_dp: coef must be 4-byte aligned");
  FEDFR_REQUIRE(std::isfinite(noise_std) && noise_std >= 0.f, "sparse_aggregate_dp: noise_std must be finite and >= 0 (got %g)", (double)noise_std);
  FEDFR_REQUIRE(offset % 4 == 0, "sparse_aggregate_dp: offset %llu is not a multiple of 4", offset);
  if (n == 0) return FEDFR_OK;
  accumulate = accumulate ? 1 : 0;
  const size_t ntiles = (n + SAGG_TILE - 1) / SAGG_TILE;
  const int grid = (int)(ntiles > TOPK_GRID_CAP ? TOPK_GRID_CAP : ntiles);
  const DpStream rs = dp_stream(seed, round, stream_id, offset);
  dispatch_int<0, 1>(last && noise_std > 0.f ? 1 : 0, [&](auto nc) {
    dispatch_int<1, 8>(k, [&](auto kc) {
      hipLaunchKernelGGL((sparse_aggregate_dp_kernel<decltype(kc)::value, decltype(nc)::value != 0>), dim3(grid), dim3(MULTI_STATE_BLOCK), 0, st, dst, base, up, coef,
                         (unsigned)n, accumulate, noise_std, rs);
    });
  });
  FEDFR_LAUNCH_CHECK("sparse_aggregate_dp");
  return FEDFR_OK;
}

// ---------------------------------------------------------------------------------------------------------
// squared norms of <= 8 top-k uploads: sq_i = sum_e double(val_e)^2 (the square of an fp32 value is exact in fp64: fma(v, v, acc) rounds
// once), one entry per thread and step, grid-stride, on the launch rule of compress.hip's norm pass for m = the largest keep; then
// block_partial_d and fedopt_sqnorm_final_kernel (optim.hip): the fixed order of fedopt_sqnorm, no float atomics, every partial written by
// its block.  The scattered vector has norm sqrt(sq_i) only if the indices are distinct and inside n: an entry with idx_e >= n or
// idx_e <= idx_(e-1) is a violation, counted per upload (an integer sum: one atomic per wave that found any).
// ---------------------------------------------------------------------------------------------------------
template <int K>
__global__ __launch_bounds__(MULTI_STATE_BLOCK) void sparse_sqnorm_kernel(SparseUploads up, unsigned n, double* __restrict__ part, int* __restrict__ violations) {
  __shared__ double red[4][8];
  double acc[K];
  unsigned bad[K];
  const size_t stride = (size_t)gridDim.x * blockDim.x, t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
#pragma unroll
  for (int i = 0; i < K; ++i) {
    acc[i] = 0.0;
    bad[i] = 0u;
    const unsigned keep = up.keep[i];
    for (size_t e = t; e < keep; e += stride) {
      const double v = (double)__builtin_nontemporal_load(up.val[i] + e);
      acc[i] = __fma_rn(v, v, acc[i]);
      const unsigned ix = up.idx[i][e];
      bad[i] += (ix >= n || (e > 0 && ix <= up.idx[i][e - 1])) ? 1u : 0u;
    }
  }
#pragma unroll
  for (int i = 0; i < K; ++i) {
    const unsigned b = wave_sum_u(bad[i]);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(&violations[i], (int)b);
  }
  block_partial_d<K>(acc, red, part, [](int i) { return i; });
}

int sparse_sqnorm(const unsigned* const* idx, const float* const* val, const size_t* keeps, const float* ws, int k, size_t n, float clip, double* sq,
                  float* coef, int* violations, void* wsp, size_t ws_bytes, hipStream_t st) {
  SparseUploads up{};
  uintptr_t al = 0;
  FEDFR_REQUIRE(sq && coef && violations && wsp, "sparse_sqnorm: null pointer (sq=%p coef=%p violations=%p workspace=%p)", (void*)sq, (void*)coef, (void*)violations,
                wsp);
  FEDFR_TRY(sparse_uploads_fill("sparse_sqnorm", "ws", up, al, idx, val, keeps, ws, k, n));
  FEDFR_REQUIRE(n > 0, "sparse_sqnorm: n must be positive");
  FEDFR_REQUIRE(clip == clip, "sparse_sqnorm: clip is NaN");
  FEDFR_REQUIRE((al & 15) == 0, "sparse_sqnorm: the index and value buffers must be 16-byte aligned");
  FEDFR_REQUIRE((((uintptr_t)sq | (uintptr_t)wsp) & 7) == 0 && (((uintptr_t)coef | (uintptr_t)violations) & 3) == 0,
                "sparse_sqnorm: sq / workspace must be 8-byte, coef / violations 4-byte aligned");
  size_t m = 0;
  for (int i = 0; i < k; ++i) m = keeps[i] > m ? keeps[i] : m;
  const int grid = multi_state_grid_per<TOPK_EPT>(m);
  if (ws_bytes < (size_t)k * grid * sizeof(double)) {
    fedfr_set_error("sparse_sqnorm: workspace of %zu bytes, %zu needed", ws_bytes, (size_t)k * grid * sizeof(double));
    return FEDFR_ERR_WORKSPACE;
  }
  double* part = reinterpret_cast<double*>(wsp);
  dispatch_int<1, 8>(k, [&](auto kc) {
    hipLaunchKernelGGL((sparse_sqnorm_kernel<decltype(kc)::value>), dim3(grid), dim3(MULTI_STATE_BLOCK), 0, st, up, (unsigned)n, part, violations);
  });
  FEDFR_LAUNCH_CHECK("sparse_sqnorm");
  return optim_fedopt_sqnorm_final(part, grid, k, ws, clip, sq, coef, st);
}

int sparse_aggregate(float* dst, const float* base, const unsigned* const* idx, const float* const* val, const size_t* keeps, const float* ws, int k,
                     size_t n, int accumulate, hipStream_t st) {
  FEDFR_REQUIRE(k >= 1 && k <= 8, "sparse_aggregate: 1 to 8 uploads per call (k=%d)", k);
  FEDFR_REQUIRE(dst && idx && val && keeps && ws, "sparse_aggregate: null pointer (dst=%p idx=%p val=%p keeps=%p ws=%p)", (void*)dst, (const void*)idx,
                (const void*)val, (const void*)keeps, (const void*)ws);
  SparseUploads up{};
  uintptr_t al = 0;
  FEDFR_TRY(sparse_uploads_fill("sparse_aggregate", "ws", up, al, idx, val, keeps, ws, k, n));
  for (int i = 0; i < k; ++i) up.w[i] = ws[i];
  FEDFR_REQUIRE((((uintptr_t)dst | (uintptr_t)base | al) & 15) == 0, "sparse_aggregate: dst, base and the index and value buffers must be 16-byte aligned");
  if (n == 0) return FEDFR_OK;
  accumulate = accumulate ? 1 : 0;
  const size_t ntiles = (n + SAGG_TILE - 1) / SAGG_TILE;
  const int grid = (int)(ntiles > TOPK_GRID_CAP ? TOPK_GRID_CAP : ntiles);
  dispatch_int<1, 8>(k, [&](auto kc) {
    hipLaunchKernelGGL((sparse_aggregate_kernel<decltype(kc)::value>), dim3(grid), dim3(MULTI_STATE_BLOCK), 0, st, dst, base, up, (unsigned)n, accumulate);
  });
  FEDFR_LAUNCH_CHECK("sparse_aggregate");
  return FEDFR_OK;
}
