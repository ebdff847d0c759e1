// Train-mode BatchNorm (+PReLU) on the row-slab mapping (ew_rowslab.h): statistics finalize, apply, backward reduce / finalize / apply, and the
// PReLU(+bias) backward of sphnet that rides on the same kernels.  Per-channel partials are reduced through LDS and written as one row per
// workgroup (deterministic, no atomics), then finalised in fp64 by a tiny second kernel.  The algebra is bn_math.h's; the channel-sliced passes
// that skip the finalize launch are in bn_sliced.hip.
#include "ew.h"
#include "ew_rowslab.h"
#include "bn_math.h"
#include "gemm_dev.h"   // ProfScope: HIP-event timing of a launch on its stream (bench.py roofline leg); slots 20.. carry algorithmic bytes

// rows whose loads are issued together in the streaming loops: 4, and 2 where the per-channel register set is large — bn_bwd_reduce with a PReLU (24 more
// per-channel registers), bn_bwd_apply with a PReLU, an addend or the next BN's reduction (two waves beside wgrad9)
constexpr int kEwUnroll = 4, kEwUnrollAlpha = 2, kEwUnrollHeavy = 2;

static inline int rows_per_pass(int C) { return EW_THREADS / (C >> 3); }
static int slab_rows(int M, int C, int max_blocks) {
  const int rpp = rows_per_pass(C);
  long long rows = (long long)rpp * 8;
  const long long need = (M + max_blocks - 1) / max_blocks;
  if (rows < need) rows = need;
  rows = (rows + rpp - 1) / rpp * rpp;
  return (int)rows;
}
static int check_mc(int M, int C, const char* who) {
  if (M <= 0 || C <= 0 || (C & 7) || (C >> 3) > EW_THREADS) {
    fedfr_set_error("%s: unsupported shape M=%d C=%d (need C%%8==0, C<=2048)", who, M, C);
    return FEDFR_ERR_ARG;
  }
  return FEDFR_OK;
}

// =====================================================================================================
// forward BN finalize
// =====================================================================================================
// stage A: [P][W] -> [S][W] partial sums (W = ncols), block = 32 cols x 32 row-groups
__global__ __launch_bounds__(1024) void colsum_stage_kernel(const float* __restrict__ in, int P, int W,
                                                           float* __restrict__ out, int S) {
  __shared__ double red[32][33];
  const int cl = threadIdx.x & 31, rg = threadIdx.x >> 5;
  const int col = blockIdx.x * 32 + cl;
  const int slice = blockIdx.y;
  double s = 0.0;
  if (col < W)
    for (int row = slice + S * rg; row < P; row += S * 32) s += (double)in[(size_t)row * W + col];
  red[rg][cl] = s;
  __syncthreads();
  if (rg == 0 && col < W) {
    double t = 0.0;
#pragma unroll 8
    for (int i = 0; i < 32; ++i) t += red[i][cl];
    out[(size_t)slice * W + col] = (float)t;
  }
}

// ---- finalize, 8 channels per block ----------------------------------------------------------------
// P x 2C (or 3C) floats are 150-300 KB per CU when C/32 = 2..16 CUs pull them, at one CU's ~0.1 TB/s: the finalize is bound by per-CU
// bandwidth, not by latency.  So a block owns 8 channels (C/8 = 8..64 blocks), thread (row-group, half) loads one float4 per statistic
// and row with every load of a trip issued before the first add, sums in fp64, and the 128 row-groups meet in LDS.
constexpr int FIN_RG = 128;
template <int NS>
__device__ __forceinline__ void fin8_accumulate(const float* __restrict__ part, int P, int C, int c0, int ns_live, double (*tot)[8]) {
  __shared__ double red[NS * 8][FIN_RG + 1];
  const int half = threadIdx.x & 1, rg = threadIdx.x >> 1;
  const int W = NS * C;
  double acc[NS][4];
#pragma unroll
  for (int s = 0; s < NS; ++s)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[s][j] = 0.0;
  const float* base = part + c0 + half * 4;
  for (int r = rg; r < P; r += 2 * FIN_RG) {
    const int r1 = r + FIN_RG;
    const bool ok1 = r1 < P;
    float4 v0[NS], v1[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const bool live = s < ns_live;
      v0[s] = live ? *reinterpret_cast<const float4*>(base + (size_t)r * W + s * C) : make_float4(0.f, 0.f, 0.f, 0.f);
      v1[s] = (live && ok1) ? *reinterpret_cast<const float4*>(base + (size_t)r1 * W + s * C) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      acc[s][0] += (double)v0[s].x + (double)v1[s].x; acc[s][1] += (double)v0[s].y + (double)v1[s].y;
      acc[s][2] += (double)v0[s].z + (double)v1[s].z; acc[s][3] += (double)v0[s].w + (double)v1[s].w;
    }
  }
#pragma unroll
  for (int s = 0; s < NS; ++s)
#pragma unroll
    for (int j = 0; j < 4; ++j) red[s * 8 + half * 4 + j][rg] = acc[s][j];
  __syncthreads();
  // value v = (stat, channel) summed by 8 consecutive lanes: 16 entries each, then 3 xor steps inside the lane group
  const int v = threadIdx.x >> 3, k = threadIdx.x & 7;
  double t = 0.0;
  if (v < NS * 8) {
#pragma unroll
    for (int i = 0; i < FIN_RG / 8; ++i) t += red[v][i * 8 + k];
  }
  t += __shfl_xor(t, 1, 64);
  t += __shfl_xor(t, 2, 64);
  t += __shfl_xor(t, 4, 64);
  if (v < NS * 8 && k == 0) tot[v >> 3][v & 7] = t;
  __syncthreads();
}

__global__ __launch_bounds__(256) void bn_finalize8_kernel(const float* __restrict__ part, int P, int C, double count,
                                                          const float* __restrict__ gamma, const float* __restrict__ beta,
                                                          float* running_mean, float* running_var, float momentum, float eps,
                                                          float* scale, float* shift, float* save_mean, float* save_rstd) {
  __shared__ double tot[2][8];
  const int c0 = blockIdx.x * 8;
  fin8_accumulate<2>(part, P, C, c0, 2, tot);
  if (threadIdx.x < 8) {
    const int c = c0 + threadIdx.x;
    const float g = gamma ? gamma[c] : 1.f, b = beta ? beta[c] : 0.f;
    const BnFwdCoef k = bn_fwd_coef(tot[0][threadIdx.x], tot[1][threadIdx.x], 1.0 / count, eps, g, b);
    scale[c] = k.scale;
    shift[c] = k.shift;
    save_mean[c] = (float)k.mean;
    save_rstd[c] = (float)k.rstd;
    if (running_mean) bn_running_update(k, count, momentum, running_mean[c], running_var[c], &running_mean[c], &running_var[c]);
  }
}

int ew_bn_finalize(const float* partials, int P, int C, double count, const float* gamma, const float* beta,
                   float* running_mean, float* running_var, float momentum, float eps, float* scale, float* shift,
                   float* save_mean, float* save_rstd, float* tmp, hipStream_t st) {
  FEDFR_REQUIRE(C > 0 && (C & 7) == 0, "bn_finalize: unsupported C=%d (need C%%8==0, as every producer of partial rows)", C);
  FEDFR_REQUIRE(partials && P > 0 && scale && shift && save_mean && save_rstd, "bn_finalize: bad args");
  ProfScope prof(23, (double)P * 2 * C * 4, st);
  const float* src = partials;
  if (P > 1024) {
    FEDFR_REQUIRE(tmp != nullptr, "bn_finalize: P=%d needs a tmp buffer", P);
    const int S = 64, W = 2 * C;
    hipLaunchKernelGGL(colsum_stage_kernel, dim3(ceil_div(W, 32), S), dim3(1024), 0, st, partials, P, W, tmp, S);
    FEDFR_LAUNCH_CHECK("colsum_stage");
    src = tmp;
    P = S;
  }
  hipLaunchKernelGGL(bn_finalize8_kernel, dim3(C / 8), dim3(256), 0, st, src, P, C, count, gamma, beta,
                     running_mean, running_var, momentum, eps, scale, shift, save_mean, save_rstd);
  FEDFR_LAUNCH_CHECK("bn_finalize");
  return FEDFR_OK;
}

// =====================================================================================================
// forward BN apply (+PReLU) (+second normalised/identity input) (+stats of the result)
// =====================================================================================================
// X2 / STATS as template parameters: as runtime tests inside the row body they were (uniform) branches between the loads of a batch and
// in front of every store, and each branch ends the region the loads of kEwUnroll rows are scheduled in
template <bool X2, bool STATS>
__global__ __launch_bounds__(EW_THREADS) void bn_apply_kernel(BnApply p, int slab) {
  extern __shared__ float red[];   // [rpp][2C] when stats
  RowSlab rs(p.C);
  const int c0 = rs.c0;
  float sc1[8], sh1[8], al[8], sc2[8], sh2[8];
  load8f(p.sc1, c0, sc1, 1.f);
  load8f(p.sh1, c0, sh1, 0.f);
  load8f(p.alpha, c0, al, 1.f);
  load8f(p.sc2, c0, sc2, 1.f);
  load8f(p.sh2, c0, sh2, 0.f);
  const bool has_alpha = p.alpha != nullptr;
  float s[8], q[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) s[j] = q[j] = 0.f;
  rs.set_slab(p.M, slab);
  auto one = [&](int m, const uint4& v1, const uint4& v2) {
    const size_t off = (size_t)m * p.C + c0;
    float f[8];
    unpack8(v1, f);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float y = f[j] * sc1[j] + sh1[j];
      if (has_alpha) y = y > 0.f ? y : al[j] * y;
      f[j] = y;
    }
    if (X2) {
      float g[8];
      unpack8(v2, g);
#pragma unroll
      for (int j = 0; j < 8; ++j) f[j] += g[j] * sc2[j] + sh2[j];
    }
    const uint4 o = pack8(f);
    if (STATS) {
      float r[8];
      unpack8(o, r);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        s[j] += r[j];
        q[j] += r[j] * r[j];
      }
    }
    if (p.nchw_hw > 0) {
      const int img = m / p.nchw_hw, hw = m - img * p.nchw_hw;
      const bf16_t* ob = reinterpret_cast<const bf16_t*>(&o);
#pragma unroll
      for (int j = 0; j < 8; ++j) p.y[((size_t)img * p.C + c0 + j) * p.nchw_hw + hw] = ob[j];
    } else {
      *reinterpret_cast<uint4*>(p.y + off) = o;
    }
  };
  if (rs.active) {
    const int rpp = rs.rpp, mend = rs.mend;
    int m = rs.mbeg + rs.rl;
    for (; m + (kEwUnroll - 1) * rpp < mend; m += kEwUnroll * rpp) {    // loads of kEwUnroll rows first (see bn_bwd_reduce)
      uint4 v1[kEwUnroll], v2[kEwUnroll];
#pragma unroll
      for (int u = 0; u < kEwUnroll; ++u) {
        const size_t off = (size_t)(m + u * rpp) * p.C + c0;
        v1[u] = ew_ld16(p.x1 + off);
        v2[u] = X2 ? *reinterpret_cast<const uint4*>(p.x2 + off) : make_uint4(0, 0, 0, 0);
      }
#pragma unroll
      for (int u = 0; u < kEwUnroll; ++u) one(m + u * rpp, v1[u], v2[u]);
    }
    for (; m < mend; m += rpp) {
      const size_t off = (size_t)m * p.C + c0;
      one(m, *reinterpret_cast<const uint4*>(p.x1 + off), X2 ? *reinterpret_cast<const uint4*>(p.x2 + off) : make_uint4(0, 0, 0, 0));
    }
  }
  if (STATS) {
    const int W = 2 * p.C;
    if (rs.active) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        red[rs.rl * W + c0 + j] = s[j];
        red[rs.rl * W + p.C + c0 + j] = q[j];
      }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < W; i += EW_THREADS) {
      float t = 0.f;
      for (int r = 0; r < rs.rpp; ++r) t += red[r * W + i];
      p.stats[(size_t)rs.bid * W + i] = t;
    }
  }
}


int ew_bn_apply_grid(int M, int C) { return ceil_div(M, slab_rows(M, C, 1024)); }

int ew_bn_apply(const BnApply& p, hipStream_t st) {
  FEDFR_TRY(check_mc(p.M, p.C, "bn_apply"));
  FEDFR_REQUIRE(p.x1 && p.y, "bn_apply: null tensor");
  const int slab = slab_rows(p.M, p.C, 1024);
  const int grid = ceil_div(p.M, slab);
  const size_t lds = p.stats ? (size_t)rows_per_pass(p.C) * 2 * p.C * sizeof(float) : 0;
  ProfScope prof(20, (double)p.M * p.C * 2 * (p.x2 ? 3 : 2), st);
  if (p.x2) {
    if (p.stats) hipLaunchKernelGGL((bn_apply_kernel<true, true>), dim3(grid), dim3(EW_THREADS), lds, st, p, slab);
    else hipLaunchKernelGGL((bn_apply_kernel<true, false>), dim3(grid), dim3(EW_THREADS), lds, st, p, slab);
  } else {
    if (p.stats) hipLaunchKernelGGL((bn_apply_kernel<false, true>), dim3(grid), dim3(EW_THREADS), lds, st, p, slab);
    else hipLaunchKernelGGL((bn_apply_kernel<false, false>), dim3(grid), dim3(EW_THREADS), lds, st, p, slab);
  }
  FEDFR_LAUNCH_CHECK("bn_apply");
  return FEDFR_OK;
}

// =====================================================================================================
// backward BN (+PReLU)
// =====================================================================================================
// These kernels run on the main stream while the weight-gradient GEMMs occupy every CU from the aux stream (2 waves per SIMD x 104
// VGPRs, 128 KB LDS): what is left per CU is ~300 VGPRs per lane and 32 KB of LDS, so they are written to be small — one template
// instance per (PReLU, next-BN reduction) case so that unused per-channel vectors cost no registers, the normalisation folded into
// two per-channel coefficients, and the cross-row reduction done in registers (wave shuffles) before 4 rows per statistic meet in LDS.

// sums v[NV][8] (8 channels x NV statistics per thread) over all rows of the workgroup and writes dst[s * C + c].
// shfl (host-decided: C/8 is a power of two <= 64): rows of a wave meet by xor-shuffles, LDS holds [4 waves][NV C]; otherwise [rpp][NV C].
template <int NV>
__device__ __forceinline__ void ew_block_colsum(float (*v)[8], int C, int tpr, int rpp, int cl, int rl, bool active, bool shfl,
                                                float* red, float* dst) {
  const int W = NV * C, c0 = cl * 8;
  int rows = rpp, row = rl;
  if (shfl) {
    for (int o = 32; o >= tpr; o >>= 1)
#pragma unroll
      for (int s = 0; s < NV; ++s)
#pragma unroll
        for (int j = 0; j < 8; ++j) v[s][j] += __shfl_xor(v[s][j], o, 64);
    rows = EW_THREADS / 64;
    row = threadIdx.x >> 6;
    active = (threadIdx.x & 63) < tpr;
  }
  if (active) {
#pragma unroll
    for (int s = 0; s < NV; ++s)
#pragma unroll
      for (int j = 0; j < 8; ++j) red[row * W + s * C + c0 + j] = v[s][j];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < W; i += EW_THREADS) {
    float t = 0.f;
    for (int r = 0; r < rows; ++r) t += red[r * W + i];
    dst[i] = t;
  }
}
static inline bool ew_shfl_ok(int C) { const int tpr = C >> 3; return tpr <= 64 && (tpr & (tpr - 1)) == 0; }
static inline size_t ew_colsum_lds(int C, int nv) {
  return (size_t)(ew_shfl_ok(C) ? EW_THREADS / 64 : rows_per_pass(C)) * nv * C * sizeof(float);
}

// PReLU pre-activation z = G x + H: the forward's own (scale, shift) when the caller has them (same expression as bn_apply, so the
// mask is the forward's), else derived from gamma / rstd / mean / beta
__device__ __forceinline__ void ew_load_gh(const BnBwd& p, int c0, const float* mean, const float* rstd, float* G, float* H) {
  if (p.sc) {
    load8f(p.sc, c0, G, 1.f);
    load8f(p.sh, c0, H, 0.f);
  } else {
    float ga[8], be[8];
    load8f(p.gamma, c0, ga, 1.f);
    load8f(p.beta, c0, be, 0.f);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      G[j] = ga[j] * rstd[j];
      H[j] = be[j] - mean[j] * G[j];
    }
  }
}

// dy and x are read with plain loads (x could be non-temporal: tools/probe/hbm_stream_probe.hip; in the step it made no difference)
template <bool ALPHA>
__global__ __launch_bounds__(EW_THREADS, ALPHA ? 4 : 5) void bn_bwd_reduce_kernel(BnBwd p, int slab, int shfl) {
  extern __shared__ float red[];
  constexpr int UNR = ALPHA ? kEwUnrollAlpha : kEwUnroll;
  RowSlab rs(p.C);
  const int c0 = rs.c0;
  float mean[8], G[8], H[8], al[8];
  load8f(p.mean, c0, mean, 0.f);
  if (ALPHA) {
    float rstd[8];
    load8f(p.rstd, c0, rstd, 1.f);
    ew_load_gh(p, c0, mean, rstd, G, H);
    load8f(p.alpha, c0, al, 1.f);
  }
  float acc[3][8];                  // sum dz | sum dz (x - mean), scaled by rstd at the end = sum dz xhat | sum dy z over z <= 0
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[0][j] = acc[1][j] = acc[2][j] = 0.f;
  rs.set_slab(p.M, slab);
  auto accum = [&](const uint4& vd, const uint4& vx) {
    float dy[8], x[8];
    unpack8(vd, dy);
    unpack8(vx, x);
#pragma unroll
    for (int j = 0; j < 8; ++j) bn_bwd_sums<ALPHA>(dy[j], x[j], mean[j], G[j], H[j], al[j], acc[0][j], acc[1][j], acc[2][j]);
  };
  if (rs.active) {
    // UNR rows per trip with all their loads issued first: in the network dy / x come cold from HBM and one 16-B load
    // pair in flight per thread left the kernel latency-bound (2x its warm-cache time)
    const int rpp = rs.rpp, mend = rs.mend;
    int m = rs.mbeg + rs.rl;
    for (; m + (UNR - 1) * rpp < mend; m += UNR * rpp) {
      uint4 vd[UNR], vx[UNR];
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        const size_t off = (size_t)(m + u * rpp) * p.C + c0;
        vd[u] = uint4(*reinterpret_cast<const uint4*>(p.dy + off));     // (copied through a temporary: assigned directly, hipcc
        vx[u] = uint4(*reinterpret_cast<const uint4*>(p.x + off));      // schedules this loop differently — bf16 build, plain variant: 96 VGPRs, not 92; profiles/ew_split_resources_v1.txt)
      }
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        accum(vd[u], vx[u]);
        __builtin_amdgcn_sched_barrier(0);          // one row's temporaries at a time (the scheduler otherwise interleaves all four: +50 VGPRs)
      }
    }
    for (; m < mend; m += rpp) {
      const size_t off = (size_t)m * p.C + c0;
      accum(*reinterpret_cast<const uint4*>(p.dy + off), *reinterpret_cast<const uint4*>(p.x + off));
    }
  }
  {
    float rstd[8];
    load8f(p.rstd, c0, rstd, 1.f);
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[1][j] *= rstd[j];
  }
  ew_block_colsum<3>(acc, p.C, rs.tpr, rs.rpp, rs.cl, rs.rl, rs.active, shfl != 0, red, p.partials + (size_t)rs.bid * 3 * p.C);
}


// workgroups a row-slab bn_bwd_reduce / bn_bwd_apply launch aims for (= partial rows it leaves).  Round 3 swept both and the loads' cache policy
// (profiles/r03_ab_ew_rowslab_options_v1.txt): nothing moved the step, the sweep's switches are gone
// Round 6: the apply pass aims for 768 workgroups (2048 in rounds 3-5) = ONE dispatch round of its three-per-CU variants on 256 CUs, and a third of
// the partial rows for the finalize launch behind it: -0.03 ... -0.04 ms per step same-box on two boxes (profiles/r06_ab_bwd_apply_blocks_v1.txt; 512 and
// 1024, and 256 / 1024 for the reduce pass: equal)
constexpr int kEwReduceBlocks = 512, kEwBwdApplyBlocks = 768;
int ew_bn_bwd_grid(int M, int C) { return ceil_div(M, slab_rows(M, C, kEwReduceBlocks)); }

int ew_bn_bwd_reduce(const BnBwd& p, hipStream_t st) {
  FEDFR_TRY(check_mc(p.M, p.C, "bn_bwd_reduce"));
  FEDFR_REQUIRE(p.dy && p.x && p.partials, "bn_bwd_reduce: null tensor");   // mean / rstd null: 0 / 1 (bias + PReLU backward)
  FEDFR_REQUIRE(!p.sc == !p.sh, "bn_bwd_reduce: scale and shift come together");
  const int slab = slab_rows(p.M, p.C, kEwReduceBlocks);
  const int grid = ceil_div(p.M, slab);
  const size_t lds = ew_colsum_lds(p.C, 3);
  const int shfl = ew_shfl_ok(p.C) ? 1 : 0;
  ProfScope prof(21, (double)p.M * p.C * 2 * 2, st);
  if (p.alpha) hipLaunchKernelGGL(bn_bwd_reduce_kernel<true>, dim3(grid), dim3(EW_THREADS), lds, st, p, slab, shfl);
  else hipLaunchKernelGGL(bn_bwd_reduce_kernel<false>, dim3(grid), dim3(EW_THREADS), lds, st, p, slab, shfl);
  FEDFR_LAUNCH_CHECK("bn_bwd_reduce");
  return FEDFR_OK;
}

// coef [3][C] for the apply pass, dx = a dz + A x + B (bn_math.h: bn_bwd_coef)
__global__ __launch_bounds__(256) void bn_bwd_finalize8_kernel(const float* __restrict__ part, int P, int C, double count,
                                                              const float* gamma, const float* mean, const float* rstd, float* dgamma,
                                                              float* dbeta, float* dalpha, float* coef) {
  __shared__ double tot[3][8];
  const int c0 = blockIdx.x * 8;
  fin8_accumulate<3>(part, P, C, c0, dalpha ? 3 : 2, tot);      // the third statistic (sum dy z over z <= 0) only feeds dalpha
  if (threadIdx.x < 8) {
    const int c = c0 + threadIdx.x;
    const double t1 = tot[0][threadIdx.x], t2 = tot[1][threadIdx.x];
    if (dgamma) dgamma[c] = (float)t2;
    if (dbeta) dbeta[c] = (float)t1;
    if (dalpha) dalpha[c] = (float)tot[2][threadIdx.x];
    const float g = gamma ? gamma[c] : 1.f, r = rstd ? rstd[c] : 1.f, mu = mean ? mean[c] : 0.f;
    const BnBwdCoef k = bn_bwd_coef(t1, t2, 1.0 / count, g, r, mu);
    coef[c] = k.a;
    coef[C + c] = k.A;
    coef[2 * C + c] = k.B;
  }
}

int ew_bn_bwd_finalize(const float* partials, int P, int C, double count, const float* gamma, const float* mean, const float* rstd,
                       float* dgamma, float* dbeta, float* dalpha, float* coef, hipStream_t st) {
  FEDFR_REQUIRE(partials && P > 0 && C > 0 && (C & 7) == 0 && coef, "bn_bwd_finalize: bad args");
  ProfScope prof(24, (double)P * 3 * C * 4, st);
  hipLaunchKernelGGL(bn_bwd_finalize8_kernel, dim3(C / 8), dim3(256), 0, st, partials, P, C, count, gamma, mean, rstd,
                     dgamma, dbeta, dalpha, coef);
  FEDFR_LAUNCH_CHECK("bn_bwd_finalize");
  return FEDFR_OK;
}

struct BnBwdDiv {
  FastDiv dHW, dW;
};

template <bool ALPHA, int NX, bool ADD>      // NX: 0 none, 1 the next BatchNorm's reduction rides along, 2 ... and that BatchNorm has a PReLU behind it
__global__ __launch_bounds__(EW_THREADS, ((ALPHA && NX) || NX == 2) ? 3 : (ALPHA || NX || ADD) ? 4 : 5) void bn_bwd_apply_kernel(BnBwd p, BnBwdDiv dv, int slab, int shfl) {
  RowSlab rs(p.C);
  if (!rs.active && !NX) return;
  extern __shared__ float red[];                    // next BN's reduction (NX)
  constexpr int UNR = (ALPHA || NX || ADD) ? kEwUnrollHeavy : kEwUnroll;
  const int c0 = rs.c0;
  float ca[8], cA[8], cB[8], G[8], H[8], al[8], nmean[8], nG[8], nH[8], nal[8];
  float nacc[NX == 2 ? 3 : 2][8];                    // sum dz | sum dz (x_next - mean_next), scaled by rstd_next at the end | (NX == 2) sum dx z over z <= 0
  load8f(p.coef, c0, ca, 1.f);
  load8f(p.coef + p.C, c0, cA, 0.f);
  load8f(p.coef + 2 * p.C, c0, cB, 0.f);
  if (ALPHA) {
    float mean[8], rstd[8];
    load8f(p.sc ? nullptr : p.mean, c0, mean, 0.f);
    load8f(p.sc ? nullptr : p.rstd, c0, rstd, 1.f);
    ew_load_gh(p, c0, mean, rstd, G, H);
    load8f(p.alpha, c0, al, 1.f);
  }
  if (NX) {
    load8f(p.nmean, c0, nmean, 0.f);
#pragma unroll
    for (int j = 0; j < 8; ++j) nacc[0][j] = nacc[1][j] = 0.f;
    if (NX == 2) {
      load8f(p.nsc, c0, nG, 1.f);
      load8f(p.nsh, c0, nH, 0.f);
      load8f(p.nalpha, c0, nal, 1.f);
#pragma unroll
      for (int j = 0; j < 8; ++j) nacc[NX == 2 ? 2 : 0][j] = 0.f;
    }
  }
  rs.set_slab(p.M, slab);
  // every tensor of a row (dy, x, the identity-path addend, the next BN's input) is fetched in the batch in front of the arithmetic:
  // loads issued inside the per-row code wait out a full memory latency each
  auto one = [&](int m, const uint4& vd, const uint4& vx, const uint4& va, const uint4& vn) {
    const size_t off = (size_t)m * p.C + c0;
    float dy[8], x[8], o[8];
    unpack8(vd, dy);
    unpack8(vx, x);
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = bn_bwd_dx<ALPHA>(dy[j], x[j], G[j], H[j], al[j], ca[j], cA[j], cB[j]);
    if (ADD) {
      float a[8];
      unpack8(va, a);
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] += a[j];
    }
    if (p.add_up) {
      const unsigned img = fdiv((unsigned)m, dv.dHW);
      const unsigned rem = (unsigned)m - img * dv.dHW.d;
      const unsigned h = fdiv(rem, dv.dW), w = rem - h * dv.dW.d;
      if (((h | w) & 1u) == 0u) {
        const size_t uoff = (((size_t)img * (p.H >> 1) + (h >> 1)) * (p.W >> 1) + (w >> 1)) * p.C + c0;
        float a[8];
        unpack8(*reinterpret_cast<const uint4*>(p.add_up + uoff), a);
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] += a[j];
      }
    }
    const uint4 ov = pack8(o);
    *reinterpret_cast<uint4*>(p.dx + off) = ov;
    if (NX) {                                        // the next BN sees the bf16-rounded dx, exactly as its own reduce pass would
      float dn[8], xn[8];
      unpack8(ov, dn);
      unpack8(vn, xn);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (NX == 2) bn_bwd_sums<true>(dn[j], xn[j], nmean[j], nG[j], nH[j], nal[j], nacc[0][j], nacc[1][j], nacc[NX == 2 ? 2 : 0][j]);
        else bn_bwd_sums(dn[j], xn[j], nmean[j], nacc[0][j], nacc[1][j]);
      }
    }
  };
  const uint4 zero4 = make_uint4(0, 0, 0, 0);
  const int rpp = rs.rpp, mend = rs.mend;
  int m = rs.first_row();
  for (; m + (UNR - 1) * rpp < mend; m += UNR * rpp) {      // loads of UNR rows first (see bn_bwd_reduce)
    uint4 vd[UNR], vx[UNR], va[UNR], vn[UNR];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const size_t off = (size_t)(m + u * rpp) * p.C + c0;
      vd[u] = ew_ld16(p.dy + off);
      vx[u] = ew_ld16(p.x + off);
      va[u] = ADD ? *reinterpret_cast<const uint4*>(p.add + off) : zero4;
      vn[u] = NX ? *reinterpret_cast<const uint4*>(p.nx + off) : zero4;
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      one(m + u * rpp, vd[u], vx[u], va[u], vn[u]);
      __builtin_amdgcn_sched_barrier(0);            // see bn_bwd_reduce
    }
  }
  for (; m < mend; m += rpp) {
    const size_t off = (size_t)m * p.C + c0;
    one(m, *reinterpret_cast<const uint4*>(p.dy + off), *reinterpret_cast<const uint4*>(p.x + off),
        ADD ? *reinterpret_cast<const uint4*>(p.add + off) : zero4, NX ? *reinterpret_cast<const uint4*>(p.nx + off) : zero4);
  }
  if (NX) {
    float nrstd[8];
    load8f(p.nrstd, c0, nrstd, 1.f);
#pragma unroll
    for (int j = 0; j < 8; ++j) nacc[1][j] *= nrstd[j];
    float* row = p.npart + (size_t)rs.bid * 3 * p.C;
    if (NX == 2) {
      ew_block_colsum<3>(nacc, p.C, rs.tpr, rs.rpp, rs.cl, rs.rl, rs.active, shfl != 0, red, row);
    } else {
      ew_block_colsum<2>(nacc, p.C, rs.tpr, rs.rpp, rs.cl, rs.rl, rs.active, shfl != 0, red, row);
      for (int i = threadIdx.x; i < p.C; i += EW_THREADS) row[2 * p.C + i] = 0.f;
    }
  }
}


int ew_bn_bwd_apply_grid(int M, int C) { return ceil_div(M, slab_rows(M, C, kEwBwdApplyBlocks)); }

int ew_bn_bwd_apply(const BnBwd& p, hipStream_t st) {
  FEDFR_TRY(check_mc(p.M, p.C, "bn_bwd_apply"));
  FEDFR_REQUIRE(p.dy && p.x && p.coef && p.dx, "bn_bwd_apply: null tensor");
  FEDFR_REQUIRE(!p.sc == !p.sh, "bn_bwd_apply: scale and shift come together");
  BnBwdDiv dv;
  dv.dHW = make_fastdiv(1);
  dv.dW = make_fastdiv(1);
  if (p.add_up) {
    FEDFR_REQUIRE(p.H > 0 && p.W > 0 && !(p.H & 1) && !(p.W & 1) && p.M % (p.H * p.W) == 0, "bn_bwd_apply: add_up needs even H, W");
    dv.dHW = make_fastdiv((unsigned)(p.H * p.W));
    dv.dW = make_fastdiv((unsigned)p.W);
  }
  if (p.nx) FEDFR_REQUIRE(p.nmean && p.nrstd && p.npart, "bn_bwd_apply: next-BN reduction needs mean / rstd / partials");
  const bool nxa = p.nx && p.nalpha;
  if (nxa) FEDFR_REQUIRE(p.nsc && p.nsh && !p.alpha && !p.add, "bn_bwd_apply: the PReLU form of the next-BN reduction needs that BN's (scale, shift) and serves the plain variant only");
  const int slab = slab_rows(p.M, p.C, kEwBwdApplyBlocks);
  const dim3 grid(ceil_div(p.M, slab));
  const size_t lds = p.nx ? ew_colsum_lds(p.C, nxa ? 3 : 2) : 0;
  const int shfl = ew_shfl_ok(p.C) ? 1 : 0;
#define BWD_APPLY(A, N, D) hipLaunchKernelGGL((bn_bwd_apply_kernel<A, N, D>), grid, dim3(EW_THREADS), lds, st, p, dv, slab, shfl)
  const int variant = nxa ? 8 : ((p.alpha ? 4 : 0) | (p.nx ? 2 : 0) | (p.add ? 1 : 0));
  // algorithmic bytes: dy + x read, dx written, + the identity addend (compact when up-sampled), + the next BN's input when its reduction rides along
  ProfScope prof(22, (double)p.M * p.C * 2 * (3.0 + (p.add ? 1.0 : 0.0) + (p.add_up ? 0.25 : 0.0) + (p.nx ? 1.0 : 0.0)), st);
  switch (variant) {
    case 0: BWD_APPLY(false, 0, false); break;
    case 1: BWD_APPLY(false, 0, true); break;
    case 2: BWD_APPLY(false, 1, false); break;
    case 3: BWD_APPLY(false, 1, true); break;
    case 4: BWD_APPLY(true, 0, false); break;
    case 5: BWD_APPLY(true, 0, true); break;
    case 6: BWD_APPLY(true, 1, false); break;
    case 7: BWD_APPLY(true, 1, true); break;
    default: BWD_APPLY(false, 2, false); break;
  }
#undef BWD_APPLY
  FEDFR_LAUNCH_CHECK("bn_bwd_apply");
  return FEDFR_OK;
}

int ew_bn_bwd_rowslab(const BnBwd& p, int rows_in, double count, float* dgamma, float* dbeta, float* dalpha, bool coef_only, hipStream_t st) {
  if (rows_in <= 0) FEDFR_TRY(ew_bn_bwd_reduce(p, st));      // else: the producing pass already wrote the partials
  FEDFR_TRY(ew_bn_bwd_finalize(p.partials, rows_in > 0 ? rows_in : ew_bn_bwd_grid(p.M, p.C), p.C, count, p.gamma, p.mean, p.rstd, dgamma, dbeta,
                               dalpha, const_cast<float*>(p.coef), st));      // (coef: const to the apply kernel that reads it, written here)
  return coef_only ? FEDFR_OK : ew_bn_bwd_apply(p, st);
}

// =====================================================================================================
// bias + PReLU backward without normalisation (sphnet: conv(+bias) -> PReLU, reference backbones/sphnet.py:4-13, :53-60):
// z = x + bias, dz = dy * (z > 0 ? 1 : alpha), dbias = sum dz, dalpha = sum dy * z [z <= 0], dx = dz (+ add).
// Runs on the BN-backward kernels with mean = 0, rstd = 1, gamma = 1, beta = bias and the coefficients (1, 0, 0).
// =====================================================================================================
__global__ __launch_bounds__(256) void prelu_bwd_finalize_kernel(const float* __restrict__ part, int P, int C, float* dbias,
                                                                float* dalpha, float* coef) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  double s1 = 0.0, s3 = 0.0;
  for (int r = 0; r < P; ++r) {
    s1 += (double)part[(size_t)r * 3 * C + c];
    s3 += (double)part[(size_t)r * 3 * C + 2 * C + c];
  }
  if (dbias) dbias[c] = (float)s1;
  if (dalpha) dalpha[c] = (float)s3;
  coef[c] = 1.f;
  coef[C + c] = 0.f;
  coef[2 * C + c] = 0.f;
}
int ew_bias_prelu_bwd(const bf16_t* dy, const bf16_t* x, const float* bias, const float* alpha, int M, int C, float* partials,
                      float* coef, float* dbias, float* dalpha, const bf16_t* add, bf16_t* dx, hipStream_t st) {
  FEDFR_REQUIRE(alpha && coef, "bias_prelu_bwd: alpha and coef are required");
  BnBwd p{};
  p.dy = dy; p.x = x; p.beta = bias; p.alpha = alpha; p.M = M; p.C = C; p.partials = partials; p.coef = coef; p.add = add; p.dx = dx;
  FEDFR_TRY(ew_bn_bwd_reduce(p, st));
  hipLaunchKernelGGL(prelu_bwd_finalize_kernel, dim3(ceil_div(C, 256)), dim3(256), 0, st, partials, ew_bn_bwd_grid(M, C), C, dbias, dalpha, coef);
  FEDFR_LAUNCH_CHECK("prelu_bwd_finalize");
  return ew_bn_bwd_apply(p, st);
}

// The same backward as ONE streaming pass (round 3; the sphnet plan, net_sph.inc): unlike a BatchNorm's, a PReLU's parameter sums do not
// feed its input gradient, so dz is written while the sums are gathered and the finalize runs off the critical path.
//   g = dy (+ add);  z = x + bias;  dz = g * (z > 0 ? 1 : alpha);  rows[blk] = (sum dz | sum g z over z <= 0);  optional gsum = g (bf16)
struct PreluBwdP {
  const bf16_t *dy, *add, *x;
  const float *bias, *alpha;
  int M, C;
  bf16_t *gsum, *dz;
  float* rows;
};
template <bool ADD>
__global__ __launch_bounds__(EW_THREADS) void prelu_bwd_pass_kernel(PreluBwdP p, int slab, int shfl) {
  extern __shared__ float red[];
  RowSlab rs(p.C);
  const int c0 = rs.c0;
  float bi[8], al[8];
  load8f(p.bias, c0, bi, 0.f);
  load8f(p.alpha, c0, al, 1.f);
  float acc[2][8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[0][j] = acc[1][j] = 0.f;
  rs.set_slab(p.M, slab);
  auto one = [&](int m, const uint4& vd, const uint4& va, const uint4& vx) {
    const size_t off = (size_t)m * p.C + c0;
    float g[8], x[8], o[8];
    unpack8(vd, g);
    unpack8(vx, x);
    if (ADD) {
      float a[8];
      unpack8(va, a);
#pragma unroll
      for (int j = 0; j < 8; ++j) g[j] += a[j];
      const uint4 gs = pack8(g);                     // the identity-path gradient the next block adds to is the bf16-rounded sum ...
      *reinterpret_cast<uint4*>(p.gsum + off) = gs;
      unpack8(gs, g);                                // ... and so is what this PReLU sees (as the two-pass form: add pass, then PReLU pass)
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float z = x[j] + bi[j];
      const float dz = bn_prelu_dz(g[j], z, al[j], acc[1][j]);
      acc[0][j] += dz;
      o[j] = dz;
    }
    const uint4 ov = pack8(o);
    *reinterpret_cast<uint4*>(p.dz + off) = ov;
  };
  const uint4 zero4 = make_uint4(0, 0, 0, 0);
  constexpr int UNR = kEwUnroll;
  const int rpp = rs.rpp, mend = rs.mend;
  int m = rs.first_row();
  for (; m + (UNR - 1) * rpp < mend; m += UNR * rpp) {
    uint4 vd[UNR], va[UNR], vx[UNR];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const size_t off = (size_t)(m + u * rpp) * p.C + c0;
      vd[u] = *reinterpret_cast<const uint4*>(p.dy + off);
      va[u] = ADD ? *reinterpret_cast<const uint4*>(p.add + off) : zero4;
      vx[u] = ew_ld16(p.x + off);
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      one(m + u * rpp, vd[u], va[u], vx[u]);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  for (; m < mend; m += rpp) {
    const size_t off = (size_t)m * p.C + c0;
    one(m, *reinterpret_cast<const uint4*>(p.dy + off), ADD ? *reinterpret_cast<const uint4*>(p.add + off) : zero4,
        *reinterpret_cast<const uint4*>(p.x + off));
  }
  // NOTE dbias of the two-pass form sums the UNROUNDED dz; so does this (acc[0] adds dz before the bf16 pack)
  ew_block_colsum<2>(acc, p.C, rs.tpr, rs.rpp, rs.cl, rs.rl, rs.active, shfl != 0, red, p.rows + (size_t)rs.bid * 2 * p.C);
}
int ew_prelu_bwd_rows(int M, int C) { return ceil_div(M, slab_rows(M, C, 512)); }
int ew_prelu_bwd_pass(const bf16_t* dy, const bf16_t* add, const bf16_t* x, const float* bias, const float* alpha, int M, int C, bf16_t* gsum,
                      bf16_t* dz, float* rows, hipStream_t st) {
  FEDFR_TRY(check_mc(M, C, "prelu_bwd_pass"));
  FEDFR_REQUIRE(dy && x && alpha && dz && rows && (!add || gsum), "prelu_bwd_pass: null tensor");
  const int slab = slab_rows(M, C, 512);
  const int grid = ceil_div(M, slab);
  const size_t lds = ew_colsum_lds(C, 2);
  const int shfl = ew_shfl_ok(C) ? 1 : 0;
  PreluBwdP p{dy, add, x, bias, alpha, M, C, gsum, dz, rows};
  ProfScope prof(22, (double)M * C * 2 * (add ? 5.0 : 3.0), st);
  if (add) hipLaunchKernelGGL(prelu_bwd_pass_kernel<true>, dim3(grid), dim3(EW_THREADS), lds, st, p, slab, shfl);
  else hipLaunchKernelGGL(prelu_bwd_pass_kernel<false>, dim3(grid), dim3(EW_THREADS), lds, st, p, slab, shfl);
  FEDFR_LAUNCH_CHECK("prelu_bwd_pass");
  return FEDFR_OK;
}
// 8 channels per workgroup, every row load of a trip in flight (fin8_accumulate): the first version walked the rows one thread per channel
// from 1-2 workgroups and took 173 us per PReLU on the sphnet plan's weight-gradient stream (62 launches = 10.7 ms per step)
__global__ __launch_bounds__(256) void prelu_rows_finalize_kernel(const float* __restrict__ rows, int P, int C, float* dbias, float* dalpha) {
  __shared__ double tot[2][8];
  const int c0 = blockIdx.x * 8;
  fin8_accumulate<2>(rows, P, C, c0, 2, tot);
  if (threadIdx.x < 8) {
    const int c = c0 + threadIdx.x;
    if (dbias) dbias[c] = (float)tot[0][threadIdx.x];
    if (dalpha) dalpha[c] = (float)tot[1][threadIdx.x];
  }
}
__global__ __launch_bounds__(256) void prelu_rows_finalize_multi_kernel(const unsigned char* __restrict__ base, float* __restrict__ grads, PreluFinTable t) {
  __shared__ double tot[3][8];
  int i = 0;
  while (i + 1 < t.n && (int)blockIdx.x >= t.e[i + 1].blk0) ++i;        // (workgroup-uniform: a scan of at most 63 scalars)
  const PreluFinEntry e = t.e[i];
  const int c0 = ((int)blockIdx.x - e.blk0) * 8;
  if (e.nv_row == 3) fin8_accumulate<3>(reinterpret_cast<const float*>(base + e.rows_off), e.P, e.C, c0, 2, tot);
  else fin8_accumulate<2>(reinterpret_cast<const float*>(base + e.rows_off), e.P, e.C, c0, 2, tot);
  if (threadIdx.x < 8) {
    const int c = c0 + threadIdx.x;
    if (e.dbias_off >= 0) grads[e.dbias_off + c] = (float)tot[0][threadIdx.x];
    grads[e.dalpha_off + c] = (float)tot[1][threadIdx.x];
  }
}
int ew_prelu_bwd_finalize_multi(const unsigned char* base, float* grads, const PreluFinTable& t, hipStream_t st) {
  FEDFR_REQUIRE(base && grads && t.n > 0 && t.n <= kMaxPreluFin && t.blocks > 0, "prelu_bwd_finalize_multi: bad table");
  hipLaunchKernelGGL(prelu_rows_finalize_multi_kernel, dim3(t.blocks), dim3(256), 0, st, base, grads, t);
  FEDFR_LAUNCH_CHECK("prelu_bwd_finalize_multi");
  return FEDFR_OK;
}
int ew_prelu_bwd_finalize(const float* rows, int P, int C, float* dbias, float* dalpha, hipStream_t st) {
  FEDFR_REQUIRE(rows && P > 0 && C > 0, "prelu_bwd_finalize: bad args");
  FEDFR_REQUIRE((C & 7) == 0, "prelu_bwd_finalize: C %% 8");
  hipLaunchKernelGGL(prelu_rows_finalize_kernel, dim3(C / 8), dim3(256), 0, st, rows, P, C, dbias, dalpha);
  FEDFR_LAUNCH_CHECK("prelu_bwd_finalize");
  return FEDFR_OK;
}
