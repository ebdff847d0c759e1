// The elementwise rest of ew.h: split-K slab reductions (the weight-gradient traffic bench.py stamps this file for), casts, weight shadows and
// layout conversions, input preprocessing and padding, dropout, eval-mode BatchNorm coefficients and BatchNorm1d.  The train-mode BatchNorm
// passes are in bn_rowslab.hip / bn_sliced.hip, the stem in stem.hip.
#include "ew.h"
#include "gemm_dev.h"   // ProfScope: HIP-event timing of a launch on its stream (bench.py roofline leg); slots 20.. carry algorithmic bytes

// =====================================================================================================
// eval-mode BatchNorm coefficients
// =====================================================================================================
__global__ __launch_bounds__(256) void bn_eval_coeffs_multi_kernel(const float* __restrict__ params, const float* __restrict__ bufs,
                                                                  float* __restrict__ save, BnEvalTable t) {
  const BnEvalEntry e = t.e[blockIdx.x];
  for (int c = blockIdx.y * 256 + threadIdx.x; c < e.C; c += gridDim.y * 256) {
    const float rstd = 1.f / sqrtf(bufs[e.rv_off + c] + t.eps);
    const float g = e.g_off >= 0 ? params[e.g_off + c] : 1.f, b = params[e.b_off + c];
    save[e.save_off + c] = g * rstd;                                   // scale
    save[e.save_off + e.C + c] = b - bufs[e.rm_off + c] * g * rstd;    // shift
    save[e.save_off + 2 * e.C + c] = bufs[e.rm_off + c];               // mean / rstd as the backward pass of a training net with frozen
    save[e.save_off + 3 * e.C + c] = rstd;                             // BatchNorms reads them (freeze_BN, iresnet.py:140-147)
  }
}
int ew_bn_eval_coeffs_multi(const float* params, const float* bufs, float* save, const BnEvalTable& t, hipStream_t st) {
  FEDFR_REQUIRE(params && bufs && save && t.n > 0 && t.n <= kMaxBnEvalEntries, "bn_eval_coeffs_multi: bad args");
  hipLaunchKernelGGL(bn_eval_coeffs_multi_kernel, dim3(t.n, 2), dim3(256), 0, st, params, bufs, save, t);
  FEDFR_LAUNCH_CHECK("bn_eval_coeffs_multi");
  return FEDFR_OK;
}

// =====================================================================================================
// BatchNorm1d on fp32 [B][C]
// =====================================================================================================
// BatchNorm1d kernels: 64 channels x BN1D_RG row groups per workgroup (one thread per channel walking all B rows three times was a
// 60 us latency chain for a 128 x 512 tensor); fp64 sums, the row groups meet in LDS.
constexpr int BN1D_RG = 8;
__device__ __forceinline__ double bn1d_rg_sum(double v, double (*red)[64], int rg, int cl) {
  __syncthreads();                                   // previous use of red is over
  red[rg][cl] = v;
  __syncthreads();
  double t = 0.0;
#pragma unroll
  for (int i = 0; i < BN1D_RG; ++i) t += red[i][cl];
  return t;
}
// CACHE (B <= BN1D_NR x BN1D_RG rows): a thread's rows are fetched ONCE, all loads in flight together, and the three passes run on registers
// (round 4: the kernel sits on the serial head chain between the forward and the backward pass; same operations in the same order)
constexpr int BN1D_NR = 16;
template <bool CACHE>
__global__ __launch_bounds__(64 * BN1D_RG) void bn1d_fwd_kernel(const float* x, float* y, int B, int C, const float* gamma, const float* beta,
                                float* rm, float* rv, float momentum, float eps, int training, float* save_mean,
                                float* save_rstd) {
  __shared__ double red[BN1D_RG][64];
  const int cl = threadIdx.x & 63, rg = threadIdx.x >> 6;
  const int c = min(blockIdx.x * 64 + cl, C - 1);
  const bool own = blockIdx.x * 64 + cl < C && rg == 0;
  float xv[CACHE ? BN1D_NR : 1];
  if constexpr (CACHE) {
#pragma unroll
    for (int j = 0; j < BN1D_NR; ++j) {
      const int b = rg + j * BN1D_RG;
      xv[j] = x[(size_t)min(b, B - 1) * C + c];
    }
  }
  float mean, rstd;
  if (training) {
    double s = 0.0;
    if constexpr (CACHE) {
#pragma unroll
      for (int j = 0; j < BN1D_NR; ++j) if (rg + j * BN1D_RG < B) s += (double)xv[j];
    } else {
      for (int b = rg; b < B; b += BN1D_RG) s += (double)x[(size_t)b * C + c];
    }
    const double mu = bn1d_rg_sum(s, red, rg, cl) / B;
    double v = 0.0;
    if constexpr (CACHE) {
#pragma unroll
      for (int j = 0; j < BN1D_NR; ++j) if (rg + j * BN1D_RG < B) { const double d = (double)xv[j] - mu; v += d * d; }
    } else {
      for (int b = rg; b < B; b += BN1D_RG) {
        const double d = (double)x[(size_t)b * C + c] - mu;
        v += d * d;
      }
    }
    v = bn1d_rg_sum(v, red, rg, cl);
    const double var = v / B;
    mean = (float)mu;
    rstd = (float)(1.0 / sqrt(var + (double)eps));
    if (own) {
      const double unb = B > 1 ? v / (B - 1) : var;
      rm[c] = (float)((1.0 - momentum) * (double)rm[c] + momentum * mu);
      rv[c] = (float)((1.0 - momentum) * (double)rv[c] + momentum * unb);
    }
  } else {
    mean = rm[c];
    rstd = 1.f / sqrtf(rv[c] + eps);
  }
  if (save_mean && own) {
    save_mean[c] = mean;
    save_rstd[c] = rstd;
  }
  if (blockIdx.x * 64 + cl >= C) return;
  const float g = gamma ? gamma[c] : 1.f, bt = beta ? beta[c] : 0.f;
  if constexpr (CACHE) {
#pragma unroll
    for (int j = 0; j < BN1D_NR; ++j) {
      const int b = rg + j * BN1D_RG;
      if (b < B) y[(size_t)b * C + c] = (xv[j] - mean) * rstd * g + bt;
    }
  } else {
    for (int b = rg; b < B; b += BN1D_RG) y[(size_t)b * C + c] = (x[(size_t)b * C + c] - mean) * rstd * g + bt;
  }
}

int ew_bn1d_fwd(const float* x, float* y, int B, int C, const float* gamma, const float* beta, float* rm, float* rv,
                float momentum, float eps, int training, float* save_mean, float* save_rstd, hipStream_t st) {
  FEDFR_REQUIRE(x && y && B > 0 && C > 0 && rm && rv, "bn1d_fwd: bad args");
  if (B <= BN1D_NR * BN1D_RG)
    hipLaunchKernelGGL(bn1d_fwd_kernel<true>, dim3(ceil_div(C, 64)), dim3(64 * BN1D_RG), 0, st, x, y, B, C, gamma, beta, rm, rv, momentum, eps,
                       training, save_mean, save_rstd);
  else
    hipLaunchKernelGGL(bn1d_fwd_kernel<false>, dim3(ceil_div(C, 64)), dim3(64 * BN1D_RG), 0, st, x, y, B, C, gamma, beta, rm, rv, momentum, eps,
                       training, save_mean, save_rstd);
  FEDFR_LAUNCH_CHECK("bn1d_fwd");
  return FEDFR_OK;
}

template <bool CACHE>
__global__ __launch_bounds__(64 * BN1D_RG) void bn1d_bwd_kernel(const float* dy, const float* x, float* dx, int B, int C, const float* gamma,
                                const float* mean, const float* rstd, float* dbeta, float* dx_colsum, bf16_t* dxb,
                                bf16_t* dxbt, int ldt, int frozen) {
  __shared__ double red[BN1D_RG][64];
  const int cl = threadIdx.x & 63, rg = threadIdx.x >> 6;
  const int c = min(blockIdx.x * 64 + cl, C - 1);
  const bool valid = blockIdx.x * 64 + cl < C, own = valid && rg == 0;
  float dv[CACHE ? BN1D_NR : 1], xv[CACHE ? BN1D_NR : 1];
  if constexpr (CACHE) {
#pragma unroll
    for (int j = 0; j < BN1D_NR; ++j) {
      const size_t o = (size_t)min(rg + j * BN1D_RG, B - 1) * C + c;
      dv[j] = dy[o];
      xv[j] = x[o];
    }
  }
  const float mu = mean[c], rs = rstd[c], g = gamma ? gamma[c] : 1.f;
  double s1 = 0.0, s2 = 0.0;
  if constexpr (CACHE) {
#pragma unroll
    for (int j = 0; j < BN1D_NR; ++j)
      if (rg + j * BN1D_RG < B) {
        s1 += dv[j];
        s2 += (double)dv[j] * (double)((xv[j] - mu) * rs);
      }
  } else {
    for (int b = rg; b < B; b += BN1D_RG) {
      const float d = dy[(size_t)b * C + c];
      s1 += d;
      s2 += (double)d * (double)((x[(size_t)b * C + c] - mu) * rs);
    }
  }
  s1 = bn1d_rg_sum(s1, red, rg, cl);
  s2 = bn1d_rg_sum(s2, red, rg, cl);
  const float m1 = frozen ? 0.f : (float)(s1 / B), m2 = frozen ? 0.f : (float)(s2 / B);     // frozen: statistics were constants, dx = g rstd dy
  if (dbeta && own) dbeta[c] = (float)s1;
  double cs = 0.0;
  auto one = [&](int b, float d, float xx) {
    const float xh = (xx - mu) * rs;
    const float v = g * rs * (d - m1 - xh * m2);
    dx[(size_t)b * C + c] = v;
    cs += v;
    if (dxb) dxb[(size_t)b * C + c] = f2bf(v);
    if (dxbt) dxbt[(size_t)c * ldt + b] = f2bf(v);
  };
  if (valid) {
    if constexpr (CACHE) {
#pragma unroll
      for (int j = 0; j < BN1D_NR; ++j) if (rg + j * BN1D_RG < B) one(rg + j * BN1D_RG, dv[j], xv[j]);
    } else {
      for (int b = rg; b < B; b += BN1D_RG) one(b, dy[(size_t)b * C + c], x[(size_t)b * C + c]);
    }
  }
  cs = bn1d_rg_sum(cs, red, rg, cl);
  if (dx_colsum && own) dx_colsum[c] = (float)cs;
}

int ew_bn1d_bwd(const float* dy, const float* x, float* dx, int B, int C, const float* gamma, const float* mean,
                const float* rstd, float* dbeta, float* dx_colsum, bf16_t* dxb, bf16_t* dxbt, int ldt, hipStream_t st, int frozen) {
  FEDFR_REQUIRE(dy && x && dx && B > 0 && C > 0 && mean && rstd, "bn1d_bwd: bad args");
  if (B <= BN1D_NR * BN1D_RG)
    hipLaunchKernelGGL(bn1d_bwd_kernel<true>, dim3(ceil_div(C, 64)), dim3(64 * BN1D_RG), 0, st, dy, x, dx, B, C, gamma, mean, rstd, dbeta,
                       dx_colsum, dxb, dxbt, ldt, frozen);
  else
    hipLaunchKernelGGL(bn1d_bwd_kernel<false>, dim3(ceil_div(C, 64)), dim3(64 * BN1D_RG), 0, st, dy, x, dx, B, C, gamma, mean, rstd, dbeta,
                       dx_colsum, dxb, dxbt, ldt, frozen);
  FEDFR_LAUNCH_CHECK("bn1d_bwd");
  return FEDFR_OK;
}

// =====================================================================================================
// split-K slab reductions, casts, transposes
// =====================================================================================================
// blockIdx.y = 1 (ew_reduce_slabs2): the second (dst, slabs) pair of the launch, same geometry
__global__ void reduce_slabs_kernel(float* dst, const float* slabs, int nsplit, size_t n4, const float* bias, int bias_n, float* dst1,
                                    const float* slabs1) {
  if (blockIdx.y) { dst = dst1; slabs = slabs1; }
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    float4 a = reinterpret_cast<const float4*>(slabs)[i];
    for (int s = 1; s < nsplit; ++s) {
      const float4 b = reinterpret_cast<const float4*>(slabs + (size_t)s * n4 * 4)[i];
      a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
    }
    if (bias) {
      const int c = (int)((i * 4) % (size_t)bias_n);
      a.x += bias[c]; a.y += bias[c + 1]; a.z += bias[c + 2]; a.w += bias[c + 3];
    }
    reinterpret_cast<float4*>(dst)[i] = a;
  }
}
// many slabs of a small tensor (the 64-channel layers' weight gradients arrive as 128 slabs of 147 KB): one thread per output walking
// all slabs is a serial chain of 128 loads on 9 K threads (93 us).  Here 8 lanes share an output (slab s goes to lane s % 8, four loads
// in flight each) and meet in LDS in a fixed order.
__global__ __launch_bounds__(256) void reduce_slabs_wide_kernel(float* dst, const float* slabs, int nsplit, size_t n4, const float* bias, int bias_n,
                                                                float* dst1, const float* slabs1) {
  if (blockIdx.y) { dst = dst1; slabs = slabs1; }
  __shared__ float4 red[8][32];
  const int o = threadIdx.x & 31, q = threadIdx.x >> 5;
  const size_t i = (size_t)blockIdx.x * 32 + o;
  float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
  if (i < n4) {
    const float4* src = reinterpret_cast<const float4*>(slabs) + i;
    int sidx = q;
    for (; sidx + 24 < nsplit; sidx += 32) {
      const float4 b0 = src[(size_t)sidx * n4], b1 = src[(size_t)(sidx + 8) * n4], b2 = src[(size_t)(sidx + 16) * n4], b3 = src[(size_t)(sidx + 24) * n4];
      a.x += (b0.x + b1.x) + (b2.x + b3.x); a.y += (b0.y + b1.y) + (b2.y + b3.y);
      a.z += (b0.z + b1.z) + (b2.z + b3.z); a.w += (b0.w + b1.w) + (b2.w + b3.w);
    }
    for (; sidx < nsplit; sidx += 8) {
      const float4 b = src[(size_t)sidx * n4];
      a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
    }
  }
  red[q][o] = a;
  __syncthreads();
  if (q == 0 && i < n4) {
#pragma unroll
    for (int k = 1; k < 8; ++k) {
      const float4 b = red[k][o];
      a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
    }
    if (bias) {
      const int c = (int)((i * 4) % (size_t)bias_n);
      a.x += bias[c]; a.y += bias[c + 1]; a.z += bias[c + 2]; a.w += bias[c + 3];
    }
    reinterpret_cast<float4*>(dst)[i] = a;
  }
}
static int reduce_slabs_launch(float* dst, const float* slabs, float* dst1, const float* slabs1, int nsplit, size_t n, const float* bias, int bias_n,
                               hipStream_t st) {
  FEDFR_REQUIRE(dst && slabs && nsplit > 0 && n > 0 && (n & 3) == 0, "reduce_slabs: bad args (n%%4)");
  if (bias) FEDFR_REQUIRE((bias_n & 3) == 0 && bias_n > 0, "reduce_slabs: bias_n%%4");
  const size_t n4 = n / 4;
  const unsigned ny = dst1 ? 2 : 1;
  ProfScope prof(25, (double)n * 4 * (nsplit + 1) * ny, st);
  if (nsplit >= 16 && n4 <= 65536) {
    hipLaunchKernelGGL(reduce_slabs_wide_kernel, dim3((unsigned)((n4 + 31) / 32), ny), dim3(256), 0, st, dst, slabs, nsplit, n4, bias, bias_n, dst1, slabs1);
    FEDFR_LAUNCH_CHECK("reduce_slabs_wide");
    return FEDFR_OK;
  }
  const int grid = (int)((n4 + 255) / 256 > 2048 ? 2048 : (n4 + 255) / 256);
  hipLaunchKernelGGL(reduce_slabs_kernel, dim3(grid, ny), dim3(256), 0, st, dst, slabs, nsplit, n4, bias, bias_n, dst1, slabs1);
  FEDFR_LAUNCH_CHECK("reduce_slabs");
  return FEDFR_OK;
}
int ew_reduce_slabs(float* dst, const float* slabs, int nsplit, size_t n, const float* bias, int bias_n, hipStream_t st) {
  return reduce_slabs_launch(dst, slabs, nullptr, nullptr, nsplit, n, bias, bias_n, st);
}
// two slab sets of the same geometry (the two 3x3 weight gradients of a residual block) in one launch
int ew_reduce_slabs2(float* dst0, const float* slabs0, float* dst1, const float* slabs1, int nsplit, size_t n, hipStream_t st) {
  FEDFR_REQUIRE(dst1 && slabs1, "reduce_slabs2: null second pair");
  return reduce_slabs_launch(dst0, slabs0, dst1, slabs1, nsplit, n, nullptr, 0, st);
}


__global__ void cast_f32_bf16_kernel(const float* src, bf16_t* dst, size_t n) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const size_t n8 = n / 8;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += stride) {
    const float4 a = reinterpret_cast<const float4*>(src)[2 * i], b = reinterpret_cast<const float4*>(src)[2 * i + 1];
    uint4 o;
    o.x = pack_bf2(a.x, a.y); o.y = pack_bf2(a.z, a.w); o.z = pack_bf2(b.x, b.y); o.w = pack_bf2(b.z, b.w);
    reinterpret_cast<uint4*>(dst)[i] = o;
  }
  for (size_t i = n8 * 8 + (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) dst[i] = f2bf(src[i]);
}
int ew_cast_f32_bf16(const float* src, bf16_t* dst, size_t n, hipStream_t st) {
  FEDFR_REQUIRE(src && dst && n > 0, "cast_f32_bf16: bad args");
  FEDFR_REQUIRE(((uintptr_t)src & 15) == 0 && ((uintptr_t)dst & 15) == 0, "cast_f32_bf16: 16-byte alignment");
  const size_t work = n / 8 + 1;
  const int grid = (int)((work + 255) / 256 > 4096 ? 4096 : (work + 255) / 256);
  hipLaunchKernelGGL(cast_f32_bf16_kernel, dim3(grid), dim3(256), 0, st, src, dst, n);
  FEDFR_LAUNCH_CHECK("cast_f32_bf16");
  return FEDFR_OK;
}

// [Cout][RS][Cin] fp32 -> [Cin][RS(flipped)][Cout] bf16, 64x64 LDS-tiled transpose
__global__ __launch_bounds__(256) void weight_dgrad_shadow_kernel(const float* __restrict__ w, bf16_t* __restrict__ dst,
                                                                  int Cout, int RS, int Cin) {
  __shared__ float tile[64][65];
  const int co0 = blockIdx.x * 64, ci0 = blockIdx.y * 64, tap = blockIdx.z;
  const int t = threadIdx.x;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = (t >> 4) + 16 * i, col = (t & 15) * 4;
    const float4 v = *reinterpret_cast<const float4*>(w + ((size_t)(co0 + row) * RS + tap) * Cin + ci0 + col);
    tile[row][col] = v.x; tile[row][col + 1] = v.y; tile[row][col + 2] = v.z; tile[row][col + 3] = v.w;
  }
  __syncthreads();
  const int tapf = RS - 1 - tap;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int ci = (t >> 3) + 32 * i, co8 = (t & 7) * 8;
    float f[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = tile[co8 + j][ci];
    *reinterpret_cast<uint4*>(dst + ((size_t)(ci0 + ci) * RS + tapf) * Cout + co0 + co8) = pack8(f);
  }
}
// the same transpose for every conv of a network: workgroup -> (layer, co tile, ci tile, tap) through the by-value table
__global__ __launch_bounds__(256) void weight_dgrad_shadow_multi_kernel(const float* __restrict__ params, bf16_t* __restrict__ shadow, ShadowTable tb) {
  __shared__ float tile[64][65];
  int lo = 0, hi = tb.n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tb.e[mid].first_blk <= blockIdx.x) lo = mid; else hi = mid - 1;
  }
  const ShadowEntry e = tb.e[lo];
  int b = (int)(blockIdx.x - e.first_blk);
  const int cob = b % e.cout64; b /= e.cout64;
  const int cib = b % e.cin64;
  const int tap = b / e.cin64;
  const int Cout = e.cout64 * 64, Cin = e.cin64 * 64, RS = e.rs;
  const float* w = params + e.src;
  bf16_t* dst = shadow + e.dst;
  const int co0 = cob * 64, ci0 = cib * 64, t = threadIdx.x;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = (t >> 4) + 16 * i, col = (t & 15) * 4;
    const float4 v = *reinterpret_cast<const float4*>(w + ((size_t)(co0 + row) * RS + tap) * Cin + ci0 + col);
    tile[row][col] = v.x; tile[row][col + 1] = v.y; tile[row][col + 2] = v.z; tile[row][col + 3] = v.w;
  }
  __syncthreads();
  const int tapf = RS - 1 - tap;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int ci = (t >> 3) + 32 * i, co8 = (t & 7) * 8;
    float f[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = tile[co8 + j][ci];
    *reinterpret_cast<uint4*>(dst + ((size_t)(ci0 + ci) * RS + tapf) * Cout + co0 + co8) = pack8(f);
  }
}
int ew_weight_dgrad_shadow_multi(const float* params, bf16_t* shadow, ShadowTable& t, hipStream_t st) {
  FEDFR_REQUIRE(params && shadow && t.n > 0 && t.n <= kMaxShadowEntries, "weight_dgrad_shadow_multi: bad table");
  unsigned blk = 0;
  for (int i = 0; i < t.n; ++i) {
    t.e[i].first_blk = blk;
    blk += (unsigned)t.e[i].cout64 * t.e[i].cin64 * t.e[i].rs;
  }
  hipLaunchKernelGGL(weight_dgrad_shadow_multi_kernel, dim3(blk), dim3(256), 0, st, params, shadow, t);
  FEDFR_LAUNCH_CHECK("weight_dgrad_shadow_multi");
  return FEDFR_OK;
}

int ew_weight_dgrad_shadow(const float* w, bf16_t* dst, int Cout, int R, int S, int Cin, hipStream_t st) {
  FEDFR_REQUIRE(w && dst && (Cout & 63) == 0 && (Cin & 63) == 0 && R > 0 && S > 0, "weight_dgrad_shadow: need Cout,Cin %%64==0");
  hipLaunchKernelGGL(weight_dgrad_shadow_kernel, dim3(Cout / 64, Cin / 64, R * S), dim3(256), 0, st, w, dst, Cout, R * S, Cin);
  FEDFR_LAUNCH_CHECK("weight_dgrad_shadow");
  return FEDFR_OK;
}

// [B][C][HW] fp32 -> [B][HW][C] bf16 through a 64 x 64 LDS tile: coalesced on both sides (round 4: the one-element-per-thread gather read with a
// stride of HW floats took 26 us for the 6.4 MB gradient of the flattened 7x7 map at the top of every backward pass)
__global__ __launch_bounds__(256) void nchw_f32_to_nhwc_bf16_kernel(const float* __restrict__ src, bf16_t* __restrict__ dst, int C, int HW) {
  __shared__ float tile[64][65];
  const int t = threadIdx.x, b = blockIdx.z, c0 = blockIdx.y * 64, p0 = blockIdx.x * 64;
  const float* s = src + (size_t)b * C * HW;
#pragma unroll 4
  for (int r = t >> 6; r < 64; r += 4) {
    const int c = c0 + r, p = p0 + (t & 63);
    tile[r][t & 63] = (c < C && p < HW) ? s[(size_t)c * HW + p] : 0.f;
  }
  __syncthreads();
  bf16_t* d = dst + (size_t)b * HW * C;
#pragma unroll 4
  for (int pp = t >> 5; pp < 64; pp += 8) {
    const int p = p0 + pp, c = c0 + (t & 31) * 2;
    if (p < HW && c + 1 < C) *reinterpret_cast<unsigned*>(d + (size_t)p * C + c) = pack_bf2(tile[(t & 31) * 2][pp], tile[(t & 31) * 2 + 1][pp]);      // (C is even: launcher)
  }
}
int ew_nchw_f32_to_nhwc_bf16(const float* src, bf16_t* dst, int B, int C, int HW, hipStream_t st) {
  FEDFR_REQUIRE(src && dst && B > 0 && C > 0 && HW > 0 && (C & 1) == 0 && B <= 65535 && (C + 63) / 64 <= 65535, "nchw_f32_to_nhwc_bf16: bad args (C even)");
  hipLaunchKernelGGL(nchw_f32_to_nhwc_bf16_kernel, dim3((HW + 63) / 64, (C + 63) / 64, B), dim3(256), 0, st, src, dst, C, HW);
  FEDFR_LAUNCH_CHECK("nchw_f32_to_nhwc_bf16");
  return FEDFR_OK;
}


// =====================================================================================================
// input pipeline on the device (reference dataset.py:81-92: ToPILImage -> RandomHorizontalFlip -> ToTensor ->
// Normalize(0.5, 0.5)): uint8 HWC images (as decoded) + one flip flag per image -> fp32 NCHW in [-1, 1], the backbone's input.
// Same fp32 operations in the same order as torchvision (x / 255, then (t - 0.5) / 0.5): bit-exact.  The host uploads 1 byte
// per pixel-channel instead of 4.
// =====================================================================================================
__global__ __launch_bounds__(256) void preprocess_u8_kernel(const unsigned char* __restrict__ src, const unsigned char* __restrict__ flip,
                                                           float* __restrict__ dst, int B, int H, int W) {
  const long long total = (long long)B * H * W;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int w = (int)(i % W);
    const long long t = i / W;
    const int h = (int)(t % H), b = (int)(t / H);
    const int ws = (flip && flip[b]) ? W - 1 - w : w;
    const unsigned char* sp = src + (((long long)b * H + h) * W + ws) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float v = __fdiv_rn((float)sp[c], 255.f);
      dst[(((long long)b * 3 + c) * H + h) * W + w] = __fdiv_rn(__fsub_rn(v, 0.5f), 0.5f);
    }
  }
}
int ew_preprocess_u8(const unsigned char* src, const unsigned char* flip, float* dst, int B, int H, int W, hipStream_t st) {
  FEDFR_REQUIRE(src && dst && B > 0 && H > 0 && W > 0, "preprocess_u8: bad args");
  const long long total = (long long)B * H * W;
  const int grid = (int)std::min<long long>((total + 255) / 256, 8192);
  hipLaunchKernelGGL(preprocess_u8_kernel, dim3(grid), dim3(256), 0, st, src, flip, dst, B, H, W);
  FEDFR_LAUNCH_CHECK("preprocess_u8");
  return FEDFR_OK;
}

// fp32 NCHW [B][C][HW] -> bf16 NHWC [B][HW][Cpad], channels >= C zero (sphnet's 3-channel input feeds the 64-channel-granular conv)
__global__ __launch_bounds__(256) void pad_input_nhwc_kernel(const float* __restrict__ src, bf16_t* __restrict__ dst, int B, int C, int HW, int Cpad) {
  const long long total = (long long)B * HW * (Cpad / 8);
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int ch = (int)(i % (Cpad / 8));
    const long long px = i / (Cpad / 8);
    const int hw = (int)(px % HW), b = (int)(px / HW);
    float f[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = ch * 8 + j;
      f[j] = c < C ? src[((long long)b * C + c) * HW + hw] : 0.f;
    }
    *reinterpret_cast<uint4*>(dst + px * Cpad + ch * 8) = pack8(f);
  }
}
int ew_pad_input_nhwc(const float* src, bf16_t* dst, int B, int C, int HW, int Cpad, hipStream_t st) {
  FEDFR_REQUIRE(src && dst && B > 0 && C > 0 && HW > 0 && Cpad >= C && (Cpad & 7) == 0, "pad_input_nhwc: bad args");
  const long long total = (long long)B * HW * (Cpad / 8);
  hipLaunchKernelGGL(pad_input_nhwc_kernel, dim3((int)std::min<long long>((total + 255) / 256, 16384)), dim3(256), 0, st, src, dst, B, C, HW, Cpad);
  FEDFR_LAUNCH_CHECK("pad_input_nhwc");
  return FEDFR_OK;
}


// =====================================================================================================
// Dropout on the flattened bn2 output (reference backbones/iresnet.py:96,169: nn.Dropout(p, inplace=True) between bn2 and fc)
// =====================================================================================================
// Counter-based mask: element i of training step `step` is kept iff a 16-bit hash of (seed, step, i) >= p * 65536, so the mask is a pure
// function of (seed, step, index) — reproducible, no RNG state on the device.  Kept values are scaled by 1 / (1 - p) (torch semantics).
__device__ __forceinline__ unsigned long long dropout_hash(unsigned long long x) {   // splitmix64 finaliser
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
__global__ __launch_bounds__(256) void dropout_fwd_kernel(bf16_t* __restrict__ t, unsigned char* __restrict__ mask, size_t n8, unsigned thr,
                                                          float inv_keep, unsigned long long seed, unsigned long long step) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += stride) {
    const unsigned long long key = seed * 0x100000001B3ull + step * 0x9E3779B1ull;
    const unsigned long long h0 = dropout_hash(key ^ (2 * i)), h1 = dropout_hash(key ^ (2 * i + 1));
    uint4 v = reinterpret_cast<uint4*>(t)[i];
    float f[8];
    unpack8(v, f);
    unsigned char m[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const unsigned r = (unsigned)(((j < 4 ? h0 : h1) >> (16 * (j & 3))) & 0xffffu);
      m[j] = r >= thr ? 1 : 0;
      f[j] = m[j] ? f[j] * inv_keep : 0.f;
    }
    reinterpret_cast<uint4*>(t)[i] = pack8(f);
    uint2 mk;
    mk.x = (unsigned)m[0] | ((unsigned)m[1] << 8) | ((unsigned)m[2] << 16) | ((unsigned)m[3] << 24);
    mk.y = (unsigned)m[4] | ((unsigned)m[5] << 8) | ((unsigned)m[6] << 16) | ((unsigned)m[7] << 24);
    reinterpret_cast<uint2*>(mask)[i] = mk;
  }
}
__global__ __launch_bounds__(256) void dropout_bwd_kernel(float* __restrict__ dx, const unsigned char* __restrict__ mask, size_t n4, float inv_keep) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    const unsigned mk = reinterpret_cast<const unsigned*>(mask)[i];
    float4 d = reinterpret_cast<float4*>(dx)[i];
    d.x = (mk & 0xffu) ? d.x * inv_keep : 0.f;
    d.y = (mk & 0xff00u) ? d.y * inv_keep : 0.f;
    d.z = (mk & 0xff0000u) ? d.z * inv_keep : 0.f;
    d.w = (mk & 0xff000000u) ? d.w * inv_keep : 0.f;
    reinterpret_cast<float4*>(dx)[i] = d;
  }
}
int ew_dropout_fwd(bf16_t* t, unsigned char* mask, size_t n, float p, unsigned long long seed, unsigned long long step, hipStream_t st) {
  FEDFR_REQUIRE(t && mask && n > 0 && (n & 7) == 0 && p > 0.f && p < 1.f, "dropout_fwd: bad args (n%%8, 0 < p < 1)");
  const size_t n8 = n / 8;
  const int grid = (int)std::min<size_t>((n8 + 255) / 256, 4096);
  hipLaunchKernelGGL(dropout_fwd_kernel, dim3(grid), dim3(256), 0, st, t, mask, n8, (unsigned)(p * 65536.f), 1.f / (1.f - p), seed, step);
  FEDFR_LAUNCH_CHECK("dropout_fwd");
  return FEDFR_OK;
}
int ew_dropout_bwd(float* dx, const unsigned char* mask, size_t n, float p, hipStream_t st) {
  FEDFR_REQUIRE(dx && mask && n > 0 && (n & 3) == 0 && p > 0.f && p < 1.f, "dropout_bwd: bad args (n%%4, 0 < p < 1)");
  const size_t n4 = n / 4;
  const int grid = (int)std::min<size_t>((n4 + 255) / 256, 4096);
  hipLaunchKernelGGL(dropout_bwd_kernel, dim3(grid), dim3(256), 0, st, dx, mask, n4, 1.f / (1.f - p));
  FEDFR_LAUNCH_CHECK("dropout_bwd");
  return FEDFR_OK;
}
