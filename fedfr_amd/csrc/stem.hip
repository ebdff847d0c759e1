// The stem: conv 3 -> 64 (3x3, stride 1, pad 1) on the fp32 NCHW input as MFMA kernels — forward with the statistics of its output, and the weight
// gradient (optionally with the stem's BatchNorm + PReLU backward applied to the incoming tile, bn_math.h) with its reduction over workgroups.
#include "ew.h"
#include "ew_rowslab.h"  // load8f
#include "bn_math.h"
#include "gemm_tn_dev.h"
#include "gemm_dev.h"    // row16_sum

// =====================================================================================================
// stem conv 3 -> 64, 3x3 s1 p1, fp32 NCHW input, one 16x16x32 MFMA per 16 pixels x 16 channels (K = 27 -> 32)
// =====================================================================================================
#if FEDFR_FP16
#define MFMA16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_f16((a), (b), (c), 0, 0, 0)
#else
#define MFMA16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_bf16((a), (b), (c), 0, 0, 0)
#endif

__global__ __launch_bounds__(256) void stem_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                       bf16_t* __restrict__ y, float* __restrict__ stats, int B, int H,
                                                       int W, int ntiles) {
  __shared__ __attribute__((aligned(16))) unsigned char sC[256 * 144];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, lg = lane >> 4;
  const int M = B * H * W;
  // weight fragments (A operand: row n = ni*16 + l15, k = 8*lg + j); KRSC index = n*27 + k
  bf16x8_t wf[4];
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) {
    s16x8_t v;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int k = 8 * lg + j;
      v[j] = (short)f2bf(k < 27 ? w[(ni * 16 + l15) * 27 + k] : 0.f);
    }
    wf[ni] = __builtin_bit_cast(bf16x8_t, v);
  }
  // this lane's eight im2col columns k = 8 lg + j: tap offsets and the element offset relative to (img, channel 0, h, w).  The gather is
  // branch-free (raw buffer loads, an out-of-image tap reads beyond the buffer = 0): predicated loads made hipcc wait for each one in turn,
  // and the kernel ran at 1.3 TB/s of the 224 MB it moves.  All 32 loads of a tile are in flight before the first conversion.
  int dr[8], ds[8], koff[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int k = 8 * lg + j;
    const int tap = k / 3, ci = k - tap * 3;
    const int r = tap / 3, s_ = tap - r * 3;
    dr[j] = k < 27 ? r - 1 : (1 << 20);                  // k >= 27: never inside the image
    ds[j] = s_ - 1;
    koff[j] = (ci * H + (r - 1)) * W + (s_ - 1);
  }
  const __amdgpu_buffer_rsrc_t rsX = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(x), 0, (int)((size_t)B * 3 * H * W * 4), 0x00020000);
  // a workgroup walks tiles of 256 pixels (the weight fragments above are set up once); the statistics rows keep the per-tile layout
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
  const int mblk = tile * 256 + wave * 64;
  f32x4_t acc[4][4];
  unsigned raw[4][8];
#pragma unroll
  for (int mi = 0; mi < 4; ++mi) {
    const int m = mblk + mi * 16 + l15;
    const bool okm = m < M;
    const int mm = okm ? m : 0;
    const int img = mm / (H * W), rem = mm - img * H * W;
    const int h = rem / W, wq = rem - h * W;
    const int base = (img * 3 * H + h) * W + wq;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const bool ok = okm & ((unsigned)(h + dr[j]) < (unsigned)H) & ((unsigned)(wq + ds[j]) < (unsigned)W);
      raw[mi][j] = __builtin_amdgcn_raw_buffer_load_b32(rsX, ok ? (base + koff[j]) * 4 : (int)0xfffffff0u, 0, 0);
    }
  }
#pragma unroll
  for (int mi = 0; mi < 4; ++mi) {
    s16x8_t v;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (short)f2bf(__uint_as_float(raw[mi][j]));
    const bf16x8_t xf = __builtin_bit_cast(bf16x8_t, v);
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
      const f32x4_t z4 = {0.f, 0.f, 0.f, 0.f};
      acc[ni][mi] = MFMA16(wf[ni], xf, z4);
    }
  }
  // D: n = ni*16 + lg*4 + reg ; m(local) = wave*64 + mi*16 + l15
  float ssum[4][4], ssq[4][4];
#pragma unroll
  for (int ni = 0; ni < 4; ++ni)
#pragma unroll
    for (int q = 0; q < 4; ++q) ssum[ni][q] = ssq[ni][q] = 0.f;
#pragma unroll
  for (int ni = 0; ni < 4; ++ni)
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
      bf16_t hh[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        hh[q] = f2bf(acc[ni][mi][q]);
        const float v = bf2f(hh[q]);
        ssum[ni][q] += v;
        ssq[ni][q] += v * v;
      }
      uint2 pk;
      pk.x = (unsigned)hh[0] | ((unsigned)hh[1] << 16);
      pk.y = (unsigned)hh[2] | ((unsigned)hh[3] << 16);
      *reinterpret_cast<uint2*>(sC + (wave * 64 + mi * 16 + l15) * 144 + (ni * 16 + lg * 4) * 2) = pk;
    }
  if (stats) {
    float* prow = stats + (size_t)(tile * 4 + wave) * 128;
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float a = row16_sum(ssum[ni][q]), b = row16_sum(ssq[ni][q]);      // DPP adds (the shuffle form was 128 ds_bpermute per tile)
        if (l15 == 0) {
          prow[ni * 16 + lg * 4 + q] = a;
          prow[64 + ni * 16 + lg * 4 + q] = b;
        }
      }
  }
  __syncthreads();
  for (int idx = tid; idx < 256 * 8; idx += 256) {
    const int row = idx >> 3, c = idx & 7;
    const int m = tile * 256 + row;
    if (m < M) *reinterpret_cast<uint4*>(y + (size_t)m * 64 + c * 8) = *reinterpret_cast<const uint4*>(sC + row * 144 + c * 16);
  }
  __syncthreads();                                     // the staged tile has been read: the next one may be written
  }
}

int ew_stem_stat_rows(int B, int H, int W) { return ceil_div((long long)B * H * W, 256) * 4; }

int ew_stem_fwd(const float* x, const float* w, bf16_t* y, float* stats, int B, int H, int W, hipStream_t st) {
  FEDFR_REQUIRE(x && w && y && B > 0 && H > 0 && W > 0, "stem_fwd: bad args");
  const int M = B * H * W;
  FEDFR_REQUIRE((size_t)B * 3 * H * W * 4 < (1ull << 31), "stem_fwd: input larger than 2 GiB (32-bit buffer offsets)");
  const int ntiles = ceil_div(M, 256);
  hipLaunchKernelGGL(stem_fwd_kernel, dim3(ntiles < 2048 ? ntiles : 2048), dim3(256), 0, st, x, w, y, stats, B, H, W, ntiles);
  FEDFR_LAUNCH_CHECK("stem_fwd");
  return FEDFR_OK;
}

__global__ __launch_bounds__(256) void stem_wgrad_reduce_kernel(const float* __restrict__ tmp, int nblk, float* __restrict__ dw) {
  __shared__ double red[8][32];
  const int co = blockIdx.x, k = threadIdx.x & 31, g = threadIdx.x >> 5;
  double s = 0.0;
  int b = g;
  for (; b + 24 < nblk; b += 32) {                  // four independent loads per trip: the walk over ~1000 blocks is a latency chain
    const float v0 = tmp[(size_t)b * 2048 + co * 32 + k], v1 = tmp[(size_t)(b + 8) * 2048 + co * 32 + k];
    const float v2 = tmp[(size_t)(b + 16) * 2048 + co * 32 + k], v3 = tmp[(size_t)(b + 24) * 2048 + co * 32 + k];
    s += ((double)v0 + (double)v1) + ((double)v2 + (double)v3);
  }
  for (; b < nblk; b += 8) s += (double)tmp[(size_t)b * 2048 + co * 32 + k];
  red[g][k] = s;
  __syncthreads();
  if (g == 0 && k < 27) {
    double t = 0.0;
#pragma unroll
    for (int i = 0; i < 8; ++i) t += red[i][k];
    dw[co * 27 + k] = (float)t;
  }
}

// ---- stem wgrad on MFMA --------------------------------------------------------------------------------------------------
// dw[co][k] = sum_px dy[px][co] * col[px][k] as a GEMM with the pixels as the reduction: A = dy^T (transpose reads of the [px][co] tile,
// gemm_tn_dev.h), B = col kept TRANSPOSED in LDS ([k][px], built by the threads from the fp32 NCHW input), split into a bf16 high and
// low part (x = hi + lo to 2^-17: two MFMAs per tile keep fp32-input accuracy).  A VALU form was compute-bound (244 us for 224 MB of
// traffic at B = 128); this one streams.
constexpr int SW_PX = 128;                    // pixels per stage (256 threads: SW_PX pixels x 256 / SW_PX slices of the 32 im2col columns)
constexpr int SW_CPITCH = 2 * SW_PX + 16;     // colT row pitch in bytes: +16 B keeps the 16 k-rows of a b128 fragment read on distinct banks
// FUSE (round 6): dy is the gradient wrt the stem's ACTIVATION and the BatchNorm + PReLU backward is applied to the tile on its way into LDS — bn_math.h's
// bn_bwd_dx, the call bn_bwd_apply_kernel<true, 0, false> makes, rounded to the same 16 bits as that kernel would have stored it: the 205 MB tensor
// d(conv output) that only this kernel ever read is neither written nor read back.
struct StemFuse {
  const bf16_t* x0;       // the stem conv's raw output [px][64]
  const float* coef;      // [3][64] from bn_bwd_finalize8_kernel
  const float *sc, *sh;   // the forward's (scale, shift): the PReLU mask is the forward's
  const float* alpha;
};
template <bool FUSE>
__global__ __launch_bounds__(256) void stem_wgrad_mfma_kernel(const float* __restrict__ x, const bf16_t* __restrict__ dy, StemFuse fz,
                                                              float* __restrict__ tmp, int B, int H, int W, int px_per_block) {
  __shared__ __attribute__((aligned(16))) unsigned char sdy[SW_PX * 128];          // [px][64 co] bf16, chunk-swizzled (tn_swz<128>)
  __shared__ __attribute__((aligned(16))) unsigned char scol[2][32 * SW_CPITCH];   // hi / lo: [k 0..31][px] bf16
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int M = B * H * W;
  const int mbeg = blockIdx.x * px_per_block, mend = min(M, mbeg + px_per_block);
  f32x4_t acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};                  // wave = co block of 16; two k blocks of 16
  const int foff = tn_frag_off<128>(wave * 16, lane);
  const int kg = lane >> 4, kn = lane & 15;
  // this thread's im2col columns k0 .. k0 + KSL - 1 of pixel pxl: tap offsets and element offsets relative to (img, channel 0, h, w).
  // Both operands are fetched with branch-free buffer loads (out of range = 0), all of a stage's loads issued before the first is used:
  // the predicated form made hipcc wait for every load in turn (stem_fwd_kernel has the same history).
  constexpr int KSL = 32 * SW_PX / 256;                 // im2col columns per thread
  const int pxl = tid % SW_PX, k0 = (tid / SW_PX) * KSL;
  int dr[KSL], ds[KSL], koff[KSL];
#pragma unroll
  for (int kk = 0; kk < KSL; ++kk) {
    const int k = k0 + kk;
    const int tap = k / 3, ci = k - tap * 3;
    const int r = tap / 3, sx = tap - r * 3;
    dr[kk] = k < 27 ? r - 1 : (1 << 20);
    ds[kk] = sx - 1;
    koff[kk] = (ci * H + (r - 1)) * W + (sx - 1);
  }
  const __amdgpu_buffer_rsrc_t rsX = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(x), 0, (int)((size_t)B * 3 * H * W * 4), 0x00020000);
  const __amdgpu_buffer_rsrc_t rsD = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16_t*>(dy) + (size_t)mbeg * 64, 0, (int)((size_t)(mend - mbeg) * 128), 0x00020000);
  const __amdgpu_buffer_rsrc_t rsX0 = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16_t*>(FUSE ? fz.x0 : dy) + (size_t)mbeg * 64, 0, (int)((size_t)(mend - mbeg) * 128), 0x00020000);
  float ca[8], cA[8], cB[8], G[8], Hs[8], al[8];      // FUSE: this thread's 16-byte chunk is the same eight channels in every stage (256 % 8 == 0)
  if (FUSE) {
    const int c0 = (tid & 7) * 8;
    load8f(fz.coef, c0, ca, 1.f);
    load8f(fz.coef + 64, c0, cA, 0.f);
    load8f(fz.coef + 128, c0, cB, 0.f);
    load8f(fz.sc, c0, G, 1.f);
    load8f(fz.sh, c0, Hs, 0.f);
    load8f(fz.alpha, c0, al, 1.f);
  }
  for (int mc = mbeg; mc < mend; mc += SW_PX) {
    uint4 dv[SW_PX / 32], xv[SW_PX / 32];
    unsigned raw[KSL];
    // dy tile: SW_PX px x 8 chunks of 16 B (rows at or beyond mend lie beyond this workgroup's descriptor: zeros)
#pragma unroll
    for (int i = 0; i < SW_PX / 32; ++i) {
      const int idx = tid + 256 * i;
      const int px = idx >> 3, c = idx & 7;
      const u32x4_t v = __builtin_amdgcn_raw_buffer_load_b128(rsD, (mc - mbeg + px) * 128 + c * 16, 0, 0);
      dv[i] = make_uint4(v[0], v[1], v[2], v[3]);
      if (FUSE) {
        const u32x4_t q = __builtin_amdgcn_raw_buffer_load_b128(rsX0, (mc - mbeg + px) * 128 + c * 16, 0, 0);
        xv[i] = make_uint4(q[0], q[1], q[2], q[3]);
      }
    }
    {   // im2col of this thread's pixel
      const int m = mc + pxl;
      const bool okm = m < mend;
      const int mm = okm ? m : 0;
      const int img = mm / (H * W), rem = mm - img * H * W;
      const int h = rem / W, wq = rem - h * W;
      const int base = (img * 3 * H + h) * W + wq;
#pragma unroll
      for (int kk = 0; kk < KSL; ++kk) {
        const bool ok = okm & ((unsigned)(h + dr[kk]) < (unsigned)H) & ((unsigned)(wq + ds[kk]) < (unsigned)W);
        raw[kk] = __builtin_amdgcn_raw_buffer_load_b32(rsX, ok ? (base + koff[kk]) * 4 : (int)0xfffffff0u, 0, 0);
      }
    }
#pragma unroll
    for (int i = 0; i < SW_PX / 32; ++i) {
      const int idx = tid + 256 * i;
      const int px = idx >> 3, c = idx & 7;
      if (FUSE) {
        float d[8], x0[8], o[8];
        unpack8(dv[i], d);
        unpack8(xv[i], x0);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          o[j] = bn_bwd_dx<true>(d[j], x0[j], G[j], Hs[j], al[j], ca[j], cA[j], cB[j]);
          // the fp32 result is kept as such and THEN rounded to 16 bits, as bn_bwd_apply does (v_pk_fma_f32 + v_cvt_pk_f16_f32): left alone, hipcc
          // folds the conversion of the fp16 build into v_fma_mixlo_f16, which rounds the exact sum once — another last bit in a few elements per
          // million, and the weight gradient no longer equals the two-kernel form's bit for bit (tests/test_stem_chain_gpu.py)
          asm("" : "+v"(o[j]));
        }
        dv[i] = mc + px < mend ? pack8(o) : make_uint4(0, 0, 0, 0);      // rows beyond this workgroup's range read as zeros, and B is not zero
      }
      *reinterpret_cast<uint4*>(sdy + px * 128 + ((c ^ tn_swz<128>(px)) << 4)) = dv[i];
    }
    // transposed: colT[k][px], k = (tap, ci), rows 27..31 zero
#pragma unroll
    for (int kk = 0; kk < KSL; ++kk) {
      const int k = k0 + kk;
      const float f = __uint_as_float(raw[kk]);
      const bf16_t hi = f2bf(f);
      const bf16_t lo = f2bf(f - bf2f(hi));
      *reinterpret_cast<bf16_t*>(scol[0] + k * SW_CPITCH + pxl * 2) = hi;
      *reinterpret_cast<bf16_t*>(scol[1] + k * SW_CPITCH + pxl * 2) = lo;
    }
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < SW_PX / 32; ++ks) {
      const bf16x8_t a = tn_frag_tr<128>(sdy + (ks >> 1) * 64 * 128, foff, ks & 1);      // dy^T fragment: 16 co x 32 px
#pragma unroll
      for (int kb = 0; kb < 2; ++kb) {
        const int boff = (kb * 16 + kn) * SW_CPITCH + (ks * 32 + kg * 8) * 2;            // colT[k][px .. px+7]
        const bf16x8_t bh = *reinterpret_cast<const bf16x8_t*>(scol[0] + boff);
        const bf16x8_t bl = *reinterpret_cast<const bf16x8_t*>(scol[1] + boff);
        acc[kb] = MFMA16(a, bh, acc[kb]);
        acc[kb] = MFMA16(a, bl, acc[kb]);
      }
    }
    __syncthreads();
  }
  // D[m = co][n = k]: lane holds co = wave 16 + (lane >> 4) 4 + r, k = kb 16 + (lane & 15)
  float* o = tmp + (size_t)blockIdx.x * 2048;
#pragma unroll
  for (int kb = 0; kb < 2; ++kb)
#pragma unroll
    for (int r = 0; r < 4; ++r) o[(wave * 16 + (lane >> 4) * 4 + r) * 32 + kb * 16 + (lane & 15)] = acc[kb][r];
}

static int stem_px_per_block(int M) {
  int ppb = ceil_div(M, 1024);
  ppb = (ppb + SW_PX - 1) / SW_PX * SW_PX;              // whole stages
  if (ppb < SW_PX) ppb = SW_PX;
  return ppb;
}
int ew_stem_wgrad_blocks(int B, int H, int W) {
  const int M = B * H * W;
  return ceil_div(M, stem_px_per_block(M));
}
int ew_stem_wgrad(const float* x, const bf16_t* dy, float* dw, float* tmp, int B, int H, int W, hipStream_t st, const bf16_t* x0, const float* coef,
                  const float* sc, const float* sh, const float* alpha) {
  FEDFR_REQUIRE(x && dy && dw && tmp && B > 0 && H > 0 && W > 0, "stem_wgrad: bad args");
  FEDFR_REQUIRE(!x0 || (coef && sc && sh && alpha), "stem_wgrad: the fused BatchNorm + PReLU backward needs coefficients, (scale, shift) and slopes");
  const int M = B * H * W;
  const int ppb = stem_px_per_block(M);
  const int nblk = ceil_div(M, ppb);
  const StemFuse fz{x0, coef, sc, sh, alpha};
  if (x0) hipLaunchKernelGGL(stem_wgrad_mfma_kernel<true>, dim3(nblk), dim3(256), 0, st, x, dy, fz, tmp, B, H, W, ppb);
  else hipLaunchKernelGGL(stem_wgrad_mfma_kernel<false>, dim3(nblk), dim3(256), 0, st, x, dy, fz, tmp, B, H, W, ppb);
  FEDFR_LAUNCH_CHECK("stem_wgrad");
  hipLaunchKernelGGL(stem_wgrad_reduce_kernel, dim3(64), dim3(256), 0, st, tmp, nblk, dw);
  FEDFR_LAUNCH_CHECK("stem_wgrad_reduce");
  return FEDFR_OK;
}
