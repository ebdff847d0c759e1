// conv3x3_glds_kernel + launcher template; one translation unit per instantiation (see gemm_dev.h).
#pragma once
#include <type_traits>
#include <algorithm>
#include "gemm_dev.h"
#include "epi_mfma.h"

// In-kernel phase stamps for tools/stamp (compiled out of the product)
#ifdef FEDFR_HALO2_STAMPS
#define GLDS_STAMP(i)                                                                       \
  do {                                                                                      \
    if (threadIdx.x == 0 && p.dbg) {                                                        \
      p.dbg[(size_t)blockIdx.x * 16 + 2 * (i)] = __builtin_readcyclecounter();             \
      p.dbg[(size_t)blockIdx.x * 16 + 2 * (i) + 1] = wall_clock64();                        \
    }                                                                                       \
  } while (0)
#else
#define GLDS_STAMP(i) do { } while (0)
#endif
#ifndef GLDS_ABLATE
#define GLDS_ABLATE 0      // timing ablations (WRONG results): 1 no in-loop LDS-DMA, 2 no per-tap barrier, 4 no fragment reads, 8 no prologue DMA / wait for the second tile of a workgroup, 16 no in-loop vmcnt waits (DMA still issued; padded-raster loop)
#endif
#ifdef GLDS_SETPRIO
#define GLDS_PRIO(x) __builtin_amdgcn_s_setprio(x)
#else
#define GLDS_PRIO(x) do { } while (0)
#endif

// =====================================================================================================
// 3x3 / stride-1 / pad-1 convolution (fwd, and dgrad with the flipped shadow) for 14x14 / 28x28 maps, Cout % 128 == 0,
// C % 128 == 0, as an implicit GEMM whose operands reach LDS by LDS-DMA (`buffer_load_dwordx4 ... lds`).
//
//   * Why: in-kernel stamps (tools/stamp) of the register-staged halo2 kernel showed its K loop at 32 % of the MFMA rate —
//     hipcc sinks the next tap's global loads to just before their ds_write, so every tap paid an L2 round trip.  LDS-DMA has
//     no register destination to sink towards: weight tiles 2-3 taps ahead and the next channel chunk's image are in flight
//     while a tap computes, retired by COUNTED s_waitcnt vmcnt(N) + one raw s_barrier per tap (never vmcnt(0) in the loop).
//   * Tile = 196 output pixels x 128 output channels: a whole 14x14 image, or 7 rows of a 28x28 image.  At the benchmark
//     batch (128) every 14x14 layer is exactly 256 tiles = one per CU (the 128-pixel tiling gave 392 = 1.53 rounds), a tile
//     never straddles images, and prologue / epilogue are paid once per 56 (not 32) MFMAs per tap and wave.
//   * A operand: the tile's pixels plus halo as a ZERO-PADDED image in LDS, one 128-B row (64 channels) per padded pixel, so a
//     filter tap is a constant row shift.  Out-of-image rows are fetched with an out-of-range buffer offset, which the hardware
//     turns into zeros in LDS (tools/probe/glds_probe.hip): no zero-fill pass, no masks.  Two image buffers (chunk cc / cc+1).
//   * B operand: one 128 (out channels) x 64 (k) slice of the KRSC weights per tap, ring of 4 buffers.
//   * LDS rows are 128 B with the 16-B chunk index XOR-ed by (row & 7): conflict-free ds_read_b128 for both operands.  An
//     LDS-DMA wave-instruction writes 1 KiB linearly (lane l -> base + 16 l), so the swizzle is applied to the per-lane SOURCE
//     address: lane l of a piece covering rows 8p..8p+7 fetches row 8p + (l >> 3), logical chunk (l & 7) ^ (l >> 3).
//   * 4 waves (2 x 2), wave tile 112 (7 fragments; 196 = 12.25 fragments, the tail is masked) x 64, v_mfma_f32_16x16x32_bf16.
//     The barrier sits in the MIDDLE of a tap, the first fragments of the next tap are read behind it, and fragment reads /
//     DMA issue are threaded between the MFMAs with sched_group_barrier.
//   * Epilogue: bf16 tile through LDS, per-column sum / sum-of-squares partials for the following BatchNorm in the layout of
//     the 128-row kernels (gemm_nt_stat_rows rows; the rows this tiling does not need are written as zeros).
// =====================================================================================================
// What an instantiation's epilogue does besides writing the tile:
//   plain   forward / dgrad: BatchNorm statistics of the output (p.stats), the eval-mode affine, the residual add, the second output
//   bnbwd   the BatchNorm-backward reduction of the layer in front (dgrad; p.bmom == 1: the forward raw moments), on the matrix cores
//   papply  sphnet's PReLU-apply (p.bmom == 2): the OUTPUT becomes dz — a per-element pass no matrix-core formulation covers
enum class Epi { plain, bnbwd, papply };

// Every compile-time fact of an instantiation: tile geometry, LDS layout, which paths it carries.  The kernel and the launcher both read it.
template <int W_, int R_, int NPA_, int WN_, Epi EPI_, int BN_, bool ONECHUNK_, int TPW_>
struct GldsGeom {
  static constexpr Epi EPI = EPI_;
  static constexpr bool ONECHUNK = ONECHUNK_, FUSED = EPI_ != Epi::plain;
  static constexpr int W = W_, R = R_, NPA = NPA_, WN = WN_, BN = BN_, TPW = TPW_;
  static constexpr int PT = R_ * W_, WM = 2, PW = W_ + 2, NW = WM * WN, NT = 64 * NW;
  static constexpr int PWL = (PW + 7) & ~7;                // LDS image pitch in rows: a multiple of 8, so that the swizzle key (row & 7) does not depend on
                                                           // the vertical tap offset -> A addresses need 3 (horizontal) variants, dy is an instruction immediate
  static constexpr int TM = 7, TN = BN / WN / 16, MW = TM * 16;   // 112 fragment rows per wave, 224 per tile (196 valid)
  static constexpr int AP = NPA / NW, BP = (BN / 8) / NW;  // LDS-DMA pieces per wave: image buffer / weight tile
  static constexpr int NABUF = ONECHUNK ? 1 : 2, NB = 4;   // image buffers; slots of the weight ring
  static constexpr int NRD = TM + TN, MPR = (TM * TN) / NRD;      // tap-major loop: fragment reads per k-half; MFMAs threaded per read
  static constexpr int TPI = W_ / R_;                      // tiles per image
  static constexpr int A_BYTES = NPA * 1024, B_BYTES = BN * 128;
  // RST: the GEMM's M index is the position q = y * PWL + x in the padded raster of the LDS image (the PWL - W_ filler columns of a
  // row are computed and thrown away: 224 positions either way), so the fragment of 16-position block rb for vertical tap dy IS the
  // fragment of block rb + dy * PWL / 16 for dy = 0: taps run dx-major and every A fragment is read from LDS once per horizontal tap
  // (9-11 row-block reads per k-step and dx instead of 21): 90 instead of 162 fragment reads per channel chunk and wave.
  static constexpr bool RST = (W_ == 14 || W_ == 28) && R_ * PWL == 2 * MW;
  static constexpr int VG = PWL / 16, NRB = TM + 2 * VG;
  // MST: column sums of the staged tile on the matrix cores (glds_epilogue_plain, glds_epilogue_bnbwd); the 224-pixel tiles sum in registers
  static constexpr bool MST = PT == 196 && BN == 16 * NW;
  // XLATE (fused, several tiles per workgroup): the two-tiles instantiation sits at the register limit, so the BatchNorm input tile cannot ride
  // through the K loop in registers.  It is requested right BEHIND the loop (after the drain of the tail DMAs: the loads fly while the
  // accumulators are staged) and the tiles' column sums meet in LDS: ONE partial row per workgroup.
  static constexpr bool XLATE = FUSED && TPW > 1;
  // this thread's share of the BatchNorm input tile x[PT][BN]: chunk column tid % CPR (8 channels) of rows tid / CPR, + RG, ...
  static constexpr int CPR = BN / 8, RG = NT / CPR, XN = FUSED ? (PT + RG - 1) / RG : 1, XPRE = (FUSED && !XLATE) ? XN : 0;
  // LDS: [NABUF][A_BYTES] images | [NB][B_BYTES] weight ring | TPW > 1: the workgroup's running partial row [<= 4][BN] floats.  Behind the K loop
  // the staged output tile (row pitch CST) lies over the images, the BatchNorm input tile (bnbwd) at SXOFF behind it, papply's scratch on the ring.
  static constexpr int XOFF = NABUF * A_BYTES, STAT_OFF = XOFF + NB * B_BYTES, CST = BN * 2 + 16, SXOFF = (PT * CST + 1023) & ~1023;
  static constexpr size_t LDS = (size_t)STAT_OFF + (TPW > 1 ? 4 * (size_t)BN * 4 : 0);
  // padded-raster kernels: the filler columns' lanes write to a dump row behind the tile (glds_stage_tile)
  static constexpr bool DUMP = RST && (PT + 1) * CST <= SXOFF;
  static constexpr int SLOT = W_ == 14 ? 12 : (W_ == 28 ? 13 : 15);   // profile slot; 15: 56x56 and 112x112
  static_assert(PT <= 2 * MW && PT > MW && W_ % R_ == 0 && (R_ + 2) * PWL <= NPA * 8 && NPA % NW == 0 && (BN / 8) % NW == 0 && MPR >= 1 &&
                    !(FUSED && ONECHUNK), "tile geometry");
  static_assert(!RST || ONECHUNK || AP <= 6, "padded-raster loop: the next chunk's image goes out one piece per tap over the first taps of a chunk");
  static_assert(XPRE == 0 || RST, "the fused instantiations run the padded-raster loop");
  static_assert(!FUSED || MST, "the fused epilogues are written for the 196-pixel tiles");
  static_assert(MST || TPW == 1, "several tiles per workgroup: the statistics come from the matrix cores");
  static_assert(EPI != Epi::bnbwd || 2 * SXOFF <= STAT_OFF, "staged tile + BatchNorm input tile must fit below the statistics row");
  static_assert(EPI != Epi::papply || (size_t)RG * 2 * BN * 4 <= (size_t)NB * B_BYTES, "reduction scratch must fit the weight ring");
  static_assert(LDS >= (size_t)PT * CST && LDS <= 160 * 1024, "LDS budget");
};

// What a thread knows about itself for the whole launch: its place in the workgroup, the LDS-DMA source plan, the fragment addresses.
template <class G>
struct GldsLane {
  int tid, lane, wave, wm, wn, l15, lg, n0;
  __amdgpu_buffer_rsrc_t rsA, rsB;
  unsigned a_src[G::AP];                                // image: byte offset of this lane's pixel/chunk at channel chunk 0 (per tile)
  unsigned b_src, b_rstep;                              // weights: this lane's row/chunk of piece 0; + j * b_rstep
  int a_adr[3][G::TM];                                  // tap-major loop: A-fragment byte offsets for the three horizontal taps
  int a_base[3];                                        // RST: row-block 0 of this wave for the three horizontal taps; block rb adds rb * 2048
  int b_addr[G::TN];
  bool m_ok[G::TM];
  int m_pix[G::TM];                                     // pixel inside the tile (row of the staged output tile)
};
struct GldsTile { int bt, img, y0, m0; };               // image tile bt: rows y0 .. of image img, output rows m0 ..
// registers the fused epilogues carry from the K loop to their reduction
template <class G>
struct GldsFused {
  uint4 xr[G::XN];                                      // this thread's share of the BatchNorm input tile
  float4 fc[2][2];                                      // papply: (bias, slope) of channels n0 + c * 8 + 4 h .. + 3
  float cf[5];                                          // bnbwd: (mean, rstd, gamma, beta, alpha) of channel n0 + 16 wave + (lane & 15)
};

typedef __attribute__((address_space(3))) void* lds_ptr_t;
constexpr unsigned GLDS_OOB = 0xfffffff0u;              // beyond any buffer: the load writes zeros to LDS (returns zeros to a register)

__device__ __forceinline__ unsigned char* glds_smem() {
  extern __shared__ __attribute__((aligned(1024))) unsigned char smem[];
  return smem;
}
template <int N_>
__device__ __forceinline__ void glds_wait_vmcnt() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N_) : "memory");
}
__device__ __forceinline__ void glds_store_out(bf16_t* dst, const uint4& v) { st16_out(dst, v); }

// A zero the compiler cannot see through.  The epilogues' index arithmetic is invariant over the tile loop: left alone it is hoisted in front of
// the K loop and lives through it (the two-tiles instantiations sit at the register limit: 256 VGPRs + spills instead of 194).  Added to this
// zero it is recomputed per tile.  ON = false: a plain 0.
template <bool ON>
__device__ __forceinline__ int opaque_zero() {
  int z = 0;
  if constexpr (ON) asm volatile("v_mov_b32 %0, 0" : "=v"(z));
  return z;
}
__device__ __forceinline__ float diag_pick(const f32x4_t& g, int qd) { return qd == 0 ? g[0] : qd == 1 ? g[1] : qd == 2 ? g[2] : g[3]; }
// the workgroup's running partial row in LDS (own column: no race, fixed summation order)
__device__ __forceinline__ void running_row_add(float* d, int ti, float t) { *d = ti == 0 ? t : *d + t; }

// ---- geometry of this thread: ids, weight source, fragment addresses
template <class G>
__device__ __forceinline__ void glds_lane_init(GldsLane<G>& L, const GemmNT& p, int bn) {
  L.tid = threadIdx.x; L.lane = L.tid & 63;
  L.wave = __builtin_amdgcn_readfirstlane(L.tid >> 6);
  L.wm = L.wave / G::WN; L.wn = L.wave % G::WN;
  L.l15 = L.lane & 15; L.lg = L.lane >> 4;
  L.n0 = bn * G::BN;
  L.rsA = make_rsrc(p.A, p.a_bytes); L.rsB = make_rsrc(p.B, p.b_bytes);
  const int prow = L.lane >> 3, pch = (L.lane & 7) ^ prow;
  L.b_src = ((unsigned)(L.n0 + L.wave * G::BP * 8 + prow) * (unsigned)p.K + (unsigned)(pch * 8)) * 2u;
  L.b_rstep = 8u * (unsigned)p.K * 2u;
#pragma unroll
  for (int mi = 0; mi < G::TM; ++mi) {
    if constexpr (G::RST) {
      const int q = L.wm * G::MW + mi * 16 + L.l15;
      const int y = q / G::PWL, x = q - y * G::PWL;
      L.m_ok[mi] = x < G::W;
      L.m_pix[mi] = L.m_ok[mi] ? y * G::W + x : 0;
    } else {
      const int t = L.wm * G::MW + mi * 16 + L.l15;       // pixel inside the tile
      L.m_ok[mi] = t < G::PT;
      L.m_pix[mi] = t;
      const int tt = L.m_ok[mi] ? t : 0;
      const int y = tt / G::W, x = tt - y * G::W;
#pragma unroll
      for (int dx = 0; dx < 3; ++dx) {
        const int r = y * G::PWL + x + dx;
        L.a_adr[dx][mi] = r * 128 + ((L.lg ^ (r & 7)) << 4);  // k-step 1 flips chunk bit 2: XOR 64
      }
    }
  }
#pragma unroll
  for (int dx = 0; dx < 3; ++dx) {
    const int r = L.wm * G::MW + L.l15 + dx;
    L.a_base[dx] = r * 128 + ((L.lg ^ (r & 7)) << 4);
  }
#pragma unroll
  for (int ni = 0; ni < G::TN; ++ni) {
    const int row = L.wn * (G::BN / G::WN) + ni * 16 + L.l15;
    L.b_addr[ni] = row * 128 + ((L.lg ^ (row & 7)) << 4);      // ks = 1 flips chunk bit 2: XOR 64
  }
}

// ---- LDS-DMA source plan and issue.  Lane l of every piece: row (l >> 3) of the piece, logical 16-B chunk (l & 7) ^ (l >> 3).
// LDS image row r <-> padded pixel (y0 + r / PWL, r % PWL) of image img; padded row 0 / H+1, column 0 / W+1 and the pitch
// filler columns are zero.
template <class G>
__device__ __forceinline__ GldsTile glds_plan_tile(GldsLane<G>& L, const GemmNT& p, int bt) {
  GldsTile T;
  T.bt = bt; T.img = bt / G::TPI; T.y0 = (bt - T.img * G::TPI) * G::R; T.m0 = bt * G::PT;
  const int prow = L.lane >> 3, pch = (L.lane & 7) ^ prow;
#pragma unroll
  for (int j = 0; j < G::AP; ++j) {
    const int r = (j * G::NW + L.wave) * 8 + prow;
    const int ry = r / G::PWL, rx = r - ry * G::PWL;
    const int yy = T.y0 + ry;
    const bool ok = ry < G::R + 2 && yy >= 1 && yy <= G::W && rx >= 1 && rx <= G::W;
    const unsigned pix = (unsigned)(T.img * (G::W * G::W) + (yy - 1) * G::W + (rx - 1));
    L.a_src[j] = ok ? (pix * (unsigned)p.C + (unsigned)(pch * 8)) * 2u : GLDS_OOB;
  }
  return T;
}
// one LDS-DMA piece: 64 lanes x 16 B from buffer offset vo (per lane) to 1 KiB of LDS at `lds`
__device__ __forceinline__ void glds_dma16(__amdgpu_buffer_rsrc_t rs, unsigned char* lds, unsigned vo) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_ptr_t)lds, 16, (int)vo, 0, 0, 0);
}
template <class G>
__device__ __forceinline__ void glds_issue_a1(const GldsLane<G>& L, int j, int cc, int abuf, bool live) {   // image piece j of this wave, channel chunk cc
  const unsigned vo = (live && L.a_src[j] != GLDS_OOB) ? L.a_src[j] + (unsigned)cc * 128u : GLDS_OOB;
  glds_dma16(L.rsA, glds_smem() + abuf * G::A_BYTES + (j * G::NW + L.wave) * 1024, vo);
}
template <class G>
__device__ __forceinline__ void glds_issue_a(const GldsLane<G>& L, int cc, int abuf, bool live) {
#pragma unroll
  for (int j = 0; j < G::AP; ++j) glds_issue_a1<G>(L, j, cc, abuf, live);
}
template <class G>
__device__ __forceinline__ void glds_issue_b(const GldsLane<G>& L, const GemmNT& p, int tap, int cc, int bbuf, bool live) {
  const unsigned koff = (unsigned)(tap * p.C + cc * 64) * 2u;
#pragma unroll
  for (int j = 0; j < G::BP; ++j) {
    const unsigned vo = live ? L.b_src + (unsigned)j * L.b_rstep + koff : GLDS_OOB;
    glds_dma16(L.rsB, glds_smem() + G::XOFF + bbuf * G::B_BYTES + (L.wave * G::BP + j) * 1024, vo);
  }
}
// prologue: image of chunk 0, weight tiles of the first three taps; wait for the image and the first tap
template <class G>
__device__ __forceinline__ void glds_prologue(const GldsLane<G>& L, const GemmNT& p, bool skip) {
  if (!skip) {
    glds_issue_a<G>(L, 0, 0, true);
    glds_issue_b<G>(L, p, 0, 0, 0, true);
    glds_issue_b<G>(L, p, G::RST ? 3 : 1, 0, 1, true);        // RST walks the taps dx-major: (dy, dx) = (0,0), (1,0), (2,0), (0,1), ...
    glds_issue_b<G>(L, p, G::RST ? 6 : 2, 0, 2, true);
    glds_wait_vmcnt<2 * G::BP>();
  }
  __builtin_amdgcn_s_barrier();
}
// This thread's share of the BatchNorm input tile, into registers (fused instantiations).  It rides through the K loop (28 VGPRs at 8 waves; one
// workgroup per CU, so 256 are there): fetched by LDS-DMA after the loop it paid the round trip plus a barrier in the open, 13 us on a 28 us kernel.
// Where the loads go: in front of the prologue's DMA they delayed the first barrier by 1.1 us per launch, right behind it still by 0.8 us (the eight
// waves' requests share one queue).  They are issued at the END of the first tap, when only the loop's 16 KB per tap are in flight, and the counted
// waits of taps 1 and 2 leave them out.  XLATE: behind the loop instead, with z an opaque zero.
template <class G>
__device__ __forceinline__ void glds_x_loads(const GldsLane<G>& L, const GemmNT& p, const GldsTile& T, uint4 (&xr)[G::XN], int z) {
  const __amdgpu_buffer_rsrc_t rsX = make_rsrc(p.bx, (unsigned)((size_t)p.M * p.N * 2));
  const int c_ = (L.tid + z) % G::CPR, rg_ = (L.tid + z) / G::CPR;
#pragma unroll
  for (int i = 0; i < G::XN; ++i) {
    const int row = rg_ + i * G::RG;
    xr[i] = buf_load16(rsX, row < G::PT ? ((unsigned)(T.m0 + row) * (unsigned)p.N + (unsigned)(L.n0 + c_ * 8)) * 2u : GLDS_OOB);
  }
}

// ---- K loop of the 14x14 / 28x28 instantiations: padded raster, taps dx-major (iteration IT: dx = IT / 3, dy = IT % 3; weight slice = tap
// dy * 3 + dx).  Per tap (K = 64 = two MFMA k-steps): [k-step 0 MFMAs | reads of this tap's NEW k-step 1 row blocks] [vmcnt + barrier: the
// next tap's weights landed, everybody is done with the previous slot] [k-step 1 MFMAs | the next tap's new k-step 0 row blocks | DMA: weights
// three taps ahead, one piece of the next chunk's image].
template <class G>
__device__ __forceinline__ void glds_k_loop_raster(const GldsLane<G>& L, const GemmNT& p, const GldsTile& T, f32x4_t (&acc)[G::TN][G::TM], uint4 (&xr)[G::XN]) {
  constexpr int TM = G::TM, TN = G::TN, VG = G::VG, AP = G::AP, BP = G::BP, NB = G::NB, A_BYTES = G::A_BYTES, B_BYTES = G::B_BYTES, XPRE = G::XPRE;
  constexpr bool ONECHUNK = G::ONECHUNK;
  const unsigned char *sA = glds_smem(), *sB = glds_smem() + G::XOFF;
  const int cpt = p.C >> 6;
  bf16x8_t fa[2][G::NRB], fb[2][TN];
  auto rd_a = [&](int ks, int rb, int dx, int boff) {
    fa[ks][rb] = *reinterpret_cast<const bf16x8_t*>(sA + ((L.a_base[dx] ^ (ks * 64)) + rb * 2048 + boff));
  };
  auto rd_b = [&](int ks, const unsigned char* cB) {
#pragma unroll
    for (int ni = 0; ni < TN; ++ni) fb[ks][ni] = *reinterpret_cast<const bf16x8_t*>(cB + (L.b_addr[ni] ^ (ks * 64)));
  };
#pragma unroll
  for (int rb = 0; rb < TM; ++rb) rd_a(0, rb, 0, 0);
  rd_b(0, sB);
  int bbuf = 0;                                          // ring slot of the current tap
  for (int cc2 = 0; cc2 < cpt; cc2 += 2) {               // channel chunks in pairs: the image buffer index is a compile-time constant
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int cc = cc2 + h;
      if (ONECHUNK && h == 1) break;
      const bool more_c = cc + 1 < cpt;
      auto tap_body = [&](auto IT_) {
        constexpr int it = decltype(IT_)::value;
        constexpr int dx = it / 3, dy = it % 3;
        constexpr int itn = it == 8 ? 0 : it + 1, dxn = itn / 3, dyn = itn % 3;
        constexpr int lo1 = dy == 0 ? 0 : TM + (dy - 1) * VG, hi1 = dy == 0 ? TM : TM + dy * VG;       // new row blocks of this tap
        constexpr int lo2 = dyn == 0 ? 0 : TM + (dyn - 1) * VG, hi2 = dyn == 0 ? TM : TM + dyn * VG;   // ... of the next tap
        constexpr int NR1 = hi1 - lo1 + TN, NR2 = hi2 - lo2 + TN, NM = TM * TN;
        constexpr bool APIECE = !ONECHUNK && it < AP;      // this tap sends piece `it` of the next chunk's image
        const int boff = (ONECHUNK ? 0 : h) * A_BYTES;
        const int boffn = (ONECHUNK ? 0 : (it == 8 ? (h ^ 1) : h)) * A_BYTES;
        const unsigned char* cB = sB + bbuf * B_BYTES;
        // ---- first half: k-step 0 MFMAs; this tap's NEW k-step 1 fragments are read between them
        if (!(GLDS_ABLATE & 4)) {
#pragma unroll
          for (int rb = lo1; rb < hi1; ++rb) rd_a(1, rb, dx, boff);
          rd_b(1, cB);
        }
        GLDS_PRIO(1);
#pragma unroll
        for (int mi = 0; mi < TM; ++mi)
#pragma unroll
          for (int ni = 0; ni < TN; ++ni) acc[ni][mi] = MFMA16(fb[0][ni], fa[0][mi + dy * VG], acc[ni][mi]);
        GLDS_PRIO(0);
#pragma unroll
        for (int i = 0; i < NR1; ++i) {
          __builtin_amdgcn_sched_group_barrier(0x008, (NM / NR1) > 0 ? (NM / NR1) : 1, 0);   // MFMAs
          __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);                               // 1 DS read
        }
        __builtin_amdgcn_sched_barrier(0);
        if (!(GLDS_ABLATE & 17)) {
          // The next chunk's image goes out ONE piece per tap (taps 0 .. AP - 1, behind the tap's weight pieces).  This tap waits for the weight
          // slice of tap it + 1, issued at tap it - 2; younger than it: the image piece of tap it - 2, then tap it - 1's weight slice and image
          // piece (and, in the first chunk of a fused launch, the x tile requested at the END of tap 0).
          constexpr int NA = ONECHUNK ? 0 : ((it >= 2 && it - 2 < AP) ? 1 : 0) + ((it >= 1 && it - 1 < AP) ? 1 : 0);
          if (XPRE > 0 && (it == 1 || it == 2) && h == 0 && cc2 == 0) glds_wait_vmcnt<BP + NA + XPRE>();
          else glds_wait_vmcnt<BP + NA>();
        }
        if (!(GLDS_ABLATE & 2)) __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        // ---- second half: k-step 1 MFMAs; the next tap's new k-step 0 fragments and this tap's DMA issue between them
        const int nb = (bbuf + 1) & (NB - 1);
        if (!(GLDS_ABLATE & 4)) {
#pragma unroll
          for (int rb = lo2; rb < hi2; ++rb) rd_a(0, rb, dxn, boffn);
          rd_b(0, sB + nb * B_BYTES);
        }
        if (!(GLDS_ABLATE & 1)) {
          constexpr int i3 = it + 3, j3 = i3 >= 9 ? i3 - 9 : i3;
          const int cc3 = i3 >= 9 ? cc + 1 : cc;
          glds_issue_b<G>(L, p, (j3 % 3) * 3 + j3 / 3, cc3, (bbuf + 3) & (NB - 1), cc3 < cpt);
          if constexpr (APIECE) glds_issue_a1<G>(L, it, cc + 1, h ^ 1, more_c);
        }
        GLDS_PRIO(1);
#pragma unroll
        for (int mi = 0; mi < TM; ++mi)
#pragma unroll
          for (int ni = 0; ni < TN; ++ni) acc[ni][mi] = MFMA16(fb[1][ni], fa[1][mi + dy * VG], acc[ni][mi]);
        GLDS_PRIO(0);
        constexpr int NE = NR2 > BP ? NR2 : BP, MP2 = (NM / NE) > 0 ? (NM / NE) : 1;
#pragma unroll
        for (int i = 0; i < NE; ++i) {
          __builtin_amdgcn_sched_group_barrier(0x008, MP2, 0);
          if (i < NR2) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
          if (i < BP + (APIECE ? 1 : 0)) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);   // 1 VMEM (LDS-DMA piece); placing them evenly over the half's MFMAs instead measured equal (profiles/r06_ab_conv_dma_spread_v1.txt)
        }
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (XPRE > 0) {
          if (it == 0 && h == 0 && cc2 == 0) {
            __builtin_amdgcn_sched_barrier(0);
            glds_x_loads<G>(L, p, T, xr, 0);
            __builtin_amdgcn_sched_barrier(0);
          }
        }
        bbuf = nb;
      };
      tap_body(std::integral_constant<int, 0>{}); tap_body(std::integral_constant<int, 1>{}); tap_body(std::integral_constant<int, 2>{});
      tap_body(std::integral_constant<int, 3>{}); tap_body(std::integral_constant<int, 4>{}); tap_body(std::integral_constant<int, 5>{});
      tap_body(std::integral_constant<int, 6>{}); tap_body(std::integral_constant<int, 7>{}); tap_body(std::integral_constant<int, 8>{});
    }
  }
}

// ---- K loop of the 224-pixel tiles (56x56, 112x112): taps in filter order (tap = dy * 3 + dx), every fragment read per tap.  Per tap (K = 64 =
// two MFMA k-steps): [28 MFMA k-step 0 | ds_read k-step 1] [vmcnt + barrier: tap+1's weights landed, everybody is done with tap-1's slot]
// [28 MFMA k-step 1 | ds_read tap+1 k-step 0 | DMA: weights of tap+3, at tap 0 the next chunk's image].
template <class G>
__device__ __forceinline__ void glds_k_loop_taps(const GldsLane<G>& L, const GemmNT& p, f32x4_t (&acc)[G::TN][G::TM]) {
  constexpr int TM = G::TM, TN = G::TN, PWL = G::PWL, AP = G::AP, BP = G::BP, NB = G::NB, A_BYTES = G::A_BYTES, B_BYTES = G::B_BYTES, NRD = G::NRD, MPR = G::MPR;
  constexpr bool ONECHUNK = G::ONECHUNK;
  const unsigned char *sA = glds_smem(), *sB = glds_smem() + G::XOFF;
  const int cpt = p.C >> 6;
  bf16x8_t f0a[TM], f0b[TN], f1a[TM], f1b[TN];
  auto read_frags = [&](bf16x8_t (&fa)[TM], bf16x8_t (&fb)[TN], int aoff, int dx, const unsigned char* cB, int ks) {
#pragma unroll
    for (int ni = 0; ni < TN; ++ni) fb[ni] = *reinterpret_cast<const bf16x8_t*>(cB + (L.b_addr[ni] ^ (ks * 64)));
#pragma unroll
    for (int mi = 0; mi < TM; ++mi) fa[mi] = *reinterpret_cast<const bf16x8_t*>(sA + (L.a_adr[dx][mi] ^ (ks * 64)) + aoff);
  };
  auto mfma_all = [&](const bf16x8_t (&fa)[TM], const bf16x8_t (&fb)[TN]) {
#pragma unroll
    for (int mi = 0; mi < TM; ++mi)
#pragma unroll
      for (int ni = 0; ni < TN; ++ni) acc[ni][mi] = MFMA16(fb[ni], fa[mi], acc[ni][mi]);
  };
  read_frags(f0a, f0b, 0, 0, sB, 0);
  int bbuf = 0;                                          // ring slot of the current tap
  for (int cc2 = 0; cc2 < cpt; cc2 += 2) {               // channel chunks in pairs: the image buffer index is a compile-time constant
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int cc = cc2 + h;
      if (ONECHUNK && h == 1) break;
      const bool more_c = cc + 1 < cpt;
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) {
        const int aoff = (ONECHUNK ? 0 : h) * A_BYTES + (tap / 3) * PWL * 128;       // buffer + vertical tap: immediates
        const int tapn = tap == 8 ? 0 : tap + 1;
        const int aoffn = (ONECHUNK ? 0 : (tap == 8 ? (h ^ 1) : h)) * A_BYTES + (tapn / 3) * PWL * 128;
        const unsigned char* cB = sB + bbuf * B_BYTES;
        // ---- first half: k-step 0 MFMAs, with the fragment reads of k-step 1 threaded between them
        if (!(GLDS_ABLATE & 4)) read_frags(f1a, f1b, aoff, tap % 3, cB, 1);
        GLDS_PRIO(1);
        mfma_all(f0a, f0b);
        GLDS_PRIO(0);
#pragma unroll
        for (int i = 0; i < NRD; ++i) {
          __builtin_amdgcn_sched_group_barrier(0x008, MPR, 0);   // MFMAs
          __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);     // 1 DS read
        }
        __builtin_amdgcn_sched_barrier(0);
        // Loads younger than the tile we need (tap+1, issued two taps ago) stay in flight: the tile of tap+2 and the next
        // chunk's image when it was issued after it (at tap 0 of this chunk: seen from taps 1 and 2).
        if (!(GLDS_ABLATE & 1)) { if (!ONECHUNK && (tap == 1 || tap == 2)) glds_wait_vmcnt<BP + AP>(); else glds_wait_vmcnt<BP>(); }
        if (!(GLDS_ABLATE & 2)) __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        // ---- second half: k-step 1 MFMAs, threaded with the reads of tap+1 / k-step 0 and this tap's DMA issue
        const int nb = (bbuf + 1) & (NB - 1);
        if (!(GLDS_ABLATE & 4)) read_frags(f0a, f0b, aoffn, tapn % 3, sB + nb * B_BYTES, 0);
        if (!(GLDS_ABLATE & 1)) {
          const int t3 = tap + 3;
          const int tap3 = t3 >= 9 ? t3 - 9 : t3, cc3 = t3 >= 9 ? cc + 1 : cc;
          glds_issue_b<G>(L, p, tap3, cc3, (bbuf + 3) & (NB - 1), cc3 < cpt);
          if (!ONECHUNK && tap == 0) glds_issue_a<G>(L, cc + 1, h ^ 1, more_c);
        }
        GLDS_PRIO(1);
        mfma_all(f1a, f1b);
        GLDS_PRIO(0);
#pragma unroll
        for (int i = 0; i < BP; ++i) {
          __builtin_amdgcn_sched_group_barrier(0x008, MPR, 0);   // MFMAs
          __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);     // 1 DS read
          __builtin_amdgcn_sched_group_barrier(0x008, MPR, 0);
          __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
          __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);     // 1 VMEM (LDS-DMA piece)
        }
#pragma unroll
        for (int i = 0; i < NRD - 2 * BP; ++i) {
          __builtin_amdgcn_sched_group_barrier(0x008, MPR, 0);
          __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
        bbuf = nb;
      }
    }
  }
}

// ---- behind the K loop: request what the fused epilogue needs, drain the (zero-writing) tail DMAs, wait until every wave is past its last
// fragment read.  The per-channel coefficients are requested HERE, in front of the drain / right behind the late x tile, as whole-vector loads:
// left to hipcc they became 62 dword loads each issued right before its first use (19 exposed waits = 10 of the epilogue's 11 us).
template <class G>
__device__ __forceinline__ void glds_drain(const GldsLane<G>& L, const GemmNT& p, const GldsTile& T, GldsFused<G>& F) {
  // papply: (bias, slope) vectors of this thread's 8 channels.  Branch-free (a branch between these loads and the barrier below made hipcc wait
  // for the x tile in front of it): without a bias the first vector is read from the slopes and never used.
  auto load_slopes = [&](int z) {
    const unsigned co = (unsigned)(L.n0 + (L.tid % G::CPR) * 8 + z) * 4u;
    const float* arr[2] = {p.bbeta ? p.bbeta : p.balpha, p.balpha};
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      const __amdgpu_buffer_rsrc_t rs = make_rsrc(arr[a], (unsigned)p.N * 4u);
      const uint4 lo = buf_load16(rs, co), hi = buf_load16(rs, co + 16u);
      F.fc[a][0] = make_float4(__uint_as_float(lo.x), __uint_as_float(lo.y), __uint_as_float(lo.z), __uint_as_float(lo.w));
      F.fc[a][1] = make_float4(__uint_as_float(hi.x), __uint_as_float(hi.y), __uint_as_float(hi.z), __uint_as_float(hi.w));
    }
  };
  if constexpr (G::EPI == Epi::papply && !G::XLATE) load_slopes(0);
  glds_wait_vmcnt<0>();
  if constexpr (G::XLATE) {
    const int z = opaque_zero<true>();
    glds_x_loads<G>(L, p, T, F.xr, z);
    if constexpr (G::EPI == Epi::papply) load_slopes(z);
  }
  if constexpr (G::EPI == Epi::bnbwd) {                    // this lane's channel, requested now, used behind the MFMA chain
    const int tz = L.tid + opaque_zero<(G::TPW > 1)>();
    const int ch = L.n0 + ((tz >> 6) << 4) + (tz & 15);
    F.cf[0] = 0.f; F.cf[1] = F.cf[2] = F.cf[4] = 1.f; F.cf[3] = 0.f;
    if (!p.bmom || p.balpha) { F.cf[0] = p.bmean[ch]; F.cf[1] = p.brstd[ch]; }
    if (p.balpha) { F.cf[2] = p.bgamma ? p.bgamma[ch] : 1.f; F.cf[3] = p.bbeta ? p.bbeta[ch] : 0.f; F.cf[4] = p.balpha[ch]; }
  }
  // (LDS only: __syncthreads() would also wait for the x / coefficient loads just issued — vmcnt(7) in the several-tiles variant, whose x tile was
  // requested a few instructions ago)
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
}

// ---- staging: the accumulators as a 16-bit tile [PT][BN] (row pitch CST) at the start of LDS; fragment rows outside the tile contribute nothing.
// ESC: eval-mode BatchNorm (+PReLU) of the output, on the fp32 accumulator.  Two copies behind ONE uniform branch in the caller: with the test
// inside, every one of the 56 values per lane paid a scalar branch around the affine.  ssum / ssq: the register statistics of the 224-pixel tiles.
template <class G, bool ESC>
__device__ __forceinline__ void glds_stage_tile(const GldsLane<G>& L, const GemmNT& p, const f32x4_t (&acc)[G::TN][G::TM], float (&ssum)[G::TN][4], float (&ssq)[G::TN][4]) {
  constexpr int TM = G::TM, TN = G::TN, PT = G::PT, CST = G::CST;
  unsigned char* sC = glds_smem();
  float esc_[TN][4], esh_[TN][4], eal_[TN][4];
  if constexpr (ESC) {
#pragma unroll
    for (int ni = 0; ni < TN; ++ni)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int n = L.n0 + L.wn * (G::BN / G::WN) + ni * 16 + L.lg * 4 + q;
        esc_[ni][q] = p.esc[n]; esh_[ni][q] = p.esh[n]; eal_[ni][q] = p.ealpha ? p.ealpha[n] : 1.f;
      }
  }
#pragma unroll
  for (int ni = 0; ni < TN; ++ni)
#pragma unroll
    for (int mi = 0; mi < TM; ++mi) {
      int ml = L.m_pix[mi];
      bool mok = L.m_ok[mi];
      if constexpr (G::TPW > 1 && G::RST) {                // (recomputed per tile: opaque_zero)
        const int q_ = L.wm * G::MW + mi * 16 + L.l15 + opaque_zero<true>();
        const int y_ = q_ / G::PWL, x_ = q_ - y_ * G::PWL;
        mok = x_ < G::W;
        ml = mok ? y_ * G::W + x_ : 0;
      }
      // (padded-raster kernels: the filler columns' lanes write to a dump row behind the tile instead of sitting out a predicated store — 14
      // s_and_saveexec / taken-branch pairs per lane in a phase that is pure overhead for the matrix cores; nothing reads row PT: the copy-out stops
      // in front of it, the transposed statistics reads select zeros beyond the tile, the x tile of the fused variants starts 1 KB-aligned behind it)
      if constexpr (G::DUMP) ml = mok ? ml : PT;
      const int nl = L.wn * (G::BN / G::WN) + ni * 16 + L.lg * 4;
      bf16_t h[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float a = acc[ni][mi][q];
        if constexpr (ESC) {
          a = a * esc_[ni][q] + esh_[ni][q];
          if (p.ealpha) a = a > 0.f ? a : eal_[ni][q] * a;
        }
        h[q] = f2bf(a);
        if constexpr (!G::MST) {
          const float v = mok ? bf2f(h[q]) : 0.f;
          ssum[ni][q] += v;
          ssq[ni][q] += v * v;
        }
      }
      uint2 pk;
      pk.x = (unsigned)h[0] | ((unsigned)h[1] << 16);
      pk.y = (unsigned)h[2] | ((unsigned)h[3] << 16);
      if constexpr (G::XLATE) {
        // inline asm on purpose: the several-tiles fused variant has just requested its x tile, and hipcc — which cannot see that the asm waits of
        // the K loop retired every LDS-DMA — puts a counted vmcnt wait in front of each LDS store it emits itself: 5 of the 7 x loads, in the open
        typedef __attribute__((ext_vector_type(2))) unsigned st8_u2_t;
        const st8_u2_t pv = {pk.x, pk.y};
        const unsigned sadr = (unsigned)reinterpret_cast<size_t>((lds_ptr_t)(sC + ml * CST + nl * 2));
        if (G::DUMP || mok) asm volatile("ds_write_b64 %0, %1" ::"v"(sadr), "v"(pv) : "memory");
      } else {
        if (G::DUMP || mok) *reinterpret_cast<uint2*>(sC + ml * CST + nl * 2) = pk;
      }
    }
}

// the BatchNorm finalize sums gemm_nt_stat_rows(M, N) partial rows (128-pixel tiling): zero the ones a one-tile-per-workgroup tiling leaves
template <class G>
__device__ __forceinline__ void zero_unused_stat_rows(const GldsLane<G>& L, const GemmNT& p, int bt, int stat_rows) {
  constexpr int LPR = G::BN / G::WN / 4;                   // (sum, sumsq) x this wave's BN/WN columns, one float4 per lane
  const int ntile = gridDim.x / p.nbn;
  for (int row = ntile * G::WM + bt * G::WM + L.wm; row < stat_rows; row += ntile * G::WM)
    if (L.lane < 2 * LPR) {
      float* z = p.stats + (size_t)row * 2 * p.N + (L.lane / LPR) * p.N + L.n0 + L.wn * (G::BN / G::WN);
      *reinterpret_cast<float4*>(z + (L.lane % LPR) * 4) = make_float4(0.f, 0.f, 0.f, 0.f);
    }
}
// register statistics of the 224-pixel tiles: one partial row per wave row
template <class G>
__device__ __forceinline__ void glds_stats_registers(const GldsLane<G>& L, const GemmNT& p, int bt, int stat_rows, const float (&ssum)[G::TN][4], const float (&ssq)[G::TN][4]) {
  float* prow_ = p.stats + (size_t)(bt * G::WM + L.wm) * 2 * p.N;
#pragma unroll
  for (int ni = 0; ni < G::TN; ++ni)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float a = row16_sum(ssum[ni][q]), b = row16_sum(ssq[ni][q]);
      const int n = L.n0 + L.wn * (G::BN / G::WN) + ni * 16 + L.lg * 4 + q;
      if (L.l15 == 0) {
        prow_[n] = a;
        prow_[p.N + n] = b;
      }
    }
  zero_unused_stat_rows<G>(L, p, bt, stat_rows);
}

// the staged tile to global memory: all LDS reads first, then the stores (the store helper is an asm statement the compiler will not move a load across)
template <class G>
__device__ __forceinline__ void copy_out(const GemmNT& p, int m0, int n0, int tidz) {
  constexpr int CPR = G::CPR, NT = G::NT, PT = G::PT, NIT = (PT * CPR + NT - 1) / NT;
  const unsigned char* sC = glds_smem();
  uint4 v[NIT];
#pragma unroll
  for (int k = 0; k < NIT; ++k) {
    const int idx = tidz + k * NT;
    const int row = idx / CPR, c = idx - row * CPR;
    if ((k + 1) * NT <= PT * CPR || idx < PT * CPR) v[k] = *reinterpret_cast<const uint4*>(sC + row * G::CST + c * 16);
  }
#pragma unroll
  for (int k = 0; k < NIT; ++k) {
    const int idx = tidz + k * NT;
    const int row = idx / CPR, c = idx - row * CPR;
    if ((k + 1) * NT <= PT * CPR || idx < PT * CPR) glds_store_out(p.Cb + (size_t)(m0 + row) * p.ldc + n0 + c * 8, v[k]);
  }
}

// Statistics on the matrix cores.  In-kernel stamps priced the register statistics at 1.9 us of VALU work on the accumulators + 1.1 us of DPP
// row sums and 4-byte stores of a 29 us launch, all with the matrix cores idle.  They are column sums of the STAGED tile Y (16-bit, in LDS):
//   sum_m Y[m][n] = (ones x Y)[.][n]          sum_m Y[m][n]^2 = diag(Y^T Y)[n]
// — wave w takes channels 16 w .. 16 w + 15; per 32-pixel step ks ONE transposed fragment serves as A and B operand.  Products of two 16-bit
// values are exact in fp32 and the accumulation is fp32 (another summation order than the register sums).
// The reader: lane (g = lane >> 4, li = lane & 15) reads 8 B of row 8 g + (li >> 2) (+ 4 for the second read), columns 4 (li & 3) .. + 3 of this
// wave's 16 (tb points there); the transposing read hands lane li column li's values of rows 8 g .. 8 g + 3 — a 16 x 16 x 32 operand fragment of
// Y^T / Y.  Rows beyond the tile hold stale LDS contents: zeros are selected (PT % 4 == 0: a group of 4 rows is in or out).
template <class G>
__device__ __forceinline__ s16x8_t tr_frag(const unsigned char* tb, int ks, int lgz) {
  typedef __attribute__((address_space(3))) s16x4_t* lds_tr_p;
  s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_tr_p)(tb + ks * 32 * G::CST));
  s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_tr_p)(tb + ks * 32 * G::CST + 4 * G::CST));
  if ((ks + 1) * 32 > G::PT) {
    const bool lo_ok = ks * 32 + 8 * lgz < G::PT, hi_ok = ks * 32 + 8 * lgz + 4 < G::PT;
#pragma unroll
    for (int j = 0; j < 4; ++j) { lo[j] = lo_ok ? lo[j] : (short)0; hi[j] = hi_ok ? hi[j] : (short)0; }
  }
  s16x8_t f8;
  f8[0] = lo[0]; f8[1] = lo[1]; f8[2] = lo[2]; f8[3] = lo[3];
  f8[4] = hi[0]; f8[5] = hi[1]; f8[6] = hi[2]; f8[7] = hi[3];
  return f8;
}
__device__ __forceinline__ bf16x8_t ones_frag() {
  s16x8_t one8;
#pragma unroll
  for (int j = 0; j < 8; ++j) one8[j] = FEDFR_FP16 ? (short)0x3c00 : (short)0x3f80;
  return __builtin_bit_cast(bf16x8_t, one8);
}
// where lane (lgz, l15z) of wave wavez starts its transposed reads of a staged tile at `tile`
template <class G>
__device__ __forceinline__ const unsigned char* tr_base(const unsigned char* tile, int wavez, int lgz, int l15z) {
  return tile + (8 * lgz + (l15z >> 2)) * G::CST + (wavez * 16 + 4 * (l15z & 3)) * 2;
}

// ---- epilogue, Epi::plain.  MST: copy-out + matrix-core statistics (one partial row per tile, or the workgroup's running row); the launches
// with a residual add / second output (one tile per workgroup only) and the 224-pixel tiles take the per-element copy-out.
template <class G>
__device__ __forceinline__ void glds_epilogue_plain(const GldsLane<G>& L, const GemmNT& p, const GldsTile& T, int ti, int stat_rows) {
  constexpr int BN = G::BN, CPR = G::CPR, CST = G::CST, PT = G::PT, TPW = G::TPW;
  const unsigned char* sC = glds_smem();
  const bool extras = TPW == 1 && (p.eadd || p.Cb2);       // (compiled out of the two-tiles-per-workgroup instantiation, which sits at the register limit: with
                                                           // this block in it spilled — 256 VGPRs + 128 B of scratch per lane, 34 -> 51 us per 28x28 conv)
  if constexpr (G::MST) {
    const int tidz = L.tid + opaque_zero<(TPW > 1)>();
    const int l15z = tidz & 15, lgz = (tidz >> 4) & 3, wavez = tidz >> 6;
    if (!extras) copy_out<G>(p, T.m0, L.n0, tidz);
    if (p.stats) {
      constexpr int KS = (PT + 31) / 32;
      const unsigned char* tb = tr_base<G>(sC, wavez, lgz, l15z);
      f32x4_t gq = {0.f, 0.f, 0.f, 0.f}, gs = {0.f, 0.f, 0.f, 0.f};
      const bf16x8_t ones = ones_frag();
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const bf16x8_t fr = __builtin_bit_cast(bf16x8_t, tr_frag<G>(tb, ks, lgz));
        gq = MFMA16(fr, fr, gq);                               // Y^T Y: lane holds rows 4 g .. 4 g + 3 of column li
        gs = MFMA16(ones, fr, gs);                             // every row = the column sums
      }
      // the diagonal of the 16 x 16 Gram block lives in the 16 lanes with (li >> 2) == g, register li & 3
      const float sq = diag_pick(gq, l15z & 3);
      if ((l15z >> 2) == lgz) {
        const int col = wavez * 16 + l15z;
        if constexpr (TPW == 1) {
          float* prow_ = p.stats + (size_t)(T.bt * G::WM) * 2 * p.N + L.n0 + col;
          prow_[0] = gs[0];
          prow_[p.N] = sq;
          prow_[2 * (size_t)p.N] = 0.f;                        // the tile's second row slot (the register path leaves one row per wave row)
          prow_[3 * (size_t)p.N] = 0.f;
        } else {
          float* d = reinterpret_cast<float*>(glds_smem() + G::STAT_OFF) + col;
          running_row_add(d, ti, gs[0]);
          running_row_add(d + BN, ti, sq);
        }
      }
      if constexpr (TPW == 1) zero_unused_stat_rows<G>(L, p, T.bt, stat_rows);
    }
  }
  if (!G::MST || extras)
    for (int idx = L.tid; idx < PT * CPR; idx += G::NT) {
      const int row = idx / CPR, c = idx - row * CPR;
      uint4 v = *reinterpret_cast<const uint4*>(sC + row * CST + c * 16);
      const size_t go = (size_t)(T.m0 + row) * p.ldc + L.n0 + c * 8;
      if (extras) {
        float f[8];
        unpack8(v, f);
        if (p.eadd) {                                        // + identity path (one more bf16 rounding than the separate bn_apply pass)
          float g[8];
          unpack8(*reinterpret_cast<const uint4*>(p.eadd + go), g);
#pragma unroll
          for (int q = 0; q < 8; ++q) f[q] += g[q];
          v = pack8(f);
          unpack8(v, f);
        }
        if (p.Cb2) {                                         // the next block's bn1 of the (bf16) output; or sphnet's activation (gemm.h)
          float y2[8];
          if (p.e2alpha || !p.esc2) {
            float a2[8];
            if (p.e2add) unpack8(*reinterpret_cast<const uint4*>(p.e2add + go), a2);
#pragma unroll
            for (int q = 0; q < 8; ++q) {
              const int n = L.n0 + c * 8 + q;
              float t = f[q] * (p.esc2 ? p.esc2[n] : 1.f) + (p.esh2 ? p.esh2[n] : 0.f);
              if (p.e2alpha) t = t > 0.f ? t : p.e2alpha[n] * t;
              y2[q] = p.e2add ? t + a2[q] : t;
            }
          } else {
#pragma unroll
            for (int q = 0; q < 8; ++q) y2[q] = f[q] * p.esc2[L.n0 + c * 8 + q] + p.esh2[L.n0 + c * 8 + q];
          }
          *reinterpret_cast<uint4*>(p.Cb2 + go) = pack8(y2);
        }
      }
      glds_store_out(p.Cb + go, v);
    }
}

// bnbwd, in front of the barrier: the BatchNorm input tile X joins the staged tile in LDS (same layout, at SXOFF behind it)
template <class G>
__device__ __forceinline__ void glds_park_x(const GldsLane<G>& L, const uint4 (&xr)[G::XN]) {
  const int tz = L.tid + opaque_zero<G::XLATE>();
  const int c = tz % G::CPR, rg = tz / G::CPR;
#pragma unroll
  for (int i = 0; i < G::XN; ++i) {
    const int row = rg + i * G::RG;
    if ((i + 1) * G::RG <= G::PT || row < G::PT) *reinterpret_cast<uint4*>(glds_smem() + G::SXOFF + row * G::CST + c * 16) = xr[i];
  }
}
// ---- epilogue, Epi::bnbwd: the reduction's column sums on the matrix cores, as glds_epilogue_plain's.  Per 32-pixel step one transposed
// fragment of the staged tile DY and one of X give
//   sum dy = (ones x DY)[.][n]      sum dy * x = diag(DY^T X)[n]      (forward raw moments: + diag(DY^T DY))
// With a PReLU in front (p.balpha: dz = dy * (z <= 0 ? alpha : 1), z = x * sc + sh) the mask is not bilinear — but it is a THRESHOLD on x:
// z <= 0  <=>  sgn(sc) x <= T = -sh / |sc|  <=>  t16 - sgn(sc) x >= 0 with t16 = the largest fp16 <= T, and the fp16 difference of two fp16 values
// has the exact sign.  One packed FMA + one packed shift + one AND per PAIR of elements build DYPOS = (z > 0 ? dy : 0) on the fragment, and
//   sum dz = S(dypos) + alpha (S(dy) - S(dypos)),  sum dz * x likewise,  sum_{z <= 0} dy * z = sc (S(dy x) - S(dypos x)) + sh (S(dy) - S(dypos))
// (the bf16 build has no packed arithmetic on its storage type: it compares the two halves of a fragment register as fp32 against T itself — 7
// operations per pair instead of 3).
template <class G>
__device__ __forceinline__ void glds_epilogue_bnbwd(const GldsLane<G>& L, const GemmNT& p, const GldsTile& T, int ti, const float (&cf)[5]) {
  constexpr int BN = G::BN, KS = (G::PT + 31) / 32;
  const int tidz = L.tid + opaque_zero<(G::TPW > 1)>();
  const int l15z = tidz & 15, lgz = (tidz >> 4) & 3, wavez = tidz >> 6;
  const bool diag = (l15z >> 2) == lgz;
  const int col = wavez * 16 + l15z;
  // (the coefficient arithmetic comes BEFORE the copy-out: vmcnt counts loads and stores on gfx9 and they retire out of order with each other,
  // so a wait for the coefficient loads placed behind the tile's stores is a vmcnt(0) that sits out the write-through stores — ~1 us, asm-checked)
  const bool prelu = p.balpha != nullptr;
  // PReLU threshold of this lane's channel (epi_mfma.h): z = x * sc + sh, sc = gamma * rstd, sh = beta - mean * sc
  const float sc_ = cf[2] * cf[1], sh_ = cf[3] - cf[0] * sc_;
  PreluThr th = {0u, 0u, 0.f, 0.f};
  if (prelu) th = prelu_threshold(sc_, sh_);
  asm volatile("" ::"v"(th.t162), "v"(th.nsgn2), "v"(sc_), "v"(sh_), "v"(th.Tf), "v"(th.nsf), "v"(cf[0]), "v"(cf[1]), "v"(cf[4]));     // (materialised here)
  __builtin_amdgcn_sched_barrier(0);
  copy_out<G>(p, T.m0, L.n0, tidz);
  const unsigned char* tb = tr_base<G>(glds_smem(), wavez, lgz, l15z);
  f32x4_t g1 = {0.f, 0.f, 0.f, 0.f}, g2 = {0.f, 0.f, 0.f, 0.f}, g3 = {0.f, 0.f, 0.f, 0.f}, g4 = {0.f, 0.f, 0.f, 0.f};
  const bf16x8_t ones = ones_frag();
  const bool mom = p.bmom != 0;
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    const s16x8_t d8 = tr_frag<G>(tb, ks, lgz), x8 = tr_frag<G>(tb + G::SXOFF, ks, lgz);
    const bf16x8_t dfr = __builtin_bit_cast(bf16x8_t, d8), xfr = __builtin_bit_cast(bf16x8_t, x8);
    g1 = MFMA16(ones, dfr, g1);                            // every row: sum over the pixels of dy (forward: y)
    g2 = MFMA16(dfr, xfr, g2);                             // diagonal: sum dy * x
    if (mom) g3 = MFMA16(dfr, dfr, g3);                    // forward raw moments: sum y * y
    if (prelu) {
      const s16x8_t pu = prelu_pos(d8, x8, th);
      const bf16x8_t pfr = __builtin_bit_cast(bf16x8_t, pu);
      g3 = MFMA16(ones, pfr, g3);                          // sum dypos
      g4 = MFMA16(pfr, xfr, g4);                           // diagonal: sum dypos * x
    }
  }
  const int qd = l15z & 3;
  float t0 = g1[0], t1 = diag_pick(g2, qd), t2 = diag_pick(g3, qd);
  if (prelu) {
    const float sp = g3[0], spx = diag_pick(g4, qd);
    const float sn = t0 - sp, snx = t1 - spx;              // sums over the elements with z <= 0
    t0 = sp + cf[4] * sn;
    t1 = spx + cf[4] * snx;
    t2 = sc_ * snx + sh_ * sn;
  }
  if (diag) {
    if constexpr (G::XLATE) {
      float* d = reinterpret_cast<float*>(glds_smem() + G::STAT_OFF) + col;
      running_row_add(d, ti, t0);
      running_row_add(d + BN, ti, t1);
      running_row_add(d + 2 * BN, ti, t2);
    } else {
      float* o = p.bpart + (size_t)T.bt * 3 * p.N + L.n0 + col;
      o[0] = t0;
      o[p.N] = p.bmom ? t1 : cf[1] * (t1 - cf[0] * t0);
      o[2 * (size_t)p.N] = t2;
    }
  }
}

// ---- epilogue, Epi::papply: a bare PReLU(+bias) sits in front of the conv's input side — z = x + bias (bias in p.bbeta, or none), the OUTPUT is
// dz = dy * (z <= 0 ? alpha : 1), and the partial rows are (sum dz, sum dy z over z <= 0) twice: what a PReLU's parameter sums need.  Per-element:
// thread owns chunk column c (8 channels) of rows rg, rg + RG, ...; dy from the staged tile, x from the registers.  The row groups' sums meet
// in the weight ring (drained before the staging).
template <class G>
__device__ __forceinline__ void glds_epilogue_papply(const GldsLane<G>& L, const GemmNT& p, const GldsTile& T, int ti, const GldsFused<G>& F) {
  constexpr int BN = G::BN, CPR = G::CPR, RG = G::RG;
  const unsigned char* sC = glds_smem();
  const int tz = L.tid + opaque_zero<G::XLATE>();
  const int c = tz % CPR, rg = tz / CPR;
  const int n = L.n0 + c * 8;
  float s1[8], s3[8], sh[8], al[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    auto at = [&](int a) { const float4 v = F.fc[a][q >> 2]; return (q & 3) == 0 ? v.x : (q & 3) == 1 ? v.y : (q & 3) == 2 ? v.z : v.w; };
    s1[q] = s3[q] = 0.f;
    sh[q] = p.bbeta ? at(0) : 0.f;
    al[q] = at(1);
  }
#pragma unroll
  for (int i = 0; i < G::XN; ++i) {
    const int row = rg + i * RG;
    if (row < G::PT) {
      float dy[8], xv[8], dzv[8];
      unpack8(*reinterpret_cast<const uint4*>(sC + row * G::CST + c * 16), dy);
      unpack8(F.xr[i], xv);
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const float z = xv[q] + sh[q];
        const bool neg = z <= 0.f;
        s3[q] += neg ? dy[q] * z : 0.f;
        dzv[q] = neg ? dy[q] * al[q] : dy[q];
        s1[q] += dzv[q];
      }
      glds_store_out(p.Cb + (size_t)(T.m0 + row) * p.ldc + n, pack8(dzv));
    }
  }
  float* red = reinterpret_cast<float*>(glds_smem() + G::XOFF);      // [RG][2][BN]
  *reinterpret_cast<float4*>(red + (rg * 2 + 0) * BN + c * 8) = make_float4(s1[0], s1[1], s1[2], s1[3]);
  *reinterpret_cast<float4*>(red + (rg * 2 + 0) * BN + c * 8 + 4) = make_float4(s1[4], s1[5], s1[6], s1[7]);
  *reinterpret_cast<float4*>(red + (rg * 2 + 1) * BN + c * 8) = make_float4(s3[0], s3[1], s3[2], s3[3]);
  *reinterpret_cast<float4*>(red + (rg * 2 + 1) * BN + c * 8 + 4) = make_float4(s3[4], s3[5], s3[6], s3[7]);
  __syncthreads();
  if (L.tid < BN) {                                        // one thread per column: the sums over the row groups
    float t0 = 0.f, t2 = 0.f;
#pragma unroll 8
    for (int r = 0; r < RG; ++r) {
      t0 += red[(r * 2 + 0) * BN + L.tid];
      t2 += red[(r * 2 + 1) * BN + L.tid];
    }
    if constexpr (G::XLATE) {
      float* d = reinterpret_cast<float*>(glds_smem() + G::STAT_OFF) + L.tid;
      running_row_add(d, ti, t0);
      running_row_add(d + 2 * BN, ti, t2);
    } else {
      float* o = p.bpart + (size_t)T.bt * 3 * p.N + L.n0 + L.tid;
      o[0] = t0;
      o[p.N] = t2;
      o[2 * (size_t)p.N] = t2;
    }
  }
}

// ---- behind the tile loop (several tiles per workgroup): the workgroup's running row leaves LDS (every tile's epilogue ended with a barrier)
template <class G>
__device__ __forceinline__ void glds_workgroup_tail(const GldsLane<G>& L, const GemmNT& p, int btw, int stat_rows) {
  constexpr int BN = G::BN;
  const float* sStat = reinterpret_cast<const float*>(glds_smem() + G::STAT_OFF);
  if constexpr (G::XLATE) {
    if (L.tid < BN) {
      const int ch = L.n0 + L.tid;
      const float t0 = sStat[L.tid], t2 = sStat[2 * BN + L.tid];
      float* o = p.bpart + (size_t)btw * 3 * p.N + ch;
      o[0] = t0;
      if constexpr (G::EPI == Epi::papply) o[p.N] = t2;
      else o[p.N] = p.bmom ? sStat[BN + L.tid] : p.brstd[ch] * (sStat[BN + L.tid] - p.bmean[ch] * t0);
      o[2 * (size_t)p.N] = t2;
    }
  } else if (p.stats) {
    const int nrows = gridDim.x / p.nbn;
    for (int i = L.tid; i < 2 * BN; i += G::NT) {
      const int stat = i / BN, col = i - stat * BN;
      p.stats[(size_t)btw * 2 * p.N + (size_t)stat * p.N + L.n0 + col] = sStat[i];
    }
    // rows the finalize kernel's row count (128-pixel tiling) has beyond ours: zeros
    for (int row = nrows + btw; row < stat_rows; row += nrows)
      for (int i = L.tid; i < 2 * BN / 4; i += G::NT) {
        const int stat = i / (BN / 4), c4 = i - stat * (BN / 4);
        *reinterpret_cast<float4*>(p.stats + (size_t)row * 2 * p.N + (size_t)stat * p.N + L.n0 + c4 * 4) = make_float4(0.f, 0.f, 0.f, 0.f);
      }
  }
}

// Template parameters of an instantiation (GldsGeom derives everything else):
//   W_, R_     map width (= height); image rows per tile: tile = R_ * W_ output pixels (196 or 224)
//   NPA        LDS-DMA pieces (1 KiB = 8 padded-image rows) per image buffer
//   WN         wave columns.  2: 4 waves, one per SIMD (112 x 64 wave tiles); 4: 8 waves, two per SIMD (112 x 32)
//   EPI        what the epilogue does (Epi above)
//   BN_        output-channel tile
//   ONECHUNK   C == 64: one channel chunk, a single image buffer
//   TPW        image tiles a workgroup computes one after the other.  2: half as many BatchNorm partial rows — one per workgroup, summed over its
//              tiles — so that the channel-sliced BatchNorm pass can reduce them itself (bn_sliced.hip)
template <int W_, int R_, int NPA, int WN, Epi EPI, int BN_ = 128, bool ONECHUNK = false, int TPW = 1>
__global__ __launch_bounds__(128 * WN) void conv3x3_glds_kernel(GemmNT p, int stat_rows) {
  using G = GldsGeom<W_, R_, NPA, WN, EPI, BN_, ONECHUNK, TPW>;
  GLDS_STAMP(0);
  const int lid = xcd_remap(blockIdx.x, gridDim.x);
  const int btw = lid / p.nbn;                            // workgroup btw computes image tiles btw * TPW .. + TPW - 1
  GldsLane<G> L;
  glds_lane_init<G>(L, p, lid % p.nbn);
  GldsFused<G> F;
  f32x4_t acc[G::TN][G::TM];
#pragma unroll 1
  for (int ti = 0; ti < TPW; ++ti) {
    const GldsTile T = glds_plan_tile<G>(L, p, btw * TPW + ti);
#pragma unroll
    for (int a = 0; a < G::TN; ++a)
#pragma unroll
      for (int b = 0; b < G::TM; ++b) acc[a][b] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    // (GLDS_ABLATE & 8: what the second tile's prologue costs — it computes on stale LDS contents)
    glds_prologue<G>(L, p, (GLDS_ABLATE & 8) && TPW > 1 && ti > 0);
    GLDS_STAMP(1);
    if constexpr (G::RST) glds_k_loop_raster<G>(L, p, T, acc, F.xr);
    else glds_k_loop_taps<G>(L, p, acc);
    glds_drain<G>(L, p, T, F);
    GLDS_STAMP(2);
    float ssum[G::TN][4] = {}, ssq[G::TN][4] = {};        // register statistics of this wave's columns (224-pixel tiles)
    // (the launcher refuses the output affine on a fused variant; compiled out of it: its 24 conditional loads made every staging write of the
    // fused two-tiles variant wait for the x tile)
    if (!G::FUSED && p.esc != nullptr) glds_stage_tile<G, true>(L, p, acc, ssum, ssq);
    else glds_stage_tile<G, false>(L, p, acc, ssum, ssq);
    GLDS_STAMP(4);                                        // (staged: conversions, statistics sums and LDS writes of this wave are issued)
    if constexpr (!G::MST) { if (p.stats) glds_stats_registers<G>(L, p, T.bt, stat_rows, ssum, ssq); }
    if constexpr (EPI == Epi::bnbwd) glds_park_x<G>(L, F.xr);
    GLDS_STAMP(5);
    if constexpr (G::XLATE) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // (the asm staging writes)
    __syncthreads();
    GLDS_STAMP(6);
    if constexpr (EPI == Epi::plain) glds_epilogue_plain<G>(L, p, T, ti, stat_rows);
    else if constexpr (EPI == Epi::bnbwd) glds_epilogue_bnbwd<G>(L, p, T, ti, F.cf);
    else glds_epilogue_papply<G>(L, p, T, ti, F);
    if (TPW > 1) __syncthreads();                         // the staged output tile has been read: the next tile's image may land on it
  }
  GLDS_STAMP(7);
  if constexpr (TPW > 1) glds_workgroup_tail<G>(L, p, btw, stat_rows);
  GLDS_STAMP(3);
}

template <int W_, int R_, int NPA, int WN, Epi EPI, int BN_ = 128, bool ONECHUNK = false, int TPW = 1>
static int launch_glds(GemmNT p, const NtPlan& plan, hipStream_t st) {
  using G = GldsGeom<W_, R_, NPA, WN, EPI, BN_, ONECHUNK, TPW>;
  constexpr int PT = G::PT;
  FEDFR_REQUIRE(p.N % BN_ == 0 && (ONECHUNK ? p.C == 64 : p.C % 128 == 0) && p.H == W_ && p.W == W_ && p.M % (W_ * W_) == 0 && p.K == 9 * p.C && p.ldc % 8 == 0,
                "conv3x3_glds: unsupported shape (N=%d C=%d H=%d W=%d M=%d)", p.N, p.C, p.H, p.W, p.M);
  FEDFR_REQUIRE(G::FUSED == (p.bpart != nullptr), "conv3x3_glds: fused / plain variant mismatch");
  if (G::FUSED) {
    FEDFR_REQUIRE(p.bx && p.bmean && p.brstd && p.ldc == p.N, "conv3x3_glds: fused BN-bwd reduction needs bx / mean / rstd and ldc == N");
    FEDFR_REQUIRE(!p.stats, "conv3x3_glds: a fused-epilogue launch leaves reduction rows (bpart), not forward statistics");
    FEDFR_REQUIRE(p.bmom != 2 || p.balpha, "conv3x3_glds: the PReLU-apply epilogue needs the slopes");
    FEDFR_REQUIRE((p.bmom == 2) == (EPI == Epi::papply), "conv3x3_glds: the PReLU-apply epilogue (bmom == 2) lives in the Epi::papply instantiations, and only it");
    FEDFR_REQUIRE(plan.part_rows == p.M / PT / TPW, "conv3x3_glds: the plan counts %d partial rows, the launch leaves %d", plan.part_rows, p.M / PT / TPW);
  }
  p.nbn = p.N / BN_;
  FEDFR_REQUIRE((p.M / PT) % TPW == 0, "conv3x3_glds: %d tiles do not split into groups of %d", p.M / PT, TPW);
  const int ntile = p.M / PT / TPW;                     // workgroups per output-channel tile
  const auto kernel = &conv3x3_glds_kernel<W_, R_, NPA, WN, EPI, BN_, ONECHUNK, TPW>;
  static PerDeviceOnce attr_once;     // hipFuncSetAttribute is per device (a Server process may drive several)
  attr_once.run([&] { hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); });
  ProfScope prof(G::SLOT, 2.0 * p.M * p.N * (double)p.K, st, gemm_nt_alg_bytes(p, 1));
  hipLaunchKernelGGL(kernel, dim3(ntile * p.nbn), dim3(128 * WN), G::LDS, st, p, gemm_nt_stat_rows(p.M, p.N));
  FEDFR_LAUNCH_CHECK("conv3x3_glds");
  return FEDFR_OK;
}
