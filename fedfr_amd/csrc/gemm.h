// Descriptors + launchers for the two MFMA workhorse kernels (bf16 in, fp32 accumulate).
//
//  gemm_nt : C[m][n] = sum_k A(m,k) * B[n][k]      A = plain row-major or conv gather (NHWC)
//            used for conv fwd, conv dgrad (flipped/transposed weight shadow), fc fwd.
//  gemm_tn : C[i][j] = sum_p P[p][i] * Q(p,j)      both operands reduction-major in memory
//            (LDS transpose reads, ds_read_b64_tr_b16); used for conv wgrad, fc dgrad/wgrad.
#pragma once
#include "common.h"

struct GemmNT {
  const bf16_t* A;
  const bf16_t* B;        // [N][K], K contiguous
  int M, N, K;
  int mode;               // 0 plain A[M][lda]; 1 conv gather
  int H, W, C;            // gather source tensor [img][H][W][C]
  int Ho, Wo;             // row m -> (img, ho, wo)
  int S;                  // filter width (tap = r*S + s)
  int stride, pad, up;    // pos = ho*stride + r - pad; up==2: pos must be even, then pos/2
  int lda;
  int cpt;                // 64-wide k-chunks per tap (C/64)
  bf16_t* Cb;             // bf16 out [M][ldc] (or null)
  int ldc;
  float* Cf;              // fp32 split-K slabs [splits][M][N] (or null)
  float* stats;           // [gridM*WM][2][N] per-column partial (sum, sumsq) of the bf16-rounded output
  int ksteps_total, ksteps_per_split;
  int nbn;                // number of N tiles (for the 1-D XCD-swizzled grid)
  unsigned a_bytes, b_bytes;   // buffer-descriptor ranges (filled by the launcher)
  // optional fused BatchNorm-backward reduction on the OUTPUT tile (dgrad launches): with dy = this GEMM's bf16
  // output and x = the BN input [M][N], writes per-M-tile partials [ceil(M/128)][3][N] of (sum dz, sum dz*xhat,
  // sum dy*min(z,0)) exactly like ew_bn_bwd_reduce.  Only some kernels implement it: NtPlan::part_rows (below) is the number of
  // partial rows the chosen one leaves, 0 if it has no such epilogue.
  const bf16_t* bx;
  const float *bmean, *brstd, *bgamma, *bbeta, *balpha;
  float* bpart;
  // bmom != 0 (forward launches, round 3): the same epilogue leaves RAW moments of the output y against a same-shape tensor bx instead —
  // rows [3][N] of (sum y, sum y * bx, sum y * y) — from which the pass that follows derives the statistics of y AND of
  // bn(y) + bx (the next block's bn1) without a pass over that sum (net.hip, conv2 of a residual block).  bmean / brstd: any readable [N] (conv_set_bmom).
  int bmom;               // 2 (dgrad launches, sphnet): a bare PReLU(+bias) precedes the conv — the OUTPUT becomes dz = dy * prelu'(bx + bias) (bias in
                          // bbeta or null, slopes in balpha), rows [3][N] = (sum dz, sum dy z over z <= 0, same): the PReLU's backward pass disappears
  // stride-2 dgrad by output-parity class (gemm.hip: nt_parity_problem): this launch computes the output pixels (2 h2 + par_h, 2 w2 + par_w)
  // of a [img][outH][outW] map with only the filter taps that reach a real (non-inserted-zero) input: 1, 2, 2 or 4 of the 9
  int par_on, par_h, par_w, outH, outW;
  // optional OUTPUT epilogue of the LDS-DMA conv kernels (eval-mode forward, where the BatchNorm that follows a conv is a known
  // per-channel affine): y = acc * esc[n] + esh[n] on the fp32 accumulators, PReLU with ealpha[n] if given, + eadd[m][n] (bf16, the
  // identity path) if given; Cb2 (optional) receives y2 = y * esc2[n] + esh2[n] (the next block's bn1 of this block's output)
  const float *esc, *esh, *ealpha;
  const bf16_t* eadd;
  const float *esc2, *esh2;
  bf16_t* Cb2;
  // ... and, for nets whose activation follows the conv with no normalisation in between (sphnet: t = prelu(conv + bias) (+ identity)):
  // Cb2 = prelu_{e2alpha}(y * esc2 + esh2) + e2add with esc2 / esh2 / e2add optional (1 / 0 / none) — the same fp32 expressions on the
  // same bf16-rounded conv output as the separate ew_bn_apply pass, so both forms give identical bits; Cb keeps the raw conv output
  const float* e2alpha;
  const bf16_t* e2add;
  unsigned long long* dbg;   // diagnostics builds only (tools/stamp_halo2.hip): per-block in-kernel clock stamps
};

struct GemmTN {
  const bf16_t* P;        // [Kp][ldp]  (dy side)
  const bf16_t* Q;        // plain [Kp][ldq] or conv gather source NHWC
  int Kp, NI, NJ;
  int mode;               // 0 plain; 1 conv gather (row p -> (img,ho,wo) of the dy tensor)
  int H, W, C, Ho, Wo, S, stride, pad;
  FastDiv dHoWo, dWo, dHo;
  int ldp, ldq;
  float* out;             // [splits][NI][NJ]
  int ksteps_total, ksteps_per_split;
  int nbj, ntiles;        // number of j tiles / of (i,j) tiles
  int use_tr;             // 1: ds_read_b64_tr_b16 fragments; 0: scalar LDS gathers (validation fallback)
  unsigned p_bytes, q_bytes;   // buffer-descriptor ranges (filled by the launcher)
};

// rows of partial stats the NT kernel writes for a given M (needed to size / finalize)
int gemm_nt_stat_rows(int M, int N);

// Which kernel serves an NT problem and what callers must know before they launch it.  gemm_nt_plan is the ONLY place that decides:
// gemm_nt_launch switches on its answer, and the launchers that know their own row count check it against the plan's.
enum class NtKernel {
  c64p,                                                  // conv_c64p.hip: persistent 64 -> 64 channel kernel (56x56, 112x112)
  glds_w112, glds_w56, glds_w56_c64_n128, glds_w56_c128_n64, glds8_w14, glds8_w28, glds8_w28_stats,      // plain LDS-DMA instantiations
  glds8_fused_w14, glds8_fused_w28, glds8_fused_w28s,    // ... with the BatchNorm-backward / raw-moment reduction epilogue (bpart)
  glds8_papply_w14, glds8_papply_w28, glds8_papply_w28s, // ... with sphnet's PReLU-apply epilogue (bmom == 2)
  ring,                                                  // gemm_nt_glds.hip: LDS-DMA ring GEMM
  nt_128x128, nt_128x64, nt_64x128, nt_64x64,            // the generic gather GEMM
};
struct NtPlan {
  NtKernel kernel;
  int profile_slot;       // slot the chosen launcher records under (gemm.hip)
  int stat_rows;          // rows a statistics buffer / finalize is sized for (gemm_nt_stat_rows)
  int stat_rows_live;     // leading rows of those that carry data when the launch writes statistics (the rest are zero filler)
  int part_rows;          // rows the bpart epilogue writes; 0: the chosen kernel has no such epilogue for the requested mode (bmom)
  bool out_epilogue;      // the chosen kernel implements the output epilogue (esc / eadd / Cb2)
};
// pure host function; a stride-2 3x3 dgrad by output-parity class (option "dgrad_parity") is planned as the per-class problem it is launched as
NtPlan gemm_nt_plan(const GemmNT& p, int splits);

// conv problems from geometry alone; callers set the operand, output and epilogue pointers on the result
inline GemmNT conv_fwd_problem(int batch, int hin, int cin, int cout, int ksize, int stride) {
  const int hout = hin / stride;
  GemmNT p{};
  p.M = batch * hout * hout; p.N = cout; p.K = ksize * ksize * cin;
  p.mode = 1; p.H = hin; p.W = hin; p.C = cin; p.Ho = hout; p.Wo = hout; p.S = ksize;
  p.stride = stride; p.pad = ksize == 3 ? 1 : 0; p.up = 1; p.ldc = cout;
  return p;
}
// dx (at the conv's INPUT resolution) = conv_transpose(dy) with the flipped / transposed weight shadow
inline GemmNT conv_dgrad_problem(int batch, int hin, int cin, int cout, int ksize, int stride) {
  const int hout = hin / stride;
  GemmNT p{};
  p.N = cin; p.K = ksize * ksize * cout; p.ldc = cin;
  if (ksize == 1) {          // 1x1 stride-s: plain GEMM at the OUTPUT resolution (compact result; caller up-samples)
    p.mode = 0; p.M = batch * hout * hout; p.lda = cout;
  } else {
    p.mode = 1; p.M = batch * hin * hin;
    p.H = hout; p.W = hout; p.C = cout; p.Ho = hin; p.Wo = hin; p.S = 3;
    p.stride = 1; p.pad = 1; p.up = stride;
  }
  return p;
}
// The epilogues of a conv problem, attached from raw pointers: the plan (net.hip, net_sph.inc) and the fedfr_conv2d_* entries (api.hip) both
// come through here.  BatchNorm-backward reduction on a dgrad's output (GemmNT::bx ...): rows [3][N] into `part`
inline void conv_set_bnbwd(GemmNT& p, const bf16_t* bn_x, const float* mean, const float* rstd, const float* gamma, const float* beta,
                           const float* alpha, float* part) {
  p.bx = bn_x; p.bmean = mean; p.brstd = rstd; p.bgamma = gamma; p.bbeta = beta; p.balpha = alpha; p.bpart = part;
}
// bmom modes: the kernels read bmean / brstd and never use them, so any readable [N] serves — the slopes where the mode has them, else the
// rows the launch itself writes (at least [3][N])
inline void conv_set_bmom(GemmNT& p, int bmom, const bf16_t* bx, float* part) {
  p.bx = bx; p.bpart = part; p.bmom = bmom;
  p.bmean = p.brstd = p.balpha ? p.balpha : part;
}
inline void conv_set_moments(GemmNT& p, const bf16_t* other, float* part) { conv_set_bmom(p, 1, other, part); }      // raw moments against same-shape `other`
// PReLU-apply dgrad (bmom = 2): the output becomes dz of the PReLU(+bias) unit whose conv output is act_x
inline void conv_set_papply(GemmNT& p, const bf16_t* act_x, const float* bias, const float* alpha, float* part) {
  p.bbeta = bias; p.balpha = alpha; conv_set_bmom(p, 2, act_x, part);
}
// eval-mode output epilogue: y = prelu?(acc * scale + shift) (+ add); y2 (optional) = y * scale2 + shift2
inline void conv_set_out_epilogue(GemmNT& p, const float* scale, const float* shift, const float* alpha, const bf16_t* add, bf16_t* y2,
                                  const float* scale2, const float* shift2) {
  p.esc = scale; p.esh = shift; p.ealpha = alpha; p.eadd = add;
  if (y2) { p.Cb2 = y2; p.esc2 = scale2; p.esh2 = shift2; }
}
extern int g_tn_use_tr;
inline GemmTN conv_wgrad_problem(int batch, int hin, int cin, int cout, int ksize, int stride) {
  const int hout = hin / stride;
  GemmTN p{};
  p.Kp = batch * hout * hout; p.NI = cout; p.NJ = ksize * ksize * cin;
  p.mode = 1; p.H = hin; p.W = hin; p.C = cin; p.Ho = hout; p.Wo = hout; p.S = ksize;
  p.stride = stride; p.pad = ksize == 3 ? 1 : 0;
  p.ldp = cout; p.ldq = 0; p.use_tr = g_tn_use_tr;
  return p;
}
// weight gradient of p (P / Q set) into dst: picks the K-splits; several of them go to `slab` (slab_floats floats, FEDFR_ERR_WORKSPACE if
// they do not fit) and are summed into dst by ew_reduce_slabs
int conv_wgrad_run(GemmTN p, float* dst, float* slab, size_t slab_floats, hipStream_t st);
// number of splits / workspace helpers
int gemm_nt_pick_splits(int M, int N, int K);
int gemm_nt_launch(GemmNT p, int splits, hipStream_t st);
int gemm_tn_launch(GemmTN p, int splits, hipStream_t st);
// the two same-shape 3x3 / stride-1 weight gradients of a residual block on the paired nine-tap kernel (wgrad9p.hip)
bool gemm_tn_w9pair_ok(const GemmTN& a, const GemmTN& b);
int gemm_tn_w9pair_splits(const GemmTN& a);
// The split-K slabs of an EARLIER paired launch, summed by a later paired launch's workgroups beside their own work (round 4: the
// separate reduce_slabs launches cost 13 of the 66 us of a pair).  dst[l] = sum over s of slab[l][s * n + i], in the summation order of the
// stand-alone kernels (ew_reduce_slabs: ascending slabs, or the 8-lane order of its wide form), so both paths give the same bits.
struct W9PJob {
  const float* slab[2];   // [nsplit][n] each
  float* dst[2];
  size_t n;               // floats per layer (0 = no job)
  int nsplit;
};
// can a paired launch of this shape carry `job`? (its loads must fit beside the launch's own sub-images: see wgrad9p.hip)
bool gemm_tn_w9pair_job_ok(const GemmTN& a, int splits, const W9PJob& job);
int gemm_tn_launch_w9pair(GemmTN a, GemmTN b, int splits, hipStream_t st, const W9PJob* job = nullptr);
// Wo > 0: conv weight gradient on a Wo x Wo output map (lets the nine-tap kernel, wgrad9.hip, be chosen)
int gemm_tn_pick_splits(int Kp, int NI, int NJ, int C_or_0, int Wo = 0, int stride = 1);
int gemm_tn_max_splits(int Kp, int NI, int NJ, int C_or_0, int Wo, int stride);
void gemm_tn_tiles(int NI, int NJ, int C_or_0, int* TI, int* TJ);

// optional HIP-event timing of every NT/TN launch (slots: see gemm.hip)
void gemm_profile_enable(int on);
int gemm_profile_read(int slot, double* total_ms, long long* launches, double* flops);
int gemm_profile_read_bytes(int slot, double* bytes);      // algorithmic HBM bytes of the same launches
