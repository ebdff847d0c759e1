// Fused head of the Branch / Sequential model of train_with_public_data (reference client.py:354-441), fp32:
//   loss = CE(margin(cos(f, fc)) * s) + bce_scale * BCE(cos(converter(f), W) ; bias) + mu * contrastive(f, f_global, f_last)
// behind ONE C call (branch_head): losses, d(loss)/d(f), d(loss)/d(fc) and the gradient of every parameter of the personalised branch.
// The GEMMs, the softmax, the row normalisations, the contrastive term and the BottleBlock are head.hip's / bottle.hip's launchers; new here:
//   bce_fused      cos [B][C] -> row_loss, dcos, dbias in one pass: the logits z, the targets gt and dz/dcos never reach memory.  A workgroup
//                  owns BCE_ROWS rows (one wave per row, four rows in flight), keeps the column sums of dz of its rows in registers and writes
//                  them as ONE partial row; a second launch adds the partial rows in ascending order (no floating-point atomics).
//   branch_dfeats  d(loss)/d(f) = normalize_bwd(sum of the split-K slabs of d(f_hat)) + d(BCE branch)/d(f) + mu * d(contrastive)/d(f),
//                  one wave per row, one pass over [B][D]
//   branch_losses  the four scalars from the three per-row loss vectors (one wave, fixed order)
#include "head.h"

namespace {
constexpr int BCE_ROWS = 16;      // rows of one workgroup of bce_fused = rows summed into one partial row of dbias
constexpr int DF_J = 8;           // branch_dfeats keeps a row of up to 64 * DF_J elements in registers

// BCE comment block of head.hip: z = r (g(cos) -/+ m) + bias, g(x) = 2 ((x + 1) / 2)^t - 1; positive (lam / r) log(1 + e^-z + 1e-8), negative
// ((1 - lam) / r) log(1 + e^z + 1e-8); the expressions are bce_logits_kernel's and bce_loss_kernel's, element for element
__global__ __launch_bounds__(256) void bce_fused_kernel(const float* __restrict__ cosv, const long long* __restrict__ label,
                                                        const float* __restrict__ bias, int B, int C, float m, float r, float t, float lam,
                                                        float gscale, float* __restrict__ row_loss, float* __restrict__ dcos,
                                                        float* __restrict__ partial) {
  __shared__ float sh_loss[BCE_ROWS];
  __shared__ float sh_col[4][256];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r0 = blockIdx.x * BCE_ROWS, nr = min(BCE_ROWS, B - r0);
  if (tid < BCE_ROWS) sh_loss[tid] = 0.f;
  __syncthreads();
  for (int c0 = 0; c0 < C; c0 += 256) {
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int i = wave; i < nr; i += 4) {                       // row r0 + i belongs to this wave alone
      const int row = r0 + i;
      const long long y = label[row];
      float ls = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = c0 + lane + 64 * j;
        if (c < C) {
          const size_t o = (size_t)row * C + c;
          const float x = cosv[o];
          const float hb = (x + 1.f) * 0.5f;
          const float pw1 = powf(hb, t - 1.f);
          const float g = 2.f * pw1 * hb - 1.f;
          const bool pos = ((long long)c == y);
          const float zz = r * (pos ? g - m : g + m) + bias[c];
          float le, dl;
          if (pos) {
            const float e = expf(-zz);
            le = (lam / r) * logf(1.f + e + 1e-8f);
            dl = (lam / r) * (-e) / (1.f + e + 1e-8f);
          } else {
            const float e = expf(zz);
            le = ((1.f - lam) / r) * logf(1.f + e + 1e-8f);
            dl = ((1.f - lam) / r) * e / (1.f + e + 1e-8f);
          }
          ls += le;
          const float gz = dl * gscale;
          dcos[o] = gz * (r * t * pw1);
          acc[j] += gz;
        }
      }
      ls = wave_sum(ls);
      if (lane == 0) sh_loss[i] += ls;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) sh_col[wave][lane + 64 * j] = acc[j];
    __syncthreads();
    if (c0 + tid < C) partial[(size_t)blockIdx.x * C + c0 + tid] = ((sh_col[0][tid] + sh_col[1][tid]) + sh_col[2][tid]) + sh_col[3][tid];
    __syncthreads();
  }
  if (tid < nr) row_loss[r0 + tid] = sh_loss[tid];
}

__global__ __launch_bounds__(256) void bce_dbias_kernel(const float* __restrict__ partial, int nblk, int C, float* __restrict__ dbias) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  float s = partial[c];
  for (int k = 1; k < nblk; ++k) s += partial[(size_t)k * C + c];
  dbias[c] = s;
}

// dx = inv * (g - xn <xn, g>) + extra_a + wb * extra_b, g = the sum of the slabs of d(xn), slab 0 first (normalize_rows_bwd_kernel's additions)
template <bool WIDE>
__global__ __launch_bounds__(256) void branch_dfeats_kernel(const float* __restrict__ xn, const float* __restrict__ inv,
                                                            const float* __restrict__ dxn, int nslab, long long slab_stride,
                                                            const float* __restrict__ extra_a, const float* __restrict__ extra_b, float wb,
                                                            float* __restrict__ dx, int R, int D) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= R) return;
  const size_t o = (size_t)row * D;
  auto tail = [&](int i, float v) {
    if (extra_a) v += extra_a[o + i];
    if (extra_b) v += wb * extra_b[o + i];
    dx[o + i] = v;
  };
  if constexpr (WIDE) {
    float gv[DF_J], xv[DF_J];
#pragma unroll
    for (int j = 0; j < DF_J; ++j) {
      const int i = min(lane + 64 * j, D - 1);
      xv[j] = xn[o + i];
      gv[j] = dxn[o + i];
    }
    for (int k = 1; k < nslab; ++k) {
      float tv[DF_J];
#pragma unroll
      for (int j = 0; j < DF_J; ++j) tv[j] = dxn[(size_t)k * slab_stride + o + min(lane + 64 * j, D - 1)];
#pragma unroll
      for (int j = 0; j < DF_J; ++j) gv[j] += tv[j];
    }
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < DF_J; ++j)
      if (lane + 64 * j < D) s += xv[j] * gv[j];
    s = wave_sum(s);
    const float iv = inv[row];
#pragma unroll
    for (int j = 0; j < DF_J; ++j) {
      const int i = lane + 64 * j;
      if (i < D) tail(i, iv * (gv[j] - xv[j] * s));
    }
  } else {
    auto g = [&](int i) {
      float v = dxn[o + i];
      for (int k = 1; k < nslab; ++k) v += dxn[(size_t)k * slab_stride + o + i];
      return v;
    };
    float s = 0.f;
    for (int i = lane; i < D; i += 64) s += xn[o + i] * g(i);
    s = wave_sum(s);
    const float iv = inv[row];
    for (int i = lane; i < D; i += 64) tail(i, iv * (g(i) - xn[o + i] * s));
  }
}

// out[0..3] = total, cos, contrastive, bce: means of the per-row losses, total = (cos + bce_scale * bce) + mu * contrastive; an absent term is 0
__global__ __launch_bounds__(64) void branch_losses_kernel(const float* __restrict__ nll, const float* __restrict__ bce_rows,
                                                           const float* __restrict__ con_rows, int B, float bce_scale, float mu,
                                                           float* __restrict__ out) {
  const int lane = threadIdx.x;
  float a = 0.f, b = 0.f, c = 0.f;
  for (int i = lane; i < B; i += 64) {
    a += nll[i];
    if (bce_rows) b += bce_rows[i];
    if (con_rows) c += con_rows[i];
  }
  a = wave_sum(a); b = wave_sum(b); c = wave_sum(c);
  if (lane != 0) return;
  const float ib = 1.f / (float)B;
  const float cosl = a * ib, bcel = b * ib, conl = c * ib;
  float total = cosl;
  if (bce_rows) total += bce_scale * bcel;
  if (con_rows) total += mu * conl;
  out[0] = total; out[1] = cosl; out[2] = conl; out[3] = bcel;
}

int split_for(int k) {            // FusedTrainer's rule (client.py _split_for): k ranges of about 128, at most 8, no empty chunk
  const int s = k / 128 < 1 ? 1 : (k / 128 > 8 ? 8 : k / 128);
  const int chunk = ceil_div(ceil_div(k, s), 32) * 32;
  return ceil_div(k, chunk);
}

// ops.sgemm's own rule (_auto_splits) for a long reduction over few output tiles, which is what FusedTrainer's plain path gets for d(f_hat) =
// d(cos) [B][C] @ fc_hat [C][D] at C > 4096 (16 workgroups walking 6100 k alone are a 0.3 ms latency chain): slabs of >= 256 k, ~512 workgroups
int auto_splits(int M, int N, int K) {
  const int tiles = ceil_div(M, 64) * ceil_div(N, 64);
  if (tiles >= 128 || K < 1024) return 1;
  int s = K / 256 < 64 ? K / 256 : 64;
  if (ceil_div(512, tiles) < s) s = ceil_div(512, tiles);
  if (s < 1) s = 1;
  const int chunk = ceil_div(ceil_div(K, s), 32) * 32;
  return ceil_div(K, chunk);
}

// workspace carving: every buffer starts on a 256-byte boundary
struct Carve {
  size_t off = 0;
  char* base;
  explicit Carve(void* b) : base(static_cast<char*>(b)) {}
  float* take(size_t nfloat) {
    float* p = base ? reinterpret_cast<float*>(base + off) : nullptr;
    off += align_up(nfloat * sizeof(float), 256);
    return p;
  }
};

struct Ws {
  float *xn, *xinv, *wn, *winv, *cos, *dxn, *dwn, *prob_t, *nll, *row_max, *row_sum, *dmul, *z_t;
  float *y, *h1, *h2, *yn, *yinv, *bwn, *bwinv, *bcos, *bdcos, *brow, *partial, *dyn, *dbwn, *dy, *dxb, *bottle_ws;
  float *crow, *dcon;
  int ks, kd;
  bool split, three;
  size_t bottle_bytes, total;
};

Ws layout(void* base, int B, int D, int C, int n_class, int conv, int detach, int contrastive) {
  Ws w{};
  Carve c(base);
  const size_t BD = (size_t)B * D;
  w.split = C >= 256 && C <= 4096 && D >= 256;
  w.three = C > 16384;                                         // rows too long for softmax_ce_fused: the three-kernel form
  w.ks = w.split ? split_for(D) : 1;
  w.kd = w.split ? split_for(C) : auto_splits(B, D, C);
  w.xn = c.take(BD); w.xinv = c.take(B);
  w.wn = c.take((size_t)C * D); w.winv = c.take(C);
  w.cos = c.take((size_t)w.ks * B * C);
  w.dxn = c.take((size_t)w.kd * BD);
  w.dwn = c.take((size_t)C * D);
  w.prob_t = c.take(B); w.nll = c.take(B);
  if (w.three) { w.row_max = c.take(B); w.row_sum = c.take(B); w.dmul = c.take(B); w.z_t = c.take(B); }
  if (conv) {
    w.y = c.take(BD);
    if (conv == 2) { w.h1 = c.take(BD); w.h2 = c.take(BD); }
    w.yn = c.take(BD); w.yinv = c.take(B);
    w.bwn = c.take((size_t)n_class * D); w.bwinv = c.take(n_class);
    w.bcos = c.take((size_t)B * n_class); w.bdcos = c.take((size_t)B * n_class);
    w.brow = c.take(B);
    w.partial = c.take((size_t)ceil_div(B, BCE_ROWS) * n_class);
    w.dyn = c.take(BD); w.dbwn = c.take((size_t)n_class * D); w.dy = c.take(BD);
    if (!detach) w.dxb = c.take(BD);
    if (conv == 2) {
      w.bottle_bytes = bottle_workspace_bytes(B, D);
      w.bottle_ws = c.take(w.bottle_bytes / sizeof(float));
    }
  }
  if (contrastive) { w.crow = c.take(B); w.dcon = c.take(BD); }
  w.total = c.off;
  return w;
}

int check_dims(const char* what, int B, int D, int C, int n_class, int conv) {
  FEDFR_REQUIRE(B >= 1 && D >= 1 && C >= 1, "%s: B = %d, D = %d, C = %d unsupported (all >= 1)", what, B, D, C);
  FEDFR_REQUIRE(conv >= 0 && conv <= 2, "%s: converter kind %d (0 = no BCE branch, 1 = Linear, 2 = BottleBlock)", what, conv);
  if (conv) FEDFR_REQUIRE(n_class >= 1, "%s: n_class = %d unsupported (>= 1)", what, n_class);
  if (conv == 2)
    FEDFR_REQUIRE(D >= 64 && D <= 512 && D % 64 == 0, "%s: D = %d unsupported by the BottleBlock converter (a multiple of 64 in [64, 512])", what, D);
  FEDFR_REQUIRE((long long)B * C < (1ll << 31) && (long long)C * D < (1ll << 31) && (long long)B * D < (1ll << 31),
                "%s: B = %d, D = %d, C = %d: a matrix of 2^31 elements or more", what, B, D, C);
  return FEDFR_OK;
}
}  // namespace

size_t branch_bce_workspace_bytes(int B, int C) {
  if (B < 1 || C < 1) return 0;
  return align_up((size_t)ceil_div(B, BCE_ROWS) * C * sizeof(float), 256);
}

int branch_bce_fused(const float* cosv, const long long* label, const float* bias, int B, int C, float m, float r, float t, float lam,
                     float loss_scale, float* row_loss, float* dcos, float* dbias, void* ws, size_t ws_bytes, hipStream_t st) {
  FEDFR_REQUIRE(B >= 1 && C >= 1, "bce_fused: B = %d, C = %d unsupported (both >= 1)", B, C);
  FEDFR_REQUIRE(cosv && label && bias && row_loss && dcos && dbias && ws, "bce_fused: null pointer");
  FEDFR_REQUIRE(cosv != dcos, "bce_fused: dcos must not be the cosine matrix");
  if (ws_bytes < branch_bce_workspace_bytes(B, C)) {
    fedfr_set_error("bce_fused: workspace of %zu bytes, %zu needed", ws_bytes, branch_bce_workspace_bytes(B, C));
    return FEDFR_ERR_WORKSPACE;
  }
  const int nblk = ceil_div(B, BCE_ROWS);
  float* partial = static_cast<float*>(ws);
  hipLaunchKernelGGL(bce_fused_kernel, dim3(nblk), dim3(256), 0, st, cosv, label, bias, B, C, m, r, t, lam, loss_scale / (float)B, row_loss, dcos,
                     partial);
  FEDFR_LAUNCH_CHECK("bce_fused");
  hipLaunchKernelGGL(bce_dbias_kernel, dim3(ceil_div(C, 256)), dim3(256), 0, st, partial, nblk, C, dbias);
  FEDFR_LAUNCH_CHECK("bce_dbias");
  return FEDFR_OK;
}

int branch_dfeats(const float* xn, const float* inv, const float* dxn, int nslab, long long slab_stride, const float* dbce, const float* dcon,
                  float mu, float* dfeats, int B, int D, hipStream_t st) {
  FEDFR_REQUIRE(B >= 1 && D >= 1 && nslab >= 1 && (nslab == 1 || slab_stride >= (long long)B * D), "branch_dfeats: bad shape");
  FEDFR_REQUIRE(xn && inv && dxn && dfeats, "branch_dfeats: null pointer");
  if (D <= 64 * DF_J)
    hipLaunchKernelGGL(branch_dfeats_kernel<true>, dim3(ceil_div(B, 4)), dim3(256), 0, st, xn, inv, dxn, nslab, slab_stride, dbce, dcon, mu, dfeats, B, D);
  else
    hipLaunchKernelGGL(branch_dfeats_kernel<false>, dim3(ceil_div(B, 4)), dim3(256), 0, st, xn, inv, dxn, nslab, slab_stride, dbce, dcon, mu, dfeats, B, D);
  FEDFR_LAUNCH_CHECK("branch_dfeats");
  return FEDFR_OK;
}

size_t branch_workspace_bytes(int B, int D, int C, int n_class, int conv, int detach, int contrastive) {
  if (B < 1 || D < 1 || C < 1 || conv < 0 || conv > 2 || (conv && n_class < 1) || (conv == 2 && (D < 64 || D > 512 || D % 64))) return 0;
  if ((long long)B * C >= (1ll << 31) || (long long)C * D >= (1ll << 31) || (long long)B * D >= (1ll << 31)) return 0;
  return layout(nullptr, B, D, C, n_class, conv, detach, contrastive).total;
}

int branch_head(const float* feats, const long long* labels, int B, int D, const float* fc, int C, int arc, float s, float m, int conv,
                const float* const* conv_params, const float* bce_w, const float* bce_b, int n_class, float bce_m, float bce_r, float bce_t,
                float bce_lam, float bce_scale, const float* gfeats, const float* lfeats, float temperature, float mu, int detach, float* losses,
                float* dfeats, float* dfc, float* const* conv_grads, float* dbce_w, float* dbce_b, void* ws, size_t ws_bytes, hipStream_t st) {
  // ---- every check before the first launch
  FEDFR_TRY(check_dims("branch_head", B, D, C, n_class, conv));
  FEDFR_REQUIRE(feats && labels && fc && losses && dfeats && dfc && ws, "branch_head: null pointer (features, labels, class weights or an output)");
  FEDFR_REQUIRE((gfeats == nullptr) == (lfeats == nullptr), "branch_head: global_feats and last_feats come together");
  const int con = gfeats != nullptr;
  if (con) FEDFR_REQUIRE(temperature > 0.f, "branch_head: temperature must be positive");
  const int nconv = conv == 1 ? 2 : 18;
  if (conv) {
    FEDFR_REQUIRE(conv_params && conv_grads && bce_w && bce_b && dbce_w && dbce_b, "branch_head: null pointer in the BCE branch");
    for (int i = 0; i < nconv; ++i) FEDFR_REQUIRE(conv_params[i] && conv_grads[i], "branch_head: converter params[%d] or grads[%d] is null", i, i);
  }
  const size_t need = branch_workspace_bytes(B, D, C, n_class, conv, detach, con);
  if (ws_bytes < need) {
    fedfr_set_error("branch_head: workspace of %zu bytes, %zu needed", ws_bytes, need);
    return FEDFR_ERR_WORKSPACE;
  }
  const Ws w = layout(ws, B, D, C, n_class, conv, detach, con);
  const long long BD = (long long)B * D, BC = (long long)B * C;
  const float inv_b = 1.f / (float)B;

  // ---- identity branch: cos = f_hat fc_hat^T -> margin, softmax, d/dcos in place -> d(f_hat) (slabs), d(fc)
  FEDFR_TRY(head_normalize_rows(feats, w.xn, w.xinv, B, D, 1e-12f, st));
  FEDFR_TRY(head_normalize_rows(fc, w.wn, w.winv, C, D, 1e-12f, st));
  if (w.split) {
    FEDFR_TRY(head_sgemm_splitk(w.xn, w.wn, w.cos, B, C, D, D, 1, 1, D, C, 1.f, w.ks, BC, st));
    FEDFR_TRY(head_softmax_ce_fused(w.cos, labels, B, C, C, s, m, arc, inv_b, w.prob_t, w.ks, BC, w.nll, st));
    FEDFR_TRY(head_sgemm_splitk(w.cos, w.wn, w.dxn, B, D, C, C, 1, D, 1, D, 1.f, w.kd, BD, st));
  } else {
    FEDFR_TRY(head_sgemm(w.xn, w.wn, w.cos, B, C, D, D, 1, 1, D, C, 1.f, 0.f, nullptr, st));
    if (w.three) {
      FEDFR_TRY(head_margin_rowmax(w.cos, labels, B, C, C, s, m, arc, w.row_max, w.dmul, w.z_t, st));
      FEDFR_TRY(head_exp_rowsum(w.cos, B, C, C, w.row_max, w.row_sum, st));
      FEDFR_TRY(head_softmax_grad(w.cos, labels, B, C, C, w.row_sum, w.dmul, s, inv_b, w.prob_t, w.row_max, w.z_t, w.nll, st));
    } else {
      FEDFR_TRY(head_softmax_ce_fused(w.cos, labels, B, C, C, s, m, arc, inv_b, w.prob_t, 1, 0, w.nll, st));
    }
    if (w.kd > 1)
      FEDFR_TRY(head_sgemm_splitk(w.cos, w.wn, w.dxn, B, D, C, C, 1, D, 1, D, 1.f, w.kd, BD, st));
    else
      FEDFR_TRY(head_sgemm(w.cos, w.wn, w.dxn, B, D, C, C, 1, D, 1, D, 1.f, 0.f, nullptr, st));
  }

  // ---- personalised branch: y = converter(f), cos = y_hat W_hat^T, fused BCE, back through the normalisations and the converter
  if (conv) {
    if (conv == 1)
      FEDFR_TRY(head_sgemm(feats, conv_params[0], w.y, B, D, D, D, 1, 1, D, D, 1.f, 0.f, conv_params[1], st));
    else
      FEDFR_TRY(bottle_forward(feats, conv_params, B, D, w.h1, w.h2, w.y, st));
    FEDFR_TRY(head_normalize_rows(w.y, w.yn, w.yinv, B, D, 1e-12f, st));
    FEDFR_TRY(head_normalize_rows(bce_w, w.bwn, w.bwinv, n_class, D, 1e-12f, st));
    FEDFR_TRY(head_sgemm(w.yn, w.bwn, w.bcos, B, n_class, D, D, 1, 1, D, n_class, 1.f, 0.f, nullptr, st));
    FEDFR_TRY(branch_bce_fused(w.bcos, labels, bce_b, B, n_class, bce_m, bce_r, bce_t, bce_lam, bce_scale, w.brow, w.bdcos, dbce_b, w.partial,
                               branch_bce_workspace_bytes(B, n_class), st));
    FEDFR_TRY(head_sgemm(w.bdcos, w.bwn, w.dyn, B, D, n_class, n_class, 1, D, 1, D, 1.f, 0.f, nullptr, st));
    FEDFR_TRY(head_normalize_rows_bwd(w.yn, w.yinv, w.dyn, w.dy, B, D, 0.f, st));
    if (conv == 1) {
      if (!detach) FEDFR_TRY(head_sgemm(w.dy, conv_params[0], w.dxb, B, D, D, D, 1, D, 1, D, 1.f, 0.f, nullptr, st));
    } else {
      FEDFR_TRY(bottle_backward(feats, conv_params, w.h1, w.h2, w.dy, B, D, detach ? nullptr : w.dxb, conv_grads, w.bottle_ws, w.bottle_bytes, st));
    }
  }
  if (con) FEDFR_TRY(head_contrastive(feats, gfeats, lfeats, B, D, temperature, w.crow, w.dcon, st));

  // ---- what the backbone waits for
  FEDFR_TRY(branch_dfeats(w.xn, w.xinv, w.dxn, w.kd, BD, conv && !detach ? w.dxb : nullptr, con ? w.dcon : nullptr, mu, dfeats, B, D, st));

  // ---- what it does not: the loss values and the gradients of the head's own parameters
  hipLaunchKernelGGL(branch_losses_kernel, dim3(1), dim3(64), 0, st, w.nll, conv ? w.brow : nullptr, con ? w.crow : nullptr, B, bce_scale, mu, losses);
  FEDFR_LAUNCH_CHECK("branch_losses");
  FEDFR_TRY(head_sgemm(w.cos, w.xn, w.dwn, C, D, B, 1, C, D, 1, D, 1.f, 0.f, nullptr, st));
  FEDFR_TRY(head_normalize_rows_bwd(w.wn, w.winv, w.dwn, dfc, C, D, 0.f, st));
  if (conv) {
    FEDFR_TRY(head_sgemm(w.bdcos, w.yn, w.dbwn, n_class, D, B, 1, n_class, D, 1, D, 1.f, 0.f, nullptr, st));
    FEDFR_TRY(head_normalize_rows_bwd(w.bwn, w.bwinv, w.dbwn, dbce_w, n_class, D, 0.f, st));
    if (conv == 1) {
      FEDFR_TRY(head_sgemm(w.dy, feats, conv_grads[0], D, D, B, 1, D, D, 1, D, 1.f, 0.f, nullptr, st));
      FEDFR_TRY(head_colsum_f32(w.dy, B, D, conv_grads[1], st));
    }
  }
  return FEDFR_OK;
}
