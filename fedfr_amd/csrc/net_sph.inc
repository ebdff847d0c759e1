// sphnet plan (reference backbones/sphnet.py:4-73 — the backbone run.sh trains): included at the end of net.hip so that it shares the conv
// helpers (conv_fwd / conv_dgrad / conv_wgrad, Ctx, Fork).  No normalisation layers: a unit is conv3x3 (+bias) -> PReLU, a block adds its
// input to two units, the net ends in a Linear on the NCHW-flattened 7x7x512 map.
//   forward : conv -> one streaming pass y = prelu(c + bias) (+ identity), both c (the PReLU backward needs its sign and value) and y kept
//   backward: ONE pass per PReLU (dz = g * prelu'(c + bias), the block's identity add folded in, partial sums for dbias / dalpha on the side),
//             dgrad on the caller's stream, weight gradients + their finalizes on the auxiliary stream (every layer has its own dz buffer:
//             no generation ring, one fork per block, one join at the end)
namespace {
struct SphBuilder {
  Builder& b;
  SphUnit unit(const std::string& conv_name, const std::string& prelu_name, int cin, int cout, int stride, int hin, bool bias) {
    SphUnit u{};
    u.cin_real = cin;
    u.conv.Cin = cin < 64 ? 64 : cin; u.conv.Cout = cout; u.conv.R = 3; u.conv.stride = stride; u.conv.Hin = hin; u.conv.Hout = hin / stride;
    u.w_param_off = b.add_param(conv_name + ".weight", 0, {cout, cin, 3, 3});
    u.conv.w_off = u.w_param_off; u.conv.wd_off = -1;
    u.b_off = bias ? b.add_param(conv_name + ".bias", 2, {cout}) : -1;
    u.a_off = b.add_param(prelu_name + ".weight", 3, {cout});
    return u;
  }
};
}  // namespace

FedfrNet* net_create_sphere(int type, int batch) {
  if ((type != 20 && type != 64) || batch <= 0) {
    fedfr_set_error("net_create_sphere: type must be 20 or 64 and batch > 0 (got %d, %d)", type, batch);
    return nullptr;
  }
  static const int kL20[4] = {1, 2, 4, 1}, kL64[4] = {3, 7, 16, 3};
  const int* L = type == 20 ? kL20 : kL64;
  FedfrNet* n = new FedfrNet();
  for (int i = 0; i < 4; ++i) n->layers[i] = L[i];
  n->sph_type = type;
  n->B = batch; n->Bp = (batch + 7) / 8 * 8; n->HW = 112; n->F = 512;
  Builder b; b.n = n;
  SphBuilder sb{b};
  static const int kF[5] = {3, 64, 128, 256, 512};
  int hin = 112;
  for (int s = 0; s < 4; ++s) {
    SphStageD st{};
    char pfx[64];
    snprintf(pfx, sizeof pfx, "layer%d.", s + 1);
    st.C = kF[s + 1]; st.H = hin / 2;
    st.head = sb.unit(std::string(pfx) + "0", std::string(pfx) + "1", kF[s], kF[s + 1], 2, hin, true);     // nn.Sequential: conv = .0, PReLU = .1
    for (int i = 0; i < L[s]; ++i) {
      char bp[64];
      snprintf(bp, sizeof bp, "layer%d.%d.", s + 1, i + 2);
      SphBlockD k{};
      k.u1 = sb.unit(std::string(bp) + "conv1", std::string(bp) + "prelu1", st.C, st.C, 1, st.H, false);
      k.u2 = sb.unit(std::string(bp) + "conv2", std::string(bp) + "prelu2", st.C, st.C, 1, st.H, false);
      st.blocks.push_back(k);
    }
    n->sph.push_back(st);
    hin = st.H;
  }
  n->final_hw = 7; n->final_C = 512; n->fc_in = 512 * 49;
  n->fc_w_off = b.add_param("fc.weight", 4, {512, n->fc_in});
  n->fc_b_off = b.add_param("fc.bias", 5, {512});
  n->trainable_count = n->param_count = b.poff;
  n->buffer_count = 0; n->nbt_count = 0;
  // ---- shadow: bf16 mirror of the parameters | padded stem weights | dgrad-layout copy of every conv but the stem ----
  long long soff = (n->trainable_count + 7) / 8 * 8;
  n->sph_w0pad_off = soff; soff += 64LL * 9 * 64;
  n->sph[0].head.conv.w_off = n->sph_w0pad_off;
  for (size_t s = 0; s < n->sph.size(); ++s) {
    auto& st = n->sph[s];
    if (s > 0) { st.head.conv.wd_off = soff; soff += (long long)st.head.conv.Cin * 9 * st.head.conv.Cout; }
    for (auto& k : st.blocks) {
      k.u1.conv.wd_off = soff; soff += (long long)st.C * 9 * st.C;
      k.u2.conv.wd_off = soff; soff += (long long)st.C * 9 * st.C;
    }
  }
  n->shadow_count = soff;
  // ---- activation arena (bf16 elements) and workspace ----
  const long long Bq = batch;
  long long aoff = 0;
  auto take = [&](long long elems) { const long long o = aoff; aoff += (elems + 7) / 8 * 8; return o; };
  size_t w = 0;
  auto wtake = [&](size_t bytes) { const size_t o = w; w += align_up(bytes, 256); return o; };
  n->sph_xin_off = take(Bq * 112 * 112 * 64);
  long long prev = n->sph_xin_off, gmax = 0, part = 0, slab = 0;
  auto layout_unit = [&](SphUnit& u, long long in) {
    const long long Mo = Bq * u.conv.Hout * u.conv.Hout;
    u.in_off = in;
    u.c_off = take(Mo * u.conv.Cout);
    u.t_off = take(Mo * u.conv.Cout);
    u.dz_off = wtake((size_t)Mo * u.conv.Cout * 2);
    u.rows_off = wtake((size_t)ew_prelu_bwd_rows((int)Mo, u.conv.Cout) * 2 * u.conv.Cout * 4);
    gmax = std::max(gmax, Mo * u.conv.Cout);     // (the gradient wrt the padded input image is never formed)
    part = std::max(part, (long long)gemm_nt_stat_rows((int)Mo, u.conv.Cout) * 2 * u.conv.Cout);
    const int NJ = 9 * u.conv.Cin;
    slab = std::max(slab, (long long)gemm_tn_max_splits((int)Mo, u.conv.Cout, NJ, u.conv.Cin, u.conv.Hout, u.conv.stride) * u.conv.Cout * NJ);
    return u.t_off;
  };
  for (auto& st : n->sph) {
    prev = layout_unit(st.head, prev);
    for (auto& k : st.blocks) {
      const long long in = prev;
      layout_unit(k.u1, in);
      prev = layout_unit(k.u2, k.u1.t_off);
    }
  }
  n->sph_flat_off = prev;                   // the last unit's activated output, written NCHW-flat
  n->t_off = prev;
  n->act_bf16_count = aoff;
  n->act_float_off_bytes = (long long)align_up((size_t)aoff * 2, 256);
  n->yfc_off = 0; n->feat_save_off = 0;
  n->mask_off_bytes = n->act_float_off_bytes;
  n->act_bytes = n->act_float_off_bytes + 256;
  slab = std::max(slab, (long long)gemm_nt_pick_splits(batch, 512, n->fc_in) * Bq * 512);
  n->g_elems = (size_t)gmax;
  n->part_floats = (size_t)std::max<long long>(part, 1024);
  n->slab_floats = (size_t)slab;
  for (int i = 0; i < 4; ++i) n->sph_ws_g[i] = wtake(n->g_elems * 2);      // gradient ping-pong (0, 1), dgrad outputs dt1 / da (2, 3)
  n->ws_part = wtake(n->part_floats * 4);
  n->ws_part2 = n->ws_part;
  n->ws_slab = wtake(n->slab_floats * 4 * kSlabRegions);
  n->sph_ws_w0g = wtake((size_t)64 * 9 * 64 * 4);
  n->sph_ws_dfe = wtake((size_t)Bq * 512 * 2 + (size_t)512 * n->Bp * 2 + 256);
  n->ws_fc = wtake((size_t)n->Bp * n->fc_in * 4);
  n->ws_small = wtake(4096);
  n->ws_bytes = w;
  return n;
}

namespace {
// fp32 [64][3][3][3] -> bf16 [64][3][3][64] (channels >= 3 zero): the stem conv through the 64-channel-granular kernels
__global__ __launch_bounds__(256) void sph_pad_w0_kernel(const float* __restrict__ w, bf16_t* __restrict__ dst) {
  const int i = blockIdx.x * 256 + threadIdx.x;          // over 64 * 9 * 64
  if (i >= 64 * 9 * 64) return;
  const int ci = i & 63, ct = i >> 6;                    // ct = co * 9 + tap
  dst[i] = ci < 3 ? f2bf(w[ct * 3 + ci]) : (bf16_t)0;
}
// fp32 [64][3][3][64] weight gradient of the padded stem conv -> [64][3][3][3]
__global__ __launch_bounds__(256) void sph_unpad_g0_kernel(const float* __restrict__ g, float* __restrict__ dst) {
  const int i = blockIdx.x * 256 + threadIdx.x;          // over 64 * 9 * 3
  if (i >= 64 * 9 * 3) return;
  dst[i] = g[(i / 3) * 64 + (i % 3)];
}
// fp32 [B][F] -> bf16 [B][F] and its transpose [F][Bp] (columns >= B zero)
__global__ __launch_bounds__(256) void sph_dfeats_kernel(const float* __restrict__ d, bf16_t* __restrict__ dyb, bf16_t* __restrict__ dybt, int B, int F, int Bp) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= F * Bp) return;
  const int f = i / Bp, bcol = i - f * Bp;
  const bf16_t v = bcol < B ? f2bf(d[(size_t)bcol * F + f]) : (bf16_t)0;
  dybt[i] = v;
  if (bcol < B) dyb[(size_t)bcol * F + f] = v;
}
int sph_act(const Ctx& c, const SphUnit& u, const bf16_t* add, bf16_t* y, int nchw_hw) {
  BnApply a{};
  a.x1 = c.actb + u.c_off; a.sc1 = nullptr; a.sh1 = u.b_off >= 0 ? c.params + u.b_off : nullptr; a.alpha = c.params + u.a_off;
  a.x2 = add; a.y = y; a.M = c.n->B * u.conv.Hout * u.conv.Hout; a.C = u.conv.Cout; a.nchw_hw = nchw_hw; a.stats = nullptr;
  return ew_bn_apply(a, c.st);
}
}  // namespace

static int sph_prepare_weights(const FedfrNet* n, const float* params, bf16_t* shadow, int fwd_shadow_too, hipStream_t st) {
  if (fwd_shadow_too) {
    FEDFR_TRY(ew_cast_f32_bf16(params, shadow, (size_t)n->trainable_count, st));
    hipLaunchKernelGGL(sph_pad_w0_kernel, dim3(ceil_div(64 * 9 * 64, 256)), dim3(256), 0, st, params + n->sph[0].head.w_param_off, shadow + n->sph_w0pad_off);
    FEDFR_LAUNCH_CHECK("sph_pad_w0");
  }
  ShadowTable t{};
  auto add = [&](const SphUnit& u) -> int {
    if (t.n == kMaxShadowEntries) { FEDFR_TRY(ew_weight_dgrad_shadow_multi(params, shadow, t, st)); t.n = 0; }
    ShadowEntry& e = t.e[t.n++];
    e.src = (unsigned long long)u.w_param_off; e.dst = (unsigned long long)u.conv.wd_off;
    e.cout64 = (unsigned short)(u.conv.Cout / 64); e.cin64 = (unsigned short)(u.conv.Cin / 64); e.rs = 9;
    return FEDFR_OK;
  };
  for (size_t s = 0; s < n->sph.size(); ++s) {
    if (s > 0) FEDFR_TRY(add(n->sph[s].head));
    for (const auto& k : n->sph[s].blocks) { FEDFR_TRY(add(k.u1)); FEDFR_TRY(add(k.u2)); }
  }
  if (t.n) FEDFR_TRY(ew_weight_dgrad_shadow_multi(params, shadow, t, st));
  return FEDFR_OK;
}

int g_sph_fuse_prelu_bwd = 1;   // option "sph_fuse_prelu_bwd": the backward of the PReLU in front of a block's conv2 rides in that conv's dgrad epilogue (14x14 / 28x28)
int g_sph_fin_multi = 1;    // option "sph_fin_multi": the PReLU parameter sums of a backward pass in one launch
int g_sph_pair_wgrad = 1;   // option "sph_pair_wgrad": a residual block's two weight gradients through conv_wgrad2 (paired kernel)
// conv of a unit with its activation: conv + the streaming pass (the activation as a second output of the conv epilogue was built in round 3 and
// measured 0.06 ms SLOWER per sphere64 step: the epilogue variants exist only on the slower conv instantiations)
static int sph_conv_act(const Ctx& c, const SphUnit& u, const bf16_t* add, bf16_t* y, int nchw_hw) {
  bf16_t* A = c.actb;
  const int M = c.n->B * u.conv.Hout * u.conv.Hout;
  FEDFR_TRY(conv_fwd(c, u.conv, A + u.in_off, A + u.c_off, false));
  return sph_act(c, u, add, y, nchw_hw);
}

static int sph_forward(const FedfrNet* n, const float* x, const float* params, const bf16_t* shadow, unsigned char* act, unsigned char* ws,
                       float* feats, hipStream_t st) {
  Ctx c{n, params, nullptr, shadow, reinterpret_cast<bf16_t*>(act), reinterpret_cast<float*>(act + n->act_float_off_bytes), ws, nullptr, st};
  const int B = n->B;
  bf16_t* A = c.actb;
  FEDFR_TRY(ew_pad_input_nhwc(x, A + n->sph_xin_off, B, 3, 112 * 112, 64, st));
  for (size_t s = 0; s < n->sph.size(); ++s) {
    const auto& stg = n->sph[s];
    const bool head_last = s + 1 == n->sph.size() && stg.blocks.empty();
    FEDFR_TRY(sph_conv_act(c, stg.head, nullptr, A + stg.head.t_off, head_last ? stg.H * stg.H : 0));
    for (size_t i = 0; i < stg.blocks.size(); ++i) {
      const auto& k = stg.blocks[i];
      FEDFR_TRY(sph_conv_act(c, k.u1, nullptr, A + k.u1.t_off, 0));
      const bool last = s + 1 == n->sph.size() && i + 1 == stg.blocks.size();      // leaves NCHW-flat for x.view(B, -1) (sphnet.py:61)
      FEDFR_TRY(sph_conv_act(c, k.u2, A + k.u1.in_off, A + k.u2.t_off, last ? stg.H * stg.H : 0));
    }
  }
  return fc_forward(c, A + n->sph_flat_off, feats);
}

static int sph_backward(const FedfrNet* n, const float* dfeats, const float* params, const bf16_t* shadow, unsigned char* act, unsigned char* ws,
                        float* grads, hipStream_t st, hipStream_t aux, NetSgd* sgd) {
  Ctx c{n, params, nullptr, shadow, reinterpret_cast<bf16_t*>(act), reinterpret_cast<float*>(act + n->act_float_off_bytes), ws, grads, st};
  const int B = n->B, F = n->F;
  bf16_t* A = c.actb;
  Fork fk{n, st, aux};
  const hipStream_t wst = aux ? aux : st;
  fk.order(st, wst);
  if (sgd) sgd->done_from = n->trainable_count;         // nothing is updated inside this pass
  // ---- fc: dW = dy^T x, db = colsum(dy), dx = dy W ----
  bf16_t* dyb = reinterpret_cast<bf16_t*>(ws + n->sph_ws_dfe);
  bf16_t* dybt = dyb + (size_t)B * F;
  hipLaunchKernelGGL(sph_dfeats_kernel, dim3(ceil_div(F * n->Bp, 256)), dim3(256), 0, st, dfeats, dyb, dybt, B, F, n->Bp);
  FEDFR_LAUNCH_CHECK("sph_dfeats");
  FEDFR_TRY(head_colsum_f32(dfeats, B, F, grads + n->fc_b_off, st));
  float* dxfc = reinterpret_cast<float*>(ws + n->ws_fc);
  FEDFR_TRY(fc_backward(c, dyb, dybt, A + n->sph_flat_off, dxfc, st));      // (sphnet keeps the weight gradient on the main stream)
  auto G = [&](int i) { return reinterpret_cast<bf16_t*>(ws + n->sph_ws_g[i]); };
  int cur = 0;
  FEDFR_TRY(ew_nchw_f32_to_nhwc_bf16(dxfc, G(cur), B, 512, 49, st));       // gradient wrt the last activation, NHWC bf16
  // PReLU backward of a unit: dz -> the unit's own buffer (weight-gradient operand), partial rows -> its own rows; finalize on the aux stream
  auto prelu_bwd = [&](const SphUnit& u, const bf16_t* dy, const bf16_t* add, bf16_t* gsum) -> int {
    const int M = B * u.conv.Hout * u.conv.Hout;
    return ew_prelu_bwd_pass(dy, add, A + u.c_off, u.b_off >= 0 ? params + u.b_off : nullptr, params + u.a_off, M, u.conv.Cout, gsum,
                             reinterpret_cast<bf16_t*>(ws + u.dz_off), reinterpret_cast<float*>(ws + u.rows_off), st);
  };
  // the PReLUs' parameter sums: ONE launch for all of them at the end of the pass (every unit keeps its own partial rows): 62 launches of
  // 8.7 us fewer on the weight-gradient stream, which bounds this network's backward pass (round 3)
  PreluFinTable fin{};
  auto fin_flush = [&]() -> int {
    if (fin.n == 0) return FEDFR_OK;
    const int rc = ew_prelu_bwd_finalize_multi(ws, grads, fin, wst);
    fin.n = 0; fin.blocks = 0;
    return rc;
  };
  auto fin_add = [&](const SphUnit& u, int fused_rows = 0) -> int {     // fused_rows > 0: the rows came from a dgrad epilogue ([3][C] each)
    const int M = B * u.conv.Hout * u.conv.Hout;
    FEDFR_REQUIRE((u.conv.Cout & 7) == 0, "sph_backward: channels %% 8");
    if (!g_sph_fin_multi && fused_rows == 0)
      return ew_prelu_bwd_finalize(reinterpret_cast<const float*>(ws + u.rows_off), ew_prelu_bwd_rows(M, u.conv.Cout), u.conv.Cout,
                                   u.b_off >= 0 ? grads + u.b_off : nullptr, grads + u.a_off, wst);
    if (fin.n == kMaxPreluFin) FEDFR_TRY(fin_flush());
    PreluFinEntry& e = fin.e[fin.n++];
    e.rows_off = (unsigned long long)u.rows_off; e.dbias_off = u.b_off >= 0 ? (long long)u.b_off : -1; e.dalpha_off = (long long)u.a_off;
    e.P = fused_rows > 0 ? fused_rows : ew_prelu_bwd_rows(M, u.conv.Cout); e.C = u.conv.Cout; e.blk0 = fin.blocks; e.nv_row = fused_rows > 0 ? 3 : 2;
    fin.blocks += u.conv.Cout / 8;
    if (!g_sph_fin_multi) return fin_flush();
    return FEDFR_OK;
  };
  // dgrad of `cv` whose epilogue also applies the backward of the PReLU(+bias) unit `pu` in FRONT of the conv: output = pu's dz, rows = pu's
  // parameter sums (GemmNT::bmom = 2).  *fused = rows written; 0, and nothing launched, where no kernel with that epilogue and one row per
  // workgroup (14x14, two-tiles 28x28) serves the shape, or the unit's row buffer does not hold its rows
  auto dgrad_prelu = [&](const ConvD& cv, const bf16_t* dy, const SphUnit& pu, int* fused) -> int {
    *fused = 0;
    GemmNT p = conv_dgrad_problem(B, cv.Hin, cv.Cin, cv.Cout, cv.R, cv.stride);
    p.A = dy; p.B = c.shadow + cv.wd_off; p.Cb = reinterpret_cast<bf16_t*>(ws + pu.dz_off);
    conv_set_papply(p, A + pu.c_off, pu.b_off >= 0 ? params + pu.b_off : nullptr, params + pu.a_off, reinterpret_cast<float*>(ws + pu.rows_off));
    const NtPlan pl = gemm_nt_plan(p, 1);
    if (!g_sph_fuse_prelu_bwd || p.N != pu.conv.Cout || (pl.kernel != NtKernel::glds8_papply_w14 && pl.kernel != NtKernel::glds8_papply_w28s) ||
        (size_t)pl.part_rows * 3 > (size_t)ew_prelu_bwd_rows(p.M, pu.conv.Cout) * 2) return FEDFR_OK;
    *fused = pl.part_rows;
    return gemm_nt_launch(p, 1, st);
  };
  WgradPending pend_w;                                  // a paired weight-gradient launch whose slabs the next one sums (wgrad9p.hip, W9PJob)
  auto unit_wgrad = [&](const SphUnit& u) -> int {      // on the weight-gradient stream
    FEDFR_TRY(wgrad_flush(c, &pend_w, wst));            // (uses the slab workspace itself)
    FEDFR_TRY(fin_add(u));
    if (u.cin_real != u.conv.Cin) {                     // the stem: gradient of the padded weights, then its 3 real input channels
      float* g0 = reinterpret_cast<float*>(ws + n->sph_ws_w0g);
      FEDFR_TRY(conv_wgrad_run(wgrad_problem(c, u.conv, A + u.in_off, reinterpret_cast<const bf16_t*>(ws + u.dz_off)), g0, c.slab(), n->slab_floats, wst));
      hipLaunchKernelGGL(sph_unpad_g0_kernel, dim3(ceil_div(64 * 9 * 3, 256)), dim3(256), 0, wst, g0, grads + u.w_param_off);
      FEDFR_LAUNCH_CHECK("sph_unpad_g0");
      return FEDFR_OK;
    }
    ConvD cv = u.conv;
    cv.w_off = u.w_param_off;                           // conv_wgrad writes grads + w_off
    return conv_wgrad(c, cv, A + u.in_off, reinterpret_cast<const bf16_t*>(ws + u.dz_off), wst);
  };
  // `g` = gradient wrt the current activation (G(cur)); `pend` = a dgrad output still to be added to it (folded into the next PReLU pass)
  const bf16_t* pend = nullptr;
  // debug capture (fedfr_net_debug_capture): the gradient every block's u2 PReLU backward and every stage head's PReLU backward differentiates
  // (16-bit NHWC, the pending branch gradient folded in), back to back in backward order; nothing is enqueued while the pointer is null
  size_t dbg_off = 0;
  for (int s = (int)n->sph.size() - 1; s >= 0; --s) {
    const auto& stg = n->sph[s];
    for (int i = (int)stg.blocks.size() - 1; i >= 0; --i) {
      const auto& k = stg.blocks[i];
      // a_out = prelu2(conv2(t1)) + a_in: the block's output gradient g (+ the pending branch gradient of the block after it)
      if (pend) { FEDFR_TRY(prelu_bwd(k.u2, pend, G(cur), G(cur ^ 1))); cur ^= 1; pend = nullptr; }
      else FEDFR_TRY(prelu_bwd(k.u2, G(cur), nullptr, nullptr));
      FEDFR_TRY(dbg_capture(G(cur), (size_t)B * stg.H * stg.H * stg.C, &dbg_off, st));      // the gradient u2's PReLU backward differentiated (pending branch folded in)
      bf16_t* dt1 = G(2);
      int f1 = 0;                                         // rows of u1's parameter sums when conv2's dgrad epilogue applied u1's backward itself
      FEDFR_TRY(dgrad_prelu(k.u2.conv, reinterpret_cast<const bf16_t*>(ws + k.u2.dz_off), k.u1, &f1));
      if (f1 == 0) {
        FEDFR_TRY(conv_dgrad(c, k.u2.conv, reinterpret_cast<const bf16_t*>(ws + k.u2.dz_off), dt1));
        FEDFR_TRY(prelu_bwd(k.u1, dt1, nullptr, nullptr));
      }
      fk.order(st, wst);
      if (g_sph_pair_wgrad || f1 > 0) {                   // the block's two same-shape weight gradients as one paired launch where the kernel serves them
        FEDFR_TRY(fin_add(k.u2));
        FEDFR_TRY(fin_add(k.u1, f1));
        ConvD c2 = k.u2.conv, c1 = k.u1.conv;
        c2.w_off = k.u2.w_param_off; c1.w_off = k.u1.w_param_off;
        FEDFR_TRY(conv_wgrad2(c, c2, A + k.u2.in_off, reinterpret_cast<const bf16_t*>(ws + k.u2.dz_off), c1, A + k.u1.in_off,
                              reinterpret_cast<const bf16_t*>(ws + k.u1.dz_off), wst, &pend_w));
      } else {
        FEDFR_TRY(unit_wgrad(k.u2));
        FEDFR_TRY(unit_wgrad(k.u1));
      }
      bf16_t* da = G(3);
      FEDFR_TRY(conv_dgrad(c, k.u1.conv, reinterpret_cast<const bf16_t*>(ws + k.u1.dz_off), da));
      pend = da;                                          // g_in = g + da: folded into the PReLU pass that consumes it
    }
    // stage head: t = prelu(conv(x) + bias)
    if (pend) { FEDFR_TRY(prelu_bwd(stg.head, pend, G(cur), G(cur ^ 1))); cur ^= 1; pend = nullptr; }
    else FEDFR_TRY(prelu_bwd(stg.head, G(cur), nullptr, nullptr));
    FEDFR_TRY(dbg_capture(G(cur), (size_t)B * stg.H * stg.H * stg.C, &dbg_off, st));
    fk.order(st, wst);
    FEDFR_TRY(unit_wgrad(stg.head));
    if (s > 0) {
      FEDFR_TRY(conv_dgrad(c, stg.head.conv, reinterpret_cast<const bf16_t*>(ws + stg.head.dz_off), G(cur ^ 1)));
      cur ^= 1;
    }
  }
  FEDFR_TRY(wgrad_flush(c, &pend_w, wst));
  FEDFR_TRY(fin_flush());
  fk.order(wst, st);
  if (!fk.ok) {
    fedfr_set_error("sph_backward: HIP event record/wait failed");
    return FEDFR_ERR_HIP;
  }
  return FEDFR_OK;
}
