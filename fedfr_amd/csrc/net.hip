// iresnet plan + forward/backward sequencing (host code only; see net.h).
// Reference behaviour: backbones/iresnet.py:46-57 (IBasicBlock.forward), :158-172 (IResNet.forward);
// backward is the hand-derived adjoint of that graph (checked against autograd of the CPU oracle).
#include "net.h"
#include "optim.h"
#include <algorithm>
#include <cstdio>
#include "ew.h"
#include "gemm.h"
#include "head.h"

static const int kPlanes[4] = {64, 128, 256, 512};
static const float kBnEps = 1e-5f, kBnMomentum = 0.1f;
int g_tn_use_tr = 1;   // option "tn_use_tr": 0 selects the scalar-LDS fallback fragments (validation)

namespace {
struct Builder {
  FedfrNet* n;
  long long poff = 0, boff = 0, nbt = 0, saveoff = 0;
  std::vector<NetTensor> frozen;
  long long add_param(const std::string& name, int kind, std::initializer_list<int> shape) {
    NetTensor t;
    t.name = name; t.kind = kind; t.region = 0; t.offset = poff; t.ndim = (int)shape.size();
    long long numel = 1; int i = 0;
    for (int s : shape) { t.shape[i++] = s; numel *= s; }
    for (; i < 4; ++i) t.shape[i] = 0;
    n->tensors.push_back(t);
    const long long o = poff;
    poff += (numel + 3) / 4 * 4;
    return o;
  }
  BnD add_bn(const std::string& p, int C, bool frozen_weight = false) {
    BnD b;
    b.C = C;
    if (frozen_weight) {
      // features.weight: requires_grad False (iresnet.py:99-100) -> lives after the trainable region
      NetTensor t; t.name = p + ".weight"; t.kind = 1; t.region = 0; t.offset = -1; t.ndim = 1;
      t.shape[0] = C; t.shape[1] = t.shape[2] = t.shape[3] = 0;
      n->tensors.push_back(t);
      b.g_off = -1;
    } else {
      b.g_off = add_param(p + ".weight", 1, {C});
    }
    b.b_off = add_param(p + ".bias", 2, {C});
    NetTensor t; t.ndim = 1; t.shape[0] = C; t.shape[1] = t.shape[2] = t.shape[3] = 0; t.region = 1;
    t.name = p + ".running_mean"; t.kind = 6; t.offset = boff; b.rm_off = boff; boff += C; n->tensors.push_back(t);
    t.name = p + ".running_var"; t.kind = 7; t.offset = boff; b.rv_off = boff; boff += C; n->tensors.push_back(t);
    t.name = p + ".num_batches_tracked"; t.kind = 8; t.region = 2; t.offset = nbt++; t.ndim = 0; t.shape[0] = 0; n->tensors.push_back(t);
    b.save_off = saveoff;
    saveoff += 4 * (long long)C;
    return b;
  }
  ConvD add_conv(const std::string& name, int Cin, int Cout, int R, int stride, int Hin) {
    ConvD c;
    c.Cin = Cin; c.Cout = Cout; c.R = R; c.stride = stride; c.Hin = Hin; c.Hout = Hin / stride;
    c.w_off = add_param(name + ".weight", 0, {Cout, Cin, R, R});
    c.wd_off = -1;
    return c;
  }
  // p: "layerL.i." inside a network, "" for a lone block (reference IBasicBlock attribute order, iresnet.py:37-43)
  BlockD add_block(const std::string& p, int cin, int cout, int stride, int Hin, bool ds) {
    BlockD k;
    k.Cin = cin; k.Cout = cout; k.stride = stride; k.Hin = Hin; k.Hout = Hin / stride; k.has_ds = ds;
    k.bn1 = add_bn(p + "bn1", k.Cin);
    k.conv1 = add_conv(p + "conv1", k.Cin, k.Cout, 3, 1, k.Hin);
    k.bn2 = add_bn(p + "bn2", k.Cout);
    k.alpha_off = add_param(p + "prelu.weight", 3, {k.Cout});
    k.conv2 = add_conv(p + "conv2", k.Cout, k.Cout, 3, k.stride, k.Hin);
    k.bn3 = add_bn(p + "bn3", k.Cout);
    if (k.has_ds) {
      k.ds = add_conv(p + "downsample.0", k.Cin, k.Cout, 1, k.stride, k.Hin);
      k.bnds = add_bn(p + "downsample.1", k.Cout);
    }
    return k;
  }
};
}  // namespace

// shadow offsets, activation arena and workspace layout of a plan whose tensor list and block list are complete
static void plan_layout(FedfrNet* n, Builder& b, int in_hw) {
  const int batch = n->B, num_features = n->F;
  n->trainable_count = b.poff;
  for (auto& t : n->tensors)
    if (t.region == 0 && t.offset < 0) { t.offset = b.poff; n->feat_bn.g_off = b.poff; b.poff += (t.shape[0] + 3) / 4 * 4; }
  n->param_count = b.poff;
  n->buffer_count = b.boff;
  n->nbt_count = b.nbt;
  // ---- shadow: bf16 mirror of the trainable region, then dgrad-layout copies of every block conv ----
  long long soff = (n->trainable_count + 7) / 8 * 8;
  for (auto& k : n->blocks) {
    k.conv1.wd_off = soff; soff += (long long)k.conv1.Cin * 9 * k.conv1.Cout;
    k.conv2.wd_off = soff; soff += (long long)k.conv2.Cin * 9 * k.conv2.Cout;
    if (k.has_ds) { k.ds.wd_off = soff; soff += (long long)k.ds.Cin * k.ds.Cout; }
  }
  n->shadow_count = soff;
  // ---- activation arena (bf16 elements) ----
  const long long Bq = batch;
  long long aoff = 0;
  auto take = [&](long long elems) { const long long o = aoff; aoff += (elems + 7) / 8 * 8; return o; };
  const long long M0 = Bq * in_hw * in_hw;
  long long prev, gmax;
  if (n->block_only) {                      // a lone IBasicBlock: its input tensor and the gradient wrt it live in the arena too
    const BlockD& k0 = n->blocks.front();
    prev = take(M0 * k0.Cin);
    n->dx_off = take(M0 * k0.Cin);
    n->c0_off = n->a0_off = -1;
    gmax = M0 * k0.Cin;
  } else {
    n->c0_off = take(M0 * 64);
    n->a0_off = take(M0 * 64);
    prev = n->a0_off;
    gmax = M0 * 64;
  }
  for (auto& k : n->blocks) {
    const long long Mi = Bq * k.Hin * k.Hin, Mo = Bq * k.Hout * k.Hout;
    k.x_off = prev;
    k.a1_off = take(Mi * k.Cin);
    k.c1_off = take(Mi * k.Cout);
    k.a2_off = take(Mi * k.Cout);
    k.c2_off = take(Mo * k.Cout);
    k.d_off = k.has_ds ? take(Mo * k.Cout) : -1;
    k.out_off = take(Mo * k.Cout);
    prev = k.out_off;
    gmax = std::max(gmax, std::max(Mi * k.Cin, Mi * k.Cout));
  }
  n->t_off = take(Bq * n->fc_in);
  n->act_bf16_count = aoff;
  n->act_float_off_bytes = (long long)align_up((size_t)aoff * 2, 256);
  long long foff = b.saveoff;                 // bnsave floats first
  n->yfc_off = foff; foff += Bq * num_features;
  n->feat_save_off = foff; foff += 2 * (long long)num_features;
  n->mask_off_bytes = n->act_float_off_bytes + (long long)align_up((size_t)foff * 4, 256);
  n->act_bytes = n->mask_off_bytes + (long long)align_up((size_t)Bq * n->fc_in, 256);
  // ---- workspace ----
  n->g_elems = (size_t)gmax;
  long long part = (long long)ew_stem_stat_rows(batch, in_hw, in_hw) * 128;
  long long slab = (long long)ew_stem_wgrad_blocks(batch, in_hw, in_hw) * 2048;
  auto upd_part = [&](long long M, int C) {
    part = std::max(part, (long long)ew_bn_apply_grid((int)M, C) * 2 * C);
    part = std::max(part, (long long)ew_bn_bwd_grid((int)M, C) * 3 * C);
    part = std::max(part, (long long)ew_bn_bwd_apply_grid((int)M, C) * 3 * C);
  };
  auto upd_conv = [&](const ConvD& c) {
    const long long Mo = Bq * c.Hout * c.Hout;
    part = std::max(part, (long long)gemm_nt_stat_rows((int)Mo, c.Cout) * 2 * c.Cout);
    const int NJ = c.R * c.R * c.Cin;
    slab = std::max(slab, (long long)gemm_tn_max_splits((int)Mo, c.Cout, NJ, c.Cin, c.Hout, c.stride) * c.Cout * NJ);
  };
  upd_part(M0, 64);
  int H = in_hw;
  for (auto& k : n->blocks) {
    const long long Mi = Bq * k.Hin * k.Hin, Mo = Bq * k.Hout * k.Hout;
    upd_part(Mi, k.Cin); upd_part(Mi, k.Cout); upd_part(Mo, k.Cout);
    upd_conv(k.conv1); upd_conv(k.conv2);
    if (k.has_ds) upd_conv(k.ds);
    H = k.Hout;
  }
  upd_part(Bq * H * H, 512);
  if (n->fc_in > 0)
    slab = std::max(slab, (long long)gemm_nt_pick_splits(batch, num_features, n->fc_in) * Bq * num_features);
  n->part_floats = (size_t)part;
  n->slab_floats = (size_t)slab;
  size_t w = 0;
  auto wtake = [&](size_t bytes) { const size_t o = w; w += align_up(bytes, 256); return o; };
  for (int i = 0; i < 2; ++i) n->ws_g[i] = wtake(n->g_elems * 2);
  for (int i = 0; i < 6; ++i) n->ws_t[i] = wtake(n->g_elems * 2);
  for (int i = 0; i < 3 * (kWgradDepth - 1); ++i) n->ws_t2[i] = wtake(n->g_elems * 2);
  n->ws_part = wtake(n->part_floats * 4);
  n->ws_part2 = wtake((size_t)kSlicedRowsMax * 3 * 1024 * 4);   // rows written by the channel-sliced BatchNorm passes (bn_sliced.hip)
  n->ws_slab = wtake(n->slab_floats * 4 * kSlabRegions);      // four regions: paired weight-gradient GEMMs write their two slab sets side by side, and the NEXT pair
                                                   // writes the other two while it sums this pair's (wgrad9p.hip, W9PJob)
  // small: coef[3*512] | finalize tmp [64*2*512] | dyfc f32 [B*F] | dyb bf16 [B*F] | dybt bf16 [F*Bp]
  n->ws_small = wtake((size_t)(3 * 512 + 64 * 2 * 512) * 4 + (size_t)Bq * num_features * 4 + (size_t)Bq * num_features * 2 +
                      (size_t)num_features * n->Bp * 2 + 1024);
  n->ws_fc = wtake((size_t)n->Bp * n->fc_in * 4);
  n->ws_stem = wtake((size_t)ew_stem_wgrad_blocks(batch, in_hw, in_hw) * 2048 * 4);     // the stem weight gradient's own partials: it runs on the main stream
                                                                                        // while the weight-gradient stream is still in the slab regions
  n->ws_bytes = w;
}

FedfrNet* net_create(const int layers[4], int batch, int in_hw, int num_features) {
  if (batch <= 0 || in_hw <= 0 || (in_hw % 16) != 0 || num_features <= 0 || (num_features % 64) != 0) {
    fedfr_set_error("net_create: need batch>0, in_hw%%16==0, num_features%%64==0 (got %d, %d, %d)", batch, in_hw, num_features);
    return nullptr;
  }
  for (int i = 0; i < 4; ++i)
    if (layers[i] <= 0) { fedfr_set_error("net_create: layers[%d]=%d", i, layers[i]); return nullptr; }
  FedfrNet* n = new FedfrNet();
  for (int i = 0; i < 4; ++i) n->layers[i] = layers[i];
  n->B = batch; n->Bp = (batch + 7) / 8 * 8; n->HW = in_hw; n->F = num_features;
  Builder b; b.n = n;
  // ---- tensors in reference state_dict order (iresnet.py:76-98, :37-43) ----
  n->stem = b.add_conv("conv1", 3, 64, 3, 1, in_hw);
  n->stem_bn = b.add_bn("bn1", 64);
  n->stem_alpha_off = b.add_param("prelu.weight", 3, {64});
  int inpl = 64, H = in_hw;
  for (int s = 0; s < 4; ++s) {
    for (int i = 0; i < layers[s]; ++i) {
      char pfx[64];
      snprintf(pfx, sizeof pfx, "layer%d.%d.", s + 1, i);
      BlockD k = b.add_block(pfx, (i == 0) ? inpl : kPlanes[s], kPlanes[s], (i == 0) ? 2 : 1, H, i == 0);
      n->blocks.push_back(k);
      H = k.Hout;
    }
    inpl = kPlanes[s];
  }
  n->bn2 = b.add_bn("bn2", 512);
  n->final_hw = H; n->final_C = 512; n->fc_in = 512 * H * H;
  n->fc_w_off = b.add_param("fc.weight", 4, {num_features, n->fc_in});
  n->fc_b_off = b.add_param("fc.bias", 5, {num_features});
  n->feat_bn = b.add_bn("features", num_features, /*frozen_weight=*/true);
  plan_layout(n, b, in_hw);
  return n;
}

// A lone IBasicBlock (reference backbones/iresnet.py:28-57) as a plan of its own: same block code as inside a network (net_forward /
// net_backward run their block loop over this one block and skip stem and tail), tensors in the reference block's state_dict order.
// Used by the block-level parity tests (tests/golden/block.npz) — x / dy / y / dx cross the ABI as fp32 NCHW like the reference's.
FedfrNet* net_create_block(int cin, int cout, int stride, int hin, int batch) {
  const bool ds = stride != 1;
  if (batch <= 0 || hin <= 0 || (hin % stride) != 0 || cin <= 0 || cout <= 0 || (cin % 64) || (cout % 64) || (stride != 1 && stride != 2) ||
      (stride == 1 && cin != cout)) {
    fedfr_set_error("block_create: need channels%%64==0, stride 1 (cin==cout) or 2 (with downsample), even map (got %d->%d s%d @%d)", cin, cout,
                    stride, hin);
    return nullptr;
  }
  FedfrNet* n = new FedfrNet();
  for (int i = 0; i < 4; ++i) n->layers[i] = 0;
  n->block_only = true;
  n->B = batch; n->Bp = (batch + 7) / 8 * 8; n->HW = hin; n->F = 64;
  Builder b; b.n = n;
  n->blocks.push_back(b.add_block("", cin, cout, stride, hin, ds));
  n->final_hw = n->blocks[0].Hout; n->final_C = cout; n->fc_in = 0;
  n->fc_w_off = n->fc_b_off = -1;
  plan_layout(n, b, hin);
  return n;
}

// ---------------------------------------------------------------------------------------------------------
struct Ctx {
  const FedfrNet* n;
  const float* params; float* bufs; const bf16_t* shadow; bf16_t* actb; float* actf; unsigned char* ws; float* grads;
  hipStream_t st;
  float* part() const { return reinterpret_cast<float*>(ws + n->ws_part); }
  // second partial-row buffer: a channel-sliced pass reduces the rows it is handed while (other workgroups of the same launch) write the
  // rows of its own output, so those go to whichever buffer it does not read
  float* part2() const { return reinterpret_cast<float*>(ws + n->ws_part2); }
  float* part_other(const float* in) const { return in == part2() ? part() : part2(); }
  float* slab(int which = 0) const { return reinterpret_cast<float*>(ws + n->ws_slab) + (size_t)which * n->slab_floats; }
  float* coef() const { return reinterpret_cast<float*>(ws + n->ws_small); }
  float* ftmp() const { return coef() + 3 * 512; }
  float* dyfc() const { return ftmp() + 64 * 2 * 512; }
  bf16_t* dyb() const { return reinterpret_cast<bf16_t*>(dyfc() + (size_t)n->B * n->F); }
  bf16_t* dybt() const { return dyb() + (size_t)n->B * n->F; }
  bf16_t* g(int i) const { return reinterpret_cast<bf16_t*>(ws + n->ws_g[i]); }
  bf16_t* t(int i) const { return reinterpret_cast<bf16_t*>(ws + n->ws_t[i]); }
  // tensors read by the weight-gradient GEMMs (dc2 = slot 0, dc1 = slot 1, dd = slot 2), double buffered per block parity
  bf16_t* tw(int slot, int par) const { return reinterpret_cast<bf16_t*>(ws + (par ? n->ws_t2[(par - 1) * 3 + slot] : n->ws_t[slot * 2])); }
};
// a BatchNorm's parameters, running statistics (forward passes only: a backward Ctx has no buffers) and the four rows it saves
struct BnPtrs { const float *gamma, *beta; float *rm, *rv, *scale, *shift, *mean, *rstd; };
static BnPtrs bn_ptrs(const Ctx& c, const BnD& b) {
  float* s = c.actf + b.save_off;
  return {c.params + b.g_off, c.params + b.b_off, c.bufs ? c.bufs + b.rm_off : nullptr, c.bufs ? c.bufs + b.rv_off : nullptr,
          s, s + b.C, s + 2 * (long long)b.C, s + 3 * (long long)b.C};
}

static GemmNT fwd_problem(const Ctx& c, const ConvD& cv, const bf16_t* in, bf16_t* out) {
  GemmNT p = conv_fwd_problem(c.n->B, cv.Hin, cv.Cin, cv.Cout, cv.R, cv.stride);
  p.A = in; p.B = c.shadow + cv.w_off; p.Cb = out;
  return p;
}
// *live_rows (optional): the leading rows of the statistics that carry data (the rest are zero filler)
static int conv_fwd(const Ctx& c, const ConvD& cv, const bf16_t* in, bf16_t* out, bool stats, int* live_rows = nullptr) {
  GemmNT p = fwd_problem(c, cv, in, out);
  p.stats = stats ? c.part() : nullptr;
  if (live_rows) *live_rows = gemm_nt_plan(p, 1).stat_rows_live;
  return gemm_nt_launch(p, 1, c.st);
}
// eval mode: the problem of a conv with the BatchNorm (+PReLU, + identity, + the next block's bn1 as a second output) that follows it applied
// in the kernel's epilogue (GemmNT::esc ...), for the layers whose kernel implements it
int g_eval_fuse = 1;   // option "eval_fuse"
static GemmNT conv_fwd_ep(const Ctx& c, const ConvD& cv, const bf16_t* in, bf16_t* out, const BnD& bn, const float* alpha, const bf16_t* add,
                             bf16_t* out2, const BnD* bn2) {
  GemmNT p = fwd_problem(c, cv, in, out);
  const BnPtrs b = bn_ptrs(c, bn), b2 = out2 ? bn_ptrs(c, *bn2) : BnPtrs{};
  conv_set_out_epilogue(p, b.scale, b.shift, alpha, add, out2, b2.scale, b2.shift);
  return p;
}
static bool conv_epilogue_ok(const Ctx& c, const ConvD& cv, const BnD& bn, bool fuse) {      // (the plan reads which pointers are set, never through them)
  return fuse && gemm_nt_plan(conv_fwd_ep(c, cv, c.actb, c.actb, bn, nullptr, nullptr, nullptr, nullptr), 1).out_epilogue;
}
int g_fwd_xmom = 1;       // option "fwd_xmom": bn3 + identity + the next block's bn1 as one pass from conv2's raw moments (14x14 / 28x28 blocks)
int g_fuse_bnbwd28 = 1;   // option "fuse_bnbwd28": ... and in the two-tiles 28x28 dgrad (with fuse_bnbwd != 0)
int g_c64p_bnbwd = 1;   // option "c64p_bnbwd": BN-backward reduction in the epilogue of the persistent 64-channel dgrad kernel (with fuse_bnbwd != 0)
int g_fuse_bnbwd = 2;   // (round 3: 2 is the default, together with wgrad9p = 1 — see the end of this comment)  option "fuse_bnbwd": BN-backward reduction in the 3x3 dgrad epilogue (1: every layer a fused kernel serves; 2: the 14x14
                        // layers only, whose 128 partial rows the channel-sliced apply pass reduces itself).  LDS-DMA kernel: the x tile rides
                        // through the K loop in registers, the coefficients are requested in front of the drain: +3.7 us on a 28.6 us dgrad
                        // (round 1: x by LDS-DMA after the loop and 62 lazily issued coefficient loads, +11 us).  Off by default all the same:
                        // alone it removes 58 reduce launches (-0.35 ms of kernel time) and LENGTHENS the dual-stream step (16.96 -> 17.25 ms),
                        // because the reduce passes were windows in which the weight-gradient workgroups share the CUs, and the convolution
                        // that now follows sooner cannot start on a CU a weight-gradient workgroup still holds (54.9 us per fused dgrad in the
                        // dual-stream trace, 32.3 alone).  With the paired weight-gradient kernel (wgrad9p = 1) beside it the step is back at
                        // 16.94: both sides of the overlap have to shrink together (profiles/r02_ab_fuse_bnbwd_v2.txt).
                        // Round 3 (after the fork / join events lost their system-scope fence): the pair fuse_bnbwd = 2 + wgrad9p = 1 measures
                        // 17.00 / 17.01 ms against 17.21 / 17.15 for the old defaults, each alone still loses (17.40 / 17.34): both are on.
// dx (at the conv's INPUT resolution) = conv_transpose(dy).  If `bn` is given, the kernel may also produce the
// BN-backward partial sums of (dx, bn_x) in its epilogue; *fused_rows > 0 then (else run ew_bn_bwd_reduce).
static int conv_dgrad(const Ctx& c, const ConvD& cv, const bf16_t* dy, bf16_t* dx, const BnD* bn = nullptr,
                      const bf16_t* bn_x = nullptr, const float* alpha = nullptr, int* fused_rows = nullptr) {
  GemmNT p = conv_dgrad_problem(c.n->B, cv.Hin, cv.Cin, cv.Cout, cv.R, cv.stride);
  p.A = dy; p.B = c.shadow + cv.wd_off; p.Cb = dx;
  if (bn && fused_rows && g_fuse_bnbwd) {
    GemmNT f = p;
    const BnPtrs b = bn_ptrs(c, *bn);
    conv_set_bnbwd(f, bn_x, b.mean, b.rstd, b.gamma, b.beta, alpha, c.part());
    const NtPlan pl = gemm_nt_plan(f, 1);
    // option value 2: only the kernels that leave one partial row per workgroup, few enough for the channel-sliced apply pass to reduce itself —
    // 14x14 (one per image), the persistent 64 -> 64 kernel (conv_c64p.hip), the two-tiles 28x28 kernel (256 at B = 128) where that pass takes them
    const bool want = g_fuse_bnbwd == 1 || pl.kernel == NtKernel::glds8_fused_w14 || (g_c64p_bnbwd && pl.kernel == NtKernel::c64p) ||
                      (g_fuse_bnbwd28 && pl.kernel == NtKernel::glds8_fused_w28s && ew_bn_sliced_ok(f.M, f.N, pl.part_rows, true));
    if (pl.part_rows > 0 && want) { p = f; *fused_rows = pl.part_rows; }
  }
  return gemm_nt_launch(p, 1, c.st);
}
static GemmTN wgrad_problem(const Ctx& c, const ConvD& cv, const bf16_t* in, const bf16_t* dy) {
  GemmTN p = conv_wgrad_problem(c.n->B, cv.Hin, cv.Cin, cv.Cout, cv.R, cv.stride);
  p.P = dy; p.Q = in;
  return p;
}
// (the slab workspace was sized at plan creation: gemm_tn_max_splits over every kernel choice)
static int conv_wgrad(const Ctx& c, const ConvD& cv, const bf16_t* in, const bf16_t* dy, hipStream_t st) {
  return conv_wgrad_run(wgrad_problem(c, cv, in, dy), c.grads + cv.w_off, c.slab(), c.n->slab_floats, st);
}
// Slab sets of a paired nine-tap launch whose reduction has not been issued yet: the NEXT paired launch on the stream carries it out beside its own
// work (wgrad9p.hip, W9PJob), or wgrad_flush() issues the stand-alone launches — before anything else uses the slab workspace or reads the
// gradients (another weight-gradient kernel, the fused SGD of a finished stage, the end of the pass).
struct WgradPending {
  W9PJob job{};          // job.n == 0: nothing pending
  int set = 1;           // slab regions {2 set, 2 set + 1} hold the pending pair (the next pair writes the other set)
};
static int wgrad_flush(const Ctx& c, WgradPending* pd, hipStream_t st) {
  if (!pd || !pd->job.n) return FEDFR_OK;
  const W9PJob j = pd->job;
  pd->job.n = 0;
  // two reduction launches on purpose: ONE launch for both layers (ew_reduce_slabs2) measured 16.00 vs 15.85 ms/step same-box in round 3 —
  // the main stream waits for whatever the weight-gradient stream has resident, and two short kernels release the CUs sooner than one long
  FEDFR_TRY(ew_reduce_slabs(j.dst[0], j.slab[0], j.nsplit, j.n, nullptr, 0, st));
  return ew_reduce_slabs(j.dst[1], j.slab[1], j.nsplit, j.n, nullptr, 0, st);
}
int g_wgrad_pair_reduce = 1;   // option "wgrad_pair_reduce": one slab-reduction launch for the two 3x3 weight gradients of a block
// the two 3x3 weight gradients of a residual block; same shape (every block but a stage's first): one paired launch
#ifdef FEDFR_DEBUG
int g_dbg_skip = 0;   // option "dbg_skip" (-DFEDFR_DEBUG builds only; timing experiments, WRONG results): 1 = no weight-gradient launches of the residual blocks' 3x3 convs
#endif
static int conv_wgrad2(const Ctx& c, const ConvD& cva, const bf16_t* ina, const bf16_t* dya, const ConvD& cvb, const bf16_t* inb,
                       const bf16_t* dyb, hipStream_t st, WgradPending* pd = nullptr) {
#ifdef FEDFR_DEBUG
  if (g_dbg_skip & 1) return FEDFR_OK;
#endif
  GemmTN a = wgrad_problem(c, cva, ina, dya), b = wgrad_problem(c, cvb, inb, dyb);
  if (gemm_tn_w9pair_ok(a, b)) {                        // both on the 64 x 64 nine-tap kernel, one launch
    const int sp = gemm_tn_w9pair_splits(a);
    FEDFR_REQUIRE((size_t)sp * a.NI * a.NJ <= c.n->slab_floats, "conv_wgrad2: %d split-K slabs of %d x %d exceed the plan's slab workspace (%zu floats)",
                  sp, a.NI, a.NJ, c.n->slab_floats);
    const int set = pd ? pd->set ^ 1 : 0;
    static_assert(kSlabRegions >= 4, "two slab sets of two regions each");
    a.out = c.slab(2 * set); b.out = c.slab(2 * set + 1);
    // the previous pair's slabs: summed by this launch where its shape allows, else by their own launches first
    const bool carry = pd && pd->job.n && gemm_tn_w9pair_job_ok(a, sp, pd->job);
    if (pd && pd->job.n && !carry) FEDFR_TRY(wgrad_flush(c, pd, st));
    FEDFR_TRY(gemm_tn_launch_w9pair(a, b, sp, st, carry ? &pd->job : nullptr));
    W9PJob mine{};
    mine.slab[0] = a.out; mine.slab[1] = b.out; mine.dst[0] = c.grads + cva.w_off; mine.dst[1] = c.grads + cvb.w_off;
    mine.n = (size_t)a.NI * a.NJ; mine.nsplit = sp;
    if (pd) {
      pd->job = mine; pd->set = set;
      return FEDFR_OK;
    }
    WgradPending now; now.job = mine;
    return wgrad_flush(c, &now, st);
  }
  FEDFR_TRY(wgrad_flush(c, pd, st));                    // every other kernel below uses slab regions 0 / 1 itself
  const int splits = gemm_tn_pick_splits(a.Kp, a.NI, a.NJ, a.C, a.Wo, a.stride);
  // same shape, same split count: each launch writes its own slab set and ONE launch reduces both (45 launches fewer per step on the
  // weight-gradient stream, and the second GEMM does not wait behind the first one's reduction)
  if (g_wgrad_pair_reduce && splits >= 2 && a.NI == b.NI && a.NJ == b.NJ && a.Kp == b.Kp && a.C == b.C && a.Wo == b.Wo && a.stride == b.stride &&
      (size_t)splits * a.NI * a.NJ <= c.n->slab_floats) {
    a.out = c.slab(0); b.out = c.slab(1);
    FEDFR_TRY(gemm_tn_launch(a, splits, st));
    FEDFR_TRY(gemm_tn_launch(b, splits, st));
    return ew_reduce_slabs2(c.grads + cva.w_off, c.slab(0), c.grads + cvb.w_off, c.slab(1), splits, (size_t)a.NI * a.NJ, st);
  }
  FEDFR_TRY(conv_wgrad(c, cva, ina, dya, st));
  return conv_wgrad(c, cvb, inb, dyb, st);
}
struct Rows { float* ptr; int P; };     // where a BatchNorm's partial statistics rows are
static int bn_coeffs(const Ctx& c, const BnD& b, Rows r, double count, bool training) {
  const BnPtrs q = bn_ptrs(c, b);
  if (training) return ew_bn_finalize(r.ptr, r.P, b.C, count, q.gamma, q.beta, q.rm, q.rv, kBnMomentum, kBnEps, q.scale, q.shift, q.mean, q.rstd, c.ftmp(), c.st);
  return FEDFR_OK;      // eval mode: every BatchNorm's (scale, shift) was computed up front by eval_coeffs_all (one launch)
}
// eval-mode coefficients of all 2-D BatchNorms of the network in one launch (they depend on parameters and running statistics only;
// one small kernel per BatchNorm cost 154 launches = 0.6 ms of a 5.7 ms forward at batch 128)
static int eval_coeffs_all(const Ctx& c) {
  BnEvalTable t{};
  t.eps = kBnEps;
  auto flush = [&]() -> int {
    if (t.n == 0) return FEDFR_OK;
    const int rc = ew_bn_eval_coeffs_multi(c.params, c.bufs, c.actf, t, c.st);
    t.n = 0;
    return rc;
  };
  auto add = [&](const BnD& b) -> int {
    if (t.n == kMaxBnEvalEntries) FEDFR_TRY(flush());
    BnEvalEntry& e = t.e[t.n++];
    e.C = b.C; e.g_off = (int)b.g_off; e.b_off = (int)b.b_off; e.rm_off = (int)b.rm_off; e.rv_off = (int)b.rv_off; e.save_off = (int)b.save_off;
    return FEDFR_OK;
  };
  if (!c.n->block_only) FEDFR_TRY(add(c.n->stem_bn));
  for (const auto& k : c.n->blocks) {
    FEDFR_TRY(add(k.bn1)); FEDFR_TRY(add(k.bn2)); FEDFR_TRY(add(k.bn3));
    if (k.has_ds) FEDFR_TRY(add(k.bnds));
  }
  if (!c.n->block_only) FEDFR_TRY(add(c.n->bn2));
  return flush();
}
static int apply(const Ctx& c, const bf16_t* x1, const BnD& b1, const float* alpha, const bf16_t* x2, const BnD* b2, bf16_t* y,
                 int M, bool stats, int nchw_hw = 0) {
  BnApply a{};
  const BnPtrs q1 = bn_ptrs(c, b1), q2 = b2 ? bn_ptrs(c, *b2) : BnPtrs{};
  a.x1 = x1; a.sc1 = q1.scale; a.sh1 = q1.shift; a.alpha = alpha;
  a.x2 = x2; a.sc2 = q2.scale; a.sh2 = q2.shift;
  a.y = y; a.M = M; a.C = b1.C; a.nchw_hw = nchw_hw; a.stats = stats ? c.part() : nullptr;
  return ew_bn_apply(a, c.st);
}

// train-mode BatchNorm whose statistics are the partial rows `r`, applied: y = prelu?(bn(x1)) (+ x2).  One channel-sliced launch that reduces
// the rows itself where the shape allows (bn_sliced.hip), else finalize + the row-slab pass.  *out (optional) = where the statistics of y are.
static int bn_apply_train(const Ctx& c, const BnD& b, Rows r, const bf16_t* x1, const float* alpha, const bf16_t* x2, bf16_t* y, int M,
                          Rows* out) {
  if (ew_bn_sliced_ok(M, b.C, r.P, false)) {
    BnApplyS a{};
    const BnPtrs q = bn_ptrs(c, b);
    a.part = r.ptr; a.P = r.P; a.count = (double)M; a.gamma = q.gamma; a.beta = q.beta; a.rm = q.rm; a.rv = q.rv; a.momentum = kBnMomentum; a.eps = kBnEps;
    a.scale = q.scale; a.shift = q.shift; a.mean = q.mean; a.rstd = q.rstd;
    a.x1 = x1; a.alpha = alpha; a.x2 = x2; a.y = y; a.M = M; a.C = b.C;
    a.stats = out ? c.part_other(r.ptr) : nullptr;
    if (out) *out = Rows{a.stats, ew_bn_sliced_rows(M, b.C)};
    return ew_bn_apply_sliced(a, c.st);
  }
  FEDFR_TRY(bn_coeffs(c, b, r, (double)M, true));
  FEDFR_TRY(apply(c, x1, b, alpha, x2, nullptr, y, M, out != nullptr));
  if (out) *out = Rows{c.part(), ew_bn_apply_grid(M, b.C)};
  return FEDFR_OK;
}

// the fc layer of either backbone.  Forward: out [B][F] = in [B][fc_in] W^T + bias, split-K slabs summed by ew_reduce_slabs
static int fc_forward(const Ctx& c, const bf16_t* in, float* out) {
  const FedfrNet* n = c.n;
  GemmNT p{};
  p.A = in; p.B = c.shadow + n->fc_w_off; p.M = n->B; p.N = n->F; p.K = n->fc_in; p.mode = 0; p.lda = n->fc_in; p.Cf = c.slab();
  const int splits = gemm_nt_pick_splits(n->B, n->F, n->fc_in);
  FEDFR_REQUIRE((size_t)splits * n->B * n->F <= n->slab_floats, "fc_forward: split-K slabs exceed the plan's slab workspace");
  FEDFR_TRY(gemm_nt_launch(p, splits, c.st));
  return ew_reduce_slabs(out, c.slab(), splits, (size_t)n->B * n->F, c.params + n->fc_b_off, n->F, c.st);
}
// Backward: the weight gradient [F][fc_in] = dY^T X (both operands batch-major -> TN kernel) on stream `wst`, and dX [Bp][fc_in] = dY W
// (reduction over F: P = dY^T [F][Bp], Q = W [F][fc_in]) on the main stream.  dy: bf16 [B][F]; dyt: its transpose [F][Bp], columns >= B zero
static int fc_backward(const Ctx& c, const bf16_t* dy, const bf16_t* dyt, const bf16_t* in, float* dx, hipStream_t wst) {
  const FedfrNet* n = c.n;
  GemmTN w{};
  w.P = dy; w.Q = in; w.Kp = n->B; w.NI = n->F; w.NJ = n->fc_in; w.ldp = n->F; w.ldq = n->fc_in; w.out = c.grads + n->fc_w_off; w.use_tr = g_tn_use_tr;
  FEDFR_TRY(gemm_tn_launch(w, 1, wst));
  GemmTN d{};
  d.P = dyt; d.Q = c.shadow + n->fc_w_off; d.Kp = n->F; d.NI = n->Bp; d.NJ = n->fc_in; d.ldp = n->Bp; d.ldq = n->fc_in; d.out = dx; d.use_tr = g_tn_use_tr;
  return gemm_tn_launch(d, 1, c.st);
}
static int sph_prepare_weights(const FedfrNet* n, const float* params, bf16_t* shadow, int fwd_shadow_too, hipStream_t st);
static int sph_forward(const FedfrNet* n, const float* x, const float* params, const bf16_t* shadow, unsigned char* act, unsigned char* ws,
                       float* feats, hipStream_t st);
static int sph_backward(const FedfrNet* n, const float* dfeats, const float* params, const bf16_t* shadow, unsigned char* act, unsigned char* ws,
                        float* grads, hipStream_t st, hipStream_t aux, NetSgd* sgd);
int net_prepare_weights(const FedfrNet* n, const float* params, bf16_t* shadow, int fwd_shadow_too, hipStream_t st) {
  FEDFR_REQUIRE(n && params && shadow, "prepare_weights: null");
  if (n->sph_type) return sph_prepare_weights(n, params, shadow, fwd_shadow_too, st);
  if (fwd_shadow_too) FEDFR_TRY(ew_cast_f32_bf16(params, shadow, (size_t)n->trainable_count, st));
  // every conv's dgrad-layout copy ([Cin][taps flipped][Cout] bf16) in ONE launch (was one small kernel per conv: 105 per step)
  ShadowTable t{};
  auto add = [&](const ConvD& cv) {
    ShadowEntry& e = t.e[t.n++];
    e.src = (unsigned long long)cv.w_off; e.dst = (unsigned long long)cv.wd_off;
    e.cout64 = (unsigned short)(cv.Cout / 64); e.cin64 = (unsigned short)(cv.Cin / 64); e.rs = (unsigned short)(cv.R * cv.R);
  };
  for (const auto& k : n->blocks) {
    FEDFR_REQUIRE(k.conv1.Cout % 64 == 0 && k.conv1.Cin % 64 == 0 && k.conv2.Cout % 64 == 0 && k.conv2.Cin % 64 == 0,
                  "prepare_weights: channels not a multiple of 64");
    if (t.n + 3 > kMaxShadowEntries) {                  // deeper nets than iresnet100: one launch per table-full
      FEDFR_TRY(ew_weight_dgrad_shadow_multi(params, shadow, t, st));
      t.n = 0;
    }
    add(k.conv1); add(k.conv2);
    if (k.has_ds) add(k.ds);
  }
  if (t.n) FEDFR_TRY(ew_weight_dgrad_shadow_multi(params, shadow, t, st));
  return FEDFR_OK;
}

int net_forward(const FedfrNet* n, const float* x, const float* params, float* bufs, const bf16_t* shadow,
                unsigned char* act, unsigned char* ws, float* feats, int training, hipStream_t st) {
  if (n && n->sph_type) {                             // sphnet: no BatchNorm, so no buffers and no train / eval difference
    FEDFR_REQUIRE(x && params && shadow && act && ws && feats, "net_forward (sphnet): null buffer");
    return sph_forward(n, x, params, shadow, act, ws, feats, st);
  }
  FEDFR_REQUIRE(n && x && params && bufs && shadow && act && ws && (feats || n->block_only), "net_forward: null buffer");
  Ctx c{n, params, bufs, shadow, reinterpret_cast<bf16_t*>(act), reinterpret_cast<float*>(act + n->act_float_off_bytes), ws, nullptr, st};
  FEDFR_REQUIRE(training >= 0 && training <= 2, "net_forward: training must be 0 (eval), 1 (train) or 2 (train, BatchNorms frozen in eval mode)");
  // training = 2: every BatchNorm normalises with its running statistics and updates nothing (freeze_BN(test_mode=True)) while the net
  // trains — dropout stays on and every activation the backward pass reads is kept: the eval body with every fused epilogue refused
  const bool tr = training == 1, frozen = training == 2;
  const bool fuse = g_eval_fuse && !frozen;
  n->bn_frozen = frozen;
  const int B = n->B, HW = n->HW;
  const int M0 = B * HW * HW;
  bf16_t* A = c.actb;
  if (!tr) FEDFR_TRY(eval_coeffs_all(c));
  Rows prev{c.part(), 0};                  // statistics of the tensor the next BatchNorm normalises
  if (n->block_only) {
    // lone block: x (fp32 NCHW) -> NHWC bf16 block input; an identity "apply" pass leaves the column statistics bn1 needs, exactly
    // where the previous block's output pass leaves them inside a network
    const BlockD& k0 = n->blocks.front();
    FEDFR_TRY(ew_nchw_f32_to_nhwc_bf16(x, c.g(0), B, k0.Cin, HW * HW, st));
    BnApply a{};
    a.x1 = c.g(0); a.y = A + k0.x_off; a.M = M0; a.C = k0.Cin; a.stats = tr ? c.part() : nullptr;
    FEDFR_TRY(ew_bn_apply(a, st));
    prev.P = ew_bn_apply_grid(M0, k0.Cin);
  } else {
    // stem: conv -> BN -> PReLU   (iresnet.py:160-162)
    FEDFR_TRY(ew_stem_fwd(x, params + n->stem.w_off, A + n->c0_off, tr ? c.part() : nullptr, B, HW, HW, st));
    FEDFR_TRY(bn_coeffs(c, n->stem_bn, Rows{c.part(), ew_stem_stat_rows(B, HW, HW)}, (double)M0, tr));
    FEDFR_TRY(apply(c, A + n->c0_off, n->stem_bn, params + n->stem_alpha_off, nullptr, nullptr, A + n->a0_off, M0, tr));
    prev.P = ew_bn_apply_grid(M0, 64);
  }
  bool a1_ready = false;                    // eval: the previous block's conv2 epilogue already wrote this block's bn1(x)
  for (size_t bi = 0; bi < n->blocks.size(); ++bi) {
    const BlockD& k = n->blocks[bi];
    const int Mi = B * k.Hin * k.Hin, Mo = B * k.Hout * k.Hout;
    if (!tr) {
      // ---- eval mode: BatchNorms are known affines -> they ride in the conv epilogues where the kernel has one and `fuse` allows it
      if (!a1_ready) FEDFR_TRY(apply(c, A + k.x_off, k.bn1, nullptr, nullptr, nullptr, A + k.a1_off, Mi, false));
      a1_ready = false;
      if (conv_epilogue_ok(c, k.conv1, k.bn2, fuse)) {
        FEDFR_TRY(gemm_nt_launch(conv_fwd_ep(c, k.conv1, A + k.a1_off, A + k.a2_off, k.bn2, params + k.alpha_off, nullptr, nullptr, nullptr), 1, st));
      } else {
        FEDFR_TRY(conv_fwd(c, k.conv1, A + k.a1_off, A + k.c1_off, false));
        FEDFR_TRY(apply(c, A + k.c1_off, k.bn2, params + k.alpha_off, nullptr, nullptr, A + k.a2_off, Mi, false));
      }
      if (k.has_ds) FEDFR_TRY(conv_fwd(c, k.ds, A + k.x_off, A + k.d_off, false));
      if (conv_epilogue_ok(c, k.conv2, k.bn3, fuse)) {
        const bf16_t* idn = A + k.x_off;
        if (k.has_ds) {                                                 // identity = bnds(ds(x)), materialised in the (unused) c2 slot
          FEDFR_TRY(apply(c, A + k.d_off, k.bnds, nullptr, nullptr, nullptr, A + k.c2_off, Mo, false));
          idn = A + k.c2_off;
        }
        const BlockD* nx = bi + 1 < n->blocks.size() ? &n->blocks[bi + 1] : nullptr;
        FEDFR_TRY(gemm_nt_launch(conv_fwd_ep(c, k.conv2, A + k.a2_off, A + k.out_off, k.bn3, nullptr, idn, nx ? A + nx->a1_off : nullptr, nx ? &nx->bn1 : nullptr), 1, st));
        a1_ready = nx != nullptr;
      } else {
        FEDFR_TRY(conv_fwd(c, k.conv2, A + k.a2_off, A + k.c2_off, false));
        if (k.has_ds) FEDFR_TRY(apply(c, A + k.c2_off, k.bn3, nullptr, A + k.d_off, &k.bnds, A + k.out_off, Mo, false));
        else FEDFR_TRY(apply(c, A + k.c2_off, k.bn3, nullptr, A + k.x_off, nullptr, A + k.out_off, Mo, false));
      }
      continue;
    }
    // a1 = bn1(x) -> conv1 -> a2 = prelu(bn2(c1)) -> conv2(stride) -> bn3(c2) + identity.  Statistics: the pass that produced x left
    // them in `prev`; a conv's epilogue leaves its output's in c.part()
    // round 3 (option fwd_xmom): where conv2 runs on an LDS-DMA kernel with the moment epilogue, out = bn3(c2) + x AND the next block's
    // bn1(out) leave ONE pass (bn_apply2, ew.h): conv2 also sums c2 * x, and the statistics of `out` follow from those moments and the
    // statistics of x this block's bn1 saved — the next block's bn1 pass disappears
    const BlockD* nxb = bi + 1 < n->blocks.size() ? &n->blocks[bi + 1] : nullptr;
    int live = 0;                               // leading statistics rows of the conv just launched that carry data
    if (!a1_ready) FEDFR_TRY(bn_apply_train(c, k.bn1, prev, A + k.x_off, nullptr, nullptr, A + k.a1_off, Mi, nullptr));
    a1_ready = false;                           // (else: the previous block's output pass wrote a1 = bn1(x) and bn1's statistics)
    FEDFR_TRY(conv_fwd(c, k.conv1, A + k.a1_off, A + k.c1_off, true, &live));
    FEDFR_TRY(bn_apply_train(c, k.bn2, Rows{c.part(), live}, A + k.c1_off, params + k.alpha_off, nullptr, A + k.a2_off, Mi, nullptr));
    GemmNT pm = fwd_problem(c, k.conv2, A + k.a2_off, A + k.c2_off);      // conv2 with the moment epilogue
    conv_set_moments(pm, A + k.x_off, c.part());
    const NtPlan plm = gemm_nt_plan(pm, 1);
    // (x must have the output's shape; one partial row per workgroup, which the sliced pass reduces itself)
    const bool xmom = g_fwd_xmom && nxb && !k.has_ds && k.conv2.Cin == k.Cout && nxb->bn1.C == k.Cout && plm.part_rows > 0 &&
                      (plm.kernel == NtKernel::glds8_fused_w14 || plm.kernel == NtKernel::glds8_fused_w28s) &&
                      ew_bn_apply2_sliced_ok(Mo, k.Cout, plm.part_rows);
    if (xmom) {
      FEDFR_TRY(gemm_nt_launch(pm, 1, c.st));
      BnApply2S a{};
      const BnPtrs q = bn_ptrs(c, k.bn3), qx = bn_ptrs(c, k.bn1), qn = bn_ptrs(c, nxb->bn1);
      a.part = c.part(); a.P = plm.part_rows; a.count = (double)Mo; a.momentum = kBnMomentum; a.eps = kBnEps;
      a.gamma = q.gamma; a.beta = q.beta; a.rm = q.rm; a.rv = q.rv; a.scale = q.scale; a.shift = q.shift; a.mean = q.mean; a.rstd = q.rstd;
      a.xmean = qx.mean; a.xrstd = qx.rstd;
      a.ngamma = qn.gamma; a.nbeta = qn.beta; a.nrm = qn.rm; a.nrv = qn.rv; a.nscale = qn.scale; a.nshift = qn.shift; a.nmean = qn.mean; a.nrstd = qn.rstd;
      a.x1 = A + k.c2_off; a.x2 = A + k.x_off; a.y = A + k.out_off; a.y2 = A + nxb->a1_off; a.M = Mo; a.C = k.Cout;
      FEDFR_TRY(ew_bn_apply2_sliced(a, c.st));
      a1_ready = true;
      prev = Rows{c.part(), 0};
      continue;
    }
    FEDFR_TRY(conv_fwd(c, k.conv2, A + k.a2_off, A + k.c2_off, true, &live));
    const Rows r2{c.part(), live};
    if (k.has_ds) {
      FEDFR_TRY(bn_coeffs(c, k.bn3, r2, (double)Mo, true));
      FEDFR_TRY(conv_fwd(c, k.ds, A + k.x_off, A + k.d_off, true));
      FEDFR_TRY(bn_coeffs(c, k.bnds, Rows{c.part(), gemm_nt_stat_rows(Mo, k.Cout)}, (double)Mo, true));
      FEDFR_TRY(apply(c, A + k.c2_off, k.bn3, nullptr, A + k.d_off, &k.bnds, A + k.out_off, Mo, true));
      prev = Rows{c.part(), ew_bn_apply_grid(Mo, k.Cout)};
    } else {
      FEDFR_TRY(bn_apply_train(c, k.bn3, r2, A + k.c2_off, nullptr, A + k.x_off, A + k.out_off, Mo, &prev));
    }
  }
  if (n->block_only) return FEDFR_OK;
  // bn2 -> flatten (NCHW order) -> fc -> features   (iresnet.py:167-171)
  const BlockD& last = n->blocks.back();
  const int hw = n->final_hw * n->final_hw, Mf = B * hw;
  FEDFR_TRY(bn_coeffs(c, n->bn2, prev, (double)Mf, tr));
  FEDFR_TRY(apply(c, A + last.out_off, n->bn2, nullptr, nullptr, nullptr, A + n->t_off, Mf, false, hw));
  if ((tr || frozen) && n->dropout_p > 0.f)            // nn.Dropout(p, inplace=True) on the flattened bn2 output (iresnet.py:169); identity in eval mode
    FEDFR_TRY(ew_dropout_fwd(A + n->t_off, act + n->mask_off_bytes, (size_t)B * n->fc_in, n->dropout_p, n->dropout_seed, n->dropout_step++, st));
  FEDFR_TRY(fc_forward(c, A + n->t_off, c.actf + n->yfc_off));
  FEDFR_TRY(ew_bn1d_fwd(c.actf + n->yfc_off, feats, B, n->F, params + n->feat_bn.g_off, params + n->feat_bn.b_off,
                        bufs + n->feat_bn.rm_off, bufs + n->feat_bn.rv_off, kBnMomentum, kBnEps, tr ? 1 : 0,
                        c.actf + n->feat_save_off, c.actf + n->feat_save_off + n->F, st));
  return FEDFR_OK;
}

// debug capture (tests): when set, net_backward copies the gradient entering every block (bf16 NHWC [B*Hout*Hout][Cout], last block first)
// and finally the gradient wrt the first block's input, back to back into this caller-owned device buffer
bf16_t* g_dbg_grads = nullptr;
size_t g_dbg_grads_elems = 0;
// detail level 1: in front of everything the gradient wrt the network's bn2 output (NHWC [B*hw][C]), and behind every block's entering gradient g also dc2, da2, dc1, (dd, dxd of a downsample block,) da1, each copied on the main stream
// right behind the kernel that produced it (dxd is the compact [B*Hout*Hout][Cin] result the bn1 pass up-samples).  Level 0: g alone
int g_dbg_detail = 0;
static int dbg_capture(const bf16_t* src, size_t elems, size_t* off, hipStream_t st) {
  if (!g_dbg_grads) return FEDFR_OK;
  FEDFR_REQUIRE(*off + elems <= g_dbg_grads_elems, "net_backward: debug gradient buffer too small (%zu + %zu > %zu elements)", *off, elems,
                g_dbg_grads_elems);
  if (hipMemcpyAsync(g_dbg_grads + *off, src, elems * 2, hipMemcpyDeviceToDevice, st) != hipSuccess) {
    fedfr_set_error("net_backward: debug capture copy failed");
    return FEDFR_ERR_HIP;
  }
  *off += elems;
  return FEDFR_OK;
}
static const int g_wgrad_depth = kWgradDepth;   // generations of weight-gradient operands in flight (fewer: the main stream waits for the weight-gradient stream)
int g_fuse_bnred_next = 1;   // option "fuse_bnred_next": a BN-backward apply pass also reduces its output for the BN that consumes it
// BatchNorm (+PReLU) backward: dx = a dz + A x + B (+ addend).  This function decides which form runs and what rides along; the launches of
// either form are ew_bn_bwd_sliced / ew_bn_bwd_rowslab (ew.h), which the C ABI entries call too.
struct NextBn {               // the BatchNorm that consumes dx (no own addend): dx is also reduced as the dy of ITS backward
  const BnD* bn = nullptr; const bf16_t* x = nullptr;      // ... and its input tensor, same [M][C] shape
  long long slope_off = -1;   // >= 0: a PReLU follows it (the stem's) — served by the row-slab apply pass without own PReLU / addend
  Rows* rows = nullptr;       // where the rows are reported
};
struct BnBwdArgs {
  const BnD* bn;
  long long slope_off = -1;   // >= 0: a PReLU with these slopes follows the BatchNorm
  const bf16_t* dy; const bf16_t* x; int M; bf16_t* dx;
  const bf16_t* add = nullptr;                // same-shape addend (identity-path gradient)
  const bf16_t* add_up = nullptr; int H = 0;  // compact [img][H/2][H/2][C] addend placed at even (h, w)
  Rows have{nullptr, 0};      // partial rows that already exist (left by the pass that produced dy); else a reduce pass runs first
  NextBn next{};
  bool coef_only = false;     // reduce if needed + finalize, no apply pass: the consumer applies c.coef() itself (the stem's weight gradient; row-slab form only)
};
static int bn_bwd(const Ctx& c, const BnBwdArgs& a) {
  const BnD& b = *a.bn; const int M = a.M;
  const float* alpha = a.slope_off >= 0 ? c.params + a.slope_off : nullptr;
  float* dalpha = a.slope_off >= 0 ? c.grads + a.slope_off : nullptr;
#ifdef FEDFR_DBG_SKIP14
  // timing experiment only (WRONG results; tools/build_ablate.sh net.hip FEDFR_DBG_SKIP14 1): the bn1 / bn3 backward passes of the 14x14 stage are free —
  // the upper bound of anything that takes them out of the dispatcher's hands
  if (FEDFR_DBG_SKIP14 && !alpha && !c.n->block_only && M == c.n->B * 196 && b.C == 256) return FEDFR_OK;
#endif
  const bool sliced_ok = ew_bn_sliced_ok(M, b.C, a.have.P > 0 ? a.have.P : ew_bn_sliced_rows(M, b.C, true), true);
  const bool nxt = a.next.bn && a.next.x && a.next.rows && g_fuse_bnred_next && a.next.bn->C == b.C &&
                   (a.next.slope_off < 0 || (!alpha && !a.add && !sliced_ok));
  const BnPtrs q = bn_ptrs(c, b), qn = nxt ? bn_ptrs(c, *a.next.bn) : BnPtrs{};
  float* rows = a.have.P > 0 ? a.have.ptr : c.part();
  // frozen BatchNorm (eval mode inside a training net): mean / rstd were constants, so dx = gamma rstd dz — the same passes with an infinite
  // count (the two mean terms vanish); dgamma / dbeta / dalpha are the same sums
  const double count = c.n->bn_frozen ? HUGE_VAL : (double)M;
  if (!a.coef_only && !a.add_up && sliced_ok) {
    BnBwdS p{};
    p.dy = a.dy; p.x = a.x; p.mean = q.mean; p.rstd = q.rstd; p.gamma = q.gamma; p.alpha = alpha; p.sc = q.scale; p.sh = q.shift;
    p.M = M; p.C = b.C; p.count = count; p.partials = rows; p.dgamma = c.grads + b.g_off; p.dbeta = c.grads + b.b_off; p.dalpha = dalpha; p.add = a.add; p.dx = a.dx;
    if (nxt) {
      p.nx = a.next.x; p.nmean = qn.mean; p.nrstd = qn.rstd; p.npart = c.part_other(rows);
      *a.next.rows = Rows{p.npart, ew_bn_sliced_rows(M, b.C, true)};
    }
    return ew_bn_bwd_sliced(p, a.have.P, c.st);
  }
  BnBwd p{};
  if (nxt) {
    // dx is the dy of the next BatchNorm's backward: its (sum, sum * xhat) partials ride along in this apply pass (one tensor read instead of
    // a separate two-tensor reduce kernel); they land in the shared partial buffer, which this BN's finalize has finished reading
    p.nx = a.next.x; p.nmean = qn.mean; p.nrstd = qn.rstd; p.npart = c.part();
    if (a.next.slope_off >= 0) { p.nsc = qn.scale; p.nsh = qn.shift; p.nalpha = c.params + a.next.slope_off; }
    *a.next.rows = Rows{c.part(), ew_bn_bwd_apply_grid(M, b.C)};
  }
  p.dy = a.dy; p.x = a.x; p.mean = q.mean; p.rstd = q.rstd; p.gamma = q.gamma; p.beta = q.beta; p.alpha = alpha; p.sc = q.scale; p.sh = q.shift;
  p.M = M; p.C = b.C; p.partials = rows; p.coef = c.coef(); p.add = a.add; p.add_up = a.add_up; p.H = a.H; p.W = a.H; p.dx = a.dx;
  return ew_bn_bwd_rowslab(p, a.have.P, count, c.grads + b.g_off, c.grads + b.b_off, dalpha, a.coef_only, c.st);
}

int g_stem_fuse_wgrad = 1;   // option "stem_fuse_wgrad": the stem's BatchNorm + PReLU backward is applied by its weight-gradient kernel on load (no d(conv output) tensor)
int g_stem_bnred = 1;     // option "stem_bnred": the stem's BatchNorm-backward reduction rides in the first block's bn1 apply pass
// (fc's weight gradient runs on the weight-gradient stream, and fork / join events are created with hipEventDisableSystemFence — a system-scope
// release per event costs the main stream ~5 us: options "fc_wgrad_aux" / "event_nofence" of rounds 3-5, removed in round 6 after losing every sweep)
// fork/join helpers for the dual-stream backward (events are created once per plan)
namespace {
struct Fork {
  const FedfrNet* n;
  hipStream_t main, aux;
  size_t next = 0;
  bool ok = true;
  hipEvent_t ev() {
    if (next == n->events.size()) {
      hipEvent_t e;
      if (hipEventCreateWithFlags(&e, hipEventDisableTiming | hipEventDisableSystemFence) != hipSuccess) { ok = false; return nullptr; }
      n->events.push_back(e);
    }
    return n->events[next++];
  }
  // everything enqueued so far on `from` happens before anything enqueued later on `to`
  void order(hipStream_t from, hipStream_t to) {
    if (!aux) return;
    hipEvent_t e = ev();
    if (!e || hipEventRecord(e, from) != hipSuccess || hipStreamWaitEvent(to, e, 0) != hipSuccess) ok = false;
  }
  hipEvent_t mark(hipStream_t s) {            // record now, wait later
    if (!aux) return nullptr;
    hipEvent_t e = ev();
    if (!e || hipEventRecord(e, s) != hipSuccess) ok = false;
    return e;
  }
  void wait(hipStream_t s, hipEvent_t e) {
    if (aux && e && hipStreamWaitEvent(s, e, 0) != hipSuccess) ok = false;
  }
};
}  // namespace

int net_backward(const FedfrNet* n, const float* x, const float* dfeats, const float* params, const bf16_t* shadow,
                 unsigned char* act, unsigned char* ws, float* grads, hipStream_t st, hipStream_t aux, NetSgd* sgd) {
  if (n && n->sph_type) {
    FEDFR_REQUIRE(dfeats && params && shadow && act && ws && grads, "net_backward (sphnet): null buffer");
    return sph_backward(n, dfeats, params, shadow, act, ws, grads, st, aux, sgd);
  }
  FEDFR_REQUIRE(n && (x || n->block_only) && dfeats && params && shadow && act && ws && grads, "net_backward: null buffer");
  Ctx c{n, params, nullptr, shadow, reinterpret_cast<bf16_t*>(act), reinterpret_cast<float*>(act + n->act_float_off_bytes), ws, grads, st};
  const int B = n->B, F = n->F, HW = n->HW;
  bf16_t* A = c.actb;
  Fork fk{n, st, aux};
  const hipStream_t wst = aux ? aux : st;          // stream of the weight-gradient GEMMs
  if (n->block_only) fk.order(st, wst);             // aux starts after everything already queued on main (forward pass); the full net forks below
  Rows pend{nullptr, 0};                           // partial rows of the next bn3 already reduced by the apply pass that produced its dy
  size_t dbg_off = 0;
  if (n->block_only) {
    const BlockD& k0 = n->blocks.front();
    FEDFR_TRY(ew_nchw_f32_to_nhwc_bf16(dfeats, c.g(1), B, k0.Cout, k0.Hout * k0.Hout, st));      // dy of the block, fp32 NCHW like the reference's
  } else {
  // ---- features (BN1d) backward; fc.bias grad = colsum(d y_fc) ----
  if (n->Bp != B && hipMemsetAsync(c.dybt(), 0, (size_t)F * n->Bp * 2, st) != hipSuccess) {      // zero padding of the batch axis of dY^T (Bp = B rounded up to 8)
    fedfr_set_error("net_backward: hipMemsetAsync failed");
    return FEDFR_ERR_HIP;
  }
  FEDFR_TRY(ew_bn1d_bwd(dfeats, c.actf + n->yfc_off, c.dyfc(), B, F, params + n->feat_bn.g_off, c.actf + n->feat_save_off,
                        c.actf + n->feat_save_off + F, grads + n->feat_bn.b_off, grads + n->fc_b_off, c.dyb(), c.dybt(), n->Bp, st,
                        n->bn_frozen ? 1 : 0));
  float* dxfc = reinterpret_cast<float*>(ws + n->ws_fc);
  // the first fork: the weight-gradient stream starts behind the forward pass and the features' backward; fc's weight gradient is its first
  // kernel (round 3: it ran on the main stream, 20 us in front of everything else)
  fk.order(st, wst);
  FEDFR_TRY(fc_backward(c, c.dyb(), c.dybt(), A + n->t_off, dxfc, wst));
  const BlockD& last = n->blocks.back();
  const int hw = n->final_hw * n->final_hw, Mf = B * hw;
  if (n->dropout_p > 0.f) FEDFR_TRY(ew_dropout_bwd(dxfc, act + n->mask_off_bytes, (size_t)B * n->fc_in, n->dropout_p, st));
  FEDFR_TRY(ew_nchw_f32_to_nhwc_bf16(dxfc, c.g(0), B, n->final_C, hw, st));
  if (g_dbg_grads && g_dbg_detail) FEDFR_TRY(dbg_capture(c.g(0), (size_t)Mf * n->final_C, &dbg_off, st));      // detail: the gradient entering bn2's backward, first
  FEDFR_TRY(bn_bwd(c, {.bn = &n->bn2, .dy = c.g(0), .x = A + last.out_off, .M = Mf, .dx = c.g(1),
                       .next = {.bn = &last.bn3, .x = A + last.c2_off, .rows = &pend}}));
  }
  int cur = 1;
  // fused SGD (NetSgd): [sgd_lo, sgd_hi) = parameter range whose gradients are complete on the main stream and whose weight gradients are
  // all queued on the weight-gradient stream; it is updated there behind the next fork (which orders it after everything queued on main).
  // Nothing reads those parameters again in this pass: dgrad uses the bf16 shadows, BatchNorm backward its own layer's gamma / slope.
  long long sgd_lo = -1, sgd_hi = -1;
  if (sgd && !n->block_only) {
    FEDFR_REQUIRE(sgd->params == params && sgd->shadow == shadow && sgd->mom, "net_backward: fused SGD wants the pass's own parameter / shadow buffers");
    sgd->done_from = n->trainable_count;
    sgd_lo = n->bn2.g_off; sgd_hi = n->trainable_count;     // bn2, fc, features: their gradients were written at the top of this pass
  }
  auto sgd_flush = [&]() -> int {
    if (sgd_lo < 0 || sgd_lo >= sgd_hi) return FEDFR_OK;
    FEDFR_REQUIRE((sgd_lo & 3) == 0, "net_backward: fused SGD range not 16-byte aligned");
    FEDFR_TRY(optim_sgd(sgd->params + sgd_lo, grads + sgd_lo, sgd->mom + sgd_lo, sgd->shadow + sgd_lo, (size_t)(sgd_hi - sgd_lo), sgd->lr, sgd->mu,
                        sgd->wd, sgd->first, wst, sgd->gscale, sgd->overflow, sgd->anchor ? sgd->anchor + sgd_lo : nullptr, sgd->prox,
                        sgd->corr ? sgd->corr + sgd_lo : nullptr));
    sgd->done_from = sgd_lo;
    sgd_hi = sgd_lo; sgd_lo = -1;
    return FEDFR_OK;
  };
  hipEvent_t wdone[kWgradDepth] = {};              // "all weight GEMMs of the block of this generation have finished"
  WgradPending pend_w;                             // a paired weight-gradient launch whose slabs the next one sums (wgrad9p.hip)
  for (int bi = (int)n->blocks.size() - 1; bi >= 0; --bi) {
    const BlockD& k = n->blocks[bi];
    const int Mi = B * k.Hin * k.Hin, Mo = B * k.Hout * k.Hout;
    const int par = bi % g_wgrad_depth;
    const bf16_t* g = c.g(cur);
    bf16_t* gin = c.g(cur ^ 1);
    FEDFR_TRY(dbg_capture(g, (size_t)Mo * k.Cout, &dbg_off, st));
    bf16_t *dc2 = c.tw(0, par), *da2 = c.t(1), *dc1 = c.tw(1, par), *da1 = c.t(3), *dd = c.tw(2, par), *dxd = c.t(5);
    auto detail = [&](const bf16_t* src, size_t elems) -> int {      // (no capture buffer or level 0: no launch)
      return g_dbg_grads && g_dbg_detail ? dbg_capture(src, elems, &dbg_off, st) : FEDFR_OK;
    };
    fk.wait(st, wdone[par]);                         // the weight GEMMs kWgradDepth blocks ago were the last readers of dc2/dc1/dd[par]
    // out = bn3(c2) + identity
    FEDFR_TRY(bn_bwd(c, {.bn = &k.bn3, .dy = g, .x = A + k.c2_off, .M = Mo, .dx = dc2, .have = pend}));
    FEDFR_TRY(detail(dc2, (size_t)Mo * k.Cout));
    pend = Rows{nullptr, 0};
    int f2 = 0, f1 = 0;
    FEDFR_TRY(conv_dgrad(c, k.conv2, dc2, da2, &k.bn2, A + k.c1_off, params + k.alpha_off, &f2));
    FEDFR_TRY(detail(da2, (size_t)Mi * k.Cout));
    // a2 = prelu(bn2(c1))
    FEDFR_TRY(bn_bwd(c, {.bn = &k.bn2, .slope_off = k.alpha_off, .dy = da2, .x = A + k.c1_off, .M = Mi, .dx = dc1, .have = Rows{c.part(), f2}}));
    FEDFR_TRY(detail(dc1, (size_t)Mi * k.Cout));
    // identity path first (its BN reduction uses the shared partial buffer), then conv1's dgrad whose epilogue may
    // leave bn1's partial sums there for the bn_bwd that follows immediately
    if (k.has_ds) {
      FEDFR_TRY(bn_bwd(c, {.bn = &k.bnds, .dy = g, .x = A + k.d_off, .M = Mo, .dx = dd}));
      FEDFR_TRY(detail(dd, (size_t)Mo * k.Cout));
    }
    // ONE fork per block: every event record costs the main stream a ~8 us bubble (kernel trace), so the block's two or three
    // weight-gradient GEMMs are released together once their last operand (dc2, dc1, dd) exists
    fk.order(st, wst);
    if (sgd_lo >= 0 && sgd_lo < sgd_hi) FEDFR_TRY(wgrad_flush(c, &pend_w, wst));      // the fused SGD reads the finished stage's gradients
    FEDFR_TRY(sgd_flush());
    FEDFR_TRY(conv_wgrad2(c, k.conv2, A + k.a2_off, dc2, k.conv1, A + k.a1_off, dc1, wst, &pend_w));
    if (k.has_ds) {
      FEDFR_TRY(wgrad_flush(c, &pend_w, wst));
      FEDFR_TRY(conv_wgrad(c, k.ds, A + k.x_off, dd, wst));
      FEDFR_TRY(conv_dgrad(c, k.ds, dd, dxd));
      FEDFR_TRY(detail(dxd, (size_t)Mo * k.Cin));
    }
    wdone[par] = fk.mark(wst);
    FEDFR_TRY(conv_dgrad(c, k.conv1, dc1, da1, &k.bn1, A + k.x_off, nullptr, &f1));
    FEDFR_TRY(detail(da1, (size_t)Mi * k.Cin));
    // a1 = bn1(x).  The identity path's gradient joins here: g itself, or the downsample conv's compact dxd.  gin is then the dy of the previous
    // block's bn3 — or, behind the first block, of the STEM's BatchNorm (+PReLU) backward, reduced here (one pass over two 205 MB tensors fewer)
    BnBwdArgs b1{.bn = &k.bn1, .dy = da1, .x = A + k.x_off, .M = Mi, .dx = gin, .have = Rows{c.part(), f1}};
    if (k.has_ds) { b1.add_up = dxd; b1.H = k.Hin; } else b1.add = g;
    if (bi > 0) b1.next = {.bn = &n->blocks[bi - 1].bn3, .x = A + n->blocks[bi - 1].c2_off, .rows = &pend};
    else if (k.has_ds && !n->block_only && g_stem_bnred) b1.next = {.bn = &n->stem_bn, .x = A + n->c0_off, .slope_off = n->stem_alpha_off, .rows = &pend};
    FEDFR_TRY(bn_bwd(c, b1));
    cur ^= 1;
    if (sgd && !n->block_only && k.has_ds && bi > 0) sgd_lo = k.bn1.g_off;      // a stage is complete: its range goes out behind the next fork
  }
  FEDFR_TRY(wgrad_flush(c, &pend_w, wst));
  // join: callers see all grads.  It sits at the very END: neither the stem's BatchNorm backward (two passes over 205 MB tensors; its dz goes to
  // t(1) — da2 of the blocks, main stream only — instead of t(0), which block 0's weight gradient may still be reading) nor the stem's
  // weight gradient (own partials, ws_stem) waits for the last weight gradients of stage 1
  if (n->block_only) fk.order(wst, st);
  const int M0 = B * HW * HW;
  FEDFR_TRY(dbg_capture(c.g(cur), (size_t)M0 * n->blocks.front().Cin, &dbg_off, st));
  if (n->block_only) {                               // the gradient wrt the block input stays readable in the arena
    if (hipMemcpyAsync(A + n->dx_off, c.g(cur), (size_t)M0 * n->blocks.front().Cin * 2, hipMemcpyDeviceToDevice, st) != hipSuccess) {
      fedfr_set_error("net_backward: hipMemcpyAsync failed");
      return FEDFR_ERR_HIP;
    }
  } else {
  // ---- stem: a0 = prelu(bn1(conv1(x))) ----
  bf16_t* dz0 = c.t(1);
  const bool fuse = g_stem_fuse_wgrad != 0;
  FEDFR_TRY(bn_bwd(c, {.bn = &n->stem_bn, .slope_off = n->stem_alpha_off, .dy = c.g(cur), .x = A + n->c0_off, .M = M0, .dx = dz0, .have = pend, .coef_only = fuse}));
  if (fuse)     // the only reader of d(conv output) is the weight gradient: it applies the backward to its operand tile (two 205 MB streams fewer at batch 128)
    FEDFR_TRY(ew_stem_wgrad(x, c.g(cur), grads + n->stem.w_off, reinterpret_cast<float*>(ws + n->ws_stem), B, HW, HW, st, A + n->c0_off, c.coef(),
                            bn_ptrs(c, n->stem_bn).scale, bn_ptrs(c, n->stem_bn).shift, params + n->stem_alpha_off));
  else
  FEDFR_TRY(ew_stem_wgrad(x, dz0, grads + n->stem.w_off, reinterpret_cast<float*>(ws + n->ws_stem), B, HW, HW, st));
  fk.order(wst, st);
  }
  if (!fk.ok) {
    fedfr_set_error("net_backward: HIP event record/wait failed");
    return FEDFR_ERR_HIP;
  }
  return FEDFR_OK;
}

#include "net_sph.inc"
