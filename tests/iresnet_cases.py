"""Block table, restated dispatch, fp64 references and tolerances for the block-by-block tests of the iresnet plan (csrc/net.hip: net_forward with
training = 1, net_backward), in the manner of sphnet_cases.py.  conv_cases, rowslab_cases, bn_sliced_cases and stem_cases are used, not copied.
Nothing here touches the GPU library or imports the oracle.

`compare` walks the blocks and holds every tensor a pass leaves behind to a float64 reference that is fed with the pass's own STORED operands: the
16-bit activations, the fp32 (scale, shift, mean, rstd) rows every BatchNorm saved, the captured 16-bit gradients of fedfr_net_debug_capture at detail
level 1, and the fp32 parameter gradients (a BatchNorm-backward apply pass forms its coefficients from the very sums it stores as dbeta and dgamma, so
dx is held to the coefficients that follow from the STORED sums, and the sums are held to the reference separately).  Nothing compounds from block
to block, and every element of every tensor is part of its comparison.

The PReLU side of an element is the sign of z = fma(c, scale, shift) in float32 (stem_cases.fma), c being the stored conv output and (scale, shift)
the stored rows.  c is the network's own output and cannot be moved off the threshold, so where |z| lies inside the float32 error of that
expression — 3 2^-24 (|c scale| + |shift|): the product's rounding, the sum's, and the contracted against the plain form — either side is accepted:
the smaller of the two ratios counts, and in the column sums the difference between the two sides of those elements is added to the bound.  No
element is excluded; `info["ambiguous"]` counts them.

Statistics a kernel forms BEFORE a 16-bit store are held to the float64 statistics of the unrounded reference value, with a bound that follows the
conditioning:
  * the next block's bn1 under fwd_xmom (bn_apply2, derived from conv2's raw moments and this block's saved bn1 statistics): mean and variance of
    scale c2 + shift + x in float64, bound in the form of bn_sliced_cases.Apply2Case.second — the fp32 chains of the three moment rows, the bound
    the saved statistics of x were themselves held to, and COEF_ULPS 2^-24 of the magnitudes of the terms that cancel;
  * the rows a dgrad epilogue leaves from its fp32 accumulator (fuse_bnbwd / c64p_bnbwd / fuse_bnbwd28): the sums of the float64 dgrad of the stored
    operands, bound conv_cases.bnbwd_q's (rows_L + 4) 2^-24 sum |terms| plus what the accumulator's own bound (K + 2) 2^-24 S leaves of each term.
Sums a pass forms from a STORED tensor are held to the float64 sums of that tensor: chain 2^-24 sum |terms|, chain = the fp32 chain of the kernel
the restated dispatch selects for that BatchNorm (Net.fwd_walk / bwd_walk: a conv epilogue's rows, the row-slab reduce / apply slabs of
stem_cases.colsum_chain, the channel-sliced pixel groups of bn_sliced_cases.passes + SUM_TREE), + 1 for the single fp32 rounding of a staged finalize.

Tolerances (element-wise, formulas of u16, 2^-24, a chain length and S = sum |terms|; none is a measured number):
  conv / dgrad output      conv_cases.out16_q + floor16                         u16 |ref| + (K + 2) 2^-24 S
  BatchNorm forward y      rowslab_cases.ApplyCase.y_q + floor16                u16 |y| + K_APPLY 2^-24 (|x sc| + |sh| (+ the addend's terms))
  saved coefficients       bn_sliced_cases.fwd_coef's COEF_ULPS 2^-24 of the magnitudes, + what the chain bound of the two sums leaves of each
  BatchNorm backward dx    stem_cases.dx_q (unconditioned) + stem_cases.bn_coef_tol for one unit in the last place of the stored sums
  dgamma / dbeta / dalpha  chain 2^-24 sum |terms| + COEF_ULPS 2^-24 |value| (bn_sliced_cases.BwdCase.grads_q), see above
  weight gradients         conv_cases.dw_q's form with sphnet_cases.dw_chain and the split count of the restated dispatch
  stem weight gradient     stem_cases.StemWgradCase.dw's (2^-17 + L 2^-24) sum |dz0 col| + what the coefficients' bound leaves of dz0, and for the 16-bit
                           rounding of the operand dz0, which is never stored, the double-rounding bound u16 sum |dz0 col|.  (Not the four standard
                           deviations of independent roundings tests/test_stem_chain_gpu.py uses at M = 3468: dz0 = a g + A x + B is dominated by a g,
                           g has 8 or 11 significant bits, so the rounding of a g is a function of g's few mantissa values and does not average out
                           over 1.6 million pixels — the bf16 build exceeds 4 sigma by 3.5 at batch 128.)
The gradient leaving a block is ONE rounding of a (da1) + A x + B + addend (the bn1 apply pass adds g, or the up-sampled dxd, in fp32): dx_q's form
with the addend among the terms — there is no second store to bound, unlike sphnet_cases.gsum_tol."""
import torch

import bn_sliced_cases as BS
import conv_cases as K
import rowslab_cases as RS
import stem_cases as S
from sphnet_cases import dw_chain, out16_tol, ratio
from stem_cases import U24, colsum_chain, f32, f64, slab_rows, u16

LAYERS = {"iresnet18": (2, 2, 2, 2), "iresnet50": (3, 4, 14, 3), "iresnet100": (3, 13, 30, 3)}
CARRY_LAYERS = (1, 1, 3, 1)                 # consecutive identity blocks at 14x14: a paired weight-gradient launch finds a pending pair
PLANES = (64, 128, 256, 512)
COEF = BS.COEF_ULPS * U24
BN_TENSORS = ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")


# ================================================================================================ the block table
class Block:
    def __init__(self, idx, prefix, cin, cout, stride, hin, has_ds):
        self.idx, self.prefix, self.cin, self.cout, self.stride, self.hin, self.hout, self.has_ds = idx, prefix, cin, cout, stride, hin, hin // stride, has_ds

    def bns(self):
        """(key, state_dict prefix, channels) of the block's BatchNorms in state_dict order"""
        out = [("bn1", self.prefix + "bn1", self.cin), ("bn2", self.prefix + "bn2", self.cout), ("bn3", self.prefix + "bn3", self.cout)]
        return out + ([("bnds", self.prefix + "downsample.1", self.cout)] if self.has_ds else [])

    def names(self):
        p, out = self.prefix, []
        bn = lambda n, c: [(n + "." + t, () if t == "num_batches_tracked" else (c,)) for t in BN_TENSORS]  # noqa: E731
        out += bn(p + "bn1", self.cin) + [(p + "conv1.weight", (self.cout, self.cin, 3, 3))] + bn(p + "bn2", self.cout)
        out += [(p + "prelu.weight", (self.cout,)), (p + "conv2.weight", (self.cout, self.cout, 3, 3))] + bn(p + "bn3", self.cout)
        if self.has_ds:
            out += [(p + "downsample.0.weight", (self.cout, self.cin, 1, 1))] + bn(p + "downsample.1", self.cout)
        return out


def build_blocks(layers4, hin, planes=PLANES, cin0=64):
    """net_create's walk: a stage's first block has stride 2 and a downsample path, the others are identity blocks"""
    out, inpl, H = [], cin0, hin
    for s, L in enumerate(layers4):
        for i in range(L):
            b = Block(len(out), "layer%d.%d." % (s + 1, i), inpl if i == 0 else planes[s], planes[s], 2 if i == 0 else 1, H, i == 0)
            out.append(b)
            H = b.hout
        inpl = planes[s]
    return out


class Net:
    """an iresnet plan (layers4 at batch B, 112 x 112 input, F features) or, with `mini` = (hin, cin0, planes), a miniature block stack of the same wiring
    without stem and tail whose dispatch facts are set by hand (mini_xmom, mini_fused, mini_splits, mini_carry)"""

    def __init__(self, layers4, B, mini=None, cus=256, F=512):
        self.layers4, self.B, self.cus, self.F, self.mini = tuple(layers4), B, cus, F, mini is not None
        hin, cin0, planes = mini if mini else (112, 64, PLANES)
        self.hin = hin
        self.blocks = build_blocks(layers4, hin, planes, cin0)
        last = self.blocks[-1]
        self.hw, self.C = last.hout * last.hout, last.cout
        self.fc_in = self.hw * self.C
        self.mini_xmom, self.mini_fused, self.mini_splits, self.mini_carry = set(), set(), 2, set()
        self.stem, self.tail = not self.mini, not self.mini      # a miniature stack may be given the tail (bn2 -> fc -> features)

    def tensor_names(self):
        bn = lambda n, c: [(n + "." + t, () if t == "num_batches_tracked" else (c,)) for t in BN_TENSORS]  # noqa: E731
        out = [("conv1.weight", (64, 3, 3, 3))] + bn("bn1", 64) + [("prelu.weight", (64,))]
        for b in self.blocks:
            out += b.names()
        return out + bn("bn2", 512) + [("fc.weight", (self.F, self.fc_in)), ("fc.bias", (self.F,))] + bn("features", self.F)

    def bn_table(self):
        """(state_dict prefix, channels) of the 2-D BatchNorms in fedfr_net_bn_info's order"""
        out = [] if self.mini else [("bn1", 64)]
        for b in self.blocks:
            out += [(n, c) for _, n, c in b.bns()]
        return out + ([] if self.mini else [("bn2", 512)])

    # ------------------------------------------------------------------------ dispatch, restated from net.hip over conv_cases / bn_sliced_cases
    def plan(self, hin, cin, cout, k, s, dgrad, want):
        """(slot, stat_rows, stat_rows_live, part_rows, out_epilogue) — conv_cases.plan_expected, what fedfr_conv2d_plan answers"""
        return K.plan_expected(self.B, hin, cin, cout, k, s, dgrad, want, cus=self.cus)

    def xmom(self, b):
        """net_forward: bn3 + identity + the next block's bn1 as one bn_apply2 pass from conv2's raw moments"""
        if self.mini:
            return b.idx in self.mini_xmom
        nxt = self.blocks[b.idx + 1] if b.idx + 1 < len(self.blocks) else None
        if nxt is None or b.has_ds or nxt.cin != b.cout:
            return False
        M = self.B * b.hout * b.hout
        slot, _, _, part, _ = self.plan(b.hin, b.cout, b.cout, 3, 1, False, K.WANT_MOMENTS)
        two = slot == 13 and part == M // 392                     # glds8_fused_w28s, the two-tiles kernel
        return part > 0 and (slot == 12 or two) and BS.apply2_ok(M, b.cout, part)

    def fused_rows(self, b, which):
        """net.hip conv_dgrad under fuse_bnbwd = 2: the partial rows the dgrad epilogue of conv2 (which = 2: for bn2, with the PReLU) or conv1 (1: for
        bn1) leaves, 0 if the BatchNorm backward reduces the stored tensor itself"""
        if self.mini:
            return 1 if (b.idx, which) in self.mini_fused else 0
        cv_in, stride = (b.cout, b.stride) if which == 2 else (b.cin, 1)
        M = self.B * b.hin * b.hin
        slot, _, _, part, _ = self.plan(b.hin, cv_in, b.cout, 3, stride, True, K.WANT_BNBWD)
        if part <= 0:
            return 0
        want = slot == 12 or (slot == 15 and cv_in == 64 and b.cout == 64) or (slot == 13 and part == M // 392 and BS.sliced_ok(M, cv_in, part, True))
        return part if want else 0

    def dgrad_slot(self, b, which):
        cv_in, stride = (b.cout, b.stride) if which == 2 else (b.cin, 1)
        return self.plan(b.hin, cv_in, b.cout, 3, stride, True, K.WANT_BNBWD if self.fused_rows(b, which) else 0)[0]

    def pair_ok(self, b):
        """wgrad9p.hip wgrad9p_applies: conv2 and conv1 of an identity block on the paired nine-tap kernel"""
        if self.mini:
            return not b.has_ds
        return (not b.has_ds and b.cin == b.cout and b.cout % 64 == 0 and
                K.wgrad9_shape_ok(self.B * b.hout * b.hout, b.cout, 9 * b.cin, b.cin, b.hout, 1))

    def wgrad(self, b, which):
        """(profile slot, split count) of the weight gradient of conv2 (2), conv1 (1) or the downsample conv (0)"""
        if self.mini:
            return None, self.mini_splits
        if which and self.pair_ok(b):
            return 16, K.wgrad9p_pick_splits(self.B * b.hout * b.hout, b.cout, 9 * b.cin, b.hout)
        if which == 2:
            return K.wgrad_slot_splits(self.B, b.hin, b.cout, b.cout, 3, b.stride)
        if which == 1:
            return K.wgrad_slot_splits(self.B, b.hin, b.cin, b.cout, 3, 1)
        return K.wgrad_slot_splits(self.B, b.hin, b.cin, b.cout, 1, b.stride)

    def job_ok(self, b, splits, job):
        """wgrad9p.hip wgrad9p_job_ok / w9p_job_geometry: the paired launch of block b sums the pending job = (floats per layer, its split count)"""
        n, nsplit = job
        stages = K.w9_stages(self.B * b.hout * b.hout, b.hout)
        grid = 2 * (b.cout // 64) * (b.cin // 64) * splits
        if n % 4 or nsplit < 1 or grid < 1:
            return False
        n4 = n // 4
        if (2 * n4) % grid:
            return False
        per = 2 * n4 // grid
        if n4 % per or nsplit * n4 * 16 >= 1 << 32:
            return False
        wide = nsplit >= 16 and n4 <= 65536
        if (nsplit != 32) if wide else (nsplit % 4 != 0):
            return False
        return K.cdiv(per, 256) * (8 if wide else nsplit // 4) <= stages // splits

    def wgrad_walk(self, bg=True, pair_reduce=True):
        """net_backward's weight-gradient stream: ([block index of every paired launch that CARRIES the previous pair's slab sums], stand-alone slab
        reductions (profile slot 25)).  bg = False: option wgrad9p_bg = 0; pair_reduce = False: option wgrad_pair_reduce = 0 (an identity block's two
        same-shape weight gradients that the paired kernel does not take — the 7x7 stage — share ONE reduction launch by default)"""
        carries, red, pending = [], 0, None
        for b in reversed(self.blocks):
            if self.pair_ok(b):
                sp = self.wgrad(b, 2)[1]
                carry = (b.idx in self.mini_carry) if self.mini else bool(bg and pending and self.job_ok(b, sp, pending))
                if pending and not carry:
                    red += 2
                if carry:
                    carries.append(b.idx)
                pending = (b.cout * 9 * b.cin, sp)
                continue
            if pending:
                red, pending = red + 2, None
            if not b.has_ds and pair_reduce and self.wgrad(b, 2)[1] > 1:
                red += 1
            else:
                red += sum(self.wgrad(b, w)[1] > 1 for w in ((2, 1, 0) if b.has_ds else (2, 1)))
        return carries, red + (2 if pending else 0)

    def fc_fwd_splits(self):
        tiles, ksteps = K.cdiv(self.B, K.nt_bm(self.B, self.F)) * K.cdiv(self.F, 128), K.cdiv(self.fc_in, 64)
        splits = max(1, min(K.cdiv(512, tiles), ksteps // 4))
        return K.cdiv(ksteps, K.cdiv(ksteps, splits))

    def forward_counts(self):
        """{profile slot: launches} of one training forward: the GEMM slots (< 18) and the slab reductions (25)"""
        out = {}

        def add(s, n=1):
            if n:
                out[s] = out.get(s, 0) + n
        for b in self.blocks:
            add(self.plan(b.hin, b.cin, b.cout, 3, 1, False, K.WANT_STATS)[0])
            add(self.plan(b.hin, b.cout, b.cout, 3, b.stride, False, K.WANT_MOMENTS if self.xmom(b) else K.WANT_STATS)[0])
            if b.has_ds:
                add(self.plan(b.hin, b.cin, b.cout, 1, b.stride, False, K.WANT_STATS)[0])
        ksteps, sp = K.cdiv(self.fc_in, 64), self.fc_fwd_splits()
        add(17 if K.cdiv(ksteps, sp) >= 16 else K.nt_generic_slot(self.B, self.F))
        add(25)
        for s_, k in self.fwd_walk()[0].items():
            add(s_, k)
        return out

    def backward_counts(self, bg=True, pair_reduce=True):
        """{profile slot: launches} of one backward pass: the GEMM slots (< 18) and the stand-alone slab reductions (25)"""
        out = {}

        def add(s, n=1):
            if n:
                out[s] = out.get(s, 0) + n
        Bp = (self.B + 7) // 8 * 8
        add(K.tn_generic_slot(self.F, self.fc_in))
        add(K.tn_generic_slot(Bp, self.fc_in))
        for b in self.blocks:
            add(self.dgrad_slot(b, 2))
            add(self.dgrad_slot(b, 1))
            if self.pair_ok(b):
                add(16)
            else:
                add(self.wgrad(b, 2)[0])
                add(self.wgrad(b, 1)[0])
            if b.has_ds:
                add(self.wgrad(b, 0)[0])
                add(self.plan(b.hin, b.cin, b.cout, 1, b.stride, True, 0)[0])
        add(25, self.wgrad_walk(bg, pair_reduce)[1])
        for s_, k in self.bwd_walk()[0].items():
            add(s_, k)
        return out

    # ------------------------------------------------------------------------ the BatchNorm launches, restated from net.hip (bn_apply_train, bn_bwd)
    @staticmethod
    def apply_grid(M, C):
        return RS.geometry(M, C, RS.APPLY_BLOCKS)["grid"]

    @staticmethod
    def sliced_rows(M, C, backward=False):
        return BS.sliced_geometry(M, C, backward)[0]

    def chain_conv(self, M, rows):
        """statistics / moment rows of a conv epilogue, of its stored output (conv_cases.stats_q): rows_L + 2, + 1 for a staged finalize"""
        return K.rows_L(M, max(rows, 1)) + 2 + 1

    @staticmethod
    def chain_apply_stats(M, C, sliced):
        """statistics rows a forward BatchNorm pass leaves of its stored output: the channel-sliced pass (bn_sliced_cases.FwdCase.stats_q) or the
        row-slab one (rowslab_cases.ApplyCase.chain), + 1 for a staged finalize"""
        if sliced:
            return BS.passes(BS.sliced_geometry(M, C)[1]) + BS.SUM_TREE + 1 + 1
        g = RS.geometry(M, C, RS.APPLY_BLOCKS)
        return g["slab"] // g["rpp"] + g["rpp"] + 2 + 1

    @staticmethod
    def chain_bwd(M, C, kind):
        """BatchNorm-backward sums of a STORED gradient by the pass that forms them: "reduce_s" / "reduce" the channel-sliced / row-slab reduce pass,
        "next_s" / "next" the reduction that rides in the producing channel-sliced / row-slab apply pass; + 1 for the fan-in's store"""
        if kind == "reduce_s":
            return BS.passes(BS.sliced_geometry(M, C, True)[1]) + BS.SUM_TREE + BS.RED_CHAIN_EXTRA + 1
        if kind == "next_s":
            return BS.passes(BS.sliced_geometry(M, C, True)[1]) + BS.SUM_TREE + BS.NEXT_CHAIN_EXTRA + 1
        return colsum_chain(slab_rows(M, C, S.REDUCE_BLOCKS if kind == "reduce" else S.APPLY_BLOCKS), C) + 1

    def fwd_walk(self):
        """net_forward (training): ({profile slot 20 | 23: launches} of the BatchNorm passes — 20 every apply pass, 23 every finalize launch —,
        {BatchNorm prefix: fp32 chain of the statistics its coefficients come from, None where bn_apply2 derives them})"""
        B, n, chain = self.B, {20: 0, 23: 0}, {}

        def train(M, C, P, want_out):
            """bn_apply_train: one channel-sliced launch that reduces the rows itself, else finalize + the row-slab pass -> (rows of y's statistics, sliced)"""
            if BS.sliced_ok(M, C, P, False):
                n[20] += 1
                return (self.sliced_rows(M, C) if want_out else 0), True
            n[23] += 1
            n[20] += 1
            return (self.apply_grid(M, C) if want_out else 0), False
        prevP, prev_sliced = 0, False
        if self.stem:
            M0 = B * self.hin * self.hin
            n[23] += 1
            n[20] += 1
            chain["bn1"] = 64 + 1                                  # stem_cases.StemFwdCase.stats_q: rows of 64 pixels
            prevP = self.apply_grid(M0, 64)
        else:
            prevP = self.apply_grid(B * self.hin * self.hin, self.blocks[0].cin)      # the block test's identity pass
        ready = False
        for b in self.blocks:
            p, Mi, Mo = b.prefix, B * b.hin * b.hin, B * b.hout * b.hout
            if ready:
                chain[p + "bn1"] = None
            else:
                chain[p + "bn1"] = self.chain_apply_stats(Mi, b.cin, prev_sliced)
                train(Mi, b.cin, prevP, False)
            ready = False
            live = self.plan(b.hin, b.cin, b.cout, 3, 1, False, K.WANT_STATS)[2]
            chain[p + "bn2"] = self.chain_conv(Mi, live)
            train(Mi, b.cout, live, False)
            if self.xmom(b):
                part = self.plan(b.hin, b.cout, b.cout, 3, 1, False, K.WANT_MOMENTS)[3]
                chain[p + "bn3"] = self.chain_conv(Mo, part)
                n[20] += 1                                         # bn_apply2: bn3 + identity + the next block's bn1
                ready = True
                continue
            live = self.plan(b.hin, b.cout, b.cout, 3, b.stride, False, K.WANT_STATS)[2]
            chain[p + "bn3"] = self.chain_conv(Mo, live)
            if b.has_ds:
                chain[p + "downsample.1"] = self.chain_conv(Mo, K.nt_stat_rows(Mo, b.cout))
                n[23] += 2
                n[20] += 1
                prevP, prev_sliced = self.apply_grid(Mo, b.cout), False
            else:
                prevP, prev_sliced = train(Mo, b.cout, live, True)
        if self.tail:
            chain["bn2"] = self.chain_apply_stats(B * self.hw, self.C, prev_sliced)
            n[23] += 1
            n[20] += 1
        return n, chain

    def bwd_walk(self):
        """net_backward: ({profile slot 21 | 22 | 24: launches} — 21 every reduce pass, 22 every apply pass, 24 every finalize launch —,
        {BatchNorm prefix: (where its sums come from: "rows" of a dgrad epilogue, "reduce_s" / "reduce" its own pass, "next_s" / "next" carried by the
        apply pass that produced its gradient; rows or 0)})"""
        B, n, src = self.B, {21: 0, 22: 0, 24: 0}, {}

        def bn_bwd(name, M, C, alpha, add, add_up, have, have_kind, next_C, next_alpha=False, coef_only=False):
            """next_C: the channels of the BatchNorm that consumes dx, None where net_backward names none; -> (rows it leaves for it or 0, their kind)"""
            P = have if have > 0 else self.sliced_rows(M, C, True)
            sliced = BS.sliced_ok(M, C, P, True)
            nxt = next_C == C and (not next_alpha or (not alpha and not add and not sliced))
            if not coef_only and not add_up and sliced:
                if have <= 0:
                    n[21] += 1
                src[name] = (have_kind, have) if have > 0 else ("reduce_s", 0)
                n[22] += 1
                return (self.sliced_rows(M, C, True), "next_s") if nxt else (0, None)
            if have <= 0:
                n[21] += 1
            src[name] = (have_kind, have) if have > 0 else ("reduce", 0)
            n[24] += 1
            if not coef_only:
                n[22] += 1
            return (K.cdiv(M, slab_rows(M, C, S.APPLY_BLOCKS)), "next") if nxt else (0, None)
        pend = (0, None)
        if self.tail:
            pend = bn_bwd("bn2", B * self.hw, self.C, False, False, False, 0, None, self.blocks[-1].cout)
        for b in reversed(self.blocks):
            p, Mi, Mo = b.prefix, B * b.hin * b.hin, B * b.hout * b.hout
            bn_bwd(p + "bn3", Mo, b.cout, False, False, False, pend[0], pend[1], None)
            bn_bwd(p + "bn2", Mi, b.cout, True, False, False, self.fused_rows(b, 2), "rows", None)
            if b.has_ds:
                bn_bwd(p + "downsample.1", Mo, b.cout, False, False, False, 0, None, None)
            first = b.idx == 0
            if first and self.mini:
                pend = bn_bwd(p + "bn1", Mi, b.cin, False, not b.has_ds, b.has_ds, self.fused_rows(b, 1), "rows", None)
            else:
                pend = bn_bwd(p + "bn1", Mi, b.cin, False, not b.has_ds, b.has_ds, self.fused_rows(b, 1), "rows", 64 if first else self.blocks[b.idx - 1].cout,
                              next_alpha=first)
        if self.stem:
            bn_bwd("stem", B * self.hin * self.hin, 64, True, False, False, pend[0], pend[1], None, coef_only=True)
        return n, src


def first_batch(pred, limit=300):
    for B in range(1, limit):
        if pred(B):
            return B
    return None


def case_batches():
    """[(layers4, B)] of the GPU test, every batch but the fixed ones computed from the restated thresholds (see tests/test_iresnet_units_gpu.py)"""
    L18 = LAYERS["iresnet18"]
    b56 = first_batch(lambda B: K.conv3x3_slot(B * 3136, 56, 64, 128, stats=True) == 15)             # 56x56 64 -> 128 on the LDS-DMA kernel
    b56s = first_batch(lambda B: not BS.sliced_ok((B + 1) * 3136, 64, 1))                            # the last batch with a sliced 56x56 BatchNorm
    b28 = first_batch(lambda B: K.conv3x3_slot(B * 784, 28, 128, 128, stats=True) == 13)
    b14 = first_batch(lambda B: K.conv3x3_slot(B * 196, 14, 256, 256, stats=True) == 12)
    carry = first_batch(lambda B: bool(Net(CARRY_LAYERS, B).wgrad_walk()[0]))
    out = [(L18, 1), (L18, 5), (L18, b56), (L18, b56 + 1), (L18, b56s), (L18, b28), (L18, b28 + 1), (L18, b14), (L18, 128),
           (CARRY_LAYERS, carry), (CARRY_LAYERS, b14)]
    seen = []
    for c in out:
        if c not in seen:
            seen.append(c)
    return seen


def pair_reduce_case():
    """the first case of case_batches() in which option wgrad_pair_reduce changes the launch sequence: an identity block whose two same-shape weight
    gradients run split-K on a kernel other than the paired one (the 7x7 stage; below that batch its weight gradients are single-split)"""
    for layers, B in case_batches():
        n = Net(layers, B)
        if n.wgrad_walk()[1] != n.wgrad_walk(pair_reduce=False)[1]:
            return layers, B
    return None


# ================================================================================================ references and tolerances
class BnP:
    """per-channel operands of one BatchNorm as stem_cases' formulas read them: gamma, beta and the four saved rows (all float32, on one device)"""

    def __init__(self, gamma, beta, save):
        self.gamma, self.beta = gamma, beta
        self.sc, self.sh, self.mean, self.rstd = save[0], save[1], save[2], save[3]


def ratio_either(got, ref_a, tol_a, ref_b, tol_b, amb):
    """as sphnet_cases.ratio, but where `amb` the smaller of the ratios against (ref_a, tol_a) and (ref_b, tol_b) counts"""
    g = got.to(f64).reshape(ref_a.shape)

    def r(ref, tol):
        e = (g - ref).abs()
        return torch.where(e == 0, torch.zeros_like(e), e / tol)
    ra = r(ref_a, tol_a)
    out = torch.where(amb, torch.minimum(ra, r(ref_b, tol_b)), ra)
    return float(torch.nan_to_num(out, nan=float("inf")).max())


def affine(x16, sc, sh):
    """(z = x sc + sh in float64, |x sc| + |sh|)"""
    x, s, h = x16.to(f64), sc.to(f64), sh.to(f64)
    return x * s + h, (x * s).abs() + h.abs()


def y_tol(y, mag, s16):
    return u16(s16) * y.abs() + RS.K_APPLY * U24 * mag + K.floor16(s16)


def prelu_side(x16, sc, sh, z, mag):
    """(z <= 0 as float32 decides it, the elements whose side the float32 error of the expression leaves open)"""
    x32 = x16.to(f32)
    z32 = S.fma(x32, sc.to(f32), sh.to(f32).expand_as(x32), f32)
    return z32 <= 0, z.abs() <= 3 * U24 * mag


def tensor_stats(x64, chain):
    """column statistics of a stored tensor x [M][C] (float64) and what an fp32 chain of that length leaves of them"""
    M = x64.shape[0]
    S0, S1 = x64.sum(0), (x64 * x64).sum(0)
    mean, e2 = S0 / M, S1 / M
    dm = chain * U24 * x64.abs().sum(0) / M
    return dict(M=M, mean=mean, var=(e2 - mean * mean).clamp_min(0.0), dm=dm, dv=chain * U24 * e2 + 2 * mean.abs() * dm, mag_m=mean.abs(), mag_v=e2 + mean * mean)


def coef_checks(st, gamma, beta, rm0, rv0):
    """{name: (reference, tolerance)} of the four saved rows and the two running statistics for the statistics st (bn_math.h bn_fwd_coef /
    bn_running_update, bn_sliced_cases.fwd_coef's forms): COEF_ULPS 2^-24 of the magnitudes for the fp64 evaluation and the fp32 store, + what the
    bounds (dm, dv) of mean and variance leave of each; rstd over the interval var -+ dv"""
    M, mean, var, dm, dv = st["M"], st["mean"], st["var"], st["dm"], st["dv"]
    f = lambda v: 1.0 / torch.sqrt(v.clamp_min(0.0) + BS.EPSF)  # noqa: E731
    r = f(var)
    dr = torch.maximum((f(var - dv) - r).abs(), (f(var + dv) - r).abs())
    g, b = gamma.to(f64), beta.to(f64)
    sc = g * r
    k = M / (M - 1.0) if M > 1 else 1.0
    m0, v0 = rm0.to(f64), rv0.to(f64)
    return {"mean": (mean, dm + COEF * st["mag_m"]), "rstd": (r, dr + COEF * r), "scale": (sc, g.abs() * dr + COEF * sc.abs()),
            "shift": (b - mean * sc, sc.abs() * dm + mean.abs() * g.abs() * dr + COEF * (b.abs() + st["mag_m"] * sc.abs())),
            "running_mean": ((1.0 - BS.MOM) * m0 + BS.MOM * mean, BS.MOM * dm + COEF * ((1.0 - BS.MOM) * m0.abs() + BS.MOM * st["mag_m"])),
            "running_var": ((1.0 - BS.MOM) * v0 + BS.MOM * var * k, BS.MOM * k * dv + COEF * ((1.0 - BS.MOM) * v0.abs() + BS.MOM * k * st["mag_v"]))}


def derived_stats(c2_64, x64, sc, sh, xsave, xst, chain):
    """the statistics of out = sc c2 + sh + x as bn_apply2 derives them (bn_sliced_cases.Apply2Case.second), held to the float64 statistics of that
    unrounded value: what the fp32 chains of the moment rows (sum c2, sum c2 x, sum c2^2) leave, the bound xst the saved statistics of x (xsave: its
    fp32 mean / rstd rows) were themselves held to and the fp32 store of that rstd, and COEF_ULPS 2^-24 of the magnitudes of the terms that cancel"""
    M = c2_64.shape[0]
    s, h = sc.to(f64), sh.to(f64)
    o = c2_64 * s + h + x64
    mean_o = o.mean(0)
    var_o = ((o - mean_o) ** 2).mean(0)
    cs = tensor_stats(c2_64, chain)
    d_cov = chain * U24 * (c2_64 * x64).abs().sum(0) / M
    mx = xsave[2].to(f64)
    vx = (1.0 / (xsave[3].to(f64) ** 2) - BS.EPSF).clamp_min(0.0)
    # (xst["round_m"], xst["round_v"]: x's saved statistics were themselves derived, of the value BEFORE its 16-bit store, while conv2's moments and
    # this reference read the STORED x — the store moves a column's mean by at most mean(d) and its variance by 2 mean(|x - m| d) + mean(d^2), d the
    # element bound of that store: bn_sliced_cases.Apply2Case.measured)
    dmx = xst["dm"] + COEF * xst["mag_m"] + xst.get("round_m", 0.0)
    dvx = xst["dv"] + 2 * COEF * (vx + BS.EPSF) + xst.get("round_v", 0.0)
    mag_m = (s * cs["mean"]).abs() + h.abs() + mx.abs()
    mag_v = s * s * cs["mag_v"] + vx + 2.0 * s.abs() * ((c2_64 * x64).abs().sum(0) / M + (cs["mean"] * mx).abs())
    dm = s.abs() * cs["dm"] + dmx
    dv = s * s * cs["dv"] + dvx + 2.0 * s.abs() * (d_cov + cs["mean"].abs() * dmx + mx.abs() * cs["dm"]) + COEF * mag_v
    return dict(M=M, mean=mean_o, var=var_o, dm=dm, dv=dv, mag_m=mag_m, mag_v=mag_v)


def bwd_sums(dy64, x16, p, alpha, chain, neg=None, amb=None, e_dy=None):
    """(sum dz | sum dz xhat | sum dy z over z <= 0) of a BatchNorm (+PReLU) backward over dy [M][C] (float64) and their bounds: chain 2^-24 of the
    |terms| in the form the kernels use (conv_cases.bnbwd_rows: rstd (|dz x| + |dz| |mean|), |dy x| |sc| + |dy| |sh|) + COEF_ULPS 2^-24 |value| for the
    fp64 fan-in and the store; + for the elements whose PReLU side is open the difference between the two sides; + with e_dy (the rows were formed
    from an fp32 accumulator within e_dy of dy) what that leaves of each term"""
    x, mu, r = x16.to(f64), p.mean.to(f64), p.rstd.to(f64)
    xh = (x - mu) * r
    zero = torch.zeros_like(dy64)
    if alpha is not None:
        al = alpha.to(f64)
        z, _ = affine(x16, p.sc, p.sh)
        d = torch.where(neg, al.expand_as(dy64), torch.ones_like(dy64))
        t2 = torch.where(neg, dy64 * z, zero)
        m2 = torch.where(neg, (dy64 * x).abs() * p.sc.to(f64).abs() + dy64.abs() * p.sh.to(f64).abs(), zero)
    else:
        d, t2, m2 = torch.ones_like(dy64), zero, zero
    dz = dy64 * d
    val = torch.stack([dz.sum(0), (dz * xh).sum(0), t2.sum(0)])
    mag = torch.stack([dz.abs().sum(0), (((dz * x).abs() + dz.abs() * mu.abs()) * r).sum(0), m2.sum(0)])
    tol = chain * U24 * mag + COEF * val.abs()
    if alpha is not None and bool(amb.any()):
        dd = torch.where(amb, dy64.abs() * (1.0 - al).abs(), zero)
        tol = tol + torch.stack([dd.sum(0), (dd * xh.abs()).sum(0), torch.where(amb, (dy64 * z).abs(), zero).sum(0)])
    if e_dy is not None:
        ed = e_dy * d.abs()
        tol = tol + torch.stack([ed.sum(0), (ed * xh.abs()).sum(0), (torch.where(neg, e_dy * z.abs(), zero).sum(0) if alpha is not None else zero.sum(0))])
    return val, tol


def bwd_dx(dz64, x16, p, S0, S1, M, extra, s16):
    """dx = a dz + A x + B (+ addend) with the coefficients of the STORED fp32 sums (S0 = dbeta, S1 = dgamma): stem_cases.bn_coef / bn_dx; dx_q
    (unconditioned) + bn_coef_tol for one unit in the last place of each stored sum"""
    c64 = S.bn_coef(S0, S1, p, float(M))
    o, mag = S.bn_dx(c64.to(f32), dz64, x16, f64, extra)
    tc = S.bn_coef_tol(c64, U24 * S0.to(f64).abs(), U24 * S1.to(f64).abs(), p, float(M))
    return o, u16(s16) * o.abs() + 2.0 ** -22 * mag + K.floor16(s16) + tc[0] * dz64.abs() + tc[1] * x16.to(f64).abs() + tc[2]


def upsample(dxd64, B, H, C):
    """the compact [B][H/2][H/2][C] dgrad of the stride-2 1x1 downsample conv at the even pixels of the H x H map (bn_bwd_apply's add_up)"""
    e = torch.zeros(B, H, H, C, dtype=f64, device=dxd64.device)
    e[:, ::2, ::2] = dxd64.reshape(B, H // 2, H // 2, C)
    return e.reshape(-1, C)


def compare(net, T, s16, dev, got=None, info=None):
    """yields (what, error / tolerance) for every comparison of the plan's stored tensors T (module docstring), every element of every tensor included.
    T: x (fp32 NCHW), par / grad {state_dict name: fp32 tensor, conv weights KRSC}, buf0 / buf {BatchNorm prefix: (running_mean, running_var)} before /
    after the forward pass, save {BatchNorm prefix: [4][C]}, blk [per block {x, a1, c1, a2, c2, d, out}: 16-bit NHWC], cap [per block {g, dc2, da2, dc1,
    dd, dxd, da1}], gin0 (the gradient wrt the first block's input); with a stem c0, a0; with a tail t ([B][fc_in]), yfc, fsave ([2][F]: the features'
    mean, rstd), feats, dfeats, gt (the captured gradient wrt the network's bn2 output, NHWC).  got: the same keys, checked
    INSTEAD of T's against references that are still fed from T.  info (optional dict): "ambiguous" counts the elements whose PReLU side was open"""
    B = net.B
    X = T if got is None else got
    D = lambda t: t.to(dev)  # noqa: E731
    d64 = lambda t: t.to(dev, f64)  # noqa: E731
    info = {} if info is None else info
    info.setdefault("ambiguous", 0)
    fchain, bsrc = net.fwd_walk()[1], net.bwd_walk()[1]      # the fp32 chain of every BatchNorm's sums, of the kernel the restated dispatch selects

    def bch(name, M, C):
        kind, rows = bsrc[name]
        return K.rows_L(M, rows) + 4 + 1 if kind == "rows" else net.chain_bwd(M, C, kind)
    stats_of = {}                                            # BatchNorm prefix -> the statistics record its coefficients were held to

    def bn_forward(name, st):
        stats_of[name] = st
        g, b = D(T["par"][name + ".weight"]), D(T["par"][name + ".bias"])
        chk = coef_checks(st, g, b, D(T["buf0"][name][0]), D(T["buf0"][name][1]))
        for i, k in enumerate(("scale", "shift", "mean", "rstd")):
            yield "%s %s" % (name, k), ratio(D(X["save"][name][i]), *chk[k])
        for i, k in enumerate(("running_mean", "running_var")):
            yield "%s %s" % (name, k), ratio(D(X["buf"][name][i]), *chk[k])

    def bnp(name):
        return BnP(D(T["par"][name + ".weight"]), D(T["par"][name + ".bias"]), D(T["save"][name]))

    def prelu_y(x16, p, alpha):
        """prelu(x sc + sh): both sides' (value, tolerance) and the open elements"""
        z, mag = affine(x16, p.sc, p.sh)
        neg, amb = prelu_side(x16, p.sc, p.sh, z, mag)
        al = alpha.to(f64)
        ya, yb = torch.where(neg, al * z, z), torch.where(neg, z, al * z)
        info["ambiguous"] += int(amb.sum())
        return ya, y_tol(ya, mag, s16), yb, y_tol(yb, mag, s16), amb

    # ---------------------------------------------------------------- forward: stem
    if "c0" in T:
        xr, wr = D(T["x"]).to(s16).to(f64), D(T["par"]["conv1.weight"]).to(s16).to(f64)
        y = S.stem_taps(xr) @ wr.reshape(64, 27).t()
        yield "c0", ratio(D(X["c0"]), y.reshape(T["c0"].shape), ((u16(s16) + 2.0 ** -20) * y.abs().amax(1, keepdim=True) + K.floor16(s16)).expand_as(y).reshape(T["c0"].shape))
        del xr, y
        c0 = D(T["c0"]).reshape(-1, 64)
        yield from bn_forward("bn1", tensor_stats(c0.to(f64), 64 + 1))                # stem_cases.StemFwdCase.stats_q: rows of 64 pixels
        ya, ta, yb, tb, amb = prelu_y(c0, bnp("bn1"), D(T["par"]["prelu.weight"]))
        yield "a0", ratio_either(D(X["a0"]).reshape(-1, 64), ya, ta, yb, tb, amb)
        del c0, ya, ta, yb, tb, amb
    # ---------------------------------------------------------------- forward, block by block
    derived = None                                           # the statistics record of this block's bn1 where the previous block derived it (fwd_xmom)
    for b in net.blocks:
        t, p = T["blk"][b.idx], b.prefix
        Mi, Mo = B * b.hin * b.hin, B * b.hout * b.hout
        tag = "[%d]" % b.idx
        x = D(t["x"]).reshape(Mi, b.cin)
        yield from bn_forward(p + "bn1", derived if derived is not None else tensor_stats(x.to(f64), fchain[p + "bn1"]))
        p1 = bnp(p + "bn1")
        z, mag = affine(x, p1.sc, p1.sh)
        yield "a1" + tag, ratio(D(X["blk"][b.idx]["a1"]).reshape(Mi, b.cin), z, y_tol(z, mag, s16))
        del z, mag
        w1 = D(T["par"][p + "conv1.weight"]).to(s16)
        r = K.conv_ref(D(t["a1"]), w1, 1, f64, dev, want=("y",))
        yield "c1" + tag, ratio(D(X["blk"][b.idx]["c1"]), r["y"], out16_tol(r["y"], r["Sy"], 9 * b.cin, s16))
        del r
        c1 = D(t["c1"]).reshape(Mi, b.cout)
        live = net.plan(b.hin, b.cin, b.cout, 3, 1, False, K.WANT_STATS)[2]
        yield from bn_forward(p + "bn2", tensor_stats(c1.to(f64), fchain[p + "bn2"]))
        ya, ta, yb, tb, amb = prelu_y(c1, bnp(p + "bn2"), D(T["par"][p + "prelu.weight"]))
        yield "a2" + tag, ratio_either(D(X["blk"][b.idx]["a2"]).reshape(Mi, b.cout), ya, ta, yb, tb, amb)
        del c1, ya, ta, yb, tb, amb
        w2 = D(T["par"][p + "conv2.weight"]).to(s16)
        r = K.conv_ref(D(t["a2"]), w2, b.stride, f64, dev, want=("y",))
        yield "c2" + tag, ratio(D(X["blk"][b.idx]["c2"]), r["y"], out16_tol(r["y"], r["Sy"], 9 * b.cout, s16))
        del r
        c2 = D(t["c2"]).reshape(Mo, b.cout)
        xm = net.xmom(b)
        pl = net.plan(b.hin, b.cout, b.cout, 3, b.stride, False, K.WANT_MOMENTS if xm else K.WANT_STATS)
        ch2 = fchain[p + "bn3"]
        yield from bn_forward(p + "bn3", tensor_stats(c2.to(f64), ch2))
        p3 = bnp(p + "bn3")
        z, mag = affine(c2, p3.sc, p3.sh)
        if b.has_ds:
            wd = D(T["par"][p + "downsample.0.weight"]).to(s16)
            r = K.conv_ref(D(t["x"]), wd, b.stride, f64, dev, want=("y",))
            yield "d" + tag, ratio(D(X["blk"][b.idx]["d"]), r["y"], out16_tol(r["y"], r["Sy"], b.cin, s16))
            del r
            d = D(t["d"]).reshape(Mo, b.cout)
            yield from bn_forward(p + "downsample.1", tensor_stats(d.to(f64), fchain[p + "downsample.1"]))
            pd = bnp(p + "downsample.1")
            z2, mag2 = affine(d, pd.sc, pd.sh)
            z, mag = z + z2, mag + mag2
            del d, z2, mag2
        else:
            z, mag = z + x.to(f64), mag + x.to(f64).abs()
        tol_o = y_tol(z, mag, s16)
        yield "out" + tag, ratio(D(X["blk"][b.idx]["out"]).reshape(Mo, b.cout), z, tol_o)
        derived = None
        if xm:
            derived = derived_stats(c2.to(f64), x.to(f64), p3.sc, p3.sh, D(T["save"][p + "bn1"]), stats_of[p + "bn1"], ch2)
            derived["round_m"] = tol_o.mean(0)
            derived["round_v"] = 2.0 * ((z - z.mean(0)).abs() * tol_o).mean(0) + (tol_o * tol_o).mean(0)
        del z, mag, tol_o
        del c2, x
    # ---------------------------------------------------------------- forward: tail
    last = net.blocks[-1]
    if "t" in T:
        Mf = B * net.hw
        o = D(T["blk"][last.idx]["out"]).reshape(Mf, net.C)
        yield from bn_forward("bn2", derived if derived is not None else tensor_stats(o.to(f64), fchain["bn2"]))
        pt = bnp("bn2")
        z, mag = affine(o, pt.sc, pt.sh)
        yield "t", ratio(D(X["t"]), RS.nchw(z, net.hw).reshape(B, net.fc_in), RS.nchw(y_tol(z, mag, s16), net.hw).reshape(B, net.fc_in))
        del o, z, mag
        flat, fw, fb = d64(T["t"]).reshape(B, net.fc_in), d64(D(T["par"]["fc.weight"]).to(s16)), d64(T["par"]["fc.bias"])
        sp = net.fc_fwd_splits()
        yield "yfc", ratio(D(X["yfc"]), flat @ fw.t() + fb, (K.cdiv(net.fc_in, sp) + 64 + sp + 2) * U24 * (flat.abs() @ fw.abs().t() + fb.abs()))
        # features: BatchNorm1d of the STORED fc output; its saved (mean, rstd) rows, running statistics and feats = (y - mean) rstd gamma + beta with
        # the stored rows (ew.hip bn1d: float64 sums, fp32 rows, the affine in fp32: five roundings of (|y| + |mean|) rstd |gamma| + |beta|)
        y = d64(T["yfc"])
        Fg, Fb = d64(T["par"]["features.weight"]), d64(T["par"]["features.bias"])
        mu = y.mean(0)
        var = ((y - mu) ** 2).mean(0)
        rs = 1.0 / torch.sqrt(var + BS.EPSF)
        m_abs = y.abs().mean(0)
        yield "features mean", ratio(D(X["fsave"][0]), mu, COEF * m_abs)
        yield "features rstd", ratio(D(X["fsave"][1]), rs, COEF * rs * (1.0 + (y * y).mean(0) * rs * rs))
        kB = B / (B - 1.0) if B > 1 else 1.0
        m0, v0 = d64(T["buf0"]["features"][0]), d64(T["buf0"]["features"][1])
        yield "features running_mean", ratio(D(X["buf"]["features"][0]), (1.0 - BS.MOM) * m0 + BS.MOM * mu, COEF * ((1.0 - BS.MOM) * m0.abs() + BS.MOM * m_abs))
        yield "features running_var", ratio(D(X["buf"]["features"][1]), (1.0 - BS.MOM) * v0 + BS.MOM * var * kB,
                                            COEF * ((1.0 - BS.MOM) * v0.abs() + BS.MOM * kB * ((y * y).mean(0) + mu * mu)))
        smu, srs = d64(T["fsave"][0]), d64(T["fsave"][1])
        yield "feats", ratio(D(X["feats"]), (y - smu) * srs * Fg + Fb, 5 * U24 * ((y.abs() + smu.abs()) * srs * Fg.abs() + Fb.abs()))
        del y, flat, fw, fb
    # ---------------------------------------------------------------- backward: features, fc, the network's bn2
    if "t" in T:
        Mf = B * net.hw
        y, dfe = d64(T["yfc"]), d64(T["dfeats"])
        Fg, smu, srs = d64(T["par"]["features.weight"]), d64(T["fsave"][0]), d64(T["fsave"][1])
        xh = (y - smu) * srs
        S1, S2 = dfe.sum(0), (dfe * xh).sum(0)
        yield "features dbeta", ratio(D(X["grad"]["features.bias"]), S1, COEF * dfe.abs().sum(0))
        # d(fc output) = gamma rstd (dfeats - S1 / B - xhat S2 / B), formed in fp32 and never stored in fp32: e_d bounds its evaluation (8 roundings of the terms)
        dy = Fg * srs * (dfe - S1 / B - xh * S2 / B)
        e_d = 8 * U24 * (Fg * srs).abs() * (dfe.abs() + S1.abs() / B + xh.abs() * S2.abs() / B)
        yield "fc.bias grad", ratio(D(X["grad"]["fc.bias"]), dy.sum(0), e_d.sum(0) + COEF * dy.abs().sum(0))
        # fc.weight grad = round16(dy)^T t and the input gradient round16(round16(dy) W): the operand's own 16-bit rounding is hidden -> the double-rounding
        # bound, u16 |dy| + e_d through the other operand, on top of the GEMM's
        e16 = u16(s16) * dy.abs() + e_d + K.floor16(s16)
        flat, fw = d64(T["t"]).reshape(B, net.fc_in), d64(D(T["par"]["fc.weight"]).to(s16))
        yield "fc.weight grad", ratio(D(X["grad"]["fc.weight"]), dy.t() @ flat, (B + 3) * U24 * (dy.abs().t() @ flat.abs()) + e16.t() @ flat.abs())
        nhwc = lambda v: v.reshape(B, net.C, net.hw).permute(0, 2, 1).reshape(Mf, net.C)  # noqa: E731
        ref, Sx = dy @ fw, dy.abs() @ fw.abs()
        yield "gt", ratio(D(X["gt"]).reshape(Mf, net.C), nhwc(ref), nhwc(out16_tol(ref, Sx, net.F, s16) + e16 @ fw.abs()))
        del flat, fw, ref, Sx, dy, e_d, e16, y, dfe, xh
        # the network's bn2: sums of the STORED gt, the gradient entering the last block
        pt, o, gt = bnp("bn2"), D(T["blk"][last.idx]["out"]).reshape(Mf, net.C), d64(T["gt"]).reshape(Mf, net.C)
        val, tol = bwd_sums(gt, o, pt, None, bch("bn2", Mf, net.C))
        yield "bn2 dbeta", ratio(D(X["grad"]["bn2.bias"]), val[0], tol[0])
        yield "bn2 dgamma", ratio(D(X["grad"]["bn2.weight"]), val[1], tol[1])
        ref, tol = bwd_dx(gt, o, pt, D(T["grad"]["bn2.bias"]), D(T["grad"]["bn2.weight"]), Mf, None, s16)
        yield "g[%d]" % last.idx, ratio(D(X["cap"][last.idx]["g"]).reshape(Mf, net.C), ref, tol)
        del o, gt, ref, tol
    # ---------------------------------------------------------------- backward, block by block (last block first)
    for b in reversed(net.blocks):
        t, c, p = T["blk"][b.idx], T["cap"][b.idx], b.prefix
        G = lambda n: D(X["grad"][n])  # noqa: E731
        Mi, Mo = B * b.hin * b.hin, B * b.hout * b.hout
        tag = "[%d]" % b.idx
        g = d64(c["g"]).reshape(Mo, b.cout)
        # out = bn3(c2) + identity: dc2
        p3, c2 = bnp(p + "bn3"), D(t["c2"]).reshape(Mo, b.cout)
        val, tol = bwd_sums(g, c2, p3, None, bch(p + "bn3", Mo, b.cout))
        yield p + "bn3 dbeta", ratio(G(p + "bn3.bias"), val[0], tol[0])
        yield p + "bn3 dgamma", ratio(G(p + "bn3.weight"), val[1], tol[1])
        o, tol = bwd_dx(g, c2, p3, D(T["grad"][p + "bn3.bias"]), D(T["grad"][p + "bn3.weight"]), Mo, None, s16)
        yield "dc2" + tag, ratio(D(X["cap"][b.idx]["dc2"]).reshape(Mo, b.cout), o, tol)
        del c2, o, tol
        # conv2's dgrad: da2, its weight gradient
        w2 = D(T["par"][p + "conv2.weight"]).to(s16)
        r = K.conv_ref(D(t["a2"]), w2, b.stride, f64, dev, dy=D(c["dc2"]), want=("dx", "dw"))
        e_da2 = out16_tol(r["dx"], r["Sdx"], 9 * b.cout, s16)
        yield "da2" + tag, ratio(D(X["cap"][b.idx]["da2"]), r["dx"], e_da2)
        yield p + "conv2 dw", ratio(G(p + "conv2.weight"), r["dw"], dw_chain(Mo, net.wgrad(b, 2)[1]) * U24 * r["Sdw"])
        da2_ref, e_acc = r["dx"].reshape(Mi, b.cout), ((9 * b.cout + 2) * U24 * r["Sdx"]).reshape(Mi, b.cout)
        del r, e_da2
        # a2 = prelu(bn2(c1)): dc1
        p2, c1, al = bnp(p + "bn2"), D(t["c1"]).reshape(Mi, b.cout), D(T["par"][p + "prelu.weight"])
        z, mag = affine(c1, p2.sc, p2.sh)
        neg, amb = prelu_side(c1, p2.sc, p2.sh, z, mag)
        del z, mag
        f2 = net.fused_rows(b, 2)
        if f2:                                                # rows of the dgrad epilogue's fp32 accumulator
            val, tol = bwd_sums(da2_ref, c1, p2, al, bch(p + "bn2", Mi, b.cout), neg, amb, e_acc)
        else:
            val, tol = bwd_sums(d64(c["da2"]).reshape(Mi, b.cout), c1, p2, al, bch(p + "bn2", Mi, b.cout), neg, amb)
        del da2_ref, e_acc
        yield p + "bn2 dbeta", ratio(G(p + "bn2.bias"), val[0], tol[0])
        yield p + "bn2 dgamma", ratio(G(p + "bn2.weight"), val[1], tol[1])
        yield p + "prelu dalpha", ratio(G(p + "prelu.weight"), val[2], tol[2])
        da2 = d64(c["da2"]).reshape(Mi, b.cout)
        S0, S1 = D(T["grad"][p + "bn2.bias"]), D(T["grad"][p + "bn2.weight"])
        a64 = al.to(f64).expand_as(da2)
        oa, ta = bwd_dx(torch.where(neg, da2 * a64, da2), c1, p2, S0, S1, Mi, None, s16)
        ob, tb = bwd_dx(torch.where(neg, da2, da2 * a64), c1, p2, S0, S1, Mi, None, s16)
        yield "dc1" + tag, ratio_either(D(X["cap"][b.idx]["dc1"]).reshape(Mi, b.cout), oa, ta, ob, tb, amb)
        del da2, a64, oa, ta, ob, tb, c1, neg, amb
        # the downsample path: dd, dxd, its weight gradient
        extra = g if not b.has_ds else None
        if b.has_ds:
            pd, d = bnp(p + "downsample.1"), D(t["d"]).reshape(Mo, b.cout)
            val, tol = bwd_sums(g, d, pd, None, bch(p + "downsample.1", Mo, b.cout))
            yield p + "downsample.1 dbeta", ratio(G(p + "downsample.1.bias"), val[0], tol[0])
            yield p + "downsample.1 dgamma", ratio(G(p + "downsample.1.weight"), val[1], tol[1])
            o, tol = bwd_dx(g, d, pd, D(T["grad"][p + "downsample.1.bias"]), D(T["grad"][p + "downsample.1.weight"]), Mo, None, s16)
            yield "dd" + tag, ratio(D(X["cap"][b.idx]["dd"]).reshape(Mo, b.cout), o, tol)
            del d, o, tol
            wd = D(T["par"][p + "downsample.0.weight"]).to(s16)
            r = K.conv_ref(D(t["x"]), wd, b.stride, f64, dev, dy=D(c["dd"]), want=("dw",))
            yield p + "downsample.0 dw", ratio(G(p + "downsample.0.weight"), r["dw"], dw_chain(Mo, net.wgrad(b, 0)[1]) * U24 * r["Sdw"])
            del r
            dd, wm = d64(c["dd"]).reshape(Mo, b.cout), wd.to(f64).reshape(b.cout, b.cin)
            ref, Sd = dd @ wm, dd.abs() @ wm.abs()
            yield "dxd" + tag, ratio(D(X["cap"][b.idx]["dxd"]).reshape(Mo, b.cin), ref, out16_tol(ref, Sd, b.cout, s16))
            del dd, ref, Sd
            extra = upsample(d64(c["dxd"]), B, b.hin, b.cin)
        # conv1's dgrad: da1, its weight gradient
        w1 = D(T["par"][p + "conv1.weight"]).to(s16)
        r = K.conv_ref(D(t["a1"]), w1, 1, f64, dev, dy=D(c["dc1"]), want=("dx", "dw"))
        yield "da1" + tag, ratio(D(X["cap"][b.idx]["da1"]), r["dx"], out16_tol(r["dx"], r["Sdx"], 9 * b.cout, s16))
        yield p + "conv1 dw", ratio(G(p + "conv1.weight"), r["dw"], dw_chain(Mi, net.wgrad(b, 1)[1]) * U24 * r["Sdw"])
        da1_ref, e_acc = r["dx"].reshape(Mi, b.cin), ((9 * b.cout + 2) * U24 * r["Sdx"]).reshape(Mi, b.cin)
        del r
        # a1 = bn1(x): the gradient leaving the block
        p1, x = bnp(p + "bn1"), D(t["x"]).reshape(Mi, b.cin)
        f1 = net.fused_rows(b, 1)
        if f1:
            val, tol = bwd_sums(da1_ref, x, p1, None, bch(p + "bn1", Mi, b.cin), e_dy=e_acc)
        else:
            val, tol = bwd_sums(d64(c["da1"]).reshape(Mi, b.cin), x, p1, None, bch(p + "bn1", Mi, b.cin))
        del da1_ref, e_acc
        yield p + "bn1 dbeta", ratio(G(p + "bn1.bias"), val[0], tol[0])
        yield p + "bn1 dgamma", ratio(G(p + "bn1.weight"), val[1], tol[1])
        o, tol = bwd_dx(d64(c["da1"]).reshape(Mi, b.cin), x, p1, D(T["grad"][p + "bn1.bias"]), D(T["grad"][p + "bn1.weight"]), Mi, extra, s16)
        leaving = X["cap"][b.idx - 1]["g"] if b.idx > 0 else X["gin0"]
        yield "gin" + tag, ratio(D(leaving).reshape(Mi, b.cin), o, tol)
        del o, tol, x, g, extra
    # ---------------------------------------------------------------- backward: stem
    if "c0" in T:
        M0 = B * net.hin * net.hin
        ps, c0, al = bnp("bn1"), D(T["c0"]).reshape(M0, 64), D(T["par"]["prelu.weight"])
        g0 = d64(T["gin0"]).reshape(M0, 64)
        z, mag = affine(c0, ps.sc, ps.sh)
        neg, amb = prelu_side(c0, ps.sc, ps.sh, z, mag)
        del z, mag
        val, tol = bwd_sums(g0, c0, ps, al, bch("stem", M0, 64), neg, amb)       # reduced from the STORED gradient (stem_cases.BnBwdCase.next_sums_q)
        yield "bn1 dbeta", ratio(D(X["grad"]["bn1.bias"]), val[0], tol[0])
        yield "bn1 dgamma", ratio(D(X["grad"]["bn1.weight"]), val[1], tol[1])
        yield "prelu dalpha", ratio(D(X["grad"]["prelu.weight"]), val[2], tol[2])
        # the weight gradient applies the backward to its operand tile: dz0 is never stored (tests/test_stem_chain_gpu.py, the chain as a unit)
        S0, S1 = D(T["grad"]["bn1.bias"]), D(T["grad"]["bn1.weight"])
        c64 = S.bn_coef(S0, S1, ps, float(M0))
        dzn = torch.where(neg, g0 * al.to(f64), g0)
        dz0, mag = S.bn_dx(c64.to(f32), dzn, c0, f64)
        tc = S.bn_coef_tol(c64, U24 * S0.to(f64).abs(), U24 * S1.to(f64).abs(), ps, float(M0))
        ddz = tc[0] * dzn.abs() + tc[1] * c0.to(f64).abs() + tc[2] + 2.0 ** -22 * mag
        ddz = ddz + torch.where(amb, g0.abs() * (1.0 - al.to(f64)).abs() * c64[0].abs(), torch.zeros_like(ddz))
        del dzn, mag, g0, neg, amb
        col = S.stem_taps(D(T["x"]).to(f64))
        ppb = S.stem_px_per_block(M0)
        L = (ppb // 128) * 4 + K.cdiv(M0, ppb)
        ad, ac = dz0.abs(), col.abs()
        tol = (2.0 ** -17 + L * U24 + u16(s16)) * (ad.t() @ ac) + ddz.t() @ ac
        yield "conv1 dw", ratio(D(X["grad"]["conv1.weight"]).reshape(64, 27), dz0.t() @ col, tol)
