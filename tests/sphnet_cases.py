"""Unit table, dispatch predictions, fp64 references and tolerances for the unit-by-unit tests of the sphnet plan (csrc/net_sph.inc), in the manner
of conv_cases.py and rowslab_cases.py, whose functions are used, not copied.  Nothing here touches the GPU library or imports the oracle.

A sphnet is a list of UNITS in forward order (per stage: the stride-2 stage head, then u1, u2 of every residual block); a unit is conv3x3 (+ bias
on the heads) -> PReLU, u2 adds the block's input.  `compare` walks that list and holds every tensor one pass leaves behind to a float64 reference
that is fed with the pass's own STORED operands (the 16-bit inputs, conv outputs, activations, dz tensors and captured gradients of the run under
test), so nothing compounds from unit to unit and no PReLU-kink flip can occur: the PReLU side of every element is taken from the stored conv
output, z = float32(c) + bias evaluated in fp32 exactly as the kernels do, z <= 0 counting as the negative side (the rule of rowslab_cases.PreluCase
and conv_cases.papply_ref).  Because of that no element of any tensor is excluded from any comparison.

Every tolerance is element-wise and a formula of u16 (2^-11 fp16 / 2^-8 bf16), 2^-24, a chain length and S = sum |terms|, with fp16's 2^-25
subnormal spacing (conv_cases.floor16) wherever a 16-bit store is involved; none is a measured number:
  16-bit conv / dgrad output   conv_cases.out16_q: u16 |ref| + (K + 2) 2^-24 S, + floor16
  activation t                 rowslab_cases.ApplyCase.y_q: u16 |y| + K_APPLY 2^-24 (|c| + |bias| + |identity|), + floor16
  feats, fc gradients          the form of conv_cases.dw_q for fp32 results of 16-bit products, with the per-split chain of dw_chain
  dz of a PReLU pass           rowslab_cases.PreluCase.dz_q: (u16 + 2 2^-24) |dz|, + floor16
  dz of u1                     TWO paths, one bound (dz_u1_tol): the dgrad epilogue multiplies its fp32 accumulator and rounds once; the
                               unfused path stores dt1 in 16 bits and the PReLU pass multiplies and rounds again — the double-rounding bound
  gradient entering a block    TWO roundings always (gsum_tol): da = round16(dgrad) is stored, then round16(g + da) by the PReLU pass
  weight gradients             conv_cases.dw_q's form with the split count the restated dispatch gives and the chain of ONE split (dw_chain)
  dbias / dalpha               chain 2^-24 sum |terms| for the partial rows (chain = stem_cases.colsum_chain of the pass's slab, or the rows_L of
                               conv_cases.papply_q where the dgrad epilogue formed them) + rowslab_cases.prelu_fin_q's finalize; for u1, whose
                               incoming gradient the unfused path has rounded to 16 bits before summing, + sum (that rounding |factor|)
"""
import torch

import conv_cases as K
import rowslab_cases as RS
from stem_cases import U24, colsum_chain, f32, f64, slab_rows, u16  # noqa: F401

LAYERS = {20: (1, 2, 4, 1), 64: (3, 7, 16, 3)}
FILTERS = (3, 64, 128, 256, 512)
U53 = 2.0 ** -53


# ================================================================================================ the unit table
class Unit:
    """one conv3x3 (+bias) -> PReLU unit.  cin is the stored width (the stem's 3 channels are padded to 64), ident the index of the unit whose
    INPUT is added behind the PReLU (u2: its block's u1), or None"""

    def __init__(self, idx, stage, kind, conv, prelu, cin_real, cout, stride, hin, bias, ident):
        self.idx, self.stage, self.kind, self.conv, self.prelu = idx, stage, kind, conv, prelu
        self.cin_real, self.cin, self.cout, self.stride, self.hin, self.hout = cin_real, max(cin_real, 64), cout, stride, hin, hin // stride
        self.bias, self.ident = bias, ident

    def names(self):
        """(name, shape) of the unit's state_dict entries, in order"""
        out = [(self.conv + ".weight", (self.cout, self.cin_real, 3, 3))]
        if self.bias:
            out.append((self.conv + ".bias", (self.cout,)))
        return out + [(self.prelu + ".weight", (self.cout,))]


def build_units(layers, filters, hin):
    """net_create_sphere's module walk: per stage `layer{s}.0` / `.1` (head conv / PReLU), then blocks `layer{s}.{i + 2}.conv1 | prelu1 | conv2 | prelu2`"""
    out = []
    for s, L in enumerate(layers):
        p = "layer%d." % (s + 1)
        out.append(Unit(len(out), s, "head", p + "0", p + "1", filters[s], filters[s + 1], 2, hin, True, None))
        hin //= 2
        for i in range(L):
            b = p + "%d." % (i + 2)
            out.append(Unit(len(out), s, "u1", b + "conv1", b + "prelu1", filters[s + 1], filters[s + 1], 1, hin, False, None))
            out.append(Unit(len(out), s, "u2", b + "conv2", b + "prelu2", filters[s + 1], filters[s + 1], 1, hin, False, len(out) - 1))
    return out


class Net:
    """a sphnet (type 20 / 64 at batch B), or with `mini` a miniature stack of the same wiring: (layers, filters, input side, features)"""

    def __init__(self, type_, B, mini=None, cus=256):
        self.type, self.B, self.cus = type_, B, cus
        layers, filters, hin, self.F = mini if mini else (LAYERS[type_], FILTERS, 112, 512)
        self.hin, self.mini = hin, mini is not None
        self.units = build_units(layers, filters, hin)
        last = self.units[-1]
        self.hw, self.C = last.hout * last.hout, last.cout
        self.fc_in = self.hw * self.C
        self.mini_splits, self.mini_fused = 2, False

    def tensor_names(self):
        out = []
        for u in self.units:
            out += u.names()
        return out + [("fc.weight", (self.F, self.fc_in)), ("fc.bias", (self.F,))]

    def captured(self):
        """the units whose incoming gradient sph_backward captures, in capture (= backward) order"""
        return [u for u in reversed(self.units) if u.kind != "u1"]

    # ---- dispatch, restated from csrc (gemm.hip gemm_nt_launch_one / gemm_tn_launch, net.hip conv_wgrad2, net_sph.inc)
    def fwd_slot(self, u):
        M = self.B * u.hout * u.hout
        if u.stride == 1:
            return K.conv3x3_slot(M, u.hin, u.cin, u.cout)
        return 17 if K.nt_glds_applies(u.cout, 9 * u.cin) else K.nt_generic_slot(M, u.cout)

    def prelu_rows(self, u):
        """ew_prelu_bwd_rows(M, C) = ceil(M / slab_rows(M, C, 512))"""
        return RS.geometry(self.B * u.hout * u.hout, u.cout, RS.PRELU_BLOCKS)["grid"]

    def dgrad_prelu_ok(self, u2):
        """net_sph.inc dgrad_prelu_ok: conv2's dgrad applies the backward of u1's PReLU in its epilogue — channel counts multiples of 128, the
        LDS-DMA kernel with the epilogue serves the shape, and u1's row buffer ([rows][2][C]) holds the epilogue's [tiles][3][C] rows"""
        if self.mini:
            return self.mini_fused
        u1 = self.units[u2.idx - 1]
        M = self.B * u2.hin * u2.hin
        if u2.stride != 1 or u2.cin % 128 or u2.cout % 128 or not K.conv_epilogue_ok(u2.hin, u2.cout, u2.cin, M, 3, 1):
            return False
        if u2.hin not in (14, 28) or (u2.hin == 28 and (M // 196) % 2):
            return False
        return K.fused_rows(M, u2.hin) * 3 <= self.prelu_rows(u1) * 2

    def dgrad_slot(self, u):
        """the dgrad of unit u's conv (None: the stem's is never formed)"""
        if u.idx == 0:
            return None
        if u.stride == 1:
            return K.conv3x3_slot(self.B * u.hin * u.hin, u.hin, u.cout, u.cin, fused=u.kind == "u2" and self.dgrad_prelu_ok(u))
        return K.nt_generic_slot(self.B * u.hin * u.hin // 4, u.cin)          # stride 2: the four output-parity classes in one launch

    def pair_ok(self, u):
        """wgrad9p.hip wgrad9p_applies for a block's two same-shape weight gradients"""
        return K.wgrad9_shape_ok(self.B * u.hout * u.hout, u.cout, 9 * u.cin, u.cin, u.hout, u.stride) and u.cout % 64 == 0

    def wgrad_slot_splits(self, u):
        if self.mini:
            return None, self.mini_splits
        if u.kind != "head" and self.pair_ok(u):
            return 16, K.wgrad9p_pick_splits(self.B * u.hout * u.hout, u.cout, 9 * u.cin, u.hout)
        return K.wgrad_slot_splits(self.B, u.hin, u.cin, u.cout, 3, u.stride)

    def fc_fwd_splits(self):
        """gemm.hip gemm_nt_pick_splits(B, F, fc_in)"""
        tiles, ksteps = K.cdiv(self.B, K.nt_bm(self.B, self.F)) * K.cdiv(self.F, 128), K.cdiv(self.fc_in, 64)
        splits = max(1, min(K.cdiv(512, tiles), ksteps // 4))
        return K.cdiv(ksteps, K.cdiv(ksteps, splits))

    def forward_counts(self):
        """{profile slot: launches} of one forward pass"""
        out = {}
        for u in self.units:
            s = self.fwd_slot(u)
            out[s] = out.get(s, 0) + 1
        ksteps, sp = K.cdiv(self.fc_in, 64), self.fc_fwd_splits()
        s = 17 if K.cdiv(ksteps, sp) >= 16 else K.nt_generic_slot(self.B, self.F)     # gemm_nt_glds_applies with `splits` splits; mode 0: no conv kernel
        out[s] = out.get(s, 0) + 1
        return out

    def backward_counts(self):
        """({profile slot: launches} of one backward pass, blocks served by the fused PReLU-backward epilogue, blocks on the paired kernel)"""
        out, fused, paired = {}, 0, 0

        def add(s, n=1):
            out[s] = out.get(s, 0) + n
        Bp = (self.B + 7) // 8 * 8
        add(K.tn_generic_slot(self.F, self.fc_in))              # fc dW: mode 0, Kp = B
        add(K.tn_generic_slot(Bp, self.fc_in))                  # fc dx: NI = Bp
        for u in self.units:
            d = self.dgrad_slot(u)
            if d is not None:
                add(d)
            if u.kind == "u2":
                fused += bool(self.dgrad_prelu_ok(u))
                if self.pair_ok(u):
                    paired += 1
                    add(16)                                     # one launch for u1 and u2
                else:
                    add(self.wgrad_slot_splits(u)[0], 2)
            elif u.kind == "head":
                add(self.wgrad_slot_splits(u)[0])
        return out, fused, paired


def first_fused_batch(type_, stage, limit=512):
    """the smallest batch at which every block of `stage` has its PReLU backward in the dgrad epilogue"""
    for B in range(1, limit):
        n = Net(type_, B)
        if all(n.dgrad_prelu_ok(u) for u in n.units if u.kind == "u2" and u.stage == stage):
            return B
    return None


def case_batches():
    """[(type, B)] of the GPU test: a one-image plan, a ragged batch (Bp = 8), the two computed thresholds from which the 28x28 / 128-channel and
    14x14 / 256-channel layers run on the LDS-DMA kernels with the fused epilogue, the bench batch; sphere64 once, for the long 14x14 stage"""
    return [(20, 1), (20, 5), (20, first_fused_batch(20, 1)), (20, first_fused_batch(20, 2)), (20, 128), (64, 64)]


# ================================================================================================ references and tolerances
def ratio(got, ref, tol):
    """max over elements of |got - ref| / tol on the tensors' device (0 / 0 counts as 0, NaN as inf)"""
    e = (got.to(f64).reshape(ref.shape) - ref).abs()
    r = torch.where(e == 0, torch.zeros_like(e), e / tol)
    return float(torch.nan_to_num(r, nan=float("inf")).max())


def w16_of(u, w, s16):
    """round16 of a unit's weights [Cout][3][3][cin_real] at the stored width (sph_pad_w0_kernel: channels >= cin_real zero)"""
    h = w.to(s16)
    if u.cin == u.cin_real:
        return h
    out = torch.zeros(u.cout, 3, 3, u.cin, dtype=s16, device=w.device)
    out[..., :u.cin_real] = h
    return out


def pad_input_ref(x, s16):
    """ew_pad_input_nhwc: fp32 NCHW [B][3][H][H] -> 16-bit NHWC [B][H][H][64], channels 3 .. 63 zero"""
    B, C, H, _ = x.shape
    out = torch.zeros(B, H, H, 64, dtype=s16, device=x.device)
    out[..., :C] = x.permute(0, 2, 3, 1).to(s16)
    return out


def out16_tol(ref, S, Kc, s16):
    """conv_cases.ConvCase.out16_q + the fp16 subnormal spacing"""
    return u16(s16) * ref.abs() + (Kc + 2) * U24 * S + K.floor16(s16)


def z_sign(c16, bias):
    """(z in float64, z <= 0 as the kernels decide it: float32(c) + bias in fp32)"""
    z32 = c16.to(f32) if bias is None else c16.to(f32) + bias.to(f32)
    z = c16.to(f64) if bias is None else c16.to(f64) + bias.to(f64)
    return z, z32 <= 0


def act_ref(c16, bias, alpha, ident16, s16):
    """t = prelu(c + bias) (+ identity): (value, tolerance)"""
    z, neg = z_sign(c16, bias)
    y = torch.where(neg, alpha.to(f64) * z, z)
    mag = c16.to(f64).abs() + (0 if bias is None else bias.to(f64).abs())
    if ident16 is not None:
        y = y + ident16.to(f64)
        mag = mag + ident16.to(f64).abs()
    return y, u16(s16) * y.abs() + RS.K_APPLY * U24 * mag + K.floor16(s16)


def prelu_bwd_ref(g, c16, bias, alpha):
    """(dz, g z over z <= 0) of an incoming gradient g (float64) — rowslab_cases.PreluCase.terms"""
    z, neg = z_sign(c16, bias)
    return torch.where(neg, g * alpha.to(f64), g), torch.where(neg, g * z, torch.zeros_like(z)), neg, z


def dz_tol(dz, s16):
    return (u16(s16) + 2 * U24) * dz.abs() + K.floor16(s16)


def dz_u1_tol(dz, S, d, Kc, s16):
    """dz of u1 = (dgrad of dz_u2) prelu'(c_u1).  Fused: round16(acc d), acc the fp32 accumulator.  Unfused: dt1 = round16(acc) is stored, then
    round16(dt1 d).  The double rounding bounds both: (2 u16 (1 + u16) + 2 2^-24) |dz| + (K + 2) 2^-24 S |d| (1 + u16) + 2 floor16"""
    u = u16(s16)
    return (2 * u * (1 + u) + 2 * U24) * dz.abs() + (Kc + 2) * U24 * S * d.abs() * (1 + u) + 2 * K.floor16(s16)


def gsum_tol(ref, da, Sda, Kc, s16):
    """the gradient entering a block = round16(g + da), da = round16(dgrad): stored, then added by the PReLU pass (a plan that added the fp32
    accumulator instead would round once and lie inside the same bound)"""
    return out16_tol(da, Sda, Kc, s16) + (u16(s16) + U24) * ref.abs() + K.floor16(s16)


def dw_chain(Kp, splits):
    """chain length of a split-K weight gradient.  conv_cases.dw_q counts Kp + splits + 2, one chain over all Kp pixels; here Kp reaches 401 408 (the stem
    at B = 128) and that bound (0.024 S) would let a whole dropped slab pass.  No kernel forms such a chain: a split accumulates its own pixels — at most
    ceil(Kp / splits) rounded up to the unit the kernel splits by, a 64-pixel K-step (gemm_tn, gemm_tn_glds) or a 196-pixel sub-image (wgrad9, wgrad9p):
    + 256 covers either — and the slabs are added afterwards: ceil(Kp / splits) + 256 + splits + 2, never more than dw_q's count + 256"""
    return K.cdiv(Kp, splits) + 256 + splits + 2


def sums_tol(v, mag, chain, P, extra=0.0):
    """dbias / dalpha: the partial rows' fp32 chains, the fp64 finalize over P rows and its one fp32 store (rowslab_cases.prelu_fin_q), + extra"""
    return chain * U24 * mag + U24 * v.abs() + U53 * P * mag + extra


def compare(net, T, s16, dev, got=None):
    """yields (what, error / tolerance) for every comparison of the plan's stored tensors T (see the module docstring; tests/test_sphnet_units_gpu.py
    and tests/test_sphnet_cases_cpu.py build T), every element of every tensor included.  T: x, xin, w / b / a (per unit, fp32), inp / c / t / dz
    (per unit, 16 bit NHWC; the last t NCHW-flat [B][C hw]), fcw, fcb, feats, dfeats, dw / db / da (per unit), dfcw, dfcb, cap {unit index: tensor}.
    got: the same keys, checked INSTEAD of T's against references that are still fed from T"""
    B, units = net.B, net.units
    X = T if got is None else got       # the values under test (the CPU test passes its float32 evaluation taken BEFORE the final store); operands always come from T
    D = lambda t: t.to(dev)  # noqa: E731
    d64 = lambda t: t.to(dev, f64)  # noqa: E731
    yield "xin", ratio(D(X["xin"]), pad_input_ref(D(T["x"]), s16).to(f64), torch.zeros((), dtype=f64, device=dev))
    # ---------------------------------------------------------------- forward
    for u in units:
        i = u.idx
        r = K.conv_ref(D(T["inp"][i]), w16_of(u, D(T["w"][i]), s16), u.stride, f64, dev, want=("y",))
        yield "c[%d]" % i, ratio(D(X["c"][i]), r["y"], out16_tol(r["y"], r["Sy"], 9 * u.cin, s16))
        del r
        ident = None if u.ident is None else D(T["inp"][u.ident])
        y, tol = act_ref(D(T["c"][i]), None if T["b"][i] is None else D(T["b"][i]), D(T["a"][i]), ident, s16)
        if u is units[-1]:                                  # stored NCHW-flat for x.view(B, -1)
            y, tol = RS.nchw(y.reshape(-1, u.cout), net.hw), RS.nchw(tol.reshape(-1, u.cout), net.hw)
        yield "t[%d]" % i, ratio(D(X["t"][i]), y.reshape(T["t"][i].shape), tol.reshape(T["t"][i].shape))
        del y, tol
    flat, fw = d64(T["t"][-1]).reshape(B, net.fc_in), d64(D(T["fcw"]).to(s16))
    fb = d64(T["fcb"])
    ref, S = flat @ fw.t() + fb, flat.abs() @ fw.abs().t() + fb.abs()
    sp = net.fc_fwd_splits()
    yield "feats", ratio(D(X["feats"]), ref, (K.cdiv(net.fc_in, sp) + 64 + sp + 2) * U24 * S)      # dw_chain's form, K-steps of 64
    # ---------------------------------------------------------------- fc backward
    dfe = d64(T["dfeats"])
    dfe16 = d64(D(T["dfeats"]).to(s16))
    yield "fc.bias grad", ratio(D(X["dfcb"]), dfe.sum(0), (B + 2) * U24 * dfe.abs().sum(0))
    yield "fc.weight grad", ratio(D(X["dfcw"]), dfe16.t() @ flat, (B + 3) * U24 * (dfe16.abs().t() @ flat.abs()))
    caps = net.captured()
    gx, Sx = dfe16 @ fw, dfe16.abs() @ fw.abs()             # [B][C hw] in NCHW order -> NHWC
    nhwc = lambda t: t.reshape(B, net.C, net.hw).permute(0, 2, 1).reshape(T["cap"][caps[0].idx].shape)  # noqa: E731
    gx, Sx = nhwc(gx), nhwc(Sx)
    yield "cap[%d] (fc dx)" % caps[0].idx, ratio(D(X["cap"][caps[0].idx]), gx, out16_tol(gx, Sx, net.F, s16))
    del flat, fw, gx, Sx, ref, S
    # ---------------------------------------------------------------- backward, unit by unit
    for u in reversed(units):
        i = u.idx
        M = B * u.hout * u.hout
        P = net.prelu_rows(u) if not net.mini else 1
        chain = colsum_chain(slab_rows(M, u.cout, RS.PRELU_BLOCKS), u.cout)
        bias, alpha = (None if T["b"][i] is None else D(T["b"][i])), D(T["a"][i])
        if u.kind != "u1":                                  # the PReLU pass of u2 / a head differentiates the captured gradient
            g = d64(T["cap"][i])
            dz, gz, neg, z = prelu_bwd_ref(g, D(T["c"][i]), bias, alpha)
            yield "dz[%d]" % i, ratio(D(X["dz"][i]), dz, dz_tol(dz, s16))
            sums = [(dz, 0.0), (gz, 0.0)]
        if u.kind == "u2":
            u1 = units[i - 1]
            Kc = 9 * u.cout
            r = K.conv_ref(torch.zeros(B, u.hin, u.hin, u.cin, dtype=s16, device=dev), w16_of(u, D(T["w"][i]), s16), 1, f64, dev, dy=D(T["dz"][i]), want=("dx",))
            dt, Sdt = r["dx"], r["Sdx"]
            a1 = D(T["a"][i - 1])
            dz1, gz1, neg1, z1 = prelu_bwd_ref(dt, D(T["c"][i - 1]), None, a1)
            d1 = torch.where(neg1, a1.to(f64).expand_as(dt), torch.ones_like(dt))
            yield "dz[%d]" % (i - 1), ratio(D(X["dz"][i - 1]), dz1, dz_u1_tol(dz1, Sdt, d1, Kc, s16))
            e_dt = out16_tol(dt, Sdt, Kc, s16)              # what the unfused path's stored dt1 may differ by
            fused = net.dgrad_prelu_ok(u)
            M1 = B * u1.hout * u1.hout
            ch1 = K.rows_L(M1, K.fused_rows(M1, u1.hout)) + 2 if (fused and not net.mini) else colsum_chain(slab_rows(M1, u1.cout, RS.PRELU_BLOCKS), u1.cout)
            P1 = (K.fused_rows(M1, u1.hout) if fused else net.prelu_rows(u1)) if not net.mini else 1
            C1 = u1.cout
            v, mag = gz1.reshape(-1, C1).sum(0), gz1.reshape(-1, C1).abs().sum(0)
            ex = torch.where(neg1, e_dt * z1.abs(), torch.zeros_like(z1)).reshape(-1, C1).sum(0)
            yield "prelu grad[%d]" % (i - 1), ratio(D(X["da"][i - 1]), v, sums_tol(v, mag, ch1, P1, ex))
            r = K.conv_ref(torch.zeros(B, u1.hin, u1.hin, u1.cin, dtype=s16, device=dev), w16_of(u1, D(T["w"][i - 1]), s16), 1, f64, dev, dy=D(T["dz"][i - 1]), want=("dx",))
            ref = g + r["dx"]
            yield "cap[%d]" % (i - 2), ratio(D(X["cap"][i - 2]), ref, gsum_tol(ref, r["dx"], r["Sdx"], 9 * u1.cout, s16))
            del r, dt, Sdt, dz1, gz1, neg1, z1, d1, e_dt, ref
        elif u.kind == "head" and i > 0:
            r = K.conv_ref(torch.zeros(B, u.hin, u.hin, u.cin, dtype=s16, device=dev), w16_of(u, D(T["w"][i]), s16), 2, f64, dev, dy=D(T["dz"][i]), want=("dx",))
            yield "cap[%d]" % (i - 1), ratio(D(X["cap"][i - 1]), r["dx"], out16_tol(r["dx"], r["Sdx"], 9 * u.cout, s16))
            del r
        if u.kind != "u1":
            C = u.cout
            if u.bias:
                v, mag = dz.reshape(-1, C).sum(0), dz.reshape(-1, C).abs().sum(0)
                yield "bias grad[%d]" % i, ratio(D(X["db"][i]), v, sums_tol(v, mag, chain, P))
                # the same against the column sum of the STORED dz, each element of which is within dz_tol of the unrounded value the pass summed
                st = d64(T["dz"][i]).reshape(-1, C)
                yield "bias grad[%d] vs stored dz" % i, ratio(D(X["db"][i]), st.sum(0), sums_tol(v, mag, chain, P, dz_tol(dz, s16).reshape(-1, C).sum(0)))
                del st
            v, mag = gz.reshape(-1, C).sum(0), gz.reshape(-1, C).abs().sum(0)
            yield "prelu grad[%d]" % i, ratio(D(X["da"][i]), v, sums_tol(v, mag, chain, P))
            del g, dz, gz, neg, z
        r = K.conv_ref(D(T["inp"][i]), torch.zeros(u.cout, 3, 3, u.cin, dtype=s16, device=dev), u.stride, f64, dev, dy=D(T["dz"][i]), want=("dw",))
        dw, S = r["dw"][..., :u.cin_real], r["Sdw"][..., :u.cin_real]      # the stem: through the 64-channel padding, its three real input channels kept
        yield "weight grad[%d]" % i, ratio(D(X["dw"][i]), dw, dw_chain(M, net.wgrad_slot_splits(u)[1]) * U24 * S)
        del r, dw, S
