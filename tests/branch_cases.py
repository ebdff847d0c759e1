"""Inputs and references for the tests of the fused branch head (csrc/branch.hip): ``fedfr_bce_fused`` and ``fedfr_branch_head``, in the
style of head_cases.py.

A case holds seeded fp32 inputs and ``ref(dtype)``: the head of ``train_with_public_data`` written as plain torch formulas on those inputs
converted to ``dtype``, differentiated by torch's CPU autograd.  ``ref(float64)`` is what the kernels are held to; ``ref(float32)`` is the
same formula at the kernels' precision, which tests/test_branch_cpu.py holds to a QUARTER of every tolerance.  Nothing here imports the
oracle; the formulas are the definitions:
    cos branch   F.normalize(f) @ F.normalize(fc).T -> CosFace (cos - m at the target) / ArcFace (cos(acos(cos) + m)) times s -> F.cross_entropy
    BCE branch   y = converter(f or f.detach()); cos = F.normalize(y) @ F.normalize(W).T; z = r (g(cos) -/+ m) + bias, g(x) = 2 ((x + 1) / 2)^t - 1;
                 mean_b sum_c (target ? (lam / r) log(1 + e^-z + 1e-8) : ((1 - lam) / r) log(1 + e^z + 1e-8)); labels >= n_class: no target
    contrastive  CE([cs(f, f_global) / T, cs(f, f_last) / T], 0), cs = nn.CosineSimilarity(dim=1, eps=1e-8) (each norm clamped from below)
    total        cos + bce_weight * bce + mu * contrastive

Tolerances: head_cases.TOL against fp64 — the four scalars at "loss", every gradient at "grad", per row (``row_err``).  dbias (a column sum
over the batch) is one row, as head_cases' colsum, and so is the Linear converter's bias gradient; its weight gradient is measured per
row like every other matrix.  Only the gradients that pass through the BottleBlock converter take the bound bottle_cases.py uses for that
block's backward: every row of a parameter gradient against the LARGEST row of the same tensor (its docstring gives the reason).  The
BottleBlock's kink rule is bottle_cases' too: where an fp64 pre-activation is within KINK of 0 relative to its row, the reference takes
leaky' from the sign of the activation the code under test produced.

Shapes (D = 512, what the converter supports): B in {1, 2, 5, 130} (130 rows = nine 16-row partial sums of dbias, 3 row tiles of the
GEMMs), n_class in {1, 3, 100}, C = n_class + n_public in {n_class, 255, 256, 4096, 4097} (both sides of the split-K rule 256 <= C <= 4096,
sizes that are no multiple of 32).  The cross product has 720 members; CASES is a cover: every value of every parameter, every
(converter, detach, contrastive) combination, and both sides of the split-K switch for every converter.

Edge rows (B >= 5; the labels of the first rows are 0, n_class - 1, n_class, C - 1 where those are < C):
  * row 1 is exactly zero: F.normalize's clamp (f_hat = 0, 1 / eps as the inverse norm) and CosineSimilarity's;
  * row 3 is the negative of class-weight row kb of the cos branch: cos = -1 there;
  * BCE weight row kp = label[2] is converter(f)[2] and row kn is -converter(f)[3], both from the fp64 forward: the BCE cosines of those
    elements are +1 (a target) and -1 (dg/dcos = 0 for t = 3) to fp32 rounding, whatever the converter is;
  * the bias has mixed signs.
  A feature row EQUAL to a class-weight row of the cos branch (cos = +1) is in the PLUS_SPECS cases only: row 4 is class-weight row ka with
  another class as its target, and those cases answer for the losses and d(features) but not for d(fc).  With ka as the target
  p_target = 1 - 1e-4 and p - 1 has no relative accuracy in fp32 (head_cases.softmax_inputs makes the same point for C = 2); with another
  target row ka of d(fc) is the rounding residue of g_ka (f_hat - f_hat <f_hat, f_hat>).  Both are properties of the input, not of a
  kernel.
"""
import functools

import torch
import torch.nn.functional as F

import bottle_cases
from head_cases import Q, TOL, check, label_sets, row_err, uniform, f32, f64  # noqa: F401

D = 512
S, M = 30.0, 0.4                                   # the client's margin module (client.py:133)
BCE_M, BCE_R, BCE_T, BCE_LAM, BCE_WEIGHT = 0.4, 30.0, 3.0, 0.7, 10.0
TEMPERATURE, MU = 0.5, 5.0
CONV_NONE, CONV_LINEAR, CONV_BOTTLE = 0, 1, 2
LOSS_NAMES = ("total", "cos", "contrastive", "bce")


def leaky(z, pos):
    return torch.where(pos, z, bottle_cases.SLOPE * z)


def bottle_apply(x, P, pos=None):
    """BottleBlock forward on tensors of one dtype; ``pos``: (pos1, pos2) overrides of `pre-activation > 0`.  -> y, z1, z2"""
    H = x.shape[1] // 4
    z1 = torch.cat([x @ P[4 * g].t() + P[4 * g + 1] for g in range(4)], 1)
    h1 = leaky(z1, z1 > 0 if pos is None else pos[0])
    z2 = torch.cat([h1[:, g * H:(g + 1) * H] @ P[4 * g + 2].t() + P[4 * g + 3] for g in range(4)], 1)
    h2 = leaky(z2, z2 > 0 if pos is None else pos[1])
    return x + h2 @ P[16].t() + P[17], z1, z2


def bce_rows(cos, label, bias, t, lam, m=BCE_M, r=BCE_R):
    Bn, C = cos.shape
    pos = torch.zeros(Bn, C, dtype=torch.bool)
    v = (label >= 0) & (label < C)
    pos[v, label[v]] = True
    hb = (cos + 1.0) * 0.5
    g = 2.0 * hb ** t - 1.0
    z = r * torch.where(pos, g - m, g + m) + bias
    e = torch.exp(torch.where(pos, -z, z))
    w = torch.where(pos, torch.full_like(z, lam / r), torch.full_like(z, (1.0 - lam) / r))
    return (w * torch.log(1.0 + e + 1e-8)).sum(1)


# ------------------------------------------------------------------------------------------------ fedfr_bce_fused alone
BCE_FUSED_SHAPES = [(1, 1), (2, 3), (5, 255), (17, 257), (130, 100), (3, 1000)]
BCE_LOSS_SCALE = 10.0


class BceCase:
    def __init__(self, B, C, t, lam, lab, i):
        self.B, self.C, self.t, self.lam, self.label = B, C, float(t), lam, lab
        self.name = "bce_fused[%d,%d,set%d,t=%g,lam=%g]" % (B, C, i, t, lam)
        self.cos = uniform((B, C), 2800 + C + i, -0.99, 0.99)
        self.cos[0, 0] = -1.0                                          # dg/dcos = 0 for t = 3
        self.cos[B - 1, C - 1] = 1.0
        self.bias = uniform((C,), 2810 + C, -0.5, 0.5)

    def ref(self, dt=f64):
        cos = self.cos.to(dt).clone().requires_grad_(True)
        bias = self.bias.to(dt).clone().requires_grad_(True)
        rows = bce_rows(cos, self.label, bias, self.t, self.lam)
        (BCE_LOSS_SCALE * rows.mean()).backward()
        return {"row_loss": Q(rows.detach(), "loss"), "dcos": Q(cos.grad, "grad"), "dbias": Q(bias.grad.reshape(1, -1), "grad")}


def bce_fused_cases():
    out = []
    for B, C in BCE_FUSED_SHAPES:
        for t, lam in ((3, 0.7), (1, 0.5)):
            for i, lab in enumerate(label_sets(B, C)):
                out.append(BceCase(B, C, t, lam, lab, i))
    return out


# ------------------------------------------------------------------------------------------------ fedfr_branch_head
class BranchCase:
    def __init__(self, B, n_class, C, conv, detach, con, arc=False, plus=False):
        assert C >= n_class >= 1
        self.B, self.n_class, self.C, self.conv, self.detach, self.con, self.arc = B, n_class, C, conv, bool(detach), bool(con), bool(arc)
        self.name = "branch[B=%d,n=%d,C=%d,conv=%d,detach=%d,con=%d,arc=%d%s]" % (B, n_class, C, conv, detach, con, arc, ",plus" if plus else "")
        self.plus = bool(plus)
        seed = 31000 + 7 * B + 13 * n_class + C
        kinds = [k for k in (0, n_class - 1, n_class, C - 1) if k < C]
        g = torch.Generator().manual_seed(seed)
        lab = [kinds[i % len(kinds)] for i in range(min(B, 4))] + torch.randint(0, C, (max(B - 4, 0),), generator=g).tolist()
        self.label = torch.tensor(lab, dtype=torch.int64)
        self.feats = uniform((B, D), seed + 1)
        self.fc = uniform((C, D), seed + 2)
        edge = B >= 5
        if B >= 2:
            self.feats[1] = 0.0
        if edge and C >= 2 and not arc:                      # (ArcFace: d acos / d cos is infinite at cos = -1)
            kb = (int(self.label[3]) + 1) % C
            self.feats[3] = -self.fc[kb]
        if plus:                                             # cos = +1 at a class that is not the row's target
            assert edge and C >= 2 and not arc
            self.feats[4] = self.fc[(int(self.label[4]) + 1) % C]
        self.conv_params = []
        self.bce_w = self.bce_b = None
        if conv:
            if conv == CONV_LINEAR:
                self.conv_params = [torch.eye(D) + uniform((D, D), seed + 3) * (0.5 / D ** 0.5), uniform((D,), seed + 4) * 0.1]
            else:
                self.conv_params = list(bottle_cases.case(B, D).params)
            self.bce_w = uniform((n_class, D), seed + 5)
            self.bce_b = uniform((n_class,), seed + 6, -0.5, 0.5)
            if n_class >= 2:                                 # mixed signs whatever the draw
                self.bce_b[0], self.bce_b[-1] = -self.bce_b[0].abs() - 0.01, self.bce_b[-1].abs() + 0.01
            if edge and n_class >= 2:
                y = self.converter(self.feats.to(f64), [p.to(f64) for p in self.conv_params])[0]
                kp = int(self.label[2])
                if kp >= n_class:
                    kp = n_class - 1
                    self.label[2] = kp
                kn = (kp + 1) % n_class
                self.bce_w[kp], self.bce_w[kn] = y[2].to(f32), (-y[3]).to(f32)
        self.gfeats = self.lfeats = None
        if con:
            self.gfeats = (0.7 * self.feats + 0.5 * uniform((B, D), seed + 7)).contiguous()
            self.lfeats = uniform((B, D), seed + 8)

    def converter(self, x, P, pos=None):
        if self.conv == CONV_LINEAR:
            return x @ P[0].t() + P[1], None, None
        return bottle_apply(x, P, pos)

    @functools.lru_cache(maxsize=None)
    def kink_masks(self):
        """BottleBlock only: where the fp64 pre-activations are too close to 0 for their sign to be a property of the inputs"""
        _, z1, z2 = self.converter(self.feats.to(f64), [p.to(f64) for p in self.conv_params])
        return tuple(z.abs() < bottle_cases.KINK * z.abs().amax(1, keepdim=True) for z in (z1, z2))

    def ref(self, dt=f64, h_got=None):
        """{name: Q}.  ``h_got`` = (h1, h2), the BottleBlock activations of the code under test: their signs decide leaky' at the kinks
        (without it the evaluation's own signs are used everywhere)."""
        leaf = lambda t: t.to(dt).clone().requires_grad_(True)                                   # noqa: E731
        x, fc = leaf(self.feats), leaf(self.fc)
        onehot = F.one_hot(self.label, self.C).to(torch.bool)
        cos = F.normalize(x, dim=1) @ F.normalize(fc, dim=1).t()
        if self.arc:
            th = torch.acos(cos)
            logits = S * torch.cos(torch.where(onehot, th + M, th))
        else:
            logits = S * (cos - M * onehot.to(dt))
        cos_loss = F.cross_entropy(logits, self.label)
        total = cos_loss
        zero = torch.zeros((), dtype=dt)
        bce = con = zero
        P = []
        if self.conv:
            P = [leaf(p) for p in self.conv_params]
            W, b = leaf(self.bce_w), leaf(self.bce_b)
            pos = None
            if self.conv == CONV_BOTTLE and h_got is not None:
                with torch.no_grad():
                    _, z1, z2 = self.converter(x.detach(), [p.detach() for p in P])
                k1, k2 = self.kink_masks()
                pos = (torch.where(k1, h_got[0].detach().cpu() > 0, z1 > 0), torch.where(k2, h_got[1].detach().cpu() > 0, z2 > 0))
            y = self.converter(x.detach() if self.detach else x, P, pos)[0]
            bcos = F.normalize(y, dim=1) @ F.normalize(W, dim=1).t()
            bce = bce_rows(bcos, self.label, b, BCE_T, BCE_LAM).mean()
            total = total + BCE_WEIGHT * bce
        if self.con:
            gf, lf = self.gfeats.to(dt), self.lfeats.to(dt)
            eps = torch.tensor(1e-8, dtype=f32).to(dt)
            nx = x.norm(dim=1).clamp_min(eps)
            pos_ = (x * gf).sum(1) / (nx * gf.norm(dim=1).clamp_min(eps)) / TEMPERATURE
            neg_ = (x * lf).sum(1) / (nx * lf.norm(dim=1).clamp_min(eps)) / TEMPERATURE
            con = F.cross_entropy(torch.stack([pos_, neg_], 1), torch.zeros(self.B, dtype=torch.int64))
            total = total + MU * con
        total.backward()
        out = {"losses": Q(torch.stack([total.detach(), cos_loss.detach(), con.detach(), bce.detach()]), "loss"),
               "dfeats": Q(x.grad, "grad")}
        if not self.plus:                                    # (module docstring: row ka of d(fc) is ill-conditioned there)
            out["dfc"] = Q(fc.grad, "grad")
        if self.conv:
            out["dbce_w"] = Q(W.grad, "grad")
            out["dbce_b"] = Q(b.grad.reshape(1, -1), "grad")
            for i, p in enumerate(P):
                g = p.grad
                if self.conv == CONV_LINEAR:                 # weight per row, bias one row
                    out["dconv%d" % i] = Q(g if g.dim() == 2 else g.reshape(1, -1), "grad")
                    continue
                rows = g if g.dim() == 2 else g.reshape(-1, 1)
                out["dconv%d" % i] = Q(g, "grad", scale=torch.full((rows.shape[0],), float(rows.abs().amax(1).max()), dtype=f64))
        return out


# (B, n_class, C, converter, detach, contrastive): see the module docstring for what the list covers
_N, _L, _K = CONV_NONE, CONV_LINEAR, CONV_BOTTLE
CASE_SPECS = [
    (1, 1, 1, _N, 0, 0), (2, 3, 3, _L, 0, 1), (5, 3, 255, _K, 0, 0), (5, 100, 256, _L, 1, 0), (5, 100, 4096, _K, 1, 1),
    (130, 100, 4097, _L, 0, 0), (130, 100, 256, _K, 0, 1), (130, 3, 255, _N, 0, 1), (5, 1, 4096, _N, 1, 0), (2, 100, 100, _K, 1, 0),
    (1, 3, 4097, _K, 0, 0), (5, 3, 4097, _L, 1, 1), (130, 1, 256, _L, 0, 1), (2, 1, 255, _N, 1, 1), (1, 100, 4096, _L, 0, 0),
]
ARC_SPEC = (5, 3, 256, _L, 0, 0)
PLUS_SPECS = [(5, 3, 256, _N, 0, 0), (130, 100, 4097, _L, 0, 1)]


@functools.lru_cache(maxsize=None)
def branch_cases():
    return tuple(BranchCase(*s) for s in CASE_SPECS) + (BranchCase(*ARC_SPEC, arc=True),) + tuple(BranchCase(*s, plus=True) for s in PLUS_SPECS)
