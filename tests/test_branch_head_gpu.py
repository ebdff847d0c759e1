"""The fused branch head (csrc/branch.hip) on the GPU: ``fedfr_bce_fused`` and ``fedfr_branch_head`` through the C ABI on raw pointers
against the fp64 formulas of tests/branch_cases.py (losses at the "loss" level, every gradient at the "grad" level, per row), against
the existing autograd composition of the same head (twice those tolerances: each side is within one of fp64), bit-reproducibility,
the error path, and ``FusedBranchTrainer`` / ``Client.train_with_public_data`` on top of it.  Outputs and the workspace are NaN before
every call."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

import branch_cases as BC  # noqa: E402
import head_cases as hc  # noqa: E402
from fedfr_amd import _C, backbones, client, losses, ops  # noqa: E402

NAN = float("nan")
f32 = torch.float32
DEV = torch.device("cuda:0")


def Dv(t):
    return t.to(DEV).contiguous()


def nans(*shape):
    return torch.full(shape, NAN, dtype=f32, device=DEV)


def chk(got, q, what, frac=1.0):
    """hc.check with the figure printed before it is asserted (pytest -s shows them)"""
    figs = []
    try:
        hc.check(got, q, what, frac=frac, out=figs)
    finally:
        for f in figs:
            print("%-100s %-5s %.3g" % f)


def pointers(ts):
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts]) if ts else None


# ------------------------------------------------------------------------------------------------ fedfr_bce_fused
def run_bce_fused(case):
    B, C = case.B, case.C
    cos, lab, bias = Dv(case.cos), Dv(case.label), Dv(case.bias)
    row_loss, dcos, dbias = nans(B), nans(B, C), nans(C)
    nbytes = _C.lib().fedfr_bce_fused_workspace_bytes(B, C)
    assert nbytes >= 4 * -(-B // 16) * C
    ws = nans(nbytes // 4)
    _C.call("fedfr_bce_fused", cos.data_ptr(), lab.data_ptr(), bias.data_ptr(), B, C, BC.BCE_M, BC.BCE_R, case.t, case.lam, BC.BCE_LOSS_SCALE,
            row_loss.data_ptr(), dcos.data_ptr(), dbias.data_ptr(), ws.data_ptr(), nbytes, _C.stream())
    torch.cuda.synchronize()
    assert torch.equal(cos.cpu(), case.cos), "the cosines were overwritten"
    return {"row_loss": row_loss, "dcos": dcos, "dbias": dbias.reshape(1, -1)}


@pytest.mark.parametrize("case", BC.bce_fused_cases(), ids=lambda c: c.name)
def test_bce_fused_vs_fp64(case):
    """B around the 16 rows of a workgroup and beyond one partial row (130 -> 9), C around the 256 columns of a chunk; labels -1, C, C - 1, 0;
    cos = -1 (dg/dcos = 0 for t = 3) and +1; twice on the same inputs: the same bits"""
    ref = case.ref()
    got = run_bce_fused(case)
    for k in ("row_loss", "dcos", "dbias"):
        assert bool(torch.isfinite(got[k]).all()), "%s %s: an output element was not written" % (case.name, k)
        chk(got[k], ref[k], "%s:%s" % (case.name, k))
    again = run_bce_fused(case)
    for k in got:
        assert torch.equal(got[k], again[k]), "%s %s: not bit-reproducible" % (case.name, k)


# ------------------------------------------------------------------------------------------------ fedfr_branch_head
def run_branch_head(case):
    B, C, n, D = case.B, case.C, case.n_class, BC.D
    feats, lab, fc = Dv(case.feats), Dv(case.label), Dv(case.fc)
    cp = [Dv(p) for p in case.conv_params]
    cg = [nans(*p.shape) for p in case.conv_params]
    bw, bb = (Dv(case.bce_w), Dv(case.bce_b)) if case.conv else (None, None)
    dbw, dbb = (nans(n, D), nans(n)) if case.conv else (None, None)
    gf, lf = (Dv(case.gfeats), Dv(case.lfeats)) if case.con else (None, None)
    losses_, dfeats, dfc = nans(4), nans(B, D), nans(C, D)
    nbytes = _C.lib().fedfr_branch_workspace_bytes(B, D, C, n, case.conv, int(case.detach), int(case.con))
    assert nbytes > 0
    ws = nans(nbytes // 4)
    keep = (cp, cg)                                                          # the pointer arrays hold no references
    _C.call("fedfr_branch_head", feats.data_ptr(), lab.data_ptr(), B, D, fc.data_ptr(), C, int(case.arc), BC.S, BC.M, case.conv, pointers(cp),
            _C.ptr(bw), _C.ptr(bb), n, BC.BCE_M, BC.BCE_R, BC.BCE_T, BC.BCE_LAM, BC.BCE_WEIGHT, _C.ptr(gf), _C.ptr(lf), BC.TEMPERATURE, BC.MU,
            int(case.detach), losses_.data_ptr(), dfeats.data_ptr(), dfc.data_ptr(), pointers(cg), _C.ptr(dbw), _C.ptr(dbb), ws.data_ptr(),
            nbytes, _C.stream())
    torch.cuda.synchronize()
    del keep
    out = {"losses": losses_, "dfeats": dfeats, "dfc": dfc}
    if case.conv:
        out["dbce_w"], out["dbce_b"] = dbw, dbb.reshape(1, -1)
        for i, g in enumerate(cg):
            out["dconv%d" % i] = g
    return out


def bottle_activations(case):
    """h1, h2 of the BottleBlock kernels on the case's features: the signs the reference uses at the kinks (the same launch runs inside branch_head)"""
    x = Dv(case.feats)
    cp = [Dv(p) for p in case.conv_params]
    h1, h2, y = nans(*x.shape), nans(*x.shape), nans(*x.shape)
    _C.call("fedfr_bottle_forward", x.data_ptr(), pointers(cp), case.B, BC.D, h1.data_ptr(), h2.data_ptr(), y.data_ptr(), _C.stream())
    torch.cuda.synchronize()
    return h1, h2


def autograd_branch_head(case):
    """the same head through the existing autograd composition: FC_module -> margin -> ops.cross_entropy, BCE_module -> BCE_loss,
    ops.contrastive_loss, .backward()"""
    D = BC.D
    fcm = client.FC_module(D, case.C, "/tmp").to(DEV)
    fcm.fc.data = Dv(case.fc)
    margin = (losses.ArcFace if case.arc else losses.CosFace)(s=BC.S, m=BC.M)
    lab = Dv(case.label)
    feats = Dv(case.feats).requires_grad_(True)
    bm = None
    with torch.enable_grad():
        cos_loss = ops.cross_entropy(margin(fcm(feats), lab), lab)
        loss = cos_loss
        zero = torch.zeros((), device=DEV)
        bce = con = zero
        if case.conv:
            bm = client.BCE_module(D, case.n_class, 1 if case.conv == BC.CONV_LINEAR else 2, m=BC.BCE_M, r=BC.BCE_R, t=int(BC.BCE_T)).to(DEV)
            conv_params = list(bm.converter.parameters())
            assert len(conv_params) == len(case.conv_params)
            for p, v in zip(conv_params, case.conv_params):
                p.data = Dv(v)
            bm.weight.data, bm.bias.data = Dv(case.bce_w), Dv(case.bce_b)
            z, gt = bm(feats.detach() if case.detach else feats, lab)
            bce = losses.BCE_loss(r=BC.BCE_R, lambda_=BC.BCE_LAM)(z, gt)
            loss = loss + BC.BCE_WEIGHT * bce
        if case.con:
            con = ops.contrastive_loss(feats, Dv(case.gfeats), Dv(case.lfeats), BC.TEMPERATURE)
            loss = loss + BC.MU * con
        loss.backward()
    torch.cuda.synchronize()
    out = {"losses": torch.stack([loss.detach(), cos_loss.detach(), con.detach(), bce.detach()]), "dfeats": feats.grad, "dfc": fcm.fc.grad}
    if case.conv:
        out["dbce_w"], out["dbce_b"] = bm.weight.grad, bm.bias.grad.reshape(1, -1)
        for i, p in enumerate(bm.converter.parameters()):
            out["dconv%d" % i] = p.grad
    return out


@pytest.mark.parametrize("case", BC.branch_cases(), ids=lambda c: c.name)
def test_branch_head_vs_fp64_and_autograd(case):
    h_got = bottle_activations(case) if case.conv == BC.CONV_BOTTLE else None
    ref = case.ref(hc.f64, h_got)
    got = run_branch_head(case)
    assert set(ref) <= set(got) and set(got) - set(ref) <= {"dfc"}
    for k, q in ref.items():
        assert bool(torch.isfinite(got[k]).all()), "%s %s: an output element was not written" % (case.name, k)
        chk(got[k].reshape(q.value.shape), q, "%s:%s" % (case.name, k))
    # bit-reproducible
    again = run_branch_head(case)
    for k in got:
        assert bool(torch.isfinite(got[k]).all()) and torch.equal(got[k], again[k]), "%s %s: not bit-reproducible" % (case.name, k)
    # the existing autograd composition: within twice the tolerances (each side is within one of fp64)
    auto = autograd_branch_head(case)
    assert set(auto) == set(got)
    for k, q in ref.items():
        v = auto[k].detach().to("cpu", hc.f64).reshape(q.value.shape)
        scale = None
        if q.scale is not None:                                              # BottleBlock gradients: against the largest row of the tensor
            rows = v if v.dim() == 2 else v.reshape(-1, 1)
            scale = torch.full((rows.shape[0],), float(rows.abs().amax(1).max()), dtype=hc.f64)
        chk(got[k].reshape(q.value.shape), hc.Q(v, q.kind, scale), "%s:%s vs autograd" % (case.name, k), frac=2.0)


@pytest.mark.parametrize("R,D_,nslab", [(1, 1, 1), (5, 65, 3), (7, 512, 2), (6, 600, 3)])
@pytest.mark.parametrize("extras", [(False, False), (True, False), (True, True)])
def test_branch_dfeats_vs_fp64(R, D_, nslab, extras):
    """``fedfr_branch_dfeats`` alone: D on both sides of the 512 elements a wave keeps in registers, R no multiple of the four rows of a
    workgroup, slabs with a gap between them, each optional addend present and absent"""
    case = hc.normalize_bwd_case(R, D_, nslab, 0.0)
    a, b, mu = BC.uniform((R, D_), 5100 + D_), BC.uniform((R, D_), 5200 + D_), 5.0
    want = case.ref()["dx"].value
    if extras[0]:
        want = want + a.to(hc.f64)
    if extras[1]:
        want = want + mu * b.to(hc.f64)
    gap = 7
    slabs = torch.full((nslab, R * D_ + gap), hc.SENTINEL, dtype=f32, device=DEV)
    slabs[:, :R * D_] = Dv(case.inputs["slabs"]).reshape(nslab, -1)
    xn, inv, out = Dv(case.inputs["xn"]), Dv(case.inputs["inv"]), nans(R, D_)
    da, db = (Dv(a) if extras[0] else None), (Dv(b) if extras[1] else None)
    _C.call("fedfr_branch_dfeats", xn.data_ptr(), inv.data_ptr(), slabs.data_ptr(), nslab, R * D_ + gap, _C.ptr(da), _C.ptr(db), mu,
            out.data_ptr(), R, D_, _C.stream())
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and bool((slabs[:, R * D_:] == hc.SENTINEL).all())
    chk(out, hc.Q(want, "grad"), "%s extras=%s" % (case.name, extras))


def test_branch_head_reports_unsupported_arguments():
    """an error string and no launch: nothing below hands a kernel a pointer it could dereference (every check comes before the first launch)"""
    lib = _C.lib()
    B, D, C, n = 2, 512, 8, 3
    feats, lab, fc = torch.zeros(B, D, device=DEV), torch.zeros(B, dtype=torch.int64, device=DEV), torch.ones(C, D, device=DEV)
    out = nans(4), nans(B, D), nans(C, D)
    ws = nans(1 << 20)
    cw, cb, bw, bb = torch.eye(D, device=DEV), torch.zeros(D, device=DEV), torch.ones(n, D, device=DEV), torch.zeros(n, device=DEV)
    cgw, cgb, dbw, dbb = nans(D, D), nans(D), nans(n, D), nans(n)

    def call(B=B, D=D, conv=1, feats=feats, cp=(cw, cb), ws_bytes=ws.numel() * 4, gf=None, lf=None):
        return lib.fedfr_branch_head(feats.data_ptr() if feats is not None else None, lab.data_ptr(), B, D, fc.data_ptr(), C, 0, 30.0, 0.4, conv,
                                     pointers(list(cp)), bw.data_ptr(), bb.data_ptr(), n, 0.4, 30.0, 3.0, 0.7, 10.0, _C.ptr(gf), _C.ptr(lf), 0.5, 5.0,
                                     0, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), pointers([cgw, cgb] * (len(cp) // 2)),
                                     dbw.data_ptr(), dbb.data_ptr(), ws.data_ptr(), ws_bytes, _C.stream())

    assert lib.fedfr_branch_workspace_bytes(0, D, C, n, 1, 0, 0) == 0 and lib.fedfr_branch_workspace_bytes(B, 100, C, n, 2, 0, 0) == 0
    assert lib.fedfr_bce_fused_workspace_bytes(0, 5) == 0
    for kw, word in ((dict(B=0), "B = 0"), (dict(D=100, conv=2, cp=(cw, cb) * 9), "BottleBlock"), (dict(feats=None), "null"),
                     (dict(ws_bytes=16), "workspace"), (dict(gf=feats), "last_feats"), (dict(conv=3), "converter kind")):
        assert call(**kw) != 0, kw
        assert word in _C.last_error(), (kw, _C.last_error())
    assert lib.fedfr_bce_fused(None, lab.data_ptr(), bb.data_ptr(), B, n, 0.4, 30.0, 3.0, 0.7, 1.0, dbb.data_ptr(), dbw.data_ptr(), dbb.data_ptr(),
                               ws.data_ptr(), ws.numel() * 4, _C.stream()) != 0
    assert "bce_fused" in _C.last_error()
    assert lib.fedfr_branch_dfeats(None, None, None, 1, 0, None, None, 0.0, out[1].data_ptr(), B, D, _C.stream()) != 0
    assert "branch_dfeats" in _C.last_error()
    torch.cuda.synchronize()
    for t in out + (cgw, cgb, dbw, dbb):
        assert bool(torch.isnan(t).all()), "a refused call wrote an output"
    assert call() == 0, _C.last_error()                                     # the same arguments without the fault run
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out[0]).all())


# ------------------------------------------------------------------------------------------------ the trainer
NL, NPUB, TB = 6, 14, 4


def _state():
    from oracle import ref_cpu as R
    return R, R.closed_form_state_dict(R.IRESNET_LAYERS["iresnet18"], tag=2.0)


def _modules(R, use_bce, conv_layer=1):
    fcm = client.FC_module(512, NL + NPUB, "/tmp").to(DEV)
    fcm.fc.data = torch.cat([R.head_fc(NL, seed=11), R.head_fc(NPUB, seed=12)]).to(DEV)
    bm = None
    if use_bce:
        torch.manual_seed(5)
        bm = client.BCE_module(512, NL, conv_layer).to(DEV)
        bm.weight.data = R.head_fc(NL, seed=13).to(DEV)
        bm.bias.data = (0.1 * BC.uniform((NL,), 17)).to(DEV)
    return fcm, bm


@pytest.mark.parametrize("use_bce,use_con,detach", [(True, True, False), (True, False, True), (False, True, False)])
def test_fused_branch_trainer_matches_head_trainer(use_bce, use_con, detach):
    """iresnet18, B = 4, the loaded library's default settings: FusedBranchTrainer and FusedHeadTrainer with train_with_public_data's closure
    start from the same state and take one step.  Loss tuples within twice the "loss" tolerance; every head parameter within
    lr * 2 TOL["grad"] * max|grad| per row.  (Backbone weights are not compared here: DESIGN.md section 4.)"""
    R, sd = _state()
    lr, mom, wd, mu, temp = 0.05, 0.9, 5e-4, 5.0, 0.5
    imgs, lab = R.closed_form_images(TB, tag=0.0).to(DEV), R.closed_form_labels(TB, NL + NPUB, tag=0).to(DEV)
    gf, lf = (BC.uniform((TB, 512), 41).to(DEV), BC.uniform((TB, 512), 42).to(DEV)) if use_con else (None, None)
    res = {}
    for which in ("fused", "closure"):
        m = backbones.iresnet18().to(DEV)
        m.load_state_dict(sd)
        fcm, bm = _modules(R, use_bce)
        params = list(fcm.parameters()) + (list(bm.parameters()) if bm is not None else [])
        before = [p.data.clone() for p in params]
        if which == "fused":
            tr = client.FusedBranchTrainer(m, fcm, bm, "CosFace", 30.0, 0.4, detach=detach, mu=mu if use_con else 0.0, temperature=temp,
                                           bce_weight=10.0, lr=lr, momentum=mom, weight_decay=wd)
            out = tr.step(imgs, lab, gf, lf)
            grads = [tr.head_grads[p].clone() for p in params]
            assert not any(p.grad is not None for p in params) and not any(t.requires_grad for t in out if t is not None)
        else:
            margin, bce_loss = losses.CosFace(s=30, m=0.4), losses.BCE_loss()
            tr = client.FusedHeadTrainer(m, params, lr=lr, momentum=mom, weight_decay=wd)

            head_loss = client.public_head_loss(margin, fcm, bm, bce_loss if use_bce else None, detach, None,
                                                {"global_feats": gf, "last_feats": lf} if use_con else None, temp, mu)
            out = tr.step(imgs, lab, head_loss)
            grads = [p.grad.clone() for p in params]
        tr.finish()
        torch.cuda.synchronize()
        res[which] = (out, [p.data.clone() for p in params], grads, before)
    (fo, fp, fg, fb), (co, cp, cg, cb) = res["fused"], res["closure"]
    assert [o is None for o in fo] == [o is None for o in co]
    for name, a, b in zip(BC.LOSS_NAMES, fo, co):
        if a is not None:
            chk(a, hc.Q(b.detach().to("cpu", hc.f64), "loss"), "trainer loss %s" % name, frac=2.0)
    for i, (a, b, g, p0a, p0b) in enumerate(zip(fp, cp, cg, fb, cb)):
        assert torch.equal(p0a, p0b)
        assert not torch.equal(a, p0a), "head parameter %d was not updated" % i
        a2, b2, g2 = (t.reshape(-1, t.shape[-1]) if t.dim() == 2 else t.reshape(1, -1) for t in (a, b, g))
        err = (a2 - b2).abs().amax(1)
        bound = lr * 2 * hc.TOL["grad"] * g2.abs().amax(1)
        print("head parameter %d: worst |diff| %.3g, smallest bound %.3g, worst ratio %.3g" % (i, float(err.max()), float(bound.min()),
                                                                                            float((err / (bound + 1e-30)).max())))
        assert bool((err <= bound).all()), "head parameter %d: row %d differs by %.3g > %.3g" % (
            i, int((err - bound).argmax()), float(err[(err - bound).argmax()]), float(bound[(err - bound).argmax()]))


@pytest.mark.parametrize("mode", ["default", "env_off", "reweight"])
def test_client_picks_the_trainer(mode, monkeypatch):
    """Client.train_with_public_data builds a FusedBranchTrainer by default, a FusedHeadTrainer under FEDFR_FUSED_BRANCH=0 or reweight_cosface"""
    R, sd = _state()
    built = []

    class RecBranch(client.FusedBranchTrainer):
        def __init__(self, *a, **k):
            built.append("branch")
            super().__init__(*a, **k)

    class RecHead(client.FusedHeadTrainer):
        def __init__(self, *a, **k):
            built.append("head")
            super().__init__(*a, **k)

    monkeypatch.setattr(client, "FusedBranchTrainer", RecBranch)
    monkeypatch.setattr(client, "FusedHeadTrainer", RecHead)
    if mode == "env_off":
        monkeypatch.setenv("FEDFR_FUSED_BRANCH", "0")
    else:
        monkeypatch.delenv("FEDFR_FUSED_BRANCH", raising=False)

    class Args:
        network, loss, local_epoch, output_dir, aggr_alg, num_client = "iresnet18", "CosFace", 1, "/tmp", "FedAvg", 4
        BCE_local, contrastive_bb, reweight_cosface = True, False, mode == "reweight"
        BCE_detach, combine_dataset = False, True

    class DS:
        ID_base, num_classes = 0, NL

    class Loader(list):
        dataset = DS()

    class Data:
        train_class_sizes, train_dataset_sizes, train_loaders = [NL], [TB], [Loader()]

    cl = client.Client(0, Args, Data, device=DEV)
    cl.backbone_state_dict = sd
    cl.fc_module.fc.data = R.head_fc(NL, seed=11)
    cl.bce_module.weight.data = R.head_fc(NL, seed=13)
    batches = [(R.closed_form_images(TB, tag=0.0), R.closed_form_labels(TB, NL + NPUB, tag=0))]
    cl.train_with_public_data(pretrained_fc=R.head_fc(NPUB, seed=12), combine_loader=batches)
    assert built == (["branch"] if mode == "default" else ["head"]), built
    assert cl.get_train_loss() > 0 and cl.bce_meter.count == 1 and cl.cos_meter.count == 1
