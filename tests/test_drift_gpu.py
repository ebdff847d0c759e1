"""FedProx and SCAFFOLD on the GPU: the six new instantiations of the SGD kernel (fedfr_sgd_step_drift) and SCAFFOLD's end-of-round pass
(fedfr_scaffold_control) bit for bit against tests/drift_cases.py; the argument errors of the three entry points; the trainers with both
terms inside the backward pass against the flat route and against a host replay; and whole server rounds with ``prox_mu`` and with
``aggr_alg="SCAFFOLD"``.  The storage type is the loaded library's: the file runs unchanged on the fp16 and the bf16 build."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import drift_cases as Dc  # noqa: E402
import step_cases as S  # noqa: E402
import tail_cases as T  # noqa: E402
from oracle import ref_cpu as R  # noqa: E402
from fedfr_amd import _C, backbones, client, losses, ops, server  # noqa: E402

NAN = float("nan")
f32 = torch.float32
GUARD = 256
FILL16 = 0x5555
DEV = torch.device("cuda:0")


def S16():
    return _C.storage_dtype()


def D(t):
    if isinstance(t, np.ndarray):
        t = torch.from_numpy(np.array(t))
    return t.to(DEV).contiguous()


def galloc(n, dtype=f32):
    """(buffer, view of n elements): NaN (fp32), a fill pattern (16-bit) or -7 (int32), with a guard band behind"""
    if dtype == f32:
        buf = torch.full((n + GUARD,), NAN, dtype=f32, device=DEV)
    elif dtype == torch.int32:
        buf = torch.full((n + GUARD,), -7, dtype=dtype, device=DEV)
    else:
        buf = torch.full((n + GUARD,), FILL16, dtype=torch.int16, device=DEV).view(dtype)
    return buf, buf[:n]


def guard_ok(buf):
    t = buf[-GUARD:]
    if t.dtype == f32:
        return bool(torch.isnan(t).all())
    if t.dtype == torch.int32:
        return bool((t == -7).all())
    return bool((t.view(torch.int16) == FILL16).all())


def loaded(src):
    buf, v = galloc(len(src))
    v.copy_(D(src))
    return buf, v


def npy(t):
    return t.detach().cpu().numpy()


def run(name, *args):
    _C.call(name, *args, _C.stream())
    torch.cuda.synchronize()


def rc_of(name, *args):
    rc = getattr(_C.lib(), name)(*args, _C.stream())
    torch.cuda.synchronize()
    return rc


def _drift_step(pd, gd, bd, sd, n, hyper, first, gs, word, anchor, a, corr):
    lr, mu, wd = hyper
    run("fedfr_sgd_step_drift", pd.data_ptr(), gd.data_ptr(), bd.data_ptr(), sd.data_ptr() if sd is not None else None, n, lr, mu, wd, first,
        gs, word.data_ptr() if word is not None else None, anchor.data_ptr() if anchor is not None else None, a,
        corr.data_ptr() if corr is not None else None)


# ------------------------------------------------------------------------------------------------ the SGD kernel
@pytest.mark.parametrize("kind", sorted(Dc.KINDS))
@pytest.mark.parametrize("n", S.SGD_N)
def test_sgd_step_drift_two_steps_bit_exact(n, kind):
    """first = 1 on a NaN momentum buffer, then first = 0 with another gradient, with the mirror, at S.SGD_HYPER: p, buf and the mirror bit
    for bit, for the unguarded and the guarded instantiation of this kind (the guarded one on a gradient buffer that holds g 2^8: it reads
    g afterwards and the word stays 0); anchor, corr and every guard band untouched"""
    p, g = S.sgd_inputs(n)
    g2 = S.sgd_second_grad(n)
    anchor, corr = Dc.drift_inputs(n)
    has_a, has_c = Dc.KINDS[kind]
    (p1, b1), (p2, b2) = Dc.drift_two_steps(n, kind)
    ad, cd = (D(anchor) if has_a else None), (D(corr) if has_c else None)
    a = Dc.DRIFT_A if has_a else 0.0
    for guarded in (False, True):
        gs = S.SGD_SCALE if guarded else 1.0
        scale = np.float32(1.0 / gs)
        (pb, pd), (gb, gd), (bb, bd), (sb, sd) = loaded(p), loaded(g * scale), galloc(n), galloc(n, S16())
        wbuf, word = galloc(1, torch.int32)
        word.fill_(0)
        for step, (gin, wp, wb) in enumerate(((g, p1, b1), (g2, p2, b2))):
            if step:
                gd.copy_(D(gin * scale))
            _drift_step(pd, gd, bd, sd, n, S.SGD_HYPER, 1 - step, gs, word if guarded else None, ad, a, cd)
            w = "drift[n=%d,%s,guarded=%d] step %d " % (n, kind, guarded, step + 1)
            S.same32(npy(pd), wp, w + "p")
            S.same32(npy(bd), wb, w + "buf")
            S.same32(npy(gd), gin, w + "gradient")
            T.same16(sd, S.shadow_ref(wp, S16()), w + "mirror")
        assert int(word[0]) == 0
        assert all(guard_ok(b) for b in (pb, gb, bb, sb, wbuf))
    if has_a:
        S.same32(npy(ad), anchor, "anchor is read-only")
    if has_c:
        S.same32(npy(cd), corr, "corr is read-only")


@pytest.mark.parametrize("kind", sorted(Dc.KINDS))
@pytest.mark.parametrize("n", [1, 3, 5, 1025, 4103, S.SGD_WRAP_N])
def test_sgd_step_drift_guard_skips_non_finite_gradients(n, kind):
    """inf, -inf and NaN gradients at S.sgd_bad_positions(n): those elements keep p and buf (0 on the first step), the word is 1, every
    other element is the clean step's — and a finite, infinite or NaN anchor / corr value AT those positions changes nothing"""
    p, g = S.sgd_inputs(n)
    (p1, b1), (p2, b2) = Dc.drift_two_steps(n, kind)
    anchor, corr = Dc.drift_inputs(n)
    has_a, has_c = Dc.KINDS[kind]
    a = Dc.DRIFT_A if has_a else 0.0
    gs = S.SGD_SCALE
    pos = S.sgd_bad_positions(n)
    planted = np.array([0.5, np.inf, np.nan, -np.inf] * len(pos), dtype=np.float32)[:len(pos)]
    for first in (1, 0):
        p0, b0, gin, clean_p, clean_b = (p, None, g, p1, b1) if first else (p1, b1, S.sgd_second_grad(n), p2, b2)
        gin = (gin / np.float32(gs)).astype(np.float32)
        gin[pos] = S.sgd_bad_values(len(pos))
        for plant in (False, True):
            an, co = anchor.copy(), corr.copy()
            if plant:
                an[pos], co[pos] = planted, planted[::-1]
            kw = {"anchor": an if has_a else None, "a": a, "corr": co if has_c else None}
            wp, wb, wg, wovf = Dc.drift_ref(p0, gin, b0, *S.SGD_HYPER, first, gs=gs, **kw)
            assert wovf == 1
            (pb, pd), (gb, gd), (sb, sd) = loaded(p0), loaded(gin), galloc(n, S16())
            bb, bd = galloc(n) if first else loaded(b0)
            wbuf, word = galloc(1, torch.int32)
            word.fill_(0)
            _drift_step(pd, gd, bd, sd, n, S.SGD_HYPER, first, gs, word, D(an) if has_a else None, a, D(co) if has_c else None)
            what = "drift guard[n=%d,%s,first=%d,planted=%d] " % (n, kind, first, plant)
            gp, gbuf = npy(pd), npy(bd)
            S.same32(gp, wp, what + "p")
            S.same32(gbuf, wb, what + "buf")
            S.same32(npy(gd), wg, what + "unscaled gradient", nan_ok=True)
            S.same32(gp[pos], p0[pos], what + "p of the skipped elements")
            S.same32(gbuf[pos], np.zeros(len(pos), np.float32) if first else b0[pos], what + "buf of the skipped elements")
            keep = np.ones(n, bool)
            keep[pos] = False
            S.same32(gp[keep], clean_p[keep], what + "p of the others")
            S.same32(gbuf[keep], clean_b[keep], what + "buf of the others")
            T.same16(sd, S.shadow_ref(wp, S16()), what + "mirror")
            assert int(word[0]) == 1, what + "overflow word"
            assert all(guard_ok(b) for b in (pb, gb, bb, sb, wbuf))


# ------------------------------------------------------------------------------------------------ SCAFFOLD's end-of-round pass
@pytest.mark.parametrize("with_corr", [True, False])
@pytest.mark.parametrize("n", Dc.CONTROL_N)
def test_scaffold_control_bit_exact(n, with_corr):
    """c_i updated in place and dc written, bit for bit; x, y and corr unchanged; nothing behind a buffer touched"""
    ci, x, y, corr = Dc.control_inputs(n)
    inv = Dc.inv_mass32(Dc.CONTROL_MASS)
    cn, dc = Dc.scaffold_control_ref(ci, x, y, corr if with_corr else None, inv)
    (cb, cd), (db, dd) = loaded(ci), galloc(n)
    xd, yd, rd = D(x), D(y), D(corr)
    run("fedfr_scaffold_control", cd.data_ptr(), dd.data_ptr(), xd.data_ptr(), yd.data_ptr(), rd.data_ptr() if with_corr else None, float(inv), n)
    what = "scaffold_control[n=%d,corr=%d] " % (n, with_corr)
    S.same32(npy(cd), cn, what + "c_i")
    S.same32(npy(dd), dc, what + "dc")
    assert guard_ok(cb) and guard_ok(db)
    for got, want in ((xd, x), (yd, y), (rd, corr)):
        S.same32(npy(got), want, what + "inputs are read-only")
    if n == 1025:                                                          # the wrapper: same bits, c_i in place, the fp64 mass rounded once
        cd2 = D(ci).clone()
        dc2 = ops.scaffold_control(cd2, xd, yd, rd if with_corr else None, Dc.CONTROL_MASS)
        torch.cuda.synchronize()
        S.same32(npy(cd2), cn, what + "ops.scaffold_control c_i")
        S.same32(npy(dc2), dc, what + "ops.scaffold_control dc")


# ------------------------------------------------------------------------------------------------ argument errors
def test_drift_entry_points_refuse_bad_arguments_before_any_launch():
    n = 64
    bufs = [torch.full((n + 8,), 0.5, dtype=f32, device=DEV) for _ in range(5)]          # p, g, buf, anchor, corr
    sh = torch.full((n + 8,), FILL16, dtype=torch.int16, device=DEV)
    P = [b.data_ptr() for b in bufs]

    def sgd(p, g, b, anchor, prox, corr, n_=n, gs=1.0):
        return rc_of("fedfr_sgd_step_drift", p, g, b, sh.data_ptr(), n_, 0.1, 0.9, 0.0, 1, gs, None, anchor, prox, corr)

    cases = {"no anchor but prox": (None, 0.1, P[4]), "anchor but prox 0": (P[3], 0.0, P[4]), "prox inf": (P[3], float("inf"), None),
             "prox nan": (P[3], NAN, None), "neither": (None, 0.0, None), "misaligned anchor": (P[3] + 4, 0.1, None),
             "misaligned corr": (None, 0.0, P[4] + 4)}
    for what, (an, prox, co) in cases.items():
        assert sgd(P[0], P[1], P[2], an, prox, co) == -1 and "sgd" in _C.last_error(), (what, _C.last_error())
    for bad in range(3):
        ptrs = [P[i] + (4 if i == bad else 0) for i in range(3)]
        assert sgd(*ptrs, P[3], 0.1, P[4]) == -1, "misaligned buffer %d" % bad
    assert sgd(P[0], P[1], P[2], P[3], 0.1, P[4], n_=0) == -1
    assert sgd(P[0], P[1], P[2], P[3], 0.1, P[4], gs=0.0) == -1

    def control(ci, dc, x, y, corr, inv=2.0, n_=n):
        return rc_of("fedfr_scaffold_control", ci, dc, x, y, corr, inv, n_)

    assert control(P[0], P[1], P[2], P[3], P[4], n_=0) == -1
    assert control(P[0], P[0], P[2], P[3], P[4]) == -1                      # c_i and dc are two buffers
    assert control(None, P[1], P[2], P[3], None) == -1 and control(P[0], P[1], None, P[3], None) == -1
    for bad in range(5):
        ptrs = [P[i] + (4 if i == bad else 0) for i in range(5)]
        assert control(*ptrs) == -1 and "scaffold_control" in _C.last_error(), "misaligned buffer %d" % bad
    for inv in (0.0, -1.0, float("inf"), NAN):
        assert control(P[0], P[1], P[2], P[3], P[4], inv=inv) == -1
    assert all(bool((b == 0.5).all()) for b in bufs) and bool((sh == FILL16).all())

    # fedfr_net_backward2_sgd_drift: the drift arguments are refused before the plan is looked at
    m = backbones.iresnet18(False, dropout=0, fp16=True).to(DEV)
    m.load_state_dict(R.closed_form_state_dict(R.IRESNET_LAYERS["iresnet18"], tag=2.0))
    m._ensure_device_state()
    m.train()
    plan = m._plan(4)
    nt = m.trainable_count()
    before = m._flat_params.clone()
    mom = torch.zeros(nt, dtype=f32, device=DEV)
    an, co = torch.zeros(nt + 4, dtype=f32, device=DEV), torch.zeros(nt + 4, dtype=f32, device=DEV)
    x, df = torch.zeros(4, 3, 112, 112, dtype=f32, device=DEV), torch.zeros(4, 512, dtype=f32, device=DEV)
    done = ctypes.c_longlong(-5)

    def net(anchor, prox, corr):
        rc = _C.lib().fedfr_net_backward2_sgd_drift(plan.handle, x.data_ptr(), df.data_ptr(), m._flat_params.data_ptr(), m._shadow.data_ptr(),
                                                    plan.act.data_ptr(), plan.ws.data_ptr(), m._flat_grads.data_ptr(), mom.data_ptr(), 0.1, 0.9,
                                                    0.0, 1, 1.0, None, anchor, prox, corr, ctypes.byref(done), _C.stream(), None)
        torch.cuda.synchronize()
        return rc

    for what, (a_, prox, c_) in {"no anchor but prox": (None, 0.1, co.data_ptr()), "anchor but prox 0": (an.data_ptr(), 0.0, None),
                                 "prox nan": (an.data_ptr(), NAN, None), "neither": (None, 0.0, None),
                                 "misaligned anchor": (an.data_ptr() + 4, 0.1, None), "misaligned corr": (None, 0.0, co.data_ptr() + 4)}.items():
        assert net(a_, prox, c_) == -1 and "net_backward2_sgd_drift" in _C.last_error(), (what, _C.last_error())
    assert done.value == -5 and torch.equal(m._flat_params, before)


# ------------------------------------------------------------------------------------------------ trainers
def _model(arch="iresnet18", tag=5.0):
    if arch == "sphnet":
        m = backbones.sphnet(False, dropout=0, fp16=True, type=20).to(DEV)
        m.load_state_dict(R.sphere_state_dict(20, tag=1.0))
        return m
    m = getattr(backbones, arch)(False, dropout=0, fp16=True)
    m.load_state_dict(R.closed_form_state_dict(R.IRESNET_LAYERS[arch], tag=tag))
    return m.to(DEV)


def _terms(m, prox=0.1):
    """anchor a hundredth away from the loaded parameters, corr a hundredth of a unit: both terms move every element"""
    m._ensure_device_state()
    n = m.trainable_count()
    p = m._flat_params[:n]
    anchor = (p + 0.01 * S.uniform((n,), 4040).to(DEV)).contiguous()
    corr = (0.01 * S.uniform((n,), 4041).to(DEV)).contiguous()
    return client.DriftTerms(anchor, prox, corr)


@pytest.mark.parametrize("which", ["FusedTrainer", "FusedHeadTrainer"])
def test_trainers_with_drift_inside_backward_are_bit_identical_to_the_flat_route(which, monkeypatch):
    """iresnet18 at B = 8 on two streams, anchor + corr, 3 steps: with FEDFR_FUSE_SGD=1 (fedfr_net_backward2_sgd_drift updates the tail and
    the finished stages on the weight-gradient stream, each range with its own slice of anchor and corr) parameters, momentum, mirror,
    gradient buffer and losses equal those of FEDFR_FUSE_SGD=0 (fedfr_net_backward2 + one flat fedfr_sgd_step_drift) bit for bit; and the
    terms do something: the run without them ends elsewhere"""
    monkeypatch.setenv("FEDFR_DUAL_STREAM", "1")
    B, C = 8, 24
    res = []
    for fuse, with_drift in (("1", True), ("0", True), ("1", False)):
        monkeypatch.setenv("FEDFR_FUSE_SGD", fuse)
        m = _model()
        drift = _terms(m) if with_drift else None
        if which == "FusedTrainer":
            fc = R.head_fc(C).to(DEV)
            tr = client.FusedTrainer(m, fc, "CosFace", 30.0, 0.4, lr=0.05, momentum=0.9, weight_decay=5e-4, drift=drift)
            step = tr.step
        else:
            fcm = client.FC_module(512, C, "/tmp").to(DEV)
            fcm.fc.data = R.head_fc(C).to(DEV)
            margin = losses.CosFace(s=30, m=0.4)
            tr = client.FusedHeadTrainer(m, list(fcm.parameters()), lr=0.05, momentum=0.9, weight_decay=5e-4, drift=drift)

            def step(imgs, lab, tr=tr, fcm=fcm, margin=margin):
                return tr.step(imgs, lab, lambda feats, labels: ops.cross_entropy(margin(fcm(feats), labels), labels))
        assert tr.fuse_sgd == (fuse == "1") and tr.aux_stream is not None and (tr.drift is not None) == with_drift
        ls = [float(step(R.closed_form_images(B, tag=float(st)).to(DEV), R.closed_form_labels(B, C, tag=st).to(DEV))) for st in range(3)]
        tr.finish()
        torch.cuda.synchronize()
        n = m.trainable_count()
        assert abs(tr.step_mass - Dc.step_mass([0.05] * 3, 0.9)) < 1e-15
        res.append((ls, m._flat_params.clone(), tr.mom.clone(), m._shadow[:n].clone(), m._flat_grads.clone()))
    a, b, plain = res
    assert a[0] == b[0], (a[0], b[0])
    for i, name in ((1, "parameters"), (2, "momentum"), (3, "mirror"), (4, "gradient buffer")):
        assert torch.equal(a[i], b[i]), name
    assert bool(torch.isfinite(a[1]).all()) and not torch.equal(a[1], plain[1])


@pytest.mark.parametrize("arch,B", [("iresnet18", 8), ("sphnet", 4)])
def test_trainer_step_with_drift_replays_on_the_host(arch, B):
    """iresnet18: one forward_backward() + optimizer_step(); sphnet20 at B = 4: one step(), which takes the flat route (the plan updates
    nothing inside its backward pass).  From the parameters before, the gradient buffer after (true gradients: the guarded kernels of the
    fp16-storage build have undone the loss scale in place) and anchor, prox, corr, drift_ref gives the trainer's new parameters and its
    momentum bit for bit; the loss is the task loss of the same step without the terms.  The update is element-wise, and the host replay of
    24 M elements would take a minute: it covers every 61st element (61 is odd: all four lanes of the float4 body), the first and last 4096
    and 4096 on either side of every range boundary of the fused schedule's flat remainder (iresnet18: stage 2's first parameter)"""
    C = 20
    lr, mu, wd = 0.05, 0.9, 5e-4
    imgs, lab = R.closed_form_images(B, tag=1.0).to(DEV), R.closed_form_labels(B, C, tag=1).to(DEV)
    out = {}
    for with_drift in (True, False):
        m = _model(arch)
        drift = _terms(m, prox=0.25) if with_drift else None
        n = m.trainable_count()
        tr = client.FusedTrainer(m, R.head_fc(C).to(DEV), "CosFace", 30.0, 0.4, lr=lr, momentum=mu, weight_decay=wd, drift=drift)
        p0 = npy(m._flat_params[:n])
        if arch == "sphnet":
            loss = float(tr.step(imgs, lab))
        else:
            loss = float(tr.forward_backward(imgs, lab))
            tr.optimizer_step()
        tr.finish()
        torch.cuda.synchronize()
        out[with_drift] = (loss, p0, npy(m._flat_grads[:n]), npy(m._flat_params[:n]), npy(tr.mom), drift)
    loss, p0, g, p1, buf1, drift = out[True]
    assert loss == out[False][0], "the reported loss is the task loss"
    assert np.isfinite(g).all()
    S.same32(g, out[False][2], "the gradient does not see the terms")
    n = len(p0)
    pick = np.zeros(n, bool)
    pick[::61] = pick[:4096] = pick[-4096:] = True
    if arch != "sphnet":
        first_s2 = dict(m.named_parameters())["layer2.0.bn1.weight"]
        off = (first_s2.data_ptr() - m._flat_params.data_ptr()) // 4
        pick[off - 4096: off + 4096] = True
    idx = np.flatnonzero(pick)
    wp, wb, _, _ = Dc.drift_ref(p0[idx], g[idx], None, lr, mu, wd, 1, anchor=npy(drift.anchor)[idx], a=drift.prox, corr=npy(drift.corr)[idx])
    S.same32(p1[idx], wp, arch + ": parameters after the step")
    S.same32(buf1[idx], wb, arch + ": momentum after the step")
    assert not np.array_equal(p1, out[False][3])
    assert (p1 != p0).mean() > 0.9, "the step moved (nearly) every element"


# ------------------------------------------------------------------------------------------------ rounds
def _tiny_world(aggr, **extra):
    """two clients on the smallest backbone and batch of the server-round tests (iresnet18, B = 4, two steps each): a copy of the helper of
    tests/test_fedopt_gpu.py"""
    class Args:
        network, loss, local_epoch, output_dir, BCE_local, aggr_alg = "iresnet18", "CosFace", 1, "/tmp", False, aggr

    for k_, v_ in extra.items():
        setattr(Args, k_, v_)

    class DS:
        ID_base = 0

    class Loader(list):
        dataset = DS()

    class Data:
        train_class_sizes = [10, 10]
        train_dataset_sizes = [300, 100]
        train_loaders = [Loader([(R.closed_form_images(4, tag=float(c * 2 + s)), R.closed_form_labels(4, 10, tag=c + s))
                                 for s in range(2)]) for c in range(2)]

    from fedfr_amd.config import config as cfg
    cfg.lr = 0.01
    torch.manual_seed(20)                      # the clients draw their class centres (torch.normal): two worlds start from the same ones
    clients = [client.Client(c, Args, Data, device=DEV) for c in range(2)]
    srv = server.Server(clients, Data, Args, device=DEV)
    srv.federated_model.load_state_dict(R.closed_form_state_dict(R.IRESNET_LAYERS["iresnet18"], tag=2.0))
    return srv, clients


def _record_trainers(monkeypatch):
    made = []

    class Recording(client.FusedTrainer):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)
    monkeypatch.setattr(client, "FusedTrainer", Recording)
    return made


def _count_drift_calls(monkeypatch):
    names = []
    real = _C.call

    def counting(name, *args):
        names.append(name)
        return real(name, *args)
    monkeypatch.setattr(_C, "call", counting)
    return names


def _globals(srv):
    """the server's whole flat parameter buffer (its first trainable_count() elements are what the trainers update)"""
    return npy(srv.federated_model.flat_state()[0])


def test_round_with_prox_mu_anchors_every_trainer_at_the_global_parameters(monkeypatch):
    """aggr_alg="FedAvg" with prox_mu = 0.5: every trainer gets anchor = the round's global parameters (a copy: training does not move it),
    prox = prox_mu and no corr, its updates go through the _drift entry points, and the round's result differs from the round without —
    which, with prox_mu absent or 0 (also under aggr_alg="FedProx"), makes no _drift call at all and gives one and the same result"""
    results = {}
    for name, aggr, extra in (("on", "FedAvg", {"prox_mu": 0.5}), ("absent", "FedAvg", {}), ("zero", "FedProx", {"prox_mu": 0.0})):
        with monkeypatch.context() as mp:
            srv, clients = _tiny_world(aggr, **extra)
            made, names = _record_trainers(mp), _count_drift_calls(mp)
            x = _globals(srv)
            assert np.isfinite(srv.train())
            torch.cuda.synchronize()
            ndrift = sum(nm.endswith("_drift") for nm in names)
            assert len(made) == 2
            if name == "on":
                assert ndrift >= 4                                                   # two clients x two steps, at least one call each
                for tr in made:
                    assert tr.drift is not None and tr.drift.prox == 0.5 and tr.drift.corr is None
                    S.same32(npy(tr.drift.anchor), x[:tr.n_train], "anchor of a trainer")
                    assert tr.drift.anchor.data_ptr() != tr.bb._flat_params.data_ptr()
            else:
                assert ndrift == 0 and all(tr.drift is None for tr in made)
                assert not any(nm == "fedfr_scaffold_control" for nm in names)
            results[name] = _globals(srv)
    S.same32(results["absent"], results["zero"], "prox_mu absent and prox_mu = 0")
    assert not np.array_equal(results["on"], results["absent"])


def test_scaffold_two_rounds(monkeypatch):
    """aggr_alg="SCAFFOLD": round 1 trains without corr (c and every c_i are zero) through today's calls, round 2 with corr = c - c_i; after
    each round every c_i and the server's c equal the restatement applied to the recorded x, y_i and step masses (c += fl((1 / N) dc_i),
    ascending i), the uploaded dc_i is the restated one, and the installed model is FedPavg's of the recorded client states, bit for bit"""
    srv, clients = _tiny_world("SCAFFOLD")
    made = _record_trainers(monkeypatch)
    names = _count_drift_calls(monkeypatch)
    uploads = []
    real = server.FedPavg

    def recording(models, weights):
        uploads.append((list(models), list(weights)))
        return real(models, weights)
    monkeypatch.setattr(server, "FedPavg", recording)
    N = len(clients)
    c = cis = None
    mu = client.cfg.momentum
    for rnd in range(2):
        x = _globals(srv)
        del made[:], names[:]
        assert np.isfinite(srv.train())
        srv.step_round()
        torch.cuda.synchronize()
        assert len(made) == 2 and len(uploads) == rnd + 1
        assert sum(nm == "fedfr_scaffold_control" for nm in names) == 2
        assert (sum(nm.endswith("_drift") for nm in names) > 0) == (rnd == 1)
        models, weights = uploads[rnd]
        n = made[0].n_train
        if c is None:
            c, cis = np.zeros(n, np.float32), [np.zeros(n, np.float32) for _ in clients]
        for i, (tr, cl) in enumerate(zip(made, clients)):
            assert abs(tr.step_mass - Dc.step_mass([tr.lr] * 2, mu)) < 1e-15 and tr.step_mass > 0
            corr = None
            if rnd == 0:
                assert tr.drift is None
            else:
                corr = c_before - cis[i]
                S.same32(npy(tr.drift.corr), corr, "corr of client %d in round 2 is c - c_i" % i)
            y = npy(models[i].flat[0][:n])
            cis[i], dc = Dc.scaffold_control_ref(cis[i], x[:n], y, corr, Dc.inv_mass32(tr.step_mass))
            S.same32(npy(cl.scaffold_ci), cis[i], "c_%d after round %d" % (i, rnd + 1))
            S.same32(npy(cl.get_control_update()), dc, "dc_%d of round %d" % (i, rnd + 1))
            c = S.axpy_ref(c, dc, np.float32(1.0 / N), True)
        S.same32(npy(srv.scaffold_c), c, "c after round %d" % (rnd + 1))
        assert float(np.abs(c).max()) > 0
        c_before = c.copy()
        want = real(models, weights)
        torch.cuda.synchronize()
        S.same32(_globals(srv), npy(want.flat[0]), "the installed model is FedPavg's")
        assert not np.array_equal(_globals(srv), x)


@pytest.mark.parametrize("setting", [{"secure_aggregation": True}, {"compress_bits": 8}, {"topk_ratio": 0.1},
                                     {"dp_noise_multiplier": 1.0, "clip_norm": 1.0}, {"clip_norm": 1.0}, {"return_all": True}, {"server_lr": 0.5},
                                     {"prox_mu": -0.1}, {"prox_mu": float("nan")}],
                         ids=["secagg", "compress", "topk", "dp", "clip", "return_all", "server_lr", "prox_negative", "prox_nan"])
def test_scaffold_and_prox_refusals_come_before_any_training(setting, monkeypatch):
    """what SCAFFOLD cannot be combined with (its control updates travel in the clear and unclipped), and a negative or non-finite prox_mu
    under any rule: ValueError from Server.train before a client has trained"""
    aggr = "FedAvg" if "prox_mu" in setting else "SCAFFOLD"
    srv, clients = _tiny_world(aggr, **setting)
    trained = []
    monkeypatch.setattr(client.Client, "train", lambda self, *a, **k: trained.append(self.cid))
    monkeypatch.setattr(client.Client, "train_with_public_data", lambda self, *a, **k: trained.append(self.cid))
    with pytest.raises(ValueError, match="prox_mu" if "prox_mu" in setting else "SCAFFOLD"):
        srv.train()
    assert trained == []
