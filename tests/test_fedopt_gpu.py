"""Server optimisers on the GPU: fedfr_fedopt_multi / fedfr_fedopt_sqnorm through the C ABI against the restatement of
tests/fedopt_cases.py (bit for bit) and its fp64 evaluation, chaining beyond 8 clients, in-place update, argument errors, and the Python
surface (server.FedOpt, Server.train with aggr_alg="FedAvgM", fedavg_all_reduce(server_opt=...))."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import fedopt_cases as F  # noqa: E402
from oracle import ref_cpu as R  # noqa: E402

from fedfr_amd import _C, backbones, client, server  # noqa: E402
from fedfr_amd.comm import SingleComm, ThreadComm  # noqa: E402

DEV = torch.device("cuda:0")
f32, f64 = np.float32, np.float64
SENT = -777.25


def G(a):
    return torch.from_numpy(np.array(a)).to(DEV)          # (a copy: the shared inputs are read-only arrays)


def N(t):
    return t.detach().cpu().numpy()


def sent(n, dtype=torch.float32):
    return torch.full((n,), SENT, dtype=dtype, device=DEV)


def ptr(t):
    return None if t is None else t.data_ptr()


def multi(kind, x_out, x, xs, coef, m, v, h, scratch=None, first=1, last=1):
    """fedfr_fedopt_multi on device tensors; returns the return code"""
    k = len(xs)
    n = (m if x is None else x).numel()
    ptrs = (C.c_void_p * max(k, 1))(*[t.data_ptr() for t in xs])
    return _C.lib().fedfr_fedopt_multi(F.KINDS[kind], ptr(x_out), ptr(x), ptrs, ptr(coef), k, n, ptr(m), ptr(v), ptr(scratch),
                                       first, last, *[float(a) for a in h], _C.stream())


def sqnorm(x, xs, ws, clip, sq, coef, wsp):
    k = len(xs)
    ptrs = (C.c_void_p * max(k, 1))(*[t.data_ptr() for t in xs])
    wv = (C.c_float * max(len(ws), 1))(*[float(w) for w in ws])
    n = (xs[0] if x is None else x).numel()
    return _C.lib().fedfr_fedopt_sqnorm(ptr(x), ptrs, wv, k, n, float(clip), ptr(sq), ptr(coef), ptr(wsp),
                                        0 if wsp is None else wsp.numel() * 8, _C.stream())


def hyper_of(kind):
    return F.hyper(lr=1.0 if kind == "AVGM" else 0.01)


def run_kernel(kind, x, xs, coef, m, v, h, in_place=False):
    xd, xsd = G(x), [G(a) for a in xs]
    md, vd = G(m), (G(v) if kind != "AVGM" else None)
    out = xd if in_place else sent(x.size)
    assert multi(kind, out, xd, xsd, G(np.array(coef, f32)), md, vd, h) == 0, _C.last_error()
    torch.cuda.synchronize()
    return N(md), (None if vd is None else N(vd)), N(out)


def same_bits(got, ref, what):
    assert got.dtype == ref.dtype == f32 and got.shape == ref.shape
    bad = np.flatnonzero(F.bits(got) != F.bits(ref))
    assert bad.size == 0, "%s: %d of %d elements differ, first at %d: %r vs %r" % (what, bad.size, got.size, bad[0], got[bad[0]], ref[bad[0]])


@pytest.mark.parametrize("n", F.SIZES)
@pytest.mark.parametrize("k", F.KS)
@pytest.mark.parametrize("kind", list(F.KINDS))
def test_fedopt_multi_bit_identical_to_the_restatement(kind, k, n):
    """m', v', x' of every kind equal the float32 restatement bit for bit (the kernel's + - * / sqrt are single correctly rounded
    operations in the restatement's order): tail-only sizes, less than one block, and the grid-stride wrap at grid * 256 * 4 + 5"""
    x, xs, m, v = F.inputs(n, k)
    coef, h = F.weights(k), hyper_of(kind)
    m_ref, v_ref, x_ref = F.run32(kind, x, xs, coef, m, v, h)
    m1, v1, x1 = run_kernel(kind, x, xs, coef, m, v, h)
    same_bits(m1, m_ref, "m'")
    if kind != "AVGM":
        same_bits(v1, v_ref, "v'")
    same_bits(x1, x_ref, "x'")


@pytest.mark.parametrize("n", F.SIZES)
@pytest.mark.parametrize("k", F.KS)
@pytest.mark.parametrize("kind", list(F.KINDS))
def test_fedopt_multi_against_fp64(kind, k, n):
    """x' against the fp64 evaluation on inputs without cancellation in Delta, within (k + 16) 2^-24 (|x| + |u| + |m| + sum |coef_i d_i|):
    the bound tests/test_fedopt_cpu.py shows the restatement alone to meet on these very inputs"""
    x, xs, m, v = F.inputs(n, k, same_sign=True)
    coef, h = F.weights(k), hyper_of(kind)
    _, _, x1 = run_kernel(kind, x, xs, coef, m, v, h)
    d, mag = F.delta64(x, xs, coef)
    _, _, X1, u = F.step64(kind, x, m, v, d, h)
    r = float(np.max(np.abs(x1.astype(f64) - X1) / F.fp64_bound(k, x, m, u, mag)))
    print("%s k=%d n=%d: worst error / bound %.3f" % (kind, k, n, r))
    assert r <= 1.0


@pytest.mark.parametrize("total", [9, 17])
@pytest.mark.parametrize("kind", list(F.KINDS))
def test_fedopt_multi_chained_passes(kind, total):
    """more than 8 clients: passes of <= 8 with first / last flags and the scratch Delta are bit-identical to the restatement's single
    ascending loop; a non-last pass writes the scratch buffer only"""
    n = 4103
    x, xs, m, v = F.inputs(n, total)
    coef, h = F.weights(total), hyper_of(kind)
    m_ref, v_ref, x_ref = F.run32(kind, x, xs, coef, m, v, h)
    xd, xsd, cd = G(x), [G(a) for a in xs], G(np.array(coef, f32))
    md, vd, out, scratch = G(m), (G(v) if kind != "AVGM" else None), sent(n), sent(n)
    for c0 in range(0, total, 8):
        last = c0 + 8 >= total
        assert multi(kind, out, xd, xsd[c0:c0 + 8], cd[c0:], md, vd, h, scratch, 1 if c0 == 0 else 0, 1 if last else 0) == 0, _C.last_error()
        if not last:
            torch.cuda.synchronize()
            assert float(out.min()) == SENT == float(out.max()) and np.array_equal(N(md), m) and (vd is None or np.array_equal(N(vd), v))
            same_bits(N(scratch), F.delta32(x, xs[:c0 + 8], coef[:c0 + 8]), "running Delta")
    torch.cuda.synchronize()
    same_bits(N(md), m_ref, "m'")
    if kind != "AVGM":
        same_bits(N(vd), v_ref, "v'")
    same_bits(N(out), x_ref, "x'")


@pytest.mark.parametrize("kind", list(F.KINDS))
def test_fedopt_multi_in_place(kind):
    n, k = F.SIZES[-1], 3
    x, xs, m, v = F.inputs(n, k)
    coef, h = F.weights(k), hyper_of(kind)
    a = run_kernel(kind, x, xs, coef, m, v, h)
    b = run_kernel(kind, x, xs, coef, m, v, h, in_place=True)
    same_bits(b[2], a[2], "x' in place")
    same_bits(b[0], a[0], "m' in place")


@pytest.mark.parametrize("n", F.SIZES)
@pytest.mark.parametrize("k", F.KS)
def test_fedopt_sqnorm(k, n):
    """sq_i within 1e-12 (relative) of numpy's fp64 sum of the same fp32 differences (only the fp64 summation order differs: ~ n 2^-53);
    coef_i within 1 ulp of float32(w_i min(1, clip / sqrt(sq_i))); clip = 0 and an all-zero delta give w_i exactly; two runs, the second
    on a workspace full of NaN, give identical bits"""
    x, xs, _, _ = F.inputs(n, k)
    ws = F.weights(k)
    sq_ref = F.sqnorm(x, xs)
    clip = float(f32(0.75 * np.sqrt(sq_ref.max())))            # the largest update is clipped (with k > 1 usually not all of them)
    xd, xsd = G(x), [G(a) for a in xs]
    nws = _C.lib().fedfr_fedopt_sqnorm_workspace_bytes(k, n)
    assert nws == 8 * k * F.grid(n)
    wsp = torch.zeros(nws // 8, dtype=torch.float64, device=DEV)
    sq, coef = sent(k, torch.float64), sent(k)
    assert sqnorm(xd, xsd, ws, clip, sq, coef, wsp) == 0, _C.last_error()
    torch.cuda.synchronize()
    sq1, coef1 = N(sq), N(coef)
    rel = np.abs(sq1 - sq_ref) / sq_ref
    print("k=%d n=%d: sq rel err %.2e" % (k, n, rel.max()))
    assert np.all(rel <= 1e-12)
    cref = F.clip_coef(sq_ref, ws, clip)
    assert np.all(np.abs(coef1.astype(f64) - cref.astype(f64)) <= np.spacing(cref).astype(f64)), (coef1, cref)
    assert coef1[int(np.argmax(sq_ref))] < ws[int(np.argmax(sq_ref))]
    # second run: same bits, whatever the workspace held
    wsp.fill_(float("nan"))
    sq2, coef2 = sent(k, torch.float64), sent(k)
    assert sqnorm(xd, xsd, ws, clip, sq2, coef2, wsp) == 0
    torch.cuda.synchronize()
    assert np.array_equal(N(sq2).view(np.uint64), sq1.view(np.uint64)) and np.array_equal(F.bits(N(coef2)), F.bits(coef1))
    # clip = 0: the weights themselves; a zero delta: sq == 0 and the weights themselves
    assert sqnorm(xd, xsd, ws, 0.0, sq, coef, wsp) == 0
    torch.cuda.synchronize()
    assert np.array_equal(N(coef), np.array(ws, f32)) and np.array_equal(N(sq).view(np.uint64), sq1.view(np.uint64))
    assert sqnorm(xd, [xd] * k, ws, 1.0, sq, coef, wsp) == 0
    torch.cuda.synchronize()
    assert np.array_equal(N(coef), np.array(ws, f32)) and np.all(N(sq) == 0.0)


def test_fedopt_argument_errors_launch_nothing():
    """every bad argument here is one the host-side checks refuse before a launch: negative return code, a message, outputs untouched"""
    n, k = 1023, 2
    x, xs, m, v = F.inputs(n, k)
    xd, xsd, md, vd, cd = G(x), [G(a) for a in xs], G(m), G(v), G(np.array(F.weights(k), f32))
    out, h = sent(n), hyper_of("ADAM")
    lib = _C.lib()

    def refused(rc, word):
        assert rc < 0
        assert word in _C.last_error(), _C.last_error()

    refused(multi("ADAM", out, None, xsd, cd, md, vd, h), "fedopt_multi")                  # null x
    refused(multi("ADAM", None, xd, xsd, cd, md, vd, h), "fedopt_multi")                   # null x_out on a last pass
    refused(multi("ADAM", out, xd, xsd, cd, md, None, h), "fedopt_multi")                  # adaptive kind without v
    refused(multi("ADAM", out, xd, xsd, None, md, vd, h), "fedopt_multi")                  # null coef
    refused(multi("ADAM", out, xd, [], cd, md, vd, h), "k=0")
    refused(multi("ADAM", out, xd, xsd * 5, cd, md, vd, h), "k=10")
    refused(multi("ADAM", out, xd, xsd * 4 + xsd[:1], cd, md, vd, h), "k=9")
    refused(multi("ADAM", out, xd, [xsd[0], xsd[1][1:]], cd, md, vd, h), "aligned")        # client state 4 bytes off
    refused(multi("ADAM", out[1:], xd, xsd, cd, md, vd, h), "aligned")
    refused(multi("ADAM", out, xd, xsd, cd, md, vd, h, None, 0, 1), "scratch")             # a chained pass without the scratch buffer
    refused(multi("ADAM", out, xd, xsd, cd, md, vd, h, None, 1, 0), "scratch")
    ptrs = (C.c_void_p * 2)(xsd[0].data_ptr(), None)
    for kind in (-1, 4):
        refused(lib.fedfr_fedopt_multi(kind, out.data_ptr(), xd.data_ptr(), ptrs, cd.data_ptr(), 1, n, md.data_ptr(), vd.data_ptr(), None, 1, 1,
                                       *[float(a) for a in h], _C.stream()), "kind")
    refused(lib.fedfr_fedopt_multi(2, out.data_ptr(), xd.data_ptr(), ptrs, cd.data_ptr(), 2, n, md.data_ptr(), vd.data_ptr(), None, 1, 1,
                                   *[float(a) for a in h], _C.stream()), "null")           # null client pointer
    refused(lib.fedfr_fedopt_multi(2, out.data_ptr(), xd.data_ptr(), ptrs, cd.data_ptr(), 1, 0, md.data_ptr(), vd.data_ptr(), None, 1, 1,
                                   *[float(a) for a in h], _C.stream()), "fedopt_multi")   # n = 0
    sq, coef = sent(k, torch.float64), sent(k)
    wsp = torch.zeros(k * F.grid(n), dtype=torch.float64, device=DEV)
    ws = F.weights(k)
    refused(sqnorm(None, xsd, ws, 1.0, sq, coef, wsp), "fedopt_sqnorm")
    refused(sqnorm(xd, xsd, ws, 1.0, None, coef, wsp), "fedopt_sqnorm")
    refused(sqnorm(xd, xsd, ws, 1.0, sq, coef, None), "fedopt_sqnorm")
    refused(sqnorm(xd, [], ws, 1.0, sq, coef, wsp), "k=0")
    refused(sqnorm(xd, xsd * 5, ws * 5, 1.0, sq, coef, wsp), "k=10")
    refused(sqnorm(xd[1:], [a[1:] for a in xsd], ws, 1.0, sq, coef, wsp), "aligned")
    refused(sqnorm(xd, xsd, ws, 1.0, sq, coef, wsp[:k * F.grid(n) - 1]), "workspace")
    assert sqnorm(xd, xsd, ws, 1.0, sq, coef, wsp[:k * F.grid(n) - 1]) == -3               # FEDFR_ERR_WORKSPACE
    torch.cuda.synchronize()
    assert float(out.min()) == SENT == float(out.max()) and float(sq.min()) == SENT == float(coef.max())
    assert np.array_equal(N(md), m) and np.array_equal(N(vd), v) and np.array_equal(N(xd), x)


# ---- server.FedOpt ---------------------------------------------------------------------------------------------------------------------
def _closed_form_backbone(tag):
    m = backbones.iresnet18(False, dropout=0, fp16=True)
    m.load_state_dict(R.closed_form_state_dict(R.IRESNET_LAYERS["iresnet18"], tag=tag))
    return m.to(DEV)


@pytest.fixture(scope="module")
def states():
    """the global state of a closed-form iresnet18 and three client states: its flat tensors perturbed in closed form (no training)"""
    g = client.flat_state_dict(_closed_form_backbone(2.0))
    p, b, c = g.flat
    j = torch.arange(p.numel(), device=DEV, dtype=torch.float64)
    jb = torch.arange(b.numel(), device=DEV, dtype=torch.float64)
    models = []
    for i in range(3):
        pi = (p.double() + 1e-3 * (i + 1) * torch.sin(0.0137 * (i + 1) * j + 0.4 * i)).float()
        bi = (b.double() * (1.0 + 0.05 * i) + 0.01 * torch.sin(0.3 * jb + i)).float()
        models.append(client.FlatStateDict.from_flat((pi, bi, c + 3 * i + 1), g.table, g.layers))
    return g, models, [300.0, 100.0, 250.0]


@pytest.mark.parametrize("kind", ["AVGM", "YOGI"])
def test_fedopt_end_to_end(states, kind):
    """parameters == the restatement (with the coefficients the norm kernel produced, themselves within 1 ulp of the numpy ones and one
    client clipped); running statistics and counters bit-identical to FedPavg; the moments persist into a second call"""
    g, models, sizes = states
    x, xs = N(g.flat[0]), [N(m.flat[0]) for m in models]
    ws = [f32(s / sum(sizes)) for s in sizes]
    sq_ref = F.sqnorm(x, xs)
    clip = float(f32(0.5 * (np.sqrt(sq_ref[1]) + np.sqrt(sq_ref[2]))))      # update norms grow with the client index: client 2 is clipped
    opt = server.ServerOptimizer(kind, lr=1.0 if kind == "AVGM" else 0.01, clip_norm=clip)
    out = server.FedOpt(g, models, sizes, opt)
    avg = server.FedPavg(models, sizes)
    torch.cuda.synchronize()
    assert isinstance(out, client.FlatStateDict) and opt.rounds == 1
    assert torch.equal(out.flat[1], avg.flat[1]) and torch.equal(out.flat[2], avg.flat[2]) and out.flat[2].dtype == torch.float32
    sq, coef = N(opt.last_update_sqnorm), N(opt.last_coef)
    assert np.all(np.abs(sq - sq_ref) <= 1e-12 * sq_ref)
    cref = F.clip_coef(sq_ref, ws, clip)
    assert np.all(np.abs(coef.astype(f64) - cref.astype(f64)) <= np.spacing(cref).astype(f64))
    assert coef[0] == ws[0] and coef[1] == ws[1] and coef[2] < ws[2]
    h = F.hyper(opt.lr, opt.beta1, opt.beta2, opt.tau)
    t = h[5]
    m0, v0 = np.zeros_like(x), np.full_like(x, t * t)
    m1, v1, x1 = F.run32(kind, x, xs, coef, m0, v0, h)
    same_bits(N(out.flat[0]), x1, "x'")
    same_bits(N(opt.m), m1, "m'")
    if kind != "AVGM":
        same_bits(N(opt.v), v1, "v'")
    # second round from the new global state: the moments carry over
    out2 = server.FedOpt(out, models, sizes, opt)
    torch.cuda.synchronize()
    coef2 = N(opt.last_coef)
    m2, v2, x2 = F.run32(kind, x1, xs, coef2, m1, v1, h)
    same_bits(N(out2.flat[0]), x2, "x'' (second round)")
    assert opt.rounds == 2 and out["conv1.weight"].shape == g["conv1.weight"].shape
    with pytest.raises(RuntimeError):
        server.FedOpt(g, [dict(m) for m in models], sizes, opt)            # plain dicts: refused, no generic path
    with pytest.raises(RuntimeError):
        server.FedOpt(g, models, sizes[:2], opt)


def test_fedopt_avgm_without_momentum_matches_fedpavg(states):
    """AVGM, beta1 = 0, lr = 1, no clip is FedAvg: parameters within (k + 3) 2^-24 (|x| + sum |w_i| |x_i - x|) of the fp64 weighted mean
    and of FedPavg (the bound of tests/test_fedopt_cpu.py::test_avgm_without_momentum_is_the_weighted_mean), everything else bit-identical"""
    g, models, sizes = states
    opt = server.ServerOptimizer("AVGM", lr=1.0, beta1=0.0)
    out = server.FedOpt(g, models, sizes, opt)
    avg = server.FedPavg(models, sizes)
    torch.cuda.synchronize()
    assert torch.equal(out.flat[1], avg.flat[1]) and torch.equal(out.flat[2], avg.flat[2])
    k = len(models)
    x = g.flat[0].double()
    ws = [float(f32(s / sum(sizes))) for s in sizes]
    mean = sum(w * m.flat[0].double() for w, m in zip(ws, models))
    bound = (k + 3) * F.U * (x.abs() + sum(w * (m.flat[0].double() - x).abs() for w, m in zip(ws, models)))
    err = (out.flat[0].double() - mean).abs()
    print("FedOpt(AVGM, beta1=0) vs the fp64 weighted mean: worst error / bound %.3f" % float((err / bound).max()))
    assert bool((err <= bound).all())
    assert bool(((out.flat[0].double() - avg.flat[0].double()).abs() <= bound).all())
    assert torch.equal(N_t(opt.last_coef), torch.tensor(ws, dtype=torch.float32))


def N_t(t):
    return t.detach().cpu()


# ---- Server.train ------------------------------------------------------------------------------------------------------------------------
def _tiny_world(aggr, **extra):
    """two clients on the smallest backbone and batch of the server-round tests of tests/test_e2e_gpu.py (iresnet18, B = 4, two steps each)"""
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


def test_server_train_fedavgm_two_rounds(monkeypatch):
    """aggr_alg="FedAvgM": the global parameters after round 2 equal the restatement applied to the recorded client states of both rounds
    with ONE momentum buffer carried across them (the optimiser lives on the server)"""
    srv, _ = _tiny_world("FedAvgM", server_lr=0.5, server_momentum=0.75)
    rec = []
    real = server.FedOpt

    def recording(global_state, models, weights, opt):
        rec.append((N(global_state.flat[0]), [N(m.flat[0]) for m in models], list(weights)))
        return real(global_state, models, weights, opt)
    monkeypatch.setattr(server, "FedOpt", recording)
    for _ in range(2):
        assert np.isfinite(srv.train())
        srv.step_round()
    torch.cuda.synchronize()
    opt = srv.server_opt
    assert len(rec) == 2 and opt.kind == "AVGM" and opt.rounds == 2 and (opt.lr, opt.beta1, opt.clip_norm) == (0.5, 0.75, 0.0)
    h = F.hyper(0.5, 0.75)
    m = np.zeros_like(rec[0][0])
    x = rec[0][0]
    for r, (xg, xs, weights) in enumerate(rec):
        same_bits(xg, x, "global parameters entering round %d" % r)
        coef = [f32(w / sum(weights)) for w in weights]
        m, _, x = F.run32("AVGM", xg, xs, coef, m, None, h)
        assert not np.array_equal(xs[0], xs[1])
    same_bits(N(srv.federated_model.flat_state()[0]), x, "global parameters after round 2")
    same_bits(N(opt.m), m, "momentum after round 2")
    assert float(np.abs(m).max()) > 0


def test_server_train_fedavg_path_is_untouched(monkeypatch):
    """aggr_alg="FedAvg" still calls FedPavg and nothing of the server optimisers: two rounds through Server.train give the bits of the
    same two rounds written out by hand with FedPavg"""
    calls = {"pavg": 0, "opt": 0}
    real = server.FedPavg
    monkeypatch.setattr(server, "FedPavg", lambda *a: (calls.__setitem__("pavg", calls["pavg"] + 1), real(*a))[1])
    monkeypatch.setattr(server, "FedOpt", lambda *a: calls.__setitem__("opt", calls["opt"] + 1))
    srv, _ = _tiny_world("FedAvg")
    for _ in range(2):
        srv.train()
        srv.step_round()
    assert calls == {"pavg": 2, "opt": 0} and srv.server_opt is None
    ref, clients = _tiny_world("FedAvg")
    epoch = 0
    for _ in range(2):
        for c in clients:
            c.slot = 0
            c.backbone_state_dict = client.flat_state_dict(ref.federated_model)
            c.local_epoch = ref.local_epoch
            c.train(epoch)
        ref.federated_model.load_state_dict(real([c.get_model() for c in clients], [c.get_data_size() for c in clients]))
        epoch += ref.local_epoch
    torch.cuda.synchronize()
    for a, b in zip(srv.federated_model.flat_state(), ref.federated_model.flat_state()):
        assert torch.equal(a, b)


# ---- fedavg_all_reduce(server_opt=...) -----------------------------------------------------------------------------------------------------
def _allreduce_case(world):
    sizes = [300.0, 100.0][:world]
    g = client.flat_state_dict(_closed_form_backbone(3.0))
    models = [_closed_form_backbone(float(r + 1)) for r in range(world)]
    for r, m in enumerate(models):
        m._flat_nbt += 3 * r
    local = [client.flat_state_dict(m) for m in models]
    expect_opt = server.ServerOptimizer("AVGM", lr=1.0, beta1=0.9)
    expect = server.FedOpt(g, local, sizes, expect_opt)
    opts = [server.ServerOptimizer("AVGM", lr=1.0, beta1=0.9) for _ in range(world)]
    prev = g.flat[0]

    def run(c):
        return server.fedavg_all_reduce(models[c.rank], sizes[c.rank], sum(sizes), c, server_opt=opts[c.rank], prev_params=prev)
    if world == 1:
        run(SingleComm())
    else:
        ThreadComm.run(world, run, device=DEV)
    torch.cuda.synchronize()
    for r in range(1, world):                                  # replicated moments, one model
        assert torch.equal(models[r]._flat_state, models[0]._flat_state) and torch.equal(opts[r].m, opts[0].m)
    got = client.flat_state_dict(models[0])
    assert torch.equal(got.flat[1], expect.flat[1])            # running statistics: the plain mean, as FedPavg
    assert torch.equal(got.flat[2], expect.flat[2].to(torch.int64))
    return g, local, sizes, got, expect, opts[0], expect_opt


def test_allreduce_server_opt_world1():
    """SingleComm: the exchange is the identity (weight 1.0), Delta = 1 * (x_1 - x): the very operations of FedOpt with one client"""
    _, _, _, got, expect, opt, expect_opt = _allreduce_case(1)
    assert torch.equal(got.flat[0], expect.flat[0]) and torch.equal(opt.m, expect_opt.m) and opt.rounds == 1
    with pytest.raises(ValueError, match="clip_norm"):
        server.fedavg_all_reduce(None, 1.0, 1.0, SingleComm(), server_opt=server.ServerOptimizer("AVGM", clip_norm=2.0), prev_params=expect.flat[0])
    with pytest.raises(ValueError, match="prev_params"):
        server.fedavg_all_reduce(None, 1.0, 1.0, SingleComm(), server_opt=server.ServerOptimizer("AVGM"))


def test_allreduce_server_opt_world2():
    """ThreadComm, two thread-ranks on one GPU, against FedOpt over the same client states.  The bound is the one
    tests/test_multirank_gpu.py::test_fedavg_all_reduce_real_kernels_four_ranks uses for FedAvg over ThreadComm against FedPavg:
    ``torch.equal`` — 0, bit for bit, "because the in-process communicator adds in ascending rank order like server.py:27-33".  It carries
    over because the exchange moves w_i (x_i - x) with FedOpt's own roundings of that term, and the communicator adds the terms in
    FedOpt's order; the moments are replicated bit for bit as well."""
    _, _, _, got, expect, opt, expect_opt = _allreduce_case(2)
    ndiff = int((got.flat[0] != expect.flat[0]).sum())
    print("all-reduce + server optimiser vs FedOpt, world 2: %d of %d parameters differ" % (ndiff, got.flat[0].numel()))
    assert torch.equal(got.flat[0], expect.flat[0])
    assert torch.equal(opt.m, expect_opt.m) and opt.rounds == 1
