"""Server.SpreadOut / SpreadOut_Module (fedfr_amd/server.py, kernels in fedfr_amd/csrc/spreadout.hip) against the reference's
server.SpreadOut_Module + torch.optim.SGD loop (server.py:48-63, :340-371), captured in tests/golden/spreadout.npz by tools/make_golden.py.

Closed form restated here in fp64 (c = 1 for 'sum', 1 / (N (N - 1)) for 'mean'; H_ij = relu(S_ij - margin), H_ii = 0):
    loss = c sum H^2,   dFn = 4c H Fn,   dFC_i = (dFn_i - Fn_i <Fn_i, dFn_i>) / max(|FC_i|, eps)

Bounds.  CPU: the fixture is the reference in fp32, the restatement fp64; the reference's fp32 loop was measured within 2.0e-6 (update) and
4.2e-7 (losses) of its own fp64 run when the feature was specified, the test asserts 1e-5 (five times that: the fixture cases are not the
probed ones).  GPU: the kernel and the reference's fp32 formulation are fp32 sums of the same D products in another order, so the bound on
the kernel's error against fp64 is four times the error of the reference's fp32 formulation on the same input (computed in the test, or
stored in the fixture for the loops), and never above the project's fp32 bar of 1e-3.  All parity is taken on gradients and on the update
FC_after - FC_before, never on FC itself (in 'mean' mode most of the motion of FC is weight decay).  Every figure is printed before it
is asserted."""
import ctypes as C
import importlib.util
import logging
import os
import types

import numpy as np
import pytest
import torch

from conftest import REPO, load_golden

MARGIN = 0.4
FP32_BAR = 1e-3
GEN_KEYS = ("amp", "a", "b", "c", "every", "w0", "w1")
f64 = torch.float64


# ---- closed-form inputs and the fp64 restatement ------------------------------------------------------------------------------------------
def closed_form_fc(N, D, amp, a, b, c, every, w0, w1):
    """tools/make_golden.py spreadout_fc: amp sin(a i (j + 1) + b j + c i), every `every`-th row of the upper half mixed with row r - N/2."""
    i, j = np.arange(N, dtype=np.float64)[:, None], np.arange(D, dtype=np.float64)[None, :]
    fc = amp * np.sin(a * i * (j + 1) + b * j + c * i)
    base = fc.copy()
    for r in range(N // 2, N):
        if r % every == 0:
            w = abs(w0 + w1 * np.sin(float(r)))
            fc[r] = w * base[r - N // 2] + (1 - w) * base[r]
    return torch.from_numpy(fc.astype(np.float32))


def restate_fn(fn, margin, mean, rows=None, chunk=2048):
    """(loss, dFn, active) of normalised rows `fn` in fp64 on fn's device, S in row chunks; `rows`: dFn for these rows only."""
    fn = fn.to(f64)
    N = fn.shape[0]
    c = 1.0 / (N * (N - 1.0)) if mean else 1.0
    dfn = torch.zeros_like(fn) if rows is None else None
    loss, active = torch.zeros((), dtype=f64, device=fn.device), 0
    for r0 in range(0, N, chunk):
        s = fn[r0:r0 + chunk] @ fn.T
        k = torch.arange(s.shape[0], device=fn.device)
        s[k, k + r0] = -2.0
        h = (s - margin).clamp_min_(0)
        loss += (h * h).sum()
        active += int((s > margin).sum())
        if rows is None:
            dfn[r0:r0 + chunk] = 4 * c * (h @ fn)
    if rows is not None:
        s = fn[rows] @ fn.T
        s[torch.arange(len(rows), device=fn.device), rows] = -2.0
        dfn = 4 * c * ((s - margin).clamp_min_(0) @ fn)
    return c * loss, dfn, active


def restate_fc(fc, margin, mean):
    """(loss, dFC, dFn, Fn, active) from unnormalised centres, fp64."""
    fc = fc.to(f64)
    n = fc.norm(dim=1, keepdim=True).clamp_min(1e-12)
    fn = fc / n
    loss, dfn, active = restate_fn(fn, margin, mean)
    return loss, (dfn - fn * (fn * dfn).sum(1, keepdim=True)) / n, dfn, fn, active


def restate_loop(fc0, mean, iters, lr, wd, margin=MARGIN):
    """The loop of Server.SpreadOut (torch.optim.SGD: coupled weight decay, momentum 0.9, first step buf = g) in fp64."""
    fc, buf, losses = fc0.to(f64).clone(), None, []
    for _ in range(iters):
        loss, g, _, _, _ = restate_fc(fc, margin, mean)
        losses.append(float(loss))
        g = g + wd * fc
        buf = g.clone() if buf is None else 0.9 * buf + g
        fc = fc - lr * buf
    return np.array(losses), fc


def rel(a, b):
    a, b = torch.as_tensor(a).to(f64).cpu(), torch.as_tensor(b).to(f64).cpu()
    return float((a - b).norm() / b.norm())


def fixture():
    z = load_golden("spreadout")
    return {k: z[k] for k in z.files}


def cases(z):
    for name in z["cases"]:
        name = str(name)
        nc, ids, D = (int(v) for v in z[name + "_shape"])
        yield name, nc, ids, D, str(z[name + "_mode"]), int(z[name + "_iters"]), float(z[name + "_cfg_lr"])


def gen_params(z):
    g = {k: float(z["gen_" + k]) for k in GEN_KEYS}
    g["every"] = int(g["every"])
    return g


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------
def test_restatement_reproduces_reference():
    z = fixture()
    wd = float(z["weight_decay"])
    assert abs(float(z["margin"]) - MARGIN) < 1e-12
    worst = {}
    for name, nc, ids, D, mode, iters, lr, in cases(z):
        N = nc * ids
        fc0 = closed_form_fc(N, D, **gen_params(z))
        losses, fc = restate_loop(fc0, mode == "mean", iters, lr * 10, wd)
        _, g0, _, fn, active = restate_fc(fc0, MARGIN, mode == "mean")
        rows = torch.from_numpy(z[name + "_rows"])
        upd = fc - fc0.to(f64)
        fin = torch.from_numpy(z[name + "_final"]).to(f64)
        upd_ref = fin - fc0.to(f64) if fin.shape[0] == N else fin - fc0.to(f64)[rows]
        e = {"loss": float(np.max(np.abs(losses - z[name + "_losses"]) / np.abs(z[name + "_losses"]))),
             "grad0": rel(g0[rows], z[name + "_grad0"]), "grad0_rownorm": rel(g0.norm(dim=1), z[name + "_grad0_rownorm"]),
             "update": rel(upd if fin.shape[0] == N else upd[rows], upd_ref),
             "update_rownorm": rel(upd.norm(dim=1), z[name + "_update_rownorm"])}
        print(name, e)
        worst[name] = e
        assert max(e.values()) <= 1e-5, "fp64 restatement vs the reference's fp32 loop, %s: %r (bound 1e-5)" % (name, e)
        # fixture properties
        frac = int(z[name + "_active"]) / (N * (N - 1.0))
        assert 1e-4 <= frac <= 1e-2, (name, frac)
        assert float(z[name + "_not_wd"]) >= 0.01, (name, float(z[name + "_not_wd"]))
        if mode == "sum":
            assert z[name + "_losses"][0] > 10 * z[name + "_losses"][-1], (name, z[name + "_losses"])
        band = D * 2.0 ** -24
        if float(z[name + "_gap0"]) > band:
            assert active == int(z[name + "_active"]), (name, active, int(z[name + "_active"]))
        else:
            print("%s: a pair lies within %.1e of the margin (fp32 dot-product error %.1e): active count not comparable" %
                  (name, float(z[name + "_gap0"]), band))
            assert False, "the generator must keep every first-iteration pair outside the fp32 error band of the margin"


@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__ as ge
    ge.build()
    from fedfr_amd import _C
    return _C


def test_spreadout_kernels_do_not_spill(built_lib):
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(REPO, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    libdir = os.path.dirname(built_lib.LIB_PATH)
    for name in ("libfedfr_hip.so", "libfedfr_hip_bf16.so"):
        ks = kr.kernels(os.path.join(libdir, name))
        for k in ("spreadout_tile_kernel", "spreadout_reduce_kernel"):
            found = [(n, r) for n, r in ks.items() if k in n]
            assert len(found) == 1, (name, k, found)
            assert all(r["scratch"] == 0 for _, r in found), (name, found)


def test_abi_workspace_and_bad_arguments(built_lib):
    """Argument checks run on the host before anything is enqueued (no GPU needed)."""
    lib = built_lib.lib()
    wsb = lib.fedfr_spreadout_workspace_bytes
    N, D = 85000, 512
    assert 0 < wsb(N, D) <= 2 * N * D * 4 + (1 << 20), wsb(N, D)      # "never materialised": N^2 fp32 would be 29 GB
    sizes = [wsb(n, D) for n in (2, 64, 65, 4000, 4001, 85000)]
    assert all(s > 0 for s in sizes) and sizes == sorted(sizes), sizes
    d = 1 << 20                                                         # never dereferenced: every call below fails its checks first

    def call(N=100, D=128, mean=0, short=0, null=None):
        need = max(wsb(N, D), 16)
        p = {n: (None if n == null else d) for n in ("fn", "dfn", "loss", "ws")}
        rc = lib.fedfr_spreadout_grad(p["fn"], N, D, 0.4, mean, p["dfn"], p["loss"], None, p["ws"], need - short, None)
        return rc, lib.fedfr_last_error_string().decode()

    for kw, word in ((dict(N=1), "N = 1"), (dict(N=0), "N = 0"), (dict(D=6), "D = 6"), (dict(D=1028), "D = 1028"), (dict(D=0), "D = 0"),
                     (dict(null="fn"), "null"), (dict(null="dfn"), "null"), (dict(null="loss"), "null"), (dict(null="ws"), "workspace"),
                     (dict(short=1), "workspace"), (dict(mean=2), "mean")):
        rc, msg = call(**kw)
        assert rc != 0 and word in msg and "spreadout_grad" in msg, (kw, rc, msg)
    for n, dd in ((1, 128), (100, 6), (100, 2048)):
        assert wsb(n, dd) == 0


def test_module_rejects_unknown_mode():
    from fedfr_amd.server import SpreadOut_Module
    with pytest.raises(ValueError, match="mode"):
        SpreadOut_Module(torch.zeros(4, 8), mode="max")


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------
def _dev():
    return torch.device("cuda:0")


def basis_case(N, D, seed):
    """Rows that are signed unit basis vectors or zero, scattered over the tiles: axis k < min(D, N // 2) carries 2 .. 4 rows with the signs
    (+, +, -, +), the other rows are zero.  Returns (fn [N, D] fp32, cnt [N] = rows j != i equal to row i)."""
    rng = np.random.default_rng(seed)
    order = rng.permutation(N)
    fn, cnt = np.zeros((N, D), np.float32), np.zeros(N, np.int64)
    signs = (1.0, 1.0, -1.0, 1.0)
    o = 0
    for k in range(D):
        g = min(2 + (k % 3), N - o)
        if g < 2:
            break
        for t in range(g):
            fn[order[o + t], k] = signs[t]
            cnt[order[o + t]] = sum(1 for u in range(g) if u != t and signs[u] == signs[t])
        o += g
    return fn, cnt


@pytest.mark.gpu
@pytest.mark.parametrize("margin", [0.4, 0.7])
@pytest.mark.parametrize("N,D", [(2, 4), (3, 4), (63, 128), (65, 4), (65, 512), (257, 128), (257, 1024), (1000, 4), (1000, 512), (1000, 1024)])
def test_known_answers(N, D, margin):
    from fedfr_amd import ops
    fn_np, cnt = basis_case(N, D, seed=N * 31 + D)
    assert cnt.sum() > 0
    fn = torch.from_numpy(fn_np).to(_dev())
    h = float(np.float32(1.0) - np.float32(margin))                     # the fp32 hinge value of a duplicate pair, as a double
    for mean in (False, True):
        c = 1.0 / (N * (N - 1.0)) if mean else 1.0
        loss, dfn, active = ops.spreadout_loss_grad(fn, margin, mean)
        torch.cuda.synchronize()
        assert int(active) == int(cnt.sum()), (int(active), int(cnt.sum()))
        want_loss = c * float(cnt.sum()) * h * h
        err_loss = abs(float(loss) - want_loss) / want_loss
        want = 4 * c * h * cnt[:, None].astype(np.float64) * fn_np.astype(np.float64)
        got = dfn.cpu().numpy().astype(np.float64)
        ulp = np.abs(got - want) / np.maximum(np.abs(want) * 2.0 ** -23, 1e-300)
        print("N %d D %d margin %.1f mean %d: loss rel err %.2e, dFn max err %.2f ulp" % (N, D, margin, mean, err_loss, ulp.max()))
        assert err_loss <= 2.0 ** -23, (float(loss), want_loss)
        assert np.array_equal(got == 0, want == 0)
        assert ulp.max() <= 4.0, ulp.max()


def planted_unit_rows(N, D, frac, seed, dev):
    """Random unit rows; a fraction `frac` of them are near-duplicates (cosine 0.5 .. 0.95) of a source row of their own.
    Returns (rows, indices of the near-duplicates followed by their sources)."""
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.randn(N, D, generator=g, device=dev, dtype=torch.float32)
    x /= x.norm(dim=1, keepdim=True)
    n = max(2, int(N * frac))
    perm = torch.randperm(N, generator=g, device=dev)
    dst, src = perm[:n], perm[n:2 * n]
    t = torch.linspace(0.5, 0.95, n, device=dev)[:, None]
    x[dst] = t * x[src] + (1 - t * t).sqrt() * x[dst]
    return x.contiguous(), torch.cat([dst, src])


def reference_fp32(fc, margin, mean, leaf_is_fn):
    """The reference's formulation (server.py:55-63) as plain torch ops in the dtype of `fc`, S materialised: (loss, gradient on the leaf)."""
    x = fc.detach().clone().requires_grad_(True)
    fn = x if leaf_is_fn else torch.nn.functional.normalize(x)
    s = fn @ fn.t()
    l = torch.relu(s.masked_select(~torch.eye(len(x), dtype=torch.bool, device=x.device)) - margin) ** 2
    loss = l.mean() if mean else l.sum()
    loss.backward()
    return loss.detach(), x.grad


def _parity_one_step(fc, mean, what):
    from fedfr_amd import ops
    from fedfr_amd.server import SpreadOut_Module
    fn, inv = ops.normalize_rows(fc)
    loss, dfn, active = ops.spreadout_loss_grad(fn, MARGIN, mean)
    mod = SpreadOut_Module(fc.clone(), margin=MARGIN, mode="mean" if mean else "sum")
    l2 = mod()
    l2.backward()
    dfc = mod.FC.grad
    # fp64 truth and the reference's fp32 error, on the same inputs: Fn for dFn and the loss, FC for dFC
    l64, dfn64, act64 = restate_fn(fn, MARGIN, mean)
    lr32, dfn32 = reference_fp32(fn, MARGIN, mean, True)
    l64fc, dfc64, _, _, _ = restate_fc(fc, MARGIN, mean)
    lfc32, dfc32 = reference_fp32(fc, MARGIN, mean, False)
    e = {"dFn": (rel(dfn, dfn64), rel(dfn32, dfn64)), "loss": (abs(float(loss) - float(l64)) / float(l64), abs(float(lr32) - float(l64)) / float(l64)),
         "dFC": (rel(dfc, dfc64), rel(dfc32, dfc64)), "loss(FC)": (abs(float(l2.detach()) - float(l64fc)) / float(l64fc), abs(float(lfc32) - float(l64fc)) / float(l64fc))}
    for k, (mine, ref) in e.items():
        print("%s mean=%d %-8s kernel %.3e   reference fp32 %.3e   (bound %.3e)" % (what, mean, k, mine, ref, min(4 * ref, FP32_BAR)))
    assert int(active) == act64, (int(active), act64)
    for k, (mine, ref) in e.items():
        assert mine <= min(4 * ref, FP32_BAR), (what, mean, k, mine, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("mean", [False, True])
def test_parity_one_step_fixture_inputs(mean):
    z = fixture()
    for nc, ids, D in ((6, 80, 128), (12, 100, 512)):
        _parity_one_step(closed_form_fc(nc * ids, D, **gen_params(z)).to(_dev()), mean, "fixture %dx%d" % (nc * ids, D))


@pytest.mark.gpu
@pytest.mark.parametrize("mean", [False, True])
def test_parity_one_step_planted_4000(mean):
    x, _ = planted_unit_rows(4000, 512, 0.01, 11, _dev())
    _parity_one_step(x * 3.0, mean, "planted 4000x512")


def stub_server(fcs, order=None, dev=None):
    from fedfr_amd.server import Server
    srv = object.__new__(Server)
    srv.clients = [types.SimpleNamespace(fc_module=types.SimpleNamespace(fc=torch.nn.Parameter(t.clone())), num_classes=t.shape[0]) for t in fcs]
    srv.current_client_list = list(range(len(fcs))) if order is None else list(order)
    srv.device = dev if dev is not None else _dev()
    srv.logger = logging.getLogger("FL_face.server")
    return srv


@pytest.mark.gpu
def test_server_spreadout_against_fixture(monkeypatch, caplog):
    from fedfr_amd.config import config as cfg
    from fedfr_amd.server import SpreadOut_Module
    z = fixture()
    dev = _dev()
    monkeypatch.setattr(cfg, "weight_decay", float(z["weight_decay"]))
    for name, nc, ids, D, mode, iters, lr in cases(z):
        N = nc * ids
        monkeypatch.setattr(cfg, "lr", lr)
        fc0 = closed_form_fc(N, D, **gen_params(z))
        srv = stub_server([fc0[k * ids:(k + 1) * ids].to(dev) for k in range(nc)])
        caplog.clear()
        with caplog.at_level(logging.INFO, logger="FL_face.server"):
            srv.SpreadOut(sp_iter=iters, mode=mode)
        lines = [r.getMessage() for r in caplog.records]
        sp = [l for l in lines if l.startswith("- SP iter")]
        losses = np.array([float(l.split("Loss :")[1].split(",")[0]) for l in sp])
        assert lines[0] == "=====Collect FC and cat to a big matrix=====" and lines[1] == "=====SpreadOut Module Create=====" \
            and lines[-1] == "=====Update FC in partial FC module=====", lines
        assert sp == ["- SP iter %d Loss :  %.5e , Start backward" % (i, v) for i, v in enumerate(losses)] and len(sp) == iters, sp
        out = [c.fc_module.fc.data for c in srv.clients]
        assert all(o.device == dev and o.dtype == torch.float32 and o.shape == (ids, D) for o in out)
        assert len({o.untyped_storage().data_ptr() for o in out}) == nc                    # independent tensors, not views of one buffer
        fin = torch.cat(out).cpu().to(f64)
        upd = fin - fc0.to(f64)
        rows = torch.from_numpy(z[name + "_rows"])
        ref_fin = torch.from_numpy(z[name + "_final"]).to(f64)
        # the logged losses carry 6 digits: half a unit of the last one is added to the bound
        e_loss = float(np.max(np.abs(losses - z[name + "_losses"]) / np.abs(z[name + "_losses"])))
        b_loss = min(4 * float(z[name + "_div_loss"]), FP32_BAR) + 0.5e-5
        print("%s losses: %.3e (reference fp32 vs fp64 %.3e, bound %.3e)" % (name, e_loss, float(z[name + "_div_loss"]), b_loss))
        assert e_loss <= b_loss, (name, e_loss, b_loss)
        if ref_fin.shape[0] == N:
            ref_upd = ref_fin - fc0.to(f64)
            for k in range(nc):
                sl = slice(k * ids, (k + 1) * ids)
                e, y = rel(upd[sl], ref_upd[sl]), float(z[name + "_div_update_slices"][k])
                print("%s client %d update: %.3e (reference fp32 vs fp64 %.3e)" % (name, k, e, y))
                assert e <= min(4 * y, FP32_BAR), (name, k, e, y)
        else:
            e, y = rel(upd[rows], ref_fin - fc0.to(f64)[rows]), float(z[name + "_div_update_rows"])
            print("%s update on %d stored rows: %.3e (reference fp32 vs fp64 %.3e)" % (name, len(rows), e, y))
            assert e <= min(4 * y, FP32_BAR), (name, e, y)
        e, y = rel(upd.norm(dim=1), z[name + "_update_rownorm"]), float(z[name + "_div_update"])
        print("%s update row norms: %.3e (reference fp32 vs fp64 %.3e)" % (name, e, y))
        assert e <= min(4 * y, FP32_BAR), (name, e, y)
        # the reference's own loop on the module: same final FC
        sp_mod = SpreadOut_Module(fc0.to(dev).clone(), margin=MARGIN, mode=mode)
        opt = torch.optim.SGD(sp_mod.parameters(), lr=lr * 10, momentum=0.9, weight_decay=float(z["weight_decay"]))
        for _ in range(iters):
            opt.zero_grad()
            loss = sp_mod()
            loss.backward()
            opt.step()
        e = rel(sp_mod.FC.data.cpu().to(f64) - fc0.to(f64), upd)
        print("%s module + torch.optim.SGD vs Server.SpreadOut, update: %.3e (bound %.3e)" % (name, e, min(4 * y, FP32_BAR)))
        assert e <= min(4 * y, FP32_BAR), (name, e, y)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["sum", "mean"])
def test_server_spreadout_order_and_unequal_counts(monkeypatch, mode):
    """A permuted client list with unequal class counts (running offsets, not idx * num_classes) against the fp64 restatement of the loop;
    the bound is four times the error of the reference's fp32 formulation driven through the same loop on the same input."""
    from fedfr_amd.config import config as cfg
    z = fixture()
    dev = _dev()
    lr, wd, iters = (0.1, 5e-4, 6) if mode == "mean" else (0.001, 5e-4, 4)
    monkeypatch.setattr(cfg, "lr", lr)
    monkeypatch.setattr(cfg, "weight_decay", wd)
    counts, order, D = [50, 120, 70, 100, 61], [3, 0, 4, 2, 1], 128
    fc0 = closed_form_fc(sum(counts), D, **gen_params(z))
    offs = np.concatenate([[0], np.cumsum([counts[i] for i in order])])
    parts = {i: fc0[offs[k]:offs[k + 1]] for k, i in enumerate(order)}          # stacked in `order`, the matrix is fc0
    srv = stub_server([parts[i].to(dev) for i in range(len(counts))], order)
    srv.SpreadOut(sp_iter=iters, mode=mode)
    _, want = restate_loop(fc0, mode == "mean", iters, lr * 10, wd)
    ref = torch.nn.Parameter(fc0.clone())
    opt = torch.optim.SGD([ref], lr=lr * 10, momentum=0.9, weight_decay=wd)
    for _ in range(iters):
        opt.zero_grad()
        fn = torch.nn.functional.normalize(ref)
        l = torch.relu((fn @ fn.t()).masked_select(~torch.eye(len(ref), dtype=torch.bool)) - MARGIN) ** 2
        (l.mean() if mode == "mean" else l.sum()).backward()
        opt.step()
    for k, i in enumerate(order):
        got = srv.clients[i].fc_module.fc.data
        assert got.shape == (counts[i], D)
        sl = slice(offs[k], offs[k + 1])
        e = rel(got.cpu().to(f64) - fc0[sl].to(f64), want[sl] - fc0[sl].to(f64))
        y = rel(ref.data[sl].to(f64) - fc0[sl].to(f64), want[sl] - fc0[sl].to(f64))
        print("%s client %d (position %d) update: %.3e, reference fp32 %.3e" % (mode, i, k, e, y))
        assert e <= min(4 * y, FP32_BAR), (mode, i, e, y)


@pytest.mark.gpu
@pytest.mark.parametrize("N,D", [(4000, 512), (1237, 132)])
def test_run_to_run_identical(N, D):
    from fedfr_amd import ops
    fn, _ = planted_unit_rows(N, D, 0.02, 5, _dev())
    a = ops.spreadout_loss_grad(fn, MARGIN, True)
    b = ops.spreadout_loss_grad(fn, MARGIN, True)
    assert int(a[2]) > 0
    for u, v in zip(a, b):
        assert torch.equal(u, v)


@pytest.mark.gpu
def test_scale_85000():
    """N = 85 000, D = 512: S would be 29 GB in fp32; the step may allocate four FC-sized buffers and 16 MiB, no N^2 term."""
    from fedfr_amd import ops
    from fedfr_amd.server import SpreadOut_Module
    N, D, dev = 85000, 512, _dev()
    fn, planted = planted_unit_rows(N, D, 0.001, 3, dev)
    mod = SpreadOut_Module(fn, margin=MARGIN, mode="sum")
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    loss_mod = mod()
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated(dev) - base
    print("extra device memory of one forward at N = %d: %.1f MiB (bound %.1f MiB)" % (N, extra / 2 ** 20, (4 * N * D * 4 + (16 << 20)) / 2 ** 20))
    assert extra <= 4 * N * D * 4 + (16 << 20), extra
    del loss_mod, mod
    fn1, _ = ops.normalize_rows(fn)
    loss, dfn, active = ops.spreadout_loss_grad(fn1, MARGIN, False)
    torch.cuda.synchronize()
    rows = torch.arange(64, device=dev) * (N // 64) + 7
    rows[:32] = planted[:32]                                                     # half of the sampled rows have an active pair
    l64, d64, act64 = restate_fn(fn1, MARGIN, False, rows=rows)
    # the reference's fp32 formulation cannot run at this size: its error is taken on the planted pairs plus the 4000 first rows
    sub = fn1[torch.unique(torch.cat([planted, torch.arange(4000, device=dev)]))]
    ls64, ds64, _ = restate_fn(sub, MARGIN, False)
    ls32, ds32 = reference_fp32(sub, MARGIN, False, True)
    y_d, y_l = rel(ds32, ds64), abs(float(ls32) - float(ls64)) / max(float(ls64), 1e-300)
    e_d, e_l = rel(dfn[rows], d64), abs(float(loss) - float(l64)) / float(l64)
    print("N = %d: loss %.3e (reference fp32 on a 4000-row subset %.3e), dFn on 64 rows %.3e (reference %.3e), active %d" %
          (N, e_l, y_l, e_d, y_d, int(active)))
    assert int(active) == act64 and act64 >= 2 * int(N * 0.001) * 0.9, (int(active), act64)
    assert float(d64[:32].norm()) > 0
    assert e_d <= min(4 * y_d, FP32_BAR), (e_d, y_d)
    assert e_l <= min(4 * y_l, FP32_BAR), (e_l, y_l)


@pytest.mark.gpu
def test_error_paths():
    from fedfr_amd import ops
    from fedfr_amd.server import SpreadOut_Module
    dev = _dev()
    x, _ = planted_unit_rows(64, 128, 0.1, 1, dev)
    with pytest.raises(RuntimeError, match="spreadout_loss_grad"):
        ops.spreadout_loss_grad(x.cpu(), MARGIN, False)
    with pytest.raises(RuntimeError, match="spreadout_loss_grad"):
        ops.spreadout_loss_grad(x.double(), MARGIN, False)
    with pytest.raises(RuntimeError, match="spreadout_loss_grad"):
        ops.spreadout_loss_grad(x[:, ::2], MARGIN, False)
    with pytest.raises(RuntimeError, match="fedfr_spreadout_grad"):
        ops.spreadout_loss_grad(x[:, :6].contiguous(), MARGIN, False)
    with pytest.raises(RuntimeError, match="SpreadOutFn"):
        SpreadOut_Module(x.cpu().clone())()
    with pytest.raises(ValueError, match="mode"):
        SpreadOut_Module(x.clone(), mode="max")
    srv = stub_server([x[:32], x[32:]])
    with pytest.raises(ValueError, match="mode"):
        srv.SpreadOut(mode="max")
    srv.current_client_list = None
    with pytest.raises(AssertionError):
        srv.SpreadOut()
