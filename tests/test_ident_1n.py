"""1:N identification (fedfr_amd.eval_1n, kernels in fedfr_amd/csrc/ident.hip) against the reference's local_all.evaluation /
combine_features / --task 1:n client loop, captured in tests/golden/ident_1n.npz by tools/make_golden.py.

CPU: a float64 numpy restatement of the reference reproduces the fixture; the new kernels do not spill; the C ABI rejects bad arguments.
GPU: exact known answers on integer-valued features (every fp64 dot exact, ties included), random features against an fp64 oracle, the
drop-ins against the fixture, the full local setting (160 000 queries x 4 000 ids x 40 clients) and the error paths."""
import ctypes as C
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

from conftest import REPO, load_golden

FARS = (1e-6, 1e-5, 1e-4, 1e-3)


# ---- float64 restatement of local_all.py:142-176 (argsort dropped: its result is never used) ---------------------------------------
def restated_evaluation(query, gallery, mask, imgs_per_id=40, fars=FARS):
    q, g = np.asarray(query, np.float64), np.asarray(gallery, np.float64)
    sim = q @ g.T
    rows = np.where(mask != -1)[0]
    pos = sim[rows, mask[rows]]
    neg_mask = np.ones(sim.shape, dtype=bool)
    neg_mask[rows, mask[rows]] = False
    neg = np.sort(sim[neg_mask])[::-1]
    result, ths = [], []
    for far in fars:
        k = math.ceil(q.shape[0] * far)
        th = neg[k - 1]
        result.append(np.sum(pos > th) / (imgs_per_id * g.shape[0]))
        ths.append(th)
    return result, ths


def client_masks(labels, nid, num_client, ipi):
    """local_all.py:280-289: client c's gallery ids and positional query mask."""
    per = nid // num_client
    for c in range(num_client):
        m = labels.copy()
        idx = np.zeros(len(m), dtype=bool)
        idx[c * per * ipi:(c + 1) * per * ipi] = True
        m[idx] -= c * per
        m[~idx] = -1
        yield c * per, (c + 1) * per, m


def fixture():
    z = load_golden("ident_1n")
    return {k: z[k] for k in z.files}


def test_restatement_reproduces_reference():
    from fedfr_amd import eval_1n
    z = fixture()
    q, g = z["query"].astype(np.float32), z["gallery"].astype(np.float32)
    nid, ipi = int(z["num_ids"]), int(z["imgs_per_id"])
    assert z["min_margin"] > 1e-5
    for n in (3, 1):
        res, ths, gals = [], [], []
        for start, end, mask in client_masks(z["query_labels"], nid, n, ipi):
            gal, ids = eval_1n.combine_features(g, z["gallery_labels"], start, end)
            assert gal.dtype == np.float32 and np.array_equal(ids, np.arange(start, end))
            r, t = restated_evaluation(q, gal, mask, ipi)
            res.append(r)
            ths.append(t)
            gals.append(gal)
        assert np.array_equal(np.array(res), z["result_c%d" % n]), n
        assert np.array_equal(np.mean(np.array(res), axis=0), z["mean_c%d" % n]), n
        assert np.abs(np.array(ths) - z["th_c%d" % n]).max() < 1e-5, n
        if n == 3:
            assert np.array_equal(np.concatenate(gals), z["gallery_mean_c3"])       # the per-id float32 mean, bit for bit


@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__ as ge
    ge.build()
    from fedfr_amd import _C
    return _C


def test_ident_kernels_do_not_spill(built_lib):
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(REPO, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    libdir = os.path.dirname(built_lib.LIB_PATH)
    for name in ("libfedfr_hip.so", "libfedfr_hip_bf16.so"):
        ks = kr.kernels(os.path.join(libdir, name))
        for k in ("ident_tile_kernel", "ident_merge_kernel"):
            found = [(n, r) for n, r in ks.items() if k in n]
            assert found, (name, k)
            assert all(r["scratch"] == 0 for _, r in found), (name, found)


def test_abi_rejects_bad_arguments(built_lib):
    """Argument checks run on the host before anything is enqueued (no GPU needed)."""
    lib = built_lib.lib()
    dummy = 1 << 20                                             # never dereferenced: every call below fails its checks first

    def call(Q=100, G=5, D=8, seg=(0, 2, 5), K=4, ws_bytes=None):
        S = len(seg) - 1
        s = (C.c_longlong * len(seg))(*seg)
        ws = lib.fedfr_ident_workspace_bytes(Q, S, max(K, 1)) if ws_bytes is None else ws_bytes
        rc = lib.fedfr_ident_topk(dummy, dummy, Q, dummy, dummy, G, D, s, S, K, dummy, dummy, dummy, dummy, ws, None)
        return rc, lib.fedfr_last_error_string().decode()

    assert lib.fedfr_ident_workspace_bytes(100, 2, 4) > 0
    for kw, word in ((dict(K=0), "K"), (dict(K=1025), "K"), (dict(D=0), "D"), (dict(seg=(0, 2, 2, 5)), "empty"),
                     (dict(seg=(0, 2, 4)), "segments"), (dict(ws_bytes=8), "workspace")):
        rc, msg = call(**kw)
        assert rc != 0 and word in msg, (kw, rc, msg)


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------
def _dev():
    return torch.device("cuda:0")


def expected_topk(query, qid, gallery, gid, seg, K):
    """Exact answer for integer-valued features (numpy fp64: every dot is exact)."""
    sim = query.astype(np.float64) @ gallery.astype(np.float64).T
    pos_mask = (qid[:, None] >= 0) & (qid[:, None] == gid[None, :])
    pos = np.full(len(qid), np.nan)
    r, c = np.nonzero(pos_mask)
    pos[r] = sim[r, c]
    S = len(seg) - 1
    top = np.full((S, K), -np.inf)
    cnt = np.zeros(S, dtype=np.int64)
    for s in range(S):
        blk = sim[:, seg[s]:seg[s + 1]][~pos_mask[:, seg[s]:seg[s + 1]]]
        cnt[s] = blk.size
        v = np.sort(blk)[::-1][:K]
        top[s, :len(v)] = v
    return pos, top, cnt


def int_case(Q, G, D, S, seed):
    rng = np.random.default_rng(seed)
    query = (rng.integers(-2, 3, size=(Q, D)) * 0.125).astype(np.float32)
    gallery = (rng.integers(-2, 3, size=(G, D)) * 0.125).astype(np.float32)
    gid = rng.permutation(G).astype(np.int64) + 7
    gid[rng.random(G) < 0.1] = -1                               # gallery columns of no identity
    qid = np.where(rng.random(Q) < 0.6, rng.choice(gid, Q), rng.integers(-1, 3, Q) * (G + 50))   # with / without a positive
    cuts = np.sort(rng.choice(np.arange(1, G), S - 1, replace=False)) if S > 1 else np.array([], dtype=np.int64)
    seg = [0] + [int(c) for c in cuts] + [G]                  # unequal segment widths
    return query, qid.astype(np.int64), gallery, gid, seg


CASES = [  # (Q, G, D, S, K)
    (1, 1, 3, 1, 1), (63, 7, 64, 3, 7), (65, 64, 100, 3, 160), (1000, 100, 512, 40, 1024), (4100, 300, 64, 40, 160),
    (4100, 300, 512, 3, 1024), (1000, 7, 3, 1, 7), (65, 300, 100, 40, 1), (63, 100, 512, 1, 160), (1, 64, 64, 3, 1024),
    (4100, 64, 3, 1, 1024), (1000, 300, 100, 3, 7),
]


@pytest.mark.gpu
@pytest.mark.parametrize("Q,G,D,S,K", CASES)
def test_exact_known_answers(Q, G, D, S, K):
    from fedfr_amd import eval_1n
    query, qid, gallery, gid, seg = int_case(Q, G, D, S, seed=Q * 7 + G * 3 + D + S + K)
    d = _dev()
    args = (torch.from_numpy(query).to(d), torch.from_numpy(qid).to(d), torch.from_numpy(gallery).to(d), torch.from_numpy(gid).to(d), seg, K)
    pos, top, cnt = eval_1n.identification_topk(*args)
    ep, et, ec = expected_topk(query, qid, gallery, gid, seg, K)
    assert np.array_equal(pos.cpu().numpy(), ep, equal_nan=True)
    assert np.array_equal(cnt.cpu().numpy(), ec)
    assert np.array_equal(top.cpu().numpy(), et)
    pos2, top2, cnt2 = eval_1n.identification_topk(*args)   # run to run: the same bits
    assert torch.equal(top, top2) and torch.equal(cnt, cnt2) and np.array_equal(pos.cpu().numpy(), pos2.cpu().numpy(), equal_nan=True)


@pytest.mark.gpu
def test_strict_threshold_on_ties():
    """pos == th must not count (the reference's strict `>`): integer-valued features make such ties, and the rates equal a direct count."""
    from fedfr_amd import eval_1n
    rng = np.random.default_rng(3)
    Q, G, D = 2000, 50, 4
    query = rng.integers(-1, 2, size=(Q, D)).astype(np.float32)
    gallery = rng.integers(-1, 2, size=(G, D)).astype(np.float32)
    mask = np.where(rng.random(Q) < 0.8, rng.integers(0, G, Q), -1).astype(np.int64)
    rates, fars = eval_1n.evaluation(query, gallery, mask)
    want, ths = restated_evaluation(query, gallery, mask)
    assert rates == want and fars == list(FARS)
    sim = query.astype(np.float64) @ gallery.astype(np.float64).T
    pos = sim[mask >= 0, mask[mask >= 0]]
    assert any(np.any(pos == t) for t in ths)                   # the case is really tied at some threshold


@pytest.mark.gpu
def test_random_features_vs_fp64_oracle():
    from fedfr_amd import eval_1n
    g = torch.Generator().manual_seed(11)
    Q, G, D, K = 3000, 500, 512, 160
    query = torch.nn.functional.normalize(torch.randn(Q, D, generator=g))
    gallery = torch.nn.functional.normalize(torch.randn(G, D, generator=g))
    qid = torch.where(torch.rand(Q, generator=g) < 0.7, torch.randint(0, G, (Q,), generator=g), torch.full((Q,), -1))
    gid = torch.arange(G)
    seg = [0, 37, 200, 201, 500]
    d = _dev()
    pos, top, cnt = eval_1n.identification_topk(query.to(d), qid.to(d), gallery.to(d), gid.to(d), seg, K)
    ep, et, ec = expected_topk(query.numpy(), qid.numpy(), gallery.numpy(), gid.numpy(), seg, K)
    p = pos.cpu().numpy()
    assert np.array_equal(np.isnan(p), np.isnan(ep)) and np.nanmax(np.abs(p - ep)) < 1e-12
    assert np.array_equal(cnt.cpu().numpy(), ec)
    t = top.cpu().numpy()
    assert np.array_equal(np.isinf(t), np.isinf(et)) and np.abs(t[np.isfinite(et)] - et[np.isfinite(et)]).max() < 1e-12
    for s in range(len(seg) - 1):
        sel = (qid.numpy() >= seg[s]) & (qid.numpy() < seg[s + 1])
        r, _ = eval_1n.identification_rates(p[sel], t[s], Q, seg[s + 1] - seg[s])
        w, _ = eval_1n.identification_rates(ep[sel], et[s], Q, seg[s + 1] - seg[s])
        assert r == w, s


@pytest.mark.gpu
def test_dropins_vs_reference():
    from fedfr_amd import eval_1n
    z = fixture()
    q, g = z["query"].astype(np.float32), z["gallery"].astype(np.float32)
    ql, gl, nid, ipi = z["query_labels"], z["gallery_labels"], int(z["num_ids"]), int(z["imgs_per_id"])
    d = _dev()
    for n in (3, 1):
        per_client = []
        for c, (start, end, mask) in enumerate(client_masks(ql, nid, n, ipi)):
            gal, _ = eval_1n.combine_features(g, gl, start, end)
            rates, fars = eval_1n.evaluation(q, gal, mask)
            assert fars == list(FARS)
            assert np.array_equal(rates, z["result_c%d" % n][c]), (n, c)
            per_client.append(rates)
            pos, top, _ = eval_1n.identification_topk(torch.from_numpy(q).to(d), torch.from_numpy(mask).to(d), torch.from_numpy(gal).to(d),
                                                      torch.arange(end - start, device=d), [0, end - start], 3)
            _, ths = eval_1n.identification_rates(pos.cpu(), top[0].cpu(), len(q), end - start)
            assert np.abs(np.array(ths) - z["th_c%d" % n][c]).max() < 1e-5
        mean, res, fars = eval_1n.local_1n(q, ql, g, gl, n, num_ids=nid, imgs_per_id=ipi)
        assert np.array_equal(res, z["result_c%d" % n]) and np.array_equal(mean, z["mean_c%d" % n]), n
        assert np.array_equal(res, np.array(per_client))


@pytest.mark.gpu
def test_single_launch_equals_separate_client_calls():
    """local_1n's one launch over all client segments gives the same bits as one launch per client gallery."""
    from fedfr_amd import eval_1n
    z = fixture()
    q, g = z["query"].astype(np.float32), z["gallery"].astype(np.float32)
    ql, gl, nid, ipi = z["query_labels"], z["gallery_labels"], int(z["num_ids"]), int(z["imgs_per_id"])
    d = _dev()
    gal = z["gallery_mean_c3"]
    qid = np.where(np.arange(len(ql)) < nid * ipi, ql, -1)
    qt = torch.from_numpy(q).to(d)
    pos, top, cnt = eval_1n.identification_topk(qt, torch.from_numpy(qid).to(d), torch.from_numpy(gal).to(d), torch.arange(nid, device=d),
                                                [0, 20, 40, 60], 3)
    for c, (start, end, mask) in enumerate(client_masks(ql, nid, 3, ipi)):
        p1, t1, c1 = eval_1n.identification_topk(qt, torch.from_numpy(mask).to(d), torch.from_numpy(gal[start:end]).to(d),
                                                 torch.arange(end - start, device=d), [0, end - start], 3)
        rows = slice(start * ipi, end * ipi)
        assert torch.equal(p1[rows], pos[rows]) and torch.equal(t1[0], top[c]) and int(c1[0]) == int(cnt[c])


@pytest.mark.gpu
def test_full_local_setting():
    """160 000 queries x 4 000 ids x D 512, 40 clients in one call: against a chunked torch fp64 oracle, and the call's memory growth is
    a small fraction of what the Q x G fp64 similarity matrix would take."""
    from fedfr_amd import eval_1n
    d = _dev()
    Q, G, D, S, K = 160000, 4000, 512, 40, 160
    g = torch.Generator(device=d).manual_seed(5)
    centers = torch.nn.functional.normalize(torch.randn(G, D, device=d, generator=g))
    qid = torch.arange(Q, device=d) // 40
    query = torch.nn.functional.normalize(centers[qid] + 1.5 * torch.randn(Q, D, device=d, generator=g) / D ** 0.5)
    gallery = torch.nn.functional.normalize(centers + 0.5 * torch.randn(G, D, device=d, generator=g) / D ** 0.5)
    gid = torch.arange(G, device=d)
    per = G // S
    seg = [s * per for s in range(S + 1)]
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated(d)
    torch.cuda.reset_peak_memory_stats(d)
    pos, top, cnt = eval_1n.identification_topk(query, qid, gallery, gid, seg, K)
    torch.cuda.synchronize()
    growth = torch.cuda.max_memory_allocated(d) - base
    assert growth < Q * G * 8 / 100, growth
    q64 = query.double()
    ref_pos = (q64 * gallery.double()[qid]).sum(1)
    assert (pos - ref_pos).abs().max().item() < 1e-12
    for s in range(S):
        sim = q64 @ gallery[seg[s]:seg[s + 1]].double().T
        rows = torch.arange(s * per * 40, (s + 1) * per * 40, device=d)
        sim[rows, qid[rows] - seg[s]] = -float("inf")
        ref = torch.topk(sim.flatten(), K).values
        assert (top[s] - ref).abs().max().item() < 1e-12, s
        assert int(cnt[s]) == Q * per - per * 40


@pytest.mark.gpu
def test_error_paths():
    from fedfr_amd import eval_1n
    d = _dev()
    q = torch.randn(10, 8, device=d)
    gal = torch.randn(4, 8, device=d)
    qid = torch.zeros(10, dtype=torch.int64, device=d)
    gid = torch.arange(4, device=d)
    with pytest.raises(ValueError, match="K"):
        eval_1n.identification_topk(q, qid, gal, gid, [0, 4], 1025)
    with pytest.raises(ValueError, match="distinct"):
        eval_1n.identification_topk(q, qid, gal, torch.tensor([0, 1, 1, 2], device=d), [0, 4], 3)
    with pytest.raises(RuntimeError, match="MI355X"):
        eval_1n.identification_topk(q.cpu(), qid, gal, gid, [0, 4], 3)
    with pytest.raises(RuntimeError, match="MI355X"):
        eval_1n.identification_topk(q, qid.cpu(), gal, gid, [0, 4], 3)
    with pytest.raises(RuntimeError, match="empty"):                     # the library's own check, through the ctypes layer
        eval_1n.identification_topk(q, qid, gal, gid, [0, 2, 2, 4], 3)
    with pytest.raises(ValueError, match="mask"):
        eval_1n.evaluation(q, gal, np.full(10, 4))
    with pytest.raises(ValueError, match="mask"):
        eval_1n.evaluation(q, gal, np.full(10, -2))
    with pytest.raises(ValueError, match="negative"):                    # 1 query, 1 gallery row, its own positive: no negative at all
        eval_1n.evaluation(q[:1], gal[:1], np.zeros(1, dtype=np.int64))
    with pytest.raises(ValueError, match="positional"):
        eval_1n.local_1n(q.cpu().numpy(), np.arange(10), gal.cpu().numpy(), np.arange(4), 2, num_ids=4, imgs_per_id=2)
