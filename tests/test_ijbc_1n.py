"""IJB-C job 1:N (fedfr_amd.eval_ijbc, kernels in fedfr_amd/csrc/ident64.hip) against the reference's ijbc_all.image2template_feature_1n /
gen_mask / evaluation, captured in tests/golden/ijbc_1n.npz by tools/make_golden.py.

CPU: a float64 numpy restatement of ``evaluation`` reproduces the fixture; the host helpers; the new kernels do not spill; the C ABI rejects
bad arguments.  GPU: exact known answers on integer-valued features (ties planted), bit-equality with fedfr_ident_topk, run-to-run
identity, the fixture end to end, the IJB-C shape against the restatement, the error paths.

Threshold tolerance (derived): reference (BLAS dgemm) and kernel sum the same D fp64 products in different orders, each within
D * 2^-53 * |q||g| of the exact dot, rows of unit norm up to rounding: two correct results differ by at most 2 * D * 2^-53; the tests use
atol = 4 * D * 2^-53.  Counts (rank, pr) equal the reference's exactly where no comparison is decided inside that band: the fixture stores
the smallest gap of all its comparisons (min_margin > 1e-9)."""
import ctypes as C
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

from conftest import REPO, load_golden

FARS = (0.01, 0.1)
MAX_K = 4096
MARGIN = 1e-9


def th_atol(D):
    return 4 * D * 2.0 ** -53


# ---- float64 restatement of ijbc_all.py:367-427 (rank by count(sim > pos) instead of argsort, thresholds by a sort) ----------------------
def restated_evaluation(query, gallery, mask, fars=FARS, K=None, partition=False):
    q, g, mask = np.asarray(query, np.float64), np.asarray(gallery, np.float64), np.asarray(mask, np.int64)
    Q = q.shape[0]
    sim = q @ g.T
    rows = np.nonzero(mask >= 0)[0]
    pos = np.full(Q, np.nan)
    pos[rows] = sim[rows, mask[rows]]
    sim[rows, mask[rows]] = -np.inf                             # out of every count below (finite scores only)
    with np.errstate(invalid="ignore"):
        gt = np.sum(sim > pos[:, None], axis=1).astype(np.int64)
        eq = np.sum(sim == pos[:, None], axis=1).astype(np.int64)
    gt[mask < 0] = eq[mask < 0] = -1
    need = [math.ceil(Q * f) for f in fars]
    K = max(need) if K is None else K
    neg_count = sim.size - len(rows)
    flat = sim.ravel()
    kk = min(K, flat.size)
    top = np.full(K, -np.inf)
    top[:kk] = -np.sort(np.partition(-flat, kk - 1)[:kk]) if partition else np.sort(flat)[::-1][:kk]
    out = {"pos": pos, "gt": gt, "eq": eq, "top": top, "neg_count": neg_count, "sim": sim}
    out["rank"] = {"top%d" % k: int(np.sum((gt >= 0) & (gt < k))) / Q for k in (1, 5, 10)}
    if neg_count >= max(need) <= K:
        out["th"] = {f: float(top[k - 1]) for f, k in zip(fars, need)}
        out["pr"] = {f: int(np.sum(pos > out["th"][f])) / Q for f in fars}
    return out


def fixture():
    z = load_golden("ijbc_1n")
    return {k: z[k] for k in z.files}


def log_lines(rank, pr):
    return ["%s : %.5f" % (r, rank[r]) for r in rank] + ["far = %.4f  pr = %.5f" % (f, pr[f]) for f in pr]


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------
def test_restatement_reproduces_reference():
    z = fixture()
    assert z["min_margin"] > MARGIN
    assert 0.0 < z["rank"][0] < 1.0
    D = z["probe_feats"].shape[1]
    r = restated_evaluation(z["probe_feats"], z["gallery_feats"], z["mask"])
    assert [r["rank"]["top1"], r["rank"]["top5"], r["rank"]["top10"]] == list(z["rank"])
    assert [r["pr"][f] for f in FARS] == list(z["pr"]) and list(z["fars"]) == list(FARS)
    assert np.abs(np.array([r["th"][f] for f in FARS]) - z["th"]).max() <= th_atol(D)
    assert np.all(r["eq"] == 0)


def test_host_helpers(tmp_path):
    from fedfr_amd import eval_ijbc
    z = fixture()
    gt = np.concatenate([z["gallery_s1_templates"], z["gallery_s2_templates"]])
    gi = np.concatenate([z["gallery_s1_ids"], z["gallery_s2_ids"]])
    uniq, ids = eval_ijbc.unique_template_ids(gt, gi)
    assert np.array_equal(uniq, z["gallery_unique_templates"]) and np.array_equal(ids, z["gallery_unique_ids"])
    uniq, ids = eval_ijbc.unique_template_ids(z["probe_templates"], z["probe_ids"])
    assert np.array_equal(uniq, z["probe_unique_templates"]) and np.array_equal(ids, z["probe_unique_ids"])
    mask = eval_ijbc.gen_mask(z["probe_unique_ids"], z["gallery_unique_ids"])
    assert mask.dtype == np.int64 and np.array_equal(mask, z["mask"])
    with pytest.raises(RuntimeError, match="RegIdsError with id = 7, duplicate = 0"):
        eval_ijbc.gen_mask([3, 7], [3, 5])
    with pytest.raises(RuntimeError, match="RegIdsError with id = 5, duplicate = 2"):
        eval_ijbc.gen_mask([3, 5], [5, 3, 5])
    assert np.array_equal(eval_ijbc.gen_mask([5, 3, 3], [3, 9, 5]), [2, 0, 0])
    path = tmp_path / "ijbc_1N_gallery_G1.csv"
    path.write_text("TEMPLATE_ID,SUBJECT_ID,FILENAME\n" + "".join("%d,%d,img/%d.jpg\n" % (t, s, t) for t, s in zip(gt, gi)))
    t, s = eval_ijbc.read_template_subject_id_list(str(path))
    assert t.dtype == np.int64 and s.dtype == np.int64 and np.array_equal(t, gt) and np.array_equal(s, gi)


@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__ as ge
    ge.build()
    from fedfr_amd import _C
    return _C


def test_ident64_kernels_do_not_spill(built_lib):
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(REPO, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    libdir = os.path.dirname(built_lib.LIB_PATH)
    for name in ("libfedfr_hip.so", "libfedfr_hip_bf16.so"):
        ks = kr.kernels(os.path.join(libdir, name))
        for k, n_inst in (("ident64_tile_kernel", 3), ("ident64_merge_kernel", 2), ("ident64_init_kernel", 1)):
            found = [(n, r) for n, r in ks.items() if k in n]
            assert len(found) == n_inst, (name, k, found)
            assert all(r["scratch"] == 0 for _, r in found), (name, found)


def test_abi_rejects_bad_arguments(built_lib):
    """Argument checks run on the host before anything is enqueued (no GPU needed)."""
    lib = built_lib.lib()
    dummy = 1 << 20                                             # never dereferenced: every call below fails its checks first

    def call(Q=100, G=5, D=8, K=4, ws_bytes=None, null=None):
        ws = lib.fedfr_ident_rank_workspace_bytes(Q, G, min(max(K, 1), MAX_K)) if ws_bytes is None else ws_bytes
        p = {n: (None if n == null else dummy) for n in ("query", "gallery", "mask", "pos", "top", "cnt", "gt", "eq", "ws", "status")}
        rc = lib.fedfr_ident_rank_topk(p["query"], Q, p["gallery"], G, D, p["mask"], K, p["pos"], p["top"], p["cnt"], p["gt"], p["eq"],
                                       p["ws"], ws, p["status"], None)
        return rc, lib.fedfr_last_error_string().decode()

    assert lib.fedfr_ident_rank_workspace_bytes(100, 5, 4) > 0
    assert lib.fedfr_ident_rank_workspace_bytes(19593, 3531, MAX_K) >= 256 * MAX_K * 8
    for kw, word in ((dict(K=0), "K"), (dict(K=MAX_K + 1), "K"), (dict(D=0), "D"), (dict(Q=0), "sizes"), (dict(G=0), "sizes"),
                     (dict(ws_bytes=8), "workspace"), (dict(null="ws"), "workspace"), (dict(null="query"), "null"),
                     (dict(null="mask"), "null"), (dict(null="eq"), "null"), (dict(null="status"), "null")):
        rc, msg = call(**kw)
        assert rc != 0 and word in msg, (kw, rc, msg)


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------
def _dev():
    return torch.device("cuda:0")


def _run(query, gallery, mask, K):
    from fedfr_amd import eval_ijbc
    d = _dev()
    return eval_ijbc.identification_rank_topk(torch.from_numpy(query).to(d), torch.from_numpy(gallery).to(d), torch.from_numpy(mask).to(d), K)


def int_case(Q, G, D, seed):
    """Integer-valued fp64 features (every dot exact, many equal scores); a fifth of the queries have no gallery row; every eighth
    gallery row repeats another one, so queries of either row tie their own score exactly."""
    rng = np.random.default_rng(seed)
    query = rng.integers(-2, 3, size=(Q, D)).astype(np.float64)
    gallery = rng.integers(-2, 3, size=(G, D)).astype(np.float64)
    if G > 1:
        dup = np.arange(0, G, 8)
        gallery[dup] = gallery[(dup + 1) % G]
    mask = np.where(rng.random(Q) < 0.8, rng.integers(0, G, Q), -1).astype(np.int64)
    return query, gallery, mask


INT_CASES = [  # (Q, G, D, K): Q and G off the 64 grid; 37 x 50 has fewer negatives than K (the -inf tail)
    (1, 1, 3, 1), (37, 50, 7, 1960), (37, 50, 7, MAX_K), (1000, 333, 40, 1), (1000, 333, 40, 1024), (1000, 333, 40, 1025),
    (1000, 333, 40, 1960), (4100, 1100, 24, MAX_K), (65, 700, 130, 1960), (63, 513, 16, 1025),
]


@pytest.mark.gpu
@pytest.mark.parametrize("Q,G,D,K", INT_CASES)
def test_exact_known_answers(Q, G, D, K):
    query, gallery, mask = int_case(Q, G, D, seed=Q * 7 + G * 3 + D + K)
    pos, top, cnt, gt, eq = _run(query, gallery, mask, K)
    r = restated_evaluation(query, gallery, mask, K=K)
    assert np.array_equal(pos.cpu().numpy(), r["pos"], equal_nan=True)
    assert int(cnt) == r["neg_count"] == Q * G - int(np.sum(mask >= 0))
    assert np.array_equal(top.cpu().numpy(), r["top"])
    assert gt.dtype == torch.int32 and np.array_equal(gt.cpu().numpy(), r["gt"])
    assert np.array_equal(eq.cpu().numpy(), r["eq"])
    if G > 8 and Q >= 37:
        assert np.any(r["eq"] > 0) and np.any(mask < 0)         # the case really has ties and rows without a positive
    if r["neg_count"] < K:
        assert np.all(np.isneginf(top.cpu().numpy()[r["neg_count"]:]))


@pytest.mark.gpu
def test_evaluation_on_ties_and_too_few_negatives():
    """evaluation on integer features: strict comparisons on exact ties (rank_gt < k, pos > th), ties reported, and a ValueError where the
    reference would index past its negatives."""
    from fedfr_amd import eval_ijbc
    query, gallery, mask = int_case(2000, 50, 4, seed=3)
    rank, pr, ties = eval_ijbc.evaluation(query, gallery, mask, return_ties=True)
    r = restated_evaluation(query, gallery, mask)
    assert rank == r["rank"] and pr == r["pr"] and list(pr) == list(FARS)
    assert ties == int(np.sum(r["eq"] > 0)) > 0
    assert any(np.any(r["pos"] == t) for t in r["th"].values())     # really tied at a threshold
    assert eval_ijbc.evaluation(query, gallery, mask) == (rank, pr)
    with pytest.raises(ValueError, match="negative"):               # one gallery row, every query's own: no negative at all
        eval_ijbc.evaluation(query[:10], gallery[:1], np.zeros(10, dtype=np.int64))
    with pytest.raises(ValueError, match="K limit"):
        eval_ijbc.evaluation(np.ones((MAX_K * 10 + 1, 2)), gallery[:, :2], np.zeros(MAX_K * 10 + 1, dtype=np.int64))


@pytest.mark.gpu
@pytest.mark.parametrize("D", [512, 100])
def test_bit_equal_to_ident_topk(D):
    """fp32-representable features, K = 1024, one segment: pos and neg_topk are the fp64 numbers fedfr_ident_topk computes."""
    from fedfr_amd import eval_1n, eval_ijbc
    g = torch.Generator().manual_seed(11)
    Q, G, K = 3000, 500, 1024
    query = torch.nn.functional.normalize(torch.randn(Q, D, generator=g))
    gallery = torch.nn.functional.normalize(torch.randn(G, D, generator=g))
    mask = torch.where(torch.rand(Q, generator=g) < 0.7, torch.randint(0, G, (Q,), generator=g), torch.full((Q,), -1))
    d = _dev()
    p32, t32, c32 = eval_1n.identification_topk(query.to(d), mask.to(d), gallery.to(d), torch.arange(G, device=d), [0, G], K)
    pos, top, cnt, gt, eq = eval_ijbc.identification_rank_topk(query.double().to(d), gallery.double().to(d), mask.to(d), K)
    assert np.array_equal(pos.cpu().numpy(), p32.cpu().numpy(), equal_nan=True)
    assert torch.equal(top, t32[0]) and int(cnt) == int(c32[0])
    r = restated_evaluation(query.double().numpy(), gallery.double().numpy(), mask.numpy(), K=K)
    assert np.nanmax(np.abs(pos.cpu().numpy() - r["pos"])) <= th_atol(D) and np.abs(top.cpu().numpy() - r["top"]).max() <= th_atol(D)


@pytest.mark.gpu
def test_run_to_run_identical():
    rng = np.random.default_rng(5)
    Q, G, D, K = 5000, 1300, 96, 1960
    query, gallery = rng.standard_normal((Q, D)), rng.standard_normal((G, D))
    mask = np.where(rng.random(Q) < 0.9, rng.integers(0, G, Q), -1).astype(np.int64)
    a = _run(query, gallery, mask, K)
    b = _run(query, gallery, mask, K)
    assert np.array_equal(a[0].cpu().numpy(), b[0].cpu().numpy(), equal_nan=True)
    for x, y in zip(a[1:], b[1:]):
        assert torch.equal(x, y)


@pytest.mark.gpu
def test_fixture_end_to_end():
    from fedfr_amd import eval_ijbc
    z = fixture()
    D = z["probe_feats"].shape[1]
    gt = np.concatenate([z["gallery_s1_templates"], z["gallery_s2_templates"]])      # ijbc_all.py:481-484
    gi = np.concatenate([z["gallery_s1_ids"], z["gallery_s2_ids"]])
    feats = z["img_feats"].astype(np.float32)
    res = eval_ijbc.ijbc_1n(feats, z["templates"], z["medias"], gt, gi, z["probe_templates"], z["probe_ids"], faceness=z["faceness"])
    want_rank = dict(zip(("top1", "top5", "top10"), z["rank"].tolist()))
    want_pr = dict(zip(FARS, z["pr"].tolist()))
    print("rank", res["rank"], "pr", res["pr"], "th", res["th"], "reference th", z["th"], "ties", res["ties"])
    assert res["rank"] == want_rank and res["pr"] == want_pr and res["ties"] == 0
    assert np.abs(np.array([res["th"][f] for f in FARS]) - z["th"]).max() <= th_atol(D)
    assert res["lines"] == log_lines(want_rank, want_pr)
    # the drop-ins one by one: template features bit for bit, then evaluation on the reference's own features
    x = feats * z["faceness"].astype(np.float32)[:, None]
    pf, pu, pids = eval_ijbc.image2template_feature_1n(x, z["templates"], z["medias"], z["probe_templates"], z["probe_ids"])
    assert isinstance(pf, np.ndarray) and np.array_equal(pf, z["probe_feats"])
    assert np.array_equal(pu, z["probe_unique_templates"]) and np.array_equal(pids, z["probe_unique_ids"])
    gf, gu, gids = eval_ijbc.image2template_feature_1n(x, z["templates"], z["medias"], gt, gi, on_gpu=True)
    assert gf.is_cuda and np.array_equal(gf.cpu().numpy(), z["gallery_feats"]) and np.array_equal(gids, z["gallery_unique_ids"])
    rank, pr = eval_ijbc.evaluation(pf, gf, eval_ijbc.gen_mask(pids, gids))
    assert rank == want_rank and pr == want_pr


IJBC_SEED = 0


def ijbc_size_inputs(seed=IJBC_SEED, Q=19593, G=3531, D=512):
    """Clustered unit features at the IJB-C 1:N shape: one centre per gallery subject, probes at a noise strength of 1 .. 8."""
    rng = np.random.default_rng(seed)
    centers = rng.standard_normal((G, D))
    centers /= np.linalg.norm(centers, axis=1, keepdims=True)
    mask = rng.integers(0, G, Q).astype(np.int64)
    gallery = centers + 0.5 * rng.standard_normal((G, D)) / D ** 0.5
    strength = rng.uniform(1.0, 8.0, (Q, 1))
    query = centers[mask] + strength * rng.standard_normal((Q, D)) / D ** 0.5
    gallery /= np.linalg.norm(gallery, axis=1, keepdims=True)
    query /= np.linalg.norm(query, axis=1, keepdims=True)
    return query, gallery, mask


def ijbc_size_margins(r, K):
    """The gaps that decide the results at the IJB-C shape.  Returns (deciding, nearest): per row the smallest of |pos - th| (both
    thresholds) and |pos - the 1st / 5th / 10th largest negative of the row|; per row the smallest |s(q, c) - pos(q)| over c != mask[q]."""
    sim, pos = r["sim"], r["pos"]
    G = sim.shape[1]
    part = np.partition(sim, [G - 10, G - 5, G - 1], axis=1)
    deciding = np.min(np.abs(part[:, [G - 10, G - 5, G - 1]] - pos[:, None]), axis=1)
    for t in r["th"].values():
        deciding = np.minimum(deciding, np.abs(pos - t))
    nearest = np.min(np.abs(sim - pos[:, None]), axis=1)
    return deciding, nearest


@pytest.mark.gpu
def test_ijbc_size():
    """Q = 19 593, G = 3 531, D = 512, K = 1 960 against the restatement on the host.  top-1 / 5 / 10 and pr must be equal: the seed is
    chosen (on the CPU, restatement alone) so that every comparison deciding them has a gap above 1e-9.  rank_gt is compared on the rows
    whose nearest other score is further than 1e-9 from the row's own; at most 0.1 % of the rows may be left out.
    Measured for seed 0 with the restatement alone: top-1 / 5 / 10 = 0.68841 / 0.79421 / 0.83515, pr = 0.51723 / 0.60634, smallest deciding
    gap 1.06e-6, smallest |s(q, c) - pos(q)| over all 69 M pairs 1.3e-8 (no row left out), gaps around the two thresholds > 4e-6."""
    query, gallery, mask = ijbc_size_inputs()
    Q, D = query.shape
    K = math.ceil(Q * max(FARS))
    assert K == 1960
    r = restated_evaluation(query, gallery, mask, partition=True)
    deciding, nearest = ijbc_size_margins(r, K)
    top = r["top"]
    k2 = math.ceil(Q * min(FARS))
    print("restatement: rank", r["rank"], "pr", r["pr"], "min deciding gap %.3e" % deciding.min(), "rows with nearest gap <= 1e-9:",
          int(np.sum(nearest <= MARGIN)), "of", Q)
    assert deciding.min() > MARGIN and 0.0 < r["rank"]["top1"] < 1.0
    assert min(top[k2 - 2] - top[k2 - 1], top[k2 - 1] - top[k2]) > MARGIN and top[K - 2] - top[K - 1] > MARGIN
    keep = nearest > MARGIN
    assert np.sum(~keep) <= Q / 1000
    from fedfr_amd import eval_ijbc
    d = _dev()
    qd, gd = torch.from_numpy(query).to(d), torch.from_numpy(gallery).to(d)
    pos, neg, cnt, gt, eq = eval_ijbc.identification_rank_topk(qd, gd, torch.from_numpy(mask).to(d), K)
    rank, pr, ties = eval_ijbc.evaluation(qd, gd, mask, return_ties=True)
    print("kernel: rank", rank, "pr", pr, "ties", ties, "max |pos - ref| %.3e" % np.abs(pos.cpu().numpy() - r["pos"]).max(),
          "max |neg_topk - ref| %.3e" % np.abs(neg.cpu().numpy() - top).max())
    assert rank == r["rank"] and pr == r["pr"]
    assert int(cnt) == r["neg_count"] == Q * (gallery.shape[0] - 1)
    assert np.abs(pos.cpu().numpy() - r["pos"]).max() <= th_atol(D)
    assert np.abs(neg.cpu().numpy() - top).max() <= th_atol(D)
    assert np.array_equal(gt.cpu().numpy()[keep], r["gt"][keep])
    assert np.array_equal(eq.cpu().numpy()[keep], r["eq"][keep])


@pytest.mark.gpu
def test_error_paths():
    from fedfr_amd import eval_ijbc
    d = _dev()
    q = torch.randn(10, 8, dtype=torch.float64, device=d)
    gal = torch.randn(4, 8, dtype=torch.float64, device=d)
    mask = torch.zeros(10, dtype=torch.int64, device=d)
    f = eval_ijbc.identification_rank_topk
    assert f(q, gal, mask, 3)[0].shape == (10,)
    for K in (0, MAX_K + 1):
        with pytest.raises(ValueError, match="K"):
            f(q, gal, mask, K)
    with pytest.raises(RuntimeError, match="MI355X"):
        f(q.cpu(), gal, mask, 3)
    with pytest.raises(RuntimeError, match="MI355X"):
        f(q, gal, mask.cpu(), 3)
    with pytest.raises(RuntimeError, match="float64"):
        f(q.float(), gal, mask, 3)
    with pytest.raises(ValueError, match="share D"):
        f(q, gal[:, :7], mask, 3)
    with pytest.raises(ValueError, match="mask"):
        f(q, gal, mask[:9], 3)
    with pytest.raises(ValueError, match="mask"):
        f(q, gal, torch.full_like(mask, 4), 3)
    qn = q.clone()
    qn[3, 2] = float("nan")
    with pytest.raises(ValueError, match="finite"):
        f(qn, gal, mask, 3)
    gi = gal.clone()
    gi[1, 0] = float("inf")
    with pytest.raises(ValueError, match="finite"):
        eval_ijbc.evaluation(q, gi, mask)
    with pytest.raises(ValueError, match="mask"):
        eval_ijbc.evaluation(q, gal, np.full(10, 4))
    with pytest.raises(ValueError, match="mask"):
        eval_ijbc.evaluation(q, gal, np.zeros(9, dtype=np.int64))
