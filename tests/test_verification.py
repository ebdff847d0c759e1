"""k-fold 1:1 verification (fedfr_amd.eval_verification, fedfr_amd.callbacks, Server.test; kernel in fedfr_amd/csrc/verif.hip) against the
reference's eval/verification.py: goldens captured from the imported reference (calculate_roc outputs, per-threshold calculate_val_far
tables; tools/make_golden.py section 16) and a numpy restatement written from its semantics (verification.test cannot be captured:
its evaluate() raises in calculate_val's interp1d with current scipy).

CPU: the host read-out of numpy-built count tables reproduces every golden exactly; fold ranges equal KFold; the threshold values the
planted ties rely on; the kernel does not spill; the C ABI rejects bad arguments; load_bin rejects a wrong image size; pca > 0 raises.
GPU: counts equal the restatement's exactly on inputs whose distances keep clear of every threshold; planted exact ties; zero and NaN
rows; xnorm; test() end to end (tail batch, both data set forms); CallBackVerification and Server.test() with their checkpoints."""
import importlib.util
import io
import logging
import os
import pickle

import numpy as np
import pytest
import torch

from conftest import REPO, load_golden

THR_A, THR_B = np.arange(0, 4, 0.01), np.arange(0, 4, 0.001)
MIN_GAP = 1e-10


# ---- numpy restatement of the reference ---------------------------------------------------------------------------------------------
def ref_normalized(emb0, emb1=None):
    """verification.test :276-277: the two sets added (fp64) and row-normalised."""
    import sklearn.preprocessing
    s = emb0.astype(np.float64) if emb1 is None else emb0.astype(np.float64) + emb1.astype(np.float64)
    return sklearn.preprocessing.normalize(s)


def ref_dist(emb):
    return np.sum(np.square(np.subtract(emb[0::2], emb[1::2])), 1)


def ref_folds(P, nfolds):
    if nfolds == 1:
        return [(np.arange(P), np.arange(P))]
    from sklearn.model_selection import KFold
    return list(KFold(n_splits=nfolds, shuffle=False).split(np.arange(P)))


def ref_counts(dist, issame, nfolds, thr):
    """[nfolds, 2, T + 1]: pairs of every fold's test set by label and k0 = #{k : thr[k] <= dist} (a NaN sorts behind every threshold)."""
    k0 = np.searchsorted(thr, dist, side="right")
    c = np.zeros((nfolds, 2, len(thr) + 1), np.int64)
    for f, (_, test) in enumerate(ref_folds(len(dist), nfolds)):
        np.add.at(c[f], (issame[test].astype(int), k0[test]), 1)
    return c


def ref_accuracy_curves(thr, dist, issame):
    """calculate_accuracy at every threshold: tpr, fpr, acc arrays."""
    pred = np.less(dist[None, :], thr[:, None])
    tp, fp = (pred & issame).sum(1), (pred & ~issame).sum(1)
    tn, fn = (~pred & ~issame).sum(1), (~pred & issame).sum(1)
    tpr = np.array([0 if a + b == 0 else float(a) / float(a + b) for a, b in zip(tp, fn)])
    fpr = np.array([0 if a + b == 0 else float(a) / float(a + b) for a, b in zip(fp, tn)])
    acc = np.array([float(a + b) / dist.size for a, b in zip(tp, tn)])
    return tpr, fpr, acc


def ref_roc(thr, dist, issame, nfolds):
    """calculate_roc :75-106."""
    tprs, fprs, accuracy = np.zeros((nfolds, len(thr))), np.zeros((nfolds, len(thr))), np.zeros(nfolds)
    for f, (train, test) in enumerate(ref_folds(len(dist), nfolds)):
        best = np.argmax(ref_accuracy_curves(thr, dist[train], issame[train])[2])
        tprs[f], fprs[f], acc = ref_accuracy_curves(thr, dist[test], issame[test])
        accuracy[f] = acc[best]
    return np.mean(tprs, 0), np.mean(fprs, 0), accuracy


def min_gap(dist):
    d = dist[np.isfinite(dist)]
    return min(np.abs(d[:, None] - THR_A[None, :]).min(), np.abs(d[:, None] - THR_B[None, :]).min())


def golden_cases():
    g = load_golden("verification")
    for name in g["cases"]:
        P, D, nfolds, seed = (int(v) for v in g[name + "_shape"])
        yield str(name), P, D, nfolds, str(g[name + "_layout"]), seed, g


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REPO, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def kernel_resources():
    return _tool("kernel_resources")


synthetic_pairs = _tool("verification_pairs").synthetic_pairs          # the fixture's input generator (frozen with the fixture)


@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__ as ge
    ge.build()
    from fedfr_amd import _C
    return _C


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------
def test_thresholds_are_pinned():
    assert len(THR_A) == 400 and len(THR_B) == 4000
    assert THR_A[200] == 2.0 and THR_B[2000] == 2.0 and THR_A[0] == 0.0 and THR_B[0] == 0.0
    from fedfr_amd import eval_verification as V
    assert np.array_equal(V.roc_thresholds(), THR_A) and np.array_equal(V.val_thresholds(), THR_B)


@pytest.mark.parametrize("P", [10, 6000, 6003])
def test_fold_ranges_equal_kfold(P):
    from fedfr_amd import eval_verification as V
    for nfolds in (1, 3, 10):
        ranges = V.fold_ranges(P, nfolds)
        for (a, b), (_, test) in zip(ranges, ref_folds(P, nfolds)):
            assert np.array_equal(np.arange(a, b), test), (P, nfolds, a, b)
    with pytest.raises(ValueError):
        V.fold_ranges(5, 6)


def test_readout_reproduces_reference_goldens():
    from fedfr_amd import eval_verification as V
    n = 0
    for name, P, D, nfolds, layout, seed, g in golden_cases():
        emb0, emb1, issame = synthetic_pairs(P, D, seed, layout)
        dist = ref_dist(ref_normalized(emb0, emb1))
        assert min_gap(dist) > MIN_GAP and np.abs(dist - g[name + "_dist"]).max() < MIN_GAP     # the fixture's inputs, regenerated
        tpr, fpr, acc, best = V.roc_from_counts(ref_counts(dist, issame, nfolds, THR_A), return_best=True)
        assert np.array_equal(tpr, g[name + "_tpr"]) and np.array_equal(fpr, g[name + "_fpr"]), name
        assert np.array_equal(acc, g[name + "_accuracy"]), name
        _, far_train = V.val_far_from_counts(ref_counts(dist, issame, nfolds, THR_B))
        assert np.array_equal(far_train, g[name + "_far_train"]), name
        r = ref_roc(THR_A, dist, issame, nfolds)                      # the restatement the GPU tests lean on agrees with the reference too
        assert all(np.array_equal(a, b) for a, b in zip(r, (tpr, fpr, acc))), name
        n += 1
    assert n >= 4
    shapes = [(P, nf) for _, P, _, nf, _, _, _ in golden_cases()]
    assert any(P % nf for P, nf in shapes) and any(nf == 1 for _, nf in shapes)


def test_far_target_pick_rule():
    """The build-defined rule where interp1d rejects duplicate FAR values: smallest threshold of every distinct FAR, linear in between."""
    from fedfr_amd import eval_verification as V
    thr = np.arange(0, 1, 0.1)
    far = np.array([0, 0, 0, 0.002, 0.002, 0.004, 0.004, 0.004, 0.5, 0.5])
    assert V.pick_far_threshold(far, thr, 1e-3) == pytest.approx(0.5 * (thr[0] + thr[3]))      # between (0, thr[0]) and (0.002, thr[3])
    assert V.pick_far_threshold(far, thr, 0.004) == pytest.approx(thr[5])
    assert V.pick_far_threshold(far * 0, thr, 1e-3) == 0.0
    strict = np.linspace(0, 0.9, 10)                                                            # no duplicates: interp1d's own answer
    assert V.pick_far_threshold(strict, thr, 0.25) == pytest.approx(np.interp(0.25, strict, thr))


def test_host_calculate_accuracy_and_val_far():
    from fedfr_amd import eval_verification as V
    dist, same = np.array([0.1, 0.5, 0.9, np.nan]), np.array([True, False, True, True])
    assert V.calculate_accuracy(0.5, dist, same) == (1 / 3, 0.0, 0.5)
    assert V.calculate_val_far(0.6, dist, same) == (1 / 3, 1.0)


def test_verif_kernel_does_not_spill(built_lib):
    kr = kernel_resources()
    libdir = os.path.dirname(built_lib.LIB_PATH)
    for name in ("libfedfr_hip.so", "libfedfr_hip_bf16.so"):
        ks = kr.kernels(os.path.join(libdir, name))
        for k in ("verif_pair_kernel", "verif_norm_reduce_kernel"):
            found = [(n, r) for n, r in ks.items() if k in n]
            assert found, (name, k)
            assert all(r["scratch"] == 0 for _, r in found), (name, found)
        assert len([n for n in ks if "verif_pair_kernel" in n]) == 2          # fp32 and fp64 inputs


def test_abi_rejects_bad_arguments(built_lib):
    """Argument checks run on the host before anything is enqueued (no GPU needed)."""
    lib = built_lib.lib()
    d = 1 << 20                                                     # never dereferenced: every call below fails its checks first

    def call(P=100, D=512, nfolds=10, Ta=400, Tb=4000, ws=None, emb0=d, issame=d, thr_a=d, thr_b=d, counts_a=d, counts_b=d, norm=d,
             status=d, fp64=0):
        ws = lib.fedfr_verif_workspace_bytes(P, nfolds) if ws is None else ws
        rc = lib.fedfr_verif_fold_counts(emb0, None, fp64, 1, issame, P, D, nfolds, thr_a, Ta, thr_b, Tb, counts_a, counts_b, None, norm,
                                         status, d, ws, None)
        return rc, lib.fedfr_last_error_string().decode()

    assert lib.fedfr_verif_workspace_bytes(6000, 10) > 0
    assert lib.fedfr_verif_workspace_bytes(0, 1) == 0 and lib.fedfr_verif_workspace_bytes(5, 6) == 0
    for kw, word in ((dict(D=510), "D = 510"), (dict(D=1028), "D = 1028"), (dict(D=0), "D = 0"), (dict(P=0, ws=8), "P = 0"),
                     (dict(nfolds=0, ws=8), "nfolds = 0"), (dict(nfolds=101, ws=8), "nfolds = 101"), (dict(ws=4), "workspace"),
                     (dict(emb0=None), "null"), (dict(issame=None), "null"), (dict(thr_a=None), "null"), (dict(counts_a=None), "null"),
                     (dict(counts_b=None), "null"), (dict(norm=None), "null"), (dict(status=None), "null"), (dict(Ta=0), "Ta = 0"),
                     (dict(Ta=5000), "counters"), (dict(emb0=d + 4), "aligned"), (dict(fp64=2), "fp64_input")):
        rc, msg = call(**kw)
        assert rc != 0 and word in msg, (kw, rc, msg)
    rc = lib.fedfr_verif_fold_counts(d, None, 0, 1, d, 100, 512, 10, d, 400, d, 4000, d, d, None, d, d, None, 1 << 20, None)
    assert rc != 0 and "workspace" in lib.fedfr_last_error_string().decode()


def _png(arr):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, format="PNG")
    return buf.getvalue()


def write_bin(path, images, issame):
    """An insightface-style .bin: pickled (list of encoded images, issame list)."""
    with open(path, "wb") as f:
        pickle.dump(([_png(im) for im in images], [bool(v) for v in issame]), f, protocol=pickle.HIGHEST_PROTOCOL)


def test_error_paths_on_the_host(tmp_path):
    from fedfr_amd import eval_verification as V
    with pytest.raises(NotImplementedError):
        V.calculate_roc(THR_A, np.zeros((4, 8)), np.zeros((4, 8)), np.zeros(4, bool), nrof_folds=2, pca=3)
    with pytest.raises(NotImplementedError):
        V.evaluate(np.zeros((8, 8)), [True] * 4, nrof_folds=2, pca=1)
    rng = np.random.default_rng(0)
    write_bin(tmp_path / "small.bin", rng.integers(0, 256, (4, 64, 64, 3), dtype=np.uint8), [True, False])
    with pytest.raises(ValueError, match="64x64"):
        V.load_bin(str(tmp_path / "small.bin"), (112, 112))
    assert not os.path.exists(tmp_path / "small.pkl")


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------
def _dev():
    return torch.device("cuda:0")


def _gpu(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _run_counts(emb0, emb1, issame, nfolds, **kw):
    from fedfr_amd import eval_verification as V
    res = V.fold_counts(_gpu(emb0), _gpu(emb1), _gpu(issame), nfolds, **kw)
    torch.cuda.synchronize()
    return res


def _check_counts(emb0, emb1, issame, nfolds, what):
    """The condition on the inputs, then exact equality of both count tables; returns (kernel result, restatement's dist)."""
    D = emb0.shape[1]
    dist = ref_dist(ref_normalized(emb0, emb1))
    gap = min_gap(dist)
    print("%s: P %d D %d folds %d  min gap to a threshold %.3e" % (what, len(dist), D, nfolds, gap))
    assert gap > MIN_GAP, (what, gap)
    res = _run_counts(emb0, emb1, issame, nfolds)
    assert int(res.status.item()) == 0
    # Both sides form sum((a / |a| - b / |b|) ** 2) in fp64 from the same fp64 row sums, in different summation orders.  Every element of
    # a normalised row carries at most ~ (D / 2 + 3) ulp of relative error from its norm (a D-term sum and a square root, halved by the
    # root) plus one division, the squared differences (each <= 4 in total) one subtraction and one product rounding, and the D-term
    # sum of them at most D ulp in any order: about (D + 16) * 2^-52 relative to the largest possible dist, 4.
    bound = (D + 16) * 2.0 ** -52 * 4
    err = np.abs(res.dist.cpu().numpy() - dist).max()
    print("%s: max |dist - restatement| %.3e (bound %.3e)" % (what, err, bound))
    assert err <= bound, (what, err, bound)
    assert np.array_equal(res.counts_a.cpu().numpy(), ref_counts(dist, issame, nfolds, THR_A)), what
    assert np.array_equal(res.counts_b.cpu().numpy(), ref_counts(dist, issame, nfolds, THR_B)), what
    return res, dist


@pytest.mark.gpu
def test_counts_and_roc_equal_reference_on_golden_cases():
    from fedfr_amd import eval_verification as V
    for name, P, D, nfolds, layout, seed, g in golden_cases():
        emb0, emb1, issame = synthetic_pairs(P, D, seed, layout)
        res, dist = _check_counts(emb0, emb1, issame, nfolds, name)
        tpr, fpr, acc = V.roc_from_counts(res.counts_a)
        assert np.array_equal(tpr, g[name + "_tpr"]) and np.array_equal(fpr, g[name + "_fpr"]) and np.array_equal(acc, g[name + "_accuracy"])
        assert np.array_equal(V.val_far_from_counts(res.counts_b)[1], g[name + "_far_train"]), name
        # the drop-in signatures, on the reference's own inputs (normalised fp64 embeddings), numpy and torch
        emb = ref_normalized(emb0, emb1)
        for e1, e2, lab in ((emb[0::2], emb[1::2], issame), (torch.from_numpy(emb[0::2].copy()), _gpu(emb[1::2]), torch.from_numpy(issame))):
            tpr, fpr, acc = V.calculate_roc(THR_A, e1, e2, lab, nrof_folds=nfolds)
            assert np.array_equal(tpr, g[name + "_tpr"]) and np.array_equal(fpr, g[name + "_fpr"]), name
            assert np.array_equal(acc, g[name + "_accuracy"]), name
        out = V.evaluate(emb, list(issame), nrof_folds=nfolds)
        assert np.array_equal(out[0], g[name + "_tpr"]) and np.array_equal(out[2], g[name + "_accuracy"]), name
        val, val_std, far = out[3:]
        assert 0.0 <= val <= 1.0 and 0.0 <= far <= 1.0 and val_std >= 0.0
        assert out[3:] == V.calculate_val(THR_B, emb[0::2], emb[1::2], issame, 1e-3, nrof_folds=nfolds), name


@pytest.mark.gpu
@pytest.mark.parametrize("P,D,nfolds,flip,seed", [(6000, 512, 10, True, 0), (6003, 512, 10, True, 5), (6000, 512, 1, True, 6),
                                                  (6000, 512, 10, False, 7), (1500, 1024, 7, True, 8), (333, 4, 3, True, 9)])
def test_counts_equal_restatement(P, D, nfolds, flip, seed):
    from fedfr_amd import eval_verification as V
    emb0, emb1, issame = synthetic_pairs(P, D, seed, "blocks" if seed % 2 == 0 else "random", flip=flip)
    res, dist = _check_counts(emb0, emb1, issame, nfolds, "P%d_D%d_f%d_flip%d" % (P, D, nfolds, flip))
    assert all(np.array_equal(a, b) for a, b in zip(V.roc_from_counts(res.counts_a), ref_roc(THR_A, dist, issame, nfolds)))
    assert int(res.counts_a.sum()) == P and int(res.counts_b.sum()) == P


@pytest.mark.gpu
def test_planted_exact_ties():
    """Distances that are exact in any summation order: 0 (identical rows) is not below threshold 0; 2.0 (distinct one-hot rows, the
    flip copy equal) is not below thr[200] = thr[2000] = 2.0."""
    P, D, nfolds = 64, 128, 4
    emb0 = np.zeros((2 * P, D), np.float32)
    issame = np.arange(P) % 3 == 0
    for p in range(P):
        emb0[2 * p, p % D] = 3.0
        emb0[2 * p + 1, (p if p % 2 == 0 else p + 1) % D] = 3.0 if p % 4 < 2 else 0.5        # even p: same direction, any length
    dist = ref_dist(ref_normalized(emb0, emb0))
    assert set(np.unique(dist)) == {0.0, 2.0}
    res = _run_counts(emb0, emb0.copy(), issame, nfolds)
    assert np.array_equal(res.dist.cpu().numpy(), dist)
    ca, cb = res.counts_a.cpu().numpy(), res.counts_b.cpu().numpy()
    assert np.array_equal(ca, ref_counts(dist, issame, nfolds, THR_A)) and np.array_equal(cb, ref_counts(dist, issame, nfolds, THR_B))
    assert ca[:, :, 1].sum() == P // 2 and ca[:, :, 201].sum() == P // 2 and cb[:, :, 1].sum() == P // 2 and cb[:, :, 2001].sum() == P // 2
    assert ca[:, :, 0].sum() == 0 and ca[:, :, 200].sum() == 0                                   # k0 = 0 would mean "accepted at threshold 0"


@pytest.mark.gpu
def test_zero_and_nan_rows():
    from fedfr_amd import eval_verification as V
    emb0, _, issame = synthetic_pairs(40, 64, 11, "alternate", flip=False)
    emb0[4] = 0.0                                                    # pair 2: a zero row stays zero; its partner is one-hot, so
    emb0[5] = 0.0                                                    # dist = 1 exactly in any summation order
    emb0[5, 9] = 2.5
    emb0[10] = 0.0
    emb0[11] = 0.0                                                   # pair 5: both zero -> dist 0
    clean = ref_dist(ref_normalized(emb0))
    assert clean[2] == 1.0 and clean[5] == 0.0
    res = _run_counts(emb0, None, issame, 4)
    assert int(res.status.item()) == 0
    d = res.dist.cpu().numpy()
    assert d[2] == 1.0 and d[5] == 0.0
    emb0[14, 3] = np.nan                                             # pair 7
    res = _run_counts(emb0, None, issame, 4)
    assert int(res.status.item()) & 1
    d = res.dist.cpu().numpy()
    assert np.isnan(d[7]) and np.isfinite(np.delete(d, 7)).all()
    ca, cb = res.counts_a.cpu().numpy(), res.counts_b.cpu().numpy()
    ref = np.where(np.isnan(d), np.nan, clean)                       # np.less(nan, thr) is False at every threshold: bin T
    fold = [f for f, (a, b) in enumerate(V.fold_ranges(40, 4)) if a <= 7 < b][0]
    assert ca[fold, int(issame[7]), 400] >= 1 and cb[fold, int(issame[7]), 4000] >= 1
    assert min_gap(clean[~np.isin(np.arange(40), (2, 5, 7))]) > MIN_GAP      # pairs 2 and 5 are exact, pair 7 is NaN
    assert np.array_equal(ca, ref_counts(ref, issame, 4, THR_A)) and np.array_equal(cb, ref_counts(ref, issame, 4, THR_B))
    assert all(np.array_equal(a, b) for a, b in zip(V.roc_from_counts(ca), ref_roc(THR_A, ref, issame, 4)))
    with pytest.warns(UserWarning, match="NaN"):
        V.evaluate(np.where(np.isnan(emb0), np.nan, emb0).astype(np.float64), list(issame), nrof_folds=4)


@pytest.mark.gpu
def test_xnorm_is_accurate_and_reproducible():
    from fedfr_amd import eval_verification as V
    emb0, emb1, issame = synthetic_pairs(6000, 512, 0, "blocks")
    a = _run_counts(emb0, emb1, issame, 10)
    b = _run_counts(emb0, emb1, issame, 10)
    assert torch.equal(a.norm_sum, b.norm_sum) and torch.equal(a.counts_a, b.counts_a) and torch.equal(a.dist, b.dist)
    rows = np.concatenate([emb0, emb1]).astype(np.float64)
    want = np.mean([np.linalg.norm(r) for r in rows])
    got = float(a.norm_sum.item()) / len(rows)
    print("xnorm %.12f numpy %.12f rel %.3e" % (got, want, abs(got - want) / want))
    assert abs(got - want) <= len(rows) * 2.0 ** -52 * want            # sequential-sum bound over the rows
    c = _run_counts(emb0, None, issame, 10)
    want0 = np.mean([np.linalg.norm(r) for r in emb0.astype(np.float64)])
    assert abs(float(c.norm_sum.item()) / len(emb0) - want0) <= len(emb0) * 2.0 ** -52 * want0


def ref_test_flow(embeddings_list, issame, nfolds):
    """verification.test :262-281 on the embeddings it returns: xnorm, flip sum, normalise, accuracy of calculate_roc."""
    xnorm = np.mean([np.linalg.norm(r) for e in embeddings_list for r in e])
    emb = ref_normalized(embeddings_list[0], embeddings_list[1])
    dist = ref_dist(emb)
    acc = ref_roc(THR_A, dist, np.asarray(issame, bool), nfolds)[2]
    return np.mean(acc), np.std(acc), xnorm, dist


class PixelBackbone:
    """A stand-in backbone whose output row is a fixed function of its own input image only (some pixels of the transformed image):
    what every row of embeddings_list must be is then known exactly, whatever batch the image travelled in."""

    def __init__(self, D):
        self.D, self.batches = D, []

    def __call__(self, img):
        assert img.is_cuda and img.dtype == torch.float32
        self.batches.append(img.shape[0])
        return img.reshape(img.shape[0], -1)[:, ::97][:, :self.D].contiguous()


@pytest.mark.gpu
def test_test_flow_tail_batch_and_both_forms():
    from fedfr_amd import eval_verification as V
    rng = np.random.default_rng(3)
    P, H, W, D, bs = 37, 16, 16, 8, 16                               # 74 images: four full batches and a tail of 10
    u8 = rng.integers(0, 256, (2 * P, H, W, 3), dtype=np.uint8)
    issame = [bool(v) for v in rng.random(P) < 0.5]
    nchw = torch.from_numpy(u8).permute(0, 3, 1, 2).float().contiguous()
    ref_form = ([nchw, torch.flip(nchw, dims=[3])], issame)          # the reference's load_bin: fp32 NCHW 0 .. 255 and its mirror image
    bb1, bb2 = PixelBackbone(D), PixelBackbone(D)
    with torch.cuda.device(_dev()):
        r1 = V.test(ref_form, bb1, bs, nfolds=5)
        r2 = V.test((torch.from_numpy(u8).to(_dev()), issame), bb2, bs, nfolds=5)
    assert bb1.batches == [bs] * 10 and bb2.batches == [bs] * 10      # full batches only: one arena size
    for flip in (0, 1):
        img = ((ref_form[0][flip] / 255) - 0.5) / 0.5
        want = img.reshape(2 * P, -1)[:, ::97][:, :D].numpy().astype(np.float64)
        assert r1[5][flip].dtype == np.float64 and np.array_equal(r1[5][flip], want)          # every row once, the tail included
        assert np.array_equal(r2[5][flip], want)
    for r in (r1, r2):
        acc2, std2, xnorm, dist = ref_test_flow(r[5], issame, 5)
        assert min_gap(dist) > MIN_GAP
        assert r[0] == 0.0 and r[1] == 0.0 and r[2] == acc2 and r[3] == std2
        assert abs(r[4] - xnorm) <= 4 * P * 2.0 ** -52 * xnorm
    assert r1[2:5] == r2[2:5]


def _tiny_images(rng, n_ids, size=112):
    """Strongly different smooth images, one per identity."""
    yy, xx = np.mgrid[0:size, 0:size].astype(np.float64) / size
    out = []
    for i in range(n_ids):
        a, b, c = rng.uniform(-1, 1, 3)
        base = rng.uniform(40, 215, 3)
        img = base[None, None, :] + 60 * np.sin(6 * (a * xx + b * yy) + 3 * c)[:, :, None] * rng.uniform(0.3, 1, 3)[None, None, :]
        out.append(np.clip(img + rng.normal(0, 4, img.shape), 0, 255).astype(np.uint8))
    return out


@pytest.mark.gpu
def test_test_flow_on_iresnet_both_forms(tmp_path):
    from oracle import ref_cpu as R
    from fedfr_amd import backbones, eval_verification as V
    rng = np.random.default_rng(4)
    ids = _tiny_images(rng, 22)
    P = 11                                                            # 22 images, batch 8: two full batches and a tail of 6
    issame = [p % 2 == 0 for p in range(P)]
    images = []
    for p in range(P):                                                # a genuine pair: the image and a noisy copy (identical images would
        noisy = np.clip(ids[2 * p].astype(np.int16) + rng.integers(-12, 13, ids[2 * p].shape), 0, 255).astype(np.uint8)   # sit on threshold 0)
        images += [ids[2 * p], noisy if issame[p] else ids[2 * p + 1]]
    write_bin(tmp_path / "tiny.bin", images, issame)
    with torch.cuda.device(_dev()):
        data, lab = V.load_bin(str(tmp_path / "tiny.bin"), (112, 112))
        assert data.is_cuda and data.dtype == torch.uint8 and tuple(data.shape) == (2 * P, 112, 112, 3) and lab == issame
        assert np.array_equal(data.cpu().numpy(), np.stack(images))
        m = backbones.iresnet18().to(_dev())
        m.load_state_dict(R.closed_form_state_dict(R.IRESNET_LAYERS["iresnet18"], tag=2.0))
        m.eval()
        nchw = data.cpu().permute(0, 3, 1, 2).float().contiguous()
        r_ref = V.test(([nchw, torch.flip(nchw, dims=[3])], issame), m, 8, nfolds=5)
        r_cmp = V.test((data, issame), m, 8, nfolds=5)
    for a, b in zip(r_ref[5], r_cmp[5]):
        assert a.shape == (2 * P, 512) and np.isfinite(a).all() and np.array_equal(a, b)
    acc2, std2, xnorm, dist = ref_test_flow(r_cmp[5], issame, 5)
    print("iresnet18 tiny set: acc %.5f+-%.5f xnorm %.5f dist %s gap %.3e" % (acc2, std2, xnorm, np.round(dist, 4), min_gap(dist)))
    assert min_gap(dist) > MIN_GAP
    assert r_cmp[2] == acc2 and r_cmp[3] == std2 and r_ref[2:5] == r_cmp[2:5]
    assert abs(r_cmp[4] - xnorm) <= 4 * P * 2.0 ** -52 * xnorm
    assert not os.path.exists(tmp_path / "tiny.pkl")


def _server_fixture(tmp_path, targets, n_pairs=20):
    from fedfr_amd.config import config as cfg
    rng = np.random.default_rng(5)
    ids = _tiny_images(rng, 2 * n_pairs)
    issame = [p % 2 == 0 for p in range(n_pairs)]
    images = []
    for p in range(n_pairs):
        images += [ids[2 * p], ids[2 * p] if issame[p] else ids[2 * p + 1]]
    val = tmp_path / "val"
    val.mkdir()
    write_bin(val / "tiny.bin", images, issame)
    cfg.val_rec, cfg.val_targets = str(val), list(targets)
    return issame


@pytest.mark.gpu
def test_callback_verification_bookkeeping(tmp_path, caplog):
    from fedfr_amd import callbacks
    from fedfr_amd.config import config as cfg
    old = cfg.val_rec, cfg.val_targets
    try:
        _server_fixture(tmp_path, ["tiny", "absent"])                # a set without a file is passed over
        with torch.cuda.device(_dev()):
            cb = callbacks.CallBackVerification(2, 0, cfg.val_targets, cfg.val_rec, num_client=3)
            assert cb.ver_name_list == ["tiny"] and len(cb.ver_list) == 1 and cb.highest_acc_list == [[0, 0.0], [0, 0.0]]

            class Net(torch.nn.Module):
                """constant output (every distance 0: accuracy 0.5) or the image's own pixels (genuine pairs are identical images)."""
                def __init__(self, good):
                    super().__init__()
                    self.good, self.w = good, torch.nn.Parameter(torch.ones(1, device=_dev()))

                def forward(self, img):
                    f = img.reshape(img.shape[0], -1)[:, ::301][:, :64].contiguous()
                    return f if self.good else torch.ones_like(f)

            bad, good = Net(False), Net(True)
            with caplog.at_level(logging.INFO, logger="FL_face.callback"):
                cb(3, bad)                                            # 3 % frequent != 0: nothing runs
                assert not caplog.records
                cb(2, bad, None, th=3)                                # below the threshold
                assert not caplog.records
                cb(4, bad)
                assert bad.training                                   # eval() for the run, train() afterwards, as the reference
                msgs = [r.getMessage() for r in caplog.records]
                assert msgs[0].startswith("[tiny][4]XNorm: ") and msgs[1] == "[tiny][4]Accuracy-Flip: 0.50000+-0.00000"
                assert msgs[2] == "[tiny][4]Accuracy-Highest: 0.50000" and cb.highest_acc_list[0] == [4, 0.5]
                caplog.clear()
                cb(6, good)
                msgs = [r.getMessage() for r in caplog.records]
                assert msgs[1] == "[tiny][6]Accuracy-Flip: 1.00000+-0.00000" and msgs[2] == "[tiny][6]Accuracy-Highest: 1.00000"
                assert cb.highest_acc_list[0] == [6, 1.0]
                caplog.clear()
                cb(8, bad)                                            # worse: the best step stays
                assert [r.getMessage() for r in caplog.records][2] == "[tiny][6]Accuracy-Highest: 1.00000"
                caplog.clear()
                cb(8, good, client=1)
                msgs = [r.getMessage() for r in caplog.records]
                assert msgs[0].startswith("Client 1 :[tiny][8]XNorm: ") and msgs[1] == "Client 1 :[tiny][8]Accuracy-Flip: 1.00000+-0.00000"
                assert msgs[2] == "Client 1 :[tiny][8]Accuracy-Highest: 1.00000"
                assert cb.client_list[1][0] == [8, 1.0] and cb.client_list[0][0] == [0, 0.0] and cb.highest_acc_list[0] == [6, 1.0]
            not_epoch = callbacks.CallBackVerification(1, 0, cfg.val_targets, cfg.val_rec, epoch_based=False)
            with caplog.at_level(logging.INFO, logger="FL_face.callback"):
                caplog.clear()
                not_epoch(399, good, None, th=0)
                assert not caplog.records
            assert callbacks.CallBackVerification(1, 1, cfg.val_targets, cfg.val_rec).ver_list == []          # other ranks load nothing
    finally:
        cfg.val_rec, cfg.val_targets = old


@pytest.mark.gpu
def test_server_test_and_checkpoints(tmp_path):
    from oracle import ref_cpu as R
    from fedfr_amd import server
    from fedfr_amd.config import config as cfg
    old = cfg.val_rec, cfg.val_targets
    out_dir = tmp_path / "out"

    class Args:
        network, loss, local_epoch, BCE_local, aggr_alg = "iresnet18", "CosFace", 1, False, "FedAvg"
        output_dir = str(out_dir)

    class Data:
        pass

    try:
        _server_fixture(tmp_path, ["tiny"])
        with torch.cuda.device(_dev()):
            srv = server.Server([], Data, Args, device=_dev())
            assert not hasattr(srv, "callback_verification") and not out_dir.exists()       # created lazily, by the first test()
            good = R.closed_form_state_dict(R.IRESNET_LAYERS["iresnet18"], tag=2.0)
            blind = {k: (torch.zeros_like(v) if k == "fc.weight" else v.clone()) for k, v in good.items()}   # every image -> one embedding
            keys = list(srv.federated_model.state_dict().keys())

            srv.federated_model.load_state_dict(blind)
            srv.test()                                                # round 0
            cb = srv.callback_verification
            assert cb.ver_name_list == ["tiny"] and cb.highest_acc_list[-1] == [0, 0.5]
            assert not (out_dir / "backbone.pth").exists() and (out_dir / "backbone_0.pth").exists()
            assert not srv.federated_model.training

            srv.step_round()
            srv.federated_model.load_state_dict(good)
            srv.test()                                                # round 1: a model that tells the images apart
            print("round 1 highest", cb.highest_acc_list)
            assert cb.highest_acc_list[-1][0] == 1 and cb.highest_acc_list[-1][1] > 0.5
            assert (out_dir / "backbone.pth").exists() and (out_dir / "backbone_1.pth").exists()
            for name in ("backbone.pth", "backbone_1.pth"):
                sd = torch.load(out_dir / name)
                assert list(sd.keys()) == keys and "layer1.0.bn1.running_mean" in sd and "features.num_batches_tracked" in sd
                assert all(not v.is_cuda for v in sd.values())
                for k in ("conv1.weight", "fc.weight", "features.running_var"):
                    assert torch.equal(sd[k], good[k].to(sd[k].dtype)), (name, k)
            stamp = os.path.getmtime(out_dir / "backbone.pth")

            srv.step_round()
            srv.federated_model.load_state_dict(blind)
            srv.test()                                                # round 2: worse again, the best checkpoint stays
            assert cb.highest_acc_list[-1][0] == 1 and (out_dir / "backbone_2.pth").exists()
            assert os.path.getmtime(out_dir / "backbone.pth") == stamp
            assert torch.equal(torch.load(out_dir / "backbone.pth")["fc.weight"], good["fc.weight"])
            assert torch.equal(torch.load(out_dir / "backbone_2.pth")["fc.weight"], blind["fc.weight"])
    finally:
        cfg.val_rec, cfg.val_targets = old
