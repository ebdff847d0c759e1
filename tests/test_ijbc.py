"""IJB-C template evaluation, job 1:1 (fedfr_amd.eval_ijbc, kernels in fedfr_amd/csrc/ijbc.hip) against a numpy restatement of the
reference's ijbc_all.py (image2template_feature_11/_1n, verification, roc_curve + the nearest-FPR pick).

CPU: numpy's summation orders that the kernels reproduce are pinned; the host TPR@FPR read-out equals sklearn on adversarial score
sets; the CSR order, the meta readers and gen_mask; the new kernels do not spill; the C ABI rejects bad arguments.
GPU: pooling bit for bit (pre-normalisation sums) in each test mode on skewed templates; pair scores bit-identical to np.sum; exact
tables on integer-valued features with planted ties; the 1:1 job end to end; a full IJB-C-sized run; the error paths."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

from conftest import REPO, load_golden

X_LABELS = [1e-6, 1e-5, 1e-4, 1e-3, 1e-2, 1e-1]


# ---- numpy restatements of the reference ---------------------------------------------------------------------------------------
def pairwise(a):
    """numpy's pairwise summation of a contiguous row, restated (the order the kernels reproduce)."""
    n = len(a)
    if n < 8:
        r = a.dtype.type(0)
        for x in a:
            r = a.dtype.type(r + x)
        return r
    if n <= 128:
        r = list(a[:8])
        i = 8
        while i < n - n % 8:
            for j in range(8):
                r[j] = r[j] + a[i + j]
            i += 8
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
        for k in range(i, n):
            res = res + a[k]
        return res
    n2 = n // 2
    n2 -= n2 % 8
    return pairwise(a[:n2]) + pairwise(a[n2:])


def ref_prepare(img_feats, faceness, use_norm_score=True, use_detector_score=True, use_flip_test=False):
    """ijbc_all.py:515-533 (F1 / N1 / D1) on float32 features."""
    x = img_feats
    if use_flip_test:
        x = x[:, :x.shape[1] // 2] + x[:, x.shape[1] // 2:]
    if not use_norm_score:
        x = x / np.sqrt(np.sum(x ** 2, -1, keepdims=True))
    if use_detector_score:
        x = x * faceness[:, np.newaxis]
    return x


def ref_template_sums(x, templates, medias, choose=None):
    """The per-template float32 sums of image2template_feature_11/_1n before normalisation (medias: mean over frames)."""
    uniq = np.unique(templates if choose is None else choose)
    out = np.zeros((len(uniq), x.shape[1]))
    for t, u in enumerate(uniq):
        (ind,) = np.where(templates == u)
        f, m = x[ind], medias[ind]
        per_media = []
        for um, ct in zip(*np.unique(m, return_counts=True)):
            (im,) = np.where(m == um)
            per_media.append(f[im] if ct == 1 else np.mean(f[im], axis=0, keepdims=True))
        out[t] = np.sum(np.array(per_media), axis=0)
    return out, uniq


def skewed_meta(rng, n_templates, max_images=400, max_frames=100, first_id=1000):
    """Templates of 1 .. max_images images; medias are single images or videos of up to max_frames frames; rows shuffled."""
    templates, medias = [], []
    mid = 50000
    for t in range(n_templates):
        n = int(rng.integers(1, max_images + 1)) if t % 7 == 0 else int(rng.integers(1, 30))
        while n > 0:
            k = min(n, int(rng.integers(2, max_frames + 1)) if rng.random() < 0.4 else 1)
            templates += [first_id + 3 * t] * k
            medias += [mid] * k
            mid += int(rng.integers(1, 5))
            n -= k
    perm = rng.permutation(len(templates))
    return np.array(templates)[perm], np.array(medias)[perm]


def ref_table(label, score, x_labels=X_LABELS):
    from fedfr_amd import eval_ijbc
    return eval_ijbc.reference_table(label, score, x_labels)[0]


def exact_counts(label, score):
    gv = np.unique(score[label == 1])[::-1]
    G = len(gv)
    k = G - np.searchsorted(gv[::-1], score, side="right")            # number of genuine values > s
    eq = np.zeros(len(score), dtype=bool)
    inb = k < G
    eq[inb] = gv[k[inb]] == score[inb]
    c = np.zeros(3 * G + 1, np.int64)
    neg = label != 1
    np.add.at(c, k[neg & ~eq], 1)
    np.add.at(c, G + 1 + k[neg & eq], 1)
    np.add.at(c, 2 * G + 1 + k[~neg], 1)
    return gv, c


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------
def test_numpy_summation_orders_are_pinned():
    """The orders the kernels reproduce: np.sum over a contiguous row is pairwise; np.mean / np.sum over axis 0 add rows in order."""
    rng = np.random.default_rng(0)
    for dt in (np.float64, np.float32):
        for D in (5, 8, 100, 128, 256, 512, 1024):
            a = (rng.standard_normal((16, D)) * rng.standard_normal((16, D))).astype(dt)
            s = np.sum(a, -1)
            assert all(s[i] == pairwise(a[i]) for i in range(16)), (dt, D)
    x = rng.standard_normal((37, 1, 512)).astype(np.float32)
    seq = x[0, 0].copy()
    for i in range(1, 37):
        seq = seq + x[i, 0]
    assert np.array_equal(np.sum(x, axis=0)[0], seq)
    m = np.mean(x[:, 0], axis=0, keepdims=True)
    assert m.dtype == np.float32 and np.array_equal(m[0], seq / np.float32(37))


def test_template_csr_follows_reference_order():
    from fedfr_amd import eval_ijbc
    templates = np.array([7, 3, 7, 3, 7, 9, 3])
    medias = np.array([2, 5, 1, 4, 2, 8, 5])
    uniq, t_off, m_off, img = eval_ijbc.template_csr(templates, medias)
    assert list(uniq) == [3, 7, 9]
    # template 3: media 4 = [3], media 5 = [1, 6]; template 7: media 1 = [2], media 2 = [0, 4]; template 9: media 8 = [5]
    assert list(t_off) == [0, 2, 4, 5] and list(m_off) == [0, 1, 3, 4, 6, 7] and list(img) == [3, 1, 6, 2, 0, 4, 5]
    uniq, t_off, m_off, img = eval_ijbc.template_csr(templates, medias, choose_templates=[9, 9, 7, 11])
    assert list(uniq) == [7, 9, 11] and list(t_off) == [0, 2, 3, 3] and list(img) == [2, 0, 4, 5]


ADVERSARIAL = {
    "ties": (np.array([1, 0, 1, 0, 0, 1, 0, 0]), np.array([0.5, 0.5, 0.3, 0.3, 0.3, 0.9, 0.1, 0.5])),
    "duplicates": (np.array([1, 1, 1, 0, 0, 0, 0, 0, 0, 0]), np.array([0.8, 0.8, 0.2, 0.5, 0.5, 0.5, 0.4, 0.4, 0.1, 0.1])),
    "all_equal": (np.array([1, 0, 0, 1, 0]), np.full(5, 0.25)),
    "no_impostor_above_top_genuine": (np.array([1, 1, 0, 0, 0, 0]), np.array([0.9, 0.7, 0.6, 0.6, 0.2, -0.4])),
}


def test_table_from_counts_equals_sklearn_on_adversarial_sets():
    from fedfr_amd import eval_ijbc
    cases = dict(ADVERSARIAL)
    # x exactly halfway between two kept points: 4 impostors, FPR points 0, 0.25, 0.5, ...; x = 0.125 and 0.375
    cases["halfway"] = (np.array([0, 1, 0, 1, 0, 0]), np.array([0.9, 0.8, 0.7, 0.6, 0.5, 0.4]))
    rng = np.random.default_rng(5)
    for i in range(400):                                              # small random sets on a coarse grid: many ties
        P = int(rng.integers(2, 50))
        lv = int(rng.integers(1, 8))
        score = rng.integers(0, lv + 1, P) / lv if i % 2 else rng.standard_normal(P)
        label = (rng.random(P) < rng.random()).astype(np.int64)
        label[0], label[-1] = 1, 0
        cases["random%d" % i] = (label, score)
    for name, (label, score) in cases.items():
        score = score.astype(np.float64)
        nneg = int(np.sum(label != 1))
        xs = X_LABELS + [0.125, 0.375, 0.5 / nneg, 1.5 / nneg, 0.5, 1.0]
        gv, c = exact_counts(label, score)
        fetch = lambda lo, hi: score[(label != 1) & (score > lo) & (score < hi)]
        assert eval_ijbc.table_from_counts(gv, c, xs, fetch) == ref_table(label, score, xs), name


def test_meta_readers(tmp_path):
    from fedfr_amd import eval_ijbc
    (tmp_path / "tid_mid.txt").write_text("1/a.jpg 11 101\n1/b.jpg 11 102\n2/c.jpg 12 103\n")
    (tmp_path / "pairs.txt").write_text("11 12 0\n11 11 1\n")
    t, m = eval_ijbc.read_template_media_list(tmp_path / "tid_mid.txt")
    assert list(t) == [11, 11, 12] and list(m) == [101, 102, 103] and t.dtype == np.int64
    p1, p2, lab = eval_ijbc.read_template_pair_list(tmp_path / "pairs.txt")
    assert list(p1) == [11, 11] and list(p2) == [12, 11] and list(lab) == [0, 1]


def test_restatement_reproduces_fixture():
    """The numpy restatement of the reference (pooling, np.sum scores, roc_curve + pick) and the count read-out reproduce ijbc.npz,
    which tools/make_golden.py captured from the reference's own functions."""
    from fedfr_amd import eval_ijbc
    from sklearn.preprocessing import normalize
    z = fixture()
    assert z["min_margin"] > 1e-9
    x = ref_prepare(z["img_feats"].astype(np.float32), z["faceness"].astype(np.float32))
    sums, uniq = ref_template_sums(x, z["templates"].astype(np.int64), z["medias"].astype(np.int64))
    assert np.array_equal(uniq, z["unique_templates"])
    tf = normalize(sums)
    assert np.array_equal(tf, z["template_feats"])
    row = {t: i for i, t in enumerate(uniq)}
    i1, i2 = np.array([row[a] for a in z["p1"]]), np.array([row[b] for b in z["p2"]])
    score = np.sum(tf[i1] * tf[i2], -1)
    assert np.array_equal(score, z["score"])
    label = z["label"].astype(np.int64)
    assert ref_table(label, score) == list(z["tpr"])
    gv, c = exact_counts(label, score)
    tprs = eval_ijbc.table_from_counts(gv, c, X_LABELS, lambda lo, hi: score[(label != 1) & (score > lo) & (score < hi)])
    assert tprs == list(z["tpr"]) and eval_ijbc.format_table(tprs) == list(z["table"])


def fixture():
    z = load_golden("ijbc")
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__ as ge
    ge.build()
    from fedfr_amd import _C
    return _C


def test_ijbc_kernels_do_not_spill(built_lib):
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(REPO, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    libdir = os.path.dirname(built_lib.LIB_PATH)
    for name in ("libfedfr_hip.so", "libfedfr_hip_bf16.so"):
        ks = kr.kernels(os.path.join(libdir, name))
        for k in ("ijbc_image_norm_kernel", "ijbc_template_pool_kernel", "ijbc_pair_kernel", "ijbc_roc_count_kernel",
                  "ijbc_count_reduce_kernel"):
            found = [(n, r) for n, r in ks.items() if k in n]
            assert found, (name, k)
            assert all(r["scratch"] == 0 for _, r in found), (name, found)


def test_abi_rejects_bad_arguments(built_lib):
    """Argument checks run on the host before anything is enqueued (no GPU needed)."""
    lib = built_lib.lib()
    d = 1 << 20                                                     # never dereferenced: every call below fails its checks first

    def pool(N=10, D=512, T=2, M=3, NI=10, mode=0, norm=0, ws=0, out=d):
        rc = lib.fedfr_template_pool(d, N, D, 0, None, norm, d, T, d, M, d, NI, mode, None, out, d if ws else None, ws, d, None)
        return rc, lib.fedfr_last_error_string().decode()

    for kw, word in ((dict(D=300), "D = 300"), (dict(D=0), "D = 0"), (dict(T=0), "T = 0"), (dict(mode=2), "mode"),
                     (dict(norm=1), "workspace"), (dict(out=None), "null")):
        rc, msg = pool(**kw)
        assert rc != 0 and word in msg, (kw, rc, msg)

    def pairs(D=512, G=3, P=1000, ws=None, gv=d, score=d):
        ws = lib.fedfr_roc_counts_workspace_bytes(P, max(G, 1)) if ws is None else ws
        rc = lib.fedfr_pair_scores_roc(d, 4, D, d, 10, d, d, P, score, d, gv, G, d, d, ws, d, None)
        return rc, lib.fedfr_last_error_string().decode()

    assert lib.fedfr_roc_counts_workspace_bytes(1000, 3) > 0
    for kw, word in ((dict(D=200), "D = 200"), (dict(G=0), "G = 0"), (dict(G=40001), "G = 40001"), (dict(P=0), "P = 0"),
                     (dict(ws=4), "workspace"), (dict(gv=None, score=None), "neither")):
        rc, msg = pairs(**kw)
        assert rc != 0 and word in msg, (kw, rc, msg)
    rc = lib.fedfr_roc_counts(d, d, 100, d, 0, d, d, 1 << 20, d, None)
    assert rc != 0 and "G = 0" in lib.fedfr_last_error_string().decode()


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------
def _dev():
    return torch.device("cuda:0")


@pytest.mark.gpu
@pytest.mark.parametrize("mode,D", [("default", 128), ("default", 512), ("flip", 512), ("no_detector", 128), ("norm_images", 128),
                                    ("norm_images", 512)])
def test_template_pool_matches_reference_order(mode, D):
    from fedfr_amd import eval_ijbc
    rng = np.random.default_rng({"default": 1, "flip": 2, "no_detector": 3, "norm_images": 4}[mode] + D)
    templates, medias = skewed_meta(rng, 60 if D == 128 else 25)
    N = len(templates)
    feats = rng.standard_normal((N, 2 * D if mode == "flip" else D)).astype(np.float32)
    face = rng.uniform(0.3, 1.0, N).astype(np.float32)
    kw = dict(use_flip_test=mode == "flip", use_detector_score=mode != "no_detector", use_norm_score=mode != "norm_images")
    x = ref_prepare(feats, face, **kw)
    sums, uniq = ref_template_sums(x, templates, medias)
    out, u, raw = eval_ijbc.template_pool(feats, templates, medias, faceness=face if kw["use_detector_score"] else None,
                                          flip=kw["use_flip_test"], norm_images=not kw["use_norm_score"], mode=0, return_raw=True)
    assert np.array_equal(u, uniq)
    raw = raw.cpu().numpy().astype(np.float64)
    assert np.array_equal(raw, sums)                                # bit for bit, image norms (N1 off) included
    from sklearn.preprocessing import normalize
    assert np.abs(out.cpu().numpy() - normalize(sums)).max() <= 1e-15     # sklearn's einsum order vs numpy's pairwise one
    # 1:N flavour: the explicit divide, numpy's order: bit for bit
    if kw["use_norm_score"]:
        choose = np.concatenate([uniq[::3], uniq[::3]])
        o1, u1 = eval_ijbc.template_pool(feats, templates, medias, choose_templates=choose,
                                         faceness=face if kw["use_detector_score"] else None, flip=kw["use_flip_test"], mode=1)
        s1, _ = ref_template_sums(x, templates, medias, choose)
        assert np.array_equal(u1, np.unique(choose))
        assert np.array_equal(o1.cpu().numpy(), s1 / np.sqrt(np.sum(s1 ** 2, -1, keepdims=True)))


@pytest.mark.gpu
@pytest.mark.parametrize("D", [5, 100, 128, 256, 512, 1024])
def test_pair_scores_bit_identical_to_numpy(D):
    from fedfr_amd import eval_ijbc
    rng = np.random.default_rng(D)
    T = 300
    f = rng.standard_normal((T, D))
    f /= np.linalg.norm(f, axis=1, keepdims=True)
    uniq = np.sort(rng.choice(100000, T, replace=False))
    P = 20011
    r1, r2 = rng.integers(0, T, P), rng.integers(0, T, P)
    got = eval_ijbc.verification(f, uniq, uniq[r1], uniq[r2])
    assert np.array_equal(got, np.sum(f[r1] * f[r2], -1))


@pytest.mark.gpu
def test_integer_features_exact_table_with_ties():
    """Integer-valued features: every fp64 dot is exact, planted ties everywhere; counts and table equal numpy / sklearn."""
    from fedfr_amd import eval_ijbc
    rng = np.random.default_rng(11)
    T, D, P = 200, 128, 30000
    f = rng.integers(-1, 2, (T, D)).astype(np.float64)
    uniq = np.arange(T) * 2 + 1
    r1, r2 = rng.integers(0, T, P), rng.integers(0, T, P)
    label = (rng.random(P) < 0.05).astype(np.int64)
    score, gv, counts = eval_ijbc.pair_scores(f, uniq, uniq[r1], uniq[r2], label)
    score = score.cpu().numpy()
    ref = np.sum(f[r1] * f[r2], -1)
    assert np.array_equal(score, ref)
    egv, ec = exact_counts(label, ref)
    assert np.array_equal(gv, egv) and np.array_equal(counts, ec)
    xs = X_LABELS + [0.3, 0.5, 0.9]
    assert eval_ijbc.tpr_fpr_table(label, score, xs) == ref_table(label, ref, xs)
    g2, c2 = eval_ijbc.roc_counts(label, score)                         # the scores-only kernel: the same counts
    assert np.array_equal(g2, egv) and np.array_equal(c2, ec)


@pytest.mark.gpu
def test_ijbc_11_job_end_to_end():
    from fedfr_amd import eval_ijbc
    rng = np.random.default_rng(21)
    templates, medias = skewed_meta(rng, 150, max_images=60, max_frames=20)
    N, D = len(templates), 128
    subj = {t: t % 40 for t in np.unique(templates)}
    centers = rng.standard_normal((40, D))
    feats = (centers[[subj[t] for t in templates]] + 1.5 * rng.standard_normal((N, D))).astype(np.float32)
    face = rng.uniform(0.5, 1.0, N).astype(np.float32)
    uniq = np.unique(templates)
    P = 8000
    p1, p2 = rng.choice(uniq, P), rng.choice(uniq, P)
    label = np.array([int(subj[a] == subj[b]) for a, b in zip(p1, p2)])
    res = eval_ijbc.ijbc_11(feats, templates, medias, p1, p2, label, faceness=face)
    sums, u = ref_template_sums(ref_prepare(feats, face), templates, medias)
    from sklearn.preprocessing import normalize
    tf = normalize(sums)
    row = {t: i for i, t in enumerate(u)}
    i1, i2 = np.array([row[a] for a in p1]), np.array([row[b] for b in p2])
    ref_score = np.sum(tf[i1] * tf[i2], -1)
    score = res["score"].cpu().numpy()
    assert np.abs(score - ref_score).max() <= 1e-15
    assert res["tpr"] == ref_table(label, score)
    assert res["table"] == eval_ijbc.format_table(ref_table(label, score))
    feats11, u11 = eval_ijbc.image2template_feature_11(ref_prepare(feats, face), templates, medias)
    assert np.array_equal(u11, u) and np.abs(feats11 - tf).max() <= 1e-15
    assert np.array_equal(eval_ijbc.verification2(feats11, u11, p1, p2), np.sum(feats11[i1] * feats11[i2], -1))


@pytest.mark.gpu
def test_error_paths():
    from fedfr_amd import eval_ijbc
    f = np.eye(4, 128)
    with pytest.raises(ValueError, match="no template feature"):
        eval_ijbc.verification(f, np.array([2, 4, 6, 8]), np.array([2, 3]), np.array([4, 4]))
    with pytest.raises(ValueError, match="no template feature"):
        eval_ijbc.verification(f, np.array([2, 4, 6, 8]), np.array([2, 9]), np.array([4, 4]))
    with pytest.raises(ValueError, match="genuine"):
        eval_ijbc.tpr_fpr_table(np.zeros(5, np.int64), np.arange(5.0))
    with pytest.raises(ValueError, match="flip"):
        eval_ijbc.template_pool(np.ones((3, 5), np.float32), [1, 1, 2], [1, 1, 2], flip=True)
    with pytest.raises(ValueError, match="finite"):
        eval_ijbc.tpr_fpr_table(np.array([1, 0, 0, 1]), np.array([0.5, np.nan, 0.1, 0.2]))
    with pytest.raises(ValueError, match="faceness"):
        eval_ijbc.ijbc_11(np.ones((3, 8), np.float32), [1, 1, 2], [1, 1, 2], [1], [2], [0])


@pytest.mark.gpu
def test_drop_ins_reproduce_fixture():
    from fedfr_amd import eval_ijbc
    z = fixture()
    feats, face = z["img_feats"].astype(np.float32), z["faceness"].astype(np.float32)
    templates, medias = z["templates"].astype(np.int64), z["medias"].astype(np.int64)
    p1, p2, label = z["p1"].astype(np.int64), z["p2"].astype(np.int64), z["label"].astype(np.int64)
    tf, uniq = eval_ijbc.image2template_feature_11(ref_prepare(feats, face), templates, medias)
    assert np.array_equal(uniq, z["unique_templates"]) and np.abs(tf - z["template_feats"]).max() <= 1e-15
    assert np.array_equal(eval_ijbc.verification(z["template_feats"], uniq, p1, p2), z["score"])      # bit for bit
    res = eval_ijbc.ijbc_11(feats, templates, medias, p1, p2, label, faceness=face)
    assert np.abs(res["score"].cpu().numpy() - z["score"]).max() <= 1e-15
    assert res["tpr"] == list(z["tpr"]) and res["table"] == list(z["table"])
    assert eval_ijbc.tpr_fpr_table(label, z["score"]) == list(z["tpr"])


@pytest.mark.gpu
def test_full_ijbc_size():
    """The full-size run in a child process under its own 3-minute limit (a hang ends there)."""
    import subprocess
    import sys
    r = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_ijbc; "
                        "test_ijbc.full_size_run()" % (REPO, os.path.join(REPO, "tests"))], timeout=180, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]


def full_size_run():
    """469 375 x 512 images, 23 124 templates, 15 658 489 pairs (19 557 genuine): sampled fp64 oracle for pooling and scores, sklearn
    on the GPU's own scores for the table."""
    from fedfr_amd import eval_ijbc
    rng = np.random.default_rng(7)
    N, D, T, P, NG = 469375, 512, 23124, 15658489, 19557
    templates = np.sort(rng.integers(0, T, N))
    templates[:T] = np.arange(T)
    templates = rng.permutation(templates) + 1
    medias = templates * 10 + rng.integers(0, 3, N)
    g = torch.Generator(device=_dev()).manual_seed(3)
    feats = torch.randn(N, D, device=_dev(), generator=g)
    face = torch.rand(N, device=_dev(), generator=g) * 0.5 + 0.5
    uniq = np.arange(1, T + 1)
    p1 = torch.randint(1, T + 1, (P,), device=_dev(), generator=g)
    p2 = torch.randint(1, T + 1, (P,), device=_dev(), generator=g)
    label = torch.zeros(P, dtype=torch.int64, device=_dev())
    label[torch.randperm(P, device=_dev(), generator=g)[:NG]] = 1
    res = eval_ijbc.ijbc_11(feats, templates, medias, p1, p2, label, faceness=face)
    torch.cuda.synchronize()
    score = res["score"].cpu().numpy()
    # pooling + scores on a sample of pairs against the restatement in fp64 numpy
    fh, fc = feats.cpu().numpy(), face.cpu().numpy()
    idx = rng.choice(P, 200, replace=False)
    a, b = p1.cpu().numpy()[idx], p2.cpu().numpy()[idx]
    need = np.unique(np.concatenate([a, b]))
    sel = np.isin(templates, need)
    sums, u = ref_template_sums(ref_prepare(fh[sel], fc[sel]), templates[sel], medias[sel])
    tf = sums / np.sqrt(np.sum(sums ** 2, -1, keepdims=True))
    row = {t: i for i, t in enumerate(u)}
    ref = np.sum(tf[[row[x] for x in a]] * tf[[row[x] for x in b]], -1)
    assert np.abs(score[idx] - ref).max() <= 1e-14
    assert res["tpr"] == ref_table(label.cpu().numpy(), score)
