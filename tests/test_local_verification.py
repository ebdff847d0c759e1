"""Local 1:1 verification (fedfr_amd.eval_local, eval_roc.roc_histogram_groups, kernel in fedfr_amd/csrc/roc_groups.hip; the
callback_verification hooks of Client.train* and Server.enable_local_verification) against the reference's eval_local.py, roc_cuda.py
and the 1:1 branch of local_all.py.

CPU: the new ABI symbol in header and ctypes table, its argument checks, no scratch in the kernel, local_11's log text and mean order on
hand-made histograms against a restatement of local_all.py:316-335, the ValueError for a group without genuine pairs, the callback's gate.
GPU: every histogram equals oracle.ref_cpu.roc_histogram per group on the target-first ordering EXACTLY (integer counts), every TPR row
equals oracle.ref_cpu.roc_tpr_at_fpr exactly; inputs are seeded and each test first asserts in numpy fp64 that no (dot + 1) * 1000
comes within 1e-9 of an integer, so the summation order cannot move a bin."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO

HEADER = os.path.join(REPO, "include", "fedfr_hip.h")
SYMBOL = "fedfr_roc_histogram_groups"
MIN_GAP = 1e-9


@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__ as ge
    ge.build()
    from fedfr_amd import _C
    return _C


# ---- inputs and the reference side --------------------------------------------------------------------------------------------------
def clustered(rng, labels, D, noise=0.3):
    """fp32 unit rows: one random centre per label plus noise."""
    cen = rng.standard_normal((int(labels.max()) + 1, D))
    cen /= np.linalg.norm(cen, axis=1, keepdims=True)
    f = cen[labels] + noise * rng.standard_normal((len(labels), D))
    return (f / np.linalg.norm(f, axis=1, keepdims=True)).astype(np.float32)


def bin_gap(f):
    """smallest distance of any pair's (dot + 1) * 1000 to an integer, in fp64 (the diagonal is no pair)."""
    x = (f.astype(np.float64) @ f.astype(np.float64).T + 1.0) * 1000.0
    g = np.abs(x - np.round(x))
    np.fill_diagonal(g, 1.0)
    return g.min()


def oracle_groups(f, lab, group, G):
    """[G, 2001, 2]: the oracle's single-range histogram with group c's rows first (roc_cuda.py:129-134), per group."""
    from oracle import ref_cpu as R
    out = np.zeros((G, 2001, 2), np.int64)
    for c in range(G):
        t = group == c
        if t.any():
            out[c] = R.roc_histogram(np.concatenate([f[t], f[~t]]), np.concatenate([lab[t], lab[~t]]), int(t.sum()))
    return out


def case_mixed(seed=1):
    """N = 331, D = 48, G = 5: groups of 70, 1, 64, 130 and 0 rows + 66 ungrouped, shuffled; 9 labels drawn independently of the groups, so
    labels span groups and ungrouped rows."""
    rng = np.random.default_rng(seed)
    group = np.concatenate([np.full(70, 0), np.full(1, 1), np.full(64, 2), np.full(130, 3), np.full(66, -1)]).astype(np.int64)
    lab = rng.integers(0, 9, len(group)).astype(np.int64)
    f = clustered(rng, lab, 48)
    p = rng.permutation(len(group))
    return f[p], lab[p], group[p], 5


def case_single(seed=2):
    rng = np.random.default_rng(seed)
    N, T = 200, 131
    lab = rng.integers(0, 11, N).astype(np.int64)
    group = np.full(N, -1, np.int64)
    group[rng.permutation(N)[:T]] = 0
    return clustered(rng, lab, 512), lab, group, 1


def case_aligned(seed=3):
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, 7, 192).astype(np.int64)
    group = rng.permutation(np.repeat(np.arange(3), 64)).astype(np.int64)
    return clustered(rng, lab, 64), lab, group, 3


def case_local11(seed=4):
    """6 identities x 40 images in identity order, as the local test set is laid out."""
    rng = np.random.default_rng(seed)
    lab = np.repeat(np.arange(6), 40).astype(np.int64)
    return clustered(rng, lab, 32, noise=0.25), lab


def ref_local_11_text(rows, num_client, num_ids, epoch):
    """local_all.py:305-335 on the rows roc_cuda.py would have logged: the text of local_log.txt, the mean parsed back from it."""
    per = num_ids // num_client
    text = '1:1 at Epoch : %d\n' % epoch
    for c, row in enumerate(rows):
        target_label = list(range(c * per, (c + 1) * per))
        text += 'Target label from %d to %d\n' % (target_label[0], target_label[-1])
        text += 'Epoch %d, TPR (-1 to -6) = %r\n' % (epoch, row)
    scores = []
    for line in text.splitlines():
        if 'Epoch %d, TPR' % epoch in line:
            s, end = line.find('['), line.find(']')
            scores.append([float(i) for i in line[s + 1:end].split(',')])
    mean = np.mean(np.array(scores), axis=0)
    text += 'Mean (-6 to -1):\n' + '['
    for i in range(len(mean)):
        text += '%.2f ' % (mean[len(mean) - 1 - i])
    text += ']\n'
    return text, mean


def handmade_hists(G, seed=0):
    rng = np.random.default_rng(seed)
    h = np.zeros((G, 2001, 2), np.int64)
    for c in range(G):
        h[c, 1200 + 40 * c:1950, 0] = rng.integers(0, 30, 750 - 40 * c)          # genuine pairs: high similarity, overlapping the
        h[c, 700:1400 + 30 * c, 1] = rng.integers(0, 5000, 700 + 30 * c)         # impostor tail
    return h


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------
def test_header_and_ctypes_table_have_the_new_symbol(built_lib):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % SYMBOL, src)
    assert m, "header does not declare " + SYMBOL
    res, args = built_lib.SIGNATURES[SYMBOL]
    assert res is ctypes.c_int and len(args) == len(m.group(1).split(","))
    assert hasattr(built_lib.lib(), SYMBOL)
    for name in ("libfedfr_hip.so", "libfedfr_hip_bf16.so"):                    # both storage builds export it
        assert hasattr(ctypes.CDLL(os.path.join(os.path.dirname(built_lib.LIB_PATH), name)), SYMBOL), name


def test_abi_rejects_bad_arguments(built_lib):
    """Argument checks run on the host before anything is enqueued (no GPU needed)."""
    lib = built_lib.lib()
    d = 1 << 20                                                      # never dereferenced: every call below ends before a launch
    tiles = np.array([0, 1, -1], np.int32)

    def call(feats=d, label=d, N=130, D=48, row_index=d, tile_group=tiles, G=2, tile_dev=d, hist=d):
        tg = None if tile_group is None else tile_group.ctypes.data
        rc = getattr(lib, SYMBOL)(feats, label, N, D, row_index, tg, 0 if tile_group is None else len(tile_group), G, tile_dev, hist, None)
        return rc, lib.fedfr_last_error_string().decode()

    for kw, word in ((dict(feats=None), "null"), (dict(label=None), "null"), (dict(row_index=None), "null"), (dict(tile_group=None), "null"),
                     (dict(tile_dev=None), "null"), (dict(hist=None), "null"), (dict(G=0), "G = 0"), (dict(G=-3), "G = -3"),
                     (dict(D=0), "D = 0"), (dict(N=0), "N = 0"), (dict(tile_group=np.zeros(0, np.int32)), "n_tiles = 0"),
                     (dict(tile_group=np.array([0, 2, -1], np.int32)), "group id 2"), (dict(G=1), "group id 1"),
                     (dict(tile_group=np.array([0, -2], np.int32)), "group id -2")):
        rc, msg = call(**kw)
        assert rc != 0 and word in msg, (kw, rc, msg)
    rc, msg = call(tile_group=np.array([-1, -1], np.int32))           # nobody has a target: nothing to launch, the histograms stay as they are
    assert rc == 0, msg


def test_grouped_kernel_does_not_spill(built_lib):
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(REPO, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    libdir = os.path.dirname(built_lib.LIB_PATH)
    for name in ("libfedfr_hip.so", "libfedfr_hip_bf16.so"):
        found = [(n, r) for n, r in kr.kernels(os.path.join(libdir, name)).items() if "roc_hist_groups_kernel" in n]
        assert len(found) == 1, (name, found)
        r = found[0][1]
        assert r["scratch"] == 0 and r["lds"] <= 64 * 1024 and r["vgpr"] <= 128, (name, r)     # 128 VGPRs: two workgroups per SIMD


def test_local_11_log_text_and_mean_order(tmp_path, capsys):
    from oracle import ref_cpu as R
    from fedfr_amd import eval_local
    G, num_ids, epoch = 3, 10, 7                                       # 10 // 3 = 3 identities per client, identity 9 is nobody's
    h = handmade_hists(G)
    want_rows = [R.roc_tpr_at_fpr(h[c]) for c in range(G)]
    assert len({tuple(r) for r in want_rows}) == G and all(r[0] > r[-1] for r in want_rows)      # distinct, non-flat rows: order matters
    want_text, want_mean = ref_local_11_text(want_rows, G, num_ids, epoch)
    (tmp_path / "local_log.txt").write_text("earlier line\n")          # the log is appended to
    rows, mean = eval_local.local_11_from_histograms(h, G, num_ids, epoch, str(tmp_path))
    assert rows == want_rows and np.array_equal(mean, want_mean)
    assert (tmp_path / "local_log.txt").read_text() == "earlier line\n" + want_text
    assert "Target label from 3 to 5\n" in want_text and "Mean (-6 to -1):\n[" in want_text
    out = capsys.readouterr().out
    assert "1:1 average results (-6 to -1):" in out and repr(['%.2f' % m for m in want_mean[::-1]]) in out
    rows2, _ = eval_local.local_11_from_histograms(torch.from_numpy(h), G, num_ids, epoch, None)      # tensors too; no directory, no file
    assert rows2 == want_rows


def test_local_11_raises_for_a_group_without_genuine_pairs(tmp_path):
    from fedfr_amd import eval_local
    h = handmade_hists(3)
    h[1, :, 0] = 0
    with pytest.raises(ValueError, match="group 1 .*same-label"):
        eval_local.local_11_from_histograms(h, 3, 9, 0, str(tmp_path))
    assert not (tmp_path / "local_log.txt").exists()                   # nothing is logged for a run that cannot finish
    h = handmade_hists(3)
    h[2, :, 1] = 0
    with pytest.raises(ValueError, match="group 2 .*different-label"):
        eval_local.local_11_from_histograms(h, 3, 9, 0, None)


def test_callback_gate_and_constructor(tmp_path):
    from fedfr_amd import eval_local

    class Ran(Exception):
        pass

    class Stub:                                                        # a backbone nobody may call on a closed gate
        def __call__(self, x):
            raise AssertionError("backbone called")

    def gated(cb, step):
        def features(backbone):
            raise Ran()
        cb.generate_features = features
        try:
            cb.veri_test(Stub(), step, [0, 1], 0)
        except Ran:
            return True
        return False

    mk = lambda **kw: eval_local.CallBack_LocalVerifi(kw.pop("frequent", 1), kw.pop("rank", 0), None, loader=[], **kw)
    assert gated(mk(), -1) and gated(mk(), 0) and gated(mk(), 5)       # the reference's defaults: th = -1, every step
    assert not gated(mk(th=0), -1) and gated(mk(th=0), 0)
    assert not gated(mk(th=3), 2) and gated(mk(th=3), 3)
    assert gated(mk(frequent=2), 4) and not gated(mk(frequent=2), 5) and not gated(mk(frequent=2), -1)
    assert not gated(mk(rank=1), 4)
    cb = mk()
    assert cb.client_record[3] == [] and cb.flip_test is False and cb.batch_size == 800 and cb.workers == 2
    with pytest.raises(NotImplementedError, match="RecordIO"):
        eval_local.CallBack_LocalVerifi(1, 0, str(tmp_path))
    (tmp_path / "idx_id_pair.txt").write_text("1 0\n2 0\n3 0\n4 1\n5 2\n")          # pandas.read_csv takes the first line as the header
    cb = eval_local.CallBack_LocalVerifi(1, 0, str(tmp_path), loader=[], verbose=False)
    assert cb.labels.tolist() == [0, 0, 1, 2]
    cb = eval_local.CallBack_LocalVerifi(1, 0, str(tmp_path), loader=[], labels=[5, 6], verbose=False)
    assert cb.labels.tolist() == [5, 6]


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------
def _dev():
    return torch.device("cuda:0")


def _gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _grouped(f, lab, group, G):
    from fedfr_amd import eval_roc
    with torch.cuda.device(_dev()):
        out = eval_roc.roc_histogram_groups(_gpu(f), _gpu(lab), _gpu(group), G)
        torch.cuda.synchronize()
    assert out.dtype == torch.int64 and tuple(out.shape) == (G, 2001, 2)
    return out.cpu().numpy()


def _pairs_with(T, N):
    return T * (T - 1) // 2 + T * (N - T)


@pytest.fixture(scope="module")
def mixed():
    f, lab, group, G = case_mixed()
    return f, lab, group, G, oracle_groups(f, lab, group, G)


@pytest.mark.gpu
def test_groups_of_every_shape_equal_oracle(mixed):
    f, lab, group, G, ref = mixed
    gap = bin_gap(f)
    print("mixed: N %d D %d G %d  min gap to a bin edge %.3e" % (f.shape[0], f.shape[1], G, gap))
    assert gap > MIN_GAP
    sizes = [int((group == c).sum()) for c in range(G)]
    assert sizes == [70, 1, 64, 130, 0] and int((group < 0).sum()) == 66
    assert any(len(set(group[lab == l])) > 2 and -1 in group[lab == l] for l in range(9))      # labels span groups and ungrouped rows
    got = _grouped(f, lab, group, G)
    for c in range(G):
        assert int(got[c].sum()) == _pairs_with(sizes[c], len(group)), c
        assert np.array_equal(got[c], ref[c]), c
    assert np.array_equal(got, _grouped(f, lab, group, G))             # integer atomics: run-to-run identical


@pytest.mark.gpu
def test_single_group_equals_oracle_and_single_range_kernel():
    from fedfr_amd import eval_roc
    f, lab, group, G = case_single()
    gap = bin_gap(f)
    print("single: min gap %.3e" % gap)
    assert gap > MIN_GAP and int((group == 0).sum()) == 131
    got = _grouped(f, lab, group, G)
    assert np.array_equal(got, oracle_groups(f, lab, group, G))
    t = group == 0
    with torch.cuda.device(_dev()):
        old = eval_roc.roc_histogram(_gpu(np.concatenate([f[t], f[~t]])), _gpu(np.concatenate([lab[t], lab[~t]])), 131).cpu().numpy()
    assert np.array_equal(got[0], old)


@pytest.mark.gpu
def test_aligned_partition_equals_oracle():
    f, lab, group, G = case_aligned()
    gap = bin_gap(f)
    print("aligned: min gap %.3e" % gap)
    assert gap > MIN_GAP and [int((group == c).sum()) for c in range(G)] == [64, 64, 64]
    got = _grouped(f, lab, group, G)
    assert np.array_equal(got, oracle_groups(f, lab, group, G))
    N = len(group)
    assert int(got.sum()) == 2 * (N * (N - 1) // 2) - 3 * (64 * 63 // 2)          # every pair twice, but once inside its own group


@pytest.mark.gpu
def test_ungrouped_rows_and_rejected_arguments():
    rng = np.random.default_rng(5)
    lab = rng.integers(0, 4, 65).astype(np.int64)
    f = clustered(rng, lab, 40)
    got = _grouped(f, lab, np.full(65, -1, np.int64), 2)
    assert not got.any()
    group = np.full(65, -1, np.int64)
    group[7] = 2
    with pytest.raises(RuntimeError, match="fedfr_amd: roc_histogram_groups"):
        _grouped(f, lab, group, 2)                                     # a group id >= G
    with pytest.raises(RuntimeError, match="fedfr_amd: roc_histogram_groups"):
        _grouped(f, lab, np.full(65, -1, np.int64), 0)                 # G = 0
    group[7] = -2
    with pytest.raises(RuntimeError, match="fedfr_amd: roc_histogram_groups"):
        _grouped(f, lab, group, 2)
    with pytest.raises(RuntimeError, match="must live on an MI355X"):
        from fedfr_amd import eval_roc
        eval_roc.roc_histogram_groups(torch.from_numpy(f), torch.from_numpy(lab), torch.from_numpy(group), 2)
    torch.cuda.synchronize()                                           # rejected, not a fault: the device is still usable
    assert not _grouped(f, lab, np.full(65, -1, np.int64), 1).any()


@pytest.mark.gpu
def test_local_11_equals_per_client_oracle(tmp_path):
    from oracle import ref_cpu as R
    from fedfr_amd import eval_local
    f, lab = case_local11()
    gap = bin_gap(f)
    print("local_11: min gap %.3e" % gap)
    assert gap > MIN_GAP
    group = lab // 2
    ref = oracle_groups(f, lab, group, 3)
    want_rows = [R.roc_tpr_at_fpr(ref[c]) for c in range(3)]
    want_text, want_mean = ref_local_11_text(want_rows, 3, 6, 12)
    with torch.cuda.device(_dev()):
        rows, mean = eval_local.local_11(_gpu(f), _gpu(lab), 3, num_ids=6, epoch=12, output_dir=str(tmp_path))
        rows_np, _ = eval_local.local_11(f, lab, 3, num_ids=6, epoch=12)           # numpy inputs, as the reference's .npy files
    print("local_11 rows", rows, "mean", mean)
    assert rows == want_rows and rows_np == want_rows and np.array_equal(mean, want_mean)
    assert (tmp_path / "local_log.txt").read_text() == want_text
    with torch.cuda.device(_dev()), pytest.raises(ValueError, match="group 2 .*same-label"):
        eval_local.local_11(f[:161], lab[:161], 3, num_ids=6)         # identities 0 - 3 and one image of 4: client 2 has no genuine pair


def _tiny_backbone():
    from oracle import ref_cpu as R
    from fedfr_amd import backbones
    m = backbones.iresnet18().to(_dev())
    m.load_state_dict(R.closed_form_state_dict(R.IRESNET_LAYERS["iresnet18"], tag=2.0))
    return m


@pytest.mark.gpu
def test_generate_features_flip_and_tail_batch():
    from oracle import ref_cpu as R
    from fedfr_amd import eval_local, ops
    imgs = torch.cat([R.closed_form_images(4, tag=1.0), R.closed_form_images(2, tag=2.0)])        # 6 images, batches of 4: a tail of 2
    labs = torch.tensor([3, 3, 4, 4, 5, 5])
    loader = [(imgs[:4], labs[:4]), (imgs[4:], labs[4:])]
    with torch.cuda.device(_dev()):
        m = _tiny_backbone()
        m.train()
        feats, got_lab = eval_local.generate_features(m, loader, flip_test=True)
        assert m.training and all(mod.training for mod in m.modules())                            # the mode is put back
        plain, none_lab = eval_local.generate_features(m.eval(), [imgs[:4], imgs[4:]], flip_test=False)
        assert not m.training and none_lab is None
        want, want_plain = [], []
        with torch.no_grad():
            for x in (imgs[:4].to(_dev()), imgs[4:].to(_dev())):                                  # the existing eval forward, same batches
                a, b = m(x), m(torch.flip(x, dims=[3]).contiguous())
                want.append(ops.normalize_rows(a + b)[0])
                want_plain.append(ops.normalize_rows(a)[0])
        torch.cuda.synchronize()
    assert feats.is_cuda and feats.dtype == torch.float32 and tuple(feats.shape) == (6, 512) and got_lab.tolist() == labs.tolist()
    assert np.array_equal(feats.cpu().numpy(), torch.cat(want).cpu().numpy())
    assert np.array_equal(plain.cpu().numpy(), torch.cat(want_plain).cpu().numpy())
    assert not np.array_equal(feats.cpu().numpy(), plain.cpu().numpy())                           # the mirrored pass was added
    assert np.abs(np.linalg.norm(feats.cpu().numpy().astype(np.float64), axis=1) - 1).max() < 1e-6


@pytest.mark.gpu
def test_callback_client_and_server_wiring(tmp_path):
    from oracle import ref_cpu as R
    from fedfr_amd import client, eval_local, server
    from fedfr_amd.config import config as cfg

    class DS:
        ID_base = 0

    class Loader(list):
        dataset = DS()

    def args(out):
        class Args:
            network, loss, local_epoch, BCE_local, aggr_alg = "iresnet18", "CosFace", 1, False, "FedAvg"
            output_dir = str(out)
        return Args

    class Data:
        train_class_sizes, train_dataset_sizes = [2, 2], [4, 4]
        train_loaders = [Loader([(R.closed_form_images(4, tag=float(c)), R.closed_form_labels(4, 2, tag=c))]) for c in range(2)]

    # the local test set: identities 0 and 1 (the clients' targets) with 4 images each, identities 2 and 3 with 2 each
    veri = [(R.closed_form_images(4, tag=10.0 + i), torch.tensor(l)) for i, l in enumerate(([0, 0, 1, 1], [0, 0, 1, 1], [2, 2, 3, 3]))]
    sd = R.closed_form_state_dict(R.IRESNET_LAYERS["iresnet18"], tag=2.0)
    old_lr = cfg.lr
    cfg.lr = 0.01
    try:
        with torch.cuda.device(_dev()):
            out = tmp_path / "with"
            cb = eval_local.CallBack_LocalVerifi(1, 0, None, output_dir=str(out), loader=veri, verbose=False)
            cl = client.Client(0, args(out), Data, device=_dev())
            cl.backbone_state_dict = sd
            fc0 = cl.fc_module.fc.data.clone()
            cl.train(0, callback_verification=cb)
            rec = cb.client_record[0]
            assert [s for s, _ in rec] == [-1, 0] and list(cb.client_record) == [0]
            assert all(len(r) == 6 and all(0.0 <= v <= 100.0 for v in r) for _, r in rec)
            log = (out / "clients" / "client_0" / "local_log.txt").read_text().splitlines()
            assert log == ["Target label from 0 to 1", "Epoch -1, TPR (-1 to -6) = %r" % rec[0][1],
                           "Target label from 0 to 1", "Epoch 0, TPR (-1 to -6) = %r" % rec[1][1]]
            saved = torch.load(out / "clients" / "client_0" / "backbone.pth")
            trained = cl.get_model()
            assert list(saved.keys()) == list(sd.keys()) and all(not v.is_cuda for v in saved.values())
            assert torch.equal(saved["conv1.weight"], trained["conv1.weight"].cpu()) and not torch.equal(saved["conv1.weight"], sd["conv1.weight"])
            m = _tiny_backbone()                                       # the logged rows are those of the incoming and of the trained model
            for step, state in ((-1, sd), (0, trained)):
                m.load_state_dict(state)
                cb.veri_test(m.eval(), 7, cl.target_ID, 5)
                assert cb.client_record[5][-1] == (7, dict(rec)[step])
            with pytest.raises(ValueError, match="client 6 .*same-label"):
                cb.veri_test(m, 7, [7, 8], 6)                          # nobody in the test set has these identities

            quiet = tmp_path / "without"
            cl2 = client.Client(0, args(quiet), Data, device=_dev())
            cl2.backbone_state_dict = sd
            cl2.fc_module.update_from_tensor(fc0)                      # the same initial head: the two runs differ in the callback only
            cl2.train(0)
            assert not quiet.exists()
            assert torch.equal(cl2.get_model()["conv1.weight"], trained["conv1.weight"])        # the hooks change nothing in the training

            out_s = tmp_path / "server"
            cbs = eval_local.CallBack_LocalVerifi(1, 0, None, output_dir=str(out_s), loader=veri, verbose=False)
            clients = [client.Client(c, args(out_s), Data, device=_dev()) for c in range(2)]
            srv = server.Server(clients, Data, args(out_s), device=_dev())
            srv.federated_model.load_state_dict(sd)
            assert srv.callback_local_veri is None and srv.local_candidates == []
            srv.train()
            assert not out_s.exists() and not cbs.client_record                                   # never enabled: as before
            srv.enable_local_verification(cbs, candidates=[0])
            srv.federated_model.load_state_dict(sd)
            srv.train()
            assert list(cbs.client_record) == [0] and [s for s, _ in cbs.client_record[0]] == [-1, 0]
            assert (out_s / "clients" / "client_0" / "backbone.pth").exists() and not (out_s / "clients" / "client_1").exists()
            assert cbs.client_record[0][0][1] == rec[0][1]                                       # same incoming model, same test set
            state = np.random.get_state()
            np.random.seed(11)
            want = sorted(int(c) for c in np.random.permutation(2)[:10])
            np.random.seed(11)
            srv.enable_local_verification(cbs)
            np.random.set_state(state)
            assert srv.local_candidates == want == [0, 1]
    finally:
        cfg.lr = old_lr
