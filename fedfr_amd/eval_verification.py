"""LFW-style k-fold 1:1 verification (reference eval/verification.py: agedb_30 / cfp_fp / lfw, run by ``server.test()`` every round).

GPU part (``fedfr_amd/csrc/verif.hip``, ``fold_counts``): one pass over the embeddings of a verification set adds the flipped set, normalises
the rows, takes the squared distance of every pair and counts the pairs by fold, label and first threshold above the distance, for the
two threshold tables of ``evaluate`` at once; the mean embedding norm (``xnorm``) comes out of the same pass.

Host part (numpy): every number the reference computes by re-reducing the pairs per fold and threshold is a function of those two
small integer tables.  ``roc_from_counts`` repeats ``calculate_roc`` / ``calculate_accuracy`` with the same float expressions
(``float(tp) / float(tp + fn)``, ``float(tp + tn) / size``, first maximum of the train accuracy), ``val_far_from_counts`` the per-threshold
``calculate_val_far`` tables of ``calculate_val``.

The FAR-target pick of ``calculate_val`` is build-defined: the reference hands the step function far_train to
``interp1d(kind='slinear')``, which rejects duplicate x values in current scipy; ``pick_far_threshold`` uses ``interp1d`` where it accepts
the table and otherwise keeps the smallest threshold of every distinct FAR value and interpolates linearly.  ``val`` / ``val_std`` /
``far`` therefore carry no reference-parity claim; ``verification.test`` discards them.

Not ported: ``pca > 0`` (never passed by the reference), ``dumpR`` (mxnet), the ``.pkl`` image cache of ``load_bin``."""
from __future__ import annotations

import io
import pickle
from collections import namedtuple
from typing import List, Sequence, Tuple

import numpy as np
import torch

from . import _C

FAR_TARGET = 1e-3                                   # evaluate(): calculate_val(..., 1e-3, ...)
STATUS_NAN = 1

FoldCounts = namedtuple("FoldCounts", "counts_a counts_b dist norm_sum status")


def roc_thresholds():
    return np.arange(0, 4, 0.01)


def val_thresholds():
    return np.arange(0, 4, 0.001)


def fold_ranges(n_pairs: int, nfolds: int) -> List[Tuple[int, int]]:
    """[start, stop) of the test set of every fold: ``KFold(n_splits=nfolds, shuffle=False)`` over ``n_pairs`` indices (the first
    ``n_pairs % nfolds`` folds hold one more).  ``nfolds`` = 1 is the reference's ``LFold``: one range, train = test."""
    if nfolds < 1 or nfolds > n_pairs:
        raise ValueError("verification: nfolds = %d must be in [1, number of pairs = %d]" % (nfolds, n_pairs))
    q, r = divmod(n_pairs, nfolds)
    out, start = [], 0
    for f in range(nfolds):
        stop = start + q + (1 if f < r else 0)
        out.append((start, stop))
        start = stop
    return out


# ---- the kernel ------------------------------------------------------------------------------------------------------------------
def _device():
    return torch.device("cuda", torch.cuda.current_device())


def _thr_tensor(thr, device):
    if thr is None:
        return None
    t = np.ascontiguousarray(np.asarray(thr.detach().cpu() if torch.is_tensor(thr) else thr, dtype=np.float64).reshape(-1))
    if t.size < 1 or np.any(np.diff(t) < 0) or not np.all(np.isfinite(t)):
        raise ValueError("verification: thresholds must be a non-empty, finite, ascending table")
    return torch.from_numpy(t).to(device)


@torch.no_grad()
def fold_counts(emb0: torch.Tensor, emb1, issame: torch.Tensor, nfolds: int, thr_a=None, thr_b=None, normalize: bool = True,
                return_dist: bool = True) -> FoldCounts:
    """One fused pass (``fedfr_verif_fold_counts``) over ``emb0`` [2P, D] and ``emb1`` [2P, D] or None (GPU tensors, both fp32 or both
    fp64), rows 2p and 2p + 1 forming pair p with label ``issame`` [P] (GPU tensor): s = emb0 + emb1, normalised per row like
    ``sklearn.preprocessing.normalize`` (``normalize=False``: taken as it is), dist = sum((s[2p] - s[2p + 1]) ** 2), all in fp64.
    ``thr_a`` / ``thr_b``: ascending threshold tables (default ``np.arange(0, 4, 0.01)`` and ``np.arange(0, 4, 0.001)``, uploaded from numpy's
    values; pass ``thr_b=False`` for one table).  Returns GPU tensors: counts_a int64 [nfolds, 2, Ta + 1] and counts_b [nfolds, 2, Tb + 1]
    (pairs by fold, issame and k0 = number of thresholds <= dist: the pair is accepted by thresholds k >= k0, never in bin T), dist [P]
    fp64, norm_sum (fp64 scalar: sum of the L2 norms of all rows of emb0 and emb1) and status (int32 [1]; bit 1: a NaN distance)."""
    if emb0.dtype not in (torch.float32, torch.float64):
        raise RuntimeError("fedfr_amd: verification embeddings must be float32 or float64 (got %s)" % emb0.dtype)
    emb0 = _C.require_gpu_tensor(emb0, emb0.dtype, "emb0")
    if emb1 is not None:
        emb1 = _C.require_gpu_tensor(emb1, emb0.dtype, "emb1")
        if emb1.shape != emb0.shape:
            raise ValueError("verification: emb0 %s and emb1 %s differ in shape" % (tuple(emb0.shape), tuple(emb1.shape)))
    if emb0.dim() != 2 or emb0.shape[0] % 2:
        raise ValueError("verification: embeddings must be [2P, D] (got %s)" % (tuple(emb0.shape),))
    P, D = emb0.shape[0] // 2, emb0.shape[1]
    same = _C.require_gpu_tensor(issame.to(torch.uint8).contiguous(), torch.uint8, "issame")
    if same.shape != (P,):
        raise ValueError("verification: issame must hold one entry per pair (%d), got %s" % (P, tuple(same.shape)))
    dev = emb0.device
    ta = _thr_tensor(roc_thresholds() if thr_a is None else thr_a, dev)
    tb = None if thr_b is False else _thr_tensor(val_thresholds() if thr_b is None else thr_b, dev)
    Ta, Tb = ta.numel(), (tb.numel() if tb is not None else 0)
    counts_a = torch.empty(nfolds, 2, Ta + 1, dtype=torch.int64, device=dev)
    counts_b = torch.empty(nfolds, 2, Tb + 1, dtype=torch.int64, device=dev) if tb is not None else None
    dist = torch.empty(P, dtype=torch.float64, device=dev) if return_dist else None
    norm_sum = torch.empty((), dtype=torch.float64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    nbytes = _C.lib().fedfr_verif_workspace_bytes(P, nfolds)
    ws = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=dev)
    _C.call("fedfr_verif_fold_counts", emb0.data_ptr(), _C.ptr(emb1), 1 if emb0.dtype == torch.float64 else 0, 1 if normalize else 0,
            same.data_ptr(), P, D, nfolds, ta.data_ptr(), Ta, _C.ptr(tb), Tb, counts_a.data_ptr(), _C.ptr(counts_b), _C.ptr(dist),
            norm_sum.data_ptr(), status.data_ptr(), ws.data_ptr(), nbytes, _C.stream(emb0))
    return FoldCounts(counts_a, counts_b, dist, norm_sum, status)


# ---- host read-out of the count tables --------------------------------------------------------------------------------------------
def _host_counts(counts) -> np.ndarray:
    c = counts.cpu().numpy() if torch.is_tensor(counts) else np.asarray(counts)
    if c.ndim != 3 or c.shape[1] != 2 or c.shape[2] < 2:
        raise ValueError("verification: counts must be [nfolds, 2, T + 1]")
    return c.astype(np.int64, copy=False)


def _accepted(counts):
    """(tp, fp) [nfolds, T] of every fold's test set at every threshold, (n_same, n_diff) [nfolds]."""
    c = _host_counts(counts)
    cum = np.cumsum(c, axis=2)[:, :, :-1]             # accepted at threshold k: k0 <= k; bin T (dist >= every threshold, NaN) never
    return cum[:, 1, :], cum[:, 0, :], c[:, 1, :].sum(axis=1), c[:, 0, :].sum(axis=1)


def _train(tp, fp, n_same, n_diff):
    """Train-set numbers of every fold: the total minus the fold's own (KFold), or the fold itself when there is only one (LFold)."""
    if tp.shape[0] == 1:
        return tp, fp, n_same, n_diff
    return tp.sum(0, keepdims=True) - tp, fp.sum(0, keepdims=True) - fp, n_same.sum() - n_same, n_diff.sum() - n_diff


def _ratio(num, den):
    """``0 if den == 0 else float(num) / float(den)`` elementwise."""
    out = np.zeros(np.broadcast(num, den).shape, np.float64)
    np.divide(num.astype(np.float64), den.astype(np.float64), out=out, where=den != 0)
    return out


def _accuracy_terms(tp, fp, n_same, n_diff):
    """calculate_accuracy at every (fold, threshold): tpr, fpr, acc."""
    fn, tn = n_same[:, None] - tp, n_diff[:, None] - fp
    size = (n_same + n_diff)[:, None]
    if np.any(size == 0):
        raise ZeroDivisionError("verification: a fold without pairs")
    return _ratio(tp, tp + fn), _ratio(fp, fp + tn), (tp + tn).astype(np.float64) / size.astype(np.float64)


def roc_from_counts(counts, return_best: bool = False):
    """``calculate_roc`` from the count table of its thresholds: (tpr [T], fpr [T], accuracy [nfolds]) — per fold the test accuracy at the
    FIRST threshold of maximal train accuracy (np.argmax), tpr / fpr the means of the folds' test curves."""
    tp, fp, n_same, n_diff = _accepted(counts)
    tprs, fprs, acc_test = _accuracy_terms(tp, fp, n_same, n_diff)
    _, _, acc_train = _accuracy_terms(*_train(tp, fp, n_same, n_diff))
    best = np.argmax(acc_train, axis=1)
    accuracy = acc_test[np.arange(tp.shape[0]), best]
    out = (np.mean(tprs, 0), np.mean(fprs, 0), accuracy)
    return out + (best,) if return_best else out


def val_far_from_counts(counts):
    """``calculate_val_far`` on every fold's TRAIN set at every threshold: (val_train, far_train) [nfolds, T] =
    float(true_accept) / float(n_same), float(false_accept) / float(n_diff)."""
    tp, fp, n_same, n_diff = _train(*_accepted(counts))
    n_same, n_diff = np.broadcast_to(n_same, (tp.shape[0],)), np.broadcast_to(n_diff, (tp.shape[0],))
    if np.any(n_same == 0) or np.any(n_diff == 0):
        raise ZeroDivisionError("float division by zero")               # what the reference's float(...) / float(0) raises
    return tp.astype(np.float64) / n_same[:, None].astype(np.float64), fp.astype(np.float64) / n_diff[:, None].astype(np.float64)


def pick_far_threshold(far_train, thresholds, far_target):
    """The threshold at which the train FAR reaches ``far_target`` (calculate_val): ``interp1d(far_train, thresholds, 'slinear')`` where
    scipy accepts the table; where it raises for duplicate FAR values (a step function always has them), the build's rule: keep the
    smallest threshold of every distinct FAR value and interpolate linearly between those points.  Any other error of ``interp1d`` (a
    table without duplicates) is raised as it is; without scipy the rule is used throughout.  0.0 when the FAR never reaches the target."""
    far_train, thresholds = np.asarray(far_train, np.float64), np.asarray(thresholds, np.float64)
    if not np.max(far_train) >= far_target:
        return 0.0
    x, first = np.unique(far_train, return_index=True)                  # far_train is non-decreasing: first index = smallest threshold
    try:
        from scipy import interpolate
        return float(interpolate.interp1d(far_train, thresholds, kind="slinear")(far_target))
    except ImportError:                                                 # no scipy: the rule below (equal to 'slinear' on a table it accepts)
        pass
    except ValueError:
        if len(x) == len(far_train):                                    # no duplicate FAR value: not the rejection the rule stands in for
            raise
    if far_target < x[0]:
        raise ValueError("verification: far_target %g below the smallest train FAR %g" % (far_target, x[0]))
    return float(np.interp(far_target, x, thresholds[first]))


def calculate_accuracy(threshold, dist, actual_issame):
    """reference eval/verification.py:109-121 (host numpy; the k-fold paths read these numbers from the count tables instead)."""
    dist, actual_issame = np.asarray(dist), np.asarray(actual_issame).astype(bool)
    predict = np.less(dist, threshold)
    tp = int(np.sum(predict & actual_issame))
    fp = int(np.sum(predict & ~actual_issame))
    tn = int(np.sum(~predict & ~actual_issame))
    fn = int(np.sum(~predict & actual_issame))
    tpr = 0 if tp + fn == 0 else float(tp) / float(tp + fn)
    fpr = 0 if fp + tn == 0 else float(fp) / float(fp + tn)
    return tpr, fpr, float(tp + tn) / dist.size


def calculate_val_far(threshold, dist, actual_issame):
    """reference eval/verification.py:165-176."""
    dist, actual_issame = np.asarray(dist), np.asarray(actual_issame).astype(bool)
    predict = np.less(dist, threshold)
    true_accept, false_accept = int(np.sum(predict & actual_issame)), int(np.sum(predict & ~actual_issame))
    n_same, n_diff = int(np.sum(actual_issame)), int(np.sum(~actual_issame))
    return float(true_accept) / float(n_same), float(false_accept) / float(n_diff)


def _val_from(counts_b, thresholds, dist, issame, far_target):
    """calculate_val's fold loop from the fine count table and the distances: (val_mean, val_std, far_mean)."""
    _, far_train = val_far_from_counts(counts_b)
    issame = np.asarray(issame).astype(bool)
    ranges = fold_ranges(len(dist), far_train.shape[0])
    val, far = np.zeros(len(ranges)), np.zeros(len(ranges))
    for f, (a, b) in enumerate(ranges):
        thr = pick_far_threshold(far_train[f], thresholds, far_target)
        val[f], far[f] = calculate_val_far(thr, dist[a:b], issame[a:b])
    return np.mean(val), np.std(val), np.mean(far)


def _pairs_to_rows(e1, e2):
    """embeddings1 / embeddings2 [P, D] (numpy or torch, any device) -> one fp64 [2P, D] GPU tensor with pair p in rows 2p, 2p + 1."""
    def gpu(x):
        t = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float64)))
        return t.to(device=_device(), dtype=torch.float64)
    a, b = gpu(e1), gpu(e2)
    assert a.shape[0] == b.shape[0]
    assert a.shape[1] == b.shape[1]
    return torch.stack((a, b), dim=1).reshape(2 * a.shape[0], a.shape[1]).contiguous()


def _labels(actual_issame, n_pairs):
    a = actual_issame.detach().cpu().numpy() if torch.is_tensor(actual_issame) else np.asarray(actual_issame)
    a = a.astype(bool).reshape(-1)
    if len(a) < n_pairs:
        raise ValueError("verification: %d labels for %d pairs" % (len(a), n_pairs))
    return a[:n_pairs]


def _check(status):
    if int(status.item()) & STATUS_NAN:
        import warnings
        warnings.warn("fedfr_amd verification: an embedding pair has a NaN distance; it is accepted by no threshold (as np.less does)")


def _no_pca(pca):
    if pca > 0:
        raise NotImplementedError("fedfr_amd verification: pca > 0 is not ported (the reference never passes it)")


@torch.no_grad()
def calculate_roc(thresholds, embeddings1, embeddings2, actual_issame, nrof_folds=10, pca=0):
    """reference eval/verification.py:54-106 through the fused kernel: (tpr, fpr, accuracy)."""
    _no_pca(pca)
    rows = _pairs_to_rows(embeddings1, embeddings2)
    same = _labels(actual_issame, rows.shape[0] // 2)
    res = fold_counts(rows, None, torch.from_numpy(same).to(rows.device), nrof_folds, thr_a=thresholds, thr_b=False, normalize=False,
                      return_dist=False)
    _check(res.status)
    return roc_from_counts(res.counts_a)


@torch.no_grad()
def calculate_val(thresholds, embeddings1, embeddings2, actual_issame, far_target, nrof_folds=10):
    """reference eval/verification.py:124-162 through the fused kernel: (val_mean, val_std, far_mean); the FAR-target pick is
    ``pick_far_threshold`` (build-defined where scipy rejects the reference's table)."""
    rows = _pairs_to_rows(embeddings1, embeddings2)
    same = _labels(actual_issame, rows.shape[0] // 2)
    res = fold_counts(rows, None, torch.from_numpy(same).to(rows.device), nrof_folds, thr_a=thresholds, thr_b=False, normalize=False)
    _check(res.status)
    return _val_from(res.counts_a, np.asarray(thresholds, np.float64), res.dist.cpu().numpy(), same, far_target)


def _evaluate_counts(res: FoldCounts, same):
    tpr, fpr, accuracy = roc_from_counts(res.counts_a)
    val, val_std, far = _val_from(res.counts_b, val_thresholds(), res.dist.cpu().numpy(), same, FAR_TARGET)
    return tpr, fpr, accuracy, val, val_std, far


@torch.no_grad()
def evaluate(embeddings, actual_issame, nrof_folds=10, pca=0):
    """reference eval/verification.py:179-197 on [2P, D] embeddings (numpy or torch; taken as they are, like the reference): one
    kernel pass for both threshold tables.  Returns (tpr, fpr, accuracy, val, val_std, far)."""
    _no_pca(pca)
    e = embeddings if torch.is_tensor(embeddings) else torch.from_numpy(np.ascontiguousarray(np.asarray(embeddings, dtype=np.float64)))
    e = e.to(device=_device(), dtype=torch.float64).contiguous()
    same = _labels(actual_issame, e.shape[0] // 2)
    res = fold_counts(e, None, torch.from_numpy(same).to(e.device), nrof_folds, normalize=False)
    _check(res.status)
    return _evaluate_counts(res, same)


# ---- data sets -------------------------------------------------------------------------------------------------------------------
def load_bin(path, image_size, device=None):
    """``(bins, issame_list)`` pickle of encoded images (the insightface .bin of lfw / cfp_fp / agedb_30) -> the compact data set
    ``(uint8 [2P, H, W, 3] tensor on the GPU, issame_list)``: one byte per pixel-channel, resident once; ``test`` mirrors it on the fly.
    Images are decoded with PIL and must already be ``image_size`` (the reference resizes with mxnet's ``resize_short``, whose
    interpolation is not reproduced).  The reference's ``.pkl`` cache beside the file is neither read nor written."""
    from PIL import Image
    try:
        with open(path, "rb") as f:
            bins, issame_list = pickle.load(f)
    except UnicodeDecodeError:
        with open(path, "rb") as f:
            bins, issame_list = pickle.load(f, encoding="bytes")
    n = len(issame_list) * 2
    H, W = int(image_size[0]), int(image_size[1])
    data = np.empty((n, H, W, 3), np.uint8)
    for idx in range(n):
        b = bins[idx]
        img = Image.open(io.BytesIO(b.tobytes() if hasattr(b, "tobytes") else bytes(b))).convert("RGB")
        if img.size != (W, H):
            raise ValueError("load_bin: image %d of %s is %dx%d, not %dx%d — resize the set offline (resize_short's interpolation is not "
                             "reproduced here)" % (idx, path, img.size[1], img.size[0], H, W))
        data[idx] = np.asarray(img)
    dev = torch.device(device) if device is not None else _device()
    return torch.from_numpy(data).to(dev), issame_list


def _embed(data, flip: int, backbone, batch_size: int, device) -> torch.Tensor:
    """The reference's batch loop (:245-259): full batches; the last one re-reads the final ``batch_size`` rows and keeps the new ones."""
    from . import ops
    n = data.shape[0]
    bs = min(int(batch_size), n)                      # a set smaller than one batch: a single batch of the whole set
    emb = None
    ba = 0
    while ba < n:
        bb = min(ba + bs, n)
        count = bb - ba
        chunk = data[bb - bs: bb]
        if chunk.dtype == torch.uint8:                # compact form: transform and mirror on the device
            chunk = chunk.to(device).contiguous()
            img = ops.preprocess_u8(chunk, torch.ones(bs, dtype=torch.uint8, device=device) if flip else None)
        else:                                         # reference form: fp32 NCHW in 0 .. 255, transformed where it lives (the host, as in
            img = (((chunk / 255) - 0.5) / 0.5).to(device)    # the reference: torch's device division by a scalar rounds differently)
        out = backbone(img.contiguous())
        if emb is None:
            emb = torch.empty(n, out.shape[1], dtype=torch.float32, device=device)
        emb[ba:bb] = out[bs - count:]
        ba = bb
    return emb


@torch.no_grad()
def test(data_set, backbone, batch_size, nfolds=10):
    """reference eval/verification.py:234-282: embed the set and its mirror image, xnorm, flip sum, normalise, ``evaluate``.  Returns
    ``(acc1 = 0.0, std1 = 0.0, acc2, std2, xnorm, embeddings_list)``; ``embeddings_list`` = two fp64 numpy arrays, read back once.
    ``data_set``: the reference's ``([fp32 [2P, 3, H, W] in 0 .. 255, the same mirrored], issame_list)`` or ``load_bin``'s compact
    ``(uint8 [2P, H, W, 3], issame_list)``.  ``backbone`` maps fp32 [B, 3, H, W] in [-1, 1] on the GPU to [B, D] (call it in eval mode)."""
    data, issame_list = data_set[0], data_set[1]
    dev = next(backbone.parameters()).device if hasattr(backbone, "parameters") else _device()
    with torch.cuda.device(dev):
        if torch.is_tensor(data):
            if data.dtype != torch.uint8 or data.dim() != 4 or data.shape[3] != 3:
                raise ValueError("verification.test: the compact data set is one uint8 [2P, H, W, 3] tensor")
            embs = [_embed(data, flip, backbone, batch_size, dev) for flip in (0, 1)]
        else:
            embs = [_embed(d, 0, backbone, batch_size, dev) for d in data]
        same = _labels(issame_list, embs[0].shape[0] // 2)
        res = fold_counts(embs[0], embs[1] if len(embs) > 1 else None, torch.from_numpy(same).to(dev), nfolds)
        _check(res.status)
        xnorm = float(res.norm_sum.item()) / (min(len(embs), 2) * embs[0].shape[0])
        _, _, accuracy, _, _, _ = _evaluate_counts(res, same)
        embeddings_list = [e.cpu().numpy().astype(np.float64) for e in embs]
    acc2, std2 = np.mean(accuracy), np.std(accuracy)
    return 0.0, 0.0, acc2, std2, xnorm, embeddings_list
