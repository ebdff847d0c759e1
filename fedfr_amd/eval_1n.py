"""1:N identification (TPIR at FPIR) of a personalised client model — reference local_all.py:142-176 ``evaluation`` and its
``--task 1:n`` client loop (:274-297).  The GPU part (``fedfr_ident_topk``) computes every query x gallery score in fp64 without
materialising the matrix and keeps, per client gallery, one positive score per query and the exact top-K of the negatives; the
read-out (K-th largest negative = threshold, rate of positives above it) is a few lines on the host, as in the reference."""
from __future__ import annotations

import math
from typing import List, Sequence, Tuple

import numpy as np
import torch

from . import _C

FARS = (1e-6, 1e-5, 1e-4, 1e-3)
MAX_K = 1024          # fedfr_ident_topk's limit on K (include/fedfr_hip.h)


@torch.no_grad()
def identification_topk(query: torch.Tensor, qid: torch.Tensor, gallery: torch.Tensor, gid: torch.Tensor, seg: Sequence[int],
                        K: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Scores <query[q], gallery[c]> in fp64 for every pair.  Pair (q, c) is positive iff qid[q] >= 0 and qid[q] == gid[c]; every other
    pair is a negative of the segment owning column c (segment s = columns [seg[s], seg[s+1]), one per client gallery).

    ``query`` [Q, D] / ``gallery`` [G, D] fp32 and ``qid`` [Q] / ``gid`` [G] int64 on the GPU; ``seg`` S+1 host integers from 0 to G.
    Returns ``pos`` [Q] fp64 (NaN where a query has no positive), ``neg_topk`` [S, K] fp64 (the K largest negatives of each segment,
    duplicates counted, descending; -inf past the segment's negative count) and ``neg_count`` [S] int64."""
    query = _C.require_gpu_tensor(query.contiguous(), torch.float32, "query")
    gallery = _C.require_gpu_tensor(gallery.contiguous(), torch.float32, "gallery")
    qid = _C.require_gpu_tensor(qid.contiguous(), torch.int64, "qid")
    gid = _C.require_gpu_tensor(gid.contiguous(), torch.int64, "gid")
    if query.dim() != 2 or gallery.dim() != 2 or query.shape[1] != gallery.shape[1]:
        raise ValueError("identification_topk: query [Q, D] and gallery [G, D] must share D (got %s, %s)"
                         % (tuple(query.shape), tuple(gallery.shape)))
    Q, D = query.shape
    G = gallery.shape[0]
    if tuple(qid.shape) != (Q,) or tuple(gid.shape) != (G,):
        raise ValueError("identification_topk: qid must be [Q] and gid [G]")
    seg_h = np.ascontiguousarray(np.asarray(seg.cpu() if torch.is_tensor(seg) else seg, dtype=np.int64))
    S = seg_h.shape[0] - 1
    if seg_h.ndim != 1 or S < 1:
        raise ValueError("identification_topk: seg must hold S + 1 >= 2 offsets")
    K = int(K)
    if not 1 <= K <= MAX_K:
        raise ValueError("identification_topk: K = %d outside [1, %d]" % (K, MAX_K))
    enrolled = gid[gid >= 0]
    if torch.unique(enrolled).numel() != enrolled.numel():
        raise ValueError("identification_topk: the non-negative gallery ids must be distinct (a query would have several positives)")
    dev = query.device
    pos = torch.empty(Q, dtype=torch.float64, device=dev)
    neg_topk = torch.empty(S, K, dtype=torch.float64, device=dev)
    neg_count = torch.empty(S, dtype=torch.int64, device=dev)
    ws = torch.empty(int(_C.lib().fedfr_ident_workspace_bytes(Q, S, K)), dtype=torch.uint8, device=dev)
    _C.call("fedfr_ident_topk", query.data_ptr(), qid.data_ptr(), Q, gallery.data_ptr(), gid.data_ptr(), G, D, seg_h.ctypes.data, S, K,
            pos.data_ptr(), neg_topk.data_ptr(), neg_count.data_ptr(), ws.data_ptr(), ws.numel(), _C.stream(query))
    return pos, neg_topk, neg_count


def required_topk(num_queries: int, fars: Sequence[float] = FARS) -> List[int]:
    """ceil(Q * far): the rank of each threshold among the negatives (local_all.py:152, Q counts every query)."""
    return [math.ceil(num_queries * x) for x in fars]


def identification_rates(pos, neg_topk, num_queries: int, num_gallery: int, imgs_per_id: int = 40,
                         fars: Sequence[float] = FARS) -> Tuple[List[float], List[float]]:
    """Host read-out of one client (local_all.py:167-173): th = the ceil(Q * far)-th largest negative, rate = count(pos > th) /
    (imgs_per_id * G).  ``pos``: the positive scores of the client's queries (NaN entries never count), ``neg_topk``: its sorted
    negatives.  Returns (rates, thresholds)."""
    pos = np.asarray(pos.cpu() if torch.is_tensor(pos) else pos, dtype=np.float64)
    neg = np.asarray(neg_topk.cpu() if torch.is_tensor(neg_topk) else neg_topk, dtype=np.float64).reshape(-1)
    rates, ths = [], []
    for k in required_topk(num_queries, fars):
        th = neg[k - 1]
        rates.append(np.sum(pos > th) / (imgs_per_id * num_gallery))
        ths.append(float(th))
    return rates, ths


def _to_gpu_f32(x, name):
    if torch.is_tensor(x):
        return _C.require_gpu_tensor(x.to(torch.float32).contiguous(), torch.float32, name)
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.cuda.current_device())


def _host_i64(x):
    return np.asarray(x.cpu() if torch.is_tensor(x) else x).astype(np.int64).reshape(-1)


def _check_negatives(num_neg: int, K: int, what: str):
    if num_neg < K:
        raise ValueError("%s: %d negative pairs but the threshold at the smallest FAR needs the %d-th largest (the reference raises "
                         "IndexError here)" % (what, num_neg, K))


def evaluation(query_feats, gallery_feats, mask, imgs_per_id: int = 40, fars: Sequence[float] = FARS):
    """Drop-in for local_all.evaluation: query [Q, D], gallery [G, D] (numpy arrays, or torch tensors on the GPU), ``mask`` [Q] =
    the gallery row of each query's identity or -1.  Returns (rates, fars) with the reference's values."""
    query = _to_gpu_f32(query_feats, "query_feats")
    gallery = _to_gpu_f32(gallery_feats, "gallery_feats")
    Q, G = query.shape[0], gallery.shape[0]
    m = _host_i64(mask)
    if m.shape[0] != Q:
        raise ValueError("evaluation: mask has %d entries for %d queries" % (m.shape[0], Q))
    if np.any((m < -1) | (m >= G)):
        raise ValueError("evaluation: mask entries must be -1 or a gallery row in [0, %d)" % G)
    K = max(required_topk(Q, fars))
    _check_negatives(Q * G - int(np.sum(m >= 0)), K, "evaluation")
    if K > MAX_K:
        raise ValueError("evaluation: ceil(Q * far) = %d exceeds the kernel's K limit %d" % (K, MAX_K))
    dev = query.device
    pos, neg, _ = identification_topk(query, torch.from_numpy(m).to(dev), gallery, torch.arange(G, dtype=torch.int64, device=dev),
                                      [0, G], K)
    rates, _ = identification_rates(pos, neg[0], Q, G, imgs_per_id, fars)
    return rates, list(fars)


def combine_features(feats, labels, start_id: int, end_id: int):
    """Per-identity float32 mean of the gallery images of ids [start_id, end_id) — local_all.py:131-140, not re-normalised."""
    feats, labels = np.asarray(feats), np.asarray(labels)
    mean_feats = [np.mean(feats[np.where(labels == i)[0]], axis=0, keepdims=True) for i in range(start_id, end_id)]
    return np.concatenate(mean_feats, axis=0), np.arange(start_id, end_id)


def local_1n(query_feats, query_labels, gallery_img_feats, gallery_img_labels, num_client: int, num_ids: int = 4000,
             imgs_per_id: int = 40, fars: Sequence[float] = FARS):
    """The reference's ``--task 1:n`` loop (local_all.py:274-297) in ONE kernel call: client c's gallery is the mean feature of ids
    [c * (num_ids // num_client), (c + 1) * ...), its enrolled queries are the rows of those ids.  The query rows must have the layout
    the reference's positional mask assumes (the first num_ids * imgs_per_id rows are ids 0, 0, ..., 1, 1, ... with imgs_per_id rows
    each).  Returns (mean over clients [4], per-client rates [num_client, 4], fars)."""
    labels = _host_i64(query_labels)
    Q = labels.shape[0]
    n_enrolled = num_ids * imgs_per_id
    if Q < n_enrolled or not np.array_equal(labels[:n_enrolled], np.repeat(np.arange(num_ids, dtype=np.int64), imgs_per_id)):
        raise ValueError("local_1n: the first %d query rows must be ids 0..%d in order, %d rows each (the reference's positional mask)"
                         % (n_enrolled, num_ids - 1, imgs_per_id))
    per = num_ids // num_client
    if per < 1:
        raise ValueError("local_1n: %d clients for %d ids" % (num_client, num_ids))
    g_feats = np.asarray(gallery_img_feats)
    g_labels = np.asarray(gallery_img_labels)
    gallery = np.concatenate([combine_features(g_feats, g_labels, c * per, (c + 1) * per)[0] for c in range(num_client)], axis=0)
    G = gallery.shape[0]                                       # = num_client * per: gallery row r holds id r
    qid = np.full(Q, -1, dtype=np.int64)
    qid[:G * imgs_per_id] = labels[:G * imgs_per_id]
    K = max(required_topk(Q, fars))
    _check_negatives(Q * per - per * imgs_per_id, K, "local_1n")
    if K > MAX_K:
        raise ValueError("local_1n: ceil(Q * far) = %d exceeds the kernel's K limit %d" % (K, MAX_K))
    query = _to_gpu_f32(query_feats, "query_feats")
    dev = query.device
    pos, neg, _ = identification_topk(query, torch.from_numpy(qid).to(dev), _to_gpu_f32(gallery, "gallery"),
                                      torch.arange(G, dtype=torch.int64, device=dev), [c * per for c in range(num_client + 1)], K)
    pos, neg = pos.cpu().numpy(), neg.cpu().numpy()
    results = []
    for c in range(num_client):
        rows = slice(c * per * imgs_per_id, (c + 1) * per * imgs_per_id)
        results.append(identification_rates(pos[rows], neg[c], Q, per, imgs_per_id, fars)[0])
    results = np.array(results)
    return np.mean(results, axis=0), results, list(fars)
