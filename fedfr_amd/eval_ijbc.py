"""IJB-C template evaluation, jobs 1:1 and 1:N (reference ijbc_all.py, driven by ijbc_conti.py): everything after the forward pass.

GPU part of job 1:1 (``fedfr_amd/csrc/ijbc.hip``): template pooling in the reference's fp32 order with the fp64 normalisation
(``fedfr_template_pool``), pair scores in numpy's summation order fused with the exact ROC counts at the genuine scores
(``fedfr_pair_scores_roc``).  The TPR@FPR table is read out on the host from those counts with the float operations of
``sklearn.metrics.roc_curve`` and the reference's nearest-FPR pick (:570-586), so no sort of the scores is needed.

Job 1:N (:261-298, 356-427, 592-627): ``template_pool(mode=1)`` gives the gallery and probe template features bit for bit, and
``fedfr_ident_rank_topk`` (``fedfr_amd/csrc/ident64.hip``) scores probes x gallery in fp64 without writing the matrix: per probe the score
of its own gallery row and the number of other rows that score higher (top-1 / 5 / 10), over all probes the exact top-K negatives
(TPIR at FAR 0.01 and 0.1).  Scores are summed in another order than the reference's BLAS ``np.dot``, so a comparison decided within
about D * 2^-52 can fall the other way; exact ties are reported (``evaluation(..., return_ties=True)``).

Not ported: face alignment (cv2 / skimage ``warpAffine``) and the embedding loop."""
from __future__ import annotations

import math
from typing import Callable, Dict, Sequence, Tuple

import numpy as np
import torch

from . import _C

X_LABELS = (1e-6, 1e-5, 1e-4, 1e-3, 1e-2, 1e-1)
FARS_1N = (0.01, 0.1)           # ijbc_all.py:368
MAX_K_1N = 4096                 # fedfr_ident_rank_topk's limit on K (include/fedfr_hip.h)


# ---- meta lists of job 1:1 (ijbc_all.py:119-134, without the removed np.int) ---------------------------------------------------------------------
def _read_columns(path, cols, sep=None, skiprows=0):
    rows = []
    with open(path) as f:
        for i, line in enumerate(f):
            if i < skiprows or not line.strip():
                continue
            parts = line.strip().split(sep)
            rows.append([int(parts[c]) for c in cols])
    a = np.array(rows, dtype=np.int64).reshape(-1, len(cols))
    return tuple(a[:, k] for k in range(len(cols)))


def read_template_media_list(path):
    """``ijbc_face_tid_mid.txt`` (``name tid mid`` per image): templates, medias."""
    return _read_columns(path, (1, 2))


def read_template_pair_list(path):
    """``ijbc_template_pair_label.txt`` (``t1 t2 label`` per pair): t1, t2, label."""
    return _read_columns(path, (0, 1, 2))


def read_template_subject_id_list(path):
    """``ijbc_1N_gallery_G1.csv`` / ``..._probe_mixed.csv`` (a header row, then ``template_id,subject_id,...``): templates, subject ids."""
    return _read_columns(path, (0, 1), sep=",", skiprows=1)


# ---- template pooling ----------------------------------------------------------------------------------------------------------
def _device():
    return torch.device("cuda", torch.cuda.current_device())


def _gpu(x, dtype, name):
    if torch.is_tensor(x):
        return _C.require_gpu_tensor(x.to(dtype).contiguous(), dtype, name)
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x), dtype=_np_dtype(dtype))).to(_device())


def _np_dtype(dtype):
    return {torch.float32: np.float32, torch.float64: np.float64, torch.int64: np.int64, torch.int32: np.int32}[dtype]


def _host(x, dtype=None):
    a = x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    return a if dtype is None else a.astype(dtype, copy=False)


def _check_status(status, what):
    s = int(status.item())
    if s & 1:
        raise ValueError("%s: bad template / media CSR or image index" % what)
    if s & 2:
        raise ValueError("%s: a pair names a template id that has no template feature (p1 / p2)" % what)
    if s & 4:
        raise RuntimeError("%s: a genuine score is missing from the genuine table" % what)
    if s & 8:
        raise ValueError("%s: scores must be finite (roc_curve rejects NaN / inf)" % what)


def template_csr(templates, medias, choose_templates=None):
    """Host CSR in the reference's order: templates sorted by id (np.unique of ``choose_templates``, default ``templates``), medias
    sorted by id within a template, images in input order within a media.  Returns (unique_templates, t_off [T+1], m_off [M+1], img)."""
    templates = _host(templates, np.int64).reshape(-1)
    medias = _host(medias, np.int64).reshape(-1)
    if templates.shape != medias.shape:
        raise ValueError("template_csr: templates and medias must have one entry per image")
    uniq = np.unique(templates if choose_templates is None else _host(choose_templates, np.int64).reshape(-1))
    n = templates.shape[0]
    order = np.lexsort((np.arange(n), medias, templates))
    order = order[np.isin(templates[order], uniq)]
    ts, ms = templates[order], medias[order]
    new_media = np.ones(len(order), dtype=bool)
    new_media[1:] = (ts[1:] != ts[:-1]) | (ms[1:] != ms[:-1])
    media_start = np.nonzero(new_media)[0]
    m_off = np.append(media_start, len(order)).astype(np.int32)
    media_t = ts[media_start]                                           # template of each media, ascending
    t_off = np.searchsorted(media_t, uniq, side="left")
    t_off = np.append(t_off, len(media_start)).astype(np.int32)
    return uniq, t_off, m_off, order.astype(np.int32)


@torch.no_grad()
def template_pool(img_feats, templates, medias, choose_templates=None, faceness=None, flip=False, norm_images=False, mode=0,
                  return_raw=False):
    """Template features on the device.  ``img_feats`` [N, D] fp32 ([N, 2D] with ``flip``: F1), ``faceness`` [N] (D1) or None,
    ``norm_images``: divide every image by its L2 norm first (use_norm_score=False).  mode 0: sklearn normalize (1:1), 1: the explicit
    divide (1:N).  Returns (feats [T, D] fp64 on the GPU, unique_templates) and, with ``return_raw``, the fp32 pre-normalisation sums."""
    feats = _gpu(img_feats, torch.float32, "img_feats")
    if feats.dim() != 2:
        raise ValueError("template_pool: img_feats must be [N, D]")
    N, W = feats.shape
    if flip and W % 2:
        raise ValueError("template_pool: flip-test features must be [N, 2D] (got width %d)" % W)
    D = W // 2 if flip else W
    if _host(templates).reshape(-1).shape[0] != N:
        raise ValueError("template_pool: templates / medias must have one entry per image (%d)" % N)
    face = None
    if faceness is not None:
        face = _gpu(faceness, torch.float32, "faceness").reshape(-1)
        if face.shape[0] != N:
            raise ValueError("template_pool: faceness must have one entry per image (%d)" % N)
    uniq, t_off, m_off, img = template_csr(templates, medias, choose_templates)
    if len(img) == 0:
        raise ValueError("template_pool: no image belongs to a chosen template")
    dev = feats.device
    T, M = len(uniq), len(m_off) - 1
    out = torch.empty(T, D, dtype=torch.float64, device=dev)
    raw = torch.empty(T, D, dtype=torch.float32, device=dev) if return_raw else None
    ws = torch.empty(max(int(_C.lib().fedfr_template_pool_workspace_bytes(N, int(norm_images))), 1), dtype=torch.uint8, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    t_off_d, m_off_d, img_d = (torch.from_numpy(a).to(dev) for a in (t_off, m_off, img))
    _C.call("fedfr_template_pool", feats.data_ptr(), N, D, int(bool(flip)), face.data_ptr() if face is not None else None,
            int(bool(norm_images)), t_off_d.data_ptr(), T, m_off_d.data_ptr(), M, img_d.data_ptr(), len(img), int(mode),
            raw.data_ptr() if raw is not None else None, out.data_ptr(), ws.data_ptr(), ws.numel(), status.data_ptr(), _C.stream(feats))
    _check_status(status, "template_pool")
    return (out, uniq, raw) if return_raw else (out, uniq)


def image2template_feature_11(img_feats=None, templates=None, medias=None):
    """Drop-in for ijbc_all.image2template_feature_11: (template_norm_feats [T, D] fp64 numpy, unique_templates)."""
    out, uniq = template_pool(img_feats, templates, medias, mode=0)
    return out.cpu().numpy(), uniq


# ---- pair scores + ROC counts ----------------------------------------------------------------------------------------------------
def _row_lut(unique_templates, dev):
    uniq = _host(unique_templates, np.int64).reshape(-1)
    if uniq.size == 0 or uniq.min() < 0:
        raise ValueError("unique_templates must be non-negative template ids")
    lut = np.full(int(uniq.max()) + 1, -1, dtype=np.int32)
    lut[uniq] = np.arange(len(uniq), dtype=np.int32)
    return torch.from_numpy(lut).to(dev)


def _sorted_genuine(gen_scores):
    v = np.unique(_host(gen_scores, np.float64))[::-1].copy()
    if v.size and not np.all(np.isfinite(v)):
        raise ValueError("ROC counts: genuine scores must be finite")
    return v


@torch.no_grad()
def pair_scores(template_feats, unique_templates, p1, p2, label=None):
    """fp64 scores of template pairs (ids p1, p2) in input order, bit-identical to the reference's np.sum(f1 * f2, -1).  With ``label``
    also returns the ROC counts (genuine values descending, counts: see include/fedfr_hip.h fedfr_pair_scores_roc).
    Returns score [P] fp64 on the GPU, or (score, genuine, counts)."""
    feats = _gpu(template_feats, torch.float64, "template_feats")
    dev = feats.device
    T, D = feats.shape
    lut = _row_lut(unique_templates, dev)
    p1 = _gpu(p1, torch.int64, "p1").reshape(-1)
    p2 = _gpu(p2, torch.int64, "p2").reshape(-1)
    P = p1.shape[0]
    if p2.shape[0] != P or P == 0:
        raise ValueError("pair_scores: p1 and p2 must hold the same non-zero number of pairs")
    score = torch.empty(P, dtype=torch.float64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    if label is None:
        _C.call("fedfr_pair_scores_roc", feats.data_ptr(), T, D, lut.data_ptr(), lut.numel(), p1.data_ptr(), p2.data_ptr(), P,
                score.data_ptr(), None, None, 0, None, None, 0, status.data_ptr(), _C.stream(feats))
        _check_status(status, "pair_scores")
        return score
    lab = _gpu(label, torch.int64, "label").reshape(-1)
    if lab.shape[0] != P:
        raise ValueError("pair_scores: label must have one entry per pair")
    gen = torch.nonzero(lab == 1).reshape(-1)
    if gen.numel() == 0 or gen.numel() == P:
        raise ValueError("pair_scores: the ROC needs genuine (label 1) and impostor pairs")
    # the genuine scores first (the same kernel: the same numbers), then every pair scored and counted in one pass
    gsc = pair_scores(feats, unique_templates, p1[gen], p2[gen])
    gv = _sorted_genuine(gsc)
    G = len(gv)
    gv_d = torch.from_numpy(gv).to(dev)
    counts = torch.zeros(3 * G + 1, dtype=torch.int64, device=dev)
    ws = torch.empty(int(_C.lib().fedfr_roc_counts_workspace_bytes(P, G)), dtype=torch.uint8, device=dev)
    _C.call("fedfr_pair_scores_roc", feats.data_ptr(), T, D, lut.data_ptr(), lut.numel(), p1.data_ptr(), p2.data_ptr(), P,
            score.data_ptr(), lab.data_ptr(), gv_d.data_ptr(), G, counts.data_ptr(), ws.data_ptr(), ws.numel(), status.data_ptr(),
            _C.stream(feats))
    _check_status(status, "pair_scores")
    return score, gv, counts.cpu().numpy()


@torch.no_grad()
def roc_counts(label, score):
    """ROC counts of given scores at their distinct genuine values (GPU).  Returns (genuine values descending, counts [3G+1])."""
    sc = _gpu(score, torch.float64, "score").reshape(-1)
    lab = _gpu(label, torch.int64, "label").reshape(-1)
    P = sc.shape[0]
    if lab.shape[0] != P or P == 0:
        raise ValueError("roc_counts: label and score must have the same non-zero length")
    gv = _sorted_genuine(sc[lab == 1])
    G = len(gv)
    if G == 0 or int((lab == 1).sum()) == P:
        raise ValueError("roc_counts: the ROC needs genuine (label 1) and impostor pairs")
    dev = sc.device
    gv_d = torch.from_numpy(gv).to(dev)
    counts = torch.zeros(3 * G + 1, dtype=torch.int64, device=dev)
    ws = torch.empty(int(_C.lib().fedfr_roc_counts_workspace_bytes(P, G)), dtype=torch.uint8, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    _C.call("fedfr_roc_counts", sc.data_ptr(), lab.data_ptr(), P, gv_d.data_ptr(), G, counts.data_ptr(), ws.data_ptr(), ws.numel(),
            status.data_ptr(), _C.stream(sc))
    _check_status(status, "roc_counts")
    return gv, counts.cpu().numpy()


def verification(template_norm_feats=None, unique_templates=None, p1=None, p2=None):
    """Drop-in for ijbc_all.verification: the fp64 score of every pair, numpy array in input order."""
    return pair_scores(template_norm_feats, unique_templates, p1, p2).cpu().numpy()


verification2 = verification          # the reference's identical twin


# ---- TPR@FPR read-out --------------------------------------------------------------------------------------------------------------
def table_from_counts(gv, counts, x_labels: Sequence[float] = X_LABELS,
                      impostors_between: Callable[[float, float], np.ndarray] = None):
    """TPR at each x of ``roc_curve`` (drop_intermediate=True) + the reference's nearest-FPR pick (ijbc_all.py:578-585), from the
    counts at the distinct genuine scores ``gv`` (descending).

    sklearn keeps a point where the step into it differs from the step out of it.  Every genuine point and the last impostor point
    before it follow from the counts alone.  An impostor-only point inside a run between two genuine values is kept only where the
    multiplicity of the impostor scores changes, and it can only matter where it lies as close to x as the best point found without it:
    for those few runs ``impostors_between(lo, hi)`` (impostor scores s with lo < s < hi) gives the exact points."""
    gv = np.asarray(gv, dtype=np.float64)
    c = np.asarray(counts, dtype=np.int64)
    G = len(gv)
    btw, eqn, npos = c[:G + 1], c[G + 1:2 * G + 1], c[2 * G + 1:3 * G + 1]
    Pn, Nn = int(npos.sum()), int(btw.sum() + eqn.sum())
    if Pn == 0 or Nn == 0:
        raise ValueError("table_from_counts: needs genuine and impostor pairs")
    fps_g = np.cumsum(btw[:G]) + np.cumsum(eqn)                         # fps at genuine point i
    tps_g = np.cumsum(npos)
    fps_start = np.concatenate([[0], fps_g])                            # fps before run k (k = 0 .. G)
    tps_run = np.concatenate([[0], tps_g])                              # tps along run k
    # skeleton points (fps, tps, key); the key orders points as sklearn's index does (larger = later = smaller threshold):
    # (major + 1) << 32 | minor, major -1 for the prepended (0, 0), 2k for the end of run k, 2k + 1 for genuine point k
    def key(major, minor):
        return ((np.asarray(major, np.int64) + 1) << 32) | np.asarray(minor, np.int64)

    ends = np.nonzero(btw > 0)[0]                                       # the run's last impostor point: always kept
    kept_g = np.ones(G, dtype=bool)                                     # a genuine point: kept unless the steps in and out are equal
    if G > 1:
        kept_g[:-1] = (btw[1:G] > 0) | (eqn[:-1] != eqn[1:]) | (npos[:-1] != npos[1:])
    if btw[0] == 0:
        kept_g[0] = True                                                # the first point overall
    gk = np.nonzero(kept_g)[0]
    sk_fps = np.concatenate([[0], fps_start[ends] + btw[ends], fps_g[gk]]).astype(np.int64)
    sk_tps = np.concatenate([[0], tps_run[ends], tps_g[gk]]).astype(np.int64)
    sk_key = np.concatenate([key([-1], [0]), key(2 * ends, 0), key(2 * gk + 1, 0)])
    nf = np.float64(Nn)

    def pick(fps, tps, keys, x):
        d = np.abs(fps.astype(np.float64) / nf - x)                     # fpr = fps / fps[-1], then abs(fpr - x), as the reference
        dmin = d.min()
        tie = np.nonzero(d == dmin)[0]
        return dmin, tps[tie[np.argmax(keys[tie])]]                     # equal distance: the later point (smallest index after flipud)

    lo_f = (fps_start + 1).astype(np.float64) / nf                      # the span of run k's possible inner points
    hi_f = (fps_start + btw - 1).astype(np.float64) / nf
    out = []
    for x in x_labels:
        fps, tps, keys = [sk_fps], [sk_tps], [sk_key]
        d0, _ = pick(sk_fps, sk_tps, sk_key, x)
        for k in np.nonzero((btw >= 2) & ~(lo_f - x > d0) & ~(x - hi_f > d0))[0]:
            if impostors_between is None:
                raise ValueError("table_from_counts: impostor scores are needed to resolve run %d" % k)
            lo = gv[k] if k < G else -np.inf
            hi = gv[k - 1] if k > 0 else np.inf
            vals, cnt = np.unique(np.asarray(impostors_between(lo, hi), dtype=np.float64), return_counts=True)
            cnt = cnt[::-1]
            if int(cnt.sum()) != btw[k]:
                raise RuntimeError("table_from_counts: run %d holds %d impostors, the counts say %d" % (k, cnt.sum(), btw[k]))
            inner = np.nonzero(cnt[:-1] != cnt[1:])[0]                  # a change of step (the last point is in the skeleton)
            if k == 0 and len(cnt) > 1:
                inner = np.union1d(inner, [0])                          # the first point overall
            fps.append(fps_start[k] + np.cumsum(cnt)[inner])
            tps.append(np.full(len(inner), tps_run[k], np.int64))
            keys.append(key(np.full(len(inner), 2 * k - 1), inner + 1))
        _, t = pick(np.concatenate(fps), np.concatenate(tps), np.concatenate(keys), x)
        out.append(float(np.float64(t) / np.float64(Pn)))
    return out


def tpr_fpr_table(label, score, x_labels: Sequence[float] = X_LABELS):
    """TPR at FPR x for each x of ``x_labels``: equal to ``roc_curve(label, score)`` + the reference's nearest-FPR pick, without sorting
    the scores (counts on the GPU)."""
    sc = _gpu(score, torch.float64, "score").reshape(-1)
    lab = _gpu(label, torch.int64, "label").reshape(-1)
    gv, counts = roc_counts(lab, sc)
    return table_from_counts(gv, counts, x_labels, _impostor_fetch(sc, lab))


def _impostor_fetch(sc, lab):
    neg = lab != 1

    def fetch(lo, hi):
        return sc[neg & (sc > lo) & (sc < hi)].cpu().numpy()
    return fetch


def format_table(tprs):
    """The reference's row cells: '%.2f' % (tpr * 100)."""
    return ["%.2f" % (t * 100) for t in tprs]


# ---- the whole 1:1 job -----------------------------------------------------------------------------------------------------------
def ijbc_11(img_feats, templates, medias, p1, p2, label, faceness=None, use_norm_score: bool = True, use_detector_score: bool = True,
            use_flip_test: bool = False, x_labels: Sequence[float] = X_LABELS) -> Dict[str, object]:
    """Job 1:1 of ijbc_all.py after the embeddings (:509-586) with the reference's test-mode defaults (N1 and D1 on, F1 off).  Template
    features stay on the device.  Returns dict(score = fp64 scores on the GPU, tpr = TPR per x, table = the '%.2f' cells)."""
    if use_detector_score and faceness is None:
        raise ValueError("ijbc_11: use_detector_score needs the faceness scores")
    feats, uniq = template_pool(img_feats, templates, medias, faceness=faceness if use_detector_score else None, flip=use_flip_test,
                                norm_images=not use_norm_score, mode=0)
    score, gv, counts = pair_scores(feats, uniq, p1, p2, label)
    lab = _gpu(label, torch.int64, "label").reshape(-1)
    tprs = table_from_counts(gv, counts, x_labels, _impostor_fetch(score, lab))
    return {"score": score, "tpr": tprs, "table": format_table(tprs)}


# ---- job 1:N -------------------------------------------------------------------------------------------------------------------
def unique_template_ids(choose_templates, choose_ids):
    """ijbc_all.py:271-272: the sorted distinct template ids of a gallery / probe list and the subject id of each (its first listing)."""
    choose_templates = _host(choose_templates, np.int64).reshape(-1)
    choose_ids = _host(choose_ids).reshape(-1)
    if choose_templates.shape != choose_ids.shape:
        raise ValueError("unique_template_ids: choose_templates and choose_ids must have one entry per listed template")
    uniq, first = np.unique(choose_templates, return_index=True)
    return uniq, choose_ids[first]


def image2template_feature_1n(img_feats=None, templates=None, medias=None, choose_templates=None, choose_ids=None, on_gpu: bool = False,
                              **pool_args):
    """Drop-in for ijbc_all.image2template_feature_1n: (template_norm_feats [T, D] fp64, unique_templates, unique_subjectids) of the
    templates named in ``choose_templates``.  ``on_gpu=True`` leaves the features on the device (a torch tensor) instead of returning
    numpy; ``pool_args`` go to ``template_pool`` (faceness, flip, norm_images)."""
    uniq, ids = unique_template_ids(choose_templates, choose_ids)
    feats, _ = template_pool(img_feats, templates, medias, choose_templates=choose_templates, mode=1, **pool_args)
    return (feats if on_gpu else feats.cpu().numpy()), uniq, ids


def gen_mask(query_ids, reg_ids):
    """Drop-in for ijbc_all.gen_mask (vectorised; an int64 array instead of a list): the gallery row of every query id.  RuntimeError when
    a query id matches no gallery id or several."""
    q, r = _host(query_ids).reshape(-1), _host(reg_ids).reshape(-1)
    order = np.argsort(r, kind="stable")
    rs = r[order]
    lo = np.searchsorted(rs, q, side="left")
    cnt = np.searchsorted(rs, q, side="right") - lo
    bad = np.nonzero(cnt != 1)[0]
    if bad.size:
        raise RuntimeError("RegIdsError with id = {}, duplicate = {} ".format(q[bad[0]], cnt[bad[0]]))
    return order[lo].astype(np.int64)


@torch.no_grad()
def identification_rank_topk(query: torch.Tensor, gallery: torch.Tensor, mask: torch.Tensor, K: int):
    """fp64 scores <query[q], gallery[c]> of every pair, never stored.  ``query`` [Q, D] / ``gallery`` [G, D] fp64 and ``mask`` [Q] int64
    (the gallery row of the query's identity, or -1) on the GPU, 1 <= K <= MAX_K_1N.  Returns ``pos`` [Q] fp64 (NaN where mask is -1),
    ``neg_topk`` [K] fp64 (the K largest scores of the pairs c != mask[q], duplicates counted, descending, -inf past ``neg_count``),
    ``neg_count`` (0-dim int64), ``rank_gt`` / ``rank_eq`` [Q] int32: the number of columns c != mask[q] that score higher than / equal
    to pos[q] (-1 where mask is -1).  ValueError on a non-finite score (a NaN / inf feature)."""
    query = _C.require_gpu_tensor(query.contiguous(), torch.float64, "query")
    gallery = _C.require_gpu_tensor(gallery.contiguous(), torch.float64, "gallery")
    mask = _C.require_gpu_tensor(mask.contiguous(), torch.int64, "mask")
    if query.dim() != 2 or gallery.dim() != 2 or query.shape[1] != gallery.shape[1]:
        raise ValueError("identification_rank_topk: query [Q, D] and gallery [G, D] must share D (got %s, %s)"
                         % (tuple(query.shape), tuple(gallery.shape)))
    Q, D = query.shape
    G = gallery.shape[0]
    if tuple(mask.shape) != (Q,):
        raise ValueError("identification_rank_topk: mask must be [Q] (got %s for Q = %d)" % (tuple(mask.shape), Q))
    K = int(K)
    if not 1 <= K <= MAX_K_1N:
        raise ValueError("identification_rank_topk: K = %d outside [1, %d]" % (K, MAX_K_1N))
    dev = query.device
    pos = torch.empty(Q, dtype=torch.float64, device=dev)
    neg_topk = torch.empty(K, dtype=torch.float64, device=dev)
    neg_count = torch.empty((), dtype=torch.int64, device=dev)
    rank_gt = torch.empty(Q, dtype=torch.int32, device=dev)
    rank_eq = torch.empty(Q, dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    ws = torch.empty(int(_C.lib().fedfr_ident_rank_workspace_bytes(Q, G, K)), dtype=torch.uint8, device=dev)
    _C.call("fedfr_ident_rank_topk", query.data_ptr(), Q, gallery.data_ptr(), G, D, mask.data_ptr(), K, pos.data_ptr(),
            neg_topk.data_ptr(), neg_count.data_ptr(), rank_gt.data_ptr(), rank_eq.data_ptr(), ws.data_ptr(), ws.numel(),
            status.data_ptr(), _C.stream(query))
    s = int(status.item())
    if s & 2:
        raise ValueError("identification_rank_topk: mask entries must be -1 or a gallery row in [0, %d)" % G)
    if s & 1:
        raise ValueError("identification_rank_topk: scores must be finite (a feature is NaN or inf)")
    return pos, neg_topk, neg_count, rank_gt, rank_eq


def _evaluate_1n(query_feats, gallery_feats, mask, fars):
    query = _gpu(query_feats, torch.float64, "query_feats")
    gallery = _gpu(gallery_feats, torch.float64, "gallery_feats")
    if query.dim() != 2 or gallery.dim() != 2:
        raise ValueError("evaluation: query_feats [Q, D] and gallery_feats [G, D] expected")
    Q, G = query.shape[0], gallery.shape[0]
    m = _host(mask, np.int64).reshape(-1)
    if m.shape[0] != Q:
        raise ValueError("evaluation: mask has %d entries for %d queries" % (m.shape[0], Q))
    if np.any((m < -1) | (m >= G)):
        raise ValueError("evaluation: mask entries must be -1 or a gallery row in [0, %d)" % G)
    need = [math.ceil(Q * x) for x in fars]                     # :406, Q counts every query
    K = max(need)
    negatives = Q * G - int(np.sum(m >= 0))
    if K < 1 or negatives < K:
        raise ValueError("evaluation: %d negative pairs but the threshold at the largest FAR needs the %d-th largest (the reference "
                         "raises IndexError here)" % (negatives, K))
    if K > MAX_K_1N:
        raise ValueError("evaluation: ceil(Q * far) = %d exceeds the kernel's K limit %d" % (K, MAX_K_1N))
    pos, neg, _, rank_gt, rank_eq = identification_rank_topk(query, gallery, torch.from_numpy(m).to(query.device), K)
    pos, neg, rank_gt, rank_eq = pos.cpu().numpy(), neg.cpu().numpy(), rank_gt.cpu().numpy(), rank_eq.cpu().numpy()
    rank = {"top%d" % k: int(np.sum((rank_gt >= 0) & (rank_gt < k))) / Q for k in (1, 5, 10)}
    th = {far: float(neg[k - 1]) for far, k in zip(fars, need)}
    pr = {far: int(np.sum(pos > th[far])) / Q for far in fars}  # NaN (no positive) never counts
    return rank, pr, th, int(np.sum(rank_eq > 0))


def evaluation(query_feats, gallery_feats, mask, fars: Sequence[float] = FARS_1N, return_ties: bool = False):
    """Drop-in for ijbc_all.evaluation: query [Q, D], gallery [G, D] (numpy, or torch tensors on the GPU; used in fp64), ``mask`` [Q] =
    the gallery row of each query's identity (or -1: never a hit).  Returns (rank, pr): rank = {'top1', 'top5', 'top10'} (query i is a
    top-k hit iff fewer than k other gallery rows score strictly higher than its own), pr = {far: rate of own-row scores above the
    ceil(Q * far)-th largest negative}.  Where a query's own score ties another row's exactly, the reference's argsort order is
    unspecified; ``return_ties=True`` adds the number of such queries as a third value."""
    rank, pr, _, ties = _evaluate_1n(query_feats, gallery_feats, mask, tuple(fars))
    return (rank, pr, ties) if return_ties else (rank, pr)


def ijbc_1n(img_feats, templates, medias, gallery_templates, gallery_ids, probe_templates, probe_ids, faceness=None,
            use_norm_score: bool = True, use_detector_score: bool = True, use_flip_test: bool = False,
            fars: Sequence[float] = FARS_1N) -> Dict[str, object]:
    """Job 1:N of ijbc_all.py after the embeddings (:515-533, 592-627): gallery (G1 + G2 lists concatenated) and probe template
    features, gen_mask and evaluation, the features staying on the device.  Returns dict(rank, pr, th = {far: threshold}, ties = queries
    whose own score ties another row's, lines = what the reference appends to log.txt after the epoch line)."""
    if use_detector_score and faceness is None:
        raise ValueError("ijbc_1n: use_detector_score needs the faceness scores")
    pool = dict(faceness=faceness if use_detector_score else None, flip=use_flip_test, norm_images=not use_norm_score, on_gpu=True)
    feats = _gpu(img_feats, torch.float32, "img_feats")
    gallery, _, gids = image2template_feature_1n(feats, templates, medias, gallery_templates, gallery_ids, **pool)
    probe, _, pids = image2template_feature_1n(feats, templates, medias, probe_templates, probe_ids, **pool)
    rank, pr, th, ties = _evaluate_1n(probe, gallery, gen_mask(pids, gids), tuple(fars))
    lines = ["%s : %.5f" % (r, rank[r]) for r in rank] + ["far = %.4f  pr = %.5f" % (far, pr[far]) for far in pr]
    return {"rank": rank, "pr": pr, "th": th, "ties": ties, "lines": lines}


# ---- test oracle --------------------------------------------------------------------------------------------------------------
def reference_table(label, score, x_labels: Sequence[float] = X_LABELS) -> Tuple[list, list]:
    """sklearn roc_curve + the reference's pick, on the host (the test oracle; needs scikit-learn)."""
    from sklearn.metrics import roc_curve
    fpr, tpr, _ = roc_curve(np.asarray(label), np.asarray(score))
    fpr, tpr = np.flipud(fpr), np.flipud(tpr)
    out = []
    for x in x_labels:
        _, i = min(zip(abs(fpr - x), range(len(fpr))))
        out.append(float(tpr[i]))
    return out, format_table(out)
