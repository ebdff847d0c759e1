"""Local 1:1 verification of a client's own identities (reference eval_local.py ``CallBack_LocalVerifi``, the ``--task 1:1`` branch of
local_all.py:303-335, :433-453, and roc_cuda.py behind both).  Names, signatures and log lines are the reference's; the bodies are written
from its behaviour.  Where the reference saves the features to ``.npy`` and shells out to ``roc_cuda.py`` once per client, this module
keeps them on the GPU and makes ONE ``eval_roc.roc_histogram_groups`` call (``fedfr_roc_histogram_groups``: the pair histograms of all
clients in one pass over the unordered pairs), then reads every histogram out as ``plot_ROC`` does (``eval_roc.tpr_at_fpr``).

Not reproduced: the MXNet RecordIO reader (``MXFaceDataset`` over ``test.rec`` / ``test.idx``).  The callback takes the test set as
``loader=`` instead: any iterable of image batches, or of ``(images, labels)`` batches, in the forms ``client.to_device_batch`` accepts."""
from __future__ import annotations

import os
import threading
from collections import defaultdict
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import eval_roc, ops
from .client import to_device_batch

FPR_EXPONENTS = tuple(range(-1, -7, -1))       # the columns of every TPR row: FPR = 1e-1 ... 1e-6 (roc_cuda.py:71)


def _device_of(backbone, device):
    if device is not None:
        return torch.device(device)
    if hasattr(backbone, "parameters"):
        for p in backbone.parameters():
            if p.is_cuda:
                return p.device
    return torch.device("cuda", torch.cuda.current_device())


@torch.no_grad()
def generate_features(backbone, loader, flip_test=False, device=None):
    """Eval-mode embeddings of every batch of ``loader`` (eval_local.py:107-152): with ``flip_test`` the embedding of the horizontally
    mirrored batch is added (:137-145), then every row is normalised (sklearn ``normalize``).  Returns ``([N, 512] fp32 on the GPU,
    int64 labels on the GPU or None when the loader yields images only)``.  ``backbone`` is any module or callable, e.g.
    ``nn.Sequential(backbone, bce_module.converter)``; the train / eval flags of its modules are put back on exit.

    The reference mirrors with ``torch.fliplr``, which on an NCHW batch reverses the CHANNEL axis; what its name and its use say is the
    horizontal mirror image of ``eval/verification.py``, and that is what is added here."""
    dev = _device_of(backbone, device)
    modes = [(m, m.training) for m in backbone.modules()] if isinstance(backbone, torch.nn.Module) else []
    for m, _ in modes:                          # the flags themselves: IResNet.train() / eval() would also drop a BatchNorm freeze
        m.training = False
    feats, labels = [], []
    try:
        with torch.cuda.device(dev):
            for batch in loader:
                img, lab = (batch[0], batch[1]) if isinstance(batch, (tuple, list)) else (batch, None)
                img, lab_dev = to_device_batch(img, lab if lab is not None else torch.zeros(len(img), dtype=torch.int64), dev, train=False)
                f = backbone(img)
                if flip_test:
                    f = ops.axpy_(f.contiguous(), backbone(torch.flip(img, dims=[3]).contiguous()).contiguous(), 1.0)
                feats.append(ops.normalize_rows(f.contiguous())[0])
                if lab is not None:
                    labels.append(lab_dev)
    finally:
        for m, t in modes:
            m.training = t
    if not feats:
        raise ValueError("generate_features: the loader yielded no batch")
    return torch.cat(feats, dim=0), (torch.cat(labels, dim=0).to(torch.int64) if labels else None)


def _check_group(hist, what):
    if int(hist[:, 0].sum()) == 0 or int(hist[:, 1].sum()) == 0:
        raise ValueError("%s has no %s pair: its TPR / FPR is undefined (the reference divides by zero here)"
                         % (what, "same-label" if int(hist[:, 0].sum()) == 0 else "different-label"))


def local_11_from_histograms(hists, num_client, num_ids=4000, epoch=0, output_dir=None) -> Tuple[List[List[float]], np.ndarray]:
    """The host half of ``local_11``: ``hists`` [num_client, 2001, 2] pair histograms -> (per-client TPR rows, their mean), printed and
    logged as local_all.py:305-335 and roc_cuda.py:72-87 do."""
    hists = np.asarray(hists.cpu() if torch.is_tensor(hists) else hists, dtype=np.int64)
    per = num_ids // num_client
    for c in range(num_client):
        _check_group(hists[c], "local_11: group %d (identities %d to %d)" % (c, c * per, (c + 1) * per - 1))
    rows = [eval_roc.tpr_at_fpr(hists[c]) for c in range(num_client)]
    mean = np.mean(np.array(rows), axis=0)
    lines = ['1:1 at Epoch : %d\n' % epoch]
    for c, row in enumerate(rows):
        head = 'Target label from %d to %d' % (c * per, (c + 1) * per - 1)
        body = 'Epoch %d, TPR (-1 to -6) = %r' % (epoch, row)
        print('-' * 80 + '\n' + head + '\n' + body + '\n' + '-' * 80)
        lines += [head + '\n', body + '\n']
    lines += ['Mean (-6 to -1):\n', '[' + ''.join('%.2f ' % mean[len(mean) - 1 - i] for i in range(len(mean))) + ']\n']
    print('-' * 40)
    print('1:1 average results (-6 to -1):')
    print('%r' % ['%.2f' % mean[len(mean) - 1 - i] for i in range(len(mean))])
    if output_dir is not None:
        os.makedirs(output_dir, exist_ok=True)
        with open(os.path.join(output_dir, 'local_log.txt'), 'a') as f:
            f.writelines(lines)
    return rows, mean


def _on_gpu(x, dtype, device=None):
    t = torch.as_tensor(x)
    if not t.is_cuda:
        t = t.to(device if device is not None else torch.device("cuda", torch.cuda.current_device()))
    return t.to(dtype).contiguous()


@torch.no_grad()
def local_11(img_feats, labels, num_client, num_ids=4000, epoch=0, output_dir=None) -> Tuple[List[List[float]], np.ndarray]:
    """local_all.py:303-335, :433-453 for one feature set: client c owns the identities [c * (num_ids // num_client),
    (c + 1) * (num_ids // num_client)); its row is the TPR (%) at FPR 1e-1 ... 1e-6 over every pair with at least one image of its
    identities.  One grouped histogram call for all clients, one ``tpr_at_fpr`` read-out each.  Returns (rows, mean); with
    ``output_dir`` the reference's lines are appended to ``<output_dir>/local_log.txt``.  The mean is over this call's rows (the
    reference re-reads every ``Epoch <epoch>, TPR`` line of the log, earlier runs of the same epoch included).  A group without a
    same-label pair or without a different-label pair raises ValueError."""
    feats = _on_gpu(img_feats, torch.float32)
    lab = _on_gpu(labels, torch.int64, feats.device).reshape(-1)
    per = num_ids // num_client
    if num_client < 1 or per < 1:
        raise ValueError("local_11: num_client = %d, num_ids = %d leave no identity per client" % (num_client, num_ids))
    with torch.cuda.device(feats.device):
        group = torch.where((lab >= 0) & (lab < per * num_client), torch.div(lab, per, rounding_mode="floor"), torch.full_like(lab, -1))
        hists = eval_roc.roc_histogram_groups(feats, lab, group, num_client)
    return local_11_from_histograms(hists, num_client, num_ids, epoch, output_dir)


class CallBack_LocalVerifi(object):
    """reference eval_local.py:74-152, handed by the server to its "local candidate" clients, which call ``veri_test`` before the first
    and after the last local epoch.  ``loader`` replaces the reference's RecordIO reader (see the module docstring); ``labels`` [N] are
    the identities of the test images in loader order — by default the second column of ``<data_dir>/idx_id_pair.txt`` (:119-121;
    its first line is the header row ``pandas.read_csv`` makes of it), or what the loader yields.  Results go to ``client_record[client_ID]``
    as ``(global_step, [TPR at FPR 1e-1 ... 1e-6])`` and, in ``plot_ROC``'s two lines, to ``<output_dir>/clients/client_<id>/local_log.txt``.
    No ``.npy`` round trip, no subprocess; ``workers`` and ``batch_size`` (roc_cuda.py's process pool) are kept for the signature only."""

    def __init__(self, frequent, rank, data_dir, th=-1, flip_test=False, output_dir=None, verbose=True, workers=2, batch_size=800,
                 loader=None, labels=None):
        if loader is None:
            raise NotImplementedError("fedfr_amd: CallBack_LocalVerifi needs loader= (an iterable of image batches of the local test set, "
                                      "in identity order): the reference's MXNet RecordIO reader of %s/test.rec is out of scope" % (data_dir,))
        self.frequent, self.rank, self.data_dir, self.th, self.flip_test = frequent, rank, data_dir, th, flip_test
        self.output_dir, self.verbose, self.workers, self.batch_size = output_dir, verbose, workers, batch_size
        self.client_record = defaultdict(list)
        self.loader = loader
        if labels is None and data_dir is not None and os.path.exists(os.path.join(data_dir, 'idx_id_pair.txt')):
            labels = np.loadtxt(os.path.join(data_dir, 'idx_id_pair.txt'), dtype=np.int64, skiprows=1, ndmin=2)[:, 1]
            if verbose:
                print('load idx_id_pair', (len(labels), 2))
        self.labels = None if labels is None else torch.as_tensor(np.asarray(labels)).to(torch.int64).reshape(-1)
        self._lock = threading.Lock()           # Server.train may run clients on threads: one evaluation at a time

    def generate_features(self, backbone):
        return generate_features(backbone, self.loader, self.flip_test)

    def veri_test(self, backbone_orign, global_step, ID_list, client_ID):
        if not (self.rank == 0 and global_step >= self.th and global_step % self.frequent == 0):
            return
        with self._lock:
            img_feats, labels = self.generate_features(backbone_orign)
            if self.labels is not None:
                labels = self.labels.to(img_feats.device)
            if labels is None or labels.shape[0] != img_feats.shape[0]:
                raise ValueError("CallBack_LocalVerifi: %d test images but %s labels (labels=, idx_id_pair.txt or a loader of (images, labels))"
                                 % (img_feats.shape[0], "no" if labels is None else labels.shape[0]))
            first, last = int(ID_list[0]), int(ID_list[-1])                 # roc_cuda.py --ID_s_e first last+1: a range of identities
            with torch.cuda.device(img_feats.device):
                group = ((labels >= first) & (labels <= last)).to(torch.int64) - 1
                hist = eval_roc.roc_histogram_groups(img_feats, labels, group, 1)[0].cpu().numpy()
            _check_group(hist, "CallBack_LocalVerifi: client %d (identities %d to %d)" % (client_ID, first, last))
            result = eval_roc.tpr_at_fpr(hist)
            head = 'Target label from %d to %d' % (first, last)
            body = 'Epoch %d, TPR (-1 to -6) = %r' % (global_step, result)
            if self.verbose:
                print('Total pair :', int(hist.sum()))
                print('-' * 80 + '\n' + head + '\n' + body + '\n' + '-' * 80)
            if self.output_dir is not None:
                client_dir = os.path.join(self.output_dir, 'clients', 'client_%d' % (client_ID))
                os.makedirs(client_dir, exist_ok=True)
                with open(os.path.join(client_dir, 'local_log.txt'), 'a') as f:
                    f.write(head + '\n' + body + '\n')
            self.client_record[client_ID].append((global_step, result))
