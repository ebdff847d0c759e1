"""Round callbacks of the server (reference utils/utils_callbacks.py): verification on the small 1:1 sets and the backbone checkpoint.
Class names, constructor arguments, public attributes and log lines are the reference's; the bodies are written from its behaviour."""
from __future__ import annotations

import logging
import os
from collections import OrderedDict

import torch

from . import eval_verification as verification

logger = logging.getLogger('FL_face.callback')

BATCH_SIZE, NFOLDS = 128, 10            # what the reference's callback hands to verification.test
STEP_BASED_START = 400                  # first update that is evaluated when the callback counts steps instead of epochs


def _fresh_records(n_sets):
    """One ``[step of the best accuracy, best accuracy]`` record per verification set, nothing seen yet."""
    return [[0, 0.0] for _ in range(n_sets)]


class CallBackVerification(object):
    """Runs ``verification.test`` (batch 128, 10 folds) on every loaded set and logs XNorm / Accuracy-Flip / Accuracy-Highest.  The
    best result per set is kept as ``[step, accuracy]`` in ``highest_acc_list`` (global model) or ``client_list[client]`` (a client's
    model).  Only rank 0 loads and evaluates.  The sets are ``load_bin``'s compact uint8 tensors, resident on the GPU; a target without
    a ``<name>.bin`` under ``rec_prefix`` is passed over, so records are indexed by position in ``ver_name_list``."""

    def __init__(self, frequent, rank, val_targets, rec_prefix, num_client=10, image_size=(112, 112), epoch_based=True):
        self.frequent, self.rank, self.num_client, self.epoch_based = frequent, rank, num_client, epoch_based
        self.client_list = {c: _fresh_records(len(val_targets)) for c in range(num_client)}
        self.highest_acc_list = _fresh_records(len(val_targets))
        self.ver_list, self.ver_name_list = [], []
        if rank == 0:
            self.init_dataset(val_targets=val_targets, data_dir=rec_prefix, image_size=image_size)

    def init_dataset(self, val_targets, data_dir, image_size):
        for name in val_targets:
            path = os.path.join(data_dir, name + ".bin")
            if not os.path.exists(path):
                continue
            self.ver_list.append(verification.load_bin(path, image_size))
            self.ver_name_list.append(name)

    def _report(self, records, prefix, i, step, acc, std, xnorm):
        """The three log lines of one set; ``records[i]`` moves to this step when the accuracy beats the best so far."""
        name = self.ver_name_list[i]
        logger.info('%s[%s][%d]XNorm: %f' % (prefix, name, step, xnorm))
        logger.info('%s[%s][%d]Accuracy-Flip: %1.5f+-%1.5f' % (prefix, name, step, acc, std))
        if acc > records[i][1]:
            records[i] = [step, acc]
        logger.info('%s[%s][%d]Accuracy-Highest: %1.5f' % (prefix, name, records[i][0], records[i][1]))

    def ver_test(self, backbone: torch.nn.Module, global_step: int, client=None):
        records = self.highest_acc_list if client is None else self.client_list[client]
        prefix = '' if client is None else 'Client %d :' % client
        for i, data_set in enumerate(self.ver_list):
            _, _, acc2, std2, xnorm, _ = verification.test(data_set, backbone, BATCH_SIZE, NFOLDS)
            self._report(records, prefix, i, global_step, acc2, std2, xnorm)

    def __call__(self, num_update, backbone: torch.nn.Module, client=None, th=3):
        first = th if self.epoch_based else STEP_BASED_START
        if self.rank != 0 or num_update < first or num_update % self.frequent:
            return
        backbone.eval()
        self.ver_test(backbone, num_update, client)
        backbone.train()                # as the reference: the caller gets its model back in training mode


def portable_state_dict(module):
    """``module.state_dict()`` as independent contiguous CPU tensors under the same keys: what ``torch.save`` should write (the backbone's
    entries are views of one flat device tensor, which would otherwise be pickled as a whole, device included)."""
    return OrderedDict((k, v.detach().cpu().contiguous().clone()) for k, v in module.state_dict().items())


class CallBackModelCheckpoint(object):
    """``backbone.pth`` under ``output``: the state_dict of the backbone (unwrapped when it is a DataParallel-style wrapper with a
    ``module`` attribute) in ``torch.save`` form, written by rank 0 from step 1 on; a PartialFC handed in saves its own parameters."""

    def __init__(self, rank, output="./"):
        self.rank, self.output = rank, output

    def __call__(self, global_step, backbone: torch.nn.Module, partial_fc=None):
        if global_step <= 0:
            return
        if self.rank == 0:
            torch.save(portable_state_dict(getattr(backbone, "module", backbone)), os.path.join(self.output, "backbone.pth"))
        if partial_fc is not None:
            partial_fc.save_params()
