"""Evaluation + checkpoints of a classifier while it is fine-tuned (reference utils/train_classif.py:10-25)."""
import os

import torch
import torch.distributed as dist

from model.nn_utils import set_net_train
from .general import is_main_process, log

__all__ = ['test_print_classif']


def _unique_str(P):
    """Name stem of a run's files: the time the parameters were created (reference utils/general.py:109-110), taken on first use here."""
    from datetime import datetime
    if getattr(P, 'uuid', None) is None:
        P.uuid = datetime.now()
    return P.uuid.strftime('%Y%m%d-%H%M%S-%f')


def test_print_classif(train_type, P, net, testset_tuple, test_net, best_score=0, epoch=0):
    """Classification accuracy on (test_set, test_train_set) with the reference's two log lines; with P.save_dir set the weights go to
    `<unique>_best_classif.pth.tar` on a new best test score and to `model_classif_<epoch>.pth.tar` at every evaluation.  Under data
    parallel every rank evaluates (same weights, same control flow), rank 0 alone writes.  The reference's `<unique>.params` snapshot of P is
    not written.  Returns the best score."""
    test_set, test_train_set = testset_tuple
    save_dir = getattr(P, 'save_dir', None)
    main = is_main_process()
    set_net_train(net, False)
    c, t = test_net(net, test_set)
    if c > best_score:
        best_score = c
        if save_dir and main:
            torch.save(net.state_dict(), os.path.join(save_dir, _unique_str(P) + '_best_classif.pth.tar'))
    log(P, 'TEST - correct: {0} / {1} - acc: {2}'.format(c, t, float(c) / max(t, 1)))
    c, t = test_net(net, test_train_set)
    if save_dir and main:
        torch.save(net.state_dict(), os.path.join(save_dir, 'model_classif_' + str(epoch) + '.pth.tar'))
    if save_dir and dist.is_available() and dist.is_initialized():
        dist.barrier()                      # nobody races ahead of (or reads) a half-written checkpoint
    log(P, 'TRAIN - correct: {0} / {1} - acc: {2}'.format(c, t, float(c) / max(t, 1)))
    set_net_train(net, True, bn_train=P.train_bn)
    return best_score
