"""The small detector of ``tests/_small.py`` with a FocalLoss as its objectness loss, and one loss
evaluation of it that also hands back the logits, targets and weights the loss saw."""
import copy

import torch

from tests import _small


def head_model(reduction='sum', loss_weight=5.0):
    from nesie_amd.votenet import build_nesie_votenet
    cfg = copy.deepcopy(_small.small_cfg())
    cfg['bbox_head']['objectness_loss'] = dict(type='FocalLoss', reduction=reduction,
                                               loss_weight=loss_weight)
    torch.manual_seed(0)
    model = build_nesie_votenet(cfg)
    # an untrained head puts no proposal within the shipped 0.3 of a box centre: widen, so that the
    # objectness term has positives and negatives
    model.train_cfg['pos_distance_thr'], model.train_cfg['neg_distance_thr'] = 1.0, 1.5
    model.bbox_head.train_cfg = model.train_cfg
    return model


def head_run(model, pts, boxes, labels):
    """-> (losses, obj_scores (B*K, 2) detached, objectness targets (B*K,), objectness weights
    (B*K,)) of that very run."""
    from nesie_amd.votenet.nesie_head import GTBatch
    gt = GTBatch.collate(boxes, labels, pts.device)
    head = model.bbox_head
    preds = head(model.extract_feat(pts), 'vote')
    targets = head.get_targets(pts, gt, None, None, None, preds)
    losses = head.loss(preds, pts, gt, None)
    return (losses, preds['obj_scores'].detach().reshape(-1, 2), targets[6].reshape(-1),
            targets[7].reshape(-1))
