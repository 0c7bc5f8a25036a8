"""``SegLoss`` with the reference's constructor and dictionary interface (mvpnet/models/loss.py:5-21: the class-weighted
cross entropy of preds['seg_logit'] (B, C, *) against labels['seg_label'] (B, *), mean over the points whose label is not
ignore_index) on the fused HIP kernel (csrc/loss.hip, seg_fwd_k): one launch reads the logits once and leaves the loss,
the per-point log-sum-exp for the backward, the hit count and the confusion counts in HBM.

The counts are left on the logits tensor as ``seg_logit._mvk_seg_stats`` so that SegAccuracy / SegIoU (metric.py) of the
same step take them instead of reading the logits again. Differences from the reference: a label outside [0, C) that is
not ignore_index does not stop the device; it is left out and reported by ``ops.seg_check_labels()``."""
from torch import nn

try:
    from ..._native import ops
except ImportError:
    from _native import ops


def leave_stats(seg_logit, seg_label, ignore_index, counts, conf):
    """The record metric.py looks for: which labels (tensor and version) and which ignore_index the counts belong to."""
    seg_logit._mvk_seg_stats = {'label': seg_label, 'label_version': seg_label._version,
                                'logit_version': seg_logit._version, 'ignore_index': int(ignore_index),
                                'counts': counts, 'conf': conf}


def stats_of(seg_logit, seg_label, ignore_index):
    """(counts int64 [2], conf int64 [C, C]) in HBM for these logits and labels: the record left on the logits when it is
    of this label tensor, unmodified since, and of this ignore_index; otherwise one metrics-only launch, whose result is
    left for the next metric."""
    st = getattr(seg_logit, '_mvk_seg_stats', None)
    if st is not None and st['label'] is seg_label and st['label_version'] == seg_label._version \
            and st['logit_version'] == seg_logit._version and st['ignore_index'] == int(ignore_index) \
            and st['conf'].shape[0] == seg_logit.shape[1]:
        return st['counts'], st['conf']
    counts, conf = ops.seg_stats(seg_logit, seg_label, ignore_index=ignore_index)
    leave_stats(seg_logit, seg_label, ignore_index, counts, conf)
    return counts, conf


class SegLoss(nn.Module):
    """Segmentation loss: {'seg_loss': scalar} from preds['seg_logit'] and labels['seg_label']."""

    def __init__(self, weight=None, ignore_index=-100):
        super(SegLoss, self).__init__()
        self.weight = weight
        self.ignore_index = ignore_index

    def forward(self, preds, labels):
        seg_logit = preds['seg_logit']
        seg_label = labels['seg_label']
        seg_loss, (counts, conf) = ops.seg_loss(seg_logit, seg_label, weight=self.weight, ignore_index=self.ignore_index,
                                                with_stats=True)
        leave_stats(seg_logit, seg_label, self.ignore_index, counts, conf)
        return {'seg_loss': seg_loss}
