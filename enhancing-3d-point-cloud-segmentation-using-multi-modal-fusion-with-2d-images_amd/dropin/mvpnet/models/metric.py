"""``SegAccuracy`` and ``SegIoU`` with the reference's interfaces (mvpnet/models/metric.py:5-73; the meter's face is that
of common/utils/metric_logger.py:11-51) over the counts of the fused HIP kernel (csrc/loss.hip, seg_fwd_k).

The reference takes argmax(1) of the logits in each metric, indexes with the ignore mask (a device-to-host read for the
size), calls ``.item()`` on the hit count and ``bincount`` on the pairs. Here ``update_dict`` takes the hit count, the kept
count and the confusion counts that SegLoss left on the logits (loss.py) -- or asks for them with one metrics-only
launch -- and adds them to accumulators in HBM. Nothing waits for the device until a value is read (``avg``,
``global_avg``, ``sum``, ``count``, ``values``, ``counts``, ``str``).

The meter lives in this file: ``common.utils`` stays the reference's own package."""
from collections import deque

import numpy as np
import torch

from .loss import stats_of


class _Meter(object):
    """The reference's AverageMeter (a window of the last `window_size` (value, count) pairs and the sums of all of them),
    whose entries may also be pairs that are still in HBM: int64 [2] tensors (value, count)."""
    default_fmt = '{avg:.4f} ({global_avg:.4f})'
    default_summary_fmt = '{global_avg:.4f}'

    def __init__(self, window_size=20, fmt=None, summary_fmt=None):
        self._window = deque(maxlen=window_size)     # (value, count) host pairs or int64 [2] device tensors
        self._host_sum = 0.0
        self._host_count = 0
        self._dev_total = None                       # int64 [2] in HBM: the sum of every device pair
        self.fmt = fmt or self.default_fmt
        self.summary_fmt = summary_fmt or self.default_summary_fmt

    def update(self, value, count=1):
        self._window.append((value, count))
        self._host_sum += value
        self._host_count += count

    def _update_device(self, pair):
        """pair: int64 [2] (value, count) in HBM; it is kept, not copied, so the caller must not change it afterwards."""
        self._window.append(pair)
        if self._dev_total is None:
            self._dev_total = pair.clone()
        else:
            self._dev_total += pair

    def _read(self):
        """One device-to-host copy for everything that is still in HBM: (total pair, window pairs as host numbers)."""
        dev = [e for e in self._window if isinstance(e, torch.Tensor)]
        if self._dev_total is None:
            total, host = (0, 0), []
        else:
            rows = torch.stack([self._dev_total] + dev).tolist()
            total, host = rows[0], rows[1:]
        it = iter(host)
        window = [tuple(next(it)) if isinstance(e, torch.Tensor) else e for e in self._window]
        return total, window

    @property
    def values(self):
        return deque((v for v, _ in self._read()[1]), maxlen=self._window.maxlen)

    @property
    def counts(self):
        return deque((c for _, c in self._read()[1]), maxlen=self._window.maxlen)

    @property
    def sum(self):
        return self._host_sum + self._read()[0][0]

    @property
    def count(self):
        return self._host_count + self._read()[0][1]

    @staticmethod
    def _ratio(window):
        with np.errstate(invalid='ignore', divide='ignore'):      # an empty window is 0 / 0 = nan, as with the reference
            return np.float64(np.sum([v for v, _ in window])) / np.float64(np.sum([c for _, c in window]))

    @property
    def avg(self):
        return self._ratio(self._read()[1])

    @property
    def global_avg(self):
        total, _ = self._read()
        count = self._host_count + total[1]
        return (self._host_sum + total[0]) / count if count != 0 else float('nan')

    def reset(self):
        self._window.clear()
        self._host_sum = 0.0
        self._host_count = 0
        self._dev_total = None

    def __str__(self):
        total, window = self._read()
        count = self._host_count + total[1]
        return self.fmt.format(avg=self._ratio(window),
                               global_avg=(self._host_sum + total[0]) / count if count != 0 else float('nan'))

    @property
    def summary_str(self):
        return self.summary_fmt.format(global_avg=self.global_avg)


def _operands(preds, labels):
    return preds['seg_logit'], labels['seg_label']


class SegAccuracy(_Meter):
    """Segmentation accuracy: the share of the points whose label is not ignore_index that are predicted right."""
    name = 'seg_acc'

    def __init__(self, ignore_index=-100):
        super(SegAccuracy, self).__init__()
        self.ignore_index = ignore_index

    def update_dict(self, preds, labels):
        seg_logit, seg_label = _operands(preds, labels)
        counts, _ = stats_of(seg_logit, seg_label, self.ignore_index)
        self._update_device(counts)


class SegIoU(object):
    """Segmentation IoU from the accumulated confusion counts ``mat`` (int64 [n, n] in HBM, rows = label, columns =
    prediction; None until the first update)."""
    name = 'seg_iou'

    def __init__(self, num_classes, ignore_index=-100):
        self.num_classes = num_classes
        self.ignore_index = ignore_index
        self.mat = None

    def update_dict(self, preds, labels):
        seg_logit, seg_label = _operands(preds, labels)
        if seg_logit.shape[1] != self.num_classes:
            raise ValueError('SegIoU: num_classes is {} but seg_logit has {} channels'.format(
                self.num_classes, seg_logit.shape[1]))
        _, conf = stats_of(seg_logit, seg_label, self.ignore_index)
        if self.mat is None:
            self.mat = conf.clone()
        else:
            self.mat += conf

    def reset(self):
        self.mat = None

    @property
    def iou(self):
        h = self.mat.float()
        diag = torch.diag(h)
        return diag / (h.sum(1) + h.sum(0) - diag)

    @property
    def global_avg(self):
        return self.iou.mean().item()

    def __str__(self):
        return '{iou:.4f}'.format(iou=self.iou.mean().item())

    @property
    def summary_str(self):
        return str(self)
