"""``Evaluator`` with the interface of the reference's mvpnet/evaluate_3d.py:11-92, written without scikit-learn and with
a device path: ``update`` on tensors in HBM counts the confusion with the kernel of csrc/chunk.hip and only the [C,C]
counts reach the host. The reference module's command-line scorer (``main``) and its ScanNet name / id tables are not
part of this drop-in."""
import numpy as np
import torch

try:
    from .._native import ops
except ImportError:
    from _native import ops

IGNORE_LABEL = -100


def _slots_numpy(values, table):
    """Position of every value in `table` (-1 where it is not in it)."""
    by_value = np.argsort(table, kind="stable")
    ordered = table[by_value]
    at = np.clip(np.searchsorted(ordered, values), 0, table.shape[0] - 1)
    return np.where(ordered[at] == values, by_value[at], -1)


def _divide(num, den):
    """num / den in float64 with NumPy's 0/0 = nan and x/0 = inf, without the warnings."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.float64(num) / np.float64(den)


class Evaluator(object):
    """Accumulates a confusion matrix (rows = truth, columns = prediction, float64 on the host) over scenes and derives
    accuracy and IoU figures from it. `labels` are the raw values that make up the rows / columns, 0..C-1 by default;
    a pair whose truth or prediction is not among them is not counted."""

    def __init__(self, class_names, labels=None):
        self.class_names = tuple(class_names)
        self.num_classes = len(self.class_names)
        self.labels = np.array(range(self.num_classes) if labels is None else labels)
        if self.labels.shape[0] != self.num_classes:
            raise AssertionError("%d labels for %d class names" % (self.labels.shape[0], self.num_classes))
        self.confusion_matrix = np.zeros((self.num_classes, self.num_classes), dtype=np.float64)

    # ------------------------------------------------------------------------------------------------- accumulation

    def _identity_table(self):
        return np.array_equal(self.labels, np.arange(self.num_classes))

    def _slots_device(self, t):
        """Raw label values -> slots of self.labels on the device (-1 outside the table)."""
        if self._identity_table():
            return t
        size = int(self.labels.max()) + 1
        lut = torch.full((size,), -1, dtype=torch.int64)
        lut[torch.from_numpy(self.labels.astype(np.int64))] = torch.arange(self.num_classes)
        lut = lut.to(t.device)
        t = t.to(torch.int64)
        inside = (t >= 0) & (t < size)
        return torch.where(inside, lut[t.clamp(0, size - 1)], torch.full_like(t, -1))

    def update(self, pred_label, gt_label):
        """Add one scene: pred_label and gt_label hold one integer per point, as NumPy arrays or as tensors in HBM.

        NumPy arrays: as in the reference, a truth of -100 is rewritten to num_classes IN THE CALLER'S ARRAY before
        counting, and a scene whose truth is negative everywhere is skipped. Tensors are counted on the device and are
        NOT modified; the reference's rewrite is not reproduced there because it cannot change a count (a truth outside
        the label table is dropped either way), and all-negative truth adds nothing because no pair is counted."""
        if isinstance(pred_label, torch.Tensor) or isinstance(gt_label, torch.Tensor):
            device = pred_label.device if isinstance(pred_label, torch.Tensor) else gt_label.device
            pred = torch.as_tensor(pred_label).to(device).reshape(-1)
            truth = torch.as_tensor(gt_label).to(device).reshape(-1)
            counts = ops.chunk_confusion(self._slots_device(pred), self._slots_device(truth), self.num_classes)
            self.confusion_matrix += counts.cpu().numpy()
            return
        if not (gt_label >= 0).any():
            return
        gt_label[gt_label == IGNORE_LABEL] = self.num_classes
        row = _slots_numpy(np.ravel(gt_label), self.labels)
        col = _slots_numpy(np.ravel(pred_label), self.labels)
        counted = (row >= 0) & (col >= 0)
        flat = np.bincount(row[counted] * self.num_classes + col[counted], minlength=self.num_classes ** 2)
        self.confusion_matrix += flat.reshape(self.num_classes, self.num_classes)

    def batch_update(self, pred_labels, gt_labels):
        if len(pred_labels) != len(gt_labels):
            raise AssertionError("%d predictions for %d truths" % (len(pred_labels), len(gt_labels)))
        for pair in zip(pred_labels, gt_labels):
            self.update(*pair)

    # ------------------------------------------------------------------------------------------------------ figures

    @property
    def overall_acc(self):
        return _divide(np.trace(self.confusion_matrix), self.confusion_matrix.sum())

    @property
    def class_seg_acc(self):
        """Per class: correct / points of that truth (nan for a class without truth), a list of num_classes values."""
        hits, truth = np.diag(self.confusion_matrix), self.confusion_matrix.sum(axis=1)
        return [_divide(h, t) for h, t in zip(hits, truth)]

    @property
    def class_iou(self):
        """Per class: intersection / union of truth and prediction, nan where the union is empty."""
        m = self.confusion_matrix
        hits = np.diag(m)
        union = m.sum(axis=0) + m.sum(axis=1) - hits
        return [float("nan") if u == 0 else h / u for h, u in zip(hits, union)]

    @property
    def overall_iou(self):
        return np.nanmean(np.asarray(self.class_iou, np.float64))      # classes with an empty union do not count

    # ------------------------------------------------------------------------------------------------------- tables

    def print_table(self):
        """One row per class: name, accuracy and IoU in per cent, number of truth points (the reference's layout)."""
        from tabulate import tabulate
        acc, iou, totals = self.class_seg_acc, self.class_iou, self.confusion_matrix.sum(axis=1)
        rows = [[name, 100 * acc[c], 100 * iou[c], int(totals[c])] for c, name in enumerate(self.class_names)]
        return tabulate(rows, headers=['Class', 'Accuracy', 'IOU', 'Total'], tablefmt='psql', floatfmt='.2f')

    def save_table(self, filename):
        """One tab-separated row, no alignment: overall accuracy, overall IoU, then every class's IoU."""
        from tabulate import tabulate
        columns = ('overall acc', 'overall iou') + self.class_names
        row = [self.overall_acc, self.overall_iou] + self.class_iou
        text = tabulate([row], headers=columns, tablefmt='tsv', floatfmt='.5f', numalign=None, stralign=None)
        with open(filename, 'w') as f:
            f.write(text)
