"""NumPy restatements of the reference's test-time voting (KPConv-PyTorch/utils/tester.py:160-186, :223-236, :273-297;
utils/trainer.py:351-378, :395-433), written for the tests of csrc/vote.hip. Nothing here reads the reference tree and
nothing needs sklearn.

Arithmetic of the vote, as the library's header states it: probabilities are float32 values, the accumulator is
float64, and one update is  smooth * old + (1 - smooth) * float64(p)  -- two float64 products and one sum, each rounded.
"""
import numpy as np


def softmax(x, dtype):
    """Row softmax evaluated entirely in `dtype`."""
    x = np.asarray(x, dtype)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return (e / e.sum(axis=1, keepdims=True)).astype(dtype)


def vote_batch(votes, probs, lengths, input_inds, cloud_inds, smooth=0.95, points=None, r2_max=None):
    """One batch (tester.py:170-186). votes: list of float64 [n_cloud, C] arrays, updated in place, sphere after sphere
    in batch order. probs [N, C]: float32 in the reference (any dtype here: it is widened to float64, which is exact
    for float32). points [N, 3] float32 + r2_max: only rows with (x*x + y*y) + z*z < r2_max in float32 vote.
    Returns the list of (cloud, rows that were written) per sphere."""
    one_minus = 1 - smooth
    written, i0 = [], 0
    for b, length in enumerate(lengths):
        length = int(length)
        p = np.asarray(probs[i0:i0 + length])
        inds = np.asarray(input_inds[i0:i0 + length]).astype(np.int64)
        c = int(cloud_inds[b])
        if points is not None and r2_max is not None and r2_max > 0:
            q = np.asarray(points[i0:i0 + length], np.float32)
            d2 = (q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]
            assert d2.dtype == np.float32
            mask = d2 < np.float32(r2_max)
            inds, p = inds[mask], p[mask]
        kept = smooth * votes[c][inds]
        added = one_minus * p.astype(np.float64)
        votes[c][inds] = kept + added
        written.append((c, inds))
        i0 += length
    return written


def column_map(label_values, ignored_labels):
    """For each slot of the full label table: the model's column, or -1 for an ignored label."""
    out, col = [], 0
    for v in label_values:
        if v in ignored_labels:
            out.append(-1)
        else:
            out.append(col)
            col += 1
    return np.asarray(out, np.int32)


def widen(probs, label_values, ignored_labels):
    """np.insert of a zero column at every ignored label's slot (tester.py:224-226), written as a scatter."""
    cm = column_map(label_values, ignored_labels)
    probs = np.asarray(probs)
    wide = np.zeros((probs.shape[0], len(cm)), probs.dtype)
    wide[:, cm >= 0] = probs
    return wide


def predict(probs, label_values, ignored_labels, proj=None):
    """Raw-label predictions (tester.py:229, :273, :292): first maximum over the widened row, reprojected rows."""
    label_values = np.asarray(label_values)
    if proj is not None:
        probs = np.asarray(probs)[np.asarray(proj).astype(np.int64)]
    return label_values[np.argmax(widen(probs, label_values, ignored_labels), axis=1)].astype(np.int32)


def confusion(truth, preds, label_values):
    """sklearn's confusion_matrix(truth, preds, labels=label_values): rows = truth, columns = prediction, int64;
    samples whose truth or prediction is not in the table are dropped."""
    label_values = [int(v) for v in label_values]
    slot = {v: i for i, v in enumerate(label_values)}
    C = np.zeros((len(label_values), len(label_values)), np.int64)
    for t, p in zip(np.asarray(truth).reshape(-1).tolist(), np.asarray(preds).reshape(-1).tolist()):
        if t in slot and p in slot:
            C[slot[t], slot[p]] += 1
    return C


def drop_ignored(C, label_values, ignored_labels):
    """np.delete of the ignored labels' rows and columns (tester.py:242-245)."""
    keep = np.asarray([v not in ignored_labels for v in label_values])
    return np.asarray(C)[keep][:, keep]


def iou(C):
    """IoU_from_confusions (utils/metrics.py:206-232) for one [C, C] matrix, float64."""
    C = np.asarray(C, np.float64)
    TP = np.diagonal(C)
    TP_plus_FN = C.sum(axis=1)
    TP_plus_FP = C.sum(axis=0)
    IoU = TP / (TP_plus_FP + TP_plus_FN - TP + 1e-6)
    mask = TP_plus_FN < 1e-3
    counts = np.sum(1 - mask)
    mIoU = IoU.sum() / (counts + 1e-6)
    return IoU + mask * mIoU
