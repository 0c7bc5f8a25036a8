"""float64 NumPy restatement of the segmentation loss / metrics contract of csrc/loss.hip (seg_*), own text.

logits (B, C, *) and labels (B, *). A point is KEPT when its label differs from ignore_index and lies in [0, C);
ignore_index wins when it is itself a class number; a label that is neither is left out and reported (`bad`). Over the
kept points, with w = 1 without class weights:
    lse_i  = log sum_c exp(x[b, c, s])
    loss   = sum w[t_i] (lse_i - x[b, t_i, s]) / sum w[t_i]                       (0 / 0 = NaN when nothing is kept)
    dx     = g w[t_i] / sum w * (softmax_c(x[b, :, s]) - onehot(t_i)),            0 for a point that is not kept
    pred_i = the LOWEST class index among the maximal logits
    counts = (#kept with pred == label, #kept),  conf[label, pred] += 1 over the kept points."""
import numpy as np


def seg_reference(logits, labels, weight=None, ignore_index=-100, grad_scale=1.0):
    x = np.asarray(logits, np.float64)
    B, C = x.shape[0], x.shape[1]
    x = x.reshape(B, C, -1)
    S = x.shape[2]
    lab = np.asarray(labels).astype(np.int64).reshape(B, S)
    w = np.ones(C, np.float64) if weight is None else np.asarray(weight, np.float64)
    not_ignored = lab != ignore_index
    in_range = (lab >= 0) & (lab < C)
    kept = not_ignored & in_range
    bad = bool((not_ignored & ~in_range).any())
    t = np.where(kept, lab, 0)

    m = x.max(axis=1, keepdims=True)
    e = np.exp(x - m)
    lse = m[:, 0, :] + np.log(e.sum(axis=1))                                   # (B, S)
    x_t = np.take_along_axis(x, t[:, None, :], axis=1)[:, 0, :]
    w_t = np.where(kept, w[t], 0.0)
    W = w_t.sum()
    with np.errstate(invalid="ignore", divide="ignore"):
        loss = np.float64((w_t * np.where(kept, lse - x_t, 0.0)).sum()) / np.float64(W)
    onehot = (np.arange(C)[None, :, None] == t[:, None, :]).astype(np.float64)
    soft = np.exp(x - lse[:, None, :])
    with np.errstate(invalid="ignore", divide="ignore"):
        grad = grad_scale * (w_t / W)[:, None, :] * (soft - onehot)
    grad = np.where(kept[:, None, :], grad, 0.0)

    pred = np.zeros((B, S), np.int64)
    best = x[:, 0, :].copy()
    for c in range(1, C):                                                      # strictly greater: the first maximum stays
        up = x[:, c, :] > best
        pred[up] = c
        best = np.where(up, x[:, c, :], best)
    hits = int((kept & (pred == lab)).sum())
    conf = np.zeros((C, C), np.int64)
    np.add.at(conf, (lab[kept], pred[kept]), 1)
    return {"loss": loss, "lse": lse, "grad": grad.reshape(np.asarray(logits).shape), "pred": pred.reshape(np.shape(labels)),
            "kept": kept.reshape(np.shape(labels)), "counts": np.array([hits, int(kept.sum())], np.int64), "conf": conf,
            "bad": bad, "weight_sum": W}


def quantised_case(shape, seed, ignore_index=-100, ignored_share=1.0 / 3.0, dtype=np.float32):
    """Logits on multiples of 0.5 in [-2, 2] (ties between classes are frequent), labels uniform over the classes with
    about `ignored_share` of them set to ignore_index, class weights in [0.5, 1.5). shape = (B, C, *)."""
    rng = np.random.default_rng(seed)
    x = (np.round(rng.standard_normal(shape) * 2.0) * 0.5).clip(-2.0, 2.0).astype(dtype)
    lshape = (shape[0],) + tuple(shape[2:])
    labels = rng.integers(0, shape[1], size=lshape).astype(np.int64)
    labels[rng.random(lshape) < ignored_share] = ignore_index
    w = (rng.random(shape[1]) + 0.5).astype(dtype)
    return x, labels, w


def loss_bound(n_points, n_classes, magnitude):
    """Bound for |loss - reference| when both are evaluated in float64: each kept term lse - x_t is a sum of n_classes
    exponentials, a log and two additions on values of size <= magnitude (a few roundings, taken as 8 + n_classes), the
    two sums over n_points add n_points roundings each: (8 + C + 2 N) * 2^-53 * max(1, magnitude)."""
    return (8 + n_classes + 2 * n_points) * 2.0 ** -53 * max(1.0, magnitude)
