"""NumPy restatements of the MVPNet baseline's whole-scene test (mvpnet/utils/chunk_util.py:4-53,
mvpnet/test_mvpnet_3d.py:141-178, mvpnet/evaluate_3d.py:19-69), written for the tests of csrc/chunk.hip, and the scenes
those tests share. Nothing here reads the reference tree and nothing needs sklearn.

Arithmetic, as the library's header states it: box membership is an inclusive comparison that is exact for float32
coordinates in any wider type; the logit sums are float32 additions in chunk order; the mean is a float32 division by
max(visits, 1); the prediction is the first maximum, C where a point was never visited.
"""
import numpy as np

CHUNK_SIZE, STRIDE, MARGIN = (1.5, 1.5), 0.5, (0.2, 0.2)


# ------------------------------------------------------------------------------------------------------------ scenes

def dyadic_scene(seed=0, n=6000, ext=(3.0, 2.5, 2.0), q=2.0 ** -6, origin=(-1.25, 0.5, 0.0)):
    """Uniform points in a box, the region x > 0.45 ext and y > 0.35 ext thinned to 3 %, coordinates on multiples of q
    around `origin`, the two extreme corners pinned. Every chunk corner is exactly representable, hundreds of points
    lie exactly on chunk edges."""
    rng = np.random.default_rng(seed)
    p = rng.random((n, 3)) * np.asarray(ext)
    keep = ~((p[:, 0] > ext[0] * 0.45) & (p[:, 1] > ext[1] * 0.35)) | (rng.random(n) < 0.03)
    p = p[keep]
    p = np.round(p / q) * q + np.asarray(origin)
    p[0] = origin
    p[1] = np.asarray(origin) + np.asarray(ext)
    return p.astype(np.float32)


def random_scene(seed, n, ext=(3.0, 2.5, 2.0), origin=(0.1, 0.3, 0.0)):
    """Non-dyadic: uniform float32 points, the same region thinned to 3 % (so that corners differ in their counts)."""
    rng = np.random.default_rng(seed)
    p = rng.random((n, 3)) * np.asarray(ext)
    keep = ~((p[:, 0] > ext[0] * 0.45) & (p[:, 1] > ext[1] * 0.35)) | (rng.random(n) < 0.03)
    return (p[keep] + np.asarray(origin)).astype(np.float32)


def median_threshold(points):
    """A threshold that keeps some corners and drops others: the median of the inner counts."""
    s = sorted(inner_counts(points))
    return s[len(s) // 2]


def small_scene(seed, n, side):
    """n points in a cube of the given side with both extreme corners present (n >= 2), or one point."""
    rng = np.random.default_rng(seed)
    p = (rng.random((n, 3)) * side).astype(np.float32)
    if n >= 2:
        p[0] = 0.0
        p[1] = side
    return p


# ------------------------------------------------------------------------------------------------------------ chunks

def corners(points, chunk_size=CHUNK_SIZE, stride=STRIDE):
    """The chunk corners in the reference's order (x outer, y inner), formed from the float32 extremes of the scene with
    the installed NumPy's promotion, as the reference forms them."""
    chunk_size = np.asarray(chunk_size)
    top, bottom = np.max(points, axis=0), np.min(points, axis=0)
    span = top - bottom
    per_axis = np.ceil((span[:2] - chunk_size) / stride).astype(int) + 1
    return [np.asarray((bottom[0] + i * stride, bottom[1] + j * stride))
            for i in range(per_axis[0]) for j in range(per_axis[1])]


def members(points, low, high):
    """Boolean mask of the points with low <= xy <= high on both axes (both ends inclusive)."""
    xy = points[:, :2]
    return np.all(np.logical_and(xy >= low, xy <= high), axis=1)


def inner_counts(points, chunk_size=CHUNK_SIZE, stride=STRIDE):
    cs = np.asarray(chunk_size)
    return [int(members(points, c, c + cs).sum()) for c in corners(points, chunk_size, stride)]


def scene2chunks(points, chunk_size=CHUNK_SIZE, stride=STRIDE, thresh=1000, margin=MARGIN):
    """(list of ascending int64 index vectors, list of float64 bboxes (x1, y1, z1, x2, y2, z2)) of the kept chunks: a
    corner is kept when its box WITHOUT margin holds >= thresh points; the indices are those of the box WITH margin."""
    cs, mg = np.asarray(chunk_size), np.asarray(margin)
    indices, bboxes = [], []
    for c in corners(points, chunk_size, stride):
        if members(points, c, c + cs).sum() < thresh:
            continue
        ind = np.nonzero(members(points, c - mg, c + cs + mg))[0]
        z = points[ind, 2]
        indices.append(ind)
        bboxes.append(np.hstack([c - mg, z.min(), c + cs + mg, z.max()]))
    return indices, bboxes


def thresholds(points):
    """Three thresholds from the scene's own inner counts: one equal to a corner's count (that corner is kept), that
    plus one (it is dropped), and one between two smaller counts."""
    s = sorted(inner_counts(points))
    assert len(s) >= 6 and s[5] > s[4] > s[3], s
    return s[5], s[5] + 1, (s[3] + s[4] + 1) // 2


# -------------------------------------------------------------------------------------------------------------- vote

def vote_scene(num_points, num_classes, chunks):
    """The loop of test_mvpnet_3d.py:141-178. chunks: iterable of (logits [C, ld] float32, chunk_ind [n] with n <= ld);
    only the first n columns vote. Returns (sums [N,C] f32 before the division, visits [N] int32, mean [N,C] f32,
    pred [N] int64)."""
    sums = np.zeros([num_points, num_classes], dtype=np.float32)
    visits = np.zeros(num_points, dtype=np.int32)
    for logits, chunk_ind in chunks:
        chunk_ind = np.asarray(chunk_ind)
        cols = np.asarray(logits, np.float32).T[:len(chunk_ind)]
        sums[chunk_ind] += cols
        visits[chunk_ind] += 1
    assert visits.max(initial=0) < 256                    # the reference's uint8 counter has not wrapped
    mean = sums / np.maximum(visits[:, np.newaxis].astype(np.uint8), 1)
    assert mean.dtype == np.float32
    pred = np.argmax(mean, axis=1) if num_points else np.zeros(0, np.int64)
    pred = pred.astype(np.int64)
    pred[visits == 0] = num_classes
    return sums, visits, mean, pred


def pad_choice(nc, min_nb_pts):
    """Rows of a sparse chunk after the reference's padding (:155-156): its own nc rows, then min_nb_pts - nc rows drawn
    from the global NumPy generator."""
    extra = np.random.randint(nc, size=min_nb_pts - nc)
    return np.concatenate([np.arange(nc), extra])


# ------------------------------------------------------------------------------------------------------------- score

def confusion(gt, pred, num_classes):
    """Rows = truth, columns = prediction, over the pairs with both in 0..C-1 (what confusion_matrix(labels=arange(C))
    counts); int64."""
    gt, pred = np.asarray(gt).reshape(-1).astype(np.int64), np.asarray(pred).reshape(-1).astype(np.int64)
    ok = (gt >= 0) & (gt < num_classes) & (pred >= 0) & (pred < num_classes)
    return np.bincount(gt[ok] * num_classes + pred[ok], minlength=num_classes ** 2).reshape(num_classes, num_classes)


def evaluator_update(matrix, pred, gt, num_classes):
    """Evaluator.update (evaluate_3d.py:19-36) on a float64 matrix, in place: all-negative truth changes nothing; the
    -100 -> C rewrite is implied by dropping truths outside 0..C-1."""
    if np.all(np.asarray(gt) < 0):
        return matrix
    matrix += confusion(gt, pred, num_classes)
    return matrix


def class_iou(matrix):
    out = []
    for i in range(matrix.shape[0]):
        tp = matrix[i, i]
        union = matrix[:, i].sum() + matrix[i, :].sum() - tp
        out.append(float("nan") if union == 0 else tp / union)
    return out


def overall_acc(matrix):
    return np.sum(np.diag(matrix)) / np.sum(matrix)


def table_logits(seed, num_classes, sizes, ld_extra=0):
    """Pre-generated random float32 logits [C, n + ld_extra] per chunk, a few exact ties among them."""
    rng = np.random.default_rng(seed)
    out = []
    for n in sizes:
        t = rng.standard_normal((num_classes, n + ld_extra)).astype(np.float32)
        t[:, ::7] = np.round(t[:, ::7])                    # small integers: ties between classes within a column
        out.append(t)
    return out
