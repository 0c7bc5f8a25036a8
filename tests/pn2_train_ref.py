"""NumPy restatement of the training-mode set abstraction kernels (csrc/pn2_rows.hip), own text.

Rows: R = B*M*K, row r = (b*M + m)*K + k. `sa_rows` builds the channel-major operand X (Cin, R) of a ball-query group
in the dtype of its inputs (a gather and ONE rounded subtraction), `rows_max` the maximum over a centroid's K rows with
the smallest k attaining it, and the backwards are their exact transposes. The ordered backward of the rows is
np.add.at over the positions in their natural (ascending) order, every addition rounded in the operand's dtype, like
tests/pn2_ordered_ref.py.
"""
import numpy as np

from pn2_ordered_ref import _ordered, flat_index


def sa_rows(xyz, feature, new_xyz, index, use_xyz=True):
    """xyz (B,3,N), feature (B,C,N) or None, new_xyz (B,3,M), index (B,M,K) -> X (Cin, B*M*K): the column of (b, m, k) is
    [feature[b, :, j] | xyz[b, :, j] - new_xyz[b, :, m]], j = index[b, m, k]; an index outside [0, N) reads as zero
    before the centroid is subtracted. Coordinates alone without features, features alone with use_xyz False."""
    b, _, n = xyz.shape
    ok = (index >= 0) & (index < n)
    j = np.where(ok, index, 0)
    parts = []
    if feature is not None:
        parts.append(np.stack([np.where(ok[bi][None], feature[bi][:, j[bi]], feature.dtype.type(0)) for bi in range(b)], 1))
    if use_xyz or feature is None:
        g = np.stack([np.where(ok[bi][None], xyz[bi][:, j[bi]], xyz.dtype.type(0)) for bi in range(b)], 1)   # (3,B,M,K)
        parts.append(g - np.transpose(new_xyz, (1, 0, 2))[..., None])
    x = np.concatenate(parts, 0)
    return np.ascontiguousarray(x.reshape(x.shape[0], -1))


def sa_rows_bwd(dx, index, c, n):
    """dX (Cin, R), index (B,M,K) -> dfeature (B,c,n) in dX's dtype: per key the sum of its positions' values in
    ascending position, rounded after every addition; rows c.. of dX (the coordinates) are not read."""
    b = index.shape[0]
    values = np.ascontiguousarray(np.transpose(dx[:c].reshape(c, b, -1), (1, 0, 2)))
    return _ordered(values, flat_index(index), n)


def sa_rows_bwd_wide(dx, index, c, n):
    """The same sums in float64 with, per element, the sum of the absolute contributions and their number (B,n): what
    the bound (T + 1) u sum|g| of the atomic form needs."""
    b = index.shape[0]
    values = np.ascontiguousarray(np.transpose(dx[:c].reshape(c, b, -1), (1, 0, 2))).astype(np.float64)
    ix = flat_index(index)
    count = np.stack([np.bincount(r[(r >= 0) & (r < n)], minlength=n)[:n] for r in ix])
    return _ordered(values, ix, n), _ordered(np.abs(values), ix, n), count


def rows_max(y, b, m, k):
    """y (B*M*K, Cout) -> out (B,Cout,M) and arg (B,Cout,M) int32, the smallest k attaining the maximum (np.argmax takes
    the first occurrence, and the first NaN when there is one)."""
    t = y.reshape(b, m, k, y.shape[1])
    arg = np.argmax(t, axis=2)
    out = np.take_along_axis(t, arg[:, :, None, :], axis=2)[:, :, 0, :]
    return np.ascontiguousarray(out.transpose(0, 2, 1)), np.ascontiguousarray(arg.transpose(0, 2, 1)).astype(np.int32)


def rows_max_bwd(g, arg, k):
    """g, arg (B,Cout,M) -> dY (B*M*K, Cout): g at k == arg, +0 elsewhere."""
    b, cout, m = g.shape
    dy = np.zeros((b, m, k, cout), g.dtype)
    np.put_along_axis(dy, arg.transpose(0, 2, 1)[:, :, None, :].astype(np.int64), g.transpose(0, 2, 1)[:, :, None, :], axis=2)
    return dy.reshape(b * m * k, cout)
