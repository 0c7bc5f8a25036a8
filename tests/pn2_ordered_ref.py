"""NumPy oracle of the ordered PointNet++ backwards (csrc/pn2_ordered.hip), own text.

An int64 index (B, N2, K) selects keys in [0, n1); per batch element it is a flat list of L = N2*K positions
p = n*K + k. `csr` is the transposed index (row (b, j) = the positions that hold key j, ascending; entries outside
[0, n1) are in no row). The two backwards add, for every key, the contributions of its positions in ascending position,
every product and every addition rounded in the dtype of the operands: np.add.at is unbuffered and walks its index
array front to back, so feeding it the positions in their natural order gives exactly those sums.
"""
import numpy as np


def flat_index(index):
    index = np.asarray(index)
    return index.reshape(index.shape[0], -1)


def csr(index, n1):
    """index (B,N2,K) or (B,L) -> row_start int32 [B*n1 + 1], entries int32 [number of in-range entries]."""
    ix = flat_index(index)
    b = ix.shape[0]
    lengths, entries = [], []
    for bi in range(b):
        pos = np.nonzero((ix[bi] >= 0) & (ix[bi] < n1))[0]
        keys = ix[bi, pos]
        entries.append(pos[np.argsort(keys, kind="stable")])           # by key, positions ascending inside a key
        lengths.append(np.bincount(keys, minlength=n1)[:n1] if n1 > 0 else np.zeros(0, np.int64))
    lengths = np.concatenate(lengths) if b else np.zeros(0, np.int64)
    row_start = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    entries = (np.concatenate(entries) if b else np.zeros(0, np.int64)).astype(np.int32)
    return row_start, entries


def _ordered(values, ix, n1):
    """values (B,C,L) in the kernel's dtype, ix (B,L) -> (B,C,n1): per key the sum of its positions' values, ascending."""
    b, c, _ = values.shape
    out = np.zeros((b, c, n1), values.dtype)
    for bi in range(b):
        pos = np.nonzero((ix[bi] >= 0) & (ix[bi] < n1))[0]            # ascending
        acc = np.zeros((n1, c), values.dtype)                           # one row per key: a row is added per position
        np.add.at(acc, ix[bi, pos], np.ascontiguousarray(values[bi][:, pos].T))
        out[bi] = acc.T
    return out


def interpolate_bwd(grad_out, index, weight, n1):
    """grad_out (B,C,N2), index (B,N2,3), weight (B,N2,3), all of one float dtype -> grad_in (B,C,n1) in that dtype."""
    dt = grad_out.dtype
    assert weight.dtype == dt and dt in (np.float32, np.float64)
    ix = flat_index(index)
    b, c, n2 = grad_out.shape
    k = ix.shape[1] // max(n2, 1) if n2 else 3
    w = np.asarray(weight).reshape(b, 1, -1)
    products = np.repeat(grad_out, k, axis=2) * w                       # g[b, c, p // 3] * w[b, p], rounded in dt
    assert products.dtype == dt
    return _ordered(products, ix, n1)


def group_points_bwd(grad_out, index, n1):
    """grad_out (B,C,N2,K), index (B,N2,K) -> grad_in (B,C,n1) in grad_out's dtype."""
    b, c = grad_out.shape[:2]
    return _ordered(np.ascontiguousarray(grad_out).reshape(b, c, -1), flat_index(index), n1)


def ordered_sum_loop(values, keys, n1):
    """The same sum for ONE (b, c) slice written out: values (L,), keys (L,) -> (n1,), an accumulator of values' dtype."""
    out = [values.dtype.type(0)] * n1
    for p in range(keys.shape[0]):
        j = int(keys[p])
        if 0 <= j < n1:
            out[j] = values.dtype.type(out[j] + values[p])
    return np.asarray(out, values.dtype)


def counts(index, n1):
    """(B, n1): the number of positions per key."""
    ix = flat_index(index)
    return np.stack([np.bincount(r[(r >= 0) & (r < n1)], minlength=n1)[:n1] for r in ix]) if ix.shape[0] else \
        np.zeros((0, n1), np.int64)


def ball_like_index(b, n2, k, n1, seed):
    """An index shaped like a ball query's: ascending hits, the tail padded with the first hit, some rows of -1."""
    rng = np.random.default_rng(seed)
    index = np.full((b, n2, k), -1, np.int64)
    for bi in range(b):
        for n in range(n2):
            hits = int(rng.integers(0, k + 1))
            if rng.random() < 0.15 or hits == 0:
                continue
            h = np.sort(rng.choice(n1, size=min(hits, n1), replace=False))
            index[bi, n, :h.size] = h
            index[bi, n, h.size:] = h[0]
    return index
