"""NumPy oracle of the pooling helpers and of their ordered (deterministic-mode) backwards, own text.

max_pool and closest_pool of the KPConv blocks (models/blocks.py:79-110) gather rows of x through an index matrix
idx [Nq, H] whose entries outside [0, Ns) select an appended zero "shadow" row; max_pool takes the maximum over the H
gathered rows, closest_pool keeps column 0. Their backwards are sums of gradient rows per support row j. In
deterministic mode (csrc/revlist.hip) every such sum has ONE accumulator per output element that starts from base[j, c]
(or zero) and adds the contributions of the query rows n that reach j in ascending n. Only additions are involved, so
the same walk in np.float32 gives the expected BITS and in np.float64 the referee.

The sums are written here in scatter form: np.add.at is unbuffered and walks its index array front to back, so feeding
it the query rows in their natural order adds, for every key, in ascending n. `ordered_sum_loop` is the same sum as a
plain Python loop over one column (the CPU test holds the two against each other).

Contract of the inputs: the real entries of one index row are DISTINCT (a neighbour matrix never lists a support
twice; the reverse-list builder ranks by counting and relies on it). Duplicate entries inside a row are out of scope:
`case` never generates them and nothing here defines what they would mean.
"""
import numpy as np

H_CASES = {"h1": 1, "h7": 7, "h8": 8, "h9": 9, "h20": 20}          # both sides of an 8-wide unrolled column trip
CASES = ("h1", "h7", "h8", "h9", "h20", "ties")
TIE_FREE = ("h1", "h7", "h8", "h9", "h20")
_SIZES = {"h1": (70, 260), "h7": (70, 260), "h8": (300, 1000), "h9": (85, 332), "h20": (300, 1200), "ties": (70, 300)}


def reverse_lists(idx, Ns, first_column=False):
    """Row j = the rows n of idx (of idx[:, 0] alone when first_column) that contain j, ascending. Python lists."""
    idx = np.asarray(idx)
    if first_column:
        idx = idx[:, :1]
    rows = [[] for _ in range(Ns)]
    for n in range(idx.shape[0]):
        for j in idx[n]:
            if 0 <= j < Ns:
                rows[int(j)].append(n)
    return rows


def _padded(x):
    return np.concatenate([x, np.zeros_like(x[:1])], 0)


def _clamped(idx, Ns):
    idx = np.asarray(idx, np.int64)
    return np.where((idx < 0) | (idx >= Ns), Ns, idx)


def max_pool_fwd(x, idx):
    """(out [Nq, C], arg [Nq, C] int32): the maximum over the gathered rows, the zero shadow row taking part, and the
    FIRST column that attains it (a later column wins only when strictly greater). H == 0: out = 0, arg = 0."""
    Ns, C = x.shape
    idx = _clamped(idx, Ns)
    Nq, H = idx.shape
    out = np.zeros((Nq, C), x.dtype)
    arg = np.zeros((Nq, C), np.int32)
    if H == 0:
        return out, arg
    xp = _padded(x)
    out[:] = xp[idx[:, 0]]
    for h in range(1, H):
        v = xp[idx[:, h]]
        better = v > out
        out = np.where(better, v, out)
        arg = np.where(better, np.int32(h), arg)
    return out, arg


def max_pool_bwd(g, arg, idx, Ns, base=None, dtype=np.float32):
    """dx[j, c] = base[j, c] + sum over n ascending with idx[n, arg[n, c]] == j of g[n, c], accumulated in `dtype`."""
    Nq, C = g.shape
    dx = np.zeros((Ns, C), dtype) if base is None else np.array(base, dtype)
    if Nq == 0 or np.asarray(idx).shape[1] == 0:
        return dx
    j = np.take_along_axis(_clamped(idx, Ns), np.asarray(arg, np.int64), axis=1)          # [Nq, C] winning support
    flat = (j * C + np.arange(C)[None, :]).reshape(-1)                                  # n-major: ascending n per key
    keep = (j < Ns).reshape(-1)
    np.add.at(dx.reshape(-1), flat[keep], np.asarray(g, dtype).reshape(-1)[keep])
    return dx


def gather_sum_rows(g, rev_lists, base=None, dtype=np.float32):
    """out[j] = base[j] + sum of g[n] over the entries n of rev_lists[j] in list order, accumulated in `dtype`: the
    backward of x_padded[idx[:, 0]] when rev_lists = reverse_lists(idx, Ns, first_column=True)."""
    Ns, C = len(rev_lists), g.shape[1]
    out = np.zeros((Ns, C), dtype) if base is None else np.array(base, dtype)
    keys = np.asarray([j for j, r in enumerate(rev_lists) for _ in r], np.int64)
    rows = np.asarray([n for r in rev_lists for n in r], np.int64)
    if rows.size:
        np.add.at(out, keys, np.asarray(g, dtype)[rows])
    return out


def ordered_sum_loop(values, keys, n_keys, start=None):
    """One column written out: values (L,), keys (L,) -> (n_keys,); key by key one accumulator of values' dtype."""
    out = [values.dtype.type(0)] * n_keys if start is None else [values.dtype.type(v) for v in start]
    for p in range(keys.shape[0]):
        j = int(keys[p])
        if 0 <= j < n_keys:
            out[j] = values.dtype.type(out[j] + values[p])
    return np.asarray(out, values.dtype)


def index_matrix(Ns, Nq, H, seed, unused=None):
    """[Nq, H] int64: every row H distinct draws from Ns + Ns // 3 values, those >= Ns clamped to the shadow value Ns
    (about a quarter of the entries, column 0 included); `unused`: a support that no row may name."""
    rng = np.random.default_rng(seed)
    idx = np.stack([rng.choice(Ns + Ns // 3, size=H, replace=False) for _ in range(Nq)]).astype(np.int64).reshape(Nq, H)
    idx[idx >= Ns] = Ns
    if unused is not None:
        idx[idx == unused] = Ns
    return idx


class Case:
    """idx [Nq, H] int64, Ns, and the rows that carry the edges (None where the width H leaves no room for one)."""

    def __init__(self, name, idx, Ns, negative, rows, tie_pair, zero_support):
        self.name, self.idx, self.Ns = name, idx, Ns
        self.Nq, self.H = idx.shape
        self.negative = negative              # supports whose features are all negative
        self.rows = rows                      # {"all_shadow": n, "negative_and_shadow": n or None, "negative_only": n}
        self.tie_pair = tie_pair              # two supports with equal, dominating features (or None)
        self.zero_support = zero_support      # a support whose features are exactly zero: ties with the shadow row
        self.unused = Ns - 1                  # its reverse row is empty

    def features(self, C, seed=0):
        """x [Ns, C] float32 with the edges of the case written in."""
        rng = np.random.default_rng(1000 * C + seed + self.Nq)
        x = rng.standard_normal((self.Ns, C)).astype(np.float32)
        x[self.negative] = -np.abs(x[self.negative]) - np.float32(0.125)
        if self.tie_pair is not None:
            a, b = self.tie_pair
            x[a] = np.abs(x[a]) + np.float32(5.0)
            x[b] = x[a]
        if self.zero_support is not None:
            x[self.zero_support] = 0.0
        return x

    def gradients(self, C, seed=0):
        """(g [Nq, C], base [Ns, C]) float32."""
        rng = np.random.default_rng(2000 * C + seed + self.Nq)
        return rng.standard_normal((self.Nq, C)).astype(np.float32), rng.standard_normal((self.Ns, C)).astype(np.float32)


def case(name):
    """The named index matrix with its edge rows. Supports [0, Ns // 4) carry negative features; support Ns - 1 is in
    no row; row 7 is all shadow; row 11 = negative supports then shadow entries; row 13 = negative supports only.
    "ties": supports (a, b) share dominating features and meet in rows 20-25 in both column orders; a zero-valued
    support meets shadow entries in rows 30 (support first) and 31 (shadow first)."""
    Ns, Nq = _SIZES[name]
    H = H_CASES.get(name, 9)
    idx = index_matrix(Ns, Nq, H, seed=sum(map(ord, name)), unused=Ns - 1)
    n_neg = Ns // 4
    negative = np.arange(n_neg)
    rows = {"all_shadow": 7, "negative_and_shadow": None, "negative_only": 13}
    idx[7] = Ns
    assert H <= n_neg
    idx[13] = np.arange(H)[::-1]
    if H >= 2:
        rows["negative_and_shadow"] = 11
        half = H // 2
        idx[11, :half] = np.arange(2, 2 + half)
        idx[11, half:] = Ns
    tie_pair = zero_support = None
    if name == "ties":
        a, b, z = n_neg + 3, n_neg + 9, n_neg + 12
        tie_pair, zero_support = (a, b), z
        idx[idx == z] = Ns                               # the zero support appears in rows 30 and 31 only
        for r, (ca, cb) in zip(range(20, 26), [(0, 1), (1, 0), (2, 8), (8, 2), (7, 8), (8, 7)]):
            row = idx[r]
            row[(row == a) | (row == b)] = Ns
            row[ca], row[cb] = a, b
        idx[30] = Ns
        idx[30, :3] = [1, z, 2]                          # negative, zero, negative, shadow ...: the zero support wins
        idx[31] = Ns
        idx[31, 1:4] = [1, z, 2]                         # shadow first: the tie goes to the shadow row, no gradient
    for n in range(Nq):                                   # the contract: real entries of a row are distinct
        real = idx[n][idx[n] < Ns]
        assert real.size == np.unique(real).size, (name, n)
    assert not (idx == Ns - 1).any()
    return Case(name, idx, Ns, negative, rows, tie_pair, zero_support)
