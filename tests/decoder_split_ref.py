"""The decoder's unary layer in its SPLIT form, restated in float64 NumPy:

    cat([x_c[idx], skip]) . W^T  =  (x_c . W[:, :C1]^T)[idx]  +  skip . W[:, C1:]^T

with G_c[j] = sum of g[n] over the fine rows n with idx[n] = j:

    dx_c = G_c . W[:, :C1]      d_skip = g . W[:, C1:]      dW = [ G_c^T . x_c | g^T . skip ]

Nothing here builds the concatenation: tests/test_decoder_split_cpu.py holds this restatement to the concatenated form
of tests/gemm_ref.upsample_cat_linear, tests/test_decoder_split_gpu.py holds the kernels to this restatement."""
import numpy as np

# (Ns, Nq, C1, C2, N): coarse rows, fine rows, coarse channels, skip channels, output channels
CASES = [
    (9, 70, 24, 12, 20),          # nothing is a multiple of a tile; dW slabs of <= 16 and > 16 columns meet
    (5, 40, 2048, 1024, 64),      # few rows and a deep reduction: both forward products split
    (300, 1000, 30, 7, 16),       # the odd case of test_upsample_cat_linear_equals_the_three_steps
    (64, 257, 64, 32, 96),        # one row over a 64-row tile
]
# the same layer at row counts where the product carries the BatchNorm-statistics epilogue: the narrow tile class
# (18 columns, not a multiple of 4: statistics above 128 rows) and the wide one (96 columns: above 1024 rows)
STATS_CASES = [(300, 1300, 30, 7, 18), (64, 1100, 64, 32, 96)]


def first_column(idx, Ns):
    """The upsampling index of every fine row; anything outside [0, Ns) is the shadow row Ns."""
    j = np.asarray(idx).reshape(len(idx), -1)[:, 0].astype(np.int64)
    return np.where((j < 0) | (j >= Ns), Ns, j)


def split_form(x, idx, skip, W, g, n_valid=None):
    x, skip, W, g = (np.asarray(t, np.float64) for t in (x, skip, W, g))
    Ns, C1 = x.shape
    N = W.shape[0]
    j = first_column(idx, Ns)
    W1, W2 = W[:, :C1], W[:, C1:]
    Yc = np.concatenate([x @ W1.T, np.zeros((1, N))])          # coarse rows, then the shadow row
    y = skip @ W2.T + Yc[j]
    Gc = np.zeros((Ns + 1, N))
    np.add.at(Gc, j, g)
    Gc = Gc[:Ns]
    out = {"y": y, "dx": Gc @ W1, "dskip": g @ W2, "dW": np.concatenate([Gc.T @ x, g.T @ skip], 1)}
    if n_valid is not None:
        v = y[:max(int(n_valid), 0)]
        out["stat_sum"] = v.sum(0)
        out["stat_m2"] = ((v - v.mean(0)) ** 2).sum(0) if len(v) else np.zeros(N)
    return out


def inputs(case, shadow=False, two_d=False, integers=False, seed=0):
    """x, idx (int64), skip, W, g of a case. shadow: a third of the fine rows point at the shadow row; two_d: the index is
    an [Nq, 4] matrix whose first column counts; integers: small integers in float32 (every product and sum exact)."""
    Ns, Nq, C1, C2, N = case
    rng = np.random.default_rng(1000 * seed + Ns + Nq + C1 + N)
    if integers:
        draw = lambda *s: rng.integers(-3, 4, s).astype(np.float32)
        x, skip, W, g = draw(Ns, C1), draw(Nq, C2), draw(N, C1 + C2), draw(Nq, N)
    else:
        x, skip = rng.normal(size=(Ns, C1)).astype(np.float32), rng.normal(size=(Nq, C2)).astype(np.float32)
        W = (rng.normal(size=(N, C1 + C2)) * 0.05).astype(np.float32)
        g = rng.normal(size=(Nq, N)).astype(np.float32)
    j = rng.integers(0, Ns, Nq)
    if shadow:
        j[rng.permutation(Nq)[:Nq // 3]] = Ns
    idx = j
    if two_d:
        idx = rng.integers(0, Ns + 1, (Nq, 4))
        idx[:, 0] = j
    return x, idx.astype(np.int64), skip, W, g
