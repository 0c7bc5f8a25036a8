"""NumPy restatements of the MVPNet baseline's point ops (reference: mvpnet/ops/cuda/*.cu), own text.

Squared distances are formed in the input dtype as ((dx*dx) + (dy*dy)) + (dz*dz): NumPy rounds every elementwise
operation, so there is no FMA -- the arithmetic contract of csrc/pn2.hip.

Farthest point sampling comes twice: `fps_literal` walks the reference kernel's own schedule (every thread scans its
strided points with a strict >, then the LDS tree halves the block with a strict <), `fps_closed` is the closed form of
what that schedule picks among ties. `fps_argmax` is the plain np.argmax version of the reference's own test, which
differs from both whenever the largest distance is shared.
"""
import math

import numpy as np

J_BITS = 23


def ref_block(n):
    """The reference's block size for n points (fps_kernel.cu:21-24 and the switch at :166-175)."""
    pow_2 = int(math.log(float(n)) / math.log(2.0))
    b = max(min(1 << pow_2, 512), 1)
    return b if b >= 16 else 16


def dist2(p, c):
    """p (..., D), c (D,) -> squared distances in p's dtype, each operation rounded."""
    d = p - c
    out = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]
    if p.shape[-1] == 3:
        out = out + d[..., 2] * d[..., 2]
    return out


def _bitrev(v, bits):
    out = np.zeros_like(v)
    for i in range(bits):
        out |= ((v >> i) & 1) << (bits - 1 - i)
    return out


def tie_key(j, n):
    """Smaller wins among points of equal distance: (bitreverse(j mod Bk, log2 Bk) << 23) | j."""
    bk = ref_block(n)
    lb = bk.bit_length() - 1
    j = np.asarray(j, np.int64)
    return (_bitrev(j % bk, lb) << J_BITS) | j


def _fps(points, m, pick):
    n = points.shape[0]
    if m < 1 or m > n:
        raise ValueError("need 1 <= num_centroids <= num_points")
    run = np.full(n, np.inf, points.dtype)
    cur, out = 0, [0]
    for _ in range(1, m):
        run = np.minimum(run, dist2(points, points[cur]))
        cur = pick(run, cur)
        out.append(cur)
    return np.asarray(out, np.int64)


def _pick_literal(run, cur):
    n = run.shape[0]
    bk = ref_block(n)
    rows = -(-n // bk)
    grid = np.full(rows * bk, -1.0, run.dtype)          # padding never passes `dist > max_dist`
    grid[:n] = run
    grid = grid.reshape(rows, bk)                       # column t = the points thread t scans, in scan order
    first = np.argmax(grid, axis=0)                     # strict >: the first of a thread's largest
    smem_dist = grid[first, np.arange(bk)]
    smem_idx = first * bk + np.arange(bk)
    none = ~(smem_dist > 0)                             # max_dist starts at 0 with max_idx = cur_idx
    smem_dist = np.where(none, run.dtype.type(0), smem_dist)
    smem_idx = np.where(none, cur, smem_idx)
    off = bk // 2
    while off > 0:                                      # if (dist1 < dist2) take the upper half's entry
        take = smem_dist[:off] < smem_dist[off:2 * off]
        smem_dist[:off] = np.where(take, smem_dist[off:2 * off], smem_dist[:off])
        smem_idx[:off] = np.where(take, smem_idx[off:2 * off], smem_idx[:off])
        off //= 2
    return int(smem_idx[0])


def _pick_closed(run, cur):
    top = run.max()
    if not top > 0:
        return cur
    cand = np.nonzero(run == top)[0]
    return int(cand[np.argmin(tie_key(cand, run.shape[0]))])


def _pick_argmax(run, cur):
    return int(np.argmax(run))


def fps_literal(points, m):
    """points (N, D) of one cloud -> (m,) int64, by the reference kernel's schedule."""
    return _fps(points, m, _pick_literal)


def fps_closed(points, m):
    return _fps(points, m, _pick_closed)


def fps_argmax(points, m):
    return _fps(points, m, _pick_argmax)


def fps_batch(points, m, one=fps_closed):
    """points (B, N, D) -> (B, m)."""
    return np.stack([one(p, m) for p in points])


def lattice_cloud(n, seed):
    """n points drawn with replacement from {0..4}^3 (float arithmetic on them is exact): ties and duplicates."""
    return np.random.default_rng(seed).integers(0, 5, size=(n, 3)).astype(np.float64)


LATTICE_CASES = ((1100, 140, 11), (70, 40, 12), (16, 16, 13))       # (points, centroids, seed)


def ball_query(query, key, radius, k):
    """query (B,N1,3), key (B,N2,3) -> index (B,N1,k) int64, distance (B,N1,k) in the input dtype.
    r*r is formed in the input dtype from the float32 radius the reference's entry point receives."""
    dt = query.dtype.type
    r = dt(np.float32(radius))
    r2 = r * r
    b, n1 = query.shape[:2]
    index = np.full((b, n1, k), -1, np.int64)
    distance = np.full((b, n1, k), -1, query.dtype)
    for bi in range(b):
        for i in range(n1):
            d = dist2(key[bi], query[bi, i])
            hit = np.nonzero(d < r2)[0][:k]
            if hit.size:
                index[bi, i, :hit.size] = hit
                index[bi, i, hit.size:] = hit[0]
                distance[bi, i, :hit.size] = d[hit]
    return index, distance


def knn3(query, key):
    """query (B,N1,3), key (B,N2,3) -> index (B,N1,3) int64, squared distance (B,N1,3): ascending, ties to the lower key."""
    if key.shape[1] < 3:
        raise ValueError("need at least 3 keys")
    b, n1 = query.shape[:2]
    index = np.empty((b, n1, 3), np.int64)
    distance = np.empty((b, n1, 3), query.dtype)
    for bi in range(b):
        for i in range(n1):
            d = dist2(key[bi], query[bi, i])
            o = np.argsort(d, kind="stable")[:3]
            index[bi, i], distance[bi, i] = o, d[o]
    return index, distance


def interpolate_fwd(feature, index, weight, dtype=np.float64):
    """feature (B,C,N1), index (B,N2,3), weight (B,N2,3) -> (B,C,N2) in `dtype` (float64; np.longdouble to referee a
    float64 kernel), and sum_k |f_k w_k| (the error scale)."""
    f, w = np.asarray(feature, dtype), np.asarray(weight, dtype)
    b = f.shape[0]
    g = np.stack([f[bi][:, index[bi]] for bi in range(b)])          # (B,C,N2,3)
    terms = g * w[:, None]
    return terms.sum(-1), np.abs(terms).sum(-1)


def interpolate_bwd(grad_out, index, weight, n1, dtype=np.float64):
    """grad_out (B,C,N2) -> grad_in (B,C,N1) in `dtype`, sum |g w| per element and the number of contributions (B,N1)."""
    g, w = np.asarray(grad_out, dtype), np.asarray(weight, dtype)
    b, c, n2 = g.shape
    gi, scale = np.zeros((b, c, n1), dtype), np.zeros((b, c, n1), dtype)
    count = np.zeros((b, n1), np.int64)
    for bi in range(b):
        for k in range(3):
            t = g[bi] * w[bi, :, k][None]                           # (C,N2)
            for ci in range(c):
                np.add.at(gi[bi, ci], index[bi, :, k], t[ci])
                np.add.at(scale[bi, ci], index[bi, :, k], np.abs(t[ci]))
            np.add.at(count[bi], index[bi, :, k], 1)
    return gi, scale, count
