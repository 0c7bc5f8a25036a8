"""The ragged point ops restated on top of tests/pn2_ref.py: cloud b of a padded batch is the rows [0, n_b) of its
block, and every result is what pn2_ref gives for that slice alone. Nothing here reads a row at or beyond n_b."""
import numpy as np

import pn2_ref


def clamp(n, size):
    return min(max(int(n), 1), int(size))


def fps(points, lengths, m, one=pn2_ref.fps_closed):
    """points (B,N,D), lengths (B,) -> (B,m) int64: `one` on points[b, :n_b]. Where m > n_b the last pick repeats: after
    n_b rounds every point is a centroid or a duplicate of one, so no distance is positive any more."""
    out = np.empty((len(points), m), np.int64)
    for b, (p, n) in enumerate(zip(points, lengths)):
        n = clamp(n, p.shape[0])
        picks = one(p[:n], min(m, n))
        out[b, :len(picks)] = picks
        out[b, len(picks):] = picks[-1]
    return out


def fps_rule_from(points, m, n_rule):
    """pn2_ref.fps_closed on one cloud (n,D), with the tie key built from the block size of n_rule >= n points."""
    def pick(run, cur):
        top = run.max()
        if not top > 0:
            return cur
        cand = np.nonzero(run == top)[0]
        return int(cand[np.argmin(pn2_ref.tie_key(cand, n_rule))])
    return pn2_ref._fps(points, m, pick)


# (n, N, centroids, seed): lattice clouds of n points inside a padded block of N
RULE_CASES = ((300, 1000, 140, 21), (70, 130, 40, 22), (17, 64, 17, 23), (511, 1024, 140, 24), (200, 257, 130, 25),
              (33, 64, 33, 26))


def ball_query(query, key, key_lengths, radius, k):
    """query (B,N1,3), key (B,N2,3), key_lengths (B,) -> index, distance (B,N1,k): pn2_ref.ball_query of batch element b
    against key[b, :n_b]."""
    parts = [pn2_ref.ball_query(query[b:b + 1], key[b:b + 1, :clamp(n, key.shape[1])], radius, k)
             for b, n in enumerate(key_lengths)]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
