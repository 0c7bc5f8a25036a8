"""``ball_query`` / ``ball_query_distance`` with the reference's signatures (mvpnet/ops/ball_query.py:17-46) on
the HIP kernel (csrc/pn2.hip)."""
try:
    from ..._native import ops
except ImportError:
    from _native import ops


def _rows(query, key, transpose):
    if transpose:
        query, key = query.transpose(1, 2), key.transpose(1, 2)
    return query.contiguous(), key.contiguous()


def ball_query(query, key, radius, max_neighbors, transpose=True, key_lengths=None):
    """query (B,3,N1), key (B,3,N2) ((B,N,3) with transpose=False) -> int64 (B,N1,max_neighbors): the first keys in
    index order inside the ball, padded with the first of them. key_lengths: (B,) int64 on the keys' device, for a
    padded batch: only the first key_lengths[b] keys of batch element b exist."""
    query, key = _rows(query, key, transpose)
    return ops.pn2_ball_query(query, key, radius, max_neighbors, key_lengths=key_lengths)


def ball_query_distance(query, key, radius, max_neighbors, transpose=True, key_lengths=None):
    """As ball_query, and the squared distances (B,N1,max_neighbors) of the hits (-1 in padded slots)."""
    query, key = _rows(query, key, transpose)
    return ops.pn2_ball_query(query, key, radius, max_neighbors, with_distance=True, key_lengths=key_lengths)
