"""``knn_distance`` with the reference's signature (mvpnet/ops/knn_distance.py:16-37) on the HIP kernel
(csrc/pn2.hip)."""
try:
    from ..._native import ops
except ImportError:
    from _native import ops


def knn_distance(query, key, k, transpose=True):
    """For each query point the k = 3 nearest keys.

    Args:
        query: (B, 3, N1); (B, N1, 3) with transpose=False
        key: (B, 3, N2); (B, N2, 3) with transpose=False
        k (int): 3 (the only value the reference's extension accepts)
    Returns:
        index (B, N1, K) int64 and squared distance (B, N1, K), ascending, both without grad
    """
    if transpose:
        query, key = query.transpose(1, 2), key.transpose(1, 2)
    return ops.knn_distance(query.contiguous(), key.contiguous(), k)
