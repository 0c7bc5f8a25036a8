"""``farthest_point_sample`` with the reference's signature (mvpnet/ops/fps.py:16-31) on the HIP kernel
(csrc/pn2.hip): same centroids as the reference's extension, ties included."""
try:
    from ..._native import ops
except ImportError:
    from _native import ops


def farthest_point_sample(points, num_centroids, transpose=True, lengths=None):
    """Farthest point sample.

    Args:
        points (torch.Tensor): (batch_size, 3, num_points); (batch_size, num_points, 3) with transpose=False
        num_centroids (int): the number of centroids to sample
        transpose (bool): whether to transpose points
        lengths (torch.Tensor, optional): (batch_size,) int64 on the points' device, for a padded batch: cloud b is its
            first lengths[b] points, the rest is never read, and row b of the result is the sample of that cloud alone
    Returns:
        torch.Tensor: (batch_size, num_centroids) int64 indices of the centroids, without grad
    """
    if transpose:
        points = points.transpose(1, 2)
    return ops.fps(points.contiguous(), num_centroids, lengths=lengths)
