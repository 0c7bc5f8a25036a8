"""``scene2chunks_legacy`` with the reference's signature (mvpnet/utils/chunk_util.py:4-53) on the HIP kernels of
csrc/chunk.hip. The reference loops over the chunk corners in Python and builds two full-N boolean masks per corner;
here the corners and box bounds are still computed on the host, with the reference's own expressions (so they follow
the installed NumPy's promotion rules exactly as the reference's would), and the scene stays in HBM: one launch counts
the points of every inner and widened box, a second set of launches writes the kept chunks' indices as one CSR.

What comes back to the host per scene: the scene's float32 minimum and maximum (six floats), the 2 n corner counts and,
with return_bbox, the kept chunks' z ranges (2 floats each). Nothing sized by the number of points."""
import numpy as np
import torch

try:
    from ..._native import ops
except ImportError:
    from _native import ops


def scene2chunks_legacy(points, chunk_size, stride, thresh=1000, margin=(0.2, 0.2), return_bbox=False):
    """Sliding chunks of a scene on the xy-plane (the z axis is never cut).

    points: (N, 3) float32, a tensor in HBM or a NumPy array (uploaded for the call). chunk_size, margin: two numbers
    each (x, y); stride: one number. A corner is kept when its chunk_size box holds at least `thresh` points; the chunk
    is then every point of that box widened by `margin` on all four sides.

    Returns the list of the kept chunks' point indices, int64 and ascending: for a tensor input they are views of one
    buffer in HBM, for a NumPy input NumPy arrays, as in the reference. With return_bbox also the list of their boxes,
    float64 arrays (x_lo, y_lo, z_lo, x_hi, y_hi, z_hi) with the z range of the chunk's own points."""
    from_host = not isinstance(points, torch.Tensor)
    if from_host:
        points = np.asarray(points)
        if points.dtype != np.float32:
            raise TypeError("scene2chunks_legacy: float32 points expected (the reference's dataset casts them), got %s"
                            % points.dtype)
        points = torch.from_numpy(np.ascontiguousarray(points)).cuda()
    elif points.dtype != torch.float32:
        raise TypeError("scene2chunks_legacy: float32 points expected, got %s" % points.dtype)
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError("scene2chunks_legacy: points (num_points, 3) expected")
    if points.shape[0] == 0:
        raise ValueError("scene2chunks_legacy: an empty scene has no extent")
    points = points.contiguous()
    nothing = ([], []) if return_bbox else []

    # The corner grid, from the scene's float32 extremes (one six-float read). The expressions are evaluated by the
    # installed NumPy on float32 scalars and the caller's Python numbers, exactly as the reference evaluates its own, so
    # the corners have the dtype (and the roundings) they have there.
    size, pad = np.asarray(chunk_size), np.asarray(margin)
    bottom, top = torch.stack([points.amin(0), points.amax(0)]).cpu().numpy()
    span = top - bottom
    per_axis = np.ceil((span[:2] - size) / stride).astype(int) + 1      # zero or negative: scene smaller than a chunk
    corners = [np.asarray((bottom[0] + ix * stride, bottom[1] + iy * stride))
               for ix in range(per_axis[0]) for iy in range(per_axis[1])]
    n = len(corners)
    if n == 0:
        return nothing

    # (x_lo, y_lo, x_hi, y_hi) without and with the margin, widened exactly to float64 for the device
    inner = np.array([np.hstack([c, c + size]) for c in corners], np.float64)
    outer = np.array([np.hstack([c - pad, c + size + pad]) for c in corners], np.float64)
    counts = ops.box_count(points, np.concatenate([inner, outer])).cpu().numpy()          # the 2 n counts: second read
    kept = np.nonzero(counts[:n] >= thresh)[0]
    if kept.size == 0:
        return nothing
    sizes = counts[n:][kept]
    if return_bbox and (sizes == 0).any():
        raise ValueError("scene2chunks_legacy: a kept chunk without points has no z range (thresh <= 0?)")
    _, flat, z_lo, z_hi = ops.box_select(points, outer[kept], sizes, with_z=return_bbox)
    cuts = np.concatenate([[0], np.cumsum(sizes)]).tolist()
    if from_host:
        flat = flat.cpu().numpy()
    chunk_indices = [flat[cuts[k]:cuts[k + 1]] for k in range(kept.size)]
    if not return_bbox:
        return chunk_indices
    z = torch.stack([z_lo, z_hi]).cpu().numpy()                                           # two floats per chunk: third read
    chunk_bboxes = [np.hstack([corners[c] - pad, z[0, k], corners[c] + size + pad, z[1, k]]) for k, c in enumerate(kept)]
    return chunk_indices, chunk_bboxes
