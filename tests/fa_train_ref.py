"""NumPy restatement of the training-mode FeatureAggregation kernels (csrc/pn2_rows.hip), own text.

The map is (B*nv, C, h, w); a flat pixel index p = view*h*w + pixel of batch element b selects image b*nv + view. Rows:
R = B*np*k, row r = (b*np + n)*k + j. `fa_rows` builds the channel-major operand X (C [+4], R) in the dtype of its
inputs: a gather, ONE rounded subtraction per coordinate, and the squared distance as (dx*dx + dy*dy) + dz*dz with every
product and sum rounded. `fa_rows_bwd` is its transpose onto the map, per pixel the sum of its positions' values in
ascending position with every addition rounded (np.add.at over the natural order, tests/pn2_ordered_ref.py). `rows_sum`
adds a point's k rows in ascending j, starting from the first row's value, and `rows_sum_bwd` copies the gradient into
each of them.
"""
import numpy as np

from pn2_ordered_ref import _ordered, flat_index


def pixel_planes(fmap, b):
    """(B*nv, C, h, w) -> (B, C, nv*h*w): batch element b's pixels in flat-index order."""
    bnv, c, h, w = fmap.shape
    nv = bnv // b
    return np.ascontiguousarray(fmap.reshape(b, nv, c, h * w).transpose(0, 2, 1, 3)).reshape(b, c, nv * h * w)


def map_from_planes(planes, nv, h, w):
    """(B, C, nv*h*w) -> (B*nv, C, h, w)."""
    b, c, _ = planes.shape
    return np.ascontiguousarray(planes.reshape(b, c, nv, h * w).transpose(0, 2, 1, 3)).reshape(b * nv, c, h, w)


def fa_rows(fmap, image_xyz, points, index, use_relation=True):
    """fmap (B*nv,C,h,w), image_xyz (B,nv,h,w,3), points (B,3,np), index (B,np,k) -> X (C [+4], B*np*k): the column of
    (b, n, j) is [fmap at pixel p | d | (d.x*d.x + d.y*d.y) + d.z*d.z], p = index[b, n, j], d = image_xyz[b, p] -
    points[b, :, n]; an index outside [0, nv*h*w) reads as zero before the point is subtracted."""
    b, nv, h, w, _ = image_xyz.shape
    p_all = nv * h * w
    ok = (index >= 0) & (index < p_all)
    j = np.where(ok, index, 0)
    planes = pixel_planes(fmap, b)
    parts = [np.stack([np.where(ok[bi][None], planes[bi][:, j[bi]], fmap.dtype.type(0)) for bi in range(b)], 1)]
    if use_relation:
        xyz = image_xyz.reshape(b, p_all, 3)
        g = np.stack([np.where(ok[bi][..., None], xyz[bi][j[bi]], xyz.dtype.type(0)) for bi in range(b)])   # (B,np,k,3)
        d = g - np.transpose(points, (0, 2, 1))[:, :, None, :]
        dist = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        parts += [np.transpose(d, (3, 0, 1, 2)), dist[None]]
    x = np.concatenate(parts, 0)
    return np.ascontiguousarray(x.reshape(x.shape[0], -1))


def _values(dx, index, c):
    b = index.shape[0]
    return np.ascontiguousarray(np.transpose(dx[:c].reshape(c, b, -1), (1, 0, 2)))


def fa_rows_bwd(dx, index, c, nv, h, w):
    """dX (C [+4], R), index (B,np,k) -> the map's gradient (B*nv,c,h,w) in dX's dtype: per pixel the sum of its
    positions' values in ascending position, rounded after every addition; rows c.. of dX are not read."""
    return map_from_planes(_ordered(_values(dx, index, c), flat_index(index), nv * h * w), nv, h, w)


def fa_rows_bwd_wide(dx, index, c, nv, h, w):
    """The same sums in float64 with, per element, the sum of the absolute contributions, and per pixel the number of
    contributions (B*nv,1,h,w): what the bound (T + 1) u sum|g| of the atomic form needs."""
    p_all = nv * h * w
    values, ix = _values(dx, index, c).astype(np.float64), flat_index(index)
    count = np.stack([np.bincount(r[(r >= 0) & (r < p_all)], minlength=p_all)[:p_all] for r in ix])
    return (map_from_planes(_ordered(values, ix, p_all), nv, h, w),
            map_from_planes(_ordered(np.abs(values), ix, p_all), nv, h, w),
            map_from_planes(count[:, None, :], nv, h, w))


def rows_sum(y, b, m, k):
    """y (B*M*K, Cout) -> (B,Cout,M): the first row, then one rounded addition per further row in ascending k."""
    t = y.reshape(b, m, k, y.shape[1])
    acc = t[:, :, 0].copy()
    for j in range(1, k):
        acc = acc + t[:, :, j]
    return np.ascontiguousarray(acc.transpose(0, 2, 1))


def rows_sum_bwd(g, k):
    """g (B,Cout,M) -> dY (B*M*K, Cout): g[b, :, m] in each of the point's k rows."""
    b, cout, m = g.shape
    return np.ascontiguousarray(np.broadcast_to(g.transpose(0, 2, 1)[:, :, None, :], (b, m, k, cout))).reshape(b * m * k, cout)
