"""NumPy restatement of the fused FeatureAggregation kernel (pn2_fa_k of csrc/pn2_mlp.hip): gather the 2D encoder's map
by flat pixel index, append the relation channels [diff_xyz | squared distance], run the affine chain with ReLU, reduce
over the k neighbours, zero the columns behind `lengths`. Everything is computed in `dtype` (the tests feed float64)."""
import numpy as np

from pn2_frozen_ref import chain, unpack


def fa_rows(feature_2d, image_xyz, points, index, use_relation=True):
    """The input rows of ONE batch element. feature_2d [nv,C,h,w], image_xyz [nv,h,w,3], points [3,N], index [N,K] flat
    pixel indices view * h * w + pixel -> [N,K,C(+4)]. An index outside [0, nv * h * w) reads as zero for the features and
    for image_xyz BEFORE the point is subtracted (group_points, then the subtraction)."""
    nv, c, h, w = feature_2d.shape
    p = nv * h * w
    ok = (index >= 0) & (index < p)
    j = np.where(ok, index, 0)
    flat = feature_2d.transpose(0, 2, 3, 1).reshape(p, c)                       # [P,C], pixel-major
    feat = np.where(ok[..., None], flat[j], 0)                                  # [N,K,C]
    if not use_relation:
        return feat
    xyz = np.where(ok[..., None], image_xyz.reshape(p, 3)[j], 0)                # [N,K,3]
    diff = xyz - points.T[:, None, :]
    dist = (diff[..., 0] * diff[..., 0] + diff[..., 1] * diff[..., 1]) + diff[..., 2] * diff[..., 2]
    return np.concatenate([feat, diff, dist[..., None]], axis=2)


def fa_mlp(feature_2d, image_xyz, points, index, params, widths, reduction="sum", use_relation=True, lengths=None,
           dtype=np.float64):
    """feature_2d [B*nv,C,h,w], image_xyz [B,nv,h,w,3], points [B,3,N], index [B,N,K] -> [B,Cout,N]: the sum over k in
    ascending order from the k = 0 value (or the maximum) of the chain's ReLU outputs; columns >= clamp(lengths[b], 1, N)
    are zeros, whatever their points and indices hold."""
    layers = unpack(params, widths, dtype)
    b, nv = image_xyz.shape[:2]
    n, k = index.shape[1:]
    feature_2d = np.asarray(feature_2d, dtype).reshape((b, nv) + feature_2d.shape[1:])
    image_xyz, points = np.asarray(image_xyz, dtype), np.asarray(points, dtype)
    out = np.zeros((b, widths[-1], n), dtype)
    for i in range(b):
        nb = n if lengths is None else int(min(max(int(lengths[i]), 1), n))
        rows = fa_rows(feature_2d[i], image_xyz[i], points[i][:, :nb], np.asarray(index[i][:nb]), use_relation)
        assert rows.shape[2] == widths[0]
        y = chain(rows, layers)                                                 # [nb,K,Cout]
        if reduction == "max":
            acc = y.max(1)
        else:
            acc = y[:, 0].copy()
            for kk in range(1, k):
                acc = acc + y[:, kk]
        out[i, :, :nb] = acc.T
    return out
