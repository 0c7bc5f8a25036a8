"""``feature_interpolate`` with the reference's signature and autograd behaviour (mvpnet/ops/interpolate.py:5-35)
on the HIP gather / scatter-add kernels (csrc/pn2.hip)."""
try:
    from ..._native import ops
except ImportError:
    from _native import ops


def feature_interpolate(feature, index, weight):
    """feature (B,C,N1) of the key points, index (B,N2,K) int64, weight (B,N2,K) -> (B,C,N2); K = 3."""
    return ops.feature_interpolate(feature, index, weight)
