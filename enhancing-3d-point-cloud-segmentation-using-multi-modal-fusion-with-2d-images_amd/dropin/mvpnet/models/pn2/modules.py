"""PointNet++ building blocks of the MVPNet baseline (reference mvpnet/models/pn2/modules.py) on the HIP point ops:
farthest point sampling, ball query, grouping, 3-NN and interpolation are kernels of csrc/pn2.hip / fusion.hip; the
shared 1x1 convolutions, BatchNorm and the max over neighbours stay PyTorch ops. Sub-module names match the reference
so its checkpoints load."""
import torch
from torch import nn

try:
    from ....common.nn import SharedMLP, batch_index_select
    from ...ops.fps import farthest_point_sample
    from ...ops.group_points import group_points
    from ...ops.ball_query import ball_query
    from ...ops.knn_distance import knn_distance
    from ...ops.interpolate import feature_interpolate
except ImportError:
    from common.nn import SharedMLP, batch_index_select
    from mvpnet.ops.fps import farthest_point_sample
    from mvpnet.ops.group_points import group_points
    from mvpnet.ops.ball_query import ball_query
    from mvpnet.ops.knn_distance import knn_distance
    from mvpnet.ops.interpolate import feature_interpolate


def _repr(obj, names):
    return ', '.join('{:s}={}'.format(n, getattr(obj, n)) for n in names)


class QueryGrouper(nn.Module):
    """Ball query around every centroid, then the neighbours' coordinates (relative to the centroid) and features."""

    def __init__(self, radius, max_neighbors):
        super(QueryGrouper, self).__init__()
        assert radius > 0.0 and max_neighbors > 0
        self.radius = radius
        self.max_neighbors = max_neighbors

    def forward(self, new_xyz, xyz, feature, use_xyz):
        """new_xyz (B,3,M), xyz (B,3,N), feature (B,C,N) or None -> group_feature (B,C[+3],M,K), group_xyz (B,3,M,K)."""
        with torch.no_grad():
            index = ball_query(new_xyz, xyz, self.radius, self.max_neighbors)
        group_xyz = group_points(xyz, index) - new_xyz.unsqueeze(-1)
        if feature is None:
            return group_xyz, group_xyz
        group_feature = group_points(feature, index)
        if use_xyz:
            group_feature = torch.cat([group_feature, group_xyz], dim=1)
        return group_feature, group_xyz

    def extra_repr(self):
        return _repr(self, ['radius', 'max_neighbors'])


class SetAbstraction(nn.Module):
    """PointNet++ set abstraction: sample centroids, group, shared MLP, max over the neighbours.
    num_centroids: 0 = one group around the origin holding every point, -1 = every point is a centroid."""

    def __init__(self, in_channels, mlp_channels, num_centroids, radius, max_neighbors, use_xyz):
        super(SetAbstraction, self).__init__()
        self.in_channels = in_channels
        self.out_channels = mlp_channels[-1]
        self.num_centroids = num_centroids
        self.radius = radius
        self.max_neighbors = max_neighbors
        self.use_xyz = use_xyz
        if self.use_xyz or self.in_channels == 0:
            self.in_channels += 3
        self.mlp = SharedMLP(self.in_channels, mlp_channels, ndim=2, bn=True)
        self.grouper = None if num_centroids == 0 else QueryGrouper(radius, max_neighbors)

    def forward(self, xyz, feature=None):
        """xyz (B,3,N), feature (B,C,N) or None -> new_xyz (B,3,M), new_feature (B,out_channels,M)."""
        if self.num_centroids == 0:
            assert feature is not None
            new_xyz = xyz.new_zeros([xyz.size(0), 3, 1])
            group_feature = feature.unsqueeze(2)
            if self.use_xyz:
                group_feature = torch.cat([group_feature, xyz.unsqueeze(2)], dim=1)
        else:
            if self.num_centroids == -1:
                new_xyz = xyz
            else:
                with torch.no_grad():
                    index = farthest_point_sample(xyz, self.num_centroids)
                new_xyz = batch_index_select(xyz, index, dim=2)
            group_feature, _ = self.grouper(new_xyz, xyz, feature, use_xyz=self.use_xyz)
        new_feature = self.mlp(group_feature)
        return new_xyz, torch.max(new_feature, dim=3)[0]

    def extra_repr(self):
        return _repr(self, ['num_centroids', 'radius', 'max_neighbors', 'use_xyz'])


class FeatureInterpolator(nn.Module):
    """Inverse-squared-distance interpolation from the 3 nearest key points, concatenated with the query's features."""

    def __init__(self, num_neighbors, eps=1e-10):
        super(FeatureInterpolator, self).__init__()
        self.num_neighbors = num_neighbors
        self._eps = eps

    def forward(self, query_xyz, key_xyz, query_feature, key_feature):
        """query_xyz (B,3,N1), key_xyz (B,3,N2), query_feature (B,C1,N1) or None, key_feature (B,C2,N2)
        -> (B,C2+C1,N1)."""
        with torch.no_grad():
            index, distance = knn_distance(query_xyz, key_xyz, self.num_neighbors)
            inv_distance = 1.0 / torch.clamp(distance, min=self._eps)
            weight = inv_distance / torch.sum(inv_distance, dim=2, keepdim=True)
        new_feature = feature_interpolate(key_feature, index, weight)
        if query_feature is not None:
            new_feature = torch.cat([new_feature, query_feature], dim=1)
        return new_feature

    def extra_repr(self):
        return _repr(self, ['num_neighbors'])


class FeaturePropagation(nn.Module):
    """PointNet++ feature propagation: interpolate the sparse level's features onto the dense level (num_neighbors 3),
    or broadcast a single global feature (num_neighbors 0), then a shared MLP."""

    def __init__(self, in_channels, in_channels_prev, mlp_channels, num_neighbors):
        super(FeaturePropagation, self).__init__()
        self.in_channels = in_channels + in_channels_prev
        self.out_channels = mlp_channels[-1]
        self.mlp = SharedMLP(self.in_channels, mlp_channels, ndim=1, bn=True)
        if num_neighbors == 0:
            self.interpolator = None
        elif num_neighbors == 3:
            self.interpolator = FeatureInterpolator(num_neighbors)
        else:
            raise ValueError('Expected value 3, but {} given.'.format(num_neighbors))

    def forward(self, dense_xyz, sparse_xyz, dense_feature, sparse_feature):
        if self.interpolator is None:
            assert sparse_xyz.size(2) == 1 and sparse_feature.size(2) == 1
            new_feature = torch.cat([sparse_feature.expand(-1, -1, dense_xyz.size(2)), dense_feature], dim=1)
        else:
            new_feature = self.interpolator(dense_xyz, sparse_xyz, dense_feature, sparse_feature)
        return self.mlp(new_feature)
