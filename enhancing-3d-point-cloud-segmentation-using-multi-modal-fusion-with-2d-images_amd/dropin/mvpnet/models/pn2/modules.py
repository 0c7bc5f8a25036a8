"""PointNet++ building blocks of the MVPNet baseline (reference mvpnet/models/pn2/modules.py) on the HIP point ops:
farthest point sampling, ball query, grouping, 3-NN and interpolation are kernels of csrc/pn2.hip / fusion.hip; the
shared 1x1 convolutions, BatchNorm and the max over neighbours stay PyTorch ops, except (a) after freeze_inference, when
a SetAbstraction or FeaturePropagation in eval mode under torch.no_grad() is its point search plus ONE fused launch
(csrc/pn2_mlp.hip), and (b) after fuse_training, when their training-mode shared MLPs run on the library's GEMM and
BatchNorm between the row builder and the max of csrc/pn2_train.hip. Sub-module names match the reference so its
checkpoints load."""
import torch
from torch import nn
import torch.nn.functional as F

try:
    from ....common.nn import SharedMLP, batch_index_select
    from ...ops.fps import farthest_point_sample
    from ...ops.group_points import group_points
    from ...ops.ball_query import ball_query
    from ...ops.knn_distance import knn_distance
    from ...ops.interpolate import feature_interpolate
    from ...._native import ops
except ImportError:
    from common.nn import SharedMLP, batch_index_select
    from mvpnet.ops.fps import farthest_point_sample
    from mvpnet.ops.group_points import group_points
    from mvpnet.ops.ball_query import ball_query
    from mvpnet.ops.knn_distance import knn_distance
    from mvpnet.ops.interpolate import feature_interpolate
    from _native import ops


def _repr(obj, names):
    return ', '.join('{:s}={}'.format(n, getattr(obj, n)) for n in names)


# ---------------------------------------------------------------- frozen inference

def fold_chain(layers, head=None):
    """The packed chain of the fused kernels for a stack of Conv{1,2}dBNReLU layers (and an optional final convolution
    `head` with a bias and no activation): (params, widths) with params = [W0|b0|W1|b1|...] float32 on the layers'
    device, W_l = conv weight * scale row-wise and b_l = conv bias * scale + shift, where scale = gamma / sqrt(running_var
    + eps) and shift = beta - running_mean * scale (computed in float64, stored as float32). None when the stack is not
    one the kernels run: more than three layers, a layer without ReLU or running statistics, a convolution that is not
    1x1, widths outside ops.pn2_mlp_supported."""
    convs = [(m.conv, m.bn, m.relu is not None) for m in layers] + ([(head, None, False)] if head is not None else [])
    if not convs:
        return None
    widths, parts = [convs[0][0].in_channels], []
    for i, (conv, bn, relu) in enumerate(convs):
        last_linear = head is not None and i == len(convs) - 1
        if relu == last_linear or any(k != 1 for k in conv.kernel_size) or conv.groups != 1 \
                or conv.in_channels != widths[-1]:
            return None
        w = conv.weight.detach().double().reshape(conv.out_channels, conv.in_channels)
        b = conv.bias.detach().double() if conv.bias is not None else torch.zeros_like(w[:, 0])
        if bn is not None:
            if bn.running_var is None or bn.running_mean is None:
                return None
            gamma = bn.weight.detach().double() if bn.weight is not None else torch.ones_like(b)
            beta = bn.bias.detach().double() if bn.bias is not None else torch.zeros_like(b)
            scale = gamma / torch.sqrt(bn.running_var.double() + bn.eps)
            shift = beta - bn.running_mean.double() * scale
            w, b = w * scale[:, None], b * scale + shift
        parts += [w.reshape(-1), b]
        widths.append(conv.out_channels)
    if not ops.pn2_mlp_supported(widths):
        return None
    return torch.cat(parts).float().contiguous(), tuple(widths)


class Freezable(object):
    """A module with a frozen inference path. _frozen is a plain attribute (no state-dict key): None, or the snapshot
    that _snapshot() took. train(True) drops it. _freeze_on_request: freeze_inference snapshots the module only when
    asked to by name (FeatureAggregation: aggregation=True)."""
    _frozen = None
    _freeze_on_request = False

    def _snapshot(self):
        raise NotImplementedError

    def _use_frozen(self, *tensors):
        """The snapshot when this forward takes the frozen path: eval mode, gradients off, float32 inputs on the
        snapshot's device."""
        fz = self._frozen
        if fz is None or self.training or torch.is_grad_enabled():
            return None
        if any(t is not None and (t.dtype != torch.float32 or t.device != fz[0].device) for t in tensors):
            return None
        return fz

    def train(self, mode=True):
        if mode:
            self._frozen = None
        return super(Freezable, self).train(mode)


def freeze_inference(net, aggregation=False):
    """Snapshot, for inference, the shared MLPs of every SetAbstraction, FeaturePropagation and PN2SSG under `net` (an
    MVPNet3D is reached through its net_3d): BatchNorm's running statistics folded into the 1x1 convolutions in
    float64, packed as float32 (fold_chain). In eval mode under torch.no_grad() a SetAbstraction with centroids is then
    farthest point sampling, centroid select, ball query and ONE ops.pn2_sa_mlp_max launch (grouping, concatenation,
    the MLP and the max over the neighbours; the (B,C,M,K) tensor is never written), a FeaturePropagation with three
    neighbours is the 3-NN search, the weight arithmetic and ONE ops.pn2_fp_mlp launch, and PN2SSG's mlp_seg + seg_logit
    are one ops.pn2_fp_mlp launch (dropout is the identity in eval mode). In training mode, with gradients enabled, or
    on inputs that are not float32, nothing changes. Modules the kernels do not cover stay as they are: num_centroids
    == 0, num_neighbors == 0, stacks of more than three layers, widths outside ops.pn2_mlp_supported.

    The snapshot is a plain attribute, not a buffer: state-dict keys stay as they are. It is a copy: after
    load_state_dict (or any other change of the parameters or running statistics, or a move to another device) call
    freeze_inference again. train(True) on a module drops its snapshot; unfreeze_inference drops all of them.

    aggregation=True additionally snapshots every FeatureAggregation under `net` (an MVPNet3D's feat_aggreg): its
    shared MLP folded the same way, plus the reduction and relation flags. MVPNet3D.forward then goes from the 2D
    encoder's map to the 3D network's input features in ONE ops.pn2_fa_mlp launch -- no transposed copy of the map, no
    group_points, no concatenation, no Conv2d / BatchNorm2d forward -- under the same conditions (eval mode, gradients
    off, float32). The default leaves FeatureAggregation modules exactly as they are. Returns net."""
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, Freezable) and (aggregation or not m._freeze_on_request):
                m._frozen = m._snapshot()
    return net


def unfreeze_inference(net):
    """Drop every snapshot of freeze_inference. Returns net."""
    for m in net.modules():
        if isinstance(m, Freezable):
            m._frozen = None
    return net


# ---------------------------------------------------------------- fused training

class FusableTraining(object):
    """A module with a fused training path. _fused_training is a plain attribute (no state-dict key) that
    fuse_training / unfuse_training set and clear; the path is taken only where _use_fused_training says so.
    _fuse_on_request: fuse_training sets the attribute only when asked to by name (FeatureAggregation:
    aggregation=True)."""
    _fused_training = False
    _fuse_on_request = False

    def _use_fused_training(self, mlp, *tensors):
        """Whether this forward runs its shared MLP on rows (rows_mlp): fuse_training was called, training mode,
        float32 inputs on the GPU, and a stack whose layers are all 1x1 Conv + BatchNorm (training mode) + ReLU."""
        if not (self._fused_training and self.training):
            return False
        if any(t is not None and (t.dtype != torch.float32 or not t.is_cuda) for t in tensors):
            return False
        return rows_stack(mlp)


def rows_stack(mlp):
    """True for a stack rows_mlp runs: every layer a bias-free 1x1 convolution, an affine BatchNorm in training mode
    and a ReLU."""
    if len(mlp) == 0:
        return False
    for m in mlp:
        conv, bn = getattr(m, 'conv', None), getattr(m, 'bn', None)
        if conv is None or bn is None or getattr(m, 'relu', None) is None:
            return False
        if any(k != 1 for k in conv.kernel_size) or any(s != 1 for s in conv.stride) \
                or any(p != 0 for p in conv.padding) or conv.groups != 1 or conv.bias is not None:
            return False
        if not isinstance(bn, nn.modules.batchnorm._BatchNorm) or not bn.training or bn.weight is None \
                or bn.bias is None:
            return False
    return True


def rows_mlp(mlp, x, transposed, dropout=None):
    """The shared MLP in training mode on rows, FeatureAggregation.forward_fused's loop: x (C, R) channel-major when
    `transposed` (the first product reads it as a transposed operand), else (R, C) -> (R, out_channels). Per layer one
    product on the f32 MFMA GEMM with BatchNorm's column statistics in its epilogue, then ops.bn_lrelu (BatchNorm over
    the R rows -- the statistics of BatchNorm{1,2}d over (B, C, ...) -- and ReLU; running statistics and
    num_batches_tracked are updated by the kernel). dropout: the probability of SharedMLPDO, applied to the rows."""
    rows = x.shape[1] if transposed else x.shape[0]
    n_valid = ops.row_count_for(rows)
    if n_valid is None:
        n_valid = ops.full_count(rows, x.device)
    for layer in mlp:
        w = layer.conv.weight
        x = ops.linear(x, w.view(w.shape[0], w.shape[1]), x_is_transposed=transposed, stats_n_valid=n_valid)
        x = ops.bn_lrelu(x, n_valid, layer.bn, 0.0)
        transposed = False
        if dropout is not None:
            x = F.dropout(x, dropout, True)
    return x


def channel_rows(x):
    """(B, C, N) -> (C, B*N) channel-major, the transposed operand of rows_mlp (one layout copy)."""
    return x.transpose(0, 1).reshape(x.shape[1], -1).contiguous()


def rows_to_channels(x, batch):
    """(B*N, C) rows -> (B, C, N) contiguous (one layout copy)."""
    return x.view(batch, -1, x.shape[1]).transpose(1, 2).contiguous()


def fuse_training(net, aggregation=False):
    """Run the training-mode shared MLPs of every SetAbstraction, FeaturePropagation and PN2SSG under `net` (an MVPNet3D
    is reached through its net_3d) on the library's GEMM and BatchNorm instead of Conv{1,2}d + BatchNorm{1,2}d. A
    SetAbstraction with centroids is then its point search, ops.pn2_sa_rows (the rows of every ball-query group as one
    channel-major operand: neither the grouped (B,C,M,K) tensor nor its concatenation with the coordinates is written),
    per layer ops.linear + ops.bn_lrelu, and ops.pn2_rows_max; a FeaturePropagation with three neighbours and PN2SSG's
    mlp_seg + seg_logit run the same layer loop on (B*N, C) rows. With ops.set_deterministic(True) such a training step
    is bit-reproducible. Taken only in training mode, on float32 GPU inputs, for stacks of 1x1 Conv + BN +
    ReLU; eval mode, the frozen path, num_centroids == 0, num_neighbors == 0, `lengths` and stacks without BatchNorm go
    on as before. A plain attribute, not a buffer: state-dict keys stay as they are. Opt-in and off by default.

    aggregation=True additionally switches every FeatureAggregation under `net` (an MVPNet3D's feat_aggreg), mirroring
    freeze_inference(net, aggregation=True): a training-mode MVPNet3D.forward then goes from the 2D encoder's map to the
    3D network's input features through ops.pn2_fa_rows (the rows of every point's k pixels as one channel-major
    operand, read from the map in place, NCHW or channels-last, with the gradient written back in that format), per
    layer ops.linear + ops.bn_lrelu, and ops.pn2_rows_sum or ops.pn2_rows_max -- no transposed copy of the map, no
    group_points, no concatenation, no Conv2d / BatchNorm2d forward. With ops.set_deterministic(True) everything after
    the 2D encoder is then bit-reproducible. A batch with `lengths`, a module without an MLP and a reduction other
    than sum or max go on as before; the default leaves FeatureAggregation modules exactly as they are. Returns net."""
    for m in net.modules():
        if isinstance(m, FusableTraining) and (aggregation or not m._fuse_on_request):
            m._fused_training = True
    return net


def unfuse_training(net):
    """Back to the PyTorch layers everywhere under `net`. Returns net."""
    for m in net.modules():
        if isinstance(m, FusableTraining):
            m._fused_training = False
    return net


class QueryGrouper(nn.Module):
    """Ball query around every centroid, then the neighbours' coordinates (relative to the centroid) and features."""

    def __init__(self, radius, max_neighbors):
        super(QueryGrouper, self).__init__()
        assert radius > 0.0 and max_neighbors > 0
        self.radius = radius
        self.max_neighbors = max_neighbors

    def forward(self, new_xyz, xyz, feature, use_xyz, key_lengths=None):
        """new_xyz (B,3,M), xyz (B,3,N), feature (B,C,N) or None -> group_feature (B,C[+3],M,K), group_xyz (B,3,M,K).
        key_lengths: (B,) int64 or None; only the first key_lengths[b] columns of xyz[b] are searched."""
        with torch.no_grad():
            index = ball_query(new_xyz, xyz, self.radius, self.max_neighbors, key_lengths=key_lengths)
        group_xyz = group_points(xyz, index) - new_xyz.unsqueeze(-1)
        if feature is None:
            return group_xyz, group_xyz
        group_feature = group_points(feature, index)
        if use_xyz:
            group_feature = torch.cat([group_feature, group_xyz], dim=1)
        return group_feature, group_xyz

    def extra_repr(self):
        return _repr(self, ['radius', 'max_neighbors'])


class SetAbstraction(Freezable, FusableTraining, nn.Module):
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

    def forward(self, xyz, feature=None, lengths=None):
        """xyz (B,3,N), feature (B,C,N) or None -> new_xyz (B,3,M), new_feature (B,out_channels,M). lengths: (B,) int64
        on xyz's device or None, for a padded batch (inference): cloud b is its first lengths[b] columns, centroids
        and neighbours are those of that cloud alone, and all M output columns are valid. It needs num_centroids > 0
        (with 0 or -1 the padding would reach the output)."""
        if lengths is not None and self.num_centroids <= 0:
            raise ValueError('SetAbstraction: lengths needs num_centroids > 0, got {}'.format(self.num_centroids))
        frozen = self._use_frozen(xyz, feature)
        if frozen is not None:
            if self.num_centroids == -1:
                new_xyz = xyz
            else:
                new_xyz = batch_index_select(xyz, farthest_point_sample(xyz, self.num_centroids, lengths=lengths), dim=2)
            index = ball_query(new_xyz, xyz, self.radius, self.max_neighbors, key_lengths=lengths)
            return new_xyz, ops.pn2_sa_mlp_max(xyz.contiguous(), None if feature is None else feature.contiguous(),
                                               new_xyz.contiguous(), index, *frozen)
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
                    index = farthest_point_sample(xyz, self.num_centroids, lengths=lengths)
                new_xyz = batch_index_select(xyz, index, dim=2)
            if lengths is None and self._use_fused_training(self.mlp, xyz, feature):
                return new_xyz, self._forward_rows(xyz, feature, new_xyz)
            group_feature, _ = self.grouper(new_xyz, xyz, feature, use_xyz=self.use_xyz, key_lengths=lengths)
        new_feature = self.mlp(group_feature)
        return new_xyz, torch.max(new_feature, dim=3)[0]

    def _forward_rows(self, xyz, feature, new_xyz):
        """The fused training path after the centroids are chosen (fuse_training): ball query, the group rows as one
        channel-major operand, the shared MLP on rows, the max over each centroid's K rows -> (B,out_channels,M)."""
        with torch.no_grad():
            index = ball_query(new_xyz, xyz, self.radius, self.max_neighbors)
        use_xyz = self.use_xyz or feature is None
        # (coordinates that require a gradient are refused by the op: the rows carry none back to them)
        x = ops.pn2_sa_rows(xyz.contiguous(), None if feature is None else feature.contiguous(), new_xyz.contiguous(),
                            index, use_xyz=use_xyz)
        x = rows_mlp(self.mlp, x, True)
        return ops.pn2_rows_max(x, index.shape[0], index.shape[1], index.shape[2])

    def _snapshot(self):
        return None if self.num_centroids == 0 else fold_chain(self.mlp)

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
        index, weight = self.weights(query_xyz, key_xyz)
        new_feature = feature_interpolate(key_feature, index, weight)
        if query_feature is not None:
            new_feature = torch.cat([new_feature, query_feature], dim=1)
        return new_feature

    def weights(self, query_xyz, key_xyz):
        """The nearest keys of every query and their normalised inverse squared distances: index, weight (B,N1,k)."""
        with torch.no_grad():
            index, distance = knn_distance(query_xyz, key_xyz, self.num_neighbors)
            inv_distance = 1.0 / torch.clamp(distance, min=self._eps)
            weight = inv_distance / torch.sum(inv_distance, dim=2, keepdim=True)
        return index, weight

    def extra_repr(self):
        return _repr(self, ['num_neighbors'])


class FeaturePropagation(Freezable, FusableTraining, nn.Module):
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

    def _snapshot(self):
        return None if self.interpolator is None else fold_chain(self.mlp)

    def forward(self, dense_xyz, sparse_xyz, dense_feature, sparse_feature):
        frozen = self._use_frozen(dense_xyz, sparse_xyz, dense_feature, sparse_feature)
        if frozen is not None:
            index, weight = self.interpolator.weights(dense_xyz, sparse_xyz)
            return ops.pn2_fp_mlp(sparse_feature.contiguous(), index, weight.contiguous(),
                                  None if dense_feature is None else dense_feature.contiguous(), *frozen)
        if self.interpolator is None:
            assert sparse_xyz.size(2) == 1 and sparse_feature.size(2) == 1
            new_feature = torch.cat([sparse_feature.expand(-1, -1, dense_xyz.size(2)), dense_feature], dim=1)
        else:
            new_feature = self.interpolator(dense_xyz, sparse_xyz, dense_feature, sparse_feature)
            if self._use_fused_training(self.mlp, new_feature):
                # two layout copies of a (B,C,N1) tensor in torch around the rows (fuse_training)
                return rows_to_channels(rows_mlp(self.mlp, channel_rows(new_feature), True), new_feature.shape[0])
        return self.mlp(new_feature)
