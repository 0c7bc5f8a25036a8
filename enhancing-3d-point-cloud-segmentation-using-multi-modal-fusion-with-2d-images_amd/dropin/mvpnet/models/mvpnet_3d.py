"""FeatureAggregation (reference mvpnet/models/mvpnet_3d.py:12-70): per (point, neighbour) feature
[feat_2d | dxyz | |dxyz|^2] -> SharedMLP (1x1 conv + BN + ReLU) -> reduction over k.
Sub-module names (mlp.{i}.conv / mlp.{i}.bn) match the reference so MVPNet checkpoints load.
MVPNet3D (reference :73-135): the baseline's wiring 2D encoder -> unprojection by group_points ->
FeatureAggregation -> 3D network (PN2SSG). After freeze_inference(net, aggregation=True) (pn2/modules.py) the
unprojection and the aggregation of an eval-mode forward under torch.no_grad() are ONE fused launch on the encoder's
map (ops.pn2_fa_mlp, csrc/pn2_mlp.hip). After fuse_training(net, aggregation=True) a training-mode forward runs them on
that map through ops.pn2_fa_rows, the library's GEMM and BatchNorm and ops.pn2_rows_sum / pn2_rows_max
(csrc/fa_train.hip), with the map's gradient written in the map's own memory format."""
import logging

import numpy as np
import torch
from torch import nn
import torch.nn.functional as F

try:
    from ...common.nn import SharedMLP, xavier_uniform
    from ..._native import ops
except ImportError:
    from common.nn import SharedMLP, xavier_uniform
    from _native import ops
from .pn2.modules import Freezable, FusableTraining, fold_chain, rows_mlp


class FeatureAggregation(Freezable, FusableTraining, nn.Module):
    """Feature Aggregation inspired by ContFuse. After freeze_inference(net, aggregation=True) it holds a snapshot
    (params, widths, reduction name, use_relation) -- a plain attribute, no state-dict key, dropped by train(True) --
    and from_encoder_map runs the whole module, grouping included, as one fused launch. After
    fuse_training(net, aggregation=True) forward_rows runs it in training mode for a batch, grouping included, on the
    library's row builder, GEMM, BatchNorm and reduction (csrc/fa_train.hip)."""
    _freeze_on_request = True
    _fuse_on_request = True

    def __init__(self, in_channels, mlp_channels=(64, 64, 64), reduction='sum', use_relation=True):
        super(FeatureAggregation, self).__init__()
        self.in_channels = in_channels
        self.use_relation = use_relation
        if mlp_channels:
            self.out_channels = mlp_channels[-1]
            self.mlp = SharedMLP(in_channels + (4 if use_relation else 0), mlp_channels, ndim=2, bn=True)
        else:
            self.out_channels = in_channels
            self.mlp = None
        if reduction == 'sum':
            self.reduction = torch.sum
        elif reduction == 'max':
            self.reduction = lambda x, dim: torch.max(x, dim)[0]
        self._reduction_name = reduction if reduction in ('sum', 'max') else None
        self.reset_parameters()

    def _snapshot(self):
        """fold_chain of the shared MLP plus the two flags, or None where the fused kernel does not apply: no MLP,
        more than three layers, unsupported widths."""
        if self.mlp is None or self._reduction_name is None:
            return None
        chain = fold_chain(self.mlp)
        return None if chain is None else chain + (self._reduction_name, bool(self.use_relation))

    def from_encoder_map(self, frozen, feature_2d, image_xyz, knn_indices, points, lengths=None):
        """The frozen module on the encoder's output as it lies: feature_2d (b*nv,c,h,w) contiguous or channels-last,
        image_xyz (b,nv,h,w,3), knn_indices (b,np,k) int64 flat pixel indices, points (b,3,np) -> (b,out,np), what
        forward() gives on the two group_points results. frozen: the snapshot _use_frozen returned. One launch
        (ops.pn2_fa_mlp); columns >= lengths[b] come out as zeros."""
        params, widths, reduction, use_relation = frozen
        if not (feature_2d.is_contiguous() or feature_2d.is_contiguous(memory_format=torch.channels_last)):
            feature_2d = feature_2d.contiguous()
        return ops.pn2_fa_mlp(feature_2d, image_xyz.contiguous(), points.contiguous(), knn_indices.contiguous(), params,
                              widths, reduction=reduction, use_relation=use_relation, lengths=lengths)

    def _use_rows(self, feature_2d, image_xyz, points):
        """Whether a training-mode batch takes forward_rows: fuse_training(net, aggregation=True) was called, training
        mode, float32 GPU inputs, an MLP of 1x1 Conv + BatchNorm + ReLU layers, sum or max over k."""
        if self.mlp is None or self._reduction_name is None:
            return False
        return self._use_fused_training(self.mlp, feature_2d, image_xyz, points)

    def forward_rows(self, feature_2d, image_xyz, knn_indices, points):
        """The module in training mode on the encoder's output as it lies (fuse_training(net, aggregation=True)):
        feature_2d (b*nv,c,h,w) contiguous or channels-last, image_xyz (b,nv,h,w,3), knn_indices (b,np,k) int64 flat
        pixel indices, points (b,3,np) -> (b,out,np), what forward() gives on the two group_points results. The rows of
        every (point, pixel) pair as one channel-major operand (ops.pn2_fa_rows: no transposed copy of the map, no
        grouped tensor, no concatenation), the shared MLP on rows (ops.linear + ops.bn_lrelu, BatchNorm over the
        b*np*k rows: BatchNorm2d's statistics over (b,C,np,k)), then the sum or max over each point's k rows. The
        gradient reaches feature_2d alone, in its memory format."""
        if self.mlp is None or self._reduction_name is None:
            raise RuntimeError("forward_rows needs an MLP and a sum or max reduction")
        if not (feature_2d.is_contiguous() or feature_2d.is_contiguous(memory_format=torch.channels_last)):
            feature_2d = feature_2d.contiguous()
        index = knn_indices if knn_indices.is_contiguous() else knn_indices.contiguous()
        x = ops.pn2_fa_rows(feature_2d, image_xyz.contiguous(), points.contiguous(), index,
                            use_relation=bool(self.use_relation))
        x = rows_mlp(self.mlp, x, True)
        b, n_pts, k = index.shape
        if self._reduction_name == 'sum':
            return ops.pn2_rows_sum(x, b, n_pts, k)
        return ops.pn2_rows_max(x, b, n_pts, k)

    def forward(self, src_xyz, tgt_xyz, feature):
        """src_xyz (b,3,np,k), tgt_xyz (b,3,np), feature (b,c,np,k) -> (b,out,np)."""
        if self.mlp is None:
            return self.reduction(feature, 3)
        x = feature
        if self.use_relation:
            diff_xyz = src_xyz - tgt_xyz.unsqueeze(-1)
            distance = torch.sum(diff_xyz ** 2, dim=1, keepdim=True)
            x = torch.cat([feature, diff_xyz, distance], dim=1)
        return self.reduction(self.mlp(x), 3)

    def forward_fused(self, feature_2d, image_xyz, knn, points):
        """Same function as forward() fed by the two group_points calls of the network
        (architectures_sphere.py:266-284), for ONE sphere and without materialising the grouped tensors:
        one HIP gather kernel builds the (C+4, np*k) MLP input straight from the encoder's (nv,C,h,w)
        feature map, the three 1x1 convolutions run on the f32 MFMA GEMM over rows, BatchNorm over the
        np*k rows (identical statistics to BatchNorm2d over (1,C,np,k)), sum over k.
        feature_2d (nv,C,h,w), image_xyz (nv,h,w,3), knn (np,k) int64, points (np,3) -> (np, out)."""
        if self.mlp is None or not self.use_relation or self.reduction is not torch.sum:
            raise RuntimeError("forward_fused covers the MV-KPConv configuration (relation features, MLP, sum)")
        n_pts, k = knn.shape
        x = ops.fa_gather(feature_2d, image_xyz, knn, points)           # [C+4, np*k] channel-major
        transposed = True
        for layer in self.mlp:
            w = layer.conv.weight
            bn = layer.bn
            rows = x.shape[1] if transposed else x.shape[0]
            if bn.training:   # HIP BatchNorm + ReLU over the np*k rows (all valid unless the level is capacity padded);
                n_valid = ops.row_count_for(rows)          # its column statistics come out of the GEMM's epilogue
                if n_valid is None:
                    n_valid = ops.full_count(rows, x.device)
                x = ops.linear(x, w.view(w.shape[0], w.shape[1]), x_is_transposed=transposed, stats_n_valid=n_valid)
                x = ops.bn_lrelu(x, n_valid, bn, 0.0)
                transposed = False
                continue
            x = ops.linear(x, w.view(w.shape[0], w.shape[1]), x_is_transposed=transposed)   # [np*k, out]
            transposed = False
            x = F.relu(F.batch_norm(x, bn.running_mean, bn.running_var, bn.weight, bn.bias, False, bn.momentum, bn.eps))
        return x.view(n_pts, k, -1).sum(dim=1)

    def reset_parameters(self):
        for m in self.modules():
            if isinstance(m, (nn.Conv1d, nn.Conv2d, nn.Linear)):
                xavier_uniform(m)


_log = logging.getLogger(__name__)


def _load_encoder_weights(net_2d, path):
    """The 'model' entry of a training checkpoint of the 2D network, read on the host."""
    state = torch.load(path, map_location="cpu")['model']
    net_2d.load_state_dict(state)
    _log.info("MVPNet3D: 2D encoder weights (%d tensors) taken from %s", len(state), path)


class MVPNet3D(nn.Module):
    """net_2d: a module mapping {'image': (b*nv,3,h,w)} to {'feature': (b*nv,c,h,w)}; net_2d_ckpt_path: a checkpoint
    whose 'model' entry is loaded into it (or a false value); net_3d: a module taking {'points', 'feature'}
    (PN2SSG); feat_aggr_kwargs: the arguments of FeatureAggregation."""

    def __init__(self, net_2d, net_2d_ckpt_path, net_3d, **feat_aggr_kwargs):
        super(MVPNet3D, self).__init__()
        if net_2d_ckpt_path:
            _load_encoder_weights(net_2d, net_2d_ckpt_path)
        # registration order (net_2d, feat_aggreg, net_3d) fixes the order of the state-dict keys
        self.net_2d = net_2d
        self.feat_aggreg = FeatureAggregation(**feat_aggr_kwargs)
        self.net_3d = net_3d

    def forward(self, data_batch):
        """images (b,nv,3,h,w), image_xyz (b,nv,h,w,3), knn_indices (b,np,k) int64 flat pixel indices
        view*h*w + row*w + col, points (b,3,np) -> the 3D network's predictions. An optional 'lengths' (b,) int64 goes
        through to net_3d (PN2SSG.forward: a padded batch at inference); the padded rows of knn_indices must be valid
        pixel indices (0 will do), and the logit columns >= lengths[b] of batch element b are unspecified."""
        images = data_batch['images']
        b, nv, _, h, w = images.size()
        feature_2d = self.net_2d({'image': images.reshape([-1] + list(images.shape[2:]))})['feature']
        knn_indices = data_batch['knn_indices']
        frozen = self.feat_aggreg._use_frozen(feature_2d, data_batch['image_xyz'], data_batch['points'])
        if frozen is not None and not self.training and knn_indices.shape[2] <= 128:
            # the 2D -> 3D hand-off as one launch on the encoder's map (freeze_inference(net, aggregation=True))
            points = data_batch['points']
            lengths = data_batch.get('lengths', None)
            batch_3d = {'points': points,
                        'feature': self.feat_aggreg.from_encoder_map(frozen, feature_2d, data_batch['image_xyz'],
                                                                     knn_indices, points, lengths=lengths)}
            if lengths is not None:
                batch_3d['lengths'] = lengths
            return self.net_3d(batch_3d)
        if data_batch.get('lengths', None) is None \
                and self.feat_aggreg._use_rows(feature_2d, data_batch['image_xyz'], data_batch['points']):
            # the hand-off in training mode on the encoder's map (fuse_training(net, aggregation=True)); BatchNorm over
            # the padded rows of a `lengths` batch would be another function, so that case goes on below
            points = data_batch['points']
            return self.net_3d({'points': points,
                                'feature': self.feat_aggreg.forward_rows(feature_2d, data_batch['image_xyz'],
                                                                         knn_indices, points)})
        feature_2d = feature_2d.reshape(b, nv, -1, h, w).transpose(1, 2).contiguous().reshape(b, -1, nv * h * w)
        feature_2d = ops.group_points(feature_2d, knn_indices)                     # (b, c, np, k)
        with torch.no_grad():
            image_xyz = data_batch['image_xyz'].permute(0, 4, 1, 2, 3).reshape(b, 3, nv * h * w)
            image_xyz = ops.group_points(image_xyz, knn_indices)                   # (b, 3, np, k)
        points = data_batch['points']
        feature_2d3d = self.feat_aggreg(image_xyz, points, feature_2d)             # (b, out, np)
        batch_3d = {'points': points, 'feature': feature_2d3d}
        if data_batch.get('lengths', None) is not None:
            batch_3d['lengths'] = data_batch['lengths']
        return self.net_3d(batch_3d)

    def get_loss(self, cfg):
        from mvpnet.models.loss import SegLoss
        weights = None
        if cfg.TRAIN.LABEL_WEIGHTS_PATH:
            weights = torch.from_numpy(np.loadtxt(cfg.TRAIN.LABEL_WEIGHTS_PATH, dtype=np.float32)).cuda()
        return SegLoss(weight=weights)

    def get_metric(self, cfg):
        from mvpnet.models.metric import SegAccuracy, SegIoU
        make = lambda: [SegAccuracy(), SegIoU(self.net_3d.num_classes)]
        return make(), make()
