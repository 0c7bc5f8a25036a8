"""PointNet++ with single-scale grouping, the 3D network of the MVPNet baseline (reference
mvpnet/models/pn2/pn2ssg.py; Qi et al., arXiv:1706.02413). Constructor arguments, defaults and sub-module names
(sa_modules.N.mlp.M.conv, fp_modules, mlp_seg, seg_logit) are the reference's, so its checkpoints load.
freeze_inference / unfreeze_inference (modules.py) switch the fused inference forward on and off, fuse_training /
unfuse_training the training-mode shared MLPs on the library's GEMM and BatchNorm."""
import numpy as np
import torch
from torch import nn

try:
    from ....common.nn import SharedMLPDO, xavier_uniform
    from .modules import (SetAbstraction, FeaturePropagation, Freezable, FusableTraining, fold_chain, freeze_inference,
                          unfreeze_inference, fuse_training, unfuse_training, rows_mlp, channel_rows, rows_to_channels)
    from ...._native import ops
except ImportError:
    from common.nn import SharedMLPDO, xavier_uniform
    from mvpnet.models.pn2.modules import (SetAbstraction, FeaturePropagation, Freezable, FusableTraining, fold_chain,
                                           freeze_inference, unfreeze_inference, fuse_training, unfuse_training,
                                           rows_mlp, channel_rows, rows_to_channels)
    from _native import ops


class PN2SSG(Freezable, FusableTraining, nn.Module):
    def __init__(self,
                 in_channels,
                 num_classes,
                 sa_channels=((32, 32, 64), (64, 64, 128), (128, 128, 256), (256, 256, 512)),
                 num_centroids=(2048, 512, 128, 32),
                 radius=(0.1, 0.2, 0.4, 0.8),
                 max_neighbors=(32, 32, 32, 32),
                 fp_channels=((256, 256), (256, 256), (256, 128), (128, 128, 128)),
                 fp_neighbors=(3, 3, 3, 3),
                 seg_channels=(128,),
                 dropout_prob=0.5,
                 use_xyz=True):
        super(PN2SSG, self).__init__()
        self.in_channels = in_channels
        self.num_classes = num_classes
        self.use_xyz = use_xyz
        levels = len(sa_channels)
        assert len(num_centroids) == levels and len(radius) == levels and len(max_neighbors) == levels
        assert len(fp_channels) == levels and len(fp_neighbors) == levels

        self.sa_modules = nn.ModuleList()
        c_in = in_channels
        for lv in range(levels):
            self.sa_modules.append(SetAbstraction(in_channels=c_in, mlp_channels=sa_channels[lv],
                                                  num_centroids=num_centroids[lv], radius=radius[lv],
                                                  max_neighbors=max_neighbors[lv], use_xyz=use_xyz))
            c_in = sa_channels[lv][-1]

        # widths of the encoder's feature maps, finest first; the input features are not propagated (width 0)
        widths = [0] + [ch[-1] for ch in sa_channels]
        self.fp_modules = nn.ModuleList()
        c_in = widths[-1]
        for lv in range(levels):
            self.fp_modules.append(FeaturePropagation(in_channels=c_in, in_channels_prev=widths[-2 - lv],
                                                      mlp_channels=fp_channels[lv], num_neighbors=fp_neighbors[lv]))
            c_in = fp_channels[lv][-1]

        self.mlp_seg = SharedMLPDO(fp_channels[-1][-1], seg_channels, ndim=1, bn=True, p=dropout_prob)
        self.seg_logit = nn.Conv1d(seg_channels[-1], num_classes, 1, bias=True)
        self.reset_parameters()

    def forward(self, data_batch):
        """data_batch['points'] (B,3,N), optional data_batch['feature'] (B,C,N) -> {'seg_logit': (B,num_classes,N)}.
        Optional data_batch['lengths'] (B,) int64 on the points' device, inference only: a padded batch of clouds of
        different sizes. Cloud b is the first lengths[b] columns; the first set abstraction samples and groups within
        them, so the logit columns [0, lengths[b]) of batch element b are those of a forward of that cloud alone. The
        logit columns >= lengths[b] are unspecified. Raises ValueError when the first set abstraction has
        num_centroids <= 0 (the next level would be ragged) and RuntimeError in training mode (batch statistics would
        include the padded columns)."""
        xyz = data_batch['points']
        feature = data_batch.get('feature', None)
        lengths = data_batch.get('lengths', None)
        if lengths is not None:
            if self.sa_modules[0].num_centroids <= 0:
                raise ValueError('PN2SSG: lengths needs num_centroids[0] > 0, got {}'.format(
                    self.sa_modules[0].num_centroids))
            if self.training:
                raise RuntimeError('PN2SSG: lengths is for inference; call eval() first')
        xyzs, feats = [xyz], [None]
        for lv, sa in enumerate(self.sa_modules):
            xyz, feature = sa(xyz, feature) if lv > 0 or lengths is None else sa(xyz, feature, lengths=lengths)
            xyzs.append(xyz)
            feats.append(feature)
        up = feats[-1]
        for lv, fp in enumerate(self.fp_modules):
            up = fp(xyzs[-2 - lv], xyzs[-1 - lv], feats[-2 - lv], up)
        frozen = self._use_frozen(up)
        if frozen is not None:      # mlp_seg + seg_logit in one launch; dropout is the identity in eval mode
            return {'seg_logit': ops.pn2_fp_mlp(None, None, None, up.contiguous(), *frozen, relu_last=False)}
        if self.seg_logit.kernel_size == (1,) and self._use_fused_training(self.mlp_seg, up):
            # mlp_seg on rows with its dropout, the logits as one more product plus the bias (fuse_training)
            x = rows_mlp(self.mlp_seg, channel_rows(up), True, dropout=self.mlp_seg.p)
            w = self.seg_logit.weight
            x = ops.linear(x, w.view(w.shape[0], w.shape[1]))
            if self.seg_logit.bias is not None:
                x = x + self.seg_logit.bias
            return {'seg_logit': rows_to_channels(x, up.shape[0])}
        return {'seg_logit': self.seg_logit(self.mlp_seg(up))}

    def _snapshot(self):
        return fold_chain(self.mlp_seg, head=self.seg_logit)

    def reset_parameters(self):
        for m in self.modules():
            if isinstance(m, (nn.Conv1d, nn.Conv2d, nn.Linear)):
                xavier_uniform(m)

    def get_loss(self, cfg):
        from mvpnet.models.loss import SegLoss
        weights = None
        if cfg.TRAIN.LABEL_WEIGHTS_PATH:
            weights = torch.from_numpy(np.loadtxt(cfg.TRAIN.LABEL_WEIGHTS_PATH, dtype=np.float32)).cuda()
        return SegLoss(weight=weights)

    def get_metric(self, cfg):
        from mvpnet.models.metric import SegAccuracy, SegIoU
        make = lambda: [SegAccuracy(), SegIoU(self.num_classes)]
        return make(), make()
