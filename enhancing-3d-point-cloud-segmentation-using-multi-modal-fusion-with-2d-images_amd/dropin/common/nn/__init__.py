"""The slice of the reference's ``common.nn`` the fusion path and the MVPNet baseline use
(common/nn/modules/mlp.py:38-95, common/nn/modules/conv.py:29-51, common/nn/init.py:22-26,
common/nn/functional.py:128-149). 1x1 convolutions and BatchNorm stay
PyTorch-ROCm library ops (plain GEMMs)."""
import warnings

import torch
from torch import nn
import torch.nn.functional as F

try:    # submodules the fusion path does not use (common.nn.freezer, .functional, ...) fall through to the reference
    from _fallthrough import extend as _extend
    __path__ = _extend(list(__path__), __name__, __file__)
except ImportError:
    pass


def _bn_native(bn, x):
    """BatchNorm with the MIOpen path switched off (PyTorch's native kernels instead): on this ROCm
    stack MIOpen's training-mode spatial BatchNorm is only ~1e-3 accurate on the (1, C, np, k)
    tensors of FeatureAggregation (measured 5e-3 abs error vs 1e-6 for the native kernel), which
    would break the 1e-4 parity bar. (Passing cudnn_enabled=False to torch.batch_norm is not enough
    on ROCm; the backend flag is what the dispatcher consults.)"""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with torch.backends.cudnn.flags(enabled=False):
            return bn(x)


class Conv1dBNReLU(nn.Module):
    def __init__(self, in_channels, out_channels, kernel_size, relu=True, bn=True, bn_momentum=0.1, **kwargs):
        super(Conv1dBNReLU, self).__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.conv = nn.Conv1d(in_channels, out_channels, kernel_size, bias=(not bn), **kwargs)
        self.bn = nn.BatchNorm1d(out_channels) if bn else None
        self.relu = nn.ReLU(inplace=True) if relu else None

    def forward(self, x):
        x = self.conv(x)
        if self.bn is not None:
            x = _bn_native(self.bn, x)
        return self.relu(x) if self.relu is not None else x


class Conv2dBNReLU(nn.Module):
    def __init__(self, in_channels, out_channels, kernel_size, relu=True, bn=True, **kwargs):
        super(Conv2dBNReLU, self).__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.conv = nn.Conv2d(in_channels, out_channels, kernel_size, bias=(not bn), **kwargs)
        self.bn = nn.BatchNorm2d(out_channels) if bn else None
        self.relu = nn.ReLU(inplace=True) if relu else None

    def forward(self, x):
        x = self.conv(x)
        if self.bn is not None:
            x = _bn_native(self.bn, x)
        return self.relu(x) if self.relu is not None else x


class SharedMLP(nn.ModuleList):
    """Stack of 1x1 conv + BN + ReLU shared over the resolution (1-D or 2-D)."""

    def __init__(self, in_channels, mlp_channels, ndim=1, bn=True):
        super(SharedMLP, self).__init__()
        self.in_channels = in_channels
        self.out_channels = mlp_channels[-1]
        self.ndim = ndim
        if ndim not in (1, 2):
            raise ValueError('SharedMLP only supports ndim=(1, 2).')
        layer = Conv1dBNReLU if ndim == 1 else Conv2dBNReLU
        c_in = in_channels
        for c_out in mlp_channels:
            self.append(layer(c_in, c_out, 1, relu=True, bn=bn))
            c_in = c_out

    def forward(self, x):
        for module in self:
            x = module(x)
        return x


class SharedMLPDO(SharedMLP):
    """SharedMLP with dropout after every layer (common/nn/modules/mlp.py:78-95): element dropout on (B,C,N)
    activations, channel dropout on (B,C,N,K)."""

    _DROPOUT = {1: F.dropout, 2: F.dropout2d}

    def __init__(self, *args, p=0.5, **kwargs):
        super(SharedMLPDO, self).__init__(*args, **kwargs)
        self.p = p

    @property
    def dropout_fn(self):
        return self._DROPOUT[self.ndim]

    def forward(self, x):
        drop = self.dropout_fn
        for layer in self:
            x = drop(layer(x), self.p, self.training)       # out of place: the ReLU before it works in place
        return x

    def extra_repr(self):
        return 'p={}'.format(self.p)


def batch_index_select(input, index, dim):
    """input (b, ...), index (b, n) -> input gathered along `dim` with a separate index row per batch element
    (common/nn/functional.py:128-149)."""
    if index.dim() != 2 or input.size(0) != index.size(0):
        raise ValueError('batch_index_select: index must be (batch, n) with the batch size of input')
    view = [1] * input.dim()
    view[0], view[dim] = index.size(0), index.size(1)
    shape = list(input.shape)
    shape[dim] = -1
    return torch.gather(input, dim, index.view(view).expand(shape))


def xavier_uniform(module):
    if module.weight is not None:
        nn.init.xavier_uniform_(module.weight)
    if module.bias is not None:
        nn.init.zeros_(module.bias)
