"""NumPy restatement of the fused frozen PointNet++ kernels (csrc/pn2_mlp.hip): "group, concatenate, affine chain, ReLU,
max over the neighbours" and "interpolate, concatenate, affine chain", in the dtype of the inputs (the tests feed
float64), plus the float64 fold of BatchNorm's running statistics into a 1x1 convolution."""
import numpy as np


def unpack(params, widths, dtype=np.float64):
    """[(W_l [widths[l+1], widths[l]], b_l [widths[l+1]])] of the packed chain [W0|b0|W1|b1|...]."""
    params = np.asarray(params, dtype).reshape(-1)
    out, off = [], 0
    for l in range(len(widths) - 1):
        cin, cout = int(widths[l]), int(widths[l + 1])
        w = params[off:off + cout * cin].reshape(cout, cin)
        off += cout * cin
        out.append((w, params[off:off + cout]))
        off += cout
    assert off == params.size
    return out


def pack(layers):
    return np.concatenate([np.concatenate([np.asarray(w).reshape(-1), np.asarray(b).reshape(-1)]) for w, b in layers])


def chain(rows, layers, relu_last=True):
    """rows [..., Cin] -> [..., Cout]: y = relu(x W^T + b) per layer, the last one linear when relu_last is False."""
    x = rows
    for l, (w, b) in enumerate(layers):
        x = x @ w.T + b
        if relu_last or l + 1 < len(layers):
            x = np.maximum(x, 0)
    return x


def group(points, index):
    """points [C,N], index [M,K] -> [C,M,K]; an index outside [0, N) reads as zero (group_points_fwd_kernel)."""
    n = points.shape[1]
    ok = (index >= 0) & (index < n)
    return np.where(ok[None], points[:, np.where(ok, index, 0)], 0)


def sa_rows(xyz, feature, new_xyz, index, use_xyz=True):
    """The input rows of one batch element, [M,K,C(+3)]: features first, then xyz(idx) - new_xyz, zero-then-subtract."""
    parts = []
    if feature is not None:
        parts.append(group(feature, index))
    if feature is None or use_xyz:
        parts.append(group(xyz, index) - new_xyz[:, :, None])
    return np.concatenate(parts, 0).transpose(1, 2, 0)


def sa_mlp_max(xyz, feature, new_xyz, index, params, widths, dtype=np.float64):
    """xyz [B,3,N], feature [B,C,N] or None, new_xyz [B,3,M], index [B,M,K] -> [B,Cout,M]."""
    layers = unpack(params, widths, dtype)
    xyz, new_xyz = np.asarray(xyz, dtype), np.asarray(new_xyz, dtype)
    feature = None if feature is None else np.asarray(feature, dtype)
    c = 0 if feature is None else feature.shape[1]
    use_xyz = widths[0] == c + 3
    out = []
    for b in range(xyz.shape[0]):
        rows = sa_rows(xyz[b], None if feature is None else feature[b], new_xyz[b], index[b], use_xyz)
        assert rows.shape[2] == widths[0]
        out.append(chain(rows, layers).max(1).T)
    return np.stack(out)


def interpolate(sparse, index, weight):
    """sparse [C2,N2], index [N1,3], weight [N1,3] -> [C2,N1], k = 0, 1, 2 accumulated in that order in the dtype of
    the inputs, every product and sum rounded; an index outside [0, N2) contributes nothing."""
    n2 = sparse.shape[1]
    acc = np.zeros((sparse.shape[0], index.shape[0]), sparse.dtype)
    for k in range(3):
        ok = (index[:, k] >= 0) & (index[:, k] < n2)
        term = sparse[:, np.where(ok, index[:, k], 0)] * weight[None, :, k]
        acc = np.where(ok[None], acc + term, acc)
    return acc


def fp_mlp(sparse, index, weight, dense, params, widths, relu_last=True, dtype=np.float64):
    """sparse [B,C2,N2], index [B,N1,3], weight [B,N1,3], dense [B,C1,N1] or None -> [B,Cout,N1]; index None: the rows
    are `dense` alone."""
    layers = unpack(params, widths, dtype)
    nb = dense.shape[0] if index is None else sparse.shape[0]
    out = []
    for b in range(nb):
        parts = []
        if index is not None:
            parts.append(interpolate(np.asarray(sparse[b], dtype), index[b], np.asarray(weight[b], dtype)))
        if dense is not None:
            parts.append(np.asarray(dense[b], dtype))
        rows = np.concatenate(parts, 0).T
        assert rows.shape[1] == widths[0]
        out.append(chain(rows, layers, relu_last).T)
    return np.stack(out)


def fold_layer(sd, prefix, eps=1e-5):
    """(W, b) float64 of one conv + BatchNorm layer `prefix` (.conv.weight, .bn.*) of a state dict of arrays:
    scale = gamma / sqrt(running_var + eps), shift = beta - running_mean * scale, W * scale row-wise."""
    w = np.asarray(sd[prefix + ".conv.weight"], np.float64)
    w = w.reshape(w.shape[0], w.shape[1])
    gamma, beta = np.asarray(sd[prefix + ".bn.weight"], np.float64), np.asarray(sd[prefix + ".bn.bias"], np.float64)
    mean, var = np.asarray(sd[prefix + ".bn.running_mean"], np.float64), np.asarray(sd[prefix + ".bn.running_var"], np.float64)
    scale = gamma / np.sqrt(var + eps)
    return w * scale[:, None], beta - mean * scale


def fold_stack(sd, prefix, n_layers, head=None, dtype=np.float32):
    """The packed chain (float32 as the drop-in stores it) and widths of layers prefix.0 .. prefix.(n_layers-1), then an
    optional plain convolution `head` (.weight, .bias)."""
    layers = [fold_layer(sd, "%s.%d" % (prefix, i)) for i in range(n_layers)]
    if head is not None:
        w = np.asarray(sd[head + ".weight"], np.float64)
        layers.append((w.reshape(w.shape[0], w.shape[1]), np.asarray(sd[head + ".bias"], np.float64)))
    widths = [layers[0][0].shape[1]] + [w.shape[0] for w, _ in layers]
    return pack(layers).astype(dtype), tuple(widths)
