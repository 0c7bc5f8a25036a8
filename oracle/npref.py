"""TEST INFRASTRUCTURE ONLY -- numpy restatement of the floating-point part of
the MV-KPConv hot path. Pinned by tests/golden (generated from the reference's
own Python modules, see tests/golden/make_golden.py).

All paths below are relative to /root/reference/.
"""
import numpy as np


# ---------------------------------------------------------------------------
# KPConv (KPConv-PyTorch/models/blocks.py:237-374, rigid + deformable/modulated)
# ---------------------------------------------------------------------------

def kp_influence(d2, extent, influence):
    """blocks.py:329-346."""
    if influence == "constant":
        return np.ones_like(d2)
    if influence == "linear":
        return np.maximum(1 - np.sqrt(d2) / d2.dtype.type(extent), 0).astype(d2.dtype)
    if influence == "gaussian":
        sig = extent * 0.3
        return np.exp(-d2 / d2.dtype.type(2 * sig ** 2 + 1e-9)).astype(d2.dtype)  # blocks.py:69-76
    raise ValueError("Unknown influence function type (config.KP_influence)")


def kpconv_weights(q, s, idx, kp, extent, influence="linear", aggregation="sum", offsets=None):
    """Influence weights w[n,h,k] (blocks.py:277-351). Returns (w, d2).

    offsets: optional [Nq,K,3] already scaled by KP_extent (blocks.py:266,287)."""
    dt = q.dtype
    Ns = s.shape[0]
    sp = np.concatenate([s, np.full((1, 3), 1e6, dt)], 0)          # :277
    rel = sp[idx] - q[:, None, :]                                     # :280-283
    kpts = kp[None, None] if offsets is None else (offsets + kp)[:, None]   # :287-290
    diff = rel[:, :, None, :] - kpts                                  # :293-294
    d2 = np.sum(diff ** 2, axis=3, dtype=dt)                          # :297
    w = kp_influence(d2, extent, influence)
    if aggregation == "closest":                                      # :349-351
        nn = np.argmin(d2, axis=2)
        w = w * np.eye(kp.shape[0], dtype=dt)[nn]
    elif aggregation != "sum":
        raise ValueError("Unknown convolution mode. Should be 'closest' or 'sum'")
    return w, d2


def deform_in_range(idx, Ns, d2, extent):
    """keep[n,h] of the deformable branch (blocks.py:306-325): entry h stays a neighbour when it is a real one and lies
    within `extent` of AT LEAST ONE deformed kernel point, strictly (d2 < extent**2); every other column is re-pointed
    to the shadow row (zero features)."""
    return (idx < Ns) & np.any(d2 < d2.dtype.type(extent) ** 2, axis=2)


def kpconv_forward(q, s, idx, x, kp, W, extent, influence="linear", aggregation="sum",
                   offsets=None, modulations=None, return_A=False):
    """y[n,:] = sum_k (sum_h w[n,h,k] x+[idx[n,h]]) @ W[k]   (SURVEY.md A.4).

    Rigid: the dense formula. Deformable (offsets given): the neighbour re-compaction of blocks.py:300-325 is applied
    as a mask on the columns (deform_in_range) for EVERY influence. Under the linear influence it only removes weights
    that are exactly 0; under the gaussian and constant influences it removes non-zero weights, so it changes A and y
    (and, in the backward, dx, dW and d_offsets)."""
    w, d2 = kpconv_weights(q, s, idx, kp, extent, influence, aggregation, offsets)
    if offsets is not None:
        w = w * deform_in_range(idx, s.shape[0], d2, extent)[:, :, None]
    xp = np.concatenate([x, np.zeros((1, x.shape[1]), x.dtype)], 0)  # :357
    nx = xp[idx]                                                      # :360  [N,H,Cin]
    A = np.einsum("nhk,nhc->nkc", w, nx)                              # :363
    if modulations is not None:
        A = A * modulations[:, :, None]                               # :366-367
    y = np.einsum("nkc,kco->no", A, W)                                # :370-374
    return (y, A, w) if return_A else y


def kpconv_backward(q, s, idx, x, kp, W, extent, g, influence="linear", aggregation="sum"):
    """Rigid KPConv backward: returns (dx [Ns,Cin], dW [K,Cin,Cout])."""
    w, _ = kpconv_weights(q, s, idx, kp, extent, influence, aggregation)
    Ns = s.shape[0]
    xp = np.concatenate([x, np.zeros((1, x.shape[1]), x.dtype)], 0)
    A = np.einsum("nhk,nhc->nkc", w, xp[idx])
    dW = np.einsum("nkc,no->kco", A, g)
    dA = np.einsum("no,kco->nkc", g, W)
    contrib = np.einsum("nhk,nkc->nhc", w, dA)
    dxp = np.zeros_like(xp)
    np.add.at(dxp, idx.reshape(-1), contrib.reshape(-1, x.shape[1]))
    return dxp[:Ns], dW


def kpconv_deform_backward(q, s, idx, x, kp, W, extent, offsets, modulations, g_y, g_min_d2, influence="linear"):
    """Deformable (and modulated) KPConv, sum aggregation, forward and every gradient of
        loss = sum(y * g_y) + sum(min_d2 * g_min_d2)
    in the dtype of the inputs (float64 for an oracle, float32 to see what the number format alone costs).
    Algebra: header of csrc/deform.hip, SURVEY.md A.4 / A.6. With rel[n,h] = s+[idx[n,h]] - q[n] (the shadow point sits at
    1e6), kpdef = kp + offsets, diff[n,h,k] = rel[n,h] - kpdef[n,k], d2 = |diff|^2, keep = deform_in_range and
    w = influence(d2) * keep:
        A[n,k,c] = sum_h w[n,h,k] x+[idx[n,h],c]        (unmodulated; Am = A * modulations)
        y = sum_k Am[:,k,:] @ W[k]                       min_d2[n,k] = min_h d2[n,h,k]   (shadow entries included)
        dW[k] = Am[:,k,:]^T g_y                          dAm = g_y W^T
        d_modulations = sum_c dAm * A                    dA = dAm * modulations
        dx[idx[n,h]] += sum_k w[n,h,k] dA[n,k,:]
        d_offsets[n,k] = sum_h keep (dw/doff)[n,h,k] B[n,h,k]  -  2 diff[n,h*,k] g_min_d2[n,k]
    with B[n,h,k] = sum_c x+[idx[n,h],c] dA[n,k,c], h* the arg-min column, and
        dw/doff = diff / (extent sqrt(d2)) inside the support (linear), 2 w diff / den (gaussian), 0 (constant).
    modulations / g_min_d2 may be None. Returns (dx, dW, d_offsets, d_modulations or None, A, y, min_d2, diag) with
    diag = {kept [Nq] kept columns per row, keep [Nq,H], kink_band: real entries with |sqrt(d2)/extent - 1| < 1e-5,
    argmin_ties: (n,k) whose minimum is approached within 1e-5 relative by ANOTHER support point,
    d_offsets_min: the min_d2 term of d_offsets alone, dA: the gradient of the unmodulated aggregate}."""
    dt = q.dtype
    Ns, Cin = s.shape[0], x.shape[1]
    ext = dt.type(extent)
    sp = np.concatenate([s, np.full((1, 3), 1e6, dt)], 0)
    rel = sp[idx] - q[:, None, :]                                     # [N,H,3]
    kpdef = kp[None] + offsets                                        # [N,K,3]
    diff = rel[:, :, None, :] - kpdef[:, None]                        # [N,H,K,3]
    d2 = np.sum(diff ** 2, axis=3, dtype=dt)                          # [N,H,K]
    hstar = np.argmin(d2, axis=1)                                     # [N,K]
    min_d2 = np.take_along_axis(d2, hstar[:, None, :], axis=1)[:, 0]
    real = idx < Ns
    keep = deform_in_range(idx, Ns, d2, extent)
    wf = kp_influence(d2, extent, influence)
    w = wf * keep[:, :, None]
    xp = np.concatenate([x, np.zeros((1, Cin), dt)], 0)
    nx = xp[idx]                                                      # [N,H,Cin]
    A = np.einsum("nhk,nhc->nkc", w, nx)
    Am = A * modulations[:, :, None] if modulations is not None else A
    y = np.einsum("nkc,kco->no", Am, W)
    dW = np.einsum("nkc,no->kco", Am, g_y)
    dAm = np.einsum("no,kco->nkc", g_y, W)
    d_mod = None
    dA = dAm
    if modulations is not None:
        d_mod = np.sum(dAm * A, axis=2, dtype=dt)
        dA = dAm * modulations[:, :, None]
    dxp = np.zeros_like(xp)
    np.add.at(dxp, idx.reshape(-1), np.einsum("nhk,nkc->nhc", w, dA).reshape(-1, Cin))
    B = np.einsum("nhc,nkc->nhk", nx, dA)
    if influence == "linear":
        inside = keep[:, :, None] & (wf > 0) & (d2 > 0)
        sc = np.where(inside, 1 / (ext * np.sqrt(np.where(inside, d2, 1))), 0).astype(dt)
    elif influence == "gaussian":
        sc = (2 * w / dt.type(2 * (extent * 0.3) ** 2 + 1e-9)).astype(dt)
    else:
        sc = np.zeros_like(d2)
    d_off = np.einsum("nhk,nhkd->nkd", sc * B, diff)
    d_off_min = np.zeros_like(d_off)
    if g_min_d2 is not None:
        at_min = np.take_along_axis(diff, hstar[:, None, :, None], axis=1)[:, 0]      # [N,K,3]
        d_off_min = -2 * at_min * g_min_d2[:, :, None]
    # diagnostics: where the function (or its gradient) jumps
    dist = np.sqrt(d2)
    kink = int(np.count_nonzero(real[:, :, None] & (np.abs(dist / ext - 1) < 1e-5)))
    other = idx[:, :, None] != np.take_along_axis(idx, hstar, axis=1)[:, None, :]   # another support point than h*'s
    ties = int(np.count_nonzero(np.any(other & (d2 <= min_d2[:, None, :] * (1 + 1e-5)), axis=1)))
    diag = dict(kept=keep.sum(1), keep=keep, kink_band=kink, argmin_ties=ties, d_offsets_min=d_off_min, dA=dA)
    return dxp[:Ns], dW, (d_off + d_off_min).astype(dt), d_mod, A, y, min_d2, diag


# ---------------------------------------------------------------------------
# pooling helpers (blocks.py:79-133)
# ---------------------------------------------------------------------------

def max_pool(x, inds):
    xp = np.concatenate([x, np.zeros((1, x.shape[1]), x.dtype)], 0)   # :103
    return xp[inds].max(axis=1)                                       # :106-110


def closest_pool(x, inds):
    xp = np.concatenate([x, np.zeros((1, x.shape[1]), x.dtype)], 0)   # :88
    return xp[inds[:, 0]]                                             # :91


# ---------------------------------------------------------------------------
# fusion inputs (KPConv-PyTorch/datasets/ScanNet_sphere_color.py)
# ---------------------------------------------------------------------------

def depth2xyz(cam_matrix, depth):
    """ScanNet_sphere_color.py:66-72 (result is float64: int64 pixel grid x float32 inverse)."""
    v, u = np.indices(depth.shape)
    u, v = u.ravel(), v.ravel()
    uv1 = np.stack([u, v, np.ones_like(u)], axis=1)
    return (np.linalg.inv(cam_matrix[:3, :3]).dot(uv1.T) * depth.ravel()).T


def unproject_frames(cam_matrix, depths_mm, poses):
    """ScanNet_sphere_color.py:409-417 per frame: depth u16 mm -> world xyz (float64) + valid mask.

    depths_mm (nv,h,w) uint16, poses (nv,4,4) float32, cam_matrix float32 (already rescaled)."""
    xyz, mask = [], []
    for d, pose in zip(depths_mm, poses):
        depth = np.asarray(d, dtype=np.float32) / 1000.                 # :410
        p = depth2xyz(cam_matrix, depth)                               # :413
        m = p[:, 2] > 0                                                # :415
        p = np.matmul(p, pose[:3, :3].T) + pose[:3, 3]                 # :417
        xyz.append(p.reshape(d.shape + (3,)))
        mask.append(m.reshape(d.shape))
    return np.stack(xyz, 0), np.stack(mask, 0)


def knn_pixels(sphere_points, image_xyz, image_mask, k=3):
    """ScanNet_sphere_color.py:436-451: exact k-NN (float64) of every sphere point among
    the valid unprojected pixels, remapped to flat pixel index view*h*w + row*w + col."""
    from . import cport
    flat_xyz = image_xyz.reshape(-1, 3)
    ind_all = np.nonzero(image_mask.reshape(-1))[0]
    idx, _ = cport.knn_f64(sphere_points.astype(np.float64), flat_xyz[ind_all], k)
    return ind_all[idx].astype(np.int64)


# ---------------------------------------------------------------------------
# group_points (mvpnet/ops/group_points.py:20-31, cuda/group_points_kernel.cu:25-47,50-89;
# restatement in mvpnet/ops/tests/test_group_points.py:6-12)
# ---------------------------------------------------------------------------

def group_points(points, index):
    """points (B,C,N1), index (B,N2,K) -> (B,C,N2,K)."""
    B, Cc, _ = points.shape
    out = np.empty((B, Cc) + index.shape[1:], points.dtype)
    for b in range(B):
        out[b] = points[b][:, index[b]]
    return out


def group_points_backward(grad_out, index, n1):
    B, Cc = grad_out.shape[:2]
    gi = np.zeros((B, Cc, n1), grad_out.dtype)
    for b in range(B):
        for c in range(Cc):
            np.add.at(gi[b, c], index[b].reshape(-1), grad_out[b, c].reshape(-1))
    return gi


# ---------------------------------------------------------------------------
# sphere picking (KPConv-PyTorch/datasets/ScanNet_sphere_color.py:556-597)
# ---------------------------------------------------------------------------

def ball_members(points, center, radius):
    """sklearn KDTree.query_radius membership: float64 rdist = dx^2+dy^2+dz^2 (in that order) <= r^2;
    returns ascending indices and rdist."""
    p = np.asarray(points, np.float64)
    c = np.asarray(center, np.float64).reshape(3)
    d = p - c
    rd = np.zeros(p.shape[0])
    rd += d[:, 0] * d[:, 0]
    rd += d[:, 1] * d[:, 1]
    rd += d[:, 2] * d[:, 2]
    idx = np.nonzero(rd <= radius * radius)[0]
    return idx, rd[idx]


def sphere_pick(pot_points, potentials, min_pot, argmin_pot, input_points, in_radius, mask_margin=0.1):
    """One critical-section iteration (:556-584) + the input-region queries (:592-597), numpy.
    potentials / min_pot / argmin_pot are updated in place; returns (cloud_ind, point_ind, center,
    input_inds, mask_inds) with ascending indices."""
    cloud_ind = int(np.argmin(min_pot))
    point_ind = int(argmin_pot[cloud_ind])
    center = np.asarray(pot_points[cloud_ind], np.float64)[point_ind]
    idx, rd = ball_members(pot_points[cloud_ind], center, in_radius)
    d2s = np.square(np.sqrt(rd))                                   # query_radius returns sqrt(rdist); :576 squares it
    tukeys = np.square(1 - d2s / np.square(in_radius))             # :578
    tukeys[d2s > np.square(in_radius)] = 0                         # :579
    potentials[cloud_ind][idx] += tukeys                           # :581
    m = int(np.argmin(potentials[cloud_ind]))
    min_pot[cloud_ind] = potentials[cloud_ind][m]
    argmin_pot[cloud_ind] = m
    inp, _ = ball_members(input_points[cloud_ind], center, in_radius)
    msk, _ = ball_members(input_points[cloud_ind], center, in_radius + mask_margin)
    return cloud_ind, point_ind, center, inp, msk
