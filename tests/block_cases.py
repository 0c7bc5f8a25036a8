"""The seeded cases of the network-block sweep, shared by tests/test_blocks_cpu.py (the conditions the inputs must meet,
on the float64 and float32 runs of the oracle alone) and tests/test_blocks_gpu.py (dropin/models/blocks.py on the HIP
kernels against the float64 run of oracle/torch_port.py). numpy only.

Geometry: N float32 points in a 0.5 cube (coordinates below 0.5 keep the float32 rounding of a distance ~ 0.06 below 2e-6
relative), strided blocks query every 4th point; neighbour / pool rows by brute force on those float32 coordinates:
points within R = 0.125, sorted by distance (ties by index), cut to H columns, padded with the shadow index Ns. One query
(ROW_SHADOW) is moved far away so that its row holds shadow entries only. Kernel points, weights and running statistics
come from a seed (util.seeded_state, parameter names of the reference); the offset convolutions of the deformable blocks
are scaled like util.g13_state so that offsets are a fraction of the extent.

Every case names the fused routes of ops.py its forward must reach (`routes`, derived from the host code of
dropin/models/blocks.py, see routes_of) and the seed its inputs are drawn from. The seed is one for which no LeakyReLU
input, no deformable kernel weight and no arg-min sits where a correct float32 implementation could legitimately land
on the other side of a kink (tests/test_blocks_cpu.py asserts it), so every element of every tensor is compared."""
import collections
import functools
import types

import numpy as np

from util import seeded_state

R = 0.125                # search radius = the radius handed to block_decider
KP_EXTENT = 1.2          # config.KP_extent; extent of a block = R * KP_EXTENT / CONV_RADIUS = 0.06
CONV_RADIUS = 2.5
K = 15
SIDE = 0.5
ROW_SHADOW = 3           # the query moved to FAR: a row of shadow entries only
FAR = 3.0
ALIAS_C = 0.25           # weight of sum(alias) in the scalar a strided case differentiates (the second consumer)
BN_MOMENTUM = 0.1

# ---- the routes (names of the ops.py entry points the spies of the GPU test count)
LINEAR_PAIR = "linear_pair"                  # returned a pair, without the statistics epilogue
LINEAR_PAIR_STATS = "linear_pair+stats"      # returned a pair whose outputs carry BatchNorm statistics
LINEAR = "linear"
LINEAR_PASS = "linear+passthrough"
MAX_POOL = "max_pool"
MAX_POOL_PASS = "max_pool+passthrough"
BN_PAIR = "bn_lrelu_pair"
BN_LINEAR = "bn_lrelu_linear"                # returned a result (the fold applied)
BN = "bn_lrelu"
BIAS = "bias_lrelu"
LINEAR_BIAS = "linear_bias_lrelu"
ADD = "add_lrelu"
UPCAT_LINEAR = "upsample_cat_linear"
DEFORM_OPERANDS = "deform_operands"
KPCONV = "kpconv"
KPCONV_REV = "kpconv+rev"
XENT = "cross_entropy_lut"

MODES = (None, "idx64", "rev", "scatter", "det", "fold")

Case = collections.namedtuple("Case", "name block cin cout N H use_bn mod mode base routes seed")


def routes_of(block, cin, cout, use_bn, mode, stats_pair=False, fold_finishes=True):
    """The routes ResnetBottleneckBlock.forward / SimpleBlock.forward take in training mode on the GPU, restated from
    dropin/models/blocks.py. stats_pair: more rows than ops.bn_single_launch_rows, so linear_pair asks for the statistics
    epilogue. fold_finishes (mode "fold"): the convolution's contraction carries the statistics epilogue at this shape,
    so it finishes them and unary2 takes forward_normalised."""
    strided, deform = "strided" in block, "deform" in block
    rev = mode in ("rev", "det")
    r = {KPCONV_REV if rev else KPCONV}
    if deform:
        r.add(DEFORM_OPERANDS)
    act = BN if use_bn else BIAS
    if block.startswith("simple"):
        r.add(act)
        return frozenset(r)
    has_u1, has_us = cin != cout // 4, cin != cout
    fold = mode == "fold" and use_bn
    if has_u1 and has_us and not strided:
        r |= {LINEAR_PAIR_STATS if (use_bn and (stats_pair or fold)) else LINEAR_PAIR, act}      # unary1 + shortcut product
    elif has_u1:
        r |= {LINEAR_PASS, act}                                                                  # unary1(passthrough=True)
    if strided:
        r.add(MAX_POOL_PASS)
    pair = has_u1 and has_us and not strided
    if fold and fold_finishes:
        # shortcut: us(shortcut) = linear + bn_lrelu, or us.batch_norm(ys); unary2 = bn_lrelu_linear (which calls linear)
        r |= {BN_LINEAR, LINEAR, BN}
    elif use_bn and has_us:
        if not pair:
            r.add(LINEAR)                                                                        # the shortcut product
        r |= {BN_PAIR, LINEAR, BN}                                                               # unary2 + joined BatchNorm
    elif use_bn:
        r |= {BN, LINEAR}
    else:
        r.add(BIAS)                                                                              # batch_norm_conv
        if has_us and not pair:
            r.add(LINEAR_BIAS)                                                                   # us(shortcut), no BatchNorm
        r |= {LINEAR, ADD}                                                                       # unary2 + x + bias + join
    return frozenset(r)


def _c(block, cin, cout, N=400, H=20, use_bn=True, mod=False, mode=None, seed=0, tag="", **kw):
    base = "%s-%d-%d%s%s%s" % (block, cin, cout, "-mod" if mod else "", "" if use_bn else "-nobn", tag)
    name = base if mode is None else base + "-" + mode
    return Case(name, block, cin, cout, N, H, use_bn, mod, mode, base, routes_of(block, cin, cout, use_bn, mode, **kw), seed)


# seeds: found by a search on the CPU over the conditions of tests/test_blocks_cpu.py (block_ref.conditions), recorded here
_SEEDS = {"resnetb-32-128": 1, "resnetb_strided-128-128": 1, "resnetb_deformable-64-128-mod": 1,
          "resnetb_deformable_strided-64-128-mod": 2, "resnetb-64-128-nobn": 1, "resnetb-64-128": 1,
          "simple_deformable-64-128-mod": 2, "resnetb_deformable-64-128": 4, "resnetb-64-128-n1030": 13}      # (every other case: 0)


def _table():
    t = [
        _c("resnetb", 64, 128),                                  # unary1 and a shortcut layer: linear_pair, bn_lrelu_pair
        _c("resnetb", 64, 128, N=100, tag="-n100"),             # single-launch BatchNorm: no statistics epilogue asked for
        _c("resnetb", 64, 128, N=1030, tag="-n1030", stats_pair=True),   # above bn_single_launch_rows: the epilogue
        _c("resnetb", 128, 128),                                 # identity shortcut: unary1(passthrough=True)
        _c("resnetb", 32, 128),                                  # unary1 is nn.Identity
        _c("resnetb_strided", 64, 128),                          # 400 -> 100 rows: max_pool(passthrough=True), skip_alias
        _c("resnetb_strided", 128, 128),
        _c("simple", 4, 64),                                     # small-row KPConv kernel
        _c("simple", 5, 64),                                     # first-layer shape
        _c("simple_strided", 64, 128),
    ]
    for mod in (False, True):
        t += [_c("resnetb_deformable", 64, 128, mod=mod), _c("resnetb_deformable_strided", 64, 128, mod=mod),
              _c("simple_deformable", 64, 128, mod=mod)]
    t += [_c("resnetb", 64, 128, use_bn=False), _c("resnetb_strided", 64, 128, use_bn=False), _c("simple", 5, 64, use_bn=False)]
    for block in ("resnetb", "resnetb_strided", "resnetb_deformable"):
        for mode in MODES[1:]:
            t.append(_c(block, 64, 128, mode=mode))
    return [c._replace(seed=_SEEDS.get(c.base, 0)) for c in t]


CASES = _table()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
BASES = [c.name for c in CASES if c.mode is None]


def config(use_bn=True, mod=False, architecture=(), first_features_dim=16, in_features_dim=5):
    """The fields oracle/torch_port.py reads (the GPU test copies them onto the product's Config)."""
    return types.SimpleNamespace(use_batch_norm=use_bn, batch_norm_momentum=BN_MOMENTUM, KP_extent=KP_EXTENT,
                                 conv_radius=CONV_RADIUS, KP_influence="linear", aggregation_mode="sum",
                                 num_kernel_points=K, modulated=mod, architecture=list(architecture),
                                 first_subsampling_dl=R / CONV_RADIUS, in_points_dim=3, fixed_kernel_points="center",
                                 first_features_dim=first_features_dim, in_features_dim=in_features_dim,
                                 deform_fitting_power=1.0, repulse_extent=1.2, variant="baseline")


# ---------------------------------------------------------------- geometry

def radius_rows(q, s, radius, H, q_cloud=None, s_cloud=None):
    """[Nq, H] int32: the supports within `radius` of every query by brute force in float32 ((dx dx + dy dy) + dz dz),
    nearest first, ties by index, padded with Ns. q_cloud / s_cloud: cloud number per point (stacked clouds)."""
    d = q[:, None, :] - s[None, :, :]
    d2 = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]).astype(np.float32)
    far = ~(d2 < np.float32(radius) * np.float32(radius))
    if q_cloud is not None:
        far |= q_cloud[:, None] != s_cloud[None, :]
    d2 = np.where(far, np.float32(np.inf), d2)
    order = np.argsort(d2, axis=1, kind="stable")[:, :H]
    kept = np.take_along_axis(d2, order, 1)
    idx = np.where(np.isinf(kept), s.shape[0], order).astype(np.int32)
    if idx.shape[1] < H:
        idx = np.concatenate([idx, np.full((idx.shape[0], H - idx.shape[1]), s.shape[0], np.int32)], 1)
    return idx


def kernel_points(rng, radius):
    """K seeded kernel points: the first at the centre, the others at 0.4 .. 0.7 of the radius."""
    d = rng.normal(size=(K, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    kp = d * rng.uniform(0.4, 0.7, size=(K, 1)) * radius
    kp[0] = 0
    return kp.astype(np.float32)


# ---------------------------------------------------------------- parameter shapes (the constructors of blocks.py restated)

def _bn_shapes(sh, prefix, d, use_bn):
    if use_bn:
        for leaf in ("weight", "bias", "running_mean", "running_var"):
            sh[prefix + ".batch_norm." + leaf] = (d,)
        sh[prefix + ".batch_norm.num_batches_tracked"] = ()
    else:
        sh[prefix + ".bias"] = (d,)


def _unary_shapes(sh, prefix, cin, cout, use_bn):
    sh[prefix + ".mlp.weight"] = (cout, cin)
    _bn_shapes(sh, prefix + ".batch_norm", cout, use_bn)


def _kpconv_shapes(sh, prefix, cin, cout, deform, mod):
    sh[prefix + ".weights"] = (K, cin, cout)
    sh[prefix + ".kernel_points"] = (K, 3)
    if deform:
        od = (4 if mod else 3) * K
        sh[prefix + ".offset_conv.weights"] = (K, cin, od)
        sh[prefix + ".offset_conv.kernel_points"] = (K, 3)
        sh[prefix + ".offset_bias"] = (od,)


def block_shapes(sh, prefix, block, cin, cout, use_bn, mod):
    """Adds the state-dict entries of block_decider(block, ., cin, cout, ., config) under `prefix` ('' or 'a.b.')."""
    deform = "deform" in block
    if block == "unary":
        _unary_shapes(sh, prefix[:-1], cin, cout, use_bn)
    elif block.startswith("simple"):
        _kpconv_shapes(sh, prefix + "KPConv", cin, cout // 2, deform, mod)
        _bn_shapes(sh, prefix + "batch_norm", cout // 2, use_bn)
    elif block.startswith("resnetb"):
        if cin != cout // 4:
            _unary_shapes(sh, prefix + "unary1", cin, cout // 4, use_bn)
        _kpconv_shapes(sh, prefix + "KPConv", cout // 4, cout // 4, deform, mod)
        _bn_shapes(sh, prefix + "batch_norm_conv", cout // 4, use_bn)
        _unary_shapes(sh, prefix + "unary2", cout // 4, cout, use_bn)
        if cin != cout:
            _unary_shapes(sh, prefix + "unary_shortcut", cin, cout, use_bn)
    return sh


def _state(sh, seed, rng, radius_of):
    """seeded_state over `sh` with seeded kernel points (radius_of(name) = the radius of that layer) and the offset
    convolutions scaled by 0.2 (util.g13_state)."""
    fixed = {n: kernel_points(rng, radius_of(n)) for n in sorted(sh) if n.endswith("kernel_points")}
    sd = seeded_state(sh, seed, fixed=fixed)
    for n in sd:
        if n.endswith("offset_conv.weights"):
            sd[n] = (sd[n] * np.float32(0.2)).astype(np.float32)
    return sd


def _freeze(*arrays):
    for a in arrays:
        if isinstance(a, dict):
            _freeze(*a.values())
        elif isinstance(a, (list, tuple)):
            _freeze(*a)
        elif isinstance(a, np.ndarray):
            a.setflags(write=False)


Inputs = collections.namedtuple("Inputs", "q s idx x go state")


@functools.lru_cache(maxsize=None)
def make_inputs(base):
    """The float32 inputs of a case (by the name of its base case: the modes share them). idx is int32; state holds the
    block's own state-dict names. Cached: read-only."""
    c = BY_NAME[base]
    rng = np.random.default_rng([c.seed, c.cin, c.cout, c.N, int(c.mod), int(c.use_bn), len(c.block)])
    s = (rng.random((c.N, 3)) * SIDE).astype(np.float32)
    if "strided" in c.block:
        q = s[::4].copy()
        q[ROW_SHADOW] = FAR
    else:
        s[ROW_SHADOW] = FAR
        q = s
    idx = radius_rows(q, s, R, c.H)
    idx[ROW_SHADOW] = c.N               # (a block that is not strided: the moved point would still find itself)
    x = rng.normal(size=(c.N, c.cin)).astype(np.float32)
    width = c.cout // 2 if c.block.startswith("simple") else c.cout
    go = rng.normal(size=(q.shape[0], width)).astype(np.float32)
    sh = block_shapes({}, "", c.block, c.cin, c.cout, c.use_bn, c.mod)
    state = _state(sh, 4000 + c.seed, rng, lambda n: R)
    _freeze(q, s, idx, x, go, state)
    return Inputs(q, s, idx, x, go, state)


# ---------------------------------------------------------------- the two-level network

NET_ARCH = ("simple", "resnetb", "resnetb_strided", "resnetb", "nearest_upsample", "unary")
NET_CLOUDS = (250, 150)
NET_CLASSES = 6                    # raw labels 0 .. 6, label 0 is ignored
NET_SEED = 2
# (no linear_pair: the pair launch does not take products as narrow as 8 -> (4, 16) and 16 -> (8, 32), mvk_gemm_f32_pair_plan;
# the two bottleneck blocks with a shortcut layer then run unary1(passthrough=True) and the shortcut product on its own)
NET_ROUTES = frozenset({KPCONV, BN, BN_PAIR, LINEAR, LINEAR_PASS, MAX_POOL_PASS, UPCAT_LINEAR, LINEAR_BIAS, XENT})

NetInputs = collections.namedtuple("NetInputs", "points neighbors pools upsamples lengths features labels state")


def net_shapes():
    """State-dict shapes of architectures.KPFCNN over NET_ARCH (build_encoder / build_decoder restated)."""
    cfg = config(architecture=NET_ARCH)
    sh = {}
    cin, cout = cfg.in_features_dim, cfg.first_features_dim
    skip_dims = []
    for i, b in enumerate(NET_ARCH):
        if "strided" in b or "upsample" in b:
            skip_dims.append(cin)
        if "upsample" in b:
            start = i
            break
        block_shapes(sh, "encoder_blocks.%d." % i, b, cin, cout, True, False)
        cin = cout // 2 if "simple" in b else cout
        if "strided" in b:
            cout *= 2
    layer = 1
    for j, b in enumerate(NET_ARCH[start:]):
        if j > 0 and "upsample" in NET_ARCH[start + j - 1]:
            cin += skip_dims[layer]
        block_shapes(sh, "decoder_blocks.%d." % j, b, cin, cout, True, False)
        cin = cout
        if "upsample" in b:
            layer -= 1
            cout //= 2
    _unary_shapes(sh, "head_mlp", cout, cfg.first_features_dim, False)
    _unary_shapes(sh, "head_softmax", cfg.first_features_dim, NET_CLASSES, False)
    return sh


@functools.lru_cache(maxsize=None)
def make_net_inputs(seed=NET_SEED):
    """Two stacked clouds of 250 and 150 points, level 1 = every 4th point of each, rows by brute force inside a cloud
    (radius R at level 0 and for the pools, 2 R at level 1 and for the upsampling), row ROW_SHADOW of level 0 moved away."""
    rng = np.random.default_rng([seed, 77])
    n0 = sum(NET_CLOUDS)
    p0 = (rng.random((n0, 3)) * SIDE).astype(np.float32)
    p0[ROW_SHADOW] = FAR
    c0 = np.repeat(np.arange(len(NET_CLOUDS)), NET_CLOUDS)
    pick = np.concatenate([np.arange(o, o + n, 4) for o, n in zip(np.cumsum((0,) + NET_CLOUDS[:-1]), NET_CLOUDS)])
    assert ROW_SHADOW not in pick
    p1, c1 = p0[pick].copy(), c0[pick]
    nb0 = radius_rows(p0, p0, R, 20, c0, c0)
    nb0[ROW_SHADOW] = n0
    nb1 = radius_rows(p1, p1, 2 * R, 20, c1, c1)
    pool0 = radius_rows(p1, p0, R, 20, c1, c0)
    up0 = radius_rows(p0, p1, 2 * R, 4, c0, c1)
    cfg = config(architecture=NET_ARCH)
    feats = rng.normal(size=(n0, cfg.in_features_dim)).astype(np.float32)
    labels = rng.integers(0, NET_CLASSES + 1, n0).astype(np.int64)
    sh = net_shapes()
    level1 = {"encoder_blocks.3."}
    state = _state(sh, 4100 + seed, rng, lambda n: 2 * R if any(n.startswith(p) for p in level1) else R)
    lengths = [np.array(NET_CLOUDS, np.int32), np.bincount(c1).astype(np.int32)]
    out = NetInputs([p0, p1], [nb0, nb1], [pool0], [up0], lengths, feats, labels, state)
    _freeze(*out)
    return out
