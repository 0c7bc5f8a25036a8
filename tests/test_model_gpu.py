"""GPU: the drop-in networks (HIP kernels) end to end against the unfused CPU port with identical
weights -- logits, loss and parameter gradients, for every fusion variant and for the deformable
architecture. Tolerances (round 3: set to ~3-10x what the runs show, profiles/r03_parity_errors.txt): 1e-4
relative on logits (measured <= 7e-6), 1e-5 on the loss (<= 2e-7). Gradients through ~36 layers with
train-mode BatchNorm over layers that hold only a handful of points are ill-conditioned: the CPU port
ALONE moves by up to 3e-2 (max-relative) between float32 and float64 on this input, so the end-to-end
gradient check is per parameter tensor a cosine > 0.999 (measured 1 - cos <= 2e-4) and a norm ratio within
3 % (measured <= 0.94 %, the deformable + modulated late-fusion net); the tight 1e-4 gradient checks are
the per-layer golden tests in test_gpu_parity.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _run(variant, deformable=False, modulated=False, spheres=1, nv=3, radius=0.6, density=2500.0, hw=(60, 80),
         gradients=True):
    import mvkpconv
    from oracle import torch_port
    from util import check_err
    tag = "%s%s%s x%d nv%d r%.1f" % (variant, " deform" if deformable else "", " mod" if modulated else "", spheres, nv, radius)
    syn = mvkpconv.sub("synthetic")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    np.random.seed(0)
    cfg = syn.make_config(variant, deformable=deformable, modulated=modulated)
    sph = [syn.raw_sphere(seed=i, radius=radius, density=density) if density else syn.raw_sphere(seed=i, radius=radius)
           for i in range(spheres)]
    views = [syn.sphere_views(s, nv=nv, h=hw[0], w=hw[1]) for s in sph] if variant != "baseline" else None
    staged = syn.stage_spheres(sph, dev, views)
    limits = syn.calibrate_limits(cfg, staged)
    batch, lens = syn.build_batch(cfg, staged, limits, torch.int64)
    net = syn.build_model(cfg, dev)
    net.train()
    seen = {}
    if hasattr(net, "net_2d"):
        for m in net.net_2d._modules.values():
            m.train(False)
        net.net_2d.register_forward_hook(lambda m, i, o: seen.__setitem__("f", o["feature"].detach().cpu()))
    if deformable:      # non-trivial offsets
        with torch.no_grad():
            for n, p in net.named_parameters():
                if n.endswith("offset_bias"):
                    p.normal_(0, 0.05)
    out = net(batch, cfg)
    loss = net.loss(out, batch.labels)
    if gradients:
        loss.backward()
    sd = {k: v.detach().cpu() for k, v in net.state_dict().items()}
    leaf = {k: sd[k].clone().requires_grad_(True) for k, p in net.named_parameters() if p.requires_grad}
    sdl = dict(sd)
    sdl.update(leaf)
    cb = torch_port.batch_to_cpu(batch)
    if "f" in seen:
        cb["feature_2d"] = seen["f"]
    ref, reg = torch_port.forward(sdl, cfg, cb, None, True)
    ref_loss = torch_port.loss_fn(ref, cb["labels"], reg, cfg)
    rel = lambda a, b: (a - b).abs().max().item() / max(b.abs().max().item(), 1e-12)
    check_err("network %s (%d points): logits vs CPU port" % (tag, lens[0]), rel(out.detach().cpu(), ref.detach()), 1e-4)
    check_err("network %s: loss vs CPU port (rel)" % tag, abs(loss.item() - ref_loss.item()) / max(1.0, abs(ref_loss.item())), 1e-5)
    if not gradients:
        return net
    ref_loss.backward()
    pairs = []
    for name, p in net.named_parameters():
        if not p.requires_grad:
            continue
        g_ref = leaf[name].grad
        if p.grad is None or g_ref is None:
            other = g_ref if p.grad is None else p.grad
            assert other is None or other.abs().max() == 0, name
            continue
        pairs.append((name, p.grad.cpu().reshape(-1).double(), g_ref.reshape(-1).double()))
    assert len(pairs) > 50
    scale = max(b.norm().item() for _, _, b in pairs)
    A, Bv = torch.cat([a for _, a, _ in pairs]), torch.cat([b for _, _, b in pairs])
    check_err("network %s: 1 - cosine of the whole gradient" % tag, 1.0 - (A @ Bv).item() / (A.norm().item() * Bv.norm().item()), 5e-4)
    worst_cos, worst_ratio = 0.0, 0.0
    for name, a, b in pairs:
        if b.norm().item() < 1e-3 * scale:
            # analytically ~0 gradients (e.g. a BatchNorm bias whose shift the next BatchNorm removes):
            # rounding noise only, bounded in absolute terms
            assert (a - b).norm().item() < 1e-3 * scale, name
            continue
        cos = (a @ b).item() / (a.norm().item() * b.norm().item())
        ratio = a.norm().item() / b.norm().item()
        worst_cos, worst_ratio = max(worst_cos, 1 - cos), max(worst_ratio, abs(ratio - 1))
        assert cos > 0.999 and abs(ratio - 1) < 3e-2, "%s grad cos %.6f norm ratio %.4f" % (name, cos, ratio)
    check_err("network %s: worst per-parameter 1 - cosine" % tag, worst_cos, 1e-3)
    check_err("network %s: worst per-parameter |norm ratio - 1|" % tag, worst_ratio, 3e-2)
    return net


@pytest.mark.parametrize("variant", ["baseline", "early", "middle", "late"])
def test_rigid_networks_vs_cpu_port(variant):
    _run(variant)


def test_two_spheres_stacked_batch():
    _run("early", spheres=2)


def test_three_spheres_one_gather_feature_aggregation_vs_cpu_port():
    """The reference's batch shape (several spheres stacked, train_ScanNet_sphere.py:232 batch_num = 5): FeatureAggregation
    as ONE gather over the stacked points of all spheres (fusion_common.lift_2d_features), BatchNorm statistics over all
    sum(np) * k rows like mvpnet_3d.py:54-61 over the concatenated grouped tensors (architectures_sphere.py:278-283) --
    three ragged spheres, late fusion (the variant that trains through the module), against the CPU port, which runs the
    reference's per-sphere group_points loop."""
    _run("late", spheres=3)


def test_deformable_middle_fusion_vs_cpu_port():
    _run("middle", deformable=True)


def test_deformable_modulated_late_fusion_vs_cpu_port():
    _run("late", deformable=True, modulated=True)


def test_five_view_middle_fusion_vs_cpu_port():
    """BASELINE configs[3]'s per-rank workload (middle fusion, deformable architecture, FIVE views) against the CPU
    port: logits, loss, gradients."""
    _run("middle", deformable=True, nv=5)


def test_full_size_early_fusion_forward_vs_cpu_port():
    """BASELINE configs[2] at its own size -- one ~19.5 k-point sphere (radius 1.2), 3 views of 120 x 160 -- through the
    HIP path against the unfused CPU port on the same weights: logits and loss (the forward only: the port's backward
    at this size takes minutes; gradients are covered at 2.3 k points above and per layer in test_gpu_parity.py)."""
    net = _run("early", radius=1.2, density=None, hw=(120, 160), gradients=False)
    assert net is not None


def test_full_size_late_fusion_deformable_40k_forward_vs_cpu_port():
    """BASELINE configs[4]'s geometry (late fusion, deformable + modulated, sphere of radius 1.7: ~55 k points on the
    synthetic room) forward against the CPU port, f32."""
    _run("late", deformable=True, modulated=True, radius=1.7, density=None, hw=(120, 160), gradients=False)


def test_network_without_batch_norm_deferred_weight_gradients_equal_inline_ones():
    """config.use_batch_norm = False (BatchNormBlock = a learned bias, models/blocks.py:462-463): the residual join then
    runs through ops.add_lrelu, and plain additions hand the SAME gradient tensor to both branches of a block. The
    fan-out sum inside unary1's backward GEMM must not add onto such a tensor in place while it is the operand of a
    recorded weight-gradient product: the gradients of a backward inside ops.defer_weight_grads() equal
    those of a plain backward, and both follow the CPU port."""
    import mvkpconv
    from oracle import torch_port
    from util import check_err
    syn, ops = mvkpconv.sub("synthetic"), mvkpconv.sub("ops")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    np.random.seed(0)
    cfg = syn.make_config("baseline")
    cfg.use_batch_norm = False
    sph = [syn.raw_sphere(seed=1, radius=0.6, density=2500.0)]
    staged = syn.stage_spheres(sph, dev, None)
    limits = syn.calibrate_limits(cfg, staged)
    batch, lens = syn.build_batch(cfg, staged, limits, torch.int32)
    net = syn.build_model(cfg, dev)
    net.train()
    with torch.no_grad():                      # without normalisation the default initialisation blows the activations up
        for n, p in net.named_parameters():
            if n.endswith("weights") or n.endswith("mlp.weight"):
                p.mul_(0.5)
            if n.endswith(".bias"):
                p.normal_(0, 0.05)

    def grads(deferred):
        net.zero_grad(set_to_none=True)
        out = net(batch, cfg)
        loss = net.loss(out, batch.labels)
        if deferred:
            with ops.defer_weight_grads():
                loss.backward()
        else:
            loss.backward()
        return out.detach(), loss.item(), {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}

    out_a, loss_a, ga = grads(False)
    out_b, loss_b, gb = grads(True)
    assert set(ga) == set(gb) and len(ga) > 40
    scale = max(v.norm().item() for v in ga.values())
    worst = max(((ga[n] - gb[n]).norm().item() / max(ga[n].norm().item(), 1e-3 * scale), n) for n in ga)
    check_err("no-BN network: deferred vs in-line weight gradients (%s)" % worst[1], worst[0], 1e-4)
    sd = {k: v.detach().cpu() for k, v in net.state_dict().items()}
    leaf = {k: sd[k].clone().requires_grad_(True) for k, p in net.named_parameters() if p.requires_grad}
    sdl = dict(sd)
    sdl.update(leaf)
    ref, reg = torch_port.forward(sdl, cfg, torch_port.batch_to_cpu(batch), None, True)
    ref_loss = torch_port.loss_fn(ref, batch.labels.cpu(), reg, cfg)
    ref_loss.backward()
    rel = lambda a, b: (a - b).abs().max().item() / max(b.abs().max().item(), 1e-12)
    check_err("no-BN network: logits vs CPU port", rel(out_a.cpu(), ref.detach()), 1e-4)
    A = torch.cat([gb[n].cpu().reshape(-1).double() for n in sorted(gb)])
    B = torch.cat([leaf[n].grad.reshape(-1).double() for n in sorted(gb)])
    check_err("no-BN network: 1 - cosine of the whole (deferred) gradient vs CPU port", 1.0 - (A @ B).item() / (A.norm().item() * B.norm().item()), 5e-4)


@pytest.mark.parametrize("variant,spheres,deformable", [("early", 1, False), ("baseline", 2, False), ("late", 1, False),
                                                        ("late", 1, True)])
def test_deterministic_mode_step_is_bit_reproducible(variant, spheres, deformable):
    """ops.set_deterministic(True): ordered split reductions (csrc/gemm.hip), the feature gradients of the rigid
    convolutions, of max_pool and of the nearest upsampling as gathers over sorted reverse lists (csrc/revlist.hip), the
    bias gradients in workgroup order -- two runs of the same step on the same batch give the same BITS in the logits,
    the loss and every parameter gradient (the reference's CPU path is deterministic; the default mode here trades that
    for ~5 % of the step). Deformable + modulated variant (round 5): the feature gradients of the
    deformable convolutions and of their offset convolutions as gathers over SORTED reverse lists of the deform-radius
    relations (rows wider than 512: rev_sort_wide_kernel), the offset gradient in a fixed order (kpconv_deform_doff_mfma),
    the regulariser and the offset-bias gradient summed by one workgroup. The frozen 2D encoder's output enters as a fixed map (MIOpen is outside this
    library); the pyramid is built once per run from the same rotations."""
    import mvkpconv
    syn, ops = mvkpconv.sub("synthetic"), mvkpconv.sub("ops")
    dev = torch.device("cuda:0")
    ops.set_deterministic(True)
    try:
        torch.manual_seed(0)
        np.random.seed(0)
        cfg = syn.make_config(variant, deformable=deformable, modulated=deformable)
        sph = [syn.raw_sphere(seed=i, radius=0.7, density=3000.0) for i in range(spheres)]
        views = [syn.sphere_views(s, nv=3, h=60, w=80) for s in sph] if variant != "baseline" else None
        staged = syn.stage_spheres(sph, dev, views)
        limits = syn.calibrate_limits(cfg, staged)
        common = mvkpconv.sub("dropin.datasets.common")
        rots = [common.random_grid_rotations(spheres) for _ in range(4)]
        net = syn.build_model(cfg, dev)
        net.train()
        if hasattr(net, "net_2d"):
            for m in net.net_2d._modules.values():
                m.train(False)
        sd0 = {k: v.clone() for k, v in net.state_dict().items()}
        fmap = torch.randn(spheres * 3, 64, 60, 80, device=dev) if variant != "baseline" else None

        def run():
            net.load_state_dict(sd0)
            net.zero_grad(set_to_none=True)
            batch, _ = syn.build_batch(cfg, staged, limits, torch.int32, rotations=rots)
            assert batch.rev_neighbors[0] is not None and batch.rev_pools[0] is not None and batch.rev_ups
            if fmap is not None:
                batch.feature_2d = fmap
            out = net(batch, cfg)
            loss = net.loss(out, batch.labels)
            with ops.defer_weight_grads():
                loss.backward()
            return out.detach().clone(), loss.detach().clone(), {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}

        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("error")                      # a scatter without its reverse list would warn
            o1, l1, g1 = run()
            o2, l2, g2 = run()
        assert torch.equal(o1, o2), "logits differ between two runs: %g" % (o1 - o2).abs().max().item()
        assert torch.equal(l1, l2)
        assert set(g1) == set(g2) and len(g1) > 50
        bad = [n for n in g1 if not torch.equal(g1[n], g2[n])]
        assert not bad, "gradients differ between two runs: %s" % bad[:5]
    finally:
        ops.set_deterministic(False)


def test_sync_batchnorm_two_ranks_equal_one_rank_with_two_spheres(tmp_path):
    """SURVEY.md 8e / models/blocks.py:453-460: BatchNorm spans the stacked batch. With ops.set_sync_batchnorm the
    statistics of every BatchNorm (blocks and FeatureAggregation) are all-reduced, so TWO ranks with ONE sphere each
    (gloo, both on this card, tests/_syncbn_worker.py) compute what ONE rank computes on the two spheres stacked:
    logits 1e-4, loss 1e-5, parameter gradients (summed over the ranks, each rank's mean loss weighted by its share of
    the points) by the cosine / norm criteria of the stacked-batch tests, BatchNorm running statistics 1e-5. The default
    stays per-rank statistics."""
    import os
    import socket
    import subprocess
    import sys
    import mvkpconv
    from util import check_err
    syn = mvkpconv.sub("synthetic")
    common = mvkpconv.sub("dropin.datasets.common")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    np.random.seed(0)
    variant, seeds, radius, density = "early", [0, 1], 0.6, 2500.0
    cfg = syn.make_config(variant)
    sph = [syn.raw_sphere(seed=s, radius=radius, density=density) for s in seeds]
    views = [syn.sphere_views(s, nv=3, h=60, w=80) for s in sph]
    staged = syn.stage_spheres(sph, dev, views)
    limits = syn.calibrate_limits(cfg, staged)
    rots = [common.random_grid_rotations(2) for _ in range(4)]
    batch, lens = syn.build_batch(cfg, staged, limits, torch.int64, rotations=rots)
    net = syn.build_model(cfg, dev)
    net.train()
    for m in net.net_2d._modules.values():
        m.train(False)
    state = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    torch.save({"variant": variant, "seeds": seeds, "radius": radius, "density": density, "limits": limits,
                "rotations": rots, "state": state}, str(tmp_path / "meta.pt"))
    out = net(batch, cfg)
    loss = net.loss(out, batch.labels)
    loss.backward()
    ref_rm = net.encoder_blocks[3].batch_norm_conv.batch_norm.running_mean.cpu()
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    procs = [subprocess.Popen([sys.executable, os.path.join(root, "tests", "_syncbn_worker.py"), str(r), "2", str(port), str(tmp_path)],
                              env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
    logs = [p.communicate(timeout=300)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(l[-1500:] for l in logs)
    r0, r1 = (torch.load(str(tmp_path / ("rank%d.pt" % r)), weights_only=False) for r in range(2))
    assert [r0["n"], r1["n"]] == lens
    rel = lambda a, b: (a - b).abs().max().item() / max(b.abs().max().item(), 1e-12)
    got = torch.cat([r0["logits"], r1["logits"]], 0)
    check_err("SyncBN 2 ranks x 1 sphere vs 1 rank x 2 spheres: logits", rel(got, out.detach().cpu()), 1e-4)
    check_err("SyncBN: loss (abs)", abs(r0["loss"].item() - loss.item()), 1e-5)
    check_err("SyncBN: BatchNorm running mean", rel(r0["running_mean"], ref_rm), 1e-5)
    worst_cos = worst_ratio = 0.0
    pairs = [(n, r0["grads"][n].reshape(-1).double(), p.grad.cpu().reshape(-1).double())
             for n, p in net.named_parameters() if p.grad is not None]
    assert len(pairs) > 50 and set(n for n, _, _ in pairs) == set(r0["grads"])
    scale = max(b.norm().item() for _, _, b in pairs)
    for n, a, b in pairs:
        if b.norm().item() < 1e-3 * scale:
            assert (a - b).norm().item() < 1e-3 * scale, n
            continue
        worst_cos = max(worst_cos, 1 - (a @ b).item() / (a.norm().item() * b.norm().item()))
        worst_ratio = max(worst_ratio, abs(a.norm().item() / b.norm().item() - 1))
    check_err("SyncBN: worst per-parameter 1 - cosine", worst_cos, 1e-3)
    check_err("SyncBN: worst per-parameter |norm ratio - 1|", worst_ratio, 3e-2)


def test_state_dict_keys_follow_the_reference_names():
    net = _run("baseline")
    keys = set(net.state_dict().keys())
    for k in ("encoder_blocks.0.KPConv.weights", "encoder_blocks.0.KPConv.kernel_points",
              "encoder_blocks.0.batch_norm.batch_norm.weight", "encoder_blocks.1.unary1.mlp.weight",
              "encoder_blocks.1.batch_norm_conv.batch_norm.running_mean", "encoder_blocks.1.unary_shortcut.mlp.weight",
              "decoder_blocks.1.mlp.weight", "head_mlp.mlp.weight", "head_softmax.batch_norm.bias"):
        assert k in keys, k


@pytest.mark.parametrize("variant,deformable", [("early", False), ("late", True)])
def test_capacity_padded_mode_equals_plain_mode(variant, deformable):
    """Capacity-padded levels + masked BatchNorm (the hipGraph replay layout) give the same logits
    and gradients as the plain layout, on the valid rows (rigid and deformable + modulated)."""
    import mvkpconv
    syn, ops = mvkpconv.sub("synthetic"), mvkpconv.sub("ops")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    np.random.seed(0)
    cfg = syn.make_config(variant, deformable=deformable, modulated=deformable)
    sph = [syn.raw_sphere(seed=3, radius=0.8, density=3000.0)]
    views = [syn.sphere_views(s, nv=3, h=60, w=80) for s in sph]
    staged = syn.stage_spheres(sph, dev, views)
    limits = syn.calibrate_limits(cfg, staged)
    batch, lens = syn.build_batch(cfg, staged, limits, torch.int32)
    net = syn.build_model(cfg, dev)
    net.train()
    for m in net.net_2d._modules.values():
        m.train(False)
    sd0 = {k: v.clone() for k, v in net.state_dict().items()}

    def run(b):
        net.load_state_dict(sd0)
        net.zero_grad(set_to_none=True)
        out = net(b, cfg)
        loss = net.loss(out, b.labels)
        loss.backward()
        return out.detach().clone(), loss.item(), {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}

    o1, l1, g1 = run(batch)
    if deformable:
        with torch.no_grad():
            for n, p in net.named_parameters():
                if n.endswith("offset_bias"):
                    p.normal_(0, 0.05)
        sd0 = {k: v.clone() for k, v in net.state_dict().items()}
        o1, l1, g1 = run(batch)
    rm1 = net.encoder_blocks[3].batch_norm_conv.batch_norm.running_mean.clone()
    static = syn.StaticBatch(batch, limits)
    assert any(c > p.shape[0] for c, p in zip(static.caps[1:], batch.points[1:]))      # really padded
    ops.set_row_counts(static.valid)
    try:
        o2, l2, g2 = run(static)
        rm2 = net.encoder_blocks[3].batch_norm_conv.batch_norm.running_mean.clone()
    finally:
        ops.set_row_counts(None)
    rel = lambda a, b: (a - b).abs().max().item() / max(b.abs().max().item(), 1e-12)
    assert rel(o2[:o1.shape[0]], o1) < 1e-4 and abs(l1 - l2) < 1e-5 * max(1.0, abs(l1))
    assert rel(rm2, rm1) < 1e-5
    A = torch.cat([g2[k].reshape(-1) for k in g1]).double()
    B = torch.cat([g1[k].reshape(-1) for k in g1]).double()
    assert (A @ B).item() / (A.norm().item() * B.norm().item()) > 0.9999


@pytest.mark.parametrize("variant,deformable,nspheres", [("early", False, 1), ("late", True, 2), ("baseline", False, 3)])
def test_device_input_chain_equals_eager_input_side(variant, deformable, nspheres):
    """The sync-free, capturable input chain (device-side counts, fixed launch geometry) fills a static
    batch with exactly what build_batch + StaticBatch.load put there: points, counts, the 13 index
    matrices, 3-NN indices, unprojected pixels -- for the same grid rotations, one or several spheres."""
    import mvkpconv
    syn, ops = mvkpconv.sub("synthetic"), mvkpconv.sub("ops")
    common = mvkpconv.sub("dropin.datasets.common")
    dev = torch.device("cuda:0")
    cfg = syn.make_config(variant, deformable=deformable, modulated=deformable)
    sph = [syn.raw_sphere(seed=20 + i, radius=0.7 + 0.1 * i, density=3000.0) for i in range(nspheres)]
    views = [syn.sphere_views(s, nv=3, h=60, w=80) for s in sph] if variant != "baseline" else None
    staged = syn.stage_spheres(sph, dev, views)
    limits = syn.calibrate_limits(cfg, staged)
    rng = np.random.RandomState(4)
    rots = [common.random_grid_rotations(nspheres, rng) for _ in range(4)]
    batch, _ = syn.build_batch(cfg, staged, limits, torch.int32, rotations=rots)
    want = syn.StaticBatch(batch, limits)
    got = syn.StaticBatch(batch, limits, caps=want.caps)
    for tl in (got.points[1:], got.neighbors, got.pools[:-1], got.upsamples[:-1], [o for o in got.orders if o is not None]):
        for x in tl:
            x.fill_(-12345)                                           # everything must be rewritten
    chain = syn.DeviceInputChain(cfg, staged, limits, got)
    for _ in range(2):                                               # twice: the chain must be re-runnable as is
        chain.draw_rotations(rots)
        chain.build(got)
    assert ops.check_neighbor_status(chain.status) >= max(limits[:1])
    L = len(want.points)
    for l in range(L):
        assert torch.equal(got.points[l], want.points[l]), l
        assert torch.equal(got._counts[l], want._counts[l]), l
        assert torch.equal(got.neighbors[l], want.neighbors[l]), l
        if l + 1 < L:
            assert torch.equal(got.pools[l], want.pools[l]) and torch.equal(got.upsamples[l], want.upsamples[l]), l
        assert (got.orders[l] is None) == (want.orders[l] is None), l          # the gather's work lists
        if want.orders[l] is not None:
            assert torch.equal(got.orders[l], want.orders[l]), l
            assert torch.equal(torch.sort(got.orders[l]).values, got._iota[l]), l
    for name in syn.StaticBatch._DENSE:
        a, b = getattr(got, name), getattr(want, name)
        assert (a is None) == (b is None) and (a is None or torch.equal(a, b)), name
    if want.knn_list is not None:
        for a, b in zip(got.knn_list, want.knn_list):
            assert torch.equal(a, b)
    # the transposed matrices the searches filled on the way (round 5: slots taken inside nb_query_kernel, one finishing
    # launch per pyramid): every row holds exactly the query rows whose list names that support (any order: arrival),
    # the tail is the shadow value, the counters are back at zero -- against the stand-alone two-launch form, sorted
    ops.check_reverse_status(chain.rev_status)
    checked = 0
    for revs, mats, qcap in ((got.rev_neighbors, got.neighbors, lambda l: got.caps[l]),
                             (got.rev_pools, got.pools, lambda l: got.caps[min(l + 1, L - 1)])):
        for l, rev in enumerate(revs or []):
            if rev is None:
                continue
            ref = ops.reverse_neighbors(mats[l], got.caps[l], width=rev.shape[1], shadow=qcap(l), sort=True)
            assert torch.equal(torch.sort(rev, dim=1).values, torch.sort(ref, dim=1).values), l
            checked += 1
    assert checked >= (0 if deformable else 5)
    for buf in getattr(chain, "_rev_count_pool", {}).values():
        assert int(buf.abs().sum()) == 0


@pytest.mark.parametrize("device_chain,fork", [(False, None), (True, None), (True, "-1"), (True, "1")])
def test_graph_replay_trains_like_eager(device_chain, fork, monkeypatch):
    """bench.py's hipGraph step (capacity-padded static batch, masked BatchNorm, input pyramid one batch
    ahead on a second stream) follows the same trajectory as plain eager steps: with the grid rotations
    pinned (so every batch is identical) the losses and the weights after 5 optimizer steps agree. fork: where the side
    branches leave the network's chain (step.py MVK_SIDE_AFTER_BLOCK; None = the default for one sphere: after encoder
    block 3; "-1" = at the step's start, as for batches of more than two spheres; "1" with the encoder two blocks later)."""
    import types
    if fork is not None:
        monkeypatch.setenv("MVK_SIDE_AFTER_BLOCK", fork)
        if fork == "1":
            monkeypatch.setenv("MVK_ENC_AFTER_BLOCK", "3")
    import mvkpconv
    bench = mvkpconv.sub("step")          # the step executor lives in the package since round 5 (was bench.py)
    syn, ops = mvkpconv.sub("synthetic"), mvkpconv.sub("ops")
    dev = torch.device("cuda:0")
    torch.cuda.set_stream(torch.cuda.Stream())
    cfg = syn.make_config("early")
    sph = [syn.raw_sphere(seed=5, radius=0.8, density=3000.0)]
    views = [syn.sphere_views(s, nv=3, h=60, w=80) for s in sph]
    staged = syn.stage_spheres(sph, dev, views)
    limits = syn.calibrate_limits(cfg, staged)
    rots = [np.stack([np.eye(3, dtype=np.float32)]) for _ in range(4)]
    shim = types.SimpleNamespace(StaticBatch=syn.StaticBatch,
                                 build_batch=lambda c, st, lim, dt, **kw: syn.build_batch(c, st, lim, dt, rotations=rots, **kw))
    if device_chain:        # the input side as a captured branch of the graph (device-side counts)
        class PinnedChain(syn.DeviceInputChain):
            def draw_rotations(self, rotations=None, upload=True):
                super().draw_rotations(rots, upload=upload)
        shim.DeviceInputChain = PinnedChain

    def make():
        torch.manual_seed(0)
        np.random.seed(0)
        net = syn.build_model(cfg, dev)
        net.train()
        for m in net.net_2d._modules.values():
            m.train(False)
        params = [p for p in net.parameters() if p.requires_grad]
        opt = torch.optim.SGD(params, lr=1e-3, momentum=0.9, weight_decay=1e-3)
        return net, params, opt

    try:
        net, params, opt = make()
        losses_e = []
        for _ in range(5):
            batch, _ = shim.build_batch(cfg, staged, limits, torch.int32)
            opt.zero_grad(set_to_none=True)
            losses_e.append(bench.net_step_captured(net, batch, cfg, params, opt, None).item())
        w_e = torch.cat([p.detach().reshape(-1) for p in params]).clone()
        net, params, opt = make()
        import warnings
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            held = bench.net_step_captured(net, shim.build_batch(cfg, staged, limits, torch.int32)[0], cfg, params, opt, None)
            # `held` keeps an eager autograd graph (and its AccumulateGrad nodes) alive across the capture, like the
            # loss of bench.py's warm-up: the capture must run on the same stream as that backward did
            step, note = bench.make_graph_step(shim, ops, cfg, net, staged, limits, params, opt, None)   # 2 eager steps inside
            assert note[0].startswith("hipGraph")
            losses_g = [step()[1].item() for _ in range(2)]
            torch.cuda.synchronize()
        assert not [w for w in caught if "AccumulateGrad" in str(w.message)], "stream mismatch between eager and captured backward"
        del held
        w_g = torch.cat([p.detach().reshape(-1) for p in params])
        assert np.allclose(losses_g, losses_e[3:], rtol=2e-3), (losses_g, losses_e)
        assert ((w_g - w_e).norm() / w_e.norm()).item() < 1e-3
    finally:
        ops.set_row_counts(None)
        ops.zero_arena_disable()
        torch.cuda.synchronize()
        torch.cuda.set_stream(torch.cuda.default_stream())


def test_graph_capture_refuses_the_default_stream():
    """Guard of the round-1 abort (segfault in capture_end): make_graph_step under the legacy default stream must
    raise instead of starting a capture that cannot succeed."""
    import mvkpconv
    bench = mvkpconv.sub("step")
    torch.cuda.set_stream(torch.cuda.default_stream())
    staged = {"points": [torch.zeros(4, 3, device="cuda")]}
    with pytest.raises(RuntimeError, match="non-default stream"):
        bench.make_graph_step(mvkpconv.sub("synthetic"), mvkpconv.sub("ops"), None, torch.nn.Linear(2, 2).cuda(), staged, None,
                              [], None, None)


def test_bench_emits_one_valid_json_line(tmp_path):
    """bench.py end to end (default workload, few steps), once plain and once with --full: exactly one JSON line on
    stdout carrying the contract's keys, no capacity overflow; with --full also the roofline and cpu_baseline objects
    and the detail file, without it neither. --dump-outputs writes the last timed step's loss and the network state it
    left, float32 / float64, within 64 MB. The plain run dumps what the full run does -- both time the same steps -- within
    the bounds of two runs of one command (test_bench_dump_outputs_are_the_same_in_two_runs)."""
    import glob
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

    def run(kind, *extra):
        dump, detail = str(tmp_path / ("outputs_" + kind)), str(tmp_path / ("detail_" + kind + ".json"))
        p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--steps", "3", "--warmup", "1",
                            "--dump-outputs", dump] + list(extra),
                           capture_output=True, text=True, timeout=300, cwd=root, env=dict(os.environ, MVK_BENCH_DETAIL=detail))
        assert p.returncode == 0, p.stderr[-2000:]
        lines = [l for l in p.stdout.splitlines() if l.strip()]
        assert len(lines) == 1, p.stdout[-2000:]
        assert len(lines[0]) < 4096, len(lines[0])      # the driver's consumer keeps a bounded tail (BENCH_r02 was not parsed)
        d = json.loads(lines[0])
        for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                  "vs_baseline", "dtype", "data", "config"):
            assert k in d, k
        assert d["n_gpus"] == 1 and d["steps"] == 3 and d["unit"] == "points/s" and d["vs_baseline"] is None
        assert d["value"] > 5e4 and d["config"]["execution"].startswith("hipGraph") and d["config"]["capacity_overflow"] is False
        files = glob.glob(os.path.join(dump, "*.npy"))
        assert sum(os.path.getsize(f) for f in files) <= 64e6
        out = {os.path.basename(f)[:-4]: np.load(f) for f in files}
        assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in out.values())
        assert abs(float(out["loss"][0]) - d["config"]["final_loss"]) <= 1e-5 * abs(d["config"]["final_loss"])     # (6 digits)
        assert float(out["lens"].sum()) == d["config"]["points_per_step_per_gpu"]
        assert any(n.startswith("state.") and n.endswith("KPConv.weights") for n in out)
        return d, out, detail

    plain, plain_out, plain_detail = run("plain")
    d, full_out, detail_path = run("full", "--full")
    for k in ("roofline", "cpu_baseline"):
        assert k in d, k
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-5     # (6 significant digits in the line)
    assert r["kernel"].startswith("kpconv_gather_") and 0.2 < r["frac"] < 1.0
    detail = json.load(open(detail_path))
    assert detail["line"]["value"] == d["value"] and len(detail["detail"]["gather_launches"]) >= 5
    c = d["cpu_baseline"]
    assert c["kind"] in ("port", "reference") and c["unit"] == "points/s" and c["cores"] >= 1 and c["value"] > 0

    assert not {"roofline", "contraction", "cpu_baseline"} & set(plain) and not os.path.exists(plain_detail)
    assert plain["config"]["points_per_step_per_gpu"] == d["config"]["points_per_step_per_gpu"]
    assert sorted(plain_out) == sorted(full_out)
    for n, b in full_out.items():
        a, b = plain_out[n].astype(np.float64), b.astype(np.float64)
        assert a.shape == b.shape, n
        bound = 1e-6 * abs(float(b[0])) if n == "loss" else 1e-4 * np.abs(b).max() + 1e-7
        assert not a.size or np.abs(a - b).max() <= bound, (n, float(np.abs(a - b).max()), bound)


def test_bench_dump_outputs_are_the_same_in_two_runs(tmp_path):
    """Two runs of bench.py with the same arguments dump the same outputs up to the rounding of one step: the dumped step
    starts from the seeded network and a fresh optimiser (the trained state of two runs is not the same -- see bench.py).
    The loss within 1e-6; every other array within 1e-4 of its largest element plus 1e-7: in one step a LeakyReLU input
    within an ulp of zero (float-atomic sums) may take the other slope in the backward and change a weight gradient's
    terms of that row (measured: 1e-5 of a KPConv weight array after the step's learning rate), and a BatchNorm bias after
    its first step is the learning rate times a sum that cancels to ~1e-4 of its terms (last bits 1e-8 apart)."""
    import glob
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    dumps = [str(tmp_path / ("run%d" % i)) for i in range(2)]
    for d in dumps:
        p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--steps", "2", "--warmup", "1", "--no-cpu-baseline",
                            "--no-eager-line", "--dump-outputs", d],
                           capture_output=True, text=True, timeout=240, cwd=root,
                           env=dict(os.environ, MVK_BENCH_DETAIL=str(tmp_path / "detail.json")))
        assert p.returncode == 0, p.stderr[-2000:]
    names = sorted(os.path.basename(f) for f in glob.glob(os.path.join(dumps[0], "*.npy")))
    assert names and names == sorted(os.path.basename(f) for f in glob.glob(os.path.join(dumps[1], "*.npy")))
    worst = []
    for n in names:
        a, b = (np.load(os.path.join(d, n)).astype(np.float64) for d in dumps)
        assert a.shape == b.shape, n
        bound = 1e-6 * abs(float(b[0])) if n == "loss.npy" else 1e-4 * np.abs(b).max() + 1e-7
        excess = np.abs(a - b).max() - bound if a.size else -1.0
        worst.append((excess, n))
    assert max(worst)[0] <= 0, sorted(worst)[-5:]


def test_dataloader_workers_build_the_pyramid_without_forking(tmp_path):
    """n2 on the GPU box: a DataLoader created like the reference script's (num_workers=2, no multiprocessing_context)
    AFTER the parent has initialised the GPU; the drop-in's `datasets` package has made `spawn` the default, so both
    workers build their pyramids with the HIP library in their own contexts. Level-0 neighbours (independent of the
    random grid orientation) must equal the parent's own search; the whole list has the reference's 5*L + 2 layout."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = "enhancing-3d-point-cloud-segmentation-using-multi-modal-fusion-with-2d-images_amd"
    (tmp_path / "workerds.py").write_text(
        "import numpy as np\n"
        "from datasets.common import PointCloudDataset\n"
        "def first(b):\n"
        "    return b[0]                      # (spawned workers unpickle the collate function: module level, like ScanNetCollate)\n"
        "class DS(PointCloudDataset):\n"
        "    def __init__(self, fields, limits):\n"
        "        PointCloudDataset.__init__(self, 'w')      # self.config = the (picklable, module-level) Config class\n"
        "        self.config.__dict__.update(fields)\n"
        "        self.neighborhood_limits = limits\n"
        "    def __len__(self):\n"
        "        return 4\n"
        "    def __getitem__(self, i):\n"
        "        rng = np.random.default_rng(i)\n"
        "        pts = (rng.random((3000, 3)) * [1.6, 1.6, 0.4]).astype(np.float32)\n"
        "        feats = np.ones((3000, 1), np.float32)\n"
        "        labels = rng.integers(0, 20, 3000).astype(np.int64)\n"
        "        return self.segmentation_inputs(pts, feats, labels, np.array([3000], np.int32)) + [np.int64(i)]\n")
    script = tmp_path / "train_like.py"
    script.write_text(
        "import os, sys\n"
        "sys.path.insert(0, %r); sys.path.append(%r); sys.path.append(%r)\n"
        "import numpy as np, torch\n"
        "from torch.utils.data import DataLoader\n"
        "import datasets.common as DC\n"
        "import workerds\n"
        "if __name__ == '__main__':\n"
        "    import mvkpconv\n"
        "    syn = mvkpconv.sub('synthetic')\n"
        "    cfg = syn.make_config('baseline')\n"
        "    x = torch.zeros(8, device='cuda'); torch.cuda.synchronize()      # the parent owns a HIP context\n"
        "    limits = [30, 30, 30, 30, 30]\n"
        "    fields = {k: getattr(cfg, k) for k in ('architecture', 'first_subsampling_dl', 'conv_radius', 'deform_radius', 'num_layers')}\n"
        "    ds = workerds.DS(fields, limits)\n"
        "    loader = DataLoader(ds, batch_size=1, num_workers=2, collate_fn=workerds.first)\n"
        "    seen = 0\n"
        "    for flat in loader:\n"
        "        L = (len(flat) - 3) // 5\n"
        "        assert L == 5 and 5 * L + 3 == len(flat), len(flat)\n"
        "        i = int(flat[-1])\n"
        "        rng = np.random.default_rng(i)\n"
        "        pts = (rng.random((3000, 3)) * [1.6, 1.6, 0.4]).astype(np.float32)\n"
        "        assert np.array_equal(flat[0], pts) and flat[L].dtype == np.int64 and flat[L].shape[0] == 3000\n"
        "        own = DC.batch_neighbors(torch.from_numpy(pts).cuda(), torch.from_numpy(pts).cuda(), np.array([3000], np.int32),\n"
        "                                 np.array([3000], np.int32), cfg.first_subsampling_dl * cfg.conv_radius, limit=30)\n"
        "        assert np.array_equal(own.cpu().numpy(), flat[L]), 'worker pyramid differs from the parent search'\n"
        "        assert flat[1].shape[0] > 100 and flat[4].shape[0] > 0 and flat[2 * L].shape[0] == flat[1].shape[0]\n"
        "        seen += 1\n"
        "    assert seen == 4\n"
        "    print('WORKER PYRAMIDS OK')\n" % (os.path.join(root, pkg, "dropin"), str(tmp_path), root))
    env = dict(os.environ)
    env.pop("MVK_DATALOADER_START", None)
    r = subprocess.run([sys.executable, str(script)], cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "WORKER PYRAMIDS OK" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])


def test_frozen_encoder_two_batches_in_one_call_equal_two_calls():
    """bench.py runs the frozen 2D encoder for the views of TWO upcoming batches in one call on every second step
    (MVK_ENCODER_PAIR): a batch's feature map must not depend on what else is in the call -- eval-mode BatchNorm folded
    into the convolutions, no cross-image operation; the library may pick other convolution plans for six views than
    for three, so the bound is the rounding class of an f32 convolution stack, not bit equality."""
    import mvkpconv
    from util import check_err
    syn = mvkpconv.sub("synthetic")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    net = syn.build_model(syn.make_config("early"), dev)
    net.net_2d.eval()
    g = torch.Generator(device="cpu").manual_seed(5)
    a = torch.rand(3, 3, 120, 160, generator=g).to(dev)
    b = torch.rand(3, 3, 120, 160, generator=g).to(dev)
    with torch.no_grad():
        fa = net.net_2d({'image': a})['feature']
        fb = net.net_2d({'image': b})['feature']
        both = net.net_2d({'image': torch.cat([a, b], 0)})['feature']
    assert both.shape[0] == 6 and both.shape[1:] == fa.shape[1:]
    scale = float(fa.abs().max())
    check_err("frozen encoder: views 0-2 of a six-view call vs a three-view call (max abs / max)",
              float((both[:3] - fa).abs().max()) / scale, 2e-5)
    check_err("frozen encoder: views 3-5 of a six-view call vs a three-view call (max abs / max)",
              float((both[3:] - fb).abs().max()) / scale, 2e-5)


def test_default_multi_gpu_step_structure_trains_like_the_single_graph_step():
    """The DEFAULT N > 1 step (three graphs -- forward + backward above the cut + pack | backward below the cut + pack |
    unpack + clip + SGD -- with eager RCCL all-reduces between them, bench.py make_graph_step) rehearsed with a one-rank
    RCCL group (MVK_BENCH_FORCE_DP=1) must train like the single-graph N = 1 step: same seeds, same spheres, same grid
    orientations => the loss after warm-up + 16 instrumented + 2 + 3 SGD steps agrees to the rounding of the float
    atomics (two single-graph runs differ by the same order; the measured differences are printed)."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

    def run(extra_env):
        env = dict(os.environ, MVK_BENCH_DETAIL=os.path.join(root, "gpurun_out", "bench_detail_test.json"), **extra_env)
        # (240 s: a run takes ~15 s; a hung child must end as a failure with its stderr, not as a silent test process)
        p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--steps", "3", "--warmup", "1", "--no-cpu-baseline"],
                           capture_output=True, text=True, timeout=240, cwd=root, env=env)
        assert p.returncode == 0, p.stderr[-2000:]
        return json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])

    one = run({})
    plain = run({"MVK_SPLIT_TAIL": "1"})           # opt-in: grouped dW + SGD of everything above the backward cut on a side branch
    dp = run({"MVK_BENCH_FORCE_DP": "1", "MASTER_PORT": "29531"})
    unpaired = run({"MVK_ENCODER_PAIR": "0"})      # the frozen encoder once per step (default: two batches on every second step)
    tag = "hipGraph[net|chain|enc2d(x2 every 2nd step)+fa]"
    assert one["config"]["execution"] == tag and one["config"]["backend"] is None
    assert unpaired["config"]["execution"] == "hipGraph[net|chain|enc2d+fa]"
    assert dp["config"]["execution"] == tag + "+eager-rccl(3 graphs)", dp["config"]["execution"]
    assert dp["config"]["backend"] == "rccl" and dp["config"]["ranks"] == 1
    assert not one["config"]["capacity_overflow"] and not dp["config"]["capacity_overflow"]
    a, b, c = one["config"]["final_loss"], dp["config"]["final_loss"], plain["config"]["final_loss"]
    print("final loss: single graph %.6f (tail on a side branch %.6f) | three graphs + eager RCCL %.6f | rel diff %.2e / %.2e"
          % (a, c, b, abs(a - c) / abs(a), abs(a - b) / abs(a)))
    assert abs(a - b) < 2e-3 * abs(a) and abs(a - c) < 2e-3 * abs(a)
    d = unpaired["config"]["final_loss"]           # same features batch by batch (other convolution plans for six views: rounding)
    print("final loss with the encoder once per step %.6f | rel diff %.2e" % (d, abs(a - d) / abs(a)))
    assert abs(a - d) < 2e-3 * abs(a)


def test_two_stage_backward_with_deformable_blocks_below_the_cut_and_deferred_weight_gradients():
    """dp.two_stage_backward with the cut INSIDE the deformable part of the encoder, every stage under
    ops.defer_weight_grads: stage 1 already gives the blocks below the cut a gradient through the regulariser (offset
    branch; a zero feature-path product for the outer weights), stage 2 then ACCUMULATES onto those .grad tensors --
    their products must run in line (not deferred into memory autograd has already consumed). Gradients must equal a
    plain loss.backward() of the same network and batch."""
    import mvkpconv
    syn, ops, dp = mvkpconv.sub("synthetic"), mvkpconv.sub("ops"), mvkpconv.sub("dp")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    np.random.seed(0)
    cfg = syn.make_config("baseline", deformable=True)
    sph = [syn.raw_sphere(seed=3, radius=0.6, density=2500.0)]
    staged = syn.stage_spheres(sph, dev, None)
    limits = syn.calibrate_limits(cfg, staged)
    batch, _ = syn.build_batch(cfg, staged, limits, torch.int32)
    net = syn.build_model(cfg, dev)
    net.train()
    with torch.no_grad():
        for n, p in net.named_parameters():
            if n.endswith("offset_bias"):
                p.normal_(0, 0.05)
    first_deform = min(i for i, b in enumerate(cfg.architecture) if "deformable" in b)
    cut = first_deform + 2                       # two deformable blocks stay below the cut
    assert "deformable" in cfg.architecture[cut - 1] and "deformable" in cfg.architecture[cut]
    sd = {k: v.clone() for k, v in net.state_dict().items()}

    def grads(two_stage):
        net.load_state_dict(sd)
        net.zero_grad(set_to_none=True)
        net.backward_cut = cut if two_stage else None
        loss = net.loss(net(batch, cfg), batch.labels)
        if two_stage:
            assert dp.deformable_below(cfg.architecture, cut) and not dp.deformable_below(cfg.architecture, first_deform)
            dp.two_stage_backward(loss, net.cut_tensors, backward_scope=ops.defer_weight_grads, retain_graph=True)
        else:
            loss.backward()
        torch.cuda.synchronize()
        net.backward_cut = None
        return {n: p.grad.detach().clone() for n, p in net.named_parameters() if p.grad is not None}, loss.item()

    # Every product unsplit for this comparison: a split reduction adds its partial sums with float atomics in a
    # run-dependent order, the last bit of a pre-activation then differs from run to run, and an element within an ulp
    # of the LeakyReLU kink takes the other slope -- two plain backward passes of this very network differ by up to
    # 1e-2 in the rows of head_mlp.mlp.weight that such an element feeds (tools/debug_two_stage.py). With one
    # workgroup per output tile the forward is bit-reproducible and the two schedules can be compared tightly.
    import os
    old_force = os.environ.get("MVK_GEMM_FORCE")
    os.environ["MVK_GEMM_FORCE"] = "2,1,1"
    try:
        want, l0 = grads(False)
        got, l1 = grads(True)
    finally:
        if old_force is None:
            os.environ.pop("MVK_GEMM_FORCE", None)
        else:
            os.environ["MVK_GEMM_FORCE"] = old_force
    assert abs(l0 - l1) < 1e-6 * abs(l0) and set(want) == set(got)
    below = [n for n in want if n.startswith("encoder_blocks.%d." % (cut - 1))]
    assert any("offset_conv.weights" in n for n in below) and any(n.endswith("KPConv.weights") for n in below)
    scale = max(v.abs().max().item() for v in want.values())
    worst = max(((got[n] - want[n]).abs().max().item() / max(want[n].abs().max().item(), 1e-3 * scale), n) for n in want)
    from util import check_err
    check_err("two-stage + deferred dW vs plain backward, worst parameter (%s)" % worst[1], worst[0], 1e-4)
