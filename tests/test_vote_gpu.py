"""GPU: test-time voting on the device (csrc/vote.hip, dropin/utils/tester.py) and the frozen inference forward
(models.blocks.freeze_inference) against the NumPy restatements of tests/vote_ref.py.

Comparison rules:
* probabilities in, float64 votes out: BIT equality (two float64 products and one sum per element, no FMA);
* logits in: the referee rule of tests/util.py with the floor of one float32 spacing below 1 --
      l2_err(device votes, float64 restatement with float64 softmax) <= REFEREE_FACTOR * e_ref + 2^-23,
  e_ref = the same restatement fed torch.softmax in float32 on the CPU (the reference's arithmetic; ~6e-8 on
  20 000 x 19 logits of sigma 3);
* predictions and confusions: equal as integers;
* frozen forward: the same referee rule on the logits, float64 value from oracle/torch_port.py in float64 on the CPU,
  e_ref = the unfrozen eval forward.
"""
import numpy as np
import pytest
import torch

import vote_ref
from util import REFEREE_FACTOR, check_err, g13_state, l2_err

pytestmark = pytest.mark.gpu

F32_SPACING = 2.0 ** -23
DEV = "cuda:0"


def _mods():
    import mvkpconv
    return mvkpconv, mvkpconv.sub("ops"), mvkpconv.sub("synthetic")


def _offsets(sizes, dev):
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return off, torch.from_numpy(off).to(dev)


def _random_batches(rng, sizes, n_batches):
    """[(lengths, input_inds, cloud_inds)]: 1-4 spheres per batch over the given clouds, distinct indices inside a sphere.
    Batch 0 is two spheres of cloud 0 that must share points (each takes 60 % of it), batch 1 is cloud pattern
    [0, last, 0]: two launches' worth of order with another cloud in between."""
    out = []
    for k in range(n_batches):
        if k == 0:
            clouds = [0, 0]
        elif k == 1:
            clouds = [0, len(sizes) - 1, 0]
        else:
            clouds = rng.integers(0, len(sizes), size=int(rng.integers(1, 5))).tolist()
        lengths, inds = [], []
        for c in clouds:
            n = int(0.6 * sizes[c]) if k < 2 else int(rng.integers(1, sizes[c] + 1))
            lengths.append(n)
            inds.append(rng.choice(sizes[c], size=n, replace=False))
        out.append((np.asarray(lengths, np.int32), np.concatenate(inds).astype(np.int64), np.asarray(clouds, np.int32)))
    return out


def _shared_rows(lengths, inds, clouds):
    """Rows of a batch's clouds that two of its spheres both write."""
    seen, shared, i0 = {}, 0, 0
    for n, c in zip(lengths, clouds):
        rows = set(inds[i0:i0 + n].tolist())
        shared += len(rows & seen.setdefault(int(c), set()))
        seen[int(c)] |= rows
        i0 += n
    return shared


# ------------------------------------------------------------------------------------------ 1. probabilities in

@pytest.mark.parametrize("C", [19, 5])
@pytest.mark.parametrize("index_dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("sizes", [(700,), (700, 450)])
def test_probability_votes_are_bit_equal_to_the_float64_restatement(C, index_dtype, sizes):
    _, ops, _ = _mods()
    rng = np.random.default_rng(1000 + C + len(sizes))
    off, off_dev = _offsets(sizes, DEV)
    votes_dev = torch.zeros((int(off[-1]), C), dtype=torch.float64, device=DEV)
    votes_ref = [np.zeros((n, C)) for n in sizes]
    batches = _random_batches(rng, sizes, 6)
    assert _shared_rows(*batches[0]) > 0 and _shared_rows(*batches[1]) > 0
    # the validation loop's per-batch confusion rides along: label table with an ignored slot, labels partly outside it
    label_values = np.concatenate([[0], 2 + np.arange(C)]).astype(np.int32)
    ignored = [0]
    cm = vote_ref.column_map(label_values, ignored)
    conf_dev = torch.zeros((C + 1, C + 1), dtype=torch.int64, device=DEV)
    conf_ref = np.zeros((C + 1, C + 1), np.int64)
    lv_dev, cm_dev = torch.from_numpy(label_values).to(DEV), torch.from_numpy(cm).to(DEV)
    for lengths, inds, clouds in batches:
        N = int(lengths.sum())
        probs = vote_ref.softmax(rng.standard_normal((N, C)) * 3, np.float32)
        labels = rng.choice(np.concatenate([label_values, [1, 99]]), size=N).astype(np.int64)
        vote_ref.vote_batch(votes_ref, probs, lengths, inds, clouds, smooth=0.95)
        conf_ref += vote_ref.confusion(labels, vote_ref.predict(probs, label_values, ignored), label_values)
        ops.vote_update_batch(votes_dev, off_dev, torch.from_numpy(probs).to(DEV), torch.from_numpy(lengths).to(DEV),
                              torch.from_numpy(inds).to(DEV, dtype=index_dtype), torch.from_numpy(clouds).to(DEV),
                              smooth=0.95, is_logits=False, labels=torch.from_numpy(labels).to(DEV),
                              label_values=lv_dev, col_map=cm_dev, confusion=conf_dev)
    got = votes_dev.cpu().numpy()
    want = np.concatenate(votes_ref, 0)
    assert got.dtype == np.float64 and np.array_equal(got.view(np.uint64), want.view(np.uint64)), \
        "%d of %d vote elements differ in their bits" % (int((got.view(np.uint64) != want.view(np.uint64)).sum()), got.size)
    assert np.array_equal(conf_dev.cpu().numpy(), conf_ref) and conf_ref.sum() > 0


# ------------------------------------------------------------------------------------------ 2. logits in

@pytest.mark.parametrize("C", [19, 5])
def test_logit_votes_within_the_referee_bound(C):
    _, ops, _ = _mods()
    rng = np.random.default_rng(2000 + C)
    sizes = (20000, 6000)
    off, off_dev = _offsets(sizes, DEV)
    votes_dev = torch.zeros((int(off[-1]), C), dtype=torch.float64, device=DEV)
    v64 = [np.zeros((n, C)) for n in sizes]
    v32 = [np.zeros((n, C)) for n in sizes]
    for k in range(4):
        clouds = np.asarray([[0], [0, 1], [1, 0, 0], [0]][k], np.int32)
        lengths = np.asarray([sizes[c] if k == 0 else int(rng.integers(sizes[c] // 2, sizes[c])) for c in clouds], np.int32)
        inds = np.concatenate([rng.choice(sizes[c], size=n, replace=False) for c, n in zip(clouds, lengths)]).astype(np.int64)
        logits = (rng.standard_normal((int(lengths.sum()), C)) * 3).astype(np.float32)
        vote_ref.vote_batch(v64, vote_ref.softmax(logits, np.float64), lengths, inds, clouds)
        vote_ref.vote_batch(v32, torch.softmax(torch.from_numpy(logits), 1).numpy(), lengths, inds, clouds)
        ops.vote_update_batch(votes_dev, off_dev, torch.from_numpy(logits).to(DEV), torch.from_numpy(lengths).to(DEV),
                              torch.from_numpy(inds).to(DEV), torch.from_numpy(clouds).to(DEV), is_logits=True)
    f64, ref32 = np.concatenate(v64, 0), np.concatenate(v32, 0)
    e_ref = l2_err(ref32, f64)
    check_err("vote_update logits C=%d: device votes vs float64 (reference float32 softmax vs float64: %.3e)" % (C, e_ref),
              l2_err(votes_dev.cpu().numpy(), f64), REFEREE_FACTOR * e_ref + F32_SPACING)


# ------------------------------------------------------------------------------------------ 3. radius mask

def test_radius_mask_selects_the_rows_the_restatement_selects():
    _, ops, _ = _mods()
    rng = np.random.default_rng(3000)
    in_radius, C, N = 1.2, 7, 30000
    r2 = (0.7 * in_radius) ** 2
    pts = rng.uniform(-0.8, 0.8, (N, 3)).astype(np.float32)
    while True:     # no row within 1e-4 r^2 of the boundary: redraw such rows (deterministic), nothing is left out
        d2 = (pts.astype(np.float64) ** 2).sum(1)
        near = np.abs(d2 - r2) < 1e-4 * r2
        if not near.any():
            break
        pts[near] = rng.uniform(-0.8, 0.8, (int(near.sum()), 3)).astype(np.float32)
    sizes = (N,)
    off, off_dev = _offsets(sizes, DEV)
    lengths, clouds = np.asarray([N // 2, N - N // 2], np.int32), np.asarray([0, 0], np.int32)
    inds = rng.permutation(N).astype(np.int64)         # two spheres of one cloud, disjoint rows
    probs = vote_ref.softmax(rng.standard_normal((N, C)), np.float32)
    votes_ref = [np.zeros((N, C))]
    written = vote_ref.vote_batch(votes_ref, probs, lengths, inds, clouds, points=pts, r2_max=r2)
    votes_dev = torch.zeros((N, C), dtype=torch.float64, device=DEV)
    ops.vote_update_batch(votes_dev, off_dev, torch.from_numpy(probs).to(DEV), torch.from_numpy(lengths).to(DEV),
                          torch.from_numpy(inds).to(DEV), torch.from_numpy(clouds).to(DEV), is_logits=False,
                          points=torch.from_numpy(pts).to(DEV), r2_max=r2)
    got = votes_dev.cpu().numpy()
    rows_ref = np.sort(np.concatenate([w[1] for w in written]))
    rows_dev = np.nonzero((got != 0).any(1))[0]         # probabilities are positive: a written row is non-zero
    assert 0.2 * N < len(rows_ref) < 0.8 * N
    assert np.array_equal(rows_dev, rows_ref)
    assert np.array_equal(got.view(np.uint64), votes_ref[0].view(np.uint64))
    # no mask: every row votes
    votes_dev.zero_()
    ops.vote_update_batch(votes_dev, off_dev, torch.from_numpy(probs).to(DEV), torch.from_numpy(lengths).to(DEV),
                          torch.from_numpy(inds).to(DEV), torch.from_numpy(clouds).to(DEV), is_logits=False,
                          points=torch.from_numpy(pts).to(DEV), r2_max=0.0)
    assert bool((votes_dev != 0).any(1).all())


# ------------------------------------------------------------------------------------------ 4. predict and score

def _predict_case(rng, Nc, C, label_values, ignored):
    votes = rng.random((Nc, C))
    votes[rng.random(Nc) < 0.15] = 0.0                                  # never-visited rows
    ties = np.nonzero(rng.random(Nc) < 0.2)[0]                          # exact ties of the maximum, in two columns
    a, b = rng.integers(0, C, len(ties)), rng.integers(0, C, len(ties))
    votes[ties, a] = votes[ties, b] = 2.0
    all_tied = np.nonzero(rng.random(Nc) < 0.05)[0]                     # every column equal and positive
    votes[all_tied] = 0.25
    pool = np.concatenate([label_values, [-1, 1000, int(label_values.max()) + 1]])     # some targets outside the table
    return votes, pool


@pytest.mark.parametrize("C,label_values,ignored", [
    (19, np.arange(20), [0]),                                           # ignored label first
    (5, np.array([1, 4, 7, 9, 12, 20, 33]), [1, 9]),                    # first and a middle slot, raw values with gaps
    (3, np.array([0, 1, 2, 3]), [2]),
])
def test_predictions_and_confusions_equal_the_restatement(C, label_values, ignored):
    mvkpconv, ops, _ = _mods()
    metrics = mvkpconv.sub("dropin.utils.metrics")
    rng = np.random.default_rng(4000 + C)
    Nc, Nfull = 5000, 12000
    votes, pool = _predict_case(rng, Nc, C, label_values, ignored)
    cm = vote_ref.column_map(label_values, ignored)
    assert (cm >= 0).sum() == C
    lv_dev = torch.from_numpy(label_values.astype(np.int32)).to(DEV)
    cm_dev = torch.from_numpy(cm).to(DEV)
    votes_dev = torch.from_numpy(votes).to(DEV)
    # one to one
    targets = rng.choice(pool, size=Nc).astype(np.int32)
    preds, conf = ops.vote_predict(votes_dev, lv_dev, cm_dev, targets=torch.from_numpy(targets).to(DEV))
    want = vote_ref.predict(votes, label_values, ignored)
    want_conf = vote_ref.confusion(targets, want, label_values)
    assert preds.dtype == torch.int32 and np.array_equal(preds.cpu().numpy(), want)
    assert conf.dtype == torch.int64 and np.array_equal(conf.cpu().numpy(), want_conf)
    assert (want[(votes == 0).all(1)] == label_values[0]).all()        # unvisited -> first label, even when ignored
    assert np.array_equal(ops.vote_predict(votes_dev, lv_dev, cm_dev).cpu().numpy(), want)
    # reprojected, accumulated onto the first confusion
    for dt in (torch.int32, torch.int64):
        proj = rng.integers(0, Nc, Nfull)
        full_targets = rng.choice(pool, size=Nfull).astype(np.int32)
        acc = conf.clone()
        preds, acc2 = ops.vote_predict(votes_dev, lv_dev, cm_dev, proj=torch.from_numpy(proj).to(DEV, dtype=dt),
                                       targets=torch.from_numpy(full_targets).to(DEV), confusion=acc)
        want_full = vote_ref.predict(votes, label_values, ignored, proj=proj)
        assert acc2 is acc and np.array_equal(preds.cpu().numpy(), want_full)
        total = want_conf + vote_ref.confusion(full_targets, want_full, label_values)
        assert np.array_equal(acc.cpu().numpy(), total)
        kept = vote_ref.drop_ignored(total, label_values, ignored)
        got_iou = metrics.IoU_from_confusions(vote_ref.drop_ignored(acc.cpu().numpy(), label_values, ignored))
        assert np.allclose(got_iou, vote_ref.iou(kept), rtol=0, atol=1e-12)


# ------------------------------------------------------------------------------------------ 5. frozen forward

def _small_net(deformable, index_dtype=torch.int32):
    """The KPFCNN (baseline variant) on a small sphere, with non-trivial running statistics (util.seeded_state)."""
    mvkpconv, ops, syn = _mods()
    dev = torch.device(DEV)
    torch.manual_seed(0)
    np.random.seed(0)
    cfg = syn.make_config("baseline", deformable=deformable, modulated=deformable)
    sph = [syn.raw_sphere(seed=5, radius=0.6, density=2500.0)]
    staged = syn.stage_spheres(sph, dev, None)
    limits = syn.calibrate_limits(cfg, staged)
    batch, lens = syn.build_batch(cfg, staged, limits, index_dtype)
    net = syn.build_model(cfg, dev)
    sd = net.state_dict()
    kp = {k: v.cpu().numpy() for k, v in sd.items() if k.endswith("kernel_points")}
    state = g13_state({k: tuple(v.shape) for k, v in sd.items()}, "baseline", deformable, kp)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    return cfg, net, batch


@pytest.mark.parametrize("deformable", [False, True])
def test_frozen_forward_within_the_referee_bound(deformable):
    mvkpconv, ops, syn = _mods()
    from oracle import torch_port
    blocks = mvkpconv.sub("dropin.models.blocks")
    cfg, net, batch = _small_net(deformable)
    net.eval()
    keys = list(net.state_dict().keys())
    with torch.no_grad():
        unfrozen = net(batch, cfg).cpu().numpy()
    blocks.freeze_inference(net)
    assert list(net.state_dict().keys()) == keys
    n_bn = sum(1 for m in net.modules() if isinstance(m, blocks.BatchNormBlock) and m.use_bn)
    assert n_bn > 30 and all(m.__dict__.get("_frozen") is not None for m in net.modules()
                             if isinstance(m, blocks.BatchNormBlock) and m.use_bn)
    calls = {"affine": 0, "bn": 0}
    real_affine, real_bn = ops.affine_lrelu, torch.nn.BatchNorm1d.forward
    try:        # the frozen path is the one that runs: every normalisation is an affine launch or rides in a GEMM
        ops.affine_lrelu = lambda *a, **k: (calls.__setitem__("affine", calls["affine"] + 1), real_affine(*a, **k))[1]
        torch.nn.BatchNorm1d.forward = lambda self, x: (calls.__setitem__("bn", calls["bn"] + 1), real_bn(self, x))[1]
        with torch.no_grad():
            frozen = net(batch, cfg).cpu().numpy()
    finally:
        ops.affine_lrelu, torch.nn.BatchNorm1d.forward = real_affine, real_bn
    assert calls["bn"] == 0 and 0 < calls["affine"] < n_bn
    # float64 value: the CPU port in eval mode
    sd64 = {k: (v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu()) for k, v in net.state_dict().items()}
    cb = torch_port.batch_to_cpu(batch)
    cb64 = {k: ([t.double() if t.is_floating_point() else t for t in v] if isinstance(v, list)
                else (v.double() if torch.is_tensor(v) and v.is_floating_point() else v)) for k, v in cb.items()}
    with torch.no_grad():
        f64 = torch_port.forward(sd64, cfg, cb64, None, False)[0].numpy()
    assert f64.dtype == np.float64
    e_ref = l2_err(unfrozen, f64)
    check_err("frozen forward %s: frozen logits vs float64 (unfrozen eval forward vs float64: %.3e)"
              % ("deformable" if deformable else "rigid", e_ref), l2_err(frozen, f64), REFEREE_FACTOR * e_ref + F32_SPACING)
    assert e_ref < 1e-3         # the unfrozen forward is the same network as the port (not two wiring errors agreeing)


def test_frozen_path_is_not_taken_with_gradients_and_train_drops_it():
    mvkpconv, ops, syn = _mods()
    blocks = mvkpconv.sub("dropin.models.blocks")
    ops.set_deterministic(True)         # two forwards of one network are bit-equal only in this mode
    try:
        cfg, net, batch = _small_net(False)
        net.eval()
        before = net(batch, cfg).detach().clone()           # gradients enabled
        with torch.no_grad():
            before_no_grad = net(batch, cfg).clone()
        blocks.freeze_inference(net)
        real_affine = ops.affine_lrelu

        def refuse(*a, **k):
            raise AssertionError("frozen path taken with gradients enabled")
        ops.affine_lrelu = refuse
        try:
            after = net(batch, cfg)
        finally:
            ops.affine_lrelu = real_affine
        assert after.requires_grad and torch.equal(after.detach(), before)
        with torch.no_grad():
            frozen = net(batch, cfg)
        assert not torch.equal(frozen, before)              # another rounding: the frozen path did run here
        net.train()
        assert all(m.__dict__.get("_frozen") is None for m in net.modules()
                   if isinstance(m, (blocks.BatchNormBlock, blocks.UnaryBlock)))
        net.eval()
        with torch.no_grad():
            assert torch.equal(net(batch, cfg), before_no_grad)     # snapshot gone: today's path again
    finally:
        ops.set_deterministic(False)


@pytest.mark.parametrize("C,addend", [(64, True), (64, False), (19, True), (6, False)])
def test_affine_lrelu_against_torch(C, addend):
    _, ops, _ = _mods()
    g = torch.Generator().manual_seed(C)
    R = 3001
    x, a = torch.randn(R, C, generator=g), torch.randn(R, C, generator=g)
    scale, shift = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    for slope in (0.1, 1.0):
        want = x * scale + shift
        if addend:
            want = want + a
        want = torch.nn.functional.leaky_relu(want, slope)
        with torch.no_grad():
            got = ops.affine_lrelu(x.to(DEV), scale.to(DEV), shift.to(DEV), slope, a.to(DEV) if addend else None)
        assert torch.equal(got.cpu(), want)                 # products and sums rounded one by one on both sides
    with pytest.raises(RuntimeError, match="forward only"):
        ops.affine_lrelu(x.to(DEV).requires_grad_(True), scale.to(DEV), shift.to(DEV))


# ------------------------------------------------------------------------------------------ 6. end to end

class _StandInDataset:
    """Two synthetic clouds with what ModelTester reads from a dataset: sub-cloud labels, full-cloud labels and their
    reprojection, a label table with one ignored label, and potentials that the loader raises every epoch."""

    def __init__(self, cloud_points, rng):
        self.set = 'validation'
        self.label_values = np.arange(21)
        self.ignored_labels = np.array([0])
        self.num_classes = 21
        self.label_to_names = {int(v): 'class %d' % v for v in self.label_values}
        self.files = [{'scan_id': 'scene%04d_00' % i} for i in range(len(cloud_points))]
        pool = np.concatenate([self.label_values, [40]])               # 40: outside the table
        self.input_labels = [rng.choice(pool, size=p.shape[0]).astype(np.int32) for p in cloud_points]
        self.test_proj = [rng.integers(0, p.shape[0], 2 * p.shape[0] + 17).astype(np.int32) for p in cloud_points]
        self.validation_labels = [rng.choice(pool, size=pr.shape[0]).astype(np.int32) for pr in self.test_proj]
        self.min_potentials = torch.zeros(len(cloud_points))
        self.cloud_points = cloud_points

    def load_evaluation_points(self, file_path):
        i = [f['scan_id'] for f in self.files].index(file_path['scan_id'])
        return self.cloud_points[i][self.test_proj[i]]


class _StandInLoader:
    """Yields the same drop-in batches every epoch (each with input_inds / cloud_inds) and raises the potentials by 5
    at the end of an epoch: the tester's second epoch ends on a reprojection checkpoint (ceil(10) % 10 == 0)."""

    def __init__(self, dataset, batches):
        self.dataset, self.batches, self.epochs = dataset, batches, 0
        self.yielded = []

    def __iter__(self):
        for b in self.batches:
            self.yielded.append(b)
            yield b
        self.dataset.min_potentials += 5.0
        self.epochs += 1


def _stand_in(cfg, syn, dev):
    """Two clouds (raw_sphere material, subsampled) and three batches of two spheres each: clouds (0, 1), (0, 0) with
    overlapping spheres, (1, 1) with overlapping spheres."""
    rng = np.random.default_rng(6000)
    sph = [syn.raw_sphere(seed=11 + i, radius=0.8, density=2500.0) for i in range(2)]
    clouds = syn.stage_spheres(sph, dev, None)
    centre = np.asarray(sph[0]['center'], np.float64)
    plan = [[(0, (0.0, 0.0, 0.0)), (1, (0.1, -0.1, 0.0))],
            [(0, (-0.15, 0.0, 0.0)), (0, (0.15, 0.05, 0.0))],
            [(1, (0.0, 0.15, 0.05)), (1, (0.05, -0.15, -0.05))]]
    specs = []
    for entry in plan:
        st = dict(points=[], colors=[], labels=[], center=[])
        inds_all, cl = [], []
        for c, shift in entry:
            ctr = torch.tensor(centre + np.asarray(shift), dtype=torch.float32, device=dev)
            pts = clouds['points'][c]
            inds = torch.nonzero(((pts - ctr) ** 2).sum(1) < cfg.in_radius ** 2)[:, 0]
            assert inds.numel() > 200
            st['points'].append(pts[inds].contiguous())
            st['colors'].append(clouds['colors'][c][inds].contiguous())
            st['labels'].append(clouds['labels'][c][inds].contiguous())
            st['center'].append(ctr)
            inds_all.append(inds)
            cl.append(c)
        specs.append((st, inds_all, cl))
    pooled = dict(points=[p for s in specs for p in s[0]['points']], center=[p for s in specs for p in s[0]['center']])
    limits = syn.calibrate_limits(cfg, pooled)
    batches = []
    for st, inds_all, cl in specs:
        batch, lens = syn.build_batch(cfg, st, limits, torch.int32)
        batch.input_inds = torch.cat(inds_all)                      # int64, HBM
        batch.cloud_inds = torch.tensor(cl, dtype=torch.int32, device=dev)
        batches.append(batch)
    dataset = _StandInDataset([p.cpu().numpy() for p in clouds['points']], rng)
    return dataset, _StandInLoader(dataset, batches)


def test_model_tester_end_to_end_on_a_stand_in_dataset(capsys):
    mvkpconv, ops, syn = _mods()
    tester_mod = mvkpconv.sub("dropin.utils.tester")
    dev = torch.device(DEV)
    torch.manual_seed(0)
    cfg = syn.make_config("baseline")
    cfg.in_radius = 0.5
    cfg.saving = False
    dataset, loader = _stand_in(cfg, syn, dev)
    assert _shared_rows([int(n) for n in loader.batches[1].lengths[0].cpu()], loader.batches[1].input_inds.cpu().numpy(),
                        [0, 0]) > 0
    net = syn.build_model(cfg, dev)
    logits = []
    net.register_forward_hook(lambda m, i, o: logits.append(o.detach().cpu().numpy()))
    tester = tester_mod.ModelTester(net, chkp_path=None)
    tester.cloud_segmentation_test(net, loader, cfg, num_votes=1)
    assert loader.epochs == 2 and len(logits) == 6                  # ended by the potentials rule: 5 -> 10, last_min 1.5 > 1
    assert not net.training

    # the restatement driven by the same logits
    sizes = [l.shape[0] for l in dataset.input_labels]
    v64 = [np.zeros((n, 20)) for n in sizes]
    v32 = [np.zeros((n, 20)) for n in sizes]
    r2 = (0.7 * cfg.in_radius) ** 2
    margin = np.inf
    for batch, out in zip(loader.yielded, logits):
        lengths = batch.lengths[0].cpu().numpy()
        inds, cl = batch.input_inds.cpu().numpy(), batch.cloud_inds.cpu().numpy()
        pts = batch.points[0].cpu().numpy()
        margin = min(margin, np.abs((pts.astype(np.float64) ** 2).sum(1) - r2).min() / r2)
        vote_ref.vote_batch(v64, vote_ref.softmax(out, np.float64), lengths, inds, cl, points=pts, r2_max=r2)
        vote_ref.vote_batch(v32, torch.softmax(torch.from_numpy(out), 1).numpy(), lengths, inds, cl, points=pts, r2_max=r2)
    assert margin > 1e-6, "a stand-in point sits on the mask's boundary (%.1e r^2): move the sphere centres" % margin
    got = [p.cpu().numpy() for p in tester.test_probs]
    f64, ref32 = np.concatenate(v64, 0), np.concatenate(v32, 0)
    e_ref = l2_err(ref32, f64)
    check_err("ModelTester end to end: device votes vs float64 (reference float32 softmax vs float64: %.3e)" % e_ref,
              l2_err(np.concatenate(got, 0), f64), REFEREE_FACTOR * e_ref + F32_SPACING)
    assert all(((g != 0).any(1) == (w != 0).any(1)).all() for g, w in zip(got, v64))      # the same rows were visited
    assert any(((g == 0).all(1)).any() for g in got)                                       # and some never were

    # predictions and confusions recomputed in NumPy from the DOWNLOADED device votes: exactly the device's
    lv, ign = dataset.label_values, list(dataset.ignored_labels)
    sub = sum(vote_ref.confusion(dataset.input_labels[c], vote_ref.predict(got[c], lv, ign), lv) for c in range(2))
    assert np.array_equal(tester.sub_confusion, sub)
    full_preds = [vote_ref.predict(got[c], lv, ign, proj=dataset.test_proj[c]) for c in range(2)]
    full = sum(vote_ref.confusion(dataset.validation_labels[c], full_preds[c], lv) for c in range(2))
    assert np.array_equal(tester.full_confusion, full)
    for c in range(2):
        assert np.array_equal(tester.full_preds[c].cpu().numpy(), full_preds[c])
    assert np.allclose(tester.full_IoUs, vote_ref.iou(vote_ref.drop_ignored(full, lv, ign)), rtol=0, atol=1e-9)
    props = np.array([sum(int((l == v).sum()) for l in dataset.validation_labels) for v in lv if v not in ign], np.float32)
    C = vote_ref.drop_ignored(sub, lv, ign).astype(np.float32)
    C *= np.expand_dims(props / (np.sum(C, axis=1) + 1e-6), 1)
    assert np.allclose(tester.sub_IoUs, vote_ref.iou(C), rtol=0, atol=1e-6)
    assert "Reproject Vote #10" in capsys.readouterr().out

    # the validation loop on the same loader: every labelled row of every batch is counted once, unmasked votes
    acc = tester_mod.VoteAccumulator(sizes, 20, lv, ign, dev)
    for b, batch in enumerate(loader.batches):                      # raw labels for the batch's rows
        batch.labels = torch.cat([torch.from_numpy(dataset.input_labels[int(c)]).to(dev)[batch.input_inds[i0:i0 + n]]
                                  for c, i0, n in zip(batch.cloud_inds.tolist(),
                                                      np.concatenate([[0], np.cumsum(batch.lengths[0].cpu().numpy())[:-1]]).tolist(),
                                                      batch.lengths[0].tolist())])
    net.train()
    IoUs = tester_mod.cloud_segmentation_validation(net, loader, cfg, acc)
    assert net.training and IoUs.shape == (20,) and np.isfinite(IoUs).all()
    conf = acc.confusion().cpu().numpy()
    counted = sum(int(np.isin(b.labels.cpu().numpy(), lv).sum()) for b in loader.batches)
    assert conf.sum() == counted and conf[:, 0].sum() == 0         # an ignored label is never predicted from a visited row
    C = vote_ref.drop_ignored(conf.astype(np.int32).astype(np.float32), lv, ign)
    C *= np.expand_dims(props / (np.sum(C, axis=1) + 1e-6), 1)
    assert np.allclose(IoUs, vote_ref.iou(C), rtol=0, atol=1e-6)
