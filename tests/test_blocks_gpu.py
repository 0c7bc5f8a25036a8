"""The network blocks of dropin/models/blocks.py on the HIP kernels against the float64 run of the unfused oracle
(oracle/torch_port.py through tests/block_ref.py), block by block over the case table of tests/block_cases.py: every
block type, both sides of the single-launch BatchNorm threshold, with and without BatchNorm, deformable and modulated,
int64 rows, the gather-form and the scatter feature gradient, deterministic mode, the BatchNorm fold, and one two-level
KPFCNN (skip alias hand-over, the decoder as two products, the BatchNorm-less head, the fused loss).

Every tensor -- y, dx, every parameter gradient, every running statistic, min_d2 and deformed_KP of the deformable
blocks, the eval-mode output before and after freeze_inference -- goes through util.referee_check with the project's own
factor and floor: err(HIP, float64) <= 3 err(oracle float32, float64) + 1e-5, L2-relative. tests/test_blocks_cpu.py shows
that no input sits where a float32 implementation may legitimately flip a kink, so nothing is masked out. Counting
spies on the fused entry points of ops.py check that a case reaches exactly the routes it declares: a block that falls
onto another path fails instead of passing on the wrong kernel.

Measured on the MI355X: every case reaches exactly its declared routes (block_cases.routes_of), every e_hip is below 2e-6
against bounds of 1.0e-5 .. 1.3e-5. Largest e_hip / e_ref of any tensor with e_ref above 1e-7, per case:
  resnetb-64-128 1.82 (-n100 1.85, -n1030 2.10, -idx64 1.62, -rev 1.64, -scatter 1.64, -det 1.67, -fold 1.92)
  resnetb-128-128 1.48, resnetb-32-128 2.09, resnetb-64-128-nobn 1.13
  resnetb_strided-64-128 1.57 (-idx64 1.61, -rev 1.66, -scatter 1.57, -det 1.58, -fold 1.97, -nobn 1.20)
  resnetb_strided-128-128 3.07, simple-4-64 2.27, simple-5-64 5.06 (-nobn 1.66), simple_strided-64-128 3.49
  resnetb_deformable-64-128 1.59 (-mod 1.71, -idx64 1.57, -rev 1.58, -scatter 1.59, -det 1.84, -fold 2.24)
  resnetb_deformable_strided-64-128 1.59 (-mod 1.52), simple_deformable-64-128 1.75 (-mod 1.76)
  two-level network 3.11 (logits 1.6, loss 1.0)
The ratios above 3 are the shadow-only row of y taken alone (one row, e_ref 1.0e-7 .. 1.5e-7, e_hip 4.5e-7 .. 5.3e-7) and one
BatchNorm weight gradient of the network (5.0e-7 against 1.6e-6): roundings under the floor, not a uniform excess."""
import contextlib
import importlib

import numpy as np
import pytest
import torch

import block_cases as bc
import block_ref as br
from util import REFEREE_FACTOR, REFEREE_FLOOR, check_err, referee_check

pytestmark = pytest.mark.gpu

PKG = "enhancing-3d-point-cloud-segmentation-using-multi-modal-fusion-with-2d-images_amd"
TINY = 1e-6          # a gradient with a float64 norm below TINY x the largest of the case: compared against that scale


@pytest.fixture(scope="module")
def mods():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    names = ("ops", "dropin.models.blocks", "dropin.models.architectures", "dropin.utils.config")
    return tuple(importlib.import_module(PKG + "." + n) for n in names)


def T(a):
    return torch.from_numpy(np.array(a)).cuda()          # (a copy: the cached inputs are read-only)


def N(t):
    return t.detach().cpu().numpy()


def _config(cfgm, ns):
    cfg = cfgm.Config()
    for k, v in vars(ns).items():
        setattr(cfg, k, v)
    return cfg


def _spies(monkeypatch, ops):
    """Wraps the fused entry points of ops.py; returns the set that collects the routes reached."""
    reached = set()

    def arg(a, k, pos, key):
        return k[key] if key in k else (a[pos] if len(a) > pos else None)

    def spy(name, label):
        real = getattr(ops, name)

        def wrapped(*a, **k):
            out = real(*a, **k)
            lab = label(a, k, out)
            if lab is not None:
                reached.add(lab)
            return out
        monkeypatch.setattr(ops, name, wrapped)

    def pair_label(a, k, out):
        if out is None:
            return None
        return bc.LINEAR_PAIR_STATS if any(ops.bn_stats_of(o) is not None for o in out) else bc.LINEAR_PAIR

    spy("linear_pair", pair_label)
    spy("linear", lambda a, k, o: bc.LINEAR_PASS if arg(a, k, 4, "passthrough") else bc.LINEAR)
    spy("max_pool", lambda a, k, o: bc.MAX_POOL_PASS if arg(a, k, 2, "passthrough") else bc.MAX_POOL)
    spy("bn_lrelu_linear", lambda a, k, o: None if o is None else bc.BN_LINEAR)
    spy("kpconv", lambda a, k, o: bc.KPCONV if arg(a, k, 13, "rev") is None else bc.KPCONV_REV)
    for name in (bc.BN_PAIR, bc.BN, bc.BIAS, bc.LINEAR_BIAS, bc.ADD, bc.UPCAT_LINEAR, bc.DEFORM_OPERANDS, bc.XENT):
        spy(name, lambda a, k, o, name=name: name)
    return reached


@contextlib.contextmanager
def _mode(ops, mode, index_rows, n_support, points):
    """The switches of a mode, every one restored at the end. rev / scatter / det register the reverse list of the block's
    rows and a work list (a seeded permutation: the result does not depend on it) per level, like a pyramid built in
    this process does (ops.remember_reverse / ops.remember_work_order)."""
    old = (ops.REVERSE_DX, ops.BN_FOLD, ops.is_deterministic())
    try:
        ops.REVERSE_DX = mode != "scatter"
        ops.BN_FOLD = mode == "fold"
        if mode == "det":
            ops.set_deterministic(True)
        if mode in ("rev", "scatter", "det"):
            ops.remember_reverse(index_rows, ops.reverse_neighbors(index_rows, n_support))
            g = torch.Generator().manual_seed(5)
            for p in points:
                ops.remember_work_order(p, torch.randperm(p.shape[0], generator=g).to(torch.int32).cuda())
        yield
    finally:
        ops.REVERSE_DX, ops.BN_FOLD = old[:2]
        if mode == "det":
            ops.set_deterministic(old[2])


class _Checker:
    """referee_check over the tensors of one case; collects the failures and the ratios."""

    def __init__(self, tag, r64, r32):
        self.tag, self.r64, self.r32 = tag, r64.tensors, r32.tensors
        self.failures, self.ratios = [], []
        grads = [v for k, v in self.r64.items() if k == "dx" or k.startswith("grad ")]
        self.scale = max(float(np.linalg.norm(v)) for v in grads) if grads else None

    def __call__(self, key, hip, rows=None, note=""):
        f64, ref32 = self.r64[key], self.r32[key]
        hip = np.asarray(hip, np.float64).reshape(f64.shape)
        if rows is not None:
            hip, f64, ref32 = hip[rows], f64[rows], ref32[rows]
        label = "block %s: %s%s" % (self.tag, key, note)
        if not np.isfinite(hip).all():
            self.failures.append(label + ": not finite")
            return
        is_grad = key == "dx" or key.startswith("grad ")
        if is_grad and np.linalg.norm(f64) < TINY * self.scale:
            e_hip, e_ref = (float(np.linalg.norm(v - f64)) / self.scale for v in (hip, ref32.astype(np.float64)))
            try:
                check_err(label + " (against the largest gradient; reference float32: %.3e)" % e_ref, e_hip,
                          REFEREE_FACTOR * e_ref + REFEREE_FLOOR)
            except AssertionError as e:
                self.failures.append(str(e))
            return
        e_hip, e_ref = referee_check(label, hip, ref32, f64, failures=self.failures)
        if e_ref > 1e-7:
            self.ratios.append((e_hip / e_ref, key))

    def finish(self):
        if self.ratios:
            worst = max(self.ratios)
            print("block %s: worst e_hip / e_ref %.2f (%s)" % (self.tag, worst[0], worst[1]))
        assert not self.failures, "\n".join(self.failures)


def _state_checks(chk, module, want_keys):
    sd = module.state_dict()
    seen = 0
    for k, v in sd.items():
        if k.endswith("num_batches_tracked"):
            assert int(v) == 1, k
        elif k.endswith(("running_mean", "running_var")):
            chk(k, N(v))
            seen += 1
    assert seen == sum(k.endswith(("running_mean", "running_var")) for k in want_keys)


@pytest.mark.parametrize("name", [c.name for c in bc.CASES])
def test_block_vs_float64_oracle(mods, monkeypatch, name):
    ops, blocks, _, cfgm = mods
    c, i = bc.BY_NAME[name], bc.make_inputs(bc.BY_NAME[name].base)
    r64, r32 = br.block64(c.base), br.block32(c.base)
    strided, deform = "strided" in c.block, "deform" in c.block
    cfg = _config(cfgm, bc.config(c.use_bn, c.mod))
    state = {k: T(v) for k, v in i.state.items()}
    block = blocks.block_decider(c.block, bc.R, c.cin, c.cout, 0, cfg).cuda()
    assert set(block.state_dict()) == set(state)
    block.load_state_dict(state)
    block.train()

    class batch:
        points = [T(i.s), T(i.q)] if strided else [T(i.s)]
        neighbors = [T(i.idx).long() if c.mode == "idx64" else T(i.idx)]
        pools = neighbors
        lengths = [torch.tensor([p.shape[0]], dtype=torch.int32) for p in points]

    x = T(i.x).requires_grad_(True)
    go = T(i.go)
    params = [(n, p) for n, p in block.named_parameters() if p.requires_grad]
    chk = _Checker(name, r64, r32)
    with _mode(ops, c.mode, batch.neighbors[0], c.N, batch.points):
        reached = _spies(monkeypatch, ops)
        y = block(x, batch)
        scalar = (y * go).sum()
        if strided and c.block.startswith("resnetb"):
            alias = block.skip_alias
            # the pooling's own second output (same storage as x): its backward then adds onto the second consumer's gradient
            assert alias is not None and alias.data_ptr() == x.data_ptr()
            assert "MaxPool" in type(alias.grad_fn).__name__, type(alias.grad_fn).__name__
        if strided:
            # a second consumer of the block input (the decoder's skip tensor): its gradient is summed into dx
            scalar = scalar + bc.ALIAS_C * (alias if c.block.startswith("resnetb") else x).sum()
        grads = torch.autograd.grad(scalar, [x] + [p for _, p in params])
        torch.cuda.synchronize()
        routes = set(reached)
        monkeypatch.undo()
    assert routes == set(c.routes), "routes reached %s, declared %s" % (sorted(routes), sorted(c.routes))
    chk("y", N(y))
    chk("y", N(y), rows=[bc.ROW_SHADOW], note=" (the shadow-only row)")
    chk("dx", N(grads[0]))
    assert {"grad " + n for n, _ in params} == {k for k in r64.tensors if k.startswith("grad ")}
    for (n, _), g in zip(params, grads[1:]):
        chk("grad " + n, N(g))
    _state_checks(chk, block, state)
    if deform:
        live = br.live_rows(c.base)
        assert not live[bc.ROW_SHADOW]
        chk("min_d2", N(block.KPConv.min_d2), rows=live)
        chk("min_d2", N(block.KPConv.min_d2), rows=~live, note=" (shadow-only rows)")
        chk("deformed_KP", N(block.KPConv.deformed_KP))
        assert {"grad KPConv.offset_conv.weights", "grad KPConv.offset_bias"} <= set(r64.tensors)
    # eval mode, on the statistics of the state dict (the training forward moved the block's own)
    block.load_state_dict(state)
    block.eval()
    with torch.no_grad():
        chk("y eval", N(block(T(i.x), batch)))
        blocks.freeze_inference(block)
        chk("y eval", N(block(T(i.x), batch)), note=" (freeze_inference)")
    chk.finish()


def test_two_level_network_vs_float64_oracle(mods, monkeypatch):
    """architectures.KPFCNN over block_cases.NET_ARCH on two stacked clouds against torch_port.forward + loss_fn in float64:
    logits, loss (labels with ignored ones, through the lookup table), every parameter gradient and running statistic,
    the eval-mode logits before and after freeze_inference."""
    ops, blocks, arch, cfgm = mods
    i = bc.make_net_inputs()
    r64, r32 = br.net64(), br.net32()
    cfg = _config(cfgm, bc.config(architecture=bc.NET_ARCH))
    net = arch.KPFCNN(cfg, list(range(bc.NET_CLASSES + 1)), [0]).cuda()
    state = {k: T(v) for k, v in i.state.items()}
    assert set(net.state_dict()) == set(state)
    net.load_state_dict(state)
    net.train()

    class batch:
        points = [T(p) for p in i.points]
        neighbors = [T(a) for a in i.neighbors]
        pools = [T(a) for a in i.pools]
        upsamples = [T(a) for a in i.upsamples]
        lengths = [torch.from_numpy(np.array(a)) for a in i.lengths]
        features = T(i.features)
        labels = T(i.labels)

    params = [(n, p) for n, p in net.named_parameters() if p.requires_grad]
    chk = _Checker("two-level network", r64, r32)
    old = (ops.REVERSE_DX, ops.BN_FOLD)
    try:
        ops.REVERSE_DX, ops.BN_FOLD = True, False
        reached = _spies(monkeypatch, ops)
        logits = net(batch, cfg)
        loss = net.loss(logits, batch.labels)
        grads = torch.autograd.grad(loss, [p for _, p in params])
        torch.cuda.synchronize()
        routes = set(reached)
        monkeypatch.undo()
    finally:
        ops.REVERSE_DX, ops.BN_FOLD = old
    assert routes == set(bc.NET_ROUTES), "routes reached %s, declared %s" % (sorted(routes), sorted(bc.NET_ROUTES))
    assert all(getattr(b, "skip_alias", None) is None for b in net.encoder_blocks)      # handed over and cleared
    chk("logits", N(logits))
    chk("loss", N(loss).reshape(1))
    assert {"grad " + n for n, _ in params} == {k for k in r64.tensors if k.startswith("grad ")}
    for (n, _), g in zip(params, grads):
        chk("grad " + n, N(g))
    _state_checks(chk, net, state)
    net.load_state_dict(state)
    net.eval()
    with torch.no_grad():
        chk("y eval", N(net(batch, cfg)))
        blocks.freeze_inference(net)
        chk("y eval", N(net(batch, cfg)), note=" (freeze_inference)")
    chk.finish()
