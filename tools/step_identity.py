"""Identity check of whole network steps across two checkouts of this repository (same built library): for changes to
the Python layer that must leave every default path calling the same exports in the same order and computing the same bits.

  python tools/step_identity.py dump --tree <checkout> --out <file.pt>      (once per checkout, on the GPU)
  python tools/step_identity.py compare <before.pt> <after.pt>               (prints the report, exit 1 on a difference)

dump runs, in deterministic mode and with fixed seeds: the four steps of
tests/test_model_gpu.py::test_deterministic_mode_step_is_bit_reproducible (forward, loss, backward under
defer_weight_grads; a fixed random feature map stands in for the frozen 2D encoder), the same for a deformable + modulated
middle-fusion net, one capacity-padded early-fusion step built like the padded run of
test_capacity_padded_mode_equals_plain_mode (ops.row_count_for answers there; plain loss.backward(), so the weight
gradients run in line), and one eval-mode forward under torch.no_grad() of the early and the late net. Per case it records
the ordered list of mvk_* exports called (the Recorder of tools/bn_handoff_identity.py) and the logits, the loss, every
parameter gradient and every BatchNorm running statistic and batch counter. compare wants equal call lists and torch.equal
tensors in every case."""
import argparse
import difflib
import importlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bn_handoff_identity import PKG, Recorder      # noqa: E402

#        name                variant   spheres deformable mode
CASES = [("early x1",          "early",    1, False, "train"),
         ("baseline x2",       "baseline", 2, False, "train"),
         ("late x1",           "late",     1, False, "train"),
         ("late x1 deform",    "late",     1, True,  "train"),
         ("middle x1 deform",  "middle",   1, True,  "train"),
         ("early x1 padded",   "early",    1, False, "padded"),
         ("early x1 eval",     "early",    1, False, "eval"),
         ("late x1 eval",      "late",     1, False, "eval")]


def step_case(syn, ops, common, variant, spheres, deformable, mode):
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    np.random.seed(0)
    cfg = syn.make_config(variant, deformable=deformable, modulated=deformable)
    sph = [syn.raw_sphere(seed=i, radius=0.7, density=3000.0) for i in range(spheres)]
    views = [syn.sphere_views(s, nv=3, h=60, w=80) for s in sph] if variant != "baseline" else None
    staged = syn.stage_spheres(sph, dev, views)
    limits = syn.calibrate_limits(cfg, staged)
    rng = np.random.RandomState(4)
    rots = [common.random_grid_rotations(spheres, rng) for _ in range(4)]
    net = syn.build_model(cfg, dev)
    net.train(mode != "eval")
    if hasattr(net, "net_2d"):
        for m in net.net_2d._modules.values():
            m.train(False)
    batch, _ = syn.build_batch(cfg, staged, limits, torch.int32, rotations=rots)
    if variant != "baseline":
        batch.feature_2d = torch.randn(spheres * 3, 64, 60, 80, generator=torch.Generator().manual_seed(5)).to(dev)
    res = {}
    if mode == "eval":
        with torch.no_grad():
            res["logits"] = net(batch, cfg)
    else:
        if mode == "padded":
            plain, batch = batch, syn.StaticBatch(batch, limits)
            assert any(c > p.shape[0] for c, p in zip(batch.caps[1:], plain.points[1:]))      # really padded
            ops.set_row_counts(batch.valid)
        try:
            out = net(batch, cfg)
            loss = net.loss(out, batch.labels)
            if mode == "padded":
                loss.backward()
            else:
                with ops.defer_weight_grads():
                    loss.backward()
        finally:
            ops.set_row_counts(None)
        res["logits"], res["loss"] = out, loss
        res.update({"grad." + n: p.grad for n, p in net.named_parameters() if p.grad is not None})
        assert len(res) > 50
    res.update({"state." + k: v for k, v in net.state_dict().items() if "running" in k or "tracked" in k})
    return res


def dump(tree, out):
    sys.path.insert(0, os.path.abspath(tree))
    ops = importlib.import_module(PKG + ".ops")
    lib_mod = importlib.import_module(PKG + "._lib")
    syn = importlib.import_module(PKG + ".synthetic")
    common = importlib.import_module(PKG + ".dropin.datasets.common")
    assert os.path.abspath(ops.__file__).startswith(os.path.abspath(tree) + os.sep), ops.__file__
    rec = Recorder(lib_mod.lib())
    lib_mod._lib = rec                           # what lib() hands out from now on
    ops.set_deterministic(True)
    result = {}
    for name, variant, spheres, deformable, mode in CASES:
        del rec.calls[:]
        tensors = step_case(syn, ops, common, variant, spheres, deformable, mode)
        torch.cuda.synchronize()
        result[name] = {"calls": list(rec.calls), "tensors": {k: v.detach().cpu().clone() for k, v in tensors.items()}}
        print("%-20s %5d calls, %3d tensors" % (name, len(rec.calls), len(tensors)), flush=True)
    ops.set_deterministic(False)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    torch.save(result, out)


def compare(before, after):
    a, b = torch.load(before), torch.load(after)
    bad = 0
    print("case                 calls before/after  tensors  differing  call-list differences")
    if list(a) != list(b):
        print("DIFFERENT CASES: %s / %s" % (list(a), list(b)))
        bad += 1
    for name in a:
        if name not in b:
            continue
        ca, cb = a[name]["calls"], b[name]["calls"]
        delta = [d for d in difflib.ndiff(ca, cb) if d[0] in "+-"] if ca != cb else []
        ta, tb = a[name]["tensors"], b[name]["tensors"]
        differing = sorted(set(ta) ^ set(tb)) + [k for k in ta if k in tb and not (
            ta[k].dtype == tb[k].dtype and ta[k].shape == tb[k].shape and torch.equal(ta[k], tb[k]))]
        bad += len(delta) + len(differing)
        print("%-20s %6d / %-6d      %5d  %9d  %s" % (name, len(ca), len(cb), len(ta), len(differing),
                                                   ", ".join(delta[:20]) if delta else "none"))
        for k in differing:
            print("    DIFFERENT TENSOR: %s" % k)
    print("result: %s" % ("IDENTICAL" if not bad else "%d DIFFERENCES" % bad))
    return 1 if bad else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    d = sub.add_parser("dump")
    d.add_argument("--tree", required=True)
    d.add_argument("--out", required=True)
    c = sub.add_parser("compare")
    c.add_argument("before")
    c.add_argument("after")
    args = ap.parse_args()
    sys.exit(dump(args.tree, args.out) if args.cmd == "dump" else compare(args.before, args.after))
