"""The conditions the cases of tests/block_cases.py must meet for tests/test_blocks_gpu.py to compare every element of
every tensor under util.referee_check's own bound (3 e_ref + 1e-5), from the float64 and float32 runs of the oracle
(oracle/torch_port.py through tests/block_ref.py) alone. No GPU. Each case is checked with the seed the table records;
nothing here searches."""
import numpy as np
import pytest

import block_cases as bc
import block_ref as br


@pytest.mark.parametrize("base", bc.BASES)
def test_reference_error_keeps_the_referee_bound_decisive(base):
    """Every compared tensor: the float32 run of the oracle within 5e-6 (L2-relative) of its float64 run, so that
    3 e_ref + 1e-5 stays about 1e-5 -- three orders below the network-level bounds."""
    errs = br.reference_errors(br.block64(base), br.block32(base), base)
    assert {"y", "dx", "y eval"} <= set(errs) and any(k.startswith("grad ") for k in errs)
    bad = {k: e for k, e in errs.items() if not e <= br.E_REF_MAX}
    assert not bad, bad


@pytest.mark.parametrize("base", bc.BASES)
def test_no_leaky_relu_input_near_its_kink(base):
    """min |z64| >= 10 max |z32 - z64| on every LeakyReLU input of the block: a correct float32 implementation has no
    legitimate reason to flip a kink, so the GPU test masks nothing out."""
    c = bc.BY_NAME[base]
    margins = br.kink_margins(br.block64(base), br.block32(base))
    assert len(margins) == (1 if c.block.startswith("simple") else (3 if c.cin != c.cout // 4 else 2))
    for n, (lo, dev) in enumerate(margins):
        assert lo >= br.MARGIN * dev, (base, n, lo, dev)


@pytest.mark.parametrize("base", [b for b in bc.BASES if "deform" in b])
def test_deformable_cases_stay_clear_of_the_extent_and_of_argmin_ties(base):
    """No (real neighbour, deformed kernel point) pair in the band |d / extent - 1| < 10 x the float32 deviation of
    d / extent (where the linear influence and the in-range filter switch), no tied min_d2 arg-min, and at least a
    quarter of the real neighbours in range of a kernel point."""
    r64, r32 = br.block64(base), br.block32(base)
    inside, width = br.deform_band(r64, r32)
    assert inside == 0, (base, inside, width)
    assert br.deform_argmin_ties(r64, r32) == 0
    assert np.array_equal(r64.d_ext < 1, r32.d_ext < 1)
    in_range = (r64.d_ext < 1).any(2) & r64.real
    assert in_range.sum() >= 0.25 * r64.real.sum(), (int(in_range.sum()), int(r64.real.sum()))
    # offsets are a fraction of the extent, and not zero
    i = bc.make_inputs(base)
    off = np.abs(r64.tensors["deformed_KP"] - i.state["KPConv.kernel_points"].astype(np.float64)[None]).max()
    assert 0.01 * 0.06 < off < 0.06, off


@pytest.mark.parametrize("base", bc.BASES)
def test_coverage_counts(base):
    """A shadow-only row, rows with fewer real neighbours than H, rows that are full, statistics that are not 0 / 1."""
    c, i = bc.BY_NAME[base], bc.make_inputs(base)
    real = (i.idx < c.N).sum(1)
    assert real[bc.ROW_SHADOW] == 0 and (i.idx[bc.ROW_SHADOW] == c.N).all()
    assert ((real > 0) & (real < c.H)).sum() >= 4
    assert i.idx.shape == (c.N // 4 if "strided" in c.block else c.N, c.H) and i.idx.dtype == np.int32
    assert float(i.q[np.arange(len(i.q)) != bc.ROW_SHADOW].max()) < 0.5 and float(i.s.min()) >= 0
    for n, v in i.state.items():
        if n.endswith("running_mean"):
            assert np.abs(v).min() > 0
        if n.endswith("running_var"):
            assert (v > 1).all()
        if n.endswith("offset_bias"):
            assert np.abs(v).min() > 0
    # sorted by distance, ties by index: the first column of a block that is not strided is the point itself
    if "strided" not in c.block:
        rows = np.arange(c.N) != bc.ROW_SHADOW
        assert (i.idx[rows, 0] == np.arange(c.N)[rows]).all()


def test_case_table_is_the_one_the_sweep_asks_for():
    """Every block type, the row counts on both sides of ops.bn_single_launch_rows (1024 for these widths), the modes on
    the three blocks that have them, and the routes every case declares (bc.routes_of) taken together reach every
    fused entry point of the bottleneck block."""
    by = bc.BY_NAME
    shapes = {(c.block, c.cin, c.cout, c.N, c.use_bn, c.mod) for c in bc.CASES if c.mode is None}
    for want in (("resnetb", 64, 128, 400, True, False), ("resnetb", 64, 128, 100, True, False), ("resnetb", 64, 128, 1030, True, False),
                 ("resnetb", 128, 128, 400, True, False), ("resnetb", 32, 128, 400, True, False),
                 ("resnetb_strided", 64, 128, 400, True, False), ("resnetb_strided", 128, 128, 400, True, False),
                 ("simple", 4, 64, 400, True, False), ("simple", 5, 64, 400, True, False), ("simple_strided", 64, 128, 400, True, False),
                 ("resnetb", 64, 128, 400, False, False), ("resnetb_strided", 64, 128, 400, False, False), ("simple", 5, 64, 400, False, False)):
        assert want in shapes, want
    for block in ("resnetb_deformable", "resnetb_deformable_strided", "simple_deformable"):
        for mod in (False, True):
            assert (block, 64, 128, 400, True, mod) in shapes
    for block in ("resnetb", "resnetb_strided", "resnetb_deformable"):
        assert {c.mode for c in bc.CASES if c.block == block and c.mode} == set(bc.MODES[1:])
    assert len(bc.CASES) == 34
    reached = set().union(*(c.routes for c in bc.CASES)) | bc.NET_ROUTES
    assert reached == {bc.LINEAR_PAIR, bc.LINEAR_PAIR_STATS, bc.LINEAR, bc.LINEAR_PASS, bc.MAX_POOL_PASS, bc.BN_PAIR, bc.BN_LINEAR,
                       bc.BN, bc.BIAS, bc.LINEAR_BIAS, bc.ADD, bc.UPCAT_LINEAR, bc.DEFORM_OPERANDS, bc.KPCONV, bc.KPCONV_REV,
                       bc.XENT}
    assert by["resnetb-64-128"].routes == {bc.LINEAR_PAIR, bc.BN, bc.KPCONV, bc.BN_PAIR, bc.LINEAR}
    assert by["resnetb-64-128-n1030"].routes == {bc.LINEAR_PAIR_STATS, bc.BN, bc.KPCONV, bc.BN_PAIR, bc.LINEAR}
    assert by["resnetb-128-128"].routes == {bc.LINEAR_PASS, bc.BN, bc.KPCONV, bc.LINEAR}
    assert by["resnetb_strided-64-128-nobn"].routes == {bc.LINEAR_PASS, bc.BIAS, bc.KPCONV, bc.MAX_POOL_PASS, bc.LINEAR_BIAS,
                                                         bc.LINEAR, bc.ADD}
    assert by["resnetb-64-128-fold"].routes == {bc.LINEAR_PAIR_STATS, bc.BN, bc.KPCONV, bc.BN_LINEAR, bc.LINEAR}
    assert by["resnetb_deformable-64-128-det"].routes == {bc.LINEAR_PAIR, bc.BN, bc.KPCONV_REV, bc.DEFORM_OPERANDS, bc.BN_PAIR,
                                                           bc.LINEAR}


def test_two_level_network_meets_the_conditions():
    """The two-level network as a full case: e_ref <= 5e-6 on logits, loss, every gradient and running statistic, no
    LeakyReLU input near its kink, and the strided block's max-pool (the one max-pool that reads computed features) with
    a gap between its two largest candidates of at least 10 x the float32 deviation of those features."""
    r64, r32 = br.net64(), br.net32()
    assert not br.conditions(r64, r32), br.conditions(r64, r32)
    assert len(r64.kinks) == 13                    # 1 + 3 + 3 + 3 block activations, the decoder layer, the two head layers
    i = bc.make_net_inputs()
    assert (i.neighbors[0][bc.ROW_SHADOW] == sum(bc.NET_CLOUDS)).all()
    assert (i.labels == 0).sum() >= 20 and len(np.unique(i.labels)) == bc.NET_CLASSES + 1
    # rows stay inside their cloud
    n0 = bc.NET_CLOUDS[0]
    nb = i.neighbors[0]
    assert (nb[:n0][nb[:n0] < sum(bc.NET_CLOUDS)] < n0).all() and (nb[n0:] >= n0).all()
    assert (i.upsamples[0][:, 0] < len(i.points[1])).mean() > 0.9
