"""The float64 oracle of the deformable KPConv (oracle/npref.py:kpconv_deform_backward) against torch.autograd and the
reference's G4 fixtures, and the conditions the cases of tests/deform_cases.py must meet for the GPU sweep
(tests/test_deform_gpu.py) to compare every element. No GPU."""
import numpy as np
import pytest
import torch

import deform_cases as dc
from conftest import load_golden
from oracle import npref
from util import rel_err, check_err

FP_TOL = 1e-4        # the bar of the G4 fixtures and of the GPU sweep (tests/test_gpu_parity.py)
NAMES = [c.name for c in dc.CASES]


def _torch_forward(q, s, idx, x, kp, W, ext, off, mod, influence):
    """Plain tensor restatement of the deformable forward (sum aggregation): (y, min_d2)."""
    Ns = s.shape[0]
    far = torch.full((1, 3), 1e6, dtype=s.dtype)
    rel = torch.cat([s, far])[idx] - q[:, None, :]
    delta = rel[:, :, None, :] - (kp[None] + off)[:, None, :, :]
    d2 = delta.pow(2).sum(-1)                                         # [N,H,K]
    min_d2 = d2.min(dim=1).values
    keep = (idx < Ns) & (d2 < ext ** 2).any(dim=2)
    if influence == "linear":
        w = (1 - d2.sqrt() / ext).clamp(min=0)
    elif influence == "gaussian":
        w = torch.exp(-d2 / (2 * (ext * 0.3) ** 2 + 1e-9))
    else:
        w = torch.ones_like(d2)
    w = w * keep[:, :, None].to(w.dtype)
    feats = torch.cat([x, torch.zeros(1, x.shape[1], dtype=x.dtype)])[idx]
    A = torch.einsum("nhk,nhc->nkc", w, feats)
    if mod is not None:
        A = A * mod[:, :, None]
    return torch.einsum("nkc,kco->no", A, W), min_d2


@pytest.mark.parametrize("name", NAMES)
def test_oracle_gradients_equal_autograd_in_float64(name):
    """Every gradient of the oracle against torch.autograd (float64) through the restatement above, 1e-10 relative."""
    c, i, o = dc.BY_NAME[name], dc.make_inputs(name), dc.oracle64(name)
    t = lambda a, grad=False: torch.from_numpy(a.astype(np.float64)).requires_grad_(grad)
    x, W, off = t(i.x, True), t(i.W, True), t(i.offsets, True)
    mod = t(i.modulations, True) if c.mod else None
    y, min_d2 = _torch_forward(t(i.q), t(i.s), torch.from_numpy(i.idx.astype(np.int64)), x, t(i.kp), W, dc.EXTENT, off, mod,
                               c.influence)
    ((y * t(i.g)).sum() + (min_d2 * t(i.gm)).sum()).backward()
    dead = dc.shadow_rows(name)
    assert rel_err(o.y, y.detach().numpy()) < 1e-10
    assert rel_err(o.min_d2, min_d2.detach().numpy()) < 1e-10
    assert rel_err(o.dx, x.grad.numpy()) < 1e-10
    assert rel_err(o.dW, W.grad.numpy()) < 1e-10
    assert rel_err(o.d_offsets, off.grad.numpy()) < 1e-10
    assert rel_err(o.d_offsets[~dead], off.grad.numpy()[~dead]) < 1e-10      # (the shadow rows are ~1e6 times larger)
    if c.mod:
        assert rel_err(o.d_modulations, mod.grad.numpy()) < 1e-10
    else:
        assert o.d_modulations is None
    # the forward alone (kpconv_forward) is the same function
    f = lambda a: None if a is None else a.astype(np.float64)
    y2, A2, _ = npref.kpconv_forward(f(i.q), f(i.s), i.idx.astype(np.int64), f(i.x), f(i.kp), f(i.W), dc.EXTENT, c.influence,
                                     offsets=f(i.offsets), modulations=f(i.modulations), return_A=True)
    assert rel_err(y2, o.y) < 1e-12
    assert rel_err(A2, o.A * f(i.modulations)[:, :, None] if c.mod else o.A) < 1e-12


def test_in_range_filter_changes_gaussian_and_constant_but_not_linear():
    """What the corrected docstring of npref.kpconv_forward says: the dense formula equals the filtered one under the
    linear influence only."""
    for name, same in (("m20", True), ("m20g", False), ("m64c", False)):
        c, i = dc.BY_NAME[name], dc.make_inputs(name)
        f = lambda a: a.astype(np.float64)
        w, d2 = npref.kpconv_weights(f(i.q), f(i.s), i.idx.astype(np.int64), f(i.kp), dc.EXTENT, c.influence, offsets=f(i.offsets))
        keep = npref.deform_in_range(i.idx, i.s.shape[0], d2, dc.EXTENT)
        real = i.idx < i.s.shape[0]
        dropped = np.abs(w * (real & ~keep)[:, :, None]).max()
        assert (dropped == 0) == same, (name, dropped)


@pytest.mark.parametrize("name,modulated", [("g4_kpconv_deform", False), ("g4_kpconv_deform_mod", True)])
def test_oracle_reproduces_deformable_golden(name, modulated):
    """Fixture G4 (the reference's deformable / modulated KPConv, loss of test_kpconv_deformable_golden) from the oracle in
    float64: the inner rigid convolution by npref.kpconv_forward / kpconv_backward, the scale and sigmoid chain here."""
    g = load_golden(name)
    K = 15
    f = lambda a: np.asarray(a, np.float64)
    q, s, idx, x, ext = f(g["q"]), f(g["s"]), g["idx"].astype(np.int64), f(g["x"]), float(g["extent"])
    okp, Wo, bo, kp, W = f(g["offset_kernel_points"]), f(g["offset_weights"]), f(g["offset_bias"]), f(g["kernel_points"]), f(g["weights"])
    feat = npref.kpconv_forward(q, s, idx, x, okp, Wo, ext) + bo
    off = feat[:, :3 * K].reshape(-1, K, 3) * ext
    mod = 2 / (1 + np.exp(-feat[:, 3 * K:])) if modulated else None
    # loss = sum(y g) + 0.5 (sum(min_d2) + sum(deformed_KP^2))
    dx, dW, d_off, d_mod, _, y, min_d2, _ = npref.kpconv_deform_backward(
        q, s, idx, x, kp, W, ext, off, mod, f(g["g"]), np.full((q.shape[0], K), 0.5))
    dkp = off + kp
    d_off = d_off + dkp
    d_feat = d_off.reshape(-1, 3 * K) * ext
    if modulated:
        d_feat = np.concatenate([d_feat, d_mod * mod * (1 - mod / 2)], 1)      # d/df of 2 sigmoid(f)
    dx_in, dWo = npref.kpconv_backward(q, s, idx, x, okp, Wo, ext, d_feat)
    for label, got, want in (("y", y, g["y"]), ("min_d2", min_d2, g["min_d2"]), ("deformed_KP", dkp, g["deformed_KP"]),
                             ("weights_grad", dW, g["weights_grad"]), ("x_grad", dx + dx_in, g["x_grad"]),
                             ("offset_weights_grad", dWo, g["offset_weights_grad"]),
                             ("offset_bias_grad", d_feat.sum(0), g["offset_bias_grad"])):
        check_err("oracle float64 vs G4 %s %s" % (name, label), rel_err(got, want), FP_TOL)


def test_case_table_covers_the_dispatch_branches():
    """The minimum coverage of the sweep, read off the table through dc.dispatch (the host code's rules restated)."""
    D = {c.name: dc.dispatch(c) for c in dc.CASES}
    mf = [c for c in dc.CASES if D[c.name]["doff"] == "mfma"]
    ve = [c for c in dc.CASES if D[c.name]["doff"] == "vector"]
    shapes = lambda cs: {(c.cin, c.H) for c in cs}
    assert {(4, 9), (16, 64), (20, 70), (64, 117), (68, 130), (256, 300), (128, 1030), (8, 40)} <= shapes(mf)
    assert all(c.Nq == 20 for c in mf if c.H == 1030) and all(c.K == 3 for c in mf if (c.cin, c.H) == (8, 40))
    assert sum(c.idx64 for c in mf) >= 3 and sum(c.idx64 for c in ve) >= 1
    assert sum(c.Nq != c.Ns for c in mf) >= 2 and any(c.Nq == c.Ns for c in mf)
    assert any(D[c.name]["ragged_block"] for c in mf) and any(D[c.name]["c0_iterations"] > 1 for c in mf)
    assert any(D[c.name]["list_cap"] > 64 for c in mf)                       # H > 256
    wpb = {(c.cin, c.H): D[c.name]["wpb"] for c in ve}
    assert wpb[(5, 40)] == 1 and wpb[(1, 12)] == 1 and wpb[(61, 150)] == 4 and wpb[(3, 300)] == 4
    assert wpb[(66, 130)] == 1 and any(c.Nq == 1025 for c in ve if c.cin == 66)
    assert (3 * 64 + 63) // 64 == 3 and (300 + 63) // 64 == 5                 # chunks of the two multi-chunk rows
    assert D["v1030"]["lds"] > 64 * 1024 and D["v1030g"]["forward"] == "lane_channel<0, DEFORM> x 3"
    assert D["v2551"]["lds"] <= 160 * 1024 < dc.doff_vector_lds(2553, 8, 12)
    for group in (mf, ve):
        for infl in ("gaussian", "constant"):
            assert len(shapes([c for c in group if c.influence == infl])) >= 2, infl
    key = lambda c: (c.cin, c.cout, c.H, c.Nq, c.Ns, c.K, c.influence)
    both = {key(c) for c in dc.CASES if c.mod} & {key(c) for c in dc.CASES if not c.mod}
    assert len(both) >= 4 and any(k[3] != k[4] for k in both)
    assert {5, 8, 20, 64, 68} <= {c.cout for c in dc.CASES if D[c.name]["gather_dx"]}
    assert {"mfma<KPM 1>", "lane_channel<0, DEFORM> x 1", "lane_channel<0, DEFORM> x 3"} <= {D[n]["forward"] for n in D}
    assert all(12 <= c.Nq <= 64 or c.Nq == 1025 for c in dc.CASES)


def test_case_inputs_meet_the_conditions_of_the_sweep():
    """From the oracle's diagnostics: an empty kink band and no arg-min tie between two support points in EVERY case (the
    only places where a correct float32 kernel may differ from float64), the two rows that keep nothing, and per
    offset-gradient kernel a wave list of more than 64 kept neighbours, a kept count that leaves a partial last tile
    and a row that keeps nothing."""
    seen = {"mfma": dict(long_list=0, partial=0, empty=0), "vector": dict(long_list=0, partial=0, empty=0)}
    single_wave_two_pieces = 0
    for c in dc.CASES:
        i, o, d = dc.make_inputs(c.name), dc.oracle64(c.name), dc.dispatch(c)
        diag = o.diag
        assert diag["kink_band"] == 0 and diag["argmin_ties"] == 0, (c.name, diag["kink_band"], diag["argmin_ties"])
        assert float(max(i.q.max(), i.s.max())) < 0.5 and float(min(i.q.min(), i.s.min())) >= 0
        real = i.idx < c.Ns
        assert not real[dc.ROW_SHADOW].any() and diag["kept"][dc.ROW_SHADOW] == 0
        assert real[dc.ROW_FAR].any() and diag["kept"][dc.ROW_FAR] == 0
        assert (diag["kept"] > 0).sum() >= 4
        lists = dc.wave_list_counts(diag["keep"], d["wpb"])
        assert lists.max() <= d["list_cap"]
        tile = 16 if d["doff"] == "mfma" else 64
        k = seen[d["doff"]]
        k["long_list"] += int((lists > 64).any())
        k["partial"] += int((diag["kept"] % tile != 0).any())
        k["empty"] += int((diag["kept"] == 0).any())
        single_wave_two_pieces += int(d["doff"] == "vector" and d["wpb"] == 1 and (diag["kept"] > 64).any())
    for kernel, k in seen.items():
        assert k["long_list"] and k["partial"] and k["empty"], (kernel, k)
    assert single_wave_two_pieces         # (v66d: pass 2 of kpconv_deform_doff<*, 1> runs more than once)


@pytest.mark.parametrize("name", NAMES)
def test_oracle_in_float32_is_inside_the_gpu_bounds(name):
    """The oracle run in float32 against its own float64 run under the bounds of the GPU sweep: what the number format
    alone costs stays inside them (measured values logged next to the bounds)."""
    c, o = dc.BY_NAME[name], dc.oracle64(name)
    r = dc.run_oracle(name, np.float32)
    dead = dc.shadow_rows(name)
    assert np.array_equal(r.diag["keep"], o.diag["keep"])
    lab = "oracle float32 vs float64 %s " % name
    dc.compare(lab + "A", r.A, o.A, FP_TOL)
    dc.compare(lab + "y", r.y, o.y, FP_TOL)
    dc.compare(lab + "min_d2", r.min_d2, o.min_d2, FP_TOL, dead)
    dc.compare(lab + "dx", r.dx, o.dx, FP_TOL)
    dc.compare(lab + "dW", r.dW, o.dW, FP_TOL)
    dc.compare(lab + "d_offsets", r.d_offsets, o.d_offsets, FP_TOL, dead)
    if c.mod:
        dc.compare(lab + "d_modulations", r.d_modulations, o.d_modulations, FP_TOL)
