"""CPU-only: the library's side of the ordered PointNet++ backwards (exports, header, ABI 9, CPU tensors refused) and
self-checks of their NumPy oracle (tests/pn2_ordered_ref.py)."""
import ctypes

import numpy as np
import pytest

import pn2_ordered_ref as ref
from test_pn2_gpu import interp_case

ORDERED_EXPORTS = ("mvk_index_csr_workspace", "mvk_index_csr", "mvk_interpolate_bwd_csr", "mvk_interpolate_bwd_csr_f64",
                   "mvk_group_points_bwd_csr", "mvk_group_points_bwd_csr_f64")


def test_library_exports_the_ordered_entry_points_at_abi_9():
    import mvkpconv
    lib_mod = mvkpconv.sub("_lib")
    raw = ctypes.CDLL(lib_mod.LIB_PATH)
    header = open(mvkpconv._ROOT + "/include/mvkpconv.h").read()
    for name in ORDERED_EXPORTS:
        assert name in lib_mod.EXPORTS and hasattr(raw, name) and (" " + name + "(") in header, name
    assert lib_mod.ABI_VERSION == 9 and lib_mod.lib().mvk_abi_version() == 9
    assert "#define MVK_ABI_VERSION 9" in header
    lib = lib_mod.lib()
    assert lib.mvk_index_csr_workspace(2, 96, 100) >= 4 * 200          # one cursor word per row at least
    assert lib.mvk_index_csr_workspace(1, 0, 0) > 0
    # the size limits are host checks: refused with the library's argument error before any launch
    word = ctypes.c_int32(0)
    p = ctypes.cast(ctypes.pointer(word), ctypes.c_void_p)
    assert lib.mvk_index_csr(p, 2, 1 << 30, 8, p, p, None, p, 1 << 40, None) == -1
    assert "2^31" in lib.mvk_last_error().decode()
    assert lib.mvk_index_csr(p, 2, 8, 1 << 30, p, p, None, p, 1 << 40, None) == -1
    assert lib.mvk_interpolate_bwd_csr(p, p, p, p, 3, 4, 1 << 30, 8, p, None) == -1


def test_index_csr_refuses_cpu_tensors_and_other_dtypes():
    import torch
    import mvkpconv
    ops = mvkpconv.sub("ops")
    with pytest.raises(RuntimeError, match="HBM"):
        ops.index_csr(torch.zeros(1, 8, 3, dtype=torch.int64), 4)
    assert ops.index_csr_for(torch.zeros(1, 8, 3, dtype=torch.int64), 4) is None


def test_oracle_csr_on_a_case_written_out():
    index = np.array([[[2, 0, 2], [-1, 2, 5], [0, 0, 1]],
                      [[1, 1, 1], [1, 4, 1], [3, 3, 3]]], np.int64)       # n1 = 4: the 5, the 4 and the -1 are in no row
    row_start, entries = ref.csr(index, 4)
    assert row_start.dtype == np.int32 and entries.dtype == np.int32
    assert row_start.tolist() == [0, 3, 4, 7, 7, 7, 12, 12, 15]
    assert entries.tolist() == [1, 6, 7, 8, 0, 2, 4, 0, 1, 2, 3, 5, 6, 7, 8]
    assert np.array_equal(ref.counts(index, 4), [[3, 1, 3, 0], [0, 5, 0, 3]])
    assert np.array_equal(ref.csr(index.reshape(2, 9), 4)[1], entries)
    row_start, entries = ref.csr(np.zeros((2, 0, 3), np.int64), 3)
    assert row_start.tolist() == [0] * 7 and entries.size == 0


def test_oracle_sums_are_the_sequential_float32_sums():
    f, idx, w, go = interp_case(3, 65, 129, 513, False)
    w32, go32 = w.astype(np.float32), go.astype(np.float32)
    got = ref.interpolate_bwd(go32, idx, w32, 129)
    assert got.dtype == np.float32 and got.shape == (3, 65, 129)
    b, c = 1, 17
    products = np.repeat(go32[b, c], 3) * w32[b].reshape(-1)
    assert products.dtype == np.float32
    want = ref.ordered_sum_loop(products, idx[b].reshape(-1), 129)
    assert np.array_equal(got[b, c].view(np.int32), want.view(np.int32))
    # and through the CSR: row by row, entries ascending
    row_start, entries = ref.csr(idx, 129)
    for j in (0, 64, 128):
        acc = np.float32(0)
        row = entries[row_start[b * 129 + j]:row_start[b * 129 + j + 1]]
        assert np.all(np.diff(row) > 0)
        for p in row:
            acc = np.float32(acc + products[p])
        assert acc.view(np.int32) == got[b, c, j].view(np.int32)
    # grouping is the same walk without the product
    g = np.random.default_rng(3).standard_normal((2, 3, 40, 5)).astype(np.float32)
    gidx = ref.ball_like_index(2, 40, 5, 11, seed=4)
    assert (gidx == -1).any() and (gidx[..., -1] == gidx[..., 0]).any()
    got = ref.group_points_bwd(g, gidx, 11)
    want = ref.ordered_sum_loop(g[1, 2].reshape(-1), gidx[1].reshape(-1), 11)
    assert np.array_equal(got[1, 2].view(np.int32), want.view(np.int32))


def test_oracle_tells_the_ascending_order_from_another_order():
    """What the bit-equality of the GPU test rests on: on its case the order of the float32 additions matters."""
    f, idx, w, go = interp_case(3, 65, 129, 513, False)
    w32, go32 = w.astype(np.float32), go.astype(np.float32)
    ascending = ref.interpolate_bwd(go32, idx, w32, 129)
    ix = ref.flat_index(idx)
    products = np.repeat(go32, 3, axis=2) * w32.reshape(3, 1, -1)
    descending = ref._ordered(np.ascontiguousarray(products[..., ::-1]), np.ascontiguousarray(ix[:, ::-1]), 129)
    differ = float((ascending.view(np.int32) != descending.view(np.int32)).mean())
    longest = int(ref.counts(idx, 129).max())
    print("descending instead of ascending: %.1f %% of the elements differ, longest row %d" % (100 * differ, longest))
    assert differ > 0.5 and longest >= 16
    assert np.allclose(ascending, descending, rtol=0, atol=1e-4)         # the same sums up to rounding
