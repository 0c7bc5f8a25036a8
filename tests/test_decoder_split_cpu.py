"""CPU: the float64 restatement of the decoder's split form (tests/decoder_split_ref.py) against the concatenated form
(tests/gemm_ref.upsample_cat_linear). Integer inputs: every product and every sum is exact, so the two forms agree to
the bit. Random inputs: they differ by float64 rounding alone -- two summation orders of the same terms, each within
(terms in the longest chain) * 2^-53 of the sum of the terms' magnitudes."""
import numpy as np
import pytest

import decoder_split_ref as dref
import gemm_ref

NAMES = ("y", "dx", "dskip", "dW")
VARIANTS = [(False, False), (True, False), (False, True), (True, True)]


@pytest.mark.parametrize("case", dref.CASES + dref.STATS_CASES, ids=str)
@pytest.mark.parametrize("shadow,two_d", VARIANTS)
def test_split_form_equals_the_concatenated_form_exactly_on_integers(case, shadow, two_d):
    x, idx, skip, W, g = dref.inputs(case, shadow, two_d, integers=True)
    got, want = dref.split_form(x, idx, skip, W, g), gemm_ref.upsample_cat_linear(x, idx, skip, W, g)
    for name in NAMES:
        assert got[name].shape == want[name].shape and np.array_equal(got[name], want[name]), name


@pytest.mark.parametrize("case", dref.CASES + dref.STATS_CASES, ids=str)
@pytest.mark.parametrize("shadow,two_d", VARIANTS)
def test_split_form_equals_the_concatenated_form_at_float64_rounding(case, shadow, two_d):
    Ns, Nq, C1, C2, N = case
    x, idx, skip, W, g = dref.inputs(case, shadow, two_d)
    got, want = dref.split_form(x, idx, skip, W, g), gemm_ref.upsample_cat_linear(x, idx, skip, W, g)
    # the same expressions over the magnitudes: the sum of |term| behind every output element
    mag = gemm_ref.upsample_cat_linear(np.abs(x), idx, np.abs(skip), np.abs(W), np.abs(g))
    chain = C1 + C2 + N + Nq          # no output sums more terms than this in either form
    for name in NAMES:
        bound = 2.0 * (chain + 2) * 2.0 ** -53 * mag[name]
        assert (np.abs(got[name] - want[name]) <= bound).all(), name


def test_shadow_rows_add_nothing_and_statistics_cover_the_valid_rows():
    case = dref.CASES[0]
    Ns, Nq, C1, C2, N = case
    x, idx, skip, W, g = dref.inputs(case, shadow=True)
    r = dref.split_form(x, idx, skip, W, g, n_valid=Nq - 7)
    j = dref.first_column(idx, Ns)
    sh = j == Ns
    assert sh.sum() == Nq // 3
    np.testing.assert_array_equal(r["y"][sh], skip.astype(np.float64)[sh] @ W.astype(np.float64)[:, C1:].T)
    np.testing.assert_allclose(r["stat_sum"], r["y"][:Nq - 7].sum(0), rtol=0, atol=0)
    assert r["stat_m2"].shape == (N,) and (r["stat_m2"] >= 0).all()
    # coarse rows nobody points at receive no gradient
    unused = np.setdiff1d(np.arange(Ns), j)
    assert not r["dx"][unused].any()
