"""The seeded cases of the deformable-KPConv variant sweep, shared by tests/test_deform_cpu.py (the oracle against
autograd, the conditions on the inputs) and tests/test_deform_gpu.py (the HIP kernels against the float64 oracle).

Geometry of the existing variant tests (test_kpconv_every_kernel_variant_vs_numpy_oracle): random points in a cube,
extent 0.06, kernel points ~ N(0, 0.05), offsets ~ N(0, 0.02), idx drawn from [0, Ns] (Ns = shadow) with half of the back
half of every row turned into shadow entries, plus ROW_SHADOW (shadow entries only) and ROW_FAR (a query in the far
corner: real neighbours, none within the extent of any deformed kernel point). The cube side is chosen per case so that
the kept counts the kernels branch on are reached (test_deform_cpu.py asserts them); the seed is one for which no entry
lies in the kink band |sqrt(d2)/extent - 1| < 1e-5 and no arg-min is tied between two support points, so that a correct
float32 kernel has no legitimate reason to differ from the float64 oracle anywhere and every element is compared."""
import collections
import functools

import numpy as np

EXTENT = 0.06
ROW_SHADOW = 5       # idx[ROW_SHADOW] = Ns: a row of shadow entries only
ROW_FAR = 7          # q[ROW_FAR] = FAR_CORNER: no neighbour within the extent of any deformed kernel point
FAR_CORNER = 0.49    # (coordinates stay below 0.5: float32 rounding of a distance ~ 0.06 below 2e-6 relative)

Case = collections.namedtuple("Case", "name cin cout H Nq Ns K idx64 influence mod side seed live_rows")


def _c(name, cin, cout, H, Nq=32, Ns=301, K=15, idx64=False, influence="linear", mod=False, side=0.3, seed=0,
       live_rows=None):
    return Case(name, cin, cout, H, Nq, Ns, K, idx64, influence, mod, side, seed, live_rows)


# name: m* -> kpconv_deform_doff_mfma (Cin % 4 == 0), v* -> kpconv_deform_doff (vector, Cin % 4 != 0); suffix m =
# modulated twin of the same shape, g / c = gaussian / constant influence
CASES = [
    # ---- MFMA offset gradient
    _c("m4", 4, 5, 9, Nq=12, side=0.15),
    _c("m4m", 4, 5, 9, Nq=12, mod=True, side=0.15),
    _c("m4c", 4, 5, 9, Nq=12, influence="constant", side=0.15),
    _c("m16", 16, 8, 64, Nq=40, idx64=True),                              # strided, 40 against 301
    _c("m16m", 16, 8, 64, Nq=40, idx64=True, mod=True),
    _c("m20", 20, 20, 70, Nq=33),                                          # ragged 16-channel block, 2 chunks
    _c("m20g", 20, 20, 70, Nq=33, influence="gaussian", mod=True),
    _c("m64", 64, 64, 117, Nq=64, Ns=64, idx64=True, side=0.2),            # Nq == Ns, q is s
    _c("m64m", 64, 64, 117, Nq=64, Ns=64, idx64=True, side=0.2, mod=True),
    _c("m64c", 64, 64, 117, Nq=48, influence="constant"),
    _c("m68", 68, 68, 130, Nq=40),                                         # strided; second c0 iteration holds 4 channels
    _c("m256", 256, 16, 300, Nq=24, side=0.15),                            # 4 full c0 iterations, 5 chunks over 4 waves
    _c("m260g", 260, 8, 70, Nq=24, influence="gaussian"),                  # forward on kpconv_lane_channel<8, .., 0, DEFORM>
    _c("m128", 128, 32, 1030, Nq=20, idx64=True, mod=True, side=0.12),     # list capacity 320 per wave
    _c("m8k3", 8, 8, 40, Nq=16, K=3, side=0.15),
    # ---- vector offset gradient
    _c("v5", 5, 5, 40, Nq=24, side=0.15),
    _c("v5m", 5, 5, 40, Nq=24, mod=True, side=0.15),
    _c("v5g", 5, 5, 40, Nq=24, idx64=True, influence="gaussian", side=0.15),      # int64 on WPB 1 and lane = channel
    _c("v1c", 1, 8, 12, Nq=12, influence="constant", side=0.15),
    _c("v61", 61, 20, 150, Nq=48, idx64=True),                             # WPB 4
    _c("v61m", 61, 20, 150, Nq=48, idx64=True, mod=True),
    _c("v61g", 61, 20, 150, Nq=48, influence="gaussian"),
    _c("v3", 3, 68, 300, Nq=32, side=0.12),                                # WPB 4, 5 chunks over 4 waves
    _c("v3c", 3, 68, 300, Nq=32, side=0.12, influence="constant", mod=True),
    _c("v66", 66, 64, 130, Nq=1025, seed=6),                               # Nq > 1024: WPB 1, 3 chunks in one wave
    # the same launch with rows that keep more than 64 neighbours (pass 2 of the single wave runs twice). A cube small
    # enough for that puts ~15 of the 2 M entries of 1025 full rows into the kink band whatever the seed, so only the
    # first 40 rows have neighbours here; the other 985 are further rows of shadow entries
    _c("v66d", 66, 64, 130, Nq=1025, side=0.12, seed=1, live_rows=40),
    _c("v1030", 1030, 5, 20, Nq=12, side=0.15),                           # dA block above 64 KiB of LDS
    _c("v1030g", 1030, 5, 20, Nq=12, influence="gaussian", side=0.15),    # forward: lane = channel, 3 launches
    _c("v2551", 2551, 5, 8, Nq=12, side=0.15),                            # the widest rows the LDS staging takes
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

Inputs = collections.namedtuple("Inputs", "q s idx x kp W offsets modulations g gm")


@functools.lru_cache(maxsize=None)
def make_inputs(name):
    """The float32 inputs of a case (idx int32 or int64). Cached: treat as read-only."""
    c = BY_NAME[name]
    rng = np.random.default_rng([c.seed, c.cin, c.H, c.Nq])
    s = (rng.random((c.Ns, 3)) * c.side).astype(np.float32)
    q = s.copy() if c.Nq == c.Ns else (rng.random((c.Nq, 3)) * c.side).astype(np.float32)
    q[ROW_FAR] = FAR_CORNER
    idx = rng.integers(0, c.Ns + 1, (c.Nq, c.H))
    idx[:, c.H // 2:][rng.random((c.Nq, c.H - c.H // 2)) < 0.5] = c.Ns
    idx[ROW_SHADOW] = c.Ns
    if c.live_rows is not None:
        idx[c.live_rows:] = c.Ns
    idx = idx.astype(np.int64 if c.idx64 else np.int32)
    x = rng.normal(size=(c.Ns, c.cin)).astype(np.float32)
    kp = (rng.normal(size=(c.K, 3)) * 0.05).astype(np.float32)
    W = (rng.normal(size=(c.K, c.cin, c.cout)) * 0.1).astype(np.float32)
    off = (rng.normal(size=(c.Nq, c.K, 3)) * 0.02).astype(np.float32)
    mod = (2 / (1 + np.exp(-rng.normal(size=(c.Nq, c.K))))).astype(np.float32) if c.mod else None
    g = rng.normal(size=(c.Nq, c.cout)).astype(np.float32)
    gm = rng.normal(size=(c.Nq, c.K)).astype(np.float32)
    for a in (q, s, idx, x, kp, W, off, mod, g, gm):
        if a is not None:
            a.setflags(write=False)
    return Inputs(q, s, idx, x, kp, W, off, mod, g, gm)


Oracle = collections.namedtuple("Oracle", "dx dW d_offsets d_modulations A y min_d2 diag")


def run_oracle(name, dtype=np.float64, with_gm=True):
    from oracle import npref
    c, i = BY_NAME[name], make_inputs(name)
    f = lambda a: None if a is None else a.astype(dtype)
    return Oracle(*npref.kpconv_deform_backward(f(i.q), f(i.s), i.idx.astype(np.int64), f(i.x), f(i.kp), f(i.W), EXTENT,
                                                f(i.offsets), f(i.modulations), f(i.g), f(i.gm) if with_gm else None,
                                                c.influence))


@functools.lru_cache(maxsize=None)
def oracle64(name):
    """The float64 oracle of a case, computed once per process. Read-only."""
    return run_oracle(name)


def dispatch(c):
    """The kernels a case reaches, restated from the host code (mvk_kpconv_deform_doff in csrc/deform.hip,
    mvk_kpconv_gather_fwd_ordered / launch_lane_channel in csrc/kpconv.hip, ops._KPConvFn.backward)."""
    d = {}
    chunks = (c.H + 63) // 64
    if c.cin % 4 == 0:
        d["doff"], d["wpb"] = "mfma", 4
        d["c0_iterations"] = (c.cin + 63) // 64
        d["ragged_block"] = c.cin % 16 != 0
        d["lds"] = 4 * 4 * max(64, (chunks + 3) // 4 * 64) + 4 * 4 * 48 + 16 * 16
    else:
        d["doff"] = "vector"
        d["wpb"] = 4 if (c.H > 64 and c.Nq <= 1024) else 1
        d["lds"] = doff_vector_lds(c.cin, c.H, c.Nq)
    d["list_cap"] = max(64, (chunks + d["wpb"] - 1) // d["wpb"] * 64)
    if c.influence == "linear":
        d["forward"] = "mfma<KPM 1>"
    else:
        d["forward"] = "lane_channel<0, DEFORM> x %d" % ((c.cin + 511) // 512)
    d["scatter"] = "lane_channel<1, DEFORM>%s x %d" % (" 4 waves" if c.H > 64 else "", (c.cin + 511) // 512)
    d["gather_dx"] = c.influence == "linear" and c.cout >= 5       # with rev: mvk_kpconv_gather_rev_deform
    return d


def doff_vector_lds(cin, H, Nq):
    """Dynamic LDS bytes of kpconv_deform_doff<IDX64, WPB> (host code of mvk_kpconv_deform_doff)."""
    wpb = 4 if (H > 64 and Nq <= 1024) else 1
    chunks = (H + 63) // 64
    cap = max(64, (chunks + wpb - 1) // wpb * 64)
    return 4 * 16 * ((cin + 3) & ~3) + 4 * wpb * cap + 4 * wpb * 48


def wave_list_counts(keep, wpb):
    """[Nq, wpb] kept columns per wave list: wave w walks the 64-column chunks w, w + wpb, ... of a row."""
    H = keep.shape[1]
    wave = (np.arange(H) // 64) % wpb
    return np.stack([keep[:, wave == w].sum(1) for w in range(wpb)], 1)


def row_err(got, want, scale_rows=None):
    """max over rows n of max|got[n] - want[n]| / max(max|want[n]|, 1e-2 max|want|): the per-row error the GPU tests
    bound by 1e-4. scale_rows: the rows whose largest value sets the floor (default all)."""
    got = np.asarray(got, np.float64).reshape(got.shape[0], -1)
    want = np.asarray(want, np.float64).reshape(want.shape[0], -1)
    top = np.abs(want if scale_rows is None else want[scale_rows]).max() if want.size else 0.0
    den = np.maximum(np.abs(want).max(1), 1e-2 * top)
    return float((np.abs(got - want).max(1) / np.maximum(den, 1e-300)).max()) if want.size else 0.0


ROW_TOL = 1e-4       # the per-row bound (row_err)


def shadow_rows(name):
    """Rows of shadow entries only: their min_d2 (~3e12) and d_offsets (~2e6 g_min_d2) are compared on their own scale
    (as test_kpconv_deformable_gather_closest_vs_numpy_oracle does) and do not set the floor of the other rows."""
    i = make_inputs(name)
    return (i.idx >= i.s.shape[0]).all(1)


def compare(label, got, want, bound, own_scale=None):
    """The two bounds of the sweep on one tensor, both logged (util.check_err): the max-norm rel_err < bound and the
    per-row row_err < ROW_TOL. own_scale: boolean rows compared on their own scale (shadow_rows), for the tensors
    where they are orders above the rest; every element is compared either way."""
    from util import rel_err, check_err
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (label, got.shape, want.shape)
    assert np.isfinite(got).all(), label
    if own_scale is None or not own_scale.any():
        check_err(label + " max-norm", rel_err(got, want), bound)
        check_err(label + " per-row", row_err(got, want), ROW_TOL)
        return
    check_err(label + " max-norm", rel_err(got[~own_scale], want[~own_scale]), bound)
    check_err(label + " max-norm (shadow rows)", rel_err(got[own_scale], want[own_scale]), bound)
    check_err(label + " per-row", row_err(got, want, scale_rows=~own_scale), ROW_TOL)
