"""Adversarial clouds for grid subsampling and the radius search (NumPy only; shared by test_cloud_cases_cpu.py,
test_cloud_cases_gpu.py and golden/make_cloud_cases.py).

Every other seeded cloud of the suite is rng.random((n, 3)) * box: non-negative, scattered, free of duplicates and never
on a voxel edge. The families here are the inputs such clouds never produce:

  S1 lattice     points ON voxel boundaries and one ulp below them, at four offsets of the lattice
  S2 columns     voxel keys iX + NX*iY + NX*NY*iZ that all fall into ONE bucket of the unordered_map's growth schedule
  S3 thresholds  voxel counts at, one below and one above every rehash threshold 13, 29, 59, 127, ...
  S4 duplicates  one point many times; every point several times
  S5 degenerate  planar (z = -0.0) and collinear clouds
  S6 signed      a ragged signed batch (a one-point cloud, an empty cloud, clouds on both sides of the multi-workgroup
                 threshold) with features, labels, label ties and max_p
  N1 lattice     neighbour rows full of exact d2 ties, supports at exactly d2 == r*r
  N2 co-located  every support three times
  N3 planar      a ragged planar batch, queries off the supports
  N4 one support and a radius larger than the cloud
  N5 cell growth two clusters 500 apart under a small radius
  N6 far queries queries at +-1e4 and +-1e9: every row is padding
  N7 wide rows   600 in-range supports per query

sub_cases() / nb_cases() return {name: case} in a fixed order, built once per process from fixed seeds; the arrays are
read-only. No voxel holds more than 2 000 points (the kernels sort a voxel's members with one lane)."""
import collections
import functools

import numpy as np

SubCase = collections.namedtuple("SubCase", "points lens dl features labels max_p reference")
SubCase.__doc__ = """(points [N,3] f32, lens [B] i32, dl, features [N,fdim] f32 | None, labels [N,ldim] i32 | None, max_p,
reference): reference=False marks inputs the compiled reference core cannot run (an empty cloud in the batch, ldim = 2 in
a batch of several clouds); for those the C oracle stands alone."""
NbCase = collections.namedtuple("NbCase", "queries supports q_lens s_lens radius tie_free ref_rows")
NbCase.__doc__ = """(queries [Nq,3] f32, supports [Ns,3] f32, q_lens [B] i32, s_lens [B] i32, radius, tie_free, ref_rows):
tie_free=True: no row holds two supports at the same float32 d2, so the reference's order is defined and must be met
exactly; otherwise rows are compared with tie groups as sets. ref_rows: the leading query rows on which the compiled
reference core is a referee -- all of them, except that the reference steps ONE cloud forward when a cloud's queries
end (neighbors.cpp:272 is an `if`, not a loop): after a cloud WITHOUT queries it searches every later query in the wrong
cloud's supports, so only the rows in front of such a cloud count; for the rest the C oracle stands alone."""

# voxel counts around the bucket counts of libstdc++'s growth schedule (13, 29, 59, 127, 257, 541, 1109)
S3_COUNTS = (1, 2, 12, 13, 14, 28, 29, 30, 58, 59, 60, 126, 127, 128, 256, 257, 258, 540, 541, 542, 1108, 1109, 1110)
S2_DIMS = ((13, 1, 200), (1, 29, 300), (13, 29, 100), (59, 1, 500), (127, 2, 50))
S1_OFFSETS = (0, -7, -1000, 513)
S1_LARGE_OFFSETS = (-7, 513)
MULTI_MIN = 8192          # points per cloud from which the multi-workgroup front end of the subsampling runs


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _freeze(case):
    for a in case:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return case


def _sub(points, lens, dl, features=None, labels=None, max_p=0, reference=True):
    points, lens = _f32(points), np.ascontiguousarray(lens, dtype=np.int32)
    assert points.shape == (int(lens.sum()), 3)
    if features is not None:
        features = _f32(features)
    if labels is not None:
        labels = np.ascontiguousarray(labels, dtype=np.int32)
    return _freeze(SubCase(points, lens, float(dl), features, labels, int(max_p), bool(reference)))


def _nb(queries, supports, q_lens, s_lens, radius, tie_free):
    q, s = _f32(queries), _f32(supports)
    ql, sl = np.ascontiguousarray(q_lens, dtype=np.int32), np.ascontiguousarray(s_lens, dtype=np.int32)
    assert q.shape == (int(ql.sum()), 3) and s.shape == (int(sl.sum()), 3) and ql.shape == sl.shape
    empty = np.flatnonzero(ql[:-1] == 0)
    ref_rows = int(ql[:empty[0]].sum()) if len(empty) else len(q)
    return _freeze(NbCase(q, s, ql, sl, float(np.float32(radius)), bool(tie_free), ref_rows))


def _lattice(shape, off, pitch):
    """float32(g + off) * float32(pitch) over the integer nodes g of a block: one float32 product per coordinate."""
    g = np.stack(np.meshgrid(*[np.arange(n) for n in shape], indexing="ij"), -1).reshape(-1, 3)
    return (g + off).astype(np.float32) * np.float32(pitch)


def _signed(rng, n, box=(3, 2, 1)):
    return ((rng.random((n, 3)) - 0.5) * np.asarray(box, np.float64)).astype(np.float32)


# ---------------------------------------------------------------------------------------------- subsampling

def _s1(cases):
    for shape, offsets, tag in (((20, 17, 9), S1_OFFSETS, "S1_lattice"), ((40, 30, 9), S1_LARGE_OFFSETS, "S1_lattice_large")):
        for off in offsets:
            rng = np.random.default_rng([1, shape[0], off + 2000])
            p = _lattice(shape, off, 0.04)
            p = p[rng.permutation(len(p))]
            below = np.nextafter(p, np.float32(-np.inf))          # one ulp towards -inf, in a cloud of its own
            cases["%s_off%d" % (tag, off)] = _sub(np.concatenate([p, below]), [len(p), len(p)], 0.04)


def _s2(cases):
    dl = 0.1
    for nx, ny, nz in S2_DIMS:
        rng = np.random.default_rng([2, nx, ny, nz])
        cells = np.concatenate([np.stack([np.zeros(nz), np.zeros(nz), np.arange(nz)], 1), [[nx - 1, ny - 1, 0]]])
        p = ((cells + 0.5) * dl).astype(np.float32)              # cell centres: the column ix = iy = 0 and the corner pin
        cases["S2_column_%dx%dx%d" % (nx, ny, nz)] = _sub(p[rng.permutation(len(p))], [len(p)], dl)


def _s3_cloud(rng, m, dl):
    flat = rng.choice(40 * 40 * 4, size=m, replace=False)
    cells = np.stack(np.unravel_index(flat, (40, 40, 4)), 1) - 2          # signed cell coordinates
    p = (np.repeat(cells, 3, axis=0) + 0.1 + 0.8 * rng.random((3 * m, 3))) * dl      # three points well inside each voxel
    return p[rng.permutation(len(p))].astype(np.float32)


def _s3(cases):
    dl = 0.05
    clouds = []
    for m in S3_COUNTS:
        p = _s3_cloud(np.random.default_rng([3, m]), m, dl)
        clouds.append(p)
        cases["S3_voxels_%d" % m] = _sub(p, [len(p)], dl)
    cases["S3_voxels_all"] = _sub(np.concatenate(clouds), [len(c) for c in clouds], dl)    # every count in one batch


def _s4(cases):
    rng = np.random.default_rng([4])
    one = np.asarray([[-0.37, 1.21, -2.5]], np.float32)
    cases["S4_duplicates_one_point"] = _sub(np.repeat(one, 1500, axis=0), [1500], 0.1)
    p = np.tile(_signed(rng, 300), (7, 1))
    cases["S4_duplicates_7x300"] = _sub(p[rng.permutation(len(p))], [1000, 1100], 0.1)


def _s5(cases):
    rng = np.random.default_rng([5])
    p = _signed(rng, 5000)
    p[:, 2] = -0.0
    cases["S5_degenerate_plane"] = _sub(p, [5000], 0.04)
    q = p.copy()
    q[:, 1] = np.float32(-0.25)
    cases["S5_degenerate_line"] = _sub(q, [5000], 0.003)


def _s6(cases):
    rng = np.random.default_rng([6])
    n = 30000
    p = _signed(rng, n)
    feats = (rng.random((n, 5)) * 2 - 1).astype(np.float32)
    lab1 = rng.integers(-3, 3, (n, 1)).astype(np.int32)
    lab2 = np.concatenate([lab1, rng.integers(-20, 20, (n, 1)).astype(np.int32)], 1)
    tie = (np.arange(n) % 2).astype(np.int32).reshape(-1, 1)
    variants = [("points", {}), ("fdim1", dict(features=feats[:, :1])), ("fdim3", dict(features=feats[:, :3])),
                ("fdim5", dict(features=feats)), ("ldim1", dict(labels=lab1)), ("ldim2", dict(labels=lab2)),
                ("fdim3_ldim1", dict(features=feats[:, 1:4], labels=lab1)), ("maxp100", dict(max_p=100)),
                ("label_ties", dict(labels=tie, dl=0.2))]
    for name, kw in variants:
        kw = dict(kw)
        dl = kw.pop("dl", 0.06)
        ldim = kw["labels"].shape[1] if "labels" in kw else 0
        # a one-point cloud, an empty cloud and clouds on both sides of the multi-workgroup threshold
        cases["S6_signed_%s_with_empty" % name] = _sub(p, [9000, 1, 0, 20999], dl, reference=False, **kw)
        cases["S6_signed_%s" % name] = _sub(p, [9000, 1, 20999], dl, reference=ldim < 2, **kw)
    cases["S6_signed_ldim2_one_cloud"] = _sub(p[:9000], [9000], 0.06, labels=lab2[:9000])


@functools.lru_cache(maxsize=None)
def sub_cases():
    cases = collections.OrderedDict()
    for fam in (_s1, _s2, _s3, _s4, _s5, _s6):
        fam(cases)
    return cases


# ---------------------------------------------------------------------------------------------- neighbours

N1_RADII = (("r0.05", np.float32(0.05)), ("r0.1", np.float32(0.1)), ("r0.15", np.float32(0.15)),
            ("r0.05sqrt2", np.float32(0.05) * np.float32(np.sqrt(2.0))))


def _n3_supports():
    rng = np.random.default_rng([13])
    s = _signed(rng, 3000, (3, 2, 0))
    s[:, 2] = 0.0
    return s, np.asarray([1000, 500, 1500], np.int32)


@functools.lru_cache(maxsize=None)
def nb_cases():
    cases = collections.OrderedDict()
    # N1: every distance between lattice nodes occurs many times; nodes at exactly one, two, three pitches and at the
    # diagonal sit on d2 == r*r up to the rounding of the float32 products
    for off in (0, -6):
        p = _lattice((12, 12, 6), off, 0.05)
        for tag, r in N1_RADII:
            cases["N1_lattice_off%d_%s" % (off, tag)] = _nb(p, p, [len(p)], [len(p)], r, False)
    # N2: co-located supports (d2 ties of three at every distance), two clouds
    rng = np.random.default_rng([12])
    s = np.tile(_signed(rng, 400, (1.5, 1.0, 0.5)), (3, 1))
    s = s[rng.permutation(len(s))]
    cases["N2_colocated_supports"] = _nb(s[:500], s, [250, 250], [600, 600], 0.2, False)
    # N3: planar, ragged, a cloud without queries; the queries lie off the supports
    s3, sl3 = _n3_supports()
    cases["N3_planar_ragged"] = _nb(s3[:1000] * np.float32(1.3), s3, [400, 0, 600], sl3, 0.07, True)
    # (the same rows with queries in every cloud: the form on which the reference referees all rows, see NbCase)
    cases["N3_planar_ragged_no_empty"] = _nb(s3[:1000] * np.float32(1.3), s3, [400, 100, 500], sl3, 0.07, True)
    # N4: one support, every query within the radius or not at all
    rng = np.random.default_rng([14])
    cases["N4_one_support"] = _nb(_signed(rng, 10, (8, 8, 8)), [[0.3, -0.2, 0.1]], [10], [1], 5.0, True)
    # N5: a bounding box of 500^3 under r = 0.03: the cell of the support grid grows by 1.3 until the grid fits
    rng = np.random.default_rng([15])
    a = _signed(rng, 50, (0.1, 0.1, 0.1))
    b = (_signed(rng, 50, (0.1, 0.1, 0.1)).astype(np.float64) + 500.0).astype(np.float32)
    s = np.concatenate([a, b])
    between = (rng.random((20, 1)) * 500.0 + _signed(rng, 20, (0.1, 0.1, 0.1))).astype(np.float32)
    cases["N5_cell_growth"] = _nb(np.concatenate([s, between]), s, [120], [100], 0.03, True)
    # N6: queries far outside the support grid (cell coordinates beyond int range at 1e9): all padding
    far = []
    for mag in (1e4, 1e9):
        for sign in (1.0, -1.0):
            for axis in range(3):
                v = np.zeros(3)
                v[axis] = sign * mag
                far.append(v)
            far.append(np.full(3, sign * mag))
    cases["N6_far_queries"] = _nb(np.asarray(far), s3, [6, 4, 6], sl3, 0.07, True)
    # N7: rows of 600 entries (the wide-row kernels; below their 1 024-entry list)
    rng = np.random.default_rng([17])
    d = rng.standard_normal((600, 3))
    s = (d / np.linalg.norm(d, axis=1, keepdims=True) * 0.05 * rng.random((600, 1)) ** (1.0 / 3.0)).astype(np.float32)
    cases["N7_wide_rows"] = _nb(s, s, [600], [600], 0.2, False)
    return cases


# ---------------------------------------------------------------------------------------------- properties

def voxel_keys(points, dl):
    """(iX, iY, iZ, NX, NY) of one cloud in the reference's float32 arithmetic (grid_subsampling.cpp:25-56):
    origin = floor(min * (1 / dl)) * dl, index = floor((p - origin) / dl)."""
    p, dl = _f32(points), np.float32(dl)
    inv = np.float32(1) / dl
    org = np.floor(p.min(0) * inv) * dl
    idx = np.floor((p - org) / dl).astype(np.int64)
    nx, ny = (np.floor((p.max(0)[:2] - org[:2]) / dl).astype(np.int64) + 1).tolist()
    return idx[:, 0], idx[:, 1], idx[:, 2], nx, ny


def voxel_stats(case):
    """Per cloud of a subsampling case: (number of voxels, largest member count, NX, NY)."""
    out, o = [], 0
    for n in case.lens.tolist():
        if n == 0:
            out.append((0, 0, 0, 0))
            continue
        ix, iy, iz, nx, ny = voxel_keys(case.points[o:o + n], case.dl)
        _, counts = np.unique(ix + nx * iy + nx * ny * iz, return_counts=True)
        out.append((len(counts), int(counts.max()), nx, ny))
        o += n
    return out


def rows_with_ties(case):
    """Number of query rows that hold two in-range supports at the same float32 d2."""
    ties = 0
    q0 = s0 = 0
    r2 = np.float32(case.radius) * np.float32(case.radius)
    for nq, ns in zip(case.q_lens.tolist(), case.s_lens.tolist()):
        q, s = case.queries[q0:q0 + nq], case.supports[s0:s0 + ns]
        for i in range(0, nq, 256):
            d = q[i:i + 256, None, :] - s[None]
            d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
            srt = np.sort(np.where(d2 < r2, d2, np.float32(np.inf)), axis=1)
            ties += int(((srt[:, 1:] == srt[:, :-1]) & np.isfinite(srt[:, 1:])).any(axis=1).sum())
        q0 += nq
        s0 += ns
    return ties


# ---------------------------------------------------------------------------------------------- fixture records

STORE_POINTS = 8000        # cases of more input points are kept in the fixture as digests
STORE_BYTES = 1 << 16      # so are output arrays of more bytes


def digest(a):
    """SHA-256 over dtype, shape and bytes of an array."""
    import hashlib
    a = np.ascontiguousarray(a)
    return hashlib.sha256(("%s%s" % (a.dtype.str, a.shape)).encode() + a.tobytes()).hexdigest()


def put(rec, key, a, store):
    """The array itself, or its digest under key + '.sha256'."""
    a = np.ascontiguousarray(a)
    if store:
        rec[key] = a
    else:
        rec[key + ".sha256"] = np.asarray(digest(a))


def sub_inputs(case):
    arrs = collections.OrderedDict(points=case.points, lens=case.lens, dl=np.float64(case.dl), max_p=np.int32(case.max_p))
    if case.features is not None:
        arrs["features"] = case.features
    if case.labels is not None:
        arrs["labels"] = case.labels
    return arrs


def sub_outputs(result, case):
    """Names for the tuple of subsample_batch: (points, lens[, features][, labels])."""
    names = ["out_points", "out_lens"] + (["out_features"] if case.features is not None else []) + \
        (["out_labels"] if case.labels is not None else [])
    assert len(names) == len(result)
    return collections.OrderedDict(zip(names, result))


def nb_inputs(case):
    return collections.OrderedDict(queries=case.queries, supports=case.supports, q_lens=case.q_lens, s_lens=case.s_lens,
                                   radius=np.float32(case.radius))


def trim_rows(nb, rows, n_supports):
    """The first `rows` rows without the columns that are padding in all of them."""
    nb = nb[:rows]
    w = int((nb < n_supports).sum(1).max()) if nb.size else 0
    assert (nb[:, w:] == n_supports).all()
    return np.ascontiguousarray(nb[:, :w])
