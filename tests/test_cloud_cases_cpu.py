"""CPU: the C oracle on the boundary, collision and tie clouds of tests/cloud_cases.py, against what the reference core
gave on them (tests/golden/g19_cloud_cases.npz, make_cloud_cases.py) and against the live core where oracle/_ref is built.
Subsampling bit for bit, output order included; neighbour rows exactly where the case is tie-free, with tie groups as sets
otherwise. The GPU twin (test_cloud_cases_gpu.py) then holds the kernels to this oracle."""
import functools

import numpy as np
import pytest

import cloud_cases as cc
from conftest import load_golden
from oracle import cport
from util import bits_equal, assert_neighbors_equal_mod_ties, canon_ties, nb_d2

SUB, NB = cc.sub_cases(), cc.nb_cases()
FAMILIES = ["S1", "S2", "S3", "S4", "S5", "S6", "N1", "N2", "N3", "N4", "N5", "N6", "N7"]


@functools.lru_cache(maxsize=None)
def fixture():
    return load_golden("g19_cloud_cases")


@functools.lru_cache(maxsize=None)
def oracle_sub(name):
    c = SUB[name]
    return cport.subsample_batch(c.points, c.lens, c.features, c.labels, c.dl, c.max_p)


@functools.lru_cache(maxsize=None)
def oracle_nb(name):
    c = NB[name]
    return cport.radius_neighbors_batch(c.queries, c.supports, c.q_lens, c.s_lens, c.radius)


def same(a, b):
    """Same dtype, shape and bytes."""
    return bits_equal(np.ascontiguousarray(a), np.ascontiguousarray(b))


def match(g, key, a):
    """a against the fixture entry: the stored array, or its digest."""
    if key in g:
        assert same(a, g[key]), key
    else:
        assert cc.digest(a) == str(g[key + ".sha256"]), key


# ---------------------------------------------------------------------------------------------- the cases themselves

def test_every_family_has_cases():
    for fam in FAMILIES:
        assert any(n.startswith(fam + "_") for n in list(SUB) + list(NB)), fam
    assert all(n[:2] in FAMILIES for n in list(SUB) + list(NB))


def test_S1_lattice_points_lie_on_voxel_boundaries_and_one_ulp_below():
    for name, c in SUB.items():
        if not name.startswith("S1_"):
            continue
        n = int(c.lens[0])
        on, below = c.points[:n], c.points[n:]
        assert np.array_equal(np.nextafter(below, np.float32(np.inf)), on) and (below < on).all()
        node = np.rint(on.astype(np.float64) / 0.04)
        assert np.array_equal((node.astype(np.float32) * np.float32(0.04)), on)          # float32(g + off) * float32(dl)
        # the ulp matters: the two clouds fall into different numbers of voxels
        assert oracle_sub(name)[1][0] != oracle_sub(name)[1][1], name
        assert (n >= cc.MULTI_MIN) == ("large" in name)


def test_S2_columns_share_one_bucket_of_the_growth_schedule():
    for (nx, ny, nz), name in zip(cc.S2_DIMS, [n for n in SUB if n.startswith("S2_")]):
        c = SUB[name]
        ix, iy, iz, NX, NY = cc.voxel_keys(c.points, c.dl)
        assert (NX, NY) == (nx, ny), name
        keys = ix + NX * iy + NX * NY * iz
        column = keys[(ix == 0) & (iy == 0)]
        assert len(column) == nz and len(np.unique(keys)) == nz + 1
        nb = [b for b in (13, 29, 59, 127) if (NX * NY) % b == 0]
        assert nb and all((column % b == 0).all() for b in nb), name                     # one chain of nz elements


def test_S3_voxel_counts_sit_on_the_rehash_thresholds():
    for m in cc.S3_COUNTS:
        c = SUB["S3_voxels_%d" % m]
        assert cc.voxel_stats(c)[0][:2] == (m, 3) and oracle_sub("S3_voxels_%d" % m)[1].tolist() == [m]
    assert oracle_sub("S3_voxels_all")[1].tolist() == list(cc.S3_COUNTS)
    for nb in (13, 29, 59, 127, 257, 541, 1109):
        assert {nb - 1, nb, nb + 1} <= set(cc.S3_COUNTS)


def test_S4_S5_S6_shapes_and_the_member_bound():
    assert oracle_sub("S4_duplicates_one_point")[1].tolist() == [1]
    # (1 500 sequential float32 additions: the barycentre of equal points is not the point, bit for bit)
    assert np.abs(oracle_sub("S4_duplicates_one_point")[0] - SUB["S4_duplicates_one_point"].points[:1]).max() < 1e-4
    p = SUB["S4_duplicates_7x300"].points
    assert len(np.unique(p, axis=0)) == 300 and len(p) == 2100
    plane, line = SUB["S5_degenerate_plane"].points, SUB["S5_degenerate_line"].points
    assert np.signbit(plane[:, 2]).all() and (plane[:, 2] == 0).all() and (plane[:, :2] < 0).any() and (plane[:, :2] > 0).any()
    assert len(np.unique(line[:, 1])) == 1 and np.signbit(line[:, 2]).all()
    s6 = SUB["S6_signed_points_with_empty"]
    assert s6.lens.tolist() == [9000, 1, 0, 20999] and s6.lens[0] >= cc.MULTI_MIN > 1 and (s6.points < 0).any()
    for name, c in SUB.items():
        assert max(s[1] for s in cc.voxel_stats(c)) <= 2000, name
        assert c.reference == bool((c.lens > 0).all() and (c.labels is None or c.labels.shape[1] < 2 or len(c.lens) == 1)), name


def test_neighbour_cases_tie_and_boundary_properties():
    for name, c in NB.items():
        assert (cc.rows_with_ties(c) == 0) == c.tie_free, name
        assert c.tie_free == (name[:2] in ("N3", "N4", "N5", "N6")), name
        assert c.ref_rows == (400 if name == "N3_planar_ragged" else len(c.queries)), name
    # N1: supports at exactly d2 == r*r exist and are excluded (strict <)
    c = NB["N1_lattice_off0_r0.05"]
    r2 = np.float32(c.radius) * np.float32(c.radius)
    d2 = nb_d2(c.queries, c.supports, c.q_lens, c.s_lens, np.tile(np.arange(864, dtype=np.int32), (864, 1)))
    assert (d2 == r2).sum() > 864                                                         # (where the differences round that way)
    nb = oracle_nb("N1_lattice_off0_r0.05")
    got = nb_d2(c.queries, c.supports, c.q_lens, c.s_lens, nb)
    assert (got[np.isfinite(got)] < r2).all() and ((d2 < r2).sum(1) == (nb < 864).sum(1)).all()
    assert (oracle_nb("N2_colocated_supports") < 1200).sum(1).min() >= 3                   # itself, three times
    assert oracle_nb("N4_one_support").shape == (10, 1) and 0 < (oracle_nb("N4_one_support") == 0).sum() < 10
    assert oracle_nb("N6_far_queries").shape == (16, 0)
    assert oracle_nb("N7_wide_rows").shape == (600, 600) and (oracle_nb("N7_wide_rows") < 600).all()
    n5 = oracle_nb("N5_cell_growth")
    assert (n5[:100, 0] == np.arange(100)).all() and (n5[100:] == 100).all()              # the points in between see nothing
    assert ((n5[:50] < 50) | (n5[:50] == 100)).all() and (n5[50:100] >= 50).all()         # no row crosses the clusters


# ---------------------------------------------------------------------------------------------- subsampling

@pytest.mark.parametrize("name", [n for n, c in SUB.items() if c.reference])
def test_subsample_oracle_vs_reference(name):
    """Inputs first (a drifted generator must not read as a wrong oracle), then every output, bit for bit: against the
    fixture always, against the live reference core where it is built."""
    c, g, res = SUB[name], fixture(), oracle_sub(name)
    pre = "sub/%s/" % name
    for k, a in cc.sub_inputs(c).items():
        match(g, pre + k, a)
    for k, a in cc.sub_outputs(res, c).items():
        match(g, pre + k, a)
    if cport.ref() is not None:
        live = cport.subsample_batch(c.points, c.lens, c.features, c.labels, c.dl, c.max_p, impl="ref")
        assert len(live) == len(res)
        for a, b in zip(res, live):
            assert same(a, b)


@pytest.mark.parametrize("name", [n for n, c in SUB.items() if not c.reference])
def test_subsample_oracle_alone_is_consistent_with_its_refereed_twin(name):
    """Inputs the reference core cannot run (never handed to it). An empty cloud adds a zero count and nothing else;
    the first of two label columns votes as it does alone. The twins are refereed above."""
    c, res = SUB[name], oracle_sub(name)
    assert name.startswith("S6_signed_")
    twin = name.replace("_with_empty", "")
    if "ldim2" in name:
        one = oracle_sub(twin.replace("ldim2", "ldim1"))
        assert same(res[0], one[0]) and same(res[-1][:, :1], one[-1])
        n0 = int(oracle_sub("S6_signed_ldim2_one_cloud")[1][0])
        assert same(res[-1][:n0], oracle_sub("S6_signed_ldim2_one_cloud")[-1])            # the first cloud, refereed
    if name.endswith("_with_empty"):
        want = oracle_sub(twin)
        assert (c.lens == 0).sum() == 1 and res[1].tolist() == want[1].tolist()[:2] + [0] + want[1].tolist()[2:]
        assert all(same(a, b) for a, b in zip(res[:1] + res[2:], want[:1] + want[2:]))


# ---------------------------------------------------------------------------------------------- neighbours

def check_rows(name, got, want):
    """Oracle rows against reference rows (both without all-padding columns): exact for tie-free cases."""
    c = NB[name]
    if c.tie_free:
        assert got.shape == want.shape and np.array_equal(got, want), name
    else:
        assert_neighbors_equal_mod_ties(got, want, c.queries[:c.ref_rows], c.supports, c.q_lens, c.s_lens)


def brute_force_rows(c, width):
    """Every support of the query's own cloud with float32 d2 < r*r, ascending (d2, index), padded with Ns."""
    out = np.full((len(c.queries), width), len(c.supports), np.int32)
    r2 = np.float32(c.radius) * np.float32(c.radius)
    q0 = s0 = 0
    for nq, ns in zip(c.q_lens.tolist(), c.s_lens.tolist()):
        idx = np.tile(np.arange(s0, s0 + ns, dtype=np.int32), (nq, 1))
        d2 = nb_d2(c.queries[q0:q0 + nq], c.supports, None, None, idx)
        for i in range(nq):
            keep = np.flatnonzero(d2[i] < r2)
            keep = keep[np.lexsort((idx[i][keep], d2[i][keep]))]
            out[q0 + i, :len(keep)] = idx[i][keep]
        q0 += nq
        s0 += ns
    return out


@pytest.mark.parametrize("name", list(NB))
def test_neighbors_oracle_vs_reference(name):
    c, g, nb = NB[name], fixture(), oracle_nb(name)
    ns = len(c.supports)
    pre = "nb/%s/" % name
    for k, a in cc.nb_inputs(c).items():
        match(g, pre + k, a)
    assert int(g[pre + "ref_rows"]) == c.ref_rows > 0
    assert nb.dtype == np.int32 and nb.shape[0] == len(c.queries)
    mine = cc.trim_rows(nb, c.ref_rows, ns)
    # the oracle's own order is the canonical one: ascending (d2, index)
    assert np.array_equal(canon_ties(mine, nb_d2(c.queries[:c.ref_rows], c.supports, c.q_lens, c.s_lens, mine)), mine)
    if pre + "out" in g:
        check_rows(name, mine, g[pre + "out"])
    else:
        assert cc.digest(mine) == str(g[pre + "out_canonical.sha256"])
    if cport.ref() is not None:
        live = cport.radius_neighbors_batch(c.queries, c.supports, c.q_lens, c.s_lens, c.radius, impl="ref")
        check_rows(name, mine, cc.trim_rows(live, c.ref_rows, ns))
    if c.ref_rows < len(c.queries):
        # past the cloud without queries the oracle stands alone: held to a NumPy restatement of the contract
        assert np.array_equal(nb, brute_force_rows(c, nb.shape[1]))
