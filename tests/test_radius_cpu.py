"""The radius search's reference (tests/radius_ref.py) on its own, for the inputs tests/test_gpu_radius.py uses: that they reach
what the kernel can get wrong (empty rows, rows longer than one and than four 64-record steps, rows that span voxel columns, exact
ties, d2 == r2, points on both sides of the predicate next to voxel planes), and that the brute force agrees with the oracle's
independent voxel-walking searches where the two are defined alike.  Plus the one check that needs the product: the symbol is
exported and bound."""
import numpy as np
import pytest

import radius_ref as rr
from oracle import oracle_c

F = np.float32


@pytest.fixture(scope="module")
def capped(oracle):
    m = oracle_c.Map(1.0, 20).insert(rr.capped_points())
    return m, m.dump()


@pytest.fixture(scope="module")
def capped_refs(capped):
    return {(r, s): rr.radius_search(capped[1], 1.0, rr.capped_queries(), rr.pose(), r, sorted=s) for r in rr.RADII for s in (False, True)}


@pytest.fixture(scope="module")
def boundary(oracle):
    d = oracle_c.Map(1.0, 0).insert(rr.boundary_points()).dump()
    return d, {r: rr.radius_search(d, 1.0, rr.boundary_queries(), rr.IDENTITY, r, sorted=True) for r in rr.BOUNDARY_RADII}


def test_the_cap_is_at_work_and_the_dump_is_in_voxel_order(capped):
    d = capped[1]
    assert len(d["xyz"]) < len(rr.capped_points()) and d["vox_count"].max() == 20
    k = d["vox_keys"].astype(np.int64)
    packed = (k[:, 0] << 42) + (k[:, 1] << 21) + k[:, 2]
    assert (np.diff(packed) > 0).all()


def test_rows_are_empty_long_and_longer(capped_refs):
    assert (capped_refs[(1e-3, False)].counts() == 0).all()
    c05, c25 = capped_refs[(0.5, False)].counts(), capped_refs[(2.5, False)].counts()
    assert (c05 == 0).any() and (c05 > 0).any()
    assert (c25 == 0).any() and (c25 > 64).any() and (c25 > 256).any()


def test_dense_rows_cross_the_step_sizes(oracle):
    d = oracle_c.Map(1.0, 0).insert(rr.dense_points()).dump()
    assert sorted(d["vox_count"].tolist()) == [300] * 5
    c = rr.radius_search(d, 1.0, rr.dense_queries(), rr.pose(), 1.0).counts()
    assert (c > 256).any() and (c == 0).any()


def test_rows_span_voxel_columns(capped, capped_refs):
    d, ref = capped[1], capped_refs[(1.0, False)]
    vox_of_pos = np.repeat(np.arange(len(d["vox_count"])), d["vox_count"])
    cols = d["vox_keys"][vox_of_pos][:, :2]
    spans = [len(np.unique(cols[ref.pos[ref.row(i)]], axis=0)) for i in range(len(ref.offsets) - 1)]
    assert max(spans) > 1
    # visit order is the order of the dump: every row's positions ascend
    assert all((np.diff(ref.pos[ref.row(i)]) > 0).all() for i in range(len(ref.offsets) - 1))


def test_boundary_points_fall_on_both_sides(boundary):
    d, refs = boundary
    pts, q = d["xyz"], rr.boundary_queries()
    for r in rr.BOUNDARY_RADII:
        ref, r2 = refs[r], rr.r2_of(r)
        seen_in = seen_out = seen_equal = 0
        for i in range(len(q)):
            dd = pts - q[i]
            d2 = (dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1]) + dd[:, 2] * dd[:, 2]
            near = np.abs(d2 - r2) < F(1e-6)  # one ulp to either side of the sphere, and on it
            seen_equal += int((d2 == r2).sum())
            seen_in += int((near & (d2 < r2)).sum())
            seen_out += int((near & (d2 > r2)).sum())
            assert not np.isin(np.flatnonzero(d2 == r2), ref.pos[ref.row(i)]).any()   # strict: d2 == r2 is out
        assert seen_in and seen_out and seen_equal, (r, seen_in, seen_out, seen_equal)


def test_exact_ties_occur_and_keep_storage_order(boundary):
    _, refs = boundary
    ref = refs[0.5]
    ties = 0
    for i in range(len(ref.offsets) - 1):
        d2, pos = ref.d2[ref.row(i)], ref.pos[ref.row(i)]
        assert (np.diff(d2) >= 0).all()
        eq = np.flatnonzero(np.diff(d2) == 0)
        ties += len(eq)
        assert (pos[eq + 1] > pos[eq]).all()
    assert ties >= 2  # the duplicates, and the two different points at one distance


@pytest.mark.parametrize("radius", [0.5, 1.0])
def test_first_sorted_result_is_the_oracle_s_nearest_neighbour(capped, capped_refs, radius):
    m, d = capped
    ref, p, r2 = capped_refs[(radius, True)], rr.transform(rr.capped_queries(), rr.pose()), rr.r2_of(radius)
    checked = 0
    for i in range(len(p)):
        ok, pt, d2, idx = m.nn_single(p[i])
        if ok and F(d2) < r2:
            a = int(ref.offsets[i])
            assert ref.offsets[i + 1] > a
            assert ref.d2[a] == F(d2) and (ref.xyz[a] == pt).all()
            checked += 1
    assert checked > 20


@pytest.mark.parametrize("radius", [0.5, 1.0])
def test_first_k_sorted_results_are_the_oracle_s_k_best(capped, capped_refs, radius):
    m, _ = capped
    ref, k = capped_refs[(radius, True)], 8
    o = oracle_c.match_points_k(m, rr.capped_queries(), rr.pose(), radius, k)
    take = np.concatenate([np.arange(ref.offsets[i], min(int(ref.offsets[i + 1]), int(ref.offsets[i]) + k))
                           for i in range(len(ref.offsets) - 1)]).astype(np.int64)
    local = np.repeat(np.arange(len(ref.offsets) - 1), np.minimum(ref.counts(), k))
    assert len(take) > 100
    assert np.array_equal(o["local_idx"], local)
    assert np.array_equal(o["global_idx"], ref.global_idx[take])
    assert np.array_equal(o["d2"].view(np.uint32), ref.d2[take].view(np.uint32))
    assert np.array_equal(o["global_xyz"].view(np.uint32), ref.xyz[take].view(np.uint32))


def test_radius_search_is_exported_and_bound():
    from mola_lidar_odometry_amd import capi
    assert hasattr(capi.lib(), "mh_nn_search_radius")
    assert callable(capi.nn_search_radius) and "mh_nn_search_radius" in capi._SIGNATURES
