"""On the references alone (no GPU): the inputs of tests/mutation_cases.py can catch a stale structure at all.  For every (update,
map kind) the partners of the test scan change -- otherwise old content behind new pointers would pass --, the hash table size
stays for some kind and changes for another (a captured graph's key cannot change in the first case), every update does the
work it is named for, and no (update, kind, route) is set apart from the list the GPU test iterates.  These are conditions on
the inputs, met by the choice of clouds, poses and masks; none is a tolerance."""
import numpy as np
import pytest

import mutation_cases as mc
from route_tables import MUTATION_ROUTES

@pytest.fixture(scope="module", autouse=True)
def _oracle(oracle):
    return oracle


def _counts(dump):
    return {tuple(k): int(c) for k, c in zip(dump["vox_keys"].tolist(), dump["vox_count"].tolist())}


def _cap(kind):
    return 0 if mc.is_occ(kind) else mc.KINDS[kind]["max_points_per_voxel"]


@pytest.mark.parametrize("mutation,kind", mc.CASES)
def test_the_partners_change(mutation, kind):
    """at least a quarter of the 2000 points get another partner (another global index, or a partner appears or is lost), at
    least one in ten a partner from another voxel (no partner: no voxel).  The share of points that are paired before and
    after and change the voxel is printed too: 0.12 - 0.42 on the point-map kinds; on the occupancy maps 0.05, there the
    second scan's walls pair points that had no partner."""
    b, (a, _) = mc.before(kind), mc.after(mutation, kind)
    ib, vb = mc.partners(b)
    ia, va = mc.partners(a)
    assert len(ib) == mc.N_PARTNERS
    changed, moved = float((ib != ia).mean()), float((vb != va).any(1).mean())
    both = float(((ib >= 0) & (ia >= 0) & (vb != va).any(1)).mean())
    print("%s %s: partners changed %.3f, voxel of origin changed %.3f (paired before and after: %.3f), paired %d -> %d, table %d -> %d, "
          "points %d -> %d, voxels %d -> %d" % (mutation, kind, changed, moved, both, int((ib >= 0).sum()), int((ia >= 0).sum()), b.table,
                                                 a.table, b.om.num_points, a.om.num_points, b.om.num_voxels, a.om.num_voxels))
    assert changed >= 0.25 and moved >= 0.10
    assert (ia >= 0).sum() >= 1000   # and the updated map still pairs most of the scan: the alignments have something to hold


@pytest.mark.parametrize("mutation", list(mc.MUTATIONS))
def test_the_table_size_is_covered_both_ways(mutation):
    kinds = [k for mu, k in mc.CASES if mu == mutation]
    same = [k for k in kinds if mc.before(k).table == mc.after(mutation, k)[0].table]
    print("%s: table size kept by %s, changed by %s" % (mutation, same, [k for k in kinds if k not in same]))
    assert same and len(same) < len(kinds)


def test_table_size_rule():
    assert [mc.table_size(v) for v in (0, 1, 32, 33, 4096, 4097)] == [64, 64, 64, 128, 8192, 16384]


@pytest.mark.parametrize("mutation,kind", mc.CASES)
def test_the_update_does_its_own_work(mutation, kind):
    b, (a, facts) = mc.before(kind), mc.after(mutation, kind)
    cap = _cap(kind)
    db, da = b.om.dump(), a.om.dump()
    if not mc.is_occ(kind):
        assert len(db["xyz"]) >= 10000            # the map that is updated holds tens of thousands of points
    if kind == "uncapped":
        assert db["vox_count"].max() > 31
    if mc.is_ndt(kind):
        pb, pa = b.om.dump_ndt()["is_plane"], a.om.dump_ndt()["is_plane"]
        kb = {tuple(k) for k, p in zip(db["vox_keys"].tolist(), pb) if p}
        ka = {tuple(k) for k, p in zip(da["vox_keys"].tolist(), pa) if p}
        print("%s: planes %d -> %d, gained %d, lost %d" % (mutation, len(kb), len(ka), len(ka - kb), len(kb - ka)))
        assert len(kb) > 100 and (ka - kb or kb - ka)
    if mutation.startswith("insert_far"):
        cb, ca = _counts(db), _counts(da)
        assert set(cb) - set(ca)                   # voxels left
        if cap:
            assert any(c == cap and cb.get(k, 0) < cap for k, c in ca.items())   # a cap was met
    if mutation == "insert_frames":
        assert facts["passes"] >= 2 and len(mc.frames(kind)) == 3
        if cap:
            assert any(c == cap and _counts(db).get(k, 0) < cap for k, c in _counts(da).items())
    if mutation.startswith("erase"):
        mid, drop = facts["mid"], facts["drop"]
        dm = mid.om.dump()
        cm, ca = _counts(dm), _counts(da)
        assert set(cm) - set(ca)                   # a whole voxel went
        assert len(da["xyz"]) == len(dm["xyz"]) - int(drop.sum()) and 0 < drop.sum() < len(drop)
        if cap:
            assert any(c == cap and 0 < ca.get(k, 0) < cap for k, c in cm.items())   # a cap slot is free again
    if mutation == "erase_points":
        first, count = dm["vox_first"].astype(np.int64), dm["vox_count"].astype(np.int64)
        ends = [(drop[f], drop[f + c - 1], drop[f:f + c].all()) for f, c in zip(first, count) if c >= 3]
        assert any(x and y and not w for x, y, w in ends)   # the first and the last record of a voxel that stays
        assert drop[::3].all()                               # every third point
    if mutation == "erase_queued":
        # the insertion in front met the cap (or the clearance): the host's bound lies above the stored count
        if cap:
            assert facts["points_bound"] > facts["points_stored"]
        assert mid.om.num_voxels < mc._insert_bound(b.om.num_points, b.om.num_voxels, len(mc.keyframe()[0]))
    if mutation == "restore_over":
        d, n_offered = mc.other_map(kind)
        assert n_offered > len(d["xyz"]) and np.array_equal(da["xyz"], d["xyz"]) and np.array_equal(a.dump()["src_idx"], d["src_idx"])
    if mutation == "occmap_insert":
        assert b.cells - a.cells and a.cells - b.cells   # occupied cells left (far removal) and came


def test_no_case_is_set_apart():
    kinds = {mu: (list(mc.OCC_KINDS) if mu == "occmap_insert" else list(mc.KINDS)) for mu in mc.MUTATIONS}
    assert set(kinds) == {"build_again", "insert_far", "insert_far_full_sort", "insert_frames", "restore_over", "erase_points",
                          "erase_queued", "occmap_insert"}
    want = set()
    for mu, ks in kinds.items():
        for k in ks:
            for r in MUTATION_ROUTES:
                if r["maps"] == "any" or (r["maps"] == "ndt") == mc.is_ndt(k):
                    want.add((mu, k, r["name"]))
    assert set(mc.GPU_LIST) == want and len(mc.GPU_LIST) == len(want)
    # every row applies to some kind, and the families the table promises are there
    assert {r["name"] for r in MUTATION_ROUTES} == {n for _, _, n in mc.GPU_LIST}
    assert {r["family"] for r in MUTATION_ROUTES} == {"align", "query", "layers", "batch"}


@pytest.mark.parametrize("kind", list(mc.KINDS) + list(mc.OCC_KINDS))
def test_the_plane_routes_find_planes(kind):
    """the plane routes are not vacuous: the KNN + PCA search (point maps) and the NDT search accept pairings before the update"""
    ref = mc.before(kind)
    row = next(r for r in MUTATION_ROUTES if r["name"] == ("pt2pl" if mc.is_ndt(kind) else "pt2pl_knn"))
    n = len(mc.reference(ref, row)["local_idx"])
    print("%s: %d plane pairings" % (kind, n))
    assert n > 50
