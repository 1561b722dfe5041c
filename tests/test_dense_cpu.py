"""The inputs of tests/dense_cases.py prove their own regime, on the CPU and from the reference alone (oracle_c.Map.dump() and the
oracle's per-iteration poses): the occupancy classes of the maps, transformed points in every class at the first and the last
iteration, exact fp32 ties on the lattice map, no case set apart by tools/fuzz_layers.py's rule (allowed share: zero), partners
that change and leave their block.  tests/test_gpu_dense_cells.py holds the device to the same references."""
import numpy as np
import pytest

import dense_cases as dc
from oracle import layers_oracle, oracle_c


@pytest.fixture(scope="module")
def inp(oracle):
    return dc.Inputs()


@pytest.fixture(scope="module")
def omaps(inp):
    return inp.omaps()


@pytest.fixture(scope="module")
def dumps(omaps):
    return {k: m.dump() for k, m in omaps.items()}


@pytest.fixture(scope="module")
def singles(inp, omaps):
    """(map, n, iterations) -> oracle_c.icp_align's result with pairs: the 16-iteration singles and the launch chain's cases"""
    keys = [(mk, n, dc.SINGLE_IT) for mk in ("room", "mixed") for n in dc.SIZES + [dc.N_SCAN]]
    keys += [("room", n, n_it) for n, n_it in dc.CHAIN_CASES if ("room", n, n_it) not in keys]
    return {(mk, n, n_it): oracle_c.icp_align(omaps[mk], dc.single_scan(inp, n), inp.T0, dc.single_params(oracle_c, n_it),
                                              prior=dc.single_prior(inp, n), want_pairs=True) for mk, n, n_it in keys}


@pytest.fixture(scope="module")
def refs(inp, omaps):
    return {name: (c, dc.case_reference(c, omaps)) for name, c in dc.cases(inp).items()}


# ------------------------------------------------------------------------------------------------------ occupancy classes
def test_occupancy_classes(dumps):
    for k, d in dumps.items():
        c = dc.occupancy(d)
        print("%-10s %6d points, %4d voxels, median %5d, > 31: %3d, <= 31: %3d, > 768: %3d, > 8192: %d, max %d" % (
            k, len(d["xyz"]), len(c), int(np.median(c)), int((c > 31).sum()), int((c <= 31).sum()), int((c > 768).sum()),
            int((c > 8192).sum()), int(c.max())))
    c = dc.occupancy(dumps["room"])
    assert (c > 31).sum() >= 100 and (c > 768).sum() >= 20 and (c > 8192).sum() == 1
    assert tuple(dumps["room"]["vox_keys"][int(np.argmax(c))]) == dc.TOWER
    # mixed: blocks of 27 voxels that hold indexed voxels (quadrant boundaries: at most 31 records) beside un-indexed ones
    d = dumps["mixed"]
    table = {tuple(k): int(n) for k, n in zip(d["vox_keys"].tolist(), dc.occupancy(d).tolist())}
    both = 0
    for key in table:
        ns = [table.get((key[0] + a, key[1] + b, key[2] + e)) for a in (-1, 0, 1) for b in (-1, 0, 1) for e in (-1, 0, 1)]
        ns = [n for n in ns if n]
        both += any(n <= 31 for n in ns) and any(n > 31 for n in ns)
    print("mixed: %d of %d blocks hold both classes" % (both, len(table)))
    assert both >= 20
    assert dc.occupancy(dumps["centres"]).min() > 31 and dc.occupancy(dumps["capped"]).max() <= 20


# ------------------------------------------------------------------------------------------- transformed points per regime
def _spread(mask):
    """at least 64 points of the class, not all in one aligned run of 64, and an aligned run that holds both kinds"""
    idx = np.flatnonzero(mask)
    runs = np.unique(idx // 64)
    mixed_run = any(0 < mask[r * 64:(r + 1) * 64].sum() < len(mask[r * 64:(r + 1) * 64]) for r in runs)
    return len(idx) >= 64 and len(runs) > 1 and mixed_run


def test_transformed_points_fall_in_every_regime(inp, dumps, singles):
    for mk in ("room", "mixed"):
        o = singles[(mk, 2000, dc.SINGLE_IT)]
        for which, T in (("first", inp.T0), ("last", o["trace"][-2]["T"])):  # the poses iteration 0 and the last one match at
            n = dc.own_voxel_count(dumps[mk], dc.transform(dc.single_scan(inp, 2000), T))
            classes = {"tower": n > 8192, "32-700": (n >= 32) & (n <= 700)}
            if mk == "mixed":
                classes["indexed"] = (n > 0) & (n <= 31)
            for name, mask in classes.items():
                print("%-6s %-5s iteration: %4d points in %s" % (mk, which, int(mask.sum()), name))
                assert _spread(mask), (mk, which, name)


# --------------------------------------------------------------------------------------------------------- ties on centres
def test_centres_queries_tie_exactly(inp, dumps):
    d = dumps["centres"]
    best = dc.brute_force_k(d, inp.queries, 4, 1e3)
    two = sum(1 for b in best if len(b) >= 2 and b[0][1] == b[1][1])
    four = sum(1 for b in best if len(b) >= 4 and b[0][1] == b[3][1])
    keys = dc.voxel_keys(d["xyz"])
    qk = dc.voxel_keys(inp.queries)
    across = sum(1 for b, k in zip(best, qk.tolist()) if len(b) >= 2 and b[0][1] == b[1][1] and
                 (keys[b[0][0]].tolist() != k or keys[b[1][0]].tolist() != k))
    print("centres: %d of %d queries tie in their two smallest d2, %d in four, %d across a voxel face" % (two, len(best), four, across))
    assert two >= 200 and four >= 50 and across >= 10
    # ... and the C oracle breaks them as the brute force does: by record index
    o = oracle_c.match_points(omap_of(inp, "centres"), inp.queries, dc.IDENTITY, 1e3)
    assert len(o["local_idx"]) == len(best)
    assert d["src_idx"][[b[0][0] for b in best]].tolist() == o["global_idx"].tolist()  # (global_idx: the record's source index)
    np.testing.assert_array_equal(np.array([b[0][1] for b in best], np.float32), o["d2"])


def test_plane_search_chooses_among_tied_records(inp, dumps):
    """the plane cases of the GPU file's tie section: queries the oracle accepts whose k-th and (k+1)-th nearest records tie
    exactly, so that the centroid shows which of them the search chose"""
    om = omap_of(inp, "centres")
    for knn, eig in dc.TIE_PLANES:
        o = oracle_c.match_pt2pl_knn(om, inp.queries, dc.IDENTITY, 0.4, eig, dc.TIE_PLANE_RADIUS, knn, dc.TIE_PLANE_MIN_POINTS)
        best = dc.brute_force_k(dumps["centres"], inp.queries, knn, dc.TIE_PLANE_RADIUS)
        tied = sum(1 for i in o["local_idx"] if len(best[i]) == knn and
                   best[i][-1][1] == dc.next_d2(dumps["centres"], inp.queries[i], best[i]))
        print("knn %d, eigenvalue threshold %g: %d accepted, %d of them choose their k-th record among tied ones" % (
            knn, eig, len(o["local_idx"]), tied))
        assert len(o["local_idx"]) > 800 and tied >= 100


def omap_of(inp, key):
    return inp.omaps([key])[key]


# -------------------------------------------------------------------------------------------------------- nothing set apart
def test_no_case_is_set_apart(inp, omaps, singles, refs):
    """tools/fuzz_layers.py's rule, read from the oracle alone.  oracle_c.icp_align records no margins: the single pairs run once
    more through layers_oracle (same matcher, float64 numpy solve), which does."""
    apart, total = [], 0
    for (mk, n, n_it), o in singles.items():
        p = dc.single_params(oracle_c, n_it)
        lo = layers_oracle.icp_align_layers([dict(map=omaps[mk], local=dc.single_scan(inp, n), threshold=p.threshold)], inp.T0, p,
                                            prior=dc.single_prior(inp, n))
        assert lo["n_iterations"] == o["n_iterations"] and [t["n_pairs"] for t in lo["trace"]] == [t["n_pairs"] for t in o["trace"]]
        assert np.abs(lo["T"] - o["T"]).max() < 1e-9
        near = layers_oracle.nearest_decision(lo["margins"])
        print("single %-6s n %4d, %2d iterations: max cond %.2e, nearest decision %s, final pairs %d" % (
            mk, n, n_it, lo["max_cond"], near, o["n_final_pairs"]))
        total += 1
        if dc.set_apart(lo):
            apart.append((mk, n, n_it))
        assert o["n_final_pairs"] > 0
    for name, (c, o) in refs.items():
        near = layers_oracle.nearest_decision(o["margins"])
        print("%-14s iterations %2d, final pairs %5d of %5d, counts %s, max cond %.2e, nearest decision %s" % (
            name, o["n_iterations"], o["n_final_pairs"], o["potential_pairings"], o["pair_counts"], o["max_cond"], near))
        total += 1
        if dc.set_apart(o):
            apart.append(name)
        assert o["n_final_pairs"] > 0, name
    print("%d of %d cases set apart" % (len(apart), total))
    assert not apart, apart


# ----------------------------------------------------------------------------------------- partners change and leave blocks
def test_partners_change_between_iterations(inp, omaps, singles):
    for (mk, n, n_it), o in singles.items():
        if n < 63 or n_it != dc.SINGLE_IT:
            continue
        scan, thr = dc.single_scan(inp, n), dc.schedule(dc.SINGLE_IT)
        poses = [inp.T0] + [t["T"] for t in o["trace"]]
        changed = 0
        prev = None
        for j in range(4):
            m = oracle_c.match_points(omaps[mk], scan, poses[j], float(thr[j]))
            cur = dict(zip(m["local_idx"].tolist(), m["global_idx"].tolist()))
            if prev is not None:
                changed += sum(1 for i, g in cur.items() if i in prev and prev[i] != g)
            prev = cur
        print("single %-6s n %4d: %d partner changes over iterations 1-3" % (mk, n, changed))
        assert changed > 0, (mk, n)


def test_previous_partners_leave_the_block(refs, omaps):
    """dense_cases.partners_that_left on a k-best pair and on the plane pairs (k = knn inside the search radius): previous
    partners leave the block, and points they leave still fill all k slots.  (Not rgbd.yaml's plane parameters: inside a radius
    of 0.8 voxels no partner can lie two voxel indices away.)"""
    for name, i in (("k2", 0), ("k8", 0), ("knn16", 0)):
        c, o = refs[name]
        e = c["pairs"][i]
        poses = ([np.asarray(c["T0"], np.float64)] + [t["T"] for t in o["trace"]])[:c["max_it"]]
        if e["plane"]:
            k, thr = e["plane"]["knn"], np.full(c["max_it"], e["plane"]["search_radius"])
        else:
            k, thr = e["k"], np.broadcast_to(e["threshold"], (c["max_it"],))
        left = dc.partners_that_left(omaps[e["map"]], e["local"], poses, thr, k)
        print("%-6s pair %d, k %2d: (points a previous partner of which left the block, of them with k pairings) per iteration %s" % (
            name, i, k, left))
        assert sum(a for a, b in left) > 0 and sum(b for a, b in left) > 0, name


def test_each_case_has_its_property(refs, inp, dumps):
    c, o = refs["gated"]  # the gated pair's first active iteration is 2
    assert o["potential_pairings"] == 700 * 2 + 1300 and (0, 0) in o["accepted"] and len(o["accepted"][(0, 1)]) == 0
    assert len(o["accepted"][(0, 2)]) > 700
    c, o = refs["unique"]  # claims are lost: fewer kept than accepted
    assert sum(len(v) for v in o["kept"].values()) < sum(len(v) for v in o["accepted"].values())
    c, o = refs["k8"]
    assert o["n_final_pairs"] > 4 * 600
    c, o = refs["rgbd"]
    assert o["n_final_pairs_pt2pl"] > 300 and o["potential_pairings"] == 1000 * 2 + 1000
    c, o = refs["knn16"]  # points whose radius takes in the tower: more than 2048 chunks of 4 records for one point
    e = c["pairs"][0]
    world = dc.transform(e["local"], o["poses"][-1]).astype(np.float64)
    lo, hi = np.asarray(dc.TOWER, np.float64), np.asarray(dc.TOWER, np.float64) + 1.0
    gap = np.linalg.norm(np.maximum(0.0, np.maximum(lo - world, world - hi)), axis=1)
    n = int(np.sum(gap < e["plane"]["search_radius"]))
    print("knn16: %d of %d points have the tower inside their radius" % (n, len(world)))
    assert n >= 64 and dc.occupancy(dumps["room"]).max() > 4 * 2048
