"""Every ICP search route on uncapped dense-voxel maps (max_points_per_voxel = 0, hundreds to thousands of records per voxel: what
mh_occmap_search_map and SparseTreesPointCloud hand to the alignments of lidar2d.yaml and rgbd.yaml), held to the oracle.

The inputs and cases are tests/dense_cases.py's; tests/test_dense_cpu.py shows on the reference alone that they cross the fixed
limits of the searches (no quadrant boundaries above 31 records, 768 / 1024 / 2048 chunks per wave, 8 / 27 candidate voxels, k
result slots, previous partners that leave the block) and that none is set apart.  Bars are the project's: per-iteration pair
counts, final local_idx / global_idx / d2 / global_xyz, termination iteration and reason bit for bit; single-pair poses within
1e-9 of oracle_c; multi-layer results through layers_oracle.compare.

A one-launch loop gives up after 20 ms and arms a hold-off of hundreds of alignments, which would change the kernels that LATER
test files run: every case here that lets a loop run asserts that it started and was not abandoned, and is sized from the
measured loop times of profiles/dense_cells.md; every other single-pair case names its kernel family by a switch, under which
no loop starts."""
import numpy as np
import pytest

import dense_cases as dc
import kbest_ref
from mola_lidar_odometry_amd import capi
from oracle import layers_oracle, oracle_c
from route_tables import FAMILIES, LOOP16_CASES, LOOPW_CASES, MULTI, SEARCH, env_id

pytestmark = pytest.mark.gpu

PAIR_KEYS = ("local_idx", "global_idx", "d2", "global_xyz")


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def inp(oracle):
    return dc.Inputs()


@pytest.fixture(scope="module")
def omaps(inp):
    return inp.omaps()


@pytest.fixture(scope="module")
def dmaps(ctx, inp):
    return inp.dmaps(ctx)


@pytest.fixture(scope="module")
def all_cases(inp):
    return dc.cases(inp)


class _Once:
    """references computed once per module, on first use, and left unchanged"""

    def __init__(self, make):
        self.make, self.done = make, {}

    def __getitem__(self, key):
        if key not in self.done:
            self.done[key] = self.make(key)
        return self.done[key]


@pytest.fixture(scope="module")
def single_refs(inp, omaps):
    """(map, n, iterations) -> oracle_c.icp_align with pairs"""
    return _Once(lambda k: oracle_c.icp_align(omaps[k[0]], dc.single_scan(inp, k[1]), inp.T0, dc.single_params(oracle_c, k[2]),
                                              prior=dc.single_prior(inp, k[1]), want_pairs=True))


@pytest.fixture(scope="module")
def refs(all_cases, omaps):
    return _Once(lambda name: dc.case_reference(all_cases[name], omaps))


def _single(dmaps, scan, inp, mk, n, n_it=dc.SINGLE_IT):
    return capi.icp_align(dmaps[mk], scan, inp.T0, dc.single_params(capi, n_it), prior=dc.single_prior(inp, n), want_pairs=True)


def _assert_single_is_the_oracles(g, o, what):
    dT = float(np.abs(np.asarray(g["T"]) - o["T"]).max())
    print("%s: iterations %d / %d, final pairs %d / %d, max |dT| %.2e" % (what, g["n_iterations"], o["n_iterations"],
                                                                          g["n_final_pairs"], o["n_final_pairs"], dT))
    assert g["n_iterations"] == o["n_iterations"] and g["termination_reason"] == o["termination_reason"], what
    assert [t["n_pairs"] for t in g["trace"]] == [t["n_pairs"] for t in o["trace"]], what
    for k in PAIR_KEYS:
        np.testing.assert_array_equal(g["pairs"][k], o["pairs"][k], err_msg="%s: %s" % (what, k))
    np.testing.assert_allclose(g["T"], o["T"], rtol=0, atol=1e-9, err_msg=what)


def _assert_same_bits(a, b, what):
    assert a["n_iterations"] == b["n_iterations"] and a["termination_reason"] == b["termination_reason"], what
    assert a["n_final_pairs"] == b["n_final_pairs"], what
    for k in ("T", "cov"):
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), (what, k)
    if "trace" in a and "trace" in b:
        assert [t["n_pairs"] for t in a["trace"]] == [t["n_pairs"] for t in b["trace"]], what
        for x, y in zip(a["trace"], b["trace"]):
            assert np.asarray(x["T"]).tobytes() == np.asarray(y["T"]).tobytes(), what
    if "pairs" in a and "pairs" in b and isinstance(a["pairs"], dict):
        for k in PAIR_KEYS:
            assert a["pairs"][k].tobytes() == b["pairs"][k].tobytes(), (what, k)


# ------------------------------------------------------------------- a. single pair, every shipped family, room and mixed
# FAMILIES x SEARCH: tests/route_tables.py (test_gpu_parity.py::test_every_kernel_variant_matches_the_oracle's list, plus the
# default route's launch chain; the one-launch loops: section b).  No loop starts under these
# switches, except under MH_MATCH=s alone: the row search's loop k_icp16.
_id = env_id


@pytest.mark.parametrize("search", SEARCH, ids=_id)
@pytest.mark.parametrize("family", FAMILIES, ids=_id)
@pytest.mark.parametrize("mk", ["room", "mixed"])
def test_single_pair_every_family(ctx, inp, dmaps, single_refs, mk, family, search, monkeypatch):
    for k, v in {**family, **search}.items():
        monkeypatch.setenv(k, v)
    s0, a0 = capi.loop_stats()
    g = _single(dmaps, capi.Scan(ctx, dc.single_scan(inp, 2000)), inp, mk, 2000)
    assert capi.loop_stats() == (s0 + (1 if family == {"MH_MATCH": "s"} else 0), a0)  # the one loop started and was not abandoned
    _assert_single_is_the_oracles(g, single_refs[(mk, 2000, dc.SINGLE_IT)], "%s %s %s" % (mk, _id(family), _id(search)))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
@pytest.mark.parametrize("match", ["f", "s"])
@pytest.mark.parametrize("mk", ["room", "mixed"])
def test_single_pair_small_layers(ctx, inp, dmaps, single_refs, mk, match, n, monkeypatch):
    monkeypatch.setenv("MH_MATCH", match)
    s0, a0 = capi.loop_stats()
    g = _single(dmaps, capi.Scan(ctx, dc.single_scan(inp, n)), inp, mk, n)
    assert capi.loop_stats() == (s0 + (1 if match == "s" else 0), a0)  # (s: k_icp16, a few groups of 32 points; not abandoned)
    _assert_single_is_the_oracles(g, single_refs[(mk, n, dc.SINGLE_IT)], "%s MH_MATCH=%s n %d" % (mk, match, n))


# --------------------------------------------------------------- b. the launch chain against the one-launch loops
# LOOP16_CASES, LOOPW_CASES: tests/route_tables.py, sized from the measured loop times of profiles/dense_cells.md
CHAIN_CASES = dc.CHAIN_CASES  # (their references pass the set-apart rule in tests/test_dense_cpu.py like every other)


@pytest.mark.parametrize("n,n_it", CHAIN_CASES)
def test_the_chain_is_the_oracles(ctx, inp, dmaps, single_refs, n, n_it, monkeypatch):
    monkeypatch.setenv("MH_NO_LOOP16", "1")
    s0 = capi.loop_stats()
    g = _single(dmaps, capi.Scan(ctx, dc.single_scan(inp, n)), inp, "room", n, n_it)
    assert capi.loop_stats() == s0
    _assert_single_is_the_oracles(g, single_refs[("room", n, n_it)], "chain n %d" % n)


def _loop_against_chain(ctx, inp, dmaps, n, n_it, monkeypatch, what):
    scan = capi.Scan(ctx, dc.single_scan(inp, n))
    s0, a0 = capi.loop_stats()
    loop = _single(dmaps, scan, inp, "room", n, n_it)
    s1, a1 = capi.loop_stats()
    assert s1 - s0 == 1 and a1 == a0, "%s: the loop started %d times, abandoned %d" % (what, s1 - s0, a1 - a0)
    monkeypatch.setenv("MH_NO_LOOP16", "1")
    chain = _single(dmaps, scan, inp, "room", n, n_it)
    assert capi.loop_stats() == (s1, a1)
    _assert_same_bits(loop, chain, what)


@pytest.mark.parametrize("n,n_it", LOOP16_CASES)
def test_k_icp16_gives_the_bits_of_the_chain(ctx, inp, dmaps, n, n_it, monkeypatch):
    _loop_against_chain(ctx, inp, dmaps, n, n_it, monkeypatch, "k_icp16 n %d" % n)


@pytest.mark.parametrize("n,n_it", LOOPW_CASES)
def test_k_icpw_gives_the_bits_of_the_chain(ctx, inp, dmaps, n, n_it, monkeypatch):
    monkeypatch.setenv("MH_LOOPW", "all")
    _loop_against_chain(ctx, inp, dmaps, n, n_it, monkeypatch, "k_icpw n %d" % n)


def test_lockstep_batch_of_loops_gives_the_bits_of_the_chain(ctx, inp, dmaps, monkeypatch):
    """three layers on contexts of their own, one map: k_icpw_b side by side"""
    sizes, n_it = [n for n, _ in LOOPW_CASES], min(it for _, it in LOOPW_CASES)
    p = dc.single_params(capi, n_it)
    ctxs = [capi.Context(0) for _ in sizes]
    try:
        scans = [capi.Scan(c, dc.single_scan(inp, n)) for c, n in zip(ctxs, sizes)]
        guesses = [inp.T0, inp.T1, inp.T0]
        s0, a0 = capi.loop_stats()
        batch = capi.icp_align_batch([dmaps["room"]] * 3, scans, guesses, p)
        s1, a1 = capi.loop_stats()
        assert s1 - s0 == 3 and a1 == a0, "the batch started %d loops, abandoned %d" % (s1 - s0, a1 - a0)
        monkeypatch.setenv("MH_NO_LOOP16", "1")
        for n, T, b in zip(sizes, guesses, batch):
            chain = capi.icp_align(dmaps["room"], capi.Scan(ctx, dc.single_scan(inp, n)), T, p, want_trace=False)
            _assert_same_bits(b, chain, "batch job n %d" % n)
        assert capi.loop_stats() == (s1, a1)
    finally:
        for c in ctxs:
            c.close()


# ------------------------------------------------------------------------------------------------ c. multi-layer on room
def _device(ctx, dmaps, c, T0=None, **kw):
    pairs, ks = dc.device_pairs(c, dmaps, lambda a: capi.Scan(ctx, a))
    return capi.icp_align_layers(pairs, c["T0"] if T0 is None else T0, dc.device_params(c), prior=c["prior"], want_pairs=True,
                                 pairings_per_point=ks, **kw)


def _compare_pairs(c, r, o):
    """point pairs bit for bit; plane pairs: the index set exactly, centroid and normal to test_gpu_parity.py's plane tolerance"""
    bad = []
    for i, (e, x, y) in enumerate(zip(c["pairs"], r["pairs"], o["pairs"])):
        if e["plane"]:
            if not np.array_equal(x["local_idx"], y["local_idx"]):
                bad.append("plane pair %d: index sets differ" % i)
                continue
            for key in ("centroid", "normal"):
                if not np.allclose(x[key], y[key], rtol=0.0, atol=1e-6):
                    bad.append("plane pair %d: %s max |d| %.3e" % (i, key, float(np.abs(x[key] - y[key]).max())))
        else:
            for key in PAIR_KEYS:
                if not np.array_equal(x[key], y[key]):
                    bad.append("pair %d: %d %s values differ" % (i, int(np.sum(x[key] != y[key])), key))
    return bad


def _check(r, c, o, what):
    dT = float(np.abs(np.asarray(r["T"]) - o["T"]).max())
    print("%s: iterations %d / %d, final pairs %d / %d, counts %s / %s, max |dT| %.2e" % (
        what, r["n_iterations"], o["n_iterations"], r["n_final_pairs"], o["n_final_pairs"], r["pair_counts"], o["pair_counts"], dT))
    diffs = layers_oracle.compare(r, o, with_pairs=False)
    if "n_final_pairs_pt2pl" in o and r["n_final_pairs_pt2pl"] != o["n_final_pairs_pt2pl"]:
        diffs.append("n_final_pairs_pt2pl %d vs %d" % (r["n_final_pairs_pt2pl"], o["n_final_pairs_pt2pl"]))
    if r["pair_counts"] == o["pair_counts"]:
        diffs += _compare_pairs(c, r, o)
    assert not diffs, (what, diffs)


@pytest.mark.parametrize("name", MULTI)
def test_multi_layer_matches_the_reference(ctx, dmaps, all_cases, refs, name):
    o = refs[name]
    assert not dc.set_apart(o) and o["n_final_pairs"] > 0
    _check(_device(ctx, dmaps, all_cases[name]), all_cases[name], o, name)


RESULT_KEYS = ("n_iterations", "termination_reason", "n_final_pairs", "n_final_pairs_pt2pl", "potential_pairings", "quality",
               "pair_counts")


@pytest.fixture(scope="module")
def three(inp):
    """three contexts with the dense map each, for the lock-step batches"""
    ctxs = [capi.Context(0) for _ in range(3)]
    maps = [inp.dmaps(c, ["room"]) for c in ctxs]
    yield ctxs, maps
    for c in ctxs:
        c.close()


@pytest.mark.parametrize("name", ["two_pairs", "k2", "unique", "gated", "rgbd"])
def test_lockstep_batch_gives_the_bits_of_the_single_calls(inp, three, all_cases, name):
    ctxs, maps = three
    c = all_cases[name]
    guesses = [inp.T0, inp.T1, inp.T_gt]
    p = dc.device_params(c)
    jobs, kpp, solo = [], [], []
    for cx, dm, T in zip(ctxs, maps, guesses):
        pairs, ks = dc.device_pairs(c, dm, lambda a, cx=cx: capi.Scan(cx, a))
        jobs.append(pairs)
        kpp.append(ks)
        solo.append(capi.icp_align_layers(pairs, T, p, want_trace=False, pairings_per_point=ks))
    got = capi.icp_align_layers_batch(jobs, guesses, p, pairings_per_point=kpp, planes_entry=True)
    for j, (r, s) in enumerate(zip(got, solo)):
        assert s["n_final_pairs"] > 0
        for k in ("T", "cov"):
            assert np.asarray(r[k]).tobytes() == np.asarray(s[k]).tobytes(), (name, j, k)
        for k in RESULT_KEYS:
            assert r[k] == s[k], (name, j, k)


# ----------------------------------------------------------------------------------- d. bound and graph independence
@pytest.mark.parametrize("name", ["k2", "rgbd"])
def test_bitwise_equal_with_and_without_bound_and_graphs(ctx, dmaps, all_cases, name, monkeypatch):
    c = all_cases[name]
    runs = [_device(ctx, dmaps, c)]
    for var in ("MH_NO_PREV_BOUND", "MH_NO_GRAPH"):
        monkeypatch.setenv(var, "1")
        runs.append(_device(ctx, dmaps, c))
        monkeypatch.delenv(var)
    runs.append(_device(ctx, dmaps, c))
    assert runs[0]["n_iterations"] >= 10 and runs[0]["n_final_pairs"] > 2000
    for other in runs[1:]:
        for key in ("T", "cov"):
            assert np.asarray(other[key]).tobytes() == np.asarray(runs[0][key]).tobytes(), key
        assert other["pair_counts"] == runs[0]["pair_counts"]
        assert [t["n_pairs"] for t in other["trace"]] == [t["n_pairs"] for t in runs[0]["trace"]]
        for a, b in zip(other["pairs"], runs[0]["pairs"]):
            for key in a:
                assert a[key].tobytes() == b[key].tobytes(), key


# ------------------------------------------------------------------------------------------------------- e. exact ties
TIE_THR = 0.2


@pytest.fixture(scope="module")
def brute(inp, omaps):
    """k -> (local_idx, global_idx, d2) of the numpy brute force over the 27-voxel block, ties by record index"""
    d = omaps["centres"].dump()

    def make(k):
        best = dc.brute_force_k(d, inp.queries, k, TIE_THR)
        li = np.array([i for i, b in enumerate(best) for _ in b], np.uint32)
        gi = np.array([d["src_idx"][r] for b in best for r, _ in b], np.uint32)
        d2 = np.array([v for b in best for _, v in b], np.float32)
        return li, gi, d2
    return _Once(make)


def _assert_is(got, want, what):
    for key, w in zip(("local_idx", "global_idx", "d2"), want):
        np.testing.assert_array_equal(got[key], w, err_msg="%s: %s" % (what, key))


def test_ties_nn_search(ctx, inp, omaps, dmaps, brute):
    scan = capi.Scan(ctx, inp.queries)
    g = capi.nn_search(dmaps["centres"], scan, dc.IDENTITY, TIE_THR)
    o = oracle_c.match_points(omaps["centres"], inp.queries, dc.IDENTITY, TIE_THR)
    assert len(o["local_idx"]) == len(inp.queries)
    _assert_is(g, (o["local_idx"], o["global_idx"], o["d2"]), "oracle")
    _assert_is(g, brute[1], "brute force")
    np.testing.assert_array_equal(g["global_xyz"], o["global_xyz"])


@pytest.mark.parametrize("k", [2, 8])
def test_ties_nn_search_k(ctx, inp, omaps, dmaps, brute, k):
    g = capi.nn_search_k(dmaps["centres"], capi.Scan(ctx, inp.queries), dc.IDENTITY, TIE_THR, k)
    o = oracle_c.match_points_k(omaps["centres"], inp.queries, dc.IDENTITY, TIE_THR, k)
    assert len(o["local_idx"]) > 1.5 * len(inp.queries)
    _assert_is(g, (o["local_idx"], o["global_idx"], o["d2"]), "oracle")
    _assert_is(g, brute[k], "brute force")
    np.testing.assert_array_equal(g["global_xyz"], o["global_xyz"])


PLANE_RADIUS, PLANE_MIN_POINTS = dc.TIE_PLANE_RADIUS, dc.TIE_PLANE_MIN_POINTS


@pytest.mark.parametrize("knn,eig", dc.TIE_PLANES)
def test_ties_nn_search_pt2pl_knn(ctx, inp, omaps, dmaps, knn, eig):
    """The k nearest of a lattice query are chosen among tied records: the centroid shows which.  (rgbd.yaml's eigenvalue
    threshold 1e-2 accepts no plane on a contour two cells deep: the two thresholds here accept 1360 and 1910 of the 2000 queries.)
    Against the C oracle, and against the numpy brute force over the 27-voxel block that breaks ties by record index: the knn
    records it chooses inside the radius are at least minimum_plane_points for every accepted query, fewer for no accepted one,
    and their float64 mean is the centroid.  (The eigenvalue and plane-distance tests, which decide the rest of the accepted set,
    and the normal have no second restatement: those are the oracle's.)"""
    args = (0.4, eig, PLANE_RADIUS, knn, PLANE_MIN_POINTS)
    g = capi.nn_search_pt2pl_knn(dmaps["centres"], capi.Scan(ctx, inp.queries), dc.IDENTITY, *args)
    o = oracle_c.match_pt2pl_knn(omaps["centres"], inp.queries, dc.IDENTITY, *args)
    print("plane pairings on the lattice: %d / %d" % (len(g["local_idx"]), len(o["local_idx"])))
    assert len(o["local_idx"]) > 800
    np.testing.assert_array_equal(g["local_idx"], o["local_idx"])
    for key in ("centroid", "normal"):  # the tolerance of test_gpu_parity.py's plane test
        np.testing.assert_allclose(g[key], o[key], rtol=0.0, atol=1e-6)
    d = omaps["centres"].dump()
    best = dc.brute_force_k(d, inp.queries, knn, PLANE_RADIUS)
    enough = np.array([len(b) >= PLANE_MIN_POINTS for b in best])
    assert enough[g["local_idx"]].all() and 0 < int(enough.sum()) <= len(best)
    xyz = d["xyz"].astype(np.float64)
    mean = np.array([xyz[[r for r, _ in best[i]]].mean(0) for i in g["local_idx"]])
    print("brute force: largest |centroid - mean| %.2e" % float(np.abs(g["centroid"] - mean).max()))
    # (tests/test_dense_cpu.py: more than a hundred of the accepted queries choose their k-th record among exactly tied ones)
    np.testing.assert_allclose(g["centroid"], mean, rtol=0.0, atol=1e-6)


@pytest.mark.parametrize("k", [1, 2])
def test_ties_one_iteration_is_the_search(ctx, inp, omaps, dmaps, brute, k):
    scan = capi.Scan(ctx, inp.queries)
    p = capi.ICPParams(max_iterations=1, kernel_param=0.5, threshold=1.0, gn=capi.GNParams(max_inner_iterations=1))
    r = capi.icp_align_layers([dict(map=dmaps["centres"], scan=scan, threshold=TIE_THR)], dc.IDENTITY, p, want_pairs=True,
                              pairings_per_point=k if k > 1 else None)
    o = oracle_c.match_points_k(omaps["centres"], inp.queries, dc.IDENTITY, TIE_THR, k)
    assert r["n_final_pairs"] == len(o["local_idx"]) and r["potential_pairings"] == len(inp.queries) * k
    _assert_is(r["pairs"][0], (o["local_idx"], o["global_idx"], o["d2"]), "oracle")
    _assert_is(r["pairs"][0], brute[k], "brute force")


# ------------------------------------------------------------------------------ f. the maps the pipelines really hand out
def _contour_scan(T, step, rng, noise=0.0):
    """the wall contour of the 6 x 5 m room at z = 0.3 as a 2-D scan in the sensor frame of T"""
    u = np.arange(0.0, 6.0, step)
    v = np.arange(0.0, 5.0, step)
    z = lambda a: np.full_like(a, 0.3)
    w = np.concatenate([np.stack([u, np.zeros_like(u), z(u)], 1), np.stack([u, np.full_like(u, 5.0), z(u)], 1),
                        np.stack([np.zeros_like(v), v, z(v)], 1), np.stack([np.full_like(v, 6.0), v, z(v)], 1)])
    return dc.pull_back(w, T, rng, noise)


def test_occupancy_search_map_alignment_matches_the_reference(ctx, oracle):
    """Two 2-D scans of the room contour in an occupancy map whose search voxel has grown to 1.0; the centres, downloaded in the
    search map's order, make an oracle map, and the k = 2 alignment on search_map() is held to the float64 reference."""
    rng = np.random.default_rng(4104)
    occ = capi.OccMap(ctx, resolution=0.02)
    for T, step in ((dc.pose(3.0, 2.5, 0.3, 0.0), 0.007), (dc.pose(2.2, 1.9, 0.3, 0.4), 0.009)):
        s = capi.Scan(ctx, _contour_scan(T, step, rng))
        occ.insert(s, T)
        s.close()
    dm = occ.search_map(1.0)
    V = occ.info().search_voxel_size
    assert V == 1.0
    d = dm.download()
    order = np.argsort(d["src_idx"], kind="stable")
    assert np.array_equal(d["src_idx"][order], np.arange(len(order), dtype=np.uint32))
    cen = np.ascontiguousarray(d["xyz"][order])
    om = oracle_c.Map(V, 0).insert(cen)
    occupancy = dc.occupancy(om.dump())
    print("occupancy map: %d centres in %d search voxels, median %d, max %d records" % (
        len(cen), len(occupancy), int(np.median(occupancy)), int(occupancy.max())))
    assert len(cen) > 400 and np.median(occupancy) > 31
    T_gt = dc.pose(2.6, 2.1, 0.3, 0.2)
    local = _contour_scan(T_gt, 0.029, rng, 0.01)
    T0 = dc.pose(2.67, 2.05, 0.32, 0.2 + np.deg2rad(1.0), np.deg2rad(0.3))
    c = dict(max_it=12, kp=np.full(12, 0.3), inner=2, pkw=dict(disable_stall_test=True))
    thr = dc.schedule(12, 0.8, 0.3)
    o = kbest_ref.reference([dict(map=om, local=local, threshold=thr, threshold_angular_deg=0.0, weight=1.0)], [2], T0,
                            kbest_ref.oracle_params(c))
    assert not dc.set_apart(o) and o["n_final_pairs"] > len(local)
    r = capi.icp_align_layers([dict(map=dm, scan=capi.Scan(ctx, local), threshold=thr)], T0, kbest_ref.device_params(c),
                              want_pairs=True, pairings_per_point=2)
    print("occupancy search map, k = 2: iterations %d / %d, final pairs %d / %d, max |dT| %.2e" % (
        r["n_iterations"], o["n_iterations"], r["n_final_pairs"], o["n_final_pairs"], float(np.abs(np.asarray(r["T"]) - o["T"]).max())))
    diffs = layers_oracle.compare(r, o)
    assert not diffs, diffs
    occ.close()


def test_clearance_map_before_and_after_a_key_frame(ctx, inp, oracle, monkeypatch):
    """room_clear (min_distance_between_points 0.02, SparseTreesPointCloud's clearance): the alignment before and after one
    key-frame is merged (Map.insert against insert_posed on the oracle) -- the records and the lazy sub-voxel index are rebuilt
    between the two."""
    pts, vs, cap, md = inp.maps["room_clear"]
    dm = capi.Map(ctx, vs, cap, min_distance_between_points=md).build(pts)
    om = oracle_c.Map(vs, cap, min_distance_between_points=md).insert(pts)
    s = inp.scan[:2000]
    c = dict(pairs=[dc._kp("m", s[0::2], dc.schedule(12), k=2), dc._kp("m", s[1::2], dc.schedule(12, 1.2, 0.5))], max_it=12,
             kp=np.full(12, 0.3), inner=2, T0=inp.T0, prior=None, pkw=dict(disable_stall_test=True), kind="k")
    kf = capi.Scan(ctx, inp.keyframe)
    for stage in ("before", "after"):
        if stage == "after":
            dm.insert(kf, inp.T_kf)
            om.insert_posed(inp.keyframe, inp.T_kf)
        g, d = dm.download(), om.dump()
        for key in ("vox_keys", "vox_first", "vox_count", "src_idx", "xyz"):
            np.testing.assert_array_equal(g[key], d[key], err_msg="%s: %s" % (stage, key))
        print("%s the key-frame: %d records, largest voxel %d" % (stage, len(d["xyz"]), int(dc.occupancy(d).max())))
        o = dc.case_reference(c, {"m": om})
        assert not dc.set_apart(o) and o["n_final_pairs"] > 2000
        _check(_device(ctx, {"m": dm}, c), c, o, "layers, %s" % stage)
        monkeypatch.setenv("MH_MATCH", "f")
        g1 = capi.icp_align(dm, capi.Scan(ctx, s), inp.T0, dc.single_params(capi, 12), want_pairs=True)
        monkeypatch.delenv("MH_MATCH")
        o1 = oracle_c.icp_align(om, s, inp.T0, dc.single_params(oracle_c, 12), want_pairs=True)
        _assert_single_is_the_oracles(g1, o1, "MH_MATCH=f, %s" % stage)
