"""Every device route far from the origin, held to the reference it is held to near the origin.

The inputs are tests/far_cases.py's: the dense-cell inputs shifted by D1 = (4099.3, -2051.7, 3.1), D2 = (-52431.7, 30011.3, -12.4)
and D3 = (4.1e5, -3.9e5, 50) metres, where the fp32 spacing is 0.5 mm, 4 mm and 1/32 m; tests/test_far_cpu.py shows on the CPU
that the references stay sound there (nothing set apart, two implementations within 5.8e-11).  The route inventory is
tests/route_tables.py's, the comparisons are the near-origin tests' own (loaded from their files): per-iteration pair counts,
final local_idx / global_idx / d2 / global_xyz, termination bit for bit, single-pair poses within 1e-9 of oracle_c, covariances
at tests/test_gpu_solver_params.py's tolerance, multi-layer results through layers_oracle.compare.  Nothing here widens a bound
for the distance: a search margin that does not scale with the coordinate fails on room07 (the 0.7 m voxel, whose voxel faces
are no fp32 numbers).

The last section probes the key-range rule (|p' / voxel_size| >= 1e6 on any axis pairs with nothing and is left out of a map)
AT the limit, for the searches only: the oracle has no key range, so it is the reference for the content the device kept and for
the queries the contract classifies as in range."""
import importlib.util
import os

import numpy as np
import pytest

import dense_cases as dc
import far_cases as fc
import radius_ref as rr
import score_ref as sr
from mola_lidar_odometry_amd import capi, synth
from oracle import oracle_c
from route_tables import (FAMILIES, LOOP16_CASES, LOOPW_CASES, MULTI, PLANE_MATCHER_KERNELS, POINT_MATCHER_KERNELS, SEARCH, env_id,
                          loop_expected)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _module(name):
    """a near-origin test file loaded by path under a private name: its comparisons keep ONE definition, nothing of it is
    collected here (as tests/test_gpu_solver_params.py loads tests/test_gpu_parity.py)"""
    spec = importlib.util.spec_from_file_location("_far_" + name, os.path.join(ROOT, "tests", name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


_dense, _solver, _occ, _pre = (_module(n) for n in ("test_gpu_dense_cells", "test_gpu_solver_params", "test_gpu_occmap",
                                                    "test_gpu_preprocess"))
_assert_single_is_the_oracles, _assert_same_bits, _Once = _dense._assert_single_is_the_oracles, _dense._assert_same_bits, _dense._Once
_assert_matches, _assert_maps_equal = _solver._assert_matches, _pre._assert_maps_equal

F = np.float32
ALL = dict(fc.OFFSETS, O=fc.ORIGIN)
COV_RTOL, COV_ATOL = 2e-5, 1e-6   # tests/test_gpu_solver_params.py::_assert_matches


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def far(ctx, oracle):
    """offset name -> (inputs, oracle maps, device maps), built on first use"""
    def make(name):
        inp = fc.far_inputs(ALL[name])
        return inp, inp.omaps(), inp.dmaps(ctx)
    return _Once(make)


@pytest.fixture(scope="module")
def single_refs(far):
    """(offset, map, n, iterations) -> oracle_c.icp_align with pairs"""
    def make(k):
        inp, omaps, _ = far[k[0]]
        return oracle_c.icp_align(omaps[k[1]], dc.single_scan(inp, k[2]), inp.T0, dc.single_params(oracle_c, k[3]),
                                  prior=dc.single_prior(inp, k[2]), want_pairs=True)
    return _Once(make)


@pytest.fixture(scope="module")
def multi_refs(far):
    """(offset, case name) -> (case, reference)"""
    cases = _Once(lambda name: dc.cases(far[name][0]))

    def make(k):
        c = cases[k[0]]["k2" if k[1] == "k2_room07" else k[1]]
        if k[1] == "k2_room07":
            c = dict(c, pairs=[dict(e, map="room07") for e in c["pairs"]])
        return c, dc.case_reference(c, far[k[0]][1])
    return _Once(make)


def _single(far, name, scan, mk, n, n_it=dc.SINGLE_IT):
    inp, _, dmaps = far[name]
    return capi.icp_align(dmaps[mk], scan, inp.T0, dc.single_params(capi, n_it), prior=dc.single_prior(inp, n), want_pairs=True)


def _assert_cov(g, o, what):
    np.testing.assert_allclose(g["cov"], o["cov"], rtol=COV_RTOL, atol=COV_ATOL * np.abs(o["cov"]).max(), err_msg=what)


def _setenv(monkeypatch, *envs):
    for env in envs:
        for k, v in env.items():
            monkeypatch.setenv(k, v)


# ----------------------------------------------------------------------------- a. single pair, every family x search switch
# room and mixed at D1 - D3; room07 (the voxel whose faces are no fp32 numbers) where records leave their slabs: D2 and D3
SINGLE_AT = [(name, mk) for name in fc.OFFSETS for mk in fc.SINGLE_MAPS] + [("D2", "room07"), ("D3", "room07")]


@pytest.mark.parametrize("search", SEARCH, ids=env_id)
@pytest.mark.parametrize("family", FAMILIES, ids=env_id)
@pytest.mark.parametrize("n", fc.SINGLE_SIZES)
@pytest.mark.parametrize("name,mk", SINGLE_AT)
def test_single_pair_every_family(ctx, far, single_refs, name, mk, n, family, search, monkeypatch):
    inp = far[name][0]
    _setenv(monkeypatch, family, search)
    s0, a0 = capi.loop_stats()
    g = _single(far, name, capi.Scan(ctx, dc.single_scan(inp, n)), mk, n)
    s1, a1 = capi.loop_stats()
    assert a1 == a0                                     # no loop was abandoned (it would change what later tests run)
    if family != {"MH_MATCH": "s"}:
        assert s1 == s0
    elif n <= 2560:
        assert s1 == s0 + 1                             # the row search's loop k_icp16
    what = "%s %s n %d %s %s" % (name, mk, n, env_id(family), env_id(search))
    o = single_refs[(name, mk, n, dc.SINGLE_IT)]
    _assert_single_is_the_oracles(g, o, what)
    _assert_cov(g, o, what)


@pytest.mark.parametrize("n", [1, 63, 64, 65])
@pytest.mark.parametrize("match", ["f", "s"])
@pytest.mark.parametrize("mk", fc.SINGLE_MAPS)
def test_single_pair_small_layers_at_the_largest_offset(ctx, far, single_refs, mk, match, n, monkeypatch):
    monkeypatch.setenv("MH_MATCH", match)
    s0, a0 = capi.loop_stats()
    g = _single(far, "D3", capi.Scan(ctx, dc.single_scan(far["D3"][0], n)), mk, n)
    assert capi.loop_stats() == (s0 + (1 if match == "s" else 0), a0)
    o = single_refs[("D3", mk, n, dc.SINGLE_IT)]
    _assert_single_is_the_oracles(g, o, "D3 %s MH_MATCH=%s n %d" % (mk, match, n))
    _assert_cov(g, o, "D3 %s MH_MATCH=%s n %d" % (mk, match, n))


# ----------------------------------------------------------------------------- b. the one-launch loops and the chain
def _loop_chain_oracle(ctx, far, single_refs, name, n, n_it, monkeypatch, what):
    scan = capi.Scan(ctx, dc.single_scan(far[name][0], n))
    s0, a0 = capi.loop_stats()
    loop = _single(far, name, scan, "room", n, n_it)
    s1, a1 = capi.loop_stats()
    assert s1 - s0 == 1 and a1 == a0, "%s: the loop started %d times, abandoned %d" % (what, s1 - s0, a1 - a0)
    monkeypatch.setenv("MH_NO_LOOP16", "1")
    chain = _single(far, name, scan, "room", n, n_it)
    assert capi.loop_stats() == (s1, a1)
    _assert_same_bits(loop, chain, what)
    _assert_single_is_the_oracles(chain, single_refs[(name, "room", n, n_it)], what + ", chain")


@pytest.mark.parametrize("n,n_it", LOOP16_CASES)
@pytest.mark.parametrize("name", ["D2", "D3"])
def test_k_icp16_gives_the_chain_s_bits_and_the_chain_the_oracle_s(ctx, far, single_refs, name, n, n_it, monkeypatch):
    _loop_chain_oracle(ctx, far, single_refs, name, n, n_it, monkeypatch, "%s k_icp16 n %d" % (name, n))


@pytest.mark.parametrize("n,n_it", LOOPW_CASES)
@pytest.mark.parametrize("name", ["D2", "D3"])
def test_k_icpw_gives_the_chain_s_bits_and_the_chain_the_oracle_s(ctx, far, single_refs, name, n, n_it, monkeypatch):
    monkeypatch.setenv("MH_LOOPW", "all")
    _loop_chain_oracle(ctx, far, single_refs, name, n, n_it, monkeypatch, "%s k_icpw n %d" % (name, n))


# ----------------------------------------------------------------------------- c. one lock-step batch, jobs at different offsets
BATCH_AT = ["O", "D2", "D3"]
RESULT_KEYS = _dense.RESULT_KEYS


@pytest.fixture(scope="module")
def three(far):
    """three contexts, each with the dense room at its own offset (origin, D2, D3)"""
    ctxs = [capi.Context(0) for _ in BATCH_AT]
    maps = [far[name][0].dmaps(c, ["room", "capped"]) for name, c in zip(BATCH_AT, ctxs)]
    yield ctxs, maps
    for c in ctxs:
        c.close()


@pytest.mark.parametrize("sizes,n_it,env,loops", [((2561, 129, 2000), 6, {}, True),                    # k_icpw_b side by side
                                                  ((2000, 2561, 129), 6, {"MH_NO_LOOP16_BATCH": "1"}, False)])
def test_lockstep_batch_of_single_pairs_across_offsets(ctx, far, three, sizes, n_it, env, loops, monkeypatch):
    """mh_icp_align_batch: the jobs of one launch sit at the origin, D2 and D3, with ragged sizes on both sides of 2560; every
    job gives the bits of its single call on the launch chain (which section b holds to the oracle).  One job's magnitudes must
    not reach another's bound or sums."""
    ctxs, maps = three
    p = dc.single_params(capi, n_it)
    inps = [far[name][0] for name in BATCH_AT]
    locals_ = [dc.single_scan(inp, n) for inp, n in zip(inps, sizes)]
    scans = [capi.Scan(c, l) for c, l in zip(ctxs, locals_)]
    guesses = [inps[0].T0, inps[1].T1, inps[2].T0]
    _setenv(monkeypatch, env)
    s0, a0 = capi.loop_stats()
    batch = capi.icp_align_batch([m["room"] for m in maps], scans, guesses, p)
    s1, a1 = capi.loop_stats()
    assert a1 == a0
    assert s1 - s0 == (len(sizes) if loops else 0)
    monkeypatch.setenv("MH_NO_LOOP16", "1")
    for name, m, l, T, b in zip(BATCH_AT, maps, locals_, guesses, batch):
        solo = capi.icp_align(far[name][2]["room"], capi.Scan(ctx, l), T, p, want_trace=False)
        assert solo["n_final_pairs"] > 100
        _assert_same_bits(b, solo, "batch job at %s, n %d" % (name, len(l)))
    assert capi.loop_stats() == (s1, a1)


@pytest.mark.parametrize("cname", ["two_pairs", "beside_capped", "k2", "unique", "gated", "rgbd"])
def test_lockstep_batch_of_layers_across_offsets(far, three, cname):
    """mh_icp_align_layers_batch, the same three offsets in one call: every job bitwise its single call"""
    ctxs, maps = three
    jobs, kpp, solo, guesses = [], [], [], []
    for name, cx, dm, which in zip(BATCH_AT, ctxs, maps, ("T0", "T1", "T0")):
        inp = far[name][0]
        c = dc.cases(inp)[cname]
        if name == "D2":   # ragged: the job in the middle loses a third of each layer
            c = dict(c, pairs=[dict(e, local=np.ascontiguousarray(e["local"][:(2 * len(e["local"])) // 3])) for e in c["pairs"]])
        p = dc.device_params(c)
        pairs, ks = dc.device_pairs(c, dm, lambda a, cx=cx: capi.Scan(cx, a))
        T = getattr(inp, which)
        jobs.append(pairs)
        kpp.append(ks)
        guesses.append(T)
        solo.append(capi.icp_align_layers(pairs, T, p, want_trace=False, pairings_per_point=ks))
    got = capi.icp_align_layers_batch(jobs, guesses, p, pairings_per_point=kpp, planes_entry=True)
    for j, (r, s) in enumerate(zip(got, solo)):
        assert s["n_final_pairs"] > 0
        for k in ("T", "cov"):
            assert np.asarray(r[k]).tobytes() == np.asarray(s[k]).tobytes(), (cname, BATCH_AT[j], k)
        for k in RESULT_KEYS:
            assert r[k] == s[k], (cname, BATCH_AT[j], k)


# ----------------------------------------------------------------------------- d. multi-layer
def _device(ctx, far, name, c):
    return _dense._device(ctx, far[name][2], c)


@pytest.mark.parametrize("cname", MULTI + ["k2_room07"])
@pytest.mark.parametrize("name", ["D2", "D3"])
def test_multi_layer_matches_the_reference(ctx, far, multi_refs, name, cname):
    c, o = multi_refs[(name, cname)]
    assert not dc.set_apart(o) and o["n_final_pairs"] > 0
    _dense._check(_device(ctx, far, name, c), c, o, "%s %s" % (name, cname))


@pytest.mark.parametrize("cname", ["k2", "rgbd", "k2_room07"])
def test_bitwise_equal_with_and_without_bound_index_and_graphs(ctx, far, multi_refs, cname, monkeypatch):
    c, _ = multi_refs[("D3", cname)]
    runs = [_device(ctx, far, "D3", c)]
    for var in ("MH_NO_PREV_BOUND", "MH_NO_QIDX", "MH_NO_GRAPH"):
        monkeypatch.setenv(var, "1")
        runs.append(_device(ctx, far, "D3", c))
        monkeypatch.delenv(var)
    runs.append(_device(ctx, far, "D3", c))
    assert runs[0]["n_iterations"] >= 10 and runs[0]["n_final_pairs"] > 2000
    for other in runs[1:]:
        for key in ("T", "cov"):
            assert np.asarray(other[key]).tobytes() == np.asarray(runs[0][key]).tobytes(), key
        assert other["pair_counts"] == runs[0]["pair_counts"]
        assert [t["n_pairs"] for t in other["trace"]] == [t["n_pairs"] for t in runs[0]["trace"]]
        for a, b in zip(other["pairs"], runs[0]["pairs"]):
            for key in a:
                assert a[key].tobytes() == b[key].tobytes(), key


# ----------------------------------------------------------------------------- e. every kernel by size, plain and NDT maps at D2
@pytest.fixture(scope="module")
def ndt_far(ctx, oracle):
    """ndt -> (device map, oracle map) of synth.ndt_cloud(11) shifted by D2"""
    cloud = fc.shift_points(_solver._cloud(), fc.D2)

    def make(ndt):
        args = _solver.NDT_ARGS if ndt else _solver.PLAIN_ARGS
        return capi.Map(ctx, *args).build(cloud), oracle_c.Map(*args).insert(cloud)
    return _Once(make)


@pytest.fixture(scope="module")
def kernel_refs(ndt_far):
    """(ndt, n, inner, skip) -> the oracle's alignment with unit weights, guess (and the plain map's prior) shifted by D2"""
    def make(k):
        ndt, n, inner, skip = k
        return oracle_c.icp_align(ndt_far[ndt][1], _solver._scan(n), _far_guess(), _solver._p(oracle_c, ndt, (1.0, 1.0), inner, skip),
                                  prior=_far_prior(ndt), want_pairs=True)
    return _Once(make)


def _far_guess():
    return fc.shift_pose(_solver._guess(), fc.D2)


def _far_prior(ndt):
    return None if ndt else (_far_guess(), _solver.LAM)


def _kernel_row(ctx, ndt_far, kernel_refs, ndt, n, env, inner, skip, monkeypatch):
    o = kernel_refs[(ndt, n, inner, skip)]
    _setenv(monkeypatch, env)
    s0, a0 = capi.loop_stats()
    g = capi.icp_align(ndt_far[ndt][0], capi.Scan(ctx, _solver._scan(n)), _far_guess(), _solver._p(capi, ndt, (1.0, 1.0), inner, skip),
                       prior=_far_prior(ndt), want_pairs=True)
    s1, a1 = capi.loop_stats()
    assert (s1 - s0, a1 - a0) == ((1, 0) if loop_expected(n, env) else (0, 0))
    print("ndt %d n %d %s: iterations %d, final pairs %d + %d planes, max |dT| %.2e" % (
        ndt, n, env_id(env), g["n_iterations"], g["n_final_pairs"], g["n_final_pairs_pt2pl"], float(np.abs(g["T"] - o["T"]).max())))
    _assert_matches(g, o)
    return g


@pytest.mark.parametrize("n,env,inner,skip", PLANE_MATCHER_KERNELS)
def test_every_plane_matcher_kernel_on_the_ndt_map(ctx, ndt_far, kernel_refs, n, env, inner, skip, monkeypatch):
    g = _kernel_row(ctx, ndt_far, kernel_refs, True, n, env, inner, skip, monkeypatch)
    assert g["n_final_pairs_pt2pl"] > n // 5


@pytest.mark.parametrize("n,env", POINT_MATCHER_KERNELS)
def test_every_point_matcher_family_on_the_plain_map(ctx, ndt_far, kernel_refs, n, env, monkeypatch):
    g = _kernel_row(ctx, ndt_far, kernel_refs, False, n, env, 2, False, monkeypatch)
    assert g["n_final_pairs"] > n // 4


def test_ndt_voxel_statistics(ndt_far):
    """test_gpu_parity.py::test_ndt_map_build_parity at D2: which voxels are planes exactly; centroids within one fp32 ulp of the
    oracle's value (an absolute 1e-6 means nothing at 5e4 m); normals to 1e-6, up to sign."""
    g, o = ndt_far[True]
    _assert_maps_equal(g.download(), o.dump())
    gn, on = g.download_ndt(), o.dump_ndt()
    np.testing.assert_array_equal(gn["is_plane"], on["is_plane"])
    pl = on["is_plane"] != 0
    assert g.info().n_planes == int(pl.sum()) > 100
    u = fc.ulps(gn["centroid"][pl], on["centroid"][pl])
    dn = np.minimum(np.abs(gn["normal"][pl] - on["normal"][pl]), np.abs(gn["normal"][pl] + on["normal"][pl]))
    print("NDT statistics at D2: %d planes, largest centroid difference %.2f ulp, largest normal difference %.2e" % (
        int(pl.sum()), float(u.max()), float(dn.max())))
    assert u.max() <= 1.0
    assert dn.max() <= 1e-6


# ----------------------------------------------------------------------------- f. stand-alone searches
def _far_T(T, D):
    return fc.shift_pose(T, D)


@pytest.fixture(scope="module")
def radius_capped(ctx, oracle):
    """offset -> (device map, oracle dump) of radius_ref.capped_points() shifted (voxel 1.0, cap 20)"""
    def make(name):
        pts = fc.shift_points(rr.capped_points(), ALL[name])
        return capi.Map(ctx, 1.0, 20).build(pts), oracle_c.Map(1.0, 20).insert(pts).dump()
    return _Once(make)


def _radius_agree(got, ref, what):
    bad = rr.same(got, ref)
    assert bad is None, (what, bad)


@pytest.mark.parametrize("radius", rr.RADII)
@pytest.mark.parametrize("name", list(fc.OFFSETS))
def test_radius_search_capped_map(ctx, radius_capped, name, radius):
    m, d = radius_capped[name]
    T = _far_T(rr.pose(), ALL[name])
    s = capi.Scan(ctx, rr.capped_queries())
    for sorted_ in (False, True):
        ref = rr.radius_search(d, 1.0, rr.capped_queries(), T, radius, sorted=sorted_)
        assert ref.counts().max() > 0 or radius < 0.1
        _radius_agree(capi.nn_search_radius(m, s, T, radius, sorted=sorted_), ref, (name, radius, sorted_))
    s.close()


# (room07: a radius of at most MH_RADIUS_MAX_VOXELS = 3 voxels of 0.7 m; its records leave their slabs from D2 on)
DENSE_RADIUS = [(name, "room", r) for name in fc.OFFSETS for r in rr.RADII] + [(name, "room07", r) for name in ("D2", "D3")
                                                                                for r in (0.5, 1.0, 2.0)]


@pytest.mark.parametrize("name,mk,radius", DENSE_RADIUS)
def test_radius_search_dense_room(ctx, far, name, mk, radius):
    """the dense room (rows of thousands of results at 2.5 m): 130 scan points under the first guess, both orders"""
    inp, omaps, dmaps = far[name]
    q = np.ascontiguousarray(inp.scan[:130])
    d = omaps[mk].dump()
    s = capi.Scan(ctx, q)
    for sorted_ in (False, True):
        ref = rr.radius_search(d, inp.maps[mk][1], q, inp.T0, radius, sorted=sorted_)
        _radius_agree(capi.nn_search_radius(dmaps[mk], s, inp.T0, radius, sorted=sorted_), ref, (name, mk, radius, sorted_))
    assert radius < 0.5 or ref.counts().max() > (1000 if radius >= 1.0 else 0)
    s.close()


@pytest.mark.parametrize("radius", rr.BOUNDARY_RADII)
@pytest.mark.parametrize("name", list(fc.OFFSETS))
def test_radius_search_boundary_points(ctx, oracle, name, radius):
    """radius_ref.boundary_points(): map points on voxel planes and one ulp to either side, p' -+ r exactly on those planes --
    shifted by the whole voxels nearest to D, so that they stay what they are (exact at D1 and D2; at D3 the ulp is 1/32 m and
    the neighbours of a plane are the lattice's)."""
    D = np.round(np.asarray(ALL[name]))
    b = rr.boundary_points()
    whole = np.round(b)
    on_plane = (whole.astype(np.float64) + D).astype(F)                     # exact: whole voxels
    pts = (b.astype(np.float64) + D).astype(F)
    beside = (b != whole) & (np.abs(b - whole) < 1e-5)                      # the neighbours of a plane near the origin ...
    pts = np.where(beside & (b < whole), np.nextafter(on_plane, F(-np.inf)), pts)   # ... are its fp32 neighbours out there
    pts = np.where(beside & (b > whole), np.nextafter(on_plane, F(np.inf)), pts).astype(F)
    assert int(beside.sum()) == 36 and (np.abs(pts - on_plane)[beside] > 0).all()
    T = _far_T(rr.IDENTITY, D)
    m = capi.Map(ctx, 1.0, 0).build(pts)
    d = oracle_c.Map(1.0, 0).insert(pts).dump()
    s = capi.Scan(ctx, rr.boundary_queries())
    for sorted_ in (False, True):
        ref = rr.radius_search(d, 1.0, rr.boundary_queries(), T, radius, sorted=sorted_)
        assert ref.counts().max() > 0
        _radius_agree(capi.nn_search_radius(m, s, T, radius, sorted=sorted_), ref, (name, radius, sorted_))
    m.close()
    s.close()


@pytest.mark.parametrize("mk", ["room", "room07"])
@pytest.mark.parametrize("name", ["D2", "D3"])
def test_score_poses_on_a_grid_around_the_true_pose(ctx, far, name, mk):
    """mh_score_poses against score_ref (the oracle's matcher per candidate): 7 x 7 x 5 candidates around the shifted true pose,
    600 scan points; n_paired and the integer cost exactly."""
    inp, omaps, dmaps = far[name]
    local = np.ascontiguousarray(inp.scan[:600])
    gt = dc.pose(0.40, -0.30, 0.10, np.deg2rad(5.0), np.deg2rad(1.0), np.deg2rad(-0.5))
    assert np.array_equal(fc.shift_pose(gt, inp.D), inp.T_gt)
    mean = np.array([0.40 + 0.2, -0.30 - 0.1, 0.10, np.deg2rad(5.0 + 1.0), np.deg2rad(1.0), np.deg2rad(-0.5)])
    poses, _ = sr.relocalization_grid(mean, sr.grid_cov(0.19, 0.19, np.deg2rad(1.3)), 0.2, np.deg2rad(2.0), 3.0)
    poses = np.array([fc.shift_pose(T, inp.D) for T in poses])
    assert len(poses) == 7 * 7 * 5
    ref = sr.score_poses(oracle_c, omaps[mk], local, poses, sr.THRESHOLD)
    got = capi.score_poses(dmaps[mk], capi.Scan(ctx, local), poses, sr.THRESHOLD)
    bad = sr.same(got, ref)
    assert bad is None, bad
    assert ref["n_paired"].max() > 400 and ref["n_paired"].min() < ref["n_paired"].max()


@pytest.mark.parametrize("knn,eig", dc.TIE_PLANES)
def test_ties_nn_search_pt2pl_knn_at_the_largest_offset(ctx, far, knn, eig):
    """test_gpu_dense_cells.py::test_ties_nn_search_pt2pl_knn on the shifted lattice: the same accepted set; centroids within one
    fp32 ulp of the oracle's value (1/32 m here: two roundings of one fp64 mean), normals to 1e-6 up to sign."""
    inp, omaps, dmaps = far["D3"]
    args = (0.4, eig, dc.TIE_PLANE_RADIUS, knn, dc.TIE_PLANE_MIN_POINTS)
    g = capi.nn_search_pt2pl_knn(dmaps["centres"], capi.Scan(ctx, inp.queries), dc.IDENTITY, *args)
    o = oracle_c.match_pt2pl_knn(omaps["centres"], inp.queries, dc.IDENTITY, *args)
    print("plane pairings on the shifted lattice: %d / %d" % (len(g["local_idx"]), len(o["local_idx"])))
    assert len(o["local_idx"]) > 100
    np.testing.assert_array_equal(g["local_idx"], o["local_idx"])
    assert fc.ulps(g["centroid"], o["centroid"]).max() <= 1.0
    dn = np.minimum(np.abs(g["normal"] - o["normal"]), np.abs(g["normal"] + o["normal"]))
    assert dn.max() <= 1e-6


@pytest.mark.parametrize("k", [1, 2, 8])
@pytest.mark.parametrize("mk", ["centres", "room07"])
@pytest.mark.parametrize("name", list(fc.OFFSETS))
def test_nn_search_k_is_the_oracle_s(ctx, far, name, mk, k):
    """the stand-alone k-best search (k = 1: mh_nn_search and the dense form) on the shifted lattice and under the odd voxel"""
    inp, omaps, dmaps = far[name]
    local, T, thr = (inp.queries, dc.IDENTITY, _dense.TIE_THR) if mk == "centres" else (np.ascontiguousarray(inp.scan[:2000]), inp.T0, 1.5)
    s = capi.Scan(ctx, local)
    o = oracle_c.match_points_k(omaps[mk], local, T, thr, k)
    g = capi.nn_search_k(dmaps[mk], s, T, thr, k) if k > 1 else capi.nn_search(dmaps[mk], s, T, thr)
    assert len(o["local_idx"]) > len(local) // 2
    for key in ("local_idx", "global_idx", "d2", "global_xyz"):
        np.testing.assert_array_equal(g[key], o[key], err_msg=key)
    if k == 1:
        dn = capi.nn_search_dense(dmaps[mk], s, T)
        big = oracle_c.match_points(omaps[mk], local, T, 1e3)
        np.testing.assert_array_equal(dn["global_idx"][big["local_idx"]], big["global_idx"])
        np.testing.assert_array_equal(dn["d2"][big["local_idx"]], big["d2"])


# ----------------------------------------------------------------------------- g. world-frame map kernels
@pytest.mark.parametrize("vs,cap,far_", [(1.0, 20, 0.0), (1.0, 20, 45.0), (0.5, 4, 30.0)])
@pytest.mark.parametrize("name", ["D2", "D3"])
def test_map_insert_keyframes_bit_exact(ctx, oracle, name, vs, cap, far_):
    """test_gpu_preprocess.py::test_map_insert_keyframes_bit_exact with every pose shifted: eviction is measured from a far pose
    cell, the stored content is the per-point CPU insertion's"""
    D = ALL[name]
    assert fc.usable(D, vs, reach=250.0)
    scene = synth.make_scene(777, 80.0, 12)
    g, o = capi.Map(ctx, vs, cap), oracle_c.Map(vs, cap)
    offered = 0
    for k in range(6):
        pose = [-40.0 + 14.0 * k, 0.6 * np.sin(k), synth.SENSOR_H, 0.05 * k, 0.002 * k, -0.001 * k]
        xyz = synth.make_scan(scene, pose, rings=32, azimuths=400, seed=100 + k)
        T = fc.shift_pose(synth.pose_from_ypr(pose), D)
        g.insert(capi.Scan(ctx, xyz), T, far_)
        o.insert_posed(xyz, T, far_)
        offered += len(xyz)
        i = g.info()
        assert (i.n_points, i.n_voxels, i.n_offered) == (o.num_points, o.num_voxels, offered)
        _assert_maps_equal(g.download(), o.dump())
        mn, mx = o.bbox()
        np.testing.assert_array_equal(np.array(i.bbox_min), mn)
        np.testing.assert_array_equal(np.array(i.bbox_max), mx)
    if far_:
        assert o.num_points < oracle_c.Map(vs, cap).insert_posed(xyz, T).num_points * 6
    got = capi.nn_search(g, capi.Scan(ctx, xyz), T, 1.5)
    ref = oracle_c.match_points(o, xyz, T, 1.5)
    for key in ("local_idx", "global_idx", "d2"):
        np.testing.assert_array_equal(got[key], ref[key], err_msg=key)
    g.close()


def test_clearance_map_before_and_after_a_key_frame(ctx, far, monkeypatch):
    """test_gpu_dense_cells.py's clearance test at D3 (room_clear: min_distance_between_points 0.02): the stored records before
    and after one key-frame, and the alignments on them"""
    inp = far["D3"][0]
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
        _assert_maps_equal(dm.download(), om.dump())
        o = dc.case_reference(c, {"m": om})
        assert not dc.set_apart(o) and o["n_final_pairs"] > 2000
        _dense._check(_dense._device(ctx, {"m": dm}, c), c, o, "D3 layers, %s" % stage)
        monkeypatch.setenv("MH_MATCH", "f")
        g1 = capi.icp_align(dm, capi.Scan(ctx, s), inp.T0, dc.single_params(capi, 12), want_pairs=True)
        monkeypatch.delenv("MH_MATCH")
        o1 = oracle_c.icp_align(om, s, inp.T0, dc.single_params(oracle_c, 12), want_pairs=True)
        _assert_single_is_the_oracles(g1, o1, "D3 MH_MATCH=f, %s" % stage)
    dm.close()


@pytest.mark.parametrize("name,res", [("D1", 0.1), ("D2", 0.25)])
def test_occupancy_insert_from_a_far_pose(ctx, name, res):
    """mh_occmap_insert from a pose at D1 (resolution 0.1: 4.1e4 cells out) and D2 (0.25: 2.1e5 cells): test_gpu_occmap.py's
    hand-built rays (scaled to the resolution) and a ball of 1000 points, cells, log-odds, counters and the search map against
    tests/occmap_ref.py."""
    D = ALL[name]
    assert fc.usable(D, res, reach=100.0)
    occ, ref = _occ.make(ctx, resolution=res)
    T = fc.shift_pose(_occ.pose(0.0, 0.0, 0.0, 0.0), D)
    pts = _occ.hand_built() * F(res / 0.1)
    wild = np.flatnonzero(np.abs(pts[:, 0]) > 1.0e4)                        # the point beyond the key range near the origin ...
    assert len(wild) == 1
    pts[wild, 0] = F(np.sign(D[0]) * 1.0e6 * res)                           # ... lies 1e6 cells from the pose: beyond it here too
    _occ.insert_both(ctx, occ, ref, pts, T)
    _occ.check(occ, ref)
    assert ref.n_left_out == 1
    T2 = fc.shift_pose(_occ.pose(0.3, -0.2, 0.1, 0.4), D)
    _occ.insert_both(ctx, occ, ref, _occ.ball(1000, 5.0, 1000), T2)
    keys, _ = _occ.check(occ, ref)
    assert len(keys) > 1000 and np.abs(keys).max() > 4.0e4
    occ.close()


# ----------------------------------------------------------------------------- the key-range limit itself, searches only
# voxel 1.0; the 1/16 m lattice between 999 997 and 1 000 002 is exact in fp32 (the spacing there IS 1/16 m)
LIMIT = 1.0e6
SPAN = np.arange(999997.0, 1000002.0 + 1e-9, 1.0 / 16.0)


def _limit_case(which):
    """(map points with the in-range ones first, local queries, pose, (axis, sign)): `x`: +x; `y`: -y; `pose`: the +x map, local
    queries 5e5 short of it and a translation-only pose that carries them across the limit.  Three rows of map points a quarter
    of a metre apart in one plane; the queries lie midway between two rows, so partners tie exactly."""
    axis, sign = (1, -1.0) if which == "y" else (0, 1.0)
    other = 1 - axis
    rows = []
    for off in (0.25, 0.5, 0.75):
        p = np.zeros((len(SPAN), 3))
        p[:, axis], p[:, other], p[:, 2] = sign * SPAN, off, 0.5
        rows.append(p)
    pts = np.concatenate(rows).astype(F)
    inside = np.abs(pts[:, axis]) < LIMIT
    pts = np.concatenate([pts[inside], pts[~inside]])          # the kept content is a prefix: source indices stay comparable
    q = np.zeros((len(SPAN), 3))
    q[:, axis], q[:, other], q[:, 2] = sign * SPAN, 0.375, 0.5625
    T = rr.IDENTITY.copy()
    if which == "pose":
        q[:, 0] -= 5.0e5
        T[3] = 5.0e5
    return pts, int(inside.sum()), np.ascontiguousarray(q, F), T


def _in_range(local, T, vs=1.0):
    """the contract's classification, from dense_cases.transform: |p' * (1 / vs)| < 1e6 on every axis"""
    p = dc.transform(local, T)
    return (np.abs(p * F(1.0 / vs)) < F(LIMIT)).all(axis=1)


@pytest.fixture(scope="module")
def limit(ctx, oracle):
    def make(which):
        pts, n_in, q, T = _limit_case(which)
        m = capi.Map(ctx, 1.0, 0)
        with pytest.raises(capi.MolahipError) as e:   # the points beyond the limit are reported, and left out
            m.build(pts)
        assert e.value.status == 4
        om = oracle_c.Map(1.0, 0).insert(pts[:n_in])  # the oracle has no key range: it gets the content the device kept
        return m, om, q, T, n_in
    return _Once(make)


WHICH = ["x", "y", "pose"]


@pytest.mark.parametrize("which", WHICH)
def test_limit_stored_count_of_a_map_build(limit, which):
    m, om, q, T, n_in = limit[which]
    assert n_in == 3 * 48                              # 999 997 ... 999 999.9375 of 81 lattice values, three rows
    assert int(m.info().n_points) == n_in == om.num_points
    _assert_maps_equal(m.download(), om.dump())
    ok = _in_range(q, T)
    assert int(ok.sum()) == 48 and not ok[48:].any()   # the queries straddle the limit at the exact boundary


def _kept(o, ok):
    """the oracle's pairings of the queries the contract classifies as in range"""
    keep = ok[o["local_idx"]]
    return {k: v[keep] for k, v in o.items() if isinstance(v, np.ndarray) and len(v) == len(keep)}


@pytest.mark.parametrize("k", [1, 2, 8])
@pytest.mark.parametrize("which", WHICH)
def test_limit_nn_search(ctx, limit, which, k):
    m, om, q, T, _ = limit[which]
    ok = _in_range(q, T)
    s = capi.Scan(ctx, q)
    o = _kept(oracle_c.match_points_k(om, q, T, 0.5, k), ok)
    g = capi.nn_search_k(m, s, T, 0.5, k) if k > 1 else capi.nn_search(m, s, T, 0.5)
    assert len(o["local_idx"]) >= 48 * min(k, 6) and not (~ok)[g["local_idx"]].any()
    for key in ("local_idx", "global_idx", "d2", "global_xyz"):
        np.testing.assert_array_equal(g[key], o[key], err_msg=key)
    if k == 1:
        dn = capi.nn_search_dense(m, s, T)
        assert (dn["global_idx"][~ok] == capi.NO_MATCH).all()
        big = _kept(oracle_c.match_points(om, q, T, 1e3), ok)
        assert len(big["local_idx"]) == 48
        np.testing.assert_array_equal(dn["global_idx"][ok], big["global_idx"])
        np.testing.assert_array_equal(dn["d2"][ok], big["d2"])


@pytest.mark.parametrize("which", WHICH)
def test_limit_nn_search_pt2pl_knn(ctx, limit, which):
    m, om, q, T, _ = limit[which]
    ok = _in_range(q, T)
    args = (0.4, 0.3, 0.8, 10, 6)
    o = _kept(oracle_c.match_pt2pl_knn(om, q, T, *args), ok)
    g = capi.nn_search_pt2pl_knn(m, capi.Scan(ctx, q), T, *args)
    assert len(o["local_idx"]) > 30
    np.testing.assert_array_equal(g["local_idx"], o["local_idx"])
    assert fc.ulps(g["centroid"], o["centroid"]).max() <= 1.0
    assert np.minimum(np.abs(g["normal"] - o["normal"]), np.abs(g["normal"] + o["normal"])).max() <= 1e-6


@pytest.mark.parametrize("sorted_", [False, True], ids=["visit", "sorted"])
@pytest.mark.parametrize("radius", [0.5, 1.0])
@pytest.mark.parametrize("which", WHICH)
def test_limit_nn_search_radius(ctx, limit, which, radius, sorted_):
    """radius_ref states the guard itself: the queries beyond the limit have empty rows"""
    m, om, q, T, _ = limit[which]
    ok = _in_range(q, T)
    ref = rr.radius_search(om.dump(), 1.0, q, T, radius, sorted=sorted_)
    assert (ref.counts()[~ok] == 0).all() and (ref.counts()[ok] > 0).all()
    _radius_agree(capi.nn_search_radius(m, capi.Scan(ctx, q), T, radius, sorted=sorted_), ref, (which, radius, sorted_))


@pytest.mark.parametrize("which", WHICH)
def test_limit_score_poses(ctx, limit, which):
    """a pose on each side: the case's own (48 of 81 queries in range), one 2 m back (all in range) and one 8 m out (none)"""
    m, om, q, T, _ = limit[which]
    axis, sign = (1, -1.0) if which == "y" else (0, 1.0)
    poses = []
    for step in (0.0, -2.0, 8.0):
        P = T.copy()
        P[3 + 4 * axis] += sign * step
        poses.append(P)
    poses = np.array(poses)
    ref = np.zeros(len(poses), sr.SCORE_DTYPE)
    for c, P in enumerate(poses):
        o = _kept(oracle_c.match_points(om, q, P, sr.THRESHOLD), _in_range(q, P))
        ref["n_paired"][c], ref["cost"][c] = sr.reduce_pairs(o["d2"], sr.THRESHOLD)
    assert ref["n_paired"][0] == 48 and ref["n_paired"][1] > 48 and ref["n_paired"][2] == 0
    bad = sr.same(capi.score_poses(m, capi.Scan(ctx, q), poses, sr.THRESHOLD), ref)
    assert bad is None, bad


@pytest.mark.parametrize("which", WHICH)
def test_limit_occupancy_insert_counts_what_it_leaves_out(ctx, which):
    """mh_occmap_insert at resolution 1.0 from a pose a few cells inside the limit: n_left_out is the number of points the
    contract classifies as out of range, the rest is stored (tests/occmap_ref.py, counters included)"""
    _, _, q, T, = _limit_case(which)
    axis, sign = (1, -1.0) if which == "y" else (0, 1.0)
    P = T.copy()
    back = 999990.5 if which != "pose" else 499990.5
    local = q.astype(np.float64)
    local[:, axis] -= sign * back          # the sensor sits at 999 990.5 along the axis; the points keep their world positions
    P[3 + 4 * axis] += sign * back
    local = np.ascontiguousarray(local, F)
    ok = _in_range(local, P)
    assert int(ok.sum()) == 48 and np.array_equal(dc.transform(local, P)[:, axis], dc.transform(q, T)[:, axis])
    occ, ref = _occ.make(ctx, resolution=1.0)
    _occ.insert_both(ctx, occ, ref, local, P)
    _occ.check(occ, ref)
    assert occ.info().n_left_out == int((~ok).sum()) == 33
    occ.close()
