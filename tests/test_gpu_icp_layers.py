"""mh_icp_align_layers on the device: one ICP alignment over several Matcher_Points_DistanceThreshold (map, scan) pairs with one
Gauss-Newton solve (the ICP blocks of the reference's pipelines/extras/lidar3d-dual-map.yaml and lidar3d-edges.yaml).

Checked against mh_icp_align for one pair, against the float64 reference oracle/layers_oracle.py for several pairs (8 pairs on
the workgroup edges, mixed weights, every robust kernel, NDT and trunc-indexed maps), against exact identities (a scan split into
pieces, permuted pairs, loop-control switches, a shared context), and through the host layer against its matcher-by-matcher loop."""
import numpy as np
import pytest

from mola_lidar_odometry_amd import capi, synth
from oracle import layers_oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    return capi.Context(0)


def _split(w):
    """The small workload as a dual-map-like shape: near / far scan layers (overlapping), a 0.5 m near map and a 1.0 m far map."""
    scan = w.scan_xyz
    rng = np.linalg.norm(scan, axis=1)
    near_l, far_l = scan[rng < 9.0], scan[rng >= 6.0]
    T0 = w.T_gt.reshape(3, 4)
    mr = np.linalg.norm(w.map_xyz - T0[:, 3], axis=1)
    near_g, far_g = w.map_xyz[mr < 12.0], w.map_xyz[::2]
    return near_l, far_l, near_g, far_g


class _Shape:
    def __init__(self, ctx, oracle, w):
        self.w = w
        self.near_l, self.far_l, near_g, far_g = _split(w)
        self.ctx = ctx
        self.maps = {"near": capi.Map(ctx, 0.5, 20).build(near_g), "far": capi.Map(ctx, 1.0, 20).build(far_g)}
        self.omaps = {"near": oracle.Map(0.5, 20).insert(near_g), "far": oracle.Map(1.0, 20).insert(far_g)}
        self.scans = {"near": capi.Scan(ctx, self.near_l), "far": capi.Scan(ctx, self.far_l)}
        self.locs = {"near": self.near_l, "far": self.far_l}
        for key, args in (("ndt", (1.0, 12, capi.INDEX_FLOOR, 0.0, 0.05, 4)), ("trunc", (0.7, 3, capi.INDEX_TRUNC))):
            self.maps[key] = capi.Map(ctx, *args).build(w.map_xyz)
            self.omaps[key] = oracle.Map(*args).insert(w.map_xyz)

    def add_scan(self, key, xyz):
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        self.scans[key], self.locs[key] = capi.Scan(self.ctx, xyz), xyz
        return key


@pytest.fixture(scope="module")
def shape(ctx, oracle, small_workload):
    return _Shape(ctx, oracle, small_workload)


def _base(sigma, n):
    k = np.arange(n, dtype=np.float64)
    return np.maximum(sigma, 2.0 * sigma - (2.0 * sigma - 0.5 * sigma) * k / 30.0)


def _reference(oracle, sh, spec, T0, max_it, kp, weights=None, prior=None, hook=None, inner=2, kernel=capi.KERNEL_GM_C4, **kw):
    """spec: [(map key, scan key, thr[max_it], angular deg)]; oracle/layers_oracle.py's result for mh_icp_align_layers with pair
    i at weights[i] (1 when None)."""
    p = oracle.ICPParams(max_iterations=max_it, kernel_param=kp,
                         gn=oracle.GNParams(max_inner_iterations=inner, robust_kernel=kernel), **kw)
    if hook is not None:
        p.hook_enabled, (p.hook_checkpoint, p.hook_min_trans, p.hook_min_rot) = True, hook
    pairs = [dict(map=sh.omaps[mk], local=sh.locs[sk], threshold=thr, threshold_angular_deg=ang,
                  weight=1.0 if weights is None else weights[i]) for i, (mk, sk, thr, ang) in enumerate(spec)]
    return layers_oracle.icp_align_layers(pairs, T0, p, prior=prior)


def _pairs(sh, spec, weights=None):
    return [dict(map=sh.maps[mk], scan=sh.scans[sk], threshold=thr, threshold_angular_deg=ang,
                 weight=1.0 if weights is None else weights[i]) for i, (mk, sk, thr, ang) in enumerate(spec)]


def _params(max_it, kp, inner=2, kernel=capi.KERNEL_GM_C4, **kw):
    return capi.ICPParams(max_iterations=max_it, kernel_param=kp, threshold=1.0,
                          gn=capi.GNParams(max_inner_iterations=inner, robust_kernel=kernel), **kw)


def _assert_matches_reference(r, o):
    """Everything mh_icp_align_layers reports, against the reference: layers_oracle.compare() lists what differs."""
    assert o["n_final_pairs"] > 0
    diffs = layers_oracle.compare(r, o)
    assert not diffs, diffs


# ---------------------------------------------------------------------------------------------------- one pair = mh_icp_align
@pytest.mark.parametrize("name", ["small", "creal", "c2"])
def test_one_pair_equals_icp_align(ctx, monkeypatch, name):
    """One pair is mh_icp_align's alignment.  The multi-layer path runs the plan / scan matcher + k_accum over 1024-point columns
    (the chain of MH_MATCH=f): bit for bit that chain's result; the default chain of a small layer sums other columns (the row
    kernels, the one-launch loops), so against it the pose agrees to rounding."""
    w = synth.workload_by_name(name)
    m = capi.Map(ctx, w.voxel_size, w.cap).build(w.map_xyz)
    s = capi.Scan(ctx, w.scan_xyz)
    p = capi.ICPParams(max_iterations=w.n_iters, threshold=w.threshold, kernel_param=w.kernel_param, threshold_angular_deg=0.2)
    lay = capi.icp_align_layers([dict(map=m, scan=s, threshold=w.threshold, threshold_angular_deg=0.2)], w.T_guess, p,
                                want_pairs=True)
    monkeypatch.setenv("MH_MATCH", "f")
    ref = capi.icp_align(m, s, w.T_guess, p, want_pairs=True)
    monkeypatch.delenv("MH_MATCH")
    dflt = capi.icp_align(m, s, w.T_guess, p)
    for k in ("T", "cov"):
        np.testing.assert_array_equal(lay[k], ref[k])
    for k in ("quality", "n_iterations", "termination_reason", "n_final_pairs", "potential_pairings"):
        assert lay[k] == ref[k], k
    assert lay["pair_counts"] == [ref["n_final_pairs"]]
    for k in ("local_idx", "global_idx", "global_xyz", "d2"):
        np.testing.assert_array_equal(lay["pairs"][0][k], ref["pairs"][k])
    assert [t["n_pairs"] for t in lay["trace"]] == [t["n_pairs"] for t in ref["trace"]]
    assert lay["n_iterations"] == dflt["n_iterations"] and lay["n_final_pairs"] == dflt["n_final_pairs"]
    np.testing.assert_allclose(lay["T"], dflt["T"], rtol=0, atol=1e-12)


# ------------------------------------------------------------------------------------------------- several pairs vs the oracle
def _specs(w, n):
    b = _base(w.sigma, 40)
    spec = [("near", "near", 2.0 * b, 0.0), ("far", "far", 1.5 * b + 0.2, 0.3)]
    if n == 3:
        spec.append(("far", "near", np.full(40, 1.1), 0.0))  # the far map twice, the near scan twice
    return spec, 0.5 * b


@pytest.mark.parametrize("n", [2, 3])
def test_several_pairs_match_an_oracle_loop(oracle, shape, n):
    w = shape.w
    spec, kp = _specs(w, n)
    r = capi.icp_align_layers(_pairs(shape, spec), w.T_guess, _params(40, kp), want_pairs=True)
    o = _reference(oracle, shape, spec, w.T_guess, 40, kp)
    assert r["termination_reason"] == o["termination_reason"]
    assert r["n_iterations"] == o["n_iterations"]
    n_pairs = o["n_final_pairs"]
    potential = sum(len(shape.locs[sk]) for _, sk, _, _ in spec)
    assert r["n_final_pairs"] == n_pairs and r["potential_pairings"] == potential
    assert r["quality"] == pytest.approx(n_pairs / potential, abs=1e-12)
    assert r["pair_counts"] == o["pair_counts"]
    for i in range(n):
        np.testing.assert_array_equal(r["pairs"][i]["local_idx"], o["pairs"][i]["local_idx"])
    np.testing.assert_allclose(r["T"], o["T"], rtol=0, atol=1e-7)
    _assert_matches_reference(r, o)
    assert r["trace"][0]["threshold"] == spec[0][2][0]  # the trace reports pair 0's threshold
    assert np.abs(r["T"] - w.T_gt).max() < 0.05


# ---------------------------------------------------------------------------------------------------------------- weights
def _prior(w):
    info = np.eye(6) * np.array([4e4, 4e4, 4e4, 1e5, 1e5, 1e5])
    Tp = w.T_gt.copy()
    Tp[3] += 0.20  # pulls 20 cm along x
    return Tp, info


def test_common_weight_with_prior_matches_the_oracle(oracle, shape):
    w = shape.w
    spec, kp = _specs(w, 2)
    prior = _prior(w)
    r3 = capi.icp_align_layers(_pairs(shape, spec, [3.0, 3.0]), w.T_guess, _params(40, kp), prior=prior)
    r1 = capi.icp_align_layers(_pairs(shape, spec), w.T_guess, _params(40, kp), prior=prior)
    o = _reference(oracle, shape, spec, w.T_guess, 40, kp, weights=[3.0, 3.0], prior=prior)
    assert r3["termination_reason"] == o["termination_reason"] and r3["n_iterations"] == o["n_iterations"]
    np.testing.assert_allclose(r3["T"], o["T"], rtol=0, atol=1e-7)
    assert np.abs(r3["T"] - r1["T"]).max() > 1e-4  # the weight matters against the prior


def test_mixed_weights_equal_duplicated_pairs(shape):
    w = shape.w
    spec, kp = _specs(w, 2)
    prior = _prior(w)
    a = capi.icp_align_layers(_pairs(shape, spec, [2.0, 1.0]), w.T_guess, _params(40, kp), prior=prior)
    b = capi.icp_align_layers(_pairs(shape, [spec[0], spec[0], spec[1]]), w.T_guess, _params(40, kp), prior=prior)
    assert a["n_iterations"] == b["n_iterations"] and a["termination_reason"] == b["termination_reason"]
    np.testing.assert_allclose(a["T"], b["T"], rtol=0, atol=1e-9)
    one = capi.icp_align_layers(_pairs(shape, spec), w.T_guess, _params(40, kp), prior=prior)
    assert np.abs(a["T"] - one["T"]).max() > 1e-4


# ------------------------------------------------------------------------------------------------------------- covariance
def test_covariance_over_the_union_of_final_pairings(ctx, shape):
    w = shape.w
    spec, kp = _specs(w, 3)
    r = capi.icp_align_layers(_pairs(shape, spec), w.T_guess, _params(40, kp), want_pairs=True)
    lp = np.concatenate([shape.locs[sk][r["pairs"][i]["local_idx"]] for i, (_, sk, _, _) in enumerate(spec)])
    gp = np.concatenate([r["pairs"][i]["global_xyz"] for i in range(len(spec))])
    cov = capi.covariance(ctx, r["T"], pt2pt=(lp, gp))
    np.testing.assert_allclose(r["cov"], cov, rtol=1e-9, atol=0)


# ------------------------------------------------------------------------------------------------------- edges and errors
def test_empty_scan_pairs(ctx, shape):
    w = shape.w
    spec, kp = _specs(w, 2)
    empty = capi.Scan(ctx, np.zeros((0, 3), np.float32))
    p = _params(40, kp)
    base = capi.icp_align_layers(_pairs(shape, spec), w.T_guess, p)
    with_empty = capi.icp_align_layers(_pairs(shape, spec) + [dict(map=shape.maps["near"], scan=empty, threshold=1.0)],
                                       w.T_guess, p)
    for k in ("T", "cov"):
        np.testing.assert_array_equal(with_empty[k], base[k])
    for k in ("n_iterations", "termination_reason", "n_final_pairs", "potential_pairings"):
        assert with_empty[k] == base[k], k
    assert with_empty["pair_counts"] == base["pair_counts"] + [0]
    none = capi.icp_align_layers([dict(map=shape.maps["near"], scan=empty, threshold=1.0),
                                  dict(map=shape.maps["far"], scan=empty, threshold=1.0)], w.T_guess, p)
    assert capi.TERM_NAMES[none["termination_reason"]] == "NoPairings" and none["n_final_pairs"] == 0


def test_device_hook_stops_where_the_oracle_loop_does(oracle, shape):
    w = shape.w
    spec, kp = _specs(w, 2)
    p = _params(40, kp, hook_enabled=True, hook_min_trans=0.2, hook_min_rot=np.deg2rad(0.5), hook_checkpoint=w.T_guess)
    r = capi.icp_align_layers(_pairs(shape, spec), w.T_guess, p)
    o = _reference(oracle, shape, spec, w.T_guess, 40, kp, hook=(w.T_guess, 0.2, np.deg2rad(0.5)))
    assert capi.TERM_NAMES[o["termination_reason"]] == "HookRequest"
    assert capi.TERM_NAMES[r["termination_reason"]] == "HookRequest" and r["n_iterations"] == o["n_iterations"]
    np.testing.assert_allclose(r["T"], o["T"], rtol=0, atol=1e-7)


def _raw_call(pairs_list, p, T):
    import ctypes as C
    cp, keep = p.c(T)
    arr = (capi.LayerPair * max(1, len(pairs_list)))(*pairs_list)
    res = capi.ICPResult()
    T0 = np.ascontiguousarray(np.asarray(T, np.float64).reshape(12))
    return capi.lib().mh_icp_align_layers(len(pairs_list), arr, C.byref(cp), T0.ctypes.data_as(capi._DP), None, C.byref(res),
                                          None, None, None, capi.MEM_HOST)


def test_error_codes_leave_the_context_usable(shape):
    w = shape.w
    spec, kp = _specs(w, 2)
    thr = np.full(40, 1.0)
    good = capi.LayerPair(shape.maps["near"]._h, shape.scans["near"]._h, thr.ctypes.data_as(capi._DP), 0.0, 1.0)
    p = _params(40, kp)
    INVALID, UNSUPPORTED = 1, 6
    assert _raw_call([], p, w.T_guess) == INVALID
    assert _raw_call([good] * 9, p, w.T_guess) == INVALID
    assert _raw_call([capi.LayerPair(shape.maps["near"]._h, None, thr.ctypes.data_as(capi._DP), 0.0, 1.0)], p, w.T_guess) == INVALID
    assert _raw_call([capi.LayerPair(None, shape.scans["near"]._h, thr.ctypes.data_as(capi._DP), 0.0, 1.0)], p, w.T_guess) == INVALID
    assert _raw_call([capi.LayerPair(shape.maps["near"]._h, shape.scans["near"]._h, None, 0.0, 1.0)], p, w.T_guess) == INVALID
    other = capi.Context(0)
    foreign = capi.Scan(other, shape.near_l)
    assert _raw_call([good, capi.LayerPair(shape.maps["near"]._h, foreign._h, thr.ctypes.data_as(capi._DP), 0.0, 1.0)],
                     p, w.T_guess) == INVALID
    from dataclasses import replace
    assert _raw_call([good], replace(p, pt2pl_threshold=1.0), w.T_guess) == INVALID
    assert _raw_call([good, good], replace(p, matched_points=1), w.T_guess) == UNSUPPORTED
    assert _raw_call([good], replace(p, profile=True), w.T_guess) == UNSUPPORTED
    assert _raw_call([good], p, w.T_guess) == 0
    r = capi.icp_align_layers(_pairs(shape, spec), w.T_guess, p)
    assert r["n_final_pairs"] > 0


def test_back_to_back_calls_equal_fresh_runs(oracle, small_workload):
    w = small_workload
    spec3, kp = _specs(w, 3)
    spec2 = spec3[:2]
    p = _params(40, kp)
    a = _Shape(capi.Context(0), oracle, w)
    capi.icp_align_layers(_pairs(a, spec3), w.T_guess, p)
    r2 = capi.icp_align_layers(_pairs(a, spec2), w.T_guess, p, want_pairs=True)
    r3 = capi.icp_align_layers(_pairs(a, spec3), w.T_guess, p, want_pairs=True)
    b = _Shape(capi.Context(0), oracle, w)
    f2 = capi.icp_align_layers(_pairs(b, spec2), w.T_guess, p, want_pairs=True)
    c = _Shape(capi.Context(0), oracle, w)
    f3 = capi.icp_align_layers(_pairs(c, spec3), w.T_guess, p, want_pairs=True)
    for x, y in ((r2, f2), (r3, f3)):
        for k in ("T", "cov"):
            np.testing.assert_array_equal(x[k], y[k])
        assert x["n_iterations"] == y["n_iterations"] and x["pair_counts"] == y["pair_counts"]
        for px, py in zip(x["pairs"], y["pairs"]):
            np.testing.assert_array_equal(px["local_idx"], py["local_idx"])


# ------------------------------------------------------------------------------- 8 pairs, kernels, maps against the reference
# workgroup edges of the flattened grids: k_match_layers 64 points, k_accum_layers 1024, k_cov_accum_layers 256
_EDGE_SIZES = [0, 63, 257, 1025, 0, 1023, 65, 0]


def _eight(shape):
    """8 pairs (the maximum) of distinct sizes on the grid edges, empty ones first, in the middle and last; four maps, two of
    them shared by three pairs each; non-integer and zero weights; angular terms on pairs 0, 2, 5 and 6."""
    w = shape.w
    b = _base(w.sigma, 40)
    spec, weights = [], [1.0, 0.37, 2.9, 0.0, 1.0, 1.3, 0.37, 2.9]
    maps = ["near", "far", "trunc", "near", "far", "ndt", "far", "near"]
    angs = [0.4, 0.0, 0.3, 0.0, 0.0, 0.5, 1.0, 0.0]
    for i, n in enumerate(_EDGE_SIZES):
        key = shape.add_scan("edge%d" % i, w.scan_xyz[(97 * i) % 500:][:n])
        spec.append((maps[i], key, (1.2 + 0.15 * i) * b, angs[i]))
    return spec, weights, 0.5 * b


def test_eight_pairs_on_grid_edges_match_the_reference(oracle, shape):
    w = shape.w
    spec, weights, kp = _eight(shape)
    r = capi.icp_align_layers(_pairs(shape, spec, weights), w.T_guess, _params(40, kp), want_pairs=True)
    o = _reference(oracle, shape, spec, w.T_guess, 40, kp, weights=weights)
    _assert_matches_reference(r, o)
    assert [r["pair_counts"][i] for i in (0, 4, 7)] == [0, 0, 0]
    assert all(c > 0 for i, c in enumerate(r["pair_counts"]) if _EDGE_SIZES[i])


@pytest.mark.parametrize("kernel", range(6))
@pytest.mark.parametrize("inner", [1, 3])
def test_every_robust_kernel_and_inner_count_match_the_reference(oracle, shape, kernel, inner):
    """k_accum_layers takes the robust kernel from each pair's MatchK; the angular term sits on pairs 0 and 2."""
    w = shape.w
    b = _base(w.sigma, 30)
    spec = [("near", "near", 2.0 * b, 0.2), ("far", "far", 1.5 * b + 0.2, 0.0), ("far", "near", np.full(30, 1.1), 0.6)]
    weights = [1.0, 0.6, 1.7]
    prior = _prior(w) if kernel % 2 else None
    r = capi.icp_align_layers(_pairs(shape, spec, weights), w.T_guess, _params(30, 0.5 * b, inner=inner, kernel=kernel),
                              prior=prior, want_pairs=True)
    o = _reference(oracle, shape, spec, w.T_guess, 30, 0.5 * b, weights=weights, prior=prior, inner=inner, kernel=kernel)
    _assert_matches_reference(r, o)


@pytest.mark.parametrize("key", ["ndt", "trunc"])
def test_ndt_and_trunc_maps(ctx, oracle, shape, monkeypatch, key):
    """As one pair: bitwise mh_icp_align under MH_MATCH=f.  In a mix of pairs: the reference."""
    w = shape.w
    b = _base(w.sigma, 30)
    p = _params(30, 0.5 * b)
    one = capi.icp_align_layers([dict(map=shape.maps[key], scan=shape.scans["far"], threshold=2.0 * b, threshold_angular_deg=0.3,
                                      weight=1.7)], w.T_guess, p, want_pairs=True)
    monkeypatch.setenv("MH_MATCH", "f")
    from dataclasses import replace
    ref = capi.icp_align(shape.maps[key], shape.scans["far"], w.T_guess,
                         replace(p, threshold=2.0 * b, threshold_angular_deg=0.3,
                                 gn=capi.GNParams(max_inner_iterations=2, weight_pt2pt=1.7)), want_pairs=True)
    monkeypatch.delenv("MH_MATCH")
    _assert_bitwise(one, ref, single=True)
    spec = [(key, "near", 2.0 * b, 0.0), ("far", "far", 1.5 * b + 0.2, 0.3), (key, "far", 1.8 * b, 0.2)]
    r = capi.icp_align_layers(_pairs(shape, spec, [0.8, 1.0, 2.2]), w.T_guess, p, want_pairs=True)
    o = _reference(oracle, shape, spec, w.T_guess, 30, 0.5 * b, weights=[0.8, 1.0, 2.2])
    _assert_matches_reference(r, o)


# ----------------------------------------------------------------------------------------------------- exact identities
def _assert_bitwise(a, b, single=False):
    for k in ("T", "cov"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    for k in ("n_iterations", "termination_reason", "n_final_pairs", "potential_pairings", "quality"):
        assert a[k] == b[k], k
    assert [t["n_pairs"] for t in a["trace"]] == [t["n_pairs"] for t in b["trace"]]
    for x, y in zip(a["trace"], b["trace"]):
        np.testing.assert_array_equal(x["T"], y["T"])
    pa, pb = (a["pairs"], [b["pairs"]]) if single else (a["pairs"], b["pairs"])
    if single:
        assert a["pair_counts"] == [b["n_final_pairs"]]
    else:
        assert a["pair_counts"] == b["pair_counts"]
    for x, y in zip(pa, pb):
        for k in ("local_idx", "global_idx", "global_xyz", "d2"):
            np.testing.assert_array_equal(x[k], y[k], err_msg=k)


def _split_check(ctx, m, xyz, cuts, T0, thr, kp, weight):
    """One scan cut into contiguous pieces at `cuts` = the same map, schedule and weight once per piece: the pairings are the
    one-pair alignment's (concatenated, local indices offset), the loop ends at the same iteration for the same reason, the pose
    agrees to the summation order."""
    edges = [0] + list(cuts) + [len(xyz)]
    pieces = [capi.Scan(ctx, xyz[a:b]) for a, b in zip(edges[:-1], edges[1:])]
    p = _params(len(kp), kp)
    whole = capi.icp_align_layers([dict(map=m, scan=capi.Scan(ctx, xyz), threshold=thr, weight=weight)], T0, p, want_pairs=True)
    cut = capi.icp_align_layers([dict(map=m, scan=s, threshold=thr, weight=weight) for s in pieces], T0, p, want_pairs=True)
    assert whole["n_final_pairs"] > 0
    for k in ("n_iterations", "termination_reason", "n_final_pairs", "potential_pairings", "quality"):
        assert cut[k] == whole[k], k
    assert [t["n_pairs"] for t in cut["trace"]] == [t["n_pairs"] for t in whole["trace"]]
    li = np.concatenate([pp["local_idx"] + np.uint32(a) for pp, a in zip(cut["pairs"], edges)])
    np.testing.assert_array_equal(li, whole["pairs"][0]["local_idx"])
    for k in ("global_idx", "d2"):
        np.testing.assert_array_equal(np.concatenate([pp[k] for pp in cut["pairs"]]), whole["pairs"][0][k])
    np.testing.assert_allclose(cut["T"], whole["T"], rtol=0, atol=1e-9)


@pytest.mark.parametrize("cuts", [[63], [64], [65], [1023], [1024], [1025], [63, 1025], [64, 1023, 1500]])
def test_split_scan_equals_one_pair(ctx, shape, cuts):
    w = shape.w
    b = _base(w.sigma, 40)
    _split_check(ctx, shape.maps["far"], w.scan_xyz, cuts, w.T_guess, 2.0 * b, 0.5 * b, 1.6)


def test_split_c2_scan_into_eight_unequal_pieces(ctx):
    w = synth.workload_c2()
    m = capi.Map(ctx, w.voxel_size, w.cap).build(w.map_xyz)
    n = len(w.scan_xyz)
    cuts = sorted({1, 64 * 37 + 1, 1024 * 11 - 1, n // 5, n // 3 + 256, n // 2 + 1, n - 1025})
    assert len(cuts) == 7
    _split_check(ctx, m, w.scan_xyz, cuts, w.T_guess, w.threshold, w.kernel_param, 0.75)


def test_permuted_pairs_permute_the_counts(shape):
    w = shape.w
    spec, weights, kp = _eight(shape)
    base = capi.icp_align_layers(_pairs(shape, spec, weights), w.T_guess, _params(40, kp), want_pairs=True)
    perm = [3, 6, 0, 7, 1, 5, 2, 4]
    r = capi.icp_align_layers(_pairs(shape, [spec[i] for i in perm], [weights[i] for i in perm]), w.T_guess, _params(40, kp),
                              want_pairs=True)
    assert r["pair_counts"] == [base["pair_counts"][i] for i in perm]
    assert r["n_iterations"] == base["n_iterations"] and r["termination_reason"] == base["termination_reason"]
    for j, i in enumerate(perm):
        np.testing.assert_array_equal(r["pairs"][j]["local_idx"], base["pairs"][i]["local_idx"])
    np.testing.assert_allclose(r["T"], base["T"], rtol=0, atol=1e-9)


@pytest.mark.parametrize("ctl", [dict(poll_every=1), dict(poll_every=3), dict(poll_every=7), dict(poll_every=64),
                                 dict(expected_iterations=2), dict(expected_iterations=40), dict(env="MH_NO_GRAPH"),
                                 dict(env="MH_NO_PREV_BOUND")], ids=lambda d: "-".join("%s" % v for v in d.values()))
def test_loop_control_gives_the_bits_of_the_default_run(shape, monkeypatch, ctl):
    w, sh = shape.w, shape
    spec, weights, kp = _eight(sh)
    p = _params(40, kp)
    default = [capi.icp_align_layers(_pairs(sh, spec, weights), w.T_guess, p, want_pairs=True) for _ in range(3)]
    ctl = dict(ctl)
    env = ctl.pop("env", None)
    if env:
        monkeypatch.setenv(env, "1")
    from dataclasses import replace
    for _ in range(3):  # (the second and third calls replay a captured graph unless MH_NO_GRAPH)
        r = capi.icp_align_layers(_pairs(sh, spec, weights), w.T_guess, replace(p, **ctl), want_pairs=True)
        _assert_bitwise(r, default[0])
    for d in default[1:]:
        _assert_bitwise(d, default[0])


def test_single_and_layers_alignments_interleaved_on_one_context(oracle, small_workload):
    """mh_icp_align and mh_icp_align_layers share ctx->graph_exec and the graph candidate: interleaved on one context, each
    result is bitwise the one of a fresh context."""
    w = small_workload

    def runs(sh):
        b = _base(w.sigma, 40)
        spec, weights, kp = _eight(sh)
        p = _params(40, kp)
        single_p = capi.ICPParams(max_iterations=w.n_iters, threshold=w.threshold, kernel_param=w.kernel_param)
        return [lambda: capi.icp_align_layers(_pairs(sh, spec, weights), w.T_guess, p, want_pairs=True),
                lambda: capi.icp_align(sh.maps["far"], sh.scans["far"], w.T_guess, single_p, want_pairs=True),
                lambda: capi.icp_align_layers(_pairs(sh, spec[:3], weights[:3]), w.T_guess, p, want_pairs=True),
                lambda: capi.icp_align(sh.maps["near"], sh.scans["near"], w.T_guess,
                                       capi.ICPParams(max_iterations=40, threshold=2.0 * b, kernel_param=0.5 * b), want_pairs=True)]

    fresh = [runs(_Shape(capi.Context(0), oracle, w))[i]() for i in range(4)]
    shared = runs(_Shape(capi.Context(0), oracle, w))
    for order in ([0, 1, 2, 3], [1, 0, 0, 3, 2, 1, 2, 0]):
        for i in order:
            r = shared[i]()
            if i in (0, 2):
                _assert_bitwise(r, fresh[i])
            else:
                _assert_single_bitwise(r, fresh[i])


def _assert_single_bitwise(a, b):
    for k in ("T", "cov"):
        np.testing.assert_array_equal(a[k], b[k])
    for k in ("n_iterations", "termination_reason", "n_final_pairs"):
        assert a[k] == b[k], k
    for k in ("local_idx", "global_idx", "d2"):
        np.testing.assert_array_equal(a["pairs"][k], b["pairs"][k])


def test_skip_with_distinct_scans_equals_pair_again(shape):
    """matched_points = SKIP only matters for a scan shared by two pairs (and is refused then): with distinct scans it is
    PAIR_AGAIN bit for bit."""
    w = shape.w
    spec, weights, kp = _eight(shape)
    p = _params(40, kp)
    from dataclasses import replace
    a = capi.icp_align_layers(_pairs(shape, spec, weights), w.T_guess, p, want_pairs=True)
    b = capi.icp_align_layers(_pairs(shape, spec, weights), w.T_guess, replace(p, matched_points=1), want_pairs=True)
    _assert_bitwise(b, a)


# ------------------------------------------------------------------------------------------------------------- host layer
_ICP_HEAD = """
class_name: mp2p_icp::ICP
params:
  maxIterations: 40
  minAbsStep_trans: 1e-4
  minAbsStep_rot: 5e-5
solvers:
  - class: mp2p_icp::Solver_GaussNewton
    params:
      maxIterations: 2
      robustKernel: 'RobustKernel::GemanMcClure'
      robustKernelParam: '0.5*max(ADAPTIVE_THRESHOLD_SIGMA, 2.0*ADAPTIVE_THRESHOLD_SIGMA-(2.0*ADAPTIVE_THRESHOLD_SIGMA-0.5*ADAPTIVE_THRESHOLD_SIGMA)*ICP_ITERATION/30)'
matchers:
"""
_MATCHER = """  - class: mp2p_icp::Matcher_Points_DistanceThreshold
    params:
      threshold: '%s'
      thresholdAngularDeg: 0
      pairingsPerPoint: 1
      allowMatchAlreadyMatchedGlobalPoints: true
      pointLayerMatches:
%s"""
_QUALITY = """quality:
  - class: mp2p_icp::QualityEvaluator_PairedRatio
    params:
      ~
"""


def _entries(pairs):
    return "".join('        - {global: "%s", local: "%s", weight: %s}\n' % (gl + (1.0,))[:3] for gl in pairs)


DUAL_MAP = _ICP_HEAD + _MATCHER % ("3.0*ADAPTIVE_THRESHOLD_SIGMA", _entries([("localmap", "decimated_for_icp")])) + \
    _MATCHER % ("2.0*ADAPTIVE_THRESHOLD_SIGMA", _entries([("localmap_far", "decimated_for_icp_near")])) + _QUALITY
EDGES = _ICP_HEAD + _MATCHER % ("2.0*max(ADAPTIVE_THRESHOLD_SIGMA, 2.0*ADAPTIVE_THRESHOLD_SIGMA-ICP_ITERATION/20)",
                                _entries([("localmap", "decimated_for_icp"), ("localmap_far", "decimated_for_icp_near")])) + _QUALITY


THREE_WEIGHTED = _ICP_HEAD + (_MATCHER % ("2.0*ADAPTIVE_THRESHOLD_SIGMA", _entries([
    ("localmap", "decimated_for_icp", 0.5), ("localmap_far", "decimated_for_icp_near", 1.0),
    ("localmap", "decimated_for_icp_near", 2.0)]))).replace("thresholdAngularDeg: 0\n", "thresholdAngularDeg: 0.2\n") + _QUALITY


@pytest.fixture(scope="module")
def hl():
    capi.lib()
    from mola_lidar_odometry_amd import _mp2p_icp_hip
    return _mp2p_icp_hip


@pytest.mark.parametrize("text", [DUAL_MAP, EDGES], ids=["dual-map", "edges"])
def test_host_layer_fused_layers_equal_its_generic_loop(hl, oracle, small_workload, text):
    """... and BOTH routes equal the float64 reference the chain oracle driver aligns with (oracle/layers_oracle.py)."""
    w = small_workload
    near_l, far_l, near_g, far_g = _split(w)
    g = hl.metric_map_t()
    for name, pts, vs in (("localmap", w.map_xyz, 1.0), ("localmap_far", far_g, 0.5)):
        hv = hl.HashedVoxelPointCloud(vs, 20)
        hv.setPoints(pts)
        g.set_layer(name, hv)
    l = hl.metric_map_t()
    l.set_layer("decimated_for_icp", hl.PointCloud(w.scan_xyz))
    l.set_layer("decimated_for_icp_near", hl.PointCloud(near_l))
    out = {}
    for generic in (False, True):
        icp, params = hl.icp_pipeline_from_yaml(hl.Config.FromYamlText(text))
        src = hl.ParameterSource()
        src.updateVariable("ADAPTIVE_THRESHOLD_SIGMA", w.sigma)
        src.updateVariable("ICP_ITERATION", 0)
        icp.attachToParameterSource(src)
        src.realize()
        icp.forceGenericPath(generic)
        assert icp.alignPath() == ("generic" if generic else "layers")
        res = icp.align(l, g, hl.TPose3D(*w.guess_ypr), params)
        assert icp.lastAlignUsedFusedPath() == (not generic)
        out[generic] = res
    a, b = out[False], out[True]
    assert a.nIterations == b.nIterations and a.terminationReason.name == b.terminationReason.name
    assert a.n_pairs() == b.n_pairs()
    np.testing.assert_allclose(a.pose(), b.pose(), rtol=0, atol=1e-7)
    assert a.quality == pytest.approx(b.quality, abs=1e-12)
    omaps = {"localmap": oracle.Map(1.0, 20).insert(w.map_xyz), "localmap_far": oracle.Map(0.5, 20).insert(far_g)}
    k = np.arange(40)
    thr = ([np.full(40, 3.0 * w.sigma), np.full(40, 2.0 * w.sigma)] if text is DUAL_MAP else
           [2.0 * np.maximum(w.sigma, 2.0 * w.sigma - k / 20.0)] * 2)
    pairs = [dict(map=omaps["localmap"], local=w.scan_xyz, threshold=thr[0], weight=1.0),
             dict(map=omaps["localmap_far"], local=near_l, threshold=thr[1], weight=1.0)]
    o = layers_oracle.icp_align_layers(pairs, synth.pose_from_ypr(w.guess_ypr), oracle.ICPParams(
        max_iterations=40, kernel_param=0.5 * _base(w.sigma, 40), gn=oracle.GNParams(max_inner_iterations=2)))
    assert layers_oracle.nearest_decision(o["margins"])[1] > 1e-9 and o["max_cond"] < 1e10  # (a comparable alignment)
    for res in (a, b):
        assert res.nIterations == o["n_iterations"] and res.terminationReason.name == capi.TERM_NAMES[o["termination_reason"]]
        assert res.n_pairs() == o["n_final_pairs"] > 0
        assert res.quality == pytest.approx(o["quality"], abs=1e-12)
        np.testing.assert_allclose(res.pose(), o["T"], rtol=0, atol=1e-7)


def test_host_layer_three_weighted_entries_match_the_reference(hl, oracle, small_workload):
    """Three pointLayerMatches entries of weights 0.5 / 1 / 2 with thresholdAngularDeg 0.2.  The host layer's generic loop solves
    with one weight per kind of pair and refuses such a pairing set (Pairings::pt2pt_weight), so the fused result is checked
    against the float64 reference instead."""
    w = small_workload
    near_l, far_l, near_g, far_g = _split(w)
    g = hl.metric_map_t()
    for name, pts, vs in (("localmap", w.map_xyz, 1.0), ("localmap_far", far_g, 0.5)):
        hv = hl.HashedVoxelPointCloud(vs, 20)
        hv.setPoints(pts)
        g.set_layer(name, hv)
    l = hl.metric_map_t()
    l.set_layer("decimated_for_icp", hl.PointCloud(w.scan_xyz))
    l.set_layer("decimated_for_icp_near", hl.PointCloud(near_l))
    res = {}
    for generic in (False, True):
        icp, params = hl.icp_pipeline_from_yaml(hl.Config.FromYamlText(THREE_WEIGHTED))
        src = hl.ParameterSource()
        src.updateVariable("ADAPTIVE_THRESHOLD_SIGMA", w.sigma)
        src.updateVariable("ICP_ITERATION", 0)
        icp.attachToParameterSource(src)
        src.realize()
        icp.forceGenericPath(generic)
        if generic:
            with pytest.raises(RuntimeError, match="different weights"):
                icp.align(l, g, hl.TPose3D(*w.guess_ypr), params)
        else:
            assert icp.alignPath() == "layers"
            res = icp.align(l, g, hl.TPose3D(*w.guess_ypr), params)
            assert icp.lastAlignUsedFusedPath()
    omaps = {"localmap": oracle.Map(1.0, 20).insert(w.map_xyz), "localmap_far": oracle.Map(0.5, 20).insert(far_g)}
    thr = np.full(40, 2.0 * w.sigma)
    pairs = [dict(map=omaps[gk], local=loc, threshold=thr, threshold_angular_deg=0.2, weight=wt)
             for gk, loc, wt in (("localmap", w.scan_xyz, 0.5), ("localmap_far", near_l, 1.0), ("localmap", near_l, 2.0))]
    o = layers_oracle.icp_align_layers(pairs, synth.pose_from_ypr(w.guess_ypr), oracle.ICPParams(
        max_iterations=40, kernel_param=0.5 * _base(w.sigma, 40), gn=oracle.GNParams(max_inner_iterations=2)))
    assert res.nIterations == o["n_iterations"] and res.terminationReason.name == capi.TERM_NAMES[o["termination_reason"]]
    assert res.n_pairs() == o["n_final_pairs"] > 0
    assert res.quality == pytest.approx(o["quality"], abs=1e-12)
    np.testing.assert_allclose(res.pose(), o["T"], rtol=0, atol=1e-7)


def test_host_layer_layers_schedule_precomputed_and_refreshed(hl, small_workload):
    """precomputeSchedule() covers the multi-layer shapes too: an alignment after it equals one without it, and a schedule
    computed for one value of the variables is not reused after the variable changes."""
    w = small_workload
    near_l, far_l, near_g, far_g = _split(w)
    g = hl.metric_map_t()
    for name, pts, vs in (("localmap", w.map_xyz, 1.0), ("localmap_far", far_g, 0.5)):
        hv = hl.HashedVoxelPointCloud(vs, 20)
        hv.setPoints(pts)
        g.set_layer(name, hv)
    l = hl.metric_map_t()
    l.set_layer("decimated_for_icp", hl.PointCloud(w.scan_xyz))
    l.set_layer("decimated_for_icp_near", hl.PointCloud(near_l))

    def run(sigma, precompute_at=None):
        icp, params = hl.icp_pipeline_from_yaml(hl.Config.FromYamlText(DUAL_MAP))
        src = hl.ParameterSource()
        src.updateVariable("ICP_ITERATION", 0)
        icp.attachToParameterSource(src)
        if precompute_at is not None:
            src.updateVariable("ADAPTIVE_THRESHOLD_SIGMA", precompute_at)
            src.realize()
            icp.precomputeSchedule(params.maxIterations)
        src.updateVariable("ADAPTIVE_THRESHOLD_SIGMA", sigma)
        src.realize()
        res = icp.align(l, g, hl.TPose3D(*w.guess_ypr), params)
        assert icp.lastAlignUsedFusedPath()
        return res

    plain, pre, stale = run(w.sigma), run(w.sigma, precompute_at=w.sigma), run(w.sigma, precompute_at=0.5 * w.sigma)
    for r in (pre, stale):
        assert r.nIterations == plain.nIterations and r.n_pairs() == plain.n_pairs()
        np.testing.assert_array_equal(r.pose(), plain.pose())
