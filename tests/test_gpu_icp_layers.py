"""mh_icp_align_layers on the device: one ICP alignment over several Matcher_Points_DistanceThreshold (map, scan) pairs with one
Gauss-Newton solve (the ICP blocks of the reference's pipelines/extras/lidar3d-dual-map.yaml and lidar3d-edges.yaml).

Checked against mh_icp_align for one pair, against a loop written with the oracle's matcher and solver for two and three pairs,
and through the host layer against its matcher-by-matcher loop."""
import numpy as np
import pytest

from mola_lidar_odometry_amd import capi, synth

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
        self.maps = {"near": capi.Map(ctx, 0.5, 20).build(near_g), "far": capi.Map(ctx, 1.0, 20).build(far_g)}
        self.omaps = {"near": oracle.Map(0.5, 20).insert(near_g), "far": oracle.Map(1.0, 20).insert(far_g)}
        self.scans = {"near": capi.Scan(ctx, self.near_l), "far": capi.Scan(ctx, self.far_l)}
        self.locs = {"near": self.near_l, "far": self.far_l}


@pytest.fixture(scope="module")
def shape(ctx, oracle, small_workload):
    return _Shape(ctx, oracle, small_workload)


def _base(sigma, n):
    k = np.arange(n, dtype=np.float64)
    return np.maximum(sigma, 2.0 * sigma - (2.0 * sigma - 0.5 * sigma) * k / 30.0)


def _oracle_loop(oracle, sh, spec, T0, max_it, kp, weight=1.0, prior=None, hook=None, inner=2):
    """spec: [(map key, scan key, thr[max_it], angular deg)]; the semantics of mh_icp_align_layers with every pair at `weight`."""
    T, Tprev, term, it = T0.copy(), T0.copy(), "MaxIterations", 0
    last = None
    for it in range(max_it):
        lp, gp, per = [], [], []
        for mk, sk, thr, ang in spec:
            r = oracle.match_points(sh.omaps[mk], sh.locs[sk], T, thr[it], ang)
            lp.append(sh.locs[sk][r["local_idx"]])
            gp.append(r["global_xyz"])
            per.append(r["local_idx"])
        last = (lp, gp, per)
        if sum(len(a) for a in lp) == 0:
            term = "NoPairings"
            break
        T = oracle.gn_solve(T, pt2pt=(np.concatenate(lp), np.concatenate(gp)),
                            params=oracle.GNParams(max_inner_iterations=inner, robust_kernel_param=kp[it], weight_pt2pt=weight),
                            prior=prior)[0]
        d = oracle.se3_log(oracle.pose_compose(oracle.pose_inverse(Tprev), T))
        if np.linalg.norm(d[:3]) < 1e-4 and np.linalg.norm(d[3:]) < 5e-5:
            term = "Stalled"
            break
        if hook is not None:
            chk, ht, hr = hook
            S = oracle.pose_compose(oracle.pose_inverse(chk), T)
            e = oracle.se3_log(S)
            if np.linalg.norm(np.reshape(S, (3, 4))[:, 3]) > ht or np.linalg.norm(e[3:]) > hr:
                term = "HookRequest"
                break
        Tprev = T.copy()
    else:
        it = max_it
    return dict(T=T, term=term, it=it, last=last)


def _pairs(sh, spec, weights=None):
    return [dict(map=sh.maps[mk], scan=sh.scans[sk], threshold=thr, threshold_angular_deg=ang,
                 weight=1.0 if weights is None else weights[i]) for i, (mk, sk, thr, ang) in enumerate(spec)]


def _params(max_it, kp, **kw):
    return capi.ICPParams(max_iterations=max_it, kernel_param=kp, threshold=1.0, gn=capi.GNParams(max_inner_iterations=2), **kw)


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
    o = _oracle_loop(oracle, shape, spec, w.T_guess, 40, kp)
    assert capi.TERM_NAMES[r["termination_reason"]] == o["term"]
    assert r["n_iterations"] == o["it"]
    lp, gp, per = o["last"]
    n_pairs = sum(len(a) for a in lp)
    potential = sum(len(shape.locs[sk]) for _, sk, _, _ in spec)
    assert r["n_final_pairs"] == n_pairs and r["potential_pairings"] == potential
    assert r["quality"] == pytest.approx(n_pairs / potential, abs=1e-12)
    assert r["pair_counts"] == [len(a) for a in per]
    for i in range(n):
        np.testing.assert_array_equal(r["pairs"][i]["local_idx"], per[i])
    np.testing.assert_allclose(r["T"], o["T"], rtol=0, atol=1e-7)
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
    o = _oracle_loop(oracle, shape, spec, w.T_guess, 40, kp, weight=3.0, prior=prior)
    assert capi.TERM_NAMES[r3["termination_reason"]] == o["term"] and r3["n_iterations"] == o["it"]
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
    o = _oracle_loop(oracle, shape, spec, w.T_guess, 40, kp, hook=(w.T_guess, 0.2, np.deg2rad(0.5)))
    assert o["term"] == "HookRequest"
    assert capi.TERM_NAMES[r["termination_reason"]] == "HookRequest" and r["n_iterations"] == o["it"]
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
    return "".join('        - {global: "%s", local: "%s", weight: 1.0}\n' % gl for gl in pairs)


DUAL_MAP = _ICP_HEAD + _MATCHER % ("3.0*ADAPTIVE_THRESHOLD_SIGMA", _entries([("localmap", "decimated_for_icp")])) + \
    _MATCHER % ("2.0*ADAPTIVE_THRESHOLD_SIGMA", _entries([("localmap_far", "decimated_for_icp_near")])) + _QUALITY
EDGES = _ICP_HEAD + _MATCHER % ("2.0*max(ADAPTIVE_THRESHOLD_SIGMA, 2.0*ADAPTIVE_THRESHOLD_SIGMA-ICP_ITERATION/20)",
                                _entries([("localmap", "decimated_for_icp"), ("localmap_far", "decimated_for_icp_near")])) + _QUALITY


@pytest.fixture(scope="module")
def hl():
    capi.lib()
    from mola_lidar_odometry_amd import _mp2p_icp_hip
    return _mp2p_icp_hip


@pytest.mark.parametrize("text", [DUAL_MAP, EDGES], ids=["dual-map", "edges"])
def test_host_layer_fused_layers_equal_its_generic_loop(hl, small_workload, text):
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
