"""-m gpu: the solver's scalar parameters off their defaults, per kernel family.

mh_gn_params::weight_pt2pt / weight_pt2pl and mh_icp_params::cov_findif_xyz / cov_findif_ang are read at many kernel and host
sites, and every stock pipeline leaves them at 1.0 and 1e-7: a weight dropped or two steps swapped in ONE kernel family passes
every other test.  Here every family that reads them runs with values that differ from the defaults and from each other --
against the CPU oracle with the same values (poses at POSE_TOL of tests/test_gpu_parity.py, pairings bit for bit, covariance
at 2e-5) and, for the covariance, against the closed form of the Jacobian (oracle/icp_oracle_np.py::covariance_analytic) at
the bound measured in tests/test_oracle_gn.py (tests/cov_cases.py).  A weight alone scales H and g alike and cancels in the step: every weight case
pairs it with plane pairings or a prior and asserts FROM THE ORACLE ALONE that the weighted pose lies more than 1e-4 (1000
POSE_TOL) from the unit-weight pose, so no case can pass because its parameter does not matter."""
import functools
import importlib.util
import os
from dataclasses import replace
from types import SimpleNamespace

import numpy as np
import pytest

from cov_cases import COV_FD_BOUND, COV_KINDS, COV_POSES, cov_inputs, scaled_gap
from mola_lidar_odometry_amd import capi, synth
from oracle import icp_oracle_np as onp
from route_tables import PLANE_MATCHER_KERNELS, POINT_MATCHER_KERNELS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _module(name):
    spec = importlib.util.spec_from_file_location("_" + name, os.path.join(ROOT, "tests", name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


# The fused-alignment helpers stay where the parity tests define them (the comparison of an alignment with the oracle has ONE
# definition); loaded by path under a private name like tests/test_gpu_icp_layers_batch.py does, so nothing of it is collected here.
_parity = _module("test_gpu_parity")
_params, assert_align_equal, I12 = _parity._params, _parity.assert_align_equal, _parity.I12

OBSERVABLE = 1e-4                                   # 1000 x POSE_TOL
W = SimpleNamespace(sigma=0.5, n_iters=60)          # the schedule of test_align_ndt_pipeline_matches_oracle
NDT_ARGS, PLAIN_ARGS = (1.0, 0, 0, 0.1, 0.05, 4), (1.0, 20)
GUESS = [0.12, -0.09, 0.06, 0.006, -0.004, 0.01]
LAM = np.diag([200.0, 200.0, 200.0, 2000.0, 2000.0, 2000.0])
STEPS = (1e-7, 0.05)                                # (findif_xyz, findif_ang): distinct, the angular truncation term visible
DIAG1E6 = np.eye(6) * 1e6


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


# ---------------------------------------------------------------------------- workloads (NDT and plain map of one cloud)
@functools.lru_cache(maxsize=None)
def _cloud():
    return synth.ndt_cloud(11)


@functools.lru_cache(maxsize=None)
def _scan(n, seed=12):
    pts = _cloud()
    rng = np.random.default_rng(seed)
    if n <= len(pts) and seed == 12:
        return pts[rng.permutation(len(pts))[:n]]
    return (pts[rng.integers(0, len(pts), n)] + rng.normal(0, 0.01, (n, 3)).astype(np.float32)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _guess(variant=0):
    return synth.pose_from_ypr(np.array(GUESS) + [0.02 * variant, -0.01 * variant, 0.0, 0.001 * variant, 0.0, 0.0])


_dev_maps = {}


def _map(ctx, ndt):
    key = (id(ctx), ndt)
    if key not in _dev_maps:
        _dev_maps[key] = capi.Map(ctx, *(NDT_ARGS if ndt else PLAIN_ARGS)).build(_cloud())
    return _dev_maps[key]


@functools.lru_cache(maxsize=None)
def _omap(oracle, ndt):
    return oracle.Map(*(NDT_ARGS if ndt else PLAIN_ARGS)).insert(_cloud())


def _p(mod, ndt, w, inner=2, skip=False, **extra):
    """ICPParams of `mod` (capi | the oracle): NDT map = the lidar3d-ndt block (both matchers), plain map = the point matcher."""
    kw = dict(gn=mod.GNParams(max_inner_iterations=inner, weight_pt2pt=w[0], weight_pt2pl=w[1]), **extra)
    if ndt:
        kw.update(min_abs_step_trans=5e-4, min_abs_step_rot=5e-4, pt2pl_threshold=0.5)
    if skip:
        kw.update(matched_points=1) if mod is capi else kw.update(pt2pt_skip_plane_paired=True)
    return _params(mod, W, **kw)


def _prior(ndt, variant=0):
    return None if ndt else (_guess(variant), LAM)  # a point weight is observable only next to a prior (or plane pairings)


@functools.lru_cache(maxsize=None)
def _oracle_align(oracle, ndt, n, w, inner=2, skip=False, seed=12, variant=0):
    return oracle.icp_align(_omap(oracle, ndt), _scan(n, seed), _guess(variant), _p(oracle, ndt, w, inner, skip),
                            prior=_prior(ndt, variant), want_pairs=True)


def _oracle_pair(oracle, ndt, n, w, **kw):
    """The oracle's run with weights `w` -- and the proof, from the oracle alone, that they matter on this input."""
    o, unit = _oracle_align(oracle, ndt, n, w, **kw), _oracle_align(oracle, ndt, n, (1.0, 1.0), **kw)
    shift = float(np.abs(o["T"] - unit["T"]).max())
    print("oracle: ndt=%d n=%d w=%s %s: pose shift against unit weights %.3e" % (ndt, n, w, kw, shift))
    assert shift > OBSERVABLE, shift
    return o


def _assert_matches(g, o):
    assert_align_equal(g, o)
    assert g["n_final_pairs_pt2pl"] == o["n_final_pairs_pt2pl"]
    for k in ("local_idx", "global_idx", "global_xyz"):
        np.testing.assert_array_equal(g["pairs"][k], o["pairs"][k])
    np.testing.assert_allclose(g["cov"], o["cov"], rtol=2e-5, atol=1e-6 * np.abs(o["cov"]).max())


def _setenv(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)


# ---------------------------------------------------------------------------- plane weight: every kernel that runs the plane matcher
@pytest.mark.parametrize("n,env,inner,skip", PLANE_MATCHER_KERNELS)   # (tests/route_tables.py: the kernel of every row)
def test_plane_weight_through_every_plane_matcher(ctx, oracle, n, env, inner, skip, monkeypatch):
    """NDT map, weights (0.25, 3.0) on (point rows, plane rows): Matcher_Point2Plane's rows are weighted at five kernel sites
    (k_icp16<true>, k_step16<true>, k_icp16_b<true>, k_accum_both, k_match_pl's fused first step -- the `FUSED` of
    mh_k_match_rows.h:132 is k_match_pl's; on an NDT layer plan_alignment never fuses the ROW kernel's first step, so there is
    no k_match16<true, true> to reach).  Which kernel a case runs follows from plan_alignment (csrc/mh_icp.hip) and is
    confirmed by the one-line mutants of DESIGN.md section 5: each is caught by the case named for its kernel."""
    w = (0.25, 3.0)
    o = _oracle_pair(oracle, True, n, w, inner=inner, skip=skip)
    _setenv(monkeypatch, env)
    s0, a0 = capi.loop_stats()
    g = capi.icp_align(_map(ctx, True), capi.Scan(ctx, _scan(n)), _guess(), _p(capi, True, w, inner, skip), want_pairs=True)
    s1, a1 = capi.loop_stats()
    if n <= 2560 and not env:
        assert s1 - s0 == 1 and a1 == a0   # the one-launch loop ran and was not abandoned
    elif env.get("MH_NO_LOOP16") or n > 2560:
        assert (s1, a1) == (s0, a0)
    _assert_matches(g, o)
    assert g["n_final_pairs_pt2pl"] > n // 5


# ---------------------------------------------------------------------------- point weight: every family of the point matcher
@pytest.mark.parametrize("n,env", POINT_MATCHER_KERNELS)               # (tests/route_tables.py: the family of every row)
@pytest.mark.parametrize("wpt", [0.25, 4.0])
def test_point_weight_next_to_a_prior_through_every_family(ctx, oracle, n, env, wpt, monkeypatch):
    """Plain map, a prior of information diag(200, 200, 200, 2000, 2000, 2000) at the guess, weight_pt2pt in {0.25, 4}: the
    weight sets the point rows against the prior factor in every kernel that sums them."""
    w = (wpt, 1.0)
    o = _oracle_pair(oracle, False, n, w)
    _setenv(monkeypatch, env)
    s0, a0 = capi.loop_stats()
    g = capi.icp_align(_map(ctx, False), capi.Scan(ctx, _scan(n)), _guess(), _p(capi, False, w), prior=_prior(False),
                       want_pairs=True)
    s1, a1 = capi.loop_stats()
    if (n <= 2560 and not env) or env.get("MH_LOOPW") == "all":
        assert s1 - s0 == 1 and a1 == a0   # k_icp16 / k_icpw ran and was not abandoned
    else:
        assert (s1, a1) == (s0, a0)
    _assert_matches(g, o)


# ---------------------------------------------------------------------------- lock-step batches: every job its own weights
PLAIN_W = [(0.25, 1.0), (4.0, 1.0), (1.0, 1.0), (0.25, 1.0)]
NDT_W = [(0.25, 3.0), (1.0, 3.0), (0.25, 1.0), (1.0, 1.0)]
SMALL = (1500, 900, 2048, 700)


@pytest.mark.parametrize("ndt,sizes,env,loops", [
    (False, SMALL, {}, True),                                    # k_icpw_b
    (False, SMALL, {"MH_LOOPW": "none"}, True),                  # k_icp16_b<false>
    (True, SMALL, {}, True),                                     # k_icp16_b<true>
    (False, SMALL, {"MH_NO_LOOP16_BATCH": "1"}, False),          # k_step16_b, launch by launch
    (True, SMALL, {"MH_NO_LOOP16_BATCH": "1"}, False),
    (False, (5000, 5000, 4000, 5000), {}, False),                # row kernel
    (True, (5000, 5000, 4000, 5000), {}, False),
    (False, (5000, 5000, 4000, 5000), {"MH_NO_STEP_CHAIN": "1"}, False),
    (True, (5000, 5000, 4000, 5000), {"MH_NO_STEP_CHAIN": "1"}, False),
    (False, (40000, 36000, 40000), {}, False),                   # plan / scan matcher
    (True, (40000, 36000, 40000), {}, False),                    # k_match_pl
    (False, (9000, 5000, 9000), {"MH_MATCH": "q"}, False),       # quad matcher
])
def test_lockstep_batch_jobs_with_their_own_weights(ctx, oracle, ndt, sizes, env, loops, monkeypatch):
    """mh_icp_align_batch with one mh_icp_params per job: the jobs of one lock-step group carry DIFFERENT weights (a kernel
    that reads the group leader's, or job 0's, fails here).  Every job: the bits of its solo run, and the oracle's result."""
    weights = (NDT_W if ndt else PLAIN_W)[:len(sizes)]
    refs = [(_oracle_pair if w != (1.0, 1.0) else _oracle_align)(oracle, ndt, n, w, seed=100 + k, variant=k)
            for k, (n, w) in enumerate(zip(sizes, weights))]
    _setenv(monkeypatch, env)
    gm = _map(ctx, ndt)
    ctxs = [capi.Context(0) for _ in sizes]
    subs = [_scan(n, 100 + k) for k, n in enumerate(sizes)]
    guesses = [_guess(k) for k in range(len(sizes))]
    priors = [_prior(ndt, k) for k in range(len(sizes))]
    ps = [_p(capi, ndt, w) for w in weights]
    solo = [capi.icp_align(gm, capi.Scan(ctx, s), g, p, prior=pr, want_trace=False, want_pairs=True)
            for s, g, p, pr in zip(subs, guesses, ps, priors)]
    scans = [capi.Scan(c, s) for c, s in zip(ctxs, subs)]
    block = np.zeros(sum(capi.pairs_block_bytes(n) for n in sizes), np.uint8)
    s0, a0 = capi.loop_stats()
    batch = capi.icp_align_batch([gm] * len(sizes), scans, guesses, ps, priors=None if ndt else priors, pairs_block=block)
    s1, a1 = capi.loop_stats()
    if loops:
        assert s1 - s0 == len(sizes) and a1 == a0  # every job ran as a one-launch loop
    else:
        assert (s1, a1) == (s0, a0)
    for a, b, pr, o in zip(solo, batch, capi.unpack_pairs_block(block, list(sizes), batch), refs):
        assert (a["n_iterations"], a["termination_reason"], a["n_final_pairs"], a["n_final_pairs_pt2pl"]) == (
            b["n_iterations"], b["termination_reason"], b["n_final_pairs"], b["n_final_pairs_pt2pl"])
        np.testing.assert_array_equal(a["T"], b["T"])
        np.testing.assert_array_equal(a["cov"], b["cov"])
        b = dict(b, pairs=pr)
        _assert_matches(b, o)
    for c in ctxs:
        c.close()


# ---------------------------------------------------------------------------- mh_gn_solve
@pytest.mark.parametrize("kernel", [0, 1, 2, 3, 4, 5])
@pytest.mark.parametrize("w", [(0.3, 4.0), (4.0, 0.3)])
def test_gn_solve_with_both_weights_matches_oracle(ctx, oracle, kernel, w):
    """test_gn_solve_matches_oracle with both weights off 1 on point pairs and plane pairs together, every robust kernel."""
    rng = np.random.default_rng(10 + kernel)
    l, q = _parity._pairs(rng, 3001)
    pl = _parity._planes(rng, 777)
    T0 = oracle.se3_exp([0.1, -0.05, 0.02, 0.01, -0.02, 0.005])
    kw = dict(max_inner_iterations=3, robust_kernel=kernel, robust_kernel_param=0.7)
    Tg, ng, ok, sg = capi.gn_solve(ctx, T0, (l, q), pl, capi.GNParams(weight_pt2pt=w[0], weight_pt2pl=w[1], **kw))
    To, no, so = oracle.gn_solve(T0, (l, q), pl, oracle.GNParams(weight_pt2pt=w[0], weight_pt2pl=w[1], **kw))
    _, _, unit = oracle.gn_solve(T0, (l, q), pl, oracle.GNParams(**kw))
    assert np.abs(unit[0]["delta"] - so[0]["delta"]).max() > OBSERVABLE  # (from the oracle alone: the weights matter)
    assert ok and ng == no == 3
    for a, b in zip(sg, so):
        scale = np.abs(b["H"]).max()
        np.testing.assert_allclose(a["H"], b["H"], rtol=1e-10, atol=1e-12 * scale)
        np.testing.assert_allclose(a["g"], b["g"], rtol=1e-9, atol=1e-11 * np.sqrt(scale * b["err_norm_sqr"]))
        np.testing.assert_allclose(a["err_norm_sqr"], b["err_norm_sqr"], rtol=1e-12)
        np.testing.assert_allclose(a["delta"], b["delta"], rtol=1e-7, atol=1e-11)
    np.testing.assert_allclose(Tg, To, atol=1e-11)


# ---------------------------------------------------------------------------- mh_covariance: steps and the closed form
def _closed_form_at_steps(ref, findif_ang):
    """The closed-form covariance a central difference of step findif_ang gives: the difference quotient of a rotation about one
    axis is EXACTLY sin(h) / h times its derivative, so every angular column of A carries that factor (the translational
    columns are linear: any step is exact)."""
    d = np.array([1.0, 1.0, 1.0] + [findif_ang / np.sin(findif_ang)] * 3)
    return ref * np.outer(d, d)


@pytest.mark.parametrize("kind", COV_KINDS)
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 5000])   # (the block is 256 threads)
def test_covariance_steps_and_closed_form(ctx, oracle, kind, n):
    """mh_covariance against the closed form at the default steps (bound: tests/test_oracle_gn.py, scaled by 1 / sqrt(diag)),
    and against the oracle with two pairs of DISTINCT steps (2e-5, scaled alike): swapped or shared steps fail.  Inputs on which
    the oracle finds A^T A singular must come back as diag(1e6) from both."""
    n_singular = 0
    for spread in (10.0, 60.0):
        pp, pl = cov_inputs(kind, n, spread)
        for x in COV_POSES:
            T = onp.T12(onp.pose_from_ypr(x))
            for steps in ((1e-7, 1e-7), STEPS, (1e-3, 1e-7)):
                co, _ = oracle.covariance(T, pp, pl, *steps)
                cg = capi.covariance(ctx, T, pp, pl, *steps)
                if np.array_equal(co, DIAG1E6):
                    n_singular += 1
                    np.testing.assert_array_equal(cg, DIAG1E6)
                    continue
                ref = _closed_form_at_steps(onp.covariance_analytic(onp.T44(T), pp, pl), steps[1])
                gap_ref = scaled_gap(cg, ref)
                print("cov %s n=%d spread=%g pose=%s steps=%s: device vs oracle %.3e, vs closed form %.3e (scaled)" % (
                    kind, n, spread, x[3:], steps, scaled_gap(cg, co), gap_ref))
                s = np.outer(1.0 / np.sqrt(np.diag(ref)), 1.0 / np.sqrt(np.diag(ref)))
                np.testing.assert_allclose(cg * s, co * s, rtol=2e-5, atol=1e-6 * np.abs(co * s).max())
                assert gap_ref < COV_FD_BOUND, (gap_ref, steps)
    rows = n * {"points": 3, "planes": 1, "both": 4}[kind]
    if rows < 6 or (kind == "points" and n == 2):   # fewer rows than unknowns; two points leave the turn about their line free
        assert n_singular == 18                      # rank <= 5 at every spread, pose and step pair
    else:
        assert n_singular == 0


# ---------------------------------------------------------------------------- the fused covariance: every route with its own prepare step
def _final_pairings(scan_xyz, scan, r, ndt):
    pp = (scan_xyz[r["pairs"]["local_idx"]], r["pairs"]["global_xyz"])
    pl = None
    if ndt:
        q = capi.icp_get_pt2pl_pairs(scan)
        assert len(q["local_idx"]) == r["n_final_pairs_pt2pl"] > 0
        pl = (scan_xyz[q["local_idx"]], q["centroid"], q["normal"])
    return pp, pl


def _assert_cov_has_the_steps(ctx, r, r_default, pp, pl):
    """The fused covariance IS mh_covariance of the final pose and pairings at the steps handed in (1e-9, the bar of
    test_covariance_over_the_union_of_final_pairings), the closed form at those steps within the bound, and away from the
    default-step result by the truncation term of the angular step."""
    np.testing.assert_array_equal(r["T"], r_default["T"])
    np.testing.assert_allclose(r["cov"], capi.covariance(ctx, r["T"], pp, pl, *STEPS), rtol=1e-9, atol=0)
    ref = onp.covariance_analytic(onp.T44(r["T"]), pp, pl)
    assert scaled_gap(r["cov"], _closed_form_at_steps(ref, STEPS[1])) < COV_FD_BOUND
    assert scaled_gap(r_default["cov"], ref) < COV_FD_BOUND
    assert 20 * COV_FD_BOUND < scaled_gap(r["cov"], r_default["cov"]) < 1e-3


@pytest.mark.parametrize("ndt,n,env", [(False, 1500, {"MH_NO_LOOP16": "1"}), (True, 1500, {"MH_NO_LOOP16": "1"}),  # launch chain
                                       (False, 1500, {}), (True, 1500, {}),                                          # k_icp16
                                       (False, 3000, {"MH_LOOPW": "all"}),                                           # k_icpw
                                       (False, 5000, {"MH_MATCH": "s", "MH_NO_STEP_CHAIN": "1"}), (False, 40000, {})])
def test_fused_covariance_takes_both_steps(ctx, oracle, ndt, n, env, monkeypatch):
    _setenv(monkeypatch, env)
    xyz = _scan(n)
    scan = capi.Scan(ctx, xyz)
    w = (1.0, 1.0)
    s0, a0 = capi.loop_stats()
    r0 = capi.icp_align(_map(ctx, ndt), scan, _guess(), _p(capi, ndt, w), want_pairs=True)
    r = capi.icp_align(_map(ctx, ndt), scan, _guess(), _p(capi, ndt, w, cov_findif_xyz=STEPS[0], cov_findif_ang=STEPS[1]),
                       want_pairs=True)
    s1, a1 = capi.loop_stats()
    assert (s1 - s0, a1 - a0) == ((2, 0) if (n <= 2560 and not env) or env.get("MH_LOOPW") == "all" else (0, 0))
    pp, pl = _final_pairings(xyz, scan, r, ndt)
    _assert_cov_has_the_steps(ctx, r, r0, pp, pl)
    o = oracle.icp_align(_omap(oracle, ndt), xyz, _guess(), _p(oracle, ndt, w, cov_findif_xyz=STEPS[0], cov_findif_ang=STEPS[1]),
                         want_pairs=True)
    _assert_matches(r, o)


@pytest.mark.parametrize("env", [{}, {"MH_LOOPW": "none"}, {"MH_NO_LOOP16_BATCH": "1"}])
def test_fused_covariance_steps_per_job_of_a_lockstep_batch(ctx, oracle, env, monkeypatch):
    """Jobs of one lock-step group of loops with their own covariance steps: default, (1e-7, 0.05), (1e-3, 1e-7)."""
    _setenv(monkeypatch, env)
    sizes = (1500, 900, 2048)
    steps = ((1e-7, 1e-7), STEPS, (1e-3, 1e-7))
    gm = _map(ctx, False)
    ctxs = [capi.Context(0) for _ in sizes]
    subs = [_scan(n, 100 + k) for k, n in enumerate(sizes)]
    scans = [capi.Scan(c, s) for c, s in zip(ctxs, subs)]
    guesses = [_guess(k) for k in range(len(sizes))]
    base = _p(capi, False, (1.0, 1.0))
    block = np.zeros(sum(capi.pairs_block_bytes(n) for n in sizes), np.uint8)
    default = capi.icp_align_batch([gm] * len(sizes), scans, guesses, [base] * len(sizes))
    ps = [replace(base, cov_findif_xyz=hx, cov_findif_ang=ha) for hx, ha in steps]
    batch = capi.icp_align_batch([gm] * len(sizes), scans, guesses, ps, pairs_block=block)
    for k, (r, r0, pr) in enumerate(zip(batch, default, capi.unpack_pairs_block(block, list(sizes), batch))):
        pp = (subs[k][pr["local_idx"]], pr["global_xyz"])
        np.testing.assert_array_equal(r["T"], r0["T"])
        np.testing.assert_allclose(r["cov"], capi.covariance(ctx, r["T"], pp, None, *steps[k]), rtol=1e-9, atol=0)
        o = oracle.icp_align(_omap(oracle, False), subs[k], guesses[k],
                             _p(oracle, False, (1.0, 1.0), cov_findif_xyz=steps[k][0], cov_findif_ang=steps[k][1]))
        assert_align_equal(r, o)
        np.testing.assert_allclose(r["cov"], o["cov"], rtol=2e-5, atol=1e-6 * np.abs(o["cov"]).max())
        if k == 1:
            _assert_cov_has_the_steps(ctx, r, r0, pp, None)
        else:  # (steps that leave no truncation term: the default result up to rounding)
            assert scaled_gap(r["cov"], r0["cov"]) < 2 * COV_FD_BOUND
    for c in ctxs:
        c.close()


def test_fused_covariance_steps_in_multi_layer_alignments(ctx, oracle):
    """mh_icp_align_layers and mh_icp_align_layers_batch copy the two steps on their own (mh_icp_layers.inl)."""
    sizes = (1500, 900)
    thr, kp = synth.threshold_schedule(W.sigma, W.n_iters)
    base = capi.ICPParams(max_iterations=W.n_iters, kernel_param=kp)
    stepped = replace(base, cov_findif_xyz=STEPS[0], cov_findif_ang=STEPS[1])
    ctxs = [capi.Context(0) for _ in range(2)]
    jobs, singles, pairings = [], [], []
    for j, c in enumerate(ctxs):
        xyz = [_scan(n, 200 + 10 * j + k) for k, n in enumerate(sizes)]
        scans = [capi.Scan(c, x) for x in xyz]
        gm = capi.Map(c, *PLAIN_ARGS).build(_cloud())   # (the maps and scans of a multi-layer alignment share a context)
        pairs = [dict(map=gm, scan=s, threshold=thr * (1.0 + 0.2 * k), weight=1.0 + k) for k, s in enumerate(scans)]
        jobs.append(pairs)
        r0 = capi.icp_align_layers(pairs, _guess(j), base, want_pairs=True)
        r = capi.icp_align_layers(pairs, _guess(j), stepped, want_pairs=True)
        pp = (np.concatenate([x[q["local_idx"]] for x, q in zip(xyz, r["pairs"])]),
              np.concatenate([q["global_xyz"] for q in r["pairs"]]))
        assert all(len(q["local_idx"]) > 100 for q in r["pairs"])
        _assert_cov_has_the_steps(c, r, r0, pp, None)
        singles.append((r, r0))
        pairings.append(pp)
    batch = capi.icp_align_layers_batch(jobs, [_guess(0), _guess(1)], [stepped, base])
    both = capi.icp_align_layers_batch(jobs, [_guess(0), _guess(1)], stepped)
    for j, (r, r0) in enumerate(singles):
        want = r if j == 0 else r0   # job 1 of the per-job batch keeps the default steps
        np.testing.assert_array_equal(batch[j]["T"], want["T"])
        np.testing.assert_array_equal(batch[j]["cov"], want["cov"])
        np.testing.assert_array_equal(both[j]["cov"], r["cov"])
        np.testing.assert_allclose(both[j]["cov"], capi.covariance(ctx, both[j]["T"], pairings[j], None, *STEPS), rtol=1e-9, atol=0)
    for c in ctxs:
        c.close()


# ---------------------------------------------------------------------------- the weights stay out of the covariance
@pytest.mark.parametrize("ndt,n,env", [(False, 1500, {}), (True, 1500, {}), (False, 1500, {"MH_NO_LOOP16": "1"}),
                                       (True, 5000, {}), (False, 3000, {"MH_LOOPW": "all"}), (True, 40000, {}), (False, 40000, {})])
def test_weights_do_not_enter_the_covariance(ctx, oracle, ndt, n, env, monkeypatch):
    """mp2p_icp::covariance [U] takes the pairings, not their weights (include/molahip.h): device and oracle both leave them out.
    Both weights scaled by the same power of two scale H and g exactly, so the step, the poses and the final pairings keep their
    bits -- and so must the covariance (a covariance of the weighted rows would be 4 or 1/4 of it)."""
    _setenv(monkeypatch, env)
    xyz = _scan(n)
    scan = capi.Scan(ctx, xyz)
    runs = [capi.icp_align(_map(ctx, ndt), scan, _guess(), _p(capi, ndt, w), want_pairs=True)
            for w in ((1.0, 1.0), (0.25, 0.25), (4.0, 4.0))]
    refs = [oracle.icp_align(_omap(oracle, ndt), xyz, _guess(), _p(oracle, ndt, w), want_pairs=True)
            for w in ((1.0, 1.0), (0.25, 0.25), (4.0, 4.0))]
    for r, o in zip(runs, refs):
        _assert_matches(r, o)
        np.testing.assert_array_equal(o["cov"], refs[0]["cov"])
        np.testing.assert_array_equal(r["T"], runs[0]["T"])
        for k in ("local_idx", "global_idx"):
            np.testing.assert_array_equal(r["pairs"][k], runs[0]["pairs"][k])
        np.testing.assert_array_equal(r["cov"], runs[0]["cov"])
    # weights that DO move the pose: the covariance is still mh_covariance of the final pose and pairings, no weight in it
    w = (0.25, 3.0) if ndt else (0.25, 1.0)
    r = capi.icp_align(_map(ctx, ndt), scan, _guess(), _p(capi, ndt, w), prior=_prior(ndt), want_pairs=True)
    pp, pl = _final_pairings(xyz, scan, r, ndt)
    np.testing.assert_allclose(r["cov"], capi.covariance(ctx, r["T"], pp, pl), rtol=1e-9, atol=0)
    assert scaled_gap(r["cov"], onp.covariance_analytic(onp.T44(r["T"]), pp, pl)) < COV_FD_BOUND
