"""mh_icp_align_layers_batch on the device: several multi-layer alignments (one context each) advancing in lock step through
k_match_layers_b / k_accum_layers_b / k_solve_b, every job ending with the bits of its own mh_icp_align_layers call -- and the
driver's general plans (dual-map, edges, one-pair chains) joining an AlignBatcher with them.

Checked against the single call on the same contexts (jobs that differ in everything, iteration counts spread from 0 to the
budget, shrinking batches interleaved with single calls, loop-control switches), against the float64 reference
oracle/layers_oracle.py, for the argument errors, and through the driver and the command line against solo runs."""
import ctypes as C
import importlib.util
import json
import os
import subprocess
import threading
from dataclasses import replace

import numpy as np
import pytest

from mola_lidar_odometry_amd import capi, synth
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _module(name):
    spec = importlib.util.spec_from_file_location("_" + name, os.path.join(ROOT, "tests", name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


layers, chains = _module("test_gpu_icp_layers"), _module("test_odometry_chains")
_Shape, _base, _eight, _pairs, _params, _prior, _reference, _specs = (
    layers._Shape, layers._base, layers._eight, layers._pairs, layers._params, layers._prior, layers._reference, layers._specs)
CHAINS, _FRONT, _ONE_MATCH, _decimate, _map, _merge, inline_pipeline = (
    chains.CHAINS, chains._FRONT, chains._ONE_MATCH, chains._decimate, chains._map, chains._merge, chains.inline_pipeline)
_write_kitti_tree = _module("test_odometry")._write_kitti_tree

pytestmark = pytest.mark.gpu
RESULT_KEYS = ("quality", "n_iterations", "termination_reason", "n_final_pairs", "potential_pairings", "pair_counts")


@pytest.fixture(scope="module")
def shapes(oracle, small_workload):
    """Five jobs' worth of maps and scans, each on a context of its own."""
    return [_Shape(capi.Context(0), oracle, small_workload) for _ in range(5)]


def _shifted(T, dx=0.0, dy=0.0):
    T = np.array(T, np.float64).reshape(12).copy()
    T[3] += dx
    T[7] += dy
    return T


def _job_defs(w):
    """Five jobs that differ in everything: (make_spec(shape) -> (spec, weights), params, guess, prior).  All with two inner steps
    and a covariance, so that they form ONE lock-step group."""
    b40, b30 = _base(w.sigma, 40), _base(w.sigma, 30)

    def one_ndt(sh):  # 1 pair, an NDT map
        return [("ndt", "far", 2.0 * b30, 0.3)], [1.7]

    def two(sh):
        return _specs(w, 2)[0], None

    def three_shared(sh):  # a shared scan (near twice), a trunc-indexed map
        b25 = _base(w.sigma, 25)
        return [("trunc", "near", 2.0 * b25, 0.0), ("far", "far", 1.5 * b25 + 0.2, 0.3), ("far", "near", np.full(25, 1.1), 0.6)], [0.8, 1.0, 2.2]

    def eight(sh):  # 8 pairs, three of them with an empty scan
        spec, weights, _ = _eight(sh)
        return spec, weights

    def two_and_empty(sh):
        b35 = _base(w.sigma, 35)
        key = sh.add_scan("none", np.zeros((0, 3), np.float32))
        return [("near", "near", 2.2 * b35, 0.1), ("near", key, np.full(35, 1.0), 0.0), ("ndt", "far", 1.4 * b35 + 0.3, 0.0)], [1.0, 1.0, 0.4]

    return [
        (one_ndt, _params(30, 0.5 * b30, kernel=capi.KERNEL_GM_C4), _shifted(w.T_guess, dx=0.03), None),
        (two, _params(40, 0.5 * b40, hook_enabled=True, hook_min_trans=0.2, hook_min_rot=np.deg2rad(0.5), hook_checkpoint=w.T_guess),
         w.T_guess, None),
        (three_shared, _params(25, 0.6 * _base(w.sigma, 25), kernel=1), _shifted(w.T_guess, dy=-0.04), _prior(w)),
        (eight, _params(40, 0.5 * b40, disable_stall_test=True), _shifted(w.T_guess, dx=-0.02, dy=0.02), None),
        (two_and_empty, _params(35, 0.4 * _base(w.sigma, 35), kernel=3, min_abs_step_trans=5e-4), w.T_guess, None),
    ]


def _build(shapes, defs, which):
    """The batch arguments of jobs `which` (indices into defs), job k on shapes[which[k]]."""
    jobs, guesses, params, priors = [], [], [], []
    for i in which:
        make, p, T, prior = defs[i]
        spec, weights = make(shapes[i])
        jobs.append(_pairs(shapes[i], spec, weights))
        guesses.append(T)
        params.append(p)
        priors.append(prior)
    return jobs, guesses, params, priors


def _solo(jobs, guesses, params, priors):
    return [capi.icp_align_layers(j, T, p, prior=pr, want_trace=False) for j, T, p, pr in zip(jobs, guesses, params, priors)]


def _assert_same_bits(got, want, what=""):
    assert len(got) == len(want)
    for i, (r, s) in enumerate(zip(got, want)):
        for k in ("T", "cov"):
            np.testing.assert_array_equal(r[k], s[k], err_msg="%s job %d %s" % (what, i, k))
        for k in RESULT_KEYS:
            assert r[k] == s[k], (what, i, k, r[k], s[k])


# ------------------------------------------------------------------------------------------------ 1. the bits of the single call
@pytest.mark.parametrize("which", [[3], [1, 3], [0, 1, 2, 3, 4]], ids=["1job", "2jobs", "5jobs"])
def test_batch_jobs_have_the_bits_of_their_single_calls(shapes, small_workload, which):
    args = _build(shapes, _job_defs(small_workload), which)
    want = _solo(*args)
    got = capi.icp_align_layers_batch(args[0], args[1], args[2], priors=args[3])
    _assert_same_bits(got, want)
    assert all(s["n_final_pairs"] > 0 for s in want)
    assert _solo(*args)[0]["n_iterations"] == want[0]["n_iterations"]  # (and the contexts go on as before)


def test_one_params_struct_for_all_jobs(shapes, small_workload):
    w = small_workload
    spec, kp = _specs(w, 3)
    p = _params(40, kp)
    jobs = [_pairs(sh, spec) for sh in shapes[:3]]
    guesses = [w.T_guess, _shifted(w.T_guess, dx=0.04), _shifted(w.T_guess, dy=0.05)]
    want = [capi.icp_align_layers(j, T, p, want_trace=False) for j, T in zip(jobs, guesses)]
    _assert_same_bits(capi.icp_align_layers_batch(jobs, guesses, p), want)


def test_jobs_of_other_loop_shapes_and_trivial_jobs_ride_along(shapes, small_workload):
    """A job with three inner steps and no covariance, one with max_iterations = 0 and one without points: none of them fits the
    group of the other two, each runs as a single call inside the batch."""
    w = small_workload
    spec, kp = _specs(w, 2)
    empty = shapes[4].add_scan("none", np.zeros((0, 3), np.float32))
    jobs = [_pairs(shapes[0], spec), _pairs(shapes[1], spec), _pairs(shapes[2], spec),
            _pairs(shapes[3], [(mk, sk, 1.0, 0.0) for mk, sk, _, _ in spec]),
            _pairs(shapes[4], [("near", empty, np.full(40, 1.0), 0.0)])]
    params = [_params(40, kp), _params(40, kp), replace(_params(40, kp, inner=3), compute_covariance=False), _params(0, 0.1),
              _params(40, kp)]
    guesses = [w.T_guess] * 5
    want = _solo(jobs, guesses, params, [None] * 5)
    got = capi.icp_align_layers_batch(jobs, guesses, params)
    _assert_same_bits(got, want)
    assert capi.TERM_NAMES[got[4]["termination_reason"]] == "NoPairings" and got[3]["n_iterations"] == 0


# ------------------------------------------------------------------------------------------------ 2. spread of iteration counts
def test_jobs_of_one_batch_end_at_different_iterations(shapes, small_workload):
    w = small_workload
    spec, kp = _specs(w, 2)
    tiny = [(mk, sk, np.full(40, 1e-6), 0.0) for mk, sk, _, _ in spec]
    drop = []
    for mk, sk, thr, _ in spec:
        t = np.array(thr, np.float64).copy()
        t[3:] = 1e-6
        drop.append((mk, sk, t, 0.0))
    jobs = [_pairs(shapes[0], spec), _pairs(shapes[1], spec), _pairs(shapes[2], tiny), _pairs(shapes[3], drop)]
    params = [_params(40, kp), _params(40, kp, disable_stall_test=True), _params(40, kp), _params(40, kp)]
    guesses = [w.T_guess] * 4
    want = _solo(jobs, guesses, params, [None] * 4)
    got = capi.icp_align_layers_batch(jobs, guesses, params)
    _assert_same_bits(got, want)
    names = [capi.TERM_NAMES[r["termination_reason"]] for r in got]
    its = [r["n_iterations"] for r in got]
    assert names[0] == "Stalled" and 0 < its[0] < 40, (names, its)
    assert names[1] == "MaxIterations" and its[1] == 40, (names, its)
    assert names[2] == "NoPairings" and its[2] == 0, (names, its)
    assert names[3] == "NoPairings" and its[3] == 3, (names, its)
    assert len(set(its)) == 4, its


# ------------------------------------------------------------------------------------------------ 3. the float64 reference
def test_three_job_batch_matches_the_reference(oracle, shapes, small_workload):
    w = small_workload
    b = _base(w.sigma, 30)
    spec2, kp2 = _specs(w, 2)
    spec3, kp3 = _specs(w, 3)
    mix = [("ndt", "near", 2.0 * b, 0.0), ("far", "far", 1.5 * b + 0.2, 0.3), ("ndt", "far", 1.8 * b, 0.2)]
    cases = [(spec2, None, 40, kp2, w.T_guess), (spec3, [1.0, 0.6, 1.7], 40, kp3, _shifted(w.T_guess, dx=0.03)),
             (mix, [0.8, 1.0, 2.2], 30, 0.5 * b, w.T_guess)]
    jobs = [_pairs(shapes[i], spec, wt) for i, (spec, wt, _, _, _) in enumerate(cases)]
    params = [_params(mi, kp) for _, _, mi, kp, _ in cases]
    got = capi.icp_align_layers_batch(jobs, [c[4] for c in cases], params)
    for i, (spec, wt, mi, kp, T0) in enumerate(cases):
        o = _reference(oracle, shapes[i], spec, T0, mi, kp, weights=wt)
        assert o["n_final_pairs"] > 0
        for k in RESULT_KEYS:
            assert got[i][k] == o[k], (i, k, got[i][k], o[k])
        np.testing.assert_allclose(got[i]["T"], o["T"], rtol=0, atol=1e-7)


# ------------------------------------------------------------------------------------------------ 4. state reuse
def test_shrinking_batches_between_single_calls_equal_fresh_contexts(oracle, small_workload):
    w = small_workload
    defs = _job_defs(w)
    used = [_Shape(capi.Context(0), oracle, w) for _ in range(5)]
    fresh_shapes = [_Shape(capi.Context(0), oracle, w) for _ in range(5)]
    fresh = _solo(*_build(fresh_shapes, defs, [0, 1, 2, 3, 4]))
    single_p = capi.ICPParams(max_iterations=w.n_iters, threshold=w.threshold, kernel_param=w.kernel_param)
    fresh_single = capi.icp_align(fresh_shapes[1].maps["far"], fresh_shapes[1].scans["far"], w.T_guess, single_p)

    def batch(which):
        a = _build(used, defs, which)
        _assert_same_bits(capi.icp_align_layers_batch(a[0], a[1], a[2], priors=a[3]), [fresh[i] for i in which], str(which))

    def single_calls():
        a = _build(used, defs, [0, 3])
        _assert_same_bits(_solo(*a), [fresh[0], fresh[3]], "single")
        r = capi.icp_align(used[1].maps["far"], used[1].scans["far"], w.T_guess, single_p)
        np.testing.assert_array_equal(r["T"], fresh_single["T"])
        assert r["n_iterations"] == fresh_single["n_iterations"]

    batch([0, 1, 2, 3, 4])
    single_calls()
    batch([0, 2, 4])
    single_calls()
    batch([3])
    batch([4, 1])  # (another leader, another order)
    single_calls()


# ------------------------------------------------------------------------------------------------ 5. loop control
@pytest.mark.parametrize("ctl", [dict(poll_every=1), dict(poll_every=3), dict(poll_every=64), dict(env="MH_NO_GRAPH"),
                                 dict(env="MH_NO_LOCKSTEP")], ids=lambda d: "-".join("%s" % v for v in d.values()))
def test_loop_control_gives_the_bits_of_the_default_batch(shapes, small_workload, monkeypatch, ctl):
    args = _build(shapes, _job_defs(small_workload), [0, 1, 2, 3, 4])
    default = capi.icp_align_layers_batch(args[0], args[1], args[2], priors=args[3])
    ctl = dict(ctl)
    env = ctl.pop("env", None)
    if env:
        monkeypatch.setenv(env, "1")
    params = [replace(p, **ctl) for p in args[2]]
    for _ in range(3):
        _assert_same_bits(capi.icp_align_layers_batch(args[0], args[1], params, priors=args[3]), default)
    if "poll_every" in ctl:
        r = capi.icp_align_layers_batch(args[0], args[1], params, priors=args[3])
        longest = max(x["n_iterations"] + (capi.TERM_NAMES[x["termination_reason"]] != "MaxIterations") for x in r)
        assert r[0]["n_host_polls"] == -(-min(longest, 40) // ctl["poll_every"])  # the chunks the slowest job needs


# ------------------------------------------------------------------------------------------------ 6. errors
def _raw_batch(job_pair_lists, params, T, n_jobs=None):
    """mh_icp_align_layers_batch on raw LayerPair lists; `params`: one ICPParams or a list (per job)."""
    n = len(job_pair_lists)
    keep = [(capi.LayerPair * max(1, len(pl)))(*pl) for pl in job_pair_lists]
    jarr = (capi.LayerJob * max(1, n))()
    for i, (pl, arr) in enumerate(zip(job_pair_lists, keep)):
        jarr[i].n_pairs = len(pl)
        jarr[i].pairs = arr
    Ts = np.ascontiguousarray(np.tile(np.asarray(T, np.float64).reshape(12), max(1, n)))
    if isinstance(params, list):
        made = [p.c(T) for p in params]
        cp = (capi.ICPParamsC * n)(*[m[0] for m in made])
        ref, per = cp, 1
    else:
        cp, made = params.c(T)
        ref, per = C.byref(cp), 0
    res = (capi.ICPResult * max(1, n))()
    return capi.lib().mh_icp_align_layers_batch(n if n_jobs is None else n_jobs, jarr, ref, per, Ts.ctypes.data_as(capi._DP), None,
                                                res, None)


def test_argument_errors_leave_the_contexts_usable(shapes, small_workload):
    w = small_workload
    spec, kp = _specs(w, 2)
    thr = np.full(40, 1.0)
    tp = thr.ctypes.data_as(capi._DP)

    def good(sh, scan="near"):
        return capi.LayerPair(sh.maps["near"]._h, sh.scans[scan]._h, tp, 0.0, 1.0)

    a, b = shapes[0], shapes[1]
    p = _params(40, kp)
    INVALID, UNSUPPORTED = 1, 6
    assert _raw_batch([], p, w.T_guess) == INVALID                                   # no job
    assert _raw_batch([[good(a)]], p, w.T_guess, n_jobs=65) == INVALID                # above MH_MAX_LAYER_BATCH_JOBS
    assert _raw_batch([[good(a)], []], p, w.T_guess) == INVALID                       # a job without pairs
    assert _raw_batch([[good(a)], [good(b)] * 9], p, w.T_guess) == INVALID            # ... with too many
    assert _raw_batch([[good(a)], [capi.LayerPair(b.maps["near"]._h, None, tp, 0.0, 1.0)]], p, w.T_guess) == INVALID
    assert _raw_batch([[good(a)], [capi.LayerPair(b.maps["near"]._h, b.scans["near"]._h, None, 0.0, 1.0)]], p, w.T_guess) == INVALID
    assert _raw_batch([[good(a)], [good(b), capi.LayerPair(b.maps["near"]._h, a.scans["near"]._h, tp, 0.0, 1.0)]], p,
                      w.T_guess) == INVALID                                           # a job on two contexts
    assert _raw_batch([[good(a)], [good(a, "far")]], p, w.T_guess) == INVALID         # two jobs on one context
    assert _raw_batch([[good(a)], [good(b)]], [p, replace(p, pt2pl_threshold=1.0)], w.T_guess) == INVALID
    bad_T = np.array(w.T_guess, np.float64).copy()
    bad_T[5] = np.nan
    assert _raw_batch([[good(a)], [good(b)]], p, bad_T) == INVALID
    assert _raw_batch([[good(a)], [good(b)]], [p, replace(p, profile=True)], w.T_guess) == UNSUPPORTED
    assert _raw_batch([[good(a)], [good(b), good(b)]], [p, replace(p, matched_points=1)], w.T_guess) == UNSUPPORTED
    if capi.device_count() > 1:  # jobs on different devices
        octx = capi.Context(1)
        om, osc = capi.Map(octx, 0.5, 20).build(w.map_xyz), capi.Scan(octx, a.near_l)
        assert _raw_batch([[good(a)], [capi.LayerPair(om._h, osc._h, tp, 0.0, 1.0)]], p, w.T_guess) == INVALID
    assert _raw_batch([[good(a)], [good(b)]], p, w.T_guess) == 0
    args = _build(shapes, _job_defs(w), [0, 1, 2, 3, 4])
    _assert_same_bits(capi.icp_align_layers_batch(args[0], args[1], args[2], priors=args[3]), _solo(*args))


# ------------------------------------------------------------------------------------------------ 7. the driver
# the structure of extras/lidar3d-kissicp-like.yaml: de-skew, a range filter, two voxel decimations, one map and one layer pair
KISS_TAIL = ("localmap_generator:\n" + _map("localmap", 20) + "observations_filter_1st_pass:\n" + _FRONT.split("  - class_name: mp2p_icp_filters::FilterBoundingBox")[0] +
             _decimate("range_filtered", "decimated_for_map", "0.5") + _decimate("decimated_for_map", "decimated_for_icp", "1.5") +
             """  - class_name: mp2p_icp_filters::FilterDeleteLayer
    params:
      pointcloud_layer_to_remove: ['raw', 'deskewed', 'range_filtered']
insert_observation_into_local_map:
""" + _merge("decimated_for_map", "localmap"))
DRIVER_CHAINS = dict(CHAINS, **{"kissicp-like": (KISS_TAIL, _ONE_MATCH)})
RECORD_KEYS = ("pose", "icp_iterations", "twist_corrections", "align_calls", "termination", "goodness", "sigma", "n_for_icp",
               "n_map_points", "map_updated", "icp_good")


@pytest.fixture(scope="module")
def host():
    from mola_lidar_odometry_amd import _mp2p_icp_hip as H
    return H


@pytest.fixture(scope="module")
def drives():
    return [synth.make_drive(n, seed=s, speed=v) for n, s, v in ((12, 4242, 8.0), (9, 777, 5.0), (14, 99, 10.0))]


def _feed(lo, d):
    for (xyz, t), st in zip(d["scans"], d["stamps"]):
        lo.onLidar(float(st), xyz, t)


def _solo_records(host, text, d):
    lo = host.LidarOdometry(0, True)
    lo.initialize(host.Config.FromYamlText(text))
    _feed(lo, d)
    return lo.records()


def _threads_with_one_batcher(host, texts, drives):
    """A thread per (pipeline text, drive) and one AlignBatcher over them; returns (records per sequence, the batcher)."""
    batcher = host.AlignBatcher(len(drives))
    los, errors = [], []
    for text in texts:
        lo = host.LidarOdometry(own_context=True)
        lo.initialize(host.Config.FromYamlText(text))
        lo.setAlignBatcher(batcher)
        los.append(lo)

    def work(lo, d):
        try:
            _feed(lo, d)
        except Exception as e:  # noqa: BLE001
            errors.append(e)
        finally:
            batcher.leave()

    th = [threading.Thread(target=work, args=(lo, d)) for lo, d in zip(los, drives)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in th), "a sequence thread is stuck"
    assert not errors, errors
    return [lo.records() for lo in los], batcher


def _assert_records_equal(got, ref):
    assert len(got) == len(ref)
    for a, b in zip(got, ref):
        for key in RECORD_KEYS:
            assert a[key] == b[key], key


@pytest.mark.timeout(600)
@pytest.mark.parametrize("chain", ["dual-map", "edges", "kissicp-like"])
def test_general_plans_share_lockstep_batches(host, drives, chain):
    """Three drives of different lengths on one chain, a thread each: their alignments run as batches (the multi-layer chains
    through mh_icp_align_layers_batch, the one-pair chain through mh_icp_align_batch) and every record is the solo run's."""
    text = inline_pipeline(*DRIVER_CHAINS[chain])
    solo = [_solo_records(host, text, d) for d in drives]
    got, batcher = _threads_with_one_batcher(host, [text] * 3, drives)
    assert batcher.jobs() > 0 and batcher.batches() < batcher.jobs()
    assert batcher.jobs() >= sum(len(d["scans"]) - 1 for d in drives)
    for g, r in zip(got, solo):
        _assert_records_equal(g, r)


@pytest.mark.timeout(600)
def test_mixed_chains_with_the_generic_route_do_not_hold_each_other_up(host, drives):
    """dual-map, near-far (the matcher-by-matcher route: no batched form) and edges beside each other on one batcher: nobody
    hangs, every record is the solo run's, and the two multi-layer sequences still meet in batches."""
    texts = [inline_pipeline(*DRIVER_CHAINS[c]) for c in ("dual-map", "near-far", "edges")]
    solo = [_solo_records(host, t, d) for t, d in zip(texts, drives)]
    got, batcher = _threads_with_one_batcher(host, texts, drives)
    assert batcher.jobs() > 0 and batcher.batches() < batcher.jobs()
    for g, r in zip(got, solo):
        _assert_records_equal(g, r)


# ------------------------------------------------------------------------------------------------ 8. the command line
@pytest.mark.timeout(900)
def test_cli_batches_a_dual_map_pipeline_over_three_sequences(drives, tmp_path):
    exe = os.path.join(ROOT, "mola_lidar_odometry_amd", "molahip-lo-cli")
    pipe = tmp_path / "dual-map.yaml"
    pipe.write_text(inline_pipeline(*CHAINS["dual-map"]))
    dirs = []
    for k, d in enumerate(drives):
        _write_kitti_tree(str(tmp_path / ("k%d" % k)), d)
        dirs.append(str(tmp_path / ("k%d" % k) / "sequences" / "00"))
    args = [exe, "--pipeline", str(pipe), "--out", str(tmp_path / "multi.tum")]
    for d in dirs:
        args += ["--seq-dir", d]
    r = subprocess.run(args, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    summary = json.loads(r.stdout.strip().splitlines()[-1])
    assert summary["sequences"] == 3 and summary["scans"] == sum(len(d["scans"]) for d in drives)
    jobs = summary["batches"] * summary["jobs_per_batch"]
    assert summary["batches"] > 0 and summary["batches"] < jobs, summary
    for k, d in enumerate(dirs):
        one = str(tmp_path / ("solo%d.tum" % k))
        r1 = subprocess.run([exe, "--pipeline", str(pipe), "--seq-dir", d, "--out", one], capture_output=True, text=True, timeout=300)
        assert r1.returncode == 0, r1.stderr
        assert open(one).read() == open(str(tmp_path / ("multi_%d.tum" % k))).read()
