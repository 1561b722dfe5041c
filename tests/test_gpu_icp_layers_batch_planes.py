"""mh_icp_align_layers_batch_planes on the device: multi-layer alignments with Matcher_Point2Plane pairs (KNN + PCA on point layers)
advancing in lock step -- k_match_layers_pl_b behind the other searches, k_accum_layers_pl_b behind every point accumulation,
k_solve_pl_b / k_cov_finalize_pl_b adding each job's second partials block behind its first -- every job ending with the bits of
its own mh_icp_align_layers_planes call; and the driver's chain with a Matcher_Point2Plane block joining an AlignBatcher.

Checked against the single call on the same contexts (two job orders, iteration counts spread from 0 to the budget, loop-control
switches), against the float64 reference of tests/planes_ref.py (cases that tests/test_planes_cpu.py covers on the CPU; none is set
apart there, none here), for the identities with mh_icp_align_layers_batch_opts, for the argument errors, and through the driver
against solo runs.  The jobs are tests/planes_batch_cases.py's.

Plane pairs of 1, 63, 64, 65 and 257 points around a wave = a match workgroup (64) and a plane accumulation workgroup (256); 700
and 2000 points for several workgroups of every launch; an empty plane pair in front; jobs of plane pairs only."""
import ctypes as C
import importlib.util
import os
from dataclasses import replace

import numpy as np
import pytest

import planes_batch_cases as pb
import planes_ref as pr
from mola_lidar_odometry_amd import capi
from oracle import layers_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _module(name):
    spec = importlib.util.spec_from_file_location("_" + name, os.path.join(ROOT, "tests", name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


pytestmark = pytest.mark.gpu
RESULT_KEYS = ("quality", "n_iterations", "termination_reason", "n_final_pairs", "n_final_pairs_pt2pl", "potential_pairings",
               "pair_counts")
INVALID = 1
ORDER_A, ORDER_B, SPREAD = pb.ORDER_A, pb.ORDER_B, pb.SPREAD


# ------------------------------------------------------------------------------------------------------------------ the jobs
class _Job:
    """One case on a context of its own: its maps, its scans, its arguments."""

    def __init__(self, name, case, inp):
        self.name, self.c = name, case
        self.ctx = capi.Context(0)
        self.maps = {}
        for e in case["pairs"]:
            if e["map"] not in self.maps:
                pts, vs, cap = inp.maps[e["map"]]
                self.maps[e["map"]] = capi.Map(self.ctx, vs, cap).build(pts)
        self.pairs, kpp = pr.device_pairs(case, self.maps, lambda a: capi.Scan(self.ctx, a))
        self.kpp = kpp  # None, or one value per pair
        self.T0, self.prior = case["T0"], case["prior"]
        self.params = pr.device_params(case)

    def solo(self, **kw):
        """mh_icp_align_layers_planes (or the entry point before it) as capi.icp_align_layers chooses it"""
        return capi.icp_align_layers(self.pairs, self.T0, replace(self.params, **kw), prior=self.prior, want_trace=False,
                                     pairings_per_point=self.kpp)


class _World:
    def __init__(self, w, names=None):
        self.inp = pr.Inputs(w)
        self.defs = pb.case_defs(self.inp)
        self.jobs = {n: _Job(n, c, self.inp) for n, c in self.defs.items() if names is None or n in names}

    def batch(self, names, planes_entry=False, **kw):
        js = [self.jobs[n] for n in names]
        return capi.icp_align_layers_batch([j.pairs for j in js], [j.T0 for j in js], [replace(j.params, **kw) for j in js],
                                           priors=[j.prior for j in js], pairings_per_point=[j.kpp for j in js],
                                           planes_entry=planes_entry)


@pytest.fixture(scope="module")
def world(oracle, small_workload):
    return _World(small_workload)


@pytest.fixture(scope="module")
def solo(world):
    """every job's single call on its own context, once"""
    return {n: j.solo() for n, j in world.jobs.items()}


def _assert_same_bits(got, want, what=""):
    assert len(got) == len(want)
    for i, (r, s) in enumerate(zip(got, want)):
        for k in ("T", "cov"):
            np.testing.assert_array_equal(r[k], s[k], err_msg="%s job %d %s" % (what, i, k))
        for k in RESULT_KEYS:
            assert r[k] == s[k], (what, i, k, r[k], s[k])


# ------------------------------------------------------------------------------------------------ 1. the bits of the single call
@pytest.mark.parametrize("order", [ORDER_A, ORDER_B], ids=["planes-first", "interleaved"])
def test_batch_jobs_have_the_bits_of_their_single_calls(world, solo, order):
    assert sorted(order) == sorted(ORDER_A) and len(order) >= 13
    got = world.batch(order)
    _assert_same_bits(got, [solo[n] for n in order], "batch")
    assert all(solo[n]["n_final_pairs"] > 0 for n in order)
    planes = [n for n in order if pb.has_plane(world.defs[n])]
    assert all(solo[n]["n_final_pairs_pt2pl"] > 0 for n in planes)
    # plane jobs without and with k > 1, at least two of each, and at least two jobs without any plane pair
    assert sum(not pb.has_kbest(world.defs[n]) for n in planes) >= 2 and sum(pb.has_kbest(world.defs[n]) for n in planes) >= 2
    assert len(order) - len(planes) >= 2 and all(solo[n]["n_final_pairs_pt2pl"] == 0 for n in order if n not in planes)
    # a job of plane pairs only, and the empty plane pair in front of its job
    assert solo["ref_n2000"]["n_final_pairs"] == solo["ref_n2000"]["n_final_pairs_pt2pl"]
    assert solo["empty_first"]["pair_counts"][0] == 0 and solo["empty_first"]["pair_counts"][1] > 0
    # (and the contexts go on as before)
    _assert_same_bits([world.jobs[n].solo() for n in (order[0], "rgbd")], [solo[order[0]], solo["rgbd"]], "single call afterwards")


# ------------------------------------------------------------------------------------------------ 2. the float64 reference
@pytest.fixture(scope="module")
def references(world):
    """the reference of every job that is a case of planes_ref, computed once and left unchanged"""
    om = world.inp.omaps()
    return {n: pr.case_reference(world.defs[n], om) for n in pb.REF_CASES}


def test_batch_matches_the_float64_reference(world, references):
    got = world.batch(ORDER_A)
    for n in pb.REF_CASES:
        r, o = got[ORDER_A.index(n)], references[n]
        assert not pr.set_apart(o), n
        dT = float(np.abs(np.asarray(r["T"]) - o["T"]).max())
        print("%s: iterations %d / %d, final pairs %d / %d (plane %d / %d), potential %d / %d, counts %s / %s, max |dT| %.2e" % (
            n, r["n_iterations"], o["n_iterations"], r["n_final_pairs"], o["n_final_pairs"], r["n_final_pairs_pt2pl"],
            o["n_final_pairs_pt2pl"], r["potential_pairings"], o["potential_pairings"], r["pair_counts"], o["pair_counts"], dT))
        # tests/test_gpu_icp_layers_planes.py's _check without what a batch does not return: the trace and the pairings
        diffs = layers_oracle.compare(dict(r, trace=o["trace"]), o, with_pairs=False)
        if r["n_final_pairs_pt2pl"] != o["n_final_pairs_pt2pl"]:
            diffs.append("n_final_pairs_pt2pl %d vs %d" % (r["n_final_pairs_pt2pl"], o["n_final_pairs_pt2pl"]))
        assert not diffs, (n, diffs)


# ------------------------------------------------------------------------------------------------ 3. spread of iteration counts
def test_plane_jobs_end_at_different_iterations(world, solo):
    assert all(pb.has_plane(world.defs[n]) for n in SPREAD)
    got = world.batch(SPREAD)
    _assert_same_bits(got, [solo[n] for n in SPREAD], "spread")
    names = [capi.TERM_NAMES[r["termination_reason"]] for r in got]
    its = [r["n_iterations"] for r in got]
    assert names[0] == "NoPairings" and its[0] == 3, (names, its)
    assert names[1] == "NoPairings" and its[1] == 0, (names, its)
    assert names[2] == "MaxIterations" and its[2] == world.defs["to_the_end"]["max_it"], (names, its)
    assert names[3] == "Stalled" and 3 < its[3] < 40, (names, its)
    assert len(set(its)) == 4, its
    assert got[2]["n_final_pairs_pt2pl"] > 0 and got[3]["n_final_pairs_pt2pl"] > 0


# ------------------------------------------------------------------------------------------------ 4. loop control
@pytest.mark.parametrize("ctl", [dict(poll_every=1), dict(poll_every=3), dict(poll_every=64), dict(env="MH_NO_GRAPH"),
                                 dict(env="MH_NO_LOCKSTEP"), dict(env="MH_NO_PREV_BOUND")],
                         ids=lambda d: "-".join("%s" % v for v in d.values()))
def test_loop_control_gives_the_bits_of_the_default_batch(world, monkeypatch, ctl):
    default = world.batch(ORDER_A)
    ctl = dict(ctl)
    env = ctl.pop("env", None)
    if env:
        monkeypatch.setenv(env, "1")
    got = world.batch(ORDER_A, **ctl)
    _assert_same_bits(got, default, str(ctl or env))
    if env == "MH_NO_PREV_BOUND":  # every search under the radius bound alone: against the single calls under the same switch
        _assert_same_bits(got, [world.jobs[n].solo() for n in ORDER_A], "solo without bounds")


# ------------------------------------------------------------------------------------------------ 5. identities
def _raw(entry, js, mode, n_jobs=None, edit=None):
    """mh_icp_align_layers_batch_opts / _planes on raw arrays: (status, results).  mode: 'null' -- no planes array in any job (the
    opts entry point has none anyway); 'zeros' -- an array of zeros in every job; 'own' -- every job's own.  opts, gates and knn
    are the jobs' own throughout.  edit(i, pair array, opts, knn, planes): changes job i's arrays in place before the call."""
    n = len(js)
    with_planes = entry == "planes"
    keep, jarr = [], ((capi.LayerJobPlanes if with_planes else capi.LayerJobOpts) * max(1, n))()
    for i, j in enumerate(js):
        arr, norm, thr_keep = capi._layer_pairs(j.pairs, j.params.max_iterations)
        npairs = len(norm)
        opts, gates, knn = (capi.LayerPairOpts * npairs)(), (capi.LayerPairGates * npairs)(), (capi.LayerPairKnn * npairs)()
        planes = (capi.LayerPairPlane * npairs)()
        for k, e in enumerate(norm):
            opts[k].unique_global = int(e.get("unique_global") or 0)
            gates[k].run_from_iteration, gates[k].run_up_to_iteration = e["run_from_iteration"], e["run_up_to_iteration"]
            knn[k].pairings_per_point = j.kpp[k] if j.kpp else 1
            q = e.get("plane")
            if q and mode == "own":
                planes[k] = capi.LayerPairPlane(q["knn"], q["minimum_plane_points"], q["plane_eigen_threshold"], q["search_radius"])
        if edit:
            edit(i, arr, opts, knn, planes)
        keep.append((arr, thr_keep, opts, gates, knn, planes))
        jarr[i].n_pairs, jarr[i].pairs, jarr[i].opts, jarr[i].gates, jarr[i].knn = npairs, arr, opts, gates, knn
        if with_planes and mode != "null":
            jarr[i].planes = planes
    T = np.ascontiguousarray(np.concatenate([np.asarray(j.T0, np.float64).reshape(-1)[:12] for j in js]))
    made = [replace(j.params, threshold=1.0).c(T[12 * i:12 * i + 12]) for i, j in enumerate(js)]
    cp = (capi.ICPParamsC * max(1, n))(*[m[0] for m in made])
    res = (capi.ICPResult * max(1, n))()
    counts = (C.c_uint64 * (max(1, n) * capi.MAX_LAYER_PAIRS))()
    st = getattr(capi.lib(), "mh_icp_align_layers_batch_" + entry)(n if n_jobs is None else n_jobs, jarr, cp, 1, T.ctypes.data_as(capi._DP),
                                                                   None, res, counts)
    out = []
    for i in range(n if st == 0 else 0):
        d = capi._result_dict(res[i])
        d["pair_counts"] = [int(counts[i * capi.MAX_LAYER_PAIRS + k]) for k in range(len(js[i].pairs))]
        out.append(d)
    return st, out


def test_without_planes_it_is_the_batch_before_it(world):
    js = [world.jobs[n] for n in pb.PLANE_LESS]
    st, old = _raw("opts", js, "null")
    assert st == 0 and all(r["n_final_pairs"] > 0 for r in old)
    for mode in ("null", "zeros"):
        st, got = _raw("planes", js, mode)
        assert st == 0, mode
        _assert_same_bits(got, old, mode)


def test_the_point_pair_jobs_of_the_batch_before_it_keep_their_bits(oracle, small_workload):
    """tests/test_gpu_icp_layers_batch_opts.py's ORDER_A -- unique pairs, gates, k > 1 -- through the entry point before and
    through the new one"""
    bo = _module("test_gpu_icp_layers_batch_opts")
    w = bo._World(small_workload, names=bo.ORDER_A)
    old = w.batch(bo.ORDER_A)
    assert all(r["n_final_pairs"] > 0 for r in old)
    js = [w.jobs[n] for n in bo.ORDER_A]
    new = capi.icp_align_layers_batch([j.pairs for j in js], [j.T0 for j in js], [j.params for j in js], priors=[j.prior for j in js],
                                      pairings_per_point=[j.kpp for j in js], planes_entry=True)
    for r, s in zip(new, old):
        for k in ("T", "cov"):
            np.testing.assert_array_equal(r[k], s[k])
        for k in RESULT_KEYS:
            assert r[k] == s[k], k


def test_one_plane_job_leaves_the_others_their_bits(world, solo):
    names = ["plain_halves", "ref_n700", "plain_split"]
    got = world.batch(names)
    _assert_same_bits(got, [solo[n] for n in names], "one plane job")
    assert got[1]["n_final_pairs_pt2pl"] > 0
    st, raw = _raw("planes", [world.jobs[n] for n in names], "own")
    assert st == 0
    _assert_same_bits(raw, got, "raw")


# ------------------------------------------------------------------------------------------------ 6. errors
def test_argument_errors_consume_nothing(oracle, small_workload, world, solo):
    bo = _module("test_gpu_icp_layers_batch_opts")
    uw = bo._World(small_workload, names=["gated_unique", "unique_and_not"])  # unique jobs: their claim epochs must not move
    fresh = bo._World(small_workload, names=["gated_unique", "unique_and_not"])
    uniq = [uw.jobs["gated_unique"], uw.jobs["unique_and_not"]]
    fresh_solo = [fresh.jobs[n].solo() for n in ("gated_unique", "unique_and_not")]
    a, b = world.jobs["ref_n700"], world.jobs["gated"]
    good = ["ref_n700", "gated", "ref_n65", "rgbd", "plane_k2"]

    def after_error():
        _assert_same_bits(world.batch(good), [solo[n] for n in good], "after an error")
        _assert_same_bits([a.solo(), b.solo()], [solo["ref_n700"], solo["gated"]], "single after an error")
        _assert_same_bits([j.solo() for j in uniq], fresh_solo, "unique single after an error")

    def on_b(fn):
        def edit(i, arr, opts, knn, planes):
            if i == 1:
                fn(arr, opts, knn, planes)
        return edit

    def unique_global(arr, opts, knn, planes):
        opts[0].unique_global = 1

    def k2(arr, opts, knn, planes):
        knn[0].pairings_per_point = 2

    def angular(arr, opts, knn, planes):
        arr[0].threshold_angular_deg = 0.5

    def knn17(arr, opts, knn, planes):
        planes[0].knn = capi.MAX_PLANE_KNN + 1

    def radius0(arr, opts, knn, planes):
        planes[0].search_radius = 0.0

    assert world.defs["gated"]["pairs"][0]["plane"] and capi.MAX_PLANE_KNN == 16
    for fn in (unique_global, k2, angular, knn17, radius0):
        st, _ = _raw("planes", [a, b] + uniq, "own", edit=on_b(fn))
        assert st == INVALID, fn.__name__
        after_error()

    # two jobs on one context
    arr_a, _, keep_a = capi._layer_pairs(a.pairs, a.params.max_iterations)

    def same_context(arr, opts, knn, planes):
        arr[0] = arr_a[0]
        arr[1] = arr_a[0]

    st, _ = _raw("planes", [a, b] + uniq, "own", edit=on_b(same_context))
    assert st == INVALID
    after_error()
    st, _ = _raw("planes", [a, b] + uniq, "own", n_jobs=0)
    assert st == INVALID
    st, _ = _raw("planes", [a, b] + uniq, "own", n_jobs=capi.MAX_LAYER_BATCH_JOBS + 1)
    assert st == INVALID
    after_error()
    st, got = _raw("planes", [a, b], "own")
    assert st == 0
    _assert_same_bits(got, [solo["ref_n700"], solo["gated"]], "good call")


# ------------------------------------------------------------------------------------------------ 7. the driver
PLANE_BLOCK = """    - class: mp2p_icp_hip::Matcher_Point2Plane
      params:
        distanceThreshold: 1.0
        planeEigenThreshold: 1e-2
        searchRadius: %s
        knn: 10
        minimumPlanePoints: 6
        pointLayerMatches:
          - {global: "localmap", local: "decimated_for_icp", weight: 1.0}
"""
SEARCH_RADIUS = "2.5"  # [m] the local map's points lie up to a voxel (1 m and more) apart: rgbd.yaml's 0.8 m finds no ten of them


@pytest.fixture(scope="module")
def host():
    from mola_lidar_odometry_amd import _mp2p_icp_hip as H
    return H


@pytest.fixture(scope="module")
def drv():
    return _module("test_gpu_icp_layers_batch")


@pytest.fixture(scope="module")
def drives():
    from mola_lidar_odometry_amd import synth
    return [synth.make_drive(n, seed=s, speed=v) for n, s, v in ((12, 4242, 8.0), (9, 777, 5.0), (14, 99, 10.0))]


def _plane_chain_text(drv):
    """the default chain with a Matcher_Point2Plane block on its point layers behind its Matcher_Points_DistanceThreshold"""
    text = open(drv.chains.PIPE).read()
    one = drv.chains._ONE_MATCH
    assert text.count(one) == 1
    return text.replace(one, one + PLANE_BLOCK % SEARCH_RADIUS)


@pytest.fixture(scope="module")
def solo_records(host, drv, drives):
    return [drv._solo_records(host, _plane_chain_text(drv), d) for d in drives]


def test_the_solo_runs_find_plane_pairings(solo_records):
    """Both matchers pair the same layer, so potential_pairings is twice its size and the point matcher alone reaches a paired
    ratio of at most one half: a goodness above that has plane pairings in it."""
    for recs in solo_records:
        good = [r["goodness"] for r in recs if r["icp_run"]]
        print("goodness %.3f .. %.3f over %d alignments" % (min(good), max(good), len(good)))
        assert len(good) >= 8 and max(good) > 0.5


@pytest.mark.timeout(600)
def test_plane_chains_share_lockstep_batches(host, drv, drives, solo_records):
    """Three drives of different lengths on the chain, a thread each, on one AlignBatcher: every alignment is a job of a batch and
    every record is the solo run's."""
    got, batcher = drv._threads_with_one_batcher(host, [_plane_chain_text(drv)] * 3, drives)
    for g, r in zip(got, solo_records):
        drv._assert_records_equal(g, r)
    assert batcher.jobs() >= sum(len(d["scans"]) - 1 for d in drives)
    assert batcher.batches() < batcher.jobs()


@pytest.mark.timeout(600)
def test_switched_off_they_run_beside_the_batches(host, drv, drives, solo_records, monkeypatch):
    """MOLA_HIP_BATCH_PLANES=0: the alignments run on their own (no job of the batcher), the records are the same"""
    monkeypatch.setenv("MOLA_HIP_BATCH_PLANES", "0")
    host.reload_plugin_switches()
    try:
        got, batcher = drv._threads_with_one_batcher(host, [_plane_chain_text(drv)] * 3, drives)
    finally:
        monkeypatch.delenv("MOLA_HIP_BATCH_PLANES")
        host.reload_plugin_switches()
    for g, r in zip(got, solo_records):
        drv._assert_records_equal(g, r)
    assert batcher.jobs() == 0
