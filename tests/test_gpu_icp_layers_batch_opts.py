"""mh_icp_align_layers_batch_opts on the device: multi-layer alignments with unique pairs (allowMatchAlreadyMatchedGlobalPoints:
false), iteration gates and pairingsPerPoint > 1 advancing in lock step -- k_claim_layers_b / k_resolve_layers_b between the match
and the first accumulation, k_match_layers_kb and the *_layers_kb accumulations in a group of the k > 1 kind -- every job ending
with the bits of its own mh_icp_align_layers_kbest call; and the driver's unique and gated chains joining an AlignBatcher.

Checked against the single call on the same contexts (two job orders, iteration counts spread from 0 to the budget with claims
outstanding, claim epochs across batches and single calls, loop-control switches), against the float64 references of
tests/kbest_ref.py and tests/gates_ref.py (cases that tests/test_kbest_cpu.py and tests/test_gates_cpu.py cover on the CPU; none
is set apart there, none here), for the identities with mh_icp_align_layers_batch, for the argument errors, and through the driver
against solo runs.

Scan sizes: 1, 65 and 257 points around a wave (64), a claim workgroup (256) and their boundaries; 700, 1025 and 2000 points for
several workgroups of every launch."""
import ctypes as C
import importlib.util
import os
from dataclasses import replace

import numpy as np
import pytest

import gates_ref as G
import kbest_ref as K
from mola_lidar_odometry_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _module(name):
    spec = importlib.util.spec_from_file_location("_" + name, os.path.join(ROOT, "tests", name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


pytestmark = pytest.mark.gpu
RESULT_KEYS = ("quality", "n_iterations", "termination_reason", "n_final_pairs", "potential_pairings", "pair_counts")
INVALID, UNSUPPORTED = 1, 6
MAX_PAIRINGS_PER_POINT = 8  # MH_MAX_PAIRINGS_PER_POINT


# ------------------------------------------------------------------------------------------------------------------ the jobs
def _pair(mk, local, thr, k=1, ang=0.0, weight=1.0, gate=(0, 0), unique=0):
    return dict(map=mk, local=np.ascontiguousarray(local, np.float32).reshape(-1, 3), threshold=thr, threshold_angular_deg=ang,
                weight=weight, gate=gate, unique=unique, k=k)


def _from_gates(c, inp):
    """a case of gates_ref in the form of kbest_ref's: k = 1 everywhere, two inner steps, gates_ref's guess"""
    assert c["hook"] is None
    return dict(pairs=[dict(e, k=1) for e in c["pairs"]], max_it=c["max_it"], kp=c["kp"], inner=2, T0=inp.T0, prior=c["prior"],
                pkw=c["pkw"])


def _case_defs(w):
    """name -> (case, which reference module's maps it names, the reference case or None).  All with two inner steps and a
    covariance: the jobs without a pair of k > 1 form one lock-step group, those with one the other."""
    gi, ki = G.Inputs(w), K.Inputs(w)
    gc, kc = G.cases(gi), K.cases(ki)
    b40 = G.base(w.sigma, 40)
    drop = np.array(2.0 * b40, np.float64).copy()
    drop[3:] = 1e-6
    own = dict(max_it=40, kp=0.5 * b40, inner=2, T0=gi.T0, prior=None, pkw={})
    out = {}
    # ---- no pair with k > 1
    out["plain"] = (dict(own, pairs=[_pair("near", gi.near_l, 2.0 * b40), _pair("far", gi.far_pool[:1360], 1.5 * b40 + 0.2, ang=0.3)]), gi, None)
    for n in (1, 65, 257, 1025):  # the near-far shape: pair 0 gated from iteration 4
        out["near_far_%d" % n] = (_from_gates(gc["near_far_%d" % n], gi), gi, ("g", "near_far_%d" % n))
    out["gated_unique"] = (_from_gates(gc["unique"], gi), gi, ("g", "unique"))
    out["nobody_at_0"] = (_from_gates(gc["nobody_at_0"], gi), gi, ("g", "nobody_at_0"))
    out["unique_and_not"] = (dict(own, pairs=[_pair("whole", gi.even, 2.0 * b40, unique=1),
                                              _pair("whole", gi.odd, 1.5 * b40 + 0.2, weight=0.5)]), gi, None)
    out["empty_first"] = (dict(own, pairs=[_pair("near", np.zeros((0, 3)), 2.0 * b40, unique=1), _pair("near", gi.near_l, 2.0 * b40, unique=1),
                                           _pair("far", gi.far_pool[:700], 1.5 * b40 + 0.2)]), gi, None)
    # (test 3) unique jobs that end at different iterations
    out["unique_drop_at_3"] = (dict(own, pairs=[_pair("whole", gi.even, drop, unique=1), _pair("whole", gi.odd, drop, unique=1)]), gi, None)
    out["unique_to_the_end"] = (dict(own, pairs=[_pair("whole", gi.even, 2.0 * b40, unique=1), _pair("whole", gi.odd, 2.0 * b40, unique=1)],
                                     pkw=dict(disable_stall_test=True)), gi, None)
    out["unique_stalls"] = (dict(own, pairs=[_pair("whole", gi.even, 2.0 * b40, unique=1), _pair("near", gi.near_l, 2.0 * b40)]), gi, None)
    # ---- a pair with k > 1
    for name in ("unique_k21", "gated", "ref_k3_n65", "ref_k2_n1", "ref_k2_n700"):  # (ref_k2_n700: every pair with k > 1)
        out[name] = (kc[name], ki, ("k", name))
    for name, (c, src, ref) in out.items():
        assert c["inner"] == 2, name
    return out, gi, ki


class _Job:
    """One case on a context of its own: its maps, its scans, its arguments."""

    def __init__(self, name, case, src):
        self.name, self.c = name, case
        self.ctx = capi.Context(0)
        self.maps = {}
        for e in case["pairs"]:
            if e["map"] not in self.maps:
                pts, vs, cap = src.maps[e["map"]]
                self.maps[e["map"]] = capi.Map(self.ctx, vs, cap).build(pts)
        self.pairs = [dict(map=self.maps[e["map"]], scan=capi.Scan(self.ctx, e["local"]), threshold=e["threshold"],
                           threshold_angular_deg=e["threshold_angular_deg"], weight=e["weight"], unique_global=e["unique"],
                           run_from_iteration=e["gate"][0], run_up_to_iteration=e["gate"][1]) for e in case["pairs"]]
        self.kpp = [e["k"] for e in case["pairs"]]
        self.T0, self.prior = case["T0"], case["prior"]
        self.params = capi.ICPParams(max_iterations=case["max_it"], kernel_param=case["kp"], threshold=1.0,
                                     gn=capi.GNParams(max_inner_iterations=case["inner"], robust_kernel=capi.KERNEL_GM_C4), **case["pkw"])

    def solo(self, **kw):
        """mh_icp_align_layers_opts / _gated / _kbest as capi.icp_align_layers chooses it"""
        return capi.icp_align_layers(self.pairs, self.T0, replace(self.params, **kw), prior=self.prior, want_trace=False,
                                     pairings_per_point=self.kpp if any(k > 1 for k in self.kpp) else None)


class _World:
    def __init__(self, w, names=None):
        self.defs, self.gi, self.ki = _case_defs(w)
        self.jobs = {n: _Job(n, c, src) for n, (c, src, ref) in self.defs.items() if names is None or n in names}

    def batch(self, names, **kw):
        js = [self.jobs[n] for n in names]
        return capi.icp_align_layers_batch([j.pairs for j in js], [j.T0 for j in js], [replace(j.params, **kw) for j in js],
                                           priors=[j.prior for j in js], pairings_per_point=[j.kpp for j in js])


# the batch of test 1, in two orders.  ORDER_A: the job without claim workgroups first, the k > 1 group led by a mixed job.
# ORDER_B: that job last, the job whose pairs all have k > 1 first in its group, the groups interleaved.
ORDER_A = ["plain", "near_far_1", "near_far_65", "near_far_257", "near_far_1025", "gated_unique", "unique_and_not", "empty_first",
           "unique_k21", "gated", "ref_k3_n65", "ref_k2_n1", "ref_k2_n700"]
ORDER_B = ["ref_k2_n700", "empty_first", "ref_k2_n1", "gated_unique", "gated", "near_far_1025", "unique_k21", "near_far_257",
           "ref_k3_n65", "unique_and_not", "near_far_65", "near_far_1", "plain"]
SPREAD = ["unique_drop_at_3", "nobody_at_0", "unique_to_the_end", "unique_stalls"]
EPOCH_JOBS = ["plain", "gated_unique", "unique_and_not", "empty_first", "unique_k21", "gated"]


@pytest.fixture(scope="module")
def world(oracle, small_workload):
    return _World(small_workload)


@pytest.fixture(scope="module")
def solo(world):
    """every job's single call on its own context, once"""
    return {n: j.solo() for n, j in world.jobs.items()}


@pytest.fixture(scope="module")
def fresh(oracle, small_workload):
    """the single calls of EPOCH_JOBS on contexts that have seen nothing else"""
    fw = _World(small_workload, names=EPOCH_JOBS)
    return {n: fw.jobs[n].solo() for n in EPOCH_JOBS}


def _assert_same_bits(got, want, what=""):
    assert len(got) == len(want)
    for i, (r, s) in enumerate(zip(got, want)):
        for k in ("T", "cov"):
            np.testing.assert_array_equal(r[k], s[k], err_msg="%s job %d %s" % (what, i, k))
        for k in RESULT_KEYS:
            assert r[k] == s[k], (what, i, k, r[k], s[k])


# ------------------------------------------------------------------------------------------------ 1. the bits of the single call
@pytest.mark.parametrize("order", [ORDER_A, ORDER_B], ids=["plain-first", "plain-last"])
def test_batch_jobs_have_the_bits_of_their_single_calls(world, solo, order):
    assert sorted(order) == sorted(ORDER_A)
    got = world.batch(order)
    _assert_same_bits(got, [solo[n] for n in order], "batch")
    assert all(solo[n]["n_final_pairs"] > 0 for n in order)
    # both kinds of group have members, with and without claim workgroups, and the unique jobs did lose claims
    assert sum(any(k > 1 for k in world.jobs[n].kpp) for n in order) >= 2
    assert solo["unique_and_not"]["pair_counts"][0] < len(world.gi.even)
    assert world.jobs[order[0]].solo()["n_iterations"] == solo[order[0]]["n_iterations"]  # (and the contexts go on as before)


# ------------------------------------------------------------------------------------------------ 2. the float64 reference
@pytest.fixture(scope="module")
def references(world):
    gm, km, cache = world.gi.omaps(), world.ki.omaps(), {}

    def get(name):
        if name not in cache:
            kind, case = world.defs[name][2]
            if kind == "g":
                cache[name] = G.case_reference(G.cases(world.gi)[case], gm, world.gi.T0)
            else:
                cache[name] = K.case_reference(K.cases(world.ki)[case], km)
        return cache[name]
    return get


def test_batch_matches_the_float64_references(world, references):
    names = [n for n in ORDER_A if world.defs[n][2] is not None]
    assert len(names) == 10
    got = world.batch(ORDER_A)
    for n in names:
        r, o = got[ORDER_A.index(n)], references(n)
        assert o["n_final_pairs"] > 0 and not K.set_apart(o), n
        dT = float(np.abs(np.asarray(r["T"]) - o["T"]).max())
        print("%s: iterations %d / %d, final pairs %d / %d, potential %d / %d, max |dT| %.2e" % (
            n, r["n_iterations"], o["n_iterations"], r["n_final_pairs"], o["n_final_pairs"], r["potential_pairings"],
            o["potential_pairings"], dT))
        for k in RESULT_KEYS:
            assert r[k] == o[k], (n, k, r[k], o[k])
        np.testing.assert_allclose(r["T"], o["T"], rtol=0, atol=1e-7, err_msg=n)


# ------------------------------------------------------------------------------------------------ 3. spread of iteration counts
def test_jobs_end_at_different_iterations_with_claims_outstanding(world, solo):
    got = world.batch(SPREAD)
    _assert_same_bits(got, [solo[n] for n in SPREAD], "spread")
    names = [capi.TERM_NAMES[r["termination_reason"]] for r in got]
    its = [r["n_iterations"] for r in got]
    assert names[0] == "NoPairings" and its[0] == 3, (names, its)
    assert names[1] == "NoPairings" and its[1] == 0, (names, its)
    assert names[2] == "MaxIterations" and its[2] == 40, (names, its)
    assert names[3] == "Stalled" and 3 < its[3] < 40, (names, its)
    assert len(set(its)) == 4, its


# ------------------------------------------------------------------------------------------------ 4. claim epochs across calls
def test_claim_epochs_across_batches_and_single_calls_equal_fresh_contexts(oracle, small_workload, fresh):
    used = _World(small_workload, names=EPOCH_JOBS)

    def batch(names):
        _assert_same_bits(used.batch(names), [fresh[n] for n in names], str(names))

    def singles(names):
        _assert_same_bits([used.jobs[n].solo() for n in names], [fresh[n] for n in names], "single " + str(names))

    batch(EPOCH_JOBS)
    singles(["gated_unique", "unique_k21", "empty_first"])
    batch(["unique_k21", "unique_and_not", "gated_unique"])  # (smaller, another leader, another order)
    # a single unique call against ANOTHER map on one of the contexts: its regions are laid out differently in the same table
    j = used.jobs["unique_and_not"]
    other = capi.Map(j.ctx, 1.0, 20).build(np.ascontiguousarray(small_workload.map_xyz[::3]))
    pairs = [dict(j.pairs[0], map=other, unique_global=1), dict(j.pairs[1], map=other, unique_global=1)]
    a = capi.icp_align_layers(pairs, j.T0, j.params, want_trace=False)
    assert a["n_final_pairs"] > 0
    batch(EPOCH_JOBS[::-1])
    b = capi.icp_align_layers(pairs, j.T0, j.params, want_trace=False)
    _assert_same_bits([b], [a], "other map")
    singles(EPOCH_JOBS)


# ------------------------------------------------------------------------------------------------ 5. loop control
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
    _assert_same_bits(world.batch(ORDER_A, **ctl), default, "again")
    if "poll_every" in ctl:
        # the jobs of a group share its chunks: as many polls as the group's slowest job needs -- single calls would each count
        # their own.  (nobody here has a budget below 8, the jobs that run to theirs are in the group without k > 1.)
        for kind in (False, True):
            rs = [r for n, r in zip(ORDER_A, got) if any(k > 1 for k in world.jobs[n].kpp) == kind]
            budget = max(world.jobs[n].params.max_iterations for n in ORDER_A if any(k > 1 for k in world.jobs[n].kpp) == kind)
            longest = max(x["n_iterations"] + (capi.TERM_NAMES[x["termination_reason"]] != "MaxIterations") for x in rs)
            assert len(rs) >= 2 and {x["n_host_polls"] for x in rs} == {-(-min(longest, budget) // ctl["poll_every"])}, (kind, ctl)
    if env == "MH_NO_PREV_BOUND":  # every search unbounded: against the single calls under the same switch
        _assert_same_bits(got, [world.jobs[n].solo() for n in ORDER_A], "solo without bounds")


# ------------------------------------------------------------------------------------------------ 6. identities
def _raw(js, mode, kpp=None, n_jobs=None, pair_lists=None):
    """mh_icp_align_layers_batch_opts on raw arrays: (status, results).  mode: 'null' -- no array in any job; 'zeros' / 'ones' --
    all three arrays in every job, opts and gates zero, knn 0 / 1; 'own' -- every job's own options.  kpp: {job index: values} that
    replace a job's pairings per point; pair_lists: {job index: LayerPair list} that replace a job's pairs."""
    n = len(js)
    keep, jarr = [], (capi.LayerJobOpts * max(1, n))()
    for i, j in enumerate(js):
        arr, norm, thr_keep = capi._layer_pairs(j.pairs, j.params.max_iterations)
        if pair_lists and i in pair_lists:
            arr = (capi.LayerPair * max(1, len(pair_lists[i])))(*pair_lists[i])
            norm = pair_lists[i]
        npairs = len(norm)
        opts, gates, knn = (capi.LayerPairOpts * max(1, npairs))(), (capi.LayerPairGates * max(1, npairs))(), (capi.LayerPairKnn * max(1, npairs))()
        for k in range(min(npairs, len(j.pairs))):
            if mode == "own":
                opts[k].unique_global = int(j.pairs[k]["unique_global"])
                gates[k].run_from_iteration, gates[k].run_up_to_iteration = j.pairs[k]["run_from_iteration"], j.pairs[k]["run_up_to_iteration"]
            knn[k].pairings_per_point = j.kpp[k] if mode == "own" else 1 if mode == "ones" else 0
        if kpp and i in kpp:
            for k, v in enumerate(kpp[i]):
                knn[k].pairings_per_point = v
        keep.append((arr, thr_keep, opts, gates, knn))
        jarr[i].n_pairs, jarr[i].pairs = npairs, arr
        if mode != "null":
            jarr[i].opts, jarr[i].gates, jarr[i].knn = opts, gates, knn
    T = np.ascontiguousarray(np.concatenate([np.asarray(j.T0, np.float64).reshape(-1)[:12] for j in js]))
    made = [replace(j.params, threshold=1.0).c(T[12 * i:12 * i + 12]) for i, j in enumerate(js)]
    cp = (capi.ICPParamsC * max(1, n))(*[m[0] for m in made])
    res = (capi.ICPResult * max(1, n))()
    counts = (C.c_uint64 * (max(1, n) * capi.MAX_LAYER_PAIRS))()
    st = capi.lib().mh_icp_align_layers_batch_opts(n if n_jobs is None else n_jobs, jarr, cp, 1, T.ctypes.data_as(capi._DP), None, res,
                                                   counts)
    out = []
    for i in range(n if st == 0 else 0):
        d = capi._result_dict(res[i])
        d["pair_counts"] = [int(counts[i * capi.MAX_LAYER_PAIRS + k]) for k in range(len(js[i].pairs))]
        out.append(d)
    return st, out


def test_without_options_it_is_the_plain_batch(small_workload):
    """three jobs without any option (contexts of their own: no prior on them), through mh_icp_align_layers_batch and through the new
    entry point with NULL arrays, arrays of zeros, and ones in knn"""
    w = small_workload
    gi = G.Inputs(w)
    b40, b30 = G.base(w.sigma, 40), G.base(w.sigma, 30)
    own = dict(max_it=40, kp=0.5 * b40, inner=2, T0=gi.T0, prior=None, pkw={})
    cases = [dict(own, pairs=[_pair("near", gi.near_l, 2.0 * b40), _pair("far", gi.far_pool[:1360], 1.5 * b40 + 0.2, ang=0.3)]),
             dict(own, pairs=[_pair("whole", gi.even, 2.0 * b40), _pair("whole", gi.odd, 1.5 * b40 + 0.2, weight=0.5)], T0=gi.T1),
             dict(own, pairs=[_pair("far", gi.far_pool[:257], 2.0 * b30), _pair("near", gi.near_l, 2.0 * b30), _pair("whole", gi.even[:65], 1.1)],
                  max_it=30, kp=0.5 * b30)]
    js = [_Job("p%d" % i, c, gi) for i, c in enumerate(cases)]
    plain = capi.icp_align_layers_batch([j.pairs for j in js], [j.T0 for j in js], [j.params for j in js])
    assert all(r["n_final_pairs"] > 0 for r in plain)
    for mode in ("null", "zeros", "ones"):
        st, got = _raw(js, mode)
        assert st == 0, mode
        _assert_same_bits(got, plain, mode)


def test_one_job_with_options_leaves_the_others_their_bits(world, solo):
    names = ["plain", "near_far_257", "unique_and_not"]
    # (near_far_257 stands in as a second job whose bits must not move; drop its gates and it is a plain job too)
    got = world.batch(names)
    _assert_same_bits(got, [solo[n] for n in names], "one with claims")
    st, raw = _raw([world.jobs[n] for n in names], "own")
    assert st == 0
    _assert_same_bits(raw, got, "raw")


# ------------------------------------------------------------------------------------------------ 7. errors
def test_argument_errors_consume_nothing(world, solo, fresh):
    a, b = world.jobs["gated_unique"], world.jobs["unique_k21"]

    def after_error():
        _assert_same_bits(world.batch(ORDER_A), [solo[n] for n in ORDER_A], "after an error")
        _assert_same_bits([a.solo(), b.solo()], [fresh["gated_unique"], fresh["unique_k21"]], "single after an error")

    st, _ = _raw([a, b], "own", kpp={1: [MAX_PAIRINGS_PER_POINT + 1, 1]})
    assert st == INVALID
    after_error()
    # two jobs on one context
    arr_a, _, keep_a = capi._layer_pairs(a.pairs, a.params.max_iterations)
    st, _ = _raw([a, b], "own", pair_lists={1: [arr_a[1]]})
    assert st == INVALID
    after_error()
    # a null scan
    arr_b, _, keep_b = capi._layer_pairs(b.pairs, b.params.max_iterations)
    bad = capi.LayerPair(arr_b[0].map, None, arr_b[0].threshold, 0.0, 1.0)
    st, _ = _raw([a, b], "own", pair_lists={1: [bad]})
    assert st == INVALID
    st, _ = _raw([a, b], "own", n_jobs=0)
    assert st == INVALID
    st, _ = _raw([a, b], "own", n_jobs=capi.MAX_LAYER_BATCH_JOBS + 1)
    assert st == INVALID
    after_error()
    st, got = _raw([a, b], "own")
    assert st == 0
    _assert_same_bits(got, [solo["gated_unique"], solo["unique_k21"]], "good call")


# ------------------------------------------------------------------------------------------------ 8. the driver
@pytest.fixture(scope="module")
def host():
    from mola_lidar_odometry_amd import _mp2p_icp_hip as H
    return H


@pytest.fixture(scope="module")
def drv():
    return _module("test_gpu_icp_layers_batch")


@pytest.fixture(scope="module")
def drives(drv):
    from mola_lidar_odometry_amd import synth
    return [synth.make_drive(n, seed=s, speed=v) for n, s, v in ((12, 4242, 8.0), (9, 777, 5.0), (14, 99, 10.0))]


def _near_far_text(drv):
    return drv.inline_pipeline(*drv.CHAINS["near-far"])


def _near_far_gated_text(drv):
    """the near-far chain with its far pair in a matcher block of its own that enters in iteration 2, as the second block of the
    reference's lidar3d-near-far.yaml does"""
    text = _near_far_text(drv)
    near, far = drv.chains.NEARFAR_MATCHES.splitlines(True)
    assert text.count(near + far) == 1
    block = text.split("  matchers:\n")[1].split("        pointLayerMatches:\n")[0]  # "    - class: ...  params: ..." of the one block
    assert block.lstrip().startswith("- class: mp2p_icp_hip::Matcher_Points_DistanceThreshold")
    return text.replace(near + far, near + block + "        runFromIteration: 2\n        pointLayerMatches:\n" + far)


def _unique_default_text(drv):
    text = open(drv.chains.PIPE).read()
    assert text.count("allowMatchAlreadyMatchedGlobalPoints: true") == 1
    return text.replace("allowMatchAlreadyMatchedGlobalPoints: true", "allowMatchAlreadyMatchedGlobalPoints: false")


def _unique_near_far_text(drv):
    text = _near_far_text(drv)
    assert text.count("allowMatchAlreadyMatchedGlobalPoints: true") == 1
    return text.replace("allowMatchAlreadyMatchedGlobalPoints: true", "allowMatchAlreadyMatchedGlobalPoints: false")


TEXTS = {"near-far": _near_far_text, "near-far-gated": _near_far_gated_text, "default-unique": _unique_default_text,
         "near-far-unique": _unique_near_far_text}


@pytest.fixture(scope="module")
def solo_records(host, drv, drives):
    cache = {}

    def get(chain):
        if chain not in cache:
            cache[chain] = [drv._solo_records(host, TEXTS[chain](drv), d) for d in drives]
        return cache[chain]
    return get


@pytest.mark.timeout(600)
@pytest.mark.parametrize("chain", ["near-far", "near-far-gated", "default-unique", "near-far-unique"])
def test_unique_and_gated_chains_share_lockstep_batches(host, drv, drives, solo_records, chain):
    """Three drives of different lengths on one chain, a thread each, on one AlignBatcher: every alignment is a job of a batch and
    every record is the solo run's."""
    text = TEXTS[chain](drv)
    got, batcher = drv._threads_with_one_batcher(host, [text] * 3, drives)
    for g, r in zip(got, solo_records(chain)):
        drv._assert_records_equal(g, r)
    assert batcher.jobs() >= sum(len(d["scans"]) - 1 for d in drives)
    assert batcher.batches() < batcher.jobs()


@pytest.mark.timeout(600)
@pytest.mark.parametrize("chain", ["near-far-gated", "near-far-unique"])
def test_switched_off_they_run_beside_the_batches(host, drv, drives, solo_records, monkeypatch, chain):
    """MOLA_HIP_BATCH_OPTS=0: the alignments run on their own (no job of the batcher), the records are the same"""
    monkeypatch.setenv("MOLA_HIP_BATCH_OPTS", "0")
    host.reload_plugin_switches()
    try:
        got, batcher = drv._threads_with_one_batcher(host, [TEXTS[chain](drv)] * 3, drives)
    finally:
        monkeypatch.delenv("MOLA_HIP_BATCH_OPTS")
        host.reload_plugin_switches()
    for g, r in zip(got, solo_records(chain)):
        drv._assert_records_equal(g, r)
    assert batcher.jobs() == 0
