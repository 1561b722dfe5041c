"""mh_icp_align_layers_kbest on the device: Matcher_Points_DistanceThreshold::pairingsPerPoint > 1 inside the fused multi-layer loop
(k_match_layers_k, mh_k_match_kbest.h).

Checked against the float64 reference (tests/kbest_ref.py: oracle/layers_oracle.py's loop over oracle_c.match_points_k) on fixed
cases none of which is set apart (tests/test_kbest_cpu.py), against mh_nn_search_k independently of the oracle, for bitwise
reproducibility with and without the search bound and the captured graphs, and for what must not change: knn NULL / 0 / 1 is
mh_icp_align_layers_gated bit for bit."""
import ctypes as C
from dataclasses import replace

import numpy as np
import pytest

import kbest_ref as kr
from mola_lidar_odometry_amd import capi
from oracle import layers_oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    return capi.Context(0)


@pytest.fixture(scope="module")
def inp(small_workload, oracle):
    return kr.Inputs(small_workload)


@pytest.fixture(scope="module")
def omaps(inp):
    return inp.omaps()


@pytest.fixture(scope="module")
def dmaps(ctx, inp):
    return {k: capi.Map(ctx, vs, cap).build(pts) for k, (pts, vs, cap) in inp.maps.items()}


@pytest.fixture(scope="module")
def all_cases(inp):
    return kr.cases(inp)


def _device(ctx, dmaps, c, **kw):
    pairs = [dict(map=dmaps[e["map"]], scan=capi.Scan(ctx, e["local"]), threshold=e["threshold"],
                  threshold_angular_deg=e["threshold_angular_deg"], weight=e["weight"], unique_global=e["unique"],
                  run_from_iteration=e["gate"][0], run_up_to_iteration=e["gate"][1]) for e in c["pairs"]]
    return capi.icp_align_layers(pairs, c["T0"], kr.device_params(c), prior=c["prior"], want_pairs=True,
                                 pairings_per_point=[e["k"] for e in c["pairs"]], **kw)


def _check(ctx, dmaps, omaps, c):
    o = kr.case_reference(c, omaps)
    assert not kr.set_apart(o) and o["n_final_pairs"] > 0
    r = _device(ctx, dmaps, c)
    dT = float(np.abs(np.asarray(r["T"]) - o["T"]).max())
    print("iterations %d / %d, final pairs %d / %d, potential %d / %d, max |dT| %.2e" % (
        r["n_iterations"], o["n_iterations"], r["n_final_pairs"], o["n_final_pairs"], r["potential_pairings"],
        o["potential_pairings"], dT))
    diffs = layers_oracle.compare(r, o)
    assert not diffs, diffs
    return r, o


# ------------------------------------------------------------------------------------------------ 1. against the reference
@pytest.mark.parametrize("n", kr.SIZES)
@pytest.mark.parametrize("k", kr.KS)
def test_matches_the_reference(ctx, dmaps, omaps, all_cases, k, n):
    r, o = _check(ctx, dmaps, omaps, all_cases["ref_k%d_n%d" % (k, n)])
    li = r["pairs"][0]["local_idx"]
    assert np.all(np.diff(li.astype(np.int64)) >= 0) and (len(li) == 0 or li.max() < n)
    same = li[1:] == li[:-1]
    assert np.all(r["pairs"][0]["d2"][1:][same] >= r["pairs"][0]["d2"][:-1][same])  # a point's pairings in ascending distance


@pytest.mark.parametrize("name", ["angular", "mixed", "inner3_prior", "sparse", "dup", "bound", "leave"])
def test_matches_the_reference_on(ctx, dmaps, omaps, all_cases, name):
    _check(ctx, dmaps, omaps, all_cases[name])


# ------------------------------------------------------------------------------------ 3. independent of the oracle: mh_nn_search_k
@pytest.mark.parametrize("k", [2, 8])
def test_one_iteration_is_nn_search_k(ctx, dmaps, inp, k):
    thr = 0.6
    scan = capi.Scan(ctx, inp.scan)
    p = capi.ICPParams(max_iterations=1, kernel_param=0.5, threshold=1.0, gn=capi.GNParams(max_inner_iterations=1))
    r = capi.icp_align_layers([dict(map=dmaps["whole"], scan=scan, threshold=thr, threshold_angular_deg=0.1)], inp.T0, p,
                              want_pairs=True, pairings_per_point=k)
    s = capi.nn_search_k(dmaps["whole"], scan, inp.T0, thr, k, threshold_angular_deg=0.1)
    assert len(s["local_idx"]) > 2000 and r["n_final_pairs"] == len(s["local_idx"])
    assert r["potential_pairings"] == s["potential_pairings"] == 2000 * k
    for key in ("local_idx", "global_idx", "global_xyz", "d2"):
        np.testing.assert_array_equal(r["pairs"][0][key], s[key])


# ------------------------------------------------------------------------------------- 4. bound exactness and reproducibility
def test_bitwise_equal_with_and_without_bound_and_graphs(ctx, dmaps, all_cases, monkeypatch):
    c = all_cases["bound"]
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
        for key in ("local_idx", "global_idx", "global_xyz", "d2"):
            assert other["pairs"][0][key].tobytes() == runs[0]["pairs"][0][key].tobytes(), key


# ------------------------------------------------------------------------------------------------------- 5. k = 1 identity
def _raw(entry, pairs, T_guess, p, opts=None, gates=None, knn="absent"):
    """mh_icp_align_layers_gated / _kbest with the arrays handed over as they are (None: NULL): (status, result dict)."""
    cp, keep = replace(p, threshold=1.0).c(T_guess)
    T0 = np.ascontiguousarray(np.asarray(T_guess, np.float64).reshape(-1)[:12])
    arr, norm, thr_keep = capi._layer_pairs(pairs, p.max_iterations)
    n = len(norm)
    res = capi.ICPResult()
    counts = (C.c_uint64 * n)()
    po, bufs = (capi.PairsOut * n)(), []
    for i, e in enumerate(norm):
        m = max(e["scan"].n if e.get("scan") is not None else 1, 1) * 8
        li, gi = np.zeros(m, np.uint32), np.zeros(m, np.uint32)
        f = [np.zeros(m, np.float32) for _ in range(4)]
        po[i] = capi.PairsOut(li.ctypes.data_as(capi._UP), gi.ctypes.data_as(capi._UP), *[a.ctypes.data_as(capi._FP) for a in f])
        bufs.append((li, gi, *f))
    args = [n, arr, opts, gates] + ([] if entry == "gated" else [knn]) + [C.byref(cp), T0.ctypes.data_as(capi._DP), None,
                                                                           C.byref(res), None, po, counts, capi.MEM_HOST]
    st = getattr(capi.lib(), "mh_icp_align_layers_" + entry)(*args)
    out = capi._result_dict(res)
    out["pair_counts"] = [int(c) for c in counts]
    out["pairs"] = [dict(local_idx=b[0][:k].copy(), global_idx=b[1][:k].copy(), d2=b[5][:k].copy())
                    for b, k in zip(bufs, out["pair_counts"])]
    return st, out


def test_k_one_is_mh_icp_align_layers_gated(ctx, dmaps, inp, all_cases):
    c = all_cases["mixed"]
    pairs = [dict(map=dmaps[e["map"]], scan=capi.Scan(ctx, e["local"]), threshold=e["threshold"], weight=e["weight"]) for e in c["pairs"]]
    p = kr.device_params(c)
    st, old = _raw("gated", pairs, c["T0"], p)
    assert st == 0 and old["n_final_pairs"] > 0
    ones, zeros = (capi.LayerPairKnn * 2)(), (capi.LayerPairKnn * 2)()
    ones[0].pairings_per_point = ones[1].pairings_per_point = 1
    for knn in (ones, zeros, None):
        st, new = _raw("kbest", pairs, c["T0"], p, knn=knn)
        assert st == 0
        for key in ("T", "cov"):
            assert np.asarray(new[key]).tobytes() == np.asarray(old[key]).tobytes(), key
        for key in ("n_iterations", "termination_reason", "n_final_pairs", "potential_pairings", "quality", "pair_counts"):
            assert new[key] == old[key], key
        for a, b in zip(new["pairs"], old["pairs"]):
            for key in ("local_idx", "global_idx", "d2"):
                np.testing.assert_array_equal(a[key], b[key])


# ------------------------------------------------------------------------------------------------- 6, 7. unique x k, gates x k
@pytest.mark.parametrize("name", ["unique_k2", "unique_k21"])
def test_unique_pairs_claim_rank_by_rank(ctx, dmaps, omaps, all_cases, name):
    r, o = _check(ctx, dmaps, omaps, all_cases[name])
    allg = np.concatenate([p["global_idx"] for p in r["pairs"]])
    assert len(np.unique(allg)) == len(allg)  # the pairs share the map: one pairing per map point over both


def test_gated_pair_with_k(ctx, dmaps, omaps, all_cases):
    r, o = _check(ctx, dmaps, omaps, all_cases["gated"])
    assert r["potential_pairings"] == 700 * 2 + 1300
    r, o = _check(ctx, dmaps, omaps, all_cases["gated_short"])  # k_last = 1: the pair with k = 2 is not active there
    assert r["potential_pairings"] == 1300 and r["pair_counts"][0] == 0


# ------------------------------------------------------------------------------------------------------------- 8. errors
def test_errors_leave_the_context_usable(ctx, dmaps, inp, all_cases):
    INVALID, UNSUPPORTED = 1, 6
    c = all_cases["ref_k2_n700"]
    scan = capi.Scan(ctx, c["pairs"][0]["local"])
    good = dict(map=dmaps["whole"], scan=scan, threshold=c["pairs"][0]["threshold"])
    p = kr.device_params(c)
    knn = (capi.LayerPairKnn * 1)()
    knn[0].pairings_per_point = 2
    st, ref = _raw("kbest", [good], c["T0"], p, knn=knn)
    assert st == 0 and ref["n_final_pairs"] > 0

    def again():
        st, r = _raw("kbest", [good], c["T0"], p, knn=knn)
        assert st == 0 and np.asarray(r["T"]).tobytes() == np.asarray(ref["T"]).tobytes()

    nine = (capi.LayerPairKnn * 1)()
    nine[0].pairings_per_point = 9
    assert _raw("kbest", [good], c["T0"], p, knn=nine)[0] == INVALID
    again()
    assert _raw("kbest", [dict(good, map=None)], c["T0"], p, knn=knn)[0] == INVALID
    again()
    # 2^26 points x 8 pairings = 2^29 entries on a unique pair: refused on the sizes, before any pairing memory is asked for
    big = capi.Scan(ctx, np.zeros((1 << 26, 3), np.float32))
    eight = (capi.LayerPairKnn * 1)()
    eight[0].pairings_per_point = 8
    uniq = (capi.LayerPairOpts * 1)()
    uniq[0].unique_global = 1
    st, _ = _raw_status_only([dict(good, scan=big)], c["T0"], p, uniq, eight)
    assert st == UNSUPPORTED
    del big
    again()


def _raw_status_only(pairs, T_guess, p, opts, knn):
    """the call without output arrays (a scan of 2^26 points would want gigabytes of them)"""
    cp, keep = replace(p, threshold=1.0).c(T_guess)
    T0 = np.ascontiguousarray(np.asarray(T_guess, np.float64).reshape(-1)[:12])
    arr, norm, thr_keep = capi._layer_pairs(pairs, p.max_iterations)
    res = capi.ICPResult()
    st = capi.lib().mh_icp_align_layers_kbest(len(norm), arr, opts, None, knn, C.byref(cp), T0.ctypes.data_as(capi._DP), None,
                                              C.byref(res), None, None, None, capi.MEM_HOST)
    return st, res


# ------------------------------------------------------------------------------------------------- 9. fall-back coverage
def test_large_first_step_hands_points_to_the_fallback(ctx, dmaps, omaps, inp, all_cases):
    """A guess 0.5 m off and a wide threshold: after the first step the previous partners lie most of a voxel away, the bound
    reaches more than kFlatMaxCand voxels for points near a voxel corner and the lane's own scan serves them; others' partners
    have left the block (bound not attained).  Held to the reference like every case."""
    s = inp.scan
    c = dict(all_cases["ref_k3_n2000"], pairs=[kr._pair("whole", s, np.full(40, 1.6), 3)])
    _check(ctx, dmaps, omaps, c)
