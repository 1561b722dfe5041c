"""mh_icp_align_layers_planes on the device: Matcher_Point2Plane on a plain point layer (KNN + PCA) inside the fused multi-layer loop
(k_match_layers_pl, mh_k_match_planes.h).

Checked against the float64 reference (tests/planes_ref.py) on fixed cases none of which is set apart (tests/test_planes_cpu.py);
by replaying oracle_c.match_pt2pl_knn at the poses the device's own trace reports (free of pose rounding); against
mh_nn_search_pt2pl_knn independently of the oracle; for what must not change (planes NULL / zeros is mh_icp_align_layers_kbest bit
for bit); for bitwise reproducibility with and without the search bound and the captured graphs; the covariance against
mh_covariance on the returned pairings; and the argument errors."""
import ctypes as C
from dataclasses import replace

import numpy as np
import pytest

import planes_ref as pr
from mola_lidar_odometry_amd import capi
from oracle import layers_oracle, oracle_c

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    return capi.Context(0)


@pytest.fixture(scope="module")
def inp(small_workload, oracle):
    return pr.Inputs(small_workload)


@pytest.fixture(scope="module")
def omaps(inp):
    return inp.omaps()


@pytest.fixture(scope="module")
def dmaps(ctx, inp):
    return {k: capi.Map(ctx, vs, cap).build(pts) for k, (pts, vs, cap) in inp.maps.items()}


@pytest.fixture(scope="module")
def all_cases(inp):
    return pr.cases(inp)


@pytest.fixture(scope="module")
def refs(all_cases, omaps):
    """every case's reference, computed once and left unchanged"""
    return {name: pr.case_reference(c, omaps) for name, c in all_cases.items()}


def _device(ctx, dmaps, c, **kw):
    pairs, ks = pr.device_pairs(c, dmaps, lambda a: capi.Scan(ctx, a))
    return capi.icp_align_layers(pairs, c["T0"], pr.device_params(c), prior=c["prior"], want_pairs=True, pairings_per_point=ks, **kw)


def _compare_pairs(c, r, o):
    bad = []
    for i, (e, x, y) in enumerate(zip(c["pairs"], r["pairs"], o["pairs"])):
        if e["plane"]:
            if not np.array_equal(x["local_idx"], y["local_idx"]):
                bad.append("plane pair %d: index sets differ" % i)
                continue
            for key in ("centroid", "normal"):  # the tolerance of test_gpu_parity.py's plane test
                if not np.allclose(x[key], y[key], rtol=0.0, atol=1e-6):
                    bad.append("plane pair %d: %s max |d| %.3e" % (i, key, float(np.abs(x[key] - y[key]).max())))
        else:
            for key in ("local_idx", "global_idx", "d2"):
                if not np.array_equal(x[key], y[key]):
                    bad.append("pair %d: %s differ" % (i, key))
    return bad


def _check(ctx, dmaps, c, o):
    assert not pr.set_apart(o)
    r = _device(ctx, dmaps, c)
    dT = float(np.abs(np.asarray(r["T"]) - o["T"]).max())
    print("iterations %d / %d, final pairs %d / %d (plane %d / %d), potential %d / %d, counts %s / %s, max |dT| %.2e" % (
        r["n_iterations"], o["n_iterations"], r["n_final_pairs"], o["n_final_pairs"], r["n_final_pairs_pt2pl"],
        o["n_final_pairs_pt2pl"], r["potential_pairings"], o["potential_pairings"], r["pair_counts"], o["pair_counts"], dT))
    diffs = layers_oracle.compare(r, o, with_pairs=False)
    if r["n_final_pairs_pt2pl"] != o["n_final_pairs_pt2pl"]:
        diffs.append("n_final_pairs_pt2pl %d vs %d" % (r["n_final_pairs_pt2pl"], o["n_final_pairs_pt2pl"]))
    if r["pair_counts"] == o["pair_counts"]:
        diffs += _compare_pairs(c, r, o)
    assert not diffs, diffs
    return r


# ------------------------------------------------------------------------------------------------ 1. against the reference
@pytest.mark.parametrize("n", pr.SIZES)
def test_matches_the_reference(ctx, dmaps, all_cases, refs, n):
    r = _check(ctx, dmaps, all_cases["ref_n%d" % n], refs["ref_n%d" % n])
    li = r["pairs"][0]["local_idx"].astype(np.int64)
    assert len(li) > 0 and np.all(np.diff(li) > 0) and li.max() < n


@pytest.mark.parametrize("name", ["rgbd", "knn16", "knn3", "sparse", "dup", "gated", "off_pose", "weight", "inner3_prior"])
def test_matches_the_reference_on(ctx, dmaps, all_cases, refs, name):
    _check(ctx, dmaps, all_cases[name], refs[name])


# ---------------------------------------------------------------------------------------------- 2. replay at the device's poses
@pytest.mark.parametrize("name", ["ref_n2000", "rgbd", "gated", "off_pose", "dup"])
def test_replay_at_the_devices_own_poses(ctx, dmaps, omaps, all_cases, name):
    c = all_cases[name]
    r = _device(ctx, dmaps, c)
    poses = [np.asarray(c["T0"], np.float64)] + [np.asarray(t["T"], np.float64) for t in r["trace"]]
    sets = None
    for j, t in enumerate(r["trace"]):  # iteration j matched at poses[j] and reported t["n_pairs"]
        total, sets = 0, {}
        for i, e in enumerate(c["pairs"]):
            if not pr.active(e["gate"], j):
                sets[i] = np.zeros(0, np.uint32)
            elif e["plane"]:
                sets[i] = pr.match_plane(omaps[e["map"]], e["local"], poses[j], float(np.broadcast_to(e["threshold"], (c["max_it"],))[j]),
                                         e["plane"])["local_idx"]
            else:
                sets[i] = oracle_c.match_points_k(omaps[e["map"]], e["local"], poses[j],
                                                  float(np.broadcast_to(e["threshold"], (c["max_it"],))[j]), e["k"])["local_idx"]
            total += len(sets[i])
        assert total == t["n_pairs"], (name, j, total, t["n_pairs"])
    # the last traced iteration is the one whose match produced the final pairings
    assert len(r["trace"]) == min(r["n_iterations"] + 1, c["max_it"])
    for i, e in enumerate(c["pairs"]):
        if e["plane"]:
            np.testing.assert_array_equal(r["pairs"][i]["local_idx"], sets[i])
            assert r["pair_counts"][i] == len(sets[i])


# --------------------------------------------------------------------- 3. independent of the oracle: mh_nn_search_pt2pl_knn
@pytest.mark.parametrize("knn", [3, 10, 16])
def test_one_iteration_is_nn_search_pt2pl_knn(ctx, dmaps, inp, knn):
    pl = dict(knn=knn, minimum_plane_points=min(knn, 6), plane_eigen_threshold=2e-2, search_radius=1.1)
    scan = capi.Scan(ctx, inp.scan)
    p = capi.ICPParams(max_iterations=1, kernel_param=0.5, threshold=1.0, gn=capi.GNParams(max_inner_iterations=1))
    r = capi.icp_align_layers([dict(map=dmaps["whole"], scan=scan, threshold=0.4, plane=pl)], inp.T0, p, want_pairs=True)
    s = capi.nn_search_pt2pl_knn(dmaps["whole"], scan, inp.T0, 0.4, pl["plane_eigen_threshold"], pl["search_radius"], knn,
                                 pl["minimum_plane_points"])
    assert len(s["local_idx"]) > 300 and r["n_final_pairs"] == r["n_final_pairs_pt2pl"] == len(s["local_idx"])
    assert r["potential_pairings"] == s["potential_pairings"] == 2000
    for key in ("local_idx", "centroid", "normal"):
        np.testing.assert_array_equal(r["pairs"][0][key], s[key])


# ------------------------------------------------------------------------------------------------- 4. what must not change
def _raw(entry, pairs, T_guess, p, opts=None, gates=None, knn=None, planes="absent"):
    """mh_icp_align_layers_kbest / _planes with the arrays handed over as they are (None: NULL): (status, result dict)."""
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
    head = [n, arr, opts, gates, knn] + ([planes] if entry == "planes" else [])
    tail = [C.byref(cp), T0.ctypes.data_as(capi._DP), None, C.byref(res), None, po] + ([None] if entry == "planes" else [])
    st = getattr(capi.lib(), "mh_icp_align_layers_" + entry)(*(head + tail + [counts, capi.MEM_HOST]))
    out = capi._result_dict(res)
    out["pair_counts"] = [int(c) for c in counts]
    out["pairs"] = [dict(local_idx=b[0][:k].copy(), global_idx=b[1][:k].copy(), d2=b[5][:k].copy())
                    for b, k in zip(bufs, out["pair_counts"])]
    return st, out


def test_no_plane_pair_is_mh_icp_align_layers_kbest(ctx, dmaps, inp):
    s = inp.scan
    thr = pr.kbest_ref.schedule(40)
    pairs = [dict(map=dmaps["whole"], scan=capi.Scan(ctx, np.ascontiguousarray(s[0::3])), threshold=thr),
             dict(map=dmaps["whole"], scan=capi.Scan(ctx, np.ascontiguousarray(s[1::3])), threshold=thr, weight=0.5),
             dict(map=dmaps["whole"], scan=capi.Scan(ctx, np.ascontiguousarray(s[2::3])), threshold=thr)]
    p = capi.ICPParams(max_iterations=40, kernel_param=np.full(40, 0.5), threshold=1.0,
                       gn=capi.GNParams(max_inner_iterations=2, robust_kernel=capi.KERNEL_GM_C4))
    knn, opts, gates = (capi.LayerPairKnn * 3)(), (capi.LayerPairOpts * 3)(), (capi.LayerPairGates * 3)()
    knn[0].pairings_per_point = 2
    opts[1].unique_global = 1
    gates[2].run_from_iteration = 2
    st, old = _raw("kbest", pairs, inp.T0, p, opts, gates, knn)
    assert st == 0 and old["n_final_pairs"] > 1000 and min(old["pair_counts"]) > 0
    zeros = (capi.LayerPairPlane * 3)()
    for planes in (None, zeros):
        st, new = _raw("planes", pairs, inp.T0, p, opts, gates, knn, planes=planes)
        assert st == 0
        for key in ("T", "cov"):
            assert np.asarray(new[key]).tobytes() == np.asarray(old[key]).tobytes(), key
        for key in ("n_iterations", "termination_reason", "n_final_pairs", "n_final_pairs_pt2pl", "potential_pairings", "quality",
                    "pair_counts"):
            assert new[key] == old[key], key
        for a, b in zip(new["pairs"], old["pairs"]):
            for key in ("local_idx", "global_idx", "d2"):
                np.testing.assert_array_equal(a[key], b[key])


# ------------------------------------------------------------------------------------------------------ 5. reproducibility
@pytest.mark.parametrize("name", ["off_pose", "rgbd"])
def test_bitwise_equal_with_and_without_bound_and_graphs(ctx, dmaps, all_cases, monkeypatch, name):
    c = all_cases[name]
    runs = [_device(ctx, dmaps, c), _device(ctx, dmaps, c)]
    for var in ("MH_NO_PREV_BOUND", "MH_NO_GRAPH"):
        monkeypatch.setenv(var, "1")
        runs.append(_device(ctx, dmaps, c))
        monkeypatch.delenv(var)
    runs.append(_device(ctx, dmaps, c))
    assert runs[0]["n_iterations"] >= 10 and runs[0]["n_final_pairs_pt2pl"] > 300
    for other in runs[1:]:
        for key in ("T", "cov"):
            assert np.asarray(other[key]).tobytes() == np.asarray(runs[0][key]).tobytes(), key
        for key in ("pair_counts", "n_final_pairs", "n_final_pairs_pt2pl", "potential_pairings", "n_iterations"):
            assert other[key] == runs[0][key], key
        assert [t["n_pairs"] for t in other["trace"]] == [t["n_pairs"] for t in runs[0]["trace"]]
        for a, b in zip(other["pairs"], runs[0]["pairs"]):
            assert sorted(a) == sorted(b)
            for key in a:
                assert a[key].tobytes() == b[key].tobytes(), key


# ------------------------------------------------------------------------------------------------------------ 6. covariance
@pytest.mark.parametrize("name", ["rgbd", "ref_n2000"])
def test_covariance_is_mh_covariance_of_the_union(ctx, dmaps, all_cases, name):
    c = all_cases[name]
    r = _device(ctx, dmaps, c)
    pt = [(e["local"][q["local_idx"]], q["global_xyz"]) for e, q in zip(c["pairs"], r["pairs"]) if not e["plane"]]
    pl = [(e["local"][q["local_idx"]], q["centroid"], q["normal"]) for e, q in zip(c["pairs"], r["pairs"]) if e["plane"]]
    pt2pt = tuple(np.concatenate([b[j] for b in pt]) for j in range(2)) if pt else None
    pt2pl = tuple(np.concatenate([b[j] for b in pl]) for j in range(3))
    co = capi.covariance(ctx, r["T"], pt2pt=pt2pt, pt2pl=pt2pl)
    cg = np.asarray(r["cov"]).reshape(6, 6)
    co = np.asarray(co).reshape(6, 6)
    assert np.abs(co).max() < 1e5  # (not the "nothing to invert" diagonal)
    assert np.allclose(cg, co, rtol=2e-5, atol=1e-6 * np.abs(co).max()), float(np.abs(cg - co).max())


# ---------------------------------------------------------------------------------------------------------------- 7. errors
def test_errors_leave_the_context_usable(ctx, dmaps, inp, all_cases):
    INVALID = 1
    c = all_cases["ref_n700"]
    scan = capi.Scan(ctx, c["pairs"][0]["local"])
    good = dict(map=dmaps["whole"], scan=scan, threshold=c["pairs"][0]["threshold"])
    p = pr.device_params(c)

    def plane(**kw):
        a = (capi.LayerPairPlane * 1)()
        q = dict(pr.RGBD, **kw)
        a[0] = capi.LayerPairPlane(q["knn"], q["minimum_plane_points"], q["plane_eigen_threshold"], q["search_radius"])
        return a

    st, ref = _raw("planes", [good], c["T0"], p, planes=plane())
    assert st == 0 and ref["n_final_pairs"] == ref["n_final_pairs_pt2pl"] > 300

    def again():
        st, r = _raw("planes", [good], c["T0"], p, planes=plane())
        assert st == 0 and np.asarray(r["T"]).tobytes() == np.asarray(ref["T"]).tobytes()

    uniq = (capi.LayerPairOpts * 1)()
    uniq[0].unique_global = 1
    two = (capi.LayerPairKnn * 1)()
    two[0].pairings_per_point = 2
    bad_thr = np.full(c["max_it"], 0.4)
    bad_thr[5] = np.inf
    for kw in (dict(opts=uniq, planes=plane()), dict(knn=two, planes=plane()), dict(planes=plane(knn=2)),
               dict(planes=plane(knn=capi.MAX_PLANE_KNN + 1)), dict(planes=plane(search_radius=0.0)),
               dict(planes=plane(search_radius=float("nan"))), dict(planes=plane(plane_eigen_threshold=float("inf")))):
        assert _raw("planes", [good], c["T0"], p, **kw)[0] == INVALID, kw
        again()
    assert _raw("planes", [dict(good, threshold_angular_deg=0.5)], c["T0"], p, planes=plane())[0] == INVALID
    again()
    assert _raw("planes", [dict(good, threshold=bad_thr)], c["T0"], p, planes=plane())[0] == INVALID
    again()
