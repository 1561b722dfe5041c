"""pairingsPerPoint > 1 on the multi-layer loop, CPU side: the fixed cases of tests/kbest_ref.py on the reference alone -- none is set
apart by tools/fuzz_layers.py's rule (so tests/test_gpu_icp_layers_kbest.py may hold the device to every bit of them), and each
has the property it is there for -- and the binding's signature."""
import ctypes as C

import numpy as np
import pytest

import kbest_ref as kr
from mola_lidar_odometry_amd import capi
from oracle import layers_oracle, oracle_c


@pytest.fixture(scope="module")
def inp(small_workload, oracle):
    return kr.Inputs(small_workload)


@pytest.fixture(scope="module")
def omaps(inp):
    return inp.omaps()


@pytest.fixture(scope="module")
def refs(inp, omaps):
    return {name: (c, kr.case_reference(c, omaps)) for name, c in kr.cases(inp).items()}


def _per_point(local_idx, n):
    return np.bincount(np.asarray(local_idx, np.int64), minlength=n)


def test_no_fixed_case_is_set_apart(refs):
    for name, (c, o) in refs.items():
        near = layers_oracle.nearest_decision(o["margins"])
        print("%-14s iterations %2d, final pairs %5d of %5d, max cond %.2e, nearest decision %s" % (
            name, o["n_iterations"], o["n_final_pairs"], o["potential_pairings"], o["max_cond"], near))
        assert o["n_final_pairs"] > 0, name
        assert o["max_cond"] < 1e10, name
        assert near[1] > 1e-9, (name, near)
        assert not kr.set_apart(o), name


@pytest.mark.parametrize("k", kr.KS)
def test_acceptance_cuts_between_the_ranks(refs, k):
    """first iteration of the whole scan: some points get 0 < accepted < k pairings; and a good share in the final one"""
    c, o = refs["ref_k%d_n2000" % k]
    first = _per_point(o["accepted"][(0, 0)], 2000)
    last = _per_point(o["pairs"][0]["local_idx"], 2000)
    print("k %d: points with 0 < accepted < k: first iteration %d, final %d" % (k, np.sum((first > 0) & (first < k)),
                                                                                 np.sum((last > 0) & (last < k))))
    assert np.sum((first > 0) & (first < k)) > 0
    assert np.sum((last > 0) & (last < k)) >= 200


def test_sparse_map_leaves_trailing_ranks_empty(inp, omaps):
    """no threshold: points whose 27-voxel block holds fewer than k = 3 records, and points whose block holds none"""
    r = oracle_c.match_points_k(omaps["sparse"], inp.scan, inp.T0, 1e3, 3)
    cnt = _per_point(r["local_idx"], len(inp.scan))
    print("records in the block: 0 for %d points, 1-2 for %d, 3 or more for %d" % (np.sum(cnt == 0), np.sum((cnt > 0) & (cnt < 3)),
                                                                               np.sum(cnt == 3)))
    assert np.sum((cnt > 0) & (cnt < 3)) > 50 and np.sum(cnt == 3) > 50


def test_duplicated_map_points_tie(inp, omaps):
    r = oracle_c.match_points_k(omaps["dup"], inp.scan[:700], inp.T0, 1e3, 3)
    same = (r["local_idx"][1:] == r["local_idx"][:-1]) & (r["d2"][1:] == r["d2"][:-1])
    assert np.sum(same) > 300
    assert np.all(r["global_idx"][1:][same] > r["global_idx"][:-1][same])  # the tie goes to the earlier scan position


@pytest.mark.parametrize("name", ["unique_k2", "unique_k21"])
def test_claims_are_lost(refs, name):
    c, o = refs[name]
    acc, kept = sum(len(a) for a in o["accepted"].values()), sum(len(a) for a in o["kept"].values())
    print("%s: accepted %d, kept %d" % (name, acc, kept))
    assert kept < acc
    for g in (p["global_idx"] for p in o["pairs"]):
        assert len(np.unique(g)) == len(g)


def test_gated_potential_follows_k_last(refs):
    c, o = refs["gated"]
    assert o["potential_pairings"] == 700 * 2 + 1300 and len(o["accepted"][(0, 1)]) == 0 and len(o["accepted"][(0, 2)]) > 0
    c, o = refs["gated_short"]  # the loop ends before the pair with k = 2 enters
    assert o["n_iterations"] == 2 and o["potential_pairings"] == 1300


def test_the_bound_case_changes_partners(refs):
    c, o = refs["bound"]
    assert o["n_iterations"] >= 10
    n = [t["n_pairs"] for t in o["trace"]]
    assert len(set(n)) > 5  # the pairings keep changing


def test_previous_partners_leave_the_block(refs, omaps):
    """the case that a bounded search must notice: its k previous partners do not bound the k nearest, and the k-th is accepted"""
    c, o = refs["leave"]
    ev = kr.bound_not_attained(c, o, omaps)
    print("(points whose bound is not attained, with the k-th nearest accepted) per iteration:", ev)
    assert sum(v for _, v in ev) >= 10 and sum(1 for _, v in ev if v) >= 3


def test_binding_declares_the_entry_point():
    assert "mh_icp_align_layers_kbest" in capi._SIGNATURES
    assert C.sizeof(capi.LayerPairKnn) == 4
    assert hasattr(capi.lib(), "mh_icp_align_layers_kbest")
