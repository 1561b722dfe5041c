"""The references of tests/test_gpu_far_origin.py are sound far from the origin, shown on the CPU from the references alone
(tests/far_cases.py: the inputs of tests/dense_cases.py shifted by D1 = 4 km, D2 = 52 km, D3 = 410 km): no case is set apart by
tools/fuzz_layers.py's rule (allowed share: zero); the two CPU implementations of the alignment -- oracle_c (C, its own sums and
solve) and layers_oracle (same matcher, float64 numpy solve) -- agree as tests/test_dense_cpu.py asserts near the origin; the
oracle's nearest neighbours are those of the float64-free exhaustive restatement dense_cases.brute_force_k; partners still
change between iterations at the largest offset.  The printed spreads are recorded in profiles/far_origin.md."""
import numpy as np
import pytest

import dense_cases as dc
import far_cases as fc
from oracle import layers_oracle, oracle_c

NAMES = list(fc.OFFSETS)


class _Once:
    """references computed once per module, on first use, and left unchanged"""

    def __init__(self, make):
        self.make, self.done = make, {}

    def __getitem__(self, key):
        if key not in self.done:
            self.done[key] = self.make(key)
        return self.done[key]


@pytest.fixture(scope="module")
def far(oracle):
    """offset name -> (inputs, oracle maps)"""
    def make(name):
        inp = fc.far_inputs(fc.OFFSETS[name])
        return inp, inp.omaps()
    return _Once(make)


@pytest.fixture(scope="module")
def singles(far):
    """(offset, map, n) -> oracle_c.icp_align with pairs, the 16-iteration single pair"""
    def make(key):
        name, mk, n = key
        inp, omaps = far[name]
        return oracle_c.icp_align(omaps[mk], dc.single_scan(inp, n), inp.T0, dc.single_params(oracle_c), prior=dc.single_prior(inp, n),
                                  want_pairs=True)
    return _Once(make)


SINGLE_KEYS = [(mk, n) for mk in fc.SINGLE_MAPS + ("room07",) for n in fc.SINGLE_SIZES]


@pytest.mark.parametrize("name", NAMES)
def test_no_case_is_set_apart_far_from_the_origin(far, singles, name):
    """test_dense_cpu.py::test_no_case_is_set_apart at every offset: single pairs on room and mixed (and on room07, the odd voxel
    size) with 129 and 2561 points, and every multi-layer case.  The two CPU implementations agree on the single pairs: same
    iteration and pair counts, poses within 1e-9."""
    inp, omaps = far[name]
    apart, total, spread = [], 0, 0.0
    for mk, n in SINGLE_KEYS:
        o = singles[(name, mk, n)]
        p = dc.single_params(oracle_c)
        lo = layers_oracle.icp_align_layers([dict(map=omaps[mk], local=dc.single_scan(inp, n), threshold=p.threshold)], inp.T0, p,
                                            prior=dc.single_prior(inp, n))
        assert lo["n_iterations"] == o["n_iterations"] and [t["n_pairs"] for t in lo["trace"]] == [t["n_pairs"] for t in o["trace"]]
        d = float(np.abs(lo["T"] - o["T"]).max())
        spread = max(spread, d)
        assert d < 1e-9, (name, mk, n, d)
        print("%s single %-6s n %4d: max cond %.2e, nearest decision %s, final pairs %d, |oracle_c - layers_oracle| %.2e" % (
            name, mk, n, lo["max_cond"], layers_oracle.nearest_decision(lo["margins"]), o["n_final_pairs"], d))
        total += 1
        if dc.set_apart(lo):
            apart.append((mk, n))
        assert o["n_final_pairs"] > 0
    for cname, c in dc.cases(inp).items():
        o = dc.case_reference(c, omaps)
        print("%s %-14s iterations %2d, final pairs %5d of %5d, max cond %.2e, nearest decision %s" % (
            name, cname, o["n_iterations"], o["n_final_pairs"], o["potential_pairings"], o["max_cond"],
            layers_oracle.nearest_decision(o["margins"])))
        total += 1
        if dc.set_apart(o):
            apart.append(cname)
        assert o["n_final_pairs"] > 0, cname
    print("%s: %d of %d cases set apart; pose spread of the two CPU implementations %.2e" % (name, len(apart), total, spread))
    assert not apart, apart


@pytest.mark.parametrize("k", [1, 2, 8])
@pytest.mark.parametrize("mk", ["room", "centres", "room07"])
@pytest.mark.parametrize("name", NAMES)
def test_oracle_neighbours_are_the_brute_force_s(far, name, mk, k):
    """oracle_c.match_points_k against dense_cases.brute_force_k over the dumped map: fp32 only, ties by record index.  room (and
    room07): the first 600 scan points under the first guess, threshold 1.5; centres: the lattice queries, threshold 0.2."""
    inp, omaps = far[name]
    if mk == "centres":
        world, local, T, thr = inp.queries, inp.queries, dc.IDENTITY, 0.2
    else:
        local, T, thr = inp.scan[:600], inp.T0, 1.5
        world = dc.transform(local, T)
    d = omaps[mk].dump()
    vs = inp.maps[mk][1]
    best = _brute(d, world, k, thr, vs)
    o = oracle_c.match_points_k(omaps[mk], local, T, thr, k)
    li = np.array([i for i, b in enumerate(best) for _ in b], np.uint32)
    gi = np.array([d["src_idx"][r] for b in best for r, _ in b], np.uint32)
    d2 = np.array([v for b in best for _, v in b], np.float32)
    assert len(li) > len(world) // 2
    np.testing.assert_array_equal(o["local_idx"], li)
    np.testing.assert_array_equal(o["global_idx"], gi)
    np.testing.assert_array_equal(o["d2"], d2)
    ties = sum(1 for b in best if len(b) >= 2 and b[0][1] == b[1][1])
    print("%s %s k %d: %d pairings, %d of %d points tie in their two smallest accepted d2" % (name, mk, k, len(li), ties, len(world)))


def _brute(dump, world, k, thr, vs):
    """dense_cases.brute_force_k, whose voxel rule is written for the 1 m voxel: the points and the table scaled by 1 / vs would
    change the arithmetic, so for another voxel size the table is keyed by the dump's own indices and the query's voxel comes
    from floor(p * (float)(1 / vs)) -- DESIGN 3.1's rule, as dense_cases.voxel_keys states it."""
    if vs == dc.VS:
        return dc.brute_force_k(dump, world, k, thr)
    xyz = np.asarray(dump["xyz"], np.float32)
    first, count = np.asarray(dump["vox_first"]).astype(np.int64), dc.occupancy(dump)
    table = {tuple(kk): (int(f), int(c)) for kk, f, c in zip(np.asarray(dump["vox_keys"]).astype(np.int64).tolist(), first.tolist(),
                                                              count.tolist())}
    thr2 = np.float32(np.float64(thr) * np.float64(thr))
    out = []
    for p, key in zip(np.asarray(world, np.float32), dc.voxel_keys(world, vs).tolist()):
        idx = [np.arange(fc_[0], fc_[0] + fc_[1]) for fc_ in (table.get((key[0] + a, key[1] + b, key[2] + c))
                                                             for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1)) if fc_]
        if not idx:
            out.append([])
            continue
        idx = np.concatenate(idx)
        e = xyz[idx] - p
        d2 = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
        order = np.lexsort((idx, d2))[:k]
        out.append([(int(idx[j]), np.float32(d2[j])) for j in order if d2[j] < thr2])
    return out


def test_partners_change_between_iterations_at_the_largest_offset(far, singles):
    """test_dense_cpu.py::test_partners_change_between_iterations at D3: a far case that pairs once and never changes partners
    would test nothing"""
    inp, omaps = far["D3"]
    for mk, n in SINGLE_KEYS:
        o = singles[("D3", mk, n)]
        scan, thr = dc.single_scan(inp, n), dc.schedule(dc.SINGLE_IT)
        poses = [inp.T0] + [t["T"] for t in o["trace"]]
        changed, prev = 0, None
        for j in range(4):
            m = oracle_c.match_points(omaps[mk], scan, poses[j], float(thr[j]))
            cur = dict(zip(m["local_idx"].tolist(), m["global_idx"].tolist()))
            if prev is not None:
                changed += sum(1 for i, g in cur.items() if i in prev and prev[i] != g)
            prev = cur
        print("D3 single %-6s n %4d: %d partner changes over iterations 1-3" % (mk, n, changed))
        assert changed > 0, (mk, n)


def test_the_odd_voxel_size_disagrees_with_its_slabs(far):
    """What room07 is there for, from the dump alone: records whose voxel index (floor(p * (float)(1 / vs))) and whose slab
    [(float)v * vs, (float)(v + 1) * vs) disagree, by ulps of the coordinate -- none under the power-of-two voxels."""
    for name in NAMES:
        inp, _ = far[name]
        out = {}
        for mk in ("room", "room07"):
            pts, vs = inp.maps[mk][0], np.float32(inp.maps[mk][1])
            v = dc.voxel_keys(pts, float(vs)).astype(np.float32)
            out[mk] = int(((pts < v * vs) | (pts >= (v + np.float32(1.0)) * vs)).any(axis=1).sum())
        print("%s: records outside the slab of their voxel: room %d, room07 %d of %d" % (name, out["room"], out["room07"], len(pts)))
        assert out["room"] == 0
        if name != "D1":
            assert out["room07"] > 0


# ------------------------------------------------------------------------------------------- the covariance far from the origin
def _pose_of(v, dt):
    """R = Rz(yaw) Ry(pitch) Rx(roll), t = (x, y, z) in the arithmetic dt: the contract's pose of (x, y, z, yaw, pitch, roll)"""
    x, y, z, yaw, pitch, roll = np.asarray(v, dt)
    cy, sy, cp, sp, cr, sr = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    return np.array([[cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr, x], [sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr, y],
                     [-sp, cp * sr, cp * cr, z]], dt)


def covariance_extended(T, local, h=1e-7):
    """(A^T A)^-1 of the point pairings' central-difference Jacobian with every f(x + h) and f(x - h) formed per pairing in
    numpy's long double (64 mantissa bits on x86): eps |t| / h is 2e-7 there at 4.1e5 m, where it is 4.6e-4 in double."""
    LD = np.longdouble
    T = np.asarray(T, np.float64).reshape(3, 4)
    v = np.array([T[0, 3], T[1, 3], T[2, 3], np.arctan2(T[1, 0], T[0, 0]), -np.arcsin(T[2, 0]), np.arctan2(T[2, 1], T[2, 2])], LD)
    L = np.asarray(local, np.float32).astype(LD)
    cols = []
    for j in range(6):
        vp, vm = v.copy(), v.copy()
        vp[j] += LD(h)
        vm[j] -= LD(h)
        P, M = _pose_of(vp, LD), _pose_of(vm, LD)
        cols.append(((L @ P[:, :3].T + P[:, 3]) - (L @ M[:, :3].T + M[:, 3])) / (2 * LD(h)))
    A = np.stack(cols, 2).reshape(-1, 6)
    return np.linalg.inv((A.T @ A).astype(np.float64))


@pytest.mark.parametrize("name", NAMES)
def test_oracle_covariance_against_extended_precision(far, name):
    """The GPU tests hold the device's covariance to oracle_c's at rtol 2e-5, atol 1e-6 max|cov| (test_gpu_solver_params.py).  So
    must the oracle itself be to the same central difference taken in extended precision, for small layers too: a difference
    formed per pairing in double carries eps |t| / h of rounding into every entry of A, which 63 pairings do not average away
    (3.3 times the tolerance at D3 before oracle_c differenced the pose instead; profiles/far_origin.md)."""
    inp, omaps = far[name]
    for n in (63, 129, 2561):
        o = oracle_c.icp_align(omaps["room"], dc.single_scan(inp, n), inp.T0, dc.single_params(oracle_c), prior=dc.single_prior(inp, n),
                               want_pairs=True)
        ref = covariance_extended(o["T"], dc.single_scan(inp, n)[o["pairs"]["local_idx"]])
        cov = np.asarray(o["cov"]).reshape(6, 6)
        share = float((np.abs(cov - ref) / (2e-5 * np.abs(ref) + 1e-6 * np.abs(ref).max())).max())
        print("%s n %4d: oracle_c covariance against the extended-precision difference: %.2f of the tolerance" % (name, n, share))
        np.testing.assert_allclose(cov, ref, rtol=2e-5, atol=1e-6 * np.abs(ref).max())
