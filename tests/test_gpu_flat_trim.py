"""-m gpu: the plan / scan matcher (MH_MATCH=f, mh_nn_flat.h) at the edges of its waves, probe passes and record rounds.

k_match_flat / k_match_flat_b form the byte offsets of their gathers in 32 bits on scalar bases when the map and the scan allow it
(flat_off32, mh_k_launch.h).  That may not change a result, so every case here is held to the repository's CPU oracle as
tests/test_gpu_parity.py does -- final pairings (local_idx, global_idx, d2) bit-equal, n_final_pairs equal, poses within that
file's 1e-7 -- and to the quad matcher (MH_MATCH=q) bit for bit, with max_iterations 1, 2, 3 and 4 (stall test off): the first pins
the unbounded iteration, the others the bounded ones.

  scan length   1, 63, 64, 65, 128, 129, 1000 points: a wave and its neighbours' edges;
  slot counts   the same cube at ~1, 4, 12 and 20 points per occupied voxel, guesses 0.02, 0.2 and 0.6 m off, 8000 points: the waves'
                candidate counts fall in every class <= 64, 65-128, 129-192, 193-256, > 256 (one to four probe passes and a second
                round of them; the chunk counts that follow fill the last record round to every degree), counted here from the
                oracle's poses alone and asserted;
  ties, empties voxels filled to the cap with one coordinate (the lowest scan position wins), points whose own voxel is empty, points
                with no record in their 27-voxel block;
  batch         nine jobs in lock step (eight dealt an XCD each, one in plain order) against single alignments and the oracle.

The 64-bit-offset instantiation of the kernels takes a map or scan of 2^32 bytes or more: not reachable at test size; it is the
kernels' earlier code, instruction for instruction (profiles/flat_trim.md)."""
import functools

import numpy as np
import pytest

from mola_lidar_odometry_amd import capi

pytestmark = pytest.mark.gpu

POSE_TOL = 1e-7  # tests/test_gpu_parity.py's
VS, CAP, HALF = 1.0, 20, 6.0  # a 12 m cube of 1 m voxels, centred: negative and positive voxel indices
ITS = (1, 2, 3, 4)
SIZES = (1, 63, 64, 65, 128, 129, 1000)
MAP_POINTS = {1: 1728, 4: 6912, 12: 20736, 20: 48000}  # ~ points per occupied voxel (12^3 voxels, cap 20) -> points offered
OFFSETS = (0.02, 0.2, 0.6)
THRESHOLD, KERNEL_PARAM = 1.0, 0.5
CLASSES = ("<=64", "65-128", "129-192", "193-256", ">256")
PRIOR_INFO = np.eye(6) * np.array([50.0, 50.0, 50.0, 200.0, 200.0, 200.0])


def pose(x, y, z, yaw, pitch, roll):
    cy, sy, cp, sp, cr, sr = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    R = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1.0]]) @ np.array([[cp, 0, sp], [0, 1, 0], [-sp, 0, cp]]) @ \
        np.array([[1, 0, 0], [0, cr, -sr], [0, sr, cr]])
    return np.ascontiguousarray(np.concatenate([R, np.array([[x], [y], [z]])], 1).reshape(-1))


T_GT = pose(0.30, -0.20, 0.10, np.deg2rad(3.0), np.deg2rad(1.0), np.deg2rad(-0.5))


def guess(off):
    """T_GT moved `off` metres (and off / 50 rad of yaw)"""
    return pose(0.30 + 0.60 * off, -0.20 - 0.64 * off, 0.10 + 0.48 * off, np.deg2rad(3.0) + off / 50.0, np.deg2rad(1.0), np.deg2rad(-0.5))


def cube_map(n, seed=7001):
    return np.ascontiguousarray(np.random.default_rng(seed).uniform(-HALF, HALF, (n, 3)), np.float32)


def pull_back(world, T, rng, noise):
    T = np.asarray(T, np.float64).reshape(3, 4)
    loc = (np.asarray(world, np.float64) - T[:, 3]) @ T[:, :3]  # R^T (p - t)
    return np.ascontiguousarray(loc + rng.normal(0.0, noise, loc.shape) if noise else loc, np.float32)


def cube_scan(mp, n, noise, seed):
    rng = np.random.default_rng(seed)
    return pull_back(mp[rng.choice(len(mp), n, replace=n > len(mp))], T_GT, rng, noise)


def transform(local, T):
    """the matchers' transform: fp64 pose times fp32 point, rounded to fp32"""
    T = np.asarray(T, np.float64).reshape(-1)[:12].reshape(3, 4)
    x, y, z = np.asarray(local, np.float32).astype(np.float64).T
    return np.stack([((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3)], 1).astype(np.float32)


def params(mod, n_it):
    return mod.ICPParams(max_iterations=n_it, threshold=THRESHOLD, kernel_param=KERNEL_PARAM, disable_stall_test=True)


def prior_for(n):
    """a layer of a few points does not hold six dimensions: a weak prior 2 cm off the true pose keeps its normal equations
    conditioned (a few dozen points outweigh it)"""
    if n >= 700:
        return None
    Tp = T_GT.copy()
    Tp[3] += 0.02
    return (Tp, PRIOR_INFO)


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


class Refs:
    """The oracle's side of a (map, scan, guess): computed once, shared by the tests that need it, never written to."""

    def __init__(self, oracle, mp, scan, T0):
        self.mp, self.scan, self.T0 = mp, scan, T0
        self.om = oracle.Map(VS, CAP).insert(mp)
        self.prior = prior_for(len(scan))
        self.runs = {k: oracle.icp_align(self.om, scan, T0, params(oracle, k), prior=self.prior, want_pairs=True) for k in ITS}


def assert_case(ctx, ref, monkeypatch, gm=None):
    """MH_MATCH=f against the oracle and against MH_MATCH=q, max_iterations 1 .. 4"""
    gm = gm or capi.Map(ctx, VS, CAP).build(ref.mp)
    gs = capi.Scan(ctx, ref.scan)
    for k in ITS:
        o = ref.runs[k]
        got = {}
        for match in ("f", "q"):
            monkeypatch.setenv("MH_MATCH", match)
            got[match] = capi.icp_align(gm, gs, ref.T0, params(capi, k), prior=ref.prior, want_pairs=True)
        f, q = got["f"], got["q"]
        assert f["n_iterations"] == o["n_iterations"] and f["n_final_pairs"] == o["n_final_pairs"], k
        assert [t["n_pairs"] for t in f["trace"]] == [t["n_pairs"] for t in o["trace"]], k
        for key in ("local_idx", "global_idx", "d2"):
            np.testing.assert_array_equal(f["pairs"][key], o["pairs"][key], err_msg="%s, max_iterations %d" % (key, k))
            np.testing.assert_array_equal(f["pairs"][key], q["pairs"][key], err_msg="%s vs q, max_iterations %d" % (key, k))
        np.testing.assert_allclose(f["T"], o["T"], atol=POSE_TOL, rtol=0)
        assert np.asarray(f["T"]).tobytes() == np.asarray(q["T"]).tobytes(), k
        assert np.asarray(f["cov"]).tobytes() == np.asarray(q["cov"]).tobytes(), k
    return gm


# ------------------------------------------------------------------------------------------------------------ scan length
@functools.lru_cache(maxsize=None)
def _length_inputs():
    mp = cube_map(MAP_POINTS[12])
    return mp, cube_scan(mp, max(SIZES), 0.01, 7002)


@pytest.fixture(scope="module")
def length_map(ctx):
    return capi.Map(ctx, VS, CAP).build(_length_inputs()[0])


@pytest.mark.parametrize("n", SIZES)
def test_scan_lengths_around_a_wave(ctx, oracle, length_map, n, monkeypatch):
    mp, scan = _length_inputs()
    assert_case(ctx, Refs(oracle, mp, scan[:n], guess(0.2)), monkeypatch, gm=length_map)


# ------------------------------------------------------------------------------------------------------------ slot counts
def candidate_counts(oracle, ref):
    """Candidate voxels per wave of 64 consecutive points for the bounded iterations 1 .. 3, from the oracle's poses alone: the bound
    of a point is its squared distance to the record it was nearest to one iteration earlier, a voxel of its 27-voxel block is a
    candidate when the squared axis gaps to it sum to no more than that bound, and a point with more than eight candidates (or
    without an earlier partner) is not planned.  The matcher's own count differs by its rounding margins only."""
    poses = [ref.T0] + [t["T"] for t in ref.runs[max(ITS)]["trace"]]
    out = []
    for j in range(1, max(ITS)):
        prev = oracle.match_points(ref.om, ref.scan, poses[j - 1], 1.0e3)  # every point with a record in its block
        p = transform(ref.scan, poses[j]).astype(np.float64)
        b0 = np.full(len(p), -1.0)
        b0[prev["local_idx"]] = ((prev["global_xyz"].astype(np.float64) - p[prev["local_idx"]]) ** 2).sum(1)
        lo = p / VS - np.floor(p / VS)          # distance to the voxel's lower / upper face, in voxels
        gaps = np.stack([(lo * VS) ** 2, np.zeros_like(lo), ((1.0 - lo) * VS) ** 2], 2)  # [point, axis, side]
        lb = gaps[:, 0, :, None, None] + gaps[:, 1, None, :, None] + gaps[:, 2, None, None, :]
        cand = (lb <= b0[:, None, None, None]).reshape(len(p), 27).sum(1)
        cand[(cand > 8) | (b0 < 0)] = 0
        pad = (-len(cand)) % 64
        out.append(np.concatenate([cand, np.zeros(pad, cand.dtype)]).reshape(-1, 64).sum(1))
    return np.concatenate(out)


def classes_of(counts):
    edges = np.array([64, 128, 192, 256])
    return {CLASSES[i] for i in np.unique(np.searchsorted(edges, counts[counts > 0], side="left"))}


@functools.lru_cache(maxsize=None)
def _slot_inputs(ppv, off):
    mp = cube_map(MAP_POINTS[ppv])
    # (a scan of the map's own points: with the guess 2 cm off its bounds shrink to nothing, one candidate per point)
    return mp, cube_scan(mp, 8000, 0.0 if off == OFFSETS[0] else 0.01, 7100 + ppv), guess(off)


_slot_refs = {}


def slot_ref(oracle, ppv, off):
    if (ppv, off) not in _slot_refs:
        _slot_refs[(ppv, off)] = Refs(oracle, *_slot_inputs(ppv, off))
    return _slot_refs[(ppv, off)]


def test_the_inputs_reach_every_class_of_candidate_count(oracle):
    """Otherwise the pass and round boundaries are not exercised: one, two, three and four probe passes, and a second round of them."""
    seen = set()
    for ppv in MAP_POINTS:
        for off in OFFSETS:
            seen |= classes_of(candidate_counts(oracle, slot_ref(oracle, ppv, off)))
    assert seen == set(CLASSES), sorted(seen)


@pytest.mark.parametrize("off", OFFSETS)
@pytest.mark.parametrize("ppv", sorted(MAP_POINTS))
def test_slot_counts(ctx, oracle, ppv, off, monkeypatch):
    assert_case(ctx, slot_ref(oracle, ppv, off), monkeypatch)


# ------------------------------------------------------------------------------------------------------- ties and empties
N_TIED, COPIES = 24, 25  # voxels that hold one coordinate COPIES times: the cap keeps the first 20


def _ties_inputs():
    rng = np.random.default_rng(7200)
    # the cube without its x > 2 part; the tied voxels' points first (copy r of voxel v at index r * N_TIED + v): they fill the cap
    cells = np.stack(np.meshgrid(np.arange(-5, 1), np.arange(-2, 2), [0], indexing="ij"), -1).reshape(-1, 3)[:N_TIED]
    tied = (cells + np.array([0.37, 0.61, 0.29])).astype(np.float32)
    rest = cube_map(4000, 7201)
    rest = rest[rest[:, 0] < 2.0]
    mp = np.ascontiguousarray(np.concatenate([np.tile(tied, (COPIES, 1)), rest]), np.float32)
    near_tied = tied[rng.integers(0, N_TIED, 200)] + rng.normal(0.0, 0.03, (200, 3))
    own_empty = np.stack([rng.uniform(2.2, 2.8, 150), rng.uniform(-5.5, 5.5, 150), rng.uniform(-5.5, 5.5, 150)], 1)
    nothing = np.stack([rng.uniform(4.2, 5.8, 100), rng.uniform(-5.5, 5.5, 100), rng.uniform(-5.5, 5.5, 100)], 1)
    plain = rest[rng.choice(len(rest), 250, replace=False)] + rng.normal(0.0, 0.01, (250, 3))
    kind = np.repeat(np.arange(4), [200, 150, 100, 250])
    order = rng.permutation(len(kind))
    world = np.concatenate([near_tied, own_empty, nothing, plain])[order]
    return mp, pull_back(world, T_GT, rng, 0.0), kind[order]


def test_ties_at_the_cap_empty_own_voxels_and_empty_blocks(ctx, oracle, monkeypatch):
    mp, scan, kind = _ties_inputs()
    ref = Refs(oracle, mp, scan, guess(0.02))
    # what the case is there for, on the oracle alone
    dump = ref.om.dump()
    keys = {tuple(k) for k in np.asarray(dump["vox_keys"]).astype(np.int64).tolist()}
    full = {tuple(k) for k, c in zip(np.asarray(dump["vox_keys"]).astype(np.int64).tolist(), np.asarray(dump["vox_count"]).tolist()) if c == CAP}
    vox = np.floor(transform(scan, ref.T0) * np.float32(1.0 / VS)).astype(np.int64)
    own = np.array([tuple(v) in keys for v in vox.tolist()])
    block = np.array([any((v[0] + a, v[1] + b, v[2] + c) in keys for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1))
                      for v in vox.tolist()])
    assert (~own & block).sum() >= 100 and (~block).sum() >= 80 and len(full) >= N_TIED
    for k in ITS:
        pr = ref.runs[k]["pairs"]
        assert ref.runs[k]["n_final_pairs"] < len(scan) - 80                  # the points without a record in their block stay unpaired
        tied = pr["global_idx"] < N_TIED * COPIES
        assert tied.sum() >= 150 and (pr["global_idx"][tied] < N_TIED).all()   # twenty equal distances: the first copy wins
        assert (kind[pr["local_idx"]] == 1).sum() >= 100                      # paired from a neighbour of their empty voxel
    assert_case(ctx, ref, monkeypatch)


# ------------------------------------------------------------------------------------------------------------------ batch
BATCH_SIZES = (1, 63, 64, 65, 128, 129, 1000, 64, 129)


def test_nine_jobs_in_lock_step(ctx, oracle, length_map, monkeypatch):
    """gridDim.y = 9: the first eight jobs are dealt an XCD each, the ninth keeps the plain order (k_match_flat_b)"""
    mp, scan = _length_inputs()
    om = oracle.Map(VS, CAP).insert(mp)
    rng = np.random.default_rng(7300)
    subs = [np.ascontiguousarray(scan[rng.permutation(len(scan))[:n]]) for n in BATCH_SIZES]
    guesses = [guess(off) for off in (0.2, 0.02, 0.2, 0.6, 0.02, 0.2, 0.6, 0.2, 0.02)]
    priors = [prior_for(1)] * len(BATCH_SIZES)  # the weak prior for every job: one group (the 1000-point job's data outweigh it)
    monkeypatch.setenv("MH_MATCH", "f")
    ctxs = [capi.Context(0) for _ in BATCH_SIZES]
    scans = [capi.Scan(c, s) for c, s in zip(ctxs, subs)]
    nbytes = sum(capi.pairs_block_bytes(n) for n in BATCH_SIZES)
    for k in ITS:
        singles = [capi.icp_align(length_map, capi.Scan(ctx, s), g, params(capi, k), prior=pr, want_trace=False, want_pairs=True)
                   for s, g, pr in zip(subs, guesses, priors)]
        block = np.zeros(nbytes, np.uint8)
        res = capi.icp_align_batch([length_map] * len(scans), scans, guesses, params(capi, k), priors=priors, pairs_block=block)
        ctxs[0].synchronize()
        for s, g, pr, a, r, bp in zip(subs, guesses, priors, singles, res, capi.unpack_pairs_block(block, list(BATCH_SIZES), res)):
            o = oracle.icp_align(om, s, g, params(oracle, k), prior=pr, want_pairs=True)
            assert (r["n_iterations"], r["n_final_pairs"]) == (a["n_iterations"], a["n_final_pairs"]) == (o["n_iterations"], o["n_final_pairs"])
            assert np.array_equal(r["T"], a["T"]) and np.array_equal(r["cov"], a["cov"])
            np.testing.assert_allclose(r["T"], o["T"], atol=POSE_TOL, rtol=0)
            for key in ("local_idx", "global_idx", "d2"):
                assert np.array_equal(bp[key], a["pairs"][key]), (k, key)
                assert np.array_equal(bp[key], o["pairs"][key]), (k, key)
    for c in ctxs:
        c.close()

