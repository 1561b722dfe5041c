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
  batch         1, 7, 8, 9, 16 and 17 jobs in lock step (k_match_flat_b deals whole groups of eight jobs an XCD each: 0, 0, 8, 8, 16, 16
                of them, and keeps 1, 7, 0, 1, 0, 1 in plain order) against single alignments and the oracle;
  graph cache   the switch below toggled under a warm graph cache: the replayed chunk is the decided instantiation's.

Both instantiations of the kernels run every case: the 32-bit-offset one as the sizes here select it, and the 64-bit-offset one --
which a map buffer above 2^32 bytes or a scan above 2^28 points selects, out of reach at test size -- under MH_NO_OFF32=1.  They
give the same bits, so a result cannot tell which of them ran: the library counts the launches of each where they are issued, a
captured graph's on every replay (capi.flat_stats), and every device run here is held to "only the counter of the instantiation
the switch names moved".  The rule that chooses between them, at its boundary: tests/test_flat_off32_cpu.py."""
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


FLAT, FLAT_WIDE, FLAT_B, FLAT_B_WIDE = range(4)  # capi.flat_stats(): k_match_flat<true>, <false>, k_match_flat_b<true>, <false>


def moved(before):
    """what the launch counters have gained since `before`"""
    return tuple(a - b for a, b in zip(capi.flat_stats(), before))


def only(which, count):
    out = [0, 0, 0, 0]
    out[which] = count
    return tuple(out)


def set_instantiation(monkeypatch, wide):
    """wide: MH_NO_OFF32=1, the 64-bit-offset kernels"""
    if wide:
        monkeypatch.setenv("MH_NO_OFF32", "1")
    else:
        monkeypatch.delenv("MH_NO_OFF32", raising=False)


def assert_case(ctx, ref, monkeypatch, gm=None):
    """MH_MATCH=f, as it is and with MH_NO_OFF32=1, against the oracle and against MH_MATCH=q, max_iterations 1 .. 4"""
    gm = gm or capi.Map(ctx, VS, CAP).build(ref.mp)
    gs = capi.Scan(ctx, ref.scan)
    for k in ITS:
        o = ref.runs[k]
        set_instantiation(monkeypatch, False)
        monkeypatch.setenv("MH_MATCH", "q")
        c0 = capi.flat_stats()
        q = capi.icp_align(gm, gs, ref.T0, params(capi, k), prior=ref.prior, want_pairs=True)
        assert moved(c0) == (0, 0, 0, 0), k  # (the quad matcher is not the plan / scan matcher)
        monkeypatch.setenv("MH_MATCH", "f")
        for wide in (False, True):
            set_instantiation(monkeypatch, wide)
            c0 = capi.flat_stats()
            f = capi.icp_align(gm, gs, ref.T0, params(capi, k), prior=ref.prior, want_pairs=True)
            # one k_match_flat launch per enqueued iteration, all of the instantiation the switch names, none of the other or of
            # the batch kernels -- else the comparisons below have checked the wrong kernel
            assert f["n_enqueued_iterations"] >= max(1, f["n_iterations"]), (k, wide)
            assert moved(c0) == only(FLAT_WIDE if wide else FLAT, f["n_enqueued_iterations"]), (k, wide)
            assert f["n_iterations"] == o["n_iterations"] and f["n_final_pairs"] == o["n_final_pairs"], (k, wide)
            assert [t["n_pairs"] for t in f["trace"]] == [t["n_pairs"] for t in o["trace"]], (k, wide)
            for key in ("local_idx", "global_idx", "d2"):
                np.testing.assert_array_equal(f["pairs"][key], o["pairs"][key], err_msg="%s, max_iterations %d, wide %d" % (key, k, wide))
                np.testing.assert_array_equal(f["pairs"][key], q["pairs"][key], err_msg="%s vs q, max_iterations %d, wide %d" % (key, k, wide))
            np.testing.assert_allclose(f["T"], o["T"], atol=POSE_TOL, rtol=0)
            assert np.asarray(f["T"]).tobytes() == np.asarray(q["T"]).tobytes(), (k, wide)
            assert np.asarray(f["cov"]).tobytes() == np.asarray(q["cov"]).tobytes(), (k, wide)
    set_instantiation(monkeypatch, False)
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


BATCH_OFFSETS = (0.2, 0.02, 0.2, 0.6, 0.02, 0.2, 0.6, 0.2, 0.02)
JOB_COUNTS = (1, 7, 8, 9, 16, 17)


@functools.lru_cache(maxsize=None)
def _batch_inputs():
    """the jobs of the largest batch; a smaller one takes the first of them (sizes and guesses go round BATCH_SIZES / BATCH_OFFSETS)"""
    _, scan = _length_inputs()
    rng = np.random.default_rng(7300)
    sizes = [BATCH_SIZES[i % len(BATCH_SIZES)] for i in range(max(JOB_COUNTS))]
    subs = [np.ascontiguousarray(scan[rng.permutation(len(scan))[:n]]) for n in sizes]
    return sizes, subs, [guess(BATCH_OFFSETS[i % len(BATCH_OFFSETS)]) for i in range(len(sizes))]


_batch_refs = {}


def batch_ref(oracle, i, k):
    """the oracle's alignment of job i with max_iterations k: computed once, shared by every batch that holds the job"""
    if not _batch_refs:
        _batch_refs["map"] = oracle.Map(VS, CAP).insert(_length_inputs()[0])
    if (i, k) not in _batch_refs:
        _, subs, guesses = _batch_inputs()
        _batch_refs[(i, k)] = oracle.icp_align(_batch_refs["map"], subs[i], guesses[i], params(oracle, k), prior=prior_for(1), want_pairs=True)
    return _batch_refs[(i, k)]


@pytest.fixture(scope="module")
def batch_ctxs():
    cs = [capi.Context(0) for _ in range(max(JOB_COUNTS))]
    yield cs
    for c in cs:
        c.close()


@pytest.mark.parametrize("wide", [False, True], ids=["off32", "off64"])
@pytest.mark.parametrize("jobs", JOB_COUNTS)
def test_jobs_in_lock_step(ctx, oracle, length_map, batch_ctxs, jobs, wide, monkeypatch):
    """gridDim.y = jobs: k_match_flat_b deals the first 8 * floor(jobs / 8) jobs an XCD each, the others keep the plain order -- none
    dealt (7 jobs), all dealt (8, 16), one left over (9, 17) -- in both instantiations, against single alignments and the oracle.

    The launch counters: the batch call moves the counter of k_match_flat_b in the instantiation the switch names and no other, by
    no more than max_iterations (a group never enqueues more iterations than its longest job may run) and no less than the
    iterations its longest job ran -- with the stall test off that is max_iterations for any job that still finds pairs, so the
    count is exact then; with two jobs or more it is below jobs x max_iterations: the jobs shared their launches.

    A batch of ONE job has no lock-step group (a job alone in its group gains nothing from one: form_groups): it takes the
    single-alignment chain, chunk by chunk, and the counter that moves is k_match_flat's.  gridDim.y = 1 does not occur.

    What no result shows: WHICH jobs are dealt.  The dealing is a bijection of (block, job) for any `whole` that is a multiple of
    eight and at most the job count, so `gridDim.y & ~15u` in place of `& ~7u` passes here (tried): it only changes which XCD's L2
    fetches a map, which is the benchmark's to see.  A `whole` that is no multiple of eight, or exceeds the job count, reads job
    descriptors that do not exist."""
    sizes, subs, guesses = (v[:jobs] for v in _batch_inputs())
    priors = [prior_for(1)] * jobs  # the weak prior for every job: one group (the 1000-point job's data outweigh it)
    monkeypatch.setenv("MH_MATCH", "f")
    set_instantiation(monkeypatch, wide)
    scans = [capi.Scan(c, s) for c, s in zip(batch_ctxs, subs)]
    nbytes = sum(capi.pairs_block_bytes(n) for n in sizes)
    if jobs == 1:
        want = FLAT_WIDE if wide else FLAT
    else:
        want = FLAT_B_WIDE if wide else FLAT_B
    for k in ITS:
        c0 = capi.flat_stats()
        singles = [capi.icp_align(length_map, capi.Scan(ctx, s), g, params(capi, k), prior=pr, want_trace=False, want_pairs=True)
                   for s, g, pr in zip(subs, guesses, priors)]
        assert moved(c0) == only(FLAT_WIDE if wide else FLAT, sum(a["n_enqueued_iterations"] for a in singles)), k
        block = np.zeros(nbytes, np.uint8)
        c0 = capi.flat_stats()
        res = capi.icp_align_batch([length_map] * jobs, scans, guesses, params(capi, k), priors=priors, pairs_block=block)
        batch_ctxs[0].synchronize()
        launches = moved(c0)
        ran = max(r["n_iterations"] for r in res)
        assert launches == only(want, launches[want]) and max(1, ran) <= launches[want] <= k, (k, launches, ran)
        assert jobs == 1 or launches[want] < jobs * k, (k, launches)
        for i, (a, r, bp) in enumerate(zip(singles, res, capi.unpack_pairs_block(block, list(sizes), res))):
            o = batch_ref(oracle, i, k)
            assert (r["n_iterations"], r["n_final_pairs"]) == (a["n_iterations"], a["n_final_pairs"]) == (o["n_iterations"], o["n_final_pairs"])
            assert np.array_equal(r["T"], a["T"]) and np.array_equal(r["cov"], a["cov"])
            np.testing.assert_allclose(r["T"], o["T"], atol=POSE_TOL, rtol=0)
            for key in ("local_idx", "global_idx", "d2"):
                assert np.array_equal(bp[key], a["pairs"][key]), (k, key)
                assert np.array_equal(bp[key], o["pairs"][key]), (k, key)


# ------------------------------------------------------------------------------------------------------------ graph cache
def test_the_switch_toggled_under_a_warm_graph_cache(ctx, length_map, monkeypatch):
    """One context, one map, one 1000-point scan, graphs on.  A chunk's launch sequence is captured when a later alignment brings
    its key again and replayed from then on: of three alignments without the switch the second captures and the third replays.
    Then two with MH_NO_OFF32=1 and two without: the instantiation is a word of the graph key, so the first of each pair misses the
    cache and launches directly, the second captures anew.  All seven results are the same bytes, and in every alignment the
    counters move on the side the switch names only -- a replayed graph counts what it holds -- by exactly max_iterations (with
    poll_every = max_iterations an alignment is ONE chunk of that many iterations, launched directly or as one graph)."""
    _, scan = _length_inputs()
    gs = capi.Scan(ctx, scan[:1000])
    n_it = 4
    p = capi.ICPParams(max_iterations=n_it, threshold=THRESHOLD, kernel_param=KERNEL_PARAM, disable_stall_test=True, poll_every=n_it)
    monkeypatch.setenv("MH_MATCH", "f")
    for var in ("MH_NO_GRAPH", "MH_NO_STREAM"):
        monkeypatch.delenv(var, raising=False)
    runs = []
    for phase, (wide, repeats) in enumerate([(False, 3), (True, 2), (False, 2)]):
        set_instantiation(monkeypatch, wide)
        for rep in range(repeats):
            c0 = capi.flat_stats()
            r = capi.icp_align(length_map, gs, guess(0.2), p, want_trace=False, want_pairs=True)
            assert moved(c0) == only(FLAT_WIDE if wide else FLAT, n_it), (phase, rep, wide)
            assert (r["n_iterations"], r["n_enqueued_iterations"], r["n_host_polls"]) == (n_it, n_it, 1), (phase, rep)
            runs.append(r)
    first = runs[0]
    assert first["n_final_pairs"] > 900
    for r in runs[1:]:
        assert np.asarray(r["T"]).tobytes() == np.asarray(first["T"]).tobytes()
        assert np.asarray(r["cov"]).tobytes() == np.asarray(first["cov"]).tobytes()
        assert r["n_final_pairs"] == first["n_final_pairs"]
        for key in ("local_idx", "global_idx", "d2", "global_xyz"):
            assert r["pairs"][key].tobytes() == first["pairs"][key].tobytes(), key

