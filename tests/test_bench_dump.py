"""bench.py --dump-outputs: the arrays of the last timed step land as float32 / float64 .npy files, inside the 64 MB budget,
with the same pairing sample on every run (CPU: synthetic result dicts in the shape the timed path returns), and the
batches of the last step are found again after the run."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402

N_POINTS = 120000


def _step(seed, n_batches=4, n_jobs=32, drop=0):
    """Result dicts of one step and the pairings of its last batch: ascending local indices, every point but a seeded
    few paired (`drop` more points left unpaired in job 0, as a build with one pair count differing would)."""
    rng = np.random.default_rng(seed)
    results = [[dict(T=rng.normal(size=12), cov=rng.normal(size=(6, 6)), quality=float(rng.random()), n_iterations=20,
                     termination_reason=3, n_final_pairs=0, n_final_pairs_pt2pl=0, potential_pairings=N_POINTS)
                for _ in range(n_jobs)] for _ in range(n_batches)]
    pairs = []
    for j in range(n_jobs):
        g = np.random.default_rng(100 + j)
        keep = np.sort(g.choice(N_POINTS, N_POINTS - 5000, replace=False)).astype(np.uint32)
        gi = g.integers(0, 1 << 20, N_POINTS).astype(np.uint32)
        xyz = g.normal(size=(N_POINTS, 3)).astype(np.float32)
        d2 = g.random(N_POINTS).astype(np.float32)
        if j == 0 and drop:
            keep = keep[drop:]
        pairs.append(dict(local_idx=keep, global_idx=gi[keep], global_xyz=xyz[keep], d2=d2[keep]))
        results[-1][j]["n_final_pairs"] = len(keep)
    return results, pairs


def _dump(path, results, pairs):
    poses = np.stack([r["T"] for r in results[-1]])[None]
    return bench.dump_outputs(str(path), results, pairs, [N_POINTS] * len(pairs), poses)


def test_dump_outputs_types_size_and_repeatability(tmp_path):
    results, pairs = _step(0)
    a, b = tmp_path / "a", tmp_path / "b"
    names = _dump(a, results, pairs)
    assert names == _dump(b, results, pairs)
    assert {"pose", "covariance", "quality", "n_iterations", "n_final_pairs", "pairs_local_idx", "pairs_d2", "pairs_paired",
            "pairs_pose_row"} <= set(names)
    total = 0
    for n in names:
        x, y = np.load(a / (n + ".npy")), np.load(b / (n + ".npy"))
        assert x.dtype in (np.float32, np.float64), n
        np.testing.assert_array_equal(x, y)
        total += os.path.getsize(a / (n + ".npy"))
    assert total <= 64 << 20
    pose = np.load(a / "pose.npy")
    assert pose.shape == (4 * 32, 12)
    np.testing.assert_array_equal(pose[-32:], np.stack([r["T"] for r in results[-1]]))
    # every sampled point names its scan's row in pose.npy and carries its own pairing, or NaN where it has none
    row = np.load(a / "pairs_pose_row.npy").astype(np.int64)
    li = np.load(a / "pairs_local_idx.npy").astype(np.int64)
    paired = np.load(a / "pairs_paired.npy") == 1
    d2 = np.load(a / "pairs_d2.npy")
    xyz = np.load(a / "pairs_global_xyz.npy")
    assert len(li) == 32 * bench.DUMP_PAIRS_PER_SCAN and set(np.unique(row)) == set(range(3 * 32, 4 * 32))
    assert 0 < (~paired).sum() < len(paired) // 10
    for j in (0, 31):
        sel = row == 3 * 32 + j
        p = pairs[j]
        at = np.searchsorted(p["local_idx"], li[sel])
        ok = paired[sel]
        np.testing.assert_array_equal(ok, np.isin(li[sel], p["local_idx"]))
        np.testing.assert_array_equal(d2[sel][ok], p["d2"][at[ok]])
        np.testing.assert_array_equal(xyz[sel][ok], p["global_xyz"][at[ok]])
        assert np.isnan(d2[sel][~ok]).all() and np.isnan(xyz[sel][~ok]).all()


def test_pairing_sample_lines_up_when_pair_counts_differ(tmp_path):
    """Two builds whose pair counts differ by a few points still dump the same sampled scan points, row for row."""
    r1, p1 = _step(0)
    r2, p2 = _step(0, drop=3)
    _dump(tmp_path / "a", r1, p1)
    _dump(tmp_path / "b", r2, p2)
    for n in ("pairs_local_idx", "pairs_pose_row"):
        np.testing.assert_array_equal(np.load(tmp_path / "a" / (n + ".npy")), np.load(tmp_path / "b" / (n + ".npy")))
    pa, pb = np.load(tmp_path / "a" / "pairs_paired.npy"), np.load(tmp_path / "b" / "pairs_paired.npy")
    assert 0 <= (pa != pb).sum() <= 3 and (pb <= pa).all()


def test_dump_outputs_without_pairings(tmp_path):
    results, _ = _step(1, n_batches=1, n_jobs=2)
    names = bench.dump_outputs(str(tmp_path), results, None, None, np.zeros((1, 2, 12)))
    assert not any(n.startswith("pairs_") for n in names)
    assert np.load(tmp_path / "n_iterations.npy").tolist() == [20.0, 20.0]


@pytest.mark.parametrize("K,up", [(4, True), (3, True), (1, True), (1, False)])
def test_batch_slots_of_a_step_are_distinct(K, up):
    """The K batches of any step use K different (buffer set, pairs block, scan set) slots -- what lets bench.py read the
    last step's results back from its marshalled calls after the run -- and consecutive batches alternate pairs blocks."""
    for steps_before in range(4):
        first = steps_before * K
        slots = [bench.batch_slot(b, K, up) for b in range(first, first + K)]
        assert sorted(s[2] for s in slots) == list(range(K))
        assert len(set(slots)) == K
        for b in range(first, first + K):
            buf, cur, _ = bench.batch_slot(b, K, up)
            assert cur == b & 1 and buf == (cur if up else 0)
