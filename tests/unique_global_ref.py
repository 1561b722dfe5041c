"""The reference of allowMatchAlreadyMatchedGlobalPoints == false (U13) for the tests: oracle/layers_oracle.py's loop with a
stateful matcher that restates upstream's serial walk -- a set of claimed map points per map, emptied for every ICP iteration,
candidates taken pair by pair in ascending local index, a candidate of a unique pair dropped when its map point is claimed and
claiming it otherwise.  Pairs that are not unique neither test nor set claims."""
import numpy as np

from oracle import layers_oracle, oracle_c


class ClaimMatcher:
    """matcher= of layers_oracle.icp_align_layers for `unique` (one flag per pair, in pair order).  The oracle calls it once per
    pair and iteration, pairs in order: call number modulo the pair count is the pair, and a wrap (or a new pose) a new iteration.
    Counts what it saw: candidates / dropped (over the unique pairs, all iterations)."""

    def __init__(self, unique, inner=oracle_c.match_points):
        self.unique = [bool(u) for u in unique]
        self.inner = inner
        self.calls = 0
        self.pose = None
        self.claimed = {}
        self.candidates = 0
        self.dropped = 0

    def __call__(self, m, loc, T, thr, ang):
        i = self.calls % len(self.unique)
        self.calls += 1
        T = np.asarray(T, np.float64).reshape(-1)[:12].copy()
        if i == 0 or self.pose is None or not np.array_equal(T, self.pose):
            assert i == 0, "the pose changed inside an iteration"
            self.claimed = {}
            self.pose = T
        r = self.inner(m, loc, T, thr, ang)
        if not self.unique[i]:
            return r
        taken = self.claimed.setdefault(id(m), set())
        keep = np.zeros(len(r["local_idx"]), bool)
        assert np.all(np.diff(r["local_idx"].astype(np.int64)) > 0)  # ascending local index: upstream's order
        for k, g in enumerate(r["global_idx"].tolist()):
            if g not in taken:
                taken.add(g)
                keep[k] = True
        self.candidates += len(keep)
        self.dropped += int(np.sum(~keep))
        out = dict(r)
        for key in ("local_idx", "global_idx", "global_xyz", "d2"):
            out[key] = r[key][keep]
        return out


def reference(pairs, unique, T0, p, prior=None):
    """layers_oracle.icp_align_layers over `pairs` (its dicts) with pair i unique where unique[i]; the result carries the
    matcher's counts as `candidates` and `dropped`."""
    m = ClaimMatcher(unique)
    o = layers_oracle.icp_align_layers(pairs, T0, p, prior=prior, matcher=m)
    o["candidates"], o["dropped"] = m.candidates, m.dropped
    return o
