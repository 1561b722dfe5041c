"""A numpy restatement of the occupancy voxel map as include/molahip.h words it at mh_occmap_insert ("the reading
implemented"), for the tests of the device implementation.  Written from that text with the SEQUENTIAL integer line walk
("add ad to an error vector; on each axis with 2 err >= M, step and subtract M"), never the closed form, so that the two
implementations do not share a derivation.  No product code, no oracle."""
import math

import numpy as np

COUNTED, ONCE = 0, 1
FAR_CHEBYSHEV, FAR_L1, FAR_L2 = 0, 1, 2
F = np.float32


def five_integers(prob_hit, prob_miss, clamp_min, clamp_max, occupied_threshold):
    """(l_hit, l_miss, l_min, l_max, l_occ): scale-16 log-odds, derived in double from the float32 parameters."""
    lo = lambda p: 16.0 * math.log(float(F(p)) / (1.0 - float(F(p))))
    rnd = lambda v: int(math.floor(v + 0.5))
    return (max(1, rnd(lo(prob_hit))), max(1, rnd(-lo(prob_miss))), rnd(lo(clamp_min)), rnd(lo(clamp_max)),
            int(math.floor(lo(occupied_threshold))) + 1)


def walk_sequential(o, e):
    """The cells strictly between o and e (integer triples): the error-vector walk, one step of k at a time."""
    o = [int(v) for v in o]
    e = [int(v) for v in e]
    ad = [abs(e[a] - o[a]) for a in range(3)]
    s = [(e[a] > o[a]) - (e[a] < o[a]) for a in range(3)]
    M = max(ad)
    c, err, out = list(o), [0, 0, 0], []
    for _ in range(1, M):
        for a in range(3):
            err[a] += ad[a]
            if 2 * err[a] >= M:
                c[a] += s[a]
                err[a] -= M
        out.append(tuple(c))
    return out


def walk_closed_form(o, e):
    """The closed form the device uses (only the CPU test that compares the two calls this)."""
    o = [int(v) for v in o]
    e = [int(v) for v in e]
    ad = [abs(e[a] - o[a]) for a in range(3)]
    s = [(e[a] > o[a]) - (e[a] < o[a]) for a in range(3)]
    M = max(ad)
    return [tuple(o[a] + s[a] * ((2 * k * ad[a] + M) // (2 * M)) for a in range(3)) for k in range(1, M)]


def _walk_many(o, E):
    """walk_sequential for many end cells at once: the same walk, every ray advanced one step per turn.  Returns [m, 3]."""
    E = np.asarray(E, np.int64).reshape(-1, 3)
    o = np.asarray(o, np.int64)
    ad = np.abs(E - o)
    s = np.sign(E - o)
    M = ad.max(axis=1) if len(E) else np.zeros(0, np.int64)
    c = np.repeat(o[None, :], len(E), 0)
    err = np.zeros_like(c)
    out = []
    for k in range(1, int(M.max()) if len(E) else 0):
        act = k < M
        err[act] += ad[act]
        step = act[:, None] & (2 * err >= M[:, None])
        c = c + np.where(step, s, 0)
        err = err - np.where(step, M[:, None], 0)
        out.append(c[act].copy())
    return np.concatenate(out) if out else np.zeros((0, 3), np.int64)


def compose(xyz, T):
    """(float)(R p + t): fp64, in the order ((T0 x + T1 y) + T2 z) + T3, rounded to float."""
    p = np.asarray(xyz, np.float32).reshape(-1, 3).astype(np.float64)
    T = np.asarray(T, np.float64).reshape(-1)[:12].reshape(3, 4)
    with np.errstate(all="ignore"):
        return np.stack([((T[a, 0] * p[:, 0] + T[a, 1] * p[:, 1]) + T[a, 2] * p[:, 2]) + T[a, 3] for a in range(3)], 1).astype(F)


class OccMapRef:
    def __init__(self, resolution=0.05, prob_hit=0.7, prob_miss=0.3, clamp_min=0.05, clamp_max=0.95, occupied_threshold=0.6,
                 ray_trace_free_space=True, decimation=1, max_range=0.0, update_rule=COUNTED, trunc=False,
                 far_voxel_metric=FAR_CHEBYSHEV):
        self.res = F(resolution)
        self.inv_res = F(1.0) / self.res
        self.l_hit, self.l_miss, self.l_min, self.l_max, self.l_occ = five_integers(prob_hit, prob_miss, clamp_min, clamp_max,
                                                                                    occupied_threshold)
        self.ray_trace, self.decimation, self.max_range = bool(ray_trace_free_space), int(decimation), F(max_range)
        self.rule, self.trunc, self.metric = update_rule, trunc, far_voxel_metric
        self.cells = {}  # (ix, iy, iz) -> log-odds
        self.n_left_out = self.n_keys = 0

    def clear(self):
        self.cells = {}
        self.n_left_out = self.n_keys = 0

    def _index(self, p):
        with np.errstate(all="ignore"):
            s = np.asarray(p, F) * self.inv_res
            return (np.trunc(s) if self.trunc else np.floor(s)), s

    def insert(self, xyz, T, remove_voxels_farther_than=0.0):
        T = np.asarray(T, np.float64).reshape(-1)[:12]
        p = compose(np.asarray(xyz, F).reshape(-1, 3)[::self.decimation], T)
        t = np.array([T[3], T[7], T[11]]).astype(F)
        o = self._index(t)[0].astype(np.int64)
        keep = np.isfinite(p).all(axis=1)
        with np.errstate(all="ignore"):
            d = p - t
            d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            if self.max_range > 0:
                keep &= ~(d2 > self.max_range * self.max_range)
            idx, s = self._index(p)
            in_range = (np.abs(s) < F(1.0e6)).all(axis=1)
        self.n_left_out = int((keep & ~in_range).sum())
        keep &= in_range
        E = idx[keep].astype(np.int64)
        hits, misses = {}, {}
        for c in map(tuple, E.tolist()):
            hits[c] = hits.get(c, 0) + 1
        n_keys = len(E)
        if self.ray_trace:
            W = _walk_many(o, E)
            n_keys += len(W)
            if len(W):
                u, cnt = np.unique(W, axis=0, return_counts=True)
                misses = {tuple(c): int(k) for c, k in zip(u.tolist(), cnt.tolist())}
        self.n_keys = n_keys
        for c in set(hits) | set(misses):
            l, h, m = self.cells.get(c, 0), hits.get(c, 0), misses.get(c, 0)
            if self.rule == COUNTED:
                if h:
                    l = min(self.l_max, l + h * self.l_hit)
                if m:
                    l = max(self.l_min, l - m * self.l_miss)
            elif h:
                l = min(self.l_max, l + self.l_hit)
            elif m:
                l = max(self.l_min, l - self.l_miss)
            self.cells[c] = l
        if remove_voxels_farther_than > 0:
            dist = int(np.ceil(F(remove_voxels_farther_than) * self.inv_res))
            far = {FAR_CHEBYSHEV: lambda a: max(a) > dist, FAR_L1: lambda a: sum(a) > dist,
                   FAR_L2: lambda a: a[0] * a[0] + a[1] * a[1] + a[2] * a[2] > dist * dist}[self.metric]
            oo = [int(v) for v in o]
            self.cells = {c: l for c, l in self.cells.items() if not far([abs(c[a] - oo[a]) for a in range(3)])}
        return self

    def download(self):
        """(indices int32 [n, 3], log-odds int32 [n]) in ascending packed-key order (= lexicographic in the indices)."""
        ks = sorted(self.cells)
        return np.array(ks, np.int32).reshape(-1, 3), np.array([self.cells[k] for k in ks], np.int32)

    def centres(self):
        """((float)index + 0.5f) * resolution of the occupied cells, ascending key order: the points of the search map."""
        k, l = self.download()
        k = k[l >= self.l_occ]
        return (k.astype(F) + F(0.5)) * self.res


def nn_k_bruteforce(centres, q, k):
    """The k nearest centres of every query in fp32 as DESIGN.md 3.1 specifies d2: (dx*dx + dy*dy) + dz*dz with d = c - q;
    ties by the lower index.  Returns (idx [n, k'], d2 [n, k'], full sorted d2 [n, m]) with k' = min(k, m)."""
    c = np.asarray(centres, F)
    q = np.asarray(q, F)
    d = c[None, :, :] - q[:, None, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    order = np.argsort(d2, axis=1, kind="stable")
    sd2 = np.take_along_axis(d2, order, 1)
    kk = min(k, c.shape[0])
    return order[:, :kk], sd2[:, :kk], sd2
