"""The reference of pairingsPerPoint > 1 on the multi-layer loop (mh_icp_align_layers_kbest) for the tests, and the inputs of their
cases: oracle/layers_oracle.py's loop with a matcher that knows which (pair, iteration) it is asked for -- oracle_c.match_points_k
with the pair's k, "no pairings" for a pair outside its runFromIteration / runUpToIteration interval, and upstream's serial claim
walk for a unique pair in (pair, local index, rank) order: match_points_k lists a point's pairings in ascending distance, so the
walk takes its output as it comes.  The oracle sums every pair's layer into potential_pairings; the contract (include/molahip.h)
counts scan_i->n * k_i over the pairs active in the iteration whose match produced the final pairings, so that figure and the
quality are corrected afterwards.

Everything here runs on the CPU: tests/test_kbest_cpu.py checks the cases on the reference alone (none set apart by
tools/fuzz_layers.py's rule, the properties each case is there for), tests/test_gpu_icp_layers_kbest.py runs the device on them."""
import numpy as np

from mola_lidar_odometry_amd import capi
from oracle import layers_oracle, oracle_c


def active(gate, k):
    frm, up = gate
    return (frm == 0 or k >= frm) and (up == 0 or k <= up)


_EMPTY = dict(local_idx=np.zeros(0, np.uint32), global_idx=np.zeros(0, np.uint32), global_xyz=np.zeros((0, 3), np.float32),
              d2=np.zeros(0, np.float32))


class KMatcher:
    """matcher= of layers_oracle.icp_align_layers: the oracle calls it once per pair and iteration, pairs in order, so call number
    n is pair n % n_pairs in iteration n // n_pairs.  accepted[(i, k)] / kept[(i, k)]: local_idx before / after the claims."""

    def __init__(self, ks, gates, unique):
        self.ks, self.gates, self.unique = [int(k) for k in ks], [tuple(g) for g in gates], [bool(u) for u in unique]
        self.calls, self.claimed, self.accepted, self.kept = 0, {}, {}, {}

    def __call__(self, m, loc, T, thr, ang):
        n = len(self.ks)
        i, it = self.calls % n, self.calls // n
        self.calls += 1
        if i == 0:
            self.claimed = {}  # claims start empty in every iteration
        if not active(self.gates[i], it):
            r = dict(_EMPTY)
        else:
            r = oracle_c.match_points_k(m, loc, T, thr, self.ks[i], ang)
        li = np.asarray(r["local_idx"]).astype(np.int64)
        assert np.all(np.diff(li) >= 0)  # point-major; a point's pairings in ascending distance
        self.accepted[(i, it)] = li.copy()
        if self.unique[i]:
            taken = self.claimed.setdefault(id(m), set())
            keep = np.zeros(len(li), bool)
            for e, g in enumerate(np.asarray(r["global_idx"]).tolist()):
                if g not in taken:
                    taken.add(g)
                    keep[e] = True
            r = dict(r)
            for key in ("local_idx", "global_idx", "global_xyz", "d2"):
                r[key] = r[key][keep]
        self.kept[(i, it)] = np.asarray(r["local_idx"]).astype(np.int64).copy()
        return r


def reference(pairs, ks, T0, p, gates=None, unique=None, prior=None):
    """layers_oracle.icp_align_layers over `pairs` (its dicts) with k_i = ks[i] pairings per point, potential_pairings and
    quality by the contract; also `accepted` / `kept` of the matcher."""
    n = len(pairs)
    gates = gates if gates is not None else [(0, 0)] * n
    km = KMatcher(ks, gates, unique if unique is not None else [0] * n)
    o = layers_oracle.icp_align_layers(pairs, T0, p, prior=prior, matcher=km)
    mi = int(p.max_iterations)
    if mi > 0:
        k_last = min(int(o["n_iterations"]), mi - 1)
        potential = int(sum(len(np.asarray(e["local"]).reshape(-1, 3)) * k for e, k, g in zip(pairs, ks, gates) if active(g, k_last)))
        o["potential_pairings"] = potential
        o["quality"] = o["n_final_pairs"] / potential if (o["n_final_pairs"] and potential) else 0.0
    o["accepted"], o["kept"] = km.accepted, km.kept
    return o


# ------------------------------------------------------------------------------------------------------------------ the cases
KS = [2, 3, 8]
SIZES = [1, 63, 64, 65, 700, 2000]  # a point; around a wave = one match workgroup; several workgroups, not a multiple; the scan


class Inputs:
    """Host arrays only; maps[key] = (points, voxel size, cap).  `whole`: the small workload's map.  `sparse`: a few hundred of its
    points -- 27-voxel blocks with fewer than k records.  `thin`: every tenth point -- most blocks hold k records, some of them
    far from the point.  `dup`: every fourth point, twice -- equal distances, ordered by scan
    position."""

    def __init__(self, w):
        self.w = w
        self.scan = np.ascontiguousarray(w.scan_xyz, np.float32)
        q = np.ascontiguousarray(w.map_xyz[::4])
        self.maps = {"whole": (w.map_xyz, w.voxel_size, w.cap), "sparse": (np.ascontiguousarray(w.map_xyz[::50]), w.voxel_size, w.cap),
                     "dup": (np.ascontiguousarray(np.concatenate([q, q])), w.voxel_size, w.cap),
                     "thin": (np.ascontiguousarray(w.map_xyz[::10]), w.voxel_size, w.cap)}
        self.T0 = w.T_guess.copy()
        # 0.3 m / 2 degrees off the true pose (the bound case): partners change and leave their blocks
        T = w.T_gt.reshape(3, 4).astype(np.float64).copy()
        a = np.deg2rad(2.0)
        Rz = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
        T[:, :3] = Rz @ T[:, :3]
        T[:, 3] += np.array([0.3, 0.0, 0.0])
        self.T_off = np.ascontiguousarray(T.reshape(-1))

    def omaps(self):
        return {k: oracle_c.Map(vs, cap).insert(pts) for k, (pts, vs, cap) in self.maps.items()}


def schedule(n, first=0.9, last=0.45):
    """a threshold schedule that ends where acceptance cuts between the ranks of a good share of the points (the map's points
    lie ~0.2-0.5 m apart: test_kbest_cpu.py asserts the share)"""
    k = np.arange(n, dtype=np.float64)
    return np.maximum(last, first - (first - last) * k / 10.0)


def _pair(mk, local, thr, k, ang=0.0, weight=1.0, gate=(0, 0), unique=0):
    return dict(map=mk, local=np.ascontiguousarray(local, np.float32), threshold=thr, threshold_angular_deg=ang, weight=weight,
                gate=gate, unique=unique, k=k)


def cases(inp):
    """name -> dict(pairs, max_it, kp, inner, T0, prior, pkw)."""
    w, s = inp.w, inp.scan
    thr, kp = schedule(40), np.full(40, 0.5)
    out = {}
    # 1. against the reference: k x n.  A slice below 700 points cannot hold the pose on its own (one point's pairings span three
    # of six dimensions): the rest of the scan aligns beside it with k = 1, at a weight that leaves the slice its say.
    for k in KS:
        for n in SIZES:
            pairs = [_pair("whole", s[:n], thr, k, weight=float(max(1.0, 200.0 / n)))]
            if n < 700:
                pairs.append(_pair("whole", s[1000:], thr, 1))
            out["ref_k%d_n%d" % (k, n)] = dict(pairs=pairs)
    out["angular"] = dict(pairs=[_pair("whole", s[:700], schedule(40, 1.0, 0.35), 2, ang=0.5)])
    out["mixed"] = dict(pairs=[_pair("whole", s[0::2], thr, 1), _pair("whole", s[1::2], schedule(40, 1.0, 0.4), 2, weight=0.25)])
    info = np.eye(6) * np.array([4e4, 4e4, 4e4, 1e5, 1e5, 1e5])
    Tp = w.T_gt.copy()
    Tp[3] += 0.20
    out["inner3_prior"] = dict(pairs=[_pair("whole", s[:700], thr, 3)], inner=3, prior=(Tp, info))
    # 2. trailing ranks empty / ties
    out["sparse"] = dict(pairs=[_pair("sparse", s, np.full(40, 1.5), 3)])
    out["dup"] = dict(pairs=[_pair("dup", s[:700], thr, 3)])
    # previous partners that leave the 27-voxel block: the thin map, everything in the block accepted (its far corner lies
    # 2 sqrt(3) voxels away), so a rank that a bounded search failed to fill would be a missing pairing
    out["leave"] = dict(pairs=[_pair("thin", s, np.full(40, 4.0), 3)])
    # 4. the bound: partners change and leave blocks
    out["bound"] = dict(pairs=[_pair("whole", s, schedule(12, 1.0, 0.45), 3)], max_it=12, T0=inp.T_off, pkw=dict(disable_stall_test=True),
                        kp=np.full(12, 0.5))
    # 6. unique x k
    out["unique_k2"] = dict(pairs=[_pair("whole", s, thr, 2, unique=1)])
    out["unique_k21"] = dict(pairs=[_pair("whole", s[0::2], thr, 2, unique=1), _pair("whole", s[1::2], thr, 1, weight=0.5, unique=1)])
    # 7. gates x k: the pair with k = 2 enters in iteration 2
    out["gated"] = dict(pairs=[_pair("whole", s[:700], thr, 2, gate=(2, 0)), _pair("whole", s[700:], thr, 1)])
    out["gated_short"] = dict(pairs=[_pair("whole", s[:700], thr[:2], 2, gate=(2, 0)), _pair("whole", s[700:], thr[:2], 1)], max_it=2,
                              kp=np.full(2, 0.5), pkw=dict(disable_stall_test=True))
    for c in out.values():
        c.setdefault("max_it", 40)
        c.setdefault("kp", kp)
        c.setdefault("inner", 2)
        c.setdefault("T0", inp.T0)
        c.setdefault("prior", None)
        c.setdefault("pkw", {})
    return out


def oracle_params(c):
    return oracle_c.ICPParams(max_iterations=c["max_it"], kernel_param=c["kp"],
                              gn=oracle_c.GNParams(max_inner_iterations=c["inner"], robust_kernel=capi.KERNEL_GM_C4), **c["pkw"])


def device_params(c):
    return capi.ICPParams(max_iterations=c["max_it"], kernel_param=c["kp"], threshold=1.0,
                          gn=capi.GNParams(max_inner_iterations=c["inner"], robust_kernel=capi.KERNEL_GM_C4), **c["pkw"])


def case_reference(c, omaps):
    pairs = [dict(map=omaps[e["map"]], local=e["local"], threshold=e["threshold"], threshold_angular_deg=e["threshold_angular_deg"],
                  weight=e["weight"]) for e in c["pairs"]]
    return reference(pairs, [e["k"] for e in c["pairs"]], c["T0"], oracle_params(c), [e["gate"] for e in c["pairs"]],
                     [e["unique"] for e in c["pairs"]], prior=c["prior"])


def bound_not_attained(c, o, omaps, i=0):
    """Per ICP iteration j >= 1 of pair i, from the reference's poses alone: (points whose k partners of iteration j - 1 do not
    bound the k nearest of iteration j -- one of them has left the block --, those among them whose k-th nearest is accepted).
    A search that trusted its bound there would lose that pairing."""
    e = c["pairs"][i]
    k, loc, m = e["k"], e["local"], omaps[e["map"]]
    n = len(loc)
    poses = [np.asarray(c["T0"], np.float64)] + [t["T"] for t in o["trace"]]
    thr = np.broadcast_to(np.asarray(e["threshold"], np.float64), (c["max_it"],))
    out = []
    for j in range(1, len(o["trace"]) + 1):
        if j >= c["max_it"]:
            break
        a = oracle_c.match_points_k(m, loc, poses[j - 1], 1e3, k)
        b = oracle_c.match_points_k(m, loc, poses[j], 1e3, k)
        ca, cb = np.bincount(a["local_idx"], minlength=n), np.bincount(b["local_idx"], minlength=n)
        T = poses[j].reshape(3, 4)
        P = loc.astype(np.float64) @ T[:, :3].T + T[:, 3]
        b0, kth = np.zeros(n), np.zeros(n)
        np.maximum.at(b0, a["local_idx"], np.sum((P[a["local_idx"]] - a["global_xyz"]) ** 2, 1))
        np.maximum.at(kth, b["local_idx"], b["d2"].astype(np.float64))
        lost = (ca == k) & (cb == k) & (kth > b0 * (1.0 + 1e-5))  # (1e-5: far above the fp32 rounding of either side)
        out.append((int(np.sum(lost)), int(np.sum(lost & (kth < thr[j] ** 2 * (1.0 - 1e-5))))))
    return out


def set_apart(o):
    """tools/fuzz_layers.py's rule, read from the oracle alone: a decision within 1e-9 of its threshold, or normal equations
    conditioned above 1e10."""
    near = layers_oracle.nearest_decision(o["margins"])
    return (near is not None and near[1] <= 1e-9) or not o["max_cond"] < 1e10
