"""The reference of Matcher::runFromIteration / runUpToIteration on the multi-layer loop (mh_icp_align_layers_gated) for the tests,
and the inputs of their cases: oracle/layers_oracle.py's loop with a matcher that knows which (pair, iteration) it is asked for
and answers "no pairings" for a pair outside its interval -- the rule of Matcher::match.  It sits INSIDE unique_global_ref's
ClaimMatcher, so a gated-off pair makes and loses no claims.  The oracle sums every pair's layer into potential_pairings; the
contract (include/molahip.h) counts the pairs that are active in the iteration whose match produced the final pairings, so that
figure and the quality are corrected afterwards.

Everything here runs on the CPU: tests/test_gates_cpu.py checks these cases on the reference alone (no decision within rounding
of its threshold, the gates change the result), tests/test_gpu_icp_layers_gates.py runs the device on the same inputs."""
import numpy as np

from mola_lidar_odometry_amd import capi
from oracle import layers_oracle, oracle_c
from unique_global_ref import ClaimMatcher


def active(gate, k):
    """Matcher::match's gate: gate = (run_from_iteration, run_up_to_iteration), 0 = no limit."""
    frm, up = gate
    return (frm == 0 or k >= frm) and (up == 0 or k <= up)


class GateMatcher:
    """inner= of ClaimMatcher (or matcher= of layers_oracle.icp_align_layers).  The oracle calls its matcher once per pair and
    iteration, pairs in order: call number n is pair n % n_pairs in iteration n // n_pairs.  `candidates[(i, k)]`: what it answered."""

    def __init__(self, gates, inner=oracle_c.match_points):
        self.gates = [tuple(int(v) for v in g) for g in gates]
        self.inner = inner
        self.calls = 0
        self.candidates = {}

    def __call__(self, m, loc, T, thr, ang):
        i, k = self.calls % len(self.gates), self.calls // len(self.gates)
        self.calls += 1
        if active(self.gates[i], k):
            r = self.inner(m, loc, T, thr, ang)
        else:
            r = dict(local_idx=np.zeros(0, np.uint32), global_idx=np.zeros(0, np.uint32), global_xyz=np.zeros((0, 3), np.float32),
                     d2=np.zeros(0, np.float32))
        self.candidates[(i, k)] = (np.asarray(r["local_idx"]).copy(), np.asarray(r["global_idx"]).copy())
        return r


class _Recorder:
    """the outermost matcher: what each (pair, iteration) kept after the claims"""

    def __init__(self, n_pairs, inner):
        self.n, self.inner, self.calls, self.kept = n_pairs, inner, 0, {}

    def __call__(self, m, loc, T, thr, ang):
        i, k = self.calls % self.n, self.calls // self.n
        self.calls += 1
        r = self.inner(m, loc, T, thr, ang)
        self.kept[(i, k)] = (np.asarray(r["local_idx"]).copy(), np.asarray(r["global_idx"]).copy())
        return r


def reference(pairs, gates, T0, p, unique=None, prior=None):
    """layers_oracle.icp_align_layers over `pairs` (its dicts) with pair i gated by gates[i] and unique where unique[i], with
    potential_pairings and quality by the contract.  Also `candidates` / `kept`: {(pair, iteration): (local_idx, global_idx)}
    before / after the claims."""
    n = len(pairs)
    gm = GateMatcher(gates)
    rec = _Recorder(n, ClaimMatcher(unique if unique is not None else [0] * n, inner=gm))
    o = layers_oracle.icp_align_layers(pairs, T0, p, prior=prior, matcher=rec)
    mi = int(p.max_iterations)
    if mi > 0:
        k_last = min(int(o["n_iterations"]), mi - 1)  # the iteration whose match produced the final pairings
        potential = int(sum(len(np.asarray(e["local"]).reshape(-1, 3)) for e, g in zip(pairs, gm.gates) if active(g, k_last)))
        o["potential_pairings"] = potential
        o["quality"] = o["n_final_pairs"] / potential if (o["n_final_pairs"] and potential) else 0.0
    o["candidates"], o["kept"] = gm.candidates, rec.kept
    return o


# ---------------------------------------------------------------------------------------------------------------- the cases
# scan-layer sizes at which a kernel's ranges can go wrong: a point; around a wave = one match workgroup (64); around a claim /
# covariance workgroup (256); around an accumulation workgroup (1024); several of each
SIZES = [1, 63, 64, 65, 255, 257, 1023, 1025, 4100]


def base(sigma, n):
    k = np.arange(n, dtype=np.float64)
    return np.maximum(sigma, 2.0 * sigma - (2.0 * sigma - 0.5 * sigma) * k / 30.0)


class Inputs:
    """The small workload split as tests/test_host_layer.py's near-far test splits it: near / far scan layers (overlapping), a
    0.5 m near map, a 1.0 m far map.  `far_pool`: the far layer continued with map points taken into the vehicle frame (noisy),
    so that a layer of ~4100 points can be cut from it.  Host arrays only; maps[key] = (points, voxel size, cap)."""

    def __init__(self, w):
        self.w = w
        scan = w.scan_xyz
        rng = np.linalg.norm(scan, axis=1)
        self.near_l = np.ascontiguousarray(scan[rng < 9.0])
        far_l = scan[rng >= 6.0]
        T = w.T_gt.reshape(3, 4)
        mr = np.linalg.norm(w.map_xyz - T[:, 3], axis=1)
        self.maps = {"near": (np.ascontiguousarray(w.map_xyz[mr < 12.0]), 0.5, 20),
                     "far": (np.ascontiguousarray(w.map_xyz[::2]), 1.0, 20),
                     "whole": (w.map_xyz, w.voxel_size, w.cap)}
        gen = np.random.default_rng(20240607)
        extra = w.map_xyz[1::7][:3000].astype(np.float64)
        extra = (extra - T[:, 3]) @ T[:, :3] + gen.normal(0.0, 0.03, extra.shape)  # R^T (q - t)
        self.far_pool = np.ascontiguousarray(np.concatenate([far_l, extra.astype(np.float32)]), np.float32)
        assert len(self.far_pool) >= max(SIZES)
        self.even, self.odd = np.ascontiguousarray(scan[0::2]), np.ascontiguousarray(scan[1::2])
        self.T0 = w.T_guess.copy()
        self.T1 = w.T_guess.copy()  # another guess (the stale-buffer runs)
        self.T1[3] -= 0.35
        self.T1[7] += 0.25

    def omaps(self):
        return {k: oracle_c.Map(vs, cap).insert(pts) for k, (pts, vs, cap) in self.maps.items()}


def _pair(mk, local, thr, ang=0.0, weight=1.0, gate=(0, 0), unique=0):
    return dict(map=mk, local=np.ascontiguousarray(local, np.float32), threshold=thr, threshold_angular_deg=ang, weight=weight,
                gate=gate, unique=unique)


def near_far_weight(n):
    """The gated pair's weight in the near-far cases: a small layer's rows are scaled to carry what ~1000 points would, else a
    one-point pair could not move the pose by the 1e-4 that test_gates_cpu.py asks of every case."""
    return float(max(1.0, 1000.0 / n))


def cases(inp):
    """name -> dict(pairs, max_it, kp, pkw (ICPParams keywords of oracle_c and capi alike), hook, prior, without): the inputs of
    cases 1-7 of tests/test_gpu_icp_layers_gates.py, and its hook and prior cases.  `without`: the pairs of the comparison that
    shows the gates matter -- None: the same pairs ungated; a list of indices: the alignment of those pairs alone, ungated."""
    w = inp.w
    b8, b40 = base(w.sigma, 8), base(w.sigma, 40)
    out = {}
    # 1. the near-far shape: pair 0 from = 4; pairs 1 and 2 ungated on one scan, pair 2 on pair 0's map.  Eight iterations without
    # the stall test: the loop ends while the late pair still pulls.
    for n in SIZES:
        out["near_far_%d" % n] = dict(
            pairs=[_pair("far", inp.far_pool[:n], 2.0 * b8, weight=near_far_weight(n), gate=(4, 0)),
                   _pair("near", inp.near_l, np.full(8, 2.0 * w.sigma)),
                   _pair("far", inp.near_l, np.full(8, 2.0 * w.sigma))],
            max_it=8, kp=0.5 * b8, pkw=dict(disable_stall_test=True))
    # 2. up_to below the final iteration: pair 0 leaves after iteration 3, the loop runs on to its stall
    out["up_to"] = dict(pairs=[_pair("near", inp.near_l, 2.0 * b40, gate=(0, 3)), _pair("far", inp.far_pool[:1360], 1.5 * b40 + 0.2, 0.3)],
                        max_it=40, kp=0.5 * b40)
    # 3. from above every executed iteration: pair 1 never runs
    out["never"] = dict(pairs=[_pair("near", inp.near_l, 2.0 * b40), _pair("far", inp.far_pool[:1360], 1.5 * b40 + 0.2, 0.3, gate=(1000, 0)),
                               _pair("far", inp.near_l, np.full(40, 1.1))], max_it=40, kp=0.5 * b40, without=[0, 2])
    # 4. from == up_to: pair 0 is active in iteration 2 alone
    out["single_iteration"] = dict(pairs=[_pair("near", inp.near_l, 2.0 * b40, gate=(2, 2)),
                                          _pair("far", inp.far_pool[:1360], 1.5 * b40 + 0.2, 0.3)], max_it=40, kp=0.5 * b40)
    # 6. NoPairings: everybody gated off in iteration 0; the active set empty in iteration 3
    out["nobody_at_0"] = dict(pairs=[_pair("near", inp.near_l, 2.0 * b40, gate=(1, 0)),
                                     _pair("far", inp.far_pool[:1360], 1.5 * b40 + 0.2, 0.3, gate=(2, 0))], max_it=40, kp=0.5 * b40)
    out["nobody_at_3"] = dict(pairs=[_pair("near", inp.near_l, 2.0 * b40, gate=(0, 2)),
                                     _pair("far", inp.far_pool[:1360], 1.5 * b40 + 0.2, 0.3, gate=(5, 0))], max_it=40, kp=0.5 * b40)
    # 7. gates with unique_global: two unique pairs on one map, the first from = 3 -- until then the second pair wins claims
    # that it loses afterwards.  Ten iterations without the stall test.
    b10 = base(w.sigma, 10)
    out["unique"] = dict(pairs=[_pair("whole", inp.even, 2.0 * b10, gate=(3, 0), unique=1),
                                _pair("whole", inp.odd, 1.5 * b10 + 0.2, weight=0.5, unique=1)],
                         max_it=10, kp=0.5 * b10, pkw=dict(disable_stall_test=True))
    # the device hook firing after the gated pair has entered; a prior
    out["hook"] = dict(pairs=[_pair("far", inp.far_pool[:1360], 2.0 * b40, gate=(2, 0)), _pair("near", inp.near_l, np.full(40, 2.0 * w.sigma))],
                       max_it=40, kp=0.5 * b40, hook=(inp.T0, 0.2, np.deg2rad(0.5)))
    info = np.eye(6) * np.array([4e4, 4e4, 4e4, 1e5, 1e5, 1e5])
    Tp = w.T_gt.copy()
    Tp[3] += 0.20
    out["prior"] = dict(pairs=[_pair("far", inp.far_pool[:1360], 2.0 * b40, gate=(4, 0)), _pair("near", inp.near_l, np.full(40, 2.0 * w.sigma))],
                        max_it=40, kp=0.5 * b40, prior=(Tp, info))
    for c in out.values():
        c.setdefault("pkw", {})
        c.setdefault("hook", None)
        c.setdefault("prior", None)
        c.setdefault("without", None)
    return out


CASES_1_TO_7 = ["near_far_%d" % n for n in SIZES] + ["up_to", "never", "single_iteration", "nobody_at_0", "nobody_at_3", "unique"]


def oracle_params(c):
    p = oracle_c.ICPParams(max_iterations=c["max_it"], kernel_param=c["kp"],
                           gn=oracle_c.GNParams(max_inner_iterations=2, robust_kernel=capi.KERNEL_GM_C4), **c["pkw"])
    if c["hook"] is not None:
        p.hook_enabled, (p.hook_checkpoint, p.hook_min_trans, p.hook_min_rot) = True, c["hook"]
    return p


def _opairs(c, omaps, idx=None):
    sel = c["pairs"] if idx is None else [c["pairs"][i] for i in idx]
    return [dict(map=omaps[e["map"]], local=e["local"], threshold=e["threshold"], threshold_angular_deg=e["threshold_angular_deg"],
                 weight=e["weight"]) for e in sel]


def case_reference(c, omaps, T0, gated=True):
    """The reference of case `c` from guess T0; gated=False: of the comparison alignment (c['without'])."""
    if gated:
        return reference(_opairs(c, omaps), [e["gate"] for e in c["pairs"]], T0, oracle_params(c), [e["unique"] for e in c["pairs"]],
                         prior=c["prior"])
    idx = c["without"] if c["without"] is not None else list(range(len(c["pairs"])))
    return reference(_opairs(c, omaps, idx), [(0, 0)] * len(idx), T0, oracle_params(c), [c["pairs"][i]["unique"] for i in idx],
                     prior=c["prior"])
