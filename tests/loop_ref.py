"""Loop closure over a key-frame set restated on the CPU: the reference of tests/test_loop_cpu.py and tests/test_gpu_loop.py.

  * the candidate rule in plain Python floats, on match lists ranked like place_ref.rank;
  * the match lists themselves: place_ref.describe of every frame's first stored layer, place_ref.search of each against all;
  * the verification of a pair on the CPU oracle: the submap around the partner (oracle_c.Map.insert_posed of the key-frames'
    layers at T_j^-1 T_q), score_ref.relocalization_grid around the recorded relative pose, score_ref.score_poses, score_ref.rank,
    oracle_c.icp_align from each kept candidate with the schedules of the pipeline's ICP block, the best quality wins, ties go to
    the better rank;
  * the pose graph: a dense numpy Gauss-Newton on r = [t(E); log R(E)], E = Z^-1 T_a^-1 T_b, with numeric Jacobians.

No product code."""
import functools
import math

import numpy as np

import place_ref as pr
import score_ref as sr
from oracle import odometry_oracle as oo
from oracle import oracle_c as oc

DEFAULTS = dict(min_travel=30.0, gate_base=5.0, gate_rate=0.02, max_place_dist=0, top_k=1, min_travel_between_closures=10.0, submap_radius=15.0,
                sigma_xy=1.5, sigma_yaw_deg=2.0, sigma=None, min_quality=0.9, odometry_sigma_xyz=0.02, odometry_sigma_rot_deg=0.05,
                loop_sigma_xyz=0.05, loop_sigma_rot_deg=0.1, max_iterations=50, min_step=1e-9)


def options(cfg):
    """the loop_closure: block of a loaded pipeline (a dict) over the defaults; sigma defaults to adaptive_threshold.initial_sigma"""
    o = dict(DEFAULTS)
    o["sigma"] = float(((cfg.get("params") or {}).get("adaptive_threshold") or {}).get("initial_sigma", 0.5))
    for k, v in (cfg.get("loop_closure") or {}).items():
        o[k] = type(DEFAULTS[k])(float(v)) if DEFAULTS[k] is not None else float(v)
    return o


# ---- candidates ------------------------------------------------------------------------------------------------------------------
def path_lengths(poses):
    P = np.asarray(poses, np.float64).reshape(-1, 12)
    s = [0.0]
    for k in range(1, len(P)):
        dx, dy, dz = (float(P[k][c]) - float(P[k - 1][c]) for c in (3, 7, 11))
        s.append(s[-1] + math.sqrt(dx * dx + dy * dy + dz * dz))
    return s


def candidates(poses, has_points, matches, opt, accept=None):
    """matches[i]: [(frame, shift, dist)] ranked by (dist, frame); accept(i, j, shift, dist) -> bool, None: always.
    -> [(i, j, shift, dist)] of the pairs handed to accept, in order"""
    P = np.asarray(poses, np.float64).reshape(-1, 12)
    s = path_lengths(P)
    tried, closed_at = [], None
    for i in range(len(P)):
        if not has_points[i]:
            continue
        if closed_at is not None and s[i] < closed_at + opt["min_travel_between_closures"]:
            continue
        n = 0
        for j, shift, dist in matches[i]:
            if n >= opt["top_k"]:
                break
            if j >= i or not has_points[j]:
                continue
            travel = s[i] - s[j]
            if not travel >= opt["min_travel"]:
                continue
            dx, dy, dz = (float(P[i][c]) - float(P[j][c]) for c in (3, 7, 11))
            if not math.sqrt(dx * dx + dy * dy + dz * dz) <= opt["gate_base"] + opt["gate_rate"] * travel:
                continue
            if opt["max_place_dist"] != 0 and dist > opt["max_place_dist"]:
                continue
            n += 1
            tried.append((i, int(j), int(shift), int(dist)))
            if accept is None or accept(i, int(j), int(shift), int(dist)):
                closed_at = s[i]
                break
    return tried


def match_lists(layers, has_points, place_params=None):
    """per frame with points: every frame with points as (frame, shift, dist), ranked by (dist ascending, frame ascending)"""
    pp = dict(place_params or pr.DEFAULT)
    idx = [k for k in range(len(layers)) if has_points[k]]
    descs = np.stack([pr.describe(layers[k], **pp) for k in idx]) if idx else None
    out = [[] for _ in layers]
    for q, k in enumerate(idx):
        shift, dist = pr.search(descs, descs[q])
        out[k] = [(idx[r], int(shift[r]), int(dist[r])) for r in pr.rank(shift, dist)]
    return out


# ---- poses -----------------------------------------------------------------------------------------------------------------------
def inv_compose(Tb, Ta):
    """T_a^-1 T_b (12 values each), in the operation order of the host layer's CPose3D so that both sides hand the same doubles to
    the maps: the inverse first, then the composition, every sum left to right"""
    a, b = [float(v) for v in Ta], [float(v) for v in Tb]
    ai = [0.0] * 12
    for i in range(3):
        for j in range(3):
            ai[i * 4 + j] = a[j * 4 + i]
        ai[i * 4 + 3] = -(a[i] * a[3] + a[4 + i] * a[7] + a[8 + i] * a[11])
    c = [0.0] * 12
    for i in range(3):
        for j in range(3):
            c[i * 4 + j] = ai[i * 4] * b[j] + ai[i * 4 + 1] * b[4 + j] + ai[i * 4 + 2] * b[8 + j]
        c[i * 4 + 3] = ai[i * 4] * b[3] + ai[i * 4 + 1] * b[7] + ai[i * 4 + 2] * b[11] + ai[i * 4 + 3]
    return np.array(c)


def to_ypr(T):
    """(x, y, z, yaw, pitch, roll) of 12 values, as TPose3D has them"""
    T = [float(v) for v in T]
    c = math.hypot(T[0], T[4])
    pitch = math.atan2(-T[8], c)
    if c > 1e-12:
        yaw, roll = math.atan2(T[4], T[0]), math.atan2(T[9], T[10])
    else:
        yaw, roll = math.atan2(-T[1], T[5]), 0.0
    return np.array([T[3], T[7], T[11], yaw, pitch, roll])


# ---- verification on the CPU oracle ----------------------------------------------------------------------------------------------------
class Verifier:
    """frames: the "frames" list of a key-frame dict (pose, layers [(map_index, xyz)] or None); maps: its "maps" list; cfg: the
    loaded pipeline (oracle.odometry_oracle.load_pipeline*)"""

    def __init__(self, maps, frames, cfg, n_threads=8, cache=None):
        self.maps, self.frames, self.cfg, self.n_threads = maps, frames, cfg, n_threads
        self.cache = cache   # {(i, j): record}: verifications of these very frames under these very settings, acceptance apart
        self.opt = options(cfg)
        self.icp = cfg.get("icp_settings_without_vel") or cfg["icp_settings_with_vel"]
        ms = [m for m in self.icp["matchers"] if oo._b((m.get("params") or {}).get("enabled", True))]
        assert len(ms) == 1 and ms[0]["class"].endswith("Matcher_Points_DistanceThreshold"), "the reference verifies single point-matcher blocks"
        self.matcher = ms[0]["params"]
        self.solver = self.icp["solvers"][0]["params"]
        g = self.matcher["pointLayerMatches"][0]["global"]
        self.map_index = [m["name"] for m in maps].index(g)
        r = cfg.get("relocalization") or {}
        self.reloc = dict(score_threshold=r.get("score_threshold"), step_xy=r.get("step_xy"), step_yaw_deg=float(r.get("step_yaw_deg", 3.0)),
                          sigmas=float(r.get("sigmas", 3.0)), refine_top_k=int(r.get("refine_top_k", 4)), max_candidates=int(r.get("max_candidates", 65536)))
        self.has_points = [f["layers"] is not None and len(f["layers"]) > 0 and len(f["layers"][0][1]) > 0 for f in frames]
        self.poses = np.array([f["pose"] for f in frames], np.float64).reshape(-1, 12)
        self.s = path_lengths(self.poses)
        self.min_range = float(cfg["params"].get("absolute_minimum_sensor_range", 5.0))
        self.pairs = []

    def _layer(self, k):
        parts = [np.asarray(xyz, np.float32).reshape(-1, 3) for m, xyz in self.frames[k]["layers"] if m == self.map_index]
        return np.concatenate(parts, 0) if parts else np.zeros((0, 3), np.float32)

    def submap(self, i, j):
        p = self.maps[self.map_index]["params"]
        m = oc.Map(np.float32(p["voxel_size"]), int(p["max_points_per_voxel"]), int(p["index_mode"]), float(np.float32(p["min_distance_between_points"])),
                   float(np.float32(p["ndt_max_eigen_ratio"])), int(p["ndt_min_points"]) if p["ndt_max_eigen_ratio"] > 0 else 4,
                   int(p["far_voxel_metric"]))
        for q in range(len(self.frames)):
            if self.has_points[q] and abs(self.s[q] - self.s[j]) <= self.opt["submap_radius"] and self.s[i] - self.s[q] >= self.opt["min_travel"]:
                for mi, xyz in self.frames[q]["layers"]:
                    if mi == self.map_index:
                        m.insert_posed(np.asarray(xyz, np.float32), inv_compose(self.poses[q], self.poses[j]), 0.0)
        return m

    def variables(self, i):
        xyz = np.asarray(self.frames[i]["layers"][0][1], np.float64)
        r = float(np.sqrt((xyz * xyz).sum(1)[np.isfinite(xyz).all(1)].max())) if len(xyz) else 0.0
        v = {k: 0.0 for k in ("vx", "vy", "vz", "wx", "wy", "wz", "robot_x", "robot_y", "robot_z", "robot_yaw", "robot_pitch", "robot_roll",
                              "ICP_ITERATION", "icp_iterations", "SENSOR_TIME_OFFSET", "twistCorrectionCount")}
        v.update(ADAPTIVE_THRESHOLD_SIGMA=self.opt["sigma"], INSTANTANEOUS_SENSOR_MAX_RANGE=20.0, ESTIMATED_SENSOR_MAX_RANGE=max(r, self.min_range))
        return v

    def refine(self, omap, local, T0, v):
        ip = self.icp["params"]
        n = int(ip["maxIterations"])
        thr, kp = np.zeros(n), np.zeros(n)
        for k in range(n):
            vk = {**v, "ICP_ITERATION": float(k)}
            thr[k] = oo.formula(self.matcher["threshold"], vk)
            kp[k] = oo.formula(self.solver["robustKernelParam"], vk)
        q = oc.ICPParams(max_iterations=n, min_abs_step_trans=float(ip["minAbsStep_trans"]), min_abs_step_rot=float(ip["minAbsStep_rot"]),
                         threshold=thr, kernel_param=kp, pt2pl_threshold=None, threshold_angular_deg=0.0,
                         gn=oc.GNParams(max_inner_iterations=int(self.solver["maxIterations"]),
                                        robust_kernel=oo._KERNELS[str(self.solver.get("robustKernel", "GemanMcClure")).split("::")[-1]]),
                         hook_enabled=False)
        return oc.icp_align(omap, local, T0, q, prior=None, n_threads=self.n_threads)

    def verify(self, i, j, shift, dist):
        if self.cache is not None and (i, j) in self.cache:
            rec = dict(self.cache[(i, j)], shift=shift, dist=dist)
            rec["accepted"] = bool(rec["ranks"] and rec["quality"] >= self.opt["min_quality"])
            self.pairs.append(rec)
            return rec["accepted"]
        omap = self.submap(i, j)
        local = self._layer(i)
        v = self.variables(i)
        e = self.reloc["score_threshold"]
        thr = oo.formula(e, v) if e not in (None, "", "~") else 0.5 * float(np.float32(self.maps[self.map_index]["params"]["voxel_size"]))
        step = self.reloc["step_xy"]
        step = float(step) if step not in (None, "", "~") and float(step) > 0 else thr
        cov = sr.grid_cov(self.opt["sigma_xy"], self.opt["sigma_xy"], math.radians(self.opt["sigma_yaw_deg"]))
        mean = to_ypr(inv_compose(self.poses[i], self.poses[j]))
        poses, _ = sr.relocalization_grid(mean, cov, step, math.radians(self.reloc["step_yaw_deg"]), self.reloc["sigmas"])
        assert len(poses) <= self.reloc["max_candidates"]
        scores = sr.score_poses(oc, omap, local, poses, thr)
        order = sr.rank(scores)[:self.reloc["refine_top_k"]]
        best = None
        for c in order:
            res = self.refine(omap, local, poses[c], v)
            if best is None or res["quality"] > best["quality"]:
                best = res
        rec = dict(i=i, j=j, shift=shift, dist=dist, candidates=len(poses), ranks=[int(c) for c in order],
                   quality=best["quality"] if best else 0.0, iterations=best["n_iterations"] if best else 0,
                   Z=np.array(best["T"]) if best else np.eye(4)[:3].reshape(12))
        rec["accepted"] = bool(best is not None and best["quality"] >= self.opt["min_quality"])
        self.pairs.append(rec)
        if self.cache is not None:
            self.cache[(i, j)] = rec
        return rec["accepted"]


def close_loops(maps, frames, cfg, n_threads=8, cache=None):
    """-> dict(pairs: one record per tried pair, poses [K, 12] after the optimisation (the input when no loop was accepted), costs)"""
    v = Verifier(maps, frames, cfg, n_threads, cache)
    layers = [f["layers"][0][1] if hp else None for f, hp in zip(frames, v.has_points)]
    r = cfg.get("relocalization") or {}
    pp = dict(n_rings=int(r.get("place_rings", 20)), n_sectors=int(r.get("place_sectors", 64)), min_range=float(r.get("place_min_range", 1.0)),
              max_range=float(r.get("place_max_range", 80.0)), z_min=float(r.get("place_z_min", -3.0)), z_max=float(r.get("place_z_max", 27.0)))
    matches = match_lists(layers, v.has_points, pp)
    tried = candidates(v.poses, v.has_points, matches, v.opt, v.verify)
    assert [(p["i"], p["j"], p["shift"], p["dist"]) for p in v.pairs] == tried
    loops = [(p["j"], p["i"], p["Z"]) for p in v.pairs if p["accepted"]]
    out = dict(pairs=v.pairs, matches=matches, poses=v.poses.copy(), costs=[0.0], options=v.opt)
    if loops:
        out["poses"], out["costs"] = optimize(v.poses, loops, v.opt)
    return out


# ---- the pose graph: dense Gauss-Newton, numeric Jacobians ---------------------------------------------------------------------------------
def _hat(w):
    return np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], np.float64)


def exp_so3(w):
    w = np.asarray(w, np.float64)
    th = float(np.linalg.norm(w))
    W = _hat(w)
    if th < 1e-5:
        return np.eye(3) + W + 0.5 * (W @ W)
    return np.eye(3) + np.sin(th) / th * W + (1.0 - np.cos(th)) / (th * th) * (W @ W)


def log_so3(R):
    v = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s2 = float(np.linalg.norm(v))
    th = math.atan2(0.5 * s2, 0.5 * (np.trace(R) - 1.0))
    assert th < 3.0, "a residual rotation near pi: not a case of these tests"
    return (0.5 * (1.0 + th * th / 6.0) if th < 1e-7 else th / s2) * v


def _to44(T12):
    return np.vstack([np.asarray(T12, np.float64).reshape(3, 4), [0, 0, 0, 1]])


def _retract(d):
    D = np.eye(4)
    D[:3, :3] = exp_so3(d[3:])
    D[:3, 3] = d[:3]
    return D


def _residual(E):
    return np.concatenate([E[:3, 3], log_so3(E[:3, :3])])


def graph_edges(poses, loops, opt):
    """[(a, b, Z 4x4, weights [6])]: the chain's edges from the poses, then the loops"""
    T = [_to44(p) for p in np.asarray(poses, np.float64).reshape(-1, 12)]
    wo = np.array([1.0 / opt["odometry_sigma_xyz"] ** 2] * 3 + [1.0 / math.radians(opt["odometry_sigma_rot_deg"]) ** 2] * 3)
    wl = np.array([1.0 / opt["loop_sigma_xyz"] ** 2] * 3 + [1.0 / math.radians(opt["loop_sigma_rot_deg"]) ** 2] * 3)
    edges = [(k - 1, k, np.linalg.inv(T[k - 1]) @ T[k], wo) for k in range(1, len(T))]
    return edges + [(int(a), int(b), _to44(Z), wl) for a, b, Z in loops]


def cost(T, edges):
    return float(sum((w * _residual(np.linalg.inv(Z) @ np.linalg.inv(T[a]) @ T[b]) ** 2).sum() for a, b, Z, w in edges))


def optimize(poses, loops, opt, iterations=40):
    """-> (poses [K, 12] at the optimum, the cost before every step and at the end).  Node 0 stays.  The Jacobians of an edge are
    central differences of r(Z^-1 D_a^-1 (T_a^-1 T_b) D_b) over the 12 tangent coordinates, Richardson-extrapolated (steps 1e-4 and
    5e-5): their error is some 1e-11, far below what the 1e-8 comparison of the optima needs."""
    T = [_to44(p) for p in np.asarray(poses, np.float64).reshape(-1, 12)]
    K = len(T)
    edges = graph_edges(poses, loops, opt)
    costs = [cost(T, edges)]
    for _ in range(iterations):
        J = np.zeros((6 * len(edges), 6 * K))
        r = np.zeros(6 * len(edges))
        sw = np.zeros(6 * len(edges))
        for e, (a, b, Z, w) in enumerate(edges):
            Zi, M = np.linalg.inv(Z), np.linalg.inv(T[a]) @ T[b]
            r[6 * e:6 * e + 6] = _residual(Zi @ M)
            sw[6 * e:6 * e + 6] = np.sqrt(w)

            def diff(node, c, h):
                d = np.zeros(6)
                d[c] = h
                Ep = Zi @ (np.linalg.inv(_retract(d)) @ M if node == a else M @ _retract(d))
                Em = Zi @ (np.linalg.inv(_retract(-d)) @ M if node == a else M @ _retract(-d))
                return (_residual(Ep) - _residual(Em)) / (2.0 * h)
            for node in (a, b):
                for c in range(6):
                    J[6 * e:6 * e + 6, 6 * node + c] = (4.0 * diff(node, c, 5e-5) - diff(node, c, 1e-4)) / 3.0
        Jw, rw = (J * sw[:, None])[:, 6:], r * sw
        delta = np.linalg.solve(Jw.T @ Jw, -Jw.T @ rw)
        for k in range(1, K):
            T[k] = T[k] @ _retract(delta[6 * (k - 1):6 * k])
        costs.append(cost(T, edges))
        if np.abs(delta).max() < 1e-11:
            break
    return np.array([t[:3].reshape(12) for t in T]), costs


# ---- the scenario's reference, once per process --------------------------------------------------------------------------------------------
_VERIFIED = {}


@functools.lru_cache(maxsize=4)
def scenario_reference(pipeline_text):
    """loop_cases.scenario() closed by the reference under `pipeline_text` (about 8 s per verified pair on the CPU); shared by the
    tests of one process and never modified.  Texts that differ only in how pairs are selected and accepted share their verified
    pairs: a pair's verification reads the frames, the ICP block, relocalization: and the options in the key below, nothing else."""
    import loop_cases as lc
    oc.build()
    s = lc.scenario()
    kf = lc.keyframe_set(s["est"], s["sweeps"])
    cfg = oo.load_pipeline_text(pipeline_text)
    o = options(cfg)
    key = (pipeline_text.split("\nloop_closure:")[0],) + tuple(o[k] for k in ("min_travel", "submap_radius", "sigma_xy", "sigma_yaw_deg", "sigma"))
    return close_loops(kf["maps"], kf["frames"], cfg, cache=_VERIFIED.setdefault(key, {}))
