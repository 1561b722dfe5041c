"""The join of two sessions restated on the CPU, from the text of mola_lidar_odometry_hip/SessionJoin.h: the reference of
tests/test_session_join_cpu.py and tests/test_gpu_session_join.py.

  * the candidate rule (anchor, forward sweep, backward sweep) in plain Python floats, poses composed in the operation order of the
    host layer's CPose3D so that both sides hand the same doubles on;
  * B's match lists: place_ref.describe of every frame's first stored layer, place_ref.search of each B frame against A's;
  * the verification of a pair on the CPU oracle, with the pieces of loop_ref.Verifier: the submap around A's frame j without the
    causality condition, the grid around the centre the rule names, score, rank, ICP from each kept candidate;
  * the pose graph with fixed nodes: a dense numpy Gauss-Newton with numeric Jacobians (loop_ref's residual and retraction).

No product code."""
import math

import numpy as np

import loop_ref as lr
import place_ref as pr
import score_ref as sr
from oracle import odometry_oracle as oo
from oracle import oracle_c as oc

ANCHOR, FORWARD, BACKWARD = 0, 1, 2
DEFAULTS = dict(top_k=0, max_place_dist=0, min_links=2, min_travel_between_links=10.0, max_anchor_frames=0)
I12 = [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0]


def options(cfg):
    """the session_join: block of a loaded pipeline (a dict) over the defaults, top_k resolved, plus what the rule reads from
    loop_closure: and relocalization:"""
    o = dict(DEFAULTS)
    for k, v in (cfg.get("session_join") or {}).items():
        o[k] = type(DEFAULTS[k])(float(v))
    r = cfg.get("relocalization") or {}
    if o["top_k"] == 0:
        o["top_k"] = max(int(r.get("place_top_k", 4)), 1)
    lo = lr.options(cfg)
    o.update(gate_base=lo["gate_base"], gate_rate=lo["gate_rate"], place_sectors=int(r.get("place_sectors", 64)))
    return o


# ---- poses, in CPose3D's operation order -----------------------------------------------------------------------------------------------
def compose(Ta, Tb):
    """T_a (+) T_b, every sum left to right"""
    a, b = [float(v) for v in Ta], [float(v) for v in Tb]
    c = [0.0] * 12
    for i in range(3):
        for j in range(3):
            c[i * 4 + j] = a[i * 4] * b[j] + a[i * 4 + 1] * b[4 + j] + a[i * 4 + 2] * b[8 + j]
        c[i * 4 + 3] = a[i * 4] * b[3] + a[i * 4 + 1] * b[7] + a[i * 4 + 2] * b[11] + a[i * 4 + 3]
    return c


def minus(Tb, Ta):
    """T_b - T_a = T_a^-1 (+) T_b"""
    return [float(v) for v in lr.inv_compose(Tb, Ta)]


def rz(yaw):
    c, s = math.cos(yaw), math.sin(yaw)
    return [c, -s, 0.0, 0.0, s, c, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0]


def _dist(a, b):
    dx, dy, dz = (float(b[c]) - float(a[c]) for c in (3, 7, 11))
    return math.sqrt(dx * dx + dy * dy + dz * dz)


# ---- the candidate rule ------------------------------------------------------------------------------------------------------------------
def candidates(poses_a, has_a, poses_b, has_b, matches_b, opt, accept=None):
    """matches_b[b]: [(A frame, shift, dist)] ranked by (dist, frame); accept(b, j, shift, dist, phase, centre) -> None or Z (12
    values); None as accept: every pair is accepted with Z = centre.
    -> (tried [(b, j, shift, dist, phase, centre)], links [(b, j, Z)]: the anchor, the forward sweep's, the backward sweep's)"""
    A = np.asarray(poses_a, np.float64).reshape(-1, 12)
    B = np.asarray(poses_b, np.float64).reshape(-1, 12)
    sB = lr.path_lengths(B)
    tried, links = [], []

    def hand_over(b, j, shift, dist, phase, centre):
        tried.append((b, int(j), int(shift), int(dist), phase, list(centre)))
        Z = list(centre) if accept is None else accept(b, int(j), int(shift), int(dist), phase, list(centre))
        return None if Z is None else (b, int(j), [float(v) for v in Z])

    def passes(dist):
        return opt["max_place_dist"] == 0 or dist <= opt["max_place_dist"]

    anchor, visited = None, 0
    for b in range(len(B)):
        if not has_b[b]:
            continue
        if opt["max_anchor_frames"] != 0 and visited >= opt["max_anchor_frames"]:
            break
        visited += 1
        n = 0
        for j, shift, dist in matches_b[b]:
            if n >= opt["top_k"]:
                break
            if not has_a[j] or not passes(dist):
                continue
            n += 1
            anchor = hand_over(b, j, shift, dist, ANCHOR, rz(-float(shift) * 2.0 * math.pi / float(opt["place_sectors"])))
            if anchor is not None:
                break
        if anchor is not None:
            break
    if anchor is None:
        return tried, links
    links.append(anchor)
    for phase, order in ((FORWARD, range(anchor[0] + 1, len(B))), (BACKWARD, range(anchor[0] - 1, -1, -1))):
        carried = anchor
        for b in order:
            if not has_b[b]:
                continue
            cb, cj, cZ = carried
            travel = abs(sB[b] - sB[cb])
            if travel < opt["min_travel_between_links"]:
                continue
            P = compose(compose(A[cj], cZ), minus(B[b], B[cb]))
            n = 0
            for j, shift, dist in matches_b[b]:
                if n >= opt["top_k"]:
                    break
                if not has_a[j] or not passes(dist):
                    continue
                if not _dist(A[j], P) <= opt["gate_base"] + opt["gate_rate"] * travel:
                    continue
                n += 1
                link = hand_over(b, j, shift, dist, phase, minus(P, A[j]))
                if link is not None:
                    carried = link
                    links.append(link)
                    break
    return tried, links


def match_lists(layers_a, has_a, layers_b, has_b, place_params=None):
    """per B frame with points: every A frame with points as (frame, shift, dist), ranked by (dist ascending, frame ascending)"""
    pp = dict(place_params or pr.DEFAULT)
    idx = [k for k in range(len(layers_a)) if has_a[k]]
    out = [[] for _ in layers_b]
    if not idx:
        return out
    descs = np.stack([pr.describe(layers_a[k], **pp) for k in idx])
    for b in range(len(layers_b)):
        if has_b[b]:
            shift, dist = pr.search(descs, pr.describe(layers_b[b], **pp))
            out[b] = [(idx[r], int(shift[r]), int(dist[r])) for r in pr.rank(shift, dist)]
    return out


# ---- the pose graph with fixed nodes: dense Gauss-Newton, numeric Jacobians ------------------------------------------------------------------
def placement(poses, n_fixed, edge):
    """the free chain (nodes n_fixed ..) moved rigidly so that `edge` (a fixed, b free, Z) has a zero residual: G = T_a Z T_b^-1"""
    P = np.asarray(poses, np.float64).reshape(-1, 12)
    a, b, Z = edge
    Gm = lr._to44(P[a]) @ lr._to44(Z) @ np.linalg.inv(lr._to44(P[b]))
    out = P.copy()
    for k in range(n_fixed, len(P)):
        out[k] = (Gm @ lr._to44(P[k]))[:3].reshape(12)
    return out


def optimize_anchored(poses, n_fixed, links, opt, iterations=40):
    """nodes [K, 12], the first n_fixed fixed, the others ONE chain (edges (k - 1, k) from the given poses, odometry weights), links
    [(a fixed, b free, Z)] with the loop weights; the chain starts where links[0] places it.
    -> (poses [K, 12] at the optimum, the cost before every step and at the end)"""
    P = np.asarray(poses, np.float64).reshape(-1, 12)
    K = len(P)
    given = [lr._to44(p) for p in P]
    wo = np.array([1.0 / opt["odometry_sigma_xyz"] ** 2] * 3 + [1.0 / math.radians(opt["odometry_sigma_rot_deg"]) ** 2] * 3)
    wl = np.array([1.0 / opt["loop_sigma_xyz"] ** 2] * 3 + [1.0 / math.radians(opt["loop_sigma_rot_deg"]) ** 2] * 3)
    edges = [(k - 1, k, np.linalg.inv(given[k - 1]) @ given[k], wo) for k in range(n_fixed + 1, K)]
    edges += [(int(a), int(b), lr._to44(Z), wl) for a, b, Z in links]
    T = [lr._to44(p) for p in placement(P, n_fixed, links[0])]
    costs = [lr.cost(T, edges)]
    nv = K - n_fixed
    for _ in range(iterations):
        J = np.zeros((6 * len(edges), 6 * nv))
        r = np.zeros(6 * len(edges))
        sw = np.zeros(6 * len(edges))
        for e, (a, b, Z, w) in enumerate(edges):
            Zi, M = np.linalg.inv(Z), np.linalg.inv(T[a]) @ T[b]
            r[6 * e:6 * e + 6] = lr._residual(Zi @ M)
            sw[6 * e:6 * e + 6] = np.sqrt(w)

            def diff(node, c, h):
                d = np.zeros(6)
                d[c] = h
                Ep = Zi @ (np.linalg.inv(lr._retract(d)) @ M if node == a else M @ lr._retract(d))
                Em = Zi @ (np.linalg.inv(lr._retract(-d)) @ M if node == a else M @ lr._retract(-d))
                return (lr._residual(Ep) - lr._residual(Em)) / (2.0 * h)
            for node in (a, b):
                if node < n_fixed:
                    continue
                for c in range(6):
                    J[6 * e:6 * e + 6, 6 * (node - n_fixed) + c] = (4.0 * diff(node, c, 5e-5) - diff(node, c, 1e-4)) / 3.0
        Jw, rw = J * sw[:, None], r * sw
        delta = np.linalg.solve(Jw.T @ Jw, -Jw.T @ rw)
        for k in range(n_fixed, K):
            T[k] = T[k] @ lr._retract(delta[6 * (k - n_fixed):6 * (k - n_fixed) + 6])
        costs.append(lr.cost(T, edges))
        if np.abs(delta).max() < 1e-11:
            break
    return np.array([t[:3].reshape(12) for t in T]), costs


# ---- verification on the CPU oracle --------------------------------------------------------------------------------------------------------
class Verifier(lr.Verifier):
    """loop_ref.Verifier over A's frames (the submaps), observing B's frames; the submap has no causality condition and the grid's
    centre and spread are the caller's"""

    def __init__(self, maps, frames_a, frames_b, cfg, n_threads=8):
        super().__init__(maps, frames_a, cfg, n_threads)
        self.frames_b = frames_b
        self.has_points_b = [f["layers"] is not None and len(f["layers"]) > 0 and len(f["layers"][0][1]) > 0 for f in frames_b]
        self.poses_b = np.array([f["pose"] for f in frames_b], np.float64).reshape(-1, 12)
        r = cfg.get("relocalization") or {}
        self.place_sigma = (float(r.get("place_sigma_xy", 1.0)), float(r.get("place_sigma_yaw_deg", 5.625)))
        self.jopt = options(cfg)
        self._submaps = {}

    def submap_around(self, j):
        if j not in self._submaps:
            p = self.maps[self.map_index]["params"]
            m = oc.Map(np.float32(p["voxel_size"]), int(p["max_points_per_voxel"]), int(p["index_mode"]), float(np.float32(p["min_distance_between_points"])),
                       float(np.float32(p["ndt_max_eigen_ratio"])), int(p["ndt_min_points"]) if p["ndt_max_eigen_ratio"] > 0 else 4,
                       int(p["far_voxel_metric"]))
            for q in range(len(self.frames)):
                if self.has_points[q] and abs(self.s[q] - self.s[j]) <= self.opt["submap_radius"]:
                    for mi, xyz in self.frames[q]["layers"]:
                        if mi == self.map_index:
                            m.insert_posed(np.asarray(xyz, np.float32), lr.inv_compose(self.poses[q], self.poses[j]), 0.0)
            self._submaps[j] = m
        return self._submaps[j]

    def variables_b(self, b):
        xyz = np.asarray(self.frames_b[b]["layers"][0][1], np.float64)
        r = float(np.sqrt((xyz * xyz).sum(1)[np.isfinite(xyz).all(1)].max())) if len(xyz) else 0.0
        v = {k: 0.0 for k in ("vx", "vy", "vz", "wx", "wy", "wz", "robot_x", "robot_y", "robot_z", "robot_yaw", "robot_pitch", "robot_roll",
                              "ICP_ITERATION", "icp_iterations", "SENSOR_TIME_OFFSET", "twistCorrectionCount")}
        v.update(ADAPTIVE_THRESHOLD_SIGMA=self.opt["sigma"], INSTANTANEOUS_SENSOR_MAX_RANGE=20.0, ESTIMATED_SENSOR_MAX_RANGE=max(r, self.min_range))
        return v

    def verify_pair(self, b, j, shift, dist, phase, centre):
        """-> Z (12 values) when accepted, None otherwise; appends the record to self.pairs"""
        omap = self.submap_around(j)
        parts = [np.asarray(xyz, np.float32).reshape(-1, 3) for m, xyz in self.frames_b[b]["layers"] if m == self.map_index]
        local = np.concatenate(parts, 0) if parts else np.zeros((0, 3), np.float32)
        v = self.variables_b(b)
        e = self.reloc["score_threshold"]
        thr = oo.formula(e, v) if e not in (None, "", "~") else 0.5 * float(np.float32(self.maps[self.map_index]["params"]["voxel_size"]))
        step = self.reloc["step_xy"]
        step = float(step) if step not in (None, "", "~") and float(step) > 0 else thr
        sxy, syaw = self.place_sigma if phase == ANCHOR else (self.opt["sigma_xy"], self.opt["sigma_yaw_deg"])
        cov = sr.grid_cov(sxy, sxy, math.radians(syaw))
        poses, _ = sr.relocalization_grid(lr.to_ypr(centre), cov, step, math.radians(self.reloc["step_yaw_deg"]), self.reloc["sigmas"])
        assert len(poses) <= self.reloc["max_candidates"]
        scores = sr.score_poses(oc, omap, local, poses, thr)
        order = sr.rank(scores)[:self.reloc["refine_top_k"]]
        best = None
        for c in order:
            res = self.refine(omap, local, poses[c], v)
            if best is None or res["quality"] > best["quality"]:
                best = res
        rec = dict(i=b, j=j, phase=phase, shift=shift, dist=dist, candidates=len(poses), ranks=[int(c) for c in order],
                   quality=best["quality"] if best else 0.0, iterations=best["n_iterations"] if best else 0,
                   Z=np.array(best["T"]) if best else np.array(I12))
        rec["accepted"] = bool(best is not None and best["quality"] >= self.opt["min_quality"])
        self.pairs.append(rec)
        return [float(x) for x in rec["Z"]] if rec["accepted"] else None


def join_sessions(a, b, cfg, n_threads=8):
    """a, b: key-frame dicts (maps, frames); cfg: the loaded pipeline.
    -> dict(pairs, links [(b, j, Z)], is_joined, poses_b [KB, 12] in A's frame (None when not joined), placed_b: the anchor-only
    placement T_AB . TB (None without an anchor), costs, options)"""
    oc.build()
    assert a["maps"] == b["maps"]
    v = Verifier(a["maps"], a["frames"], b["frames"], cfg, n_threads)
    layers_a = [f["layers"][0][1] if hp else None for f, hp in zip(a["frames"], v.has_points)]
    layers_b = [f["layers"][0][1] if hp else None for f, hp in zip(b["frames"], v.has_points_b)]
    r = cfg.get("relocalization") or {}
    pp = dict(n_rings=int(r.get("place_rings", 20)), n_sectors=int(r.get("place_sectors", 64)), min_range=float(r.get("place_min_range", 1.0)),
              max_range=float(r.get("place_max_range", 80.0)), z_min=float(r.get("place_z_min", -3.0)), z_max=float(r.get("place_z_max", 27.0)))
    matches = match_lists(layers_a, v.has_points, layers_b, v.has_points_b, pp)
    tried, links = candidates(v.poses, v.has_points, v.poses_b, v.has_points_b, matches, v.jopt, v.verify_pair)
    assert [(p["i"], p["j"], p["shift"], p["dist"], p["phase"]) for p in v.pairs] == [t[:5] for t in tried]
    out = dict(pairs=v.pairs, tried=tried, links=links, matches=matches, is_joined=len(links) >= v.jopt["min_links"], poses_b=None, placed_b=None,
               costs=[0.0], options=v.jopt)
    if links:
        KA = len(v.poses)
        both = np.concatenate([v.poses, v.poses_b], 0)
        edges = [(j, KA + bb, Z) for bb, j, Z in links]
        out["placed_b"] = placement(both, KA, edges[0])[KA:]
        if out["is_joined"]:
            if len(edges) == 1:
                out["poses_b"] = out["placed_b"].copy()
            else:
                poses, out["costs"] = optimize_anchored(both, KA, edges, v.opt)
                out["poses_b"] = poses[KA:]
    return out
