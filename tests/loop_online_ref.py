"""Online loop closure (mola_hip::OnlineLoopCloser, LidarOdometry's online_loop_closure: block): the data and the numpy restatements
of tests/test_loop_online_cpu.py and tests/test_gpu_loop_online.py.

  * the pose rules of the driver in 4x4 numpy: the raw chain, the correction delta and its rebase, the corrected trajectory, the
    key-frames a closure rebuilds a local map from;
  * the fold of the per-frame candidate step;
  * the drive of the driver tests: the street canyon of mola_lidar_odometry_amd.synth driven 31 m forward and, in reverse gear, back
    again (the heading stays, so a revisit's descriptor needs no column shift), 120 sweeps of 32 x 600, and its pipeline text;
  * the key-frames the CPU oracle's driver records on that drive (the store's rule is tests/simplemap_ref.py), on which
    tests/loop_ref.py is the reference: the condition of the driver tests.

Data and reference code only (loop_ref, simplemap_ref, loop_cases); no product code."""
import functools
import os

import numpy as np

import loop_cases as lc
import loop_ref as lr
import simplemap_ref
from mola_lidar_odometry_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIPE = os.path.join(ROOT, "pipelines", "lidar3d-default-hip.yaml")

# ---- the drive ---------------------------------------------------------------------------------------------------------------------
N_SCANS, DT, PEAK_SPEED = 120, 0.1, 8.0   # v_k = 8 sin(2 pi k / 120) m/s: 30.6 m forward in 60 scans, then back
KF_SPACING = 2.5                          # [m] between stored key-frames, measured from the last one (a revisit is stored again)
# a partner at least 25 m of path back; after a closure the next one 8 m on; the rest are the defaults (gate 5 m + 2 %, quality 0.9)
LOOP_OPTIONS = "\nloop_closure:\n  min_travel: 25\n  min_travel_between_closures: 8\n"
ENV = ("MOLA_LOAD_MM", "MOLA_MAPPING_ENABLED", "MOLA_INITIAL_LOCALIZATION_ENABLED", "MOLA_GENERATE_SIMPLEMAP", "MOLA_LOAD_SM", "MOLA_SIMPLEMAP_OUTPUT",
       "MOLA_SIMPLEMAP_MIN_XYZ", "MOLA_SIMPLEMAP_MIN_ROT", "MOLA_SIMPLEMAP_GENERATE_LAZY_LOAD", "MOLA_SIMPLEMAP_ALSO_NON_KEYFRAMES",
       "MOLA_LOCAL_MAP_MAX_SIZE", "MOLA_LOCALMAP_MAX_POINTS_PER_VOXEL", "MOLA_MINIMUM_ICP_QUALITY", "MOLA_OPTIMIZE_TWIST", "MOLA_INITIAL_VX")


def pipeline_text(block=""):
    """the default pipeline recording key-frames KF_SPACING apart from the LAST one, the loop options of the drive, then `block`"""
    text = open(PIPE).read()
    assert text.count("  simplemap:\n    generate: ${MOLA_GENERATE_SIMPLEMAP|false}") == 1
    text = text.replace("  simplemap:\n    generate: ${MOLA_GENERATE_SIMPLEMAP|false}", "  simplemap:\n    measure_from_last_kf_only: true\n    generate: true")
    text = text.replace("${MOLA_SIMPLEMAP_MIN_XYZ|(1.0e-2 + sqrt(wx^2+wy^2+wz^2)*1.0)*ESTIMATED_SENSOR_MAX_RANGE}", "%g" % KF_SPACING)
    text = text.replace("${MOLA_SIMPLEMAP_OUTPUT|'final_map.simplemap'}", "''")
    assert "min_translation_between_keyframes: %g " % KF_SPACING in text
    return text + LOOP_OPTIONS + block


def online_block(correct_driver=True, every=1):
    return "\nonline_loop_closure:\n  enabled: true\n  correct_driver: %s\n  check_every_n_keyframes: %d\n" % ("true" if correct_driver else "false", every)


@functools.lru_cache(maxsize=1)
def drive():
    """dict(scans [(xyz, t)], stamps, poses [n, 12] ground truth): synth.make_drive's scene and sweep model under the out-and-back
    twist.  (Some 24 s of ray casting, once per process.  A street of synth_city, whose ray caster is compiled, does not serve: at
    32 x 600 its facades leave the motion along the street open, and the CPU oracle's driver stays where it started.)"""
    scene = synth.make_scene(4242, 120.0, 160)
    T = synth.pose_from_ypr([-60.0, 0.5, synth.SENSOR_H, 0.0, 0.0, 0.0]).reshape(3, 4)
    poses, scans, stamps = [], [], []
    for k in range(N_SCANS):
        tw = np.array([PEAK_SPEED * np.sin(2.0 * np.pi * k / N_SCANS), 0.0, 0.0, 0.0, 0.0, 0.02 * np.sin(0.3 * k)])
        poses.append(T.reshape(12).copy())
        scans.append(synth.make_sweep(scene, T.reshape(12), tw, DT, 32, 600, 4242 + 10 * k))
        stamps.append(1000.0 + k * DT)
        Rn = synth._so3_exp((tw[3:] * DT)[None])[0]
        T = np.concatenate([T[:, :3] @ Rn, (T[:, :3] @ (tw[:3] * DT) + T[:, 3])[:, None]], axis=1)
    return dict(scans=scans, stamps=stamps, poses=np.array(poses))


# ---- poses -------------------------------------------------------------------------------------------------------------------------
def compose(a, b):
    """a (+) b, 12 values each"""
    return lc.to12(lc.to44(a) @ lc.to44(b))


def inverse(a):
    return lc.to12(np.linalg.inv(lc.to44(a)))


def raw_pose(raw_prev, P, S_prev):
    """raw_k = raw_{k-1} (+) (P_k (-) S_{k-1})"""
    return compose(raw_prev, compose(inverse(S_prev), P))


def correction(C, P):
    """delta = C (+) P^-1"""
    return compose(C, inverse(P))


def anchor(P, S):
    """rel = P (-) S"""
    return compose(inverse(S), P)


def corrected_trajectory(trajectory, anchors, rels, C):
    """trajectory: [(t, pose)]; anchors[n]: the last stored frame at or before entry n (-1: none); rels[n] = P (-) S_a when the entry
    was made; C [K, 12]: the corrected poses -> [(t, C_a (+) rel)], entries without a frame as they are"""
    return [(t, np.asarray(p, np.float64) if a < 0 else compose(C[a], rel)) for (t, p), a, rel in zip(trajectory, anchors, rels)]


def rebuild_frames(kf, k, C_i):
    """the frames a closure rebuilds map k from: with points, corrected position within the map's recorded remove_voxels_farther_than
    of C_i (0: all)"""
    far = float(kf["maps"][k]["remove_voxels_farther_than"])
    c = np.asarray(C_i, np.float64)[[3, 7, 11]]
    return [n for n, f in enumerate(kf["frames"])
            if f["layers"] is not None and (not far > 0.0 or float(np.linalg.norm(np.asarray(f["pose"], np.float64)[[3, 7, 11]] - c)) <= far)]


# ---- the candidate step folded ---------------------------------------------------------------------------------------------------------
def fold_candidates(step, poses, has_points, matches, opt, accept=None, frames=None):
    """loop_candidates as the fold of the per-frame step over `frames` (default: all); step = host.loop_candidates_step"""
    poses = np.asarray(poses, np.float64).reshape(-1, 12)
    tried, state = [], None
    for i in (range(len(poses)) if frames is None else frames):
        got, _, state = step(poses[:i + 1], list(has_points[:i + 1]), matches[i], opt, state, accept)
        tried += [tuple(p) for p in got]
    return tried


# ---- the reference's key-frames of the drive ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def oracle_keyframes():
    """the key-frame dict the CPU oracle's driver records on drive() under pipeline_text(): the scans tests/simplemap_ref.py's rule
    stores (every one with points), their poses and the map layer their second pass left"""
    d = drive()
    o = lr.oo.OdometryOracle(text=pipeline_text())
    recs, layers = [], []
    for (xyz, t), st in zip(d["scans"], d["stamps"]):
        recs.append(dict(o.on_lidar(st, xyz, t)))
        layers.append(np.array(o.for_map, np.float32))
    live = [n for n, r in enumerate(recs) if not r["dropped"]]
    lim_r = [15.0 + 500.0 * float(np.linalg.norm(recs[n]["twist"][3:])) for n in live]   # the pipeline file's formula [deg]
    stored, keyframe = simplemap_ref.decide([recs[n]["pose"] for n in live], [recs[n]["icp_good"] for n in live], KF_SPACING, lim_r,
                                            measure_from_last_kf_only=True, first_scan=[recs[n]["first_scan"] for n in live])
    assert list(stored) == list(keyframe)
    maps = [dict(name="localmap", class_name="HashedVoxelPointCloud", remove_voxels_farther_than=float(o.remove_far),
                 params=dict(lc.MAP_PARAMS, voxel_size=float(o._map_args[0]), max_points_per_voxel=int(o._map_args[1]),
                             min_distance_between_points=float(o._map_args[3])))]
    frames = [dict(timestamp=recs[n]["timestamp"], pose=[float(v) for v in recs[n]["pose"]], cov=[0.0] * 36, twist=None, layers=[(0, layers[n])])
              for n, s in zip(live, stored) if s]
    return dict(maps=maps, frames=frames, records=recs)


@functools.lru_cache(maxsize=1)
def oracle_reference():
    """tests/loop_ref.py on the oracle's key-frames of the drive, under the drive's options"""
    kf = oracle_keyframes()
    return lr.close_loops(kf["maps"], kf["frames"], lr.oo.load_pipeline_text(pipeline_text()))


# ---- the CPU oracle's driver with the key-frame store and the feedback rules --------------------------------------------------------------
class OnlineOracle(lr.oo.OdometryOracle):
    """oracle.odometry_oracle.OdometryOracle on the pipeline of pipeline_text(): after every scan's own map update the store's rule
    (measure_from_last_kf_only), the raw chain, the candidate rule for the new frame (tests/loop_ref.py's, one frame of it) on match
    lists of tests/place_ref.py against the frames before, loop_ref.Verifier's verification on the raw frames, loop_ref.optimize from
    the raw chain with every loop so far; with correct_driver the store's poses follow, and a closure moves the last pose and the
    motion model by delta, rebuilds the map from the key-frames around and makes their poses the local-map key-frame list."""

    def __init__(self, block="", correct_driver=True):
        super().__init__(text=pipeline_text(block))
        self.correct = correct_driver
        self.opt = lr.options(self.cfg)
        self.frames, self.raw, self.descs = [], [], []   # the store (dicts like a key-frame file's), the raw poses, the descriptors
        self.checker_frame, self.closed_at, self.loops, self.verified, self.cache = None, None, [], [], {}
        self.corrected = np.zeros((0, 12))

    def _maps(self):
        return [dict(name="localmap", class_name="HashedVoxelPointCloud", remove_voxels_farther_than=float(self.remove_far),
                     params=dict(lc.MAP_PARAMS, voxel_size=float(self._map_args[0]), max_points_per_voxel=int(self._map_args[1]),
                                 min_distance_between_points=float(self._map_args[3])))]

    def _stored(self, rec):
        pose = np.array(rec["pose"], np.float64)
        if rec["first_scan"]:
            return True                                   # (the checker is not touched)
        if not rec["icp_good"]:
            return False
        enough = self.checker_frame is None
        if not enough:
            d, a = simplemap_ref._rel(pose, self.checker_pose)
            enough = d > KF_SPACING or a > np.deg2rad(15.0 + 500.0 * float(np.linalg.norm(rec["twist"][3:])))
        if enough:
            self.checker_frame, self.checker_pose = len(self.frames), pose
        return enough

    def on_lidar(self, stamp, xyz, t=None):
        rec = super().on_lidar(stamp, xyz, t)
        rec.update(simplemap_frame=False, loop_tried=False, loop_closed=False, loop_pairs=[])
        if rec["dropped"] or rec["restarted"] or not self._stored(rec):
            return rec
        rec["simplemap_frame"] = True
        P = np.array(rec["pose"], np.float64)
        k = len(self.frames)
        raw = P if k == 0 or np.array_equal(self.raw[-1], self.frames[-1]["pose"]) else raw_pose(self.raw[-1], P, self.frames[-1]["pose"])
        self.frames.append(dict(timestamp=stamp, pose=P.copy(), layers=[(0, np.array(self.for_map, np.float32))]))
        self.raw.append(np.asarray(raw, np.float64))
        # the new frame against the frames before it, then into the database
        desc = lr.pr.describe(self.frames[k]["layers"][0][1], **lr.pr.DEFAULT)
        matches = []
        if k:
            shift, dist = lr.pr.search(np.stack(self.descs), desc)
            matches = [(int(r), int(shift[r]), int(dist[r])) for r in lr.pr.rank(shift, dist)]
        self.descs.append(desc)
        raw_frames = [dict(f, pose=[float(v) for v in r]) for f, r in zip(self.frames, self.raw)]
        v = lr.Verifier(self._maps(), raw_frames, self.cfg, cache=self.cache)
        s = v.s
        closed = False
        if not (self.closed_at is not None and s[k] < self.closed_at + self.opt["min_travel_between_closures"]):
            n = 0
            for j, shift, dist in matches:      # loop_ref.candidates, frame k of it
                if n >= self.opt["top_k"]:
                    break
                travel = s[k] - s[j]
                if not travel >= self.opt["min_travel"]:
                    continue
                if not float(np.linalg.norm(self.raw[k][[3, 7, 11]] - self.raw[j][[3, 7, 11]])) <= self.opt["gate_base"] + self.opt["gate_rate"] * travel:
                    continue
                if self.opt["max_place_dist"] != 0 and dist > self.opt["max_place_dist"]:
                    continue
                n += 1
                ok = v.verify(k, j, shift, dist)
                p = v.pairs[-1]
                self.verified.append(p)
                rec["loop_pairs"].append((k, j, p["quality"], p["accepted"]))
                if ok:
                    self.loops.append((j, k, p["Z"]))
                    self.closed_at, closed = s[k], True
                    break
        rec["loop_tried"], rec["loop_closed"] = len(rec["loop_pairs"]) > 0, closed
        self.corrected = lr.optimize(np.array(self.raw), self.loops, self.opt)[0] if self.loops else np.array(self.raw)
        if not self.correct or not self.loops:
            return rec
        for f, c in zip(self.frames, self.corrected):
            f["pose"] = np.array(c, np.float64)
        if self.checker_frame is not None:
            self.checker_pose = self.frames[self.checker_frame]["pose"]
        if closed:
            C = self.frames[-1]["pose"]
            delta = correction(C, self.last_pose)
            self.last_pose = C.copy()
            if self.nav_last is not None:
                self.nav_last = (self.nav_last[0], compose(delta, self.nav_last[1]))
            if self.last_mm is not None:
                self.last_mm = (compose(delta, self.last_mm[0]),) + tuple(self.last_mm[1:])
            keep = rebuild_frames(dict(maps=self._maps(), frames=self.frames), 0, C)
            self.map = lr.oc.Map(*self._map_args)
            for q in keep:
                self.map.insert_posed(self.frames[q]["layers"][0][1], self.frames[q]["pose"], 0.0)
            self.kfs = [self.frames[q]["pose"].copy() for q in keep]
            rec["pose"] = self.last_pose.copy()
            rec["loop_rebuilt_frames"] = len(keep)
            self._record_maps(rec)
        return rec
