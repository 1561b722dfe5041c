"""relocalizeInKeyFrames restated on the CPU: PlaceOracle extends tests/localize_ref.py's LocalizeOracle (which is not touched)
by the request without a coarse pose --

  * the descriptors of the key-frames' first stored layer and of this scan's map-input layer: tests/place_ref.py;
  * search, rank by (dist ascending, frame ascending), keep place_top_k;
  * per kept frame mean = frame pose (+) Rz(-shift * 2 pi / S) and score_ref.relocalization_grid around it with
    diag(place_sigma_xy^2, place_sigma_xy^2, ., place_sigma_yaw^2, ., .); the lists concatenated in rank order;
  * the tail of LocalizeOracle._serve on the concatenated list: score, rank, refine, accept.

No product code."""
import math

import numpy as np

import localize_ref
import place_ref as pr
import score_ref as sr
from oracle import oracle_c as oc

PLACE_DEFAULTS = dict(place_rings=20, place_sectors=64, place_min_range=1.0, place_max_range=80.0, place_z_min=-3.0, place_z_max=27.0,
                      place_top_k=4, place_sigma_xy=1.0, place_sigma_yaw_deg=5.625)


def to44(T12):
    return np.vstack([np.asarray(T12, np.float64).reshape(3, 4), [0, 0, 0, 1]])


def place_mean(frame_pose12, shift, n_sectors):
    """frame pose (+) Rz(-shift * 2 pi / S) as (x, y, z, yaw, pitch, roll)"""
    rz = oc.pose_from_ypr(np.array([0, 0, 0, -float(shift) * 2.0 * math.pi / n_sectors, 0, 0]))
    return oc.pose_to_ypr((to44(frame_pose12) @ to44(rz))[:3].reshape(12))


class PlaceOracle(localize_ref.LocalizeOracle):
    def __init__(self, pipeline_yaml_path=None, n_threads=8, text=None):
        super().__init__(pipeline_yaml_path, n_threads=n_threads, text=text)
        r = self.cfg.get("relocalization") or {}
        self.place = {k: type(v)(float(r.get(k, v))) for k, v in PLACE_DEFAULTS.items()}
        self.keyframes = []   # (frame index, pose12, xyz of layers[0]) of the frames with points
        self.in_keyframes = False

    def params(self):
        p = self.place
        return dict(n_rings=p["place_rings"], n_sectors=p["place_sectors"], min_range=p["place_min_range"], max_range=p["place_max_range"],
                    z_min=p["place_z_min"], z_max=p["place_z_max"])

    def set_keyframes(self, frames):
        """frames: the "frames" list of host.read_keyframe_file() / lo.keyFrames()"""
        self.keyframes = [(i, np.array(f["pose"], np.float64), np.asarray(f["layers"][0][1], np.float32))
                          for i, f in enumerate(frames) if f["layers"] is not None and len(f["layers"]) and len(f["layers"][0][1])]
        self._descs = np.stack([pr.describe(xyz, **self.params()) for _, _, xyz in self.keyframes]) if self.keyframes else None

    def relocalize_in_keyframes(self):
        self.in_keyframes = True
        self.request = "keyframes"

    def place_search(self, layer):
        """[(frame, shift, dist)] of every key-frame with points, ranked"""
        shift, dist = pr.search(self._descs, pr.describe(layer, **self.params()))
        frames = np.array([i for i, _, _ in self.keyframes])
        order = np.lexsort((frames, dist))
        return [(int(frames[k]), int(shift[k]), int(dist[k])) for k in order]

    def _serve(self, stamp, rec):
        if not self.in_keyframes:
            return super()._serve(stamp, rec)
        p = self.place
        kept = self.place_search(self.for_map)[:p["place_top_k"]]
        rec.update(place_tried=True, place_frames=[k[0] for k in kept], place_shifts=[k[1] for k in kept], place_dists=[k[2] for k in kept])
        thr = self._score_threshold()
        step = self.reloc["step_xy"]
        step = float(step) if step not in (None, "", "~") and float(step) > 0 else thr
        cov = sr.grid_cov(p["place_sigma_xy"], p["place_sigma_xy"], math.radians(p["place_sigma_yaw_deg"]))
        pose_of = {i: T for i, T, _ in self.keyframes}
        lists = [sr.relocalization_grid(place_mean(pose_of[f], s, p["place_sectors"]), cov, step, math.radians(self.reloc["step_yaw_deg"]),
                                        self.reloc["sigmas"])[0] for f, s, _ in kept]
        poses = np.concatenate(lists, 0)
        assert len(poses) <= self.reloc["max_candidates"]
        # ---- from here on: LocalizeOracle._serve, word for word, on the concatenated list
        scores = sr.score_poses(oc, self.map, self.for_icp, poses, thr)
        order = sr.rank(scores)[:self.reloc["refine_top_k"]]
        rec.update(relocalization_tried=True, relocalized=False, reloc_candidates=len(poses), reloc_ranks=[int(c) for c in order],
                   reloc_best_n_paired=int(scores["n_paired"][order[0]]) if len(order) else 0)
        best = None
        for c in order:
            res = self._refine(poses[c])
            if best is None or res["quality"] > best["quality"]:
                best = res
        rec["reloc_best_quality"] = best["quality"] if best is not None else 0.0
        if best is not None and best["quality"] >= float(self.p["min_icp_goodness"]):
            self._nav_reset()
            self._seed(stamp, best["T"])
            self.last_pose = best["T"].copy()
            self.request = None
            self.in_keyframes = False
            rec["relocalized"] = True

    def _register(self, stamp, rec):
        rec.update(place_tried=False, place_frames=[], place_shifts=[], place_dists=[])
        return super()._register(stamp, rec)


def cpu_session(pipe, scene):
    """The scenario of place_cases on the CPU alone: every key-frame sweep through a fresh reference driver as its first scan
    (its map-input layer is what a key-frame stores), then the session map of all frames as the oracle's map stores it.
    -> (frames as read_keyframe_file() gives them, the map as read_local_map_file() gives it)"""
    import place_cases as pc
    frames, args = [], None
    for k, (xyz, t) in enumerate(pc.kf_sweeps(scene)):
        o = PlaceOracle(pipe)
        assert o.on_lidar(1000.0 + k, xyz, t)["first_scan"]
        if args is None:
            args = o._map_args
        frames.append(dict(timestamp=1000.0 + k, pose=[float(v) for v in pc.synth.pose_from_ypr(pc.kf_pose(k))], cov=[0.0] * 36, twist=None,
                           layers=[(0, o.for_map.copy())]))
    m = oc.Map(*args)
    for f in frames:
        m.insert_posed(f["layers"][0][1], np.array(f["pose"]), 0.0)
    rec = dict(name="localmap", params=dict(voxel_size=args[0], max_points_per_voxel=args[1], index_mode=args[2], min_distance_between_points=args[3],
                                            ndt_max_eigen_ratio=args[4], ndt_min_points=args[5]), remove_voxels_farther_than=0.0,
               xyz=m.dump()["xyz"])
    return frames, rec
