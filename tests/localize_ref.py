"""Localization in a saved map restated on the CPU oracle driver: LocalizeOracle subclasses oracle.odometry_oracle.OdometryOracle
(nothing under oracle/ is touched) and adds what mola_hip::LidarOdometry adds --

  * a preloaded map: the oracle's map filled from a dump in storage order (voxel by voxel, in-voxel insertion order: inserting
    the stored points in that order into an empty map stores exactly them again -- every one passed the cap and the clearance
    rule against its predecessors when it was first stored);
  * initial_localization: the fixed pose fused into the motion model at t - 0.2 and t - 0.1, once, at the first observation that
    reaches registration;
  * the relocalization request: grid (score_ref.relocalization_grid) -> score_ref.score_poses -> rank, top k ->
    oracle_c.icp_align from each, no prior, no hook -> the best quality wins, ties to the better rank -> accepted at
    min_icp_goodness: motion model reset and seeded, last pose set.

No product code."""
import math
import os

import numpy as np

import score_ref as sr
from oracle import odometry_oracle as oo
from oracle import oracle_c as oc


class LocalizeOracle(oo.OdometryOracle):
    def __init__(self, pipeline_yaml_path=None, n_threads=8, text=None):
        self._preload = None
        super().__init__(pipeline_yaml_path, n_threads=n_threads, text=text)
        il = self.cfg.get("initial_localization") or {}
        self.il_enabled = oo._b(il.get("enabled", False))
        self.il_pose = np.array([float(v) for v in il.get("fixed_initial_pose", [0.0] * 6)])
        rs = il.get("relocalize_sigmas") or []
        self.il_sigmas = [float(v) for v in rs] if len(rs) == 3 else None
        r = self.cfg.get("relocalization") or {}
        self.reloc = dict(score_threshold=r.get("score_threshold"), step_xy=r.get("step_xy"), step_yaw_deg=float(r.get("step_yaw_deg", 3.0)),
                          sigmas=float(r.get("sigmas", 3.0)), refine_top_k=int(r.get("refine_top_k", 4)),
                          max_candidates=int(r.get("max_candidates", 65536)))

    # ---- a saved map
    def preload(self, rec):
        """rec: one map of host.read_local_map_file() (name, params, remove_voxels_farther_than, xyz in storage order)"""
        self._preload = rec
        self._restore()

    def _restore(self):
        p = self._preload["params"]
        self._map_args = (np.float32(p["voxel_size"]), int(p["max_points_per_voxel"]), int(p["index_mode"]),
                          float(np.float32(p["min_distance_between_points"])), float(np.float32(p["ndt_max_eigen_ratio"])),
                          int(p["ndt_min_points"]) if p["ndt_max_eigen_ratio"] > 0 else 4)
        self.voxel_size = float(np.float32(p["voxel_size"]))
        self.remove_far = float(np.float32(self._preload["remove_voxels_farther_than"]))
        self.map = oc.Map(*self._map_args)
        if len(self._preload["xyz"]):
            self.map.insert(self._preload["xyz"])

    def reset(self):
        super().reset()
        self._init_done = False
        self.request = None   # (mean as x y z yaw pitch roll, 6x6 covariance)
        if self._preload is not None:
            self._restore()

    # ---- initial localization and relocalization
    def _seed(self, stamp, pose):
        self._nav_fuse(stamp - 0.2, pose)
        self._nav_fuse(stamp - 0.1, pose)

    def relocalize_near_pose(self, mean_ypr, cov):
        self.request = (np.asarray(mean_ypr, np.float64), np.asarray(cov, np.float64).reshape(36))

    def _score_threshold(self):
        e = self.reloc["score_threshold"]
        return oo.formula(e, self.vars) if e not in (None, "", "~") else 0.5 * self.voxel_size

    def _refine(self, T0):
        ip = self.icp["params"]
        n = int(ip["maxIterations"])
        thr, kp, pl = self._schedules(n)
        q = oc.ICPParams(max_iterations=n, min_abs_step_trans=float(ip["minAbsStep_trans"]), min_abs_step_rot=float(ip["minAbsStep_rot"]),
                         threshold=thr, kernel_param=kp, pt2pl_threshold=pl, threshold_angular_deg=0.0,
                         gn=oc.GNParams(max_inner_iterations=int(self.solver["maxIterations"]),
                                        robust_kernel=oo._KERNELS[str(self.solver.get("robustKernel", "GemanMcClure")).split("::")[-1]]),
                         hook_enabled=False,
                         pt2pt_skip_plane_paired=os.environ.get("MOLA_HIP_MATCHED_POINTS", "again") in ("skip", "1"))
        return self._align(T0, q, None, {})

    def _serve(self, stamp, rec):
        mean, cov = self.request
        thr = self._score_threshold()
        step = self.reloc["step_xy"]
        step = float(step) if step not in (None, "", "~") and float(step) > 0 else thr
        poses, rows = sr.relocalization_grid(mean, cov, step, math.radians(self.reloc["step_yaw_deg"]), self.reloc["sigmas"])
        assert len(poses) <= self.reloc["max_candidates"]
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
            rec["relocalized"] = True

    def _register(self, stamp, rec):
        rec.update(relocalization_tried=False, relocalized=False, reloc_candidates=0, reloc_best_n_paired=0, reloc_best_quality=0.0,
                   reloc_ranks=[])
        if self.il_enabled and not self._init_done:
            if self.il_sigmas is not None:
                self.relocalize_near_pose(self.il_pose, sr.grid_cov(self.il_sigmas[0], self.il_sigmas[1], math.radians(self.il_sigmas[2])))
            else:
                self._seed(stamp, oc.pose_from_ypr(self.il_pose))
            self._init_done = True
        if self.request is not None and not self._maps_empty():
            self._serve(stamp, rec)
        return super()._register(stamp, rec)
