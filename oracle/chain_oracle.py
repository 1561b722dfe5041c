"""CPU oracle of the stand-alone driver on GENERAL filter chains (the C++ driver's GeneralPlan): ordered filter steps over named
observation layers, one local map per localmap_generator entry, one FilterMerge per (layer, map), and every pointLayerMatches
entry of the ICP pipeline as a weighted (map, layer) pair of one Gauss-Newton solve.

TEST INFRASTRUCTURE, like the rest of oracle/.  ChainOdometryOracle keeps OdometryOracle's motion model, adaptive threshold,
key-frame list, restart logic and twist-hook loop unchanged (it overrides only the parts that touch layers and maps) and its own
reading of the YAML; nothing here imports the C++ host layer.  Every step runs on the CPU restatement that pins the device
entry point of the same name: oracle_c.{deskew, filter_by_range, filter_bbox, decimate_*, adjust_timestamps} and
oracle/filters_np.py.  The alignment is oracle/layers_oracle.py (float64, numpy solve), whose `margins` and `max_cond` -- with
the goodness and key-frame comparisons OdometryOracle adds -- are kept per scan so that a comparison against the device can
tell a decision within rounding of its threshold from a mismatch (ChainOdometryOracle.set_apart).  A pipeline with a
Matcher_Point2Plane (one pair per matcher: the NDT pipeline) goes through oracle_c.icp_align as OdometryOracle's does.

Layers are dicts {xyz (n,3) float32, t (n) float32 or None, intensity (n) float32 or None, src_idx (n) uint32 or None}.  src_idx
follows the device's rule: 'raw' has none; FilterDeskew hands its input's on; every other filter gives each output point its
index in 'raw'.

Which moment `layer_sizes` describes: the layers that were finally aligned and merged, i.e. AFTER the last re-run of the 2nd
pass the twist hook asked for -- what mola::LidarOdometry::onLidarImpl hands to its last align() and to the map update
(module/src/LidarOdometry.cpp:973-1004, 1158-1206)."""
from __future__ import annotations

import math

import numpy as np

from . import filters_np as fnp
from . import layers_oracle as lo
from . import oracle_c as oc
from .odometry_oracle import OdometryOracle, _b, _bbox_radius, _decimate_method, formula

_TWIST = ("vx", "vy", "vz", "wx", "wy", "wz")


def ulp_distance(a, b):
    """Largest distance, in float32 steps, between the elements of two float32 arrays of one shape (inf for a NaN mismatch)."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape:
        return math.inf
    if a.size == 0:
        return 0
    if not np.array_equal(np.isnan(a), np.isnan(b)):
        return math.inf
    def key(x):  # order-preserving integers: adjacent floats differ by 1 (-0 and +0 coincide)
        i = x.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    d = np.abs(key(a) - key(b))
    d[np.isnan(a)] = 0
    return int(d.max())


def _layer(xyz, t=None, intensity=None, src=None):
    return dict(xyz=np.ascontiguousarray(xyz, np.float32).reshape(-1, 3), t=t, intensity=intensity, src_idx=src)


def _take(lay, idx):
    """The points `idx` of a layer (indices or mask) as a filter output: src_idx = index in 'raw'."""
    idx = np.nonzero(idx)[0] if getattr(idx, "dtype", None) == np.bool_ else np.asarray(idx, np.int64)
    src = idx.astype(np.uint32) if lay["src_idx"] is None else lay["src_idx"][idx]
    return dict(xyz=lay["xyz"][idx], t=None if lay["t"] is None else lay["t"][idx],
                intensity=None if lay["intensity"] is None else lay["intensity"][idx], src_idx=src)


def _names(v):
    return [] if v is None else ([str(e) for e in v] if isinstance(v, (list, tuple)) else [str(v)])


class ChainOdometryOracle(OdometryOracle):
    # ---------------------------------------------------------------- the plan
    def _load_chain(self, c):
        self.steps = []  # dicts: kind, pass, cls, in, out [...], the step's parameters (formulas unevaluated)
        self.ts_method, self.ts_offset = oc.TS_NONE, 0.0
        for e in c.get("observations_filter_adjust_timestamps") or []:
            assert e["class_name"].endswith("FilterAdjustTimestamps"), e["class_name"]
            p = e["params"]
            assert p.get("pointcloud_layer", "raw") == "raw"
            m = str(p.get("method", "TimestampAdjustMethod::MiddleIsZero"))
            self.ts_method = oc.TS_MIDDLE_IS_ZERO if m.endswith("MiddleIsZero") else oc.TS_EARLIEST_IS_ZERO
            assert m.endswith("MiddleIsZero") or m.endswith("EarliestIsZero"), m
            self.ts_offset = p.get("time_offset", 0.0)
        known = {"raw"}
        for pass_, key in ((1, "observations_filter_1st_pass"), (2, "observations_filter_2nd_pass")):
            for e in c.get(key) or []:
                self._load_step(e["class_name"].split("::")[-1], e.get("params") or {}, pass_, known)
        self.map_defs = []  # (name, metric_map_definition)
        for e in c["localmap_generator"]:
            p = e["params"]
            self.map_defs.append((str(p.get("target_layer", "localmap")), p["metric_map_definition"]))
        assert len({n for n, _ in self.map_defs}) == len(self.map_defs) > 0
        self.merges = []  # (layer, map name)
        for e in c["insert_observation_into_local_map"]:
            assert e["class_name"].endswith("FilterMerge"), e["class_name"]
            p = e["params"]
            layer, target = str(p["input_pointcloud_layer"]), str(p.get("target_layer", "localmap"))
            assert layer in known and target in dict(self.map_defs), (layer, target)
            assert _b(p.get("input_layer_in_local_coordinates", True))
            self.merges.append((layer, target))
        assert self.merges
        # ICP: every pointLayerMatches entry of every point matcher, in matching order
        self.pair_defs, self.plane_matchers = [], []
        for j, m in enumerate(self.matchers):
            if not _b((m.get("params") or {}).get("enabled", True)):
                continue
            if m["class"].endswith("Matcher_Point2Plane"):
                self.plane_matchers.append(m)
                continue
            assert m["class"].endswith("Matcher_Points_DistanceThreshold"), m["class"]
            for lm in m["params"]["pointLayerMatches"]:
                self.pair_defs.append(dict(map=str(lm["global"]), local=str(lm["local"]), weight=float(lm.get("weight", 1.0)),
                                           threshold=m["params"]["threshold"],
                                           angular=m["params"].get("thresholdAngularDeg", 0.0)))
        if self.plane_matchers:  # (layers_oracle stacks point-to-point rows only)
            assert len(self.pair_defs) == 1 and len(self.plane_matchers) == 1, "Matcher_Point2Plane next to several point pairs"

    def _load_step(self, cls, p, pass_, known):
        st = dict(cls=cls, p=p)
        st["pass"] = pass_

        def inp(key="input_pointcloud_layer"):
            st["in"] = str(p[key])
            assert st["in"] in known, "%s reads layer '%s', which no earlier filter writes" % (cls, st["in"])

        def outs(keys):
            st["out"] = [str(p[k]) if p.get(k) else "" for k in keys]
            assert any(st["out"]) and all(o not in ("raw", st["in"]) for o in st["out"] if o)
            known.update(o for o in st["out"] if o)

        if cls == "FilterDeleteLayer":
            st["kind"], st["out"] = "delete", _names(p["pointcloud_layer_to_remove"])
            known.difference_update(st["out"])
        elif cls == "FilterDeskew":
            st["kind"] = "deskew"
            inp()
            outs(["output_pointcloud_layer"])
        elif cls == "FilterByRange":
            st["kind"] = "range"
            inp()
            assert "output_layer_outside" not in p and "center" not in p
            outs(["output_layer_between"])
        elif cls == "FilterBoundingBox":  # one step per output layer, inside first (as the C++ plan splits it)
            for key, inside in (("inside_pointcloud_layer", True), ("outside_pointcloud_layer", False)):
                if p.get(key):
                    b = dict(cls=cls, p=p, kind="bbox", inside=inside)
                    b["pass"] = pass_
                    b["in"] = str(p["input_pointcloud_layer"])
                    assert b["in"] in known
                    b["out"] = [str(p[key])]
                    self.steps.append(b)
            assert self.steps and self.steps[-1]["p"] is p, "FilterBoundingBox without an output layer"
            known.update(s["out"][0] for s in self.steps if s["p"] is p)
            return
        elif cls == "FilterDecimateVoxels":
            st["kind"], st["method"] = "decimate", _decimate_method(p)
            inp()
            outs(["output_pointcloud_layer"])
        elif cls == "FilterCurvature":
            st["kind"] = "curvature"
            inp()
            outs(["output_layer_larger_curvature", "output_layer_smaller_curvature", "output_layer_other"])
        elif cls == "FilterNormalizeIntensity":
            assert pass_ == 1, "FilterNormalizeIntensity in observations_filter_2nd_pass"
            st["kind"], st["out"] = "normalize", []
            inp("pointcloud_layer")
            st["remember"] = _b(p.get("remember_intensity_range", False))
        elif cls == "FilterByIntensity":
            st["kind"] = "by_intensity"
            inp()
            outs(["output_layer_low_intensity", "output_layer_mid_intensity", "output_layer_high_intensity"])
        else:
            raise ValueError("unsupported filter " + cls)
        self.steps.append(st)

    def describe(self):
        """The plan in the words of the C++ driver's describePipeline(): steps, maps, merges, weighted pairs."""
        lines = []
        for st in self.steps:
            line = "pass%d %s" % (st["pass"], st["cls"])
            if st["kind"] == "delete":
                line += " " + ",".join(st["out"])
            elif st["kind"] == "normalize":
                line += " " + st["in"] + " (in place" + (", remembered range)" if st["remember"] else ")")
            else:
                line += " " + st["in"] + " ->" + "".join(("," if i else " ") + (o or "-") for i, o in enumerate(st["out"]))
                if st["kind"] == "bbox":
                    line += " (inside)" if st["inside"] else " (outside)"
            lines.append(line)
        return dict(steps=lines, maps={n: d["class"] for n, d in self.map_defs}, merges=list(self.merges),
                    pairs=[(d["map"], d["local"], d["weight"]) for d in self.pair_defs], timestamp_method=self.ts_method)

    # ---------------------------------------------------------------- state
    def reset(self):
        super().reset()
        self.maps = {}        # name -> dict(map, args, voxel_size, remove_far), created at the first key-frame
        self.remembered = {}  # index of a FilterNormalizeIntensity step -> its remembered {min, max}
        self.layers = {}
        self.forced = None

    # ---------------------------------------------------------------- filters
    def _run_pass(self, pass_, layers):
        v = self.vars
        tw = [v[k] for k in _TWIST]
        for k, st in enumerate(self.steps):
            if st["pass"] != pass_:
                continue
            kind, p = st["kind"], st["p"]
            if kind == "delete":
                for n in st["out"]:
                    layers.pop(n, None)
                continue
            assert st["in"] in layers, "%s reads the deleted layer '%s'" % (st["cls"], st["in"])
            src = layers[st["in"]]
            if kind == "normalize":  # in place; the remembered range belongs to the step
                if src["intensity"] is None:
                    raise ValueError("FilterNormalizeIntensity: the layer carries no intensity")
                rng = self.remembered.get(k, np.array([np.nan, np.nan], np.float32)) if st["remember"] else None
                new, rng = fnp.normalize_np(src["intensity"], rng)
                layers[st["in"]] = dict(src, intensity=new)
                if st["remember"]:
                    self.remembered[k] = rng
                continue
            if kind == "deskew":
                name = st["out"][0]
                if src["t"] is None or _b(p.get("skip_deskew", False)) or len(src["xyz"]) == 0:
                    xyz = src["xyz"].copy()
                else:
                    xyz = oc.deskew(src["xyz"], src["t"], tw)
                if self.forced is not None and name in self.forced:
                    # the device's de-skewed layer (fp64 sin / cos differ between libm and the device): held to 1 ulp, then
                    # taken over, so that everything downstream is compared bit for bit
                    d = ulp_distance(xyz, self.forced[name])
                    self.deskew_ulps[name] = d
                    if d <= 1:
                        xyz = np.ascontiguousarray(self.forced[name], np.float32).reshape(-1, 3).copy()
                layers[name] = dict(src, xyz=xyz)
                continue
            if kind in ("range", "bbox", "decimate"):
                fin = np.nonzero(np.isfinite(src["xyz"]).all(1))[0]  # (every preprocess call keeps the finite points)
                x = src["xyz"][fin]
                if kind == "range":
                    keep = oc.filter_by_range(x, formula(p["range_min"], v), formula(p["range_max"], v))
                elif kind == "bbox":
                    keep = oc.filter_bbox(x, [formula(e, v) for e in p["bounding_box_min"]],
                                          [formula(e, v) for e in p["bounding_box_max"]], keep_inside=st["inside"])
                else:
                    fn = oc.decimate_first_point if st["method"] == oc.DECIMATE_FIRST_POINT else oc.decimate_closest_to_average
                    keep = fn(x, formula(p["voxel_filter_resolution"], v), int(float(p.get("minimum_input_points_to_filter", 0))))
                layers[st["out"][0]] = _take(src, fin[keep])
                continue
            if kind == "curvature":
                cls = fnp.curvature_classes(src["xyz"], formula(p["max_cosine"], v), formula(p["min_clearance"], v),
                                            formula(p["max_gap"], v))
            else:
                if src["intensity"] is None:
                    raise ValueError("FilterByIntensity: the layer carries no intensity")
                cls = fnp.intensity_classes(src["intensity"], formula(p["low_threshold"], v), formula(p["high_threshold"], v))
            for c, name in enumerate(st["out"]):
                if name:
                    layers[name] = _take(src, cls == c)
        return layers

    def _sizes(self, rec):
        rec["layer_sizes"] = {n: len(l["xyz"]) for n, l in self.layers.items()}
        rec["n_for_icp"] = sum(rec["layer_sizes"].values())
        rec["n_for_map"] = sum(rec["layer_sizes"][n] for n, _ in self.merges if n in rec["layer_sizes"])

    def _run_filters(self, xyz, t, rec):
        # 'raw' carries the intensity only when a filter reads it (the driver ignores the field otherwise)
        reads_i = any(st["kind"] in ("normalize", "by_intensity") for st in self.steps)
        if reads_i and self._intensity is None:
            raise ValueError("the pipeline's intensity filters need a per-point intensity, and this scan carries none")
        raw = _layer(xyz, None if t is None else np.ascontiguousarray(t, np.float32),
                     np.ascontiguousarray(self._intensity, np.float32) if reads_i else None)
        if self.ts_method != oc.TS_NONE:  # (a preprocess call of its own on the device: finite points, indexed into 'raw')
            raw = _take(raw, np.isfinite(raw["xyz"]).all(1))
            if raw["t"] is not None:
                raw["t"] = oc.adjust_timestamps(raw["t"], self.ts_method, formula(self.ts_offset, self.vars))
        self.deskew_ulps = {}
        self.layers1 = self._run_pass(1, {"raw": raw})
        self.layers = self._run_pass(2, dict(self.layers1))
        self._sizes(rec)
        rec["decim_map_resolution"] = rec["decim_icp_resolution"] = 0.0
        # the sensor-range estimate reads the alphabetically first layer of the observation (LidarOdometry.cpp:1515-1545)
        if not self.layers:
            return np.zeros((0, 3), np.float32)
        first = self.layers[sorted(self.layers)[0]]["xyz"]
        return first[np.isfinite(first).all(1)]

    def _redo_second_pass(self, rec):
        self.layers = self._run_pass(2, dict(self.layers1))  # from the layers alive after the 1st pass
        self._sizes(rec)

    # ---------------------------------------------------------------- maps
    def _maps_empty(self):
        return not self.maps or sum(m["map"].num_points for m in self.maps.values()) == 0

    def _clear_maps(self):
        for m in self.maps.values():
            m["map"] = oc.Map(*m["args"])
        self.map = self.maps[self.map_defs[0][0]]["map"] if self.maps else None

    def _create_maps(self):
        for name, d in self.map_defs:
            args, voxel_size, far = self._map_args_of(d)
            self.maps[name] = dict(map=oc.Map(*args), args=args, voxel_size=voxel_size, remove_far=far)
        self.map = self.maps[self.map_defs[0][0]]["map"]
        self.voxel_size = self.maps[self.map_defs[0][0]]["voxel_size"]

    def _insert_into_maps(self):
        for layer, target in self.merges:
            if layer in self.layers:
                m = self.maps[target]
                m["map"].insert_posed(self.layers[layer]["xyz"], self.last_pose, m["remove_far"])

    def _record_maps(self, rec):
        rec["maps"] = {n: (m["map"].num_points, m["map"].num_voxels, m["voxel_size"]) for n, m in self.maps.items()}
        rec["n_map_points"] = sum(v[0] for v in rec["maps"].values())
        rec["n_map_voxels"] = sum(v[1] for v in rec["maps"].values())

    # ---------------------------------------------------------------- ICP
    def _align(self, T0, q, prior, rec):
        n = q.max_iterations
        if self.plane_matchers:  # one point pair + one plane matcher: the C oracle, as OdometryOracle
            d = self.pair_defs[0]
            return oc.icp_align(self.maps[d["map"]]["map"], self.layers[d["local"]]["xyz"], T0, q, prior=prior,
                                n_threads=self.n_threads)
        pairs = []
        for d in self.pair_defs:
            thr = np.array([formula(d["threshold"], {**self.vars, "ICP_ITERATION": float(k)}) for k in range(max(1, n))])
            pairs.append(dict(map=self.maps[d["map"]]["map"], local=self.layers[d["local"]]["xyz"], threshold=thr,
                              threshold_angular_deg=formula(d["angular"], self.vars), weight=d["weight"]))
        res = lo.icp_align_layers(pairs, T0, q, prior=prior, n_threads=self.n_threads)
        rec.setdefault("icp_margins", []).extend(res["margins"])
        rec["max_cond"] = max(rec.get("max_cond", 0.0), res["max_cond"])
        return res

    def _schedules(self, n):
        if self.plane_matchers:
            return super()._schedules(n)
        kp = np.array([formula(self.solver["robustKernelParam"], {**self.vars, "ICP_ITERATION": float(k)}) for k in range(n)])
        return np.zeros(n), kp, None  # (every pair carries its own threshold schedule)

    # ---------------------------------------------------------------- entry
    def on_lidar(self, stamp, xyz, t=None, intensity=None, forced=None):
        """forced: {name: xyz} of de-skewed layers as the device produced them for THIS scan (see _run_pass); the distance of
        each to the oracle's own is left in rec["deskew_ulps"].  Without it the oracle runs free."""
        self._intensity, self.forced = intensity, forced
        rec = super().on_lidar(stamp, xyz, t)
        rec["deskew_ulps"] = dict(self.deskew_ulps) if forced is not None and not rec["dropped"] else {}
        return rec

    @staticmethod
    def set_apart(rec):
        """Why a comparison of this scan against another implementation cannot be held to the decision level -- the rule of
        tools/fuzz_layers.py and no other: its nearest floating-point decision lies within 1e-9 (relative) of its threshold, or
        it solved normal equations of condition number above 1e10.  None when neither holds."""
        nd = lo.nearest_decision(list(rec.get("margins", [])) + list(rec.get("icp_margins", [])))
        if nd is not None and nd[1] <= 1e-9:
            return "decision %s within %.1e (relative) of its threshold" % nd
        if rec.get("max_cond", 0.0) > 1e10:
            return "normal equations of condition number %.1e" % rec["max_cond"]
        return None
