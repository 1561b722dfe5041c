"""development aid: random VALID general filter chains through the C++ driver and through oracle/chain_oracle.py, scan by scan
with the checks of oracle/chain_compare.py (decisions, layer sizes and contents, every map's counts and content, scalars, twist,
pose).  `fuzz_chains.py <cases> <seed> [oracle]`; prints `mismatches: N`.

Per case: 1-3 maps (plain or NDT, own voxel size / cap / far-voxel distance), 1-4 weighted layer pairs in one or two matchers,
a guaranteed well-populated pair (two decimations of the whole cloud into the first map) plus 2-6 random range / box (inside,
outside, both) / decimation (FirstPoint, ClosestToAverage, minimum_input_points_to_filter) / curvature / intensity steps reading
any earlier layer, a random FilterDeleteLayer, the de-skew first in the 1st pass, first in the 2nd pass (everything then filters
after it, and the twist hook re-runs it) or absent, either time-stamp method or none, now and then scans without time stamps;
thresholds drawn around the drive's point spacing, so layers are sometimes tiny or empty.  Each over a 4-6-scan slice of
synth.make_drive(14).  The YAML text goes through Config.FromYamlText and through the oracle's own loader.

A case whose oracle reports a decision within 1e-9 of its threshold or normal equations conditioned above 1e10 is set apart
(ChainOdometryOracle.set_apart, the rule of fuzz_layers.py): counted and printed; from 50 cases up more than 2 % of the cases
set apart fail the run (a shorter run cannot measure such a share: one case of 30 is 3.3 %).  `oracle` as third
argument runs the oracle alone (no device): the share of set-apart cases of a generator can be tuned on the CPU."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mola_lidar_odometry_amd import synth  # noqa: E402
from oracle import chain_compare, chain_oracle  # noqa: E402

n_cases = int(sys.argv[1]) if len(sys.argv) > 1 else 10
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 31)
ORACLE_ONLY = len(sys.argv) > 3 and sys.argv[3] == "oracle"
if not ORACLE_ONLY:
    from mola_lidar_odometry_amd import capi  # noqa: E402
    capi.lib()
    from mola_lidar_odometry_amd import _mp2p_icp_hip as host  # noqa: E402

PIPE = os.path.join(ROOT, "pipelines", "lidar3d-default-hip.yaml")
HEAD = open(PIPE).read().split("\nlocalmap_generator:")[0] + "\n"
_M0 = HEAD.index("    - class: mp2p_icp_hip::Matcher_Points_DistanceThreshold")
_M1 = HEAD.index("\n  quality:")
MATCHER = HEAD[_M0:_M1].rstrip("\n") + "\n"
ONE = '          - {global: "localmap", local: "decimated_for_icp", weight: 1.0}\n'
assert ONE in MATCHER and "threshold: '2.0*max(" in MATCHER
E = "ESTIMATED_SENSOR_MAX_RANGE"


def u(a, b):
    return float(rng.uniform(a, b))


def step(cls, **params):
    return "  - class_name: mp2p_icp_filters::%s\n    params:\n" % cls + "".join("      %s: %s\n" % kv for kv in params.items())


def q(name):
    return "'%s'" % name


def generate():
    intensity = bool(rng.integers(0, 2))
    ts = str(rng.choice(["none", "MiddleIsZero", "EarliestIsZero"]))
    mode = str(rng.choice(["first", "pass2", "none"]))
    passes = {1: "", 2: ""}
    if mode == "first":
        passes[1] += step("FilterDeskew", input_pointcloud_layer=q("raw"), output_pointcloud_layer=q("L0"), silently_ignore_no_timestamps="true")
        src, fp = "L0", 1
    elif mode == "pass2":
        passes[1] += step("FilterDecimateVoxels", input_pointcloud_layer=q("raw"), output_pointcloud_layer=q("pre"),
                          voxel_filter_resolution="%.3f" % u(0.15, 0.3), decimate_method="DecimateMethod::FirstPoint")
        passes[2] += step("FilterDeskew", input_pointcloud_layer=q("pre"), output_pointcloud_layer=q("L0"), silently_ignore_no_timestamps="true")
        src, fp = "L0", 2
    else:
        src, fp = "raw", 1
    # the well-populated pair: two decimations of the whole cloud
    passes[fp] += step("FilterDecimateVoxels", input_pointcloud_layer=q(src), output_pointcloud_layer=q("base_map"),
                       voxel_filter_resolution="%.3f*1e-2*%s" % (u(0.5, 1.0), E), decimate_method="DecimateMethod::FirstPoint")
    passes[fp] += step("FilterDecimateVoxels", input_pointcloud_layer=q("base_map"), output_pointcloud_layer=q("base_icp"),
                       voxel_filter_resolution="%.3f" % u(0.8, 1.6),
                       decimate_method="DecimateMethod::" + str(rng.choice(["FirstPoint", "ClosestToAverage"])))
    pool, extra, normalized = [src, "base_map"], [], set()
    for k in range(int(rng.integers(2, 7))):
        kind = str(rng.choice(["range", "box", "decimate", "curvature"] + (["normalize", "by_intensity"] if intensity else [])))
        inp = str(rng.choice(pool))
        if kind == "range":
            out = ["x%d" % k]
            passes[fp] += step("FilterByRange", input_pointcloud_layer=q(inp), output_layer_between=q(out[0]),
                               range_min="%.3f" % u(0.0, 5.0), range_max=str(rng.choice(["%.3f" % u(8.0, 60.0), "%.2f*%s" % (u(0.2, 1.2), E)])))
        elif kind == "box":
            which = int(rng.integers(0, 3))
            out = [n for n, on in (("x%di" % k, which != 1), ("x%do" % k, which != 0)) if on]
            p = dict(input_pointcloud_layer=q(inp))
            if which != 1:
                p["inside_pointcloud_layer"] = q(out[0])
            if which != 0:
                p["outside_pointcloud_layer"] = q(out[-1])
            p["bounding_box_min"] = "[%.2f, %.2f, %.2f]" % (-u(3, 25), -u(3, 25), -u(1, 5))
            p["bounding_box_max"] = "[%.2f, %.2f, %.2f]" % (u(3, 25), u(3, 25), u(0, 8))
            passes[fp] += step("FilterBoundingBox", **p)
        elif kind == "decimate":
            out = ["x%d" % k]
            passes[fp] += step("FilterDecimateVoxels", input_pointcloud_layer=q(inp), output_pointcloud_layer=q(out[0]),
                               voxel_filter_resolution="%.3f" % u(0.1, 3.0), minimum_input_points_to_filter=int(rng.choice([0, 0, 500, 5000])),
                               decimate_method="DecimateMethod::" + str(rng.choice(["FirstPoint", "ClosestToAverage"])))
        elif kind == "curvature":
            on = rng.integers(0, 2, 3)
            on[int(rng.integers(0, 3))] = 1
            out = ["x%d%s" % (k, s) for s, o in zip("lso", on) if o]
            p = dict(input_pointcloud_layer=q(inp))
            for key, s, o in zip(("output_layer_larger_curvature", "output_layer_smaller_curvature", "output_layer_other"), "lso", on):
                if o:
                    p[key] = q("x%d%s" % (k, s))
            passes[fp] += step("FilterCurvature", max_cosine="%.3f" % u(0.2, 0.8), min_clearance="%.3f" % u(0.01, 0.3),
                               max_gap="%.3f" % u(0.05, 2.0), **p)
        elif kind == "normalize":
            if fp != 1 or inp == "raw":  # (in place, 1st pass only; 'raw' feeds everything)
                continue
            passes[1] += step("FilterNormalizeIntensity", pointcloud_layer=q(inp), remember_intensity_range=str(rng.choice(["true", "false"])))
            normalized.add(inp)
            continue
        else:
            on = rng.integers(0, 2, 3)
            on[int(rng.integers(0, 3))] = 1
            out = ["x%d%s" % (k, s) for s, o in zip("lmh", on) if o]
            p = dict(input_pointcloud_layer=q(inp))
            for key, s, o in zip(("output_layer_low_intensity", "output_layer_mid_intensity", "output_layer_high_intensity"), "lmh", on):
                if o:
                    p[key] = q("x%d%s" % (k, s))
            passes[fp] += step("FilterByIntensity", low_threshold="%.3f" % u(0.05, 0.5), high_threshold="%.3f" % u(0.5, 1.0), **p)
        pool += out
        extra += out
    n_maps = int(rng.integers(1, 4))
    maps = ""
    for m in range(n_maps):
        ndt = rng.integers(0, 3) == 0
        maps += """  - class_name: mp2p_icp_filters::Generator
    params:
      target_layer: 'm%d'
      metric_map_definition:
        class: mola::%s
        creationOpts:
          voxel_size: %s
        insertOpts:
          max_points_per_voxel: %d
          min_distance_between_points: %s
          remove_voxels_farther_than: %s
%s""" % (m, "NDT" if ndt else "HashedVoxelPointCloud", str(rng.choice(["'$f{max(0.5, 0.01*%s)}'" % E, "%.2f" % u(0.4, 1.5)])),
         int(rng.choice([5, 10, 20])), "0.1" if ndt else "0", str(rng.choice(["'$f{max(100.0, 1.50*%s)}'" % E, "30.0", "0"])),
         "          max_eigen_ratio_for_planes: 0.05\n" if ndt else "")
    merges = [("base_map", 0)] + [(str(rng.choice(extra + ["base_map"])), m) for m in range(1, n_maps)]
    pairs = [(0, "base_icp", 1.0)] + [(int(rng.integers(0, n_maps)), str(rng.choice(extra)), float(rng.choice([0.25, 0.5, 1.0, 2.0])))
                                       for _ in range(int(rng.integers(0, 4)) if extra else 0)]
    used = {n for n, _ in merges} | {n for _, n, _ in pairs}
    gone = [n for n in ["raw", "pre", "L0"] + pool if n not in used and n in (["raw"] + (["pre"] if mode == "pass2" else []) + pool)
            and rng.integers(0, 2)]
    gone = sorted(set(gone))
    if gone:
        passes[2 if mode == "pass2" else 1] += step("FilterDeleteLayer", pointcloud_layer_to_remove="[%s]" % ", ".join(q(n) for n in gone))
    split = int(rng.integers(1, len(pairs) + 1))  # the first `split` entries in one matcher, the rest in a second
    entry = '          - {global: "m%d", local: "%s", weight: %s}\n'
    matchers = MATCHER.replace(ONE, "".join(entry % e for e in pairs[:split]))
    if split < len(pairs):
        matchers += MATCHER.replace(ONE, "".join(entry % e for e in pairs[split:])).replace("threshold: '2.0*max(", "threshold: '3.0*max(")
    text = HEAD[:_M0] + matchers + HEAD[_M1:] + "localmap_generator:\n" + maps
    if ts != "none":
        text += ("observations_filter_adjust_timestamps:\n" +
                 step("FilterAdjustTimestamps", pointcloud_layer=q("raw"), silently_ignore_no_timestamps="true", time_offset=0,
                      method=q("TimestampAdjustMethod::" + ts)))
    text += "observations_filter_1st_pass:\n" + passes[1]
    if passes[2]:
        text += "observations_filter_2nd_pass:\n" + passes[2]
    text += "insert_observation_into_local_map:\n" + "".join(
        step("FilterMerge", input_pointcloud_layer=q(n), target_layer=q("m%d" % m), input_layer_in_local_coordinates="true",
             robot_pose="[robot_x, robot_y, robot_z, robot_yaw, robot_pitch, robot_roll]") for n, m in merges)
    note = "deskew=%s ts=%s intensity=%d maps=%d pairs=%d/%d steps=%d" % (mode, ts, intensity, n_maps, len(pairs), 1 + (split < len(pairs)),
                                                                       passes[1].count("class_name") + passes[2].count("class_name"))
    return text, intensity, note


DRIVE = synth.make_drive(14)
INTENSITY = synth.drive_intensities(DRIVE)
bad, apart_cases = 0, 0
for case in range(n_cases):
    text, with_i, note = generate()
    n = int(rng.integers(4, 7))
    first = int(rng.integers(0, len(DRIVE["scans"]) - n + 1))
    bare = rng.integers(0, 8) == 0
    sl = slice(first, first + n)
    scans = [(xyz, None if bare else t) for xyz, t in DRIVE["scans"][sl]]
    inten = INTENSITY[sl] if with_i else None
    ok, why, apart = True, "", []
    try:
        o = chain_oracle.ChainOdometryOracle(text=text, n_threads=8)
        if ORACLE_ONLY:
            for k, ((xyz, t), st) in enumerate(zip(scans, DRIVE["stamps"][sl])):
                r = o.on_lidar(float(st), xyz, t, intensity=None if inten is None else inten[k])
                if o.set_apart(r):
                    apart.append((first + k, o.set_apart(r)))
                    break
        else:
            lo = host.LidarOdometry(0, True)
            lo.setIntensityInput(with_i)
            lo.initialize(host.Config.FromYamlText(text))
            _, apart = chain_compare.drive_against_oracle(lo, o, scans, DRIVE["stamps"][sl], inten, first=first)
    except AssertionError as e:
        ok, why = False, "scan, key, values: %s" % (str(e).splitlines()[0][:300],)
    except Exception as e:  # a chain one side refuses, or a failing call: a finding as well
        ok, why = False, "%s: %s" % (type(e).__name__, str(e)[:300])
    bad += 0 if ok else 1
    apart_cases += 1 if apart else 0
    print("case %3d scans %d-%d%s %s -> %s %s" % (case, first, first + n - 1, " (no time stamps)" if bare else "", note,
                                                 "ok" if ok and not apart else ("SET APART %s" % (apart,) if ok else "MISMATCH"), why), flush=True)
    if not ok:
        print("---- pipeline of case %d (from localmap_generator on)\n%s----" % (case, text[text.index("localmap_generator:"):]), flush=True)
share = apart_cases / max(1, n_cases)
print("cases set apart (near a threshold or ill-conditioned): %d of %d (%.1f %%; at most 2 %%)" % (apart_cases, n_cases, 100.0 * share))
print("mismatches:", bad)
sys.exit(1 if bad or (n_cases >= 50 and share > 0.02) else 0)
