"""The C++ driver's general plan held to oracle/chain_oracle.py scan by scan: what tests/test_odometry_chains.py,
tests/test_odometry_intensity.py and tools/fuzz_chains.py share.

TEST INFRASTRUCTURE.  Nothing here imports the host layer: `lo` is the pybind LidarOdometry object the caller made (onLidar,
records, downloadLayer, downloadMap, localMapStats), `o` a ChainOdometryOracle of the same pipeline text.

Equal per scan: the sixteen decision keys of tests/test_odometry.py::test_hip_driver_matches_oracle_driver (n_for_map / n_for_icp
in their general-plan meaning), layer_sizes, every live layer's src_idx, xyz, time stamps and intensity bit for bit, points /
voxels / voxel size of every map.  The oracle's own de-skewed layers within 1 float ulp of the device's (fp64 sin / cos differ
between libm and the device), after which the oracle continues from the device's.  goodness, sigma and both sensor ranges to
1e-9 relative, the twist to 1e-6 absolute, the pose to 1e-6.  After the last scan every map's content: vox_keys, vox_count and
src_idx equal, xyz within 1 float ulp (the two sides' key-frame poses differ by ~1e-10)."""
import numpy as np

from .chain_oracle import ulp_distance

DECISION_KEYS = ("dropped", "first_scan", "icp_run", "icp_good", "had_motion_model", "map_updated", "restarted", "icp_iterations",
                 "twist_corrections", "align_calls", "termination", "n_raw", "n_for_map", "n_for_icp", "n_map_points",
                 "n_map_voxels")
SCALAR_KEYS = ("goodness", "sigma", "estimated_sensor_max_range", "instantaneous_sensor_max_range")


def feed(lo, stamp, xyz, t, intensity):
    if intensity is None:
        return lo.onLidar(float(stamp), xyz, t)
    cols = [xyz, (np.zeros(len(xyz), np.float32) if t is None else t)[:, None], intensity[:, None]]
    return lo.onLidar(float(stamp), np.concatenate(cols, 1).astype(np.float32), None, [0, 1, 2], -1 if t is None else 3, 4)


def _same_floats(a, b):
    return np.array_equal(np.asarray(a, np.float32), np.asarray(b, np.float32), equal_nan=True)


def compare_scan(k, lo, a, o, b):
    """One scan: the driver `lo` with its record `a`, the chain oracle `o` with its record `b`.  Raises AssertionError naming the
    scan and the key (or layer / map and field) that differs."""
    for key in DECISION_KEYS:
        assert a[key] == b[key], (k, key, a[key], b[key])
    if b["dropped"]:
        return
    assert a["layer_sizes"] == b["layer_sizes"], (k, "layer_sizes", a["layer_sizes"], b["layer_sizes"])
    # the de-skewed layers: the oracle's own within 1 float ulp of the device's (the bar of test_gpu_preprocess.py::test_deskew);
    # everything else was derived from the device's de-skewed layer on both sides, so it is compared bit for bit
    for name, d in b["deskew_ulps"].items():
        assert d <= 1, (k, "de-skewed layer " + name, "ulps", d)
    for name, lay in o.layers.items():
        dev = lo.downloadLayer(name)
        assert dev["alive"], (k, name, "not alive on the device")
        n = len(lay["xyz"])
        assert len(dev["xyz"]) == n, (k, name, "size", len(dev["xyz"]), n)
        want_src = np.zeros(n, np.uint32) if lay["src_idx"] is None else lay["src_idx"]
        assert np.array_equal(dev["src_idx"], want_src), (k, name, "src_idx", int(np.sum(dev["src_idx"] != want_src)))
        assert _same_floats(dev["xyz"], lay["xyz"]), (k, name, "xyz", ulp_distance(dev["xyz"], lay["xyz"]))
        if lay["t"] is not None:
            assert _same_floats(dev["t"], lay["t"]), (k, name, "t")
        if lay["intensity"] is not None and n:
            assert dev["intensity"] is not None and _same_floats(dev["intensity"], lay["intensity"]), (k, name, "intensity")
    stats = lo.localMapStats()
    assert sorted(stats) == sorted(n for n, _ in o.map_defs), (k, "maps", sorted(stats))
    for name, _ in o.map_defs:
        want = b["maps"].get(name, (0, 0, 0.0))
        assert stats[name][:2] == want[:2], (k, "map " + name, "points, voxels", stats[name], want)
        assert abs(stats[name][2] - want[2]) <= 1e-9 * max(1.0, abs(want[2])) and np.float32(stats[name][2]) == np.float32(want[2]), \
            (k, "map " + name, "voxel size", stats[name][2], want[2])
    for key in SCALAR_KEYS:
        assert abs(a[key] - b[key]) <= 1e-9 * max(1.0, abs(b[key])), (k, key, a[key], b[key])
    np.testing.assert_allclose(a["twist"], b["twist"], rtol=0, atol=1e-6, err_msg="scan %d twist" % k)
    d = float(np.abs(np.array(a["pose"]) - b["pose"]).max())
    assert d < 1e-6, (k, "pose", d)


def compare_maps(k, lo, o):
    """Every map's content: the device's mh_map_download against the oracle map's dump().  vox_keys, vox_count and src_idx are
    demanded equal outright: the key-frame poses of the two sides differ by ~1e-10, so a point would have to lie that close to a
    voxel face to change voxel.  Should that ever happen it shows here as a plain mismatch, without evidence: whoever meets it
    checks the oracle map's float64 coordinate of the point against the face (within one float ulp = legitimate) by hand."""
    for name, _ in o.map_defs:
        dev = lo.downloadMap(name)
        if name not in o.maps:
            assert len(dev["xyz"]) == 0, (k, "map " + name, "exists on the device only")
            continue
        ref = o.maps[name]["map"].dump()
        for key in ("vox_keys", "vox_count", "src_idx"):
            assert np.array_equal(dev[key], ref[key]), (k, "map " + name, key)
        assert ulp_distance(dev["xyz"], ref["xyz"]) <= 1, (k, "map " + name, "xyz ulps", ulp_distance(dev["xyz"], ref["xyz"]))


def drive_against_oracle(lo, o, scans, stamps, intensity=None, first=0):
    """Feeds the scans to driver and oracle side by side and compares every scan (compare_scan), and every map's content after
    the last.  The oracle continues each scan's chain from the device's de-skewed layers (oracle/chain_oracle.py, `forced`).
    A scan whose nearest floating-point decision lies within 1e-9 of its threshold, or whose normal equations are conditioned
    above 1e10 (ChainOdometryOracle.set_apart: the rule of tools/fuzz_layers.py), ends the comparison of this drive: returned
    as [(scan, evidence)], and the callers here assert that list EMPTY for the committed drives.  Returns (records of both, apart)."""
    deskewed = [st["out"][0] for st in o.steps if st["kind"] == "deskew"]
    recs, apart = [], []
    for k, ((xyz, t), stamp) in enumerate(zip(scans, stamps)):
        it = None if intensity is None else intensity[k]
        a = feed(lo, stamp, xyz, t, it)
        forced = {} if a["dropped"] else {n: lo.downloadLayer(n)["xyz"] for n in deskewed}
        b = o.on_lidar(float(stamp), xyz, t, intensity=it, forced=forced)
        a = lo.records()[-1]  # (with the map counters of this scan)
        why = o.set_apart(b)
        if why is not None:
            print("scan %d set apart: %s" % (first + k, why))
            apart.append((first + k, why))
            break
        compare_scan(first + k, lo, a, o, b)
        recs.append((a, b))
    else:
        compare_maps(first + len(recs) - 1, lo, o)
    return recs, apart
