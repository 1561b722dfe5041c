"""The odometry driver with the gyro_deskew: block (mola_lidar_odometry_hip/GyroDeskew.h) on the drive of tests/motion_cases.py --
a room, a sensor whose yaw and pitch rates swing inside every sweep, a 400 Hz gyro from the same formula -- scan by scan against
tests/motion_ref.MotionOracle (the CPU oracle's driver with its de-skew replaced by the two restated rules): the same decisions,
poses within 1e-6.  Then: its error against the ground truth is below the same driver's without the block; a gap cut into the
gyro stream falls back to the constant twist for those scans and is recorded; an absent or disabled block changes no byte; a
general plan whose FilterDeskew step is a Kind::Deskew of the driver (the dual-map chain) takes the table too.

The oracle's drives (a few seconds each) and the device's are made once per module and shared.  Measured (profiles/gyro_deskew.md):
ATE of the device driver 0.044 m with the block, 0.245 m without it."""
import os

import numpy as np
import pytest

import motion_cases as mc
import motion_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIPE = os.path.join(ROOT, "pipelines", "lidar3d-default-hip.yaml")
OFF = "\ngyro_deskew:\n  enabled: false\n  segments: 7\n"
GAP = (mc.T0 + 1.23, mc.T0 + 1.61)   # no samples in here: the windows of four sweeps hold a step above max_gap


@pytest.fixture(scope="module")
def host():
    from mola_lidar_odometry_amd import _mp2p_icp_hip as H
    return H


def _text(block, keyframes=False):
    text = open(PIPE).read()
    if keyframes:
        assert text.count("generate: ${MOLA_GENERATE_SIMPLEMAP|false}") == 1
        text = text.replace("generate: ${MOLA_GENERATE_SIMPLEMAP|false}", "generate: true").replace("${MOLA_SIMPLEMAP_OUTPUT|'final_map.simplemap'}", "''")
    return text + block


def _drive_through(on_gyro, on_lidar, gap=None, zero=0.0):
    """every scan after the samples a driver has received by the end of its sweep; samples inside `gap` never arrive"""
    d = mc.drive()
    g0 = 0
    for (xyz, t), st in zip(d["scans"], d["stamps"]):
        a, b = mc.gyro_until(d, st + 0.1, g0)
        for j in range(a, b):
            if gap is None or not (gap[0] <= d["gyro_t"][j] <= gap[1]):
                on_gyro(float(d["gyro_t"][j]), d["gyro_w"][j])
        g0 = b
        on_lidar(float(st), xyz, t)


def _oracle_run(gap=None):
    o = ref.MotionOracle(text=_text(mc.GYRO_BLOCK), n_threads=8, gyro_options=mc.GYRO_OPTIONS)
    _drive_through(o.on_gyro, o.on_lidar, gap)
    return o


def _device_run(host, text, gap=None):
    lo = host.LidarOdometry()
    lo.initialize(host.Config.FromYamlText(text))
    _drive_through(lambda t, w: lo.onGyro(t, [float(c) for c in w]), lo.onLidar, gap)
    return lo


@pytest.fixture(scope="module")
def oracle_full():
    return _oracle_run()


@pytest.fixture(scope="module")
def device_full(host):
    return _device_run(host, _text(mc.GYRO_BLOCK))


@pytest.fixture(scope="module")
def device_plain(host):
    return _device_run(host, _text(""))


def _follows(lo, o):
    recs = lo.records()
    assert len(recs) == len(o.records) == mc.N_SCANS
    worst_t = worst_r = 0.0
    for k, (a, b) in enumerate(zip(recs, o.records)):
        for key in ("dropped", "first_scan", "icp_run", "icp_good", "had_motion_model", "map_updated", "restarted", "icp_iterations",
                    "twist_corrections", "align_calls", "termination", "n_raw", "n_for_map", "n_for_icp", "n_map_points", "n_map_voxels",
                    "gyro_deskew", "gyro_segments"):
            assert a[key] == b[key], (k, key, a[key], b[key])
        np.testing.assert_allclose(a["twist"], b["twist"], rtol=0, atol=1e-6)
        Ta, Tb = np.array(a["pose"]).reshape(3, 4), b["pose"].reshape(3, 4)
        worst_t = max(worst_t, float(np.linalg.norm(Ta[:, 3] - Tb[:, 3])))
        worst_r = max(worst_r, float(np.linalg.norm(Ta[:, :3] - Tb[:, :3])))
    assert worst_t < 1e-6 and worst_r < 1e-6, (worst_t, worst_r)
    return recs


def test_the_driver_follows_the_restatement_scan_by_scan(device_full, oracle_full):
    recs = _follows(device_full, oracle_full)
    assert all(r["gyro_deskew"] and r["gyro_segments"] == 12 for r in recs)
    assert device_full.scansGyroDeskewed() == mc.N_SCANS and device_full.gyroSamplesDropped() == 0
    assert sum(r["twist_corrections"] for r in recs) > 0     # the twist hook re-ran the pass: a new v, the same rotations


def test_the_error_is_below_the_constant_twist_s(device_full, device_plain):
    d = mc.drive()
    with_gyro, without = mc.ate(device_full.trajectory(), d), mc.ate(device_plain.trajectory(), d)
    print("ATE against the ground truth: %.4f m with the gyro_deskew: block, %.4f m without it (ratio %.2f)" % (with_gyro, without, with_gyro / without))
    assert not any(r["gyro_deskew"] for r in device_plain.records()) and device_plain.scansGyroDeskewed() == 0
    assert with_gyro < without


def test_a_gap_in_the_stream_falls_back_and_is_recorded(host):
    o = _oracle_run(GAP)
    lo = _device_run(host, _text(mc.GYRO_BLOCK), GAP)
    recs = _follows(lo, o)
    fell_back = [k for k, r in enumerate(recs) if not r["gyro_deskew"]]
    d = mc.drive()
    # the step over the gap, from the last sample before it to the first after it, lies between the sample that starts a sweep's
    # interpolant and the one that ends it unless it ends at or before lo or starts at or after hi
    s_a, s_b = d["gyro_t"][d["gyro_t"] < GAP[0]].max(), d["gyro_t"][d["gyro_t"] > GAP[1]].min()
    want = [k for k, st in enumerate(d["stamps"]) if s_b > st + mc.TIME_ZERO - 0.06 and s_a < st + mc.TIME_ZERO + 0.06]
    assert fell_back == want and len(want) == 5, (fell_back, want)
    assert all(recs[k]["gyro_segments"] == 0 for k in fell_back)
    assert lo.scansGyroDeskewed() == mc.N_SCANS - len(fell_back)


def test_a_dropped_sample_is_counted(host):
    lo = host.LidarOdometry()
    lo.initialize(host.Config.FromYamlText(_text(mc.GYRO_BLOCK)))
    lo.onGyro(10.0, [0.0, 0.0, 0.1])
    lo.onGyro(10.0, [0.0, 0.0, 0.2])      # the time does not increase
    lo.onGyro(9.5, [0.0, 0.0, 0.3])
    lo.onGyro(10.1, [0.0, float("nan"), 0.0])
    lo.onGyro(10.2, [0.0, 0.0, 0.4])
    assert lo.gyroSamplesDropped() == 3
    off = host.LidarOdometry()
    off.initialize(host.Config.FromYamlText(_text(OFF)))
    off.onGyro(10.0, [0.0, 0.0, 0.1])
    off.onGyro(10.0, [0.0, 0.0, 0.1])
    assert off.gyroSamplesDropped() == 0  # a disabled block ignores the samples altogether


def test_an_absent_or_disabled_block_changes_nothing(host, tmp_path):
    runs = {}
    for name, block in (("absent", ""), ("disabled", OFF), ("enabled", mc.GYRO_BLOCK)):
        lo = _device_run(host, _text(block, keyframes=True))
        kf = tmp_path / (name + ".kf")
        lo.saveKeyFrames(str(kf))
        m = lo.downloadMap("localmap")
        recs = [{k: (v.tobytes() if isinstance(v, np.ndarray) else v) for k, v in r.items()} for r in lo.records()]
        runs[name] = dict(recs=recs, traj=[(t, tuple(np.asarray(p).reshape(-1))) for t, p in lo.trajectory()],
                          map={k: np.asarray(v).tobytes() for k, v in m.items()}, kf=kf.read_bytes(), n=lo.scansGyroDeskewed())
    a, b, e = runs["absent"], runs["disabled"], runs["enabled"]
    assert a["recs"] == b["recs"] and a["traj"] == b["traj"] and a["map"] == b["map"] and a["kf"] == b["kf"] and a["n"] == b["n"] == 0
    assert all(not r["gyro_deskew"] and r["gyro_segments"] == 0 for r in a["recs"])
    assert e["n"] == mc.N_SCANS and e["traj"] != a["traj"] and e["map"] != a["map"]


def test_a_general_plan_s_deskew_step_takes_the_table(host):
    """the dual-map chain (tests/test_odometry_chains.py): its FilterDeskew is a Kind::Deskew step of the driver's general plan, in
    the FIRST pass, on the raw stamps (the chain adjusts none: the zero of the stamps is the scan's own).  With optimize_twist
    off the record's twist is the one that step used, so the de-skewed layer can be held to the two restated rules directly."""
    import test_odometry_chains as chains
    d = mc.drive()
    head = chains.inline_pipeline(*chains.CHAINS["dual-map"]).replace("'${MOLA_OPTIMIZE_TWIST|true}'", "false")
    los = {}
    for name, block in (("gyro", "\ngyro_deskew:\n  enabled: true\n"), ("plain", "")):
        lo = host.LidarOdometry()
        lo.initialize(host.Config.FromYamlText(head + block))
        assert lo.describePipeline()["plan"] == "general"
        _drive_through(lambda t, w, lo=lo: lo.onGyro(t, [float(c) for c in w]), lo.onLidar)
        los[name] = lo
    recs = los["gyro"].records()
    assert all(r["gyro_deskew"] and r["gyro_segments"] == 12 for r in recs) and not any(r["gyro_deskew"] for r in los["plain"].records())
    assert all(r["twist_corrections"] == 0 for r in recs)
    # the last scan's de-skew, restated: the table of the samples received by then, the record's v
    raw, got = los["gyro"].downloadLayer("raw"), los["gyro"].downloadLayer("deskewed")
    buf = ref.GyroBufferRef()
    for t, w in zip(d["gyro_t"], d["gyro_w"]):
        if t <= d["stamps"][-1] + 0.1:
            buf.push(t, w)
    tab = ref.build_motion_table(buf, d["stamps"][-1], {}, recs[-1]["twist"][:3])
    want, _ = ref.deskew_motion(raw["xyz"], raw["t"], tab["knots"], tab["R"], tab["w"], tab["v"])
    assert len(raw["xyz"]) == len(got["xyz"]) == mc.RINGS * mc.AZIMUTHS
    err = np.abs(got["xyz"].astype(np.float64) - want)
    assert (err <= np.spacing(np.maximum(np.abs(want), 1e-3).astype(np.float32))).all(), float(err.max())
    assert np.array_equal(got["t"], raw["t"])
    assert float(np.abs(got["xyz"] - raw["xyz"]).max()) > 0.05   # (and it is no copy: the sweep was bent by decimetres)
    # poses against the ground truth at the scans' own stamps (this chain's zero)
    G = np.tile(np.eye(4), (mc.N_SCANS, 1, 1))
    R, p = mc.pose_at(mc.DT * np.arange(mc.N_SCANS))
    G[:, :3, :3], G[:, :3, 3] = R, p
    G = np.linalg.inv(G[0])[None] @ G

    def ate(lo):
        tr = lo.trajectory()
        idx = np.rint((np.array([t for t, _ in tr]) - mc.T0) / mc.DT).astype(int)
        E = np.array([np.asarray(q, np.float64).reshape(3, 4)[:, 3] for _, q in tr])
        return float(np.sqrt(np.mean(np.sum((E - G[idx, :3, 3]) ** 2, axis=1))))

    # (recorded, not asserted: the condition on the scenario -- tests/test_motion_cpu.py -- is held for the default plan only)
    print("dual-map chain: ATE %.4f m with the gyro_deskew: block, %.4f m without it" % (ate(los["gyro"]), ate(los["plain"])))
