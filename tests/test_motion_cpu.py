"""De-skew with gyroscope samples, the parts that need no device: the gyro_deskew: options and their refusals,
mola_hip::GyroBuffer and build_motion_table against the restatement of tests/motion_ref.py within 1e-12 (the entries of R are
bounded by 1, the chain has at most 64 fp64 products, the rates here stay below 10 rad/s), what the driver and the command line
refuse, the --gyro-file parser -- and the condition on the scenario of tests/motion_cases.py that the device tests rely on:
with the oracle alone, the drive's ATE with the gyro is at most half of the constant twist's (measured: 0.044 m against 0.245 m)."""
import os
import subprocess

import numpy as np
import pytest

import motion_cases as mc
import motion_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIPE = os.path.join(ROOT, "pipelines", "lidar3d-default-hip.yaml")
CLI = os.path.join(ROOT, "mola_lidar_odometry_amd", "molahip-lo-cli")
TOL = 1e-12


@pytest.fixture(scope="module")
def host():
    from mola_lidar_odometry_amd import _mp2p_icp_hip as H
    return H


# ---- options -------------------------------------------------------------------------------------------------------------------------
def test_the_defaults_are_the_restatement_s(host):
    assert dict(host.gyro_deskew_options(None)) == ref.DEFAULTS == dict(host.gyro_deskew_options("gyro_deskew:\n"))
    assert dict(host.gyro_deskew_options(host.Config.FromYamlText("other: 1\n"))) == ref.DEFAULTS
    lo = host.LidarOdometry()
    lo.initialize(host.Config.FromYamlFile(PIPE))
    assert dict(lo.gyroDeskewOptions()) == ref.DEFAULTS and lo.scansGyroDeskewed() == 0 and lo.gyroSamplesDropped() == 0


ROT_Z90 = [0.0, -1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0]


@pytest.mark.parametrize("key,text,value", [("enabled", "true", True), ("window", "[-0.1, 0.02]", [-0.1, 0.02]), ("segments", "1", 1),
                                            ("segments", "64", 64), ("max_gap", "0.004", 0.004), ("time_zero_offset", "-0.05", -0.05),
                                            ("gyro_bias", "[0.01, -0.02, 0.03]", [0.01, -0.02, 0.03]),
                                            ("sensor_rotation", str(ROT_Z90), ROT_Z90), ("buffer_seconds", "0.5", 0.5)])
def test_each_key_is_read(host, key, text, value):
    assert dict(host.gyro_deskew_options("gyro_deskew:\n  %s: %s\n" % (key, text))) == dict(ref.DEFAULTS, **{key: value})


@pytest.mark.parametrize("key,text", [("enabled", "maybe"), ("window", "[0.06, -0.06]"), ("window", "[0, 0]"), ("window", "[-0.06]"), ("window", "0.06"),
                                      ("window", "[nan, 1]"), ("window", "[-20, 20]"), ("segments", "0"), ("segments", "65"), ("segments", "2.5"),
                                      ("segments", "abc"), ("max_gap", "0"), ("max_gap", "inf"), ("time_zero_offset", "nan"),
                                      ("gyro_bias", "[0, 0]"), ("gyro_bias", "[0, 0, inf]"), ("sensor_rotation", "[1, 0, 0, 0, 1, 0, 0, 0]"),
                                      ("sensor_rotation", "[2, 0, 0, 0, 1, 0, 0, 0, 1]"), ("sensor_rotation", "[1, 0, 0, 0, 1, 0, 0, 0, -1]"),
                                      ("buffer_seconds", "0"), ("buffer_seconds", "0.05"), ("no_such_key", "1"), ("bias", "[0, 0, 0]")])
def test_a_bad_value_or_an_unknown_key_is_refused_by_name(host, key, text):
    with pytest.raises(RuntimeError, match=r"gyro_deskew: %s\b" % key):
        host.gyro_deskew_options("gyro_deskew:\n  %s: %s\n" % (key, text))
    with pytest.raises(RuntimeError, match=r"gyro_deskew: %s\b" % key):   # the driver reads the block whether enabled or not
        host.LidarOdometry().initialize(host.Config.FromYamlText(open(PIPE).read() + "\ngyro_deskew:\n  %s: %s\n" % (key, text)))


def test_what_the_driver_refuses_with_the_block(host):
    import rgbd_inline
    on = "\ngyro_deskew:\n  enabled: true\n"
    with pytest.raises(RuntimeError, match="gyro_deskew: enabled on a depth-image pipeline"):
        host.LidarOdometry().initialize(host.Config.FromYamlText(rgbd_inline.pipeline() + on))
    host.LidarOdometry().initialize(host.Config.FromYamlText(rgbd_inline.pipeline() + "\ngyro_deskew:\n  enabled: false\n"))
    lo = host.LidarOdometry()
    lo.initialize(host.Config.FromYamlText(open(PIPE).read() + on))
    with pytest.raises(RuntimeError, match="setAlignBatcher: not available with gyro_deskew: enabled is not available with an AlignBatcher"):
        lo.setAlignBatcher(host.AlignBatcher(2))


# ---- the buffer and the builder ------------------------------------------------------------------------------------------------------
def _rates(t, seed):
    rng = np.random.default_rng(seed)
    a, f, ph = rng.uniform(0.2, 3.0, (3, 3)), rng.uniform(0.5, 9.0, (3, 3)), rng.uniform(0, 6.28, (3, 3))
    return (a[None] * np.sin(2 * np.pi * f[None] * t[:, None, None] + ph[None])).sum(1)


def _both(host, t, w, stamp, opt, v=(1.0, -2.0, 0.5)):
    """(host table or None, restated table or None, host dropped, restated dropped)"""
    text = "gyro_deskew:\n" + "".join("  %s: %s\n" % (k, list(x) if isinstance(x, (list, tuple, np.ndarray)) else x) for k, x in opt.items())
    got = host.gyro_motion_table(np.asarray(t, np.float64), np.asarray(w, np.float64).reshape(-1, 3), float(stamp), text, list(v))
    buf = ref.GyroBufferRef(dict(ref.DEFAULTS, **opt)["buffer_seconds"])
    for tt, ww in zip(t, np.asarray(w, np.float64).reshape(-1, 3)):
        buf.push(tt, ww)
    want = ref.build_motion_table(buf, stamp, opt, v)
    assert got["kept"] == len(buf.t)
    return got["table"], want, got["dropped"], buf.dropped


def _same(got, want, what=""):
    assert (got is None) == (want is None), what
    if got is None:
        return
    for key in ("knots", "R", "w", "v"):
        a, b = np.asarray(got[key], np.float64), np.asarray(want[key], np.float64)
        assert a.shape == b.shape, (what, key)
        assert float(np.abs(a - b).max()) <= TOL, (what, key, float(np.abs(a - b).max()))
    R = np.asarray(got["R"])
    assert float(np.abs(R @ np.swapaxes(R, 1, 2) - np.eye(3)).max()) < 1e-13, what   # rotations, and the identity at t = 0:
    s0 = int(ref.segment_of(got["knots"], np.array([0.0]))[0])
    at0 = R[s0] @ ref.so3_exp(np.asarray(got["w"])[s0] * (0.0 - got["knots"][s0]))
    assert float(np.abs(at0 - np.eye(3)).max()) < 1e-13, what


@pytest.mark.parametrize("hz,max_gap", [(50.0, 0.025), (400.0, 0.02), (1000.0, 0.02)])
@pytest.mark.parametrize("window", [[-0.06, 0.06], [0.01, 0.11], [-0.11, -0.01], [-0.05, 0.0], [0.0, 0.05]])
@pytest.mark.parametrize("K", [1, 12, 64])
def test_the_builder_equals_the_restatement(host, hz, max_gap, window, K):
    stamp = 1234.5
    t = stamp - 0.3 + np.arange(int(0.6 * hz) + 1) / hz
    w = _rates(t - stamp, int(hz) + K)
    opt = dict(window=window, segments=K, max_gap=max_gap, gyro_bias=[0.01, -0.02, 0.005], sensor_rotation=ROT_Z90, time_zero_offset=-0.0123)
    got, want, _, _ = _both(host, t, w, stamp, opt)
    assert want is not None
    _same(got, want, "%g Hz %s K %d" % (hz, window, K))
    knots = np.asarray(got["knots"])
    assert knots[0] == window[0] and np.all(np.diff(knots) > 0) and len(knots) == K


def test_a_constant_rate_gives_the_constant_twist_s_table(host):
    w0 = np.array([0.3, -0.2, 1.1])
    t = 50.0 + np.arange(-100, 101) * 0.0025
    got, want, _, _ = _both(host, t, np.tile(w0, (len(t), 1)), 50.0, dict(segments=12))
    _same(got, want)
    R, ws = ref.constant_rate_table(got["knots"], w0)
    assert float(np.abs(np.asarray(got["R"]) - R).max()) < 1e-14 and float(np.abs(np.asarray(got["w"]) - ws).max()) < 1e-14


def test_samples_exactly_on_lo_and_hi_cover_the_window(host):
    stamp = 64.0                                                   # (binary fractions: the sample times are exact)
    lo, hi, step = -0.0625, 0.0625, 0.0078125
    t = stamp + lo + step * np.arange(17)
    assert t[0] - stamp == lo and t[-1] - stamp == hi
    w = _rates(t - stamp, 5)
    opt = dict(window=[lo, hi], segments=8)
    got, want, _, _ = _both(host, t, w, stamp, opt)
    assert got is not None
    _same(got, want, "on the ends")
    for cut, what in ((slice(1, None), "no sample at or before lo"), (slice(None, -1), "no sample at or after hi")):
        got, want, _, _ = _both(host, t[cut], w[cut], stamp, opt)
        assert got is None and want is None, what


def test_each_kind_of_coverage_failure_and_the_edge_of_max_gap(host):
    stamp = 10.0
    t = stamp + np.arange(-40, 41) * 0.0025
    w = _rates(t - stamp, 9)
    ok = lambda tt, ww, **o: _both(host, tt, ww, stamp, dict(o))[:2]
    got, want = ok(t, w)
    assert got is not None and want is not None
    assert ok(t[t > stamp - 0.0575], w[t > stamp - 0.0575]) == (None, None)          # starts after lo
    assert ok(t[t < stamp + 0.0575], w[t < stamp + 0.0575]) == (None, None)          # ends before hi
    assert ok(t[:0], w[:0]) == (None, None) and ok(t[:1], w[:1]) == (None, None)     # empty, one sample
    hole = (t < stamp - 0.01) | (t > stamp + 0.0125)                                 # a step of 0.025 s inside the window
    assert ok(t[hole], w[hole]) == (None, None)
    got, want = ok(t[hole], w[hole], max_gap=0.03)
    assert got is not None
    _same(got, want, "a wider max_gap bridges the hole")
    outside = (t < stamp - 0.1) | (t > stamp - 0.07)                                 # a hole before the window does not matter
    got, want = ok(t[outside], w[outside])
    assert got is not None
    _same(got, want, "hole outside")
    far = stamp + 5.0 + np.arange(0, 41) * 0.0025                                    # another time altogether
    assert ok(far, w[:41]) == (None, None)


def test_dropped_samples_are_counted_and_leave_the_table_alone(host):
    stamp = 10.0
    t = stamp + np.arange(-40, 41) * 0.0025
    w = _rates(t - stamp, 3)
    clean, want, d0, r0 = _both(host, t, w, stamp, {})
    assert d0 == r0 == 0
    tt, ww = list(t), [list(x) for x in w]
    for at, (bt, bw) in ((60, (t[59], [9.0, 9.0, 9.0])), (45, (t[20], [9.0, 9.0, 9.0])), (30, (np.nan, [0.0, 0.0, 0.0])),
                         (10, (t[9] + 0.001, [np.inf, 0.0, 0.0]))):          # a repeat, a step back, a NaN time, an infinite rate
        tt.insert(at, bt), ww.insert(at, bw)
    got, want2, d1, r1 = _both(host, np.array(tt), np.array(ww), stamp, {})
    assert d1 == r1 == 4
    _same(got, want2)
    for key in ("knots", "R", "w"):
        assert np.array_equal(np.asarray(got[key]), np.asarray(clean[key]))
    # the buffer forgets what is older than buffer_seconds
    long_t = stamp - 3.0 + np.arange(0, 1300) * 0.0025
    got = host.gyro_motion_table(long_t, np.zeros((len(long_t), 3)), stamp, "gyro_deskew:\n  buffer_seconds: 0.5\n")
    assert got["kept"] == 201 and got["dropped"] == 0 and got["table"] is not None


def test_two_hundred_random_cases(host):
    rng = np.random.default_rng(2024)
    n_tables = 0
    for case in range(200):
        hz = float(rng.choice([50.0, 100.0, 400.0, 1000.0]))
        stamp = float(rng.uniform(0.0, 2.0e5))
        lo = float(rng.uniform(-0.15, 0.05))
        hi = lo + float(rng.uniform(0.01, 0.15))
        K = int(rng.integers(1, 65))
        jitter = rng.uniform(-0.2, 0.2, 400) / hz
        t = stamp + float(rng.uniform(-0.3, -0.1)) + np.arange(400) / hz + jitter
        t = t[t < stamp + float(rng.uniform(0.0, 0.4))]
        if rng.uniform() < 0.3 and len(t) > 20:                      # a hole somewhere
            a = int(rng.integers(0, len(t) - 10))
            t = np.delete(t, slice(a, a + int(rng.integers(1, 10))))
        w = _rates(t - stamp, case)
        A = ref.so3_exp(rng.uniform(-1, 1, 3))
        opt = dict(window=[lo, hi], segments=K, max_gap=float(rng.choice([0.004, 0.02, 0.05])), time_zero_offset=float(rng.uniform(-0.02, 0.02)),
                   gyro_bias=[float(c) for c in rng.uniform(-0.05, 0.05, 3)], sensor_rotation=["%.17g" % c for c in A.reshape(9)], buffer_seconds=float(rng.choice([0.3, 2.0])))
        ref_opt = dict(opt, sensor_rotation=[float(c) for c in opt["sensor_rotation"]])
        text_opt = dict(opt, sensor_rotation="[" + ", ".join(opt["sensor_rotation"]) + "]")
        text = "gyro_deskew:\n" + "".join("  %s: %s\n" % (k, x if isinstance(x, str) else (list(x) if isinstance(x, list) else repr(x))) for k, x in text_opt.items())
        v = list(rng.uniform(-10, 10, 3))
        got = host.gyro_motion_table(t, w, stamp, text, v)
        buf = ref.GyroBufferRef(opt["buffer_seconds"])
        for tt, ww in zip(t, w):
            buf.push(tt, ww)
        want = ref.build_motion_table(buf, stamp, ref_opt, v)
        assert got["kept"] == len(buf.t) and got["dropped"] == buf.dropped, case
        _same(got["table"], want, "case %d" % case)
        n_tables += want is not None
    assert 40 < n_tables < 190, n_tables       # both outcomes are well represented


# ---- the command line ----------------------------------------------------------------------------------------------------------------
def test_the_gyro_file_parser(host):
    t, w = host.parse_gyro_text("# t wx wy wz\n10.0 0.1 0.2 0.3\n\n  10.0025\t-1e-3 0 2.5   # trailing\n#only a comment\n10.005 0 0 0")
    assert t.tolist() == [10.0, 10.0025, 10.005] and w.tolist() == [[0.1, 0.2, 0.3], [-1e-3, 0.0, 2.5], [0.0, 0.0, 0.0]]
    t, w = host.parse_gyro_text("")
    assert t.shape == (0,) and w.shape == (0, 3)
    for text, what in (("10.0 0.1 0.2\n", "line 1"), ("1 0 0 0\n2 0 0 0 0\n", "line 2"), ("1 0 0 0\n# c\n3 0 x 0\n", "line 3: 'x'"), ("1 0 0 nan\n", "line 1: 'nan'")):
        with pytest.raises(RuntimeError, match="gyro file: " + what):
            host.parse_gyro_text(text)


def test_the_cli_s_refusals(tmp_path):
    on, off = tmp_path / "on.yaml", tmp_path / "off.yaml"
    on.write_text(open(PIPE).read() + "\ngyro_deskew:\n  enabled: true\n")
    off.write_text(open(PIPE).read())
    good, bad = tmp_path / "gyro.txt", tmp_path / "bad.txt"
    good.write_text("# t wx wy wz\n0.0 0 0 0.1\n0.0025 0 0 0.1\n")
    bad.write_text("0.0 0 0 0.1\n0.0025 0 0\n")
    run = lambda *a: subprocess.run([CLI] + [str(x) for x in a], capture_output=True, text=True, timeout=60)
    r = run("--pipeline", on, "--seq-dir", "a", "--seq-dir", "b")
    assert r.returncode == 2 and "gyro_deskew: block is enabled: one sequence on one device only" in r.stderr
    r = run("--pipeline", on, "--seq-dir", "a", "--devices", "0,1")
    assert r.returncode == 2 and "gyro_deskew: block is enabled: one sequence on one device only" in r.stderr
    r = run("--pipeline", off, "--seq-dir", "a", "--seq-dir", "b", "--gyro-file", good)
    assert r.returncode == 2 and "--gyro-file: one sequence on one device only" in r.stderr
    r = run("--pipeline", off, "--seq-dir", "a", "--gyro-file", good)
    assert r.returncode == 2 and "--gyro-file needs the pipeline's gyro_deskew: block with enabled: true" in r.stderr
    r = run("--pipeline", on, "--seq-dir", "a", "--gyro-file", bad)
    assert r.returncode == 2 and "--gyro-file: gyro file: line 2" in r.stderr
    r = run("--pipeline", on, "--seq-dir", "a", "--gyro-file", tmp_path / "none.txt")
    assert r.returncode == 2 and "cannot open" in r.stderr and "none.txt" in r.stderr
    r = run("--pipeline", on, "--seq-dir", "a", "--gyro-file")
    assert r.returncode == 2 and "missing value for --gyro-file" in r.stderr
    # the usage names the option only where the run asks for the gyro de-skew: otherwise it is what it was
    assert "--gyro-file" not in run().stderr and "--gyro-file" not in run("--pipeline", off).stderr
    assert "--gyro-file FILE" in run("--pipeline", on).stderr and "--gyro-file FILE" in run("--gyro-file", good).stderr


# ---- the condition on the scenario ---------------------------------------------------------------------------------------------------
def test_the_scenario_makes_the_constant_twist_fail_visibly():
    """with the oracle alone: the gyro's ATE is at most half of the constant twist's (a condition on the inputs of
    tests/test_gpu_odometry_motion.py, not a measurement of the code under test)"""
    from oracle import odometry_oracle as oo
    d = mc.drive()
    assert len(d["scans"]) == mc.N_SCANS == 40 and all(len(x) == mc.RINGS * mc.AZIMUTHS == 5760 for x, _ in d["scans"])
    swing, flips = [], []   # inside every sweep the yaw rate swings by more than 1 rad/s, the pitch rate by more than 0.7 rad/s
    for st in d["stamps"]:
        w = d["gyro_w"][(d["gyro_t"] >= st - 0.05) & (d["gyro_t"] <= st + 0.05)]
        swing.append((np.ptp(w[:, 2]), np.ptp(w[:, 1])))
        flips.append((w[:, 2].min() < 0 < w[:, 2].max(), w[:, 1].min() < 0 < w[:, 1].max()))
    assert np.min(swing, axis=0)[0] > 1.0 and np.min(swing, axis=0)[1] > 0.7
    assert np.sum(flips, axis=0)[0] >= 25 and np.sum(flips, axis=0)[1] == mc.N_SCANS   # ... and changes sign inside most of them
    plain = oo.OdometryOracle(PIPE, n_threads=8)
    with_gyro = ref.MotionOracle(PIPE, n_threads=8, gyro_options=mc.GYRO_OPTIONS)
    g0 = 0
    for (xyz, t), st in zip(d["scans"], d["stamps"]):
        a, b = mc.gyro_until(d, st + 0.1, g0)
        for j in range(a, b):
            with_gyro.on_gyro(d["gyro_t"][j], d["gyro_w"][j])
        g0 = b
        plain.on_lidar(st, xyz, t)
        with_gyro.on_lidar(st, xyz, t)
    assert all(r["gyro_deskew"] for r in with_gyro.records)
    a, b = mc.ate(with_gyro.trajectory, d), mc.ate(plain.trajectory, d)
    print("ATE of the oracle: %.4f m with the gyro, %.4f m with the constant twist" % (a, b))
    assert len(with_gyro.trajectory) == len(plain.trajectory) == mc.N_SCANS
    assert a <= 0.5 * b, (a, b)
