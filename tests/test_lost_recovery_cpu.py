"""lost_recovery:, the parts that need no device: the options and what initialize() / setAlignBatcher refuse, the state machine
(mola_hip::LostRecovery through host.LostRecovery, one scan per call) on scripted sequences and on 200 random ones against the Python
fold of tests/lost_recovery_ref.py, and the condition of tests/test_gpu_lost_recovery.py: the reference alone loses the vehicle of
tests/lost_recovery_cases.py, skips the `near` attempt, fails two `keyframes` attempts between two key-frames and recovers with the
third."""
import os

import numpy as np
import pytest

import lost_recovery_cases as lc
import lost_recovery_ref as lrr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIPE = os.path.join(ROOT, "pipelines", "lidar3d-default-hip.yaml")
DEFAULTS = dict(enabled=False, bad_scans_to_lost=3, method="near_then_keyframes", near_sigma_xy=3.0, near_sigma_yaw_deg=15.0,
                retry_every_n_scans=5, max_attempts=0)
GENERATE = ("MOLA_GENERATE_SIMPLEMAP", "true")


@pytest.fixture(scope="module")
def host():
    from mola_lidar_odometry_amd import _mp2p_icp_hip as H
    return H


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for v in lc.ENV:
        monkeypatch.delenv(v, raising=False)


def _cfg(host, block=""):
    return host.Config.FromYamlText(open(PIPE).read() + block)


# ---- options ---------------------------------------------------------------------------------------------------------------------
def test_the_defaults_are_the_documented_ones(host):
    assert lrr.DEFAULTS == DEFAULTS
    assert host.lost_recovery_options(_cfg(host)) == DEFAULTS                          # absent
    assert host.lost_recovery_options(_cfg(host, "\nlost_recovery:\n")) == DEFAULTS    # empty
    assert host.lost_recovery_options(_cfg(host, lc.block(False))) == DEFAULTS
    text = lc.block(True, bad_scans_to_lost=2, method="keyframes", near_sigma_xy=1.5, near_sigma_yaw_deg=10, retry_every_n_scans=1, max_attempts=7)
    want = dict(enabled=True, bad_scans_to_lost=2, method="keyframes", near_sigma_xy=1.5, near_sigma_yaw_deg=10.0, retry_every_n_scans=1, max_attempts=7)
    assert host.lost_recovery_options(_cfg(host, text)) == want
    import yaml
    assert lrr.options(yaml.safe_load(text)) == want
    lo = host.LidarOdometry()
    lo.initialize(_cfg(host, lc.block(False, method="near", max_attempts=2)))
    assert lo.lostRecoveryOptions() == dict(DEFAULTS, method="near", max_attempts=2)
    assert not lo.isLost() and (lo.timesLost(), lo.recoveryAttempts(), lo.timesRecovered()) == (0, 0, 0)


@pytest.mark.parametrize("key,value", [("enabled", "maybe"), ("bad_scans_to_lost", 0), ("bad_scans_to_lost", 1.5), ("bad_scans_to_lost", -1),
                                       ("bad_scans_to_lost", "nan"), ("method", "gnss"), ("method", "Near"), ("near_sigma_xy", -1),
                                       ("near_sigma_xy", "inf"), ("near_sigma_xy", "wide"), ("near_sigma_yaw_deg", -0.5), ("near_sigma_yaw_deg", "nan"),
                                       ("retry_every_n_scans", 0), ("retry_every_n_scans", 2.5), ("max_attempts", -1), ("max_attempts", 0.5),
                                       ("max_attempts", "many")])
def test_a_bad_value_is_refused_by_its_key(host, key, value):
    text = "\nlost_recovery:\n  %s: %s\n" % (key, value)
    with pytest.raises(RuntimeError, match=r"^lost_recovery: %s\b" % key):
        host.lost_recovery_options(_cfg(host, text))
    with pytest.raises(RuntimeError, match=r"lost_recovery: %s\b" % key):   # ... by the driver too, enabled or not
        host.LidarOdometry().initialize(_cfg(host, text))


def test_the_option_dicts_of_the_other_blocks_are_unchanged(host):
    on = lc.block(True, method="near")
    for fn in ("loop_closure_options", "online_loop_closure_options", "session_join_options"):
        assert getattr(host, fn)(_cfg(host, on)) == getattr(host, fn)(_cfg(host)), fn
    a, b = host.LidarOdometry(), host.LidarOdometry()
    a.initialize(_cfg(host, on))
    b.initialize(_cfg(host))
    assert a.relocalizationOptions() == b.relocalizationOptions() and a.initialLocalization() == b.initialLocalization()
    assert a.simplemapOptions() == b.simplemapOptions()


# ---- what the driver refuses ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["keyframes", "near_then_keyframes"])
def test_a_method_that_needs_key_frames_is_refused_without_a_source_of_them(host, monkeypatch, method):
    with pytest.raises(RuntimeError, match=r"lost_recovery: method '%s' needs key-frames.*simplemap\.generate.*load_existing_simple_map" % method):
        host.LidarOdometry().initialize(_cfg(host, lc.block(True, method=method)))
    host.LidarOdometry().initialize(_cfg(host, lc.block(False, method=method)))   # a disabled block asks for nothing
    host.LidarOdometry().initialize(_cfg(host, lc.block(True, method="near")))    # near needs none
    monkeypatch.setenv(*GENERATE)
    monkeypatch.setenv("MOLA_SIMPLEMAP_OUTPUT", "")
    lo = host.LidarOdometry()
    lo.initialize(_cfg(host, lc.block(True, method=method)))                      # with the store: accepted, and without a device
    assert lo.lostRecoveryOptions()["enabled"] and not lo.isLost() and not lo.relocalizationPending()


def test_the_online_loop_closer_and_lost_recovery_exclude_each_other(host, monkeypatch):
    monkeypatch.setenv(*GENERATE)
    monkeypatch.setenv("MOLA_SIMPLEMAP_OUTPUT", "")
    online = "\nonline_loop_closure:\n  enabled: true\n"
    with pytest.raises(RuntimeError, match=r"lost_recovery: enabled together with online_loop_closure: enabled"):
        host.LidarOdometry().initialize(_cfg(host, online + lc.block(True)))
    host.LidarOdometry().initialize(_cfg(host, online + lc.block(False)))
    host.LidarOdometry().initialize(_cfg(host, "\nonline_loop_closure:\n  enabled: false\n" + lc.block(True)))


def test_set_align_batcher_is_refused_in_the_words_of_the_request(host):
    lo = host.LidarOdometry()
    lo.initialize(_cfg(host, lc.block(True, method="near")))
    with pytest.raises(RuntimeError, match=r"^LidarOdometry::setAlignBatcher: not available with lost_recovery: enabled: LidarOdometry::relocalizeInKeyFrames: "
                                           r"not available with an AlignBatcher \(the batch protocol has no slot for the extra alignments of one member\)"):
        lo.setAlignBatcher(host.AlignBatcher(2))
    off = host.LidarOdometry()
    off.initialize(_cfg(host, lc.block(False)))
    with pytest.raises(RuntimeError, match="process-wide default context"):   # (the older refusal: the block asks for nothing)
        off.setAlignBatcher(host.AlignBatcher(2))


def test_an_icp_block_without_a_point_matcher_is_refused_in_the_words_of_the_requests(host, monkeypatch):
    """what relocalizeNearPose / relocalizeInKeyFrames refuse of the plan, by their own check: the no-motion-model ICP block's only
    matcher a plane matcher (the pipeline of tests/test_loop_online_cpu.py), so that there is nothing to score candidates with"""
    text = open(PIPE).read()
    assert text.count("Matcher_Points_DistanceThreshold") == 1
    a, b = text.index("    - class: mp2p_icp_hip::Matcher_Points_DistanceThreshold"), text.index("  quality:")
    off = text[:a] + ("    - class: mp2p_icp_hip::Matcher_Point2Plane\n      params:\n        distanceThreshold: '1.0*ADAPTIVE_THRESHOLD_SIGMA'\n"
                      "        pointLayerMatches:\n          - {global: \"localmap\", local: \"decimated_for_icp\", weight: 1.0}\n\n") + text[b:]
    cfg = host.Config.FromYamlText
    lo = host.LidarOdometry()
    lo.initialize(cfg(off))                                            # the plan itself is fine ...
    none = r"the no-motion-model ICP block has no enabled Matcher_Points_DistanceThreshold to score candidates with"
    with pytest.raises(RuntimeError, match=r"^LidarOdometry::relocalizeInKeyFrames: " + none):   # ... and this is the request's refusal
        lo.relocalizeInKeyFrames()
    with pytest.raises(RuntimeError, match=r"lost_recovery: enabled, but LidarOdometry::relocalizeNearPose: " + none):
        host.LidarOdometry().initialize(cfg(off + lc.block(True, method="near")))
    host.LidarOdometry().initialize(cfg(off + lc.block(False, method="near")))               # a disabled block asks for nothing
    monkeypatch.setenv(*GENERATE)
    monkeypatch.setenv("MOLA_SIMPLEMAP_OUTPUT", "")
    for method in ("keyframes", "near_then_keyframes"):
        with pytest.raises(RuntimeError, match=r"lost_recovery: enabled, but LidarOdometry::relocalizeInKeyFrames: " + none):
            host.LidarOdometry().initialize(cfg(off + lc.block(True, method=method)))
        host.LidarOdometry().initialize(cfg(off + lc.block(False, method=method)))


# ---- the state machine on scripted sequences ---------------------------------------------------------------------------------------------
G, B, N = True, False, None   # a good alignment, a rejected one, none (the alignment did not run, or the scan restarted the map)


def _machine(host, **kw):
    return host.LostRecovery(_cfg(host, lc.block(True, **kw)))


def _run(m, script):
    """script: [(icp_good, outcome, caller_request, near_fits)] or shorter tuples / bare icp_good -> the dicts of m.scan"""
    out = []
    for s in script:
        s = s if isinstance(s, tuple) else (s,)
        s = s + (False, False, True)[len(s) - 1:]
        out.append(m.scan(s[0], s[1], s[2], s[3]))
    return out


def _col(recs, key):
    return [r[key] for r in recs]


@pytest.mark.parametrize("n", [1, 3])
def test_n_rejected_alignments_in_a_row_make_the_driver_lost(host, n):
    m = _machine(host, bad_scans_to_lost=n, method="keyframes")
    r = _run(m, [G, G] + [B] * n + [B])
    assert _col(r, "bad_streak") == [0, 0] + list(range(1, n + 2))
    assert _col(r, "lost") == [False] * (2 + n) + [True]           # the state the scan ARRIVED in
    assert _col(r, "placed") == [0] * (1 + n) + [2, 0]             # the scan that loses places the request ...
    assert _col(r, "recovery_attempt") == [0] * (2 + n) + [2]      # ... the next one serves it
    assert m.isLost() and m.timesLost() == 1 and m.recoveryAttempts() == 1 and m.timesRecovered() == 0


def test_a_good_scan_inside_a_bad_streak_resets_it_and_scans_without_an_alignment_stand_outside(host):
    m = _machine(host, bad_scans_to_lost=3, method="keyframes")
    r = _run(m, [B, B, G, B, B, N, N, B])
    assert _col(r, "bad_streak") == [1, 2, 0, 1, 2, 2, 2, 3]
    assert not any(_col(r, "lost")) and m.isLost() and _col(r, "placed") == [0] * 7 + [2]


@pytest.mark.parametrize("every", [1, 5])
def test_failed_attempts_are_cleared_and_come_every_n_scans(host, every):
    m = _machine(host, bad_scans_to_lost=1, method="keyframes", retry_every_n_scans=every)
    r = _run(m, [B] + [B] * (3 * every + 1))
    served = [k for k, x in enumerate(r) if x["recovery_attempt"]]
    assert served == [1 + every * j for j in range(4)][:len(served)] and len(served) >= 3
    assert all(x["recovery_attempt"] in (0, 2) and not x["recovery_succeeded"] for x in r)
    # a failed own request does not stay pending: between two attempts nothing waits
    for k, x in enumerate(r[1:], 1):
        assert x["pending"] == (x["placed"] != 0), (k, x)
    assert m.recoveryAttempts() == len(served) and m.isLost()


def test_near_then_keyframes_tries_near_once_per_loss(host):
    m = _machine(host, bad_scans_to_lost=1, retry_every_n_scans=1)
    r = _run(m, [B, B, B, (G, True), G, B, B, B])
    assert _col(r, "recovery_attempt") == [0, 1, 2, 2, 0, 0, 1, 2]
    assert _col(r, "recovery_succeeded") == [False, False, False, True, False, False, False, False]
    assert _col(r, "lost") == [False, True, True, True, False, False, True, True]
    assert (m.timesLost(), m.recoveryAttempts(), m.timesRecovered()) == (2, 5, 1)


def test_a_near_attempt_whose_grid_does_not_fit_is_skipped(host):
    m = _machine(host, bad_scans_to_lost=1, retry_every_n_scans=2)
    r = _run(m, [(B, False, False, False), (G, True)])
    assert _col(r, "placed") == [2, 0] and _col(r, "recovery_attempt") == [0, 2] and r[1]["recovery_succeeded"]
    assert (m.recoveryAttempts(), m.skipped(), m.timesRecovered()) == (1, 1, 1)        # a skip is no attempt
    m = _machine(host, bad_scans_to_lost=1, retry_every_n_scans=2, method="near", max_attempts=1)
    r = _run(m, [(B, False, False, False)] * 5 + [B, B])
    assert _col(r, "placed") == [0] * 6 + [1] and _col(r, "pending") == [False] * 6 + [True]   # looked at scans 0, 2, 4; fits at 6
    assert (m.recoveryAttempts(), m.skipped()) == (0, 3) and not m.gaveUp() and not any(_col(r, "recovery_gave_up"))
    # ... so max_attempts: 1 still buys one attempt with device work
    m = _machine(host, bad_scans_to_lost=1, retry_every_n_scans=1, max_attempts=1)
    r = _run(m, [(B, False, False, False), B, B, B])
    assert _col(r, "placed") == [2, 0, 0, 0] and _col(r, "recovery_attempt") == [0, 2, 0, 0] and _col(r, "recovery_gave_up") == [False, True, True, True]
    assert (m.recoveryAttempts(), m.skipped()) == (1, 1) and m.gaveUp()


def test_max_attempts_reached_the_driver_stays_lost_and_says_so(host):
    m = _machine(host, bad_scans_to_lost=1, method="keyframes", retry_every_n_scans=1, max_attempts=2)
    r = _run(m, [B] * 8)
    assert _col(r, "recovery_attempt") == [0, 2, 2, 0, 0, 0, 0, 0] and _col(r, "lost") == [False] + [True] * 7
    assert m.gaveUp() and m.isLost() and m.recoveryAttempts() == 2
    assert _col(r, "recovery_gave_up") == [False, False] + [True] * 6     # the records say so, from the scan of the last attempt on
    # a new loss counts from zero
    r = _run(m, [G, B, B, B, B])
    assert _col(r, "recovery_gave_up") == [False, False, False, True, True]
    assert not r[1]["lost"] and _col(r, "recovery_attempt") == [0, 0, 2, 2, 0] and m.recoveryAttempts() == 4 and m.timesLost() == 2


def test_a_callers_request_takes_precedence(host):
    m = _machine(host, bad_scans_to_lost=1, method="keyframes", retry_every_n_scans=1)
    # lost at scan 0 (own request placed); the caller places one before scan 1: it replaces the driver's, fails and stays pending, so
    # the driver places none; it succeeds at scan 3: TRACKING, and not as an attempt of the driver's
    r = _run(m, [B, (B, False, True), B, (G, True)])
    assert _col(r, "recovery_attempt") == [0, 0, 0, 0] and _col(r, "placed") == [2, 0, 0, 0] and _col(r, "pending") == [True, True, True, False]
    assert not r[3]["recovery_succeeded"] and r[3]["lost"] and not m.isLost()
    assert (m.timesLost(), m.recoveryAttempts(), m.timesRecovered()) == (1, 0, 1)
    # while TRACKING a caller's request is served as ever and touches nothing but the streak
    r = _run(m, [B, (G, True, True)])
    assert _col(r, "bad_streak") == [1, 0] and not m.isLost()


@pytest.mark.parametrize("n", [1, 3])
def test_n_good_alignments_in_a_row_are_tracking_again(host, n):
    m = _machine(host, bad_scans_to_lost=n, method="keyframes", retry_every_n_scans=50)
    r = _run(m, [B] * n + [B] + [G] * (n - 1) + [B] + [G] * n + [G])
    assert _col(r, "lost") == [False] * n + [True] * (2 * n + 1) + [False]
    assert (m.timesLost(), m.timesRecovered()) == (1, 1) and not m.isLost()


def test_reset_is_tracking_with_every_count_at_zero(host):
    m = _machine(host, bad_scans_to_lost=1, method="keyframes")
    _run(m, [B, B])
    assert m.isLost() and m.timesLost() == 1 and m.recoveryAttempts() == 1
    m.reset()
    assert not m.isLost() and (m.timesLost(), m.recoveryAttempts(), m.timesRecovered(), m.skipped()) == (0, 0, 0, 0)
    r = _run(m, [G, B])
    assert _col(r, "bad_streak") == [0, 1] and _col(r, "placed") == [0, 2]
    lo = host.LidarOdometry()
    lo.initialize(_cfg(host, lc.block(True, method="near")))
    lo.reset()
    assert not lo.isLost() and (lo.timesLost(), lo.recoveryAttempts(), lo.timesRecovered()) == (0, 0, 0)


def test_200_random_sequences_equal_the_python_fold(host):
    rng = np.random.Generator(np.random.PCG64(20260))
    methods = ["near", "keyframes", "near_then_keyframes"]
    for case in range(200):
        opt = dict(bad_scans_to_lost=int(rng.integers(1, 5)), method=methods[int(rng.integers(3))], retry_every_n_scans=int(rng.integers(1, 7)),
                   max_attempts=int(rng.integers(0, 4)))
        p_good = float(rng.choice([0.1, 0.5, 0.9]))
        script = [(None if rng.random() < 0.1 else bool(rng.random() < p_good), bool(rng.random() < 0.25), bool(rng.random() < 0.05),
                   bool(rng.random() < 0.8)) for _ in range(int(rng.integers(20, 80)))]
        m = _machine(host, **opt)
        got = _run(m, script)
        want, ref = lrr.fold(dict(opt, enabled=True), script)
        assert got == want, (case, opt, next(k for k in range(len(got)) if got[k] != want[k]))
        assert (m.isLost(), m.timesLost(), m.recoveryAttempts(), m.timesRecovered(), m.skipped(), m.gaveUp()) == \
               (ref.lost, ref.times_lost, ref.attempts, ref.times_recovered, ref.skipped, ref.gave_up()), (case, opt)


# ---- the scenario on the reference alone ---------------------------------------------------------------------------------------------------
def test_the_reference_alone_recovers(oracle):
    """no product code: tests/lost_recovery_ref.py on the kidnap of tests/lost_recovery_cases.py under the default block.
    Measured: rejected 0.652, 0.660, 0.655 -> LOST at scan 12; the near grid (107911 nodes) is skipped; keyframes attempts at scans 13
    (0.666) and 18 (0.669) fail, the one at scan 23 succeeds (0.998, key-frames [6, 8]); errors from there on <= 0.089 m."""
    d = lc.drive("kidnap")
    recs, o = lc.reference_run("kidnap", lc.block(True))
    cut = d["cut"]
    assert all(r["icp_good"] and not r["lost"] for r in recs[:cut])
    n = lrr.DEFAULTS["bad_scans_to_lost"]
    streak = recs[cut:cut + n]
    print("rejected qualities after the cut:", [round(r["goodness"], 3) for r in streak])
    assert all(r["icp_run"] and not r["icp_good"] for r in streak) and [r["bad_streak"] for r in streak] == list(range(1, n + 1))
    assert not recs[cut + n - 1]["lost"] and recs[cut + n]["lost"]
    attempts = [(k, r["recovery_attempt"], r["recovery_succeeded"], round(r["reloc_best_quality"], 3)) for k, r in enumerate(recs) if r["recovery_attempt"]]
    print("attempts (scan, kind, succeeded, quality):", attempts, "skipped:", o.m.skipped)
    assert o.m.skipped == 1 and all(kind == lrr.KEYFRAMES for _, kind, _, _ in attempts)           # near: skipped, not tried
    assert [ok for _, _, ok, _ in attempts] == [False] * (len(attempts) - 1) + [True] and len(attempts) >= 2
    won = attempts[-1][0]
    assert recs[won]["lost"] and not recs[won + 1]["lost"] and not o.m.lost
    assert (o.m.times_lost, o.m.attempts, o.m.times_recovered) == (1, len(attempts), 1)
    errs = [lc.position_error(r, d["poses"][k]) for k, r in enumerate(recs)]
    print("errors from the recovering scan on [m]: max %.3f, last %.3f" % (max(errs[won:]), errs[-1]))
    assert max(errs[won:]) < lc.GT_BOUND
    # nothing went into the map while LOST
    assert len({r["n_map_points"] for r in recs[cut - 1:won]}) == 1 and recs[won]["n_map_points"] > recs[won - 1]["n_map_points"]
    # without the block the vehicle stays lost
    off, _ = lc.reference_run("kidnap", "")
    assert not any(r["icp_good"] for r in off[cut:]) and lc.position_error(off[-1], d["poses"][-1]) > 10.0


def test_the_reference_alone_recovers_from_the_short_cut_with_a_near_attempt(oracle):
    """Measured: a 3 m cut, rejected 0.764, 0.753, 0.730; the near attempt (sigma 1.5 m / 10 deg: 20181 candidates) at scan 13 succeeds
    with 0.998; errors from there on <= 0.039 m."""
    d = lc.drive("short")
    recs, o = lc.reference_run("short", lc.NEAR_BLOCK)
    attempts = [(k, r["recovery_attempt"], r["recovery_succeeded"]) for k, r in enumerate(recs) if r["recovery_attempt"]]
    assert attempts == [(d["cut"] + 3, lrr.NEAR, True)] and o.m.skipped == 0
    assert max(lc.position_error(r, d["poses"][k]) for k, r in enumerate(recs) if k >= d["cut"] + 3) < lc.GT_BOUND
    off, _ = lc.reference_run("short", "")
    assert not any(r["icp_good"] for r in off[d["cut"]:])    # what the alignment alone does not bridge


def test_the_reference_alone_keeps_good_alignments_out_of_the_map_while_lost(oracle):
    """the glitch of tests/lost_recovery_cases.py: four foreign sweeps (0.649, 0.660, 0.656, 0.673) make the driver LOST, the caller's
    wrong request fails on every scan (75 candidates), scans 14 - 16 align (1.0, 1.0, 0.998) without entering the map -- 16 has a motion
    model and would have --, scan 17 is TRACKING and is merged; errors after the glitch <= 0.066 m."""
    d = lc.glitch_drive()
    recs, o = lc.glitch_reference_run()
    last = lc.GLITCH_AT[-1]
    assert [r["icp_good"] for r in recs[last - 3:last + 1]] == [False] * 4 and [r["lost"] for r in recs[last + 1:last + 6]] == [True] * 4 + [False]
    assert all(r["icp_good"] and not r["map_updated"] and not r["relocalized"] for r in recs[last + 1:last + 4])
    assert recs[last + 3]["had_motion_model"] and recs[last + 4]["map_updated"]
    assert len({r["n_map_points"] for r in recs[last:last + 4]}) == 1
    assert max(lc.position_error(r, d["poses"][k]) for k, r in enumerate(recs) if k > last) < lc.GT_BOUND
    assert (o.m.lost, o.m.times_lost, o.m.attempts, o.m.skipped, o.m.times_recovered) == (False, 1, 0, 1, 1) and o.request is not None
