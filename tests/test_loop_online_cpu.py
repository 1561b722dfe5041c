"""Online loop closure, the parts that need no device: the online_loop_closure: options, what initialize() and setAlignBatcher refuse,
the per-frame candidate step (mola_hip::loop_candidates_step) folded over the frames against the loop form and tests/loop_ref.py,
the driver's pose rules and the motion model's rebase against tests/loop_online_ref.py, and the two conditions of
tests/test_gpu_loop_online.py: the reference closes the scenario of tests/loop_cases.py, and it closes a loop on the key-frames the
CPU oracle's driver records on the out-and-back drive."""
import os

import numpy as np
import pytest

import loop_cases as lc
import loop_online_ref as ol
import loop_ref as lr
import test_loop_cpu as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIPE = os.path.join(ROOT, "pipelines", "lidar3d-default-hip.yaml")
ENABLED = "\nonline_loop_closure:\n  enabled: true\n"
GENERATE = ("MOLA_GENERATE_SIMPLEMAP", "true")


@pytest.fixture(scope="module")
def host():
    from mola_lidar_odometry_amd import _mp2p_icp_hip as H
    return H


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for v in ol.ENV:
        monkeypatch.delenv(v, raising=False)


def _cfg(host, block=""):
    return host.Config.FromYamlText(open(PIPE).read() + block)


# ---- options ---------------------------------------------------------------------------------------------------------------------
def test_the_defaults_are_the_documented_ones(host):
    want = dict(enabled=False, correct_driver=True, check_every_n_keyframes=1)
    assert host.online_loop_closure_options(_cfg(host)) == want
    assert host.online_loop_closure_options(_cfg(host, "\nonline_loop_closure:\n")) == want
    got = host.online_loop_closure_options(_cfg(host, "\nonline_loop_closure:\n  enabled: true\n  correct_driver: false\n  check_every_n_keyframes: 3\n"))
    assert got == dict(enabled=True, correct_driver=False, check_every_n_keyframes=3)


@pytest.mark.parametrize("key,value", [("check_every_n_keyframes", 0), ("check_every_n_keyframes", -2), ("check_every_n_keyframes", 1.5),
                                       ("check_every_n_keyframes", "nan"), ("enabled", "maybe"), ("correct_driver", 2)])
def test_a_value_out_of_range_is_refused_by_name(host, key, value):
    with pytest.raises(RuntimeError, match=r"online_loop_closure: %s\b" % key):
        host.online_loop_closure_options(_cfg(host, "\nonline_loop_closure:\n  %s: %s\n" % (key, value)))
    with pytest.raises(RuntimeError, match=r"online_loop_closure: %s\b" % key):   # ... by the driver too, enabled or not
        host.LidarOdometry().initialize(_cfg(host, "\nonline_loop_closure:\n  %s: %s\n" % (key, value)))


def test_the_loop_closure_block_s_dict_is_the_pinned_one_beside_the_new_block(host):
    want = dict(min_travel=30.0, gate_base=5.0, gate_rate=0.02, max_place_dist=0, top_k=1, min_travel_between_closures=10.0, submap_radius=15.0,
                sigma_xy=1.5, sigma_yaw_deg=2.0, sigma=2.0, min_quality=0.9, odometry_sigma_xyz=0.02, odometry_sigma_rot_deg=0.05,
                loop_sigma_xyz=0.05, loop_sigma_rot_deg=0.1, max_iterations=50, min_step=1e-9)
    assert host.loop_closure_options(_cfg(host, ENABLED + "  check_every_n_keyframes: 4\n")) == want
    assert host.loop_closure_options(_cfg(host, "\nloop_closure:\n  top_k: 2\n" + ENABLED)) == dict(want, top_k=2)


def test_a_loop_closure_block_out_of_range_stops_the_driver_only_with_the_online_block(host, monkeypatch):
    bad = "\nloop_closure:\n  top_k: 0\n"
    host.LidarOdometry().initialize(_cfg(host, bad))                                                   # as before: only close_loops reads it
    host.LidarOdometry().initialize(_cfg(host, bad + "\nonline_loop_closure:\n  enabled: false\n"))
    monkeypatch.setenv(*GENERATE)
    monkeypatch.setenv("MOLA_SIMPLEMAP_OUTPUT", "")
    with pytest.raises(RuntimeError, match=r"loop_closure: top_k\b"):
        host.LidarOdometry().initialize(_cfg(host, bad + ENABLED))


# ---- what the driver refuses ----------------------------------------------------------------------------------------------------------
def test_initialize_demands_the_key_frame_store(host, monkeypatch):
    with pytest.raises(RuntimeError, match=r"online_loop_closure: enabled needs params\.simplemap\.generate"):
        host.LidarOdometry().initialize(_cfg(host, ENABLED))
    monkeypatch.setenv(*GENERATE)
    monkeypatch.setenv("MOLA_SIMPLEMAP_OUTPUT", "")
    lo = host.LidarOdometry()
    lo.initialize(_cfg(host, ENABLED))          # with the store: accepted, and without a device
    assert lo.loopCloser() is None and lo.rawKeyFrames()["frames"] == [] and lo.correctedTrajectory() == []
    lo = host.LidarOdometry()
    lo.initialize(_cfg(host, "\nonline_loop_closure:\n  enabled: false\n"))   # a disabled block asks for nothing
    monkeypatch.delenv("MOLA_GENERATE_SIMPLEMAP")
    host.LidarOdometry().initialize(_cfg(host, "\nonline_loop_closure:\n  enabled: false\n"))


def test_initialize_refuses_an_occupancy_map_plan(host):
    import lidar2d_inline
    text = lidar2d_inline.pipeline()          # the lidar2d-shaped pipeline with its CVoxelMap
    assert text.startswith("params:\n") and "CVoxelMap" in text and "simplemap:" not in text
    text = text.replace("params:\n", "params:\n  simplemap:\n    generate: true\n    save_final_map_to_file: ''\n", 1)
    host.LidarOdometry().initialize(host.Config.FromYamlText(text))          # the plan itself is fine
    with pytest.raises(RuntimeError, match=r"online_loop_closure: local map '\w+' is a 'CVoxelMap'"):
        host.LidarOdometry().initialize(host.Config.FromYamlText(text + ENABLED))


def test_initialize_refuses_an_icp_block_without_an_enabled_point_matcher(host, monkeypatch):
    monkeypatch.setenv(*GENERATE)
    monkeypatch.setenv("MOLA_SIMPLEMAP_OUTPUT", "")
    text = open(PIPE).read()
    assert text.count("Matcher_Points_DistanceThreshold") == 1
    # the block's only matcher a plane matcher: it names the plan's map, but there is no point matcher to score candidates with
    a, b = text.index("    - class: mp2p_icp_hip::Matcher_Points_DistanceThreshold"), text.index("  quality:")
    off = text[:a] + ("    - class: mp2p_icp_hip::Matcher_Point2Plane\n      params:\n        distanceThreshold: '1.0*ADAPTIVE_THRESHOLD_SIGMA'\n"
                      "        pointLayerMatches:\n          - {global: \"localmap\", local: \"decimated_for_icp\", weight: 1.0}\n\n") + text[b:]
    host.LidarOdometry().initialize(host.Config.FromYamlText(off))            # the plan itself is fine
    with pytest.raises(RuntimeError, match="online_loop_closure: the ICP block has no enabled Matcher_Points_DistanceThreshold"):
        host.LidarOdometry().initialize(host.Config.FromYamlText(off + ENABLED))
    other = text.replace("global: 'localmap'", "global: 'elsewhere'").replace("global: \"localmap\"", "global: \"elsewhere\"").replace("global: localmap", "global: elsewhere")
    assert other != text   # a global layer that is no local map of the plan
    with pytest.raises(RuntimeError, match="online_loop_closure: the ICP block matches against the global layer 'elsewhere'"):
        host.LidarOdometry().initialize(host.Config.FromYamlText(other + ENABLED))


def test_set_align_batcher_throws_on_an_enabled_instance(host, monkeypatch):
    monkeypatch.setenv(*GENERATE)
    monkeypatch.setenv("MOLA_SIMPLEMAP_OUTPUT", "")
    lo = host.LidarOdometry()
    lo.initialize(_cfg(host, ENABLED))
    with pytest.raises(RuntimeError, match=r"setAlignBatcher: not available with online_loop_closure: enabled .*AlignBatcher"):
        lo.setAlignBatcher(host.AlignBatcher(2))   # (the refusal of this feature, not the older one of a shared device context)
    plain = host.LidarOdometry()
    plain.initialize(_cfg(host))
    with pytest.raises(RuntimeError, match="process-wide default context"):
        plain.setAlignBatcher(host.AlignBatcher(2))


# ---- the candidate step, folded -----------------------------------------------------------------------------------------------------------
class _Folded:
    """the host module with loop_candidates replaced by the fold of loop_candidates_step: the tests of tests/test_loop_cpu.py then
    hold the step to the reference, with their own cases, seeds and accept callbacks"""

    def __init__(self, host):
        self._host = host
        self.calls = 0

    def __getattr__(self, name):
        return getattr(self._host, name)

    def loop_candidates(self, poses, has_points, matches, options=None, accept=None):
        self.calls += 1
        for m in matches:
            for f, _, _ in m:
                if f >= len(has_points):
                    raise RuntimeError("a match names frame %d of %d" % (f, len(has_points)))
        return ol.fold_candidates(self._host.loop_candidates_step, poses, has_points, matches, options or {}, accept)


def test_the_fold_is_the_loop_form_on_the_scenario(host):
    f = _Folded(host)
    tc.test_the_scenario_s_candidates_are_the_reference_s(f)
    assert f.calls == 4
    s = lc.scenario()
    has = [True] * len(s["est"])
    matches = lr.match_lists(s["sweeps"], has)
    opt = host.loop_closure_options(_cfg(host, lc.OPTIONS))
    for accept in (None, lambda i, j, shift, dist: False, lambda i, j, shift, dist: i % 2 == 0):
        assert ol.fold_candidates(host.loop_candidates_step, s["est"], has, matches, opt, accept) == [tuple(p) for p in host.loop_candidates(s["est"], has, matches, opt, accept)]
    # a growing database gives frame i the matches among the frames < i only: the same pairs
    causal = [[m for m in matches[i] if m[0] < i] for i in range(len(matches))]
    assert ol.fold_candidates(host.loop_candidates_step, s["est"], has, causal, opt) == [(56, 1) + p[2:] for p in host.loop_candidates(s["est"], has, matches, opt)][:1] + \
        [tuple(p) for p in host.loop_candidates(s["est"], has, matches, opt)][1:]


def test_the_fold_is_the_loop_form_on_the_random_cases(host):
    f = _Folded(host)
    tc.test_random_cases_equal_the_reference_exactly(f)      # the 200 cases of that test, its seeds, its accept callbacks
    assert f.calls == 200
    tc.test_the_travel_rule_and_the_gate_are_closed(f)
    tc.test_a_frame_without_points_is_never_a_partner_but_counts_in_the_path(f)


def test_the_step_carries_its_state(host):
    poses = np.array([tc._pose(0, 0), tc._pose(0, 12), tc._pose(0.5, 0), tc._pose(1, 0), tc._pose(1.5, 0)])   # s = 0, 12, 24.01, 24.51, 25.01
    opt = dict(min_travel=20.0, gate_base=2.0, gate_rate=0.0, min_travel_between_closures=0.8)
    m = [(0, 3, 10)]
    got, accepted, state = host.loop_candidates_step(poses[:3], [True] * 3, m, opt)
    assert got == [(2, 0, 3, 10)] and accepted and state[0] and abs(state[1] - lr.path_lengths(poses)[2]) == 0.0
    got, accepted, state2 = host.loop_candidates_step(poses[:4], [True] * 4, m, opt, state)      # 0.5 m after the closure: skipped
    assert got == [] and not accepted and state2 == state
    got, accepted, state3 = host.loop_candidates_step(poses[:5], [True] * 5, m, opt, state)      # 1.0 m after it: tried again
    assert got == [(4, 0, 3, 10)] and accepted and state3[1] == lr.path_lengths(poses)[4]
    got, accepted, state4 = host.loop_candidates_step(poses[:5], [True] * 5, m, opt, None, lambda i, j, shift, dist: False)
    assert got == [(4, 0, 3, 10)] and not accepted and state4 == (False, 0.0)


# ---- pose algebra -----------------------------------------------------------------------------------------------------------------------
def _random_pose(rng, spread=30.0):
    T = np.eye(4)
    T[:3, :3] = lc.exp_so3(rng.normal(0, 0.7, 3))
    T[:3, 3] = rng.normal(0, spread, 3)
    return lc.to12(T)


def test_the_pose_rules_are_the_numpy_ones(host):
    rng = np.random.default_rng(7)
    worst = 0.0
    for _ in range(50):
        R, P, S, C = (_random_pose(rng) for _ in range(4))
        for got, want in ((host.loop_raw_pose(list(R), list(P), list(S)), ol.raw_pose(R, P, S)),
                          (host.loop_correction(list(C), list(P)), ol.correction(C, P)),
                          (host.trajectory_anchor(list(P), list(S)), ol.anchor(P, S)),
                          (host.trajectory_corrected(list(C), list(host.trajectory_anchor(list(P), list(S)))), ol.compose(C, ol.anchor(P, S)))):
            worst = max(worst, float(np.abs(np.array(got) - want).max()))
        # delta (+) P = C, and an uncorrected store (S == raw) leaves the chain where the scans put it
        worst = max(worst, float(np.abs(ol.compose(host.loop_correction(list(C), list(P)), P) - C).max()),
                    float(np.abs(np.array(host.loop_raw_pose(list(S), list(P), list(S))) - P).max()))
    print("worst difference", worst)
    assert worst < 1e-12 * 30.0 * 4   # 1e-12 relative to the translations composed (some 30 m, up to three compositions)


def test_the_raw_chain_undoes_a_correction_of_the_store(host):
    """a store whose poses were moved by delta between two frames: the raw chain goes on as if nothing had happened"""
    rng = np.random.default_rng(8)
    steps = [lc.to12(np.vstack([np.hstack([lc.exp_so3(rng.normal(0, 0.05, 3)), rng.normal(0, 2.0, (3, 1))]), [0, 0, 0, 1]])) for _ in range(12)]
    truth = [np.array(tc._pose(0, 0), np.float64)]
    for d in steps:
        truth.append(ol.compose(truth[-1], d))
    raw, store, frame = [truth[0]], [truth[0]], np.array(tc._pose(0, 0), np.float64)   # frame: what the corrections have done to the map frame so far
    for k in range(1, len(truth)):
        P = ol.compose(store[-1], steps[k - 1])          # the scan is registered against the (corrected) map
        raw.append(np.array(host.loop_raw_pose(list(raw[-1]), list(P), list(store[-1]))))
        store.append(P)
        if k % 4 == 0:                                   # a closure: every stored pose moves
            delta = _random_pose(rng, 3.0)
            store = [ol.compose(delta, s) for s in store]
    assert float(np.abs(np.array(raw) - np.array(truth)).max()) < 1e-11


def test_rebase_left_composes_the_pose_and_keeps_the_twist(host):
    rng = np.random.default_rng(9)
    a, b, delta = _random_pose(rng), None, _random_pose(rng, 5.0)
    step = lc.to12(np.vstack([np.hstack([lc.exp_so3([0.0, 0.01, 0.03]), [[0.8], [0.02], [0.0]]]), [0, 0, 0, 1]]))
    b = ol.compose(a, step)
    plain, moved = host.NavStateFuse(), host.NavStateFuse()
    for n in (plain, moved):
        n.fuse_pose(10.0, list(a))
        n.fuse_pose(10.1, list(b))
    moved.rebase(list(delta))
    (p0, tw0), (p1, tw1) = plain.estimated_navstate(10.2), moved.estimated_navstate(10.2)
    assert tw0 == tw1                                                        # the vehicle-frame twist, bit for bit
    assert float(np.abs(np.array(p1) - ol.compose(delta, p0)).max()) < 1e-12 * 30.0
    assert host.NavStateFuse().estimated_navstate(1.0) is None
    empty = host.NavStateFuse()
    empty.rebase(list(delta))                                                # nothing fused yet: nothing to move
    assert empty.estimated_navstate(1.0) is None
    # the next increment is measured in the moved frame: fusing delta (+) c gives the twist that fusing c gives without the rebase
    c = ol.compose(b, step)
    plain.fuse_pose(10.2, list(c))
    moved.fuse_pose(10.2, list(ol.compose(delta, c)))
    assert float(np.abs(np.array(plain.estimated_navstate(10.3)[1]) - np.array(moved.estimated_navstate(10.3)[1])).max()) < 1e-9


def test_the_corrected_trajectory_rule(host):
    rng = np.random.default_rng(10)
    store = [_random_pose(rng) for _ in range(4)]
    entries, anchors, rels = [], [], []
    for n in range(10):
        P = _random_pose(rng)
        a = -1 if n < 2 else min(3, (n - 2) // 2)
        entries.append((100.0 + n, P))
        anchors.append(a)
        rels.append(None if a < 0 else np.array(host.trajectory_anchor(list(P), list(store[a]))))
    # nothing corrected: the entries come back within rounding; corrected poses: every entry follows its frame
    same = ol.corrected_trajectory(entries, anchors, rels, np.array(store))
    assert max(float(np.abs(p - q).max()) for (_, p), (_, q) in zip(same, entries)) < 1e-12 * 30.0 * 4
    C = np.array([ol.compose(_random_pose(rng, 2.0), s) for s in store])
    moved = ol.corrected_trajectory(entries, anchors, rels, C)
    for (t, p), (t0, p0), a, rel in zip(moved, entries, anchors, rels):
        assert t == t0
        if a < 0:
            assert np.array_equal(p, p0)
        else:
            assert float(np.abs(np.array(host.trajectory_corrected(list(C[a]), list(rel))) - p).max()) < 1e-12 * 30.0 * 4
            # the entry keeps its place relative to its frame
            assert float(np.abs(ol.anchor(p, C[a]) - ol.anchor(p0, store[a])).max()) < 1e-11


# ---- the conditions of the device tests ------------------------------------------------------------------------------------------------------
def test_the_reference_still_closes_the_scenario_s_four_pairs(oracle):
    ref = lr.scenario_reference(open(PIPE).read() + lc.OPTIONS)
    assert [(p["i"], p["j"], p["accepted"]) for p in ref["pairs"]] == [(56, 1, True), (59, 2, True), (62, 5, True), (65, 8, True)]


def test_the_reference_closes_a_loop_on_the_oracle_s_key_frames_of_the_drive(oracle):
    """the out-and-back drive of tests/loop_online_ref.py as the CPU oracle's driver records it: tests/loop_ref.py accepts a pair"""
    kf = ol.oracle_keyframes()
    recs = [r for r in kf["records"] if not r["dropped"]]
    assert len(recs) == ol.N_SCANS <= 150 and all(r["icp_good"] for r in recs if r["icp_run"])
    ref = ol.oracle_reference()
    print("key-frames", len(kf["frames"]), "pairs", [(p["i"], p["j"], p["shift"], p["dist"], round(p["quality"], 4), p["accepted"]) for p in ref["pairs"]])
    assert sum(p["accepted"] for p in ref["pairs"]) >= 1
    for p in ref["pairs"]:
        if p["accepted"]:   # a revisit indeed: the two frames stand within the gate of each other on the ground truth's street
            assert abs(kf["frames"][p["i"]]["pose"][3] - kf["frames"][p["j"]]["pose"][3]) < 6.0
