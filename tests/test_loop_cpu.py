"""Loop closure, the parts that need no device: the loop_closure: options, the candidate rule (mola_hip::loop_candidates) against
tests/loop_ref.py, the pose-graph optimiser (mola_hip::optimize_pose_graph) against the reference's dense Gauss-Newton, the
corrected key-frame file, and the reference alone on the scenario of tests/loop_cases.py -- a condition on the scenario: its
revisits must be found, verified and closed by the restatement before the device is held to it (tests/test_gpu_loop.py).

Measured here: the reference tries (56, 1), (59, 2), (62, 5), (65, 8), accepts all four at quality 0.988-0.994 with edges 0.027-
0.052 m from the truth; the end-position error goes from 3.29 m to 0.23 m, the maximum over the frames from 4.13 m to 0.78 m."""
import os
import time

import numpy as np
import pytest

import loop_cases as lc
import loop_ref as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIPE = os.path.join(ROOT, "pipelines", "lidar3d-default-hip.yaml")
PIPE_NDT = os.path.join(ROOT, "pipelines", "lidar3d-ndt-hip.yaml")
EDGE_BOUND, END_BOUND, MAX_BOUND = 0.1, 0.6, 1.0   # [m] against the ground truth: every accepted edge, the last frame, every frame


@pytest.fixture(scope="module")
def host():
    from mola_lidar_odometry_amd import _mp2p_icp_hip as H
    return H


def _cfg(host, block=""):
    return host.Config.FromYamlText(open(PIPE).read() + block)


# ---- options ---------------------------------------------------------------------------------------------------------------------
def test_the_defaults_are_the_documented_ones(host):
    want = dict(min_travel=30.0, gate_base=5.0, gate_rate=0.02, max_place_dist=0, top_k=1, min_travel_between_closures=10.0, submap_radius=15.0,
                sigma_xy=1.5, sigma_yaw_deg=2.0, sigma=2.0, min_quality=0.9, odometry_sigma_xyz=0.02, odometry_sigma_rot_deg=0.05,
                loop_sigma_xyz=0.05, loop_sigma_rot_deg=0.1, max_iterations=50, min_step=1e-9)   # sigma: the file's initial_sigma
    assert host.loop_closure_options(_cfg(host)) == want
    assert host.loop_closure_options(_cfg(host, "\nloop_closure:\n")) == want                     # an empty block is an absent one
    assert host.loop_closure_options(host.Config.FromYamlText("loop_closure:\n  top_k: 3\n"))["sigma"] == 0.5   # no params: the driver's default
    got = host.loop_closure_options(_cfg(host, "\nloop_closure:\n  min_travel: 12.5\n  top_k: 3\n  sigma: 0.75\n  max_place_dist: 9000\n  min_step: 1e-7\n"))
    assert got == dict(want, min_travel=12.5, top_k=3, sigma=0.75, max_place_dist=9000, min_step=1e-7)
    assert lr.options(lr.oo.load_pipeline_text(open(PIPE).read() + lc.OPTIONS)) == host.loop_closure_options(_cfg(host, lc.OPTIONS))


@pytest.mark.parametrize("key,value", [("min_travel", -1), ("gate_base", -0.5), ("gate_rate", -0.01), ("max_place_dist", -3), ("top_k", 0),
                                       ("min_travel_between_closures", -2), ("submap_radius", -1), ("sigma_xy", 0), ("sigma_yaw_deg", -1),
                                       ("sigma", 0), ("odometry_sigma_xyz", 0), ("odometry_sigma_rot_deg", -0.1), ("loop_sigma_xyz", 0),
                                       ("loop_sigma_rot_deg", 0), ("min_step", -1e-9), ("sigma_xy", "nan")])
def test_a_value_out_of_range_is_refused_by_name(host, key, value):
    with pytest.raises(RuntimeError, match=r"loop_closure: %s\b" % key):
        host.loop_closure_options(_cfg(host, "\nloop_closure:\n  %s: %s\n" % (key, value)))


@pytest.mark.parametrize("pipe", [PIPE, PIPE_NDT])
def test_the_shipped_pipelines_initialize_with_the_block(host, pipe):
    lo = host.LidarOdometry()
    lo.initialize(host.Config.FromYamlText(open(pipe).read() + "\nloop_closure:\n  min_travel: 40\n  top_k: 2\n"))
    assert lo.describePipeline()


# ---- the candidate rule ------------------------------------------------------------------------------------------------------------
def _pose(x, y, z=0.0):
    return [1.0, 0, 0, x, 0, 1.0, 0, y, 0, 0, 1.0, z]


def test_the_scenario_s_candidates_are_the_reference_s(host):
    s = lc.scenario()
    has = [True] * len(s["est"])
    matches = lr.match_lists(s["sweeps"], has)
    for block, accept in ((lc.OPTIONS, None), ("", None), (lc.OPTIONS, lambda i, j, shift, dist: False), (lc.OPTIONS, lambda i, j, shift, dist: i % 2 == 0)):
        opt = lr.options(lr.oo.load_pipeline_text(open(PIPE).read() + block))
        ref = lr.candidates(s["est"], has, matches, opt, accept)
        got = host.loop_candidates(s["est"], has, matches, host.loop_closure_options(_cfg(host, block)), accept)
        assert [tuple(p) for p in got] == ref and len(ref) > 0
    # with the scenario's options every closure is the true revisit, 57 frames back (one lap is 57.4 frames)
    ref = lr.candidates(s["est"], has, matches, lr.options(lr.oo.load_pipeline_text(open(PIPE).read() + lc.OPTIONS)))
    assert [(i, j) for i, j, _, _ in ref] == [(56, 1), (59, 2), (62, 5), (65, 8)]


def test_random_cases_equal_the_reference_exactly(host):
    rng = np.random.default_rng(20261019)
    n_pairs = 0
    for case in range(200):
        K = int(rng.integers(2, 40))
        steps = rng.normal(0.0, rng.uniform(0.5, 6.0), (K, 3)) * np.array([1.0, 1.0, 0.1])
        if case % 3 == 0:
            steps = np.round(steps)   # whole numbers: path lengths and distances land exactly on thresholds now and then
        t = np.cumsum(steps, 0)
        poses = np.array([_pose(*p) for p in t])
        has = [bool(v) for v in rng.uniform(size=K) < 0.85]
        idx = [k for k in range(K) if has[k]]
        matches = [[] for _ in range(K)]
        for k in idx:
            dist = rng.integers(0, 6, len(idx)) * 1000   # many ties: the order inside a tie is the frame's
            order = np.lexsort((np.array(idx), dist))
            matches[k] = [(idx[r], int(rng.integers(0, 64)), int(dist[r])) for r in order]
        opt = dict(min_travel=float(rng.choice([0.0, 3.0, 10.0, 30.0])), gate_base=float(rng.choice([0.0, 2.0, 5.0, 50.0])),
                   gate_rate=float(rng.choice([0.0, 0.02, 0.5])), max_place_dist=int(rng.choice([0, 1000, 3000])), top_k=int(rng.integers(1, 4)),
                   min_travel_between_closures=float(rng.choice([0.0, 5.0, 20.0])))
        mode = case % 4
        accept = None if mode == 0 else (lambda i, j, shift, dist, m=mode: (i * 7 + j * 3 + shift) % m != 0)
        ref = lr.candidates(poses, has, matches, dict(lr.DEFAULTS, **opt), accept)
        got = host.loop_candidates(poses, has, matches, opt, accept)
        assert [tuple(p) for p in got] == ref, (case, opt)
        n_pairs += len(ref)
    assert n_pairs > 300   # the cases do select


def test_the_travel_rule_and_the_gate_are_closed(host):
    # s = 0, 5, 10 (two 3-4-5 steps, the middle frame off the line): travel = 10 = min_travel, and |t_2 - t_0| = 8 = 3 + 0.5 * 10: on the gate
    poses = np.array([_pose(0, 0), _pose(4, 3), _pose(8, 0)])
    s = lr.path_lengths(poses)
    assert s[1] == 5.0 and s[2] == 10.0
    matches = [[], [], [(2, 0, 0), (0, 5, 700), (1, 0, 900)]]
    opt = dict(min_travel=10.0, gate_base=3.0, gate_rate=0.5)
    assert host.loop_candidates(poses, [True] * 3, matches, opt) == [(2, 0, 5, 700)] == lr.candidates(poses, [True] * 3, matches, dict(lr.DEFAULTS, **opt))
    for tighter in (dict(opt, min_travel=10.000001), dict(opt, gate_rate=0.4999999)):
        assert host.loop_candidates(poses, [True] * 3, matches, tighter) == [] == lr.candidates(poses, [True] * 3, matches, dict(lr.DEFAULTS, **tighter))
    # max_place_dist is closed too, and 0 switches it off
    assert host.loop_candidates(poses, [True] * 3, matches, dict(opt, max_place_dist=700)) == [(2, 0, 5, 700)]
    assert host.loop_candidates(poses, [True] * 3, matches, dict(opt, max_place_dist=699)) == []


def test_a_frame_without_points_is_never_a_partner_but_counts_in_the_path(host):
    poses = np.array([_pose(0, 0), _pose(0, 10), _pose(0.5, 0), _pose(1, 0)])   # s = 0, 10, 20.01, 20.51
    opt = dict(min_travel=20.2, gate_base=2.0, gate_rate=0.0, min_travel_between_closures=0.0)
    full = [(0, 0, 10), (1, 0, 20), (2, 0, 30), (3, 0, 40)]
    matches = [full, full, full, full]
    # frame 1 carries no points: it is no i and no j, yet its 10 m detour makes frame 3's travel from frame 0 20.51 >= 20.2
    assert host.loop_candidates(poses, [True, False, True, True], matches, opt) == [(3, 0, 0, 10)]
    assert lr.candidates(poses, [True, False, True, True], matches, dict(lr.DEFAULTS, **opt)) == [(3, 0, 0, 10)]
    # without frame 0's points nothing is left: frame 1 is near no-one, frame 2 is not far enough back
    assert host.loop_candidates(poses, [False, True, True, True], matches, opt) == []
    # a frame without points is never i either
    assert host.loop_candidates(poses, [True, True, True, False], matches, dict(opt, min_travel=0.0, gate_base=100.0)) == [(1, 0, 0, 10), (2, 0, 0, 10)]
    with pytest.raises(RuntimeError, match="names frame 9"):
        host.loop_candidates(poses, [True] * 4, [[(9, 0, 0)], [], [], []], opt)


# ---- the optimiser ---------------------------------------------------------------------------------------------------------------------
def _circle(K, seed, radius=20.0):
    """ground truth on a circle driven once and a little further (the last nodes revisit the first), and noisy odometry"""
    rng = np.random.default_rng(seed)
    ang = np.linspace(0.0, 2.0 * np.pi * 1.08, K)
    gt = [lc.to44(lc.synth.pose_from_ypr([radius * np.sin(a), radius * (1 - np.cos(a)), 0.3 * np.sin(2 * a), a, 0.02 * np.sin(a), 0.01])) for a in ang]
    est = [gt[0]]
    for k in range(1, K):
        D = np.linalg.inv(gt[k - 1]) @ gt[k]
        N = np.eye(4)
        N[:3, :3] = lc.exp_so3(rng.normal(0, 0.004, 3))
        N[:3, 3] = rng.normal(0, 0.03, 3)
        est.append(est[-1] @ D @ N)
    return np.array([lc.to12(T) for T in gt]), np.array([lc.to12(T) for T in est]), rng


def _loop(gt, a, b, rng):
    N = np.eye(4)
    N[:3, :3] = lc.exp_so3(rng.normal(0, 0.002, 3))
    N[:3, 3] = rng.normal(0, 0.02, 3)
    return (a, b, [float(v) for v in lc.to12(np.linalg.inv(lc.to44(gt[a])) @ lc.to44(gt[b]) @ N)])


def _pose_distance(A, B):
    """the largest translation difference [m] and rotation difference [rad] over the nodes"""
    dt = dr = 0.0
    for a, b in zip(np.asarray(A).reshape(-1, 12), np.asarray(B).reshape(-1, 12)):
        E = np.linalg.inv(lc.to44(a)) @ lc.to44(b)
        dt, dr = max(dt, float(np.linalg.norm(lc.to44(a)[:3, 3] - lc.to44(b)[:3, 3]))), max(dr, float(np.linalg.norm(lr.log_so3(E[:3, :3]))))
    return dt, dr


def test_a_chain_without_loops_comes_back_bit_for_bit(host):
    _, est, _ = _circle(25, 3)
    r = host.optimize_pose_graph(est, [])
    assert r["poses"].tobytes() == est.tobytes() and r["cost_before"] == 0.0 == r["cost_after"] and r["iterations"] == 0 and list(r["costs"]) == [0.0]


@pytest.mark.parametrize("n_loops", [1, 3])
def test_a_noisy_circle_reaches_the_reference_optimum(host, n_loops):
    gt, est, rng = _circle(40, 11 + n_loops)
    loops = [_loop(gt, a, b, rng) for a, b in [(0, 37), (2, 39), (1, 38)][:n_loops]]
    r = host.optimize_pose_graph(est, loops)
    ref, ref_costs = lr.optimize(est, loops, lr.DEFAULTS)
    dt, dr = _pose_distance(r["poses"], ref)
    print("loops", n_loops, "iterations", r["iterations"], "cost", r["cost_before"], "->", r["cost_after"], "reference", ref_costs[-1], "|dt|", dt, "|dr|", dr)
    assert dt < 1e-8 and dr < 1e-8
    assert r["poses"][0].tobytes() == est[0].tobytes()   # node 0 is fixed
    c = np.array(r["costs"])
    assert len(c) >= 2 and np.all(np.diff(c) <= 0.0) and c[0] == r["cost_before"] and c[-1] == r["cost_after"]
    assert abs(r["cost_after"] - ref_costs[-1]) <= 1e-6 * ref_costs[-1]
    assert abs(r["cost_before"] - ref_costs[0]) <= 1e-9 * ref_costs[0]
    # ... and the loop pulls the chain towards the truth
    assert lc.position_errors(r["poses"], gt)[-1] < 0.5 * lc.position_errors(est, gt)[-1]


def test_edges_that_touch_the_fixed_node_and_edges_given_backwards(host):
    gt, est, rng = _circle(12, 5)
    fwd = _loop(gt, 0, 11, rng)
    # the same measurement named from the other end: its residual lives in the other node's frame (E is conjugated by Z), so it
    # is another cost with another optimum -- each is held to the reference's for that very edge
    back = (11, 0, [float(v) for v in lc.to12(np.linalg.inv(lc.to44(fwd[2])))])
    far = (7, 2, [float(v) for v in _loop(gt, 7, 2, rng)[2]])   # a > b away from the fixed node
    for loops in ([fwd], [back], [back, far]):
        got = host.optimize_pose_graph(est, loops)
        ref, _ = lr.optimize(est, loops, lr.DEFAULTS)
        dt, dr = _pose_distance(got["poses"], ref)
        assert dt < 1e-8 and dr < 1e-8 and got["poses"][0].tobytes() == est[0].tobytes(), (loops, dt, dr)


def test_an_edge_out_of_range_throws(host):
    _, est, _ = _circle(6, 1)
    I = [1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0]
    with pytest.raises(RuntimeError, match="names node 6 of 6"):
        host.optimize_pose_graph(est, [(0, 6, I)])
    with pytest.raises(RuntimeError, match="to itself"):
        host.optimize_pose_graph(est, [(3, 3, I)])
    with pytest.raises(RuntimeError, match="12 values"):
        host.optimize_pose_graph(est, [(0, 3, I[:11])])
    with pytest.raises(RuntimeError, match="loop_closure: loop_sigma_xyz"):
        host.optimize_pose_graph(est, [(0, 3, I)], dict(loop_sigma_xyz=0.0))


def test_three_thousand_nodes_with_forty_loops(host):
    """five laps of 600 nodes, 40 loop edges that span one to four laps: the envelope holds 36 x (K + the spans) doubles, no dense
    matrix; the wall time goes into profiles/loop_closure.md"""
    K, lap = 3000, 600
    rng = np.random.default_rng(77)
    ang = 2.0 * np.pi * np.arange(K) / lap
    gt = [lc.to44(lc.synth.pose_from_ypr([60.0 * np.sin(a), 60.0 * (1 - np.cos(a)), 0.0, a, 0.0, 0.0])) for a in ang]
    est = [gt[0]]
    for k in range(1, K):
        N = np.eye(4)
        N[:3, :3] = lc.exp_so3(rng.normal(0, 0.0004, 3))
        N[:3, 3] = rng.normal(0, 0.004, 3)
        est.append(est[-1] @ np.linalg.inv(gt[k - 1]) @ gt[k] @ N)
    gt12, est12 = np.array([lc.to12(T) for T in gt]), np.array([lc.to12(T) for T in est])
    loops = []
    for n in range(40):
        b = int(rng.integers(lap, K))
        a = b - lap * int(rng.integers(1, b // lap + 1)) + int(rng.integers(-3, 4))
        loops.append(_loop(gt12, max(a, 0), b, rng))
    t0 = time.perf_counter()
    r = host.optimize_pose_graph(est12, loops)
    dt = time.perf_counter() - t0
    e0, e1 = lc.position_errors(est12, gt12), lc.position_errors(r["poses"], gt12)
    print("K", K, "loops", len(loops), "iterations", r["iterations"], "seconds", dt, "cost", r["cost_before"], "->", r["cost_after"],
          "max position error", e0.max(), "->", e1.max())
    assert r["iterations"] >= 1 and r["cost_after"] < r["cost_before"] and np.all(np.diff(r["costs"]) <= 0.0)
    assert r["poses"][0].tobytes() == est12[0].tobytes() and e1.max() < 0.5 * e0.max()


# ---- the corrected file ---------------------------------------------------------------------------------------------------------------
def test_a_corrected_set_differs_from_its_input_in_the_pose_bytes_only(host, tmp_path):
    """what close_loops writes: the input set with the optimiser's poses (tests/test_gpu_loop.py holds close_loops' own file to this)"""
    gt, est, rng = _circle(9, 2)
    pts = [rng.uniform(-20, 20, (50 + 7 * k, 3)).astype(np.float32) for k in range(9)]
    kf = lc.keyframe_set(est, pts)
    kf["frames"][3]["layers"] = None                       # a frame without points
    kf["frames"][5]["twist"] = [0.5, 0, 0, 0, 0, 0.1]      # ... and one with a twist
    kf["frames"][6]["cov"] = [float(v) for v in np.eye(6).reshape(36) * 1e-4]
    r = host.optimize_pose_graph(est, [_loop(gt, 0, 8, rng)])
    out = dict(maps=kf["maps"], frames=[dict(f, pose=[float(v) for v in p]) for f, p in zip(kf["frames"], r["poses"])])
    a, b = str(tmp_path / "in.mhkf"), str(tmp_path / "out.mhkf")
    host.write_keyframe_file(a, kf)
    host.write_keyframe_file(b, out)
    back = host.read_keyframe_file(b)                      # (the reader checks the checksum)
    assert [f["pose"] for f in back["frames"]] == [list(p) for p in r["poses"]]
    assert_only_poses_differ(open(a, "rb").read(), open(b, "rb").read(), kf)
    assert host.KEYFRAME_FILE_VERSION == 1


def pose_byte_ranges(kf):
    """[start, end) of every frame's 96 pose bytes in the version-1 file of the key-frame dict `kf` (INTEGRATION.md has the layout)"""
    pos = 8 + 4 + 4
    for m in kf["maps"]:
        pos += 4 + len(m["name"].encode()) + 4 + len(m["class_name"].encode()) + 7 * 4 + 4
    pos += 8
    out = []
    for f in kf["frames"]:
        pos += 8
        out.append((pos, pos + 96))
        pos += 96 + 36 * 8 + 1 + (48 if f["twist"] is not None else 0) + 1
        if f["layers"] is not None:
            pos += 4 + sum(4 + 8 + 12 * len(xyz) for _, xyz in f["layers"])
    return out, pos   # pos: where the checksum starts


def assert_only_poses_differ(a, b, kf):
    ranges, end = pose_byte_ranges(kf)
    assert len(a) == len(b) == end + 8
    A, B = np.frombuffer(a, np.uint8), np.frombuffer(b, np.uint8)
    mask = np.zeros(len(A), bool)
    for lo, hi in ranges:
        mask[lo:hi] = True
    mask[end:] = True   # the checksum follows the content
    assert np.array_equal(A[~mask], B[~mask])
    assert not np.array_equal(A[ranges[-1][0]:ranges[-1][1]], B[ranges[-1][0]:ranges[-1][1]])
    assert np.array_equal(A[ranges[0][0]:ranges[0][1]], B[ranges[0][0]:ranges[0][1]])   # node 0 is fixed


# ---- the reference alone on the scenario ----------------------------------------------------------------------------------------------------
def test_the_reference_closes_the_scenario_s_loop(host, oracle):
    s = lc.scenario()
    e0 = lc.position_errors(s["est"], s["gt"])
    assert abs(e0[-1] - 3.29) < 0.01 and abs(e0.max() - 4.13) < 0.01 and len(s["gt"]) == 66
    ref = lr.scenario_reference(open(PIPE).read() + lc.OPTIONS)
    accepted = [p for p in ref["pairs"] if p["accepted"]]
    assert len(accepted) >= 1
    for p in ref["pairs"]:
        err = float(np.linalg.norm((p["Z"] - lc.relative(s["gt"][p["j"]], s["gt"][p["i"]]))[[3, 7, 11]]))
        print("pair", p["i"], p["j"], "shift", p["shift"], "dist", p["dist"], "candidates", p["candidates"], "ranks", p["ranks"], "quality", p["quality"],
              "iterations", p["iterations"], "accepted", p["accepted"], "|Z - truth| [m]", err)
        assert p["candidates"] == 19 * 19 * 5
        if p["accepted"]:
            assert err < EDGE_BOUND
    e1 = lc.position_errors(ref["poses"], s["gt"])
    print("end error", e0[-1], "->", e1[-1], "max over the frames", e0.max(), "->", e1.max(), "cost", ref["costs"][0], "->", ref["costs"][-1])
    assert e1[-1] <= END_BOUND and e1.max() <= MAX_BOUND
    # the scenario's graph, the reference's edges: the product's optimiser reaches the reference's optimum
    loops = [(p["j"], p["i"], [float(v) for v in p["Z"]]) for p in accepted]
    r = host.optimize_pose_graph(s["est"], loops, host.loop_closure_options(_cfg(host, lc.OPTIONS)))
    dt, dr = _pose_distance(r["poses"], ref["poses"])
    print("optimiser against the reference: |dt|", dt, "|dr|", dr, "iterations", r["iterations"])
    assert dt < 1e-8 and dr < 1e-8 and np.all(np.diff(r["costs"]) <= 0.0) and r["poses"][0].tobytes() == s["est"][0].tobytes()
