"""Joining two sessions, the parts that need no device: the session_join: options, the refusals, the candidate rule
(mola_hip::join_candidates / join_candidates_step) against the restatement of tests/join_ref.py -- exactly --, the optimiser with fixed
nodes (mola_hip::optimize_pose_graph_anchored) against the restatement's dense Gauss-Newton, the joined key-frame file, and the
restatement alone on the scenario of tests/join_cases.py -- a condition on the scenario: it must be joined through both overlaps by
the restatement before the device is held to it (tests/test_gpu_session_join.py).

Measured here: the restatement anchors B's frame 0 on A's frame 41 (quality 0.989), then accepts (3, 44), (16, 0), (19, 2), (22, 5)
and (25, 8) at 0.984-0.9995; B's last frame ends 0.30 m from the truth where the anchor alone leaves it 3.31 m away (A's own drift,
2.7-3.2 m at its end, stays: A is never moved)."""
import os

import numpy as np
import pytest

import join_cases as jc
import join_ref as jr
import loop_cases as lc
import loop_ref as lr
import test_loop_cpu as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIPE = os.path.join(ROOT, "pipelines", "lidar3d-default-hip.yaml")


@pytest.fixture(scope="module")
def host():
    from mola_lidar_odometry_amd import _mp2p_icp_hip as H
    return H


def _cfg(host, block=""):
    return host.Config.FromYamlText(open(PIPE).read() + block)


# ---- options ---------------------------------------------------------------------------------------------------------------------
def test_the_defaults_are_the_documented_ones(host):
    want = dict(top_k=0, max_place_dist=0, min_links=2, min_travel_between_links=10.0, max_anchor_frames=0)
    assert host.session_join_options(_cfg(host)) == want == jr.DEFAULTS
    assert host.session_join_options(_cfg(host, "\nsession_join:\n")) == want   # an empty block is an absent one
    got = host.session_join_options(_cfg(host, "\nsession_join:\n  top_k: 3\n  max_place_dist: 9000\n  min_links: 4\n  min_travel_between_links: 7.5\n  max_anchor_frames: 12\n"))
    assert got == dict(top_k=3, max_place_dist=9000, min_links=4, min_travel_between_links=7.5, max_anchor_frames=12)
    # the restatement reads the scenario's block as the product does, and resolves top_k: 0 to relocalization.place_top_k
    o = jr.options(lr.oo.load_pipeline_text(open(PIPE).read() + jc.OPTIONS))
    assert {k: o[k] for k in want} == host.session_join_options(_cfg(host, jc.OPTIONS))
    assert jr.options(lr.oo.load_pipeline_text(open(PIPE).read()))["top_k"] == 4


@pytest.mark.parametrize("key,value", [("top_k", -1), ("top_k", 1.5), ("max_place_dist", -3), ("min_links", 0), ("min_links", -2),
                                       ("min_travel_between_links", -1), ("min_travel_between_links", "nan"), ("max_anchor_frames", -1)])
def test_a_value_out_of_range_is_refused_by_name(host, key, value):
    with pytest.raises(RuntimeError, match=r"session_join: %s\b" % key):
        host.session_join_options(_cfg(host, "\nsession_join:\n  %s: %s\n" % (key, value)))


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def _tiny(n, seed=0, points=True):
    rng = np.random.default_rng(seed)
    sweeps = [rng.uniform(-20, 20, (50, 3)).astype(np.float32) for _ in range(n)]
    kf = lc.keyframe_set([tc._pose(2.0 * k, 0.0) for k in range(n)], sweeps)
    if not points:
        for f in kf["frames"]:
            f["layers"] = None
    return kf


def test_sessions_recorded_for_other_maps_are_refused(host):
    a = _tiny(3)
    for change, what in ((lambda m: m.update(name="other"), r"map 0 is 'localmap' in the first and 'other' in the second"),
                         (lambda m: m.update(class_name="NDT"), r"'HashedVoxelPointCloud' in the first and a 'NDT' in the second"),
                         (lambda m: m["params"].update(voxel_size=2.0), r"voxel_size 1\.0+ in the first and 2\.0+ in the second"),
                         (lambda m: m["params"].update(max_points_per_voxel=21), r"max_points_per_voxel 20\.0+ in the first and 21"),
                         (lambda m: m.update(remove_voxels_farther_than=50.0), r"remove_voxels_farther_than")):
        b = _tiny(2, 1)
        change(b["maps"][0])
        with pytest.raises(RuntimeError, match=r"join_sessions: .*same target maps: .*" + what):
            host.join_sessions(a, b, _cfg(host))
    b = _tiny(2, 1)
    b["maps"].append(dict(b["maps"][0], name="second"))
    with pytest.raises(RuntimeError, match="the first names 1, the second 2"):
        host.join_sessions(a, b, _cfg(host))


def test_a_header_with_an_occupancy_map_is_refused(host):
    a, b = _tiny(3), _tiny(2, 1)
    for kf in (a, b):
        kf["maps"][0]["class_name"] = "CVoxelMap"
    with pytest.raises(RuntimeError, match=r"join_sessions: target map 'localmap' is a 'CVoxelMap': an occupancy map"):
        host.join_sessions(a, b, _cfg(host))


def test_an_option_out_of_range_stops_the_join_itself(host):
    with pytest.raises(RuntimeError, match=r"session_join: min_links\b"):
        host.join_sessions(_tiny(3), _tiny(2, 1), _cfg(host, "\nsession_join:\n  min_links: 0\n"))
    with pytest.raises(RuntimeError, match=r"loop_closure: sigma_xy\b"):
        host.join_sessions(_tiny(3), _tiny(2, 1), _cfg(host, "\nloop_closure:\n  sigma_xy: 0\n"))


def test_an_empty_session_and_one_without_points_are_not_joined(host, tmp_path):
    a = _tiny(4)
    want = str(tmp_path / "a.mhkf")
    host.write_keyframe_file(want, a)
    for n, (b, name) in enumerate(((dict(maps=a["maps"], frames=[]), "empty"), (_tiny(3, 1, points=False), "bare"))):
        out = str(tmp_path / ("%s.mhkf" % name))
        joined, is_joined, report = host.join_sessions(a, b, _cfg(host), out)
        assert is_joined is False and report["joined"] is False and report["links_accepted"] == 0 and report["pairs"] == []
        assert not os.path.exists(out)                                       # nothing is written for sessions that are not joined
        got = str(tmp_path / ("got%d.mhkf" % n))
        host.write_keyframe_file(got, joined)
        assert open(got, "rb").read() == open(want, "rb").read()            # `joined` is A


# ---- the candidate rule ------------------------------------------------------------------------------------------------------------
def _same(got, ref):
    """tried pairs, their order and phase, exactly; the grid centres to rounding; the links -- the carried state -- exactly"""
    (gt, gl), (rt, rl) = got, ref
    assert [tuple(p[:5]) for p in gt] == [tuple(p[:5]) for p in rt]
    for p, q in zip(gt, rt):
        assert np.abs(np.array(p[5]) - np.array(q[5])).max() <= 1e-9 * max(1.0, np.abs(np.array(q[5])).max())
    assert [(b, j, list(Z)) for b, j, Z in gl] == [(b, j, list(Z)) for b, j, Z in rl]


def _line():
    """A: ten frames 10 m apart on the x axis.  B: seven frames 5 m apart whose true places are x = 10, 15, .., 40, recorded in a
    frame shifted by (-110, 50, 0): whole numbers and no rotation, so that every sum of the rule is exact."""
    A = np.array([tc._pose(10.0 * j, 0.0) for j in range(10)])
    W = np.array([tc._pose(10.0 + 5.0 * b, 0.0) for b in range(7)])
    B = np.array([tc._pose(5.0 * b - 100.0, 50.0) for b in range(7)])
    matches = []
    for b in range(7):
        d = [int(abs(W[b][3] - A[j][3]) * 100) for j in range(10)]
        matches.append([(j, (3 * b + j) % 64, d[j]) for j in sorted(range(10), key=lambda j: (d[j], j))])
    return A, W, B, matches


def _true_Z(A, W):
    return lambda b, j: [float(v) for v in lc.relative(A[j], W[b])]


@pytest.mark.parametrize("anchor_at", [0, 3, 6])
@pytest.mark.parametrize("top_k", [1, 3])
def test_a_hand_made_case_with_the_anchor_at_the_first_a_middle_and_the_last_frame(host, anchor_at, top_k):
    A, W, B, matches = _line()
    Z = _true_Z(A, W)
    opt = dict(top_k=top_k, min_travel_between_links=10.0, gate_base=5.0, gate_rate=0.0, place_sectors=64)

    def accept(b, j, shift, dist, phase, centre):
        if phase == jr.ANCHOR:
            return Z(b, j) if b == anchor_at else None
        return Z(b, j) if dist <= 500 and j % 2 == 0 else None   # a partner with an odd index is rejected: the next in rank is tried
    has = [True] * 10
    got = host.join_candidates(A, has, B, [True] * 7, matches, opt, accept)
    ref = jr.candidates(A, has, B, [True] * 7, matches, dict(jr.DEFAULTS, **opt), accept)
    _same(got, ref)
    tried, links = got
    assert links[0][:2] == (anchor_at, {0: 1, 3: 2, 6: 4}[anchor_at])                # the first in rank: x = 25 is as far from A's frame 2 as from 3
    phases = [p[4] for p in tried]
    assert phases == sorted(phases) and phases.count(jr.ANCHOR) >= 1                 # anchor, then forward, then backward
    assert (jr.FORWARD in phases) == (anchor_at + 2 <= 6) and (jr.BACKWARD in phases) == (anchor_at >= 2)
    # the anchor's centre is the yaw the shift stands for, no translation; a link's centre is the predicted pose in the partner's frame
    b, j, shift = tried[0][:3]
    assert np.allclose(tried[0][5], jr.rz(-shift * 2.0 * np.pi / 64.0), atol=1e-15)
    for p in tried:
        if p[4] != jr.ANCHOR:
            assert np.allclose(p[5], Z(p[0], p[1]), atol=1e-12)   # the prediction from a true link is the true place


def test_the_gate_and_the_travel_rule_are_closed(host):
    A, W, B, matches = _line()
    Z = _true_Z(A, W)
    has = [True] * 10
    accept = lambda b, j, shift, dist, phase, centre: Z(b, j)   # noqa: E731
    # from the anchor (0, 1): frame 1 is 5 m of travel on: tried only when min_travel_between_links <= 5; its place x = 15 is 5 m from A's
    # frames 1 and 2: inside a gate of exactly 5
    opt = dict(top_k=1, min_travel_between_links=5.0, gate_base=5.0, gate_rate=0.0, place_sectors=64, max_anchor_frames=1)
    for o, want in ((opt, [0, 1, 2, 3, 4, 5, 6]), (dict(opt, min_travel_between_links=5.000001), [0, 2, 4, 6]), (dict(opt, gate_base=4.999999), [0, 2, 4, 6]),
                    # ... and with a rate: frame 3, 15 m on, stands at x = 25, 5 = 1.25 + 0.25 * 15 m from A's frames 2 and 3
                    (dict(opt, min_travel_between_links=15.0, gate_base=1.25, gate_rate=0.25), [0, 3, 6]),
                    (dict(opt, min_travel_between_links=15.0, gate_base=1.25, gate_rate=0.2499999), [0, 4]),
                    (dict(opt, min_travel_between_links=0.0, gate_base=0.0), [0, 2, 4, 6])):
        got = host.join_candidates(A, has, B, [True] * 7, matches, o, accept)
        _same(got, jr.candidates(A, has, B, [True] * 7, matches, dict(jr.DEFAULTS, **o), accept))
        assert [p[0] for p in got[0]] == want, o
    # max_place_dist is closed too, and 0 switches it off: frame 1's best partner is at dist 500
    for bound, want in ((500, [0, 1, 2, 3, 4, 5, 6]), (499, [0, 2, 4, 6])):
        o = dict(opt, max_place_dist=bound)
        got = host.join_candidates(A, has, B, [True] * 7, matches, o, accept)
        _same(got, jr.candidates(A, has, B, [True] * 7, matches, dict(jr.DEFAULTS, **o), accept))
        assert [p[0] for p in got[0]] == want
    # without a verification every pair is accepted with Z = its centre
    _same(host.join_candidates(A, has, B, [True] * 7, matches, opt), jr.candidates(A, has, B, [True] * 7, matches, dict(jr.DEFAULTS, **opt)))


def test_frames_without_points_and_the_anchor_budget(host):
    A, W, B, matches = _line()
    Z = _true_Z(A, W)
    accept = lambda b, j, shift, dist, phase, centre: Z(b, j)   # noqa: E731
    opt = dict(top_k=2, min_travel_between_links=5.0, gate_base=5.0, gate_rate=0.0, place_sectors=64)
    has_a = [True, False, True, True, True, True, True, True, True, True]   # A's frame 1 is never a partner
    has_b = [False, True, True, False, True, True, True]                    # B's frames 0 and 3 are never tried, yet count in the path
    got = host.join_candidates(A, has_a, B, has_b, matches, opt, accept)
    _same(got, jr.candidates(A, has_a, B, has_b, matches, dict(jr.DEFAULTS, **opt), accept))
    assert got[1][0][:2] == (1, 2) and all(p[1] != 1 and p[0] not in (0, 3) for p in got[0])
    # the anchor is looked for among the first max_anchor_frames frames WITH points: with every anchor rejected, 2 frames x 2 partners
    reject_anchor = lambda b, j, shift, dist, phase, centre: None   # noqa: E731
    o = dict(opt, max_anchor_frames=2)
    got = host.join_candidates(A, has_a, B, has_b, matches, o, reject_anchor)
    _same(got, jr.candidates(A, has_a, B, has_b, matches, dict(jr.DEFAULTS, **o), reject_anchor))
    assert [p[0] for p in got[0]] == [1, 1, 2, 2] and got[1] == []
    with pytest.raises(RuntimeError, match="names frame 10 of 10"):
        host.join_candidates(A, has_a, B, has_b, [[(10, 0, 0)]] + [[]] * 6, opt)


def test_one_step_of_a_sweep_carries_the_link_as_the_fold_does(host):
    A, W, B, matches = _line()
    Z = _true_Z(A, W)
    accept = lambda b, j, shift, dist, phase, centre: Z(b, j) if j != 3 else None   # noqa: E731
    opt = dict(top_k=3, min_travel_between_links=10.0, gate_base=5.0, gate_rate=0.0, place_sectors=64)
    has = [True] * 10
    tried, links = host.join_candidates(A, has, B, [True] * 7, matches, opt,
                                        lambda b, j, s, d, phase, c: (Z(b, j) if b == 2 else None) if phase == jr.ANCHOR else accept(b, j, s, d, phase, c))
    assert links[0][:2] == (2, 2)
    for phase, order in ((jr.FORWARD, range(3, 7)), (jr.BACKWARD, range(1, -1, -1))):
        carried, mine, mine_links = links[0], [], []
        for b in order:
            t, accepted, after = host.join_candidates_step(A, has, B, [True] * 7, b, phase, matches[b], opt, carried, accept)
            mine += t
            assert accepted == (after != carried)
            if accepted:
                mine_links.append(after)
            carried = after
        assert [tuple(p[:5]) for p in mine] == [tuple(p[:5]) for p in tried if p[4] == phase]
        want = [l for l in links[1:] if (l[0] > 2) == (phase == jr.FORWARD)]
        assert [(l[0], l[1], list(l[2])) for l in mine_links] == [(l[0], l[1], list(l[2])) for l in want] and len(want) >= 1


def _random_pose(rng, t, yaw, wobble):
    T = np.eye(4)
    T[:3, :3] = lc.exp_so3([0, 0, yaw]) @ lc.exp_so3(rng.normal(0, wobble, 3))
    T[:3, 3] = t
    return T


def test_random_cases_equal_the_restatement_exactly(host):
    rng = np.random.default_rng(20261020)
    n_pairs, n_links, anchors, phases_seen = 0, 0, set(), set()
    for case in range(200):
        whole = case % 3 == 0   # whole numbers, no rotation: predicted places land exactly on the gate now and then
        KA, KB = int(rng.integers(3, 30)), int(rng.integers(1, 25))
        steps = rng.normal(0.0, rng.uniform(1.0, 6.0), (KA, 3)) * np.array([1.0, 1.0, 0.1])
        tA = np.cumsum(np.round(steps) if whole else steps, 0)
        A44 = [_random_pose(rng, tA[k], 0.0 if whole else rng.uniform(-3, 3), 0.0 if whole else 0.05) for k in range(KA)]
        # B's true places wander along A's path; its record is in a frame of its own
        at = np.clip(np.cumsum(rng.integers(-1, 3, KB)) + int(rng.integers(0, KA)), 0, KA - 1)
        off = rng.normal(0.0, 2.0, (KB, 3)) * np.array([1.0, 1.0, 0.1])
        W44 = [_random_pose(rng, tA[at[b]] + (np.round(off[b]) if whole else off[b]), 0.0 if whole else rng.uniform(-3, 3), 0.0 if whole else 0.05) for b in range(KB)]
        Gi = _random_pose(rng, np.round(rng.uniform(-200, 200, 3)), 0.0 if whole else rng.uniform(-3, 3), 0.0 if whole else 0.3)
        A = np.array([lc.to12(T) for T in A44])
        B = np.array([lc.to12(Gi @ T) for T in W44])
        has_a = [bool(v) for v in rng.uniform(size=KA) < 0.85]
        has_b = [bool(v) for v in rng.uniform(size=KB) < 0.85]
        idx = [k for k in range(KA) if has_a[k]]
        matches = [[] for _ in range(KB)]
        for b in range(KB):
            if has_b[b] and idx:
                dist = rng.integers(0, 6, len(idx)) * 1000   # many ties: the order inside a tie is the frame's
                order = np.lexsort((np.array(idx), dist))
                matches[b] = [(idx[r], int(rng.integers(0, 64)), int(dist[r])) for r in order]
        noise = rng.normal(0.0, 0.3, (KB, KA, 3)) * (0.0 if whole else 1.0)
        table = {(b, j): [float(v) for v in lc.to12(np.linalg.inv(A44[j]) @ W44[b] @ _random_pose(rng, noise[b, j], 0.0, 0.0))] for b in range(KB) for j in range(KA)}
        opt = dict(top_k=int(rng.integers(1, 4)), max_place_dist=int(rng.choice([0, 1000, 3000])), min_travel_between_links=float(rng.choice([0.0, 5.0, 20.0])),
                   max_anchor_frames=int(rng.choice([0, 1, 3])), gate_base=float(rng.choice([0.0, 2.0, 5.0, 50.0])), gate_rate=float(rng.choice([0.0, 0.02, 0.5])),
                   place_sectors=int(rng.choice([32, 64])))
        mode = 2 + case % 4
        accept = lambda b, j, shift, dist, phase, centre, m=mode: table[(b, j)] if (b * 7 + j * 3 + shift + phase) % m != 0 else None   # noqa: E731
        ref = jr.candidates(A, has_a, B, has_b, matches, dict(jr.DEFAULTS, **opt), accept)
        got = host.join_candidates(A, has_a, B, has_b, matches, opt, accept)
        _same(got, ref)
        n_pairs += len(ref[0])
        n_links += len(ref[1])
        phases_seen |= {p[4] for p in ref[0]}
        if ref[1]:
            with_points = [b for b in range(KB) if has_b[b]]
            anchors.add("first" if ref[1][0][0] == with_points[0] else "last" if ref[1][0][0] == with_points[-1] else "middle")
    print("pairs", n_pairs, "links", n_links, "anchors", sorted(anchors))
    assert n_pairs > 600 and n_links > 300 and phases_seen == {0, 1, 2} and anchors == {"first", "middle", "last"}   # the cases do select


# ---- the optimiser with fixed nodes ------------------------------------------------------------------------------------------------------
N_FIXED, N_FREE = 15, 30


def _two_sessions(seed):
    """a circle driven once and a little further: A is nodes 0 .. 14 of one noisy drive, B nodes 12 .. 41 of another, in its own frame"""
    gt, est_a, rng = tc._circle(45, seed)
    _, est_b, _ = tc._circle(45, seed + 100)
    Gb = lc.to44(lc.synth.pose_from_ypr([40.0, -25.0, 2.0, 1.1, 0.05, -0.03]))
    poses = np.concatenate([est_a[:N_FIXED], jc.moved(est_b[12:12 + N_FREE], Gb)], 0)

    def link(j, k):   # A's node j, B's node k: the true relative pose and a little noise
        a, b, Z = tc._loop(gt, j, 12 + k, rng)
        return (j, N_FIXED + k, Z)
    return gt, poses, link


@pytest.mark.parametrize("n_links", [2, 5])
def test_b_s_chain_reaches_the_reference_optimum(host, n_links):
    gt, poses, link = _two_sessions(21 + n_links)
    links = [link(j, k) for j, k in [(12, 0), (0, 29), (14, 2), (1, 28), (13, 1)][:n_links]]
    r = host.optimize_pose_graph_anchored(poses, N_FIXED, [], links)
    ref, ref_costs = jr.optimize_anchored(poses, N_FIXED, links, lr.DEFAULTS)
    dt, dr = tc._pose_distance(r["poses"], ref)
    print("links", n_links, "iterations", r["iterations"], "cost", r["cost_before"], "->", r["cost_after"], "reference", ref_costs[-1], "|dt|", dt, "|dr|", dr)
    assert dt < 1e-8 and dr < 1e-8
    assert r["poses"][:N_FIXED].tobytes() == poses[:N_FIXED].tobytes()   # the fixed nodes, bit for bit
    c = np.array(r["costs"])
    assert len(c) >= 2 and np.all(np.diff(c) <= 0.0) and c[0] == r["cost_before"] and c[-1] == r["cost_after"]
    assert abs(r["cost_after"] - ref_costs[-1]) <= 1e-6 * ref_costs[-1]
    assert abs(r["cost_before"] - ref_costs[0]) <= 1e-9 * ref_costs[0]
    # ... and the second overlap pulls B's end towards the truth, which the placement by the first link alone leaves adrift
    placed = jr.placement(poses, N_FIXED, links[0])
    assert lc.position_errors(r["poses"][N_FIXED:], gt[12:42])[-1] < 0.5 * lc.position_errors(placed[N_FIXED:], gt[12:42])[-1]


def test_one_link_gives_the_rigid_placement(host):
    _, poses, link = _two_sessions(7)
    for l in (link(12, 0), link(0, 29), link(14, 17)):
        r = host.optimize_pose_graph_anchored(poses, N_FIXED, [], [l])
        assert r["cost_before"] == 0.0 == r["cost_after"] and r["iterations"] == 0 and list(r["costs"]) == [0.0]
        assert np.abs(r["poses"] - jr.placement(poses, N_FIXED, l)).max() < 1e-12
        assert r["poses"][:N_FIXED].tobytes() == poses[:N_FIXED].tobytes()
        # the same link named from B's end places the chain by its inverse
        back = (l[1], l[0], [float(v) for v in lc.to12(np.linalg.inv(lc.to44(l[2])))])
        assert np.abs(host.optimize_pose_graph_anchored(poses, N_FIXED, [], [back])["poses"] - r["poses"]).max() < 1e-9


def test_the_chain_form_equals_optimize_pose_graph_with_one_fixed_node(host):
    """one fixed node and one chain placed where it already stands: the graph optimize_pose_graph solves, held to its result"""
    gt, est, rng = tc._circle(40, 12)
    loops = [tc._loop(gt, 0, 37, rng), tc._loop(gt, 2, 39, rng)]
    first = (0, 1, [float(v) for v in lc.relative(est[0], est[1])])   # the chain's own first step: places it where it stands
    a = host.optimize_pose_graph_anchored(est, 1, [], [first] + loops, dict(loop_sigma_xyz=0.02, loop_sigma_rot_deg=0.05))
    b = host.optimize_pose_graph(est, loops, dict(loop_sigma_xyz=0.02, loop_sigma_rot_deg=0.05))
    dt, dr = tc._pose_distance(a["poses"], b["poses"])
    assert dt < 1e-8 and dr < 1e-8


def test_graphs_that_cannot_be_solved_are_refused(host):
    _, poses, link = _two_sessions(3)
    I = jr.I12
    for args, what in (((poses, 0, [], [link(12, 0)]), "0 fixed nodes of 45"), ((poses, N_FIXED, [], [(3, 4, I)]), r"\(3, 4\) joins two fixed nodes"),
                       ((poses, N_FIXED, [], [(3, 45, I)]), "names node 45 of 45"), ((poses, N_FIXED, [], [(20, 20, I)]), "to itself"),
                       ((poses, N_FIXED, [5], [link(12, 0)]), "cannot start at node 5"), ((poses, N_FIXED, [30], [link(12, 0)]), "starts at node 30 has no edge from a fixed node"),
                       ((poses, N_FIXED, [], []), "starts at node 15 has no edge from a fixed node"), ((poses, N_FIXED, [], [(3, 20, I[:11])]), "12 values")):
        with pytest.raises(RuntimeError, match=what):
            host.optimize_pose_graph_anchored(*args)
    with pytest.raises(RuntimeError, match="loop_closure: loop_sigma_xyz"):
        host.optimize_pose_graph_anchored(poses, N_FIXED, [], [link(12, 0)], dict(loop_sigma_xyz=0.0))
    # two chains, each with its own links
    r = host.optimize_pose_graph_anchored(poses, N_FIXED, [30], [link(12, 0), link(13, 1), link(0, 29), link(1, 28)])
    assert r["iterations"] >= 1 and r["poses"][:N_FIXED].tobytes() == poses[:N_FIXED].tobytes()


# ---- the joined file ---------------------------------------------------------------------------------------------------------------------
def test_a_joined_set_round_trips_and_holds_a_s_frames_byte_for_byte(host, tmp_path):
    """the set join_sessions composes -- A's header, A's frames, then B's with other poses -- written, read back and compared with A's
    own file: between the header and the checksum A's frame bytes stand unchanged at the front of the frame block"""
    rng = np.random.default_rng(5)
    a, b = _tiny(5), _tiny(4, 1)
    a["frames"][2]["twist"] = [0.5, 0.0, 0.1, 0.0, 0.0, 0.02]
    a["frames"][3]["layers"] = None
    b["frames"][1]["cov"] = [float(v) for v in rng.uniform(0, 1, 36)]
    poses = np.array([f["pose"] for f in a["frames"]] + [f["pose"] for f in b["frames"]])
    placed = host.optimize_pose_graph_anchored(poses, 5, [], [(1, 5, tc._pose(0.5, -0.25, 0.1))])["poses"]
    joined = dict(maps=a["maps"], frames=a["frames"] + [dict(f, pose=[float(v) for v in placed[5 + k]]) for k, f in enumerate(b["frames"])])
    fa, fj, fe = str(tmp_path / "a.mhkf"), str(tmp_path / "joined.mhkf"), str(tmp_path / "empty.mhkf")
    host.write_keyframe_file(fa, a)
    host.write_keyframe_file(fj, joined)
    host.write_keyframe_file(fe, dict(maps=a["maps"], frames=[]))
    A, J, header = open(fa, "rb").read(), open(fj, "rb").read(), len(open(fe, "rb").read()) - 16   # (a frame count and a checksum follow the header)
    assert J[:header] == A[:header] and int.from_bytes(J[header:header + 8], "little") == 9 and int.from_bytes(A[header:header + 8], "little") == 5
    assert J[header + 8:header + 8 + len(A) - header - 16] == A[header + 8:-8]
    back = host.read_keyframe_file(fj)
    again = str(tmp_path / "again.mhkf")
    host.write_keyframe_file(again, back)
    assert open(again, "rb").read() == J
    assert [f["pose"] for f in back["frames"][5:]] == [[float(v) for v in placed[5 + k]] for k in range(4)]
    assert [f["timestamp"] for f in back["frames"]] == [f["timestamp"] for f in a["frames"] + b["frames"]] and back["frames"][6]["cov"] == b["frames"][1]["cov"]


# ---- the scenario: a condition on the data, checked on the restatement alone ------------------------------------------------------------------
def test_the_restatement_joins_the_scenario_through_both_overlaps(host, oracle):
    ref = scenario_reference()
    s = jc.scenario()
    print("pairs", [(p["i"], p["j"], p["phase"], round(p["quality"], 4), p["iterations"], p["accepted"]) for p in ref["pairs"]])
    links = ref["links"]
    assert ref["is_joined"] and len(links) >= ref["options"]["min_links"]
    assert any(j >= 40 for _, j, _ in links) and any(j <= 6 for _, j, _ in links)
    e_placed, e_joined = lc.position_errors(ref["placed_b"], s["b_gt"]), lc.position_errors(ref["poses_b"], s["b_gt"])
    print("B's last frame: anchor only", e_placed[-1], "joined", e_joined[-1], "maximum over B", e_placed.max(), "->", e_joined.max())
    assert e_joined[-1] < e_placed[-1]


_REFERENCE = {}


def scenario_reference(block=None):
    """join_cases' sessions joined by the restatement (about 30 s on the CPU); once per process, shared, never modified"""
    block = jc.OPTIONS if block is None else block
    if block not in _REFERENCE:
        a, b = jc.sessions()
        _REFERENCE[block] = jr.join_sessions(a, b, lr.oo.load_pipeline_text(open(PIPE).read() + block))
    return _REFERENCE[block]
