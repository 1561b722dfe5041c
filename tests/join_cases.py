"""The scenario of the session-join tests (tests/test_session_join_cpu.py, tests/test_gpu_session_join.py), built from
tests/loop_cases.py: session A is the first 46 key-frames of its drive (arcs 0 .. 270 m, three sides of the block and the start of
the fourth, with their drifted poses); session B is a second vehicle on the same path from 243 m to 393 m -- the end of A's drive,
the rest of the block (a lap is 344 m), and 49 m into A's first street -- 26 key-frames 6 m apart, 3 m out of phase with A's at its
end, 0.3 m to the right of the path, cast anew with seeds of their own, drifting from their own origin, and recorded in a frame
that has nothing to do with A's (G).  No B scan equals an A scan; B overlaps A twice, at A's frames 40 .. 45 and at A's frames
0 .. 8.
Data generation only (mola_lidar_odometry_amd.synth / synth_city through loop_cases); no product code."""
import functools

import numpy as np
import pytest

import loop_cases as lc
from mola_lidar_odometry_amd import synth, synth_city

N_A = 46                                              # A: frames 0 .. 45 of loop_cases.scenario()
B_ARCS = np.arange(243.0, 394.0, 6.0)                 # B: 243, 249, ..., 393 m -> 26 frames
B_LATERAL = -0.3                                      # [m] left of the path
B_SEED = 900                                          # frame n is cast with seed 900 + n (A's are 500 + n)
G_YAW_DEG, G_T = 77.0, (120.0, -45.0, 3.0)            # B's frame in the world ...
G2_YPR_DEG, G2_T = (-160.0, 4.0, -3.0), (-800.0, 310.0, -12.0)   # ... and another one, for the test that the join does not look at it
# the session_join: block of the tests: every third B frame is tried for a link (18 m of B's path), two partners per frame at the
# most, the anchor is looked for among B's first three frames -- about six verifications, which is what the restatement on the CPU
# oracle can afford (tests/loop_ref.py: some 8 s each)
OPTIONS = "\nsession_join:\n  top_k: 2\n  min_travel_between_links: 18\n  max_anchor_frames: 3\n"


def rigid(yaw_deg, t, pitch_deg=0.0, roll_deg=0.0):
    return lc.to44(synth.pose_from_ypr([t[0], t[1], t[2], np.deg2rad(yaw_deg), np.deg2rad(pitch_deg), np.deg2rad(roll_deg)]))


G = rigid(G_YAW_DEG, G_T)
G2 = rigid(G2_YPR_DEG[0], G2_T, G2_YPR_DEG[1], G2_YPR_DEG[2])


def poses_at(arcs, lateral):
    """[n, 12] poses on the path of loop_cases.ROUTE at the given arcs, `lateral` metres to its left"""
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(synth_city, "ROUTE", lc.ROUTE)
        px, py, ph, _ = synth_city._planned_path(0.1)
    arc = np.concatenate([[0.0], np.cumsum(np.hypot(np.diff(px), np.diff(py)))])
    assert arc[-1] > max(arcs)
    out = []
    for a in arcs:
        k = int(np.searchsorted(arc, a))
        h = ph[k]
        out.append(synth.pose_from_ypr([px[k] - lateral * np.sin(h), py[k] + lateral * np.cos(h), synth.SENSOR_H, h, 0.0, 0.0]))
    return np.array(out).reshape(-1, 12)


def moved(poses, M):
    """M . T for every pose"""
    return np.array([lc.to12(M @ lc.to44(T)) for T in poses])


@functools.lru_cache(maxsize=1)
def scenario():
    """dict(a_gt, a_est [46, 12], a_sweeps; b_gt [26, 12] (world), b_local [26, 12]: B's drifted poses from its own origin -- the
    recorded poses are moved(b_local, G) --, b_sweeps: 26 float32 [n, 3] arrays (32 rings x 600 azimuths at rest))"""
    s = lc.scenario()
    b_gt = poses_at(B_ARCS, B_LATERAL)
    rc = synth_city.Raycaster(synth_city.make_city(2024))
    b_sweeps = [np.ascontiguousarray(rc.sweep(T, np.zeros(6), rings=32, azimuths=600, seed=B_SEED + n)[0], np.float32) for n, T in enumerate(b_gt)]
    rc.close()
    b_local = lc.drifted(moved(b_gt, np.linalg.inv(lc.to44(b_gt[0]))))   # est_0 = the identity: B's own origin
    return dict(a_gt=s["gt"][:N_A], a_est=s["est"][:N_A], a_sweeps=s["sweeps"][:N_A], b_gt=b_gt, b_local=b_local, b_sweeps=b_sweeps)


def sessions(M=None):
    """(A, B) as the dicts host.join_sessions takes; B recorded in the frame M (default G)"""
    s = scenario()
    a = lc.keyframe_set(s["a_est"], s["a_sweeps"])
    b = lc.keyframe_set(moved(s["b_local"], G if M is None else M), s["b_sweeps"])
    for k, f in enumerate(b["frames"]):
        f["timestamp"] = 5000.0 + k
    return a, b
