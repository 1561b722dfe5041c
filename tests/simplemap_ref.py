"""The key-frame rule of the session's key-frame store (params.simplemap), restated in numpy: a pure function of the scans'
poses, their icp_good flags and the two limits of every scan.  Scans that never reached registration (dropped, waiting,
ignored) are not passed in."""
import numpy as np


def _rel(p, q):
    """(translation norm, rotation angle [rad]) of p relative to q; poses are 12 values, row-major [R|t]"""
    P, Q = np.asarray(p, float).reshape(3, 4), np.asarray(q, float).reshape(3, 4)
    R = Q[:, :3].T @ P[:, :3]
    w = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    return float(np.linalg.norm(P[:, 3] - Q[:, 3])), float(np.arctan2(np.linalg.norm(w), 0.5 * (np.trace(R) - 1.0)))


def decide(poses, icp_good, min_translation, min_rotation_deg, measure_from_last_kf_only=False, add_non_keyframes_too=False,
           first_scan=None):
    """-> (stored [n] bool, keyframe [n] bool).  first_scan: the scans that became the map without an ICP (default: scan 0
    only); they are key-frames and do not enter the checker.  A good scan is a key-frame iff the checker is empty, or its
    translation or rotation from the closest (by translation) or the last key-frame in the checker exceeds its limits."""
    n = len(poses)
    first = np.zeros(n, bool) if first_scan is None else np.asarray(first_scan, bool)
    if first_scan is None and n:
        first[0] = True
    lim_t, lim_r = np.broadcast_to(min_translation, (n,)), np.deg2rad(np.broadcast_to(min_rotation_deg, (n,)))
    stored, keyframe, checker = np.zeros(n, bool), np.zeros(n, bool), []
    for k in range(n):
        if first[k]:
            stored[k] = keyframe[k] = True
            continue
        if not icp_good[k]:
            continue
        if not checker:
            enough = True
        else:
            ref = checker[-1] if measure_from_last_kf_only else min(checker, key=lambda q: _rel(poses[k], q)[0])
            d, a = _rel(poses[k], ref)
            enough = d > lim_t[k] or a > lim_r[k]
        keyframe[k] = enough
        stored[k] = enough or add_non_keyframes_too
        if enough:
            checker.append(poses[k])
    return stored, keyframe
