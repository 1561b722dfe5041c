"""What the multi-LiDAR tests share: the repository's default pipeline text with a rig's two parameter groups written into
its `params:` block (params.multiple_lidars, params.lidar_sensor_labels), optionally without its
observations_filter_adjust_timestamps block, and a synthetic rig: every sweep of a drive split by azimuth into the halves a
front and a rear LiDAR would see, each expressed in its own sensor frame.  No product code."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_BASE = os.path.join(ROOT, "pipelines", "lidar3d-default-hip.yaml")

FRONT, REAR = "lidar_a_front", "lidar_b_rear"  # byte-wise order: front before rear
LABELS_RE = "lidar_.*"
REAR_DELAY = 0.004  # [s] the rear sensor's clock: its observations are stamped this much later


def pipeline(lidar_count=1, max_time_offset=0.01, labels=LABELS_RE, adjust_timestamps=True, min_time_between_scans=None):
    """The default chain for a rig of `lidar_count` sensors.  labels: a regular expression, a list of them, or None (no key)."""
    text = open(_BASE).read()
    block = "  multiple_lidars:\n    lidar_count: %d\n    max_time_offset: %r\n" % (lidar_count, max_time_offset)
    if labels is not None:
        block += "  lidar_sensor_labels: %s\n" % ("'%s'" % labels if isinstance(labels, str) else "[%s]" % ", ".join("'%s'" % l for l in labels))
    head, n = re.subn(r"(?m)^params:\n", "params:\n" + block, text, count=1)
    assert n == 1
    if min_time_between_scans is not None:
        head, n = re.subn(r"(?m)^  min_time_between_scans:.*$", "  min_time_between_scans: %r" % min_time_between_scans, head, count=1)
        assert n == 1
    if not adjust_timestamps:
        head, n = re.subn(r"(?ms)^observations_filter_adjust_timestamps:\n.*?(?=^observations_filter_1st_pass:)", "", head, count=1)
        assert n == 1
    return head


def _pose(yaw_deg, xyz):
    c, s = np.cos(np.deg2rad(yaw_deg)), np.sin(np.deg2rad(yaw_deg))
    return np.array([[c, -s, 0.0, xyz[0]], [s, c, 0.0, xyz[1]], [0.0, 0.0, 1.0, xyz[2]]])


# the sensors on the vehicle: a yaw of tens of degrees and a lever arm of about a metre
POSE = {FRONT: _pose(25.0, (1.1, 0.2, 0.3)), REAR: _pose(-160.0, (-0.9, -0.15, 0.45))}


def to_sensor_frame(P, xyz):
    """Vehicle-frame points in the frame of the sensor mounted at P (3x4): R^T (p - t), float64, rounded to float32."""
    p = np.asarray(xyz, np.float64)
    d = p - P[:, 3]
    R = P[:, :3]
    return np.stack([R[0, c] * d[:, 0] + R[1, c] * d[:, 1] + R[2, c] * d[:, 2] for c in range(3)], 1).astype(np.float32)


def split(xyz, t):
    """One sweep (vehicle frame) as the rig sees it: {label: (xyz in the sensor frame, per-point stamps relative to THAT
    sensor's time stamp)}.  Front: the points ahead (x >= 0).  The rear sensor's stamp is REAR_DELAY later, so its per-point
    stamps are REAR_DELAY smaller."""
    ahead = xyz[:, 0] >= 0
    out = {}
    for label, m, delay in ((FRONT, ahead, 0.0), (REAR, ~ahead, REAR_DELAY)):
        out[label] = (to_sensor_frame(POSE[label], xyz[m]), (t[m].astype(np.float64) - delay).astype(np.float32))
    return out
