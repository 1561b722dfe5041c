"""The scenarios of the live-map-cleaning tests (tests/test_live_cpu.py, tests/test_gpu_odometry_live.py).  Data generation and
book-keeping only (mola_lidar_odometry_amd.synth, tests/clean_cases.py); no product code.

  - the street: tests/clean_cases.scenario() -- 20 sweeps at rest, 3 m apart, exact poses, one car-sized mover per sweep.
  - drive(): a drive the odometry can track, along the street of synth.make_scene(4242, 120, 160) that the loop-closure drive of
    tests/loop_online_ref.py uses (a street of synth_city leaves the motion along it open at 32 x 600), at that drive's spacing:
    0.1 s between scans, up to 7.5 m/s (0.75 m per scan) after a ramp from rest over the first RAMP scans, as synth.make_drive
    starts its drives (the first alignments have no motion model to start from) -- every scan updates the local map.  The mover follows the rule of
    clean_cases: a car's body that begins CLEARANCE above the road, AHEAD of the vehicle in its lane for the first HALF scans, then
    crossing the street before the vehicle gets there; afterwards it has left the street.  Lane and crossing lie where the
    scene's boxes leave room: neither the vehicle nor the mover passes through one, and none is taken out (the odometry needs
    what stands beside and ahead of the lane to observe the motion along the street).  The drive goes on for 16 scans after
    the mover has left: the scans that followed the mover re-observed its trail, their views agree with it, and every erasing
    counts every kept view afresh, so a trail point goes only once those views have left the ring of 24 (with 36 scans the
    driver's own run kept 28 of 369 mover points, 7.6 %); it stops short of the kiosk that stands in the lane at x = -29.
  - Ledger: which stored points came from the mover.  A point is known by the bits of its world coordinates, which are those
    the map stores ((float)(R p + t) in float64, un-fused: clean_ref.transform)."""
import functools

import numpy as np

import clean_cases as cc
import clean_ref as cr
from mola_lidar_odometry_amd import synth

MAP_ARGS = (1.0, 20, 0, 0.0, 0.0, 4)   # oracle_c.Map arguments of clean_cases.MAP_PARAMS

# ---- the drive
N_SCANS, DT, SPEED, RAMP = 40, 0.1, 7.5, 8          # (40 scans: see the module's text)
START = (-60.0, 2.3)                                # a lane the scene's boxes leave free as far as the drive goes
AHEAD = 18.0
HALF = 18                                           # the mover is AHEAD during scans 0 .. HALF - 1
V = [SPEED * min(1.0, k / float(RAMP)) for k in range(N_SCANS)]          # the speed during scan k
X = [START[0] + DT * sum(V[:k]) for k in range(N_SCANS)]                 # the vehicle at the reference time of scan k
CROSS_X = -44.75                                    # where the scene's boxes leave the most room across the street ...
CROSS_Y = (-4.9, -1.0)                              # ... from the far side up to the vehicle's lane
CROSS_SCANS = 6                                     # the crossing takes scans HALF .. HALF + CROSS_SCANS - 1: the vehicle is 1.5 m short of it then


def drive_scene():
    return synth.make_scene(4242, 120.0, 160)


def drive_mover_box(k, x_vehicle):
    """[xmin, ymin, zmin, xmax, ymax, zmax] of the mover during scan k, or None once it has left the street"""
    l, w, h = cc.BOX
    if k < HALF:
        cx, cy, sx, sy = x_vehicle + AHEAD, START[1], l, w
    elif k < HALF + CROSS_SCANS:
        u = (k - HALF) / float(CROSS_SCANS - 1)
        cx, cy, sx, sy = CROSS_X, CROSS_Y[0] + u * (CROSS_Y[1] - CROSS_Y[0]), w, l
    else:
        return None
    return np.array([cx - sx / 2, cy - sy / 2, cc.CLEARANCE, cx + sx / 2, cy + sy / 2, h], np.float64)


@functools.lru_cache(maxsize=1)
def drive():
    """dict(scans [(xyz, t)], stamps, poses [n, 12] ground truth, twists [n, 6], boxes, mover: a bool mask per scan over its raw points)"""
    scene = drive_scene()
    poses, scans, stamps, boxes, mover, twists = [], [], [], [], [], []
    for k in range(N_SCANS):
        x = X[k]
        tw = np.array([V[k], 0.0, 0.0, 0.0, 0.0, 0.0])
        twists.append(tw)
        T = synth.pose_from_ypr([x, START[1], synth.SENSOR_H, 0.0, 0.0, 0.0])
        box = drive_mover_box(k, x)
        sc = scene if box is None else synth.Scene(scene.half_extent, scene.end_wall_x, np.concatenate([scene.boxes, box[None]], 0))
        xyz, t = synth.make_sweep(sc, T, tw, DT, 32, 600, 7000 + 10 * k)
        # where each return lies in the world: fired from the pose at its own firing time (pure translation along x)
        world = xyz.astype(np.float64) + np.array([x, START[1], synth.SENSOR_H]) + t.astype(np.float64)[:, None] * tw[None, :3]
        poses.append(np.asarray(T, np.float64).reshape(12))
        scans.append((xyz, t))
        stamps.append(3000.0 + k * DT)
        boxes.append(box)
        mover.append(np.zeros(len(xyz), bool) if box is None else cc.in_box(world, box, cc.INFLATE))
    return dict(scans=scans, stamps=stamps, poses=np.array(poses), twists=np.array(twists), boxes=boxes, mover=mover)


# ---- which stored points are the mover's
def _keys(xyz):
    a = np.ascontiguousarray(np.asarray(xyz, np.float32).reshape(-1, 3))
    return a.view(np.dtype((np.void, 12))).reshape(-1)


class Ledger:
    def __init__(self):
        self.mover = set()
        self.erased_mover = self.erased_other = 0

    def offered(self, scan_xyz, T, mask):
        """a scan about to be inserted at pose T; mask: its mover points"""
        world = cr.transform(T, scan_xyz)
        self.mover.update(k.tobytes() for k in _keys(world[np.asarray(mask, bool)]))

    def is_mover(self, map_xyz):
        return np.array([k.tobytes() in self.mover for k in _keys(map_xyz)], bool)

    def on_erase(self, map_xyz, drop):
        m = self.is_mover(map_xyz)
        self.erased_mover += int((drop & m).sum())
        self.erased_other += int((drop & ~m).sum())

    def tally(self, final_xyz):
        """(mover points left, other points left, other points erased, other points that ever were in the map)"""
        m = self.is_mover(final_xyz)
        left, others = int(m.sum()), int((~m).sum())
        return left, others, self.erased_other, others + self.erased_other


def fold(sweeps, poses, mover, host=None, params=None, clean=True):
    """the sweeps inserted at their poses into a map of MAP_ARGS, with (clean) or without the rule of LiveMapCleaning.h behind every
    insertion -> Ledger.tally of the final map"""
    import live_ref as lr
    led = Ledger()
    f = lr.LiveFold(MAP_ARGS, params, host, on_erase=led.on_erase)
    for xyz, T, m in zip(sweeps, poses, mover):
        led.offered(xyz, T, m)
        if clean:
            f.update(xyz, T)
        else:
            f.map.insert_posed(xyz, T, 0.0)
    return led.tally(f.map.dump()["xyz"]), f


def drive_deskewed():
    """the drive's sweeps de-skewed with the exact twists (what a driver that knew the truth would insert), poses, mover masks"""
    from oracle import oracle_c as oc
    d = drive()
    return [oc.deskew(xyz, t, tw) for (xyz, t), tw in zip(d["scans"], d["twists"])], d["poses"], d["mover"]
