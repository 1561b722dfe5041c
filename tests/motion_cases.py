"""The scenario of the gyro de-skew tests (tests/test_motion_cpu.py, tests/test_gpu_odometry_motion.py): data generation only, no
product code.

  - the room: a closed box of six planes, ROOM, with axis-aligned boxes standing in it (asymmetric, so that neither a rotation by
    pi nor a shift along a wall maps the room onto itself); rays are cast analytically (the slab test; from the inside the room
    is the far side of its own slab).
  - the sensor: 16 rings by 360 azimuths at 10 Hz, N_SCANS sweeps; azimuth column j fires at t_j = (j / 360 - 0.5) * DT relative
    to the scan's stamp, from the pose of that very moment -- every point lies in the sensor's frame AT ITS FIRING TIME (skewed).
  - the trajectory, closed form: the position walks a slow ellipse (below 1 m/s), the attitude is R(t) = Rz(yaw(t)) Ry(pitch(t))
    with yaw(t) = YAW_DRIFT t + YAW_A sin(2 pi YAW_F t), pitch(t) = PITCH_A sin(2 pi PITCH_F t + 1): rates that swing at 3.7 Hz
    and 5.3 Hz: inside every 0.1 s sweep the yaw rate swings by more than 1 rad/s and the pitch rate by more than 0.7 rad/s, and
    they change sign inside most sweeps, so no twist taken from two poses 0.1 s apart describes them (neither frequency is a
    multiple of 5 Hz: sampled at 10 Hz the swing does not vanish).
  - the gyro: the body rate of R(t), w = (-sin(pitch) yaw', pitch', cos(pitch) yaw'), sampled at 400 Hz from the same formula.
  - ground truth: the pose at stamp + TIME_ZERO, the moment FilterAdjustTimestamps(MiddleIsZero) calls zero -- the middle
    between the first and the last column's stamp, 0.5 * DT / 360 before the scan's stamp; the block's time_zero_offset.

The amplitudes are chosen so that the constant twist visibly fails: tests/test_motion_cpu.py holds the condition on the CPU with
the oracle alone (MotionOracle's ATE at most half of plain OdometryOracle's).  Measured there: plain 0.245 m, with the gyro 0.044 m
(ratio 0.18); the neighbouring amplitudes (yaw 0.06 .. 0.10 rad, pitch 0.02 .. 0.04 rad) gave ratios between 0.17 and 0.36."""
import functools

import numpy as np

ROOM = np.array([-9.0, -6.0, 0.0, 11.0, 7.0, 5.0])          # xmin, ymin, zmin, xmax, ymax, zmax
BOXES = np.array([[4.0, 3.5, 0.0, 6.5, 7.0, 2.2],            # a cupboard against the +y wall
                  [-9.0, -6.0, 0.0, -6.5, -2.0, 3.0],        # a block in the (-x, -y) corner
                  [2.0, -6.0, 0.0, 3.2, -4.2, 1.2],          # a desk at the -y wall
                  [-3.5, 2.8, 0.0, -2.3, 4.0, 5.0],          # a pillar
                  [8.0, -3.0, 0.0, 11.0, -1.0, 1.6],         # a bench at the +x wall
                  [-1.0, -2.6, 0.0, 0.2, -1.6, 0.9]])        # a crate near the middle
RINGS, AZIMUTHS, DT, N_SCANS, T0 = 16, 360, 0.1, 40, 500.0
EL_DEG = (30.0, -30.0)   # (a field of view that puts six rings on the floor and six on the ceiling: height, pitch and roll are observed)
GYRO_HZ = 400.0
TIME_ZERO = -0.5 * DT / AZIMUTHS
CENTER, AX, AY, HEIGHT, LOOP_S = np.array([0.5, 0.3]), 2.0, 1.2, 1.6, 14.0
YAW_DRIFT, YAW_A, YAW_F = 0.15, 0.08, 3.7
PITCH_A, PITCH_F, PITCH_PH = 0.02, 5.3, 1.0
RANGE_NOISE = 0.005

GYRO_BLOCK = "\ngyro_deskew:\n  enabled: true\n  time_zero_offset: %.17g\n" % TIME_ZERO
GYRO_OPTIONS = dict(time_zero_offset=TIME_ZERO)


def _rz(a):
    c, s, z, o = np.cos(a), np.sin(a), np.zeros_like(a), np.ones_like(a)
    return np.stack([np.stack([c, -s, z], -1), np.stack([s, c, z], -1), np.stack([z, z, o], -1)], -2)


def _ry(a):
    c, s, z, o = np.cos(a), np.sin(a), np.zeros_like(a), np.ones_like(a)
    return np.stack([np.stack([c, z, s], -1), np.stack([z, o, z], -1), np.stack([-s, z, c], -1)], -2)


def angles(t):
    """yaw, pitch and their rates at the (relative) times t"""
    t = np.asarray(t, np.float64)
    wy, wp = 2 * np.pi * YAW_F, 2 * np.pi * PITCH_F
    yaw = YAW_DRIFT * t + YAW_A * np.sin(wy * t)
    dyaw = YAW_DRIFT + YAW_A * wy * np.cos(wy * t)
    pitch = PITCH_A * np.sin(wp * t + PITCH_PH)
    dpitch = PITCH_A * wp * np.cos(wp * t + PITCH_PH)
    return yaw, pitch, dyaw, dpitch


def pose_at(t):
    """(R [..., 3, 3], p [..., 3]) at the times t [s] since T0"""
    t = np.asarray(t, np.float64)
    yaw, pitch, _, _ = angles(t)
    ph = 2 * np.pi * t / LOOP_S
    p = np.stack([CENTER[0] + AX * np.cos(ph), CENTER[1] + AY * np.sin(ph), HEIGHT + 0.0 * t], -1)
    return _rz(yaw) @ _ry(pitch), p


def body_rate(t):
    """the gyro's reading at the times t: R^T dR/dt of R = Rz(yaw) Ry(pitch), as a vector in the body frame"""
    _, pitch, dyaw, dpitch = angles(t)
    return np.stack([-np.sin(pitch) * dyaw, dpitch, np.cos(pitch) * dyaw], -1)


def raycast(o, d):
    """distance along each ray (origins o [n, 3] inside the room, unit directions d [n, 3]) to the first surface"""
    with np.errstate(divide="ignore", invalid="ignore"):
        t0, t1 = (ROOM[None, :3] - o) / d, (ROOM[None, 3:] - o) / d
        tmin = np.nanmin(np.maximum(t0, t1), axis=1)  # the room from the inside: where the ray leaves its slab
        for b in BOXES:
            t0, t1 = (b[None, :3] - o) / d, (b[None, 3:] - o) / d
            tn, tf = np.nanmax(np.minimum(t0, t1), axis=1), np.nanmin(np.maximum(t0, t1), axis=1)
            tmin = np.where((tf >= tn) & (tn > 1e-6), np.minimum(tmin, tn), tmin)
    return tmin


def sweep(k):
    """(xyz [n, 3] float32 in the sensor's frame at firing time, t [n] float32 relative to the scan's stamp), ring-major"""
    rng = np.random.Generator(np.random.PCG64(9000 + k))
    el = np.deg2rad(np.linspace(EL_DEG[0], EL_DEG[1], RINGS))
    az = np.linspace(-np.pi, np.pi, AZIMUTHS, endpoint=False)
    tcol = (np.arange(AZIMUTHS) / AZIMUTHS - 0.5) * DT
    E, A = np.meshgrid(el, az, indexing="ij")
    tt = np.broadcast_to(tcol[None, :], E.shape).reshape(-1)
    d_local = np.stack([np.cos(E) * np.cos(A), np.cos(E) * np.sin(A), np.sin(E)], -1).reshape(-1, 3)
    R, p = pose_at(k * DT + tt)
    rng_true = raycast(p, np.einsum("nij,nj->ni", R, d_local))
    assert np.isfinite(rng_true).all() and (rng_true > 0.2).all()
    r = rng_true + rng.normal(0.0, RANGE_NOISE, len(rng_true))
    return np.ascontiguousarray(d_local * r[:, None], np.float32), np.ascontiguousarray(tt, np.float32)


@functools.lru_cache(maxsize=1)
def drive():
    """dict(scans [(xyz, t)], stamps [n], poses [n, 12] ground truth at stamp + TIME_ZERO, gyro_t [m], gyro_w [m, 3])"""
    scans = [sweep(k) for k in range(N_SCANS)]
    stamps = T0 + DT * np.arange(N_SCANS)
    R, p = pose_at(DT * np.arange(N_SCANS) + TIME_ZERO)
    poses = np.concatenate([R, p[..., None]], -1).reshape(N_SCANS, 12)
    m = int(round((N_SCANS * DT + 0.4) * GYRO_HZ))
    rel = -0.2 + np.arange(m) / GYRO_HZ
    return dict(scans=scans, stamps=stamps, poses=poses, gyro_t=T0 + rel, gyro_w=body_rate(rel))


def gyro_until(d, t_end, start=0):
    """indices [start, stop) of the samples with time <= t_end: what a driver has received when the scan ending there arrives"""
    return start, int(np.searchsorted(d["gyro_t"], t_end, side="right"))


def gt_relative(d):
    """the ground-truth poses in the frame of the first one, [n, 4, 4]"""
    G = np.tile(np.eye(4), (len(d["poses"]), 1, 1))
    G[:, :3, :] = d["poses"].reshape(-1, 3, 4)
    return np.linalg.inv(G[0])[None] @ G


def ate(trajectory, d):
    """RMSE of the translation differences against the ground truth, both in the frame of their first pose, over the scans the
    trajectory holds (absolute trajectory error without alignment)"""
    stamps = np.array([t for t, _ in trajectory])
    idx = np.rint((stamps - T0) / DT).astype(int)
    E = np.tile(np.eye(4), (len(idx), 1, 1))
    E[:, :3, :] = np.array([np.asarray(p, np.float64).reshape(3, 4) for _, p in trajectory])
    G = gt_relative(d)[idx]
    return float(np.sqrt(np.mean(np.sum((E[:, :3, 3] - G[:, :3, 3]) ** 2, axis=1))))
