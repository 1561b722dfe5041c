"""mh_score_poses (include/molahip.h) restated on the CPU oracle, the candidate grid of a relocalization restated in numpy, and
the inputs their tests share.

Per candidate pose the oracle's matcher (oracle_c.match_points: Matcher_Points_DistanceThreshold over the oracle's own map)
gives the accepted pairs and their fp32 d2; n_paired is their number, and the cost is the integer sum of
q = (d2 * qscale >= 16777215) ? 0xFFFFFF : trunc(d2 * qscale) with qscale = (float)(2^20 / (double)(float)(thr^2)), computed in
numpy float32 (un-fused).  No product code."""
import math

import numpy as np

from mola_lidar_odometry_amd import synth

F = np.float32
SCORE_DTYPE = np.dtype([("n_paired", np.uint32), ("reserved_", np.uint32), ("cost", np.uint64)])


def qscale_of(threshold):
    thr2 = F(np.float64(threshold) * np.float64(threshold))
    return F(np.float64(1048576.0) / np.float64(thr2))


def quantise(d2, threshold):
    """q of every accepted d2 (uint64 array)"""
    with np.errstate(over="ignore"):
        qs = np.asarray(d2, F) * qscale_of(threshold)
    sat = qs >= F(16777215.0)
    return np.where(sat, np.uint64(0xFFFFFF), np.where(sat, F(0), qs).astype(np.uint64))


def score_poses(oracle_c, omap, scan_xyz, poses, threshold, threshold_angular_deg=0.0):
    """omap: an oracle_c.Map.  Returns a structured array like capi.score_poses'.  (oracle_c.match_points, called through the
    oracle's C entry point with the arrays allocated once: a reference over 70 000 candidates stays a matter of a second.)"""
    import ctypes as C
    P = np.ascontiguousarray(np.asarray(poses, np.float64).reshape(-1, 12))
    out = np.zeros(len(P), SCORE_DTYPE)
    l = np.asarray(scan_xyz, F).reshape(-1, 3)
    n = len(l)
    if n == 0:
        return out
    lx, ly, lz = (np.ascontiguousarray(l[:, a]) for a in range(3))
    li, gi = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    gx, gy, gz, d2 = (np.zeros(n, F) for _ in range(4))
    fp, up = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    args_in = [a.ctypes.data_as(fp) for a in (lx, ly, lz)]
    args_out = [li.ctypes.data_as(up), gi.ctypes.data_as(up)] + [a.ctypes.data_as(fp) for a in (gx, gy, gz, d2)]
    st = oracle_c._MatchStats()
    fn = oracle_c.lib().orc_match_points
    threads = min(8, oracle_c.max_threads()) if n >= 1000 else 1
    base = P.ctypes.data
    for c in range(len(P)):
        k = fn(omap._h, *args_in, n, C.cast(base + 96 * c, C.POINTER(C.c_double)), float(threshold), float(threshold_angular_deg),
               *args_out, C.byref(st), threads)
        out["n_paired"][c] = k
        out["cost"][c] = quantise(d2[:k], threshold).sum(dtype=np.uint64)
    return out


def reduce_pairs(d2, threshold):
    """(n_paired, cost) of one candidate from the accepted d2 of any matcher"""
    return len(d2), int(quantise(d2, threshold).sum(dtype=np.uint64))


def same(got, ref):
    """None, or what differs (bit for bit)"""
    if len(got) != len(ref):
        return f"length {len(got)} != {len(ref)}"
    for f in ("n_paired", "cost", "reserved_"):
        bad = np.flatnonzero(np.asarray(got[f]) != np.asarray(ref[f]))
        if len(bad):
            c = int(bad[0])
            return f"{f}: {len(bad)} of {len(ref)} candidates differ, first #{c}: got {got[f][c]}, reference {ref[f][c]}"
    return None


def rank(scores):
    """candidate indices by (n_paired descending, cost ascending, index ascending)"""
    n = len(scores)
    return np.lexsort((np.arange(n), scores["cost"].astype(np.uint64), -scores["n_paired"].astype(np.int64)))


# ---- the candidate grid --------------------------------------------------------------------------------------------------------
def axis_nodes(var, step, sigmas):
    """n = 2 * ceil(sigmas * sigma / step) + 1 nodes at (i - (n - 1) / 2) * step, sigma = sqrt of the axis' variance"""
    n = 2 * int(math.ceil(sigmas * math.sqrt(var) / step)) + 1
    return [(i - (n - 1) / 2) * step for i in range(n)]


def grid_cov(sigma_x, sigma_y, sigma_yaw):
    """a 6x6 covariance in (x, y, z, yaw, pitch, roll) order with these standard deviations on its diagonal"""
    c = np.zeros((6, 6))
    c[0, 0], c[1, 1], c[3, 3] = sigma_x * sigma_x, sigma_y * sigma_y, sigma_yaw * sigma_yaw
    return c.reshape(36)


def relocalization_grid(mean_ypr, cov, step_xy, step_yaw, sigmas=3.0):
    """Poses [k, 12] and the TPose3D rows [k, 6] of the grid over (x, y, yaw) around mean_ypr = (x, y, z, yaw, pitch, roll)
    [m, rad] with the 6x6 covariance `cov` (only its x, y and yaw diagonal entries are read): x outer, y middle, yaw inner;
    offsets are added to the mean's fields."""
    mean = [float(v) for v in mean_ypr]
    cov = np.asarray(cov, np.float64).reshape(36)
    rows = []
    for dx in axis_nodes(cov[0], step_xy, sigmas):
        for dy in axis_nodes(cov[7], step_xy, sigmas):
            for dyaw in axis_nodes(cov[21], step_yaw, sigmas):
                rows.append([mean[0] + dx, mean[1] + dy, mean[2], mean[3] + dyaw, mean[4], mean[5]])
    rows = np.array(rows, np.float64).reshape(-1, 6)
    return np.array([synth.pose_from_ypr(r) for r in rows]).reshape(-1, 12), rows


# ---- shared inputs ---------------------------------------------------------------------------------------------------------------
THRESHOLD = 0.5
STEP_XY, STEP_YAW = 0.5, np.deg2rad(3.0)
MEAN_OFFSET = np.array([1.3, -0.8, 0.0, np.deg2rad(5.0), 0.0, 0.0])


def small_grid(w):
    """13 x 13 x 9 = 1521 candidates around a mean 1.3 m / -0.8 m / 5 deg off the truth of synth.workload_small()"""
    return relocalization_grid(w.pose_gt_ypr + MEAN_OFFSET, grid_cov(1.0, 1.0, np.deg2rad(4.0)), STEP_XY, STEP_YAW, 3.0)


def pose(yaw=0.3, t=(0.31, -0.27, 0.12)):
    return synth.pose_from_ypr([t[0], t[1], t[2], yaw, -0.1, 0.05])


def cube_points(n=3000, seed=20261019, lo=-3.0, hi=3.0):
    return np.random.default_rng(seed).uniform(lo, hi, (n, 3)).astype(F)


def cube_scan(n, seed=7):
    return np.random.default_rng(seed).uniform(-3.5, 3.5, (n, 3)).astype(F)


def cube_poses(k, seed=5):
    """k poses near the identity: the scan stays over the map, every pose different"""
    rng = np.random.default_rng(seed)
    rows = np.zeros((k, 6))
    rows[:, :3] = rng.uniform(-0.6, 0.6, (k, 3))
    rows[:, 3:] = rng.uniform(-0.2, 0.2, (k, 3))
    return np.array([synth.pose_from_ypr(r) for r in rows]).reshape(-1, 12)


def dense_points():
    """five neighbouring voxels with 300 records each (uncapped): runs longer than the 31 records an indexed voxel can have"""
    rng = np.random.default_rng(3)
    corners = [[0, 0, 0], [0, 0, 1], [0, 0, 2], [1, 0, 0], [2, 0, 0]]
    return np.concatenate([rng.uniform(0.01, 0.99, (300, 3)) + np.array(c, np.float64) for c in corners]).astype(F)
