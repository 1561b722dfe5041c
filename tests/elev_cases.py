"""Cases for the tests of include/molahip_elevation.h and the traversability map (tests/test_elev_cpu.py, tests/test_gpu_elev.py):
seeded random key-frames, hand-made edge points, and one analytic outdoor scenario.  Frames are (xyz float32 [n, 3], T [12]) pairs.

THE SCENARIO.  Surfaces are sampled on a jittered lattice of pitch 0.1 m (jitter +-0.04 m, so every 0.2 m cell of a surface holds
exactly four samples of a view), seen from 12 poses 1.8 m above the surface they stand on and cut at 30 m; there is no ray caster,
so a surface under another one is sampled too.  The world frame is the one a recorded drive has: its origin is the first sensor
pose, so the road lies at z = -1.8 m.  Cell size 0.2 m; heights below are over the road:
    road      x in [0, 60],  y in [-4, 4],  0
    ramp      x in [60, 80], y in [-4, 4],  0.15 (x - 60): a 15 % ramp rising 3 m
    sidewalk  x in [0, 60],  y in [4, 6],   0.20: a 0.20 m kerb along y = 4
    box       x in [20, 21], y in [-0.6, 0.4], top at 1 and four side faces (0.01 m inside the footprint), on the road
    deck      x in [35, 45], y in [-4, 4],  4: 4 m above a stretch of road
What the geometry gives (SCENARIO_OPTIONS: slope window of one cell, so that one cell inside a region no window reaches across its
border): heights over the road in quanta of 0.01 m are road {-1, 0}, sidewalk {19, 20}, box top {99, 100}, deck about 400
(rounding of the fp32 round trip through the vehicle frame); the stored heights are these minus 180.  Road, sidewalk: flat,
relief <= 1.  Ramp: the ground of cell column i is floor(3 i + 15 d), d in [0.01, 0.09] the offset of its lowest sample: 3 i or
3 i + 1, so three columns differ by at most 7 = rise_q = floor(tan(20 deg) * 0.2 / 0.01) and by far less than step_q = 15: free.  The kerb: the rows on either side of y = 4 differ
by at least 19 > step_q: lethal.  The box: its top stands 99 or more over the road under it, above step_q = 15 and below
clearance_q = 200: obstacle points, lethal.  The deck: 400 > clearance_q: overhead, the road under it is free."""
import functools

import numpy as np

F = np.float32
RES = 0.2
I12 = np.eye(4)[:3].reshape(12)


def pose(x=0.0, y=0.0, z=0.0, yaw=0.0):
    c, s = np.cos(yaw), np.sin(yaw)
    return np.array([c, -s, 0, x, s, c, 0, y, 0, 0, 1, z], np.float64)


def random_frames(sizes, seed, reach=3.0, spread=1.0, height=3.0):
    """One frame per entry of `sizes`: points within `reach` of the vehicle and `height` above or below it, poses scattered by `spread`."""
    rng = np.random.default_rng(seed)
    out = []
    for n in sizes:
        xyz = rng.uniform(-reach, reach, (n, 3)).astype(F)
        xyz[:, 2] *= height / reach
        out.append((xyz, pose(*rng.uniform(-spread, spread, 3) * np.array([1, 1, 0.2]), yaw=rng.uniform(-np.pi, np.pi))))
    return out


def window_of(frames, resolution=RES, margin=0):
    """(x0, y0, nx, ny) that holds every finite point of the frames less than 10 km from the origin (computed in fp64: a margin of
    one cell covers the rounding); a negative margin cuts points off on every side"""
    with np.errstate(all="ignore"):
        pts = np.concatenate([np.asarray(x, np.float64).reshape(-1, 3) @ np.asarray(T).reshape(3, 4)[:, :3].T + np.asarray(T).reshape(3, 4)[:, 3]
                              for x, T in frames if len(x)])
        pts = pts[np.isfinite(pts).all(axis=1) & (np.abs(pts) < 1.0e4).all(axis=1)]
    lo = np.floor(pts[:, :2].min(axis=0) / resolution).astype(int) - 1 - margin
    hi = np.floor(pts[:, :2].max(axis=0) / resolution).astype(int) + 1 + margin
    return int(lo[0]), int(lo[1]), int(hi[0] - lo[0] + 1), int(hi[1] - lo[1] + 1)


def edge_points(resolution=RES, z_quantum=0.01):
    """Points exactly on cell edges and on height-quantum edges as fp32 computes them (k * resolution, k * z_quantum in fp32), and one
    ulp to either side, under the identity pose."""
    out = []
    for k in (-3, -1, 0, 1, 2, 7):
        for j in (-2, 0, 5):
            x, y, z = F(k) * F(resolution), F(j) * F(resolution), F(k * 3 + j) * F(z_quantum)
            for d in (-1, 0, 1):
                step = lambda v: np.nextafter(v, F(np.inf) * F(d)) if d else v
                out.append((step(x), step(y), step(z)))
    return [(np.array(out, F), I12.copy())]


def height_steps(step_q=15, clearance_q=200, z_quantum=0.01):
    """Two cells: a ground point at height 0 in each, then points at exactly h = step_q, step_q + 1, clearance_q and clearance_q + 1
    quanta (mid-quantum, so that fp32 rounding cannot move them)."""
    q = z_quantum
    pts = [(0.1, 0.1, 0.5 * q), (0.3, 0.1, 0.5 * q)]
    pts += [(0.1, 0.1, (step_q + 0.5) * q), (0.3, 0.1, (step_q + 1.5) * q), (0.1, 0.1, (clearance_q + 0.5) * q), (0.3, 0.1, (clearance_q + 1.5) * q)]
    return [(np.array(pts, F), I12.copy())]


def wild_frames(seed=5):
    """Frames with non-finite points, points outside the index range (|p / resolution| >= 1e6) and heights outside the quantum range
    (|z / z_quantum| >= 2^30) among good ones."""
    out = random_frames([65, 64, 33], seed)
    for k, (xyz, T) in enumerate(out):
        xyz[3] = (np.nan, 0.1, 0.1)
        xyz[7] = (0.2, np.inf, 0.0)
        xyz[9] = (0.2, 0.1, -np.inf)
        xyz[11 + k] = (2.4e5, 0.0, 0.0)
        xyz[20] = (0.0, -2.8e5, 1.0)
        xyz[25] = (0.5, 0.5, 1.2e7)      # |z / 0.01| >= 2^30: left out by the passes, inside for the bounds
    return out


# ---- the scenario -------------------------------------------------------------------------------------------------------------------
PITCH, JITTER, RANGE, SENSOR_HEIGHT, N_POSES = 0.1, 0.04, 30.0, 1.8, 12
ROAD_Z = -SENSOR_HEIGHT      # the world frame's origin is the first sensor pose
ROAD_Q = -180                # ... in quanta of 0.01 m
SCENARIO_OPTIONS = "traversability:\n  slope_radius_cells: 1\n"
SCENARIO_OPTIONS_DICT = dict(slope_radius_cells=1)
BOX = (20.0, 21.0, -0.6, 0.4, 1.0)
DECK = (35.0, 45.0, -4.0, 4.0, 4.0)


def _lattice(rng, u0, u1, v0, v1):
    """jittered lattice over [u0, u1] x [v0, v1]: one sample per PITCH x PITCH square, JITTER around its centre"""
    nu, nv = int(round((u1 - u0) / PITCH)), int(round((v1 - v0) / PITCH))
    u = u0 + (np.arange(nu) + 0.5) * PITCH
    v = v0 + (np.arange(nv) + 0.5) * PITCH
    U, V = np.meshgrid(u, v, indexing="ij")
    return (U + rng.uniform(-JITTER, JITTER, U.shape)).ravel(), (V + rng.uniform(-JITTER, JITTER, V.shape)).ravel()


def surface_height(x):
    """the height of road and ramp at x, world frame"""
    return ROAD_Z + np.where(x > 60.0, 0.15 * (x - 60.0), 0.0)


def scenario_world(seed=14):
    """float64 [n, 3]: the samples of every surface in the world frame"""
    rng = np.random.default_rng(seed)
    parts = []
    x, y = _lattice(rng, 0.0, 80.0, -4.0, 4.0)                  # road and ramp
    parts.append(np.stack([x, y, surface_height(x)], axis=1))
    x, y = _lattice(rng, 0.0, 60.0, 4.0, 6.0)                   # sidewalk
    parts.append(np.stack([x, y, np.full_like(x, ROAD_Z + 0.20)], axis=1))
    bx0, bx1, by0, by1, bh = BOX
    x, y = _lattice(rng, bx0, bx1, by0, by1)                    # box: top
    parts.append(np.stack([x, y, np.full_like(x, ROAD_Z + bh)], axis=1))
    e = 0.01
    for fixed, axis in ((bx0 + e, 0), (bx1 - e, 0), (by0 + e, 1), (by1 - e, 1)):   # ... and side faces
        lo, hi = (by0, by1) if axis == 0 else (bx0, bx1)
        u, z = _lattice(rng, lo, hi, ROAD_Z, ROAD_Z + bh)
        parts.append(np.stack([np.full_like(u, fixed), u, z], axis=1) if axis == 0 else np.stack([u, np.full_like(u, fixed), z], axis=1))
    x, y = _lattice(rng, *DECK[:4])                             # deck
    parts.append(np.stack([x, y, np.full_like(x, ROAD_Z + DECK[4])], axis=1))
    return np.concatenate(parts)


def scenario_poses():
    xs = 3.0 + 6.5 * np.arange(N_POSES)
    return [pose(x, 0.3 * np.sin(k), float(surface_height(x)) + SENSOR_HEIGHT, yaw=0.05 * np.cos(2.0 * k)) for k, x in enumerate(xs)]


@functools.lru_cache(maxsize=1)
def scenario():
    """(frames as (xyz, T) pairs, the key-frame set as the dict the host takes)"""
    world = scenario_world()
    frames = []
    for T in scenario_poses():
        M = T.reshape(3, 4)
        seen = world[np.linalg.norm(world - M[:, 3], axis=1) <= RANGE]
        frames.append((np.ascontiguousarray(((seen - M[:, 3]) @ M[:, :3]).astype(F)), T))      # R^T (p - t)
    params = dict(voxel_size=1.0, max_points_per_voxel=20, index_mode=0, min_distance_between_points=0.0, ndt_max_eigen_ratio=0.0,
                  ndt_min_points=0, far_voxel_metric=0)
    kfset = dict(maps=[dict(name="localmap", class_name="HashedVoxelPointCloud", params=params, remove_voxels_farther_than=0.0)],
                 frames=[dict(timestamp=100.0 + k, pose=T.tolist(), cov=[0.0] * 36, twist=None, layers=[(0, xyz)])
                         for k, (xyz, T) in enumerate(frames)])
    return frames, kfset


def scenario_regions(g):
    """name -> (bool mask [ny, nx] of the cells at least one cell inside the region, the class the geometry gives: 'free' or 'lethal').
    Cells are addressed by their index: column i covers x in [0.2 i, 0.2 (i + 1))."""
    ix = g["x0"] + np.arange(g["nx"])[None, :]
    iy = g["y0"] + np.arange(g["ny"])[:, None]
    c = lambda v: int(round(v / RES))                            # the cell whose low edge is v
    rect = lambda x0, x1, y0, y1: (ix >= c(x0) + 1) & (ix <= c(x1) - 2) & (iy >= c(y0) + 1) & (iy <= c(y1) - 2)
    bx0, bx1, by0, by1, _ = BOX
    near_box = (ix >= c(bx0) - 1) & (ix <= c(bx1)) & (iy >= c(by0) - 1) & (iy <= c(by1))   # the box and the ring of road cells around it
    road = rect(0.0, 60.0, -4.0, 4.0) & ~near_box
    under_deck = rect(*DECK[:4])
    return dict(road=(road & ~under_deck, "free"), under_deck=(under_deck, "free"), ramp=(rect(60.0, 80.0, -4.0, 4.0), "free"),
                sidewalk=(rect(0.0, 60.0, 4.0, 6.0), "free"), box=(rect(bx0, bx1, by0, by1), "lethal"),
                kerb=((ix >= c(0.0) + 1) & (ix <= c(60.0) - 2) & ((iy == c(4.0) - 1) | (iy == c(4.0))), "lethal"))


def scenario_disagreement(g):
    """name -> (interior cells, of which not of the class the geometry gives); g holds `cost` [ny, nx] and the window"""
    cost = np.asarray(g["cost"])
    out = {}
    for name, (mask, want) in scenario_regions(g).items():
        got = np.where(cost[mask] == 254, "lethal", np.where(cost[mask] == 255, "unknown", "free"))
        out[name] = (int(mask.sum()), int((got != want).sum()))
    return out


def ramp_in_band(g, z_lo=0.0, z_hi=1.15):
    """bool mask [ny, nx] over a grid with window x0, y0, nx, ny at cell size RES: interior ramp cells whose surface lies wholly
    between the world heights z_lo and z_hi -- inside the default height band (-0.10 .. 1.50 m) of the occupancy grid"""
    ix = g["x0"] + np.arange(g["nx"])[None, :]
    iy = g["y0"] + np.arange(g["ny"])[:, None]
    x_lo, x_hi = 60.0 + (z_lo - ROAD_Z) / 0.15, 60.0 + (z_hi - ROAD_Z) / 0.15
    return (ix * RES >= x_lo) & ((ix + 1) * RES <= x_hi) & (iy >= int(round(-4.0 / RES)) + 1) & (iy <= int(round(4.0 / RES)) - 2)
