"""A numpy restatement of include/molahip_elevation.h and of the host rule of mola_lidar_odometry_hip/Traversability.h: the point
rule (composition in fp64 rounded to float, the range test, the cell and height indices in fp32), the index bounds, the two point
passes, the relief stencil, the classification, the window and the bytes of the four files.  Written from the headers' text.  No
product code."""
import math

import numpy as np

F = np.float32
NONE = -(1 << 31)                  # MH_ELEV_NONE
GROUND_EMPTY = (1 << 31) - 1
TOP_EMPTY = -(1 << 31)
UNKNOWN, LETHAL = 255, 254         # cost bytes
PGM_OCCUPIED, PGM_FREE, PGM_UNKNOWN = 0, 254, 205

DEFAULTS = dict(resolution=0.20, z_quantum=0.01, max_range=0.0, vehicle_height=2.0, max_step=0.15, slope_radius_cells=2,
                max_slope_deg=20.0, min_points_per_cell=2, min_obstacle_points=2, target_map="", margin_cells=2)


def compose(xyz, T):
    """Step 0: (float)(((T0*px + T1*py) + T2*pz) + T3) per row in fp64, rounded to float once."""
    p = np.asarray(xyz, F).reshape(-1, 3).astype(np.float64)
    T = np.asarray(T, np.float64).reshape(3, 4)
    with np.errstate(all="ignore"):
        return np.stack([((T[r, 0] * p[:, 0] + T[r, 1] * p[:, 1]) + T[r, 2] * p[:, 2]) + T[r, 3] for r in range(3)], axis=1).astype(F)


def point_rule(xyz, T, resolution, z_quantum, max_range, use_z=True):
    """Steps 0 to 3 for one frame: (passes bool [n], ix, iy, zq as int64 [n]; entries of points that do not pass are 0)."""
    P = compose(xyz, T)
    T = np.asarray(T, np.float64).reshape(3, 4)
    inv, invq = F(1.0) / F(resolution), F(1.0) / F(z_quantum if use_z else 1.0)
    with np.errstate(all="ignore"):
        ok = np.isfinite(P).all(axis=1)
        if max_range > 0:
            d = P - T[:, 3].astype(F)[None, :]
            d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            assert d2.dtype == F
            ok &= ~(d2 > F(max_range) * F(max_range))
        sx, sy, sz = P[:, 0] * inv, P[:, 1] * inv, P[:, 2] * invq
        assert sx.dtype == F and sz.dtype == F
        ok &= (np.abs(sx) < F(1.0e6)) & (np.abs(sy) < F(1.0e6))
        if use_z:
            ok &= np.abs(sz) < F(1073741824.0)
        ix = np.where(ok, np.floor(np.where(ok, sx, 0)), 0).astype(np.int64)
        iy = np.where(ok, np.floor(np.where(ok, sy, 0)), 0).astype(np.int64)
        zq = np.where(ok, np.floor(np.where(ok, sz, 0)), 0).astype(np.int64) if use_z else np.zeros(len(P), np.int64)
    return ok, ix, iy, zq


def bounds(frames, resolution, max_range=0.0):
    """mh_elev_bounds_frames: (lo [2], hi [2], n_in); lo / hi None when nothing passes."""
    lo, hi, n_in = None, None, 0
    for xyz, T in frames:
        ok, ix, iy, _ = point_rule(xyz, T, resolution, 1.0, max_range, use_z=False)
        if ok.any():
            a = np.array([ix[ok].min(), iy[ok].min()])
            b = np.array([ix[ok].max(), iy[ok].max()])
            lo = a if lo is None else np.minimum(lo, a)
            hi = b if hi is None else np.maximum(hi, b)
            n_in += int(ok.sum())
    return lo, hi, n_in


class ElevRef:
    def __init__(self, resolution=0.2, z_quantum=0.01, max_range=0.0, x0=0, y0=0, nx=1, ny=1, clearance_q=200, step_q=15):
        self.p = dict(resolution=resolution, z_quantum=z_quantum, max_range=max_range)
        self.x0, self.y0, self.nx, self.ny, self.clearance_q, self.step_q = x0, y0, nx, ny, clearance_q, step_q
        self.clear()

    def clear(self):
        self.ground = np.full((self.ny, self.nx), GROUND_EMPTY, np.int64)
        self.top = np.full((self.ny, self.nx), TOP_EMPTY, np.int64)
        self.count = np.zeros((self.ny, self.nx), np.int64)
        self.obstacle = np.zeros((self.ny, self.nx), np.int64)
        self.info = dict(n_offered=0, n_counted=0, n_left_out=0, n_outside_window=0, n_mark_offered=0, n_mark_left_out=0,
                         n_mark_outside_window=0, ground_frozen=0)

    def _kept(self, xyz, T):
        ok, ix, iy, zq = point_rule(xyz, T, **self.p)
        cx, cy = ix - self.x0, iy - self.y0
        inside = ok & (cx >= 0) & (cx < self.nx) & (cy >= 0) & (cy < self.ny)
        return int((~ok).sum()), int((ok & ~inside).sum()), cx[inside], cy[inside], zq[inside]

    def add_frames(self, frames):
        for xyz, T in frames:
            left, outside, cx, cy, zq = self._kept(xyz, T)
            np.minimum.at(self.ground, (cy, cx), zq)
            np.add.at(self.count, (cy, cx), 1)
            self.info["n_offered"] += len(xyz)
            self.info["n_left_out"] += left
            self.info["n_outside_window"] += outside
            self.info["n_counted"] += len(zq)
        return self

    def mark_frames(self, frames):
        for xyz, T in frames:
            left, outside, cx, cy, zq = self._kept(xyz, T)
            h = zq - self.ground[cy, cx]
            low = h <= self.clearance_q
            np.maximum.at(self.top, (cy[low], cx[low]), zq[low])
            obs = low & (h > self.step_q)
            np.add.at(self.obstacle, (cy[obs], cx[obs]), 1)
            self.info["n_mark_offered"] += len(xyz)
            self.info["n_mark_left_out"] += left
            self.info["n_mark_outside_window"] += outside
            if len(xyz):
                self.info["ground_frozen"] = 1
        return self

    def relief(self, radius, min_points):
        return relief(self.ground, self.count, radius, min_points)

    def download(self):
        return self.ground.astype(np.int32), self.count.astype(np.uint32), self.obstacle.astype(np.uint32), self.top.astype(np.int32)


def relief(ground, count, radius, min_points):
    """int32 [ny, nx]: separable windowed max - min of `ground` over the known cells; NONE where the cell itself is not known."""
    ground, count = np.asarray(ground, np.int64), np.asarray(count, np.int64)
    ny, nx = ground.shape
    known = count >= min_points
    lo = np.where(known, ground, GROUND_EMPTY)
    hi = np.where(known, ground, TOP_EMPTY)
    plo = np.full((ny + 2 * radius, nx + 2 * radius), GROUND_EMPTY, np.int64)
    phi = np.full((ny + 2 * radius, nx + 2 * radius), TOP_EMPTY, np.int64)
    plo[radius:radius + ny, radius:radius + nx] = lo
    phi[radius:radius + ny, radius:radius + nx] = hi
    mn, mx = lo.copy(), hi.copy()
    for dy in range(2 * radius + 1):
        for dx in range(2 * radius + 1):
            mn = np.minimum(mn, plo[dy:dy + ny, dx:dx + nx])
            mx = np.maximum(mx, phi[dy:dy + ny, dx:dx + nx])
    return np.where(known, mx - mn, NONE).astype(np.int32)


def relief_brute(ground, count, radius, min_points):
    """The same by the definition's double loop (for the restatement's own test)."""
    ground, count = np.asarray(ground, np.int64), np.asarray(count, np.int64)
    ny, nx = ground.shape
    out = np.full((ny, nx), NONE, np.int64)
    for r in range(ny):
        for c in range(nx):
            if count[r, c] < min_points:
                continue
            vals = [ground[rr, cc] for rr in range(max(0, r - radius), min(ny, r + radius + 1))
                    for cc in range(max(0, c - radius), min(nx, c + radius + 1)) if count[rr, cc] >= min_points]
            out[r, c] = max(vals) - min(vals)
    return out.astype(np.int32)


# ---- the host rule ------------------------------------------------------------------------------------------------------------------
def derived(opt):
    """(clearance_q, step_q, rise_q): floor(v / z_quantum) in fp64."""
    q = float(opt["z_quantum"])
    clearance_q = int(math.floor(float(opt["vehicle_height"]) / q))
    step_q = int(math.floor(float(opt["max_step"]) / q))
    rise_q = int(math.floor(math.tan(float(opt["max_slope_deg"]) * math.pi / 180.0) * opt["slope_radius_cells"] * float(opt["resolution"]) / q))
    return clearance_q, step_q, rise_q


def classify(count, obstacle, relief1, reliefR, step_q, rise_q, min_points, min_obstacle_points):
    """uint8 cost [ny, nx]: UNKNOWN, LETHAL, or max(252 * relief1 // (step_q + 1), 252 * reliefR // (rise_q + 1))."""
    count, obstacle = np.asarray(count, np.int64), np.asarray(obstacle, np.int64)
    r1, rR = np.asarray(relief1, np.int64), np.asarray(reliefR, np.int64)
    known = count >= min_points
    lethal = known & ((obstacle >= min_obstacle_points) | (r1 > step_q) | (rR > rise_q))
    cost = np.maximum(252 * np.where(known, r1, 0) // (step_q + 1), 252 * np.where(known, rR, 0) // (rise_q + 1))
    return np.where(~known, UNKNOWN, np.where(lethal, LETHAL, cost)).astype(np.uint8)


def window(lo, hi, margin_cells):
    return (int(lo[0]) - margin_cells, int(lo[1]) - margin_cells, int(hi[0]) - int(lo[0]) + 1 + 2 * margin_cells,
            int(hi[1]) - int(lo[1]) + 1 + 2 * margin_cells)


def build(frames, **options):
    """The whole path on (xyz, T) frames, in the order of build_traversability_map.  Returns a dict with the keys of the host's map."""
    opt = dict(DEFAULTS, **options)
    clearance_q, step_q, rise_q = derived(opt)
    lo, hi, n_in = bounds(frames, opt["resolution"], opt["max_range"])
    x0, y0, nx, ny = window(lo, hi, opt["margin_cells"])
    m = ElevRef(opt["resolution"], opt["z_quantum"], opt["max_range"], x0, y0, nx, ny, clearance_q, step_q)
    m.add_frames(frames).mark_frames(frames)
    r1, rR = m.relief(1, opt["min_points_per_cell"]), m.relief(opt["slope_radius_cells"], opt["min_points_per_cell"])
    ground, count, obstacle, top = m.download()
    cost = classify(count, obstacle, r1, rR, step_q, rise_q, opt["min_points_per_cell"], opt["min_obstacle_points"])
    return dict(x0=x0, y0=y0, nx=nx, ny=ny, resolution=opt["resolution"], z_quantum=opt["z_quantum"], clearance_q=clearance_q, step_q=step_q,
                rise_q=rise_q, ground=ground, count=count, obstacle_count=obstacle, top=top, relief1=r1, reliefR=rR, cost=cost,
                cells_lethal=int((cost == LETHAL).sum()), cells_unknown=int((cost == UNKNOWN).sum()),
                cells_free=int((cost < LETHAL).sum()), points_in=n_in, info=dict(m.info))


# ---- the files ----------------------------------------------------------------------------------------------------------------------
def trinary_pgm_bytes(cost):
    """prefix.pgm: g12's trinary image: lethal = occupied (0), known and not lethal = free (254), unknown = 205; row 0 = largest y."""
    cost = np.asarray(cost, np.uint8)
    ny, nx = cost.shape
    px = np.where(cost == LETHAL, PGM_OCCUPIED, np.where(cost == UNKNOWN, PGM_UNKNOWN, PGM_FREE)).astype(np.uint8)
    return b"P5\n%d %d\n255\n" % (nx, ny) + px[::-1].tobytes()


def cost_pgm_bytes(cost):
    """prefix_cost.pgm: the cost bytes, row 0 = largest y."""
    cost = np.asarray(cost, np.uint8)
    ny, nx = cost.shape
    return b"P5\n%d %d\n255\n" % (nx, ny) + cost[::-1].tobytes()


def height_bytes(ground, count, min_points, z_quantum):
    """prefix_height.f32: little-endian float32, row 0 = smallest y: (float)(ground * z_quantum in fp64), NaN where unknown."""
    h = np.where(np.asarray(count, np.int64) >= min_points, np.asarray(ground, np.float64) * float(z_quantum), np.nan).astype("<f4")
    return h.tobytes()


def yaml_text(prefix_name, resolution, x0, y0, z_quantum):
    return ("image: %s.pgm\nresolution: %.9g\norigin: [%.9g, %.9g, 0]\nnegate: 0\noccupied_thresh: 0.65\nfree_thresh: 0.196\n"
            "cost_image: %s_cost.pgm\nheight_file: %s_height.f32\nz_quantum: %.9g\nheight_row_order: bottom_up\n"
            % (prefix_name, resolution, x0 * float(resolution), y0 * float(resolution), prefix_name, prefix_name, z_quantum))
