"""A numpy restatement of what include/molahip_occgrid.h and mola_lidar_odometry_hip/OccupancyGrid.h add to the occupancy map of
tests/occmap_ref.py: the index bounds, the projection of a height band, the trinary rule, the height-to-index rule, the window, the
PGM / YAML bytes, and the whole key-frames-to-grid path driven through OccMapRef (the loop of single inserts IS the definition of
the batched insertion, so there is nothing else to restate for it).  Written from the headers' text.  No product code."""
import numpy as np

import lidar2d_inline as L2
import occmap_ref as R

NONE = -(1 << 31)                      # MH_OCCGRID_NONE
FREE, OCCUPIED, UNKNOWN = 0, 100, -1   # the cells of a grid
PGM_OCCUPIED, PGM_FREE, PGM_UNKNOWN = 0, 254, 205
F = np.float32

DEFAULTS = dict(resolution=0.05, prob_hit=0.70, prob_miss=0.30, clamp_min=0.05, clamp_max=0.95, occupied_threshold=0.60,
                ray_trace_free_space=True, max_range=0.0, decimation=1, update_rule="counted", target_map="", z_min=-0.10, z_max=1.50,
                margin_cells=2)


def index_bounds(keys):
    """(lo [3], hi [3]) over the stored cells, or None for an empty map."""
    keys = np.asarray(keys, np.int64).reshape(-1, 3)
    return (keys.min(axis=0), keys.max(axis=0)) if len(keys) else None


def project(keys, logodds, x0, y0, nx, ny, z_lo, z_hi):
    """int32 [ny, nx]: per column the maximum log-odds over the stored cells inside the band, NONE where there is none."""
    out = np.full((ny, nx), NONE, np.int64)
    for (kx, ky, kz), l in zip(np.asarray(keys, np.int64).reshape(-1, 3).tolist(), np.asarray(logodds).tolist()):
        if z_lo <= kz <= z_hi and 0 <= kx - x0 < nx and 0 <= ky - y0 < ny:
            out[ky - y0, kx - x0] = max(out[ky - y0, kx - x0], l)
    return out.astype(np.int32)


def classify(max_logodds, l_occ):
    """(int8 cells, occupied, free, unknown): UNKNOWN where the maximum is NONE, OCCUPIED where it is >= l_occ, FREE otherwise."""
    m = np.asarray(max_logodds, np.int64)
    cells = np.where(m == NONE, UNKNOWN, np.where(m >= l_occ, OCCUPIED, FREE)).astype(np.int8)
    return cells, int((cells == OCCUPIED).sum()), int((cells == FREE).sum()), int((cells == UNKNOWN).sum())


def z_index(z, resolution):
    """floor(z * (double)(1.0f / (float)resolution)): the map's floor rule with its own fp32 reciprocal, in fp64."""
    return int(np.floor(np.float64(z) * np.float64(F(1.0) / F(resolution))))


def window(lo, hi, margin_cells):
    """(x0, y0, nx, ny) from the index bounds over all stored cells."""
    return (int(lo[0]) - margin_cells, int(lo[1]) - margin_cells, int(hi[0]) - int(lo[0]) + 1 + 2 * margin_cells,
            int(hi[1]) - int(lo[1]) + 1 + 2 * margin_cells)


def pgm_bytes(cells):
    """Binary P5: row 0 of the image is the largest y; 0 occupied, 254 free, 205 unknown."""
    cells = np.asarray(cells, np.int8)
    ny, nx = cells.shape
    px = np.where(cells == OCCUPIED, PGM_OCCUPIED, np.where(cells == FREE, PGM_FREE, PGM_UNKNOWN)).astype(np.uint8)
    return b"P5\n%d %d\n255\n" % (nx, ny) + px[::-1].tobytes()


def yaml_text(pgm_name, resolution, x0, y0):
    return ("image: %s\nresolution: %.9g\norigin: [%.9g, %.9g, 0]\nnegate: 0\noccupied_thresh: 0.65\nfree_thresh: 0.196\n"
            % (pgm_name, resolution, x0 * float(resolution), y0 * float(resolution)))


def occmap_ref(opt):
    rule = {"counted": R.COUNTED, "once": R.ONCE}[opt["update_rule"]]
    return R.OccMapRef(opt["resolution"], opt["prob_hit"], opt["prob_miss"], opt["clamp_min"], opt["clamp_max"], opt["occupied_threshold"],
                       opt["ray_trace_free_space"], opt["decimation"], opt["max_range"], rule)


def build(frames, **options):
    """The whole path on (xyz, T) frames: the loop of single inserts into a fresh map, the window from the bounds plus the margin,
    the projection of the band, the trinary rule.  Returns a dict with the keys of the host's grid."""
    opt = dict(DEFAULTS, **options)
    m = occmap_ref(opt)
    for xyz, T in frames:
        m.insert(xyz, T)
    keys, lo = m.download()
    b = index_bounds(keys)
    x0, y0, nx, ny = window(b[0], b[1], opt["margin_cells"])
    z_lo, z_hi = z_index(opt["z_min"], opt["resolution"]), z_index(opt["z_max"], opt["resolution"])
    mx = project(keys, lo, x0, y0, nx, ny, z_lo, z_hi)
    cells, n_occ, n_free, n_unk = classify(mx, m.l_occ)
    return dict(x0=x0, y0=y0, nx=nx, ny=ny, resolution=opt["resolution"], z_lo=z_lo, z_hi=z_hi, l_occ=m.l_occ, max_logodds=mx, cells=cells,
                cells_occupied=n_occ, cells_free=n_free, cells_unknown=n_unk, map_cells=len(keys))


# ---- the session of the host-path test: 12 key-frames of lidar2d_inline's analytic ray caster in its 10 m x 8 m room -----------
ROOM_FRAMES = 12


def room_session():
    """(frames as (xyz, T [12]) pairs, the key-frame set as the dict the host takes): a lidar2d session, a CVoxelMap plan."""
    stamps, poses, scans = L2.drive(n_scans=ROOM_FRAMES, step_deg=170.0 / (ROOM_FRAMES - 1))   # (from -150 to +20 degrees: clear of the box)
    frames = [(s, p[:3].reshape(12).copy()) for s, p in zip(scans, poses)]
    params = dict(voxel_size=L2.RESOLUTION, max_points_per_voxel=0, index_mode=0, min_distance_between_points=0.0, ndt_max_eigen_ratio=0.0,
                  ndt_min_points=0, far_voxel_metric=0)
    kfset = dict(maps=[dict(name="localmap", class_name="CVoxelMap", params=params, remove_voxels_farther_than=0.0)],
                 frames=[dict(timestamp=float(t), pose=T.tolist(), cov=[0.0] * 36, twist=None, layers=[(0, xyz)])
                         for t, (xyz, T) in zip(stamps, frames)])
    return frames, kfset


def room_truth(g):
    """Which cells of grid g must read what, from the room's geometry alone (walls on x = +-5, y = +-4; the box [1, 2.5] x [1, 2]).
    A hit that lies exactly on a wall falls, after rounding, into the cell on either side of it, so a wall SITE is the pair of cells
    across the wall line at one position along it.  Returns (interior mask, outside mask, wall sites as [k, 2, 2] (row, col))."""
    res = g["resolution"]
    ix = g["x0"] + np.arange(g["nx"])
    iy = g["y0"] + np.arange(g["ny"])
    X0, Y0 = np.meshgrid(ix * res, iy * res)               # lower-left corners
    X1, Y1 = X0 + res, Y0 + res
    pad = 2 * res                                          # two cells clear of every wall
    in_room = (X0 >= -5 + pad) & (X1 <= 5 - pad) & (Y0 >= -4 + pad) & (Y1 <= 4 - pad)
    near_box = (X1 > 1.0 - pad) & (X0 < 2.5 + pad) & (Y1 > 1.0 - pad) & (Y0 < 2.0 + pad)
    interior = in_room & ~near_box
    outside = (X1 <= -5 - pad) | (X0 >= 5 + pad) | (Y1 <= -4 - pad) | (Y0 >= 4 + pad)
    col = lambda x: int(round(x / res)) - g["x0"]          # the column whose LEFT edge is x
    row = lambda y: int(round(y / res)) - g["y0"]
    sites = []
    for x in (-5.0, 5.0):                                  # the walls of the room, corners left out
        sites += [[(r, col(x) - 1), (r, col(x))] for r in range(row(-4.0) + 2, row(4.0) - 2)]
    for y in (-4.0, 4.0):
        sites += [[(row(y) - 1, c), (row(y), c)] for c in range(col(-5.0) + 2, col(5.0) - 2)]
    return interior, outside, np.array(sites, np.int64)


def room_shares(g):
    """(interior cells, of which unknown, of which occupied; wall sites, of which with no occupied cell; outside cells, of which known)."""
    interior, outside, sites = room_truth(g)
    cells = np.asarray(g["cells"])
    occ_site = (cells[sites[:, 0, 0], sites[:, 0, 1]] == OCCUPIED) | (cells[sites[:, 1, 0], sites[:, 1, 1]] == OCCUPIED)
    return (int(interior.sum()), int((cells[interior] == UNKNOWN).sum()), int((cells[interior] == OCCUPIED).sum()), len(sites),
            int((~occ_site).sum()), int(outside.sum()), int((cells[outside] != UNKNOWN).sum()))
