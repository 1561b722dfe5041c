"""Inputs and cases of the dense-cell tests: uncapped maps (max_points_per_voxel = 0) whose voxels hold hundreds to thousands of
records -- what lidar2d.yaml (mh_occmap_search_map) and rgbd.yaml (SparseTreesPointCloud) align on -- where every fixed limit of
the searches inside the ICP loops is crossed: no quadrant boundaries above 31 records, 768 / 1024 / 2048 chunks of 4 records per
wave, 8 / 27 candidate voxels, k result slots.  Host arrays only; maps[key] = (points, voxel size, cap, min distance); all plain
point maps, floor indexing, cap 0.

The references are the existing ones, unchanged: oracle_c.icp_align for single pairs; for the multi-layer cases
oracle/layers_oracle.py through kbest_ref.reference (its matcher also restates gates_ref's gates and unique_global_ref's claim
walk) and planes_ref.reference.  tests/test_dense_cpu.py shows
on the reference alone that the inputs reach the regime they are there for and that no case is set apart;
tests/test_gpu_dense_cells.py runs the device on them.

Layer sizes are 1, 63, 64, 65, 129 and 2000 (2561 for k_icpw alone), not the workload's: MH_MATCH=f runs k_match_flat at any size,
so no layer above 32 768 points is needed to reach the large-layer matcher."""
import numpy as np

from mola_lidar_odometry_amd import capi
from oracle import oracle_c

import kbest_ref
import planes_ref

VS = 1.0
TOWER = (2, 2, 0)          # the voxel that holds the tower: 9000 points, more than 4 x 2048 records, beside its share of the floor
SIZES = [1, 63, 64, 65, 129, 2000]
N_SCAN = 2561              # k_icp16 takes layers up to 2560 points: the first size only k_icpw runs
N_STRAY = 120              # scan points pushed ~1 m out of a wall: their partners leave the block as they cross a voxel face
CLEARANCE = 0.02           # SparseTreesPointCloud's min_distance_between_points


def _grid(a, b, step=0.03):
    u, v = np.meshgrid(np.arange(0.0, a, step), np.arange(0.0, b, step), indexing="ij")
    return u.reshape(-1), v.reshape(-1)


def room_points(seed=4101):
    """A 6 x 5 x 3 m room: the floor z = 0 and the walls x = 0.007 and y = 0.007 on a 3 cm grid with 4 mm jitter (the jitter splits
    the floor over the two voxel layers it separates; of a wall it leaves one record in 25 on the outer side: voxels of a
    thousand records beside voxels of a few dozen), and 9000 uniform points inside the voxel TOWER."""
    rng = np.random.default_rng(seed)
    u, v = _grid(6.0, 5.0)
    floor = np.stack([u, v, np.zeros_like(u)], 1)
    u, v = _grid(5.0, 3.0)
    wall_x = np.stack([np.full_like(u, 0.007), u, v], 1)
    u, v = _grid(6.0, 3.0)
    wall_y = np.stack([u, np.full_like(u, 0.007), v], 1)
    surf = np.concatenate([floor, wall_x, wall_y])
    surf = surf + rng.normal(0.0, 0.004, surf.shape)
    tower = np.asarray(TOWER, np.float64) + rng.uniform(0.001, 0.999, (9000, 3))
    pts = np.concatenate([surf, tower])
    return np.ascontiguousarray(pts[rng.permutation(len(pts))], np.float32)


def voxel_keys(pts, vs=VS):
    """floor(p * (1 / voxel)) in fp32, the rule of DESIGN 3.1"""
    return np.floor(np.asarray(pts, np.float32) * np.float32(1.0 / vs)).astype(np.int64)


def thin_odd_voxels(pts, limit=31):
    """every voxel of odd ix + iy thinned to at most `limit` records (every n-th of the voxel's points, in insertion order)"""
    key = voxel_keys(pts)
    keep = np.ones(len(pts), bool)
    odd = ((key[:, 0] + key[:, 1]) % 2) != 0
    _, inv = np.unique(key, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    for v in np.unique(inv[odd]):
        idx = np.flatnonzero(inv == v)
        n = -(-len(idx) // limit)
        keep[idx] = False
        keep[idx[::n]] = True
    return np.ascontiguousarray(pts[keep])


def centre_points(seed=4102, res=0.05):
    """What an occupancy map hands out: cell centres (i + 0.5) * res, here two cells deep along the contour of the 6 x 5 m room at
    three adjacent z levels, in a seeded random permutation (record order is not spatial order)."""
    nx, ny = int(round(6.0 / res)), int(round(5.0 / res))
    cells = set()
    for i in range(nx):
        for d in (0, 1):
            cells.add((i, d))
            cells.add((i, ny - 1 - d))
    for j in range(ny):
        for d in (0, 1):
            cells.add((d, j))
            cells.add((nx - 1 - d, j))
    ij = np.array(sorted(cells), np.float32)
    lev = []
    for kz in (6, 7, 8):
        lev.append(np.concatenate([(ij + np.float32(0.5)) * np.float32(res),
                                   np.full((len(ij), 1), (np.float32(kz) + np.float32(0.5)) * np.float32(res), np.float32)], 1))
    pts = np.concatenate(lev).astype(np.float32)
    return np.ascontiguousarray(pts[np.random.default_rng(seed).permutation(len(pts))])


def centre_queries(pts, res=0.05):
    """Queries on half-lattice offsets of `pts`: between two cells along x, along y, between four cells in the xy and the xz
    plane -- two or four records tie exactly in fp32 d^2 (test_dense_cpu.py counts them), across voxel faces too (the cells
    19 and 20 of a metre lie at 0.975 and 1.025)."""
    h = np.float32(0.5 * res)
    offs = np.array([[h, 0, 0], [0, h, 0], [h, h, 0], [h, 0, h], [-h, h, 0]], np.float32)
    q = np.concatenate([pts[k::len(offs)] + offs[k] for k in range(len(offs))])
    return np.ascontiguousarray(q[:2000], np.float32)


def pose(x, y, z, yaw, pitch=0.0, roll=0.0):
    cy, sy, cp, sp, cr, sr = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    R = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1.0]]) @ np.array([[cp, 0, sp], [0, 1, 0], [-sp, 0, cp]]) @ \
        np.array([[1, 0, 0], [0, cr, -sr], [0, sr, cr]])
    return np.ascontiguousarray(np.concatenate([R, np.array([[x], [y], [z]])], 1).reshape(-1))


def pull_back(world, T, rng, noise=0.01):
    T = np.asarray(T, np.float64).reshape(3, 4)
    loc = (np.asarray(world, np.float64) - T[:, 3]) @ T[:, :3]  # R^T (p - t)
    return np.ascontiguousarray(loc + rng.normal(0.0, noise, loc.shape), np.float32)


def draw_scan(pts, T, n, rng, every=15):
    """n points of `pts` in the sensor frame of T with 1 cm noise, every `every`-th pushed 0.94 - 1.06 m out through the wall
    or the floor it lies nearest to (the random draws of tools/fuzz_bound.py and tools/fuzz_layers.py with the argument `dense`)"""
    world = np.asarray(pts, np.float64)[rng.choice(len(pts), n, replace=n > len(pts))]
    for i in range(5, n, every):
        ax = 2 if Inputs.in_tower(world[i]) else int(np.argmin(np.abs(world[i])))
        world[i, ax] = -rng.uniform(0.94, 1.06)
    return pull_back(world, T, rng)


class Inputs:
    """maps: room, mixed, centres, room_clear (`room` under the 2 cm clearance, before its key-frame) and capped (every third point
    of `room`, voxel 0.5, cap 20), each (points, voxel size, cap, min distance).
    scan: N_SCAN points of `room` in the sensor frame of T_gt, 1 cm noise.  Every fifteenth of the first 1800 (both parities: the
    cases split the scan in even and odd points) is pushed 0.94 - 1.06 m out through the wall or the floor it lies nearest to
    (a tower point: under the floor); a wall's records lie almost all on its inner side, so such a point's partners lie a voxel
    away and leave its block when it crosses the next voxel face.
    T0: 8 cm and about 1 degree off."""

    def __init__(self):
        rng = np.random.default_rng(4103)
        room = room_points()
        self.T_gt = pose(0.40, -0.30, 0.10, np.deg2rad(5.0), np.deg2rad(1.0), np.deg2rad(-0.5))
        self.T0 = pose(0.46, -0.35, 0.13, np.deg2rad(5.9), np.deg2rad(1.3), np.deg2rad(-0.9))
        self.T1 = pose(0.35, -0.24, 0.06, np.deg2rad(4.2), np.deg2rad(0.6), np.deg2rad(-0.1))
        world = room[rng.choice(len(room), N_SCAN, replace=False)].astype(np.float64)
        stray = np.arange(5, 15 * N_STRAY, 15)  # (not the first point: the layer of one point keeps its pairing)
        for i in stray:  # out through the surface the point lies nearest to
            ax = int(np.argmin(np.abs(world[i]))) if not self.in_tower(world[i]) else 2
            world[i, ax] = -rng.uniform(0.94, 1.06)
        self.stray = stray
        self.scan = pull_back(world, self.T_gt, rng)
        # the key-frame of room_clear: a second view, 2 cm off the first pose, of other points of the room
        self.T_kf = pose(0.42, -0.30, 0.10, np.deg2rad(5.2), np.deg2rad(1.0), np.deg2rad(-0.5))
        self.keyframe = pull_back(room[rng.choice(len(room), 4000, replace=False)], self.T_kf, rng, 0.012)
        self.maps = {"room": (room, VS, 0, 0.0), "mixed": (thin_odd_voxels(room), VS, 0, 0.0),
                     "centres": (centre_points(), VS, 0, 0.0), "room_clear": (room, VS, 0, CLEARANCE),
                     "capped": (np.ascontiguousarray(room[::3]), 0.5, 20, 0.0)}
        self.queries = centre_queries(self.maps["centres"][0])

    @staticmethod
    def in_tower(p):
        return tuple(np.floor(p).astype(int)) == TOWER

    def omaps(self, keys=None):
        return {k: oracle_c.Map(vs, cap, min_distance_between_points=md).insert(pts)
                for k, (pts, vs, cap, md) in self.maps.items() if keys is None or k in keys}

    def dmaps(self, ctx, keys=None):
        return {k: capi.Map(ctx, vs, cap, min_distance_between_points=md).build(pts)
                for k, (pts, vs, cap, md) in self.maps.items() if keys is None or k in keys}


def schedule(n, first=1.5, last=0.35):
    """Thresholds that start wide enough to pair the stray points (their partners lie a voxel away) and end at a few grid steps."""
    k = np.arange(n, dtype=np.float64)
    return np.maximum(last, first - (first - last) * k / 8.0)


# ------------------------------------------------------------------------------------------------------- single-pair cases
SINGLE_IT = 16


def single_params(mod, n_it=SINGLE_IT):
    """ICPParams of oracle_c or capi for the single-pair cases: two inner steps, the GM kernel, no stall test (every run takes
    its whole budget, so partners keep changing under a shrinking threshold)."""
    return mod.ICPParams(max_iterations=n_it, threshold=schedule(n_it), kernel_param=np.full(n_it, 0.3), disable_stall_test=True,
                         gn=mod.GNParams(max_inner_iterations=2, robust_kernel=capi.KERNEL_GM_C4))


IDENTITY = np.eye(4)[:3].reshape(12)
PRIOR_INFO = np.eye(6) * np.array([50.0, 50.0, 50.0, 200.0, 200.0, 200.0])


def single_prior(inp, n):
    """A layer below 700 points does not hold six dimensions well (one point: three): a weak prior 2 cm off the true pose keeps
    its normal equations conditioned -- a few dozen points already outweigh it, so partners still change."""
    if n >= 700:
        return None
    Tp = inp.T_gt.copy()
    Tp[3] += 0.02
    return (Tp, PRIOR_INFO)


# the plane searches of the tie section on `centres`: (knn, eigenvalue threshold); rgbd.yaml's 1e-2 accepts no plane on a contour
# two cells deep
TIE_PLANES = [(16, 0.3), (10, 0.5)]
TIE_PLANE_RADIUS, TIE_PLANE_MIN_POINTS = 0.8, 6

# the launch chain's cases of tests/test_gpu_dense_cells.py beside the 16-iteration singles: (points, iterations) on `room`
CHAIN_CASES = [(129, 6), (2000, 6), (2561, 6), (2561, 16)]


def single_scan(inp, n):
    """the layer of n points: a slice that holds its share of stray points; 2561: the whole scan"""
    return inp.scan[:n]


# --------------------------------------------------------------------------------------------------------- multi-layer cases
RGBD = planes_ref.RGBD
KNN16 = dict(knn=16, minimum_plane_points=6, plane_eigen_threshold=5e-2, search_radius=1.5)  # the radius takes in the tower


def _kp(mk, local, thr, k=1, weight=1.0, gate=(0, 0), unique=0, plane=None):
    return dict(map=mk, local=np.ascontiguousarray(local, np.float32), threshold=thr, threshold_angular_deg=0.0, weight=weight,
                gate=gate, unique=unique, k=k, plane=dict(plane) if plane else None)


def cases(inp):
    """name -> dict(kind, pairs, max_it, kp, inner, T0, prior, pkw); kind: "k" (kbest_ref.case_reference: k-best, gates, unique)
    or "pl" (planes_ref.case_reference)."""
    s = inp.scan[:2000]
    t12, t14 = schedule(12), schedule(14, 1.3, 0.4)
    pthr = np.full(12, 0.4)
    out = {}
    # two pairs sharing the dense map, weights and schedules of their own
    out["two_pairs"] = dict(kind="k", pairs=[_kp("room", s[0::2], t12), _kp("room", s[1::2], schedule(12, 1.2, 0.5), weight=0.25)])
    # the dense map beside a cap-20 map in one table
    out["beside_capped"] = dict(kind="k", pairs=[_kp("room", s[:1000], t12), _kp("capped", s[1000:], schedule(12, 1.0, 0.4), weight=0.5)])
    # pairings_per_point 2 (what both pipelines set) and 8
    out["k2"] = dict(kind="k", pairs=[_kp("room", s[0::2], t12, k=2), _kp("room", s[1::2], schedule(12, 1.2, 0.5), k=2, weight=0.5)])
    out["k8"] = dict(kind="k", pairs=[_kp("room", s[:600], t12, k=8)])
    out["k2_mixed"] = dict(kind="k", pairs=[_kp("mixed", s[:1000], t12, k=2)])
    for n in (1, 63, 64, 65, 129):
        out["k2_n%d" % n] = dict(kind="k", pairs=[_kp("room", s[:n], t12, k=2, weight=float(max(1.0, 200.0 / n))),
                                                   _kp("room", s[1000:], t12)])
    out["unique"] = dict(kind="k", pairs=[_kp("room", s[0::2], t12, unique=1), _kp("room", s[1::2], t12, weight=0.5, unique=1)])
    out["gated"] = dict(kind="k", pairs=[_kp("room", s[:700], t12, k=2, gate=(2, 0)), _kp("room", s[700:], t12)])
    # plane pairs: rgbd.yaml's parameters beside its k = 2 point pair; knn 16 with a radius that takes in the tower
    out["rgbd"] = dict(kind="pl", pairs=[_kp("room", s[0::2], t12, k=2), _kp("room", s[1::2], pthr, plane=RGBD)])
    out["knn16"] = dict(kind="pl", pairs=[_kp("room", s[:700], pthr, plane=KNN16), _kp("room", s[1000:], t12)])
    for c in out.values():
        c.setdefault("max_it", 12)
        c.setdefault("kp", np.full(c["max_it"], 0.3))
        c.setdefault("inner", 2)
        c.setdefault("T0", inp.T0)
        c.setdefault("prior", None)
        c.setdefault("pkw", dict(disable_stall_test=True))
    return out


def case_reference(c, omaps):
    if c["kind"] == "pl":
        return planes_ref.case_reference(c, omaps)
    return kbest_ref.case_reference(c, omaps)


def device_pairs(c, dmaps, scans):
    """capi.icp_align_layers' pairs and pairings_per_point of a case; scans(array) -> capi.Scan."""
    pairs = []
    for e in c["pairs"]:
        d = dict(map=dmaps[e["map"]], scan=scans(e["local"]), threshold=e["threshold"], weight=e["weight"], unique_global=e["unique"],
                 run_from_iteration=e["gate"][0], run_up_to_iteration=e["gate"][1])
        if e["plane"]:
            d["plane"] = e["plane"]
        pairs.append(d)
    ks = [e["k"] for e in c["pairs"]]
    return pairs, (ks if any(k > 1 for k in ks) else None)


device_params = kbest_ref.device_params
set_apart = kbest_ref.set_apart


# ------------------------------------------------------------------------------------------------ what the CPU test reads
def occupancy(dump):
    """records per voxel of an oracle_c.Map.dump()"""
    return np.asarray(dump["vox_count"]).astype(np.int64)


def own_voxel_count(dump, world):
    """for every world point: the record count of the voxel it falls in (0: no such voxel)"""
    keys = np.asarray(dump["vox_keys"]).astype(np.int64)
    table = {tuple(k): int(c) for k, c in zip(keys.tolist(), occupancy(dump).tolist())}
    return np.array([table.get(tuple(k), 0) for k in voxel_keys(world).tolist()], np.int64)


def transform(local, T):
    """the device's and the oracle's transform: fp64 pose times fp32 point, rounded to fp32"""
    T = np.asarray(T, np.float64).reshape(-1)[:12].reshape(3, 4)
    x, y, z = np.asarray(local, np.float32).astype(np.float64).T
    return np.stack([((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3)], 1).astype(np.float32)


def brute_force_k(dump, world, k, threshold):
    """The k nearest records of each fp32 world point inside its 27-voxel block, nn_consider's un-fused fp32 expression
    d2 = (dx dx + dy dy) + dz dz, ties by record index (the order of the dump), accepted while d2 < threshold^2: per point the
    list of (record index, d2).  Plain numpy, independent of the C oracle."""
    xyz = np.asarray(dump["xyz"], np.float32)
    keys = np.asarray(dump["vox_keys"]).astype(np.int64)
    first, count = np.asarray(dump["vox_first"]).astype(np.int64), occupancy(dump)
    table = {tuple(kk): (int(f), int(c)) for kk, f, c in zip(keys.tolist(), first.tolist(), count.tolist())}
    thr2 = np.float32(np.float64(threshold) * np.float64(threshold))
    out = []
    for p, key in zip(np.asarray(world, np.float32), voxel_keys(world).tolist()):
        idx = []
        for dx in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dz in (-1, 0, 1):
                    fc = table.get((key[0] + dx, key[1] + dy, key[2] + dz))
                    if fc:
                        idx.append(np.arange(fc[0], fc[0] + fc[1]))
        if not idx:
            out.append([])
            continue
        idx = np.concatenate(idx)
        d = xyz[idx] - p
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]  # fp32 throughout
        order = np.lexsort((idx, d2))[:k]
        out.append([(int(idx[j]), np.float32(d2[j])) for j in order if d2[j] < thr2])
    return out


def partners_that_left(m, local, poses, thresholds, k):
    """Per iteration j >= 1, from the reference's poses alone: (points one of whose k partners of iteration j - 1 lies outside
    the 27-voxel block the point falls in at pose j -- no record of the block attains the bound those partners give, the slot
    k - 1 of a bounded search stays empty --, those among them that still have k accepted pairings at pose j: a search that
    trusted its bound would lose one).  Read from voxel indices, so rounding of a distance plays no part."""
    local = np.asarray(local, np.float32).reshape(-1, 3)
    out = []
    for j in range(1, len(poses)):
        a = oracle_c.match_points_k(m, local, poses[j - 1], float(thresholds[j - 1]), k)
        b = oracle_c.match_points_k(m, local, poses[j], float(thresholds[j]), k)
        now = voxel_keys(transform(local, poses[j]))
        away = np.abs(voxel_keys(a["global_xyz"]) - now[a["local_idx"]]).max(1) > 1
        left = np.zeros(len(local), bool)
        left[a["local_idx"][away]] = True
        full = np.bincount(b["local_idx"], minlength=len(local)) == k
        out.append((int(left.sum()), int((left & full).sum())))
    return out


def next_d2(dump, q, chosen):
    """the smallest fp32 d2 of `q` to a record of its 27-voxel block that is not among `chosen` (brute_force_k's entries for q):
    equal to the last chosen d2 when the choice of the k-th record was made among tied ones"""
    more = brute_force_k(dump, np.asarray(q, np.float32).reshape(1, 3), len(chosen) + 1, 1e3)[0]
    return more[-1][1] if len(more) > len(chosen) else np.float32(np.inf)
