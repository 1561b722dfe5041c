"""Inputs, map updates and references of the warm-map tests: every search route (route_tables.MUTATION_ROUTES) on a handle that has
been searched before and is then updated by mh_map_build, mh_map_insert, mh_map_insert_frames, mh_map_restore,
mh_map_erase_points, mh_map_insert + mh_map_erase_seen_through or mh_occmap_insert -- the promise of include/molahip.h and
include/molahip_live.h that an updated map "gives the same answers from every search route".

Host arrays and references only.  Every update is a pair of functions over the same inputs: MUTATIONS[name].oracle(kind) builds
the oracle's map of the history with no device in the loop, MUTATIONS[name].device(kind, dev) drives a device map through it.
The reference after a restore or an erasing is "exactly the points given" (mh_map_restore's definition): an oracle map with cap
0 and clearance 0 that is handed the surviving points in download order, its global indices mapped back through the surviving
src_idx; the surviving set comes from the oracle's own dump(), for the queued erasing through clean_ref.vote / decide.

tests/test_mutation_cpu.py shows on the references alone that the inputs can catch a stale structure (partners change, the
table size stays for some kinds and changes for others, every update does its own work); tests/test_gpu_map_mutations.py runs
the device.

The world: a 24 x 24 x 4 m box of 1 m voxels.  Below z = 0 every point lies on its voxel's sheet (a 1 cm thick plane through
the voxel's centre whose normal axis is (ix + iy + iz) mod 3): NDT voxels find planes there and the KNN + PCA plane pair finds
neighbourhoods to fit; above, points are uniform: partners in every direction."""
import functools
from types import SimpleNamespace

import numpy as np

import clean_ref as cr
import dense_cases as dc
import occmap_ref
import radius_ref as rr
import score_ref as sr
from mola_lidar_odometry_amd import capi
from oracle import oracle_c
from route_tables import MUTATION_IT, MUTATION_ROUTES, mutation_routes

F = np.float32
VS = 1.0
KINDS = {  # tests/test_gpu_map_restore.py's four
    "capped_floor": dict(voxel_size=VS, max_points_per_voxel=20, index_mode="floor"),
    "capped_trunc": dict(voxel_size=VS, max_points_per_voxel=20, index_mode="trunc"),
    "ndt": dict(voxel_size=VS, max_points_per_voxel=20, index_mode="floor", ndt_max_eigen_ratio=0.1, min_distance_between_points=0.05),
    "uncapped": dict(voxel_size=VS, max_points_per_voxel=0, index_mode="floor"),
}
# the occupancy map's own inner map (an uncapped point map over the occupied cells' centres): (resolution, second scan's share)
OCC_KINDS = {"occ_5cm": dict(resolution=0.05, share=0.35), "occ_10cm": dict(resolution=0.1, share=1.0)}
IDX = {"floor": (capi.INDEX_FLOOR, oracle_c.INDEX_FLOOR), "trunc": (capi.INDEX_TRUNC, oracle_c.INDEX_TRUNC)}
BOX_LO, BOX_HI = (-12.0, -12.0, -2.0), (12.0, 12.0, 2.0)
N_FIRST = dict(capped_floor=14000, capped_trunc=14000, ndt=14000, uncapped=30900)
# the last points of the first cloud that arrive by an insertion under the identity pose, not with the build: the table is then
# sized from the insertion's voxel bound (stored voxels + new points), not from the build's (every point a voxel), so that an
# erasing -- whose bound is the stored voxels -- can keep it
N_FIRST_INSERTED = dict(capped_floor=0, capped_trunc=0, ndt=1000, uncapped=0)
I12 = np.eye(4)[:3].reshape(12)
N_SCAN = 2561
N_PARTNERS = 2000        # the test scan of the partner shares
THR_PARTNERS = 1.0
N_RADIUS = 257           # queries of the radius search (its restatement is a brute force over the map)
FAR = 7.0
T_GT = dc.pose(0.40, -0.30, 0.10, np.deg2rad(5.0), np.deg2rad(1.0), np.deg2rad(-0.5))
T0 = dc.pose(0.46, -0.35, 0.13, np.deg2rad(5.9), np.deg2rad(1.3), np.deg2rad(-0.9))
T1 = dc.pose(0.35, -0.24, 0.06, np.deg2rad(4.2), np.deg2rad(0.6), np.deg2rad(-0.1))
T_KF = dc.pose(4.0, -0.5, 0.1, 0.05, 0.01, -0.02)
PLANE = dict(knn=10, minimum_plane_points=6, plane_eigen_threshold=5e-2, search_radius=0.8)


def is_ndt(kind):
    return kind == "ndt"


def is_occ(kind):
    return kind in OCC_KINDS


def map_params(kind, which):
    """capi.Map's (which = 0) or oracle_c.Map's (1) keyword arguments"""
    p = dict(KINDS[kind])
    p["index_mode"] = IDX[p["index_mode"]][which]
    return p


def voxel_of(kind, xyz):
    """the voxel index of fp32 points under the kind's index mode (p * (1 / voxel) in fp32)"""
    s = np.asarray(xyz, F) * F(1.0 / VS)
    trunc = not is_occ(kind) and KINDS[kind]["index_mode"] == "trunc"
    return (np.trunc(s) if trunc else np.floor(s)).astype(np.int64)


def table_size(voxel_bound):
    """map_build_prologue's rule: the smallest power of two >= 2 x the voxel bound, at least 64"""
    t = 64
    while t < 2 * int(voxel_bound):
        t <<= 1
    return t


# ------------------------------------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def cloud(seed, n, lo=BOX_LO, hi=BOX_HI):
    rng = np.random.default_rng(seed)
    p = rng.uniform(lo, hi, (n, 3))
    k = np.floor(p)
    axis = (k.sum(1).astype(np.int64)) % 3
    sheet = p[:, 2] < 0.0
    rows = np.flatnonzero(sheet)
    p[rows, axis[rows]] = k[rows, axis[rows]] + 0.5 + rng.normal(0.0, 0.01, len(rows))
    out = np.ascontiguousarray(p, F)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def first_cloud(kind):
    # three crowded voxels: caps are met there from the start; uncapped, they hold more than the 31 records of an indexed voxel
    rng = np.random.default_rng(4202)
    crowd = [rng.uniform(0.01, 0.99, (300, 3)) + np.array(v, np.float64) for v in ((1, 1, 0), (2, 1, 0), (1, 2, 1))]
    c = np.concatenate(crowd + [cloud(4201, N_FIRST[kind] - 900)])
    c = np.ascontiguousarray(c, F)
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def scan(kind=None):
    """N_SCAN points of the world in the sensor frame of T_GT, 1 cm noise; the layers of every route are slices of it"""
    rng = np.random.default_rng(4203)
    return dc.pull_back(cloud(4204, N_SCAN, (-10.0, -10.0, -1.8), (10.0, 10.0, 1.8)), T_GT, rng)


def prior(n):
    """dense_cases.single_prior: a layer below 700 points gets a weak prior 2 cm off the true pose"""
    if n >= 700:
        return None
    Tp = T_GT.copy()
    Tp[3] += 0.02
    return (Tp, dc.PRIOR_INFO)


@functools.lru_cache(maxsize=None)
def keyframe(seed=4210, n=12000):
    """a key-frame around T_KF, 4 m along x from the first cloud's centre: (points in the sensor frame, pose)"""
    rng = np.random.default_rng(seed + 1)
    return dc.pull_back(cloud(seed, n, (-3.0, -8.0, -2.0), (11.0, 6.0, 2.0)), T_KF, rng, 0.0), T_KF


N_FRAME = dict(capped_floor=6000, capped_trunc=9000, ndt=6000, uncapped=10000)
FRAME_BUDGET = dict(capped_floor=13000, capped_trunc=10000, ndt=7000, uncapped=13000)


@functools.lru_cache(maxsize=None)
def frames(kind):
    """three key-frames over the whole box, each under a pose of its own"""
    out = []
    for j in range(3):
        T = dc.pose(1.5 * j, -0.4 * j, 0.1, 0.05 * j, 0.01, -0.02)
        out.append((dc.pull_back(cloud(4220 + j, N_FRAME[kind]), T, np.random.default_rng(4230 + j), 0.0), T))
    return out


N_SECOND = dict(capped_floor=15000, capped_trunc=20000, ndt=9000, uncapped=22000)


def second_cloud(kind):
    """build_again's cloud: other points, another number of them, in a box shifted 3 m along x and y"""
    return cloud(4240, N_SECOND[kind], (-9.0, -15.0, -2.0), (15.0, 9.0, 2.0))


N_OTHER = dict(capped_floor=15000, capped_trunc=6000, ndt=15000, uncapped=25000)

# erase_queued's views: two far shells (every bin of a narrow elevation window holds a point 30 - 40 m away), seen from two
# places in the box: whatever lies in a window nearer than the shell is seen through
VIEW_PARAMS = dict(cr.DEFAULT, el_min=float(np.radians(-6.0)), el_max=float(np.radians(6.0)), win_rings=0, win_sectors=0)
NBR_VIEW = np.array([0, 1], np.uint32)
NBR_T = np.stack([np.eye(4)[:3].reshape(12), dc.pose(-3.0, -2.0, -0.3, 0.5)])
VOTE = dict(min_through_votes=1, agree_weight=1)


@functools.lru_cache(maxsize=None)
def view_clouds():
    out = []
    for seed in (4250, 4251):
        rng = np.random.default_rng(seed)
        n = 40000
        az, el, r = rng.uniform(-np.pi, np.pi, n), rng.uniform(VIEW_PARAMS["el_min"], VIEW_PARAMS["el_max"], n), rng.uniform(30.0, 40.0, n)
        out.append(np.ascontiguousarray(np.stack([r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el)], 1), F))
    return out


@functools.lru_cache(maxsize=None)
def views():
    return [cr.view(c, **VIEW_PARAMS) for c in view_clouds()]


# ---------------------------------------------------------------------------------------------------------------- references
class Ref:
    """The oracle's map of one history.  src: None, or the device's global index of the oracle's record i (a map that holds
    "exactly the points given": the oracle numbers them as they come, the device keeps their src_idx).  table: the hash table
    size the device chooses for it, from the voxel bound its host knows."""

    def __init__(self, kind, om, voxel_bound, src=None):
        self.kind, self.om, self.src, self.table = kind, om, None if src is None else np.asarray(src, np.uint32), table_size(voxel_bound)
        self.done = {}

    def fix(self, r):
        """the oracle's result with the device's global indices"""
        if self.src is None:
            return r
        if "pairs" in r:
            ps = r["pairs"]
            r = dict(r, pairs=self.fix(ps) if isinstance(ps, dict) else [self.fix(p) for p in ps])
        if "global_idx" in r:
            r = dict(r, global_idx=self.src[r["global_idx"]])
        return r

    def dump(self):
        d = self.om.dump()
        return d if self.src is None else dict(d, src_idx=self.src[d["src_idx"]])

    def once(self, key, make):
        if key not in self.done:
            self.done[key] = make()
        return self.done[key]


def oracle_map(kind, exactly=False):
    """an empty oracle map of the kind; exactly: cap 0 and clearance 0, for "exactly the points given" """
    p = map_params(kind, 1)
    if exactly:
        p.update(max_points_per_voxel=0, min_distance_between_points=0.0)
    return oracle_c.Map(**p)


def exactly(kind, xyz, src, voxel_bound):
    """the reference after mh_map_restore(xyz, src): the points in download order, indices mapped back through src"""
    return Ref(kind, oracle_map(kind, True).insert(np.asarray(xyz, F).reshape(-1, 3)) if len(xyz) else oracle_map(kind, True),
               voxel_bound, src)


@functools.lru_cache(maxsize=None)
def before(kind):
    """the map every test starts from: one build of the first cloud (an occupancy map: its first scan)"""
    if is_occ(kind):
        return _occ_ref(kind, 1)
    return Ref(kind, _started(kind)[0], _first_bound(kind))


def _started(kind):
    """a fresh oracle map in the state of before(kind), to be updated: (map, stored points, voxels)"""
    c, k = first_cloud(kind), N_FIRST_INSERTED[kind]
    om = oracle_map(kind).insert(c[:len(c) - k])
    if k:
        om.insert_posed(c[len(c) - k:], I12)
    return om, om.num_points, om.num_voxels


def _first_bound(kind):
    c, k = first_cloud(kind), N_FIRST_INSERTED[kind]
    if not k:
        return len(c)
    built = oracle_map(kind).insert(c[:len(c) - k])
    return _insert_bound(built.num_points, built.num_voxels, k)


def _insert_bound(n_old, v_old, n_new):
    """map_build_prologue's voxel bound of an insertion: every offered point kept, every new point a voxel of its own"""
    return min(n_old + n_new, v_old + n_new)


# ---- build_again
def _o_build_again(kind):
    c = second_cloud(kind)
    return Ref(kind, oracle_map(kind).insert(c), len(c)), {}


def _d_build_again(kind, dev):
    dev.m.build(np.zeros((0, 3), F))   # to empty ...
    dev.m.build(second_cloud(kind))    # ... and back


# ---- insert_far (merge path, and under MH_MAP_FULL_SORT=1)
def _o_insert_far(kind):
    om, n_old, v_old = _started(kind)
    kf, T = keyframe()
    om.insert_posed(kf, T, FAR)
    return Ref(kind, om, _insert_bound(n_old, v_old, len(kf))), {}


def _d_insert_far(kind, dev):
    dev.m.insert(dev.scan(keyframe()[0]), keyframe()[1], FAR)


def _d_insert_far_full_sort(kind, dev):
    dev.monkeypatch.setenv("MH_MAP_FULL_SORT", "1")
    try:
        _d_insert_far(kind, dev)
    finally:
        dev.monkeypatch.delenv("MH_MAP_FULL_SORT")


# ---- insert_frames
def frame_passes(kind):
    """mh_map_insert_frames' passes: frames in order while they fit the budget"""
    fr, out, f0 = frames(kind), [], 0
    while f0 < len(fr):
        f1, P = f0, 0
        while f1 < len(fr) and (P == 0 or P + len(fr[f1][0]) <= FRAME_BUDGET[kind]):
            P += len(fr[f1][0])
            f1 += 1
        out.append((f0, f1))
        f0 = f1
    return out


def _o_insert_frames(kind):
    om, _, _ = _started(kind)
    bound = 0
    for f0, f1 in frame_passes(kind):
        n_old, v_old = om.num_points, om.num_voxels   # (every pass takes the counts of the one before in)
        for xyz, T in frames(kind)[f0:f1]:
            om.insert_posed(xyz, T)
        bound = _insert_bound(n_old, v_old, sum(len(x) for x, _ in frames(kind)[f0:f1]))
    return Ref(kind, om, bound), dict(passes=len(frame_passes(kind)))


def _d_insert_frames(kind, dev):
    dev.m.insert_frames(frames(kind), FRAME_BUDGET[kind])


# ---- restore_over
@functools.lru_cache(maxsize=None)
def other_map(kind):
    """another map's download and n_offered: a build plus one insertion with far-voxel removal, from the oracle's dump"""
    c = cloud(4260, N_OTHER[kind], (-10.0, -14.0, -2.0), (14.0, 10.0, 2.0))
    kf, T = keyframe(4270, 8000)
    om = oracle_map(kind).insert(c).insert_posed(kf, T, FAR + 2.0)
    return om.dump(), len(c) + len(kf)


def _o_restore_over(kind):
    d, _ = other_map(kind)
    return exactly(kind, d["xyz"], d["src_idx"], len(d["xyz"])), {}


def _d_restore_over(kind, dev):
    d, n_offered = other_map(kind)
    dev.m.restore(d["xyz"], d["src_idx"], n_offered)


# ---- erase_points
@functools.lru_cache(maxsize=None)
def erase_mask(kind):
    """drop flags over before(kind)'s dump: whole voxels (every third of a diagonal family), the first and the last record of
    the fullest voxel that stays, and every third point"""
    d = before(kind).om.dump()
    keys, first, count = d["vox_keys"].astype(np.int64), d["vox_first"].astype(np.int64), d["vox_count"].astype(np.int64)
    drop = np.arange(len(d["xyz"])) % 3 == 0
    whole = (keys.sum(1) % 3) == 0
    for v in np.flatnonzero(whole):
        drop[first[v]:first[v] + count[v]] = True
    stays = np.flatnonzero(~whole)
    v = stays[np.argmax(count[stays])]
    drop[[first[v], first[v] + count[v] - 1]] = True
    return drop


def _o_erase_points(kind):
    b = before(kind)
    d, drop = b.om.dump(), erase_mask(kind)
    return exactly(kind, d["xyz"][~drop], d["src_idx"][~drop], b.om.num_voxels), dict(mid=b, drop=drop)


def _d_erase_points(kind, dev):
    from mola_lidar_odometry_amd import capi_live
    capi_live.erase_points(dev.m, erase_mask(kind))


# ---- erase_queued: an insertion and, with nothing between them that takes its counts in, mh_map_erase_seen_through
def _o_erase_queued(kind):
    om, n_old, v_old = _started(kind)
    kf, T = keyframe()
    om.insert_posed(kf, T)
    mid = Ref(kind, om, _insert_bound(n_old, v_old, len(kf)))
    d = om.dump()
    drop = cr.decide(cr.vote(d["xyz"], views(), NBR_VIEW, NBR_T, **VIEW_PARAMS), **VOTE)
    # the erasing rebuilds from the insertion's bounds: its own voxel bound is the insertion's
    after = exactly(kind, d["xyz"][~drop], d["src_idx"][~drop], _insert_bound(n_old, v_old, len(kf)))
    return after, dict(mid=mid, drop=drop, points_bound=n_old + len(kf), points_stored=om.num_points)


def _d_erase_queued(kind, dev):
    from mola_lidar_odometry_amd import capi_live
    v, s = dev.views(), dev.scan(keyframe()[0])
    dev.m.insert(s, keyframe()[1], 0.0)
    capi_live.erase_seen_through(dev.m, v, NBR_VIEW, NBR_T, VOTE["min_through_votes"], VOTE["agree_weight"])


# ---- occmap_insert
def _room(x0, x1, y0, y1, step, levels):
    u, v = np.arange(x0, x1, step), np.arange(y0, y1, step)
    ring = np.concatenate([np.stack([u, np.full_like(u, y0)], 1), np.stack([u, np.full_like(u, y1)], 1),
                           np.stack([np.full_like(v, x0), v], 1), np.stack([np.full_like(v, x1), v], 1)])
    return np.concatenate([np.concatenate([ring, np.full((len(ring), 1), z)], 1) for z in levels])


OCC_T = [dc.pose(6.0, 5.0, 0.5, 0.0), dc.pose(9.0, 5.0, 0.5, 0.3)]
OCC_FAR = 8.0
OCC_LEVELS = np.arange(0.03, 1.2, 0.06)


@functools.lru_cache(maxsize=None)
def occ_scans(kind):
    """two scans of wall contours at many heights, in the sensor frames of OCC_T: a 12 x 10 m room; then a room shifted by
    (2, -2) seen from 3 m further along x, whose insertion removes what lies farther than OCC_FAR"""
    rng = np.random.default_rng(4280)
    a = _room(0.0, 12.0, 0.0, 10.0, 0.04, OCC_LEVELS)
    b = _room(2.0, 16.0, -2.0, 10.0, 0.04, OCC_LEVELS)
    b = b[:int(len(b) * OCC_KINDS[kind]["share"])]
    return [dc.pull_back(a, OCC_T[0], rng, 0.0), dc.pull_back(b, OCC_T[1], rng, 0.0)]


@functools.lru_cache(maxsize=None)
def occ_scan_queries():
    """N_SCAN points near both rooms' walls in the sensor frame of T_GT"""
    rng = np.random.default_rng(4281)
    w = np.concatenate([_room(0.0, 12.0, 0.0, 10.0, 0.05, OCC_LEVELS[::3]), _room(2.0, 16.0, -2.0, 10.0, 0.05, OCC_LEVELS[::3])])
    return dc.pull_back(w[rng.choice(len(w), N_SCAN, replace=False)], T_GT, rng, 0.03)


def occ_args(kind):
    return dict(resolution=OCC_KINDS[kind]["resolution"], ray_trace_free_space=False)


@functools.lru_cache(maxsize=None)
def _occ_ref(kind, n_inserts):
    ref = occmap_ref.OccMapRef(**occ_args(kind))
    for k in range(n_inserts):
        ref.insert(occ_scans(kind)[k], OCC_T[k], OCC_FAR if k else 0.0)
    cen = ref.centres()
    r = Ref(kind, oracle_c.Map(VS, 0).insert(cen) if len(cen) else oracle_c.Map(VS, 0), len(cen))
    r.cells = set(map(tuple, ref.download()[0][ref.download()[1] >= ref.l_occ].tolist()))
    return r


def _o_occmap_insert(kind):
    return _occ_ref(kind, 2), {}


def _d_occmap_insert(kind, dev):
    dev.occ.insert(dev.scan(occ_scans(kind)[1]), OCC_T[1], OCC_FAR)
    dev.m = dev.occ.search_map(VS)   # the handle is fetched again after the insert, as include/molahip.h requires


MUTATIONS = {name: SimpleNamespace(name=name, oracle=o, device=d) for name, o, d in [
    ("build_again", _o_build_again, _d_build_again),
    ("insert_far", _o_insert_far, _d_insert_far),
    ("insert_far_full_sort", _o_insert_far, _d_insert_far_full_sort),
    ("insert_frames", _o_insert_frames, _d_insert_frames),
    ("restore_over", _o_restore_over, _d_restore_over),
    ("erase_points", _o_erase_points, _d_erase_points),
    ("erase_queued", _o_erase_queued, _d_erase_queued),
    ("occmap_insert", _o_occmap_insert, _d_occmap_insert),
]}
QUEUED = ("insert_far", "insert_far_full_sort", "erase_queued")   # updates that leave their counts on the way
SECOND_CONTEXT_ROUTES = ("nn", "q", "f")
CASES = [(mu, k) for mu in MUTATIONS if mu != "occmap_insert" for k in KINDS] + [("occmap_insert", k) for k in OCC_KINDS]


def routes(kind):
    return mutation_routes(is_ndt(kind))


# what tests/test_gpu_map_mutations.py iterates: (mutation, kind, route name)
GPU_LIST = [(mu, k, r["name"]) for mu, k in CASES for r in routes(k)]


@functools.lru_cache(maxsize=None)
def after(mutation, kind):
    """(the reference after the update, what the update's oracle side noted)"""
    o = MUTATIONS[mutation].oracle
    return o(kind) if mutation != "insert_far_full_sort" else after("insert_far", kind)


def first_device_map(kind, ctx, dev=None):
    """the device map of before(kind) on `ctx`: (map handle, the occupancy map that owns it or None)"""
    if is_occ(kind):
        occ = capi.OccMap(ctx, **occ_args(kind))
        s = capi.Scan(ctx, occ_scans(kind)[0])
        occ.insert(s, OCC_T[0])
        s.close()
        return occ.search_map(VS), occ
    return first_state(kind, capi.Map(ctx, **map_params(kind, 0)), ctx), None


def first_state(kind, m, ctx):
    """bring a (used) handle of the kind to the state of before(kind)"""
    c, k = first_cloud(kind), N_FIRST_INSERTED[kind]
    m.build(c[:len(c) - k])
    if k:
        s = capi.Scan(ctx, c[len(c) - k:])
        m.insert(s, I12, 0.0)
        s.close()
    return m


def the_scan(kind):
    return occ_scan_queries() if is_occ(kind) else scan()


# ------------------------------------------------------------------------------------------------- partners (the CPU test's)
def partners(ref):
    """per point of the test scan under T0: (the device's global index of its partner or -1, the partner's voxel or None)"""
    s = the_scan(ref.kind)[:N_PARTNERS]
    r = ref.fix(oracle_c.match_points(ref.om, s, T0, THR_PARTNERS))
    idx = np.full(len(s), -1, np.int64)
    idx[r["local_idx"]] = r["global_idx"]
    vox = np.full((len(s), 3), np.iinfo(np.int64).min, np.int64)
    vox[r["local_idx"]] = voxel_of(ref.kind, r["global_xyz"])
    return idx, vox


# ------------------------------------------------------------------------------------------------ the routes' references
def align_params(mod, kind, inner=2, skip=False):
    """dense_cases.single_params at MUTATION_IT iterations; on the NDT kind both matchers of the lidar3d-ndt block"""
    kw = dict(max_iterations=MUTATION_IT, threshold=dc.schedule(MUTATION_IT), kernel_param=np.full(MUTATION_IT, 0.3),
              disable_stall_test=True)
    if is_ndt(kind):
        kw.update(gn=mod.GNParams(max_inner_iterations=inner), pt2pl_threshold=0.5)
        if skip:
            kw.update(matched_points=1) if mod is capi else kw.update(pt2pt_skip_plane_paired=True)
    else:
        kw.update(gn=mod.GNParams(max_inner_iterations=inner, robust_kernel=capi.KERNEL_GM_C4))
    return mod.ICPParams(**kw)


SCORE_THR, NN_THR, K3_THR, RADIUS, PL_THR = 0.5, 0.7, 1.0, 1.0, 0.5
BATCH_SIZES = (129, 2000, 2561)
BATCH_GUESSES = (T0, T1, T0)


@functools.lru_cache(maxsize=None)
def score_poses16():
    rng = np.random.default_rng(4290)
    return np.stack([dc.pose(*(np.array([0.46, -0.35, 0.13, 0.1, 0.02, -0.015]) + rng.uniform(-1, 1, 6) * [0.3, 0.3, 0.05, 0.03, 0.01, 0.01]))
                     for _ in range(16)])


@functools.lru_cache(maxsize=None)
def layer_cases(kind):
    """dense_cases-style multi-layer cases on the one map "m": name -> case"""
    s = the_scan(kind)[:2000]
    t, t2 = dc.schedule(MUTATION_IT), dc.schedule(MUTATION_IT, 1.2, 0.5)
    out = {
        "two_pairs": dict(kind="k", pairs=[dc._kp("m", s[0::2], t), dc._kp("m", s[1::2], t2, weight=0.25)]),
        "k2": dict(kind="k", pairs=[dc._kp("m", s[0::2], t, k=2), dc._kp("m", s[1::2], t2, k=2, weight=0.5)]),
        "plane_pair": dict(kind="pl", pairs=[dc._kp("m", s[0::2], t, k=2), dc._kp("m", s[1::2], np.full(MUTATION_IT, 0.4), plane=PLANE)]),
        "unique": dict(kind="k", pairs=[dc._kp("m", s[0::2], t, unique=1), dc._kp("m", s[1::2], t, weight=0.5, unique=1)]),
    }
    for c in out.values():
        c.update(max_it=MUTATION_IT, kp=np.full(MUTATION_IT, 0.3), inner=2, T0=T0, prior=None, pkw=dict(disable_stall_test=True))
    return out


def _oracle_align(ref, n, guess, inner, skip):
    return ref.fix(oracle_c.icp_align(ref.om, the_scan(ref.kind)[:n], guess, align_params(oracle_c, ref.kind, inner, skip), prior=prior(n),
                                      want_pairs=True))


def reference(ref, row):
    """the oracle's answer to a row of MUTATION_ROUTES on `ref`, computed once per reference and left unchanged"""
    kind, fam, name = ref.kind, row["family"], row["name"]
    s = the_scan(kind)
    if fam == "align":
        inner, skip = row.get("inner", 2), row.get("skip", False)
        return ref.once(("align", row["n"], inner, skip), lambda: _oracle_align(ref, row["n"], T0, inner, skip))
    if fam == "batch":
        return ref.once("batch", lambda: [_oracle_align(ref, n, T, 2, False) for n, T in zip(BATCH_SIZES, BATCH_GUESSES)])
    if fam == "layers":
        return ref.once(("layers", name), lambda: ref.fix(dc.case_reference(layer_cases(kind)[name], {"m": ref.om})))
    q = s[:2000]
    make = {
        "dense": lambda: ref.fix(oracle_c.match_points(ref.om, q, T0, 1e9)),
        "nn": lambda: ref.fix(oracle_c.match_points(ref.om, q, T0, NN_THR)),
        "nn_k3": lambda: ref.fix(oracle_c.match_points_k(ref.om, q, T0, K3_THR, 3)),
        "radius": lambda: rr.radius_search(ref.dump(), VS, s[:N_RADIUS], T0, RADIUS, sorted=False),
        "radius_sorted": lambda: rr.radius_search(ref.dump(), VS, s[:N_RADIUS], T0, RADIUS, sorted=True),
        "score16": lambda: sr.score_poses(oracle_c, ref.om, q, score_poses16(), SCORE_THR),
        "pt2pl": lambda: oracle_c.match_pt2pl(ref.om, q, T0, PL_THR),
        "pt2pl_knn": lambda: oracle_c.match_pt2pl_knn(ref.om, q, T0, 0.4, PLANE["plane_eigen_threshold"], PLANE["search_radius"],
                                                       PLANE["knn"], PLANE["minimum_plane_points"]),
    }[name]
    return ref.once(("query", name), make)


assert len({r["name"] for r in MUTATION_ROUTES}) == len(MUTATION_ROUTES)
