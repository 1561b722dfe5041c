"""The radius search of include/molahip.h (mh_nn_search_radius) restated in numpy, and the inputs its tests share.

The restatement is a brute force over ALL stored points with no voxel logic: the stored content and its order come from the
oracle's map (oracle_c.Map(...).insert(...) / .dump()), the query point is the fp64 -> fp32 transform of every other search,
d2 = (dx*dx + dy*dy) + dz*dz in fp32 (numpy's float32 arithmetic is un-fused), a result is d2 < (float)(radius * radius), visit
order is the order of the dump, and the sorted form is a stable argsort of d2.  No product code."""
import numpy as np

F = np.float32
IDENTITY = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float64)


def transform(xyz, T):
    """p' = (float)(R*l + t), fp64, in the operation order of transform_point"""
    T = np.asarray(T, np.float64).reshape(-1)[:12]
    l = np.asarray(xyz, F).reshape(-1, 3).astype(np.float64)
    with np.errstate(all="ignore"):
        cols = [((T[4 * r] * l[:, 0] + T[4 * r + 1] * l[:, 1]) + T[4 * r + 2] * l[:, 2]) + T[4 * r + 3] for r in range(3)]
        return np.stack(cols, 1).astype(F)


def r2_of(radius):
    return F(np.float64(radius) * np.float64(radius))


class Results:
    """offsets [n + 1] uint32; global_idx, pos (index in the dump), xyz [k, 3], d2 of all results, query after query"""

    def __init__(self, offsets, global_idx, pos, xyz, d2):
        self.offsets, self.global_idx, self.pos, self.xyz, self.d2 = offsets, global_idx, pos, xyz, d2

    def counts(self):
        return np.diff(self.offsets.astype(np.int64))

    def row(self, i):
        return slice(int(self.offsets[i]), int(self.offsets[i + 1]))


def radius_search(dump, voxel_size, queries, T, radius, sorted=False):
    """dump: what oracle_c.Map.dump() (or capi.Map.download()) returns; voxel_size only enters the guard of the query point."""
    pts, src = np.asarray(dump["xyz"], F).reshape(-1, 3), np.asarray(dump["src_idx"], np.uint32)
    p = transform(queries, T)
    r2 = r2_of(radius)
    inv_vs = F(1.0) / F(voxel_size)
    with np.errstate(all="ignore"):
        ok = (np.abs(p * inv_vs) < F(1.0e6)).all(axis=1)  # NaN and inf fail it as well
    offsets, gi, pos, d2s = [0], [], [], []
    for i in range(len(p)):
        hit, d2 = np.zeros(0, np.int64), np.zeros(0, F)
        if ok[i] and len(pts):
            d = pts - p[i]
            d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            hit = np.flatnonzero(d2 < r2)
            if sorted:
                hit = hit[np.argsort(d2[hit], kind="stable")]
        gi.append(src[hit])
        pos.append(hit.astype(np.int64))
        d2s.append(d2[hit])
        offsets.append(offsets[-1] + len(hit))
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)  # noqa: E731
    pos = cat(pos, np.int64)
    return Results(np.array(offsets, np.uint32), cat(gi, np.uint32), pos, pts[pos].reshape(-1, 3), cat(d2s, F))


def same(got, ref):
    """got: (offsets, global_idx, xyz, d2) of the product; every comparison bit for bit.  Returns None or what differs."""
    off, gi, xyz, d2 = got
    if not np.array_equal(np.asarray(off, np.uint32), ref.offsets):
        return "offsets"
    if not np.array_equal(np.asarray(gi, np.uint32), ref.global_idx):
        return "global_idx"
    if not np.array_equal(np.ascontiguousarray(xyz, F).view(np.uint32).reshape(-1, 3), ref.xyz.view(np.uint32).reshape(-1, 3)):
        return "xyz bits"
    if not np.array_equal(np.ascontiguousarray(d2, F).view(np.uint32), ref.d2.view(np.uint32)):
        return "d2 bits"
    return None


# ---- shared inputs ------------------------------------------------------------------------------------------------------------
RADII = (1e-3, 0.5, 1.0, 2.5)


def pose():
    """a non-identity fp64 pose: yaw 0.3, pitch -0.1, roll 0.05, translation (0.31, -0.27, 0.12)"""
    cy, sy, cp, sp, cr, sr = np.cos(0.3), np.sin(0.3), np.cos(-0.1), np.sin(-0.1), np.cos(0.05), np.sin(0.05)
    R = np.array([[cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr],
                  [sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr],
                  [-sp, cp * sr, cp * cr]])
    return np.concatenate([R, np.array([[0.31], [-0.27], [0.12]])], 1).reshape(12)


def capped_points():
    """about 3 000 points in a 6 m cube straddling the origin (voxel 1.0, cap 20: some voxels are full; TRUNC's voxel 0 is used)"""
    return np.random.default_rng(20261019).uniform(-3.0, 3.0, (3000, 3)).astype(F)


def capped_queries():
    """257 queries (4 waves + 1, no multiple of 64), a cube wider than the map's so that some have no neighbour at all"""
    return np.random.default_rng(7).uniform(-4.5, 4.5, (257, 3)).astype(F)


def second_keyframe():
    return np.random.default_rng(11).uniform(-2.0, 5.0, (1500, 3)).astype(F)


def dense_points():
    """three neighbouring voxels along z and three along x, 300 records each (uncapped): a run longer than a 64-record step and
    than the 31 records a voxel with quadrant boundaries can have"""
    rng = np.random.default_rng(3)
    corners = [[0, 0, 0], [0, 0, 1], [0, 0, 2], [1, 0, 0], [2, 0, 0]]
    return np.concatenate([rng.uniform(0.01, 0.99, (300, 3)) + np.array(c, np.float64) for c in corners]).astype(F)


def dense_queries():
    return np.random.default_rng(5).uniform(-0.5, 3.5, (70, 3)).astype(F)


def boundary_points():
    """Map points at voxel planes and one ulp to either side of them, for queries whose p' - r and p' + r lie exactly on those
    planes (identity pose); both signs, so that TRUNC's mirrored voxels are met too.  With them a point at exactly d2 == r2, a
    pair of duplicates (the sorted tie between different storage positions) and two different points at one distance."""
    pts = []
    for sgn in (1.0, -1.0):
        for plane in (1.0, 2.0, 3.0):
            v = F(plane)
            for x in (v, np.nextafter(v, F(0)), np.nextafter(v, F(10))):
                pts.append([sgn * x, sgn * F(0.5), sgn * F(0.5)])
                pts.append([sgn * F(0.5), sgn * x, sgn * F(0.5)])
                pts.append([sgn * F(0.5), sgn * F(0.5), sgn * x])
        pts += [[sgn * F(2.3), sgn * F(0.5), sgn * F(0.5)]] * 2   # duplicates
        pts.append([sgn * F(2.7), sgn * F(0.5), sgn * F(0.5)])    # as far from (2.5, .5, .5) as the duplicates
    return np.array(pts, F)


def boundary_queries():
    """(queries, radius) pairs: p' -+ r on voxel planes"""
    q = []
    for sgn in (1.0, -1.0):
        q += [[sgn * 2.5, sgn * 0.5, sgn * 0.5], [sgn * 0.5, sgn * 2.5, sgn * 0.5], [sgn * 0.5, sgn * 0.5, sgn * 2.5],   # r = 0.5
              [sgn * 2.0, sgn * 0.5, sgn * 0.5], [sgn * 0.5, sgn * 2.0, sgn * 0.5], [sgn * 0.5, sgn * 0.5, sgn * 2.0]]   # r = 1.0
    return np.array(q, F)


BOUNDARY_RADII = (0.5, 1.0)
