"""The scan pre-processing chain of mh_preprocess.hip restated in plain numpy, independent of the library and of the C oracle
(include/molahip.h has the arithmetic): FilterAdjustTimestamps, both FilterDecimateVoxels methods, FilterByRange,
FilterBoundingBox, their chain, the bounding box and FilterDeskew.  Everything the device does in float32 is float32 here with
the written parentheses; the min / max of the stamps and of the box are numpy's own (the device's ordered-uint image of the
float bits is what the tests hold against this, so it is not restated); de-skew is long double so that callers can measure
both the device and the oracle against it."""
import numpy as np

F = np.float32
L = np.longdouble
TS_NONE, TS_MIDDLE_IS_ZERO, TS_EARLIEST_IS_ZERO = 0, 1, 2
INDEX_FLOOR, INDEX_TRUNC = 0, 1
FIRST_POINT, CLOSEST_TO_AVERAGE = 0, 1
BBOX_OFF, BBOX_KEEP_OUTSIDE, BBOX_KEEP_INSIDE = 0, 1, 2
KEY_LIMIT = F(1.0e6)  # |coordinate * (1 / resolution)| below this on every axis fits the packed voxel key

# the parameters of a chain: the keyword arguments of capi.preprocess_params / oracle_c.preprocess, stages off
PARAMS = dict(decim_map_resolution=0.0, decim_icp_resolution=0.0, min_points_to_filter=0, index_mode=INDEX_FLOOR, range_min=0.0,
              range_max=0.0, range_center=(0.0, 0.0, 0.0), bbox_mode=BBOX_OFF, bbox_min=(0.0, 0.0, 0.0), bbox_max=(0.0, 0.0, 0.0),
              decim_map_method=FIRST_POINT, decim_icp_method=FIRST_POINT)


def params(**kw):
    assert set(kw) <= set(PARAMS), sorted(set(kw) - set(PARAMS))
    return dict(PARAMS, **kw)


def _xyz(xyz):
    return np.asarray(xyz, F).reshape(-1, 3)


def finite_rows(xyz):
    return np.isfinite(_xyz(xyz)).all(axis=1)


def adjust(t, method, offset):
    """FilterAdjustTimestamps: t' = (t - d) + offset in float32, d = 0.5f * (tmin + tmax) or tmin over ALL stamps."""
    t = np.asarray(t, F)
    if method == TS_NONE or len(t) == 0:
        return t.copy()
    tmin, tmax = t.min(), t.max()
    d = F(0.5) * F(tmin + tmax) if method == TS_MIDDLE_IS_ZERO else tmin
    return ((t - F(d)) + F(offset)).astype(F)


def cells(xyz, res, index_mode):
    """([n,3] int64 cell of every row, [n] bool: the row is finite and |s| < 1e6 on every axis), s = x * (1.0f / res) in
    float32; floor or truncation of s per index_mode.  Rows that are not finite get cell 0."""
    p = _xyz(xyz)
    fin = finite_rows(p)
    inv = F(1) / F(res)
    s = (np.where(fin[:, None], p, F(0)) * inv).astype(F)
    c = (np.trunc(s) if index_mode == INDEX_TRUNC else np.floor(s)).astype(np.int64)
    return c, fin & (np.abs(s) < KEY_LIMIT).all(axis=1)


def _groups(xyz, res, index_mode):
    """(rows: ascending indices of the finite rows, inverse: the cell number of each of them)"""
    c, _ = cells(xyz, res, index_mode)
    rows = np.nonzero(finite_rows(xyz))[0]
    if not len(rows):
        return rows, np.zeros(0, np.int64)
    _, inverse = np.unique(c[rows], axis=0, return_inverse=True)
    return rows, np.asarray(inverse).reshape(-1)


def decimate_first(xyz, res, min_points, index_mode):
    """FirstPoint: the smallest index of every cell over the finite rows, ascending; an input below min_points, or res <= 0,
    passes all its finite rows."""
    p = _xyz(xyz)
    if res <= 0 or len(p) < min_points:
        return np.nonzero(finite_rows(p))[0].astype(np.uint32)
    rows, inv = _groups(p, res, index_mode)
    first = np.full(inv.max() + 1 if len(inv) else 0, len(p), np.int64)
    np.minimum.at(first, inv, rows)
    return np.sort(first).astype(np.uint32)


def decimate_closest(xyz, res, min_points, index_mode):
    """ClosestToAverage: per cell mean = (float32 sum of its rows in input order) * (1.0f / count); the survivor is the first
    row strictly closest to it, error (dx*dx + dy*dy) + dz*dz in float32."""
    p = _xyz(xyz)
    if res <= 0 or len(p) < min_points:
        return np.nonzero(finite_rows(p))[0].astype(np.uint32)
    rows, inv = _groups(p, res, index_mode)
    order = np.argsort(inv, kind="stable")  # input order inside a cell
    bounds = np.nonzero(np.diff(inv[order], prepend=-1, append=-2))[0]
    out = []
    for a, b in zip(bounds[:-1], bounds[1:]):
        idx = rows[order[a:b]]
        q = p[idx]
        mean = np.add.accumulate(q, axis=0, dtype=F)[-1] * (F(1) / F(b - a))  # (accumulate adds one after the other)
        d = q - mean.astype(F)
        e = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        out.append(idx[int(np.argmin(e))])  # (argmin: the first of equals)
    return np.sort(np.asarray(out, np.int64)).astype(np.uint32)


def decimate(xyz, res, min_points, index_mode, method):
    return (decimate_closest if method == CLOSEST_TO_AVERAGE else decimate_first)(xyz, res, min_points, index_mode)


def range_sq(xyz, center):
    p = _xyz(xyz)
    c = np.asarray(center, F)
    dx, dy, dz = p[:, 0] - c[0], p[:, 1] - c[1], p[:, 2] - c[2]
    return ((dx * dx + dy * dy) + dz * dz).astype(F)


def by_range(xyz, range_min, range_max, center):
    """FilterByRange: keep mask; the band is inclusive; the stage is skipped when range_max <= 0."""
    if range_max <= 0:
        return np.ones(len(_xyz(xyz)), bool)
    sq = range_sq(xyz, center)
    return (sq >= F(range_min) * F(range_min)) & (sq <= F(range_max) * F(range_max))


def by_box(xyz, bmin, bmax, mode):
    """FilterBoundingBox: keep mask; the faces belong to the inside."""
    p = _xyz(xyz)
    if mode == BBOX_OFF:
        return np.ones(len(p), bool)
    inside = ((p >= np.asarray(bmin, F)) & (p <= np.asarray(bmax, F))).all(axis=1)
    return inside if mode == BBOX_KEEP_INSIDE else ~inside


def chain(xyz, pp):
    """raw -> decimate(map res) -> by-range -> bounding box -> idx_map -> decimate(icp res) -> idx_icp: indices into the raw
    scan, ascending.  The second decimation's minimum counts what the first stage left."""
    p = _xyz(xyz)
    cur = decimate(p, pp["decim_map_resolution"], pp["min_points_to_filter"], pp["index_mode"], pp["decim_map_method"]).astype(np.int64)
    cur = cur[by_range(p[cur], pp["range_min"], pp["range_max"], pp["range_center"])]
    cur = cur[by_box(p[cur], pp["bbox_min"], pp["bbox_max"], pp["bbox_mode"])]
    sel = decimate(p[cur], pp["decim_icp_resolution"], pp["min_points_to_filter"], pp["index_mode"], pp["decim_icp_method"])
    return cur.astype(np.uint32), cur[sel].astype(np.uint32)


def bbox(xyz):
    """(min[3], max[3], count) over the rows whose three coordinates are finite; zeros and 0 when there are none."""
    p = _xyz(xyz)
    q = p[finite_rows(p)]
    if not len(q):
        return np.zeros(3, F), np.zeros(3, F), 0
    return q.min(axis=0), q.max(axis=0), len(q)


SERIES_BELOW = L(1.0e-4)  # below: three series terms of sin(th)/th and (1 - cos th)/th^2; the fourth is < 1e-20 relative


def deskew(xyz, t, twist):
    """FilterDeskew in long double: p' = Exp_SO3(w t) p + v t, twist = (vx, vy, vz, wx, wy, wz); closed-form Rodrigues,
    R p = p + a (u x p) + b (u x (u x p)) with u = w t, a = sin(th)/th, b = 2 sin^2(th/2)/th^2.  Returns [n,3] long double."""
    p = _xyz(xyz).astype(L)
    tt = np.asarray(t, F).astype(L)[:, None]
    tw = np.asarray(twist, np.float64).astype(L)
    u = tw[None, 3:] * tt
    th2 = (u * u).sum(axis=1)
    th = np.sqrt(th2)
    small = th < SERIES_BELOW
    ths = np.where(small, L(1), th)
    sh = np.sin(L(0.5) * ths)
    a = np.where(small, L(1) - th2 / L(6) + th2 * th2 / L(120), np.sin(ths) / ths)
    b = np.where(small, L(0.5) - th2 / L(24) + th2 * th2 / L(720), L(2) * sh * sh / (ths * ths))
    up = np.cross(u, p)
    uup = np.cross(u, up)
    return p + a[:, None] * up + b[:, None] * uup + tw[None, :3] * tt


def deskew_bound(xyz, t, twist, ref):
    """The bound on |device - ref| per coordinate, derived and not measured: the kernel computes in fp64 and rounds once to
    float, so one float ulp at |ref| (a half-ulp rounding can land on either side), plus c * 2^-52 * (|x| + |y| + |z| + |v t|)
    with c = 16 for the roughly dozen fp64 operations and the 1-2 ulp device sin in front of the rounding.  The second term is
    ~1e7 times smaller than the first and matters only where the sum cancels to near zero."""
    p = np.abs(_xyz(xyz).astype(L))
    vt = np.sqrt((np.asarray(twist, np.float64)[:3].astype(L) ** 2).sum()) * np.abs(np.asarray(t, F).astype(L))
    ulp = np.spacing(np.abs(np.asarray(ref, L)).astype(F)).astype(L)
    return ulp + (L(16) * L(2) ** -52 * (p.sum(axis=1) + vt))[:, None]


def ulps32(got, ref):
    """|got - ref| in float32 ulps at |ref|, elementwise (ref may be long double)"""
    ref = np.asarray(ref, L)
    return np.abs(np.asarray(got, F).astype(L) - ref) / np.spacing(np.abs(ref).astype(F)).astype(L)
