"""See-through voting on key-frame views restated in numpy, straight from the text of include/molahip_clean.h: tables built in
float64 and rounded once to float32, point arithmetic in float32 (numpy does not fuse), integer minima and counts.  The device
has to reproduce every word of this file; the host rules of MapCleaning.h (neighbours, relative pose, decision) are folded here
too."""
import numpy as np

F = np.float32
EMPTY = np.uint32(0xFFFFFFFF)
DEFAULT = dict(n_rings=32, n_sectors=128, el_min=float(np.radians(-25.0)), el_max=float(np.radians(15.0)), min_range=2.0,
               max_range=60.0, rel_margin=0.10, origin=(0.0, 0.0, 0.0), win_rings=0, win_sectors=1)
HOST_DEFAULT = dict(max_view_distance=30.0, max_views_per_frame=24, min_through_votes=2, agree_weight=1)


def tables(n_rings, n_sectors, el_min, el_max, min_range, max_range, rel_margin, origin, win_rings, win_sectors):
    A, S = int(n_rings), int(n_sectors)
    e0, e1, r0, r1, mg = (float(F(v)) for v in (el_min, el_max, min_range, max_range, rel_margin))  # the struct holds floats
    j = np.arange(S // 8, dtype=np.float64)
    tan_edge = np.tan(2.0 * np.pi * j / S).astype(F)  # [0] unused
    k = np.arange(A + 1, dtype=np.float64)
    e = e0 + k * (e1 - e0) / A
    tn = np.tan(e)
    return dict(A=A, S=S, tan_edge=tan_edge, el_tan2=(tn * tn).astype(F), el_sign=np.sign(e).astype(np.int64),
                min_r2=F(r0 * r0), max_r2=F(r1 * r1), far2=F((1.0 + mg) * (1.0 + mg)), origin=np.asarray(origin, F),
                wr=int(win_rings), ws=int(win_sectors))


def _above(t, k, h2, z, zz):
    m = t["el_tan2"][k] * h2
    s = t["el_sign"][k]
    if s > 0:
        return (z > 0) & (zz >= m)
    if s == 0:
        return z >= 0
    return (z >= 0) | (zz <= m)


def _sector(t, x, y):
    S = t["S"]
    c0 = (x > 0) & (y >= 0)
    c1 = (x <= 0) & (y > 0)
    c2 = (x < 0) & (y <= 0)
    Q = np.where(c0, 0, np.where(c1, 1, np.where(c2, 2, 3)))
    a = np.where(c0, x, np.where(c1, y, np.where(c2, -x, -y))).astype(F)
    b = np.where(c0, y, np.where(c1, -x, np.where(c2, -y, x))).astype(F)
    E = S // 8
    lo = np.zeros(len(x), np.int64)
    hi = np.zeros(len(x), np.int64)
    for j in range(1, E):
        lo += b >= t["tan_edge"][j] * a
        hi += a > t["tan_edge"][j] * b
    return Q * (S // 4) + np.where(b < a, lo, (2 * E - 1) - hi)


def bins(xyz, t):
    """(kept mask, ring, sector, r2 float32) of every point given in the vehicle frame; t = tables(**params)."""
    p = np.asarray(xyz, dtype=F).reshape(-1, 3)
    with np.errstate(all="ignore"):
        x, y, z = p[:, 0] - t["origin"][0], p[:, 1] - t["origin"][1], p[:, 2] - t["origin"][2]
        h2 = x * x + y * y
        zz = z * z
        r2 = h2 + zz
        keep = np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
        keep &= ~((x == 0) & (y == 0))
        keep &= (r2 >= t["min_r2"]) & (r2 < t["max_r2"])
        keep &= _above(t, 0, h2, z, zz) & ~_above(t, t["A"], h2, z, zz)
        ring = np.zeros(len(p), np.int64)
        for k in range(1, t["A"]):
            ring += _above(t, k, h2, z, zz)
        sector = _sector(t, x, y)
    return keep, ring, sector, r2.astype(F)


def view(xyz, **params):
    """uint32 [A, S]: the bits of the smallest r2 per bin, 0xFFFFFFFF = empty."""
    t = tables(**params)
    keep, ring, sector, r2 = bins(xyz, t)
    v = np.full(t["A"] * t["S"], EMPTY, np.uint32)
    np.minimum.at(v, (ring * t["S"] + sector)[keep], r2.view(np.uint32)[keep])
    return v.reshape(t["A"], t["S"])


def transform(T, xyz):
    """(float)(((T0*px + T1*py) + T2*pz) + T3) per row, in float64."""
    T = np.asarray(T, np.float64).reshape(12)
    p = np.asarray(xyz, dtype=F).reshape(-1, 3).astype(np.float64)
    with np.errstate(all="ignore"):
        rows = [((T[4 * r] * p[:, 0] + T[4 * r + 1] * p[:, 1]) + T[4 * r + 2] * p[:, 2]) + T[4 * r + 3] for r in range(3)]
        return np.stack(rows, 1).astype(F)


def evidence(xyz, view_j, T, t):
    """(through mask, agree mask) of every point against one view under T."""
    A, S = t["A"], t["S"]
    img = np.asarray(view_j, np.uint32).reshape(A, S)
    keep, ring, sector, r2q = bins(transform(T, xyz), t)
    with np.errstate(all="ignore"):
        lim = r2q * t["far2"]
        all_far = keep.copy()
        for dr in range(-t["wr"], t["wr"] + 1):
            rr = ring + dr
            inside = (rr >= 0) & (rr < A)
            rc = np.clip(rr, 0, A - 1)
            for ds in range(-t["ws"], t["ws"] + 1):
                w = img[rc, (sector + ds) % S]
                all_far &= ~inside | ((w != EMPTY) & (w.view(F) > lim))
        own = img[ring, sector]
        r2o = own.view(F)
        agree = keep & ~all_far & (own != EMPTY) & (r2q <= r2o * t["far2"]) & (r2o <= lim)
    return all_far, agree


def vote(xyz, views, nbr_view, nbr_T, weights=None, **params):
    """uint32 [n]: through | agree << 16 of one frame's points against the views nbr_view[k] under nbr_T[k]; weights[k] counts
    entry k that many times (a list that repeats one entry)."""
    t = tables(**params)
    n = len(np.asarray(xyz).reshape(-1, 3))
    th = np.zeros(n, np.int64)
    ag = np.zeros(n, np.int64)
    nbr_T = np.asarray(nbr_T, np.float64).reshape(-1, 12)
    for k, j in enumerate(nbr_view):
        a, b = evidence(xyz, views[j], nbr_T[k], t)
        w = 1 if weights is None else int(weights[k])
        th += w * a
        ag += w * b
    return (np.minimum(th, 65535) | (np.minimum(ag, 65535) << 16)).astype(np.uint32)


def relative_pose(T_i, T_j):
    """T_j^-1 T_i entry by entry as molahip_clean.h states it; poses are 3x4 (or 12) float64 rigid transforms."""
    Ti = np.asarray(T_i, np.float64).reshape(-1)[:12].reshape(3, 4)
    Tj = np.asarray(T_j, np.float64).reshape(-1)[:12].reshape(3, 4)
    out = np.zeros((3, 4))
    d = [Ti[m, 3] - Tj[m, 3] for m in range(3)]
    for r in range(3):
        for c in range(3):
            out[r, c] = (Tj[0, r] * Ti[0, c] + Tj[1, r] * Ti[1, c]) + Tj[2, r] * Ti[2, c]
        out[r, 3] = (Tj[0, r] * d[0] + Tj[1, r] * d[1]) + Tj[2, r] * d[2]
    return out.reshape(12)


def neighbours(poses, has_points, max_view_distance=30.0, max_views_per_frame=24, **_):
    """cleaning_neighbours: for frame i the frames j != i with points whose positions lie within max_view_distance (squared
    distance ((dx*dx + dy*dy) + dz*dz) <= d*d in float64), the nearest max_views_per_frame of them, ties to the lower index, in
    ascending index order.  A frame without points has no neighbours."""
    P = [np.asarray(T, np.float64).reshape(-1)[:12].reshape(3, 4)[:, 3] for T in poses]
    lim = float(max_view_distance) * float(max_view_distance)
    out = []
    for i in range(len(P)):
        cand = []
        if has_points[i]:
            for j in range(len(P)):
                if j == i or not has_points[j]:
                    continue
                dx, dy, dz = P[j][0] - P[i][0], P[j][1] - P[i][1], P[j][2] - P[i][2]
                d2 = (dx * dx + dy * dy) + dz * dz
                if d2 <= lim:
                    cand.append((d2, j))
        cand.sort()
        out.append(sorted(j for _, j in cand[:int(max_views_per_frame)]))
    return out


def decide(votes, min_through_votes=2, agree_weight=1, **_):
    """True: the point is removed."""
    v = np.asarray(votes, np.uint32).astype(np.int64)
    th, ag = v & 0xFFFF, v >> 16
    return (th >= int(min_through_votes)) & (th > int(agree_weight) * ag)


def clean(frames, poses, params=None, host=None):
    """The whole call on lists of xyz [n, 3] and poses: (removed masks, votes, neighbour lists)."""
    params = dict(DEFAULT, **(params or {}))
    host = dict(HOST_DEFAULT, **(host or {}))
    has = [len(f) > 0 for f in frames]
    nb = neighbours(poses, has, **host)
    views = [view(f, **params) for f in frames]
    votes, masks = [], []
    for i, f in enumerate(frames):
        v = vote(f, views, nb[i], [relative_pose(poses[i], poses[j]) for j in nb[i]], **params)
        votes.append(v)
        masks.append(decide(v, **host))
    return masks, votes, nb


def quarter_turn(xyz):
    """(x, y) -> (-y, x): exact in floating point."""
    p = np.asarray(xyz, dtype=F).reshape(-1, 3)
    return np.stack([-p[:, 1], p[:, 0], p[:, 2]], 1)


def edge_cloud(n, seed, **params):
    """n points (float32 [n, 3]) for the word-for-word comparisons: random points in and around the shell and the elevation
    window, mixed with points placed exactly on what decides a bin -- axes, diagonals and sector boundaries, elevation edges
    (z = +-sqrt(el_tan2[k]) * h and its fp32 neighbours, the two limits included), exactly min_range and max_range, the origin,
    NaN / inf.  The special points come first in a seeded shuffle, so a short cloud holds some.  Coordinates are relative to
    the origin parameter, which is added at the end."""
    t = tables(**params)
    A, S = t["A"], t["S"]
    rng = np.random.default_rng(seed)
    r0, r1 = float(np.sqrt(np.float64(t["min_r2"]))), float(np.sqrt(np.float64(t["max_r2"])))
    rmid = F(0.5 * (r0 + r1) / 1.5)
    up, dn = (lambda v: np.nextafter(F(v), F(np.inf))), (lambda v: np.nextafter(F(v), F(-np.inf)))
    sp = []
    for a in (rmid, F(rmid * F(0.37))):  # sector boundaries, at level height
        sp += [(a, 0, 0), (-a, 0, 0), (0, a, 0), (0, -a, 0), (a, a, 0), (-a, a, 0), (-a, -a, 0), (a, -a, 0), (a, -0.0, -0.0),
               (-0.0, a, 0)]
        for j in range(1, S // 8):
            b = F(t["tan_edge"][j] * a)
            for bb in (dn(b), b, up(b)):
                sp += [(a, bb, 0), (-bb, a, 0), (-a, -bb, 0), (bb, -a, 0), (bb, a, 0), (-a, bb, 0), (-bb, -a, 0), (a, -bb, 0)]
    for k in range(A + 1):  # elevation edges: h = 8 and h = 8 * sqrt(2) on a diagonal, z on the edge and beside it
        tk = np.sqrt(np.float64(t["el_tan2"][k])) * (1.0 if t["el_sign"][k] >= 0 else -1.0)
        for (x, y) in ((F(8), F(0)), (F(-8), F(8)), (F(3), F(-5))):
            h = np.sqrt(np.float64(x) ** 2 + np.float64(y) ** 2)
            z = F(tk * h)
            sp += [(x, y, dn(z)), (x, y, z), (x, y, up(z))]
    for r in (r0, r1):  # exactly on the range limits (on an axis r2 = r * r is exact when r is short in binary)
        rf = F(r)
        sp += [(dn(rf), 0, 0), (rf, 0, 0), (up(rf), 0, 0), (0, -rf, 0), (0, rf, -0.0)]
    sp += [(0, 0, rmid), (-0.0, 0.0, 1), (np.nan, 1, 0), (rmid, np.inf, 0), (rmid, 1, np.nan), (-np.inf, 0, 0), (rmid, 1, np.inf),
           (F(3e38), F(3e38), 0), (F(1e-30), F(1e-30), rmid), (rmid, 1, -rmid), (rmid, 1, F(5) * rmid)]
    sp = np.array(sp, dtype=F)
    sp = sp[rng.permutation(len(sp))]
    m = max(n - len(sp), n // 2)
    ang = rng.uniform(0, 2 * np.pi, m)
    rad = rng.uniform(0.5 * r0, 1.1 * r1, m)
    e0, e1 = float(F(params["el_min"])), float(F(params["el_max"]))
    el = rng.uniform(e0 - 0.1 * (e1 - e0), e1 + 0.1 * (e1 - e0), m)
    rnd = np.stack([rad * np.cos(el) * np.cos(ang), rad * np.cos(el) * np.sin(ang), rad * np.sin(el)], 1).astype(F)
    out = np.concatenate([sp[:n - m], rnd], 0)[:n]
    out = out[rng.permutation(len(out))] + np.asarray(params["origin"], F)[None]
    return np.ascontiguousarray(out.astype(F))
