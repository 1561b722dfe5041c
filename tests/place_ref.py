"""The place descriptor and its search restated in numpy, straight from the text of include/molahip.h at mh_place_describe /
mh_place_search: tables built in float64 and rounded once to float32, point arithmetic in float32 (numpy does not fuse),
integer maxima and sums.  The device has to reproduce every byte and every match of this file."""
import numpy as np

F = np.float32
DEFAULT = dict(n_rings=20, n_sectors=64, min_range=1.0, max_range=80.0, z_min=-3.0, z_max=27.0)


def tables(n_rings, n_sectors, min_range, max_range, z_min, z_max):
    R, S = int(n_rings), int(n_sectors)
    r0, r1, z0, z1 = (float(F(v)) for v in (min_range, max_range, z_min, z_max))  # the struct holds floats
    k = np.arange(R + 1, dtype=np.float64)
    e = r0 + k * (r1 - r0) / R
    ring_edge2 = (e * e).astype(F)
    j = np.arange(S // 8, dtype=np.float64)
    tan_edge = np.tan(2.0 * np.pi * j / S).astype(F)  # [0] unused
    zscale = F(254.0 / (z1 - z0))
    return dict(R=R, S=S, ring_edge2=ring_edge2, tan_edge=tan_edge, z_min=F(z0), z_max=F(z1), zscale=zscale)


def bins(xyz, **params):
    """(kept mask, ring, sector, level) of every point."""
    t = tables(**params)
    R, S = t["R"], t["S"]
    p = np.asarray(xyz, dtype=F).reshape(-1, 3)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        r2 = x * x + y * y
        keep = np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
        keep &= ~((x == 0) & (y == 0))
        keep &= (r2 >= t["ring_edge2"][0]) & (r2 < t["ring_edge2"][R])
        keep &= (z >= t["z_min"]) & (z < t["z_max"])
        ring = np.zeros(len(p), np.int64)
        for k in range(1, R):
            ring += t["ring_edge2"][k] <= r2
        zz = np.where(keep, z, t["z_min"])
        level = np.minimum(255, 1 + ((zz - t["z_min"]) * t["zscale"]).astype(np.uint32).astype(np.int64))
        c0 = (x > 0) & (y >= 0)
        c1 = (x <= 0) & (y > 0)
        c2 = (x < 0) & (y <= 0)
        Q = np.where(c0, 0, np.where(c1, 1, np.where(c2, 2, 3)))
        a = np.where(c0, x, np.where(c1, y, np.where(c2, -x, -y))).astype(F)
        b = np.where(c0, y, np.where(c1, -x, np.where(c2, -y, x))).astype(F)
        E = S // 8
        lo = np.zeros(len(p), np.int64)
        hi = np.zeros(len(p), np.int64)
        for j in range(1, E):
            lo += b >= t["tan_edge"][j] * a
            hi += a > t["tan_edge"][j] * b
        o = np.where(b < a, lo, (2 * E - 1) - hi)
    sector = Q * (S // 4) + o
    return keep, ring, sector, level


def describe(xyz, **params):
    """uint8 [R, S]: the maximum level per bin, 0 = empty."""
    R, S = int(params["n_rings"]), int(params["n_sectors"])
    keep, ring, sector, level = bins(xyz, **params)
    d = np.zeros(R * S, np.int64)
    np.maximum.at(d, (ring * S + sector)[keep], level[keep])
    return d.reshape(R, S).astype(np.uint8)


def distances(stored, query):
    """D[k, s] = sum |q[r][(c + s) mod S] - d_k[r][c]| for every stored descriptor and shift: int64 [K, S]."""
    d = np.asarray(stored, np.uint8)
    q = np.asarray(query, np.uint8)
    S = q.shape[-1]
    d = d.reshape(-1, q.shape[0], S).astype(np.int64)
    out = np.zeros((len(d), S), np.int64)
    for s in range(S):
        out[:, s] = np.abs(np.roll(q, -s, axis=1).astype(np.int64)[None] - d).sum(axis=(1, 2))
    return out


def search(stored, query):
    """(shift [K], dist [K]): the smallest D per stored descriptor, ties to the smallest shift."""
    D = distances(stored, query)
    if len(D) == 0:
        return np.zeros(0, np.uint32), np.zeros(0, np.uint32)
    s = np.argmin(D, axis=1)  # (the first minimum)
    return s.astype(np.uint32), D[np.arange(len(D)), s].astype(np.uint32)


def quarter_turn(xyz):
    """(x, y) -> (-y, x): exact in floating point."""
    p = np.asarray(xyz, dtype=F).reshape(-1, 3)
    return np.stack([-p[:, 1], p[:, 0], p[:, 2]], 1)


def edge_cloud(n, seed, **params):
    """n points (float32 [n, 3]) for the byte-for-byte comparisons: random points in and around the annulus and the z window,
    mixed with points placed exactly on what decides a bin -- ring edges (sqrt of the table values and their fp32 neighbours, on
    an axis and on a diagonal), sector boundaries (axes, diagonals, b == tan_edge[j] * a in every octant), the origin, NaN / inf,
    both ends of the z window, the level steps.  The special points come first in a seeded shuffle, so a short cloud holds some."""
    t = tables(**params)
    R, S = t["R"], t["S"]
    rng = np.random.default_rng(seed)
    r0, r1 = float(np.sqrt(np.float64(t["ring_edge2"][0]))), float(np.sqrt(np.float64(t["ring_edge2"][R])))
    z0, z1 = float(t["z_min"]), float(t["z_max"])
    zmid = F(0.5 * (z0 + z1))
    sp = []
    for k in range(R + 1):  # ring edges
        r = F(np.sqrt(np.float64(t["ring_edge2"][k])))
        for v in (np.nextafter(r, F(0)), r, np.nextafter(r, F(np.inf))):
            sp += [(v, 0, zmid), (0, -v, zmid)]
            h = F(np.float64(v) / np.sqrt(2.0))
            sp += [(h, h, zmid), (-h, np.nextafter(h, F(np.inf)), zmid)]
    rmid = F(0.5 * (r0 + r1) / 1.5)
    for a in (rmid, F(rmid * F(0.37)), F(rmid * F(1.21))):  # sector boundaries
        sp += [(a, 0, zmid), (-a, 0, zmid), (0, a, zmid), (0, -a, zmid), (a, a, zmid), (-a, a, zmid), (-a, -a, zmid), (a, -a, zmid),
               (a, -0.0, zmid), (-0.0, a, zmid)]
        for j in range(1, S // 8):
            b = F(t["tan_edge"][j] * a)
            for bb in (np.nextafter(b, F(0)), b, np.nextafter(b, F(np.inf))):
                sp += [(a, bb, zmid), (-bb, a, zmid), (-a, -bb, zmid), (bb, -a, zmid),   # b < a side of each quadrant
                       (bb, a, zmid), (-a, bb, zmid), (-bb, -a, zmid), (a, -bb, zmid)]  # the mirrored octants
    sp += [(0, 0, zmid), (-0.0, 0.0, zmid), (np.nan, 1, zmid), (rmid, np.inf, zmid), (rmid, 1, np.nan), (-np.inf, 0, zmid),
           (rmid, 1, np.inf), (F(3e38), F(3e38), zmid)]
    for z in (z0, z1):  # both ends of the z window
        zf = F(z)
        sp += [(rmid, 1, np.nextafter(zf, F(-np.inf))), (rmid, 2, zf), (rmid, 3, np.nextafter(zf, F(np.inf)))]
    for m in list(range(0, 6)) + list(range(120, 126)) + list(range(249, 256)):  # the level steps
        z = F(z0 + m / float(t["zscale"]))
        for v in (np.nextafter(z, F(-np.inf)), z, np.nextafter(z, F(np.inf))):
            sp.append((-rmid, F(m % 7) - 3, v))
    sp = np.array(sp, dtype=F)
    sp = sp[rng.permutation(len(sp))]
    m = max(n - len(sp), n // 2)
    ang = rng.uniform(0, 2 * np.pi, m)
    rad = rng.uniform(max(0.0, r0 - 0.1 * (r1 - r0)), r1 + 0.1 * (r1 - r0), m)
    rnd = np.stack([rad * np.cos(ang), rad * np.sin(ang), rng.uniform(z0 - 0.1 * (z1 - z0), z1 + 0.1 * (z1 - z0), m)], 1).astype(F)
    out = np.concatenate([sp[:n - m], rnd], 0)[:n]
    return np.ascontiguousarray(out[rng.permutation(len(out))])


def rank(shift, dist):
    """frames ordered by (dist ascending, frame ascending)."""
    return np.lexsort((np.arange(len(dist)), np.asarray(dist)))
