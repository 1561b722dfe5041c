"""mh_scan_merge_sensors restated in numpy, independent of the library (include/molahip.h has the arithmetic): every source's
points through its sensor pose in float64 with the written parentheses, rounded once to float32; its time stamps adjusted by
ITS min / max alone, in float32; the sources appended in order.  No `@`, no BLAS: their summation order is not the library's."""
import numpy as np

TS_NONE, TS_MIDDLE_IS_ZERO, TS_EARLIEST_IS_ZERO = 0, 1, 2
F = np.float32


def transform(P, xyz):
    """[n,3] float32 points through the row-major 3x4 pose P: (float)(((P[r,0]*x + P[r,1]*y) + P[r,2]*z) + P[r,3]), fp64."""
    P = np.asarray(P, np.float64).reshape(3, 4)
    p = np.asarray(xyz, F).reshape(-1, 3).astype(np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    out = np.empty((len(p), 3), F)
    for r in range(3):
        out[:, r] = (((P[r, 0] * x + P[r, 1] * y) + P[r, 2] * z) + P[r, 3]).astype(F)
    return out


def _ord(t):
    """The order-preserving unsigned image of float32 bits that the device's min / max reduction compares (-0 below +0)."""
    u = np.asarray(t, F).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def _unord(u):
    u = np.uint32(u)
    v = (u & np.uint32(0x7FFFFFFF)) if (u & np.uint32(0x80000000)) else np.uint32(~u)
    return np.array([v], np.uint32).view(F)[0]


def tmin_tmax(t):
    o = _ord(t)
    return _unord(o.min()), _unord(o.max())


def adjust(t, method, offset):
    """FilterAdjustTimestamps over one source's stamps: t' = (t - d) + offset in float32; TS_NONE: unchanged."""
    t = np.asarray(t, F)
    if method == TS_NONE or len(t) == 0:
        return t.copy()
    tmin, tmax = tmin_tmax(t)
    d = F(0.5) * (tmin + tmax) if method == TS_MIDDLE_IS_ZERO else tmin
    return ((t - F(d)) + F(offset)).astype(F)


def merge(sources):
    """sources: a list of dicts {xyz [n,3], t (or None), i (or None), pose (3x4 or None = identity), method, offset}.
    Returns dict(xyz, t, i): the sources appended in order; t / i are None when no non-empty source carries them."""
    live = [s for s in sources if len(s["xyz"])]
    has_t = bool(live) and all(s.get("t") is not None for s in live)
    has_i = bool(live) and all(s.get("i") is not None for s in live)
    assert has_t or not any(s.get("t") is not None for s in live), "a mix of sources with and without time stamps"
    assert has_i or not any(s.get("i") is not None for s in live), "a mix of sources with and without intensity"
    xyz, t, inten = [np.zeros((0, 3), F)], [np.zeros(0, F)], [np.zeros(0, F)]
    for s in live:
        P = np.eye(4)[:3] if s.get("pose") is None else s["pose"]
        xyz.append(transform(P, s["xyz"]))
        if has_t:
            t.append(adjust(s["t"], s.get("method", TS_NONE), s.get("offset", 0.0)))
        if has_i:
            inten.append(np.asarray(s["i"], F).copy())
    return dict(xyz=np.concatenate(xyz), t=np.concatenate(t) if has_t else None, i=np.concatenate(inten) if has_i else None)
