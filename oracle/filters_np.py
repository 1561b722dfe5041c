"""float32 numpy restatements of the device filters whose rules include/molahip.h states in full: FilterCurvature
(mh_scan_curvature), FilterNormalizeIntensity (mh_scan_normalize_intensity) and FilterByIntensity (mh_scan_by_intensity).

TEST INFRASTRUCTURE, like the rest of oracle/: tests/test_curvature.py and tests/test_intensity.py pin them on hand-built cases
and hold the device kernels to them bit for bit; oracle/chain_oracle.py runs filter chains on them."""
import numpy as np

LARGER, SMALLER, OTHER = 0, 1, 2  # FilterCurvature outputs
LOW, MID, HIGH = 0, 1, 2          # FilterByIntensity outputs


def curvature_classes(xyz, max_cosine=0.4, min_clearance=0.20, max_gap=1.0):
    """Class of every point (-1: end points, in no output), float32 throughout, in the order molahip.h writes it.  numpy's
    float32 +, -, *, / and sqrt are correctly rounded, and nothing here is fused."""
    p = np.asarray(xyz, np.float32).reshape(-1, 3)
    n = len(p)
    cls = np.full(n, -1, np.int64)
    if n < 3:
        return cls
    f = np.float32
    mc, mcl, mg = f(max_cosine), f(min_clearance), f(max_gap)
    gap2, clr2 = mg * mg, mcl * mcl
    with np.errstate(all="ignore"):
        a = p[1:-1] - p[:-2]
        b = p[2:] - p[1:-1]
        na = (a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2]
        nb = (b[:, 0] * b[:, 0] + b[:, 1] * b[:, 1]) + b[:, 2] * b[:, 2]
        dot = (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]
        c = dot / (np.sqrt(na) * np.sqrt(nb))
        gap = (na > gap2) | (nb > gap2)
        clear = (na < clr2) | (nb < clr2)
        inner = np.where(c < mc, LARGER, SMALLER)
    cls[1:-1] = np.where(gap | clear, OTHER, inner)
    return cls


def curvature_np(xyz, t=None, src=None, **kw):
    """The three outputs as dicts {xyz, t, src_idx} (t None without time stamps), in input order."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    cls = curvature_classes(xyz, **kw)
    src = np.arange(len(xyz), dtype=np.uint32) if src is None else np.asarray(src, np.uint32)
    out = []
    for k in (LARGER, SMALLER, OTHER):
        m = cls == k
        out.append(dict(xyz=xyz[m], t=None if t is None else np.asarray(t, np.float32)[m], src_idx=src[m]))
    return out


def _ord(a):
    """Order-preserving uint32 of float32 values (-0 < +0), what the device's min / max compare."""
    u = np.asarray(a, np.float32).view(np.uint32).astype(np.uint64)
    return np.where(u & 0x80000000, (~u) & 0xFFFFFFFF, u | 0x80000000).astype(np.uint64)


def normalize_np(i, range_=None):
    """FilterNormalizeIntensity as molahip.h states it: returns (new values, new range or None).  `range_` is the remembered
    {min, max} ({nan, nan}: none); None = remember_intensity_range false."""
    i = np.asarray(i, np.float32)
    f = np.float32
    good = i[~np.isnan(i)]
    lo = hi = f(np.nan)
    if len(good):
        o = _ord(good)
        lo, hi = good[np.argmin(o)], good[np.argmax(o)]
    if range_ is not None:
        rlo, rhi = f(range_[0]), f(range_[1])
        if not np.isnan(rlo) and (np.isnan(lo) or rlo < lo):
            lo = rlo
        if not np.isnan(rhi) and (np.isnan(hi) or rhi > hi):
            hi = rhi
    if np.isnan(lo) and np.isnan(hi):
        return i.copy(), (None if range_ is None else np.asarray(range_, np.float32).copy())
    with np.errstate(all="ignore"):
        d = f(hi - lo)
        k = f(f(1.0) / d) if d > 0 else f(0.0)
        out = ((i - lo) * k).astype(np.float32)
    return out, (None if range_ is None else np.array([lo, hi], np.float32))


def intensity_classes(i, low=0.1, high=0.9):
    i = np.asarray(i, np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(i < np.float32(low), LOW, np.where(i > np.float32(high), HIGH, MID))


def by_intensity_np(xyz, i, t=None, src=None, low=0.1, high=0.9):
    """The three outputs as dicts {xyz, t, i, src_idx} in input order."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    i = np.asarray(i, np.float32)
    cls = intensity_classes(i, low, high)
    src = np.arange(len(xyz), dtype=np.uint32) if src is None else np.asarray(src, np.uint32)
    return [dict(xyz=xyz[cls == k], t=None if t is None else np.asarray(t, np.float32)[cls == k], i=i[cls == k],
                 src_idx=src[cls == k]) for k in (LOW, MID, HIGH)]
