"""A restatement of include/molahip_replan.h and of the host rules of mola_lidar_odometry_hip/Replan.h, written from the two headers
alone.  The field after an update is NOT restated here: it is tests/plan_ref.py's Dijkstra on the current plane.  What is here:
n_withdrawn by peeling, straight from the definition of the largest self-supporting set K; withdraw-then-relax as whole-plane rounds,
which tests/test_replan_cpu.py holds against Dijkstra so that the peeling is known to mean what the header says; the counts of a patch;
the grown rectangle, the metre rectangle and the events text.  Nothing here is shaped like the device code (no tiles, no flags)."""
import numpy as np

import plan_ref as R

UNREACHED = R.UNREACHED
BIG = 1 << 62


def _pad(a, fill):
    out = np.full((a.shape[0] + 2, a.shape[1] + 2), fill, a.dtype)
    out[1:-1, 1:-1] = a
    return out


def _views(cost, price, below):
    """ok and price planes with a one-cell rim of impassable cells"""
    cost = np.asarray(cost, np.uint8)
    table = np.zeros(256, np.int64)
    table[:below] = np.asarray(price, np.int64)
    ok = cost < below
    return _pad(ok, False), _pad(np.where(ok, table[cost], 0), 0)


def _shift(a, dx, dy):
    """the plane of a's values at (x + dx, y + dy), a carrying a rim"""
    ny, nx = a.shape[0] - 2, a.shape[1] - 2
    return a[1 + dy:1 + dy + ny, 1 + dx:1 + dx + nx]


def _steps(ok, p):
    """per step of the field rule: (dx, dy, whether it exists from each cell, its weight)"""
    out = []
    for dx, dy, L in R.STEPS:
        allowed = _shift(ok, 0, 0) & _shift(ok, dx, dy)
        if dx and dy:
            allowed = allowed & _shift(ok, dx, 0) & _shift(ok, 0, dy)
        out.append((dx, dy, allowed, L * (_shift(p, 0, 0) + _shift(p, dx, dy))))
    return out


def kept(F, cost_new, price, below=253):
    """K as a boolean plane: peel, round by round, every cell that is not supported inside what is left"""
    F = np.asarray(F, np.uint32)
    ok, p = _views(cost_new, price, below)
    steps = _steps(ok, p)
    f = np.where(F == UNREACHED, BIG, F.astype(np.int64))
    S = _shift(ok, 0, 0) & (F != UNREACHED)
    while True:
        Sp, fp = _pad(S, False), _pad(f, BIG)
        held = f == 0
        for dx, dy, allowed, w in steps:
            held = held | (allowed & _shift(Sp, dx, dy) & (_shift(fp, dx, dy) + w <= f))
        nxt = S & held
        if (nxt == S).all():
            return S
        S = nxt


def n_withdrawn(F, cost_new, price, below=253):
    F = np.asarray(F, np.uint32)
    return int((F != UNREACHED).sum() - kept(F, cost_new, price, below).sum())


def repair(F, cost_new, goals_xy, price, below=253):
    """withdraw-then-relax as plain rounds over the whole plane: (the field, n_withdrawn)"""
    F = np.asarray(F, np.uint32)
    cost_new = np.asarray(cost_new, np.uint8)
    ny, nx = cost_new.shape
    K = kept(F, cost_new, price, below)
    f = np.where(K, F.astype(np.int64), BIG)
    for x, y in np.asarray(goals_xy, np.int64).reshape(-1, 2).tolist():
        if 0 <= x < nx and 0 <= y < ny and cost_new[y, x] < below:
            f[y, x] = 0
    ok, p = _views(cost_new, price, below)
    steps = _steps(ok, p)
    while True:
        fp = _pad(f, BIG)
        best = f.copy()
        for dx, dy, allowed, w in steps:
            best = np.minimum(best, np.where(allowed & (_shift(fp, dx, dy) < BIG), _shift(fp, dx, dy) + w, BIG))
        if (best == f).all():
            break
        f = best
    return np.where(f >= BIG, UNREACHED, f).astype(np.uint32), int((F != UNREACHED).sum() - K.sum())


def patch(cost, x0, y0, new, price, below=253):
    """(the new plane, n_cells_changed, n_cells_repriced)"""
    cost = np.asarray(cost, np.uint8)
    new = np.asarray(new, np.uint8)
    h, w = new.shape
    old = cost[y0:y0 + h, x0:x0 + w]
    table = np.zeros(256, np.int64)
    table[:below] = np.asarray(price, np.int64)
    out = cost.copy()
    out[y0:y0 + h, x0:x0 + w] = new
    return out, int((old != new).sum()), int((table[old] != table[new]).sum())


# ---- the host rules -----------------------------------------------------------------------------------------------------------------
def grown_rect(col0, row0, w, h, max_cells, nx, ny):
    """the rectangle grown by max_cells on every side and clipped to the window: (col0, row0, w, h)"""
    a, b = max(col0 - max_cells, 0), max(row0 - max_cells, 0)
    c, d = min(col0 + w + max_cells, nx), min(row0 + h + max_cells, ny)
    return a, b, c - a, d - b


def metre_rect(xa, ya, xb, yb, x0, y0, nx, ny, resolution):
    """the cells of a rectangle in metres: the floor rule on both corners, the range inclusive and clipped; (col0, row0, w, h), None when
    no cell is left; raises ValueError when a corner has no cell index"""
    ix = [R.cell_of(v, resolution) for v in (xa, xb)]
    iy = [R.cell_of(v, resolution) for v in (ya, yb)]
    if None in ix or None in iy:
        raise ValueError("a corner has no cell index")
    c0, c1 = max(min(ix) - x0, 0), min(max(ix) - x0, nx - 1)
    r0, r1 = max(min(iy) - y0, 0), min(max(iy) - y0, ny - 1)
    if c0 > c1 or r0 > r1:
        return None
    return c0, r0, c1 - c0 + 1, r1 - r0 + 1


def parse_events(text):
    """a list of (verb, numbers, line number); raises ValueError naming the line.  '#' begins a comment; blank lines are skipped."""
    out = []
    for n, line in enumerate(text.split("\n"), 1):
        tok = line.split("#", 1)[0].split()
        if not tok:
            continue
        want = {"block": 4, "clear": 4, "at": 2}.get(tok[0])
        if want is None:
            raise ValueError("events: line %d: unknown verb" % n)
        if len(tok) != 1 + want:
            raise ValueError("events: line %d: %s takes %d numbers" % (n, tok[0], want))
        try:
            v = [float(t) for t in tok[1:]]
        except ValueError:
            raise ValueError("events: line %d: not a number" % n)
        if not all(np.isfinite(v)) or any("x" in t.lower() or "_" in t for t in tok[1:]):        # (decimal, as strtod reads it whole)
            raise ValueError("events: line %d: not a finite decimal number" % n)
        out.append((tok[0], v, n))
    return out
