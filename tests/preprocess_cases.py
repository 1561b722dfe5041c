"""Case tables for the first-generation scan kernels of mh_preprocess.hip (time-stamp min / max, both voxel decimations, range
and box predicates, compaction, bounding box, de-skew): named, seeded, host arrays only.  tests/test_preprocess_cpu.py shows on
the CPU that preprocess_ref and the C oracle agree on every case and that every case has the property it was built for;
tests/test_gpu_preprocess_edges.py holds the device to them.

  A  sizes      n on and off the wave / workgroup / grid boundaries (the stamp reduction's grid-stride loop wraps above 32 768)
  B  stamps     negative, mixed (minimum at 0, n-1, lane 63), equal, single, +-1e-30 beside +-0.05; both methods, an offset
  C  runs       known cell sequences: one cell, runs across lane 63/64 and thread 255/256, NaN inside a run, the cell's
                smallest index before the run, ABAB, every point its own cell (tables exactly half full); both methods, both stages
  D  cell edges coordinates k * res, +-0.3 res, +-0.999 res, +-0.0 under FLOOR and TRUNC
  E  minimum    350 raw points leave 299 / 300 / 301 for the second decimation (by duplicates, by the range band), minimum 300
  F  predicates points exactly on range_min / range_max around a non-zero centre and on the six box faces, one float step off
  G  key range  a finite point with |x / res| >= 1e6 among ordinary ones
  H  box        sizes around 1 024 and 65 536, octants, +-0.0, +-3e38, +-1e-40, extremes at 0 / n-1 / the last wave, non-finite rows
  I  de-skew    theta = |w t| at 0, 1e-9, either side of 1e-2, 0.5, 3; layer pairs around the 1 024-point workgroups"""
import functools

import numpy as np

import preprocess_ref as ref

F = np.float32


class Case:
    """One filter-chain job: raw cloud, optional stamps / intensity, chain parameters, stamp adjustment, with or without ICP layer"""

    def __init__(self, name, xyz, pp, t=None, inten=None, ts_method=ref.TS_NONE, ts_offset=0.0, want_icp=True, **props):
        self.name, self.xyz, self.pp = name, np.ascontiguousarray(xyz, F).reshape(-1, 3), pp
        self.t = None if t is None else np.ascontiguousarray(t, F)
        self.inten = None if inten is None else np.ascontiguousarray(inten, F)
        self.ts_method, self.ts_offset, self.want_icp = ts_method, ts_offset, want_icp
        self.props = props  # what the case promises (checked from the reference alone in test_preprocess_cpu.py)

    def __repr__(self):
        return self.name


def _seed(*parts):
    return np.random.default_rng([ord(c) for c in "".join(str(p) for p in parts)])


METHODS4 = ((0, 0), (1, 0), (0, 1), (1, 1))  # (decim_map_method, decim_icp_method)

# ---- A. sizes -----------------------------------------------------------------------------------------------------------------
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 32768, 32769, 40001)


@functools.lru_cache(None)
def table_a():
    out = []
    for k, n in enumerate(SIZES):
        rng = _seed("A", n)
        xyz = rng.uniform(-40, 40, (n, 3)).astype(F)
        t = rng.uniform(-0.05, 0.05, n).astype(F)
        inten = rng.uniform(0, 1, n).astype(F)
        mm, mi = METHODS4[k % 4] if n <= 1025 else (0, 0)
        pp = ref.params(decim_map_resolution=8.0, decim_icp_resolution=16.0, range_min=5.0, range_max=60.0, range_center=(1.0, -2.0, 0.5),
                        bbox_mode=ref.BBOX_KEEP_OUTSIDE, bbox_min=(-6.0, -6.0, -6.0), bbox_max=(6.0, 6.0, 6.0), index_mode=k % 2,
                        decim_map_method=mm, decim_icp_method=mi)
        for want_icp in (True, False):
            out.append(Case("A-n%d-%s" % (n, "icp" if want_icp else "map_only"), xyz, pp, t, inten,
                            (ref.TS_MIDDLE_IS_ZERO, ref.TS_EARLIEST_IS_ZERO)[k % 2], 0.01, want_icp))
    return out


# ---- B. stamps ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def table_b():
    n = 200
    rng = _seed("B")
    xyz = rng.uniform(-20, 20, (n, 3)).astype(F)
    mixed = rng.uniform(-0.05, 0.05, n).astype(F)
    stamps = {"all_negative": -rng.uniform(0.001, 0.1, n), "all_equal": np.full(n, 0.0125), "all_equal_negative": np.full(n, -0.0125),
              "tiny_mixed": np.tile([1e-30, -1e-30, 0.05, -0.05], n // 4), "tiny_negative": np.tile([-1e-30, -0.05], n // 2),
              "tiny_positive": np.tile([1e-30, 0.05], n // 2)}
    for where, k in (("first", 0), ("last", n - 1), ("lane63", 63)):
        for what, v in (("min", -0.06), ("max", 0.06)):
            s = mixed.copy()
            s[k] = v
            stamps["mixed_%s_%s" % (what, where)] = s
    out = []
    pp = ref.params()
    for name, s in stamps.items():
        for method in (ref.TS_MIDDLE_IS_ZERO, ref.TS_EARLIEST_IS_ZERO):
            out.append(Case("B-%s-m%d" % (name, method), xyz, pp, np.asarray(s, F), None, method, 0.0125, True))
    for method in (ref.TS_MIDDLE_IS_ZERO, ref.TS_EARLIEST_IS_ZERO):
        out.append(Case("B-single-m%d" % method, xyz[:1], pp, np.array([-0.02], F), None, method, 0.0125, True))
    return out


# ---- C. runs of equal voxels --------------------------------------------------------------------------------------------------
C_RES = 0.35
C_LATTICE = 16 * 16 * 9  # distinct cells cell_xyz() can name


def cell_xyz(k):
    """the k-th cell of a 16 x 16 x 9 block around the origin"""
    k = np.asarray(k, np.int64)
    return np.stack([k % 16 - 8, (k // 16) % 16 - 8, k // 256 - 4], axis=-1)


def points_in_cells(seq, res, rng):
    """one point per entry of `seq`, inside cell cell_xyz(seq[i]) of the `res` grid, a tenth of a cell off its faces"""
    c = cell_xyz(seq).astype(np.float64)
    return ((c + rng.uniform(0.1, 0.9, c.shape)) * res).astype(F)


def _run_seq(n, lo, hi, earlier=None):
    """every index its own cell, except lo..hi (inclusive), which share one cell -- that `earlier` (an index) shares too"""
    seq = np.arange(n, dtype=np.int64)
    seq[lo:hi + 1] = n
    if earlier is not None:
        seq[earlier] = n
    return seq


@functools.lru_cache(None)
def c_arrangements():
    """name -> (cell sequence, indices of NaN rows)"""
    arr = {}
    for n in (64, 256, 1000):
        arr["one_cell_n%d" % n] = (np.zeros(n, np.int64), ())
    n = 320
    for lo, hi, edge in ((59, 68, 63), (251, 260, 255)):
        tag = "run%d_%d" % (lo, hi)
        arr[tag] = (_run_seq(n, lo, hi), ())
        for where, k in (("edge_lo", edge), ("edge_hi", edge + 1), ("mid", lo + 2)):
            arr["%s_nan_%s" % (tag, where)] = (_run_seq(n, lo, hi), (k,))
        arr["%s_first_before" % tag] = (_run_seq(n, lo, hi, earlier=5), ())
    arr["run123_132_first_before"] = (_run_seq(n, 123, 132, earlier=5), ())
    arr["abab"] = (np.tile([0, 1], n // 2).astype(np.int64), ())
    for n in (32, 33, 2048, 2049):  # (table: the power of two >= 2 n, at least 64 -- 32 and 2048 fill it to exactly one half)
        arr["own_cell_n%d" % n] = (np.arange(n, dtype=np.int64), ())
    return arr


@functools.lru_cache(None)
def table_c():
    out = []
    for name, (seq, nans) in c_arrangements().items():
        rng = _seed("C", name)
        xyz = points_in_cells(seq, C_RES, rng)
        for k in nans:
            xyz[k, rng.integers(0, 3)] = np.nan
        for stage in (1, 2):
            for method in (ref.FIRST_POINT, ref.CLOSEST_TO_AVERAGE):
                if stage == 1:  # the sequence is what the first decimation sees; the second works on its survivors
                    pp = ref.params(decim_map_resolution=C_RES, decim_icp_resolution=2 * C_RES, decim_map_method=method, decim_icp_method=method)
                else:           # the first stage only drops the NaN rows: the second decimation sees the sequence
                    pp = ref.params(decim_map_resolution=0.0, decim_icp_resolution=C_RES, decim_icp_method=method)
                out.append(Case("C-%s-stage%d-method%d" % (name, stage, method), xyz, pp, None, None, ref.TS_NONE, 0.0, True,
                                arrangement=name, stage=stage))
    return out


# ---- D. cell edges ------------------------------------------------------------------------------------------------------------
D_RES = (0.25, 0.35, 1.1)


def d_points(res):
    r = F(res)
    # (the fractions first: under FLOOR -0.3 res claims cell -1 before -1 res arrives, under TRUNC it claims cell 0 -- with the
    #  lattice points first both modes would keep the same FirstPoint survivors)
    vals = [F(s * f) * r for s in (-1, 1) for f in (0.3, 0.999)] + [F(-0.0), F(0.0)] + [F(k) * r for k in range(-3, 4)]
    m = F(0.5) * r
    pts = []
    for v in vals:
        pts += [(v, m, m), (m, v, m), (m, m, v), (v, v, v)]
    pts = np.asarray(pts, F)
    rng = _seed("D", res)
    return np.concatenate([pts, pts[rng.permutation(len(pts))]])  # every point twice: a cell's survivor is not a given


@functools.lru_cache(None)
def table_d():
    out = []
    for res in D_RES:
        xyz = d_points(res)
        for mode in (ref.INDEX_FLOOR, ref.INDEX_TRUNC):
            for method in (ref.FIRST_POINT, ref.CLOSEST_TO_AVERAGE):
                pp = ref.params(decim_map_resolution=res, decim_icp_resolution=2 * res, index_mode=mode, decim_map_method=method,
                                decim_icp_method=method)
                out.append(Case("D-res%g-mode%d-method%d" % (res, mode, method), xyz, pp, None, None, ref.TS_NONE, 0.0, True, res=res, mode=mode,
                                method=method))
    return out


# ---- E. the second stage's minimum --------------------------------------------------------------------------------------------
E_MIN, E_RAW, E_RES = 300, 350, 0.5
E_COUNTS = (299, 300, 301)


def _e_cell(k):
    k = np.asarray(k, np.int64)
    return np.stack([k % 8, (k // 8) % 8, k // 64], axis=-1).astype(np.float64)


@functools.lru_cache(None)
def table_e():
    out = []
    for N in E_COUNTS:
        # by duplicates: N distinct map cells, the other 350 - N rows are further points of cells already there
        rng = _seed("E", "dup", N)
        seq = np.concatenate([np.arange(N), rng.integers(0, N, E_RAW - N)])
        seq[N // 2:] = rng.permutation(seq[N // 2:])
        xyz = ((_e_cell(seq) + rng.uniform(0.1, 0.9, (E_RAW, 3))) * E_RES).astype(F)
        # by the band: 350 distinct cells, of which the range band (it runs between the two decimations) keeps the N nearest
        rng = _seed("E", "band", N)
        xyz_b = ((_e_cell(rng.permutation(E_RAW)) + rng.uniform(0.1, 0.9, (E_RAW, 3))) * E_RES).astype(F)
        centre = (1.9, 2.1, 1.4)
        sq = np.sort(ref.range_sq(xyz_b, centre).astype(np.float64))
        assert sq[N] - sq[N - 1] > 1e-4 * sq[N]
        rmax = float(np.sqrt(0.5 * (sq[N - 1] + sq[N])))
        for mm, mi in ((0, 0), (1, 1)):
            base = dict(decim_map_resolution=E_RES, decim_icp_resolution=2 * E_RES, min_points_to_filter=E_MIN, decim_map_method=mm, decim_icp_method=mi)
            out.append(Case("E-dup-N%d-methods%d%d" % (N, mm, mi), xyz, ref.params(**base), None, None, ref.TS_NONE, 0.0, True, N=N))
            out.append(Case("E-band-N%d-methods%d%d" % (N, mm, mi), xyz_b, ref.params(range_min=0.0, range_max=rmax, range_center=centre, **base),
                            None, None, ref.TS_NONE, 0.0, True, N=N))
    return out


# ---- F. predicates at equality ------------------------------------------------------------------------------------------------
F_CENTRE = (1.0, -2.0, 3.0)
F_RMIN, F_RMAX = 5.0, 13.0
F_ON_MIN = ((3, 4, 0), (0, 0, 5), (-4, 3, 0), (0, -5, 0), (0, 3, -4))
F_ON_MAX = ((5, 12, 0), (0, 0, 13), (3, 4, 12), (-12, 0, 5), (0, -13, 0))
F_BMIN, F_BMAX = (-2.1, -3.0, -1.8), (4.3, 5.0, 2.5)


def _stepped(p, thr_sq, want_above):
    """p moved by the fewest float steps of one coordinate that bring its float32 squared range strictly above / below thr_sq"""
    for steps in range(1, 9):
        for a in range(3):
            for direction in (np.inf, -np.inf):
                q = np.array(p, F)
                for _ in range(steps):
                    q[a] = np.nextafter(q[a], F(direction))
                sq = ref.range_sq(q[None], F_CENTRE)[0]
                if (sq > thr_sq) if want_above else (sq < thr_sq):
                    return q
    raise AssertionError("no float step changes the squared range of %r" % (p,))


@functools.lru_cache(None)
def f_points():
    """(xyz, tags): tags[i] = (kind, where) with kind in range_on_min / range_on_max / box_face / filler and where in on / in / out"""
    pts, tags = [], []
    c = np.asarray(F_CENTRE, F)
    for kind, offs, r in (("range_on_min", F_ON_MIN, F_RMIN), ("range_on_max", F_ON_MAX, F_RMAX)):
        thr = F(r) * F(r)
        for o in offs:
            p = (np.asarray(o, F) + c).astype(F)
            assert ref.range_sq(p[None], F_CENTRE)[0] == thr  # bit for bit on the threshold
            above, below = _stepped(p, thr, True), _stepped(p, thr, False)
            inside, outside = (above, below) if kind == "range_on_min" else (below, above)
            pts += [p, inside, outside]
            tags += [(kind, "on"), (kind, "in"), (kind, "out")]
    bmin, bmax = np.asarray(F_BMIN, F), np.asarray(F_BMAX, F)
    mid = (F(0.5) * (bmin + bmax)).astype(F)
    for a in range(3):
        for face, outward in ((bmin, -np.inf), (bmax, np.inf)):
            on = mid.copy()
            on[a] = face[a]
            out_, in_ = on.copy(), on.copy()
            out_[a] = np.nextafter(face[a], F(outward))
            in_[a] = np.nextafter(face[a], F(-outward))
            pts += [on, in_, out_]
            tags += [("box_face", "on"), ("box_face", "in"), ("box_face", "out")]
    rng = _seed("F")
    fill = rng.uniform(-15, 15, (150, 3)).astype(F)
    pts += list(fill)
    tags += [("filler", "")] * len(fill)
    order = rng.permutation(len(pts))
    return np.asarray(pts, F)[order], [tags[k] for k in order]


@functools.lru_cache(None)
def table_f():
    xyz, _ = f_points()
    band = dict(range_min=F_RMIN, range_max=F_RMAX, range_center=F_CENTRE)
    box = dict(bbox_min=F_BMIN, bbox_max=F_BMAX)
    variants = (("range", ref.params(**band)), ("box_inside", ref.params(bbox_mode=ref.BBOX_KEEP_INSIDE, **box)),
                ("box_outside", ref.params(bbox_mode=ref.BBOX_KEEP_OUTSIDE, **box)),
                ("range_and_box_inside", ref.params(bbox_mode=ref.BBOX_KEEP_INSIDE, **band, **box)),
                ("range_off_zero_max", ref.params(range_min=F_RMIN, range_max=0.0, range_center=F_CENTRE)),
                ("range_off_negative_max", ref.params(range_min=F_RMIN, range_max=-1.0, range_center=F_CENTRE)))
    return [Case("F-" + name, xyz, pp, None, None, ref.TS_NONE, 0.0, True, variant=name) for name, pp in variants]


TABLES = {"A": table_a, "B": table_b, "C": table_c, "D": table_d, "E": table_e, "F": table_f}


@functools.lru_cache(None)
def expected(case):
    """(idx_map, idx_icp, adjusted stamps or None) of a case, from preprocess_ref; computed once, shared, never written to"""
    im, ii = ref.chain(case.xyz, case.pp)
    ta = None if case.t is None else ref.adjust(case.t, case.ts_method, case.ts_offset)
    for a in (im, ii, ta):
        if a is not None:
            a.setflags(write=False)
    return im, ii, ta


# ---- G. key range -------------------------------------------------------------------------------------------------------------
G_RES, G_AT = 0.5, 137
G_LIMIT_X = 5.0e5  # x * (1.0f / 0.5f) == 1e6 exactly: the first value outside the key range


@functools.lru_cache(None)
def g_cloud():
    xyz = _seed("G").uniform(-20, 20, (400, 3)).astype(F)
    xyz.setflags(write=False)
    return xyz


def g_with(x):
    """the ordinary cloud with row G_AT replaced by (x, 1, 1)"""
    xyz = g_cloud().copy()
    xyz[G_AT] = (x, 1.0, 1.0)
    return xyz


def g_params(**kw):
    return ref.params(**dict(dict(decim_map_resolution=G_RES, decim_icp_resolution=2 * G_RES, range_min=2.0, range_max=1.0e7), **kw))


def chain_without(xyz, pp, drop):
    """the chain's result for the scan without row `drop`, as indices into the scan WITH it"""
    keep = np.delete(np.arange(len(xyz)), drop)
    im, ii = ref.chain(np.asarray(xyz, F)[keep], pp)
    return keep[im].astype(np.uint32), keep[ii].astype(np.uint32)


# ---- H. bounding box ----------------------------------------------------------------------------------------------------------
H_SIZES = (1, 63, 64, 65, 1023, 1024, 1025, 65535, 65536, 65537, 70001)  # 65 536 / 65 537: k_pp_bbox_one / k_pp_bbox
H_ONE_LIMIT, H_GRID = 65536, 128 * 256


def h_last_wave_index(n):
    """an index that the last wave of the last workgroup reads on its last lap: k_pp_bbox_one is one workgroup of 1024 striding
    by 1024; k_pp_bbox is min(ceil(n / 256), 128) workgroups of 256 striding by the grid"""
    stride = 1024 if n <= H_ONE_LIMIT else min((n + 255) // 256, 128) * 256
    lane = stride - 11
    k = (n - 1 - lane) // stride * stride + lane if n > lane else n - 1
    return int(k)


@functools.lru_cache(None)
def table_h():
    """[(name, xyz)]"""
    out = []
    for n in H_SIZES:
        for kind, lo, hi in (("mixed", -50, 50), ("negative", -50, -1), ("positive", 1, 50)):
            out.append(("H-%s-n%d" % (kind, n), _seed("H", kind, n).uniform(lo, hi, (n, 3)).astype(F)))
    rng = _seed("H", "values")
    out.append(("H-signed_zeros", rng.choice(np.array([0.0, -0.0], F), (130, 3))))
    z = -rng.uniform(0, 5, (130, 3)).astype(F)
    z[77] = -0.0
    out.append(("H-negative_zero_is_max", z))
    out.append(("H-huge_and_tiny", rng.choice(np.array([3e38, -3e38, 1e-40, -1e-40, 1.0, -1.0], F), (300, 3))))
    out.append(("H-subnormal_extremes", rng.choice(np.array([1e-40, -1e-40, 0.0, 3e-41], F), (300, 3))))
    out.append(("H-only_huge_negative", np.full((70, 3), -3e38, F)))
    for n in (300, 1025, 65536, 65537, 70001):
        for where, k in (("first", 0), ("last", n - 1), ("last_wave", h_last_wave_index(n))):
            xyz = _seed("H", "extreme", n).uniform(-10, 10, (n, 3)).astype(F)
            k2 = k + 1 if k + 1 < n else k - 1
            xyz[k] = (-99.0, -98.0, -97.0)
            xyz[k2] = (96.0, 95.0, 94.0)
            out.append(("H-extremes_%s-n%d" % (where, n), xyz))
    for n in (65, 1025, 70001):
        xyz = _seed("H", "nonfinite", n).uniform(-10, 10, (n, 3)).astype(F)
        for k, row in ((0, (np.nan, 1e3, -1e3)), (n // 2, (1e3, np.inf, -1e3)), (n - 1, (-1e3, 1e3, -np.inf)), (h_last_wave_index(n) - 1, (2e3, -2e3, np.nan))):
            xyz[k] = row
        out.append(("H-nonfinite_rows_would_be_extremes-n%d" % n, xyz))
    for n in (1, 100, 65536, 70001):
        xyz = np.ones((n, 3), F)
        xyz[np.arange(n), np.arange(n) % 3] = (np.nan, np.inf, -np.inf, np.nan)[n % 4]
        out.append(("H-all_rows_nonfinite-n%d" % n, xyz))
    out.append(("H-empty", np.zeros((0, 3), F)))
    return out


# ---- I. de-skew ---------------------------------------------------------------------------------------------------------------
I_UNIT_W = np.array([2.0, -1.0, 2.0]) / 3.0  # |w| = 1: theta = |t|
I_TWISTS = {"linear_only": np.array([14.0, -0.3, 0.05, 0.0, 0.0, 0.0]), "angular_only": np.array([0.0, 0.0, 0.0, 0.01, -0.02, 0.7]),
            "unit_rate": np.concatenate([[14.0, -0.3, 0.05], I_UNIT_W])}
# theta under unit_rate: 0, 1e-9, just below / above the series switch at 1e-2 (F(0.01) < 1e-2 < its successor), 0.5, 3
I_STAMPS = np.array([0.0, -0.0, 1e-9, -1e-9, 0.01, np.nextafter(F(0.01), F(1)), -0.01, -np.nextafter(F(0.01), F(1)), 0.0099, 0.0101, 0.5, -0.5,
                     3.0, -3.0], F)
I_PAIRS = ((1, 1), (1023, 64), (1024, 1024), (1025, 1025), (5000, 3000), (5000, 1), (64, 3000))  # (large, small)


def i_layer(tag, n, nonfinite):
    """(xyz, t, inten): t starts with I_STAMPS (as many as fit), the rest U(-0.05, 0.05); one non-finite row when asked"""
    rng = _seed("I", tag, n)
    xyz = rng.uniform(-30, 30, (n, 3)).astype(F)
    t = rng.uniform(-0.05, 0.05, n).astype(F)
    k = min(n, len(I_STAMPS))
    t[:k] = I_STAMPS[:k] if n > 1 else I_STAMPS[10:11]
    if nonfinite:
        xyz[n // 2, n % 3] = (np.nan, np.inf)[n % 2]
    return xyz, t, rng.uniform(0, 1, n).astype(F)
