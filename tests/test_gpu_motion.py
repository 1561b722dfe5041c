"""-m gpu: mh_scan_deskew_motion and mh_scan_deskew_motion_pair (include/molahip_motion.h, k_motion_deskew and
k_motion_deskew_pair of mh_k_motion.h) through the C ABI against the float64 restatement of tests/motion_ref.py.

Coordinates: |got - ref| <= spacing(float32(max(|ref|, 1e-3))) -- the one-ulp rule of test_gpu_preprocess.py::test_deskew; the 1e-3
floor covers cancellation in R u + v t (the fp64 evaluation error at 200 m is below 1e-12, the float spacing at 1e-3 is 1.2e-10).
The tables here give every segment a rotation of its own, unrelated to its neighbours', so a point put into the wrong segment
lands metres away: the coordinate bound is the check of the segment choice as well.  Stamps, src_idx and intensity: bit for bit.
The share of bit-equal coordinates is printed, not asserted."""
import ctypes as C

import numpy as np
import pytest

import motion_ref as ref
import preprocess_ref as pref
from mola_lidar_odometry_amd import capi, capi_motion as cm

pytestmark = pytest.mark.gpu

F = np.float32
ERR_INVALID = 1  # MH_ERR_INVALID_ARGUMENT


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx2():
    c = capi.Context(0)
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def make_table(K, seed, span=0.1):
    """knots on float32 values (so that a float32 stamp can sit ON a knot), 0 among them when K >= 3; unrelated rotations"""
    rng = np.random.default_rng(seed)
    knots = np.sort(rng.uniform(-0.5 * span, 0.5 * span, K)).astype(F)
    if K >= 3:
        knots[K // 2] = 0.0
        knots = np.sort(knots)
    knots = np.unique(knots).astype(np.float64)
    assert len(knots) == K
    R = ref.so3_exp(rng.uniform(-1.5, 1.5, (K, 3)))
    w = rng.uniform(-3.0, 3.0, (K, 3))
    v = rng.uniform(-20.0, 20.0, 3)
    return dict(knots=knots, R=R, w=w, v=v)


def special_stamps(knots):
    k32 = knots.astype(F)
    return np.concatenate([k32, np.nextafter(k32, F(-np.inf)), np.nextafter(k32, F(np.inf)),
                           np.array([k32[0] - F(0.01), k32[0] - F(1.0), k32[-1] + F(0.01), k32[-1] + F(1.0), 0.0, -0.0, np.nan, np.inf, -np.inf], F)])


def make_layer(n, knots, seed, nan_points=True):
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-100.0, 100.0, (n, 3)).astype(F)
    sp = special_stamps(knots)
    t = np.concatenate([sp, np.sort(rng.uniform(knots[0] - 0.02, knots[-1] + 0.02, max(n - len(sp), 0))).astype(F)])[:n]
    if nan_points and n > 40:
        xyz[n - 3, 0] = np.nan
        xyz[n - 2, 1] = np.nan
        xyz[n - 1] = np.nan
    inten = rng.uniform(0.0, 255.0, n).astype(F)
    return xyz, t.astype(F), inten


def upload(c, xyz, t=None, inten=None):
    s = capi.Scan(c, xyz) if len(xyz) else capi.Scan(c)
    if t is not None and len(xyz):
        s.set_timestamps(t)
    if inten is not None and len(xyz):
        s.set_intensity(inten)
    return s


def table_of(tab):
    return cm.motion_table(tab["knots"], tab["R"], tab["w"], tab["v"])


def bound_of(want):
    return np.spacing(np.maximum(np.abs(want), 1e-3).astype(F)).astype(np.float64)


STATS = dict(equal=0, total=0)


def check_coords(got_xyz, xyz, t, tab, what):
    want, _ = ref.deskew_motion(xyz, t, tab["knots"], tab["R"], tab["w"], tab["v"])
    fin = np.isfinite(want).all(axis=1)
    assert np.isnan(want[~fin]).all(), what  # (the reference: a NaN coordinate or a NaN / infinite stamp makes the whole row NaN)
    assert np.isnan(got_xyz[~fin]).all(), what
    err = np.abs(got_xyz[fin].astype(np.float64) - want[fin])
    bound = bound_of(want[fin])
    assert (err <= bound).all(), (what, float((err / bound).max()), int(np.argmax((err / bound).max(axis=1))))
    STATS["equal"] += int((_bits(got_xyz[fin]) == _bits(want[fin].astype(F))).sum())
    STATS["total"] += int(fin.sum()) * 3


def check_scan(scan, xyz, t, inten, src, tab, what):
    assert scan.n == len(xyz), what
    d = scan.download()
    np.testing.assert_array_equal(_bits(d["t"]), _bits(t), err_msg=what)
    if src is not None:
        np.testing.assert_array_equal(d["src_idx"], src, err_msg=what)
    if inten is not None and len(xyz):
        np.testing.assert_array_equal(_bits(scan.download_intensity()), _bits(inten), err_msg=what)
    if len(xyz):
        check_coords(d["xyz"], xyz, t, tab, what)


def check_untouched(scan, xyz, t):
    d = scan.download()
    np.testing.assert_array_equal(_bits(d["xyz"]), _bits(xyz))
    if t is not None:
        np.testing.assert_array_equal(_bits(d["t"]), _bits(t))


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049, 5000])
def test_single_over_sizes(ctx, n):
    tab = make_table(3, 100 + n)
    xyz, t, inten = make_layer(n, tab["knots"], n)
    inten = inten if n % 2 else None  # layers with and without an intensity
    keep, T = table_of(tab)
    src_scan = upload(ctx, xyz, t, inten)
    out = capi.Scan(ctx)
    cm.deskew_motion(src_scan, T, out)
    check_scan(out, xyz, t, inten, None, tab, "n = %d" % n)
    check_untouched(src_scan, xyz, t)
    src_scan.close(), out.close()


@pytest.mark.parametrize("K", [1, 2, 3, 12, 32, 33, 63, 64])
def test_single_over_segment_counts(ctx, K):
    """K <= 32 travels as a kernel argument, K > 32 through the stream-ordered copy; every special stamp of every knot is present"""
    tab = make_table(K, 7 * K)
    n = 1025
    xyz, t, inten = make_layer(n, tab["knots"], K)
    assert len(special_stamps(tab["knots"])) < n - 3
    keep, T = table_of(tab)
    src_scan, out = upload(ctx, xyz, t, inten), capi.Scan(ctx)
    cm.deskew_motion(src_scan, T, out)
    check_scan(out, xyz, t, inten, None, tab, "K = %d" % K)
    print("K = %d: %d of %d finite coordinates bit-equal to the rounded float64 restatement so far" % (K, STATS["equal"], STATS["total"]))
    src_scan.close(), out.close()


def _derived_layer(c, xyz, t, inten):
    """the layer as a filter chain hands it on (source indices that are not 0..n-1, stamps, intensity): a pass-through of a raw
    scan that has three NaN rows more"""
    n = len(xyz) + 3
    keep = np.delete(np.arange(n), [0, n // 2, n - 1])
    rx, rt, ri = np.full((n, 3), np.nan, F), np.zeros(n, F), np.zeros(n, F)
    rx[keep], rt[keep], ri[keep] = xyz, t, inten
    raw = capi.Scan(c, rx).set_timestamps(rt).set_intensity(ri)
    layer = capi.Scan(c)
    raw.preprocess(capi.preprocess_params(**pref.params()), layer, None)
    raw.close()
    return layer, keep.astype(np.uint32)


def test_a_derived_layer_carries_src_idx_and_intensity(ctx):
    tab = make_table(12, 5)
    xyz, t, inten = make_layer(777, tab["knots"], 5, nan_points=False)
    layer, src = _derived_layer(ctx, xyz, t, inten)  # (the pass-through keeps rows by their coordinates, whatever their stamps)
    assert layer.n == len(xyz)
    keep, T = table_of(tab)
    out = capi.Scan(ctx)
    cm.deskew_motion(layer, T, out)
    check_scan(out, xyz, t, inten, src, tab, "derived layer")
    layer.close(), out.close()


@pytest.mark.parametrize("small_n", [0, 1, 1024, 1025, 65536, 65537])
def test_pair_equals_the_singles_and_the_box(ctx, small_n):
    """fused launch (1 .. 65536) and the fall-backs (empty, above 65536, no table, no stamps): bit for bit the two single calls and
    mh_scan_bbox of out_b"""
    K = 64 if small_n in (1025, 65537) else 12
    tab = make_table(K, 900 + small_n % 97)
    keep, T = table_of(tab)
    bx, bt, bi = make_layer(2049, tab["knots"], 1)
    sx, st, si = make_layer(small_n, tab["knots"], 2)
    for variant in ("table", "no_table", "no_stamps"):
        if variant != "table" and small_n not in (1, 1025):
            continue
        stamped = variant != "no_stamps"
        big = upload(ctx, bx, bt if stamped else None, bi)
        small = upload(ctx, sx, st if stamped else None, None)
        a, b, a1, b1 = (capi.Scan(ctx) for _ in range(4))
        tt = T if variant != "no_table" else None
        mn, mx, nf = cm.deskew_motion_pair(big, small, tt, a, b)
        cm.deskew_motion(big, tt, a1)
        cm.deskew_motion(small, tt, b1)
        what = "%s small %d" % (variant, small_n)
        for got, sep, (xyz, t, inten) in ((a, a1, (bx, bt, bi)), (b, b1, (sx, st, None))):
            d, ds = got.download(), sep.download()
            assert got.n == sep.n == len(xyz), what
            np.testing.assert_array_equal(_bits(d["xyz"]), _bits(ds["xyz"]), err_msg=what)
            np.testing.assert_array_equal(_bits(d["t"]), _bits(ds["t"]), err_msg=what)
            if stamped:
                np.testing.assert_array_equal(_bits(d["t"]), _bits(t), err_msg=what)
            if inten is not None:
                np.testing.assert_array_equal(_bits(got.download_intensity()), _bits(inten), err_msg=what)
            if variant == "table":
                check_scan(got, xyz, t, inten, None, tab, what)
            else:
                np.testing.assert_array_equal(_bits(d["xyz"]), _bits(xyz), err_msg=what)  # a copy
        bmn, bmx, bnf = b1.bbox()
        assert nf == bnf, what
        np.testing.assert_array_equal(_bits(mn), _bits(bmn), err_msg=what)
        np.testing.assert_array_equal(_bits(mx), _bits(bmx), err_msg=what)
        db = b.download()["xyz"]
        rmn, rmx, rcnt = pref.bbox(db)  # ... and the box of the pair's own output, exactly
        assert nf == rcnt, what
        np.testing.assert_array_equal(mn, rmn, err_msg=what)
        np.testing.assert_array_equal(mx, rmx, err_msg=what)
        check_untouched(big, bx, bt if stamped else None)
        for s in (big, small, a, b, a1, b1):
            s.close()


def test_a_constant_rate_is_mh_scan_deskew(ctx):
    """K = 1 with knot 0, R = I and (v, w), and a table cut from the same constant rate at 12 knots: both are mh_scan_deskew(twist =
    (v, w)) within the coordinate bound"""
    rng = np.random.default_rng(11)
    n = 4099
    xyz = rng.uniform(-100.0, 100.0, (n, 3)).astype(F)
    t = np.sort(rng.uniform(-0.06, 0.06, n)).astype(F)
    v, w = np.array([12.0, -0.7, 0.3]), np.array([0.21, -0.35, 1.3])
    src_scan, plain, out = upload(ctx, xyz, t), capi.Scan(ctx), capi.Scan(ctx)
    src_scan.deskew(np.concatenate([v, w]), plain)
    want = plain.download()["xyz"]
    knots12 = (-0.06 + 0.01 * np.arange(12)).astype(F).astype(np.float64)
    R12, w12 = ref.constant_rate_table(knots12, w)
    for name, tab in (("one segment", dict(knots=np.zeros(1), R=np.eye(3)[None], w=w[None], v=v)), ("twelve", dict(knots=knots12, R=R12, w=w12, v=v))):
        keep, T = table_of(tab)
        cm.deskew_motion(src_scan, T, out)
        got = out.download()["xyz"]
        err = np.abs(got.astype(np.float64) - want.astype(np.float64))
        assert (err <= bound_of(want.astype(np.float64))).all(), (name, float((err / bound_of(want.astype(np.float64))).max()))
        print("%s: %.2f %% of the coordinates bit-equal to mh_scan_deskew" % (name, 100.0 * float((_bits(got) == _bits(want)).mean())))
    for s in (src_scan, plain, out):
        s.close()


@pytest.mark.parametrize("Ks", [(12, 12), (64, 64), (12, 64), (64, 12), (33, 40)])
def test_two_queued_calls_each_read_their_own_table(ctx, Ks):
    """the staging hazard: two calls with different tables queued back to back on one stream, their caller's tables overwritten
    at once, read only after both"""
    n = 120000
    tabs = [make_table(K, 40 + i) for i, K in enumerate(Ks)]
    xyz, t, _ = make_layer(n, np.array([-0.05, 0.05]), 3)
    src_scan, outs = upload(ctx, xyz, t), [capi.Scan(ctx), capi.Scan(ctx)]
    for o in outs:  # sized beforehand, so that nothing but the two calls sits between them
        cm.deskew_motion(src_scan, table_of(tabs[0])[1], o)
    ctx.synchronize()
    for tab, o in zip(tabs, outs):
        keep, T = table_of(tab)
        cm.deskew_motion(src_scan, T, o)
        C.memset(keep, 0xFF, C.sizeof(keep))  # the caller's block is free to change as soon as the call has returned
        T.v[:] = [1e9, 1e9, 1e9]
    for tab, o, K in zip(tabs, outs, Ks):
        check_coords(o.download()["xyz"], xyz, t, tab, "queued, K = %d" % K)
    for s in [src_scan] + outs:
        s.close()


def test_copies_and_a_second_context(ctx, ctx2):
    tab = make_table(12, 77)
    keep, T = table_of(tab)
    xyz, t, inten = make_layer(1500, tab["knots"], 8)
    out = capi.Scan(ctx)
    # motion NULL: a copy, channels included
    s = upload(ctx, xyz, t, inten)
    cm.deskew_motion(s, None, out)
    d = out.download()
    np.testing.assert_array_equal(_bits(d["xyz"]), _bits(xyz))
    np.testing.assert_array_equal(_bits(d["t"]), _bits(t))
    np.testing.assert_array_equal(_bits(out.download_intensity()), _bits(inten))
    s.close()
    # no time stamps: a copy
    s = upload(ctx, xyz, None, inten)
    cm.deskew_motion(s, T, out)
    np.testing.assert_array_equal(_bits(out.download()["xyz"]), _bits(xyz))
    np.testing.assert_array_equal(_bits(out.download_intensity()), _bits(inten))
    s.close()
    # `in` belongs to a second context of the same device
    s = upload(ctx2, xyz, t, inten)
    ctx2.synchronize()
    cm.deskew_motion(s, T, out)
    check_scan(out, xyz, t, inten, None, tab, "second context")
    check_untouched(s, xyz, t)
    s.close(), out.close()


def test_every_refusal_and_the_context_after_it(ctx):
    L = cm.lib()
    good = make_table(3, 1)
    xyz, t, _ = make_layer(300, good["knots"], 9)
    s, s2, out, out2 = upload(ctx, xyz, t), upload(ctx, xyz, t), capi.Scan(ctx), capi.Scan(ctx)
    keep, T = table_of(good)
    cm.deskew_motion(s, T, out)
    before = _bits(out.download()["xyz"]).copy()
    mn, mx, nf = (C.c_float * 3)(), (C.c_float * 3)(), C.c_uint64(0)

    def bad_tables():
        K3 = good["knots"]
        yield "n_segments 0", cm.motion_table(K3, good["R"], good["w"], good["v"], n_segments=0)
        yield "n_segments 65", cm.motion_table(np.arange(65) * 0.001, np.tile(np.eye(3), (65, 1, 1)), np.zeros((65, 3)), good["v"])
        kp, tb = table_of(good)
        tb.segments = None
        yield "NULL segments", (kp, tb)
        yield "equal knots", cm.motion_table([K3[0], K3[0], K3[2]], good["R"], good["w"], good["v"])
        yield "descending knots", cm.motion_table(K3[::-1].copy(), good["R"], good["w"], good["v"])
        for bad in (np.nan, np.inf, -np.inf):
            k = K3.copy(); k[1] = bad
            yield "knot %r" % bad, cm.motion_table(k, good["R"], good["w"], good["v"])
            R = good["R"].copy(); R[2, 1, 1] = bad
            yield "R %r" % bad, cm.motion_table(K3, R, good["w"], good["v"])
            w = good["w"].copy(); w[0, 2] = bad
            yield "w %r" % bad, cm.motion_table(K3, good["R"], w, good["v"])
            v = good["v"].copy(); v[1] = bad
            yield "v %r" % bad, cm.motion_table(K3, good["R"], good["w"], v)

    def refused(status, what):
        assert status == ERR_INVALID, what
        assert L.mh_last_error_string(), what
        np.testing.assert_array_equal(_bits(out.download()["xyz"]), before, err_msg=what)  # `out` untouched
        cm.deskew_motion(s, T, out2)  # the context is as good as before
        np.testing.assert_array_equal(_bits(out2.download()["xyz"]), before, err_msg=what)

    for what, (kp, tb) in bad_tables():
        refused(L.mh_scan_deskew_motion(s._h, C.byref(tb), out._h), what)
        refused(L.mh_scan_deskew_motion_pair(s._h, s2._h, C.byref(tb), out._h, out2._h, mn, mx, C.byref(nf)), "pair: " + what)
        no_t = upload(ctx, xyz)  # refused before the fall-back to a copy is taken
        refused(L.mh_scan_deskew_motion(no_t._h, C.byref(tb), out._h), what + " (no stamps)")
        no_t.close()
    refused(L.mh_scan_deskew_motion(None, C.byref(T), out._h), "NULL in")
    refused(L.mh_scan_deskew_motion(s._h, C.byref(T), None), "NULL out")
    refused(L.mh_scan_deskew_motion(out._h, C.byref(T), out._h), "out == in")
    refused(L.mh_scan_deskew_motion(out._h, None, out._h), "out == in without a table")
    pair = L.mh_scan_deskew_motion_pair
    refused(pair(None, s2._h, C.byref(T), out._h, out2._h, mn, mx, C.byref(nf)), "pair: NULL in_a")
    refused(pair(s._h, None, C.byref(T), out._h, out2._h, mn, mx, C.byref(nf)), "pair: NULL in_b")
    refused(pair(s._h, s2._h, C.byref(T), None, out2._h, mn, mx, C.byref(nf)), "pair: NULL out_a")
    refused(pair(s._h, s2._h, C.byref(T), out._h, None, mn, mx, C.byref(nf)), "pair: NULL out_b")
    refused(pair(s._h, s2._h, C.byref(T), out._h, out2._h, None, mx, C.byref(nf)), "pair: NULL bb_min")
    refused(pair(s._h, s2._h, C.byref(T), out._h, out2._h, mn, None, C.byref(nf)), "pair: NULL bb_max")
    refused(pair(s._h, s2._h, C.byref(T), out._h, out._h, mn, mx, C.byref(nf)), "pair: out_a == out_b")
    refused(pair(s._h, s2._h, C.byref(T), s._h, out2._h, mn, mx, C.byref(nf)), "pair: out_a == in_a")
    assert pair(s._h, s2._h, C.byref(T), out._h, out2._h, mn, mx, None) == 0  # n_finite may be NULL
    np.testing.assert_array_equal(_bits(out.download()["xyz"]), before)
    if capi.device_count() >= 2:  # scans of different devices
        other = capi.Context(1)
        far = capi.Scan(other)
        refused(L.mh_scan_deskew_motion(s._h, C.byref(T), far._h), "different devices")
        refused(pair(s._h, s2._h, C.byref(T), out._h, far._h, mn, mx, C.byref(nf)), "pair: different devices")
        far.close(), other.close()
    for x in (s, s2, out, out2):
        x.close()
