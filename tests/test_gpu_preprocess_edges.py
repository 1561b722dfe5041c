"""-m gpu: the first-generation scan kernels of mh_preprocess.hip (k_pp_tminmax_b, k_pp_insert_b, k_cta_*, k_pp_flag_b,
k_pp_compact_b, k_pp_bbox_one, k_pp_bbox, k_pp_deskew, k_pp_deskew_pair) at their edges, against the numpy restatement of
tests/preprocess_ref.py and the C oracle, over the case tables of tests/preprocess_cases.py (tests/test_preprocess_cpu.py shows
the two references equal on every case, and that every case has the property it was built for).

Tables A-F: source indices, coordinates, intensity bit for bit, stamps by value -- case by case, then all cases of a table as the
jobs of ONE mh_scan_preprocess_batch call in table order and in reverse, so that ragged neighbours of 1, 63, 64, 65 points sit
side by side in the shared flag / position arrays and tables.  G: MH_ERR_OUT_OF_RANGE and what the outputs hold then.  H: the
bounding box against numpy's min / max, count included.  I: de-skew against a long-double reference under the bound
preprocess_ref.deskew_bound derives (one float ulp + 16 * 2^-52 * (|x| + |y| + |z| + |v t|)); the fused pair kernel bit for bit
against the separate calls and its box against the box of its own output."""
import numpy as np
import pytest

import preprocess_cases as pc
import preprocess_ref as ref
from mola_lidar_odometry_amd import capi

pytestmark = pytest.mark.gpu

F = np.float32
ERR_OUT_OF_RANGE = 4  # MH_ERR_OUT_OF_RANGE


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def pool():
    """contexts for the jobs of a batch (each job in its own, as mh_scan_preprocess_batch allows), made once and shared"""
    ctxs = []

    def get(n):
        while len(ctxs) < n:
            ctxs.append(capi.Context(0))
        return ctxs[:n]

    yield get
    for c in ctxs:
        c.close()


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _upload(c, case):
    raw = capi.Scan(c, case.xyz)
    if case.t is not None:
        raw.set_timestamps(case.t)
    if case.inten is not None:
        raw.set_intensity(case.inten)
    return raw


def _params(case):
    return capi.preprocess_params(timestamp_method=case.ts_method, time_offset=case.ts_offset, **case.pp)


def _check_layer(scan, idx, case, ta, what):
    msg = "%s %s" % (case.name, what)
    assert scan.n == len(idx), msg
    d = scan.download()
    np.testing.assert_array_equal(d["src_idx"], idx, err_msg=msg)
    np.testing.assert_array_equal(_bits(d["xyz"]), _bits(case.xyz[idx]), err_msg=msg)
    np.testing.assert_array_equal(d["t"], ta[idx] if ta is not None else np.zeros(len(idx), F), err_msg=msg)
    if case.inten is not None and len(idx):
        np.testing.assert_array_equal(_bits(scan.download_intensity()), _bits(case.inten[idx]), err_msg=msg)


def _check_case(case, om, oi):
    im, ii, ta = pc.expected(case)
    _check_layer(om, im, case, ta, "map layer")
    if case.want_icp:
        _check_layer(oi, ii, case, ta, "icp layer")


@pytest.mark.parametrize("letter", sorted(pc.TABLES))
def test_chain_case_by_case(ctx, oracle, letter):
    for case in pc.TABLES[letter]():
        raw, om, oi = _upload(ctx, case), capi.Scan(ctx), capi.Scan(ctx) if case.want_icp else None
        raw.preprocess(_params(case), om, oi)
        _check_case(case, om, oi)
        cm, ci = oracle.preprocess(case.xyz, **case.pp)  # the C oracle as well
        np.testing.assert_array_equal(om.download()["src_idx"], cm, err_msg=case.name)
        if case.want_icp:
            np.testing.assert_array_equal(oi.download()["src_idx"], ci, err_msg=case.name)
        if case.t is not None:
            np.testing.assert_array_equal(om.download()["t"], oracle.adjust_timestamps(case.t, case.ts_method, case.ts_offset)[cm], err_msg=case.name)
        for s in (raw, om, oi):
            if s is not None:
                s.close()


@pytest.mark.parametrize("order", ["table_order", "reversed"])
@pytest.mark.parametrize("letter", sorted(pc.TABLES))
def test_chain_table_as_one_batch(pool, letter, order):
    cases = pc.TABLES[letter]()
    cases = cases[::-1] if order == "reversed" else cases
    ctxs = pool(len(cases))
    raws = [_upload(c, case) for c, case in zip(ctxs, cases)]
    oms = [capi.Scan(c) for c in ctxs]
    ois = [capi.Scan(c) if case.want_icp else None for c, case in zip(ctxs, cases)]
    capi.preprocess_batch(raws, [_params(case) for case in cases], oms, ois)
    for case, om, oi in zip(cases, oms, ois):
        _check_case(case, om, oi)
    for s in raws + oms + ois:
        if s is not None:
            s.close()


def _layers_equal(om, oi, im, ii, xyz, what):
    for scan, idx in ((om, im), (oi, ii)):
        assert scan.n == len(idx), what
        d = scan.download()
        np.testing.assert_array_equal(d["src_idx"], idx, err_msg=what)
        np.testing.assert_array_equal(_bits(d["xyz"]), _bits(np.asarray(xyz, F)[idx]), err_msg=what)


def test_key_range(ctx, pool):
    """A finite point whose |x / res| reaches 1e6: a decimating stage leaves it out and the call returns MH_ERR_OUT_OF_RANGE with
    both outputs complete (the chain's result for the scan without the point); a stage that does not decimate passes it; a
    non-finite point raises nothing; the next call on the context is an ordinary one; in a batch the other jobs are complete."""
    om, oi = capi.Scan(ctx), capi.Scan(ctx)
    pp = pc.g_params()

    def run(xyz, pp_, fails):
        raw = capi.Scan(ctx, xyz)
        if fails:
            with pytest.raises(capi.MolahipError) as e:
                raw.preprocess(capi.preprocess_params(**pp_), om, oi)
            assert e.value.status == ERR_OUT_OF_RANGE
        else:
            raw.preprocess(capi.preprocess_params(**pp_), om, oi)
        raw.close()

    for x in (pc.G_LIMIT_X, -pc.G_LIMIT_X, 6.0e5):  # both stages decimate
        xyz = pc.g_with(x)
        run(xyz, pp, True)
        _layers_equal(om, oi, *pc.chain_without(xyz, pp, pc.G_AT), xyz, "decimating, x = %g" % x)
        run(pc.g_cloud(), pp, False)  # the context is as good as before
        _layers_equal(om, oi, *ref.chain(pc.g_cloud(), pp), pc.g_cloud(), "ordinary call after the failed one")
    xyz = pc.g_with(np.nextafter(F(pc.G_LIMIT_X), F(0)))  # one float inside the range: an ordinary point in a cell of its own
    run(xyz, pp, False)
    _layers_equal(om, oi, *ref.chain(xyz, pp), xyz, "just inside")
    assert pc.G_AT in om.download()["src_idx"]
    xyz = pc.g_with(pc.G_LIMIT_X)
    for name, quiet in (("resolution 0", pc.g_params(decim_map_resolution=0.0, decim_icp_resolution=0.0)),
                        ("below the minimum", pc.g_params(min_points_to_filter=len(xyz) + 1))):
        run(xyz, quiet, False)
        _layers_equal(om, oi, *ref.chain(xyz, quiet), xyz, name)
        assert pc.G_AT in om.download()["src_idx"] and pc.G_AT in oi.download()["src_idx"]
    # the first stage passes the point, the second (at the resolution that puts it out of range) leaves it out and raises
    second_only = pc.g_params(decim_map_resolution=0.0, decim_icp_resolution=pc.G_RES)
    run(xyz, second_only, True)
    _layers_equal(om, oi, ref.chain(xyz, second_only)[0], pc.chain_without(xyz, second_only, pc.G_AT)[1], xyz, "second stage only")
    xyz_nan = pc.g_with(np.nan)
    run(xyz_nan, pp, False)
    _layers_equal(om, oi, *ref.chain(xyz_nan, pp), xyz_nan, "non-finite")
    # a batch: the offending job fails the call, every job's outputs are complete and equal to their single calls
    clouds = [pc.g_cloud(), pc.g_with(pc.G_LIMIT_X), pc.g_cloud()[::-1].copy()]
    pps = [pp, pp, pc.g_params(index_mode=ref.INDEX_TRUNC)]
    ctxs = pool(3)
    raws = [capi.Scan(c, x) for c, x in zip(ctxs, clouds)]
    oms, ois = [capi.Scan(c) for c in ctxs], [capi.Scan(c) for c in ctxs]
    with pytest.raises(capi.MolahipError) as e:
        capi.preprocess_batch(raws, [capi.preprocess_params(**p) for p in pps], oms, ois)
    assert e.value.status == ERR_OUT_OF_RANGE
    for k in range(3):
        want = pc.chain_without(clouds[k], pps[k], pc.G_AT) if k == 1 else ref.chain(clouds[k], pps[k])
        _layers_equal(oms[k], ois[k], *want, clouds[k], "batch job %d" % k)
        sm, si = capi.Scan(ctxs[k]), capi.Scan(ctxs[k])
        try:
            raws[k].preprocess(capi.preprocess_params(**pps[k]), sm, si)
            assert k != 1
        except capi.MolahipError as err:
            assert k == 1 and err.status == ERR_OUT_OF_RANGE
        for got, single in ((oms[k], sm), (ois[k], si)):
            a, b = got.download(), single.download()
            np.testing.assert_array_equal(a["src_idx"], b["src_idx"])
            np.testing.assert_array_equal(_bits(a["xyz"]), _bits(b["xyz"]))


def test_bbox_against_reference(ctx):
    """mh_scan_bbox == numpy's min / max over the finite rows, count included: k_pp_bbox_one up to 65 536 points, k_pp_bbox above"""
    for name, xyz in pc.table_h():
        s = capi.Scan(ctx, xyz) if len(xyz) else capi.Scan(ctx)
        mn, mx, cnt = s.bbox()
        rmn, rmx, rcnt = ref.bbox(xyz)
        assert cnt == rcnt, name
        np.testing.assert_array_equal(mn, rmn, err_msg=name)
        np.testing.assert_array_equal(mx, rmx, err_msg=name)
        s.close()


def _derived_layer(ctx, xyz, t, inten):
    """the layer as a filter chain hands it on: a pass-through of a raw scan that has three NaN rows more, so that the layer
    carries source indices that are not 0..n-1, stamps and intensity"""
    n = len(xyz) + 3
    drop = np.array([0, n // 2, n - 1])
    keep = np.delete(np.arange(n), drop)
    rx, rt, ri = np.full((n, 3), np.nan, F), np.zeros(n, F), np.zeros(n, F)
    rx[keep], rt[keep], ri[keep] = xyz, t, inten
    raw = capi.Scan(ctx, rx).set_timestamps(rt).set_intensity(ri)
    layer = capi.Scan(ctx)
    raw.preprocess(capi.preprocess_params(**ref.params()), layer, None)
    raw.close()
    return layer, keep.astype(np.uint32)


@pytest.mark.parametrize("variant", ["plain_with_nonfinite", "derived_with_src_and_intensity"])
def test_deskew_edges(ctx, variant):
    """mh_scan_deskew and mh_scan_deskew_pair over the twists and stamps of table I (theta = 0, 1e-9, either side of the series
    switch at 1e-2, 0.5, 3; zero angular rate; zero linear rate) and layer pairs around the pair kernel's 1 024-point workgroups.
    Measured on an MI355X against the long-double reference: see profiles/preprocess_edges.md (recorded, not a threshold)."""
    worst = (0.0, "")
    for big_n, small_n in pc.I_PAIRS:
        layers = []
        for tag, n in (("big", big_n), ("small", small_n)):
            if variant == "plain_with_nonfinite":
                xyz, t, inten = pc.i_layer(tag, n, nonfinite=True)
                inten = inten if tag == "big" else None  # one layer with an intensity, one without
                scan = capi.Scan(ctx, xyz).set_timestamps(t)
                if inten is not None:
                    scan.set_intensity(inten)
                src = None
            else:
                xyz, t, inten = pc.i_layer(tag, n, nonfinite=False)
                scan, src = _derived_layer(ctx, xyz, t, inten)
            assert scan.n == n
            layers.append((scan, xyz, t, inten, src))
        (big, *_), (small, *_) = layers
        for tw_name, tw in pc.I_TWISTS.items():
            what = "%s big %d small %d" % (tw_name, big_n, small_n)
            a, b, a1, b1 = (capi.Scan(ctx) for _ in range(4))
            mn, mx, nf = big.deskew_pair(small, tw, a, b)
            big.deskew(tw, a1)
            small.deskew(tw, b1)
            for got, sep, (scan, xyz, t, inten, src) in ((a, a1, layers[0]), (b, b1, layers[1])):
                d, ds = got.download(), sep.download()
                assert got.n == sep.n == len(xyz), what
                np.testing.assert_array_equal(_bits(d["xyz"]), _bits(ds["xyz"]), err_msg=what)  # pair == separate, bit for bit
                for dd in (d, ds):  # what rides along is carried unchanged
                    np.testing.assert_array_equal(_bits(dd["t"]), _bits(t), err_msg=what)
                    if src is not None:
                        np.testing.assert_array_equal(dd["src_idx"], src, err_msg=what)
                if inten is not None:
                    np.testing.assert_array_equal(_bits(got.download_intensity()), _bits(inten), err_msg=what)
                    np.testing.assert_array_equal(_bits(sep.download_intensity()), _bits(inten), err_msg=what)
                fin = ref.finite_rows(xyz)
                assert not np.isfinite(d["xyz"][~fin]).all(axis=1).any(), what  # a non-finite point stays non-finite
                want = ref.deskew(xyz[fin], t[fin], tw)
                err = np.abs(d["xyz"][fin].astype(ref.L) - want)
                bound = ref.deskew_bound(xyz[fin], t[fin], tw, want)
                u = ref.ulps32(d["xyz"][fin], want)
                if u.size and float(u.max()) > worst[0]:
                    worst = (float(u.max()), what)
                assert (err <= bound).all(), (what, float((err / bound).max()), int(np.argmax((err / bound).max(axis=1))))
            db = b.download()["xyz"]
            rmn, rmx, rcnt = ref.bbox(db)  # the pair's box == the box of the pair's own output, exactly
            assert nf == rcnt == int(ref.finite_rows(layers[1][1]).sum()), what
            np.testing.assert_array_equal(mn, rmn, err_msg=what)
            np.testing.assert_array_equal(mx, rmx, err_msg=what)
            bmn, bmx, bnf = b1.bbox()
            assert bnf == nf and np.array_equal(bmn, mn) and np.array_equal(bmx, mx), what
            for s in (a, b, a1, b1):
                s.close()
        for scan, xyz, t, inten, src in layers:  # the input layers are untouched
            d = scan.download()
            np.testing.assert_array_equal(_bits(d["xyz"]), _bits(xyz))
            if src is not None:
                np.testing.assert_array_equal(d["src_idx"], src)
            np.testing.assert_array_equal(_bits(d["t"]), _bits(t))
            scan.close()
    print("de-skew on the device vs the long-double reference (%s): largest difference %.4f float ulps, at %s" % (variant, worst[0], worst[1]))
