"""No GPU: the references that tests/test_gpu_preprocess_edges.py holds the device to are sound, and its case tables have the
properties they were built for.

  * for every case of tables A-F of tests/preprocess_cases.py the numpy restatement (tests/preprocess_ref.py) and the C oracle
    give the same index sets and the same adjusted stamps, bit for bit (stamps by value);
  * from the reference alone: the run positions of C, the survivor counts of E, for F every threshold point kept and its
    one-step-out neighbour dropped, for D different sets under TRUNC and FLOOR -- so no case quietly tests nothing;
  * the one toleranced comparison: the long-double de-skew, rounded to float32, against the oracle's fp64 one, inside the
    bound preprocess_ref.deskew_bound derives."""
import numpy as np
import pytest

import preprocess_cases as pc
import preprocess_ref as ref

F = np.float32


@pytest.mark.parametrize("letter", sorted(pc.TABLES))
def test_reference_equals_oracle(oracle, letter):
    for case in pc.TABLES[letter]():
        im, ii, ta = pc.expected(case)
        om, oi = oracle.preprocess(case.xyz, **case.pp)
        np.testing.assert_array_equal(im, om, err_msg=case.name)
        np.testing.assert_array_equal(ii, oi, err_msg=case.name)
        assert np.all(np.diff(im.astype(np.int64)) > 0) and np.isin(ii, im).all(), case.name
        if case.t is not None:
            np.testing.assert_array_equal(ta, oracle.adjust_timestamps(case.t, case.ts_method, case.ts_offset), err_msg=case.name)


def test_single_filters_equal_oracle(oracle):
    """the pieces of the chain one by one, on the clouds where each decides something"""
    for case in pc.table_d() + pc.table_c()[::4]:
        res, mode = case.pp["decim_map_resolution"] or case.pp["decim_icp_resolution"], case.pp["index_mode"]
        np.testing.assert_array_equal(ref.decimate_first(case.xyz, res, 0, mode), oracle.decimate_first_point(case.xyz, res, 0, mode))
        np.testing.assert_array_equal(ref.decimate_closest(case.xyz, res, 0, mode), oracle.decimate_closest_to_average(case.xyz, res, 0, mode))
        n = len(case.xyz)
        np.testing.assert_array_equal(ref.decimate_first(case.xyz, res, n + 1, mode), np.nonzero(ref.finite_rows(case.xyz))[0])
    xyz, _ = pc.f_points()
    np.testing.assert_array_equal(np.nonzero(ref.by_range(xyz, pc.F_RMIN, pc.F_RMAX, pc.F_CENTRE))[0],
                                  oracle.filter_by_range(xyz, pc.F_RMIN, pc.F_RMAX, pc.F_CENTRE))
    for mode in (ref.BBOX_KEEP_INSIDE, ref.BBOX_KEEP_OUTSIDE):
        np.testing.assert_array_equal(np.nonzero(ref.by_box(xyz, pc.F_BMIN, pc.F_BMAX, mode))[0],
                                      oracle.filter_bbox(xyz, pc.F_BMIN, pc.F_BMAX, mode == ref.BBOX_KEEP_INSIDE))


def test_table_a_and_b_properties():
    assert {len(c.xyz) for c in pc.table_a()} == set(pc.SIZES)
    assert {c.want_icp for c in pc.table_a()} == {True, False}
    for case in pc.table_a():
        im, ii, ta = pc.expected(case)
        n = len(case.xyz)
        assert (case.t < 0).any() or n < 3
        if n >= 1023:  # every stage of the chain drops something and leaves something
            assert 0 < len(ii) < len(im) < n, case.name
    by_name = {c.name: c for c in pc.table_b()}
    for where, k in (("first", 0), ("last", 199), ("lane63", 63)):
        assert int(np.argmin(by_name["B-mixed_min_%s-m1" % where].t)) == k and int(np.argmax(by_name["B-mixed_max_%s-m1" % where].t)) == k
    assert (by_name["B-all_negative-m2"].t < 0).all() and np.ptp(by_name["B-all_equal-m1"].t) == 0
    assert by_name["B-tiny_negative-m2"].t.max() == F(-1e-30) and by_name["B-tiny_positive-m2"].t.min() == F(1e-30)
    for case in pc.table_b():
        assert np.isfinite(case.t).all() and case.ts_offset != 0.0
        ta = pc.expected(case)[2]
        if case.ts_method == ref.TS_EARLIEST_IS_ZERO:  # (t - tmin) + offset: the earliest stamp lands on the offset exactly
            assert ta.min() == F(case.ts_offset), case.name


def test_table_c_has_its_runs():
    """the cell sequence along the array, recomputed from the points by the reference, is the one the table names"""
    arrangements = pc.c_arrangements()
    for case in pc.table_c()[::4]:
        seq, nans = arrangements[case.props["arrangement"]]
        cells, ok = ref.cells(case.xyz, pc.C_RES, ref.INDEX_FLOOR)
        fin = ref.finite_rows(case.xyz)
        assert sorted(np.nonzero(~fin)[0]) == sorted(nans) and ok[fin].all(), case.name
        np.testing.assert_array_equal(cells[fin], pc.cell_xyz(seq)[fin], err_msg=case.name)
    seq = arrangements["run59_68"][0]
    assert len(set(seq[59:69])) == 1 and seq[58] != seq[59] != seq[69] and 59 <= 63 < 64 <= 68
    seq = arrangements["run251_260"][0]
    assert len(set(seq[251:261])) == 1 and seq[250] != seq[251] != seq[261] and 251 <= 255 < 256 <= 260
    for name in ("run59_68_first_before", "run251_260_first_before", "run123_132_first_before"):
        seq = arrangements[name][0]
        lo = int(name[3:].split("_")[0])
        assert seq[5] == seq[lo] and 5 < lo - 1 and seq[lo - 1] != seq[lo]
    for n in (32, 2048):  # half load: the table of n points is the power of two >= 2 n (at least 64)
        assert len(set(arrangements["own_cell_n%d" % n][0])) == n and max(64, 1 << int(np.ceil(np.log2(2 * n)))) == 2 * n
    # the survivors say the same: one per cell, the run's first index (FirstPoint, first stage)
    by_name = {c.name: c for c in pc.table_c()}
    assert list(pc.expected(by_name["C-one_cell_n1000-stage1-method0"])[0]) == [0]
    im = pc.expected(by_name["C-run59_68-stage1-method0"])[0]
    assert 59 in im and not set(range(60, 69)) & set(im) and len(im) == 320 - 9
    im = pc.expected(by_name["C-run59_68_nan_edge_hi-stage1-method0"])[0]
    assert 59 in im and not set(range(60, 69)) & set(im) and len(im) == 320 - 9
    im = pc.expected(by_name["C-run251_260_first_before-stage1-method0"])[0]
    assert 5 in im and not set(range(251, 261)) & set(im)
    assert len(pc.expected(by_name["C-abab-stage2-method0"])[1]) == 2
    # ClosestToAverage picks other points than FirstPoint somewhere
    assert not np.array_equal(pc.expected(by_name["C-one_cell_n1000-stage1-method1"])[0], [0])


def test_table_d_modes_differ():
    by_name = {c.name: c for c in pc.table_d()}
    for res in pc.D_RES:
        for method in (0, 1):
            floor_, trunc_ = (pc.expected(by_name["D-res%g-mode%d-method%d" % (res, mode, method)]) for mode in (0, 1))
            assert not np.array_equal(floor_[0], trunc_[0]), (res, method)
            if method == 0:  # rows 0..3 are -0.3 res on x, y, z and all three: four cells under FLOOR, the cell of +0.3 res under TRUNC
                assert set(range(4)) <= set(floor_[0]) and set(range(1, 4)).isdisjoint(trunc_[0]) and 0 in trunc_[0]
        xyz = pc.d_points(res)
        cf, _ = ref.cells(xyz, res, ref.INDEX_FLOOR)
        ct, _ = ref.cells(xyz, res, ref.INDEX_TRUNC)
        neg = (xyz < 0) & (xyz > -F(res))
        assert neg.any() and (cf[neg] == -1).all() and (ct[neg] == 0).all()
        assert (cf[xyz == 0] == 0).all()  # (+-0.0 alike)


def test_table_e_counts():
    for case in pc.table_e():
        im, ii, _ = pc.expected(case)
        N = case.props["N"]
        assert len(case.xyz) == pc.E_RAW and len(im) == N, case.name
        if N < pc.E_MIN:
            np.testing.assert_array_equal(ii, im)  # below the minimum: the second decimation passes its input
        else:
            coarse, _ = ref.cells(case.xyz[im], 2 * pc.E_RES, ref.INDEX_FLOOR)
            assert len(ii) == len(np.unique(coarse, axis=0)) < pc.E_COUNTS[0], case.name


def test_table_f_thresholds():
    xyz, tags = pc.f_points()
    by_name = {c.name: c for c in pc.table_f()}
    idx = lambda kind, where: [k for k, tg in enumerate(tags) if tg == (kind, where)]
    sq = ref.range_sq(xyz, pc.F_CENTRE)
    assert (sq[idx("range_on_min", "on")] == F(pc.F_RMIN) ** 2).all() and (sq[idx("range_on_max", "on")] == F(pc.F_RMAX) ** 2).all()
    assert any(v != 0 for v in pc.F_CENTRE)
    kept = set(pc.expected(by_name["F-range"])[0])
    for kind in ("range_on_min", "range_on_max"):
        assert len(idx(kind, "on")) == 5
        assert set(idx(kind, "on")) <= kept and set(idx(kind, "in")) <= kept and not set(idx(kind, "out")) & kept
    inside = set(pc.expected(by_name["F-box_inside"])[0])
    outside = set(pc.expected(by_name["F-box_outside"])[0])
    assert len(idx("box_face", "on")) == 6
    assert set(idx("box_face", "on")) <= inside and set(idx("box_face", "in")) <= inside and not set(idx("box_face", "out")) & inside
    assert set(idx("box_face", "out")) <= outside and not set(idx("box_face", "on") + idx("box_face", "in")) & outside
    assert inside | outside == set(range(len(xyz))) and not inside & outside
    for name in ("F-range_off_zero_max", "F-range_off_negative_max"):
        assert len(pc.expected(by_name[name])[0]) == len(xyz) and by_name[name].pp["range_min"] > 0


def test_key_range_verdicts():
    for x, inside in ((pc.G_LIMIT_X, False), (-pc.G_LIMIT_X, False), (np.nextafter(F(pc.G_LIMIT_X), F(0)), True), (6.0e5, False)):
        _, ok = ref.cells(pc.g_with(x), pc.G_RES, ref.INDEX_FLOOR)
        assert ok[pc.G_AT] == inside and ok.sum() == len(ok) - (not inside)
    _, ok = ref.cells(pc.g_with(np.nan), pc.G_RES, ref.INDEX_FLOOR)
    assert not ok[pc.G_AT]  # (not finite: no cell, and nothing to raise)
    # in a cell of its own, so the chain without it is the chain with it minus that index
    pp = pc.g_params()
    xyz = pc.g_with(pc.G_LIMIT_X)
    im, ii = ref.chain(xyz, pp)
    wm, wi = pc.chain_without(xyz, pp, pc.G_AT)
    assert pc.G_AT in im and pc.G_AT in ii
    np.testing.assert_array_equal(np.setdiff1d(im, [pc.G_AT]), wm)
    np.testing.assert_array_equal(np.setdiff1d(ii, [pc.G_AT]), wi)


def test_bbox_table_properties():
    names = [name for name, _ in pc.table_h()]
    assert len(set(names)) == len(names)
    assert pc.h_last_wave_index(70001) == 65525 and pc.h_last_wave_index(65536) == 65525 and pc.h_last_wave_index(1025) == 1013
    for name, xyz in pc.table_h():
        mn, mx, cnt = ref.bbox(xyz)
        if name.startswith("H-extremes_"):
            np.testing.assert_array_equal(mn, [-99, -98, -97])
            np.testing.assert_array_equal(mx, [96, 95, 94])
        if "nonfinite_rows_would_be" in name:
            assert cnt == len(xyz) - 4 and np.abs(mn).max() <= 10 and np.abs(mx).max() <= 10
        if "all_rows_nonfinite" in name or name == "H-empty":
            assert cnt == 0 and not mn.any() and not mx.any()
        if name == "H-subnormal_extremes":
            assert (mn == F(-1e-40)).all() and (mx == F(1e-40)).all() and F(1e-40) != 0
        if name == "H-huge_and_tiny":
            assert (mn == F(-3e38)).all() and (mx == F(3e38)).all()
        if name == "H-negative_zero_is_max":
            assert (mx == 0).all() and (mn < 0).all()


def test_deskew_reference_against_oracle(oracle, monkeypatch):
    """long double, rounded once to float32, against the oracle's fp64 se3 exponential rounded to float32: within the bound that
    the device is held to (one float ulp + 16 * 2^-52 * (|x| + |y| + |z| + |v t|)).  Prints what it observed."""
    worst, equal, total = 0.0, 0, 0
    for big, small in pc.I_PAIRS:
        for tag, n in (("big", big), ("small", small)):
            xyz, t, _ = pc.i_layer(tag, n, nonfinite=False)
            for name, tw in pc.I_TWISTS.items():
                want = ref.deskew(xyz, t, tw)
                got = oracle.deskew(xyz, t, tw)
                bound = ref.deskew_bound(xyz, t, tw, want)
                err = np.abs(got.astype(ref.L) - want)
                assert (err <= bound).all(), (name, n, float((err / bound).max()))
                worst = max(worst, float(ref.ulps32(got, want).max()))
                equal += int((got == want.astype(F)).sum())
                total += got.size
    print("de-skew, long-double reference vs C oracle: largest difference %.4f float ulps, %.4f %% of %d coordinates bit-equal"
          % (worst, 100.0 * equal / total, total))
    assert equal > 0.99 * total
    # the reference itself at its own switch: below it the three series terms and the closed form agree to long-double rounding
    t = np.array([1e-9, 5e-5, 9.9e-5], F)
    p = np.array([[1.0, 2.0, 3.0]] * 3, F)
    series = ref.deskew(p, t, pc.I_TWISTS["unit_rate"])
    monkeypatch.setattr(ref, "SERIES_BELOW", ref.L(0))
    assert np.abs(ref.deskew(p, t, pc.I_TWISTS["unit_rate"]) - series).max() < 1e-16
    monkeypatch.undo()
    # theta = 0: the linear part alone
    np.testing.assert_array_equal(ref.deskew(p[:1], np.zeros(1, F), pc.I_TWISTS["unit_rate"]).astype(F), p[:1])
