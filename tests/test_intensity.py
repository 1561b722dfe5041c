"""The optional intensity channel of device layers and the two intensity filters (mh_scan_normalize_intensity,
mh_scan_by_intensity): numpy float32 restatements of the rules include/molahip.h states, pinned on hand-built cases (CPU),
the ctypes layout of mh_by_intensity_params and the new symbols (CPU), and on the GPU: the channel's round trips, the
propagation contract out.i[k] == raw.i[out.src_idx[k]] through every call that derives a layer, and both filters against
their restatements bit for bit."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

from mola_lidar_odometry_amd import capi
from oracle.filters_np import HIGH, LOW, MID, _ord, by_intensity_np, intensity_classes, normalize_np  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MH_ERR_INVALID_ARGUMENT = 1  # include/molahip.h
NEW_SYMBOLS = ("mh_scan_set_intensity", "mh_scan_update_aos_i", "mh_scan_download_intensity", "mh_scan_normalize_intensity",
               "mh_scan_by_intensity")


# ------------------------------------------------------------------------------------------------ CPU: the restatements
def test_normalize_maps_the_range_to_unit_interval():
    out, r = normalize_np([2.0, 4.0, 3.0, 6.0])
    assert out.tolist() == [0.0, 0.5, 0.25, 1.0] and r is None


def test_normalize_keeps_nan_and_ignores_it_for_the_range():
    out, _ = normalize_np([np.nan, 1.0, 3.0, np.nan])
    assert np.isnan(out[0]) and np.isnan(out[3]) and out[1:3].tolist() == [0.0, 1.0]


def test_normalize_all_equal_gives_zero():
    out, r = normalize_np([5.0, 5.0, 5.0], np.array([np.nan, np.nan], np.float32))
    assert out.tolist() == [0.0, 0.0, 0.0] and r.tolist() == [5.0, 5.0]


def test_normalize_empty_and_all_nan_change_nothing():
    for vals in ([], [np.nan, np.nan]):
        rng = np.array([np.nan, np.nan], np.float32)
        out, r = normalize_np(vals, rng)
        assert out.tobytes() == np.asarray(vals, np.float32).tobytes() and np.isnan(r).all()
    # nothing in the layer but a remembered range: the range stays, the (empty) layer too
    out, r = normalize_np([], np.array([1.0, 2.0], np.float32))
    assert len(out) == 0 and r.tolist() == [1.0, 2.0]


def test_normalize_remembered_range_widens():
    out, r = normalize_np([2.0, 3.0], np.array([0.0, 4.0], np.float32))
    assert out.tolist() == [0.5, 0.75] and r.tolist() == [0.0, 4.0]
    out, r = normalize_np([-1.0, 3.0], np.array([0.0, 2.0], np.float32))
    assert r.tolist() == [-1.0, 3.0] and out.tolist() == [0.0, 1.0]
    # a sequence: the range only grows
    r = np.array([np.nan, np.nan], np.float32)
    for vals, want in (([1.0, 2.0], [1.0, 2.0]), ([1.5], [1.0, 2.0]), ([0.5, 1.2], [0.5, 2.0]), ([3.0], [0.5, 3.0])):
        _, r = normalize_np(vals, r)
        assert r.tolist() == want


def test_normalize_is_float_unfused():
    i = np.array([0.1, 0.7, 0.3], np.float32)
    out, _ = normalize_np(i)
    f = np.float32
    k = f(1.0) / (f(0.7) - f(0.1))
    assert out[2] == (f(0.3) - f(0.1)) * k


def test_by_intensity_thresholds_are_strict_and_nan_is_mid():
    f = np.float32
    i = [0.0, 0.1, 0.5, 0.9, 1.0, np.nan, np.nextafter(f(0.1), f(0)), np.nextafter(f(0.9), f(1)), -np.inf, np.inf]
    assert intensity_classes(i).tolist() == [LOW, MID, MID, MID, HIGH, MID, LOW, HIGH, LOW, HIGH]
    # low above high: everything below low is low first, the rest above high is high
    assert intensity_classes([0.2, 0.5, 0.8], low=0.6, high=0.4).tolist() == [LOW, LOW, HIGH]


def test_by_intensity_outputs_keep_order_and_channels():
    rng = np.random.default_rng(4)
    xyz = rng.normal(0, 5, (300, 3)).astype(np.float32)
    i = rng.uniform(-0.2, 1.2, 300).astype(np.float32)
    t = rng.uniform(-0.05, 0.05, 300).astype(np.float32)
    src = np.sort(rng.choice(9000, 300, replace=False)).astype(np.uint32)
    outs = by_intensity_np(xyz, i, t, src)
    assert sum(len(o["src_idx"]) for o in outs) == 300
    for o in outs:
        assert (np.diff(o["src_idx"].astype(np.int64)) > 0).all()
        k = np.searchsorted(src, o["src_idx"])
        assert (o["xyz"] == xyz[k]).all() and (o["i"] == i[k]).all() and (o["t"] == t[k]).all()


# ------------------------------------------------------------------------------------------------ CPU: the boundary
def test_by_intensity_params_layout_matches_c(tmp_path):
    prog = tmp_path / "bp.c"
    prog.write_text(r'''
#include <stdio.h>
#include <stddef.h>
#include "molahip.h"
int main(void){
  printf("%zu %zu %zu\n", sizeof(mh_by_intensity_params), offsetof(mh_by_intensity_params, low_threshold),
    offsetof(mh_by_intensity_params, high_threshold));
  return 0; }''')
    exe = tmp_path / "bp"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    vals = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    P = capi.ByIntensityParams
    assert vals == [C.sizeof(P), P.low_threshold.offset, P.high_threshold.offset]
    p = capi.by_intensity_params()
    assert (p.low_threshold, p.high_threshold) == (np.float32(0.1), np.float32(0.9))


def test_intensity_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "molahip.h")).read()
    L = capi.lib()
    for name in NEW_SYMBOLS:
        assert f"MH_API mh_status {name}(" in header, name
        assert hasattr(L, name) and name in capi._SIGNATURES, name
    for meth in ("set_intensity", "download_intensity", "normalize_intensity", "by_intensity", "update_interleaved_i"):
        assert callable(getattr(capi.Scan, meth)), meth
    assert callable(capi.scan_normalize_intensity) and callable(capi.scan_by_intensity)
    assert int(L.mh_abi_version()) == capi._header_abi_version() == 7


# ------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def ctx():
    return capi.Context(0)


def _scan(ctx, xyz, i=None, t=None):
    s = capi.Scan(ctx, np.asarray(xyz, np.float32))
    if t is not None:
        s.set_timestamps(t)
    if i is not None:
        s.set_intensity(i)
    return s


def _has_i(scan):
    try:
        scan.download_intensity()
        return True
    except capi.MolahipError as e:
        assert e.status == MH_ERR_INVALID_ARGUMENT
        return False


def _check_propagated(out, raw_i):
    """The contract: out.i[k] == raw.i[out.src_idx[k]], bit for bit."""
    d = out.download()
    got = out.download_intensity()
    assert got.tobytes() == np.asarray(raw_i, np.float32)[d["src_idx"]].tobytes()


def _drive_scan(k=1):
    from mola_lidar_odometry_amd import synth
    d = synth.make_drive(k + 1)
    xyz, t = (np.asarray(a, np.float32) for a in d["scans"][k])
    return xyz, t, synth.drive_intensities(d)[k]


@pytest.mark.gpu
def test_device_set_and_download_round_trip(ctx):
    rng = np.random.default_rng(1)
    xyz = rng.normal(0, 3, (1001, 3)).astype(np.float32)
    i = rng.uniform(0, 255, 1001).astype(np.float32)
    i[::97] = np.nan
    s = _scan(ctx, xyz)
    assert not _has_i(s)
    s.set_intensity(i)
    assert s.download_intensity().tobytes() == i.tobytes()
    with pytest.raises(capi.MolahipError):
        s.set_intensity(i[:-1])  # count differs from the scan size
    s.update(xyz[:10])  # new points: the channel is gone
    assert not _has_i(s)


@pytest.mark.gpu
@pytest.mark.parametrize("k, fields", [(4, (0, 1, 2, 3)), (5, (1, 2, 3, 4)), (6, (3, 0, 5, 1)), (8, (7, 2, 4, 6))])
def test_device_update_aos_i_round_trip(ctx, k, fields):
    """Records of k float32 fields with x, y, z, intensity at the given columns (permuted), plus a time stamp column when one
    is free: the SoA channels come back bit for bit; update_aos / update drop the intensity."""
    rng = np.random.default_rng(k)
    n = 3000 + k
    rec = rng.normal(0, 10, (n, k)).astype(np.float32)
    fx, fy, fz, fi = fields
    free = [c for c in range(k) if c not in fields]
    ft = free[0] if free else -1
    s = capi.Scan(ctx)
    s.update_interleaved_i(rec, 4 * fx, 4 * fy, 4 * fz, 4 * ft if ft >= 0 else -1, 4 * fi)
    d = s.download()
    assert d["xyz"].tobytes() == np.ascontiguousarray(rec[:, [fx, fy, fz]]).tobytes()
    assert s.download_intensity().tobytes() == np.ascontiguousarray(rec[:, fi]).tobytes()
    if ft >= 0:
        assert d["t"].tobytes() == np.ascontiguousarray(rec[:, ft]).tobytes()
    s.update_interleaved(rec, 4 * fx, 4 * fy, 4 * fz)
    assert not _has_i(s) and s.download()["xyz"].tobytes() == np.ascontiguousarray(rec[:, [fx, fy, fz]]).tobytes()
    s.update_interleaved_i(rec, 4 * fx, 4 * fy, 4 * fz, -1, 4 * fi)
    assert _has_i(s)
    s.update(rec[:, :3])
    assert not _has_i(s)
    with pytest.raises(capi.MolahipError):
        s.update_interleaved_i(rec, 0, 4, 8, -1, 4 * k)  # outside the record


@pytest.mark.gpu
@pytest.mark.parametrize("method", [capi.DECIMATE_FIRST_POINT, capi.DECIMATE_CLOSEST_TO_AVERAGE])
def test_device_preprocess_carries_intensity(ctx, method):
    xyz, t, i = _drive_scan()
    raw = _scan(ctx, xyz, i, t)
    pp = capi.preprocess_params(0.4, 1.2, min_points_to_filter=0, range_min=1.0, range_max=60.0, bbox_mode=capi.BBOX_KEEP_OUTSIDE,
                                bbox_min=(-3, -3, 0.5), bbox_max=(3, 3, 4), timestamp_method=capi.TS_MIDDLE_IS_ZERO,
                                decim_map_method=method, decim_icp_method=method)
    om, oi = capi.Scan(ctx), capi.Scan(ctx)
    raw.preprocess(pp, om, oi)
    assert 0 < len(oi) < len(om) < len(xyz)
    _check_propagated(om, i)
    _check_propagated(oi, i)
    # the same without intensity: same points, no channel
    plain = _scan(ctx, xyz, None, t)
    pm, pi = capi.Scan(ctx), capi.Scan(ctx)
    plain.preprocess(pp, pm, pi)
    assert not _has_i(pm) and not _has_i(pi)
    for a, b in ((om, pm), (oi, pi)):
        da, db = a.download(), b.download()
        assert all(da[key].tobytes() == db[key].tobytes() for key in ("xyz", "t", "src_idx"))


@pytest.mark.gpu
def test_device_preprocess_batch_mixes_jobs_with_and_without_intensity(ctx):
    xyz, t, i = _drive_scan()
    raws = [_scan(ctx, xyz, i, t), _scan(ctx, xyz[::2], None, t[::2]), _scan(ctx, xyz[1::3], i[1::3], None)]
    pp = capi.preprocess_params(0.3, 1.0, min_points_to_filter=0, range_min=0.5, range_max=80.0)
    oms, ois = [capi.Scan(ctx) for _ in raws], [capi.Scan(ctx) for _ in raws]
    capi.preprocess_batch(raws, pp, oms, ois)
    _check_propagated(oms[0], i)
    _check_propagated(ois[0], i)
    assert not _has_i(oms[1]) and not _has_i(ois[1])
    _check_propagated(oms[2], i[1::3])
    _check_propagated(ois[2], i[1::3])


@pytest.mark.gpu
def test_device_deskew_and_pair_carry_intensity(ctx):
    xyz, t, i = _drive_scan()
    raw = _scan(ctx, xyz, i, t)
    twist = np.array([8.0, 0.1, 0.0, 0.0, 0.0, 0.12])
    for tw in (twist, None):  # the kernel and the copy
        out = capi.Scan(ctx)
        raw.deskew(tw, out)
        assert out.download_intensity().tobytes() == i.tobytes()
    pp = capi.preprocess_params(0.4, 1.2, min_points_to_filter=0)
    om, oi = capi.Scan(ctx), capi.Scan(ctx)
    raw.preprocess(pp, om, oi)
    for tw in (twist, None):  # the fused launch and the fallback
        a, b = capi.Scan(ctx), capi.Scan(ctx)
        om.deskew_pair(oi, tw, a, b)
        _check_propagated(a, i)
        _check_propagated(b, i)


@pytest.mark.gpu
def test_device_curvature_carries_intensity(ctx):
    xyz, t, i = _drive_scan()
    raw = _scan(ctx, xyz, i, t)
    outs = [capi.Scan(ctx) for _ in range(3)]
    raw.curvature(capi.curvature_params(), *outs)
    assert sum(len(o) for o in outs) == len(xyz) - 2
    for o in outs:
        _check_propagated(o, i)


def _c2_intensity():
    from mola_lidar_odometry_amd import synth
    xyz = np.asarray(synth.workload_c2().scan_xyz, np.float32)
    p = xyz.astype(np.float64)
    i = 40.0 + 30.0 * np.sin(0.7 * p[:, 0]) * np.cos(0.3 * p[:, 1]) + 5.0 * p[:, 2]
    return xyz, i.astype(np.float32)


@pytest.mark.gpu
def test_device_normalize_c2_bit_for_bit(ctx):
    xyz, i = _c2_intensity()
    assert len(xyz) > 100000
    s = _scan(ctx, xyz, i)
    s.normalize_intensity()
    want, _ = normalize_np(i)
    assert s.download_intensity().tobytes() == want.tobytes()
    assert s.download()["xyz"].tobytes() == xyz.tobytes()


@pytest.mark.gpu
def test_device_normalize_fuzzed_sizes_and_nans(ctx):
    rng = np.random.default_rng(77)
    sizes = [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 65537]
    sizes += [int(v) for v in rng.integers(1, 300000, 6)]
    for n in sizes:
        i = (rng.normal(0, 1, n) * rng.choice([1e-3, 1.0, 1e3])).astype(np.float32)
        kind = rng.integers(4)
        if kind == 1:
            i[rng.random(n) < 0.1] = np.nan
        elif kind == 2:
            i[:] = np.float32(rng.normal())  # all equal
        elif kind == 3:
            i[rng.integers(n)] = -0.0
        s = _scan(ctx, np.zeros((n, 3), np.float32), i)
        rem = np.array([np.nan, np.nan], np.float32) if n % 2 else None
        s.normalize_intensity(rem)
        want, wr = normalize_np(i, None if rem is None else np.array([np.nan, np.nan], np.float32))
        assert s.download_intensity().tobytes() == want.tobytes(), n
        if rem is not None:
            assert rem.tobytes() == wr.tobytes(), n
    # all NaN: nothing changes, the remembered "none" stays
    i = np.full(300, np.nan, np.float32)
    s = _scan(ctx, np.zeros((300, 3), np.float32), i)
    rem = np.array([np.nan, np.nan], np.float32)
    s.normalize_intensity(rem)
    assert s.download_intensity().tobytes() == i.tobytes() and np.isnan(rem).all()
    # empty layer with intensity: a no-op that keeps the remembered range
    e = _scan(ctx, np.zeros((0, 3), np.float32), np.zeros(0, np.float32))
    rem = np.array([1.0, 2.0], np.float32)
    e.normalize_intensity(rem)
    assert rem.tolist() == [1.0, 2.0]


@pytest.mark.gpu
def test_device_normalize_sequence_carries_the_range(ctx):
    from mola_lidar_odometry_amd import synth
    d = synth.make_drive(5)
    inten = synth.drive_intensities(d)
    rem_dev = np.array([np.nan, np.nan], np.float32)
    rem_np = np.array([np.nan, np.nan], np.float32)
    for k in range(5):
        xyz, _ = d["scans"][k]
        s = _scan(ctx, xyz, inten[k])
        s.normalize_intensity(rem_dev)
        want, rem_np = normalize_np(inten[k], rem_np)
        assert s.download_intensity().tobytes() == want.tobytes(), k
        assert rem_dev.tobytes() == rem_np.tobytes(), k
    assert rem_dev.tolist() == [min(a.min() for a in inten), max(a.max() for a in inten)]


def _check_split(outs, xyz, i, t=None, src=None, low=0.1, high=0.9):
    ref = by_intensity_np(xyz, i, t, src, low, high)
    for k, (o, r) in enumerate(zip(outs, ref)):
        if o is None:
            continue
        d = o.download()
        assert d["src_idx"].tobytes() == r["src_idx"].tobytes(), k
        assert d["xyz"].tobytes() == r["xyz"].tobytes(), k
        assert o.download_intensity().tobytes() == r["i"].tobytes(), k
        if t is not None:
            assert d["t"].tobytes() == r["t"].tobytes(), k


@pytest.mark.gpu
@pytest.mark.parametrize("which", [w for w in itertools.product([True, False], repeat=3) if any(w)])
def test_device_by_intensity_null_output_combinations(ctx, which):
    rng = np.random.default_rng(sum(1 << q for q, w in enumerate(which) if w))
    n = 5003
    xyz = rng.normal(0, 10, (n, 3)).astype(np.float32)
    i = rng.uniform(-0.1, 1.1, n).astype(np.float32)
    i[rng.random(n) < 0.03] = np.nan
    i[:4] = [0.1, 0.9, np.float32(0.1), np.float32(0.9)]  # on the thresholds: mid
    t = rng.uniform(-0.05, 0.05, n).astype(np.float32)
    s = _scan(ctx, xyz, i, t)
    outs = [capi.Scan(ctx) if w else None for w in which]
    s.by_intensity(capi.by_intensity_params(0.1, 0.9), *outs)
    _check_split(outs, xyz, i, t)


@pytest.mark.gpu
def test_device_by_intensity_chains_src_to_raw(ctx):
    xyz, t, i = _drive_scan()
    raw = _scan(ctx, xyz, i, t)
    om = capi.Scan(ctx)
    raw.preprocess(capi.preprocess_params(0.5, 0.0, min_points_to_filter=0), om)
    om.normalize_intensity()
    f = om.download()
    fi = om.download_intensity()
    outs = [capi.Scan(ctx) for _ in range(3)]
    om.by_intensity(capi.by_intensity_params(0.1, 0.9), *outs)
    _check_split(outs, f["xyz"], fi, f["t"], f["src_idx"])
    assert len(outs[2]) > 0


@pytest.mark.gpu
def test_device_by_intensity_packing_boundary(ctx):
    n = (1 << 21) - 1
    xyz = np.zeros((n, 3), np.float32)
    xyz[:, 0] = np.arange(n, dtype=np.float32)
    i = np.full(n, 0.95, np.float32)  # every point in ONE class: the field that fills up
    s = _scan(ctx, xyz, i)
    outs = [capi.Scan(ctx) for _ in range(3)]
    s.by_intensity(capi.by_intensity_params(), *outs)
    assert [len(o) for o in outs] == [0, 0, n]
    _check_split(outs, xyz, i)
    big = _scan(ctx, np.zeros((n + 1, 3), np.float32), np.zeros(n + 1, np.float32))
    with pytest.raises(capi.MolahipError) as e:
        big.by_intensity(capi.by_intensity_params(), capi.Scan(ctx))
    assert e.value.status == MH_ERR_INVALID_ARGUMENT


@pytest.mark.gpu
def test_device_argument_errors_leave_outputs_alone(ctx):
    rng = np.random.default_rng(9)
    xyz = rng.normal(0, 5, (500, 3)).astype(np.float32)
    i = rng.uniform(0, 1, 500).astype(np.float32)
    s = _scan(ctx, xyz, i)
    no_i = _scan(ctx, xyz)
    o1, o2 = _scan(ctx, xyz[:7], i[:7]), _scan(ctx, xyz[:9])
    before = [o.download()["xyz"].tobytes() for o in (o1, o2)]
    before_i = o1.download_intensity().tobytes()
    p = capi.by_intensity_params()
    foreign = capi.Scan(capi.Context(0), xyz[:5])
    L = capi.lib()
    for args in ((s, o1, s, None), (s, None, None, None), (s, o1, o1, None), (s, o1, None, o1), (s, o1, foreign, None),
                 (no_i, o1, o2, None)):
        st = L.mh_scan_by_intensity(args[0]._h, C.byref(p), *[a._h if a is not None else None for a in args[1:]])
        assert st == MH_ERR_INVALID_ARGUMENT, args
    assert L.mh_scan_by_intensity(s._h, None, o1._h, None, None) == MH_ERR_INVALID_ARGUMENT
    rng2 = np.array([3.0, 4.0], np.float32)
    assert L.mh_scan_normalize_intensity(no_i._h, rng2.ctypes.data_as(C.POINTER(C.c_float))) == MH_ERR_INVALID_ARGUMENT
    assert rng2.tolist() == [3.0, 4.0] and not _has_i(no_i)
    assert no_i.download()["xyz"].tobytes() == xyz.tobytes()
    assert [len(o1), len(o2), len(foreign)] == [7, 9, 5]
    assert [o.download()["xyz"].tobytes() for o in (o1, o2)] == before and o1.download_intensity().tobytes() == before_i
    assert not _has_i(o2)
    # and the scans work as before
    outs = [capi.Scan(ctx) for _ in range(3)]
    s.by_intensity(p, *outs)
    _check_split(outs, xyz, i)
