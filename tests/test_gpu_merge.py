"""-m gpu: mh_scan_merge_sensors through the C ABI, bit for bit against its numpy restatement (tests/merge_ref.py), two
identities against entry points the oracle already pins (mh_scan_update_aos_i, mh_scan_preprocess), and its refusals."""
import ctypes as C
import itertools

import numpy as np
import pytest

from mola_lidar_odometry_amd import capi

import merge_ref as MR

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def _rot(rpy_deg, t):
    r, p, y = np.deg2rad(rpy_deg)
    Rx = np.array([[1, 0, 0], [0, np.cos(r), -np.sin(r)], [0, np.sin(r), np.cos(r)]])
    Ry = np.array([[np.cos(p), 0, np.sin(p)], [0, 1, 0], [-np.sin(p), 0, np.cos(p)]])
    Rz = np.array([[np.cos(y), -np.sin(y), 0], [np.sin(y), np.cos(y), 0], [0, 0, 1]])
    return np.concatenate([Rz @ Ry @ Rx, np.asarray(t, float)[:, None]], 1)


POSES = [None,                                                        # identity
         np.concatenate([np.eye(3), [[1.25], [-0.5], [0.375]]], 1),   # pure translation
         _rot((3.0, -7.0, 155.0), (-0.9, 0.13, 0.41)),                # general rotations
         _rot((-1.5, 2.0, 31.0), (1.07, 0.21, 0.3))]
METHODS = [MR.TS_MIDDLE_IS_ZERO, MR.TS_NONE, MR.TS_EARLIEST_IS_ZERO]


def _sources(sizes, with_t, with_i, seed=0):
    rng = np.random.default_rng(seed + sum(sizes))
    out = []
    for k, n in enumerate(sizes):
        out.append(dict(xyz=rng.uniform(-60, 60, (n, 3)).astype(F),
                        t=(rng.uniform(-0.07, 0.04, n) - 0.01 * k).astype(F) if with_t else None,  # negative stamps too
                        i=rng.uniform(0, 255, n).astype(F) if with_i else None,
                        pose=POSES[(k + len(sizes)) % len(POSES)], method=METHODS[k % 3], offset=0.004 * k - 0.002))
    return out


def _upload(ctx, s):
    """One source as the driver uploads it: interleaved records through mh_scan_update_aos_i."""
    cols = [s["xyz"]] + [c[:, None] for c in (s["t"], s["i"]) if c is not None]
    rec = np.ascontiguousarray(np.concatenate(cols, 1), F)
    off_t = 12 if s["t"] is not None else -1
    off_i = -1 if s["i"] is None else (16 if s["t"] is not None else 12)
    scan = capi.Scan(ctx)
    scan.update_interleaved_i(rec.reshape(len(s["xyz"]), rec.shape[1]), off_t=off_t, off_i=off_i)
    return scan


def _merge(ctx, srcs, out=None):
    scans = [_upload(ctx, s) for s in srcs]
    params = [capi.merge_source(s.get("pose"), s.get("method", 0), s.get("offset", 0.0)) for s in srcs]
    out = out if out is not None else capi.Scan(ctx)
    capi.scan_merge_sensors(scans, params, out)
    return out, scans


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _check(out, want, has_t, has_i):
    d = out.download()
    assert out.n == len(want["xyz"])
    np.testing.assert_array_equal(_bits(d["xyz"]), _bits(want["xyz"]))
    if has_t:
        np.testing.assert_array_equal(_bits(d["t"]), _bits(want["t"]))
    else:
        assert want["t"] is None and not d["t"].any()  # (a scan without stamps downloads zeros)
    if has_i:
        np.testing.assert_array_equal(_bits(out.download_intensity()), _bits(want["i"]))
    else:
        with pytest.raises(capi.MolahipError):
            out.download_intensity()
    assert not d["src_idx"].any()  # no src_idx channel


SIZES = [(1,), (63, 64, 65), (255, 257, 1), (300, 17, 64, 0, 129, 256, 2, 1000), (70001, 5)]


@pytest.mark.parametrize("sizes", SIZES, ids=lambda s: "x".join(map(str, s)))
def test_merge_bit_exact_sizes(ctx, sizes):
    """Boundaries off the multiples of 64 and 256 (waves and workgroups that straddle two or three sources), an empty source in
    the middle of eight, and a source whose min / max reduction wraps its grid-stride loop (70001 > 128 x 256)."""
    srcs = _sources(sizes, True, True)
    out, _ = _merge(ctx, srcs)
    _check(out, MR.merge(srcs), True, True)


@pytest.mark.parametrize("with_t,with_i", list(itertools.product([False, True], repeat=2)))
def test_merge_bit_exact_channels(ctx, with_t, with_i):
    srcs = _sources((130, 67, 259), with_t, with_i, seed=5)
    out, _ = _merge(ctx, srcs)
    _check(out, MR.merge(srcs), with_t, with_i)
    # the same output scan again, smaller and with other channels: sized and channelled by THIS call
    srcs = _sources((9, 3), not with_t, with_i, seed=6)
    out, _ = _merge(ctx, srcs, out)
    _check(out, MR.merge(srcs), not with_t, with_i)


@pytest.mark.parametrize("methods", [(0, 0, 0), (1, 1, 1), (2, 2, 2), (2, 0, 1), (1, 2, 0)])
@pytest.mark.parametrize("pose", range(len(POSES)))
def test_merge_bit_exact_methods_and_poses(ctx, methods, pose):
    srcs = _sources((200, 321, 77), True, False, seed=17 + pose)
    for s, m in zip(srcs, methods):
        s["method"], s["pose"] = m, POSES[pose]
    srcs[1]["t"] = -np.abs(srcs[1]["t"]) - F(0.5)  # all negative
    srcs[2]["t"][::2] = 0.0
    srcs[2]["t"][1] = -0.0
    out, _ = _merge(ctx, srcs)
    _check(out, MR.merge(srcs), True, False)


def test_empty_sources_alone_give_an_empty_scan(ctx):
    srcs = _sources((0, 0), False, False)
    out, _ = _merge(ctx, srcs)
    assert out.n == 0
    # an empty source without stamps beside sources with stamps is no mix
    srcs = _sources((40, 0, 90), True, True)
    srcs[1]["t"] = srcs[1]["i"] = None
    out, _ = _merge(ctx, srcs)
    _check(out, MR.merge(srcs), True, True)


def test_identity_one_equals_the_uploaded_scan(ctx):
    """One source, identity pose, MH_TS_NONE == what mh_scan_update_aos_i makes of the same bytes (as float VALUES: the
    transform turns -0 into +0, as it does everywhere else)."""
    s = _sources((4099,), True, True, seed=3)[0]
    s["xyz"][5] = [-0.0, 0.0, -0.0]
    s.update(pose=None, method=MR.TS_NONE, offset=0.7)
    out, (scan,) = _merge(ctx, [s])
    a, b = out.download(), scan.download()
    np.testing.assert_array_equal(a["xyz"], b["xyz"])
    np.testing.assert_array_equal(_bits(a["t"]), _bits(b["t"]))
    np.testing.assert_array_equal(_bits(out.download_intensity()), _bits(scan.download_intensity()))
    assert out.n == scan.n == 4099


@pytest.mark.parametrize("method,offset", [(MR.TS_MIDDLE_IS_ZERO, 0.004), (MR.TS_EARLIEST_IS_ZERO, -0.0125)])
def test_identity_two_adjustment_commutes_with_the_filter_chain(ctx, method, offset):
    """merge(identity, M, o) then mh_scan_preprocess(MH_TS_NONE) == mh_scan_update_aos then mh_scan_preprocess(M, o): 5000 points,
    the default chain's parameters at an 80 m sensor range."""
    rng = np.random.default_rng(23)
    n = 5000
    xyz = np.stack([rng.uniform(-45, 45, n), rng.uniform(-45, 45, n), np.abs(rng.normal(0, 1.5, n))], 1).astype(F)
    t = np.sort(rng.uniform(-0.05, 0.05, n)).astype(F)
    rec = np.ascontiguousarray(np.concatenate([xyz, t[:, None]], 1))
    chain = dict(decim_map_resolution=0.44, decim_icp_resolution=1.28, min_points_to_filter=2000, range_min=2.4, range_max=96.0,
                 bbox_mode=capi.BBOX_KEEP_OUTSIDE, bbox_min=(-16.0, -16.0, 0.8), bbox_max=(16.0, 16.0, 8.0))
    plain = capi.Scan(ctx)
    plain.update_interleaved(rec, off_t=12)
    pm, pi = capi.Scan(ctx), capi.Scan(ctx)
    plain.preprocess(capi.preprocess_params(timestamp_method=method, time_offset=offset, **chain), pm, pi)
    merged = capi.Scan(ctx)
    capi.scan_merge_sensors([plain], [capi.merge_source(None, method, offset)], merged)
    mm, mi = capi.Scan(ctx), capi.Scan(ctx)
    merged.preprocess(capi.preprocess_params(timestamp_method=capi.TS_NONE, **chain), mm, mi)
    assert 0 < pi.n < pm.n < n
    for got, want in ((mm, pm), (mi, pi)):
        g, w = got.download(), want.download()
        assert got.n == want.n
        np.testing.assert_array_equal(g["src_idx"], w["src_idx"])
        np.testing.assert_array_equal(_bits(g["xyz"]), _bits(w["xyz"]))
        np.testing.assert_array_equal(_bits(g["t"]), _bits(w["t"]))


def test_refusals_leave_the_output_untouched(ctx):
    L = capi.lib()
    a, b = capi.Scan(ctx, np.ones((5, 3), F)), capi.Scan(ctx, np.ones((7, 3), F)).set_timestamps(np.zeros(7, F))
    out = capi.Scan(ctx, np.full((3, 3), 9.0, F))
    before = out.download()
    other_ctx = capi.Context(0)
    foreign = capi.Scan(other_ctx, np.ones((2, 3), F))
    one = (capi.MergeSource * 9)(*[capi.merge_source() for _ in range(9)])
    bad = (capi.MergeSource * 1)(capi.merge_source(None, 3))

    def handles(*scans):
        return (C.c_void_p * len(scans))(*[s._h if s is not None else None for s in scans])

    cases = {
        "no source": (0, handles(a), one, out._h),
        "nine sources": (9, handles(*([a] * 9)), one, out._h),
        "null sources": (1, None, one, out._h),
        "null params": (1, handles(a), None, out._h),
        "null out": (1, handles(a), one, None),
        "a null source": (2, handles(a, None), one, out._h),
        "out among the sources": (2, handles(a, out), one, out._h),
        "another context": (2, handles(a, foreign), one, out._h),
        "bad method": (1, handles(a), bad, out._h),
        "negative method": (1, handles(a), (capi.MergeSource * 1)(capi.merge_source(None, -1)), out._h),
        "mixed time stamps": (2, handles(a, b), one, out._h),
    }
    for what, (n, hs, ps, o) in cases.items():
        st = L.mh_scan_merge_sensors(n, hs, ps, o)
        assert st == 1, what  # MH_ERR_INVALID_ARGUMENT
        msg = L.mh_last_error_string().decode()
        assert msg.startswith("mh_scan_merge_sensors: ") and len(msg) > 30, (what, msg)
        after = out.download()
        assert out.n == 3 and np.array_equal(after["xyz"], before["xyz"]), what
    with_i = capi.Scan(ctx, np.ones((4, 3), F)).set_intensity(np.ones(4, F))
    with pytest.raises(capi.MolahipError, match="intensity"):
        capi.scan_merge_sensors([a, with_i], [capi.merge_source()] * 2, out)
    assert out.n == 3
    foreign.close()
    other_ctx.close()


def test_a_total_at_the_index_limit_is_refused(ctx):
    """Eight times one source of 2^28 points: 2^31 >= 2^31 - 16, refused before anything is allocated for the output."""
    import torch
    z = torch.zeros(1 << 28, dtype=torch.float32, device="cuda:0")
    big = capi.Scan.from_torch(ctx, z, z, z)
    del z
    out = capi.Scan(ctx, np.full((3, 3), 9.0, F))
    with pytest.raises(capi.MolahipError, match="2\\^31 - 16") as e:
        capi.scan_merge_sensors([big] * 8, [capi.merge_source()] * 8, out)
    assert e.value.status == 1 and out.n == 3 and np.array_equal(out.download()["xyz"], np.full((3, 3), 9.0, F))
    big.close()
    torch.cuda.empty_cache()
