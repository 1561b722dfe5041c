"""mh_scan_edges_from_range_image through the C ABI, bit for bit against the numpy restatement (tests/rimg_ref.py): point
counts, xyz as uint32 views and the pixel indices of both layers.  The kernel owns a row in segments of 256 columns (SEG) and
stages a halo of W samples on either side, so the shapes sit on those edges."""
import numpy as np
import pytest

import rimg_ref as RR

pytestmark = pytest.mark.gpu

SEG = 256  # k_rimg_classify's segment width
POSE = np.array([[0.9362934, -0.2896295, 0.1986693, 0.25],
                 [0.3129918, 0.9447025, -0.0978434, -0.10],
                 [-0.1593451, 0.1537920, 0.9751703, 1.30]])  # a non-trivial sensor pose (a rotation about all three axes)


@pytest.fixture(scope="module")
def capi():
    from mola_lidar_odometry_amd import capi as c
    return c


@pytest.fixture(scope="module")
def ctx(capi):
    return capi.Context(0)


def cam(capi, R, W=6, thr=10.0, depth=True, pose=POSE, **kw):
    rows, cols = R.shape
    a = dict(fx=0.9 * cols, fy=0.93 * cols, cx=0.5 * cols - 0.25, cy=0.5 * rows + 0.75, range_units=0.001)
    a.update(kw)
    return capi.range_image_params(rows, cols, range_is_depth=depth, sensor_pose=pose, row_window_length=W, score_threshold=thr,
                                   **a)


def expect(R, p):
    P = np.array(list(p.sensor_pose)).reshape(3, 4)
    return RR.generate(R, p.row_window_length, p.score_threshold, p.fx, p.fy, p.cx, p.cy, p.range_units, bool(p.range_is_depth), P)


def run(capi, ctx, R, p, edges=True, planes=True, mem=None, src=None):
    e = capi.Scan(ctx) if edges else None
    q = capi.Scan(ctx) if planes else None
    capi.scan_edges_from_range_image(ctx, R if src is None else src, p, e, q, capi.MEM_HOST if mem is None else mem)
    return (e.download() if e is not None else None), (q.download() if q is not None else None)


def same(got, xyz, idx):
    assert got["xyz"].shape == xyz.shape, (got["xyz"].shape, xyz.shape)
    assert np.array_equal(np.ascontiguousarray(got["xyz"]).view(np.uint32), np.ascontiguousarray(xyz).view(np.uint32))
    assert np.array_equal(got["src_idx"], idx)


def check(capi, ctx, R, p):
    ge, gp = run(capi, ctx, R, p)
    ex, px, ei, pi = expect(R, p)
    same(ge, ex, ei)
    same(gp, px, pi)
    return len(ei), len(pi)


def wavy(rows, cols, seed, zeros=0.0):
    """A smooth surface with steps and noise: both classes occur; `zeros` = share of no-return pixels."""
    rng = np.random.default_rng(seed)
    c = np.arange(cols)[None, :]
    r = np.arange(rows)[:, None]
    R = 2000 + 3 * c + 7 * r + 400 * ((c // 37 + r // 5) % 2) + rng.integers(0, 3, (rows, cols))
    R = R.astype(np.uint16)
    if zeros:
        R[rng.random((rows, cols)) < zeros] = 0
    return R


@pytest.mark.parametrize("W", [1, 6])
@pytest.mark.parametrize("extra", [0, 1, 2])
def test_none_one_and_two_scored_columns(capi, ctx, W, extra):
    R = wavy(3, 2 * W + extra, 11)
    ne, np_ = check(capi, ctx, R, cam(capi, R, W=W, thr=4.0))
    assert ne + np_ == 3 * extra


@pytest.mark.parametrize("W", [6, 64])
@pytest.mark.parametrize("rows", [1, 3])
def test_three_segments_with_zeros_on_every_segment_edge(capi, ctx, W, rows):
    thr = {6: 180.0, 64: 28500.0}[W]  # (inside the spread of |S| on this image at either window: both classes occur)
    cols = 2 * SEG + 88  # three segments, the last one partial; the halo crosses the boundaries (at W = 64: more than a wave)
    R = wavy(rows, cols, 5)
    ne, np_ = check(capi, ctx, R, cam(capi, R, W=W, thr=thr))
    assert ne > 0 and np_ > 0
    for k, c in enumerate([0, SEG - 1, SEG, 2 * SEG - 1, 2 * SEG, cols - 1]):  # one at a time: each unscores its own window
        Z = R.copy()
        Z[k % rows, c] = 0
        ze, zp = check(capi, ctx, Z, cam(capi, Z, W=W, thr=thr))
        assert ze + zp < ne + np_ or c < W or c >= cols - W
    Z = R.copy()
    Z[:, [0, SEG - 1, SEG, 2 * SEG - 1, 2 * SEG, cols - 1]] = 0
    check(capi, ctx, Z, cam(capi, Z, W=W, thr=thr))


def test_all_zero_image(capi, ctx):
    R = np.zeros((4, 300), np.uint16)
    assert check(capi, ctx, R, cam(capi, R)) == (0, 0)


@pytest.mark.parametrize("W", [6, 64])
def test_int32_extremes_of_the_score(capi, ctx, W):
    cols = 4 * W + 3
    R = np.full((2, cols), 65535, np.uint16)
    R[0, 2 * W + 1] = 1  # S = -2W * 65534 at that pixel, +65534 at its 2W neighbours
    R[1, :] = 1
    R[1, 2 * W + 1] = 65535  # S = +2W * 65534 there
    for thr in (10.0, float(2 * W * 65534), float(2 * W * 65534) - 8.0):
        check(capi, ctx, R, cam(capi, R, W=W, thr=thr))
    scored, S = RR.scores(R, W)
    assert S.min() == -2 * W * 65534 and S.max() == 2 * W * 65534


def test_score_equal_to_the_threshold_is_a_plane(capi, ctx):
    W = 2
    R = np.full((1, 9), 1000, np.uint16)
    R[0, 4] = 1008  # S = -32 at column 4, +8 at columns 2, 3, 5, 6
    ge, gp = run(capi, ctx, R, cam(capi, R, W=W, thr=32.0))
    assert len(ge["xyz"]) == 0 and list(gp["src_idx"]) == [2, 3, 4, 5, 6]
    ge, gp = run(capi, ctx, R, cam(capi, R, W=W, thr=31.0))
    assert list(ge["src_idx"]) == [4] and list(gp["src_idx"]) == [2, 3, 5, 6]
    check(capi, ctx, R, cam(capi, R, W=W, thr=8.0))


@pytest.mark.parametrize("depth", [True, False])
def test_one_output_only_and_both_range_kinds(capi, ctx, depth):
    R = wavy(7, 300, 3, zeros=0.02)
    p = cam(capi, R, depth=depth)
    ex, px, ei, pi = expect(R, p)
    assert len(ei) > 0 and len(pi) > 0
    ge, none = run(capi, ctx, R, p, planes=False)
    assert none is None
    same(ge, ex, ei)
    none, gp = run(capi, ctx, R, p, edges=False)
    assert none is None
    same(gp, px, pi)
    check(capi, ctx, R, p)
    if not depth:  # the ray length differs from the depth off the axis: the two kinds give different points
        dx = expect(R, cam(capi, R, depth=True))[0]
        assert not np.array_equal(dx, ex)


def test_host_pinned_and_device_input_and_a_second_run_give_the_same_bits(capi, ctx):
    import torch
    R = wavy(9, 2 * SEG + 5, 8, zeros=0.03)
    p = cam(capi, R, depth=False)
    ex, px, ei, pi = expect(R, p)
    for _ in range(2):
        ge, gp = run(capi, ctx, R, p)
        same(ge, ex, ei)
        same(gp, px, pi)
    t = torch.from_numpy(R.view(np.int16).copy())
    pinned = t.pin_memory()
    ge, gp = run(capi, ctx, R, p, mem=capi.MEM_HOST_PINNED, src=pinned.data_ptr())
    same(ge, ex, ei)
    same(gp, px, pi)
    dev = t.cuda()
    torch.cuda.synchronize()
    ge, gp = run(capi, ctx, R, p, mem=capi.MEM_DEVICE, src=dev.data_ptr())
    same(ge, ex, ei)
    same(gp, px, pi)


def test_randomised_image_with_a_tenth_of_zeros(capi, ctx):
    for seed in (20261, 20262):
        rng = np.random.default_rng(seed)
        R = rng.integers(500, 520, (97, 211)).astype(np.uint16)
        R[rng.random(R.shape) < 0.10] = 0
        ne, np_ = check(capi, ctx, R, cam(capi, R, W=2, thr=12.0, depth=bool(seed & 1)))
        assert ne > 100 and np_ > 100


def test_refusals_leave_the_outputs_untouched(capi, ctx):
    R = wavy(4, 40, 1)
    keep = np.array([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]], np.float32)
    e, q = capi.Scan(ctx, keep), capi.Scan(ctx, keep[:1])
    other = capi.Scan(capi.Context(0), keep)

    def refused(status, edges=e, planes=q, img=R, **kw):
        p = cam(capi, img)
        for k, v in kw.items():
            setattr(p, k, v)
        with pytest.raises(capi.MolahipError) as err:
            capi.scan_edges_from_range_image(ctx, img.ctypes.data, p, edges, planes, capi.MEM_HOST)
        assert err.value.status == status
        for s, want in ((e, keep), (q, keep[:1]), (other, keep)):
            assert np.array_equal(s.download()["xyz"], want)

    inval, unsup = 1, 6  # MH_ERR_INVALID_ARGUMENT, MH_ERR_UNSUPPORTED
    refused(inval, rows=0)
    refused(inval, cols=0)
    refused(inval, row_window_length=0)
    refused(inval, row_window_length=65)
    refused(inval, fx=0.0)
    refused(inval, fy=-1.0)
    refused(inval, range_units=0.0)
    refused(inval, score_threshold=-1.0)
    refused(inval, score_threshold=float("inf"))
    refused(inval, score_threshold=float("nan"))
    refused(inval, edges=None, planes=None)
    refused(inval, edges=other)
    refused(inval, planes=other)
    refused(unsup, rows=1 << 11, cols=1 << 10)  # 2^21 pixels: one above the limit (refused before the image is read)
    capi.scan_edges_from_range_image(ctx, R, cam(capi, R), e, q)  # and the same handles still work
    assert len(e) + len(q) > 0
