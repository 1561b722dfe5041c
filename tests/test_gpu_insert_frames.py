"""mh_map_insert_frames: a group of key-frames inserted at once gives, bit for bit, the map that mh_map_insert called for every
frame in order gives on a twin -- downloads, NDT statistics, counts and bounding box, mh_nn_search on 300 queries, and one more
mh_map_insert applied to both afterwards -- whatever the pass size and wherever the arrays live.  The loop's results are computed
once per case and shared."""
import ctypes as C
import warnings

import numpy as np
import pytest

from mola_lidar_odometry_amd import capi, synth

pytestmark = pytest.mark.gpu

F = np.float32
INVALID, OUT_OF_RANGE, WARN_PREVIOUS = 1, 4, 64
PLAIN = dict(voxel_size=1.0, max_points_per_voxel=4)
NDT = dict(voxel_size=1.0, max_points_per_voxel=20, min_distance_between_points=0.05, ndt_max_eigen_ratio=0.1)


def _pose(j):
    """a few metres apart at most: the frames share voxels"""
    k = j % 7
    return synth.pose_from_ypr([0.9 * k, -0.35 * k, 0.1 * (j % 3), 0.07 * k, 0.01 * k, -0.02])


def _cloud(n, seed):
    return np.random.default_rng(seed).uniform(-3.0, 3.0, (n, 3)).astype(F)


def _frames_sizes(sizes, seed):
    return [(_cloud(n, seed + j), _pose(j)) for j, n in enumerate(sizes)]


def _frames_jitter():
    """consecutive frames: the same cloud plus 1 cm of jitter under nearly the same pose -- most points of a later frame lie
    within min_distance_between_points of one an earlier frame stored"""
    rng = np.random.default_rng(11)
    base = rng.uniform(-3.0, 3.0, (700, 3))
    return [((base + rng.normal(0.0, 0.01, base.shape)).astype(F), synth.pose_from_ypr([0.002 * j, 0.001 * j, 0, 0.0005 * j, 0, 0]))
            for j in range(6)]


CASES = {
    # waves that straddle frames (prefix 0, 0, 1, 64, 128, 193), an empty frame, the cap of 4 biting across frames
    "straddle": (PLAIN, lambda: _frames_sizes([0, 1, 63, 64, 65, 1500], 100)),
    # one wave over five frames (points 1664..1727 of the pass), empty frames in the middle and at the end
    "straddle_many": (PLAIN, lambda: _frames_sizes([1500, 0, 65, 64, 63, 1, 0, 7, 3, 200, 0], 200)),
    # a prefix table longer than a workgroup
    "single_points": (PLAIN, lambda: _frames_sizes([1] * 300, 300)),
    # clearance decisions across frames, NDT statistics
    "ndt_jitter": (NDT, _frames_jitter),
}
EXTRA = (_cloud(900, 999), _pose(2))  # the one more insertion applied to both afterwards
QUERIES = np.random.default_rng(5).uniform(-3.5, 6.0, (300, 3)).astype(F)
Q_POSE = synth.pose_from_ypr([0.3, -0.2, 0.05, 0.1, 0.0, 0.0])


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def _new_map(ctx, params, start):
    m = capi.Map(ctx, **params)
    if start == "built":
        m.build(_cloud(5000, 1))
    return m


def _info_tuple(i, with_status=True):
    return (i.n_points, i.n_offered, i.n_voxels, i.n_planes, tuple(F(v).tobytes() for v in i.bbox_min),
            tuple(F(v).tobytes() for v in i.bbox_max)) + ((i.deferred_status,) if with_status else ())


def _state(ctx, m, with_status=True):
    """everything the definition names, as bytes"""
    d, n = m.download(), m.download_ndt()
    q = capi.Scan(ctx, QUERIES)
    nn = capi.nn_search(m, q, Q_POSE, 1.0)
    q.close()
    assert len(nn["global_idx"]) > 20   # (the comparison is not vacuous)
    out = {k: (v.dtype, v.shape, v.tobytes()) for k, v in d.items()}
    out.update({"ndt_" + k: v.tobytes() for k, v in n.items()})
    out.update({"nn_" + k: nn[k].tobytes() for k in ("local_idx", "global_idx", "global_xyz", "d2")})
    out["info"] = _info_tuple(m.info(), with_status)
    return out


def _insert_loop(ctx, m, frames):
    for xyz, T in frames:
        sc = capi.Scan(ctx, xyz)
        m.insert(sc, T, 0.0)
        sc.close()


def _states_with_extra(ctx, m, with_status=True):
    a = _state(ctx, m, with_status)
    _insert_loop(ctx, m, [EXTRA])
    return a, _state(ctx, m, with_status)


@pytest.fixture(scope="module")
def reference(ctx):
    """(case, start) -> the loop's (state, state after one more insertion), computed once"""
    done = {}

    def get(case, start):
        if (case, start) not in done:
            params, make = CASES[case]
            m = _new_map(ctx, params, start)
            _insert_loop(ctx, m, make())
            done[case, start] = _states_with_extra(ctx, m)
            m.close()
        return done[case, start]
    return get


def _assert_same(got, want):
    assert got.keys() == want.keys()
    for k in want:
        assert got[k] == want[k], k


@pytest.mark.parametrize("pass_points", [0, 100, 1])
@pytest.mark.parametrize("start", ["empty", "built"])
@pytest.mark.parametrize("case", list(CASES))
def test_batched_equals_the_loop(ctx, reference, case, start, pass_points):
    params, make = CASES[case]
    frames = make()
    want, want_after = reference(case, start)
    m = _new_map(ctx, params, start)
    n0 = m.info().n_offered
    m.insert_frames(frames, pass_points)
    got, got_after = _states_with_extra(ctx, m)
    _assert_same(got, want)
    _assert_same(got_after, want_after)
    # what the case is there for
    n_new = sum(len(x) for x, _ in frames)
    assert got["info"][1] == n0 + n_new
    assert case == "single_points" or got["info"][0] < n0 + n_new   # cap / clearance dropped something
    src = np.frombuffer(got["src_idx"][2], np.uint32)
    assert src.max() >= n0 and (start == "empty" or src.min() < n0)
    if case == "ndt_jitter" and start == "empty":
        assert got["info"][3] > 0   # (the NDT download compares statistics of voxels that are planes, too)
        # the later frames were decided against the earlier ones: far fewer points stored than a frame per frame would give
        per_frame = [((src >= n0 + 700 * j) & (src < n0 + 700 * (j + 1))).sum() for j in range(6)]
        assert per_frame[0] > 300 and sum(per_frame[1:]) < per_frame[0]
    m.close()


@pytest.mark.parametrize("start", ["empty", "built"])
def test_device_resident_input(ctx, reference, start):
    import torch
    params, make = CASES["straddle_many"]
    frames = make()
    want, want_after = reference("straddle_many", start)
    keep, dev = [], []
    for xyz, T in frames:
        t = [torch.from_numpy(np.ascontiguousarray(xyz[:, a])).to("cuda:0") for a in range(3)]
        keep.append(t)
        dev.append((t[0].data_ptr() if len(xyz) else None, t[1].data_ptr() if len(xyz) else None,
                    t[2].data_ptr() if len(xyz) else None, len(xyz), T))
    torch.cuda.synchronize()
    for pass_points in (0, 100):
        m = _new_map(ctx, params, start)
        m.insert_frames_device(dev, pass_points)
        got, got_after = _states_with_extra(ctx, m)
        _assert_same(got, want)
        _assert_same(got_after, want_after)
        m.close()


@pytest.mark.parametrize("pass_points", [0, 1])
def test_out_of_range_point_is_one_deferred_verdict(ctx, pass_points):
    frames = _frames_sizes([40, 50, 60], 400)
    frames[1][0][17] = (3.0e6, 0.5, 0.5)   # voxel 1.0: beyond the key range
    a, b = capi.Map(ctx, **PLAIN), capi.Map(ctx, **PLAIN)
    with warnings.catch_warnings(record=True) as w:   # the loop reports it from its third insertion
        warnings.simplefilter("always")
        _insert_loop(ctx, a, frames)
    assert len(w) == 1 and a.info().deferred_status == 0
    b.insert_frames(frames, pass_points)
    ib = b.info()
    assert ib.deferred_status == OUT_OF_RANGE
    _assert_same(_state(ctx, b, with_status=False), _state(ctx, a, with_status=False))   # left out on both routes
    assert ib.n_offered == 150 and (b.download()["src_idx"] != 40 + 17).all()
    assert b.info().deferred_status == OUT_OF_RANGE   # (accessors do not take the verdict)
    # the next insertion returns the warning and inserts
    sc = capi.Scan(ctx, EXTRA[0])
    T = capi._T12(EXTRA[1])
    assert capi.lib().mh_map_insert(b._h, sc._h, T.ctypes.data_as(capi._DP), 0.0) == WARN_PREVIOUS
    a.insert(sc, EXTRA[1], 0.0)
    assert b.info().deferred_status == 0 and b.info().n_offered == 150 + 900
    _assert_same(_state(ctx, b), _state(ctx, a))
    # ... and so does a following mh_map_insert_frames when the verdict is a batched call's
    b.insert_frames(frames, pass_points)
    with pytest.warns(RuntimeWarning):
        b.insert_frames([EXTRA], pass_points)
    assert b.info().deferred_status == 0 and b.info().n_offered == 150 + 900 + 150 + 900
    for h in (a, b, sc):
        h.close()


def _raw(m, entries, n_frames=None, mem=capi.MEM_HOST, keep=None):
    """entries: (x, y, z, n, T) with arrays, integers (addresses) or None"""
    arr = (capi.MapFrame * max(len(entries), 1))()
    for e, (x, y, z, n, T) in zip(arr, entries):
        for name, v in (("x", x), ("y", y), ("z", z)):
            setattr(e, name, v.ctypes.data_as(C.c_void_p) if isinstance(v, np.ndarray) else v)
        e.n = n
        e.T[:] = list(T)
    return capi.lib().mh_map_insert_frames(m._h if m is not None else None, arr if entries or keep else None,
                                           len(entries) if n_frames is None else n_frames, mem, 0)


def test_refusals_leave_the_map_untouched(ctx):
    m = capi.Map(ctx, **PLAIN).build(_cloud(2000, 3))
    before = _state(ctx, m)
    x, y, z = (np.ascontiguousarray(_cloud(10, 4)[:, a]) for a in range(3))
    T = list(capi._T12(_pose(1)))
    ok = (x, y, z, 10, T)

    def bad_pose(v, at):
        t = list(T)
        t[at] = v
        return t

    refused = [
        lambda: _raw(None, [ok]),                                        # a NULL map
        lambda: capi.lib().mh_map_insert_frames(m._h, None, 1, capi.MEM_HOST, 0),   # NULL frames with n_frames > 0
        lambda: _raw(m, [ok], mem=7),                                    # a bad mem
        lambda: _raw(m, [ok], mem=-1),
        lambda: _raw(m, [ok, (x, None, z, 10, T)]),                      # NULL arrays with n > 0
        lambda: _raw(m, [(None, None, None, 1, T)]),
        lambda: _raw(m, [ok, (x, y, z, 10, bad_pose(np.nan, 3))]),       # a non-finite pose entry
        lambda: _raw(m, [(x, y, z, 10, bad_pose(np.inf, 0)), ok]),
        lambda: _raw(m, [ok, (None, None, None, 0, bad_pose(-np.inf, 11))]),   # ... of an empty frame too
        lambda: _raw(m, [ok], n_frames=capi.MAX_INSERT_FRAMES + 1),      # too many frames (refused before any is read)
        lambda: _raw(m, [(x, y, z, 0x7FFFFFF0, T)]),                     # too many points in one frame (never read)
        lambda: _raw(m, [(x, y, z, 0x40000000, T), (x, y, z, 0x40000000, T)]),   # ... and summed over the call
    ]
    for k, call in enumerate(refused):
        assert call() == INVALID, k
        _assert_same(_state(ctx, m), before)
    # n_offered + offered points beyond what 32-bit source indices can number
    d = m.download()
    r = capi.Map(ctx, **PLAIN).restore(d["xyz"], d["src_idx"], 0xFFFFFFE0)
    r_before = _state(ctx, r)
    x16 = np.zeros(16, F)
    assert _raw(r, [(x16, x16, x16, 10, T), (x16, x16, x16, 6, T)]) == INVALID
    _assert_same(_state(ctx, r), r_before)
    # nothing to do: MH_OK and nothing changes
    assert _raw(m, [], keep=True) == 0 and capi.lib().mh_map_insert_frames(m._h, None, 0, capi.MEM_HOST, 0) == 0
    assert _raw(m, [(None, None, None, 0, T), (x, y, z, 0, T)]) == 0
    _assert_same(_state(ctx, m), before)
    # the refused handle is usable
    assert _raw(m, [ok]) == 0 and m.info().n_offered == 2010
    m.close()
    r.close()


def test_out_of_memory_in_a_later_pass_keeps_the_earlier_passes():
    """The buffers are grow-only: after a warm-up with 200-point frames (twice: the first build and the merge path) and a clear, a
    first pass of 120 points allocates nothing and a second pass of 5000 points has to grow its staging first -- the injected
    failure (first attempt and retry) hits there, before the stored content is touched."""
    ctx = capi.Context(0)   # (a context of its own: nobody else has grown its staging)
    try:
        m = capi.Map(ctx, **PLAIN)
        for seed in (1, 2):
            m.insert_frames([(_cloud(200, seed), _pose(seed))])
        m.build(np.zeros((0, 3), F))
        small, big = (_cloud(120, 7), _pose(1)), (_cloud(5000, 8), _pose(2))
        capi.fail_allocations(1, 1)
        try:
            with pytest.raises(capi.MolahipError) as e:
                m.insert_frames([small, big], 150)   # two passes: 120 points, then the frame that is larger than the budget
        finally:
            capi.fail_allocations(0, 0)
        assert e.value.status == 3   # MH_ERR_OUT_OF_MEMORY
        twin = capi.Map(ctx, **PLAIN)
        _insert_loop(ctx, twin, [small])
        i = m.info()
        assert (i.n_offered, i.n_points) == (120, twin.info().n_points) and i.n_points > 0   # the first pass stays, n_offered says how far
        _assert_same(_state(ctx, m), _state(ctx, twin))
        m.insert_frames([big], 150)              # the handle is usable: the rest goes in, and the map is the loop's
        _insert_loop(ctx, twin, [big])
        _assert_same(_state(ctx, m), _state(ctx, twin))
    finally:
        ctx.close()
