"""include/molahip_occgrid.h on the device.  mh_occmap_insert_frames is held to its definition -- bit for bit the loop of
mh_occmap_insert -- twice: against that loop on a twin handle of the library, and against tests/occmap_ref.OccMapRef fed the same
loop.  Compared: the download (keys and log-odds), n_cells / n_occupied, the search map's content and V, the info totals.  The index
bounds, the projection and the host path (key-frames to grid to files, through pybind and the CLI) are held to tests/occgrid_ref.py.

The room (test_the_host_path_reads_the_room...): the restatement alone leaves 548 of 29 505 interior cells unknown (the shadow of the
box) and 10 of 704 wall sites without an occupied cell (tests/test_occgrid_cpu.py computes both); the bounds are twice these shares:
1 096 cells and 20 sites."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from mola_lidar_odometry_amd import capi
from mola_lidar_odometry_amd import capi_occgrid as og

import occgrid_cases as oc
import occgrid_ref as G
import occmap_ref as R

pytestmark = pytest.mark.gpu

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "mola_lidar_odometry_amd", "molahip-lo-cli")


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def insert_single(ctx, occ, xyz, T):
    if len(xyz) == 0:      # (an insert of no points changes no cell)
        return 0, 0
    s = capi.Scan(ctx, np.asarray(xyz, F).reshape(-1, 3))
    occ.insert(s, T, 0.0)
    s.close()
    i = occ.info()
    return int(i.n_left_out), int(i.n_keys)


def same(a, b, ref):
    """the batched map against the twin and against the restatement: cells, log-odds, counts, the search map and its voxel"""
    ka, la = a.download()
    kb, lb = b.download()
    kr, lr = ref.download()
    assert ka.shape == kb.shape == kr.shape and np.array_equal(ka, kb) and np.array_equal(ka, kr)
    assert np.array_equal(la, lb) and np.array_equal(la, lr)
    ia, ib = a.info(), b.info()
    cen = ref.centres()
    assert ia.n_cells == ib.n_cells == len(kr) and ia.n_occupied == ib.n_occupied == len(cen)
    assert ia.search_voxel_size == ib.search_voxel_size
    da, db = a.search_map(0.0).download(), b.search_map(0.0).download()
    for k in ("xyz", "src_idx", "vox_keys", "vox_first", "vox_count"):       # the same centres in the same order, the same voxels
        assert da[k].shape == db[k].shape and np.array_equal(da[k].view(np.uint32) if da[k].dtype == F else da[k],
                                                             db[k].view(np.uint32) if db[k].dtype == F else db[k]), k
    order = np.argsort(da["src_idx"], kind="stable")
    assert np.array_equal(da["src_idx"][order], np.arange(len(cen), dtype=np.uint32))
    assert np.array_equal(bits(da["xyz"][order]), bits(cen))


def run(ctx, frames, pre=(), post=(), max_points_per_pass=0, batched_keys_per_pass=0, insert=None, **kw):
    """pre: single inserts before the call, on all three; frames: ONE batched call on `a`, the loop on the twin and the restatement;
    post: single inserts after.  batched_keys_per_pass: the chunk size of the batched map alone (the twin keeps the default)."""
    kw.setdefault("resolution", oc.RES)
    a = capi.OccMap(ctx, max_keys_per_pass=batched_keys_per_pass, **kw)
    b = capi.OccMap(ctx, **kw)
    ref = R.OccMapRef(**kw)
    for xyz, T in pre:
        for m in (a, b):
            insert_single(ctx, m, xyz, T)
        ref.insert(xyz, T)
    (insert or og.insert_frames)(a, frames, max_points_per_pass)
    left = keys = rleft = rkeys = 0
    for xyz, T in frames:
        l, k = insert_single(ctx, b, xyz, T)
        left, keys = left + l, keys + k
        if len(xyz):
            ref.insert(xyz, T)
            rleft, rkeys = rleft + ref.n_left_out, rkeys + ref.n_keys
    same(a, b, ref)
    ia = a.info()
    if sum(len(x) for x, _ in frames):                       # the call's totals
        assert (ia.n_left_out, ia.n_keys) == (left, keys) == (rleft, rkeys)
        if max_points_per_pass == 0:                         # one pass: its keys in chunks
            per = batched_keys_per_pass or (1 << 24)
            assert ia.n_passes == -(-keys // per)
    for xyz, T in post:
        for m in (a, b):
            insert_single(ctx, m, xyz, T)
        ref.insert(xyz, T)
    if post:
        same(a, b, ref)
    return a, b, ref


# ---- the batched insertion ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_frames", [0, 1, 2, 3, 17])
def test_frame_counts(ctx, n_frames):
    a, _, _ = run(ctx, oc.random_frames([65] * n_frames, seed=n_frames))
    assert (a.info().n_cells > 0) == (n_frames > 0)


@pytest.mark.parametrize("rule", [capi.OCC_COUNTED, capi.OCC_ONCE])
def test_frame_sizes_with_empty_frames_between_full_ones(ctx, rule):
    sizes = [0, 1, 63, 0, 64, 65, 0, 0, 257, 2000, 0]
    run(ctx, oc.random_frames(sizes, seed=3, reach=1.0), update_rule=rule)


def test_only_empty_frames_change_nothing(ctx):
    a, b, ref = run(ctx, oc.random_frames([0, 0, 0], seed=1), pre=oc.random_frames([65], seed=2))
    before = a.info()
    og.insert_frames(a, [])
    og.insert_frames(a, oc.random_frames([0], seed=1))
    after = a.info()
    assert (before.n_cells, before.n_keys, before.n_passes, before.n_left_out) == (after.n_cells, after.n_keys, after.n_passes, after.n_left_out)
    same(a, b, ref)


@pytest.mark.parametrize("rule", [capi.OCC_COUNTED, capi.OCC_ONCE])
def test_ray_shapes(ctx, rule):
    """M = 0, 1, 2 and about 300 cells; axis-aligned and diagonal; points exactly on cell faces; three poses"""
    frames = oc.ray_shapes()
    a, _, ref = run(ctx, frames, update_rule=rule)
    assert max(np.abs(k).max() for k in [a.download()[0]]) >= 299
    assert ref.cells[(0, 0, 0)] > 0                        # the M = 0 points hit the origin cell itself


@pytest.mark.parametrize("rule,name", [(capi.OCC_COUNTED, "counted"), (capi.OCC_ONCE, "once")])
def test_the_clamp_case_is_folded_in_frame_order(ctx, rule, name):
    """six hits to l_max, eight looks through to l_min, one hit: -33; the summed counts would give -47 (counted) or 14 (once)"""
    for budget, per in [(0, 0), (4, 0), (0, 64), (1, 64)]:
        a, _, ref = run(ctx, oc.clamp_frames(), update_rule=rule, max_points_per_pass=budget, batched_keys_per_pass=per)
        keys, lo = a.download()
        wall = int(lo[(keys == np.array(oc.WALL)).all(axis=1)][0])
        assert wall == ref.cells[oc.WALL] == oc.WALL_IN_ORDER != oc.WALL_SUMMED[name]


def test_the_once_rule_s_own_order_case(ctx):
    for per in (0, 64):
        a, _, ref = run(ctx, oc.clamp_frames_once_own(), update_rule=capi.OCC_ONCE, batched_keys_per_pass=per)
        keys, lo = a.download()
        assert int(lo[(keys == np.array(oc.WALL)).all(axis=1)][0]) == ref.cells[oc.WALL] == 14


@pytest.mark.parametrize("kw", [dict(ray_trace_free_space=False), dict(decimation=3), dict(decimation=3, update_rule=capi.OCC_ONCE),
                                dict(max_range=1.2), dict(max_range=1.2, decimation=3, ray_trace_free_space=False),
                                dict(resolution=0.25, prob_hit=0.9, prob_miss=0.4, clamp_min=0.12, clamp_max=0.97, occupied_threshold=0.5)])
def test_the_insert_options(ctx, kw):
    frames = oc.random_frames([257, 0, 64, 65, 1, 130], seed=7)
    a, _, ref = run(ctx, frames, **kw)
    if kw.get("max_range"):                                                   # the range cuts some points, not all
        n_all = sum(len(x[::kw.get("decimation", 1)]) for x, _ in frames)
        assert 0 < int((np.array(list(ref.cells.values())) > 0).sum()) < n_all


def test_wild_points_are_left_out_and_counted(ctx):
    a, _, _ = run(ctx, oc.wild_frames())
    assert a.info().n_left_out == 6                                           # two per frame leave the key range; the non-finite ones are not counted


def test_a_map_that_already_holds_cells_and_a_single_insert_after_the_call(ctx):
    pre, frames, post = oc.random_frames([130, 65], seed=21), oc.random_frames([64, 0, 257, 65], seed=22), oc.random_frames([130], seed=23)
    a, b, ref = run(ctx, frames, pre=pre, post=post)
    og.insert_frames(a, frames[::-1])                                         # ... and a second batched call after that
    for xyz, T in frames[::-1]:
        insert_single(ctx, b, xyz, T)
        if len(xyz):
            ref.insert(xyz, T)
    same(a, b, ref)


@pytest.mark.parametrize("budget,per", [(100, 0), (0, 64), (0, 1000), (100, 64), (100, 1000), (1, 0)])
def test_pass_sizes_do_not_change_a_bit(ctx, budget, per):
    frames = oc.random_frames([65, 0, 33, 257, 64, 1, 99], seed=31) + oc.clamp_frames()[:8]
    a, _, _ = run(ctx, frames, pre=oc.random_frames([65], seed=32), max_points_per_pass=budget, batched_keys_per_pass=per)
    d, _, _ = run(ctx, frames, pre=oc.random_frames([65], seed=32))           # the library's sizes
    for x, y in zip(a.download(), d.download()):
        assert np.array_equal(x, y)
    if budget == 100 and per == 0:
        assert a.info().n_passes == 5                                          # [65 0 33] [257] [64 1] [99 1] [1 x 7]: one chunk each
    assert a.info().n_keys == d.info().n_keys


def test_pinned_and_device_arrays_give_the_same_bits(ctx):
    import torch
    frames = oc.random_frames([65, 0, 257, 64], seed=41)

    def from_tensors(mem, to):
        def insert(occ, frames, budget):
            keep = [[to(torch.from_numpy(np.ascontiguousarray(x[:, k]))) for k in range(3)] for x, _ in frames]
            torch.cuda.synchronize()
            rows = [(t[0].data_ptr() if len(x) else None, t[1].data_ptr() if len(x) else None, t[2].data_ptr() if len(x) else None, len(x), T)
                    for t, (x, T) in zip(keep, frames)]
            og.insert_frames_ptr(occ, rows, mem, budget)
        return insert

    for budget in (0, 100):
        run(ctx, frames, insert=from_tensors(capi.MEM_DEVICE, lambda t: t.cuda()), max_points_per_pass=budget)
        run(ctx, frames, insert=from_tensors(capi.MEM_HOST_PINNED, lambda t: t.pin_memory()), max_points_per_pass=budget)


def test_refusals_come_before_any_device_work_and_leave_the_map_alone(ctx):
    a, b, ref = run(ctx, oc.random_frames([65, 64], seed=51))
    L = og.lib()
    good = oc.random_frames([5, 0], seed=52)
    before = a.info()

    def refused(frames=good, n=None, mem=capi.MEM_HOST, handle=None, edit=None, null_frames=False):
        keep, arr = og.frame_table(frames)
        if edit:
            edit(arr)
        st = L.mh_occmap_insert_frames(a._h if handle is None else handle, None if null_frames else arr, len(frames) if n is None else n, mem, 0)
        assert st == 1, L.mh_last_error_string()

    refused(handle=C.c_void_p(None))
    refused(null_frames=True)
    refused(mem=7)
    refused(mem=-1)
    refused(edit=lambda arr: setattr(arr[0], "x", None))
    refused(edit=lambda arr: setattr(arr[0], "z", None))
    for bad in (np.nan, np.inf, -np.inf):
        refused(edit=lambda arr: arr[0].T.__setitem__(5, bad))
        refused(edit=lambda arr: arr[1].T.__setitem__(11, bad))               # the pose of an EMPTY frame too
    refused(edit=lambda arr: arr[0].T.__setitem__(3, 6.0e4))                  # a pose outside the key range (1.2e6 cells)
    refused(n=og.MAX_INSERT_FRAMES + 1)
    st = L.mh_occmap_insert_frames(a._h, None, 0, capi.MEM_HOST, 0)          # no frames at all is fine
    assert st == 0
    after = a.info()
    assert (before.n_cells, before.n_occupied, before.n_keys, before.n_passes) == (after.n_cells, after.n_occupied, after.n_keys, after.n_passes)
    same(a, b, ref)
    # the projection's and the bounds' refusals
    out = (C.c_int32 * 16)()
    for w in [og.GridWindow(0, 0, 0, 4, 0, 0), og.GridWindow(0, 0, 4, 0, 0, 0), og.GridWindow(0, 0, 1 << 14, (1 << 14) + 1, 0, 0),
              og.GridWindow(0, 0, 4, 4, 1, 0)]:
        assert L.mh_occmap_project_grid(a._h, C.byref(w), out) == 1
    assert L.mh_occmap_project_grid(a._h, None, out) == 1 and L.mh_occmap_project_grid(a._h, C.byref(og.GridWindow(0, 0, 4, 4, 0, 0)), None) == 1
    three, n = (C.c_int32 * 3)(), C.c_uint64(0)
    assert L.mh_occmap_index_bounds(a._h, None, three, C.byref(n)) == 1 and L.mh_occmap_index_bounds(a._h, three, three, None) == 1
    same(a, b, ref)


# ---- bounds and projection ---------------------------------------------------------------------------------------------------------
def cells_map(ctx, points, **kw):
    """a map (ray tracing off) whose stored cells are the cells of `points`, one insert per entry of the list"""
    occ = capi.OccMap(ctx, resolution=oc.RES, ray_trace_free_space=False, **kw)
    ref = R.OccMapRef(resolution=oc.RES, ray_trace_free_space=False, **kw)
    for xyz in points:
        insert_single(ctx, occ, xyz, oc.I12)
        ref.insert(xyz, oc.I12)
    return occ, ref


def centre(ix, iy, iz):
    return [(ix + 0.5) * oc.RES, (iy + 0.5) * oc.RES, (iz + 0.5) * oc.RES]


def projected(occ, ref, x0, y0, nx, ny, z_lo, z_hi):
    got = og.project_grid(occ, x0, y0, nx, ny, z_lo, z_hi)
    want = G.project(*ref.download(), x0, y0, nx, ny, z_lo, z_hi)
    assert got.shape == want.shape == (ny, nx) and np.array_equal(got, want)
    return got


def test_bounds_and_projection_of_an_empty_map_and_of_one_cell(ctx):
    occ, ref = cells_map(ctx, [])
    assert og.index_bounds(occ) == (None, None, 0)                            # lo / hi untouched (the binding asserts it)
    assert (projected(occ, ref, -3, -3, 7, 5, -10, 10) == G.NONE).all()
    occ, ref = cells_map(ctx, [np.array([centre(-7, 3, 2)], F)])
    lo, hi, n = og.index_bounds(occ)
    assert n == 1 and lo.tolist() == hi.tolist() == [-7, 3, 2]
    g = projected(occ, ref, -8, 2, 3, 4, 2, 2)
    assert g[1, 1] == 14 and (g == G.NONE).sum() == 11
    assert (projected(occ, ref, -8, 2, 3, 4, 3, 9) == G.NONE).all()           # a band that excludes everything
    assert (projected(occ, ref, -8, 2, 3, 4, -9, 1) == G.NONE).all()
    assert projected(occ, ref, -7, 3, 1, 1, -5, 5)[0, 0] == 14                # a window of one cell


def test_a_window_that_cuts_the_map_on_each_side_and_negative_indices(ctx):
    rng = np.random.default_rng(61)
    idx = rng.integers(-40, 41, (3000, 3))
    idx[:, 2] = rng.integers(-3, 4, 3000)
    pts = [np.array([centre(*k) for k in idx[:1500]], F), np.array([centre(*k) for k in idx[1000:]], F)]   # some cells hit twice
    occ, ref = cells_map(ctx, pts)
    lo, hi, n = og.index_bounds(occ)
    b = G.index_bounds(ref.download()[0])
    assert n == len(ref.cells) and lo.tolist() == b[0].tolist() and hi.tolist() == b[1].tolist() and lo[0] < 0 < hi[0]
    projected(occ, ref, *G.window(lo, hi, 2), -3, 3)                          # everything, with a margin
    for x0, y0, nx, ny in [(-10, -50, 20, 100), (-50, -10, 100, 20), (-45, -45, 30, 30), (15, 15, 30, 30), (0, 0, 1, 1), (-300, -300, 7, 7)]:
        projected(occ, ref, x0, y0, nx, ny, -1, 1)
    g = projected(occ, ref, -41, -41, 83, 83, -100, 100)
    assert (g != G.NONE).sum() == len({(k[0], k[1]) for k in ref.cells})


def test_the_maximum_of_a_column_wins(ctx):
    """two cells in one column, one free and one occupied"""
    occ = capi.OccMap(ctx, resolution=oc.RES)
    ref = R.OccMapRef(resolution=oc.RES)
    hit = np.array([centre(10, 0, 0)], F)
    for xyz, T in [(hit, oc.I12), (np.array([centre(20, 0, 0)], F), oc.pose(0, 0, 2 * oc.RES))]:   # seen from two cells up: the ray passes (10, 0, 2)
        insert_single(ctx, occ, xyz, T)
        ref.insert(xyz, T)
    assert ref.cells[(10, 0, 0)] == 14 and ref.cells[(10, 0, 2)] == -14
    g = projected(occ, ref, 0, -1, 25, 3, 0, 2)
    assert g[1, 10] == 14 and g[1, 11] == -14 and g[1, 20] == 14
    assert projected(occ, ref, 0, -1, 25, 3, 1, 2)[1, 10] == -14              # the band without the occupied cell
    assert G.classify(g, 7)[0][1, 10] == G.OCCUPIED


# ---- the host path -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def room():
    frames, kfset = G.room_session()
    return frames, kfset, G.build(frames)


def test_the_voxel_map_s_three_methods(room):
    from mola_lidar_odometry_amd import _mp2p_icp_hip as H
    frames = room[0][:3]
    m = H.CVoxelMap(oc.RES)
    assert m.indexBounds() is None
    m.insertPointCloudFrames([(xyz, T.tolist()) for xyz, T in frames])
    ref = R.OccMapRef(resolution=oc.RES)
    for xyz, T in frames:
        ref.insert(xyz, T)
    keys, lo = m.download()
    assert np.array_equal(keys, ref.download()[0]) and np.array_equal(lo, ref.download()[1])
    assert m.size() == len(ref.centres()) and m.voxelCount() == len(ref.cells)
    b = G.index_bounds(keys)
    assert m.indexBounds() == (tuple(b[0].tolist()), tuple(b[1].tolist()))
    w = G.window(b[0], b[1], 1)
    assert np.array_equal(m.projectGrid(*w, 0, 0), G.project(keys, lo, *w, 0, 0))
    with pytest.raises(RuntimeError, match="no batched insertion"):           # the point-layer insertion stays refused
        m.insertFrames([(xyz, T.tolist()) for xyz, T in frames])


def test_the_host_path_reads_the_room_as_the_restatement_does(room, tmp_path):
    """12 key-frames of the analytic ray caster, a CVoxelMap plan: the grid equals the restatement's cell for cell; the interior
    reads free, the walls and the box occupied, the outside unknown.  Restatement alone: 548 of 29 505 interior cells unknown, the
    shadow of the box (bound: 1 096), 10 of 704 wall sites without an occupied cell (bound: 20)."""
    from mola_lidar_odometry_amd import _mp2p_icp_hip as H
    frames, kfset, want = room
    g = H.build_occupancy_grid(kfset)
    for k in ("x0", "y0", "nx", "ny", "resolution", "z_lo", "z_hi", "l_occ", "cells_occupied", "cells_free", "cells_unknown", "map_cells"):
        assert g[k] == want[k], k
    assert g["frames"] == 12 and g["points"] == 12 * 720
    assert np.array_equal(g["max_logodds"], want["max_logodds"]) and np.array_equal(g["cells"], want["cells"])
    n_in, in_unknown, in_occupied, n_sites, sites_open, n_out, out_known = G.room_shares(g)
    assert n_in == 29505 and n_sites == 704 and in_unknown <= 1096 and in_occupied == 0 and sites_open <= 20 and out_known == 0
    cells = g["cells"]
    box = cells[int(round(1.0 / oc.RES)) - g["y0"] - 1:int(round(2.0 / oc.RES)) - g["y0"] + 1,
                int(round(1.0 / oc.RES)) - g["x0"] - 1:int(round(2.5 / oc.RES)) - g["x0"] + 1]
    assert (box == G.OCCUPIED).sum() >= 30 and (box[3:-3, 3:-3] == G.UNKNOWN).all()   # the face towards the drive is 30 cells long; its inside is never seen
    # the same with passes of one frame and another band that holds the plane z = 0
    g2 = H.build_occupancy_grid(kfset, "occupancy_grid:\n  z_min: 0.0\n  z_max: 0.04\n", max_points_per_pass=720)
    assert np.array_equal(g2["cells"], want["cells"]) and (g2["z_lo"], g2["z_hi"]) == (0, 0)
    g3 = H.build_occupancy_grid(kfset, "occupancy_grid:\n  z_min: 0.05\n")           # a band above the plane: nothing known
    assert g3["cells_unknown"] == g3["nx"] * g3["ny"]
    with pytest.raises(RuntimeError, match="target_map 'other'"):
        H.build_occupancy_grid(kfset, "occupancy_grid:\n  target_map: other\n")
    # the files, and the CLI on the written key-frame file
    prefix = str(tmp_path / "room")
    H.write_occupancy_grid(g, prefix)
    pgm = open(prefix + ".pgm", "rb").read()
    assert pgm == G.pgm_bytes(want["cells"])
    assert open(prefix + ".yaml").read() == G.yaml_text("room.pgm", 0.05, want["x0"], want["y0"])
    kf = str(tmp_path / "room.kf")
    H.write_keyframe_file(kf, kfset)
    r = subprocess.run([CLI, "--build-occupancy-grid", kf, str(tmp_path / "cli")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    line = json.loads(r.stdout.strip().split("\n")[-1])
    assert (line["grid_nx"], line["grid_ny"], line["cells_occupied"], line["cells_free"], line["cells_unknown"]) == (
        want["nx"], want["ny"], want["cells_occupied"], want["cells_free"], want["cells_unknown"])
    assert open(str(tmp_path / "cli.pgm"), "rb").read() == pgm
    assert open(str(tmp_path / "cli.yaml")).read() == G.yaml_text("cli.pgm", 0.05, want["x0"], want["y0"])


# ---- allocation: buffers that did not grow in step, and a failure in a later pass ---------------------------------------------------
@pytest.mark.parametrize("n_bare", [3, 14, 15, 16, 17, 18, 19, 40])   # (the appended arrays are about the 16th growth of a call)
def test_scratch_blocks_that_grew_out_of_step_change_nothing(ctx, n_bare):
    """the next n_bare buffer growths of the library get the bare need instead of the doubled block (the path a device short of
    memory takes), so the three arrays of the chunks' appended entries end with different capacities: the same bits"""
    def insert(occ, frames, budget):
        try:
            capi.fail_allocations(n_bare, 0)
            og.insert_frames(occ, frames, budget)
        finally:
            capi.fail_allocations(0, 0)
    frames = oc.random_frames([65, 33, 257, 64], seed=71) + oc.clamp_frames_once_own()
    a, _, _ = run(ctx, frames, insert=insert, batched_keys_per_pass=64)
    og.insert_frames(a, frames)                       # ... and the handle goes on with those blocks
    d, _, _ = run(ctx, frames + frames)
    for x, y in zip(a.download(), d.download()):
        assert np.array_equal(x, y)


def test_a_failure_in_a_later_pass_leaves_the_completed_passes_and_their_totals(ctx):
    small, big = oc.random_frames([65], seed=81)[0], oc.random_frames([2000], seed=82)[0]
    a, b, ref = run(ctx, [small], post=[small, small])                        # warm: every buffer of a pass of `small` is in place
    keys_small = a.info().n_keys
    before = a.info().n_cells
    try:
        capi.fail_allocations(1 << 20, 1 << 20)                               # no buffer can grow: the pass of `big` cannot run
        with pytest.raises(capi.MolahipError) as e:
            og.insert_frames(a, [small, big], max_points_per_pass=65)
        assert e.value.status == 3
    finally:
        capi.fail_allocations(0, 0)
    i = a.info()
    assert (i.n_keys, i.n_passes, i.n_left_out, i.n_cells) == (keys_small, 1, 0, before)   # the totals of the completed pass alone
    insert_single(ctx, b, *small)
    ref.insert(*small)
    og.insert_frames(a, [big])                                                # the handle is usable; the first pass had been applied
    insert_single(ctx, b, *big)
    ref.insert(*big)
    same(a, b, ref)
