"""include/molahip_nav.h on the device.  Every plane (d2, cost, reach) is compared bit for bit with tests/nav_ref.py, the numpy
restatement written from the header (brute-force distances, a flood fill by repeated dilation); the host path (key-frames to source
map to costmap to files, through pybind and the command line) is held to the same restatement on the outdoor scenario of
tests/elev_cases.py, and to the facts its geometry gives.

The scenario: an 8 m road, a 1 m box 0.4 m off the centre line.  The traversability map marks the box lethal and every road cell
beside it free; whether a vehicle of 1 m or of 2 m radius passes cannot be read from it.  Here: at 1 m no key-frame is blocked and
all twelve are reached from the first; at 2 m the fourth key-frame (8 cells from the box) is blocked and, with unknown cells as
obstacles, the drive ends at the box: the key-frames reached are {0, 1, 2}."""
import json
import os
import subprocess

import numpy as np
import pytest

from mola_lidar_odometry_amd import capi
from mola_lidar_odometry_amd import capi_nav as cn

import elev_cases as ec
import elev_ref as ER
import nav_cases as nc
import nav_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "mola_lidar_odometry_amd", "molahip-lo-cli")


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def inflate_same(ctx, base, Rc, table=None, unknown=False):
    """the device's d2 and cost of a base plane against the restatement's; returns the handle and the restatement's pair"""
    base = np.asarray(base, np.uint8)
    ny, nx = base.shape
    table = nc.ramp_table(Rc) if table is None else table
    nav = cn.NavMap(ctx, nx, ny).set_base(base).inflate(Rc, table, unknown)
    d2, cost, _ = nav.download(reach=False)
    want_d2, want_cost = R.inflate(base, Rc, table, unknown)
    assert d2.dtype == np.uint16 and cost.dtype == np.uint8
    bad = np.argwhere(d2 != want_d2)
    assert len(bad) == 0, ("d2", nx, ny, Rc, bad[:5].tolist())
    bad = np.argwhere(cost != want_cost)
    assert len(bad) == 0, ("cost", nx, ny, Rc, bad[:5].tolist())
    return nav, want_d2, want_cost


def reach_same(nav, cost, seeds, below=253):
    nav.reach(seeds, below)
    got = nav.download(d2=False, cost=False)[2]
    want, info = R.reach(cost, seeds, below)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, ("reach", bad[:5].tolist())
    i = nav.info()
    assert (int(i.n_reached), int(i.n_seeds_blocked), int(i.n_seeds_outside)) == (info["n_reached"], info["n_seeds_blocked"], info["n_seeds_outside"])
    return got, int(i.n_sweeps)


# ---- distance and cost --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Rc", nc.RADII)
def test_every_window_at_every_radius(ctx, Rc):
    """random planes with lethal and unknown cells and costs of 0 .. 253 under them, in every window of the list (33 x 9 at R = 255
    is a window smaller than the halo), unknown cells as obstacles and not"""
    for k, (nx, ny) in enumerate(nc.WINDOWS):
        dense = nx * ny < 1000
        base = nc.random_base(nx, ny, seed=100 * Rc + k, lethal=0.05 if dense else 0.002, unknown=0.05 if dense else 0.001)
        inflate_same(ctx, base, Rc, unknown=False)
        inflate_same(ctx, base, Rc, unknown=True)


@pytest.mark.parametrize("shape", [(530000, 1), (1, 530000)])
def test_one_row_and_one_column_of_530000_cells(ctx, shape):
    nx, ny = shape
    rng = np.random.default_rng(53)
    base = nc.empty(nx, ny)
    at = rng.choice(nx * ny, 300, replace=False)
    base.reshape(-1)[at] = nc.LETHAL
    base.reshape(-1)[rng.choice(nx * ny, 300, replace=False)] = 77
    for Rc in (2, 255):
        nav, d2, cost = inflate_same(ctx, base, Rc)
    free = np.flatnonzero(base.reshape(-1) != nc.LETHAL)
    seeds = np.stack([free[[0, -1]] % nx, free[[0, -1]] // nx], axis=1).astype(np.int32)
    nav.reach(seeds, 254)                        # the two end corridors between obstacles 1 766 cells apart on average: the dilation
    got = nav.download(d2=False, cost=False)[2]  # loop of the restatement would take as many passes over the plane, so the walk from
    assert np.array_equal(got, R.components_of(cost, seeds, 254))    # the seeds stands in for it (the tests below hold one to the other)
    assert int(nav.info().n_reached) == int(got.sum()) > 0


def test_no_obstacle_every_cell_an_obstacle_and_obstacles_at_the_rim(ctx):
    for nx, ny in ((1, 1), (33, 9), (32, 8), (70, 1), (1, 70), (130, 67)):
        for Rc in (0, 2, 255):
            _, d2, _ = inflate_same(ctx, nc.random_base(nx, ny, 3, lethal=0.0, unknown=0.1), Rc)      # no obstacle at all
            assert (d2 == R.FAR).all()
            _, d2, _ = inflate_same(ctx, nc.empty(nx, ny, nc.LETHAL), Rc)                           # every cell an obstacle
            assert (d2 == 0).all()
            _, d2, _ = inflate_same(ctx, nc.empty(nx, ny, nc.UNKNOWN), Rc, unknown=True)
            assert (d2 == 0).all()
            for b in nc.corners(nx, ny) + [nc.first_row(nx, ny), nc.last_column(nx, ny)]:
                inflate_same(ctx, b, Rc)
    for b in nc.corners(300, 260) + [nc.first_row(300, 260), nc.last_column(300, 260)]:
        inflate_same(ctx, b, 255)
        inflate_same(ctx, b, 30)


def test_obstacles_on_the_edges_of_segments_and_tiles(ctx):
    """the row pass works in segments of ROW_SEGMENT cells, the column pass in tiles of COL_TILE x COL_TILE: obstacles in the last
    cell of one, the first of the next and one further, in windows that end on such an edge, one short of it and one beyond"""
    S, T = cn.ROW_SEGMENT, cn.COL_TILE
    assert (S, T) == (256, 64)
    xs = [S - 1, S, S + 1, 2 * S - 1, 2 * S, 2 * S + 1, T - 1, T, T + 1]
    ys = [T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1]
    for nx, ny in ((2 * S + 1, 2 * T + 2), (2 * S, 2 * T), (2 * S - 1, 2 * T - 1), (S + 1, T + 1), (S, T), (S - 1, T - 1)):
        b = nc.on_edges(nx, ny, xs, ys)
        for Rc in (1, 30, 255):
            inflate_same(ctx, b, Rc)
        for x in (x for x in xs if x < nx):                      # one obstacle alone in such a column, and in such a row
            one = nc.empty(nx, ny)
            one[ny // 2, x] = nc.LETHAL
            inflate_same(ctx, one, 255)
        for y in (y for y in ys if y < ny):
            one = nc.empty(nx, ny)
            one[y, nx // 2] = nc.LETHAL
            inflate_same(ctx, one, 255)


@pytest.mark.parametrize("Rc", [1, 2, 8, 30, 255])
def test_a_cell_at_exactly_the_radius_and_one_beyond(ctx, Rc):
    _, d2, _ = inflate_same(ctx, nc.at_radius(Rc), Rc)
    assert d2[0, Rc] == Rc * Rc and d2[Rc, 0] == Rc * Rc
    assert d2[0, Rc + 1] == R.FAR and d2[Rc + 1, 0] == R.FAR and d2[1, Rc] == R.FAR


def test_the_table_is_applied_under_the_maximum_with_the_base(ctx):
    Rc = 3
    table = np.array([0, 253, 200, 0, 150, 120, 0, 0, 100, 50], np.uint8)       # (table[0] is never read)
    base = nc.empty(16, 5)
    base[0, :], base[1, :], base[3, :], base[4, :] = 0, 100, 251, 253
    base[2, :8], base[2, 8], base[2, 9:] = 100, nc.LETHAL, 251
    _, d2, cost = inflate_same(ctx, base, Rc, table)
    assert cost[2, 7] == 253 and cost[2, 6] == 150 and cost[2, 5] == 100 and cost[2, 4] == 100         # max(100, table)
    assert cost[2, 9] == 253 and cost[2, 10] == 251 and cost[2, 12] == 251                             # max(251, table)
    assert cost[0, 8] == 150 and cost[1, 8] == 253 and cost[3, 8] == 253 and cost[4, 8] == 253         # bases 0, 100, 251, 253
    with_zero = table.copy()
    with_zero[0] = 253
    inflate_same(ctx, base, Rc, with_zero)
    assert np.array_equal(R.inflate(base, Rc, with_zero)[1], cost)                                     # table[0] plays no part


def test_the_row_pass_without_its_early_stop_gives_the_same_bits(ctx, monkeypatch):
    monkeypatch.setenv("MH_NAV_NO_EARLY_STOP", "1")                              # (read per call: the measuring switch)
    for Rc in (2, 30, 255):
        inflate_same(ctx, nc.random_base(300, 260, 5, lethal=0.002), Rc)
        inflate_same(ctx, nc.random_base(33, 9, 6, lethal=0.05), Rc, unknown=True)


def test_pinned_and_device_bases_give_the_same_bits(ctx):
    import torch
    base = nc.random_base(300, 260, 8)
    table = nc.ramp_table(8)
    want = R.inflate(base, 8, table)
    t = torch.from_numpy(base.copy())
    for mem, arr in ((capi.MEM_DEVICE, t.cuda()), (capi.MEM_HOST_PINNED, t.pin_memory())):
        torch.cuda.synchronize()
        nav = cn.NavMap(ctx, 300, 260).set_base(arr.data_ptr(), mem).inflate(8, table)
        d2, cost, _ = nav.download(reach=False)
        assert np.array_equal(d2, want[0]) and np.array_equal(cost, want[1]), mem


def test_two_handles_and_a_new_base_invalidates(ctx):
    a_base, b_base = nc.random_base(70, 40, 1), nc.random_base(33, 90, 2)
    a, _, a_cost = inflate_same(ctx, a_base, 8)
    b, _, b_cost = inflate_same(ctx, b_base, 30)
    reach_same(a, a_cost, [[1, 1], [60, 30]])
    reach_same(b, b_cost, [[2, 2]])
    d2, cost, _ = a.download(reach=False)
    assert np.array_equal(cost, a_cost)
    a.set_base(b_base[:40, :].repeat(3, axis=1)[:, :70])
    i = a.info()
    assert (i.has_base, i.has_cost, i.has_reach) == (1, 0, 0)
    for planes in (dict(reach=False, cost=False), dict(d2=False, reach=False), dict(d2=False, cost=False)):
        with pytest.raises(capi.MolahipError) as e:
            a.download(**planes)
        assert e.value.status == 1
    with pytest.raises(capi.MolahipError) as e:
        a.reach([[1, 1]])                                                         # reach before inflate
    assert e.value.status == 1
    a.inflate(2, nc.ramp_table(2))
    assert a.download(d2=False, reach=False)[1] is not None
    with pytest.raises(capi.MolahipError):
        a.download(d2=False, cost=False)                                          # inflate alone does not bring reach back


# ---- reach --------------------------------------------------------------------------------------------------------------------------
def test_seeds_on_passable_and_impassable_cells_and_outside(ctx):
    base = nc.random_base(130, 67, 21, lethal=0.25, unknown=0.05, costs=False)
    nav, _, cost = inflate_same(ctx, base, 0, nc.zero_table(0))
    free = np.argwhere(cost < 253)[:, ::-1]
    blocked = np.argwhere(cost >= 253)[:, ::-1]
    outside = np.array([[-1, 0], [0, -1], [130, 0], [0, 67], [1 << 30, 3], [-(1 << 31), -(1 << 31)]])
    rng = np.random.default_rng(3)
    reach_same(nav, cost, np.zeros((0, 2), np.int32))                             # no seed: an all-zero plane
    assert nav.info().n_sweeps == 0
    reach_same(nav, cost, free[:1])
    reach_same(nav, cost, blocked[:3])
    assert nav.info().n_sweeps == 0
    reach_same(nav, cost, outside)
    many = np.concatenate([free[rng.integers(0, len(free), 3000)], blocked[rng.integers(0, len(blocked), 1500)], outside[rng.integers(0, 6, 500)]])
    rng.shuffle(many)
    assert len(many) == 5000
    got, _ = reach_same(nav, cost, many)
    again, _ = reach_same(nav, cost, many[rng.permutation(5000)])                 # the order of the seeds plays no part
    assert np.array_equal(got, again)
    assert np.array_equal(R.components_of(cost, many, 253), got)


def test_passable_below_at_its_ends(ctx):
    base = np.tile(np.arange(256, dtype=np.uint8), (3, 1))                        # every byte value in a row
    nav, _, cost = inflate_same(ctx, base, 0, nc.zero_table(0))
    for below, n in ((1, 1), (253, 253), (254, 254)):
        got, _ = reach_same(nav, cost, [[0, 1]], below)
        assert got.sum() == 3 * n and got[:, :n].all()
    for below in (0, 255, 1000):
        with pytest.raises(capi.MolahipError) as e:
            nav.reach([[0, 1]], below)
        assert e.value.status == 1


def test_diagonal_neighbours_walls_and_gaps(ctx):
    b = nc.diagonal_touch(12)
    nav, _, cost = inflate_same(ctx, b, 0, nc.zero_table(0))
    got, _ = reach_same(nav, cost, [[2, 2]])
    assert got[1:6, 1:6].all() and not got[6:, 6:].any()                          # touching at a corner does not join
    TX, TY = cn.REACH_TILE_X, cn.REACH_TILE_Y
    assert (TX, TY) == (64, 16)
    for x, gap in ((70, None), (70, 20), (TX - 1, TY - 1), (TX, TY), (TX, TY - 1), (TX - 1, TY), (2 * TX, 2 * TY), (2 * TX - 1, 2 * TY - 1)):
        b = nc.wall(200, 50, x, gap)                                              # a wall with no gap, with one, with one on a tile corner
        nav, _, cost = inflate_same(ctx, b, 0, nc.zero_table(0))
        got, _ = reach_same(nav, cost, [[3, 3]])
        assert got[:, :x].all() and bool(got[:, x + 1:].all()) == (gap is not None) and bool(got[:, x + 1:].any()) == (gap is not None)


def test_a_serpentine_needs_more_than_one_sweep(ctx):
    b = nc.serpentine(65)
    nav, _, cost = inflate_same(ctx, b, 0, nc.zero_table(0))
    got, sweeps = reach_same(nav, cost, [[0, 0]])
    print("serpentine 65 x 65: sweeps", sweeps)
    assert got[64].all() and got.sum() == (b == 0).sum() and sweeps >= 2


def test_corridors_of_one_cell(ctx):
    for nx, ny in ((70, 1), (1, 70)):
        b = nc.empty(nx, ny)
        b.reshape(-1)[50] = nc.LETHAL
        nav, _, cost = inflate_same(ctx, b, 0, nc.zero_table(0))
        got, _ = reach_same(nav, cost, [[0, 0]])
        assert got.reshape(-1)[:50].all() and not got.reshape(-1)[50:].any()
        got, _ = reach_same(nav, cost, [[nx - 1, ny - 1], [0, 0]])
        assert got.sum() == 69


def test_every_refusal(ctx):
    L = cn.lib()
    h = cn.C.c_void_p()
    for nx, ny in ((0, 4), (4, 0), (8193, 8192), (1 << 31, 1)):
        assert L.mh_nav_create(ctx._h, nx, ny, cn.C.byref(h)) == 1 and not h.value
    assert L.mh_nav_create(ctx._h, 4, 4, None) == 1
    nav = cn.NavMap(ctx, 6, 5)
    base = nc.random_base(6, 5, 1)
    t = nc.ramp_table(2)
    tp = t.ctypes.data_as(cn._U8P)
    assert L.mh_nav_inflate(nav._h, 2, 0, tp, 5) == 1                             # before set_base
    assert L.mh_nav_set_base(nav._h, None, 0) == 1 and L.mh_nav_set_base(nav._h, base.ctypes.data, 7) == 1
    assert nav.info().has_base == 0
    nav.set_base(base)
    assert L.mh_nav_inflate(nav._h, 256, 0, tp, 65537) == 1                       # R > 255
    assert L.mh_nav_inflate(nav._h, 2, 0, tp, 4) == 1 and L.mh_nav_inflate(nav._h, 2, 0, tp, 6) == 1      # a wrong n_table
    assert L.mh_nav_inflate(nav._h, 2, 0, None, 5) == 1
    for k in (0, 3, 4):
        badt = t.copy()
        badt[k] = 254
        assert L.mh_nav_inflate(nav._h, 2, 0, badt.ctypes.data_as(cn._U8P), 5) == 1                     # an entry > 253
    assert nav.info().has_cost == 0
    nav.inflate(2, t)
    want = R.inflate(base, 2, t)
    assert L.mh_nav_reach(nav._h, None, 1, 253) == 1
    one = np.array([[1, 1]], np.int32)
    for below in (0, 255):
        assert L.mh_nav_reach(nav._h, one.ctypes.data_as(cn._I32P), 1, below) == 1
    assert nav.info().has_reach == 0
    d2, cost, _ = nav.download(reach=False)                                       # the refused calls left the handle as it was
    assert np.array_equal(d2, want[0]) and np.array_equal(cost, want[1])


# ---- the host path: the scenario ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scenario():
    frames, kfset = ec.scenario()
    return frames, kfset, ER.build(frames, **ec.SCENARIO_OPTIONS_DICT)


KEYS = ("x0", "y0", "nx", "ny", "resolution", "max_cells", "cells_lethal", "cells_inscribed", "cells_inflated", "cells_free", "cells_unknown",
        "cells_reached", "cells_unreachable_free", "keyframe_d2", "keyframe_cost", "keyframe_reached", "keyframes_blocked", "seeds_blocked",
        "seeds_outside")


def equal_costmaps(c, want):
    for k in KEYS:
        assert c[k] == want[k], k
    for k in ("d2", "cost", "reach"):
        assert c[k].dtype == want[k].dtype and np.array_equal(c[k], want[k]), k
    assert abs(c["trajectory_min_clearance_m"] - want["trajectory_min_clearance_m"]) < 1e-12


def restated(src, frames, **opt):
    return R.build(src["cost"], src["x0"], src["y0"], 0.2, [T for _, T in frames], **opt)


def test_the_scenario_at_one_metre_every_key_frame_is_reached(scenario):
    from mola_lidar_odometry_amd import _mp2p_icp_hip as H
    frames, kfset, src = scenario
    assert (src["nx"], src["ny"], src["cells_lethal"], src["cells_unknown"]) == (404, 54, 626, 2816)
    regions = ec.scenario_regions(src)
    for unknown in (False, True):
        c = H.build_costmap_from_keyframes(kfset, nc.scenario_pipeline(1.0, 2.0, unknown, "first"))
        equal_costmaps(c, restated(src, frames, inscribed_radius=1.0, inflation_radius=2.0, unknown_is_obstacle=unknown, reach_from="first"))
        print("1 m, unknown_is_obstacle", unknown, ": sweeps", c["sweeps"], "reached", c["cells_reached"])
        assert c["keyframes_blocked"] == 0 and c["keyframe_reached"] == [1] * 12 and c["keyframe_d2"][3] == 64
        assert abs(c["trajectory_min_clearance_m"] - 1.6) < 1e-12
        assert all(v == R.FAR for k, v in enumerate(c["keyframe_d2"]) if k != 3)          # every other key-frame is farther than 2 m
        # the defect this product exists for: the traversability map reads every road cell beside the box as free; the vehicle of
        # 1 m radius cannot stand on the ring of cells around the box, nor on the road cells along the kerb
        road, _ = regions["road"]
        free_in_source = int((src["cost"][road] == 0).sum())
        passable = int((c["cost"][road] < 253).sum())
        print("region road: cost-0 cells of the traversability map", free_in_source, "passable here", passable)
        assert passable < free_in_source
        ix = src["x0"] + np.arange(src["nx"])[None, :]
        iy = src["y0"] + np.arange(src["ny"])[:, None]
        cell = lambda v: int(round(v / ec.RES))
        bx0, bx1, by0, by1, _ = ec.BOX
        ring = (ix >= cell(bx0) - 1) & (ix <= cell(bx1)) & (iy >= cell(by0) - 1) & (iy <= cell(by1)) & (src["cost"] != 254)
        assert ring.sum() > 0 and (src["cost"][ring] < 254).all() and (c["cost"][ring] >= 253).all()


def test_the_scenario_at_two_metres_the_box_closes_the_road(scenario):
    from mola_lidar_odometry_amd import _mp2p_icp_hip as H
    frames, kfset, src = scenario
    c = H.build_costmap_from_keyframes(kfset, nc.scenario_pipeline(2.0, 3.0, True, "first"))
    equal_costmaps(c, restated(src, frames, inscribed_radius=2.0, inflation_radius=3.0, unknown_is_obstacle=True, reach_from="first"))
    print("2 m, unknown cells obstacles: sweeps", c["sweeps"], "reached", c["cells_reached"])
    assert c["keyframe_cost"][3] >= 253 and c["keyframes_blocked"] == 1
    assert [k for k, r in enumerate(c["keyframe_reached"]) if r] == [0, 1, 2]    # both corridors beside the box are under 4 m wide
    c = H.build_costmap_from_keyframes(kfset, nc.scenario_pipeline(2.0, 3.0, False, "first"))
    equal_costmaps(c, restated(src, frames, inscribed_radius=2.0, inflation_radius=3.0, unknown_is_obstacle=False, reach_from="first"))
    print("2 m, unknown cells no obstacles: sweeps", c["sweeps"], "reached", c["cells_reached"])
    assert [k for k, r in enumerate(c["keyframe_reached"]) if not r] == [3]      # round the box where the road simply ends
    c = H.build_costmap_from_keyframes(kfset, nc.scenario_pipeline(2.0, 3.0, False, "keyframes"))
    equal_costmaps(c, restated(src, frames, inscribed_radius=2.0, inflation_radius=3.0, reach_from="keyframes"))
    assert c["seeds_blocked"] == 1
    c = H.build_costmap_from_keyframes(kfset, nc.scenario_pipeline(2.0, 3.0, False, "none"))
    assert c["cells_reached"] == 0 and c["sweeps"] == 0


def test_the_scenario_through_build_costmap_the_files_and_the_command_line(scenario, tmp_path):
    from mola_lidar_odometry_amd import _mp2p_icp_hip as H
    frames, kfset, src = scenario
    poses = [T.tolist() for _, T in frames]
    text = nc.scenario_pipeline(2.0, 3.0, True, "first")
    want = restated(src, frames, inscribed_radius=2.0, inflation_radius=3.0, unknown_is_obstacle=True, reach_from="first")
    c = H.build_costmap(dict(x0=src["x0"], y0=src["y0"], nx=src["nx"], ny=src["ny"], resolution=0.2, cost=src["cost"]), poses, text)
    equal_costmaps(c, want)
    # an occupancy grid as the source: occupied -> 254, unknown -> 255, free -> 0
    og = H.build_occupancy_grid(kfset, "occupancy_grid:\n  resolution: 0.2\n  update_rule: once\n")
    c_og = H.build_costmap(og, poses, text)
    equal_costmaps(c_og, R.build(R.base_of_grid(og["cells"]), og["x0"], og["y0"], 0.2, [T for _, T in frames], inscribed_radius=2.0,
                                 inflation_radius=3.0, unknown_is_obstacle=True, reach_from="first"))
    prefix = str(tmp_path / "road")
    H.write_costmap(c, prefix)
    files = {".pgm": R.trinary_pgm_bytes(want["cost"]), "_cost.pgm": R.cost_pgm_bytes(want["cost"]), "_reach.pgm": R.reach_pgm_bytes(want["reach"])}
    for s, b in files.items():
        assert open(prefix + s, "rb").read() == b, s
    assert open(prefix + ".yaml").read() == R.yaml_text("road", 0.2, want["x0"], want["y0"], 2.0, 3.0)
    kf = str(tmp_path / "road.kf")
    H.write_keyframe_file(kf, kfset)
    pipeline = tmp_path / "pipeline.yaml"
    pipeline.write_text(text)
    r = subprocess.run([CLI, "--build-costmap", kf, str(tmp_path / "cli"), "-c", str(pipeline)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    line = json.loads(r.stdout.strip().split("\n")[-1])
    for k_line, k_want in (("grid_nx", "nx"), ("grid_ny", "ny"), ("max_cells", "max_cells"), ("cells_lethal", "cells_lethal"),
                           ("cells_inscribed", "cells_inscribed"), ("cells_inflated", "cells_inflated"), ("cells_free", "cells_free"),
                           ("cells_unknown", "cells_unknown"), ("cells_reached", "cells_reached"),
                           ("cells_unreachable_free", "cells_unreachable_free"), ("keyframes_blocked", "keyframes_blocked")):
        assert line[k_line] == want[k_want], k_line
    assert line["keyframes"] == 12 and abs(line["trajectory_min_clearance_m"] - 1.6) < 1e-6
    for s, b in files.items():
        assert open(str(tmp_path / "cli") + s, "rb").read() == b, s
    assert open(str(tmp_path / "cli.yaml")).read() == R.yaml_text("cli", 0.2, want["x0"], want["y0"], 2.0, 3.0)
    back = H.read_costmap(str(tmp_path / "cli"))
    assert np.array_equal(back["cost"], want["cost"]) and np.array_equal(back["reach"], want["reach"]) and back["d2"].size == 0
    H.write_costmap(back, str(tmp_path / "back"))
    for s, b in files.items():                                                    # read back to the same bytes
        assert open(str(tmp_path / "back") + s, "rb").read() == b, s
    assert open(str(tmp_path / "back.yaml")).read() == R.yaml_text("back", 0.2, want["x0"], want["y0"], 2.0, 3.0)
