"""The costmap of a recorded session, the parts that need no device: the costmap: options and every refusal by name, the inflation
table against tests/nav_ref.py -- exactly --, the base plane from both kinds of source map, the seeds, the counts, the files and their
round trip, the command line's refusals, and the restatement's own properties, on which the device tests of tests/test_gpu_nav.py
rest (the brute-force distance against a second formulation; the dilation loop against a walk from the seeds)."""
import os
import subprocess

import numpy as np
import pytest

import nav_cases as nc
import nav_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "mola_lidar_odometry_amd", "molahip-lo-cli")


@pytest.fixture(scope="module")
def host():
    from mola_lidar_odometry_amd import _mp2p_icp_hip as H
    return H


def block(**kv):
    return "costmap:\n" + "".join("  %s: %s\n" % (k, v) for k, v in kv.items())


def pose(x, y):
    return [1.0, 0, 0, x, 0, 1.0, 0, y, 0, 0, 1.0, 0]


# ---- options -----------------------------------------------------------------------------------------------------------------------
def test_the_defaults_and_a_full_block(host):
    assert host.costmap_options() == R.DEFAULTS
    want = dict(source="occupancy_grid", inscribed_radius=0.25, inflation_radius=0.25, cost_scaling=10.0, unknown_is_obstacle=True, reach_from="first")
    assert host.costmap_options(block(source="occupancy_grid", inscribed_radius=0.25, inflation_radius=0.25, cost_scaling=10,
                                      unknown_is_obstacle="true", reach_from="first")) == want
    assert host.costmap_options("traversability:\n  resolution: 0.1\n") == R.DEFAULTS                 # another block is not this one
    assert host.costmap_options(block(reach_from="none"))["reach_from"] == "none"


@pytest.mark.parametrize("key,value", [("source", "points"), ("inscribed_radius", -0.1), ("inscribed_radius", "nan"), ("inscribed_radius", "wide"),
                                       ("inflation_radius", 0.4), ("inflation_radius", "inf"), ("cost_scaling", 0), ("cost_scaling", -1),
                                       ("cost_scaling", "inf"), ("unknown_is_obstacle", "maybe"), ("reach_from", "last"), ("reach_from", "Keyframes"),
                                       ("no_such_key", 1), ("inflationradius", 2.0)])
def test_a_bad_value_or_an_unknown_key_is_refused_by_name(host, key, value):
    with pytest.raises(RuntimeError, match=r"costmap: %s\b" % key):
        host.costmap_options(block(**{key: value}))


def test_a_radius_of_more_than_255_cells_is_refused_by_name(host):
    assert len(host.inflation_table(block(inscribed_radius=0.5, inflation_radius=51.0), 0.2)) == 255 * 255 + 1
    with pytest.raises(RuntimeError, match=r"costmap: inflation_radius\b.*255 cells"):
        host.inflation_table(block(inflation_radius=51.3), 0.2)
    with pytest.raises(RuntimeError, match="resolution"):
        host.inflation_table(None, 0.0)
    kfset = dict(maps=[], frames=[])
    with pytest.raises(RuntimeError, match=r"costmap: inflation_radius\b"):                            # before the source map is built
        host.build_costmap_from_keyframes(kfset, block(inflation_radius=60.0))


# ---- the table ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("resolution", [0.05, 0.2, 0.25])
def test_the_table_is_the_restatement_s(host, resolution):
    cases = [dict(), dict(inscribed_radius=1.0, inflation_radius=2.0), dict(inscribed_radius=0.0, inflation_radius=0.0),
             dict(inscribed_radius=0.3, inflation_radius=0.77, cost_scaling=0.5), dict(inscribed_radius=2.0, inflation_radius=3.0, cost_scaling=12.5),
             dict(inscribed_radius=0.75, inflation_radius=0.75),                                       # inscribed == inflation
             dict(inscribed_radius=10 * resolution, inflation_radius=20 * resolution),                 # radii on an exact cell multiple
             dict(inscribed_radius=100 * resolution, inflation_radius=255 * resolution)]               # R == 255
    for opt in cases:
        got = host.inflation_table(block(**opt) if opt else None, resolution)
        want = R.table(resolution, **dict(R.DEFAULTS, **opt))
        assert got.dtype == np.uint8 and np.array_equal(got, want), opt
        assert got[0] == 0 and (got <= 253).all()


def test_the_table_s_three_boundaries_are_where_the_rule_puts_them(host):
    # radii on an exact multiple of the cell: the cell AT the radius belongs to it (d <= radius), the next does not
    t = host.inflation_table(block(inscribed_radius=1.0, inflation_radius=2.0), 0.25)
    assert len(t) == 8 * 8 + 1 and t[16] == 253 and t[17] == int(np.floor(252 * np.exp(-3.0 * (np.sqrt(17.0) * 0.25 - 1.0)))) < 253
    assert t[64] == int(np.floor(252 * np.exp(-3.0))) == 12 and t[63] >= 12
    # inscribed == inflation: 253 up to the radius, nothing beyond; R = ceil(0.75 / 0.2) = 4, and 4 cells = 0.8 m lie beyond
    t = host.inflation_table(block(inscribed_radius=0.75, inflation_radius=0.75), 0.2)
    assert len(t) == 17 and [int(v) for v in t] == [0] + [253] * 14 + [0, 0]      # sqrt(14) * 0.2 = 0.748, sqrt(15) * 0.2 = 0.775
    # R == 255
    t = host.inflation_table(block(inscribed_radius=0.5, inflation_radius=12.75, cost_scaling=0.2), 0.05)
    assert len(t) == 65026 and t[100] == 253 and t[101] == 251 and t[65025] == int(np.floor(252 * np.exp(-0.2 * 12.25))) == 21
    t = host.inflation_table(block(inscribed_radius=0.0, inflation_radius=0.0), 0.2)
    assert [int(v) for v in t] == [0]                                             # R = 0: only table[0], never read


# ---- base plane, seeds, counts ------------------------------------------------------------------------------------------------------
def test_the_base_plane_of_both_map_kinds(host):
    cost = nc.random_base(7, 5, 3)
    trav = dict(x0=-3, y0=2, nx=7, ny=5, resolution=0.2, cost=cost)
    got = host.costmap_base(trav)
    assert got.dtype == np.uint8 and np.array_equal(got, cost)                     # the traversability bytes as they are
    cells = np.array([[0, 100, -1], [-1, 0, 100]], np.int8)
    grid = dict(x0=0, y0=0, nx=3, ny=2, resolution=0.05, cells=cells)
    assert np.array_equal(host.costmap_base(grid), R.base_of_grid(cells))
    assert host.costmap_base(grid).tolist() == [[0, 254, 255], [255, 0, 254]]
    with pytest.raises(RuntimeError, match="neither occupied"):
        host.costmap_base(dict(grid, cells=np.array([[0, 50, -1], [-1, 0, 100]], np.int8)))
    with pytest.raises(RuntimeError, match="ny \\* nx"):
        host.costmap_base(dict(trav, nx=8))


def test_the_seeds_fall_where_the_floor_rule_puts_them(host):
    F = np.float32
    res = 0.2
    win = dict(x0=-5, y0=-3, nx=12, ny=9, resolution=res, cost=np.zeros((9, 12), np.uint8))
    edge = float(F(3) * F(res))                                                   # a cell edge as fp32 computes it
    poses = [pose(0.0, 0.0), pose(-0.01, -0.01), pose(edge, np.nextafter(F(edge), F(-1))), pose(1.39, 1.19), pose(1.41, 0.0), pose(0.0, 1.21),
             pose(-1.01, 0.0), pose(0.0, -0.61), pose(np.nan, 0.0), pose(0.0, np.inf), pose(3.0e5, 0.0), pose(-1.0, -0.6)]
    want = R.seeds(poses, -5, -3, 12, 9, res)
    assert want.tolist()[:4] == [[5, 3], [4, 2], [8, 5], [11, 8]] and want.tolist()[4:11] == [[-1, -1]] * 7 and want.tolist()[11] == [0, 0]
    for mode in ("keyframes", "first", "none"):
        got = np.array(host.costmap_seeds(win, poses, mode), np.int32).reshape(-1, 2)
        assert np.array_equal(got, R.seeds(poses, -5, -3, 12, 9, res, mode)), mode
    assert len(host.costmap_seeds(win, poses, "first")) == 2 and host.costmap_seeds(win, poses, "none") == []
    assert host.costmap_seeds(win, [], "first") == []
    with pytest.raises(RuntimeError, match="costmap: reach_from"):
        host.costmap_seeds(win, poses, "all")
    for res in (0.05, 0.25):                                                      # the other resolutions, on and beside cell edges
        rng = np.random.default_rng(int(res * 100))
        poses = [pose(float(F(k) * F(res)) + d, float(rng.uniform(-2, 2))) for k in range(-20, 20) for d in (-1e-7, 0.0, 1e-7)]
        win = dict(x0=-25, y0=-50, nx=50, ny=100, resolution=res, cost=np.zeros((100, 50), np.uint8))
        got = np.array(host.costmap_seeds(win, poses, "keyframes"), np.int32).reshape(-1, 2)
        assert np.array_equal(got, R.seeds(poses, -25, -50, 50, 100, res))


def test_the_counts_and_the_trajectory(host):
    base = nc.random_base(40, 30, 9, lethal=0.03, unknown=0.05, costs=False)
    opt = dict(inscribed_radius=0.4, inflation_radius=1.0)
    poses = [pose(0.1 + 0.37 * k, 0.1 + 0.21 * k) for k in range(25)] + [pose(-1.0, 0.0), pose(100.0, 1.0)]
    want = R.build(base, 0, 0, 0.2, poses, **opt)
    got = host.costmap_summarise(dict(x0=0, y0=0, nx=40, ny=30, resolution=0.2, inscribed_radius=0.4, inflation_radius=1.0, d2=want["d2"],
                                      cost=want["cost"], reach=want["reach"]), poses)
    for k in ("cells_lethal", "cells_inscribed", "cells_inflated", "cells_free", "cells_unknown", "cells_reached", "cells_unreachable_free",
              "keyframe_d2", "keyframe_cost", "keyframe_reached", "keyframes_blocked"):
        assert got[k] == want[k], k
    assert abs(got["trajectory_min_clearance_m"] - want["trajectory_min_clearance_m"]) < 1e-12
    assert got["cells_lethal"] + got["cells_inscribed"] + got["cells_inflated"] + got["cells_free"] + got["cells_unknown"] == 1200
    assert got["keyframe_cost"][-2:] == [255, 255] and got["keyframe_d2"][-2:] == [R.FAR, R.FAR] and got["keyframes_blocked"] >= 2
    far = host.costmap_summarise(dict(x0=0, y0=0, nx=4, ny=4, resolution=0.2, inscribed_radius=0.4, inflation_radius=1.0,
                                      d2=np.full((4, 4), R.FAR, np.uint16), cost=np.zeros((4, 4), np.uint8), reach=np.ones((4, 4), np.uint8)),
                                 [pose(0.1, 0.1)])
    assert far["trajectory_min_clearance_m"] == -1.0 and far["cells_free"] == 16 and far["cells_reached"] == 16
    with pytest.raises(RuntimeError, match="ny \\* nx entries"):
        host.costmap_summarise(dict(x0=0, y0=0, nx=5, ny=4, resolution=0.2, inscribed_radius=0.4, inflation_radius=1.0,
                                    cost=np.zeros((4, 4), np.uint8), reach=np.ones((4, 4), np.uint8)), [])


# ---- files -------------------------------------------------------------------------------------------------------------------------
def _costmap(seed=4):
    base = nc.random_base(23, 11, seed, lethal=0.04, unknown=0.06)
    return R.build(base, -7, 3, 0.25, [pose(0.3, 1.2)], inscribed_radius=0.3, inflation_radius=0.8)


def test_the_files_are_the_restatement_s_bytes_and_read_back_to_the_same_bytes(host, tmp_path):
    want = _costmap()
    want["cost"][-1, :3] = (10, 32, 9)              # the image's first pixels are white space to a careless header parser
    want.update(R.summarise(want["d2"], want["cost"], want["reach"], -7, 3, 0.25, [pose(0.3, 1.2)]))
    prefix = str(tmp_path / "m")
    host.write_costmap(want, prefix)
    files = {".pgm": R.trinary_pgm_bytes(want["cost"]), "_cost.pgm": R.cost_pgm_bytes(want["cost"]), "_reach.pgm": R.reach_pgm_bytes(want["reach"]),
             ".yaml": R.yaml_text("m", 0.25, -7, 3, 0.3, 0.8).encode()}
    for s, b in files.items():
        assert open(prefix + s, "rb").read() == b, s
    assert sorted(os.listdir(tmp_path)) == ["m.pgm", "m.yaml", "m_cost.pgm", "m_reach.pgm"]
    back = host.read_costmap(prefix)
    for k in ("x0", "y0", "nx", "ny", "resolution", "inscribed_radius", "inflation_radius", "cells_lethal", "cells_inscribed", "cells_unknown",
              "cells_reached", "cells_unreachable_free"):
        assert back[k] == want[k], k
    assert np.array_equal(back["cost"], want["cost"]) and np.array_equal(back["reach"], want["reach"]) and back["d2"].size == 0
    host.write_costmap(back, str(tmp_path / "n"))
    for s, b in files.items():
        assert open(str(tmp_path / "n") + s, "rb").read() == (b if s != ".yaml" else R.yaml_text("n", 0.25, -7, 3, 0.3, 0.8).encode()), s
    g = host.read_occupancy_grid(prefix)                                          # the trinary pair is the occupancy grid's
    assert np.array_equal(g["cells"], np.where(want["cost"] == 255, -1, np.where(want["cost"] >= 253, 100, 0)))


def test_the_reader_and_the_writer_refuse_what_they_cannot_take(host, tmp_path):
    want = _costmap()
    with pytest.raises(RuntimeError, match="nowhere"):
        host.read_costmap(str(tmp_path / "nowhere"))
    with pytest.raises(RuntimeError, match="cannot write"):
        host.write_costmap(want, str(tmp_path / "no_such_dir" / "m"))
    with pytest.raises(RuntimeError, match="holds no cells"):
        host.write_costmap(dict(want, nx=24), str(tmp_path / "bad"))
    prefix = str(tmp_path / "m")
    host.write_costmap(want, prefix)
    os.rename(prefix + "_reach.pgm", prefix + "_reach.away")
    with pytest.raises(RuntimeError, match="m_reach.pgm"):
        host.read_costmap(prefix)
    os.rename(prefix + "_reach.away", prefix + "_reach.pgm")
    cost = bytearray(open(prefix + "_cost.pgm", "rb").read())
    at = len(cost) - 1 - int(np.flatnonzero(want["cost"][::-1].reshape(-1)[::-1] < 253)[0])
    cost[at] = 254
    open(prefix + "_cost.pgm", "wb").write(bytes(cost))
    with pytest.raises(RuntimeError, match="disagrees"):
        host.read_costmap(prefix)
    host.write_costmap(want, prefix)
    reach = bytearray(open(prefix + "_reach.pgm", "rb").read())
    reach[-1] = 7
    open(prefix + "_reach.pgm", "wb").write(bytes(reach))
    with pytest.raises(RuntimeError, match="neither 0 nor 255"):
        host.read_costmap(prefix)
    host.write_costmap(want, prefix)
    text = open(prefix + ".yaml").read()
    open(prefix + ".yaml", "w").write(text.replace("reach_image", "reachimage"))
    with pytest.raises(RuntimeError, match="lacks cost_image"):
        host.read_costmap(prefix)


@pytest.mark.parametrize("image", ["_cost.pgm", "_reach.pgm"])
@pytest.mark.parametrize("change", [(b"255\n", b"255 "), (b"255\n", b"255\n\n"), (b"255\n", b"254\n"), (b"23 11", b"11 23"), (b"23 11", b"23 12")])
def test_an_image_whose_header_is_not_the_writer_s_is_refused(host, tmp_path, image, change):
    want = _costmap()
    prefix = str(tmp_path / "m")
    host.write_costmap(want, prefix)
    raw = open(prefix + image, "rb").read()
    assert raw[:13] == b"P5\n23 11\n255\n" and len(raw) == 13 + 23 * 11
    open(prefix + image, "wb").write(raw[:13].replace(*change) + raw[13:])
    with pytest.raises(RuntimeError, match="is not an image of the window of"):
        host.read_costmap(prefix)
    open(prefix + image, "wb").write(raw)
    assert np.array_equal(host.read_costmap(prefix)["cost"], want["cost"])


# ---- the command line ---------------------------------------------------------------------------------------------------------------
def test_the_command_line_refuses_before_a_device_is_asked_for(tmp_path):
    run = lambda *a: subprocess.run([CLI, *a], capture_output=True, text=True, timeout=60)
    kf = str(tmp_path / "nowhere.kf")
    assert run("--build-costmap", kf).returncode == 2                             # no output prefix
    r = run("--build-costmap", kf, str(tmp_path / "x"), "--build-traversability", kf, str(tmp_path / "y"))
    assert r.returncode == 2 and "--build-costmap takes" in r.stderr
    assert run("--build-costmap", kf, str(tmp_path / "x"), "--devices", "0,1").returncode == 2     # one device
    r = run("--build-costmap", kf, str(tmp_path / "x"))
    assert r.returncode == 1 and "nowhere.kf" in r.stderr
    pipeline = tmp_path / "p.yaml"
    pipeline.write_text(block(inflation_radius=0.1))
    r = run("--build-costmap", kf, str(tmp_path / "x"), "-c", str(pipeline))
    assert r.returncode == 1 and "costmap: inflation_radius" in r.stderr and "nowhere" not in r.stderr
    assert "--build-costmap KEYFRAMES OUT_PREFIX" in run("--help").stderr + run("--help").stdout
    assert not os.path.exists(str(tmp_path / "x.pgm"))


# ---- the restatement's own properties -----------------------------------------------------------------------------------------------
def _distance_by_rings(base, Rc, unknown):
    """another formulation: grow the obstacle set offset by offset, in ascending dx^2 + dy^2"""
    ob = R.obstacles(base, unknown)
    ny, nx = ob.shape
    out = np.full((ny, nx), R.FAR, np.int64)
    offsets = sorted((dx * dx + dy * dy, dx, dy) for dx in range(-Rc, Rc + 1) for dy in range(-Rc, Rc + 1) if dx * dx + dy * dy <= Rc * Rc)
    for d2, dx, dy in reversed(offsets):                                          # descending, so that the smallest is written last
        ys, xs = np.nonzero(ob)
        u, v = xs + dx, ys + dy
        ok = (u >= 0) & (u < nx) & (v >= 0) & (v < ny)
        out[v[ok], u[ok]] = np.minimum(out[v[ok], u[ok]], d2)
    return out.astype(np.uint16)


@pytest.mark.parametrize("shape", [(1, 1), (9, 33), (70, 1), (64, 48)])
def test_the_brute_force_distance_is_the_ring_formulation_s(shape):
    nx, ny = shape
    for seed, Rc in enumerate((0, 1, 2, 8, 30)):
        base = nc.random_base(nx, ny, seed, lethal=0.03, unknown=0.03)
        for unknown in (False, True):
            assert np.array_equal(R.distance2(base, Rc, unknown), _distance_by_rings(base, Rc, unknown)), (shape, Rc, unknown)
    many = nc.random_base(64, 48, 77, lethal=0.0005)                              # both ways through distance2 give the same
    assert np.array_equal(R.distance2(many, 30, chunk=1), R.distance2(many, 30))


def test_the_dilation_loop_is_the_walk_from_the_seeds():
    rng = np.random.default_rng(5)
    for k, b in enumerate([nc.serpentine(17), nc.diagonal_touch(), nc.wall(30, 9, 12, 4), nc.wall(30, 9, 12), nc.random_base(40, 30, 1, lethal=0.3)]):
        seeds = rng.integers(-2, 32, (6, 2))
        for below in (1, 253, 254):
            got, info = R.reach(b, seeds, below)
            assert np.array_equal(got, R.components_of(b, seeds, below)), k
            assert info["n_reached"] == int(got.sum())
    assert R.reach(nc.serpentine(17), [[0, 0]], 253)[0][16].all()
    assert not R.reach(nc.diagonal_touch(), [[2, 2]], 253)[0][6:, 6:].any()


def test_the_scenario_s_geometry():
    """what the issue states about the outdoor scenario, on the restatement alone: the window, the fourth key-frame 8 cells from the
    box, and which key-frames a vehicle of 1 m and of 2 m radius reaches from the first"""
    import elev_cases as ec
    import elev_ref as ER
    frames, _ = ec.scenario()
    src = ER.build(frames, **ec.SCENARIO_OPTIONS_DICT)
    assert (src["nx"], src["ny"], src["cells_lethal"], src["cells_unknown"]) == (404, 54, 626, 2816)
    poses = [T for _, T in frames]
    for unknown in (False, True):
        c = R.build(src["cost"], src["x0"], src["y0"], 0.2, poses, inscribed_radius=1.0, inflation_radius=2.0, unknown_is_obstacle=unknown,
                    reach_from="first")
        assert c["keyframes_blocked"] == 0 and c["keyframe_reached"] == [1] * 12 and c["keyframe_d2"][3] == 64
    c = R.build(src["cost"], src["x0"], src["y0"], 0.2, poses, inscribed_radius=2.0, inflation_radius=3.0, unknown_is_obstacle=True, reach_from="first")
    print("2 m, unknown cells obstacles: reached cells", c["cells_reached"])
    assert c["keyframe_cost"][3] >= 253 and [k for k, r in enumerate(c["keyframe_reached"]) if r] == [0, 1, 2]
    c = R.build(src["cost"], src["x0"], src["y0"], 0.2, poses, inscribed_radius=2.0, inflation_radius=3.0, unknown_is_obstacle=False, reach_from="first")
    assert [k for k, r in enumerate(c["keyframe_reached"]) if not r] == [3]
