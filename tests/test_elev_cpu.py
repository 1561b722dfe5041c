"""The elevation and traversability map of a recorded session, the parts that need no device: the traversability: options and every
refusal by name, the host rule on hand-made planes against tests/elev_ref.py -- exactly --, the four files and their round trip, and
the restatement's own properties, on which the device tests of tests/test_gpu_elev.py rest:

 * the two point passes do not depend on the order of the frames nor on how they are split into calls;
 * the separable relief equals the definition's double loop;
 * the scenario of tests/elev_cases.py, the restatement alone (slope window of one cell): road 9 451, under the deck 1 824, ramp 3 724,
   sidewalk 2 384, box 9 and kerb 596 interior cells, none of which disagrees with the class the geometry gives -- inside the
   condition of at most 1 % per region."""
import os

import numpy as np
import pytest

import elev_cases as ec
import elev_ref as R

F = np.float32


@pytest.fixture(scope="module")
def host():
    from mola_lidar_odometry_amd import _mp2p_icp_hip as H
    return H


# ---- options -----------------------------------------------------------------------------------------------------------------------
def test_the_defaults_and_the_derived_integers(host):
    o = host.traversability_options()
    for k, v in R.DEFAULTS.items():
        assert o[k] == v, k
    assert (o["clearance_q"], o["step_q"], o["rise_q"]) == R.derived(R.DEFAULTS) == (200, 15, 14)
    text = ("traversability:\n  resolution: 0.25\n  z_quantum: 0.02\n  max_range: 60\n  vehicle_height: 1.5\n  max_step: 0.1\n  slope_radius_cells: 4\n"
            "  max_slope_deg: 30\n  min_points_per_cell: 1\n  min_obstacle_points: 5\n  target_map: points\n  margin_cells: 0\n")
    want = dict(resolution=0.25, z_quantum=0.02, max_range=60.0, vehicle_height=1.5, max_step=0.1, slope_radius_cells=4, max_slope_deg=30.0,
                min_points_per_cell=1, min_obstacle_points=5, target_map="points", margin_cells=0)
    o = host.traversability_options(text)
    for k, v in want.items():
        assert o[k] == v, k
    assert (o["clearance_q"], o["step_q"], o["rise_q"]) == R.derived(want)
    assert host.traversability_options("occupancy_grid:\n  resolution: 0.1\n")["resolution"] == 0.20     # another block is not this one


@pytest.mark.parametrize("key,value", [("resolution", 0), ("resolution", -1), ("resolution", "inf"), ("resolution", "coarse"), ("z_quantum", 0),
                                       ("z_quantum", "nan"), ("max_range", -1), ("max_range", "inf"), ("vehicle_height", 0), ("vehicle_height", 1e9),
                                       ("max_step", -0.1), ("max_step", 1e9), ("slope_radius_cells", 0), ("slope_radius_cells", 5),
                                       ("slope_radius_cells", 1.5), ("max_slope_deg", 0), ("max_slope_deg", 90), ("max_slope_deg", "nan"),
                                       ("min_points_per_cell", 0), ("min_points_per_cell", -2), ("min_obstacle_points", 0),
                                       ("margin_cells", -1), ("margin_cells", 100000), ("no_such_key", 1), ("zquantum", 0.01)])
def test_a_bad_value_or_an_unknown_key_is_refused_by_name(host, key, value):
    with pytest.raises(RuntimeError, match=r"traversability: %s\b" % key):
        host.traversability_options("traversability:\n  %s: %s\n" % (key, value))


def test_a_set_without_points_or_an_unknown_target_is_refused_before_a_device_is_asked_for(host):
    maps = [dict(name="localmap", class_name="HashedVoxelPointCloud", params=ec.scenario()[1]["maps"][0]["params"], remove_voxels_farther_than=0.0)]
    empty = dict(maps=maps, frames=[dict(timestamp=1.0, pose=ec.I12.tolist(), cov=[0.0] * 36, twist=None, layers=[(0, np.zeros((0, 3), F))])])
    with pytest.raises(RuntimeError, match="hold no points"):
        host.build_traversability_map(empty)
    with pytest.raises(RuntimeError, match="target_map 'other'"):
        host.build_traversability_map(empty, "traversability:\n  target_map: other\n")
    with pytest.raises(RuntimeError, match="names no target map"):
        host.build_traversability_map(dict(maps=[], frames=[]))


def test_without_a_device_the_host_path_raises_too(host):
    from mola_lidar_odometry_amd import capi
    if capi.device_count() == 0:
        with pytest.raises(RuntimeError):                     # nothing falls back to the host
            host.build_traversability_map(ec.scenario()[1])


# ---- the host rule -----------------------------------------------------------------------------------------------------------------
def _classify(host, count, obstacle, r1, rR, step_q=15, rise_q=14, min_points=2, min_obstacle=2, ground=None, q=0.01):
    count = np.asarray(count, np.uint32)
    ground = np.zeros(count.shape, np.int32) if ground is None else np.asarray(ground, np.int32)
    got = host.traversability_classify(ground, count, np.asarray(obstacle, np.uint32), np.asarray(r1, np.int32), np.asarray(rR, np.int32), step_q,
                                       rise_q, min_points, min_obstacle, q)
    want = R.classify(count, obstacle, r1, rR, step_q, rise_q, min_points, min_obstacle)
    assert got[0].dtype == np.uint8 and np.array_equal(got[0], want)
    assert (got[2], got[3], got[4]) == (int((want == 254).sum()), int((want < 254).sum()), int((want == 255).sum()))
    return got


def test_every_lethal_cause_alone_the_cost_at_its_ends_and_unknown(host):
    #            unknown  free@0  obstacle  step  slope  step at its bound  slope at its bound  both at their bounds  one point short
    count =    [[1,       2,      2,        2,    2,     2,                 2,                  2,                    0]]
    obstacle = [[9,       0,      2,        1,    1,     0,                 1,                  1,                    0]]
    r1 =       [[R.NONE,  0,      0,        16,   0,     15,                0,                  15,                   R.NONE]]
    rR =       [[R.NONE,  0,      0,        16,   15,    0,                 14,                 14,                   R.NONE]]
    cost = _classify(host, count, obstacle, r1, rR)[0][0].tolist()
    assert cost == [255, 0, 254, 254, 254, 252 * 15 // 16, 252 * 14 // 15, max(252 * 15 // 16, 252 * 14 // 15), 255]
    assert cost[5] == 236 and cost[6] == 235
    # the cost formula over its whole range, both terms, and zero thresholds
    r = np.arange(0, 16)[None, :]
    c = _classify(host, np.full_like(r, 5), np.zeros_like(r), r, np.zeros_like(r))[0][0]
    assert c.tolist() == [252 * k // 16 for k in range(16)] and c.max() < 252
    r = np.arange(0, 15)[None, :]
    c = _classify(host, np.full_like(r, 5), np.zeros_like(r), np.zeros_like(r), r)[0][0]
    assert c.tolist() == [252 * k // 15 for k in range(15)]
    c = _classify(host, [[3, 3]], [[0, 0]], [[0, 1]], [[0, 0]], step_q=0, rise_q=0)[0][0]
    assert c.tolist() == [0, 254]
    # min_obstacle_points and min_points_per_cell at their edges
    assert _classify(host, [[3, 3, 3]], [[2, 3, 4]], [[0] * 3], [[0] * 3], min_points=3, min_obstacle=3)[0][0].tolist() == [0, 254, 254]
    assert _classify(host, [[2, 3]], [[0, 0]], [[R.NONE, 0]], [[R.NONE, 0]], min_points=3)[0][0].tolist() == [255, 0]


def test_random_planes_and_the_heights(host):
    rng = np.random.default_rng(3)
    for trial in range(20):
        ny, nx = rng.integers(1, 40, 2)
        count = rng.integers(0, 6, (ny, nx))
        obstacle = rng.integers(0, 4, (ny, nx))
        ground = rng.integers(-5000, 5000, (ny, nx))
        known = count >= 2
        r1 = np.where(known, rng.integers(0, 30, (ny, nx)), R.NONE)
        rR = np.where(known, rng.integers(0, 30, (ny, nx)), R.NONE)
        q = [0.01, 0.05, 0.013][trial % 3]
        got = _classify(host, count, obstacle, r1, rR, ground=ground, q=q)
        assert got[1].dtype == F and got[1].tobytes() == R.height_bytes(ground, count, 2, q)
    with pytest.raises(RuntimeError, match="ny \\* nx entries"):
        host.traversability_classify(np.zeros((2, 2), np.int32), np.zeros((2, 2), np.uint32), np.zeros((2, 2), np.uint32), np.zeros((2, 2), np.int32),
                                     np.zeros((2, 1), np.int32), 15, 14)


# ---- the files ---------------------------------------------------------------------------------------------------------------------
def _hand_map(x0=-7, y0=3, q=0.01):
    cost = np.array([[255, 0, 17, 254], [251, 254, 255, 1], [0, 0, 0, 0]], np.uint8)
    ground = np.array([[0, -3, 120, 4], [9, 9, 0, -250], [1, 2, 3, 4]], np.int32)
    count = np.where(cost == 255, 0, 5)
    height = np.frombuffer(R.height_bytes(ground, count, 2, q), "<f4").reshape(cost.shape)
    return dict(x0=x0, y0=y0, nx=4, ny=3, resolution=0.2, z_quantum=q, cost=cost, height=height), ground, count


def test_the_four_files_are_the_restatement_s_bytes_and_read_back_to_the_same_bytes(host, tmp_path):
    m, ground, count = _hand_map()
    m["cost"][-1, :3] = (10, 32, 9)                # the image's first pixels are white space to a careless header parser
    prefix = str(tmp_path / "hill")
    host.write_traversability_map(m, prefix)
    files = {s: open(prefix + s, "rb").read() for s in (".pgm", ".yaml", "_cost.pgm", "_height.f32")}
    assert files[".pgm"] == R.trinary_pgm_bytes(m["cost"])
    assert files[".yaml"].decode() == R.yaml_text("hill", 0.2, -7, 3, 0.01)
    assert files["_cost.pgm"] == R.cost_pgm_bytes(m["cost"])
    assert files["_height.f32"] == R.height_bytes(ground, count, 2, 0.01) and len(files["_height.f32"]) == 48
    assert np.isnan(np.frombuffer(files["_height.f32"], "<f4")[[0, 6]]).all() and np.frombuffer(files["_height.f32"], "<f4")[2] == F(1.2)
    back = host.read_traversability_map(prefix)
    assert (back["x0"], back["y0"], back["nx"], back["ny"], back["resolution"], back["z_quantum"]) == (-7, 3, 4, 3, 0.2, 0.01)
    assert np.array_equal(back["cost"], m["cost"]) and back["height"].tobytes() == m["height"].tobytes()
    assert (back["cells_lethal"], back["cells_free"], back["cells_unknown"]) == (2, 8, 2)
    assert back["ground"].size == 0 and back["relief1"].size == 0            # (the planes are not in the files)
    again = str(tmp_path / "again")
    host.write_traversability_map(back, again)
    for s, b in files.items():
        assert open(again + s, "rb").read() == (b if s != ".yaml" else R.yaml_text("again", 0.2, -7, 3, 0.01).encode()), s
    # the trinary pair is g12's: its reader takes it
    g = host.read_occupancy_grid(prefix)
    assert (g["x0"], g["y0"], g["nx"], g["ny"]) == (-7, 3, 4, 3)
    assert np.array_equal(g["cells"], np.where(m["cost"] == 254, 100, np.where(m["cost"] == 255, -1, 0)))


@pytest.mark.parametrize("v", [9, 10, 11, 12, 13, 32])
def test_a_cost_image_whose_first_pixel_is_white_space_reads_back(host, tmp_path, v):
    m, _, _ = _hand_map()
    m["cost"][-1, 0] = v                           # (the largest y, column 0: the byte behind the header)
    prefix = str(tmp_path / "m")
    host.write_traversability_map(m, prefix)
    raw = open(prefix + "_cost.pgm", "rb").read()
    assert raw == R.cost_pgm_bytes(m["cost"]) and raw[:11] == b"P5\n4 3\n255\n" and raw[11] == v
    back = host.read_traversability_map(prefix)
    assert back["cost"].tobytes() == m["cost"].tobytes() and back["height"].tobytes() == m["height"].tobytes()
    assert (back["cells_lethal"], back["cells_free"], back["cells_unknown"]) == (2, 8, 2)


@pytest.mark.parametrize("header", [b"P5\n4 3\n255 ", b"P5\n4 3\n255\n\n", b"P5\n4 3\n254\n", b"P5\n3 4\n255\n", b"P5\n4 4\n255\n"])
def test_a_cost_image_whose_header_is_not_the_writer_s_is_refused(host, tmp_path, header):
    m, _, _ = _hand_map()
    prefix = str(tmp_path / "m")
    host.write_traversability_map(m, prefix)
    raw = open(prefix + "_cost.pgm", "rb").read()
    assert raw[:11] == b"P5\n4 3\n255\n"
    open(prefix + "_cost.pgm", "wb").write(header + raw[11:])
    with pytest.raises(RuntimeError, match="is not the cost image of"):
        host.read_traversability_map(prefix)
    open(prefix + "_cost.pgm", "wb").write(raw)
    assert np.array_equal(host.read_traversability_map(prefix)["cost"], m["cost"])


def test_the_reader_and_the_writer_refuse_what_they_cannot_take(host, tmp_path):
    m, _, _ = _hand_map()
    with pytest.raises(RuntimeError, match="nowhere"):
        host.read_traversability_map(str(tmp_path / "nowhere"))
    with pytest.raises(RuntimeError, match="cannot write"):
        host.write_traversability_map(m, str(tmp_path / "no_such_dir" / "m"))
    with pytest.raises(RuntimeError, match="holds no cells"):
        host.write_traversability_map(dict(m, cost=m["cost"][:2]), str(tmp_path / "short"))
    prefix = str(tmp_path / "m")
    host.write_traversability_map(m, prefix)
    raw = open(prefix + "_height.f32", "rb").read()
    open(prefix + "_height.f32", "wb").write(raw[:-1])
    with pytest.raises(RuntimeError, match="m_height.f32"):
        host.read_traversability_map(prefix)
    open(prefix + "_height.f32", "wb").write(raw)
    raw = open(prefix + "_cost.pgm", "rb").read()
    open(prefix + "_cost.pgm", "wb").write(raw[:-2] + b"\xfe" + raw[-1:])  # lethal in the cost image, free (17) in the trinary one
    with pytest.raises(RuntimeError, match="disagrees"):
        host.read_traversability_map(prefix)
    open(prefix + "_cost.pgm", "wb").write(raw)
    g12 = str(tmp_path / "g12")                                             # a plain occupancy grid is not a traversability map
    host.write_occupancy_grid(dict(x0=0, y0=0, nx=4, ny=3, resolution=0.2, cells=np.zeros((3, 4), np.int8)), g12)
    with pytest.raises(RuntimeError, match="lacks cost_image"):
        host.read_traversability_map(g12)


# ---- the restatement's own properties ----------------------------------------------------------------------------------------------
def _planes(m):
    return [a.copy() for a in m.download()] + [dict(m.info)]


def _same(a, b):
    for x, y in zip(a[:4], b[:4]):
        assert np.array_equal(x, y)
    assert a[4] == b[4]


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_passes_depend_neither_on_frame_order_nor_on_how_the_frames_are_split(seed):
    frames = ec.random_frames([65, 0, 257, 64, 1, 700], seed) + ec.wild_frames(seed)
    w = dict(zip(("x0", "y0", "nx", "ny"), ec.window_of(frames, margin=-8)))       # (a window that cuts points off on every side)
    kw = dict(resolution=ec.RES, z_quantum=0.01, max_range=3.5, clearance_q=200, step_q=15, **w)
    base = _planes(R.ElevRef(**kw).add_frames(frames).mark_frames(frames))
    assert base[4]["n_left_out"] > 0 and base[4]["n_outside_window"] > 0 and base[2].sum() > 0 and (base[1] > 1).any()
    rng = np.random.default_rng(seed)
    order = rng.permutation(len(frames))
    shuffled = [frames[k] for k in order]
    m = R.ElevRef(**kw)
    for f in shuffled:                                   # one call per frame, another order, the mark pass in yet another
        m.add_frames([f])
    for f in shuffled[::-1]:
        m.mark_frames([f])
    _same(base, _planes(m))
    halves = [(x[:len(x) // 2], T) for x, T in frames] + [(x[len(x) // 2:], T) for x, T in frames]   # frames cut in two
    _same(base, _planes(R.ElevRef(**kw).add_frames(halves).mark_frames(halves)))


@pytest.mark.parametrize("radius", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("min_points", [1, 3])
def test_the_separable_relief_is_the_double_loop(radius, min_points):
    rng = np.random.default_rng(10 * radius + min_points)
    for ny, nx in [(1, 1), (1, 70), (33, 9), (20, 23)]:
        count = rng.integers(0, 5, (ny, nx))
        ground = np.where(count > 0, rng.integers(-300, 300, (ny, nx)), R.GROUND_EMPTY)
        got = R.relief(ground, count, radius, min_points)
        assert np.array_equal(got, R.relief_brute(ground, count, radius, min_points))
        assert ((got == R.NONE) == (count < min_points)).all() and (got[count >= min_points] >= 0).all()
        if radius == 0:
            assert (got[count >= min_points] == 0).all()


def test_the_edge_points_fall_where_fp32_puts_them():
    (xyz, T), = ec.edge_points()
    ok, ix, iy, zq = R.point_rule(xyz, T, ec.RES, 0.01, 0.0)
    assert ok.all()
    inv, invq = F(1) / F(ec.RES), F(1) / F(0.01)
    assert np.array_equal(ix, np.floor((xyz[:, 0] * inv).astype(np.float64))) and np.array_equal(zq, np.floor((xyz[:, 2] * invq).astype(np.float64)))
    assert len(set(zip(ix.tolist(), iy.tolist()))) > 20 and len(np.unique(zq)) > 10           # ... on both sides of many edges
    m = R.ElevRef(x0=0, y0=0, nx=2, ny=1).add_frames(ec.height_steps()).mark_frames(ec.height_steps())
    g, c, o, t = m.download()
    assert g.tolist() == [[0, 0]] and c.tolist() == [[3, 3]] and o.tolist() == [[1, 1]] and t.tolist() == [[200, 16]]


# ---- the scenario, the restatement alone -------------------------------------------------------------------------------------------
def test_the_restatement_reads_the_scenario_as_its_geometry_says():
    frames, kfset = ec.scenario()
    assert len(frames) == ec.N_POSES == 12 and sum(len(x) for x, _ in frames) == 642017
    g = R.build(frames, **ec.SCENARIO_OPTIONS_DICT)
    assert (g["clearance_q"], g["step_q"], g["rise_q"]) == (200, 15, 7)
    shares = ec.scenario_disagreement(g)
    assert {k: v[0] for k, v in shares.items()} == dict(road=9451, under_deck=1824, ramp=3724, sidewalk=2384, box=9, kerb=596)
    for name, (n, wrong) in shares.items():
        assert wrong * 100 <= n, (name, n, wrong)                              # the condition: at most 1 % per region
    regions = ec.scenario_regions(g)
    assert set(np.unique(g["ground"][regions["road"][0]]).tolist()) <= {ec.ROAD_Q - 1, ec.ROAD_Q}
    assert set(np.unique(g["ground"][regions["sidewalk"][0]]).tolist()) <= {ec.ROAD_Q + 19, ec.ROAD_Q + 20}
    assert g["relief1"][regions["ramp"][0]].max() <= 7 and g["obstacle_count"][regions["box"][0]].min() >= 2
    assert (g["top"][regions["under_deck"][0]] <= ec.ROAD_Q).all()                     # the deck is overhead: it never became a top
    assert g["info"]["n_left_out"] == 0 and g["info"]["n_outside_window"] == 0 and g["info"]["n_counted"] == 642017
