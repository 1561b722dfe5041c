"""The references of tests/test_gpu_far_session.py are sound far from the origin, shown with no device (tests/far_session_cases.py:
recorded sessions whose poses are shifted by D1 = 4 km, D2 = 52 km, D3 = 410 km, or turned by 0.7 rad about z and shifted): the
cleaning restatement gives the origin's votes word for word under a pure shift and keeps the scenario's two conditions under the
turn, where the ties of the neighbour rule at exactly max_view_distance flip; the live fold keeps tests/test_live_cpu.py's
condition at every offset; the occupancy and the elevation restatements leave out, at the end of the key range, exactly the points
an exhaustive fp32 count names; and the three grid-file writers give back x0, y0 and every byte for windows out to +-9e5 cells.
The printed counts are recorded in profiles/far_origin.md."""
import numpy as np
import pytest

import clean_cases as cc
import clean_ref as cr
import elev_ref as ER
import far_session_cases as fs
import live_cases as lc
import nav_ref as NR
import occgrid_ref as G
import occmap_ref as R
from test_live_cpu import _condition

F = np.float32
NAMES = list(fs.OFFSETS)


@pytest.fixture(scope="module")
def host():
    from mola_lidar_odometry_amd import _mp2p_icp_hip as H
    return H


# ---- clean_ref.clean on the street ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def street():
    """the scenario and the restatement's run at the origin, computed once"""
    sc = cc.scenario()
    assert len(sc["sweeps"]) == 20 and sum(len(s) for s in sc["sweeps"]) == 366242
    masks, votes, nb = cr.clean(sc["sweeps"], sc["poses"])
    return dict(sc=sc, masks=masks, votes=votes, nb=nb)


@pytest.mark.parametrize("name", NAMES)
def test_a_shifted_street_gets_the_origin_s_votes_word_for_word(street, name):
    """A pure shift leaves R as it was.  The street's translations are whole metres apart and, with D added, lie in one fp64 binade
    at each offset: they carry the same rounding, t_i - t_j is the origin's exactly, and so are the relative poses and the ties at
    30 m.  Measured: 0 differing vote words, masks and lists at D1, D2 and D3.  Asserted: equality."""
    sc = street["sc"]
    masks, votes, nb = cr.clean(sc["sweeps"], fs.move_poses(sc["poses"], fs.OFFSETS[name]))
    print("%s shifted: %d differing vote words, %d differing masks, %d differing neighbour lists" % (
        name, fs.words_differing(votes, street["votes"]), fs.words_differing(masks, street["masks"]),
        sum(a != b for a, b in zip(nb, street["nb"]))))
    assert nb == street["nb"]
    assert all(np.array_equal(a, b) for a, b in zip(votes, street["votes"]))
    assert all(np.array_equal(a, b) for a, b in zip(masks, street["masks"]))


@pytest.mark.parametrize("name", ["O"] + NAMES)
def test_a_turned_street_keeps_its_two_conditions_and_flips_a_tie(street, name):
    """Turned by 0.7 (at the origin and at every offset) the distance of two key-frames 30 m apart is a rounded sum of squares: the
    ties of the neighbour rule flip.  Measured over O, D1, D2, D3: 16 to 86 masks differ from the unturned run; 9 761 to 9 763 of
    9 790 mover points and 377 to 439 of 356 452 others go.  Asserted: the two conditions of
    test_clean_cpu.py::test_the_scenario_meets_its_two_conditions_with_the_default_options, unchanged, and that at least one
    neighbour list differs -- the tie tests/test_gpu_far_session.py has to see."""
    sc = street["sc"]
    D = fs.ORIGIN if name == "O" else fs.OFFSETS[name]
    masks, votes, nb = cr.clean(sc["sweeps"], fs.move_poses(sc["poses"], D, fs.YAW))
    mv, rm = np.concatenate(sc["mover"]), np.concatenate(masks)
    lists = sum(a != b for a, b in zip(nb, street["nb"]))
    print("%s turned: %d neighbour lists and %d masks differ from the unturned run; mover points %d, removed %d; others %d, removed %d" % (
        name, lists, fs.words_differing(masks, street["masks"]), int(mv.sum()), int((mv & rm).sum()), int((~mv).sum()), int((~mv & rm).sum())))
    assert (mv & rm).sum() >= 0.90 * mv.sum()
    assert (~mv & rm).sum() <= 0.01 * (~mv).sum()
    assert lists >= 1


# ---- live_cases.fold on the street ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["O"] + NAMES)
def test_the_live_fold_keeps_its_condition_at_every_offset(oracle, name):
    """measured (mover points left plain / cleaned, others erased of others in all): O 1 654 / 13, 518 of 107 576; D1 1 876 / 13,
    549 of 80 558; D2 1 965 / 12, 576 of 83 062; D3 1 659 / 13, 527 of 107 509 -- the voxel faces fall elsewhere among the points at
    every offset, so the cap of 20 keeps other points"""
    s = cc.scenario()
    D = fs.ORIGIN if name == "O" else fs.OFFSETS[name]
    print(name, end=" ")
    _condition(s["sweeps"], fs.move_poses(s["poses"], D), s["mover"])


# ---- the end of the key range --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", [r for _, r in fs.OCC_CASES])
def test_the_occupancy_restatement_leaves_out_what_an_exhaustive_count_names(res):
    """poses at x = (1e6 - 40) * resolution: a point is left out when |p * (1 / res)| >= 1e6 holds in fp32 on any axis"""
    frames = fs.limit_frames(res)
    ref = R.OccMapRef(resolution=res)
    left = want = total = 0
    for xyz, T in frames:
        if len(xyz) == 0:
            continue
        ref.insert(xyz, T)
        left += ref.n_left_out
        inv = F(1.0) / F(res)
        for p in fs.composed(xyz, T):
            want += int(any(not (abs(F(c) * inv) < F(1.0e6)) for c in p))
        total += len(xyz)
    print("occupancy, resolution %g: %d of %d points left out" % (res, left, total))
    assert left == want and 0 < want < total
    keys = ref.download()[0]
    assert keys[:, 0].max() == 999999 and np.abs(keys).max() < 1000000


@pytest.mark.parametrize("res", [r for _, r in fs.ELEV_CASES])
def test_the_elevation_restatement_leaves_out_what_an_exhaustive_count_names(res):
    """molahip_elevation.h, step 3: left out when |Px * inv| >= 1e6 or |Py * inv| >= 1e6 or |Pz * invq| >= 2^30 in fp32 (no point of
    these frames is non-finite or beyond a max_range: n_left_out counts step 3 alone)"""
    frames = fs.limit_frames(res)
    x0, y0, nx, ny = fs.window_of(frames, res)
    ref = ER.ElevRef(resolution=res, x0=x0, y0=y0, nx=nx, ny=ny).add_frames(frames)
    inv, invq = F(1.0) / F(res), F(1.0) / F(0.01)
    want = 0
    for xyz, T in frames:
        for p in fs.composed(xyz, T):
            want += int(not (abs(p[0] * inv) < F(1.0e6)) or not (abs(p[1] * inv) < F(1.0e6)) or not (abs(p[2] * invq) < F(1073741824.0)))
    total = sum(len(x) for x, _ in frames)
    print("elevation, resolution %g: %d of %d points left out, %d outside the window" % (res, ref.info["n_left_out"], total, ref.info["n_outside_window"]))
    assert ref.info["n_left_out"] == want and 0 < want < total
    assert ref.info["n_outside_window"] == 0 and ref.info["n_counted"] == total - want
    assert ref.count[:, 1000000 - x0:].sum() == 0 and ref.count[:, 999999 - x0].sum() > 0
    lo, hi, n_in = ER.bounds(frames, res)
    assert hi[0] == 999999 and n_in == total - want


# ---- the files -----------------------------------------------------------------------------------------------------------------------
def test_grid_files_give_back_far_windows_and_every_byte(host, tmp_path):
    """a few hundred random (x0, y0) in +-9e5 cells at every resolution of the list, through the three writers and their readers"""
    rng = np.random.default_rng(2024)
    for trial in range(300):
        res = fs.FILE_RESOLUTIONS[trial % len(fs.FILE_RESOLUTIONS)]
        x0, y0 = (int(v) for v in rng.integers(-900000, 900001, 2))
        if trial < 12:                                               # the corners of the range and the values next to them
            x0, y0 = [(900000, -900000), (-900000, 899999), (899999, 900000), (-899999, -899999)][trial % 4]
        nx, ny = (int(v) for v in rng.integers(1, 9, 2))
        prefix = str(tmp_path / ("g%d" % trial))
        name = "g%d" % trial
        # the occupancy grid
        cells = rng.choice(np.array([G.FREE, G.OCCUPIED, G.UNKNOWN], np.int8), (ny, nx))
        host.write_occupancy_grid(dict(x0=x0, y0=y0, nx=nx, ny=ny, resolution=res, cells=cells), prefix)
        assert open(prefix + ".pgm", "rb").read() == G.pgm_bytes(cells)
        assert open(prefix + ".yaml").read() == G.yaml_text(name + ".pgm", res, x0, y0)
        back = host.read_occupancy_grid(prefix)
        assert (back["x0"], back["y0"], back["nx"], back["ny"], back["resolution"]) == (x0, y0, nx, ny, res), (trial, res, x0, y0)
        assert np.array_equal(back["cells"], cells)
        # the traversability map
        cost = rng.integers(0, 256, (ny, nx)).astype(np.uint8)
        cost[(cost == 252) | (cost == 253)] = 251                    # (this product writes 0 .. 251, 254 and 255; its reader refuses the rest)
        ground = rng.integers(-5000, 5000, (ny, nx))
        count = np.where(cost == 255, 0, 5)
        height = np.frombuffer(ER.height_bytes(ground, count, 2, 0.01), "<f4").reshape(ny, nx)
        prefix_t = prefix + "t"
        host.write_traversability_map(dict(x0=x0, y0=y0, nx=nx, ny=ny, resolution=res, z_quantum=0.01, cost=cost, height=height), prefix_t)
        assert open(prefix_t + ".yaml").read() == ER.yaml_text(name + "t", res, x0, y0, 0.01)
        assert open(prefix_t + ".pgm", "rb").read() == ER.trinary_pgm_bytes(cost) and open(prefix_t + "_cost.pgm", "rb").read() == ER.cost_pgm_bytes(cost)
        back = host.read_traversability_map(prefix_t)
        assert (back["x0"], back["y0"], back["nx"], back["ny"], back["resolution"]) == (x0, y0, nx, ny, res), (trial, res, x0, y0)
        assert np.array_equal(back["cost"], cost) and back["height"].tobytes() == height.tobytes()
        # the costmap
        reach = rng.integers(0, 2, (ny, nx)).astype(np.uint8)
        cmap = rng.integers(0, 256, (ny, nx)).astype(np.uint8)
        prefix_c = prefix + "c"
        host.write_costmap(dict(x0=x0, y0=y0, nx=nx, ny=ny, resolution=res, max_cells=3, inscribed_radius=0.5, inflation_radius=1.5,
                                d2=np.zeros((ny, nx), np.uint16), cost=cmap, reach=reach), prefix_c)
        assert open(prefix_c + ".yaml").read() == NR.yaml_text(name + "c", res, x0, y0, 0.5, 1.5)
        assert open(prefix_c + ".pgm", "rb").read() == NR.trinary_pgm_bytes(cmap) and open(prefix_c + "_cost.pgm", "rb").read() == NR.cost_pgm_bytes(cmap)
        assert open(prefix_c + "_reach.pgm", "rb").read() == NR.reach_pgm_bytes(reach)
        back = host.read_costmap(prefix_c)
        assert (back["x0"], back["y0"], back["nx"], back["ny"], back["resolution"]) == (x0, y0, nx, ny, res), (trial, res, x0, y0)
        assert np.array_equal(back["cost"], cmap) and np.array_equal(back["reach"], reach)
