"""The parts of include/molahip_replan.h and mola_lidar_odometry_hip/Replan.h that need no device.  The update rule: withdrawing what
lies outside the largest self-supporting set and relaxing from the rest gives Dijkstra's field on the new plane (tests/replan_ref.py
against tests/plan_ref.py), which is what keeps the n_withdrawn that the device tests compare with honest; lowering-only patches
withdraw nothing.  The host rules: the events text and its refusals, the metre rectangle, the growth and the clipping -- the restatement
and the host layer against it."""
import numpy as np
import pytest

import plan_cases as pc
import plan_ref as R
import replan_ref as RR


def small_cases():
    rng = np.random.default_rng(17)
    for k in range(60):
        nx, ny = int(rng.integers(1, 24)), int(rng.integers(1, 24))
        cost = pc.random_cost(nx, ny, 1000 + k, (0.02, 0.1, 0.25)[k % 3])
        price = (pc.stepped(), pc.flat(), pc.by_cost())[(k // 3) % 3]
        lists = pc.goal_lists(cost, k)
        yield rng, nx, ny, cost, price, lists[k % len(lists)]


def test_withdraw_then_relax_is_dijkstra_on_the_new_plane():
    n_updates = n_withdrawing = 0
    for rng, nx, ny, cost, price, goals in small_cases():
        f, _ = R.field(cost, goals, price)
        for step in range(4):
            w, h = int(rng.integers(1, nx + 1)), int(rng.integers(1, ny + 1))
            x0, y0 = int(rng.integers(0, nx - w + 1)), int(rng.integers(0, ny - h + 1))
            new = (rng.integers(0, 256, (h, w)) if step % 2 == 0 else np.where(rng.random((h, w)) < 0.5, 254, cost[y0:y0 + h, x0:x0 + w])).astype(np.uint8)
            cost, _, repriced = RR.patch(cost, x0, y0, new, price)
            want, _ = R.field(cost, goals, price)
            got, n = RR.repair(f, cost, goals, price)
            assert np.array_equal(got, want), (nx, ny, x0, y0, w, h)
            assert n == RR.n_withdrawn(f, cost, price)
            if repriced == 0:
                assert n == 0
            # what is kept are upper bounds of the new field, and exact where the old value still holds
            K = RR.kept(f, cost, price)
            assert (want[K] <= f[K]).all() and (want[K] != R.UNREACHED).all()
            n_updates += 1
            n_withdrawing += n > 0
            f = want
    assert n_updates == 240 and n_withdrawing >= 40


def test_an_update_that_only_lowers_prices_or_opens_cells_withdraws_nothing():
    for rng, nx, ny, cost, price, goals in small_cases():
        f, _ = R.field(cost, goals, price)
        new = np.where(cost >= 253, rng.integers(0, 253, cost.shape), cost // 2).astype(np.uint8)
        keep = rng.random(cost.shape) < 0.5
        new = np.where(keep, cost, new).astype(np.uint8)
        assert (np.diff(np.asarray(price, np.int64)) >= 0).all()                # (a lower cost byte never has a higher price in these tables)
        assert RR.n_withdrawn(f, new, price) == 0
        got, n = RR.repair(f, new, goals, price)
        assert n == 0 and np.array_equal(got, R.field(new, goals, price)[0])


def test_the_peeling_on_planes_with_a_known_answer():
    b = pc.wall(30, 10, 15, 4)
    f, _ = R.field(b, [[2, 2]], pc.flat())
    closed = b.copy()
    closed[4, 15] = 254
    assert RR.n_withdrawn(f, closed, pc.flat()) == 14 * 10 + 1                 # the far side and the gap cell
    assert RR.n_withdrawn(f, b, pc.flat()) == 0                                # nothing changed: the field supports itself
    d = pc.beside_diagonal()
    opened = d.copy()
    opened[1, 2] = 0
    f, _ = R.field(opened, [[2, 2]], pc.flat())
    K = RR.kept(f, d, pc.flat())
    assert not K[1, 1] and not K[1, 2] and K[2, 1] and K[2, 2]                 # (1, 1) rested on the diagonal step the lethal cell forbids


def test_the_grown_rectangle():
    assert RR.grown_rect(10, 12, 3, 4, 5, 100, 100) == (5, 7, 13, 14)
    assert RR.grown_rect(2, 1, 3, 4, 5, 100, 100) == (0, 0, 10, 10)            # clipped at the low edges
    assert RR.grown_rect(95, 97, 5, 3, 5, 100, 100) == (90, 92, 10, 8)         # ... and at the high ones
    assert RR.grown_rect(0, 0, 1, 1, 0, 1, 1) == (0, 0, 1, 1) and RR.grown_rect(3, 3, 2, 2, 255, 8, 9) == (0, 0, 8, 9)


def test_a_rectangle_in_metres():
    win = dict(x0=-5, y0=-3, nx=12, ny=9, resolution=0.2)
    assert RR.metre_rect(0.0, 0.0, 0.39, 0.19, **win) == (5, 3, 2, 1)          # the floor rule on both corners, inclusive
    assert RR.metre_rect(0.39, 0.19, 0.0, 0.0, **win) == (5, 3, 2, 1)          # the corners in either order
    assert RR.metre_rect(-0.01, -0.01, -0.01, -0.01, **win) == (4, 2, 1, 1)
    assert RR.metre_rect(-100.0, -100.0, 100.0, 100.0, **win) == (0, 0, 12, 9)  # clipped
    assert RR.metre_rect(1.3, 1.1, 50.0, 50.0, **win) == (11, 8, 1, 1)
    assert RR.metre_rect(1.41, 0.0, 50.0, 1.0, **win) is None and RR.metre_rect(0.0, -9.0, 1.0, -0.61, **win) is None     # no cell: not an error
    with pytest.raises(ValueError):
        RR.metre_rect(0.0, 0.0, 3.0e5, 0.0, **win)


EVENTS = """# a lorry parks across the road
block 1 2 3.5 -4e0   # trailing comment

at 0.5 0.25
clear 1 2 3.5 -4
  at\t-1 +2
"""


def test_the_events_text():
    want = [("block", [1.0, 2.0, 3.5, -4.0], 2), ("at", [0.5, 0.25], 4), ("clear", [1.0, 2.0, 3.5, -4.0], 5), ("at", [-1.0, 2.0], 6)]
    assert RR.parse_events(EVENTS) == want
    assert RR.parse_events("") == [] and RR.parse_events("# nothing\n\n") == []
    assert RR.parse_events("at 1 2") == [("at", [1.0, 2.0], 1)]                # no newline at the end
    for bad, line in (("block 1 2 3", 1), ("at 1", 1), ("at 1 2 3", 1), ("\nmove 1 2", 2), ("at 1 two", 1), ("block 1 2 3 nan", 1), ("at inf 0", 1),
                      ("at 0x10 0", 1), ("at 1 2\nblock", 2), ("at 1 2\nclear 1 2 3 4 5", 2), ("BLOCK 1 2 3 4", 1), ("at 1e999 0", 1)):
        with pytest.raises(ValueError) as e:
            RR.parse_events(bad)
        assert "events: line %d" % line in str(e.value), bad


def test_the_host_layer_reads_events_and_rectangles_as_the_restatement():
    from mola_lidar_odometry_amd import _mp2p_icp_hip as H
    got = H.replan_parse_events(EVENTS)
    assert [(e["verb"], e["numbers"], e["line"]) for e in got] == RR.parse_events(EVENTS)
    for bad in ("block 1 2 3", "\nmove 1 2", "at 1 two", "block 1 2 3 nan", "at 0x10 0", "at 1e999 0", "at 1 2\nblock"):
        with pytest.raises(RuntimeError) as e:
            H.replan_parse_events(bad)
        with pytest.raises(ValueError) as r:
            RR.parse_events(bad)
        assert str(r.value).split(":")[1] in str(e.value)                      # the same line is named
    win = dict(x0=-5, y0=-3, nx=12, ny=9, resolution=0.2)
    rng = np.random.default_rng(3)
    for _ in range(200):
        xa, ya, xb, yb = (rng.random(4) * 6 - 3).tolist()
        want = RR.metre_rect(xa, ya, xb, yb, **win)
        assert H.replan_metre_rect(win, xa, ya, xb, yb) == want
        col0, row0, w, h = (int(v) for v in rng.integers(0, 9, 4))
        w, h = min(w + 1, 12 - col0), min(h + 1, 9 - row0)
        m = int(rng.integers(0, 6))
        assert H.replan_grown_rect(col0, row0, w, h, m, 12, 9) == RR.grown_rect(col0, row0, w, h, m, 12, 9)
    with pytest.raises(RuntimeError):
        H.replan_metre_rect(win, 0.0, 0.0, 3.0e5, 0.0)
