"""The stand-alone driver on the lidar2d-shaped pipeline (tests/lidar2d_inline.py): its local map is the occupancy voxel map
(mrpt::maps::CVoxelMap stand-in).  Scans come from an analytic 2-D ray caster (a 10 m x 8 m room with one box, 720 beams,
z = 0).  The driver's wiring of the map -- pose, origin, options, far removal -- is pinned by replaying its own key-frames
through the numpy restatement (tests/occmap_ref.py); the trajectory is held against the generator's exact poses, with the
same drive on a mola::HashedVoxelPointCloud map (voxel 0.25 m, cap 20), which the driver ran before this map existed, as the
yardstick.

Measured on an MI355X (the 30-scan drive; profiles/occmap.md): ATE 0.0267 m with the occupancy map at 0.05 m
(MOLA_HIP_VOXELMAP_UPDATE=counted; 0.0247 m with `once`) against 0.0012 m for the yardstick: the bar, 2 x 0.0012 + 0.05 =
0.0524 m, is met."""
import threading
import time

import numpy as np
import pytest

from mola_lidar_odometry_amd import trajectory

import lidar2d_inline as L2
import occmap_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host():
    from mola_lidar_odometry_amd import _mp2p_icp_hip as H
    return H


@pytest.fixture(scope="module")
def the_drive():
    return L2.drive(30)


def new_driver(host, text):
    lo = host.LidarOdometry(0, True)
    lo.initialize(host.Config.FromYamlText(text))
    return lo


def run(host, text, drv, on_record=None):
    stamps, _, scans = drv
    lo = new_driver(host, text)
    t0 = time.perf_counter()
    for st, xyz in zip(stamps, scans):
        rec = lo.onLidar(float(st), xyz)
        if on_record:
            on_record(lo, rec)
    return lo, len(scans) / (time.perf_counter() - t0)


def ate(lo, drv):
    stamps, poses, _ = drv
    traj = lo.trajectory()
    assert len(traj) >= len(stamps) - 2, "the driver lost track"
    at = [int(np.argmin(np.abs(stamps - t))) for t, _ in traj]
    est = np.array([trajectory.to44(np.array(T)) for _, T in traj])
    return trajectory.ate_rmse(est, poses[at], align="origin")


@pytest.fixture(scope="module")
def voxelmap_run(host, the_drive):
    """The drive on the occupancy map, with the restatement fed the driver's own key-frames on the way."""
    ref = R.OccMapRef(resolution=L2.RESOLUTION)
    updates = []

    def replay(lo, rec):
        if rec["restarted"]:
            ref.clear()
        if rec["map_updated"]:
            layer = lo.downloadLayer("decimated")["xyz"]
            ref.insert(layer, np.array(rec["pose"]), 60.0)
            updates.append(len(layer))

    lo, rate = run(host, L2.pipeline(), the_drive, replay)
    return lo, ref, updates, rate


def test_drive_updates_and_searches_the_occupancy_map(voxelmap_run, the_drive):
    lo, ref, updates, _ = voxelmap_run
    recs = lo.records()
    assert len(recs) == 30 and sum(r["icp_run"] for r in recs) == 29 and all(r["icp_good"] for r in recs if r["icp_run"])
    assert len(updates) >= 5 and all(n > 600 for n in updates)
    assert lo.describePipeline()["icp_path"] == "layers"
    assert lo.profile()["icp.fused_align_calls"] == sum(r["align_calls"] for r in recs)
    sizes = lo.localMapSizes()
    assert sizes == {"localmap": len(ref.centres())} and sizes["localmap"] > 500
    n_pts, n_cells, res = lo.localMapStats()["localmap"]
    assert (n_pts, n_cells) == (len(ref.centres()), len(ref.cells)) and abs(res - 0.05) < 1e-12


def test_replay_of_the_drive_gives_the_driver_s_map_bit_for_bit(voxelmap_run):
    lo, ref, _, _ = voxelmap_run
    v = lo.downloadVoxelMap("localmap")
    rk, rl = ref.download()
    assert v["keys"].shape == rk.shape and np.array_equal(v["keys"], rk)
    assert np.array_equal(v["logodds"], rl)
    assert rl.min() < 0 < ref.l_occ <= rl.max()  # free space was traced, walls were hit
    m = lo.downloadMap("localmap")  # the search structure: the occupied centres, global index = rank in key order
    cen = ref.centres()
    order = np.argsort(m["src_idx"], kind="stable")
    assert np.array_equal(m["src_idx"][order], np.arange(len(cen), dtype=np.uint32))
    assert np.array_equal(np.ascontiguousarray(m["xyz"][order]).view(np.uint32), cen.view(np.uint32))


def test_trajectory_against_the_exact_poses(host, voxelmap_run, the_drive):
    lo, _, _, rate = voxelmap_run
    lo_y, rate_y = run(host, L2.pipeline(L2.HASHED), the_drive)
    a, a_y = ate(lo, the_drive), ate(lo_y, the_drive)
    print(f"ATE occupancy map {a:.4f} m  yardstick (HashedVoxelPointCloud 0.25 m, cap 20) {a_y:.4f} m  "
          f"bar {2 * a_y + L2.RESOLUTION:.4f} m;  scans/s {rate:.1f} (with the replay) / {rate_y:.1f}")
    # the map's points are voxel centres, up to resolution * sqrt(3) / 2 off the surface: the resolution term; the factor of two
    # is for the sparser map
    assert a <= 2.0 * a_y + L2.RESOLUTION


# a Matcher_Point2Plane (KNN + PCA on the map's points) behind the point matcher, on the SAME map layer and with a search radius
# above the occupancy map's first search voxel (1 m): the second pair makes the search map grow, to 4 m, after the first pair's
# distances (0.4 m) were known -- both pairs have to be handed the map that exists when the alignment is queued
PLANE_MATCHER = """    - class: mp2p_icp::Matcher_Point2Plane
      params:
        distanceThreshold: 0.40
        planeEigenThreshold: 1e-2
        searchRadius: 2.5
        knn: 10
        minimumPlanePoints: 6
        pointLayerMatches:
          - {global: "localmap", local: "decimated", weight: 1.0}
"""


def test_two_matchers_on_one_occupancy_layer_with_a_growing_radius(host):
    drv = L2.drive(16, z_layers=(-0.4, -0.2, 0.0, 0.2, 0.4))  # the walls as planes
    text = L2.pipeline(resolution=0.1, more_matchers=PLANE_MATCHER)
    runs = [run(host, text, drv)[0] for _ in range(2)]
    lo = runs[0]
    assert lo.describePipeline()["icp_path"] == "layers"
    recs = lo.records()
    assert sum(r["icp_run"] for r in recs) == 15 and all(r["icp_good"] for r in recs if r["icp_run"])
    assert lo.profile()["icp.fused_align_calls"] == sum(r["align_calls"] for r in recs)
    v = lo.downloadVoxelMap("localmap")
    assert v["search_voxel_size"] == 4.0 and len(v["logodds"]) > 1000
    lo_y = run(host, L2.pipeline(L2.HASHED, more_matchers=PLANE_MATCHER), drv)[0]  # the same two matchers on the point map
    a, a_y = ate(lo, drv), ate(lo_y, drv)
    print(f"two matchers: ATE occupancy map (0.1 m) {a:.4f} m  yardstick {a_y:.4f} m  bar {2 * a_y + 0.1:.4f} m")
    assert a <= 2.0 * a_y + 0.1  # the bar of test_trajectory_against_the_exact_poses at this resolution
    t0, t1 = runs[0].trajectory(), runs[1].trajectory()  # and the run repeats itself, byte for byte
    assert len(t0) == len(t1) == 16 and all(np.array(p[1]).tobytes() == np.array(q[1]).tobytes() for p, q in zip(t0, t1))
    v1 = runs[1].downloadVoxelMap("localmap")
    assert np.array_equal(v["keys"], v1["keys"]) and np.array_equal(v["logodds"], v1["logodds"])


def test_two_sequences_through_one_batcher_equal_their_solo_runs(host):
    drives = [L2.drive(12), L2.drive(12, phase=15.0)]
    text = L2.pipeline()
    solo_los = [run(host, text, d)[0] for d in drives]
    solo = [lo.trajectory() for lo in solo_los]
    batcher = host.AlignBatcher(len(drives))
    los, errors = [], []
    for _ in drives:
        lo = new_driver(host, text)
        lo.setAlignBatcher(batcher)
        los.append(lo)

    def work(lo, d):
        try:
            for st, xyz in zip(d[0], d[2]):
                lo.onLidar(float(st), xyz)
        except Exception as e:  # noqa: BLE001
            errors.append(e)
        finally:
            batcher.leave()

    th = [threading.Thread(target=work, args=(lo, d)) for lo, d in zip(los, drives)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in th), "a sequence thread is stuck"
    assert not errors, errors
    assert batcher.jobs() >= 2 * 11 and batcher.batches() < batcher.jobs()
    for lo, s, slo in zip(los, solo, solo_los):
        v, sv = lo.downloadVoxelMap("localmap"), slo.downloadVoxelMap("localmap")  # the maps went the same way as well
        assert len(v["logodds"]) > 1000 and np.array_equal(v["keys"], sv["keys"]) and np.array_equal(v["logodds"], sv["logodds"])
        got = lo.trajectory()
        assert len(got) == len(s) == 12
        assert np.array(got[-1][1]).tobytes() == np.array(s[-1][1]).tobytes()
        assert all(a[0] == b[0] and np.array(a[1]).tobytes() == np.array(b[1]).tobytes() for a, b in zip(got, s))
