"""The stand-alone driver on the rgbd-shaped pipeline (tests/rgbd_inline.py): depth images through onDepthImage, the
GeneratorEdgesFromRangeImage step, a HashedVoxelPointCloud map for the edges and a SparseTreesPointCloud map for the planes.
Frames come from an analytic renderer (a room with six boxes, 160 x 120 pixels, depth in millimetres) with exact poses.

The generator's layers and the four decimations are pinned bit for bit by tests/rimg_ref.py followed by the oracle's
ClosestToAverage; the SparseTreesPointCloud stand-in is pinned by the identity it claims (an uncapped HashedVoxelPointCloud
whose voxel is the cell gives the same trajectory, bit for bit); the trajectory is held against the exact poses with the same
drive on a HashedVoxelPointCloud planes map of that voxel with max_points_per_voxel 20 as the yardstick (profiles/rgbd.md has
the measured pair).

Measured on an MI355X (the 30-frame drive): ATE 0.0056 m with the SparseTreesPointCloud planes map against 0.0063 m for the
yardstick: the bar, 2 x 0.0063 + 0.025 = 0.0376 m, is met (the per-frame step is 0.03 m); 0.0057 m with
minimum_points_clearance 0.02, which leaves 26 027 of 44 146 points in the planes map."""
import threading
import time

import numpy as np
import pytest

from mola_lidar_odometry_amd import trajectory

import rgbd_inline as RG
import rimg_ref as RR

pytestmark = pytest.mark.gpu

N_FRAMES = 30


@pytest.fixture(scope="module")
def host():
    from mola_lidar_odometry_amd import _mp2p_icp_hip as H
    return H


@pytest.fixture(scope="module")
def the_drive():
    return RG.drive(N_FRAMES)


def new_driver(host, text):
    lo = host.LidarOdometry(0, True)
    lo.initialize(host.Config.FromYamlText(text))
    return lo


def run(host, text, drv, on_record=None, lo=None):
    stamps, _, images = drv
    lo = lo or new_driver(host, text)
    t0 = time.perf_counter()
    for st, img in zip(stamps, images):
        rec = lo.onDepthImage(float(st), img, **RG.CAMERA)
        if on_record:
            on_record(lo, rec, img)
    return lo, len(images) / (time.perf_counter() - t0)


def ate(lo, drv):
    stamps, poses, _ = drv
    traj = lo.trajectory()
    assert len(traj) >= len(stamps) - 2, "the driver lost track"
    at = [int(np.argmin(np.abs(stamps - t))) for t, _ in traj]
    est = np.array([trajectory.to44(np.array(T)) for _, T in traj])
    return trajectory.ate_rmse(est, poses[at], align="origin")


def same_trajectory(a, b):
    return len(a) == len(b) and all(p[0] == q[0] and np.array(p[1]).tobytes() == np.array(q[1]).tobytes() for p, q in zip(a, b))


@pytest.fixture(scope="module")
def sparse_run(host, the_drive):
    """The drive on the rgbd-shaped text, with the layers of its first frames kept on the way."""
    layers = []

    def keep(lo, rec, img):
        if len(layers) < 3:
            layers.append((img, {name: lo.downloadLayer(name) for name in RG.RES}, dict(rec["layer_sizes"])))

    lo, rate = run(host, RG.pipeline(), the_drive, keep)
    return lo, layers, rate


def test_drive_initialises_creates_both_maps_and_inserts_key_frames(sparse_run):
    lo, _, rate = sparse_run
    recs = lo.records()
    assert len(recs) == N_FRAMES and recs[0]["first_scan"] and not any(r["dropped"] for r in recs)
    assert sum(r["icp_run"] for r in recs) == N_FRAMES - 1 and all(r["icp_good"] for r in recs if r["icp_run"])
    assert sum(r["map_updated"] for r in recs) >= 3  # the first frame and at least two key-frames after it
    assert all(r["n_raw"] == RG.ROWS * RG.COLS for r in recs)
    assert lo.localMapClasses() == {"localmap_edges": "HashedVoxelPointCloud", "localmap_planes": "SparseTreesPointCloud"}
    d = lo.describePipeline()
    assert d["input"] == "depth_image" and d["icp_path"] == "layers"
    assert lo.profile()["icp.fused_align_calls"] == sum(r["align_calls"] for r in recs)  # the plane job of the fused loop
    stats = lo.localMapStats()
    assert stats["localmap_planes"][2] == 1.0 and stats["localmap_edges"][2] == 0.5  # grid_size / voxel_size at a 10 m range
    assert stats["localmap_planes"][0] > 10000 and stats["localmap_edges"][0] > 1000
    assert stats["localmap_planes"][0] > 100 * stats["localmap_planes"][1]  # uncapped cells: hundreds of points each
    print(f"rgbd drive: {rate:.1f} frames/s (with the layer downloads of the first frames); maps {stats}")


def test_layers_of_the_first_frames_bit_for_bit(sparse_run, oracle):
    _, layers, _ = sparse_run
    assert len(layers) == 3
    for img, got, sizes in layers:
        ex, px, _, _ = RR.generate(img, RG.W, RG.SCORE_THRESHOLD, RG.FX, RG.FY, RG.CX, RG.CY, RG.RANGE_UNITS, True, RG.SENSOR_POSE)
        assert len(ex) > 300 and len(px) > 8000
        assert set(sizes) == set(RG.RES)  # 'edges' and 'planes' were deleted
        for name, res in RG.RES.items():
            src = ex if name.startswith("edges") else px
            want = src[oracle.decimate_closest_to_average(src, res)]
            assert sizes[name] == len(want), (name, sizes[name], len(want))
            assert got[name]["alive"]
            assert np.array_equal(np.ascontiguousarray(got[name]["xyz"]).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)), name


def test_sparse_trees_is_the_uncapped_hashed_map_bit_for_bit(host, sparse_run, the_drive):
    lo, _, _ = sparse_run
    lo_h, _ = run(host, RG.pipeline(RG.HASHED_PLANES.format(cap=0)), the_drive)
    assert lo_h.localMapClasses()["localmap_planes"] == "HashedVoxelPointCloud"
    assert same_trajectory(lo.trajectory(), lo_h.trajectory()) and len(lo.trajectory()) == N_FRAMES
    a, b = lo.downloadMap("localmap_planes"), lo_h.downloadMap("localmap_planes")
    assert len(a["xyz"]) > 10000 and a["xyz"].tobytes() == b["xyz"].tobytes() and np.array_equal(a["vox_keys"], b["vox_keys"])


def test_trajectory_against_the_exact_poses(host, sparse_run, the_drive):
    lo, _, _ = sparse_run
    lo_y, rate_y = run(host, RG.pipeline(RG.HASHED_PLANES.format(cap=20)), the_drive)
    a, a_y = ate(lo, the_drive), ate(lo_y, the_drive)
    bar = 2.0 * a_y + RG.PLANES_MAP_RESOLUTION
    print(f"ATE SparseTreesPointCloud {a:.4f} m  yardstick (HashedVoxelPointCloud, the same cell, cap 20) {a_y:.4f} m  "
          f"bar {bar:.4f} m;  yardstick frames/s {rate_y:.1f}")
    assert a_y < RG.STEP, "the yardstick itself does not track on this room"
    # the factor of two is for the different map content, the additive term is one cell of the planes_for_map decimation
    assert a <= bar


def test_clearance_reaches_the_map(host, sparse_run, the_drive):
    lo, _, _ = sparse_run
    lo_c, _ = run(host, RG.pipeline(clearance=0.02), the_drive)
    n, n_c = lo.localMapSizes()["localmap_planes"], lo_c.localMapSizes()["localmap_planes"]
    a_c = ate(lo_c, the_drive)
    print(f"planes map: {n} points without clearance, {n_c} with minimum_points_clearance 0.02; ATE with it {a_c:.4f} m")
    assert 0 < n_c < n
    assert a_c < RG.STEP  # it still tracks
    assert lo.localMapSizes()["localmap_edges"] > 0 and lo_c.localMapSizes()["localmap_edges"] > 0


def test_two_sequences_through_one_batcher_equal_their_solo_runs(host):
    drives = [RG.drive(10), RG.drive(10, phase=-6.0)]
    text = RG.pipeline()
    solo = [run(host, text, d)[0].trajectory() for d in drives]
    batcher = host.AlignBatcher(len(drives))
    los, errors = [], []
    for _ in drives:
        lo = new_driver(host, text)
        lo.setAlignBatcher(batcher)
        los.append(lo)

    def work(lo, d):
        try:
            run(host, text, d, lo=lo)
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
    assert batcher.jobs() >= 2 * 9 and batcher.batches() < batcher.jobs()  # at least one batch of two plane jobs
    for lo, s in zip(los, solo):
        got = lo.trajectory()
        assert len(got) == len(s) == 10 and same_trajectory(got, s)
