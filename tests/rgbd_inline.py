"""What the depth-image tests share: a pipeline text with the structure and values of the reference's RGB-D pipeline
(pipelines/rgbd.yaml: a GeneratorEdgesFromRangeImage, four ClosestToAverage decimations and a FilterDeleteLayer, a point pair
with pairingsPerPoint 2 beside a Matcher_Point2Plane, a HashedVoxelPointCloud map for the edges and a SparseTreesPointCloud map
for the planes, no 2nd pass, no de-skew), written inline, and an analytic depth renderer for its frames.  No product code."""
import numpy as np

SPARSE_TREES = """        class: mola::SparseTreesPointCloud
        creationOpts:
          grid_size: '$f{{max(1.0, min(5.0, 0.10*ESTIMATED_SENSOR_MAX_RANGE))}}'
        insertOpts:
          minimum_points_clearance: {clearance}
          remove_submaps_farther_than: '$f{{max(100.0, 1.50*ESTIMATED_SENSOR_MAX_RANGE)}}'
        likelihoodOpts:
          sigma_dist: 1.0
          max_corr_distance: 2.0
          decimation: 10
        renderOpts:
          point_size: 1.0
          show_inner_grid_boxes: false
"""

# the same cells as a HashedVoxelPointCloud: cap 0 is the identity the SparseTreesPointCloud stand-in claims, cap 20 the yardstick
HASHED_PLANES = """        class: mola::HashedVoxelPointCloud
        creationOpts:
          voxel_size: '$f{{max(1.0, min(5.0, 0.10*ESTIMATED_SENSOR_MAX_RANGE))}}'
        insertOpts:
          max_points_per_voxel: {cap}
          min_distance_between_points: 0
          remove_voxels_farther_than: '$f{{max(100.0, 1.50*ESTIMATED_SENSOR_MAX_RANGE)}}'
"""

_TEXT = """params:
  min_time_between_scans: 1e-3
  max_sensor_range_filter_coefficient: 0.999
  absolute_minimum_sensor_range: 10.0
  local_map_updates:
    enabled: true
    min_translation_between_keyframes: '(0.03 + sqrt(WX^2+WY^2+WZ^2)*0.1)*ESTIMATED_SENSOR_MAX_RANGE'
    min_rotation_between_keyframes: 15.0
    max_distance_to_keep_keyframes: 'max(50.0, 2.50*ESTIMATED_SENSOR_MAX_RANGE)'
    check_for_removal_every_n: 100
  min_icp_goodness: 0.05
  adaptive_threshold:
    enabled: true
    initial_sigma: 0.20
    min_motion: 0.10
navstate_fuse_params:
  max_time_to_use_velocity_model: 2.0
  sigma_random_walk_acceleration_linear: 10.0
  sigma_random_walk_acceleration_angular: 10.0
icp_settings_with_vel:
  class_name: mp2p_icp::ICP
  params:
    maxIterations: 300
    minAbsStep_trans: 1e-4
    minAbsStep_rot: 5e-5
  solvers:
    - class: mp2p_icp::Solver_GaussNewton
      params:
        maxIterations: 2
        robustKernel: 'RobustKernel::GemanMcClure'
        robustKernelParam: 0.02
  matchers:
    - class: mp2p_icp::Matcher_Points_DistanceThreshold
      params:
        threshold: 0.20
        thresholdAngularDeg: 0.5
        pairingsPerPoint: 2
        allowMatchAlreadyMatchedGlobalPoints: true
        pointLayerMatches:
          - {global: "localmap_edges", local: "edges_for_icp", weight: 1.0}
    - class: mp2p_icp::Matcher_Point2Plane
      params:
        distanceThreshold: 0.40
        planeEigenThreshold: 1e-2
        searchRadius: 0.80
        knn: 10
        minimumPlanePoints: 6
        pointLayerMatches:
          - {global: "localmap_planes", local: "planes_for_icp", weight: 1.0}
  quality:
    - class: mp2p_icp::QualityEvaluator_PairedRatio
      params:
        ~
localmap_generator:
  - class_name: mp2p_icp_filters::Generator
    params:
      target_layer: 'localmap_edges'
      throw_on_unhandled_observation_class: true
      process_class_names_regex: ''
      metric_map_definition:
        class: mola::HashedVoxelPointCloud
        creationOpts:
          voxel_size: '$f{max(0.05, min(0.5, 0.10*ESTIMATED_SENSOR_MAX_RANGE))}'
        insertOpts:
          max_points_per_voxel: 20
          min_distance_between_points: 0
          remove_voxels_farther_than: '$f{max(100.0, 1.50*ESTIMATED_SENSOR_MAX_RANGE)}'
        likelihoodOpts:
          sigma_dist: 1.0
          max_corr_distance: 2.0
          decimation: 10
  - class_name: mp2p_icp_filters::Generator
    params:
      target_layer: 'localmap_planes'
      throw_on_unhandled_observation_class: true
      process_class_names_regex: ''
      metric_map_definition:
PLANESMAP
observations_generator:
  - class_name: mp2p_icp_filters::GeneratorEdgesFromRangeImage
    params:
      target_layer: 'edges'
      planes_target_layer: 'planes'
      throw_on_unhandled_observation_class: true
      process_class_names_regex: '.*'
      process_sensor_labels_regex: '.*'
      score_threshold: 10
      row_window_length: 6
observations_filter_1st_pass:
  - class_name: mp2p_icp_filters::FilterDecimateVoxels
    params:
      input_pointcloud_layer: 'planes'
      output_pointcloud_layer: 'planes_for_map'
      voxel_filter_resolution: 0.025
      decimate_method: DecimateMethod::ClosestToAverage
  - class_name: mp2p_icp_filters::FilterDecimateVoxels
    params:
      input_pointcloud_layer: 'planes'
      output_pointcloud_layer: 'planes_for_icp'
      voxel_filter_resolution: 0.050
      decimate_method: DecimateMethod::ClosestToAverage
  - class_name: mp2p_icp_filters::FilterDecimateVoxels
    params:
      input_pointcloud_layer: 'edges'
      output_pointcloud_layer: 'edges_for_map'
      voxel_filter_resolution: 0.05
      decimate_method: DecimateMethod::ClosestToAverage
  - class_name: mp2p_icp_filters::FilterDecimateVoxels
    params:
      input_pointcloud_layer: 'edges'
      output_pointcloud_layer: 'edges_for_icp'
      voxel_filter_resolution: 0.10
      decimate_method: DecimateMethod::ClosestToAverage
  - class_name: mp2p_icp_filters::FilterDeleteLayer
    params:
      pointcloud_layer_to_remove: ['edges', 'planes']
insert_observation_into_local_map:
  - class_name: mp2p_icp_filters::FilterMerge
    params:
      input_pointcloud_layer: 'edges_for_map'
      target_layer: 'localmap_edges'
      input_layer_in_local_coordinates: true
      robot_pose: [robot_x, robot_y, robot_z, robot_yaw, robot_pitch, robot_roll]
  - class_name: mp2p_icp_filters::FilterMerge
    params:
      input_pointcloud_layer: 'planes_for_map'
      target_layer: 'localmap_planes'
      input_layer_in_local_coordinates: true
      robot_pose: [robot_x, robot_y, robot_z, robot_yaw, robot_pitch, robot_roll]
"""

W, SCORE_THRESHOLD = 6, 10.0          # the generator's values in the text above
RES = dict(planes_for_map=0.025, planes_for_icp=0.050, edges_for_map=0.05, edges_for_icp=0.10)  # the four decimations
PLANES_MAP_RESOLUTION = RES["planes_for_map"]


def pipeline(planes_map=None, clearance=0):
    """The rgbd-shaped pipeline; planes_map: the metric_map_definition body of 'localmap_planes' (default: the
    SparseTreesPointCloud one with `clearance` as minimum_points_clearance; HASHED_PLANES.format(cap=...) for the others)."""
    return _TEXT.replace("PLANESMAP\n", planes_map if planes_map is not None else SPARSE_TREES.format(clearance=clearance))


# ---- the camera: 160 x 120 pixels, depth along the optical axis in millimetres; sensor frame x forward, y left, z up
ROWS, COLS = 120, 160
FX = FY = 140.0
CX, CY = 79.5, 59.5
RANGE_UNITS = 0.001
MAX_RANGE = 8.0                                         # [m] beyond: no return
SENSOR_POSE = np.array([[1.0, 0.0, 0.0, 0.10],
                        [0.0, 1.0, 0.0, 0.00],
                        [0.0, 0.0, 1.0, 1.20]])         # the camera on the vehicle
CAMERA = dict(fx=FX, fy=FY, cx=CX, cy=CY, range_units=RANGE_UNITS, range_is_depth=True, sensor_pose=list(SENSOR_POSE.ravel()))

# ---- the scene: an axis-aligned room seen from inside, and a few boxes seen from outside (min corner, max corner)
_ROOM = np.array([[-2.0, -3.0, 0.0], [6.0, 3.0, 2.6]])
_BOXES = np.array([[[3.0, -1.6, 0.0], [3.6, -0.9, 1.5]],
                   [[4.2, 0.4, 0.0], [4.9, 1.3, 1.9]],
                   [[2.4, 1.5, 0.0], [2.9, 2.1, 1.1]],
                   [[5.0, -2.6, 0.0], [5.6, -1.9, 2.2]],
                   [[3.4, -0.2, 0.0], [3.7, 0.2, 0.8]],
                   [[5.6, -0.6, 1.4], [6.0, 0.1, 2.1]]])


def _slabs(o, d, box):
    """Entry and exit parameter of every ray o + t d [n, 3] through the axis-aligned box (min, max)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        t0 = (box[0] - o) / d
        t1 = (box[1] - o) / d
    lo, hi = np.minimum(t0, t1), np.maximum(t0, t1)
    lo = np.where(np.isnan(lo), -np.inf, lo)
    hi = np.where(np.isnan(hi), np.inf, hi)
    return lo.max(axis=1), hi.min(axis=1)


def render(pose):
    """The depth image [ROWS, COLS] uint16 (millimetres, 0 = no return) of the camera on the vehicle at the 4x4 `pose`."""
    cam = pose @ np.vstack([SENSOR_POSE, [0, 0, 0, 1]])
    r, c = np.mgrid[0:ROWS, 0:COLS]
    d_s = np.stack([np.ones(r.size), (CX - c.ravel()) / FX, (CY - r.ravel()) / FY], 1)  # x = 1: t is the depth
    d = d_s @ cam[:3, :3].T
    o = np.broadcast_to(cam[:3, 3], d.shape)
    _, t = _slabs(o, d, _ROOM)                                  # from inside: where the ray leaves the room
    for b in _BOXES:
        t_in, t_out = _slabs(o, d, b)
        hit = (t_in < t_out) & (t_in > 1e-6)
        t = np.where(hit & (t_in < t), t_in, t)
    mm = np.rint(t / RANGE_UNITS)
    mm = np.where(np.isfinite(t) & (t > 0) & (t <= MAX_RANGE), mm, 0)
    return mm.reshape(ROWS, COLS).astype(np.uint16)


STEP = 0.03  # [m] per frame


def drive(n_frames=30, phase=0.0, dt=0.1, step=STEP, yaw_step_deg=0.5):
    """A gentle left arc through the room at `step` metres and yaw_step_deg per frame: (stamps, exact 4x4 poses, images)."""
    yaws = np.deg2rad(phase) + np.arange(n_frames) * np.deg2rad(yaw_step_deg)
    xs = np.concatenate([[0.0], np.cumsum(step * np.cos(yaws[:-1]))])
    ys = -0.4 + np.concatenate([[0.0], np.cumsum(step * np.sin(yaws[:-1]))])
    poses = np.zeros((n_frames, 4, 4))
    poses[:, 3, 3] = poses[:, 2, 2] = 1.0
    poses[:, 0, 0], poses[:, 0, 1], poses[:, 1, 0], poses[:, 1, 1] = np.cos(yaws), -np.sin(yaws), np.sin(yaws), np.cos(yaws)
    poses[:, 0, 3], poses[:, 1, 3] = xs, ys
    return np.arange(n_frames) * dt, poses, [render(p) for p in poses]
