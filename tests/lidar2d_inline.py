"""What the occupancy-voxel-map tests share: a pipeline text with the structure and values of the reference's 2-D LiDAR
pipeline (pipelines/lidar2d.yaml: one point pair with pairingsPerPoint 2, the de-skew / decimate / by-range / delete chain, one
FilterMerge into an mrpt::maps::CVoxelMap), written inline, and an analytic 2-D ray caster for its scans.  No product code."""
import numpy as np

VOXELMAP = """        class: mrpt::maps::CVoxelMap
        creationOpts:
          resolution: {resolution}
        insertOpts:
          prob_miss: 0.30
          prob_hit: 0.70
          clamp_min: 0.05
          clamp_max: 0.95
          ray_trace_free_space: true
          decimation: 1
          remove_voxels_farther_than: 60
        likelihoodOpts:
          occupiedThreshold: 0.60
"""

HASHED = """        class: mola::HashedVoxelPointCloud
        creationOpts:
          voxel_size: 0.25
        insertOpts:
          max_points_per_voxel: 20
          min_distance_between_points: 0
          remove_voxels_farther_than: 60
"""

_TEXT = """params:
  min_time_between_scans: 1e-3
  max_sensor_range_filter_coefficient: 0.999
  absolute_minimum_sensor_range: 20.0
  local_map_updates:
    enabled: true
    min_translation_between_keyframes: '0.02*ESTIMATED_SENSOR_MAX_RANGE'
    min_rotation_between_keyframes: 15.0
    max_distance_to_keep_keyframes: 'max(100.0, 1.50*ESTIMATED_SENSOR_MAX_RANGE)'
    check_for_removal_every_n: 100
  min_icp_goodness: 0.25
  adaptive_threshold:
    enabled: true
    initial_sigma: 0.20
    min_motion: 0.10
    kp: 2.0
    alpha: 0.99
navstate_fuse_params:
  initial_twist: [0.0, 0.0, 0.0,  0.0, 0.0, 0.0]
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
        robustKernelParam: '0.50*ADAPTIVE_THRESHOLD_SIGMA'
  matchers:
    - class: mp2p_icp::Matcher_Points_DistanceThreshold
      params:
        threshold: '2.0*ADAPTIVE_THRESHOLD_SIGMA'
        thresholdAngularDeg: 0
        pairingsPerPoint: 2
        allowMatchAlreadyMatchedGlobalPoints: true
        pointLayerMatches:
          - {global: "localmap", local: "decimated", weight: 1.0}
MORE_MATCHERS  quality:
    - class: mp2p_icp::QualityEvaluator_PairedRatio
      params:
        ~
localmap_generator:
  - class_name: mp2p_icp_filters::Generator
    params:
      target_layer: 'localmap'
      metric_map_definition:
MAPDEF
observations_filter_1st_pass:
  - class_name: mp2p_icp_filters::FilterDeskew
    params:
      input_pointcloud_layer: 'raw'
      output_pointcloud_layer: 'deskewed'
      silently_ignore_no_timestamps: true
      twist: [vx,vy,vz,wx,wy,wz]
  - class_name: mp2p_icp_filters::FilterDecimateVoxels
    params:
      input_pointcloud_layer: 'deskewed'
      output_pointcloud_layer: 'decimated_pre'
      voxel_filter_resolution: 0.05
      minimum_input_points_to_filter: 2000
      decimate_method: DecimateMethod::FirstPoint
  - class_name: mp2p_icp_filters::FilterByRange
    params:
      input_pointcloud_layer: 'decimated_pre'
      output_layer_between: 'decimated'
      range_min: max(0.10, 0.03*ESTIMATED_SENSOR_MAX_RANGE)
      range_max: 1.25*ESTIMATED_SENSOR_MAX_RANGE
  - class_name: mp2p_icp_filters::FilterDeleteLayer
    params:
      pointcloud_layer_to_remove: ['raw','deskewed', 'decimated_pre']
insert_observation_into_local_map:
  - class_name: mp2p_icp_filters::FilterMerge
    params:
      input_pointcloud_layer: 'decimated'
      target_layer: 'localmap'
      input_layer_in_local_coordinates: true
      robot_pose: [robot_x, robot_y, robot_z, robot_yaw, robot_pitch, robot_roll]
"""

RESOLUTION = 0.05


def pipeline(map_def=None, resolution=RESOLUTION, more_matchers=""):
    """The lidar2d-shaped pipeline; map_def: a metric_map_definition body (default: the CVoxelMap one); more_matchers: entries
    of the ICP block's `matchers` list behind the point matcher."""
    text = _TEXT.replace("MAPDEF\n", map_def if map_def is not None else VOXELMAP.format(resolution=resolution))
    return text.replace("MORE_MATCHERS", more_matchers)


# ---- the scene: a 10 m x 8 m room with one box, seen by 720 beams in the plane z = 0
_SEGMENTS = np.array([[-5, -4, 5, -4], [5, -4, 5, 4], [5, 4, -5, 4], [-5, 4, -5, -4],          # the room
                      [1.0, 1.0, 2.5, 1.0], [2.5, 1.0, 2.5, 2.0], [2.5, 2.0, 1.0, 2.0], [1.0, 2.0, 1.0, 1.0]], np.float64)


def cast(x, y, yaw, n_beams=720):
    """The scan at pose (x, y, yaw): [n_beams, 3] float32 points in the vehicle frame, z = 0 (exact ray / segment hits)."""
    a = yaw + np.arange(n_beams) * (2.0 * np.pi / n_beams)
    d = np.stack([np.cos(a), np.sin(a)], 1)                       # [n, 2]
    p0, p1 = _SEGMENTS[:, :2], _SEGMENTS[:, 2:]
    e = p1 - p0                                                   # [s, 2]
    w = p0 - np.array([x, y])                                     # [s, 2]
    den = d[:, None, 0] * e[None, :, 1] - d[:, None, 1] * e[None, :, 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (w[None, :, 0] * e[None, :, 1] - w[None, :, 1] * e[None, :, 0]) / den   # along the beam
        u = (w[None, :, 0] * d[:, None, 1] - w[None, :, 1] * d[:, None, 0]) / den   # along the segment
    ok = (np.abs(den) > 1e-12) & (t > 1e-9) & (u >= 0.0) & (u <= 1.0)
    r = np.where(ok, t, np.inf).min(axis=1)
    b = np.arange(n_beams) * (2.0 * np.pi / n_beams)              # beam angle in the vehicle frame
    return np.stack([r * np.cos(b), r * np.sin(b), np.zeros(n_beams)], 1).astype(np.float32)


def drive(n_scans=30, phase=0.0, dt=0.1, step_deg=120.0 / 29.0, z_layers=(0.0,)):
    """A curved path through the room, step_deg of a 2.5 m circle per scan: (stamps, exact 4x4 poses, scans).  z_layers: the
    heights at which every beam's hit is repeated (the walls as vertical planes; the default is the 2-D scan)."""
    a = np.deg2rad(-150.0 + phase) + np.arange(n_scans) * np.deg2rad(step_deg)
    xs, ys, yaws = 2.5 * np.cos(a), -0.5 + 2.5 * np.sin(a), a + np.pi / 2
    poses = np.zeros((n_scans, 4, 4))
    poses[:, 3, 3] = poses[:, 2, 2] = 1.0
    poses[:, 0, 0], poses[:, 0, 1], poses[:, 1, 0], poses[:, 1, 1] = np.cos(yaws), -np.sin(yaws), np.sin(yaws), np.cos(yaws)
    poses[:, 0, 3], poses[:, 1, 3] = xs, ys
    scans = [np.concatenate([cast(x, y, w) + np.array([0, 0, z], np.float32) for z in z_layers]) for x, y, w in zip(xs, ys, yaws)]
    return np.arange(n_scans) * dt, poses, scans
