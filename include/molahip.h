/* molahip.h -- C ABI of libmolahip: the MI355X-native (gfx950 / HIP) implementation of the per-scan
 * ICP registration hot path that mola::LidarOdometry runs through mp2p_icp::ICP::align().
 *
 * This is the drop-in boundary.  No C++ or torch types cross it: opaque handles,
 * plain pointers + sizes, POD structs, integer status codes.  Every entry point names the reference
 * interface it stands in for ("file:line" is relative to /root/reference; [U] marks upstream classes
 * that the reference selects by name from its YAML but does not vendor -- SURVEY.md 0.1).
 * The C++ host layer (mola_lidar_odometry_amd/host/, namespace mp2p_icp_hip) and the mp2p_icp
 * plugin adapter are thin wrappers over exactly these functions.
 *
 * Conventions
 *  - Poses are `double T[12]`: row-major 3x4 [R|t] of "local wrt global" (the 3rd argument of
 *    ICP::align, LidarOdometry.cpp:961-962; mrpt::poses::CPose3D).
 *  - Tangent vectors / 6x6 matrices use [v(3); w(3)] ordering (LidarOdometry.cpp:977-984); the
 *    covariance is in (x,y,z,yaw,pitch,roll) like mrpt::poses::CPose3DPDFGaussian.
 *  - Point clouds are SoA float arrays (mrpt CPointsMap::getPointsBufferRef_{x,y,z} [U]).
 *  - `mem` arguments say where the caller's arrays live: MH_MEM_HOST (borrowed for the call, copied),
 *    MH_MEM_DEVICE (HIP device pointers on the context's device, read in place) or, where an entry point says
 *    so, MH_MEM_HOST_PINNED: page-locked host memory (hipHostMalloc / torch pin_memory) that the caller keeps
 *    valid and unmodified until the context's stream has passed the copy (mh_ctx_synchronize, or the return of
 *    the next blocking call that uses the scan) -- the copy is then asynchronous on the context's stream and
 *    the call returns at once, so uploads of the next scans overlap the alignment of the current ones.
 *  - Every function returns mh_status (0 = OK), never throws, never aborts; a message for the last
 *    failure on the calling thread is available from mh_last_error_string().
 *  - One context = one HIP device + one stream.  Contexts are independent and may be driven from
 *    different host threads; a single context (and the maps/scans created from it) must not be used
 *    from two threads at once -- the reference itself keeps one align() in flight per LidarOdometry
 *    instance (LidarOdometry.h:548-549, LidarOdometry.cpp:634).
 *  - There is NO CPU fallback: without a HIP device mh_ctx_create fails with MH_ERR_NO_DEVICE.
 */
#ifndef MOLAHIP_H
#define MOLAHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MH_API __attribute__((visibility("default")))

#define MH_VERSION_MAJOR 0
#define MH_VERSION_MINOR 1
#define MH_VERSION_PATCH 0
/* The parameter structs of this header carry no size field: they grow at the END, and every growth bumps MH_ABI_VERSION (6:
 * mh_preprocess_params' two decimation-method fields, round 5; 7: mh_layer_pair and mh_icp_align_layers, later also
 * mh_curvature_params and mh_scan_curvature, then the intensity channel's entry points and mh_by_intensity_params,
 * mh_layer_pair_gates and mh_icp_align_layers_gated, mh_layer_pair_knn and mh_icp_align_layers_kbest, mh_layer_pair_plane and
 * mh_icp_align_layers_planes, mh_layer_job_opts and mh_icp_align_layers_batch_opts, mh_layer_job_planes and
 * mh_icp_align_layers_batch_planes, mh_occmap_params / mh_occmap_info and the mh_occmap_* entry points, mh_range_image_params and
 * mh_scan_edges_from_range_image, mh_radius_out / mh_radius_info and mh_nn_search_radius: new structs and entry
 * points change no existing layout, and a binder that lacks
 * an entry point finds out when it resolves the symbol).  A binder built against this header checks
 * `mh_abi_version() == MH_ABI_VERSION` once after loading the library (capi.py does; the C++ host layer links the header it was
 * built with) and zero-initialises every struct it passes -- a field the binder does not know then reads as its default. */
#define MH_ABI_VERSION 7

typedef int32_t mh_status;
enum {
  MH_OK = 0,
  MH_ERR_INVALID_ARGUMENT = 1,
  MH_ERR_HIP = 2,            /* a HIP runtime call failed; see mh_last_error_string() */
  MH_ERR_OUT_OF_MEMORY = 3,
  MH_ERR_OUT_OF_RANGE = 4,   /* a voxel index does not fit the 21-bit-per-axis key */
  MH_ERR_NO_DEVICE = 5,
  MH_ERR_UNSUPPORTED = 6,
  MH_ERR_INTERNAL = 7,
  /* not a failure: the call has done what it was asked to; an EARLIER asynchronous call left something out (mh_map_insert) */
  MH_WARN_PREVIOUS_OUT_OF_RANGE = 64
};

enum { MH_MEM_HOST = 0, MH_MEM_DEVICE = 1, MH_MEM_HOST_PINNED = 2 };

/* coordinate -> voxel index rule (FLOOR is the default) */
enum { MH_INDEX_FLOOR = 0, MH_INDEX_TRUNC = 1 };

/* Voxel-index distance used by remove_voxels_farther_than (lidar3d-default.yaml:237-238; the comment there says "L1",
 * upstream's code is unverified [U]): max(|dk|) (default), |dkx|+|dky|+|dkz|, or sqrt(dkx^2+dky^2+dkz^2), each
 * compared with ceil(remove_voxels_farther_than / voxel_size).  A run-time switch until the reference decides it. */
enum { MH_FAR_CHEBYSHEV = 0, MH_FAR_L1 = 1, MH_FAR_L2 = 2 };

/* mp2p_icp::RobustKernel [U] as selected at lidar3d-default.yaml:188.  The exact upstream form of
 * GemanMcClure is unverified (SURVEY App.B U1), hence the variants. */
enum {
  MH_KERNEL_NONE = 0,
  MH_KERNEL_GM_C4 = 1,     /* w = c^4/(c^2+e^2)^2  (default) */
  MH_KERNEL_GM_KISS = 2,   /* w = c^2/(c+e^2)^2 */
  MH_KERNEL_GM_BARRON = 3, /* w = 1/(e^2/(4c^2)+1)^2 */
  MH_KERNEL_CAUCHY = 4,    /* w = c^2/(c^2+e^2) */
  MH_KERNEL_GM_C2 = 5      /* w = c^2/(c^2+e^2)^2 */
};

/* mp2p_icp::IterTermReason [U] (used in-tree at LidarOdometry.cpp:970,1007,1019) */
enum {
  MH_TERM_UNDEFINED = 0,
  MH_TERM_NO_PAIRINGS = 1,
  MH_TERM_SOLVER_ERROR = 2,
  MH_TERM_MAX_ITERATIONS = 3,
  MH_TERM_STALLED = 4,
  MH_TERM_QUALITY_CHECKPOINT_FAILED = 5,
  MH_TERM_HOOK_REQUEST = 6
};

typedef struct mh_ctx mh_ctx;
typedef struct mh_map mh_map;
typedef struct mh_scan mh_scan;

/* ------------------------------------------------------------------------------------------------
 * Library / context
 * ---------------------------------------------------------------------------------------------- */
MH_API mh_status mh_version(uint32_t* major, uint32_t* minor, uint32_t* patch);
MH_API const char* mh_last_error_string(void);
/* MH_ABI_VERSION of the loaded library (see above). */
MH_API uint32_t mh_abi_version(void);
/* A status at or above MH_WARN_PREVIOUS_OUT_OF_RANGE is not a failure: the call did its work (MH_SUCCEEDED is the test a binder
 * wants where it would write `== MH_OK`). */
#define MH_SUCCEEDED(status) ((status) == MH_OK || (status) >= MH_WARN_PREVIOUS_OUT_OF_RANGE)
MH_API const char* mh_status_string(mh_status s);
MH_API mh_status mh_device_count(int32_t* n);

/* `hip_stream`: a hipStream_t to run on (e.g. the caller's torch stream), or NULL to let the context
 * create and own a non-blocking stream. */
MH_API mh_status mh_ctx_create(int32_t device, void* hip_stream, mh_ctx** out);
MH_API mh_status mh_ctx_destroy(mh_ctx* ctx);
MH_API mh_status mh_ctx_synchronize(mh_ctx* ctx);
MH_API mh_status mh_ctx_stream(mh_ctx* ctx, void** hip_stream_out);
/* Free / total device memory [bytes] of the context's GPU after draining its stream (capacity planning for batches of
 * maps and scans; also how the tests check that destroyed handles give their memory back). */
MH_API mh_status mh_ctx_memory_info(mh_ctx* ctx, uint64_t* free_bytes, uint64_t* total_bytes);

/* Page-locked host memory for MH_MEM_HOST_PINNED uploads (hipHostMalloc / hipHostFree behind the C ABI, for host code
 * that does not link the HIP runtime itself). */
MH_API mh_status mh_host_alloc_pinned(size_t bytes, void** out);
MH_API mh_status mh_host_free_pinned(void* p);

/* ------------------------------------------------------------------------------------------------
 * Local map: the NN-search target.  Replaces mola::HashedVoxelPointCloud [U] as configured at
 * lidar3d-default.yaml:228-242 (creationOpts.voxel_size :233, insertOpts.max_points_per_voxel :235)
 * in its role as mrpt::maps::NearestNeighborsCapable [U] for the matcher.
 * Device layout: open-addressing hash table of 16-byte slots {packed voxel key, first, count} plus
 * voxel-contiguous 16-byte point records {x,y,z,source index}; see DESIGN.md.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  float voxel_size;              /* [m] > 0 */
  uint32_t max_points_per_voxel; /* 0 = unlimited */
  uint32_t index_mode;           /* MH_INDEX_* */
  /* mola::NDT [U] role (lidar3d-ndt.yaml:236-254); all 0 = plain HashedVoxelPointCloud */
  float min_distance_between_points; /* insertOpts: drop a point closer than this to a stored point of its voxel */
  float ndt_max_eigen_ratio;         /* insertOpts.max_eigen_ratio_for_planes; > 0 enables per-voxel NDT statistics */
  uint32_t ndt_min_points;           /* voxels with fewer stored points carry no NDT (0 -> 4) */
  uint32_t far_voxel_metric;         /* MH_FAR_* : how mh_map_insert measures "farther than" (see there) */
} mh_map_params;

typedef struct {
  uint64_t n_points;   /* stored points (after the per-voxel cap) */
  uint64_t n_offered;  /* points offered to the last build */
  uint64_t n_voxels;   /* occupied voxels */
  uint64_t table_size; /* hash slots (power of two) */
  float bbox_min[3], bbox_max[3];
  float voxel_size;
  uint32_t max_points_per_voxel;
  uint64_t n_planes;   /* voxels whose NDT is a plane (0 when NDT statistics are off) */
  uint32_t deferred_status; /* MH_OK, or the verdict of the last mh_map_insert that no call has reported yet (see there) */
  uint32_t reserved_;
} mh_map_info;

MH_API mh_status mh_map_create(mh_ctx* ctx, const mh_map_params* params, mh_map** out);
MH_API mh_status mh_map_destroy(mh_map* map);
/* (Re)build from n points: equivalent to clear() + insertPoint() for each point in order
 * (HashedVoxelPointCloud::insertPoint [U] via FilterMerge, lidar3d-default.yaml:362-368): a point whose
 * voxel already holds max_points_per_voxel is dropped; non-finite points are dropped.  The "global
 * index" reported by the NN search is the point's index in these arrays. */
/* Testing hook (fault injection; no effect on results): the next `first_attempts` device allocations of the library's grow-only
 * buffers report out-of-memory on their first attempt (the library then returns its retired blocks to the runtime and asks for
 * exactly what it needs), the next `retries` of those second attempts fail as well (the call then returns MH_ERR_OUT_OF_MEMORY
 * and leaves every handle usable).  Process-wide counters. */
MH_API mh_status mh_debug_fail_allocations(int32_t first_attempts, int32_t retries);
MH_API mh_status mh_map_build(mh_map* map, const float* x, const float* y, const float* z, size_t n, int32_t mem);
MH_API mh_status mh_map_get_info(const mh_map* map, mh_map_info* info);
/* Incremental key-frame update, device resident.  Replaces FilterMerge ->
 * HashedVoxelPointCloud::insertPointCloud [U] (lidar3d-default.yaml:362-368, LidarOdometry.cpp:1161-1206) for the
 * layer `scan` (vehicle frame, input_layer_in_local_coordinates: true): every point is composed with the robot
 * pose T (row-major 3x4, fp64, result rounded to float) and offered to insertPoint in order, after everything the
 * map already stores; then, if remove_voxels_farther_than > 0 (insertOpts, yaml:238), every voxel whose index
 * distance (mh_map_params::far_voxel_metric; default max(|dkx|,|dky|,|dkz|)) to the voxel of T's translation exceeds
 * ceil(remove_voxels_farther_than/voxel_size) is erased [U].  The source index of a new point is (points ever offered to this map) + its index in `scan`.
 * Nothing travels to the host except four counters, and those lazily: the call returns once the update is QUEUED.
 * Deferred verdict: points whose voxel index leaves the +-2^20 range of the packed key are left out, and that is known
 * only when the counters arrive.  It is reported -- once, as MH_WARN_PREVIOUS_OUT_OF_RANGE, a status of its own that is NOT a
 * failure -- by the NEXT mh_map_insert on this map, which performs its own insertion as always (a caller can tell "inserted" from
 * "not inserted": every MH_ERR_* means not inserted, this one and MH_OK mean inserted; the wrappers log it and go on); until then
 * mh_map_get_info shows it in mh_map_info::deferred_status (as MH_ERR_OUT_OF_RANGE).  mh_map_get_info and the downloads
 * never fail for it.  (mh_map_build is synchronous about it: it builds the map without the offending points, sets
 * n_offered, and returns MH_ERR_OUT_OF_RANGE itself.) */
MH_API mh_status mh_map_insert(mh_map* map, const mh_scan* scan, const double T[12], float remove_voxels_farther_than);
/* Copy the stored content to HOST arrays (any may be NULL): points voxel by voxel, voxels in ascending
 * (kx,ky,kz), in-voxel insertion order.  xyz/src_idx hold n_points entries, vox_* hold n_voxels. */
MH_API mh_status mh_map_download(const mh_map* map, float* x, float* y, float* z, uint32_t* src_idx,
                                 int32_t* vox_keys_xyz, uint32_t* vox_first, uint32_t* vox_count);
/* NDT statistics per occupied voxel, same voxel order as mh_map_download (HOST arrays of n_voxels entries, any may be
 * NULL): centroid, unit normal (largest component positive) and the plane flag.  Zeros when NDT is off. */
MH_API mh_status mh_map_download_ndt(const mh_map* map, float* cx, float* cy, float* cz, float* nx, float* ny, float* nz,
                                     uint32_t* is_plane);
/* Snapshot restore: the inverse of mh_map_download.  The input is exactly what mh_map_download returns -- n points voxel by
 * voxel, voxels in ascending packed key (kx, ky, kz), in-voxel insertion order, with the source index of every point -- plus
 * mh_map_info::n_offered; arrays live in `mem` (MH_MEM_HOST or MH_MEM_DEVICE).  Whatever the map held before is replaced.
 *  - Afterwards the map is indistinguishable from the one that was downloaded: the same mh_map_download and
 *    mh_map_download_ndt bits (the NDT statistics are recomputed from the stored points, as every rebuild does), the same
 *    n_points / n_offered / n_voxels / n_planes and bounding box in mh_map_get_info (table_size is an implementation matter: it
 *    follows the history of a map and no query depends on it), the same answers from every search route, and the same result
 *    of a following mh_map_insert: its source indices continue from n_offered, its cap and clearance rule see the restored
 *    points as stored ones.
 *  - Restore stores exactly the points given: it applies no cap and no min_distance_between_points decision of its own.
 *  - MH_ERR_INVALID_ARGUMENT, and the map is left EMPTY (n_offered 0), when the input could not have been a download of a map
 *    with these mh_map_params: voxel keys not non-decreasing in input order under the map's voxel size and index mode; a voxel
 *    holding more than max_points_per_voxel points (when that is > 0); a non-finite point or one outside the key range
 *    (|coord| / voxel_size >= 1e6); n_offered < n.  The checks are one device pass over the keys (an adjacent-key compare into
 *    the build's flag word), not a host loop.  (A NULL map, a bad `mem`, NULL arrays with n > 0, n or n_offered beyond what
 *    32-bit source indices can number: MH_ERR_INVALID_ARGUMENT too, and the map is not touched.)
 *  - n == 0: an empty map that keeps n_offered (arrays may be NULL).
 *  - Like mh_map_build the call is synchronous about its verdict and leaves nothing in flight. */
MH_API mh_status mh_map_restore(mh_map* map, const float* x, const float* y, const float* z, const uint32_t* src_idx, size_t n,
                                uint64_t n_offered, int32_t mem);
/* A whole group of key-frames inserted at once: the session map of a recorded drive built from its key-frames without K
 * rebuilds of everything stored (K calls of mh_map_insert gather, re-sort and rebuild the stored content K times).
 *  - Definition.  The map afterwards is bit for bit the map after
 *        for f in 0 .. n_frames-1:  mh_map_insert(map, scan(frames[f]), frames[f].T, 0)
 *    -- the same mh_map_download and mh_map_download_ndt bits, the same n_points / n_offered / n_voxels / n_planes and bounding
 *    box, the same answers from every search route, the same result of a following mh_map_insert.  The source index of point i
 *    of frame f is (n_offered before the call) + sum of n_g over g < f + i.  The cap and min_distance_between_points see the
 *    points of earlier frames as stored ones.  There is no far removal.  (table_size is an implementation matter, as for
 *    mh_map_restore.)
 *  - Composition.  Each point is composed with its frame's pose as mh_map_insert composes it:
 *    (float)(((T0*px + T1*py) + T2*pz) + T3) per row, in fp64, un-fused.
 *  - Passes.  Frames are taken in order into passes of at most max_points_per_pass points (0: the library's default, 2^21 points
 *    = 24 MB of staged coordinates); a frame larger than that is a pass of its own.  Each pass is one upload (host arrays are
 *    packed into a page-locked mirror; device arrays are read in place and only the tables travel), one compose launch over all
 *    its frames behind the stored points, and one rebuild.  By the definition the result does not depend on the pass size; a
 *    small value exists for tests only (as mh_occmap_params::max_keys_per_pass does).
 *  - Arrays live in `mem`: MH_MEM_HOST, MH_MEM_HOST_PINNED or MH_MEM_DEVICE (x, y, z of a frame may be NULL when its n is 0).
 *  - Out-of-range points (|coord| / voxel_size >= 1e6 after composition) are left out and reported as ONE deferred verdict for
 *    the call, by the protocol of mh_map_insert: mh_map_info::deferred_status until the next insertion on this map returns
 *    MH_WARN_PREVIOUS_OUT_OF_RANGE; a verdict pending from an earlier insertion is returned by this call in the same way.
 *  - MH_ERR_INVALID_ARGUMENT before any device work, the map untouched: a NULL map; NULL frames with n_frames > 0; a bad `mem`;
 *    NULL arrays with n > 0; a non-finite pose entry (of an empty frame too); n_frames > MH_MAX_INSERT_FRAMES; totals beyond
 *    mh_map_insert's limits summed over the whole call (stored + offered points >= 0x7FFFFFF0, n_offered + offered >= 0xFFFFFFF0).
 *    (The totals check needs the stored count, so it follows the lazy read-back of the previous update's counts; nothing is
 *    launched, and a pending verdict stays pending.)
 *  - n_frames == 0 or only empty frames: MH_OK, nothing changes.
 *  - A failure in a later pass (out of memory): earlier passes stay inserted and n_offered says how far the call got; the handle
 *    stays usable.  A call that fails has not returned a verdict pending from an earlier insertion: that verdict stays pending,
 *    together with this call's own.  Staging and scratch are reserved before the stored content is touched; should the rebuild itself run out of
 *    memory the map reads as empty, as after a failed mh_map_insert.
 *  - The call returns once the caller's arrays may be reused (device arrays: once the last compose launch has read them); counts
 *    and verdict travel lazily, as for mh_map_insert. */
#define MH_MAX_INSERT_FRAMES 1048576
typedef struct {
  const float *x, *y, *z; /* n points, vehicle frame, arrays in `mem`; may be NULL when n == 0 */
  uint64_t n;
  double T[12];           /* row-major 3x4, the key-frame's pose */
} mh_map_frame;           /* 128 bytes */
MH_API mh_status mh_map_insert_frames(mh_map* map, const mh_map_frame* frames, size_t n_frames, int32_t mem,
                                      uint64_t max_points_per_pass);

/* ------------------------------------------------------------------------------------------------
 * Scan: the local point layer handed to align() ("decimated_for_icp", lidar3d-default.yaml:204),
 * untransformed, in the vehicle frame.
 * ---------------------------------------------------------------------------------------------- */
MH_API mh_status mh_scan_create(mh_ctx* ctx, const float* x, const float* y, const float* z, size_t n, int32_t mem,
                                mh_scan** out);
/* Replace the points (e.g. after the caller re-ran its de-skew, LidarOdometry.cpp:992-999).  `mem` may be
 * MH_MEM_HOST_PINNED (asynchronous upload, see Conventions). */
MH_API mh_status mh_scan_update(mh_scan* scan, const float* x, const float* y, const float* z, size_t n, int32_t mem);
/* Replace the points from an interleaved buffer, the form raw sensor data arrives in: point i has float32 x/y/z at
 * data + i*point_step + off_{x,y,z} and, with off_t >= 0, a float32 time stamp [s] at off_t (a KITTI velodyne .bin is
 * point_step 16 / offsets 0,4,8; a sensor_msgs/PointCloud2 payload gives its own).  This is the step the reference's
 * observations_generator (mp2p_icp_filters::Generator, lidar3d-default.yaml:250-262) performs on the CPU when it turns
 * the raw observation into the SoA 'raw' layer; here: ONE copy of the bytes and a de-interleave kernel.  point_step and
 * the offsets are multiples of 4.  With off_t < 0 the scan carries no time stamps afterwards.  `mem` may be
 * MH_MEM_HOST_PINNED (asynchronous upload, see Conventions). */
MH_API mh_status mh_scan_update_aos(mh_scan* scan, const void* data, size_t n, size_t point_step, size_t off_x,
                                    size_t off_y, size_t off_z, int64_t off_t, int32_t mem);
/* The same, plus an optional float32 intensity at off_i (< 0: none; KITTI / MulRan rows: 12).  mh_scan_update_aos is the
 * off_i = -1 case.  mh_scan_update and mh_scan_update_aos leave a scan without intensity. */
MH_API mh_status mh_scan_update_aos_i(mh_scan* scan, const void* data, size_t n, size_t point_step, size_t off_x,
                                      size_t off_y, size_t off_z, int64_t off_t, int64_t off_i, int32_t mem);
/* Kept for the ABI: checks its arguments (scan, voxel_size > 0) and does nothing else.  It used to queue the scan's search
 * order for the tile matcher, which was removed; the matchers search the scan as it is. */
MH_API mh_status mh_scan_prepare(const mh_scan* scan, float voxel_size);
MH_API mh_status mh_scan_destroy(mh_scan* scan);
MH_API mh_status mh_scan_size(const mh_scan* scan, uint64_t* n);

/* ------------------------------------------------------------------------------------------------
 * Scan pre-processing on the device: the observation filter chain that produces the
 * layers `decimated_for_map` / `decimated_for_icp` from the raw sensor cloud.  Replaces, for the
 * configuration of lidar3d-default.yaml:270-350, mp2p_icp_filters::{FilterAdjustTimestamps,
 * FilterDecimateVoxels(FirstPoint | ClosestToAverage), FilterByRange, FilterBoundingBox, FilterDeskew} [U].
 * ---------------------------------------------------------------------------------------------- */
enum { MH_TS_NONE = 0, MH_TS_MIDDLE_IS_ZERO = 1, MH_TS_EARLIEST_IS_ZERO = 2 }; /* TimestampAdjustMethod (yaml:275) */
enum { MH_BBOX_OFF = 0, MH_BBOX_KEEP_OUTSIDE = 1, MH_BBOX_KEEP_INSIDE = 2 };
/* FilterDecimateVoxels decimate_method [U]: FirstPoint (the shipped lidar3d pipelines, yaml:291) keeps the first point of every
 * voxel in input order; ClosestToAverage (rgbd.yaml:254-278; the commented alternative at lidar3d-default.yaml:292) keeps, per
 * voxel, the point closest to the voxel's mean -- mean = (float sum of the voxel's points in input order) * (1.0f / count),
 * squared error (dx*dx + dy*dy) + dz*dz in float, the first of equally close points. */
enum { MH_DECIMATE_FIRST_POINT = 0, MH_DECIMATE_CLOSEST_TO_AVERAGE = 1 };

typedef struct {
  float decim_map_resolution;    /* FilterDecimateVoxels #1 voxel_filter_resolution (yaml:289); 0 = stage skipped */
  float decim_icp_resolution;    /* FilterDecimateVoxels #2 (yaml:316); 0 = stage skipped */
  uint32_t min_points_to_filter; /* minimum_input_points_to_filter (yaml:290,317): smaller inputs pass undecimated */
  int32_t index_mode;            /* MH_INDEX_FLOOR | MH_INDEX_TRUNC of the decimation grid */
  float range_min, range_max;    /* FilterByRange (yaml:301-302), inclusive; range_max <= 0 = stage skipped */
  float range_center[3];
  int32_t bbox_mode;             /* FilterBoundingBox (yaml:305-310): MH_BBOX_* ; the pipeline keeps the OUTSIDE */
  float bbox_min[3], bbox_max[3];
  int32_t timestamp_method;      /* FilterAdjustTimestamps (yaml:270-276): MH_TS_* ; ignored without time stamps */
  float time_offset;
  int32_t decim_map_method;      /* decimate_method of FilterDecimateVoxels #1: MH_DECIMATE_* (0 = FirstPoint) */
  int32_t decim_icp_method;      /* ... of FilterDecimateVoxels #2 */
} mh_preprocess_params;

/* Attach per-point time stamps [s] (relative to the scan's reference time) to a scan of the same size. */
MH_API mh_status mh_scan_set_timestamps(mh_scan* scan, const float* t, size_t n, int32_t mem);
/* Attach a per-point intensity to a scan of the same size (the optional channel of the intensity filters below).  Every call
 * that derives a layer -- mh_scan_preprocess(_batch), mh_scan_deskew(_pair), mh_scan_curvature, mh_scan_by_intensity --
 * gives its outputs the input's intensity when the input has one: out.i[k] == raw.i[out.src_idx[k]], bit for bit.  Maps,
 * matching and alignment ignore the channel. */
MH_API mh_status mh_scan_set_intensity(mh_scan* scan, const float* i, size_t n, int32_t mem);
/* raw -> decimate(map res) -> by-range -> bounding box -> out_map -> decimate(icp res) -> out_icp (may be NULL).
 * Survivors keep the raw order (upstream's FirstPoint decimation emits them in the iteration order of its hash
 * container, which is implementation-defined: same set, deterministic order here).  The outputs carry adjusted
 * time stamps (when `raw` has them) and each point's index in `raw`; they are the *_skewed layers.
 * A finite point with |coordinate / resolution| >= 1e6 on any axis does not fit the packed voxel key of a decimation:
 * a stage that decimates leaves it out, and the call returns MH_ERR_OUT_OF_RANGE with both outputs complete -- the
 * chain's result for the scan without such points.  A stage that does not decimate (resolution 0, or an input below
 * min_points_to_filter) passes the point like any other, and a non-finite point raises nothing. */
MH_API mh_status mh_scan_preprocess(const mh_scan* raw, const mh_preprocess_params* params, mh_scan* out_map,
                                    mh_scan* out_icp);
/* The same chain for the scans of several sequences at once: every step is ONE launch over all of them, issued on the
 * stream of the first scan's context (work still queued on the other scans' streams is waited for), and one read-back
 * brings all counts -- N sequences in one process cost the host one sequence's launches (the callers' threads contend
 * for the runtime otherwise).  `params` is an array with `params_stride` bytes between entries (0: one set for all);
 * `out_icps` may be NULL, or hold NULL entries.  Outputs are those of n_jobs separate mh_scan_preprocess calls, bit for
 * bit.  Each job's three scans belong to one context; the contexts may differ from job to job (same device).
 * When a job has a point outside the key range (see mh_scan_preprocess) the call returns MH_ERR_OUT_OF_RANGE; the
 * outputs of every job, that one included, are complete and equal to those of their single calls. */
MH_API mh_status mh_scan_preprocess_batch(size_t n_jobs, const mh_scan* const* raws, const mh_preprocess_params* params,
                                          size_t params_stride, mh_scan* const* out_maps, mh_scan* const* out_icps);
/* FilterDeskew (yaml:328-350): p' = Exp_SO3(w*t_i)*p + v*t_i with twist = (vx,vy,vz,wx,wy,wz) in the vehicle frame,
 * fp64, rounded to float [U].  twist == NULL or a scan without time stamps copies the points (skip_deskew /
 * silently_ignore_no_timestamps).  `out` must differ from `in`; it is what align() and mh_map_insert() consume, and
 * `in` stays valid for the re-de-skew inside the ICP loop (LidarOdometry.cpp:992-999) with no host round trip.
 * `in` may belong to another context of the same device (a layer prepared on a second stream whose work the caller
 * has synchronised); the kernel is ordered on `out`'s stream. */
MH_API mh_status mh_scan_deskew(const mh_scan* in, const double twist[6], mh_scan* out);
/* Both layers of a scan (`a`: the large one for the map, `b`: the small one for the ICP) de-skewed by ONE launch, which
 * also leaves the bounding box of the de-skewed `b` -- the input of the sensor-range low-pass that runs next
 * (LidarOdometry.cpp:744, 1515-1545) -- in host memory: one launch and one wait on the per-scan chain instead of
 * mh_scan_deskew x 2 + mh_scan_bbox.  Same results bit for bit; falls back to those calls for copies (twist NULL or no
 * time stamps), empty layers and a `b` above 65536 points. */
MH_API mh_status mh_scan_deskew_pair(const mh_scan* in_a, const mh_scan* in_b, const double twist[6], mh_scan* out_a,
                                     mh_scan* out_b, float bb_min[3], float bb_max[3], uint64_t* n_finite);
/* Axis-aligned bounding box of the finite points (CPointsMap::boundingBox [U], used by the sensor-range estimate at
 * LidarOdometry.cpp:1503-1508, 1517-1534).  n_finite (nullable) = number of finite points; zeros for an empty scan. */
MH_API mh_status mh_scan_bbox(const mh_scan* scan, float bb_min[3], float bb_max[3], uint64_t* n_finite);
/* FilterCurvature [U] (extras/lidar3d-edges.yaml:252-259): splits a layer into points of larger and smaller curvature and
 * the rest.  Upstream's source is not vendored, so this is a restatement; parity with it is unpinned.  The layer carries no
 * ring channel: it is read in storage order (the synthetic sweeps and KITTI / MulRan rows are ring-major).  For a layer of
 * N points p_0..p_{N-1}, in float, unfused, in the order written, every point i in [1, N-2]:
 *   a = p_i - p_{i-1}, b = p_{i+1} - p_i (component-wise);  na = (a.x*a.x + a.y*a.y) + a.z*a.z, nb the same from b;
 *   gap2 = max_gap*max_gap, clr2 = min_clearance*min_clearance;
 *   na > gap2 || nb > gap2             -> other
 *   else na < clr2 || nb < clr2        -> other
 *   else c = ((a.x*b.x + a.y*b.y) + a.z*b.z) / (sqrtf(na) * sqrtf(nb))   (correctly rounded divide and square root)
 *        c < max_cosine                -> larger (output_layer_larger_curvature)
 *        otherwise                     -> smaller (output_layer_smaller_curvature)
 * IEEE comparisons decide as written (a NaN neighbour difference lands in `smaller`).  Points 0 and N-1 are in no output.
 * Each output keeps the input order, carries the input's time stamps when it has them, and src_idx = the input's src_idx[i]
 * when it has one, else i.  Any output may be NULL, not all of them; the outputs differ from `in` and from each other; all
 * scans belong to one context.  Layers of up to 2^21 - 1 points (three 21-bit counters share one 64-bit scan word; larger:
 * MH_ERR_INVALID_ARGUMENT).  Queued on the context's stream; one read-back of the three counts ends the call. */
typedef struct {
  float max_cosine;     /* cosine of the angle between a and b below which a point is a curvature point */
  float min_clearance;  /* [m] a neighbour closer than this: other */
  float max_gap;        /* [m] a neighbour farther than this: other */
} mh_curvature_params;
MH_API mh_status mh_scan_curvature(const mh_scan* in, const mh_curvature_params* p, mh_scan* out_larger, mh_scan* out_smaller,
                                   mh_scan* out_other);
/* FilterNormalizeIntensity [U] (extras/lidar3d-intensity.yaml:260-263), in place on `layer`.  Upstream's source is not
 * vendored: a restatement, parity unpinned.  A layer without intensity: MH_ERR_INVALID_ARGUMENT, the layer untouched.
 *   lo, hi = min and max of the layer's non-NaN intensities;
 *   range: a HOST pointer or NULL.  NULL = remember_intensity_range: false.  Otherwise it holds the remembered {min, max} on
 *     entry ({NaN, NaN}: none yet); lo and hi are widened by it and the result is written back;
 *   no non-NaN value and nothing remembered: the layer and `range` stay unchanged;
 *   d = hi - lo;  k = d > 0 ? 1.0f / d : 0.0f (correctly rounded);
 *   every value I becomes (I - lo) * k, in float, unfused (NaN stays NaN).
 * Queued on the layer's context stream; one wait ends the call. */
MH_API mh_status mh_scan_normalize_intensity(mh_scan* layer, float range[2]);
/* FilterByIntensity [U] (extras/lidar3d-intensity.yaml:265-270): I < low_threshold -> low; else I > high_threshold -> high;
 * else mid (NaN lands in mid).  Each output keeps the input order and carries xyz, time stamps (when the input has them),
 * the intensity, and src_idx = the input's src_idx when it has one, else the input index.  Any output may be NULL, not all of
 * them; the outputs differ from `in` and from each other; all scans belong to one context.  An input without intensity:
 * MH_ERR_INVALID_ARGUMENT, the outputs untouched.  Layers of up to 2^21 - 1 points (the packed counters of
 * mh_scan_curvature, whose scan and scatter this call shares); one read-back of the three counts ends the call. */
typedef struct {
  float low_threshold;   /* values below: output_layer_low_intensity */
  float high_threshold;  /* values above: output_layer_high_intensity */
} mh_by_intensity_params;
MH_API mh_status mh_scan_by_intensity(const mh_scan* in, const mh_by_intensity_params* p, mh_scan* out_low, mh_scan* out_mid,
                                      mh_scan* out_high);
/* GeneratorEdgesFromRangeImage [U] (rgbd.yaml:233-244): turns an organised range image into an `edges` and a `planes` layer.
 * Upstream's source is not vendored, so this is a restatement; parity with it is unpinned.  `range` is row-major rows x cols,
 * R[r, c]; 0 means "no return".  With W = row_window_length:
 *   Classification, per row r, in integers:
 *     pixel (r, c) is scored iff W <= c < cols - W and all 2W+1 samples R[r, c-W .. c+W] are non-zero;
 *     S = (sum of those 2W+1 samples) - (2W+1) * R[r, c]            (exact in int32: |S| <= 128 * 65535)
 *     (float)|S| > score_threshold  -> edges (a strict comparison);  every other scored pixel -> planes;
 *     unscored pixels go to neither layer.
 *   Point of a pixel, in float, unfused, in the order written (correctly rounded divide and square root):
 *     d = (float)R * range_units;  kx = (cx - (float)c) / fx;  ky = (cy - (float)r) / fy;
 *     range_is_depth != 0:  xs = d, ys = d*kx, zs = d*ky            (the MRPT sensor frame: x forward, y left, z up)
 *     otherwise:            xs = (float)((double)d / sqrt((1.0 + (double)kx*kx) + (double)ky*ky)), ys = xs*kx, zs = xs*ky
 *     vehicle frame, P = sensor_pose, coordinate i:  (float)(((P[4i]*xs + P[4i+1]*ys) + P[4i+2]*zs) + P[4i+3])  in fp64.
 *   Order: both layers hold their pixels in row-major pixel order (an order-preserving compaction, as every filter here).
 * The outputs carry no time stamps and no intensity; src_idx = the pixel index r * cols + c.  `edges` or `planes` may be
 * NULL, not both; they differ from each other and belong to `ctx`.  `mem`: MH_MEM_HOST, MH_MEM_DEVICE or MH_MEM_HOST_PINNED
 * (see Conventions).  Refused before any device work, the outputs untouched: MH_ERR_INVALID_ARGUMENT for zero rows or cols,
 * W outside 1..64, fx, fy or range_units not > 0, a negative or non-finite score_threshold, both outputs NULL, a scan of
 * another context; MH_ERR_UNSUPPORTED for more than 2^21 - 1 pixels (the packed counters of mh_scan_curvature, whose scan
 * this call shares).  An image with cols < 2W+1 is valid and yields two empty layers.  Queued on the context's stream; one
 * read-back of the two counts ends the call.  Bitwise reproducible: no float atomics, no waiting between workgroups. */
typedef struct {
  uint32_t rows, cols;        /* > 0 */
  float fx, fy, cx, cy;       /* pinhole intrinsics [px]; fx, fy > 0 */
  float range_units;          /* metres per count, > 0 */
  uint32_t range_is_depth;    /* != 0: the value is the depth along the optical axis; 0: the distance along the ray */
  double sensor_pose[12];     /* sensor on the vehicle, row-major 3x4 */
  uint32_t row_window_length; /* W, 1..64 (rgbd.yaml:244 has 6) */
  float score_threshold;      /* rgbd.yaml:243 has 10; finite, >= 0 */
} mh_range_image_params;
MH_API mh_status mh_scan_edges_from_range_image(mh_ctx* ctx, const uint16_t* range, int32_t mem, const mh_range_image_params* p,
                                                mh_scan* edges, mh_scan* planes);
/* The clouds of the sensors of one rig, each in its own sensor frame, merged into one vehicle-frame layer: what
 * mola::LidarOdometry::onLidarImpl does on the CPU for every observation of a synchronised group (LidarOdometry.cpp:704-721: the
 * generator applies the sensor's pose, FilterAdjustTimestamps runs with that sensor's SENSOR_TIME_OFFSET, merge_with appends).
 * `out` holds the sum of the sources' sizes: source 0's points first in their own order, then source 1's, and so on.  Point j
 * of source k, with P = params[k].sensor_pose and x, y, z promoted to double:
 *   x' = (float)(((P[0]*x + P[1]*y) + P[2]*z) + P[3]);  y' and z' with rows 1 and 2 of P            (fp64, unfused, rounded once)
 *   time stamp, timestamp_method != MH_TS_NONE: tmin_k, tmax_k = min and max over ALL stamps of source k alone, compared as the
 *     order-preserving unsigned image of their bits (-0 below +0), as mh_scan_preprocess takes them;
 *     d = 0.5f*(tmin_k + tmax_k) for MH_TS_MIDDLE_IS_ZERO, tmin_k for MH_TS_EARLIEST_IS_ZERO;  t' = (t - d) + time_offset, in float
 *   time stamp, MH_TS_NONE: t' = t.   Intensity: copied.
 * `out` carries time stamps only when every non-empty source does (a mix: MH_ERR_INVALID_ARGUMENT), and intensity likewise; it
 * carries no src_idx, as after mh_scan_update_aos_i.  Empty sources are legal and contribute
 * nothing; a source may appear more than once.  Refused with a message (mh_last_error_string) before any device work, `out`
 * untouched, all MH_ERR_INVALID_ARGUMENT: n_sources 0 or above MH_MAX_MERGE_SOURCES, a NULL pointer, `out` among the sources,
 * scans of different contexts, a bad timestamp_method, a total of 2^31 - 16 points or more.  Asynchronous on the context's
 * stream like mh_scan_deskew: the host knows the output size, nothing is read back.  At most two launches (the min / max of
 * the stamps, skipped when no source adjusts its stamps; the fill) and one small copy, whatever n_sources is. */
#define MH_MAX_MERGE_SOURCES 8
typedef struct {
  double sensor_pose[12];   /* the sensor on the vehicle, row-major 3x4 */
  int32_t timestamp_method; /* MH_TS_*, applied to THIS source's stamps alone */
  float time_offset;        /* this source's SENSOR_TIME_OFFSET; ignored with MH_TS_NONE, as in mh_scan_preprocess */
} mh_merge_source;          /* 104 bytes */
MH_API mh_status mh_scan_merge_sensors(size_t n_sources, const mh_scan* const* sources, const mh_merge_source* params,
                                       mh_scan* out);
/* Copy a scan to HOST arrays (any may be NULL; t / src_idx are zero-filled when the scan has none). */
MH_API mh_status mh_scan_download(const mh_scan* scan, float* x, float* y, float* z, float* t, uint32_t* src_idx);
/* Copy a scan's intensity to a HOST array of n entries; MH_ERR_INVALID_ARGUMENT when the scan carries none. */
MH_API mh_status mh_scan_download_intensity(const mh_scan* scan, float* i);

/* ------------------------------------------------------------------------------------------------
 * Matcher-granular path.  Replaces mp2p_icp::Matcher_Points_DistanceThreshold::implMatchOneLayer [U]
 * (lidar3d-default.yaml:195-204; pairingsPerPoint 1, allowMatchAlreadyMatchedGlobalPoints true) on
 * top of NearestNeighborsCapable::nn_single_search [U]: p' = (float)(R*l+t); NN over the 3x3x3 voxel
 * block around voxel(p'); accepted iff d^2 < thr^2 + ang^2*|p'|^2.  Output = mp2p_icp::Pairings::
 * paired_pt2pt [U] as SoA, compacted in ascending local index.  Output arrays hold scan-size entries,
 * live in `mem`, and any of them may be NULL.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  uint32_t* local_idx;
  uint32_t* global_idx;
  float* gx;
  float* gy;
  float* gz;
  float* d2; /* errorSquareAfterTransformation */
} mh_pairs_out;

typedef struct {
  uint64_t n_pairs;
  uint64_t potential_pairings; /* Pairings::potential_pairings [U] = scan size * pairingsPerPoint */
} mh_match_info;

MH_API mh_status mh_nn_search(const mh_map* map, const mh_scan* scan, const double T[12], double threshold,
                              double threshold_angular_deg, const mh_pairs_out* out, int32_t mem,
                              mh_match_info* info);
/* The same matcher with pairingsPerPoint = k > 1 (rgbd.yaml:135-141) on NearestNeighborsCapable::nn_multiple_search [U]
 * ("same scan keeping k best sorted"): per local point the k nearest map points of the 27-voxel block in
 * ascending (d^2, scan position), accepted in that order while d^2 < thr^2 + ang^2*|p'|^2.  Pairs in ascending local index, a
 * point's pairs in ascending distance; output arrays hold scan-size * k entries; potential_pairings = scan size * k.
 * pairings_per_point 1 is mh_nn_search. */
#define MH_MAX_PAIRINGS_PER_POINT 8
MH_API mh_status mh_nn_search_k(const mh_map* map, const mh_scan* scan, const double T[12], double threshold,
                                double threshold_angular_deg, uint32_t pairings_per_point, const mh_pairs_out* out,
                                int32_t mem, mh_match_info* info);
/* Un-compacted variant: one entry per scan point; global_idx = 0xFFFFFFFF where nothing was found in
 * the 27-voxel block (no threshold applied).  Arrays hold scan-size entries; any may be NULL. */
MH_API mh_status mh_nn_search_dense(const mh_map* map, const mh_scan* scan, const double T[12], uint32_t* global_idx,
                                    float* gx, float* gy, float* gz, float* d2, int32_t mem);

/* Radius search: mrpt::maps::NearestNeighborsCapable::nn_radius_search [U] on the hashed voxel map, batched over a scan -- the
 * one neighbour query with a VARIABLE number of results per point.  Upstream's source is not vendored, so parity with it is
 * unpinned [U] as for every other map query; what follows is the specification.
 *  - The query point of scan point l is p' = (float)(R*l + t), as in every other search.
 *  - Its results are EVERY stored map point (x, y, z) with d2 < r2, where dx = x - p'x (dy, dz alike),
 *    d2 = (dx*dx + dy*dy) + dz*dz in fp32, un-fused, and r2 = (float)(radius * radius) with the square taken in fp64.  The
 *    comparison is strict: d2 == r2 is out.  The set is defined over all stored points; which voxels are visited is an
 *    implementation matter (a conservative block around voxel_of(p' -+ radius) per axis, widened against fp32 rounding:
 *    extra voxels cost time and never change results).
 *  - Order.  MH_RADIUS_VISIT_ORDER: the map's storage order -- voxels ascending in (kx, ky, kz), insertion order inside a
 *    voxel.  That is the order of mh_map_download, so a point's results are a subsequence of the download.
 *    MH_RADIUS_SORTED: ascending (d2, visit position); the first result of a point is then mh_nn_search_dense's answer
 *    whenever that answer lies within the radius.
 *  - Both index modes.  On an NDT map the two statistics records of a voxel are never results.
 *  - A non-finite p', or one with |p' / voxel_size| >= 1e6 on any axis (the guard of the other searches), has no results.  A
 *    voxel of the block whose index leaves the key range is skipped.
 *  - Outputs.  The arrays of mh_radius_out live in `mem` (MH_MEM_HOST or MH_MEM_DEVICE); any may be NULL, and so may `out`.
 *    `offsets` (scan size + 1 entries; the results of point i are entries [offsets[i], offsets[i+1])) and `info` are always
 *    filled; max_per_query is the largest result count of any point.  The result arrays are written only if
 *    capacity >= n_results, and then n_written = n_results; otherwise n_written = 0, they are not touched, and the status is
 *    still MH_OK: a count-only first call (capacity 0) and a sized second call are the intended use.
 *  - The call blocks like mh_nn_search_dense and orders itself behind a queued mh_map_insert.  An empty scan: MH_OK, offsets[0] = 0.
 *  - Refusals, all decided before anything is queued: MH_ERR_INVALID_ARGUMENT for a NULL map, scan, T or info, a bad `mem`, a
 *    non-finite pose, a radius that is not finite or not > 0, unknown flag bits, map and scan on different devices;
 *    MH_ERR_UNSUPPORTED for radius > MH_RADIUS_MAX_VOXELS x voxel_size (a block wider than 8 voxels per axis).
 *    MH_ERR_UNSUPPORTED also for a total of 2^32 results or more (known once they are counted; info holds the count). */
enum { MH_RADIUS_VISIT_ORDER = 0, MH_RADIUS_SORTED = 1 };
#define MH_RADIUS_MAX_VOXELS 3
typedef struct {       /* arrays live in `mem`; any may be NULL */
  uint32_t* offsets;    /* scan size + 1 entries: results of point i are [offsets[i], offsets[i+1]) */
  uint32_t* global_idx; /* source index of the map point, as the other searches report it */
  float *gx, *gy, *gz, *d2;
  uint64_t capacity;    /* entries each result array can hold */
} mh_radius_out;
typedef struct {
  uint64_t n_results, n_written;
  uint32_t max_per_query, reserved_;
} mh_radius_info;
MH_API mh_status mh_nn_search_radius(const mh_map* map, const mh_scan* scan, const double T[12], double radius, uint32_t flags,
                                     const mh_radius_out* out, int32_t mem, mh_radius_info* info);

/* Pose-candidate scoring: how well does one scan fit one map under each of MANY candidate poses -- the data-parallel core of a
 * relocalization (a grid of starts around a coarse pose, scored before the best few are refined by ICP).  One launch scores
 * every candidate; everything is exact, there are no tolerances.
 *  - Per candidate c (poses + 12 * c: row-major 3x4, fp64, HOST memory) and scan point l: p' = (float)(R_c*l + t_c) exactly as
 *    in every other search; the neighbour is mh_nn_search_dense's answer, the first minimum over the 27-voxel block.
 *  - Acceptance is mh_nn_search's own test: thr2 = (float)(threshold * threshold), ang = threshold_angular_deg * pi / 180,
 *    ang2 = (float)(ang * ang) (both squares in fp64); accepted iff a neighbour was found and d2 < thr2 + ang2 * |p'|^2, with
 *    |p'|^2 = (px*px + py*py) + pz*pz, all in fp32, un-fused.
 *  - n_paired = the number of accepted points.  cost = the sum over the accepted points of
 *    q = (d2 * qscale >= 16777215.0f) ? 0xFFFFFF : (uint32_t)(d2 * qscale),  qscale = (float)(1048576.0 / (double)thr2):
 *    one fp32 multiply, truncation -- a quantised squared residual in units of thr2 / 2^20.  An integer sum does not depend on
 *    the order of summation, so scores are bit-identical from run to run and between any two implementations (which an fp64
 *    sum of d2 would not be).
 *  - A non-finite p', or one with |p' / voxel_size| >= 1e6 on any axis, pairs with nothing.  On an NDT map the statistics
 *    records are never neighbours.  Both index modes.
 *  - `scores` holds n_poses entries in `mem` (MH_MEM_HOST or MH_MEM_DEVICE); reserved_ is 0.  The call orders itself behind a
 *    queued mh_map_insert and blocks until the scores are in `mem`.  n_poses == 0 or an empty scan: MH_OK, zeroed scores.
 *  - Refusals, all decided before anything is queued: MH_ERR_INVALID_ARGUMENT for a NULL map, scan or scores, NULL poses with
 *    n_poses > 0, a bad `mem`, map and scan on different devices, any non-finite pose entry, a threshold that is not finite or
 *    outside [1e-3, 1e3] m, a negative or non-finite angular threshold; MH_ERR_UNSUPPORTED for n_poses > MH_SCORE_MAX_POSES. */
#define MH_SCORE_MAX_POSES 1048576
typedef struct {
  uint32_t n_paired;
  uint32_t reserved_;
  uint64_t cost;
} mh_pose_score; /* 16 bytes */
MH_API mh_status mh_score_poses(const mh_map* map, const mh_scan* scan, const double* poses, size_t n_poses, double threshold,
                                double threshold_angular_deg, mh_pose_score* scores, int32_t mem);

/* Place recognition by a polar height descriptor (in the manner of Scan Context): from "this scan" to "these few stored frames
 * look like it, under this yaw" -- the coarse pose a relocalization needs when nobody supplies one.  A descriptor is R rings x S
 * sectors of bytes around the vehicle, desc[ring * S + sector], each the quantised height of the highest point of its bin (0:
 * empty).  Everything is integer or compare-only fp32: results are exact and do not depend on the order of the points.
 *
 * THE DESCRIPTOR (this text is the specification; tests/place_ref.py restates it in numpy and every byte must agree).  No
 * transcendental function runs on the device; every boundary comes from a table the host builds in fp64 and rounds once to
 * fp32; all point arithmetic is un-fused fp32.
 *  - Parameters: R = n_rings in [1, MH_PLACE_MAX_RINGS]; S = n_sectors, a multiple of 8 in [8, MH_PLACE_MAX_SECTORS];
 *    0 <= min_range < max_range; z_min < z_max; all values finite (and the tables below finite in fp32).
 *  - Host tables: ring_edge2[k] = (float)(e_k * e_k), e_k = min_range + k * (max_range - min_range) / R in fp64, k = 0..R;
 *    tan_edge[j] = (float)tan(2 * pi * j / S), j = 1..S/8-1;  zscale = (float)(254.0 / ((double)z_max - (double)z_min)).
 *  - A point (x, y, z) is skipped when a coordinate is non-finite; when x = y = 0; when r2 = x*x + y*y lies outside
 *    [ring_edge2[0], ring_edge2[R]); when z lies outside [z_min, z_max).
 *  - ring = the number of k in 1..R-1 with ring_edge2[k] <= r2.
 *  - level = min(255, 1 + (uint32)((z - z_min) * zscale)): one subtraction, one multiplication, a truncation.
 *  - sector, by quarter turns; each case gives a > 0 and b >= 0:
 *        x > 0 and y >= 0: Q = 0, (a, b) = (x, y);        x <= 0 and y > 0: Q = 1, (a, b) = (y, -x);
 *        x < 0 and y <= 0: Q = 2, (a, b) = (-x, -y);      x >= 0 and y < 0: Q = 3, (a, b) = (-y, x).
 *    With E = S / 8:  if b < a:  o = #{j in 1..E-1 : b >= tan_edge[j] * a};  otherwise  o = (2E - 1) - #{j : a > tan_edge[j] * b}.
 *    sector = Q * (S / 4) + o.  This is floor(atan2(y, x) * S / 2pi) mod S away from the boundaries; axes and diagonals lie on
 *    the closed lower end of their sector.
 *  - A bin holds the maximum level of its points.
 *  - Binding property: turning every point by an exact quarter turn, (x, y) -> (-y, x), shifts the descriptor by exactly S/4
 *    columns: desc'[r][(c + S/4) mod S] = desc[r][c].
 *
 * THE SEARCH.  For the stored descriptor d_k and the query q,  D(k, s) = sum over r, c of | q[r][(c + s) mod S] - d_k[r][c] |;
 * out[k] = {shift, dist} is the smallest D(k, .) and the smallest s that attains it.  D <= 32 * 128 * 255 < 2^20.  With this sign
 * a query taken by a vehicle turned by yaw psi against the stored frame gives shift ~ -psi * S / 2pi (mod S).
 *
 *  - mh_place_describe: the descriptor of one scan, n_rings * n_sectors bytes in `mem`.  An empty scan gives all zeros.
 *  - mh_place_db_create / _destroy / _size: a database of descriptors of one parameter set on the context's device.
 *  - mh_place_db_add: appends n_desc ready descriptors (n_desc * R * S bytes in `mem`); n_desc == 0 changes nothing.
 *  - mh_place_db_add_frames: bit for bit the loop  for f: mh_place_describe(scan(frames[f])); mh_place_db_add  -- in passes of
 *    one upload and one flat launch over all points of the pass, as mh_map_insert_frames.  frames[f].T is ignored; an empty
 *    frame appends an all-zero descriptor; x, y, z may be NULL when n is 0.  Device arrays live on the database's device.
 *  - mh_place_search: `out` holds mh_place_db_size entries in `mem`, `query` R * S bytes in `query_mem`.  An empty database:
 *    MH_OK, nothing is written.
 *  - `mem`: MH_MEM_HOST, MH_MEM_HOST_PINNED or MH_MEM_DEVICE.  Every call orders itself on the context's stream and blocks
 *    until its output is in `mem` (and the caller's arrays may be reused).
 *  - Refusals, all decided before any device work, the database untouched: MH_ERR_INVALID_ARGUMENT for NULL handles or arrays
 *    (NULL point arrays with n > 0), a bad `mem`, parameters outside the ranges above; MH_ERR_UNSUPPORTED when the database
 *    would hold more than MH_PLACE_MAX_DESCRIPTORS descriptors.  (No entry point takes both a scan and a database, so there
 *    is no pair of handles that could live on different devices.) */
#define MH_PLACE_MAX_RINGS 32
#define MH_PLACE_MAX_SECTORS 128
#define MH_PLACE_MAX_DESCRIPTORS 1048576
typedef struct {
  uint32_t n_rings, n_sectors;
  float min_range, max_range, z_min, z_max;
} mh_place_params; /* 24 bytes */
typedef struct {
  uint32_t shift, dist;
} mh_place_match; /* 8 bytes */
typedef struct mh_place_db mh_place_db;
MH_API mh_status mh_place_describe(const mh_scan* scan, const mh_place_params* params, uint8_t* desc, int32_t mem);
MH_API mh_status mh_place_db_create(mh_ctx* ctx, const mh_place_params* params, mh_place_db** out);
MH_API mh_status mh_place_db_destroy(mh_place_db* db);
MH_API mh_status mh_place_db_size(const mh_place_db* db, uint64_t* n);
MH_API mh_status mh_place_db_add(mh_place_db* db, const uint8_t* desc, size_t n_desc, int32_t mem);
MH_API mh_status mh_place_db_add_frames(mh_place_db* db, const mh_map_frame* frames, size_t n_frames, int32_t mem);
MH_API mh_status mh_place_search(const mh_place_db* db, const uint8_t* query, int32_t query_mem, mh_place_match* out, int32_t mem);

/* Replaces mp2p_icp::Matcher_Point2Plane::implMatchOneLayer [U] on a mola::NDT [U] map (lidar3d-ndt.yaml:195-200,
 * 236-254).  The upstream semantics are unverified (SURVEY App.B U10); implemented default: among
 * the planar voxels of the 3x3x3 block around voxel(p') the one with the nearest centroid is taken (fp32 d^2, first
 * minimum in scan order) and the pairing {centroid, normal, local point} is emitted iff |n.(p'-c)| < distance_threshold.
 * Needs a map built with ndt_max_eigen_ratio > 0.  Output = Pairings::paired_pt2pl [U] as SoA, ascending local index. */
typedef struct {
  uint32_t* local_idx;
  float *cx, *cy, *cz; /* plane centroid */
  float *nx, *ny, *nz; /* plane unit normal */
} mh_pairs_pl_out;

/* What Matcher_Point2Plane.distanceThreshold (lidar3d-ndt.yaml:197) is compared with -- SURVEY App.B U10, a run-time
 * switch until the reference decides it: the point-to-plane distance |n.(p'-c)| (default) or the distance to the
 * plane's centroid |p'-c| (fp32 squares, un-fused).  The search for the nearest planar voxel is the same. */
enum { MH_PT2PL_PLANE_DISTANCE = 0, MH_PT2PL_CENTROID_DISTANCE = 1 };
/* Matcher_Points_Base::allowMatchAlreadyMatchedPoints [U] (default false upstream, not set by either target pipeline): a
 * matcher skips the local points an earlier matcher of the same iteration has paired.  In lidar3d-ndt.yaml:195-210 that keeps
 * plane-paired points out of Matcher_Points_DistanceThreshold.  Unverified (U12), hence a switch; PAIR_AGAIN is what rounds
 * 1-3 did and stays the default until the reference decides (MOLA_HIP_MATCHED_POINTS=skip|again in the host layers). */
enum { MH_MATCHED_POINTS_PAIR_AGAIN = 0, MH_MATCHED_POINTS_SKIP = 1 };
/* Matcher_Points_DistanceThreshold::allowMatchAlreadyMatchedGlobalPoints [U] (default FALSE upstream; every reference pipeline
 * writes true): with false a matcher runs serially and a point of a global layer is paired once per ICP iteration, by the first
 * candidate in matching order; the "already paired" bits (MatchState::globalPairedBitField) live for one iteration and are shared
 * by its matchers.  Unverified (U13).  Not a switch but a per-pair option: mh_layer_pair_opts::unique_global of
 * mh_icp_align_layers_opts (below), which states the semantics; the other alignment entry points pair a map point as often as it
 * is nearest.  The host layers set it from the pipeline's key; the mirror classes' default stays true. */

MH_API mh_status mh_nn_search_pt2pl(const mh_map* map, const mh_scan* scan, const double T[12], double distance_threshold,
                                    uint32_t mode, const mh_pairs_pl_out* out, int32_t mem, mh_match_info* info);
/* The same matcher on a map WITHOUT plane statistics -- a mola::HashedVoxelPointCloud layer, /root/reference/pipelines/rgbd.yaml:143-151
 * (distanceThreshold 0.40, planeEigenThreshold 1e-2, searchRadius 0.80, knn 10, minimumPlanePoints 6); SURVEY 8a row a13 "otherwise
 * KNN + PCA" [U]: per transformed local point the knn nearest map points of the 27-voxel block (nn_multiple_search [U]), those
 * with d^2 < searchRadius^2 (a prefix: ascending distances), none if fewer than max(3, minimumPlanePoints); mean + covariance of
 * them (fp64), eigenvalues e0 <= e1 <= e2; a plane iff e2 > 0 and e0 <= planeEigenThreshold * e2; normal = unit eigenvector of e0
 * (sign: largest component positive -- the residual and its Jacobian are even in n); pairing {centroid, normal, local point} iff
 * |n.(p'-c)| <= distanceThreshold.  Output as mh_nn_search_pt2pl; works on any map (the NDT statistics, if any, are not used). */
#define MH_MAX_PLANE_KNN 16
typedef struct {
  double distance_threshold;      /* [m] */
  double plane_eigen_threshold;   /* e0 / e2 */
  double search_radius;           /* [m] */
  uint32_t knn;                   /* 3 .. MH_MAX_PLANE_KNN */
  uint32_t minimum_plane_points;  /* >= 3 */
} mh_pt2pl_knn_params;
MH_API mh_status mh_nn_search_pt2pl_knn(const mh_map* map, const mh_scan* scan, const double T[12], const mh_pt2pl_knn_params* params,
                                        const mh_pairs_pl_out* out, int32_t mem, mh_match_info* info);

/* ------------------------------------------------------------------------------------------------
 * Solver-granular path.  Replaces mp2p_icp::Solver_GaussNewton::impl_optimal_pose /
 * optimal_tf_gauss_newton [U] (lidar3d-default.yaml:184-190): robust-weighted point-to-point (3-row)
 * and point-to-plane (1-row) terms, optional prior factor (LidarOdometry.cpp:859-875), 6x6 LDL^T,
 * T <- T (+) exp(delta), repeated max_inner_iterations times on the same pairings.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  const float *lx, *ly, *lz; /* local (untransformed) */
  const float *gx, *gy, *gz; /* global */
  size_t n;
} mh_pairs_pt2pt;

typedef struct {
  const float *lx, *ly, *lz; /* local point */
  const float *cx, *cy, *cz; /* plane centroid */
  const float *nx, *ny, *nz; /* plane unit normal */
  size_t n;
} mh_pairs_pt2pl;

typedef struct {
  double mean[12]; /* prior pose (CPose3DPDFGaussianInf::mean) */
  double info[36]; /* 6x6 information matrix, row-major (cov_inv) */
} mh_prior;

typedef struct {
  uint32_t max_inner_iterations; /* Solver_GaussNewton maxIterations (yaml:187) */
  uint32_t robust_kernel;        /* MH_KERNEL_* (yaml:188) */
  double robust_kernel_param;    /* yaml:190 */
  double min_delta;              /* inner early exit, 1e-7 */
  double max_cost;               /* "target error" early exit, 0 */
  double weight_pt2pt;           /* 1.0 */
  double weight_pt2pl;           /* 1.0 */
} mh_gn_params;

typedef struct {
  double H[36];
  double g[6];
  double err_norm_sqr;
  double delta[6];
  double T_after[12];
} mh_gn_step;

/* T_io: linearisation point in (SolverContext::guessRelativePose [U]), solution out.
 * `n_steps` receives the number of solves performed; `trace` (nullable) holds max_inner_iterations
 * entries.  Returns MH_OK with *solver_ok = 0 when the 6x6 solve produced non-finite values. */
MH_API mh_status mh_gn_solve(mh_ctx* ctx, const mh_pairs_pt2pt* pt2pt, const mh_pairs_pt2pl* pt2pl, int32_t mem,
                             const mh_gn_params* params, const mh_prior* prior, double T_io[12], int32_t* n_steps,
                             int32_t* solver_ok, mh_gn_step* trace);

/* Replaces mp2p_icp::covariance() [U] (result consumed at LidarOdometry.cpp:1009,1035-1036,2090):
 * central-difference Jacobian of the stacked residuals wrt (x,y,z,yaw,pitch,roll) -- steps findif_xyz for the first three
 * columns, findif_ang for the last three -- cov = (A^T A)^-1; diag(1e6) when there are no pairings or A^T A is singular.
 * Singular means singular to working precision: a Cholesky pivot of A^T A not above 1e-10 of its diagonal entry (the differences
 * carry rounding into A, so a pivot that is exactly zero -- fewer than six rows, two point pairings -- arrives as a tiny number
 * of either sign).
 * [U] The pairings enter unweighted: a point pairing gives three rows and a plane pairing one, whatever
 * mh_gn_params::weight_pt2pt / weight_pt2pl were during the alignment (upstream's covariance() takes the pairings and the
 * pose, no weights).  The fused path (mh_icp_result::cov) is this function of the final pose and pairings. */
MH_API mh_status mh_covariance(mh_ctx* ctx, const mh_pairs_pt2pt* pt2pt, const mh_pairs_pt2pl* pt2pl, int32_t mem,
                               const double T[12], double findif_xyz, double findif_ang, double cov[36]);

/* ------------------------------------------------------------------------------------------------
 * Fused path.  Replaces mp2p_icp::ICP::align [U] as called at LidarOdometry.cpp:961-962 with the
 * pipeline of lidar3d-default.yaml:162-209 (one Matcher_Points_DistanceThreshold, one
 * Solver_GaussNewton, QualityEvaluator_PairedRatio).  The whole loop -- match, accumulate, 6x6 solve,
 * stall test, hook test, quality, covariance -- runs on the device; the host only enqueues kernels and
 * polls a termination flag every `poll_every` iterations.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  uint32_t max_iterations;      /* mp2p_icp::Parameters::maxIterations (yaml:173) */
  double min_abs_step_trans;    /* yaml:174 */
  double min_abs_step_rot;      /* yaml:175 */
  uint32_t disable_stall_test;  /* 1: run exactly max_iterations (BASELINE configs[1]) */
  /* Per-iteration values of the run-time formulas of yaml:198 (matcher threshold) and yaml:190
   * (robust kernel parameter), indexed by ICP_ITERATION; HOST arrays of max_iterations entries. */
  const double* threshold;
  const double* kernel_param;
  double threshold_angular_deg; /* yaml:200 */
  /* NULL, or max_iterations values of Matcher_Point2Plane.distanceThreshold (lidar3d-ndt.yaml:197): that matcher
   * then runs before the point matcher in every iteration and both pairing sets go to one solve (ndt yaml:195-210). */
  const double* pt2pl_threshold;
  mh_gn_params gn;              /* robust_kernel_param ignored (kernel_param[k] is used) */
  /* Device-side equivalent of the in-tree iteration hook (LidarOdometry.cpp:923-952): request a stop
   * when the pose has moved more than hook_min_trans [m] or hook_min_rot [rad] from hook_checkpoint. */
  uint32_t hook_enabled;
  double hook_min_trans;
  double hook_min_rot;
  double hook_checkpoint[12];
  uint32_t compute_covariance;
  double cov_findif_xyz;        /* 1e-7 */
  double cov_findif_ang;        /* 1e-7 */
  uint32_t poll_every;          /* ICP iterations enqueued between host polls of the done flag; 0 = automatic: the
                                   first chunk as long as the context's previous alignment of the same kind ran (a fresh
                                   call and a re-entry after a hook request are predicted separately, see
                                   expected_iterations), then short ones */
  uint32_t expected_iterations; /* with poll_every = 0: the caller's own estimate of how many iterations this call will
                                   run (e.g. what its previous call of the same kind ran), 0 = let the library predict */
  uint32_t pt2pl_mode;          /* MH_PT2PL_* : the acceptance test of the point-to-plane matcher (with pt2pl_threshold) */
  uint32_t matched_points;      /* MH_MATCHED_POINTS_* : what the point matcher does with local points that the point-to-plane
                                   matcher of the same iteration has paired (with pt2pt_threshold) */
  uint32_t profile;             /* 1: time every match kernel with HIP events on the context stream (such a job is
                                   enqueued kernel by kernel instead of replaying the captured graph); 2: in
                                   mh_icp_align_batch, do that for job 0 only (lock step: its share of the launches) */
} mh_icp_params;

typedef struct {
  double T[12];
  uint32_t n_pairs;
  double threshold;
  double kernel_param;
  double delta_trans; /* |log(T_prev^-1 T_new)| translation part */
  double delta_rot;
} mh_icp_iter;

typedef struct {
  double T[12];                /* Results::optimal_tf.mean */
  double cov[36];              /* Results::optimal_tf.cov (x,y,z,yaw,pitch,roll) */
  double quality;              /* Results::quality (PairedRatio) */
  uint32_t n_iterations;       /* Results::nIterations */
  uint32_t termination_reason; /* Results::terminationReason, MH_TERM_* */
  uint32_t n_final_pairs;
  uint64_t potential_pairings;
  /* profile == 1 only: */
  uint32_t n_match_launches;
  double match_kernel_ms;      /* sum of the match kernel durations */
  double total_ms;             /* stream time of the whole align */
  uint32_t n_final_pairs_pt2pl; /* how many of n_final_pairs are point-to-plane */
  /* host-side bookkeeping of the device loop (what a latency budget wants to know): */
  uint32_t n_host_polls;          /* times the host waited for the device loop (1 = the first chunk was long enough) */
  uint32_t n_enqueued_iterations; /* iterations worth of kernels enqueued; those beyond the executed ones were early-exit launches */
} mh_icp_result;

/* `trace` (nullable, HOST, max_iterations entries) receives one record per executed iteration;
 * `final_pairs` (nullable, arrays in `pairs_mem`, scan-size entries) receives Results::finalPairings. */
MH_API mh_status mh_icp_align(const mh_map* map, const mh_scan* scan, const mh_icp_params* params,
                              const double T_guess[12], const mh_prior* prior, mh_icp_result* result,
                              mh_icp_iter* trace, const mh_pairs_out* final_pairs, int32_t pairs_mem);

/* Scheduling hint for callers that merge the alignments of several sequences into mh_icp_align_batch calls: *yes = 1 when a
 * single mh_icp_align of this scan with these parameters would run its whole loop in ONE kernel launch (layers of at most 2560
 * points under automatic loop control, see mh_debug_loop_stats) AND the loops of `concurrent_callers` such callers fit into
 * 70 % of the device's CUs together (four 1400-point layers on 256 CUs; the callers' other stages run beside the loops).  Such an alignment is better issued on its own at once than held
 * back for a lock-step batch (4 sequences of the default pipeline: 4450 against 3620 scans/s); with more callers than fit,
 * lock-step batches are faster (8 sequences: 4950 against 4100).  Results do not depend on the choice. */
MH_API mh_status mh_icp_align_prefers_solo(const mh_scan* scan, const mh_icp_params* params, uint32_t concurrent_callers,
                                           int32_t* yes);

/* Statistics (process-wide, no effect on results): single alignments of small layers (<= 2560 points) run their whole loop
 * in ONE kernel launch whose workgroups exchange partial sums among themselves, as long as the workgroups of all such loops
 * running on the device fit its CUs; `loops_started` counts them, `loops_abandoned` those whose workgroups gave up waiting for
 * each other and that were run again launch by launch (same result bit for bit; expected to stay 0).  Either may be NULL. */
MH_API void mh_debug_loop_stats(uint64_t* loops_started, uint64_t* loops_abandoned);

/* Statistics (process-wide, no effect on results): launches of the plan / scan matcher (large layers, MH_MATCH=f) that went to the
 * device so far, by kernel: launches[0] k_match_flat with 32-bit byte offsets, [1] k_match_flat with 64-bit offsets (a map buffer
 * above 2^32 bytes, a scan above 2^28 points, or MH_NO_OFF32=1), [2] and [3] the same for k_match_flat_b, the lock-step batches'.
 * They count what ran, not what was decided: a launch replayed from a captured graph counts each time that graph is launched.
 * The two instantiations give the same bits; the test suite reads these counters to know which one it has checked. */
MH_API void mh_debug_flat_stats(uint64_t launches[4]);

/* Always 0.  It used to tell the development library from the shipped one; the development library no longer exists: the matcher
 * families it carried -- MH_MATCH=t (tile matcher, map records staged in LDS), w (wave matcher), o (sorted scan) -- lost to the
 * product kernels and were removed, and mh_icp_align / mh_icp_align_batch reject those three letters. */
MH_API int32_t mh_debug_dev_variants(void);

/* Results::finalPairings.paired_pt2pl [U] of the LAST mh_icp_align run on `scan`'s context (arrays in `mem`, scan-size
 * entries, any may be NULL). */
MH_API mh_status mh_icp_get_pt2pl_pairs(const mh_scan* scan, const mh_pairs_pl_out* out, int32_t mem, uint64_t* n_pairs);

/* Many independent alignments from one host thread, one context per job.  Job i uses maps[i], scans[i] (distinct
 * contexts), params[i] when params_per_job != 0 (else the one *params: N sequences have N adaptive thresholds, iteration
 * budgets and hook check points), guesses + 12*i, priors[i] (array or entries may be NULL), and writes results[i]; every
 * result is bitwise what mh_icp_align gives for that job alone.  Jobs that run the same kernel chain advance in LOCK
 * STEP: each kernel of an iteration is one launch over all of them (the jobs' tails fill each other's idle lanes) --
 * large layers (quad / plan-scan matcher), 8-12 k-point layers (row matcher with the fused accumulation), layers up to 8 k
 * points (k_step16: search + sums per launch, the Gauss-Newton step carried into the next launch; also with
 * Matcher_Point2Plane on NDT maps); the rest is interleaved, one stream per job.  With profile = 2, job 0's match_kernel_ms is its share of the lock-step match
 * launches.  Work still queued on the jobs' own streams (asynchronous uploads, de-skew, filters) is ordered before the
 * batch, whichever stream the batch runs on.
 *
 * `pairs_block` (nullable): Results::finalPairings of every job.  Job i's part starts at byte offset
 * sum_{j<i} mh_pairs_block_bytes(scan size of job j) and holds six arrays of S = mh_pairs_block_bytes(n)/24 entries
 * each -- local_idx | global_idx (uint32) | gx | gy | gz | d2 (float) -- of which the first
 * results[i].n_final_pairs - results[i].n_final_pairs_pt2pl are valid, ascending local index.  `pairs_mem`:
 * MH_MEM_DEVICE, MH_MEM_HOST, or MH_MEM_HOST_PINNED: the download is then queued on a copy stream of the first job's
 * context and the call returns without waiting for it (it overlaps the next batch); mh_ctx_synchronize(scans[0]'s
 * context) waits for it, and so does the next batch before it overwrites the device-side staging. */
MH_API size_t mh_pairs_block_bytes(size_t n_scan_points);
MH_API mh_status mh_icp_align_batch(size_t n_jobs, const mh_map* const* maps, const mh_scan* const* scans,
                                    const mh_icp_params* params, int32_t params_per_job, const double* T_guesses,
                                    const mh_prior* const* priors, mh_icp_result* results, void* pairs_block,
                                    int32_t pairs_mem);

/* Fused path over several point-layer pairs.  Replaces mp2p_icp::ICP::align [U] with an ICP block of one or more
 * Matcher_Points_DistanceThreshold whose pointLayerMatches hold several {global, local, weight} entries and one
 * Solver_GaussNewton (pipelines/extras/lidar3d-dual-map.yaml:115-132, lidar3d-edges.yaml:120-129; pairingsPerPoint 1; matchers with
 * allowMatchAlreadyMatchedGlobalPoints false: mh_icp_align_layers_opts, with runFromIteration / runUpToIteration gates
 * (lidar3d-near-far.yaml:183): mh_icp_align_layers_gated, both below).
 *  - Matching: in every ICP iteration k, pair i runs the matcher of mh_nn_search on (map_i, scan_i): the 27-voxel exact search,
 *    accepted iff d^2 < (float)(threshold_i[k]^2) + ang_i^2*|p'|^2 with ang_i from threshold_angular_deg_i as in mh_icp_align.
 *  - Solve: the pairings of ALL pairs go to one robust Gauss-Newton solve; pair i's rows are scaled by weight_i.  Inner steps,
 *    the kernel-parameter schedule, prior, stall test, device hook, poll_every and expected_iterations behave as in mh_icp_align.
 *  - Counts: n_final_pairs (and the trace's n_pairs) is the sum over the pairs, potential_pairings = sum of scan_i->n, quality =
 *    their ratio (PairedRatio); NoPairings when the sum is 0.  The covariance is mh_icp_align's over the union of the final
 *    pairings.
 *  - Ignored fields of mh_icp_params: threshold, threshold_angular_deg, gn.weight_pt2pt (every pair carries its own); the trace's
 *    threshold reports pair 0's.
 *  - final_pairs[i] (nullable; arrays in pairs_mem of scan_i-size entries) receives pair i's final pairings in ascending local
 *    index, final_pair_counts[i] (nullable) their number.
 *  - Pairs may share a map and may share a scan: a shared scan pairs its points again for every pair (MH_MATCHED_POINTS_PAIR_AGAIN).
 *  - MH_ERR_INVALID_ARGUMENT: n_pairs 0 or above MH_MAX_LAYER_PAIRS, a null map / scan / threshold, maps and scans on more than
 *    one context, pt2pl_threshold != NULL.  MH_ERR_UNSUPPORTED: matched_points == MH_MATCHED_POINTS_SKIP with a scan shared by
 *    two pairs, profile != 0, a map of 2^30 or more records.
 * Per ICP iteration 1 + 2 * gn.max_inner_iterations launches, whatever the number of pairs.  No one-launch loops or streaming
 * control on this path; several such alignments advance in lock step through mh_icp_align_layers_batch (below). */
#define MH_MAX_LAYER_PAIRS 8
typedef struct {
  const mh_map* map;            /* global layer */
  const mh_scan* scan;          /* local layer (vehicle frame, untransformed) */
  const double* threshold;      /* HOST, max_iterations entries: this matcher's threshold per ICP_ITERATION */
  double threshold_angular_deg;
  double weight;                /* pointLayerMatches {..., weight} */
} mh_layer_pair;

MH_API mh_status mh_icp_align_layers(size_t n_pairs, const mh_layer_pair* pairs, const mh_icp_params* params,
                                     const double T_guess[12], const mh_prior* prior, mh_icp_result* result,
                                     mh_icp_iter* trace, const mh_pairs_out* final_pairs /* n_pairs entries or NULL */,
                                     uint64_t* final_pair_counts /* n_pairs entries or NULL */, int32_t pairs_mem);

/* mh_icp_align_layers with Matcher_Points_DistanceThreshold::allowMatchAlreadyMatchedGlobalPoints per pair (U13 [U]: upstream's
 * default is false, MatchState::globalPairedBitField).  opts == NULL or unique_global == 0 in every entry IS mh_icp_align_layers:
 * the same launches, the same cached graphs, the same bits (mh_icp_align_layers calls this function with NULL).  Otherwise the
 * contract above, n_pairs 1 included, plus:
 *  - Claims: within one ICP iteration the accepted candidates (i, g) -- local point i of a pair, map point g -- are taken in
 *    matching order: pairs in array order, local points in ascending index.  A candidate of a pair with unique_global != 0 is
 *    dropped when g of that map has been claimed already, otherwise it is kept and claims g; a dropped point has no pairing in
 *    that iteration (it is not offered its second-nearest neighbour).  A pair with unique_global == 0 neither tests nor sets
 *    claims.  Claims are per MAP: pairs that share a map share its claims; they start empty in every iteration.  (The device
 *    computes the equivalent minimum: the winner of g is the candidate with the smallest (pair, local index) naming it.)
 *  - Counts: potential_pairings is unchanged; quality, NoPairings, the trace's n_pairs, the covariance, final_pairs and
 *    final_pair_counts see the kept pairings only.
 *  - Two more launches per ICP iteration, whatever the number of pairs.  Results are bitwise reproducible, MH_NO_GRAPH=1 included.
 *  - MH_ERR_UNSUPPORTED also for: a unique pair whose scan has 2^29 or more points, or whose map has been offered 2^28 or more
 *    points (mh_map_info::n_offered: the claim table has an 8-byte entry per source index of the map, owned by the context).
 * Lock-step batch form: mh_icp_align_layers_batch_opts (below) takes a job's opts. */
typedef struct {
  uint32_t unique_global;       /* 1: allowMatchAlreadyMatchedGlobalPoints == false (U13) */
} mh_layer_pair_opts;

MH_API mh_status mh_icp_align_layers_opts(size_t n_pairs, const mh_layer_pair* pairs,
                                          const mh_layer_pair_opts* opts /* n_pairs entries or NULL */,
                                          const mh_icp_params* params, const double T_guess[12], const mh_prior* prior,
                                          mh_icp_result* result, mh_icp_iter* trace,
                                          const mh_pairs_out* final_pairs /* n_pairs entries or NULL */,
                                          uint64_t* final_pair_counts /* n_pairs entries or NULL */, int32_t pairs_mem);

/* mh_icp_align_layers_opts with Matcher::runFromIteration / runUpToIteration per pair (lidar3d-near-far.yaml:183), the rule of
 * Matcher::match [U].  (A struct and an entry point of their own: mh_layer_pair_opts keeps its layout and MH_ABI_VERSION its
 * value.)  gates == NULL or every field 0 IS mh_icp_align_layers_opts: the same launches, the same graph keys, the same upload, the
 * same bits (mh_icp_align_layers_opts calls this function with NULL).  Otherwise the contracts above, n_pairs 1 included, plus:
 *  - Active: pair i is active in ICP iteration k iff (from == 0 || k >= from) && (up_to == 0 || k <= up_to).
 *  - An inactive pair neither searches nor contributes: it has no pairings in that iteration (nothing in the solve, nothing in the
 *    trace's n_pairs), makes and loses no claims when it is unique_global, has nothing in the covariance, nothing in final_pairs[i]
 *    (the arrays are not written) and final_pair_counts[i] == 0.
 *  - NoPairings is decided on the active pairs' sum: at iteration 0 when every pair is gated off there (n_iterations 0), in a later
 *    iteration when the active set becomes empty.
 *  - potential_pairings: with k_last the iteration whose match produced the final pairings (the one that terminated the loop, or
 *    max_iterations - 1), the sum of scan_i->n over the pairs active in k_last; quality = n_final_pairs / potential_pairings.
 *  - The trace's threshold stays pair 0's schedule entry, active or not.
 *  - The launch count is unchanged (1 + 2 * inner, + 2 with a unique pair): the gates are data of the uploaded pair table, tested
 *    on the device with the iteration counter; a cached graph is reused whatever the gates are, nothing of them is in its key.  An
 *    inactive pair's match workgroups store "not paired" for its points instead of searching.
 * Lock-step batch form: mh_icp_align_layers_batch_opts (below) takes a job's gates; they are no part of a group's key. */
typedef struct {
  uint32_t run_from_iteration;   /* Matcher::runFromIteration, 0 = no limit */
  uint32_t run_up_to_iteration;  /* Matcher::runUpToIteration, 0 = no limit */
} mh_layer_pair_gates;

MH_API mh_status mh_icp_align_layers_gated(size_t n_pairs, const mh_layer_pair* pairs,
                                           const mh_layer_pair_opts* opts /* n_pairs entries or NULL */,
                                           const mh_layer_pair_gates* gates /* n_pairs entries or NULL */,
                                           const mh_icp_params* params, const double T_guess[12], const mh_prior* prior,
                                           mh_icp_result* result, mh_icp_iter* trace,
                                           const mh_pairs_out* final_pairs /* n_pairs entries or NULL */,
                                           uint64_t* final_pair_counts /* n_pairs entries or NULL */, int32_t pairs_mem);

/* mh_icp_align_layers_gated with Matcher_Points_DistanceThreshold::pairingsPerPoint per pair (lidar2d.yaml:156, rgbd.yaml:138 use
 * 2).  (A struct and an entry point of their own again: the structs above keep their layout and MH_ABI_VERSION its value.)
 * knn == NULL or every entry 0 or 1 IS mh_icp_align_layers_gated: the same launches, the same graph keys, the same upload, the same
 * bits (mh_icp_align_layers_gated calls this function with NULL).  Otherwise the contracts above, n_pairs 1 included, plus, with
 * k_i = pairings_per_point of pair i:
 *  - Matching: in every iteration in which it is active, pair i runs the matcher of mh_nn_search_k with k_i: per local point the
 *    k_i smallest (d^2, scan position) of the 27-voxel block, in that order, accepted in that order while d^2 < (float)(thr^2) +
 *    ang^2*|p'|^2 -- the accepted ones are a prefix.
 *  - Solve: every accepted pairing is one row block of the Gauss-Newton sums, scaled by the pair's weight; a local point
 *    contributes up to k_i times.
 *  - Counts: potential_pairings = sum of scan_i->n * k_i over the pairs active in k_last (pcLocal.size() * pairingsPerPoint [U], as
 *    mh_nn_search_k reports it); quality, the trace's n_pairs and n_final_pairs count pairings.
 *  - final_pairs[i]: arrays of scan_i->n * k_i entries, in ascending local index, a point's pairings in ascending distance (the
 *    order of mh_nn_search_k).
 *  - unique_global: the matching order gains a third level -- pair, local index, rank; each of a point's candidates is tested, and
 *    claims, on its own.
 *  - Gates: an inactive pair has no pairing in any of its scan_i->n * k_i entries.
 *  - One more launch per ICP iteration when any k_i > 1 (the search of those pairs), whatever their number; the set of such pairs
 *    and their k are part of the graph key.  Results are bitwise reproducible, MH_NO_GRAPH=1 and MH_NO_PREV_BOUND=1 included.
 *  - MH_ERR_INVALID_ARGUMENT: a pairings_per_point above MH_MAX_PAIRINGS_PER_POINT.  MH_ERR_UNSUPPORTED: scan_i->n * k_i >= 2^32, or
 *    >= 2^29 on a unique pair (the claim key's local field).
 * Lock-step batch form: mh_icp_align_layers_batch_opts (below) takes a job's knn; jobs with a k_i > 1 form groups of their own. */
typedef struct {
  uint32_t pairings_per_point;  /* 0 or 1: one; up to MH_MAX_PAIRINGS_PER_POINT */
} mh_layer_pair_knn;

MH_API mh_status mh_icp_align_layers_kbest(size_t n_pairs, const mh_layer_pair* pairs,
                                           const mh_layer_pair_opts* opts /* n_pairs entries or NULL */,
                                           const mh_layer_pair_gates* gates /* n_pairs entries or NULL */,
                                           const mh_layer_pair_knn* knn /* n_pairs entries or NULL */,
                                           const mh_icp_params* params, const double T_guess[12], const mh_prior* prior,
                                           mh_icp_result* result, mh_icp_iter* trace,
                                           const mh_pairs_out* final_pairs /* n_pairs entries or NULL */,
                                           uint64_t* final_pair_counts /* n_pairs entries or NULL */, int32_t pairs_mem);

/* mh_icp_align_layers_kbest with Matcher_Point2Plane on a plain point layer (KNN + PCA) per pair: rgbd.yaml:133-151 has one
 * Matcher_Points_DistanceThreshold (pairingsPerPoint 2) on its edge layers and one Matcher_Point2Plane on its plane layers, both
 * feeding one Solver_GaussNewton.  (A struct and an entry point of their own once more: the structs above keep their layout and
 * MH_ABI_VERSION its value.)  planes == NULL or knn == 0 in every entry IS mh_icp_align_layers_kbest: the same launches, the same
 * graph keys, the same upload, the same bits (mh_icp_align_layers_kbest calls this function with NULL).  Otherwise the contracts
 * above, n_pairs 1 included, plus, for a PLANE pair i (planes[i].knn != 0):
 *  - Matching: in every iteration in which it is active, pair i runs the matcher of mh_nn_search_pt2pl_knn on (map_i, scan_i) at the
 *    iteration's pose, with distance_threshold = pairs[i].threshold[k] (this matcher's schedule) and the other four parameters
 *    from planes[i].  Given the same pose, the centroids, the normals and the index set are those of mh_nn_search_pt2pl_knn, bit
 *    for bit.  (The map's NDT statistics, if any, are not used.)
 *  - Solve: each plane pairing is ONE row, e = n.(R l + t - c), with the iteration's robust kernel and kernel_param, scaled by
 *    pairs[i].weight.  gn.weight_pt2pl is ignored, as gn.weight_pt2pt already is.
 *  - Counts: a plane pair adds scan_i->n to potential_pairings (over the pairs active in k_last, the gated rule); its pairings go
 *    into n_final_pairs, the trace's n_pairs and final_pair_counts[i]; n_final_pairs_pt2pl is the sum over the plane pairs;
 *    NoPairings is decided on the total.
 *  - Covariance: mh_covariance over the union -- three rows per point pairing, one per plane pairing, unweighted.
 *  - final_plane_pairs[i] (nullable array of n_pairs entries; arrays in pairs_mem of scan_i->n entries) receives the pair's plane
 *    pairings in ascending local index.  final_pairs[i] is not written for a plane pair, final_plane_pairs[i] not for a point pair.
 *  - Gates act on a plane pair as on any pair: outside its interval it has no pairing and nothing in any count.
 *  - A scan shared between a plane pair and a point pair is paired again for each; the MH_MATCHED_POINTS_SKIP refusal is unchanged.
 *  - MH_ERR_INVALID_ARGUMENT: a plane pair with unique_global != 0, pairings_per_point > 1 or threshold_angular_deg != 0; a knn,
 *    search_radius, plane_eigen_threshold or an entry of its threshold schedule that mh_nn_search_pt2pl_knn rejects (the same
 *    code decides; minimum_plane_points below 3 counts as 3 there and here).  Everything is validated before any device work;
 *    afterwards the context stays usable.
 *  - Launches per ICP iteration, with P = 1 when any pair is a plain point pair (k = 1) and 0 otherwise, K = 1 when any pair has
 *    k > 1, A = 1 when any pair is a point pair (of either kind), U = 2 with a unique pair:
 *        P + K + 1 + U + (A + 1 + 1) * gn.max_inner_iterations
 *    -- the plane search, and per inner step the point accumulation (when there is a point pair), the plane accumulation and the
 *    solve.  With point pairs that is 1 + gn.max_inner_iterations more than without the plane pairs; a table of plane pairs only
 *    launches neither the plain search nor the point accumulation (1 + 2 * gn.max_inner_iterations).  The covariance that closes
 *    the loop has one more launch.  The set of plane pairs and their knn are part of the graph key.  Results are bitwise
 *    reproducible, MH_NO_GRAPH=1 and MH_NO_PREV_BOUND=1 included.
 * Lock-step batch form: mh_icp_align_layers_batch_planes (below) takes a job's planes; plane jobs form groups of their own. */
typedef struct {
  uint32_t knn;                   /* 0: a point pair (everything as before); 3 .. MH_MAX_PLANE_KNN: a plane pair */
  uint32_t minimum_plane_points;  /* >= 3 */
  double plane_eigen_threshold;
  double search_radius;
} mh_layer_pair_plane;

MH_API mh_status mh_icp_align_layers_planes(size_t n_pairs, const mh_layer_pair* pairs,
                                            const mh_layer_pair_opts* opts /* n_pairs entries or NULL */,
                                            const mh_layer_pair_gates* gates /* n_pairs entries or NULL */,
                                            const mh_layer_pair_knn* knn /* n_pairs entries or NULL */,
                                            const mh_layer_pair_plane* planes /* n_pairs entries or NULL */,
                                            const mh_icp_params* params, const double T_guess[12], const mh_prior* prior,
                                            mh_icp_result* result, mh_icp_iter* trace,
                                            const mh_pairs_out* final_pairs /* n_pairs entries or NULL */,
                                            const mh_pairs_pl_out* final_plane_pairs /* n_pairs entries or NULL */,
                                            uint64_t* final_pair_counts /* n_pairs entries or NULL */, int32_t pairs_mem);

/* Many multi-layer alignments from one host thread, one context per job: mh_icp_align_batch for mh_icp_align_layers.  Job i has
 * all its maps and scans on ONE context, distinct jobs have distinct contexts of the same device, and each job's pairs obey the
 * contract above.  Job i uses params[i] when params_per_job != 0 (else the one *params), T_guesses + 12*i and priors[i] (array or
 * entries may be NULL).  results[i] is bitwise what mh_icp_align_layers returns for job i alone -- T, cov, quality, n_iterations,
 * termination_reason, n_final_pairs, potential_pairings -- and final_pair_counts[i * MH_MAX_LAYER_PAIRS + p] (nullable) is that
 * call's final_pair_counts[p]; n_host_polls and n_enqueued_iterations describe the batch's loop control and may differ.  No trace
 * and no final pairings: a caller that wants them calls mh_icp_align_layers.
 *  - Jobs with equal gn.max_inner_iterations and compute_covariance form a lock-step group: every kernel of an iteration is ONE
 *    launch over all pairs of all its jobs (per ICP iteration 1 + 2 * gn.max_inner_iterations launches for the whole group); a job
 *    that has terminated leaves every later launch at once, so the jobs of a group end at different iterations.  Chunked loop
 *    control on the first job's stream (poll_every of the group's first job; 0 = the longest of the jobs' own estimates), launched
 *    directly, never from a captured graph.  A job alone in its group, trivial jobs (max_iterations == 0, no points) and every
 *    job under MH_NO_LOCKSTEP=1 run through mh_icp_align_layers, one after the other.
 *  - Work still queued on the jobs' own streams is ordered before the batch.
 *  - Everything is validated before any device work.  MH_ERR_INVALID_ARGUMENT: n_jobs 0 or above MH_MAX_LAYER_BATCH_JOBS, a job
 *    that mh_icp_align_layers rejects with that code, two jobs on one context, jobs on different devices.  MH_ERR_UNSUPPORTED: a
 *    job that mh_icp_align_layers rejects with that code.  After an error every context stays usable.
 *  - No opts, gates or knn here: mh_icp_align_layers_batch_opts (below) takes them per job, and this function is that one with
 *    the three arrays NULL in every job -- the same launches, the same uploads, the same bits. */
#define MH_MAX_LAYER_BATCH_JOBS 64
typedef struct {
  size_t n_pairs;              /* 1 .. MH_MAX_LAYER_PAIRS */
  const mh_layer_pair* pairs;
} mh_layer_job;

MH_API mh_status mh_icp_align_layers_batch(size_t n_jobs, const mh_layer_job* jobs, const mh_icp_params* params,
                                           int32_t params_per_job, const double* T_guesses, const mh_prior* const* priors,
                                           mh_icp_result* results,
                                           uint64_t* final_pair_counts /* n_jobs * MH_MAX_LAYER_PAIRS entries or NULL */);

/* mh_icp_align_layers_batch for mh_icp_align_layers_kbest: every job with its own opts, gates and knn (each n_pairs entries or
 * NULL, as that call takes them).  (A struct and an entry point of their own: mh_layer_job keeps its layout and MH_ABI_VERSION its
 * value.)  Everything mh_icp_align_layers_batch promises holds, with "what the single call returns" read as
 * mh_icp_align_layers_kbest(job i's pairs, opts, gates, knn): T, cov, quality, n_iterations, termination_reason, n_final_pairs,
 * potential_pairings (by the gated / k-best rule above) and the per-pair counts, bit for bit.  All three arrays NULL (or zeros, or
 * ones in knn) in every job IS mh_icp_align_layers_batch.  Otherwise, plus:
 *  - Groups: the key is gn.max_inner_iterations, compute_covariance and ONE more bit -- whether the job has a pair with k_i > 1
 *    (the single call chooses its accumulation kernels by exactly that).  Unique pairs and gates are not part of it.
 *  - Launches per ICP iteration, for the whole group: 1 + 2 * gn.max_inner_iterations; + 1 in a group of the k > 1 kind (the search
 *    of those pairs; the plain search is skipped when every pair of the group has k > 1); + 2 when any job has a unique pair (claim
 *    and resolve -- a job without a unique pair owns no workgroup of them).  Claims stay per context: every job's claim table is
 *    its own, so keys of different jobs never meet, and its epochs are consumed as by its single call.
 *  - A job alone in its group, trivial jobs (max_iterations == 0, nothing active in iteration 0) and every job under
 *    MH_NO_LOCKSTEP=1 run through mh_icp_align_layers_kbest with their arrays, one after the other.
 *  - Everything is validated before any device work, for every job: MH_ERR_INVALID_ARGUMENT also for a pairings_per_point above
 *    MH_MAX_PAIRINGS_PER_POINT; MH_ERR_UNSUPPORTED also for scan_i->n * k_i >= 2^32, a unique pair with 2^29 or more entries or whose
 *    map has been offered 2^28 or more points.  After an error every context stays usable and no claim epoch has been consumed. */
typedef struct {
  size_t n_pairs;                      /* 1 .. MH_MAX_LAYER_PAIRS */
  const mh_layer_pair* pairs;
  const mh_layer_pair_opts* opts;      /* n_pairs entries or NULL */
  const mh_layer_pair_gates* gates;    /* n_pairs entries or NULL */
  const mh_layer_pair_knn* knn;        /* n_pairs entries or NULL */
} mh_layer_job_opts;

MH_API mh_status mh_icp_align_layers_batch_opts(size_t n_jobs, const mh_layer_job_opts* jobs, const mh_icp_params* params,
                                                int32_t params_per_job, const double* T_guesses, const mh_prior* const* priors,
                                                mh_icp_result* results,
                                                uint64_t* final_pair_counts /* n_jobs * MH_MAX_LAYER_PAIRS entries or NULL */);

/* mh_icp_align_layers_batch_opts for mh_icp_align_layers_planes: every job with its own planes as well (n_pairs entries or NULL,
 * as that call takes them).  (A struct and an entry point of their own: mh_layer_job_opts keeps its layout and MH_ABI_VERSION its
 * value.)  Everything mh_icp_align_layers_batch_opts promises holds, with "the single call" read as
 * mh_icp_align_layers_planes(job i's pairs, opts, gates, knn, planes): n_final_pairs_pt2pl and the per-pair counts of plane pairs
 * included, bit for bit.  planes NULL (or knn 0 in every entry) in every job IS mh_icp_align_layers_batch_opts, which calls this
 * function: the same uploads, the same launches, the same bits.  Otherwise, plus:
 *  - Groups: the key is gn.max_inner_iterations, compute_covariance, whether the job has a pair with k_i > 1 and ONE more bit --
 *    whether the job has a plane pair.  A group without a plane job issues exactly the kernels it issued before.
 *  - Launches of a group of plane jobs per ICP iteration, for the whole group, by the single call's formula with P, K, U and A
 *    taken over all jobs of the group:  P + K + 1 + U + (A + 1 + 1) * gn.max_inner_iterations.  A launch without workgroups is
 *    skipped, the point accumulation and the point covariance accumulation of a group of plane pairs only included.  The solve and
 *    the covariance finalisation add each job's plane rows behind its point rows in the single call's fixed order.
 *  - A job alone in its group, trivial jobs and every job under MH_NO_LOCKSTEP=1 run through mh_icp_align_layers_planes with
 *    their arrays, one after the other.
 *  - Everything is validated before any device work, for every job: a plane pair by the rules of mh_icp_align_layers_planes
 *    (MH_ERR_INVALID_ARGUMENT for unique_global != 0, pairings_per_point > 1, threshold_angular_deg != 0, and for whatever
 *    mh_nn_search_pt2pl_knn rejects).  After an error every context stays usable and no claim epoch has been consumed. */
typedef struct {
  size_t n_pairs;                      /* 1 .. MH_MAX_LAYER_PAIRS */
  const mh_layer_pair* pairs;
  const mh_layer_pair_opts* opts;      /* n_pairs entries or NULL */
  const mh_layer_pair_gates* gates;    /* n_pairs entries or NULL */
  const mh_layer_pair_knn* knn;        /* n_pairs entries or NULL */
  const mh_layer_pair_plane* planes;   /* n_pairs entries or NULL */
} mh_layer_job_planes;

MH_API mh_status mh_icp_align_layers_batch_planes(size_t n_jobs, const mh_layer_job_planes* jobs, const mh_icp_params* params,
                                                  int32_t params_per_job, const double* T_guesses, const mh_prior* const* priors,
                                                  mh_icp_result* results,
                                                  uint64_t* final_pair_counts /* n_jobs * MH_MAX_LAYER_PAIRS entries or NULL */);

/* ------------------------------------------------------------------------------------------------
 * Occupancy voxel map: the local map class of pipelines/lidar2d.yaml:183-198, mrpt::maps::CVoxelMap [U] -- a log-odds
 * occupancy map updated by ray tracing and searched through the centres of its occupied voxels.  Upstream's source is not
 * vendored, so this is a restatement; parity with it is unpinned.  The reading implemented:
 *
 * Cells.  A cell is addressed by the packed 3 x 21-bit biased voxel index of mh_map: index = floor(p * (1/resolution)) in
 *   fp32, un-fused (index_mode as in mh_map_params; a point is inside the key range when |p * (1/resolution)| < 1e6 per axis,
 *   the test of mh_map).  A new cell starts at log-odds 0.
 * Log-odds.  Integers with scale 16.  The host derives five integers once, in double (round(v) = floor(v + 0.5)), and the
 *   device only ever sees them:
 *     l_hit  = max(1, round(16 ln(prob_hit / (1 - prob_hit))))       l_min = round(16 ln(clamp_min / (1 - clamp_min)))
 *     l_miss = max(1, round(16 ln((1 - prob_miss) / prob_miss)))     l_max = round(16 ln(clamp_max / (1 - clamp_max)))
 *     l_occ  = floor(16 ln(t / (1 - t))) + 1,  t = occupied_threshold
 *   A cell is occupied iff l >= l_occ.  (lidar2d.yaml's values: 14, 14, -47, 47, 7.)
 * One insert of a layer (vehicle frame) at pose T:
 *   1. every decimation-th point (0, decimation, ...) is composed with T: fp64, rounded to float, exactly as mh_map_insert;
 *   2. a point is left out when it is non-finite; else when max_range > 0 and (dx*dx + dy*dy) + dz*dz > max_range*max_range
 *      with d = p - (float)t in fp32; else when its index leaves the key range (these are counted: mh_occmap_info::n_left_out);
 *   3. the end cell of every kept point gets one hit;
 *   4. with ray_trace_free_space, every cell strictly between the cell o of T's translation and the end cell e gets one miss.
 *      With ad = |e - o| per axis, s = sign(e - o), M = max(ad), these are the M - 1 cells, k = 1 .. M-1,
 *        o_a + s_a * floor((2 k ad_a + M) / (2 M))   per axis a, in 64-bit integers
 *      -- the closed form of the sequential integer line walk "add ad to an error vector; on each axis with 2 err >= M, step and
 *      subtract M".  A cell that several steps or rays name gets one count from each;
 *   5. the counts (h, m) of the whole insert are applied once per cell, independent of thread order:
 *        MH_OCC_COUNTED: l = min(l_max, l + h l_hit) when h > 0, then l = max(l_min, l - m l_miss) when m > 0;
 *        MH_OCC_ONCE:    l = min(l_max, l + l_hit) when h > 0; otherwise l = max(l_min, l - l_miss) when m > 0;
 *   6. if remove_voxels_farther_than > 0, cells are erased by the rule and metric of mh_map_insert (far_voxel_metric, the
 *      distance ceil(remove_voxels_farther_than / resolution) in cells), measured from the cell of T's translation.
 * Search structure.  After every insert the centres ((float)index + 0.5f) * resolution (un-fused) of the occupied cells, in
 *   ascending packed-key order, are built into an inner uncapped mh_map (max_points_per_voxel = 0) of voxel size V; every
 *   matcher and ICP entry point takes that mh_map unchanged, and a matcher's global index is the centre's rank in that order.
 *   Upstream searches a k-d tree over these centres; the 27-voxel search is that search exactly for pair distances <= V.  V
 *   starts at search_voxel_size (0: 1.0 m) and only grows: mh_occmap_search_map takes the largest radius the coming alignment
 *   can use and, if it exceeds V, rebuilds the inner map once with V doubled until it suffices.  Results depend on V only
 *   through exact d2 ties between two centres.
 * Memory.  An insert writes one 64-bit key per (ray, step) and per end cell; above max_keys_per_pass keys it works in passes
 *   whose per-cell counts are summed before the rule is applied: the result does not depend on the pass size.  Every pass ends
 *   in a read-back of its run count, so a pass size far below the key count of an insert is for tests only.
 * The calls are synchronous (a few counters travel to the host per insert: a key-frame event, not a per-scan one).
 * ---------------------------------------------------------------------------------------------- */
enum { MH_OCC_COUNTED = 0, MH_OCC_ONCE = 1 };
typedef struct mh_occmap mh_occmap;
typedef struct {
  float resolution;              /* creationOpts.resolution [m] > 0 */
  float prob_hit, prob_miss;     /* insertOpts, inside (0, 1) */
  float clamp_min, clamp_max;    /* insertOpts, inside (0, 1), clamp_min < clamp_max */
  float occupied_threshold;      /* likelihoodOpts.occupiedThreshold, inside (0, 1) */
  uint32_t ray_trace_free_space; /* insertOpts */
  uint32_t decimation;           /* insertOpts, >= 1 */
  float max_range;               /* insertOpts [m]; 0 = no limit */
  uint32_t update_rule;          /* MH_OCC_* */
  uint32_t index_mode;           /* MH_INDEX_* */
  uint32_t far_voxel_metric;     /* MH_FAR_* */
  float search_voxel_size;       /* the first V [m]; 0 = 1.0 */
  uint32_t reserved_;
  uint64_t max_keys_per_pass;    /* 0 = 2^24 */
} mh_occmap_params;
typedef struct {
  uint64_t n_cells;                             /* stored cells */
  uint64_t n_occupied;                          /* ... of which occupied: the points of the search map */
  int32_t l_hit, l_miss, l_min, l_max, l_occ;   /* the five integers */
  float search_voxel_size;                      /* the current V */
  uint64_t n_left_out;                          /* last insert: points whose index left the key range */
  uint64_t n_keys;                              /* last insert: keys written */
  uint32_t n_passes;                            /* last insert: passes */
  uint32_t reserved_;
} mh_occmap_info;
/* Refusals (MH_ERR_INVALID_ARGUMENT, before any device work): a NULL argument, resolution <= 0, a probability or clamp outside
 * (0, 1), clamp_min >= clamp_max, decimation 0, an unknown rule; mh_occmap_insert: a scan of another context. */
MH_API mh_status mh_occmap_create(mh_ctx* ctx, const mh_occmap_params* params, mh_occmap** out);
MH_API mh_status mh_occmap_destroy(mh_occmap* occ);
/* Forget every cell; the search voxel starts over: a cleared map behaves as a new one. */
MH_API mh_status mh_occmap_clear(mh_occmap* occ);
MH_API mh_status mh_occmap_insert(mh_occmap* occ, const mh_scan* scan, const double T[12], float remove_voxels_farther_than);
MH_API mh_status mh_occmap_get_info(const mh_occmap* occ, mh_occmap_info* info);
/* The cells in ascending key order to HOST arrays (either may be NULL): 3 indices and one log-odds value per cell. */
MH_API mh_status mh_occmap_download(const mh_occmap* occ, int32_t* keys_xyz, int32_t* logodds);
/* The search map for alignments whose pair distances do not exceed min_radius (see "Search structure").  The handle is the
 * occupancy map's own: valid until the next insert, clear or growing call, never to be destroyed by the caller. */
MH_API mh_status mh_occmap_search_map(mh_occmap* occ, float min_radius, const mh_map** out);

#ifdef __cplusplus
}
#endif
#endif /* MOLAHIP_H */
