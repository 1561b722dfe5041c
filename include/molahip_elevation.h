/* molahip_elevation.h -- a 2.5-D elevation map of a recorded session's key-frames: the sixth public header of libmolahip.so
 * (DESIGN.md row g14).  It adds to include/molahip.h and changes nothing there: MH_ABI_VERSION stays what it is, this surface has
 * a version of its own.  Conventions (status codes, `mem` spaces, streams, ownership) are molahip.h's; mh_map_frame, the
 * composition of a point with its frame's pose, the passes and the refusals of a batched posed-frame call are those written down
 * at mh_map_insert_frames there.
 *
 * An mh_elev is a window of nx * ny cells of the world's x-y plane.  It holds four planes of 32-bit integers, ny * nx entries, y
 * outer (entry [r * nx + c] is the cell with index (x0 + c, y0 + r)):
 *     ground          int32   the lowest height seen in the cell, in height quanta      initially INT32_MAX
 *     count           uint32  the points that fell into the cell                        initially 0
 *     obstacle_count  uint32  the points that stand higher than a step over the ground  initially 0
 *     top             int32   the highest height below the vehicle's clearance          initially INT32_MIN
 * Everything after the composition is integer (minimum, maximum, sum): results are exact and depend neither on thread order nor
 * on how the work is split into passes or calls.
 *
 * THE POINT RULE (shared by the three point passes).  With inv = 1.0f / resolution and invq = 1.0f / z_quantum, both in fp32:
 *   0. the point p of frame f is composed with the frame's pose T as mh_map_insert_frames composes it, per row
 *      (float)(((T0*px + T1*py) + T2*pz) + T3) in fp64, un-fused, rounded to float once: P = (Px, Py, Pz);
 *   1. the point is left out when Px, Py or Pz is non-finite;
 *   2. else, when max_range > 0, it is left out when (dx*dx + dy*dy) + dz*dz > max_range*max_range with d = P - (float)t in fp32,
 *      un-fused, t = (T3, T7, T11): the expression of mh_occmap_insert step 2 (max_range*max_range is one fp32 product);
 *   3. else, with sx = Px * inv, sy = Py * inv, sz = Pz * invq (fp32, un-fused), it is left out when |sx| >= 1e6 or |sy| >= 1e6 or
 *      |sz| >= 2^30 (1073741824.0f);
 *      otherwise ix = (int32) floorf(sx), iy = (int32) floorf(sy) -- the floor rule of mh_occmap -- and zq = (int32) floorf(sz);
 *   4. the point lies outside the window when ix - x0 is not in [0, nx) or iy - y0 is not in [0, ny) (in 64-bit integers).
 *   Points of cases 1 to 3 are counted in n_left_out, points of case 4 in n_outside_window; the others are KEPT, c is their cell.
 *
 * mh_elev_bounds_frames -- sizes the window before a map exists: lo[2] / hi[2] = the minimum and maximum of (ix, iy) over the
 *   points of the frames that pass cases 1 to 3, *n_in = their number.  No quantum is known here, so the height part of case 3
 *   (|sz| >= 2^30) is not applied: the bounds can only be wider than what mh_elev_add_frames keeps.  With *n_in == 0, lo and hi
 *   are left untouched.  (One lane per point; the wave reduces, then integer atomics.)  Scratch is allocated for the call and
 *   released before it returns: a call per session, not per scan.
 *
 * mh_elev_create.  MH_ERR_INVALID_ARGUMENT: a NULL argument; resolution or z_quantum not finite or <= 0; max_range not finite or
 *   < 0; nx or ny of 0; nx * ny > 2^26; clearance_q < 0 or step_q < 0.  clearance_q and step_q are height quanta: the caller
 *   derives them on the host (mola_hip::TraversabilityOptions: floor(v / z_quantum) in fp64), the device only sees the integers.
 * mh_elev_clear -- the four planes and every counter as after mh_elev_create; the ground is no longer frozen.
 *
 * mh_elev_add_frames -- pass 1.  Per kept point:  ground[c] = min(ground[c], zq);  count[c] += 1.
 * mh_elev_mark_frames -- pass 2, over the same frames once the ground is complete.  Per kept point, with h = zq - ground[c] in
 *   64-bit integers (a cell no point was added to has ground INT32_MAX: h < 0):
 *     h > clearance_q : nothing happens, the point is overhead (a bridge, a canopy);
 *     otherwise       : top[c] = max(top[c], zq), and when h > step_q: obstacle_count[c] += 1.
 *   The first mark call freezes the ground: mh_elev_add_frames then returns MH_ERR_INVALID_ARGUMENT until mh_elev_clear.  Because
 *   the ground is frozen, marking is independent of frame order, of the pass size and of how the frames are split over calls.
 * Both calls:
 *  - Passes, staging and `mem` are mh_map_insert_frames': frames in order into passes of at most max_points_per_pass points (0:
 *    the library's default, 2^21), a larger frame is a pass of its own; host arrays travel through a page-locked mirror, device
 *    arrays are read in place (x, y, z of a frame may be NULL when its n is 0).  The calls are synchronous: on return the caller's
 *    arrays may be reused and mh_elev_get_info is up to date.
 *  - MH_ERR_INVALID_ARGUMENT before any device work, the map untouched: a NULL map; NULL frames with n_frames > 0; a bad `mem`;
 *    NULL arrays with n > 0; a non-finite pose entry (of an empty frame too); n_frames > MH_MAX_INSERT_FRAMES; a frame of
 *    0x7FFFFFF0 points or more; a call whose points, added to the points that the same kind of call has KEPT since the last clear
 *    (n_counted; for the mark pass its offered points less its left-out and outside ones), would exceed 0xFFFFFFF0: the counters
 *    of a cell are 32 bits wide, and the call's points bound what it can add to one.
 *  - n_frames == 0 or only empty frames: MH_OK, nothing changes (an empty mark call does not freeze the ground).
 *  - A failure in a later pass (out of memory) leaves the earlier passes applied and the info totals those of the completed passes.
 *
 * mh_elev_relief -- a windowed stencil over the ground.  A cell is KNOWN when count >= min_points.  relief_host is a HOST array of
 *   ny * nx int32: for a known cell, the maximum minus the minimum of `ground` over the known cells of its (2 radius + 1)^2 window
 *   (the cell itself is one of them; window cells outside the grid do not exist); MH_ELEV_NONE for a cell that is not known.
 *   MH_ERR_INVALID_ARGUMENT: a NULL argument, radius > 4, min_points == 0.
 * mh_elev_download -- the planes to HOST arrays of ny * nx entries; any of the four may be NULL.
 *
 * Threads.  As every handle of the library, an mh_elev is not to be used by two calls at once; mh_elev_relief, mh_elev_download
 * and mh_elev_get_info take a const handle because they leave the planes alone, but they use the handle's scratch. */
#ifndef MOLAHIP_ELEVATION_H_
#define MOLAHIP_ELEVATION_H_

#include "molahip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MH_ELEV_API_VERSION 1
#define MH_ELEV_NONE INT32_MIN
#define MH_ELEV_MAX_RELIEF_RADIUS 4

typedef struct mh_elev mh_elev;
typedef struct {
  float resolution;    /* cell size [m] > 0 */
  float z_quantum;     /* height quantum [m] > 0 */
  float max_range;     /* [m]; 0 = no limit */
  int32_t x0, y0;      /* cell index of column 0 / row 0 */
  uint32_t nx, ny;     /* columns, rows; nx * ny <= 2^26 */
  int32_t clearance_q; /* heights above this over the ground are overhead [quanta] >= 0 */
  int32_t step_q;      /* the largest passable step [quanta] >= 0 */
  uint32_t reserved_;
} mh_elev_params;      /* 40 bytes */
typedef struct {
  uint64_t n_offered;             /* mh_elev_add_frames since the last clear: points of its calls */
  uint64_t n_counted;             /* ... of which kept: the sum of the count plane */
  uint64_t n_left_out;            /* ... cases 1 to 3 */
  uint64_t n_outside_window;      /* ... case 4 */
  uint64_t n_mark_offered;        /* mh_elev_mark_frames since the last clear: points of its calls */
  uint64_t n_mark_left_out;       /* ... cases 1 to 3 */
  uint64_t n_mark_outside_window; /* ... case 4 */
  uint32_t ground_frozen;         /* 1 after the first mark call that held a point */
  uint32_t reserved_;
} mh_elev_info;                   /* 64 bytes */

/* MH_ELEV_API_VERSION of the loaded library. */
MH_API uint32_t mh_elev_api_version(void);
MH_API mh_status mh_elev_bounds_frames(mh_ctx* ctx, const mh_map_frame* frames, size_t n_frames, int32_t mem, float resolution,
                                       float max_range, uint64_t max_points_per_pass, int32_t lo[2], int32_t hi[2], uint64_t* n_in);
MH_API mh_status mh_elev_create(mh_ctx* ctx, const mh_elev_params* params, mh_elev** out);
MH_API mh_status mh_elev_destroy(mh_elev* elev);
MH_API mh_status mh_elev_clear(mh_elev* elev);
MH_API mh_status mh_elev_get_info(const mh_elev* elev, mh_elev_info* info);
MH_API mh_status mh_elev_add_frames(mh_elev* elev, const mh_map_frame* frames, size_t n_frames, int32_t mem,
                                    uint64_t max_points_per_pass);
MH_API mh_status mh_elev_mark_frames(mh_elev* elev, const mh_map_frame* frames, size_t n_frames, int32_t mem,
                                     uint64_t max_points_per_pass);
MH_API mh_status mh_elev_relief(const mh_elev* elev, uint32_t radius, uint32_t min_points, int32_t* relief_host);
MH_API mh_status mh_elev_download(const mh_elev* elev, int32_t* ground, uint32_t* count, uint32_t* obstacle_count, int32_t* top);

#ifdef __cplusplus
}
#endif
#endif /* MOLAHIP_ELEVATION_H_ */
