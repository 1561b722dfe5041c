/* molahip_clean.h -- removal of moving objects from recorded key-frames by see-through voting: the second public header of
 * libmolahip.so.  It adds to include/molahip.h and changes nothing there: MH_ABI_VERSION stays what it is,
 * this surface has a version of its own.  Conventions (status codes, `mem` spaces, streams, ownership) are molahip.h's.
 *
 * The idea.  Each key-frame is a view of the world from a known pose.  A stored point that several OTHER frames look straight
 * through, to something farther, was not there when they looked: a car, a cyclist, a pedestrian.  A view is a small polar
 * range image; a vote is one projection and a handful of comparisons.  Everything is integer or compare-only fp32: results are
 * exact and depend neither on the order of the points nor on how the work is split into passes.
 *
 * THE RULE (this text is the specification; tests/clean_ref.py restates it in numpy and every word must agree).  No
 * transcendental function and no square root run on the device; every boundary comes from a table the host builds in fp64 and
 * rounds once to fp32; all point arithmetic is un-fused fp32.
 *
 *  - Parameters (mh_clean_params): A = n_rings in [1, MH_CLEAN_MAX_RINGS]; S = n_sectors, a multiple of 8 in
 *    [8, MH_CLEAN_MAX_SECTORS]; A * S <= MH_CLEAN_MAX_BINS (one view fits 16 KB of LDS); -pi/2 < el_min < el_max < pi/2
 *    (elevation window, radians); 0 < min_range < max_range; rel_margin > 0; origin[3] = the sensor's position in the vehicle
 *    frame; win_rings, win_sectors in 0..2 (window half-widths); all values finite (and the tables below finite in fp32,
 *    min_r2 > 0).
 *  - Host tables:
 *        tan_edge[j] = (float)tan(2 * pi * j / S), j = 1..S/8-1              (mh_place_describe's table)
 *        e_k = el_min + k * (el_max - el_min) / A in fp64, k = 0..A;  el_tan2[k] = (float)(tan(e_k) * tan(e_k));
 *        el_sign[k] = +1 if e_k > 0, -1 if e_k < 0, 0 if e_k == 0             (decided in fp64)
 *        min_r2 = (float)(min_range * min_range), max_r2 = (float)(max_range * max_range)   (products in fp64)
 *        far2 = (float)((1 + rel_margin) * (1 + rel_margin))                  (in fp64)
 *  - BINNING a point (px, py, pz) given in the vehicle frame:  x = px - origin[0], y = py - origin[1], z = pz - origin[2];
 *        h2 = x*x + y*y;   zz = z*z;   r2 = h2 + zz.
 *    The point is skipped when a coordinate of (x, y, z) is non-finite; when x = y = 0; when r2 lies outside [min_r2, max_r2);
 *    when its elevation lies outside the window (below).
 *  - Elevation.  "Edge k lies at or below the point", above(k), is decided with m_k = el_tan2[k] * h2 by the sign of the edge:
 *        el_sign[k] > 0:  z > 0 and zz >= m_k;     el_sign[k] == 0:  z >= 0;     el_sign[k] < 0:  z >= 0 or zz <= m_k.
 *    A point exactly on an edge (zz == m_k with the matching sign of z) lies at or above it: it belongs to the ring above.
 *    The point is skipped when not above(0) or when above(A);  ring = #{k in 1..A-1 : above(k)}.
 *  - Sector: exactly mh_place_describe's rule on (x, y) -- quarter turns, then the tan_edge comparisons (molahip.h states it).
 *  - A VIEW of a frame is A x S 32-bit words, view[ring * S + sector]: the bit pattern of the smallest r2 among the frame's
 *    points of that bin, 0xFFFFFFFF for an empty bin.  Positive floats order as unsigned integers, so the minimum is an integer
 *    minimum: exact, whatever the order in which the points arrive.
 *  - THE VOTE of point p of frame i against the view of frame j:
 *      1. q = (float)(((T0*px + T1*py) + T2*pz) + T3) per row, in fp64, un-fused, with T = T_j^-1 T_i (nbr_T, twelve doubles,
 *         row-major 3x4).  The caller forms T; mola_hip::clean_keyframes forms it from the rigid poses [R_i | t_i], [R_j | t_j] as
 *             T[r][c] = (R_j[0][r]*R_i[0][c] + R_j[1][r]*R_i[1][c]) + R_j[2][r]*R_i[2][c],            c = 0..2
 *             T[r][3] = (R_j[0][r]*(t_i[0]-t_j[0]) + R_j[1][r]*(t_i[1]-t_j[1])) + R_j[2][r]*(t_i[2]-t_j[2])
 *         in fp64, un-fused, in this order.
 *      2. q is binned as above (origin subtracted); r2_q is its r2.  A skipped q gives no evidence.
 *      3. The window: rings ring-win_rings .. ring+win_rings that lie inside 0..A-1 (rings outside the image are left out),
 *         sectors sector-win_sectors .. sector+win_sectors modulo S (sectors wrap).  r2_img is a bin's word read as fp32.
 *           THROUGH: every bin of the window is non-empty and has r2_img > r2_q * far2.
 *           AGREE:   otherwise, if the point's own bin is non-empty and r2_q <= r2_img * far2 and r2_img <= r2_q * far2.
 *           Neither: no evidence (occluded, or the view is empty there).
 *         The every-bin rule is deliberate: on ground seen at a shallow angle the next ring down always holds a nearer return,
 *         and a single-bin see-through test votes wrongly there.
 *  - Per point:  votes = through | agree << 16, each count saturating at 65535, summed over the frame's neighbour list.
 *  - Binding properties: a view does not depend on the order of its points; turning every point of a frame by an exact
 *    quarter turn, (x, y) -> (-y, x) (origin 0), shifts its view by exactly S/4 columns; a frame voted against its own view under
 *    the identity pose collects no through vote (its own bin holds r2_img <= r2_q <= r2_q * far2).
 *
 *  - mh_views_create / _destroy / _size: a store of views of one parameter set on the context's device.
 *  - mh_views_add_frames: appends one view per frame, in passes of at most max_points_per_pass points (0: the library's default,
 *    2^21) -- one upload and one flat launch over all points of the pass, as mh_map_insert_frames; a frame larger than the
 *    budget is a pass of its own.  frames[f].T is ignored; an empty frame appends an all-empty view; x, y, z may be NULL when n
 *    is 0.  The result does not depend on the pass size.
 *  - mh_views_download: views first .. first+n-1 as n * A * S words to host memory `out`.
 *  - mh_views_vote_frames: one word per point, votes_out[sum of n_g over g < f + i] for point i of frames[f], in `mem`.
 *    The neighbour list is CSR in HOST memory: frame f votes against the views nbr_view[k] under nbr_T[12*k .. 12*k+11] for
 *    k in nbr_start[f] .. nbr_start[f+1]-1.  A frame with no neighbours gets zeros.  A view may appear any number of times.
 *    Passes as above; by the definition the result does not depend on the pass size.
 *  - `mem` (of the frames' arrays and of votes_out): MH_MEM_HOST, MH_MEM_HOST_PINNED or MH_MEM_DEVICE.  Every call orders itself
 *    on the context's stream and blocks until its output is in place (and the caller's arrays may be reused).
 *  - Refusals, all decided before any device work, the store untouched: MH_ERR_INVALID_ARGUMENT for NULL handles or arrays
 *    (NULL point arrays with n > 0; NULL nbr_view / nbr_T with a non-empty list; NULL votes_out with points to vote on), a bad
 *    `mem`, parameters outside the ranges above, a frame of 0x7FFFFFF0 points or more, a download range beyond the store, a
 *    neighbour index beyond the store, a non-finite pose entry in nbr_T, nbr_start not non-decreasing. */
#ifndef MOLAHIP_CLEAN_H_
#define MOLAHIP_CLEAN_H_

#include "molahip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MH_CLEAN_API_VERSION 1
#define MH_CLEAN_MAX_RINGS 64
#define MH_CLEAN_MAX_SECTORS 256
#define MH_CLEAN_MAX_BINS 4096
#define MH_CLEAN_EMPTY 0xFFFFFFFFu

typedef struct {
  uint32_t n_rings, n_sectors;
  float el_min, el_max;       /* radians */
  float min_range, max_range;
  float rel_margin;
  float origin[3];
  uint32_t win_rings, win_sectors;
} mh_clean_params; /* 48 bytes */

typedef struct mh_views mh_views;
/* MH_CLEAN_API_VERSION of the loaded library. */
MH_API uint32_t mh_clean_api_version(void);
MH_API mh_status mh_views_create(mh_ctx* ctx, const mh_clean_params* params, mh_views** out);
MH_API mh_status mh_views_destroy(mh_views* views);
MH_API mh_status mh_views_size(const mh_views* views, uint64_t* n);
MH_API mh_status mh_views_add_frames(mh_views* views, const mh_map_frame* frames, size_t n_frames, int32_t mem,
                                     uint64_t max_points_per_pass);
MH_API mh_status mh_views_download(const mh_views* views, uint64_t first, uint64_t n, uint32_t* out);
MH_API mh_status mh_views_vote_frames(const mh_views* views, const mh_map_frame* frames, size_t n_frames, const uint32_t* nbr_start,
                                      const uint32_t* nbr_view, const double* nbr_T, uint32_t* votes_out, int32_t mem,
                                      uint64_t max_points_per_pass);

#ifdef __cplusplus
}
#endif
#endif /* MOLAHIP_CLEAN_H_ */
