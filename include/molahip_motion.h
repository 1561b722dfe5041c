/* molahip_motion.h -- de-skew a scan with a piecewise motion table: the fifth public header of libmolahip.so (DESIGN.md row
 * g13).  It adds to include/molahip.h and changes nothing there: MH_ABI_VERSION stays what it is, this surface has a version of
 * its own.  Conventions (status codes, streams, ownership, what a scan carries) are molahip.h's.
 *
 * mh_scan_deskew computes p' = Exp_SO3(w t_i) p + v t_i with ONE angular rate w for the whole sweep.  Where the rate changes
 * inside a sweep (a hand-held or head-mounted sensor, a drone, cobbles, a sharp turn-in) a gyroscope next to the LiDAR
 * measures what no constant twist can describe.  The host cuts the gyro samples of the sweep into K segments of constant rate
 * (mola_hip::build_motion_table, GyroDeskew.h) and hands the table to the device:
 *
 *   segment s = { knot_s [s], R_s (row-major 3x3: the rotation at knot_s), w_s [rad/s] }, 1 <= K <= MH_MOTION_MAX_SEGMENTS,
 *   knots strictly ascending, plus one linear velocity v [m/s] for the whole sweep.
 *
 * THE RULE per point (x, y, z) with time stamp tf (fp32), all arithmetic in fp64 and only the result rounded to float:
 *     t  = (double)tf
 *     s  = clamp(#{k : knot_k <= t} - 1, 0, K - 1)
 *     d  = t - knot_s
 *     u  = Exp_SO3(w_s * d) * p                  (Rodrigues, the library's se3_exp with a zero translation part)
 *     p' = (float)(R_s * u + v * t)              (each row summed left to right: ((r0 ux + r1 uy) + r2 uz) + v t)
 *   - a point before the first knot uses segment 0 with a negative d, one after the last knot the last segment;
 *   - a NaN stamp counts no knot, so s = 0, and its coordinates come out NaN; an infinite stamp gives NaN coordinates too;
 *   - a point with a non-finite coordinate stays non-finite.
 *   Only the rotation is piecewise; the translation stays the reference's v t.  A table cut from a constant rate w (R_s =
 *   Exp_SO3(w knot_s), w_s = w) is therefore mh_scan_deskew(twist = (v, w)) up to rounding, and so is K = 1, knot 0, R = I.
 *   In numpy (float64; tests/motion_ref.py holds the same lines):
 *     cnt = (knot[None, :] <= t[:, None]).sum(1);  s = np.clip(cnt - 1, 0, K - 1);  d = t - knot[s]
 *     u   = np.einsum('nij,nj->ni', so3_exp(w[s] * d[:, None]), p)
 *     out = (np.einsum('nij,nj->ni', R[s], u) + v[None, :] * t[:, None]).astype(np.float32)
 *
 * mh_scan_deskew_motion -- everything else follows mh_scan_deskew: time stamps, src_idx and intensity are carried bit for bit;
 *   `motion == NULL` or a scan without time stamps copies the points; `out` must differ from `in`; `in` may belong to another
 *   context of the same device (complete by now); the call is queued on `out`'s stream and nothing is read back.
 *
 * mh_scan_deskew_motion_pair -- DEFINITION: mh_scan_deskew_motion(in_a -> out_a), mh_scan_deskew_motion(in_b -> out_b) and
 *   mh_scan_bbox(out_b), bit for bit.  One launch and one wait when both layers carry stamps, neither is empty and `b` holds at
 *   most 65536 points (workgroup 0 walks `b` and reduces its box into page-locked host memory); the three separate calls
 *   otherwise (copies, empty layers, a larger `b`).  n_finite may be NULL.
 *
 * THE TABLE IN FLIGHT.  A caller may queue several de-skews without waiting (the twist hook of the ICP loop does), each with a
 *   table of its own, and may reuse or free `motion` and `motion->segments` as soon as a call returns.  No call reads host
 *   memory after it returns, and no queued call can see a later call's table:
 *   - K <= 32: the table travels as a KERNEL ARGUMENT of its launch (3.4 KB; the launch owns its copy);
 *   - K  > 32: a STREAM-ORDERED COPY from a pageable host block (staged by the runtime before the copy call returns) into a
 *     device block of `out`'s context, followed on the same stream by the launch that reads it; the next call's copy is
 *     ordered behind that launch.
 *   There is no pinned staging buffer.  Inside the kernel the table is staged once per workgroup in LDS (at most 6.7 KB).
 *
 * MH_ERR_INVALID_ARGUMENT, before any device work and with `out` untouched: a NULL argument other than `motion` (and n_finite);
 *   n_segments of 0 or above MH_MOTION_MAX_SEGMENTS; NULL segments; knots not strictly ascending; a non-finite knot, R, w or
 *   v; out == in (the pair: any two of the four scans equal); scans of different devices (the pair: outputs of different
 *   contexts).  R is not checked for orthonormality: the rule is defined for any finite matrix.
 *
 * Threads: as every call on a context, not concurrently with other calls on `out`'s context. */
#ifndef MOLAHIP_MOTION_H_
#define MOLAHIP_MOTION_H_

#include "molahip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MH_MOTION_API_VERSION 1
#define MH_MOTION_MAX_SEGMENTS 64

typedef struct {
  double knot; /* start of the segment [s], on the time axis of the scan's stamps */
  double R[9]; /* rotation at `knot`, row-major */
  double w[3]; /* angular rate of the segment [rad/s] */
} mh_motion_segment; /* 104 bytes */

typedef struct {
  uint32_t n_segments; /* 1 .. MH_MOTION_MAX_SEGMENTS */
  uint32_t reserved_;
  const mh_motion_segment* segments; /* HOST memory */
  double v[3];                       /* linear velocity of the whole sweep [m/s] */
} mh_motion_table;                   /* 40 bytes */

/* MH_MOTION_API_VERSION of the loaded library. */
MH_API uint32_t mh_motion_api_version(void);
MH_API mh_status mh_scan_deskew_motion(const mh_scan* in, const mh_motion_table* motion, mh_scan* out);
MH_API mh_status mh_scan_deskew_motion_pair(const mh_scan* in_a, const mh_scan* in_b, const mh_motion_table* motion,
                                            mh_scan* out_a, mh_scan* out_b, float bb_min[3], float bb_max[3], uint64_t* n_finite);

#ifdef __cplusplus
}
#endif
#endif /* MOLAHIP_MOTION_H_ */
