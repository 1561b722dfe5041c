/* molahip_live.h -- erasing moving objects from a LIVE local map by see-through voting: the third public header of
 * libmolahip.so.  It adds to include/molahip.h and include/molahip_clean.h and changes nothing there:
 * MH_ABI_VERSION and MH_CLEAN_API_VERSION stay what they are, this surface has a version of its own.  Conventions (status
 * codes, `mem` spaces, streams, ownership) are molahip.h's; THE RULE (binning, view, vote) is molahip_clean.h's, word for word.
 *
 * molahip_clean.h votes on the points of recorded key-frames before a session map is built.  Here the votes fall on the stored
 * records of an mh_map while it is being driven: the caller keeps a small fixed ring of views (one per recent map update, written
 * from the device-resident scan that was just inserted), and after an update the stored points that enough of those views look
 * straight through are taken out of the map.
 *
 *  - mh_views_put_scan: the view of a device-resident scan (points in the vehicle frame; time stamps, source indices and
 *    intensity ignored) into `slot` of the store: slot == size appends, slot < size overwrites, slot > size is
 *    MH_ERR_INVALID_ARGUMENT.  The words are exactly those mh_views_add_frames gives for the same points; an empty scan gives an
 *    all-empty view.  Queued on the context's stream (no host wait); the scan is read in stream order, as mh_map_insert reads it.
 *    Scan and views must belong to one context.
 *  - mh_views_vote_map: one word per STORED POINT of the map, in mh_map_download order, votes_out[0 .. n_points-1] in `mem`
 *    (MH_MEM_HOST, MH_MEM_HOST_PINNED or MH_MEM_DEVICE).  The word is through | agree << 16, exactly THE VOTE of
 *    molahip_clean.h with p = the stored point (world frame) and T = nbr_T[12*k .. 12*k+11] the world-to-view transform of view
 *    nbr_view[k], k = 0 .. n_nbr-1 (both lists in HOST memory): step 1's fp64 un-fused transform, the binning, the window and
 *    the saturation are unchanged.  n_nbr <= MH_LIVE_MAX_VIEWS; a view may repeat; n_nbr == 0 gives zeros.  Synchronous: it
 *    blocks until votes_out is in place.
 *  - mh_map_erase_points: drop[i] != 0 removes stored point i (mh_map_download order; `drop` in `mem`, n bytes).  n must equal
 *    the stored count, else MH_ERR_INVALID_ARGUMENT and the map is untouched.
 *    DEFINITION.  Afterwards the map is indistinguishable from a fresh map of the same mh_map_params after mh_map_restore of
 *    (its download minus the dropped records, the same n_offered): the same mh_map_download and mh_map_download_ndt bits with
 *    the source indices kept, the same counts and bounding box, a voxel that loses its last point is gone, the same answers
 *    from every search route, the same result of a following mh_map_insert (freed cap slots are free again, clearance sees only
 *    what is left).  mh_map_info::table_size is a capacity sized from a bound the host knows and is not part of this.  All
 *    zeros leaves every bit unchanged.  A pending deferred verdict (molahip.h, mh_map_insert) stays pending.
 *    The rebuild is the one of mh_map_insert -- NDT statistics are recomputed as every rebuild does -- and is queued the same
 *    way: its counts are read back lazily by whoever asks next.  To compare n the call first takes in the counts of the map's
 *    previous update (it waits for that update if it still runs).  Host `drop` arrays may be reused on return; a device array
 *    is read in stream order.
 *  - mh_map_erase_seen_through: by definition mh_views_vote_map, then drop = through >= min_through_votes && through >
 *    agree_weight * agree, then mh_map_erase_points -- entirely on the device, queued like mh_map_insert: nothing is read back
 *    and nothing is waited for on the calling thread, not even the counts of an mh_map_insert queued just before (the kernels
 *    go by the device's own counters); the erased count travels with the map's own counters.
 *  - mh_map_erased_total: the points the two calls above have erased since the map was created (a rebuild by mh_map_build or
 *    mh_map_restore does not reset it).  It takes in what is pending.
 *  - Ordering: views and map belong to one context, and views are written and maps are updated on that context's one stream:
 *    a view written by mh_views_put_scan is seen by every vote queued after it.
 *  - Refusals, all decided before any device work, map and store untouched: MH_ERR_INVALID_ARGUMENT for NULL handles, a NULL
 *    votes_out / drop with points stored, NULL nbr_view / nbr_T with n_nbr > 0, a bad `mem`, n_nbr > MH_LIVE_MAX_VIEWS,
 *    `capacity` below the stored count, a neighbour index beyond the store, a non-finite pose entry, handles of different
 *    contexts, slot > size, n other than the stored count. */
#ifndef MOLAHIP_LIVE_H_
#define MOLAHIP_LIVE_H_

#include "molahip_clean.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MH_LIVE_API_VERSION 1
#define MH_LIVE_MAX_VIEWS 64

/* MH_LIVE_API_VERSION of the loaded library. */
MH_API uint32_t mh_live_api_version(void);
MH_API mh_status mh_views_put_scan(mh_views* views, uint64_t slot, const mh_scan* scan);
MH_API mh_status mh_views_vote_map(const mh_views* views, const mh_map* map, uint32_t n_nbr, const uint32_t* nbr_view,
                                   const double* nbr_T, uint32_t* votes_out, uint64_t capacity, int32_t mem);
MH_API mh_status mh_map_erase_points(mh_map* map, const uint8_t* drop, uint64_t n, int32_t mem);
MH_API mh_status mh_map_erase_seen_through(mh_map* map, const mh_views* views, uint32_t n_nbr, const uint32_t* nbr_view,
                                           const double* nbr_T, uint32_t min_through_votes, uint32_t agree_weight);
MH_API mh_status mh_map_erased_total(const mh_map* map, uint64_t* n);

#ifdef __cplusplus
}
#endif
#endif /* MOLAHIP_LIVE_H_ */
