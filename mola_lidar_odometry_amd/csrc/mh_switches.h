// mh_switches.h -- the run-time switches of the library, read in ONE place.  Every public entry point that depends
// on them takes one snapshot at its start (read_switches) and passes it down: they are read live, the test suite toggles them
// between calls.
#pragma once
#include <limits.h>
#include <stdint.h>
#include <stdlib.h>

#include <algorithm>

#ifndef MH_LOOPW_DEFAULT
#define MH_LOOPW_DEFAULT "batch"
#endif

namespace mh {

// one field per switch, named after it (MH_NO_STREAM -> no_stream); MH_MATCH / MH_LOOPW keep their value's first letter
struct Switches {
  char match = 0, loopw = 0;
  bool no_loopw = false, no_loop16 = false, no_loop16_batch = false;
  long loop16_wait_us = 2000;  // admission wait before the chain is taken
  int loop16_cus = -1;         // admission limit in CUs (-1: the device's count)
  uint32_t solo_max_callers = 4, lockstep_groups = 1;
  bool no_step_chain = false, no_fuse16 = false, no_stream = false, no_graph = false, no_lockstep = false;
  bool no_prev_bound = false, no_qidx = false, map_full_sort = false, map_no_collect = false;
  bool no_off32 = false;  // the plan / scan matcher's 64-bit-offset instantiation whatever the sizes (flat_off32, mh_k_launch.h)
  long keep_lds = LONG_MAX;  // (clamped to 1..kKeepLds where it is used)
  bool loop16_test_abandon = false, debug_verify_batch = false;
  bool nav_no_early_stop = false;  // mh_nav_inflate's row pass walks every dx (MH_NAV_NO_EARLY_STOP=1: for measuring what the stop saves; same bits)
  bool plan_all_tiles = false;  // mh_plan_field runs every tile in every sweep (MH_PLAN_ALL_TILES=1: for measuring what the active-tile flags save; same bits)
  bool replan_full = false;  // an update of molahip_replan.h patches the bytes and computes the whole field from nothing (MH_REPLAN_FULL=1: for measuring what the repair saves, and as a twin in tests; same bits)
};

inline Switches read_switches() {
  auto on = [](const char* name) { return getenv(name) != nullptr; };
  Switches sw;
  const char* e;
  if ((e = getenv("MH_MATCH"))) sw.match = e[0];
  sw.loopw = (e = getenv("MH_LOOPW")) ? e[0] : MH_LOOPW_DEFAULT[0];
  sw.no_loopw = on("MH_NO_LOOPW");
  sw.no_loop16 = on("MH_NO_LOOP16");
  sw.no_loop16_batch = on("MH_NO_LOOP16_BATCH");
  if ((e = getenv("MH_LOOP16_WAIT_US"))) sw.loop16_wait_us = atol(e);
  if ((e = getenv("MH_LOOP16_CUS"))) sw.loop16_cus = std::max(0, atoi(e));
  if ((e = getenv("MH_SOLO_MAX_CALLERS"))) sw.solo_max_callers = (uint32_t)std::max(1, atoi(e));
  if ((e = getenv("MH_LOCKSTEP_GROUPS")) && atoi(e)) sw.lockstep_groups = (uint32_t)atoi(e);
  sw.no_step_chain = on("MH_NO_STEP_CHAIN");
  sw.no_fuse16 = on("MH_NO_FUSE16");
  sw.no_stream = on("MH_NO_STREAM");
  sw.no_graph = on("MH_NO_GRAPH");
  sw.no_lockstep = on("MH_NO_LOCKSTEP");
  sw.no_prev_bound = on("MH_NO_PREV_BOUND");
  sw.no_qidx = on("MH_NO_QIDX");
  sw.no_off32 = on("MH_NO_OFF32");
  sw.map_full_sort = on("MH_MAP_FULL_SORT");
  sw.map_no_collect = on("MH_MAP_NO_COLLECT");
  if ((e = getenv("MH_KEEP_LDS"))) sw.keep_lds = atol(e);
  sw.loop16_test_abandon = on("MH_LOOP16_TEST_ABANDON");
  sw.debug_verify_batch = on("MH_DEBUG_VERIFY_BATCH");
  sw.nav_no_early_stop = on("MH_NAV_NO_EARLY_STOP");
  sw.plan_all_tiles = on("MH_PLAN_ALL_TILES");
  sw.replan_full = on("MH_REPLAN_FULL");
  return sw;
}

}  // namespace mh
