// mh_nav_internal.h -- the body of the costmap handle, shared by mh_nav.hip and mh_plan.hip (mh_plan_set_cost_from_nav copies its
// cost plane device to device).
#pragma once
#include "../../include/molahip_nav.h"
#include "mh_internal.h"

struct mh_nav {
  mh_ctx* ctx = nullptr;
  uint32_t nx = 0, ny = 0;
  size_t n_cells = 0;
  mh::DevBuf bytes;   // base | cost | reach, n_cells bytes each (256-byte aligned sections)
  mh::DevBuf words;   // d2 | g, n_cells uint16 each
  mh::DevBuf table;   // the inflation table of the last inflate
  mh::DevBuf seeds;   // the seeds of the last reach
  mh::DevBuf ctr;     // uint32 [4]: seeds blocked, seeds placed, cells reached, the sweep's flag
  mh::PinnedBuf h_ctr;
  size_t stride = 0;  // of a byte plane
  mh_nav_info info{};
  uint8_t* base() const { return bytes.as<uint8_t>(); }
  uint8_t* cost() const { return bytes.as<uint8_t>() + stride; }
  uint8_t* reach() const { return bytes.as<uint8_t>() + 2 * stride; }
  uint16_t* d2() const { return words.as<uint16_t>(); }
  uint16_t* g() const { return words.as<uint16_t>() + stride; }
};
