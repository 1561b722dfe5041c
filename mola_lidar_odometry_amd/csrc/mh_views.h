// mh_views.h -- the store of views behind the opaque handle mh_views, shared by mh_clean.hip (key-frames: add_frames,
// vote_frames) and mh_live.hip (a live map: put_scan, vote_map).
#pragma once
#include "mh_internal.h"
#include "mh_see_through.h"

struct mh_views {
  mh_ctx* ctx = nullptr;
  mh_clean_params params{};
  mh::CleanTables tab{};
  mh::DevBuf img;          // size * A*S words, img[k][ring * S + sector]
  uint64_t size = 0;
  mh::PinnedBuf h_frames;  // page-locked mirror of one pass's upload
  mh::DevBuf nbr;          // vote_frames: the neighbour list of the call (start | view | T)
};

namespace mh {

// room for n_total views; what is stored moves along when the block grows (the outgrown block stays valid behind it)
inline mh_status views_reserve(mh_views* v, uint64_t n_total) {
  const size_t AS = (size_t)v->tab.A * v->tab.S * sizeof(uint32_t);
  void* old = v->img.p;
  MH_TRY(v->img.reserve(n_total * AS));
  if (old && old != v->img.p && v->size) MH_HIP(hipMemcpyAsync(v->img.p, old, v->size * AS, hipMemcpyDeviceToDevice, v->ctx->stream));
  return MH_OK;
}

}  // namespace mh
