// map_cleaning.cpp -- see mola_lidar_odometry_hip/MapCleaning.h.  Host logic only: the device is reached through the two calls of
// include/molahip_clean.h.
#include "mola_lidar_odometry_hip/MapCleaning.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <utility>

#include "config_block.h"

namespace mola_hip {

using namespace mp2p_icp_hip;

namespace {

struct Timer {  // adds the wall time of its scope to a report entry
  CleaningReport& r;
  const char* name;
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  Timer(CleaningReport& rep, const char* n) : r(rep), name(n) {}
  ~Timer() { r.seconds[name] += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }
};

bool frame_has_points(const molahip_host::KeyFrame& f) {
  if (!f.has_points) return false;
  for (const auto& l : f.layers)
    if (!l.x.empty()) return true;
  return false;
}

struct ViewsHandle {  // mh_views with a scope
  mh_views* h = nullptr;
  ~ViewsHandle() { mh_views_destroy(h); }
};

}  // namespace

// ================================================================== options
const std::vector<std::string>& cleaning_shared_keys() {
  static const std::vector<std::string> keys = {"n_rings", "n_sectors", "el_min_deg", "el_max_deg", "min_range", "max_range", "rel_margin",
                                                "origin_x", "origin_y", "origin_z", "win_rings", "win_sectors", "max_view_distance",
                                                "min_through_votes", "agree_weight"};
  return keys;
}

void read_cleaning_shared_keys(const Config& block_config, const std::string& block, MapCleaningOptions& o) {
  const ConfigBlock c(block_config, block);
  c.count("n_rings", o.n_rings); c.count("n_sectors", o.n_sectors);
  c.number("el_min_deg", o.el_min_deg); c.number("el_max_deg", o.el_max_deg);
  c.number("min_range", o.min_range); c.number("max_range", o.max_range); c.number("rel_margin", o.rel_margin);
  c.number("origin_x", o.origin[0]); c.number("origin_y", o.origin[1]); c.number("origin_z", o.origin[2]);
  c.count("win_rings", o.win_rings); c.count("win_sectors", o.win_sectors);
  c.number("max_view_distance", o.max_view_distance);
  c.count("min_through_votes", o.min_through_votes); c.count("agree_weight", o.agree_weight);
}

MapCleaningOptions MapCleaningOptions::FromConfig(const Config& cfg) {
  MapCleaningOptions o;
  if (cfg.has("map_cleaning") && !cfg["map_cleaning"].isNull()) {
    const ConfigBlock c(cfg["map_cleaning"], "map_cleaning");
    c.knownKeys({"max_views_per_frame"}, cleaning_shared_keys());
    read_cleaning_shared_keys(cfg["map_cleaning"], "map_cleaning", o);
    c.count("max_views_per_frame", o.max_views_per_frame);
  }
  o.validate();
  return o;
}

void MapCleaningOptions::validate() const { validateAs("map_cleaning"); }

void MapCleaningOptions::validateAs(const std::string& block) const {
  auto bad = [&](const std::string& key, const std::string& what) { bad_option(block, key, what); };
  if (n_rings < 1 || n_rings > MH_CLEAN_MAX_RINGS) bad("n_rings", "must be in 1.." + std::to_string(MH_CLEAN_MAX_RINGS));
  if (n_sectors < 8 || n_sectors > MH_CLEAN_MAX_SECTORS || n_sectors % 8)
    bad("n_sectors", "must be a multiple of 8 in 8.." + std::to_string(MH_CLEAN_MAX_SECTORS));
  if ((uint64_t)n_rings * n_sectors > MH_CLEAN_MAX_BINS) bad("n_sectors", "times n_rings must be <= " + std::to_string(MH_CLEAN_MAX_BINS));
  if (!(el_min_deg > -90.0 && el_min_deg < 90.0)) bad("el_min_deg", "must lie inside (-90, 90)");
  if (!(el_max_deg > el_min_deg && el_max_deg < 90.0)) bad("el_max_deg", "must lie inside (el_min_deg, 90)");
  if (!(min_range > 0.0) || !std::isfinite(min_range)) bad("min_range", "must be finite and > 0");
  if (!(max_range > min_range) || !std::isfinite(max_range)) bad("max_range", "must be finite and > min_range");
  if (!(rel_margin > 0.0) || !std::isfinite(rel_margin)) bad("rel_margin", "must be finite and > 0");
  static const char* const axes[] = {"origin_x", "origin_y", "origin_z"};
  for (int a = 0; a < 3; a++)
    if (!std::isfinite(origin[a])) bad(axes[a], "must be finite");
  if (win_rings > 2) bad("win_rings", "must be in 0..2");
  if (win_sectors > 2) bad("win_sectors", "must be in 0..2");
  if (!(max_view_distance >= 0.0) || !std::isfinite(max_view_distance)) bad("max_view_distance", "must be finite and >= 0");
  if (max_views_per_frame < 1) bad("max_views_per_frame", "must be an integer >= 1");
  if (min_through_votes < 1) bad("min_through_votes", "must be an integer >= 1");
}

mh_clean_params MapCleaningOptions::deviceParams() const {
  const double deg = 3.14159265358979323846 / 180.0;
  mh_clean_params p{};
  p.n_rings = n_rings; p.n_sectors = n_sectors;
  p.el_min = (float)(el_min_deg * deg); p.el_max = (float)(el_max_deg * deg);
  p.min_range = (float)min_range; p.max_range = (float)max_range;
  p.rel_margin = (float)rel_margin;
  for (int a = 0; a < 3; a++) p.origin[a] = (float)origin[a];
  p.win_rings = win_rings; p.win_sectors = win_sectors;
  return p;
}

// ================================================================== host rules
std::vector<std::vector<uint32_t>> cleaning_neighbours(const std::vector<double>& poses, const std::vector<uint8_t>& has_points,
                                                       const MapCleaningOptions& opt) {
  const size_t K = has_points.size();
  if (poses.size() != 12 * K) throw std::runtime_error("cleaning_neighbours: poses needs 12 values per frame");
  const double lim = opt.max_view_distance * opt.max_view_distance;
  std::vector<std::vector<uint32_t>> out(K);
  std::vector<std::pair<double, uint32_t>> cand;
  for (size_t i = 0; i < K; i++) {
    if (!has_points[i]) continue;
    cand.clear();
    const double* a = &poses[12 * i];
    for (size_t j = 0; j < K; j++) {
      if (j == i || !has_points[j]) continue;
      const double* b = &poses[12 * j];
      const double dx = b[3] - a[3], dy = b[7] - a[7], dz = b[11] - a[11];
      const double d2 = (dx * dx + dy * dy) + dz * dz;
      if (d2 <= lim) cand.emplace_back(d2, (uint32_t)j);
    }
    std::sort(cand.begin(), cand.end());  // (distance, then index: ties to the lower index)
    if (cand.size() > opt.max_views_per_frame) cand.resize(opt.max_views_per_frame);
    for (const auto& c : cand) out[i].push_back(c.second);
    std::sort(out[i].begin(), out[i].end());
  }
  return out;
}

void cleaning_relative_pose(const double Ti[12], const double Tj[12], double T[12]) {
  const double d[3] = {Ti[3] - Tj[3], Ti[7] - Tj[7], Ti[11] - Tj[11]};
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) T[4 * r + c] = (Tj[r] * Ti[c] + Tj[4 + r] * Ti[4 + c]) + Tj[8 + r] * Ti[8 + c];
    T[4 * r + 3] = (Tj[r] * d[0] + Tj[4 + r] * d[1]) + Tj[8 + r] * d[2];
  }
}

size_t cleaning_apply(molahip_host::KeyFrame& frame, const uint32_t* votes, const MapCleaningOptions& opt) {
  size_t at = 0, removed = 0;
  for (auto& l : frame.layers) {
    const size_t n = l.x.size();
    size_t w = 0;
    for (size_t k = 0; k < n; k++) {
      if (cleaning_removes(votes[at + k], opt)) continue;
      l.x[w] = l.x[k]; l.y[w] = l.y[k]; l.z[w] = l.z[k];
      w++;
    }
    removed += n - w;
    l.x.resize(w); l.y.resize(w); l.z.resize(w);
    at += n;
  }
  return removed;
}

// ================================================================== the whole thing
std::string CleaningReport::toJson() const {
  char buf[512];
  snprintf(buf, sizeof(buf),
           "{\"frames\": %zu, \"points_in\": %llu, \"points_removed\": %llu, \"pairs\": %llu, \"seconds\": {\"views\": %.6f, \"votes\": %.6f, "
           "\"removal\": %.6f}}",
           frames.size(), (unsigned long long)points_in, (unsigned long long)points_removed, (unsigned long long)pairs,
           seconds.count("views") ? seconds.at("views") : 0.0, seconds.count("votes") ? seconds.at("votes") : 0.0,
           seconds.count("removal") ? seconds.at("removal") : 0.0);
  return buf;
}

CleaningResult clean_keyframes(const molahip_host::KeyFrameSet& set, const MapCleaningOptions& opt, std::shared_ptr<DeviceContext> ctx) {
  opt.validate();
  for (const auto& t : set.maps)
    if (t.class_name == "CVoxelMap")
      throw std::runtime_error("clean_keyframes: target map '" + t.name + "' is a '" + t.class_name + "': an occupancy map is not built from "
                               "key-frames, so there is no session map to clean them for (HashedVoxelPointCloud, NDT and SparseTreesPointCloud are)");
  CleaningResult out;
  out.cleaned = set;
  CleaningReport& rep = out.report;
  const size_t K = set.frames.size();
  rep.frames.resize(K);
  std::vector<uint8_t> has(K, 0);
  std::vector<double> poses(12 * K);
  bool any = false;
  for (size_t k = 0; k < K; k++) {
    const auto& f = set.frames[k];
    for (int e = 0; e < 12; e++)
      if (!std::isfinite(f.pose[e])) throw std::runtime_error("clean_keyframes: non-finite pose");
    std::copy(f.pose, f.pose + 12, &poses[12 * k]);
    has[k] = frame_has_points(f) ? 1 : 0;
    any = any || has[k];
    if (f.has_points)
      for (const auto& l : f.layers) rep.frames[k].points_in += l.x.size();
    rep.points_in += rep.frames[k].points_in;
  }
  if (!any) return out;  // nothing to look at: unchanged, and no device is asked for
  const std::vector<std::vector<uint32_t>> nb = cleaning_neighbours(poses, has, opt);
  if (!ctx) ctx = DeviceContext::Default();
  const mh_clean_params params = opt.deviceParams();
  ViewsHandle views;
  check(mh_views_create(ctx->get(), &params, &views.h), "mh_views_create");

  // one frame's entries together: x | y | z of all its points, in entry order (an entry alone is used in place)
  std::vector<uint32_t> with;       // the frames with points; view k belongs to frame with[k]
  std::vector<uint32_t> view_of(K, 0);
  std::vector<std::vector<float>> joined(K);
  std::vector<mh_map_frame> frames;
  uint64_t total = 0;
  for (size_t k = 0; k < K; k++) {
    if (!has[k]) continue;
    const auto& f = set.frames[k];
    mh_map_frame m{};
    const size_t n = (size_t)rep.frames[k].points_in;
    if (f.layers.size() == 1) {
      m.x = f.layers[0].x.data(); m.y = f.layers[0].y.data(); m.z = f.layers[0].z.data();
    } else {
      std::vector<float>& j = joined[k];
      j.resize(3 * n);
      size_t at = 0;
      for (const auto& l : f.layers) {
        std::copy(l.x.begin(), l.x.end(), j.begin() + at);
        std::copy(l.y.begin(), l.y.end(), j.begin() + n + at);
        std::copy(l.z.begin(), l.z.end(), j.begin() + 2 * n + at);
        at += l.x.size();
      }
      m.x = j.data(); m.y = j.data() + n; m.z = j.data() + 2 * n;
    }
    m.n = n;
    std::copy(f.pose, f.pose + 12, m.T);
    view_of[k] = (uint32_t)with.size();
    with.push_back((uint32_t)k);
    frames.push_back(m);
    total += n;
  }
  {
    Timer t(rep, "views");
    check(mh_views_add_frames(views.h, frames.data(), frames.size(), MH_MEM_HOST, 0), "mh_views_add_frames");
  }
  std::vector<uint32_t> nbr_start(with.size() + 1, 0), nbr_view;
  std::vector<double> nbr_T;
  std::vector<uint32_t> votes(total);
  {
    Timer t(rep, "votes");
    for (size_t v = 0; v < with.size(); v++) {
      const uint32_t i = with[v];
      for (uint32_t j : nb[i]) {
        nbr_view.push_back(view_of[j]);
        nbr_T.resize(nbr_T.size() + 12);
        cleaning_relative_pose(&poses[12 * i], &poses[12 * j], &nbr_T[nbr_T.size() - 12]);
      }
      nbr_start[v + 1] = (uint32_t)nbr_view.size();
      rep.frames[i].neighbours = (uint32_t)nb[i].size();
    }
    rep.pairs = nbr_view.size();
    check(mh_views_vote_frames(views.h, frames.data(), frames.size(), nbr_start.data(), nbr_view.data(), nbr_T.data(), votes.data(), MH_MEM_HOST, 0),
          "mh_views_vote_frames");
  }
  {
    Timer t(rep, "removal");
    size_t at = 0;
    for (size_t v = 0; v < with.size(); v++) {
      const uint32_t i = with[v];
      rep.frames[i].points_removed = cleaning_apply(out.cleaned.frames[i], votes.data() + at, opt);
      rep.points_removed += rep.frames[i].points_removed;
      at += (size_t)rep.frames[i].points_in;
    }
  }
  return out;
}

CleaningReport clean_keyframes_file(const std::string& input_keyframe_file, const std::string& output_keyframe_file, const MapCleaningOptions& opt,
                                    std::shared_ptr<DeviceContext> ctx) {
  const CleaningResult r = clean_keyframes(molahip_host::read_keyframe_file(input_keyframe_file), opt, std::move(ctx));
  molahip_host::write_keyframe_file(output_keyframe_file, r.cleaned);
  return r.report;
}

}  // namespace mola_hip
