// molahip-lo-cli: stand-alone LiDAR odometry over a KITTI odometry sequence folder, no Python in the loop.
//
// The role mola-lidar-odometry-cli plays in the reference's evaluation scripts (eval/cli_kitti.sh:23-50, relative to
// /root/reference): one sequence in, one TUM trajectory out.  Everything numeric happens in mola_hip::LidarOdometry
// (device-resident filters, ICP, local map); this file only reads velodyne/*.bin (float32 x,y,z,intensity rows),
// times.txt, and announces the next scan so that its upload and first filter pass overlap with the current ICP loop.
//
//   molahip-lo-cli --pipeline pipelines/lidar3d-default-hip.yaml --seq-dir /data/kitti/sequences/00 --out 00.tum
//                  [--device 0 | --devices 0,1,..|all] [--no-prefetch] [--max-scans N] [--time-field BYTES] [--intensity-field BYTES] [--scan-log FILE]
// --devices: config 4 of BASELINE.json without Python -- the sequences are assigned to the listed GPUs by LPT (longest
// sequence first onto the least loaded device, what eval/cli_kitti.sh:9,23-36 leaves to GNU parallel's job slots), every
// device runs its share like a --seq-dir list on one GPU (a host thread per sequence, one AlignBatcher per device); the
// "gather" is the host-side join of the per-sequence TUM files and ONE summary line.  A device may be listed twice
// (two independent batchers on it: the multi-device code path on a single-GPU box).  --plan-only prints the assignment.
// --seq-dir also takes a MulRan sequence folder (eval/cli_mulran.sh:23-36, `--input-mulran-seq KAIST01` with
// MULRAN_BASE_DIR, apps/mola-lidar-odometry-cli.cpp:186-208): <dir>/sensor_data/Ouster/<stamp in ns>.bin (or <dir>/Ouster/),
// float32 x,y,z,intensity rows like KITTI's, the scan's time stamp is its file name.
// --intensity-field 12: the rows' fourth float is the intensity the filters of extras/lidar3d-intensity.yaml read (it also calls
// LidarOdometry::setIntensityInput(true)); without it the field is ignored.
// Several --seq-dir run together on the one GPU (what eval/cli_kitti.sh:23 does with GNU parallel -j3, as processes):
// a host thread per sequence, their alignments merged into lock-step batches (mp2p_icp_hip::AlignBatcher).
#include <algorithm>
#include <chrono>
#include <unistd.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <stdexcept>
#include <memory>
#include <map>
#include <string>
#include <thread>
#include <vector>

#include <dirent.h>

#include <sys/stat.h>

#include <atomic>
#include <condition_variable>
#include <mutex>

#include "mola_lidar_odometry_hip/LidarOdometry.h"
#include "mola_lidar_odometry_hip/LoopClosure.h"
#include "mola_lidar_odometry_hip/MapCleaning.h"
#include "mola_lidar_odometry_hip/OccupancyGrid.h"
#include "mola_lidar_odometry_hip/Traversability.h"
#include "mola_lidar_odometry_hip/NavCostmap.h"
#include "mola_lidar_odometry_hip/Replan.h"
#include "mola_lidar_odometry_hip/RoutePlan.h"
#include "mola_lidar_odometry_hip/SessionJoin.h"
#include "molahip.h"

namespace {

std::vector<std::string> list_bins(const std::string& dir) {
  std::vector<std::string> out;
  DIR* d = opendir(dir.c_str());
  if (!d) throw std::runtime_error("cannot open " + dir);
  while (dirent* e = readdir(d)) {
    const std::string n = e->d_name;
    if (n.size() > 4 && n.compare(n.size() - 4, 4, ".bin") == 0) out.push_back(dir + "/" + n);
  }
  closedir(d);
  std::sort(out.begin(), out.end());
  return out;
}

bool dir_exists(const std::string& d) {
  DIR* h = opendir(d.c_str());
  if (h) closedir(h);
  return h != nullptr;
}
// ".../1561000444390857630.bin" -> 1561000444.390857630 [s]
double stamp_of_name(const std::string& path) {
  const size_t slash = path.rfind('/');
  const std::string base = path.substr(slash == std::string::npos ? 0 : slash + 1);
  return 1e-9 * strtod(base.c_str(), nullptr);
}

std::vector<float> read_bin(const std::string& path) {
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) throw std::runtime_error("cannot read " + path);
  fseek(f, 0, SEEK_END);
  const long bytes = ftell(f);
  fseek(f, 0, SEEK_SET);
  if (bytes < 0 || bytes % 16 != 0) {
    fclose(f);
    throw std::runtime_error(path + ": not a sequence of float32 x,y,z,intensity rows");
  }
  std::vector<float> v((size_t)bytes / 4);
  const size_t got = v.empty() ? 0 : fread(v.data(), 4, v.size(), f);
  fclose(f);
  if (got != v.size()) throw std::runtime_error("short read on " + path);
  return v;
}

constexpr size_t kWarmScans = 5;

struct SequenceReport {
  std::string seq_dir, out;
  size_t scans = 0, good = 0, keyframes = 0, iterations = 0;
  std::shared_ptr<void> keep_alive;        // the sequence's driver object (device buffers and all), destroyed after the reports
  double seconds = 0, steady_seconds = 0;  // steady: without the first kWarmScans scans (context, code objects, first map)
  size_t steady_scans = 0;
  std::string error;
  std::map<std::string, double> profile;  // LidarOdometry::profile(): host seconds per stage, whole run
  int device = 0;
  double mean_icp_points = 0, mean_map_layer_points = 0, mean_raw_points = 0;
  uint64_t final_map_points = 0, max_map_points = 0, final_map_voxels = 0;
  std::vector<double> scan_seconds;  // --scan-log: registration time of every scan
  bool online_loop_closure = false;  // the pipeline's online_loop_closure: block is enabled ...
  size_t loops_closed = 0;           // ... and closed this many loops while driving
  bool lost_recovery = false;        // the pipeline's lost_recovery: block is enabled ...
  unsigned times_lost = 0, recovery_attempts = 0, times_recovered = 0;  // ... LidarOdometry::timesLost() and its like
  bool online_map_cleaning = false;   // the pipeline's online_map_cleaning: block is enabled ...
  uint64_t map_points_erased = 0;     // ... LidarOdometry::mapPointsErased()
  bool gyro_deskew = false;           // the pipeline's gyro_deskew: block is enabled ...
  uint64_t scans_gyro_deskewed = 0;   // ... LidarOdometry::scansGyroDeskewed()
};

struct RunOptions {
  long max_scans = -1;
  bool prefetch = true;
  long long time_field = -1;  // byte offset of a float32 per-point time stamp inside the 16-byte record, or -1
  long long intensity_field = -1;  // byte offset of the float32 intensity inside the record (KITTI / MulRan: 12), or -1
  std::string scan_log;       // CSV of per-scan registration times and layer / map sizes
  std::string save_local_map;  // --save-local-map: the local maps at the end of the sequence (FILE_<k> for several sequences)
  std::string output_simplemap;    // --output-simplemap: record key-frames (params.simplemap.generate) and save them at the end (FILE_<k> likewise)
  bool relocalize_in_keyframes = false;  // --relocalize-in-keyframes: LidarOdometry::relocalizeInKeyFrames() before the first scan
  std::string output_session_map;  // --output-session-map: ... and the maps of the whole drive built from them, as a local-map file (FILE_<k> likewise)
  std::string output_corrected_trajectory;  // --output-corrected-trajectory: LidarOdometry::correctedTrajectory() as a TUM file
  std::string gyro_file;  // --gyro-file: lines "t wx wy wz" on the clock of the scans' stamps, fed through LidarOdometry::onGyro (gyro_deskew:)
};

// what the replay leaves behind besides the trajectory: layer and map sizes (records()), optionally a per-scan CSV
void finish_report(const mola_hip::LidarOdometry& lo, const RunOptions& opt, SequenceReport& rep) {
  const auto& recs = lo.records();  // (resolves the map counters)
  double s_icp = 0, s_map = 0, s_raw = 0;
  size_t n_icp = 0;
  for (const auto& r : recs) {
    s_raw += (double)r.n_raw;
    if (r.icp_run) {
      s_icp += (double)r.n_for_icp;
      s_map += (double)r.n_for_map;
      n_icp++;
    }
    rep.max_map_points = std::max<uint64_t>(rep.max_map_points, r.n_map_points);
  }
  if (n_icp) rep.mean_icp_points = s_icp / (double)n_icp, rep.mean_map_layer_points = s_map / (double)n_icp;
  if (!recs.empty()) {
    rep.mean_raw_points = s_raw / (double)recs.size();
    rep.final_map_points = recs.back().n_map_points;
    rep.final_map_voxels = recs.back().n_map_voxels;
  }
  if (!opt.scan_log.empty()) {
    const std::string path = rep.out.size() > 4 && opt.scan_log == "auto" ? rep.out.substr(0, rep.out.size() - 4) + "_scans.csv" : opt.scan_log;
    FILE* f = fopen(path.c_str(), "w");
    if (f) {
      fprintf(f, "scan,seconds,n_raw,n_for_map,n_for_icp,n_map_points,icp_iterations,align_calls,goodness,sigma,map_updated,icp_good\n");
      for (size_t k = 0; k < recs.size(); k++)
        fprintf(f, "%zu,%.7f,%llu,%llu,%llu,%llu,%u,%u,%.4f,%.4f,%d,%d\n", k, k < rep.scan_seconds.size() ? rep.scan_seconds[k] : 0.0,
                (unsigned long long)recs[k].n_raw, (unsigned long long)recs[k].n_for_map, (unsigned long long)recs[k].n_for_icp,
                (unsigned long long)recs[k].n_map_points, recs[k].icp_iterations, recs[k].align_calls, recs[k].goodness, recs[k].sigma,
                (int)recs[k].map_updated, (int)recs[k].icp_good);
      fclose(f);
    }
  }
}

// files + stamps of a KITTI or MulRan sequence folder
void list_sequence(const std::string& seq_dir, long max_scans, std::vector<std::string>& files, std::vector<double>& stamps) {
  const std::string ouster = dir_exists(seq_dir + "/sensor_data/Ouster") ? seq_dir + "/sensor_data/Ouster"
                             : (dir_exists(seq_dir + "/Ouster") ? seq_dir + "/Ouster" : std::string());
  if (!dir_exists(seq_dir + "/velodyne") && !ouster.empty()) {
    // MulRan: one <time stamp in nanoseconds>.bin per sweep (numeric order = lexical order for equal-length names)
    files = list_bins(ouster);
    std::sort(files.begin(), files.end(), [](const std::string& a, const std::string& b) { return stamp_of_name(a) < stamp_of_name(b); });
    const double t0 = files.empty() ? 0.0 : stamp_of_name(files[0]);
    for (const auto& f : files) stamps.push_back(stamp_of_name(f) - t0);  // relative seconds (TUM output keeps sub-ms digits)
  } else {
    files = list_bins(seq_dir + "/velodyne");
    std::ifstream ts(seq_dir + "/times.txt");
    double t;
    while (ts >> t) stamps.push_back(t);
  }
  if (max_scans >= 0 && (size_t)max_scans < files.size()) files.resize((size_t)max_scans);
  while (stamps.size() < files.size()) stamps.push_back(0.1 * (double)stamps.size());  // 10 Hz when times.txt is absent
}

// cfg[key] = value for a scalar, the map entry made if absent
mp2p_icp_hip::Config& config_child(mp2p_icp_hip::Config& c, const std::string& key) {
  for (auto& kv : c.map)
    if (kv.first == key) return kv.second;
  c.kind = mp2p_icp_hip::Config::Kind::Map;
  c.map.emplace_back(key, mp2p_icp_hip::Config());
  return c.map.back().second;
}
void config_set(mp2p_icp_hip::Config& c, const std::string& key, const std::string& value) {
  mp2p_icp_hip::Config& n = config_child(c, key);
  n = mp2p_icp_hip::Config();
  n.kind = mp2p_icp_hip::Config::Kind::Scalar;
  n.scalar = value;
}

// one sequence, start to end; with a batcher its alignments join those of the other sequences of the process.  `suffix` ("" for a
// single sequence, "_<k>" for sequence k of several) goes behind every output name of --save-local-map, --output-simplemap and
// --output-session-map, so that no two sequences write one file.
void run_sequence(const std::string& pipeline, const std::string& seq_dir, const std::string& out, int device, const RunOptions& opt,
                  std::shared_ptr<mp2p_icp_hip::AlignBatcher> batcher, SequenceReport& rep, const std::string& suffix) {
  rep.seq_dir = seq_dir;
  rep.out = out;
  rep.device = device;
  const long max_scans = opt.max_scans;
  const bool prefetch = opt.prefetch;
  mp2p_icp_hip::AlignBatcher::Membership member(batcher);  // leave() however this sequence ends
  try {
    // (a page-locked read-ahead ring with asynchronous uploads was tried here: the eight copies and the filter batch then land
    // on the alignment's first iterations -- 8 sequences 4000 scans/s against 4700, one sequence 0.89 ms per scan against
    // 0.86 -- so the threads keep uploading from pageable memory.  Round 3 also had a mode with every sequence a ucontext
    // fiber of ONE host thread, --fibers: 2410-2650 scans/s for eight sequences against 4580-4920 with threads; removed.)
    std::vector<std::string> files;
    std::vector<double> stamps;
    list_sequence(seq_dir, max_scans, files, stamps);

    // MOLAHIP_STARTUP_LOG=1: where a sequence's first second goes (stderr; seconds since the process's first sequence started)
    static const bool startup_log = getenv("MOLAHIP_STARTUP_LOG") != nullptr;
    static const auto t_proc = std::chrono::steady_clock::now();
    auto stamp = [&](const char* what, size_t k = 0) {
      if (startup_log)
        fprintf(stderr, "[startup %s] %.4f s  %s %zu\n", out.c_str(), std::chrono::duration<double>(std::chrono::steady_clock::now() - t_proc).count(), what, k);
    };
    stamp("files listed");
    // (on the heap, handed to the report at the end: its tear-down -- a hipFree per buffer, each a device-wide wait -- is not part
    //  of the run; main() prints the reports first and then leaves without it)
    auto lo_owner = std::make_shared<mola_hip::LidarOdometry>(std::make_shared<mp2p_icp_hip::DeviceContext>(device));
    mola_hip::LidarOdometry& lo = *lo_owner;
    rep.keep_alive = lo_owner;
    stamp("device context");
    if (opt.intensity_field >= 0) lo.setIntensityInput(true);  // (before initialize(): the intensity filters need it)
    mp2p_icp_hip::Config cfg = mp2p_icp_hip::Config::FromYamlFile(pipeline);
    if (!opt.output_simplemap.empty() || !opt.output_session_map.empty()) {
      // params.simplemap.generate on, whatever the file says; saved explicitly below (the driver object outlives the report and is
      // never torn down, so its destructor writes nothing)
      mp2p_icp_hip::Config& sm = config_child(config_child(cfg, "params"), "simplemap");
      config_set(sm, "generate", "true");
      config_set(sm, "save_final_map_to_file", "");
    }
    lo.initialize(cfg);
    stamp("pipeline initialised");
    if (batcher) lo.setAlignBatcher(batcher);
    if (opt.relocalize_in_keyframes) lo.relocalizeInKeyFrames();  // served by the first scan that reaches registration
    // --gyro-file: before a scan the driver gets the samples up to the end of that scan's window (and a step beyond, for coverage)
    std::vector<mola_hip::GyroSample> gyro;
    size_t gyro_next = 0;
    if (!opt.gyro_file.empty()) gyro = mola_hip::read_gyro_file(opt.gyro_file);
    const mola_hip::GyroDeskewOptions& go = lo.gyroDeskewOptions();
    const double gyro_ahead = go.time_zero_offset + go.window[1] + 2.0 * go.max_gap;

    std::vector<float> cur, nxt;  // both stay alive while the driver may still read them
    if (!files.empty()) cur = read_bin(files[0]);
    for (size_t k = 0; k < files.size(); k++) {
      const bool has_next = k + 1 < files.size();
      if (has_next) nxt = read_bin(files[k + 1]);  // (file reading is not part of the registration time)
      for (; gyro_next < gyro.size() && gyro[gyro_next].t <= stamps[k] + gyro_ahead; gyro_next++) lo.onGyro(gyro[gyro_next].t, gyro[gyro_next].w);
      const auto t0 = std::chrono::steady_clock::now();
      if (has_next && prefetch) lo.prefetchInterleaved(nxt.data(), nxt.size() / 4, 16, 0, 4, 8, opt.time_field, nullptr, opt.intensity_field);
      const auto& rec = lo.onLidarInterleaved(stamps[k], cur.data(), cur.size() / 4, 16, 0, 4, 8, opt.time_field, nullptr, opt.intensity_field);
      const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      rep.seconds += dt;
      rep.scan_seconds.push_back(dt);
      if (k >= kWarmScans) {
        rep.steady_seconds += dt;
        rep.steady_scans++;
      }
      if (k < 8 || k + 1 == files.size()) stamp("scan done", k);
      if (k + 1 == kWarmScans) lo.resetProfile();  // the stage table is the steady state's (context, code objects, first map left out)
      rep.good += rec.icp_good ? 1 : 0;
      rep.keyframes += rec.map_updated ? 1 : 0;
      rep.iterations += rec.icp_iterations;
      rep.scans++;
      if (has_next) {
        // the announced buffer must keep its address until it has been registered: swap contents, not storage roles
        cur.swap(nxt);
      }
    }
    lo.saveTrajectoryTUM(out);
    if (!opt.output_corrected_trajectory.empty()) lo.saveCorrectedTrajectoryTUM(opt.output_corrected_trajectory + suffix);
    rep.online_loop_closure = mola_hip::OnlineLoopClosureOptions::FromConfig(cfg).enabled;
    if (lo.loopCloser()) rep.loops_closed = lo.loopCloser()->loops().size();
    rep.lost_recovery = lo.lostRecoveryOptions().enabled;
    rep.times_lost = lo.timesLost(), rep.recovery_attempts = lo.recoveryAttempts(), rep.times_recovered = lo.timesRecovered();
    rep.online_map_cleaning = lo.onlineMapCleaningOptions().enabled;
    if (rep.online_map_cleaning) rep.map_points_erased = lo.mapPointsErased();
    rep.gyro_deskew = go.enabled;
    rep.scans_gyro_deskewed = lo.scansGyroDeskewed();
    stamp("trajectory saved");
    if (!opt.save_local_map.empty()) lo.saveLocalMaps(opt.save_local_map + suffix);  // (what params.local_map_updates.load_existing_local_map of a later run reads)
    if (!opt.output_simplemap.empty()) lo.saveKeyFrames(opt.output_simplemap + suffix);
    if (!opt.output_session_map.empty())
      mola_hip::build_session_map_file(lo.keyFrames(), opt.output_session_map + suffix, std::make_shared<mp2p_icp_hip::DeviceContext>(device));
    rep.profile = lo.profile();
    finish_report(lo, opt, rep);
    stamp("report finished");
  } catch (const std::exception& e) {
    rep.error = e.what();
  }
}

// Longest-processing-time assignment of sequences (cost = number of scans) to device slots: the schedule DESIGN.md section 4
// prices config 4 with (11 KITTI sequences on 8 GPUs: makespan = sequence 02).  Returns slot index per sequence.
std::vector<size_t> lpt_assign(const std::vector<size_t>& scans, size_t n_slots, std::vector<size_t>* load_out = nullptr) {
  std::vector<size_t> order(scans.size()), slot(scans.size(), 0), load(n_slots, 0);
  for (size_t k = 0; k < order.size(); k++) order[k] = k;
  std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return scans[a] > scans[b]; });
  for (size_t k : order) {
    const size_t best = (size_t)(std::min_element(load.begin(), load.end()) - load.begin());  // first of the least loaded
    slot[k] = best;
    load[best] += scans[k];
  }
  if (load_out) *load_out = load;
  return slot;
}

std::vector<int> parse_devices(const std::string& arg) {
  std::vector<int> out;
  if (arg == "all") {
    int n = 0;
    if (mh_device_count(&n) != MH_OK || n <= 0) throw std::runtime_error("--devices all: no HIP device");
    for (int d = 0; d < n; d++) out.push_back(d);
    return out;
  }
  size_t pos = 0;
  while (pos <= arg.size()) {
    const size_t c = arg.find(',', pos);
    const std::string tok = arg.substr(pos, c == std::string::npos ? std::string::npos : c - pos);
    if (tok.empty() || tok.find_first_not_of("0123456789") != std::string::npos) throw std::runtime_error("--devices: expected a list like 0,1,2 or 'all'");
    out.push_back(atoi(tok.c_str()));
    if (c == std::string::npos) break;
    pos = c + 1;
  }
  return out;
}

}  // namespace

int main(int argc, char** argv) {
  std::string pipeline, out = "trajectory.tum";
  std::vector<std::string> seq_dirs;
  std::vector<int> devices;
  RunOptions opt;
  bool print_profile = false, plan_only = false;
  std::string build_from;  // --build-session-map
  std::string close_from, loop_report;  // --close-loops, --loop-report
  std::vector<std::string> join_files;  // --join-sessions A B
  std::vector<std::string> clean_files;  // --clean-keyframes IN OUT
  std::vector<std::string> grid_files;   // --build-occupancy-grid KEYFRAMES OUT_PREFIX
  std::vector<std::string> trav_files;   // --build-traversability KEYFRAMES OUT_PREFIX
  std::vector<std::string> cost_files;   // --build-costmap KEYFRAMES OUT_PREFIX
  std::vector<std::string> route_files;  // --plan-route COSTMAP_PREFIX OUT_PREFIX
  std::vector<std::string> replan_files;  // --replan-route KEYFRAMES EVENTS OUT_PREFIX
  const char* usage = "usage: molahip-lo-cli --pipeline FILE.yaml --seq-dir DIR [--seq-dir DIR ...] --out FILE.tum [--device N | --devices 0,1,..|all] "
                      "[--no-prefetch] [--max-scans N] [--profile] [--time-field BYTES] [--intensity-field BYTES] [--scan-log FILE|auto] [--plan-only]\n"
                      "                      [--save-local-map FILE] [--output-simplemap FILE] [--output-session-map FILE] [--relocalize-in-keyframes]\n"
                      "       molahip-lo-cli --build-session-map KEYFRAMES --save-local-map FILE [--device N]\n"
                      "       molahip-lo-cli --close-loops KEYFRAMES --pipeline FILE.yaml --output-simplemap FILE [--output-session-map FILE] [--loop-report FILE.json] [--device N]\n"
                      "       molahip-lo-cli --join-sessions KEYFRAMES_A KEYFRAMES_B --pipeline FILE.yaml --output-simplemap FILE [--output-session-map FILE] [--loop-report FILE.json] [--device N]\n"
                      "       molahip-lo-cli --clean-keyframes KEYFRAMES_IN KEYFRAMES_OUT [-c FILE.yaml] [--device N]\n"
                      "       molahip-lo-cli --build-occupancy-grid KEYFRAMES OUT_PREFIX [-c FILE.yaml] [--device N]\n"
                      "       molahip-lo-cli --build-traversability KEYFRAMES OUT_PREFIX [-c FILE.yaml] [--device N]\n"
                      "       molahip-lo-cli --build-costmap KEYFRAMES OUT_PREFIX [-c FILE.yaml] [--device N]\n"
                      "       molahip-lo-cli --plan-route COSTMAP_PREFIX OUT_PREFIX -c FILE.yaml [--device N]\n"
                      "       molahip-lo-cli --replan-route KEYFRAMES EVENTS OUT_PREFIX [-c FILE.yaml] [--device N]\n"
                      "  several --seq-dir: the sequences run together, one host thread each, the alignments of the sequences that share\n"
                      "  a GPU merged into lock-step batches; trajectories go to FILE_<k>.tum\n"
                      "  --save-local-map: the local maps at the end of the run (FILE_<k> for several sequences); a later run loads one through\n"
                      "  the pipeline's params.local_map_updates.load_existing_local_map (MOLA_LOAD_MM), and starts at initial_localization (MOLA_INITIAL_*)\n"
                      "  --output-simplemap: record the key-frames of the session (params.simplemap.generate) and save them to FILE at the end\n"
                      "  (FILE_<k> for several sequences)\n"
                      "  --output-session-map: ... and build the maps of the whole drive from them into FILE (FILE_<k> for several sequences),\n"
                      "  a local-map file like --save-local-map's\n"
                      "  --build-session-map: no sequence is run: the maps are built from the key-frame file KEYFRAMES into --save-local-map's FILE\n"
                      "  --close-loops: no sequence is run: revisits among the key-frames of KEYFRAMES are detected, verified on the device and closed\n"
                      "  (the pipeline's loop_closure: block); the key-frames with corrected poses go to --output-simplemap's FILE, the maps built from\n"
                      "  them to --output-session-map's, the report (pairs tried, qualities, optimiser cost, stage times) to --loop-report's\n"
                      "  --join-sessions: no sequence is run: the drive of KEYFRAMES_B is found in the one of KEYFRAMES_A (place recognition, links verified\n"
                      "  on the device; the pipeline's session_join: block) and its key-frames are put into A's frame; A's key-frames and then B's go to\n"
                      "  --output-simplemap's FILE, the maps built from them to --output-session-map's, the report to --loop-report's; when the sessions\n"
                      "  cannot be joined nothing is written and the exit status is 1\n"
                      "  --clean-keyframes: no sequence is run: points that other key-frames look straight through (moving objects) are taken out of\n"
                      "  the key-frames of KEYFRAMES_IN (the pipeline's map_cleaning: block; -c or --pipeline, optional) and the set goes to KEYFRAMES_OUT;\n"
                      "  run it after --close-loops / --join-sessions and before --build-session-map\n"
                      "  --build-occupancy-grid: no sequence is run: every key-frame of KEYFRAMES is ray-traced from its pose into an occupancy map and a\n"
                      "  height band of it is projected to a 2-D grid (the pipeline's occupancy_grid: block; -c or --pipeline, optional), written as\n"
                      "  OUT_PREFIX.pgm and OUT_PREFIX.yaml for a map server; a key-frame file of any plan is taken\n"
                      "  --build-traversability: no sequence is run: the points of every key-frame of KEYFRAMES are binned into a 2.5-D elevation map (the\n"
                      "  lowest height per cell), obstacles are marked over that ground, and slope and step give every cell a cost (the pipeline's\n"
                      "  traversability: block; -c or --pipeline, optional); written as OUT_PREFIX.pgm + OUT_PREFIX.yaml (lethal / free / unknown, for a\n"
                      "  map server), OUT_PREFIX_cost.pgm (the cost bytes) and OUT_PREFIX_height.f32 (the ground height); run it after --close-loops\n"
                      "  and --clean-keyframes\n"
                      "  --build-costmap: no sequence is run: the source map of KEYFRAMES is built (the pipeline's costmap: source, traversability by default,\n"
                      "  with that map's own block), obstacles are inflated by the vehicle's radius with an exact distance transform, and the cells the\n"
                      "  vehicle can reach from its key-frames are flooded (the pipeline's costmap: block; -c or --pipeline, optional); written as\n"
                      "  OUT_PREFIX.pgm + OUT_PREFIX.yaml (for a map server), OUT_PREFIX_cost.pgm and OUT_PREFIX_reach.pgm\n"
                      "  --plan-route: no sequence is run: the costmap written by --build-costmap under COSTMAP_PREFIX is read, the cost-to-go field to\n"
                      "  the goal is computed and the route from the start traced down it (the pipeline's route: block with start_x, start_y, goal_x and\n"
                      "  goal_y in metres; -c or --pipeline); written as OUT_PREFIX_route.txt (x y per cell) and OUT_PREFIX_route.pgm\n"
                      "  --replan-route: no sequence is run: the costmap of KEYFRAMES is built as by --build-costmap and the cost-to-go field to the goal\n"
                      "  (the route: block's goal_x and goal_y, or goal_keyframe) is computed once; then the lines of the text file EVENTS are run in\n"
                      "  order: 'block X0 Y0 X1 Y1' makes a rectangle [m] of the base map lethal, 'clear X0 Y0 X1 Y1' makes it free -- the costmap is\n"
                      "  inflated again and the field is repaired round the change, not recomputed -- and 'at X Y' traces the route from that point,\n"
                      "  written as OUT_PREFIX_route_K.txt and OUT_PREFIX_route_K.pgm for the K-th 'at' line (from 0); one summary line per event\n"
                      "  --relocalize-in-keyframes: the vehicle is found in a saved session without a prior pose: place recognition over the\n"
                      "  key-frames of MOLA_LOAD_SM, then a pose search in the map of MOLA_LOAD_MM (run with MOLA_MAPPING_ENABLED=false);\n"
                      "  one sequence per device only\n"
                      "  --devices: the sequences are spread over the listed GPUs (longest first onto the least loaded device)\n";
  // (shown after it when the run asks for the gyro de-skew: the pipeline's gyro_deskew: block, or the option itself)
  const char* usage_gyro = "  --gyro-file FILE: gyroscope samples, text lines 't wx wy wz' ([s] on the clock of the scans' stamps, [rad/s]; '#' starts a\n"
                           "  comment), for the pipeline's gyro_deskew: block: every scan is de-skewed with the rotation measured during its sweep; one\n"
                           "  sequence only\n";
  auto gyro_enabled = [&]() {
    if (pipeline.empty()) return false;
    try {
      return mola_hip::GyroDeskewOptions::FromConfig(mp2p_icp_hip::Config::FromYamlFile(pipeline)).enabled;
    } catch (const std::exception&) {
      return false;  // (the run itself reports what is wrong with the file)
    }
  };
  // (shown after it when the run asks for online loop closure: the pipeline's online_loop_closure: block, or the option itself)
  const char* usage_online = "  --output-corrected-trajectory: with the pipeline's online_loop_closure: block enabled loops are closed while driving; the\n"
                             "  trajectory as the closures correct it goes to FILE (TUM), --out keeps what was estimated at the time; one sequence only\n";
  auto online_enabled = [&]() {
    if (pipeline.empty()) return false;
    try {
      return mola_hip::OnlineLoopClosureOptions::FromConfig(mp2p_icp_hip::Config::FromYamlFile(pipeline)).enabled;
    } catch (const std::exception&) {
      return false;  // (the run itself reports what is wrong with the file)
    }
  };
  for (int i = 1; i < argc; i++) {
    const std::string a = argv[i];
    auto val = [&](const char* name) -> std::string {
      if (i + 1 >= argc) throw std::runtime_error(std::string("missing value for ") + name);
      return argv[++i];
    };
    try {
      if (a == "--pipeline" || a == "-c") pipeline = val("--pipeline");
      else if (a == "--seq-dir") seq_dirs.push_back(val("--seq-dir"));
      else if (a == "--out") out = val("--out");
      else if (a == "--device") devices = {atoi(val("--device").c_str())};
      else if (a == "--devices") devices = parse_devices(val("--devices"));
      else if (a == "--max-scans") opt.max_scans = atol(val("--max-scans").c_str());
      else if (a == "--time-field") opt.time_field = atoll(val("--time-field").c_str());
      else if (a == "--intensity-field") opt.intensity_field = atoll(val("--intensity-field").c_str());
      else if (a == "--scan-log") opt.scan_log = val("--scan-log");
      else if (a == "--save-local-map") opt.save_local_map = val("--save-local-map");
      else if (a == "--output-simplemap") opt.output_simplemap = val("--output-simplemap");
      else if (a == "--output-session-map") opt.output_session_map = val("--output-session-map");
      else if (a == "--output-corrected-trajectory") opt.output_corrected_trajectory = val("--output-corrected-trajectory");
      else if (a == "--gyro-file") opt.gyro_file = val("--gyro-file");
      else if (a == "--build-session-map") build_from = val("--build-session-map");
      else if (a == "--close-loops") close_from = val("--close-loops");
      else if (a == "--loop-report") loop_report = val("--loop-report");
      else if (a == "--join-sessions") {
        join_files.push_back(val("--join-sessions"));
        join_files.push_back(val("--join-sessions"));
      }
      else if (a == "--clean-keyframes") {
        clean_files.push_back(val("--clean-keyframes"));
        clean_files.push_back(val("--clean-keyframes"));
      }
      else if (a == "--build-occupancy-grid") {
        grid_files.push_back(val("--build-occupancy-grid"));
        grid_files.push_back(val("--build-occupancy-grid"));
      }
      else if (a == "--build-traversability") {
        trav_files.push_back(val("--build-traversability"));
        trav_files.push_back(val("--build-traversability"));
      }
      else if (a == "--build-costmap") {
        cost_files.push_back(val("--build-costmap"));
        cost_files.push_back(val("--build-costmap"));
      }
      else if (a == "--plan-route") {
        route_files.push_back(val("--plan-route"));
        route_files.push_back(val("--plan-route"));
      }
      else if (a == "--replan-route") {
        for (int k = 0; k < 3; k++) replan_files.push_back(val("--replan-route"));
      }
      else if (a == "--relocalize-in-keyframes") opt.relocalize_in_keyframes = true;
      else if (a == "--no-prefetch") opt.prefetch = false;
      else if (a == "--profile") print_profile = true;
      else if (a == "--plan-only") plan_only = true;
      else throw std::runtime_error("unknown argument " + a);
    } catch (const std::exception& e) {
      fprintf(stderr, "%s\n%s", e.what(), usage);
      return 2;
    }
  }
  if (!replan_files.empty()) {  // routes that follow a costmap whose base changes, from a recorded drive's key-frames, no sequence
    if (replan_files.size() != 3 || !seq_dirs.empty() || !build_from.empty() || !close_from.empty() || !join_files.empty() || !clean_files.empty() ||
        !grid_files.empty() || !trav_files.empty() || !cost_files.empty() || !route_files.empty() || devices.size() > 1) {
      fprintf(stderr, "--replan-route takes one key-frame file, one events file and one output prefix, once, and takes no sequence and one device\n%s", usage);
      return 2;
    }
    try {
      const mp2p_icp_hip::Config cfg = pipeline.empty() ? mp2p_icp_hip::Config::FromYamlText("") : mp2p_icp_hip::Config::FromYamlFile(pipeline);
      (void)mola_hip::route_price_table(mola_hip::RouteOptions::FromConfig(cfg));  // (bad blocks and a bad events file are refused before the
      (void)mola_hip::NavCostmapOptions::FromConfig(cfg);                          // key-frames are read and a device is asked for)
      const std::vector<mola_hip::ReplanEvent> events = mola_hip::read_replan_events(replan_files[1]);
      const molahip_host::KeyFrameSet set = molahip_host::read_keyframe_file(replan_files[0]);
      auto ctx = std::make_shared<mp2p_icp_hip::DeviceContext>(devices.empty() ? 0 : devices[0]);
      const mola_hip::ReplanRun run = mola_hip::replan_route_from_keyframes(set, cfg, events, ctx);
      mola_hip::write_replan_routes(run, replan_files[2]);
      for (size_t k = 0; k < run.events.size(); k++) printf("%s\n", mola_hip::replan_event_summary(run, k).c_str());
      printf("{\"keyframe_file\": \"%s\", \"events_file\": \"%s\", \"prefix\": \"%s\", \"events\": %zu, \"routes\": %zu, \"rects_outside\": %llu}\n",
             replan_files[0].c_str(), replan_files[1].c_str(), replan_files[2].c_str(), run.events.size(), run.routes.size(), (unsigned long long)run.rects_outside);
    } catch (const std::exception& e) {
      fprintf(stderr, "molahip-lo-cli: %s\n", e.what());
      return 1;
    }
    return 0;
  }
  if (!route_files.empty()) {  // a route over a costmap read back from files, no sequence
    if (route_files.size() != 2 || !seq_dirs.empty() || !build_from.empty() || !close_from.empty() || !join_files.empty() || !clean_files.empty() ||
        !grid_files.empty() || !trav_files.empty() || !cost_files.empty() || devices.size() > 1 || pipeline.empty()) {
      fprintf(stderr, "--plan-route takes one costmap prefix to read and one output prefix, once, with a pipeline file, and takes no sequence and one device\n%s", usage);
      return 2;
    }
    try {
      const mola_hip::RouteOptions ropt = mola_hip::RouteOptions::FromConfig(mp2p_icp_hip::Config::FromYamlFile(pipeline));
      (void)mola_hip::route_price_table(ropt);  // (a bad block is refused before the files are read)
      const mola_hip::NavCostmap c = mola_hip::read_costmap(route_files[0]);  // (missing files are refused before a device is asked for)
      auto ctx = std::make_shared<mp2p_icp_hip::DeviceContext>(devices.empty() ? 0 : devices[0]);
      const mola_hip::RoutePlan r = mola_hip::plan_route(c, ropt, ctx);
      mola_hip::write_route(r, c, route_files[1]);
      printf("{\"costmap\": \"%s\", \"route\": \"%s\", \"status\": \"%s\", \"cells\": %llu, \"length_m\": %.6f, \"cost_to_go\": %u, \"max_cost\": %u, "
             "\"min_clearance_m\": %.6f, \"sweeps\": %u, \"tile_runs\": %llu, \"cells_with_field\": %llu, \"seconds_field\": %.6f, \"seconds_trace\": %.6f}\n",
             route_files[0].c_str(), route_files[1].c_str(), r.status.c_str(), (unsigned long long)(r.cells.size() / 2), r.length_m, r.cost_to_go, r.max_cost,
             r.min_clearance_m, r.sweeps, (unsigned long long)r.tile_runs, (unsigned long long)r.cells_with_field, r.seconds_field, r.seconds_trace);
    } catch (const std::exception& e) {
      fprintf(stderr, "molahip-lo-cli: %s\n", e.what());
      return 1;
    }
    return 0;
  }
  if (!cost_files.empty()) {  // an inflated costmap with the reachable region from a recorded drive's key-frames, no sequence
    if (cost_files.size() != 2 || !seq_dirs.empty() || !build_from.empty() || !close_from.empty() || !join_files.empty() || !clean_files.empty() ||
        !grid_files.empty() || !trav_files.empty() || devices.size() > 1) {
      fprintf(stderr, "--build-costmap takes one key-frame file to read and one output prefix, once, and takes no sequence and one device\n%s", usage);
      return 2;
    }
    try {
      const mp2p_icp_hip::Config cfg = pipeline.empty() ? mp2p_icp_hip::Config::FromYamlText("") : mp2p_icp_hip::Config::FromYamlFile(pipeline);
      (void)mola_hip::NavCostmapOptions::FromConfig(cfg);  // (a bad block is refused before the file is read)
      const molahip_host::KeyFrameSet set = molahip_host::read_keyframe_file(cost_files[0]);  // (a missing file is refused before a device is asked for)
      auto ctx = std::make_shared<mp2p_icp_hip::DeviceContext>(devices.empty() ? 0 : devices[0]);
      const mola_hip::NavCostmap c = mola_hip::build_costmap_from_keyframes(set, cfg, ctx);
      mola_hip::write_costmap(c, cost_files[1]);
      printf("{\"keyframe_file\": \"%s\", \"costmap\": \"%s\", \"keyframes\": %llu, \"grid_x0\": %d, \"grid_y0\": %d, \"grid_nx\": %u, \"grid_ny\": %u, "
             "\"max_cells\": %u, \"cells_lethal\": %llu, \"cells_inscribed\": %llu, \"cells_inflated\": %llu, \"cells_free\": %llu, "
             "\"cells_unknown\": %llu, \"cells_reached\": %llu, \"cells_unreachable_free\": %llu, \"keyframes_blocked\": %llu, "
             "\"trajectory_min_clearance_m\": %.6f, \"seeds_blocked\": %llu, \"seeds_outside\": %llu, \"sweeps\": %u, "
             "\"seconds_source\": %.6f, \"seconds_inflate\": %.6f, \"seconds_reach\": %.6f}\n",
             cost_files[0].c_str(), cost_files[1].c_str(), (unsigned long long)c.keyframe_cost.size(), c.x0, c.y0, c.nx, c.ny, c.max_cells,
             (unsigned long long)c.cells_lethal, (unsigned long long)c.cells_inscribed, (unsigned long long)c.cells_inflated,
             (unsigned long long)c.cells_free, (unsigned long long)c.cells_unknown, (unsigned long long)c.cells_reached,
             (unsigned long long)c.cells_unreachable_free, (unsigned long long)c.keyframes_blocked, c.trajectory_min_clearance_m,
             (unsigned long long)c.seeds_blocked, (unsigned long long)c.seeds_outside, c.sweeps, c.seconds_source, c.seconds_inflate, c.seconds_reach);
    } catch (const std::exception& e) {
      fprintf(stderr, "molahip-lo-cli: %s\n", e.what());
      return 1;
    }
    return 0;
  }
  if (!trav_files.empty()) {  // an elevation map with a traversability cost from a recorded drive's key-frames, no sequence
    if (trav_files.size() != 2 || !seq_dirs.empty() || !build_from.empty() || !close_from.empty() || !join_files.empty() || !clean_files.empty() ||
        !grid_files.empty()) {
      fprintf(stderr, "--build-traversability takes one key-frame file to read and one output prefix, once, and takes no sequence\n%s", usage);
      return 2;
    }
    try {
      const mola_hip::TraversabilityOptions topt =
          mola_hip::TraversabilityOptions::FromConfig(pipeline.empty() ? mp2p_icp_hip::Config::FromYamlText("") : mp2p_icp_hip::Config::FromYamlFile(pipeline));
      const molahip_host::KeyFrameSet set = molahip_host::read_keyframe_file(trav_files[0]);  // (a missing file is refused before a device is asked for)
      auto ctx = std::make_shared<mp2p_icp_hip::DeviceContext>(devices.empty() ? 0 : devices[0]);
      const mola_hip::TraversabilityMap t = mola_hip::build_traversability_map(set, topt, ctx);
      mola_hip::write_traversability_map(t, trav_files[1]);
      printf("{\"keyframe_file\": \"%s\", \"traversability\": \"%s\", \"frames\": %llu, \"points\": %llu, \"points_counted\": %llu, "
             "\"points_left_out\": %llu, \"grid_x0\": %d, \"grid_y0\": %d, \"grid_nx\": %u, \"grid_ny\": %u, \"cells_lethal\": %llu, "
             "\"cells_free\": %llu, \"cells_unknown\": %llu, \"seconds_bounds\": %.6f, \"seconds_add\": %.6f, \"seconds_mark\": %.6f, "
             "\"seconds_relief\": %.6f}\n",
             trav_files[0].c_str(), trav_files[1].c_str(), (unsigned long long)t.frames, (unsigned long long)t.points,
             (unsigned long long)t.points_counted, (unsigned long long)t.points_left_out, t.x0, t.y0, t.nx, t.ny, (unsigned long long)t.cells_lethal,
             (unsigned long long)t.cells_free, (unsigned long long)t.cells_unknown, t.seconds_bounds, t.seconds_add, t.seconds_mark, t.seconds_relief);
    } catch (const std::exception& e) {
      fprintf(stderr, "molahip-lo-cli: %s\n", e.what());
      return 1;
    }
    return 0;
  }
  if (!grid_files.empty()) {  // a navigation occupancy grid from a recorded drive's key-frames, no sequence
    if (grid_files.size() != 2 || !seq_dirs.empty() || !build_from.empty() || !close_from.empty() || !join_files.empty() || !clean_files.empty()) {
      fprintf(stderr, "--build-occupancy-grid takes one key-frame file to read and one output prefix, once, and takes no sequence\n%s", usage);
      return 2;
    }
    try {
      const mola_hip::OccupancyGridOptions gopt =
          mola_hip::OccupancyGridOptions::FromConfig(pipeline.empty() ? mp2p_icp_hip::Config::FromYamlText("") : mp2p_icp_hip::Config::FromYamlFile(pipeline));
      const molahip_host::KeyFrameSet set = molahip_host::read_keyframe_file(grid_files[0]);  // (a missing file is refused before a device is asked for)
      auto ctx = std::make_shared<mp2p_icp_hip::DeviceContext>(devices.empty() ? 0 : devices[0]);
      const mola_hip::OccupancyGrid g = mola_hip::build_occupancy_grid(set, gopt, ctx);
      mola_hip::write_occupancy_grid(g, grid_files[1]);
      printf("{\"keyframe_file\": \"%s\", \"occupancy_grid\": \"%s\", \"frames\": %llu, \"points\": %llu, \"map_cells\": %llu, \"grid_x0\": %d, "
             "\"grid_y0\": %d, \"grid_nx\": %u, \"grid_ny\": %u, \"cells_occupied\": %llu, \"cells_free\": %llu, \"cells_unknown\": %llu, "
             "\"seconds_insert\": %.6f, \"seconds_project\": %.6f}\n",
             grid_files[0].c_str(), grid_files[1].c_str(), (unsigned long long)g.frames, (unsigned long long)g.points, (unsigned long long)g.map_cells,
             g.x0, g.y0, g.nx, g.ny, (unsigned long long)g.cells_occupied, (unsigned long long)g.cells_free, (unsigned long long)g.cells_unknown,
             g.seconds_insert, g.seconds_project);
    } catch (const std::exception& e) {
      fprintf(stderr, "molahip-lo-cli: %s\n", e.what());
      return 1;
    }
    return 0;
  }
  if (!clean_files.empty()) {  // moving objects taken out of a recorded drive's key-frames, no sequence
    if (clean_files.size() != 2 || !seq_dirs.empty() || !build_from.empty() || !close_from.empty() || !join_files.empty()) {
      fprintf(stderr, "--clean-keyframes takes one key-frame file to read and one to write, once, and takes no sequence\n%s", usage);
      return 2;
    }
    try {
      const mola_hip::MapCleaningOptions copt =
          mola_hip::MapCleaningOptions::FromConfig(pipeline.empty() ? mp2p_icp_hip::Config::FromYamlText("") : mp2p_icp_hip::Config::FromYamlFile(pipeline));
      auto ctx = std::make_shared<mp2p_icp_hip::DeviceContext>(devices.empty() ? 0 : devices[0]);
      const mola_hip::CleaningReport r = mola_hip::clean_keyframes_file(clean_files[0], clean_files[1], copt, ctx);
      printf("{\"keyframe_file\": \"%s\", \"output_simplemap\": \"%s\", \"cleaning\": %s}\n", clean_files[0].c_str(), clean_files[1].c_str(),
             r.toJson().c_str());
    } catch (const std::exception& e) {
      fprintf(stderr, "molahip-lo-cli: %s\n", e.what());
      return 1;
    }
    return 0;
  }
  if (!join_files.empty()) {  // two recorded drives put into one frame, no sequence
    if (join_files.size() != 2 || pipeline.empty() || opt.output_simplemap.empty() || !seq_dirs.empty() || !build_from.empty() || !close_from.empty()) {
      fprintf(stderr, "--join-sessions takes two key-frame files once, needs --pipeline FILE and --output-simplemap FILE and takes no sequence\n%s", usage);
      return 2;
    }
    try {
      auto ctx = std::make_shared<mp2p_icp_hip::DeviceContext>(devices.empty() ? 0 : devices[0]);
      const mola_hip::SessionJoinResult r = mola_hip::join_sessions(molahip_host::read_keyframe_file(join_files[0]), molahip_host::read_keyframe_file(join_files[1]),
                                                                    mp2p_icp_hip::Config::FromYamlFile(pipeline), ctx);
      const std::string json = r.report.toJson();
      if (!loop_report.empty()) {
        FILE* f = fopen(loop_report.c_str(), "w");
        if (!f) throw std::runtime_error("cannot write " + loop_report);
        fputs(json.c_str(), f);
        fclose(f);
      } else {
        fputs(json.c_str(), stdout);
      }
      if (r.is_joined) {
        molahip_host::write_keyframe_file(opt.output_simplemap, r.joined);
        if (!opt.output_session_map.empty()) mola_hip::build_session_map_file(r.joined, opt.output_session_map, ctx);
      }
      printf("{\"keyframe_files\": [\"%s\", \"%s\"], \"frames\": %zu, \"pairs_tried\": %zu, \"links_accepted\": %u, \"joined\": %s, \"cost_before\": %.9g, "
             "\"cost_after\": %.9g, \"optimizer_iterations\": %u, \"output_simplemap\": \"%s\"}\n",
             join_files[0].c_str(), join_files[1].c_str(), r.joined.frames.size(), r.report.pairs.size(), r.report.links_accepted, r.is_joined ? "true" : "false",
             r.report.cost_before, r.report.cost_after, r.report.optimizer_iterations, r.is_joined ? opt.output_simplemap.c_str() : "");
      if (!r.is_joined) {
        fprintf(stderr, "molahip-lo-cli: the sessions were not joined: %u accepted links (the pipeline's session_join: min_links decides); nothing written\n",
                r.report.links_accepted);
        return 1;
      }
    } catch (const std::exception& e) {
      fprintf(stderr, "molahip-lo-cli: %s\n", e.what());
      return 1;
    }
    return 0;
  }
  if (!close_from.empty()) {  // the loops of a recorded drive closed, no sequence
    if (pipeline.empty() || opt.output_simplemap.empty() || !seq_dirs.empty() || !build_from.empty()) {
      fprintf(stderr, "--close-loops needs --pipeline FILE and --output-simplemap FILE and takes no sequence\n%s", usage);
      return 2;
    }
    try {
      auto ctx = std::make_shared<mp2p_icp_hip::DeviceContext>(devices.empty() ? 0 : devices[0]);
      const mola_hip::LoopClosureResult r =
          mola_hip::close_loops(molahip_host::read_keyframe_file(close_from), mp2p_icp_hip::Config::FromYamlFile(pipeline), ctx);
      molahip_host::write_keyframe_file(opt.output_simplemap, r.corrected);
      if (!opt.output_session_map.empty()) mola_hip::build_session_map_file(r.corrected, opt.output_session_map, ctx);
      const std::string json = r.report.toJson();
      if (!loop_report.empty()) {
        FILE* f = fopen(loop_report.c_str(), "w");
        if (!f) throw std::runtime_error("cannot write " + loop_report);
        fputs(json.c_str(), f);
        fclose(f);
      }
      size_t accepted = 0;
      for (const auto& p : r.report.pairs) accepted += p.accepted ? 1 : 0;
      printf("{\"keyframe_file\": \"%s\", \"frames\": %zu, \"pairs_tried\": %zu, \"loops_closed\": %zu, \"cost_before\": %.9g, \"cost_after\": %.9g, "
             "\"optimizer_iterations\": %u, \"output_simplemap\": \"%s\"}\n",
             close_from.c_str(), r.corrected.frames.size(), r.report.pairs.size(), accepted, r.report.cost_before, r.report.cost_after,
             r.report.optimizer_iterations, opt.output_simplemap.c_str());
    } catch (const std::exception& e) {
      fprintf(stderr, "molahip-lo-cli: %s\n", e.what());
      return 1;
    }
    return 0;
  }
  if (!build_from.empty()) {  // the maps of a recorded drive, no sequence
    if (opt.save_local_map.empty() || !seq_dirs.empty()) {
      fprintf(stderr, "--build-session-map needs --save-local-map FILE and takes no sequence\n%s", usage);
      return 2;
    }
    try {
      const molahip_host::KeyFrameSet set = molahip_host::read_keyframe_file(build_from);
      const auto maps = mola_hip::build_session_maps(set, std::make_shared<mp2p_icp_hip::DeviceContext>(devices.empty() ? 0 : devices[0]));
      molahip_host::write_local_map_file(opt.save_local_map, maps);
      size_t with_points = 0;
      for (const auto& f : set.frames) with_points += f.has_points ? 1 : 0;
      printf("{\"keyframe_file\": \"%s\", \"frames\": %zu, \"keyframes\": %zu, \"local_map_file\": \"%s\", \"maps\": [", build_from.c_str(),
             set.frames.size(), with_points, opt.save_local_map.c_str());
      for (size_t k = 0; k < maps.size(); k++)
        printf("%s{\"name\": \"%s\", \"points\": %zu, \"offered\": %llu}", k ? ", " : "", maps[k].name.c_str(), maps[k].x.size(),
               (unsigned long long)maps[k].n_offered);
      printf("]}\n");
    } catch (const std::exception& e) {
      fprintf(stderr, "molahip-lo-cli: %s\n", e.what());
      return 1;
    }
    return 0;
  }
  if (pipeline.empty() || seq_dirs.empty()) {
    fprintf(stderr, "%s%s%s", usage, !opt.output_corrected_trajectory.empty() || online_enabled() ? usage_online : "",
            !opt.gyro_file.empty() || gyro_enabled() ? usage_gyro : "");
    return 2;
  }
  if (devices.empty()) devices = {0};
  const size_t N = seq_dirs.size(), D = devices.size();
  if (N > 1 || D > 1) {
    bool cleaning = false;
    try {
      cleaning = mola_hip::OnlineMapCleaningOptions::FromConfig(mp2p_icp_hip::Config::FromYamlFile(pipeline)).enabled;
    } catch (const std::exception&) {  // (the run itself reports what is wrong with the file)
    }
    if (cleaning) {
      fprintf(stderr, "molahip-lo-cli: the pipeline's online_map_cleaning: block is enabled: one sequence on one device only (several sequences of a "
                      "process align through an AlignBatcher, whose protocol has no place for map updates queued between its rounds)\n");
      return 2;
    }
  }
  {
    // gyro_deskew: and --gyro-file: one sequence on one device; the file is read (and refused by line) before any device work
    const bool gyro_on = gyro_enabled();
    if ((N > 1 || D > 1) && (gyro_on || !opt.gyro_file.empty())) {
      fprintf(stderr, "molahip-lo-cli: %s: one sequence on one device only (one gyro stream belongs to one drive, and several sequences of a "
                      "process align through an AlignBatcher, which has no slot for a motion table per member)\n",
              gyro_on ? "the pipeline's gyro_deskew: block is enabled" : "--gyro-file");
      return 2;
    }
    if (!opt.gyro_file.empty()) {
      if (!gyro_on) {
        fprintf(stderr, "molahip-lo-cli: --gyro-file needs the pipeline's gyro_deskew: block with enabled: true (the samples would be ignored)\n");
        return 2;
      }
      try {
        (void)mola_hip::read_gyro_file(opt.gyro_file);
      } catch (const std::exception& e) {
        fprintf(stderr, "molahip-lo-cli: --gyro-file: %s\n", e.what());
        return 2;
      }
    }
  }
  if ((N > 1 || D > 1) && online_enabled()) {
    fprintf(stderr, "molahip-lo-cli: the pipeline's online_loop_closure: block is enabled: one sequence on one device only (several sequences of a "
                    "process align through an AlignBatcher, whose batch protocol has no slot for the extra alignments that verify a loop)\n");
    return 2;
  }
  // which sequence runs where: scan counts are known from the folders (no GPU needed for the plan)
  std::vector<size_t> n_scans(N, 0), slot(N, 0), load(D, 0);
  try {
    for (size_t k = 0; k < N; k++) {
      std::vector<std::string> files;
      std::vector<double> stamps;
      list_sequence(seq_dirs[k], opt.max_scans, files, stamps);
      n_scans[k] = files.size();
    }
  } catch (const std::exception& e) {
    fprintf(stderr, "molahip-lo-cli: %s\n", e.what());
    return 1;
  }
  slot = lpt_assign(n_scans, D, &load);
  const std::string stem = out.size() > 4 && out.compare(out.size() - 4, 4, ".tum") == 0 ? out.substr(0, out.size() - 4) : out;
  if (plan_only) {
    size_t total = 0, makespan = 0;
    for (size_t k = 0; k < N; k++) total += n_scans[k];
    for (size_t d = 0; d < D; d++) makespan = std::max(makespan, load[d]);
    printf("{\"plan\": [");
    for (size_t k = 0; k < N; k++)
      printf("%s{\"sequence_dir\": \"%s\", \"scans\": %zu, \"slot\": %zu, \"device\": %d}", k ? ", " : "", seq_dirs[k].c_str(), n_scans[k], slot[k], devices[slot[k]]);
    printf("], \"device_load_scans\": [");
    for (size_t d = 0; d < D; d++) printf("%s%zu", d ? ", " : "", load[d]);
    printf("], \"total_scans\": %zu, \"makespan_scans\": %zu, \"speedup_bound\": %.4f}\n", total, makespan, makespan ? (double)total / (double)makespan : 0.0);
    return 0;
  }
  std::vector<SequenceReport> reps(N);
  std::vector<std::shared_ptr<mp2p_icp_hip::AlignBatcher>> batchers(D);
  std::vector<size_t> per_slot(D, 0);
  for (size_t k = 0; k < N; k++) per_slot[slot[k]]++;
  if (opt.relocalize_in_keyframes && N > 1)
    for (size_t d = 0; d < D; d++)
      if (per_slot[d] > 1) {  // (those sequences share an AlignBatcher, which has no slot for a relocalization's extra alignments)
        fprintf(stderr, "molahip-lo-cli: --relocalize-in-keyframes takes one sequence per device; device %d would run %zu\n", devices[d], per_slot[d]);
        return 2;
      }
  const auto t0 = std::chrono::steady_clock::now();
  {  // the HIP runtime is initialised ONCE, here, inside the measured wall clock -- eight threads doing it at the same moment took
     // 0.20 s to their first context against 0.12 s (MOLAHIP_STARTUP_LOG=1)
    int32_t n_dev = 0;
    (void)mh_device_count(&n_dev);
  }
  if (N == 1) {
    run_sequence(pipeline, seq_dirs[0], out, devices[0], opt, nullptr, reps[0], std::string());
  } else {
    // a batcher per device slot: the sequences of a slot advance together, the slots independently of each other
    for (size_t d = 0; d < D; d++)
      if (per_slot[d] > 1) batchers[d] = std::make_shared<mp2p_icp_hip::AlignBatcher>(per_slot[d]);
    std::vector<std::thread> th;
    for (size_t k = 0; k < N; k++)
      th.emplace_back(run_sequence, pipeline, seq_dirs[k], stem + "_" + std::to_string(k) + ".tum", devices[slot[k]], std::cref(opt),
                      batchers[slot[k]], std::ref(reps[k]), "_" + std::to_string(k));
    for (auto& t : th) t.join();
  }
  const double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  int rc = 0;
  size_t total = 0;
  for (const auto& r : reps) {
    if (!r.error.empty()) {
      fprintf(stderr, "molahip-lo-cli: %s: %s\n", r.seq_dir.c_str(), r.error.c_str());
      rc = 1;
    }
    total += r.scans;
    printf("{\"sequence_dir\": \"%s\", \"device\": %d, \"scans\": %zu, \"good\": %zu, \"keyframes\": %zu, \"icp_iterations\": %zu, "
           "\"seconds\": %.6f, \"scans_per_s\": %.3f, \"steady_scans_per_s\": %.3f, \"mean_raw_points\": %.1f, \"mean_icp_points\": %.1f, "
           "\"mean_map_layer_points\": %.1f, \"final_map_points\": %llu, \"max_map_points\": %llu, \"final_map_voxels\": %llu, \"tum\": \"%s\"",
           r.seq_dir.c_str(), r.device, r.scans, r.good, r.keyframes, r.iterations, r.seconds, r.seconds > 0 ? r.scans / r.seconds : 0.0,
           r.steady_seconds > 0 ? r.steady_scans / r.steady_seconds : 0.0, r.mean_raw_points, r.mean_icp_points, r.mean_map_layer_points,
           (unsigned long long)r.final_map_points, (unsigned long long)r.max_map_points, (unsigned long long)r.final_map_voxels, r.out.c_str());
    if (r.online_loop_closure) printf(", \"loops_closed\": %zu", r.loops_closed);
    if (r.lost_recovery)  // (the pipeline's lost_recovery: block; absent or disabled, the line is as before)
      printf(", \"times_lost\": %u, \"recovery_attempts\": %u, \"times_recovered\": %u", r.times_lost, r.recovery_attempts, r.times_recovered);
    if (r.online_map_cleaning)  // (the pipeline's online_map_cleaning: block; absent or disabled, the line is as before)
      printf(", \"map_points_erased\": %llu", (unsigned long long)r.map_points_erased);
    if (r.gyro_deskew)  // (the pipeline's gyro_deskew: block; absent or disabled, the line is as before)
      printf(", \"scans_gyro_deskewed\": %llu", (unsigned long long)r.scans_gyro_deskewed);
    printf("}\n");
    if (print_profile && r.scans) {  // host milliseconds per scan and stage (LidarOdometry::profile()), steady state
      const double ns = (double)(r.steady_scans ? r.steady_scans : r.scans);
      printf("{\"profile_ms_per_scan\": {");
      bool first = true;
      for (const auto& kv : r.profile) {
        // "icp.*" and "prefetch_*" entries are COUNTS per scan (align calls, host polls, iterations), the rest milliseconds
        const bool count = kv.first.compare(0, 4, "icp.") == 0 || kv.first.compare(0, 9, "prefetch_") == 0;
        printf("%s\"%s\": %.4f", first ? "" : ", ", kv.first.c_str(), (count ? 1.0 : 1e3) * kv.second / ns);
        first = false;
      }
      printf("}}\n");
    }
  }
  {
    // the sequences of a device advance together (one batch per round), so a device's slowest thread is its registration
    // time; the job's is the slowest device's (the makespan): steady rate = all steady scans / that
    size_t steady = 0, n_batches = 0, n_jobs = 0, f_batches = 0, f_jobs = 0, f_timeouts = 0;
    double slowest = 0, assembling = 0, running = 0;
    std::vector<double> dev_seconds(D, 0), dev_steady_seconds(D, 0);
    std::vector<size_t> dev_scans(D, 0), dev_steady(D, 0);
    for (size_t k = 0; k < N; k++) {
      const auto& r = reps[k];
      steady += r.steady_scans;
      slowest = std::max(slowest, r.steady_seconds);
      dev_scans[slot[k]] += r.scans;
      dev_steady[slot[k]] += r.steady_scans;
      dev_seconds[slot[k]] = std::max(dev_seconds[slot[k]], r.seconds);
      dev_steady_seconds[slot[k]] = std::max(dev_steady_seconds[slot[k]], r.steady_seconds);
    }
    for (const auto& b : batchers)
      if (b) {
        n_batches += b->batches(), n_jobs += b->jobs(), f_batches += b->filterBatches(), f_jobs += b->filterJobs(), f_timeouts += b->filterTimeouts();
        assembling += b->secondsAssembling(), running += b->secondsRunning();
      }
    const double nb = n_batches ? (double)n_batches : 1.0;
    uint64_t loops_started = 0, loops_abandoned = 0;
    mh_debug_loop_stats(&loops_started, &loops_abandoned);
    printf("{\"sequences\": %zu, \"devices\": %zu, \"scans\": %zu, \"wall_seconds\": %.6f, \"scans_per_s\": %.3f, \"steady_scans_per_s\": %.3f, "
           "\"batches\": %zu, \"jobs_per_batch\": %.2f, \"ms_per_batch_assembling\": %.4f, \"ms_per_batch_running\": %.4f, "
           "\"filter_batches\": %zu, \"filter_jobs\": %zu, \"filter_timeouts\": %zu, \"one_launch_loops\": %llu, "
           "\"one_launch_loops_abandoned\": %llu, \"per_device\": [",
           N, D, total, wall, wall > 0 ? total / wall : 0.0, slowest > 0 ? steady / slowest : 0.0, n_batches, n_jobs / nb,
           1e3 * assembling / nb, 1e3 * running / nb, f_batches, f_jobs, f_timeouts, (unsigned long long)loops_started,
           (unsigned long long)loops_abandoned);
    for (size_t d = 0; d < D; d++)
      printf("%s{\"slot\": %zu, \"device\": %d, \"sequences\": %zu, \"scans\": %zu, \"registration_seconds\": %.6f, \"scans_per_s\": %.3f, "
             "\"steady_scans_per_s\": %.3f}",
             d ? ", " : "", d, devices[d], per_slot[d], dev_scans[d], dev_seconds[d], dev_seconds[d] > 0 ? dev_scans[d] / dev_seconds[d] : 0.0,
             dev_steady_seconds[d] > 0 ? dev_steady[d] / dev_steady_seconds[d] : 0.0);
    printf("]");
    size_t loops_closed = 0;
    bool online = false;
    for (const auto& r : reps) online = online || r.online_loop_closure, loops_closed += r.loops_closed;
    if (online) printf(", \"loops_closed\": %zu", loops_closed);  // (the pipeline's online_loop_closure: block; absent, the line is as before)
    unsigned times_lost = 0, recovery_attempts = 0, times_recovered = 0;
    bool recovery = false;
    for (const auto& r : reps)
      recovery = recovery || r.lost_recovery, times_lost += r.times_lost, recovery_attempts += r.recovery_attempts, times_recovered += r.times_recovered;
    if (recovery) printf(", \"times_lost\": %u, \"recovery_attempts\": %u, \"times_recovered\": %u", times_lost, recovery_attempts, times_recovered);
    uint64_t map_points_erased = 0;
    bool cleaning = false;
    for (const auto& r : reps) cleaning = cleaning || r.online_map_cleaning, map_points_erased += r.map_points_erased;
    if (cleaning) printf(", \"map_points_erased\": %llu", (unsigned long long)map_points_erased);
    uint64_t scans_gyro_deskewed = 0;
    bool gyro = false;
    for (const auto& r : reps) gyro = gyro || r.gyro_deskew, scans_gyro_deskewed += r.scans_gyro_deskewed;
    if (gyro) printf(", \"scans_gyro_deskewed\": %llu", (unsigned long long)scans_gyro_deskewed);
    printf("}\n");
  }
  // Everything asked for is on disk and on stdout.  The drivers' destructors would now hipFree a few hundred buffers one by one,
  // each call a wait for the whole device: 0.2 s for eight sequences -- the operating system takes the memory back faster
  // (MOLAHIP_FULL_TEARDOWN=1 runs them, e.g. under a leak checker).
  fflush(stdout);
  fflush(stderr);
  // (exit(), not _exit(): handlers registered with atexit -- a profiler's finalisation, the runtime's own -- still run; the
  //  drivers, held by `reps` on this frame, are not destroyed by it)
  if (getenv("MOLAHIP_FULL_TEARDOWN") == nullptr) exit(rc);
  return rc;
}
